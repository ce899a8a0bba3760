"""ctypes loader for the HIP library (kmcuda_amd/libKMCUDA.so).

There is NO fallback: if the gfx950 library is missing or does not load, importing the step
API raises.  Build it with `python -c "import __graft_entry__ as g; g.build()"` or
`make -C kmcuda_amd/csrc`.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# KMCUDA_AMD_LIB: another build of the same library (A/B runs of kernel variants, scripts/coarse_variants.sh)
LIB_PATH = os.environ.get("KMCUDA_AMD_LIB") or os.path.join(_HERE, "libKMCUDA.so")

u32, i32, f32 = ctypes.c_uint32, ctypes.c_int32, ctypes.c_float
vp = ctypes.c_void_p

_lib = None

# every symbol include/kmcuda.h and include/kmcuda_amd.h declare
EXPORTS = [
    "kmeans_cuda", "knn_cuda", "kmamd_kmeans_weighted", "kmamd_set_weights",
    "kmamd_engine_create", "kmamd_engine_destroy", "kmamd_engine_stream", "kmamd_engine_sync",
    "kmamd_lloyd_assign", "kmamd_lloyd_assign_exact", "kmamd_set_half_rows", "kmamd_set_row_cache", "kmamd_profile_read_coarse", "kmamd_set_filter", "kmamd_counters_read", "kmamd_counters_reset", "kmamd_yy_hint_stats",
    "kmamd_move_deltas", "kmamd_apply_delta", "kmamd_transpose", "kmamd_afkmc2_draws", "kmamd_reduce_len", "kmamd_reduce_fill",
    "kmamd_reduce_apply", "kmamd_reduce_apply_stop", "kmamd_reduce_apply_prepare", "kmamd_stop_report", "kmamd_stop_clear", "kmamd_centroids_written", "kmamd_set_carry", "kmamd_carry_stats", "kmamd_carry_pair_stats", "kmamd_duo_rows", "kmamd_carry_policy_sim", "kmamd_set_update_mode", "kmamd_last_run_stats", "kmamd_last_run_collective", "kmamd_adjust_exact", "kmamd_yy_configure", "kmamd_yy_init", "kmamd_yy_drifts", "kmamd_yy_filters",
    "kmamd_knn_index_create", "kmamd_knn_index_query", "kmamd_knn_index_query_probe", "kmamd_knn_index_destroy",
    "kmamd_knn_index_radius_count", "kmamd_knn_index_radius_fill", "kmamd_knn_index_add", "kmamd_knn_index_info",
    "kmamd_knn_index_remove", "kmamd_knn_index_radii",
    "kmamd_knn_index_query_allow", "kmamd_knn_index_query_probe_allow", "kmamd_knn_index_radii_allow",
    "kmamd_knn_index_radius_count_allow", "kmamd_knn_index_radius_fill_allow",
    "kmamd_knn_index_query_capped", "kmamd_knn_index_query_probe_capped",
    "kmamd_kmeans_assign", "kmamd_assigned_distances",
    "kmamd_kmeans_assign_top", "kmamd_assign_top_stats",
    "kmamd_kmeans_seed_parallel",
    "kmamd_minibatch_create", "kmamd_minibatch_step", "kmamd_minibatch_fit", "kmamd_minibatch_read",
    "kmamd_minibatch_destroy",
    "kmamd_copy_to_device", "kmamd_profile_reset", "kmamd_profile_read", "kmamd_profile_enable", "kmamd_filter_kind", "kmamd_build_arch",
]


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "kmcuda_amd: %s is missing -- the HIP library has not been built "
            "(run `make -C kmcuda_amd/csrc`); there is no CPU fallback." % LIB_PATH)
    L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    L.kmeans_cuda.restype = i32
    L.kmeans_cuda.argtypes = [i32, vp, f32, f32, i32, u32, ctypes.c_uint16, u32, u32, u32, i32, i32, i32,
                              vp, vp, vp, vp]
    # kmeans_cuda's arguments + the per-row sample weights (float32; host or device pointer like `samples`)
    L.kmamd_kmeans_weighted.restype = i32
    L.kmamd_kmeans_weighted.argtypes = [i32, vp, f32, f32, i32, u32, ctypes.c_uint16, u32, u32, u32, i32, i32, i32,
                                        vp, vp, vp, vp, vp]
    L.kmamd_set_weights.restype = i32
    L.kmamd_set_weights.argtypes = [vp, vp]
    L.knn_cuda.restype = i32
    L.knn_cuda.argtypes = [ctypes.c_uint16, i32, u32, ctypes.c_uint16, u32, u32, i32, i32, i32, vp, vp, vp, vp]
    L.kmamd_engine_create.restype = i32
    L.kmamd_engine_create.argtypes = [ctypes.POINTER(vp), i32, u32, u32, u32, i32, i32, vp]
    L.kmamd_engine_destroy.restype = None
    L.kmamd_engine_destroy.argtypes = [vp]
    L.kmamd_engine_stream.restype = vp
    L.kmamd_engine_stream.argtypes = [vp]
    L.kmamd_engine_sync.restype = i32
    L.kmamd_engine_sync.argtypes = [vp]
    for name in ("kmamd_lloyd_assign", "kmamd_lloyd_assign_exact"):
        fn = getattr(L, name)
        fn.restype = i32
        fn.argtypes = [vp, vp, vp, vp, vp]
    L.kmamd_set_filter.restype = i32
    L.kmamd_set_filter.argtypes = [vp, i32]
    L.kmamd_set_half_rows.restype = i32
    L.kmamd_set_half_rows.argtypes = [vp, vp]
    L.kmamd_set_row_cache.restype = i32
    L.kmamd_set_row_cache.argtypes = [vp, i32]
    L.kmamd_counters_read.restype = i32
    L.kmamd_counters_read.argtypes = [vp, ctypes.POINTER(u32)]
    L.kmamd_counters_reset.restype = i32
    L.kmamd_counters_reset.argtypes = [vp, i32]
    L.kmamd_yy_hint_stats.restype = i32
    L.kmamd_yy_hint_stats.argtypes = [vp, vp]
    L.kmamd_move_deltas.restype = i32
    L.kmamd_move_deltas.argtypes = [vp, vp, vp, vp, vp, vp]
    L.kmamd_apply_delta.restype = i32
    L.kmamd_apply_delta.argtypes = [vp, vp, vp, vp, vp]
    L.kmamd_reduce_len.restype = ctypes.c_size_t
    L.kmamd_reduce_len.argtypes = [vp]
    L.kmamd_reduce_fill.restype = i32
    L.kmamd_reduce_fill.argtypes = [vp, vp, vp, vp, vp]
    L.kmamd_reduce_apply.restype = i32
    L.kmamd_reduce_apply.argtypes = [vp, vp, vp, vp]
    L.kmamd_reduce_apply_stop.restype = i32
    L.kmamd_reduce_apply_stop.argtypes = [vp, vp, vp, vp, f32, u32]
    L.kmamd_reduce_apply_prepare.restype = i32
    L.kmamd_reduce_apply_prepare.argtypes = [vp, vp, vp, vp, f32, u32]
    L.kmamd_stop_report.restype = i32
    L.kmamd_stop_report.argtypes = [vp, u32, ctypes.POINTER(u32)]
    L.kmamd_stop_clear.restype = i32
    L.kmamd_stop_clear.argtypes = [vp]
    L.kmamd_centroids_written.restype = i32
    L.kmamd_centroids_written.argtypes = [vp]
    L.kmamd_set_carry.restype = i32
    L.kmamd_set_carry.argtypes = [vp, i32]
    L.kmamd_carry_stats.restype = i32
    L.kmamd_carry_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
    L.kmamd_carry_pair_stats.restype = i32
    L.kmamd_carry_pair_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_uint64)]
    L.kmamd_duo_rows.restype = i32
    L.kmamd_duo_rows.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    L.kmamd_carry_policy_sim.restype = i32
    L.kmamd_carry_policy_sim.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_float, ctypes.POINTER(ctypes.c_uint32),
                                         ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)]
    L.kmamd_set_update_mode.restype = i32
    L.kmamd_set_update_mode.argtypes = [vp, i32]
    L.kmamd_last_run_stats.restype = i32
    L.kmamd_last_run_stats.argtypes = [ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_double),
                                       ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.kmamd_last_run_collective.restype = i32
    L.kmamd_last_run_collective.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32)]
    L.kmamd_afkmc2_draws.restype = i32
    L.kmamd_afkmc2_draws.argtypes = [vp, ctypes.c_uint64, ctypes.c_uint64, u32, u32, vp]
    L.kmamd_transpose.restype = i32
    L.kmamd_transpose.argtypes = [vp, vp, u32, u32, vp]
    L.kmamd_adjust_exact.restype = i32
    L.kmamd_adjust_exact.argtypes = [vp, vp, vp, vp, vp, vp]
    L.kmamd_yy_init.restype = i32
    L.kmamd_yy_configure.restype = i32
    L.kmamd_yy_configure.argtypes = [vp, u32, vp]
    L.kmamd_yy_init.argtypes = [vp, vp, vp, vp, vp]
    L.kmamd_yy_drifts.restype = i32
    L.kmamd_yy_drifts.argtypes = [vp, vp, vp, vp]
    L.kmamd_yy_filters.restype = i32
    L.kmamd_yy_filters.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.kmamd_profile_reset.restype = i32
    L.kmamd_profile_reset.argtypes = [vp]
    L.kmamd_filter_kind.restype = i32
    L.kmamd_filter_kind.argtypes = [vp, ctypes.POINTER(ctypes.c_uint32)]
    L.kmamd_profile_enable.restype = i32
    L.kmamd_profile_enable.argtypes = [vp, i32]
    L.kmamd_profile_read_coarse.restype = i32
    L.kmamd_profile_read_coarse.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.kmamd_profile_read.restype = i32
    L.kmamd_profile_read.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32),
                                     ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
    L.kmamd_knn_index_create.restype = i32
    L.kmamd_knn_index_create.argtypes = [ctypes.POINTER(vp), i32, i32, i32, u32, u32, u32, vp, vp, vp, i32, i32]
    L.kmamd_knn_index_query.restype = i32
    L.kmamd_knn_index_query.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, i32]
    L.kmamd_knn_index_query_probe.restype = i32
    L.kmamd_knn_index_query_probe.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, vp, i32]
    L.kmamd_knn_index_radius_count.restype = i32
    L.kmamd_knn_index_radius_count.argtypes = [vp, f32, u32, vp, vp, vp, vp, i32]
    L.kmamd_knn_index_radius_fill.restype = i32
    L.kmamd_knn_index_radius_fill.argtypes = [vp, f32, u32, vp, vp, vp, vp, vp, i32]
    L.kmamd_knn_index_add.restype = i32
    L.kmamd_knn_index_add.argtypes = [vp, u32, vp, vp, vp, ctypes.POINTER(u32), i32]
    L.kmamd_knn_index_info.restype = i32
    L.kmamd_knn_index_info.argtypes = [vp, ctypes.POINTER(u32), ctypes.POINTER(u32), ctypes.POINTER(ctypes.c_int)]
    L.kmamd_knn_index_remove.restype = i32
    L.kmamd_knn_index_remove.argtypes = [vp, u32, vp, ctypes.POINTER(u32), i32]
    L.kmamd_knn_index_radii.restype = i32
    L.kmamd_knn_index_radii.argtypes = [vp, vp]
    L.kmamd_knn_index_query_allow.restype = i32
    L.kmamd_knn_index_query_allow.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp, i32, vp]
    L.kmamd_knn_index_query_probe_allow.restype = i32
    L.kmamd_knn_index_query_probe_allow.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp, vp, i32, vp]
    L.kmamd_knn_index_radii_allow.restype = i32
    L.kmamd_knn_index_radii_allow.argtypes = [vp, vp, i32, vp]
    L.kmamd_knn_index_radius_count_allow.restype = i32
    L.kmamd_knn_index_radius_count_allow.argtypes = [vp, f32, u32, vp, vp, vp, vp, i32, vp]
    L.kmamd_knn_index_radius_fill_allow.restype = i32
    L.kmamd_knn_index_radius_fill_allow.argtypes = [vp, f32, u32, vp, vp, vp, vp, vp, i32, vp]
    L.kmamd_knn_index_query_capped.restype = i32
    L.kmamd_knn_index_query_capped.argtypes = [vp, u32, f32, u32, vp, vp, vp, vp, vp, i32, vp]
    L.kmamd_knn_index_query_probe_capped.restype = i32
    L.kmamd_knn_index_query_probe_capped.argtypes = [vp, u32, f32, u32, u32, vp, vp, vp, vp, vp, i32, vp]
    L.kmamd_knn_index_destroy.restype = None
    L.kmamd_knn_index_destroy.argtypes = [vp]
    L.kmamd_kmeans_assign.restype = i32
    L.kmamd_kmeans_assign.argtypes = [i32, u32, ctypes.c_uint16, u32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.kmamd_assigned_distances.restype = i32
    L.kmamd_assigned_distances.argtypes = [i32, u32, u32, u32, i32, vp, vp, vp, vp, vp]
    L.kmamd_kmeans_assign_top.restype = i32
    L.kmamd_kmeans_assign_top.argtypes = [i32, u32, ctypes.c_uint16, u32, u32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.kmamd_assign_top_stats.restype = i32
    L.kmamd_assign_top_stats.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.kmamd_kmeans_seed_parallel.restype = i32
    L.kmamd_kmeans_seed_parallel.argtypes = [i32, u32, ctypes.c_uint16, u32, u32, f32, u32, i32, i32, i32, i32, vp, vp,
                                             vp, vp, u32, vp, vp, vp]
    L.kmamd_minibatch_create.restype = i32
    L.kmamd_minibatch_create.argtypes = [ctypes.POINTER(vp), i32, u32, u32, i32, i32, i32, vp, vp]
    L.kmamd_minibatch_step.restype = i32
    L.kmamd_minibatch_step.argtypes = [vp, u32, i32, vp, vp, vp, i32]
    L.kmamd_minibatch_fit.restype = i32
    L.kmamd_minibatch_fit.argtypes = [vp, ctypes.c_uint64, i32, vp, vp, u32, u32, u32, i32]
    L.kmamd_minibatch_read.restype = i32
    L.kmamd_minibatch_read.argtypes = [vp, vp, vp, ctypes.POINTER(ctypes.c_uint64), i32]
    L.kmamd_minibatch_destroy.restype = None
    L.kmamd_minibatch_destroy.argtypes = [vp]
    L.kmamd_copy_to_device.restype = i32
    L.kmamd_copy_to_device.argtypes = [i32, vp, vp, ctypes.c_size_t]
    L.kmamd_build_arch.restype = ctypes.c_char_p
    _lib = L
    return L


STATUS = {0: "Success", 1: "InvalidArguments", 2: "NoSuchDevice", 3: "MemoryAllocationFailure",
          4: "RuntimeError", 5: "MemoryCopyError"}


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, STATUS.get(rc, rc)))
