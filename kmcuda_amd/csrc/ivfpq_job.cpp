// ivfpq_job.cpp -- kmamd_ivfpq_search, kmamd_ivfpq4_search, kmamd_ivfpq_search_f16, kmamd_ivfpq_search_precomputed,
// kmamd_ivfpq_search_nonresidual, kmamd_ivfpq_search_nonresidual_f16, kmamd_ivfpq_terms, kmamd_ivfpq_residuals, the
// query-tile rules and kmamd_ivfpq_row_split of include/kmcuda_amd.h: IVF-PQ search (4-bit codes
// 4.25; fp16 lookup tables 4.26; non-residual lists 4.27).  The kernels are ivfpq_scan.hip's,
// pq4_scan.hip's, pq16_scan.hip's and pq_scan.hip's merge; nothing here goes through an Engine.
//
// The index goes to the device whole.  The queries are cut into chunks whose partial keys stay within kIvfPqPartBytes;
// per chunk seven launches on one stream -- the pair sort (clear, count, prefix, scatter), the fill of the partial
// keys, scan, merge -- and no host round trip before the end.  The precomputed search adds two launches per chunk, the
// chunk's query terms and pair norms, and keeps the query terms within kIvfPqPartBytes as well.  The non-residual
// searches add one, the chunk's query tables, under the same bound.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "../../include/kmcuda_amd.h"
#include "host_job.hpp"

using namespace kmx;

namespace {

constexpr size_t kIvfPqPartBytes = (size_t)512 << 20;   // the partial keys of one query chunk at one row split

// Queries per chunk; KMCUDA_AMD_IVFPQ_QUERY_CHUNK: queries per chunk (the tests force small chunks).  qterm_subspaces:
// M where the chunk's query terms or query tables (M x 256 entries per query, M KB as floats) are held as well -- a
// bound of 2^27 entries the override does not lift, because the scan indexes them in 32 bits --, else 0
uint32_t ivfpq_query_chunk(uint32_t nprobe, uint32_t k, uint32_t qterm_subspaces) {
  size_t chunk = kIvfPqPartBytes / ((size_t)nprobe * k * sizeof(uint64_t));
  if (const char *v = getenv("KMCUDA_AMD_IVFPQ_QUERY_CHUNK")) {
    const long long n = atoll(v);
    if (n > 0) chunk = (size_t)std::min<long long>(n, 1 << 20);
  }
  if (qterm_subspaces) chunk = std::min(chunk, kIvfPqPartBytes / ((size_t)qterm_subspaces * 256 * sizeof(float)));
  return (uint32_t)(chunk < 1 ? 1 : chunk);
}

// The searches: with `precomputed` the tables come from `terms`, else from the residuals (4.22).
// bits 8: a code per byte, M <= 64, ksub <= 256; bits 4: two per byte, M <= 128, ksub <= 16, never precomputed (4.25).
// f16: the byte codes over tables of halves built from the residuals (4.26), never precomputed and never with bits 4.
// !residual: the lists hold the codes of the rows themselves and the tables are the queries' own (4.27), as floats or
// with f16 as halves; never precomputed and never with bits 4; `centroids` is checked and not read.
int ivfpq_search_job(bool precomputed, uint32_t bits, bool f16, bool residual, uint32_t queries_size, uint64_t list_rows, uint32_t features_size,
                     uint32_t clusters_size, uint32_t subspaces, uint32_t sub_features, uint32_t sub_clusters,
                     uint32_t k, uint32_t nprobe, int metric, int32_t fp16x2, int device, int32_t device_ptrs,
                     int32_t verbosity, const float *queries, const float *centroids, const float *codebooks,
                     const uint8_t *codes, const uint32_t *ids, const uint32_t *offsets, const uint32_t *probes,
                     const float *terms, uint32_t *indices, float *distances) {
  const uint32_t Q = queries_size, K = clusters_size, M = subspaces, dsub = sub_features, ksub = sub_clusters;
  const uint64_t L = list_rows;
  const bool nib = bits == 4;
  const uint32_t width = nib ? (M + 1) / 2 : M;   // bytes of a code row
  // everything that is refused, before any device work
  if (M == 0 || M > (nib ? 128u : 64u) || dsub == 0 || dsub > 64 || ksub == 0 || ksub > (nib ? 16u : 256u))
    return kmcudaInvalidArguments;
  if ((nib || f16 || !residual) && precomputed) return kmcudaInvalidArguments;
  if (nib && !residual) return kmcudaInvalidArguments;
  if (features_size != M * dsub || metric != 0 || fp16x2 != 0) return kmcudaInvalidArguments;
  if (L == 0 || L > 0xFFFFFFFEull || k == 0 || k > 256) return kmcudaInvalidArguments;
  if (K == 0 || nprobe == 0 || nprobe > std::min(K, 64u)) return kmcudaInvalidArguments;
  if (device < 0 || (device_ptrs >= 0 && device_ptrs != device)) return kmcudaInvalidArguments;
  if (!centroids || !codebooks || !codes || !ids || !offsets || (precomputed && !terms)) return kmcudaInvalidArguments;
  if (Q != 0 && (!queries || !probes || !indices || !distances)) return kmcudaInvalidArguments;
  if (Q == 0) return kmcudaSuccess;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return kmcudaNoSuchDevice;
  if (hipSetDevice(device) != hipSuccess) return kmcudaNoSuchDevice;
  g_verbosity = verbosity;
  const bool host = device_ptrs < 0;
  if (!host) (void)hipDeviceSynchronize();   // the caller's writes, as kmamd_kmeans_assign

  DeviceArena w;
  w.dev = device;
  w.stream = pooled_stream_acquire(device);
  if (!w.stream) return kmcudaRuntimeError;
  const hipStream_t st = w.stream;
  const float *qry = nullptr;
  const uint32_t *prb = nullptr;
  IvfPqGeom g{};
  KNN_TRY(w.stage_in(queries, (size_t)Q * features_size, device_ptrs, &qry));
  KNN_TRY(w.stage_in(probes, (size_t)Q * nprobe, device_ptrs, &prb));
  if (residual) KNN_TRY(w.stage_in(centroids, (size_t)K * features_size, device_ptrs, &g.centroids));
  KNN_TRY(w.stage_in(codebooks, (size_t)M * ksub * dsub, device_ptrs, &g.codebooks));
  KNN_TRY(w.stage_in(codes, (size_t)L * width, device_ptrs, &g.codes));
  KNN_TRY(w.stage_in(ids, (size_t)L, device_ptrs, &g.ids));
  KNN_TRY(w.stage_in(offsets, (size_t)K + 1, device_ptrs, &g.offsets));
  const float *trm = nullptr;
  if (precomputed) KNN_TRY(w.stage_in(terms, (size_t)K * M * ksub, device_ptrs, &trm));
  uint32_t *idx = indices;
  float *dist = distances;
  if (host) {
    KNN_TRY(w.alloc(&idx, (size_t)Q * k));
    KNN_TRY(w.alloc(&dist, (size_t)Q * k));
  }
  g.L = L; g.K = K; g.M = M; g.dsub = dsub; g.ksub = ksub; g.k = k; g.nprobe = nprobe;
  // no staging tile in the precomputed block, none of its own in the 4-bit block and the fp16-table block
  g.QT = nib ? pq4_query_tile(M, k) : f16 ? pq16_query_tile(M, k) : precomputed || !residual ? pq_query_tile(M, k)
                                                                                             : ivfpq_query_tile(M, k);
  g.cap = pq_candidate_cap(k);
  const uint32_t chunk = std::min(ivfpq_query_chunk(nprobe, k, precomputed || !residual ? M : 0), Q);
  // the full chunks and the last one differ in their row split: the keys are sized for the larger of the two
  size_t part_keys = 0;
  for (uint32_t qc : {chunk, Q % chunk})
    if (qc != 0)
      part_keys = std::max(part_keys, (size_t)qc * nprobe * ivfpq_row_split((uint64_t)qc * nprobe, g.QT, L) * k);
  uint32_t *hist = nullptr, *pair_start = nullptr, *tile_start = nullptr, *cursor = nullptr, *pairs = nullptr;
  uint64_t *part = nullptr;
  KNN_TRY(w.alloc(&hist, (size_t)K));
  KNN_TRY(w.alloc(&pair_start, (size_t)K + 1));
  KNN_TRY(w.alloc(&tile_start, (size_t)K + 1));
  KNN_TRY(w.alloc(&cursor, (size_t)K + 1));
  KNN_TRY(w.alloc(&pairs, (size_t)chunk * nprobe));
  KNN_TRY(w.alloc(&part, part_keys));
  float *qterms = nullptr, *norms = nullptr;
  if (precomputed) {
    KNN_TRY(w.alloc(&qterms, (size_t)chunk * M * 256));
    KNN_TRY(w.alloc(&norms, (size_t)chunk * nprobe));
  }
  uint16_t *qtables16 = nullptr;   // the non-residual searches' query tables: qterms as floats, these as halves
  if (!residual && f16) KNN_TRY(w.alloc(&qtables16, (size_t)chunk * M * 256));
  if (!residual && !f16) KNN_TRY(w.alloc(&qterms, (size_t)chunk * M * 256));
  for (uint32_t q0 = 0; q0 < Q; q0 += chunk) {
    const uint32_t qc = std::min(chunk, Q - q0), P = qc * nprobe;
    g.S = ivfpq_row_split(P, g.QT, L);
    const uint32_t tiles = (uint32_t)std::min<uint64_t>(P, (uint64_t)(P + g.QT - 1) / g.QT + K);
    if (verbosity > 1)
      printf("ivfpq_search%s%s: queries [%u, %u), %u pairs, tile %u, at most %u tiles x %u row splits\n",
             precomputed ? " (precomputed)" : residual ? "" : " (non-residual)",
             nib ? " (4-bit)" : f16 ? " (fp16 tables)" : "", q0, q0 + qc, P, g.QT, tiles, g.S);
    KMX_HIPRT(launch_ivfpq_group(prb + (size_t)q0 * nprobe, P, nprobe, K, g.QT, hist, pair_start, tile_start, cursor,
                                 pairs, st));
    KMX_HIPRT(launch_batched_fill(reinterpret_cast<uint32_t *>(part), (uint64_t)P * g.S * k * 2, ~0u, st));
    const float *qc_rows = qry + (size_t)q0 * features_size;
    const uint32_t *qc_probes = prb + (size_t)q0 * nprobe;
    if (precomputed) {
      KMX_HIPRT(launch_ivfpq_query_terms(qc_rows, qc, g.codebooks, M, dsub, ksub, qterms, st));
      KMX_HIPRT(launch_ivfpq_pair_norms(qc_rows, g.centroids, qc_probes, P, nprobe, K, features_size, norms, st));
      KMX_HIPRT(launch_ivfpq_scan_pre(g, trm, qterms, norms, tiles, pair_start, tile_start, pairs, part, st));
    } else if (!residual && f16) {
      KMX_HIPRT(launch_ivfpq_query_tables_f16(qc_rows, qc, g.codebooks, M, dsub, ksub, qtables16, st));
      KMX_HIPRT(launch_ivfpq16_scan_nonres(g, qtables16, tiles, pair_start, tile_start, pairs, part, st));
    } else if (!residual) {
      KMX_HIPRT(launch_ivfpq_query_tables(qc_rows, qc, g.codebooks, M, dsub, ksub, qterms, st));
      KMX_HIPRT(launch_ivfpq_scan_nonres(g, qterms, tiles, pair_start, tile_start, pairs, part, st));
    } else if (nib) {
      KMX_HIPRT(launch_ivfpq4_scan(g, qc_rows, tiles, pair_start, tile_start, pairs, part, st));
    } else if (f16) {
      KMX_HIPRT(launch_ivfpq16_scan(g, qc_rows, tiles, pair_start, tile_start, pairs, part, st));
    } else {
      KMX_HIPRT(launch_ivfpq_scan(g, qc_rows, tiles, pair_start, tile_start, pairs, part, st));
    }
    KMX_HIPRT(launch_pq_merge(part, qc, nprobe * g.S, k, idx + (size_t)q0 * k, dist + (size_t)q0 * k, st));
  }
  if (host) {
    KMX_HIPCP(hipMemcpyAsync(indices, idx, (size_t)Q * k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KMX_HIPCP(hipMemcpyAsync(distances, dist, (size_t)Q * k * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    if (verbosity > 0) printf("kmamd_ivfpq_search failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  return kmcudaSuccess;
}

}  // namespace

extern "C" {

uint32_t kmamd_ivfpq_query_tile(uint32_t subspaces, uint32_t k) { return ivfpq_query_tile(subspaces, k); }

uint32_t kmamd_ivfpq4_query_tile(uint32_t subspaces, uint32_t k) { return pq4_query_tile(subspaces, k); }

uint32_t kmamd_ivfpq_f16_query_tile(uint32_t subspaces, uint32_t k) { return pq16_query_tile(subspaces, k); }

uint32_t kmamd_ivfpq_row_split(uint64_t pairs, uint32_t query_tile, uint64_t list_rows) {
  return ivfpq_row_split(pairs, query_tile, list_rows);
}

int kmamd_ivfpq_search(uint32_t queries_size, uint64_t list_rows, uint32_t features_size, uint32_t clusters_size,
                       uint32_t subspaces, uint32_t sub_features, uint32_t sub_clusters, uint32_t k, uint32_t nprobe,
                       int metric, int32_t fp16x2, int device, int32_t device_ptrs, int32_t verbosity,
                       const float *queries, const float *centroids, const float *codebooks, const uint8_t *codes,
                       const uint32_t *ids, const uint32_t *offsets, const uint32_t *probes, uint32_t *indices,
                       float *distances) {
  return ivfpq_search_job(false, 8, false, true, queries_size, list_rows, features_size, clusters_size, subspaces, sub_features,
                          sub_clusters, k, nprobe, metric, fp16x2, device, device_ptrs, verbosity, queries, centroids,
                          codebooks, codes, ids, offsets, probes, nullptr, indices, distances);
}

int kmamd_ivfpq4_search(uint32_t queries_size, uint64_t list_rows, uint32_t features_size, uint32_t clusters_size,
                        uint32_t subspaces, uint32_t sub_features, uint32_t sub_clusters, uint32_t k, uint32_t nprobe,
                        int metric, int32_t fp16x2, int device, int32_t device_ptrs, int32_t verbosity,
                        const float *queries, const float *centroids, const float *codebooks, const uint8_t *codes,
                        const uint32_t *ids, const uint32_t *offsets, const uint32_t *probes, uint32_t *indices,
                        float *distances) {
  return ivfpq_search_job(false, 4, false, true, queries_size, list_rows, features_size, clusters_size, subspaces, sub_features,
                          sub_clusters, k, nprobe, metric, fp16x2, device, device_ptrs, verbosity, queries, centroids,
                          codebooks, codes, ids, offsets, probes, nullptr, indices, distances);
}

int kmamd_ivfpq_search_f16(uint32_t queries_size, uint64_t list_rows, uint32_t features_size, uint32_t clusters_size,
                           uint32_t subspaces, uint32_t sub_features, uint32_t sub_clusters, uint32_t k,
                           uint32_t nprobe, int metric, int32_t fp16x2, int device, int32_t device_ptrs,
                           int32_t verbosity, const float *queries, const float *centroids, const float *codebooks,
                           const uint8_t *codes, const uint32_t *ids, const uint32_t *offsets, const uint32_t *probes,
                           uint32_t *indices, float *distances) {
  return ivfpq_search_job(false, 8, true, true, queries_size, list_rows, features_size, clusters_size, subspaces,
                          sub_features, sub_clusters, k, nprobe, metric, fp16x2, device, device_ptrs, verbosity,
                          queries, centroids, codebooks, codes, ids, offsets, probes, nullptr, indices, distances);
}

int kmamd_ivfpq_search_precomputed(uint32_t queries_size, uint64_t list_rows, uint32_t features_size,
                                   uint32_t clusters_size, uint32_t subspaces, uint32_t sub_features,
                                   uint32_t sub_clusters, uint32_t k, uint32_t nprobe, int metric, int32_t fp16x2,
                                   int device, int32_t device_ptrs, int32_t verbosity, const float *queries,
                                   const float *centroids, const float *codebooks, const uint8_t *codes,
                                   const uint32_t *ids, const uint32_t *offsets, const uint32_t *probes,
                                   const float *terms, uint32_t *indices, float *distances) {
  return ivfpq_search_job(true, 8, false, true, queries_size, list_rows, features_size, clusters_size, subspaces, sub_features,
                          sub_clusters, k, nprobe, metric, fp16x2, device, device_ptrs, verbosity, queries, centroids,
                          codebooks, codes, ids, offsets, probes, terms, indices, distances);
}

int kmamd_ivfpq_search_nonresidual(uint32_t queries_size, uint64_t list_rows, uint32_t features_size,
                                   uint32_t clusters_size, uint32_t subspaces, uint32_t sub_features,
                                   uint32_t sub_clusters, uint32_t k, uint32_t nprobe, int metric, int32_t fp16x2,
                                   int device, int32_t device_ptrs, int32_t verbosity, const float *queries,
                                   const float *centroids, const float *codebooks, const uint8_t *codes,
                                   const uint32_t *ids, const uint32_t *offsets, const uint32_t *probes,
                                   uint32_t *indices, float *distances) {
  return ivfpq_search_job(false, 8, false, false, queries_size, list_rows, features_size, clusters_size, subspaces,
                          sub_features, sub_clusters, k, nprobe, metric, fp16x2, device, device_ptrs, verbosity,
                          queries, centroids, codebooks, codes, ids, offsets, probes, nullptr, indices, distances);
}

int kmamd_ivfpq_search_nonresidual_f16(uint32_t queries_size, uint64_t list_rows, uint32_t features_size,
                                       uint32_t clusters_size, uint32_t subspaces, uint32_t sub_features,
                                       uint32_t sub_clusters, uint32_t k, uint32_t nprobe, int metric, int32_t fp16x2,
                                       int device, int32_t device_ptrs, int32_t verbosity, const float *queries,
                                       const float *centroids, const float *codebooks, const uint8_t *codes,
                                       const uint32_t *ids, const uint32_t *offsets, const uint32_t *probes,
                                       uint32_t *indices, float *distances) {
  return ivfpq_search_job(false, 8, true, false, queries_size, list_rows, features_size, clusters_size, subspaces,
                          sub_features, sub_clusters, k, nprobe, metric, fp16x2, device, device_ptrs, verbosity,
                          queries, centroids, codebooks, codes, ids, offsets, probes, nullptr, indices, distances);
}

int kmamd_ivfpq_terms(uint32_t clusters_size, uint32_t features_size, uint32_t subspaces, uint32_t sub_features,
                      uint32_t sub_clusters, int device, int32_t device_ptrs, int32_t verbosity,
                      const float *centroids, const float *codebooks, float *terms) {
  const uint32_t K = clusters_size, M = subspaces, dsub = sub_features, ksub = sub_clusters;
  if (M == 0 || M > 64 || dsub == 0 || dsub > 64 || ksub == 0 || ksub > 256) return kmcudaInvalidArguments;
  if (features_size != M * dsub || K == 0) return kmcudaInvalidArguments;
  if (device < 0 || (device_ptrs >= 0 && device_ptrs != device)) return kmcudaInvalidArguments;
  if (!centroids || !codebooks || !terms) return kmcudaInvalidArguments;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return kmcudaNoSuchDevice;
  if (hipSetDevice(device) != hipSuccess) return kmcudaNoSuchDevice;
  g_verbosity = verbosity;
  const bool host = device_ptrs < 0;
  if (!host) (void)hipDeviceSynchronize();

  DeviceArena w;
  w.dev = device;
  w.stream = pooled_stream_acquire(device);
  if (!w.stream) return kmcudaRuntimeError;
  const hipStream_t st = w.stream;
  const float *cen = nullptr, *books = nullptr;
  const size_t count = (size_t)K * M * ksub;
  KNN_TRY(w.stage_in(centroids, (size_t)K * features_size, device_ptrs, &cen));
  KNN_TRY(w.stage_in(codebooks, (size_t)M * ksub * dsub, device_ptrs, &books));
  float *out = terms;
  if (host) KNN_TRY(w.alloc(&out, count));
  KMX_HIPRT(launch_ivfpq_terms(cen, books, K, M, dsub, ksub, out, st));
  if (host) KMX_HIPCP(hipMemcpyAsync(terms, out, count * sizeof(float), hipMemcpyDeviceToHost, st));
  if (hipStreamSynchronize(st) != hipSuccess) {
    if (verbosity > 0) printf("kmamd_ivfpq_terms failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  return kmcudaSuccess;
}

int kmamd_ivfpq_residuals(uint64_t samples_size, uint32_t features_size, uint32_t clusters_size, int device,
                          int32_t device_ptrs, int32_t verbosity, const float *samples, const float *centroids,
                          const uint32_t *assignments, float *residuals) {
  const uint64_t N = samples_size;
  const uint32_t D = features_size, K = clusters_size;
  if (D == 0 || K == 0 || N > 0xFFFFFFFFull) return kmcudaInvalidArguments;
  if (device < 0 || (device_ptrs >= 0 && device_ptrs != device)) return kmcudaInvalidArguments;
  if (!centroids || (N != 0 && (!samples || !assignments || !residuals))) return kmcudaInvalidArguments;
  if (N == 0) return kmcudaSuccess;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device >= ndev) return kmcudaNoSuchDevice;
  if (hipSetDevice(device) != hipSuccess) return kmcudaNoSuchDevice;
  g_verbosity = verbosity;
  const bool host = device_ptrs < 0;
  if (!host) (void)hipDeviceSynchronize();

  DeviceArena w;
  w.dev = device;
  w.stream = pooled_stream_acquire(device);
  if (!w.stream) return kmcudaRuntimeError;
  const hipStream_t st = w.stream;
  const float *x = nullptr, *cen = nullptr;
  const uint32_t *a = nullptr;
  KNN_TRY(w.stage_in(samples, (size_t)N * D, device_ptrs, &x));
  KNN_TRY(w.stage_in(centroids, (size_t)K * D, device_ptrs, &cen));
  KNN_TRY(w.stage_in(assignments, (size_t)N, device_ptrs, &a));
  float *out = residuals;
  if (host) KNN_TRY(w.alloc(&out, (size_t)N * D));
  KMX_HIPRT(launch_ivfpq_residuals(x, cen, a, N, D, K, out, st));
  if (host) KMX_HIPCP(hipMemcpyAsync(residuals, out, (size_t)N * D * sizeof(float), hipMemcpyDeviceToHost, st));
  if (hipStreamSynchronize(st) != hipSuccess) {
    if (verbosity > 0) printf("kmamd_ivfpq_residuals failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  return kmcudaSuccess;
}

}  // extern "C"
