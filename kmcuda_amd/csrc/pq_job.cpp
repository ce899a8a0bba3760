// pq_job.cpp -- kmamd_pq_search, kmamd_pq4_search, kmamd_pq_search_f16 and their query-tile rules of
// include/kmcuda_amd.h: top-k search over product-quantiser codes, one per byte (with fp16 lookup
// tables 4.26) or two (4.25).  The kernels are pq_scan.hip's, pq4_scan.hip's and pq16_scan.hip's; nothing here goes
// through an Engine.
//
// The codes go to the device whole.  The queries are cut into chunks whose tables stay within kPqTableBytes; per chunk
// three launches on one stream -- tables, scan, merge -- and no host round trip before the end.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "../../include/kmcuda_amd.h"
#include "host_job.hpp"

using namespace kmx;

namespace {

constexpr size_t kPqTableBytes = (size_t)512 << 20;   // the tables of one query chunk
constexpr uint32_t kPqBlocks = 512;                   // the grid (row chunks x query tiles) aims at two blocks per CU

// Queries per chunk, a multiple of QT, their tables `bytes` per sub-space and query; KMCUDA_AMD_PQ_QUERY_CHUNK: queries
// per chunk (the tests force small chunks)
uint32_t pq_query_chunk(uint32_t M, size_t bytes, uint32_t QT) {
  size_t chunk = kPqTableBytes / ((size_t)M * bytes);
  if (const char *v = getenv("KMCUDA_AMD_PQ_QUERY_CHUNK")) {
    const long long n = atoll(v);
    if (n > 0) chunk = (size_t)std::min<long long>(n, 1 << 20);
  }
  chunk = chunk / QT * QT;
  return (uint32_t)(chunk < QT ? QT : chunk);
}

// Row chunks for a launch of `tiles` query tiles: whole 256-row tiles, about kPqBlocks blocks in all, every chunk with
// a row in it
void pq_row_chunks(uint64_t N, uint32_t tiles, PqGeom *g) {
  const uint64_t row_tiles = (N + 255) / 256;
  uint64_t want = (kPqBlocks + tiles - 1) / tiles;
  if (want > row_tiles) want = row_tiles;
  g->R = (row_tiles + want - 1) / want * 256;
  g->G = (uint32_t)((N + g->R - 1) / g->R);
}

// The searches.  bits 8: a code per byte, M <= 64, ksub <= 256; bits 4: two per byte, M <= 128, ksub <= 16.  f16: the
// byte codes over tables of halves (never with bits 4)
int pq_search_job(uint32_t bits, bool f16, uint32_t queries_size, uint64_t samples_size, uint32_t features_size,
                  uint32_t subspaces, uint32_t sub_features, uint32_t sub_clusters, uint32_t k, int metric,
                  int32_t fp16x2, int device, int32_t device_ptrs, int32_t verbosity, const float *queries,
                  const float *codebooks, const uint8_t *codes, uint32_t *indices, float *distances) {
  const uint32_t Q = queries_size, M = subspaces, dsub = sub_features, ksub = sub_clusters;
  const uint64_t N = samples_size;
  const bool nib = bits == 4;
  const uint32_t entries = nib ? 16 : 256, width = nib ? (M + 1) / 2 : M;   // of a sub-space's table; of a code row
  const size_t entry_bytes = f16 ? sizeof(uint16_t) : sizeof(float);
  // everything that is refused, before any device work
  if (M == 0 || M > (nib ? 128u : 64u) || dsub == 0 || dsub > 64 || ksub == 0 || ksub > entries)
    return kmcudaInvalidArguments;
  if (features_size != M * dsub || metric != 0 || fp16x2 != 0) return kmcudaInvalidArguments;
  if (N == 0 || N > 0xFFFFFFFFull || k == 0 || k > 256 || k > N) return kmcudaInvalidArguments;
  if (device < 0 || (device_ptrs >= 0 && device_ptrs != device)) return kmcudaInvalidArguments;
  if (!codebooks || !codes || (Q != 0 && (!queries || !indices || !distances))) return kmcudaInvalidArguments;
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
  const float *qry = nullptr, *books = nullptr;
  PqGeom g{};
  KNN_TRY(w.stage_in(queries, (size_t)Q * features_size, device_ptrs, &qry));
  KNN_TRY(w.stage_in(codebooks, (size_t)M * ksub * dsub, device_ptrs, &books));
  KNN_TRY(w.stage_in(codes, (size_t)N * width, device_ptrs, &g.codes));
  uint32_t *idx = indices;
  float *dist = distances;
  if (host) {
    KNN_TRY(w.alloc(&idx, (size_t)Q * k));
    KNN_TRY(w.alloc(&dist, (size_t)Q * k));
  }
  g.N = N; g.M = M; g.k = k;
  g.QT = nib ? pq4_query_tile(M, k) : f16 ? pq16_query_tile(M, k) : pq_query_tile(M, k);
  g.cap = pq_candidate_cap(k);
  const uint32_t chunk =
      std::min<uint64_t>(pq_query_chunk(M, entries * entry_bytes, g.QT), ((uint64_t)Q + g.QT - 1) / g.QT * g.QT);
  // the full chunks and the last one differ in their row chunks: the keys are sized for the larger of the two
  size_t part_keys = 0;
  for (uint32_t qc : {std::min(chunk, Q), Q % chunk}) {
    if (qc == 0) continue;
    pq_row_chunks(N, (qc + g.QT - 1) / g.QT, &g);
    part_keys = std::max(part_keys, (size_t)qc * g.G * k);
  }
  uint8_t *table_bytes = nullptr;
  uint64_t *part = nullptr;
  KNN_TRY(w.alloc(&table_bytes, (size_t)chunk * M * entries * entry_bytes));
  float *tables = reinterpret_cast<float *>(table_bytes);
  uint16_t *tables16 = reinterpret_cast<uint16_t *>(table_bytes);
  KNN_TRY(w.alloc(&part, part_keys));
  for (uint32_t q0 = 0; q0 < Q; q0 += chunk) {
    const uint32_t qc = std::min(chunk, Q - q0);
    pq_row_chunks(N, (qc + g.QT - 1) / g.QT, &g);
    if (verbosity > 1)
      printf("%s: queries [%u, %u), tile %u, %u row chunks of %llu rows\n",
             nib ? "pq4_search" : f16 ? "pq_search_f16" : "pq_search", q0, q0 + qc, g.QT, g.G,
             (unsigned long long)g.R);
    const float *qc_rows = qry + (size_t)q0 * features_size;
    if (nib) {
      KMX_HIPRT(launch_pq4_tables(qc_rows, qc, books, M, dsub, ksub, g.QT, tables, st));
      KMX_HIPRT(launch_pq4_scan(g, tables, qc, part, st));
    } else if (f16) {
      KMX_HIPRT(launch_pq16_tables(qc_rows, qc, books, M, dsub, ksub, g.QT, tables16, st));
      KMX_HIPRT(launch_pq16_scan(g, tables16, qc, part, st));
    } else {
      KMX_HIPRT(launch_pq_tables(qc_rows, qc, books, M, dsub, ksub, g.QT, tables, st));
      KMX_HIPRT(launch_pq_scan(g, tables, qc, part, st));
    }
    KMX_HIPRT(launch_pq_merge(part, qc, g.G, k, idx + (size_t)q0 * k, dist + (size_t)q0 * k, st));
  }
  if (host) {
    KMX_HIPCP(hipMemcpyAsync(indices, idx, (size_t)Q * k * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    KMX_HIPCP(hipMemcpyAsync(distances, dist, (size_t)Q * k * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  if (hipStreamSynchronize(st) != hipSuccess) {
    if (verbosity > 0) printf("kmamd_pq_search failed: %s\n", hipGetErrorString(hipGetLastError()));
    return kmcudaRuntimeError;
  }
  return kmcudaSuccess;
}

}  // namespace

extern "C" {

uint32_t kmamd_pq_query_tile(uint32_t subspaces, uint32_t k) { return pq_query_tile(subspaces, k); }

uint32_t kmamd_pq4_query_tile(uint32_t subspaces, uint32_t k) { return pq4_query_tile(subspaces, k); }

uint32_t kmamd_pq_f16_query_tile(uint32_t subspaces, uint32_t k) { return pq16_query_tile(subspaces, k); }

int kmamd_pq_search(uint32_t queries_size, uint64_t samples_size, uint32_t features_size, uint32_t subspaces,
                    uint32_t sub_features, uint32_t sub_clusters, uint32_t k, int metric, int32_t fp16x2, int device,
                    int32_t device_ptrs, int32_t verbosity, const float *queries, const float *codebooks,
                    const uint8_t *codes, uint32_t *indices, float *distances) {
  return pq_search_job(8, false, queries_size, samples_size, features_size, subspaces, sub_features, sub_clusters, k, metric,
                       fp16x2, device, device_ptrs, verbosity, queries, codebooks, codes, indices, distances);
}

int kmamd_pq4_search(uint32_t queries_size, uint64_t samples_size, uint32_t features_size, uint32_t subspaces,
                     uint32_t sub_features, uint32_t sub_clusters, uint32_t k, int metric, int32_t fp16x2, int device,
                     int32_t device_ptrs, int32_t verbosity, const float *queries, const float *codebooks,
                     const uint8_t *codes, uint32_t *indices, float *distances) {
  return pq_search_job(4, false, queries_size, samples_size, features_size, subspaces, sub_features, sub_clusters, k, metric,
                       fp16x2, device, device_ptrs, verbosity, queries, codebooks, codes, indices, distances);
}

int kmamd_pq_search_f16(uint32_t queries_size, uint64_t samples_size, uint32_t features_size, uint32_t subspaces,
                        uint32_t sub_features, uint32_t sub_clusters, uint32_t k, int metric, int32_t fp16x2, int device,
                        int32_t device_ptrs, int32_t verbosity, const float *queries, const float *codebooks,
                        const uint8_t *codes, uint32_t *indices, float *distances) {
  return pq_search_job(8, true, queries_size, samples_size, features_size, subspaces, sub_features, sub_clusters, k,
                       metric, fp16x2, device, device_ptrs, verbosity, queries, codebooks, codes, indices, distances);
}

}  // extern "C"
