/*
 * kmcuda_oracle.c -- TEST INFRASTRUCTURE ONLY (see kmcuda_oracle.h).
 *
 * Plain-C CPU restatement of the arithmetic of src-d/kmcuda's distance/assignment hot
 * path.  fp32 semantics restated from fp_abstraction.h:23-98:
 *   _fma(acc,a,b) = __fmaf_rd(a,b,acc)  -> fused multiply-add rounded toward -inf
 *   _add/_sub/_mul                      -> IEEE round-to-nearest
 *   _sqrt = __fsqrt_rn, _reciprocal = __frcp_rn -> correctly rounded (sqrtf, 1.0f/x)
 * Build with -ffp-contract=off and without -ffast-math (oracle/Makefile).
 *
 * Parity pinning: reference is CUDA-only => no oracle/_ref; pinned on the reference's own
 * known-answer tests (src/test.py iteration counts + sklearn agreement).  The angular
 * metric goes through libm acosf, which is not bit-identical to CUDA's acosf
 * ("parity unpinned" for angular beyond the reference's own loose thresholds).  The AFK-MC2
 * seeding draws from a restatement of XORWOW, not from cuRAND: "parity unpinned" beyond the
 * reference's iteration-count pins for that init (see the section comment below).
 */
#include "kmcuda_oracle.h"

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

/* ------------------------------------------------------------------------------------ */
/* round-down FMA                                                                       */
/* ------------------------------------------------------------------------------------ */

float kmo_fma_rd_portable(float a, float b, float c) {
  /* a*b is exact in binary64 (24+24 <= 53 bits, exponent range suffices). */
  const double p = (double)a * (double)b;
  const double cd = (double)c;
  const double z = p + cd;                       /* RN(p + c) */
  if (z != z) return (float)z;                   /* NaN */
  if (isinf(z)) {
    if (isinf(p) || isinf(cd)) return (float)z;  /* genuine infinity */
  }
  /* TwoSum: p + cd == z + e exactly (when finite). */
  const double bb = z - p;
  const double e = (p - (z - bb)) + (cd - bb);
  if (z == 0.0 && e == 0.0) {
    /* exact zero: round-down gives -0 unless both addends are zeros of the same sign */
    if (p == 0.0 && cd == 0.0 && (signbit(p) == signbit(cd))) return signbit(p) ? -0.0f : 0.0f;
    return -0.0f;
  }
  float f = (float)z;                            /* RN to binary32 */
  const double fd = (double)f;
  if (fd > z || (fd == z && e < 0.0)) f = nextafterf(f, -INFINITY);
  return f;
}

#if defined(__x86_64__)
__attribute__((target("avx512f"))) static float fma_rd_avx512(float a, float b, float c) {
  __m128 r = _mm_fmadd_round_ss(_mm_set_ss(a), _mm_set_ss(b), _mm_set_ss(c),
                                _MM_FROUND_TO_NEG_INF | _MM_FROUND_NO_EXC);
  return _mm_cvtss_f32(r);
}
#endif

static int g_avx512 = -1;
#ifdef _OPENMP
#include <omp.h>
#endif
/* threads the OpenMP loops of this file run on (bench.py reports it as cpu_baseline.cores) */
int kmo_num_threads(void) {
#ifdef _OPENMP
  return omp_get_max_threads();
#else
  return 1;
#endif
}

int kmo_have_avx512(void) {
  if (g_avx512 < 0) {
#if defined(__x86_64__)
    g_avx512 = __builtin_cpu_supports("avx512f") ? 1 : 0;
    if (getenv("KMO_FORCE_PORTABLE")) g_avx512 = 0;
#else
    g_avx512 = 0;
#endif
  }
  return g_avx512;
}

float kmo_fma_rd(float a, float b, float c) {
#if defined(__x86_64__)
  if (kmo_have_avx512()) return fma_rd_avx512(a, b, c);
#endif
  return kmo_fma_rd_portable(a, b, c);
}

/* Kahan step, kmeans.cu:335-340: y=fma_rd(a,b,corr); t=acc+y; corr=y-(t-acc); acc=t */
#define KAHAN_STEP(FMA, acc, corr, a, b)        \
  do {                                          \
    const float y_ = FMA((a), (b), (corr));     \
    const float t_ = (acc) + y_;                \
    (corr) = y_ - (t_ - (acc));                 \
    (acc) = t_;                                 \
  } while (0)

static float kahan_dot_portable(const float *a, const float *b, uint32_t D) {
  float acc = 0.f, corr = 0.f;
  for (uint32_t f = 0; f < D; f++) KAHAN_STEP(kmo_fma_rd_portable, acc, corr, a[f], b[f]);
  return acc;
}
static float kahan_sqdiff_portable(const float *a, const float *b, uint32_t D) {
  float acc = 0.f, corr = 0.f;
  for (uint32_t f = 0; f < D; f++) {
    const float d = a[f] - b[f];
    KAHAN_STEP(kmo_fma_rd_portable, acc, corr, d, d);
  }
  return acc;
}
#if defined(__x86_64__)
__attribute__((target("avx512f"))) static float kahan_dot_avx512(const float *a, const float *b, uint32_t D) {
  float acc = 0.f, corr = 0.f;
  for (uint32_t f = 0; f < D; f++) KAHAN_STEP(fma_rd_avx512, acc, corr, a[f], b[f]);
  return acc;
}
__attribute__((target("avx512f"))) static float kahan_sqdiff_avx512(const float *a, const float *b, uint32_t D) {
  float acc = 0.f, corr = 0.f;
  for (uint32_t f = 0; f < D; f++) {
    const float d = a[f] - b[f];
    KAHAN_STEP(fma_rd_avx512, acc, corr, d, d);
  }
  return acc;
}
#endif

float kmo_kahan_dot(const float *a, const float *b, uint32_t D) {
#if defined(__x86_64__)
  if (kmo_have_avx512()) return kahan_dot_avx512(a, b, D);
#endif
  return kahan_dot_portable(a, b, D);
}
static float kahan_sqdiff(const float *a, const float *b, uint32_t D) {
#if defined(__x86_64__)
  if (kmo_have_avx512()) return kahan_sqdiff_avx512(a, b, D);
#endif
  return kahan_sqdiff_portable(a, b, D);
}

/* metric_abstraction.h:171-177 / :248-253: angular distance from a dot product */
static float cos_dist_from_prod(float fp) {
  if (fp >= 1.f) return 0.f;
  if (fp <= -1.f) return (float)M_PI;
  return acosf(fp);
}

/* ------------------------------------------------------------------------------------ */
/* fp16x2: the reference's half2 arithmetic (fp_abstraction.h:100-182, CUDA_ARCH >= 60).     */
/* F = half2: every sample / centroid element is a PAIR of halves (low = feature 2i, high =  */
/* feature 2i+1), every _add/_sub/_mul/_fma is the packed IEEE binary16 operation rounded to  */
/* nearest even (__hadd2, __hsub2, __hmul2, __hfma2 = one rounding), Kahan sums therefore run  */
/* as TWO interleaved half accumulators (even / odd features) with their own compensation       */
/* terms, _fin(v) = __hadd(high, low) folds them in half precision, _const<half2>(int) =        */
/* __int2half_rd (round DOWN), _fmax = 65504, compares are half compares (__hlt).  Values are  */
/* carried here as floats that hold exactly-representable halves; each operation is evaluated */
/* in double (exact for halves: products have 22 significant bits, sums of a product and a   */
/* half fit 53 bits whenever the result is in half range) and rounded ONCE to binary16 by     */
/* h_rn() -- no dependence on the host's _Float16 support.                                    */
/* g_fp16_mode: 0 = fp32 arithmetic, 1 = "storage" (this product's fp16 semantics: the fp32     */
/* arithmetic on half VALUES, centroids rounded to half after every update), 2 = the             */
/* reference's half2 arithmetic restated.                                                      */
/* ------------------------------------------------------------------------------------ */
static int g_fp16_mode = 0;

static float h_rn(double v) {                       /* double -> nearest-even binary16, as float */
  if (v != v || v == 0.0) return (float)v;
  const double a = fabs(v);
  if (a == (double)INFINITY) return (float)v;
  int e;
  (void)frexp(a, &e);                               /* a = m * 2^e, m in [0.5, 1) */
  e -= 1;                                           /* a in [2^e, 2^(e+1)) */
  if (e < -14) e = -14;                             /* subnormal halves: fixed quantum 2^-24 */
  const double q = ldexp(1.0, e - 10);
  const double r = rint(a / q) * q;                 /* exact scaling; rint = nearest-even (default mode) */
  if (r > 65504.0) return v < 0 ? -INFINITY : INFINITY;
  return (float)(v < 0 ? -r : r);
}
static inline float h_add(float a, float b) { return h_rn((double)a + (double)b); }
static inline float h_sub(float a, float b) { return h_rn((double)a - (double)b); }
static inline float h_mul(float a, float b) { return h_rn((double)a * (double)b); }
static inline float h_fma(float a, float b, float c) { return h_rn((double)a * (double)b + (double)c); }  /* __hfma */
static inline float h_from_float(float v) { return h_rn((double)v); }                                   /* __float2half (RN) */
static float h_from_int_rd(int64_t v) {                                                                  /* __int2half_rd */
  float h = h_rn((double)v);
  if (h == INFINITY) return 65504.f;                /* rounding down never reaches +inf */
  if ((double)h > (double)v) {                      /* step to the next half below */
    int e;
    (void)frexp(fabs((double)h), &e);
    e -= 1;
    if (e < -14) e = -14;
    double q = ldexp(1.0, e - 10);
    if (h > 0 && fabs((double)h) == ldexp(1.0, e) && e > -14) q *= 0.5;   /* crossing a binade downward */
    h = (float)((double)h - q);
  }
  return h;
}
#define H2_KAHAN(acc, corr, a, b) do { const float y__ = h_fma((a), (b), (corr)); const float t__ = h_add((acc), y__); \
                                       (corr) = h_sub(y__, h_sub(t__, (acc))); (acc) = t__; } while (0)

/* metric_abstraction.h:21-36, F = half2: returns the two lanes' sums */
static void h2_sum_squares(int metric, const float *vec, uint32_t D, float *lo, float *hi) {
  if (metric != KMO_L2) { *lo = 1.f; *hi = 1.f; return; }   /* :149-158 */
  float s[2] = {0.f, 0.f}, c[2] = {0.f, 0.f};
  for (uint32_t f = 0; f + 1 < D; f += 2)
    for (int l = 0; l < 2; l++) H2_KAHAN(s[l], c[l], vec[f + l], vec[f + l]);
  *lo = s[0]; *hi = s[1];
}
/* Kahan dot product per lane (kmeans.cu:331-341 with F = half2) */
static void h2_dot(const float *a, const float *b, uint32_t D, float *lo, float *hi) {
  float s[2] = {0.f, 0.f}, c[2] = {0.f, 0.f};
  for (uint32_t f = 0; f + 1 < D; f += 2)
    for (int l = 0; l < 2; l++) H2_KAHAN(s[l], c[l], a[f + l], b[f + l]);
  *lo = s[0]; *hi = s[1];
}
/* METRIC::distance(sqr1, sqr2, prod) -> half (metric_abstraction.h:55-57, :171-177) */
static float h2_distance3(int metric, float sq_lo, float sq_hi, float p_lo, float p_hi) {
  if (metric == KMO_L2) {
    const float lo = h_fma(-2.f, p_lo, h_add(0.f, sq_lo)), hi = h_fma(-2.f, p_hi, h_add(0.f, sq_hi));
    return h_add(hi, lo);                           /* _fin */
  }
  const float fp = h_add(p_hi, p_lo);               /* _float(_fin(prod)) */
  if (fp >= 1.f) return 0.f;
  if (fp <= -1.f) return h_from_float((float)M_PI);
  return h_from_float(acosf(fp));
}
/* METRIC::distance / distance_t / distance_tt (:59-101, :179-218) -> float */
static float h2_distance(int metric, const float *a, const float *b, uint32_t D) {
  float s[2] = {0.f, 0.f}, c[2] = {0.f, 0.f};
  if (metric == KMO_L2) {
    for (uint32_t f = 0; f + 1 < D; f += 2)
      for (int l = 0; l < 2; l++) {
        const float d = h_sub(a[f + l], b[f + l]);
        H2_KAHAN(s[l], c[l], d, d);
      }
    return sqrtf(h_add(s[1], s[0]));                /* _sqrt(_float(_fin(dist))): float sqrt of the half sum */
  }
  for (uint32_t f = 0; f + 1 < D; f += 2)
    for (int l = 0; l < 2; l++) H2_KAHAN(s[l], c[l], a[f + l], b[f + l]);
  return h2_distance3(metric, 1.f, 1.f, s[0], s[1]);
}

/* metric_abstraction.h:59-101 (L2: sqrt of Kahan sum of squared differences),
 * :179-218 (cos: acos of Kahan dot).  distance, distance_t and distance_tt share it. */
float kmo_distance(int metric, const float *a, const float *b, uint32_t D) {
  if (g_fp16_mode == 2) return h2_distance(metric, a, b, D);
  if (metric == KMO_L2) return sqrtf(kahan_sqdiff(a, b, D));
  return cos_dist_from_prod(kmo_kahan_dot(a, b, D));
}

/* metric_abstraction.h:21-36: ssqr = Kahan sum fma_rd(v,v,corr);  :149-158: cos -> 1 */
void kmo_sum_squares(int metric, uint32_t K, uint32_t D, const float *centroids, float *csqr) {
  for (uint32_t c = 0; c < K; c++) {
    csqr[c] = (metric == KMO_L2) ? kmo_kahan_dot(centroids + (size_t)c * D, centroids + (size_t)c * D, D) : 1.f;
  }
}

/* ------------------------------------------------------------------------------------ */
/* Lloyd assignment, kmeans.cu:293-364                                                   */
/* ------------------------------------------------------------------------------------ */

/* metric_abstraction.h:55-57: distance(sqr1=0, sqr2=csqr, prod) = fma_rd(-2, prod, 0+csqr) */
static inline float lloyd_dist_scalar(int metric, float csqr, float prod) {
  if (metric == KMO_L2) return kmo_fma_rd(-2.f, prod, 0.f + csqr);
  return cos_dist_from_prod(prod);
}

static void lloyd_finish_row(uint32_t s, int insane, uint32_t nearest, uint32_t K, uint32_t *assignments,
                             uint32_t *assignments_prev, uint32_t *changed) {
  if (nearest == UINT32_MAX) {              /* kmeans.cu:349-357 */
    if (!insane) return;                    /* "nearest neighbor search failed": leaves everything untouched */
    nearest = K;
  }
  const uint32_t ass = assignments[s];      /* kmeans.cu:358-363 */
  assignments_prev[s] = ass;
  if (ass != nearest) {
    assignments[s] = nearest;
    (*changed)++;
  }
}

static void lloyd_assign_portable(int metric, uint32_t N, uint32_t D, uint32_t K, const float *X,
                                  const float *C, const float *csqr, uint32_t *asg, uint32_t *prev,
                                  uint32_t *changed) {
  uint32_t total = 0;
#pragma omp parallel for schedule(static) reduction(+ : total)
  for (uint32_t s = 0; s < N; s++) {
    const float *x = X + (size_t)s * D;
    const int insane = (x[0] != x[0]);      /* kmeans.cu:312 */
    float min_dist = FLT_MAX;
    uint32_t nearest = UINT32_MAX;
    if (!insane) {
      for (uint32_t c = 0; c < K; c++) {
        const float prod = kahan_dot_portable(x, C + (size_t)c * D, D);
        const float dist = (metric == KMO_L2) ? kmo_fma_rd_portable(-2.f, prod, 0.f + csqr[c])
                                              : cos_dist_from_prod(prod);
        if (dist < min_dist) {              /* strict <, ascending c: first minimum wins */
          min_dist = dist;
          nearest = c;
        }
      }
    }
    uint32_t ch = 0;
    lloyd_finish_row(s, insane, nearest, K, asg, prev, &ch);
    total += ch;
  }
  *changed += total;
}

#if defined(__x86_64__)
/* 16 centroids per vector lane group; CT is the centroid matrix transposed and padded:
 * CT[f*K16 + c].  Per-lane arithmetic is exactly the scalar chain above. */
__attribute__((target("avx512f"))) static void lloyd_assign_avx512(
    int metric, uint32_t N, uint32_t D, uint32_t K, const float *X, const float *CT, uint32_t K16,
    const float *csqr16, uint32_t *asg, uint32_t *prev, uint32_t *changed) {
  const int RD = _MM_FROUND_TO_NEG_INF | _MM_FROUND_NO_EXC;
  uint32_t total = 0;
#pragma omp parallel for schedule(static) reduction(+ : total)
  for (uint32_t s = 0; s < N; s++) {
    const float *x = X + (size_t)s * D;
    const int insane = (x[0] != x[0]);
    float min_dist = FLT_MAX;
    uint32_t nearest = UINT32_MAX;
    if (!insane) {
      for (uint32_t cb = 0; cb < K16; cb += 64) {
        __m512 acc[4], corr[4];
        const int nv = (K16 - cb) >= 64 ? 4 : (int)((K16 - cb) / 16);
        for (int v = 0; v < 4; v++) { acc[v] = _mm512_setzero_ps(); corr[v] = _mm512_setzero_ps(); }
        for (uint32_t f = 0; f < D; f++) {
          const __m512 xv = _mm512_set1_ps(x[f]);
          const float *ct = CT + (size_t)f * K16 + cb;
          for (int v = 0; v < nv; v++) {
            const __m512 cv = _mm512_loadu_ps(ct + 16 * v);
            const __m512 y = _mm512_fmadd_round_ps(xv, cv, corr[v], RD);
            const __m512 t = _mm512_add_ps(acc[v], y);
            corr[v] = _mm512_sub_ps(y, _mm512_sub_ps(t, acc[v]));
            acc[v] = t;
          }
        }
        for (int v = 0; v < nv; v++) {
          float dist[16] __attribute__((aligned(64)));
          if (metric == KMO_L2) {
            const __m512 cs = _mm512_add_ps(_mm512_setzero_ps(), _mm512_loadu_ps(csqr16 + cb + 16 * v));
            _mm512_store_ps(dist, _mm512_fmadd_round_ps(_mm512_set1_ps(-2.f), acc[v], cs, RD));
          } else {
            float pr[16] __attribute__((aligned(64)));
            _mm512_store_ps(pr, acc[v]);
            for (int j = 0; j < 16; j++) dist[j] = cos_dist_from_prod(pr[j]);
          }
          for (int j = 0; j < 16; j++) {
            const uint32_t c = cb + 16 * v + j;
            if (c < K && dist[j] < min_dist) {
              min_dist = dist[j];
              nearest = c;
            }
          }
        }
      }
    }
    uint32_t ch = 0;
    lloyd_finish_row(s, insane, nearest, K, asg, prev, &ch);
    total += ch;
  }
  *changed += total;
}
#endif

/* kmeans.cu:293-364 with F = half2: products, csqr, distance and the running minimum are halves */
static void lloyd_assign_h2(int metric, uint32_t N, uint32_t D, uint32_t K, const float *X, const float *C,
                            uint32_t *asg, uint32_t *prev, uint32_t *changed) {
  float *sq = (float *)malloc(sizeof(float) * 2 * (size_t)K);
  for (uint32_t c = 0; c < K; c++) h2_sum_squares(metric, C + (size_t)c * D, D, &sq[2 * c], &sq[2 * c + 1]);
  uint32_t total = 0;
#pragma omp parallel for schedule(static) reduction(+ : total)
  for (uint32_t s = 0; s < N; s++) {
    const float *x = X + (size_t)s * D;
    const int insane = (x[0] != x[0]) || (x[1] != x[1]);   /* _neq(half2, half2) = !__hbeq2: either lane NaN */
    float min_dist = 65504.f;                               /* _fmax<half>() */
    uint32_t nearest = UINT32_MAX;
    if (!insane)
      for (uint32_t c = 0; c < K; c++) {
        float plo, phi;
        h2_dot(x, C + (size_t)c * D, D, &plo, &phi);
        const float dist = h2_distance3(metric, sq[2 * c], sq[2 * c + 1], plo, phi);
        if (dist < min_dist) { min_dist = dist; nearest = c; }   /* __hlt: false for NaN */
      }
    uint32_t ch = 0;
    lloyd_finish_row(s, insane, nearest, K, asg, prev, &ch);
    total += ch;
  }
  *changed += total;
  free(sq);
}

void kmo_lloyd_assign(int metric, uint32_t N, uint32_t D, uint32_t K, const float *samples,
                      const float *centroids, uint32_t *assignments, uint32_t *assignments_prev,
                      uint32_t *changed) {
  if (g_fp16_mode == 2) {
    lloyd_assign_h2(metric, N, D, K, samples, centroids, assignments, assignments_prev, changed);
    return;
  }
  float *csqr = (float *)malloc(sizeof(float) * (K + 64));
  kmo_sum_squares(metric, K, D, centroids, csqr);
#if defined(__x86_64__)
  if (kmo_have_avx512()) {
    const uint32_t K16 = (K + 15) / 16 * 16;
    float *CT = (float *)calloc((size_t)D * K16, sizeof(float));
    float *csqr16 = (float *)calloc(K16 + 64, sizeof(float));
    for (uint32_t c = 0; c < K; c++) {
      csqr16[c] = csqr[c];
      for (uint32_t f = 0; f < D; f++) CT[(size_t)f * K16 + c] = centroids[(size_t)c * D + f];
    }
    lloyd_assign_avx512(metric, N, D, K, samples, CT, K16, csqr16, assignments, assignments_prev, changed);
    free(CT);
    free(csqr16);
    free(csqr);
    return;
  }
#endif
  lloyd_assign_portable(metric, N, D, K, samples, centroids, csqr, assignments, assignments_prev, changed);
  free(csqr);
}

/* ------------------------------------------------------------------------------------ */
/* Centroid update, kmeans.cu:366-429                                                    */
/* ------------------------------------------------------------------------------------ */

void kmo_adjust(int metric, uint32_t N, uint32_t D, uint32_t K, const float *samples,
                const uint32_t *assignments_prev, const uint32_t *assignments,
                float *centroids, uint32_t *ccounts) {
  /* Per-centroid event lists (sample, sign) in ascending sample order == the serial scan of
   * kmeans.cu:389-424 restricted to the samples that touch this centroid. */
  uint32_t *cnt = (uint32_t *)calloc((size_t)K + 1, sizeof(uint32_t));
  for (uint32_t s = 0; s < N; s++) {
    const uint32_t p = assignments_prev[s], a = assignments[s];
    if (p == a) continue;
    if (p < K) cnt[p + 1]++;
    if (a < K) cnt[a + 1]++;
  }
  for (uint32_t c = 0; c < K; c++) cnt[c + 1] += cnt[c];
  const uint32_t total = cnt[K];
  uint32_t *ev = (uint32_t *)malloc(sizeof(uint32_t) * (total ? total : 1));
  int8_t *sg = (int8_t *)malloc(total ? total : 1);
  uint32_t *fill = (uint32_t *)malloc(sizeof(uint32_t) * K);
  memcpy(fill, cnt, sizeof(uint32_t) * K);
  for (uint32_t s = 0; s < N; s++) {
    const uint32_t p = assignments_prev[s], a = assignments[s];
    if (p == a) continue;
    if (p < K) { ev[fill[p]] = s; sg[fill[p]++] = -1; }
    if (a < K) { ev[fill[a]] = s; sg[fill[a]++] = 1; }
  }
#pragma omp parallel for schedule(dynamic, 4)
  for (uint32_t c = 0; c < K; c++) {
    float *cen = centroids + (size_t)c * D;
    uint32_t my_count = ccounts[c];
    if (g_fp16_mode == 2) {                                 /* kmeans.cu:366-429 with F = half2 */
      const float fmy = h_from_int_rd(my_count);            /* _const<half2>(my_count) = __int2half_rd */
      for (uint32_t f = 0; f < D; f++) cen[f] = h_mul(cen[f], fmy);
      float corr[2] = {0.f, 0.f};                           /* ONE half2 corr for all f and s: one per lane */
      for (uint32_t e = cnt[c]; e < cnt[c + 1]; e++) {
        const float *x = samples + (size_t)ev[e] * D;
        const float fsign = (float)sg[e];
        if (sg[e] < 0) my_count--; else my_count++;
        for (uint32_t f = 0; f + 1 < D; f += 2)
          for (int l = 0; l < 2; l++) {
            const float y = h_fma(x[f + l], fsign, corr[l]);
            const float t = h_add(cen[f + l], y);
            corr[l] = h_sub(y, h_sub(t, cen[f + l]));
            cen[f + l] = t;
          }
      }
      if (metric == KMO_L2) {                               /* metric_abstraction.h:138-144: h2rcp(_const(count)) */
        const float cnt_h = h_from_int_rd(my_count);
        const float rc = h_rn(1.0 / (double)cnt_h);
        for (uint32_t f = 0; f < D; f++) cen[f] = h_mul(cen[f], rc);
      } else {                                              /* :274-300: fp32 norm, HIGH half first, then low */
        float norm = 0.f, ncorr = 0.f;
        for (uint32_t f = 0; f + 1 < D; f += 2) {
          KAHAN_STEP(kmo_fma_rd, norm, ncorr, cen[f + 1], cen[f + 1]);
          KAHAN_STEP(kmo_fma_rd, norm, ncorr, cen[f], cen[f]);
        }
        norm = 1.0f / sqrtf(norm);
        const float norm2 = h_from_float(norm);
        for (uint32_t f = 0; f < D; f++) cen[f] = h_mul(cen[f], norm2);
      }
      ccounts[c] = my_count;
      continue;
    }
    const float fmy = (float)my_count;                      /* _const<F>(my_count) */
    for (uint32_t f = 0; f < D; f++) cen[f] = cen[f] * fmy; /* kmeans.cu:381-385 */
    float corr = 0.f;                                       /* ONE corr for all f and s, :388 */
    for (uint32_t e = cnt[c]; e < cnt[c + 1]; e++) {
      const float *x = samples + (size_t)ev[e] * D;
      const float fsign = (float)sg[e];
      if (sg[e] < 0) my_count--; else my_count++;
      for (uint32_t f = 0; f < D; f++) {
        const float y = kmo_fma_rd(x[f], fsign, corr);
        const float t = cen[f] + y;
        corr = y - (t - cen[f]);
        cen[f] = t;
      }
    }
    if (metric == KMO_L2) {                                 /* metric_abstraction.h:138-144 */
      const float rc = 1.0f / (float)my_count;
      for (uint32_t f = 0; f < D; f++) cen[f] = cen[f] * rc;
    } else {                                                /* metric_abstraction.h:255-272 */
      float norm = 0.f, ncorr = 0.f;
      for (uint32_t f = 0; f < D; f++) KAHAN_STEP(kmo_fma_rd, norm, ncorr, cen[f], cen[f]);
      norm = 1.0f / sqrtf(norm);
      for (uint32_t f = 0; f < D; f++) cen[f] = cen[f] * norm;
    }
    ccounts[c] = my_count;
  }
  free(cnt); free(ev); free(sg); free(fill);
}

/* ------------------------------------------------------------------------------------ */
/* Yinyang kernels, kmeans.cu:431-672.  bounds layout: bounds[(1+g)*N + s], bounds[s]=upper */
/* ------------------------------------------------------------------------------------ */

void kmo_yy_init(int metric, uint32_t N, uint32_t D, uint32_t K, uint32_t G, const float *samples,
                 const float *centroids, const uint32_t *assignments, const uint32_t *groups,
                 float *bounds) {
#pragma omp parallel for schedule(static)
  for (uint32_t s = 0; s < N; s++) {
    for (uint32_t i = 0; i < G + 1; i++) bounds[(size_t)N * i + s] = FLT_MAX;
    const uint32_t nearest = assignments[s];
    for (uint32_t c = 0; c < K; c++) {
      const uint32_t group = groups[c];
      if (group >= G) continue;                            /* NaN centroid, :468-471 */
      const float dist = kmo_distance(metric, samples + (size_t)s * D, centroids + (size_t)c * D, D);
      if (c != nearest) {
        const size_t gi = (size_t)N * (1 + group) + s;
        if (dist < bounds[gi]) bounds[gi] = dist;
      } else {
        bounds[s] = dist;
      }
    }
  }
}

void kmo_yy_calc_drifts(int metric, uint32_t D, uint32_t K, const float *centroids, float *drifts) {
  for (uint32_t c = 0; c < K; c++) {
    drifts[(size_t)K * D + c] = kmo_distance(metric, centroids + (size_t)c * D, drifts + (size_t)c * D, D);
  }
}

void kmo_yy_group_max_drifts(uint32_t D, uint32_t K, uint32_t G, const uint32_t *groups, float *drifts) {
  const size_t doffset = (size_t)K * D;
  float *gm = (float *)malloc(sizeof(float) * (G ? G : 1));
  for (uint32_t g = 0; g < G; g++) {
    float my_max = -FLT_MAX;
    for (uint32_t c = 0; c < K; c++) {
      if (groups[c] == g) {
        const float d = drifts[doffset + c];
        if (my_max < d) my_max = d;
      }
    }
    gm[g] = my_max;
  }
  for (uint32_t g = 0; g < G; g++) drifts[g] = gm[g];      /* overlays old centroids, :537 */
  free(gm);
}

uint32_t kmo_yy_global_filter(int metric, uint32_t N, uint32_t D, uint32_t K, uint32_t G,
                              const float *samples, const float *centroids, const uint32_t *groups,
                              const float *drifts, const uint32_t *assignments,
                              uint32_t *assignments_prev, float *bounds, uint32_t *passed) {
  (void)groups;
  const size_t doffset = (size_t)K * D;
  uint8_t *flag = (uint8_t *)calloc(N ? N : 1, 1);
#pragma omp parallel for schedule(static)
  for (uint32_t s = 0; s < N; s++) {
    const uint32_t cluster = assignments[s];
    assignments_prev[s] = cluster;
    float upper_bound = bounds[s];
    const float cluster_drift = drifts[doffset + cluster];
    upper_bound += cluster_drift;
    float min_lower_bound = FLT_MAX;
    for (uint32_t g = 0; g < G; g++) {
      const size_t gi = (size_t)N * (1 + g) + s;
      const float lower_bound = bounds[gi] - drifts[g];
      bounds[gi] = lower_bound;
      if (lower_bound < min_lower_bound) min_lower_bound = lower_bound;
    }
    if (min_lower_bound >= upper_bound) {                  /* group filter try #1 */
      bounds[s] = upper_bound;
      continue;
    }
    upper_bound = kmo_distance(metric, samples + (size_t)s * D, centroids + (size_t)cluster * D, D);
    bounds[s] = upper_bound;
    if (min_lower_bound >= upper_bound) continue;          /* try #2 */
    flag[s] = 1;
  }
  /* The reference appends with a warp-aggregated atomic (order nondeterministic); the passed
   * list is a set as far as results go (every entry is processed independently). */
  uint32_t np = 0;
  for (uint32_t s = 0; s < N; s++) if (flag[s]) passed[np++] = s;
  free(flag);
  return np;
}

uint32_t kmo_yy_local_filter(int metric, uint32_t N, uint32_t D, uint32_t K, uint32_t G,
                             const float *samples, const uint32_t *passed, uint32_t npassed,
                             const float *centroids, const uint32_t *groups, const float *drifts,
                             uint32_t *assignments, float *bounds) {
  const size_t doffset = (size_t)K * D;
  uint32_t changed = 0;
#pragma omp parallel for schedule(dynamic, 64) reduction(+ : changed)
  for (uint32_t pi = 0; pi < npassed; pi++) {
    const uint32_t s = passed[pi];
    const float upper_bound = bounds[s];
    const uint32_t cluster = assignments[s];
    float min_dist = upper_bound, second_min_dist = FLT_MAX;
    uint32_t nearest = cluster;
    for (uint32_t c = 0; c < K; c++) {
      if (c == cluster) continue;
      const uint32_t group = groups[c];
      if (group >= G) continue;
      float lower_bound = bounds[(size_t)N * (1 + group) + s];
      if (lower_bound >= upper_bound) {
        if (lower_bound < second_min_dist) second_min_dist = lower_bound;
        continue;
      }
      lower_bound += drifts[group] - drifts[doffset + c];
      if (second_min_dist < lower_bound) continue;
      const float dist = kmo_distance(metric, samples + (size_t)s * D, centroids + (size_t)c * D, D);
      if (dist < min_dist) {
        second_min_dist = min_dist;
        min_dist = dist;
        nearest = c;
      } else if (dist < second_min_dist) {
        second_min_dist = dist;
      }
    }
    const uint32_t nearest_group = groups[nearest];
    const uint32_t previous_group = groups[cluster];
    bounds[(size_t)N * (1 + nearest_group) + s] = second_min_dist;
    if (nearest_group != previous_group) {
      const size_t gi = (size_t)N * (1 + previous_group) + s;
      const float pb = bounds[gi];
      if (pb > upper_bound) bounds[gi] = upper_bound;
    }
    bounds[s] = min_dist;
    if (cluster != nearest) {
      assignments[s] = nearest;
      changed++;
    }
  }
  return changed;
}

/* ------------------------------------------------------------------------------------ */
/* Seeding, kmcuda.cc:222-336 + kmeans.cu:42-67,774-828                                  */
/* ------------------------------------------------------------------------------------ */

/* kmeans.cu:42-67: one k-means++ step; returns the sum as the reference forms it:
 * float butterfly (shfl_down 16..1) over each aligned group of 32 samples, then a double
 * accumulation of the per-warp sums (atomicAdd on double; order-insensitive to ~1e-16). */
static double kmpp_step(int metric, uint32_t N, uint32_t D, uint32_t cc, const float *samples,
                        const float *centroid, float *dists) {
#pragma omp parallel for schedule(static)
  for (uint32_t s = 0; s < N; s++) {
    const float *x = samples + (size_t)s * D;
    float dist = 0.f;
    if (x[0] == x[0] && (g_fp16_mode != 2 || x[1] == x[1])) dist = kmo_distance(metric, x, centroid, D);
    if (cc == 1 || dist < dists[s]) dists[s] = dist;
  }
  double sum = 0.0;
  for (uint32_t base = 0; base < N; base += 32) {
    float lane[32];
    for (int l = 0; l < 32; l++) lane[l] = (base + l < N) ? dists[base + l] : 0.f;
    for (int off = 16; off > 0; off /= 2)
      for (int l = 0; l < 32; l++)                 /* val += shfl_down(val, off) */
        lane[l] = lane[l] + ((l + off < 32) ? lane[l + off] : lane[l]);
    sum += (double)lane[0];
  }
  return sum;
}

/* ------------------------------------------------------------------------------------ */
/* AFK-MC2 seeding: kmeans.cu:69-212 (kernels), kmcuda.cc:337-396 (host chain).            */
/* Third-party arithmetic: the reference draws from cuRAND's XORWOW (CUDA toolkit 8.0,    */
/* curand_init(seed, thread, step) + curand_uniform), which is not in /root/reference.    */
/* Restated from the published algorithm, piece by piece:                                 */
/*  - the generator: Marsaglia's xorwow (5 x 32-bit xorshift + a Weyl sequence, increment */
/*    362437), output d + x[4] -- the same lines in curand_kernel.h and rocrand_xorwow.h;  */
/*  - skipping: subsequence = 2^67 draws, offset = single draws, both as powers of the    */
/*    recurrence's matrix (a property of the recurrence, not of a library); the powers    */
/*    come from the system header rocrand_xorwow_precomputed.h; the Weyl value moves by   */
/*    offset * 362437;                                                                    */
/*  - the SEED SCRAMBLING is where the two libraries differ: cuRAND (curand_kernel.h,     */
/*    _curand_init_scratch, as the builder knows it -- not verifiable offline) salts the  */
/*    seed's halves with 0xaad26b49 / 0xf7dcefdd and multiplies by 1099087573 /           */
/*    2591861531; rocRAND's xorwow_engine uses 0x2c7f967f / 0xa03697cb and 1228688033 /   */
/*    2073658381.  The reference's only anchors for this init are four iteration counts   */
/*    (test.py:248-289, :499-509): rocRAND's seeding (flavour 0) meets all four, the      */
/*    quoted cuRAND constants (flavour 1) three -- the half2 run takes 5; an arbitrary    */
/*    stream gives 4 iterations with probability ~0.6, so neither proves a stream.        */
/*    DEFAULT: flavour 0, the one that meets every pin the reference holds;               */
/*    kmo_set_afkmc2_seeding(1) / KMCUDA_AMD_AFKMC2_SEEDING=curand (product) the other;   */
/*  - cuRAND's uint -> (0,1] map x * 2^-32 + 2^-33.                                        */
/* Everything but the constants is checked against a second implementation (rocRAND's     */
/* host generator, tests/test_gpu_afkmc2_rng.py).  PARITY UNPINNED beyond the pins.        */
/* ------------------------------------------------------------------------------------ */
#define __device__
#include <rocrand/rocrand_xorwow_precomputed.h>
#undef __device__

typedef struct { uint32_t x[5]; uint32_t d; } xorwow_t;

static void xorwow_mul(const unsigned int *m, uint32_t *v) {
  uint32_t r[XORWOW_N] = {0, 0, 0, 0, 0};
  for (int i = 0; i < XORWOW_N; i++)
    for (int j = 0; j < XORWOW_M; j++)
      if (v[i] & (1u << j))
        for (int k = 0; k < XORWOW_N; k++) r[k] ^= m[i * XORWOW_M * XORWOW_N + j * XORWOW_N + k];
  for (int k = 0; k < XORWOW_N; k++) v[k] = r[k];
}

static void xorwow_jump(xorwow_t *st, unsigned long long v, const unsigned int mats[XORWOW_JUMP_MATRICES][XORWOW_SIZE]) {
  unsigned mi = 0;
  while (v > 0) {
    const unsigned is = (unsigned)v & ((1u << XORWOW_JUMP_LOG2) - 1u);
    for (unsigned i = 0; i < is; i++) xorwow_mul(mats[mi], st->x);
    mi++;
    v >>= XORWOW_JUMP_LOG2;
  }
}

static void xorwow_init_flavour(xorwow_t *st, int curand_seeding, unsigned long long seed, unsigned long long subsequence,
                                unsigned long long offset) {
  st->x[0] = 123456789u; st->x[1] = 362436069u; st->x[2] = 521288629u; st->x[3] = 88675123u; st->x[4] = 5783321u;
  st->d = 6615241u;
  const uint32_t s0 = (uint32_t)seed ^ (curand_seeding ? 0xaad26b49u : 0x2c7f967fu);
  const uint32_t s1 = (uint32_t)(seed >> 32) ^ (curand_seeding ? 0xf7dcefddu : 0xa03697cbu);
  const uint32_t t0 = (curand_seeding ? 1099087573u : 1228688033u) * s0, t1 = (curand_seeding ? 2591861531u : 2073658381u) * s1;
  st->x[0] += t0; st->x[1] ^= t0; st->x[2] += t1; st->x[3] ^= t1; st->x[4] += t0;
  st->d += t1 + t0;
  xorwow_jump(st, subsequence, h_xorwow_sequence_jump_matrices);
  xorwow_jump(st, offset, h_xorwow_jump_matrices);
  st->d += (uint32_t)offset * 362437u;
}

static int g_afk_curand_seeding = 0;
void kmo_set_afkmc2_seeding(int curand) { g_afk_curand_seeding = curand != 0; }
static void xorwow_init(xorwow_t *st, unsigned long long seed, unsigned long long subsequence, unsigned long long offset) {
  xorwow_init_flavour(st, g_afk_curand_seeding, seed, subsequence, offset);
}

static uint32_t xorwow_next(xorwow_t *st) {
  const uint32_t t = st->x[0] ^ (st->x[0] >> 2);
  st->x[0] = st->x[1]; st->x[1] = st->x[2]; st->x[2] = st->x[3]; st->x[3] = st->x[4];
  st->x[4] = (st->x[4] ^ (st->x[4] << 4)) ^ (t ^ (t << 1));
  st->d += 362437u;
  return st->d + st->x[4];
}

/* n raw draws of the stream (seed, subsequence, offset) -- the tests' window on the restatement */
void kmo_xorwow_draws(int curand_seeding, unsigned long long seed, unsigned long long subsequence,
                      unsigned long long offset, uint32_t n, uint32_t *out) {
  xorwow_t st;
  xorwow_init_flavour(&st, curand_seeding, seed, subsequence, offset);
  for (uint32_t i = 0; i < n; i++) out[i] = xorwow_next(&st);
}

static float afk_uniform(uint32_t x) { return fmaf((float)x, 2.3283064e-10f, 2.3283064e-10f / 2.0f); }

static uint32_t g_afk_m = 0;
void kmo_set_afkmc2_m(uint32_t m) { g_afk_m = m; }

static int afkmc2_init(int metric, uint32_t N, uint32_t D, uint32_t K, uint32_t seed, uint32_t m,
                       const float *samples, float *centroids) {
  if (m == 0) m = 200;
  else if (m > N / 2) return 1;
  uint32_t first_index;
  float smoke = NAN;
  while (smoke != smoke) {
    first_index = (uint32_t)(rand() % (long)N);
    smoke = samples[(size_t)first_index * D];
  }
  memcpy(centroids, samples + (size_t)first_index * D, sizeof(float) * D);
  /* q relative to sample (first_index / D) -- the reference's quirk, kmcuda.cc:356-362 */
  const float *c1 = samples + (size_t)(first_index / D) * D;
  float *q = (float *)malloc(sizeof(float) * N);
  for (uint32_t s = 0; s < N; s++) {
    const float d = kmo_distance(metric, samples + (size_t)s * D, c1, D);
    q[s] = d * d;
  }
  double dsum = 0.0;                                   /* warp butterfly sums of 32, double accumulation */
  for (uint32_t base = 0; base < N; base += 32) {
    float lane[32];
    for (int l = 0; l < 32; l++) lane[l] = (base + l < N) ? q[base + l] : 0.f;
    for (int off = 16; off > 0; off /= 2)
      for (int l = 0; l < 32; l++) lane[l] = lane[l] + ((l + off < 32) ? lane[l + off] : lane[l]);
    dsum += (double)lane[0];
  }
  const float dsumf = (float)dsum;
  for (uint32_t s = 0; s < N; s++) q[s] = 1 / (2.f * N) + q[s] / (2 * dsumf);     /* kmeans.cu:108 */
  uint32_t *cand = (uint32_t *)calloc(m, sizeof(uint32_t));
  float *rand_a = (float *)malloc(sizeof(float) * m), *p_cand = (float *)malloc(sizeof(float) * m);
  for (uint32_t k = 1; k < K; k++) {
    for (uint32_t ti = 0; ti < m; ti++) {                                            /* kmeans.cu:111-164 */
      xorwow_t st;
      xorwow_init(&st, seed, ti, k);
      const float part = afk_uniform(xorwow_next(&st));
      rand_a[ti] = afk_uniform(xorwow_next(&st));
      float accum = 0.f, corr = 0.f;
      uint32_t i = 0;
      for (; i < N && accum < part; i++) {
        const float y = corr + q[i];
        const float t = accum + y;
        corr = y - (t - accum);
        accum = t;
      }
      if (accum >= part) cand[ti] = i - 1;
    }
    for (uint32_t chi = 0; chi < m; chi++) {                                         /* kmeans.cu:166-183 */
      float min_dist = FLT_MAX;
      for (uint32_t c = 0; c < k; c++) {
        const float dist = kmo_distance(metric, samples + (size_t)cand[chi] * D, centroids + (size_t)c * D, D);
        if (dist < min_dist) min_dist = dist;
      }
      p_cand[chi] = min_dist * min_dist;
    }
    float curr_prob = 0;                                                             /* kmcuda.cc:381-388 */
    uint32_t curr_ind = 0;
    for (uint32_t j = 0; j < m; j++) {
      const float cand_prob = p_cand[j] / q[cand[j]];
      if (curr_prob == 0 || cand_prob / curr_prob > rand_a[j]) {
        curr_ind = j;
        curr_prob = cand_prob;
      }
    }
    memcpy(centroids + (size_t)k * D, samples + (size_t)cand[curr_ind] * D, sizeof(float) * D);
  }
  free(q); free(cand); free(rand_a); free(p_cand);
  return 0;
}

int kmo_init_centroids(int method, int metric, uint32_t N, uint32_t D, uint32_t K, uint32_t seed,
                       const float *samples, float *centroids) {
  srand(seed);                                               /* kmcuda.cc:222 */
  if (method == KMO_INIT_IMPORT) return 0;
  if (method == KMO_INIT_RANDOM) {                           /* kmcuda.cc:245-261 */
    uint32_t *chosen = (uint32_t *)malloc(sizeof(uint32_t) * N);
    for (uint32_t s = 0; s < N; s++) chosen[s] = s;
    /* libstdc++ std::random_shuffle(first,last): for i=1..N-1: swap(a[i], a[rand() % (i+1)]) */
    for (uint32_t i = 1; i < N; i++) {
      const uint32_t j = (uint32_t)(rand() % (long)(i + 1));
      const uint32_t tmp = chosen[i]; chosen[i] = chosen[j]; chosen[j] = tmp;
    }
    for (uint32_t c = 0; c < K; c++)
      memcpy(centroids + (size_t)c * D, samples + (size_t)chosen[c] * D, sizeof(float) * D);
    free(chosen);
    return 0;
  }
  if (method == KMO_INIT_PLUSPLUS) {                         /* kmcuda.cc:262-336 */
    uint32_t first_index;
    float smoke = NAN;
    while (smoke != smoke) {
      first_index = (uint32_t)(rand() % (long)N);
      smoke = samples[(size_t)first_index * D];              /* feature 0 of that sample */
    }
    memcpy(centroids, samples + (size_t)first_index * D, sizeof(float) * D);
    float *host_dists = (float *)malloc(sizeof(float) * N);
    for (uint32_t i = 1; i < K; i++) {
      const double dist_sum = kmpp_step(metric, N, D, i, samples, centroids + (size_t)(i - 1) * D, host_dists);
      const double choice = ((rand() + .0) / RAND_MAX);
      const uint32_t choice_approx = (uint32_t)(choice * N);
      const double choice_sum = choice * dist_sum;
      uint32_t j;
      if (choice_approx < 100) {
        double dist_sum2 = 0;
        for (j = 0; j < N && dist_sum2 < choice_sum; j++) dist_sum2 += host_dists[j];
      } else {
        double dist_sum2 = 0;
        for (uint32_t t = 0; t < choice_approx; t++) dist_sum2 += host_dists[t];
        if (dist_sum2 < choice_sum) {
          for (j = choice_approx; j < N && dist_sum2 < choice_sum; j++) dist_sum2 += host_dists[j];
        } else {
          for (j = choice_approx; j > 1 && dist_sum2 >= choice_sum; j--) dist_sum2 -= host_dists[j];
          j++;
        }
      }
      if (j == 0 || j > N) { free(host_dists); return 2; }
      memcpy(centroids + (size_t)i * D, samples + (size_t)(j - 1) * D, sizeof(float) * D);
    }
    free(host_dists);
    return 0;
  }
  if (method == KMO_INIT_AFKMC2) return afkmc2_init(metric, N, D, K, seed, g_afk_m, samples, centroids);
  return 3;
}

/* kmeans.cu:674-691: float warp butterfly sums, double accumulation, / N */
float kmo_average_distance(int metric, uint32_t N, uint32_t D, const float *samples,
                           const float *centroids, const uint32_t *assignments) {
  float *d = (float *)malloc(sizeof(float) * (N ? N : 1));
#pragma omp parallel for schedule(static)
  for (uint32_t s = 0; s < N; s++)
    d[s] = kmo_distance(metric, samples + (size_t)s * D, centroids + (size_t)assignments[s] * D, D);
  double sum = 0.0;
  for (uint32_t base = 0; base < N; base += 32) {
    float lane[32];
    for (int l = 0; l < 32; l++) lane[l] = (base + l < N) ? d[base + l] : 0.f;
    for (int off = 16; off > 0; off /= 2)
      for (int l = 0; l < 32; l++) lane[l] = lane[l] + ((l + off < 32) ? lane[l + off] : lane[l]);
    sum += (double)lane[0];
  }
  free(d);
  return (float)(sum / N);
}

/* ------------------------------------------------------------------------------------ */
/* Drivers, kmeans.cu:934-1263                                                           */
/* ------------------------------------------------------------------------------------ */

typedef struct {
  uint32_t *log; uint32_t cap; uint32_t n;
} iterlog_t;

static void log_iter(iterlog_t *L, uint32_t changed) {
  if (L && L->log && L->n < L->cap) L->log[L->n] = changed;
  if (L) L->n++;
}

/* kmeans.cu:697-717: returns 1 to stop */
static int check_changed(float tolerance, uint32_t N, uint32_t *changed, iterlog_t *L, int print) {
  if (print) log_iter(L, *changed);
  if (*changed <= tolerance * N) return 1;     /* float * uint32 in float, :707; NOT zeroed */
  *changed = 0;
  return 0;
}

/* fp16x2 storage mode (fp_abstraction.h:100-182 keeps centroids in half2): this repository's fp16
 * semantics are "the fp32 arithmetic on the half values, centroids rounded to half (RN) after every
 * update"  -- NOT the reference's half2 accumulation, which is tolerance-only. */
#define g_fp16_storage (g_fp16_mode == 1)
void kmo_set_fp16_storage(int on) { g_fp16_mode = on ? 1 : 0; }
/* 0 fp32, 1 storage semantics, 2 the reference's half2 arithmetic (inputs must hold half values, D even) */
void kmo_set_fp16_mode(int mode) { g_fp16_mode = mode; }
float kmo_h_rn(double v) { return h_rn(v); }
float kmo_h_from_int_rd(long long v) { return h_from_int_rd(v); }

/* round-to-nearest-even float -> IEEE half -> float */
float kmo_quantize_half(float x) {
  union { float f; uint32_t u; } v = { x };
  const uint32_t sign = v.u & 0x80000000u;
  uint32_t a = v.u & 0x7FFFFFFFu;
  if (a >= 0x7F800000u) return x;                          /* inf / NaN */
  if (a >= 0x477FF000u) {                                   /* >= 65520: rounds to inf */
    v.u = sign | 0x7F800000u; return v.f;
  }
  if (a < 0x33000001u) { v.u = sign; return v.f; }          /* < 2^-25 (or == 2^-25: ties to even 0) */
  int e = (int)(a >> 23) - 127;
  int drop = e >= -14 ? 13 : (13 + (-14 - e));              /* mantissa bits to drop (subnormal halves) */
  uint32_t m = (a & 0x007FFFFFu) | 0x00800000u;             /* 24-bit significand */
  if (drop >= 25) { v.u = sign; return v.f; }
  const uint32_t half_ulp = 1u << (drop - 1), mask = (1u << drop) - 1u;
  uint32_t r = m & mask;
  m >>= drop;
  if (r > half_ulp || (r == half_ulp && (m & 1u))) m++;
  /* rebuild: value = m * 2^(e - 23 + drop) */
  double val = (double)m * ldexp(1.0, e - 23 + drop);
  float out = (float)val;                                    /* exact: m has <= 12 significant bits */
  v.f = out; v.u |= sign; return v.f;
}

static void quantize_centroids(float *c, size_t n) {
  if (!g_fp16_storage) return;
  for (size_t i = 0; i < n; i++) c[i] = kmo_quantize_half(c[i]);
}

/* kmeans.cu:934-1026 */
static int lloyd_loop(float tolerance, int metric, uint32_t N, uint32_t D, uint32_t K, int resume,
                      const float *samples, float *centroids, uint32_t *ccounts, uint32_t *prev,
                      uint32_t *asg, uint32_t *changed, iterlog_t *L) {
  *changed = 0;                                 /* prepare_mem, :719-746 */
  if (!resume) {
    memset(ccounts, 0, sizeof(uint32_t) * K);
    memset(asg, 0xff, sizeof(uint32_t) * N);
    memset(prev, 0xff, sizeof(uint32_t) * N);
  }
  for (int iter = 1;; iter++) {
    if (!resume || iter > 1) {
      kmo_lloyd_assign(metric, N, D, K, samples, centroids, asg, prev, changed);
      if (check_changed(tolerance, N, changed, L, 1)) return iter;
    }
    kmo_adjust(metric, N, D, K, samples, prev, asg, centroids, ccounts);
    quantize_centroids(centroids, (size_t)K * D);
  }
}

int kmo_kmeans(int init, float tolerance, float yinyang_t, int metric, uint32_t N, uint32_t D,
               uint32_t K, uint32_t seed, const float *samples, float *centroids,
               uint32_t *assignments, float *average_distance,
               uint32_t *iter_log, uint32_t iter_log_cap, uint32_t *n_iter_log) {
  /* kmcuda.cc:19-61 */
  if (K < 2 || K == UINT32_MAX || D == 0 || N < K) return 1;
  if (!samples || !centroids || !assignments) return 1;
  if (tolerance < 0 || tolerance > 1) return 1;
  if (yinyang_t < 0 || yinyang_t > 0.5) return 1;
  iterlog_t L = {iter_log, iter_log_cap, 0};
  const uint32_t G = (uint32_t)(yinyang_t * K);             /* kmcuda.cc:417, float product */
  uint32_t *prev = (uint32_t *)malloc(sizeof(uint32_t) * N);
  uint32_t *ccounts = (uint32_t *)malloc(sizeof(uint32_t) * K);
  uint32_t changed = 0;
  int rc = kmo_init_centroids(init, metric, N, D, K, seed, samples, centroids);
  if (rc) { free(prev); free(ccounts); return rc; }

  if (G == 0 || 0.11 <= tolerance) {                         /* kmeans.cu:1037-1050 */
    lloyd_loop(tolerance, metric, N, D, K, 0, samples, centroids, ccounts, prev, assignments, &changed, &L);
  } else {
    int iter = lloyd_loop(0.11f, metric, N, D, K, 0, samples, centroids, ccounts, prev, assignments,
                          &changed, &L);                     /* :1054-1057 */
    if (!check_changed(tolerance, N, &changed, &L, 0)) {     /* :1058 */
      /* groups: k-means++(seed 0) + Lloyd(tol .02) on the centroids themselves, :1062-1100 */
      uint32_t *groups = (uint32_t *)malloc(sizeof(uint32_t) * K);
      float *cyy = (float *)malloc(sizeof(float) * (size_t)G * D);
      {
        uint32_t *gprev = (uint32_t *)malloc(sizeof(uint32_t) * K);
        uint32_t *gcnt = (uint32_t *)malloc(sizeof(uint32_t) * G);
        uint32_t gchanged = 0;
        kmo_init_centroids(KMO_INIT_PLUSPLUS, metric, K, D, G, 0, centroids, cyy);
        lloyd_loop(0.02f, metric, K, D, G, 0, centroids, cyy, gcnt, gprev, groups, &gchanged, &L);
        free(gprev); free(gcnt);
      }
      float *bounds = (float *)malloc(sizeof(float) * (size_t)N * (G + 1));
      float *drifts = (float *)malloc(sizeof(float) * ((size_t)K * D + K));
      uint32_t *passed = (uint32_t *)malloc(sizeof(uint32_t) * N);
      changed = 0;                                           /* prepare_mem(resume=true) */
      int refresh = 1;
      uint32_t npassed = 0;
      for (;; iter++) {                                      /* :1119-1262 */
        if (!refresh) {
          if (check_changed(tolerance, N, &changed, &L, 1)) break;
          if (1.f - (npassed + 0.f) / N < 1e-4) refresh = 1; /* YINYANG_REFRESH_EPSILON, :1136 */
        }
        if (refresh) {
          kmo_yy_init(metric, N, D, K, G, samples, centroids, assignments, groups, bounds);
          refresh = 0;
        }
        memcpy(drifts, centroids, sizeof(float) * (size_t)K * D);
        kmo_adjust(metric, N, D, K, samples, prev, assignments, centroids, ccounts);
        quantize_centroids(centroids, (size_t)K * D);
        kmo_yy_calc_drifts(metric, D, K, centroids, drifts);
        kmo_yy_group_max_drifts(D, K, G, groups, drifts);
        npassed = kmo_yy_global_filter(metric, N, D, K, G, samples, centroids, groups, drifts,
                                       assignments, prev, bounds, passed);
        changed += kmo_yy_local_filter(metric, N, D, K, G, samples, passed, npassed, centroids,
                                       groups, drifts, assignments, bounds);
      }
      free(groups); free(cyy); free(bounds); free(drifts); free(passed);
    }
  }
  if (average_distance)
    *average_distance = kmo_average_distance(metric, N, D, samples, centroids, assignments);
  if (n_iter_log) *n_iter_log = L.n;
  free(prev); free(ccounts);
  return 0;
}

/* ------------------------------------------------------------------------------------ */
/* k-NN, knn.cu + kmcuda.cc:648-691                                                      */
/* ------------------------------------------------------------------------------------ */

/* kmcuda.cc:648-691: std::sort of (cluster, index) tuples => members ascending by index;
 * offsets[c] .. offsets[c+1].  Assignments >= K (NaN samples) sort last and are dropped by
 * the offsets construction (offsets[K] = first index with cluster >= K ... the reference sets
 * offsets[icls]=s for icls<=newcls<=K only when newcls<=K; with newcls==K offsets[K]=s). */
void kmo_knn_inverse(uint32_t N, uint32_t K, const uint32_t *assignments, uint32_t *inv, uint32_t *offsets) {
  uint32_t *cnt = (uint32_t *)calloc((size_t)K + 2, sizeof(uint32_t));
  for (uint32_t s = 0; s < N; s++) { const uint32_t a = assignments[s] < K ? assignments[s] : K; cnt[a + 1]++; }
  for (uint32_t c = 0; c <= K; c++) cnt[c + 1] += cnt[c];
  for (uint32_t c = 0; c <= K; c++) offsets[c] = cnt[c];
  uint32_t *fill = (uint32_t *)malloc(sizeof(uint32_t) * (K + 1));
  memcpy(fill, cnt, sizeof(uint32_t) * (K + 1));
  for (uint32_t s = 0; s < N; s++) { const uint32_t a = assignments[s] < K ? assignments[s] : K; inv[fill[a]++] = s; }
  free(cnt); free(fill);
}

/* metric_abstraction.h:103-136 / :220-253: partial / finalize */
static float knn_partial(int metric, const float *a, const float *b, uint32_t n) {
  if (g_fp16_mode == 2) {                             /* F = half2: two interleaved half sums, _float(_fin(.)) */
    float s[2] = {0.f, 0.f}, c[2] = {0.f, 0.f};
    for (uint32_t f = 0; f + 1 < n; f += 2)
      for (int l = 0; l < 2; l++) {
        if (metric == KMO_L2) { const float d = h_sub(a[f + l], b[f + l]); H2_KAHAN(s[l], c[l], d, d); }
        else H2_KAHAN(s[l], c[l], a[f + l], b[f + l]);
      }
    return h_add(s[1], s[0]);
  }
  if (metric == KMO_L2) return kahan_sqdiff(a, b, n);
  return kmo_kahan_dot(a, b, n);
}
static float knn_finalize(int metric, float p) {
  if (metric == KMO_L2) return sqrtf(p);
  return cos_dist_from_prod(p);
}

/* knn.cu:19-58: chunks of cent_step=min(8192/512, D) features, sample_dists += partial */
void kmo_knn_radiuses(int metric, uint32_t N, uint32_t D, uint32_t K, const float *samples,
                      const float *centroids, const uint32_t *inv, const uint32_t *offsets, float *radiuses) {
  (void)N;
  /* 16 elements of F: with F = half2 (D counts halves here) that is 32 halves */
  const uint32_t fstep16 = g_fp16_mode == 2 ? 32 : 16;
  const uint32_t cent_step = D < fstep16 ? D : fstep16;
#pragma omp parallel for schedule(dynamic, 4)
  for (uint32_t ci = 0; ci < K; ci++) {
    float max_dist = -1.f;
    for (uint32_t a = offsets[ci]; a < offsets[ci + 1]; a++) {
      const float *x = samples + (size_t)inv[a] * D;
      float sd = 0.f;
      for (uint32_t cfi = 0; cfi < D; cfi += cent_step) {
        const uint32_t fsize = (D - cfi) < cent_step ? (D - cfi) : cent_step;
        sd += knn_partial(metric, x + cfi, centroids + (size_t)ci * D + cfi, fsize);
      }
      const float dist = knn_finalize(metric, sd);
      if (dist > max_dist) max_dist = dist;
    }
    radiuses[ci] = max_dist > -1.f ? max_dist : NAN;
  }
}

/* knn.cu:61-131: fstep = 12288/512 = 24-feature chunks, distances += partial; finalize; mirror */
void kmo_knn_cluster_distances(int metric, uint32_t D, uint32_t K, const float *centroids, float *dists) {
  const uint32_t fstep = g_fp16_mode == 2 ? 48 : 24;   /* 24 elements of F */
#pragma omp parallel for schedule(static)
  for (uint32_t i = 0; i < K; i++) {
    for (uint32_t j = 0; j < K; j++) {
      float acc = 0.f;
      for (uint32_t fpos = 0; fpos < D; fpos += fstep) {
        const uint32_t fsize = (D - fpos) < fstep ? (D - fpos) : fstep;
        acc += knn_partial(metric, centroids + (size_t)i * D + fpos, centroids + (size_t)j * D + fpos, fsize);
      }
      dists[(size_t)i * K + j] = knn_finalize(metric, acc);
    }
  }
}

/* knn.cu:133-175 */
static void push_sample(uint32_t k, float dist, uint32_t index, float *heap) {
  uint32_t pos = 0;
  uint32_t *heapi = (uint32_t *)heap;
  for (;;) {
    float left = 0, right = 0;
    int left_le, right_le;
    if ((2 * pos + 1) < k) { left = heap[4 * pos + 2]; left_le = dist >= left; } else left_le = 1;
    if ((2 * pos + 2) < k) { right = heap[4 * pos + 4]; right_le = dist >= right; } else right_le = 1;
    if (left_le && right_le) {
      heap[2 * pos] = dist;
      heapi[2 * pos + 1] = index;
      break;
    }
    if (!left_le && !right_le) {
      if (left <= right) {
        heap[2 * pos] = right; heapi[2 * pos + 1] = heapi[4 * pos + 5]; pos = 2 * pos + 2;
      } else {
        heap[2 * pos] = left; heapi[2 * pos + 1] = heapi[4 * pos + 3]; pos = 2 * pos + 1;
      }
    } else if (left_le) {
      heap[2 * pos] = right; heapi[2 * pos + 1] = heapi[4 * pos + 5]; pos = 2 * pos + 2;
    } else {
      heap[2 * pos] = left; heapi[2 * pos + 1] = heapi[4 * pos + 3]; pos = 2 * pos + 1;
    }
  }
}

/* knn.cu:177-243 (knn_assign_shmem; the gmem variant yields the same list): the search of ONE row x of cluster mycls.
 * self = the row's own corpus index, skipped in its cluster (knn.cu:204-206), or UINT32_MAX for a row that is not in
 * the corpus (a query: nothing is skipped).  heap: 2k floats of scratch.  distances may be NULL.  Returns the number of
 * candidates of the clusters it visited (the reference's dists_calced). */
static uint64_t knn_search_row(uint32_t k, int metric, uint32_t D, uint32_t K, const float *samples,
                               const float *centroids, const float *x, uint32_t mycls, uint32_t self,
                               const uint32_t *inv, const uint32_t *offsets, const float *radiuses, const float *cdist,
                               float *heap, uint32_t *neighbors, float *distances) {
  uint64_t calced = 0;
  const float mydist = kmo_distance(metric, x, centroids + (size_t)mycls * D, D);
  float mndist = FLT_MAX;
  for (uint32_t i = 0; i < k; i++) { heap[2 * i] = FLT_MAX; ((uint32_t *)heap)[2 * i + 1] = 0; }
  calced += offsets[mycls + 1] - offsets[mycls];
  for (uint32_t pos = offsets[mycls]; pos < offsets[mycls + 1]; pos++) {
    const uint32_t other = inv[pos];
    if (other == self) continue;
    const float dist = kmo_distance(metric, x, samples + (size_t)other * D, D);
    if (dist <= mndist) { push_sample(k, dist, other, heap); mndist = heap[0]; }
  }
  for (uint32_t cls = 0; cls < K; cls++) {
    if (cls == mycls) continue;
    const float cd = cdist[(size_t)cls * K + mycls];
    if (cd != cd) continue;
    const float lim = cd - mydist - radiuses[cls];
    if (lim > mndist) continue;
    calced += offsets[cls + 1] - offsets[cls];
    for (uint32_t pos = offsets[cls]; pos < offsets[cls + 1]; pos++) {
      const uint32_t other = inv[pos];
      const float dist = kmo_distance(metric, x, samples + (size_t)other * D, D);
      if (dist <= mndist) { push_sample(k, dist, other, heap); mndist = heap[0]; }
    }
  }
  for (int i = (int)k - 1; i >= 0; i--) {
    neighbors[i] = ((uint32_t *)heap)[1];
    if (distances) distances[i] = heap[0];
    push_sample(k, -1.f, UINT32_MAX, heap);
  }
  return calced;
}

/* The corpus side of a search: CSR, radii, centroid distances (kmcuda.cc:648-691, knn.cu:19-131) */
typedef struct { uint32_t *inv, *offsets; float *radiuses, *cdist; } knn_corpus_t;
static void knn_corpus_init(knn_corpus_t *p, int metric, uint32_t N, uint32_t D, uint32_t K, const float *samples,
                            const float *centroids, const uint32_t *assignments) {
  p->inv = (uint32_t *)malloc(sizeof(uint32_t) * N);
  p->offsets = (uint32_t *)malloc(sizeof(uint32_t) * (K + 2));
  p->radiuses = (float *)malloc(sizeof(float) * K);
  p->cdist = (float *)malloc(sizeof(float) * (size_t)K * K);
  kmo_knn_inverse(N, K, assignments, p->inv, p->offsets);
  kmo_knn_radiuses(metric, N, D, K, samples, centroids, p->inv, p->offsets, p->radiuses);
  kmo_knn_cluster_distances(metric, D, K, centroids, p->cdist);
}
static void knn_corpus_free(knn_corpus_t *p) { free(p->inv); free(p->offsets); free(p->radiuses); free(p->cdist); }

int kmo_knn(uint32_t k, int metric, uint32_t N, uint32_t D, uint32_t K, const float *samples,
            const float *centroids, const uint32_t *assignments, uint32_t *neighbors,
            uint64_t *dists_calced) {
  if (k == 0 || K < 2 || D == 0 || N < K) return 1;
  knn_corpus_t p;
  knn_corpus_init(&p, metric, N, D, K, samples, centroids, assignments);
  uint64_t calced = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : calced)
  for (uint32_t s = 0; s < N; s++) {
    const uint32_t mycls = assignments[s];
    if (mycls >= K) {   /* no cluster (NaN sample): no neighbours, as the product defines it; never a candidate either */
      for (uint32_t i = 0; i < k; i++) neighbors[(size_t)s * k + i] = UINT32_MAX;
      continue;
    }
    float *heap = (float *)malloc(sizeof(float) * 2 * k);
    calced += knn_search_row(k, metric, D, K, samples, centroids, samples + (size_t)s * D, mycls, s, p.inv, p.offsets,
                             p.radiuses, p.cdist, heap, neighbors + (size_t)s * k, NULL);
    free(heap);
  }
  if (dists_calced) *dists_calced = calced;
  knn_corpus_free(&p);
  return 0;
}

/* k-NN of rows that are NOT in the corpus (this repository's index, DESIGN.md 4.8 point 2): the list of query q is
 * what the search above gives for q as one more row of cluster query_assignments[q], nothing skipped; distances = the
 * values the heap compared (FLT_MAX in the slots no candidate filled, whose index is 0).  A query with a non-finite
 * feature or a cluster id >= K has no cluster: indices UINT32_MAX, distances NaN. */
int kmo_knn_query(uint32_t k, int metric, uint32_t N, uint32_t D, uint32_t K, const float *samples,
                  const float *centroids, const uint32_t *assignments, uint32_t Q, const float *queries,
                  const uint32_t *query_assignments, uint32_t *neighbors, float *distances) {
  if (k == 0 || K == 0 || D == 0 || N == 0) return 1;
  knn_corpus_t p;
  knn_corpus_init(&p, metric, N, D, K, samples, centroids, assignments);
#pragma omp parallel for schedule(dynamic, 16)
  for (uint32_t q = 0; q < Q; q++) {
    const float *x = queries + (size_t)q * D;
    uint32_t mycls = query_assignments[q];
    for (uint32_t f = 0; f < D; f++)
      if (!(x[f] - x[f] == 0.f)) mycls = K;
    if (mycls >= K) {
      for (uint32_t i = 0; i < k; i++) { neighbors[(size_t)q * k + i] = UINT32_MAX; distances[(size_t)q * k + i] = NAN; }
      continue;
    }
    float *heap = (float *)malloc(sizeof(float) * 2 * k);
    knn_search_row(k, metric, D, K, samples, centroids, x, mycls, UINT32_MAX, p.inv, p.offsets, p.radiuses, p.cdist, heap,
                   neighbors + (size_t)q * k, distances + (size_t)q * k);
    free(heap);
  }
  knn_corpus_free(&p);
  return 0;
}
