// mr_ensemble.hip — combination models and the reference's threshold mAP on
// the device, over dense models of one context's shard (n_te x width of the
// context's out_dtype, NaN = no pair). MR = MusicRecommender.scala:
//   getLinearCombinationModel(P)      MR:317-351  out = ubm*alpha + ibm*(1-alpha)
//   getAggregationModel(P)            MR:361-418  pair index < (int)(p*P) -> ibm, else ubm
//   getStochasticCombinationModel(P)  MR:429-481  nextFloat() < p -> ibm, else ubm; the
//                                     reference's java.util.Random is unseeded, here a
//                                     seeded counter-based stream over the pair index
//   evaluateModel                     MR:521-639  global min/max (MR:524-525), per-class
//                                     confusion counts at the thresholds (MR:541-553):
//                                     0.0..0.9 (10, MR:590) or 0.0..1.0 (11, the
//                                     distributed evaluation, distributed.scala:395);
//                                     AP per class and the mean (mr_eval_map[_device])
// The pair index is the position of (u, s) in the driver's sorted model
// (main.scala:57-59 sorts by (user, song): the interned order, heard songs
// skipped): idx(u, s) = pair_base + u*n_s - te_off[u] + s - |{t in T(u): t < s}|.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mr_engine.h"
#include "mr_hip_util.h"
#include "mr_internal.h"

namespace {

using mr_hip::Tmp;
using mr_host::fail;

constexpr int kThreads = 256;
// Thresholds: the first n of 0.0, 0.1, ..., 1.0 — n = 10 for MusicRecommender's
// evaluateModel (MR:590: 0.0 :: ... :: 0.9 :: Nil), n = 11 for the distributed
// evaluation (distributed.scala:395: Array(0.0, ..., 1.0)); the same literals.
constexpr int kThresholds = 11;  // the most any evaluation uses
#define MR_THRESHOLDS {0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0}
__constant__ double kThr[kThresholds] = MR_THRESHOLDS;
constexpr double kThrHost[kThresholds] = MR_THRESHOLDS;

inline int thresholds_or_default(int n) { return n == 0 ? 10 : n; }

// ---- combination models -----------------------------------------------------
struct CombParams {
  int n_te, width, song_lo, n_songs, kind;
  double param;
  unsigned long long seed;
  long long pair_base, threshold;
  const long long* te_off;
  const int* te_songs;
  const void* ubm;
  const void* ibm;
  void* out;
};

// splitmix64 finaliser over (seed, pair index): a stateless stream, so every
// pair's draw is independent of launch geometry and shard count.
__host__ __device__ inline unsigned long long splitmix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
// 24 random bits / 2^24, the distribution of java.util.Random.nextFloat.
__host__ __device__ inline float pair_uniform(unsigned long long seed, long long idx) {
  const unsigned long long z = splitmix64(seed + (unsigned long long)(idx + 1) * 0x9E3779B97F4A7C15ull);
  return (float)(unsigned)(z >> 40) * (1.0f / 16777216.0f);
}

#ifndef MR_COMB_PER
#define MR_COMB_PER 8  // C5: 86.44 vs 87.00 ms per step at 4 (profiles/r04/s35)
#endif
constexpr int kCombPer = MR_COMB_PER;  // songs per thread (strided by kThreads: coalesced)

// One (user, kThreads * kCombPer-song block) per workgroup. The pair index
// needs |{t in T(u): t < s}|: one binary search per block for the first heard
// song at or after the block, then the few heard songs inside the block are
// walked per element (T(u) is sorted; rows are short).
template <typename OutT>
__global__ __launch_bounds__(kThreads) void k_combine(CombParams p) {
  const int u = blockIdx.y;
  const int i0 = blockIdx.x * kThreads * kCombPer + threadIdx.x;
  const size_t row = (size_t)u * p.width;
  const OutT* ubm = reinterpret_cast<const OutT*>(p.ubm) + row;
  const OutT* ibm = reinterpret_cast<const OutT*>(p.ibm) + row;
  OutT* out = reinterpret_cast<OutT*>(p.out) + row;
  OutT a4[kCombPer], b4[kCombPer];
#pragma unroll
  for (int r = 0; r < kCombPer; ++r) {
    const int i = i0 + r * kThreads;
    a4[r] = i < p.width ? ubm[i] : (OutT)0;
    b4[r] = i < p.width ? ibm[i] : (OutT)0;
  }
  if (p.kind == MR_COMB_LINEAR) {  // MR:327: rank1 * alpha + rank2 * (1 - alpha); NaN stays NaN
#pragma unroll
    for (int r = 0; r < kCombPer; ++r) {
      const int i = i0 + r * kThreads;
      if (i < p.width) out[i] = (OutT)((double)a4[r] * p.param + (double)b4[r] * (1.0 - p.param));
    }
    return;
  }
  const long long t0 = p.te_off[u], t1 = p.te_off[u + 1];
  const int s_blk = p.song_lo + blockIdx.x * kThreads * kCombPer;  // first song of the block
  long long a = t0, b = t1;  // first song of T(u) >= s_blk (uniform over the block)
  while (a < b) {
    const long long m = (a + b) >> 1;
    if (p.te_songs[m] < s_blk) a = m + 1; else b = m;
  }
#pragma unroll
  for (int r = 0; r < kCombPer; ++r) {
    const int i = i0 + r * kThreads;
    if (i >= p.width) continue;
    const int s = p.song_lo + i;
    long long j = a;  // first song of T(u) >= s
    while (j < t1 && p.te_songs[j] < s) ++j;
    if (j < t1 && p.te_songs[j] == s) {  // heard: no pair (MR:109)
      out[i] = (OutT)NAN;
      continue;
    }
    const long long idx = p.pair_base + (long long)u * p.n_songs - t0 + s - (j - t0);
    const bool take_ibm = p.kind == MR_COMB_AGGREGATION ? idx < p.threshold                   // MR:380-381
                                                        : (double)pair_uniform(p.seed, idx) < p.param;  // MR:414-415
    out[i] = take_ibm ? b4[r] : a4[r];
  }
}

// The driver's three combinations in one pass (mr_combine_all_device): each
// block reads its ubm / ibm elements once and writes the linear, aggregation
// and stochastic outputs with k_combine's exact expressions; with part != null
// it also leaves the min / max of each output over its pairs (NaN skipped, in
// the element type, as k_minmax) in part[block][6].
struct Comb3Params {
  int n_te, width, song_lo, n_songs;
  double alpha, p_sto;
  unsigned long long seed;
  long long pair_base, threshold;
  const long long* te_off;
  const int* te_songs;
  const void* ubm;
  const void* ibm;
  void* out[3];  // linear, aggregation, stochastic
  double* part;
};
template <typename OutT>
__global__ __launch_bounds__(kThreads) void k_combine3(Comb3Params p) {
  __shared__ double sm[6][kThreads];
  const int u = blockIdx.y;
  const int i0 = blockIdx.x * kThreads * kCombPer + threadIdx.x;
  const size_t row = (size_t)u * p.width;
  const OutT* ubm = reinterpret_cast<const OutT*>(p.ubm) + row;
  const OutT* ibm = reinterpret_cast<const OutT*>(p.ibm) + row;
  OutT* o_lin = reinterpret_cast<OutT*>(p.out[0]) + row;
  OutT* o_agg = reinterpret_cast<OutT*>(p.out[1]) + row;
  OutT* o_sto = reinterpret_cast<OutT*>(p.out[2]) + row;
  OutT a4[kCombPer], b4[kCombPer];
#pragma unroll
  for (int r = 0; r < kCombPer; ++r) {
    const int i = i0 + r * kThreads;
    a4[r] = i < p.width ? ubm[i] : (OutT)0;
    b4[r] = i < p.width ? ibm[i] : (OutT)0;
  }
  const long long t0 = p.te_off[u], t1 = p.te_off[u + 1];
  const int s_blk = p.song_lo + blockIdx.x * kThreads * kCombPer;  // first song of the block
  long long a = t0, b = t1;  // first song of T(u) >= s_blk (uniform over the block)
  while (a < b) {
    const long long m = (a + b) >> 1;
    if (p.te_songs[m] < s_blk) a = m + 1; else b = m;
  }
  OutT mn[3], mx[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) { mn[c] = (OutT)INFINITY; mx[c] = (OutT)-INFINITY; }
  auto track = [&](int c, OutT x) {
    if (x != x) return;
    mn[c] = x < mn[c] ? x : mn[c];
    mx[c] = x > mx[c] ? x : mx[c];
  };
#pragma unroll
  for (int r = 0; r < kCombPer; ++r) {
    const int i = i0 + r * kThreads;
    if (i >= p.width) continue;
    const OutT lin = (OutT)((double)a4[r] * p.alpha + (double)b4[r] * (1.0 - p.alpha));  // MR:327
    o_lin[i] = lin;
    track(0, lin);
    const int s = p.song_lo + i;
    long long j = a;  // first song of T(u) >= s
    while (j < t1 && p.te_songs[j] < s) ++j;
    if (j < t1 && p.te_songs[j] == s) {  // heard: no pair (MR:109)
      o_agg[i] = (OutT)NAN;
      o_sto[i] = (OutT)NAN;
      continue;
    }
    const long long idx = p.pair_base + (long long)u * p.n_songs - t0 + s - (j - t0);
    const OutT agg = idx < p.threshold ? b4[r] : a4[r];                               // MR:380-381
    const OutT sto = (double)pair_uniform(p.seed, idx) < p.p_sto ? b4[r] : a4[r];     // MR:414-415
    o_agg[i] = agg;
    o_sto[i] = sto;
    track(1, agg);
    track(2, sto);
  }
  if (!p.part) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    sm[2 * c][threadIdx.x] = (double)mn[c];
    sm[2 * c + 1][threadIdx.x] = (double)mx[c];
  }
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        sm[2 * c][threadIdx.x] = fmin(sm[2 * c][threadIdx.x], sm[2 * c][threadIdx.x + h]);
        sm[2 * c + 1][threadIdx.x] = fmax(sm[2 * c + 1][threadIdx.x], sm[2 * c + 1][threadIdx.x + h]);
      }
    __syncthreads();
  }
  if (threadIdx.x < 6) p.part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = sm[threadIdx.x][0];
}

// part[n][6] (min, max, min, max, min, max) -> part2[gridDim.x][6]
__global__ __launch_bounds__(kThreads) void k_minmax6(const double* part, long long n, double* part2) {
  __shared__ double sm[6][kThreads];
  double v[6] = {INFINITY, -INFINITY, INFINITY, -INFINITY, INFINITY, -INFINITY};
  for (long long b = (long long)blockIdx.x * kThreads + threadIdx.x; b < n; b += (long long)gridDim.x * kThreads)
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] = (c & 1) ? fmax(v[c], part[b * 6 + c]) : fmin(v[c], part[b * 6 + c]);
#pragma unroll
  for (int c = 0; c < 6; ++c) sm[c][threadIdx.x] = v[c];
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h)
#pragma unroll
      for (int c = 0; c < 6; ++c)
        sm[c][threadIdx.x] = (c & 1) ? fmax(sm[c][threadIdx.x], sm[c][threadIdx.x + h])
                                     : fmin(sm[c][threadIdx.x], sm[c][threadIdx.x + h]);
    __syncthreads();
  }
  if (threadIdx.x < 6) part2[(size_t)blockIdx.x * 6 + threadIdx.x] = sm[threadIdx.x][0];
}

// ---- evaluation ------------------------------------------------------------
constexpr int kMinmaxPer = 8;  // loads in flight per thread per iteration

template <typename OutT>
__global__ __launch_bounds__(kThreads) void k_minmax(const OutT* d, long long n, double* part) {
  __shared__ double smn[kThreads], smx[kThreads];
  OutT mn = (OutT)INFINITY, mx = (OutT)-INFINITY;  // min/max are exact in the element type
  const long long stride = (long long)gridDim.x * kThreads;
  for (long long i0 = (long long)blockIdx.x * kThreads + threadIdx.x; i0 < n; i0 += stride * kMinmaxPer) {
    OutT x[kMinmaxPer];
#pragma unroll
    for (int r = 0; r < kMinmaxPer; ++r) {
      const long long i = i0 + r * stride;
      x[r] = i < n ? d[i] : (OutT)NAN;
    }
#pragma unroll
    for (int r = 0; r < kMinmaxPer; ++r) {
      if (x[r] != x[r]) continue;
      mn = x[r] < mn ? x[r] : mn;
      mx = x[r] > mx ? x[r] : mx;
    }
  }
  smn[threadIdx.x] = (double)mn;
  smx[threadIdx.x] = (double)mx;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      smn[threadIdx.x] = fmin(smn[threadIdx.x], smn[threadIdx.x + h]);
      smx[threadIdx.x] = fmax(smx[threadIdx.x], smx[threadIdx.x + h]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    part[2 * blockIdx.x] = smn[0];
    part[2 * blockIdx.x + 1] = smx[0];
  }
}

struct EvalParams {
  int n_te, width, song_lo, users_per_block, n_thr;
  double mn, mx;
  const void* dense;
  int* pred;  // [width][n_thr]: users with (x - min) / (max - min) > t_i (MR:529)
  int* tp;    // [width][n_thr]: of those, users whose labels hold the song (MR:545)
  const int* lab_u;
  const int* lab_s;
  long long n_lab;
  float xt_f[kThresholds];   // smallest score with (x - min) / (max - min) > t_i (f32 models)
  double xt_d[kThresholds];  // the same for f64 models
};

// The level test (x - mn) / (mx - mn) > t of MR:529 is monotone in x (fp64
// subtraction and division by a positive range are monotone under rounding),
// so it equals x >= xt with xt the smallest score of the model's element type
// that passes. Found on the host by bisection over the ordered bit patterns of
// that type, with the same fp64 expression: exact, and the kernel then needs
// n_thr compares per element instead of an fp64 division.
template <typename T, typename U>
T level_floor(double mn, double mx, double t) {
  constexpr int B = sizeof(T) * 8;
  const U sign = (U)1 << (B - 1);
  auto key = [&](T x) { U b; std::memcpy(&b, &x, sizeof b); return (b & sign) ? (U)~b : (U)(b | sign); };
  auto val = [&](U k) { U b = (k & sign) ? (U)(k & ~sign) : (U)~k; T x; std::memcpy(&x, &b, sizeof x); return x; };
  auto pass = [&](U k) { return ((double)val(k) - mn) / (mx - mn) > t; };
  U lo = key(-INFINITY), hi = key(INFINITY);  // NaN patterns lie outside [lo, hi]
  if (!pass(hi)) return (T)NAN;               // nothing passes (mx == mn: 0 / 0)
  while (lo < hi) {                           // smallest passing key
    const U m = lo + (hi - lo) / 2;
    if (pass(m)) hi = m; else lo = m + 1;
  }
  return val(lo);
}

__device__ __forceinline__ int levels(double x, double mn, double mx, int n_thr) {
  const double v = (x - mn) / (mx - mn);  // MR:529 (NaN > t is false)
  int c = 0;
#pragma unroll
  for (int t = 0; t < kThresholds; ++t) c += (t < n_thr && v > kThr[t]) ? 1 : 0;
  return c;  // thresholds ascend: predicted at t_i for every i < c
}

// one thread per song column, a block of users per blockIdx.y (rows read coalesced)
#ifndef MR_EVAL_U
#define MR_EVAL_U 16  // C5: 86.53 vs 87.00 ms per step at 8 (profiles/r04/s35)
#endif
template <typename OutT>
__global__ __launch_bounds__(kThreads) void k_eval_pred(EvalParams p) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.width) return;
  const int u0 = blockIdx.y * p.users_per_block, u1 = min(p.n_te, u0 + p.users_per_block);
  const OutT* d = reinterpret_cast<const OutT*>(p.dense);
  OutT xt[kThresholds];
#pragma unroll
  for (int t = 0; t < kThresholds; ++t)  // unused slots: +inf, reached by a +inf score only; never stored
    xt[t] = t < p.n_thr ? (sizeof(OutT) == 4 ? (OutT)p.xt_f[t] : (OutT)p.xt_d[t]) : (OutT)INFINITY;
  int cnt[kThresholds];
#pragma unroll
  for (int t = 0; t < kThresholds; ++t) cnt[t] = 0;
  constexpr int U = MR_EVAL_U;  // rows in flight per thread
  for (int ub = u0; ub < u1; ub += U) {
    OutT x[U];
#pragma unroll
    for (int r = 0; r < U; ++r) x[r] = ub + r < u1 ? d[(size_t)(ub + r) * p.width + i] : (OutT)NAN;
#pragma unroll
    for (int r = 0; r < U; ++r)
#pragma unroll
      for (int t = 0; t < kThresholds; ++t) cnt[t] += x[r] >= xt[t] ? 1 : 0;  // NaN (no pair): never
  }
  if (gridDim.y == 1) {  // one user block: this thread owns the song's counts (no zeroing, no atomics)
#pragma unroll
    for (int t = 0; t < kThresholds; ++t)
      if (t < p.n_thr) p.pred[(size_t)i * p.n_thr + t] = cnt[t];
    return;
  }
#pragma unroll
  for (int t = 0; t < kThresholds; ++t)  // t < n_thr: a +inf score passes the unused slots' +inf
    if (t < p.n_thr && cnt[t]) atomicAdd(&p.pred[(size_t)i * p.n_thr + t], cnt[t]);
}

template <typename OutT>
__global__ __launch_bounds__(kThreads) void k_eval_tp(EvalParams p) {
  const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.n_lab) return;
  const int u = p.lab_u[j], g = p.lab_s[j] - p.song_lo;
  if (g < 0 || g >= p.width) return;  // other shard, or a label-only song (never predicted)
  const double x = (double)reinterpret_cast<const OutT*>(p.dense)[(size_t)u * p.width + g];
  if (x != x) return;
  const int c = levels(x, p.mn, p.mx, p.n_thr);
  for (int t = 0; t < c; ++t) atomicAdd(&p.tp[(size_t)g * p.n_thr + t], 1);
}

// AP of the label classes cls[0..n) of the shard (shard-local song ids, np =
// their label counts pos, all > 0; MR:588-618), the host fold's exact double
// operations (mr_eval_map) per class.
__global__ __launch_bounds__(kThreads) void k_eval_ap(int n, int n_thr, const int* cls, const int* cpos,
                                                      const int* pred, const int* tp, double* ap) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= n) return;
  const int g = cls[c];
  const int np = cpos[c];
  double P[kThresholds], R[kThresholds];
#pragma unroll
  for (int t = 0; t < kThresholds; ++t) {
    const size_t i = (size_t)g * n_thr + (t < n_thr ? t : 0);
    P[t] = pred[i] > 0 ? (double)tp[i] / (double)pred[i] : 0.0;
    R[t] = (double)tp[i] / (double)np;
  }
  // AP = sum over i of: (R_i - R_{i+1}) * P_i, (R_{n-2} - 0.0) * P_{n-2} at
  // i = n - 2, 0 at i = n - 1 (MR:601-609, distributed.scala:405-413), left fold
  double a = 0.0;
#pragma unroll
  for (int t = 0; t < kThresholds; ++t) {
    if (t >= n_thr) break;
    const double term = t == n_thr - 1 ? 0.0 : t == n_thr - 2 ? (R[t] - 0.0) * P[t] : (R[t] - R[t + 1]) * P[t];
    a = a + term;
  }
  ap[c] = a;
}

// The label classes' rows of the shard's counts, in a class-indexed block
// that every rank lays out alike (the global class list): out[0][c][t] =
// pred, out[1][c][t] = tp of class c when its song is in [song_lo, song_hi),
// else 0 — so summing the blocks over ranks (one all-reduce) gives the counts
// of MR:541-553 over every test user, whatever the layout.
__global__ __launch_bounds__(kThreads) void k_eval_gather(int n_cls, int n_thr, int song_lo, int width,
                                                          const int* cls, const int* pred, const int* tp,
                                                          int* out) {
  const int j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_cls * n_thr) return;
  const int c = j / n_thr, t = j - c * n_thr;
  const int g = cls[c] - song_lo;
  const bool in = g >= 0 && g < width;
  out[j] = in ? pred[(size_t)g * n_thr + t] : 0;
  out[(size_t)n_cls * n_thr + j] = in ? tp[(size_t)g * n_thr + t] : 0;
}

// The label CSR of the context's test users as (user, song) pairs, one per
// label (at least one slot, so the staging buffers are never empty).
int label_pairs(int n_te, const int64_t* lab_off, const int32_t* lab_songs, std::vector<int32_t>& lu,
                std::vector<int32_t>& ls) {
  const long long n_lab = lab_off[n_te];
  if (n_lab > 0 && !lab_songs) return fail(MR_E_INVALID, "null label songs");
  lu.assign((size_t)std::max<long long>(1, n_lab), 0);
  ls.assign((size_t)std::max<long long>(1, n_lab), 0);
  for (int u = 0; u < n_te; ++u)
    for (int64_t j = lab_off[u]; j < lab_off[u + 1]; ++j) {
      if (j < 0 || j >= n_lab || lab_off[u + 1] < lab_off[u]) return fail(MR_E_INVALID, "bad label CSR");
      lu[j] = u;
      ls[j] = lab_songs[j];
    }
  return MR_OK;
}

// pred / tp counts of the shard into the device buffers d_pred / d_tp
// ([width][n_thr], stream-ordered on the context stream; the caller frees
// them), for n_models dense models in turn: the labels are staged once, and
// after model i's counts are queued after(i) queues what consumes them (the
// buffers are reused by model i + 1, in stream order).
template <typename After>
int eval_counts(mr_ctx* ctx, int n_models, const void* const* dense, const double* mn, const double* mx,
                const int64_t* lab_off, const int32_t* lab_songs, int n_thr, mr_view& v, Tmp<int>& d_pred,
                Tmp<int>& d_tp, After&& after) {
  if (!ctx || !dense || !lab_off || !mn || !mx || n_models < 1) return fail(MR_E_INVALID, "null argument");
  for (int i = 0; i < n_models; ++i)
    if (!dense[i]) return fail(MR_E_INVALID, "null dense model %d", i);
  if (n_thr != 10 && n_thr != 11)
    return fail(MR_E_INVALID, "%d thresholds: 10 (MR:590) or 11 (distributed.scala:395)", n_thr);
  int rc = mr_view_get(ctx, &v);
  if (rc) return rc;
  MR_HIP(hipSetDevice(v.device));
  const int width = v.song_hi - v.song_lo, n_te = v.n_test_users;
  std::vector<int32_t> lu, ls;
  if ((rc = label_pairs(n_te, lab_off, lab_songs, lu, ls))) return rc;
  const long long n_lab = lab_off[n_te];
  hipStream_t st = (hipStream_t)v.stream;
  Tmp<int> d_lu, d_ls;
  const size_t nc = (size_t)width * n_thr;
  if (int rc_ = d_pred.alloc(std::max<size_t>(1, nc), st)) return rc_;
  if (int rc_ = d_tp.alloc(std::max<size_t>(1, nc), st)) return rc_;
  if (int rc_ = d_lu.alloc(lu.size(), st)) return rc_;
  if (int rc_ = d_ls.alloc(ls.size(), st)) return rc_;
  MR_HIP(hipMemcpyAsync(d_lu.p, lu.data(), lu.size() * 4, hipMemcpyHostToDevice, st));
  MR_HIP(hipMemcpyAsync(d_ls.p, ls.data(), ls.size() * 4, hipMemcpyHostToDevice, st));
  // (song block x user block) workgroups: ~1024 of them fill the chip (a
  // thread keeps 16 rows' loads in flight); a user block per workgroup row
  // adds its counts atomically, so split the users only when the songs alone
  // give too few workgroups (narrow shards). One user block (the whole model
  // of a wide shard, any user count): plain stores, no zeroing, no atomics —
  // the atomics, not the model's bytes, were the pass's cost at a few hundred
  // users (C5's 250-user blocks at 8 GPUs: 0.84 ms per model).
  const int sx = (width + kThreads - 1) / kThreads;
  const int uy = std::max(1, std::min((n_te + 15) / 16, (1024 + sx - 1) / sx));
  const bool f64 = v.out_dtype == MR_OUT_F64;
  for (int i = 0; i < n_models; ++i) {
    if (uy > 1) MR_HIP(hipMemsetAsync(d_pred.p, 0, nc * 4, st));
    MR_HIP(hipMemsetAsync(d_tp.p, 0, nc * 4, st));
    EvalParams ep{n_te, width, v.song_lo, (n_te + uy - 1) / uy, n_thr, mn[i], mx[i], dense[i], d_pred.p, d_tp.p,
                  d_lu.p, d_ls.p, n_lab};
    for (int t = 0; t < n_thr; ++t) {
      const double thr = kThrHost[t];
      ep.xt_f[t] = level_floor<float, uint32_t>(mn[i], mx[i], thr);
      ep.xt_d[t] = level_floor<double, uint64_t>(mn[i], mx[i], thr);
    }
    if (width > 0) {
      if (f64) hipLaunchKernelGGL(k_eval_pred<double>, dim3(sx, uy), dim3(kThreads), 0, st, ep);
      else hipLaunchKernelGGL(k_eval_pred<float>, dim3(sx, uy), dim3(kThreads), 0, st, ep);
      MR_HIP(hipGetLastError());
    }
    if (n_lab > 0) {
      const int lb = (int)((n_lab + kThreads - 1) / kThreads);
      if (f64) hipLaunchKernelGGL(k_eval_tp<double>, dim3(lb), dim3(kThreads), 0, st, ep);
      else hipLaunchKernelGGL(k_eval_tp<float>, dim3(lb), dim3(kThreads), 0, st, ep);
      MR_HIP(hipGetLastError());
    }
    if ((rc = after(i))) return rc;
  }
  // the label staging is freed in stream order after these kernels (Tmp)
  return MR_OK;
}

// ---- parameter sweep ---------------------------------------------------------
// The threshold mAP of one combination kind at P parameter values without
// materialising a combined model: out_j(u, s) is formed in registers from ubm
// and ibm with k_combine's expressions (same element type, same fp64
// operations), three times — for the extremes, the predicted counts and the
// true positives. The tail (class block, k_eval_ap, ordered host sum) is the
// evaluation's own.
#ifndef MR_SWEEP_G
#define MR_SWEEP_G 4  // parameters per counting pass: G x n_thr register counters per thread
#endif
#ifndef MR_SWEEP_U
#define MR_SWEEP_U 8  // rows in flight per thread: 2 x 8 loads, k_eval_pred's 16
#endif
constexpr int kSweepG = MR_SWEEP_G;
constexpr int kSweepMax = MR_SWEEP_MAX_PARAMS;
constexpr int kWave = 64;

struct SweepTab {  // per parameter j, device-resident for the call
  double p[kSweepMax];        // p_j
  double q[kSweepMax];        // 1.0 - p_j (the linear weight of ibm, MR:327)
  long long thr[kSweepMax];   // (long long)(p_j * n_pairs) (aggregation, MR:371)
  double mn[kSweepMax], mx[kSweepMax];  // global extremes of out_j
  float xt_f[kSweepMax][kThresholds];   // level_floor per threshold (+inf past n_thr)
  double xt_d[kSweepMax][kThresholds];
};

struct SweepParams {
  int n_te, width, song_lo, n_songs, n_params, n_thr, users_per_block;
  unsigned long long seed;
  long long pair_base;
  const long long* te_off;
  const int* te_songs;
  const void* ubm;
  const void* ibm;
  const SweepTab* tab;
  int* pred;  // [G][width][n_thr], the counts of one group of parameters
  int* tp;
  const int* lab_u;
  const int* lab_s;
  long long n_lab;
  double* part;  // [blocks][n_params][2]
};

// first index in te_songs[a, b) (sorted) whose song is >= s
__device__ __forceinline__ long long first_heard(const int* te_songs, long long a, long long b, int s) {
  while (a < b) {
    const long long m = (a + b) >> 1;
    if (te_songs[m] < s) a = m + 1; else b = m;
  }
  return a;
}

// Index of pair (u, s) as k_combine computes it (pair_base + u * n_s - t0 + s
// - (j - t0)), j = first index of T(u) = te_songs[.., t1) with a song >= s;
// -1 for a heard song (no pair, MR:109).
__device__ __forceinline__ long long sweep_pair(const SweepParams& p, int u, int s, long long j, long long t1) {
  if (j < t1 && p.te_songs[j] == s) return -1;
  return p.pair_base + (long long)u * p.n_songs + s - j;
}

// What selects ibm over ubm for one element, shared by every parameter: the
// pair index (aggregation) or the pair's uniform draw (stochastic).
template <int K>
struct SweepKey { long long v; };
template <>
struct SweepKey<MR_COMB_STOCHASTIC> { float v; };

template <int K>
__device__ __forceinline__ SweepKey<K> sweep_key(const SweepParams& p, long long idx) {
  SweepKey<K> k;
  if constexpr (K == MR_COMB_STOCHASTIC) k.v = pair_uniform(p.seed, idx);
  else k.v = idx;
  return k;
}

// out_j of one element: the value k_combine<OutT> stores for param = p_j
// (a, b = NaN for a heard song of the selecting kinds).
template <typename OutT, int K>
__device__ __forceinline__ OutT sweep_out(OutT a, OutT b, SweepKey<K> key, double pj, double qj, long long thr) {
  if constexpr (K == MR_COMB_LINEAR) return (OutT)((double)a * pj + (double)b * qj);  // MR:327
  else if constexpr (K == MR_COMB_AGGREGATION) return key.v < thr ? b : a;           // MR:380-381
  else return (double)key.v < pj ? b : a;                                            // MR:414-415
}

__device__ __forceinline__ float wave_xor(float x, int m) { return __shfl_xor(x, m, kWave); }
__device__ __forceinline__ double wave_xor(double x, int m) { return __shfl_xor(x, m, kWave); }

// Extremes pass. A workgroup takes one kThreads * kCombPer song block (as
// k_combine) and walks the users blockIdx.y, + gridDim.y, ...: the elements of
// one (user, block) stay in registers while the P outputs are formed from them
// in turn; each output's min / max (NaN skipped, in the element type) is
// reduced over the wave and folded into the wave's running pair in LDS (lane 0
// owns its wave's slots: no barrier inside the loop). The user walk keeps the
// partials at [blocks][P][2] for a few thousand blocks whatever the user
// count, and grid-y far below its limit.
template <typename OutT, int K>
__global__ __launch_bounds__(kThreads) void k_sweep_minmax(SweepParams p) {
  __shared__ double sm[kThreads / kWave][kSweepMax][2];
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const SweepTab* __restrict__ tab = p.tab;
  for (int j = lane; j < p.n_params; j += kWave) {
    sm[wave][j][0] = INFINITY;
    sm[wave][j][1] = -INFINITY;
  }
  __syncthreads();
  const int i0 = blockIdx.x * kThreads * kCombPer + threadIdx.x;
  const int s_blk = p.song_lo + blockIdx.x * kThreads * kCombPer;  // first song of the block
  for (int u = blockIdx.y; u < p.n_te; u += gridDim.y) {
    const size_t row = (size_t)u * p.width;
    const OutT* ubm = reinterpret_cast<const OutT*>(p.ubm) + row;
    const OutT* ibm = reinterpret_cast<const OutT*>(p.ibm) + row;
    OutT a4[kCombPer], b4[kCombPer];
    SweepKey<K> key[kCombPer] = {};
#pragma unroll
    for (int r = 0; r < kCombPer; ++r) {  // past the width: NaN, skipped
      const int i = i0 + r * kThreads;
      a4[r] = i < p.width ? ubm[i] : (OutT)NAN;
      b4[r] = i < p.width ? ibm[i] : (OutT)NAN;
    }
    if constexpr (K != MR_COMB_LINEAR) {
      const long long t1 = p.te_off[u + 1];
      const long long j0 = first_heard(p.te_songs, p.te_off[u], t1, s_blk);  // uniform over the block
#pragma unroll
      for (int r = 0; r < kCombPer; ++r) {
        const int i = i0 + r * kThreads;
        key[r] = SweepKey<K>{};
        if (i >= p.width) continue;
        const int s = p.song_lo + i;
        long long j = j0;
        while (j < t1 && p.te_songs[j] < s) ++j;
        const long long idx = sweep_pair(p, u, s, j, t1);
        if (idx < 0) a4[r] = b4[r] = (OutT)NAN;
        key[r] = sweep_key<K>(p, idx);
      }
    }
    for (int j = 0; j < p.n_params; ++j) {
      const double pj = tab->p[j], qj = tab->q[j];
      const long long thr = tab->thr[j];
      OutT mn = (OutT)INFINITY, mx = (OutT)-INFINITY;
#pragma unroll
      for (int r = 0; r < kCombPer; ++r) {
        const OutT x = sweep_out<OutT, K>(a4[r], b4[r], key[r], pj, qj, thr);
        if (x != x) continue;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
      }
#pragma unroll
      for (int m = kWave / 2; m > 0; m >>= 1) {
        const OutT on = wave_xor(mn, m), ox = wave_xor(mx, m);
        mn = on < mn ? on : mn;
        mx = ox > mx ? ox : mx;
      }
      if (lane == 0) {
        sm[wave][j][0] = fmin(sm[wave][j][0], (double)mn);
        sm[wave][j][1] = fmax(sm[wave][j][1], (double)mx);
      }
    }
  }
  __syncthreads();
  const size_t blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
  for (int j = threadIdx.x; j < p.n_params; j += kThreads) {
    double mn = sm[0][j][0], mx = sm[0][j][1];
#pragma unroll
    for (int w = 1; w < kThreads / kWave; ++w) {
      mn = fmin(mn, sm[w][j][0]);
      mx = fmax(mx, sm[w][j][1]);
    }
    p.part[(blk * p.n_params + j) * 2] = mn;
    p.part[(blk * p.n_params + j) * 2 + 1] = mx;
  }
}

// part[n][P][2] -> out[P][2]: workgroup j reduces parameter j over the n blocks
__global__ __launch_bounds__(kThreads) void k_sweep_minmax2(const double* part, long long n, int n_params,
                                                            double* out) {
  __shared__ double smn[kThreads], smx[kThreads];
  const int j = blockIdx.x;
  double mn = INFINITY, mx = -INFINITY;
  for (long long b = threadIdx.x; b < n; b += kThreads) {
    mn = fmin(mn, part[(b * n_params + j) * 2]);
    mx = fmax(mx, part[(b * n_params + j) * 2 + 1]);
  }
  smn[threadIdx.x] = mn;
  smx[threadIdx.x] = mx;
  __syncthreads();
  for (int h = kThreads / 2; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) {
      smn[threadIdx.x] = fmin(smn[threadIdx.x], smn[threadIdx.x + h]);
      smx[threadIdx.x] = fmax(smx[threadIdx.x], smx[threadIdx.x + h]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[2 * j] = smn[0];
    out[2 * j + 1] = smx[0];
  }
}

// Predicted-count pass of parameters [j0, j0 + G): k_eval_pred's shape (one
// thread per song column, a block of users per blockIdx.y, rows in flight),
// each row's element combined G ways and compared against that parameter's
// level floors; G x n_thr counters per thread, into pred[g][song][t].
template <typename OutT, int K>
__global__ __launch_bounds__(kThreads) void k_sweep_pred(SweepParams p, int j0) {
  constexpr int G = kSweepG;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.width) return;
  const int u0 = blockIdx.y * p.users_per_block, u1 = min(p.n_te, u0 + p.users_per_block);
  const OutT* ubm = reinterpret_cast<const OutT*>(p.ubm);
  const OutT* ibm = reinterpret_cast<const OutT*>(p.ibm);
  const SweepTab* __restrict__ tab = p.tab;
  const int ng = min(G, p.n_params - j0);
  OutT xt[G][kThresholds];
  double pg[G], qg[G];
  long long tg[G];
  int cnt[G][kThresholds];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    const int j = j0 + (g < ng ? g : 0);  // a short last group: the spare slots repeat its first, never stored
    pg[g] = tab->p[j];
    qg[g] = tab->q[j];
    tg[g] = tab->thr[j];
#pragma unroll
    for (int t = 0; t < kThresholds; ++t) {
      xt[g][t] = sizeof(OutT) == 4 ? (OutT)tab->xt_f[j][t] : (OutT)tab->xt_d[j][t];
      cnt[g][t] = 0;
    }
  }
  constexpr int U = MR_SWEEP_U;  // rows in flight per thread
  const int s = p.song_lo + i;
  const int s_blk = p.song_lo + blockIdx.x * kThreads;  // first song of the block
  for (int ub = u0; ub < u1; ub += U) {
    OutT a[U], b[U];
    SweepKey<K> key[U] = {};
#pragma unroll
    for (int r = 0; r < U; ++r) {
      a[r] = ub + r < u1 ? ubm[(size_t)(ub + r) * p.width + i] : (OutT)NAN;
      b[r] = ub + r < u1 ? ibm[(size_t)(ub + r) * p.width + i] : (OutT)NAN;
    }
    if constexpr (K != MR_COMB_LINEAR) {
#pragma unroll
      for (int r = 0; r < U; ++r) {
        key[r] = SweepKey<K>{};
        if (ub + r >= u1) continue;
        const long long t1 = p.te_off[ub + r + 1];
        long long j = first_heard(p.te_songs, p.te_off[ub + r], t1, s_blk);  // uniform over the block
        while (j < t1 && p.te_songs[j] < s) ++j;
        const long long idx = sweep_pair(p, ub + r, s, j, t1);
        if (idx < 0) a[r] = b[r] = (OutT)NAN;
        key[r] = sweep_key<K>(p, idx);
      }
    }
#pragma unroll
    for (int r = 0; r < U; ++r)
#pragma unroll
      for (int g = 0; g < G; ++g) {
        const OutT x = sweep_out<OutT, K>(a[r], b[r], key[r], pg[g], qg[g], tg[g]);
#pragma unroll
        for (int t = 0; t < kThresholds; ++t) cnt[g][t] += x >= xt[g][t] ? 1 : 0;  // NaN (no pair): never
      }
  }
#pragma unroll
  for (int g = 0; g < G; ++g) {  // (conditions, not breaks: the counters stay in registers)
    int* pred = p.pred + ((size_t)g * p.width + i) * p.n_thr;
#pragma unroll
    for (int t = 0; t < kThresholds; ++t) {
      if (g < ng && t < p.n_thr) {
        if (gridDim.y == 1) pred[t] = cnt[g][t];  // one user block: this thread owns the song's counts
        else if (cnt[g][t]) atomicAdd(&pred[t], cnt[g][t]);
      }
    }
  }
}

// True-positive pass of parameters [j0, j0 + ng): one thread per label (u, s),
// as k_eval_tp, the element combined ng ways.
template <typename OutT, int K>
__global__ __launch_bounds__(kThreads) void k_sweep_tp(SweepParams p, int j0, int ng) {
  const long long l = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (l >= p.n_lab) return;
  const int u = p.lab_u[l], s = p.lab_s[l], i = s - p.song_lo;
  if (i < 0 || i >= p.width) return;  // other shard, or a label-only song (never predicted)
  OutT a = reinterpret_cast<const OutT*>(p.ubm)[(size_t)u * p.width + i];
  OutT b = reinterpret_cast<const OutT*>(p.ibm)[(size_t)u * p.width + i];
  SweepKey<K> key{};
  if constexpr (K != MR_COMB_LINEAR) {
    const long long t1 = p.te_off[u + 1];
    const long long idx = sweep_pair(p, u, s, first_heard(p.te_songs, p.te_off[u], t1, s), t1);
    if (idx < 0) return;
    key = sweep_key<K>(p, idx);
  }
  const SweepTab* __restrict__ tab = p.tab;
  for (int g = 0; g < ng; ++g) {
    const int j = j0 + g;
    const double x = (double)sweep_out<OutT, K>(a, b, key, tab->p[j], tab->q[j], tab->thr[j]);
    if (x != x) continue;
    const int c = levels(x, tab->mn[j], tab->mx[j], p.n_thr);
    int* tp = p.tp + ((size_t)g * p.width + i) * p.n_thr;
    for (int t = 0; t < c; ++t) atomicAdd(&tp[t], 1);
  }
}

#define MR_SWEEP_LAUNCH(KERNEL, f64, kind, grid, st, ...)                                                        \
  do {                                                                                                           \
    if (f64) {                                                                                                   \
      if (kind == MR_COMB_LINEAR)                                                                                \
        hipLaunchKernelGGL((KERNEL<double, MR_COMB_LINEAR>), grid, dim3(kThreads), 0, st, __VA_ARGS__);          \
      else if (kind == MR_COMB_AGGREGATION)                                                                      \
        hipLaunchKernelGGL((KERNEL<double, MR_COMB_AGGREGATION>), grid, dim3(kThreads), 0, st, __VA_ARGS__);     \
      else                                                                                                       \
        hipLaunchKernelGGL((KERNEL<double, MR_COMB_STOCHASTIC>), grid, dim3(kThreads), 0, st, __VA_ARGS__);      \
    } else {                                                                                                     \
      if (kind == MR_COMB_LINEAR)                                                                                \
        hipLaunchKernelGGL((KERNEL<float, MR_COMB_LINEAR>), grid, dim3(kThreads), 0, st, __VA_ARGS__);           \
      else if (kind == MR_COMB_AGGREGATION)                                                                      \
        hipLaunchKernelGGL((KERNEL<float, MR_COMB_AGGREGATION>), grid, dim3(kThreads), 0, st, __VA_ARGS__);      \
      else                                                                                                       \
        hipLaunchKernelGGL((KERNEL<float, MR_COMB_STOCHASTIC>), grid, dim3(kThreads), 0, st, __VA_ARGS__);       \
    }                                                                                                            \
    MR_HIP(hipGetLastError());                                                                                   \
  } while (0)

// One sweep call's state: the validated arguments, the context view and the
// parameter table (host copy and its device twin).
struct Sweep {
  mr_view v;
  int kind = 0, n_params = 0;
  bool f64 = false;
  hipStream_t st = nullptr;
  SweepParams sp{};
  SweepTab tab{};
  Tmp<SweepTab> d_tab;

  // validation in mr_combine_device's order; fills the table's p / q / thr
  int open(mr_ctx* ctx, int kind_, int32_t n_params_, const double* params, uint64_t seed, int64_t pair_base,
           int64_t n_pairs, const void* ubm, const void* ibm) {
    if (!ctx || !params || !ubm || !ibm) return fail(MR_E_INVALID, "null argument");
    if (kind_ != MR_COMB_LINEAR && kind_ != MR_COMB_AGGREGATION && kind_ != MR_COMB_STOCHASTIC)
      return fail(MR_E_INVALID, "unknown combination kind %d", kind_);
    if (n_params_ < 1 || n_params_ > kSweepMax)
      return fail(MR_E_INVALID, "%d sweep parameters: 1 to %d", (int)n_params_, kSweepMax);
    for (int j = 0; j < n_params_; ++j)  // MR:366-369 / MR:434-437
      if (kind_ != MR_COMB_LINEAR && !(params[j] >= 0.0 && params[j] <= 1.0))
        return fail(MR_E_INVALID, "percentage/probability %g (parameter %d) must be between 0 and 1", params[j], j);
    int rc = mr_view_get(ctx, &v);
    if (rc) return rc;
    if (pair_base < 0 || n_pairs < 0) return fail(MR_E_INVALID, "negative pair_base / n_pairs");
    MR_HIP(hipSetDevice(v.device));
    kind = kind_;
    n_params = n_params_;
    f64 = v.out_dtype == MR_OUT_F64;
    st = (hipStream_t)v.stream;
    for (int j = 0; j < n_params; ++j) {
      tab.p[j] = params[j];
      tab.q[j] = 1.0 - params[j];
      tab.thr[j] = (long long)(params[j] * (double)n_pairs);  // (p * length).toInt, MR:371
      tab.mn[j] = INFINITY;
      tab.mx[j] = -INFINITY;
    }
    sp.n_te = v.n_test_users;
    sp.width = v.song_hi - v.song_lo;
    sp.song_lo = v.song_lo;
    sp.n_songs = v.n_songs;
    sp.n_params = n_params;
    sp.seed = (unsigned long long)seed;
    sp.pair_base = (long long)pair_base;
    sp.te_off = reinterpret_cast<const long long*>(v.te_off);
    sp.te_songs = v.te_songs;
    sp.ubm = ubm;
    sp.ibm = ibm;
    if (int rc_ = d_tab.alloc(1, st)) return rc_;
    sp.tab = d_tab.p;
    return MR_OK;
  }

  int upload() {  // the host table is read when the copy is queued or before the call's last wait
    MR_HIP(hipMemcpyAsync(d_tab.p, &tab, sizeof(SweepTab), hipMemcpyHostToDevice, st));
    return MR_OK;
  }

  // extremes of every out_j over the shard's pairs (+inf / -inf without one); waits
  int minmax(double* mn, double* mx) {
    for (int j = 0; j < n_params; ++j) { mn[j] = INFINITY; mx[j] = -INFINITY; }
    if (sp.width <= 0 || sp.n_te <= 0) return MR_OK;
    int rc = upload();
    if (rc) return rc;
    const int gx = (sp.width + kThreads * kCombPer - 1) / (kThreads * kCombPer);
    const int gy = std::max(1, std::min(sp.n_te, (8192 + gx - 1) / gx));
    const long long nblk = (long long)gx * gy;
    Tmp<double> part, out;
    if (int rc_ = part.alloc((size_t)nblk * n_params * 2, st)) return rc_;
    if (int rc_ = out.alloc((size_t)n_params * 2, st)) return rc_;
    SweepParams q = sp;
    q.part = part.p;
    MR_SWEEP_LAUNCH(k_sweep_minmax, f64, kind, dim3(gx, gy), st, q);
    hipLaunchKernelGGL(k_sweep_minmax2, dim3(n_params), dim3(kThreads), 0, st, part.p, nblk, n_params, out.p);
    MR_HIP(hipGetLastError());
    double h[kSweepMax * 2];
    MR_HIP(hipMemcpyAsync(h, out.p, (size_t)n_params * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    MR_HIP(hipStreamSynchronize(st));
    for (int j = 0; j < n_params; ++j) { mn[j] = h[2 * j]; mx[j] = h[2 * j + 1]; }
    return MR_OK;
  }

  // The label classes' counts of every parameter into counts[P][2][n_classes]
  // [n_thr] (device), groups of G parameters through one [G][width][n_thr]
  // scratch pair: each group is gathered into the class block before the next
  // reuses the scratch (stream order). mn / mx: the GLOBAL extremes. Waits.
  int class_counts(const double* mn, const double* mx, const int64_t* lab_off, const int32_t* lab_songs,
                   int32_t n_classes, const int32_t* classes, int32_t* counts, int n_thr) {
    for (int j = 0; j < n_params; ++j) {
      tab.mn[j] = mn[j];
      tab.mx[j] = mx[j];
      for (int t = 0; t < kThresholds; ++t) {
        const bool on = t < n_thr && mn[j] <= mx[j];  // no pair: nothing passes (NaN floor)
        tab.xt_f[j][t] = t >= n_thr ? INFINITY : on ? level_floor<float, uint32_t>(mn[j], mx[j], kThrHost[t]) : NAN;
        tab.xt_d[j][t] = t >= n_thr ? INFINITY : on ? level_floor<double, uint64_t>(mn[j], mx[j], kThrHost[t]) : NAN;
      }
    }
    const int width = sp.width, n_te = sp.n_te;
    std::vector<int32_t> lu, ls;
    int rc = label_pairs(n_te, lab_off, lab_songs, lu, ls);
    if (rc) return rc;
    const long long n_lab = lab_off[n_te];
    if ((rc = upload())) return rc;
    const size_t blk = (size_t)2 * n_classes * n_thr;  // one parameter's block
    if (width <= 0 || n_te <= 0) {  // no element: every count is 0
      if (blk) MR_HIP(hipMemsetAsync(counts, 0, blk * n_params * 4, st));
      MR_HIP(hipStreamSynchronize(st));
      return MR_OK;
    }
    Tmp<int> d_pred, d_tp, d_lu, d_ls, d_cls;
    const size_t nc = (size_t)kSweepG * width * n_thr;
    if (int rc_ = d_pred.alloc(nc, st)) return rc_;
    if (int rc_ = d_tp.alloc(nc, st)) return rc_;
    if (int rc_ = d_lu.alloc(lu.size(), st)) return rc_;
    if (int rc_ = d_ls.alloc(ls.size(), st)) return rc_;
    MR_HIP(hipMemcpyAsync(d_lu.p, lu.data(), lu.size() * 4, hipMemcpyHostToDevice, st));
    MR_HIP(hipMemcpyAsync(d_ls.p, ls.data(), ls.size() * 4, hipMemcpyHostToDevice, st));
    if (n_classes > 0) {
      if (int rc_ = d_cls.alloc((size_t)n_classes, st)) return rc_;
      MR_HIP(hipMemcpyAsync(d_cls.p, classes, (size_t)n_classes * 4, hipMemcpyHostToDevice, st));
    }
    // the workgroup shape of eval_counts: users split only when the songs alone give too few workgroups
    const int sx = (width + kThreads - 1) / kThreads;
    const int uy = std::max(1, std::min((n_te + 15) / 16, (1024 + sx - 1) / sx));
    SweepParams q = sp;
    q.n_thr = n_thr;
    q.users_per_block = (n_te + uy - 1) / uy;
    q.pred = d_pred.p;
    q.tp = d_tp.p;
    q.lab_u = d_lu.p;
    q.lab_s = d_ls.p;
    q.n_lab = n_lab;
    for (int j0 = 0; j0 < n_params; j0 += kSweepG) {
      const int ng = std::min(kSweepG, n_params - j0);
      if (uy > 1) MR_HIP(hipMemsetAsync(d_pred.p, 0, nc * 4, st));
      MR_HIP(hipMemsetAsync(d_tp.p, 0, nc * 4, st));
      MR_SWEEP_LAUNCH(k_sweep_pred, f64, kind, dim3(sx, uy), st, q, j0);
      if (n_lab > 0) {
        const int lb = (int)((n_lab + kThreads - 1) / kThreads);
        MR_SWEEP_LAUNCH(k_sweep_tp, f64, kind, dim3(lb), st, q, j0, ng);
      }
      for (int g = 0; g < ng && n_classes > 0; ++g) {
        const int n = n_classes * n_thr;
        hipLaunchKernelGGL(k_eval_gather, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, n_classes, n_thr,
                           v.song_lo, width, d_cls.p, d_pred.p + (size_t)g * width * n_thr,
                           d_tp.p + (size_t)g * width * n_thr, counts + (size_t)(j0 + g) * blk);
        MR_HIP(hipGetLastError());
      }
    }
    MR_HIP(hipStreamSynchronize(st));  // the host staging (table, labels, classes) has been read
    return MR_OK;
  }
};

int sweep_thresholds(int32_t n_thresholds, int* n_thr) {
  *n_thr = thresholds_or_default(n_thresholds);
  if (*n_thr != 10 && *n_thr != 11)
    return fail(MR_E_INVALID, "%d thresholds: 10 (MR:590) or 11 (distributed.scala:395)", *n_thr);
  return MR_OK;
}

}  // namespace

extern "C" {

int mr_combine_device(mr_ctx* ctx, int kind, double param, uint64_t seed, int64_t pair_base, int64_t n_pairs,
                      const void* ubm, const void* ibm, void* out) {
  if (!ctx || !ubm || !ibm || !out) return fail(MR_E_INVALID, "null argument");
  if (kind != MR_COMB_LINEAR && kind != MR_COMB_AGGREGATION && kind != MR_COMB_STOCHASTIC)
    return fail(MR_E_INVALID, "unknown combination kind %d", kind);
  // MR:366-369 / MR:434-437: the reference prints and calls System.exit(-1)
  if (kind != MR_COMB_LINEAR && !(param >= 0.0 && param <= 1.0))
    return fail(MR_E_INVALID, "percentage/probability %g must be between 0 and 1", param);
  mr_view v;
  int rc = mr_view_get(ctx, &v);
  if (rc) return rc;
  if (pair_base < 0 || n_pairs < 0) return fail(MR_E_INVALID, "negative pair_base / n_pairs");
  MR_HIP(hipSetDevice(v.device));
  const int width = v.song_hi - v.song_lo;
  CombParams cp{v.n_test_users, width, v.song_lo, v.n_songs, kind, param, (unsigned long long)seed,
                (long long)pair_base, (long long)(param * (double)n_pairs),  // (p * length).toInt, MR:371
                reinterpret_cast<const long long*>(v.te_off), v.te_songs, ubm, ibm, out};
  hipStream_t st = (hipStream_t)v.stream;
  const int rows = mr_internal::launch_rows(mr_internal::kGridRows);
  for (int y0 = 0; y0 < v.n_test_users; y0 += rows) {
    CombParams q = cp;
    const int ny = std::min(rows, v.n_test_users - y0);
    const size_t esz = v.out_dtype == MR_OUT_F64 ? 8 : 4;
    q.n_te = ny;
    q.te_off = cp.te_off + y0;  // values index the whole te_songs: pairs before user y0 + u are
    q.pair_base = cp.pair_base + (long long)y0 * v.n_songs;  // (y0 + u) * n_s - te_off[y0 + u]
    q.ubm = (const char*)ubm + (size_t)y0 * width * esz;
    q.ibm = (const char*)ibm + (size_t)y0 * width * esz;
    q.out = (char*)out + (size_t)y0 * width * esz;
    dim3 grid((width + kThreads * kCombPer - 1) / (kThreads * kCombPer), ny);
    if (v.out_dtype == MR_OUT_F64) hipLaunchKernelGGL(k_combine<double>, grid, dim3(kThreads), 0, st, q);
    else hipLaunchKernelGGL(k_combine<float>, grid, dim3(kThreads), 0, st, q);
    MR_HIP(hipGetLastError());
  }
  MR_HIP(hipStreamSynchronize(st));
  return MR_OK;
}

int mr_combine_all_device(mr_ctx* ctx, double alpha, double ibm_percentage, double ibm_probability, uint64_t seed,
                          int64_t pair_base, int64_t n_pairs, const void* ubm, const void* ibm, void* out_linear,
                          void* out_aggregation, void* out_stochastic, double* minmax) {
  if (!ctx || !ubm || !ibm || !out_linear || !out_aggregation || !out_stochastic)
    return fail(MR_E_INVALID, "null argument");
  // MR:366-369 / MR:434-437: the reference prints and calls System.exit(-1)
  if (!(ibm_percentage >= 0.0 && ibm_percentage <= 1.0) || !(ibm_probability >= 0.0 && ibm_probability <= 1.0))
    return fail(MR_E_INVALID, "percentage %g / probability %g must be between 0 and 1", ibm_percentage,
                ibm_probability);
  mr_view v;
  int rc = mr_view_get(ctx, &v);
  if (rc) return rc;
  if (pair_base < 0 || n_pairs < 0) return fail(MR_E_INVALID, "negative pair_base / n_pairs");
  MR_HIP(hipSetDevice(v.device));
  const int width = v.song_hi - v.song_lo;
  const size_t esz = v.out_dtype == MR_OUT_F64 ? 8 : 4;
  Comb3Params cp{v.n_test_users, width, v.song_lo, v.n_songs, alpha, ibm_probability, (unsigned long long)seed,
                 (long long)pair_base, (long long)(ibm_percentage * (double)n_pairs),  // (p * length).toInt, MR:371
                 reinterpret_cast<const long long*>(v.te_off), v.te_songs, ubm, ibm,
                 {out_linear, out_aggregation, out_stochastic}, nullptr};
  hipStream_t st = (hipStream_t)v.stream;
  const int gx = (width + kThreads * kCombPer - 1) / (kThreads * kCombPer);
  const long long nblk = (long long)gx * v.n_test_users;
  Tmp<double> part, part2;
  constexpr int kRed = 256;  // k_minmax6 blocks
  if (minmax && nblk > 0) {
    if (int rc_ = part.alloc((size_t)nblk * 6, st)) return rc_;
    if (int rc_ = part2.alloc((size_t)kRed * 6, st)) return rc_;
  }
  const int rows = mr_internal::launch_rows(mr_internal::kGridRows);
  for (int y0 = 0; gx > 0 && y0 < v.n_test_users; y0 += rows) {
    Comb3Params q = cp;
    const int ny = std::min(rows, v.n_test_users - y0);
    q.n_te = ny;
    q.te_off = cp.te_off + y0;  // values index the whole te_songs (see mr_combine_device)
    q.pair_base = cp.pair_base + (long long)y0 * v.n_songs;
    q.ubm = (const char*)ubm + (size_t)y0 * width * esz;
    q.ibm = (const char*)ibm + (size_t)y0 * width * esz;
    for (int c = 0; c < 3; ++c) q.out[c] = (char*)cp.out[c] + (size_t)y0 * width * esz;
    q.part = part.p ? part.p + (size_t)y0 * gx * 6 : nullptr;
    dim3 grid(gx, ny);
    if (v.out_dtype == MR_OUT_F64) hipLaunchKernelGGL(k_combine3<double>, grid, dim3(kThreads), 0, st, q);
    else hipLaunchKernelGGL(k_combine3<float>, grid, dim3(kThreads), 0, st, q);
    MR_HIP(hipGetLastError());
  }
  if (minmax) {
    double h[kRed * 6];
    for (int c = 0; c < 6; ++c) minmax[c] = (c & 1) ? -INFINITY : INFINITY;
    if (nblk > 0) {
      hipLaunchKernelGGL(k_minmax6, dim3(kRed), dim3(kThreads), 0, st, part.p, nblk, part2.p);
      MR_HIP(hipGetLastError());
      MR_HIP(hipMemcpyAsync(h, part2.p, sizeof h, hipMemcpyDeviceToHost, st));
      MR_HIP(hipStreamSynchronize(st));
      for (int b = 0; b < kRed; ++b)
        for (int c = 0; c < 6; ++c)
          minmax[c] = (c & 1) ? std::fmax(minmax[c], h[b * 6 + c]) : std::fmin(minmax[c], h[b * 6 + c]);
    }
  }
  MR_HIP(hipStreamSynchronize(st));
  return MR_OK;
}

int mr_eval_minmax_device(mr_ctx* ctx, const void* dense, double* mn, double* mx) {
  if (!ctx || !dense || !mn || !mx) return fail(MR_E_INVALID, "null argument");
  mr_view v;
  int rc = mr_view_get(ctx, &v);
  if (rc) return rc;
  MR_HIP(hipSetDevice(v.device));
  const long long n = (long long)v.n_test_users * (v.song_hi - v.song_lo);
  const int blocks = (int)std::max<long long>(1, std::min<long long>(4096, (n + kThreads - 1) / kThreads));
  hipStream_t st = (hipStream_t)v.stream;
  Tmp<double> part;
  if (int rc_ = part.alloc((size_t)blocks * 2, st)) return rc_;
  if (v.out_dtype == MR_OUT_F64)
    hipLaunchKernelGGL(k_minmax<double>, dim3(blocks), dim3(kThreads), 0, st, (const double*)dense, n, part.p);
  else
    hipLaunchKernelGGL(k_minmax<float>, dim3(blocks), dim3(kThreads), 0, st, (const float*)dense, n, part.p);
  MR_HIP(hipGetLastError());
  std::vector<double> h((size_t)blocks * 2);
  MR_HIP(hipMemcpyAsync(h.data(), part.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  MR_HIP(hipStreamSynchronize(st));
  double a = INFINITY, b = -INFINITY;
  for (int i = 0; i < blocks; ++i) {
    a = std::fmin(a, h[2 * i]);
    b = std::fmax(b, h[2 * i + 1]);
  }
  *mn = a;
  *mx = b;
  return MR_OK;
}

int mr_eval_counts_device(mr_ctx* ctx, const void* dense, double mn, double mx, const int64_t* lab_off,
                          const int32_t* lab_songs, int32_t* pred_counts, int32_t* tp_counts, int32_t n_thresholds) {
  if (!pred_counts || !tp_counts) return fail(MR_E_INVALID, "null argument");
  const int n_thr = thresholds_or_default(n_thresholds);
  mr_view v;
  Tmp<int> d_pred, d_tp;
  int rc = eval_counts(ctx, 1, &dense, &mn, &mx, lab_off, lab_songs, n_thr, v, d_pred, d_tp, [](int) { return 0; });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)v.stream;
  const size_t nc = (size_t)(v.song_hi - v.song_lo) * n_thr;
  MR_HIP(hipMemcpyAsync(pred_counts, d_pred.p, nc * 4, hipMemcpyDeviceToHost, st));
  MR_HIP(hipMemcpyAsync(tp_counts, d_tp.p, nc * 4, hipMemcpyDeviceToHost, st));
  MR_HIP(hipStreamSynchronize(st));
  return MR_OK;
}

int mr_eval_map_device(mr_ctx* ctx, const void* dense, double mn, double mx, const int64_t* lab_off,
                       const int32_t* lab_songs, const int32_t* pos, int32_t n_label_songs, double* map_out,
                       int32_t n_thresholds) {
  if (!pos || !map_out) return fail(MR_E_INVALID, "null argument");
  const int n_thr = thresholds_or_default(n_thresholds);
  mr_view v;
  Tmp<int> d_pred, d_tp;
  int rc = eval_counts(ctx, 1, &dense, &mn, &mx, lab_off, lab_songs, n_thr, v, d_pred, d_tp, [](int) { return 0; });
  if (rc) return rc;
  hipStream_t st = (hipStream_t)v.stream;
  const int width = v.song_hi - v.song_lo;
  // Only the label classes (pos > 0, ascending) cross PCIe: their ids and
  // counts in, their AP out (C5: ~1/10 of the shard's songs).
  std::vector<int32_t> cls, cpos;
  for (int g = 0; g < width; ++g)
    if (pos[v.song_lo + g] > 0) { cls.push_back(g); cpos.push_back(pos[v.song_lo + g]); }
  const int nc = (int)cls.size();
  Tmp<int> d_cls, d_cpos;
  Tmp<double> d_ap;
  std::vector<double> ap((size_t)std::max(1, nc));
  if (nc > 0) {
    if (int rc_ = d_cls.alloc((size_t)nc, st)) return rc_;
    if (int rc_ = d_cpos.alloc((size_t)nc, st)) return rc_;
    if (int rc_ = d_ap.alloc((size_t)nc, st)) return rc_;
    MR_HIP(hipMemcpyAsync(d_cls.p, cls.data(), (size_t)nc * 4, hipMemcpyHostToDevice, st));
    MR_HIP(hipMemcpyAsync(d_cpos.p, cpos.data(), (size_t)nc * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_eval_ap, dim3((nc + kThreads - 1) / kThreads), dim3(kThreads), 0, st, nc, n_thr, d_cls.p,
                       d_cpos.p, d_pred.p, d_tp.p, d_ap.p);
    MR_HIP(hipGetLastError());
    MR_HIP(hipMemcpyAsync(ap.data(), d_ap.p, (size_t)nc * 8, hipMemcpyDeviceToHost, st));
  }
  MR_HIP(hipStreamSynchronize(st));
  double total = 0.0;  // classes in song-id order, as mr_eval_map (MR:625-627)
  for (int c = 0; c < nc; ++c) total += ap[c];
  *map_out = n_label_songs > 0 ? total / (double)n_label_songs : NAN;
  return MR_OK;
}

int mr_eval_class_counts_device(mr_ctx* ctx, int32_t n_models, const void* const* dense, const double* mn,
                                const double* mx, const int64_t* lab_off, const int32_t* lab_songs, int32_t n_classes,
                                const int32_t* classes, int32_t* counts, int32_t n_thresholds) {
  if (!counts || (n_classes > 0 && !classes) || n_classes < 0) return fail(MR_E_INVALID, "null argument");
  for (int32_t c = 1; c < n_classes; ++c)
    if (classes[c] <= classes[c - 1]) return fail(MR_E_INVALID, "classes not strictly ascending at %d", (int)c);
  const int n_thr = thresholds_or_default(n_thresholds);
  mr_view v;
  Tmp<int> d_pred, d_tp, d_cls;
  const size_t blk = (size_t)2 * n_classes * n_thr;  // one model's block
  auto gather = [&](int i) -> int {
    if (n_classes == 0) return 0;
    hipStream_t st = (hipStream_t)v.stream;
    if (!d_cls.p) {  // the class list, staged once (after eval_counts resolved the context)
      if (int rc_ = d_cls.alloc((size_t)n_classes, st)) return rc_;
      MR_HIP(hipMemcpyAsync(d_cls.p, classes, (size_t)n_classes * 4, hipMemcpyHostToDevice, st));
    }
    const int n = n_classes * n_thr;
    hipLaunchKernelGGL(k_eval_gather, dim3((n + kThreads - 1) / kThreads), dim3(kThreads), 0, st, n_classes, n_thr,
                       v.song_lo, v.song_hi - v.song_lo, d_cls.p, d_pred.p, d_tp.p, counts + (size_t)i * blk);
    MR_HIP(hipGetLastError());
    return 0;
  };
  int rc = eval_counts(ctx, n_models, dense, mn, mx, lab_off, lab_songs, n_thr, v, d_pred, d_tp, gather);
  if (rc) return rc;
  MR_HIP(hipStreamSynchronize((hipStream_t)v.stream));  // the host staging (labels, classes) has been read
  return MR_OK;
}

int mr_eval_map_counts_device(mr_ctx* ctx, int32_t n_models, int32_t n_classes, const int32_t* class_pos,
                              const int32_t* counts, int32_t n_label_songs, double* maps_out, int32_t n_thresholds) {
  if (!ctx || !maps_out || n_models < 1 || n_classes < 0 || (n_classes > 0 && (!class_pos || !counts)))
    return fail(MR_E_INVALID, "null argument");
  for (int32_t c = 0; c < n_classes; ++c)
    if (class_pos[c] <= 0) return fail(MR_E_INVALID, "class %d has no positive (pos %d)", (int)c, (int)class_pos[c]);
  const int n_thr = thresholds_or_default(n_thresholds);
  if (n_thr != 10 && n_thr != 11)
    return fail(MR_E_INVALID, "%d thresholds: 10 (MR:590) or 11 (distributed.scala:395)", n_thr);
  mr_view v;
  int rc = mr_view_get(ctx, &v);
  if (rc) return rc;
  MR_HIP(hipSetDevice(v.device));
  hipStream_t st = (hipStream_t)v.stream;
  const size_t nap = (size_t)n_models * n_classes;
  std::vector<double> ap(std::max<size_t>(1, nap));
  if (n_classes > 0) {
    // every model's classes as one launch: AP row m * n_classes + c reads
    // model m's block, pred at [m][0][c][t], tp at [m][1][c][t] — tp is the
    // pred pointer + n_classes * n_thr, so index the classes of model m as
    // m * 2 * n_classes + c
    std::vector<int32_t> cls(nap), cpos(nap);
    for (int m = 0; m < n_models; ++m)
      for (int c = 0; c < n_classes; ++c) {
        cls[(size_t)m * n_classes + c] = 2 * m * n_classes + c;
        cpos[(size_t)m * n_classes + c] = class_pos[c];
      }
    Tmp<int> d_cls, d_cpos;
    Tmp<double> d_ap;
    if (int rc_ = d_cls.alloc(nap, st)) return rc_;
    if (int rc_ = d_cpos.alloc(nap, st)) return rc_;
    if (int rc_ = d_ap.alloc(nap, st)) return rc_;
    MR_HIP(hipMemcpyAsync(d_cls.p, cls.data(), nap * 4, hipMemcpyHostToDevice, st));
    MR_HIP(hipMemcpyAsync(d_cpos.p, cpos.data(), nap * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_eval_ap, dim3((unsigned)((nap + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (int)nap,
                       n_thr, d_cls.p, d_cpos.p, counts, counts + (size_t)n_classes * n_thr, d_ap.p);
    MR_HIP(hipGetLastError());
    MR_HIP(hipMemcpyAsync(ap.data(), d_ap.p, nap * 8, hipMemcpyDeviceToHost, st));
  }
  MR_HIP(hipStreamSynchronize(st));
  for (int m = 0; m < n_models; ++m) {
    double total = 0.0;  // classes in song-id order, as mr_eval_map (MR:625-627)
    for (int c = 0; c < n_classes; ++c) total += ap[(size_t)m * n_classes + c];
    maps_out[m] = n_label_songs > 0 ? total / (double)n_label_songs : NAN;
  }
  return MR_OK;
}

int mr_sweep_minmax_device(mr_ctx* ctx, int kind, int32_t n_params, const double* params, uint64_t seed,
                           int64_t pair_base, int64_t n_pairs, const void* ubm, const void* ibm, double* mn,
                           double* mx) {
  if (!mn || !mx) return fail(MR_E_INVALID, "null argument");
  Sweep s;
  int rc = s.open(ctx, kind, n_params, params, seed, pair_base, n_pairs, ubm, ibm);
  if (rc) return rc;
  return s.minmax(mn, mx);
}

int mr_sweep_class_counts_device(mr_ctx* ctx, int kind, int32_t n_params, const double* params, uint64_t seed,
                                 int64_t pair_base, int64_t n_pairs, const void* ubm, const void* ibm,
                                 const double* mn, const double* mx, const int64_t* lab_off,
                                 const int32_t* lab_songs, int32_t n_classes, const int32_t* classes,
                                 int32_t* counts, int32_t n_thresholds) {
  if (!mn || !mx || !lab_off || !counts || (n_classes > 0 && !classes) || n_classes < 0)
    return fail(MR_E_INVALID, "null argument");
  for (int32_t c = 1; c < n_classes; ++c)
    if (classes[c] <= classes[c - 1]) return fail(MR_E_INVALID, "classes not strictly ascending at %d", (int)c);
  int n_thr;
  int rc = sweep_thresholds(n_thresholds, &n_thr);
  if (rc) return rc;
  Sweep s;
  if ((rc = s.open(ctx, kind, n_params, params, seed, pair_base, n_pairs, ubm, ibm))) return rc;
  return s.class_counts(mn, mx, lab_off, lab_songs, n_classes, classes, counts, n_thr);
}

int mr_sweep_map_device(mr_ctx* ctx, int kind, int32_t n_params, const double* params, uint64_t seed,
                        int64_t pair_base, int64_t n_pairs, const void* ubm, const void* ibm, const int64_t* lab_off,
                        const int32_t* lab_songs, const int32_t* pos, int32_t n_label_songs, double* maps_out,
                        double* minmax_out, int32_t n_thresholds) {
  if (!lab_off || !pos || !maps_out) return fail(MR_E_INVALID, "null argument");
  int n_thr;
  int rc = sweep_thresholds(n_thresholds, &n_thr);
  if (rc) return rc;
  Sweep s;
  if ((rc = s.open(ctx, kind, n_params, params, seed, pair_base, n_pairs, ubm, ibm))) return rc;
  double mn[kSweepMax], mx[kSweepMax];
  if ((rc = s.minmax(mn, mx))) return rc;
  for (int j = 0; minmax_out && j < n_params; ++j) {
    minmax_out[2 * j] = mn[j];
    minmax_out[2 * j + 1] = mx[j];
  }
  for (int j = 0; j < n_params; ++j) {
    if (!(mn[j] <= mx[j]))  // the reference throws here (MR:524)
      return fail(MR_E_INVALID, "parameter %d (%g): the model has no pairs, min/max undefined", j, params[j]);
  }
  // the label classes (pos > 0, ascending) of the context's songs, as mr_eval_map_device
  std::vector<int32_t> cls, cpos;
  for (int g = s.v.song_lo; g < s.v.song_hi; ++g)
    if (pos[g] > 0) { cls.push_back(g); cpos.push_back(pos[g]); }
  const int nc = (int)cls.size();
  Tmp<int> d_counts;
  const size_t n = std::max<size_t>(1, (size_t)n_params * 2 * nc * n_thr);
  if (int rc_ = d_counts.alloc(n, s.st)) return rc_;
  if ((rc = s.class_counts(mn, mx, lab_off, lab_songs, nc, cls.data(), d_counts.p, n_thr))) return rc;
  return mr_eval_map_counts_device(ctx, n_params, nc, cpos.data(), d_counts.p, n_label_songs, maps_out, n_thr);
}

}  // extern "C"
