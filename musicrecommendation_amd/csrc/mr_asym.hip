// mr_asym.hip — the asymmetric-cosine, locality-q item-based model
// (mr_ibm_asym_device, mr_asym_tables; include/mr_engine.h): the neighbourhood
// method of the Million Song Dataset Challenge literature,
//   score(u, s) = Σ_{s2 ∈ T(u)} ( C(s, s2) / (c(s)^alpha * c(s2)^(1-alpha)) )^q,
// which at alpha = 0.5, q = 1 is the reference's ItemBasedModel (MR:230-257).
//
// k_asym_score: one 1024-thread workgroup per (song sub-range, test user).
//   1. u32 counters in LDS cover the sub-range (at most kAsymMaxSub songs; a
//      wider tile is cut into several sub-ranges, each its own workgroup that
//      walks the tile's lists and keeps the ids of its range);
//   2. the fp64 accumulators live in registers: thread tid owns the songs
//      tid + j * 1024 of the sub-range, j < kAsymAcc;
//   3. for each s2 of T(u), ascending (te_off / te_songs): the workgroup walks
//      the train listeners L_tr(s2) through the tile-major train CSR with the
//      shared walk_tile_lists (csrc/mr_tile_walk.h) in its 2-byte segment-load
//      form, as k_similar_count does (LDS adds without a returned value), then
//      after a barrier every thread folds t = w^q, w = (double)C / (pow_a[s] *
//      pow_b[s2]), into its accumulators for its songs with C >= 1 and clears
//      the counters it read (so the next s2 starts from zero), then a barrier;
//   4. the heard songs of the range are marked in the (zero) counters and the
//      row is stored coalesced, NaN where heard.
// The counts are integer sums (order-free); the fold order is the order of
// T(u); every fp64 operation is a single IEEE *, / or + (no pow, no
// contraction): the result is a pure function of the dataset, alpha, q and
// the columns held, bit-equal to evaluation.asym_item_model.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "mr_engine.h"
#include "mr_hip_util.h"
#include "mr_internal.h"
#include "mr_tile_walk.h"

namespace {

using mr_hip::Drain;
using mr_hip::Tmp;
using mr_host::fail;

constexpr int kAsymThreads = 1024;
constexpr int kAsymR = 2;          // listeners per thread and iteration
constexpr int kAsymSeg = 4;        // segment ids loaded together
constexpr int kAsymAcc = 8;        // fp64 accumulators per thread
constexpr int kAsymMaxSub = kAsymThreads * kAsymAcc;  // songs per sub-range: 32 KiB of u32 counters
constexpr int kAsymMaxBatch = mr_internal::kGridRows;  // test users per launch (grid y)

struct AsymParams {
  int n_tr, song_lo, song_hi, block_songs, sub, n_sub;  // sub: songs per sub-range, n_sub: sub-ranges per tile
  int q, f64, user0;
  const long long* trs_off;
  const int* trs_users;
  const int* toff;
  const unsigned short* tsongs;
  const long long* te_off;
  const int* te_songs;
  const double* pow_a;  // c(s)^alpha [n_s]
  const double* pow_b;  // c(s)^(1-alpha) [n_s]
  void* out;            // [n_te][width] of the context's out_dtype
};

// (8 waves per SIMD = at most 64 VGPRs: two workgroups share a CU, one walks while the other folds)
__global__ __launch_bounds__(kAsymThreads, 8) void k_asym_score(AsymParams p) {
  __shared__ unsigned asym_cnt[kAsymMaxSub];
  constexpr int NT = kAsymThreads, R = kAsymR;
  const int tid = threadIdx.x;
  const SubRange g = sub_range(blockIdx.x, p.n_sub, p.sub, p.song_lo, p.song_hi, p.block_songs);
  const int s0 = g.s0, sw = g.sw;
  const int u = p.user0 + blockIdx.y;
  const int width = p.song_hi - p.song_lo;
  if (s0 >= g.bw) return;  // (block-uniform) the last tile is partial: no such sub-range
  const int* toff_t = p.toff + (size_t)g.tile * p.n_tr;
  const long long t0 = p.te_off[u], t1 = p.te_off[u + 1];

  const double* pow_a = p.pow_a + g.blo + s0;  // the sub-range's c(s)^alpha, read only where C >= 1
  double acc[kAsymAcc];
#pragma unroll
  for (int j = 0; j < kAsymAcc; ++j) acc[j] = 0.0;
  for (int i = tid; i < sw; i += NT) asym_cnt[i] = 0u;
  __syncthreads();

  auto add = [&](unsigned x, unsigned) {
    const unsigned loc = x - (unsigned)s0;
    if (loc < (unsigned)sw)  // result unused: an LDS add without return
      (void)__hip_atomic_fetch_add(&asym_cnt[loc], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  };

  for (long long ti = t0; ti < t1; ++ti) {  // T(u) ascending: the fold order
    const int s2 = p.te_songs[ti];
    const long long l0 = p.trs_off[s2];
    const int n = (int)(p.trs_off[s2 + 1] - l0);
    if (n == 0) continue;  // (block-uniform) no train listener: every C is 0, every term +0.0
    const int* lst = p.trs_users + l0;
    const double pb = p.pow_b[s2];

    auto load_list = [&](int k0, int (&v)[R], unsigned (&w)[R]) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = k0 + r * NT;
        v[r] = k < n ? lst[k] : -1;
        w[r] = 1u;
      }
    };
    walk_tile_lists<NT, R, kAsymSeg, unsigned, false>(tid, n, load_list, toff_t, p.tsongs, add);
    __syncthreads();
    // t = w^q by q - 1 multiplications, w = C / (c(s)^alpha * c(s2)^(1-alpha)); acc = acc + t
#pragma unroll
    for (int j = 0; j < kAsymAcc; ++j) {
      const int i = tid + j * NT;
      if (i < sw) {
        const unsigned c = asym_cnt[i];
        if (c != 0u) {
          asym_cnt[i] = 0u;  // this thread alone reads and clears counter i
          acc[j] = acc[j] + asym_weight(c, pow_a[i] * pb, p.q);
        }
      }
    }
    __syncthreads();  // the next s2 adds into the cleared counters
  }

  // the heard songs of this sub-range (the counters are all zero here)
  for (long long i = t0 + tid; i < t1; i += NT) {
    const unsigned loc = (unsigned)(p.te_songs[i] - (g.blo + s0));
    if (loc < (unsigned)sw) asym_cnt[loc] = 1u;
  }
  __syncthreads();
  const size_t o = (size_t)u * (size_t)width + (size_t)(g.blo + s0 - p.song_lo);
#pragma unroll
  for (int j = 0; j < kAsymAcc; ++j) {
    const int i = tid + j * NT;
    if (i < sw) store_model_value(p.out, p.f64, o + i, asym_cnt[i] != 0u, acc[j]);
  }
}

}  // namespace

extern "C" {

int mr_asym_tables(double alpha, int32_t n, const int32_t* counts, double* pow_a, double* pow_b) {
  if (!(alpha >= 0.0 && alpha <= 1.0)) return fail(MR_E_INVALID, "alpha=%g must be in [0,1]", alpha);
  if (n < 0) return fail(MR_E_INVALID, "n=%d must not be negative", n);
  if (!counts || !pow_a || !pow_b) return fail(MR_E_INVALID, "null argument");
  for (int32_t i = 0; i < n; ++i) {
    const double cd = (double)counts[i];
    if (alpha == 0.5) {
      pow_a[i] = pow_b[i] = std::sqrt(cd);  // the scoring's sqrt_c
    } else if (alpha == 0.0) {
      pow_a[i] = 1.0;
      pow_b[i] = cd;
    } else if (alpha == 1.0) {
      pow_a[i] = cd;
      pow_b[i] = 1.0;
    } else {
      pow_a[i] = std::pow(cd, alpha);
      pow_b[i] = std::pow(cd, 1.0 - alpha);
    }
  }
  return MR_OK;
}

int mr_ibm_asym_device(mr_ctx* ctx, double alpha, int32_t q, void* dense_dev) {
  if (!ctx) return fail(MR_E_INVALID, "null context");
  int rc = mr_hip::check_asym_args(alpha, q);
  if (rc) return rc;
  if (!dense_dev) return fail(MR_E_INVALID, "null dense_dev");
  mr_internal::ShardTables t;
  if ((rc = mr_internal::shard_tables(ctx, "asymmetric item-based model", &t))) return rc;
  const int width = t.song_hi - t.song_lo;
  if (t.n_te <= 0 || width <= 0) return MR_OK;

  std::vector<double> pow_a((size_t)t.n_s), pow_b((size_t)t.n_s);
  if ((rc = mr_asym_tables(alpha, t.n_s, t.song_count, pow_a.data(), pow_b.data()))) return rc;

  MR_HIP(hipSetDevice(t.device));
  hipStream_t st = (hipStream_t)t.stream;
  Drain drain;
  drain.st = st;
  Tmp<double> d_a, d_b;
  if ((rc = d_a.alloc((size_t)t.n_s, st)) || (rc = d_b.alloc((size_t)t.n_s, st))) return rc;
  MR_HIP(hipMemcpyAsync(d_a.p, pow_a.data(), (size_t)t.n_s * 8, hipMemcpyHostToDevice, st));
  MR_HIP(hipMemcpyAsync(d_b.p, pow_b.data(), (size_t)t.n_s * 8, hipMemcpyHostToDevice, st));

  // MR_ASYM_SUB (diagnostic): a smaller sub-range, so that small tiles take the multi-sub-range path
  const int sub = std::min(t.block_songs, mr_hip::env_clamped("MR_ASYM_SUB", 64, kAsymMaxSub));
  const int n_sub = (t.block_songs + sub - 1) / sub;
  const int rows = mr_internal::launch_rows(kAsymMaxBatch);  // (MR_LAUNCH_ROWS, diagnostic: fewer users per launch)
  for (int u0 = 0; u0 < t.n_te; u0 += rows) {
    const int nb = std::min(rows, t.n_te - u0);
    AsymParams ap{t.n_tr,    t.song_lo,   t.song_hi, t.block_songs, sub,      n_sub,      q,     t.f64, u0,
                  t.trs_off, t.trs_users, t.toff,    t.tsongs,      t.te_off, t.te_songs, d_a.p, d_b.p, dense_dev};
    hipLaunchKernelGGL(k_asym_score, dim3(t.n_tiles * n_sub, nb), dim3(kAsymThreads), 0, st, ap);
    MR_HIP(hipGetLastError());
  }
  MR_HIP(hipStreamSynchronize(st));
  return MR_OK;
}

}  // extern "C"
