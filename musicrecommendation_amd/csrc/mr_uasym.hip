// mr_uasym.hip — the asymmetric-cosine, locality-q user-based model
// (mr_ubm_asym_device; include/mr_engine.h): the user-based half of the
// Million Song Dataset Challenge's neighbourhood method,
//   score(u, s) = Σ_{v ∈ L_tr(s)} ( |T(u) ∩ S(v)| / (|u|^alpha * |v|^(1-alpha)) )^q,
// defined the way the engine's own ubm is: the per-neighbour weight is computed
// in fp64, quantised once to a fixed-point integer and summed in int64, so that
// the result has no summation order. At alpha = 0.5, q = 1 and the context's
// frac_bits it is mr_run(MR_UBM)'s dense model bit for bit.
//
// k_uasym_weights: one 512-thread workgroup per (train-user chunk, test user).
//   1. u32 overlap counters in LDS cover the chunk's train users (internal
//      ids [c * chunk, (c + 1) * chunk));
//   2. wave w takes the songs s2 of T(u) with index = w (mod 8): the part of
//      L_tr(s2) inside the chunk is a contiguous range of the ascending list
//      (two wave-uniform binary searches; none when there is one chunk), which
//      the lanes walk with LDS adds without a returned value;
//   3. after a barrier every v with y >= 1 gets its key,
//        w = (double)y / (pa[u] * pb[v]) (0.0 for a zero denominator),
//        t = w, q - 1 times t = t * w, key = (int64)rint(t * 2^F),
//      and (v, key) is written compacted in ascending v by ballot rank
//      (k_neighbours' layout): user row r of the batch owns n_tr slots, chunk
//      c's list starts at slot c * chunk, its length is nbr_cnt[r][c].
// k_uasym_score: one 1024-thread workgroup per (song sub-range, test user).
//   1. int64 accumulators in LDS cover the sub-range (at most kUasymMaxSub
//      songs; a wider tile is cut into several sub-ranges, each its own
//      workgroup that walks the tile's rows and keeps the ids of its range);
//   2. thread tid takes the neighbours tid, tid + 1024, ... of every chunk's
//      list and walks the neighbour's row of the tile-major train CSR (toff /
//      tsongs) with the shared walk_tile_row (csrc/mr_tile_walk.h), adding the
//      key with a 64-bit LDS add without a returned value;
//   3. the heard songs of the range are marked and the row is stored
//      coalesced: (double)acc * 2^-F, NaN where heard (f32: rounded once).
// The overlaps and the scores are integer sums (order-free); every fp64
// operation is a single IEEE *, / or rint (no pow, no contraction): the result
// is a pure function of the dataset, alpha, q, F and the columns held,
// bit-equal to evaluation.asym_user_model.
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
using mr_hip::env_clamped;
using mr_hip::Tmp;
using mr_host::fail;

constexpr int kUwThreads = 512;                 // k_uasym_weights
constexpr int kUwWaves = kUwThreads / 64;
constexpr int kUasymChunk = 8192;               // train users per chunk: 32 KiB of u32 counters
constexpr int kUsThreads = 1024;                // k_uasym_score
constexpr int kUsSeg = 4;                       // segment ids loaded together
constexpr int kUasymMaxSub = 8192;              // songs per sub-range: 64 KiB of int64 accumulators
constexpr int kUasymMaxBatch = mr_internal::kGridRows;  // test users per launch (grid y)
constexpr unsigned long long kHeard = 0x8000000000000000ull;  // no sum reaches it (headroom rule)

struct UwParams {
  int n_tr, chunk, n_chunks, q;
  int u0, r0;  // first test user of the batch, first batch row of this launch
  double two_f;
  const long long* te_off;
  const int* te_songs;
  const long long* trs_off;
  const int* trs_users;
  const double* pa;  // te_len[u]^alpha [n_te]
  const double* pb;  // tr_len[v]^(1-alpha) [n_tr], v the context's train id
  int* nbr_v;        // [batch][n_tr]: chunk c's list at c * chunk
  long long* nbr_key;
  int* nbr_cnt;      // [batch][n_chunks]
};

// First index in the ascending trs_users[lo, hi) whose user is >= v.
__device__ __forceinline__ long long uasym_lower_bound(const int* trs_users, long long lo, long long hi, int v) {
  while (lo < hi) {
    const long long m = (lo + hi) >> 1;
    if (trs_users[m] < v) lo = m + 1; else hi = m;
  }
  return lo;
}

__global__ __launch_bounds__(kUwThreads) void k_uasym_weights(UwParams p) {
  __shared__ unsigned uw_cnt[kUasymChunk];
  __shared__ int uw_scan[kUwWaves];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = blockIdx.x;
  const int bu = p.r0 + blockIdx.y, u = p.u0 + bu;
  const int cv0 = c * p.chunk, cv1 = min(p.n_tr, cv0 + p.chunk), cw = cv1 - cv0;
  for (int i = tid; i < cw; i += kUwThreads) uw_cnt[i] = 0u;
  __syncthreads();

  const long long t0 = p.te_off[u], t1 = p.te_off[u + 1];
  for (long long ti = t0 + w; ti < t1; ti += kUwWaves) {  // (wave-uniform) one song of T(u) per wave
    const int s2 = p.te_songs[ti];
    long long lo = p.trs_off[s2], hi = p.trs_off[s2 + 1];
    if (p.n_chunks > 1) {  // the chunk's part of the ascending list
      lo = uasym_lower_bound(p.trs_users, lo, hi, cv0);
      hi = uasym_lower_bound(p.trs_users, lo, hi, cv1);
    }
    for (long long k = lo + lane; k < hi; k += 64) {
      const unsigned loc = (unsigned)(p.trs_users[k] - cv0);
      if (loc < (unsigned)cw)  // result unused: an LDS add without return
        (void)__hip_atomic_fetch_add(&uw_cnt[loc], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
  __syncthreads();

  // Compaction, order kept: wave w owns a contiguous span of the chunk (a
  // multiple of 64 ids), counts its non-zeros by ballot, one scan of the wave
  // totals, then writes by ballot rank.
  const double pa_u = p.pa[u];
  int* out_v = p.nbr_v + (size_t)bu * p.n_tr + cv0;
  long long* out_k = p.nbr_key + (size_t)bu * p.n_tr + cv0;
  const int span = (cw + kUwThreads - 1) / kUwThreads * 64;
  const int wb = min(cw, w * span), we = min(cw, wb + span);
  int nz = 0;
  for (int i0 = wb; i0 < we; i0 += 64) {
    const int i = i0 + lane;
    nz += __popcll(__ballot(i < we && uw_cnt[i] != 0u));
  }
  if (lane == 0) uw_scan[w] = nz;
  __syncthreads();
  int base = 0, written = 0;
#pragma unroll
  for (int x = 0; x < kUwWaves; ++x) {
    base += x < w ? uw_scan[x] : 0;
    written += uw_scan[x];
  }
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  for (int i0 = wb; i0 < we; i0 += 64) {
    const int i = i0 + lane;
    const unsigned y = i < we ? uw_cnt[i] : 0u;
    const unsigned long long m = __ballot(y != 0u);
    if (y != 0u) {
      const int pos = base + __popcll(m & below);
      const int v = cv0 + i;
      out_v[pos] = v;
      out_k[pos] = (long long)rint(asym_weight(y, pa_u * p.pb[v], p.q) * p.two_f);
    }
    base += __popcll(m);
  }
  if (tid == 0) p.nbr_cnt[(size_t)bu * p.n_chunks + c] = written;
}

struct UsParams {
  int n_tr, song_lo, song_hi, block_songs, sub, n_sub;  // sub: songs per sub-range, n_sub: sub-ranges per tile
  int chunk, n_chunks, f64;
  int u0, r0;  // first test user of the batch, first batch row of this launch
  double inv_f;
  const int* toff;
  const unsigned short* tsongs;
  const long long* te_off;
  const int* te_songs;
  const int* nbr_v;
  const long long* nbr_key;
  const int* nbr_cnt;
  void* out;  // [n_te][width] of the context's out_dtype
};

__global__ __launch_bounds__(kUsThreads) void k_uasym_score(UsParams p) {
  __shared__ unsigned long long us_acc[kUasymMaxSub];
  constexpr int NT = kUsThreads;
  const int tid = threadIdx.x;
  const SubRange g = sub_range(blockIdx.x, p.n_sub, p.sub, p.song_lo, p.song_hi, p.block_songs);
  const int s0 = g.s0, sw = g.sw;
  const int bu = p.r0 + blockIdx.y, u = p.u0 + bu;
  const int width = p.song_hi - p.song_lo;
  if (s0 >= g.bw) return;  // (block-uniform) the last tile is partial: no such sub-range
  const int* toff_t = p.toff + (size_t)g.tile * p.n_tr;
  for (int i = tid; i < sw; i += NT) us_acc[i] = 0ull;
  __syncthreads();

  for (int c = 0; c < p.n_chunks; ++c) {  // the written prefix of every chunk's list
    const int n = p.nbr_cnt[(size_t)bu * p.n_chunks + c];
    const int* lv = p.nbr_v + (size_t)bu * p.n_tr + (size_t)c * p.chunk;
    const long long* lk = p.nbr_key + (size_t)bu * p.n_tr + (size_t)c * p.chunk;
    for (int i = tid; i < n; i += NT) {
      const unsigned long long key = (unsigned long long)lk[i];
      if (key == 0ull) continue;  // a weight below 2^-(F+1): contributes nothing
      const int v = lv[i];
      // the neighbour's row of the tile, un-pipelined (csrc/mr_tile_walk.h)
      walk_tile_row<kUsSeg>(toff_t[v], toff_t[v + 1], p.tsongs, [&](unsigned x) {
        const unsigned loc = x - (unsigned)s0;
        if (loc < (unsigned)sw)  // result unused: a 64-bit LDS add without return
          (void)__hip_atomic_fetch_add(&us_acc[loc], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      });
    }
  }
  __syncthreads();

  // the heard songs of this sub-range
  const long long t0 = p.te_off[u], t1 = p.te_off[u + 1];
  for (long long i = t0 + tid; i < t1; i += NT) {
    const unsigned loc = (unsigned)(p.te_songs[i] - (g.blo + s0));
    if (loc < (unsigned)sw) us_acc[loc] = kHeard;
  }
  __syncthreads();
  const size_t o = (size_t)u * (size_t)width + (size_t)(g.blo + s0 - p.song_lo);
  for (int i = tid; i < sw; i += NT) {
    const unsigned long long a = us_acc[i];
    store_model_value(p.out, p.f64, o + i, a == kHeard, (double)(long long)a * p.inv_f);
  }
}

}  // namespace

extern "C" {

int mr_ubm_asym_device(mr_ctx* ctx, double alpha, int32_t q, int32_t frac_bits, void* dense_dev) {
  if (!ctx) return fail(MR_E_INVALID, "null context");
  int rc = mr_hip::check_asym_args(alpha, q);
  if (rc) return rc;
  if (frac_bits != 0 && (frac_bits < 8 || frac_bits > 52))
    return fail(MR_E_INVALID, "frac_bits=%d must be 0 (the context's) or in [8,52]", frac_bits);
  if (!dense_dev) return fail(MR_E_INVALID, "null dense_dev");
  mr_internal::ShardTables t;
  if ((rc = mr_internal::shard_tables(ctx, "asymmetric user-based model", &t))) return rc;
  const int F = frac_bits ? frac_bits : t.frac_bits;
  int bits = 0;  // ceil(log2(max c_tr + 1)): the sum of max c_tr keys of at most about 2^F each stays in int64
  while ((1ll << bits) < (long long)t.max_ctr + 1) ++bits;
  if (F + bits > 62)
    return fail(MR_E_INVALID, "frac_bits=%d + %d bits for the largest train-listener count %d exceeds 62", F, bits,
                t.max_ctr);
  const int n_te = t.n_te, n_tr = t.n_tr;
  const int width = t.song_hi - t.song_lo;
  if (n_te <= 0 || width <= 0) return MR_OK;

  // pa = te_len^alpha, pb = tr_len^(1-alpha): the halves of two mr_asym_tables calls that are read
  std::vector<double> pa((size_t)n_te), pb((size_t)std::max(1, n_tr));
  {
    std::vector<double> unused((size_t)std::max(n_te, std::max(1, n_tr)));
    if ((rc = mr_asym_tables(alpha, n_te, t.te_len, pa.data(), unused.data()))) return rc;
    if (n_tr > 0 && (rc = mr_asym_tables(alpha, n_tr, t.tr_len, unused.data(), pb.data()))) return rc;
  }

  // the three diagnostic settings (results identical): smaller chunks, batches and sub-ranges
  const int chunk = env_clamped("MR_UASYM_CHUNK", 16, kUasymChunk);
  const int n_chunks = (n_tr + chunk - 1) / chunk;
  const size_t per_user = (size_t)std::max(1, n_tr) * 12 + (size_t)std::max(1, n_chunks) * 4;
  const int fit = (int)std::min<size_t>((size_t)n_te, std::max<size_t>(1, (size_t)MR_UASYM_SCRATCH_BYTES / per_user));
  const int batch = env_clamped("MR_UASYM_BATCH", 1, fit);
  const int sub = std::min(t.block_songs, env_clamped("MR_UASYM_SUB", 64, kUasymMaxSub));
  const int n_sub = (t.block_songs + sub - 1) / sub;
  const int rows = mr_internal::launch_rows(kUasymMaxBatch);  // (MR_LAUNCH_ROWS, diagnostic: fewer users per launch)

  MR_HIP(hipSetDevice(t.device));
  hipStream_t st = (hipStream_t)t.stream;
  Drain drain;
  drain.st = st;
  Tmp<double> d_a, d_b;
  Tmp<int> d_v, d_cnt;
  Tmp<long long> d_key;
  const size_t slots = (size_t)batch * (size_t)std::max(1, n_tr);
  if ((rc = d_a.alloc(pa.size(), st)) || (rc = d_b.alloc(pb.size(), st)) || (rc = d_v.alloc(slots, st)) ||
      (rc = d_key.alloc(slots, st)) || (rc = d_cnt.alloc((size_t)batch * std::max(1, n_chunks), st)))
    return rc;
  MR_HIP(hipMemcpyAsync(d_a.p, pa.data(), pa.size() * 8, hipMemcpyHostToDevice, st));
  MR_HIP(hipMemcpyAsync(d_b.p, pb.data(), pb.size() * 8, hipMemcpyHostToDevice, st));

  for (int u0 = 0; u0 < n_te; u0 += batch) {  // batches: the neighbour scratch of `batch` users
    const int nb = std::min(batch, n_te - u0);
    for (int r0 = 0; r0 < nb && n_chunks > 0; r0 += rows) {
      const int nr = std::min(rows, nb - r0);
      UwParams wp{n_tr,      chunk,       n_chunks, q,     u0,    r0,      std::ldexp(1.0, F), t.te_off, t.te_songs,
                  t.trs_off, t.trs_users, d_a.p,    d_b.p, d_v.p, d_key.p, d_cnt.p};
      hipLaunchKernelGGL(k_uasym_weights, dim3(n_chunks, nr), dim3(kUwThreads), 0, st, wp);
      MR_HIP(hipGetLastError());
    }
    for (int r0 = 0; r0 < nb; r0 += rows) {
      const int nr = std::min(rows, nb - r0);
      UsParams sp{n_tr,   t.song_lo, t.song_hi, t.block_songs, sub,      n_sub,      chunk, n_chunks, t.f64, u0,      r0,
                  std::ldexp(1.0, -F), t.toff,    t.tsongs,      t.te_off, t.te_songs, d_v.p, d_key.p,  d_cnt.p, dense_dev};
      hipLaunchKernelGGL(k_uasym_score, dim3(t.n_tiles * n_sub, nr), dim3(kUsThreads), 0, st, sp);
      MR_HIP(hipGetLastError());
    }
  }
  MR_HIP(hipStreamSynchronize(st));
  return MR_OK;
}

}  // extern "C"
