// mr_similar.hip — similar-song queries: the item-item cosine rows of the
// reference's cosineSimilarity (MusicRecommender.scala:230-239) for given
// query songs against every song of one context's shard, and their top-K
// lists (mr_similar_songs_device, include/mr_engine.h).
//
// k_similar_count: one 1024-thread workgroup per (song tile, query).
//   1. u32 counters in LDS cover the tile (a tile wider than kSimMaxCounters
//      songs is processed in song sub-ranges, the listeners walked once per
//      sub-range);
//   2. the workgroup walks the query's train listeners L_tr(q) =
//      trs_users[trs_off[q] .. trs_off[q+1]): listener v's songs in this tile
//      are tsongs[toff[t*n_tr+v] .. toff[t*n_tr+v+1]), and every one of them
//      gets +1 by an LDS add without a returned value. The walk is the shared
//      walk_tile_lists (csrc/mr_tile_walk.h: listener id -> toff pair ->
//      segment ids, software-pipelined three levels deep) in its 2-byte
//      segment-load form. Rows of the tile CSR are duplicate-free, so a listener
//      adds at most 1 per song: the counter is C(q, s) = |L_tr(q) ∩ L_tr(s)|;
//   3. the epilogue writes (double)C / (sqrt_c[q] * sqrt_c[s]) (0.0 for a zero
//      denominator; fp64 * and / only, no contraction) coalesced to the dense
//      row and, for the lists, to a scratch row with NaN where C = 0.
// The counts are integer sums (order-free), so the rows are a pure function of
// the dataset and the query. The lists are k_rank_dense (csrc/mr_rank.hip)
// over the scratch rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mr_engine.h"
#include "mr_hip_util.h"
#include "mr_internal.h"
#include "mr_tile_walk.h"

namespace {

using mr_hip::Tmp;
using mr_host::fail;

constexpr int kSimThreads = 1024;
constexpr int kSimR = 2;                  // listeners per thread and iteration
constexpr int kSimSeg = 4;                // segment ids loaded together
constexpr int kSimMaxCounters = 32768;    // u32 counters per pass: 128 KiB of the CU's 160 KiB LDS
constexpr int kSimMaxBatch = mr_internal::kGridRows;  // queries per launch (grid y)
static_assert(MR_SIMILAR_SCRATCH_BYTES >= 8, "one value");

struct SimParams {
  int n_tr, song_lo, song_hi, block_songs, sub;  // sub: counters per pass (<= kSimMaxCounters)
  const long long* trs_off;
  const int* trs_users;
  const int* toff;
  const unsigned short* tsongs;
  const double* sqrt_c;
  const int* queries;  // this launch's query songs (global ids)
  double* dense;       // [queries][width], or null
  double* listed;      // [queries][width] with NaN where C = 0, or null
};

__global__ __launch_bounds__(kSimThreads) void k_similar_count(SimParams p) {
  extern __shared__ unsigned sim_cnt[];
  constexpr int NT = kSimThreads, R = kSimR;
  const int tid = threadIdx.x, tile = blockIdx.x, qi = blockIdx.y;
  const int q = p.queries[qi];
  const int width = p.song_hi - p.song_lo;
  const int blo = p.song_lo + tile * p.block_songs;
  const int bw = min(p.song_hi, blo + p.block_songs) - blo;
  const long long l0 = p.trs_off[q];
  const int n = (int)(p.trs_off[q + 1] - l0);
  const int* lst = p.trs_users + l0;
  const int* toff_t = p.toff + (size_t)tile * p.n_tr;
  const double sq = p.sqrt_c[q];
  const double nan = __longlong_as_double(0x7FF8000000000000ll);

  auto load_list = [&](int k0, int (&v)[R], unsigned (&w)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = k0 + r * NT;
      v[r] = k < n ? lst[k] : -1;
      w[r] = 1u;
    }
  };

  for (int s0 = 0; s0 < bw; s0 += p.sub) {
    const int sw = min(p.sub, bw - s0);
    for (int i = tid; i < sw; i += NT) sim_cnt[i] = 0u;
    __syncthreads();
    auto add = [&](unsigned x, unsigned) {
      const unsigned loc = x - (unsigned)s0;
      if (loc < (unsigned)sw)  // result unused: an LDS add without return
        (void)__hip_atomic_fetch_add(&sim_cnt[loc], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
    walk_tile_lists<NT, R, kSimSeg, unsigned, false>(tid, n, load_list, toff_t, p.tsongs, add);
    __syncthreads();
    // cos(q, s) = C / (sqrt(c(q)) * sqrt(c(s))), MR:236-238
    for (int i = tid; i < sw; i += NT) {
      const int s = blo + s0 + i;
      const unsigned c = sim_cnt[i];
      const double den = sq * p.sqrt_c[s];
      const double cosv = den != 0.0 ? (double)c / den : 0.0;
      const size_t o = (size_t)qi * (size_t)width + (size_t)(s - p.song_lo);
      if (p.dense) p.dense[o] = s == q ? nan : cosv;
      if (p.listed) p.listed[o] = (s == q || c == 0u) ? nan : cosv;
    }
    __syncthreads();  // the next pass rezeroes the counters
  }
}

}  // namespace

extern "C" {

int mr_similar_songs_device(mr_ctx* ctx, int32_t n_q, const int32_t* query_songs, int32_t K, int32_t* songs_dev,
                            double* scores_dev, double* dense_dev) {
  if (!ctx) return fail(MR_E_INVALID, "null context");
  if (K < 0 || K > MR_RANK_MAX_K) return fail(MR_E_INVALID, "K=%d must be in [0,%d]", K, MR_RANK_MAX_K);
  if (n_q < 0) return fail(MR_E_INVALID, "n_q=%d must not be negative", n_q);
  if (n_q > 0 && !query_songs) return fail(MR_E_INVALID, "null query_songs");
  if (K == 0 && !dense_dev) return fail(MR_E_INVALID, "K = 0 needs dense_dev");
  if (K >= 1 && !songs_dev) return fail(MR_E_INVALID, "K >= 1 needs songs_dev");
  mr_internal::ShardTables t;
  int rc = mr_internal::shard_tables(ctx, "similar-song query", &t);
  if (rc) return rc;
  for (int i = 0; i < n_q; ++i)
    if (query_songs[i] < 0 || query_songs[i] >= t.n_s)
      return fail(MR_E_INVALID, "query %d: song id %d outside [0,%d)", i, query_songs[i], t.n_s);
  const int width = t.song_hi - t.song_lo;
  if (n_q == 0 || width <= 0) return MR_OK;

  MR_HIP(hipSetDevice(t.device));
  hipStream_t st = (hipStream_t)t.stream;
  // queries per launch: the lists' scratch rows stay within MR_SIMILAR_SCRATCH_BYTES (one row at least;
  // MR_LAUNCH_ROWS, diagnostic: fewer queries per launch)
  const int per = (int)std::max<int64_t>(
      1, std::min<int64_t>(std::min(n_q, mr_internal::launch_rows(kSimMaxBatch)),
                           (int64_t)MR_SIMILAR_SCRATCH_BYTES / (8 * (int64_t)width)));
  Tmp<int> d_q;
  Tmp<double> d_listed;
  if ((rc = d_q.alloc((size_t)n_q, st))) return rc;
  MR_HIP(hipMemcpyAsync(d_q.p, query_songs, (size_t)n_q * 4, hipMemcpyHostToDevice, st));
  if (K >= 1 && (rc = d_listed.alloc((size_t)per * width, st))) return rc;

  // MR_SIMILAR_COUNTERS (diagnostic): fewer counters per pass, so that small tiles take the sub-range path
  const int sub = std::min(t.block_songs, mr_hip::env_clamped("MR_SIMILAR_COUNTERS", 64, kSimMaxCounters));
  const size_t lds = (size_t)sub * 4;
  MR_HIP(hipFuncSetAttribute((const void*)k_similar_count, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (int b0 = 0; b0 < n_q; b0 += per) {
    const int nb = std::min(per, n_q - b0);
    SimParams sp{t.n_tr,  t.song_lo, t.song_hi, t.block_songs, sub,
                 t.trs_off, t.trs_users, t.toff, t.tsongs, t.sqrt_c,
                 d_q.p + b0, dense_dev ? dense_dev + (size_t)b0 * width : nullptr, d_listed.p};
    hipLaunchKernelGGL(k_similar_count, dim3(t.n_tiles, nb), dim3(kSimThreads), lds, st, sp);
    MR_HIP(hipGetLastError());
    if (K >= 1 &&
        (rc = mr_internal::rank_rows_async(st, 1, nb, width, t.song_lo, d_listed.p, K, songs_dev + (size_t)b0 * K,
                                           scores_dev ? scores_dev + (size_t)b0 * K : nullptr)))
      return rc;
  }
  MR_HIP(hipStreamSynchronize(st));
  return MR_OK;
}

}  // extern "C"
