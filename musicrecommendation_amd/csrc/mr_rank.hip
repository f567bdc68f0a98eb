// mr_rank.hip — full ranked recommendation lists (K <= MR_RANK_MAX_K) of a
// dense model of one context's shard (n_te x width of the context's out_dtype,
// NaN = no pair), and the challenge's truncated mAP@k over such lists.
//
// k_rank_dense: one 1024-thread workgroup per test user.
//   1. every value maps to an order-preserving unsigned key (sign-flip on the
//      bit pattern, -0.0 canonicalised on the bits, NaN -> key 0 = "no entry");
//   2. an MSB radix select over 11-bit digits (LDS histogram, block suffix
//      scan) narrows the K-th key: after each digit it knows the lower bound L
//      of the K-th entry's bucket and the count of keys >= L;
//   3. as soon as that count fits the LDS candidate buffer (kCap), or at once
//      when the row itself fits, an ordered pass over the row (ballot + wave and
//      block prefix, no atomics) copies every key >= L into the buffer; when
//      the select runs to the last digit instead (a tie group larger than the
//      buffer) the pass takes every key > T and the first K - G keys == T in
//      column order, and stops when that quota is full;
//   4. a bitonic network sorts the candidates by (key desc, column asc); the
//      first K leave, empty slots as song -1 / score NaN.
// The histogram's LDS atomics only count (their sum does not depend on arrival
// order); which entries are kept is decided by keys and column positions
// alone, so the lists are a pure function of the row.
// mr_internal::rank_rows_async enqueues the kernel over any n_rows rows of either
// element type: mr_rank_dense_device ranks a model's rows through it, the
// similar-song query (csrc/mr_similar.hip) its cosine rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "mr_engine.h"
#include "mr_hip_util.h"
#include "mr_internal.h"

namespace {

using mr_hip::Tmp;
using mr_host::fail;

constexpr int kRankThreads = 1024;
constexpr int kRankWaves = kRankThreads / 64;
constexpr int kDigitBits = 11;
constexpr int kBins = 1 << kDigitBits;
// Candidate buffer: 4096 (key, column) pairs. f64: 32 KiB keys + 16 KiB columns
// + 8 KiB histogram = 56 KiB of static LDS (f32: 40 KiB), two workgroups per CU.
constexpr int kCap = 4096;
static_assert(kBins == 2 * kRankThreads, "the suffix scan gives every thread two bins");
static_assert(MR_RANK_MAX_K <= kCap && MR_RANK_MAX_K <= kRankThreads, "K fits the buffer and one store per thread");

template <typename T> struct Bits;
template <> struct Bits<float> {
  using U = uint32_t;
  static constexpr int n = 32;
  static constexpr U exp_mask = 0x7F800000u;
};
template <> struct Bits<double> {
  using U = uint64_t;
  static constexpr int n = 64;
  static constexpr U exp_mask = 0x7FF0000000000000ull;
};

// Order-preserving key of a stored bit pattern: larger key = higher rank;
// 0 = NaN (no valid value maps to 0: -inf is ~0xFF80.. > 0). Bit operations
// only, so denormals stay distinct whatever the float mode.
template <typename T>
__host__ __device__ inline typename Bits<T>::U key_of_bits(typename Bits<T>::U b) {
  using U = typename Bits<T>::U;
  constexpr U sign = U(1) << (Bits<T>::n - 1);
  if ((b & ~sign) > Bits<T>::exp_mask) return 0;  // NaN
  if (b == sign) b = 0;                            // -0.0 ranks as +0.0
  return (b & sign) ? U(~b) : U(b | sign);
}
template <typename T>
__host__ __device__ inline double score_of_key(typename Bits<T>::U k) {
  using U = typename Bits<T>::U;
  constexpr U sign = U(1) << (Bits<T>::n - 1);
  const U b = (k & sign) ? U(k ^ sign) : U(~k);
  T v;
  memcpy(&v, &b, sizeof v);
  return (double)v;  // f32 widens exactly
}

struct RankParams {
  int width, song_lo, K;
  const void* dense;
  int* songs;
  double* scores;
};

__device__ inline int lanes_below(unsigned long long m) {  // set bits of m below this lane
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

template <typename T>
__global__ __launch_bounds__(kRankThreads) void k_rank_dense(RankParams p) {
  using U = typename Bits<T>::U;
  constexpr int kBits = Bits<T>::n;
  __shared__ U ckey[kCap];
  __shared__ int csong[kCap];
  __shared__ int hist[kBins];
  __shared__ int wtot[2][kRankWaves];
  __shared__ int sel[4];  // digit, keys >= digit in the bucket, keys == digit, all keys counted

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int width = p.width, K = p.K;
  const U* row = reinterpret_cast<const U*>(p.dense) + (size_t)blockIdx.x * (size_t)width;

  // ---- select: lower bound of the candidates -------------------------------
  U bound = 0;         // candidates: key >= bound (exact: key > bound, and the first `need` key == bound)
  bool exact = false;  // the select ran to the last digit: bound is the K-th key itself
  int need = K;        // rank of the K-th entry inside the current bucket
  int G = 0;           // keys above the current bucket
  int n_c = width;     // number of candidates (an upper bound when the row is taken whole)
  if (width > kCap) {
    U prefix = 0;
    int shift = kBits;  // bits below the digits fixed so far
    exact = true;
    while (shift > 0) {
      const int w = shift < kDigitBits ? shift : kDigitBits;
      const int dshift = shift - w;
      __syncthreads();  // the previous pass's sel / hist have been read
      hist[2 * tid] = 0;
      hist[2 * tid + 1] = 0;
      if (tid == 0) sel[0] = -1;
      __syncthreads();
      for (int c0 = tid; c0 < width; c0 += 4 * kRankThreads) {
        U b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {  // four loads in flight
          const int c = c0 + i * kRankThreads;
          b[i] = c < width ? row[c] : U(Bits<T>::exp_mask | 1);  // a NaN past the end
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const U key = key_of_bits<T>(b[i]);
          const bool in = key != 0 && (shift == kBits || (key >> (shift & (kBits - 1))) == (prefix >> (shift & (kBits - 1))));
          if (in) {
            const int digit = (int)((key >> dshift) & U((1 << w) - 1));
            // one add per wave when its lanes agree (tie-heavy rows would
            // otherwise serialise 64 adds on one LDS word)
            const int d0 = __builtin_amdgcn_readfirstlane(digit);
            const unsigned long long act = __ballot(1), same = __ballot(digit == d0);
            if (same == act) {
              if (lane == __ffsll((long long)act) - 1) atomicAdd(&hist[d0], __popcll(act));
            } else {
              atomicAdd(&hist[digit], 1);
            }
          }
        }
      }
      __syncthreads();
      // S[b] = keys of the bucket with digit >= b: block suffix scan, two bins a thread
      const int h0 = hist[2 * tid], h1 = hist[2 * tid + 1], s = h0 + h1;
      int incl = s;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_down(incl, off);
        if (lane + off < 64) incl += o;
      }
      if (lane == 0) wtot[0][wave] = incl;
      __syncthreads();
      for (int w2 = wave + 1; w2 < kRankWaves; ++w2) incl += wtot[0][w2];
      if (tid == 0) sel[3] = incl;
      // the digit d with S[d] >= need > S[d + 1]: in exactly one thread's bins
      if (incl >= need && incl - s < need) {
        const bool upper = incl - h0 >= need;
        sel[0] = 2 * tid + (upper ? 1 : 0);
        sel[1] = upper ? incl - h0 : incl;
        sel[2] = upper ? h1 : h0;
      }
      __syncthreads();
      const int d = sel[0], sd = sel[1], hd = sel[2];
      if (d < 0) {  // fewer than K valid entries (first pass only): take them all
        bound = 0;
        n_c = sel[3];
        exact = false;
        break;
      }
      prefix |= U(d) << dshift;
      shift = dshift;
      bound = prefix;
      if (G + sd <= kCap) {  // every key >= bound fits the buffer: sort decides the rest
        n_c = G + sd;
        exact = false;
        break;
      }
      G += sd - hd;
      need -= sd - hd;
    }
    if (exact) n_c = K;
  }

  // ---- ordered collect ------------------------------------------------------
  int P = 64;
  while (P < n_c && P < kCap) P <<= 1;  // n_c <= kCap
  __syncthreads();
  for (int i = tid; i < P; i += kRankThreads) {
    ckey[i] = 0;
    csong[i] = INT_MAX;
  }
  __syncthreads();
  {
    int base_gt = 0, base_eq = 0;
    U nxt = tid < width ? row[tid] : U(Bits<T>::exp_mask | 1);
    for (int c0 = 0; c0 < width; c0 += kRankThreads) {
      const int col = c0 + tid;
      const U key = key_of_bits<T>(nxt);
      const int cn = col + kRankThreads;
      nxt = cn < width ? row[cn] : U(Bits<T>::exp_mask | 1);  // in flight across the barrier
      const bool gt = key != 0 && (exact ? key > bound : key >= bound);
      const bool eq = exact && key == bound;
      const unsigned long long mgt = __ballot(gt), meq = __ballot(eq);
      const int buf = (c0 / kRankThreads) & 1;
      if (lane == 0) wtot[buf][wave] = __popcll(mgt) | (__popcll(meq) << 16);  // <= 1024 each over the block
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int w2 = 0; w2 < kRankWaves; ++w2) {
        const int v = wtot[buf][w2];
        total += v;
        if (w2 < wave) before += v;
      }
      if (gt) {
        const int pos = base_gt + (before & 0xffff) + lanes_below(mgt);
        if (pos < P) {
          ckey[pos] = key;
          csong[pos] = col;
        }
      } else if (eq) {
        const int r = base_eq + (before >> 16) + lanes_below(meq);  // rank among the ties, in column order
        if (r < need && G + r < P) {
          ckey[G + r] = key;
          csong[G + r] = col;
        }
      }
      base_gt += total & 0xffff;
      base_eq += total >> 16;
      if (exact && base_gt >= G && base_eq >= need) break;  // quota full (uniform)
    }
  }
  __syncthreads();

  // ---- bitonic sort by (key desc, column asc) --------------------------------
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += kRankThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const U ka = ckey[i], kb = ckey[l];
        const int sa = csong[i], sb = csong[l];
        const bool a_first = ka > kb || (ka == kb && sa < sb);
        const bool b_first = kb > ka || (ka == kb && sb < sa);
        if ((i & k2) == 0 ? b_first : a_first) {
          ckey[i] = kb;
          ckey[l] = ka;
          csong[i] = sb;
          csong[l] = sa;
        }
      }
      __syncthreads();
    }
  }

  if (tid < K) {
    const U key = tid < P ? ckey[tid] : U(0);
    const size_t o = (size_t)blockIdx.x * (size_t)K + tid;
    p.songs[o] = key ? csong[tid] + p.song_lo : -1;
    if (p.scores) p.scores[o] = key ? score_of_key<T>(key) : (double)NAN;
  }
}

// ---- truncated mAP@k over ranked lists -----------------------------------------
// One wave per test user: the lanes look 64 slots up in the user's sorted,
// distinct labels (binary search), lane 0 folds the hits in rank order.
constexpr int kMapThreads = 256;

__global__ __launch_bounds__(kMapThreads) void k_rank_map(int n_te, int K, int k_eval, const int* songs,
                                                          const long long* lab_off, const int* lab_songs,
                                                          double* ap) {
  const int lane = threadIdx.x & 63;
  const int u = blockIdx.x * (kMapThreads / 64) + (threadIdx.x >> 6);
  if (u >= n_te) return;  // whole waves
  const long long lo = lab_off[u];
  const long long n_u = lab_off[u + 1] - lo;
  const int* lab = lab_songs + lo;
  double a = 0.0;
  int h = 0;
  for (int c0 = 0; c0 < k_eval; c0 += 64) {
    const int i = c0 + lane;
    bool hit = false;
    if (i < k_eval) {
      const int s = songs[(size_t)u * K + i];
      if (s >= 0) {
        long long l = 0, r = n_u;
        while (l < r) {
          const long long m = (l + r) >> 1;
          if (lab[m] < s) l = m + 1;
          else r = m;
        }
        hit = l < n_u && lab[l] == s;
      }
    }
    unsigned long long m = __ballot(hit);
    if (lane == 0)
      while (m) {
        const int b = __ffsll((long long)m) - 1;
        m &= m - 1;
        ++h;
        a = a + (double)h / (double)(c0 + b + 1);  // a miss adds 0.0: a unchanged
      }
  }
  if (lane == 0) ap[u] = n_u > 0 ? a / (double)(n_u < k_eval ? n_u : (long long)k_eval) : 0.0;
}

// Sorted, distinct labels per user as a CSR (labels are a set).
int distinct_labels(int n_te, const int64_t* lab_off, const int32_t* lab_songs, std::vector<long long>& off,
                    std::vector<int32_t>& songs) {
  if (lab_off[0] < 0) return fail(MR_E_INVALID, "bad label CSR");
  off.assign((size_t)n_te + 1, 0);
  songs.clear();
  for (int u = 0; u < n_te; ++u) {
    if (lab_off[u + 1] < lab_off[u]) return fail(MR_E_INVALID, "bad label CSR");
    if (lab_off[u + 1] > lab_off[u] && !lab_songs) return fail(MR_E_INVALID, "null label songs");
    const size_t b = songs.size();
    songs.insert(songs.end(), lab_songs + lab_off[u], lab_songs + lab_off[u + 1]);
    std::sort(songs.begin() + b, songs.end());
    songs.erase(std::unique(songs.begin() + b, songs.end()), songs.end());
    off[u + 1] = (long long)songs.size();
  }
  return MR_OK;
}

int check_map_args(int32_t n_te, const int32_t* songs, int32_t K, int32_t k_eval, const int64_t* lab_off,
                   double* map_out) {
  if (n_te < 0 || (n_te > 0 && !songs) || !lab_off || !map_out) return fail(MR_E_INVALID, "null argument");
  if (K < 1 || K > MR_RANK_MAX_K) return fail(MR_E_INVALID, "K=%d must be in [1,%d]", K, MR_RANK_MAX_K);
  if (k_eval < 1 || k_eval > K) return fail(MR_E_INVALID, "k_eval=%d must be in [1,K=%d]", k_eval, K);
  return MR_OK;
}

double mean_ap(int n_te, const double* ap) {
  double total = 0.0;  // left fold in user order
  for (int u = 0; u < n_te; ++u) total = total + ap[u];
  return n_te > 0 ? total / (double)n_te : 0.0;
}

}  // namespace

namespace mr_internal {

int rank_rows_async(void* stream, int f64, int32_t n_rows, int32_t width, int32_t song_lo, const void* dense,
                    int32_t K, int32_t* songs, double* scores) {
  if (n_rows <= 0) return MR_OK;
  hipStream_t st = (hipStream_t)stream;
  RankParams rp{width, song_lo, K, dense, songs, scores};
  if (f64)
    hipLaunchKernelGGL(k_rank_dense<double>, dim3(n_rows), dim3(kRankThreads), 0, st, rp);
  else
    hipLaunchKernelGGL(k_rank_dense<float>, dim3(n_rows), dim3(kRankThreads), 0, st, rp);
  MR_HIP(hipGetLastError());
  return MR_OK;
}

}  // namespace mr_internal

extern "C" {

int mr_rank_dense_device(mr_ctx* ctx, const void* dense_dev, int32_t K, int32_t* songs_dev, double* scores_dev) {
  if (!ctx || !dense_dev || !songs_dev) return fail(MR_E_INVALID, "null argument");
  if (K < 1 || K > MR_RANK_MAX_K) return fail(MR_E_INVALID, "K=%d must be in [1,%d]", K, MR_RANK_MAX_K);
  mr_view v;
  int rc = mr_view_get(ctx, &v);
  if (rc) return rc;
  MR_HIP(hipSetDevice(v.device));
  hipStream_t st = (hipStream_t)v.stream;
  if ((rc = mr_internal::rank_rows_async(st, v.out_dtype == MR_OUT_F64, v.n_test_users, v.song_hi - v.song_lo, v.song_lo,
                                         dense_dev, K, songs_dev, scores_dev)))
    return rc;
  MR_HIP(hipStreamSynchronize(st));
  return MR_OK;
}

int mr_rank_merge_host(int32_t n_lists, int32_t n_te, int32_t K, const int32_t* songs_in, const double* scores_in,
                       int32_t* songs_out, double* scores_out) {
  if (!songs_in || !scores_in || !songs_out || !scores_out) return fail(MR_E_INVALID, "null argument");
  if (n_lists < 1 || n_te < 0) return fail(MR_E_INVALID, "bad merge shape");
  if (K < 1 || K > MR_RANK_MAX_K) return fail(MR_E_INVALID, "K=%d must be in [1,%d]", K, MR_RANK_MAX_K);
  struct Item {
    uint64_t key;
    int32_t song;
  };
  std::vector<Item> items;
  for (int u = 0; u < n_te; ++u) {
    items.clear();
    for (int g = 0; g < n_lists; ++g) {
      const size_t base = ((size_t)g * n_te + u) * K;
      for (int i = 0; i < K; ++i) {
        if (songs_in[base + i] < 0) continue;
        uint64_t b;
        memcpy(&b, &scores_in[base + i], sizeof b);
        const uint64_t key = key_of_bits<double>(b);
        if (key) items.push_back({key, songs_in[base + i]});
      }
    }
    std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
      return a.key > b.key || (a.key == b.key && a.song < b.song);
    });
    for (int i = 0; i < K; ++i) {
      const bool have = (size_t)i < items.size();
      songs_out[(size_t)u * K + i] = have ? items[i].song : -1;
      scores_out[(size_t)u * K + i] = have ? score_of_key<double>(items[i].key) : (double)NAN;
    }
  }
  return MR_OK;
}

int mr_rank_map_host(int32_t n_te, const int32_t* songs, int32_t K, int32_t k_eval, const int64_t* lab_off,
                     const int32_t* lab_songs, double* ap_out, double* map_out) {
  int rc = check_map_args(n_te, songs, K, k_eval, lab_off, map_out);
  if (rc) return rc;
  std::vector<long long> off;
  std::vector<int32_t> lab;
  if ((rc = distinct_labels(n_te, lab_off, lab_songs, off, lab))) return rc;
  std::vector<double> ap((size_t)std::max(1, n_te));
  for (int u = 0; u < n_te; ++u) {
    const int32_t* lb = lab.data() + off[u];
    const long long n_u = off[u + 1] - off[u];
    double a = 0.0;
    int h = 0;
    for (int i = 0; i < k_eval; ++i) {
      const int s = songs[(size_t)u * K + i];
      if (s >= 0 && std::binary_search(lb, lb + n_u, s)) {
        ++h;
        a = a + (double)h / (double)(i + 1);
      }
    }
    ap[u] = n_u > 0 ? a / (double)std::min<long long>(k_eval, n_u) : 0.0;
    if (ap_out) ap_out[u] = ap[u];
  }
  *map_out = mean_ap(n_te, ap.data());
  return MR_OK;
}

int mr_rank_map_device(mr_ctx* ctx, const int32_t* songs_dev, int32_t K, int32_t k_eval, const int64_t* lab_off,
                       const int32_t* lab_songs, double* ap_out, double* map_out) {
  if (!ctx || !songs_dev) return fail(MR_E_INVALID, "null argument");
  int rc = check_map_args(0, nullptr, K, k_eval, lab_off, map_out);
  if (rc) return rc;
  mr_view v;
  if ((rc = mr_view_get(ctx, &v))) return rc;
  const int n_te = v.n_test_users;
  std::vector<long long> off;
  std::vector<int32_t> lab;
  if ((rc = distinct_labels(n_te, lab_off, lab_songs, off, lab))) return rc;
  if (lab.empty()) lab.push_back(0);  // the staging buffer is never empty
  MR_HIP(hipSetDevice(v.device));
  hipStream_t st = (hipStream_t)v.stream;
  std::vector<double> ap((size_t)std::max(1, n_te));
  Tmp<long long> d_off;
  Tmp<int> d_lab;
  Tmp<double> d_ap;
  if (n_te > 0) {
    if (int rc_ = d_off.alloc(off.size(), st)) return rc_;
    if (int rc_ = d_lab.alloc(lab.size(), st)) return rc_;
    if (int rc_ = d_ap.alloc((size_t)n_te, st)) return rc_;
    MR_HIP(hipMemcpyAsync(d_off.p, off.data(), off.size() * 8, hipMemcpyHostToDevice, st));
    MR_HIP(hipMemcpyAsync(d_lab.p, lab.data(), lab.size() * 4, hipMemcpyHostToDevice, st));
    const int per = kMapThreads / 64;
    hipLaunchKernelGGL(k_rank_map, dim3((n_te + per - 1) / per), dim3(kMapThreads), 0, st, n_te, K, k_eval, songs_dev,
                       d_off.p, d_lab.p, d_ap.p);
    MR_HIP(hipGetLastError());
    MR_HIP(hipMemcpyAsync(ap.data(), d_ap.p, (size_t)n_te * 8, hipMemcpyDeviceToHost, st));
  }
  MR_HIP(hipStreamSynchronize(st));
  if (ap_out)
    for (int u = 0; u < n_te; ++u) ap_out[u] = ap[u];
  *map_out = mean_ap(n_te, ap.data());
  return MR_OK;
}

}  // extern "C"
