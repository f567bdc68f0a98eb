// mr_tile_walk.h — device code shared by the engine's .hip translation units:
// the walk over the tile-major train CSR (toff / tsongs), the song sub-range
// of a workgroup, the NaN-or-value store of a dense model and the asymmetric
// models' weight. Everything is a __device__ __forceinline__ function over the
// caller's lambdas: no function pointers, no LDS, no kernel arguments of its own.
#ifndef MR_TILE_WALK_H
#define MR_TILE_WALK_H

#include <hip/hip_runtime.h>

// One row of the tile-major train CSR in chunks of kSeg: every tile-local song
// x of tsongs[a, b) gets add(x), the kSeg loads of a chunk issued together.
// The tail loop of walk_tile_lists and the whole stage 2 of k_uasym_score.
template <int kSeg, typename Add>
__device__ __forceinline__ void walk_tile_row(int a, int b, const unsigned short* tsongs, Add&& add) {
  for (int x0 = a; x0 < b; x0 += kSeg) {
    int st[kSeg];
#pragma unroll
    for (int j = 0; j < kSeg; ++j) st[j] = x0 + j < b ? (int)tsongs[x0 + j] : -1;
#pragma unroll
    for (int j = 0; j < kSeg; ++j)
      if (st[j] >= 0) add((unsigned)st[j]);
  }
}

// Stage 2 of the wide shape as a walk over a list of train users: entry k <
// cnt of the list is (v, w) = load_list(k) (v = -1 past the end); every
// tile-local song x of v's segment in this tile (tsongs[toff_t[v] ..
// toff_t[v+1])) gets add(x, w), an LDS atomic of the caller's. R entries per
// thread per iteration. Used by the two-hop scoring (list = the test user's
// neighbours, w = their int64 weights), by the co-listening index build, the
// similar-song counts and the asymmetric item-based model (list = one song's
// train listeners, w = 1).
// kWordSeg: a segment's first kSeg entries are loaded as 8-B words, else as
// kSeg 2-B loads.
template <int NT, int R, int kSeg, typename WT, bool kWordSeg, typename LoadList, typename Add>
__device__ __forceinline__ void walk_tile_lists(int tid, int cnt, LoadList&& load_list, const int* toff_t,
                                                const unsigned short* tsongs, Add&& add) {
  // Software pipeline over iterations: iteration i gathers its segments
  // while the toff pairs of i+1 and the list entries of i+2 are in flight
  // (one memory latency covers the three dependent levels).
  auto load_offs = [&](const int (&v)[R], int (&a)[R], int (&b)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      a[r] = b[r] = 0;
      if (v[r] >= 0) { a[r] = toff_t[v[r]]; b[r] = toff_t[v[r] + 1]; }
    }
  };
  int v0[R], a0[R], b0[R], v1[R], a1[R], b1[R], v2[R];
  WT q0[R], q1[R], q2[R];
  load_list(tid, v0, q0);
  load_offs(v0, a0, b0);
  load_list(tid + R * NT, v1, q1);
  for (int k0 = tid; k0 < cnt; k0 += R * NT) {
    // a segment's first kSeg entries as 8-B words (4 tile-local ids each)
    // from the aligned word holding entry a0: kW loads instead of kSeg
    // 2-B loads (C4 21.9 vs 22.9 ms per 704-user batch, C3 1.093 vs 1.141 ms
    // per step; MR_WIDE_U16 builds the 2-B form, profiles/r02/c4/vec_seg_ab.txt)
    constexpr int kW = (kSeg + 3) / 4 + 1;
    uint2 sw[R][kW];  // (the word form's)
    int so[R];
    int sg[R][kSeg];  // (the 2-B form's)
    if constexpr (kWordSeg) {
      const uint2* tw = reinterpret_cast<const uint2*>(tsongs);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int wb = a0[r] >> 2;
        const int we = b0[r] > a0[r] ? (b0[r] + 3) >> 2 : wb;
        so[r] = a0[r] & 3;
#pragma unroll
        for (int j = 0; j < kW; ++j) sw[r][j] = wb + j < we ? tw[wb + j] : make_uint2(0u, 0u);
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < kSeg; ++j) sg[r][j] = a0[r] + j < b0[r] ? (int)tsongs[a0[r] + j] : -1;
    }
    load_offs(v1, a1, b1);                 // iteration i+1
    load_list(k0 + 2 * R * NT, v2, q2);    // iteration i+2
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if constexpr (kWordSeg) {
#pragma unroll
        for (int j = 0; j < kSeg; ++j) {
          if (a0[r] + j < b0[r]) {
            const int e = (j & 3) + so[r];  // 0..6: word j/4 or the next one
            const uint2 wv = e >= 4 ? sw[r][(j >> 2) + 1] : sw[r][j >> 2];
            const unsigned x = ((e & 3) < 2 ? wv.x : wv.y) >> ((e & 1) * 16);
            add(x & 0xffffu, q0[r]);
          }
        }
      } else {
#pragma unroll
        for (int j = 0; j < kSeg; ++j)
          if (sg[r][j] >= 0) add((unsigned)sg[r][j], q0[r]);
      }
      walk_tile_row<kSeg>(a0[r] + kSeg, b0[r], tsongs, [&](unsigned x) { add(x, q0[r]); });
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      a0[r] = a1[r]; b0[r] = b1[r]; q0[r] = q1[r];
      v1[r] = v2[r]; q1[r] = q2[r];
    }
  }
  (void)v0;
}

// The song sub-range of one workgroup of a (tile x sub-range, user) grid:
// block b of grid x is sub-range b % n_sub (sub songs wide) of tile b / n_sub.
// The range is the tile-local songs [s0, s0 + sw) of the tile's bw songs
// [blo, blo + bw); s0 >= bw (block-uniform) when the last tile is partial and
// has no such sub-range: the caller returns.
struct SubRange {
  int tile, s0, blo, bw, sw;
};
__device__ __forceinline__ SubRange sub_range(unsigned block, int n_sub, int sub, int song_lo, int song_hi,
                                              int block_songs) {
  SubRange r;
  r.tile = block / n_sub;  // (unsigned division, as blockIdx.x's: no sign handling)
  r.s0 = (block % n_sub) * sub;
  r.blo = song_lo + r.tile * block_songs;
  r.bw = min(song_hi, r.blo + block_songs) - r.blo;
  r.sw = min(sub, r.bw - r.s0);
  return r;
}

// One value of a dense model in the context's element type (f64 != 0: double,
// else float, rounded once): NaN where the user has heard the song.
__device__ __forceinline__ void store_model_value(void* out, int f64, size_t index, bool heard, double value) {
  if (f64)
    static_cast<double*>(out)[index] = heard ? __longlong_as_double(0x7FF8000000000000ll) : value;
  else
    static_cast<float*>(out)[index] = heard ? __int_as_float(0x7FC00000) : (float)value;
}

// The asymmetric models' weight w^q, w = count / den (0.0 for a zero
// denominator): one fp64 /, then q - 1 single *. The numpy twins
// (evaluation.asym_item_model, asym_user_model) pin this order bit for bit.
__device__ __forceinline__ double asym_weight(unsigned count, double den, int q) {
  const double w = den != 0.0 ? (double)count / den : 0.0;
  double t = w;
  for (int k = 1; k < q; ++k) t = t * w;
  return t;
}

#endif  // MR_TILE_WALK_H
