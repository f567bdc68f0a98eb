// mr_internal.h — entry points shared between the engine's translation units
// (not part of the C ABI in include/mr_engine.h).
#ifndef MR_INTERNAL_H
#define MR_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#include "mr_engine.h"

namespace mr_internal {

// k_topk_merge of n_shards [shard][n_te][k] device lists into [n_te][k] outputs,
// enqueued on the context's stream (no host wait).
int merge_async(mr_ctx* c, int32_t n_shards, int32_t n_te, int32_t k, const int32_t* songs_in,
                const int64_t* keys_in, int32_t* songs_out, int64_t* keys_out, double* scores_out);

// The same over G gathered record blocks (keys [n_te*k] int64 at byte 0,
// songs [n_te*k] int32 at byte 8*n_te*k, block stride rec_bytes).
int merge_records_async(mr_ctx* c, int32_t n_shards, int32_t n_te, int32_t k, const void* records, int64_t rec_bytes,
                        int32_t* songs_out, int64_t* keys_out, double* scores_out);

// The context's own top-k record block (the exchange's send buffer; valid
// until mr_load / mr_destroy) and its size in bytes.
int topk_records(mr_ctx* c, void** records, int64_t* rec_bytes);

// mr_load's input checks (CSR shapes, sorted rows, id ranges, counts) without
// loading: what mr_group_load runs before it reads the dataset itself.
int validate_dataset(const mr_dataset* d);

// Synchronous device -> host copy of rows (pitched), staged through the
// context's pinned buffers when the destination is large pageable memory.
int d2h_staged(mr_ctx* c, void* dst, size_t dpitch, const void* src, size_t spitch, size_t row_bytes, size_t rows);

// Number of contexts of one process that share this context's device (set
// by mr_group_load before mr_load, default 1): the lazily allocated neighbour
// lists' budget (free device memory / 8 at load) is divided by it, since the
// group's contexts measure free memory at once, before any of them allocates.
int set_device_share(mr_ctx* c, int n);

// The loaded tables of the context's shard that the models outside
// mr_engine.hip read (csrc/mr_similar.hip, mr_asym.hip, mr_uasym.hip): geometry,
// device pointers and the HOST copies mr_load keeps of mr_dataset.song_count,
// te_len and tr_len (4 * (n_s + n_te + n_tr) bytes). Everything is valid until
// mr_load / mr_destroy.
struct ShardTables {
  int n_tr, n_te, n_s, song_lo, song_hi, block_songs, n_tiles, device;
  int f64;                       // != 0: the dense model is double, else float (mr_options.out_dtype)
  int frac_bits;                 // mr_options.frac_bits of the context
  int32_t max_ctr;               // max over every song s of c_tr(s) = |L_tr(s)|
  void* stream;                  // the context's hipStream_t
  // device
  const long long* trs_off;      // song -> train listeners CSR [n_s + 1] (every song, not only the shard's)
  const int* trs_users;          //   listeners as the context's (renumbered) train users, ascending
  const int* toff;               // tile-major train CSR over the shard [n_tiles * n_tr + 1]
  const unsigned short* tsongs;  //   tile-local song ids, rows duplicate-free
  const double* sqrt_c;          // sqrt(c(s)) [n_s] (train + test lines, duplicates counted)
  const long long* te_off;       // test user -> distinct visible songs T(u) [n_te + 1]
  const int* te_songs;           //   ascending song ids
  // host
  const int32_t* song_count;     // c(s) [n_s]
  const int32_t* te_len;         // |T(u)| with duplicates [n_te]
  const int32_t* tr_len;         // |S(v)| with duplicates [n_tr], v the context's internal train id (the ids
                                 //   trs_users and toff are indexed by), not the dataset's train order
};
// MR_E_STATE "<what> before mr_load" when the context has no dataset.
int shard_tables(mr_ctx* c, const char* what, ShardTables* out);

// k_rank_dense over n_rows rows of `width` values (f64 != 0: double, else
// float; NaN = no entry) into songs / scores [n_rows][K] (scores may be NULL),
// song id = song_lo + column: enqueued on `stream` (a hipStream_t), no host
// wait; arguments are the caller's to check (csrc/mr_rank.hip).
int rank_rows_async(void* stream, int f64, int32_t n_rows, int32_t width, int32_t song_lo, const void* dense,
                    int32_t K, int32_t* songs, double* scores);

// The grid-row limit (grid y <= 65535), and the limit where the XCD remap
// pads the grid to a multiple of 8 rows.
constexpr int kGridRows = 65535;
constexpr int kGridRowsXcd = 65528;

// Rows (grid y: test users or queries) of one launch of every host loop that
// splits a call at the grid-row limit: production_max (kGridRows, or
// kGridRowsXcd under the XCD remap), unless
// MR_LAUNCH_ROWS=n (diagnostic, n >= 8, read at each call) lowers it to n
// rounded down to a multiple of 8, so that a few dozen rows take the second
// and later iterations. Never below 8; any other value is ignored.
int launch_rows(int production_max);

// Set the calling thread's mr_last_error() message; returns code.
int set_error(int code, const char* msg);

}  // namespace mr_internal

#endif  // MR_INTERNAL_H
