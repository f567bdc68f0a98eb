"""Full ranked lists at C5 size, on one GPU in f32: ranks K = 500 per test user
(DeviceEnsemble.rank, k_rank_dense) on the synthetic C5 user-based model — 2,000
test users x the synthetic C5 song count — and on a model of the same shape
with random values and no ties. Each is timed with device events on the
engine's stream over --reps repetitions after --warmup untimed ones (minimum,
median and maximum printed), next to

  (a) the one-pass read floor of the model: its bytes / 8 TB/s, and
  (b) torch.topk(t.nan_to_num(nan=-inf), K, sorted=True) on the same tensor in
      the same session (events on torch's stream) — an outside yardstick only:
      it does not fix the order of tied songs, so it cannot replace the kernel.

The kernel's lists are checked against evaluation.rank_lists on a few users.

    python scripts/rank_probe.py [--K 500] [--reps 20] [--warmup 3] [--config c5]
"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from musicrecommendation_amd import evaluation, synth
from musicrecommendation_amd.engine import Engine
from musicrecommendation_amd.ensemble import DeviceEnsemble

ap = argparse.ArgumentParser()
ap.add_argument("--config", default="c5")
ap.add_argument("--n-test", type=int, default=None)
ap.add_argument("--K", type=int, default=500)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
a = ap.parse_args()
HBM_BYTES_PER_S = 8e12

if not torch.cuda.is_available():
    sys.exit("rank_probe: no GPU (a timing needs the device; there is no fallback)")

t0 = time.perf_counter()
ds = synth.config(a.config, n_test=a.n_test).dataset()
eng = Engine(ds, device=0, out_dtype="f32", topk=10)
ens = DeviceEnsemble(eng)
ubm = ens.model("ubm")
gen = torch.Generator(device=ens.device).manual_seed(1)
rnd = torch.rand(ubm.shape, dtype=torch.float32, device=ens.device, generator=gen)
rnd[torch.isnan(ubm)] = float("nan")  # the same heard-song mask
torch.cuda.synchronize()
M = ubm.numel() * ubm.element_size()
print(f"{a.config}: {ds.n_test} x {ds.n_songs} f32, model {M / 1e9:.3f} GB, K = {a.K} "
      f"(setup {time.perf_counter() - t0:.1f} s)", flush=True)
print(f"(a) one-pass read floor at 8 TB/s: {1e3 * M / HBM_BYTES_PER_S:.3f} ms", flush=True)


def timed(stream, f):
    """Device ms of f() per repetition: events on `stream` either side."""
    ms = []
    for i in range(a.warmup + a.reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            s.record()
            f()
            e.record()
        e.synchronize()
        if i >= a.warmup:
            ms.append(s.elapsed_time(e))
    return ms


def row_passes(row, K, cap=4096):
    """Passes over the row that k_rank_dense makes for it (f32): the radix
    select's histogram passes (restated in numpy: 11 + 11 + 10 bit digits, stop
    when the keys at or above the K-th entry's bucket fit the candidate buffer)
    plus the ordered collect."""
    if row.size <= cap:
        return 1
    v = row[~np.isnan(row)] + np.float32(0)
    b = v.view(np.uint32)
    key = np.where(b >> 31 != 0, ~b, b | np.uint32(1 << 31)).astype(np.int64)
    need, above, passes = K, 0, 0
    for shift, w in ((21, 11), (10, 11), (0, 10)):
        passes += 1
        if key.size < need:
            break
        digit = (key >> shift) & ((1 << w) - 1)
        hist = np.bincount(digit, minlength=1 << w)
        suffix = np.cumsum(hist[::-1])[::-1]
        d = int(np.nonzero(suffix >= need)[0].max())
        if above + suffix[d] <= cap:
            break
        above += suffix[d] - hist[d]
        need -= suffix[d] - hist[d]
        key = key[digit == d]
    return passes + 1


def line(what, ms):
    print(f"  {what:34s} min {min(ms):8.3f}  median {statistics.median(ms):8.3f}  max {max(ms):8.3f} ms "
          f"({len(ms)} reps; min = {min(ms) / (1e3 * M / HBM_BYTES_PER_S):.1f} x the read floor)", flush=True)


ext = torch.cuda.ExternalStream(eng.stream, device=ens.device)
cur = torch.cuda.current_stream(ens.device)
for name, t in (("user-based model", ubm), ("random values, no ties", rnd)):
    songs = torch.empty((eng.n_test, a.K), dtype=torch.int32, device=ens.device)
    scores = torch.empty((eng.n_test, a.K), dtype=torch.float64, device=ens.device)
    torch.cuda.synchronize()
    print(name, flush=True)
    line("k_rank_dense", timed(ext, lambda: eng.rank_dense(t.data_ptr(), a.K, songs.data_ptr(), scores.data_ptr())))
    line("(b) torch.topk(nan_to_num, sorted)",
         timed(cur, lambda: torch.topk(t.nan_to_num(nan=float("-inf")), a.K, sorted=True)))
    line("    torch.topk alone", timed(cur, lambda: torch.topk(t, a.K, sorted=True)))
    rows = [0, eng.n_test // 2, eng.n_test - 1]
    exp = evaluation.rank_lists(t[rows].cpu().numpy(), a.K)
    got = songs[rows].cpu().numpy(), scores[rows].cpu().numpy()
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1], equal_nan=True), name
    print(f"  row passes of users {rows}: {[row_passes(t[r].cpu().numpy(), a.K) for r in rows]}", flush=True)
    vals = t[rows[1]][~torch.isnan(t[rows[1]])]
    print(f"  lists equal evaluation.rank_lists on users {rows}; user {rows[1]}: {vals.numel()} pairs, "
          f"{torch.unique(vals).numel()} distinct values", flush=True)
eng.close()
