"""The asymmetric-cosine, locality-q user-based model at the C2 and C3 shapes on
one GPU: times mr_ubm_asym_device at (alpha, q) = (0.5, 1) and (0.15, 3) with
device events on the engine's stream over --reps repetitions after --warmup
untimed ones (minimum, median, maximum printed). Each time covers the whole
call: the host tables, their upload, the scratch allocation and both kernels.

Beside each time, the work the path does (computed from the dataset): the
listener ids stage 1 reads, the neighbours (v with a common song) it writes,
and the tile-local song ids stage 2 walks (every sub-range workgroup of a tile
walks the tile's rows).

The yardstick, same session and same context: one dense UserBasedModel step
(Engine.run("ubm")), a code path this model does not touch. The device rows of
--twin-users sampled test users are checked against the numpy twin
(evaluation.asym_user_model), bit for bit.

    python scripts/uasym_probe.py [--configs c2,c3] [--reps 5] [--warmup 1] [--out FILE]
"""
import argparse, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from musicrecommendation_amd import evaluation, synth
from musicrecommendation_amd.engine import Engine
from musicrecommendation_amd.ensemble import DeviceEnsemble

ap = argparse.ArgumentParser()
ap.add_argument("--configs", default="c2,c3")
ap.add_argument("--points", default="0.5:1,0.15:3", help="comma-separated ALPHA:Q")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--twin-users", type=int, default=3, help="sampled test users whose rows are checked against the twin")
ap.add_argument("--out", default=None, help="also append the report to this file")
a = ap.parse_args()
MAX_SUB, CHUNK = 8192, 8192  # songs per sub-range, train users per chunk (csrc/mr_uasym.hip)

if not torch.cuda.is_available():
    sys.exit("uasym_probe: no GPU (a timing needs the device; there is no fallback)")


def say(text=""):
    print(text, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


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


def probe(config):
    t0 = time.perf_counter()
    ds = synth.config(config).dataset()
    eng = Engine(ds, device=0, out_dtype="f32", topk=10)
    ens = DeviceEnsemble(eng)
    ext = torch.cuda.ExternalStream(eng.stream, device=ens.device)
    c_tr = np.bincount(np.asarray(ds.tr_songs), minlength=ds.n_songs).astype(np.int64)  # train listeners per song
    deg = np.diff(np.asarray(ds.tr_off)).astype(np.int64)
    n_sub = -(-eng.block_songs // min(eng.block_songs, MAX_SUB))
    n_chunks = -(-ds.n_train // CHUNK)
    keys = evaluation.asym_user_keys(ds, 0.5, 1, 32)
    nbrs = sum(int(v.size) for v, _k in keys)
    walked = sum(int(deg[v].sum()) for v, _k in keys) * n_sub
    say(f"{config}: {ds.n_train} train users, {ds.n_test} test users, {ds.n_songs} songs; shape {eng.shape}, "
        f"{eng.n_tiles} tiles of {eng.block_songs} songs, {n_sub} sub-range(s) per tile, {n_chunks} train-user chunk(s) "
        f"(setup {time.perf_counter() - t0:.1f} s)")
    say(f"  work per call: {int(c_tr[np.asarray(ds.te_songs)].sum()) } listener ids read and {nbrs} neighbours written by "
        f"{n_chunks * ds.n_test} stage-1 workgroups; {walked} tile-local song ids walked by "
        f"{eng.n_tiles * n_sub * ds.n_test} stage-2 workgroups; scratch {12 * ds.n_train * ds.n_test} B")
    out = ens.empty()
    rng = np.random.default_rng(23)
    users = np.sort(rng.choice(ds.n_test, size=min(a.twin_users, ds.n_test), replace=False))
    med = {}
    for point in a.points.split(","):
        alpha, q = float(point.split(":")[0]), int(point.split(":")[1])
        torch.cuda.synchronize()
        ms = timed(ext, lambda: eng.ubm_asym(alpha, q, out.data_ptr()))
        exp = evaluation.asym_user_model(ds, alpha, q, 32, users=users).astype(np.float32)
        got = out[torch.from_numpy(users).to(out.device)].cpu().numpy()
        assert np.array_equal(got.view(np.int32), exp.view(np.int32)), (config, point)
        med[point] = statistics.median(ms)
        say(f"  mr_ubm_asym_device alpha={alpha} q={q} F=32 (f32 out): min {min(ms):.3f}  median {med[point]:.3f}  "
            f"max {max(ms):.3f} ms ({len(ms)} reps); rows of users {users.tolist()} bit-equal to the numpy twin")
    ms = timed(ext, lambda: (eng.run("ubm"), eng.sync()))
    ubm = statistics.median(ms)
    say(f"  one UserBasedModel step of this context (top-10 + dense f32): "
        f"min {min(ms):.3f}  median {ubm:.3f}  max {max(ms):.3f} ms")
    say("  ratio of medians, call / UserBasedModel step: " + ", ".join(f"{p} {m / ubm:.1f}x" for p, m in med.items()))
    eng.close()


for cfg in [c for c in a.configs.split(",") if c]:
    probe(cfg)
