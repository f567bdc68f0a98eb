"""The asymmetric-cosine, locality-q item-based model at the C2, C3 (and C4)
shapes on one GPU: times mr_ibm_asym_device at (alpha, q) = (0.15, 3) and
(0.5, 1) with device events on the engine's stream over --reps repetitions
after --warmup untimed ones (minimum, median, maximum printed).

Beside each time, the work the path does (computed from the dataset): the
listener-list walks, one per (test user, heard song with train listeners, song
sub-range), and the listener ids and tile-local song ids they read.

Same-session context, no margin attached to it: one ItemBasedModel step
(Engine.run("ibm")) of the same context. The device rows of --twin-users
sampled test users are checked against the numpy twin
(evaluation.asym_item_model), bit for bit.

    python scripts/asym_probe.py [--configs c2,c3] [--reps 5] [--warmup 1] [--out FILE]
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
ap.add_argument("--points", default="0.15:3,0.5:1", help="comma-separated ALPHA:Q")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--twin-users", type=int, default=3, help="sampled test users whose rows are checked against the twin")
ap.add_argument("--out", default=None, help="also append the report to this file")
a = ap.parse_args()
MAX_SUB = 8192  # songs per sub-range (csrc/mr_asym.hip)

if not torch.cuda.is_available():
    sys.exit("asym_probe: no GPU (a timing needs the device; there is no fallback)")


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
    tr_songs = np.asarray(ds.tr_songs)
    c_tr = np.bincount(tr_songs, minlength=ds.n_songs).astype(np.int64)   # train listeners per song
    deg = np.diff(np.asarray(ds.tr_off)).astype(np.int64)
    seg = np.bincount(tr_songs, weights=np.repeat(deg, deg), minlength=ds.n_songs)  # Σ_{v in L_tr(s)} |S(v)|
    te = np.asarray(ds.te_songs)
    n_sub = -(-eng.block_songs // min(eng.block_songs, MAX_SUB))
    walks = int((c_tr[te] > 0).sum()) * eng.n_tiles * n_sub
    ids = int(c_tr[te].sum()) * eng.n_tiles * n_sub
    say(f"{config}: {ds.n_train} train users, {ds.n_test} test users, {ds.n_songs} songs; shape {eng.shape}, "
        f"{eng.n_tiles} tiles of {eng.block_songs} songs, {n_sub} sub-range(s) per tile "
        f"(setup {time.perf_counter() - t0:.1f} s)")
    say(f"  work per call: {te.size} (user, heard song) pairs, {walks} listener-list walks, {ids} listener ids and "
        f"{int(seg[te].sum()) * n_sub} tile-local song ids read, {eng.n_tiles * n_sub * ds.n_test} workgroups")
    out = ens.empty()
    rng = np.random.default_rng(23)
    users = np.sort(rng.choice(ds.n_test, size=min(a.twin_users, ds.n_test), replace=False))
    for point in a.points.split(","):
        alpha, q = float(point.split(":")[0]), int(point.split(":")[1])
        torch.cuda.synchronize()
        ms = timed(ext, lambda: eng.ibm_asym(alpha, q, out.data_ptr()))
        t1 = time.perf_counter()
        exp = evaluation.asym_item_model(ds, alpha, q, users=users).astype(np.float32)
        twin_s = (time.perf_counter() - t1) / users.size
        got = out[torch.from_numpy(users).to(out.device)].cpu().numpy()
        assert np.array_equal(got.view(np.int32), exp.view(np.int32)), (config, point)
        say(f"  mr_ibm_asym_device alpha={alpha} q={q} (f32 out): min {min(ms):.3f}  median {statistics.median(ms):.3f}  "
            f"max {max(ms):.3f} ms ({len(ms)} reps); rows of users {users.tolist()} bit-equal to the numpy twin "
            f"({twin_s:.2f} s per user on the host)")
    ms = timed(ext, lambda: (eng.run("ibm"), eng.sync()))
    say(f"  one ItemBasedModel step of this context (route {eng.ibm_route}, top-10 + dense f32): "
        f"min {min(ms):.3f}  median {statistics.median(ms):.3f}  max {max(ms):.3f} ms")
    eng.close()


for cfg in [c for c in a.configs.split(",") if c]:
    probe(cfg)
