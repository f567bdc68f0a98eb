"""Parameter sweep against the materialised loop it replaces, on one GPU in f32:
for each config (default c3 c5) the two models are computed once, then 11
linear and 11 stochastic values are evaluated both ways — ens.linear /
ens.stochastic + ens.threshold_map per value, and ens.sweep — each timed with
a device synchronisation either side, minimum of 3 repeats. Prints both times,
their ratio and the byte-model ratio 5·P·M : 2M·(1 + ceil(P/G)); asserts that
the two paths return identical mAPs.

    python scripts/sweep_probe.py [--group G] [config ...]

--group only labels the byte model: G is the library's compile-time
MR_SWEEP_G (a variant library is selected with MR_ENGINE_LIB)."""
import argparse, math, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from musicrecommendation_amd import evaluation, synth
from musicrecommendation_amd.engine import Engine
from musicrecommendation_amd.ensemble import DeviceEnsemble

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["c3", "c5"])
ap.add_argument("--group", type=int, default=4)
ap.add_argument("--values", type=int, default=11)
a = ap.parse_args()
P, G = a.values, a.group
params = [i / (P - 1) for i in range(P)] if P > 1 else [0.5]


def best_of(f, n=3):
    ts, r = [], None
    for _ in range(n):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t))
    return min(ts), r


print(f"library variant: {os.environ.get('MR_ENGINE_LIB', '') or 'default'}; P = {P}, G = {G}", flush=True)
for name in a.configs:
    t0 = time.perf_counter()
    ds = synth.config(name).dataset()
    eng = Engine(ds, device=0, out_dtype="f32", topk=10)
    ens = DeviceEnsemble(eng, pos=evaluation.label_pos(ds), n_label_songs=ds.n_label_songs)
    ubm, ibm = ens.model("ubm"), ens.model("ibm")
    torch.cuda.synchronize()
    M = ubm.numel() * ubm.element_size()
    print(f"{name}: {ds.n_test} x {ds.n_songs} f32, M = {M / 1e9:.3f} GB (setup {time.perf_counter() - t0:.1f} s)",
          flush=True)
    model = 5.0 * P * M / (2.0 * M * (1 + math.ceil(P / G)))
    for kind, make in (("linear", lambda p: ens.linear(ubm, ibm, p)),
                       ("stochastic", lambda p: ens.stochastic(ubm, ibm, p, seed=1))):
        t_mat, m_mat = best_of(lambda: [ens.threshold_map(make(p)) for p in params])
        t_swp, m_swp = best_of(lambda: ens.sweep(kind, ubm, ibm, params, seed=1))
        assert m_mat == m_swp, (name, kind, m_mat, m_swp)
        print(f"  {kind:10s} materialised {t_mat:9.2f} ms   sweep {t_swp:9.2f} ms   ratio {t_mat / t_swp:5.2f}x"
              f"   byte model {model:4.2f}x   best {max(zip(m_swp, params))[1]:.2f} (mAP {max(m_swp):.6f})",
              flush=True)
    eng.close()
    del ubm, ibm, ens, eng
    torch.cuda.empty_cache()
