"""Spark-free equivalent of the reference's drivers (src/main/scala/main.scala
MN:8-123, src/main/scala/distributed.scala DS:55-602) on the MI355X engine.

    python -m musicrecommendation_amd.driver TRAIN_N TEST_N [--resources DIR]
        [--devices 0,1,...] [--song-shards G_s] [--user-blocks G_u] [--distributed] [--quiet]
        [--sweep KIND:LO:HI:N ...] [--recommend K[:PATH]] [--similar K[:PATH]] [--asym ALPHA:Q]
        [--asym-user ALPHA:Q[:F]]

Same flow and output as main.scala: load train_{N}_{M}.txt, test_{N}_{M}.txt,
test_labels_{N}_{M}.txt (MN:21-23), build the recommender (untimed, MN:27),
time the user- and item-based models (MN:37-40), sort them by (user, song,
-score) (MN:57-59), time the linear / aggregation / stochastic combinations
with 0.5 (MN:62-89), evaluate all five with the threshold mAP (MN:101-110) and
print the mAPs rounded to 10 decimals (MN:112-121). Times print as
MyUtils.time does (my_utils/MyUtils.scala:4-15). --distributed follows
distributed.scala instead: defaults 300 / 10 (DS:61-62) and its evaluation's
11 thresholds 0.0..1.0 (DS:395-415) for every mAP.

The models stay on the device as dense buffers (ensemble.DeviceEnsemble): the
combinations and the mAP run as HIP kernels, nothing is materialised as a
pair list. With --devices / --song-shards / --user-blocks the two similarity
models are ALSO scored through one multi-GPU group (mr_group_*, the
distributed.scala strategies 1/2 as a single call: song shards x user blocks,
in-library RCCL across GPUs) and checked bit for bit against the
single-context models. The reference's sequential/parallel pairs collapse into
one GPU run each (seq = par holds by construction, README.md:254-261).

--sweep KIND:LO:HI:N (repeatable; KIND = linear, aggregation or stochastic)
runs after that flow: the mAP of that combination at N evenly spaced parameter
values from LO to HI over the same two device models, one line per value and
the best one — the experiment the reference's README leaves open, where the
driver and main.scala hard-code 0.5 (DeviceEnsemble.sweep: no combined model
is materialised).

--recommend K[:PATH] (K <= 1024) ranks each of the five models after the flow:
per test user the K best songs by (score desc, song asc), selected on the
device (DeviceEnsemble.rank), and prints each model's mAP truncated at K — the
Million Song Dataset Challenge's metric at K = 500 — beside the threshold
mAPs. With PATH the linear-combination model's lists are written there, one
"user<TAB>song<TAB>score" line per recommendation in (user, rank) order.

--similar K[:PATH] (K <= 1024) answers, after the flow, which songs are most
like each distinct song the test users have heard — the cosineSimilarity rows
(MR:230-239) the ItemBasedModel consumes: per such song the K songs with the
highest cosine over common train listeners (DeviceEnsemble.similar_songs). It
prints the query count and the time; with PATH the lists are written there,
one "song<TAB>other<TAB>cosine" line per entry in (song, rank) order.

--asym ALPHA:Q (ALPHA in [0, 1], Q in 1..8) adds a sixth model to the run,
asymmetricItemBasedModel: the item-based model with the similarity C /
(c(s)^ALPHA * c(s2)^(1-ALPHA)) raised to the power Q before the sum over T(u)
(DeviceEnsemble.item_based; 0.5:1 is the reference's model summed in fp64),
timed, evaluated and, with --recommend, ranked like the others.

--asym-user ALPHA:Q[:F] (ALPHA in [0, 1], Q in 1..8, F in 8..52, default: the
engine's 32) adds asymmetricUserBasedModel in the same way: the user-based model
with the neighbour weight |T(u) ∩ S(v)| / (|u|^ALPHA * |v|^(1-ALPHA)) raised to
the power Q, in fixed point with F fraction bits (DeviceEnsemble.user_based;
0.5:1 is the user-based model bit for bit). Both flags may be given.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import Callable, List, Optional, Sequence, Tuple, TypeVar

T = TypeVar("T")


def timed(f: Callable[[], T], what: str, verbose: bool = True) -> T:
    """MyUtils.time (MyUtils.scala:4-15): run, print the elapsed wall time."""
    import torch

    t0 = time.perf_counter_ns()
    r = f()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    dt = time.perf_counter_ns() - t0
    if verbose:
        print(f"Elapsed time for {what}:\t{dt // 1_000_000}ms ({dt}ns)", flush=True)
    return r


def round_at(p: int, x: float) -> float:
    """MyUtils.roundAt (MyUtils.scala:17): math.round(x * 10^p) / 10^p."""
    import math

    s = 10 ** p
    return math.floor(x * s + 0.5) / s


def parse_sweep(spec: str) -> Tuple[str, float, float, int]:
    """--sweep KIND:LO:HI:N -> (kind, lo, hi, n); ValueError on a bad spec."""
    from .ensemble import KINDS

    parts = spec.split(":")
    if len(parts) != 4:
        raise ValueError(f"--sweep {spec!r}: expected KIND:LO:HI:N")
    kind = parts[0]
    if kind not in KINDS:
        raise ValueError(f"--sweep {spec!r}: KIND must be one of {', '.join(KINDS)}")
    try:
        lo, hi, n = float(parts[1]), float(parts[2]), int(parts[3])
    except ValueError:
        raise ValueError(f"--sweep {spec!r}: LO and HI are numbers, N an integer") from None
    if n < 1:
        raise ValueError(f"--sweep {spec!r}: N must be at least 1")
    return kind, lo, hi, n


def parse_recommend(spec) -> Tuple[int, Optional[str]]:
    """--recommend K[:PATH] (or an int K, or (K, PATH)) -> (K, path or None);
    ValueError on a bad spec."""
    from ._lib import MR_RANK_MAX_K

    if isinstance(spec, (tuple, list)):
        k, path = spec[0], (spec[1] if len(spec) > 1 else None)
    elif isinstance(spec, str):
        head, sep, tail = spec.partition(":")
        k, path = head, (tail if sep else None)
        if sep and not tail:
            raise ValueError(f"--recommend {spec!r}: empty PATH")
    else:
        k, path = spec, None
    try:
        k = int(k)
    except (TypeError, ValueError):
        raise ValueError(f"--recommend {spec!r}: expected K[:PATH], K an integer") from None
    if not 1 <= k <= MR_RANK_MAX_K:
        raise ValueError(f"--recommend {spec!r}: K must be in [1, {MR_RANK_MAX_K}]")
    return k, (os.fspath(path) if path is not None else None)


def parse_similar(spec) -> Tuple[int, Optional[str]]:
    """--similar K[:PATH] (or an int K, or (K, PATH)) -> (K, path or None),
    parsed like --recommend; ValueError on a bad spec."""
    try:
        return parse_recommend(spec)
    except ValueError as e:
        raise ValueError(str(e).replace("--recommend", "--similar", 1)) from None


def parse_asym(spec) -> Tuple[float, int]:
    """--asym ALPHA:Q (or (alpha, q)) -> (alpha, q); ValueError on a bad spec."""
    from ._lib import MR_ASYM_MAX_Q

    if isinstance(spec, (tuple, list)):
        if len(spec) != 2:
            raise ValueError(f"--asym {spec!r}: expected ALPHA:Q")
        a, q = spec
    else:
        a, sep, q = str(spec).partition(":")
        if not sep:
            raise ValueError(f"--asym {spec!r}: expected ALPHA:Q")
    try:
        a, q = float(a), int(q)
    except (TypeError, ValueError):
        raise ValueError(f"--asym {spec!r}: ALPHA is a number, Q an integer") from None
    if not 0.0 <= a <= 1.0:  # NaN fails both comparisons
        raise ValueError(f"--asym {spec!r}: ALPHA must be in [0, 1]")
    if not 1 <= q <= MR_ASYM_MAX_Q:
        raise ValueError(f"--asym {spec!r}: Q must be in [1, {MR_ASYM_MAX_Q}]")
    return a, q


def parse_asym_user(spec) -> Tuple[float, int, Optional[int]]:
    """--asym-user ALPHA:Q[:F] (or (alpha, q) / (alpha, q, F)) -> (alpha, q, F
    or None for the engine's); ValueError on a bad spec."""
    if isinstance(spec, (tuple, list)):
        parts = list(spec)
    else:
        parts = str(spec).split(":")
    if len(parts) not in (2, 3):
        raise ValueError(f"--asym-user {spec!r}: expected ALPHA:Q[:F]")
    try:
        a, q = parse_asym(tuple(parts[:2]))
    except ValueError as e:  # the same checks, named for this flag
        raise ValueError(f"--asym-user {spec!r}: {str(e).rsplit(': ', 1)[-1]}") from None
    f = None
    if len(parts) == 3 and parts[2] is not None:
        try:
            f = int(parts[2])
        except (TypeError, ValueError):
            raise ValueError(f"--asym-user {spec!r}: F is an integer") from None
        if not 8 <= f <= 52:
            raise ValueError(f"--asym-user {spec!r}: F must be in [8, 52]")
    return a, q, f


def sweep_grid(lo: float, hi: float, n: int) -> List[float]:
    """N evenly spaced values LO + i*(HI-LO)/(N-1) (N = 1: LO alone)."""
    return [lo + i * (hi - lo) / (n - 1) for i in range(n)] if n > 1 else [lo]


def run(train_n: int, test_n: int, resources: str, devices: Optional[Sequence[int]] = None,
        song_shards: Optional[int] = None, user_blocks: int = 1, verbose: bool = True, seed: int = 1,
        distributed: bool = False, sweeps: Optional[Sequence[str]] = None, recommend=None, similar=None,
        asym=None, asym_user=None) -> dict:
    import numpy as np

    from .dataset import Dataset
    from .engine import Engine
    from .ensemble import DeviceEnsemble, best

    specs = [parse_sweep(s) if isinstance(s, str) else tuple(s) for s in (sweeps or [])]  # before any work
    rec = parse_recommend(recommend) if recommend is not None else None
    sim = parse_similar(similar) if similar is not None else None
    asy = parse_asym(asym) if asym is not None else None
    uasy = parse_asym_user(asym_user) if asym_user is not None else None

    n_thr = 11 if distributed else 10  # DS:395 vs MR:590
    if song_shards is None:  # one song shard per listed GPU and user block (DS:477-479's song partition)
        song_shards = max(1, len(devices) // max(1, user_blocks)) if devices else 1
    if verbose:
        print(f"Train users: {train_n}\nTest users: {test_n}", flush=True)
    paths = [os.path.join(resources, f"{k}_{train_n}_{test_n}.txt") for k in ("train", "test", "test_labels")]
    for p in paths:
        if not os.path.exists(p):
            raise FileNotFoundError(p)
    if verbose:
        print("Loaded files", flush=True)
    ds = Dataset.from_tsv(*paths)                                     # MN:27, untimed
    dev = devices[0] if devices else 0
    eng = Engine(ds, device=dev, out_dtype="f64", topk=10)
    ens = DeviceEnsemble(eng)
    if verbose:
        print("MusicRecommender instanced", flush=True)
    ubm = timed(lambda: ens.model("ubm"), "user-based model", verbose)     # MN:37-38
    ibm = timed(lambda: ens.model("ibm"), "item-based model", verbose)     # MN:39-40
    group_checked = None
    if devices and (len(devices) > 1 or song_shards > 1 or user_blocks > 1):
        from .group import Group

        with Group(ds, song_shards=song_shards, user_blocks=user_blocks, devices=devices, out_dtype="f64",
                   topk=10) as g:
            for name, t in (("user-based", ubm), ("item-based", ibm)):
                # run AND drain every context's stream inside the timed region
                timed(lambda: (g.run("ubm" if name == "user-based" else "ibm"), g.sync()),
                      f"{name} model ({g.transport}, {song_shards} song shards x {user_blocks} user blocks)",
                      verbose)
                if not np.array_equal(g.dense(), t.cpu().numpy(), equal_nan=True):
                    raise AssertionError(f"multi-GPU {name} model differs from the single-context model")
        group_checked = True
    # MN:57-59 sorts by (user, song, -score): the dense rows are in that order
    # already (lexicographic ids), the combinations index pairs in it.
    lcm = timed(lambda: ens.linear(ubm, ibm, 0.5), "linear-combination model", verbose)          # MN:62-69
    am = timed(lambda: ens.aggregation(ubm, ibm, 0.5), "aggregation model", verbose)             # MN:70-77
    scm = timed(lambda: ens.stochastic(ubm, ibm, 0.5, seed=seed), "stochastic-combination model", verbose)
    models = [("user-based", ubm), ("item-based", ibm), ("linear-combination", lcm), ("aggregation", am),
              ("stochastic-combination", scm)]
    if asy is not None:
        models.append(("asymmetricItemBasedModel",
                       timed(lambda: ens.item_based(*asy), f"asymmetricItemBasedModel (alpha {asy[0]}, q {asy[1]})",
                             verbose)))
    if uasy is not None:
        models.append(("asymmetricUserBasedModel",
                       timed(lambda: ens.user_based(*uasy),
                             f"asymmetricUserBasedModel (alpha {uasy[0]}, q {uasy[1]})", verbose)))
    maps = {}
    for name, t in models:
        maps[name] = timed(lambda: ens.threshold_map(t, n_thresholds=n_thr), f"{name} model mAP", verbose)  # MN:101-110
    for name, v in maps.items():
        print(f"{name} model mAP: {round_at(10, v)}", flush=True)                              # MN:112-121
    ranked = {}
    if rec is not None:
        from . import modelio

        rk, rpath = rec
        for name, t in models:
            lists = timed(lambda: ens.rank(t, rk), f"{name} model top-{rk} lists", verbose)
            ranked[name] = ens.map_at(lists, rk)
            if rpath is not None and name == "linear-combination":
                songs, scores = lists[0].cpu().numpy(), lists[1].cpu().numpy()
                modelio.write_recommendations(rpath, [
                    (ds.test_names(u), [(ds.song_names(int(g)), float(x))
                                        for g, x in zip(songs[u], scores[u]) if g >= 0])
                    for u in range(ds.n_test)])
        for name, v in ranked.items():
            print(f"{name} model mAP@{rk}: {round_at(10, v)}", flush=True)
    swept = []
    for kind, lo, hi, n in specs:
        params = sweep_grid(lo, hi, n)
        vals = timed(lambda: ens.sweep(kind, ubm, ibm, params, seed=seed, n_thresholds=n_thr),
                     f"{kind} sweep ({n} values)", verbose)
        for p, v in zip(params, vals):
            print(f"{kind} sweep {p} mAP: {round_at(10, v)}", flush=True)
        b = best(params, vals)
        print(f"{kind} sweep best: {b} mAP: {round_at(10, vals[params.index(b)])}", flush=True)
        swept.append({"kind": kind, "params": params, "mAP": vals, "best": b})
    n_sim = 0
    if sim is not None:
        from . import modelio

        sk, spath = sim
        queries = np.unique(np.asarray(ds.te_songs, dtype=np.int32))  # every song of some T(u)
        n_sim = int(queries.size)
        print(f"similar-song queries: {n_sim}", flush=True)
        lists = timed(lambda: ens.similar_songs(queries, sk), f"top-{sk} similar songs of {n_sim} songs", verbose)
        if spath is not None:
            songs, scores = lists[0].cpu().numpy(), lists[1].cpu().numpy()
            modelio.write_recommendations(spath, [
                (ds.song_names(int(q)), [(ds.song_names(int(g)), float(x))
                                         for g, x in zip(songs[i], scores[i]) if g >= 0])
                for i, q in enumerate(queries)])
    eng.close()
    out = {"mAP": maps, "multi_gpu_checked": group_checked, "thresholds": n_thr,
           "layout": (song_shards, user_blocks)}
    if specs:
        out["sweeps"] = swept
    if rec is not None:
        out["mAP@K"] = ranked
        out["recommend"] = {"K": rec[0], "path": rec[1]}
    if asy is not None:
        out["asym"] = {"alpha": asy[0], "q": asy[1]}
    if uasy is not None:
        out["asym_user"] = {"alpha": uasy[0], "q": uasy[1], "frac_bits": uasy[2]}
    if sim is not None:
        out["similar"] = {"K": sim[0], "path": sim[1], "queries": n_sim}
    return out


def _sweep_arg(spec: str) -> Tuple[str, float, float, int]:
    try:
        return parse_sweep(spec)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _recommend_arg(spec: str) -> Tuple[int, Optional[str]]:
    try:
        return parse_recommend(spec)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _similar_arg(spec: str) -> Tuple[int, Optional[str]]:
    try:
        return parse_similar(spec)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _asym_arg(spec: str) -> Tuple[float, int]:
    try:
        return parse_asym(spec)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _asym_user_arg(spec: str) -> Tuple[float, int, Optional[int]]:
    try:
        return parse_asym_user(spec)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def main(argv: Optional[Sequence[str]] = None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("train_n", type=int, nargs="?", default=None)  # MN:15 default 100 (DS:61: 300)
    ap.add_argument("test_n", type=int, nargs="?", default=10)     # MN:16 / DS:62 default
    ap.add_argument("--resources", default=".", help="directory of the train/test/test_labels TSV files")
    ap.add_argument("--devices", default="", help="comma-separated GPU ids for the multi-GPU group")
    ap.add_argument("--song-shards", type=int, default=None,
                    help="default: one per listed device and user block")
    ap.add_argument("--user-blocks", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1, help="stochastic combination seed (the reference's is unseeded)")
    ap.add_argument("--distributed", action="store_true",
                    help="distributed.scala's flow: defaults 300/10, 11-threshold mAP (DS:61-62, DS:395)")
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--sweep", action="append", default=[], metavar="KIND:LO:HI:N", type=_sweep_arg,
                    help="after the flow, the mAP of KIND (linear, aggregation, stochastic) at N evenly spaced "
                         "parameter values from LO to HI; repeatable")
    ap.add_argument("--recommend", default=None, metavar="K[:PATH]", type=_recommend_arg,
                    help="after the flow, rank the K best songs per test user of each model (K <= 1024), print "
                         "each model's mAP@K, and write the linear-combination model's lists to PATH")
    ap.add_argument("--similar", default=None, metavar="K[:PATH]", type=_similar_arg,
                    help="after the flow, the K songs most like each distinct song the test users have heard "
                         "(K <= 1024; cosine over common train listeners); the lists are written to PATH")
    ap.add_argument("--asym", default=None, metavar="ALPHA:Q", type=_asym_arg,
                    help="add the asymmetric-cosine (ALPHA in [0, 1]), locality-Q (1..8) item-based model to the run "
                         "as asymmetricItemBasedModel")
    ap.add_argument("--asym-user", default=None, metavar="ALPHA:Q[:F]", type=_asym_user_arg,
                    help="add the asymmetric-cosine (ALPHA in [0, 1]), locality-Q (1..8) user-based model with F "
                         "fraction bits (8..52, default: the engine's) to the run as asymmetricUserBasedModel")
    a = ap.parse_args(argv)
    devices = [int(x) for x in a.devices.split(",") if x.strip()] if a.devices else None
    train_n = a.train_n if a.train_n is not None else (300 if a.distributed else 100)
    run(train_n, a.test_n, a.resources, devices, a.song_shards, a.user_blocks, verbose=not a.quiet, seed=a.seed,
        distributed=a.distributed, sweeps=a.sweep, recommend=a.recommend, similar=a.similar, asym=a.asym,
        asym_user=a.asym_user)
    return 0


if __name__ == "__main__":
    sys.exit(main())
