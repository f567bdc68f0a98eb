"""C2 kernel A/B: device time per step of the fused C2 step (graph of K steps,
HIP events on the engine stream, as bench.py), for engine options given as
key=value pairs, several rounds interleaved so drift hits every variant alike.
The library variant comes from MR_ENGINE_LIB (scripts/build_variant.py).

    python scripts/c2_ab.py [--steps 2000] [--rounds 3] "label:topk_lists=1" "label2:"

An UPPER_CASE key is an environment variable that mr_load reads, set while
that variant's engine is built: "nt512:MR_FUSED_NT=512,MR_FUSED_LEAN=1".

--other-tree DIR adds the engine of another checkout (DIR holds its own
musicrecommendation_amd package with its built library) twice, as `other_a`
and `other_b`, in the same process and rounds: the gap between their medians
is the session's noise, and the line carries `noise_us` and, per variant,
whether its slowest round beats the other tree's fastest by more than five
times that gap.
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401

from musicrecommendation_amd import synth  # noqa: E402
from musicrecommendation_amd.engine import Engine  # noqa: E402


def parse(spec):
    label, _, kv = spec.partition(":")
    opts, env = {}, {}
    for item in filter(None, kv.split(",")):
        k, v = item.split("=")
        if k.isupper():
            env[k] = v
            continue
        opts[k] = {"0": False, "1": True}.get(v, v) if k in ("topk_lists",) else (
            int(v) if v.lstrip("-").isdigit() else v)
    return label, opts, env


def other_engine_class(tree):
    """The Engine class of another checkout, its package loaded under an alias
    (its ctypes binding opens that tree's own library)."""
    pkg = os.path.join(os.path.abspath(tree), "musicrecommendation_amd")
    spec = importlib.util.spec_from_file_location("mr_other_tree", os.path.join(pkg, "__init__.py"),
                                                  submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["mr_other_tree"] = mod
    spec.loader.exec_module(mod)
    import mr_other_tree.engine as oe
    import mr_other_tree.synth as osynth
    return oe.Engine, osynth


def build(cls, ds, opts, env, model, steps):
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = cls(ds, out_dtype="f32", topk=10, **opts)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    e.graph_capture(model, steps)
    e.graph_launch()
    e.sync()
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("variants", nargs="*")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--config", default="c2")
    ap.add_argument("--model", default="ibm")
    ap.add_argument("--other-tree", default=None)
    a = ap.parse_args()
    ds = synth.config(a.config).dataset()
    engines, info = [], {}
    if a.other_tree:
        cls, osynth = other_engine_class(a.other_tree)
        ods = osynth.config(a.config).dataset()
        for label in ("other_a", "other_b"):
            engines.append((label, build(cls, ods, {}, {}, a.model, a.steps)))
    for spec in a.variants:
        label, opts, env = parse(spec)
        e = build(Engine, ds, opts, env, a.model, a.steps)
        info[label] = {"fused_threads": e.fused_threads, "fused_lean": e.fused_lean, "block_songs": e.block_songs,
                       "n_tiles": e.n_tiles}
        engines.append((label, e))
    res = {label: [] for label, _ in engines}
    for _ in range(a.rounds):
        for label, e in engines:
            e.timing_begin()
            e.graph_launch()
            _n, ms = e.timing_end()
            res[label].append(ms / a.steps * 1e3)
    out = {"lib": os.environ.get("MR_ENGINE_LIB", "prod"), "config": a.config, "model": a.model, "steps": a.steps,
           "us_per_step": {k: sorted(v) for k, v in res.items()}, "engines": info}
    if a.other_tree:
        ma, mb = (statistics.median(res[k]) for k in ("other_a", "other_b"))
        noise = abs(ma - mb)
        fastest = min(res["other_a"] + res["other_b"])
        out["noise_us"] = noise
        out["other_fastest_us"] = fastest
        out["clears_bar"] = {k: fastest - max(v) > 5 * noise for k, v in res.items() if not k.startswith("other_")}
        out["not_slower"] = {k: statistics.median(v) <= max(ma, mb) for k, v in res.items()
                             if not k.startswith("other_")}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
