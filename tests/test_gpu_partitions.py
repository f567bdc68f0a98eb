"""Every host loop that cuts a device call into pieces, past its first iteration.

Two kinds of loop split the work of the entry points that give one grid row to
a test user (or a query): the two-hop user batch of run_model
(LaunchPlan.batch, sized from a memory budget) and the launch splits at the
grid-row limit (65,535 / 65,528 rows). On every input small enough for a test
both run once, so the offset arithmetic of the later pieces — top_key +
(user0 + y0) * k, nbr_v + y0 * cap against a launch-local user, pair_base +
y0 * n_songs with a shifted te_off, part + y0 * gx * 6, dense_dev + b0 * width
— is never executed. The diagnostic settings MR_BATCH_USERS (read by mr_load)
and MR_LAUNCH_ROWS (read by every call that launches) lower both limits:
with 37 test users, MR_BATCH_USERS=16 gives batches of 16, 16 and 5 users and
MR_LAUNCH_ROWS=8 launches of 8, 8, 8, 8 and 5 rows — the last one partial and
padded, and no piece count divides 37 (21 users: launches of 8, 8 and 5).

Every comparison is bitwise, against the references the suite already uses
(the fixed-point oracle, the numpy twins in evaluation, the host merge, the
reference combination formulas), never against an unsplit run alone.
"""
import numpy as np
import pytest
import torch

from musicrecommendation_amd import _lib, evaluation, synth
from musicrecommendation_amd.engine import Engine, merge_topk_host
from musicrecommendation_amd.ensemble import AGGREGATION, LINEAR, STOCHASTIC, DeviceEnsemble
from musicrecommendation_amd.group import Group
from musicrecommendation_amd.sharding import song_shards
from oracle import native

from helpers import pair_index, reference_combination

pytestmark = pytest.mark.gpu

N_TEST = 37
BATCH, ROWS = 16, 8
KNOBS = [(BATCH, None), (None, ROWS), (BATCH, ROWS)]
MODELS = ("ubm", "ibm")
# tiling -> Engine keywords: many tiles, the shape's own tiling, one tile (the
# kernel writes the lists itself: no merge launch)
TILINGS = {
    "many": dict(block_songs=256),
    "default": dict(),
    "single": dict(song_lo=2000, song_hi=2000 + 8192, block_songs=8192),
}

_ds = {}
_oracle = {}
_twin = {}


def dataset(n_test=N_TEST):
    if n_test not in _ds:
        _ds[n_test] = synth.config("c2", n_test=n_test).dataset()
    return _ds[n_test]


def oracle(model, lo=0, hi=0, k=10, n_test=N_TEST):
    """The fixed-point oracle's (dense, songs, keys) of a shard: computed once, never written to."""
    key = (n_test, model, lo, hi, k)
    if key not in _oracle:
        out = native.fp_model(dataset(n_test), model, song_lo=lo, song_hi=hi, k=k)
        for a in out:
            a.setflags(write=False)
        _oracle[key] = out
    return _oracle[key]


def set_knobs(monkeypatch, batch, rows):
    for name, value in (("MR_BATCH_USERS", batch), ("MR_LAUNCH_ROWS", rows)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))


def pieces(n, per):
    return -(-n // per)


def launches_per_run(n_test, batch, rows):
    """Scoring launches of one two-hop run: each batch is cut into launches of `rows` users."""
    return sum(pieces(min(batch, n_test - u0), rows) for u0 in range(0, n_test, batch))


def assert_lists(e, model, k):
    songs, scores, keys = e.topk()
    _, ts, tk = oracle(model, e.song_lo, e.song_hi, k, e.n_test)
    assert np.array_equal(songs, ts), "top-k songs differ from the fixed-point oracle"
    assert np.array_equal(keys, tk), "top-k keys differ from the fixed-point oracle"
    valid = keys >= 0
    assert np.array_equal(scores[valid], keys[valid].view(np.float64))
    assert np.isnan(scores[~valid]).all()


def assert_dense(e, model, k, dtype="f64"):
    exp = oracle(model, e.song_lo, e.song_hi, k, e.n_test)[0]
    if dtype == "f32":
        exp = exp.astype(np.float32)  # rounded once
    got = e.dense()
    assert got.dtype == exp.dtype
    assert np.array_equal(got, exp, equal_nan=True), "dense scores differ from the fixed-point oracle"
    return exp


def assert_minmax(e, exp):
    """The scoring kernels' per-user min / max rows (wide shape) against the min/max kernel and numpy."""
    mm = e.dense_minmax()
    assert mm is not None
    assert mm == e.eval_minmax(e.device_outputs()[0])
    assert mm == (float(np.nanmin(exp)), float(np.nanmax(exp)))


def open_engine(shape, model, **kw):
    return Engine(dataset(kw.pop("n_test", N_TEST)), stage1=shape, ibm_route="two_hop" if model == "ibm" else "auto",
                  **kw)


def assert_batch(e, shape, batch):
    assert e.shape == shape
    assert e.batch == (batch if batch is not None and shape != "fused" else e.n_test)


# ---- 1. two-hop runs ----------------------------------------------------------
@pytest.mark.parametrize("tiling", list(TILINGS))
@pytest.mark.parametrize("batch,rows", KNOBS)
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", ["separate", "wide", "fused"])
def test_two_hop_runs(shape, model, batch, rows, tiling, monkeypatch):
    set_knobs(monkeypatch, batch, rows)
    with open_engine(shape, model, out_dtype="f64", topk=10, **TILINGS[tiling]) as e:
        assert_batch(e, shape, batch)
        assert e.n_test == N_TEST
        assert tiling == "default" or (e.n_tiles == 1) == (tiling == "single")
        e.run(model)
        exp = assert_dense(e, model, 10)
        assert_lists(e, model, 10)
        if shape == "wide":
            assert_minmax(e, exp)
        e.run(model)  # hand-off counters and batch buffers are reusable after a split run
        assert_lists(e, model, 10)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("shape", ["separate", "wide", "fused"])
def test_two_hop_runs_f32(shape, model, monkeypatch):
    set_knobs(monkeypatch, BATCH, ROWS)
    with open_engine(shape, model, out_dtype="f32", topk=10) as e:
        assert_batch(e, shape, BATCH)
        e.run(model)
        exp = assert_dense(e, model, 10, "f32")
        assert_lists(e, model, 10)
        if shape == "wide":
            assert_minmax(e, exp)


@pytest.mark.parametrize("k", [1, 16])
@pytest.mark.parametrize("tiling", ["many", "default"])
@pytest.mark.parametrize("batch,rows", KNOBS)
@pytest.mark.parametrize("model", MODELS)
def test_wide_topk_only_candidate_mode(model, batch, rows, tiling, k, monkeypatch):
    set_knobs(monkeypatch, batch, rows)
    monkeypatch.delenv("MR_WIDE_CAND", raising=False)
    with open_engine("wide", model, topk=k, dense=False, **TILINGS[tiling]) as e:
        assert_batch(e, "wide", batch)
        assert e.candidate_topk
        e.run(model)
        assert_lists(e, model, k)
        assert e.dense_minmax() is None


# ---- 2. co-listening route ------------------------------------------------------
@pytest.mark.parametrize("tiling", list(TILINGS))
def test_colistening_route(tiling, monkeypatch):
    ds = dataset()
    kw = dict(stage1="wide", ibm_route="cooc", topk=10, **TILINGS[tiling])
    set_knobs(monkeypatch, None, None)
    with Engine(ds, out_dtype="f64", **kw) as e:
        e.run("ibm")
        ref_stats, ref_bytes = e.cooc_stats(), e.cooc_bytes()
    set_knobs(monkeypatch, None, ROWS)
    with Engine(ds, out_dtype="f64", **kw) as e:
        assert e.ibm_route == "cooc" and e.shape == "wide" and e.batch == N_TEST
        e.run("ibm")
        exp = assert_dense(e, "ibm", 10)
        assert_lists(e, "ibm", 10)
        assert_minmax(e, exp)
        assert e.cooc_stats() == ref_stats and e.cooc_bytes() == ref_bytes
        e.run("ubm")  # the two-hop model of the same context, split the same way
        assert_dense(e, "ubm", 10)
        assert_lists(e, "ubm", 10)
    for k in (1, 16):
        ref = None
        for rows in (None, ROWS):
            set_knobs(monkeypatch, None, rows)
            with Engine(ds, dense=False, **dict(kw, topk=k)) as e:
                assert e.ibm_route == "cooc" and e.candidate_topk
                e.run("ibm")
                assert_lists(e, "ibm", k)
                got = (e.cooc_stats(), e.cooc_bytes())
            ref = got if ref is None else ref
            assert got == ref


# ---- 3. graph capture and timing ---------------------------------------------------
@pytest.mark.parametrize("model,route", [("ubm", "auto"), ("ibm", "two_hop"), ("ibm", "cooc")])
def test_graph_capture_of_several_batches(model, route, monkeypatch):
    set_knobs(monkeypatch, BATCH, ROWS)
    with Engine(dataset(), out_dtype="f64", topk=10, stage1="wide", ibm_route=route) as e:
        assert e.batch == BATCH
        e.graph_capture(model, 3)
        for _ in range(2):
            e.graph_launch()
        e.sync()
        assert_lists(e, model, 10)
        assert_dense(e, model, 10)


@pytest.mark.parametrize("model,route", [("ubm", "auto"), ("ibm", "two_hop"), ("ibm", "cooc")])
def test_timing_counts_launches_and_batches(model, route, monkeypatch):
    """The timing window counts one launch per scoring launch; the kernel
    timing takes one ring slot per two-hop batch (one per co-listening run)."""
    set_knobs(monkeypatch, BATCH, ROWS)
    R = 3
    per_run = pieces(N_TEST, ROWS) if route == "cooc" else launches_per_run(N_TEST, BATCH, ROWS)
    assert per_run == 5
    with Engine(dataset(), out_dtype="f64", topk=10, stage1="wide", ibm_route=route) as e:
        e.run(model)
        e.sync()
        e.timing_begin()
        for _ in range(R):
            e.run(model)
        n, _ms = e.timing_end()
        assert n == R * per_run
        assert_lists(e, model, 10)
    with Engine(dataset(), out_dtype="f64", topk=10, stage1="wide", ibm_route=route, time_kernels=True) as e:
        for _ in range(R):
            e.run(model)
        slots = R if route == "cooc" else R * pieces(N_TEST, BATCH)
        assert e.kernel_times("score")[0] == slots
        assert e.kernel_times("neighbours")[0] == slots
        assert_lists(e, model, 10)
        assert_dense(e, model, 10)


# ---- 4. combinations ------------------------------------------------------------------
N_COMB = 21
COMB_LAYOUTS = {"full": (0, 0, 0, N_COMB), "song_shard": (3000, 9000, 0, N_COMB), "user_block": (0, 0, 3, 20)}
COMB_CASES = [("linear", LINEAR, 0.3), ("aggregation", AGGREGATION, 0.37), ("stochastic", STOCHASTIC, 0.5)]
# (0.37 of the pairs end inside the first launch's users; 0.6 puts the switch from ibm to ubm in the second launch)
COMB_EXTRA = [("aggregation", AGGREGATION, 0.6)]


SEED = 5
_comb_ref = {}


class CombContext:
    """One layout's context with its own ubm and ibm on the device, and the
    reference combination of exactly those two models (computed once per
    layout, dtype, kind and parameter)."""

    def __init__(self, layout, dtype):
        ds = dataset(N_COMB)
        song_lo, song_hi, a, b = COMB_LAYOUTS[layout]
        sub = ds if (a, b) == (0, ds.n_test) else ds.subset_test_users(a, b)
        self.key = (layout, dtype)
        self.dtype = dtype
        self.base = a * ds.n_songs - int(ds.te_off[a])
        self.n_pairs = ds.n_pairs()
        assert (self.base > 0) == (layout == "user_block") and sub.n_test > 2 * ROWS
        self.e = Engine(sub, out_dtype=dtype, song_lo=song_lo, song_hi=song_hi)
        self.ens = DeviceEnsemble(self.e, pair_base=self.base, n_pairs=self.n_pairs)
        self.u_t, self.i_t = self.ens.model("ubm"), self.ens.model("ibm")
        self.sub = sub

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()

    def reference(self, name, param):
        key = self.key + (name, param)
        if key not in _comb_ref:
            ubm = self.u_t.cpu().numpy().astype(np.float64)
            ibm = self.i_t.cpu().numpy().astype(np.float64)
            tail = ~np.isnan(ubm[ROWS:])
            assert (ubm[ROWS:][tail] != ibm[ROWS:][tail]).any()  # a wrong choice in a later launch shows
            idx = pair_index(self.sub, self.e.song_lo, self.e.song_hi, pair_base=self.base)
            exp = reference_combination(name, ubm, ibm, param, idx, self.n_pairs, seed=SEED)
            if self.dtype == "f32":
                exp = exp.astype(np.float32).astype(np.float64)  # rounded once
            exp.setflags(write=False)
            _comb_ref[key] = exp
        return _comb_ref[key]

    def combine(self, kind, param):
        out = self.ens.empty()
        self.ens._after_torch()
        self.e.combine(kind, param, self.u_t.data_ptr(), self.i_t.data_ptr(), out.data_ptr(), seed=SEED,
                       pair_base=self.base, n_pairs=self.n_pairs)
        return out.cpu().numpy()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("name,kind,param", COMB_CASES + COMB_EXTRA)
@pytest.mark.parametrize("layout", list(COMB_LAYOUTS))
def test_combine_device(layout, name, kind, param, dtype, monkeypatch):
    set_knobs(monkeypatch, None, ROWS)
    with CombContext(layout, dtype) as c:
        got = c.combine(kind, param)
        assert np.array_equal(got.astype(np.float64), c.reference(name, param), equal_nan=True)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("layout", list(COMB_LAYOUTS))
def test_combine_all_device(layout, dtype, monkeypatch):
    set_knobs(monkeypatch, None, ROWS)
    with CombContext(layout, dtype) as c:
        outs = (c.ens.empty(), c.ens.empty(), c.ens.empty())
        c.ens._after_torch()
        mms = c.e.combine_all(0.3, 0.37, 0.5, c.u_t.data_ptr(), c.i_t.data_ptr(), tuple(t.data_ptr() for t in outs),
                              seed=SEED, pair_base=c.base, n_pairs=c.n_pairs)
        for (name, kind, param), t, mm in zip(COMB_CASES, outs, mms):
            got = t.cpu().numpy()
            assert np.array_equal(got, c.combine(kind, param), equal_nan=True), name
            assert np.array_equal(got.astype(np.float64), c.reference(name, param), equal_nan=True), name
            assert mm == (float(np.nanmin(got)), float(np.nanmax(got))), name  # the carried min / max rows


# ---- 5. mr_topk_dense_device ----------------------------------------------------------
@pytest.mark.parametrize("k", [1, 16])
def test_dense_topk(k, monkeypatch):
    set_knobs(monkeypatch, None, ROWS)
    ds = dataset()
    with Engine(ds, out_dtype="f64", topk=k) as e:
        ens = DeviceEnsemble(e)
        u_t, i_t = ens.model("ubm"), ens.model("ibm")
        c = ens.linear(u_t, i_t, 0.5)
        songs, scores, keys = ens.topk(c)
        x = c.cpu().numpy()
        cols = np.arange(x.shape[1])
        for u in range(ds.n_test):  # every user, not only the first launch's
            valid = cols[~np.isnan(x[u])]
            order = valid[np.lexsort((valid, -x[u, valid]))][:k]  # score descending, song ascending
            assert songs[u].tolist() == order.tolist(), u
            assert np.array_equal(scores[u], x[u, order]), u
            assert np.array_equal(keys[u].view(np.float64), x[u, order]), u
        # the only negative score sits in a row of the third launch
        bad = u_t.clone()
        row = 20
        assert 2 * ROWS <= row < 3 * ROWS
        col = int(np.flatnonzero(~np.isnan(x[row]))[3])
        bad[row, col] = -1.0
        torch.cuda.synchronize()
        with pytest.raises(_lib.EngineError) as ei:
            ens.topk(bad)
        assert ei.value.code == _lib.MR_E_INVALID
        with pytest.raises(_lib.EngineError) as ei:
            e.topk()
        assert ei.value.code == _lib.MR_E_STATE
        s2, _sc2, k2 = ens.topk(c)  # the flag is cleared by the next call
        assert np.array_equal(s2, songs) and np.array_equal(k2, keys)


# ---- 6. device merges --------------------------------------------------------------------
def test_device_merges_of_song_shards(monkeypatch):
    set_knobs(monkeypatch, None, ROWS)
    ds = dataset()
    k, n_shards = 10, 3
    ss, kk = [], []
    for lo, hi in song_shards(ds, n_shards):
        with Engine(ds, topk=k, dense=False, song_lo=lo, song_hi=hi) as e:
            e.run("ibm")
            assert_lists(e, "ibm", k)
            s, _sc, keys = e.topk()
        ss.append(s)
        kk.append(keys)
    ss, kk = np.stack(ss), np.stack(kk)
    hs, hsc, hk = merge_topk_host(ss, kk)
    _, ts, tk = oracle("ibm", 0, 0, k)
    assert np.array_equal(hs, ts) and np.array_equal(hk, tk)

    def outputs():
        return (torch.empty((N_TEST, k), dtype=torch.int32, device="cuda"),
                torch.empty((N_TEST, k), dtype=torch.int64, device="cuda"),
                torch.empty((N_TEST, k), dtype=torch.float64, device="cuda"))

    def check(o_s, o_k, o_sc):
        assert np.array_equal(o_s.cpu().numpy(), ts) and np.array_equal(o_k.cpu().numpy(), tk)
        assert np.array_equal(o_sc.cpu().numpy(), hsc, equal_nan=True)

    with Engine(ds, topk=k, dense=False) as e:
        g_s, g_k = torch.tensor(ss, device="cuda"), torch.tensor(kk, device="cuda")
        o_s, o_k, o_sc = outputs()
        torch.cuda.synchronize()
        e.merge_topk_device(n_shards, g_s.data_ptr(), g_k.data_ptr(), o_s.data_ptr(), o_k.data_ptr(), o_sc.data_ptr())
        check(o_s, o_k, o_sc)
        # record blocks: keys at byte 0, songs at byte 8 * n_test * k, padded to the record size
        rec = e.record_bytes()
        n = N_TEST * k
        assert rec >= 12 * n
        blocks = np.zeros((n_shards, rec), dtype=np.uint8)
        for g in range(n_shards):
            blocks[g, :8 * n] = kk[g].reshape(-1).view(np.uint8)
            blocks[g, 8 * n:12 * n] = ss[g].reshape(-1).view(np.uint8)
        records = torch.tensor(blocks, device="cuda")
        o_s, o_k, o_sc = outputs()
        torch.cuda.synchronize()
        e.merge_topk_records(n_shards, records.data_ptr(), rec, o_s.data_ptr(), o_k.data_ptr(), o_sc.data_ptr())
        e.sync()
        check(o_s, o_k, o_sc)


def test_group_exchange(monkeypatch):
    """2 song shards x 2 user blocks on one device (device-copy transport):
    every context runs in batches and split launches, the exchange's merge in
    split launches too."""
    set_knobs(monkeypatch, BATCH, ROWS)
    ds = dataset()
    with Group(ds, song_shards=2, user_blocks=2, out_dtype="f64", topk=10, stage1="wide") as g:
        assert g.transport == "copy" and len(g.layout) == 4
        assert all(uhi - ulo > BATCH for _slo, _shi, ulo, uhi, _d in g.layout)
        for model in MODELS:
            g.run(model)
            songs, scores, keys = g.topk()
            exp, ts, tk = oracle(model, 0, 0, 10)
            assert np.array_equal(songs, ts) and np.array_equal(keys, tk), model
            valid = keys >= 0
            assert np.array_equal(scores[valid], keys[valid].view(np.float64))
            assert np.array_equal(g.dense(), exp, equal_nan=True), model


# ---- 7. mr_ibm_asym_device -------------------------------------------------------------------
N_ASYM = 21


def asym_twin(alpha, q):
    if (alpha, q) not in _twin:
        t = evaluation.asym_item_model(dataset(N_ASYM), alpha, q)
        t.setflags(write=False)
        _twin[(alpha, q)] = t
    return _twin[(alpha, q)]


def assert_model_bits(t, exp, dtype):
    got = t.cpu().numpy()
    if dtype == "f32":
        exp, view = exp.astype(np.float32), np.int32  # rounded once
    else:
        view = np.int64
    assert got.dtype == exp.dtype and got.shape == exp.shape
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert np.array_equal(got[ok].view(view), exp[ok].view(view))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("alpha,q", [(0.5, 1), (0.15, 3)])
def test_asymmetric_item_model(alpha, q, dtype, monkeypatch):
    set_knobs(monkeypatch, None, ROWS)
    monkeypatch.delenv("MR_ASYM_SUB", raising=False)
    ds = dataset(N_ASYM)
    exp = asym_twin(alpha, q)
    with Engine(ds, out_dtype=dtype) as e:
        assert_model_bits(DeviceEnsemble(e).item_based(alpha, q), exp, dtype)
    lo, hi = 3000, 9000
    with Engine(ds, out_dtype=dtype, song_lo=lo, song_hi=hi) as e:
        assert e.block_songs > 256
        assert_model_bits(DeviceEnsemble(e).item_based(alpha, q), exp[:, lo:hi], dtype)
        monkeypatch.setenv("MR_ASYM_SUB", "256")  # several sub-ranges per tile
        assert_model_bits(DeviceEnsemble(e).item_based(alpha, q), exp[:, lo:hi], dtype)


# ---- 8. mr_similar_songs_device ----------------------------------------------------------------
def test_similar_songs(monkeypatch):
    """per = 8 queries per launch: the loop the scratch bound drives in production."""
    set_knobs(monkeypatch, None, ROWS)
    monkeypatch.delenv("MR_SIMILAR_COUNTERS", raising=False)
    ds = dataset()
    lo, hi = 3000, 9000
    c_tr = np.bincount(ds.tr_songs, minlength=ds.n_songs)
    no_listener = np.flatnonzero(c_tr[lo:hi] == 0)[:1] + lo
    assert no_listener.size == 1
    popular = np.argsort(-c_tr, kind="stable")
    inside = popular[(popular >= lo) & (popular < hi)][:12]
    outside = popular[(popular < lo) | (popular >= hi)][:5]
    q = np.concatenate([inside[:6], outside[:3], no_listener, inside[6:], outside[3:], inside[:3]]).astype(np.int32)
    assert q.size == 21 and np.unique(q).size < q.size
    K = 5
    for shard in ((lo, hi), (0, 0)):
        with Engine(ds, song_lo=shard[0], song_hi=shard[1]) as e:
            ens = DeviceEnsemble(e)
            exp = evaluation.song_similarity(ds, q, e.song_lo, e.song_hi)
            assert np.count_nonzero(np.nan_to_num(exp[2 * ROWS:])) > 0  # the last launch has something to get wrong

            def assert_rows(rows):
                got = rows.cpu().numpy()
                assert got.dtype == np.float64 and got.shape == exp.shape
                assert np.array_equal(np.isnan(got), np.isnan(exp))
                ok = ~np.isnan(exp)
                assert np.array_equal(got[ok].view(np.int64), exp[ok].view(np.int64))

            def assert_similar_lists(songs, scores):
                songs, scores = songs.cpu().numpy(), scores.cpu().numpy()
                exp_songs, exp_scores = evaluation.similar_lists(exp, K, song_lo=e.song_lo)
                assert songs.dtype == np.int32 and scores.dtype == np.float64
                assert np.array_equal(songs, exp_songs)
                assert np.array_equal(np.isnan(scores), exp_songs < 0)
                ok = exp_songs >= 0
                assert np.array_equal(scores[ok].view(np.int64), exp_scores[ok].view(np.int64))
                return exp_songs

            songs, scores, rows = ens.similar_songs(q, K, dense=True)
            assert_rows(rows)
            listed = assert_similar_lists(songs, scores)
            assert (listed[q == no_listener[0]] == -1).all()
            assert_rows(ens.similar_songs(q, 0, dense=True)[2])  # K = 0: rows only
            assert_similar_lists(*ens.similar_songs(q, K))       # lists only: no dense_dev


# ---- 9. knob hygiene ------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,rows", [("0", "0"), ("-3", "-3"), ("abc", "abc"), (None, "7")])
def test_invalid_knob_values_are_ignored(batch, rows, monkeypatch):
    set_knobs(monkeypatch, batch, rows)
    for model, route in (("ubm", "auto"), ("ibm", "two_hop"), ("ibm", "cooc")):
        with Engine(dataset(), out_dtype="f64", topk=10, stage1="wide", ibm_route=route) as e:
            assert e.batch == N_TEST
            e.run(model)
            e.sync()
            e.timing_begin()
            e.run(model)
            e.run(model)
            assert e.timing_end()[0] == 2
            assert_dense(e, model, 10)
            assert_lists(e, model, 10)
