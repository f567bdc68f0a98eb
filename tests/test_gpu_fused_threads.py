"""GPU: the fused scoring kernel at 256, 512 and 1024 threads, general and lean.

mr_load reads MR_FUSED_NT (threads per fused workgroup) and MR_FUSED_LEAN (the
lean instantiation where its launch-time conditions hold). Integer LDS adds, a
total order of the candidates and unchanged per-song fp64 operations make the
result independent of both, so every case here is compared bitwise — dense
scores, top-k songs and keys, both models — with oracle.native.fp_model, and
every case asserts the geometry the engine reports (Engine.fused_threads /
fused_lean) against lean_expected(), the test's own statement of the lean
kernel's conditions.

Shapes: the smallest that exercise the thread-count plumbing (a tile narrower
than the workgroup, a partial last tile that is no multiple of 64, fewer train
users than threads, a test user without any schedule entry, one with several
schedule batches and more visible songs than threads), k on both sides of the
threshold path's limits, n_tiles x k on both sides of NT (register-resident
against staged merge), and rank_survivors' regimes at each NT's row geometry,
asserted from the oracle's output as tests/test_gpu_topk_adversarial.py does.
"""
import functools

import numpy as np
import pytest

import topk_cases as tc
from helpers import dataset_from_lines
from musicrecommendation_amd import synth
from musicrecommendation_amd.engine import Engine
from oracle import native

pytestmark = pytest.mark.gpu
MODELS = ("ibm", "ubm")
NTS = (256, 512, 1024)
VARIANTS = [(nt, lean) for nt in NTS for lean in (0, 1)]
VARIANT_IDS = [f"nt{nt}-lean{lean}" for nt, lean in VARIANTS]
TILE_ROWS = 32  # MR_TILE_ROWS: threshold rows of the fused tile top-k


def lean_expected(nt, lean, k, block_songs, n_tiles, sched=True, lists=False):
    """The launch-time conditions of the lean kernel (lean_ok in csrc/mr_engine.hip)."""
    return bool(lean and sched and not lists and 1 <= k <= min(TILE_ROWS, nt // 16) and n_tiles * k <= nt
                and block_songs <= 1024)


def shape_of(nt):
    """The fused tile top-k at NT threads: 32 rows of NT / 32 threads, cap 256,
    one wave past nc^2 > 16384 at every NT."""
    return tc.Shape(nt, TILE_ROWS, 16384 // nt, None)


@functools.lru_cache(maxsize=None)
def oracle_of(key, model, k):
    out = native.fp_model(DATASETS[key](), model, k=k)
    for a in out:
        a.setflags(write=False)
    return out


def run_exact(key, model, k, nt, lean, monkeypatch, *, sched=True, expect_lean=None, **kw):
    ds = DATASETS[key]()
    monkeypatch.setenv("MR_FUSED_NT", str(nt))
    monkeypatch.setenv("MR_FUSED_LEAN", str(lean))
    monkeypatch.setenv("MR_FUSED_SCHED", "1" if sched else "0")
    exp, ts, tk = oracle_of(key, model, k)
    with Engine(ds, out_dtype="f64", topk=k, stage1="fused", **kw) as e:
        assert e.shape == "fused" and e.fused_threads == nt
        want = lean_expected(nt, lean, k, e.block_songs, e.n_tiles, sched, kw.get("topk_lists", False))
        assert e.fused_lean == want, (e.fused_lean, want, e.block_songs, e.n_tiles)
        if expect_lean is not None:
            assert want == bool(expect_lean and lean)
        got = e.score_dense(model)
        songs, scores, keys = e.topk()
        geometry = (e.block_songs, e.n_tiles)
    assert np.array_equal(got, exp, equal_nan=True), "dense scores differ from the fixed-point oracle"
    assert np.array_equal(songs, ts), "top-k songs differ from the fixed-point oracle"
    assert np.array_equal(keys, tk), "top-k keys differ from the fixed-point oracle"
    valid = keys >= 0
    assert np.array_equal(scores[valid], keys[valid].view(np.float64)) and np.isnan(scores[~valid]).all()
    return geometry


# ---- datasets ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plumbing_dataset():
    """300 train users over 1,000 songs (tiles of 256: a partial last tile of
    232 songs; tiles of 768: one of 232 too, and a tile narrower than 1024
    threads); test users: random ones, one whose songs no train user heard (no
    schedule entry), one who heard a third of the catalogue."""
    rng = np.random.default_rng(11)
    rows = [set(rng.choice(1000, int(rng.integers(3, 40)), replace=False).tolist()) for _ in range(300)]
    rows[0] |= set(range(1000)) - set().union(*rows)  # every song has a listener
    train = [f"t{v:03d}\ts{s:04d}\t1" for v, row in enumerate(rows) for s in sorted(row)]
    test = []
    for u in range(5):
        test += [f"u{u}\ts{int(s):04d}\t1" for s in rng.choice(1000, 12 + 7 * u, replace=False)]
    test += [f"cold\tx{j}\t1" for j in range(4)]
    test += [f"big\ts{int(s):04d}\t1" for s in rng.choice(1000, 330, replace=False)]
    ds = dataset_from_lines(train, test, ["u0\ts0001\t1"])
    assert ds.n_train == 300 and ds.n_songs == 1004
    return ds


@functools.lru_cache(maxsize=None)
def batches_dataset():
    """The generator of test_fused_walk_schedule_batches with a heavier first
    user: H has 1,100 visible songs (more than 1024 threads: the heard-song
    tail loop at every NT) and 600 x 40 = 24,000 (song, listener) entries, a
    dozen batches of the 2,048 one batch covers; E has no entry at all."""
    rng = np.random.default_rng(7)
    train = []
    for v in range(700):
        songs = set(range(40)) if v < 600 else set()
        songs |= set(rng.choice(np.arange(40, 2000), size=20, replace=False).tolist())
        train += [f"t{v:04d}\ts{s:04d}\t1" for s in sorted(songs)]
    test = [f"H\ts{s:04d}\t1" for s in range(1100)]
    test += [f"E\tx{j}\t1" for j in range(5)]
    test += [f"N\ts{int(s):04d}\t1" for s in rng.choice(2000, 30, replace=False)]
    return dataset_from_lines(train, test, ["H\ts1500\t1", "E\ts0001\t1", "N\ts0002\t1"])


@functools.lru_cache(maxsize=None)
def tiles_dataset(n_tiles):
    """n_tiles tiles of 256 songs (the last one partial), 120 train users."""
    rng = np.random.default_rng(100 + n_tiles)
    n_songs = (n_tiles - 1) * 256 + 77
    rows = [set(rng.choice(n_songs, 60, replace=False).tolist()) for _ in range(120)]
    rows[0] |= set(range(n_songs)) - set().union(*rows)  # every song has a listener
    train = [f"t{v:03d}\ts{s:05d}\t1" for v, row in enumerate(rows) for s in sorted(row)]
    test = []
    for u in range(3):
        test += [f"u{u}\ts{int(s):05d}\t1" for s in rng.choice(n_songs, 25, replace=False)]
    ds = dataset_from_lines(train, test, ["u0\ts00001\t1"])
    assert ds.n_songs == n_songs
    return ds


class Regime(tuple):
    """(nt, k, block, n_tiles, tile, m, tied, regime) of one packed_rows case."""


def packed(nt, k, block, n_tiles, tile, m, tied, regime):
    return Regime((nt, k, block, n_tiles, tile, m, tied, regime))


# Per NT (rows of NT / 32 threads): the parallel ranking's last size and the
# one-wave select's first (128 / 129), the cap (256) and the first overflow
# (257, into block_topk on a 1024-song tile), and an overflow on an 8192-song
# tile (into block_topk_wide, whose 256 lists do not grow with NT).
REGIMES = [c for nt in NTS for c in (
    packed(nt, 10, 768, 3, 1, 127, False, "parallel"),
    packed(nt, 10, 768, 3, 1, 128, False, "one_wave"),
    packed(nt, 10, 768, 3, 1, 128, True, "one_wave"),
    packed(nt, 16, 1024, 3, 1, 255, False, "one_wave"),
    packed(nt, 16, 1024, 3, 1, 256, False, "overflow"),
    packed(nt, 16, 1024, 3, 1, 300, True, "overflow"),
    packed(nt, 10, 8192, 2, 0, 300, False, "overflow"),
)]


@functools.lru_cache(maxsize=None)
def regime_case(c):
    nt, k, block, n_tiles, tile, m, tied, _ = c
    case = tc.packed_rows(nt, TILE_ROWS, tile, k, m, block=block, n_tiles=n_tiles, tied=tied)
    return case, dataset_from_lines(*case.lines)


@functools.lru_cache(maxsize=None)
def flood_dataset(m):
    return dataset_from_lines(*tc.tie_flood(m).lines)


@functools.lru_cache(maxsize=None)
def boundary_dataset(n_tiles):
    return dataset_from_lines(*tc.boundary_ties(256, n_tiles).lines)


DATASETS = {"plumbing": plumbing_dataset, "batches": batches_dataset, "c2_40": lambda: c2_40()}
for _n in (9, 25, 26, 51, 52, 102, 103):
    DATASETS[f"tiles{_n}"] = functools.partial(tiles_dataset, _n)
for _c in REGIMES:
    DATASETS[_c] = functools.partial(lambda c: regime_case(c)[1], _c)
for _m in (140, 300):
    DATASETS[f"flood{_m}"] = functools.partial(flood_dataset, _m)
for _n in (3, 17):
    DATASETS[f"boundary{_n}"] = functools.partial(boundary_dataset, _n)


@functools.lru_cache(maxsize=None)
def c2_40():
    return synth.config("c2", n_test=40).dataset()


# ---- the thread-count plumbing ---------------------------------------------------------
@pytest.mark.parametrize("block", [256, 768, 1024])
@pytest.mark.parametrize("sched", [True, False])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("nt,lean", VARIANTS, ids=VARIANT_IDS)
def test_small_shapes(nt, lean, model, sched, block, monkeypatch):
    """300 train users (fewer than 512 / 1024 threads), tiles of 256 and 768
    songs over 1,004 songs, and one tile of 1024 (the tile publishes the
    user's list itself); MR_FUSED_SCHED=0 runs the segment search of the
    general kernel whatever MR_FUSED_LEAN asks."""
    bs, n_tiles = run_exact("plumbing", model, 10, nt, lean, monkeypatch, sched=sched, block_songs=block,
                            expect_lean=sched)
    assert (bs, n_tiles) == (block, -(-1004 // block))


@pytest.mark.parametrize("sched", [True, False])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("nt,lean", VARIANTS, ids=VARIANT_IDS)
def test_schedule_batches_and_heard_tail(nt, lean, model, sched, monkeypatch):
    """More schedule entries than one batch of kSE x NT = 2,048, more visible
    songs than threads, and a user with no entry; k = 1 and 10."""
    for k in (1, 10):
        run_exact("batches", model, k, nt, lean, monkeypatch, sched=sched)


@pytest.mark.parametrize("k", [1, 10, 16, 32, 33, 64])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("nt,lean", VARIANTS, ids=VARIANT_IDS)
def test_topk_sizes(nt, lean, model, k, monkeypatch):
    """k up to the threshold path's limit (NT / 16 and 32 rows) and past it (33,
    64: block_topk in the general kernel at every NT)."""
    run_exact("plumbing", model, k, nt, lean, monkeypatch, block_songs=256)


@pytest.mark.parametrize("n_tiles", [25, 26, 51, 52, 102, 103])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("nt,lean", VARIANTS, ids=VARIANT_IDS)
def test_merge_both_sides_of_nt(nt, lean, model, n_tiles, monkeypatch):
    """k = 10 candidates per tile: 25 / 26, 51 / 52 and 102 / 103 tiles put
    n_tiles x k on both sides of 256, 512 and 1024 — one candidate per thread in
    registers, or the lists staged in LDS (the general kernel)."""
    bs, nt_got = run_exact(f"tiles{n_tiles}", model, 10, nt, lean, monkeypatch, block_songs=256,
                           expect_lean=n_tiles * 10 <= nt)
    assert (bs, nt_got) == (256, n_tiles)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("nt,lean", VARIANTS, ids=VARIANT_IDS)
def test_register_merge_overflows_into_staged_merge(nt, lean, model, monkeypatch):
    """9 tiles x k = 32 = 288 candidates, all valid (asserted from the oracle's
    dense row). At NT = 512 / 1024 they fit one per thread, but occupy only 18 /
    9 of the merge's 32 threshold rows: fewer than k rows hold an entry, tau is
    "every valid key", and 288 survivors overflow the 256 slots — the only way
    the register-resident merge (and with it the lean kernel) reaches the
    staged merge. At NT = 256 the 288 candidates go to the staged merge at once."""
    k, n_tiles = 32, 9
    ds = tiles_dataset(n_tiles)
    exp = oracle_of("tiles9", model, k)
    for u in range(ds.n_test):
        keys = tc.keys_of(exp[0][u])
        assert all((keys[t * 256:(t + 1) * 256] >= 0).sum() >= k for t in range(n_tiles))
    if nt > 256:
        rows_used = -(-n_tiles * k // (nt // 32))
        assert n_tiles * k <= nt and rows_used < k and n_tiles * k > 256
    bs, got_tiles = run_exact("tiles9", model, k, nt, lean, monkeypatch, block_songs=256, expect_lean=nt > 256)
    assert (bs, got_tiles) == (256, n_tiles)


# ---- the selection regimes at each NT's geometry ------------------------------------------------
@pytest.mark.parametrize("lean", [0, 1])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("c", REGIMES, ids=lambda c: "nt{}-k{}-b{}-m{}{}-{}".format(c[0], c[1], c[2], c[5],
                                                                                 "t" if c[6] else "", c[7]))
def test_packed_rows_regimes(c, model, lean, monkeypatch):
    """rank_survivors' parallel ranking, the one-wave select and the overflow
    into block_topk / block_topk_wide, packed into NT / 32-thread rows of the
    middle tile; the regime is asserted from the oracle's keys."""
    nt, k, block, n_tiles, tile, m, tied, regime = c
    case, ds = regime_case(c)
    exp = oracle_of(c, model, k)
    got = tc.tile_regime(tc.keys_of(exp[0][0]), case.info["blo"], min(case.info["bhi"], ds.n_songs), shape_of(nt), k)
    assert got == (m + 1, regime)
    geometry = run_exact(c, model, k, nt, lean, monkeypatch, block_songs=block)
    assert geometry == (block, n_tiles)


@pytest.mark.parametrize("block", [1024, 8192])
@pytest.mark.parametrize("m", [140, 300])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("nt,lean", VARIANTS, ids=VARIANT_IDS)
def test_tie_flood(nt, lean, model, m, block, monkeypatch):
    """m songs of one positive score, 17 ids apart, k = 10. The exact keys'
    tau is a (key, song) pair, so every row best ties and the survivors are the
    flood's first songs by id: each tile ranks k (or, at 32-thread rows, up to
    2 k) of them in parallel — the tie is broken by song id in the threshold,
    the ranking and the merge. One tile of 8192 songs publishes the user's
    list itself (n_tiles = 1, the general kernel); tiles of 1024 hand over."""
    ds = flood_dataset(m)
    exp = oracle_of(f"flood{m}", model, 10)
    keys = tc.keys_of(exp[0][0])
    n_tiles = -(-ds.n_songs // block)
    for t in range(n_tiles):
        nc, regime = tc.tile_regime(keys, t * block, min((t + 1) * block, ds.n_songs), shape_of(nt), 10)
        assert regime == "parallel" and (nc >= 10 or t == n_tiles - 1)
    geometry = run_exact(f"flood{m}", model, 10, nt, lean, monkeypatch, block_songs=block, expect_lean=block == 1024)
    assert geometry == (block, n_tiles)


BOUNDARY_REGIMES = {(10, 512): {"parallel", "one_wave"}, (10, 1024): {"one_wave"}, (16, 512): {"one_wave"},
                    (16, 1024): {"one_wave"}}


@pytest.mark.parametrize("n_tiles,k", [(3, 1), (3, 4), (3, 10), (3, 16), (17, 16)])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("nt,lean", VARIANTS, ids=VARIANT_IDS)
def test_boundary_ties(nt, lean, model, n_tiles, k, monkeypatch):
    """Equal-score groups astride the boundaries of 256-song tiles, the k-th
    place inside a group; 17 tiles x 16 = 272 candidates leave the register
    merge at NT = 256 only. A tile of 256 songs fills half or a quarter of the
    rows of a wider workgroup, so fewer than k rows hold an entry there, tau is
    "every valid key" and the tile's 256 songs all survive: the one-wave
    select at its capacity (BOUNDARY_REGIMES, asserted from the oracle)."""
    key = f"boundary{n_tiles}"
    ds = boundary_dataset(n_tiles)
    exp = oracle_of(key, model, k)
    keys = tc.keys_of(exp[0][0])
    regimes = {tc.tile_regime(keys, t * 256, min((t + 1) * 256, ds.n_songs), shape_of(nt), k)[1]
               for t in range(n_tiles)}
    assert regimes == BOUNDARY_REGIMES.get((k, nt), {"parallel"})
    run_exact(key, model, k, nt, lean, monkeypatch, block_songs=256, expect_lean=n_tiles * k <= nt)


# ---- the hand-off counters under the default geometry -------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_counters_self_reset_default(model):
    """30 back-to-back runs, then one replay of a 50-step graph, at C2 with 40
    test users and whatever geometry mr_load picks by default: every launch
    leaves the per-user counters ready for the next."""
    ds = c2_40()
    exp, ts, tk = oracle_of("c2_40", model, 10)
    with Engine(ds, out_dtype="f64", topk=10, stage1="fused") as e:
        assert e.fused_threads in NTS
        assert e.fused_lean == lean_expected(e.fused_threads, e.fused_lean, 10, e.block_songs, e.n_tiles)
        for _ in range(30):
            e.run(model)
        assert np.array_equal(e.dense(), exp, equal_nan=True)
        songs, _, keys = e.topk()
        assert np.array_equal(songs, ts) and np.array_equal(keys, tk)
        e.graph_capture(model, 50)
        e.graph_launch()
        e.sync()
        assert np.array_equal(e.dense(), exp, equal_nan=True)
        songs, _, keys = e.topk()
        assert np.array_equal(songs, ts) and np.array_equal(keys, tk)
