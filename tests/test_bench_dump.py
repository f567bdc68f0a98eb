"""bench.py --dump-outputs: the writer of the last step's outputs (CPU only)."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_dtypes_and_exact_integers(tmp_path):
    rng = np.random.default_rng(3)
    dense = rng.standard_normal((4, 33)).astype(np.float32)
    dense[1, 5] = np.nan  # a heard song
    songs = rng.integers(0, 2 ** 31 - 1, size=(4, 10), dtype=np.int32)
    keys = rng.integers(-2 ** 62, 2 ** 62, size=(4, 10), dtype=np.int64)
    scores = rng.standard_normal((4, 10))
    bench.dump_outputs(str(tmp_path), {"dense": dense, "topk_songs": songs, "topk_scores": scores, "topk_keys": keys})
    got = {f[:-4]: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert set(got) == {"dense", "dense_nan", "topk_songs", "topk_scores", "topk_keys_hi", "topk_keys_lo"}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    # the heard-song NaN: 0 in the values, 1 in the mask; both together restore the model
    mask = got["dense_nan"]
    assert mask.dtype == np.float32 and mask.sum() == 1 and mask[1, 5] == 1 and got["dense"][1, 5] == 0
    assert got["dense"].dtype == np.float32
    assert np.array_equal(np.where(mask == 1, np.float32(np.nan), got["dense"]), dense, equal_nan=True)
    assert np.array_equal(got["topk_scores"], scores)
    assert np.array_equal(got["topk_songs"].astype(np.int32), songs)
    back = (got["topk_keys_hi"].astype(np.int64) << 32) | got["topk_keys_lo"].astype(np.int64)
    assert np.array_equal(back, keys)


def test_dump_outputs_samples_large_arrays_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 2 * 2 * 100)  # 100 elements for each of two arrays (and a mask each)
    big = np.arange(1000, dtype=np.float32).reshape(10, 100)
    small = np.arange(7, dtype=np.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": torch.from_numpy(big) if d == "b" else big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (100,) and np.array_equal(a, b)  # numpy array and torch tensor: the same positions
    assert np.all(np.diff(a) >= 0) and set(a.tolist()) <= set(big.ravel().tolist())
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 8 * 2 * 2 * 100 + 2 * 128  # the budget plus the two .npy headers
