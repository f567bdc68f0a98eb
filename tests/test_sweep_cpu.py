"""Parameter sweep, the parts that need no device: the C ABI rejects null
arguments, the driver's --sweep specs parse (or are refused), the grid is
evenly spaced, best() picks the first maximum."""
import pytest

from musicrecommendation_amd import _lib, driver
from musicrecommendation_amd.ensemble import best, sweep_kind


def test_sweep_null_arguments_are_rejected():
    L = _lib.lib()
    assert L.mr_sweep_minmax_device(None, 0, 1, None, 0, 0, 0, None, None, None, None) == _lib.MR_E_INVALID
    assert L.mr_sweep_class_counts_device(None, 0, 1, None, 0, 0, 0, None, None, None, None, None, None, 0, None,
                                          None, 10) == _lib.MR_E_INVALID
    assert L.mr_sweep_map_device(None, 0, 1, None, 0, 0, 0, None, None, None, None, None, 0, None, None,
                                 10) == _lib.MR_E_INVALID
    assert _lib.MR_SWEEP_MAX_PARAMS == 64


def test_sweep_spec_parsing():
    assert driver.parse_sweep("linear:0:1:5") == ("linear", 0.0, 1.0, 5)
    assert driver.parse_sweep("stochastic:0.25:0.75:3") == ("stochastic", 0.25, 0.75, 3)
    assert driver.parse_sweep("aggregation:0.5:0.5:1") == ("aggregation", 0.5, 0.5, 1)
    for bad in ("cubic:0:1:5", "linear:0:1:0", "linear:0:1:-2", "linear:a:1:5", "linear:0:b:5", "linear:0:1:2.5",
                "linear:0:1", "linear"):
        with pytest.raises(ValueError):
            driver.parse_sweep(bad)
    with pytest.raises(SystemExit):  # argparse refuses the option before anything runs
        driver.main(["8", "8", "--sweep", "cubic:0:1:5"])


def test_sweep_grid():
    assert driver.sweep_grid(0.0, 1.0, 5) == [0.0, 0.25, 0.5, 0.75, 1.0]
    assert driver.sweep_grid(0.0, 1.0, 11)[0] == 0.0 and driver.sweep_grid(0.0, 1.0, 11)[-1] == 1.0
    assert driver.sweep_grid(0.3, 0.9, 1) == [0.3]
    assert driver.sweep_grid(1.0, 0.0, 3) == [1.0, 0.5, 0.0]


def test_best_picks_the_first_maximum():
    assert best([0.1, 0.2, 0.3, 0.4], [0.5, 0.9, 0.9, 0.1]) == 0.2
    assert best([0.7], [0.0]) == 0.7
    assert best([0.0, 1.0], [float("nan"), 0.25]) == 1.0
    with pytest.raises(ValueError):
        best([], [])
    with pytest.raises(ValueError):
        best([0.1, 0.2], [0.3])


def test_sweep_kind_names():
    assert [sweep_kind(k) for k in ("linear", "aggregation", "stochastic")] == [
        _lib.MR_COMB_LINEAR, _lib.MR_COMB_AGGREGATION, _lib.MR_COMB_STOCHASTIC]
    assert sweep_kind(2) == 2
    with pytest.raises(ValueError):
        sweep_kind("cubic")
