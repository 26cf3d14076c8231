"""The host side of grt_pipeline_run_sky_channels, without a device: grt_channel_pair_count against channel_model.py's
pair_count at the edges of the 128-point blocks, -1 for every kind of channel list the entry point refuses, and
channel_model.py's own restatement against what pins it down -- the whole-grid channel with the trapezoid's weights is the
oracle's integral, the brightness temperature inverts planck() -- and grtcode_amd.channels' two builders."""
import ctypes as C

import numpy as np
import pytest

from channel_model import (centroid, channel_brightness, channel_mean, magnitude, pair_count, sign_ratio, weight_sum)
from grtcode_amd import api, channels
from lw_jacobian_model import planck
from pipeline_support import TRAP_ULPS


def count(first, weights, n, center=None):
    g, keep = api.make_channels(first, weights, center)
    return api.channel_pair_count(g, n), keep


def ones(*counts):
    return [np.ones(k) for k in counts]


# ---- grt_channel_pair_count ---------------------------------------------------------------------------------------------- #
N = 257
CASES = {
    "one point at 0 and one at n - 1": ([0, N - 1], ones(1, 1), N),
    "the whole grid": ([0], ones(N), N),
    "wave and block edges": ([60, 120, 127], ones(8, 16, 2), N),
    "duplicates": ([120, 120, 120], ones(16, 16, 16), N),
    "descending order": ([255, 127, 120, 60, 0], ones(2, 2, 16, 8, 1), N),
    "n = 2": ([0, 1, 0], ones(1, 1, 2), 2),
    "a long grid": ([0, 3_249_000, 127], ones(3_250_000, 1000, 130), 3_250_000),
}


@pytest.mark.parametrize("name", list(CASES))
def test_pair_count_equals_the_model(name):
    first, weights, n = CASES[name]
    got, keep = count(first, weights, n)
    want = pair_count(first, keep["counts"], n)
    print(name, got, want)
    assert got == want and got >= len(first)


def test_pair_count_by_hand():
    assert count([60, 120, 127], ones(8, 16, 2), N)[0] == 1 + 2 + 2
    assert count([0], ones(N), N)[0] == 3
    assert count([0], ones(128), 128)[0] == 1 and count([0], ones(129), 129)[0] == 2


def raw(first, offset, weights, center=None, C_=None):
    """A GrtChannels of these arrays as they are (None: a NULL pointer)."""
    arr = [None if first is None else np.ascontiguousarray(first, dtype=np.int32),
           None if offset is None else np.ascontiguousarray(offset, dtype=np.int32),
           None if weights is None else np.ascontiguousarray(weights, dtype=np.float64),
           None if center is None else np.ascontiguousarray(center, dtype=np.float64)]
    ip = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    g = api.GrtChannels(len(first) if C_ is None else C_, ip(arr[0]), ip(arr[1]), dp(arr[2]), dp(arr[3]), None, None)
    g.keep = arr
    return g


GOOD = dict(first=[0, 5], offset=[0, 3, 5], weights=[1.0, 2.0, 1.0, -0.25, 1.0], center=[700.0, 900.0])
REFUSED = {
    "first NULL": dict(first=None, C_=2),
    "offset NULL": dict(offset=None),
    "weights NULL": dict(weights=None),
    "no channels": dict(C_=0),
    "a negative count": dict(C_=-1),
    "too many channels": dict(C_=api.GRT_MAX_CHANNELS + 1),
    "offset[0] not 0": dict(offset=[1, 3, 5]),
    "offset not increasing": dict(offset=[0, 3, 3]),
    "offset decreasing": dict(offset=[0, 3, 2]),
    "first below 0": dict(first=[-1, 5]),
    "a channel past the grid": dict(first=[0, 11]),
    "a NaN weight": dict(weights=[1.0, float("nan"), 1.0, -0.25, 1.0]),
    "an infinite weight": dict(weights=[1.0, 2.0, 1.0, -0.25, float("inf")]),
    "a sum of 0": dict(weights=[1.0, -2.0, 1.0, -0.25, 1.0]),
    "a sum below 0": dict(weights=[1.0, 2.0, 1.0, -1.25, 1.0]),
    "a sum that overflows": dict(weights=[1e308, 1e308, 1.0, -0.25, 1.0]),
    "a NaN center": dict(center=[700.0, float("nan")]),
    "an infinite center": dict(center=[float("inf"), 900.0]),
    "a center of 0": dict(center=[0.0, 900.0]),
    "a center below 0": dict(center=[700.0, -900.0]),
}


def test_the_good_channels_count(lib):
    assert lib.grt_channel_pair_count(C.byref(raw(**GOOD)), 12) == 2
    assert lib.grt_channel_pair_count(C.byref(raw(**dict(GOOD, center=None))), 12) == 2
    assert lib.grt_channel_pair_count(C.byref(raw(**GOOD)), 10) == 2                     # (5 + 2 points end at n - 1 = 6 < 10)
    assert lib.grt_channel_pair_count(C.byref(raw(**GOOD)), 7) == 2


@pytest.mark.parametrize("name", list(REFUSED))
def test_pair_count_refuses(lib, name):
    assert lib.grt_channel_pair_count(C.byref(raw(**dict(GOOD, **REFUSED[name]))), 12) == -1


def test_pair_count_refuses_null_and_no_grid(lib):
    assert lib.grt_channel_pair_count(None, 12) == -1
    assert lib.grt_channel_pair_count(C.byref(raw(**GOOD)), 0) == -1
    assert lib.grt_channel_pair_count(C.byref(raw(**GOOD)), 6) == -1                     # (the second channel ends at point 6)


# ---- the restatement ------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("n,seed", [(2, 1), (65, 2), (257, 3), (3250, 4)])
def test_whole_grid_trapezoid_channel_is_the_oracles_integral(oracle, n, seed):
    dw = 0.37
    row = np.random.default_rng(seed).uniform(0.1, 2.0, n)
    w = np.full(n, dw)
    w[0] = w[-1] = 0.5 * dw
    mean = channel_mean(row, [0], [w])[0]
    mag = magnitude(row, [0], [w])[0]
    want = oracle.integrate_row(row, dw)
    err = abs(mean * weight_sum(w) - want)
    print(n, err, TRAP_ULPS * 2.0 ** -52 * mag * weight_sum(w))
    # (magnitude is per unit of sum W: the product carries it back)
    assert err <= TRAP_ULPS * 2.0 ** -52 * mag * weight_sum(w)
    assert sign_ratio([w])[0] == pytest.approx(1.0, abs=1e-12)


def test_brightness_inverts_planck():
    v = np.array([650.0, 900.0, 1200.0, 2400.0])
    for T in np.linspace(180.0, 320.0, 29):
        got = channel_brightness(planck(T, v), v)
        assert np.abs(got - T).max() <= 1e-10, (T, got)
    out = channel_brightness(np.array([0.0, -1.0, -0.0]), v[:3])
    assert np.all(out == 0.0) and not np.any(np.signbit(out))


def test_channel_mean_by_hand():
    rows = np.arange(20.0).reshape(2, 10)
    got = channel_mean(rows, [2, 0], [[1.0, 3.0], [2.0]])
    assert np.array_equal(got, [[(2.0 + 9.0) / 4.0, 0.0], [(12.0 + 39.0) / 4.0, 10.0]])
    assert np.array_equal(centroid([2, 0], [[1.0, 3.0], [2.0]], 100.0, 0.5), [(101.0 + 3 * 101.5) / 4.0, 100.0])
    assert sign_ratio([[2.0, -0.5]])[0] == 2.5 / 1.5


# ---- grtcode_amd.channels ------------------------------------------------------------------------------------------------------ #
def test_gaussian_is_symmetric_and_clipped():
    w0, dw, n = 100.0, 0.5, 401                                            # 100 .. 300 cm-1
    first, weights, centers = channels.gaussian(w0, dw, n, [200.0, 101.0, 299.5, 92.0], 2.0)
    assert np.array_equal(centers, [200.0, 101.0, 299.5, 92.0]) and first.dtype == np.int32
    # on-grid centre, inside: +-8 cm-1 = 16 points either side, symmetric, 1 at the centre
    assert first[0] == 200 - 16 and weights[0].size == 33
    assert np.array_equal(weights[0], weights[0][::-1]) and weights[0][16] == 1.0
    assert weights[0][14] == pytest.approx(0.5, rel=1e-14)                # (half the maximum at half the width)
    # clipped at the lower end, at the upper end, and a centre off the grid whose wing is on it
    assert first[1] == 0 and weights[1].size == 2 + 16 + 1 and weights[1][2] == 1.0
    assert first[2] + weights[2].size == n and weights[2][-2] == 1.0
    assert first[3] == 0 and weights[3].size == 1
    g, keep = api.make_channels(first, weights, centers)
    assert api.channel_pair_count(g, n) == pair_count(first, keep["counts"], n)
    with pytest.raises(ValueError):
        channels.gaussian(w0, dw, n, [200.0, 320.0], 2.0)
    with pytest.raises(ValueError):
        channels.gaussian(w0, dw, n, [80.0], 2.0)


def test_boxcar_is_clipped():
    w0, dw, n = 100.0, 1.0, 201                                            # 100 .. 300 cm-1
    first, weights, centers = channels.boxcar(w0, dw, n, [150.0, 50.0, 290.0, 120.25], [199.0, 110.0, 400.0, 120.75 + 1.0])
    assert np.array_equal(first, [50, 0, 190, 21])
    assert [w.size for w in weights] == [50, 11, 11, 1] and all(np.all(w == 1.0) for w in weights)
    assert np.array_equal(centers, [174.5, 80.0, 345.0, 121.0])
    with pytest.raises(ValueError):
        channels.boxcar(w0, dw, n, [301.0], [350.0])
    with pytest.raises(ValueError):
        channels.boxcar(w0, dw, n, [120.25], [120.75])
