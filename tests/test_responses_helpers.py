"""grtcode_amd/responses.py: the response functions api.make_responses takes, on published numbers (no GPU needed)."""
import numpy as np
import pytest

from grtcode_amd import responses as R


def test_erythemal_action_spectrum():
    lam = np.array([250.0, 298.0, 300.0, 328.0, 400.0, 401.0, 249.0])
    want = np.array([1.0, 1.0, 0.6486, 1.514e-3, 1.259e-4, 0.0, 0.0])
    got = R.erythemal_action(lam)
    assert got[0] == 1.0 and got[1] == 1.0 and got[5] == 0.0 and got[6] == 0.0
    assert np.all(np.abs(got[2:5] - want[2:5]) <= 1e-3 * want[2:5]), got
    # continuous where the three pieces meet
    assert abs(R.erythemal_action(np.array([298.0 + 1e-9]))[0] - 1.0) < 1e-8
    a, b = R.erythemal_action(np.array([328.0, 328.0 + 1e-9]))
    assert abs(a - b) <= 2e-3 * a


def test_erythemal_on_a_grid():
    # 24 000 .. 41 000 cm-1 in steps of 100: the response covers 25 000 (400 nm) .. 40 000 (250 nm)
    w0, dw, n = 24000.0, 100.0, 171
    first, weights = R.erythemal(w0, dw, n)
    assert list(first) == [10] and weights[0].size == 151
    lam = 1e7 / (w0 + (10 + np.arange(151)) * dw)
    assert np.allclose(weights[0], R.erythemal_action(lam), rtol=1e-12, atol=0.0)
    assert abs(weights[0][0] - 1.259e-4) <= 1e-3 * 1.259e-4 and weights[0][-1] == 1.0
    at_300 = weights[0][np.argmin(np.abs(lam - 300.0))]
    assert 0.6 < at_300 < 0.7
    with pytest.raises(ValueError):
        R.erythemal(1000.0, 10.0, 500)           # a grid that ends at 5 990 cm-1


def test_photon_weight():
    assert abs(R.photon_weight_at(1e7 / 500.0) - 4.1796) <= 1e-4 * 4.1796
    first, weights = R.photon_weight(10000.0, 100.0, 201)         # 10 000 .. 30 000 cm-1
    lo, hi = R.PAR_LIMITS
    assert first[0] == 43 and weights[0].size == 108              # 14 300 .. 25 000 cm-1
    assert weights[0][-1] == R.photon_weight_at(25000.0)
    assert np.all(np.diff(weights[0]) < 0.0)                      # fewer photons per joule towards the blue
    with pytest.raises(ValueError):
        R.photon_weight(30000.0, 100.0, 10)


def test_band():
    first, weights = R.band(100.0, 1.0, 400, 150.0, 160.0)
    assert list(first) == [50] and np.array_equal(weights[0], np.ones(11))
    first, weights = R.band(100.0, 1.0, 400, 50.0, 100.0)         # clipped to the grid's first point
    assert list(first) == [0] and weights[0].size == 1
    with pytest.raises(ValueError):
        R.band(100.0, 1.0, 400, 600.0, 700.0)


def test_tabulated_in_wavenumbers_clips_and_refuses():
    w0, dw, n = 1000.0, 10.0, 101                                 # 1 000 .. 2 000 cm-1
    first, weights = R.tabulated(w0, dw, n, [1205.0, 1300.0, 1400.0], [0.0, 1.0, 0.0])
    assert list(first) == [21] and weights[0].size == 20          # 1 210 .. 1 400 cm-1
    assert abs(weights[0][0] - 5.0 / 95.0) < 1e-15 and weights[0][9] == 1.0 and weights[0][-1] == 0.0
    assert abs(weights[0][14] - 0.5) < 1e-15
    # clipped to the grid: a table that starts below it and ends above it
    first, weights = R.tabulated(w0, dw, n, [0.0, 4000.0], [0.0, 4.0])
    assert list(first) == [0] and weights[0].size == n
    assert np.allclose(weights[0], (w0 + np.arange(n) * dw) / 1000.0, rtol=1e-14, atol=0.0)
    for x in ([10.0, 20.0], [2001.0, 2100.0], [1201.0, 1209.0]):
        with pytest.raises(ValueError):
            R.tabulated(w0, dw, n, x, [1.0, 1.0])
    with pytest.raises(ValueError):
        R.tabulated(w0, dw, n, [1300.0, 1200.0], [1.0, 1.0])
    with pytest.raises(ValueError):
        R.tabulated(w0, dw, n, [1200.0, 1300.0], [1.0, 1.0], unit="um")


def test_tabulated_in_nanometres_against_wavenumbers():
    w0, dw, n = 20000.0, 50.0, 401                                # 20 000 .. 40 000 cm-1: 500 .. 250 nm
    knots_nm = np.array([300.0, 320.0, 350.0, 400.0])
    values = np.array([1.0, 0.5, 0.25, 0.0])
    first, weights = R.tabulated(w0, dw, n, knots_nm, values, unit="nm")
    # the grid points between 1e7/400 = 25 000 and 1e7/300 = 33 333.3 cm-1
    assert list(first) == [100] and weights[0].size == 167
    lam = 1e7 / (w0 + (100 + np.arange(167)) * dw)
    assert np.allclose(weights[0], np.interp(lam, knots_nm, values), rtol=1e-13, atol=1e-15)
    assert weights[0][0] == 0.0                                   # 400 nm
    # linear in nm is not linear in cm-1: the same knots given in cm-1 agree at the knots and differ between them
    first_w, weights_w = R.tabulated(w0, dw, n, (1e7 / knots_nm)[::-1], values[::-1])
    assert list(first_w) == list(first) and weights_w[0].size == weights[0].size
    at_350 = np.argmin(np.abs(lam - 350.0))
    assert abs(weights[0][at_350] - weights_w[0][at_350]) < 2e-3
    assert np.max(np.abs(weights[0] - weights_w[0])) > 5e-3


def test_join():
    a, b = R.band(100.0, 1.0, 400, 150.0, 160.0), R.band(100.0, 1.0, 400, 100.0, 499.0)
    first, weights = R.join(a, b, a)
    assert list(first) == [50, 0, 50] and [w.size for w in weights] == [11, 400, 11]
