"""response_model.py's restatement of grt_pipeline_run_sky_weighted's rows against the oracle, on the CPU: with r = 1 on the
whole grid every weighted row is the oracle's trapezoid of the level's spectral row, and without scattering over a black
surface -- where the downward flux is the beam and nothing comes up -- the actinic flux is the beam's alone, S/mu0, exactly.
That is what keeps test_gpu_pipeline_weighted.py from judging the kernels against a wrong reference."""
import numpy as np
import pytest

from direct_beam_model import direct_beam
from pipeline_support import assert_trapezoid
from response_model import MU_DIF, actinic, mean_in_order, trapezoid_weights, weighted_rows

L, N, DW = 12, 150, 10.0
TSI = 1360.0


def layers(seed):
    rng = np.random.default_rng(seed)
    tau = 10.0 ** rng.uniform(-4.0, 1.0, (L, N))
    return tau, rng.uniform(0.0, 0.9, (L, N)), rng.uniform(50.0, 400.0, N), rng


def whole_grid():
    return [0], [np.ones(N)]


def test_trapezoid_weights():
    t = trapezoid_weights(5, 2.0)
    assert np.array_equal(t, [1.0, 2.0, 2.0, 2.0, 1.0])
    assert np.array_equal(trapezoid_weights(2, 3.0), [1.5, 1.5])


@pytest.mark.parametrize("mu0", [1.0, 0.3])
def test_all_ones_is_the_oracles_trapezoid_shortwave(oracle, mu0):
    tau, g, solar, rng = layers(21)
    omega, alb = rng.uniform(0.0, 0.99, (L, N)), rng.uniform(0.0, 0.8, N)
    up, dn = oracle.sw_fluxes(omega, g, tau, mu0, MU_DIF, alb, alb, TSI, solar)
    beam = direct_beam(tau, omega, g, mu0, TSI, solar)
    for name, rows in (("up", up), ("down", dn), ("direct", beam)):
        got = weighted_rows(rows, DW, *whole_grid())
        assert got.shape == (1, L + 1)
        for lev in range(L + 1):
            assert_trapezoid(got[0, lev], rows[lev], DW, (name, lev))
            assert_trapezoid(oracle.integrate_row(rows[lev], DW), rows[lev], DW, (name, lev, "oracle"))


def test_all_ones_is_the_oracles_trapezoid_longwave(oracle):
    tau, _, _, rng = layers(22)
    omega, emis = np.zeros((L, N)), rng.uniform(0.5, 1.0, N)
    t_lev = np.linspace(220.0, 290.0, L + 1)
    t_lay = 0.5 * (t_lev[1:] + t_lev[:-1])
    up, dn = oracle.lw_fluxes(100.0, DW, 291.0, t_lay, t_lev, tau, omega, emis)
    for name, rows in (("up", up), ("down", dn)):
        got = weighted_rows(rows, DW, *whole_grid())
        for lev in range(L + 1):
            assert_trapezoid(got[0, lev], rows[lev], DW, (name, lev))
            assert_trapezoid(oracle.integrate_row(rows[lev], DW), rows[lev], DW, (name, lev, "oracle"))


@pytest.mark.parametrize("mu0", [1.0, 0.5, 0.05])
def test_actinic_flux_of_a_beam_alone(oracle, mu0):
    tau, g, solar, rng = layers(23)
    omega, black = np.zeros((L, N)), np.zeros(N)
    up, dn = oracle.sw_fluxes(omega, g, tau, mu0, MU_DIF, black, black, TSI, solar)
    assert np.all(up == 0.0)
    first = [0, 40, 77]
    weights = [np.ones(N), rng.uniform(-1.0, 2.0, 50), np.array([3.5])]
    U, D = weighted_rows(up, DW, first, weights), weighted_rows(dn, DW, first, weights)
    # nothing is scattered and nothing reflected: the oracle's downward flux is the beam, S = D, and U = 0
    A = actinic(D, D, U, mu0)
    assert np.array_equal(A, D / mu0)
    # ... and the restated beam is that downward flux (test_direct_beam_model.py: 1e-13 of the level-0 value per point)
    S = weighted_rows(direct_beam(tau, omega, g, mu0, TSI, solar), DW, first, weights)
    scale = weighted_rows(np.abs(dn[:1]), DW, first, [np.abs(w) for w in weights])[:, 0]
    assert np.all(np.abs(S - D) <= 1e-12 * scale[:, None])
    err = np.abs(actinic(S, D, U, mu0) - S / mu0)
    assert np.all(err <= (1.0 / MU_DIF) * 1e-12 * scale[:, None])


def test_responses_are_linear_and_local():
    rng = np.random.default_rng(24)
    rows = rng.uniform(0.0, 5.0, (3, N))
    r = rng.uniform(-1.0, 1.0, 30)
    one = weighted_rows(rows, DW, [100], [r])
    assert np.array_equal(weighted_rows(rows, DW, [100], [2.0 * r]), 2.0 * one)
    assert np.array_equal(weighted_rows(rows, DW, [100], [-r]), -one)
    assert np.array_equal(weighted_rows(rows, DW, [5, 100, 100], [np.ones(3), r, r])[1:], np.vstack([one, one]))
    assert np.all(weighted_rows(rows, DW, [100], [np.zeros(30)]) == 0.0)
    # a single end point carries dw/2
    assert weighted_rows(rows, DW, [0], [np.array([1.0])])[0, 1] == rows[1, 0] * (0.5 * DW)
    assert weighted_rows(rows, DW, [N - 1], [np.array([2.0])])[0, 2] == rows[2, N - 1] * (0.5 * DW * 2.0)
    assert weighted_rows(rows, DW, [7], [np.array([1.0])])[0, 0] == rows[0, 7] * DW
    assert np.array_equal(mean_in_order([rows, rows]), rows)
