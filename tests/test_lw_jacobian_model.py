"""lw_jacobian_model.py's restatement of dF_up/dT_surf against the oracle's own longwave solver, on the CPU, by central
differences (lw_fluxes(T_surf + d) - lw_fluxes(T_surf - d)) / 2 d of the upward rows.  B(T_surf) enters the upward fluxes
linearly, so the difference quotient misses the true derivative by d^2/6 B'''/B' of it at most; in Wien's form B'''/B' =
(x^2 - 6 x + 6)/T^2, x = c2 w/T, largest at the top of a grid that reaches x >= 6, and a factor 2 covers the Bose
factor's departure from Wien's law.  Halving d must cut the difference by four (second order, towards the restatement),
and the downward rows must not move at all.  That is what keeps test_gpu_pipeline_jacobian.py from judging the kernels
against a wrong reference."""
import math

import numpy as np
import pytest

from lw_jacobian_model import (PLANCK_C2, STREAM_C2, planck, planck_derivative, surface_closed_form, surface_jacobian,
                               three)

L, N = 12, 50
W0, DW = 50.0, 50.0                 # 50 .. 2 500 cm-1: x_max = c2 w_n / T_surf is 11 to 15 at the temperatures below


def truncation_bound(delta, t_surf, w_top):
    """Relative to the largest level value: 2 d^2/6 (x_max^2 - 6 x_max + 6)/T_surf^2."""
    x_max = PLANCK_C2 * w_top / t_surf
    assert x_max >= 6.0
    return 2.0 * delta * delta / 6.0 * (x_max * x_max - 6.0 * x_max + 6.0) / (t_surf * t_surf)


def column(seed, t_surf):
    """Layer optical depths from 1e-4 to 5, shuffled per point; single-scattering albedo up to 0.5; an emissivity between
    0.3 and 1 with both ends met; layer and level temperatures that do not matter to the derivative."""
    rng = np.random.default_rng(seed)
    tau = np.empty((L, N))
    for i in range(N):
        tau[:, i] = rng.permutation(np.logspace(-4.0, np.log10(5.0), L))
    omega = rng.uniform(0.0, 0.5, (L, N))
    emis = rng.uniform(0.3, 1.0, N)
    emis[0], emis[-1] = 1.0, 0.3
    t_levels = np.linspace(210.0, t_surf - 2.0, L + 1)
    t_layers = 0.5 * (t_levels[1:] + t_levels[:-1])
    return dict(tau=tau, omega=omega, emis=emis, t_surf=t_surf, t_layers=t_layers, t_levels=t_levels)


@pytest.mark.parametrize("seed,t_surf", [(21, 288.15), (22, 310.0), (23, 245.0)])
def test_restatement_is_the_derivative_of_the_oracles_solver(oracle, seed, t_surf):
    c = column(seed, t_surf)
    w = W0 + np.arange(N) * DW
    jac = surface_jacobian(c["tau"], c["omega"], c["emis"], t_surf, w)
    assert jac.shape == (L + 1, N)
    largest = np.abs(jac).max()
    assert largest > 0.0
    diff = {}
    for delta in (0.1, 0.05):
        up_p, dn_p = oracle.lw_fluxes(W0, DW, t_surf + delta, c["t_layers"], c["t_levels"], c["tau"], c["omega"], c["emis"])
        up_m, dn_m = oracle.lw_fluxes(W0, DW, t_surf - delta, c["t_layers"], c["t_levels"], c["tau"], c["omega"], c["emis"])
        quotient = (up_p - up_m) / (2.0 * delta)
        diff[delta] = quotient - jac
        bound = truncation_bound(delta, t_surf, w[-1]) * largest
        print("T_surf", t_surf, "delta", delta, "largest difference", np.abs(diff[delta]).max(), "bound", bound)
        assert np.all(np.abs(diff[delta]) <= bound), (delta, np.abs(diff[delta]).max(), bound)
        # the longwave has no scattering: the downward rows do not know the surface
        assert np.all((dn_p - dn_m) / (2.0 * delta) == 0.0)
    # second order, towards the restatement: halving delta cuts the difference by four
    big = np.abs(diff[0.1]) > 1e-11 * largest
    assert np.count_nonzero(big) > big.size // 2
    ratio = diff[0.1][big] / diff[0.05][big]
    print("ratio of the differences at 0.1 K and 0.05 K:", ratio.min(), "to", ratio.max(), "on", np.count_nonzero(big))
    assert np.all((ratio >= 3.5) & (ratio <= 4.5)), (ratio.min(), ratio.max())


def test_restatement_cases():
    w = W0 + np.arange(N) * DW
    c = column(31, 300.0)
    jac = surface_jacobian(c["tau"], c["omega"], c["emis"], 300.0, w)
    # the surface row is the closed form, point by point, and the rows never increase upward
    assert np.allclose(jac[-1], c["emis"] * planck_derivative(300.0, w) * sum(STREAM_C2), rtol=1e-15, atol=0.0)
    assert np.all(jac >= 0.0) and np.all(jac[:-1] <= jac[1:])
    # an empty atmosphere passes the surface row on unchanged; a black one lets nothing through
    assert np.array_equal(surface_jacobian(np.zeros((L, N)), c["omega"], c["emis"], 300.0, w), np.tile(jac[-1], (L + 1, 1)))
    assert np.all(surface_jacobian(np.full((L, N), 1e4), np.zeros((L, N)), c["emis"], 300.0, w)[:-1] == 0.0)
    # no emissivity, no derivative; and where planck_law clamps its exponent the derivative is 0
    assert np.all(surface_jacobian(c["tau"], c["omega"], np.zeros(N), 300.0, w) == 0.0)
    assert planck_derivative(2.0, np.array([1000.0]))[0] == 0.0 and planck(2.0, np.array([1000.0]))[0] > 0.0
    # dB/dT against a difference of planck itself
    d = (planck(300.05, w) - planck(299.95, w)) / 0.1
    assert np.all(np.abs(d - planck_derivative(300.0, w)) <= 1e-6 * planck_derivative(300.0, w).max())
    assert np.array_equal(three(np.array([3.0, 2.0, 1.0]), -1), [3.0, 1.0, 0.0])
    assert np.array_equal(three(np.array([3.0, 2.0, 1.0]), 1), [3.0, 1.0, 2.0])
    f = [float(v) for v in c["emis"] * planck_derivative(300.0, w) * sum(STREAM_C2)]
    exact = DW * math.fsum([0.5 * f[0]] + f[1:-1] + [0.5 * f[-1]])
    assert abs(surface_closed_form(c["emis"], 300.0, w, DW) - exact) <= 1e-14 * exact
