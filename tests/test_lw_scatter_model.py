"""The float64 model of the longwave scattering correction (tests/lw_scatter_model.py), which the GPU tests compare the
kernel with, held to what it has to be first: the adding form against a dense solve of the boundary-value equations,
float64 against mpmath at 50 digits on the very cases the kernel test uses, and the identities and signs of the correction
(no GPU needed).  All bounds are fractions of the column's largest flux."""
import numpy as np
import pytest

import lw_scatter_model as m

LAYERS = (1, 2, 15)          # V = 2, 3, 16: the kernel test's


def column_scale(fu, fd):
    return max(np.abs(fu).max(), np.abs(fd).max())


def random_columns(L, count, seed):
    rng = np.random.default_rng(seed)
    tau = 10.0 ** rng.uniform(-6, 2, (count, L))
    omega = rng.uniform(0, 0.98, (count, L))
    g = rng.uniform(-1, 1, (count, L))
    emis = rng.uniform(0, 1, count)
    t_layers, t_levels, t_surf = m.temperatures(L, count, seed=seed)
    w = rng.uniform(50.0, 2500.0, count)
    return tau, omega, g, t_layers, t_levels, t_surf, emis, w


@pytest.mark.parametrize("L", LAYERS)
def test_adding_agrees_with_a_dense_solve(L):
    tau, omega, g, t_layers, t_levels, t_surf, emis, w = random_columns(L, 100, 11 + L)
    pu, pd = m.sources(tau, omega, t_layers, t_levels, w[:, None])
    R, T, su, sd, _ = m.layer(tau, omega, g, pu, pd)
    A_L, U_L = 1.0 - emis, emis * np.pi * m.planck(t_surf, w)
    fu, fd = m.adding(R, T, su, sd, A_L, U_L)
    worst = 0.0
    for c in range(len(w)):
        du, dd = m.dense_fluxes(R[c], T[c], su[c], sd[c], A_L[c], U_L[c])
        worst = max(worst, max(np.abs(du - fu[c]).max(), np.abs(dd - fd[c]).max()) / column_scale(fu[c], fd[c]))
    print(f"L = {L}: adding against the dense solve, worst {worst:.2e} of scale")
    assert worst <= 1e-13


@pytest.mark.parametrize("L", LAYERS)
def test_float64_agrees_with_mpmath_on_the_kernel_cases(L):
    """Every case of case_list(L) under three temperature profiles and as many wavenumbers.  Measured on this list: worst
    6.6e-15 of scale (V = 16, a column with one layer of omega = 1 - 1e-9); the bound is a quarter of the GPU test's 1e-12."""
    mp = pytest.importorskip("mpmath")
    N = len(m.case_list(L)["emis"])
    inp = m.kernel_inputs(3, L, N)
    mine = m.model_on_inputs(inp)
    worst, where = 0.0, None
    for c in range(3):
        for i in range(N):
            ref = m.mp_scatter_delta(inp["tau"][c, :, i], inp["omega"][c, :, i], inp["g"][c, :, i], inp["t_layers"][c],
                                     inp["t_levels"][c], inp["t_surf"][c], inp["emis"][c, i], inp["w"][i])
            scale = max(abs(float(x)) for x in ref[2] + ref[3])
            for have, want in zip(mine, ref):
                err = max(abs(float(want[k] - mp.mpf(float(have[c, k, i])))) for k in range(L + 1)) / scale
                if err > worst:
                    worst, where = err, (c, int(inp["case"][c, i]))
    print(f"L = {L}: float64 against mpmath, worst {worst:.2e} of scale at (column, case) {where}")
    assert worst <= 2.5e-13


@pytest.mark.parametrize("L", LAYERS)
def test_no_scattering_gives_exactly_zero(L):
    tau, omega, g, t_layers, t_levels, t_surf, emis, w = random_columns(L, 50, 5 + L)
    du, dd, _, _ = m.scatter_delta(tau, np.zeros_like(omega), g, t_layers, t_levels, t_surf, emis, w)
    for d in (du, dd):
        assert np.array_equal(d, np.zeros_like(d)) and not np.signbit(d).any()


@pytest.mark.parametrize("L", LAYERS)
def test_forward_scattering_alone_changes_nothing(L):
    """g = 1: every scattered photon goes on as it came, and the layer is its absorption twin"""
    tau, omega, g, t_layers, t_levels, t_surf, emis, w = random_columns(L, 50, 23 + L)
    du, dd, fu, fd = m.scatter_delta(tau, omega, np.ones_like(g), t_layers, t_levels, t_surf, emis, w)
    scale = np.maximum(np.abs(fu).max(axis=-1), np.abs(fd).max(axis=-1))[:, None]
    assert (np.abs(du) <= 1e-13 * scale).all() and (np.abs(dd) <= 1e-13 * scale).all()


def test_reflectance_transmittance_and_emissivity_add_up():
    rng = np.random.default_rng(3)
    n = 20000
    tau = 10.0 ** rng.uniform(-8, 3, n)
    omega = np.where(rng.uniform(size=n) < 0.1, 1.0, rng.uniform(0, 1, n))
    g = rng.uniform(-1, 1, n)
    R, T, _, _, eps = m.layer(tau, omega, g, np.ones(n), np.ones(n))
    assert (np.abs((R + T + eps) - 1.0) <= 4 * np.finfo(np.float64).eps).all()
    assert (R >= 0).all() and (T >= 0).all() and (eps >= 0).all()


def test_a_cold_cloud_over_a_warm_surface():
    """tau = 5, omega = 0.7, g = 0.85 in one layer of a thin gas column: the cloud scatters the warm surface's light back
    down and lets less of it out at the top"""
    L = 8
    tau = np.full(L, 0.05)
    omega = np.zeros(L)
    g = np.zeros(L)
    tau[2], omega[2], g[2] = 5.0, 0.7, 0.85
    t_levels = np.linspace(210.0, 295.0, L + 1)
    t_layers = 0.5 * (t_levels[:-1] + t_levels[1:])
    du, dd, fu, fd = m.scatter_delta(tau, omega, g, t_layers, t_levels, 300.0, 0.98, 900.0)
    twin_up_top = fu[0] - du[0]
    print(f"delta_up at the top {du[0] / twin_up_top:+.3%} of the twin's flux, delta_down at the surface {dd[-1]:+.3e}")
    assert du[0] < 0 and du[0] / twin_up_top < -0.01
    assert dd[-1] > 0
