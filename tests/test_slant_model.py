"""slant_model.py's restatement of the shortwave solver against the oracle's, on the CPU: with every layer at one cosine
the restatement is the reference's solver, so the two must agree to rounding at every level and point -- for each of
pipeline_support.MU0 (0.5 = mu_dif; 1e-3 clamps tau/mu at 700 in most layers) and for optics with clouds and an aerosol
among the layers.  That is what keeps test_gpu_sky_zeniths_slant.py from judging the kernels against a wrong reference.
The bound is slant_model.PIN_BOUND: ten times the largest difference measured here, relative to the column's largest flux."""
import numpy as np
import pytest

from direct_beam_model import direct_beam
from pipeline_support import MU0
from slant_model import PIN_BOUND, sw_fluxes

L, N = 15, 48
TSI = 1360.0


def optics(oracle, clouds):
    """A gas (no scattering; 1e-6 to 50 per layer, shuffled per point), Rayleigh scattering, and -- clouds -- an aerosol
    in the lower half and two cloud layers (optical depth 30 and 4000, nearly conservative, g = 0.85), added with the
    oracle's add_optics.  Without clouds g = 0 everywhere: the delta-scaling is the identity."""
    rng = np.random.default_rng(31 + clouds)
    gas = np.empty((L, N))
    for i in range(N):
        gas[:, i] = rng.permutation(np.logspace(-6.0, np.log10(50.0), L))
    z = np.zeros((L, N))
    ray = np.outer(np.linspace(1e-4, 0.3, L), np.linspace(0.1, 1.0, N))
    taus, omegas, gs = [gas, ray], [z, np.ones((L, N))], [z, z]
    if clouds:
        aer = z.copy()
        aer[L // 2:] = rng.uniform(0.01, 0.4, (L - L // 2, N))
        cloud = z.copy()
        cloud[4], cloud[9] = 30.0, 4000.0
        cloud[9, ::3] = 0.0
        taus += [aer, cloud]
        omegas += [np.where(aer > 0.0, 0.92, 0.0), np.where(cloud > 0.0, 0.999999, 0.0)]
        gs += [np.where(aer > 0.0, 0.7, 0.0), np.where(cloud > 0.0, 0.85, 0.0)]
    tau, omega, g = oracle.add_optics(taus, omegas, gs)
    tau[2] = 1e-20                                           # exp(t/mu) <= 1: a layer that holds nothing
    return tau, omega, g


@pytest.mark.parametrize("clouds", [False, True])
@pytest.mark.parametrize("mu0", MU0)
def test_one_cosine_in_every_layer_is_the_oracles_solver(oracle, mu0, clouds):
    tau, omega, g = optics(oracle, clouds)
    rng = np.random.default_rng(7)
    solar = rng.uniform(50.0, 400.0, N)
    alb_dir, alb_dif = rng.uniform(0.0, 0.9, N), rng.uniform(0.0, 0.9, N)
    alb_dir[0], alb_dif[0], alb_dir[-1], alb_dif[-1] = 0.0, 1.0, 1.0, 0.0
    want_up, want_dn = oracle.sw_fluxes(omega, g, tau, mu0, 0.5, alb_dir, alb_dif, TSI, solar)
    for cosines in (mu0, np.full(L, mu0)):
        up, dn, direct = sw_fluxes(omega, g, tau, cosines, 0.5, alb_dir, alb_dif, TSI, solar, mu0)
        ff = max(np.abs(want_up).max(), np.abs(want_dn).max())
        err = max(np.abs(up - want_up).max(), np.abs(dn - want_dn).max()) / ff
        print("mu0", mu0, "clouds", clouds, "largest difference over the largest flux", err, "bound", PIN_BOUND)
        assert ff > 0.0 and err <= PIN_BOUND, err
        assert np.array_equal(direct, direct_beam(tau, omega, g, mu0, TSI, solar))
        assert np.all(direct <= dn) and np.array_equal(direct[0], dn[0])


def test_a_cosine_per_layer_changes_the_beam_below_that_layer_alone(oracle):
    """Raising the cosine of one layer leaves the direct beam above it as it was and strengthens it below; the scale stays
    solar x mu0 (level 0 does not move)."""
    tau, omega, g = optics(oracle, True)
    solar, alb = np.full(N, 100.0), np.full(N, 0.2)
    mu0, j = 0.05, 6
    base = sw_fluxes(omega, g, tau, np.full(L, mu0), 0.5, alb, alb, TSI, solar, mu0)
    cosines = np.full(L, mu0)
    cosines[j] = 0.4
    got = sw_fluxes(omega, g, tau, cosines, 0.5, alb, alb, TSI, solar, mu0)
    assert np.array_equal(got[2][:j + 1], base[2][:j + 1])
    assert np.all(got[2][j + 1:] >= base[2][j + 1:]) and np.any(got[2][j + 1] > base[2][j + 1])
    assert np.array_equal(got[1][0], base[1][0])
