"""direct_beam_model.py's restatement of the solver's direct beam against the oracle, on the CPU.  Without scattering in
the atmosphere (omega = 0 in every layer) and with a black surface nothing is reflected anywhere, so the oracle's
downward shortwave flux IS the direct beam: the restatement must give the same number at every level and point.  That is
what keeps test_gpu_pipeline_direct.py from judging the kernels against a wrong reference."""
import numpy as np
import pytest

from direct_beam_model import direct_beam, pure_transmission, three

L, N = 24, 40
TSI = 1360.0


def layers(seed):
    """Layer optical depths from 1e-6 to 50, each decade in some layer of every point, shuffled per point."""
    rng = np.random.default_rng(seed)
    tau = np.empty((L, N))
    for i in range(N):
        tau[:, i] = rng.permutation(np.logspace(-6.0, np.log10(50.0), L))
    tau[0, 0], tau[-1, -1] = 1e-6, 50.0
    return tau, rng.uniform(0.0, 0.9, (L, N)), rng.uniform(50.0, 400.0, N)


@pytest.mark.parametrize("mu0", [1.0, 0.5, 0.3, 0.05])
def test_restatement_is_the_oracles_downward_flux_without_scattering(oracle, mu0):
    tau, g, solar = layers(11)
    omega, black = np.zeros((L, N)), np.zeros(N)
    up, dn = oracle.sw_fluxes(omega, g, tau, mu0, 0.5, black, black, TSI, solar)
    got = direct_beam(tau, omega, g, mu0, TSI, solar)
    assert got.shape == dn.shape == (L + 1, N)
    assert np.all(up == 0.0)
    err = np.abs(got - dn) / dn[0]
    print("mu0", mu0, "largest error over the level-0 value", err.max(), "smallest beam", got[-1].min() / got[0].max())
    assert np.all(err <= 1e-13), err.max()
    assert np.array_equal(got[0], dn[0])
    assert got[-1].min() < 1e-12 * got[0].max() and got[1].max() > 0.99 * got[0].min()      # both ends of the range are met


@pytest.mark.parametrize("mu0", [1.0, 0.3, 0.05, 1e-3])
def test_direct_beam_is_at_most_the_downward_flux(oracle, mu0):
    tau, g, solar = layers(12)
    rng = np.random.default_rng(13)
    omega = rng.uniform(1e-6, 1.0 - 1e-6, (L, N))
    tau[3] = 1e-20                      # exp(t/mu) <= 1: a layer that holds nothing
    tau[5, ::2] = 4000.0                # the clamp of shortwave.c:137-145 strikes (either branch, by omega and mu0)
    for alb in (np.zeros(N), rng.uniform(0.0, 0.9, N)):
        up, dn = oracle.sw_fluxes(omega, g, tau, mu0, 0.5, alb, alb, TSI, solar)
        got = direct_beam(tau, omega, g, mu0, TSI, solar)
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
        assert np.all(got <= dn), np.max(got - dn)
        assert np.all(got[1:] <= got[:-1])
        assert np.array_equal(got[0], dn[0])
        assert np.array_equal(got[4], got[3])        # the empty layer passes the beam on unchanged


def test_pure_transmission_cases():
    mu = 0.4
    one = np.ones((1, 1))
    assert pure_transmission(2.0 * one, 0.0 * one, 0.5 * one, mu)[0, 0] == np.exp(-2.0 / mu)
    assert pure_transmission(1e-20 * one, 0.5 * one, 0.5 * one, mu)[0, 0] == 1.0
    # delta-scaling: the beam sees tau (1 - omega g^2)
    assert pure_transmission(2.0 * one, 0.5 * one, 0.8 * one, mu)[0, 0] == np.exp(-(2.0 * (1.0 - 0.5 * 0.8 * 0.8)) / mu)
    # the clamp: 1/mu > k and tau/mu > 700 -> t = 700 mu
    assert pure_transmission(4000.0 * one, 0.5 * one, 0.0 * one, mu)[0, 0] == np.exp(-(700.0 * mu) / mu)
    assert np.array_equal(three(np.array([3.0, 2.0, 1.0]), -1), [3.0, 1.0, 0.0])
    assert np.array_equal(three(np.array([3.0, 2.0, 1.0]), 1), [3.0, 1.0, 2.0])
