"""radiance_model.py's restatement of the longwave radiance at a viewing angle against the oracle's own longwave solver, on
the CPU.  The solver's four streams are radiances at the secants -c1[s], so the c2-weighted sum, in stream order, of the
restatement's radiances at those four secants is the solver's flux: upward at the top, downward at the surface, to one-ulp
differences of exp (numpy's against libm's; 1e-12 of the row's largest value is the project's bound for those,
test_gpu_optics_solvers.py).  Then the limits that pin the definition down: no atmosphere, an isothermal black cavity, an
opaque atmosphere, and limb darkening.  That is what keeps test_gpu_pipeline_radiances.py from judging the kernel against a
wrong reference."""
import numpy as np
import pytest

from lw_jacobian_model import planck
from radiance_model import STREAM_SECANTS, brightness, radiances, stream_sum
from test_lw_jacobian_model import DW, L, N, W0, column

SECANTS = (1.0, 1.5, 14.402613260847248, 1e3)
W = W0 + np.arange(N) * DW


@pytest.mark.parametrize("seed,t_surf", [(21, 288.15), (22, 310.0), (23, 245.0)])
def test_stream_secants_give_the_oracles_fluxes(oracle, seed, t_surf):
    c = column(seed, t_surf)
    up, dn = oracle.lw_fluxes(W0, DW, t_surf, c["t_layers"], c["t_levels"], c["tau"], c["omega"], c["emis"])
    rad = radiances(c["tau"], c["omega"], c["emis"], t_surf, c["t_layers"], c["t_levels"], W, STREAM_SECANTS)
    assert rad.shape == (4, 2, N)
    for name, got, want in (("up at the top", stream_sum(rad[:, 0]), up[0]), ("down at the surface", stream_sum(rad[:, 1]), dn[L])):
        err = np.abs(got - want).max() / np.abs(want).max()
        print("T_surf", t_surf, name, "relative to the row's largest value:", err)
        assert np.abs(want).max() > 0.0 and err <= 1e-12, (name, err)


def test_no_atmosphere():
    c = column(31, 300.0)
    rad = radiances(np.zeros((L, N)), c["omega"], c["emis"], 300.0, c["t_layers"], c["t_levels"], W, SECANTS)
    for k in range(len(SECANTS)):
        assert np.array_equal(rad[k, 0], c["emis"] * planck(300.0, W))
        assert np.all(rad[k, 1] == 0.0)


def test_isothermal_black_cavity():
    c = column(32, 300.0)
    T = 275.0
    rad = radiances(c["tau"], c["omega"], np.ones(N), T, np.full(L, T), np.full(L + 1, T), W, SECANTS)
    b = planck(T, W)
    assert np.all(np.abs(rad[:, 0] - b) <= 1e-12 * b)
    tb = brightness(rad[:, 0], W)
    assert np.all(np.abs(tb - T) <= 1e-12 * T), np.abs(tb - T).max()
    assert np.array_equal(brightness(np.array([0.0, -1.0]), W[:2]), [0.0, 0.0])


def test_opaque_atmosphere_hides_the_surface():
    c = column(33, 300.0)
    tau = np.full((L, N), 1e4)
    a = radiances(tau, np.zeros((L, N)), c["emis"], 300.0, c["t_layers"], c["t_levels"], W, SECANTS)
    b = radiances(tau, np.zeros((L, N)), np.full(N, 0.2), 220.0, c["t_layers"], c["t_levels"], W, SECANTS)
    assert np.array_equal(a[:, 0], b[:, 0]) and np.all(a[:, 0] > 0.0)


def test_limb_darkening():
    """A column that cools upward under a black surface: the longer the path, the colder the layer the radiance comes from."""
    c = column(34, 300.0)
    assert np.all(np.diff(c["t_levels"]) > 0.0) and c["t_levels"][-1] < 300.0          # (index 0 is the top)
    secants = sorted(SECANTS + (2.0, 5.0, 40.0))
    rad = radiances(c["tau"], c["omega"], np.ones(N), 300.0, c["t_layers"], c["t_levels"], W, secants)
    up = rad[:, 0]
    assert np.all(up[1:] <= up[:-1])
    assert np.any(up[-1] < 0.99 * up[0])
