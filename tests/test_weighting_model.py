"""weighting_model.py's restatement of the level-to-space transmittance and of the contribution function against what pins
it down, on the CPU: the V + 1 contribution rows add up to radiance_model.py's upward radiance at the top (closure) on
optics the oracle combined, for one layer, two and twelve, at the radiance tests' secants -- 1e3, where the transmittance
underflows, among them -- and under a surface with emissivities 0 and 1 in it; the transmittance starts at exactly 1, never
rises and stays within [0, 1]; a black surface reflects nothing and a perfect mirror emits nothing, exactly; and at the
four stream secants the c2-weighted sum of the closures is the oracle's own upward flux at the top, to the bound
test_radiance_model.py uses (1e-12 of the row's largest value), which ties the model to the reference solver.  That is
what keeps test_gpu_pipeline_weighting.py from judging the kernel against a wrong reference."""
import numpy as np
import pytest

from radiance_model import STREAM_SECANTS, radiances, stream_sum
from test_radiance_model import SECANTS
from weighting_model import closure_bound, weighting

N = 50
W0, DW = 50.0, 50.0                 # 50 .. 2 500 cm-1
W = W0 + np.arange(N) * DW


def column(oracle, V, seed, t_surf=288.15):
    """Two objects of L = V - 1 layers -- an absorber with layer optical depths from 1e-4 to 5, shuffled per point, and a
    scatterer -- combined by the oracle's add_optics; an emissivity between 0 and 1 with both ends met."""
    L = V - 1
    rng = np.random.default_rng(seed)
    tau_a = np.empty((L, N))
    for i in range(N):
        tau_a[:, i] = rng.permutation(np.logspace(-4.0, np.log10(5.0), L))
    tau_s = rng.uniform(0.0, 0.3, (L, N))
    z = np.zeros((L, N))
    tau, omega, g = oracle.add_optics([tau_a, tau_s], [z, rng.uniform(0.2, 1.0, (L, N))], [z, rng.uniform(0.0, 0.8, (L, N))])
    emis = rng.uniform(0.0, 1.0, N)
    emis[0], emis[1], emis[-1] = 1.0, 0.0, 0.3
    t_levels = np.linspace(210.0, t_surf - 2.0, V)
    t_layers = 0.5 * (t_levels[1:] + t_levels[:-1])
    return dict(tau=tau, omega=omega, emis=emis, t_surf=t_surf, t_layers=t_layers, t_levels=t_levels)


def both(c, secants, emis=None):
    emis = c["emis"] if emis is None else emis
    T, K = weighting(c["tau"], c["omega"], emis, c["t_surf"], c["t_layers"], c["t_levels"], W, secants)
    rad = radiances(c["tau"], c["omega"], emis, c["t_surf"], c["t_layers"], c["t_levels"], W, secants)
    return T, K, rad


@pytest.mark.parametrize("V", [2, 3, 13])
def test_rows_add_up_to_the_upward_radiance(oracle, V):
    c = column(oracle, V, 40 + V)
    assert np.any(c["omega"] > 0.0) and np.any(c["emis"] == 0.0) and np.any(c["emis"] == 1.0)
    T, K, rad = both(c, SECANTS)
    assert T.shape == (len(SECANTS), V, N) and K.shape == (len(SECANTS), V + 1, N)
    total = K.sum(axis=1)
    bound = closure_bound(K)
    assert np.array_equal(bound, 4.0 * (V + 1) * 2.0 ** -52 * np.abs(K).sum(axis=1))      # (L + 2 = V + 1 terms)
    err = np.abs(total - rad[:, 0])
    print("V", V, "closure: worst", (err / np.maximum(bound, 1e-300)).max(), "of the bound")
    assert np.all(err <= bound) and np.all(rad[:, 0] > 0.0)
    assert np.any(T[-1, V - 1] == 0.0) or V == 2              # (secant 1e3: the surface is out of sight)
    assert np.all(K >= 0.0)


@pytest.mark.parametrize("V", [2, 3, 13])
def test_transmittance_profile(oracle, V):
    c = column(oracle, V, 50 + V)
    T, K, rad = both(c, SECANTS)
    assert np.all(T[:, 0] == 1.0)
    assert np.all(np.diff(T, axis=1) <= 0.0)
    assert np.all((T >= 0.0) & (T <= 1.0))
    # the longer path is the darker one
    assert np.all(T[1] <= T[0]) and np.all(T[3] <= T[2])


def test_degenerate_surfaces(oracle):
    c = column(oracle, 13, 61)
    T, K, rad = both(c, SECANTS, emis=np.ones(N))
    assert np.all(K[:, -1] == 0.0) and np.all(K[0, -2] > 0.0)
    T, K, rad = both(c, SECANTS, emis=np.zeros(N))
    assert np.all(K[:, -2] == 0.0) and np.all(K[0, -1] > 0.0)
    # the rows of the atmosphere's own emission do not know the surface
    T1, K1, rad1 = both(c, SECANTS)
    assert np.array_equal(K1[:, :-2], K[:, :-2]) and np.array_equal(T1, T)


@pytest.mark.parametrize("V,seed,t_surf", [(13, 21, 288.15), (3, 22, 310.0), (2, 23, 245.0)])
def test_stream_secants_give_the_oracles_upward_flux(oracle, V, seed, t_surf):
    c = column(oracle, V, seed, t_surf)
    up, dn = oracle.lw_fluxes(W0, DW, t_surf, c["t_layers"], c["t_levels"], c["tau"], c["omega"], c["emis"])
    T, K, rad = both(c, STREAM_SECANTS)
    got, want = stream_sum(K.sum(axis=1)), up[0]
    err = np.abs(got - want).max() / np.abs(want).max()
    print("V", V, "T_surf", t_surf, "relative to the row's largest value:", err)
    assert np.abs(want).max() > 0.0 and err <= 1e-12, err
