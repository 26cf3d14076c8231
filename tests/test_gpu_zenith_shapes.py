"""grt_pipeline_run_zeniths at the shapes where its kernels and indexing go wrong: grids of two points up to one live lane
past two solver blocks, one-layer columns (the sweeps have no interior), 1 angle up to one past two chunks of the
shared-layer kernel, a chunk that is only partly filled, night angles in the last chunk only and in every chunk, an angle
at mu_dif, the user level at and next to both ends (levels 1 and L - 1 force the two sweeps), and a park block that
forces one launch per angle.  The references are the oracle and, in the deterministic mode, grt_pipeline_run and
grt_pipeline_run_profiles fed one angle at a time: bit for bit."""
import numpy as np
import pytest

from grtcode_amd import api
from pipeline_support import (LEVEL_TOL, SOLVER_NS as NS, _deterministic, columns, oracle_column, surface, user_index)
from pipeline_support import solver_bands as bands  # noqa: F401  (module fixture)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

ZN = api.GRT_ZENITH_CHUNK
ZS = (1, ZN - 1, ZN, ZN + 1, 2 * ZN + 1)
POOL = (1.0, 0.5, 0.05, 1e-3, 0.3, 0.999, 0.01, 0.7, 0.2)      # 0.5 = mu_dif; 1e-3 clamps tau/mu at 700 in most layers

# grid length, levels, angles, user level, where the night samples are
CASES = [(2, 2, ZS[0], "-1", "none"), (3, 3, ZS[1], "0", "none"), (64, 16, ZS[2], "L", "some"),
         (65, 2, ZS[3], "1", "last_chunk"), (128, 3, ZS[4], "L-1", "last_chunk"), (129, 16, ZS[4], "1", "some"),
         (257, 16, ZS[3], "-1", "last_chunk"), (65, 3, ZS[2], "0", "all"), (129, 3, ZS[4], "-1", "last_chunk"),
         (257, 2, ZS[1], "L-1", "some"), (128, 16, ZS[0], "L", "none")]
assert {n for n, *_ in CASES} == set(NS) and {v for _, v, *_ in CASES} == {2, 3, 16}
assert {z for _, _, z, *_ in CASES} == set(ZS) and {u for *_, u, _ in CASES} == {"-1", "0", "1", "L-1", "L"}


def angles(ncol, Z, night):
    """[ncol][Z] from POOL, another order per column; night: none, some (one per column, at another place in each),
    last_chunk (the samples of the last chunk of ZN, and only those) or all."""
    mu = np.array([[POOL[(k + 2 * c) % len(POOL)] for k in range(Z)] for c in range(ncol)])
    if night == "some":
        for c in range(ncol):
            mu[c, (c + 1) % Z] = (0.0, -0.3)[c % 2]
    elif night == "last_chunk":
        mu[:, ((Z - 1) // ZN) * ZN:] = -0.1
    elif night == "all":
        mu[:] = -0.5
    return mu


def under(cols, mu_k):
    """The columns under one angle each; a night sample's column runs under 1.0 and is not compared."""
    return [dict(col, mu0=(m if m > 0.0 else 1.0)) for col, m in zip(cols, mu_k)]


def fold(weights, rows):
    """sum_k w_k F_k in the mean kernel's order: each product rounded, the angles k = 0 .. Z - 1 in order."""
    acc = weights[:, 0, None] * rows[:, 0]
    for k in range(1, rows.shape[1]):
        acc = acc + weights[:, k, None] * rows[:, k]
    return acc


def check_against_run(pipe, cols, mu, angles6, prof, ks):
    """Angles ks of every column: the six rows are grt_pipeline_run's and the levels grt_pipeline_run_profiles' for that
    angle, bit for bit; night samples are zeros."""
    ncol = len(cols)
    for k in ks:
        g1, keep1 = api.make_columns(under(cols, mu[:, k]), MOL_ORDER, cfc_order=(0, 1))
        day = mu[:, k] > 0.0
        if angles6 is not None:
            pipe.run(g1)
            one = pipe.fluxes(ncol)
            assert np.array_equal(angles6[day, k], one[day, 6:]), k
            assert np.all(angles6[~day, k] == 0.0) and not np.any(np.signbit(angles6[~day, k])), k
        if prof is not None:
            pipe.run_profiles(g1)
            p1 = pipe.profiles(ncol)
            assert np.array_equal(prof["angle_up"][day, k], p1["sw_up"][day]), k
            assert np.array_equal(prof["angle_down"][day, k], p1["sw_down"][day]), k
            assert np.array_equal(prof["angle_fluxes"][day, k], p1["fluxes"][day, 6:]), k
            assert np.all(prof["angle_up"][~day, k] == 0.0) and np.all(prof["angle_down"][~day, k] == 0.0), k
            assert np.array_equal(prof["lw_up"], p1["lw_up"]) and np.array_equal(prof["lw_down"], p1["lw_down"]), k


@pytest.mark.parametrize("n,V,Z,ul,night", CASES, ids=[f"n{n}-V{V}-Z{Z}-ul{u}-night_{w}" for n, V, Z, u, w in CASES])
def test_zeniths_at_edge_shapes(bands, oracle, lib, device, monkeypatch, n, V, Z, ul, night):
    L = V - 1
    user_level = user_index(ul, L)
    lwb, swb = bands[n]
    cols = columns(V)
    ncol = len(cols)
    mu = angles(ncol, Z, night)
    wt = np.array([[0.25 + 0.125 * ((c + 3 * k) % 5) for k in range(Z)] for c in range(ncol)])
    go_lw, _ = lwb.gas_optics(device, V)
    go_sw, grid_sw = swb.gas_optics(device, V)
    emis, _ = surface(n, 1 + n)
    _, alb = surface(n, 2 + n)
    solar = api.create_solar_flux(grid_sw, swb.files["solar"])
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gz, keep_z = api.make_zeniths(mu, wt)
    fused = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=False)
    mat = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=True)

    # ---- the default mode against the oracle: two day angles of the first and the last column ----------------------- #
    got = {}
    for pipe in (fused, mat):
        pipe.run_zeniths(gcols, gz)
        fluxes, angles6 = pipe.zenith_fluxes(ncol, Z)
        pipe.run_zeniths(gcols, gz, profiles=True)
        got[pipe] = (fluxes, angles6, pipe.zenith_profiles(ncol, Z))
    for c in (0, ncol - 1):
        days = [k for k in range(Z) if mu[c, k] > 0.0]
        for k in sorted({days[0], days[-1]} if days else ()):
            w = oracle_column(oracle, lib, swb, dict(cols[c], mu0=mu[c, k]), False, emis, alb, solar, user_level)
            up_w = np.array([oracle.integrate_row(r, swb.dw) for r in w["up"]])
            dn_w = np.array([oracle.integrate_row(r, swb.dw) for r in w["dn"]])
            ff = max(np.abs(up_w).max(), np.abs(dn_w).max())
            assert ff > 0.0
            for pipe in (fused, mat):
                fluxes, angles6, prof = got[pipe]
                what = (c, k, pipe.keep_spectra)
                assert np.max(np.abs(angles6[c, k] - w["integ"])) <= LEVEL_TOL * ff, what
                assert np.max(np.abs(prof["angle_fluxes"][c, k] - w["integ"])) <= LEVEL_TOL * ff, what
                assert np.max(np.abs(prof["angle_up"][c, k] - up_w)) <= LEVEL_TOL * ff, what
                assert np.max(np.abs(prof["angle_down"][c, k] - dn_w)) <= LEVEL_TOL * ff, what
                if user_level < 0:
                    assert angles6[c, k, 2] == 0.0 and angles6[c, k, 5] == 0.0, what

    # ---- the deterministic mode's identities ----------------------------------------------------------------------- #
    _deterministic(lib, True)
    try:
        fused.run_zeniths(gcols, gz)
        fluxes, angles6 = fused.zenith_fluxes(ncol, Z)
        fused.run_zeniths(gcols, gz, profiles=True)
        prof = fused.zenith_profiles(ncol, Z)
        check_against_run(fused, cols, mu, angles6, prof, range(Z))
        assert np.array_equal(fluxes[:, 6:], fold(wt, angles6))
        assert np.array_equal(prof["sw_up"], fold(wt, prof["angle_up"]))
        assert np.array_equal(prof["sw_down"], fold(wt, prof["angle_down"]))
        if night == "all":
            assert np.all(fluxes[:, 6:] == 0.0) and np.all(prof["sw_heating"] == 0.0)
        # without weights: the sum, then one division by Z
        gz0, keep_0 = api.make_zeniths(mu)
        fused.run_zeniths(gcols, gz0)
        f0, a0 = fused.zenith_fluxes(ncol, Z)
        assert np.array_equal(a0, angles6) and np.array_equal(f0[:, 6:], fold(np.ones_like(mu), angles6) / float(Z))
        # the zenith instance of the six-row solver in place of the shared-layer kernel
        monkeypatch.setenv("GRT_ZENITH_SHARED", "0")
        fused.run_zeniths(gcols, gz)
        f1, a1 = fused.zenith_fluxes(ncol, Z)
        monkeypatch.delenv("GRT_ZENITH_SHARED")
        assert np.array_equal(f1, fluxes) and np.array_equal(a1, angles6)
        # two sweeps: the six-row form's rows are the profile form's level rows at 0, L and the user level
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        fused.run_zeniths(gcols, gz)
        f2, a2 = fused.zenith_fluxes(ncol, Z)
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        assert np.array_equal(a2, prof["angle_fluxes"]) and np.array_equal(f2, prof["fluxes"])
        assert np.array_equal(a2[:, :, 0], prof["angle_up"][:, :, 0]) and np.array_equal(a2[:, :, 4], prof["angle_down"][:, :, L])
        # the materialised form, first and last angle
        mat.run_zeniths(gcols, gz)
        fm, am = mat.zenith_fluxes(ncol, Z)
        mat.run_zeniths(gcols, gz, profiles=True)
        pm = mat.zenith_profiles(ncol, Z)
        check_against_run(mat, cols, mu, am, pm, sorted({0, Z - 1}))
        assert np.array_equal(fm[:, 6:], fold(wt, am))
    finally:
        _deterministic(lib, False)
    for pipe in (fused, mat):
        pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("ul", ["1", "-1"])
def test_a_park_block_of_the_batch_size_takes_one_launch_per_angle(bands, lib, device, ul):
    """max_columns = ncol = 2, Z = 3: the park block holds one angle of the batch, so the two-sweep forms run in three
    launches in stream order (the profile form always; the six-row form with the user level inside the column)."""
    n, V, Z = 65, 7, 3
    user_level = user_index(ul, V - 1)
    lwb, swb = bands[n]
    cols = columns(V)[:2]
    mu = angles(2, Z, "none")
    mu[1, 1] = -0.25
    go_lw, _ = lwb.gas_optics(device, V)
    go_sw, grid_sw = swb.gas_optics(device, V)
    emis, _ = surface(n, 5)
    _, alb = surface(n, 6)
    solar = api.create_solar_flux(grid_sw, swb.files["solar"])
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gz, keep_z = api.make_zeniths(mu)
    pipe = api.Pipeline(go_lw, go_sw, 2, user_level, emis, alb, solar, spectral=False)
    _deterministic(lib, True)
    try:
        pipe.run_zeniths(gcols, gz)
        fluxes, angles6 = pipe.zenith_fluxes(2, Z)
        pipe.run_zeniths(gcols, gz, profiles=True)
        prof = pipe.zenith_profiles(2, Z)
        check_against_run(pipe, cols, mu, angles6, prof, range(Z))
        assert np.array_equal(prof["sw_up"], fold(np.ones_like(mu), prof["angle_up"]) / float(Z))
        assert np.array_equal(fluxes[:, 6:], fold(np.ones_like(mu), angles6) / float(Z))
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
