"""grt_pipeline_run_sky_zeniths_direct: grt_pipeline_run_sky_zeniths with a direct-beam albedo per (column, angle) and every
angle's direct beam.  The yardstick is in the tree: per angle, grt_pipeline_run_sky_direct under that angle with that
angle's knots as the direct albedo of the surface in force -- bit for bit in the deterministic mode; then the folds, the
reductions to grt_pipeline_run_sky_zeniths, the two forms of the pipeline against each other, the oracle with the angle's
row as alb_dir and direct_beam_model's restatement, the edge shapes of test_gpu_sky_zenith_shapes.py with 2, 3 and 9
knots, batch indexing, what the entry point refuses, and the older entry points before and after it on one pipeline."""
import ctypes as C

import numpy as np
import pytest

from aerosol_model import oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from direct_beam_model import direct_beam, three
from grtcode_amd import api
from pipeline_support import LEVEL_TOL, SETS, SOLVER_NS, _deterministic, _sentinel, limits, make, user_index
from pipeline_support import solver_bands as bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from sky_zenith_support import (AEROSOL, ALL, BOTH, CLEAN, CLOUD, NAMES, aerosols_of, angles, fold, positions, positive_zero,
                                run_sky, run_sky_zeniths, under)
from surface_support import host_rows
from test_gpu_sky_zenith_shapes import Inputs

pytestmark = pytest.mark.gpu

ZN = api.GRT_ZENITH_CHUNK
ZS = (1, ZN - 1, ZN, ZN + 1, 2 * ZN + 1)
NS = (2, 65, 129, 257)
NCOL = 3
DIRECT_KEYS = ("direct", "direct_levels", "angle_direct", "angle_direct_levels")

# grid length, levels, angles, draws, sets, user level, where the night samples are, knots
CASES = [(2, 2, ZS[0], 1, CLEAN, "-1", "none", 2), (65, 3, ZS[1], 2, AEROSOL, "0", "none", 3),
         (129, 16, ZS[2], 3, CLOUD, "L", "some", 9), (257, 2, ZS[3], 1, BOTH, "1", "last_chunk", 2),
         (65, 16, ZS[4], 2, ALL, "L-1", "last_chunk", 3), (129, 3, ZS[3], 3, ALL, "1", "some", 9),
         (257, 16, ZS[2], 2, ALL, "-1", "all", 3), (2, 3, ZS[4], 1, ALL, "0", "some", 2)]
assert {c[0] for c in CASES} == set(NS) <= set(SOLVER_NS) and {c[1] for c in CASES} == {2, 3, 16}
assert {c[2] for c in CASES} == set(ZS) and {c[3] for c in CASES} == {1, 2, 3}
assert {c[4] for c in CASES} >= {CLEAN, AEROSOL, CLOUD, BOTH, ALL} and {c[5] for c in CASES} == {"-1", "0", "1", "L-1", "L"}
assert {c[6] for c in CASES} == {"none", "some", "last_chunk", "all"} and {c[7] for c in CASES} == {2, 3, 9}


def knot_grid(band, nk):
    """nk knots strictly inside the band -- its first and last points lie in the two constant ranges, the last one reads the
    last segment's value --; with more than two grid points one knot lies exactly on a grid point."""
    x = np.linspace(band.w0 + 0.26 * (band.wn - band.w0), band.w0 + 0.71 * (band.wn - band.w0), nk)
    if band.nw > 2:
        j = 1 if nk > 2 else 0
        x[j] = band.w0 + int(round((x[j] - band.w0) / band.dw)) * band.dw
        w = band.w0 + np.arange(band.nw, dtype=np.uint64).astype(np.float64) * band.dw
        assert np.any(w == x[j])
    assert np.all(np.diff(x) > 0.0) and band.w0 < x[0] and x[-1] < band.wn
    return x


def knot_values(shape, seed):
    """Knots in [0, 1], 0 and 1 among them."""
    v = np.random.default_rng(seed).uniform(0.02, 0.9, shape)
    v.reshape(-1)[0], v.reshape(-1)[-1] = 1.0, 0.0
    return v


def run_zd(pipe, x, sets, mu, wt, gsurf, direct, profiles, gcols=None, gclouds=None, gaer=None, ncol=None):
    """grt_pipeline_run_sky_zeniths_direct -> one dict: run_sky_zeniths()' keys (sky_zenith_support) and the direct ones."""
    gsky, keep = api.make_sky(gclouds or x.gclouds, gaer or x.gaer, x.S, sets)
    gz, keep_z = api.make_zeniths(mu, wt)
    pipe.run_sky_zeniths_direct(gcols or x.gcols, gsky, gz, gsurface=gsurf, direct=direct, profiles=profiles)
    n = x.ncol if ncol is None else ncol
    if profiles:
        return pipe.sky_zenith_direct_profiles(n, keep["nsets"], mu.shape[1])
    return pipe.sky_zenith_direct_fluxes(n, keep["nsets"], mu.shape[1])


def direct_under(pipe, x, sets, mu_k, profiles):
    """grt_pipeline_run_sky_direct of the batch under one angle per column (a night sample's column under 1.0)."""
    g1, keep1 = api.make_columns(under(x.cols, mu_k), MOL_ORDER, cfc_order=(0, 1))
    gsky, keep = api.make_sky(x.gclouds, x.gaer, x.S, sets)
    pipe.run_sky_direct(g1, gsky, profiles=profiles)
    n = keep["nsets"]
    if profiles:
        return dict(pipe.sky_profiles(x.ncol, n), **pipe.sky_direct_profiles(x.ncol, n))
    return dict(fluxes=pipe.sky_fluxes(x.ncol, n), direct=pipe.sky_direct_fluxes(x.ncol, n))


def surface_of(ncol, xa, direct, diffuse):
    return api.make_surface(ncol, albedo=(xa, direct, diffuse))


def check_per_angle(x, B, sets, mu, six_rows, prof, surface_k, ks=None):
    """(1) every day angle's rows of every set, the direct ones included, are grt_pipeline_run_sky_direct's on pipeline B
    under that angle and surface_k(k) (None: B's surface as it is); a night angle's are +0.0; the longwave is run_sky's."""
    for k in range(mu.shape[1]) if ks is None else ks:
        day = mu[:, k] > 0.0
        if surface_k is not None:
            gs, keep_s = surface_k(k)
            B.set_surface(gs)
        one, p1 = direct_under(B, x, sets, mu[:, k], False), direct_under(B, x, sets, mu[:, k], True)
        assert np.array_equal(six_rows["angle_fluxes"][day][:, :, k], one["fluxes"][day][:, :, 6:]), k
        assert np.array_equal(six_rows["angle_direct"][day][:, :, k], one["direct"][day]), k
        assert np.array_equal(six_rows["fluxes"][:, :, :6], one["fluxes"][:, :, :6]), k
        assert np.array_equal(prof["angle_up"][day][:, :, k], p1["sw_up"][day]), k
        assert np.array_equal(prof["angle_down"][day][:, :, k], p1["sw_down"][day]), k
        assert np.array_equal(prof["angle_fluxes"][day][:, :, k], p1["fluxes"][day][:, :, 6:]), k
        assert np.array_equal(prof["angle_direct"][day][:, :, k], p1["direct"][day]), k
        assert np.array_equal(prof["angle_direct_levels"][day][:, :, k], p1["direct_levels"][day]), k
        for key in ("lw_up", "lw_down", "lw_heating"):
            assert np.array_equal(prof[key], p1[key]), (k, key)
        for out in (six_rows, prof):
            for key in [q for q in out if q.startswith("angle_")]:
                assert positive_zero(out[key][~day][:, :, k]), (k, key)


def check_folds(mu, wt, six_rows, prof, user_level):
    """(2) every mean row is the fold of the per-angle rows in the stated order; the direct TOA row of an angle is its down
    TOA row; rows 0, V - 1 and the user level of the per-angle direct levels are the six-row form's three."""
    w = wt if wt is not None else np.ones_like(mu)
    div = 1.0 if wt is not None else float(mu.shape[1])
    assert np.array_equal(six_rows["fluxes"][:, :, 6:], fold(w, six_rows["angle_fluxes"]) / div)
    assert np.array_equal(six_rows["direct"], fold(w, six_rows["angle_direct"]) / div)
    assert np.array_equal(prof["sw_up"], fold(w, prof["angle_up"]) / div)
    assert np.array_equal(prof["sw_down"], fold(w, prof["angle_down"]) / div)
    assert np.array_equal(prof["direct_levels"], fold(w, prof["angle_direct_levels"]) / div)
    assert np.array_equal(prof["direct"], fold(w, prof["angle_direct"]) / div)
    for out in (six_rows, prof):
        assert np.array_equal(out["angle_direct"][..., 0], out["angle_fluxes"][..., 3])
    lv = prof["angle_direct_levels"]
    picked = np.stack([lv[..., 0], lv[..., -1], lv[..., user_level] if user_level >= 0 else np.zeros_like(lv[..., 0])], axis=-1)
    assert np.array_equal(picked, prof["angle_direct"]) and np.array_equal(picked, six_rows["angle_direct"])
    assert np.array_equal(prof["direct"], six_rows["direct"])


def largest(out, c):
    keys = [k for k in ("fluxes", "angle_fluxes", "sw_up", "sw_down", "angle_up", "angle_down") if k in out]
    return max(np.abs(out[k][c][..., 6:] if k == "fluxes" else out[k][c]).max() for k in keys)


def check_close(a, b, ncol, what):
    """(3) the two forms of the pipeline: within LEVEL_TOL of the column's largest flux"""
    keys = [k for k in a if k.startswith("angle_") or k in DIRECT_KEYS + ("sw_up", "sw_down", "fluxes")]
    for c in range(ncol):
        ff = largest(a, c)
        for key in keys:
            pa, pb = (o[key][c][..., 6:] if key == "fluxes" else o[key][c] for o in (a, b))      # (the shortwave's six)
            err = np.max(np.abs(pa - pb))
            print(what, "column", c, key, err, "of", LEVEL_TOL * ff)
            assert err <= LEVEL_TOL * ff, (what, c, key, err, ff)


class Case:
    """The inputs of one shape, its knots (xa [nk]; knots [ncol][Z][nk], another row [ncol][nk] in force on pipeline A, the
    diffuse knots [ncol][nk] of both) and the pipelines."""

    def __init__(self, bands, tables, device, n, V, Z, S, nk, ncol=NCOL):
        self.x = Inputs(bands, tables, device, n, V, S, ncol=ncol)
        self.xa = knot_grid(self.x.swb, nk)
        self.knots = knot_values((ncol, Z, nk), 5 * n + Z)
        self.other = knot_values((ncol, nk), 7 * n + Z)
        self.dif = knot_values((ncol, nk), 11 * n + Z)
        self.gsurf, self.keep_surf = api.make_zenith_surface(self.xa, self.knots)

    def pipeline(self, user_level, spectral, in_force=True, max_columns=None):
        pipe = self.x.pipeline(user_level, spectral, max_columns=max_columns)
        if in_force:
            gs, keep_s = surface_of(self.x.ncol, self.xa, self.other, self.dif)
            pipe.set_surface(gs)
        return pipe

    def surface_k(self, k):
        return surface_of(self.x.ncol, self.xa, self.knots[:, k], self.dif)


@pytest.mark.parametrize("n,V,Z,S,sets,ul,night,nk", CASES,
                         ids=[f"n{n}-V{V}-Z{Z}-S{S}-sets{s}-ul{u}-night_{w}-knots{q}" for n, V, Z, S, s, u, w, q in CASES])
def test_per_angle_rows_folds_and_forms_at_edge_shapes(bands, tables, lib, device, monkeypatch, n, V, Z, S, sets, ul, night, nk):
    """(1), (2), (3) and (5): deterministic mode, fast = 0, three columns."""
    user_level = user_index(ul, V - 1)
    case = Case(bands, tables, device, n, V, Z, S, nk)
    x = case.x
    mu = angles(x.ncol, Z, night, ZN)
    wt = np.array([[0.25 + 0.125 * ((c + 3 * k) % 5) for k in range(Z)] for c in range(x.ncol)])
    A, B, mat = case.pipeline(user_level, False), case.pipeline(user_level, False), case.pipeline(user_level, True)
    _deterministic(lib, True)
    try:
        six_rows = run_zd(A, x, sets, mu, wt, case.gsurf, True, False)
        prof = run_zd(A, x, sets, mu, wt, case.gsurf, True, True)
        assert six_rows["angle_direct"].shape == (x.ncol, len(positions(sets)), Z, 3)
        check_per_angle(x, B, sets, mu, six_rows, prof, case.surface_k)
        check_folds(mu, wt, six_rows, prof, user_level)
        if night == "all":
            assert positive_zero(six_rows["direct"]) and positive_zero(prof["direct_levels"])
        # without weights: the same angles, the sum and one division by Z
        s0, p0 = run_zd(A, x, sets, mu, None, case.gsurf, True, False), run_zd(A, x, sets, mu, None, case.gsurf, True, True)
        assert np.array_equal(s0["angle_direct"], six_rows["angle_direct"])
        assert np.array_equal(p0["angle_direct_levels"], prof["angle_direct_levels"])
        check_folds(mu, None, s0, p0, user_level)
        # the zenith instances of the solver and the shared-layer kernel's instances: the same bits
        for value in ("0", "1"):
            monkeypatch.setenv("GRT_ZENITH_SHARED", value)
            s1 = run_zd(A, x, sets, mu, wt, case.gsurf, True, False)
            only_surface = run_zd(A, x, sets, mu, wt, case.gsurf, False, False)
            only_direct = run_zd(A, x, sets, mu, wt, None, True, False)
            monkeypatch.delenv("GRT_ZENITH_SHARED")
            for key in six_rows:
                assert np.array_equal(s1[key], six_rows[key]), (value, key)
            for key in only_surface:
                assert np.array_equal(only_surface[key], six_rows[key]), (value, key)
            if value == "0":
                direct_zn = only_direct
            for key in only_direct:
                assert np.array_equal(only_direct[key], direct_zn[key]), (value, key)
        # surface = NULL: everything grt_pipeline_run_sky_zeniths also writes has its bits, in both forms
        for p in (False, True):
            old = run_sky_zeniths(A, x.gcols, x.gclouds, x.gaer, S, sets, mu, wt, x.ncol, p)
            new = run_zd(A, x, sets, mu, wt, None, True, p)
            for key in old:
                assert np.array_equal(new[key], old[key]), (p, key)
            # direct = NULL and every (column, angle)'s knots those of the surface in force: likewise
            same, keep_same = api.make_zenith_surface(case.xa, np.repeat(case.other[:, None, :], Z, axis=1))
            new = run_zd(A, x, sets, mu, wt, same, False, p)
            assert not set(new) & set(DIRECT_KEYS)
            for key in old:
                assert np.array_equal(new[key], old[key]), (p, key)
        # two sweeps: the six-row form's rows are the profile form's
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        s2 = run_zd(A, x, sets, mu, wt, case.gsurf, True, False)
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        for key in ("fluxes", "angle_fluxes", "direct", "angle_direct"):
            assert np.array_equal(s2[key], prof[key]), key
        # the materialised form
        check_close(six_rows, run_zd(mat, x, sets, mu, wt, case.gsurf, True, False), x.ncol, "six rows")
        check_close(prof, run_zd(mat, x, sets, mu, wt, case.gsurf, True, True), x.ncol, "profiles")
        sm, pm = run_zd(mat, x, sets, mu, wt, case.gsurf, True, False), run_zd(mat, x, sets, mu, wt, case.gsurf, True, True)
        check_folds(mu, wt, sm, pm, user_level)
    finally:
        _deterministic(lib, False)
    for pipe in (A, B, mat):
        pipe.destroy()
    x.destroy()


@pytest.mark.parametrize("spectral", [False, True])
def test_constant_knots_on_the_creation_time_albedo(bands, tables, lib, device, spectral):
    """(1), repeated with no grt_pipeline_set_surface on either side: a pipeline created with a constant albedo, and that
    constant at every knot -- a constant row is its knots' value exactly (0 w + b)."""
    n, V, Z, S = 65, 7, ZN + 1, 2
    x = Inputs(bands, tables, device, n, V, S)
    x.alb = np.full(n, 0.3125)
    mu = angles(x.ncol, Z, "some", ZN)
    gsurf, keep_surf = api.make_zenith_surface(knot_grid(x.swb, 3), np.full((x.ncol, Z, 3), 0.3125))
    A, B = x.pipeline(2, spectral), x.pipeline(2, spectral)
    _deterministic(lib, True)
    try:
        six_rows, prof = run_zd(A, x, ALL, mu, None, gsurf, True, False), run_zd(A, x, ALL, mu, None, gsurf, True, True)
        if not spectral:
            check_per_angle(x, B, ALL, mu, six_rows, prof, None)
        else:
            # (the materialised form's run_sky_direct averages the spectra of the draws: the sets of one atmosphere)
            old = run_sky_zeniths(B, x.gcols, x.gclouds, x.gaer, S, ALL, mu, None, x.ncol, True)
            for key in old:
                assert np.array_equal(prof[key], old[key]), key
        check_folds(mu, None, six_rows, prof, 2)
    finally:
        _deterministic(lib, False)
    A.destroy()
    B.destroy()
    x.destroy()


@pytest.mark.parametrize("ul", ["1", "-1"])
def test_a_park_block_of_the_batch_size_takes_one_launch_per_draw_and_angle(bands, tables, lib, device, ul):
    """(5) max_columns = ncol = 2, Z = 3, S = 2: the two-sweep forms run one (draw, angle) per launch."""
    n, V, Z, S = 65, 7, 3, 2
    case = Case(bands, tables, device, n, V, Z, S, 3, ncol=2)
    x = case.x
    mu = angles(2, Z, "none", ZN)
    mu[1, 1] = -0.25
    user_level = user_index(ul, V - 1)
    A, B = case.pipeline(user_level, False, max_columns=2), case.pipeline(user_level, False, max_columns=2)
    _deterministic(lib, True)
    try:
        six_rows, prof = run_zd(A, x, ALL, mu, None, case.gsurf, True, False), run_zd(A, x, ALL, mu, None, case.gsurf, True, True)
        check_per_angle(x, B, ALL, mu, six_rows, prof, case.surface_k)
        check_folds(mu, None, six_rows, prof, user_level)
    finally:
        _deterministic(lib, False)
    A.destroy()
    B.destroy()
    x.destroy()


# ---- (4) against the oracle ------------------------------------------------------------------------------------------ #
def oracle_set_direct(name, orc, lib, band, col, tables, liquid, ice, thickness, x, optics, alb_dir, alb_dif, solar):
    """One set of one column under col["mu0"]: the objects combined as sky_zenith_support.oracle_sky combines them, per draw
    the oracle's solver with alb_dir, alb_dif and direct_beam_model's direct beam, each integrated, then the draws' mean."""
    L = col["p"].size - 1
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    taus, omegas, gs = [tau_gas, tr], [z, om_r], [z, g_r]
    if name in ("aerosol", "both"):
        aer = oracle_aerosol_optics(orc, band, x, optics)
        taus, omegas, gs = taus + [aer[0]], omegas + [aer[1]], gs + [aer[2]]
    draws = [None]
    if name in ("cloud", "both"):
        B = liquid.shape[2]
        w = driver_limits(band.w0, band.dw, band.nw)
        (llo, lhi), (ilo, ihi) = limits(tables, "liquid"), limits(tables, "ice")
        maps = (band_map(llo, lhi, B, B, w), band_map(ilo, ihi, ilo.size, B, w))
        draws = [grid_optics(liquid[j], ice[j], thickness, maps) for j in range(liquid.shape[0])]
    total = None
    for d in draws:
        t, o, g = (taus, omegas, gs) if d is None else (taus + [d[0], d[3]], omegas + [d[1], d[4]], gs + [d[2], d[5]])
        tau, omega, gg = orc.add_optics(t, o, g)
        up, dn = orc.sw_fluxes(omega, gg, tau, col["mu0"], 0.5, alb_dir, alb_dif, col["tsi"], solar)
        beam = direct_beam(tau, omega, gg, col["mu0"], col["tsi"], solar)
        rows = [np.array([orc.integrate_row(r, band.dw) for r in a]) for a in (up, dn, beam)]
        total = rows if total is None else [a + b for a, b in zip(total, rows)]
    up_int, dn_int, direct = (a / float(len(draws)) for a in total)
    return dict(up_int=up_int, dn_int=dn_int, direct=direct)


@pytest.mark.parametrize("name", NAMES)
def test_against_the_oracle(bands, tables, oracle, lib, device, name):
    """(4) one case per set: the oracle's sw_fluxes with alb_dir the angle's row from interpolate_to_grid, and
    direct_beam_model.direct_beam, within LEVEL_TOL of the column's largest flux; both forms of the pipeline."""
    n, V, Z, S, nk, user_level = 129, 7, 2, 2, 3, 3
    sets = {"clean": CLEAN, "aerosol": AEROSOL, "cloud": CLOUD, "both": BOTH}[name]
    case = Case(bands, tables, device, n, V, Z, S, nk, ncol=2)
    x = case.x
    mu = np.array([[0.8, 0.25], [0.1, -0.5]])
    at = positions(sets)[name]
    grid = api.create_spectral_grid(x.swb.w0, x.swb.wn, x.swb.dw)
    dif_rows = host_rows(lib, grid, case.xa, case.dif)
    for spectral in (False, True):
        pipe = case.pipeline(user_level, spectral)
        six_rows, prof = run_zd(pipe, x, sets, mu, None, case.gsurf, True, False), run_zd(pipe, x, sets, mu, None, case.gsurf, True, True)
        for c in range(x.ncol):
            for k in [q for q in range(Z) if mu[c, q] > 0.0]:
                alb_dir = host_rows(lib, grid, case.xa, case.knots[c, k:k + 1])[0]
                w = oracle_set_direct(name, oracle, lib, x.swb, dict(x.cols[c], mu0=mu[c, k]), tables, x.cl["sw_liquid"][c],
                                      x.cl["sw_ice"][c], x.cl["thickness"][c], x.xs[1], x.f[1][c], alb_dir, dif_rows[c], x.solar)
                ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
                want6 = np.concatenate([three(w["up_int"], user_level), three(w["dn_int"], user_level)])
                errs = (np.max(np.abs(six_rows["angle_fluxes"][c, at, k] - want6)),
                        np.max(np.abs(prof["angle_fluxes"][c, at, k] - want6)),
                        np.max(np.abs(prof["angle_up"][c, at, k] - w["up_int"])),
                        np.max(np.abs(prof["angle_down"][c, at, k] - w["dn_int"])),
                        np.max(np.abs(six_rows["angle_direct"][c, at, k] - three(w["direct"], user_level))),
                        np.max(np.abs(prof["angle_direct"][c, at, k] - three(w["direct"], user_level))),
                        np.max(np.abs(prof["angle_direct_levels"][c, at, k] - w["direct"])))
                print(name, spectral, c, k, "errors", errs, "of", LEVEL_TOL * ff)
                assert ff > 0.0 and max(errs) <= LEVEL_TOL * ff, (name, spectral, c, k)
        pipe.destroy()
    x.destroy()


# ---- (6) batch indexing ---------------------------------------------------------------------------------------------- #
def test_batch_indexing(bands, tables, lib, device):
    """A column alone has the bits it has in its batch; any subset of the set mask gives each of its sets the same bits;
    column c's angle k reads its own knots: with two knot rows swapped, exactly those outputs change, and -- the two angles
    of one column under one sun -- they swap."""
    n, V, Z, S, nk = 129, 16, ZN + 1, 2, 9
    case = Case(bands, tables, device, n, V, Z, S, nk)
    x = case.x
    ncol = x.ncol
    mu = angles(ncol, Z, "none", ZN)
    mu[1, 3] = mu[1, 0]                                  # (one column, two angles under one sun)
    mu[2, 2] = -0.1
    wt = np.array([[0.5 + 0.25 * ((c + k) % 3) for k in range(Z)] for c in range(ncol)])
    pipe = case.pipeline(V - 2, False)
    _deterministic(lib, True)
    try:
        full = {p: run_zd(pipe, x, ALL, mu, wt, case.gsurf, True, p) for p in (False, True)}
        for sets in (CLEAN, AEROSOL, CLOUD, BOTH, AEROSOL | CLOUD, CLOUD | BOTH):
            for p in (False, True):
                part = run_zd(pipe, x, sets, mu, wt, case.gsurf, True, p)
                for name, at in positions(sets).items():
                    for key in part:
                        assert np.array_equal(part[key][:, at], full[p][key][:, NAMES.index(name)]), (sets, p, name, key)
        # a column alone (the surface in force has the batch's columns: one of its own for the single column)
        for c in (0, ncol - 1):
            g1, keep1 = api.make_columns([x.cols[c]], MOL_ORDER, cfc_order=(0, 1))
            gc1, keep_c1 = make(tables, {k: v[c:c + 1] for k, v in x.cl.items()})
            ga1, keep_a1 = aerosols_of(tuple(f[c:c + 1] for f in x.f), x.xs)
            gs1, keep_s1 = api.make_zenith_surface(case.xa, case.knots[c:c + 1])
            gin, keep_in = surface_of(1, case.xa, case.other[c:c + 1], case.dif[c:c + 1])
            pipe.set_surface(gin)
            for p in (False, True):
                one = run_zd(pipe, x, ALL, mu[c:c + 1], wt[c:c + 1], gs1, True, p, gcols=g1, gclouds=gc1, gaer=ga1, ncol=1)
                for key in one:
                    assert np.array_equal(one[key][0], full[p][key][c]), (c, p, key)
        gin, keep_in = surface_of(ncol, case.xa, case.other, case.dif)
        pipe.set_surface(gin)
        # swapped knot rows
        for (c1, k1), (c2, k2), swaps in (((1, 0), (1, 3), True), ((0, 1), (2, 4), False)):
            knots = case.knots.copy()
            knots[c1, k1], knots[c2, k2] = case.knots[c2, k2], case.knots[c1, k1]
            gsw, keep_sw = api.make_zenith_surface(case.xa, knots)
            for p in (False, True):
                got = run_zd(pipe, x, ALL, mu, wt, gsw, True, p)
                for key in [q for q in got if q.startswith("angle_") and "direct" not in q]:
                    a, b = got[key], full[p][key]
                    changed = np.zeros(a.shape[:1] + a.shape[2:3], dtype=bool)
                    changed[c1, k1] = changed[c2, k2] = True
                    for c in range(ncol):
                        for k in range(Z):
                            equal = np.array_equal(a[c, :, k], b[c, :, k])
                            assert equal != changed[c, k], (key, c, k, p)
                    if swaps:
                        assert np.array_equal(a[c1, :, k1], b[c2, :, k2]) and np.array_equal(a[c2, :, k2], b[c1, :, k1]), (key, p)
                # (the direct beam does not see the surface)
                for key in [q for q in got if q.startswith("angle_direct")]:
                    assert np.array_equal(got[key], full[p][key]), (key, p)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    x.destroy()


# ---- (7) refusals ---------------------------------------------------------------------------------------------------- #
def test_refused_inputs(bands, tables, lib, device):
    """Each refusal returns GRTCODE_VALUE_ERR with sentinel-filled outputs untouched; afterwards grt_pipeline_run_sky_zeniths
    gives the bits it gave before (the surface in force is as it was)."""
    n, V, Z, S, nk = 65, 3, 3, 2, 3
    case = Case(bands, tables, device, n, V, Z, S, nk)
    x = case.x
    ncol = x.ncol
    pipe = case.pipeline(-1, False)
    mu = angles(ncol, Z, "none", ZN)
    _deterministic(lib, True)
    before = {p: run_sky_zeniths(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, mu, None, ncol, p) for p in (False, True)}
    rows = (4 * V, 2 * (V - 1), 12, Z * 6, Z * 2 * V, 3, V, Z * 3, Z * V)
    sizes = [4 * r * (ncol + 1) for r in rows]
    bufs = [_sentinel(device, k) for k in sizes]

    def call(gsky, gz, gsurf, gdirect, form, gcols=None):
        gz.zenith_fluxes_dev = bufs[3].ptr
        gz.zenith_level_fluxes_dev = bufs[4].ptr if form == "profile" else None
        outs = [b.ptr for b in bufs[:3]] if form == "profile" else [None, None, bufs[2].ptr]
        return lib.grt_pipeline_run_sky_zeniths_direct(pipe.p, C.byref(gcols or x.gcols), None if gsky is None else C.byref(gsky),
                                                       None if gz is None else C.byref(gz),
                                                       None if gsurf is None else C.byref(gsurf),
                                                       None if gdirect is None else C.byref(gdirect), *outs)

    def direct_of(form, which=(0, 1, 2, 3)):
        ptrs = [bufs[5 + k].ptr if k in which and (form == "profile" or k in (0, 2)) else None for k in range(4)]
        return api.GrtZenithDirect(ptrs[0], ptrs[1], ptrs[2], ptrs[3])

    def refused(gsurf=case.gsurf, direct=True, sets=ALL, cos=mu, weight=None, gclouds=x.gclouds, S_=S, which=(0, 1, 2, 3),
                forms=("profile", "six"), levels_in_six=None, gcols=None):
        gsky, ks = api.make_sky(gclouds, x.gaer, S_, sets)
        for form in forms:
            gz, kz = api.make_zeniths(cos, weight)
            gdirect = direct_of(form, which) if direct else None
            if levels_in_six is not None:
                setattr(gdirect, levels_in_six, bufs[6].ptr if levels_in_six == "direct_level_fluxes_dev" else bufs[8].ptr)
            with pytest.raises(api.GrtError) as e:
                api.check(call(gsky, gz, gsurf, gdirect, form, gcols))
            assert e.value.code == api.VALUE_ERR, e.value
        pipe.sync()
        for b, k in zip(bufs, sizes):
            assert np.all(b.to_host((k,)) == -7.25)

    try:
        # ---- everything grt_pipeline_run_sky_zeniths refuses (test_gpu_sky_zenith_shapes.py has the whole list)
        refused(sets=16)
        refused(gclouds=None)
        refused(S_=0)
        m = mu.copy()
        m[1, 1] = 1.0 + 1e-12
        refused(cos=m)
        w = np.ones_like(mu)
        w[0, 2] = -1e-300
        refused(weight=w)
        big, keep_big = api.make_columns(x.cols + x.cols[:1], MOL_ORDER, cfc_order=(0, 1))
        refused(gcols=big)
        # ---- surface and direct both NULL; all four direct outputs NULL; a level output in the six-row form
        refused(gsurf=None, direct=False)
        refused(which=())
        refused(gsurf=None, which=())
        for field in ("direct_level_fluxes_dev", "zenith_direct_level_fluxes_dev"):
            refused(forms=("six",), levels_in_six=field)
        # ---- NS < 2; a NULL grid or albedo array; a grid that is not strictly increasing; a knot outside [0, 1] or not finite
        for bad in (1, 0, -1):
            g, k = api.make_zenith_surface(case.xa, case.knots)
            g.albedo_num_points = bad
            refused(gsurf=g)
            refused(gsurf=g, direct=False)
        for field in ("albedo_grid", "direct_albedo"):
            g, k = api.make_zenith_surface(case.xa, case.knots)
            setattr(g, field, None)
            refused(gsurf=g)
        for xs in (case.xa[[0, 2, 1]], case.xa[[0, 1, 1]], np.array([case.xa[0], np.nan, case.xa[2]])):
            g, k = api.make_zenith_surface(np.array(xs), case.knots)
            refused(gsurf=g)
        for bad, where in ((-1e-300, (0, 0, 0)), (1.0 + 1e-12, (ncol - 1, Z - 1, nk - 1)), (np.nan, (1, 1, 1)), (np.inf, (2, 0, 1))):
            g, k = api.make_zenith_surface(case.xa, case.knots.copy())
            k["direct_albedo"][where] = bad
            refused(gsurf=g)
        # (a night angle's knots are checked too)
        night = mu.copy()
        night[1, 1] = -0.5
        g, k = api.make_zenith_surface(case.xa, case.knots.copy())
        k["direct_albedo"][1, 1, 0] = 1.5
        refused(gsurf=g, cos=night)
        # ---- afterwards: the bits of before, and an accepted call writes what it was given
        for p in (False, True):
            after = run_sky_zeniths(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, mu, None, ncol, p)
            for key in after:
                assert np.array_equal(after[key], before[p][key]), (p, key)
        gsky, ks = api.make_sky(x.gclouds, x.gaer, S, ALL)
        gz, kz = api.make_zeniths(mu)
        api.check(call(gsky, gz, case.gsurf, direct_of("profile", which=(0, 2)), "profile"))
        pipe.sync()
        for at, r in ((5, 3), (7, Z * 3)):
            got = bufs[at].to_host((ncol + 1, 4 * r))
            assert np.all(np.isfinite(got[:ncol])) and np.all(got[:ncol] != -7.25) and np.all(got[ncol] == -7.25)
        for at in (6, 8):
            assert np.all(bufs[at].to_host((sizes[at],)) == -7.25)
    finally:
        _deterministic(lib, False)
    for b in bufs:
        b.free()
    pipe.destroy()
    x.destroy()


# ---- (8) the older entry points ---------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("spectral", [False, True])
def test_existing_entry_points_unchanged(bands, tables, lib, device, spectral):
    """On one pipeline grt_pipeline_run_sky, _run_sky_direct, _run_zeniths and _run_sky_zeniths give the same bits before
    and after the new entry point: the surface in force and every shared buffer survive it."""
    n, V, Z, S, nk = 129, 7, ZN + 1, 2, 9
    case = Case(bands, tables, device, n, V, Z, S, nk)
    x = case.x
    ncol = x.ncol
    mu = angles(ncol, Z, "some", ZN)
    pipe = case.pipeline(2, spectral)

    def older():
        out = {}
        for p in (False, True):
            out["sky", p] = run_sky(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, ncol, p)
            out["direct", p] = direct_under(pipe, x, ALL, np.array([c["mu0"] for c in x.cols]), p)
            out["sky_zeniths", p] = run_sky_zeniths(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, mu, None, ncol, p)
            gz, keep_z = api.make_zeniths(mu)
            pipe.run_zeniths(x.gcols, gz, profiles=p)
            out["zeniths", p] = pipe.zenith_profiles(ncol, Z) if p else dict(zip(("fluxes", "angles"), pipe.zenith_fluxes(ncol, Z)))
        return out

    _deterministic(lib, True)
    try:
        before = older()
        for p in (False, True):
            got = run_zd(pipe, x, ALL, mu, None, case.gsurf, True, p)
            assert np.all(np.isfinite(got["angle_direct"]))
        after = older()
        for key in before:
            for name in before[key]:
                assert np.array_equal(after[key][name], before[key][name]), (key, name)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    x.destroy()


def test_a_pipeline_without_a_shortwave_band(bands, tables, lib, device):
    """It runs the longwave and writes +0.0 to every shortwave and direct output."""
    n, V, Z, S = 65, 3, 3, 2
    case = Case(bands, tables, device, n, V, Z, S, 3)
    x = case.x
    ncol = x.ncol
    mu = angles(ncol, Z, "none", ZN)
    pipe = api.Pipeline(x.go_lw, None, ncol, 0, x.emis, None, None, spectral=False)
    want = api.Pipeline(x.go_lw, None, ncol, 0, x.emis, None, None, spectral=False)
    _deterministic(lib, True)
    try:
        for p in (False, True):
            got = run_zd(pipe, x, ALL, mu, None, case.gsurf, True, p)
            sky = run_sky(want, x.gcols, x.gclouds, x.gaer, S, ALL, ncol, p)
            for key in [k for k in got if k.startswith("angle_") or k in DIRECT_KEYS]:
                assert positive_zero(got[key]), (p, key)
            for key in sky:
                assert np.array_equal(got[key], sky[key]), (p, key)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    want.destroy()
    x.destroy()
