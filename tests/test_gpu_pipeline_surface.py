"""grt_pipeline_set_surface: each column's own surface emissivity, direct and diffuse albedo through every entry point of
the batched pipeline, at the solver kernels' edge shapes.  The expected row of a column is the library's own host
interpolate_to_grid(..., linear_sample, constant_extrapolation); the fluxes are the oracle's, column by column, over that
row (shortwave: orc.sw_fluxes with the direct and the diffuse row).  Then the bit-for-bit identities of the deterministic
mode, what the setter and a run refuse, and the batch driver's -surface-per-column.

Bounds (none is new): the reference's operation order (fast = 0) is held to what test_gpu_solver_shapes.py,
test_gpu_subcolumn_shapes.py and test_gpu_band_profile_shapes.py hold the same kernels to at the same shapes -- LEVEL_TOL
(1e-10) of the column's largest flux for six rows, levels, spectral rows and bins, heating rates within the bound derived
from it; the production arithmetic (fast = 3) to test_gpu_pipeline_production.py's 1e-3 W m-2 and derived heating bound."""
import ctypes as C
import os

import numpy as np
import pytest

from aerosol_model import aerosol_fields, oracle_aerosol_column
from driver_support import batch_flags, build_example, rfmip_like_columns, run_driver, write_grtc_dump
from grtcode_amd import api
from pipeline_support import (CP, GRAVITY, LEVEL_TOL, _sentinel, cached, clouds_for, columns, heating, make,
                              oracle_allsky_levels, oracle_column, six)
from pipeline_support import oracle_cache, solver_bands, tables  # noqa: F401  (module fixtures)
from scenario import Band, MOL_ORDER
from surface_support import host_rows

pytestmark = pytest.mark.gpu

FLUX_TOL = 1e-3                     # W m-2: test_gpu_pipeline_production.py's bound on the production arithmetic
# (grid points, levels, surface knots): every n with both level counts or both knot counts among them
SHAPES = [(2, 2, 2), (3, 16, 5), (129, 2, 5), (257, 16, 2)]
SHAPE_IDS = [f"n{n}-V{V}-NS{ns}" for n, V, ns in SHAPES]
NCOL = 3
CREATE_EMIS, CREATE_ALB = 0.98, 0.2             # the creation-time constants: none of the columns' own values


def surface_knots(band, ns, seed):
    """A surface grid that starts and ends inside the band -- points below it (y[0]), inside it and above it (y[NS-2]) --
    and NCOL columns of knot values in [0, 1], 0 and 1 among them, the last two knots of every column different."""
    span = (band.nw - 1) * band.dw
    x = np.linspace(band.w0 + 0.2 * span, band.w0 + 0.7 * span, ns)
    rng = np.random.default_rng(seed)
    y = rng.uniform(0.05, 0.95, (NCOL, ns))
    y[0, 0], y[1, ns - 1], y[2, ns - 2] = 0.0, 1.0, 1.0
    assert np.all(y[:, ns - 2] != y[:, ns - 1])
    return x, y


class Case:
    """One shape: its bands, columns, each column's knots and expected rows, and the oracle over them."""

    def __init__(self, bands, n, V, ns, lib, orc, cache, fast=0):
        self.pair, self.n, self.V, self.ns, self.lib, self.orc, self.cache, self.fast = bands[n], n, V, ns, lib, orc, cache, fast
        self.cols = columns(V)[:NCOL]
        lwb, swb = self.pair
        self.grids = [api.create_spectral_grid(b.w0, b.wn, b.dw) for b in self.pair]
        self.xe, self.emis = surface_knots(lwb, ns, 11 + n)
        self.xa, self.adir = surface_knots(swb, ns, 12 + n)
        _, self.adif = surface_knots(swb, ns, 13 + n)
        self.rows = dict(emis=host_rows(lib, self.grids[0], self.xe, self.emis),
                         adir=host_rows(lib, self.grids[1], self.xa, self.adir),
                         adif=host_rows(lib, self.grids[1], self.xa, self.adif))
        for r in self.rows.values():
            assert r.min() >= 0.0 and r.max() <= 1.0 and len({row.tobytes() for row in r}) == NCOL
        assert np.any(self.rows["adir"] != self.rows["adif"])

    def open(self, device, ncol=NCOL, user_level=None, spectral=False):
        ul = min(1, self.V - 1) if user_level is None else user_level
        self.user_level = ul
        self.go_lw, _ = self.pair[0].gas_optics(device, self.V, fast=self.fast)
        self.go_sw, grid_sw = self.pair[1].gas_optics(device, self.V, fast=self.fast)
        self.solar = api.create_solar_flux(grid_sw, self.pair[1].files["solar"])
        self.create = (np.full(self.n, CREATE_EMIS), np.full(self.n, CREATE_ALB))
        return self.pipeline(ncol, spectral)

    def pipeline(self, ncol=NCOL, spectral=False, emis=None, alb=None):
        return api.Pipeline(self.go_lw, self.go_sw, ncol, self.user_level, self.create[0] if emis is None else emis,
                            self.create[1] if alb is None else alb, self.solar, spectral=spectral)

    def close(self):
        self.go_lw.destroy()
        self.go_sw.destroy()

    def gcols(self, order=None):
        return api.make_columns([self.cols[c] for c in (order or range(NCOL))], MOL_ORDER, cfc_order=(0, 1))

    def gsurface(self, order=None, diffuse=True, same_diffuse=False):
        o = list(order or range(NCOL))
        dif = (self.adir if same_diffuse else self.adif)[o] if diffuse else None
        return api.make_surface(len(o), emissivity=(self.xe, self.emis[o]), albedo=(self.xa, self.adir[o], dif))

    def solved(self, bi, c, w, dif=True):
        """An oracle result's optics solved over column c's own rows: every level's spectra and integrals."""
        band, col, orc = self.pair[bi], self.cols[c], self.orc
        if bi == 0:
            up, dn = orc.lw_fluxes(band.w0, band.dw, col["t_surf"], col["t_layer"], col["t"], w["tau"], w["omega"],
                                   self.rows["emis"][c])
        else:
            up, dn = orc.sw_fluxes(w["omega"], w["g"], w["tau"], col["mu0"], 0.5, self.rows["adir"][c],
                                   self.rows["adif" if dif else "adir"][c], col["tsi"], self.solar)
        return dict(up=up, dn=dn, up_int=np.array([orc.integrate_row(r, band.dw) for r in up]),
                    dn_int=np.array([orc.integrate_row(r, band.dw) for r in dn]))

    def clear(self, bi, c):
        def make_it():
            w = oracle_column(self.orc, self.lib, self.pair[bi], self.cols[c], bi == 0, emis=self.rows["emis"][c],
                              alb=self.rows["adir"][c], solar=self.solar)
            return self.solved(bi, c, w)
        return cached(self.cache, ("clear", self.n, self.V, self.ns, self.fast, bi, c), make_it)

    def allsky(self, bi, c, tables, liquid, ice, thickness):
        w = oracle_allsky_levels(self.orc, self.lib, self.pair[bi], self.cols[c], bi == 0, tables, liquid, ice, thickness,
                                 self.rows["emis"][c], self.rows["adir"][c], self.solar)
        return self.solved(bi, c, w)

    def aerosol(self, bi, c, x, optics):
        w = oracle_aerosol_column(self.orc, self.lib, self.pair[bi], self.cols[c], bi == 0, x, optics, self.rows["emis"][c],
                                  self.rows["adir"][c], self.solar)
        return self.solved(bi, c, w)


def check_six(got6, w, user_level, tol, what):
    want = six(w["up_int"], w["dn_int"], user_level)
    err = np.max(np.abs(got6 - want))
    print(what, "six rows", err, "bound", tol)
    assert err <= tol, (what, err, tol)


def check_prof(prof, c, key, col, w, tol, heat_tol, what, fast=0):
    up, dn, hr = prof[key + "_up"][c], prof[key + "_down"][c], prof[key + "_heating"][c]
    err = max(np.max(np.abs(up - w["up_int"])), np.max(np.abs(dn - w["dn_int"])))
    print(what, "levels", err, "bound", tol)
    assert err <= tol, (what, err, tol)
    want_hr = heating(w["up_int"], w["dn_int"], col["p"])
    bound = 4.0 * heat_tol * GRAVITY / (CP * 100.0 * (col["p"][1:] - col["p"][:-1])) * 86400.0
    # (fast = 0: test_gpu_solver_shapes.py's bound, with its rounding term; fast = 3: test_gpu_pipeline_production.py's)
    assert np.all(np.abs(hr - want_hr) <= bound + (0.0 if fast else 1e-12 * np.abs(want_hr).max())), what


def tols(w, fast):
    """(flux bound, the flux error the heating bound derives from) of a column and band"""
    if fast:
        return FLUX_TOL, FLUX_TOL
    ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
    assert ff > 0.0
    return LEVEL_TOL * ff, LEVEL_TOL * ff


# ---- 1. parity ------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("fast", [0, 3])
@pytest.mark.parametrize("n,V,ns", SHAPES, ids=SHAPE_IDS)
def test_run_and_run_profiles_match_the_oracle(solver_bands, oracle_cache, oracle, lib, device, n, V, ns, fast):
    case = Case(solver_bands, n, V, ns, lib, oracle, oracle_cache, fast)
    gcols, keep = case.gcols()
    gsurf, keep_s = case.gsurface()
    for spectral in (False, True):
        pipe = case.open(device, spectral=spectral)
        pipe.set_surface(gsurf)
        pipe.run(gcols)
        f = pipe.fluxes(NCOL)
        pipe.run_profiles(gcols)
        prof = pipe.profiles(NCOL)
        for bi, key in enumerate(("lw", "sw")):
            for c, col in enumerate(case.cols):
                w = case.clear(bi, c)
                tol, htol = tols(w, fast)
                what = f"{key} column {c} {'materialised' if spectral else 'fused'} fast {fast}"
                check_six(f[c, 6 * bi: 6 * bi + 6], w, case.user_level, tol, "run " + what)
                check_six(prof["fluxes"][c, 6 * bi: 6 * bi + 6], w, case.user_level, tol, "run_profiles " + what)
                check_prof(prof, c, key, col, w, tol, htol, "run_profiles " + what, fast)
        pipe.destroy()
        case.close()


@pytest.mark.parametrize("n,V,ns", SHAPES, ids=SHAPE_IDS)
def test_allsky_aerosols_and_spectral_match_the_oracle(solver_bands, tables, oracle_cache, oracle, lib, device, n, V, ns):
    case = Case(solver_bands, n, V, ns, lib, oracle, oracle_cache)
    L = V - 1
    gcols, keep = case.gcols()
    gsurf, keep_s = case.gsurface()
    pipe = case.open(device)
    pipe.set_surface(gsurf)
    ul = case.user_level
    cl = clouds_for(case.cols, tables, 30 + V)
    gclouds, keep_c = make(tables, cl)
    # all-sky: both sets
    pipe.run_allsky(gcols, gclouds)
    clear, cloudy = pipe.allsky_fluxes(NCOL)
    # aerosols: a grid across both bands' points
    ax = [np.linspace(b.w0 - 0.5 * b.dw, b.wn - 0.4 * b.dw, 4) for b in case.pair]
    af = [aerosol_fields(NCOL, L, ax[0], 51, lw=True), aerosol_fields(NCOL, L, ax[1], 52, lw=False)]
    gaer, keep_a = api.make_aerosols(lw=(ax[0], af[0]), sw=(ax[1], af[1]))
    pipe.run_aerosols(gcols, gaer)
    clean, aer = pipe.aerosol_fluxes(NCOL)
    # spectral rows with bins (one bin on two points)
    edges = np.array([0, n // 2, n - 1] if n > 2 else [0, 1], dtype=np.int32)
    pipe.run_spectral(gcols, gclouds, lw_edges=edges, sw_edges=edges)
    sp = pipe.spectral(NCOL)
    for bi, key in enumerate(("lw", "sw")):
        band = case.pair[bi]
        for c in range(NCOL):
            w_clear = case.clear(bi, c)
            w_cloud = case.allsky(bi, c, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c], cl["thickness"][c])
            w_aer = case.aerosol(bi, c, ax[bi], af[bi][c])
            tol, _ = tols(w_clear, 0)
            s6 = slice(6 * bi, 6 * bi + 6)
            check_six(clear[c, s6], w_clear, ul, tol, f"run_allsky clear {key} {c}")
            check_six(cloudy[c, s6], w_cloud, ul, tol, f"run_allsky all-sky {key} {c}")
            check_six(clean[c, s6], w_clear, ul, tol, f"run_aerosols clean {key} {c}")
            check_six(aer[c, s6], w_aer, ul, tol, f"run_aerosols aerosol {key} {c}")
            for s, w in enumerate((w_clear, w_cloud)):
                check_six(sp["fluxes"][c, 12 * s + 6 * bi: 12 * s + 6 * bi + 6], w, ul, tol, f"run_spectral {key} {c} set {s}")
                fs = max(np.abs(w["up"]).max(), np.abs(w["dn"]).max())
                want = np.array([w["up"][0], w["up"][-1], w["up"][ul], w["dn"][0], w["dn"][-1], w["dn"][ul]])
                assert np.max(np.abs(sp[key][c, s] - want)) <= LEVEL_TOL * fs, (key, c, s)
                for b in range(edges.size - 1):
                    wb = np.array([oracle.integrate_row(r[edges[b]: edges[b + 1] + 1], band.dw) for r in want])
                    assert np.max(np.abs(sp[key + "_bins"][c, s, :, b] - wb)) <= tol, (key, c, s, b)
    pipe.destroy()
    case.close()


@pytest.mark.parametrize("n,V,ns", SHAPES, ids=SHAPE_IDS)
def test_subcolumns_and_band_profiles_match_the_oracle(solver_bands, tables, oracle_cache, oracle, lib, device, n, V, ns):
    case = Case(solver_bands, n, V, ns, lib, oracle, oracle_cache)
    S = 2
    gcols, keep = case.gcols()
    gsurf, keep_s = case.gsurface()
    pipe = case.open(device)
    pipe.set_surface(gsurf)
    ul = case.user_level
    one = [clouds_for(case.cols, tables, 40 + V + j) for j in range(S)]           # S draws per column and pass
    cl = {k: (np.stack([d[k] for d in one], axis=1) if k != "thickness" else one[0][k]) for k in one[0]}
    gclouds, keep_c = make(tables, cl)
    pipe.run_subcolumns(gcols, gclouds, S)
    clear6, mean6 = pipe.subcolumn_fluxes(NCOL)
    pipe.run_subcolumns(gcols, gclouds, S, profiles=True)
    clear_p, mean_p = pipe.subcolumn_profiles(NCOL)
    edges = np.array([0, n // 2, n - 1], dtype=np.int32) if n > 2 else None     # 2 bins need 3 points
    if edges is not None:
        pipe.run_band_profiles(gcols, None, lw_edges=edges, sw_edges=edges)
        bp = pipe.band_profiles(NCOL)
    for bi, key in enumerate(("lw", "sw")):
        band = case.pair[bi]
        for c, col in enumerate(case.cols):
            w_clear = case.clear(bi, c)
            draws = [case.allsky(bi, c, tables, cl[key + "_liquid"][c, j], cl[key + "_ice"][c, j], cl["thickness"][c])
                     for j in range(S)]
            up, dn = sum(d["up"] for d in draws) / float(S), sum(d["dn"] for d in draws) / float(S)
            w_mean = dict(up_int=np.array([oracle.integrate_row(r, band.dw) for r in up]),
                          dn_int=np.array([oracle.integrate_row(r, band.dw) for r in dn]))
            tol, htol = tols(w_clear, 0)
            s6 = slice(6 * bi, 6 * bi + 6)
            check_six(clear6[c, s6], w_clear, ul, tol, f"run_subcolumns clear {key} {c}")
            check_six(mean6[c, s6], w_mean, ul, tol, f"run_subcolumns mean {key} {c}")
            check_prof(clear_p, c, key, col, w_clear, tol, htol, f"run_subcolumns profiles clear {key} {c}")
            check_prof(mean_p, c, key, col, w_mean, tol, htol, f"run_subcolumns profiles mean {key} {c}")
            if edges is None:
                continue
            for b in range(2):
                for name, spec in (("_up", w_clear["up"]), ("_down", w_clear["dn"])):
                    wb = np.array([oracle.integrate_row(r[edges[b]: edges[b + 1] + 1], band.dw) for r in spec])
                    assert np.max(np.abs(bp[key + name][c, 0, b] - wb)) <= tol, (key, c, b, name)
    pipe.destroy()
    case.close()


# ---- 2. bit identities in the deterministic mode ------------------------------------------------------------------- #
@pytest.fixture
def deterministic(lib):
    api.check(lib.grt_set_deterministic(1))
    yield
    api.check(lib.grt_set_deterministic(-1))


def everything(pipe, gcols, gclouds, ncol):
    """The outputs of run, run_profiles, run_allsky and run_subcolumns (S = 2, both forms) as one list of arrays."""
    pipe.run(gcols)
    out = [pipe.fluxes(ncol)]
    pipe.run_profiles(gcols)
    p = pipe.profiles(ncol)
    out += [p[k] for k in sorted(p)]
    g1, g2 = gclouds
    pipe.run_allsky(gcols, g1)
    out += list(pipe.allsky_fluxes(ncol))
    pipe.run_subcolumns(gcols, g2, 2)
    out += list(pipe.subcolumn_fluxes(ncol))
    pipe.run_subcolumns(gcols, g2, 2, profiles=True)
    for p in pipe.subcolumn_profiles(ncol):
        out += [p[k] for k in sorted(p)]
    return out


def cloud_inputs(case, tables, order=None):
    o = list(order or range(NCOL))
    cols = [case.cols[c] for c in o]
    one = [clouds_for(case.cols, tables, 60 + case.V + j) for j in range(2)]
    two = {k: (np.stack([d[k] for d in one], axis=1) if k != "thickness" else one[0][k]) for k in one[0]}
    assert len(cols) == len(o)
    return (make(tables, {k: v[o] for k, v in one[0].items()}), make(tables, {k: v[o] for k, v in two.items()}))


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("n,V,ns", [(129, 16, 5), (2, 2, 2)], ids=["n129-V16-NS5", "n2-V2-NS2"])
def test_a_column_of_a_batch_is_a_pipeline_of_its_own_rows(solver_bands, tables, oracle_cache, oracle, lib, device,
                                                           deterministic, n, V, ns, spectral):
    """Identity 1 (diffuse_albedo NULL), with the batch in order and permuted."""
    case = Case(solver_bands, n, V, ns, lib, oracle, oracle_cache)
    pipe = case.open(device, spectral=spectral)
    got = {}
    for order in ((0, 1, 2), (2, 0, 1)):
        gcols, keep = case.gcols(order)
        gsurf, keep_s = case.gsurface(order, diffuse=False)
        (g1, k1), (g2, k2) = cloud_inputs(case, tables, order)
        pipe.set_surface(gsurf)
        got[order] = everything(pipe, gcols, (g1, g2), NCOL)
    pipe.destroy()
    for c in range(NCOL):
        own = case.pipeline(1, spectral, emis=case.rows["emis"][c], alb=case.rows["adir"][c])
        gcols, keep = case.gcols((c,))
        (g1, k1), (g2, k2) = cloud_inputs(case, tables, (c,))
        want = everything(own, gcols, (g1, g2), 1)
        own.destroy()
        for order in got:
            j = order.index(c)
            assert same([a[j: j + 1] for a in got[order]], want), (c, order)
    case.close()


@pytest.mark.parametrize("spectral", [False, True])
def test_constant_knots_clearing_and_an_equal_diffuse_albedo(solver_bands, tables, oracle_cache, oracle, lib, device,
                                                             deterministic, spectral):
    """Identities 2, 3 and 4."""
    n, V, ns = 257, 16, 5
    case = Case(solver_bands, n, V, ns, lib, oracle, oracle_cache)
    pipe = case.open(device, spectral=spectral)
    gcols, keep = case.gcols()
    (g1, k1), (g2, k2) = cloud_inputs(case, tables)
    never = everything(pipe, gcols, (g1, g2), NCOL)
    # 2: constant knots equal to the creation-time constants
    const, keep_k = api.make_surface(NCOL, emissivity=(case.xe, np.full((NCOL, ns), CREATE_EMIS)),
                                     albedo=(case.xa, np.full((NCOL, ns), CREATE_ALB)))
    pipe.set_surface(const)
    assert same(everything(pipe, gcols, (g1, g2), NCOL), never)
    # 4: a diffuse albedo equal to the direct one is no diffuse albedo
    gnull, keep_n = case.gsurface(diffuse=False)
    gsame, keep_e = case.gsurface(same_diffuse=True)
    pipe.set_surface(gnull)
    with_null = everything(pipe, gcols, (g1, g2), NCOL)
    assert not same(with_null, never)
    pipe.set_surface(gsame)
    assert same(everything(pipe, gcols, (g1, g2), NCOL), with_null)
    # ... and a different one is not
    gdif, keep_d = case.gsurface()
    pipe.set_surface(gdif)
    assert not same(everything(pipe, gcols, (g1, g2), NCOL), with_null)
    # one band only: the other keeps its creation-time array
    glw, keep_l = api.make_surface(NCOL, emissivity=(case.xe, case.emis))
    pipe.set_surface(glw)
    pipe.run(gcols)
    f = pipe.fluxes(NCOL)
    assert np.array_equal(f[:, 6:], never[0][:, 6:]) and np.array_equal(f[:, :6], with_null[0][:, :6])
    # 3: cleared
    pipe.set_surface(None)
    assert same(everything(pipe, gcols, (g1, g2), NCOL), never)
    pipe.destroy()
    case.close()


# ---- 3. what is refused ------------------------------------------------------------------------------------------------ #
def test_refusals_keep_the_surface_in_force(solver_bands, oracle_cache, oracle, lib, device, deterministic):
    n, V, ns = 129, 2, 5
    case = Case(solver_bands, n, V, ns, lib, oracle, oracle_cache)
    pipe = case.open(device)
    gcols, keep = case.gcols()
    gsurf, keep_s = case.gsurface()
    pipe.set_surface(gsurf)
    pipe.run(gcols)
    first = pipe.fluxes(NCOL)

    def surface(**change):
        f = dict(ncol=NCOL, emissivity_num_points=ns, albedo_num_points=ns, emissivity_grid=case.xe, albedo_grid=case.xa,
                 emissivity=case.emis, direct_albedo=case.adir, diffuse_albedo=case.adif)
        f.update(change)
        arrays = {k: (None if v is None else np.ascontiguousarray(v, dtype=np.float64)) for k, v in f.items()
                  if not isinstance(v, int)}
        ptr = {k: (None if a is None else a.ctypes.data_as(api.c_double_p)) for k, a in arrays.items()}
        return api.GrtSurface(f["ncol"], f["emissivity_num_points"], f["albedo_num_points"], ptr["emissivity_grid"],
                              ptr["albedo_grid"], ptr["emissivity"], ptr["direct_albedo"], ptr["diffuse_albedo"]), arrays

    def off(a, i, v):
        b = np.array(a, dtype=np.float64)
        b.flat[i] = v
        return b

    flat = case.xe.copy()
    flat[2] = flat[1]
    down = case.xa[::-1].copy()
    bad = [dict(ncol=0), dict(ncol=-1), dict(ncol=NCOL + 1),
           dict(emissivity_num_points=1), dict(albedo_num_points=1), dict(emissivity_num_points=-2), dict(albedo_num_points=-1),
           dict(emissivity_grid=None), dict(albedo_grid=None), dict(emissivity=None), dict(direct_albedo=None),
           dict(emissivity_grid=flat), dict(albedo_grid=down),
           dict(emissivity=off(case.emis, 4, 1.0 + 1e-12)), dict(emissivity=off(case.emis, 0, -1e-300)),
           dict(direct_albedo=off(case.adir, 7, 1.5)), dict(diffuse_albedo=off(case.adif, 2, -0.25)),
           dict(emissivity=off(case.emis, 1, np.nan))]
    for change in bad:
        gs, keep_b = surface(**change)
        with pytest.raises(api.GrtError) as e:
            pipe.set_surface(gs)
        assert e.value.code == api.VALUE_ERR, change
        pipe.run(gcols)
        assert np.array_equal(pipe.fluxes(NCOL), first), change                 # the surface before is still in force
    # a run of another ncol: refused, nothing written
    gtwo, keep2 = case.gcols((0, 1))
    buf = _sentinel(device, 2 * 24)
    V2 = 2 * 8 * V
    lev, heat = _sentinel(device, V2), _sentinel(device, V2)
    with pytest.raises(api.GrtError) as e:
        pipe.run(gtwo, out_ptr=buf.ptr)
    assert e.value.code == api.VALUE_ERR
    rc = lib.grt_pipeline_run_profiles(pipe.p, C.byref(gtwo), lev.ptr, heat.ptr, buf.ptr)
    assert rc == api.VALUE_ERR
    pipe.sync()
    assert np.all(buf.to_host(2 * 24) == -7.25) and np.all(lev.to_host(V2) == -7.25) and np.all(heat.to_host(V2) == -7.25)
    # cleared: the two columns run
    pipe.set_surface(None)
    pipe.run(gtwo, out_ptr=buf.ptr)
    pipe.sync()
    assert np.all(buf.to_host(2 * 12) != -7.25)
    for b in (buf, lev, heat):
        b.free()
    pipe.destroy()
    case.close()


def test_the_surface_kernel_is_timed_under_tag_15(solver_bands, oracle_cache, oracle, lib, device):
    case = Case(solver_bands, 257, 2, 2, lib, oracle, oracle_cache)
    pipe = case.open(device)
    api.profile_enable(True)
    try:
        for diffuse, launches in ((True, 3), (False, 2)):
            gsurf, keep_s = case.gsurface(diffuse=diffuse)
            pipe.set_surface(gsurf)
            pipe.sync()
            ms, count = api.profile_read(api.TAG_SURFACE, reset=True)
            assert count == launches and ms > 0.0
    finally:
        api.profile_enable(False)
    pipe.destroy()
    case.close()


# ---- 4. the batch driver ----------------------------------------------------------------------------------------------- #
def test_batch_driver_surface_per_column(tmp_path):
    """-surface-per-column: column i's line is the line of a dump that holds column i alone; without the flag the last
    column's values serve every column, as before."""
    V, ncol = 9, 3
    cols, raw = rfmip_like_columns(ncol, V)
    raw = raw.reshape(ncol, -1).copy()
    scal = V + (V - 1) + V + (V - 1)                    # surface_temperature, emissivity, albedo, zenith angle, irradiance
    for c, (emis, alb, sza) in enumerate(((0.91, 0.31, 20.0), (0.99, 0.05, 55.0), (0.95, 0.6, 70.0))):
        raw[c, scal + 1: scal + 4] = emis, alb, sza
    swb = Band(str(tmp_path / "data"), 1.0, 3000.0, 5.0, 2000, sw=True)
    exe = build_example("rfmip_batch_driver", str(tmp_path / "rfmip_batch_driver"), backtrace=True)
    # the reference's operation order (the first -fast counts): in the production arithmetic the launch shape follows the
    # batch size (test_gpu_pipeline_production.py pins the tile for this comparison; the driver has no such option)
    flags = ["-fast", "0"] + batch_flags(swb, ("1", "1000", "1"), ("1", "3000", "5"), 2)
    env = dict(os.environ, GRT_DETERMINISTIC="1")

    def lines(rows, *extra):
        dump = write_grtc_dump(str(tmp_path / f"columns{len(rows)}_{rows[0]}.bin"), len(rows), V, raw[list(rows)].ravel())
        r = run_driver([exe, swb.par, swb.files["solar"], dump, *flags, *extra], env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        return [l.split(":", 1)[1] for l in r.stdout.splitlines() if l.startswith("col ")]

    per_column = lines((0, 1, 2), "-surface-per-column")
    alone = [lines((c,))[0] for c in range(ncol)]
    assert per_column == alone
    assert len(set(per_column)) == ncol
    # without the flag: the last column's surface everywhere -- each column as a dump of itself and a copy of the last column's
    # surface values
    shared = lines((0, 1, 2))
    assert shared[2] == alone[2] and shared[0] != alone[0] and shared[1] != alone[1]
    keep = raw.copy()
    for c in range(ncol - 1):
        raw[c, scal + 1: scal + 3] = keep[2, scal + 1: scal + 3]
        assert lines((c,))[0] == shared[c]
