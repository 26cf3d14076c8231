"""grt_pipeline_run_sky_radiances: grt_pipeline_run_sky's six-row form with the longwave radiances of every set at the
columns' viewing angles.  Against radiance_model.py's restatement fed by the oracle (validated against the oracle's own
solver on the CPU: test_radiance_model.py), fused and materialised, at the edge shapes of the kernel (wave, block and
partial-block grids, one, a full chunk of and one past a chunk of angles, one and three draws, one and three columns); the
bit-for-bit tie to the existing solver through the four stream secants; the bit-for-bit identities of the deterministic
mode; what the entry point refuses; a pipeline without a longwave band; and the production arithmetic.  fast = 0 unless
said otherwise.

Bounds.  Per point: 1e-12 of the row's largest value (one-ulp differences of exp, test_gpu_optics_solvers.py).  An
integrated value against its own spectral row: pipeline_support.assert_trapezoid.  An integrated value against the model's,
where no spectral row leaves (a cloud set of three draws): the per-point bound through the trapezoid's weights, whose sum
is (n - 1) dw, plus assert_trapezoid's own bound with its magnitude at most n dw times the row's largest value.  Brightness
temperatures: 1e-10 K of the formula on the kernel's own radiances.  Production (fast = 3): FLUX_TOL/pi W m-2 sr-1 -- a
radiance error uniform over the hemisphere is pi times that in flux, and both follow from the same bound on tau; the worst
value met on an MI355X: 5.1e-8."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID, aerosol_fields
from grtcode_amd import api, synthetic as syn
from pipeline_support import (SETS, TRAP_ULPS, _deterministic, _sentinel, _setup, assert_trapezoid, clouds_for, make,
                              make_shape_bands, pick, subcolumn_clouds, surface)
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from radiance_model import STREAM_SECANTS, brightness, oracle_radiance_sets, stream_sum
from scenario import MOL_ORDER
from test_gpu_parity_production import record
from test_gpu_pipeline_sky import (ALL, AEROSOL, BOTH, CLEAN, CLOUD, NAMES, aerosols_of, fields, run_sky, shape_grid,
                                   sky_columns)

pytestmark = pytest.mark.gpu

SECANTS = (1.0, 1.5, 14.402613260847248, 1e3)
POINT_TOL = 1e-12            # of the row's largest value
BRIGHTNESS_TOL = 1e-10       # K
V1, UL1, S_MAX = 16, 5, 3
CLOUD_SEED, AEROSOL_SEED = 81, 83


def secants_of(ncol, A):
    """[ncol][A]: the module's four secants, each column starting at another one."""
    return np.array([[SECANTS[(c + k) % len(SECANTS)] for k in range(A)] for c in range(ncol)])


def run_rad(pipe, gcols, gclouds, gaer, S, sets, ncol, secants, spectral=False, bright=False, fluxes=True):
    """-> dict of radiances [ncol][nsets][A][2] and, as asked for, spectral, brightness [ncol][nsets][A][2][n] and
    run_sky()'s fluxes [ncol][nsets][12]."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    secants = np.ascontiguousarray(secants, dtype=np.float64)
    pipe.run_sky_radiances(gcols, gsky, secants, spectral=spectral, brightness=bright, fluxes=fluxes)
    n, A = keep["nsets"], secants.shape[1]
    out = dict(radiances=pipe.sky_radiances(ncol, n, A))
    if spectral:
        out["spectral"] = pipe.sky_spectral_radiances(ncol, n, A)
    if bright:
        out["brightness"] = pipe.sky_brightness(ncol, n, A)
    if fluxes:
        out["fluxes"] = pipe.sky_fluxes(ncol, n)
    return out


def grid_of(band):
    return band.w0 + np.arange(band.nw) * band.dw


def check_points(got, c, k, want, band, what):
    """Set k of column c, every angle and both rows: per point against the model, the integrated value against the
    kernel's own spectral row, the brightness temperature against the formula on the kernel's own radiances."""
    w = grid_of(band)
    for a in range(want["rad"].shape[0]):
        for d in range(2):
            row, ref = got["spectral"][c, k, a, d], want["rad"][a, d]
            err, largest = np.abs(row - ref).max(), np.abs(ref).max()
            print(what, "column", c, "set", k, "angle", a, "row", d, "per point", err, "of", POINT_TOL * largest)
            assert err <= POINT_TOL * largest, (what, c, k, a, d, err, largest)
            assert_trapezoid(got["radiances"][c, k, a, d], row, band.dw, (what, c, k, a, d))
            tb = got["brightness"][c, k, a, d]
            err = np.abs(tb - brightness(row, w)).max()
            assert err <= BRIGHTNESS_TOL, (what, c, k, a, d, err)
            assert np.all(tb[row <= 0.0] == 0.0) and not np.any(np.signbit(tb[row <= 0.0]))


def check_integrated(got, c, k, want, band, what):
    """... the integrated values against the model's (the module's note on this bound)."""
    n, dw = band.nw, band.dw
    tol = (POINT_TOL * (n - 1) * dw + 2.0 * TRAP_ULPS * 2.0 ** -52 * n * dw) * want["largest"]
    err = np.abs(got["radiances"][c, k] - want["integ"])
    print(what, "column", c, "set", k, "integrated: worst", (err / np.maximum(tol, 1e-300)).max(), "of its bound")
    assert np.all(err <= tol), (what, c, k, err, tol)


# ---- 1. edge shapes, against the model fed by the oracle ------------------------------------------------------------------ #
NS = (2, 3, 65, 129, 257)
# (n, V, A, S, ncol): every grid length, level count, angle count, draw count and batch size of the issue's list
SHAPES = [(2, 2, 1, 1, 1), (3, 3, 4, 3, 3), (65, 13, 5, 1, 3), (129, 2, 5, 3, 1), (257, 3, 1, 3, 3), (129, 13, 4, 1, 1),
          (257, 13, 5, 3, 3)]
shape_bands = make_shape_bands(NS, 100.0, 2000.0)


class Shape:
    """The inputs of one edge shape: gas optics of both bands, a surface with 0 and 1 in it, columns, S draws of clouds,
    aerosols on a two-point grid."""

    def __init__(self, shape_bands, tables, device, n, V, S, ncol):
        L = V - 1
        self.lwb, self.swb = shape_bands[n]
        self.cols = [syn.profile(900 + V + c, V) for c in range(3)][:ncol]
        self.go_lw, _ = self.lwb.gas_optics(device, V)
        self.go_sw, grid_sw = self.swb.gas_optics(device, V)
        self.emis, self.alb = surface(n, n + V)
        self.solar = api.create_solar_flux(grid_sw, self.swb.files["solar"])
        self.xs = (shape_grid(self.lwb, "two"), shape_grid(self.swb, "more"))
        self.f = (aerosol_fields(ncol, L, self.xs[0], 60 + n, lw=True), aerosol_fields(ncol, L, self.xs[1], 61 + n, lw=False))
        self.gaer, self.keep_aer = aerosols_of(self.f, self.xs)
        draws = [clouds_for(self.cols, tables, 90 + n + V + j) for j in range(S)]
        self.cl = {k: (np.stack([d[k] for d in draws], axis=1) if k in SETS else draws[0][k]) for k in draws[0]}
        self.gclouds, self.keep_clouds = make(tables, self.cl)
        self.gcols, self.keep = api.make_columns(self.cols, MOL_ORDER, cfc_order=(0, 1))

    def pipeline(self, spectral, max_columns=3, user_level=-1):
        return api.Pipeline(self.go_lw, self.go_sw, max_columns, user_level, self.emis, self.alb, self.solar,
                            spectral=spectral)

    def model(self, oracle, lib, tables, c, secants, clouds=True, aerosols=True):
        cl = self.cl
        return oracle_radiance_sets(oracle, lib, self.lwb, self.cols[c], tables, cl["lw_liquid"][c] if clouds else None,
                                    cl["lw_ice"][c] if clouds else None, cl["thickness"][c], self.xs[0],
                                    self.f[0][c] if aerosols else None, self.emis, secants)

    def destroy(self):
        self.go_lw.destroy()
        self.go_sw.destroy()


@pytest.mark.parametrize("n,V,A,S,ncol", SHAPES, ids=[f"n{n}-V{V}-A{A}-S{S}-c{c}" for n, V, A, S, c in SHAPES])
def test_edge_shapes(shape_bands, tables, oracle, lib, device, n, V, A, S, ncol):
    sh = Shape(shape_bands, tables, device, n, V, S, ncol)
    sec = secants_of(ncol, A)
    want = [sh.model(oracle, lib, tables, c, sec[c]) for c in range(ncol)]
    assert all(np.all(w["largest"][:, 0] > 0.0) for ws in want for w in ws)
    for spectral in (False, True):
        what = f"spectral={spectral}"
        pipe = sh.pipeline(spectral)
        got = run_rad(pipe, sh.gcols, sh.gclouds, sh.gaer, S, ALL, ncol, sec)
        assert got["radiances"].shape == (ncol, 4, A, 2)
        for c in range(ncol):
            for k in range(4):
                check_integrated(got, c, k, want[c][k], sh.lwb, what)
        # every point: all four sets with one draw; the two sets without clouds otherwise
        sets, ks = (ALL, (0, 1, 2, 3)) if S == 1 else (AEROSOL, (0, 1))
        pts = run_rad(pipe, sh.gcols, sh.gclouds if S == 1 else None, sh.gaer, S, sets, ncol, sec, spectral=True, bright=True)
        assert pts["spectral"].shape == (ncol, len(ks), A, 2, n)
        for c in range(ncol):
            for j, k in enumerate(ks):
                check_points(pts, c, j, want[c][k], sh.lwb, what)
                check_integrated(pts, c, j, want[c][k], sh.lwb, what)
        pipe.destroy()
    sh.destroy()


# ---- 2. the four stream secants are the solver, bit for bit ---------------------------------------------------------------- #
@pytest.mark.parametrize("spectral", [False, True])
def test_stream_secants_are_the_solvers_fluxes(shape_bands, tables, lib, device, spectral):
    """((0 + c2[0] R_0) + c2[1] R_1) + c2[2] R_2) + c2[3] R_3 per point is the upward flux at the top and the downward flux at
    the surface of the same pipeline: the materialised form's through grt_pipeline_views, the fused form's through
    grt_pipeline_run_spectral; the clean set and the cloud set of one draw."""
    n, V, ncol = 129, 13, 3
    sh = Shape(shape_bands, tables, device, n, V, 1, ncol)
    pipe = sh.pipeline(spectral)
    sec = np.tile(np.array(STREAM_SECANTS), (ncol, 1))
    _deterministic(lib, True)
    try:
        for sets, k in ((CLEAN, 0), (CLOUD, 1)):
            got = run_rad(pipe, sh.gcols, sh.gclouds if k else None, None, 1, sets, ncol, sec, spectral=True)
            if spectral:
                v = pipe.views(0)
                up = api.device_to_host(device, v["flux_up"], (ncol, V, n))[:, 0]
                dn = api.device_to_host(device, v["flux_down"], (ncol, V, n))[:, V - 1]
            else:
                gcl, keep_cl = make(tables, {key: (a[:, 0] if key in SETS else a) for key, a in sh.cl.items()})
                pipe.run_spectral(sh.gcols, gcl if k else None)
                rows = pipe.spectral(ncol)["lw"]
                up, dn = rows[:, k, 0], rows[:, k, 4]
            assert np.all(up > 0.0)
            for c in range(ncol):
                assert np.array_equal(stream_sum(got["spectral"][c, k, :, 0]), up[c]), (sets, c)
                assert np.array_equal(stream_sum(got["spectral"][c, k, :, 1]), dn[c]), (sets, c)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    sh.destroy()


# ---- 3. identities, bit for bit, in the deterministic mode ------------------------------------------------------------------ #
class Case1:
    def __init__(self, tables):
        self.cols = sky_columns(300, V1)
        self.ncol = len(self.cols)
        self.cl = subcolumn_clouds(self.cols, tables, CLOUD_SEED, S_MAX)
        self.f = fields(self.ncol, V1 - 1, AEROSOL_SEED)

    def clouds(self, S):
        return pick(self.cl, subcolumns=range(S))


@pytest.fixture(scope="module")
def case1(tables):
    return Case1(tables)


@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_identities_bit_for_bit(bands, tables, case1, lib, device, S, spectral):
    cols, ncol = case1.cols, case1.ncol
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    gclouds, keep_clouds = make(tables, cl)
    gaer, keep_aer = aerosols_of(case1.f)
    gzero, keep_zero = aerosols_of(tuple(np.zeros_like(f) for f in case1.f))
    clear = clouds_for(cols, tables, CLOUD_SEED, clear=True)
    gclear, keep_clear = make(tables, {k: (np.repeat(v[:, None], 1, axis=1) if k in SETS else v) for k, v in clear.items()})
    sec = secants_of(ncol, 5)
    every = S == 1                       # (the outputs at every point go with one draw per column)
    keys = ("radiances",) + (("spectral", "brightness") if every else ())
    _deterministic(lib, True)
    try:
        full = run_rad(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, spectral=every, bright=every)
        assert np.all(full["radiances"][..., 0] > 0.0) and np.all(np.isfinite(full["radiances"]))
        assert len({full["radiances"][0, k, 0, 0].tobytes() for k in range(4)}) == 4       # the four sets differ
        # every output run_sky also writes is run_sky's
        assert np.array_equal(full["fluxes"], run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, False)["fluxes"])
        # an angle's values do not depend on which other angles, or how many, share the call
        for a in (0, 3, 4):
            one = run_rad(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec[:, a:a + 1], spectral=every, bright=every)
            for key in keys:
                assert np.array_equal(one[key][:, :, 0], full[key][:, :, a]), (key, a)
        four = run_rad(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec[:, 1:5])
        assert np.array_equal(four["radiances"], full["radiances"][:, :, 1:5])
        # a column alone is the column in the batch
        for c in (0, ncol - 1):
            g1, k1 = api.make_columns([cols[c]], MOL_ORDER, cfc_order=(0, 1))
            gc1, kc1 = make(tables, pick(cl, columns=[c]))
            ga1, ka1 = aerosols_of(tuple(np.ascontiguousarray(f[[c]]) for f in case1.f))
            alone = run_rad(pipe, g1, gc1, ga1, S, ALL, 1, sec[[c]], spectral=every, bright=every)
            for key in keys + ("fluxes",):
                assert np.array_equal(alone[key][0], full[key][c]), (key, c)
        # an aerosol of zeros: the aerosol sets are the clean and the cloud sets
        z = run_rad(pipe, gcols, gclouds, gzero, S, ALL, ncol, sec, spectral=every, bright=every)
        for key in keys:
            assert np.array_equal(z[key][:, 1], z[key][:, 0]) and np.array_equal(z[key][:, 3], z[key][:, 2]), key
            assert np.array_equal(z[key][:, [0, 2]], full[key][:, [0, 2]]), key
        # cloud-free tables (one draw): the cloud sets are the clean and the aerosol sets
        nc = run_rad(pipe, gcols, gclear, gaer, 1, ALL, ncol, sec, spectral=True, bright=True)
        for key in ("radiances", "spectral", "brightness"):
            assert np.array_equal(nc[key][:, 2], nc[key][:, 0]) and np.array_equal(nc[key][:, 3], nc[key][:, 1]), key
        assert np.array_equal(nc["radiances"][:, [0, 1]], full["radiances"][:, [0, 1]])
        # without fluxes: the radiances unchanged, no flux buffer touched, and a night column is no error
        fill = np.full(pipe.buffers["sky"].nbytes // 8, -7.25)
        api.check(lib.grt_host_to_device(device, pipe.buffers["sky"].ptr, fill.ctypes.data_as(C.c_void_p),
                                         C.c_size_t(fill.nbytes)))
        night = [dict(c, mu0=-0.2) for c in cols]
        gnight, keep_night = api.make_columns(night, MOL_ORDER, cfc_order=(0, 1))
        for g in (gcols, gnight):
            alone = run_rad(pipe, g, gclouds, gaer, S, ALL, ncol, sec, spectral=every, bright=every, fluxes=False)
            for key in keys:
                assert np.array_equal(alone[key], full[key]), key
            assert np.all(pipe.buffers["sky"].to_host((fill.size,)) == -7.25)
        with pytest.raises(api.GrtError):                    # (with fluxes the night column is run_sky's error)
            run_rad(pipe, gnight, gclouds, gaer, S, ALL, ncol, sec)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_radiances_alone_launch_no_solver(bands, tables, case1, lib, device):
    """fluxes_dev NULL: the longwave gas optics and the radiance kernel, and nothing of the flux solvers or the shortwave."""
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, case1.clouds(S))
    gaer, keep_aer = aerosols_of(case1.f)
    idle = (api.TAG_GAS_SW, api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_AEROSOL_LW, api.TAG_AEROSOL_SW, api.TAG_ALLSKY_LW,
            api.TAG_ALLSKY_SW, api.TAG_SKY_LW, api.TAG_SKY_SW)
    api.profile_enable(True)
    try:
        api.profile_read(api.TAG_RADIANCE, reset=True)
        run_rad(pipe, gcols, gclouds, gaer, S, ALL, ncol, secants_of(ncol, 5), fluxes=False)
        counts = {tag: api.profile_read(tag)[1] for tag in idle}
        assert all(v == 0 for v in counts.values()), counts
        assert api.profile_read(api.TAG_RADIANCE)[1] == 4 and api.profile_read(api.TAG_GAS_LW)[1] >= 1
        run_rad(pipe, gcols, gclouds, gaer, S, ALL, ncol, secants_of(ncol, 5))
        assert api.profile_read(api.TAG_RADIANCE)[1] == 8 and api.profile_read(api.TAG_SKY_SW)[1] >= 1
    finally:
        api.profile_enable(False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 4. refusals, and a pipeline without a longwave band --------------------------------------------------------------------- #
def test_refused_inputs(bands, tables, case1, lib, device):
    cols, ncol, S, A = case1.cols, case1.ncol, 3, 5
    n = bands[0].nw
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    sizes = (4 * A * 2 * (ncol + 1), 4 * A * 2 * n * (ncol + 1), 4 * A * 2 * n * (ncol + 1), 4 * 12 * (ncol + 1))
    bufs = [_sentinel(device, k) for k in sizes]
    rad, spec, tb, fx = (b.ptr for b in bufs)
    good = secants_of(ncol, A)
    tags = (api.TAG_GAS_LW, api.TAG_GAS_SW, api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_AEROSOL_LW, api.TAG_AEROSOL_SW,
            api.TAG_ALLSKY_LW, api.TAG_ALLSKY_SW, api.TAG_SKY_LW, api.TAG_SKY_SW, api.TAG_SUBCOLUMN_MEAN, api.TAG_RADIANCE)

    def struct(secants=good, A_=None, out=rad, spectral=None, bright=None):
        m = None if secants is None else np.ascontiguousarray(secants, dtype=np.float64)
        g = api.GrtRadiances(A if A_ is None else A_, None if m is None else m.ctypes.data_as(C.POINTER(C.c_double)), out,
                             spectral, bright)
        g.keep = m
        return g

    def refused(gc, gcl, ga, S_, sets, grad, sky=True, fluxes=(fx, None)):
        gsky, ks = api.make_sky(gcl, ga, S_, sets)
        for f in fluxes:
            with pytest.raises(api.GrtError) as e:
                api.check(lib.grt_pipeline_run_sky_radiances(pipe.p, C.byref(gc), C.byref(gsky) if sky else None,
                                                             C.byref(grad) if grad is not None else None, f))
            assert e.value.code == api.VALUE_ERR, (sets, e.value)
        pipe.sync()
        for b, k in zip(bufs, sizes):
            assert np.all(b.to_host((k,)) == -7.25)

    gclouds, kc = make(tables, cl)
    gone, k1 = make(tables, case1.clouds(1))
    gaer, ka = aerosols_of(case1.f)
    api.profile_enable(True)
    try:
        api.profile_read(tags[0], reset=True)
        # the radiance inputs and outputs
        refused(gcols, gclouds, gaer, S, ALL, None)
        refused(gcols, gclouds, gaer, S, ALL, struct(out=None))
        refused(gcols, gclouds, gaer, S, ALL, struct(out=None, spectral=spec, bright=tb))
        refused(gcols, gclouds, gaer, S, ALL, struct(secants=None))
        for bad in (0, -1, api.GRT_MAX_VIEW_ANGLES + 1):
            refused(gcols, gclouds, gaer, S, ALL, struct(secants=np.ones((ncol, max(bad, 1))), A_=bad))
        for bad in (float("nan"), float("inf"), -float("inf"), 0.999999, 0.0, -2.0):
            for at in ((0, 0), (ncol - 1, A - 1)):
                m = good.copy()
                m[at] = bad
                refused(gcols, gclouds, gaer, S, ALL, struct(secants=m))
        # the outputs at every point with a cloud set of several draws
        refused(gcols, gclouds, gaer, S, ALL, struct(spectral=spec))
        refused(gcols, gclouds, gaer, S, CLOUD, struct(bright=tb))
        refused(gcols, gclouds, gaer, 2, BOTH, struct(spectral=spec, bright=tb))
        # everything grt_pipeline_run_sky refuses
        refused(gcols, gclouds, gaer, S, ALL, struct(), sky=False)
        for stray in (16, ALL | 32, 1 << 31):
            refused(gcols, gclouds, gaer, S, stray, struct())
        for sets in (CLOUD, BOTH, ALL):
            refused(gcols, None, gaer, S, sets, struct())
        for sets in (AEROSOL, BOTH, ALL):
            refused(gcols, gclouds, None, S, sets, struct())
        for bad in (0, -1, api.GRT_MAX_SUBCOLUMNS + 1):
            refused(gcols, gclouds, gaer, bad, ALL, struct())
        for field in SETS[:2] + ("thickness", "liquid_band_lo"):
            g, k = make(tables, cl)
            setattr(g, field, None)
            refused(gcols, g, gaer, S, ALL, struct())
        for field, value in (("lw_num_points", 1), ("lw_grid", None)):
            g, k = aerosols_of(case1.f)
            setattr(g, field, value)
            refused(gcols, gclouds, g, S, ALL, struct())
        big_cols = sky_columns(300, V1, n=4)
        big, keep_big = api.make_columns(big_cols, MOL_ORDER, cfc_order=(0, 1))
        gb, kb = make(tables, subcolumn_clouds(big_cols, tables, CLOUD_SEED, S))
        ab, kab = aerosols_of(fields(4, V1 - 1, AEROSOL_SEED))
        refused(big, gb, ab, S, ALL, struct(secants=secants_of(4, A)))
        gcols.ncol = 0
        refused(gcols, gclouds, gaer, S, ALL, struct())
        gcols.ncol = ncol
        counts = {tag: api.profile_read(tag)[1] for tag in tags}
        assert all(v == 0 for v in counts.values()), counts
    finally:
        api.profile_enable(False)
    # and the call accepted: one draw per column with the outputs at every point, the rows past the batch untouched
    gsky, ks = api.make_sky(gone, gaer, 1, ALL)
    api.check(lib.grt_pipeline_run_sky_radiances(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(struct(spectral=spec, bright=tb)),
                                                 None))
    pipe.sync()
    rows = bufs[0].to_host((ncol + 1, 4, A, 2))
    assert np.all(np.isfinite(rows[:ncol])) and np.all(rows[:ncol, :, :, 0] > 0.0) and np.all(rows[ncol] == -7.25)
    pts = bufs[1].to_host((ncol + 1, 4, A, 2, n))
    assert np.all(np.isfinite(pts[:ncol])) and np.all(pts[ncol] == -7.25)
    temps = bufs[2].to_host((ncol + 1, 4, A, 2, n))
    assert np.all((temps[:ncol, :, :, 0] > 100.0) & (temps[:ncol, :, :, 0] < 400.0)) and np.all(temps[ncol] == -7.25)
    assert np.all(bufs[3].to_host((sizes[3],)) == -7.25)
    for b in bufs:
        b.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_no_longwave_band(bands, tables, case1, lib, device):
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)
    sec = secants_of(ncol, 5)
    sw_only = api.Pipeline(None, go_sw, ncol, UL1, None, alb, solar, spectral=False)
    _deterministic(lib, True)
    try:
        run_rad(sw_only, gcols, gclouds, gaer, S, ALL, ncol, sec)                    # (allocates the buffers)
        buf = sw_only.buffers["sky.radiances"]
        fill = np.full(buf.nbytes // 8, -7.25)                                       # zeros are written, not left
        api.check(lib.grt_host_to_device(device, buf.ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(fill.nbytes)))
        out = run_rad(sw_only, gcols, gclouds, gaer, S, ALL, ncol, sec)
        assert np.all(out["radiances"] == 0.0) and not np.any(np.signbit(out["radiances"]))
        assert np.array_equal(out["fluxes"], run_sky(sw_only, gcols, gclouds, gaer, S, ALL, ncol, False)["fluxes"])
        assert np.all(out["fluxes"][:, :, :6] == 0.0) and np.all(out["fluxes"][:, :, 6] > 0.0)
        assert np.all(run_rad(sw_only, gcols, gclouds, gaer, S, ALL, ncol, sec, fluxes=False)["radiances"] == 0.0)
    finally:
        _deterministic(lib, False)
    sw_only.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 5. the production arithmetic -------------------------------------------------------------------------------------------- #
def test_production_form_matches_the_model(bands, tables, oracle, lib, device):
    """fast = 3 on the 3 000-line band, four columns, all four sets, two draws: the integrated radiances against the model on
    the oracle's tau within FLUX_TOL/pi, and the pipeline's own quadrature identity -- the c2-weighted sum of its
    radiances at the four stream secants against its own flux rows -- to 1e-12 of the flux.  The worst value met on an
    MI355X: 5.1e-8 W m-2 sr-1 against the bound 3.2e-4."""
    FLUX_TOL, S = 1e-3, 2
    bound = FLUX_TOL / math.pi
    cols = sky_columns(320, V1, n=4)
    ncol = len(cols)
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1, fast=3)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, CLOUD_SEED + 1, S)
    gclouds, keep_clouds = make(tables, cl)
    f = fields(ncol, V1 - 1, AEROSOL_SEED + 2)
    gaer, keep_aer = aerosols_of(f)
    sec = np.tile(np.array(STREAM_SECANTS + (1.0, 1.5, 1e3)), (ncol, 1))
    got = run_rad(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec)
    assert go_lw.last_launch()["fast"] == 3
    worst = 0.0
    for c, col in enumerate(cols):
        want = oracle_radiance_sets(oracle, lib, bands[0], col, tables, cl["lw_liquid"][c], cl["lw_ice"][c], cl["thickness"][c],
                                    AEROSOL_GRID, f[0][c], emis, sec[c])
        for k, wk in enumerate(want):
            err = np.abs(got["radiances"][c, k] - wk["integ"]).max()
            worst = max(worst, float(err))
            print("production column", c, "set", NAMES[k], "error", err, "bound", bound)
            for d, row in ((0, 0), (1, 4)):
                flux = got["fluxes"][c, k, row]
                quad = stream_sum(got["radiances"][c, k, :4, d])
                print("  quadrature row", row, abs(quad - flux), "of", 1e-12 * flux)
                assert flux > 0.0 and abs(quad - flux) <= 1e-12 * flux, (c, k, row, quad, flux)
    mode = "deterministic" if os.environ.get("GRT_DETERMINISTIC", "0") not in ("", "0") else "default"
    record("run_sky_radiances." + mode, {"radiances": {"worst": worst, "bound": bound}}, file="parity_pipeline_production.json")
    assert worst <= bound, (worst, bound)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
