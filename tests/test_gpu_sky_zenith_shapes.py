"""grt_pipeline_run_sky_zeniths at the shapes where its kernels and indexing go wrong: grids of two points up to one live
lane past two solver blocks, one-layer columns, 1 angle up to one past two chunks of the shared-layer kernel, 1 to 3 cloud
draws, every set alone and all four, the user level at and next to both ends (levels 1 and L - 1 force the two sweeps),
night samples nowhere, once per column, in the whole last chunk and everywhere, and a park block that holds one (draw,
angle) of the batch.  The references are the oracle column under each angle and, in the deterministic mode,
grt_pipeline_run_sky fed one angle at a time and grt_pipeline_run_zeniths: bit for bit."""
import ctypes as C

import numpy as np
import pytest

from aerosol_model import aerosol_fields
from grtcode_amd import api
from pipeline_support import (LEVEL_TOL, SETS, SOLVER_NS, _deterministic, _sentinel, clouds_for, columns, make, surface,
                              user_index)
from pipeline_support import solver_bands as bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from sky_zenith_support import (AEROSOL, ALL, BOTH, CLEAN, CLOUD, NAMES, aerosols_of, angles, fold, oracle_set, positions,
                                positive_zero, run_sky, run_sky_zeniths, six, under)

pytestmark = pytest.mark.gpu

# (every instance of the shared-layer kernel carries the same number of angles)
ZN = api.GRT_ZENITH_CHUNK
ZS = (1, ZN - 1, ZN, ZN + 1, 2 * ZN + 1)
NS = (2, 65, 129, 257)
NCOL = 3

# grid length, levels, angles, draws, sets, user level, where the night samples are
CASES = [(2, 2, ZS[0], 1, CLEAN, "-1", "none"), (65, 3, ZS[1], 2, AEROSOL, "0", "none"),
         (129, 16, ZS[2], 3, CLOUD, "L", "some"), (257, 2, ZS[3], 1, BOTH, "1", "last_chunk"),
         (65, 16, ZS[4], 2, ALL, "L-1", "last_chunk"), (129, 3, ZS[3], 3, ALL, "1", "some"),
         (257, 16, ZS[2], 2, ALL, "-1", "all"), (2, 3, ZS[4], 1, ALL, "0", "some"),
         (129, 2, ZS[1], 3, BOTH, "-1", "none"), (65, 16, ZS[0], 3, CLOUD | AEROSOL, "1", "none")]
assert {c[0] for c in CASES} == set(NS) <= set(SOLVER_NS) and {c[1] for c in CASES} == {2, 3, 16}
assert {c[2] for c in CASES} == set(ZS) and {c[3] for c in CASES} == {1, 2, 3}
assert {c[4] for c in CASES} >= {CLEAN, AEROSOL, CLOUD, BOTH, ALL} and {c[5] for c in CASES} == {"-1", "0", "1", "L-1", "L"}
assert {c[6] for c in CASES} == {"none", "some", "last_chunk", "all"}


class Inputs:
    """A batch on the grids of n points: columns, surface, S cloud draws per column, an aerosol on a grid that reaches
    past both ends of each band, and the pipelines' ingredients."""

    def __init__(self, bands, tables, device, n, V, S, ncol=NCOL):
        self.lwb, self.swb = bands[n]
        self.V, self.S, self.ncol = V, S, ncol
        self.cols = columns(V)[:ncol]
        self.go_lw, _ = self.lwb.gas_optics(device, V)
        self.go_sw, grid_sw = self.swb.gas_optics(device, V)
        self.emis, _ = surface(n, 1 + n)
        _, self.alb = surface(n, 2 + n)
        self.solar = api.create_solar_flux(grid_sw, self.swb.files["solar"])
        # (from below the band's first point -- above 0 cm-1: the fields scale with the wavenumber -- to past its last)
        self.xs = tuple(np.linspace(max(b.w0 - 2.5 * b.dw, 0.5 * b.w0), b.wn + 2.5 * b.dw, min(b.nw + 3, 9))
                        for b in (self.lwb, self.swb))
        self.f = (aerosol_fields(ncol, V - 1, self.xs[0], 60 + n, lw=True), aerosol_fields(ncol, V - 1, self.xs[1], 61 + n, lw=False))
        draws = [clouds_for(self.cols, tables, 90 + n + V + j) for j in range(S)]
        self.cl = {k: (np.stack([d[k] for d in draws], axis=1) if k in SETS else draws[0][k]) for k in draws[0]}
        self.tables = tables
        self.gcols, self.keep = api.make_columns(self.cols, MOL_ORDER, cfc_order=(0, 1))
        self.gclouds, self.keep_clouds = make(tables, self.cl)
        self.gaer, self.keep_aer = aerosols_of(self.f, self.xs)

    def pipeline(self, user_level, spectral, max_columns=None):
        return api.Pipeline(self.go_lw, self.go_sw, max_columns or self.ncol, user_level, self.emis, self.alb, self.solar,
                            spectral=spectral)

    def zeniths(self, pipe, sets, mu, wt, profiles, gclouds=None, gaer=None):
        return run_sky_zeniths(pipe, self.gcols, gclouds or self.gclouds, gaer or self.gaer, self.S, sets, mu, wt, self.ncol,
                               profiles)

    def sky_under(self, pipe, sets, mu_k, profiles):
        g1, keep1 = api.make_columns(under(self.cols, mu_k), MOL_ORDER, cfc_order=(0, 1))
        return run_sky(pipe, g1, self.gclouds, self.gaer, self.S, sets, self.ncol, profiles)

    def destroy(self):
        self.go_lw.destroy()
        self.go_sw.destroy()


def check_against_run_sky(x, pipe, sets, mu, six_rows, prof, ks, at=None):
    """Angles ks of every column and set (at: of the sets at these places): the six rows and the levels are
    grt_pipeline_run_sky's for that angle, bit for bit; night samples are +0.0; the longwave rows are
    grt_pipeline_run_sky's."""
    at = list(range(len(positions(sets)))) if at is None else list(at)
    for k in ks:
        day = mu[:, k] > 0.0
        one = x.sky_under(pipe, sets, mu[:, k], False)
        assert np.array_equal(six_rows["angle_fluxes"][day][:, at, k], one["fluxes"][day][:, at, 6:]), k
        assert positive_zero(six_rows["angle_fluxes"][~day, :, k]), k
        assert np.array_equal(six_rows["fluxes"][:, :, :6], one["fluxes"][:, :, :6]), k
        p1 = x.sky_under(pipe, sets, mu[:, k], True)
        assert np.array_equal(prof["angle_up"][day][:, at, k], p1["sw_up"][day][:, at]), k
        assert np.array_equal(prof["angle_down"][day][:, at, k], p1["sw_down"][day][:, at]), k
        assert np.array_equal(prof["angle_fluxes"][day][:, at, k], p1["fluxes"][day][:, at, 6:]), k
        assert positive_zero(prof["angle_up"][~day, :, k]) and positive_zero(prof["angle_down"][~day, :, k]), k
        assert positive_zero(prof["angle_fluxes"][~day, :, k]), k
        for key in ("lw_up", "lw_down", "lw_heating"):
            assert np.array_equal(prof[key], p1[key]), (k, key)


def check_folds(mu, wt, six_rows, prof):
    """The mean rows are the fold of the per-angle rows in the stated order (wt None: the sum, then one division by Z)."""
    w = wt if wt is not None else np.ones_like(mu)
    div = 1.0 if wt is not None else float(mu.shape[1])
    assert np.array_equal(six_rows["fluxes"][:, :, 6:], fold(w, six_rows["angle_fluxes"]) / div)
    assert np.array_equal(prof["sw_up"], fold(w, prof["angle_up"]) / div)
    assert np.array_equal(prof["sw_down"], fold(w, prof["angle_down"]) / div)


@pytest.mark.parametrize("n,V,Z,S,sets,ul,night", CASES,
                         ids=[f"n{n}-V{V}-Z{Z}-S{S}-sets{s}-ul{u}-night_{w}" for n, V, Z, S, s, u, w in CASES])
def test_sky_zeniths_at_edge_shapes(bands, tables, oracle, lib, device, monkeypatch, n, V, Z, S, sets, ul, night):
    L = V - 1
    user_level = user_index(ul, L)
    x = Inputs(bands, tables, device, n, V, S)
    ncol = x.ncol
    mu = angles(ncol, Z, night, ZN)
    wt = np.array([[0.25 + 0.125 * ((c + 3 * k) % 5) for k in range(Z)] for c in range(ncol)])
    place = positions(sets)
    fused, mat = x.pipeline(user_level, False), x.pipeline(user_level, True)

    # ---- the default mode against the oracle: the first and last day angle of the first and the last column ---------- #
    got = {pipe: (x.zeniths(pipe, sets, mu, wt, False), x.zeniths(pipe, sets, mu, wt, True)) for pipe in (fused, mat)}
    assert got[fused][0]["angle_fluxes"].shape == (ncol, len(place), Z, 6)
    for c in (0, ncol - 1):
        days = [k for k in range(Z) if mu[c, k] > 0.0]
        for k in sorted({days[0], days[-1]} if days else ()):
            col = dict(x.cols[c], mu0=mu[c, k])
            for name, at in place.items():
                w = oracle_set(name, oracle, lib, x.swb, col, tables, x.cl["sw_liquid"][c], x.cl["sw_ice"][c],
                               x.cl["thickness"][c], x.xs[1], x.f[1][c], x.emis, x.alb, x.solar)
                ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
                assert ff > 0.0
                want6 = six(w["up_int"], w["dn_int"], user_level)
                for pipe in (fused, mat):
                    six_rows, prof = got[pipe]
                    what = (c, k, name, pipe.keep_spectra)
                    errs = (np.max(np.abs(six_rows["angle_fluxes"][c, at, k] - want6)),
                            np.max(np.abs(prof["angle_fluxes"][c, at, k] - want6)),
                            np.max(np.abs(prof["angle_up"][c, at, k] - w["up_int"])),
                            np.max(np.abs(prof["angle_down"][c, at, k] - w["dn_int"])))
                    print(what, "errors", errs, "of", LEVEL_TOL * ff)
                    assert max(errs) <= LEVEL_TOL * ff, what
                    if user_level < 0:
                        assert six_rows["angle_fluxes"][c, at, k, 2] == 0.0 and six_rows["angle_fluxes"][c, at, k, 5] == 0.0

    # ---- the deterministic mode's identities ----------------------------------------------------------------------- #
    _deterministic(lib, True)
    try:
        six_rows, prof = x.zeniths(fused, sets, mu, wt, False), x.zeniths(fused, sets, mu, wt, True)
        check_against_run_sky(x, fused, sets, mu, six_rows, prof, range(Z))
        check_folds(mu, wt, six_rows, prof)
        if night == "all":
            assert positive_zero(six_rows["fluxes"][:, :, 6:]) and np.all(prof["sw_heating"] == 0.0)
        # without weights: the same angles, the sum and one division by Z; Z = 1: grt_pipeline_run_sky
        s0, p0 = x.zeniths(fused, sets, mu, None, False), x.zeniths(fused, sets, mu, None, True)
        assert np.array_equal(s0["angle_fluxes"], six_rows["angle_fluxes"]) and np.array_equal(p0["angle_up"], prof["angle_up"])
        check_folds(mu, None, s0, p0)
        if Z == 1:
            day = mu[:, 0] > 0.0
            assert np.array_equal(s0["fluxes"][day], x.sky_under(fused, sets, mu[:, 0], False)["fluxes"][day])
            one = x.sky_under(fused, sets, mu[:, 0], True)
            for key in one:
                assert np.array_equal(p0[key][day], one[key][day]), key
        # the clean set is grt_pipeline_run_zeniths'
        gz, keep_z = api.make_zeniths(mu, wt)
        fused.run_zeniths(x.gcols, gz)
        zf, za = fused.zenith_fluxes(ncol, Z)
        assert np.array_equal(six_rows["fluxes"][:, 0], zf) and np.array_equal(six_rows["angle_fluxes"][:, 0], za)
        fused.run_zeniths(x.gcols, gz, profiles=True)
        zp = fused.zenith_profiles(ncol, Z)
        for key in zp:
            assert np.array_equal(prof[key][:, 0], zp[key]), key
        # the zenith instances of the solver, and the shared-layer kernel's instances with the joins: the same bits
        for value in ("0", "1"):
            monkeypatch.setenv("GRT_ZENITH_SHARED", value)
            s1 = x.zeniths(fused, sets, mu, wt, False)
            monkeypatch.delenv("GRT_ZENITH_SHARED")
            assert np.array_equal(s1["fluxes"], six_rows["fluxes"]), value
            assert np.array_equal(s1["angle_fluxes"], six_rows["angle_fluxes"]), value
        # two sweeps: the six-row form's rows are the profile form's level rows at 0, L and the user level
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        s2 = x.zeniths(fused, sets, mu, wt, False)
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        assert np.array_equal(s2["angle_fluxes"], prof["angle_fluxes"]) and np.array_equal(s2["fluxes"], prof["fluxes"])
        assert np.array_equal(s2["angle_fluxes"][..., 0], prof["angle_up"][..., 0])
        assert np.array_equal(s2["angle_fluxes"][..., 4], prof["angle_down"][..., L])
        # the materialised form, first and last angle.  (Its grt_pipeline_run_sky averages the spectra of S > 1 draws and
        # integrates the mean; here every draw's rows are integrated and the mean kernel averages them, the order this
        # entry point states: the cloud sets of several draws agree with the oracle above, not bit for bit with run_sky.)
        sm, pm = x.zeniths(mat, sets, mu, wt, False), x.zeniths(mat, sets, mu, wt, True)
        literal = [at for name, at in place.items() if S == 1 or name in ("clean", "aerosol")]
        check_against_run_sky(x, mat, sets, mu, sm, pm, sorted({0, Z - 1}), at=literal)
        check_folds(mu, wt, sm, pm)
    finally:
        _deterministic(lib, False)
    for pipe in (fused, mat):
        pipe.destroy()
    x.destroy()


@pytest.mark.parametrize("ul", ["1", "-1"])
def test_a_park_block_of_the_batch_size_takes_one_launch_per_draw_and_angle(bands, tables, lib, device, ul):
    """max_columns = ncol = 2, Z = 3, S = 2: the park block holds one (draw, angle) of the batch, so the two-sweep forms
    run in six launches in stream order (the profile form always; the six-row form with the user level inside)."""
    n, V, Z, S = 65, 7, 3, 2
    x = Inputs(bands, tables, device, n, V, S, ncol=2)
    mu = angles(2, Z, "none", ZN)
    mu[1, 1] = -0.25
    pipe = x.pipeline(user_index(ul, V - 1), False, max_columns=2)
    _deterministic(lib, True)
    try:
        six_rows, prof = x.zeniths(pipe, ALL, mu, None, False), x.zeniths(pipe, ALL, mu, None, True)
        check_against_run_sky(x, pipe, ALL, mu, six_rows, prof, range(Z))
        check_folds(mu, None, six_rows, prof)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    x.destroy()


def test_sets_inputs_of_nothing_permuted_angles_and_single_columns(bands, tables, lib, device):
    """Deterministic mode, one batch (n = 129, V = 16, Z = 5, S = 2, one night sample per column): any subset of the masks
    gives each set the bits of the four-set run; sets == CLEAN is grt_pipeline_run_zeniths; cloud-free tables make the
    cloud sets the clean and aerosol sets, an aerosol of exact zeros makes the aerosol sets the clean and cloud sets;
    permuting the angles permutes their rows; a column run alone has the bits it has in its batch."""
    n, V, Z, S = 129, 16, ZN + 1, 2
    x = Inputs(bands, tables, device, n, V, S)
    ncol = x.ncol
    mu = angles(ncol, Z, "some", ZN)
    wt = np.array([[0.5 + 0.25 * ((c + k) % 3) for k in range(Z)] for c in range(ncol)])
    pipe = x.pipeline(V - 1, False)
    _deterministic(lib, True)
    try:
        full = {p: x.zeniths(pipe, ALL, mu, wt, p) for p in (False, True)}
        for sets in (CLEAN, AEROSOL, CLOUD, BOTH, AEROSOL | CLOUD, CLOUD | BOTH):
            for p in (False, True):
                part = x.zeniths(pipe, sets, mu, wt, p)
                for name, at in positions(sets).items():
                    for key in part:
                        assert np.array_equal(part[key][:, at], full[p][key][:, NAMES.index(name)]), (sets, p, name, key)
        gz, keep_z = api.make_zeniths(mu, wt)
        pipe.run_zeniths(x.gcols, gz)
        zf, za = pipe.zenith_fluxes(ncol, Z)
        only = x.zeniths(pipe, CLEAN, mu, wt, False)
        assert np.array_equal(only["fluxes"][:, 0], zf) and np.array_equal(only["angle_fluxes"][:, 0], za)
        # cloud-free tables
        clear = [clouds_for(x.cols, tables, 7 + j, clear=True) for j in range(S)]
        gclear, keep_clear = make(tables, {k: (np.stack([d[k] for d in clear], axis=1) if k in SETS else clear[0][k])
                                           for k in clear[0]})
        # an aerosol of exact zeros
        gzero, keep_zero = aerosols_of(tuple(np.zeros_like(f) for f in x.f), x.xs)
        for p in (False, True):
            a = x.zeniths(pipe, ALL, mu, wt, p, gclouds=gclear)
            b = x.zeniths(pipe, ALL, mu, wt, p, gaer=gzero)
            for key in a:
                assert np.array_equal(a[key][:, 2], a[key][:, 0]) and np.array_equal(a[key][:, 3], a[key][:, 1]), (p, key)
                assert np.array_equal(a[key][:, :2], full[p][key][:, :2]), (p, key)
                assert np.array_equal(b[key][:, 1], b[key][:, 0]) and np.array_equal(b[key][:, 3], b[key][:, 2]), (p, key)
                assert np.array_equal(b[key][:, 0], full[p][key][:, 0]) and np.array_equal(b[key][:, 2], full[p][key][:, 2]), (p, key)
        # permuted angles
        order = np.array([(3 * k + 1) % Z for k in range(Z)])
        assert sorted(order) == list(range(Z))
        for p in (False, True):
            q = x.zeniths(pipe, ALL, mu[:, order], wt[:, order], p)
            for key in ("angle_fluxes",) + (("angle_up", "angle_down") if p else ()):
                assert np.array_equal(q[key], full[p][key][:, :, order]), (p, key)
        # a column alone
        for c in (0, ncol - 1):
            g1, keep1 = api.make_columns([x.cols[c]], MOL_ORDER, cfc_order=(0, 1))
            gc1, keep_c1 = make(tables, {k: v[c:c + 1] for k, v in x.cl.items()})
            ga1, keep_a1 = aerosols_of(tuple(f[c:c + 1] for f in x.f), x.xs)
            for p in (False, True):
                one = run_sky_zeniths(pipe, g1, gc1, ga1, S, ALL, mu[c:c + 1], wt[c:c + 1], 1, p)
                for key in one:
                    assert np.array_equal(one[key][0], full[p][key][c]), (c, p, key)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    x.destroy()


def test_refused_inputs(bands, tables, lib, device):
    """Everything grt_pipeline_run_sky refuses in `sky`, everything grt_pipeline_run_zeniths refuses in `zeniths`, and no
    output at all: GRTCODE_VALUE_ERR, and sentinel-filled outputs stay as they were."""
    n, V, Z, S = 65, 3, 3, 2
    x = Inputs(bands, tables, device, n, V, S)
    ncol, L = x.ncol, V - 1
    pipe = x.pipeline(-1, False)
    mu = angles(ncol, Z, "none", ZN)
    sizes = (4 * 4 * V * (ncol + 1), 4 * 2 * L * (ncol + 1), 4 * 12 * (ncol + 1), 4 * Z * 6 * (ncol + 1),
             4 * Z * 2 * V * (ncol + 1))
    bufs = [_sentinel(device, k) for k in sizes]

    def refused(gcols=None, gclouds=x.gclouds, gaer=x.gaer, S_=S, sets=ALL, cos=mu, weight=None, sky=True, zen=True,
                num_zeniths=None, forms=None):
        gsky, ks = api.make_sky(gclouds, gaer, S_, sets)
        gz, kz = api.make_zeniths(mu if cos is None else cos, weight)
        if cos is None:
            gz.cos_zenith = None
        if num_zeniths is not None:
            gz.num_zeniths = num_zeniths
        for form in forms or ("profile", "six"):
            gz.zenith_fluxes_dev = bufs[3].ptr
            gz.zenith_level_fluxes_dev = bufs[4].ptr if form == "profile" else None
            outs = [b.ptr for b in bufs[:3]] if form == "profile" else [None, None, bufs[2].ptr]
            with pytest.raises(api.GrtError) as e:
                api.check(lib.grt_pipeline_run_sky_zeniths(pipe.p, C.byref(gcols or x.gcols), C.byref(gsky) if sky else None,
                                                           C.byref(gz) if zen else None, *outs))
            assert e.value.code == api.VALUE_ERR, e.value
        pipe.sync()
        for b, k in zip(bufs, sizes):
            assert np.all(b.to_host((k,)) == -7.25)

    # ---- what grt_pipeline_run_sky refuses in sky
    refused(sky=False)
    for stray in (16, ALL | 32, 1 << 31):
        refused(sets=stray)
    for sets in (CLOUD, BOTH, ALL):
        refused(gclouds=None, sets=sets)
    for sets in (AEROSOL, BOTH, ALL):
        refused(gaer=None, sets=sets)
    for bad in (0, -1, api.GRT_MAX_SUBCOLUMNS + 1):
        refused(S_=bad)
        refused(gaer=None, S_=bad, sets=CLOUD)
    for field in SETS + ("thickness", "liquid_band_lo"):
        g, k = make(tables, x.cl)
        setattr(g, field, None)
        refused(gclouds=g)
    g, k = make(tables, x.cl)
    g.num_liquid_bands = 0
    refused(gclouds=g, sets=CLOUD | AEROSOL)
    for field, value in (("lw_num_points", 1), ("sw_num_points", -1), ("lw_grid", None), ("sw_optics", None)):
        g, k = aerosols_of(x.f, x.xs)
        setattr(g, field, value)
        refused(gaer=g)
        refused(gclouds=None, gaer=g, sets=AEROSOL)
    bad_grid = x.xs[0].copy()
    bad_grid[1], bad_grid[2] = bad_grid[2], bad_grid[1]
    g, k = aerosols_of(x.f, (bad_grid, x.xs[1]))
    refused(gaer=g, sets=BOTH)
    big_cols = columns(V)
    big, keep_big = api.make_columns(big_cols, MOL_ORDER, cfc_order=(0, 1))
    refused(gcols=big, cos=angles(len(big_cols), Z, "none", ZN))
    x.gcols.ncol = 0
    refused()
    x.gcols.ncol = ncol
    # ---- what grt_pipeline_run_zeniths refuses in zeniths
    refused(zen=False)
    for bad in (0, -1, api.GRT_MAX_ZENITHS + 1):
        refused(num_zeniths=bad)
    refused(cos=None)
    for bad in (np.nan, 1.0 + 1e-12):
        m = mu.copy()
        m[ncol - 1, Z - 1] = bad
        refused(cos=m)
    for bad in (np.nan, -1e-300):
        w = np.ones_like(mu)
        w[1, 0] = bad
        refused(weight=w)
    # the per-angle level fluxes in the six-row form; no output at all
    gsky, ks = api.make_sky(x.gclouds, x.gaer, S, ALL)
    gz, kz = api.make_zeniths(mu)
    gz.zenith_level_fluxes_dev = bufs[4].ptr
    for outs, angle_six in (([None, None, bufs[2].ptr], bufs[3].ptr), ([None, bufs[1].ptr, None], None)):
        gz.zenith_fluxes_dev = angle_six
        gz.zenith_level_fluxes_dev = bufs[4].ptr if angle_six is not None else None
        with pytest.raises(api.GrtError) as e:
            api.check(lib.grt_pipeline_run_sky_zeniths(pipe.p, C.byref(x.gcols), C.byref(gsky), C.byref(gz), *outs))
        assert e.value.code == api.VALUE_ERR
    pipe.sync()
    for b, k in zip(bufs, sizes):
        assert np.all(b.to_host((k,)) == -7.25)
    # and accepted: the per-angle six rows alone
    gz.zenith_fluxes_dev, gz.zenith_level_fluxes_dev = bufs[3].ptr, None
    api.check(lib.grt_pipeline_run_sky_zeniths(pipe.p, C.byref(x.gcols), C.byref(gsky), C.byref(gz), None, None, None))
    pipe.sync()
    a6 = bufs[3].to_host((ncol + 1, 4, Z, 6))
    assert np.all(np.isfinite(a6[:ncol])) and np.all(a6[:ncol] != -7.25) and np.all(a6[ncol] == -7.25)
    assert all(np.all(b.to_host((k,)) == -7.25) for b, k in list(zip(bufs, sizes))[:3])
    for b in bufs:
        b.free()
    pipe.destroy()
    x.destroy()


def test_a_pipeline_without_a_shortwave_band_zeroes_every_shortwave_output(bands, tables, lib, device):
    n, V, Z, S = 65, 3, 3, 2
    x = Inputs(bands, tables, device, n, V, S)
    ncol = x.ncol
    mu = angles(ncol, Z, "none", ZN)
    pipe = api.Pipeline(x.go_lw, None, ncol, 0, x.emis, None, None, spectral=False)
    want = api.Pipeline(x.go_lw, None, ncol, 0, x.emis, None, None, spectral=False)
    _deterministic(lib, True)
    try:
        for p in (False, True):
            got = x.zeniths(pipe, ALL, mu, None, p)
            sky = run_sky(want, x.gcols, x.gclouds, x.gaer, S, ALL, ncol, p)
            for key in [k for k in got if k.startswith("angle_")]:
                assert positive_zero(got[key]), (p, key)
            for key in sky:
                assert np.array_equal(got[key], sky[key]), (p, key)
            assert positive_zero(got["fluxes"][:, :, 6:])
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    want.destroy()
    x.destroy()
