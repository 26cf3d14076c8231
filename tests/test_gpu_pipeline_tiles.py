"""grt_pipeline_run_sky_tiles: several surface tiles per column -- emissivity, direct and diffuse albedo, skin temperature --
through every sky set on one gas-optics pass, at the shapes where its kernels and indexing go wrong: grids of two points
up to one live lane past two solver blocks, one-layer columns, 1 tile up to one past two chunks of the tile kernels, 1 to
3 cloud draws, every set alone and all four, the user level at and next to both ends (levels 1 and L - 1 force the two
sweeps), no fractions, fractions with a zero entry and fractions that do not sum to one.  The reference of every tile is
the oracle column solved over that tile's interpolated rows and temperature (LEVEL_TOL of the column's largest flux, the
margin test_gpu_sky_zenith_shapes.py holds the same rows to); in the deterministic mode, grt_pipeline_run_sky after
grt_pipeline_set_surface with the tile's knots, bit for bit, and the entry point's other identities."""
import ctypes as C

import numpy as np
import pytest

from aerosol_model import aerosol_fields
from grtcode_amd import api
from pipeline_support import (LEVEL_TOL, SETS, SOLVER_NS, _deterministic, _sentinel, cached, clouds_for, columns, make, six,
                              surface, user_index)
from pipeline_support import oracle_cache, solver_bands as bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from sky_zenith_support import AEROSOL, ALL, BOTH, CLEAN, CLOUD, aerosols_of, positions, positive_zero, run_sky
from surface_tiles_support import (NAMES, fold_tiles, oracle_tile, run_sky_tiles, set_optics, tile_fractions, tile_knots,
                                   tile_rows, tile_temperatures)

pytestmark = pytest.mark.gpu

# (every instance of the tile kernels carries the same number of tiles)
TN = api.GRT_TILE_CHUNK
TS = (1, TN - 1, TN, TN + 1, 2 * TN + 1)
NS = (2, 65, 129, 257)
NCOL, MAX_COLUMNS = 3, 4
BLIND = [3, 4, 5, 9]        # the rows that cannot see the surface: the longwave down at the top, the surface and the user
                            # level, the shortwave down at the top

# grid length, levels, tiles, draws, sets, user level, fractions, knots per tile (longwave, shortwave)
CASES = [(2, 2, TS[0], 1, CLEAN, "-1", None, (2, 3)), (65, 3, TS[1], 2, AEROSOL, "0", "zero", (5, 2)),
         (129, 16, TS[2], 3, CLOUD, "L", "free", (4, 5)), (257, 2, TS[3], 1, BOTH, "1", None, (3, 4)),
         (65, 16, TS[4], 2, ALL, "L-1", "zero", (5, 3)), (129, 3, TS[3], 3, ALL, "1", "free", (2, 5)),
         (257, 16, TS[2], 2, ALL, "-1", None, (4, 2)), (2, 3, TS[4], 1, ALL, "0", "zero", (3, 3)),
         (129, 2, TS[1], 3, BOTH, "-1", "free", (5, 4)), (65, 16, TS[0], 3, CLOUD | AEROSOL, "1", None, (3, 5))]
assert {c[0] for c in CASES} == set(NS) <= set(SOLVER_NS) and {c[1] for c in CASES} == {2, 3, 16}
assert {c[2] for c in CASES} == set(TS) and {c[3] for c in CASES} == {1, 2, 3}
assert {c[4] for c in CASES} >= {CLEAN, AEROSOL, CLOUD, BOTH, ALL} and {c[5] for c in CASES} == {"-1", "0", "1", "L-1", "L"}
assert {c[6] for c in CASES} == {None, "zero", "free"}
IDS = [f"n{n}-V{V}-T{T}-S{S}-sets{s}-ul{u}-f_{f}" for n, V, T, S, s, u, f, k in CASES]


class Inputs:
    """A batch on the grids of n points: columns, the creation-time surface, S cloud draws per column, an aerosol on a grid
    that reaches past both ends of each band, T tiles per column, and the pipelines' ingredients."""

    def __init__(self, bands, tables, device, lib, n, V, S, T, fractions=None, knots=(3, 3), ncol=NCOL, fast=0):
        self.lwb, self.swb = bands[n]
        self.n, self.V, self.S, self.T, self.ncol, self.lib = n, V, S, T, ncol, lib
        self.cols = columns(V)[:ncol]
        self.go_lw, _ = self.lwb.gas_optics(device, V, fast=fast)
        self.go_sw, grid_sw = self.swb.gas_optics(device, V, fast=fast)
        self.emis, _ = surface(n, 1 + n)
        _, self.alb = surface(n, 2 + n)
        self.solar = api.create_solar_flux(grid_sw, self.swb.files["solar"])
        self.xs = tuple(np.linspace(max(b.w0 - 2.5 * b.dw, 0.5 * b.w0), b.wn + 2.5 * b.dw, min(b.nw + 3, 9))
                        for b in (self.lwb, self.swb))
        self.f = (aerosol_fields(ncol, V - 1, self.xs[0], 60 + n, lw=True), aerosol_fields(ncol, V - 1, self.xs[1], 61 + n, lw=False))
        draws = [clouds_for(self.cols, tables, 90 + n + V + j) for j in range(S)]
        self.cl = {k: (np.stack([d[k] for d in draws], axis=1) if k in SETS else draws[0][k]) for k in draws[0]}
        self.tables = tables
        self.gcols, self.keep = api.make_columns(self.cols, MOL_ORDER, cfc_order=(0, 1))
        self.gclouds, self.keep_clouds = make(tables, self.cl)
        self.gaer, self.keep_aer = aerosols_of(self.f, self.xs)
        # the tiles: knots, temperatures, fractions, and every tile's expected rows on the two grids
        self.xe, self.ke, _, _ = tile_knots(self.lwb, knots[0], ncol, T, 700 + n)
        self.xa, _, self.kd, self.kf = tile_knots(self.swb, knots[1], ncol, T, 800 + n)
        self.ts = tile_temperatures(self.cols, T)
        self.fr = tile_fractions(ncol, T, fractions)
        self.rows = dict(emis=tile_rows(lib, self.lwb, self.xe, self.ke), adir=tile_rows(lib, self.swb, self.xa, self.kd),
                         adif=tile_rows(lib, self.swb, self.xa, self.kf))
        for r in self.rows.values():
            assert r.min() >= 0.0 and r.max() <= 1.0
        assert self.rows["emis"].min() == 0.0 and self.rows["adir"].max() == 1.0

    def pipeline(self, user_level, spectral, max_columns=MAX_COLUMNS):
        return api.Pipeline(self.go_lw, self.go_sw, max_columns, user_level, self.emis, self.alb, self.solar, spectral=spectral)

    def gtiles(self, order=None, columns_=None, emissivity=True, albedo=True, fraction=True):
        o = list(range(self.T)) if order is None else list(order)
        cs = list(range(self.ncol)) if columns_ is None else list(columns_)
        pick = lambda a: a[cs][:, o]                                        # noqa: E731
        return api.make_surface_tiles(len(cs), pick(self.ts), fraction=pick(self.fr) if fraction and self.fr is not None else None,
                                      emissivity=(self.xe, pick(self.ke)) if emissivity else None,
                                      albedo=(self.xa, pick(self.kd), pick(self.kf)) if albedo else None)

    def tiles(self, pipe, sets, **kw):
        gt, keep = self.gtiles(**kw)
        ncol = keep["shape"][0]
        return run_sky_tiles(pipe, self.gcols, self.gclouds, self.gaer, self.S, sets, gt, ncol)

    def sky_over_tile(self, pipe, sets, t, emissivity=True, albedo=True):
        """grt_pipeline_run_sky after grt_pipeline_set_surface with tile t's knots, the columns at tile t's temperatures;
        the surface in force is cleared afterwards."""
        gs, keep_s = api.make_surface(self.ncol, emissivity=(self.xe, self.ke[:, t]) if emissivity else None,
                                      albedo=(self.xa, self.kd[:, t], self.kf[:, t]) if albedo else None)
        g1, keep1 = api.make_columns([dict(col, t_surf=self.ts[c, t]) for c, col in enumerate(self.cols)], MOL_ORDER,
                                     cfc_order=(0, 1))
        pipe.set_surface(gs)
        out = run_sky(pipe, g1, self.gclouds, self.gaer, self.S, sets, self.ncol, False)["fluxes"]
        pipe.set_surface(None)
        return out

    def oracle_rows(self, orc, cache, name, c, t, user_level):
        """Tile t of column c in set `name`: the twelve rows of the oracle over the tile's rows and temperature, and the
        largest flux of each band's column."""
        twelve, largest = [], []
        for bi, band in enumerate((self.lwb, self.swb)):
            liquid, ice = (self.cl["lw_liquid"], self.cl["lw_ice"]) if bi == 0 else (self.cl["sw_liquid"], self.cl["sw_ice"])
            draws = cached(cache, ("optics", self.n, self.V, self.S, name, bi, c),
                           lambda: set_optics(name, orc, self.lib, band, self.cols[c], self.tables, liquid[c], ice[c],
                                              self.cl["thickness"][c], self.xs[bi], self.f[bi][c]))
            w = oracle_tile(orc, band, self.cols[c], bi == 0, draws, self.ts[c, t], self.rows["emis"][c, t],
                            self.rows["adir"][c, t], self.rows["adif"][c, t], self.solar)
            twelve.append(six(w["up_int"], w["dn_int"], user_level))
            largest.append(max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max()))
        return np.concatenate(twelve), largest

    def destroy(self):
        self.go_lw.destroy()
        self.go_sw.destroy()


@pytest.mark.parametrize("n,V,T,S,sets,ul,fractions,knots", CASES, ids=IDS)
def test_sky_tiles_at_edge_shapes(bands, tables, oracle_cache, oracle, lib, device, monkeypatch, n, V, T, S, sets, ul,
                                  fractions, knots):
    L = V - 1
    user_level = user_index(ul, L)
    x = Inputs(bands, tables, device, lib, n, V, S, T, fractions, knots)
    ncol = x.ncol
    place = positions(sets)
    fused, mat = x.pipeline(user_level, False), x.pipeline(user_level, True)

    # ---- 1. parity, default mode: every tile of every column and set against the oracle, both forms -------------------- #
    got = {pipe: x.tiles(pipe, sets) for pipe in (fused, mat)}
    assert got[fused]["tiles"].shape == (ncol, len(place), T, 12) and got[fused]["fluxes"].shape == (ncol, len(place), 12)
    for c in range(ncol):
        for name, at in place.items():
            for t in range(T):
                want, largest = x.oracle_rows(oracle, oracle_cache, name, c, t, user_level)
                assert min(largest) > 0.0
                for pipe in (fused, mat):
                    rows = got[pipe]["tiles"][c, at, t]
                    errs = [np.max(np.abs(rows[6 * bi: 6 * bi + 6] - want[6 * bi: 6 * bi + 6])) for bi in (0, 1)]
                    bounds = [LEVEL_TOL * ff for ff in largest]
                    if t in (0, T - 1):
                        print((c, name, t, pipe.keep_spectra), "errors", errs, "of", bounds)
                    assert errs[0] <= bounds[0] and errs[1] <= bounds[1], (c, name, t, pipe.keep_spectra, errs, bounds)
                    if user_level < 0:
                        assert np.all(rows[[2, 5, 8, 11]] == 0.0)
    for pipe in (fused, mat):
        assert np.all(np.isfinite(got[pipe]["fluxes"]))

    # ---- 2. the deterministic mode's identities --------------------------------------------------------------------- #
    _deterministic(lib, True)
    try:
        det = x.tiles(fused, sets)
        # (1) a tile's rows are grt_pipeline_run_sky's over that tile; T = 1 without fractions: the whole output
        for t in sorted({0, T - 1}):
            one = x.sky_over_tile(fused, sets, t)
            assert np.array_equal(det["tiles"][:, :, t], one), t
            if T == 1 and x.fr is None:
                assert np.array_equal(det["fluxes"], one)
        # (2) what cannot see the surface is the same double in every tile
        assert np.array_equal(det["tiles"][:, :, :, BLIND], np.repeat(det["tiles"][:, :, :1, BLIND], T, axis=2))
        assert len({det["tiles"][0, 0, t, :].tobytes() for t in range(T)}) == T
        # (3) permuted tiles
        order = [(3 * k + 1) % T for k in range(T)] if T % 3 else list(range(T))[::-1]
        assert sorted(order) == list(range(T))
        q = x.tiles(fused, sets, order=order)
        assert np.array_equal(q["tiles"], det["tiles"][:, :, order])
        # (4) every set has the bits it has in the four-set run; of a four-set run, each set alone
        full = det if sets == ALL else x.tiles(fused, ALL)
        for name, at in place.items():
            for key in det:
                assert np.array_equal(det[key][:, at], full[key][:, NAMES.index(name)]), (name, key)
        for alone in ((CLEAN, AEROSOL, CLOUD, BOTH) if sets == ALL else ()):
            part = x.tiles(fused, alone)
            for name, at in positions(alone).items():
                for key in part:
                    assert np.array_equal(part[key][:, at], full[key][:, NAMES.index(name)]), (alone, name, key)
        # (5) a column alone
        for c in (0, ncol - 1):
            g1, keep1 = api.make_columns([x.cols[c]], MOL_ORDER, cfc_order=(0, 1))
            gc1, keep_c1 = make(tables, {k: v[c:c + 1] for k, v in x.cl.items()})
            ga1, keep_a1 = aerosols_of(tuple(f[c:c + 1] for f in x.f), x.xs)
            gt1, keep_t1 = x.gtiles(columns_=[c])
            one = run_sky_tiles(fused, g1, gc1, ga1, S, sets, gt1, 1)
            for key in one:
                assert np.array_equal(one[key][0], det[key][c]), (c, key)
        # (6) the mean is the stated fold of the stored tile rows
        assert np.array_equal(det["fluxes"], fold_tiles(x.fr, det["tiles"]))
        # without fractions: the same tile rows, the sum and one division by T
        plain = x.tiles(fused, sets, fraction=False)
        assert np.array_equal(plain["tiles"], det["tiles"]) and np.array_equal(plain["fluxes"], fold_tiles(None, det["tiles"]))
        # two sweeps wherever one would do: the same surface rows, the top's upward flux to rounding
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        s2 = x.tiles(fused, sets)
        one = x.sky_over_tile(fused, sets, T - 1)
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        assert np.array_equal(s2["tiles"][:, :, T - 1], one)
        assert np.array_equal(s2["tiles"][..., :6], det["tiles"][..., :6])
        # the materialised form.  (Its grt_pipeline_run_sky averages the spectra of S > 1 draws and integrates the mean; here
        # every draw's rows are integrated and the mean kernel averages them, the order this entry point states: the cloud
        # sets of several draws agree with the oracle above, not bit for bit with run_sky.)
        dm = x.tiles(mat, sets)
        literal = [at for name, at in place.items() if S == 1 or name in ("clean", "aerosol")]
        for t in sorted({0, T - 1}):
            assert np.array_equal(dm["tiles"][:, literal, t], x.sky_over_tile(mat, sets, t)[:, literal]), t
        assert np.array_equal(dm["fluxes"], fold_tiles(x.fr, dm["tiles"]))
    finally:
        _deterministic(lib, False)
    for pipe in (fused, mat):
        pipe.destroy()
    x.destroy()


def test_a_band_without_knots_takes_the_surface_in_force_which_the_call_leaves_alone(bands, tables, lib, device):
    """Deterministic mode, n = 129, V = 16, T = TN + 1, S = 2, all four sets.  A point count of 0: that band's tiles all take
    the surface in force -- a surface set with grt_pipeline_set_surface, else the creation-time arrays --, so tiles that
    differ only in temperature are a valid call; and a surface set before the call gives grt_pipeline_run_sky the same bits
    after it as before (identity 7)."""
    n, V, T, S = 129, 16, TN + 1, 2
    x = Inputs(bands, tables, device, lib, n, V, S, T, "free", (4, 3))
    ncol = x.ncol
    for spectral in (False, True):
        pipe = x.pipeline(1, spectral)
        _deterministic(lib, True)
        try:
            # no surface in force: the creation-time arrays in the band without knots
            for emissivity, albedo in ((False, True), (True, False), (False, False)):
                got = x.tiles(pipe, ALL, emissivity=emissivity, albedo=albedo)
                for t in (0, T - 1):
                    one = x.sky_over_tile(pipe, ALL, t, emissivity=emissivity, albedo=albedo)
                    at = [0, 1] if spectral else [0, 1, 2, 3]          # (materialised cloud sets of S > 1: another order)
                    assert np.array_equal(got["tiles"][:, at, t], one[:, at]), (spectral, emissivity, albedo, t)
                if not albedo:
                    assert np.array_equal(got["tiles"][..., 6:], np.repeat(got["tiles"][:, :, :1, 6:], T, axis=2))
                assert np.array_equal(got["fluxes"], fold_tiles(x.fr, got["tiles"]))
            # a surface in force: tile T - 1's knots for every column
            gs, keep_s = api.make_surface(ncol, emissivity=(x.xe, x.ke[:, T - 1]), albedo=(x.xa, x.kd[:, T - 1], x.kf[:, T - 1]))
            pipe.set_surface(gs)
            before = run_sky(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, ncol, False)["fluxes"]
            own = x.tiles(pipe, ALL)                                       # tiles with knots of their own in both bands
            after = run_sky(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, ncol, False)["fluxes"]
            assert np.array_equal(before, after)
            bare = x.tiles(pipe, ALL, emissivity=False, albedo=False)      # tiles that differ in temperature alone
            assert np.array_equal(run_sky(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, ncol, False)["fluxes"], before)
            pipe.set_surface(None)
            assert np.array_equal(own["tiles"], x.tiles(pipe, ALL)["tiles"])
            at = [0, 1] if spectral else [0, 1, 2, 3]
            assert np.array_equal(bare["tiles"][:, at, T - 1], own["tiles"][:, at, T - 1])
            assert not np.array_equal(bare["tiles"][:, :, 0], own["tiles"][:, :, 0])
        finally:
            _deterministic(lib, False)
        pipe.destroy()
    x.destroy()


@pytest.mark.parametrize("which", ["longwave", "shortwave"])
def test_a_pipeline_with_one_band_zeroes_the_other_band_s_rows(bands, tables, lib, device, which):
    n, V, T, S = 65, 3, TN + 1, 2
    x = Inputs(bands, tables, device, lib, n, V, S, T, "zero", (3, 3))
    ncol = x.ncol
    lw = which == "longwave"
    for spectral in (False, True):
        pipe = api.Pipeline(x.go_lw if lw else None, None if lw else x.go_sw, MAX_COLUMNS, 1, x.emis if lw else None,
                            None if lw else x.alb, None if lw else x.solar, spectral=spectral)
        mine, other = (slice(0, 6), slice(6, 12)) if lw else (slice(6, 12), slice(0, 6))
        _deterministic(lib, True)
        try:
            got = x.tiles(pipe, ALL)
            assert positive_zero(got["tiles"][..., other]) and positive_zero(got["fluxes"][..., other])
            assert np.all(got["tiles"][..., mine][..., [0, 1]] > 0.0)
            assert np.array_equal(got["fluxes"], fold_tiles(x.fr, got["tiles"]))
            at = [0, 1] if spectral else [0, 1, 2, 3]
            for t in (0, T - 1):
                assert np.array_equal(got["tiles"][:, at, t], x.sky_over_tile(pipe, ALL, t)[:, at]), (spectral, t)
            if not lw:
                # no longwave band: the temperatures are not read and may be NULL
                gt, keep = x.gtiles()
                gt.surface_temperature = None
                again = run_sky_tiles(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, gt, ncol)
                assert np.array_equal(again["tiles"], got["tiles"])
        finally:
            _deterministic(lib, False)
        pipe.destroy()
    x.destroy()


def test_tags_and_one_gas_optics_launch_per_band_whatever_the_number_of_tiles(bands, tables, lib, device):
    """grt_profile_read shows launches under the three new tags, and the production form's gas optics (fast = 3; the line
    kernels' and their gathers' tags) are launched as often per call as grt_pipeline_run_sky's, under each tag: once per
    band, not once per tile."""
    n, V, S = 129, 3, 2
    gas = (api.TAG_GAS_LW, api.TAG_GAS_SW, api.TAG_FAR_LW, api.TAG_FAR_SW)
    new = (api.TAG_TILE_LW, api.TAG_TILE_SW, api.TAG_TILE_MEAN)
    counts = {}
    api.profile_enable(True)
    try:
        for T in (1, 2 * TN + 1):
            x = Inputs(bands, tables, device, lib, n, V, S, T, None, (3, 3), fast=3)
            pipe = x.pipeline(-1, False)
            api.profile_read(gas[0], reset=True)                 # (a reset clears the brackets of every tag)
            run_sky(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, x.ncol, False)
            sky = [api.profile_read(tag)[1] for tag in gas]
            assert sum(sky) >= 1 and all(api.profile_read(tag)[1] == 0 for tag in new), sky
            api.profile_read(gas[0], reset=True)
            x.tiles(pipe, ALL)
            counts[T] = [api.profile_read(tag)[1] for tag in gas + new]
            print("T", T, "launches of run_sky", sky, "of run_sky_tiles", counts[T])
            assert counts[T][:4] == sky, (T, counts[T], sky)
            assert counts[T][4] >= 1 and counts[T][5] >= 1 and counts[T][6] == 2 * 4, (T, counts[T])
            pipe.destroy()
            x.destroy()
        assert counts[1][:4] == counts[2 * TN + 1][:4]
    finally:
        api.profile_enable(False)


def test_refused_inputs_and_the_row_past_the_outputs(bands, tables, lib, device):
    """Everything grt_pipeline_run_sky refuses in `sky`, everything grt_pipeline_set_surface refuses in grids, counts and
    values, and the tiles' own rules: GRTCODE_VALUE_ERR, and sentinel-filled outputs stay as they were.  An accepted call
    writes [ncol][N][T][12] and [ncol][N][12] and not the row behind either."""
    n, V, T, S = 65, 3, TN + 1, 2
    x = Inputs(bands, tables, device, lib, n, V, S, T, "free", (3, 4))
    ncol = x.ncol
    pipe = x.pipeline(-1, False)
    sizes = (4 * 12 * (ncol + 1), 4 * T * 12 * (ncol + 1))
    bufs = [_sentinel(device, k) for k in sizes]

    def call(gcols, gsky, gt, out, tile_out):
        if gt is not None:
            gt.tile_fluxes_dev = tile_out
        return lib.grt_pipeline_run_sky_tiles(pipe.p, C.byref(gcols), C.byref(gsky) if gsky is not None else None,
                                              C.byref(gt) if gt is not None else None, out)

    def refused(gcols=None, gclouds=x.gclouds, gaer=x.gaer, S_=S, sets=ALL, sky=True, gt=None, tiles=True, outs=None,
                **fields):
        gsky, ks = api.make_sky(gclouds, gaer, S_, sets)
        if gt is None:
            gt, kt = x.gtiles()
        for k, v in fields.items():
            setattr(gt, k, v)
        out, tile_out = outs if outs is not None else (bufs[0].ptr, bufs[1].ptr)
        with pytest.raises(api.GrtError) as e:
            api.check(call(gcols or x.gcols, gsky if sky else None, gt if tiles else None, out, tile_out))
        assert e.value.code == api.VALUE_ERR, e.value
        pipe.sync()
        for b, k in zip(bufs, sizes):
            assert np.all(b.to_host((k,)) == -7.25)

    def tiles_with(**arrays):
        """the tiles with some arrays replaced (a copy is changed, never x's own)"""
        a = dict(ts=x.ts.copy(), fr=x.fr.copy(), xe=x.xe.copy(), ke=x.ke.copy(), xa=x.xa.copy(), kd=x.kd.copy(), kf=x.kf.copy())
        for k, (index, value) in arrays.items():
            a[k][index] = value
        return api.make_surface_tiles(ncol, a["ts"], fraction=a["fr"], emissivity=(a["xe"], a["ke"]),
                                      albedo=(a["xa"], a["kd"], a["kf"]))

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
    for field in SETS + ("thickness", "liquid_band_lo"):
        g, k = make(tables, x.cl)
        setattr(g, field, None)
        refused(gclouds=g)
    for field, value in (("lw_num_points", 1), ("sw_num_points", -1), ("lw_grid", None), ("sw_optics", None)):
        g, k = aerosols_of(x.f, x.xs)
        setattr(g, field, value)
        refused(gaer=g)
    # ---- ncol outside 1 .. max_columns
    big_cols = columns(V) + columns(V)[:1]
    assert len(big_cols) == MAX_COLUMNS + 1
    big, keep_big = api.make_columns(big_cols, MOL_ORDER, cfc_order=(0, 1))
    refused(gcols=big)
    x.gcols.ncol = 0
    refused()
    x.gcols.ncol = ncol
    # ---- what grt_pipeline_set_surface refuses in grids, counts and values
    for field, value in (("num_emissivity_points", 1), ("num_albedo_points", -1), ("emissivity_grid", None),
                         ("albedo_grid", None), ("emissivity", None), ("direct_albedo", None)):
        refused(**{field: value})
    for key in ("xe", "xa"):
        gt, kt = tiles_with(**{key: (1, getattr(x, key)[0])})          # (not strictly increasing)
        refused(gt=gt)
        gt, kt = tiles_with(**{key: (1, np.nan)})
        refused(gt=gt)
    for key in ("ke", "kd", "kf"):
        for bad in (-1e-300, 1.0 + 1e-12, np.nan):
            gt, kt = tiles_with(**{key: ((ncol - 1, T - 1, 1), bad)})
            refused(gt=gt)
    # ---- the tiles' own rules
    refused(tiles=False)
    for bad in (0, -1, api.GRT_MAX_TILES + 1):
        refused(num_tiles=bad)
    refused(surface_temperature=None)
    for bad in (99.999, 500.001, np.nan):
        gt, kt = tiles_with(ts=((ncol - 1, T - 1), bad))
        refused(gt=gt)
    for bad in (-1e-300, np.nan):
        gt, kt = tiles_with(fr=((1, 0), bad))
        refused(gt=gt)
    refused(outs=(None, None))
    # ---- accepted: both outputs, the mean alone, the tiles alone; fractions may exceed one; nothing behind the last row
    gsky, ks = api.make_sky(x.gclouds, x.gaer, S, ALL)
    gt, kt = tiles_with(fr=((0, 0), 7.5))
    api.check(call(x.gcols, gsky, gt, bufs[0].ptr, bufs[1].ptr))
    pipe.sync()
    both = [b.to_host(shape) for b, shape in zip(bufs, ((ncol + 1, 4, 12), (ncol + 1, 4, T, 12)))]
    for a in both:
        assert np.all(np.isfinite(a[:ncol])) and np.all(a[:ncol] != -7.25) and np.all(a[ncol] == -7.25)
    for b in bufs:
        b.free()
    bufs = [_sentinel(device, k) for k in sizes]
    api.check(call(x.gcols, gsky, gt, bufs[0].ptr, None))
    api.check(call(x.gcols, gsky, gt, None, bufs[1].ptr))
    pipe.sync()
    for b, shape, want in zip(bufs, ((ncol + 1, 4, 12), (ncol + 1, 4, T, 12)), both):
        alone = b.to_host(shape)
        # (the default mode: the gas optics' sums are not in a fixed order from one call to the next)
        assert np.allclose(alone[:ncol], want[:ncol], rtol=1e-9, atol=0.0) and np.all(alone[ncol] == -7.25)
    for b in bufs:
        b.free()
    pipe.destroy()
    x.destroy()
