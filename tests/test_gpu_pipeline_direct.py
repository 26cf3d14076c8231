"""grt_pipeline_run_sky_direct: grt_pipeline_run_sky's sets with the direct beam of each set's shortwave beside them.
Against direct_beam_model.py's restatement (validated against the oracle on the CPU: test_direct_beam_model.py), fused and
materialised, six-row and profile form; the bit-for-bit identities with grt_pipeline_run_sky and within the new rows;
ordering; batch indexing; edge shapes of the sinks and partial sums; the production arithmetic; missing bands; what the
entry point refuses; and the older entry points before and after it on one pipeline."""
import ctypes as C

import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID, aerosol_fields
from direct_beam_model import oracle_direct_sets, three
from grtcode_amd import api, synthetic as syn
from pipeline_support import (LEVEL_TOL, SETS, _deterministic, _sentinel, _setup, cached, clouds_for, make,
                              make_shape_bands, pick, subcolumn_clouds)
from pipeline_support import bands, oracle_cache, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from test_gpu_pipeline_sky import (ALL, AEROSOL, BOTH, CLEAN, CLOUD, NAMES, aerosols_of, fields, positions, run_sky, same,
                                   shape_grid, sky_columns)

pytestmark = pytest.mark.gpu

V1, UL1, S_MAX = 16, 5, 3
CLOUD_SEED, AEROSOL_SEED = 81, 83
DIRECT_KEYS = ("direct", "direct_levels")


def run_direct(pipe, gcols, gclouds, gaer, S, sets, ncol, profiles):
    """-> run_sky()'s dict, and with it direct [ncol][nsets][3] and (profile form) direct_levels [ncol][nsets][V]."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    pipe.run_sky_direct(gcols, gsky, profiles=profiles)
    n = keep["nsets"]
    if profiles:
        return dict(pipe.sky_profiles(ncol, n), **pipe.sky_direct_profiles(ncol, n))
    return dict(fluxes=pipe.sky_fluxes(ncol, n), direct=pipe.sky_direct_fluxes(ncol, n))


def without_direct(out):
    return {k: v for k, v in out.items() if k not in DIRECT_KEYS}


def check_order(out, profiles):
    """(c): 0 <= direct <= down row by row (a margin of 1e-12 of the down value), and the levels never increase downward."""
    down = out["fluxes"][:, :, 9:12]
    assert np.all(out["direct"] >= 0.0) and np.all(out["direct"] <= down * (1.0 + 1e-12)), np.max(out["direct"] - down)
    if profiles:
        lv = out["direct_levels"]
        assert np.all(lv >= 0.0) and np.all(lv <= out["sw_down"] * (1.0 + 1e-12)), np.max(lv - out["sw_down"])
        assert np.all(lv[..., 1:] <= lv[..., :-1])


def check_direct(out, c, k, want, user_level, profiles, tol, what):
    err = np.max(np.abs(out["direct"][c, k] - three(want["direct"], user_level)))
    print(what, "column", c, "set", k, "direct rows", err, "of", tol)
    assert err <= tol, (what, c, k, err, tol)
    if user_level < 0:
        assert out["direct"][c, k, 2] == 0.0 and not np.signbit(out["direct"][c, k, 2])
    if profiles:
        err = np.max(np.abs(out["direct_levels"][c, k] - want["direct"]))
        print(what, "column", c, "set", k, "direct levels", err, "of", tol)
        assert err <= tol, (what, c, k, err, tol)


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


def oracle_of(cache, orc, lib, band, tables, case, alb, solar, S):
    cl = case.clouds(S)
    return [cached(cache, ("direct", c, S), lambda: oracle_direct_sets(
        orc, lib, band, col, tables, cl["sw_liquid"][c], cl["sw_ice"][c], cl["thickness"][c], AEROSOL_GRID, case.f[1][c],
        alb, solar)) for c, col in enumerate(case.cols)]


# ---- (a) against the reference, (c) ordering ----------------------------------------------------------------------------- #
@pytest.mark.parametrize("profiles", [False, True])
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_direct_beam_matches_the_restatement(bands, tables, oracle, oracle_cache, case1, lib, device, S, spectral, profiles):
    cols, ncol = case1.cols, case1.ncol
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    want = oracle_of(oracle_cache, oracle, lib, bands[1], tables, case1, alb, solar, S)
    # on the oracle's numbers: under cloud the direct beam at the surface is well below the total -- handing back the
    # downward flux does not pass
    ratio = [w[2]["direct"][-1] / w[2]["dn_int"][-1] for w in want]
    print("cloud set, direct / down at the surface:", ratio)
    assert min(ratio) < 0.9, ratio
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, case1.clouds(S))
    gaer, keep_aer = aerosols_of(case1.f)
    got = run_direct(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
    assert got["direct"].shape == (ncol, 4, 3)
    check_order(got, profiles)
    for c in range(ncol):
        for k, w in enumerate(want[c]):
            ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())       # the column's largest shortwave flux
            check_direct(got, c, k, w, UL1, profiles, LEVEL_TOL * ff, NAMES[k])
            # (and the set's own rows are the oracle's: the restatement's inputs are the set's)
            assert np.max(np.abs(got["fluxes"][c, k, 9:12] - three(w["dn_int"], UL1))) <= LEVEL_TOL * ff
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (b) identities ------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_identities_bit_for_bit(bands, tables, case1, lib, device, monkeypatch, S, spectral):
    cols, ncol, L = case1.cols, case1.ncol, V1 - 1
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    gclouds, keep_clouds = make(tables, cl)
    gaer, keep_aer = aerosols_of(case1.f)
    gzero, keep_zero = aerosols_of(tuple(np.zeros_like(f) for f in case1.f))
    clear = clouds_for(cols, tables, CLOUD_SEED, clear=True)
    gclear, keep_clear = make(tables, {k: (np.repeat(v[:, None], 1, axis=1) if k in SETS else v) for k, v in clear.items()})
    _deterministic(lib, True)
    try:
        full = {}
        for profiles in (False, True):
            out = full[profiles] = run_direct(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
            check_order(out, profiles)
            # every output run_sky also writes is run_sky's
            assert same(without_direct(out), run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)), profiles
            # the beam at the top is the downward flux there
            assert np.array_equal(out["direct"][:, :, 0], out["fluxes"][:, :, 9]), profiles
            if profiles:
                assert np.array_equal(out["direct_levels"][:, :, [0, L, UL1]], out["direct"])
                assert np.array_equal(out["direct_levels"][:, :, 0], out["sw_down"][:, :, 0])
            # the four sets' beams differ below the top
            assert len({out["direct"][0, k, 1].tobytes() for k in range(4)}) == 4
            # an aerosol of zeros: the aerosol sets' rows are the clean and the cloud sets'
            z = run_direct(pipe, gcols, gclouds, gzero, S, ALL, ncol, profiles)
            for key in DIRECT_KEYS[:1 + profiles]:
                assert np.array_equal(z[key][:, 1], z[key][:, 0]) and np.array_equal(z[key][:, 3], z[key][:, 2]), key
                assert np.array_equal(z[key][:, [0, 2]], out[key][:, [0, 2]]), key
            # cloud-free tables (one draw): the cloud sets' rows are the clean and the aerosol sets'
            n = run_direct(pipe, gcols, gclear, gaer, 1, ALL, ncol, profiles)
            for key in DIRECT_KEYS[:1 + profiles]:
                assert np.array_equal(n[key][:, 2], n[key][:, 0]) and np.array_equal(n[key][:, 3], n[key][:, 1]), key
                assert np.array_equal(n[key][:, [0, 1]], out[key][:, [0, 1]]), key
            if S == 1:
                # S = 1 is the single draw: the draw given twice runs the subcolumn instances and the mean, and (x + x)/2 is
                # x to the bit
                twice = {k: (np.repeat(v, 2, axis=1) if k in SETS else v) for k, v in cl.items()}
                two_draws = run_direct(pipe, gcols, make(tables, twice)[0], gaer, 2, ALL, ncol, profiles)
                for key in out:
                    assert np.array_equal(two_draws[key], out[key]), (key, profiles)
            # any subset of the four sets has the rows it has in the full call
            for mask in range(16):
                sub = run_direct(pipe, gcols, gclouds if mask & (CLOUD | BOTH) else None,
                                 gaer if mask & (AEROSOL | BOTH) else None, S, mask, ncol, profiles)
                where = positions(mask)
                assert sub["direct"].shape[1] == len(where)
                for name, k in where.items():
                    for key in sub:
                        assert np.array_equal(sub[key][:, k], out[key][:, NAMES.index(name)]), (mask, name, key, profiles)
        # rows 0, L and the user level of the profile form are the six-row form's three, under either sweep rule
        assert np.array_equal(full[True]["direct"], full[False]["direct"])
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        two = run_direct(pipe, gcols, gclouds, gaer, S, ALL, ncol, False)
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        assert np.array_equal(two["direct"], full[True]["direct"])
        assert np.array_equal(two["fluxes"], full[True]["fluxes"])
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_clear_sky_split_alone_and_one_draw(bands, tables, case1, lib, device):
    """sets = GRT_SKY_CLEAN with no clouds and no aerosols; and S = 1 through the subcolumn count of the cloud tables."""
    cols, ncol = case1.cols, case1.ncol
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gaer, keep_aer = aerosols_of(case1.f)
    _deterministic(lib, True)
    try:
        for profiles in (False, True):
            full = run_direct(pipe, gcols, make(tables, case1.clouds(1))[0], gaer, 1, ALL, ncol, profiles)
            alone = run_direct(pipe, gcols, None, None, 0, CLEAN, ncol, profiles)
            assert alone["direct"].shape == (ncol, 1, 3)
            for key in alone:
                assert np.array_equal(alone[key][:, 0], full[key][:, 0]), key
            pipe.run(gcols)
            assert np.array_equal(pipe.fluxes(ncol), alone["fluxes"][:, 0])
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (d) batch indexing -------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("profiles", [False, True])
@pytest.mark.parametrize("spectral", [False, True])
def test_batch_indexing(bands, tables, case1, lib, device, spectral, profiles):
    """A batch at max_columns against its columns one at a time and in reversed order, the clouds and aerosols permuted
    against the columns (column c of the batch takes the clouds of column order[c] and the aerosol of another)."""
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    cl = case1.clouds(S)
    cloud_of, aer_of = [1, 2, 0], [2, 0, 1]
    _deterministic(lib, True)
    try:
        def run(order):
            g, k = api.make_columns([cols[c] for c in order], MOL_ORDER, cfc_order=(0, 1))
            gc, kc = make(tables, pick(cl, columns=[cloud_of[c] for c in order]))
            ga, ka = aerosols_of(tuple(np.ascontiguousarray(f[[aer_of[c] for c in order]]) for f in case1.f))
            return run_direct(pipe, g, gc, ga, S, ALL, len(order), profiles)
        batch = run([0, 1, 2])
        straight, ka0 = aerosols_of(case1.f)
        plain = run_direct(pipe, api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))[0], make(tables, cl)[0], straight, S,
                           ALL, ncol, profiles)
        assert not np.array_equal(plain["direct"][:, 1:, 1], batch["direct"][:, 1:, 1])        # the pairing matters
        rev = run([2, 1, 0])
        for key in batch:
            assert np.array_equal(rev[key], batch[key][::-1]), key
        for c in range(ncol):
            alone = run([c])
            for key in batch:
                assert np.array_equal(alone[key][0], batch[key][c]), (key, c)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (e) edge shapes ----------------------------------------------------------------------------------------------------- #
NS = (2, 127, 128, 129, 257)
# a reduced Latin square: every grid length twice, with level counts, subcolumn counts, user levels (mid: an interior level,
# which takes the six-row form through its two sweeps), batch sizes (1 and max_columns = 3) and forms rotating
SHAPES = [(2, 61, 3, "L", 3, True), (127, 2, 1, "0", 1, False), (128, 201, 1, "-1", 3, True), (129, 3, 3, "mid", 1, False),
          (257, 61, 1, "mid", 3, False), (127, 3, 3, "-1", 3, True), (129, 201, 3, "0", 1, False), (2, 2, 1, "L", 1, True),
          (257, 2, 3, "-1", 1, False), (128, 61, 3, "mid", 3, True)]
shape_bands = make_shape_bands(NS, 100.0, 2000.0)


@pytest.mark.parametrize("n,V,S,ul,ncol,profiles", SHAPES,
                         ids=[f"n{n}-V{V}-S{S}-ul{u}-c{c}-{'prof' if p else 'six'}" for n, V, S, u, c, p in SHAPES])
def test_edge_shapes(shape_bands, tables, oracle, lib, device, n, V, S, ul, ncol, profiles):
    L = V - 1
    user_level = {"-1": -1, "0": 0, "L": L, "mid": (L + 1) // 2}[ul]
    assert ul != "mid" or 0 < user_level < L
    lwb, swb = shape_bands[n]
    cols = [syn.profile(900 + V + c, V) for c in range(3)]
    for c, mu in zip(cols, (1.0, 0.05, 1e-3)):                      # overhead sun, low sun, the sun on the horizon
        c["mu0"] = mu
    cols = cols[:ncol]
    go_lw, _ = lwb.gas_optics(device, V)
    go_sw, grid_sw = swb.gas_optics(device, V)
    rng = np.random.default_rng(n + V)
    emis, alb = rng.uniform(0.3, 1.0, n), rng.uniform(0.0, 0.7, n)
    solar = api.create_solar_flux(grid_sw, swb.files["solar"])
    xs = (shape_grid(lwb, "two"), shape_grid(swb, "more"))
    f = (aerosol_fields(ncol, L, xs[0], 60 + n, lw=True), aerosol_fields(ncol, L, xs[1], 61 + n, lw=False))
    gaer, keep_aer = aerosols_of(f, xs)
    draws = [clouds_for(cols, tables, 90 + n + V + j) for j in range(S)]
    cl = {k: (np.stack([d[k] for d in draws], axis=1) if k in SETS else draws[0][k]) for k in draws[0]}
    gclouds, keep_clouds = make(tables, cl)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    pipes = {s: api.Pipeline(go_lw, go_sw, 3, user_level, emis, alb, solar, spectral=s) for s in (False, True)}
    got = {s: run_direct(pipes[s], gcols, gclouds, gaer, S, ALL, ncol, profiles) for s in (False, True)}
    for c, col in enumerate(cols):
        want = oracle_direct_sets(oracle, lib, swb, col, tables, cl["sw_liquid"][c], cl["sw_ice"][c], cl["thickness"][c],
                                  xs[1], f[1][c], alb, solar)
        for s in (False, True):
            check_order(got[s], profiles)
            for k, w in enumerate(want):
                ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
                assert ff > 0.0
                check_direct(got[s], c, k, w, user_level, profiles, LEVEL_TOL * ff, f"spectral={s}")
    for s in (False, True):
        pipes[s].destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (f) the production arithmetic --------------------------------------------------------------------------------------- #
def test_production_form_matches_the_restatement(bands, tables, oracle, lib, device):
    """fast = 3 on the 3 000-line bands: the direct rows and levels within the interface's flux contract, 1e-3 W m-2
    (test_gpu_pipeline_production.py), of the restatement."""
    FLUX_TOL, S = 1e-3, 2
    cols = sky_columns(320, V1, n=4)
    ncol = len(cols)
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1, fast=3)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, CLOUD_SEED + 1, S)
    gclouds, keep_clouds = make(tables, cl)
    f = fields(ncol, V1 - 1, AEROSOL_SEED + 2)
    gaer, keep_aer = aerosols_of(f)
    got = {p: run_direct(pipe, gcols, gclouds, gaer, S, ALL, ncol, p) for p in (False, True)}
    assert go_sw.last_launch()["fast"] == 3
    for c, col in enumerate(cols):
        want = oracle_direct_sets(oracle, lib, bands[1], col, tables, cl["sw_liquid"][c], cl["sw_ice"][c],
                                  cl["thickness"][c], AEROSOL_GRID, f[1][c], alb, solar)
        for p in (False, True):
            check_order(got[p], p)
            for k, w in enumerate(want):
                check_direct(got[p], c, k, w, UL1, p, FLUX_TOL, "production")
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (g) missing bands --------------------------------------------------------------------------------------------------- #
def test_missing_bands(bands, tables, case1, lib, device):
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)
    _deterministic(lib, True)
    try:
        both = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
        full = {p: run_direct(both, gcols, gclouds, gaer, S, ALL, ncol, p) for p in (False, True)}
        both.destroy()
        lw_only = api.Pipeline(go_lw, None, ncol, UL1, emis, None, None, spectral=False)
        sw_only = api.Pipeline(None, go_sw, ncol, UL1, None, alb, solar, spectral=False)
        for profiles in (False, True):
            run_direct(lw_only, gcols, gclouds, gaer, S, ALL, ncol, profiles)        # (allocates this form's buffers)
            name = "sky_profiles" if profiles else "sky"
            for key in [name + ".direct"] + ([name + ".direct_levels"] if profiles else []):
                fill = np.full(lw_only.buffers[key].nbytes // 8, -7.25)              # zeros are written, not left
                api.check(lib.grt_host_to_device(device, lw_only.buffers[key].ptr, fill.ctypes.data_as(C.c_void_p),
                                                 C.c_size_t(fill.nbytes)))
            out = run_direct(lw_only, gcols, gclouds, gaer, S, ALL, ncol, profiles)
            for key in DIRECT_KEYS[:1 + profiles]:
                assert np.all(out[key] == 0.0), key
            assert same(without_direct(out), run_sky(lw_only, gcols, gclouds, gaer, S, ALL, ncol, profiles))
            assert np.array_equal(out["fluxes"][:, :, :6], full[profiles]["fluxes"][:, :, :6])
            out = run_direct(sw_only, gcols, gclouds, gaer, S, ALL, ncol, profiles)
            for key in DIRECT_KEYS[:1 + profiles]:
                assert np.array_equal(out[key], full[profiles][key]), key
            assert np.all(out["fluxes"][:, :, :6] == 0.0)
        lw_only.destroy()
        sw_only.destroy()
    finally:
        _deterministic(lib, False)
    go_lw.destroy()
    go_sw.destroy()


# ---- (h) refusals -------------------------------------------------------------------------------------------------------- #
def test_refused_inputs(bands, tables, case1, lib, device):
    cols, ncol, L, S = case1.cols, case1.ncol, V1 - 1, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    sizes = (4 * 4 * V1 * (ncol + 1), 4 * 2 * L * (ncol + 1), 4 * 12 * (ncol + 1), 4 * 3 * (ncol + 1), 4 * V1 * (ncol + 1))
    bufs = [_sentinel(device, n) for n in sizes]
    lv, hr, fx, d3, dl = (b.ptr for b in bufs)
    tags = (api.TAG_GAS_LW, api.TAG_GAS_SW, api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_AEROSOL_LW, api.TAG_AEROSOL_SW,
            api.TAG_ALLSKY_LW, api.TAG_ALLSKY_SW, api.TAG_SKY_LW, api.TAG_SKY_SW, api.TAG_SUBCOLUMN_MEAN,
            api.TAG_DIRECT_BEAM)

    def call(gc, gsky, gdirect, form):
        api.check(lib.grt_pipeline_run_sky_direct(pipe.p, C.byref(gc), C.byref(gsky) if gsky is not None else None,
                                                  C.byref(gdirect) if gdirect is not None else None, *form))

    def refused(gc, gcl, ga, S_, sets, code=api.VALUE_ERR, sky=True, forms=None):
        gsky, ks = api.make_sky(gcl, ga, S_, sets)
        forms = forms or ((api.GrtDirectBeam(d3, dl), (lv, hr, fx)), (api.GrtDirectBeam(d3, None), (None, None, fx)))
        for gdirect, form in forms:
            with pytest.raises(api.GrtError) as e:
                call(gc, gsky if sky else None, gdirect, form)
            assert e.value.code == code, (sets, e.value)
        pipe.sync()
        for b, n in zip(bufs, sizes):
            assert np.all(b.to_host((n,)) == -7.25)

    gclouds, kc = make(tables, cl)
    gaer, ka = aerosols_of(case1.f)
    api.profile_enable(True)
    try:
        api.profile_read(tags[0], reset=True)
        # the direct outputs
        refused(gcols, gclouds, gaer, S, ALL, forms=((None, (lv, hr, fx)), (None, (None, None, fx))))
        refused(gcols, gclouds, gaer, S, ALL, forms=((api.GrtDirectBeam(None, dl), (lv, hr, fx)),
                                                     (api.GrtDirectBeam(None, None), (None, None, fx))))
        refused(gcols, gclouds, gaer, S, ALL, forms=((api.GrtDirectBeam(d3, dl), (None, None, fx)),))
        # everything grt_pipeline_run_sky refuses
        refused(gcols, gclouds, gaer, S, ALL, sky=False)
        for stray in (16, ALL | 32, 1 << 31):
            refused(gcols, gclouds, gaer, S, stray)
        for sets in (CLOUD, BOTH, ALL):
            refused(gcols, None, gaer, S, sets)
        for sets in (AEROSOL, BOTH, ALL):
            refused(gcols, gclouds, None, S, sets)
        for bad in (0, -1, api.GRT_MAX_SUBCOLUMNS + 1):
            refused(gcols, gclouds, gaer, bad, ALL)
        for field in SETS + ("thickness", "liquid_band_lo"):
            g, k = make(tables, cl)
            setattr(g, field, None)
            refused(gcols, g, gaer, S, ALL)
        g, k = make(tables, cl)
        g.num_liquid_bands = 0
        refused(gcols, g, gaer, S, CLOUD | AEROSOL)
        for field, value in (("lw_num_points", 1), ("sw_num_points", -1), ("lw_grid", None), ("sw_optics", None)):
            g, k = aerosols_of(case1.f)
            setattr(g, field, value)
            refused(gcols, gclouds, g, S, ALL)
        bad_grid = np.array([150.0, 900.0, 300.0, 1200.0])
        g, k = api.make_aerosols(lw=(bad_grid, np.ascontiguousarray(case1.f[0][..., :4])), sw=(AEROSOL_GRID, case1.f[1]))
        refused(gcols, gclouds, g, S, BOTH)
        big_cols = sky_columns(300, V1, n=4)
        big, keep_big = api.make_columns(big_cols, MOL_ORDER, cfc_order=(0, 1))
        gb, kb = make(tables, subcolumn_clouds(big_cols, tables, CLOUD_SEED, S))
        ab, kab = aerosols_of(fields(4, L, AEROSOL_SEED))
        refused(big, gb, ab, S, ALL)
        gcols.ncol = 0
        refused(gcols, gclouds, gaer, S, ALL)
        gcols.ncol = ncol
        gsky, ks = api.make_sky(gclouds, gaer, S, ALL)
        with pytest.raises(api.GrtError) as e:                                      # nothing to write
            call(gcols, gsky, api.GrtDirectBeam(d3, None), (None, hr, None))
        assert e.value.code == api.VALUE_ERR
        night = [dict(c) for c in cols]
        night[1]["mu0"] = 0.0
        gnight, keep_night = api.make_columns(night, MOL_ORDER, cfc_order=(0, 1))
        refused(gnight, gclouds, gaer, S, ALL, code=api.RANGE_ERR)
        pipe.sync()
        counts = {tag: api.profile_read(tag)[1] for tag in tags}
        assert all(n == 0 for n in counts.values()), counts
    finally:
        api.profile_enable(False)
    # and the call accepted: the outputs that may be NULL are
    call(gcols, gsky, api.GrtDirectBeam(d3, None), (lv, None, None))
    pipe.sync()
    rows = bufs[3].to_host((ncol + 1, 4, 3))
    assert np.all(np.isfinite(rows[:ncol])) and np.all(rows[:ncol, :, 2] == 0.0) and np.all(rows[ncol] == -7.25)
    assert np.all(rows[:ncol, :, :2] > 0.0) and np.all(bufs[4].to_host((sizes[4],)) == -7.25)
    call(gcols, gsky, api.GrtDirectBeam(d3, dl), (lv, None, None))
    pipe.sync()
    levels = bufs[4].to_host((ncol + 1, 4, V1))
    # the rows and the levels of ONE call, bit for bit: two default-mode calls are not (the gas-optics kernels add into
    # their tiles with atomics in the order the waves are scheduled in: scenario.RUN_TO_RUN_FUSED, test_gpu_tips_iso.py)
    rows = bufs[3].to_host((ncol + 1, 4, 3))
    assert np.array_equal(levels[:ncol][:, :, [0, L]], rows[:ncol, :, :2]) and np.all(levels[ncol] == -7.25)
    assert np.all(rows[:ncol, :, 2] == 0.0) and np.all(rows[ncol] == -7.25)
    for b in bufs:
        b.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (i) the existing entry points, before and after --------------------------------------------------------------------- #
@pytest.mark.parametrize("spectral", [False, True])
def test_existing_entry_points_unchanged(bands, tables, case1, lib, device, spectral):
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)
    mu = np.array([[c["mu0"], 0.5 * c["mu0"], -0.1] for c in cols])

    def older():
        out = {}
        pipe.run(gcols)
        out["run"] = pipe.fluxes(ncol)
        pipe.run_profiles(gcols)
        out.update({"run_profiles." + k: v for k, v in pipe.profiles(ncol).items()})
        for profiles in (False, True):
            out.update({f"run_sky.{profiles}.{k}": v for k, v in
                        run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles).items()})
            pipe.run_subcolumns(gcols, gclouds, S, profiles=profiles)
            if profiles:
                out.update({f"run_subcolumns.{s}.{k}": v for s, d in enumerate(pipe.subcolumn_profiles(ncol))
                            for k, v in d.items()})
            else:
                out["run_subcolumns"] = np.stack(pipe.subcolumn_fluxes(ncol))
            gz, kz = api.make_zeniths(mu)
            pipe.run_zeniths(gcols, gz, profiles=profiles)
            if profiles:
                out.update({"run_zeniths." + k: v for k, v in pipe.zenith_profiles(ncol, 3).items()})
            else:
                out["run_zeniths"], out["run_zeniths.angles"] = pipe.zenith_fluxes(ncol, 3)
        return out

    _deterministic(lib, True)
    try:
        before = older()
        for profiles in (False, True):
            run_direct(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
        after = older()
        assert before.keys() == after.keys()
        for k in before:
            assert np.array_equal(before[k], after[k]), k
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
