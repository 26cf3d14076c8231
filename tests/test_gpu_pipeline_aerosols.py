"""grt_pipeline_run_aerosols: the clear-clean set and the clear-sky-with-aerosols set of the batched pipeline, six-row and
profile form, fused and materialised, against the oracle's column-by-column restatement of driver.c:426-472 (gas, Rayleigh
and the aerosol interpolated onto the grid, through add_optics of three objects and the same solvers); the bit-for-bit
identities of the pass; batch indexing; edge shapes; what the entry point refuses."""
import ctypes as C

import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID, aerosol_fields, oracle_aerosol_column
from grtcode_amd import api, synthetic as syn
from pipeline_support import CP, GRAVITY, _sentinel, _setup, check_levels, heating, make_shape_bands, oracle_column
from pipeline_support import bands  # noqa: F401  (a module fixture)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

# Edge shapes: the bound test_gpu_solver_shapes.py holds the same solver kernels to at the same shapes, 1e-10 of the
# column's largest level flux (the aerosol instances add three multiply-adds and one more term to the combination)
LEVEL_TOL = 1e-10


def fields(ncol, L, seed, grid=AEROSOL_GRID):
    return aerosol_fields(ncol, L, grid, seed, lw=True), aerosol_fields(ncol, L, grid, seed + 1, lw=False)


def run(pipe, gcols, gaer, ncol, profiles):
    """-> (clean, aerosol): dicts with allsky_profiles()' keys; the six-row form has "fluxes" only."""
    pipe.run_aerosols(gcols, gaer, profiles=profiles)
    if profiles:
        return pipe.aerosol_profiles(ncol)
    clean, aer = pipe.aerosol_fluxes(ncol)
    return dict(fluxes=clean), dict(fluxes=aer)


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


# ---- 1. against the oracle -------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("profiles", [False, True])
@pytest.mark.parametrize("spectral", [False, True])
def test_aerosol_fluxes_match_the_oracle(bands, oracle, lib, device, spectral, profiles):
    lwb, swb = bands
    V, ncol, user_level = 16, 3, 5
    L = V - 1
    cols = [syn.profile(260 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    lw_f, sw_f = fields(ncol, L, 41)
    gaer, keep_aer = api.make_aerosols(lw=(AEROSOL_GRID, lw_f), sw=(AEROSOL_GRID, sw_f))
    clean, aer = run(pipe, gcols, gaer, ncol, profiles)
    if spectral:
        views = [pipe.views(bi) for bi in range(2)]
        got_opt = [{k: api.device_to_host(device, v[k], (ncol, L, band.nw)) for k in ("tau", "omega", "g")}
                   for v, band in zip(views, bands)]
    for bi, (band, lw, key, f) in enumerate(((lwb, True, "lw", lw_f), (swb, False, "sw", sw_f))):
        effect = 0.0
        for c, col in enumerate(cols):
            want_clean = oracle_column(oracle, lib, band, col, lw, emis, alb, solar, user_level)
            w = oracle_aerosol_column(oracle, lib, band, col, lw, AEROSOL_GRID, f[c], emis, alb, solar, user_level)
            print(key, c, "clean", np.max(np.abs(clean["fluxes"][c, 6 * bi: 6 * bi + 6] - want_clean["integ"])),
                  "aerosol", np.max(np.abs(aer["fluxes"][c, 6 * bi: 6 * bi + 6] - w["integ"])),
                  "effect", np.max(np.abs(w["integ"] - want_clean["integ"])))
            assert np.max(np.abs(clean["fluxes"][c, 6 * bi: 6 * bi + 6] - want_clean["integ"])) < 1e-9, key
            assert np.max(np.abs(aer["fluxes"][c, 6 * bi: 6 * bi + 6] - w["integ"])) < 1e-9, key
            effect = max(effect, np.max(np.abs(w["integ"] - want_clean["integ"])))
            assert np.any(w["aerosol"][0] == 0.0) and np.any(w["aerosol"][0] > 0.0)    # points without and with aerosol
            if profiles:
                cu = np.array([oracle.integrate_row(want_clean["up"][k], band.dw) for k in range(V)])
                cd = np.array([oracle.integrate_row(want_clean["dn"][k], band.dw) for k in range(V)])
                check_levels(clean, c, key, col, cu, cd)
                check_levels(aer, c, key, col, w["up_int"], w["dn_int"])
            if spectral:
                o = got_opt[bi]
                assert np.max(np.abs(o["tau"][c] - w["tau"]) / np.abs(w["tau"]).max(axis=1, keepdims=True)) < 1e-11
                assert np.max(np.abs(o["omega"][c] - w["omega"])) < 1e-11
                assert np.max(np.abs(o["g"][c] - w["g"])) < 1e-11
                assert np.max(np.abs(w["g"])) > 0.1                 # aerosol asymmetry reached the combination
        assert effect > 1e-2, key                                   # the oracle's aerosol set is not its clean set
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 2. identities ---------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("spectral", [False, True])
def test_zero_aerosol_gives_the_clean_rows(bands, lib, device, spectral):
    V, ncol = 16, 2
    cols = [syn.profile(275 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 4, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    zero = np.zeros((ncol, 3, V - 1, AEROSOL_GRID.size))
    gaer, keep_aer = api.make_aerosols(lw=(AEROSOL_GRID, zero), sw=(AEROSOL_GRID, zero))
    for profiles in (False, True):
        clean, aer = run(pipe, gcols, gaer, ncol, profiles)
        assert same(clean, aer), profiles
        assert np.all(clean["fluxes"][:, [0, 6]] > 0.0)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("spectral", [False, True])
def test_a_band_without_aerosol_is_its_clean_set(bands, oracle, lib, device, spectral):
    lwb, swb = bands
    V, ncol, user_level = 16, 2, 9
    L = V - 1
    cols = [syn.profile(280 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    lw_f, sw_f = fields(ncol, L, 43)
    for none in (0, 1):
        gaer, keep_aer = api.make_aerosols(lw=None if none == 0 else (AEROSOL_GRID, lw_f),
                                           sw=None if none == 1 else (AEROSOL_GRID, sw_f))
        band, lw, key, f = ((swb, False, "sw", sw_f), (lwb, True, "lw", lw_f))[none]
        other = 1 - none
        for profiles in (False, True):
            clean, aer = run(pipe, gcols, gaer, ncol, profiles)
            assert np.array_equal(clean["fluxes"][:, 6 * none: 6 * none + 6], aer["fluxes"][:, 6 * none: 6 * none + 6])
            assert not np.array_equal(clean["fluxes"][:, 6 * other: 6 * other + 6], aer["fluxes"][:, 6 * other: 6 * other + 6])
            if profiles:
                pre = ("lw", "sw")[none]
                assert all(np.array_equal(clean[pre + k], aer[pre + k]) for k in ("_up", "_down", "_heating"))
            for c, col in enumerate(cols):
                w = oracle_aerosol_column(oracle, lib, band, col, lw, AEROSOL_GRID, f[c], emis, alb, solar, user_level)
                assert np.max(np.abs(aer["fluxes"][c, 6 * other: 6 * other + 6] - w["integ"])) < 1e-9, key
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("spectral", [False, True])
def test_clean_set_is_run_and_the_forms_agree(bands, lib, device, monkeypatch, spectral):
    V, ncol, user_level = 16, 3, 7
    L = V - 1
    cols = [syn.profile(285 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    lw_f, sw_f = fields(ncol, L, 45)
    gaer, keep_aer = api.make_aerosols(lw=(AEROSOL_GRID, lw_f), sw=(AEROSOL_GRID, sw_f))
    api.check(lib.grt_set_deterministic(1))
    try:
        pipe.run(gcols)
        first = pipe.fluxes(ncol)
        api.profile_enable(True)
        clean, aer = run(pipe, gcols, gaer, ncol, False)
        lw_ms, lw_n = api.profile_read(api.TAG_AEROSOL_LW)
        sw_ms, sw_n = api.profile_read(api.TAG_AEROSOL_SW)
        api.profile_enable(False)
        assert lw_n == 1 and sw_n == 1 and lw_ms > 0.0 and sw_ms > 0.0          # the aerosol solvers' tags
        assert np.array_equal(clean["fluxes"], first)
        assert not np.array_equal(aer["fluxes"], first)
        pipe.run_profiles(gcols)
        prof = pipe.profiles(ncol)
        pclean, paer = run(pipe, gcols, gaer, ncol, True)
        assert same(pclean, prof)
        again = run(pipe, gcols, gaer, ncol, True)
        assert same(again[0], pclean) and same(again[1], paer)
        # rows 0, L and the user level of the profile form are the six-row form's with two shortwave sweeps
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        clean2, aer2 = run(pipe, gcols, gaer, ncol, False)
        for p, six_all in ((pclean, clean2["fluxes"]), (paer, aer2["fluxes"])):
            assert np.array_equal(p["fluxes"], six_all)
            for bi, key in enumerate(("lw", "sw")):
                six = six_all[:, 6 * bi: 6 * bi + 6]
                up, dn = p[key + "_up"], p[key + "_down"]
                assert np.array_equal(up[:, [0, L, user_level]], six[:, :3]), key
                assert np.array_equal(dn[:, [0, L, user_level]], six[:, 3:]), key
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        pipe.run(gcols)
        assert np.array_equal(pipe.fluxes(ncol), first)
    finally:
        api.profile_enable(False)
        api.check(lib.grt_set_deterministic(-1))
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 3. batch indexing ------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spectral", [False, True])
def test_batch_indexing_and_a_changing_grid(bands, lib, device, spectral):
    V, ncol = 16, 4
    L = V - 1
    cols = [syn.profile(290 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 3, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    lw_f, sw_f = fields(ncol, L, 47)
    gaer, keep_aer = api.make_aerosols(lw=(AEROSOL_GRID, lw_f), sw=(AEROSOL_GRID, sw_f))
    other_grid = np.array([50.0, 320.5, 2000.0, 4990.0, 6000.0])
    lw_o, sw_o = fields(2, L, 49, other_grid)
    api.check(lib.grt_set_deterministic(1))
    try:
        for profiles in (False, True):
            clean, aer = run(pipe, gcols, gaer, ncol, profiles)
            assert len({aer["fluxes"][c].tobytes() for c in range(ncol)}) == ncol
            for c in range(ncol):
                g1, k1 = api.make_columns(cols[c:c + 1], MOL_ORDER, cfc_order=(0, 1))
                a1, ka1 = api.make_aerosols(lw=(AEROSOL_GRID, lw_f[c:c + 1]), sw=(AEROSOL_GRID, sw_f[c:c + 1]))
                one_clean, one_aer = run(pipe, g1, a1, 1, profiles)
                assert all(np.array_equal(one_clean[k][0], clean[k][c]) for k in clean), (c, profiles)
                assert all(np.array_equal(one_aer[k][0], aer[k][c]) for k in aer), (c, profiles)
            # fewer columns on another aerosol grid (the maps are rebuilt), then the first grid again
            g2, k2 = api.make_columns(cols[1:3], MOL_ORDER, cfc_order=(0, 1))
            a2, ka2 = api.make_aerosols(lw=(other_grid, lw_o), sw=(other_grid, sw_o))
            two_clean, two_aer = run(pipe, g2, a2, 2, profiles)
            assert all(np.array_equal(two_clean[k], clean[k][1:3]) for k in clean)
            assert not np.array_equal(two_aer["fluxes"][:, :6], aer["fluxes"][1:3, :6])
            assert not np.array_equal(two_aer["fluxes"][:, 6:], aer["fluxes"][1:3, 6:])
            a3, ka3 = api.make_aerosols(lw=(other_grid, lw_o[1:]), sw=(other_grid, sw_o[1:]))
            g3, k3 = api.make_columns(cols[2:3], MOL_ORDER, cfc_order=(0, 1))
            three = run(pipe, g3, a3, 1, profiles)
            assert all(np.array_equal(three[1][k][0], two_aer[k][1]) for k in two_aer)
            back = run(pipe, gcols, gaer, ncol, profiles)
            assert same(back[0], clean) and same(back[1], aer)
    finally:
        api.check(lib.grt_set_deterministic(-1))
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 4. edge shapes --------------------------------------------------------------------------------------------------- #
NS = (2, 127, 128, 129, 257)
# a reduced Latin square: every grid length once, with level counts, aerosol grid sizes (2 points / more points than the
# grid has), user levels and forms rotating against each other
SHAPES = [(2, 61, "more", "L", True), (127, 2, "two", "0", False), (128, 201, "more", "-1", False),
          (129, 3, "two", "L", True), (257, 61, "two", "0", True), (127, 3, "more", "-1", True),
          (129, 201, "more", "0", False), (2, 2, "two", "-1", False)]
shape_bands = make_shape_bands(NS, 100.0, 2000.0)


def shape_grid(band, kind):
    span = band.wn - band.w0
    if kind == "two":
        if band.nw == 2:
            return np.array([band.w0 - 0.5 * band.dw, band.wn + 0.5 * band.dw])
        return np.array([band.w0 + 0.3 * span, band.w0 + 0.8 * span])           # points below, inside and above
    return np.linspace(band.w0 - 2.5 * band.dw, band.wn + 2.5 * band.dw, band.nw + 3)


@pytest.mark.parametrize("n,V,na_kind,ul,profiles", SHAPES, ids=[f"n{n}-V{V}-{k}-ul{u}-{'prof' if p else 'six'}"
                                                                for n, V, k, u, p in SHAPES])
def test_edge_shapes(shape_bands, oracle, lib, device, n, V, na_kind, ul, profiles):
    L = V - 1
    user_level = {"-1": -1, "0": 0, "L": L}[ul]
    lwb, swb = shape_bands[n]
    mus = (1.0, 0.05, 0.0)                                          # overhead sun, low sun, night
    cols = [syn.profile(700 + V + c, V) for c in range(len(mus))]
    for c, mu in zip(cols, mus):
        c["mu0"] = mu
    ncol = len(cols)
    go_lw, _ = lwb.gas_optics(device, V)
    go_sw, grid_sw = swb.gas_optics(device, V)
    rng = np.random.default_rng(n + V)
    emis, alb = rng.uniform(0.3, 1.0, n), rng.uniform(0.0, 0.7, n)
    solar = api.create_solar_flux(grid_sw, swb.files["solar"])
    xs = (shape_grid(lwb, na_kind), shape_grid(swb, na_kind))
    f = (aerosol_fields(ncol, L, xs[0], 50 + n, lw=True), aerosol_fields(ncol, L, xs[1], 51 + n, lw=False))
    gaer, keep_aer = api.make_aerosols(lw=(xs[0], f[0]), sw=(xs[1], f[1]))
    pipes = {s: api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=s) for s in (False, True)}
    # a night column in the launch: the batch is refused as the other entry points refuse it (night columns are the caller's
    # to skip), nothing is written
    gnight, keep_night = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    guard = _sentinel(device, 24 * ncol)
    with pytest.raises(api.GrtError) as e:
        api.check(lib.grt_pipeline_run_aerosols(pipes[False].p, C.byref(gnight), C.byref(gaer), None, None, guard.ptr))
    assert e.value.code == api.RANGE_ERR
    pipes[False].sync()
    assert np.all(guard.to_host((24 * ncol,)) == -7.25)
    guard.free()
    cols[2]["mu0"] = 1e-3                                           # the sun on the horizon: tau/mu clamps at 700
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    got = {s: run(pipes[s], gcols, gaer, ncol, profiles) for s in (False, True)}
    for bi, (band, lw, key) in enumerate(((lwb, True, "lw"), (swb, False, "sw"))):
        for c, col in enumerate(cols):
            w = oracle_aerosol_column(oracle, lib, band, col, lw, xs[bi], f[bi][c], emis, alb, solar, user_level)
            wc = oracle_column(oracle, lib, band, col, lw, emis, alb, solar, user_level)
            ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
            assert ff > 0.0
            for s in (False, True):
                clean, aer = got[s]
                err = np.max(np.abs(aer["fluxes"][c, 6 * bi: 6 * bi + 6] - w["integ"]))
                print(key, c, s, "aerosol six", err / ff)
                assert err <= LEVEL_TOL * ff, (key, c, s)
                assert np.max(np.abs(clean["fluxes"][c, 6 * bi: 6 * bi + 6] - wc["integ"])) <= LEVEL_TOL * ff, (key, c, s)
                if user_level < 0:
                    assert np.all(aer["fluxes"][c, [6 * bi + 2, 6 * bi + 5]] == 0.0)
                if profiles:
                    assert np.max(np.abs(aer[key + "_up"][c] - w["up_int"])) <= LEVEL_TOL * ff, (key, c, s)
                    assert np.max(np.abs(aer[key + "_down"][c] - w["dn_int"])) <= LEVEL_TOL * ff, (key, c, s)
                    mass = 100.0 * (col["p"][1:] - col["p"][:-1]) / GRAVITY
                    bound = 4.0 * LEVEL_TOL * ff / (CP * mass) * 86400.0
                    want_hr = heating(w["up_int"], w["dn_int"], col["p"])
                    assert np.all(np.abs(aer[key + "_heating"][c] - want_hr) <= bound + 1e-12 * np.abs(want_hr).max())
    # an aerosol of zeros at this shape: the clean set, bit for bit
    gzero, keep_zero = api.make_aerosols(lw=(xs[0], np.zeros_like(f[0])), sw=(xs[1], np.zeros_like(f[1])))
    for s in (False, True):
        clean, aer = run(pipes[s], gcols, gzero, ncol, profiles)
        assert same(clean, aer), s
        pipes[s].destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------ #
def test_refused_inputs(bands, lib, device):
    V, ncol = 16, 2
    L = V - 1
    cols = [syn.profile(250 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    lw_f, sw_f = fields(ncol + 1, L, 53)
    sizes = (8 * V * (ncol + 1), 4 * L * (ncol + 1), 24 * (ncol + 1))
    bufs = [_sentinel(device, n) for n in sizes]

    def make(nc=ncol):
        return api.make_aerosols(lw=(AEROSOL_GRID, lw_f[:nc]), sw=(AEROSOL_GRID, sw_f[:nc]))

    def refused(gc, ga, ptrs=None):
        ptrs = [b.ptr for b in bufs] if ptrs is None else ptrs
        for form in (ptrs, [None, None, ptrs[2]]):
            with pytest.raises(api.GrtError) as e:
                api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gc), C.byref(ga) if ga is not None else None, *form))
            assert e.value.code == api.VALUE_ERR
        pipe.sync()
        for b, n in zip(bufs, sizes):
            assert np.all(b.to_host((n,)) == -7.25)

    refused(gcols, None)
    for field, value in (("lw_num_points", 1), ("sw_num_points", 1), ("lw_num_points", -3), ("sw_num_points", -1),
                         ("lw_grid", None), ("sw_grid", None), ("lw_optics", None), ("sw_optics", None)):
        g, k = make()
        setattr(g, field, value)
        refused(gcols, g)
    for bad in (np.array([150.0, 300.0, 300.0, 900.0]), np.array([150.0, 900.0, 300.0, 1200.0])):   # equal, decreasing
        f4 = np.ascontiguousarray(lw_f[:ncol, :, :, :4])
        for g, k in (api.make_aerosols(lw=(bad, f4), sw=(AEROSOL_GRID, sw_f[:ncol])),
                     api.make_aerosols(lw=(AEROSOL_GRID, lw_f[:ncol]), sw=(bad, f4))):
            refused(gcols, g)
    g, k = make()
    with pytest.raises(api.GrtError) as e:                                      # nothing to write
        api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gcols), C.byref(g), None, None, None))
    assert e.value.code == api.VALUE_ERR
    with pytest.raises(api.GrtError) as e:
        api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gcols), C.byref(g), None, bufs[1].ptr, None))
    assert e.value.code == api.VALUE_ERR
    big, keep_big = api.make_columns([syn.profile(250 + c, V) for c in range(ncol + 1)], MOL_ORDER, cfc_order=(0, 1))
    gb, kb = make(ncol + 1)
    refused(big, gb)
    gcols.ncol = 0
    refused(gcols, g)
    gcols.ncol = ncol
    # and the same calls accepted: both forms, NULL heating_dev and fluxes_dev in the profile form
    api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gcols), C.byref(g), None, None, bufs[2].ptr))
    api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gcols), C.byref(g), bufs[0].ptr, None, None))
    pipe.sync()
    assert np.all(np.isfinite(bufs[2].to_host((ncol + 1, 24))[:ncol])) and np.all(bufs[2].to_host((ncol + 1, 24))[ncol] == -7.25)
    lv = bufs[0].to_host((ncol + 1, 8, V))
    assert np.all(np.isfinite(lv[:ncol])) and np.all(lv[ncol] == -7.25) and np.all(bufs[1].to_host((sizes[1],)) == -7.25)
    for b in bufs:
        b.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_one_band_pipelines_ignore_the_other_bands_fields(bands, lib, device):
    """A band without a gas-optics object ignores its aerosol fields (even ones that would be refused) and writes zeros."""
    V, ncol = 16, 2
    L = V - 1
    cols = [syn.profile(255 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    lw_f, sw_f = fields(ncol, L, 55)
    for which in (0, 1):
        pipe = api.Pipeline(go_lw if which == 0 else None, go_sw if which == 1 else None, ncol, -1, emis if which == 0 else None,
                            alb if which == 1 else None, solar if which == 1 else None, spectral=False)
        g, k = api.make_aerosols(lw=(AEROSOL_GRID, lw_f), sw=(AEROSOL_GRID, sw_f))
        if which == 0:
            g.sw_num_points, g.sw_grid = 1, None
        else:
            g.lw_num_points, g.lw_optics = -2, None
        for profiles in (False, True):
            clean, aer = run(pipe, gcols, g, ncol, profiles)
            missing = slice(6 * (1 - which), 6 * (1 - which) + 6)
            present = slice(6 * which, 6 * which + 6)
            assert np.all(clean["fluxes"][:, missing] == 0.0) and np.all(aer["fluxes"][:, missing] == 0.0)
            assert not np.array_equal(aer["fluxes"][:, present], clean["fluxes"][:, present])
        pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
