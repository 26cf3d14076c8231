"""grt_pipeline_run_spectral: the six output rows at every grid point and their wavenumber bins, clear sky and all-sky,
in the production (fused) and the materialised form -- against the oracle's column-by-column restatement of
driver.c:285-356 without -integrated, against the same call's broadband values and the pipeline's other runs, at the
grid and bin shapes where a block-wise sum goes wrong, and at the bench's shortwave width."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api, synthetic as syn
from pipeline_support import _setup, block_edges, cloud_columns, limits, make, make_shape_bands, oracle_rows
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from scenario import Band, MOL_ORDER

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-10      # of the band's flux scale: the bound test_gpu_pipeline.py puts on the spectral views
BIN_TOL = 1e-9       # W m-2
MU0 = (1.0, 0.5, 0.05, 1e-3)


def want_bins(orc, rows, edges, dw):
    return np.array([[orc.integrate_row(r[edges[b]:edges[b + 1] + 1], dw) for b in range(edges.size - 1)] for r in rows])


def check_band(orc, got_rows, got_bins, want, edges, dw):
    scale = np.abs(want).max()
    assert scale > 0.0
    assert np.max(np.abs(got_rows - want)) <= ROW_TOL * scale
    if edges is not None:
        assert np.max(np.abs(got_bins - want_bins(orc, want, edges, dw))) <= BIN_TOL


@pytest.mark.parametrize("user_level", [5, -1])
@pytest.mark.parametrize("allsky", [False, True])
@pytest.mark.parametrize("spectral", [False, True])
def test_spectral_rows_and_bins_match_the_oracle(bands, tables, oracle, lib, device, spectral, allsky, user_level):
    lwb, swb = bands
    V, ncol = 16, 2
    cols = [syn.profile(300 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup((lwb, swb), device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 31) if allsky else None
    gclouds, keep_clouds = make(tables, cl) if allsky else (None, None)
    edges = {"lw": block_edges(lwb.nw), "sw": np.array([0, 3, 127, 128, 129, 300, 383, 384, 385, 498, 499], np.int32)}
    pipe.run_spectral(gcols, gclouds, edges["lw"], edges["sw"])
    got = pipe.spectral(ncol)
    sets = 2 if allsky else 1
    assert got["lw"].shape == (ncol, sets, 6, lwb.nw) and got["sw"].shape == (ncol, sets, 6, swb.nw)
    assert got["fluxes"].shape == (ncol, 12 * sets)
    for c, col in enumerate(cols):
        for bi, (band, lw, key) in enumerate(((lwb, True, "lw"), (swb, False, "sw"))):
            for s in range(sets):
                cloud = None if s == 0 else (cl[key + "_liquid"][c], cl[key + "_ice"][c], cl["thickness"][c])
                want = oracle_rows(oracle, lib, band, col, lw, user_level, cloud, tables, emis, alb, solar)
                check_band(oracle, got[key][c, s], got[key + "_bins"][c, s], want, edges[key], band.dw)
                integ = [oracle.integrate_row(r, band.dw) for r in want]
                assert np.max(np.abs(got["fluxes"][c, 12 * s + 6 * bi: 12 * s + 6 * bi + 6] - integ)) <= BIN_TOL
                if user_level < 0:
                    assert np.all(got[key][c, s, [2, 5]] == 0.0) and np.all(got[key + "_bins"][c, s, [2, 5]] == 0.0)
                else:
                    assert np.all(got[key][c, s, [2, 5]] != 0.0)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("spectral", [False, True])
def test_a_bin_over_the_whole_grid_is_the_broadband_value(bands, tables, lib, device, spectral, deterministic):
    lwb, swb = bands
    V, ncol = 16, 3
    cols = [syn.profile(310 + c, V) for c in range(ncol)]
    for c, mu in zip(cols, MU0):
        c["mu0"] = mu
    go_lw, go_sw, emis, alb, solar = _setup((lwb, swb), device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 7, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, cloud_columns(cols, tables, 32))
    whole = [np.array([0, b.nw - 1], np.int32) for b in (lwb, swb)]
    api.check(lib.grt_set_deterministic(1 if deterministic else 0))
    try:
        for gcl in (None, gclouds):
            pipe.run_spectral(gcols, gcl, *whole)
            got = pipe.spectral(ncol)
            sets = 1 if gcl is None else 2
            for s in range(sets):
                for bi, key in ((0, "lw"), (1, "sw")):
                    six = got["fluxes"][:, 12 * s + 6 * bi: 12 * s + 6 * bi + 6]
                    binned = got[key + "_bins"][:, s, :, 0]
                    if not spectral:
                        assert np.array_equal(binned, six), (key, s)
                    else:
                        assert np.max(np.abs(binned - six)) <= 1e-12 * np.abs(six).max(), (key, s)
    finally:
        api.check(lib.grt_set_deterministic(-1))
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("spectral", [False, True])
def test_fluxes_are_those_of_run_and_run_allsky(bands, tables, lib, device, spectral):
    lwb, swb = bands
    V, ncol = 16, 3
    cols = [syn.profile(320 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup((lwb, swb), device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 4, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, cloud_columns(cols, tables, 33))
    edges = (block_edges(lwb.nw), block_edges(swb.nw))
    api.check(lib.grt_set_deterministic(1))
    try:
        pipe.run(gcols)
        run = pipe.fluxes(ncol)
        pipe.run_allsky(gcols, gclouds)
        allsky = np.concatenate(pipe.allsky_fluxes(ncol), axis=1)
        pipe.run_spectral(gcols, None, *edges)
        clear = pipe.spectral(ncol)
        pipe.run_spectral(gcols, gclouds, *edges)
        cloudy = pipe.spectral(ncol)
        pipe.run(gcols)
        again = pipe.fluxes(ncol)
    finally:
        api.check(lib.grt_set_deterministic(-1))
    assert np.array_equal(clear["fluxes"], run)
    assert np.array_equal(cloudy["fluxes"], allsky)
    assert np.array_equal(again, run)
    # the clear-sky set of the all-sky call is the clear-sky call's
    for key in ("lw", "sw", "lw_bins", "sw_bins"):
        assert np.array_equal(cloudy[key][:, 0], clear[key][:, 0]), key
        assert np.max(np.abs(cloudy[key][:, 1] - cloudy[key][:, 0])) > 0.0, key
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("spectral", [False, True])
def test_contiguous_bins_add_up_and_one_interval_bins_are_the_trapezoid(bands, lib, device, spectral):
    lwb, swb = bands
    V, ncol = 16, 2
    cols = [syn.profile(330 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup((lwb, swb), device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 3, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    fine = (np.array([0, 1, 2, 60, 127, 128, 129, 200, 256, 257, 390, 398, 399], np.int32),
            np.array([5, 6, 100, 127, 128, 129, 130, 255, 256, 257, 400, 497, 498, 499], np.int32))
    api.check(lib.grt_set_deterministic(1))
    try:
        pipe.run_spectral(gcols, None, *fine)
        got = pipe.spectral(ncol)
        for lo, hi in ((0, 4), (2, 9), (3, 12)):
            union = (np.array([fine[0][lo], fine[0][min(hi, fine[0].size - 1)]], np.int32),
                     np.array([fine[1][lo], fine[1][min(hi, fine[1].size - 1)]], np.int32))
            pipe.run_spectral(gcols, None, *union)
            u = pipe.spectral(ncol)
            for bi, key in ((0, "lw"), (1, "sw")):
                h = min(hi, fine[bi].size - 1)
                parts = got[key + "_bins"][:, 0, :, lo:h]
                assert np.all(np.abs(parts.sum(axis=-1) - u[key + "_bins"][:, 0, :, 0])
                              <= 1e-12 * np.abs(parts).sum(axis=-1)), (key, lo, hi)
    finally:
        api.check(lib.grt_set_deterministic(-1))
    for bi, (band, key) in enumerate(((lwb, "lw"), (swb, "sw"))):
        e = fine[bi]
        rows, bins = got[key][:, 0], got[key + "_bins"][:, 0]
        for b in range(e.size - 1):
            if e[b + 1] == e[b] + 1:
                i = e[b]
                want = 0.5 * (rows[:, :, i] + rows[:, :, i + 1]) * band.dw
                assert np.all(np.abs(bins[:, :, b] - want) <= 1e-15 * np.abs(want)), (key, b)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


NS = (2, 127, 128, 129, 257)
shape_bands = make_shape_bands(NS, 100.0, 1000.0)


@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("n", NS)
def test_edge_shapes_against_the_oracle(shape_bands, tables, oracle, lib, device, n, spectral):
    """Grids around the 128-point block, V = 2 and 16, bins on and next to block boundaries, one-interval bins at both
    ends, num_bins = n - 1, columns of cos(zenith) 1, 0.5, 0.05 and 1e-3; clear sky and (V = 16: cloud_columns needs a
    few layers) all-sky."""
    lwb, swb = shape_bands[n]
    V = 2 if n in (2, 128) else 16
    user_level = V - 2 if V > 2 else -1
    cols = [syn.profile(400 + n + c, V) for c in range(len(MU0))]
    for c, mu in zip(cols, MU0):
        c["mu0"] = mu
    ncol = len(cols)
    go_lw, go_sw, emis, alb, solar = _setup((lwb, swb), device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 34) if V > 2 else None
    gclouds, keep_clouds = make(tables, cl) if V > 2 else (None, None)
    sets = 2 if V > 2 else 1
    every = np.arange(n, dtype=np.int32)
    want = {}
    for edges in ((block_edges(n), every), (every, block_edges(n))):
        pipe.run_spectral(gcols, gclouds, *edges)
        got = pipe.spectral(ncol)
        for c, col in enumerate(cols):
            for bi, (band, lw, key) in enumerate(((lwb, True, "lw"), (swb, False, "sw"))):
                for s in range(sets):
                    if (c, key, s) not in want:
                        cloud = None if s == 0 else (cl[key + "_liquid"][c], cl[key + "_ice"][c], cl["thickness"][c])
                        want[c, key, s] = oracle_rows(oracle, lib, band, col, lw, user_level, cloud, tables, emis, alb,
                                                      solar)
                    check_band(oracle, got[key][c, s], got[key + "_bins"][c, s], want[c, key, s], edges[bi], band.dw)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("spectral", [False, True])
def test_a_null_band_takes_no_room_and_its_bins_are_refused(bands, lib, device, spectral):
    lwb, swb = bands
    V, ncol = 16, 2
    cols = [syn.profile(340 + c, V) for c in range(ncol)]
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    both = _setup((lwb, swb), device, V)
    ref = api.Pipeline(*both[:2], ncol, -1, *both[2:], spectral=spectral)
    ref.run_spectral(gcols, None, block_edges(lwb.nw), block_edges(swb.nw))
    full = ref.spectral(ncol)
    ref.destroy()
    for missing in (0, 1):
        go_lw, go_sw, emis, alb, solar = _setup((lwb if missing else None, swb if not missing else None), device, V)
        pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=spectral)
        have = 1 - missing
        edges = [None, None]
        edges[have] = block_edges((lwb, swb)[have].nw)
        pipe.run_spectral(gcols, None, *edges)
        got = pipe.spectral(ncol)
        key, gone = ("lw", "sw")[have], ("lw", "sw")[missing]
        assert got[gone].shape == (ncol, 1, 6, 0) and got[gone + "_bins"].shape == (ncol, 1, 6, 0)
        scale = np.abs(full[key]).max()
        assert np.max(np.abs(got[key] - full[key])) <= 1e-9 * scale
        assert np.all(got["fluxes"][:, 6 * missing: 6 * missing + 6] == 0.0)
        bad = [None, None]
        bad[missing] = np.array([0, 1], np.int32)
        with pytest.raises(api.GrtError) as e:
            pipe.run_spectral(gcols, None, *bad)
        assert e.value.code == api.VALUE_ERR
        pipe.destroy()
        for g in (go_lw, go_sw):
            if g is not None:
                g.destroy()


def test_refused_inputs_launch_nothing(bands, tables, lib, device):
    lwb, swb = bands
    V, ncol = 16, 2
    cols = [syn.profile(350 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup((lwb, swb), device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 35)
    nl, ns = lwb.nw, swb.nw
    sentinel = -12345.0
    sizes = {"spectral": ncol * 2 * 6 * (nl + ns), "binned": ncol * 2 * 6 * 8, "fluxes": ncol * 24}
    bufs = {k: api.DeviceBuffer(device, 8 * v) for k, v in sizes.items()}

    def fill():
        for k, v in sizes.items():
            h = np.full(v, sentinel)
            api.check(lib.grt_host_to_device(device, bufs[k].ptr, h.ctypes.data_as(C.c_void_p), 8 * v))

    def refused(gc, gcl, le, lnb, se, snb, spectral=True, binned=True, fluxes=True):
        lp = None if le is None else np.ascontiguousarray(le, np.int32)
        sp = None if se is None else np.ascontiguousarray(se, np.int32)
        with pytest.raises(api.GrtError) as e:
            api.check(lib.grt_pipeline_run_spectral(
                pipe.p, C.byref(gc), C.byref(gcl) if gcl is not None else None,
                None if lp is None else lp.ctypes.data_as(C.c_void_p), lnb,
                None if sp is None else sp.ctypes.data_as(C.c_void_p), snb,
                bufs["spectral"].ptr if spectral else None, bufs["binned"].ptr if binned else None,
                bufs["fluxes"].ptr if fluxes else None))
        assert e.value.code == api.VALUE_ERR

    fill()
    ok = np.array([0, 10, nl - 1])
    refused(gcols, None, ok, 2, None, 0, spectral=False)
    refused(gcols, None, ok, 2, None, 0, fluxes=False)
    refused(gcols, None, ok, -1, None, 0)
    refused(gcols, None, None, 0, ok, -2)
    refused(gcols, None, None, 2, None, 0)                                      # bins without edges
    refused(gcols, None, ok, 2, None, 0, binned=False)                          # bins without binned_dev
    refused(gcols, None, np.array([0, 10, 10]), 2, None, 0)                     # not strictly increasing
    refused(gcols, None, np.array([0, 20, 10]), 2, None, 0)
    refused(gcols, None, np.array([-1, 10]), 1, None, 0)                        # outside 0 .. n - 1
    refused(gcols, None, np.array([0, nl]), 1, None, 0)
    refused(gcols, None, None, 0, np.array([0, ns]), 1)
    gcols.ncol = 0
    refused(gcols, None, ok, 2, None, 0)
    gcols.ncol = ncol + 1
    refused(gcols, None, ok, 2, None, 0)
    gcols.ncol = ncol
    g, k = make(tables, cl)
    g.num_liquid_bands = 0
    refused(gcols, g, ok, 2, None, 0)
    for field in ("thickness", "lw_liquid", "sw_ice"):
        g, k = make(tables, cl)
        setattr(g, field, None)
        refused(gcols, g, ok, 2, None, 0)
    pipe.sync()
    for k, v in sizes.items():
        assert np.all(bufs[k].to_host((v,)) == sentinel), k
    # and the same call accepted
    g, k = make(tables, cl)
    le = np.ascontiguousarray(ok, np.int32)
    api.check(lib.grt_pipeline_run_spectral(pipe.p, C.byref(gcols), C.byref(g), le.ctypes.data_as(C.c_void_p), 2, None,
                                            0, bufs["spectral"].ptr, bufs["binned"].ptr, bufs["fluxes"].ptr))
    pipe.sync()
    assert np.all(np.isfinite(bufs["fluxes"].to_host((sizes["fluxes"],))))
    for b in bufs.values():
        b.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_full_shortwave_width(tmp_path, tables, oracle, lib, device):
    """The bench's shortwave grid (1-50 000 cm-1 @ 1): two columns in the production form, all-sky, one of them against
    the oracle, 10 cm-1 bins."""
    band = Band(str(tmp_path), 1.0, 50000.0, 1.0, 2000, sw=True)
    V, ncol = 16, 2
    cols = [syn.profile(360 + c, V) for c in range(ncol)]
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 36)
    go, grid = band.gas_optics(device, V)
    solar = api.create_solar_flux(grid, band.files["solar"])
    alb = np.full(band.nw, 0.3)
    pipe = api.Pipeline(None, go, ncol, -1, None, alb, solar, spectral=False)
    gclouds, keep_clouds = api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), cl["thickness"], None, None,
                                           cl["sw_liquid"], cl["sw_ice"])
    edges = np.unique(np.append(np.arange(0, band.nw, 10), band.nw - 1)).astype(np.int32)
    pipe.run_spectral(gcols, gclouds, None, edges)
    got = pipe.spectral(ncol)
    pipe.destroy()
    go.destroy()
    for s in range(2):
        cloud = None if s == 0 else (cl["sw_liquid"][1], cl["sw_ice"][1], cl["thickness"][1])
        want = oracle_rows(oracle, lib, band, cols[1], False, -1, cloud, tables, alb=alb, solar=solar)
        check_band(oracle, got["sw"][1, s], got["sw_bins"][1, s], want, edges, band.dw)
    assert np.max(np.abs(got["sw"][:, 1] - got["sw"][:, 0])) > 0.0
