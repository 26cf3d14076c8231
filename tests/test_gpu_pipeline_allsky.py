"""grt_pipeline_run_allsky: the all-sky (cloudy, aerosol-free) fluxes of the batched pipeline, against the oracle's
column-by-column restatement of driver.c:474-597 (gas, Rayleigh, liquid and ice cloud through add_optics of four objects,
the same solvers), against the pipeline's own clear-sky pass, and at the bench's shortwave width."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api, synthetic as syn
from pipeline_support import _setup, cloud_columns, limits, make, oracle_allsky_column, oracle_column
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from scenario import Band, MOL_ORDER

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("spectral", [False, True])
def test_allsky_fluxes_match_the_oracle(bands, tables, oracle, lib, device, spectral):
    lwb, swb = bands
    V, ncol, user_level = 16, 3, 5
    L = V - 1
    cols = [syn.profile(60 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 11)
    gclouds, keep_clouds = make(tables, cl)
    pipe.run_allsky(gcols, gclouds)
    clear, cloudy = pipe.allsky_fluxes(ncol)
    if spectral:
        views = [pipe.views(bi) for bi in range(2)]
        got_opt = [{k: api.device_to_host(device, v[k], (ncol, L, band.nw)) for k in ("tau", "omega", "g")}
                   for v, band in zip(views, bands)]
    effect = 0.0
    for bi, (band, lw, key) in enumerate(((lwb, True, "lw"), (swb, False, "sw"))):
        for c, col in enumerate(cols):
            want_clear = oracle_column(oracle, lib, band, col, lw, emis, alb, solar, user_level)["integ"]
            w = oracle_allsky_column(oracle, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
                                     cl["thickness"][c], emis, alb, solar, user_level)
            assert np.max(np.abs(clear[c, 6 * bi: 6 * bi + 6] - want_clear)) < 1e-9, key
            assert np.max(np.abs(cloudy[c, 6 * bi: 6 * bi + 6] - w["integ"])) < 1e-9, key
            effect = max(effect, np.max(np.abs(w["integ"] - want_clear)))
            assert np.any(w["maps"][0] < 0)                     # the gap: points with no liquid band
            if spectral:
                o = got_opt[bi]
                assert np.max(np.abs(o["tau"][c] - w["tau"]) / np.abs(w["tau"]).max(axis=1, keepdims=True)) < 1e-11
                assert np.max(np.abs(o["omega"][c] - w["omega"])) < 1e-11
                assert np.max(np.abs(o["g"][c] - w["g"])) < 1e-11
                assert np.max(np.abs(w["g"])) > 0.1                 # cloud asymmetry reached the combination
    assert effect > 0.5                                             # the clouds matter
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_clear_rows_are_runs_and_run_is_undisturbed(bands, tables, lib, device):
    V, ncol = 16, 3
    cols = [syn.profile(70 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 7, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, cloud_columns(cols, tables, 12))
    api.check(lib.grt_set_deterministic(1))
    try:
        pipe.run(gcols)
        first = pipe.fluxes(ncol)
        api.profile_enable(True)
        pipe.run_allsky(gcols, gclouds)
        clear, cloudy = pipe.allsky_fluxes(ncol)
        lw_ms, lw_n = api.profile_read(api.TAG_ALLSKY_LW)
        sw_ms, sw_n = api.profile_read(api.TAG_ALLSKY_SW)
        api.profile_enable(False)
        assert np.array_equal(clear, first)
        assert not np.array_equal(cloudy, first)
        assert lw_n == 1 and sw_n == 1 and lw_ms > 0.0 and sw_ms > 0.0     # the all-sky solvers' tags
        pipe.run_allsky(gcols, gclouds)
        again = pipe.allsky_fluxes(ncol)
        assert np.array_equal(again[0], clear) and np.array_equal(again[1], cloudy)
        pipe.run(gcols)
        assert np.array_equal(pipe.fluxes(ncol), first)
    finally:
        api.profile_enable(False)
        api.check(lib.grt_set_deterministic(-1))
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("spectral", [False, True])
def test_no_cloud_gives_the_clear_rows(bands, tables, lib, device, spectral):
    V, ncol = 16, 2
    cols = [syn.profile(75 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 4, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 13, clear=True)
    assert all(np.all(cl[k][:, 0] == 0.0) for k in ("lw_liquid", "lw_ice", "sw_liquid", "sw_ice"))
    gclouds, keep_clouds = make(tables, cl)
    pipe.run_allsky(gcols, gclouds)
    clear, cloudy = pipe.allsky_fluxes(ncol)
    assert np.array_equal(clear, cloudy)
    assert np.all(clear[:, [0, 6]] > 0.0)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_refused_inputs(bands, tables, lib, device):
    V, ncol = 16, 2
    cols = [syn.profile(50 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 14)
    out = api.DeviceBuffer(device, 8 * api.GRT_ALLSKY_FLUXES_PER_COLUMN * (ncol + 1))

    def refused(gc, gcl):
        with pytest.raises(api.GrtError) as e:
            api.check(lib.grt_pipeline_run_allsky(pipe.p, C.byref(gc), C.byref(gcl) if gcl is not None else None, out.ptr))
        assert e.value.code == api.VALUE_ERR

    refused(gcols, None)
    g, k = make(tables, cl)
    g.num_liquid_bands = 0
    refused(gcols, g)
    g, k = make(tables, cl)
    g.num_ice_bands = g.num_liquid_bands - 1
    refused(gcols, g)
    for field in ("liquid_band_lo", "liquid_band_hi", "ice_band_lo", "ice_band_hi", "thickness", "lw_liquid", "lw_ice",
                  "sw_liquid", "sw_ice"):
        g, k = make(tables, cl)
        setattr(g, field, None)
        refused(gcols, g)
    big, keep_big = api.make_columns([syn.profile(50 + c, V) for c in range(ncol + 1)], MOL_ORDER, cfc_order=(0, 1))
    g, k = make(tables, cloud_columns([syn.profile(50 + c, V) for c in range(ncol + 1)], tables, 14))
    refused(big, g)
    gcols.ncol = 0
    g, k = make(tables, cl)
    refused(gcols, g)
    gcols.ncol = ncol
    api.check(lib.grt_pipeline_run_allsky(pipe.p, C.byref(gcols), C.byref(g), out.ptr))      # and the same call accepted
    pipe.sync()
    assert np.all(np.isfinite(out.to_host((ncol + 1, 24))[:ncol]))
    out.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_full_shortwave_width(tmp_path, tables, oracle, lib, device):
    """The bench's shortwave grid (1-50 000 cm-1 @ 1): two columns in the production form, one of them against the oracle."""
    band = Band(str(tmp_path), 1.0, 50000.0, 1.0, 2000, sw=True)
    V, ncol = 16, 2
    cols = [syn.profile(90 + c, V) for c in range(ncol)]
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 15)
    go, grid = band.gas_optics(device, V)
    solar = api.create_solar_flux(grid, band.files["solar"])
    alb = np.full(band.nw, 0.3)
    pipe = api.Pipeline(None, go, ncol, -1, None, alb, solar, spectral=False)
    gclouds, keep_clouds = api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), cl["thickness"], None, None,
                                           cl["sw_liquid"], cl["sw_ice"])
    pipe.run_allsky(gcols, gclouds)
    clear, cloudy = pipe.allsky_fluxes(ncol)
    pipe.destroy()
    go.destroy()
    w = oracle_allsky_column(oracle, lib, band, cols[1], False, tables, cl["sw_liquid"][1], cl["sw_ice"][1],
                             cl["thickness"][1], alb=alb, solar=solar)
    scale = np.abs(w["integ"]).max()
    assert np.max(np.abs(cloudy[1, 6:] - w["integ"])) <= 1e-12 * scale
    assert np.max(np.abs(cloudy[:, 6:] - clear[:, 6:])) > 0.5
