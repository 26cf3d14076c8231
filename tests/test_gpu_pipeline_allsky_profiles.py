"""grt_pipeline_run_allsky_profiles: the broadband flux at every level and the heating rate of every layer, clear sky and
all-sky, from one batched call -- against the oracle's column-by-column restatement of driver.c:474-597 level by level,
against the pipeline's own run_profiles and run_allsky, and at the bench's shortwave width."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api, synthetic as syn
from pipeline_support import (KEYS, LEVEL_KEYS, _sentinel, _setup, check_levels, cloud_columns, heating, limits, make,
                              oracle_allsky_levels, oracle_column)
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from scenario import Band, MOL_ORDER

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("spectral", [False, True])
def test_level_fluxes_and_heating_rates_match_the_oracle(bands, tables, oracle, lib, device, spectral):
    lwb, swb = bands
    V, ncol, user_level = 16, 3, 5
    cols = [syn.profile(110 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 21)
    gclouds, keep_clouds = make(tables, cl)
    pipe.run_allsky_profiles(gcols, gclouds)
    clear, cloudy = pipe.allsky_profiles(ncol)
    largest = 0.0
    for c, col in enumerate(cols):
        for band, lw, key in ((lwb, True, "lw"), (swb, False, "sw")):
            w = oracle_column(oracle, lib, band, col, lw, emis, alb, solar, user_level)
            want_up = np.array([oracle.integrate_row(w["up"][k], band.dw) for k in range(V)])
            want_dn = np.array([oracle.integrate_row(w["dn"][k], band.dw) for k in range(V)])
            check_levels(clear, c, key, col, want_up, want_dn, closure=True)
            a = oracle_allsky_levels(oracle, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
                                     cl["thickness"][c], emis, alb, solar)
            check_levels(cloudy, c, key, col, a["up_int"], a["dn_int"], closure=True)
            # every column has an overcast layer: the clouds change its all-sky rows
            effect = max(np.abs(cloudy[key + "_up"][c] - clear[key + "_up"][c]).max(),
                         np.abs(cloudy[key + "_down"][c] - clear[key + "_down"][c]).max())
            assert effect > 1e-3, key
            largest = max(largest, effect)
        for s in (clear, cloudy):
            assert np.all(s["fluxes"][c, [2, 5, 8, 11]] != 0.0)                         # a user level was asked for
    assert largest > 0.5                                                                # the clouds matter
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("user_level", [-1, 0, 7, 15])
def test_sets_are_run_profiles_and_run_allsky(bands, tables, lib, device, user_level, monkeypatch):
    V, ncol = 16, 3
    L = V - 1
    cols = [syn.profile(120 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, cloud_columns(cols, tables, 22))
    api.check(lib.grt_set_deterministic(1))
    try:
        pipe.run_profiles(gcols)
        prof = pipe.profiles(ncol)
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "0")
        pipe.run_allsky(gcols, gclouds)
        one = np.concatenate(pipe.allsky_fluxes(ncol), axis=1)
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        pipe.run_allsky(gcols, gclouds)
        two = np.concatenate(pipe.allsky_fluxes(ncol), axis=1)
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        pipe.run_allsky_profiles(gcols, gclouds)
        clear, cloudy = pipe.allsky_profiles(ncol)
    finally:
        api.check(lib.grt_set_deterministic(-1))
    for k in KEYS:
        assert np.array_equal(clear[k], prof[k]), k
    for bi, key in ((0, "lw"), (1, "sw")):
        up, dn = cloudy[key + "_up"], cloudy[key + "_down"]
        six = two[:, 12 + 6 * bi: 12 + 6 * bi + 6]
        assert np.array_equal(up[:, 0], six[:, 0]) and np.array_equal(up[:, L], six[:, 1])
        assert np.array_equal(dn[:, 0], six[:, 3]) and np.array_equal(dn[:, L], six[:, 4])
        if user_level >= 0:
            assert np.array_equal(up[:, user_level], six[:, 2]) and np.array_equal(dn[:, user_level], six[:, 5])
        else:
            assert np.all(six[:, [2, 5]] == 0.0)
    got = np.concatenate([clear["fluxes"], cloudy["fluxes"]], axis=1)
    assert np.array_equal(got, two)
    assert np.max(np.abs(got - one)) <= 1e-13 * np.abs(one).max()          # the default one-sweep shortwave
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("spectral", [False, True])
def test_no_cloud_gives_the_clear_rows(bands, tables, lib, device, spectral):
    V, ncol = 16, 2
    cols = [syn.profile(130 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 4, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 23, clear=True)
    assert all(np.all(cl[k][:, 0] == 0.0) for k in ("lw_liquid", "lw_ice", "sw_liquid", "sw_ice"))
    gclouds, keep_clouds = make(tables, cl)
    pipe.run_allsky_profiles(gcols, gclouds)
    clear, cloudy = pipe.allsky_profiles(ncol)
    for k in KEYS:
        assert np.array_equal(clear[k], cloudy[k]), k
    assert np.all(clear["lw_up"] > 0.0) and np.all(clear["sw_down"][:, 0] > 0.0)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_repeatable_and_no_interference(bands, tables, lib, device):
    V, ncol = 16, 3
    cols = [syn.profile(140 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 7, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, cloud_columns(cols, tables, 24))
    api.check(lib.grt_set_deterministic(1))
    try:
        pipe.run(gcols)
        run0 = pipe.fluxes(ncol)
        pipe.run_profiles(gcols)
        prof0 = pipe.profiles(ncol)
        pipe.run_allsky(gcols, gclouds)
        allsky0 = pipe.allsky_fluxes(ncol)
        api.profile_enable(True)
        for tag in (api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_ALLSKY_LW, api.TAG_ALLSKY_SW):
            api.profile_read(tag, reset=True)
        pipe.run_allsky_profiles(gcols, gclouds)
        a = pipe.allsky_profiles(ncol)
        counts = {tag: api.profile_read(tag) for tag in (api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_ALLSKY_LW, api.TAG_ALLSKY_SW)}
        api.profile_enable(False)
        for tag, (ms, n) in counts.items():
            assert n == 1 and ms > 0.0, tag                 # one clear-sky (3, 4) and one all-sky (8, 9) solver per band
        pipe.run_allsky_profiles(gcols, gclouds)
        b = pipe.allsky_profiles(ncol)
        for s in range(2):
            assert all(np.array_equal(a[s][k], b[s][k]) for k in KEYS)
        pipe.run(gcols)
        assert np.array_equal(pipe.fluxes(ncol), run0)
        pipe.run_profiles(gcols)
        prof1 = pipe.profiles(ncol)
        assert all(np.array_equal(prof1[k], prof0[k]) for k in KEYS)
        pipe.run_allsky(gcols, gclouds)
        allsky1 = pipe.allsky_fluxes(ncol)
        assert np.array_equal(allsky1[0], allsky0[0]) and np.array_equal(allsky1[1], allsky0[1])
    finally:
        api.profile_enable(False)
        api.check(lib.grt_set_deterministic(-1))
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_edge_cases(bands, tables, lib, device):
    V, ncol = 16, 2
    cols = [syn.profile(150 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 25)
    gclouds, keep_clouds = make(tables, cl)
    # NULL heating_dev and fluxes_dev are accepted: the same levels
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    api.check(lib.grt_set_deterministic(1))
    try:
        pipe.run_allsky_profiles(gcols, gclouds)
        want = pipe.allsky_profiles(ncol)
        levels = api.DeviceBuffer(device, 8 * ncol * 8 * V)
        api.check(lib.grt_pipeline_run_allsky_profiles(pipe.p, C.byref(gcols), C.byref(gclouds), levels.ptr, None, None))
        pipe.sync()
        lv = levels.to_host((ncol, 2, 4, V))
        levels.free()
    finally:
        api.check(lib.grt_set_deterministic(-1))
    for s in range(2):
        for r, k in enumerate(LEVEL_KEYS):
            assert np.array_equal(lv[:, s, r], want[s][k]), k

    # refused inputs: GRTCODE_VALUE_ERR, nothing launched -- sentinel-filled outputs untouched after a sync
    outs = [_sentinel(device, (ncol + 1) * n) for n in (8 * V, 4 * (V - 1), 24)]

    def refused(gc, gcl, level_ptr=outs[0].ptr):
        with pytest.raises(api.GrtError) as e:
            api.check(lib.grt_pipeline_run_allsky_profiles(pipe.p, C.byref(gc), C.byref(gcl) if gcl is not None else None,
                                                           level_ptr, outs[1].ptr, outs[2].ptr))
        assert e.value.code == api.VALUE_ERR

    refused(gcols, gclouds, None)
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
    big_cols = [syn.profile(150 + c, V) for c in range(ncol + 1)]
    big, keep_big = api.make_columns(big_cols, MOL_ORDER, cfc_order=(0, 1))
    g, k = make(tables, cloud_columns(big_cols, tables, 25))
    refused(big, g)
    gcols.ncol = 0
    refused(gcols, gclouds)
    gcols.ncol = ncol
    pipe.sync()
    for buf, n in zip(outs, (8 * V, 4 * (V - 1), 24)):
        assert np.all(buf.to_host(((ncol + 1) * n,)) == -7.25)
        buf.free()
    pipe.destroy()

    # one band only: the other band's rows are zero in both sets
    for lw_only in (True, False):
        if lw_only:
            pipe = api.Pipeline(go_lw, None, ncol, -1, emis, None, None, spectral=False)
            g, k = api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), cl["thickness"], cl["lw_liquid"],
                                   cl["lw_ice"], None, None)
        else:
            pipe = api.Pipeline(None, go_sw, ncol, -1, None, alb, solar, spectral=False)
            g, k = api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), cl["thickness"], None, None,
                                   cl["sw_liquid"], cl["sw_ice"])
        pipe.run_allsky_profiles(gcols, g)
        got = pipe.allsky_profiles(ncol)
        off, on = ("sw", "lw") if lw_only else ("lw", "sw")
        for s in range(2):
            for k in ("_up", "_down", "_heating"):
                assert np.all(got[s][off + k] == 0.0), off + k
                assert np.all(np.isfinite(got[s][on + k])), on + k
            assert np.abs(got[s][on + "_heating"]).max() > 0.0
            f = got[s]["fluxes"]
            assert np.all((f[:, 6:] if lw_only else f[:, :6]) == 0.0)
        assert np.abs(got[1][on + "_down"] - got[0][on + "_down"]).max() > 1e-3    # the clouds reached the band
        pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_full_shortwave_width(tmp_path, tables, oracle, lib, device):
    """The bench's shortwave grid (1-50 000 cm-1 @ 1) at 61 levels: two columns in the production form, the all-sky
    levels of one against the oracle."""
    band = Band(str(tmp_path), 1.0, 50000.0, 1.0, 2000, sw=True)
    V, ncol = 61, 2
    cols = [syn.profile(160 + c, V) for c in range(ncol)]
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = cloud_columns(cols, tables, 26)
    go, grid = band.gas_optics(device, V)
    solar = api.create_solar_flux(grid, band.files["solar"])
    alb = np.full(band.nw, 0.3)
    pipe = api.Pipeline(None, go, ncol, -1, None, alb, solar, spectral=False)
    gclouds, keep_clouds = api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), cl["thickness"], None, None,
                                           cl["sw_liquid"], cl["sw_ice"])
    pipe.run_allsky_profiles(gcols, gclouds)
    clear, cloudy = pipe.allsky_profiles(ncol)
    pipe.destroy()
    go.destroy()
    w = oracle_allsky_levels(oracle, lib, band, cols[1], False, tables, cl["sw_liquid"][1], cl["sw_ice"][1],
                             cl["thickness"][1], alb=alb, solar=solar)
    scale = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
    assert scale > 0.0
    assert np.max(np.abs(cloudy["sw_up"][1] - w["up_int"])) <= 1e-12 * scale
    assert np.max(np.abs(cloudy["sw_down"][1] - w["dn_int"])) <= 1e-12 * scale
    assert np.max(np.abs(cloudy["sw_down"] - clear["sw_down"])) > 0.5
    for s in (clear, cloudy):
        for c, col in enumerate(cols):
            want = heating(s["sw_up"][c], s["sw_down"][c], col["p"])
            assert np.max(np.abs(s["sw_heating"][c] - want)) <= 1e-12 * np.abs(want).max()
    assert np.all(cloudy["lw_up"] == 0.0) and np.all(cloudy["lw_heating"] == 0.0)
