"""grt_pipeline_run_subcolumns: all-sky fluxes averaged over several cloud subcolumns per column, against the oracle's
literal restatement of driver.c:503-589 (per subcolumn: cloud optics, add_optics of four objects, the solver; the spectral
fluxes summed, divided by S, then integrated), against the single-subcolumn entry points, and in its averaging identities,
indexing, refusals and at the bench's shortwave width."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api, synthetic as syn
from pipeline_support import (KEYS, SETS, _deterministic, _sentinel, _setup, check_levels, limits, make,
                              oracle_subcolumns, pick, six, subcolumn_clouds)
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from scenario import Band, MOL_ORDER

pytestmark = pytest.mark.gpu

@pytest.mark.parametrize("spectral", [False, True])
def test_subcolumn_means_match_the_oracle(bands, tables, oracle, lib, device, spectral):
    lwb, swb = bands
    V, ncol, user_level, S = 16, 3, 5, 3
    cols = [syn.profile(210 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, 31, S)
    gclouds, keep_clouds = make(tables, cl)
    assert keep_clouds["subcolumns"] == S
    pipe.run_subcolumns(gcols, gclouds, S)
    clear6, cloudy6 = pipe.subcolumn_fluxes(ncol)
    pipe.run_subcolumns(gcols, gclouds, S, profiles=True)
    clear, cloudy = pipe.subcolumn_profiles(ncol)
    one = make(tables, pick(cl, subcolumns=[0]))
    pipe.run_allsky(gcols, one[0])
    first = pipe.allsky_fluxes(ncol)[1]
    spread = 0.0
    for c, col in enumerate(cols):
        for bi, (band, lw, key) in enumerate(((lwb, True, "lw"), (swb, False, "sw"))):
            w = oracle_subcolumns(oracle, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
                                  cl["thickness"][c], emis, alb, solar)
            assert np.max(np.abs(cloudy6[c, 6 * bi: 6 * bi + 6] - six(w["up_int"], w["dn_int"], user_level))) < 1e-9, key
            check_levels(cloudy, c, key, col, w["up_int"], w["dn_int"], closure=True)
            assert np.max(np.abs(cloudy["fluxes"][c, 6 * bi: 6 * bi + 6] - cloudy6[c, 6 * bi: 6 * bi + 6])) < 1e-9, key
            spread = max(spread, np.max(np.abs(cloudy6[c, 6 * bi: 6 * bi + 6] - first[c, 6 * bi: 6 * bi + 6])))
        assert np.max(np.abs(clear["fluxes"][c] - clear6[c])) < 1e-9
    assert spread > 1e-3                                            # the mean is not the first draw
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("two_sweeps", [None, "0", "1"])
def test_one_subcolumn_is_run_allsky(bands, tables, lib, device, two_sweeps, monkeypatch):
    V, ncol, user_level = 16, 3, 7
    cols = [syn.profile(220 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, 32, 1)
    g1, k1 = make(tables, cl)
    g0, k0 = make(tables, {k: (v[:, 0] if k in SETS else v) for k, v in cl.items()})     # [ncol][3][B][L]
    if two_sweeps is not None:
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", two_sweeps)
    _deterministic(lib, True)
    try:
        pipe.run_allsky(gcols, g0)
        want = np.concatenate(pipe.allsky_fluxes(ncol), axis=1)
        pipe.run_subcolumns(gcols, g1, 1)
        got = np.concatenate(pipe.subcolumn_fluxes(ncol), axis=1)
        pipe.run_allsky_profiles(gcols, g0)
        want_p = pipe.allsky_profiles(ncol)
        pipe.run_subcolumns(gcols, g1, 1, profiles=True)
        got_p = pipe.subcolumn_profiles(ncol)
    finally:
        _deterministic(lib, False)
    assert np.array_equal(got, want)
    assert not np.array_equal(got[:, 12:], got[:, :12])
    for s in range(2):
        for k in KEYS:
            assert np.array_equal(got_p[s][k], want_p[s][k]), k
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("profiles", [False, True])
def test_averaging_identities(bands, tables, lib, device, profiles):
    V, ncol, user_level = 16, 3, 6
    cols = [syn.profile(230 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, 33, 4)
    clear_cl = subcolumn_clouds(cols, tables, 34, 2, clear=True)

    def run(c, S):
        g, k = make(tables, c)
        pipe.run_subcolumns(gcols, g, S, profiles=profiles)
        if not profiles:
            return np.concatenate(pipe.subcolumn_fluxes(ncol), axis=1)
        out = pipe.subcolumn_profiles(ncol)
        return np.concatenate([np.concatenate([out[s][k].reshape(ncol, -1) for k in KEYS], axis=1) for s in range(2)],
                              axis=1)

    _deterministic(lib, True)
    try:
        base = run(pick(cl, subcolumns=[1]), 1)
        twice = run(pick(cl, subcolumns=[1, 1]), 2)
        five = run(pick(cl, subcolumns=[1] * 5), 5)
        fwd = run(cl, 4)
        rev = run(pick(cl, subcolumns=[3, 2, 1, 0]), 4)
        none = run(clear_cl, 2)
    finally:
        _deterministic(lib, False)
    assert np.array_equal(twice, base)
    scale = np.abs(base).max()
    assert np.max(np.abs(five - base)) <= 1e-15 * scale
    assert np.max(np.abs(rev - fwd)) <= 1e-13 * np.abs(fwd).max()
    assert not np.array_equal(fwd, base)
    h = none.shape[1] // 2
    assert np.array_equal(none[:, h:], none[:, :h])                # cloud-free subcolumns: the clear rows
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


@pytest.mark.parametrize("profiles", [False, True])
def test_a_column_does_not_depend_on_its_batch(bands, tables, lib, device, profiles):
    V, ncol, S, k = 16, 5, 4, 2
    cols = [syn.profile(240 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 9, emis, alb, solar, spectral=False)
    cl = subcolumn_clouds(cols, tables, 35, S)

    def run(order):
        gcols, keep = api.make_columns([cols[i] for i in order], MOL_ORDER, cfc_order=(0, 1))
        g, kc = make(tables, pick(cl, columns=order))
        pipe.run_subcolumns(gcols, g, S, profiles=profiles)
        n = len(order)
        if not profiles:
            return np.concatenate(pipe.subcolumn_fluxes(n), axis=1)
        out = pipe.subcolumn_profiles(n)
        return np.concatenate([np.concatenate([out[s][key].reshape(n, -1) for key in KEYS], axis=1) for s in range(2)],
                              axis=1)

    _deterministic(lib, True)
    try:
        batch = run(list(range(ncol)))
        alone = run([k])
        moved = run([4, 3, 2, 1, 0])
    finally:
        _deterministic(lib, False)
    assert np.array_equal(batch[k], alone[0])
    assert np.array_equal(batch[k], moved[ncol - 1 - k])
    assert np.array_equal(batch[::-1], moved)
    assert not np.array_equal(batch[k], batch[k + 1])
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_refused_inputs_and_no_interference(bands, tables, lib, device):
    V, ncol = 16, 3
    cols = [syn.profile(250 + c, V) for c in range(ncol)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, ncol, 7, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, 36, 8)
    g8, k8 = make(tables, cl)
    g0, k0 = make(tables, {k: (v[:, 0] if k in SETS else v) for k, v in cl.items()})
    outs = [_sentinel(device, ncol * n) for n in (8 * V, 4 * (V - 1), 24)]

    def refused(S, gcl=g8, level_ptr=outs[0].ptr, fluxes_ptr=outs[2].ptr):
        with pytest.raises(api.GrtError) as e:
            api.check(lib.grt_pipeline_run_subcolumns(pipe.p, C.byref(gcols), C.byref(gcl) if gcl is not None else None,
                                                      S, level_ptr, outs[1].ptr, fluxes_ptr))
        assert e.value.code == api.VALUE_ERR

    for S in (0, -1, api.GRT_MAX_SUBCOLUMNS + 1):
        refused(S)
        refused(S, level_ptr=None)
    refused(2, level_ptr=None, fluxes_ptr=None)
    refused(2, gcl=None)
    for field in SETS:
        g, k = make(tables, cl)
        setattr(g, field, None)
        refused(2, gcl=g)
        refused(2, gcl=g, level_ptr=None)
    pipe.sync()
    for buf, n in zip(outs, (8 * V, 4 * (V - 1), 24)):
        assert np.all(buf.to_host((ncol * n,)) == -7.25)
        buf.free()

    _deterministic(lib, True)
    try:
        pipe.run(gcols)
        run0 = pipe.fluxes(ncol)
        pipe.run_allsky(gcols, g0)
        allsky0 = pipe.allsky_fluxes(ncol)
        pipe.run_allsky_profiles(gcols, g0)
        prof0 = pipe.allsky_profiles(ncol)
        api.profile_enable(True)
        for tag in (api.TAG_ALLSKY_LW, api.TAG_ALLSKY_SW, api.TAG_SUBCOLUMN_MEAN):
            api.profile_read(tag, reset=True)
        pipe.run_subcolumns(gcols, g8, 8)
        means = pipe.subcolumn_fluxes(ncol)
        counts = {tag: api.profile_read(tag) for tag in (api.TAG_ALLSKY_LW, api.TAG_ALLSKY_SW, api.TAG_SUBCOLUMN_MEAN)}
        api.profile_enable(False)
        assert counts[api.TAG_ALLSKY_LW][1] == 1 and counts[api.TAG_ALLSKY_SW][1] == 1, counts
        assert counts[api.TAG_SUBCOLUMN_MEAN][1] == 2, counts
        assert all(ms > 0.0 for ms, n in counts.values())
        pipe.run_subcolumns(gcols, g8, 8, profiles=True)
        pmeans = pipe.subcolumn_profiles(ncol)
        pipe.run(gcols)
        assert np.array_equal(pipe.fluxes(ncol), run0)
        pipe.run_allsky(gcols, g0)
        allsky1 = pipe.allsky_fluxes(ncol)
        assert np.array_equal(allsky1[0], allsky0[0]) and np.array_equal(allsky1[1], allsky0[1])
        pipe.run_allsky_profiles(gcols, g0)
        prof1 = pipe.allsky_profiles(ncol)
        assert all(np.array_equal(prof1[s][k], prof0[s][k]) for s in range(2) for k in KEYS)
        assert np.array_equal(means[0], allsky0[0])
        assert all(np.array_equal(pmeans[0][k], prof0[0][k]) for k in KEYS)
    finally:
        api.profile_enable(False)
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_full_shortwave_width(tmp_path, tables, oracle, lib, device):
    """The bench's shortwave grid (1-50 000 cm-1 @ 1): one column, two subcolumns, the production form against the
    oracle."""
    band = Band(str(tmp_path), 1.0, 50000.0, 1.0, 2000, sw=True)
    V, S = 16, 2
    cols = [syn.profile(260, V)]
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, 37, S)
    go, grid = band.gas_optics(device, V)
    solar = api.create_solar_flux(grid, band.files["solar"])
    alb = np.full(band.nw, 0.3)
    pipe = api.Pipeline(None, go, 1, -1, None, alb, solar, spectral=False)
    gclouds, keep_clouds = api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), cl["thickness"], None, None,
                                           cl["sw_liquid"], cl["sw_ice"])
    pipe.run_subcolumns(gcols, gclouds, S)
    clear, cloudy = pipe.subcolumn_fluxes(1)
    pipe.destroy()
    go.destroy()
    w = oracle_subcolumns(oracle, lib, band, cols[0], False, tables, cl["sw_liquid"][0], cl["sw_ice"][0],
                          cl["thickness"][0], alb=alb, solar=solar)
    want = six(w["up_int"], w["dn_int"], -1)
    assert np.max(np.abs(cloudy[0, 6:] - want)) <= 1e-12 * np.abs(want).max()
    assert np.max(np.abs(cloudy[:, 6:] - clear[:, 6:])) > 0.5
