"""grt_pipeline_run_sky_scattering: grt_pipeline_run_sky, and with it the scattering correction of every set's longwave.
The corrections against the float64 model (tests/lw_scatter_model.py) applied to the layer optics the other sky tests
build on the CPU -- add_optics of {gas, Rayleigh, aerosol, liquid, ice} per subcolumn, the mean over the draws, the
trapezoid --, fused and materialised, six-row and profile form, one draw and several, the clean set alone and all four;
the bit-for-bit identities with grt_pipeline_run_sky and within the entry point; what it refuses.

The clouds' longwave single-scattering albedo is this module's own input, up to 0.8: before the device is compared, the
model itself must show a cloud set's upward correction at the top to be negative and at least 1e-3 of the set's upward
flux there, so that an entry point that hands back zeros cannot pass."""
import ctypes as C

import numpy as np
import pytest

import lw_scatter_model as m
from aerosol_model import AEROSOL_GRID, aerosol_fields, oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from grtcode_amd import api, synthetic as syn
from pipeline_support import (CP, GRAVITY, LEVEL_TOL, _deterministic, _sentinel, _setup, cached, heating, limits, make, pick,
                              subcolumn_clouds)
from pipeline_support import bands, oracle_cache, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

CLEAN, AEROSOL, CLOUD, BOTH, ALL = (api.GRT_SKY_CLEAN, api.GRT_SKY_AEROSOL, api.GRT_SKY_CLOUD,
                                    api.GRT_SKY_CLOUD_AEROSOL, api.GRT_SKY_ALL)
NAMES = ("clean", "aerosol", "cloud", "both")
V1, UL1, S_MAX = 16, 5, 3
L1 = V1 - 1


# ---- inputs -------------------------------------------------------------------------------------------------------------- #
class Case:
    def __init__(self, tables):
        self.cols = []
        for c, (fp, mu) in enumerate(zip((1.0, 0.9, 1.03), (0.6, 1.0, 0.3))):
            col = syn.profile(700 + c, V1)
            col["p"] = col["p"] * fp
            col["mu0"] = mu
            self.cols.append(col)
        self.ncol = len(self.cols)
        self.cl = subcolumn_clouds(self.cols, tables, 91, S_MAX)
        # the longwave clouds scatter: albedo 0.3 .. 0.8 and asymmetry 0.6 .. 0.9 wherever a table holds a cloud
        rng = np.random.default_rng(17)
        for k in ("lw_liquid", "lw_ice"):
            a = self.cl[k]                                           # [ncol][S][3][B][L]
            cloudy = a[:, :, 0] > 0.0
            a[:, :, 1] = np.where(cloudy, rng.uniform(0.3, 0.8, cloudy.shape), 0.0)
            a[:, :, 2] = np.where(cloudy, rng.uniform(0.6, 0.9, cloudy.shape), 0.0)
        self.f = (aerosol_fields(self.ncol, L1, AEROSOL_GRID, 93, lw=True), aerosol_fields(self.ncol, L1, AEROSOL_GRID, 94, lw=False))

    def clouds(self, S, columns=None):
        return pick(self.cl, columns=columns, subcolumns=range(S))


@pytest.fixture(scope="module")
def case(tables):
    return Case(tables)


def aerosols_of(f):
    return api.make_aerosols(lw=(AEROSOL_GRID, f[0]), sw=(AEROSOL_GRID, f[1]))


def run_sky(pipe, gcols, gclouds, gaer, S, sets, ncol, profiles, scattering):
    """-> (run_sky's outputs as dicts of [ncol][nsets][..] arrays, the corrections: scatter [ncol][nsets][6] and, profile
    form, scatter_up, scatter_down [ncol][nsets][V]; None without scattering)"""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    n = keep["nsets"]
    if scattering:
        pipe.run_sky_scattering(gcols, gsky, profiles=profiles)
        sc = pipe.sky_scatter_profiles(ncol, n) if profiles else dict(scatter=pipe.sky_scatter_fluxes(ncol, n))
    else:
        pipe.run_sky(gcols, gsky, profiles=profiles)
        sc = None
    return (pipe.sky_profiles(ncol, n) if profiles else dict(fluxes=pipe.sky_fluxes(ncol, n))), sc


def positions(sets):
    bits = [b for b in (CLEAN, AEROSOL, CLOUD, BOTH) if (sets | CLEAN) & b]
    return {NAMES[(CLEAN, AEROSOL, CLOUD, BOTH).index(b)]: k for k, b in enumerate(bits)}


# ---- the model on the CPU's layer optics --------------------------------------------------------------------------------- #
def model_sets(orc, lib, band, col, tables, liquid, ice, thickness, x, optics, emis):
    """The four sets of one column of the longwave band, in bit order: dict(up, down [V]: the integrated correction, the
    mean over the S draws of liquid / ice [S][3][B][L]; flux_up, flux_down [V]: the scattering solve's own, likewise)."""
    L, S, B = col["p"].size - 1, liquid.shape[0], liquid.shape[2]
    w = driver_limits(band.w0, band.dw, band.nw)
    (llo, lhi), (ilo, ihi) = limits(tables, "liquid"), limits(tables, "ice")
    maps = (band_map(llo, lhi, B, B, w), band_map(ilo, ihi, ilo.size, B, w))
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    aer = oracle_aerosol_optics(orc, band, x, optics)
    wn = band.w0 + band.dw * np.arange(band.nw)

    def solve(objects):
        tau, omega, g = orc.add_optics(*[list(o) for o in zip(*objects)])
        res = m.scatter_delta(tau.T, omega.T, g.T, col["t_layer"], col["t"], col["t_surf"], emis, wn)
        return [r.T for r in res]                                    # [V][nw] each

    def integrated(rows):
        return np.array([orc.integrate_row(np.ascontiguousarray(r), band.dw) for r in rows])

    def one(objects):
        return [integrated(r) for r in solve(objects)]

    def mean(per_draw):
        return [sum(d[k] for d in per_draw) / float(S) if S > 1 else per_draw[0][k] for k in range(4)]

    gas, ray, aerosol = (tau_gas, z, z), (tr, om_r, g_r), (aer[0], aer[1], aer[2])
    draws = []
    for j in range(S):
        lt, lo, lg, it, io, ig = grid_optics(liquid[j], ice[j], thickness, maps)
        draws.append(((lt, lo, lg), (it, io, ig)))
    sets = [one([gas, ray]), one([gas, ray, aerosol]), mean([one([gas, ray, li, ic]) for li, ic in draws]),
            mean([one([gas, ray, aerosol, li, ic]) for li, ic in draws])]
    return [dict(up=s[0], down=s[1], flux_up=s[2], flux_down=s[3]) for s in sets]


def six_of(up, down, user_level):
    u = user_level
    return np.array([up[0], up[-1], up[u] if u >= 0 else 0.0, down[0], down[-1], down[u] if u >= 0 else 0.0])


def model_of(cache, orc, lib, band, tables, case, emis, S):
    cl = case.clouds(S)
    return [cached(cache, ("scatter", c, S), lambda: model_sets(orc, lib, band, col, tables, cl["lw_liquid"][c], cl["lw_ice"][c],
                                                                cl["thickness"][c], AEROSOL_GRID, case.f[0][c], emis))
            for c, col in enumerate(case.cols)]


# ---- 1. against the model, and the identities ---------------------------------------------------------------------------- #
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_corrections_match_the_model_and_add_up(bands, tables, oracle, oracle_cache, case, lib, device, S, spectral):
    cols, ncol, L = case.cols, case.ncol, L1
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    want = model_of(oracle_cache, oracle, lib, bands[0], tables, case, emis, S)
    # the model's own numbers first: the cloud sets' correction is there, and has the sign of a scattering cloud
    for c in range(ncol):
        for k in (2, 3):
            w = want[c][k]
            print("model, column", c, NAMES[k], "delta_up at the top", w["up"][0], "of", w["flux_up"][0],
                  "delta_down at the surface", w["down"][-1])
            assert w["up"][0] < 0.0 and -w["up"][0] >= 1e-3 * w["flux_up"][0], (c, k)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case.clouds(S)
    gclouds, keep_clouds = make(tables, cl)
    gaer, keep_aer = aerosols_of(case.f)
    _deterministic(lib, True)
    try:
        full = {}
        for profiles in (False, True):
            base, _ = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles, False)
            out, sc = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles, True)
            again, _ = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles, False)
            assert all(np.array_equal(base[k], again[k]) for k in base), profiles      # run_sky is what it was
            full[profiles] = (out, sc)
            assert sc["scatter"].shape == (ncol, 4, 6)
            # against the model
            for c in range(ncol):
                for k in range(4):
                    w = want[c][k]
                    ff = max(np.abs(w["flux_up"]).max(), np.abs(w["flux_down"]).max())
                    err = np.max(np.abs(sc["scatter"][c, k] - six_of(w["up"], w["down"], UL1)))
                    print("column", c, NAMES[k], "six rows", err / ff, "of scale")
                    assert err <= LEVEL_TOL * ff, (profiles, c, k, err, ff)
                    if profiles:
                        for name, key in (("scatter_up", "up"), ("scatter_down", "down")):
                            err = np.max(np.abs(sc[name][c, k] - w[key]))
                            assert err <= LEVEL_TOL * ff, (name, c, k, err, ff)
            # corrected == run_sky + delta, one addition; the shortwave is run_sky's
            assert np.array_equal(out["fluxes"][:, :, 6:], base["fluxes"][:, :, 6:])
            if profiles:
                assert np.array_equal(out["lw_up"], base["lw_up"] + sc["scatter_up"])
                assert np.array_equal(out["lw_down"], base["lw_down"] + sc["scatter_down"])
                assert np.array_equal(out["sw_up"], base["sw_up"]) and np.array_equal(out["sw_down"], base["sw_down"])
                assert np.array_equal(out["sw_heating"], base["sw_heating"])
                assert np.array_equal(out["fluxes"][:, :, 0:3], out["lw_up"][:, :, [0, L, UL1]])
                assert np.array_equal(out["fluxes"][:, :, 3:6], out["lw_down"][:, :, [0, L, UL1]])
                assert np.array_equal(sc["scatter"][:, :, 0:3], sc["scatter_up"][:, :, [0, L, UL1]])
                assert np.array_equal(sc["scatter"][:, :, 3:6], sc["scatter_down"][:, :, [0, L, UL1]])
                assert np.all(sc["scatter_down"][:, :, 0] == 0.0)
                # the heating rates are the corrected levels'
                for c, col in enumerate(cols):
                    hr = out["lw_heating"][c]
                    assert np.max(np.abs(hr - heating(out["lw_up"][c], out["lw_down"][c], col["p"]))) <= 1e-12 * np.abs(hr).max()
                assert not np.array_equal(out["lw_heating"], base["lw_heating"])
            else:
                assert np.array_equal(out["fluxes"][:, :, :6], base["fluxes"][:, :, :6] + sc["scatter"])
            # every set has a correction: Rayleigh alone makes the clean set's tiny, not zero
            assert np.all(sc["scatter"][:, :, 0] != 0.0)
            assert np.all(np.abs(sc["scatter"][:, 0, 0]) < 1e-3 * np.abs(sc["scatter"][:, 2, 0]))
            # any subset of the four: each of its sets has the bits it has in the four-set run
            for mask in (CLEAN, AEROSOL, CLOUD, BOTH, CLOUD | BOTH, AEROSOL | CLOUD):
                sub, ssc = run_sky(pipe, gcols, gclouds if mask & (CLOUD | BOTH) else None,
                                   gaer if mask & (AEROSOL | BOTH) else None, S, mask, ncol, profiles, True)
                for name, k in positions(mask).items():
                    q = NAMES.index(name)
                    assert all(np.array_equal(sub[key][:, k], out[key][:, q]) for key in out), (mask, name, profiles)
                    assert all(np.array_equal(ssc[key][:, k], sc[key][:, q]) for key in sc), (mask, name, profiles)
            # a column alone has the bits it has in its batch
            c = 1
            g1, k1 = api.make_columns(cols[c:c + 1], MOL_ORDER, cfc_order=(0, 1))
            c1, kc1 = make(tables, case.clouds(S, columns=[c]))
            a1, ka1 = aerosols_of(tuple(f[c:c + 1] for f in case.f))
            alone, asc = run_sky(pipe, g1, c1, a1, S, ALL, 1, profiles, True)
            assert all(np.array_equal(alone[k][0], out[k][c]) for k in out), profiles
            assert all(np.array_equal(asc[k][0], sc[k][c]) for k in sc), profiles
        # the six-row form's corrections are rows 0, L and the user level of the profile form's
        assert np.array_equal(full[False][1]["scatter"], full[True][1]["scatter"])
        assert np.array_equal(full[False][0]["fluxes"][:, :, :6], full[True][0]["fluxes"][:, :, :6])
        if S > 1:
            # room for every draw of every column in one launch: the bits of the launches split by the park block
            wide = api.Pipeline(go_lw, go_sw, ncol * S, UL1, emis, alb, solar, spectral=spectral)
            for profiles in (False, True):
                out1, sc1 = run_sky(wide, gcols, gclouds, gaer, S, ALL, ncol, profiles, True)
                out, sc = full[profiles]
                assert all(np.array_equal(out1[k], out[k]) for k in out), profiles
                assert all(np.array_equal(sc1[k], sc[k]) for k in sc), profiles
            wide.destroy()
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_the_pass_has_profile_tags_of_its_own(bands, tables, case, lib, device):
    cols, ncol, S = case.cols, case.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, case.clouds(S))
    gaer, keep_aer = aerosols_of(case.f)
    api.profile_enable(True)
    try:
        api.profile_read(api.TAG_GAS_LW, reset=True)
        run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, False, False)
        assert api.profile_read(api.TAG_SCATTER_LW)[1] == 0 and api.profile_read(api.TAG_SCATTER_FINISH)[1] == 0
        api.profile_read(api.TAG_GAS_LW, reset=True)
        run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, False, True)
        ms, launches = api.profile_read(api.TAG_SCATTER_LW)
        # one bracket per set; a cloud set's draws in ncol/ncol = 1 column's worth of park rows each: S launches inside it
        assert launches == 4 and ms > 0.0
        assert api.profile_read(api.TAG_SCATTER_FINISH)[1] == 5          # one reduction per set, and the addition
        assert api.profile_read(api.TAG_GAS_LW)[1] >= 1
    finally:
        api.profile_enable(False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------- #
def test_refused_inputs(bands, tables, case, lib, device):
    cols, ncol, L, S = case.cols, case.ncol, L1, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case.clouds(S))
    gaer, ka = aerosols_of(case.f)
    sizes = (4 * 4 * V1 * (ncol + 1), 4 * 2 * L * (ncol + 1), 4 * 12 * (ncol + 1), 4 * 2 * V1 * (ncol + 1), 4 * 6 * (ncol + 1))
    bufs = [_sentinel(device, n) for n in sizes]
    ptrs = [b.ptr for b in bufs]
    six_row = [None, None, ptrs[2], None, ptrs[4]]

    def refused(p, gc, gsky, form, code=api.VALUE_ERR):
        with pytest.raises(api.GrtError) as e:
            api.check(lib.grt_pipeline_run_sky_scattering(p.p, C.byref(gc), C.byref(gsky) if gsky is not None else None, *form))
        assert e.value.code == code, e.value
        p.sync()
        for b, n in zip(bufs, sizes):
            assert np.all(b.to_host((n,)) == -7.25)

    gsky, ks = api.make_sky(gclouds, gaer, S, ALL)
    refused(pipe, gcols, gsky, ptrs[:3] + [None, None])                      # both scatter outputs NULL
    refused(pipe, gcols, gsky, [None, None, ptrs[2], None, None])
    refused(pipe, gcols, gsky, [None, None, ptrs[2], ptrs[3], ptrs[4]])      # scatter_levels_dev in the six-row form
    refused(pipe, gcols, gsky, [None, None, ptrs[2], ptrs[3], None])
    refused(pipe, gcols, gsky, [None, ptrs[1], None, None, ptrs[4]])         # nothing to write (run_sky's)
    # everything run_sky refuses, in both forms
    for form in (ptrs, six_row):
        refused(pipe, gcols, None, form)
        for stray in (16, ALL | 32):
            g, k = api.make_sky(gclouds, gaer, S, stray)
            refused(pipe, gcols, g, form)
        g, k = api.make_sky(None, gaer, S, CLOUD)
        refused(pipe, gcols, g, form)
        g, k = api.make_sky(gclouds, None, S, AEROSOL)
        refused(pipe, gcols, g, form)
        for bad in (0, api.GRT_MAX_SUBCOLUMNS + 1):
            g, k = api.make_sky(gclouds, gaer, bad, ALL)
            refused(pipe, gcols, g, form)
        gcols.ncol = ncol + 1
        refused(pipe, gcols, gsky, form)
        gcols.ncol = 0
        refused(pipe, gcols, gsky, form)
        gcols.ncol = ncol
    # a pipeline without a longwave band
    sw_only = api.Pipeline(None, go_sw, ncol, -1, None, alb, solar, spectral=False)
    for form in (ptrs, six_row):
        refused(sw_only, gcols, gsky, form)
    sw_only.destroy()
    # and the same calls accepted: either scatter output alone in the profile form, no shortwave band
    _deterministic(lib, True)
    api.check(lib.grt_pipeline_run_sky_scattering(pipe.p, C.byref(gcols), C.byref(gsky), ptrs[0], None, None, None, ptrs[4]))
    pipe.sync()
    six = bufs[4].to_host((ncol + 1, 4, 6))
    assert np.all(np.isfinite(six[:ncol])) and np.all(six[ncol] == -7.25) and np.all(six[:ncol, :, [2, 5]] == 0.0)
    assert np.all(bufs[3].to_host((sizes[3],)) == -7.25) and np.all(bufs[2].to_host((sizes[2],)) == -7.25)
    api.check(lib.grt_pipeline_run_sky_scattering(pipe.p, C.byref(gcols), C.byref(gsky), ptrs[0], None, None, ptrs[3], None))
    pipe.sync()
    lv = bufs[3].to_host((ncol + 1, 4, 2, V1))
    assert np.all(np.isfinite(lv[:ncol])) and np.all(lv[ncol] == -7.25)
    assert np.array_equal(lv[:ncol, :, 0, [0, L]], six[:ncol, :, [0, 1]]) and np.array_equal(lv[:ncol, :, 1, [0, L]], six[:ncol, :, [3, 4]])
    lw_only = api.Pipeline(go_lw, None, ncol, -1, emis, None, None, spectral=False)
    api.check(lib.grt_pipeline_run_sky_scattering(lw_only.p, C.byref(gcols), C.byref(gsky), *six_row))
    lw_only.sync()
    out = bufs[2].to_host((ncol + 1, 4, 12))
    assert np.all(out[:ncol, :, 6:] == 0.0) and np.all(out[ncol] == -7.25)
    assert np.array_equal(bufs[4].to_host((ncol + 1, 4, 6))[:ncol], six[:ncol])
    lw_only.destroy()
    _deterministic(lib, False)
    for b in bufs:
        b.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
