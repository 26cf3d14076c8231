"""grt_pipeline_run_sky: up to four sets of one driver.c column -- clear-clean, with aerosol, with clouds, with both -- from
one call and one gas-optics pass per band.  Against the oracle's column-by-column restatement (the complete set:
add_optics of {gas, Rayleigh, aerosol, liquid, ice}, the solver per subcolumn, the mean), fused and materialised, six-row
and profile form; the bit-for-bit identities with the entry points it gathers and within the new set; batch indexing
with aerosols and clouds paired differently; edge shapes; the production arithmetic; what the entry point refuses."""
import ctypes as C
import itertools

import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID, aerosol_fields, oracle_aerosol_column, oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from grtcode_amd import api, synthetic as syn
from pipeline_support import (CP, GRAVITY, LEVEL_TOL, SETS, _deterministic, _integrals, _sentinel, _setup, _solve,
                              cached, clouds_for, heating, limits, make, make_shape_bands, oracle_column,
                              oracle_subcolumns, pick, six, subcolumn_clouds)
from pipeline_support import bands, oracle_cache, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

CLEAN, AEROSOL, CLOUD, BOTH, ALL = (api.GRT_SKY_CLEAN, api.GRT_SKY_AEROSOL, api.GRT_SKY_CLOUD,
                                    api.GRT_SKY_CLOUD_AEROSOL, api.GRT_SKY_ALL)
NAMES = ("clean", "aerosol", "cloud", "both")          # the four sets in bit order
BANDS = (("lw", True), ("sw", False))
V1, UL1, S_MAX = 16, 5, 3
CLOUD_SEED, AEROSOL_SEED = 81, 83


# ---- inputs and the call ----------------------------------------------------------------------------------------------- #
def sky_columns(seed, V, n=3):
    """n synthetic columns of different surface pressure (x 1, 0.9, 1.03, 0.8) and sun."""
    out = []
    for c, (fp, mu) in enumerate(zip((1.0, 0.9, 1.03, 0.8), (0.6, 1.0, 0.3, 0.05))):
        col = syn.profile(seed + c, V)
        col["p"] = col["p"] * fp
        col["mu0"] = mu
        out.append(col)
    return out[:n]


def fields(ncol, L, seed, grids=(AEROSOL_GRID, AEROSOL_GRID)):
    return aerosol_fields(ncol, L, grids[0], seed, lw=True), aerosol_fields(ncol, L, grids[1], seed + 1, lw=False)


def aerosols_of(f, grids=(AEROSOL_GRID, AEROSOL_GRID)):
    return api.make_aerosols(lw=(grids[0], f[0]), sw=(grids[1], f[1]))


def run_sky(pipe, gcols, gclouds, gaer, S, sets, ncol, profiles):
    """-> dict with profiles()' keys, every array [ncol][nsets][..]; the six-row form has "fluxes" only."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    pipe.run_sky(gcols, gsky, profiles=profiles)
    if profiles:
        return pipe.sky_profiles(ncol, keep["nsets"])
    return dict(fluxes=pipe.sky_fluxes(ncol, keep["nsets"]))


def positions(sets):
    """Where each of the four sets lies among the packed sets of a run with these bits (the clean set always first)."""
    bits = [b for b in (CLEAN, AEROSOL, CLOUD, BOTH) if (sets | CLEAN) & b]
    return {NAMES[(CLEAN, AEROSOL, CLOUD, BOTH).index(b)]: k for k, b in enumerate(bits)}


def same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)


def one_set(out, k):
    return {key: v[:, k] for key, v in out.items()}


# ---- the oracle of the complete set ------------------------------------------------------------------------------------- #
def oracle_sky(orc, lib, band, col, lw, tables, liquid, ice, thickness, x, optics, emis=None, alb=None, solar=None):
    """One column and band with liquid / ice [S][3][B][L] and the aerosol optics [3][L][NA] on the grid x: per subcolumn
    add_optics of {gas, Rayleigh, aerosol, liquid, ice}, the solver; the fluxes summed, divided by S, every level
    integrated (oracle_subcolumns with the fifth object in slot 2).  tau, omega, g: the last subcolumn's."""
    L, S, B = col["p"].size - 1, liquid.shape[0], liquid.shape[2]
    w = driver_limits(band.w0, band.dw, band.nw)
    (llo, lhi), (ilo, ihi) = limits(tables, "liquid"), limits(tables, "ice")
    maps = (band_map(llo, lhi, B, B, w), band_map(ilo, ihi, ilo.size, B, w))
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    aer = oracle_aerosol_optics(orc, band, x, optics)
    up_sum, dn_sum = np.zeros((L + 1, band.nw)), np.zeros((L + 1, band.nw))
    for j in range(S):
        lt, lo, lg, it, io, ig = grid_optics(liquid[j], ice[j], thickness, maps)
        tau, omega, g = orc.add_optics([tau_gas, tr, aer[0], lt, it], [z, om_r, aer[1], lo, io], [z, g_r, aer[2], lg, ig])
        up, dn = _solve(orc, band, col, lw, tau, omega, g, emis, alb, solar)
        up_sum += up
        dn_sum += dn
    up_sum /= float(S)
    dn_sum /= float(S)
    up_int, dn_int = _integrals(orc, band, up_sum, dn_sum)
    return dict(up_int=up_int, dn_int=dn_int, tau=tau, omega=omega, g=g)


def oracle_sets(orc, lib, band, col, lw, tables, liquid, ice, thickness, x, optics, emis, alb, solar):
    """The four sets of one column and band, in bit order: each a dict with up_int, dn_int [V]."""
    clean = oracle_column(orc, lib, band, col, lw, emis, alb, solar)
    cu, cd = _integrals(orc, band, clean["up"], clean["dn"])
    aer = oracle_aerosol_column(orc, lib, band, col, lw, x, optics, emis, alb, solar)
    cloud = oracle_subcolumns(orc, lib, band, col, lw, tables, liquid, ice, thickness, emis, alb, solar)
    both = oracle_sky(orc, lib, band, col, lw, tables, liquid, ice, thickness, x, optics, emis, alb, solar)
    return (dict(up_int=cu, dn_int=cd), aer, cloud, both)


def check_set(got, c, k, bi, key, col, w, user_level, profiles, flux_tol, level_tol):
    """Set k of column c and band bi against the oracle's w: the six rows within flux_tol, and (profile form) every level
    within level_tol and the heating rates within the bound that follows from it: a layer's rate moves with four level
    fluxes (test_gpu_pipeline_aerosols.py's edge shapes)."""
    want = six(w["up_int"], w["dn_int"], user_level)
    err = np.max(np.abs(got["fluxes"][c, k, 6 * bi: 6 * bi + 6] - want))
    print(key, "column", c, NAMES[k] if len(NAMES) > k else k, "six rows", err)
    assert err <= flux_tol, (key, c, k, err)
    if user_level < 0:
        assert np.all(got["fluxes"][c, k, [6 * bi + 2, 6 * bi + 5]] == 0.0)
    if not profiles:
        return
    for name, a, ref in (("up", got[key + "_up"][c, k], w["up_int"]), ("down", got[key + "_down"][c, k], w["dn_int"])):
        err = np.max(np.abs(a - ref))
        print(key, "column", c, k, name, err, "of", level_tol)
        assert err <= level_tol, (key, c, k, name, err)
    mass = 100.0 * (col["p"][1:] - col["p"][:-1]) / GRAVITY
    bound = 4.0 * level_tol / (CP * mass) * 86400.0
    want_hr = heating(w["up_int"], w["dn_int"], col["p"])
    d = np.abs(got[key + "_heating"][c, k] - want_hr)
    print(key, "column", c, k, "heating", np.max(d / bound), "of its bound")
    assert np.all(d <= bound + 1e-12 * np.abs(want_hr).max()), (key, c, k)


# ---- 1. against the oracle -------------------------------------------------------------------------------------------- #
class Case1:
    """The inputs of parts 1 and 2, the same for every case, so that the module computes each oracle result once."""

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


def oracle_of(cache, orc, lib, bands, tables, case, surface, S):
    """[band][column] -> the four sets, each oracle result computed once per module."""
    emis, alb, solar = surface
    cl = case.clouds(S)
    return [[cached(cache, (key, c, S), lambda: oracle_sets(
        orc, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c], cl["thickness"][c], AEROSOL_GRID,
        case.f[bi][c], emis, alb, solar)) for c, col in enumerate(case.cols)]
        for bi, (band, (key, lw)) in enumerate(zip(bands, BANDS))]


@pytest.mark.parametrize("profiles", [False, True])
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_four_sets_match_the_oracle(bands, tables, oracle, oracle_cache, case1, lib, device, S, spectral, profiles):
    cols, ncol, L = case1.cols, case1.ncol, V1 - 1
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, case1.clouds(S))
    gaer, keep_aer = aerosols_of(case1.f)
    got = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
    assert got["fluxes"].shape == (ncol, 4, 12)
    if spectral:
        got_opt = [{k: api.device_to_host(device, pipe.views(bi)[k], (ncol, L, band.nw)) for k in ("tau", "omega", "g")}
                   for bi, band in enumerate(bands)]
    want = oracle_of(oracle_cache, oracle, lib, bands, tables, case1, (emis, alb, solar), S)
    for bi, (band, (key, lw)) in enumerate(zip(bands, BANDS)):
        from_cloud = from_aerosol = 0.0
        for c, col in enumerate(cols):
            sets = want[bi][c]
            for k, w in enumerate(sets):
                ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())      # the band's largest level flux
                check_set(got, c, k, bi, key, col, w, UL1, profiles, 1e-9, LEVEL_TOL * ff)
            both = six(sets[3]["up_int"], sets[3]["dn_int"], UL1)
            from_aerosol = max(from_aerosol, np.max(np.abs(both - six(sets[1]["up_int"], sets[1]["dn_int"], UL1))))
            from_cloud = max(from_cloud, np.max(np.abs(both - six(sets[2]["up_int"], sets[2]["dn_int"], UL1))))
            if spectral:
                # the views show the last pass: the complete set's last subcolumn
                o, w = got_opt[bi], sets[3]
                assert np.max(np.abs(o["tau"][c] - w["tau"]) / np.abs(w["tau"]).max(axis=1, keepdims=True)) < 1e-11
                assert np.max(np.abs(o["omega"][c] - w["omega"])) < 1e-11
                assert np.max(np.abs(o["g"][c] - w["g"])) < 1e-11
        # the oracle's complete set is neither its cloud set nor its aerosol set: a kernel that drops an object fails
        print(key, "complete set from the cloud set", from_cloud, "from the aerosol set", from_aerosol)
        assert from_cloud > 1e-2 and from_aerosol > 1e-2, key
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 2. bit identities ------------------------------------------------------------------------------------------------ #
def existing(pipe, gcols, gclouds, gaer, S, ncol, profiles):
    """The clean, aerosol and cloud sets from the entry points that had them: dicts as one_set gives them."""
    if profiles:
        pipe.run_profiles(gcols)
        clean = pipe.profiles(ncol)
        pipe.run_aerosols(gcols, gaer, profiles=True)
        aer = pipe.aerosol_profiles(ncol)[1]
        pipe.run_subcolumns(gcols, gclouds, S, profiles=True)
        cloud = pipe.subcolumn_profiles(ncol)[1]
        return clean, aer, cloud
    pipe.run(gcols)
    clean = dict(fluxes=pipe.fluxes(ncol))
    pipe.run_aerosols(gcols, gaer)
    aer = dict(fluxes=pipe.aerosol_fluxes(ncol)[1])
    pipe.run_subcolumns(gcols, gclouds, S)
    cloud = dict(fluxes=pipe.subcolumn_fluxes(ncol)[1])
    return clean, aer, cloud


@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_sets_are_the_existing_entry_points_and_subsets_agree(bands, tables, case1, lib, device, monkeypatch, S, spectral):
    cols, ncol, L = case1.cols, case1.ncol, V1 - 1
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    gclouds, keep_clouds = make(tables, cl)
    gaer, keep_aer = aerosols_of(case1.f)
    gzero, keep_zero = aerosols_of(tuple(np.zeros_like(f) for f in case1.f))
    # cloud-free tables: clouds_for(..., clear=True)'s one draw, S times
    clear = clouds_for(cols, tables, CLOUD_SEED, clear=True)
    gclear, keep_clear = make(tables, {k: (np.repeat(v[:, None], S, axis=1) if k in SETS else v) for k, v in clear.items()})
    _deterministic(lib, True)
    try:
        full = {}
        for profiles in (False, True):
            out = full[profiles] = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
            clean, aer, cloud = existing(pipe, gcols, gclouds, gaer, S, ncol, profiles)
            assert same(one_set(out, 0), clean), profiles
            assert same(one_set(out, 1), aer), profiles
            assert same(one_set(out, 2), cloud), profiles
            if S == 1:
                g0, k0 = make(tables, {k: (v[:, 0] if k in SETS else v) for k, v in cl.items()})
                if profiles:
                    pipe.run_allsky_profiles(gcols, g0)
                    assert same(one_set(out, 2), pipe.allsky_profiles(ncol)[1])
                else:
                    pipe.run_allsky(gcols, g0)
                    assert np.array_equal(out["fluxes"][:, 2], pipe.allsky_fluxes(ncol)[1])
            # the four sets differ, in both bands
            for a, b in itertools.combinations(range(4), 2):
                assert not np.array_equal(out["fluxes"][:, a, :6], out["fluxes"][:, b, :6]), (a, b)
                assert not np.array_equal(out["fluxes"][:, a, 6:], out["fluxes"][:, b, 6:]), (a, b)
            # an aerosol of zeros: the complete set is the cloud set; cloud-free tables: it is the aerosol set
            z = run_sky(pipe, gcols, gclouds, gzero, S, ALL, ncol, profiles)
            assert same(one_set(z, 3), one_set(z, 2)) and same(one_set(z, 2), one_set(out, 2)), profiles
            assert same(one_set(z, 1), one_set(z, 0))
            n = run_sky(pipe, gcols, gclear, gaer, S, ALL, ncol, profiles)
            assert same(one_set(n, 1), one_set(out, 1)) and same(one_set(n, 0), one_set(out, 0)), profiles
            if S == 1:
                assert same(one_set(n, 3), one_set(n, 1)) and same(one_set(n, 2), one_set(n, 0)), profiles
            else:
                # (x + x + x)/3 is not x to the bit: the mean of S equal draws within test_averaging_identities' bound
                # for such a mean, 1e-15 of the largest flux (test_gpu_pipeline_subcolumns.py); a heating rate moves
                # with four level fluxes
                tol = 1e-15 * np.abs(n["fluxes"]).max()
                dp = np.array([col["p"][1:] - col["p"][:-1] for col in cols])
                hr_tol = 4.0 * tol * GRAVITY / (CP * 100.0 * dp) * 86400.0
                for a, b in ((3, 1), (2, 0)):
                    for k in n:
                        d = np.abs(n[k][:, a] - n[k][:, b])
                        assert np.all(d <= (hr_tol if k.endswith("heating") else tol)), (a, b, k, profiles)
            # any subset of the four: each of its sets has the bits it has in the four-set run
            for mask in range(16):
                sub = run_sky(pipe, gcols, gclouds if mask & (CLOUD | BOTH) else None,
                              gaer if mask & (AEROSOL | BOTH) else None, S, mask, ncol, profiles)
                where = positions(mask)
                assert sub["fluxes"].shape[1] == len(where) == api.sky_set_count(mask)
                for name, k in where.items():
                    assert same(one_set(sub, k), one_set(out, NAMES.index(name))), (mask, name, profiles)
            # a column alone has the bits it has in its batch
            c = 1
            g1, k1 = api.make_columns(cols[c:c + 1], MOL_ORDER, cfc_order=(0, 1))
            c1, kc1 = make(tables, pick(cl, columns=[c]))
            a1, ka1 = aerosols_of(tuple(f[c:c + 1] for f in case1.f))
            alone = run_sky(pipe, g1, c1, a1, S, ALL, 1, profiles)
            assert all(np.array_equal(alone[k][0], out[k][c]) for k in out), profiles
        # rows 0, L and the user level of the profile form are the six-row form's with two shortwave sweeps
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        two = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, False)["fluxes"]
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        prof = full[True]
        assert np.array_equal(prof["fluxes"], two)
        for bi, key in enumerate(("lw", "sw")):
            assert np.array_equal(prof[key + "_up"][:, :, [0, L, UL1]], two[:, :, 6 * bi: 6 * bi + 3]), key
            assert np.array_equal(prof[key + "_down"][:, :, [0, L, UL1]], two[:, :, 6 * bi + 3: 6 * bi + 6]), key
        assert np.array_equal(two[:, :, :6], full[False]["fluxes"][:, :, :6])     # (the longwave has one form)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_the_complete_set_has_profile_tags_of_its_own(bands, tables, case1, lib, device):
    cols, ncol = case1.cols, case1.ncol
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, case1.clouds(3))
    gaer, keep_aer = aerosols_of(case1.f)
    gas = (api.TAG_GAS_LW, api.TAG_GAS_SW)
    solvers = (api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_AEROSOL_LW, api.TAG_AEROSOL_SW, api.TAG_ALLSKY_LW,
               api.TAG_ALLSKY_SW, api.TAG_SKY_LW, api.TAG_SKY_SW)
    api.profile_enable(True)
    try:
        api.profile_read(gas[0], reset=True)                   # (a reset clears the brackets of every tag)
        pipe.run(gcols)
        pipe.sync()
        one_pass = {tag: api.profile_read(tag)[1] for tag in gas + solvers}
        api.profile_read(gas[0], reset=True)
        run_sky(pipe, gcols, gclouds, gaer, 3, ALL, ncol, False)
        counts = {tag: api.profile_read(tag) for tag in gas + solvers}
    finally:
        api.profile_enable(False)
    # the gas optics of one grt_pipeline_run per band, and one solve per set and band, each under its pass's tags
    assert all(counts[tag][1] == one_pass[tag] >= 1 for tag in gas), (counts, one_pass)
    assert all(counts[tag][1] == 1 and counts[tag][0] > 0.0 for tag in solvers), counts
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- batch indexing ---------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("profiles", [False, True])
@pytest.mark.parametrize("spectral", [False, True])
def test_aerosols_stay_with_their_column_in_every_subcolumn(bands, tables, case1, lib, device, spectral, profiles):
    """Three columns with different aerosols, S = 3.  Two columns swap their aerosols and keep their clouds: the outputs
    change for exactly those two, and each equals a single-column run of the same pairing.  A kernel that reads the
    aerosol table at the subcolumn's table index s*ncol + c instead of the column c does not pass."""
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    gclouds, keep_clouds = make(tables, cl)
    order = [2, 1, 0]
    swapped = tuple(np.ascontiguousarray(f[order]) for f in case1.f)
    _deterministic(lib, True)
    try:
        gaer, keep_aer = aerosols_of(case1.f)
        base = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
        gswap, keep_swap = aerosols_of(swapped)
        moved = run_sky(pipe, gcols, gclouds, gswap, S, ALL, ncol, profiles)
        for k in base:
            assert np.array_equal(moved[k][1], base[k][1]), k                  # the column that kept its aerosol
            assert np.array_equal(moved[k][:, [0, 2]], base[k][:, [0, 2]]), k  # the sets without aerosol
        for c in (0, 2):
            for k in (1, 3):
                assert not np.array_equal(moved["fluxes"][c, k, :6], base["fluxes"][c, k, :6]), (c, k)
                assert not np.array_equal(moved["fluxes"][c, k, 6:], base["fluxes"][c, k, 6:]), (c, k)
            g1, k1 = api.make_columns(cols[c:c + 1], MOL_ORDER, cfc_order=(0, 1))
            c1, kc1 = make(tables, pick(cl, columns=[c]))
            a1, ka1 = aerosols_of(tuple(f[c:c + 1] for f in swapped))
            alone = run_sky(pipe, g1, c1, a1, S, ALL, 1, profiles)
            assert all(np.array_equal(alone[k][0], moved[k][c]) for k in moved), c
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 3. edge shapes --------------------------------------------------------------------------------------------------- #
NS = (2, 127, 128, 129, 257)
# a reduced Latin square: every grid length, with level counts, subcolumn counts, aerosol grid kinds (2 points / more
# points than the grid has), user levels and forms rotating against each other
SHAPES = [(2, 61, 3, "more", "L", True), (127, 2, 1, "two", "0", False), (128, 201, 1, "more", "-1", False),
          (129, 3, 3, "two", "L", True), (257, 61, 1, "two", "0", True), (127, 3, 3, "more", "-1", True),
          (129, 201, 3, "more", "0", False), (2, 2, 1, "two", "-1", False)]
shape_bands = make_shape_bands(NS, 100.0, 2000.0)


def shape_grid(band, kind):
    """test_gpu_pipeline_aerosols.py's two kinds of aerosol grid on a band"""
    span = band.wn - band.w0
    if kind == "two":
        if band.nw == 2:
            return np.array([band.w0 - 0.5 * band.dw, band.wn + 0.5 * band.dw])
        return np.array([band.w0 + 0.3 * span, band.w0 + 0.8 * span])           # points below, inside and above
    return np.linspace(band.w0 - 2.5 * band.dw, band.wn + 2.5 * band.dw, band.nw + 3)


@pytest.mark.parametrize("n,V,S,na_kind,ul,profiles", SHAPES,
                         ids=[f"n{n}-V{V}-S{S}-{k}-ul{u}-{'prof' if p else 'six'}" for n, V, S, k, u, p in SHAPES])
def test_edge_shapes(shape_bands, tables, oracle, lib, device, n, V, S, na_kind, ul, profiles):
    L = V - 1
    user_level = {"-1": -1, "0": 0, "L": L}[ul]
    lwb, swb = shape_bands[n]
    cols = [syn.profile(900 + V + c, V) for c in range(3)]
    for c, mu in zip(cols, (1.0, 0.05, 1e-3)):                      # overhead sun, low sun, the sun on the horizon
        c["mu0"] = mu
    ncol = len(cols)
    go_lw, _ = lwb.gas_optics(device, V)
    go_sw, grid_sw = swb.gas_optics(device, V)
    rng = np.random.default_rng(n + V)
    emis, alb = rng.uniform(0.3, 1.0, n), rng.uniform(0.0, 0.7, n)
    solar = api.create_solar_flux(grid_sw, swb.files["solar"])
    xs = (shape_grid(lwb, na_kind), shape_grid(swb, na_kind))
    f = (aerosol_fields(ncol, L, xs[0], 60 + n, lw=True), aerosol_fields(ncol, L, xs[1], 61 + n, lw=False))
    gaer, keep_aer = aerosols_of(f, xs)
    draws = [clouds_for(cols, tables, 90 + n + V + j) for j in range(S)]
    cl = {k: (np.stack([d[k] for d in draws], axis=1) if k in SETS else draws[0][k]) for k in draws[0]}
    gclouds, keep_clouds = make(tables, cl)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    pipes = {s: api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=s) for s in (False, True)}
    got = {s: run_sky(pipes[s], gcols, gclouds, gaer, S, ALL, ncol, profiles) for s in (False, True)}
    for bi, (band, (key, lw)) in enumerate(zip((lwb, swb), BANDS)):
        for c, col in enumerate(cols):
            sets = oracle_sets(oracle, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
                               cl["thickness"][c], xs[bi], f[bi][c], emis, alb, solar)
            for s in (False, True):
                for k, w in enumerate(sets):
                    ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
                    assert ff > 0.0
                    check_set(got[s], c, k, bi, key, col, w, user_level, profiles, LEVEL_TOL * ff, LEVEL_TOL * ff)
    for s in (False, True):
        pipes[s].destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 4. the production form ------------------------------------------------------------------------------------------- #
def test_production_form_matches_the_oracle(bands, tables, oracle, lib, device):
    """fast = 3, four columns, all four sets in the profile form: the project's contract -- fluxes and level fluxes within
    1e-3 W m-2 of the oracle, heating rates within the bound that follows from it.  Worst values met on
    an MI355X: see the DESIGN section 5 table."""
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
    got = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, True)
    six_rows = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, False)
    assert go_lw.last_launch()["fast"] == 3 and go_sw.last_launch()["fast"] == 3
    worst = {"flux": 0.0, "level": 0.0, "heating_of_bound": 0.0}
    for bi, (band, (key, lw)) in enumerate(zip(bands, BANDS)):
        for c, col in enumerate(cols):
            sets = oracle_sets(oracle, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
                               cl["thickness"][c], AEROSOL_GRID, f[bi][c], emis, alb, solar)
            mass = 100.0 * (col["p"][1:] - col["p"][:-1]) / GRAVITY
            bound = 4.0 * FLUX_TOL / (CP * mass) * 86400.0
            for k, w in enumerate(sets):
                want = six(w["up_int"], w["dn_int"], UL1)
                for out in (got, six_rows):
                    worst["flux"] = max(worst["flux"], np.max(np.abs(out["fluxes"][c, k, 6 * bi: 6 * bi + 6] - want)))
                worst["level"] = max(worst["level"], np.max(np.abs(got[key + "_up"][c, k] - w["up_int"])),
                                     np.max(np.abs(got[key + "_down"][c, k] - w["dn_int"])))
                d = np.abs(got[key + "_heating"][c, k] - heating(w["up_int"], w["dn_int"], col["p"]))
                worst["heating_of_bound"] = max(worst["heating_of_bound"], np.max(d / bound))
    print("production form, worst:", worst)
    assert worst["flux"] <= FLUX_TOL and worst["level"] <= FLUX_TOL and worst["heating_of_bound"] <= 1.0, worst
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 5. refusals ------------------------------------------------------------------------------------------------------ #
def test_refused_inputs(bands, tables, case1, lib, device):
    cols, ncol, L, S = case1.cols, case1.ncol, V1 - 1, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    sizes = (4 * 4 * V1 * (ncol + 1), 4 * 2 * L * (ncol + 1), 4 * 12 * (ncol + 1))
    bufs = [_sentinel(device, n) for n in sizes]

    def refused(gc, gcl, ga, S_, sets, code=api.VALUE_ERR, sky=True):
        gsky, ks = api.make_sky(gcl, ga, S_, sets)
        for form in ([b.ptr for b in bufs], [None, None, bufs[2].ptr]):
            with pytest.raises(api.GrtError) as e:
                api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gc), C.byref(gsky) if sky else None, *form))
            assert e.value.code == code, (sets, e.value)
        pipe.sync()
        for b, n in zip(bufs, sizes):
            assert np.all(b.to_host((n,)) == -7.25)

    gclouds, kc = make(tables, cl)
    gaer, ka = aerosols_of(case1.f)
    refused(gcols, gclouds, gaer, S, ALL, sky=False)
    for stray in (16, ALL | 32, 1 << 31):                                        # unknown set bits
        refused(gcols, gclouds, gaer, S, stray)
    for sets in (CLOUD, BOTH, ALL):                                             # a cloud set without clouds
        refused(gcols, None, gaer, S, sets)
    for sets in (AEROSOL, BOTH, ALL):                                           # an aerosol set without aerosols
        refused(gcols, gclouds, None, S, sets)
    for bad in (0, -1, api.GRT_MAX_SUBCOLUMNS + 1):                             # subcolumns out of range
        refused(gcols, gclouds, gaer, bad, ALL)
        refused(gcols, gclouds, None, bad, CLOUD)
    for field in SETS + ("thickness", "liquid_band_lo"):                        # check_clouds
        g, k = make(tables, cl)
        setattr(g, field, None)
        refused(gcols, g, gaer, S, ALL)
    g, k = make(tables, cl)
    g.num_liquid_bands = 0
    refused(gcols, g, gaer, S, CLOUD | AEROSOL)
    for field, value in (("lw_num_points", 1), ("sw_num_points", -1), ("lw_grid", None), ("sw_optics", None)):
        g, k = aerosols_of(case1.f)                                             # check_aerosol_band
        setattr(g, field, value)
        refused(gcols, gclouds, g, S, ALL)
        refused(gcols, None, g, S, AEROSOL)
    bad_grid = np.array([150.0, 900.0, 300.0, 1200.0])
    g, k = api.make_aerosols(lw=(bad_grid, np.ascontiguousarray(case1.f[0][..., :4])), sw=(AEROSOL_GRID, case1.f[1]))
    refused(gcols, gclouds, g, S, BOTH)
    big_cols = sky_columns(300, V1, n=4)                                        # check_columns
    big, keep_big = api.make_columns(big_cols, MOL_ORDER, cfc_order=(0, 1))
    gb, kb = make(tables, subcolumn_clouds(big_cols, tables, CLOUD_SEED, S))
    ab, kab = aerosols_of(fields(4, L, AEROSOL_SEED))
    refused(big, gb, ab, S, ALL)
    gcols.ncol = 0
    refused(gcols, gclouds, gaer, S, ALL)
    gcols.ncol = ncol
    night = [dict(c) for c in cols]                                             # a night column
    night[1]["mu0"] = 0.0
    gnight, keep_night = api.make_columns(night, MOL_ORDER, cfc_order=(0, 1))
    refused(gnight, gclouds, gaer, S, ALL, code=api.RANGE_ERR)
    gsky, ks = api.make_sky(gclouds, gaer, S, ALL)
    with pytest.raises(api.GrtError) as e:                                      # nothing to write
        api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(gsky), None, bufs[1].ptr, None))
    assert e.value.code == api.VALUE_ERR
    # and the same call accepted: inputs no requested set needs are not looked at, outputs that may be NULL are
    g, k = make(tables, cl)
    g.lw_liquid = None
    gsky2, ks2 = api.make_sky(g, gaer, 0, AEROSOL)
    api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(gsky2), None, None, bufs[2].ptr))
    api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(gsky), bufs[0].ptr, None, None))
    pipe.sync()
    six2 = bufs[2].to_host((sizes[2],))
    assert np.all(np.isfinite(six2[:ncol * 24])) and np.all(six2[:ncol * 24] != -7.25) and np.all(six2[ncol * 24:] == -7.25)
    lv = bufs[0].to_host((ncol + 1, 4, 4, V1))
    assert np.all(np.isfinite(lv[:ncol])) and np.all(lv[ncol] == -7.25) and np.all(bufs[1].to_host((sizes[1],)) == -7.25)
    for b in bufs:
        b.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_missing_bands_and_bands_without_aerosol(bands, tables, case1, lib, device):
    """A band the pipeline lacks gives zeros in every set; a band that was given no aerosol runs its aerosol sets without
    the object: the aerosol set is the clean set there and the complete set the cloud set, bit for bit."""
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case1.clouds(S))
    for which in (0, 1):
        pipe = api.Pipeline(go_lw if which == 0 else None, go_sw if which == 1 else None, ncol, UL1,
                            emis if which == 0 else None, alb if which == 1 else None, solar if which == 1 else None,
                            spectral=False)
        gaer, ka = aerosols_of(case1.f)
        missing, present = slice(6 * (1 - which), 6 * (1 - which) + 6), slice(6 * which, 6 * which + 6)
        for profiles in (False, True):
            out = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
            assert np.all(out["fluxes"][:, :, missing] == 0.0)
            assert len({out["fluxes"][0, k, present].tobytes() for k in range(4)}) == 4
            if profiles:
                pre = ("sw", "lw")[which]
                assert all(np.all(out[pre + k] == 0.0) for k in ("_up", "_down", "_heating"))
        pipe.destroy()
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    for none in (0, 1):
        gaer, ka = api.make_aerosols(lw=None if none == 0 else (AEROSOL_GRID, case1.f[0]),
                                     sw=None if none == 1 else (AEROSOL_GRID, case1.f[1]))
        rows = slice(6 * none, 6 * none + 6)
        for profiles in (False, True):
            out = run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
            assert np.array_equal(out["fluxes"][:, 1, rows], out["fluxes"][:, 0, rows])
            assert np.array_equal(out["fluxes"][:, 3, rows], out["fluxes"][:, 2, rows])
            assert not np.array_equal(out["fluxes"][:, 2, rows], out["fluxes"][:, 0, rows])
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
