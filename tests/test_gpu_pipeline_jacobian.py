"""grt_pipeline_run_sky_jacobian: grt_pipeline_run_sky's sets with dF_up/dT_surf of each set's longwave beside them.
Against lw_jacobian_model.py's restatement (validated against the oracle on the CPU: test_lw_jacobian_model.py), fused and
materialised, six-row and profile form; the bit-for-bit identities with grt_pipeline_run_sky and within the new rows; the
closed form of the surface row and the ordering; a central difference of the device's own fluxes; batch indexing and the
per-column surface; edge shapes of the sinks and partial sums; the production arithmetic; missing bands; what the entry
point refuses; and the older entry points before and after it on one pipeline.

Two notes on bounds.  (1) The surface row of a cloud set is the mean over S draws of one and the same double x, summed in
order and divided once: ((x + x) + x)/3 is not x for about one double in seven, so "the same double in all four sets"
holds as written for S = 1; for S = 3 the fused form is held to exactly ((x + x) + x)/3 of the clean set's double (its
mean kernel's arithmetic) and the materialised form, which takes the mean per grid point before the trapezoid, to 4 ulp.
(2) The truncation bound of the central difference, 2 d^2/6 (x_max^2 - 6 x_max + 6)/T_surf^2, is stated for a grid whose
top has x_max >= 6.  The module's longwave band ends at 400 cm-1 (x_max about 2), where that expression is negative; the
bound used is its meaning, 2 d^2/6 max_w |x^2 - 6 x + 6| / T_surf^2 over the grid's points, which is the stated expression
whenever x_max >= 6 and is conservative below (B'''/B' tends to 0 in the Rayleigh-Jeans range, Wien's form to 6/T^2)."""
import ctypes as C
import os

import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID, aerosol_fields
from grtcode_amd import api, synthetic as syn
from lw_jacobian_model import (PLANCK_C2, oracle_jacobian_sets, planck, planck_derivative, surface_closed_form, three)
from pipeline_support import (LEVEL_TOL, SETS, _deterministic, _sentinel, _setup, cached, clouds_for, make,
                              make_shape_bands, pick, subcolumn_clouds)
from pipeline_support import bands, oracle_cache, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from test_gpu_parity_production import record
from test_gpu_pipeline_sky import (ALL, AEROSOL, BOTH, CLEAN, CLOUD, NAMES, aerosols_of, fields, run_sky, same, shape_grid,
                                   sky_columns)

pytestmark = pytest.mark.gpu

V1, UL1, S_MAX = 16, 5, 3
CLOUD_SEED, AEROSOL_SEED = 81, 83         # (chosen on the CPU: a column's cloud-set TOA value is below 0.9 of its clean one)
JAC_KEYS = ("jacobian", "jacobian_levels")


def run_jac(pipe, gcols, gclouds, gaer, S, sets, ncol, profiles):
    """-> run_sky()'s dict, and with it jacobian [ncol][nsets][3] and (profile form) jacobian_levels [ncol][nsets][V]."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    pipe.run_sky_jacobian(gcols, gsky, profiles=profiles)
    n = keep["nsets"]
    if profiles:
        return dict(pipe.sky_profiles(ncol, n), **pipe.sky_jacobian_profiles(ncol, n))
    return dict(fluxes=pipe.sky_fluxes(ncol, n), jacobian=pipe.sky_jacobian_fluxes(ncol, n))


def without_jac(out):
    return {k: v for k, v in out.items() if k not in JAC_KEYS}


def grid_of(band):
    return band.w0 + np.arange(band.nw) * band.dw


def check_order(out, profiles):
    """J >= 0 and never increases upward; every value of a cloud set is at most the matching clean or aerosol one's."""
    j = out["jacobian"]
    assert np.all(j >= 0.0) and np.all(j[:, :, 0] <= j[:, :, 1]) and np.all(j[:, :, 2] <= j[:, :, 1])
    groups = [j] + ([out["jacobian_levels"]] if profiles else [])
    if profiles:
        lv = out["jacobian_levels"]
        assert np.all(lv >= 0.0) and np.all(lv[..., :-1] <= lv[..., 1:])
    if j.shape[1] == 4:
        for a in groups:
            assert np.all(a[:, 2] <= a[:, 0] * (1.0 + 1e-12)), np.max(a[:, 2] - a[:, 0])


def check_jac(out, c, k, want, user_level, profiles, tol, what):
    err = np.max(np.abs(out["jacobian"][c, k] - three(want["jacobian"], user_level)))
    print(what, "column", c, "set", k, "jacobian rows", err, "of", tol)
    assert err <= tol, (what, c, k, err, tol)
    if user_level < 0:
        assert out["jacobian"][c, k, 2] == 0.0 and not np.signbit(out["jacobian"][c, k, 2])
    if profiles:
        err = np.max(np.abs(out["jacobian_levels"][c, k] - want["jacobian"]))
        print(what, "column", c, "set", k, "jacobian levels", err, "of", tol)
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


def oracle_of(cache, orc, lib, band, tables, case, emis, S):
    cl = case.clouds(S)
    return [cached(cache, ("jacobian", c, S), lambda: oracle_jacobian_sets(
        orc, lib, band, col, tables, cl["lw_liquid"][c], cl["lw_ice"][c], cl["thickness"][c], AEROSOL_GRID, case.f[0][c],
        emis)) for c, col in enumerate(case.cols)]


# ---- 1. against the restatement ------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("profiles", [False, True])
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_jacobian_matches_the_restatement(bands, tables, oracle, oracle_cache, case1, lib, device, S, spectral, profiles):
    cols, ncol = case1.cols, case1.ncol
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    want = oracle_of(oracle_cache, oracle, lib, bands[0], tables, case1, emis, S)
    # on the oracle's numbers: under cloud less of the surface's change reaches the top -- handing back the clean Jacobian
    # does not pass
    ratio = [w[2]["jacobian"][0] / w[0]["jacobian"][0] for w in want]
    print("cloud set / clean set, dF_up/dT_surf at the top:", ratio)
    assert min(ratio) < 0.9, ratio
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, case1.clouds(S))
    gaer, keep_aer = aerosols_of(case1.f)
    got = run_jac(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
    assert got["jacobian"].shape == (ncol, 4, 3)
    check_order(got, profiles)
    for c in range(ncol):
        jj = max(np.abs(w["jacobian"]).max() for w in want[c])                    # the column's largest Jacobian value
        for k, w in enumerate(want[c]):
            check_jac(got, c, k, w, UL1, profiles, LEVEL_TOL * jj, NAMES[k])
            # (and the set's own rows are the oracle's: the restatement's inputs are the set's)
            ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
            assert np.max(np.abs(got["fluxes"][c, k, 0:3] - three(w["up_int"], UL1))) <= LEVEL_TOL * ff
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 2. identities -------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_identities_bit_for_bit(bands, tables, case1, lib, device, S, spectral):
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
            out = full[profiles] = run_jac(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
            check_order(out, profiles)
            # every output run_sky also writes is run_sky's
            assert same(without_jac(out), run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)), profiles
            if profiles:
                assert np.array_equal(out["jacobian_levels"][:, :, [0, L, UL1]], out["jacobian"])
            # the surface row does not know the atmosphere (the module's note 1 on the mean over three draws)
            sfc = out["jacobian"][:, :, 1]
            assert np.array_equal(sfc[:, 1], sfc[:, 0]) and np.array_equal(sfc[:, 3], sfc[:, 2])
            if S == 1:
                assert np.array_equal(sfc[:, 2], sfc[:, 0])
            elif not spectral:
                assert np.array_equal(sfc[:, 2], ((sfc[:, 0] + sfc[:, 0]) + sfc[:, 0]) / 3.0)
            else:
                assert np.all(np.abs(sfc[:, 2] - sfc[:, 0]) <= 4.0 * 2.0 ** -52 * sfc[:, 0])
            # the four sets differ above the surface
            assert len({out["jacobian"][0, k, 0].tobytes() for k in range(4)}) == 4
            # an aerosol of zeros: the aerosol sets' rows are the clean and the cloud sets'
            z = run_jac(pipe, gcols, gclouds, gzero, S, ALL, ncol, profiles)
            for key in JAC_KEYS[:1 + profiles]:
                assert np.array_equal(z[key][:, 1], z[key][:, 0]) and np.array_equal(z[key][:, 3], z[key][:, 2]), key
                assert np.array_equal(z[key][:, [0, 2]], out[key][:, [0, 2]]), key
            # cloud-free tables (one draw): the cloud sets' rows are the clean and the aerosol sets'
            n = run_jac(pipe, gcols, gclear, gaer, 1, ALL, ncol, profiles)
            for key in JAC_KEYS[:1 + profiles]:
                assert np.array_equal(n[key][:, 2], n[key][:, 0]) and np.array_equal(n[key][:, 3], n[key][:, 1]), key
                assert np.array_equal(n[key][:, [0, 1]], out[key][:, [0, 1]]), key
            if S == 1:
                # S = 1 is the single draw: the draw given twice runs the subcolumn instances and the mean, and (x + x)/2 is
                # x to the bit
                twice = {k: (np.repeat(v, 2, axis=1) if k in SETS else v) for k, v in cl.items()}
                two_draws = run_jac(pipe, gcols, make(tables, twice)[0], gaer, 2, ALL, ncol, profiles)
                for key in out:
                    assert np.array_equal(two_draws[key], out[key]), (key, profiles)
            # the clear-sky Jacobian on its own
            alone = run_jac(pipe, gcols, None, None, 0, CLEAN, ncol, profiles)
            assert alone["jacobian"].shape == (ncol, 1, 3)
            for key in alone:
                assert np.array_equal(alone[key][:, 0], out[key][:, 0]), key
        # rows 0, L and the user level of the profile form are the six-row form's three
        assert np.array_equal(full[True]["jacobian"], full[False]["jacobian"])
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 3. closed form and ordering ------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spectral", [False, True])
def test_closed_form_and_zero_emissivity(bands, tables, case1, lib, device, spectral):
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, case1.clouds(S))
    gaer, keep_aer = aerosols_of(case1.f)
    w = grid_of(bands[0])
    for profiles in (False, True):
        out = run_jac(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
        check_order(out, profiles)
        for c, col in enumerate(cols):
            closed = surface_closed_form(emis, col["t_surf"], w, bands[0].dw)
            err = np.max(np.abs(out["jacobian"][c, :, 1] - closed)) / closed
            print("column", c, "surface row", closed, "relative error", err)
            assert err <= 1e-12, (c, err)
    knots = np.array([0.5, 150.0, 400.5])
    gzero, keep_zero = api.make_surface(ncol, emissivity=(knots, np.zeros((ncol, 3))))
    pipe.set_surface(gzero)
    for profiles in (False, True):
        out = run_jac(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
        for key in JAC_KEYS[:1 + profiles]:
            assert np.all(out[key] == 0.0) and not np.any(np.signbit(out[key])), key
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 4. against a difference of the device's own fluxes ------------------------------------------------------------------ #
def test_central_difference_of_the_devices_fluxes(bands, tables, case1, lib, device):
    """Independent of the restatement: run_sky at T_surf +- 0.1 K on the same pipeline (fast = 0, deterministic mode)."""
    cols, ncol, S, delta = case1.cols, case1.ncol, 3, 0.1
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1, fast=0)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gclouds, keep_clouds = make(tables, case1.clouds(S))
    gaer, keep_aer = aerosols_of(case1.f)
    w = grid_of(bands[0])
    _deterministic(lib, True)
    try:
        gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
        jac = run_jac(pipe, gcols, gclouds, gaer, S, ALL, ncol, True)
        up = {}
        for sign in (1.0, -1.0):
            moved = [dict(c, t_surf=c["t_surf"] + sign * delta) for c in cols]
            g, k = api.make_columns(moved, MOL_ORDER, cfc_order=(0, 1))
            out = run_sky(pipe, g, gclouds, gaer, S, ALL, ncol, True)
            up[sign] = out["lw_up"]
            if sign > 0:
                assert np.array_equal(out["lw_down"], jac["lw_down"])          # the downward rows do not know the surface
    finally:
        _deterministic(lib, False)
    quotient = (up[1.0] - up[-1.0]) / (2.0 * delta)
    for c, col in enumerate(cols):
        x = PLANCK_C2 * w / col["t_surf"]
        q = np.abs(x * x - 6.0 * x + 6.0).max()                                # (the module's note 2)
        largest = jac["jacobian_levels"][c].max()
        bound = 2.0 * delta * delta / 6.0 * q / col["t_surf"] ** 2 * largest + 8.0 * 2.0 ** -52 * up[1.0][c].max() / delta
        err = np.abs(quotient[c] - jac["jacobian_levels"][c]).max()
        print("column", c, "central difference against J:", err, "bound", bound, "largest J", largest)
        assert err <= bound, (c, err, bound)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 5. batch indexing and the per-column surface ------------------------------------------------------------------------- #
@pytest.mark.parametrize("profiles", [False, True])
@pytest.mark.parametrize("spectral", [False, True])
def test_batch_indexing(bands, tables, case1, lib, device, spectral, profiles):
    """A batch at max_columns against its columns one at a time and in reversed order, the clouds, aerosols and surfaces
    permuted against the columns; each column's surface row is the closed form of its own emissivity knots."""
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    cl = case1.clouds(S)
    cloud_of, aer_of = [1, 2, 0], [2, 0, 1]
    knots = np.array([0.5, 150.0, 400.5])
    values = np.array([[0.95, 0.6, 0.9], [0.5, 0.99, 0.7], [0.8, 0.8, 0.3]])
    w = grid_of(bands[0])
    _deterministic(lib, True)
    try:
        def run(order):
            g, k = api.make_columns([cols[c] for c in order], MOL_ORDER, cfc_order=(0, 1))
            gc, kc = make(tables, pick(cl, columns=[cloud_of[c] for c in order]))
            ga, ka = aerosols_of(tuple(np.ascontiguousarray(f[[aer_of[c] for c in order]]) for f in case1.f))
            gs, ks = api.make_surface(len(order), emissivity=(knots, np.ascontiguousarray(values[order])))
            pipe.set_surface(gs)
            return run_jac(pipe, g, gc, ga, S, ALL, len(order), profiles)
        batch = run([0, 1, 2])
        sfc = batch["jacobian"][:, 0, 1]
        assert len({v.tobytes() for v in sfc}) == ncol
        for c, col in enumerate(cols):
            closed = surface_closed_form(np.interp(w, knots, values[c]), col["t_surf"], w, bands[0].dw)
            assert abs(sfc[c] - closed) <= 1e-12 * closed, (c, sfc[c], closed)
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


# ---- 6. edge shapes ------------------------------------------------------------------------------------------------------- #
NS = (2, 127, 128, 129, 257)
# the direct-beam module's reduced Latin square: every grid length twice, with level counts, subcolumn counts, user levels
# (mid: an interior level), batch sizes (1 and max_columns = 3) and forms rotating
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
    cols = [syn.profile(900 + V + c, V) for c in range(3)][:ncol]
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
    got = {s: run_jac(pipes[s], gcols, gclouds, gaer, S, ALL, ncol, profiles) for s in (False, True)}
    for c, col in enumerate(cols):
        want = oracle_jacobian_sets(oracle, lib, lwb, col, tables, cl["lw_liquid"][c], cl["lw_ice"][c], cl["thickness"][c],
                                    xs[0], f[0][c], emis)
        jj = max(np.abs(w["jacobian"]).max() for w in want)
        assert jj > 0.0
        for s in (False, True):
            check_order(got[s], profiles)
            for k, w in enumerate(want):
                check_jac(got[s], c, k, w, user_level, profiles, LEVEL_TOL * jj, f"spectral={s}")
    for s in (False, True):
        pipes[s].destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 7. the production arithmetic ----------------------------------------------------------------------------------------- #
def test_production_form_matches_the_restatement(bands, tables, oracle, lib, device):
    """fast = 3 on the 3 000-line bands against the restatement on the oracle's tau.  The bound is the interface's flux
    contract, 1e-3 W m-2 (test_gpu_pipeline_production.py), carried through the largest dB/dT / B of the grid at the
    column's surface temperature."""
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
    got = {p: run_jac(pipe, gcols, gclouds, gaer, S, ALL, ncol, p) for p in (False, True)}
    assert go_lw.last_launch()["fast"] == 3
    w = grid_of(bands[0])
    worst = {"worst": 0.0, "bound": 0.0}
    for c, col in enumerate(cols):
        want = oracle_jacobian_sets(oracle, lib, bands[0], col, tables, cl["lw_liquid"][c], cl["lw_ice"][c],
                                    cl["thickness"][c], AEROSOL_GRID, f[0][c], emis)
        bound = FLUX_TOL * np.max(planck_derivative(col["t_surf"], w) / planck(col["t_surf"], w))
        for p in (False, True):
            check_order(got[p], p)
            for k, wk in enumerate(want):
                err = np.abs(got[p]["jacobian"][c, k] - three(wk["jacobian"], UL1)).max()
                if p:
                    err = max(err, np.abs(got[p]["jacobian_levels"][c, k] - wk["jacobian"]).max())
                if err >= worst["worst"]:
                    worst = {"worst": float(err), "bound": float(bound)}
                print("production column", c, "set", k, "profiles", p, "error", err, "bound", bound)
    mode = "deterministic" if os.environ.get("GRT_DETERMINISTIC", "0") not in ("", "0") else "default"
    record("run_sky_jacobian." + mode, {"jacobian": worst}, file="parity_pipeline_production.json")
    assert worst["worst"] <= worst["bound"], worst
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 8. missing bands and refusals ---------------------------------------------------------------------------------------- #
def test_missing_bands(bands, tables, case1, lib, device):
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)
    _deterministic(lib, True)
    try:
        both = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
        full = {p: run_jac(both, gcols, gclouds, gaer, S, ALL, ncol, p) for p in (False, True)}
        both.destroy()
        lw_only = api.Pipeline(go_lw, None, ncol, UL1, emis, None, None, spectral=False)       # a night-only pipeline
        sw_only = api.Pipeline(None, go_sw, ncol, UL1, None, alb, solar, spectral=False)
        for profiles in (False, True):
            run_jac(sw_only, gcols, gclouds, gaer, S, ALL, ncol, profiles)           # (allocates this form's buffers)
            name = "sky_profiles" if profiles else "sky"
            for key in [name + ".jacobian"] + ([name + ".jacobian_levels"] if profiles else []):
                fill = np.full(sw_only.buffers[key].nbytes // 8, -7.25)              # zeros are written, not left
                api.check(lib.grt_host_to_device(device, sw_only.buffers[key].ptr, fill.ctypes.data_as(C.c_void_p),
                                                 C.c_size_t(fill.nbytes)))
            out = run_jac(sw_only, gcols, gclouds, gaer, S, ALL, ncol, profiles)
            for key in JAC_KEYS[:1 + profiles]:
                assert np.all(out[key] == 0.0), key
            assert same(without_jac(out), run_sky(sw_only, gcols, gclouds, gaer, S, ALL, ncol, profiles))
            assert np.array_equal(out["fluxes"][:, :, 6:], full[profiles]["fluxes"][:, :, 6:])
            out = run_jac(lw_only, gcols, gclouds, gaer, S, ALL, ncol, profiles)
            for key in JAC_KEYS[:1 + profiles]:
                assert np.array_equal(out[key], full[profiles][key]), key
            assert np.all(out["fluxes"][:, :, 6:] == 0.0)
        lw_only.destroy()
        sw_only.destroy()
    finally:
        _deterministic(lib, False)
    go_lw.destroy()
    go_sw.destroy()


def test_refused_inputs(bands, tables, case1, lib, device):
    cols, ncol, L, S = case1.cols, case1.ncol, V1 - 1, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    sizes = (4 * 4 * V1 * (ncol + 1), 4 * 2 * L * (ncol + 1), 4 * 12 * (ncol + 1), 4 * 3 * (ncol + 1), 4 * V1 * (ncol + 1))
    bufs = [_sentinel(device, n) for n in sizes]
    lv, hr, fx, j3, jl = (b.ptr for b in bufs)
    tags = (api.TAG_GAS_LW, api.TAG_GAS_SW, api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_AEROSOL_LW, api.TAG_AEROSOL_SW,
            api.TAG_ALLSKY_LW, api.TAG_ALLSKY_SW, api.TAG_SKY_LW, api.TAG_SKY_SW, api.TAG_SUBCOLUMN_MEAN,
            api.TAG_SURFACE_JACOBIAN)

    def call(gc, gsky, gjac, form):
        api.check(lib.grt_pipeline_run_sky_jacobian(pipe.p, C.byref(gc), C.byref(gsky) if gsky is not None else None,
                                                    C.byref(gjac) if gjac is not None else None, *form))

    def refused(gc, gcl, ga, S_, sets, code=api.VALUE_ERR, sky=True, forms=None):
        gsky, ks = api.make_sky(gcl, ga, S_, sets)
        forms = forms or ((api.GrtSurfaceJacobian(j3, jl), (lv, hr, fx)), (api.GrtSurfaceJacobian(j3, None), (None, None, fx)))
        for gjac, form in forms:
            with pytest.raises(api.GrtError) as e:
                call(gc, gsky if sky else None, gjac, form)
            assert e.value.code == code, (sets, e.value)
        pipe.sync()
        for b, n in zip(bufs, sizes):
            assert np.all(b.to_host((n,)) == -7.25)

    gclouds, kc = make(tables, cl)
    gaer, ka = aerosols_of(case1.f)
    api.profile_enable(True)
    try:
        api.profile_read(tags[0], reset=True)
        # the Jacobian outputs
        refused(gcols, gclouds, gaer, S, ALL, forms=((None, (lv, hr, fx)), (None, (None, None, fx))))
        refused(gcols, gclouds, gaer, S, ALL, forms=((api.GrtSurfaceJacobian(None, jl), (lv, hr, fx)),
                                                     (api.GrtSurfaceJacobian(None, None), (None, None, fx))))
        refused(gcols, gclouds, gaer, S, ALL, forms=((api.GrtSurfaceJacobian(j3, jl), (None, None, fx)),))
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
            call(gcols, gsky, api.GrtSurfaceJacobian(j3, None), (None, hr, None))
        assert e.value.code == api.VALUE_ERR
        pipe.sync()
        counts = {tag: api.profile_read(tag)[1] for tag in tags}
        assert all(n == 0 for n in counts.values()), counts
    finally:
        api.profile_enable(False)
    # and the call accepted: the outputs that may be NULL are (two calls compared to the bit: the deterministic mode)
    _deterministic(lib, True)
    try:
        call(gcols, gsky, api.GrtSurfaceJacobian(j3, None), (lv, None, None))
        pipe.sync()
        rows = bufs[3].to_host((ncol + 1, 4, 3))
        assert np.all(np.isfinite(rows[:ncol])) and np.all(rows[:ncol, :, 2] == 0.0) and np.all(rows[ncol] == -7.25)
        assert np.all(rows[:ncol, :, :2] > 0.0) and np.all(bufs[4].to_host((sizes[4],)) == -7.25)
        call(gcols, gsky, api.GrtSurfaceJacobian(j3, jl), (lv, None, None))
        pipe.sync()
        levels = bufs[4].to_host((ncol + 1, 4, V1))
        assert np.array_equal(levels[:ncol][:, :, [0, L]], rows[:ncol, :, :2]) and np.all(levels[ncol] == -7.25)
    finally:
        _deterministic(lib, False)
    for b in bufs:
        b.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 9. the existing entry points, before and after ------------------------------------------------------------------------ #
@pytest.mark.parametrize("spectral", [False, True])
def test_existing_entry_points_unchanged(bands, tables, case1, lib, device, spectral):
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)

    def older():
        out = {}
        pipe.run(gcols)
        out["run"] = pipe.fluxes(ncol)
        pipe.run_profiles(gcols)
        out.update({"run_profiles." + k: v for k, v in pipe.profiles(ncol).items()})
        for profiles in (False, True):
            out.update({f"run_sky.{profiles}.{k}": v for k, v in
                        run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles).items()})
            gsky, ks = api.make_sky(gclouds, gaer, S, ALL)
            pipe.run_sky_direct(gcols, gsky, profiles=profiles)
            out[f"run_sky_direct.{profiles}"] = pipe.sky_direct_fluxes(ncol, 4, profiles=profiles)
            if profiles:
                out.update({"run_sky_direct." + k: v for k, v in pipe.sky_direct_profiles(ncol, 4).items()})
                out.update({"run_sky_direct.sky." + k: v for k, v in pipe.sky_profiles(ncol, 4).items()})
            else:
                out["run_sky_direct.sky"] = pipe.sky_fluxes(ncol, 4)
            pipe.run_subcolumns(gcols, gclouds, S, profiles=profiles)
            if profiles:
                out.update({f"run_subcolumns.{s}.{k}": v for s, d in enumerate(pipe.subcolumn_profiles(ncol))
                            for k, v in d.items()})
            else:
                out["run_subcolumns"] = np.stack(pipe.subcolumn_fluxes(ncol))
        return out

    _deterministic(lib, True)
    try:
        before = older()
        for profiles in (False, True):
            run_jac(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles)
        after = older()
        assert before.keys() == after.keys()
        for k in before:
            assert np.array_equal(before[k], after[k]), k
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
