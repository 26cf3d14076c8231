"""The batched pipeline in the PRODUCTION arithmetic (fast = 3: fp32 line preparation in the lean loop, far wings by cell
moments in two passes, the cell hierarchy on fine grids) -- the form a new gas-optics object runs, bench.py times and an
unchanged driver gets -- through every entry point against the oracle, in the identities that do not depend on the form,
and at the shapes where the launch planning of grt_gas_launch.c (tile and slice choice, lean and narrow eligibility, the
hierarchy switch, per-column moment scratch and column groups, the work list, continua handed to the solvers) goes wrong.
Every other pipeline module runs the reference's operation order (Band.gas_optics' default, fast = 0).

All bounds are the project's own, none comes from a measurement made here:
  tau_gas          2e-6 of each layer's largest optical depth   (FAST_TOL of test_gpu_moment_kernel.py, BOUNDS[3])
  integrated flux  1e-3 W m-2                                    (FLUX_TOL, BASELINE.json north star)
  spectra          1e-5 of the band's largest flux               (BOUNDS[3]["spectral_flux_rel"])
  bins             1e-3 W m-2 each
  heating rates    4 FLUX_TOL g/(c_p 100 dp) 86400 K day-1: a layer's rate moves with four level fluxes, each within FLUX_TOL
  heating formula  1e-12 of the largest rate, on the kernel's own levels (check_levels' first assertion)
The worst value met per entry point and quantity goes to parity_pipeline_production.json, next to the record
test_gpu_parity_production.py keeps of its own worst cases."""
import os

import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID, aerosol_fields, oracle_aerosol_column
from grtcode_amd import api, synthetic as syn
from pipeline_support import (CP, ENTRIES, GRAVITY, KEYS, SETS, SOLVER_NS, _setup, block_edges, cached,
                              cloud_columns, clouds_for, columns, heating, make, oracle_allsky_levels, oracle_column,
                              oracle_subcolumns, pick, run_entry, six, spectral_rows, subcolumn_clouds, surface, user_index)
from pipeline_support import bands, oracle_cache, solver_bands, tables  # noqa: F401  (module fixtures)
from scenario import Band, MOL_ORDER
from test_gpu_parity_production import record

pytestmark = pytest.mark.gpu

FAST = 3
TAU_TOL = 2e-6        # of each layer's largest optical depth
FLUX_TOL = 1e-3       # W m-2
SPECTRAL_REL = 1e-5   # of the band's largest flux
BIN_TOL = 1e-3        # W m-2
FORMULA_TOL = 1e-12   # of the largest heating rate
BANDS = (("lw", True), ("sw", False))

V1, UL1 = 16, 5       # part 1: levels, user level
CLOUD_SEED, SUB_SEED, SUB_S, AEROSOL_SEED = 71, 72, 3, 73


# ---- the record -------------------------------------------------------------------------------------------------------- #
WORST = {}


def note(lib, entry, quantity, value, bound):
    """Keep the largest `value` met for (entry, quantity) next to the bound it is held to, and write the record: one
    section per mode the suite was started in (plain, or GRT_DETERMINISTIC=1 in the environment)."""
    e = WORST.setdefault(entry, {})
    q = e.setdefault(quantity, {"worst": 0.0, "bound": bound})
    q["worst"] = max(q["worst"], float(value))
    mode = "deterministic" if os.environ.get("GRT_DETERMINISTIC", "0") not in ("", "0") else "default"
    record(mode, WORST, file="parity_pipeline_production.json")
    return value


# ---- inputs ------------------------------------------------------------------------------------------------------------ #
def varied_columns(seed, V, n=4, pressure=1.0, factors=(1.0, 0.9, 1.03, 0.8)):
    """n synthetic columns whose surface pressures (x 1, 0.9, 1.03, 0.8), temperatures (+0, -6, +4, -11 K) and suns
    differ: a batch in which no per-column quantity of the launch may be taken from another column."""
    out = []
    for c, (fp, dt, mu) in enumerate(zip(factors, (0.0, -6.0, 4.0, -11.0), (0.6, 1.0, 0.3, 0.05))):
        col = syn.profile(seed + c, V)
        col["p"] = col["p"] * (fp * pressure)
        col["t"] = col["t"] + dt
        col["t_layer"] = col["t_layer"] + dt
        col["t_surf"] = col["t_surf"] + dt
        col["mu0"] = mu
        out.append(col)
    return out[:n]


def assert_production(*gas):
    """No silent fall-back to another form: the comparison would be vacuous."""
    for go in gas:
        info = go.last_launch()
        assert info["fast"] == FAST, info


def shape_of(go):
    info = go.last_launch()
    return tuple(info[k] for k in ("fast", "tile", "nslice", "tree_levels", "halo", "moments"))


def with_integrals(orc, band, w):
    """An oracle result with its level spectra up, dn [V][nw]: their integrals up_int, dn_int [V] added."""
    if "up_int" not in w:
        w["up_int"] = np.array([orc.integrate_row(r, band.dw) for r in w["up"]])
        w["dn_int"] = np.array([orc.integrate_row(r, band.dw) for r in w["dn"]])
    return w


class Part1:
    """Part 1's inputs and its oracle results, each computed once per module (oracle_cache)."""

    def __init__(self, bands, tables, cache, orc, lib, device):
        self.bands, self.tables, self.cache, self.orc, self.lib, self.device = bands, tables, cache, orc, lib, device
        self.cols = varied_columns(800, V1)
        self.ncol = len(self.cols)
        self.cl = cloud_columns(self.cols, tables, CLOUD_SEED)
        self.lw_f = aerosol_fields(self.ncol, V1 - 1, AEROSOL_GRID, AEROSOL_SEED, lw=True)
        self.sw_f = aerosol_fields(self.ncol, V1 - 1, AEROSOL_GRID, AEROSOL_SEED + 1, lw=False)
        lwb, swb = bands
        grid_sw = api.create_spectral_grid(swb.w0, swb.wn, swb.dw)
        self.surface = (np.full(lwb.nw, 0.98), np.full(swb.nw, 0.2), api.create_solar_flux(grid_sw, swb.files["solar"]))

    def open(self, spectral, user_level=UL1, fast=FAST, tile=0):
        self.go_lw, self.go_sw, self.emis, self.alb, self.solar = _setup(self.bands, self.device, V1, fast=fast)
        if tile:
            for go in (self.go_lw, self.go_sw):
                go.tune(tile=tile, nslice=1, fast=fast)
        self.pipe = api.Pipeline(self.go_lw, self.go_sw, self.ncol, user_level, self.emis, self.alb, self.solar,
                                 spectral=spectral)
        self.gcols, self.keep = api.make_columns(self.cols, MOL_ORDER, cfc_order=(0, 1))
        return self.pipe

    def close(self):
        self.pipe.destroy()
        self.go_lw.destroy()
        self.go_sw.destroy()

    def surface_of(self):
        """Emissivity, albedo and sun: _setup's."""
        return self.surface

    def clear(self, bi, c):
        band, (key, lw) = self.bands[bi], BANDS[bi]
        emis, alb, solar = self.surface_of()
        return cached(self.cache, ("clear", key, c), lambda: with_integrals(self.orc, band, oracle_column(
            self.orc, self.lib, band, self.cols[c], lw, emis, alb, solar)))

    def allsky(self, bi, c):
        band, (key, lw) = self.bands[bi], BANDS[bi]
        emis, alb, solar = self.surface_of()
        cl = self.cl
        return cached(self.cache, ("allsky", key, c), lambda: oracle_allsky_levels(
            self.orc, self.lib, band, self.cols[c], lw, self.tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
            cl["thickness"][c], emis, alb, solar))

    def subcolumns(self, bi, c, cl):
        band, (key, lw) = self.bands[bi], BANDS[bi]
        emis, alb, solar = self.surface_of()
        return cached(self.cache, ("subcolumns", key, c), lambda: oracle_subcolumns(
            self.orc, self.lib, band, self.cols[c], lw, self.tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
            cl["thickness"][c], emis, alb, solar))

    def aerosol(self, bi, c):
        band, (key, lw) = self.bands[bi], BANDS[bi]
        emis, alb, solar = self.surface_of()
        f = (self.lw_f, self.sw_f)[bi]
        return cached(self.cache, ("aerosol", key, c), lambda: oracle_aerosol_column(
            self.orc, self.lib, band, self.cols[c], lw, AEROSOL_GRID, f[c], emis, alb, solar))


@pytest.fixture
def p1(bands, tables, oracle_cache, oracle, lib, device):
    return Part1(bands, tables, oracle_cache, oracle, lib, device)


# ---- checks ------------------------------------------------------------------------------------------------------------ #
def check_tau_gas(lib, entry, device, pipe, bands, ncol, L, want_of):
    """The tau_gas view of both bands, every column: want_of(bi, c) -> the oracle's gas optical depths [L][nw]."""
    for bi, band in enumerate(bands):
        got = api.device_to_host(device, pipe.views(bi)["tau_gas"], (ncol, L, band.nw))
        for c in range(ncol):
            want = want_of(bi, c)
            layer_max = np.abs(want).max(axis=1, keepdims=True)
            assert np.all(layer_max > 0.0)
            rel = np.abs(got[c] - want) / layer_max
            err = note(lib, entry, "tau_gas_of_layer_max", rel.max(), TAU_TOL)
            i, k = np.unravel_index(rel.argmax(), rel.shape)
            assert err <= TAU_TOL, f"{entry} {BANDS[bi][0]} column {c}: tau_gas {err} of the layer maximum, layer {i}, point {k}"


def check_six(lib, entry, what, got6, w, user_level):
    want = six(w["up_int"], w["dn_int"], user_level)
    err = note(lib, entry, "flux_w_m2", np.max(np.abs(got6 - want)), FLUX_TOL)
    assert err <= FLUX_TOL, f"{entry} {what}: six rows {err} W m-2 from the oracle (row {np.argmax(np.abs(got6 - want))})"
    if user_level < 0:
        assert got6[2] == 0.0 and got6[5] == 0.0, (entry, what)


def check_profile(lib, entry, what, prof, c, key, col, w):
    """One column, band and set of a profile form: every level, the heating rates against the bound derived from the flux
    contract, and the heating formula on the kernel's own levels."""
    up, dn, hr = prof[key + "_up"][c], prof[key + "_down"][c], prof[key + "_heating"][c]
    for name, a, want in (("up", up, w["up_int"]), ("down", dn, w["dn_int"])):
        err = note(lib, entry, "level_flux_w_m2", np.max(np.abs(a - want)), FLUX_TOL)
        assert err <= FLUX_TOL, f"{entry} {what} {name}: {err} W m-2 from the oracle at level {np.argmax(np.abs(a - want))}"
    p = col["p"]
    bound = 4.0 * FLUX_TOL * GRAVITY / (CP * 100.0 * (p[1:] - p[:-1])) * 86400.0
    d = np.abs(hr - heating(w["up_int"], w["dn_int"], p))
    note(lib, entry, "heating_of_its_bound", np.max(d / bound), 1.0)
    note(lib, entry, "heating_k_per_day", d.max(), float(bound.min()))
    j = int(np.argmax(d / bound))
    assert np.all(d <= bound), f"{entry} {what}: heating {d[j]} K day-1 from the oracle in layer {j}, bound {bound[j]}"
    hmax = np.abs(hr).max()
    assert hmax > 0.0, (entry, what)
    err = np.max(np.abs(hr - heating(up, dn, p)))
    assert err <= FORMULA_TOL * hmax, f"{entry} {what}: heating {err} from the formula on its own levels, largest {hmax}"


def check_level_spectra(lib, entry, what, device, pipe, bi, band, ncol, V, c, w):
    """The materialised form's level spectra of band bi, column c against the oracle's."""
    v = pipe.views(bi)
    scale = max(np.abs(w["up"]).max(), np.abs(w["dn"]).max())
    assert scale > 0.0
    for name, view, want in (("up", "flux_up", w["up"]), ("down", "flux_down", w["dn"])):
        got = api.device_to_host(device, v[view], (ncol, V, band.nw))[c]
        d = np.abs(got - want)
        err = note(lib, entry, "level_spectra_rel", d.max() / scale, SPECTRAL_REL)
        k, i = np.unravel_index(d.argmax(), d.shape)
        assert err <= SPECTRAL_REL, f"{entry} {what} {name}: {err} of the band's largest flux at level {k}, point {i}"


def bits(r):
    """Everything run_entry returned, as one list of arrays."""
    out = [r["six"]] + ([r["clear"]] if r["clear"] is not None else [])
    for p in (r["prof"], r["clear_prof"]):
        if p is not None:
            out += [p[k] for k in KEYS]
    return out


def same_bits(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- 0. the default ------------------------------------------------------------------------------------------------------ #
def test_an_untuned_object_runs_the_production_form(bands, lib, device, monkeypatch):
    """No tune() call, no GRT_GAS_OPTICS_FAST in the environment: the pipeline's launches are fast = 3."""
    monkeypatch.delenv("GRT_GAS_OPTICS_FAST", raising=False)
    cols = varied_columns(790, V1, 2)
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1, fast=None)
    pipe = api.Pipeline(go_lw, go_sw, 2, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    pipe.run(gcols)
    got = pipe.fluxes(2)
    assert go_lw.last_launch()["fast"] == 3 and go_sw.last_launch()["fast"] == 3
    assert np.all(got[:, [0, 6]] > 0.0)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 1. every entry point against the oracle ----------------------------------------------------------------------------- #
@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_base_entry_points_match_the_oracle(p1, tables, lib, device, entry, spectral):
    allsky, profile = "allsky" in entry, "profiles" in entry
    pipe = p1.open(spectral)
    gclouds, keep_clouds = make(tables, p1.cl) if allsky else (None, None)
    got = run_entry(pipe, entry, p1.gcols, gclouds, p1.ncol)
    assert_production(p1.go_lw, p1.go_sw)
    check_tau_gas(lib, entry, device, pipe, p1.bands, p1.ncol, V1 - 1, lambda bi, c: p1.clear(bi, c)["tau_gas"])
    for bi, (key, lw) in enumerate(BANDS):
        for c, col in enumerate(p1.cols):
            what = f"{key} column {c}"
            w = p1.allsky(bi, c) if allsky else p1.clear(bi, c)
            check_six(lib, entry, what, got["six"][c, 6 * bi: 6 * bi + 6], w, UL1)
            if allsky:
                check_six(lib, entry, what + " clear set", got["clear"][c, 6 * bi: 6 * bi + 6], p1.clear(bi, c), UL1)
            if profile:
                check_profile(lib, entry, what, got["prof"], c, key, col, w)
                if allsky:
                    check_profile(lib, entry, what + " clear set", got["clear_prof"], c, key, col, p1.clear(bi, c))
            if spectral:
                check_level_spectra(lib, entry, what, device, pipe, bi, p1.bands[bi], p1.ncol, V1, c, w)
    p1.close()


def want_bins(orc, rows, edges, dw):
    return np.array([[orc.integrate_row(r[edges[b]:edges[b + 1] + 1], dw) for b in range(edges.size - 1)] for r in rows])


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
@pytest.mark.parametrize("allsky", [False, True], ids=["clear", "allsky"])
def test_run_spectral_matches_the_oracle(p1, tables, oracle, lib, device, allsky, spectral):
    """The six rows at every grid point, their bins on 128-point block boundaries, and the call's broadband values."""
    entry = "run_spectral"
    pipe = p1.open(spectral)
    gclouds, keep_clouds = make(tables, p1.cl) if allsky else (None, None)
    edges = [block_edges(b.nw) for b in p1.bands]
    pipe.run_spectral(p1.gcols, gclouds, *edges)
    got = pipe.spectral(p1.ncol)
    assert_production(p1.go_lw, p1.go_sw)
    check_tau_gas(lib, entry, device, pipe, p1.bands, p1.ncol, V1 - 1, lambda bi, c: p1.clear(bi, c)["tau_gas"])
    for bi, (key, lw) in enumerate(BANDS):
        band = p1.bands[bi]
        for c in range(p1.ncol):
            for s in range(2 if allsky else 1):
                what = f"{key} column {c} set {s}"
                w = p1.allsky(bi, c) if s == 1 else p1.clear(bi, c)
                want = spectral_rows(w, UL1)
                scale = max(np.abs(w["up"]).max(), np.abs(w["dn"]).max())
                d = np.abs(got[key][c, s] - want)
                err = note(lib, entry, "rows_rel", d.max() / scale, SPECTRAL_REL)
                r, i = np.unravel_index(d.argmax(), d.shape)
                assert err <= SPECTRAL_REL, f"{what}: {err} of the band's largest flux in row {r} at point {i}"
                d = np.abs(got[key + "_bins"][c, s] - want_bins(oracle, want, edges[bi], band.dw))
                err = note(lib, entry, "bin_w_m2", d.max(), BIN_TOL)
                r, b = np.unravel_index(d.argmax(), d.shape)
                assert err <= BIN_TOL, f"{what}: bin {b} of row {r} {err} W m-2 from the oracle's"
                check_six(lib, entry, what, got["fluxes"][c, 12 * s + 6 * bi: 12 * s + 6 * bi + 6], w, UL1)
    p1.close()


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
@pytest.mark.parametrize("S", [1, SUB_S])
def test_run_subcolumns_matches_the_oracle(p1, tables, lib, device, S, spectral):
    """The six-row and the profile form; S = 1 draws the all-sky cases' cloud, whose oracle result it shares."""
    entry = "run_subcolumns"
    cl = subcolumn_clouds(p1.cols, tables, CLOUD_SEED if S == 1 else SUB_SEED, S)
    if S == 1:
        assert all(np.array_equal(cl[k][:, 0], p1.cl[k]) for k in SETS)
    pipe = p1.open(spectral)
    gclouds, keep_clouds = make(tables, cl)
    pipe.run_subcolumns(p1.gcols, gclouds, S)
    clear6, cloudy6 = pipe.subcolumn_fluxes(p1.ncol)
    assert_production(p1.go_lw, p1.go_sw)
    pipe.run_subcolumns(p1.gcols, gclouds, S, profiles=True)
    clear, cloudy = pipe.subcolumn_profiles(p1.ncol)
    assert_production(p1.go_lw, p1.go_sw)
    check_tau_gas(lib, entry, device, pipe, p1.bands, p1.ncol, V1 - 1, lambda bi, c: p1.clear(bi, c)["tau_gas"])
    for bi, (key, lw) in enumerate(BANDS):
        for c, col in enumerate(p1.cols):
            what = f"{key} column {c} S {S}"
            w = p1.allsky(bi, c) if S == 1 else p1.subcolumns(bi, c, cl)
            rows = slice(6 * bi, 6 * bi + 6)
            check_six(lib, entry, what, cloudy6[c, rows], w, UL1)
            check_six(lib, entry, what + " clear set", clear6[c, rows], p1.clear(bi, c), UL1)
            check_six(lib, entry, what + " profile form", cloudy["fluxes"][c, rows], w, UL1)
            check_profile(lib, entry, what, cloudy, c, key, col, w)
            check_profile(lib, entry, what + " clear set", clear, c, key, col, p1.clear(bi, c))
    p1.close()


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
@pytest.mark.parametrize("profiles", [False, True], ids=["six", "profiles"])
def test_run_aerosols_matches_the_oracle(p1, lib, device, profiles, spectral):
    entry = "run_aerosols"
    pipe = p1.open(spectral)
    gaer, keep_aer = api.make_aerosols(lw=(AEROSOL_GRID, p1.lw_f), sw=(AEROSOL_GRID, p1.sw_f))
    pipe.run_aerosols(p1.gcols, gaer, profiles=profiles)
    if profiles:
        clean, aer = pipe.aerosol_profiles(p1.ncol)
    else:
        clean, aer = (dict(fluxes=f) for f in pipe.aerosol_fluxes(p1.ncol))
    assert_production(p1.go_lw, p1.go_sw)
    check_tau_gas(lib, entry, device, pipe, p1.bands, p1.ncol, V1 - 1, lambda bi, c: p1.clear(bi, c)["tau_gas"])
    for bi, (key, lw) in enumerate(BANDS):
        for c, col in enumerate(p1.cols):
            what = f"{key} column {c}"
            w = p1.aerosol(bi, c)
            rows = slice(6 * bi, 6 * bi + 6)
            check_six(lib, entry, what, aer["fluxes"][c, rows], w, UL1)
            check_six(lib, entry, what + " clean set", clean["fluxes"][c, rows], p1.clear(bi, c), UL1)
            if profiles:
                check_profile(lib, entry, what, aer, c, key, col, w)
                check_profile(lib, entry, what + " clean set", clean, c, key, col, p1.clear(bi, c))
            if spectral:
                check_level_spectra(lib, entry, what, device, pipe, bi, p1.bands[bi], p1.ncol, V1, c, w)
    p1.close()


# ---- 2. identities that do not depend on the arithmetic form ------------------------------------------------------------- #
@pytest.fixture
def deterministic(lib):
    api.check(lib.grt_set_deterministic(1))
    yield
    api.check(lib.grt_set_deterministic(-1))


PIN_TILE = 128     # a power of two (the two-pass form's cell tiles) below both grids' lengths


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
@pytest.mark.parametrize("entry", ["run_profiles", "run_allsky_profiles", "run_allsky"])
def test_a_column_does_not_depend_on_its_batch(p1, tables, lib, device, deterministic, entry, spectral):
    """Column c of a batch is the column run alone, and a permuted batch gives the permuted results, bit for bit.  tile and
    nslice are pinned (auto_tune reads ncol), and on these single-level grids plan() derives nothing else from the batch
    that reaches the arithmetic: rcap is 12 and halo the window; the tile tables' pressure bound (the batch's largest
    pressure) only widens each tile's candidate list, membership is decided line by line in the kernel; the work list is
    off in the deterministic mode.  (The tree form's halo does follow the batch: test_cell_hierarchy_feeds_the_solvers.)"""
    pipe = p1.open(spectral, tile=PIN_TILE)
    allsky = "allsky" in entry

    def run(order):
        gcols, keep = api.make_columns([p1.cols[i] for i in order], MOL_ORDER, cfc_order=(0, 1))
        g, k = make(tables, pick(p1.cl, columns=order)) if allsky else (None, None)
        r = bits(run_entry(pipe, entry, gcols, g, len(order)))
        assert_production(p1.go_lw, p1.go_sw)
        return r, (shape_of(p1.go_lw), shape_of(p1.go_sw))

    whole, shape = run(range(p1.ncol))
    assert shape[0][1] == PIN_TILE and shape[1][1] == PIN_TILE and shape[0][2] == 1, shape
    assert len({whole[0][c].tobytes() for c in range(p1.ncol)}) == p1.ncol          # the columns differ
    for c in range(p1.ncol):
        one, shape1 = run([c])
        assert shape1 == shape, (shape1, shape)
        assert all(np.array_equal(a[0], b[c]) for a, b in zip(one, whole)), (entry, c)
    order = [2, 0, 3, 1]
    perm, shape_p = run(order)
    assert shape_p == shape
    assert all(np.array_equal(a, b[order]) for a, b in zip(perm, whole)), entry
    p1.close()


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
def test_clear_sets_and_inputs_of_zeros(p1, tables, lib, device, deterministic, spectral):
    """The clear-sky set of the all-sky forms is run / run_profiles; a cloud of zeros gives the clear set; one subcolumn is
    the all-sky form; an aerosol of zeros gives the clean set, which is run / run_profiles too."""
    pipe = p1.open(spectral)
    gclouds, keep_clouds = make(tables, p1.cl)
    n = p1.ncol
    run = run_entry(pipe, "run", p1.gcols, None, n)
    prof = run_entry(pipe, "run_profiles", p1.gcols, None, n)
    a6 = run_entry(pipe, "run_allsky", p1.gcols, gclouds, n)
    ap = run_entry(pipe, "run_allsky_profiles", p1.gcols, gclouds, n)
    assert_production(p1.go_lw, p1.go_sw)
    assert np.array_equal(a6["clear"], run["six"])
    assert not np.array_equal(a6["six"], a6["clear"])
    assert all(np.array_equal(ap["clear_prof"][k], prof["prof"][k]) for k in KEYS)
    # a cloud of zeros
    zero = cloud_columns(p1.cols, tables, CLOUD_SEED, clear=True)
    assert all(np.all(zero[k] == 0.0) for k in SETS)
    gzero, keep_zero = make(tables, zero)
    z6 = run_entry(pipe, "run_allsky", p1.gcols, gzero, n)
    zp = run_entry(pipe, "run_allsky_profiles", p1.gcols, gzero, n)
    assert np.array_equal(z6["six"], z6["clear"]) and np.array_equal(z6["clear"], run["six"])
    assert all(np.array_equal(zp["prof"][k], zp["clear_prof"][k]) for k in KEYS)
    # one subcolumn
    g1, k1 = make(tables, subcolumn_clouds(p1.cols, tables, CLOUD_SEED, 1))
    pipe.run_subcolumns(p1.gcols, g1, 1)
    s_clear, s_cloudy = pipe.subcolumn_fluxes(n)
    assert np.array_equal(s_clear, a6["clear"]) and np.array_equal(s_cloudy, a6["six"])
    pipe.run_subcolumns(p1.gcols, g1, 1, profiles=True)
    sp = pipe.subcolumn_profiles(n)
    for got, want in zip(sp, (ap["clear_prof"], ap["prof"])):
        assert all(np.array_equal(got[k], want[k]) for k in KEYS)
    # an aerosol of zeros
    z = np.zeros((n, 3, V1 - 1, AEROSOL_GRID.size))
    gaer, keep_aer = api.make_aerosols(lw=(AEROSOL_GRID, z), sw=(AEROSOL_GRID, z))
    pipe.run_aerosols(p1.gcols, gaer)
    clean6, aer6 = pipe.aerosol_fluxes(n)
    assert np.array_equal(clean6, aer6) and np.array_equal(clean6, run["six"])
    pipe.run_aerosols(p1.gcols, gaer, profiles=True)
    clean, aer = pipe.aerosol_profiles(n)
    assert all(np.array_equal(clean[k], aer[k]) and np.array_equal(clean[k], prof["prof"][k]) for k in KEYS)
    assert_production(p1.go_lw, p1.go_sw)
    p1.close()


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
@pytest.mark.parametrize("user_level", [-1, 0, 7, V1 - 1])
def test_profile_rows_are_the_six_rows_with_two_sweeps(p1, tables, lib, device, deterministic, monkeypatch, user_level,
                                                      spectral):
    monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
    pipe = p1.open(spectral, user_level=user_level)
    gclouds, keep_clouds = make(tables, p1.cl)
    L, n = V1 - 1, p1.ncol
    for six_entry, prof_entry in (("run", "run_profiles"), ("run_allsky", "run_allsky_profiles")):
        sr = run_entry(pipe, six_entry, p1.gcols, gclouds, n)
        pr = run_entry(pipe, prof_entry, p1.gcols, gclouds, n)
        assert_production(p1.go_lw, p1.go_sw)
        sets = [(pr["prof"], sr["six"])] + ([(pr["clear_prof"], sr["clear"])] if sr["clear"] is not None else [])
        for prof, six_all in sets:
            assert np.array_equal(prof["fluxes"], six_all)
            for bi, (key, lw) in enumerate(BANDS):
                s6 = six_all[:, 6 * bi: 6 * bi + 6]
                up, dn = prof[key + "_up"], prof[key + "_down"]
                assert np.array_equal(up[:, 0], s6[:, 0]) and np.array_equal(up[:, L], s6[:, 1]), (prof_entry, key)
                assert np.array_equal(dn[:, 0], s6[:, 3]) and np.array_equal(dn[:, L], s6[:, 4]), (prof_entry, key)
                if user_level >= 0:
                    assert np.array_equal(up[:, user_level], s6[:, 2]) and np.array_equal(dn[:, user_level], s6[:, 5])
                else:
                    assert np.all(s6[:, [2, 5]] == 0.0)
    p1.close()


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
def test_bins_add_up_and_the_whole_grid_is_the_broadband_value(p1, tables, lib, device, deterministic, spectral):
    pipe = p1.open(spectral)
    gclouds, keep_clouds = make(tables, p1.cl)
    n = p1.ncol
    whole = [np.array([0, b.nw - 1], np.int32) for b in p1.bands]
    pipe.run_spectral(p1.gcols, gclouds, *whole)
    got = pipe.spectral(n)
    assert_production(p1.go_lw, p1.go_sw)
    for s in range(2):
        for bi, (key, lw) in enumerate(BANDS):
            s6 = got["fluxes"][:, 12 * s + 6 * bi: 12 * s + 6 * bi + 6]
            binned = got[key + "_bins"][:, s, :, 0]
            if not spectral:
                assert np.array_equal(binned, s6), (key, s)
            else:
                assert np.max(np.abs(binned - s6)) <= 1e-12 * np.abs(s6).max(), (key, s)
    # contiguous bins against their union (test_contiguous_bins_add_up_and_one_interval_bins_are_the_trapezoid's bound)
    fine = [block_edges(b.nw) for b in p1.bands]
    pipe.run_spectral(p1.gcols, gclouds, *fine)
    parts = pipe.spectral(n)
    for lo, hi in ((0, 3), (2, 7), (1, fine[0].size - 1)):
        union = [np.array([e[lo], e[min(hi, e.size - 1)]], np.int32) for e in fine]
        pipe.run_spectral(p1.gcols, gclouds, *union)
        u = pipe.spectral(n)
        for bi, (key, lw) in enumerate(BANDS):
            h = min(hi, fine[bi].size - 1)
            p = parts[key + "_bins"][:, :, :, lo:h]
            assert np.all(np.abs(p.sum(axis=-1) - u[key + "_bins"][:, :, :, 0]) <= 1e-12 * np.abs(p).sum(axis=-1)), (key, lo, hi)
    p1.close()


@pytest.mark.parametrize("entry", ["run_profiles", "run_allsky"])
def test_column_groups_give_the_bits_of_the_undivided_batch(bands, tables, lib, device, deterministic, monkeypatch, entry):
    """Eight columns whose moments are capped to three columns' room in the longwave object (GRT_SCRATCH_CAP_MB,
    test_gpu_batch.py): groups of 3, 3 and 2 through one scratch, every group with the plan of the undivided batch -- the
    same integrated fluxes and heating rates to the last bit.  (The cap is one number for both bands; the shortwave band's
    columns are larger, so it runs in groups too, of fewer columns.)"""
    ncol = 8
    cols = varied_columns(810, V1) + varied_columns(820, V1, pressure=0.97)
    cl = cloud_columns(cols[:4], tables, 74)
    cl2 = cloud_columns(cols[4:], tables, 75)
    cl = {k: np.concatenate([cl[k], cl2[k]]) for k in cl}
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, cl)
    got, info = {}, {}
    for grouped in (False, True):
        go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1, fast=FAST)       # fresh objects: nothing allocated yet
        pipe = api.Pipeline(go_lw, go_sw, ncol, 4, emis, alb, solar, spectral=False)
        if grouped:
            per_col = info[False][0]["moment_bytes"] / ncol
            monkeypatch.setenv("GRT_SCRATCH_CAP_MB", repr(3.5 * per_col / 1048576.0))
        got[grouped] = bits(run_entry(pipe, entry, gcols, gclouds, ncol))
        info[grouped] = (go_lw.last_launch(), go_sw.last_launch())
        assert_production(go_lw, go_sw)
        shapes = (shape_of(go_lw), shape_of(go_sw))
        if grouped:
            assert shapes == info["shapes"], (shapes, info["shapes"])
        info["shapes"] = shapes
        pipe.destroy()
        go_lw.destroy()
        go_sw.destroy()
    monkeypatch.delenv("GRT_SCRATCH_CAP_MB")
    assert info[False][0]["columns_per_launch"] == ncol and info[False][1]["columns_per_launch"] == ncol, info
    assert info[True][0]["columns_per_launch"] == 3, info
    assert 1 <= info[True][1]["columns_per_launch"] <= 3, info
    assert same_bits(got[True], got[False]), entry
    assert len({got[False][0][c].tobytes() for c in range(ncol)}) == ncol


@pytest.mark.parametrize("entry", ["run_profiles", "run_aerosols"])
def test_continua_in_the_solver_or_in_the_gas_optics_kernel_same_bits(p1, lib, device, deterministic, monkeypatch, entry):
    """GRT_DEFER_CONTINUA=1 (the shortwave solver adds the spectral tables' part of tau: skip_tables) against 0 (the
    gas-optics kernel adds it), production form: the same levels, heating rates and fluxes."""
    gaer, keep_aer = api.make_aerosols(lw=(AEROSOL_GRID, p1.lw_f), sw=(AEROSOL_GRID, p1.sw_f))
    got = {}
    for defer in ("1", "0"):
        monkeypatch.setenv("GRT_DEFER_CONTINUA", defer)
        pipe = p1.open(False)
        if entry == "run_profiles":
            pipe.run_profiles(p1.gcols)
            sets = (pipe.profiles(p1.ncol),)
        else:
            pipe.run_aerosols(p1.gcols, gaer, profiles=True)
            sets = pipe.aerosol_profiles(p1.ncol)
        assert_production(p1.go_lw, p1.go_sw)
        got[defer] = [s[k] for s in sets for k in KEYS]
        p1.close()
    assert same_bits(got["1"], got["0"])
    assert np.all(got["1"][KEYS.index("sw_down")][:, -1] > 0.0)


# ---- 3. edge shapes ------------------------------------------------------------------------------------------------------ #
# Per entry point one case per grid length of SOLVER_NS; every level count (2, 3, 7, 8, 61, 201) with every entry point, 201
# levels on grids of 65 points or fewer (the oracle's share of the run time); user levels -1, 0 and L rotating.
VS = {"run": (201, 2, 61, 7, 8, 3, 2), "run_profiles": (2, 201, 7, 61, 3, 8, 7),
      "run_allsky": (3, 61, 201, 2, 7, 61, 8), "run_allsky_profiles": (61, 3, 2, 201, 8, 7, 3)}
ULS = {"run": ("-1", "0", "L", "-1", "0", "L", "-1"), "run_profiles": ("0", "L", "-1", "0", "L", "-1", "0"),
       "run_allsky": ("L", "-1", "0", "L", "-1", "0", "L"), "run_allsky_profiles": ("-1", "L", "0", "L", "0", "-1", "0")}
CASES = [(e, VS[e][k], n, ULS[e][k]) for e in ENTRIES for k, n in enumerate(SOLVER_NS)]


@pytest.mark.parametrize("entry,V,n,ul", CASES, ids=[f"{e}-V{V}-n{n}-ul{u}" for e, V, n, u in CASES])
def test_pipeline_at_edge_shapes(solver_bands, tables, oracle, lib, device, entry, V, n, ul):
    """A few hundred lines on 2 to 257 points: the +-25 cm-1 window is wider than the grid, the cell tile is wider than the
    grid, most lines sit outside it; one-layer columns to MAX_NUM_LEVELS; cos(zenith) down to 1e-3."""
    L = V - 1
    user_level = user_index(ul, L)
    pair = solver_bands[n]
    allsky, profile = "allsky" in entry, "profiles" in entry
    cols = columns(V)
    ncol = len(cols)
    go_lw, _ = pair[0].gas_optics(device, V, fast=FAST)
    go_sw, grid_sw = pair[1].gas_optics(device, V, fast=FAST)
    emis, _ = surface(n, 1 + n)
    _, alb = surface(n, 2 + n)
    solar = api.create_solar_flux(grid_sw, pair[1].files["solar"])
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = clouds_for(cols, tables, 30 + V) if allsky else None
    gclouds, keep_clouds = make(tables, cl) if allsky else (None, None)
    name = "edge_shapes." + entry
    want, clear = {}, {}
    for bi, (key, lw) in enumerate(BANDS):
        for c, col in enumerate(cols):
            clear[bi, c] = oracle_column(oracle, lib, pair[bi], col, lw, emis, alb, solar)
            if allsky:
                want[bi, c] = oracle_allsky_levels(oracle, lib, pair[bi], col, lw, tables, cl[key + "_liquid"][c],
                                                   cl[key + "_ice"][c], cl["thickness"][c], emis, alb, solar)
            else:
                want[bi, c] = clear[bi, c]
            with_integrals(oracle, pair[bi], want[bi, c])
            with_integrals(oracle, pair[bi], clear[bi, c])
    for spectral in (False, True):
        pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)
        got = run_entry(pipe, entry, gcols, gclouds, ncol)
        assert_production(go_lw, go_sw)
        check_tau_gas(lib, name, device, pipe, pair, ncol, L, lambda bi, c: clear[bi, c]["tau_gas"])
        for bi, (key, lw) in enumerate(BANDS):
            for c, col in enumerate(cols):
                what = f"{key} column {c} {'materialised' if spectral else 'fused'}"
                w = want[bi, c]
                check_six(lib, name, what, got["six"][c, 6 * bi: 6 * bi + 6], w, user_level)
                if allsky:
                    check_six(lib, name, what + " clear set", got["clear"][c, 6 * bi: 6 * bi + 6], clear[bi, c], user_level)
                if profile:
                    check_profile(lib, name, what, got["prof"], c, key, col, w)
                    if allsky:
                        check_profile(lib, name, what + " clear set", got["clear_prof"], c, key, col, clear[bi, c])
                if spectral:
                    check_level_spectra(lib, name, what, device, pipe, bi, pair[bi], ncol, V, c, w)
        pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def one_band_case(lib, device, oracle, name, band, cols, oracle_column_index, expect_tree, pin_tile):
    """A longwave-only pipeline on `band`, V = 9, run and run_profiles, fused and materialised: tau_gas and the integrated
    fluxes of one column against the oracle, the other columns against themselves run alone."""
    V = cols[0]["p"].size
    L, ncol = V - 1, len(cols)
    go, grid = band.gas_optics(device, V, from_file=False, fast=FAST)
    if pin_tile:
        go.tune(tile=pin_tile, nslice=1, fast=FAST)
    emis = np.full(band.nw, 0.98)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    c0 = oracle_column_index
    w = with_integrals(oracle, band, oracle_column(oracle, lib, band, cols[c0], True, emis))
    api.check(lib.grt_set_deterministic(1))
    try:
        for spectral in (False, True):
            pipe = api.Pipeline(go, None, ncol, 3, emis, None, None, spectral=spectral)
            for entry in ("run", "run_profiles"):
                got = run_entry(pipe, entry, gcols, None, ncol)
                info = go.last_launch()
                assert info["fast"] == FAST and (info["tree_levels"] > 0) == expect_tree, info
                shape = shape_of(go)
                tau = api.device_to_host(device, pipe.views(0)["tau_gas"], (ncol, L, band.nw)).copy()
                check_tau_gas(lib, name, device, pipe, (band,), ncol, L, lambda bi, c: w["tau_gas"] if c == c0 else tau[c])
                check_six(lib, name, f"column {c0}", got["six"][c0, :6], w, 3)
                assert np.all(got["six"][:, 6:] == 0.0)                         # no shortwave band
                if entry == "run_profiles":
                    check_profile(lib, name, f"column {c0}", got["prof"], c0, "lw", cols[c0], w)
                whole = bits(got)
                for c in range(ncol):
                    if c == c0:
                        continue
                    g1, k1 = api.make_columns([cols[c]], MOL_ORDER, cfc_order=(0, 1))
                    one = bits(run_entry(pipe, entry, g1, None, 1))
                    tau1 = api.device_to_host(device, pipe.views(0)["tau_gas"], (1, L, band.nw))[0]
                    if shape_of(go) == shape:
                        assert np.array_equal(tau1, tau[c]), (entry, c)
                        assert all(np.array_equal(a[0], b[c]) for a, b in zip(one, whole)), (entry, c)
                    else:
                        # the launch's shape followed the batch (the tree form's halo): through part 1's bounds
                        layer_max = np.abs(tau1).max(axis=1, keepdims=True)
                        err = note(lib, name, "batch_vs_alone_tau_of_layer_max", np.max(np.abs(tau[c] - tau1) / layer_max), TAU_TOL)
                        assert err <= TAU_TOL, (entry, c, err)
                        err = note(lib, name, "batch_vs_alone_flux_w_m2", max(np.max(np.abs(a[0] - b[c])) for a, b in
                                                                                zip(one[:1], whole[:1])), FLUX_TOL)
                        assert err <= FLUX_TOL, (entry, c, err)
            pipe.destroy()
    finally:
        api.check(lib.grt_set_deterministic(-1))
    go.destroy()


def test_cell_hierarchy_feeds_the_solvers(tmp_path, oracle, lib, device):
    """2000-2060 cm-1 at 0.002 cm-1 (test_gpu_batch.py's tree case): windows of 12 500 points a side, far field through the
    cell hierarchy.  Column 1 against the oracle.  A column alone against the column in the batch: near_halo_bound() takes
    the hierarchy's halo from the batch's widest line, and in the deterministic mode the first pass's phases follow the halo
    (nphase = 2 halo/tile + 2), so where the alone launch's shape differs from the batch's the comparison is held to the
    tau and flux bounds, and to equal bits where it does not."""
    band = Band(str(tmp_path), 2000.0, 2060.0, 0.002, 2500)
    one_band_case(lib, device, oracle, "cell_hierarchy", band, varied_columns(830, 9, 3), 1, True, 0)


def test_wide_near_field_under_three_atmospheres_feeds_the_solvers(tmp_path, oracle, lib, device):
    """600-800 cm-1 at 0.5 cm-1 under three times the surface pressure (test_high_pressure_widens_the_near_field): Lorentz
    widths of several tenths of a grid step in the lowest layers, a near-field radius that differs from layer to layer and
    from column to column (near_radius_kernel).  The thinnest column comes first and the oracle's column, the thickest,
    second: a radius taken from another column would be too small for it.  Single-level form, tile pinned: a column alone
    has the batch's bits."""
    band = Band(str(tmp_path), 600.0, 800.0, 0.5, 6000)
    cols = varied_columns(840, 9, 4, pressure=3.0, factors=(0.8, 1.03, 0.9, 1.0))
    one_band_case(lib, device, oracle, "three_atmospheres", band, cols, 1, False, 128)
