"""The fused and spectral solver kernels at the shapes where a kernel goes wrong: one-layer columns and the level counts
around the sweeps' six-layer chunk up to MAX_NUM_LEVELS, grids of one and two lanes, one block, an exact multiple of the
solver block and one live lane past it, the user level at and next to both ends, and columns of one launch whose direct
beam is clamped and whose is not.  Each case runs the batched pipeline's four entry points against the oracle, its
integrals against an exactly rounded trapezoid of the kernel's own spectra, and the bit-for-bit identities of the
deterministic mode.  Also: the spectral tables the shortwave solver adds beyond the ones it keeps in registers, the
reference-shaped solvers at the same shapes, and what the library refuses."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api, synthetic as syn
from pipeline_support import (CP, ENTRIES, GRAVITY, LEVEL_TOL, MU0, SOLVER_NS as NS, assert_trapezoid, clouds_for, columns,
                              heating, make, oracle_allsky_levels, oracle_column, run_entry, surface, user_index)
from pipeline_support import solver_bands as bands, tables  # noqa: F401  (module fixtures)
from scenario import Band, MOL_ORDER
from test_gpu_optics_solvers import random_optics

pytestmark = pytest.mark.gpu

# Per entry point, one case per grid length; each level count and user level (-1, 0, 1, L-1, L) appears with every entry
# point, and 201 levels only on grids of 65 points or fewer (the oracle's share of the run time).
VS = {"run": (201, 2, 3, 7, 8, 2, 3), "run_profiles": (2, 201, 7, 8, 3, 7, 8),
      "run_allsky": (3, 7, 201, 2, 8, 3, 2), "run_allsky_profiles": (7, 8, 2, 201, 3, 8, 7)}
ULS = {"run": ("-1", "0", "1", "L-1", "L", "0", "L"), "run_profiles": ("0", "1", "L-1", "L", "-1", "1", "L-1"),
       "run_allsky": ("1", "L-1", "L", "-1", "0", "L", "-1"), "run_allsky_profiles": ("L-1", "L", "-1", "0", "1", "-1", "0")}
CASES = [(e, VS[e][k], n, ULS[e][k]) for e in ENTRIES for k, n in enumerate(NS)]


@pytest.mark.parametrize("entry,V,n,ul", CASES, ids=[f"{e}-V{V}-n{n}-ul{u}" for e, V, n, u in CASES])
def test_pipeline_at_edge_shapes(bands, tables, oracle, lib, device, monkeypatch, entry, V, n, ul):
    L = V - 1
    user_level = user_index(ul, L)
    lwb, swb = bands[n]
    allsky = "allsky" in entry
    profile = "profiles" in entry
    cols = columns(V)
    ncol = len(cols)
    go_lw, _ = lwb.gas_optics(device, V)
    go_sw, grid_sw = swb.gas_optics(device, V)
    emis, _ = surface(n, 1 + n)
    _, alb = surface(n, 2 + n)
    solar = api.create_solar_flux(grid_sw, swb.files["solar"])
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = clouds_for(cols, tables, 30 + V) if allsky else None
    gclouds, keep_clouds = make(tables, cl) if allsky else (None, None)
    fused = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=False)
    mat = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=True)
    pipes = (fused, mat)

    # ---- the default mode against the oracle: levels, six rows, heating rates --------------------------------------- #
    got = {False: run_entry(fused, entry, gcols, gclouds, ncol), True: run_entry(mat, entry, gcols, gclouds, ncol)}
    views = [mat.views(bi) for bi in range(2)]
    spec = [(api.device_to_host(device, v["flux_up"], (ncol, V, b.nw)), api.device_to_host(device, v["flux_down"], (ncol, V, b.nw)))
            for v, b in zip(views, (lwb, swb))]
    for bi, (band, lw, key) in enumerate(((lwb, True, "lw"), (swb, False, "sw"))):
        for c, col in enumerate(cols):
            if allsky:
                w = oracle_allsky_levels(oracle, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
                                         cl["thickness"][c], emis, alb, solar)
            else:
                w = oracle_column(oracle, lib, band, col, lw, emis, alb, solar)
            up_w = np.array([oracle.integrate_row(w["up"][k], band.dw) for k in range(V)])
            dn_w = np.array([oracle.integrate_row(w["dn"][k], band.dw) for k in range(V)])
            fs = max(np.abs(w["up"]).max(), np.abs(w["dn"]).max())
            assert fs > 0.0
            assert np.max(np.abs(spec[bi][0][c] - w["up"])) <= LEVEL_TOL * fs, key
            assert np.max(np.abs(spec[bi][1][c] - w["dn"])) <= LEVEL_TOL * fs, key
            ff = max(np.abs(up_w).max(), np.abs(dn_w).max())
            six_w = np.array([up_w[0], up_w[L], up_w[user_level] if user_level >= 0 else 0.0,
                              dn_w[0], dn_w[L], dn_w[user_level] if user_level >= 0 else 0.0])
            for form in (False, True):
                six = got[form]["six"][c, 6 * bi: 6 * bi + 6]
                assert np.max(np.abs(six - six_w)) <= LEVEL_TOL * ff, (key, form)
                if user_level < 0:
                    assert six[2] == 0.0 and six[5] == 0.0
                if not profile:
                    continue
                p = got[form]["prof"]
                up, dn, hr = p[key + "_up"][c], p[key + "_down"][c], p[key + "_heating"][c]
                assert np.max(np.abs(up - up_w)) <= LEVEL_TOL * ff, (key, form)
                assert np.max(np.abs(dn - dn_w)) <= LEVEL_TOL * ff, (key, form)
                # the heating rate of a layer moves with its two levels' net fluxes over the layer's mass
                mass = 100.0 * (col["p"][1:] - col["p"][:-1]) / GRAVITY
                bound = 4.0 * LEVEL_TOL * ff / (CP * mass) * 86400.0
                want_hr = heating(up_w, dn_w, col["p"])
                assert np.all(np.abs(hr - want_hr) <= bound + 1e-12 * np.abs(want_hr).max()), (key, form)

    # ---- the deterministic mode: exact trapezoid of the kernel's own spectra, and bit-for-bit identities ----------- #
    api.check(lib.grt_set_deterministic(1))
    try:
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        det = {False: run_entry(fused, entry, gcols, gclouds, ncol), True: run_entry(mat, entry, gcols, gclouds, ncol)}
        spec = [(api.device_to_host(device, v["flux_up"], (ncol, V, b.nw)),
                 api.device_to_host(device, v["flux_down"], (ncol, V, b.nw))) for v, b in zip(views, (lwb, swb))]
        for bi, (band, key) in enumerate(((lwb, "lw"), (swb, "sw"))):
            up_s, dn_s = spec[bi]
            for c in range(ncol):
                for form in (False, True):
                    six = det[form]["six"][c, 6 * bi: 6 * bi + 6]
                    for r, (rows, lev) in enumerate(((up_s, 0), (up_s, L), (up_s, user_level),
                                                     (dn_s, 0), (dn_s, L), (dn_s, user_level))):
                        if lev >= 0:
                            assert_trapezoid(six[r], rows[c, lev], band.dw, (key, form, r))
                    if profile:
                        p = det[form]["prof"]
                        for k in range(V):
                            assert_trapezoid(p[key + "_up"][c, k], up_s[c, k], band.dw, (key, form, "up", k))
                            assert_trapezoid(p[key + "_down"][c, k], dn_s[c, k], band.dw, (key, form, "down", k))
        # the six-row forms against the profile forms (shortwave: both take two sweeps here)
        if profile:
            six_entry = "run_allsky" if allsky else "run"
            for form in (False, True):
                sr = run_entry(pipes[int(form)], six_entry, gcols, gclouds, ncol)
                pr = det[form]
                sets = [(pr["prof"], sr["six"])] + ([(pr["clear_prof"], sr["clear"])] if allsky else [])
                for prof, six_all in sets:
                    for bi, key in enumerate(("lw", "sw")):
                        six = six_all[:, 6 * bi: 6 * bi + 6]
                        up, dn = prof[key + "_up"], prof[key + "_down"]
                        assert np.array_equal(up[:, 0], six[:, 0]) and np.array_equal(up[:, L], six[:, 1]), (key, form)
                        assert np.array_equal(dn[:, 0], six[:, 3]) and np.array_equal(dn[:, L], six[:, 4]), (key, form)
                        if user_level >= 0:
                            assert np.array_equal(up[:, user_level], six[:, 2]), (key, form)
                            assert np.array_equal(dn[:, user_level], six[:, 5]), (key, form)
                        else:
                            assert np.all(six[:, [2, 5]] == 0.0)
        else:
            # one shortwave sweep against two: surface and top-down the same doubles, top-up to rounding
            monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "0")
            one = run_entry(fused, entry, gcols, gclouds, ncol)
            two = det[False]
            for a, b in ((one["six"], two["six"]),) + (((one["clear"], two["clear"]),) if allsky else ()):
                assert np.array_equal(a[:, :6], b[:, :6])                       # longwave: untouched
                exact = [7, 9, 10, 11] + ([8] if user_level != 0 else [])       # up at the user level = up at the top
                assert np.array_equal(a[:, exact], b[:, exact])
                top_up = [6] + ([8] if user_level == 0 else [])
                assert np.max(np.abs(a[:, top_up] - b[:, top_up])) <= 1e-13 * np.abs(b[:, 6:]).max()
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        # no cloud: the all-sky sets are the clear ones
        if allsky:
            cl_clear = clouds_for(cols, tables, 30 + V, clear=True)
            assert all(np.all(cl_clear[k][:, 0] == 0.0) for k in ("lw_liquid", "lw_ice", "sw_liquid", "sw_ice"))
            gclear, keep_clear = make(tables, cl_clear)
            for pipe in pipes:
                r = run_entry(pipe, entry, gcols, gclear, ncol)
                assert np.array_equal(r["six"], r["clear"])
                if profile:
                    assert all(np.array_equal(r["prof"][k], r["clear_prof"][k]) for k in r["prof"])
    finally:
        api.check(lib.grt_set_deterministic(-1))
    for pipe in pipes:
        pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- what the library refuses --------------------------------------------------------------------------------------- #
def test_refusals(bands, lib, device):
    lwb, swb = bands[3]
    V = 7
    cols = columns(V)
    go_lw, _ = lwb.gas_optics(device, V)
    go_sw, grid_sw = swb.gas_optics(device, V)
    emis, alb = surface(3, 1)
    solar = api.create_solar_flux(grid_sw, swb.files["solar"])
    grid = api.create_spectral_grid(lwb.w0, lwb.wn, lwb.dw)
    with pytest.raises(api.GrtError) as e:                       # V = 202 > MAX_NUM_LEVELS
        api.GasOpticsObject(202, grid, device, lwb.par)
    assert e.value.code == api.RANGE_ERR
    for ul in (V, V + 3, -2, -7):                                # user level past the surface or below -1
        with pytest.raises(api.GrtError) as e:
            api.Pipeline(go_lw, go_sw, 2, ul, emis, alb, solar, spectral=False)
        assert e.value.code == api.RANGE_ERR, ul
    for spectral in (False, True):
        pipe = api.Pipeline(go_lw, go_sw, len(cols), 0, emis, alb, solar, spectral=spectral)
        for mu in (0.0, -0.5, 1.0 + 1e-12, 2.0):
            bad = [dict(c) for c in cols]
            bad[2]["mu0"] = mu
            gcols, keep = api.make_columns(bad, MOL_ORDER, cfc_order=(0, 1))
            with pytest.raises(api.GrtError) as e:
                pipe.run(gcols)
            assert e.value.code == api.RANGE_ERR, mu
            with pytest.raises(api.GrtError) as e:
                pipe.run_profiles(gcols)
            assert e.value.code == api.RANGE_ERR, mu
        pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_one_point_grids_are_refused(bands, lib, device):
    """No grid of fewer than two points reaches a solver: create_spectral_grid refuses wn <= w0, and the objects built on a
    grid refuse one of fewer than two points (a caller may fill the struct in itself)."""
    for w0, wn in ((500.0, 500.0), (500.0, 499.0)):
        with pytest.raises(api.GrtError) as e:
            api.create_spectral_grid(w0, wn, 1.0)
        assert e.value.code == api.RANGE_ERR
    lwb, swb = bands[2]
    for n in (0, 1):
        g = api.SpectralGrid()
        C.memmove(C.byref(g), C.byref(api.create_spectral_grid(lwb.w0, lwb.wn, lwb.dw)), C.sizeof(g))
        g.n = n
        with pytest.raises(api.GrtError) as e:
            api.GasOpticsObject(3, g, device, lwb.par)
        assert e.value.code == api.VALUE_ERR, n
        with pytest.raises(api.GrtError) as e:
            api.LongwaveObject(3, g, device)
        assert e.value.code == api.VALUE_ERR, n
        with pytest.raises(api.GrtError) as e:
            api.ShortwaveObject(3, g, device)
        assert e.value.code == api.VALUE_ERR, n
    # a gas-optics object whose grid was changed after it was made: the pipeline refuses it before anything is allocated
    emis, alb = surface(2, 1)
    solar = np.full(2, 0.5)
    for which in (0, 1):
        go_lw, _ = lwb.gas_optics(device, 3)
        go_sw, _ = swb.gas_optics(device, 3)
        go = (go_lw, go_sw)[which]
        go.c.grid.n = 1
        try:
            with pytest.raises(api.GrtError) as e:
                api.Pipeline(go_lw, go_sw, 2, -1, emis, alb, solar, spectral=False)
            assert e.value.code == api.VALUE_ERR
        finally:
            go.c.grid.n = 2
        go_lw.destroy()
        go_sw.destroy()


# ---- the reference-shaped solvers ----------------------------------------------------------------------------------- #
@pytest.mark.parametrize("L", [1, 6, 7, 199, 200])
@pytest.mark.parametrize("n", [2, 65, 129, 257])
def test_spectral_solvers_at_edge_shapes(oracle, device, monkeypatch, L, n):
    rng = np.random.default_rng(9000 + 7 * L + n)
    lw_grid = api.create_spectral_grid(300.0, 300.0 + (n - 1) * 1.0, 1.0)
    sw_grid = api.create_spectral_grid(2000.0, 2000.0 + (n - 1) * 10.0, 10.0)
    assert lw_grid.n == n and sw_grid.n == n
    col = syn.profile(60 + L, L + 1)
    tau, omega, g = random_optics(rng, L, n, True)
    tau[0, : max(n // 4, 1)] = 800.0                             # beyond the 700 clamp at any cos(zenith)
    emis, alb = surface(n, L)
    solar = rng.uniform(0.0, 1e-4, n)
    o_lw, o_sw = api.OpticsObject(L, lw_grid, device), api.OpticsObject(L, sw_grid, device)
    o_lw.update(tau, omega, g)
    o_sw.update(tau, omega, g)
    lw = api.LongwaveObject(L + 1, lw_grid, device)
    sw = api.ShortwaveObject(L + 1, sw_grid, device)
    mu = MU0[(L + n) % len(MU0)]
    up, dn = (x.copy() for x in lw.fluxes(o_lw, col["t_surf"], col["t_layer"], col["t"], emis))
    wu, wd = oracle.lw_fluxes(lw_grid.w0, lw_grid.dw, col["t_surf"], col["t_layer"], col["t"], tau, omega, emis)
    scale = max(np.abs(wu).max(), np.abs(wd).max())
    assert np.max(np.abs(up - wu)) <= 1e-12 * scale and np.max(np.abs(dn - wd)) <= 1e-12 * scale
    sup, sdn = (x.copy() for x in sw.fluxes(o_sw, mu, 0.5, alb, alb, 1360.0, solar))
    wu, wd = oracle.sw_fluxes(omega, g, tau, mu, 0.5, alb, alb, 1360.0, solar)
    scale = max(np.abs(wu).max(), np.abs(wd).max())
    assert scale > 0.0
    assert np.max(np.abs(sup - wu)) <= 1e-12 * scale and np.max(np.abs(sdn - wd)) <= 1e-12 * scale
    monkeypatch.setenv("GRT_LW_COLUMN_CHAINS", "1")
    monkeypatch.setenv("GRT_SW_COLUMN_CHAINS", "1")
    up1, dn1 = lw.fluxes(o_lw, col["t_surf"], col["t_layer"], col["t"], emis)
    assert np.array_equal(up, up1) and np.array_equal(dn, dn1)
    sup1, sdn1 = sw.fluxes(o_sw, mu, 0.5, alb, alb, 1360.0, solar)
    assert np.array_equal(sup, sup1) and np.array_equal(sdn, sdn1)
    for x in (lw, sw, o_lw, o_sw):
        x.destroy()


# ---- the spectral tables the shortwave solver adds -------------------------------------------------------------------- #
NCFC = 21


def table_band(root, with_ctm, with_tables):
    """600-1500 cm-1 at 1 cm-1 (n = 901, odd: every other table row starts off 16-byte alignment), no lines: tau is the
    tables.  with_tables: the ozone continuum, 21 CFCs over 700-1300 cm-1 (spans that start and end inside blocks) and the
    three CIA pairs."""
    return Band(root, 600.0, 1500.0, 1.0, 0, sw=True, with_ctm=with_ctm, with_cfc=with_tables, with_cia=with_tables)


def table_gas_optics(band, device, V, with_tables):
    grid = api.create_spectral_grid(band.w0, band.wn, band.dw)
    go = api.GasOpticsObject(V, grid, device, band.par, band.h2o_dir if band.with_ctm else None,
                             band.files["o3_ctm"] if with_tables else None)
    for m in band.mols:
        go.add_molecule_lines(m, band.lines[m])
    if with_tables:
        for k in range(NCFC):
            go.add_cfc(k, band.files["cfc11" if k % 2 == 0 else "cfc12"])
        for a, b, name in (((0, 0, "cia_n2n2"), (1, 0, "cia_o2n2"), (1, 1, "cia_o2o2"))):
            go.add_cia(a, b, band.files[name])
    go.tune(fast=0)
    return go, grid


@pytest.mark.parametrize("kind", ["all_tables", "h2o_only", "none"])
def test_tables_added_by_the_shortwave_solver(tmp_path, oracle, lib, device, monkeypatch, kind):
    with_ctm, with_tables = kind != "none", kind == "all_tables"
    band = table_band(str(tmp_path), with_ctm, with_tables)
    assert band.nw == 901
    V = 9
    cols = columns(V)[:3]
    for c, col in enumerate(cols):                               # 21 species, distinct abundances
        col["cfc_ppmv"] = {k: np.full(V, 1.0e-4 * (1 + k + c)) for k in range(NCFC)}
    go, grid = table_gas_optics(band, device, V, with_tables)
    _, alb = surface(band.nw, 3)
    solar = api.create_solar_flux(grid, band.files["solar"])
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=tuple(range(NCFC)) if with_tables else ())
    api.check(lib.grt_set_deterministic(1))
    try:
        flux, tau = {}, {}
        for defer in ("1", "0"):
            monkeypatch.setenv("GRT_DEFER_CONTINUA", defer)
            pipe = api.Pipeline(None, go, len(cols), 3, None, alb, solar, spectral=False)
            junk = np.full((len(cols), api.GRT_FLUXES_PER_COLUMN), 123.5)    # what the caller's buffer held before
            api.check(lib.grt_host_to_device(device, pipe.out.ptr, junk.ctypes.data_as(C.c_void_p), junk.nbytes))
            pipe.run(gcols)
            flux[defer] = pipe.fluxes(len(cols))
            assert np.all(flux[defer][:, :6] == 0.0)                          # no longwave band: its six are zeros
            tau[defer] = api.device_to_host(device, pipe.views(1)["tau_gas"], (len(cols), V - 1, band.nw)).copy()
            pipe.destroy()
        monkeypatch.delenv("GRT_DEFER_CONTINUA")
        assert np.array_equal(flux["1"], flux["0"])
        assert np.array_equal(tau["1"], tau["0"])
        assert np.all(flux["1"][:, 6:] != 0.0)
        for c, col in enumerate(cols):
            for m in band.mols:
                go.set_molecule_ppmv(m, col["ppmv"][m])
            if with_tables:
                for k in range(NCFC):
                    go.set_cfc_ppmv(k, col["cfc_ppmv"][k])
                go.set_cia_ppmv(0, col["ppmv"][syn.N2])
                go.set_cia_ppmv(1, col["ppmv"][syn.O2])
            opt = api.OpticsObject(V - 1, grid, device)
            go.calculate_optical_depth(col["p"], col["t"], opt)
            direct = opt.read()[0]
            opt.destroy()
            assert np.array_equal(direct, tau["1"][c])
            kw = band.oracle_inputs(oracle, lib, col)
            if not with_tables:                                  # the water-vapour continuum alone
                kw.pop("o3_xs", None)
                for m in kw["mols"]:
                    m["o3_ctm"] = 0
            if with_tables:
                kw["cfcs"] = [(col["cfc_ppmv"][k] * 1e-6, band.table_on_grid(oracle, "cfc11" if k % 2 == 0 else "cfc12"))
                              for k in range(NCFC)]
            want = oracle.gas_optics(col["p"], col["t"], band.w0, band.dw, band.nw, **kw)
            got = tau["1"][c]
            if kind == "none":
                assert np.all(got == 0.0) and np.all(want == 0.0)
                continue
            assert np.all(want > 0.0)
            layer_max = np.abs(want).max(axis=1, keepdims=True)
            assert np.max(np.abs(got - want) / layer_max) <= 1e-11
            assert np.max(np.abs(got - want) / np.abs(want)) <= 1e-11   # pointwise: where one CFC is a small part of tau
    finally:
        api.check(lib.grt_set_deterministic(-1))
    go.destroy()
