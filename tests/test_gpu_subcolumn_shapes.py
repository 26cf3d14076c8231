"""grt_pipeline_run_subcolumns at the shapes where its indexing goes wrong: one- and two-layer columns, the level counts
around the sweeps' six-layer chunk up to MAX_NUM_LEVELS, grids of two points up to one live lane past two solver blocks,
1 to GRT_MAX_SUBCOLUMNS subcolumns, the user level at and next to both ends; batches whose subcolumns the host splits into
several launches (the 65 535-row cap and the shortwave park block, remainder launches included); buffers that regrow
and are reused across calls of other shapes; pipelines of one band.  Against the oracle (the mean spectra of the
materialised form point by point), and in the deterministic mode's exact identities: the mean is the left fold of the
single-subcolumn entry points' results divided by S, bit for bit."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api, synthetic as syn
from pipeline_support import (CP, GRAVITY, KEYS, LEVEL_KEYS, LEVEL_TOL, SETS, SOLVER_NS as NS, _deterministic,
                              _sentinel, assert_trapezoid, columns, heating, limits, make, oracle_subcolumns, pick, six,
                              subcolumn_clouds, surface, user_index)
from pipeline_support import solver_bands as bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

ROW_CAP = 65535                     # grid rows of one subcolumn launch

# ---- A: the Latin square.  Per (layout, form), one case per grid length; every level count, subcolumn count and user
# level appears with every layout and form.  201 levels only on grids of 65 points or fewer and with S <= 7; S of 63 and
# 64 only with V <= 8 (the oracle's share of the run time).
FORMS = (("six", False), ("six", True), ("profile", False), ("profile", True))
VS = {FORMS[0]: (201, 2, 3, 7, 8, 2, 3), FORMS[1]: (2, 201, 7, 8, 3, 7, 8),
      FORMS[2]: (3, 7, 201, 2, 8, 3, 2), FORMS[3]: (7, 8, 2, 201, 3, 8, 7)}
SS = {FORMS[0]: (7, 64, 1, 2, 63, 3, 64), FORMS[1]: (3, 2, 64, 63, 7, 1, 2),
      FORMS[2]: (64, 7, 3, 1, 2, 63, 64), FORMS[3]: (2, 63, 7, 3, 64, 1, 7)}
ULS = {FORMS[0]: ("-1", "0", "1", "L-1", "L", "0", "L"), FORMS[1]: ("0", "1", "L-1", "L", "-1", "1", "L-1"),
       FORMS[2]: ("1", "L-1", "L", "-1", "0", "L", "-1"), FORMS[3]: ("L-1", "L", "-1", "0", "1", "-1", "0")}
CASES = [(f[0], f[1], VS[f][k], n, SS[f][k], ULS[f][k]) for f in FORMS for k, n in enumerate(NS)]
assert all(set(VS[f]) == {2, 3, 7, 8, 201} and set(SS[f]) == {1, 2, 3, 7, 63, 64} and
           set(ULS[f]) == {"-1", "0", "1", "L-1", "L"} for f in FORMS)
assert all(n <= 65 and S <= 7 for _, _, V, n, S, _ in CASES if V == 201)
assert all(V <= 8 for _, _, V, _, S, _ in CASES if S >= 63)


def drawn_clouds(cols, S, seed, B=6):
    """Band tables [ncol][S][3][B][L] of make_clouds drawn directly: per (column, layer) clear, overcast or partly cloudy
    (there each draw is cloudy with probability 1/2), every fourth subcolumn clear throughout, extinctions over six decades
    up to 1 m-1 (tau/mu0 past the 700 clamp in thick layers), albedo and asymmetry where there is cloud."""
    ncol, L = len(cols), cols[0]["p"].size - 1
    rng = np.random.default_rng(seed)
    state = rng.integers(0, 3, (ncol, L))              # 0 clear, 1 overcast, 2 partly cloudy
    state[:, 0] = np.arange(ncol) % 3                  # each kind in every batch of three columns or more
    if L > 1:
        state[:, 1] = (np.arange(ncol) + 1) % 3        # (no column of two or more layers clear throughout)
    clear_sub = (np.arange(S)[None, :] + np.arange(ncol)[:, None]) % 4 == 3
    out = {"thickness": np.array([29.3 * c["t_layer"] * np.log(c["p"][1:] / c["p"][:-1]) for c in cols])}
    for k in SETS:
        cloudy = (state[:, None, :] == 1) | ((state[:, None, :] == 2) & (rng.random((ncol, S, L)) < 0.5))
        cloudy &= ~clear_sub[:, :, None]
        m = cloudy[:, :, None, :]
        ext = np.where(m, 10.0 ** rng.uniform(-6.0, 0.0, (ncol, S, B, L)), 0.0)
        alb = np.where(m, rng.uniform(0.0, 0.9999, (ncol, S, B, L)), 0.0)
        asy = np.where(m, rng.uniform(0.0, 0.95, (ncol, S, B, L)), 0.0)
        out[k] = np.ascontiguousarray(np.stack([ext, alb, asy], axis=2))
    return out


def case_clouds(cols, tables, seed, S):
    L = cols[0]["p"].size - 1
    if L >= 6 and S <= 7:
        return subcolumn_clouds(cols, tables, seed, S)
    return drawn_clouds(cols, S, seed)


def one_draw(cl, j):
    """Subcolumn j of every column as [ncol][3][B][L] sets: the single-subcolumn entry points' input."""
    return {k: (np.ascontiguousarray(v[:, j]) if k in SETS else v) for k, v in cl.items()}


def as_sets(out, profile):
    """(clear, all-sky) as dicts: the six-row layout's rows under "fluxes", the profile layout's under KEYS."""
    if profile:
        return out
    return {"fluxes": out[0]}, {"fluxes": out[1]}


def run_subcolumns(pipe, gcols, gcl, S, profile, ncol):
    pipe.run_subcolumns(gcols, gcl, S, profiles=profile)
    return as_sets(pipe.subcolumn_profiles(ncol) if profile else pipe.subcolumn_fluxes(ncol), profile)


def run_allsky(pipe, gcols, gcl, profile, ncol):
    if profile:
        pipe.run_allsky_profiles(gcols, gcl)
        return pipe.allsky_profiles(ncol)
    pipe.run_allsky(gcols, gcl)
    return as_sets(pipe.allsky_fluxes(ncol), False)


def run_clear(pipe, gcols, profile, ncol):
    if profile:
        pipe.run_profiles(gcols)
        return pipe.profiles(ncol)
    pipe.run(gcols)
    return {"fluxes": pipe.fluxes(ncol)}


def spectra(pipe, device, ncol):
    """The materialised form's spectral fluxes after the last run (read after its outputs): per band (up, down)
    [ncol][V][nw]."""
    V = pipe.num_levels
    out = []
    for bi, nw in enumerate(pipe.nw):
        v = pipe.views(bi)
        out.append(tuple(api.device_to_host(device, v[k], (ncol, V, nw)).copy() for k in ("flux_up", "flux_down")))
    return out


def fold_mean(xs):
    """(((x_0 + x_1) + x_2) + ... + x_{S-1}) / S in doubles: subcolumn_mean_kernel's and flux_mean_kernel's order."""
    acc = xs[0].copy()
    for x in xs[1:]:
        acc = acc + x
    return acc / float(len(xs))


def identities(pipe, device, tables, gcols, cl, S, profile, ncol, make_fn=make):
    """B, in the deterministic mode: fused form, run_subcolumns(S) is the left fold of run_allsky (run_allsky_profiles)
    on each subcolumn alone, divided by S (six-row layout: the six rows; profile layout: the level rows); materialised
    form, its mean spectra are the same fold of the per-subcolumn spectra; its clear-sky set is run's (run_profiles').
    -> the run_subcolumns result (clear, all-sky) and, materialised form, its spectra."""
    xs, specs = [], []
    for j in range(S):
        g, k = make_fn(tables, one_draw(cl, j))
        xs.append(run_allsky(pipe, gcols, g, profile, ncol)[1])
        if pipe.keep_spectra:
            specs.append(spectra(pipe, device, ncol))
    g, k = make_fn(tables, cl)
    got = run_subcolumns(pipe, gcols, g, S, profile, ncol)
    got_spec = spectra(pipe, device, ncol) if pipe.keep_spectra else None
    if not pipe.keep_spectra:
        # fused form: subcolumn_mean_kernel folds the subcolumns' integrals (the materialised form integrates the mean
        # spectrum instead: check_trapezoids)
        for key in (LEVEL_KEYS if profile else ("fluxes",)):
            assert np.array_equal(got[1][key], fold_mean([x[key] for x in xs])), key
    else:
        for bi in range(2):
            for r in range(2):
                assert np.array_equal(got_spec[bi][r], fold_mean([sp[bi][r] for sp in specs])), (bi, r)
    clear = run_clear(pipe, gcols, profile, ncol)
    for key in (KEYS if profile else ("fluxes",)):
        assert np.array_equal(got[0][key], clear[key]), key
    return got, got_spec


def check_levels_are_six(got, L, user_level):
    """Profile layout: each set's six rows are its level rows at 0, L and the user level, bit for bit."""
    for s in range(2):
        f = got[s]["fluxes"]
        for bi, key in enumerate(("lw", "sw")):
            up, dn = got[s][key + "_up"], got[s][key + "_down"]
            assert np.array_equal(f[:, 6 * bi], up[:, 0]) and np.array_equal(f[:, 6 * bi + 1], up[:, L]), (s, key)
            assert np.array_equal(f[:, 6 * bi + 3], dn[:, 0]) and np.array_equal(f[:, 6 * bi + 4], dn[:, L]), (s, key)
            if user_level >= 0:
                assert np.array_equal(f[:, 6 * bi + 2], up[:, user_level]), (s, key)
                assert np.array_equal(f[:, 6 * bi + 5], dn[:, user_level]), (s, key)
            else:
                assert np.all(f[:, [6 * bi + 2, 6 * bi + 5]] == 0.0)


def check_trapezoids(got, spec, bands_, profile, L, user_level):
    """Materialised form: every integrated all-sky row is the exactly rounded trapezoid of the mean spectrum, to
    TRAP_ULPS."""
    ncol = spec[0][0].shape[0]
    for bi, (band, key) in enumerate(zip(bands_, ("lw", "sw"))):
        up_s, dn_s = spec[bi]
        for c in range(ncol):
            f = got[1]["fluxes"][c, 6 * bi: 6 * bi + 6]
            for r, (rows, lev) in enumerate(((up_s, 0), (up_s, L), (up_s, user_level),
                                             (dn_s, 0), (dn_s, L), (dn_s, user_level))):
                if lev >= 0:
                    assert_trapezoid(f[r], rows[c, lev], band.dw, (key, c, r))
            if profile:
                for k in range(L + 1):
                    assert_trapezoid(got[1][key + "_up"][c, k], up_s[c, k], band.dw, (key, c, "up", k))
                    assert_trapezoid(got[1][key + "_down"][c, k], dn_s[c, k], band.dw, (key, c, "down", k))


def check_oracle(oracle, lib, tables, bands_, cols, cl, got, spec, which, profile, user_level, emis, alb, solar):
    """Columns `which` of the all-sky set of got (and of spec, materialised form) against the oracle's subcolumn mean:
    within LEVEL_TOL of the column's largest flux, heating rates within test_pipeline_at_edge_shapes' bound."""
    for bi, (band, lw, key) in enumerate(zip(bands_, (True, False), ("lw", "sw"))):
        for c in which:
            col = cols[c]
            w = oracle_subcolumns(oracle, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
                                  cl["thickness"][c], emis, alb, solar)
            ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
            assert ff > 0.0
            f = got[1]["fluxes"][c, 6 * bi: 6 * bi + 6]
            assert np.max(np.abs(f - six(w["up_int"], w["dn_int"], user_level))) <= LEVEL_TOL * ff, (key, c)
            if user_level < 0:
                assert f[2] == 0.0 and f[5] == 0.0
            if spec is not None:
                fs = max(np.abs(w["up"]).max(), np.abs(w["dn"]).max())
                assert np.max(np.abs(spec[bi][0][c] - w["up"])) <= LEVEL_TOL * fs, (key, c)
                assert np.max(np.abs(spec[bi][1][c] - w["dn"])) <= LEVEL_TOL * fs, (key, c)
            if not profile:
                continue
            up, dn, hr = got[1][key + "_up"][c], got[1][key + "_down"][c], got[1][key + "_heating"][c]
            assert np.max(np.abs(up - w["up_int"])) <= LEVEL_TOL * ff, (key, c)
            assert np.max(np.abs(dn - w["dn_int"])) <= LEVEL_TOL * ff, (key, c)
            mass = 100.0 * (col["p"][1:] - col["p"][:-1]) / GRAVITY
            bound = 4.0 * LEVEL_TOL * ff / (CP * mass) * 86400.0
            want_hr = heating(w["up_int"], w["dn_int"], col["p"])
            assert np.all(np.abs(hr - want_hr) <= bound + 1e-12 * np.abs(want_hr).max()), (key, c)


def check_sweeps(one, two, user_level):
    """Six-row layout, the shortwave's one sweep (`one`) against its two (`two`), in both sets: longwave, surface and
    top-down rows the same doubles, top-up to rounding (test_pipeline_at_edge_shapes' rule)."""
    for s in range(2):
        a, b = one[s]["fluxes"], two[s]["fluxes"]
        assert np.array_equal(a[:, :6], b[:, :6])
        exact = [7, 9, 10, 11] + ([8] if user_level != 0 else [])
        assert np.array_equal(a[:, exact], b[:, exact])
        top_up = [6] + ([8] if user_level == 0 else [])
        assert np.max(np.abs(a[:, top_up] - b[:, top_up])) <= 1e-13 * np.abs(b[:, 6:]).max()


def gas(bands_, device, V):
    lwb, swb = bands_
    go_lw, _ = lwb.gas_optics(device, V)
    go_sw, grid_sw = swb.gas_optics(device, V)
    return go_lw, go_sw, api.create_solar_flux(grid_sw, swb.files["solar"])


# ---- A and B at edge shapes ------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("layout,spectral,V,n,S,ul", CASES,
                         ids=[f"{lay}-{'mat' if sp else 'fused'}-V{V}-n{n}-S{S}-ul{u}" for lay, sp, V, n, S, u in CASES])
def test_subcolumns_at_edge_shapes(bands, tables, oracle, lib, device, monkeypatch, layout, spectral, V, n, S, ul):
    L = V - 1
    user_level = user_index(ul, L)
    profile = layout == "profile"
    bands_ = bands[n]
    cols = columns(V)
    ncol = len(cols)
    go_lw, go_sw, solar = gas(bands_, device, V)
    emis, _ = surface(n, 1 + n)
    _, alb = surface(n, 2 + n)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case_clouds(cols, tables, 40 + V + S, S)
    gcl, keep_cl = make(tables, cl)
    assert keep_cl["subcolumns"] == S
    pipe = api.Pipeline(go_lw, go_sw, ncol, user_level, emis, alb, solar, spectral=spectral)

    # ---- A: the default mode against the oracle --------------------------------------------------------------------- #
    got = run_subcolumns(pipe, gcols, gcl, S, profile, ncol)
    spec = spectra(pipe, device, ncol) if spectral else None
    check_oracle(oracle, lib, tables, bands_, cols, cl, got, spec, range(ncol), profile, user_level, emis, alb, solar)
    if profile:
        check_levels_are_six(got, L, user_level)

    # ---- B: the deterministic mode's identities ---------------------------------------------------------------------- #
    _deterministic(lib, True)
    try:
        det, det_spec = identities(pipe, device, tables, gcols, cl, S, profile, ncol)
        if spectral:
            check_trapezoids(det, det_spec, bands_, profile, L, user_level)
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        two = run_subcolumns(pipe, gcols, gcl, S, False, ncol)
        if profile:
            check_levels_are_six(det, L, user_level)
            # the six-row layout (two sweeps) is the profile layout's level rows at 0, L and the user level
            for s in range(2):
                for bi, key in enumerate(("lw", "sw")):
                    f, up, dn = two[s]["fluxes"][:, 6 * bi: 6 * bi + 6], det[s][key + "_up"], det[s][key + "_down"]
                    assert np.array_equal(f[:, 0], up[:, 0]) and np.array_equal(f[:, 1], up[:, L]), (s, key)
                    assert np.array_equal(f[:, 3], dn[:, 0]) and np.array_equal(f[:, 4], dn[:, L]), (s, key)
                    if user_level >= 0:
                        assert np.array_equal(f[:, 2], up[:, user_level]), (s, key)
                        assert np.array_equal(f[:, 5], dn[:, user_level]), (s, key)
        elif spectral or user_level not in (-1, 0, L):
            # the materialised form has no sweep choice; a user level inside the column takes the two sweeps either way
            assert all(np.array_equal(det[s]["fluxes"], two[s]["fluxes"]) for s in range(2))
        else:
            check_sweeps(det, two, user_level)
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- C: launch splits ------------------------------------------------------------------------------------------------ #
def launches(max_columns, ncol, S, park):
    """band_solve_subcolumns' split of S subcolumns of ncol columns into launches, restated: at most 65 535 grid rows per
    launch or -- where the shortwave parks -- at most max_columns parked columns; the last launch takes the remainder.
    -> [(first, count)]"""
    group = min(max_columns // ncol if park else ROW_CAP // ncol, S)
    return [(f, min(group, S - f)) for f in range(0, S, group)]


def parks(profile, user_level, V):
    """Whether the shortwave pass parks (GRT_SW_TWO_SWEEPS unset): always in the profile layout, and in the six-row
    layout for a user level inside the column (grt_sw_one_sweep)."""
    return profile or not (user_level < 0 or user_level == 0 or user_level == V - 1)


# max_columns, ncol, S, V, n, user level, counts per launch: longwave, shortwave six-row, shortwave profile
SPLITS = [
    (1285, 1285, 64, 2, 65, -1, [51, 13], [51, 13], [1] * 64),       # the first launch: 51 x 1285 = 65 535 rows
    (1285, 1025, 64, 3, 2, -1, [63, 1], [63, 1], [1] * 64),
    (1285, 1100, 64, 2, 2, -1, [59, 5], [59, 5], [1] * 64),
    (7, 3, 7, 3, 65, 1, [7], [2, 2, 2, 1], [2, 2, 2, 1]),
    (7, 2, 64, 3, 2, 1, [64], [3] * 21 + [1], [3] * 21 + [1]),
    (7, 1, 64, 3, 65, 1, [64], [7] * 9 + [1], [7] * 9 + [1]),
    (7, 7, 5, 3, 2, 1, [5], [1] * 5, [1] * 5),
]


def split_columns(ncol, V):
    """Distinct columns: profiles of their own seeds, surface temperature and cos(zenith) varied per column (mu0 from 1
    down to 1e-3)."""
    cols = [syn.profile(900 + c, V) for c in range(ncol)]
    for c, col in enumerate(cols):
        col["t_surf"] = col["t_surf"] + 0.037 * (c % 311) - 5.0
        col["mu0"] = 10.0 ** (-3.0 * ((c * 0.6180339887) % 1.0))
    return cols


@pytest.mark.parametrize("max_columns,ncol,S,V,n,ul,lw_counts,sw_six,sw_profile", SPLITS,
                         ids=[f"max{m}-C{c}-S{s}" for m, c, s, *_ in SPLITS])
@pytest.mark.parametrize("profile", [False, True], ids=["six", "profile"])
def test_launch_splits(bands, tables, oracle, lib, device, profile, max_columns, ncol, S, V, n, ul, lw_counts, sw_six,
                       sw_profile):
    L = V - 1
    assert [c for _, c in launches(max_columns, ncol, S, False)] == lw_counts
    assert [c for _, c in launches(max_columns, ncol, S, parks(False, ul, V))] == sw_six
    assert [c for _, c in launches(max_columns, ncol, S, parks(True, ul, V))] == sw_profile
    bands_ = bands[n]
    cols = split_columns(ncol, V)
    go_lw, go_sw, solar = gas(bands_, device, V)
    emis, _ = surface(n, 3 + n)
    _, alb = surface(n, 4 + n)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = drawn_clouds(cols, S, 70 + ncol)
    mu = np.array([c["mu0"] for c in cols])
    tau = cl["sw_liquid"][:, :, 0] * cl["thickness"][:, None, None, :]
    assert np.any(tau / mu[:, None, None, None] > 700.0)            # some direct beams clamped
    assert np.any(tau.max(axis=(2, 3)) == 0.0)                      # some subcolumns clear throughout
    pipe = api.Pipeline(go_lw, go_sw, max_columns, ul, emis, alb, solar, spectral=False)
    _deterministic(lib, True)
    try:
        got, _ = identities(pipe, device, tables, gcols, cl, S, profile, ncol)
        check_oracle(oracle, lib, tables, bands_, cols, cl, got, None, sorted({0, ncol // 2, ncol - 1}), profile, ul,
                     emis, alb, solar)
        if profile:
            check_levels_are_six(got, L, ul)
        # a column alone (every subcolumn in one launch or another split) is the same column inside the batch
        for k in sorted({0, ncol // 2, ncol - 1}):
            g1, keep1 = api.make_columns([cols[k]], MOL_ORDER, cfc_order=(0, 1))
            c1, kc1 = make(tables, pick(cl, columns=[k]))
            alone = run_subcolumns(pipe, g1, c1, S, profile, 1)
            for s in range(2):
                for key in got[s]:
                    assert np.array_equal(alone[s][key][0], got[s][key][k]), (k, s, key)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- D: buffer regrowth and reuse ------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "mat"])
def test_buffers_regrow_and_are_reused(bands, tables, lib, device, spectral):
    V, n, ul, M = 8, 65, 3, 7
    L = V - 1
    bands_ = bands[n]
    cols = split_columns(M, V)
    go_lw, go_sw, solar = gas(bands_, device, V)
    emis, _ = surface(n, 5)
    _, alb = surface(n, 6)
    cl = drawn_clouds(cols, 64, 81)
    # the same draws on the first four liquid bands: the staged tables shrink, the band map is rebuilt
    cl4 = {k: (np.ascontiguousarray(v[:, :, :, :4]) if k in SETS else v) for k, v in cl.items()}
    llo, lhi = limits(tables, "liquid")

    def make4(t, c):
        return api.make_clouds((llo[:4], lhi[:4]), limits(t, "ice"), c["thickness"], *[c[k] for k in SETS])

    def call(pipe, S, ncol, B, profile):
        gcols, keep = api.make_columns(cols[:ncol], MOL_ORDER, cfc_order=(0, 1))
        g, k = (make if B == 6 else make4)(tables, pick(cl if B == 6 else cl4, range(ncol), range(S)))
        out = run_subcolumns(pipe, gcols, g, S, profile, ncol)
        return out, (spectra(pipe, device, ncol) if spectral else None)

    # (S, ncol, liquid bands, profile layout): sub_partials and the staged tables grow (S = 64), stage_clouds regrows
    # (S = 7 at 7 columns), fewer bands, then the layouts alternate
    calls = [(2, 7, 6, False), (64, 1, 6, False), (7, 7, 6, False), (7, 7, 4, False), (7, 7, 4, True), (64, 1, 6, False),
             (2, 7, 6, True), (3, 5, 4, False), (64, 1, 4, True), (7, 7, 6, False)]
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    g1, k1 = make(tables, one_draw(cl, 5))
    pipe = api.Pipeline(go_lw, go_sw, M, ul, emis, alb, solar, spectral=spectral)
    _deterministic(lib, True)
    try:
        allsky0, run0 = run_allsky(pipe, gcols, g1, False, M), run_clear(pipe, gcols, False, M)
        for S, ncol, B, profile in calls:
            got, spec = call(pipe, S, ncol, B, profile)
            fresh = api.Pipeline(go_lw, go_sw, M, ul, emis, alb, solar, spectral=spectral)
            want, want_spec = call(fresh, S, ncol, B, profile)
            fresh.destroy()
            for s in range(2):
                for key in want[s]:
                    assert np.array_equal(got[s][key], want[s][key]), (S, ncol, B, profile, s, key)
            if spectral:
                for bi in range(2):
                    for r in range(2):
                        assert np.array_equal(spec[bi][r], want_spec[bi][r]), (S, ncol, B, profile, bi, r)
            if profile:
                check_levels_are_six(got, L, ul)
        # B's identities on the grown buffers
        g5, k5 = api.make_columns(cols[:5], MOL_ORDER, cfc_order=(0, 1))
        identities(pipe, device, tables, g5, pick(cl4, range(5), range(3)), 3, True, 5, make_fn=make4)
        allsky1, run1 = run_allsky(pipe, gcols, g1, False, M), run_clear(pipe, gcols, False, M)
        for s in range(2):
            assert np.array_equal(allsky1[s]["fluxes"], allsky0[s]["fluxes"]), s
        assert np.array_equal(run1["fluxes"], run0["fluxes"])
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- E: pipelines of one band ---------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("S", [2, 64])
@pytest.mark.parametrize("present", ["lw", "sw"])
@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "mat"])
def test_one_band_pipelines(bands, tables, lib, device, spectral, present, S):
    V, n, ul = 7, 129, 1
    L = V - 1
    bands_ = bands[n]
    cols = columns(V)
    ncol = len(cols)
    go_lw, go_sw, solar = gas(bands_, device, V)
    emis, _ = surface(n, 7)
    _, alb = surface(n, 8)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = drawn_clouds(cols, S, 90 + S)
    on, off = (0, 1) if present == "lw" else (1, 0)
    g1, k1 = api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), cl["thickness"],
                             *[cl[k] if k.startswith(present) else None for k in SETS])
    both = api.Pipeline(go_lw, go_sw, ncol, ul, emis, alb, solar, spectral=spectral)
    one = (api.Pipeline(go_lw, None, ncol, ul, emis, None, None, spectral=spectral) if present == "lw" else
           api.Pipeline(None, go_sw, ncol, ul, None, alb, solar, spectral=spectral))
    _deterministic(lib, True)
    try:
        for profile in (False, True):
            want, _ = identities(both, device, tables, gcols, cl, S, profile, ncol)
            sizes = (ncol * 2 * 4 * V, ncol * 2 * 2 * L, ncol * 24) if profile else (ncol * 24,)
            bufs = [_sentinel(device, m) for m in sizes]
            ptrs = [b.ptr for b in bufs] if profile else [None, None, bufs[0].ptr]
            api.check(lib.grt_pipeline_run_subcolumns(one.p, C.byref(gcols), C.byref(g1), S, *ptrs))
            one.sync()
            fx = bufs[-1].to_host((ncol, 2, 12))
            assert not np.any(fx == -7.25), profile
            for s in range(2):
                assert np.all(fx[:, s, 6 * off: 6 * off + 6] == 0.0), (profile, s)
                assert np.array_equal(fx[:, s, 6 * on: 6 * on + 6], want[s]["fluxes"][:, 6 * on: 6 * on + 6]), (profile, s)
            if profile:
                lv = bufs[0].to_host((ncol, 2, 4, V))
                hr = bufs[1].to_host((ncol, 2, 2, L))
                assert not np.any(lv == -7.25) and not np.any(hr == -7.25)
                for s in range(2):
                    assert np.all(lv[:, s, 2 * off: 2 * off + 2] == 0.0) and np.all(hr[:, s, off] == 0.0), s
                    assert np.array_equal(lv[:, s, 2 * on], want[s][present + "_up"]), s
                    assert np.array_equal(lv[:, s, 2 * on + 1], want[s][present + "_down"]), s
                    assert np.array_equal(hr[:, s, on], want[s][present + "_heating"]), s
            for b in bufs:
                b.free()
    finally:
        _deterministic(lib, False)
    both.destroy()
    one.destroy()
    go_lw.destroy()
    go_sw.destroy()
