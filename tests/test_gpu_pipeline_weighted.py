"""grt_pipeline_run_sky_weighted: grt_pipeline_run_sky's profile form with every level's rows under spectral responses, and
the actinic flux of the shortwave's, beside them.  Against response_model.py's restatement (held to the oracle on the CPU:
test_response_model.py), fused and materialised; the bit-for-bit identities with grt_pipeline_run_sky, _run_sky_direct and
within the new rows; edge shapes of the sink's lists, the staged weights and the pairs' partial sums; the production
arithmetic; missing bands; what the entry point refuses; and the older entry points before and after it on one pipeline."""
import ctypes as C

import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID, aerosol_fields
from grtcode_amd import api, synthetic as syn
from pipeline_support import (LEVEL_KEYS, LEVEL_TOL, SETS, TRAP_ULPS, _deterministic, _sentinel, _setup, cached, clouds_for, make,
                              make_shape_bands, pick, subcolumn_clouds)
from pipeline_support import bands, oracle_cache, tables  # noqa: F401  (module fixtures)
from response_model import MU_DIF, actinic, oracle_spectral_sets, weighted_set
from scenario import MOL_ORDER
from test_gpu_pipeline_direct import AEROSOL_SEED, CLOUD_SEED, UL1, V1, Case1, run_direct
from test_gpu_pipeline_sky import (ALL, AEROSOL, BANDS, BOTH, CLEAN, CLOUD, NAMES, aerosols_of, fields, positions, run_sky,
                                   same, shape_grid, sky_columns)

pytestmark = pytest.mark.gpu

WEIGHTED_KEYS = {"lw": ("lw_up", "lw_down"), "sw": ("sw_up", "sw_down", "sw_direct", "sw_actinic")}
MODEL_KEYS = {"lw_up": "up", "lw_down": "dn", "sw_up": "up", "sw_down": "dn", "sw_direct": "direct", "sw_actinic": "actinic"}


@pytest.fixture(scope="module")
def case1(tables):
    return Case1(tables)


def run_weighted(pipe, gcols, gclouds, gaer, S, sets, ncol, lw, sw):
    """-> (run_sky's profile dict, sky_weighted's dict), every array [ncol][nsets][..]."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    gresp, keep_resp = api.make_responses(lw=lw, sw=sw)
    pipe.run_sky_weighted(gcols, gsky, gresp)
    return pipe.sky_profiles(ncol, keep["nsets"]), pipe.sky_weighted(ncol, keep["nsets"])


def five_responses(n, seed):
    """All ones on the whole grid, a Gaussian, a box across a block edge, a single point, random weights of both signs."""
    rng = np.random.default_rng(seed)
    x = np.arange(-45, 46)
    return ([0, n // 2 - 45, 120, 200, 250],
            [np.ones(n), 3.0 * np.exp(-0.5 * (x / 15.0) ** 2), np.ones(16), np.array([0.7]), rng.uniform(-1.0, 2.0, 77)])


def oracle_of(cache, orc, lib, bands, tables, case, surface, S):
    """[band][column] -> the four sets' level spectra, each computed once per module."""
    emis, alb, solar = surface
    cl = case.clouds(S)
    return [[cached(cache, ("spectra", key, c, S), lambda: oracle_spectral_sets(
        orc, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c], cl["thickness"][c], AEROSOL_GRID,
        case.f[bi][c], emis, alb, solar)) for c, col in enumerate(case.cols)]
        for bi, (band, (key, lw)) in enumerate(zip(bands, BANDS))]


def check_against_model(wt, c, k, key, band, col, spectra, resp, rel_tol, abs_tol, what):
    """Set k of column c of band `key` against the restatement on the oracle's spectra: per response within rel_tol x
    max|r| x ff + abs_tol x max|r| -- ff the set's largest level flux of the band --, the actinic rows within that x (1/mu0 +
    3/mu_dif), the error of three rows through the formula."""
    first, weights = resp
    want = weighted_set(spectra, band.dw, first, weights, col["mu0"])
    ones = weighted_set({q: spectra[q] for q in ("up", "dn")}, band.dw, [0], [np.ones(band.nw)])
    ff = max(np.abs(ones["up"]).max(), np.abs(ones["dn"]).max())
    assert ff > 0.0
    for name in WEIGHTED_KEYS[key]:
        for j, r in enumerate(weights):
            tol = (rel_tol * ff + abs_tol) * np.abs(r).max()
            if name == "sw_actinic":
                tol *= 1.0 / col["mu0"] + 3.0 / MU_DIF
            err = np.max(np.abs(wt[name][c, k, j] - want[MODEL_KEYS[name]][j]))
            print(what, name, "column", c, "set", k, "response", j, err, "of", tol)
            assert err <= tol, (what, name, c, k, j, err, tol)
    return want


# ---- (a) against the restatement ------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_weighted_rows_match_the_restatement(bands, tables, oracle, oracle_cache, case1, lib, device, S, spectral):
    cols, ncol = case1.cols, case1.ncol
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    resp = [five_responses(b.nw, 5 + bi) for bi, b in enumerate(bands)]
    spectra = oracle_of(oracle_cache, oracle, lib, bands, tables, case1, (emis, alb, solar), S)
    # on the oracle's numbers, so that the test can fail: under cloud some response's beam at the surface is well below
    # its downward flux, and two responses differ at the surface
    ratios = []
    for c, col in enumerate(cols):
        w = weighted_set(spectra[1][c][2], bands[1].dw, *resp[1], col["mu0"])
        ratios.append(w["direct"][:4, -1] / w["dn"][:4, -1])             # (the responses without negative weights)
        assert abs(w["dn"][1, -1] - w["dn"][2, -1]) > 1e-3 * abs(w["dn"][1, -1])
    print("cloud set, weighted direct / down at the surface:", ratios)
    assert np.min(ratios) < 0.9, ratios
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, keep_clouds = make(tables, case1.clouds(S))
    gaer, keep_aer = aerosols_of(case1.f)
    prof, wt = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, resp[0], resp[1])
    assert wt["lw_up"].shape == (ncol, 4, 5, V1) and wt["sw_actinic"].shape == (ncol, 4, 5, V1)
    for bi, (band, (key, lw)) in enumerate(zip(bands, BANDS)):
        for c, col in enumerate(cols):
            for k in range(4):
                check_against_model(wt, c, k, key, band, col, spectra[bi][c][k], resp[bi], LEVEL_TOL, 0.0,
                                    f"S={S} spectral={spectral}")
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (b) identities ------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_identities_bit_for_bit(bands, tables, case1, lib, device, S, spectral):
    """Deterministic mode.  The materialised form's broadband rows come from another kernel (one workgroup per row, four
    waves) than its response rows (the fused solvers' association), as test_gpu_band_profiles.py says of its bins: there
    the all-ones response is held to the trapezoid bound both keep to their common spectra, twice TRAP_ULPS 2^-52 sum |f| dw
    <= that of the value itself, all fluxes being of one sign.  Every other identity is bit for bit in both forms."""
    cols, ncol = case1.cols, case1.ncol
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    gclouds, keep_clouds = make(tables, cl)
    gaer, keep_aer = aerosols_of(case1.f)
    gzero, keep_zero = aerosols_of(tuple(np.zeros_like(f) for f in case1.f))
    clear = clouds_for(cols, tables, CLOUD_SEED, clear=True)
    gclear, keep_clear = make(tables, {k: (np.repeat(v[:, None], 1, axis=1) if k in SETS else v) for k, v in clear.items()})
    lw, sw = (five_responses(b.nw, 5 + bi) for bi, b in enumerate(bands))
    mu0 = np.array([c["mu0"] for c in cols])[:, None, None, None]
    _deterministic(lib, True)
    try:
        prof, wt = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, lw, sw)
        # every output run_sky (profile form) writes is run_sky's
        assert same(prof, run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, True))
        # the all-ones response: the band's rows of level_fluxes_dev, and run_sky_direct's direct levels
        direct = run_direct(pipe, gcols, gclouds, gaer, S, ALL, ncol, True)
        for key, ref in [(key, prof[key]) for key in LEVEL_KEYS] + [("sw_direct", direct["direct_levels"])]:
            if not spectral:
                assert np.array_equal(wt[key][:, :, 0], ref), key
            else:
                assert np.all(np.abs(wt[key][:, :, 0] - ref) <= 2 * TRAP_ULPS * 2.0 ** -52 * np.abs(ref)), key
        # the actinic rows are the formula, in its order, on the three returned rows; at the top the beam is the downward flux
        assert np.array_equal(wt["sw_actinic"], actinic(wt["sw_direct"], wt["sw_down"], wt["sw_up"], mu0))
        assert np.array_equal(wt["sw_down"][..., 0], wt["sw_direct"][..., 0])
        assert np.all(wt["sw_actinic"][:, :, 0] > 0.0)
        # the four sets' rows differ
        assert len({wt["sw_down"][0, k, 1, -1].tobytes() for k in range(4)}) == 4

        def only(band_resp, j):
            return [band_resp[0][j]], [band_resp[1][j]]

        # a response alone, duplicated, reordered among others, and without the other band's responses
        for j in (1, 2, 4):
            _, alone = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, only(lw, j), only(sw, j))
            for key in wt:
                assert np.array_equal(alone[key][:, :, 0], wt[key][:, :, j]), (key, j)
        order = [3, 1, 1, 4, 0, 2]
        _, mixed = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, ([lw[0][j] for j in order], [lw[1][j] for j in order]),
                                ([sw[0][j] for j in order[::-1]], [sw[1][j] for j in order[::-1]]))
        for key in wt:
            o = order if key.startswith("lw") else order[::-1]
            assert np.array_equal(mixed[key], wt[key][:, :, o]), key
        _, no_lw = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, None, sw)
        _, no_sw = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, lw, None)
        assert no_lw["lw_up"].shape == (ncol, 4, 0, V1) and no_sw["sw_actinic"].shape == (ncol, 4, 0, V1)
        for key in wt:
            assert np.array_equal((no_lw if key.startswith("sw") else no_sw)[key], wt[key]), key
        # 2 r gives exactly twice the rows, -r their negatives, weights of zero 0.0
        def scaled(band_resp, j):
            r = band_resp[1][j]
            return [band_resp[0][j]] * 3, [2.0 * r, -r, np.zeros_like(r)]
        _, lin = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, scaled(lw, 4), scaled(sw, 4))
        for key in wt:
            assert np.array_equal(lin[key][:, :, 0], 2.0 * wt[key][:, :, 4]), key
            assert np.array_equal(lin[key][:, :, 1], -wt[key][:, :, 4]), key
            assert np.all(lin[key][:, :, 2] == 0.0), key
        # a column alone, and the batch in reversed order
        def run_columns(order):
            g, k = api.make_columns([cols[c] for c in order], MOL_ORDER, cfc_order=(0, 1))
            gc, kc = make(tables, pick(cl, columns=order))
            ga, ka = aerosols_of(tuple(np.ascontiguousarray(f[list(order)]) for f in case1.f))
            return run_weighted(pipe, g, gc, ga, S, ALL, len(order), lw, sw)[1]
        rev = run_columns([2, 1, 0])
        one = run_columns([1])
        for key in wt:
            assert np.array_equal(rev[key], wt[key][::-1]), key
            assert np.array_equal(one[key][0], wt[key][1]), key
        # any subset of the four sets has its rows of the full call
        for mask in range(16):
            _, sub = run_weighted(pipe, gcols, gclouds if mask & (CLOUD | BOTH) else None,
                                  gaer if mask & (AEROSOL | BOTH) else None, S, mask, ncol, lw, sw)
            where = positions(mask)
            for name, k in where.items():
                for key in wt:
                    assert sub[key].shape[1] == len(where)
                    assert np.array_equal(sub[key][:, k], wt[key][:, NAMES.index(name)]), (mask, name, key)
        # an aerosol of zeros: the aerosol sets' rows are the clean and the cloud sets'
        _, z = run_weighted(pipe, gcols, gclouds, gzero, S, ALL, ncol, lw, sw)
        for key in wt:
            assert np.array_equal(z[key][:, 1], z[key][:, 0]) and np.array_equal(z[key][:, 3], z[key][:, 2]), key
            assert np.array_equal(z[key][:, [0, 2]], wt[key][:, [0, 2]]), key
        # cloud-free tables (one draw): the cloud sets' rows are the clean and the aerosol sets'
        _, n = run_weighted(pipe, gcols, gclear, gaer, 1, ALL, ncol, lw, sw)
        for key in wt:
            assert np.array_equal(n[key][:, 2], n[key][:, 0]) and np.array_equal(n[key][:, 3], n[key][:, 1]), key
            assert np.array_equal(n[key][:, [0, 1]], wt[key][:, [0, 1]]), key
        if S == 1:
            # the draw given twice runs the subcolumn instances and the mean, and (x + x)/2 is x to the bit
            twice = {k: (np.repeat(v, 2, axis=1) if k in SETS else v) for k, v in cl.items()}
            gtwice, keep_twice = make(tables, twice)
            _, two = run_weighted(pipe, gcols, gtwice, gaer, 2, ALL, ncol, lw, sw)
            for key in wt:
                assert np.array_equal(two[key], wt[key]), key
        # not bitwise: boxes that partition the grid, each point in exactly one, add up to the all-ones response
        for band, key in zip(bands, ("lw", "sw")):
            cuts = [0, 1, 127, 128, 129, 300, band.nw - 1, band.nw]
            boxes = (cuts[:-1], [np.ones(b - a) for a, b in zip(cuts[:-1], cuts[1:])])
            _, parts = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, boxes if key == "lw" else None,
                                    boxes if key == "sw" else None)
            ff = max(np.abs(prof[key + "_up"]).max(), np.abs(prof[key + "_down"]).max())
            for name in WEIGHTED_KEYS[key][:-1] if key == "sw" else WEIGHTED_KEYS[key]:
                err = np.max(np.abs(parts[name].sum(axis=2) - wt[name][:, :, 0]))
                print(name, "partition of the grid against the all-ones response", err, "of", LEVEL_TOL * ff)
                assert err <= LEVEL_TOL * ff, (name, err)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (c) edge shapes ----------------------------------------------------------------------------------------------------- #
NS = (2, 127, 128, 129, 257)
# a reduced Latin square: every grid length twice, with level counts, subcolumn counts and batch sizes (1 and max_columns
# = 3) rotating; both forms of the pipeline in every case
SHAPES = [(2, 61, 3, 3), (127, 2, 1, 1), (128, 201, 1, 3), (129, 3, 3, 1), (257, 61, 1, 3), (127, 3, 3, 3), (129, 201, 3, 1),
          (2, 2, 1, 1), (257, 2, 3, 1), (128, 61, 3, 3)]
shape_bands = make_shape_bands(NS, 100.0, 2000.0)


def shape_responses(n, limit, seed):
    """Responses that start at 0, end at n - 1 (the dw/2 ends), are one point wide at 127 and at 128, span 127 .. 128 and
    overlap, wherever the grid has those points; then as many more inside block 0 as bring its list to exactly `limit`."""
    rng = np.random.default_rng(seed)
    spans = [(0, n)]                            # starts at 0, ends at n - 1, overlaps every other
    if n > 127:
        spans += [(127, 128)]
    if n > 128:
        spans += [(128, 129), (127, 129)]
    in_block0 = sum(1 for a, b in spans if a < 128)
    assert in_block0 <= limit, (in_block0, limit)
    if in_block0 + 2 <= limit:                  # (where the limit leaves room: the two end points alone)
        spans += [(0, 1), (n - 1, n)]
        in_block0 += 1 + (n <= 128)
    for j in range(limit - in_block0):          # (inside block 0, so that no other block holds more)
        a = int(rng.integers(0, min(n, 128)))
        spans.append((a, min(a + 1 + j % 5, n, 128)))
    held = [sum(1 for a, b in spans if a < 128 * (k + 1) and b > 128 * k) for k in range((n + 127) // 128)]
    assert max(held) == held[0] == limit, (held, limit)
    return [a for a, b in spans], [rng.uniform(-1.0, 2.0, b - a) for a, b in spans]


@pytest.mark.parametrize("n,V,S,ncol", SHAPES, ids=[f"n{n}-V{V}-S{S}-c{c}" for n, V, S, c in SHAPES])
def test_edge_shapes(shape_bands, tables, oracle, lib, device, n, V, S, ncol):
    L = V - 1
    lwb, swb = shape_bands[n]
    cols = [syn.profile(900 + V + c, V) for c in range(3)]
    for c, mu in zip(cols, (1.0, 0.05, 1e-3)):                      # overhead sun, low sun, the sun on the horizon
        c["mu0"] = mu
    cols = cols[:ncol]
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
    pipes = {s: api.Pipeline(go_lw, go_sw, 3, -1, emis, alb, solar, spectral=s) for s in (False, True)}
    limits = [pipes[False].response_block_limit(bi) for bi in (0, 1)]
    G = (2, 3)
    assert limits == [(65536 - 16 * g * V) // (16 * g * V + 1024) for g in G] and limits == \
        [pipes[True].response_block_limit(bi) for bi in (0, 1)]
    resp = [shape_responses(n, min(limits[bi], api.GRT_MAX_RESPONSES - 12), 7 * n + V + bi) for bi in (0, 1)]
    got = {s: run_weighted(pipes[s], gcols, gclouds, gaer, S, ALL, ncol, resp[0], resp[1])[1] for s in (False, True)}
    for bi, (band, (key, lw)) in enumerate(zip((lwb, swb), BANDS)):
        assert api.response_pair_count(api.make_responses(**{key: resp[bi]})[0], bi, n) >= len(resp[bi][0])
        for c, col in enumerate(cols):
            spectra = oracle_spectral_sets(oracle, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
                                           cl["thickness"][c], xs[bi], f[bi][c], emis, alb, solar)
            for s in (False, True):
                for k in range(4):
                    check_against_model(got[s], c, k, key, band, col, spectra[k], resp[bi], LEVEL_TOL, 0.0, f"spectral={s}")
    for s in (False, True):
        pipes[s].destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (d) the production arithmetic --------------------------------------------------------------------------------------- #
def test_production_form_matches_the_restatement(bands, tables, oracle, lib, device):
    """fast = 3 on the 3 000-line bands: the weighted rows within the interface's flux contract, 1e-3 W m-2
    (test_gpu_pipeline_production.py), times the response's largest weight, of the restatement."""
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
    resp = [five_responses(b.nw, 5 + bi) for bi, b in enumerate(bands)]
    prof, wt = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, resp[0], resp[1])
    assert go_sw.last_launch()["fast"] == 3 and go_lw.last_launch()["fast"] == 3
    for bi, (band, (key, lw)) in enumerate(zip(bands, BANDS)):
        for c, col in enumerate(cols):
            spectra = oracle_spectral_sets(oracle, lib, band, col, lw, tables, cl[key + "_liquid"][c], cl[key + "_ice"][c],
                                           cl["thickness"][c], AEROSOL_GRID, f[bi][c], emis, alb, solar)
            for k in range(4):
                check_against_model(wt, c, k, key, band, col, spectra[k], resp[bi], 0.0, FLUX_TOL, "production")
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (e) missing bands --------------------------------------------------------------------------------------------------- #
def test_missing_bands(bands, tables, case1, lib, device):
    """A pipeline without a band: that band's rows of level_fluxes_dev are zeros -- written, not left --, it can carry no
    responses, and the other band's rows are the two-band pipeline's, bit for bit."""
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)
    lw, sw = (five_responses(b.nw, 5 + bi) for bi, b in enumerate(bands))
    _deterministic(lib, True)
    try:
        both = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
        full_prof, full = run_weighted(both, gcols, gclouds, gaer, S, ALL, ncol, lw, sw)
        both.destroy()
        lw_only = api.Pipeline(go_lw, None, ncol, UL1, emis, None, None, spectral=False)
        sw_only = api.Pipeline(None, go_sw, ncol, UL1, None, alb, solar, spectral=False)
        for pipe, mine, other, resp in ((lw_only, "lw", "sw", dict(lw=lw, sw=None)), (sw_only, "sw", "lw", dict(lw=None, sw=sw))):
            run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, resp["lw"], resp["sw"])      # (allocates the buffers)
            for name in ("sky_profiles.levels", "sky.weighted_levels"):
                fill = np.full(pipe.buffers[name].nbytes // 8, -7.25)
                api.check(lib.grt_host_to_device(device, pipe.buffers[name].ptr, fill.ctypes.data_as(C.c_void_p),
                                                 C.c_size_t(fill.nbytes)))
            prof, wt = run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, resp["lw"], resp["sw"])
            assert np.all(prof[other + "_up"] == 0.0) and np.all(prof[other + "_down"] == 0.0)
            assert np.array_equal(prof[mine + "_up"], full_prof[mine + "_up"])
            for key in WEIGHTED_KEYS[mine]:
                assert np.array_equal(wt[key], full[key]), key
            for key in WEIGHTED_KEYS[other]:
                assert wt[key].shape[2] == 0
            # responses for the band that is not there are refused
            gsky, ks = api.make_sky(gclouds, gaer, S, ALL)
            gresp, kr = api.make_responses(lw=lw, sw=sw)
            with pytest.raises(api.GrtError) as e:
                pipe.run_sky_weighted(gcols, gsky, gresp)
            assert e.value.code == api.VALUE_ERR
        lw_only.destroy()
        sw_only.destroy()
    finally:
        _deterministic(lib, False)
    go_lw.destroy()
    go_sw.destroy()


# ---- (f) refusals -------------------------------------------------------------------------------------------------------- #
def test_refused_inputs(bands, tables, case1, lib, device):
    cols, ncol, L, S = case1.cols, case1.ncol, V1 - 1, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    lw_only = api.Pipeline(go_lw, None, ncol, -1, emis, None, None, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    R = 48                                      # responses the sentinel buffers have room for
    sizes = (4 * 4 * V1 * (ncol + 1), 4 * 2 * L * (ncol + 1), 4 * 12 * (ncol + 1), 4 * 5 * R * V1 * (ncol + 1),
             4 * R * V1 * (ncol + 1))
    bufs = [_sentinel(device, n) for n in sizes]
    lv, hr, fx, wl, al = (b.ptr for b in bufs)
    tags = (api.TAG_GAS_LW, api.TAG_GAS_SW, api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_AEROSOL_LW, api.TAG_AEROSOL_SW,
            api.TAG_ALLSKY_LW, api.TAG_ALLSKY_SW, api.TAG_SKY_LW, api.TAG_SKY_SW, api.TAG_SUBCOLUMN_MEAN,
            api.TAG_DIRECT_BEAM, api.TAG_BAND_PROFILES)
    gclouds, kc = make(tables, cl)
    gaer, ka = aerosols_of(case1.f)
    one = np.ones(1)

    def responses(lw=([5], [one]), sw=([5], [one]), weighted=wl, act=al):
        g, k = api.make_responses(lw=lw, sw=sw)
        g.weighted_levels_dev, g.actinic_levels_dev = weighted, act
        return g

    def refused(gresp, gc=gcols, gcl=gclouds, ga=gaer, S_=S, sets=ALL, code=api.VALUE_ERR, sky=True, form=(lv, hr, fx), p=pipe):
        gsky, ks = api.make_sky(gcl, ga, S_, sets)
        with pytest.raises(api.GrtError) as e:
            api.check(lib.grt_pipeline_run_sky_weighted(p.p, C.byref(gc), C.byref(gsky) if sky else None,
                                                        C.byref(gresp) if gresp is not None else None, *form))
        assert e.value.code == code, e.value
        p.sync()
        for b, n in zip(bufs, sizes):
            assert np.all(b.to_host((n,)) == -7.25)

    api.profile_enable(True)
    try:
        api.profile_read(tags[0], reset=True)
        for tag in tags:
            api.profile_read(tag, reset=True)
        refused(None)
        refused(responses(weighted=None))
        refused(responses(lw=None, sw=None, act=None))                                  # both counts 0
        for band in ("lw", "sw"):
            for count in (-1, api.GRT_MAX_RESPONSES + 1):
                g = responses()
                setattr(g, band + "_num_responses", count)
                refused(g)
            for field in ("first", "offset", "weights"):
                g = responses()
                setattr(g, f"{band}_{field}", None)
                refused(g)
            n = bands[0].nw if band == "lw" else bands[1].nw
            for bad in (([-1], [one]), ([n], [one]), ([n - 1], [np.ones(2)]), ([3], [np.array([1.0, np.nan])]),
                        ([3], [np.array([np.inf, 1.0])])):
                refused(responses(**{band: bad}))
            g = responses(**{band: ([5, 9], [np.ones(2), np.ones(3)])})
            g.keep[band + "_offset"][0] = 1
            refused(g)
            g.keep[band + "_offset"][:] = [0, 2, 2]
            refused(g)
            # one response more than the block limit in one block
            limit = pipe.response_block_limit(0 if band == "lw" else 1)
            assert limit == (65536 - 16 * (2 if band == "lw" else 3) * V1) // (16 * (2 if band == "lw" else 3) * V1 + 1024)
            refused(responses(**{band: ([130 + j for j in range(limit + 1)], [np.ones(2)] * (limit + 1))}))
        refused(responses(), p=lw_only)                                                 # a band the pipeline lacks
        refused(responses(sw=None, act=al))                                             # actinic rows of no response
        refused(responses(), form=(None, hr, fx))                                       # level_fluxes_dev
        # everything grt_pipeline_run_sky refuses
        refused(responses(), sky=False)
        for stray in (16, ALL | 32):
            refused(responses(), sets=stray)
        refused(responses(), gcl=None)
        refused(responses(), ga=None)
        for bad in (0, api.GRT_MAX_SUBCOLUMNS + 1):
            refused(responses(), S_=bad)
        gcols.ncol = 0
        refused(responses())
        gcols.ncol = ncol
        night = [dict(c) for c in cols]
        night[1]["mu0"] = 0.0
        gnight, keep_night = api.make_columns(night, MOL_ORDER, cfc_order=(0, 1))
        refused(responses(), gc=gnight, code=api.RANGE_ERR)
        pipe.sync()
        counts = {tag: api.profile_read(tag)[1] for tag in tags}
        assert all(n == 0 for n in counts.values()), counts
        # and the calls accepted: exactly the limit in one block; heating_dev, fluxes_dev and actinic_levels_dev NULL
        limit = pipe.response_block_limit(1)
        gsky, ks = api.make_sky(gclouds, gaer, S, ALL)
        g = responses(lw=None, sw=([130 + j for j in range(limit)], [np.ones(2)] * limit), act=None)
        api.check(lib.grt_pipeline_run_sky_weighted(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(g), lv, None, None))
        pipe.sync()
        rows = bufs[3].to_host((sizes[3],))
        used = ncol * 4 * 3 * limit * V1
        assert np.all(np.isfinite(rows[:used])) and np.all(rows[:used] != -7.25) and np.all(rows[used:] == -7.25)
        assert np.all(bufs[4].to_host((sizes[4],)) == -7.25) and np.all(bufs[1].to_host((sizes[1],)) == -7.25)
        assert api.profile_read(api.TAG_BAND_PROFILES)[1] == 4      # one finishing launch per set of the one band, no actinic
    finally:
        api.profile_enable(False)
    for b in bufs:
        b.free()
    pipe.destroy()
    lw_only.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- (g) the existing entry points, before and after --------------------------------------------------------------------- #
@pytest.mark.parametrize("spectral", [False, True])
def test_existing_entry_points_unchanged(bands, tables, case1, lib, device, spectral):
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)
    lw, sw = (five_responses(b.nw, 5 + bi) for bi, b in enumerate(bands))
    edges = (np.array([0, 100, bands[0].nw - 1], dtype=np.int32), np.array([0, 130, bands[1].nw - 1], dtype=np.int32))

    def older():
        out = {}
        pipe.run(gcols)
        out["run"] = pipe.fluxes(ncol)
        pipe.run_profiles(gcols)
        out.update({"run_profiles." + k: v for k, v in pipe.profiles(ncol).items()})
        for profiles in (False, True):
            out.update({f"run_sky.{profiles}.{k}": v for k, v in
                        run_sky(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles).items()})
            out.update({f"run_sky_direct.{profiles}.{k}": v for k, v in
                        run_direct(pipe, gcols, gclouds, gaer, S, ALL, ncol, profiles).items()})
        pipe.run_band_profiles(gcols, None, lw_edges=edges[0], sw_edges=edges[1])
        out.update({"run_band_profiles." + k: v for k, v in pipe.band_profiles(ncol).items()})
        return out

    _deterministic(lib, True)
    try:
        before = older()
        run_weighted(pipe, gcols, gclouds, gaer, S, ALL, ncol, lw, sw)
        run_weighted(pipe, gcols, gclouds, gaer, 1, CLEAN | CLOUD, ncol, None, sw)
        after = older()
        assert before.keys() == after.keys() and len(before) > 20
        for k in before:
            assert np.array_equal(before[k], after[k]), k
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
