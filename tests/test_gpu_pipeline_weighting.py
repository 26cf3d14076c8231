"""grt_pipeline_run_sky_weighting: grt_pipeline_run_sky_channels with, for the upward radiance at the top, each channel's
level-to-space transmittance profile and contribution function, reduced on the device layer by layer.  Against
weighting_model.py (test_weighting_model.py holds it against radiance_model.py and the oracle's solver) at the edge shapes
of the channel tests -- the same grids, level counts, angle counts, draws and batch sizes, the same instrument of one-point,
whole-grid, edge-crossing, negative-lobed and repeated channels, ascending and descending, and a dense instrument of
channels one point apart, of which a block meets more than it has threads --, fused and materialised; the
closure of the contribution rows on the device; the bit-for-bit identities of the deterministic mode; what the entry point
refuses; a pipeline without a longwave band; and the production arithmetic.  fast = 0 unless said otherwise.

Bounds.  A value against the oracle-fed model: (POINT_TOL largest + TRAP_ULPS 2^-52 largest) sum |W| / sum W, the channel
tests' model bound.  `largest` is the row's largest magnitude at a point over the draws, 1 for a transmittance row.
Derivation: a row's value at a point is a product of up to L extinctions and one emission term, each of the kernel's exp
and divisions within an ulp or two of numpy's, so it stays within POINT_TOL = 1e-12 of the row's largest value as a
radiance does (the radiance tests' per-point bound: a contribution row is one term of that radiance); a weighted mean
magnifies a per-point error by sum |W| / sum W at most; and the additions -- a product and up to 128 sequential additions in
a block, three blocks, three draws, two divisions, against numpy's pairwise sum -- cost 2^-52 largest sum |W| / sum W each
at most, which the second term covers for the instrument's channels of up to 16 points and which POINT_TOL, seventy times
larger, covers for the three wider ones.  Closure: the sum of a channel's V + 1 contribution rows against the channel
radiance of the same call, within twice the sum of the rows' bounds above (each side is within it of the model: the
largest radiance of a row is at most the sum of the rows' largest values) plus weighting_model.closure_bound carried
through |W| / sum W.  Transmittance row 0: 1 within 2^-52 sum |W| / sum W (the instrument's weights are dyadic, so the
device's block-wise sum of them is the host's).  Production (fast = 3): BOUNDS[3]["spectral_flux_rel"] = 1e-5 times the
row's largest model value (1 for a transmittance) times sum |W| / sum W, the channel test's production bound."""
import ctypes as C
import os

import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID
from grtcode_amd import api, channels
from pipeline_support import TRAP_ULPS, _deterministic, _sentinel, _setup, make, pick, subcolumn_clouds
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from test_gpu_parity_production import BOUNDS, record
from test_gpu_pipeline_channels import SHAPES, Instrument, case_instrument, edge_instrument, run_chan
from test_gpu_pipeline_channels import shape_bands  # noqa: F401  (module fixture)
from test_gpu_pipeline_radiances import AEROSOL_SEED, CLOUD_SEED, POINT_TOL, UL1, V1, Shape, run_rad, secants_of
from test_gpu_pipeline_radiances import case1  # noqa: F401  (module fixture)
from test_gpu_pipeline_sky import ALL, NAMES, aerosols_of, fields, sky_columns
from weighting_model import channel_sets, oracle_weighting_points

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52


def run_wt(pipe, gcols, gclouds, gaer, S, sets, ncol, secants, inst, transmittance=True, contribution=True, bright=False,
           spectral=False, fluxes=True):
    """-> dict of trans [ncol][nsets][A][V][C] and contrib [ncol][nsets][A][V + 1][C] (as asked for), channels
    [ncol][nsets][A][2][C], radiances [ncol][nsets][A][2] and, as asked for, tb, spectral and fluxes."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    secants = np.ascontiguousarray(secants, dtype=np.float64)
    pipe.run_sky_weighting(gcols, gsky, secants, inst.g, transmittance=transmittance, contribution=contribution,
                           brightness=bright, spectral=spectral, fluxes=fluxes)
    n, A = keep["nsets"], secants.shape[1]
    out = dict(channels=pipe.sky_channel_radiances(ncol, n, A, inst.C), radiances=pipe.sky_radiances(ncol, n, A))
    if transmittance:
        out["trans"] = pipe.sky_channel_transmittances(ncol, n, A, inst.C)
    if contribution:
        out["contrib"] = pipe.sky_channel_contributions(ncol, n, A, inst.C)
    if bright:
        out["tb"] = pipe.sky_channel_brightness(ncol, n, A, inst.C)
    if spectral:
        out["spectral"] = pipe.sky_spectral_radiances(ncol, n, A)
    if fluxes:
        out["fluxes"] = pipe.sky_fluxes(ncol, n)
    return out


def model_bounds(want, inst):
    """-> (the transmittances' bound [C], the contributions' [A][V + 1][C])"""
    both = POINT_TOL + TRAP_ULPS * ULP
    return both * inst.ratio, both * want["largest"][..., None] * inst.ratio


DENSE_WEIGHTS = np.array([-0.25, 0.5, 1.0, 2.0, 1.5, 0.75, -0.5])      # dyadic, lopsided, negative lobes: sum 5, sum |W| 6.5


def dense_instrument(n, most=None):
    """Channels of seven points (fewer on a shorter grid) one point apart from point 0 on, `most` of them at most: a
    128-point block meets up to 134 of them, more than it has threads, so the gather's loop over a block's list goes round
    twice; every wave's and block's edge is crossed by six of them."""
    w = DENSE_WEIGHTS[:min(n, DENSE_WEIGHTS.size)]
    count = n - w.size + 1 if most is None else min(most, n - w.size + 1)
    return Instrument(np.arange(count), [w] * count)


# ---- 1. and 2. edge shapes: against the model, and the closure on the device -------------------------------------------------- #
_edge = {}


def edge_results(shape, shape_bands, tables, oracle, lib, device):
    """The runs of one edge shape, made once and shared by the two tests below: a list of (what, inst, got, want) for both
    forms of the pipeline, both orders of the channel tests' instrument and the dense instrument, want[c][k] the model's set k
    of column c."""
    if shape in _edge:
        return _edge[shape]
    n, V, A, S, ncol = shape
    sh = Shape(shape_bands, tables, device, n, V, S, ncol)
    sec = secants_of(ncol, A)
    band = sh.lwb
    points = [oracle_weighting_points(oracle, lib, band, sh.cols[c], tables, sh.cl["lw_liquid"][c], sh.cl["lw_ice"][c],
                                      sh.cl["thickness"][c], sh.xs[0], sh.f[0][c], sh.emis, sec[c]) for c in range(ncol)]
    variants = []
    for descending, with_centers in ((False, False), (True, True)):
        inst, whole = edge_instrument(n, band.dw, descending, with_centers)
        variants.append((f"descending={descending}", inst,
                         [channel_sets(points[c], inst.first, inst.weights) for c in range(ncol)]))
    inst = dense_instrument(n)
    variants.append(("dense", inst, [channel_sets(points[c], inst.first, inst.weights) for c in range(ncol)]))
    runs = []
    for spectral in (False, True):
        pipe = sh.pipeline(spectral)
        for name, inst, want in variants:
            got = run_wt(pipe, sh.gcols, sh.gclouds, sh.gaer, S, ALL, ncol, sec, inst)
            runs.append((f"spectral={spectral} {name}", inst, got, want))
        pipe.destroy()
    sh.destroy()
    _edge[shape] = runs
    return runs


IDS = [f"n{n}-V{V}-A{A}-S{S}-c{c}" for n, V, A, S, c in SHAPES]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_edge_shapes(shape_bands, tables, oracle, lib, device, shape):
    """Every value within (POINT_TOL largest + TRAP_ULPS 2^-52 largest) sum |W| / sum W of the model (the module's note)."""
    n, V, A, S, ncol = shape
    for what, inst, got, want in edge_results(shape, shape_bands, tables, oracle, lib, device):
        assert got["trans"].shape == (ncol, 4, A, V, inst.C) and got["contrib"].shape == (ncol, 4, A, V + 1, inst.C)
        assert np.all(np.isfinite(got["trans"])) and np.all(np.isfinite(got["contrib"]))
        worst_t = worst_k = 0.0
        for c in range(ncol):
            for k in range(4):
                tol_t, tol_k = model_bounds(want[c][k], inst)
                err_t = np.abs(got["trans"][c, k] - want[c][k]["trans"]) / tol_t
                err_k = np.abs(got["contrib"][c, k] - want[c][k]["contrib"]) / np.maximum(tol_k, 1e-300)
                # (a row that is 0 at every point in the model, under a surface of emissivity 1 say, is 0 on the device)
                err_k = np.where(tol_k > 0.0, err_k, np.where(got["contrib"][c, k] == want[c][k]["contrib"], 0.0, np.inf))
                worst_t, worst_k = max(worst_t, err_t.max()), max(worst_k, err_k.max())
        print(what, "transmittances: worst", worst_t, "of the bound; contributions: worst", worst_k, "of the bound")
        assert worst_t <= 1.0 and worst_k <= 1.0, (what, worst_t, worst_k)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_closure_on_the_device(shape_bands, tables, oracle, lib, device, shape):
    """Per column, set, angle and channel the V + 1 contribution rows add up to the channel's upward radiance of the same
    call within twice the rows' model bounds plus the model's closure bound carried through the weights; transmittance row
    0 is 1 within 2^-52 sum |W| / sum W."""
    n, V, A, S, ncol = shape
    for what, inst, got, want in edge_results(shape, shape_bands, tables, oracle, lib, device):
        worst = 0.0
        for c in range(ncol):
            for k in range(4):
                tol_t, tol_k = model_bounds(want[c][k], inst)
                tol = 2.0 * tol_k.sum(axis=-2) + want[c][k]["closure"]
                err = np.abs(got["contrib"][c, k].sum(axis=-2) - got["channels"][c, k, :, 0]) / tol
                worst = max(worst, err.max())
        top = np.abs(got["trans"][:, :, :, 0] - 1.0) / (ULP * inst.ratio)
        print(what, "closure: worst", worst, "of the bound; transmittance row 0 against 1: worst", top.max(), "of the bound")
        assert worst <= 1.0, (what, worst)
        assert np.all(top <= 1.0), (what, top.max())
        assert np.all(got["channels"][..., 0, :][..., inst.ratio == 1.0] > 0.0)


# ---- 3. identities, bit for bit, in the deterministic mode ------------------------------------------------------------------ #
@pytest.mark.parametrize("S,spectral", [(1, False), (3, False), (3, True)])
def test_identities_bit_for_bit(bands, tables, case1, lib, device, S, spectral):
    cols, ncol = case1.cols, case1.ncol
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = case1.clouds(S)
    gclouds, keep_clouds = make(tables, cl)
    gaer, keep_aer = aerosols_of(case1.f)
    sec = secants_of(ncol, 5)
    inst = case_instrument(bands[0])
    keys = ("trans", "contrib")
    _deterministic(lib, True)
    try:
        full = run_wt(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst, bright=True)
        assert full["trans"].shape == (ncol, 4, 5, V1, inst.C) and full["contrib"].shape == (ncol, 4, 5, V1 + 1, inst.C)
        # (row 0 is sum W / sum W, the device's sum block by block, the host's in one go: each within count/2 ulps)
        slack = inst.keep["counts"] * ULP
        assert np.all(np.abs(full["trans"][:, :, :, 0] - 1.0) <= slack)
        assert np.all((full["trans"] >= 0.0) & (full["trans"] <= 1.0 + slack))
        assert np.all(np.diff(full["trans"], axis=3) <= slack) and np.all(full["contrib"] >= 0.0)
        assert len({full["contrib"][0, k, 0].tobytes() for k in range(4)}) == 4                # the four sets differ
        # every output run_sky_channels and run_sky_radiances also write is theirs
        chan = run_chan(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst)
        for key in ("channels", "tb", "radiances", "fluxes"):
            assert np.array_equal(full[key], chan[key]), key
        plain = run_rad(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec)
        for key in ("radiances", "fluxes"):
            assert np.array_equal(full[key], plain[key]), key
        # two consecutive calls
        again = run_wt(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst, bright=True)
        for key in keys + ("channels", "tb", "radiances", "fluxes"):
            assert np.array_equal(again[key], full[key]), key
        # duplicates are equal; a sub-instrument gives its channels, with one angle or five
        for key in keys:
            assert np.array_equal(full[key][..., 3], full[key][..., inst.C - 1]), key
        for idx in ((10,), (12, 5, 10, 3)):
            part = inst.take(idx)
            for a in (slice(0, 5), slice(3, 4)):
                one = run_wt(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec[:, a], part)
                for key in keys:
                    assert np.array_equal(one[key], full[key][:, :, a][..., list(idx)]), (key, idx, a)
        # the dense instrument (a block's list longer than the workgroup): channels of it alone, across a block's edge and
        # where the list goes round, with one angle or five, are the channels among the others
        dense = dense_instrument(bands[0].nw, most=300)
        crowd = run_wt(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, dense)
        assert np.all(np.abs(crowd["trans"][:, :, :, 0] - 1.0) <= ULP * dense.ratio)
        for idx in ((0,), (299, 127, 128, 122, 250, 5)):
            part = dense.take(idx)
            for a in (slice(0, 5), slice(4, 5)):
                one = run_wt(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec[:, a], part)
                for key in keys + ("channels",):
                    assert np.array_equal(one[key], crowd[key][:, :, a][..., list(idx)]), (key, idx, a)
        # a column alone is the column in the batch
        c = ncol - 1
        g1, k1 = api.make_columns([cols[c]], MOL_ORDER, cfc_order=(0, 1))
        gc1, kc1 = make(tables, pick(cl, columns=[c]))
        ga1, ka1 = aerosols_of(tuple(np.ascontiguousarray(f[[c]]) for f in case1.f))
        alone = run_wt(pipe, g1, gc1, ga1, S, ALL, 1, sec[[c]], inst)
        for key in keys + ("channels", "radiances", "fluxes"):
            assert np.array_equal(alone[key][0], full[key][c]), (key, c)
        # one of the two outputs alone is that output of the call for both
        only_t = run_wt(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst, contribution=False)
        assert np.array_equal(only_t["trans"], full["trans"]) and np.array_equal(only_t["channels"], full["channels"])
        only_k = run_wt(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst, transmittance=False)
        assert np.array_equal(only_k["contrib"], full["contrib"]) and np.array_equal(only_k["channels"], full["channels"])
        # without fluxes: the same outputs; one weighting launch per radiance launch, one finishing launch per set
        api.profile_enable(True)
        try:
            api.profile_read(api.TAG_RADIANCE, reset=True)
            bare = run_wt(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst, fluxes=False)
            for key in keys + ("channels", "radiances"):
                assert np.array_equal(bare[key], full[key]), key
            per_call = 4 if not spectral or S == 1 else 2 + 2 * S
            assert api.profile_read(api.TAG_RADIANCE)[1] == per_call
            assert api.profile_read(api.TAG_WEIGHTING)[1] == per_call
            assert api.profile_read(api.TAG_CHANNELS)[1] == 4 and api.profile_read(api.TAG_WEIGHTING_FINISH)[1] == 4
        finally:
            api.profile_enable(False)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 4. refusals, and a pipeline without a longwave band --------------------------------------------------------------------- #
def test_refused_inputs(bands, tables, case1, lib, device):
    cols, ncol, S, A = case1.cols, case1.ncol, 3, 5
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    inst = case_instrument(bands[0])
    NC = inst.C
    rows = 4 * A * 2 * (ncol + 1)
    per_level = 4 * A * NC * (ncol + 1)
    sizes = (rows, 4 * 12 * (ncol + 1), rows * NC, rows * NC, per_level * V1, per_level * (V1 + 1))
    bufs = [_sentinel(device, k) for k in sizes]
    rad, fx, ch_rad, ch_tb, wt_t, wt_k = (b.ptr for b in bufs)
    good = secants_of(ncol, A)
    tags = tuple(range(1, api.TAG_WEIGHTING_FINISH + 1))
    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)

    def radiances(secants=good):
        m = np.ascontiguousarray(secants, dtype=np.float64)
        g = api.GrtRadiances(m.shape[1], m.ctypes.data_as(C.POINTER(C.c_double)), rad, None, None)
        g.keep = m
        return g

    def chans(offset=None):
        g, k = api.make_channels(inst.first, inst.weights, inst.center)
        g.channel_radiances_dev, g.channel_brightness_dev = ch_rad, ch_tb
        if offset is not None:
            k["bad"] = np.ascontiguousarray(offset, dtype=np.int32)
            g.offset = k["bad"].ctypes.data_as(C.POINTER(C.c_int))
        g.keep2 = k
        return g

    def call(gch, gw, grad, sets, fluxes):
        gsky, ks = api.make_sky(gclouds, gaer, S, sets)
        return lib.grt_pipeline_run_sky_weighting(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(grad), C.byref(gch),
                                                  C.byref(gw) if gw is not None else None, fluxes)

    def refused(gw, gch=None, grad=None, sets=ALL):
        for f in (fx, None):
            with pytest.raises(api.GrtError) as e:
                api.check(call(chans() if gch is None else gch, gw, radiances() if grad is None else grad, sets, f))
            assert e.value.code == api.VALUE_ERR, e.value
        pipe.sync()
        for b, k in zip(bufs, sizes):
            assert np.all(b.to_host((k,)) == -7.25)

    api.profile_enable(True)
    try:
        api.profile_read(tags[0], reset=True)
        refused(None)
        refused(api.GrtWeighting(None, None))
        # one refusal each of the channels', the radiances' and the sky's layer
        bad = inst.keep["offset"].copy()
        bad[4] = bad[3]
        refused(api.GrtWeighting(wt_t, wt_k), gch=chans(offset=bad))
        bad = good.copy()
        bad[ncol - 1, A - 1] = 0.5
        refused(api.GrtWeighting(wt_t, wt_k), grad=radiances(secants=bad))
        refused(api.GrtWeighting(wt_t, wt_k), sets=16)
        counts = {tag: api.profile_read(tag)[1] for tag in tags}
        assert all(v == 0 for v in counts.values()), counts
    finally:
        api.profile_enable(False)
    # and the call accepted, with either output alone: the rows past the batch untouched, the output not asked for too
    api.check(call(chans(), api.GrtWeighting(wt_t, None), radiances(), ALL, None))
    pipe.sync()
    got = bufs[4].to_host((ncol + 1, 4, A, V1, NC))
    assert np.all(np.abs(got[:ncol, :, :, 0] - 1.0) <= inst.keep["counts"] * ULP) and np.all(got[ncol] == -7.25)
    assert np.all(bufs[5].to_host((sizes[5],)) == -7.25) and np.all(bufs[1].to_host((sizes[1],)) == -7.25)
    api.check(call(chans(), api.GrtWeighting(None, wt_k), radiances(), ALL, None))
    pipe.sync()
    got = bufs[5].to_host((ncol + 1, 4, A, V1 + 1, NC))
    assert np.all(np.isfinite(got[:ncol])) and np.all(got[:ncol].sum(axis=3) > 0.0) and np.all(got[ncol] == -7.25)
    for b in bufs:
        b.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_no_longwave_band(bands, tables, case1, lib, device):
    cols, ncol, S = case1.cols, case1.ncol, 3
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)
    sec = secants_of(ncol, 5)
    inst = Instrument([0, 10 ** 6], [np.ones(3), np.ones(2)], [700.0, 900.0])
    sw_only = api.Pipeline(None, go_sw, ncol, UL1, None, alb, solar, spectral=False)
    run_wt(sw_only, gcols, gclouds, gaer, S, ALL, ncol, sec, inst)                       # (allocates the buffers)
    for name in ("sky.channel_transmittances", "sky.channel_contributions"):
        buf = sw_only.buffers[name]
        fill = np.full(buf.nbytes // 8, -7.25)                                           # zeros are written, not left
        api.check(lib.grt_host_to_device(device, buf.ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(fill.nbytes)))
    for fluxes in (True, False):
        out = run_wt(sw_only, gcols, gclouds, gaer, S, ALL, ncol, sec, inst, fluxes=fluxes)
        for key in ("trans", "contrib", "channels", "radiances"):
            assert np.all(out[key] == 0.0) and not np.any(np.signbit(out[key])), key
    assert out["trans"].shape == (ncol, 4, 5, V1, 2) and out["contrib"].shape == (ncol, 4, 5, V1 + 1, 2)
    sw_only.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 5. the production arithmetic -------------------------------------------------------------------------------------------- #
def test_production_form_matches_the_model(bands, tables, oracle, lib, device):
    """fast = 3 on the 3 000-line band, two columns, all four sets, two draws, three angles, Gaussian channels every 100
    cm-1 (FWHM 50 cm-1) and three one-point channels, against the model on the oracle's tau: contributions within
    BOUNDS[3]["spectral_flux_rel"] x the row's largest model value x sum |W| / sum W, transmittances within the same
    relative figure of 1.  The worst values met on an MI355X: contributions 1.8e-2 of their bound, transmittances 9.9e-3 of
    theirs."""
    S = 2
    rel = BOUNDS[3]["spectral_flux_rel"]
    band = bands[0]
    cols = sky_columns(320, V1, n=2)
    ncol = len(cols)
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1, fast=3)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, CLOUD_SEED + 1, S)
    gclouds, keep_clouds = make(tables, cl)
    f = fields(ncol, V1 - 1, AEROSOL_SEED + 2)
    gaer, keep_aer = aerosols_of(f)
    sec = np.tile(np.array((1.0, 1.5, 3.0)), (ncol, 1))
    w_end = band.w0 + (band.nw - 1) * band.dw
    first, weights, centers = channels.gaussian(band.w0, band.dw, band.nw, np.arange(100.0, w_end + 1.0, 100.0), 50.0)
    points = [0, band.nw // 2 + 1, band.nw - 1]
    inst = Instrument(list(first) + points, weights + [np.ones(1)] * 3,
                      list(centers) + [band.w0 + p * band.dw for p in points])
    got = run_wt(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst)
    assert go_lw.last_launch()["fast"] == 3
    worst_t = worst_k = 0.0
    for c, col in enumerate(cols):
        pts = oracle_weighting_points(oracle, lib, band, col, tables, cl["lw_liquid"][c], cl["lw_ice"][c], cl["thickness"][c],
                                      AEROSOL_GRID, f[0][c], emis, sec[c])
        for k, wk in enumerate(channel_sets(pts, inst.first, inst.weights)):
            frac_t = float((np.abs(got["trans"][c, k] - wk["trans"]) / (rel * inst.ratio)).max())
            tol_k = rel * wk["largest"][..., None] * inst.ratio
            frac_k = float((np.abs(got["contrib"][c, k] - wk["contrib"]) / tol_k).max())
            worst_t, worst_k = max(worst_t, frac_t), max(worst_k, frac_k)
            print("production column", c, "set", NAMES[k], "worst error as a fraction of its bound: transmittances", frac_t,
                  "contributions", frac_k)
    mode = "deterministic" if os.environ.get("GRT_DETERMINISTIC", "0") not in ("", "0") else "default"
    record("run_sky_weighting." + mode, {"transmittances": {"worst_fraction_of_bound": worst_t, "relative_bound": rel},
                                         "contributions": {"worst_fraction_of_bound": worst_k, "relative_bound": rel}},
           file="parity_pipeline_production.json")
    assert worst_t <= 1.0 and worst_k <= 1.0, (worst_t, worst_k)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
