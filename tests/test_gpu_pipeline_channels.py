"""grt_pipeline_run_sky_channels: grt_pipeline_run_sky_radiances with the radiances and brightness temperatures of an
instrument's channels, reduced on the device.  Against channel_model.py (test_channel_model.py holds it against the oracle's
trapezoid and planck()) at the edge shapes of the kernel -- channels of one point at both grid ends, the whole grid, across
a wave's and a block's edge, with negative weights, twice, and in descending order --, fused and materialised; the
bit-for-bit identities of the deterministic mode; what the entry point refuses; a pipeline without a longwave band; and the
production arithmetic.  fast = 0 unless said otherwise.

Bounds.  A channel value against channel_mean of the kernel's own spectral row (one draw): TRAP_ULPS 2^-52 magnitude,
magnitude = sum |W I| / sum W; TRAP_ULPS = 64 bounds the depth of the addition tree here (product, six shuffle steps, two
waves, three blocks, three draws, two divisions): derived from the code, not measured.  Against the oracle-fed model (three
draws): (POINT_TOL largest + TRAP_ULPS 2^-52 largest) sum |W| / sum W, the radiance tests' per-point bound carried through
a weighted mean.  The whole-grid trapezoid channel times sum W: assert_trapezoid on the kernel's own row where there is
one, and against radiances_dev of the same call by assert_trapezoid's bound, TRAP_ULPS 2^-52 dw sum |row| -- the row the
kernel's own where it leaves, else (three draws) the model's rows, the mean over the draws.  Brightness: 1e-10 K of
the formula on the kernel's own channel radiance.  Production (fast = 3): the project's pointwise spectral bound,
BOUNDS[3]["spectral_flux_rel"] = 1e-5, times the row's largest model radiance times sum |W| / sum W -- a flux at a point
is the positively weighted sum of four such radiances, so the bound carries over to a radiance, and a weighted mean cannot
exceed it by more than the sign ratio."""
import ctypes as C
import os

import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID
from channel_model import (channel_brightness, channel_mean, centroid, magnitude, oracle_channel_sets, pair_count,
                           sign_ratio, weight_sum)
from grtcode_amd import api, channels
from pipeline_support import (SETS, TRAP_ULPS, _deterministic, _sentinel, _setup, assert_trapezoid, clouds_for, make,
                              make_shape_bands, pick, subcolumn_clouds)
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from radiance_model import STREAM_SECANTS
from scenario import MOL_ORDER
from test_gpu_parity_production import BOUNDS, record
from test_gpu_pipeline_radiances import (AEROSOL_SEED, BRIGHTNESS_TOL, CLOUD_SEED, POINT_TOL, UL1, V1, Shape, run_rad,
                                         secants_of)
from test_gpu_pipeline_radiances import case1  # noqa: F401  (module fixture)
from test_gpu_pipeline_sky import ALL, CLOUD, NAMES, aerosols_of, fields, sky_columns

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -52
shape_bands = make_shape_bands((2, 65, 129, 257), 100.0, 2000.0)


class Instrument:
    """first [C], weights (a list of C arrays), center [C] or None (the centroid), and the struct of them."""

    def __init__(self, first, weights, center=None):
        self.first = [int(f) for f in first]
        self.weights = [np.asarray(w, dtype=np.float64) for w in weights]
        self.center = None if center is None else np.asarray(center, dtype=np.float64)
        self.g, self.keep = api.make_channels(self.first, self.weights, self.center)
        self.C = len(self.first)
        self.ratio = sign_ratio(self.weights)
        self.sum_w = np.array([weight_sum(w) for w in self.weights])

    def centers(self, band):
        return self.center if self.center is not None else centroid(self.first, self.weights, band.w0, band.dw)

    def take(self, idx, center=True):
        return Instrument([self.first[i] for i in idx], [self.weights[i] for i in idx],
                          None if self.center is None or not center else self.center[list(idx)])


def run_chan(pipe, gcols, gclouds, gaer, S, sets, ncol, secants, inst, bright=True, spectral=False, fluxes=True):
    """-> dict of channels [ncol][nsets][A][2][C], tb (the same, if asked for), radiances [ncol][nsets][A][2] and, as asked
    for, spectral [ncol][nsets][A][2][n] and fluxes [ncol][nsets][12]."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    secants = np.ascontiguousarray(secants, dtype=np.float64)
    pipe.run_sky_channels(gcols, gsky, secants, inst.g, brightness=bright, spectral=spectral, fluxes=fluxes)
    n, A = keep["nsets"], secants.shape[1]
    out = dict(channels=pipe.sky_channel_radiances(ncol, n, A, inst.C), radiances=pipe.sky_radiances(ncol, n, A))
    if bright:
        out["tb"] = pipe.sky_channel_brightness(ncol, n, A, inst.C)
    if spectral:
        out["spectral"] = pipe.sky_spectral_radiances(ncol, n, A)
    if fluxes:
        out["fluxes"] = pipe.sky_fluxes(ncol, n)
    return out


def trapezoid_weights(n, dw):
    w = np.full(n, dw)
    w[0] = w[-1] = 0.5 * dw
    return w


def edge_instrument(n, dw, descending, with_centers):
    """The channels of the issue's list that exist on n points; channel 0 (ascending) or the last one (descending) is the
    whole grid with the trapezoid's weights.  With centres given, a two-point channel of nearly cancelling weights joins:
    where the radiance rises by more than 1 % from point 0 to point 1 its value is negative."""
    first, weights = [0, 0, n - 1], [trapezoid_weights(n, dw), [1.0], [2.5]]
    for lo, hi in ((60, 67), (120, 135), (127, 128)):
        if hi < n:
            first.append(lo)
            weights.append(0.25 + np.arange(hi - lo + 1) * 0.5)
    if n > 200:
        lobes = np.full(101, -0.5)                                     # sum |W| / sum W = 76 / 26
        lobes[25:76] = 1.0
        first += [100]
        weights += [lobes]
    first += [first[-1], first[-1]]                                    # the same channel twice more
    weights += [weights[-1], weights[-1]]
    if with_centers:
        first.append(0)
        weights.append([1.0, -0.99])
    order = np.argsort(first, kind="stable")
    order = order[::-1] if descending else order
    center = 150.0 + 7.0 * np.arange(len(first)) if with_centers else None
    inst = Instrument([first[i] for i in order], [weights[i] for i in order], center)
    return inst, int(np.flatnonzero(order == 0)[0])


# ---- 1. edge shapes, against the model ---------------------------------------------------------------------------------------- #
SHAPES = [(2, 2, 1, 1, 1), (65, 13, 5, 1, 3), (129, 2, 5, 3, 1), (257, 3, 1, 3, 3), (257, 13, 4, 1, 3)]


def check_own_row(got, inst, whole, band, what):
    """One draw: every channel value against channel_mean of the kernel's own spectral row, the whole-grid channel against
    the integrated radiance of the same call, the brightness temperatures."""
    rows = got["spectral"]
    want, mag = channel_mean(rows, inst.first, inst.weights), magnitude(rows, inst.first, inst.weights)
    err = np.abs(got["channels"] - want)
    print(what, "channels against the kernel's own rows: worst", (err / np.maximum(TRAP_ULPS * ULP * mag, 1e-300)).max(),
          "of the bound")
    assert np.all(err <= TRAP_ULPS * ULP * mag), (what, err.max())
    integral = got["channels"][..., whole] * inst.sum_w[whole]
    worst = 0.0
    for at in np.ndindex(integral.shape):
        assert_trapezoid(integral[at], rows[at], band.dw, (what, at))
        mag_t = band.dw * np.abs(rows[at]).sum()
        worst = max(worst, abs(integral[at] - got["radiances"][at]) / (TRAP_ULPS * ULP * mag_t))
        assert abs(integral[at] - got["radiances"][at]) <= TRAP_ULPS * ULP * mag_t, (what, at)
    print(what, "whole-grid channel against the integrated radiance: worst", worst, "of the bound")


def check_brightness(got, inst, band, what):
    tb, R = got["tb"], got["channels"]
    err = np.abs(tb - channel_brightness(R, inst.centers(band))).max()
    print(what, "brightness temperatures: worst", err, "K;", int((R <= 0.0).sum()), "values without radiance")
    assert err <= BRIGHTNESS_TOL, (what, err)
    assert np.all(tb[R <= 0.0] == 0.0) and not np.any(np.signbit(tb[R <= 0.0]))
    assert np.all(np.isfinite(tb))


def check_model(got, c, k, want, inst, whole, band, what):
    """Set k of column c against the oracle-fed model, and the whole-grid channel against the call's integrated radiance."""
    largest = want["largest"][..., None]
    tol = (POINT_TOL * largest + TRAP_ULPS * ULP * largest) * inst.ratio
    err = np.abs(got["channels"][c, k] - want["chan"])
    print(what, "column", c, "set", k, "against the model: worst", (err / tol).max(), "of the bound")
    assert np.all(err <= tol), (what, c, k, (err / tol).max())
    integral = got["channels"][c, k, :, :, whole] * inst.sum_w[whole]
    mag_t = band.dw * want["absolute"]         # (assert_trapezoid's magnitude, from the model's rows: none leaves here)
    err_t = np.abs(integral - got["radiances"][c, k]) / (TRAP_ULPS * ULP * mag_t)
    print(what, "column", c, "set", k, "whole-grid channel against the integrated radiance: worst", err_t.max(), "of the bound")
    assert np.all(err_t <= 1.0), (what, c, k, err_t.max())


@pytest.mark.parametrize("n,V,A,S,ncol", SHAPES, ids=[f"n{n}-V{V}-A{A}-S{S}-c{c}" for n, V, A, S, c in SHAPES])
def test_edge_shapes(shape_bands, tables, oracle, lib, device, n, V, A, S, ncol):
    sh = Shape(shape_bands, tables, device, n, V, S, ncol)
    sec = secants_of(ncol, A)
    band = sh.lwb
    variants = []
    for descending, with_centers in ((False, False), (True, True)):
        inst, whole = edge_instrument(n, band.dw, descending, with_centers)
        assert api.channel_pair_count(inst.g, n) == pair_count(inst.first, inst.keep["counts"], n)
        want = None
        if S > 1 or not descending:
            want = [oracle_channel_sets(oracle, lib, band, sh.cols[c], tables, sh.cl["lw_liquid"][c], sh.cl["lw_ice"][c],
                                        sh.cl["thickness"][c], sh.xs[0], sh.f[0][c], sh.emis, sec[c], inst.first, inst.weights)
                    for c in range(ncol)]
        variants.append((descending, inst, whole, want))
    for spectral in (False, True):
        pipe = sh.pipeline(spectral)
        for descending, inst, whole, want in variants:
            what = f"spectral={spectral} descending={descending}"
            got = run_chan(pipe, sh.gcols, sh.gclouds, sh.gaer, S, ALL, ncol, sec, inst, spectral=S == 1)
            assert got["channels"].shape == (ncol, 4, A, 2, inst.C) and np.all(np.isfinite(got["channels"]))
            check_brightness(got, inst, band, what)
            if S == 1:
                check_own_row(got, inst, whole, band, what)
            if want is not None:
                for c in range(ncol):
                    for k in range(4):
                        check_model(got, c, k, want[c][k], inst, whole, band, what)
        pipe.destroy()
    sh.destroy()


# ---- 2. identities, bit for bit, in the deterministic mode ------------------------------------------------------------------ #
def case_instrument(band, center=True):
    """Gaussian channels every 37 cm-1 (FWHM 11 cm-1: most lie across a block's edge or a wave's), a boxcar over the whole
    grid, one-point channels at both ends, one channel twice."""
    n = band.nw
    first, weights, centers = channels.gaussian(band.w0, band.dw, n, band.w0 + 20.0 + 37.0 * np.arange(10), 11.0)
    bf, bw, bc = channels.boxcar(band.w0, band.dw, n, [band.w0 - 5.0], [band.w0 + n * band.dw])
    first = list(first) + list(bf) + [0, n - 1, int(first[3])]
    weights = weights + bw + [np.ones(1), np.ones(1), weights[3]]
    centers = list(centers) + list(bc) + [band.w0, band.w0 + (n - 1) * band.dw, centers[3]]
    return Instrument(first, weights, centers if center else None)


@pytest.mark.parametrize("spectral", [False, True])
@pytest.mark.parametrize("S", [1, 3])
def test_identities_bit_for_bit(bands, tables, case1, lib, device, S, spectral):
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
    sec = secants_of(ncol, 5)
    inst = case_instrument(bands[0])
    every = S == 1
    keys = ("channels", "tb")
    tags = (api.TAG_GAS_SW, api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_AEROSOL_LW, api.TAG_AEROSOL_SW, api.TAG_ALLSKY_LW,
            api.TAG_ALLSKY_SW, api.TAG_SKY_LW, api.TAG_SKY_SW)
    _deterministic(lib, True)
    try:
        full = run_chan(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst, spectral=every)
        assert np.all(full["channels"][..., 0, :] > 0.0) and np.all(np.isfinite(full["channels"]))
        assert np.all((full["tb"][..., 0, :] > 100.0) & (full["tb"][..., 0, :] < 400.0))
        assert len({full["channels"][0, k, 0, 0].tobytes() for k in range(4)}) == 4          # the four sets differ
        # every output run_sky_radiances also writes is run_sky_radiances'
        plain = run_rad(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, spectral=every)
        for key in ("radiances", "fluxes") + (("spectral",) if every else ()):
            assert np.array_equal(full[key], plain[key]), key
        if every:
            # (the Python call has no per-point brightness: the C entry point with brightness_dev)
            want_tb = run_rad(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, bright=True)["brightness"]
            rows, n_lw = ncol * 4 * 5 * 2, bands[0].nw
            bufs = [_sentinel(device, k) for k in (rows, rows * n_lw, rows * inst.C)]
            m = np.ascontiguousarray(sec)
            grad = api.GrtRadiances(5, m.ctypes.data_as(C.POINTER(C.c_double)), bufs[0].ptr, None, bufs[1].ptr)
            gch, kch = api.make_channels(inst.first, inst.weights, inst.center)
            gch.channel_radiances_dev = bufs[2].ptr
            gsky, ks = api.make_sky(gclouds, gaer, S, ALL)
            api.check(lib.grt_pipeline_run_sky_channels(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(grad), C.byref(gch), None))
            pipe.sync()
            assert np.array_equal(bufs[1].to_host((ncol, 4, 5, 2, n_lw)), want_tb)
            assert np.array_equal(bufs[2].to_host((ncol, 4, 5, 2, inst.C)), full["channels"])
            for b in bufs:
                b.free()
        # duplicates are equal
        assert np.array_equal(full["channels"][..., 3], full["channels"][..., inst.C - 1])
        assert np.array_equal(full["tb"][..., 3], full["tb"][..., inst.C - 1])
        # a channel alone, first, last and among the others, with one angle or five
        for idx in ((3,), (10,), (3, 0, 10, 5), (12, 5, 10, 3), (10, 11, 3)):
            part = inst.take(idx)
            for a in (slice(0, 5), slice(3, 4)):
                one = run_chan(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec[:, a], part)
                for key in keys:
                    assert np.array_equal(one[key], full[key][:, :, a][..., list(idx)]), (key, idx, a)
        # the keyed table: the same instrument again equals the first call, another one in between does not disturb it
        again = run_chan(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst, spectral=every)
        for key in keys:
            assert np.array_equal(again[key], full[key]), key
        # the centroid of a one-point channel is its point: the same temperatures without centres
        ends = run_chan(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst.take((11, 12), center=False))
        assert np.array_equal(ends["tb"], full["tb"][..., [11, 12]])
        # a column alone is the column in the batch
        for c in (0, ncol - 1):
            g1, k1 = api.make_columns([cols[c]], MOL_ORDER, cfc_order=(0, 1))
            gc1, kc1 = make(tables, pick(cl, columns=[c]))
            ga1, ka1 = aerosols_of(tuple(np.ascontiguousarray(f[[c]]) for f in case1.f))
            alone = run_chan(pipe, g1, gc1, ga1, S, ALL, 1, sec[[c]], inst)
            for key in keys + ("fluxes", "radiances"):
                assert np.array_equal(alone[key][0], full[key][c]), (key, c)
        # an aerosol of zeros: the aerosol sets are the clean and the cloud sets
        z = run_chan(pipe, gcols, gclouds, gzero, S, ALL, ncol, sec, inst)
        for key in keys:
            assert np.array_equal(z[key][:, 1], z[key][:, 0]) and np.array_equal(z[key][:, 3], z[key][:, 2]), key
            assert np.array_equal(z[key][:, [0, 2]], full[key][:, [0, 2]]), key
        # cloud-free tables (one draw): the cloud sets are the clean and the aerosol sets
        nc = run_chan(pipe, gcols, gclear, gaer, 1, ALL, ncol, sec, inst)
        for key in keys:
            assert np.array_equal(nc[key][:, 2], nc[key][:, 0]) and np.array_equal(nc[key][:, 3], nc[key][:, 1]), key
            assert np.array_equal(nc[key][:, [0, 1]], full[key][:, [0, 1]]), key
        # without fluxes: the channel outputs unchanged, no flux solver and no shortwave, and a night column is no error
        night = [dict(c, mu0=-0.2) for c in cols]
        gnight, keep_night = api.make_columns(night, MOL_ORDER, cfc_order=(0, 1))
        api.profile_enable(True)
        try:
            api.profile_read(api.TAG_RADIANCE, reset=True)
            for g in (gcols, gnight):
                alone = run_chan(pipe, g, gclouds, gaer, S, ALL, ncol, sec, inst, fluxes=False)
                for key in keys + ("radiances",):
                    assert np.array_equal(alone[key], full[key]), key
            # (fused form only: the materialised form's pass optics count under the aerosol and all-sky tags)
            if not spectral:
                counts = {tag: api.profile_read(tag)[1] for tag in tags}
                assert all(v == 0 for v in counts.values()), counts
            # (the materialised form's radiance kernel runs once per draw of a cloud set)
            per_call = 4 if not spectral or S == 1 else 2 + 2 * S
            assert api.profile_read(api.TAG_RADIANCE)[1] == 2 * per_call
            assert api.profile_read(api.TAG_CHANNELS)[1] == 2 * 4                            # one launch per set
        finally:
            api.profile_enable(False)
        with pytest.raises(api.GrtError):                    # (with fluxes the night column is run_sky's error)
            run_chan(pipe, gnight, gclouds, gaer, S, ALL, ncol, sec, inst)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 3. refusals, and a pipeline without a longwave band --------------------------------------------------------------------- #
def test_refused_inputs(bands, tables, case1, lib, device):
    cols, ncol, S, A = case1.cols, case1.ncol, 3, 5
    n = bands[0].nw
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1)
    pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    inst = case_instrument(bands[0])
    NC = inst.C
    rows = 4 * A * 2 * (ncol + 1)
    sizes = (rows, rows * n, rows * n, 4 * 12 * (ncol + 1), rows * NC, rows * NC)
    bufs = [_sentinel(device, k) for k in sizes]
    rad, spec, tb, fx, ch_rad, ch_tb = (b.ptr for b in bufs)
    good = secants_of(ncol, A)
    tags = tuple(range(1, api.TAG_CHANNELS + 1))

    def radiances(out=rad, spectral=None, bright=None, secants=good):
        m = np.ascontiguousarray(secants, dtype=np.float64)
        g = api.GrtRadiances(m.shape[1], m.ctypes.data_as(C.POINTER(C.c_double)), out, spectral, bright)
        g.keep = m
        return g

    def chans(out=ch_rad, bright=ch_tb, **changes):
        """The instrument's struct with these fields replaced."""
        g, k = api.make_channels(inst.first, inst.weights, inst.center)
        g.channel_radiances_dev, g.channel_brightness_dev = out, bright
        arrays = []
        for name, value in changes.items():
            if name in ("first", "offset") and value is not None:
                value = np.ascontiguousarray(value, dtype=np.int32)
                arrays.append(value)
                value = value.ctypes.data_as(C.POINTER(C.c_int))
            elif name in ("weights", "center") and value is not None:
                value = np.ascontiguousarray(value, dtype=np.float64)
                arrays.append(value)
                value = value.ctypes.data_as(C.POINTER(C.c_double))
            setattr(g, name, value)
        g.keep2 = (k, arrays)
        return g

    def refused(gch, grad=None, gcl=None, ga=None, S_=S, sets=ALL, sky=True, gc=gcols, fluxes=(fx, None)):
        gsky, ks = api.make_sky(gclouds if gcl is None else gcl, gaer if ga is None else ga, S_, sets)
        grad = radiances() if grad is None else grad
        for f in fluxes:
            with pytest.raises(api.GrtError) as e:
                api.check(lib.grt_pipeline_run_sky_channels(pipe.p, C.byref(gc), C.byref(gsky) if sky else None, C.byref(grad),
                                                            C.byref(gch) if gch is not None else None, f))
            assert e.value.code == api.VALUE_ERR, (sets, e.value)
        pipe.sync()
        for b, k in zip(bufs, sizes):
            assert np.all(b.to_host((k,)) == -7.25)

    gclouds, kc = make(tables, case1.clouds(S))
    gaer, ka = aerosols_of(case1.f)
    offset, weights, center = inst.keep["offset"], inst.keep["weights"], inst.center
    api.profile_enable(True)
    try:
        api.profile_read(tags[0], reset=True)
        refused(None)
        refused(chans(out=None))
        for name in ("first", "offset", "weights"):
            refused(chans(**{name: None}))
        for bad in (0, -1, api.GRT_MAX_CHANNELS + 1):
            refused(chans(num_channels=bad))
        bad = offset.copy()
        bad[0] = 1
        refused(chans(offset=bad))
        bad = offset.copy()
        bad[4] = bad[3]
        refused(chans(offset=bad))
        bad = offset.copy()
        bad[NC] = bad[NC - 1] - 1
        refused(chans(offset=bad))
        for at, value in ((0, -1), (12, n), (10, 1)):                 # (10: the whole grid, one point on)
            bad = np.array(inst.first)
            bad[at] = value
            refused(chans(first=bad))
        for value in (float("nan"), float("inf"), -float("inf")):
            for at in (0, weights.size - 1):
                bad = weights.copy()
                bad[at] = value
                refused(chans(weights=bad))
        bad = weights.copy()
        bad[offset[11]] = 0.0                                                   # a one-point channel of weight 0
        refused(chans(weights=bad))
        bad[offset[11]] = -1.0
        refused(chans(weights=bad))
        bad = weights.copy()
        bad[offset[2]:offset[3]] = 1e308                                        # a sum that overflows
        refused(chans(weights=bad))
        for value in (float("nan"), float("inf"), 0.0, -500.0):
            bad = center.copy()
            bad[NC - 1] = value
            refused(chans(center=bad))
        # everything grt_pipeline_run_sky_radiances refuses: its own inputs, the outputs at every point of several draws, the sky
        refused(chans(), grad=radiances(out=None))
        bad = good.copy()
        bad[ncol - 1, A - 1] = 0.5
        refused(chans(), grad=radiances(secants=bad))
        refused(chans(), grad=radiances(spectral=spec))
        refused(chans(), grad=radiances(bright=tb), sets=CLOUD)
        refused(chans(), sky=False)
        refused(chans(), sets=16)
        refused(chans(), S_=0)
        gcols.ncol = 0
        refused(chans())
        gcols.ncol = ncol
        counts = {tag: api.profile_read(tag)[1] for tag in tags}
        assert all(v == 0 for v in counts.values()), counts
    finally:
        api.profile_enable(False)
    # and the call accepted: a cloud set of three draws with channel outputs, the rows past the batch untouched
    gsky, ks = api.make_sky(gclouds, gaer, S, ALL)
    api.check(lib.grt_pipeline_run_sky_channels(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(radiances()), C.byref(chans()),
                                                None))
    pipe.sync()
    got = bufs[4].to_host((ncol + 1, 4, A, 2, NC))
    assert np.all(np.isfinite(got[:ncol])) and np.all(got[:ncol, :, :, 0] > 0.0) and np.all(got[ncol] == -7.25)
    temps = bufs[5].to_host((ncol + 1, 4, A, 2, NC))
    assert np.all((temps[:ncol, :, :, 0] > 100.0) & (temps[:ncol, :, :, 0] < 400.0)) and np.all(temps[ncol] == -7.25)
    integ = bufs[0].to_host((ncol + 1, 4, A, 2))
    assert np.all(integ[:ncol, :, :, 0] > 0.0) and np.all(integ[ncol] == -7.25)
    for k in (1, 2, 3):
        assert np.all(bufs[k].to_host((sizes[k],)) == -7.25)
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
    # (no range check on first: a channel far past any longwave grid)
    inst = Instrument([0, 10 ** 6], [np.ones(3), np.ones(2)], [700.0, 900.0])
    sw_only = api.Pipeline(None, go_sw, ncol, UL1, None, alb, solar, spectral=False)
    run_chan(sw_only, gcols, gclouds, gaer, S, ALL, ncol, sec, inst)                     # (allocates the buffers)
    for name in ("sky.channel_radiances", "sky.channel_brightness"):
        buf = sw_only.buffers[name]
        fill = np.full(buf.nbytes // 8, -7.25)                                           # zeros are written, not left
        api.check(lib.grt_host_to_device(device, buf.ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(fill.nbytes)))
    for fluxes in (True, False):
        out = run_chan(sw_only, gcols, gclouds, gaer, S, ALL, ncol, sec, inst, fluxes=fluxes)
        for key in ("channels", "tb", "radiances"):
            assert np.all(out[key] == 0.0) and not np.any(np.signbit(out[key])), key
    assert out["channels"].shape == (ncol, 4, 5, 2, 2)
    sw_only.destroy()
    go_lw.destroy()
    go_sw.destroy()


# ---- 4. the production arithmetic -------------------------------------------------------------------------------------------- #
def test_production_form_matches_the_model(bands, tables, oracle, lib, device):
    """fast = 3 on the 3 000-line band, four columns, all four sets, two draws, Gaussian channels every 100 cm-1 (FWHM 50
    cm-1) and three one-point channels, against the model on the oracle's tau within BOUNDS[3]["spectral_flux_rel"] x the
    row's largest model radiance x sum |W| / sum W.  The worst value met on an MI355X: 1.6e-3 of that bound, in both modes
    (DESIGN section 5)."""
    S = 2
    rel = BOUNDS[3]["spectral_flux_rel"]
    band = bands[0]
    cols = sky_columns(320, V1, n=4)
    ncol = len(cols)
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1, fast=3)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, CLOUD_SEED + 1, S)
    gclouds, keep_clouds = make(tables, cl)
    f = fields(ncol, V1 - 1, AEROSOL_SEED + 2)
    gaer, keep_aer = aerosols_of(f)
    sec = np.tile(np.array(STREAM_SECANTS + (1.0, 1.5, 2.0)), (ncol, 1))
    w_end = band.w0 + (band.nw - 1) * band.dw
    first, weights, centers = channels.gaussian(band.w0, band.dw, band.nw, np.arange(100.0, w_end + 1.0, 100.0), 50.0)
    points = [0, band.nw // 2 + 1, band.nw - 1]
    inst = Instrument(list(first) + points, weights + [np.ones(1)] * 3,
                      list(centers) + [band.w0 + p * band.dw for p in points])
    got = run_chan(pipe, gcols, gclouds, gaer, S, ALL, ncol, sec, inst)
    assert go_lw.last_launch()["fast"] == 3
    worst = 0.0
    for c, col in enumerate(cols):
        want = oracle_channel_sets(oracle, lib, band, col, tables, cl["lw_liquid"][c], cl["lw_ice"][c], cl["thickness"][c],
                                   AEROSOL_GRID, f[0][c], emis, sec[c], inst.first, inst.weights)
        for k, wk in enumerate(want):
            tol = rel * wk["largest"][..., None] * inst.ratio
            frac = float((np.abs(got["channels"][c, k] - wk["chan"]) / tol).max())
            worst = max(worst, frac)
            print("production column", c, "set", NAMES[k], "worst error as a fraction of its bound", frac)
    mode = "deterministic" if os.environ.get("GRT_DETERMINISTIC", "0") not in ("", "0") else "default"
    record("run_sky_channels." + mode, {"channels": {"worst_fraction_of_bound": worst, "relative_bound": rel}},
           file="parity_pipeline_production.json")
    assert worst <= 1.0, worst
    check_brightness(got, inst, band, "production")
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
