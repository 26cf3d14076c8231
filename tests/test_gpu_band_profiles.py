"""grt_pipeline_run_band_profiles: every level's flux and every layer's heating rate per wavenumber bin, clear sky and
all-sky, in the production (fused) and the materialised form, reference operation order (fast = 0) -- against the
oracle's level spectra integrated per bin on the CPU by an exactly rounded trapezoid, against grt_pipeline_run_profiles
and grt_pipeline_run_allsky_profiles bit for bit, against the call's own spectra, and in what it refuses.

Bounds, none of them measured here:
  bins and levels   1e-9 W m-2, check_levels' bound on the broadband level flux: a bin is a partial sum of that value
  heating rates     1e-12 of the bin's largest rate against the formula on the call's own levels, 1e-6 of it against the
                    formula on the oracle's levels (check_levels' margins)
  own spectra, additivity   TRAP_ULPS 2^-52 sum |f| dw, assert_trapezoid's bound
A pipeline of fewer than 2 levels cannot be created through the public interface (a gas-optics object needs two), so
that refusal is the one the suite cannot reach."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api, synthetic as syn
from pipeline_support import (LEVEL_KEYS, TRAP_ULPS, _deterministic, _sentinel, _setup, assert_trapezoid, block_edges,
                              cached, check_levels, cloud_columns, exact_trapezoid, make, oracle_allsky_levels, oracle_column)
from pipeline_support import bands, oracle_cache, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

BANDS = (("lw", True), ("sw", False))
SW_EDGES = np.array([0, 3, 127, 128, 129, 300, 383, 384, 385, 498, 499], np.int32)
CLOUD_SEED = 41


def bin_levels(w, edges, dw):
    """up, dn [bins][V]: the oracle's level spectra w["up"], w["dn"] [V][nw] integrated over each bin, exactly rounded"""
    pairs = list(zip(edges[:-1], edges[1:]))
    return tuple(np.array([[exact_trapezoid(r[a:b + 1], dw)[0] for r in w[k]] for a, b in pairs]) for k in ("up", "dn"))


def oracle_levels(cache, orc, lib, band, key, lw, c, col, surface, cloud=None, tables=None):
    emis, alb, solar = surface
    column = (col["p"].tobytes(), col["t"].tobytes(), float(col["mu0"]))
    if cloud is None:
        return cached(cache, ("clear", key, column),
                      lambda: oracle_column(orc, lib, band, col, lw, emis, alb, solar))
    return cached(cache, ("allsky", key, column),
                  lambda: oracle_allsky_levels(orc, lib, band, col, lw, tables, *cloud, emis, alb, solar))


def check_bins(got, c, s, key, col, want_up, want_dn):
    """check_levels for every bin of one column, set and band"""
    for b in range(want_up.shape[0]):
        one = {key + "_up": got[key + "_up"][:, s, b], key + "_down": got[key + "_down"][:, s, b],
               key + "_heating": got[key + "_heating"][:, s, b]}
        check_levels(one, c, key, col, want_up[b], want_dn[b])


class Case:
    """Two bands, a few columns, their clouds; pipelines of either form on them."""

    def __init__(self, bands, tables, device, V, ncol, seed, user_level=-1):
        self.bands, self.tables, self.device, self.V, self.ncol, self.user_level = bands, tables, device, V, ncol, user_level
        self.cols = [syn.profile(seed + c, V) for c in range(ncol)]
        for col, mu in zip(self.cols, (1.0, 0.5, 0.05, 1e-3)):
            col["mu0"] = mu
        self.go_lw, self.go_sw, self.emis, self.alb, self.solar = _setup(bands, device, V)
        self.surface = (self.emis, self.alb, self.solar)
        self.gcols, self.keep = api.make_columns(self.cols, MOL_ORDER, cfc_order=(0, 1))
        self.cl = cloud_columns(self.cols, tables, CLOUD_SEED)
        self.gclouds, self.keep_clouds = make(tables, self.cl)
        self.pipes = []

    def pipe(self, spectral, max_columns=None):
        p = api.Pipeline(self.go_lw, self.go_sw, max_columns or self.ncol, self.user_level, self.emis, self.alb, self.solar,
                         spectral=spectral)
        self.pipes.append(p)
        return p

    def cloud(self, key, c):
        return (self.cl[key + "_liquid"][c], self.cl[key + "_ice"][c], self.cl["thickness"][c])

    def close(self):
        for p in self.pipes:
            p.destroy()
        self.go_lw.destroy()
        self.go_sw.destroy()


# ---- the oracle ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("user_level", [5, -1])
@pytest.mark.parametrize("allsky", [False, True], ids=["clear", "allsky"])
@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
def test_bins_of_every_level_match_the_oracle(bands, tables, oracle_cache, oracle, lib, device, spectral, allsky, user_level):
    V, ncol = 16, 2
    k = Case(bands, tables, device, V, ncol, 300, user_level)
    pipe = k.pipe(spectral)
    edges = {"lw": block_edges(bands[0].nw), "sw": SW_EDGES}
    pipe.run_band_profiles(k.gcols, k.gclouds if allsky else None, edges["lw"], edges["sw"])
    got = pipe.band_profiles(ncol)
    sets = 2 if allsky else 1
    for (key, lw), band in zip(BANDS, bands):
        nb = edges[key].size - 1
        assert got[key + "_up"].shape == (ncol, sets, nb, V) and got[key + "_down"].shape == (ncol, sets, nb, V)
        assert got[key + "_heating"].shape == (ncol, sets, nb, V - 1)
        for c, col in enumerate(k.cols):
            for s in range(sets):
                w = oracle_levels(oracle_cache, oracle, lib, band, key, lw, c, col, k.surface,
                                  k.cloud(key, c) if s == 1 else None, tables)
                check_bins(got, c, s, key, col, *bin_levels(w, edges[key], band.dw))
        if allsky:
            assert np.max(np.abs(got[key + "_up"][:, 1] - got[key + "_up"][:, 0])) > 0.0, key
    k.close()


# ---- bit identities ------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
def test_one_bin_over_the_grid_is_run_profiles(bands, tables, lib, device, spectral):
    """Deterministic mode.  Production form: the single bin {0, n - 1} per band is run_profiles' level rows and heating
    rates bit for bit, and with clouds both sets are run_allsky_profiles'.  The materialised form's broadband rows come
    from another kernel (one workgroup per row, four waves) than its bins (the fused solvers' association): there the two
    are held to the trapezoid bound both keep to their common spectra, twice TRAP_ULPS 2^-52 sum |f| dw <= that of the
    value itself, all fluxes being of one sign."""
    V, ncol = 16, 3
    k = Case(bands, tables, device, V, ncol, 310, 7)
    pipe = k.pipe(spectral)
    whole = [np.array([0, b.nw - 1], np.int32) for b in bands]
    _deterministic(lib, True)
    try:
        pipe.run_profiles(k.gcols)
        clear = pipe.profiles(ncol)
        pipe.run_allsky_profiles(k.gcols, k.gclouds)
        both = pipe.allsky_profiles(ncol)
        pipe.run_band_profiles(k.gcols, None, *whole)
        one = pipe.band_profiles(ncol)
        pipe.run_band_profiles(k.gcols, k.gclouds, *whole)
        two = pipe.band_profiles(ncol)
    finally:
        _deterministic(lib, False)
    for name in LEVEL_KEYS + ("lw_heating", "sw_heating"):
        assert one[name].shape[1:3] == (1, 1) and two[name].shape[1:3] == (2, 1)
        pairs = [(one[name][:, 0, 0], clear[name]), (two[name][:, 0, 0], both[0][name]), (two[name][:, 1, 0], both[1][name])]
        for a, b in pairs:
            if not spectral:
                assert np.array_equal(a, b), name
            elif "heating" not in name:
                assert np.all(np.abs(a - b) <= 2 * TRAP_ULPS * 2.0 ** -52 * np.abs(b)), name
    assert np.max(np.abs(two["lw_up"][:, 1] - two["lw_up"][:, 0])) > 0.0
    k.close()


# ---- the call's own spectra, additivity ------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("allsky", [False, True], ids=["clear", "allsky"])
def test_bins_are_the_trapezoid_of_the_own_spectra(bands, tables, lib, device, allsky):
    """keep_spectra = 1: grt_pipeline_views shows the last pass (the all-sky one with clouds); every bin of that set
    against the exactly rounded trapezoid of those flux rows."""
    V, ncol = 16, 2
    k = Case(bands, tables, device, V, ncol, 320)
    pipe = k.pipe(True)
    edges = {"lw": block_edges(bands[0].nw), "sw": SW_EDGES}
    pipe.run_band_profiles(k.gcols, k.gclouds if allsky else None, edges["lw"], edges["sw"])
    got = pipe.band_profiles(ncol)
    s = 1 if allsky else 0
    for bi, ((key, lw), band) in enumerate(zip(BANDS, bands)):
        v = pipe.views(bi)
        rows = {"up": api.device_to_host(device, v["flux_up"], (ncol, V, band.nw)),
                "down": api.device_to_host(device, v["flux_down"], (ncol, V, band.nw))}
        e = edges[key]
        for d in ("up", "down"):
            for c in range(ncol):
                for b in range(e.size - 1):
                    for lev in range(V):
                        assert_trapezoid(got[f"{key}_{d}"][c, s, b, lev], rows[d][c, lev, e[b]:e[b + 1] + 1], band.dw,
                                         (key, d, c, b, lev))
    k.close()


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
def test_contiguous_bins_add_up_to_the_bin_over_their_union(bands, tables, lib, device, spectral):
    """Deterministic mode (two calls on one tau_gas).  Every part and the union keep assert_trapezoid's bound to the same
    spectra; the fluxes are of one sign, so sum |f| dw of the union is at least the sum of the parts, which stands in for
    it: a bound no wider than the one the spectra would give."""
    V, ncol = 16, 2
    k = Case(bands, tables, device, V, ncol, 330)
    pipe = k.pipe(spectral)
    fine = (np.array([0, 1, 2, 60, 127, 128, 129, 200, 256, 257, 390, 398, 399], np.int32),
            np.array([5, 6, 100, 127, 128, 129, 130, 255, 256, 257, 400, 497, 498, 499], np.int32))
    _deterministic(lib, True)
    try:
        pipe.run_band_profiles(k.gcols, k.gclouds, *fine)
        got = pipe.band_profiles(ncol)
        for lo, hi in ((0, 4), (2, 9), (3, 12)):
            his = [min(hi, e.size - 1) for e in fine]
            union = [np.array([e[lo], e[h]], np.int32) for e, h in zip(fine, his)]
            pipe.run_band_profiles(k.gcols, k.gclouds, *union)
            u = pipe.band_profiles(ncol)
            for (key, lw), h in zip(BANDS, his):
                for name in (key + "_up", key + "_down"):
                    parts = got[name][:, :, lo:h]
                    assert np.all(parts >= 0.0)
                    err = np.abs(parts.sum(axis=2) - u[name][:, :, 0])
                    assert np.all(err <= TRAP_ULPS * 2.0 ** -52 * parts.sum(axis=2)), (name, lo, hi)
    finally:
        _deterministic(lib, False)
    k.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------- #
def test_refused_inputs_launch_nothing(bands, tables, lib, device):
    V, ncol = 16, 2
    k = Case(bands, tables, device, V, ncol, 350)
    pipe = k.pipe(False)
    nl, ns = bands[0].nw, bands[1].nw
    sizes = {"levels": ncol * 2 * 2 * 8 * V, "heating": ncol * 2 * 8 * (V - 1)}
    bufs = {name: _sentinel(device, n) for name, n in sizes.items()}
    gcols = k.gcols

    def call(gcl, le, lnb, se, snb, levels=True, heating=True):
        lp = None if le is None else np.ascontiguousarray(le, np.int32)
        sp = None if se is None else np.ascontiguousarray(se, np.int32)
        return lib.grt_pipeline_run_band_profiles(
            pipe.p, C.byref(gcols), C.byref(gcl) if gcl is not None else None,
            None if lp is None else lp.ctypes.data_as(C.c_void_p), lnb,
            None if sp is None else sp.ctypes.data_as(C.c_void_p), snb,
            bufs["levels"].ptr if levels else None, bufs["heating"].ptr if heating else None)

    def refused(*a, **kw):
        with pytest.raises(api.GrtError) as e:
            api.check(call(*a, **kw))
        assert e.value.code == api.VALUE_ERR

    ok = np.array([0, 10, nl - 1])
    refused(None, ok, 2, None, 0, levels=False)                          # a NULL band_levels_dev
    refused(None, None, 0, None, 0)                                      # no bins at all
    refused(None, ok, 0, ok, 0)
    refused(None, ok, -1, None, 0)
    refused(None, None, 0, ok, -2)
    refused(None, None, 2, None, 0)                                      # bins without edges
    refused(None, np.array([0, 10, 10]), 2, None, 0)                     # not strictly increasing
    refused(None, np.array([0, 20, 10]), 2, None, 0)
    refused(None, np.array([-1, 10]), 1, None, 0)                        # outside 0 .. n - 1
    refused(None, np.array([0, nl]), 1, None, 0)
    refused(None, None, 0, np.array([0, ns]), 1)
    limit = pipe.band_profile_bin_limit()
    assert limit >= 65536 // (32 * V)
    # more bins in one block than the limit: one-interval bins from point 127 on all have a point in block 1 (128 .. 255)
    assert limit + 1 <= 129 and 127 + limit + 2 <= ns
    refused(None, None, 0, np.arange(127, 127 + limit + 2), limit + 1)
    gcols.ncol = 0
    refused(None, ok, 2, None, 0)
    refused(k.gclouds, ok, 2, None, 0)
    gcols.ncol = ncol + 1
    refused(None, ok, 2, None, 0)
    refused(k.gclouds, ok, 2, None, 0)
    gcols.ncol = ncol
    g, keep = make(tables, k.cl)
    g.num_liquid_bands = 0
    refused(g, ok, 2, None, 0)
    g, keep = make(tables, k.cl)
    g.num_ice_bands = g.num_liquid_bands - 1
    refused(g, ok, 2, None, 0)
    for field in ("thickness", "lw_liquid", "sw_ice", "liquid_band_lo"):
        g, keep = make(tables, k.cl)
        setattr(g, field, None)
        refused(g, ok, 2, None, 0)
    pipe.sync()
    for name, n in sizes.items():
        assert np.all(bufs[name].to_host((n,)) == -7.25), name
    # and the same call accepted, with and without the heating rates
    api.check(call(k.gclouds, ok, 2, None, 0, heating=False))
    pipe.sync()
    assert np.all(bufs["heating"].to_host((sizes["heating"],)) == -7.25)
    lv = bufs["levels"].to_host((sizes["levels"],))
    used = ncol * 2 * 2 * 2 * V
    assert np.all(np.isfinite(lv[:used])) and np.all(lv[:used] != -7.25) and np.all(lv[used:] == -7.25)
    api.check(call(k.gclouds, ok, 2, None, 0))
    pipe.sync()
    hr = bufs["heating"].to_host((sizes["heating"],))
    assert np.all(hr[:ncol * 2 * 2 * (V - 1)] != -7.25) and np.all(hr[ncol * 2 * 2 * (V - 1):] == -7.25)
    for b in bufs.values():
        b.free()
    k.close()


# ---- the bin limit --------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
def test_the_bin_limit_at_61_levels(bands, tables, oracle_cache, oracle, lib, device, spectral):
    """V = 61: edges 0, 1, .., limit -- `limit` one-interval bins in the first block -- pass and match the oracle; one more
    is refused."""
    V, ncol = 61, 1
    k = Case(bands, tables, device, V, ncol, 360)
    pipe = k.pipe(spectral)
    limit = pipe.band_profile_bin_limit()
    assert limit >= 65536 // (32 * V) == 33
    assert limit + 2 <= min(b.nw for b in bands)
    full = np.arange(limit + 1, dtype=np.int32)
    over = np.arange(limit + 2, dtype=np.int32)
    for edges in ((over, full), (full, over), (over, None), (None, over)):
        with pytest.raises(api.GrtError) as e:
            pipe.run_band_profiles(k.gcols, None, *edges)
        assert e.value.code == api.VALUE_ERR
    pipe.run_band_profiles(k.gcols, None, full, full)
    got = pipe.band_profiles(ncol)
    for (key, lw), band in zip(BANDS, bands):
        assert got[key + "_up"].shape == (ncol, 1, limit, V)
        w = oracle_levels(oracle_cache, oracle, lib, band, key, lw, 0, k.cols[0], k.surface)
        check_bins(got, 0, 0, key, k.cols[0], *bin_levels(w, full, band.dw))
    k.close()


# ---- edge cases ------------------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
def test_a_null_band_gives_no_rows_and_takes_no_room(bands, tables, lib, device, spectral):
    lwb, swb = bands
    V, ncol = 16, 2
    k = Case(bands, tables, device, V, ncol, 340)
    edges = (block_edges(lwb.nw), SW_EDGES)
    ref = k.pipe(spectral)
    _deterministic(lib, True)
    ref.run_band_profiles(k.gcols, k.gclouds, *edges)
    full = ref.band_profiles(ncol)
    # a band without bins is left out in the same way
    for have in (0, 1):
        e = [None, None]
        e[have] = edges[have]
        ref.run_band_profiles(k.gcols, k.gclouds, *e)
        part = ref.band_profiles(ncol)
        key, gone = ("lw", "sw")[have], ("lw", "sw")[1 - have]
        assert part[gone + "_up"].shape == (ncol, 2, 0, V) and part[gone + "_heating"].shape == (ncol, 2, 0, V - 1)
        for name in (key + "_up", key + "_down", key + "_heating"):
            assert np.max(np.abs(part[name] - full[name])) <= 1e-9, name
    for missing in (0, 1):
        have = 1 - missing
        go_lw, go_sw, emis, alb, solar = _setup((lwb if missing else None, swb if not missing else None), device, V)
        pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=spectral)
        e = [None, None]
        e[have] = edges[have]
        pipe.run_band_profiles(k.gcols, k.gclouds, *e)
        got = pipe.band_profiles(ncol)
        key, gone = ("lw", "sw")[have], ("lw", "sw")[missing]
        assert got[gone + "_up"].shape == (ncol, 2, 0, V) and got[gone + "_heating"].shape == (ncol, 2, 0, V - 1)
        for name in (key + "_up", key + "_down", key + "_heating"):
            assert got[name].shape == full[name].shape
            assert np.max(np.abs(got[name] - full[name])) <= 1e-9, name
        bad = [None, None]
        bad[missing] = np.array([0, 1], np.int32)
        with pytest.raises(api.GrtError) as err:
            pipe.run_band_profiles(k.gcols, None, *bad)
        assert err.value.code == api.VALUE_ERR
        pipe.destroy()
        for g in (go_lw, go_sw):
            if g is not None:
                g.destroy()
    _deterministic(lib, False)
    k.close()


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
def test_a_full_batch_agrees_with_its_columns_run_alone(bands, tables, lib, device, spectral):
    """max_columns columns in one call against each of them alone in the same pipeline: every bin within 1e-9 W m-2 (both
    keep that bound to the oracle), the heating rates within 1e-6 of the bin's largest."""
    V, ncol = 16, 4
    k = Case(bands, tables, device, V, ncol, 370)
    pipe = k.pipe(spectral)
    edges = (block_edges(bands[0].nw), SW_EDGES)
    _deterministic(lib, True)
    try:
        pipe.run_band_profiles(k.gcols, k.gclouds, *edges)
        whole = pipe.band_profiles(ncol)
        for c in range(ncol):
            g1, keep1 = api.make_columns([k.cols[c]], MOL_ORDER, cfc_order=(0, 1))
            gc1, keepc1 = make(tables, {name: v[c:c + 1] for name, v in k.cl.items()})
            pipe.run_band_profiles(g1, gc1, *edges)
            one = pipe.band_profiles(1)
            for name in LEVEL_KEYS:
                assert np.max(np.abs(one[name][0] - whole[name][c])) <= 1e-9, (name, c)
            for name in ("lw_heating", "sw_heating"):
                hmax = np.abs(whole[name][c]).max(axis=-1, keepdims=True)
                assert np.all(np.abs(one[name][0] - whole[name][c]) <= 1e-6 * hmax), (name, c)
    finally:
        _deterministic(lib, False)
    assert len({whole["lw_up"][c].tobytes() for c in range(ncol)}) == ncol          # the columns differ
    k.close()
