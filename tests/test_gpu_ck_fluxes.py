"""grt_pipeline_run_ck_fluxes on the device against ck_flux_model.py.

Sums: points, class weights, class sums of tau and of the data rows (emissivity, solar curve, albedos) and of the Rayleigh
row BIT FOR BIT against the model applied to the tau_gas the pipeline shows afterwards.  The Planck rows within a bound
derived here, not measured: per class sum |got - want| <= (2 e^x/(e^x - 1) + m + 4) 2^-52 sum |w_i B_i|, x the smallest
c2 v/T of the case and m the bin's points -- one unit in the last place for each of the device's and numpy's exp, amplified
by e^x/(e^x - 1) in B, plus the roundings of B's other operations and of the sum.
Solve: the device's up, down against the model's solve of the device's own sums (the shortwave: the oracle) within
pipeline_support.LEVEL_TOL of the column's largest class flux; bin sums bit for bit the sequential sum of the device's
class fluxes.  One point per class: the oracle's line-by-line fluxes, point by point, and grt_pipeline_run_band_profiles'
bins, within the same margin of the column's largest flux.

The conditions on the inputs are asserted on the CPU from the model's map before the device is compared.  Three populated
classes per bin, an empty class and a class of a single point cannot all hold where K = 2 or a bin has two points (the
"pairs" bins, n = 2): a bin of more than two points must populate min(3, K, its points) classes, the bins of a column
together that many in any case, and the empty class is asked for where K > 2.
The class edges are cut between the sorted key values of column 0 (geometric means of neighbours: no key lies within
rounding of an edge), so that the first two distinct values fall into classes of their own and the top class stays empty."""
import ctypes as C

import numpy as np
import pytest

import ck_flux_model as ck
from grtcode_amd import api
from kdist_correlated_model import KEY_ROW, KEY_SUM, class_map, mapped_rows
from kdist_model import same_bits
from lw_jacobian_model import PLANCK_C2
from pipeline_support import (LEVEL_TOL, LW_W0, MU0, SW_W0, _deterministic, _sentinel, _setup, cached, columns, make_shape_bands,
                              oracle_cache, oracle_column, surface)  # noqa: F401  (oracle_cache: a module fixture)
from scenario import MOL_ORDER
from test_gpu_kdist_correlated import SOLVER_TAGS, bin_sets, upload

pytestmark = pytest.mark.gpu

NS = (2, 3, 64, 65, 257)
shape_bands = make_shape_bands(NS, LW_W0, SW_W0)
NAMES = ("points", "weight", "tau", "source", "up", "down", "bin_up", "bin_down")


class Case:
    def __init__(self, bands, device, V, ncol, fast=0, spectral=True, seed=1, mu=None, lw_only=False, isothermal=None):
        self.bands, self.device, self.V, self.L, self.ncol = bands, device, V, V - 1, ncol
        self.cols = columns(V)[:ncol]
        for c, m in zip(self.cols, mu or ()):
            c["mu0"] = m
        if isothermal is not None:
            for c in self.cols:
                c["t"], c["t_layer"], c["t_surf"] = np.full(V, isothermal), np.full(V - 1, isothermal), float(isothermal)
        use = (bands[0], None) if lw_only else bands
        self.go_lw, self.go_sw, _e, _a, self.solar = _setup(use, device, V, fast=fast)
        self.emis, self.alb = surface(bands[0].nw, seed)
        if isothermal is not None:
            self.emis = np.ones(bands[0].nw)
        if lw_only:
            self.alb = None
        self.gcols, self.keep = api.make_columns(self.cols, MOL_ORDER, cfc_order=(0, 1))
        self.spectral = spectral
        self.pipes = []
        self.pipe = self.make()

    def make(self, max_columns=None):
        p = api.Pipeline(self.go_lw, self.go_sw, max_columns or self.ncol, -1, self.emis, self.alb, self.solar,
                         spectral=self.spectral)
        self.pipes.append(p)
        return p

    def tau_gas(self, pipe, bi, ncol=None):
        return api.device_to_host(self.device, pipe.views(bi)["tau_gas"], (ncol or self.ncol, self.L, self.bands[bi].nw)).copy()

    def rows(self, bi, cols=None):
        """the rows whose class sums are the sources"""
        b = self.bands[bi]
        w = ck.wavenumbers(b.w0, b.dw, b.nw)
        cols = self.cols if cols is None else cols
        if bi == 0:
            return ck.lw_rows(cols, w, self.emis)
        return ck.sw_rows(len(cols), w, self.solar, self.alb, self.alb)

    def close(self):
        for p in self.pipes:
            p.destroy()
        for go in (self.go_lw, self.go_sw):
            if go is not None:
                go.destroy()


def edges_between(key, K):
    """K - 1 class edges cut between the sorted distinct values of key: the first two values in classes of their own, the
    top class empty (K > 2)"""
    k = np.unique(key[key > 0.0])
    mids = np.sqrt(k[:-1] * k[1:])
    mids = mids[(mids > k[:-1]) & (mids < k[1:])]
    if K == 2:
        return mids[mids.size // 2:mids.size // 2 + 1]
    take = min(K - 2, mids.size)
    idx = np.unique(np.concatenate(([0, 1][:take], np.linspace(0, mids.size - 1, take).astype(int))))[:take]
    chosen = mids[np.sort(idx)]
    above = k[-1] * 1e3 * np.arange(1.0, K - chosen.size)          # (beyond every column's key)
    return np.concatenate((chosen, above))


def assert_conditions(m, edges, K):
    """what every case of the first group must have (module docstring)"""
    m = m.astype(np.int64)
    single = False
    for c in range(m.shape[0]):
        for lo, hi in zip(edges[:-1], edges[1:]):
            counts = np.bincount(m[c, lo:hi + 1], minlength=K)
            if c == 0 and hi - lo + 1 > 2:
                assert np.count_nonzero(counts) >= min(3, K, hi - lo + 1), (lo, hi, counts)
            single = single or bool(np.any(counts == 1))
            assert K == 2 or np.any(counts == 0)
    assert single, "no class of a single point"
    assert np.count_nonzero(np.bincount(m[0, edges[0]:edges[-1] + 1], minlength=K)) >= min(3, K, edges[-1] - edges[0] + 1)


def planck_bound(case, rows, m, edges, K, dw):
    """per (column, Planck row, bin, class): (2 e^x/(e^x - 1) + points of the bin + 4) 2^-52 sum |w_i B_i|"""
    b = case.bands[0]
    temps = np.concatenate([np.concatenate((c["t"], c["t_layer"], [c["t_surf"]])) for c in case.cols])
    x = PLANCK_C2 * b.w0 / temps.max()
    amp = 2.0 * np.exp(x) / np.expm1(x)
    mag = mapped_rows(np.abs(rows), m, dw, edges, K)[2]
    pts = np.array([hi - lo + 1 for lo, hi in zip(edges[:-1], edges[1:])], dtype=np.float64)
    return (amp + pts[None, None, :, None] + 4.0) * 2.0 ** -52 * mag


def assert_sums(case, got, bi, m, edges, K, pipe=None, cols=None):
    """the device's sums of one band against the model on the tau_gas the pipeline shows"""
    b = case.bands[bi]
    ncol = m.shape[0]
    tau = case.tau_gas(pipe or case.pipe, bi, ncol)
    want = mapped_rows(tau, m, b.dw, edges, K)
    assert got["points"].dtype == np.int32 and np.array_equal(got["points"], want[0])
    assert same_bits(got["weight"], want[1]) and same_bits(got["tau"], want[2])
    rows = case.rows(bi, cols)
    src = ck.source_sums(rows, m, b.dw, edges, K)
    V = case.V
    if bi == 1:
        assert same_bits(got["source"], src), "Rayleigh, solar, albedo rows"
        return
    assert same_bits(got["source"][:, 2 * V], src[:, 2 * V]), "emissivity row"
    bound = planck_bound(case, rows[:, :2 * V], m, edges, K, b.dw)
    err = np.abs(got["source"][:, :2 * V] - src[:, :2 * V])
    worst = np.max(np.where(bound > 0.0, err / np.where(bound > 0.0, bound, 1.0), 0.0))
    print(f"Planck rows: worst error / bound = {worst:.3f}")
    assert np.all(err <= bound), worst


def assert_solve(case, orc, got, bi, cols=None):
    """the device's fluxes against the model's solve of the device's own sums, and the bin sums of its own fluxes"""
    cols = case.cols if cols is None else cols
    V = case.V
    for c, col in enumerate(cols):
        if bi == 0:
            up, dn = ck.lw_solve(got["weight"][c], got["tau"][c], got["source"][c])
        else:
            up, dn = ck.sw_solve(orc, got["weight"][c], got["tau"][c], got["source"][c], ck.air_columns(col["p"]), col["mu0"],
                                 col["tsi"])
        empty = np.broadcast_to(got["weight"][c] == 0.0, up.shape)
        zero = np.zeros(up.shape)
        for name, have, want in (("up", got["up"][c], up), ("down", got["down"][c], dn)):
            assert same_bits(have[empty], zero[empty]), (name, c, "empty classes")
            if bi == 1 and not col["mu0"] > 0.0:
                assert same_bits(have, zero), (name, c, "night")
                continue
            top = max(np.abs(up).max(), np.abs(dn).max())
            assert top > 0.0
            err = np.abs(have - want).max()
            assert err <= LEVEL_TOL * top, (name, bi, c, err, top)
    assert got["up"].shape == (len(cols), V) + got["weight"].shape[1:]
    assert same_bits(got["bin_up"], ck.bin_sums(got["up"])) and same_bits(got["bin_down"], ck.bin_sums(got["down"]))


# ---- 1, 2. sums and solve at edge shapes ------------------------------------------------------------------------------------ #
# n, K, V, columns, bins; columns x bins x K: 2, 192, 12, 65 and 64 (below a solver workgroup of 128), 378, 128 (on it), 130
# (just above), 4096, 2313, 3072, 195
SHAPES = [(2, 2, 2, 1, "whole"), (2, 64, 5, 3, "pairs"), (3, 2, 5, 3, "pairs"), (3, 65, 2, 1, "whole"),
          (64, 64, 2, 1, "whole"), (64, 2, 5, 3, "pairs"), (65, 2, 2, 1, "pairs"), (65, 65, 2, 2, "whole"),
          (65, 64, 5, 1, "pairs"), (65, 257, 2, 3, "three"), (257, 1024, 2, 1, "three"), (257, 65, 5, 3, "whole")]


@pytest.mark.parametrize("shape", SHAPES, ids=["n%d-K%d-V%d-C%d-%s" % s for s in SHAPES])
def test_sums_equal_the_model_and_the_solve_follows_from_them(shape_bands, oracle, lib, device, shape):
    n, K, V, ncol, bins = shape
    sets = bin_sets(n)
    edges = np.array(sets[bins], dtype=np.int32)
    mu = list(MU0[:ncol])
    if ncol == 3:
        mu[1] = 0.0 if K == 64 else -0.25          # a night column
    k = Case(shape_bands[n], device, V, ncol, seed=n + K, mu=mu)
    try:
        # the keys: the columns' vertical optical depth (longwave), the bottom layer's (shortwave); a first run shows tau_gas
        keys = (("sum",), ("layer", V - 2))
        k.pipe.run_ck_fluxes(k.gcols, np.logspace(-6.0, 2.0, K - 1), lw_edges=edges, sw_edges=edges, lw_key=keys[0],
                             sw_key=keys[1])
        k.pipe.sync()
        key0 = [class_key(k.tau_gas(k.pipe, bi), keys[bi])[0] for bi in range(2)]
        for bi, name in enumerate(("lw", "sw")):
            ce = edges_between(key0[bi], K)
            assert ce.size == K - 1 and np.all(np.diff(ce) > 0.0)
            kw = dict(lw_edges=edges, lw_key=keys[0]) if bi == 0 else dict(sw_edges=edges, sw_key=keys[1])
            k.pipe.run_ck_fluxes(k.gcols, ce, keep_map=True, **kw)
            got = k.pipe.ck_fluxes(ncol)[name]
            tau = k.tau_gas(k.pipe, bi)
            m = class_map(tau, KEY_SUM if bi == 0 else KEY_ROW, ce, V - 2)
            assert_conditions(m, edges, K)
            assert got["map"].dtype == np.uint16 and np.array_equal(got["map"], m)
            assert_sums(k, got, bi, m, edges, K)
            assert_solve(k, oracle, got, bi)
    finally:
        k.close()


def class_key(tau, spec):
    return tau.sum(axis=1) if spec[0] == "sum" else tau[:, spec[1]]


# ---- 3. one point per class is the line-by-line solve ----------------------------------------------------------------------- #
def identity_map(device, ncol, n):
    return upload(device, np.tile(np.arange(n, dtype=np.uint16), (ncol, 1)))


def line_by_line(orc, band, col, lw, tau_gas, emis, alb, solar):
    """the oracle's solvers on a given tau_gas [L][n] (the production form's own)"""
    if lw:
        return orc.lw_fluxes(band.w0, band.dw, col["t_surf"], col["t_layer"], col["t"], tau_gas, np.zeros_like(tau_gas), emis)
    tr, om_r, g_r = orc.rayleigh(tau_gas.shape[0], col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    tau, omega, g = orc.add_optics([tau_gas, tr], [z, om_r], [z, g_r])
    return orc.sw_fluxes(omega, g, tau, col["mu0"], 0.5, alb, alb, col["tsi"], solar)


@pytest.mark.parametrize("n,fast", [(65, 0), (257, 0), (65, 3)])
def test_one_point_per_class_is_the_line_by_line_solve(shape_bands, oracle, oracle_cache, lib, device, n, fast):
    V, ncol = 5, 2
    k = Case(shape_bands[n], device, V, ncol, fast=fast, spectral=fast == 0, seed=40 + n)
    mbuf = identity_map(device, ncol, n)
    try:
        for bins in ("whole", "pairs"):
            edges = np.array(bin_sets(n)[bins], dtype=np.int32)
            k.pipe.run_ck_fluxes(k.gcols, n, lw_edges=edges, sw_edges=edges, lw_map=mbuf, sw_map=mbuf)
            got = k.pipe.ck_fluxes(ncol)
            taus = [k.tau_gas(k.pipe, bi) for bi in range(2)]
            k.pipe.run_band_profiles(k.gcols, lw_edges=edges, sw_edges=edges)
            prof = k.pipe.band_profiles(ncol)
            for bi, name in enumerate(("lw", "sw")):
                band = k.bands[bi]
                for c, col in enumerate(k.cols):
                    if fast == 0:
                        o = cached(oracle_cache, (n, bi, c), lambda: oracle_column(
                            oracle, lib, band, col, bi == 0, k.emis, k.alb, k.solar))
                        want_up, want_dn = o["up"], o["dn"]
                    else:
                        want_up, want_dn = line_by_line(oracle, band, col, bi == 0, taus[bi][c], k.emis, k.alb, k.solar)
                    top = max(np.abs(want_up).max(), np.abs(want_dn).max())
                    for b, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
                        W = got[name]["weight"][c, b, lo:hi + 1]
                        assert np.all(W > 0.0) and np.all(got[name]["points"][c, b, lo:hi + 1] == 1)
                        for have, want in ((got[name]["up"], want_up), (got[name]["down"], want_dn)):
                            err = np.abs(have[c, :, b, lo:hi + 1] / W - want[:, lo:hi + 1]).max()
                            assert err <= LEVEL_TOL * top, (name, bins, c, b, err, top)
                    ptop = max(np.abs(prof[name + "_up"][c, 0]).max(), np.abs(prof[name + "_down"][c, 0]).max())
                    for mine, theirs in (("bin_up", "_up"), ("bin_down", "_down")):
                        err = np.abs(got[name][mine][c].T - prof[name + theirs][c, 0]).max()
                        assert err <= LEVEL_TOL * ptop, (name, bins, c, mine, err, ptop)
    finally:
        mbuf.free()
        k.close()


# ---- 4. an isothermal column closes for any map --------------------------------------------------------------------------- #
def test_an_isothermal_column_closes_for_any_map(shape_bands, lib, device):
    n, V, ncol, K = 257, 5, 2, 4
    k = Case(shape_bands[n], device, V, ncol, lw_only=True, isothermal=250.0)
    edges = np.array(bin_sets(n)["three"], dtype=np.int32)
    scrambled = upload(device, np.random.default_rng(4).integers(0, K, (ncol, n)).astype(np.uint16))
    try:
        k.pipe.run_band_profiles(k.gcols, lw_edges=edges)
        want = k.pipe.band_profiles(ncol)["lw_up"][:, 0]                  # [ncol][bins][V]
        top = np.abs(want).max(axis=(1, 2))
        k.pipe.run_ck_fluxes(k.gcols, np.logspace(-3.0, 1.0, K - 1), lw_edges=edges)
        k.pipe.sync()
        ce = np.quantile(k.tau_gas(k.pipe, 0).sum(axis=1)[0], (0.25, 0.5, 0.75))       # the quartiles of column 0's key
        assert np.all(np.diff(ce) > 0.0)
        for kw in (dict(lw_key=("sum",)), dict(lw_map=scrambled)):
            k.pipe.run_ck_fluxes(k.gcols, ce, lw_edges=edges, **kw)
            got = k.pipe.ck_fluxes(ncol)["lw"]
            assert np.count_nonzero(got["points"].sum(axis=(0, 1))) >= 3
            err = np.abs(got["bin_up"].transpose(0, 2, 1) - want).max(axis=(1, 2))
            assert np.all(err <= LEVEL_TOL * top), (sorted(kw), err, top)
    finally:
        scrambled.free()
        k.close()


# ---- raw calls ------------------------------------------------------------------------------------------------------------ #
FIELDS = ("points_dev", "weight_dev", "tau_dev", "source_dev", "flux_up_dev", "flux_down_dev", "bin_up_dev", "bin_down_dev")


def counts(ncol, V, nb, K, lw=True):
    R = 2 * V + 1 if lw else 4
    c = ncol * nb * K
    return dict(zip(FIELDS, (c, c, c * (V - 1), c * R, c * V, c * V, ncol * nb * V, ncol * nb * V)))


def raw_band(band, edges, key=(api.KDIST_KEY_SUM, 0), map_dev=None, given=None, outs=None):
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.int32)
    band.edges = None if e is None else e.ctypes.data_as(api.c_int_p)
    band.num_bins = 0 if e is None else e.size - 1
    band.key.kind, band.key.layer = key
    band.key.map_dev = map_dev
    band.map_given_dev = given
    for f in FIELDS:
        setattr(band, f, (outs or {}).get(f))
    return e


def raw_call(lib, pipe, gcols, K, ce, lw=None, sw=None, null_ck=False):
    gk = api.GrtCkFluxes()
    e = None if ce is None else np.ascontiguousarray(ce, dtype=np.float64)
    gk.num_classes, gk.class_edges = K, None if e is None else e.ctypes.data_as(api.c_double_p)
    keep = [raw_band(gk.lw, **(lw or dict(edges=None))), raw_band(gk.sw, **(sw or dict(edges=None)))]
    rc = lib.grt_pipeline_run_ck_fluxes(pipe.p, C.byref(gcols), None if null_ck else C.byref(gk))
    del keep
    return rc


class Frames:
    """sentinel-framed device outputs of one band"""
    def __init__(self, device, sizes, frame=256):
        self.sizes, self.frame = sizes, frame
        # (points are ints: their count in doubles, rounded up)
        self.doubles = {f: (c + 1) // 2 if f == "points_dev" else c for f, c in sizes.items()}
        self.bufs = {f: _sentinel(device, d + 2 * frame) for f, d in self.doubles.items()}

    def ptrs(self, only=None):
        return {f: C.c_void_p(b.ptr.value + 8 * self.frame) for f, b in self.bufs.items() if only is None or f in only}

    def read(self, f, shape):
        h = self.bufs[f].to_host(self.doubles[f] + 2 * self.frame)
        assert np.all(h[:self.frame] == -7.25) and np.all(h[self.frame + self.doubles[f]:] == -7.25), f
        body = h[self.frame:self.frame + self.doubles[f]]
        if f == "points_dev":
            return body.view(np.int32)[:self.sizes[f]].reshape(shape).copy()
        return body.reshape(shape).copy()

    def untouched(self):
        return all(np.all(b.to_host(b.nbytes // 8) == -7.25) for b in self.bufs.values())

    def free(self):
        for b in self.bufs.values():
            b.free()


def shapes(ncol, V, nb, K, lw=True):
    R = 2 * V + 1 if lw else 4
    return dict(zip(FIELDS, ((ncol, nb, K), (ncol, nb, K), (ncol, V - 1, nb, K), (ncol, R, nb, K), (ncol, V, nb, K),
                             (ncol, V, nb, K), (ncol, V, nb), (ncol, V, nb))))


def read_all(frames, ncol, V, nb, K, lw=True):
    sh = shapes(ncol, V, nb, K, lw)
    return {name: frames.read(f, sh[f]) for name, f in zip(NAMES, FIELDS)}


@pytest.fixture(scope="module")
def case65(shape_bands, device):
    """65 points, five levels, three columns (the last a night column), the reference's order: shared by the cases that
    leave it as they found it"""
    k = Case(shape_bands[65], device, 5, 3, seed=65, mu=(1.0, 0.05, -0.25))
    yield k
    k.close()


CE8 = np.logspace(-4.0, 1.0, 7)


# ---- 5. keys, given maps and bad entries ---------------------------------------------------------------------------------- #
def test_a_kept_map_given_back_yields_the_same_bits(case65, oracle, lib, device):
    k, K, ncol = case65, 8, 3
    edges = np.array(bin_sets(65)["three"], dtype=np.int32)
    _deterministic(lib, True)
    try:
        k.pipe.run_kdist_correlated(k.gcols, CE8, lw_edges=edges, sw_edges=edges, lw_key=("layer", 1), sw_key=("sum",),
                                    keep_map=True)
        kept = k.pipe.kdist_correlated(ncol)
        k.pipe.run_ck_fluxes(k.gcols, CE8, lw_edges=edges, sw_edges=edges, lw_key=("layer", 1), sw_key=("sum",), keep_map=True)
        keyed = k.pipe.ck_fluxes(ncol)
        k.pipe.run_ck_fluxes(k.gcols, K, lw_edges=edges, sw_edges=edges, lw_map=k.pipe.buffers["kdist_corr.lw.map"],
                             sw_map=k.pipe.buffers["kdist_corr.sw.map"], keep_map=True)
        given = k.pipe.ck_fluxes(ncol)
    finally:
        _deterministic(lib, False)
    for bi, name in enumerate(("lw", "sw")):
        tau = k.tau_gas(k.pipe, bi)
        m = class_map(tau, KEY_ROW if bi == 0 else KEY_SUM, CE8, 1)
        assert np.array_equal(keyed[name]["map"], m) and np.array_equal(kept[name]["map"], m) and given[name]["map"] is None
        for x in ("points", "weight", "tau"):
            assert same_bits(keyed[name][x].astype(np.float64), kept[name][x].astype(np.float64)), (name, x)
        for x in NAMES:
            assert same_bits(given[name][x].astype(np.float64), keyed[name][x].astype(np.float64)), (name, x)
        assert_sums(k, given[name], bi, m, edges, K)
        assert_solve(k, oracle, given[name], bi)


def test_given_map_entries_that_name_no_class_are_counted_nowhere_and_write_nowhere(case65, oracle, lib, device):
    k, K, ncol, n, V = case65, 8, 3, 65, 5
    edges = np.array([0, 31, 64], dtype=np.int32)
    m = np.random.default_rng(12).integers(0, K - 1, (ncol, n)).astype(np.uint16)       # (class K - 1 stays empty)
    bad_at = [(0, 7), (0, 31), (1, 0), (2, 64), (2, 40)]
    for j, (c, i) in enumerate(bad_at):
        m[c, i] = (K, K + 1, 0xffff, 1024, 300)[j]
    mbuf = upload(device, m)
    map_sent = _sentinel(device, ncol * n // 4 + 64)
    frames = [Frames(device, counts(ncol, V, 2, K, lw)) for lw in (True, False)]
    try:
        rc = raw_call(lib, k.pipe, k.gcols, K, None,
                      lw=dict(edges=edges, given=mbuf.ptr, map_dev=map_sent.ptr, outs=frames[0].ptrs()),
                      sw=dict(edges=edges, given=mbuf.ptr, map_dev=map_sent.ptr, outs=frames[1].ptrs()))
        api.check(rc)
        k.pipe.sync()
        assert np.all(map_sent.to_host(map_sent.nbytes // 8) == -7.25), "map_dev is written though a map was given"
        for bi in range(2):
            got = read_all(frames[bi], ncol, V, 2, K, bi == 0)
            # (point 31 is an edge of both bins, and lost to both)
            assert got["points"].sum() == ncol * (32 + 34) - 6
            assert_sums(k, got, bi, m, edges, K)
            assert_solve(k, oracle, got, bi)
    finally:
        for b in [mbuf, map_sent] + frames:
            b.free()


# ---- 6. determinism and independence -------------------------------------------------------------------------------------- #
def test_the_same_bits_every_time_alone_in_a_batch_and_with_fewer_outputs(case65, lib, device):
    k, K, ncol, V = case65, 8, 3, 5
    edges = np.array(bin_sets(65)["three"], dtype=np.int32)
    wide = k.make(max_columns=5)
    one, _keep = api.make_columns(k.cols[1:2], MOL_ORDER, cfc_order=(0, 1))
    frames = [Frames(device, counts(ncol, V, 3, K, lw)) for lw in (True, False)]
    kw = dict(lw_edges=edges, sw_edges=edges, lw_key=("sum",), sw_key=("layer", 3))
    try:
        # the default mode: whatever tau_gas a run made, its outputs are the model's of that tau_gas
        k.pipe.run_ck_fluxes(k.gcols, CE8, keep_map=True, **kw)
        loose = k.pipe.ck_fluxes(ncol)
        for bi, name in enumerate(("lw", "sw")):
            tau = k.tau_gas(k.pipe, bi)
            assert_sums(k, loose[name], bi, class_map(tau, KEY_SUM if bi == 0 else KEY_ROW, CE8, 3), edges, K)
        _deterministic(lib, True)
        try:
            wide.run_ck_fluxes(k.gcols, CE8, **kw)
            first = wide.ck_fluxes(ncol)
            wide.run_ck_fluxes(k.gcols, CE8, **kw)
            again = wide.ck_fluxes(ncol)
            k.pipe.run_ck_fluxes(k.gcols, CE8, **kw)
            narrow = k.pipe.ck_fluxes(ncol)
            wide.run_ck_fluxes(one, CE8, **kw)
            alone = wide.ck_fluxes(1)
            # each optional output alone beside the fluxes, then the fluxes alone
            for only in FIELDS[:4] + ("bins", None):
                for f in frames:
                    f.free()
                frames = [Frames(device, counts(ncol, V, 3, K, lw)) for lw in (True, False)]
                want = {"flux_up_dev", "flux_down_dev"} | ({"bin_up_dev", "bin_down_dev"} if only == "bins" else {only})
                api.check(raw_call(lib, k.pipe, k.gcols, K, CE8,
                                   lw=dict(edges=edges, outs=frames[0].ptrs(want)),
                                   sw=dict(edges=edges, key=(api.KDIST_KEY_ROW, 3), outs=frames[1].ptrs(want))))
                k.pipe.sync()
                for bi, name in enumerate(("lw", "sw")):
                    sh = shapes(ncol, V, 3, K, bi == 0)
                    for x, f in zip(NAMES, FIELDS):
                        if f in want:
                            assert same_bits(frames[bi].read(f, sh[f]).astype(np.float64),
                                             first[name][x].astype(np.float64)), (only, name, x)
                        else:
                            assert np.all(frames[bi].bufs[f].to_host(frames[bi].bufs[f].nbytes // 8) == -7.25), (only, name, x)
        finally:
            _deterministic(lib, False)
        for name in ("lw", "sw"):
            for x in NAMES:
                f64 = [r[name][x].astype(np.float64) for r in (first, again, narrow, alone)]
                assert same_bits(f64[1], f64[0]), (name, x, "the same call again")
                assert same_bits(f64[2], f64[0]), (name, x, "a pipeline of exactly these columns")
                assert same_bits(f64[3][0], f64[0][1]), (name, x, "column 1 alone")
    finally:
        for f in frames:
            f.free()


# ---- 7. what runs and what is refused --------------------------------------------------------------------------------------- #
CK_TAGS = (api.TAG_CK_SOURCES, api.TAG_CK_LW, api.TAG_CK_SW, api.TAG_KDIST_MAP, api.TAG_KDIST_MAPPED)


def launches(tags):
    return {t: api.profile_read(t)[1] for t in tags}


def test_what_runs(case65, lib, device):
    k, K = case65, 8
    edges = np.array(bin_sets(65)["three"], dtype=np.int32)
    idle = SOLVER_TAGS + (api.TAG_KDIST,)
    mbuf = upload(device, np.zeros((3, 65), dtype=np.uint16))
    api.profile_enable(True)
    api.profile_read(api.TAG_KDIST_MAP, reset=True)
    try:
        k.pipe.run_ck_fluxes(k.gcols, CE8, lw_edges=edges, sw_edges=edges)
        k.pipe.sync()
        assert launches(CK_TAGS) == dict(zip(CK_TAGS, (2, 1, 1, 2, 2)))
        assert not any(launches(idle).values()), launches(idle)
        assert api.profile_read(api.TAG_GAS_LW)[1] >= 1 and api.profile_read(api.TAG_GAS_SW)[1] >= 1
        # a given map: no map kernel; longwave bins alone: the shortwave band is not computed
        api.profile_read(api.TAG_KDIST_MAP, reset=True)
        k.pipe.run_ck_fluxes(k.gcols, K, lw_edges=edges, lw_map=mbuf)
        k.pipe.sync()
        assert launches(CK_TAGS) == dict(zip(CK_TAGS, (1, 1, 0, 0, 1)))
        quiet = idle + (api.TAG_GAS_SW, api.TAG_FAR_SW)
        assert not any(launches(quiet).values()), launches(quiet)
        assert api.profile_read(api.TAG_GAS_LW)[1] >= 1
    finally:
        api.profile_enable(False)
        mbuf.free()


def test_refused_calls_and_the_wrong_lane(shape_bands, lib, device):
    n, V, ncol, K = 65, 5, 2, 8
    k = Case(shape_bands[n], device, V, ncol, lw_only=True)
    narrow = k.make(max_columns=1)
    edges = np.array([0, 20, 64], dtype=np.int32)
    frames = Frames(device, counts(ncol, V, 2, K))
    map_sent = _sentinel(device, ncol * n // 4 + 64)
    mbuf = upload(device, np.zeros((ncol, n), dtype=np.uint16))
    none, _keep = api.make_columns(k.cols, MOL_ORDER, cfc_order=(0, 1))
    none.ncol = 0

    def run(pipe=None, gcols=None, ce=CE8, classes=K, lw=edges, sw=None, key=(api.KDIST_KEY_SUM, 0), given=None, drop=(),
            null_ck=False):
        outs = {f: p for f, p in frames.ptrs().items() if f not in drop}
        return raw_call(lib, pipe or k.pipe, gcols if gcols is not None else k.gcols, classes, ce,
                        lw=dict(edges=lw, key=key, map_dev=map_sent.ptr, given=given, outs=outs),
                        sw=None if sw is None else dict(edges=sw, outs=outs), null_ck=null_ck)

    cases = {
        "NULL ck": lambda: run(null_ck=True),
        "K = 1": lambda: run(classes=1, ce=np.array([])),
        "K = 1025, a map given": lambda: run(classes=1025, ce=None, given=mbuf.ptr),
        "class edges equal": lambda: run(ce=np.array([0.1] * 7)),
        "class edge NaN": lambda: run(ce=np.where(np.arange(7) == 3, np.nan, CE8)),
        "NULL class edges and no map": lambda: run(ce=None),
        "key kind 2": lambda: run(key=(2, 0)),
        "layer -1": lambda: run(key=(api.KDIST_KEY_ROW, -1)),
        "layer L": lambda: run(key=(api.KDIST_KEY_ROW, V - 1)),
        "no bins in either band": lambda: run(lw=None),
        "bins for a band the pipeline lacks": lambda: run(sw=[0, 5, 9]),
        "edges beyond the grid": lambda: run(lw=[0, 5, n]),
        "edges equal": lambda: run(lw=[0, 5, 5, 64]),
        "flux_up_dev NULL": lambda: run(drop=("flux_up_dev",)),
        "flux_down_dev NULL": lambda: run(drop=("flux_down_dev",)),
        "bin_up_dev without bin_down_dev": lambda: run(drop=("bin_down_dev",)),
        "bin_down_dev without bin_up_dev": lambda: run(drop=("bin_up_dev",)),
        "ncol = 0": lambda: run(gcols=none),
        "more columns than max_columns": lambda: run(pipe=narrow),
    }
    api.profile_enable(True)
    api.profile_read(api.TAG_KDIST_MAP, reset=True)
    try:
        for name, call in cases.items():
            assert call() == api.VALUE_ERR, name
        api.use_lane(device, 1)
        try:
            assert run() == api.VALUE_ERR
            with pytest.raises(api.GrtError, match="lane"):
                k.pipe.run_ck_fluxes(k.gcols, CE8, lw_edges=edges)
        finally:
            api.use_lane(device, 0)
        api.device_synchronize(device)
        assert not any(launches(CK_TAGS + (api.TAG_GAS_LW,)).values())
        assert frames.untouched() and np.all(map_sent.to_host(map_sent.nbytes // 8) == -7.25)
        # ... and the call they all fall short of is taken (the layer with SUM is ignored)
        assert run(key=(api.KDIST_KEY_SUM, 99)) == 0
        k.pipe.sync()
        assert launches(CK_TAGS) == dict(zip(CK_TAGS, (1, 1, 0, 1, 1)))
        tau = k.tau_gas(k.pipe, 0)
        m = class_map(tau, KEY_SUM, CE8)
        assert np.array_equal(map_sent.to_host((ncol, n), dtype=np.uint16), m)
        assert_sums(k, read_all(frames, ncol, V, 2, K), 0, m, edges, K)
    finally:
        api.profile_enable(False)
        for b in (frames, map_sent, mbuf):
            b.free()
        k.close()


# ---- the surface in force ------------------------------------------------------------------------------------------------- #
def test_the_sources_take_the_surface_in_force_column_by_column(shape_bands, oracle, lib, device):
    """grt_pipeline_set_surface with knots that are constant along the grid and differ from column to column (the rows
    are then those constants exactly, 0 and 1 among them): the emissivity and the two albedo rows are each column's own."""
    n, V, ncol, K = 65, 5, 3, 8
    k = Case(shape_bands[n], device, V, ncol, seed=7)
    edges = np.array(bin_sets(n)["three"], dtype=np.int32)
    e, ad, af = np.array([0.0, 1.0, 0.625]), np.array([1.0, 0.0, 0.25]), np.array([0.5, 0.125, 0.0])
    knots = [np.array([b.w0 + b.dw, b.w0 + 10 * b.dw]) for b in k.bands]
    two = np.ones((1, 2))
    gs, _keep = api.make_surface(ncol, emissivity=(knots[0], e[:, None] * two),
                                 albedo=(knots[1], ad[:, None] * two, af[:, None] * two))
    try:
        k.pipe.set_surface(gs)
        k.pipe.run_ck_fluxes(k.gcols, CE8, lw_edges=edges, sw_edges=edges, keep_map=True)
        got = k.pipe.ck_fluxes(ncol)
        ones = np.ones(n)
        w = [ck.wavenumbers(b.w0, b.dw, b.nw) for b in k.bands]
        rows = (ck.lw_rows(k.cols, w[0], e[:, None] * ones),
                ck.sw_rows(ncol, w[1], k.solar, ad[:, None] * ones, af[:, None] * ones))
        for bi, name in enumerate(("lw", "sw")):
            m = class_map(k.tau_gas(k.pipe, bi), KEY_SUM, CE8)
            assert np.array_equal(got[name]["map"], m)
            src = ck.source_sums(rows[bi], m, k.bands[bi].dw, edges, K)
            data = [2 * V] if bi == 0 else [1, 2, 3]
            assert same_bits(got[name]["source"][:, data], src[:, data]), name
            assert_solve(k, oracle, got[name], bi)
    finally:
        k.close()
