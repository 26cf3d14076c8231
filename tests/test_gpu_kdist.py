"""grt_kdist_rows and grt_pipeline_run_kdist: the k-distribution of optical-depth rows per bin and class, against
kdist_model.py's sequential sums BIT FOR BIT -- the counts with ==, the two sums through their int64 views --, at the
kernel's edge shapes, on the class boundaries, with and without weights, from run to run and in the deterministic mode; the
pipeline's outputs against the model applied to the tau_gas the pipeline shows afterwards, in the reference's operation
order (and there against the oracle's tau) and in the production form; and everything the calls refuse.

Shapes: grid lengths around the wave (64), the workgroup (256) and the points the kernel stages at a time (P, read from the
library): P - 1, P, P + 1 and, with K = 257, 2 P + 1; class counts around a wave's and a workgroup's threads and the
largest, 1024 (a thread owns four classes).  Each n meets two K and each K two n.

Bounds, none of them measured here: the device against the model, none (equality).  Against the oracle, per layer and bin,
1e-11 (the fast = 0 bound on tau, grt_ext.h) of the layer's largest tau on every point's weight, plus the summation bound
(m + 2) 2^-53 of the value, m the bin's points."""
import ctypes as C
import math

import numpy as np
import pytest

from grtcode_amd import api
from kdist_model import classes, kdist_row, kdist_rows, same_bits
from pipeline_support import _deterministic, _sentinel, _setup, columns, exact_trapezoid
from pipeline_support import bands  # noqa: F401  (a module fixture)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

DW = 0.37
SOLVER_TAGS = (api.TAG_SOLVER_LW, api.TAG_SOLVER_SW, api.TAG_CLEAR_OPTICS, api.TAG_ALLSKY_LW, api.TAG_ALLSKY_SW,
               api.TAG_AEROSOL_LW, api.TAG_AEROSOL_SW, api.TAG_SKY_LW, api.TAG_SKY_SW, api.TAG_ZENITH_SW, api.TAG_BINS,
               api.TAG_BAND_PROFILES, api.TAG_RADIANCE)


def upload(device, a):
    a = np.ascontiguousarray(a)
    buf = api.DeviceBuffer(device, a.nbytes)
    api.check(api.load_library().grt_host_to_device(device, buf.ptr, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes)))
    return buf


def log_uniform(rows, n, seed):
    """tau, log-uniform over eight decades"""
    return 10.0 ** np.random.default_rng(seed).uniform(-6.0, 2.0, (rows, n))


def log_classes(K):
    """K - 1 edges that leave part of the eight decades below the first and above the last"""
    return np.logspace(-5.0, 1.0, K - 1)


def bin_sets(n):
    """{0, n - 1}; every two-point bin; three unequal contiguous bins; two bins that leave the ends of the grid out --
    those of them a grid of n points has room for"""
    sets = {"whole": [0, n - 1], "pairs": list(range(n))}
    if n >= 8:
        sets["three"] = [0, n // 7 + 1, n // 2 + 1, n - 1]
    if n >= 5:
        sets["inner"] = [1, n // 3 + 1, n - 2]
    return sets


def assert_equals_model(got, want, what):
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0]), (what, "points")
    assert same_bits(got[1], want[1]), (what, "weight")
    assert same_bits(got[2], want[2]), (what, "tau")


# ---- 1. shapes ----------------------------------------------------------------------------------------------------------- #
SHAPES = [("2", 2), ("2", 1024), ("3", 3), ("3", 257), ("64", 64), ("64", 2), ("65", 65), ("65", 3), ("128", 256),
          ("128", 64), ("129", 257), ("129", 65), ("257", 1024), ("257", 256), ("P-1", 2), ("P-1", 257), ("P", 64),
          ("P", 1024), ("P+1", 65), ("P+1", 256), ("2P+1", 257), ("2P+1", 3)]


@pytest.mark.parametrize("n_name,K", SHAPES)
def test_edge_shapes_equal_the_model(lib, device, n_name, K):
    P = lib.grt_kdist_chunk_points()
    n = {"P-1": P - 1, "P": P, "P+1": P + 1, "2P+1": 2 * P + 1}.get(n_name) or int(n_name)
    tau = log_uniform(3, n, 1000 + n)
    ce = log_classes(K)
    buf = upload(device, tau)
    try:
        for name, edges in bin_sets(n).items():
            want = kdist_rows(tau, DW, edges, ce)
            assert want[0].sum() == 3 * sum(b - a + 1 for a, b in zip(edges[:-1], edges[1:]))
            for rows in (3, 1):
                got = api.kdist_rows(device, buf.ptr, rows, n, DW, ce, edges)
                assert got[0].shape == (rows, len(edges) - 1, K)
                assert_equals_model(got, [w[:rows] for w in want], (n, K, name, rows))
    finally:
        buf.free()


# ---- 2. class boundaries ------------------------------------------------------------------------------------------------- #
def test_values_on_and_beside_the_class_edges(lib, device):
    """The class edges themselves, their neighbours in double on both sides, 0, -1, +inf; and a NaN in a bin of its own
    (with the one ordinary point a bin needs beside it): counts as grt_ext.h says, the NaN in class 0 and in no other sum."""
    ce = np.array([1e-300, 3e-7, 0.1, 1.0, 1.0 + 2.0 ** -52, 7.0, 1e10, 1e300])
    K = ce.size + 1
    main = np.concatenate((ce, np.nextafter(ce, -np.inf), np.nextafter(ce, np.inf), [0.0, -1.0, np.inf]))
    m = main.size
    tau = np.concatenate((main, [0.5, np.nan]))[None, :]
    edges = [0, m - 1, m, m + 1]
    # per edge k: itself and its upper neighbour in class k + 1, its lower neighbour in class k; 0 and -1 in class 0, +inf
    # in the last.  (Edges 3 and 4 are neighbours in double: 1's upper neighbour IS edge 4, and goes to class 5.)
    want_main = np.zeros(K, dtype=np.int64)
    for k in range(ce.size):
        want_main[k] += 1
        want_main[k + 1] += 2
    want_main[0] += 2
    want_main[K - 1] += 1
    want_main[4] -= 1
    want_main[5] += 1
    assert np.array_equal(classes_count(main, ce, K), want_main)
    assert np.array_equal(np.bincount(classes(main, ce), minlength=K), want_main)
    buf = upload(device, tau)
    try:
        points, weight, tsum = api.kdist_rows(device, buf.ptr, 1, tau.size, 1.0, ce, edges)
    finally:
        buf.free()
    model = kdist_row(tau[0], 1.0, edges, ce)
    assert np.array_equal(model[0][0], classes_count(main, ce, K))
    assert np.array_equal(points[0, 0], classes_count(main, ce, K))
    assert points[0, 0].sum() == m and points[0, 0, 0] >= 3 and points[0, 0, K - 1] == 3
    assert np.array_equal(points[0], model[0])
    assert same_bits(weight[0], model[1])
    # the NaN: class 0 of the last bin, whose tau sum alone it poisons
    assert points[0, 2].tolist() == [1] + [0] * 2 + [1] + [0] * (K - 4)     # NaN -> 0, 0.5 -> class 3
    assert np.isnan(tsum[0, 2, 0]) and np.isnan(model[2][2, 0])
    rest = np.ones(tsum[0].shape, dtype=bool)
    rest[2, 0] = False
    assert not np.isnan(tsum[0][rest]).any()
    assert same_bits(tsum[0][rest], model[2][rest])
    assert np.isposinf(tsum[0, 0, K - 1]) and weight[0, 2, 0] == 0.5


def classes_count(values, ce, K):
    """grt_ext.h's rule, value by value in plain Python"""
    out = np.zeros(K, dtype=np.int32)
    for v in values:
        out[sum(1 for e in ce if float(e) <= float(v))] += 1
    return out


# ---- 3. weights ---------------------------------------------------------------------------------------------------------- #
def raw_call(lib, device, tau_ptr, rows, n, dw, ce, edges, weight, outs):
    """grt_kdist_rows with the three output pointers as given (None: NULL) -> the return code"""
    ce = np.ascontiguousarray(ce, dtype=np.float64)
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.int32)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    band = api.GrtKdistBand(None if e is None else e.ctypes.data_as(api.c_int_p), 0 if e is None else e.size - 1,
                            None if w is None else w.ctypes.data_as(api.c_double_p), *outs)
    return lib.grt_kdist_rows(device, tau_ptr, rows, n, dw, ce.size + 1, ce.ctypes.data_as(api.c_double_p), C.byref(band))


def test_weights_and_outputs_left_out(lib, device):
    rows, n, K = 2, 300, 12
    tau = log_uniform(rows, n, 77)
    ce = log_classes(K)
    edges = [0, 100, 299]
    rng = np.random.default_rng(78)
    s = rng.uniform(0.0, 4.0, n)
    s[rng.integers(0, n, 30)] = 0.0
    s[[0, 100, 299]] = [0.0, 2.5, 0.0]
    buf = upload(device, tau)
    try:
        plain = api.kdist_rows(device, buf.ptr, rows, n, DW, ce, edges)
        ones = api.kdist_rows(device, buf.ptr, rows, n, DW, ce, edges, weight=np.ones(n))
        assert_equals_model(ones, plain, "a weight of ones")
        got = api.kdist_rows(device, buf.ptr, rows, n, DW, ce, edges, weight=s)
        assert_equals_model(got, kdist_rows(tau, DW, edges, ce, s), "random weight")
        assert not same_bits(got[1], plain[1])
        # each output left out in turn: the other two as before, the sentinel where the third would go
        count = rows * 2 * K
        for skip in range(3):
            sent = [_sentinel(device, count) for _ in range(3)]
            outs = [None if k == skip else sent[k].ptr for k in range(3)]
            api.check(raw_call(lib, device, buf.ptr, rows, n, DW, ce, edges, s, outs))
            api.device_synchronize(device)
            for k in range(3):
                if k == skip:
                    assert np.all(sent[k].to_host(count) == -7.25)
                elif k == 0:
                    assert np.array_equal(sent[0].to_host((rows, 2, K), dtype=np.int32), got[0])
                else:
                    assert same_bits(sent[k].to_host((rows, 2, K)), got[k])
            for b in sent:
                b.free()
    finally:
        buf.free()


# ---- 4. order ------------------------------------------------------------------------------------------------------------ #
def test_the_same_bits_every_time_and_the_sequential_order(lib, device):
    P = lib.grt_kdist_chunk_points()
    rows, n, K = 3, P + 300, 70
    tau = log_uniform(rows, n, 5)
    ce = log_classes(K)
    edges = [0, 9, P + 299]
    s = np.random.default_rng(6).uniform(0.0, 2.0, n)
    buf = upload(device, tau)
    try:
        first = api.kdist_rows(device, buf.ptr, rows, n, DW, ce, edges, weight=s)
        again = api.kdist_rows(device, buf.ptr, rows, n, DW, ce, edges, weight=s)
        _deterministic(lib, True)
        try:
            fixed = api.kdist_rows(device, buf.ptr, rows, n, DW, ce, edges, weight=s)
        finally:
            _deterministic(lib, False)
    finally:
        buf.free()
    assert_equals_model(again, first, "the same call again")
    assert_equals_model(fixed, first, "the deterministic mode")
    assert_equals_model(first, kdist_rows(tau, DW, edges, ce, s), "the model")

    # one class that holds values over sixteen decades, largest first: the left-to-right sum is not the exact one, nor any
    # other association's
    n = 1500
    rng = np.random.default_rng(8)
    row = (10.0 ** np.linspace(8.0, -8.0, n)) * rng.uniform(1.0, 2.0, n)
    ce, edges = np.array([1e-30]), [0, n - 1]
    model = kdist_row(row, DW, edges, ce)
    w = np.full(n, DW)
    w[0] = w[-1] = 0.5 * DW
    assert model[0][0].tolist() == [0, n]
    assert model[2][0, 1] != math.fsum(w * row), "the case cannot tell a sequential sum from an exact one"
    assert model[2][0, 1] != np.sum(w * row), "the case cannot tell a sequential sum from a pairwise one"
    buf = upload(device, row)
    try:
        got = api.kdist_rows(device, buf.ptr, 1, n, DW, ce, edges)
    finally:
        buf.free()
    assert_equals_model(got, [m[None] for m in model], "sixteen decades")


# ---- the pipeline's cases -------------------------------------------------------------------------------------------------- #
V, NCOL, K_PIPE = 5, 3, 24
PIPE_CLASSES = np.logspace(-9.0, 2.0, K_PIPE - 1)


class Case:
    def __init__(self, bands, device, fast, spectral, lw_only=False):
        self.bands, self.device = bands, device
        self.cols = columns(V)[:NCOL]
        use = (bands[0], None) if lw_only else bands
        self.go_lw, self.go_sw, self.emis, self.alb, self.solar = _setup(use, device, V, fast=fast)
        self.gcols, self.keep = api.make_columns(self.cols, MOL_ORDER, cfc_order=(0, 1))
        self.pipes = []
        self.pipe = self.make(spectral)

    def make(self, spectral, max_columns=NCOL):
        p = api.Pipeline(self.go_lw, self.go_sw, max_columns, -1, self.emis, self.alb, self.solar, spectral=spectral)
        self.pipes.append(p)
        return p

    def tau_gas(self, pipe, bi):
        return api.device_to_host(self.device, pipe.views(bi)["tau_gas"], (NCOL, V - 1, self.bands[bi].nw)).copy()

    def close(self):
        for p in self.pipes:
            p.destroy()
        for go in (self.go_lw, self.go_sw):
            if go is not None:
                go.destroy()


def pipe_edges(bands):
    return [np.array([0, b.nw // 5, b.nw // 2 + 3, b.nw - 1], np.int32) for b in bands]


def assert_pipeline_equals_model(k, pipe, got, edges, weights=(None, None)):
    for bi, key in enumerate(("lw", "sw")):
        if edges[bi] is None:
            assert got[key]["points"].shape == (NCOL, V - 1, 0, K_PIPE)
            continue
        tau = k.tau_gas(pipe, bi)
        want = kdist_rows(tau.reshape(NCOL * (V - 1), -1), k.bands[bi].dw, edges[bi], PIPE_CLASSES, weights[bi])
        shape = (NCOL, V - 1, len(edges[bi]) - 1, K_PIPE)
        assert got[key]["points"].shape == shape
        assert_equals_model([got[key][name] for name in ("points", "weight", "tau")], [w.reshape(shape) for w in want], key)
        assert got[key]["points"].sum() == NCOL * (V - 1) * sum(b - a + 1 for a, b in zip(edges[bi][:-1], edges[bi][1:]))
        assert np.count_nonzero(got[key]["points"].sum(axis=(0, 1, 2))) >= 3, "the classes do not spread the band's tau"


# ---- 6. reference order ------------------------------------------------------------------------------------------------------ #
def test_pipeline_in_reference_order_equals_the_model_and_the_oracle(bands, oracle, lib, device):
    k = Case(bands, device, 0, True)
    edges = pipe_edges(bands)
    try:
        k.pipe.run_kdist(k.gcols, PIPE_CLASSES, lw_edges=edges[0], sw_edges=edges[1])
        got = k.pipe.kdist(NCOL)
        assert_pipeline_equals_model(k, k.pipe, got, edges)
        for bi, key in enumerate(("lw", "sw")):
            band = bands[bi]
            for c, col in enumerate(k.cols):
                tau_o = band.oracle_tau(oracle, oracle, lib, col)
                for j in range(V - 1):
                    for b, (lo, hi) in enumerate(zip(edges[bi][:-1], edges[bi][1:])):
                        m = int(hi - lo + 1)
                        value = math.fsum(got[key]["tau"][c, j, b])
                        ref, _mag = exact_trapezoid(tau_o[j, lo:hi + 1], band.dw)
                        tol = 1e-11 * tau_o[j].max() * m * band.dw + (m + 2) * 2.0 ** -53 * abs(ref)
                        assert abs(value - ref) <= tol, (key, c, j, b, value, ref, tol)
                        width = math.fsum(got[key]["weight"][c, j, b])
                        assert abs(width - (m - 1) * band.dw) <= (m + 2) * 2.0 ** -53 * width
    finally:
        k.close()


def test_longwave_bins_alone_leave_the_shortwave_and_the_solvers_alone(bands, lib, device):
    k = Case(bands, device, 0, True)
    edges = [pipe_edges(bands)[0], None]
    try:
        api.profile_enable(True)
        api.profile_read(api.TAG_GAS_LW, reset=True)
        k.pipe.run_kdist(k.gcols, PIPE_CLASSES, lw_edges=edges[0])
        k.pipe.sync()
        launches = {tag: api.profile_read(tag)[1] for tag in SOLVER_TAGS + (api.TAG_GAS_SW, api.TAG_FAR_SW)}
        assert api.profile_read(api.TAG_GAS_LW)[1] >= 1 and api.profile_read(api.TAG_KDIST)[1] == 1
        assert not any(launches.values()), launches
        assert_pipeline_equals_model(k, k.pipe, k.pipe.kdist(NCOL), edges)
    finally:
        api.profile_enable(False)
        k.close()


# ---- 7. production form ------------------------------------------------------------------------------------------------------ #
def test_production_form_reduces_the_whole_tau_and_leaves_no_state(bands, lib, device):
    """fast = 3, no spectra kept.  The array that was reduced holds the spectral tables' part -- it is, in the deterministic
    mode, the tau_gas a pipeline that keeps its spectra shows --, and run, run_kdist, run gives the first fluxes again."""
    k = Case(bands, device, 3, False)
    edges = pipe_edges(bands)
    weights = (None, np.asarray(k.solar, dtype=np.float64))
    _deterministic(lib, True)
    try:
        k.pipe.run(k.gcols)
        before = k.pipe.fluxes(NCOL)
        k.pipe.run_kdist(k.gcols, PIPE_CLASSES, lw_edges=edges[0], sw_edges=edges[1], sw_weight=weights[1])
        got = k.pipe.kdist(NCOL)
        assert_pipeline_equals_model(k, k.pipe, got, edges, weights)
        reduced = k.tau_gas(k.pipe, 1)
        k.pipe.run(k.gcols)
        after = k.pipe.fluxes(NCOL)
        assert same_bits(before, after) and np.all(before[:, 0] > 0.0)
        full = k.make(True)
        full.run(k.gcols)
        assert np.array_equal(k.tau_gas(full, 1), reduced)
        # the same inputs again: the same bits
        k.pipe.run_kdist(k.gcols, PIPE_CLASSES, lw_edges=edges[0], sw_edges=edges[1], sw_weight=weights[1])
        again = k.pipe.kdist(NCOL)
        for key in ("lw", "sw"):
            assert_equals_model([again[key][x] for x in ("points", "weight", "tau")],
                                [got[key][x] for x in ("points", "weight", "tau")], key)
    finally:
        _deterministic(lib, False)
        k.close()


# ---- 5. and 8. refusals ------------------------------------------------------------------------------------------------------ #
def test_refused_rows_calls(lib, device):
    rows, n, K = 2, 40, 5
    tau = log_uniform(rows, n, 3)
    ce = log_classes(K)
    edges = [0, 10, 39]
    ok = np.ones(n)
    buf = upload(device, tau)
    count = rows * 2 * 1100
    sent = [_sentinel(device, count) for _ in range(3)]
    outs = [b.ptr for b in sent]

    def bad_weight(v):
        w = ok.copy()
        w[17] = v
        return w

    cases = {
        "K = 1": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, np.zeros(0), edges, None, outs),
        "K = 1025": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, np.logspace(-5, 1, 1024), edges, None, outs),
        "class edges equal": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, [0.1, 0.1, 1.0, 2.0], edges, None, outs),
        "class edges falling": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, [0.1, 1.0, 0.5, 2.0], edges, None, outs),
        "class edge NaN": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, [0.1, np.nan, 1.0, 2.0], edges, None, outs),
        "class edge inf": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, [0.1, 0.5, 1.0, np.inf], edges, None, outs),
        "NULL edges": lambda: lib.grt_kdist_rows(
            device, buf.ptr, rows, n, DW, K, ce.ctypes.data_as(api.c_double_p),
            C.byref(api.GrtKdistBand(None, 2, None, *outs))),
        "negative bins": lambda: lib.grt_kdist_rows(
            device, buf.ptr, rows, n, DW, K, ce.ctypes.data_as(api.c_double_p),
            C.byref(api.GrtKdistBand(np.array(edges, np.int32).ctypes.data_as(api.c_int_p), -1, None, *outs))),
        "no bins": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, ce, [0], None, outs),
        "edges below the grid": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, ce, [-1, 10, 39], None, outs),
        "edges beyond the grid": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, ce, [0, 10, 40], None, outs),
        "edges equal": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, ce, [0, 10, 10, 39], None, outs),
        "edges falling": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, ce, [0, 20, 10, 39], None, outs),
        "no outputs": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, ce, edges, None, [None, None, None]),
        "weight negative": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, ce, edges, bad_weight(-1e-300), outs),
        "weight NaN": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, ce, edges, bad_weight(np.nan), outs),
        "weight inf": lambda: raw_call(lib, device, buf.ptr, rows, n, DW, ce, edges, bad_weight(np.inf), outs),
        "rows = 0": lambda: raw_call(lib, device, buf.ptr, 0, n, DW, ce, edges, None, outs),
        "n = 1": lambda: raw_call(lib, device, buf.ptr, rows, 1, DW, ce, [0], None, outs),
        "dw = 0": lambda: raw_call(lib, device, buf.ptr, rows, n, 0.0, ce, edges, None, outs),
        "dw < 0": lambda: raw_call(lib, device, buf.ptr, rows, n, -DW, ce, edges, None, outs),
        "dw NaN": lambda: raw_call(lib, device, buf.ptr, rows, n, np.nan, ce, edges, None, outs),
        "dw inf": lambda: raw_call(lib, device, buf.ptr, rows, n, np.inf, ce, edges, None, outs),
        "NULL band": lambda: lib.grt_kdist_rows(device, buf.ptr, rows, n, DW, K, ce.ctypes.data_as(api.c_double_p), None),
        "NULL class edges": lambda: lib.grt_kdist_rows(
            device, buf.ptr, rows, n, DW, K, None,
            C.byref(api.GrtKdistBand(np.array(edges, np.int32).ctypes.data_as(api.c_int_p), 2, None, *outs))),
    }
    api.profile_enable(True)
    api.profile_read(api.TAG_KDIST, reset=True)
    try:
        for name, call in cases.items():
            assert call() == api.VALUE_ERR, name
        api.device_synchronize(device)
        assert api.profile_read(api.TAG_KDIST)[1] == 0
        for b in sent:
            assert np.all(b.to_host(count) == -7.25)
        # ... and the call they all fall short of is taken
        assert raw_call(lib, device, buf.ptr, rows, n, DW, ce, edges, ok, outs) == 0
        assert api.profile_read(api.TAG_KDIST)[1] == 1
        assert np.array_equal(sent[0].to_host((rows, 2, K), dtype=np.int32), kdist_rows(tau, DW, edges, ce)[0])
    finally:
        api.profile_enable(False)
        buf.free()
        for b in sent:
            b.free()


def test_refused_pipeline_calls_and_the_wrong_lane(bands, lib, device):
    k = Case(bands, device, 0, False, lw_only=True)
    wide = k.make(False, max_columns=2)             # (for a batch of more columns than it was made for)
    nl = bands[0].nw
    edges = pipe_edges(bands)[0]
    rows = NCOL * (V - 1)
    count = rows * 3 * 1100
    sent = [_sentinel(device, count) for _ in range(3)]

    def run(pipe=None, gcols=None, classes_=PIPE_CLASSES, lw=edges, sw=None, weight=None, outs=True, kdist=True):
        gk, _keep = api.make_kdist(classes_, lw, sw, lw_weight=weight)
        for band in (gk.lw, gk.sw):
            if outs:
                band.points_dev, band.weight_dev, band.tau_dev = (b.ptr for b in sent)
        return lib.grt_pipeline_run_kdist((pipe or k.pipe).p, C.byref(gcols if gcols is not None else k.gcols),
                                          C.byref(gk) if kdist else None)

    none, _keep_none = api.make_columns(k.cols, MOL_ORDER, cfc_order=(0, 1))
    none.ncol = 0
    bad = np.ones(nl)
    bad[5] = -2.0
    many = np.logspace(-9.0, 2.0, 1024)

    def null_class_edges():
        gk, _keep = api.make_kdist(PIPE_CLASSES, edges)
        gk.class_edges = None
        gk.lw.points_dev = sent[0].ptr
        return lib.grt_pipeline_run_kdist(k.pipe.p, C.byref(k.gcols), C.byref(gk))

    def negative_bins():
        gk, _keep = api.make_kdist(PIPE_CLASSES, edges)
        gk.lw.num_bins = -3
        gk.lw.points_dev = sent[0].ptr
        return lib.grt_pipeline_run_kdist(k.pipe.p, C.byref(k.gcols), C.byref(gk))

    def null_edges():
        gk, _keep = api.make_kdist(PIPE_CLASSES, edges)
        gk.lw.edges = None
        gk.lw.points_dev = sent[0].ptr
        return lib.grt_pipeline_run_kdist(k.pipe.p, C.byref(k.gcols), C.byref(gk))

    cases = {
        "NULL kdist": lambda: run(kdist=False),
        "NULL class edges": null_class_edges,
        "K = 1": lambda: run(classes_=np.zeros(0)),
        "K = 1025": lambda: run(classes_=many),
        "class edges falling": lambda: run(classes_=[1.0, 0.5]),
        "class edge NaN": lambda: run(classes_=[1.0, np.nan]),
        "class edge inf": lambda: run(classes_=[1.0, np.inf]),
        "negative bins": negative_bins,
        "NULL edges": null_edges,
        "edges beyond the grid": lambda: run(lw=[0, 5, nl]),
        "edges below the grid": lambda: run(lw=[-1, 5, nl - 1]),
        "edges equal": lambda: run(lw=[0, 5, 5, nl - 1]),
        "bins for a band the pipeline lacks": lambda: run(sw=[0, 5, 9]),
        "no bins in either band": lambda: run(lw=None),
        "no outputs": lambda: run(outs=False),
        "weight negative": lambda: run(weight=bad),
        "weight NaN": lambda: run(weight=np.where(bad < 0, np.nan, bad)),
        "ncol = 0": lambda: run(gcols=none),
        "more columns than max_columns": lambda: run(pipe=wide),
    }
    api.profile_enable(True)
    api.profile_read(api.TAG_KDIST, reset=True)
    try:
        for name, call in cases.items():
            assert call() == api.VALUE_ERR, name
        # the wrong lane: refused as grt_pipeline_run is
        api.use_lane(device, 1)
        try:
            assert run() == api.VALUE_ERR
            with pytest.raises(api.GrtError, match="lane"):
                k.pipe.run_kdist(k.gcols, PIPE_CLASSES, lw_edges=edges)
            with pytest.raises(api.GrtError, match="lane"):
                k.pipe.run(k.gcols)
        finally:
            api.use_lane(device, 0)
        api.device_synchronize(device)
        assert api.profile_read(api.TAG_KDIST)[1] == 0
        assert api.profile_read(api.TAG_GAS_LW)[1] == 0
        for b in sent:
            assert np.all(b.to_host(count) == -7.25)
        assert run() == 0                           # ... and the call they all fall short of is taken
        k.pipe.sync()
        assert api.profile_read(api.TAG_KDIST)[1] == 1
        want = kdist_rows(k.tau_gas(k.pipe, 0).reshape(rows, nl), bands[0].dw, edges, PIPE_CLASSES)
        assert np.array_equal(sent[0].to_host((rows, 3, K_PIPE), dtype=np.int32), want[0])
        assert same_bits(sent[2].to_host((rows, 3, K_PIPE)), want[2])
    finally:
        api.profile_enable(False)
        for b in sent:
            b.free()
        k.close()
