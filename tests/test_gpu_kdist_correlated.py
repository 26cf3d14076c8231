"""grt_kdist_class_map, grt_kdist_mapped_rows and grt_pipeline_run_kdist_correlated: the class map of a key row or of the
rows' sum, and every row of a group reduced under it, against kdist_correlated_model.py BIT FOR BIT -- the map with
array_equal, the counts with ==, the sums through their int64 views -- at the kernels' edge shapes, on the class boundaries
of the key, tied to grt_kdist_rows, through a group stride and under maps that name no class, from run to run and in the
deterministic mode; the pipeline's outputs against the model applied to the tau_gas the pipeline shows afterwards, in the
reference's operation order and in the production form; the g-class fluxes of grt_pipeline_run_spectral's rows; and what
the calls refuse once they have a device.

Shapes: grid lengths around the wave (64), the workgroup (256) and the points the kernels stage at a time (P, read from the
library); class counts around a wave's and a workgroup's threads and the largest, 1024.  Each n meets two K and each K
three n; the rows per group (1, 2, 5) and the groups (3, 1) each meet each other; the key (the sum, the first row, the last
row) and the weight (none, one) rotate over the bin sets and the cases, so that every bin set meets every key and both.

Bounds, none of them measured here: the device against the model, none (equality).  The g-class fluxes against the bins of
grt_pipeline_run_spectral, per row and bin, 2 (m + K) 2^-53 sum |W_i f_i|, m the bin's points: two orderings of one sum."""
import ctypes as C
import math

import numpy as np
import pytest

from grtcode_amd import api
from kdist_correlated_model import KEY_ROW, KEY_SUM, class_map, mapped_rows
from kdist_model import same_bits
from pipeline_support import _deterministic, _sentinel, _setup, columns
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


def log_uniform(shape, seed):
    """tau, log-uniform over eight decades"""
    return 10.0 ** np.random.default_rng(seed).uniform(-6.0, 2.0, shape)


def log_classes(K, rows=1):
    """K - 1 edges that leave part of the eight decades (of a sum of `rows` such values) below the first and above the last"""
    return np.logspace(-5.0, 1.0, K - 1) * rows


def bin_sets(n):
    """{0, n - 1}; every two-point bin; three unequal contiguous bins; two bins that leave the ends of the grid out --
    those of them a grid of n points has room for"""
    sets = {"whole": [0, n - 1], "pairs": list(range(n))}
    if n >= 8:
        sets["three"] = [0, n // 7 + 1, n // 2 + 1, n - 1]
    if n >= 5:
        sets["inner"] = [1, n // 3 + 1, n - 2]
    return sets


def device_map(device, x_ptr, G, R, n, ce, kind, key_row=0):
    """api.kdist_class_map of the device array at x_ptr -> (the map's device buffer, its host copy [G][n])"""
    mbuf = api.kdist_class_map(device, x_ptr, G, R, n, ce, kind, key_row)
    api.device_synchronize(device)
    return mbuf, mbuf.to_host((G, n), dtype=np.uint16)


def assert_equals_model(got, want, what):
    assert got[0].dtype == np.int32 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0]), (what, "points")
    assert same_bits(got[1], want[1]), (what, "weight")
    assert same_bits(got[2], want[2]), (what, "tau")


# ---- 1. shapes ----------------------------------------------------------------------------------------------------------- #
SHAPES = [("2", 2, 5, 3), ("2", 1024, 1, 1), ("3", 64, 2, 3), ("3", 257, 5, 1), ("64", 65, 1, 3), ("64", 2, 2, 1),
          ("65", 256, 5, 3), ("65", 64, 1, 1), ("257", 1024, 2, 3), ("257", 65, 5, 1), ("P-1", 2, 1, 3),
          ("P-1", 257, 2, 1), ("P", 64, 5, 3), ("P", 1024, 2, 1), ("P+1", 65, 1, 3), ("P+1", 256, 2, 3),
          ("2P+1", 257, 5, 1), ("2P+1", 256, 2, 3)]


@pytest.mark.parametrize("case", range(len(SHAPES)), ids=["%s-K%d-R%d-G%d" % s for s in SHAPES])
def test_edge_shapes_equal_the_model(lib, device, case):
    n_name, K, R, G = SHAPES[case]
    P = lib.grt_kdist_chunk_points()
    n = {"P-1": P - 1, "P": P, "P+1": P + 1, "2P+1": 2 * P + 1}.get(n_name) or int(n_name)
    x = log_uniform((G, R, n), 2000 + 7 * n + K)
    s = np.random.default_rng(case).uniform(0.0, 3.0, n)
    keys = [(KEY_SUM, 0, log_classes(K, R)), (KEY_ROW, 0, log_classes(K)), (KEY_ROW, R - 1, log_classes(K))]
    xbuf = upload(device, x)
    maps = []
    try:
        for kind, row, ce in keys:
            want = class_map(x, kind, ce, row)
            mbuf, got = device_map(device, xbuf.ptr, G, R, n, ce, kind, row)
            maps.append((mbuf, want))
            assert got.dtype == np.uint16 and np.array_equal(got, want), (n, K, R, G, kind, row)
            assert want.max() < K
        for bi, (name, edges) in enumerate(bin_sets(n).items()):
            mbuf, m = maps[(bi + case) % 3]
            weight = s if (bi + case // 3) % 2 else None
            want = mapped_rows(x, m, DW, edges, K, weight)
            assert want[0].sum() == G * sum(b - a + 1 for a, b in zip(edges[:-1], edges[1:]))
            got = api.kdist_mapped_rows(device, xbuf.ptr, R * n, mbuf.ptr, G, R, n, DW, K, edges, weight)
            assert got[0].shape == (G, len(edges) - 1, K) and got[2].shape == (G, R, len(edges) - 1, K)
            assert_equals_model(got, want, (n, K, R, G, name))
    finally:
        xbuf.free()
        for mbuf, _m in maps:
            mbuf.free()


# ---- 2. class boundaries in the key -------------------------------------------------------------------------------------- #
def classes_by_rule(values, ce):
    """grt_ext.h's rule, value by value in plain Python"""
    return np.array([sum(1 for e in ce if float(e) <= float(v)) for v in values], dtype=np.uint16)


def test_key_values_on_and_beside_the_class_edges(lib, device):
    ce = np.array([1e-300, 3e-7, 0.1, 1.0, 1.0 + 2.0 ** -52, 7.0, 1e10, 1e300])
    K = ce.size + 1
    key = np.concatenate((ce, np.nextafter(ce, -np.inf), np.nextafter(ce, np.inf), [0.0, -1.0, np.inf, np.nan, 0.5]))
    n = key.size
    want = classes_by_rule(key, ce)
    assert want[n - 2] == 0 and want[n - 3] == K - 1 and want[n - 4] == 0 and want[n - 5] == 0 and want[3] == 4
    # a key row between two others; then values of three rows with one NaN, reduced under that map
    x = np.stack((log_uniform(n, 1), key, log_uniform(n, 2)))[None]
    values = log_uniform((1, 3, n), 3)
    j = 5
    values[0, 1, j] = np.nan
    edges = [0, n // 2, n - 1]
    xbuf, vbuf = upload(device, x), upload(device, values)
    try:
        mbuf, m = device_map(device, xbuf.ptr, 1, 3, n, ce, KEY_ROW, 1)
        try:
            assert np.array_equal(m[0], want) and np.array_equal(m, class_map(x, KEY_ROW, ce, 1))
            got = api.kdist_mapped_rows(device, vbuf.ptr, 3 * n, mbuf.ptr, 1, 3, n, 1.0, K, edges)
        finally:
            mbuf.free()
    finally:
        xbuf.free()
        vbuf.free()
    model = mapped_rows(values, m, 1.0, edges, K)
    assert np.array_equal(got[0], model[0]) and same_bits(got[1], model[1])
    assert np.array_equal(got[0].sum(axis=1)[0] - np.bincount(want.astype(int), minlength=K),
                          np.bincount([int(want[n // 2])], minlength=K))
    # the NaN: its own row's sum of its own class in its own bin, and nothing else
    nan_at = np.zeros(got[2].shape, dtype=bool)
    nan_at[0, 1, 0, want[j]] = True
    assert np.array_equal(np.isnan(got[2]), nan_at) and np.array_equal(np.isnan(model[2]), nan_at)
    assert same_bits(got[2][~nan_at], model[2][~nan_at])


def test_key_sums_on_the_class_edges(lib, device):
    """Rows that add to exactly an edge (and to it only after rounding), a sum that overflows, a sum with a NaN row, and
    an order of rows that matters: ((0 + 1e16) + 1) - 1e16 is 0, the other way round it would be 1."""
    ce = np.array([0.5, 1.0, 1.0 + 2.0 ** -52, 1e300])
    K = ce.size + 1
    cols = np.array([[0.25, 0.75, 0.0],                 # exactly the edge 1.0            -> 2
                     [1.0, 2.0 ** -54, 0.0],            # 1 + 2^-54 rounds to 1.0          -> 2
                     [1.0, 2.0 ** -52, 0.0],            # exactly the next edge           -> 3
                     [0.25, 0.25 - 2.0 ** -54, 0.0],    # one ulp short of 0.5            -> 0
                     [1e308, 1e308, -1e308],            # inf - 1e308 = inf               -> K - 1
                     [1.0, np.nan, 1.0],                # NaN                             -> 0
                     [1e16, 1.0, -1e16],                # 0 in this order                 -> 0
                     [-1.0, 0.25, 0.5]]).T              # below the first edge            -> 0
    want = np.array([2, 2, 3, 0, K - 1, 0, 0, 0], dtype=np.uint16)
    x = cols[None]
    n = x.shape[2]
    assert np.array_equal(class_map(x, KEY_SUM, ce)[0], want)
    xbuf = upload(device, x)
    try:
        mbuf, m = device_map(device, xbuf.ptr, 1, 3, n, ce, KEY_SUM)
        mbuf.free()
    finally:
        xbuf.free()
    assert np.array_equal(m[0], want)


# ---- 3. the tie to grt_kdist_rows ------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("K", [64, 257, 1024])
def test_the_key_rows_own_outputs_are_kdist_rows(lib, device, K):
    P = lib.grt_kdist_chunk_points()
    G, R, n = 2, 3, P + 300
    x = log_uniform((G, R, n), 40 + K)
    ce = log_classes(K)
    edges = [0, 9, P + 5, n - 1]
    s = np.random.default_rng(K).uniform(0.0, 2.0, n)
    xbuf = upload(device, x)
    try:
        for r in (0, R - 1):
            mbuf, _m = device_map(device, xbuf.ptr, G, R, n, ce, KEY_ROW, r)
            try:
                points, weight, tau = api.kdist_mapped_rows(device, xbuf.ptr, R * n, mbuf.ptr, G, R, n, DW, K, edges, s)
            finally:
                mbuf.free()
            plain = api.kdist_rows(device, xbuf.ptr, G * R, n, DW, ce, edges, weight=s)
            plain = [p.reshape(G, R, len(edges) - 1, K)[:, r] for p in plain]
            assert_equals_model((points, weight, tau[:, r]), plain, (K, r))
    finally:
        xbuf.free()


# ---- 4. strides and bad maps ------------------------------------------------------------------------------------------------- #
def raw_mapped(lib, device, values_ptr, stride, map_ptr, G, R, n, dw, K, edges, weight, outs):
    """grt_kdist_mapped_rows with the three output pointers as given (None: NULL) -> the return code"""
    e = np.ascontiguousarray(edges, dtype=np.int32)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    band = api.GrtKdistBand(e.ctypes.data_as(api.c_int_p), e.size - 1,
                            None if w is None else w.ctypes.data_as(api.c_double_p), *outs)
    return lib.grt_kdist_mapped_rows(device, values_ptr, stride, map_ptr, G, R, n, dw, K, C.byref(band))


def test_a_group_stride_skips_what_lies_between_the_groups(lib, device):
    G, R, n, K, gap = 3, 2, 301, 70, 37
    x = log_uniform((G, R, n), 50)
    ce = log_classes(K, R)
    edges = [0, 100, 300]
    strided = np.full((G, R * n + gap), np.nan)          # (a NaN that is read shows in a sum)
    strided[:, :R * n] = x.reshape(G, R * n)
    xbuf, sbuf = upload(device, x), upload(device, strided)
    try:
        mbuf, m = device_map(device, xbuf.ptr, G, R, n, ce, KEY_SUM)
        try:
            got = api.kdist_mapped_rows(device, sbuf.ptr, R * n + gap, mbuf.ptr, G, R, n, DW, K, edges)
        finally:
            mbuf.free()
    finally:
        xbuf.free()
        sbuf.free()
    assert not np.isnan(got[2]).any()
    assert_equals_model(got, mapped_rows(x, m, DW, edges, K), "strided")


@pytest.mark.parametrize("K", [5, 257])
def test_map_entries_that_name_no_class_are_counted_nowhere_and_write_nowhere(lib, device, K):
    G, R, n, frame = 2, 3, 400, 512
    x = log_uniform((G, R, n), 60)
    m = class_map(x, KEY_SUM, log_classes(K, R))
    bad_at = [(0, 7), (0, 255), (1, 0), (1, 256), (1, 399)]
    for k, (g, i) in enumerate(bad_at):
        m[g, i] = (K, K + 1, 0xffff, 1024, 300)[k]
    edges = [0, 255, 399]
    want = mapped_rows(x, m, DW, edges, K)
    # (point 255 is an edge of both bins, and lost to both)
    lost = sum(1 for g, i in bad_at for a, b in zip(edges[:-1], edges[1:]) if a <= i <= b)
    assert want[0].sum() == G * (256 + 145) - lost and lost == 6
    counts = (G * 2 * K, G * 2 * K, G * R * 2 * K)
    xbuf, mbuf = upload(device, x), upload(device, m)
    sent = [_sentinel(device, c + 2 * frame) for c in counts]
    try:
        outs = [C.c_void_p(b.ptr.value + 8 * frame) for b in sent]
        api.check(raw_mapped(lib, device, xbuf.ptr, R * n, mbuf.ptr, G, R, n, DW, K, edges, None, outs))
        api.device_synchronize(device)
        host = [b.to_host(c + 2 * frame) for b, c in zip(sent, counts)]
    finally:
        for b in [xbuf, mbuf] + sent:
            b.free()
    for h, c in zip(host, counts):
        assert np.all(h[:frame] == -7.25) and np.all(h[frame + c:] == -7.25)
    # (the counts are ints: G 2 K of them lie in the first half of their frame's doubles, the rest is untouched)
    points = host[0][frame:frame + counts[0]].view(np.int32)[:counts[0]].reshape(G, 2, K)
    assert np.all(host[0][frame + (counts[0] + 1) // 2:] == -7.25)
    got = (points, host[1][frame:frame + counts[1]].reshape(G, 2, K), host[2][frame:frame + counts[2]].reshape(G, R, 2, K))
    assert_equals_model(got, want, "bad map")
    assert got[0].sum() == G * (256 + 145) - lost


# ---- 5. determinism and independence --------------------------------------------------------------------------------------- #
def test_the_same_bits_every_time_alone_and_in_a_batch(lib, device):
    P = lib.grt_kdist_chunk_points()
    G, R, n, K = 3, 4, P + 300, 70
    x = log_uniform((G, R, n), 70)
    ce = log_classes(K, R)
    edges = [0, 9, P + 299]
    s = np.random.default_rng(71).uniform(0.0, 2.0, n)
    xbuf = upload(device, x)
    try:
        mbuf, m = device_map(device, xbuf.ptr, G, R, n, ce, KEY_SUM)
        again_buf, again_m = device_map(device, xbuf.ptr, G, R, n, ce, KEY_SUM)
        again_buf.free()
        assert np.array_equal(m, again_m)
        try:
            first = api.kdist_mapped_rows(device, xbuf.ptr, R * n, mbuf.ptr, G, R, n, DW, K, edges, s)
            again = api.kdist_mapped_rows(device, xbuf.ptr, R * n, mbuf.ptr, G, R, n, DW, K, edges, s)
            _deterministic(lib, True)
            try:
                fixed_buf, fixed_m = device_map(device, xbuf.ptr, G, R, n, ce, KEY_SUM)
                fixed_buf.free()
                fixed = api.kdist_mapped_rows(device, xbuf.ptr, R * n, mbuf.ptr, G, R, n, DW, K, edges, s)
            finally:
                _deterministic(lib, False)
            # group 1 alone: its rows and its map are where the batch's group 1 lies
            alone = api.kdist_mapped_rows(device, xbuf.ptr.value + 8 * R * n, R * n, mbuf.ptr.value + 2 * n, 1, R, n, DW, K,
                                          edges, s)
            alone_buf, alone_m = device_map(device, xbuf.ptr.value + 8 * R * n, 1, R, n, ce, KEY_SUM)
            alone_buf.free()
            # each output alone
            count = G * 2 * K
            for only in range(3):
                sent = _sentinel(device, count * (R if only == 2 else 1))
                outs = [sent.ptr if k == only else None for k in range(3)]
                try:
                    api.check(raw_mapped(lib, device, xbuf.ptr, R * n, mbuf.ptr, G, R, n, DW, K, edges, s, outs))
                    api.device_synchronize(device)
                    if only == 0:
                        assert np.array_equal(sent.to_host((G, 2, K), dtype=np.int32), first[0])
                    else:
                        assert same_bits(sent.to_host(first[only].shape), first[only]), only
                finally:
                    sent.free()
        finally:
            mbuf.free()
    finally:
        xbuf.free()
    assert_equals_model(again, first, "the same call again")
    assert_equals_model(fixed, first, "the deterministic mode")
    assert np.array_equal(fixed_m, m) and np.array_equal(alone_m[0], m[1])
    assert_equals_model(alone, [f[1:2] for f in first], "a group alone")
    assert_equals_model(first, mapped_rows(x, m, DW, edges, K, s), "the model")


# ---- the pipeline's cases -------------------------------------------------------------------------------------------------- #
V, K_PIPE = 5, 24
L = V - 1
PIPE_CLASSES = np.logspace(-9.0, 2.0, K_PIPE - 1)
NAMES = ("points", "weight", "tau")


class Case:
    def __init__(self, bands, device, fast, spectral, ncol, lw_only=False):
        self.bands, self.device, self.ncol = bands, device, ncol
        self.cols = columns(V)[:ncol]
        use = (bands[0], None) if lw_only else bands
        self.go_lw, self.go_sw, self.emis, self.alb, self.solar = _setup(use, device, V, fast=fast)
        self.gcols, self.keep = api.make_columns(self.cols, MOL_ORDER, cfc_order=(0, 1))
        self.pipes = []
        self.pipe = self.make(spectral)

    def make(self, spectral, max_columns=None):
        p = api.Pipeline(self.go_lw, self.go_sw, max_columns or self.ncol, -1, self.emis, self.alb, self.solar,
                         spectral=spectral)
        self.pipes.append(p)
        return p

    def tau_gas(self, pipe, bi):
        return api.device_to_host(self.device, pipe.views(bi)["tau_gas"], (self.ncol, L, self.bands[bi].nw)).copy()

    def close(self):
        for p in self.pipes:
            p.destroy()
        for go in (self.go_lw, self.go_sw):
            if go is not None:
                go.destroy()


def pipe_edges(bands):
    return [np.array([0, b.nw // 5, b.nw // 2 + 3, b.nw - 1], np.int32) for b in bands]


def key_of(spec):
    return (KEY_SUM, 0) if spec[0] == "sum" else (KEY_ROW, spec[1])


def assert_pipeline_equals_model(k, pipe, got, edges, keys, weights=(None, None), kept=False):
    for bi, name in enumerate(("lw", "sw")):
        if edges[bi] is None:
            assert got[name]["points"].shape == (k.ncol, 0, K_PIPE) and got[name]["map"] is None
            continue
        tau = k.tau_gas(pipe, bi)
        kind, row = key_of(keys[bi])
        m = class_map(tau, kind, PIPE_CLASSES, row)
        if kept:
            assert got[name]["map"].dtype == np.uint16 and np.array_equal(got[name]["map"], m), name
        want = mapped_rows(tau, m, k.bands[bi].dw, edges[bi], K_PIPE, weights[bi])
        assert got[name]["tau"].shape == (k.ncol, L, len(edges[bi]) - 1, K_PIPE)
        assert_equals_model([got[name][x] for x in NAMES], want, (name, keys[bi]))
        assert got[name]["points"].sum() == k.ncol * sum(b - a + 1 for a, b in zip(edges[bi][:-1], edges[bi][1:]))
        assert np.count_nonzero(got[name]["points"].sum(axis=(0, 1))) >= 3, "the classes do not spread the band's tau"


@pytest.fixture(scope="module")
def reference_case(bands, device):
    """the reference's operation order, spectra kept, two columns: shared by the cases that leave it as they found it"""
    k = Case(bands, device, 0, True, 2)
    yield k
    k.close()


# ---- 6. the pipeline --------------------------------------------------------------------------------------------------------- #
def test_pipeline_in_reference_order_equals_the_model(reference_case, bands, lib, device):
    k = reference_case
    edges = pipe_edges(bands)
    api.profile_enable(True)
    api.profile_read(api.TAG_KDIST_MAP, reset=True)
    try:
        for keys in ((("sum",), ("layer", L - 1)), (("layer", 0), ("sum",))):
            k.pipe.run_kdist_correlated(k.gcols, PIPE_CLASSES, lw_edges=edges[0], sw_edges=edges[1], lw_key=keys[0],
                                        sw_key=keys[1], keep_map=True)
            got = k.pipe.kdist_correlated(k.ncol)
            assert_pipeline_equals_model(k, k.pipe, got, edges, keys, kept=True)
        launches = {tag: api.profile_read(tag)[1] for tag in SOLVER_TAGS + (api.TAG_KDIST,)}
        assert not any(launches.values()), launches
        assert api.profile_read(api.TAG_KDIST_MAP)[1] == 4 and api.profile_read(api.TAG_KDIST_MAPPED)[1] == 4
        # the maps in pipeline scratch: the same sums
        k.pipe.run_kdist_correlated(k.gcols, PIPE_CLASSES, lw_edges=edges[0], sw_edges=edges[1], lw_key=keys[0],
                                    sw_key=keys[1])
        scratch = k.pipe.kdist_correlated(k.ncol)
        assert_pipeline_equals_model(k, k.pipe, scratch, edges, keys)
        assert scratch["lw"]["map"] is None and scratch["sw"]["map"] is None
        # longwave bins alone: the shortwave band is not computed
        api.profile_read(api.TAG_GAS_SW, reset=True)
        k.pipe.run_kdist_correlated(k.gcols, PIPE_CLASSES, lw_edges=edges[0], lw_key=("layer", 1), keep_map=True)
        k.pipe.sync()
        idle = {tag: api.profile_read(tag)[1] for tag in SOLVER_TAGS + (api.TAG_GAS_SW, api.TAG_FAR_SW, api.TAG_KDIST)}
        assert not any(idle.values()), idle
        assert api.profile_read(api.TAG_GAS_LW)[1] >= 1
        assert api.profile_read(api.TAG_KDIST_MAP)[1] == 1 and api.profile_read(api.TAG_KDIST_MAPPED)[1] == 1
        assert_pipeline_equals_model(k, k.pipe, k.pipe.kdist_correlated(k.ncol), [edges[0], None], (("layer", 1), None),
                                     kept=True)
    finally:
        api.profile_enable(False)


def test_production_form_with_one_column_and_run_kdist_next(bands, lib, device):
    """fast = 3, no spectra kept, one column, a weight on the shortwave; then run_kdist gives what it gives on a fresh
    pipeline (the deterministic mode makes two gas-optics passes comparable)."""
    k = Case(bands, device, 3, False, 1)
    edges = pipe_edges(bands)
    weights = (None, np.asarray(k.solar, dtype=np.float64))
    keys = (("layer", L - 1), ("sum",))
    _deterministic(lib, True)
    try:
        k.pipe.run_kdist_correlated(k.gcols, PIPE_CLASSES, lw_edges=edges[0], sw_edges=edges[1], lw_key=keys[0],
                                    sw_key=keys[1], sw_weight=weights[1], keep_map=True)
        got = k.pipe.kdist_correlated(k.ncol)
        assert_pipeline_equals_model(k, k.pipe, got, edges, keys, weights, kept=True)
        k.pipe.run_kdist(k.gcols, PIPE_CLASSES, lw_edges=edges[0], sw_edges=edges[1], sw_weight=weights[1])
        after = k.pipe.kdist(k.ncol)
        fresh = k.make(False)
        fresh.run_kdist(k.gcols, PIPE_CLASSES, lw_edges=edges[0], sw_edges=edges[1], sw_weight=weights[1])
        want = fresh.kdist(k.ncol)
        for name in ("lw", "sw"):
            assert_equals_model([after[name][x] for x in NAMES], [want[name][x] for x in NAMES], name)
        # the key layer's own correlated sums are its plain ones
        assert same_bits(got["lw"]["tau"][:, L - 1], after["lw"]["tau"][:, L - 1])
        assert np.array_equal(got["lw"]["points"], after["lw"]["points"][:, L - 1])
    finally:
        _deterministic(lib, False)
        k.close()


# ---- 7. g-class fluxes ------------------------------------------------------------------------------------------------------- #
def test_g_class_fluxes_of_the_spectral_rows(reference_case, bands, lib, device):
    k = reference_case
    nl, ns = bands[0].nw, bands[1].nw
    dw = bands[0].dw
    edges = pipe_edges(bands)[0]
    k.pipe.run_kdist_correlated(k.gcols, PIPE_CLASSES, lw_edges=edges, keep_map=True)
    m = k.pipe.kdist_correlated(k.ncol)["lw"]["map"]
    k.pipe.run_spectral(k.gcols, lw_edges=edges)
    sp = k.pipe.spectral(k.ncol)
    rows, bins = sp["lw"][:, 0], sp["lw_bins"][:, 0]            # [ncol][6][n], [ncol][6][bins]
    points, weight, flux = api.kdist_mapped_rows(device, k.pipe.buffers["spectral"].ptr, 6 * (nl + ns),
                                                 k.pipe.buffers["kdist_corr.lw.map"].ptr, k.ncol, 6, nl, dw, K_PIPE, edges)
    assert_equals_model((points, weight, flux), mapped_rows(rows, m, dw, edges, K_PIPE), "g-class fluxes")
    assert np.any(flux != 0.0)
    for c in range(k.ncol):
        for r in range(6):
            for b, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
                w = np.full(hi - lo + 1, dw)
                w[0] = w[-1] = 0.5 * dw
                bound = 2 * (hi - lo + 1 + K_PIPE) * 2.0 ** -53 * math.fsum(np.abs(w * rows[c, r, lo:hi + 1]))
                total = math.fsum(flux[c, r, b])
                assert abs(total - bins[c, r, b]) <= bound, (c, r, b, total, bins[c, r, b], bound)


# ---- 8. refusals that need a device or a pipeline -------------------------------------------------------------------------- #
def test_refused_pipeline_calls_and_the_wrong_lane(bands, lib, device):
    ncol = 2
    k = Case(bands, device, 0, False, ncol, lw_only=True)
    narrow = k.make(False, max_columns=1)             # (for a batch of more columns than it was made for)
    nl = bands[0].nw
    edges = pipe_edges(bands)[0]
    count = ncol * L * 3 * K_PIPE + 64
    sent = [_sentinel(device, count) for _ in range(3)]
    map_sent = _sentinel(device, ncol * nl // 4 + 64)

    def run(pipe=None, gcols=None, lw=edges, sw=None, key=(api.KDIST_KEY_SUM, 0), keys=True, own_map=True):
        gk, _keep = api.make_kdist(PIPE_CLASSES, lw, sw)
        for band in (gk.lw, gk.sw):
            band.points_dev, band.weight_dev, band.tau_dev = (b.ptr for b in sent)
        ks = api.GrtKdistKeys()
        ks.lw.kind, ks.lw.layer = key
        ks.lw.map_dev = map_sent.ptr if own_map else None
        ks.sw.kind, ks.sw.layer, ks.sw.map_dev = api.KDIST_KEY_SUM, 0, None
        return lib.grt_pipeline_run_kdist_correlated((pipe or k.pipe).p, C.byref(gcols if gcols is not None else k.gcols),
                                                     C.byref(gk), C.byref(ks) if keys else None)

    none, _keep_none = api.make_columns(k.cols, MOL_ORDER, cfc_order=(0, 1))
    none.ncol = 0
    cases = {
        "NULL keys": lambda: run(keys=False),
        "key kind 2": lambda: run(key=(2, 0)),
        "key kind -1": lambda: run(key=(-1, 0)),
        "layer -1": lambda: run(key=(api.KDIST_KEY_ROW, -1)),
        "layer L": lambda: run(key=(api.KDIST_KEY_ROW, L)),
        "layer L, map in scratch": lambda: run(key=(api.KDIST_KEY_ROW, L), own_map=False),
        "bins for a band the pipeline lacks": lambda: run(sw=[0, 5, 9]),
        "no bins in either band": lambda: run(lw=None),
        "edges beyond the grid": lambda: run(lw=[0, 5, nl]),
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
                k.pipe.run_kdist_correlated(k.gcols, PIPE_CLASSES, lw_edges=edges)
        finally:
            api.use_lane(device, 0)
        api.device_synchronize(device)
        for tag in (api.TAG_KDIST_MAP, api.TAG_KDIST_MAPPED, api.TAG_GAS_LW):
            assert api.profile_read(tag)[1] == 0, tag
        for b in sent + [map_sent]:
            assert np.all(b.to_host(b.nbytes // 8) == -7.25)
        # ... and the call they all fall short of is taken (the layer with SUM is ignored)
        assert run(key=(api.KDIST_KEY_SUM, 99)) == 0
        k.pipe.sync()
        assert api.profile_read(api.TAG_KDIST_MAP)[1] == 1 and api.profile_read(api.TAG_KDIST_MAPPED)[1] == 1
        tau = k.tau_gas(k.pipe, 0)
        m = class_map(tau, KEY_SUM, PIPE_CLASSES)
        assert np.array_equal(map_sent.to_host((ncol, nl), dtype=np.uint16), m)
        want = mapped_rows(tau, m, bands[0].dw, edges, K_PIPE)
        assert np.array_equal(sent[0].to_host((ncol, 3, K_PIPE), dtype=np.int32), want[0])
        assert same_bits(sent[2].to_host((ncol, L, 3, K_PIPE)), want[2])
    finally:
        api.profile_enable(False)
        for b in sent + [map_sent]:
            b.free()
        k.close()
