"""The window table of instrument channels and spectral responses (grt_kernels.h, "The window table"), built on the host by
grt_window_table and sized by grt_window_table_ints: every int against a numpy restatement of that comment, on windows
inside one solver block, across a block edge, over the whole grid, in the last block, identical and overlapping, with
blocks that hold none, 256 of one point each, and on a grid of one point; and what both kinds of window are refused for,
kind by kind (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api

BLOCK = 128             # GRT_SOLVER_BLOCK
INTS = 5                # GRT_WINDOW_INTS
c_int_p = C.POINTER(C.c_int)

# name: (grid points, first, points per window)
CASES = {
    "one point": (257, [5], [1]),
    "across a block edge": (257, [127], [2]),
    "the whole grid": (257, [0], [257]),
    "the last block": (257, [256], [1]),
    "four windows, 3 + 2 + 1 + 1 pairs": (257, [0, 127, 128, 0], [257, 2, 1, 128]),
    "two identical windows": (257, [3, 3], [4, 4]),
    "blocks 1 .. 6 empty": (1000, [10, 900, 20], [5, 50, 100]),
    "256 windows of one point": (257, list(range(256)), [1]*256),
    "a grid of one point": (1, [0], [1]),
}


def restated(n, first, counts):
    """-> (entry [N][5], block_start [nblocks + 1], block_list [pairs]) as the comment in grt_kernels.h lays them out"""
    nblocks = (n + BLOCK - 1)//BLOCK
    first, counts = np.asarray(first), np.asarray(counts)
    lo, hi = first//BLOCK, (first + counts - 1)//BLOCK
    offset = np.concatenate(([0], np.cumsum(counts)))[:-1]
    first_pair = np.concatenate(([0], np.cumsum(hi - lo + 1)))[:-1]
    entry = np.stack([first, counts, offset, lo, first_pair], axis=1)
    lists = [[k for k in range(first.size) if lo[k] <= b <= hi[k]] for b in range(nblocks)]
    block_start = np.concatenate(([0], np.cumsum([len(l) for l in lists])))
    return entry, block_start, np.array([k for l in lists for k in l], dtype=np.int64)


def built(lib, n, first, counts):
    """-> grt_window_table's ints for these windows, as (entry, block_start, block_list, nblocks, pairs)"""
    first = np.ascontiguousarray(first, dtype=np.int32)
    offset = np.ascontiguousarray(np.concatenate(([0], np.cumsum(counts))), dtype=np.int32)
    nblocks = (n + BLOCK - 1)//BLOCK
    g, keep = api.make_responses(sw=(first, [np.ones(c) for c in counts]))
    pairs = api.response_pair_count(g, 1, n)
    lib.grt_window_table_ints.restype = C.c_size_t
    lib.grt_window_table.restype = None
    ints = lib.grt_window_table_ints(C.c_int(first.size), C.c_size_t(nblocks), C.c_longlong(pairs))
    assert ints == INTS*first.size + nblocks + 1 + pairs
    table = np.full(ints + 8, -77, dtype=np.int32)          # (eight more: nothing is written behind the table)
    lib.grt_window_table(first.ctypes.data_as(c_int_p), offset.ctypes.data_as(c_int_p), C.c_int(first.size),
                         C.c_size_t(nblocks), table.ctypes.data_as(c_int_p))
    assert (table[ints:] == -77).all()
    at = INTS*first.size
    return table[:at].reshape(first.size, INTS), table[at:at + nblocks + 1], table[at + nblocks + 1:ints], nblocks, pairs


@pytest.mark.parametrize("name", list(CASES))
def test_every_int_is_the_layouts(lib, name):
    n, first, counts = CASES[name]
    entry, block_start, block_list, nblocks, pairs = built(lib, n, first, counts)
    want_entry, want_start, want_list = restated(n, first, counts)
    assert (entry == want_entry).all()
    assert (block_start == want_start).all()
    assert (block_list == want_list).all()


@pytest.mark.parametrize("name", list(CASES))
def test_pairs_and_lists(lib, name):
    n, first, counts = CASES[name]
    entry, block_start, block_list, nblocks, pairs = built(lib, n, first, counts)
    weights = [np.ones(c) for c in counts]
    for band, kw in ((0, "lw"), (1, "sw")):
        g, keep = api.make_responses(**{kw: (first, weights)})
        assert api.response_pair_count(g, band, n) == pairs
    g, keep = api.make_channels(first, weights)
    assert api.channel_pair_count(g, n) == pairs
    assert block_start[0] == 0 and block_start[nblocks] == pairs == block_list.size
    for b in range(nblocks):
        mine = block_list[block_start[b]:block_start[b + 1]]
        assert (np.diff(mine) > 0).all(), b
    blocks = (entry[:, 0] + entry[:, 1] - 1)//BLOCK - entry[:, 3] + 1
    assert (entry[:, 4] + (blocks - 1) < pairs).all()
    assert blocks.sum() == pairs


def test_the_expected_pairs_of_the_hand_cases(lib):
    assert built(lib, *CASES["four windows, 3 + 2 + 1 + 1 pairs"])[4] == 3 + 2 + 1 + 1
    entry, block_start, block_list, nblocks, pairs = built(lib, *CASES["blocks 1 .. 6 empty"])
    assert nblocks == 8 and pairs == 3
    assert list(block_start) == [0, 2, 2, 2, 2, 2, 2, 2, 3]            # (flat over the blocks that hold no window)
    assert built(lib, *CASES["256 windows of one point"])[4] == 256


# ---- what every window set is refused for, whichever kind it is ------------------------------------------------------------ #
def pointers(first, offset, weights, null):
    """the three fields as ctypes pointers (`null`: that one NULL), and the arrays they point into"""
    arrays = {"first": np.ascontiguousarray(first, dtype=np.int32), "offset": np.ascontiguousarray(offset, dtype=np.int32),
              "weights": np.ascontiguousarray(weights, dtype=np.float64)}
    ptr = {k: None if k == null else v.ctypes.data_as(c_int_p if v.dtype == np.int32 else C.POINTER(C.c_double))
           for k, v in arrays.items()}
    return [ptr["first"], ptr["offset"], ptr["weights"]], arrays


def channel_count(first, offset, weights, n, null=None, count=None):
    fields, arrays = pointers(first, offset, weights, null)
    return api.channel_pair_count(api.GrtChannels(len(first) if count is None else count, *fields, None, None, None), n)


def response_count(band, first, offset, weights, n, null=None, count=None, ask=None):
    """the pairs of the windows as band `band`'s responses, the other band having none (ask: the band asked for)"""
    fields, arrays = pointers(first, offset, weights, null)
    mine, none = [len(first) if count is None else count] + fields, [0, None, None, None]
    g = api.GrtResponses(*(mine + none if band == 0 else none + mine), None, None)
    return api.response_pair_count(g, band if ask is None else ask, n)


GOOD = dict(first=[5, 9], offset=[0, 2, 5], weights=[1.0, 2.0, 1.0, 0.5, 1.0], n=257)
REFUSED = {
    "first NULL": dict(null="first"),
    "offset NULL": dict(null="offset"),
    "weights NULL": dict(null="weights"),
    "offset[0] not 0": dict(offset=[1, 2, 5]),
    "offset not increasing": dict(offset=[0, 2, 2]),
    "offset decreasing": dict(offset=[0, 3, 2]),
    "first below 0": dict(first=[-1, 9]),
    "a window past the grid": dict(first=[5, 255]),
    "a window behind the grid": dict(first=[5, 257]),
    "a NaN weight": dict(weights=[1.0, np.nan, 1.0, 0.5, 1.0]),
    "an infinite weight": dict(weights=[1.0, 2.0, 1.0, 0.5, np.inf]),
    "a negative infinite weight": dict(weights=[-np.inf, 2.0, 1.0, 0.5, 1.0]),
}


def test_the_good_windows_count(lib):
    assert channel_count(**GOOD) == 2
    assert response_count(0, **GOOD) == 2 and response_count(1, **GOOD) == 2


@pytest.mark.parametrize("name", list(REFUSED))
def test_both_kinds_are_refused_alike(lib, name):
    case = dict(GOOD, **REFUSED[name])
    assert channel_count(**case) == -1
    assert response_count(0, **case) == -1 and response_count(1, **case) == -1


# ---- what each kind checks of its own, around the shared check: the count, the grid, the struct, the band ------------------- #
@pytest.mark.parametrize("null", [None, "first", "offset", "weights"])
def test_the_count_limits_of_each_kind(lib, null):
    for count in (0, -1, api.GRT_MAX_CHANNELS + 1):
        assert channel_count(**GOOD, null=null, count=count) == -1, count
    for band in (0, 1):
        for count in (-1, api.GRT_MAX_RESPONSES + 1):
            assert response_count(band, **GOOD, null=null, count=count) == -1, (band, count)
        assert response_count(band, **GOOD, null=null, count=0) == 0            # (no responses: nothing, whatever the fields)


def test_the_most_windows_of_each_kind(lib):
    for most, count in ((api.GRT_MAX_CHANNELS, channel_count), (api.GRT_MAX_RESPONSES, lambda **kw: response_count(1, **kw))):
        assert count(first=np.arange(most), offset=np.arange(most + 1), weights=np.ones(most), n=most) == most


@pytest.mark.parametrize("null", [None, "first", "offset", "weights"])
@pytest.mark.parametrize("n", [0, -3])
def test_no_grid(lib, n, null):
    case = dict(GOOD, n=n, null=null)
    assert channel_count(**case) == -1
    assert response_count(0, **case) == -1 and response_count(1, **case) == -1
    assert response_count(1, **dict(case, count=0)) == -1 and response_count(0, **case, ask=1) == -1


def test_a_null_struct_and_a_band_that_is_none(lib):
    assert lib.grt_channel_pair_count(None, 257) == -1
    for band in (0, 1):
        assert lib.grt_response_pair_count(None, band, 257) == -1
    for ask in (-1, 2):
        assert response_count(1, **GOOD, ask=ask) == -1
    assert response_count(1, **GOOD, ask=0) == 0 and response_count(0, **GOOD, ask=1) == 0      # (the other band has none)
