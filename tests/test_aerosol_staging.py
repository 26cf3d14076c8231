"""The host staging of grt_pipeline_run_aerosols (no GPU needed): each grid point's interval of the aerosol grid and the
slope and intercept tables, against a NumPy restatement of interpolate2 / linear_sample that the oracle's interp_to_grid
judges first."""
import ctypes as C

import numpy as np
import pytest

from aerosol_model import interval_map, numpy_interp, slope_tables

c_double_p = C.POINTER(C.c_double)

# spectral grid 100, 102, .. 198 cm-1 (50 points, all exactly representable)
W0, DW, NW = 100.0, 2.0, 50
GRIDS = {
    "starts on a grid point": np.array([100.0, 111.0, 150.0, 177.5]),          # w = x[0]: no aerosol there
    "inner point on a grid point": np.array([95.0, 120.0, 121.0, 160.0, 250.0]),   # w = 120 = x[1]: interval 0
    "ends on a grid point": np.array([131.0, 140.5, 198.0]),                   # w = 198 = x[NA-1]: the last interval
    "wholly below": np.array([10.0, 50.0, 99.0]),
    "wholly above": np.array([198.5, 300.0]),
    "wider than the grid": np.array([1.0, 1000.0]),                            # NA = 2
    "two points inside": np.array([133.0, 135.0]),                             # NA = 2, one grid point in the interval
    "more points than the grid": np.linspace(90.3, 210.7, 131),
}


def staged(lib, x, optics, L):
    ncol, na = optics.shape[0], x.size
    interval = np.full(NW, 77, dtype=np.int32)
    tables = np.full((ncol, 3, na - 1, 2, L), np.nan)
    lib.grt_aerosol_interval_map.restype = None
    lib.grt_aerosol_tables.restype = None
    lib.grt_aerosol_interval_map(C.c_double(W0), C.c_double(DW), C.c_uint64(NW), x.ctypes.data_as(c_double_p), C.c_int(na),
                                 interval.ctypes.data_as(C.POINTER(C.c_int)))
    lib.grt_aerosol_tables(x.ctypes.data_as(c_double_p), C.c_int(na), C.c_int(ncol), C.c_int(L),
                           optics.ctypes.data_as(c_double_p), tables.ctypes.data_as(c_double_p))
    return interval, tables


@pytest.mark.parametrize("name", list(GRIDS))
def test_interval_map_and_tables(lib, oracle, name):
    x = np.ascontiguousarray(GRIDS[name])
    ncol, L, na = 2, 3, x.size
    rng = np.random.default_rng(na)
    optics = np.ascontiguousarray(rng.random((ncol, 3, L, na)) + 0.1)
    # the oracle judges the restatement: same covered points, same values
    for y in (optics[0, 0, 0], optics[1, 2, 1]):
        want = oracle.interp_to_grid(W0, DW, NW, x, y, constant_extrap=False)
        got = numpy_interp(W0, DW, NW, x, y)
        assert np.array_equal(want != 0.0, got != 0.0)
        assert np.max(np.abs(want - got)) <= 4 * np.finfo(float).eps * np.abs(y).max() * (1 + np.abs(x).max() / np.diff(x).min())
    want_map, w = interval_map(W0, DW, NW, x)
    interval, tables = staged(lib, x, optics, L)
    assert np.array_equal(interval, want_map)
    assert np.array_equal(tables, slope_tables(x, optics))           # the reference's two expressions: the same doubles
    # the named edges
    if name == "starts on a grid point":
        assert interval[0] == -1 and interval[1] == 0
    if name == "inner point on a grid point":
        assert interval[10] == 0 and interval[11] == 2 and w[10] == x[1]
    if name == "ends on a grid point":
        assert interval[-1] == na - 2 and np.all(interval[:16] == -1)
    if name in ("wholly below", "wholly above"):
        assert np.all(interval == -1)
    if name == "wider than the grid":
        assert np.all(interval == 0)
    if name == "two points inside":
        assert np.count_nonzero(interval == 0) == 1 and interval[17] == 0
    # what a kernel thread computes from the two: the restatement's values
    jj = np.where(interval < 0, 0, interval)
    val = np.where(interval < 0, 0.0, tables[1, 2, jj, 0, 1] * w + tables[1, 2, jj, 1, 1])
    assert np.array_equal(val, numpy_interp(W0, DW, NW, x, optics[1, 2, 1]))
