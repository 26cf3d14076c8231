"""What the tests of grt_pipeline_set_surface share: the library's own host interpolate_to_grid(..., linear_sample,
constant_extrapolation) as the reference for a column's surface row, the host staging functions behind ctypes, and the
rows a kernel thread forms from their tables."""
import ctypes as C

import numpy as np

from grtcode_amd import api

c_double_p = C.POINTER(C.c_double)


def host_rows(lib, grid, x, values):
    """[ncol][n]: each column's values [ncol][NS] on `grid` (api.SpectralGrid) by the library's host interpolate_to_grid with
    linear_sample and constant_extrapolation -- driver.c:101-117's call."""
    x, values = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(values, dtype=np.float64)
    lib.interpolate_to_grid.argtypes = [api.SpectralGrid, c_double_p, c_double_p, C.c_size_t, c_double_p, C.c_void_p,
                                        C.c_void_p]
    interp, extrap = (C.cast(f, C.c_void_p) for f in (lib.linear_sample, lib.constant_extrapolation))
    out = np.full((values.shape[0], grid.n), np.nan)
    for c, y in enumerate(values):
        api.check(lib.interpolate_to_grid(grid, x.ctypes.data_as(c_double_p), y.ctypes.data_as(c_double_p), x.size,
                                          out[c].ctypes.data_as(c_double_p), interp, extrap))
    return out


def staged(lib, grid, x, values):
    """-> (entry [n] int32, tables [ncol][NS + 1][2]) of grt_surface_entry_map and grt_surface_tables"""
    x, values = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(values, dtype=np.float64)
    ncol, ns = values.shape
    entry = np.full(grid.n, -77, dtype=np.int32)
    tables = np.full((ncol, ns + 1, 2), np.nan)
    lib.grt_surface_entry_map.restype = None
    lib.grt_surface_tables.restype = None
    lib.grt_surface_entry_map(C.c_double(grid.w0), C.c_double(grid.dw), C.c_uint64(grid.n), x.ctypes.data_as(c_double_p),
                              C.c_int(ns), entry.ctypes.data_as(C.POINTER(C.c_int)))
    lib.grt_surface_tables(x.ctypes.data_as(c_double_p), C.c_int(ns), C.c_int(ncol), values.ctypes.data_as(c_double_p),
                           tables.ctypes.data_as(c_double_p))
    return entry, tables


def thread_rows(grid, entry, tables):
    """What spread_surface_kernel's threads store: slope x w, rounded, then + intercept, w = w0 + i dw."""
    w = grid.w0 + np.arange(grid.n, dtype=np.uint64).astype(np.float64) * grid.dw
    product = tables[:, entry, 0] * w[None, :]
    return product + tables[:, entry, 1]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))
