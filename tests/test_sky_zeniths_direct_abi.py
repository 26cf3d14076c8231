"""grt_pipeline_run_sky_zeniths_direct's C ABI and host staging (no GPU needed): the symbol and its nine arguments, the two
grt_sizeof kinds and ctypes structs in the header's field order, the open-water albedo helper, make_zenith_surface's shapes,
and the staged pairs of [ncol][Z] knot rows against grt_surface_tables called row by row."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from grtcode_amd import api, surfaces
from surface_support import same_bits, staged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def fields_of(src, tag):
    body = re.search(rf"typedef struct {tag}\s*\{{(.*?)\}}\s*{tag}_t;", src, re.S)
    assert body, f"{tag}_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";")]
    return [re.search(r"(\w+)$", d).group(1) for d in decls if d]


def test_the_entry_point_is_exported_and_declared(lib):
    for name in ("grt_pipeline_run_sky_zeniths_direct", "grt_zenith_surface_tables"):
        assert name in api.EXPORTS and hasattr(lib, name), name
    assert len(lib.grt_pipeline_run_sky_zeniths_direct.argtypes) == 9
    m = re.search(r"EXTERN int grt_pipeline_run_sky_zeniths_direct\(([^;]*)\);", header("include", "grt_ext.h"))
    assert m, "grt_pipeline_run_sky_zeniths_direct is not declared in grt_ext.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9
    for a, kind in zip(args[1:6], ("GrtColumns_t", "GrtSky_t", "GrtZeniths_t", "GrtZenithSurface_t", "GrtZenithDirect_t")):
        assert a.startswith(kind + " const *"), a
    assert all(a.startswith("fp_t *") for a in args[6:])


def test_sizes_and_layouts(lib):
    src = header("include", "grt_ext.h")
    kinds = [k.strip() for k in re.search(r"enum grt_struct_kind\s*\{(.*?)\}", src, re.S).group(1).replace("= 0", "").split(",")]
    more = re.search(r"enum grt_struct_kind_more\s*\{\s*GRT_ZENITH_SURFACE = GRT_LW_SCATTER \+ 1, GRT_ZENITH_DIRECT\s*\}", src)
    assert more and kinds[-1] == "GRT_LW_SCATTER"
    assert (api.GRT_ZENITH_SURFACE, api.GRT_ZENITH_DIRECT) == (len(kinds), len(kinds) + 1)
    assert lib.grt_sizeof(api.GRT_ZENITH_SURFACE) == C.sizeof(api.GrtZenithSurface) > 0
    assert lib.grt_sizeof(api.GRT_ZENITH_DIRECT) == C.sizeof(api.GrtZenithDirect) == 4 * C.sizeof(C.c_void_p)
    assert fields_of(src, "GrtZenithSurface") == [f[0] for f in api.GrtZenithSurface._fields_]
    assert fields_of(src, "GrtZenithDirect") == [f[0] for f in api.GrtZenithDirect._fields_]
    want = {"albedo_num_points": C.c_int, "albedo_grid": api.c_double_p, "direct_albedo": api.c_double_p}
    assert all(want[n] is t for n, t in api.GrtZenithSurface._fields_)
    assert all(t is C.c_void_p for _, t in api.GrtZenithDirect._fields_)


def test_ocean_direct_albedo():
    assert abs(surfaces.ocean_direct_albedo(1.0) - 0.0296) < 1e-15
    assert surfaces.ocean_direct_albedo(0.0) == 0.037 / 0.15
    mu = np.array([[1.0, 0.5, 0.0, -0.3]])
    a = surfaces.ocean_direct_albedo(mu)
    assert a.shape == mu.shape and np.all(np.diff(a[0, :3]) > 0.0) and a[0, 3] == a[0, 2]
    assert a[0, 1] == 0.037 / (1.1 * 0.5 ** 1.4 + 0.15) and np.all((a >= 0.0) & (a <= 1.0))


def test_make_zenith_surface_shapes():
    grid = np.array([500.0, 2000.0, 9000.0])
    knots = np.random.default_rng(3).uniform(0.0, 1.0, (4, 5, 3))
    gs, keep = api.make_zenith_surface(grid, knots)
    assert gs.albedo_num_points == 3 and keep["shape"] == (4, 5)
    assert np.array_equal(np.ctypeslib.as_array(gs.direct_albedo, shape=(4, 5, 3)), knots)
    assert np.array_equal(np.ctypeslib.as_array(gs.albedo_grid, shape=(3,)), grid)
    for bad_grid, bad_knots in ((grid[:1], knots[:, :, :1]), (grid, knots[:, :, :2]), (grid, knots[0]), (grid.reshape(1, 3), knots)):
        with pytest.raises(ValueError):
            api.make_zenith_surface(bad_grid, bad_knots)
    assert all(callable(getattr(api.Pipeline, name)) for name in (
        "run_sky_zeniths_direct", "sky_zenith_direct_fluxes", "sky_zenith_direct_profiles"))


@pytest.mark.parametrize("ncol,Z,ns", [(1, 1, 2), (3, 5, 3), (2, 64, 9)])
def test_staged_tables_are_grt_surface_tables_row_by_row(lib, ncol, Z, ns):
    grid = api.create_spectral_grid(1000.0, 3560.0, 10.0)
    x = np.linspace(1203.0, 2900.0, ns)
    x[ns - 1] = 2900.0 + 10.0 / 3.0
    values = np.random.default_rng(ns + Z).uniform(0.0, 1.0, (ncol, Z, ns))
    values[0, 0, 0], values[-1, -1, -1] = 0.0, 1.0
    tables = np.full((ncol, Z, ns + 1, 2), np.nan)
    by_angle = np.full((Z, ncol, ns + 1, 2), np.nan)
    p = api.c_double_p
    lib.grt_zenith_surface_tables(x.ctypes.data_as(p), ns, ncol, Z, values.ctypes.data_as(p), tables.ctypes.data_as(p),
                                  by_angle.ctypes.data_as(p))
    for c in range(ncol):
        for k in range(Z):
            entry, row = staged(lib, grid, x, values[c, k:k + 1])
            assert same_bits(tables[c, k], row[0]), (c, k)
            assert same_bits(by_angle[k, c], row[0]), (c, k)
    only = np.full((ncol, Z, ns + 1, 2), np.nan)
    lib.grt_zenith_surface_tables(x.ctypes.data_as(p), ns, ncol, Z, values.ctypes.data_as(p), only.ctypes.data_as(p), None)
    assert same_bits(only, tables)
