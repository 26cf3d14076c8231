"""The aerosol entry point's C ABI: exported, declared with its six arguments, its profile tags documented, and
make_aerosols' packing (no GPU needed)."""
import os
import re

import numpy as np
import pytest

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "grt_ext.h")).read()


def test_run_aerosols_is_exported(lib):
    assert "grt_pipeline_run_aerosols" in api.EXPORTS
    assert hasattr(lib, "grt_pipeline_run_aerosols")
    assert len(lib.grt_pipeline_run_aerosols.argtypes) == 6


def test_run_aerosols_is_declared():
    m = re.search(r"EXTERN int grt_pipeline_run_aerosols\(([^;]*)\);", _header())
    assert m, "grt_pipeline_run_aerosols is not declared in grt_ext.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 6
    assert args[0].startswith("GrtPipeline_t *") and args[1].startswith("GrtColumns_t const *")
    assert args[2].startswith("GrtAerosols_t const *") and all(a.startswith("fp_t *") for a in args[3:])
    s = re.search(r"typedef struct GrtAerosols\s*\{(.*?)\}\s*GrtAerosols_t;", _header(), re.S)
    assert s
    body = re.sub(r"/\*.*?\*/", "", s.group(1), flags=re.S)
    assert re.search(r"int\s+lw_num_points,\s*sw_num_points;", body)
    assert re.search(r"fp_t const \*lw_grid, \*sw_grid;", body) and re.search(r"fp_t const \*lw_optics, \*sw_optics;", body)


def test_profile_tags_are_documented():
    assert re.search(r"12 / 13 = LW / SW solver of the aerosol pass", _header())


def test_struct_layout_matches_the_header_order():
    assert [f[0] for f in api.GrtAerosols._fields_] == ["lw_num_points", "sw_num_points", "lw_grid", "sw_grid", "lw_optics",
                                                       "sw_optics"]


def test_make_aerosols_packs_bands_and_refuses_a_one_point_grid():
    ncol, L, na = 2, 5, 4
    grid = np.array([10.0, 20.0, 45.0, 50.0])
    optics = np.zeros((ncol, 3, L, na))
    g, keep = api.make_aerosols(lw=(grid, optics), sw=None)
    assert (g.lw_num_points, g.sw_num_points) == (na, 0) and keep["num_points"] == (na, 0)
    assert keep["shapes"] == ((ncol, 3, L, na), None)
    assert not g.sw_grid and not g.sw_optics and g.lw_grid and g.lw_optics
    g, keep = api.make_aerosols(lw=None, sw=(grid[:2], optics[..., :2]))
    assert (g.lw_num_points, g.sw_num_points) == (0, 2) and keep["shapes"] == (None, (ncol, 3, L, 2))
    g, keep = api.make_aerosols()
    assert keep["num_points"] == (0, 0)
    with pytest.raises(ValueError):
        api.make_aerosols(lw=(grid[:1], optics[..., :1]))
    with pytest.raises(ValueError):
        api.make_aerosols(sw=(grid, optics[..., :3]))
