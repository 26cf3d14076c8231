"""The subcolumn entry point's C ABI: exported, declared with its seven arguments, and its subcolumn cap known to Python
(no GPU needed)."""
import os
import re

import numpy as np

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "grt_ext.h")).read()


def test_run_subcolumns_is_exported(lib):
    assert "grt_pipeline_run_subcolumns" in api.EXPORTS
    assert hasattr(lib, "grt_pipeline_run_subcolumns")
    assert len(lib.grt_pipeline_run_subcolumns.argtypes) == 7


def test_run_subcolumns_is_declared():
    m = re.search(r"EXTERN int grt_pipeline_run_subcolumns\(([^;]*)\);", _header())
    assert m, "grt_pipeline_run_subcolumns is not declared in grt_ext.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 7
    assert args[3].startswith("int ") and all(a.startswith("fp_t *") for a in args[4:])
    assert re.search(r"11 = the subcolumn-mean kernel", _header())


def test_max_subcolumns_matches_the_header():
    m = re.search(r"#define GRT_MAX_SUBCOLUMNS (\d+)", _header())
    assert m and int(m.group(1)) == api.GRT_MAX_SUBCOLUMNS == 64


def test_make_clouds_takes_subcolumn_sets():
    ncol, S, B, L = 2, 3, 4, 5
    lo, hi = np.arange(B, dtype=float), np.arange(B, dtype=float) + 1.0
    th = np.ones((ncol, L))
    one = np.zeros((ncol, 3, B, L))
    many = np.zeros((ncol, S, 3, B, L))
    g, keep = api.make_clouds((lo, hi), (lo, hi), th, one, one, one, one)
    assert keep["subcolumns"] == 1
    g, keep = api.make_clouds((lo, hi), (lo, hi), th, many, many, None, None)
    assert keep["subcolumns"] == S and g.num_liquid_bands == B
