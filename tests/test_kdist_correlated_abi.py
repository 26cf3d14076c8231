"""The correlated k-distribution entry points' C ABI: grt_kdist_class_map, grt_kdist_mapped_rows and
grt_pipeline_run_kdist_correlated exported and declared with their argument lists, GrtKdistKey_t and GrtKdistKeys_t field
for field the ctypes structures, the two key kinds and the two profile tags named once and equal to the Python module's,
both kernels in the build, the Python calls, and every refusal the host decides before it needs a device (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

from grtcode_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("grt_kdist_class_map", "grt_kdist_mapped_rows", "grt_pipeline_run_kdist_correlated")


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def declared(name, returns="int"):
    m = re.search(r"EXTERN %s %s\(([^;]*)\);" % (returns, name), header("include", "grt_ext.h"))
    assert m, f"{name} is not declared in grt_ext.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_three_functions_are_exported(lib):
    for name in NEW:
        assert name in api.EXPORTS and hasattr(lib, name), name
    assert list(lib.grt_kdist_class_map.argtypes) == [C.c_int, C.c_void_p, C.c_longlong, C.c_longlong, C.c_longlong,
                                                      C.c_int, C.c_longlong, C.c_int, C.POINTER(C.c_double), C.c_void_p]
    assert list(lib.grt_kdist_mapped_rows.argtypes) == [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p, C.c_longlong,
                                                        C.c_longlong, C.c_longlong, C.c_double, C.c_int,
                                                        C.POINTER(api.GrtKdistBand)]
    assert list(lib.grt_pipeline_run_kdist_correlated.argtypes) == [C.c_void_p, C.POINTER(api.GrtColumns),
                                                                    C.POINTER(api.GrtKdist), C.POINTER(api.GrtKdistKeys)]


def test_the_three_functions_are_declared_with_these_arguments():
    assert declared("grt_kdist_class_map") == ["Device_t device", "fp_t const *x_dev", "long long groups",
                                               "long long rows_per_group", "long long n", "int key_kind",
                                               "long long key_row", "int num_classes", "fp_t const *class_edges",
                                               "unsigned short *map_dev"]
    assert declared("grt_kdist_mapped_rows") == ["Device_t device", "fp_t const *values_dev", "long long group_stride",
                                                 "unsigned short const *map_dev", "long long groups",
                                                 "long long rows_per_group", "long long n", "fp_t dw", "int num_classes",
                                                 "GrtKdistBand_t const *band"]
    assert declared("grt_pipeline_run_kdist_correlated") == ["GrtPipeline_t *pipeline", "GrtColumns_t const *columns",
                                                             "GrtKdist_t const *kdist", "GrtKdistKeys_t const *keys"]


def struct_decls(name):
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s_t;" % (name, name), header("include", "grt_ext.h"), re.S)
    assert body, f"{name}_t is not declared in grt_ext.h"
    return [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if d.strip()]


def test_the_struct_layouts_match_ctypes():
    assert struct_decls("GrtKdistKey") == ["int kind", "int layer", "unsigned short *map_dev"]
    names = ["kind", "layer", "map_dev"]
    assert [f[0] for f in api.GrtKdistKey._fields_] == names
    assert [f[1] for f in api.GrtKdistKey._fields_] == [C.c_int, C.c_int, C.c_void_p]
    assert C.sizeof(api.GrtKdistKey) == 16
    assert [getattr(api.GrtKdistKey, n).offset for n in names] == [0, 4, 8]

    assert struct_decls("GrtKdistKeys") == ["GrtKdistKey_t lw, sw"]
    assert [f[0] for f in api.GrtKdistKeys._fields_] == ["lw", "sw"]
    assert [f[1] for f in api.GrtKdistKeys._fields_] == [api.GrtKdistKey, api.GrtKdistKey]
    assert C.sizeof(api.GrtKdistKeys) == 32
    assert [getattr(api.GrtKdistKeys, n).offset for n in ("lw", "sw")] == [0, 16]


def test_the_key_kinds_and_the_tags_are_named_once_and_equal_the_modules():
    text = header("include", "grt_ext.h")
    assert re.findall(r"GRT_KDIST_KEY_ROW = (\d+)", text) == ["0"] and api.KDIST_KEY_ROW == 0
    assert re.findall(r"GRT_KDIST_KEY_SUM = (\d+)", text) == ["1"] and api.KDIST_KEY_SUM == 1
    assert re.findall(r"GRT_TAG_KDIST_MAP = (\d+)", text) == ["30"] and api.TAG_KDIST_MAP == 30
    assert re.findall(r"GRT_TAG_KDIST_MAPPED = (\d+)", text) == ["31"] and api.TAG_KDIST_MAPPED == 31
    assert api.TAG_KDIST == 29 and api.TAG_GAS_LW == 1


def test_both_kernels_are_in_the_build():
    assert "k_kdist.hip" in build.HIP_SRC and "grt_kdist.c" in build.HOST_SRC
    src = header("grtcode_amd", "csrc", "hip", "k_kdist.hip")
    assert len(re.findall(r"__global__[^\n]*void kdist_map_kernel\(", src)) == 1
    assert len(re.findall(r"__global__[^\n]*void kdist_mapped_kernel\(", src)) == 1
    # phase 2 is stated once, as a device function that the plain and the mapped kernel both call
    assert len(re.findall(r"__device__[^\n]*void sum_chunk\(", src)) == 1 and len(re.findall(r"sum_chunk<NC>\(", src)) == 2
    assert "#pragma clang fp contract(off)" in src
    kernels = header("grtcode_amd", "csrc", "grt_kernels.h")
    for name in ("GrtKdistMapArgs", "GrtKdistMappedArgs", "grt_launch_kdist_map", "grt_launch_kdist_mapped"):
        assert name in kernels, name


def test_python_has_the_correlated_calls():
    for name in ("run_kdist_correlated", "kdist_correlated"):
        assert callable(getattr(api.Pipeline, name))
    assert callable(api.kdist_class_map) and callable(api.kdist_mapped_rows)
    from grtcode_amd import kdist
    assert callable(kdist.correlated_k_of_g)


# ---- refusals the host decides before it needs a device ------------------------------------------------------------------- #
FAKE = C.c_void_p(0x1000)       # a device pointer that no refused call may look behind


def class_map(lib, x=FAKE, groups=2, rows=3, n=10, kind=api.KDIST_KEY_SUM, key_row=0, ce=(0.1, 1.0, 10.0), K=None, out=FAKE):
    e = None if ce is None else np.ascontiguousarray(ce, dtype=np.float64)
    return lib.grt_kdist_class_map(0, x, groups, rows, n, kind, key_row, (e.size + 1 if e is not None else 4) if K is None else K,
                                   None if e is None else e.ctypes.data_as(api.c_double_p), out)


def mapped(lib, values=FAKE, stride=30, map_=FAKE, groups=2, rows=3, n=10, dw=0.5, K=4, edges=(0, 4, 9), weight=None,
           outs=(FAKE, FAKE, FAKE), band=True, num_bins=None):
    e = None if edges is None else np.ascontiguousarray(edges, dtype=np.int32)
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    b = api.GrtKdistBand(None if e is None else e.ctypes.data_as(api.c_int_p),
                         (e.size - 1 if e is not None else 2) if num_bins is None else num_bins,
                         None if w is None else w.ctypes.data_as(api.c_double_p), *outs)
    return lib.grt_kdist_mapped_rows(0, values, stride, map_, groups, rows, n, dw, K, C.byref(b) if band else None)


def test_refused_class_map_calls(lib):
    cases = {
        "NULL x_dev": lambda: class_map(lib, x=None),
        "NULL map_dev": lambda: class_map(lib, out=None),
        "NULL class edges": lambda: class_map(lib, ce=None),
        "K = 1": lambda: class_map(lib, ce=()),
        "K = 1025": lambda: class_map(lib, ce=np.logspace(-5, 1, 1024)),
        "class edges equal": lambda: class_map(lib, ce=(0.1, 0.1, 1.0)),
        "class edges falling": lambda: class_map(lib, ce=(0.1, 1.0, 0.5)),
        "class edge NaN": lambda: class_map(lib, ce=(0.1, np.nan, 1.0)),
        "class edge inf": lambda: class_map(lib, ce=(0.1, 1.0, np.inf)),
        "groups = 0": lambda: class_map(lib, groups=0),
        "rows = 0": lambda: class_map(lib, rows=0),
        "n = 1": lambda: class_map(lib, n=1),
        "kind 2": lambda: class_map(lib, kind=2),
        "kind -1": lambda: class_map(lib, kind=-1),
        "key row -1": lambda: class_map(lib, kind=api.KDIST_KEY_ROW, key_row=-1),
        "key row = rows": lambda: class_map(lib, kind=api.KDIST_KEY_ROW, key_row=3),
    }
    for name, call in cases.items():
        assert call() == api.VALUE_ERR, name


def test_refused_mapped_rows_calls(lib):
    bad = np.ones(10)
    bad[4] = -1.0
    cases = {
        "NULL values_dev": lambda: mapped(lib, values=None),
        "NULL map_dev": lambda: mapped(lib, map_=None),
        "NULL band": lambda: mapped(lib, band=False),
        "K = 1": lambda: mapped(lib, K=1),
        "K = 1025": lambda: mapped(lib, K=1025),
        "groups = 0": lambda: mapped(lib, groups=0),
        "rows = 0": lambda: mapped(lib, rows=0),
        "n = 1": lambda: mapped(lib, n=1, stride=3, edges=(0,)),
        "stride below rows x n": lambda: mapped(lib, stride=29),
        "stride 0": lambda: mapped(lib, stride=0),
        "stride negative": lambda: mapped(lib, stride=-30),
        "dw = 0": lambda: mapped(lib, dw=0.0),
        "dw < 0": lambda: mapped(lib, dw=-0.5),
        "dw NaN": lambda: mapped(lib, dw=float("nan")),
        "dw inf": lambda: mapped(lib, dw=float("inf")),
        "NULL edges": lambda: mapped(lib, edges=None),
        "negative bins": lambda: mapped(lib, num_bins=-1),
        "no bins": lambda: mapped(lib, edges=(0,)),
        "edges below the grid": lambda: mapped(lib, edges=(-1, 4, 9)),
        "edges beyond the grid": lambda: mapped(lib, edges=(0, 4, 10)),
        "edges equal": lambda: mapped(lib, edges=(0, 4, 4, 9)),
        "edges falling": lambda: mapped(lib, edges=(0, 6, 4, 9)),
        "no outputs": lambda: mapped(lib, outs=(None, None, None)),
        "weight negative": lambda: mapped(lib, weight=bad),
        "weight NaN": lambda: mapped(lib, weight=np.where(bad < 0, np.nan, bad)),
        "weight inf": lambda: mapped(lib, weight=np.where(bad < 0, np.inf, bad)),
    }
    for name, call in cases.items():
        assert call() == api.VALUE_ERR, name


def test_the_pipeline_call_refuses_null_keys(lib):
    gk, _keep = api.make_kdist([0.1, 1.0], lw_edges=[0, 5])
    # (keys are looked at first: no pipeline is needed to be told so)
    assert lib.grt_pipeline_run_kdist_correlated(None, None, C.byref(gk), None) == api.VALUE_ERR
