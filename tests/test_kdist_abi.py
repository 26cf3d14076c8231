"""The k-distribution entry points' C ABI: grt_kdist_rows, grt_pipeline_run_kdist and grt_kdist_chunk_points exported and
declared with their argument lists, GrtKdistBand_t and GrtKdist_t field for field the ctypes structures, at most 1024
classes, the profile tag named once and equal to the Python module's, the chunk the library reports the kernel's own
constant, the kernel in the build, and the Python calls (no GPU needed)."""
import ctypes as C
import os
import re

from grtcode_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("grt_kdist_rows", "grt_pipeline_run_kdist", "grt_kdist_chunk_points")


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def declared(name, returns="int"):
    m = re.search(r"EXTERN %s %s\(([^;]*)\);" % (returns, name), header("include", "grt_ext.h"))
    assert m, f"{name} is not declared in grt_ext.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_three_functions_are_exported(lib):
    for name in NEW:
        assert name in api.EXPORTS and hasattr(lib, name), name
    assert "GrtKdist" in dir(api) and "GrtKdistBand" in dir(api)
    assert list(lib.grt_kdist_rows.argtypes) == [C.c_int, C.c_void_p, C.c_longlong, C.c_longlong, C.c_double, C.c_int,
                                                 C.POINTER(C.c_double), C.POINTER(api.GrtKdistBand)]
    assert list(lib.grt_pipeline_run_kdist.argtypes) == [C.c_void_p, C.POINTER(api.GrtColumns), C.POINTER(api.GrtKdist)]
    assert list(lib.grt_kdist_chunk_points.argtypes) == []


def test_the_three_functions_are_declared_with_these_arguments():
    assert declared("grt_kdist_rows") == ["Device_t device", "fp_t const *tau_dev", "long long rows", "long long n",
                                          "fp_t dw", "int num_classes", "fp_t const *class_edges",
                                          "GrtKdistBand_t const *band"]
    assert declared("grt_pipeline_run_kdist") == ["GrtPipeline_t *pipeline", "GrtColumns_t const *columns",
                                                  "GrtKdist_t const *kdist"]
    assert declared("grt_kdist_chunk_points") == ["void"]


def struct_decls(name):
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s_t;" % (name, name), header("include", "grt_ext.h"), re.S)
    assert body, f"{name}_t is not declared in grt_ext.h"
    return [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if d.strip()]


def test_the_struct_layouts_match_ctypes():
    assert struct_decls("GrtKdistBand") == ["int const *edges", "int num_bins", "fp_t const *weight", "int *points_dev",
                                            "fp_t *weight_dev", "fp_t *tau_dev"]
    names = ["edges", "num_bins", "weight", "points_dev", "weight_dev", "tau_dev"]
    assert [f[0] for f in api.GrtKdistBand._fields_] == names
    assert [f[1] for f in api.GrtKdistBand._fields_] == [C.POINTER(C.c_int), C.c_int, C.POINTER(C.c_double), C.c_void_p,
                                                         C.c_void_p, C.c_void_p]
    assert C.sizeof(api.GrtKdistBand) == 48
    assert [getattr(api.GrtKdistBand, n).offset for n in names] == [0, 8, 16, 24, 32, 40]

    assert struct_decls("GrtKdist") == ["int num_classes", "fp_t const *class_edges", "GrtKdistBand_t lw, sw"]
    names = ["num_classes", "class_edges", "lw", "sw"]
    assert [f[0] for f in api.GrtKdist._fields_] == names
    assert [f[1] for f in api.GrtKdist._fields_] == [C.c_int, C.POINTER(C.c_double), api.GrtKdistBand, api.GrtKdistBand]
    assert C.sizeof(api.GrtKdist) == 112
    assert [getattr(api.GrtKdist, n).offset for n in names] == [0, 8, 16, 64]


def test_the_constants():
    assert re.findall(r"#define GRT_KDIST_MAX_CLASSES (\d+)", header("include", "grt_ext.h")) == ["1024"]
    assert api.KDIST_MAX_CLASSES == 1024
    # the kernel's own limit (a thread owns at most four classes, a class is parked in 16 bits)
    assert re.findall(r"#define GRT_KDIST_CLASS_LIMIT (\d+)", header("grtcode_amd", "csrc", "grt_kernels.h")) == ["1024"]


def test_the_tag_is_named_once_and_equals_the_modules():
    assert re.findall(r"GRT_TAG_KDIST = (\d+)", header("include", "grt_ext.h")) == ["29"]
    assert api.TAG_KDIST == 29
    assert api.TAG_WEIGHTING_FINISH == 28 and api.TAG_GAS_LW == 1


def test_the_chunk_is_the_kernels_constant(lib):
    src = header("grtcode_amd", "csrc", "hip", "k_kdist.hip")
    chunk = re.findall(r"constexpr int kChunkPoints = (\d+);", src)
    assert len(chunk) == 1
    assert lib.grt_kdist_chunk_points() == int(chunk[0]) == api.kdist_chunk_points()
    assert int(chunk[0]) % 256 == 0


def test_the_kernel_and_its_host_file_are_built():
    assert "k_kdist.hip" in build.HIP_SRC and "grt_kdist.c" in build.HOST_SRC
    # the static archives a C driver links hold both: grt_pipeline.o calls into them
    assert {"grt_kdist", "k_kdist"} <= set(build.ARCHIVES["libgrtcode_hip_ext.a"])


def test_python_has_the_kdist_calls():
    for name in ("run_kdist", "kdist"):
        assert callable(getattr(api.Pipeline, name))
    assert callable(api.make_kdist) and callable(api.kdist_rows)
    gk, keep = api.make_kdist([0.1, 1.0, 10.0], lw_edges=[0, 5, 9], sw_weight=[1.0, 2.0])
    assert gk.num_classes == 4 and gk.lw.num_bins == 2 and gk.sw.num_bins == 0
    assert not gk.lw.weight and not gk.sw.edges and gk.sw.weight[1] == 2.0 and gk.lw.edges[2] == 9
    assert gk.class_edges[2] == 10.0 and keep["class_edges"].size == 3
    from grtcode_amd import kdist
    assert callable(kdist.cumulative) and callable(kdist.k_of_g)
