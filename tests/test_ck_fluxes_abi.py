"""grt_pipeline_run_ck_fluxes' C ABI: exported and declared with its argument list, GrtCkBand_t and GrtCkFluxes_t field for
field the ctypes structures, the three profile tags named once and equal to the Python module's, the kernels in the
build and stated where the issue puts them, the Python calls, and the refusals the host decides before it needs a device or
a pipeline (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

from grtcode_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def struct_decls(name):
    body = re.search(r"typedef struct %s\s*\{(.*?)\}\s*%s_t;" % (name, name), text("include", "grt_ext.h"), re.S)
    assert body, f"{name}_t is not declared in grt_ext.h"
    return [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if d.strip()]


def test_the_function_is_exported_and_declared(lib):
    name = "grt_pipeline_run_ck_fluxes"
    assert name in api.EXPORTS and hasattr(lib, name)
    assert list(lib.grt_pipeline_run_ck_fluxes.argtypes) == [C.c_void_p, C.POINTER(api.GrtColumns), C.POINTER(api.GrtCkFluxes)]
    m = re.search(r"EXTERN int %s\(([^;]*)\);" % name, text("include", "grt_ext.h"))
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == [
        "GrtPipeline_t *pipeline", "GrtColumns_t const *columns", "GrtCkFluxes_t const *ck"]


def test_the_struct_layouts_match_ctypes():
    assert struct_decls("GrtCkBand") == [
        "int const *edges", "int num_bins", "GrtKdistKey_t key", "unsigned short const *map_given_dev", "int *points_dev",
        "fp_t *weight_dev", "fp_t *tau_dev", "fp_t *source_dev", "fp_t *flux_up_dev, *flux_down_dev",
        "fp_t *bin_up_dev, *bin_down_dev"]
    names = ["edges", "num_bins", "key", "map_given_dev", "points_dev", "weight_dev", "tau_dev", "source_dev", "flux_up_dev",
             "flux_down_dev", "bin_up_dev", "bin_down_dev"]
    assert [f[0] for f in api.GrtCkBand._fields_] == names
    assert [f[1] for f in api.GrtCkBand._fields_] == [C.POINTER(C.c_int), C.c_int, api.GrtKdistKey] + [C.c_void_p] * 9
    assert [getattr(api.GrtCkBand, n).offset for n in names] == [0, 8, 16, 32, 40, 48, 56, 64, 72, 80, 88, 96]
    assert C.sizeof(api.GrtCkBand) == 104

    assert struct_decls("GrtCkFluxes") == ["int num_classes", "fp_t const *class_edges", "GrtCkBand_t lw, sw"]
    assert [f[0] for f in api.GrtCkFluxes._fields_] == ["num_classes", "class_edges", "lw", "sw"]
    assert [getattr(api.GrtCkFluxes, n).offset for n in ("num_classes", "class_edges", "lw", "sw")] == [0, 8, 16, 120]
    assert C.sizeof(api.GrtCkFluxes) == 224


def test_the_tags_are_named_once_and_equal_the_modules():
    header = text("include", "grt_ext.h")
    for name, value in (("CK_SOURCES", 32), ("CK_LW", 33), ("CK_SW", 34)):
        assert re.findall(r"GRT_TAG_%s = (\d+)" % name, header) == [str(value)], name
        assert getattr(api, "TAG_" + name) == value
    assert api.TAG_KDIST_MAPPED == 31 and api.TAG_GAS_LW == 1


def test_the_kernels_are_where_they_belong():
    kd = text("grtcode_amd", "csrc", "hip", "k_kdist.hip")
    assert len(re.findall(r"__global__[^\n]*void kdist_sources_kernel\(", kd)) == 1
    assert len(re.findall(r"__global__[^\n]*void ck_bin_sum_kernel\(", kd)) == 1
    # phase 2 stays stated once; the source kernel calls it as the other two do
    assert len(re.findall(r"__device__[^\n]*void sum_chunk\(", kd)) == 1 and len(re.findall(r"sum_chunk<\w+>\(", kd)) == 3
    lw, sw = text("grtcode_amd", "csrc", "hip", "k_longwave.hip"), text("grtcode_amd", "csrc", "hip", "k_shortwave.hip")
    assert len(re.findall(r"__global__[^\n]*void ck_lw_kernel\(", lw)) == 1
    assert len(re.findall(r"__global__[^\n]*void ck_sw_kernel\(", sw)) == 1
    # one Planck function for the solver and the source sums
    planck = r"__device__[^\n]*double planck\("
    assert len(re.findall(planck, text("grtcode_amd", "csrc", "hip", "planck_dev.h"))) == 1
    assert not re.findall(planck, lw) and not re.findall(planck, kd)
    for src in (lw, kd):
        assert '#include "planck_dev.h"' in src
    # the solvers' own layer steps
    body = lw[lw.index("void ck_lw_kernel("):]
    body = body[:body.index("\n}\n")]
    for step in ("effective_planck(", "stream_step(", "surface_step(", "extinction("):
        assert step in body, step
    body = sw[sw.index("void ck_sw_kernel("):]
    body = body[:body.index("\n}\n")]
    for step in ("clear_sky_combine(", "layer_props(", "sweep1_step(", "sweep2_step(", "level_flux("):
        assert step in body, step
    kernels = text("grtcode_amd", "csrc", "grt_kernels.h")
    for name in ("GrtCkSourceArgs", "GrtCkSolveArgs", "grt_launch_ck_sources", "grt_launch_ck_lw", "grt_launch_ck_sw",
                 "grt_launch_ck_bin_sum"):
        assert name in kernels, name
    assert "k_kdist.hip" in build.HIP_SRC


def test_python_has_the_calls():
    for name in ("run_ck_fluxes", "ck_fluxes"):
        assert callable(getattr(api.Pipeline, name))
    from grtcode_amd import kdist
    w = np.array([[2.0, 0.0, 0.5]])
    tau = np.array([[[4.0, 0.0, 1.0]], [[1.0, 0.0, 0.25]]])
    src = np.array([[[6.0, 0.0, 2.0]]])
    t, s = kdist.ck_means(w, tau, src)
    assert np.array_equal(t, [[[2.0, 0.0, 2.0]], [[0.5, 0.0, 0.5]]]) and np.array_equal(s, [[[3.0, 0.0, 4.0]]])


def test_refusals_that_need_no_pipeline(lib):
    ck = api.GrtCkFluxes()
    # (the pipeline and the columns are looked at first)
    assert lib.grt_pipeline_run_ck_fluxes(None, None, C.byref(ck)) != 0
    fake = C.c_void_p(0x1000)
    cols = api.GrtColumns()
    assert lib.grt_pipeline_run_ck_fluxes(fake, C.byref(cols), None) == api.VALUE_ERR
    # the classes are decided before the pipeline is looked behind
    bad = np.array([0.1, 0.1, 1.0])
    for K, ce in ((1, None), (1025, None), (4, bad), (1, np.array([])), (3, np.array([0.1, np.nan]))):
        ck = api.GrtCkFluxes()
        ck.num_classes = K
        ck.class_edges = None if ce is None else ce.ctypes.data_as(api.c_double_p)
        assert lib.grt_pipeline_run_ck_fluxes(fake, C.byref(cols), C.byref(ck)) == api.VALUE_ERR, (K, ce)
