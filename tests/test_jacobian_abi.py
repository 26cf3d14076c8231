"""grt_pipeline_run_sky_jacobian's C ABI: exported and declared with its seven arguments, GrtSurfaceJacobian_t field for
field the ctypes structure, three rows per set, its profile tag named once and equal to the Python module's, and the
Python methods (no GPU needed)."""
import ctypes as C
import os
import re

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_run_sky_jacobian_is_exported(lib):
    assert "grt_pipeline_run_sky_jacobian" in api.EXPORTS
    assert hasattr(lib, "grt_pipeline_run_sky_jacobian")
    types = lib.grt_pipeline_run_sky_jacobian.argtypes
    assert list(types) == [C.c_void_p, C.POINTER(api.GrtColumns), C.POINTER(api.GrtSky), C.POINTER(api.GrtSurfaceJacobian),
                           C.c_void_p, C.c_void_p, C.c_void_p]


def test_run_sky_jacobian_is_declared_with_seven_arguments():
    src = header("include", "grt_ext.h")
    m = re.search(r"EXTERN int grt_pipeline_run_sky_jacobian\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_sky_jacobian is not declared in grt_ext.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 7
    assert args[0].startswith("GrtPipeline_t *") and args[1].startswith("GrtColumns_t const *")
    assert args[2].startswith("GrtSky_t const *") and args[3].startswith("GrtSurfaceJacobian_t const *")
    assert [a.split("*")[1] for a in args[4:]] == ["level_fluxes_dev", "heating_dev", "fluxes_dev"]
    assert all(a.startswith("fp_t *") for a in args[4:])


def test_the_struct_layout_matches_ctypes():
    src = header("include", "grt_ext.h")
    body = re.search(r"typedef struct GrtSurfaceJacobian\s*\{(.*?)\}\s*GrtSurfaceJacobian_t;", src, re.S)
    assert body, "GrtSurfaceJacobian_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if d.strip()]
    assert decls == ["fp_t *jacobian_fluxes_dev", "fp_t *jacobian_level_fluxes_dev"]
    assert [f[0] for f in api.GrtSurfaceJacobian._fields_] == ["jacobian_fluxes_dev", "jacobian_level_fluxes_dev"]
    assert all(t is C.c_void_p for _, t in api.GrtSurfaceJacobian._fields_)
    assert C.sizeof(api.GrtSurfaceJacobian) == 16
    assert api.GrtSurfaceJacobian.jacobian_fluxes_dev.offset == 0
    assert api.GrtSurfaceJacobian.jacobian_level_fluxes_dev.offset == 8
    # the direct beam's struct, which the call's route through the code is shared with, is what it was
    assert [f[0] for f in api.GrtDirectBeam._fields_] == ["direct_fluxes_dev", "direct_level_fluxes_dev"]


def test_three_rows_per_set():
    src = header("include", "grt_ext.h")
    assert re.findall(r"#define GRT_JACOBIAN_ROWS_PER_SET (\d+)", src) == ["3"]
    assert api.GRT_JACOBIAN_ROWS_PER_SET == 3


def test_the_tag_is_named_once_and_equals_the_modules():
    src = header("include", "grt_ext.h")
    assert re.findall(r"GRT_TAG_SURFACE_JACOBIAN = (\d+)", src) == ["24"]
    assert api.TAG_SURFACE_JACOBIAN == 24
    assert api.TAG_DIRECT_BEAM == 21 and api.TAG_SKY_ZENITH_SW == 22 and api.TAG_SKY_ZENITH_MEAN == 23


def test_python_pipeline_has_the_jacobian_calls():
    for name in ("run_sky_jacobian", "sky_jacobian_fluxes", "sky_jacobian_profiles"):
        assert callable(getattr(api.Pipeline, name))
