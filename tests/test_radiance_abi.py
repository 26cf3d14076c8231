"""grt_pipeline_run_sky_radiances' C ABI: exported and declared with its five arguments, GrtRadiances_t field for field the
ctypes structure, at most 16 viewing angles and two rows per angle, its profile tag named once and equal to the Python
module's, and the Python methods (no GPU needed)."""
import ctypes as C
import os
import re

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_run_sky_radiances_is_exported(lib):
    assert "grt_pipeline_run_sky_radiances" in api.EXPORTS
    assert "GrtRadiances" in dir(api)
    assert hasattr(lib, "grt_pipeline_run_sky_radiances")
    types = lib.grt_pipeline_run_sky_radiances.argtypes
    assert list(types) == [C.c_void_p, C.POINTER(api.GrtColumns), C.POINTER(api.GrtSky), C.POINTER(api.GrtRadiances),
                           C.c_void_p]


def test_run_sky_radiances_is_declared_with_five_arguments():
    src = header("include", "grt_ext.h")
    m = re.search(r"EXTERN int grt_pipeline_run_sky_radiances\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_sky_radiances is not declared in grt_ext.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 5
    assert args[0].startswith("GrtPipeline_t *") and args[1].startswith("GrtColumns_t const *")
    assert args[2].startswith("GrtSky_t const *") and args[3].startswith("GrtRadiances_t const *")
    assert args[4] == "fp_t *fluxes_dev"


def test_the_struct_layout_matches_ctypes():
    src = header("include", "grt_ext.h")
    body = re.search(r"typedef struct GrtRadiances\s*\{(.*?)\}\s*GrtRadiances_t;", src, re.S)
    assert body, "GrtRadiances_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if d.strip()]
    assert decls == ["int num_angles", "fp_t const *view_secant", "fp_t *radiances_dev", "fp_t *spectral_radiances_dev",
                     "fp_t *brightness_dev"]
    names = ["num_angles", "view_secant", "radiances_dev", "spectral_radiances_dev", "brightness_dev"]
    assert [f[0] for f in api.GrtRadiances._fields_] == names
    assert [f[1] for f in api.GrtRadiances._fields_] == [C.c_int, C.POINTER(C.c_double), C.c_void_p, C.c_void_p, C.c_void_p]
    assert C.sizeof(api.GrtRadiances) == 40
    assert [getattr(api.GrtRadiances, n).offset for n in names] == [0, 8, 16, 24, 32]


def test_the_constants():
    src = header("include", "grt_ext.h")
    assert re.findall(r"#define GRT_MAX_VIEW_ANGLES (\d+)", src) == ["16"]
    assert re.findall(r"#define GRT_RADIANCE_ROWS_PER_ANGLE (\d+)", src) == ["2"]
    assert api.GRT_MAX_VIEW_ANGLES == 16 and api.GRT_RADIANCE_ROWS_PER_ANGLE == 2


def test_the_tag_is_named_once_and_equals_the_modules():
    src = header("include", "grt_ext.h")
    assert re.findall(r"GRT_TAG_RADIANCE = (\d+)", src) == ["25"]
    assert api.TAG_RADIANCE == 25
    assert api.TAG_SURFACE_JACOBIAN == 24 and api.TAG_SKY_ZENITH_MEAN == 23


def test_python_pipeline_has_the_radiance_calls():
    for name in ("run_sky_radiances", "sky_radiances", "sky_spectral_radiances", "sky_brightness"):
        assert callable(getattr(api.Pipeline, name))
