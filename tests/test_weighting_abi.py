"""grt_pipeline_run_sky_weighting's C ABI: exported and declared with its seven arguments, GrtWeighting_t field for field
the ctypes structure, its two profile tags named once and equal to the Python module's, and the Python methods (no GPU
needed)."""
import ctypes as C
import os
import re

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_run_sky_weighting_is_exported(lib):
    assert "grt_pipeline_run_sky_weighting" in api.EXPORTS
    assert "GrtWeighting" in dir(api)
    assert hasattr(lib, "grt_pipeline_run_sky_weighting")
    assert list(lib.grt_pipeline_run_sky_weighting.argtypes) == [
        C.c_void_p, C.POINTER(api.GrtColumns), C.POINTER(api.GrtSky), C.POINTER(api.GrtRadiances),
        C.POINTER(api.GrtChannels), C.POINTER(api.GrtWeighting), C.c_void_p]


def test_run_sky_weighting_is_declared_with_seven_arguments():
    src = header("include", "grt_ext.h")
    m = re.search(r"EXTERN int grt_pipeline_run_sky_weighting\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_sky_weighting is not declared in grt_ext.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 7
    assert args[0].startswith("GrtPipeline_t *") and args[1].startswith("GrtColumns_t const *")
    assert args[2].startswith("GrtSky_t const *") and args[3].startswith("GrtRadiances_t const *")
    assert args[4].startswith("GrtChannels_t const *") and args[5].startswith("GrtWeighting_t const *")
    assert args[6] == "fp_t *fluxes_dev"


def test_the_struct_layout_matches_ctypes():
    src = header("include", "grt_ext.h")
    body = re.search(r"typedef struct GrtWeighting\s*\{(.*?)\}\s*GrtWeighting_t;", src, re.S)
    assert body, "GrtWeighting_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if d.strip()]
    assert decls == ["fp_t *transmittance_dev", "fp_t *contribution_dev"]
    names = ["transmittance_dev", "contribution_dev"]
    assert [f[0] for f in api.GrtWeighting._fields_] == names
    assert [f[1] for f in api.GrtWeighting._fields_] == [C.c_void_p, C.c_void_p]
    assert C.sizeof(api.GrtWeighting) == 16
    assert [getattr(api.GrtWeighting, n).offset for n in names] == [0, 8]


def test_the_tags_are_named_once_and_equal_the_modules():
    src = header("include", "grt_ext.h")
    assert re.findall(r"GRT_TAG_WEIGHTING = (\d+)", src) == ["27"]
    assert re.findall(r"GRT_TAG_WEIGHTING_FINISH = (\d+)", src) == ["28"]
    assert api.TAG_WEIGHTING == 27 and api.TAG_WEIGHTING_FINISH == 28
    assert api.TAG_CHANNELS == 26 and api.TAG_RADIANCE == 25


def test_python_has_the_weighting_calls():
    for name in ("run_sky_weighting", "sky_channel_transmittances", "sky_channel_contributions"):
        assert callable(getattr(api.Pipeline, name))
