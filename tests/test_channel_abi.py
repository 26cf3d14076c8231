"""grt_pipeline_run_sky_channels' C ABI: exported and declared with its six arguments, GrtChannels_t field for field the
ctypes structure, at most 16384 channels, its profile tag named once and equal to the Python module's, and the Python
methods (no GPU needed)."""
import ctypes as C
import os
import re

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_run_sky_channels_is_exported(lib):
    assert "grt_pipeline_run_sky_channels" in api.EXPORTS and "grt_channel_pair_count" in api.EXPORTS
    assert "GrtChannels" in dir(api)
    assert hasattr(lib, "grt_pipeline_run_sky_channels") and hasattr(lib, "grt_channel_pair_count")
    types = lib.grt_pipeline_run_sky_channels.argtypes
    assert list(types) == [C.c_void_p, C.POINTER(api.GrtColumns), C.POINTER(api.GrtSky), C.POINTER(api.GrtRadiances),
                           C.POINTER(api.GrtChannels), C.c_void_p]
    assert list(lib.grt_channel_pair_count.argtypes) == [C.POINTER(api.GrtChannels), C.c_longlong]
    assert lib.grt_channel_pair_count.restype == C.c_longlong


def test_run_sky_channels_is_declared_with_six_arguments():
    src = header("include", "grt_ext.h")
    m = re.search(r"EXTERN int grt_pipeline_run_sky_channels\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_sky_channels is not declared in grt_ext.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 6
    assert args[0].startswith("GrtPipeline_t *") and args[1].startswith("GrtColumns_t const *")
    assert args[2].startswith("GrtSky_t const *") and args[3].startswith("GrtRadiances_t const *")
    assert args[4].startswith("GrtChannels_t const *") and args[5] == "fp_t *fluxes_dev"
    m = re.search(r"EXTERN long long grt_channel_pair_count\(([^;]*)\);", src)
    assert m, "grt_channel_pair_count is not declared in grt_ext.h"
    assert [" ".join(a.split()) for a in m.group(1).split(",")] == ["GrtChannels_t const *channels", "long long num_points"]


def test_the_struct_layout_matches_ctypes():
    src = header("include", "grt_ext.h")
    body = re.search(r"typedef struct GrtChannels\s*\{(.*?)\}\s*GrtChannels_t;", src, re.S)
    assert body, "GrtChannels_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if d.strip()]
    assert decls == ["int num_channels", "int const *first", "int const *offset", "fp_t const *weights",
                     "fp_t const *center", "fp_t *channel_radiances_dev", "fp_t *channel_brightness_dev"]
    names = ["num_channels", "first", "offset", "weights", "center", "channel_radiances_dev", "channel_brightness_dev"]
    assert [f[0] for f in api.GrtChannels._fields_] == names
    assert [f[1] for f in api.GrtChannels._fields_] == [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                                        C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p, C.c_void_p]
    assert C.sizeof(api.GrtChannels) == 56
    assert [getattr(api.GrtChannels, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48]


def test_the_constants():
    src = header("include", "grt_ext.h")
    assert re.findall(r"#define GRT_MAX_CHANNELS (\d+)", src) == ["16384"]
    assert api.GRT_MAX_CHANNELS == 16384


def test_the_tag_is_named_once_and_equals_the_modules():
    src = header("include", "grt_ext.h")
    assert re.findall(r"GRT_TAG_CHANNELS = (\d+)", src) == ["26"]
    assert api.TAG_CHANNELS == 26
    assert api.TAG_RADIANCE == 25 and api.TAG_SURFACE_JACOBIAN == 24


def test_python_has_the_channel_calls():
    for name in ("run_sky_channels", "sky_channel_radiances", "sky_channel_brightness"):
        assert callable(getattr(api.Pipeline, name))
    assert callable(api.make_channels) and callable(api.channel_pair_count)
    from grtcode_amd import channels
    assert callable(channels.gaussian) and callable(channels.boxcar)
