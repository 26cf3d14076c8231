"""grt_pipeline_run_sky's C ABI: exported, declared with its six arguments, the set count of every mask, and a ctypes
struct in the header's field order (no GPU needed)."""
import ctypes as C
import os
import re

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sky_symbols_are_exported(lib):
    for name, nargs in (("grt_pipeline_run_sky", 6), ("grt_pipeline_sky_set_count", 1)):
        assert name in api.EXPORTS
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs


def test_set_count_of_every_mask(lib):
    for mask in range(16):
        assert lib.grt_pipeline_sky_set_count(mask) == bin(mask | api.GRT_SKY_CLEAN).count("1"), mask
        assert api.sky_set_count(mask) == lib.grt_pipeline_sky_set_count(mask)
    assert lib.grt_pipeline_sky_set_count(api.GRT_SKY_ALL) == api.GRT_SKY_MAX_SETS
    for stray in (16, 16 | api.GRT_SKY_ALL, 1 << 31, 32 | api.GRT_SKY_CLOUD):
        assert lib.grt_pipeline_sky_set_count(stray) == 0, stray


def test_sky_is_declared_and_the_struct_matches():
    src = open(os.path.join(ROOT, "include", "grt_ext.h")).read()
    m = re.search(r"EXTERN int grt_pipeline_run_sky\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_sky is not declared in grt_ext.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 6
    assert args[1].startswith("GrtColumns_t const *") and args[2].startswith("GrtSky_t const *")
    assert all(a.startswith("fp_t *") for a in args[3:])
    assert re.search(r"EXTERN int grt_pipeline_sky_set_count\(unsigned \w+\);", src)
    for name, value in (("CLEAN", 1), ("AEROSOL", 2), ("CLOUD", 4), ("CLOUD_AEROSOL", 8)):
        assert re.search(rf"#define GRT_SKY_{name}\s+{value}u\b", src), name
        assert getattr(api, "GRT_SKY_" + name) == value
    assert re.search(r"#define GRT_SKY_MAX_SETS\s+4\b", src)
    body = re.search(r"typedef struct GrtSky\s*\{(.*?)\}\s*GrtSky_t;", src, re.S)
    assert body, "GrtSky_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";")]
    names = [re.search(r"(\w+)$", d).group(1) for d in decls if d]
    assert names == [f[0] for f in api.GrtSky._fields_]
    kinds = {"clouds": C.POINTER(api.GrtClouds), "aerosols": C.POINTER(api.GrtAerosols), "num_subcolumns": C.c_int,
             "sets": C.c_uint}
    assert all(kinds[n] is t for n, t in api.GrtSky._fields_)
    assert re.search(r"GRT_TAG_SKY_LW = 17", src) and re.search(r"GRT_TAG_SKY_SW = 18", src)
    assert (api.TAG_SKY_LW, api.TAG_SKY_SW) == (17, 18)


def test_python_pipeline_has_the_sky_calls():
    for name in ("run_sky", "sky_fluxes", "sky_profiles"):
        assert callable(getattr(api.Pipeline, name))
    assert callable(api.make_sky)
