"""grt_pipeline_run_zeniths' C ABI: exported and declared with its six arguments, its two profile tags, its limits and
a ctypes struct in the header's field order (no GPU needed)."""
import ctypes as C
import os
import re

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_run_zeniths_is_exported(lib):
    assert "grt_pipeline_run_zeniths" in api.EXPORTS
    assert hasattr(lib, "grt_pipeline_run_zeniths")
    assert len(lib.grt_pipeline_run_zeniths.argtypes) == 6


def test_tags_and_limits_equal_the_headers():
    src = header("include", "grt_ext.h")
    for name, value in (("ZENITH_SW", api.TAG_ZENITH_SW), ("ZENITH_MEAN", api.TAG_ZENITH_MEAN)):
        m = re.search(rf"GRT_TAG_{name} = (\d+)", src)
        assert m and int(m.group(1)) == value, name
        assert len(re.findall(rf"GRT_TAG_{name} = ", src)) == 1, name
    assert api.TAG_ZENITH_SW != api.TAG_ZENITH_MEAN and min(api.TAG_ZENITH_SW, api.TAG_ZENITH_MEAN) > api.TAG_SKY_SW
    m = re.search(r"#define GRT_MAX_ZENITHS\s+(\d+)\b", src)
    assert m and int(m.group(1)) == api.GRT_MAX_ZENITHS
    m = re.search(r"#define GRT_ZENITH_CHUNK\s+(\d+)\b", header("grtcode_amd", "csrc", "grt_kernels.h"))
    assert m and int(m.group(1)) == api.GRT_ZENITH_CHUNK and api.GRT_ZENITH_CHUNK in (2, 4, 8)


def test_run_zeniths_is_declared_and_the_struct_matches():
    src = header("include", "grt_ext.h")
    m = re.search(r"EXTERN int grt_pipeline_run_zeniths\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_zeniths is not declared in grt_ext.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 6
    assert args[1].startswith("GrtColumns_t const *") and args[2].startswith("GrtZeniths_t const *")
    assert all(a.startswith("fp_t *") for a in args[3:])
    body = re.search(r"typedef struct GrtZeniths\s*\{(.*?)\}\s*GrtZeniths_t;", src, re.S)
    assert body, "GrtZeniths_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";")]
    names = [re.search(r"(\w+)$", d).group(1) for d in decls if d]
    assert names == [f[0] for f in api.GrtZeniths._fields_]
    kinds = {"num_zeniths": C.c_int, "cos_zenith": api.c_double_p, "weight": api.c_double_p,
             "zenith_fluxes_dev": C.c_void_p, "zenith_level_fluxes_dev": C.c_void_p}
    assert all(kinds[n] is t for n, t in api.GrtZeniths._fields_)


def test_python_pipeline_has_the_zenith_calls():
    for name in ("run_zeniths", "zenith_fluxes", "zenith_profiles"):
        assert callable(getattr(api.Pipeline, name))
    gz, keep = api.make_zeniths([[1.0, 0.5, -0.2], [0.3, 0.0, 1.0]], weight=[[0.2, 0.3, 0.5]] * 2)
    assert gz.num_zeniths == 3 and keep["shape"] == (2, 3)
