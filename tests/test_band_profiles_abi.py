"""The band-profile entry points' C ABI: exported, declared with their nine arguments and one argument, and known to
Python (no GPU needed)."""
import os
import re

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_profile_symbols_are_exported(lib):
    for name, nargs in (("grt_pipeline_run_band_profiles", 9), ("grt_pipeline_band_profile_bin_limit", 1)):
        assert name in api.EXPORTS
        assert hasattr(lib, name)
        assert len(getattr(lib, name).argtypes) == nargs


def test_band_profile_symbols_are_declared():
    src = open(os.path.join(ROOT, "include", "grt_ext.h")).read()
    m = re.search(r"EXTERN int grt_pipeline_run_band_profiles\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_band_profiles is not declared in grt_ext.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 9
    assert args[2].startswith("GrtClouds_t const *")
    assert args[3].startswith("int const *") and args[5].startswith("int const *")
    assert args[4].startswith("int ") and args[6].startswith("int ")
    assert all(a.startswith("fp_t *") for a in args[7:])
    m = re.search(r"EXTERN int grt_pipeline_band_profile_bin_limit\(([^;]*)\);", src)
    assert m, "grt_pipeline_band_profile_bin_limit is not declared in grt_ext.h"
    assert len(m.group(1).split(",")) == 1 and m.group(1).strip().startswith("GrtPipeline_t const *")
    assert re.search(r"14 = the per-bin reduction", src)
    assert re.search(r"10 = the\s+\*?\s*wavenumber-bin kernel", src)          # (tag 10's text stays)


def test_python_pipeline_has_the_band_profile_calls():
    for name in ("run_band_profiles", "band_profiles", "band_profile_bin_limit"):
        assert callable(getattr(api.Pipeline, name))
