"""The spectral entry point's C ABI: exported, declared with its ten arguments, and known to Python (no GPU needed)."""
import os
import re

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_spectral_is_exported(lib):
    assert "grt_pipeline_run_spectral" in api.EXPORTS
    assert hasattr(lib, "grt_pipeline_run_spectral")
    assert len(lib.grt_pipeline_run_spectral.argtypes) == 10


def test_run_spectral_is_declared():
    src = open(os.path.join(ROOT, "include", "grt_ext.h")).read()
    m = re.search(r"EXTERN int grt_pipeline_run_spectral\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_spectral is not declared in grt_ext.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10
    assert args[3].startswith("int const *") and args[5].startswith("int const *")
    assert all(a.startswith("fp_t *") for a in args[7:])
    assert re.search(r"10 = the\s+\*?\s*wavenumber-bin kernel", src)
