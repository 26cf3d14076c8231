"""The all-sky entry point's C ABI: exported, and the cloud-input struct laid out alike in C and ctypes (no GPU needed)."""
import ctypes as C

from grtcode_amd import api


def test_run_allsky_is_exported(lib):
    assert "grt_pipeline_run_allsky" in api.EXPORTS
    assert hasattr(lib, "grt_pipeline_run_allsky")


def test_clouds_struct_layout_matches_between_c_and_ctypes(lib):
    assert lib.grt_sizeof(api.GRT_CLOUDS) == C.sizeof(api.GrtClouds) > 0
