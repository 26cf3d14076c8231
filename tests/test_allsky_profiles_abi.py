"""The all-sky profile entry point's C ABI: exported, declared, and its row counts alike in C and Python (no GPU needed)."""
import os
import re

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_run_allsky_profiles_is_exported(lib):
    assert "grt_pipeline_run_allsky_profiles" in api.EXPORTS
    assert hasattr(lib, "grt_pipeline_run_allsky_profiles")


def test_row_counts_are_two_sets_of_the_profile_rows():
    assert api.GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN == 8
    assert api.GRT_ALLSKY_HEATING_ROWS_PER_COLUMN == 4
    src = open(os.path.join(ROOT, "include", "grt_ext.h")).read()
    for name, base in (("GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN", "GRT_PROFILE_ROWS_PER_COLUMN"),
                       ("GRT_ALLSKY_HEATING_ROWS_PER_COLUMN", "GRT_HEATING_ROWS_PER_COLUMN")):
        assert re.search(r"#define\s+%s\s+\(2\*%s\)" % (name, base), src), name
