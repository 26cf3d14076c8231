"""The longwave kernels (k_longwave.hip) bit for bit: a change that only moves what the kernels say -- the point set-up,
the sweeps, the pair sums -- leaves every operation and every rounding where it was, so in deterministic mode every output
of every pipeline entry point that reaches one of them is the bits recorded from the commit named in
tests/golden/lw_point_bits.npz (tests/golden/make_lw_point_bits.py wrote it).  The shapes and the runs are said in
tests/lw_point_cases.py: a longwave-only pipeline, fused and keep_spectra = 1, 129 points, 2 columns, 4 levels, 3 cloud
draws, an aerosol object, 5 viewing angles, 3 channels."""
import os

import numpy as np
import pytest

import lw_point_cases as cases
from grtcode_amd import api

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lw_point_bits.npz")


def golden_arrays():
    with np.load(GOLDEN) as z:
        assert int(z["seed"]) == cases.SEED
        return str(z["commit"]), {k: z[k] for k in z.files if k not in ("commit", "seed")}


COMMIT, WANT = golden_arrays()


@pytest.fixture(scope="module")
def outputs(lib, device, tmp_path_factory):
    """Every output of every run, computed once in deterministic mode."""
    api.check(lib.grt_set_deterministic(1))
    try:
        return cases.run_all(cases.Inputs(str(tmp_path_factory.mktemp("lw_point"))), device)
    finally:
        api.check(lib.grt_set_deterministic(-1))


def test_the_recorded_runs_are_the_cases_runs(outputs):
    assert sorted(outputs) == sorted(WANT)
    # both forms of every entry point that takes both, and run() on the keep_spectra pipeline
    for form in ("fused", "spectra"):
        for run in ("S1.sky", "S3.sky", "S1.sky_profiles", "S3.sky_profiles", "jacobian", "jacobian_profiles", "S3.weighting",
                    "S1.weighting", "S1.radiances", "band_profiles", "spectral"):
            assert any(k.startswith(f"{form}.{run}.") for k in WANT), (form, run)
    assert "spectra.run.fluxes" in WANT


@pytest.mark.parametrize("name", sorted(WANT))
def test_bits_are_the_recorded_ones(name, outputs):
    got, want = outputs[name], WANT[name]
    # (a band that is missing gives zeros on both sides: the recorded array itself has to hold something)
    assert np.all(np.isfinite(want)) and np.any(want != 0.0)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64
    differ = np.argwhere(got != want)
    print(f"{name}: {len(differ)} of {got.size} values differ from commit {COMMIT}"
          + (f"; first at {differ[0].tolist()}: {got[tuple(differ[0])]!r} != {want[tuple(differ[0])]!r}" if len(differ) else ""))
    assert np.array_equal(got, want)
