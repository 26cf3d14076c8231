"""Cost of grt_pipeline_run_allsky_profiles against grt_pipeline_run_allsky on the G1 workload (grtcode_amd.workload: 64
columns, 61 levels, the bench's grids and line lists, fast = 3), with the synthetic cloud fields of
scripts/pipeline_timing.py.

Five alternating repetitions of three steps on one pipeline:
  allsky            grt_pipeline_run_allsky, default (the shortwave's one sweep where the user level allows it)
  allsky_two        grt_pipeline_run_allsky with GRT_SW_TWO_SWEEPS=1 (the reference's two sweeps)
  allsky_profiles   grt_pipeline_run_allsky_profiles (level fluxes and heating rates of both passes)
Per step: the solver times by HIP-event profile tag (grt_ext.h: 3 / 4 longwave / shortwave clear-sky solver, 8 / 9 the
all-sky pass's) and the wall time of the whole step, synchronised.  Result: profiles/pipeline_allsky_profiles_timing.json
(or the path given).

    python scripts/time_pipeline_allsky_profiles.py [--reps 5] [--out profiles/pipeline_allsky_profiles_timing.json]
"""
import os

import numpy as np

from pipeline_timing import Session, synthetic_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

TAGS = {"lw_solver_ms": api.TAG_SOLVER_LW, "sw_solver_ms": api.TAG_SOLVER_SW,
        "lw_allsky_solver_ms": api.TAG_ALLSKY_LW, "sw_allsky_solver_ms": api.TAG_ALLSKY_SW}


def main():
    s = Session("pipeline_allsky_profiles_timing.json")
    pipe, gcols, ncol, V = s.pipe, s.gcols, s.ncol, s.V
    gclouds, keep_clouds = synthetic_clouds(s.keep["p"], s.keep["tl"])
    out = s.buffer(api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    levels, heating, prof_out = s.profile_outputs(2)

    def step(mode):
        if mode == "allsky_profiles":
            api.check(s.lib.grt_pipeline_run_allsky_profiles(pipe.p, api.C.byref(gcols), api.C.byref(gclouds),
                                                             levels.ptr, heating.ptr, prof_out.ptr))
            return
        if mode == "allsky_two":
            os.environ["GRT_SW_TWO_SWEEPS"] = "1"
        try:
            api.check(s.lib.grt_pipeline_run_allsky(pipe.p, api.C.byref(gcols), api.C.byref(gclouds), out.ptr))
        finally:
            os.environ.pop("GRT_SW_TWO_SWEEPS", None)

    samples, median, _ = s.measure(("allsky", "allsky_two", "allsky_profiles"), step, TAGS)
    f = prof_out.to_host((ncol, api.GRT_ALLSKY_FLUXES_PER_COLUMN))
    hr = heating.to_host((ncol, api.GRT_ALLSKY_HEATING_ROWS_PER_COLUMN, V - 1))
    prof, two, one = median["allsky_profiles"], median["allsky_two"], median["allsky"]
    result = {"workload": s.workload + "; synthetic clouds in about a third of the layers",
              "reps": s.args.reps, "order": "allsky, allsky_two, allsky_profiles alternating; medians over the repetitions",
              "median": median, "samples": samples,
              "allsky_profile_solver_over_two_sweep_allsky_solver": {
                  b: prof[f"{b}_allsky_solver_ms"] / two[f"{b}_allsky_solver_ms"] for b in ("lw", "sw")},
              "allsky_profile_solver_over_one_sweep_allsky_solver": {
                  b: prof[f"{b}_allsky_solver_ms"] / one[f"{b}_allsky_solver_ms"] for b in ("lw", "sw")},
              "allsky_profiles_step_over_allsky_step": prof["wall_ms"] / one["wall_ms"],
              "targets": {"solver_over_two_sweep": 1.5, "step_over_allsky_step": 1.10},
              "mean_abs_cloud_effect_on_heating_k_day": {
                  "lw": float(np.mean(np.abs(hr[:, 2] - hr[:, 0]))), "sw": float(np.mean(np.abs(hr[:, 3] - hr[:, 1])))},
              # (largest difference of the 24 values from the last two-sweep run_allsky, relative to the largest value:
              # the gas optics of the default mode add with atomics, so two calls agree to rounding, not to the bit)
              "fluxes_equal_run_allsky_to": float(np.max(np.abs(f - out.to_host(f.shape))) / np.abs(f).max())}
    s.finish(result, ("median", "allsky_profile_solver_over_two_sweep_allsky_solver", "allsky_profiles_step_over_allsky_step",
                      "mean_abs_cloud_effect_on_heating_k_day", "fluxes_equal_run_allsky_to"))


if __name__ == "__main__":
    main()
