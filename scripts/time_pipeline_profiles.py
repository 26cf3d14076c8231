"""Cost of grt_pipeline_run_profiles against the six-row forms on the G1 workload (grtcode_amd.workload: 64 columns,
61 levels, the bench's grids and line lists, fast = 3).

Five alternating repetitions of three steps on one pipeline:
  run        grt_pipeline_run (the shortwave's default one-sweep form)
  run_two    grt_pipeline_run with GRT_SW_TWO_SWEEPS=1 (the two-sweep form: the park block)
  profiles   grt_pipeline_run_profiles (every level's flux and the heating rates)
Per step: the longwave and shortwave solver times (HIP-event profile tags 3 and 4, grt_ext.h) and the wall time of the
whole step, synchronised.  Result: profiles/pipeline_profiles_timing.json (or the path given).

    python scripts/time_pipeline_profiles.py [--reps 5] [--out profiles/pipeline_profiles_timing.json]
"""
import os

from pipeline_timing import Session  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

TAGS = {"lw_solver_ms": api.TAG_SOLVER_LW, "sw_solver_ms": api.TAG_SOLVER_SW}


def main():
    s = Session("pipeline_profiles_timing.json")
    pipe, gcols = s.pipe, s.gcols
    levels, heating, fluxes = s.profile_outputs(1)

    def step(mode):
        if mode == "profiles":
            api.check(s.lib.grt_pipeline_run_profiles(pipe.p, api.C.byref(gcols), levels.ptr, heating.ptr, fluxes.ptr))
            return
        if mode == "run_two":
            os.environ["GRT_SW_TWO_SWEEPS"] = "1"
        try:
            pipe.run(gcols)
        finally:
            os.environ.pop("GRT_SW_TWO_SWEEPS", None)

    samples, median, _ = s.measure(("run", "run_two", "profiles"), step, TAGS)
    ratio = {band: median["profiles"][f"{band}_solver_ms"] / median["run_two"][f"{band}_solver_ms"] for band in ("lw", "sw")}
    result = {"workload": s.workload,
              "reps": s.args.reps, "order": "run, run_two, profiles alternating; medians over the repetitions",
              "median": median, "samples": samples,
              "profile_over_two_sweep_solver": ratio,
              "profile_over_one_sweep_solver": {band: median["profiles"][f"{band}_solver_ms"] / median["run"][f"{band}_solver_ms"]
                                                for band in ("lw", "sw")}}
    s.finish(result, ("median", "profile_over_two_sweep_solver"))


if __name__ == "__main__":
    main()
