"""Cost of grt_pipeline_run_allsky against grt_pipeline_run on the G1 workload (grtcode_amd.workload: 64 columns,
61 levels, the bench's grids and line lists, fast = 3), with synthetic cloud fields: cloud in about a third of the
layers, liquid in the lower ones, ice in the upper ones, band optics on 8 liquid and 10 ice bands across both grids.

Five alternating repetitions of two steps on one pipeline:
  run      grt_pipeline_run (clear sky)
  allsky   grt_pipeline_run_allsky (the clear-sky pass and the all-sky pass)
Per step: the solver times by HIP-event profile tag (grt_ext.h: 3 / 4 longwave / shortwave clear-sky solver, 8 / 9 the
all-sky pass's) and the wall time of the whole step, synchronised.  Result: profiles/pipeline_allsky_timing.json (or the
path given).

    python scripts/time_pipeline_allsky.py [--reps 5] [--out profiles/pipeline_allsky_timing.json]
"""
import numpy as np

from pipeline_timing import Session, synthetic_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

TAGS = {"lw_solver_ms": api.TAG_SOLVER_LW, "sw_solver_ms": api.TAG_SOLVER_SW,
        "lw_allsky_solver_ms": api.TAG_ALLSKY_LW, "sw_allsky_solver_ms": api.TAG_ALLSKY_SW}


def main():
    s = Session("pipeline_allsky_timing.json")
    pipe, gcols = s.pipe, s.gcols
    gclouds, keep_clouds = synthetic_clouds(s.keep["p"], s.keep["tl"])
    out = s.buffer(api.GRT_ALLSKY_FLUXES_PER_COLUMN)

    def step(mode):
        if mode == "allsky":
            api.check(s.lib.grt_pipeline_run_allsky(pipe.p, api.C.byref(gcols), api.C.byref(gclouds), out.ptr))
        else:
            pipe.run(gcols)

    samples, median, _ = s.measure(("run", "allsky"), step, TAGS)
    f = out.to_host((s.ncol, api.GRT_ALLSKY_FLUXES_PER_COLUMN))
    result = {"workload": s.workload + "; synthetic clouds in about a third of the layers",
              "reps": s.args.reps, "order": "run, allsky alternating; medians over the repetitions",
              "median": median, "samples": samples,
              "allsky_pass_over_clear_solver": {b: median["allsky"][f"{b}_allsky_solver_ms"] / median["allsky"][f"{b}_solver_ms"]
                                                for b in ("lw", "sw")},
              "allsky_step_over_run_step": median["allsky"]["wall_ms"] / median["run"]["wall_ms"],
              "mean_abs_cloud_effect_w_m2": {"lw_up_toa": float(np.mean(np.abs(f[:, 12] - f[:, 0]))),
                                             "lw_down_surface": float(np.mean(np.abs(f[:, 16] - f[:, 4]))),
                                             "sw_up_toa": float(np.mean(np.abs(f[:, 18] - f[:, 6]))),
                                             "sw_down_surface": float(np.mean(np.abs(f[:, 22] - f[:, 10])))}}
    s.finish(result, ("median", "allsky_pass_over_clear_solver", "allsky_step_over_run_step", "mean_abs_cloud_effect_w_m2"))


if __name__ == "__main__":
    main()
