"""Cost of grt_pipeline_run_aerosols against grt_pipeline_run, grt_pipeline_run_allsky and grt_pipeline_run_allsky_profiles
on the G1 workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), with a
synthetic aerosol on NA = 16 points per band and the synthetic clouds of scripts/pipeline_timing.py.

Five alternating repetitions of these steps on one pipeline, in one process:
  run               grt_pipeline_run
  allsky            grt_pipeline_run_allsky (the yardstick of the six-row aerosol step)
  allsky_profiles   grt_pipeline_run_allsky_profiles (the yardstick of the aerosol profile step)
  aerosols          grt_pipeline_run_aerosols, six-row form
  aerosol_profiles  grt_pipeline_run_aerosols, profile form
Per step: the solver times by HIP-event profile tag (grt_ext.h: 3 / 4 clear, 8 / 9 all-sky, 12 / 13 aerosol pass) and the
wall time of the whole step, synchronised.  Required: each aerosol step no slower than its yardstick plus that yardstick's
spread (max - min over the repetitions) in this run; likewise tags 12 / 13 against 8 / 9.  Result:
profiles/pipeline_aerosols_timing.json (or the path given).

    python scripts/time_pipeline_aerosols.py [--reps 5] [--out profiles/pipeline_aerosols_timing.json]
"""
import numpy as np

from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

TAGS = {"lw_clear_ms": api.TAG_SOLVER_LW, "sw_clear_ms": api.TAG_SOLVER_SW, "lw_allsky_ms": api.TAG_ALLSKY_LW,
        "sw_allsky_ms": api.TAG_ALLSKY_SW, "lw_aerosol_ms": api.TAG_AEROSOL_LW, "sw_aerosol_ms": api.TAG_AEROSOL_SW}
NA = 16


def synthetic_aerosols(grid, ncol, L, seed, lw):
    """NA irregular points inside the band (its ends have no aerosol); optical depth decaying with height, albedo and
    asymmetry varying along the grid and between the columns."""
    rng = np.random.default_rng(seed)
    span = grid.wn - grid.w0
    x = grid.w0 + span * np.sort(0.05 + 0.9 * (np.arange(NA) + 0.8 * rng.random(NA)) / NA)
    height = np.exp(-3.0 * (L - 1 - np.arange(L)) / (L - 1))[None, :, None]
    o = np.zeros((ncol, 3, L, NA))
    o[:, 0] = 0.2 * height * (0.5 + rng.random((ncol, 1, NA))) * (0.8 + 0.4 * rng.random((ncol, L, NA)))
    o[:, 1] = (0.2 + 0.4 * rng.random((ncol, L, NA))) if lw else (0.85 + 0.14 * rng.random((ncol, L, NA)))
    o[:, 2] = 0.5 + 0.3 * rng.random((ncol, L, NA))
    return x, o


def main():
    s = Session("pipeline_aerosols_timing.json")
    pipe, gcols, lib, C, ncol, V = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], 1)[1]   # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    out = s.buffer(api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    levels, heating, prof_out = s.profile_outputs(2)

    def step(mode):
        if mode == "run":
            api.check(lib.grt_pipeline_run(pipe.p, C.byref(gcols), out.ptr))
        elif mode == "allsky":
            api.check(lib.grt_pipeline_run_allsky(pipe.p, C.byref(gcols), C.byref(gclouds), out.ptr))
        elif mode == "allsky_profiles":
            api.check(lib.grt_pipeline_run_allsky_profiles(pipe.p, C.byref(gcols), C.byref(gclouds), levels.ptr, heating.ptr,
                                                           prof_out.ptr))
        elif mode == "aerosols":
            api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gcols), C.byref(gaer), None, None, out.ptr))
        else:
            api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gcols), C.byref(gaer), levels.ptr, heating.ptr,
                                                    prof_out.ptr))

    modes = ["run", "allsky", "allsky_profiles", "aerosols", "aerosol_profiles"]
    samples, median, spread = s.measure(modes, step, TAGS)

    def target(new, new_key, yard, yard_key):
        got, limit = median[new][new_key], median[yard][yard_key] + spread[yard][yard_key]
        return {"median_ms": got, "yardstick_median_ms": median[yard][yard_key], "yardstick_spread_ms": spread[yard][yard_key],
                "ratio": got / median[yard][yard_key], "met": bool(got <= limit)}

    checks = {"six_row_step_vs_allsky_step": target("aerosols", "wall_ms", "allsky", "wall_ms"),
              "profile_step_vs_allsky_profiles_step": target("aerosol_profiles", "wall_ms", "allsky_profiles", "wall_ms"),
              "six_row_lw_tag12_vs_tag8": target("aerosols", "lw_aerosol_ms", "allsky", "lw_allsky_ms"),
              "six_row_sw_tag13_vs_tag9": target("aerosols", "sw_aerosol_ms", "allsky", "sw_allsky_ms"),
              "profile_lw_tag12_vs_tag8": target("aerosol_profiles", "lw_aerosol_ms", "allsky_profiles", "lw_allsky_ms"),
              "profile_sw_tag13_vs_tag9": target("aerosol_profiles", "sw_aerosol_ms", "allsky_profiles", "sw_allsky_ms")}
    result = {"workload": s.workload + f"; synthetic aerosol on {NA} points per band, synthetic clouds in about a third of the "
                                       "layers",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples, "targets": checks,
              "step_over_run_step": {m: median[m]["wall_ms"] / median["run"]["wall_ms"] for m in modes}}
    s.finish(result, ("targets", "step_over_run_step"))


if __name__ == "__main__":
    main()
