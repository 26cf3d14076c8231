"""Cost of grt_pipeline_run_subcolumns against grt_pipeline_run_allsky and grt_pipeline_run_allsky_profiles on the G1
workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), with S draws of the
synthetic cloud fields of scripts/pipeline_timing.py per column and pass.

Five alternating repetitions of these steps on one pipeline:
  allsky            grt_pipeline_run_allsky on subcolumn 0 (the shortwave's one sweep where the user level allows it)
  allsky_profiles   grt_pipeline_run_allsky_profiles on subcolumn 0
  sub_S             grt_pipeline_run_subcolumns, six-row form, S = 1, 2, 4, 8
  subprof_S         grt_pipeline_run_subcolumns, profile form, S = 1, 2, 4, 8
Per step: the all-sky solver times by HIP-event profile tag (grt_ext.h: 8 / 9 longwave / shortwave, 11 the subcolumn
mean) and the wall time of the whole step, synchronised.  Result: profiles/pipeline_subcolumns_timing.json (or the path
given).

    python scripts/time_pipeline_subcolumns.py [--reps 5] [--out profiles/pipeline_subcolumns_timing.json]
"""
from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

TAGS = {"lw_allsky_solver_ms": api.TAG_ALLSKY_LW, "sw_allsky_solver_ms": api.TAG_ALLSKY_SW,
        "subcolumn_mean_ms": api.TAG_SUBCOLUMN_MEAN}
COUNTS = (1, 2, 4, 8)


def main():
    s = Session("pipeline_subcolumns_timing.json")
    pipe, gcols, lib, C = s.pipe, s.gcols, s.lib, api.C
    clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], max(COUNTS))
    out = s.buffer(api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    levels, heating, prof_out = s.profile_outputs(2)

    def step(mode):
        kind, _, n = mode.partition("_")
        if mode == "allsky":
            api.check(lib.grt_pipeline_run_allsky(pipe.p, C.byref(gcols), C.byref(clouds[1][0]), out.ptr))
        elif mode == "allsky_profiles":
            api.check(lib.grt_pipeline_run_allsky_profiles(pipe.p, C.byref(gcols), C.byref(clouds[1][0]), levels.ptr,
                                                           heating.ptr, prof_out.ptr))
        elif kind == "sub":
            api.check(lib.grt_pipeline_run_subcolumns(pipe.p, C.byref(gcols), C.byref(clouds[int(n)][0]), int(n), None,
                                                      None, out.ptr))
        else:
            api.check(lib.grt_pipeline_run_subcolumns(pipe.p, C.byref(gcols), C.byref(clouds[int(n)][0]), int(n),
                                                      levels.ptr, heating.ptr, prof_out.ptr))

    modes = ["allsky", "allsky_profiles"] + [f"sub_{n}" for n in COUNTS] + [f"subprof_{n}" for n in COUNTS]
    samples, median, _ = s.measure(modes, step, TAGS)
    solver = {m: median[m]["lw_allsky_solver_ms"] + median[m]["sw_allsky_solver_ms"] for m in modes}
    result = {"workload": s.workload + "; synthetic clouds in about a third of the layers of each subcolumn",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "samples": samples,
              "six_row_step_over_allsky_step": {n: median[f"sub_{n}"]["wall_ms"] / median["allsky"]["wall_ms"]
                                                for n in COUNTS},
              "profile_step_over_allsky_profiles_step": {
                  n: median[f"subprof_{n}"]["wall_ms"] / median["allsky_profiles"]["wall_ms"] for n in COUNTS},
              "allsky_solver_over_s1": {
                  "six_row": {n: solver[f"sub_{n}"] / solver["sub_1"] for n in COUNTS},
                  "profile": {n: solver[f"subprof_{n}"] / solver["subprof_1"] for n in COUNTS}},
              "subcolumn_mean_ms": {m: median[m]["subcolumn_mean_ms"] for m in modes if m.split("_")[-1] != "1"},
              "targets": {"six_row_step_s8_over_allsky": 1.35, "profile_step_s4_over_allsky_profiles": 1.35,
                          "allsky_solver_s8_over_s1": 8.5, "subcolumn_mean_ms": 1.0}}
    s.finish(result, ("six_row_step_over_allsky_step", "profile_step_over_allsky_profiles_step", "allsky_solver_over_s1",
                      "subcolumn_mean_ms"))


if __name__ == "__main__":
    main()
