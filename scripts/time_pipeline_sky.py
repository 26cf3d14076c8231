"""Cost of grt_pipeline_run_sky against the two calls it replaces, on the G1 workload (grtcode_amd.workload: 64 columns,
61 levels, the bench's grids and line lists, fast = 3), with the synthetic aerosol of scripts/time_pipeline_aerosols.py and
S draws of the synthetic cloud fields of scripts/pipeline_timing.py per column and pass.

Five alternating repetitions of these steps on one pipeline, in one process, six-row form:
  two_calls    grt_pipeline_run_aerosols, then grt_pipeline_run_subcolumns: two gas-optics passes and two clear-clean solves
               per band; what a caller had to do for the aerosol and the cloud set of a column
  sky_two      grt_pipeline_run_sky with GRT_SKY_AEROSOL | GRT_SKY_CLOUD: the same outputs (clean, aerosol, cloud) from one
               gas-optics pass and one clear-clean solve per band
  sky_four     grt_pipeline_run_sky with all four sets: the complete set (aerosol and clouds) as well
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 1 / 2 and 6 / 7 gas optics, 3 / 4 clear-clean, 12 / 13
aerosol pass, 8 / 9 all-sky pass, 17 / 18 the pass with both, 11 the subcolumn mean) and the wall time of the whole step,
synchronised.  Required: sky_two below two_calls.  Result: profiles/pipeline_sky_timing.json (or the path given).

    python scripts/time_pipeline_sky.py [--reps 5] [--subcolumns 4] [--out profiles/pipeline_sky_timing.json]
"""
from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_aerosols import synthetic_aerosols

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW,
        "lw_clear_ms": api.TAG_SOLVER_LW, "sw_clear_ms": api.TAG_SOLVER_SW, "lw_aerosol_ms": api.TAG_AEROSOL_LW,
        "sw_aerosol_ms": api.TAG_AEROSOL_SW, "lw_allsky_ms": api.TAG_ALLSKY_LW, "sw_allsky_ms": api.TAG_ALLSKY_SW,
        "lw_sky_ms": api.TAG_SKY_LW, "sw_sky_ms": api.TAG_SKY_SW, "subcolumn_mean_ms": api.TAG_SUBCOLUMN_MEAN}


def main():
    s = Session("pipeline_sky_timing.json", lambda ap: ap.add_argument("--subcolumns", type=int, default=4))
    pipe, gcols, lib, C, ncol, V, S = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.subcolumns
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], S)[S]   # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    sky = {"sky_two": api.make_sky(gclouds, gaer, S, api.GRT_SKY_AEROSOL | api.GRT_SKY_CLOUD),
           "sky_four": api.make_sky(gclouds, gaer, S, api.GRT_SKY_ALL)}
    aer_out, sub_out = s.buffer(api.GRT_ALLSKY_FLUXES_PER_COLUMN), s.buffer(api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    sky_out = s.buffer(api.GRT_SKY_MAX_SETS * api.GRT_FLUXES_PER_COLUMN)

    def step(mode):
        if mode == "two_calls":
            api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gcols), C.byref(gaer), None, None, aer_out.ptr))
            api.check(lib.grt_pipeline_run_subcolumns(pipe.p, C.byref(gcols), C.byref(gclouds), S, None, None, sub_out.ptr))
        else:
            api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(sky[mode][0]), None, None, sky_out.ptr))

    modes = ["two_calls", "sky_two", "sky_four"]
    samples, median, spread = s.measure(modes, step, TAGS)
    wall = {m: median[m]["wall_ms"] for m in modes}
    result = {"workload": s.workload + f"; synthetic aerosol on 16 points per band, {S} draws of synthetic clouds in about a "
                                       "third of the layers",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples, "wall_ms": wall,
              "wall_spread_ms": {m: spread[m]["wall_ms"] for m in modes},
              "sky_two_over_two_calls": wall["sky_two"] / wall["two_calls"],
              "sky_four_over_two_calls": wall["sky_four"] / wall["two_calls"],
              "sky_two_below_two_calls": bool(wall["sky_two"] < wall["two_calls"])}
    s.finish(result, ("wall_ms", "wall_spread_ms", "sky_two_over_two_calls", "sky_four_over_two_calls",
                      "sky_two_below_two_calls", "median"))


if __name__ == "__main__":
    main()
