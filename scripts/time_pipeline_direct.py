"""Cost of the direct-beam rows of grt_pipeline_run_sky_direct over grt_pipeline_run_sky, on the G1 workload
(grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), all four sets, with the
synthetic aerosol of scripts/time_pipeline_aerosols.py and S draws of the synthetic cloud fields of
scripts/pipeline_timing.py per column and pass.

Alternating repetitions of these steps on one pipeline, in one process:
  sky_six        grt_pipeline_run_sky, six-row form
  direct_six     grt_pipeline_run_sky_direct, six-row form: the same launches in the instances that leave the direct beam too
  sky_levels     grt_pipeline_run_sky, profile form
  direct_levels  grt_pipeline_run_sky_direct, profile form, direct_level_fluxes_dev given
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 4 clear-clean, 13 aerosol pass, 9 all-sky pass, 18 the
pass with both -- the shortwave solvers, which are what the direct beam rides in --, their longwave counterparts, the gas
optics and the subcolumn mean) and the wall time of the whole step, synchronised.  Reported, not gated: the ratio of
the shortwave solver tags' sum, direct over sky, per form, with the spread of the repetitions.
Result: profiles/pipeline_direct_timing.json (or the path given).

    python scripts/time_pipeline_direct.py [--reps 3] [--subcolumns 3] [--out profiles/pipeline_direct_timing.json]
"""
from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_aerosols import synthetic_aerosols

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW,
        "lw_clear_ms": api.TAG_SOLVER_LW, "sw_clear_ms": api.TAG_SOLVER_SW, "lw_aerosol_ms": api.TAG_AEROSOL_LW,
        "sw_aerosol_ms": api.TAG_AEROSOL_SW, "lw_allsky_ms": api.TAG_ALLSKY_LW, "sw_allsky_ms": api.TAG_ALLSKY_SW,
        "lw_sky_ms": api.TAG_SKY_LW, "sw_sky_ms": api.TAG_SKY_SW, "subcolumn_mean_ms": api.TAG_SUBCOLUMN_MEAN}
SW_SOLVERS = ("sw_clear_ms", "sw_aerosol_ms", "sw_allsky_ms", "sw_sky_ms")


def main():
    s = Session("pipeline_direct_timing.json", lambda ap: ap.add_argument("--subcolumns", type=int, default=3))
    pipe, gcols, lib, C, ncol, V, S = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.subcolumns
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], S)[S]   # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    gsky, keep_sky = api.make_sky(gclouds, gaer, S, api.GRT_SKY_ALL)
    N = api.GRT_SKY_MAX_SETS
    six = s.buffer(N * api.GRT_FLUXES_PER_COLUMN)
    levels = s.buffer(N * api.GRT_PROFILE_ROWS_PER_COLUMN * V)
    heating = s.buffer(N * api.GRT_HEATING_ROWS_PER_COLUMN * (V - 1))
    direct = api.GrtDirectBeam(s.buffer(N * api.GRT_DIRECT_ROWS_PER_SET).ptr, None)
    direct_levels = api.GrtDirectBeam(direct.direct_fluxes_dev, s.buffer(N * V).ptr)
    forms = {"six": (None, None, six.ptr), "levels": (levels.ptr, heating.ptr, six.ptr)}

    def step(mode):
        entry, form = mode.split("_")
        if entry == "sky":
            api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(gsky), *forms[form]))
        else:
            api.check(lib.grt_pipeline_run_sky_direct(pipe.p, C.byref(gcols), C.byref(gsky),
                                                      C.byref(direct if form == "six" else direct_levels), *forms[form]))

    modes = ["sky_six", "direct_six", "sky_levels", "direct_levels"]
    samples, median, spread = s.measure(modes, step, TAGS)

    def solvers(mode, rep):
        return sum(samples[mode][k][rep] for k in SW_SOLVERS)

    ratios = {form: [solvers("direct_" + form, r) / solvers("sky_" + form, r) for r in range(s.args.reps)]
              for form in ("six", "levels")}
    result = {"workload": s.workload + f"; all four sets, synthetic aerosol on 16 points per band, {S} draws of synthetic "
                                       "clouds in about a third of the layers",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "sw_solver_tags_ms": {m: [solvers(m, r) for r in range(s.args.reps)] for m in modes},
              "direct_over_sky_sw_solver_tags": ratios,
              "direct_over_sky_spread": {form: max(r) - min(r) for form, r in ratios.items()},
              "wall_ms": {m: median[m]["wall_ms"] for m in modes}}
    s.finish(result, ("sw_solver_tags_ms", "direct_over_sky_sw_solver_tags", "direct_over_sky_spread", "wall_ms"))


if __name__ == "__main__":
    main()
