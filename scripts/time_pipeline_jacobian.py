"""Cost of the surface-temperature Jacobian of grt_pipeline_run_sky_jacobian over grt_pipeline_run_sky, on the G1 workload
(grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), all four sets, with the
synthetic aerosol of scripts/time_pipeline_aerosols.py and S draws of the synthetic cloud fields of
scripts/pipeline_timing.py per column and pass.

Alternating repetitions of these steps on one pipeline, in one process:
  sky_six          grt_pipeline_run_sky, six-row form
  jacobian_six     grt_pipeline_run_sky_jacobian, six-row form: the same launches, the longwave's in the instances whose
                   upward sweep carries the four derivatives too
  sky_levels       grt_pipeline_run_sky, profile form
  jacobian_levels  grt_pipeline_run_sky_jacobian, profile form, jacobian_level_fluxes_dev given
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 3 clear-clean, 12 aerosol pass, 8 all-sky pass, 17 the
pass with both -- the longwave solvers, which are what the Jacobian rides in --, their shortwave counterparts, the gas
optics, the subcolumn mean and 24, the materialised form's Jacobian kernel, which the fused form never launches) and the
wall time of the whole step, synchronised.  Reported, not gated: the wall times, and the ratio of the longwave solver
tags' sum, jacobian over sky, per form, with the spread of the repetitions.
Result: profiles/pipeline_jacobian_timing.json (or the path given).

    python scripts/time_pipeline_jacobian.py [--reps 5] [--subcolumns 4] [--out profiles/pipeline_jacobian_timing.json]
"""
from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_aerosols import synthetic_aerosols

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW,
        "lw_clear_ms": api.TAG_SOLVER_LW, "sw_clear_ms": api.TAG_SOLVER_SW, "lw_aerosol_ms": api.TAG_AEROSOL_LW,
        "sw_aerosol_ms": api.TAG_AEROSOL_SW, "lw_allsky_ms": api.TAG_ALLSKY_LW, "sw_allsky_ms": api.TAG_ALLSKY_SW,
        "lw_sky_ms": api.TAG_SKY_LW, "sw_sky_ms": api.TAG_SKY_SW, "subcolumn_mean_ms": api.TAG_SUBCOLUMN_MEAN,
        "surface_jacobian_ms": api.TAG_SURFACE_JACOBIAN}
LW_SOLVERS = ("lw_clear_ms", "lw_aerosol_ms", "lw_allsky_ms", "lw_sky_ms")


def main():
    s = Session("pipeline_jacobian_timing.json", lambda ap: ap.add_argument("--subcolumns", type=int, default=4))
    pipe, gcols, lib, C, ncol, V, S = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.subcolumns
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], S)[S]   # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    gsky, keep_sky = api.make_sky(gclouds, gaer, S, api.GRT_SKY_ALL)
    N = api.GRT_SKY_MAX_SETS
    six = s.buffer(N * api.GRT_FLUXES_PER_COLUMN)
    levels = s.buffer(N * api.GRT_PROFILE_ROWS_PER_COLUMN * V)
    heating = s.buffer(N * api.GRT_HEATING_ROWS_PER_COLUMN * (V - 1))
    jac = api.GrtSurfaceJacobian(s.buffer(N * api.GRT_JACOBIAN_ROWS_PER_SET).ptr, None)
    jac_levels = api.GrtSurfaceJacobian(jac.jacobian_fluxes_dev, s.buffer(N * V).ptr)
    forms = {"six": (None, None, six.ptr), "levels": (levels.ptr, heating.ptr, six.ptr)}

    def step(mode):
        entry, form = mode.split("_")
        if entry == "sky":
            api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(gsky), *forms[form]))
        else:
            api.check(lib.grt_pipeline_run_sky_jacobian(pipe.p, C.byref(gcols), C.byref(gsky),
                                                        C.byref(jac if form == "six" else jac_levels), *forms[form]))

    modes = ["sky_six", "jacobian_six", "sky_levels", "jacobian_levels"]
    samples, median, spread = s.measure(modes, step, TAGS)

    def solvers(mode, rep):
        return sum(samples[mode][k][rep] for k in LW_SOLVERS)

    ratios = {form: [solvers("jacobian_" + form, r) / solvers("sky_" + form, r) for r in range(s.args.reps)]
              for form in ("six", "levels")}
    result = {"workload": s.workload + f"; all four sets, synthetic aerosol on 16 points per band, {S} draws of synthetic "
                                       "clouds in about a third of the layers",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "lw_solver_tags_ms": {m: [solvers(m, r) for r in range(s.args.reps)] for m in modes},
              "jacobian_over_sky_lw_solver_tags": ratios,
              "jacobian_over_sky_spread": {form: max(r) - min(r) for form, r in ratios.items()},
              "wall_ms": {m: median[m]["wall_ms"] for m in modes}}
    s.finish(result, ("wall_ms", "lw_solver_tags_ms", "jacobian_over_sky_lw_solver_tags", "jacobian_over_sky_spread"))


if __name__ == "__main__":
    main()
