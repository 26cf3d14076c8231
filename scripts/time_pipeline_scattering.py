"""Cost of grt_pipeline_run_sky_scattering against grt_pipeline_run_sky, on the G1 workload (grtcode_amd.workload: 64
columns, 61 levels, the bench's grids and line lists, fast = 3), all four sets, with the synthetic aerosol of
scripts/time_pipeline_aerosols.py and S draws of the synthetic cloud fields of scripts/pipeline_timing.py per column and
pass, S = 1 and 4.

Five alternating repetitions of these steps on one pipeline, in one process, six-row form:
  sky_S         grt_pipeline_run_sky: the four sets
  scattering_S  grt_pipeline_run_sky_scattering: the same, and behind every set's longwave solve the scattering kernel, its
                reduction and the addition
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 1 / 2 and 6 / 7 gas optics, 3, 12, 8, 17 the longwave
solves of the four sets, 38 the scattering kernel, 39 its reductions and the addition) and the wall time of the whole
step, synchronised.  There is no target: the longwave solvers are latency chains, and a second launch per
set is the expected price.  Result: profiles/pipeline_scattering_timing.json (or the path given).

    python scripts/time_pipeline_scattering.py [--reps 5] [--out profiles/pipeline_scattering_timing.json]
"""
from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_aerosols import synthetic_aerosols

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW,
        "lw_clear_ms": api.TAG_SOLVER_LW, "lw_aerosol_ms": api.TAG_AEROSOL_LW, "lw_allsky_ms": api.TAG_ALLSKY_LW,
        "lw_sky_ms": api.TAG_SKY_LW, "scatter_ms": api.TAG_SCATTER_LW, "scatter_finish_ms": api.TAG_SCATTER_FINISH}
DRAWS = (1, 4)


def main():
    s = Session("pipeline_scattering_timing.json")
    pipe, gcols, lib, C, ncol, V = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V
    clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], max(DRAWS))           # (the structs point into the kept arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    sky = {S: api.make_sky(clouds[S][0], gaer, S, api.GRT_SKY_ALL) for S in DRAWS}
    out = s.buffer(api.GRT_SKY_MAX_SETS * api.GRT_FLUXES_PER_COLUMN)
    delta = s.buffer(api.GRT_SKY_MAX_SETS * 6)

    def step(mode):
        kind, S = mode.split("_")
        gsky = sky[int(S)][0]
        if kind == "sky":
            api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(gsky), None, None, out.ptr))
        else:
            api.check(lib.grt_pipeline_run_sky_scattering(pipe.p, C.byref(gcols), C.byref(gsky), None, None, out.ptr, None,
                                                          delta.ptr))

    modes = [f"{kind}_{S}" for S in DRAWS for kind in ("sky", "scattering")]
    samples, median, spread = s.measure(modes, step, TAGS)
    wall = {m: median[m]["wall_ms"] for m in modes}
    lw = ("lw_clear_ms", "lw_aerosol_ms", "lw_allsky_ms", "lw_sky_ms")
    result = {"workload": s.workload + "; four sets, synthetic aerosol on 16 points per band, 1 and 4 draws of synthetic "
                                       "clouds in about a third of the layers",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples, "wall_ms": wall,
              "wall_spread_ms": {m: spread[m]["wall_ms"] for m in modes},
              "scattering_over_sky": {str(S): wall[f"scattering_{S}"] / wall[f"sky_{S}"] for S in DRAWS},
              "scatter_kernels_over_lw_solvers": {
                  str(S): median[f"scattering_{S}"]["scatter_ms"] / sum(median[f"scattering_{S}"][k] for k in lw)
                  for S in DRAWS}}
    s.finish(result, ("wall_ms", "wall_spread_ms", "scattering_over_sky", "scatter_kernels_over_lw_solvers"))


if __name__ == "__main__":
    main()
