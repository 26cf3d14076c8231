"""Cost of grt_pipeline_run_band_profiles against grt_pipeline_run_profiles and grt_pipeline_run_allsky_profiles on the G1
workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3).

Five alternating repetitions of four steps on one pipeline:
  profiles              grt_pipeline_run_profiles
  band_profiles         grt_pipeline_run_band_profiles, clear sky, --bins contiguous bins of equal width per band
  allsky_profiles       grt_pipeline_run_allsky_profiles (pipeline_timing.py's synthetic clouds)
  allsky_band_profiles  grt_pipeline_run_band_profiles with the same clouds and bins
Per step: the solver times (HIP-event profile tags 3 / 4, all-sky pass 8 / 9), the per-bin reduction and heating-rate
kernel (tag 14) and the wall time of the whole step, synchronised, with each one's spread (max - min) over the
repetitions.  Result: profiles/pipeline_band_profiles_timing.json (or the path given).

    python scripts/time_pipeline_band_profiles.py [--reps 5] [--bins 16] [--out profiles/pipeline_band_profiles_timing.json]
"""
import numpy as np

from pipeline_timing import Session, synthetic_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

TAGS = {"lw_solver_ms": api.TAG_SOLVER_LW, "sw_solver_ms": api.TAG_SOLVER_SW,
        "lw_allsky_solver_ms": api.TAG_ALLSKY_LW, "sw_allsky_solver_ms": api.TAG_ALLSKY_SW, "bins_ms": api.TAG_BAND_PROFILES}


def equal_bins(n, bins):
    """grid-point edges of `bins` contiguous bins over the whole grid, as equal as they come"""
    return np.unique(np.round(np.linspace(0, n - 1, bins + 1)).astype(np.int32))


def main():
    s = Session("pipeline_band_profiles_timing.json", lambda ap: ap.add_argument("--bins", type=int, default=16))
    pipe, gcols, wl, V = s.pipe, s.gcols, s.wl, s.V
    gclouds, keep_clouds = synthetic_clouds(s.keep["p"], s.keep["tl"])
    el, es = equal_bins(wl.grid_lw.n, s.args.bins), equal_bins(wl.grid_sw.n, s.args.bins)
    nbl, nbs = el.size - 1, es.size - 1
    levels, heating, fluxes = s.profile_outputs(2)
    band_levels = s.buffer(2 * 2 * (nbl + nbs) * V)
    band_heating = s.buffer(2 * (nbl + nbs) * (V - 1))
    ptr = lambda e: e.ctypes.data_as(api.C.c_void_p)  # noqa: E731

    def step(mode):
        cl = api.C.byref(gclouds) if mode.startswith("allsky") else None
        if mode == "profiles":
            api.check(s.lib.grt_pipeline_run_profiles(pipe.p, api.C.byref(gcols), levels.ptr, heating.ptr, fluxes.ptr))
        elif mode == "allsky_profiles":
            api.check(s.lib.grt_pipeline_run_allsky_profiles(pipe.p, api.C.byref(gcols), cl, levels.ptr, heating.ptr,
                                                             fluxes.ptr))
        else:
            api.check(s.lib.grt_pipeline_run_band_profiles(pipe.p, api.C.byref(gcols), cl, ptr(el), nbl, ptr(es), nbs,
                                                           band_levels.ptr, band_heating.ptr))

    modes = ("profiles", "band_profiles", "allsky_profiles", "allsky_band_profiles")
    samples, median, spread = s.measure(modes, step, TAGS)
    ratios = {"band_over_profile_solver": {b: median["band_profiles"][f"{b}_solver_ms"] / median["profiles"][f"{b}_solver_ms"]
                                           for b in ("lw", "sw")},
              "allsky_band_over_allsky_profile_solver": {
                  b: median["allsky_band_profiles"][f"{b}_allsky_solver_ms"] / median["allsky_profiles"][f"{b}_allsky_solver_ms"]
                  for b in ("lw", "sw")},
              "band_over_profile_step": median["band_profiles"]["wall_ms"] / median["profiles"]["wall_ms"],
              "allsky_band_over_allsky_profile_step":
                  median["allsky_band_profiles"]["wall_ms"] / median["allsky_profiles"]["wall_ms"]}
    result = {"workload": s.workload,
              "bins": f"{nbl} longwave, {nbs} shortwave, contiguous over the whole grid",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians and spreads over the repetitions",
              "median": median, "spread": spread, "ratios": ratios, "samples": samples}
    s.finish(result, ("median", "spread", "ratios"))


if __name__ == "__main__":
    main()
