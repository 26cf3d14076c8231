"""Cost of grt_pipeline_run_spectral against grt_pipeline_run and grt_pipeline_run_allsky on the G1 workload
(grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3).

Five alternating repetitions of four steps on one pipeline:
  run              grt_pipeline_run
  spectral         grt_pipeline_run_spectral, clear sky, 10 cm-1 bins in both bands
  allsky           grt_pipeline_run_allsky (pipeline_timing.py's synthetic clouds)
  allsky_spectral  grt_pipeline_run_spectral with the same clouds and bins
Per step: the solver times (HIP-event profile tags 3 / 4, all-sky pass 8 / 9), the binning kernel (tag 10) and the wall
time of the whole step, synchronised.  Result: profiles/pipeline_spectral_timing.json (or the path given).

    python scripts/time_pipeline_spectral.py [--reps 5] [--bin-width 10] [--out profiles/pipeline_spectral_timing.json]
"""
import numpy as np

from pipeline_timing import Session, synthetic_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

TAGS = {"lw_solver_ms": api.TAG_SOLVER_LW, "sw_solver_ms": api.TAG_SOLVER_SW,
        "lw_allsky_solver_ms": api.TAG_ALLSKY_LW, "sw_allsky_solver_ms": api.TAG_ALLSKY_SW, "bins_ms": api.TAG_BINS}


def edges_every(n, points):
    """grid-point edges every `points` points from the first, the last bin shorter"""
    return np.unique(np.append(np.arange(0, n, points), n - 1)).astype(np.int32)


def main():
    s = Session("pipeline_spectral_timing.json", lambda ap: ap.add_argument("--bin-width", type=float, default=10.0))
    pipe, gcols, wl, width = s.pipe, s.gcols, s.wl, s.args.bin_width
    gclouds, keep_clouds = synthetic_clouds(s.keep["p"], s.keep["tl"])
    nl, ns = wl.grid_lw.n, wl.grid_sw.n
    el = edges_every(nl, max(int(round(width / wl.grid_lw.dw)), 1))
    es = edges_every(ns, max(int(round(width / wl.grid_sw.dw)), 1))
    nbl, nbs = el.size - 1, es.size - 1
    out = s.buffer(api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    spectral = s.buffer(2 * 6 * (nl + ns))
    binned = s.buffer(2 * 6 * (nbl + nbs))
    fluxes = s.buffer(api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    ptr = lambda e: e.ctypes.data_as(api.C.c_void_p)  # noqa: E731

    def step(mode):
        if mode == "run":
            pipe.run(gcols)
        elif mode == "allsky":
            api.check(s.lib.grt_pipeline_run_allsky(pipe.p, api.C.byref(gcols), api.C.byref(gclouds), out.ptr))
        else:
            cl = api.C.byref(gclouds) if mode == "allsky_spectral" else None
            api.check(s.lib.grt_pipeline_run_spectral(pipe.p, api.C.byref(gcols), cl, ptr(el), nbl, ptr(es), nbs,
                                                      spectral.ptr, binned.ptr, fluxes.ptr))

    samples, median, _ = s.measure(("run", "spectral", "allsky", "allsky_spectral"), step, TAGS)
    ratios = {"spectral_over_six_row_solver": {b: median["spectral"][f"{b}_solver_ms"] / median["run"][f"{b}_solver_ms"]
                                               for b in ("lw", "sw")},
              "allsky_spectral_over_six_row_solver": {
                  b: median["allsky_spectral"][f"{b}_allsky_solver_ms"] / median["allsky"][f"{b}_allsky_solver_ms"]
                  for b in ("lw", "sw")},
              "spectral_over_run_step": median["spectral"]["wall_ms"] / median["run"]["wall_ms"],
              "allsky_spectral_over_allsky_step": median["allsky_spectral"]["wall_ms"] / median["allsky"]["wall_ms"],
              "bins_ms_per_set": median["spectral"]["bins_ms"]}
    result = {"workload": s.workload,
              "bins": f"every {width} cm-1: {nbl} longwave, {nbs} shortwave",
              "reps": s.args.reps, "order": "run, spectral, allsky, allsky_spectral alternating; medians over the repetitions",
              "median": median, "ratios": ratios, "samples": samples}
    s.finish(result, ("median", "ratios"))


if __name__ == "__main__":
    main()
