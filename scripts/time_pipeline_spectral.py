"""Cost of grt_pipeline_run_spectral against grt_pipeline_run and grt_pipeline_run_allsky on the G1 workload
(grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3).

Five alternating repetitions of four steps on one pipeline:
  run              grt_pipeline_run
  spectral         grt_pipeline_run_spectral, clear sky, 10 cm-1 bins in both bands
  allsky           grt_pipeline_run_allsky (time_pipeline_allsky.py's synthetic clouds)
  allsky_spectral  grt_pipeline_run_spectral with the same clouds and bins
Per step: the solver times (HIP-event profile tags 3 / 4, all-sky pass 8 / 9), the binning kernel (tag 10) and the wall
time of the whole step, synchronised.  Result: profiles/pipeline_spectral_timing.json (or the path given).

    python scripts/time_pipeline_spectral.py [--reps 5] [--bin-width 10] [--out profiles/pipeline_spectral_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from grtcode_amd import api, workload as W  # noqa: E402
from time_pipeline_allsky import synthetic_clouds  # noqa: E402

TAGS = {"lw_solver_ms": 3, "sw_solver_ms": 4, "lw_allsky_solver_ms": 8, "sw_allsky_solver_ms": 9, "bins_ms": 10}


def edges_every(n, points):
    """grid-point edges every `points` points from the first, the last bin shorter"""
    return np.unique(np.append(np.arange(0, n, points), n - 1)).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--bin-width", type=float, default=10.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_spectral_timing.json"))
    args = ap.parse_args()
    device = api.create_device(0)
    ncol = args.columns
    wl = W.G1Workload(device, ncol, fast=3)
    (gcols, keep), _ = wl.columns(0, ncol)
    pipe = wl.pipe
    V = wl.num_levels
    gclouds, keep_clouds = synthetic_clouds(keep["p"], keep["tl"])
    nl, ns = wl.grid_lw.n, wl.grid_sw.n
    el = edges_every(nl, max(int(round(args.bin_width / wl.grid_lw.dw)), 1))
    es = edges_every(ns, max(int(round(args.bin_width / wl.grid_sw.dw)), 1))
    nbl, nbs = el.size - 1, es.size - 1
    out = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    spectral = api.DeviceBuffer(device, 8 * ncol * 2 * 6 * (nl + ns))
    binned = api.DeviceBuffer(device, 8 * ncol * 2 * 6 * (nbl + nbs))
    fluxes = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    lib = api.load_library()
    ptr = lambda e: e.ctypes.data_as(api.C.c_void_p)  # noqa: E731

    def step(mode):
        if mode == "run":
            pipe.run(gcols)
        elif mode == "allsky":
            api.check(lib.grt_pipeline_run_allsky(pipe.p, api.C.byref(gcols), api.C.byref(gclouds), out.ptr))
        else:
            cl = api.C.byref(gclouds) if mode == "allsky_spectral" else None
            api.check(lib.grt_pipeline_run_spectral(pipe.p, api.C.byref(gcols), cl, ptr(el), nbl, ptr(es), nbs,
                                                    spectral.ptr, binned.ptr, fluxes.ptr))
        pipe.sync()

    api.profile_enable(True)
    modes = ("run", "spectral", "allsky", "allsky_spectral")
    for mode in modes:                       # warm-up: every buffer allocated, every kernel loaded
        step(mode)
    samples = {m: {k: [] for k in list(TAGS) + ["wall_ms"]} for m in modes}
    for rep in range(args.reps):
        for mode in modes:
            api.profile_read(1, reset=True)
            t0 = time.perf_counter()
            step(mode)
            wall = 1e3 * (time.perf_counter() - t0)
            for k, tag in TAGS.items():
                samples[mode][k].append(api.profile_read(tag)[0])
            samples[mode]["wall_ms"].append(wall)
    api.profile_enable(False)
    median = {m: {k: statistics.median(v) for k, v in s.items()} for m, s in samples.items()}
    ratios = {"spectral_over_six_row_solver": {b: median["spectral"][f"{b}_solver_ms"] / median["run"][f"{b}_solver_ms"]
                                               for b in ("lw", "sw")},
              "allsky_spectral_over_six_row_solver": {
                  b: median["allsky_spectral"][f"{b}_allsky_solver_ms"] / median["allsky"][f"{b}_allsky_solver_ms"]
                  for b in ("lw", "sw")},
              "spectral_over_run_step": median["spectral"]["wall_ms"] / median["run"]["wall_ms"],
              "allsky_spectral_over_allsky_step": median["allsky_spectral"]["wall_ms"] / median["allsky"]["wall_ms"],
              "bins_ms_per_set": median["spectral"]["bins_ms"]}
    result = {"workload": f"G1: {ncol} columns, {V} levels, LW {nl} + SW {ns} points, fast 3",
              "bins": f"every {args.bin_width} cm-1: {nbl} longwave, {nbs} shortwave",
              "reps": args.reps, "order": "run, spectral, allsky, allsky_spectral alternating; medians over the repetitions",
              "median": median, "ratios": ratios, "samples": samples}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"median": median, "ratios": ratios}))
    for b in (out, spectral, binned, fluxes):
        b.free()
    wl.destroy()


if __name__ == "__main__":
    main()
