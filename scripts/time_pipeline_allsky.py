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
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from grtcode_amd import api, workload as W  # noqa: E402

TAGS = {"lw_solver_ms": 3, "sw_solver_ms": 4, "lw_allsky_solver_ms": 8, "sw_allsky_solver_ms": 9}


def synthetic_clouds(p, tl, seed=1):
    """Band optics [ncol][3][B][L] of two draws (longwave, shortwave pass) and layer thickness [ncol][L] m."""
    ncol, L = tl.shape
    rng = np.random.default_rng(seed)
    liquid_edges = np.array([10.0, 350.0, 700.0, 1200.0, 2000.0, 3500.0, 8000.0, 20000.0, 50000.0])
    ice_edges = np.array([10.0, 250.0, 500.0, 800.0, 1300.0, 2200.0, 4000.0, 9000.0, 18000.0, 30000.0, 52000.0])
    B = liquid_edges.size - 1
    thickness = 29.3 * tl * np.log(p[:, 1:] / p[:, :-1])
    sets = []
    for _ in range(2):
        cloudy = rng.random((ncol, L)) < 1.0 / 3.0
        low = np.arange(L)[None, :] >= L // 2
        liq, ice = np.zeros((ncol, 3, B, L)), np.zeros((ncol, 3, B, L))
        for phase, where, ext in ((liq, cloudy & low, 2e-2), (ice, cloudy & ~low, 2e-3)):
            w = np.broadcast_to(where[:, None, :], (ncol, B, L))
            phase[:, 0] = np.where(w, ext * rng.random((ncol, B, L)), 0.0)
            phase[:, 1] = np.where(w, 0.5 + 0.49 * rng.random((ncol, B, L)), 0.0)
            phase[:, 2] = np.where(w, 0.7 + 0.2 * rng.random((ncol, B, L)), 0.0)
        sets.append((liq, ice))
    return api.make_clouds((liquid_edges[:-1], liquid_edges[1:]), (ice_edges[:-1], ice_edges[1:]), thickness,
                           sets[0][0], sets[0][1], sets[1][0], sets[1][1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_allsky_timing.json"))
    args = ap.parse_args()
    device = api.create_device(0)
    ncol = args.columns
    wl = W.G1Workload(device, ncol, fast=3)
    (gcols, keep), _ = wl.columns(0, ncol)
    pipe = wl.pipe
    V = wl.num_levels
    gclouds, keep_clouds = synthetic_clouds(keep["p"], keep["tl"])
    out = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    lib = api.load_library()

    def step(mode):
        if mode == "allsky":
            api.check(lib.grt_pipeline_run_allsky(pipe.p, api.C.byref(gcols), api.C.byref(gclouds), out.ptr))
        else:
            pipe.run(gcols)
        pipe.sync()

    api.profile_enable(True)
    modes = ("run", "allsky")
    for mode in modes:                       # warm-up: every buffer allocated, every kernel loaded
        step(mode)
    samples = {m: {**{k: [] for k in TAGS}, "wall_ms": []} for m in modes}
    for rep in range(args.reps):
        for mode in modes:
            for tag in TAGS.values():
                api.profile_read(tag, reset=True)
            api.profile_read(1, reset=True)
            t0 = time.perf_counter()
            step(mode)
            wall = 1e3 * (time.perf_counter() - t0)
            for k, tag in TAGS.items():
                samples[mode][k].append(api.profile_read(tag)[0])
            samples[mode]["wall_ms"].append(wall)
    api.profile_enable(False)
    f = out.to_host((ncol, api.GRT_ALLSKY_FLUXES_PER_COLUMN))
    median = {m: {k: statistics.median(v) for k, v in s.items()} for m, s in samples.items()}
    result = {"workload": f"G1: {ncol} columns, {V} levels, LW {wl.grid_lw.n} + SW {wl.grid_sw.n} points, fast 3; "
                          "synthetic clouds in about a third of the layers",
              "reps": args.reps, "order": "run, allsky alternating; medians over the repetitions",
              "median": median, "samples": samples,
              "allsky_pass_over_clear_solver": {b: median["allsky"][f"{b}_allsky_solver_ms"] / median["allsky"][f"{b}_solver_ms"]
                                                for b in ("lw", "sw")},
              "allsky_step_over_run_step": median["allsky"]["wall_ms"] / median["run"]["wall_ms"],
              "mean_abs_cloud_effect_w_m2": {"lw_up_toa": float(np.mean(np.abs(f[:, 12] - f[:, 0]))),
                                             "lw_down_surface": float(np.mean(np.abs(f[:, 16] - f[:, 4]))),
                                             "sw_up_toa": float(np.mean(np.abs(f[:, 18] - f[:, 6]))),
                                             "sw_down_surface": float(np.mean(np.abs(f[:, 22] - f[:, 10])))}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(result, fo, indent=1)
    print(json.dumps({k: result[k] for k in ("median", "allsky_pass_over_clear_solver", "allsky_step_over_run_step",
                                             "mean_abs_cloud_effect_w_m2")}))
    out.free()
    wl.destroy()


if __name__ == "__main__":
    main()
