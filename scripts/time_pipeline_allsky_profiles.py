"""Cost of grt_pipeline_run_allsky_profiles against grt_pipeline_run_allsky on the G1 workload (grtcode_amd.workload: 64
columns, 61 levels, the bench's grids and line lists, fast = 3), with the synthetic cloud fields of
scripts/time_pipeline_allsky.py.

Five alternating repetitions of three steps on one pipeline:
  allsky            grt_pipeline_run_allsky, default (the shortwave's one sweep where the user level allows it)
  allsky_two        grt_pipeline_run_allsky with GRT_SW_TWO_SWEEPS=1 (the reference's two sweeps)
  allsky_profiles   grt_pipeline_run_allsky_profiles (level fluxes and heating rates of both passes)
Per step: the solver times by HIP-event profile tag (grt_ext.h: 3 / 4 longwave / shortwave clear-sky solver, 8 / 9 the
all-sky pass's) and the wall time of the whole step, synchronised.  Result: profiles/pipeline_allsky_profiles_timing.json
(or the path given).

    python scripts/time_pipeline_allsky_profiles.py [--reps 5] [--out profiles/pipeline_allsky_profiles_timing.json]
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

TAGS = {"lw_solver_ms": 3, "sw_solver_ms": 4, "lw_allsky_solver_ms": 8, "sw_allsky_solver_ms": 9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_allsky_profiles_timing.json"))
    args = ap.parse_args()
    device = api.create_device(0)
    ncol = args.columns
    wl = W.G1Workload(device, ncol, fast=3)
    (gcols, keep), _ = wl.columns(0, ncol)
    pipe = wl.pipe
    V = wl.num_levels
    gclouds, keep_clouds = synthetic_clouds(keep["p"], keep["tl"])
    out = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    levels = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN * V)
    heating = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_HEATING_ROWS_PER_COLUMN * (V - 1))
    prof_out = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    lib = api.load_library()

    def step(mode):
        if mode == "allsky_profiles":
            api.check(lib.grt_pipeline_run_allsky_profiles(pipe.p, api.C.byref(gcols), api.C.byref(gclouds),
                                                           levels.ptr, heating.ptr, prof_out.ptr))
        else:
            if mode == "allsky_two":
                os.environ["GRT_SW_TWO_SWEEPS"] = "1"
            try:
                api.check(lib.grt_pipeline_run_allsky(pipe.p, api.C.byref(gcols), api.C.byref(gclouds), out.ptr))
            finally:
                os.environ.pop("GRT_SW_TWO_SWEEPS", None)
        pipe.sync()

    api.profile_enable(True)
    modes = ("allsky", "allsky_two", "allsky_profiles")
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
    f = prof_out.to_host((ncol, api.GRT_ALLSKY_FLUXES_PER_COLUMN))
    hr = heating.to_host((ncol, api.GRT_ALLSKY_HEATING_ROWS_PER_COLUMN, V - 1))
    median = {m: {k: statistics.median(v) for k, v in s.items()} for m, s in samples.items()}
    prof, two, one = median["allsky_profiles"], median["allsky_two"], median["allsky"]
    result = {"workload": f"G1: {ncol} columns, {V} levels, LW {wl.grid_lw.n} + SW {wl.grid_sw.n} points, fast 3; "
                          "synthetic clouds in about a third of the layers",
              "reps": args.reps, "order": "allsky, allsky_two, allsky_profiles alternating; medians over the repetitions",
              "median": median, "samples": samples,
              "allsky_profile_solver_over_two_sweep_allsky_solver": {
                  b: prof[f"{b}_allsky_solver_ms"] / two[f"{b}_allsky_solver_ms"] for b in ("lw", "sw")},
              "allsky_profile_solver_over_one_sweep_allsky_solver": {
                  b: prof[f"{b}_allsky_solver_ms"] / one[f"{b}_allsky_solver_ms"] for b in ("lw", "sw")},
              "allsky_profiles_step_over_allsky_step": prof["wall_ms"] / one["wall_ms"],
              "targets": {"solver_over_two_sweep": 1.5, "step_over_allsky_step": 1.10},
              "mean_abs_cloud_effect_on_heating_k_day": {
                  "lw": float(np.mean(np.abs(hr[:, 2] - hr[:, 0]))), "sw": float(np.mean(np.abs(hr[:, 3] - hr[:, 1])))},
              # (largest difference of the 24 values from the last two-sweep run_allsky, relative to the largest value:
              # the gas optics of the default mode add with atomics, so two calls agree to rounding, not to the bit)
              "fluxes_equal_run_allsky_to": float(np.max(np.abs(f - out.to_host(f.shape))) / np.abs(f).max())}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(result, fo, indent=1)
    print(json.dumps({k: result[k] for k in ("median", "allsky_profile_solver_over_two_sweep_allsky_solver",
                                             "allsky_profiles_step_over_allsky_step",
                                             "mean_abs_cloud_effect_on_heating_k_day", "fluxes_equal_run_allsky_to")}))
    for b in (out, levels, heating, prof_out):
        b.free()
    wl.destroy()


if __name__ == "__main__":
    main()
