"""Cost of grt_pipeline_run_aerosols against grt_pipeline_run, grt_pipeline_run_allsky and grt_pipeline_run_allsky_profiles
on the G1 workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), with a
synthetic aerosol on NA = 16 points per band and the synthetic clouds of scripts/time_pipeline_subcolumns.py.

Five alternating repetitions of these steps on one pipeline, in one process:
  run               grt_pipeline_run
  allsky            grt_pipeline_run_allsky (the yardstick of the six-row aerosol step)
  allsky_profiles   grt_pipeline_run_allsky_profiles (the yardstick of the aerosol profile step)
  aerosols          grt_pipeline_run_aerosols, six-row form
  aerosol_profiles  grt_pipeline_run_aerosols, profile form
Per step: the solver times by HIP-event profile tag (grt_ext.h: 3 / 4 clear, 8 / 9 all-sky, 12 / 13 aerosol pass) and the
wall time of the whole step, synchronised.  Required: each aerosol step no slower than its yardstick plus that yardstick's
spread (max - min over the repetitions) in this run; likewise tags 12 / 13 against 8 / 9.  Result:
profiles/pipeline_aerosols_timing.json (or the path given).

    python scripts/time_pipeline_aerosols.py [--reps 5] [--out profiles/pipeline_aerosols_timing.json]
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
from time_pipeline_subcolumns import subcolumn_clouds  # noqa: E402

TAGS = {"lw_clear_ms": 3, "sw_clear_ms": 4, "lw_allsky_ms": 8, "sw_allsky_ms": 9, "lw_aerosol_ms": 12, "sw_aerosol_ms": 13}
NA = 16


def synthetic_aerosols(grid, ncol, L, seed, lw):
    """NA irregular points inside the band (its ends have no aerosol); optical depth decaying with height, albedo and
    asymmetry varying along the grid and between the columns."""
    rng = np.random.default_rng(seed)
    span = grid.wn - grid.w0
    x = grid.w0 + span * np.sort(0.05 + 0.9 * (np.arange(NA) + 0.8 * rng.random(NA)) / NA)
    height = np.exp(-3.0 * (L - 1 - np.arange(L)) / (L - 1))[None, :, None]
    o = np.zeros((ncol, 3, L, NA))
    o[:, 0] = 0.2 * height * (0.5 + rng.random((ncol, 1, NA))) * (0.8 + 0.4 * rng.random((ncol, L, NA)))
    o[:, 1] = (0.2 + 0.4 * rng.random((ncol, L, NA))) if lw else (0.85 + 0.14 * rng.random((ncol, L, NA)))
    o[:, 2] = 0.5 + 0.3 * rng.random((ncol, L, NA))
    return x, o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_aerosols_timing.json"))
    args = ap.parse_args()
    device = api.create_device(0)
    ncol = args.columns
    wl = W.G1Workload(device, ncol, fast=3)
    (gcols, keep), _ = wl.columns(0, ncol)
    pipe = wl.pipe
    V = wl.num_levels
    gclouds, keep_clouds = subcolumn_clouds(keep["p"], keep["tl"], 1)[1]     # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(wl.grid_sw, ncol, V - 1, 4, False))
    out = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    levels = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN * V)
    heating = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_HEATING_ROWS_PER_COLUMN * (V - 1))
    prof_out = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    lib = api.load_library()
    C = api.C

    def step(mode):
        if mode == "run":
            api.check(lib.grt_pipeline_run(pipe.p, C.byref(gcols), out.ptr))
        elif mode == "allsky":
            api.check(lib.grt_pipeline_run_allsky(pipe.p, C.byref(gcols), C.byref(gclouds), out.ptr))
        elif mode == "allsky_profiles":
            api.check(lib.grt_pipeline_run_allsky_profiles(pipe.p, C.byref(gcols), C.byref(gclouds), levels.ptr, heating.ptr,
                                                           prof_out.ptr))
        elif mode == "aerosols":
            api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gcols), C.byref(gaer), None, None, out.ptr))
        else:
            api.check(lib.grt_pipeline_run_aerosols(pipe.p, C.byref(gcols), C.byref(gaer), levels.ptr, heating.ptr,
                                                    prof_out.ptr))
        pipe.sync()

    api.profile_enable(True)
    modes = ["run", "allsky", "allsky_profiles", "aerosols", "aerosol_profiles"]
    for mode in modes:                       # warm-up: every buffer allocated, every kernel loaded
        step(mode)
    samples = {m: {**{k: [] for k in TAGS}, "wall_ms": []} for m in modes}
    for rep in range(args.reps):
        for mode in modes:
            for tag in TAGS.values():
                api.profile_read(tag, reset=True)
            t0 = time.perf_counter()
            step(mode)
            wall = 1e3 * (time.perf_counter() - t0)
            for k, tag in TAGS.items():
                samples[mode][k].append(api.profile_read(tag)[0])
            samples[mode]["wall_ms"].append(wall)
    api.profile_enable(False)
    median = {m: {k: statistics.median(v) for k, v in s.items()} for m, s in samples.items()}
    spread = {m: {k: max(v) - min(v) for k, v in s.items()} for m, s in samples.items()}

    def target(new, new_key, yard, yard_key):
        got, limit = median[new][new_key], median[yard][yard_key] + spread[yard][yard_key]
        return {"median_ms": got, "yardstick_median_ms": median[yard][yard_key], "yardstick_spread_ms": spread[yard][yard_key],
                "ratio": got / median[yard][yard_key], "met": bool(got <= limit)}

    checks = {"six_row_step_vs_allsky_step": target("aerosols", "wall_ms", "allsky", "wall_ms"),
              "profile_step_vs_allsky_profiles_step": target("aerosol_profiles", "wall_ms", "allsky_profiles", "wall_ms"),
              "six_row_lw_tag12_vs_tag8": target("aerosols", "lw_aerosol_ms", "allsky", "lw_allsky_ms"),
              "six_row_sw_tag13_vs_tag9": target("aerosols", "sw_aerosol_ms", "allsky", "sw_allsky_ms"),
              "profile_lw_tag12_vs_tag8": target("aerosol_profiles", "lw_aerosol_ms", "allsky_profiles", "lw_allsky_ms"),
              "profile_sw_tag13_vs_tag9": target("aerosol_profiles", "sw_aerosol_ms", "allsky_profiles", "sw_allsky_ms")}
    result = {"workload": f"G1: {ncol} columns, {V} levels, LW {wl.grid_lw.n} + SW {wl.grid_sw.n} points, fast 3; "
                          f"synthetic aerosol on {NA} points per band, synthetic clouds in about a third of the layers",
              "reps": args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples, "targets": checks,
              "step_over_run_step": {m: median[m]["wall_ms"] / median["run"]["wall_ms"] for m in modes}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(result, fo, indent=1)
    print(json.dumps({"targets": checks, "step_over_run_step": result["step_over_run_step"]}))
    for b in (out, levels, heating, prof_out):
        b.free()
    wl.destroy()


if __name__ == "__main__":
    main()
