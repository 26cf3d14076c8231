"""Cost of grt_pipeline_run_profiles against the six-row forms on the G1 workload (grtcode_amd.workload: 64 columns,
61 levels, the bench's grids and line lists, fast = 3).

Five alternating repetitions of three steps on one pipeline:
  run        grt_pipeline_run (the shortwave's default one-sweep form)
  run_two    grt_pipeline_run with GRT_SW_TWO_SWEEPS=1 (the two-sweep form: the park block)
  profiles   grt_pipeline_run_profiles (every level's flux and the heating rates)
Per step: the longwave and shortwave solver times (HIP-event profile tags 3 and 4, grt_ext.h) and the wall time of the
whole step, synchronised.  Result: profiles/pipeline_profiles_timing.json (or the path given).

    python scripts/time_pipeline_profiles.py [--reps 5] [--out profiles/pipeline_profiles_timing.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from grtcode_amd import api, workload as W  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_profiles_timing.json"))
    args = ap.parse_args()
    device = api.create_device(0)
    ncol = args.columns
    wl = W.G1Workload(device, ncol, fast=3)
    (gcols, keep), _ = wl.columns(0, ncol)
    pipe = wl.pipe
    V = wl.num_levels
    levels = api.DeviceBuffer(device, 8 * ncol * api.GRT_PROFILE_ROWS_PER_COLUMN * V)
    heating = api.DeviceBuffer(device, 8 * ncol * api.GRT_HEATING_ROWS_PER_COLUMN * (V - 1))
    fluxes = api.DeviceBuffer(device, 8 * ncol * api.GRT_FLUXES_PER_COLUMN)
    lib = api.load_library()

    def step(mode):
        if mode == "run_two":
            os.environ["GRT_SW_TWO_SWEEPS"] = "1"
        else:
            os.environ.pop("GRT_SW_TWO_SWEEPS", None)
        if mode == "profiles":
            api.check(lib.grt_pipeline_run_profiles(pipe.p, api.C.byref(gcols), levels.ptr, heating.ptr, fluxes.ptr))
        else:
            pipe.run(gcols)
        pipe.sync()

    api.profile_enable(True)
    modes = ("run", "run_two", "profiles")
    for mode in modes:                       # warm-up: every buffer allocated, every kernel loaded
        step(mode)
    samples = {m: {"lw_solver_ms": [], "sw_solver_ms": [], "wall_ms": []} for m in modes}
    for rep in range(args.reps):
        for mode in modes:
            api.profile_read(1, reset=True)
            t0 = time.perf_counter()
            step(mode)
            wall = 1e3 * (time.perf_counter() - t0)
            samples[mode]["lw_solver_ms"].append(api.profile_read(3)[0])
            samples[mode]["sw_solver_ms"].append(api.profile_read(4)[0])
            samples[mode]["wall_ms"].append(wall)
    os.environ.pop("GRT_SW_TWO_SWEEPS", None)
    api.profile_enable(False)
    median = {m: {k: statistics.median(v) for k, v in s.items()} for m, s in samples.items()}
    ratio = {band: median["profiles"][f"{band}_solver_ms"] / median["run_two"][f"{band}_solver_ms"] for band in ("lw", "sw")}
    result = {"workload": f"G1: {ncol} columns, {V} levels, LW {wl.grid_lw.n} + SW {wl.grid_sw.n} points, fast 3",
              "reps": args.reps, "order": "run, run_two, profiles alternating; medians over the repetitions",
              "median": median, "samples": samples,
              "profile_over_two_sweep_solver": ratio,
              "profile_over_one_sweep_solver": {band: median["profiles"][f"{band}_solver_ms"] / median["run"][f"{band}_solver_ms"]
                                                for band in ("lw", "sw")}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({"median": median, "profile_over_two_sweep_solver": ratio}))
    for b in (levels, heating, fluxes):
        b.free()
    wl.destroy()


if __name__ == "__main__":
    main()
