"""Cost of grt_pipeline_run_subcolumns against grt_pipeline_run_allsky and grt_pipeline_run_allsky_profiles on the G1
workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), with S draws of the
synthetic cloud fields of scripts/time_pipeline_allsky.py per column and pass.

Five alternating repetitions of these steps on one pipeline:
  allsky            grt_pipeline_run_allsky on subcolumn 0 (the shortwave's one sweep where the user level allows it)
  allsky_profiles   grt_pipeline_run_allsky_profiles on subcolumn 0
  sub_S             grt_pipeline_run_subcolumns, six-row form, S = 1, 2, 4, 8
  subprof_S         grt_pipeline_run_subcolumns, profile form, S = 1, 2, 4, 8
Per step: the all-sky solver times by HIP-event profile tag (grt_ext.h: 8 / 9 longwave / shortwave, 11 the subcolumn
mean) and the wall time of the whole step, synchronised.  Result: profiles/pipeline_subcolumns_timing.json (or the path
given).

    python scripts/time_pipeline_subcolumns.py [--reps 5] [--out profiles/pipeline_subcolumns_timing.json]
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

TAGS = {"lw_allsky_solver_ms": 8, "sw_allsky_solver_ms": 9, "subcolumn_mean_ms": 11}
COUNTS = (1, 2, 4, 8)


def subcolumn_clouds(p, tl, S, seed=1):
    """time_pipeline_allsky.synthetic_clouds' fields with S draws per column and pass: optics sets [ncol][S][3][B][L]."""
    ncol, L = tl.shape
    rng = np.random.default_rng(seed)
    liquid_edges = np.array([10.0, 350.0, 700.0, 1200.0, 2000.0, 3500.0, 8000.0, 20000.0, 50000.0])
    ice_edges = np.array([10.0, 250.0, 500.0, 800.0, 1300.0, 2200.0, 4000.0, 9000.0, 18000.0, 30000.0, 52000.0])
    B = liquid_edges.size - 1
    thickness = 29.3 * tl * np.log(p[:, 1:] / p[:, :-1])
    sets = []
    for _ in range(2):
        cloudy = rng.random((ncol, S, L)) < 1.0 / 3.0
        low = np.arange(L)[None, None, :] >= L // 2
        liq, ice = np.zeros((ncol, S, 3, B, L)), np.zeros((ncol, S, 3, B, L))
        for phase, where, ext in ((liq, cloudy & low, 2e-2), (ice, cloudy & ~low, 2e-3)):
            w = np.broadcast_to(where[:, :, None, :], (ncol, S, B, L))
            phase[:, :, 0] = np.where(w, ext * rng.random((ncol, S, B, L)), 0.0)
            phase[:, :, 1] = np.where(w, 0.5 + 0.49 * rng.random((ncol, S, B, L)), 0.0)
            phase[:, :, 2] = np.where(w, 0.7 + 0.2 * rng.random((ncol, S, B, L)), 0.0)
        sets.append((liq, ice))
    bands = ((liquid_edges[:-1], liquid_edges[1:]), (ice_edges[:-1], ice_edges[1:]))
    return {S_: api.make_clouds(*bands, thickness, *(np.ascontiguousarray(x[:, :S_]) for x in
                                                     (sets[0][0], sets[0][1], sets[1][0], sets[1][1])))
            for S_ in range(1, S + 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pipeline_subcolumns_timing.json"))
    args = ap.parse_args()
    device = api.create_device(0)
    ncol = args.columns
    wl = W.G1Workload(device, ncol, fast=3)
    (gcols, keep), _ = wl.columns(0, ncol)
    pipe = wl.pipe
    V = wl.num_levels
    clouds = subcolumn_clouds(keep["p"], keep["tl"], max(COUNTS))
    out = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    levels = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN * V)
    heating = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_HEATING_ROWS_PER_COLUMN * (V - 1))
    prof_out = api.DeviceBuffer(device, 8 * ncol * api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    lib = api.load_library()
    C = api.C

    def step(mode):
        kind, _, s = mode.partition("_")
        if mode == "allsky":
            api.check(lib.grt_pipeline_run_allsky(pipe.p, C.byref(gcols), C.byref(clouds[1][0]), out.ptr))
        elif mode == "allsky_profiles":
            api.check(lib.grt_pipeline_run_allsky_profiles(pipe.p, C.byref(gcols), C.byref(clouds[1][0]), levels.ptr,
                                                           heating.ptr, prof_out.ptr))
        elif kind == "sub":
            api.check(lib.grt_pipeline_run_subcolumns(pipe.p, C.byref(gcols), C.byref(clouds[int(s)][0]), int(s), None,
                                                      None, out.ptr))
        else:
            api.check(lib.grt_pipeline_run_subcolumns(pipe.p, C.byref(gcols), C.byref(clouds[int(s)][0]), int(s),
                                                      levels.ptr, heating.ptr, prof_out.ptr))
        pipe.sync()

    api.profile_enable(True)
    modes = ["allsky", "allsky_profiles"] + [f"sub_{s}" for s in COUNTS] + [f"subprof_{s}" for s in COUNTS]
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
    solver = {m: median[m]["lw_allsky_solver_ms"] + median[m]["sw_allsky_solver_ms"] for m in modes}
    result = {"workload": f"G1: {ncol} columns, {V} levels, LW {wl.grid_lw.n} + SW {wl.grid_sw.n} points, fast 3; "
                          "synthetic clouds in about a third of the layers of each subcolumn",
              "reps": args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "samples": samples,
              "six_row_step_over_allsky_step": {s: median[f"sub_{s}"]["wall_ms"] / median["allsky"]["wall_ms"]
                                                for s in COUNTS},
              "profile_step_over_allsky_profiles_step": {
                  s: median[f"subprof_{s}"]["wall_ms"] / median["allsky_profiles"]["wall_ms"] for s in COUNTS},
              "allsky_solver_over_s1": {
                  "six_row": {s: solver[f"sub_{s}"] / solver["sub_1"] for s in COUNTS},
                  "profile": {s: solver[f"subprof_{s}"] / solver["subprof_1"] for s in COUNTS}},
              "subcolumn_mean_ms": {m: median[m]["subcolumn_mean_ms"] for m in modes if m.split("_")[-1] != "1"},
              "targets": {"six_row_step_s8_over_allsky": 1.35, "profile_step_s4_over_allsky_profiles": 1.35,
                          "allsky_solver_s8_over_s1": 8.5, "subcolumn_mean_ms": 1.0}}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fo:
        json.dump(result, fo, indent=1)
    print(json.dumps({k: result[k] for k in ("six_row_step_over_allsky_step", "profile_step_over_allsky_profiles_step",
                                             "allsky_solver_over_s1", "subcolumn_mean_ms")}))
    for b in (out, levels, heating, prof_out):
        b.free()
    wl.destroy()


if __name__ == "__main__":
    main()
