"""Cost of grt_pipeline_run_sky_zeniths against grt_pipeline_run_sky on the G1 workload (grtcode_amd.workload: 64 columns,
61 levels, the bench's grids and line lists, fast = 3), six-row form, all four sets, S draws of the synthetic cloud fields
of scripts/pipeline_timing.py, the synthetic aerosol of scripts/time_pipeline_aerosols.py, every sample a day angle.

Five alternating repetitions of these steps on one pipeline, in one process:
  sky        grt_pipeline_run_sky: one sun angle per column
  zeniths    grt_pipeline_run_zeniths at Z = 8: the clean set alone (the existing path)
  rows_Z     grt_pipeline_run_sky_zeniths with Z = 1, 4, 8 angles per column: the zenith instances of the solver, one grid
             row per (column, draw, angle) -- the default for the sets with aerosol or clouds
  shared_Z   the same with GRT_ZENITH_SHARED=1: the shared-layer kernel's instances with the joins
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 1 / 2 and 6 / 7 gas optics; 4, 13, 9, 18 the shortwave
solvers of run_sky's four sets; 19 the clean set's zenith launches, 22 the other sets'; 20 and 23 the mean kernels) and
the wall time of the whole step, synchronised; medians, and spreads = max - min.

--yardstick-tree TREE: a built checkout of the parent commit.  Its `sky` and `zeniths` steps are taken first, in a process of
its own that loads TREE's library (GRT_LIB_PATH), and the result states
  (a) the run_sky_zeniths step at Z = 8 over 8 x the parent's run_sky step (expected far below 1);
  (b) tags 19 + 22 of the shared-layer form at Z = 8 against 8 x the parent's run_sky tags 4 + 13 + 9 + 18, the parent's
      spread as the margin: if it is not below, the row-mapped instances stay the default for the joined sets;
  (c) run_sky and run_zeniths at this commit against the parent's, within the parent's spread.
Result: profiles/pipeline_sky_zeniths_timing.json (or the path given).

    python scripts/time_pipeline_sky_zeniths.py [--reps 5] [--subcolumns 3] [--yardstick-tree TREE] [--out ...]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_aerosols import synthetic_aerosols

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW,
        "sw_clear_ms": api.TAG_SOLVER_SW, "sw_aerosol_ms": api.TAG_AEROSOL_SW, "sw_allsky_ms": api.TAG_ALLSKY_SW,
        "sw_sky_ms": api.TAG_SKY_SW, "zenith_sw_ms": api.TAG_ZENITH_SW, "zenith_mean_ms": api.TAG_ZENITH_MEAN}
NEW_TAGS = {"sky_zenith_sw_ms": getattr(api, "TAG_SKY_ZENITH_SW", 0), "sky_zenith_mean_ms": getattr(api, "TAG_SKY_ZENITH_MEAN", 0)}
SKY_SW = ("sw_clear_ms", "sw_aerosol_ms", "sw_allsky_ms", "sw_sky_ms")
COUNTS = (1, 4, 8)


def arguments(ap):
    ap.add_argument("--yardstick-tree", default=None)
    ap.add_argument("--subcolumns", type=int, default=3)
    ap.add_argument("--existing-only", action="store_true", help="time run_sky and run_zeniths alone (the yardstick's process)")


def yardstick(tree, reps, columns, subcolumns):
    """The parent's run_sky and run_zeniths steps: this script with --existing-only on the library of `tree`, in a child."""
    lib = os.path.join(os.path.abspath(tree), "grtcode_amd", "lib", "libgrtcode_hip.so")
    if not os.path.exists(lib):
        raise SystemExit(f"{lib} not found: build the yardstick tree first")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "yardstick.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--existing-only", "--reps", str(reps), "--columns",
                        str(columns), "--subcolumns", str(subcolumns), "--out", out], check=True,
                       env=dict(os.environ, GRT_LIB_PATH=lib), stdout=subprocess.DEVNULL)
        with open(out) as f:
            got = json.load(f)
    med, spr = got["median"], got["spread_max_minus_min"]
    return {"library": lib, "sky_wall_ms": med["sky"]["wall_ms"], "sky_wall_spread_ms": spr["sky"]["wall_ms"],
            "zeniths_wall_ms": med["zeniths"]["wall_ms"], "zeniths_wall_spread_ms": spr["zeniths"]["wall_ms"],
            "sky_sw_solvers_ms": sum(med["sky"][k] for k in SKY_SW),
            "sky_sw_solvers_spread_ms": sum(spr["sky"][k] for k in SKY_SW), "samples": got["samples"]}


def main():
    # (the yardstick first, before this process opens the device: one process on the GPU at a time)
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--yardstick-tree", default=None)
    pre.add_argument("--reps", type=int, default=5)
    pre.add_argument("--columns", type=int, default=64)
    pre.add_argument("--subcolumns", type=int, default=3)
    known, _ = pre.parse_known_args()
    parent = yardstick(known.yardstick_tree, known.reps, known.columns, known.subcolumns) if known.yardstick_tree else None
    s = Session("pipeline_sky_zeniths_timing.json", arguments)
    pipe, gcols, lib, C, ncol, V, S = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.subcolumns
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], S)[S]   # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    gsky, keep_sky = api.make_sky(gclouds, gaer, S, api.GRT_SKY_ALL)
    out = s.buffer(api.GRT_SKY_MAX_SETS * api.GRT_FLUXES_PER_COLUMN)
    zen = {n: api.make_zeniths(np.array([np.roll(np.linspace(0.15, 1.0, n), c) for c in range(ncol)])) for n in COUNTS}
    tags = dict(TAGS)
    modes = ["sky", "zeniths"]
    if not s.args.existing_only:
        tags.update(NEW_TAGS)
        modes += [f"rows_{n}" for n in COUNTS] + [f"shared_{n}" for n in COUNTS]

    def step(mode):
        kind, _, n = mode.partition("_")
        if mode == "sky":
            api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(gsky), None, None, out.ptr))
        elif mode == "zeniths":
            api.check(lib.grt_pipeline_run_zeniths(pipe.p, C.byref(gcols), C.byref(zen[8][0]), None, None, out.ptr))
        else:
            if kind == "shared":
                os.environ["GRT_ZENITH_SHARED"] = "1"
            api.check(lib.grt_pipeline_run_sky_zeniths(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(zen[int(n)][0]), None,
                                                       None, out.ptr))
            os.environ.pop("GRT_ZENITH_SHARED", None)

    samples, median, spread = s.measure(modes, step, tags)
    result = {"workload": s.workload + f"; four sets, synthetic aerosol on 16 points per band, {S} draws of synthetic clouds; "
                                       "every sample a day angle, 0.15 to 1 in another order per column",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "wall_ms": {m: median[m]["wall_ms"] for m in modes}}
    show = ["wall_ms"]
    if not s.args.existing_only:
        solver = {m: median[m]["zenith_sw_ms"] + median[m]["sky_zenith_sw_ms"] for m in modes if "_" in m}
        result["zenith_solvers_ms"] = solver
        result["step_over_z_sky_steps"] = {m: median[m]["wall_ms"] / (int(m.split("_")[1]) * median["sky"]["wall_ms"])
                                           for m in solver}
        result["shared_over_rows_solvers"] = {n: solver[f"shared_{n}"] / solver[f"rows_{n}"] for n in COUNTS}
        show += ["zenith_solvers_ms", "step_over_z_sky_steps", "shared_over_rows_solvers"]
    if parent is not None:
        a = median["rows_8"]["wall_ms"] / (8.0 * parent["sky_wall_ms"])
        bound = 8.0 * parent["sky_sw_solvers_ms"] - parent["sky_sw_solvers_spread_ms"]
        result["yardstick"] = parent
        result["a_whole_step_z8_over_8_parent_sky_steps"] = a
        result["b_shared_tags_19_22_z8_ms"] = result["zenith_solvers_ms"]["shared_8"]
        result["b_rows_tags_19_22_z8_ms"] = result["zenith_solvers_ms"]["rows_8"]
        result["b_bound_8_parent_sky_solvers_minus_spread_ms"] = bound
        result["b_shared_below_bound"] = bool(result["zenith_solvers_ms"]["shared_8"] < bound)
        for name in ("sky", "zeniths"):
            result[f"c_{name}_ms"] = median[name]["wall_ms"]
            result[f"c_parent_{name}_ms"] = parent[f"{name}_wall_ms"]
            result[f"c_{name}_within_parent_spread"] = bool(abs(median[name]["wall_ms"] - parent[f"{name}_wall_ms"])
                                                            <= parent[f"{name}_wall_spread_ms"])
        show += [k for k in result if k[:2] in ("a_", "b_", "c_")]
    s.finish(result, show)


if __name__ == "__main__":
    main()
