"""Cost of grt_pipeline_run_zeniths against grt_pipeline_run on the G1 workload (grtcode_amd.workload: 64 columns, 61
levels, the bench's grids and line lists, fast = 3), six-row form, every sample a day angle.

Five alternating repetitions of these steps on one pipeline, in one process:
  run        grt_pipeline_run: one sun angle per column
  zen_Z      grt_pipeline_run_zeniths with Z = 1, 4, 8 angles per column: the shared-layer kernel (the default)
  rows_Z     the same with GRT_ZENITH_SHARED=0: the zenith instance of the six-row solver, one grid row per angle
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 1 / 2 and 6 / 7 gas optics, 3 / 4 the clear-clean solvers,
19 the zenith solver launches, 20 the mean kernel) and the wall time of the whole step, synchronised; medians, and
spreads = max - min.

--yardstick-tree TREE: a built checkout of the parent commit.  Its `run` step and its tag-4 solver time are taken first, in
a process of its own that loads TREE's library (GRT_LIB_PATH), and the result states
  (a) the run_zeniths step at Z = 8 over 8 x the parent's run step (required: below 1);
  (b) the zenith solver's tag time at Z = 8 against 8 x the parent's tag-4 time, the parent's spread as the margin;
  (c) run at this commit against the parent's, within the parent's spread.
Result: profiles/pipeline_zeniths_timing.json (or the path given).

    python scripts/time_pipeline_zeniths.py [--reps 5] [--yardstick-tree TREE] [--out profiles/pipeline_zeniths_timing.json]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

from pipeline_timing import Session  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW,
        "lw_solver_ms": api.TAG_SOLVER_LW, "sw_solver_ms": api.TAG_SOLVER_SW}
ZENITH_TAGS = {"zenith_sw_ms": getattr(api, "TAG_ZENITH_SW", 0), "zenith_mean_ms": getattr(api, "TAG_ZENITH_MEAN", 0)}
COUNTS = (1, 4, 8)


def arguments(ap):
    ap.add_argument("--yardstick-tree", default=None)
    ap.add_argument("--run-only", action="store_true", help="time grt_pipeline_run alone (the yardstick's process)")


def yardstick(tree, reps, columns):
    """The parent's run step and tag-4 time: this script with --run-only on the library of `tree`, in a child process."""
    lib = os.path.join(os.path.abspath(tree), "grtcode_amd", "lib", "libgrtcode_hip.so")
    if not os.path.exists(lib):
        raise SystemExit(f"{lib} not found: build the yardstick tree first")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "yardstick.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--run-only", "--reps", str(reps), "--columns",
                        str(columns), "--out", out], check=True, env=dict(os.environ, GRT_LIB_PATH=lib),
                       stdout=subprocess.DEVNULL)
        with open(out) as f:
            got = json.load(f)
    return {"library": lib, "run_wall_ms": got["median"]["run"]["wall_ms"],
            "run_wall_spread_ms": got["spread_max_minus_min"]["run"]["wall_ms"],
            "sw_solver_ms": got["median"]["run"]["sw_solver_ms"],
            "sw_solver_spread_ms": got["spread_max_minus_min"]["run"]["sw_solver_ms"], "samples": got["samples"]["run"]}


def main():
    # (the yardstick first, before this process opens the device: one process on the GPU at a time)
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument("--yardstick-tree", default=None)
    pre.add_argument("--reps", type=int, default=5)
    pre.add_argument("--columns", type=int, default=64)
    known, _ = pre.parse_known_args()
    parent = yardstick(known.yardstick_tree, known.reps, known.columns) if known.yardstick_tree else None
    s = Session("pipeline_zeniths_timing.json", arguments)
    pipe, gcols, lib, C, ncol = s.pipe, s.gcols, s.lib, api.C, s.ncol
    out = s.buffer(api.GRT_FLUXES_PER_COLUMN)
    tags = dict(TAGS)
    modes = ["run"]
    zen = {}
    if not s.args.run_only:
        tags.update(ZENITH_TAGS)
        modes += [f"zen_{n}" for n in COUNTS] + [f"rows_{n}" for n in COUNTS]
        for n in COUNTS:
            mu = np.array([np.roll(np.linspace(0.15, 1.0, n), c) for c in range(ncol)])
            zen[n] = api.make_zeniths(mu)

    def step(mode):
        kind, _, n = mode.partition("_")
        if mode == "run":
            api.check(lib.grt_pipeline_run(pipe.p, C.byref(gcols), out.ptr))
            return
        os.environ["GRT_ZENITH_SHARED"] = "0" if kind == "rows" else "1"
        api.check(lib.grt_pipeline_run_zeniths(pipe.p, C.byref(gcols), C.byref(zen[int(n)][0]), None, None, out.ptr))
        del os.environ["GRT_ZENITH_SHARED"]

    samples, median, spread = s.measure(modes, step, tags)
    result = {"workload": s.workload + "; every sample a day angle, 0.15 to 1 in another order per column",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "wall_ms": {m: median[m]["wall_ms"] for m in modes}}
    show = ["wall_ms"]
    if not s.args.run_only:
        result["zenith_chunk"] = api.GRT_ZENITH_CHUNK
        result["zenith_sw_ms"] = {m: median[m]["zenith_sw_ms"] for m in modes if m != "run"}
        result["step_over_z_run_steps"] = {m: median[m]["wall_ms"] / (int(m.split("_")[1]) * median["run"]["wall_ms"])
                                           for m in modes if m != "run"}
        result["shared_over_rows_solver"] = {n: median[f"zen_{n}"]["zenith_sw_ms"] / median[f"rows_{n}"]["zenith_sw_ms"]
                                             for n in COUNTS}
        show += ["zenith_sw_ms", "step_over_z_run_steps", "shared_over_rows_solver"]
    if parent is not None:
        a = median["zen_8"]["wall_ms"] / (8.0 * parent["run_wall_ms"])
        bound = 8.0 * parent["sw_solver_ms"] - parent["sw_solver_spread_ms"]
        result["yardstick"] = parent
        result["a_whole_step_z8_over_8_parent_run_steps"] = a
        result["a_lower"] = bool(a < 1.0)
        result["b_shared_kernel_z8_ms"] = median["zen_8"]["zenith_sw_ms"]
        result["b_bound_8_parent_tag4_minus_spread_ms"] = bound
        result["b_below_bound"] = bool(median["zen_8"]["zenith_sw_ms"] < bound)
        result["c_run_ms"] = median["run"]["wall_ms"]
        result["c_parent_run_ms"] = parent["run_wall_ms"]
        result["c_within_parent_spread"] = bool(abs(median["run"]["wall_ms"] - parent["run_wall_ms"])
                                                <= parent["run_wall_spread_ms"])
        show += ["a_whole_step_z8_over_8_parent_run_steps", "a_lower", "b_shared_kernel_z8_ms",
                 "b_bound_8_parent_tag4_minus_spread_ms", "b_below_bound", "c_run_ms", "c_parent_run_ms",
                 "c_within_parent_spread"]
    s.finish(result, show)


if __name__ == "__main__":
    main()
