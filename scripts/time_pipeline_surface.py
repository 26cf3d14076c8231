"""Cost of a per-column surface (grt_pipeline_set_surface) on the G1 workload (grtcode_amd.workload: 64 columns, 61 levels,
the bench's grids and line lists, fast = 3).

Yardstick: a grt_pipeline_run step and a grt_pipeline_run_profiles step of the PARENT commit, measured by this script in a
process of its own on a built checkout of that commit, --yardstick-tree PATH (its package, its library and its
scripts/pipeline_timing.py; it knows nothing of a surface, so that process runs the two plain steps only).  Without
--yardstick-tree the plain steps of this commit stand in for it, and the result says so.

Five alternating repetitions in one process of
  run, run_profiles                       (a) no surface set
  run_surface, run_profiles_surface       (b) a surface set beforehand, outside the timed region: emissivity, direct and
                                              diffuse albedo on NS = 16 points, every column its own
each synchronised; medians and spreads (max - min).  Required of (b): no slower than the yardstick's median plus the
yardstick's spread in the same run; (a) is expected equal to the yardstick within the spreads.
(c) one grt_pipeline_set_surface call for NS = 2 and NS = 16: host wall time until the call returns, wall time until the
lane has drained, and the kernel time under api.TAG_SURFACE (three launches); next to it the upload it replaces, [ncol][n_lw]
+ 2 [ncol][n_sw] doubles through grt_host_to_device, timed once.
Result: profiles/pipeline_surface_timing.json (or the path given).

    python scripts/time_pipeline_surface.py [--reps 5] [--yardstick-tree PATH] [--out profiles/pipeline_surface_timing.json]
"""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

from pipeline_timing import Session  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

PLAIN = ["run", "run_profiles"]


def add_arguments(ap):
    ap.add_argument("--yardstick-tree", default=None, help="a built checkout of the parent commit")
    ap.add_argument("--plain-only", action="store_true", help="the two plain steps only (what the yardstick process runs)")


def synthetic_surface(grid, ncol, ns, seed):
    """ns knots across the band (points below, inside and above the surface grid) and every column's own values"""
    rng = np.random.default_rng(seed)
    x = np.linspace(grid.w0 + 0.1 * (grid.wn - grid.w0), grid.w0 + 0.8 * (grid.wn - grid.w0), ns)
    return x, rng.uniform(0.0, 1.0, (ncol, ns))


def make(s, ns):
    xe, e = synthetic_surface(s.wl.grid_lw, s.ncol, ns, 5)
    xa, a = synthetic_surface(s.wl.grid_sw, s.ncol, ns, 6)
    _, d = synthetic_surface(s.wl.grid_sw, s.ncol, ns, 7)
    return api.make_surface(s.ncol, emissivity=(xe, e), albedo=(xa, a, d))


def main():
    s = Session("pipeline_surface_timing.json", add_arguments)
    pipe, gcols, lib, C = s.pipe, s.gcols, s.lib, api.C
    out = s.buffer(api.GRT_FLUXES_PER_COLUMN)
    levels, heating, prof_out = s.profile_outputs(1)
    modes = PLAIN if s.args.plain_only else PLAIN + ["run_surface", "run_profiles_surface"]
    surfaces = {} if s.args.plain_only else {ns: make(s, ns) for ns in (2, 16)}

    def prepare(mode):
        """the surface of the step, set (or cleared) and on the device before the step's clock starts"""
        if not s.args.plain_only:
            pipe.set_surface(surfaces[16][0] if mode.endswith("_surface") else None)
            pipe.sync()

    def step(mode):
        if mode.startswith("run_profiles"):
            api.check(lib.grt_pipeline_run_profiles(pipe.p, C.byref(gcols), levels.ptr, heating.ptr, prof_out.ptr))
        else:
            api.check(lib.grt_pipeline_run(pipe.p, C.byref(gcols), out.ptr))

    for mode in modes:                                  # warm-up: every buffer allocated, every kernel loaded
        prepare(mode)
        step(mode)
        pipe.sync()
    samples = {m: [] for m in modes}
    for rep in range(s.args.reps):
        for mode in modes:
            prepare(mode)
            t0 = time.perf_counter()
            step(mode)
            pipe.sync()
            samples[mode].append(1e3 * (time.perf_counter() - t0))
    median = {m: statistics.median(v) for m, v in samples.items()}
    spread = {m: max(v) - min(v) for m, v in samples.items()}
    result = {"workload": s.workload, "reps": s.args.reps,
              "order": ", ".join(modes) + " alternating; medians over the repetitions; wall ms of a synchronised step",
              "median_ms": median, "spread_max_minus_min_ms": spread, "samples_ms": samples}
    if s.args.plain_only:
        s.finish(result, ("median_ms", "spread_max_minus_min_ms"))
        return

    # the yardstick: the parent's library in a process of its own
    yard = {"source": "this commit's plain steps (no --yardstick-tree given)", "median_ms": {m: median[m] for m in PLAIN},
            "spread_max_minus_min_ms": {m: spread[m] for m in PLAIN}}
    if s.args.yardstick_tree:
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "yardstick.json")
            # this file, run with the other tree's scripts/ first on the path: its pipeline_timing, package and library
            argv = [__file__, "--plain-only", "--reps", str(s.args.reps), "--columns", str(s.ncol), "--out", path]
            boot = ("import runpy, sys; sys.path.insert(0, sys.argv[1]); sys.argv = sys.argv[2:]; "
                    "runpy.run_path(sys.argv[0], run_name='__main__')")
            subprocess.run([sys.executable, "-c", boot, os.path.join(os.path.abspath(s.args.yardstick_tree), "scripts")] + argv,
                           check=True, timeout=900)
            y = json.load(open(path))
        yard = {"source": "a checkout of the parent commit, same steps, a process of its own", "median_ms": y["median_ms"],
                "spread_max_minus_min_ms": y["spread_max_minus_min_ms"], "samples_ms": y["samples_ms"]}
    result["yardstick"] = yard

    def target(mode, plain):
        limit = yard["median_ms"][plain] + yard["spread_max_minus_min_ms"][plain]
        return {"median_ms": median[mode], "yardstick_median_ms": yard["median_ms"][plain],
                "yardstick_spread_ms": yard["spread_max_minus_min_ms"][plain], "ratio": median[mode] / yard["median_ms"][plain],
                "met": bool(median[mode] <= limit)}

    result["targets"] = {"a_run_no_surface": target("run", "run"), "a_run_profiles_no_surface": target("run_profiles", "run_profiles"),
                         "b_run_with_surface": target("run_surface", "run"),
                         "b_run_profiles_with_surface": target("run_profiles_surface", "run_profiles")}

    # (c) the setter itself
    setter = {}
    api.profile_enable(True)
    for ns, (gs, keep) in surfaces.items():
        host, drained, kernel = [], [], []
        for rep in range(s.args.reps + 1):              # (the first call of a grid builds its per-point entries: left out)
            pipe.sync()
            api.profile_read(api.TAG_GAS_LW, reset=True)
            t0 = time.perf_counter()
            pipe.set_surface(gs)
            t1 = time.perf_counter()
            pipe.sync()
            t2 = time.perf_counter()
            ms, launches = api.profile_read(api.TAG_SURFACE)
            assert launches == 3, launches
            if rep > 0:
                host.append(1e3 * (t1 - t0))
                drained.append(1e3 * (t2 - t0))
                kernel.append(ms)
        setter[f"NS={ns}"] = {"host_call_ms": statistics.median(host), "call_and_drain_ms": statistics.median(drained),
                              "kernel_tag15_ms": statistics.median(kernel), "launches": 3,
                              "staged_bytes": 8 * 3 * s.ncol * (ns + 1) * 2}
    api.profile_enable(False)
    pipe.set_surface(None)
    rows = np.zeros(s.ncol * (s.wl.grid_lw.n + 2 * s.wl.grid_sw.n))
    buf = api.DeviceBuffer(s.device, rows.nbytes)
    pipe.sync()
    t0 = time.perf_counter()
    api.check(lib.grt_host_to_device(s.device, buf.ptr, rows.ctypes.data_as(C.c_void_p), C.c_size_t(rows.nbytes)))
    setter["upload_it_replaces"] = {"bytes": int(rows.nbytes), "grt_host_to_device_ms": 1e3 * (time.perf_counter() - t0)}
    buf.free()
    result["set_surface"] = setter
    s.finish(result, ("targets", "set_surface"))


if __name__ == "__main__":
    main()
