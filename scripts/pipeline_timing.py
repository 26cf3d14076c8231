"""The session the scripts/time_pipeline_*.py share: the G1 workload (grtcode_amd.workload: 64 columns, 61 levels, the
bench's grids and line lists, fast = 3) on one pipeline, device buffers for a script's own calls of the C entry points,
alternating repetitions of its steps with the solver times by HIP-event profile tag (grt_ext.h) and the synchronised
wall time of each, the JSON result; and the synthetic cloud fields the all-sky steps run on."""
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


def cloud_fields(p, tl, S, seed=1):
    """Cloud in about a third of the layers of each subcolumn, liquid in the lower ones, ice in the upper ones, band optics
    on 8 liquid and 10 ice bands across both grids, S draws per column and pass.  -> (liquid, ice) band limits, layer
    thickness [ncol][L] m, and the longwave liquid, longwave ice, shortwave liquid and shortwave ice optics, each
    [ncol][S][3][B][L]: make_clouds' arguments."""
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
        sets += [liq, ice]
    return ((liquid_edges[:-1], liquid_edges[1:]), (ice_edges[:-1], ice_edges[1:])), thickness, sets


def synthetic_clouds(p, tl, seed=1):
    """make_clouds of one draw per column and pass: optics sets [ncol][3][B][L]."""
    bands, thickness, sets = cloud_fields(p, tl, 1, seed)
    return api.make_clouds(*bands, thickness, *(x[:, 0] for x in sets))


def subcolumn_clouds(p, tl, S, seed=1):
    """{S': make_clouds of the first S' of S draws per column and pass, optics sets [ncol][S'][3][B][L]} for S' = 1 .. S."""
    bands, thickness, sets = cloud_fields(p, tl, S, seed)
    return {n: api.make_clouds(*bands, thickness, *(np.ascontiguousarray(x[:, :n]) for x in sets)) for n in range(1, S + 1)}


class Session:
    def __init__(self, out_name, add_arguments=None):
        """Parses --reps, --columns, --out (default profiles/<out_name>) and what add_arguments(parser) adds; opens the
        G1 workload and its first `columns` columns."""
        ap = argparse.ArgumentParser()
        ap.add_argument("--reps", type=int, default=5)
        ap.add_argument("--columns", type=int, default=64)
        ap.add_argument("--out", default=os.path.join(ROOT, "profiles", out_name))
        if add_arguments is not None:
            add_arguments(ap)
        self.args = ap.parse_args()
        self.device = api.create_device(0)
        self.ncol = self.args.columns
        self.wl = W.G1Workload(self.device, self.ncol, fast=3)
        (self.gcols, self.keep), _ = self.wl.columns(0, self.ncol)
        self.pipe, self.V, self.lib = self.wl.pipe, self.wl.num_levels, api.load_library()
        self.workload = (f"G1: {self.ncol} columns, {self.V} levels, LW {self.wl.grid_lw.n} + SW {self.wl.grid_sw.n} points, "
                         "fast 3")
        self.buffers = []

    def buffer(self, per_column):
        """A device buffer of per_column doubles for each column, freed by finish()."""
        self.buffers.append(api.DeviceBuffer(self.device, 8 * self.ncol * per_column))
        return self.buffers[-1]

    def profile_outputs(self, sets):
        """levels, heating, fluxes of a profile entry point with `sets` sets per column (1 or 2)."""
        return (self.buffer(sets * api.GRT_PROFILE_ROWS_PER_COLUMN * self.V),
                self.buffer(sets * api.GRT_HEATING_ROWS_PER_COLUMN * (self.V - 1)),
                self.buffer(sets * api.GRT_FLUXES_PER_COLUMN))

    def measure(self, modes, step, tags):
        """step(mode) once for every mode (warm-up: every buffer allocated, every kernel loaded), then --reps times over
        the modes in turn, each followed by the pipeline's sync.  -> samples {mode: {tag name: [ms], "wall_ms": [ms]}},
        their medians and their spreads (max - min)."""
        api.profile_enable(True)
        for mode in modes:
            step(mode)
            self.pipe.sync()
        samples = {m: {**{k: [] for k in tags}, "wall_ms": []} for m in modes}
        for rep in range(self.args.reps):
            for mode in modes:
                api.profile_read(api.TAG_GAS_LW, reset=True)         # (a reset clears the brackets of every tag)
                t0 = time.perf_counter()
                step(mode)
                self.pipe.sync()
                wall = 1e3 * (time.perf_counter() - t0)
                for k, tag in tags.items():
                    samples[mode][k].append(api.profile_read(tag)[0])
                samples[mode]["wall_ms"].append(wall)
        api.profile_enable(False)
        median = {m: {k: statistics.median(v) for k, v in s.items()} for m, s in samples.items()}
        spread = {m: {k: max(v) - min(v) for k, v in s.items()} for m, s in samples.items()}
        return samples, median, spread

    def finish(self, result, show):
        """Writes result to --out, prints its keys `show` as one JSON line, frees the buffers and the workload."""
        out = os.path.abspath(self.args.out)
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as fo:
            json.dump(result, fo, indent=1)
        print(json.dumps({k: result[k] for k in show}))
        for b in self.buffers:
            b.free()
        self.wl.destroy()
