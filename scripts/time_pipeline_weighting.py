"""Cost of the channel transmittance profiles and contribution functions of grt_pipeline_run_sky_weighting over
grt_pipeline_run_sky_channels, on the G1 workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line
lists, fast = 3), all four sets, with the synthetic aerosol of scripts/time_pipeline_aerosols.py and S draws of the
synthetic cloud fields of scripts/pipeline_timing.py per column and pass, at ONE viewing angle per column (a sounder sees a
column at one angle; the outputs grow with A x C x V), without flux rows (fluxes_dev NULL), for the two instruments of
scripts/time_pipeline_channels.py: 16 boxcars 50 cm-1 wide and Gaussian channels every 1 cm-1 with FWHM 2 cm-1.

Alternating repetitions of these steps on one pipeline, in one process, per instrument:
  radiances_alone           grt_pipeline_run_sky_radiances (what tag 25 costs without channels)
  <instrument>.channels_alone   grt_pipeline_run_sky_channels
  <instrument>.weighting        grt_pipeline_run_sky_weighting, both outputs
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 25, the radiance kernel and its channel form; 26, the
channels' finishing kernel; 27, the weighting kernel; 28, its finishing kernel) and the wall time of the whole step,
synchronised; per instrument P (grt_channel_pair_count) and the scratch bytes, max_columns x S x A x (2 V + 1) x P doubles.
Beside tag 27 stands what the channel form's per-row wave sums would have cost for 2 V + 1 rows, extrapolated from the same
run: (tag 25 with channels - tag 25 without) x (2 V + 1) / 2.  Reported, not gated.

The yardstick for channels_alone is the parent commit's build: run the script once with GRT_LIB_PATH naming that library
-- it has no weighting entry point, so only radiances_alone and channels_alone are measured -- and give the result to the
second run as --parent.  Result: profiles/pipeline_weighting_timing.json (or the path given).

    GRT_LIB_PATH=<parent build> python scripts/time_pipeline_weighting.py --out parent.json
    python scripts/time_pipeline_weighting.py --parent parent.json [--reps 5] [--subcolumns 4] [--out ...]
"""
import json

import numpy as np

from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_aerosols import synthetic_aerosols
from time_pipeline_channels import instruments

# (grt_ext.h; an older library's module has no name for the last two)
TAGS = {"radiance_ms": 25, "channels_ms": 26, "weighting_ms": 27, "weighting_finish_ms": 28, "lw_gas_ms": api.TAG_GAS_LW}


def arguments(ap):
    ap.add_argument("--subcolumns", type=int, default=4)
    ap.add_argument("--parent", default=None, help="the result of a run under GRT_LIB_PATH = the parent commit's build")


def main():
    s = Session("pipeline_weighting_timing.json", arguments)
    pipe, gcols, lib, C, ncol, V, S, A = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.subcolumns, 1
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], S)[S]   # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    gsky, keep_sky = api.make_sky(gclouds, gaer, S, api.GRT_SKY_ALL)
    N = api.GRT_SKY_MAX_SETS
    rows = N * A * api.GRT_RADIANCE_ROWS_PER_ANGLE
    secants = np.ascontiguousarray(np.full((ncol, A), 1.25))
    grad = api.GrtRadiances(A, secants.ctypes.data_as(C.POINTER(C.c_double)), s.buffer(rows).ptr, None, None)
    has_weighting = hasattr(lib, "grt_pipeline_run_sky_weighting")
    inst, weight, facts = {}, {}, {}
    for name, (first, weights, centers) in instruments(s.wl.grid_lw).items():
        g, keep = api.make_channels(first, weights, centers)
        g.channel_radiances_dev = s.buffer(rows * g.num_channels).ptr
        g.channel_brightness_dev = s.buffer(rows * g.num_channels).ptr
        inst[name] = g
        P = api.channel_pair_count(g, int(s.wl.grid_lw.n))
        facts[name] = {"channels": int(g.num_channels), "weights": int(keep["counts"].sum()), "pairs_P": P,
                       "scratch_bytes": 8 * ncol * S * A * (2 * V + 1) * P}
        if has_weighting:
            weight[name] = api.GrtWeighting(s.buffer(N * A * V * g.num_channels).ptr,
                                            s.buffer(N * A * (V + 1) * g.num_channels).ptr)

    def step(mode):
        if mode == "radiances_alone":
            api.check(lib.grt_pipeline_run_sky_radiances(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(grad), None))
            return
        name, what = mode.split(".")
        if what == "channels_alone":
            api.check(lib.grt_pipeline_run_sky_channels(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(grad),
                                                        C.byref(inst[name]), None))
        else:
            api.check(lib.grt_pipeline_run_sky_weighting(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(grad),
                                                         C.byref(inst[name]), C.byref(weight[name]), None))

    modes = ["radiances_alone"]
    for name in inst:
        modes += [name + ".channels_alone"] + ([name + ".weighting"] if has_weighting else [])
    samples, median, spread = s.measure(modes, step, TAGS)
    result = {"workload": s.workload + f"; all four sets, synthetic aerosol on 16 points per band, {S} draws of synthetic "
                                       f"clouds in about a third of the layers, one viewing angle per column, no flux rows",
              "library": "this build" if has_weighting else "a build without grt_pipeline_run_sky_weighting (the yardstick)",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples, "instruments": facts,
              "wall_ms": {m: median[m]["wall_ms"] for m in modes},
              "kernel_ms": {m: {k: median[m][k] for k in ("radiance_ms", "channels_ms", "weighting_ms", "weighting_finish_ms")}
                            for m in modes}}
    if has_weighting:
        # what the channel form's per-(channel, row) wave sums would have cost for 2 V + 1 rows instead of 2
        base = median["radiances_alone"]["radiance_ms"]
        result["wave_sum_extrapolation_ms"] = {
            name: (median[name + ".channels_alone"]["radiance_ms"] - base) * (2 * V + 1) / 2.0 for name in inst}
        result["weighting_kernel_ms"] = {name: median[name + ".weighting"]["weighting_ms"] for name in inst}
    if s.args.parent is not None:
        with open(s.args.parent) as fi:
            parent = json.load(fi)
        result["parent"] = {k: parent[k] for k in ("library", "reps", "median", "spread_max_minus_min", "samples")}
        for m in parent["wall_ms"]:
            result["wall_ms"]["parent_" + m] = parent["wall_ms"][m]
    s.finish(result, ("wall_ms", "kernel_ms", "instruments"))


if __name__ == "__main__":
    main()
