"""Cost of the instrument channels of grt_pipeline_run_sky_channels over grt_pipeline_run_sky_radiances, on the G1 workload
(grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), all four sets, with the
synthetic aerosol of scripts/time_pipeline_aerosols.py and S draws of the synthetic cloud fields of
scripts/pipeline_timing.py per column and pass, at A viewing angles per column (secants 1 to 3, evenly spaced), all
without flux rows (fluxes_dev NULL: the longwave gas optics and the radiance kernel alone).

Alternating repetitions of these steps on one pipeline, in one process:
  radiances_alone   grt_pipeline_run_sky_radiances
  boxcar            grt_pipeline_run_sky_channels, 16 boxcar channels 50 cm-1 wide, side by side from the grid's start
  gaussian          grt_pipeline_run_sky_channels, Gaussian channels every 1 cm-1 with FWHM 2 cm-1 (cut off at 4 FWHM)
each channel step with brightness temperatures.  Per step: the kernel times by HIP-event profile tag (grt_ext.h: 25, the
radiance kernel, whose channel form forms the channels' sums; 26, the channels' finishing kernel; the longwave gas
optics) and the wall time of the whole step, synchronised; per instrument P (grt_channel_pair_count) and the scratch
bytes, max_columns x S x A x 2 x P doubles.  Reported, not gated.

The yardstick is the parent commit's build: run the script once with GRT_LIB_PATH naming that library -- it has no
channel entry point, so only radiances_alone is measured -- and give the result to the second run as --parent.
Result: profiles/pipeline_channels_timing.json (or the path given).

    GRT_LIB_PATH=<parent build> python scripts/time_pipeline_channels.py --out parent.json
    python scripts/time_pipeline_channels.py --parent parent.json [--reps 5] [--subcolumns 4] [--angles 8] [--out ...]
"""
import json

import numpy as np

from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api, channels
from time_pipeline_aerosols import synthetic_aerosols

TAG_RADIANCE, TAG_CHANNELS = 25, 26      # (grt_ext.h; an older library's module has no name for the second)
TAGS = {"radiance_ms": TAG_RADIANCE, "channels_ms": TAG_CHANNELS, "lw_gas_ms": api.TAG_GAS_LW, "lw_far_ms": api.TAG_FAR_LW}


def arguments(ap):
    ap.add_argument("--subcolumns", type=int, default=4)
    ap.add_argument("--angles", type=int, default=8)
    ap.add_argument("--parent", default=None, help="the result of a run under GRT_LIB_PATH = the parent commit's build")


def instruments(grid):
    """{name: (first, weights, centers)} on the longwave grid."""
    w0, dw, n = grid.w0, grid.dw, int(grid.n)
    lo = w0 + 50.0 * np.arange(16)
    w_end = w0 + (n - 1) * dw
    return {"boxcar": channels.boxcar(w0, dw, n, lo, lo + 50.0 - dw),
            "gaussian": channels.gaussian(w0, dw, n, np.arange(np.ceil(w0), w_end + 0.5, 1.0), 2.0)}


def main():
    s = Session("pipeline_channels_timing.json", arguments)
    pipe, gcols, lib, C, ncol, V, S, A = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.subcolumns, s.args.angles
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], S)[S]   # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    gsky, keep_sky = api.make_sky(gclouds, gaer, S, api.GRT_SKY_ALL)
    N = api.GRT_SKY_MAX_SETS
    rows = N * A * api.GRT_RADIANCE_ROWS_PER_ANGLE
    secants = np.ascontiguousarray(np.tile(np.linspace(1.0, 3.0, A), (ncol, 1)))
    grad = api.GrtRadiances(A, secants.ctypes.data_as(C.POINTER(C.c_double)), s.buffer(rows).ptr, None, None)
    has_channels = hasattr(lib, "grt_pipeline_run_sky_channels")
    inst, facts = {}, {}
    if has_channels:
        for name, (first, weights, centers) in instruments(s.wl.grid_lw).items():
            g, keep = api.make_channels(first, weights, centers)
            g.channel_radiances_dev = s.buffer(rows * g.num_channels).ptr
            g.channel_brightness_dev = s.buffer(rows * g.num_channels).ptr
            inst[name] = g
            P = api.channel_pair_count(g, int(s.wl.grid_lw.n))
            facts[name] = {"channels": int(g.num_channels), "weights": int(keep["counts"].sum()), "pairs_P": P,
                           "scratch_bytes": 8 * ncol * S * A * api.GRT_RADIANCE_ROWS_PER_ANGLE * P}

    def step(mode):
        if mode == "radiances_alone":
            api.check(lib.grt_pipeline_run_sky_radiances(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(grad), None))
        else:
            api.check(lib.grt_pipeline_run_sky_channels(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(grad),
                                                        C.byref(inst[mode]), None))

    modes = ["radiances_alone"] + list(inst)
    samples, median, spread = s.measure(modes, step, TAGS)
    result = {"workload": s.workload + f"; all four sets, synthetic aerosol on 16 points per band, {S} draws of synthetic "
                                       f"clouds in about a third of the layers, {A} viewing angles per column, no flux rows",
              "library": "this build" if has_channels else "a build without grt_pipeline_run_sky_channels (the yardstick)",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples, "instruments": facts,
              "wall_ms": {m: median[m]["wall_ms"] for m in modes},
              "radiance_kernel_ms": {m: median[m]["radiance_ms"] for m in modes},
              "channel_finish_ms": {m: median[m]["channels_ms"] for m in modes}}
    if s.args.parent is not None:
        with open(s.args.parent) as fi:
            parent = json.load(fi)
        result["parent"] = {k: parent[k] for k in ("library", "reps", "median", "spread_max_minus_min", "samples")}
        result["wall_ms"]["parent_radiances_alone"] = parent["wall_ms"]["radiances_alone"]
        result["radiance_kernel_ms"]["parent_radiances_alone"] = parent["radiance_kernel_ms"]["radiances_alone"]
    s.finish(result, ("wall_ms", "radiance_kernel_ms", "channel_finish_ms", "instruments"))


if __name__ == "__main__":
    main()
