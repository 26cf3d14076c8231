"""Cost of the correlated k-distribution of grt_pipeline_run_kdist_correlated -- the class-map kernel and the mapped
reduction -- beside grt_pipeline_run_kdist's own kernel for the same request, on the G1 workload (grtcode_amd.workload: 64
columns, 61 levels, the bench's grids and line lists, fast = 3).

Alternating repetitions of these steps on one pipeline, in one process:
  kdist            grt_pipeline_run_kdist, --bins contiguous bins of equal width per band, --classes classes log-spaced
                   over twelve decades, no weight (the yardstick: every layer bisects its own optical depths)
  correlated       grt_pipeline_run_kdist_correlated for the same request, the key the column's vertical optical depth
                   (GRT_KDIST_KEY_SUM), the maps in pipeline scratch
  correlated_row   the same with the lowest layer as the key (GRT_KDIST_KEY_ROW)
  kdist_1024, correlated_1024   both with 1024 classes (a thread owns four)
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 29, grt_pipeline_run_kdist's kernel; 30, the class map;
31, the mapped reduction -- each both bands' launches together; 1 / 2 and 6 / 7, the gas optics) and the wall time of the
whole step, synchronised.  Reported, not gated.  Result: profiles/pipeline_kdist_correlated_timing.json (or the path given).

    python scripts/time_pipeline_kdist_correlated.py [--reps 5] [--bins 16] [--classes 64] [--out ...]
"""
import numpy as np

from pipeline_timing import Session  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_band_profiles import equal_bins

TAGS = {"kdist_ms": api.TAG_KDIST, "map_ms": api.TAG_KDIST_MAP, "mapped_ms": api.TAG_KDIST_MAPPED,
        "lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW}


def arguments(ap):
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--classes", type=int, default=64)


def main():
    s = Session("pipeline_kdist_correlated_timing.json", arguments)
    pipe, gcols, wl = s.pipe, s.gcols, s.wl
    el, es = equal_bins(wl.grid_lw.n, s.args.bins), equal_bins(wl.grid_sw.n, s.args.bins)
    L = s.V - 1
    few, many = np.logspace(-10.0, 2.0, s.args.classes - 1), np.logspace(-10.0, 2.0, 1023)
    modes = {"kdist": (few, None), "correlated": (few, (api.KDIST_KEY_SUM, 0)),
             "correlated_row": (few, (api.KDIST_KEY_ROW, L - 1)), "kdist_1024": (many, None),
             "correlated_1024": (many, (api.KDIST_KEY_SUM, 0))}
    calls = {}
    for mode, (ce, key) in modes.items():
        gk, keep = api.make_kdist(ce, el, es)
        for band in (gk.lw, gk.sw):
            # (per column: the correlated form's counts and weight sums have no layer axis)
            shared = band.num_bins * gk.num_classes * (L if key is None else 1)
            band.points_dev, band.weight_dev = s.buffer(shared).ptr, s.buffer(shared).ptr
            band.tau_dev = s.buffer(band.num_bins * gk.num_classes * L).ptr
        keys = None
        if key is not None:
            keys = api.GrtKdistKeys()
            for k in (keys.lw, keys.sw):
                k.kind, k.layer, k.map_dev = key[0], key[1], None
        calls[mode] = (gk, keep, keys)

    def step(mode):
        gk, _keep, keys = calls[mode]
        if keys is None:
            api.check(s.lib.grt_pipeline_run_kdist(pipe.p, api.C.byref(gcols), api.C.byref(gk)))
        else:
            api.check(s.lib.grt_pipeline_run_kdist_correlated(pipe.p, api.C.byref(gcols), api.C.byref(gk), api.C.byref(keys)))

    names = tuple(modes)
    samples, median, spread = s.measure(names, step, TAGS)
    result = {"workload": s.workload + f"; {el.size - 1} longwave and {es.size - 1} shortwave bins, contiguous over the whole "
                                       f"grid; {s.args.classes} classes (..._1024: 1024); no weight",
              "reps": s.args.reps, "order": ", ".join(names) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "wall_ms": {m: median[m]["wall_ms"] for m in names},
              "kdist_kernel_ms": {m: median[m]["kdist_ms"] for m in names},
              "map_kernel_ms": {m: median[m]["map_ms"] for m in names},
              "mapped_kernel_ms": {m: median[m]["mapped_ms"] for m in names},
              "kernel_spread_ms": {m: {k: spread[m][k] for k in ("kdist_ms", "map_ms", "mapped_ms")} for m in names}}
    s.finish(result, ("wall_ms", "kdist_kernel_ms", "map_kernel_ms", "mapped_kernel_ms", "kernel_spread_ms"))


if __name__ == "__main__":
    main()
