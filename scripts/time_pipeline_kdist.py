"""Cost of the k-distribution kernel of grt_pipeline_run_kdist beside the gas optics of the same call, on the G1 workload
(grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3).

Alternating repetitions of these steps on one pipeline, in one process:
  run         grt_pipeline_run: the gas optics and the clear-sky solvers (the yardstick)
  kdist       grt_pipeline_run_kdist, --bins contiguous bins of equal width per band, --classes classes log-spaced over
              twelve decades, no weight
  kdist_sun   the same with the solar spectrum as the shortwave band's weight
  kdist_1024  the same bins with 1024 classes (a thread owns four), no weight
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 29, the k-distribution kernel, both bands' launches
together; 1 / 2 and 6 / 7, the gas optics) and the wall time of the whole step, synchronised.  Reported, not gated.
Result: profiles/pipeline_kdist_timing.json (or the path given).

    python scripts/time_pipeline_kdist.py [--reps 5] [--bins 16] [--classes 64] [--out ...]
"""
import numpy as np

from pipeline_timing import Session  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_band_profiles import equal_bins

TAGS = {"kdist_ms": api.TAG_KDIST, "lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW,
        "sw_far_ms": api.TAG_FAR_SW, "lw_solver_ms": api.TAG_SOLVER_LW, "sw_solver_ms": api.TAG_SOLVER_SW}


def arguments(ap):
    ap.add_argument("--bins", type=int, default=16)
    ap.add_argument("--classes", type=int, default=64)


def main():
    s = Session("pipeline_kdist_timing.json", arguments)
    pipe, gcols, wl = s.pipe, s.gcols, s.wl
    el, es = equal_bins(wl.grid_lw.n, s.args.bins), equal_bins(wl.grid_sw.n, s.args.bins)
    classes = {"kdist": np.logspace(-10.0, 2.0, s.args.classes - 1), "kdist_1024": np.logspace(-10.0, 2.0, 1023)}
    classes["kdist_sun"] = classes["kdist"]
    solar = np.ascontiguousarray(wl.solar, dtype=np.float64)
    L = s.V - 1
    calls = {}
    for mode, ce in classes.items():
        gk, keep = api.make_kdist(ce, el, es, sw_weight=solar if mode == "kdist_sun" else None)
        for band in (gk.lw, gk.sw):
            per_column = L * band.num_bins * gk.num_classes
            band.points_dev, band.weight_dev, band.tau_dev = (s.buffer(per_column).ptr for _ in range(3))
        calls[mode] = (gk, keep)

    def step(mode):
        if mode == "run":
            pipe.run(gcols)
        else:
            api.check(s.lib.grt_pipeline_run_kdist(pipe.p, api.C.byref(gcols), api.C.byref(calls[mode][0])))

    modes = ("run", "kdist", "kdist_sun", "kdist_1024")
    samples, median, spread = s.measure(modes, step, TAGS)
    gas = {m: sum(median[m][k] for k in ("lw_gas_ms", "sw_gas_ms", "lw_far_ms", "sw_far_ms")) for m in modes}
    result = {"workload": s.workload + f"; {el.size - 1} longwave and {es.size - 1} shortwave bins, contiguous over the whole "
                                       f"grid; {s.args.classes} classes (kdist_1024: 1024)",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "wall_ms": {m: median[m]["wall_ms"] for m in modes},
              "kdist_kernel_ms": {m: median[m]["kdist_ms"] for m in modes}, "gas_optics_ms": gas}
    s.finish(result, ("wall_ms", "kdist_kernel_ms", "gas_optics_ms"))


if __name__ == "__main__":
    main()
