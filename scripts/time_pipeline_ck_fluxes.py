"""Cost of grt_pipeline_run_ck_fluxes -- the source sums, the solves on the g-classes and the bin sums behind the map and
the mapped reduction -- beside grt_pipeline_run_kdist_correlated for the same request, and how far the correlated-k fluxes
are from the line-by-line ones, on the G1 workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line
lists, fast = 3).

Alternating repetitions of these steps on one pipeline, in one process, with --bins contiguous bins of equal width per
band, the key the column's vertical optical depth (GRT_KDIST_KEY_SUM), classes log-spaced over the range of that key that
the columns populate (found by a first call with 1024 classes over 1e-12 .. 1e12: classes over a range the key never
visits would leave one g-point a bin):
  correlated_16, correlated_64   grt_pipeline_run_kdist_correlated (the yardstick: kdist_mapped_kernel reduces L rows a band)
  ck_16, ck_64                   grt_pipeline_run_ck_fluxes, every output taken
  correlated_lw_64, ck_lw_64, correlated_sw_64, ck_sw_64   the same with one band's bins alone: the tags are both bands'
                                 together, and the bands' grids differ in length
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 30, the class map; 31, the mapped reduction; 32, the source
sums; 33 / 34, the longwave / shortwave solve with its bin sums; 1 / 2 and 6 / 7, the gas optics) and the wall time of the
whole step, synchronised; the mapped reduction and the source sums also per row and band (L rows against 2 V + 1 longwave
and 4 shortwave rows).  Then, per K and band: the largest and the RMS difference in W m-2, over columns and levels, between
bin_up / bin_down summed over the bins and grt_pipeline_run_band_profiles' line-by-line values summed over the same bins.
Reported, not gated.  Result: profiles/pipeline_ck_fluxes_timing.json (or the path given).

    python scripts/time_pipeline_ck_fluxes.py [--reps 5] [--bins 16] [--out ...]
"""
import numpy as np

from pipeline_timing import Session  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_band_profiles import equal_bins

TAGS = {"map_ms": api.TAG_KDIST_MAP, "mapped_ms": api.TAG_KDIST_MAPPED, "sources_ms": api.TAG_CK_SOURCES,
        "ck_lw_ms": api.TAG_CK_LW, "ck_sw_ms": api.TAG_CK_SW, "lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW,
        "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW}
CLASSES = (16, 64)


def arguments(ap):
    ap.add_argument("--bins", type=int, default=16)


def main():
    s = Session("pipeline_ck_fluxes_timing.json", arguments)
    pipe, gcols, wl, ncol, V = s.pipe, s.gcols, s.wl, s.ncol, s.V
    el, es = equal_bins(wl.grid_lw.n, s.args.bins), equal_bins(wl.grid_sw.n, s.args.bins)
    # the range of the key that the columns populate, both bands
    probe = np.logspace(-12.0, 12.0, 1023)
    pipe.run_kdist_correlated(gcols, probe, lw_edges=el, sw_edges=es)
    found = pipe.kdist_correlated(ncol)
    used = np.flatnonzero(found["lw"]["points"].sum(axis=(0, 1)) + found["sw"]["points"].sum(axis=(0, 1)))
    lo, hi = probe[max(used[0] - 1, 0)], probe[min(used[-1], probe.size - 1)]
    edges = {K: np.logspace(np.log10(lo), np.log10(hi), K - 1) for K in CLASSES}

    def step(mode):
        kind, *band, K = mode.split("_")
        run = pipe.run_kdist_correlated if kind == "correlated" else pipe.run_ck_fluxes
        run(gcols, edges[int(K)], lw_edges=el if band != ["sw"] else None, sw_edges=es if band != ["lw"] else None)

    names = tuple(f"{kind}_{K}" for K in CLASSES for kind in ("correlated", "ck"))
    names += tuple(f"{kind}_{band}_64" for band in ("lw", "sw") for kind in ("correlated", "ck"))
    samples, median, spread = s.measure(names, step, TAGS)
    L = V - 1
    per_row = {band: {"points": int(n), "mapped_ms_per_row": median[f"ck_{band}_64"]["mapped_ms"] / L,
                      "mapped_ms_per_row_in_run_kdist_correlated": median[f"correlated_{band}_64"]["mapped_ms"] / L,
                      "sources_ms_per_row": median[f"ck_{band}_64"]["sources_ms"] / rows}
               for band, n, rows in (("lw", wl.grid_lw.n, 2 * V + 1), ("sw", wl.grid_sw.n, 4))}

    # the second number: correlated-k minus line-by-line, both summed over the bins
    pipe.run_band_profiles(gcols, lw_edges=el, sw_edges=es)
    lbl = pipe.band_profiles(ncol)
    differences = {}
    for K in CLASSES:
        pipe.run_ck_fluxes(gcols, edges[K], lw_edges=el, sw_edges=es)
        ck = pipe.ck_fluxes(ncol)
        differences[f"{K}"] = {}
        for band in ("lw", "sw"):
            for mine, theirs in (("bin_up", "_up"), ("bin_down", "_down")):
                d = ck[band][mine].sum(axis=2) - lbl[band + theirs][:, 0].sum(axis=1)          # [ncol][V]
                differences[f"{K}"][f"{band}_{mine[4:]}"] = {
                    "max_abs_w_m2": float(np.abs(d).max()), "rms_w_m2": float(np.sqrt(np.mean(d * d))),
                    "largest_line_by_line_w_m2": float(np.abs(lbl[band + theirs][:, 0].sum(axis=1)).max())}
    result = {"workload": s.workload + f"; {el.size - 1} longwave and {es.size - 1} shortwave bins, contiguous over the whole "
                                       f"grid; 16 and 64 classes log-spaced over {lo:.3e} .. {hi:.3e}, the range of the key; the SUM key",
              "class_range": [float(lo), float(hi)],
              "reps": s.args.reps, "order": ", ".join(names) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "wall_ms": {m: median[m]["wall_ms"] for m in names},
              "kernel_ms": {m: {k: median[m][k] for k in ("map_ms", "mapped_ms", "sources_ms", "ck_lw_ms", "ck_sw_ms")}
                            for m in names},
              "per_row_at_64_classes": per_row,
              "ck_minus_line_by_line": differences}
    s.finish(result, ("wall_ms", "kernel_ms", "per_row_at_64_classes", "class_range", "ck_minus_line_by_line"))


if __name__ == "__main__":
    main()
