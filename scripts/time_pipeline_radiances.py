"""Cost of the longwave radiances of grt_pipeline_run_sky_radiances over grt_pipeline_run_sky, on the G1 workload
(grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), all four sets, with the
synthetic aerosol of scripts/time_pipeline_aerosols.py and S draws of the synthetic cloud fields of
scripts/pipeline_timing.py per column and pass, at A viewing angles per column (secants 1 to 3, evenly spaced).

Alternating repetitions of these steps on one pipeline, in one process:
  sky               grt_pipeline_run_sky, six-row form
  radiances         grt_pipeline_run_sky_radiances with fluxes_dev: the same launches and, behind each set's longwave
                    solver, the radiance kernel
  radiances_alone   grt_pipeline_run_sky_radiances with fluxes_dev NULL: the longwave gas optics and the radiance kernel,
                    no flux solver and nothing of the shortwave
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 25, the radiance kernel; the longwave and shortwave gas
optics and solvers; the subcolumn mean) and the wall time of the whole step, synchronised.  Reported, not gated.
Result: profiles/pipeline_radiances_timing.json (or the path given).

    python scripts/time_pipeline_radiances.py [--reps 5] [--subcolumns 4] [--angles 8] [--out ...]
"""
import numpy as np

from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from time_pipeline_aerosols import synthetic_aerosols

TAGS = {"radiance_ms": api.TAG_RADIANCE, "lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW,
        "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW, "lw_clear_ms": api.TAG_SOLVER_LW,
        "sw_clear_ms": api.TAG_SOLVER_SW, "lw_aerosol_ms": api.TAG_AEROSOL_LW, "sw_aerosol_ms": api.TAG_AEROSOL_SW,
        "lw_allsky_ms": api.TAG_ALLSKY_LW, "sw_allsky_ms": api.TAG_ALLSKY_SW, "lw_sky_ms": api.TAG_SKY_LW,
        "sw_sky_ms": api.TAG_SKY_SW, "subcolumn_mean_ms": api.TAG_SUBCOLUMN_MEAN}


def arguments(ap):
    ap.add_argument("--subcolumns", type=int, default=4)
    ap.add_argument("--angles", type=int, default=8)


def main():
    s = Session("pipeline_radiances_timing.json", arguments)
    pipe, gcols, lib, C, ncol, V, S, A = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.subcolumns, s.args.angles
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], S)[S]   # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    gsky, keep_sky = api.make_sky(gclouds, gaer, S, api.GRT_SKY_ALL)
    N = api.GRT_SKY_MAX_SETS
    six = s.buffer(N * api.GRT_FLUXES_PER_COLUMN)
    secants = np.ascontiguousarray(np.tile(np.linspace(1.0, 3.0, A), (ncol, 1)))
    grad = api.GrtRadiances(A, secants.ctypes.data_as(C.POINTER(C.c_double)),
                            s.buffer(N * A * api.GRT_RADIANCE_ROWS_PER_ANGLE).ptr, None, None)

    def step(mode):
        if mode == "sky":
            api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(gsky), None, None, six.ptr))
        else:
            api.check(lib.grt_pipeline_run_sky_radiances(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(grad),
                                                         six.ptr if mode == "radiances" else None))

    modes = ["sky", "radiances", "radiances_alone"]
    samples, median, spread = s.measure(modes, step, TAGS)
    result = {"workload": s.workload + f"; all four sets, synthetic aerosol on 16 points per band, {S} draws of synthetic "
                                       f"clouds in about a third of the layers, {A} viewing angles per column",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "wall_ms": {m: median[m]["wall_ms"] for m in modes},
              "radiance_kernel_ms": {m: median[m]["radiance_ms"] for m in modes}}
    s.finish(result, ("wall_ms", "radiance_kernel_ms"))


if __name__ == "__main__":
    main()
