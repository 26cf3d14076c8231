"""Cost of the response rows of grt_pipeline_run_sky_weighted over grt_pipeline_run_sky and grt_pipeline_run_sky_direct in
their profile forms, on the G1 workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists,
fast = 3), all four sets, with the synthetic aerosol of scripts/time_pipeline_aerosols.py and S draws of the synthetic
cloud fields of scripts/pipeline_timing.py per column and pass.

Alternating repetitions of these steps on one pipeline, in one process:
  sky_levels       grt_pipeline_run_sky, profile form
  direct_levels    grt_pipeline_run_sky_direct, profile form, direct_level_fluxes_dev given
  weighted_narrow  grt_pipeline_run_sky_weighted, 8 responses per band, each 40 points inside one 128-point solver block
  weighted_broad   grt_pipeline_run_sky_weighted, 8 responses per band, each a tenth of the grid wide, one after the other
Per step: the kernel times by HIP-event profile tag (grt_ext.h: the solvers of the four passes in both bands, the gas
optics, the subcolumn mean, and 14, under which the finishing and actinic kernels count) and the wall time of the whole
step, synchronised.  Reported, not gated: the wall time and the solver tags' sum of each step over direct_levels', with
the spread of the repetitions; and the (response, block) pairs and scratch doubles of the two response sets.
Result: profiles/pipeline_weighted_timing.json (or the path given).

    python scripts/time_pipeline_weighted.py [--reps 3] [--subcolumns 4] [--out profiles/pipeline_weighted_timing.json]
"""
from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
import numpy as np
from grtcode_amd import api
from time_pipeline_aerosols import synthetic_aerosols

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW,
        "lw_clear_ms": api.TAG_SOLVER_LW, "sw_clear_ms": api.TAG_SOLVER_SW, "lw_aerosol_ms": api.TAG_AEROSOL_LW,
        "sw_aerosol_ms": api.TAG_AEROSOL_SW, "lw_allsky_ms": api.TAG_ALLSKY_LW, "sw_allsky_ms": api.TAG_ALLSKY_SW,
        "lw_sky_ms": api.TAG_SKY_LW, "sw_sky_ms": api.TAG_SKY_SW, "subcolumn_mean_ms": api.TAG_SUBCOLUMN_MEAN,
        "finish_ms": api.TAG_BAND_PROFILES}
SOLVERS = ("lw_clear_ms", "sw_clear_ms", "lw_aerosol_ms", "sw_aerosol_ms", "lw_allsky_ms", "sw_allsky_ms", "lw_sky_ms",
           "sw_sky_ms")
R = 8


def narrow(n):
    """R responses of 40 points, each inside one solver block, spread over the grid."""
    blocks = np.linspace(0, (n - 1) // 128 - 1, R).astype(int)
    return [int(b) * 128 + 44 for b in blocks], [np.hanning(42)[1:-1] for _ in blocks]


def broad(n):
    """R responses a tenth of the grid wide, one after the other from the grid's first point."""
    width = n // 10
    return [k * width for k in range(R)], [np.hanning(width + 2)[1:-1] for _ in range(R)]


def main():
    s = Session("pipeline_weighted_timing.json", lambda ap: ap.add_argument("--subcolumns", type=int, default=4))
    pipe, gcols, lib, C, ncol, V, S = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.subcolumns
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], S)[S]   # (the struct points into keep_clouds' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    gsky, keep_sky = api.make_sky(gclouds, gaer, S, api.GRT_SKY_ALL)
    N = api.GRT_SKY_MAX_SETS
    six = s.buffer(N * api.GRT_FLUXES_PER_COLUMN)
    levels = s.buffer(N * api.GRT_PROFILE_ROWS_PER_COLUMN * V)
    heating = s.buffer(N * api.GRT_HEATING_ROWS_PER_COLUMN * (V - 1))
    direct = api.GrtDirectBeam(s.buffer(N * api.GRT_DIRECT_ROWS_PER_SET).ptr, s.buffer(N * V).ptr)
    weighted, act = s.buffer(N * 5 * R * V), s.buffer(N * R * V)
    n_lw, n_sw = int(s.wl.grid_lw.n), int(s.wl.grid_sw.n)
    responses, shape = {}, {}
    for name, make in (("narrow", narrow), ("broad", broad)):
        g, keep = api.make_responses(lw=make(n_lw), sw=make(n_sw))
        g.weighted_levels_dev, g.actinic_levels_dev = weighted.ptr, act.ptr
        pairs = [api.response_pair_count(g, bi, n) for bi, n in ((0, n_lw), (1, n_sw))]
        responses[name] = g
        shape[name] = {"pairs_lw": pairs[0], "pairs_sw": pairs[1],
                       "scratch_doubles": ncol * S * V * (2 * pairs[0] + 3 * pairs[1])}
    form = (levels.ptr, heating.ptr, six.ptr)

    def step(mode):
        entry, kind = mode.split("_")
        if entry == "sky":
            api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(gcols), C.byref(gsky), *form))
        elif entry == "direct":
            api.check(lib.grt_pipeline_run_sky_direct(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(direct), *form))
        else:
            api.check(lib.grt_pipeline_run_sky_weighted(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(responses[kind]), *form))

    modes = ["sky_levels", "direct_levels", "weighted_narrow", "weighted_broad"]
    samples, median, spread = s.measure(modes, step, TAGS)

    def solvers(mode, rep):
        return sum(samples[mode][k][rep] for k in SOLVERS)

    reps = range(s.args.reps)
    over = {m: {"solver_tags": [solvers(m, r) / solvers("direct_levels", r) for r in reps],
                "wall": [samples[m]["wall_ms"][r] / samples["direct_levels"]["wall_ms"][r] for r in reps]} for m in modes}
    result = {"workload": s.workload + f"; all four sets, synthetic aerosol on 16 points per band, {S} draws of synthetic "
                                       f"clouds in about a third of the layers; {R} responses per band",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "responses": shape, "block_limit": [pipe.response_block_limit(0), pipe.response_block_limit(1)],
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "solver_tags_ms": {m: [solvers(m, r) for r in reps] for m in modes},
              "over_direct_levels": over,
              "wall_ms": {m: median[m]["wall_ms"] for m in modes},
              "finish_ms": {m: median[m]["finish_ms"] for m in modes}}
    s.finish(result, ("responses", "solver_tags_ms", "over_direct_levels", "wall_ms", "finish_ms"))


if __name__ == "__main__":
    main()
