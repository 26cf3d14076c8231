"""Cost of grt_pipeline_run_sky_tiles against the route that exists without it -- T times grt_pipeline_set_surface +
grt_pipeline_run_sky -- on the G1 workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists,
fast = 3), six-row form, the clean and the cloud set, S = 4 draws of the synthetic cloud fields of
scripts/pipeline_timing.py, T = 1, 4, 8 tiles per column with knots of their own in both bands.

Every step once as a warm-up (every buffer allocated, every kernel loaded, every shape seen), then five alternating
repetitions of these steps on one pipeline, in one process, each followed by the pipeline's sync:
  loop_T     the parent commit's route: for each of T tiles set_surface with the tile's knots, then run_sky with the
             columns at the tile's temperatures (T gas-optics passes per band)
  tiles_T    one grt_pipeline_run_sky_tiles with T tiles per column (one gas-optics pass per band)
Per step: the kernel times by HIP-event profile tag (grt_ext.h: 1 / 2 and 6 / 7 gas optics; 3, 4, 8, 9 the solvers of
run_sky's two sets; 11 its subcolumn mean; 15 the surface rows; 35, 36 the tile kernels, 37 their mean) and the wall time of
the whole step, synchronised; medians, and spreads = max - min.
Result: profiles/pipeline_tiles_timing.json (or the path given).

    python scripts/time_pipeline_tiles.py [--reps 5] [--subcolumns 4] [--out ...]
"""
import numpy as np

from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "lw_far_ms": api.TAG_FAR_LW, "sw_far_ms": api.TAG_FAR_SW,
        "lw_clear_ms": api.TAG_SOLVER_LW, "sw_clear_ms": api.TAG_SOLVER_SW, "lw_allsky_ms": api.TAG_ALLSKY_LW,
        "sw_allsky_ms": api.TAG_ALLSKY_SW, "subcolumn_mean_ms": api.TAG_SUBCOLUMN_MEAN, "surface_rows_ms": api.TAG_SURFACE,
        "tile_lw_ms": api.TAG_TILE_LW, "tile_sw_ms": api.TAG_TILE_SW, "tile_mean_ms": api.TAG_TILE_MEAN}
GAS = ("lw_gas_ms", "sw_gas_ms", "lw_far_ms", "sw_far_ms")
TILE = ("tile_lw_ms", "tile_sw_ms", "tile_mean_ms")
COUNTS = (1, 4, 8)
KNOTS = 6


def arguments(ap):
    ap.add_argument("--subcolumns", type=int, default=4)


def tile_inputs(grid_lw, grid_sw, t_surf, T, seed):
    """Knot grids inside each band, and per (column, tile) knot values in [0.05, 0.95] and a temperature near the column's."""
    rng = np.random.default_rng(seed)
    ncol = t_surf.size
    grids = [np.linspace(g.w0 + 0.1 * (g.n - 1) * g.dw, g.w0 + 0.9 * (g.n - 1) * g.dw, KNOTS) for g in (grid_lw, grid_sw)]
    emis = rng.uniform(0.8, 0.95, (ncol, T, KNOTS))
    adir, adif = rng.uniform(0.05, 0.6, (ncol, T, KNOTS)), rng.uniform(0.05, 0.6, (ncol, T, KNOTS))
    ts = t_surf[:, None] + rng.uniform(-5.0, 5.0, (ncol, T))
    fraction = rng.uniform(0.1, 1.0, (ncol, T))
    return grids, emis, adir, adif, ts, fraction / fraction.sum(axis=1, keepdims=True)


def main():
    s = Session("pipeline_tiles_timing.json", arguments)
    pipe, lib, C, ncol, S = s.pipe, s.lib, api.C, s.ncol, s.args.subcolumns
    gclouds, keep_clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], S)[S]   # (the struct points into keep_clouds' arrays)
    gsky, keep_sky = api.make_sky(gclouds, None, S, api.GRT_SKY_CLEAN | api.GRT_SKY_CLOUD)
    nsets = keep_sky["nsets"]
    out = s.buffer(nsets * api.GRT_FLUXES_PER_COLUMN)
    tile_out = s.buffer(nsets * max(COUNTS) * api.GRT_FLUXES_PER_COLUMN)
    tiles, surfaces, columns = {}, {}, {}
    t_surf = np.array(s.keep["ts"], dtype=np.float64)
    for T in COUNTS:
        grids, emis, adir, adif, ts, fraction = tile_inputs(s.wl.grid_lw, s.wl.grid_sw, t_surf, T, 17 + T)
        tiles[T] = api.make_surface_tiles(ncol, ts, fraction=fraction, emissivity=(grids[0], emis),
                                          albedo=(grids[1], adir, adif))
        tiles[T][0].tile_fluxes_dev = tile_out.ptr
        surfaces[T] = [api.make_surface(ncol, emissivity=(grids[0], emis[:, t]), albedo=(grids[1], adir[:, t], adif[:, t]))
                       for t in range(T)]
        columns[T] = ts
    modes = [f"loop_{T}" for T in COUNTS] + [f"tiles_{T}" for T in COUNTS]
    own_ts = s.keep["ts"].copy()

    def step(mode):
        kind, _, n = mode.partition("_")
        T = int(n)
        if kind == "tiles":
            api.check(lib.grt_pipeline_run_sky_tiles(pipe.p, C.byref(s.gcols), C.byref(gsky), C.byref(tiles[T][0]), out.ptr))
            return
        for t in range(T):
            pipe.set_surface(surfaces[T][t][0])
            pipe.sync()                                       # (the columns' temperatures are read during the call)
            s.keep["ts"][:] = columns[T][:, t]
            api.check(lib.grt_pipeline_run_sky(pipe.p, C.byref(s.gcols), C.byref(gsky), None, None, out.ptr))
        pipe.sync()
        s.keep["ts"][:] = own_ts
        pipe.set_surface(None)

    samples, median, spread = s.measure(modes, step, TAGS)
    result = {"workload": s.workload + f"; sets clean and cloud, {S} draws of synthetic clouds; T = {COUNTS} tiles per column, "
                                       f"{KNOTS} knots per tile and band",
              "tile_chunk": api.GRT_TILE_CHUNK, "reps": s.args.reps,
              "order": ", ".join(modes) + " alternating after one warm-up pass; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples,
              "wall_ms": {m: median[m]["wall_ms"] for m in modes},
              "gas_optics_ms": {m: sum(median[m][k] for k in GAS) for m in modes},
              "tile_kernels_ms": {m: sum(median[m][k] for k in TILE) for m in modes if m.startswith("tiles")},
              "tiles_over_loop_wall": {T: median[f"tiles_{T}"]["wall_ms"] / median[f"loop_{T}"]["wall_ms"] for T in COUNTS},
              "tiles_T_over_tiles_1_wall": {T: median[f"tiles_{T}"]["wall_ms"] / median["tiles_1"]["wall_ms"] for T in COUNTS}}
    s.finish(result, ["wall_ms", "gas_optics_ms", "tile_kernels_ms", "tiles_over_loop_wall", "tiles_T_over_tiles_1_wall"])


if __name__ == "__main__":
    main()
