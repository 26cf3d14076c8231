"""Cost of grt_pipeline_run_sky_zeniths_slant against grt_pipeline_run_sky_zeniths_direct of the parent commit's library, on
the G1 workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), six-row form,
all four sets, Z = 8 day angles per column, S = 1 and 4 draws of the synthetic cloud fields of scripts/pipeline_timing.py,
the synthetic aerosol of scripts/time_pipeline_aerosols.py, open water's direct albedo on three knots per (column, angle)
and every angle's direct beam.

Two runs, each alternating repetitions of its steps on one pipeline, in one process, for each S:
  under the parent's library (GRT_LIB_PATH names it; it lacks the new entry point):
    direct_S      grt_pipeline_run_sky_zeniths_direct with the surface and the direct beam: the yardstick
  under this tree's library, with --parent naming the first run's result:
    direct_S      the same call of this tree's library (its kernels are the parent's, instruction for instruction)
    slant_S       the new call with the layer cosines of a spherical planet over the columns' hypsometric heights
    slant_flat_S  the new call with every layer at the angle's own cosine: direct_S's arithmetic, the loads added
Per step the synchronised wall time and the kernel times by HIP-event profile tag; medians, and spreads = max - min.
The expectation to check, not a threshold: the new call loses a few scalar loads per layer and angle in kernels bound by
fp64 arithmetic.  Result: profiles/pipeline_sky_zeniths_slant_timing.json (or the path given), the parent's run inside it.

    GRT_LIB_PATH=<parent's libgrtcode_hip.so> python scripts/time_pipeline_sky_zeniths_slant.py --out parent.json
    python scripts/time_pipeline_sky_zeniths_slant.py --parent parent.json [--reps 5] [--zeniths 8] [--out ...]
"""
import json

import numpy as np

from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api, surfaces
from time_pipeline_aerosols import synthetic_aerosols

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "zenith_sw_ms": api.TAG_ZENITH_SW,
        "sky_zenith_sw_ms": api.TAG_SKY_ZENITH_SW, "sky_zenith_mean_ms": api.TAG_SKY_ZENITH_MEAN}
DRAWS = (1, 4)


def arguments(ap):
    ap.add_argument("--zeniths", type=int, default=8)
    ap.add_argument("--parent", default=None, help="the result of the run under the parent's library")


def main():
    s = Session("pipeline_sky_zeniths_slant_timing.json", arguments)
    pipe, gcols, lib, C, ncol, V, Z = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.zeniths
    has_slant = hasattr(lib, "grt_pipeline_run_sky_zeniths_slant")
    clouds = subcolumn_clouds(s.keep["p"], s.keep["tl"], max(DRAWS))           # (the structs point into their keeps' arrays)
    gaer, keep_aer = api.make_aerosols(lw=synthetic_aerosols(s.wl.grid_lw, ncol, V - 1, 3, True),
                                       sw=synthetic_aerosols(s.wl.grid_sw, ncol, V - 1, 4, False))
    sky = {S: api.make_sky(clouds[S][0], gaer, S, api.GRT_SKY_ALL) for S in DRAWS}
    mu = np.ascontiguousarray([np.roll(np.linspace(0.15, 1.0, Z), c) for c in range(ncol)])
    gz, keep_z = api.make_zeniths(mu)
    sw = s.wl.grid_sw
    span = sw.dw * (sw.n - 1)
    xa = np.array([sw.w0 + 0.1 * span, sw.w0 + 0.5 * span, sw.w0 + 0.9 * span])
    knots = np.ascontiguousarray(surfaces.ocean_direct_albedo(mu)[:, :, None] * np.array([0.8, 1.0, 1.1])[None, None, :])
    gsurf, keep_surf = api.make_zenith_surface(xa, knots)
    kinds = ["direct"]
    slants = {}
    if has_slant:
        from grtcode_amd import geometry
        heights = geometry.level_heights(np.asarray(s.keep["p"]).reshape(ncol, V), np.asarray(s.keep["tl"]).reshape(ncol, V - 1))
        slants = {"slant": api.make_zenith_slant(geometry.slant_cosines(geometry.EARTH_RADIUS, heights, mu)),
                  "slant_flat": api.make_zenith_slant(np.repeat(mu[:, :, None], V - 1, axis=2))}
        kinds += list(slants)
    nsets = api.GRT_SKY_MAX_SETS
    out = s.buffer(nsets * api.GRT_FLUXES_PER_COLUMN)
    angle_six = s.buffer(nsets * Z * 6)
    direct_three, angle_three = s.buffer(nsets * api.GRT_DIRECT_ROWS_PER_SET), s.buffer(nsets * Z * api.GRT_DIRECT_ROWS_PER_SET)
    gz.zenith_fluxes_dev = angle_six.ptr
    gdirect = api.GrtZenithDirect(direct_three.ptr, None, angle_three.ptr, None)
    modes = [f"{kind}_{S}" for S in DRAWS for kind in kinds]

    def step(mode):
        kind, _, S = mode.rpartition("_")
        gsky = sky[int(S)][0]
        if kind == "direct":
            api.check(lib.grt_pipeline_run_sky_zeniths_direct(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(gz), C.byref(gsurf),
                                                              C.byref(gdirect), None, None, out.ptr))
        else:
            api.check(lib.grt_pipeline_run_sky_zeniths_slant(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(gz),
                                                             C.byref(slants[kind][0]), C.byref(gsurf), C.byref(gdirect), None,
                                                             None, out.ptr))

    samples, median, spread = s.measure(modes, step, TAGS)
    wall = {m: median[m]["wall_ms"] for m in modes}
    result = {"workload": s.workload + f"; four sets, synthetic aerosol on 16 points per band, synthetic clouds; Z = {Z} day "
                                       "angles, 0.15 to 1 in another order per column; open water's direct albedo on three knots; "
                                       "every angle's direct beam",
              "library": "this tree's" if has_slant else "the parent commit's (GRT_LIB_PATH)",
              "reps": s.args.reps, "zeniths": Z,
              "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples, "wall_ms": wall}
    show = ["library", "wall_ms"]
    if has_slant:
        result["zenith_chunk_slant"] = [api.GRT_ZENITH_CHUNK_SLANT, api.GRT_ZENITH_CHUNK_SLANT_SURFACE]
    if has_slant and s.args.parent is not None:
        with open(s.args.parent) as f:
            parent = json.load(f)
        result["parent"] = parent
        pw, ps = parent["wall_ms"], parent["spread_max_minus_min"]
        result["over_parent_run_sky_zeniths_direct"] = {m: wall[m] / pw[f"direct_{m.rpartition('_')[2]}"] for m in modes}
        result["solver_ms_over_parent"] = {
            m: (median[m]["zenith_sw_ms"] + median[m]["sky_zenith_sw_ms"]) /
               (parent["median"][f"direct_{m.rpartition('_')[2]}"]["zenith_sw_ms"] +
                parent["median"][f"direct_{m.rpartition('_')[2]}"]["sky_zenith_sw_ms"]) for m in modes}
        result["parent_wall_spread_over_median"] = {m: ps[m]["wall_ms"] / pw[m] for m in pw}
        show += ["over_parent_run_sky_zeniths_direct", "solver_ms_over_parent", "parent_wall_spread_over_median"]
    s.finish(result, show)


if __name__ == "__main__":
    main()
