"""Cost of grt_pipeline_run_sky_zeniths_direct against grt_pipeline_run_sky_zeniths and against the loop it replaces, on the
G1 workload (grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), six-row form, all
four sets, Z = 8 day angles per column, S = 1 and 4 draws of the synthetic cloud fields of scripts/pipeline_timing.py, the
synthetic aerosol of scripts/time_pipeline_aerosols.py, open water's direct albedo (surfaces.ocean_direct_albedo) on three
knots per (column, angle).

Alternating repetitions of these steps on one pipeline, in one process, for each S:
  zeniths_S   grt_pipeline_run_sky_zeniths: the parent's entry point on the same inputs
  surface_S   the new call with the surface only
  direct_S    the new call with the direct beam only
  both_S      the new call with both
  rounds_S    Z rounds of grt_pipeline_set_surface + grt_pipeline_run_sky_direct, one per angle: a gas-optics pass each
Per step the synchronised wall time and the kernel times by HIP-event profile tag; medians, and spreads = max - min.
The expectation to check, not a threshold: the new call costs run_sky_zeniths plus a few per cent (it adds three rows to
the sums and one table read per angle); the loop of rounds costs several times as much.
Result: profiles/pipeline_sky_zeniths_direct_timing.json (or the path given).

    python scripts/time_pipeline_sky_zeniths_direct.py [--reps 5] [--zeniths 8] [--out ...]
"""
import numpy as np

from pipeline_timing import Session, subcolumn_clouds  # (first: it puts the repository root on sys.path)
from grtcode_amd import api, surfaces
from time_pipeline_aerosols import synthetic_aerosols

TAGS = {"lw_gas_ms": api.TAG_GAS_LW, "sw_gas_ms": api.TAG_GAS_SW, "zenith_sw_ms": api.TAG_ZENITH_SW,
        "zenith_mean_ms": api.TAG_ZENITH_MEAN, "sky_zenith_sw_ms": api.TAG_SKY_ZENITH_SW,
        "sky_zenith_mean_ms": api.TAG_SKY_ZENITH_MEAN, "surface_ms": api.TAG_SURFACE, "sw_clear_ms": api.TAG_SOLVER_SW,
        "sw_aerosol_ms": api.TAG_AEROSOL_SW, "sw_allsky_ms": api.TAG_ALLSKY_SW, "sw_sky_ms": api.TAG_SKY_SW}
DRAWS = (1, 4)
KINDS = ("zeniths", "surface", "direct", "both", "rounds")


def arguments(ap):
    ap.add_argument("--zeniths", type=int, default=8)


def main():
    s = Session("pipeline_sky_zeniths_direct_timing.json", arguments)
    pipe, gcols, lib, C, ncol, V, Z = s.pipe, s.gcols, s.lib, api.C, s.ncol, s.V, s.args.zeniths
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
    # the loop of rounds: angle k's knots as the surface in force, the columns under angle k
    rounds = []
    for k in range(Z):
        g = type(gcols)()
        C.pointer(g)[0] = gcols
        mu_k = np.ascontiguousarray(mu[:, k])
        g.cos_zenith = mu_k.ctypes.data_as(api.c_double_p)
        rounds.append((g, mu_k, api.make_surface(ncol, albedo=(xa, np.ascontiguousarray(knots[:, k])))))
    nsets = api.GRT_SKY_MAX_SETS
    out = s.buffer(nsets * api.GRT_FLUXES_PER_COLUMN)
    angle_six = s.buffer(nsets * Z * 6)
    direct_three, angle_three = s.buffer(nsets * api.GRT_DIRECT_ROWS_PER_SET), s.buffer(nsets * Z * api.GRT_DIRECT_ROWS_PER_SET)
    gz.zenith_fluxes_dev = angle_six.ptr
    gdirect = api.GrtZenithDirect(direct_three.ptr, None, angle_three.ptr, None)
    gbeam = api.GrtDirectBeam(direct_three.ptr, None)
    modes = [f"{kind}_{S}" for S in DRAWS for kind in KINDS]

    def step(mode):
        kind, _, S = mode.partition("_")
        gsky = sky[int(S)][0]
        if kind == "zeniths":
            api.check(lib.grt_pipeline_run_sky_zeniths(pipe.p, C.byref(gcols), C.byref(gsky), C.byref(gz), None, None, out.ptr))
        elif kind == "rounds":
            for g, mu_k, (gs, keep_s) in rounds:
                pipe.set_surface(gs)
                api.check(lib.grt_pipeline_run_sky_direct(pipe.p, C.byref(g), C.byref(gsky), C.byref(gbeam), None, None, out.ptr))
            pipe.set_surface(None)
        else:
            api.check(lib.grt_pipeline_run_sky_zeniths_direct(
                pipe.p, C.byref(gcols), C.byref(gsky), C.byref(gz), C.byref(gsurf) if kind in ("surface", "both") else None,
                C.byref(gdirect) if kind in ("direct", "both") else None, None, None, out.ptr))

    samples, median, spread = s.measure(modes, step, TAGS)
    wall = {m: median[m]["wall_ms"] for m in modes}
    result = {"workload": s.workload + f"; four sets, synthetic aerosol on 16 points per band, synthetic clouds; Z = {Z} day "
                                       "angles, 0.15 to 1 in another order per column; open water's direct albedo on three knots",
              "reps": s.args.reps, "zeniths": Z, "zenith_chunk": api.GRT_ZENITH_CHUNK,
              "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread_max_minus_min": spread, "samples": samples, "wall_ms": wall,
              "new_call_over_run_sky_zeniths": {f"{kind}_{S}": wall[f"{kind}_{S}"] / wall[f"zeniths_{S}"]
                                                for S in DRAWS for kind in ("surface", "direct", "both")},
              "rounds_over_new_call_with_both": {str(S): wall[f"rounds_{S}"] / wall[f"both_{S}"] for S in DRAWS}}
    s.finish(result, ["wall_ms", "new_call_over_run_sky_zeniths", "rounds_over_new_call_with_both"])


if __name__ == "__main__":
    main()
