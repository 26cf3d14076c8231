"""The cases of tests/test_gpu_sw_sweep_bits.py and of tests/golden/make_sw_sweep_bits.py, which recorded their expected
bits: every entry point of the batched pipeline that reaches a kernel of k_shortwave.hip or one of the finishing
reductions of k_optics.hip behind them, on a pipeline with a shortwave band alone -- the surface tiles on one with both
bands, all twelve rows of a tile, since lw_tile_kernel shares the tile chunk's rule --, in both of its forms (fused, and
keep_spectra = 1) wherever the entry point takes both.

The shapes are the smallest at which those kernels can still go wrong: a grid of 129 points (two workgroups of 128, the
second with one live lane), 2 columns, 4 levels, 3 cloud draws and S = 1, an aerosol object on a two-point grid, 5 sun
angles per column (every chunk size in use is 4: a full chunk and a short one) of which one is a night angle -- in the
first chunk of column 0, the whole short chunk of column 1 --, 5 surface tiles (4 + 1) with per-tile albedo rows, direct and
diffuse, and with none, three bins (one inside a workgroup, one up to its edge, one across it), four g-classes of which
the last is empty.  Every pipeline exists at two user levels: 2 (inside: two sweeps, parking) and -1 (one sweep), and the
fused form's one-sweep runs are made once more under GRT_SW_TWO_SWEEPS=1.

Combinations that are left out, because the entry point refuses them or they say nothing new: a night column
(mu_dir <= 0) is accepted by run_ck_fluxes alone, every other entry point refuses it, so only that run has one (column 1);
run_sky_zeniths_slant is refused by the keep_spectra form; GRT_SW_TWO_SWEEPS is read by the fused form alone, so the
keep_spectra pipelines do not repeat their runs under it.  run_all() gives every output by name; the names are the
fixture's keys."""
import os
from contextlib import contextmanager

import numpy as np

from aerosol_model import aerosol_fields
from grtcode_amd import api, synthetic as syn
from lw_point_cases import cloud_tables
from pipeline_support import SETS, few_layer_clouds, make, pick, surface
from scenario import MOL_ORDER, Band

N, V, NCOL, S_MAX, Z, T = 129, 4, 2, 3, 5, 5
L = V - 1
LW_W0, SW_W0, SW_DW = 100.0, 1000.0, 10.0
SEED = 20261021
#: (name, user level, GRT_SW_TWO_SWEEPS): inside; the one sweep; the one-sweep user level in two sweeps (fused form alone)
MODES = (("inside", 2, False), ("ends", -1, False), ("ends_two_sweeps", -1, True))
FORMS = (("fused", False), ("spectra", True))
ALL = api.GRT_SKY_ALL
#: one night angle per column: in the first chunk of column 0, the whole short chunk of column 1
MU = np.array([[1.0, -0.3, 0.05, 0.5, 0.3], [0.999, 0.01, 0.7, 0.2, 0.0]])
WEIGHT = np.array([[0.25 + 0.125 * ((c + 3 * k) % 5) for k in range(Z)] for c in range(NCOL)])
SW_EDGES = np.array([0, 40, 127, 128])          # three bins: one inside a workgroup, one up to its edge, one across it
#: (first point, weights): inside one wave; across the boundary of the two workgroups; the last point alone
RESPONSES = ([10, 122, N - 1], [np.array([0.25, 0.5, 1.0, 2.0, 1.0, 0.5, -0.25]),
                                np.array([0.5, 1.0, 1.5, 2.0, 1.5, 1.0, 0.5]), np.array([1.0])])
CLASS_EDGES = np.array([1e-4, 1e-2, 1e30])      # four classes, the last one empty
POOL = (1.0, 0.5, 0.05, 1e-3, 0.3, 0.999, 0.01, 0.7, 0.2)      # (sky_zenith_support's: 1e-3 clamps tau/mu at 700)
assert all(Z % chunk for chunk in (api.GRT_ZENITH_CHUNK, api.GRT_ZENITH_CHUNK_SLANT, api.GRT_ZENITH_CHUNK_SLANT_SURFACE))
assert T % api.GRT_TILE_CHUNK


@contextmanager
def environment(**values):
    """the process environment with these variables set, as it was afterwards (the library reads both at every call)"""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


class Inputs:
    """Everything the runs need that is made on the host: the bands' files under root, columns, S_MAX draws of clouds,
    the aerosol fields of both bands, the surface, the per-angle knots and layer cosines, the tiles."""

    def __init__(self, root):
        self.lwb = Band(os.path.join(root, "lw"), LW_W0, LW_W0 + (N - 1) * 1.0, 1.0, 300)
        self.swb = Band(os.path.join(root, "sw"), SW_W0, SW_W0 + (N - 1) * SW_DW, SW_DW, 300, sw=True)
        assert self.lwb.nw == N and self.swb.nw == N
        self.tables = cloud_tables(os.path.join(root, "clouds"))
        self.cols = [syn.profile(900 + V + c, V) for c in range(NCOL)]
        self.night = [dict(col, mu0=(col["mu0"], -0.2)[c]) for c, col in enumerate(self.cols)]
        self.emis, self.alb = surface(N, N + V)
        # (two points: grid points below, between and above them)
        self.xa = tuple(w0 + np.array([0.3, 0.8]) * (N - 1) * dw for w0, dw in ((LW_W0, 1.0), (SW_W0, SW_DW)))
        self.fa = tuple(aerosol_fields(NCOL, L, x, SEED + bi, lw=bi == 0) for bi, x in enumerate(self.xa))
        draws = [few_layer_clouds(self.cols, self.tables, SEED % 1000 + j) for j in range(S_MAX)]
        self.cl = {k: (np.stack([d[k] for d in draws], axis=1) if k in SETS else draws[0][k]) for k in draws[0]}
        rng = np.random.default_rng(SEED)
        self.xk = SW_W0 + np.array([0.26, 0.5, 0.71]) * (N - 1) * SW_DW
        self.knots = rng.uniform(0.02, 0.9, (NCOL, Z, self.xk.size))
        self.cosines = np.asarray(POOL)[rng.integers(0, len(POOL), MU.shape + (L,))]
        self.cosines[~(MU > 0.0)] = np.nan                                   # (a night angle's are not read)
        self.t_tiles = np.array([[col["t_surf"] + 3.0 * ((2 * t + c) % 5 - 2) for t in range(T)]
                                 for c, col in enumerate(self.cols)])
        self.fraction = 0.375 * np.array([[1.0 + ((c + 2 * t) % 3) for t in range(T)] for c in range(NCOL)])
        self.xt = (LW_W0 + np.array([0.2, 0.45, 0.7]) * (N - 1), SW_W0 + np.array([0.2, 0.45, 0.7]) * (N - 1) * SW_DW)
        self.tile_knots = rng.uniform(0.0, 1.0, (3, NCOL, T, 3))             # emissivity, direct and diffuse albedo


def sw_of(d):
    """the shortwave's part of a profile dict, or of a six-row dict: its six of the twelve rows"""
    out = {k: a for k, a in d.items() if k.startswith("sw_") or k.startswith("angle_") or k.startswith("direct")}
    if "fluxes" in d:
        out["fluxes"] = d["fluxes"][..., 6:]
    return out


def shortwave_runs(inp, pipe, spectral, gcols, gnight, clouds, gaer, put):
    """every entry point on one shortwave-only pipeline; put(run, {key: array})"""
    gsky = {S: api.make_sky(clouds[S][0], gaer, S, ALL) for S in (1, S_MAX)}
    n = gsky[1][1]["nsets"]
    assert n == 4
    for S in (1, S_MAX):
        pipe.run_sky(gcols, gsky[S][0], profiles=False)
        put(f"S{S}.sky", sw_of(dict(fluxes=pipe.sky_fluxes(NCOL, n))))
        pipe.run_sky(gcols, gsky[S][0], profiles=True)
        put(f"S{S}.sky_profiles", sw_of(pipe.sky_profiles(NCOL, n)))
    g3 = gsky[S_MAX][0]
    pipe.run_sky_direct(gcols, g3, profiles=False)
    put("direct", sw_of(dict(fluxes=pipe.sky_fluxes(NCOL, n), direct=pipe.sky_direct_fluxes(NCOL, n))))
    pipe.run_sky_direct(gcols, g3, profiles=True)
    put("direct_profiles", sw_of(dict(pipe.sky_profiles(NCOL, n), **pipe.sky_direct_profiles(NCOL, n))))
    gresp, keep_resp = api.make_responses(lw=None, sw=RESPONSES)
    pipe.run_sky_weighted(gcols, g3, gresp)
    put("weighted", sw_of(pipe.sky_weighted(NCOL, n)))
    # sun angles: the clean pass with and without weights, then every set
    for name, wt in (("zeniths", None), ("zeniths_weighted", WEIGHT)):
        gz, keep_z = api.make_zeniths(MU, wt)
        pipe.run_zeniths(gcols, gz, profiles=False)
        fluxes, per_angle = pipe.zenith_fluxes(NCOL, Z)
        put(name, sw_of(dict(fluxes=fluxes, angle_fluxes=per_angle)))
        pipe.run_zeniths(gcols, gz, profiles=True)
        put(name + "_profiles", sw_of(pipe.zenith_profiles(NCOL, Z)))
    gz, keep_z = api.make_zeniths(MU, WEIGHT)
    gsurf, keep_surf = api.make_zenith_surface(inp.xk, inp.knots)
    gslant, keep_slant = api.make_zenith_slant(inp.cosines)
    for shared in ("0", "1"):
        with environment(GRT_ZENITH_SHARED=shared):
            pipe.run_sky_zeniths(gcols, g3, gz, profiles=False)
            fluxes, per_angle = pipe.sky_zenith_fluxes(NCOL, n, Z)
            put(f"sky_zeniths.shared{shared}", sw_of(dict(fluxes=fluxes, angle_fluxes=per_angle)))
            pipe.run_sky_zeniths(gcols, g3, gz, profiles=True)
            put(f"sky_zeniths_profiles.shared{shared}", sw_of(pipe.sky_zenith_profiles(NCOL, n, Z)))
            for name, gs in (("zen_direct", None), ("zen_direct_surface", gsurf)):
                pipe.run_sky_zeniths_direct(gcols, g3, gz, gsurface=gs, direct=True, profiles=False)
                put(f"{name}.shared{shared}", sw_of(pipe.sky_zenith_direct_fluxes(NCOL, n, Z)))
            pipe.run_sky_zeniths_direct(gcols, g3, gz, gsurface=gsurf, direct=True, profiles=True)
            put(f"zen_direct_surface_profiles.shared{shared}", sw_of(pipe.sky_zenith_direct_profiles(NCOL, n, Z)))
            if not spectral:
                for name, gs in (("slant", None), ("slant_surface", gsurf)):
                    pipe.run_sky_zeniths_slant(gcols, g3, gz, gslant, gsurface=gs, direct=True, profiles=False)
                    put(f"{name}.shared{shared}", sw_of(pipe.sky_zenith_direct_fluxes(NCOL, n, Z)))
    if not spectral:
        pipe.run_sky_zeniths_slant(gcols, g3, gz, gslant, gsurface=gsurf, direct=True, profiles=True)
        put("slant_surface_profiles", sw_of(pipe.sky_zenith_direct_profiles(NCOL, n, Z)))
    # bins, every point, the g-classes
    pipe.run_band_profiles(gcols, clouds[1][0], sw_edges=SW_EDGES)
    put("band_profiles", sw_of(pipe.band_profiles(NCOL)))
    pipe.run_spectral(gcols, clouds[1][0], sw_edges=SW_EDGES)
    sp = pipe.spectral(NCOL)
    put("spectral", dict(sw=sp["sw"], sw_bins=sp["sw_bins"]))
    pipe.run_ck_fluxes(gnight, CLASS_EDGES, sw_edges=SW_EDGES)
    ck = pipe.ck_fluxes(NCOL)["sw"]
    assert np.all(ck["points"][..., -1] == 0) and np.all(ck["points"].sum(axis=(1, 2)) > 0)
    put("ck", {k: ck[k] for k in ("up", "down", "bin_up", "bin_down")})
    if spectral:
        pipe.run(gcols)
        put("run", sw_of(dict(fluxes=pipe.fluxes(NCOL))))


def tile_runs(inp, pipe, gcols, clouds, gaer, put):
    """run_sky_tiles on one pipeline of both bands: all four sets of three draws over the tiles' own rows, and of one draw
    over the surface in force; all twelve rows of every tile"""
    rows, keep_rows = api.make_surface_tiles(NCOL, inp.t_tiles, fraction=inp.fraction, emissivity=(inp.xt[0], inp.tile_knots[0]),
                                             albedo=(inp.xt[1], inp.tile_knots[1], inp.tile_knots[2]))
    none, keep_none = api.make_surface_tiles(NCOL, inp.t_tiles)
    for name, gtiles, S in (("tiles_rows", rows, S_MAX), ("tiles_none", none, 1)):
        gsky, keep = api.make_sky(clouds[S][0], gaer, S, ALL)
        pipe.run_sky_tiles(gcols, gsky, gtiles)
        fluxes, tiles = pipe.sky_tile_fluxes(NCOL, keep["nsets"], T)
        put(name, dict(fluxes=fluxes, tiles=tiles))


def run_all(inp, device):
    """-> {name: array}: every output of every case.  `device` from api.create_device; deterministic mode is the
    caller's to set."""
    go_lw, _ = inp.lwb.gas_optics(device, V)
    go_sw, grid_sw = inp.swb.gas_optics(device, V)
    solar = api.create_solar_flux(grid_sw, inp.swb.files["solar"])
    gcols, keep_cols = api.make_columns(inp.cols, MOL_ORDER, cfc_order=(0, 1))
    gnight, keep_night = api.make_columns(inp.night, MOL_ORDER, cfc_order=(0, 1))
    gaer_sw, keep_sw = api.make_aerosols(lw=None, sw=(inp.xa[1], inp.fa[1]))
    gaer, keep_aer = api.make_aerosols(lw=(inp.xa[0], inp.fa[0]), sw=(inp.xa[1], inp.fa[1]))
    clouds = {S: make(inp.tables, pick(inp.cl, subcolumns=range(S))) for S in (1, S_MAX)}
    out = {}
    for form, spectral in FORMS:
        for mode, user_level, two_sweeps in MODES:
            if two_sweeps and spectral:
                continue

            def put(run, arrays):
                for k, a in arrays.items():
                    out[f"{form}.{mode}.{run}.{k}"] = np.array(a, copy=True)

            with environment(**({"GRT_SW_TWO_SWEEPS": "1"} if two_sweeps else {})):
                pipe = api.Pipeline(None, go_sw, NCOL, user_level, None, inp.alb, solar, spectral=spectral)
                shortwave_runs(inp, pipe, spectral, gcols, gnight, clouds, gaer_sw, put)
                pipe.destroy()
                pipe = api.Pipeline(go_lw, go_sw, NCOL, user_level, inp.emis, inp.alb, solar, spectral=spectral)
                tile_runs(inp, pipe, gcols, clouds, gaer, put)
                pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
    return out
