"""The cases of tests/test_gpu_lw_point_bits.py and of tests/golden/make_lw_point_bits.py, which recorded their expected
bits: every entry point of the batched pipeline that reaches a longwave kernel of k_longwave.hip, on a pipeline with a
longwave band alone, in both of its forms (fused, and keep_spectra = 1) wherever the entry point takes both.

The shapes are the smallest that still reach every line of those kernels: a grid of 129 points (two workgroups of 128, the
second with one live lane), 2 columns, 4 levels with the user level inside, 3 cloud draws, an aerosol object on a two-point
grid, 5 viewing angles (chunks of 4 + 1) and 3 channels -- one inside one wave, one across the workgroup boundary, one the
last point alone.  run_all() gives every output by name; the names are the fixture's keys."""
import os

import numpy as np

from aerosol_model import aerosol_fields
from cloud_model import synthetic_tables
from grtcode_amd import api, synthetic as syn
from pipeline_support import ICE_EDGES, LIQUID_EDGES, SETS, few_layer_clouds, make, pick, surface
from scenario import MOL_ORDER, Band

N, V, NCOL, S_MAX, USER_LEVEL = 129, 4, 2, 3, 2
W0 = 100.0
SEED = 20261021
SECANTS = np.array([[1.0, 1.5, 14.402613260847248, 1e3, 2.25], [3.0302159969901132, 1.0, 1e3, 1.5, 1.0746123148178333]])
#: (first point, weights): inside one wave; across the boundary of the two workgroups; the last point alone
CHANNELS = ((10, np.array([0.25, 0.5, 1.0, 2.0, 1.0, 0.5, -0.25])), (122, np.array([0.5, 1.0, 1.5, 2.0, 1.5, 1.0, 0.5])),
            (N - 1, np.array([1.0])))
ALL = api.GRT_SKY_ALL
LW_EDGES = np.array([0, 40, 127, 128])          # three bins: one inside a workgroup, one up to its edge, one across it


def cloud_tables(root):
    """pipeline_support.tables' synthetic parametrisations"""
    os.makedirs(os.path.join(root, "i"), exist_ok=True)
    _, t = synthetic_tables(root, seed=4, band_edges=LIQUID_EDGES)
    _, ti = synthetic_tables(os.path.join(root, "i"), seed=9, band_edges=ICE_EDGES)
    t["ice"] = ti["ice"]
    t["liquid"]["Band_limits_upr"][1] = np.float64(np.float32(150.0))
    return t


class Inputs:
    """Everything the runs need that is made on the host: the band's files under root, columns, S_MAX draws of clouds,
    the aerosol fields, the surface."""

    def __init__(self, root):
        self.band = Band(os.path.join(root, "lw"), W0, W0 + (N - 1) * 1.0, 1.0, 300)
        assert self.band.nw == N
        self.tables = cloud_tables(os.path.join(root, "clouds"))
        self.cols = [syn.profile(900 + V + c, V) for c in range(NCOL)]
        self.emis, _ = surface(N, N + V)
        self.xa = np.array([W0 + 0.3 * (N - 1), W0 + 0.8 * (N - 1)])        # points below, between and above the two
        self.fa = aerosol_fields(NCOL, V - 1, self.xa, SEED, lw=True)
        draws = [few_layer_clouds(self.cols, self.tables, SEED % 1000 + j) for j in range(S_MAX)]
        self.cl = {k: (np.stack([d[k] for d in draws], axis=1) if k in SETS else draws[0][k]) for k in draws[0]}


def run_all(inp, device):
    """-> {name: array}: every output of every case.  `device` from api.create_device; deterministic mode is the
    caller's to set."""
    go, _ = inp.band.gas_optics(device, V)
    gcols, keep_cols = api.make_columns(inp.cols, MOL_ORDER, cfc_order=(0, 1))
    gaer, keep_aer = api.make_aerosols(lw=(inp.xa, inp.fa), sw=None)
    clouds = {S: make(inp.tables, pick(inp.cl, subcolumns=range(S))) for S in (1, S_MAX)}
    first = [f for f, _ in CHANNELS]
    weights = [w for _, w in CHANNELS]
    centers = [W0 + f + 0.5 * (w.size - 1) for f, w in CHANNELS]
    gch, keep_ch = api.make_channels(first, weights, centers)
    NC = len(CHANNELS)
    A = SECANTS.shape[1]
    out = {}

    def put(prefix, arrays):
        for k, a in arrays.items():
            out[prefix + "." + k] = np.array(a, copy=True)

    for spectral in (False, True):
        form = "spectra" if spectral else "fused"
        pipe = api.Pipeline(go, None, NCOL, USER_LEVEL, inp.emis, None, None, spectral=spectral)
        for S in (1, S_MAX):
            gsky, keep_sky = api.make_sky(clouds[S][0], gaer, S, ALL)
            n = keep_sky["nsets"]
            assert n == 4
            # run_sky: all four sets, six-row and profile form
            pipe.run_sky(gcols, gsky, profiles=False)
            put(f"{form}.S{S}.sky", dict(fluxes=pipe.sky_fluxes(NCOL, n)[..., :6]))
            pipe.run_sky(gcols, gsky, profiles=True)
            prof = pipe.sky_profiles(NCOL, n)
            put(f"{form}.S{S}.sky_profiles", {k: prof[k] for k in ("lw_up", "lw_down", "lw_heating")})
            put(f"{form}.S{S}.sky_profiles", dict(fluxes=prof["fluxes"][..., :6]))
        # run_sky_jacobian
        pipe.run_sky_jacobian(gcols, gsky, profiles=False)
        put(f"{form}.jacobian", dict(fluxes=pipe.sky_fluxes(NCOL, n)[..., :6], rows=pipe.sky_jacobian_fluxes(NCOL, n)))
        pipe.run_sky_jacobian(gcols, gsky, profiles=True)
        jac = pipe.sky_jacobian_profiles(NCOL, n)
        put(f"{form}.jacobian_profiles", dict(lw_up=pipe.sky_profiles(NCOL, n)["lw_up"], rows=jac["jacobian"],
                                              levels=jac["jacobian_levels"]))
        # run_sky_weighting: three draws; then one draw with the radiances and brightness temperatures at every point
        pipe.run_sky_weighting(gcols, gsky, SECANTS, gch, brightness=True)
        put(f"{form}.S{S_MAX}.weighting",
            dict(radiances=pipe.sky_radiances(NCOL, n, A), channels=pipe.sky_channel_radiances(NCOL, n, A, NC),
                 channel_tb=pipe.sky_channel_brightness(NCOL, n, A, NC),
                 transmittances=pipe.sky_channel_transmittances(NCOL, n, A, NC),
                 contributions=pipe.sky_channel_contributions(NCOL, n, A, NC), fluxes=pipe.sky_fluxes(NCOL, n)[..., :6]))
        gsky1, keep_sky1 = api.make_sky(clouds[1][0], gaer, 1, ALL)
        pipe.run_sky_weighting(gcols, gsky1, SECANTS, gch, brightness=True, spectral=True)
        put(f"{form}.S1.weighting",
            dict(radiances=pipe.sky_radiances(NCOL, n, A), spectral=pipe.sky_spectral_radiances(NCOL, n, A),
                 channels=pipe.sky_channel_radiances(NCOL, n, A, NC), channel_tb=pipe.sky_channel_brightness(NCOL, n, A, NC),
                 transmittances=pipe.sky_channel_transmittances(NCOL, n, A, NC),
                 contributions=pipe.sky_channel_contributions(NCOL, n, A, NC)))
        pipe.run_sky_radiances(gcols, gsky1, SECANTS, brightness=True, fluxes=False)
        put(f"{form}.S1.radiances", dict(brightness=pipe.sky_brightness(NCOL, n, A)))
        # run_band_profiles and run_spectral, each with clouds
        pipe.run_band_profiles(gcols, clouds[1][0], lw_edges=LW_EDGES)
        bp = pipe.band_profiles(NCOL)
        put(f"{form}.band_profiles", {k: bp[k] for k in ("lw_up", "lw_down", "lw_heating")})
        pipe.run_spectral(gcols, clouds[1][0], lw_edges=LW_EDGES)
        sp = pipe.spectral(NCOL)
        put(f"{form}.spectral", dict(lw=sp["lw"], lw_bins=sp["lw_bins"]))
        if spectral:
            pipe.run(gcols)
            put(f"{form}.run", dict(fluxes=pipe.fluxes(NCOL)[:, :6]))
        pipe.destroy()
    go.destroy()
    return out
