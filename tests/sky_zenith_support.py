"""What the tests of grt_pipeline_run_sky_zeniths share: the helpers test_gpu_pipeline_sky.py and
test_gpu_zenith_shapes.py keep inside their modules, restated (set positions, the aerosol inputs, the five-object oracle,
the angles of a batch, the mean kernel's fold), and the calls that return every output of a run as one dict."""
import numpy as np

from aerosol_model import oracle_aerosol_column, oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from grtcode_amd import api
from pipeline_support import _integrals, _solve, limits, oracle_column, oracle_subcolumns, six

CLEAN, AEROSOL, CLOUD, BOTH, ALL = (api.GRT_SKY_CLEAN, api.GRT_SKY_AEROSOL, api.GRT_SKY_CLOUD,
                                    api.GRT_SKY_CLOUD_AEROSOL, api.GRT_SKY_ALL)
BITS = (CLEAN, AEROSOL, CLOUD, BOTH)
NAMES = ("clean", "aerosol", "cloud", "both")          # the four sets in bit order
POOL = (1.0, 0.5, 0.05, 1e-3, 0.3, 0.999, 0.01, 0.7, 0.2)      # 0.5 = mu_dif; 1e-3 clamps tau/mu at 700 in most layers


def positions(sets):
    """Where each of the four sets lies among the packed sets of a run with these bits (the clean set always first)."""
    bits = [b for b in BITS if (sets | CLEAN) & b]
    return {NAMES[BITS.index(b)]: k for k, b in enumerate(bits)}


def aerosols_of(f, grids):
    return api.make_aerosols(lw=(grids[0], f[0]), sw=(grids[1], f[1]))


def angles(ncol, Z, night, chunk):
    """[ncol][Z] from POOL, another order per column; night: none, some (one per column, at another place in each),
    last_chunk (the samples of the last chunk of `chunk` angles, and only those) or all."""
    mu = np.array([[POOL[(k + 2 * c) % len(POOL)] for k in range(Z)] for c in range(ncol)])
    if night == "some":
        for c in range(ncol):
            mu[c, (c + 1) % Z] = (0.0, -0.3)[c % 2]
    elif night == "last_chunk":
        mu[:, ((Z - 1) // chunk) * chunk:] = -0.1
    elif night == "all":
        mu[:] = -0.5
    return mu


def under(cols, mu_k):
    """The columns under one angle each; a night sample's column runs under 1.0 and is not compared."""
    return [dict(col, mu0=(m if m > 0.0 else 1.0)) for col, m in zip(cols, mu_k)]


def fold(weights, rows):
    """sum_k w_k F_k over axis 2 of rows [ncol][nsets][Z][...] in the mean kernel's order: each product rounded, the angles
    k = 0 .. Z - 1 in order; weights [ncol][Z]."""
    w = weights.reshape(weights.shape[0], 1, weights.shape[1], *([1] * (rows.ndim - 3)))
    acc = w[:, :, 0] * rows[:, :, 0]
    for k in range(1, rows.shape[2]):
        acc = acc + w[:, :, k] * rows[:, :, k]
    return acc


def oracle_sky(orc, lib, band, col, lw, tables, liquid, ice, thickness, x, optics, emis=None, alb=None, solar=None):
    """One column and band with liquid / ice [S][3][B][L] and the aerosol optics [3][L][NA] on the grid x: per subcolumn
    add_optics of {gas, Rayleigh, aerosol, liquid, ice}, the solver; the fluxes summed, divided by S, every level
    integrated."""
    L, S, B = col["p"].size - 1, liquid.shape[0], liquid.shape[2]
    w = driver_limits(band.w0, band.dw, band.nw)
    (llo, lhi), (ilo, ihi) = limits(tables, "liquid"), limits(tables, "ice")
    maps = (band_map(llo, lhi, B, B, w), band_map(ilo, ihi, ilo.size, B, w))
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    aer = oracle_aerosol_optics(orc, band, x, optics)
    up_sum, dn_sum = np.zeros((L + 1, band.nw)), np.zeros((L + 1, band.nw))
    for j in range(S):
        lt, lo, lg, it, io, ig = grid_optics(liquid[j], ice[j], thickness, maps)
        tau, omega, g = orc.add_optics([tau_gas, tr, aer[0], lt, it], [z, om_r, aer[1], lo, io], [z, g_r, aer[2], lg, ig])
        up, dn = _solve(orc, band, col, lw, tau, omega, g, emis, alb, solar)
        up_sum += up
        dn_sum += dn
    up_sum /= float(S)
    dn_sum /= float(S)
    up_int, dn_int = _integrals(orc, band, up_sum, dn_sum)
    return dict(up_int=up_int, dn_int=dn_int)


def oracle_set(name, orc, lib, band, col, tables, liquid, ice, thickness, x, optics, emis, alb, solar):
    """The shortwave of one of the four sets of one column (under col["mu0"]): up_int, dn_int [V]."""
    if name == "clean":
        w = oracle_column(orc, lib, band, col, False, emis, alb, solar)
        up, dn = _integrals(orc, band, w["up"], w["dn"])
        return dict(up_int=up, dn_int=dn)
    if name == "aerosol":
        return oracle_aerosol_column(orc, lib, band, col, False, x, optics, emis, alb, solar)
    if name == "cloud":
        return oracle_subcolumns(orc, lib, band, col, False, tables, liquid, ice, thickness, emis, alb, solar)
    return oracle_sky(orc, lib, band, col, False, tables, liquid, ice, thickness, x, optics, emis, alb, solar)


def run_sky(pipe, gcols, gclouds, gaer, S, sets, ncol, profiles):
    """grt_pipeline_run_sky -> dict with sky_profiles()' keys, every array [ncol][nsets][..]; six rows: "fluxes" only."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    pipe.run_sky(gcols, gsky, profiles=profiles)
    if profiles:
        return pipe.sky_profiles(ncol, keep["nsets"])
    return dict(fluxes=pipe.sky_fluxes(ncol, keep["nsets"]))


def run_sky_zeniths(pipe, gcols, gclouds, gaer, S, sets, mu, weight, ncol, profiles):
    """grt_pipeline_run_sky_zeniths -> dict: "fluxes" [ncol][nsets][12] and "angle_fluxes" [ncol][nsets][Z][6]; profiles:
    sky_zenith_profiles()' keys."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    gz, keep_z = api.make_zeniths(mu, weight)
    pipe.run_sky_zeniths(gcols, gsky, gz, profiles=profiles)
    if profiles:
        return pipe.sky_zenith_profiles(ncol, keep["nsets"], mu.shape[1])
    fluxes, angle_fluxes = pipe.sky_zenith_fluxes(ncol, keep["nsets"], mu.shape[1])
    return dict(fluxes=fluxes, angle_fluxes=angle_fluxes)


def positive_zero(a):
    return bool(np.all(a == 0.0) and not np.any(np.signbit(a)))


__all__ = ["ALL", "AEROSOL", "BOTH", "CLEAN", "CLOUD", "NAMES", "aerosols_of", "angles", "fold", "oracle_set", "positions",
           "positive_zero", "run_sky", "run_sky_zeniths", "six", "under"]
