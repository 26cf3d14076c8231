"""What the tests of grt_pipeline_run_sky_tiles share: the tiles of a batch (knots with 0 and 1 among them, temperatures,
fractions), each tile's expected rows on a band's grid (surface_support.host_rows: the library's host interpolate_to_grid),
the oracle's optics of a set and cloud draw of one column -- formed once and solved per tile over the tile's rows and
temperature --, the mean kernel's fold in numpy, and the call that returns both outputs of a run as one dict."""
import numpy as np

from aerosol_model import oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from grtcode_amd import api
from pipeline_support import _integrals, limits, surface
from sky_zenith_support import NAMES
from surface_support import host_rows


def tile_knots(band, ns, ncol, T, seed):
    """A surface grid that starts and ends inside the band, and knot values [ncol][T][ns] in [0, 1] for (emissivity, direct
    albedo, diffuse albedo): pipeline_support.surface's values -- 0 and 1 at both ends and, from four knots on, in the
    middle -- with the tiles of a column apart from each other between them."""
    span = (band.nw - 1) * band.dw
    x = np.linspace(band.w0 + 0.2 * span, band.w0 + 0.7 * span, ns)
    out = np.empty((3, ncol, T, ns))
    for c in range(ncol):
        for t in range(T):
            out[0, c, t], out[1, c, t] = surface(ns, seed + 31 * c + t)
            out[2, c, t] = surface(ns, seed + 31 * c + t + 500)[1]
            # (two knots: both are ends.  The tiles still differ: the last knot is the tile's own)
            if ns == 2:
                out[0, c, t, 1] = 1.0 - 0.5 * t / T
                out[1, c, t, 1] = 0.5 * t / T
                out[2, c, t, 1] = 0.25 * t / T
    return x, out[0], out[1], out[2]


def tile_temperatures(cols, T):
    """[ncol][T] K: around each column's own surface temperature, every tile another one."""
    return np.array([[col["t_surf"] + 3.0 * ((2 * t + c) % 5 - 2) for t in range(T)] for c, col in enumerate(cols)])


def tile_fractions(ncol, T, kind):
    """None; "zero": sums to one with a zero entry where T allows one; "free": does not sum to one."""
    if kind is None:
        return None
    f = np.array([[1.0 + ((c + 2 * t) % 3) for t in range(T)] for c in range(ncol)], dtype=np.float64)
    if kind == "zero":
        if T > 1:
            for c in range(ncol):
                f[c, (c + 1) % T] = 0.0
        return f / f.sum(axis=1, keepdims=True)
    return 0.375 * f


def tile_rows(lib, band, x, values):
    """[ncol][T][n]: every tile's knots [ncol][T][NS] on the band's grid, as driver.c:101-117 puts a column's there."""
    grid = api.create_spectral_grid(band.w0, band.wn, band.dw)
    ncol, T, ns = values.shape
    return host_rows(lib, grid, x, values.reshape(ncol * T, ns)).reshape(ncol, T, -1)


def set_optics(name, orc, lib, band, col, tables, liquid, ice, thickness, x, optics):
    """The oracle's tau, omega, g of one of the four sets of one column and band, one triple per cloud draw (one for a set
    without clouds): add_optics of {gas, Rayleigh[, aerosol][, liquid, ice]} in the reference driver's order."""
    L = col["p"].size - 1
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    taus, omegas, gs = [tau_gas, tr], [z, om_r], [z, g_r]
    if name in ("aerosol", "both"):
        aer = oracle_aerosol_optics(orc, band, x, optics)
        taus, omegas, gs = taus + [aer[0]], omegas + [aer[1]], gs + [aer[2]]
    if name in ("clean", "aerosol"):
        return [orc.add_optics(taus, omegas, gs)]
    B = liquid.shape[2]
    w = driver_limits(band.w0, band.dw, band.nw)
    (llo, lhi), (ilo, ihi) = limits(tables, "liquid"), limits(tables, "ice")
    maps = (band_map(llo, lhi, B, B, w), band_map(ilo, ihi, ilo.size, B, w))
    out = []
    for j in range(liquid.shape[0]):
        lt, lo, lg, it, io, ig = grid_optics(liquid[j], ice[j], thickness, maps)
        out.append(orc.add_optics(taus + [lt, it], omegas + [lo, io], gs + [lg, ig]))
    return out


def oracle_tile(orc, band, col, lw, draws, t_surf, emis, adir, adif, solar):
    """One tile of one column, set and band: the reference's solver over each draw's optics with the tile's rows and
    temperature; the draws' fluxes summed and divided by their number, every level integrated: up_int, dn_int [V]."""
    up_sum = dn_sum = None
    for tau, omega, g in draws:
        if lw:
            up, dn = orc.lw_fluxes(band.w0, band.dw, t_surf, col["t_layer"], col["t"], tau, omega, emis)
        else:
            up, dn = orc.sw_fluxes(omega, g, tau, col["mu0"], 0.5, adir, adif, col["tsi"], solar)
        up_sum = up.copy() if up_sum is None else up_sum + up
        dn_sum = dn.copy() if dn_sum is None else dn_sum + dn
    up_sum, dn_sum = up_sum / float(len(draws)), dn_sum / float(len(draws))
    up_int, dn_int = _integrals(orc, band, up_sum, dn_sum)
    return dict(up_int=up_int, dn_int=dn_int)


def fold_tiles(fraction, tiles):
    """The mean over axis 2 of tiles [ncol][nsets][T][12] in the mean kernel's order: with fractions [ncol][T] sum f_t F_t,
    each product rounded, the tiles t = 0 .. T - 1 in order; without, the sum and one division by T."""
    T = tiles.shape[2]
    f = np.ones(tiles.shape[:1] + (T,)) if fraction is None else fraction
    w = f.reshape(f.shape[0], 1, T, 1)
    acc = w[:, :, 0] * tiles[:, :, 0]
    for t in range(1, T):
        acc = acc + w[:, :, t] * tiles[:, :, t]
    return acc if fraction is not None else acc / float(T)


def run_sky_tiles(pipe, gcols, gclouds, gaer, S, sets, gtiles, ncol):
    """grt_pipeline_run_sky_tiles -> dict: "fluxes" [ncol][nsets][12] and "tiles" [ncol][nsets][T][12]."""
    gsky, keep = api.make_sky(gclouds, gaer, S, sets)
    pipe.run_sky_tiles(gcols, gsky, gtiles)
    fluxes, tiles = pipe.sky_tile_fluxes(ncol, keep["nsets"], gtiles.num_tiles)
    return dict(fluxes=fluxes, tiles=tiles)


__all__ = ["NAMES", "fold_tiles", "oracle_tile", "run_sky_tiles", "set_optics", "tile_fractions", "tile_knots", "tile_rows",
           "tile_temperatures"]
