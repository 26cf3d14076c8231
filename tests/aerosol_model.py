"""Helpers of the aerosol tests: synthetic aerosol fields on a coarse wavenumber grid, a NumPy restatement of the
reference's interpolate2 / linear_sample onto a spectral grid (utilities.c:149-222, :235-246), and the oracle's
column-by-column restatement of the aerosol pass (driver.c:426-472)."""
import numpy as np

# an irregular aerosol grid that starts inside the tests' longwave band (1-400 cm-1) and ends inside their shortwave band
# (1-5000 cm-1): both bands have points with and without aerosol
AEROSOL_GRID = np.array([150.5, 210.0, 333.0, 400.0, 655.0, 910.25, 1480.0, 2100.0, 2790.0, 3300.0, 3950.5, 4405.0])


def aerosol_fields(ncol, L, grid, seed, lw):
    """[ncol][3][L][NA]: layer optical depths decaying with height (index 0 is the top), single-scattering albedo
    0.85-0.99 in the shortwave and 0.2-0.6 in the longwave, asymmetry 0.5-0.8; all vary along the aerosol grid and between
    the columns."""
    rng = np.random.default_rng(seed)
    na = grid.size
    out = np.zeros((ncol, 3, L, na))
    height = np.exp(-3.0 * (L - 1 - np.arange(L)) / max(L - 1, 1))[:, None]           # 1 at the surface
    for c in range(ncol):
        spectral = (0.5 + rng.random(na)) * (grid / grid[0]) ** (-0.3 if lw else 0.6)   # Angstrom-like, either sign
        out[c, 0] = (0.15 + 0.1 * c) * height * spectral[None, :] * (0.8 + 0.4 * rng.random((L, na)))
        lo, hi = (0.2, 0.6) if lw else (0.85, 0.99)
        out[c, 1] = lo + (hi - lo) * rng.random((L, na))
        out[c, 2] = 0.5 + 0.3 * rng.random((L, na))
    return out


def interval_map(w0, dw, nw, x):
    """The interval j (x[j] < w <= x[j+1]) of each grid point w0 + i dw, -1 for w <= x[0] and w > x[-1]."""
    w = w0 + np.arange(nw, dtype=np.float64) * dw
    j = np.searchsorted(x, w, side="left") - 1          # x[j] < w <= x[j+1]
    j[(w <= x[0]) | (w > x[-1])] = -1
    return j.astype(np.int32), w


def slope_tables(x, optics):
    """optics [ncol][3][L][NA] -> [ncol][3][NA-1][2][L]: linear_sample's m = (y1 - y0)/(x1 - x0), b = y0 - m x0."""
    m = (optics[..., 1:] - optics[..., :-1]) / (x[1:] - x[:-1])
    b = optics[..., :-1] - m * x[:-1]
    return np.ascontiguousarray(np.stack([m, b], axis=-1).transpose(0, 1, 3, 4, 2))    # [c][p][j][2][L]


def numpy_interp(w0, dw, nw, x, y):
    """interpolate2(..., linear_sample, NULL) into a zero-filled array: m w + b where an interval holds w, 0 elsewhere."""
    j, w = interval_map(w0, dw, nw, x)
    m = (y[1:] - y[:-1]) / (x[1:] - x[:-1])
    b = y[:-1] - m * x[:-1]
    jj = np.where(j < 0, 0, j)
    return np.where(j < 0, 0.0, m[jj] * w + b[jj])


def oracle_aerosol_optics(orc, band, x, optics):
    """One column's aerosol object on the band's grid, [3][L][nw]: the oracle's interp_to_grid per layer and property
    into zero-filled arrays."""
    L = optics.shape[1]
    out = np.zeros((3, L, band.nw))
    for p in range(3):
        for l in range(L):
            out[p, l] = orc.interp_to_grid(band.w0, band.dw, band.nw, x, optics[p, l], constant_extrap=False)
    return out


def oracle_aerosol_column(orc, lib, band, col, lw, x, optics, emis=None, alb=None, solar=None, user_level=-1):
    """driver.c:426-472 for one column and band: add_optics of {gas, Rayleigh, aerosol}, the solver, the -integrated rows
    and every level's integral.  x None: no aerosol in this band (an aerosol of zeros)."""
    L = col["p"].size - 1
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    aer = oracle_aerosol_optics(orc, band, x, optics) if x is not None else np.zeros((3, L, band.nw))
    tau, omega, g = orc.add_optics([tau_gas, tr, aer[0]], [z, om_r, aer[1]], [z, g_r, aer[2]])
    if lw:
        up, dn = orc.lw_fluxes(band.w0, band.dw, col["t_surf"], col["t_layer"], col["t"], tau, omega, emis)
    else:
        up, dn = orc.sw_fluxes(omega, g, tau, col["mu0"], 0.5, alb, alb, col["tsi"], solar)
    up_int = np.array([orc.integrate_row(up[k], band.dw) for k in range(L + 1)])
    dn_int = np.array([orc.integrate_row(dn[k], band.dw) for k in range(L + 1)])
    u = user_level
    integ = np.array([up_int[0], up_int[L], up_int[u] if u >= 0 else 0.0, dn_int[0], dn_int[L], dn_int[u] if u >= 0 else 0.0])
    return dict(tau=tau, omega=omega, g=g, up=up, dn=dn, up_int=up_int, dn_int=dn_int, integ=integ, aerosol=aer)
