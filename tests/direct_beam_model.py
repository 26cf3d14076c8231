"""The direct beam of the shortwave solver, restated in numpy for grt_pipeline_run_sky_direct's tests: from a set's
combined tau, omega, g [L][n] the delta-scaling of shortwave.c:86-89, T_pure of every layer (meador_weaver_1980,
shortwave.c:114-168, with the optical-depth clamp of :137-145 and the tp <= 1 case), the running product from the top
(dir_beam, :306 and :323), the scaling by solar_flux mu0 and the total solar irradiance (:401-405, :447-451), the oracle's
trapezoid and, for cloud sets, the mean over the subcolumns in order.  test_direct_beam_model.py holds the restatement
against the oracle's own downward flux where the two are the same number (no scattering, a black surface)."""
import numpy as np

from aerosol_model import oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from pipeline_support import limits

MAX_EXP_ARG = 700.0          # grtcode_config.h:41


def pure_transmission(tau, omega, g, mu):
    """T_pure [L][n] of layers tau, omega, g [L][n] for a beam of cosine mu."""
    tau, omega, g = (np.asarray(a, dtype=np.float64) for a in (tau, omega, g))
    gs = g / (g + 1.0)                                                     # shortwave.c:86-89
    f = g * g
    os = (1.0 - f) * omega / (1.0 - omega * f)
    ts = tau * (1.0 - omega * f)
    gamma1 = 0.25 * (7.0 - os * (4.0 + 3.0 * gs))                          # :226-227
    gamma2 = -0.25 * (1.0 - os * (4.0 - 3.0 * gs))
    with np.errstate(invalid="ignore", over="ignore"):
        k = np.sqrt(gamma1 * gamma1 - gamma2 * gamma2)
        t = ts.copy()                                                      # :137-145
        first = (1.0 / mu > k) & (ts / mu > MAX_EXP_ARG)
        second = ~first & (ts * k > MAX_EXP_ARG)
        t = np.where(first, MAX_EXP_ARG * mu, np.where(second, MAX_EXP_ARG / k, t))
        tp = np.exp(t / mu)
        scattering = np.where(tp <= 1.0, 1.0, np.exp(-t / mu))             # :149-168
        return np.where(os <= 0.0, np.exp(-ts / mu), scattering)           # :114-122


def direct_beam(tau, omega, g, mu0, tsi, solar):
    """The direct beam at every level and grid point, [V][n], levels top first, W m-2 per cm-1."""
    tp = pure_transmission(tau, omega, g, mu0)
    beam = np.ones((tp.shape[0] + 1, tp.shape[1]))
    for j in range(tp.shape[0]):                                           # the running product, layer by layer
        beam[j + 1] = beam[j] * tp[j]
    return tsi * (beam * (np.asarray(solar, dtype=np.float64) * mu0))


def three(direct_int, user_level):
    """The three rows of GrtDirectBeam.direct_fluxes_dev from the integrated levels [V]."""
    return np.array([direct_int[0], direct_int[-1], direct_int[user_level] if user_level >= 0 else 0.0])


def oracle_direct_sets(orc, lib, band, col, tables, liquid, ice, thickness, x, optics, alb, solar):
    """The four sets of one column of the shortwave band, in bit order (clean, aerosol, cloud, both), each a dict of
    direct, up_int, dn_int [V]: the objects combined exactly as test_gpu_pipeline_sky.py's oracle_sky combines them
    (add_optics of gas, Rayleigh, then the aerosol, then liquid and ice), per subcolumn the restatement above and the
    oracle's solver, each integrated with the oracle's trapezoid, then the mean over the subcolumns s = 0 .. S - 1 in
    order.  liquid / ice [S][3][B][L] (None: no cloud sets asked for: two sets), optics [3][L][NA] on the grid x."""
    L = col["p"].size - 1
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    aer = oracle_aerosol_optics(orc, band, x, optics)
    draws = []
    if liquid is not None:
        B = liquid.shape[2]
        w = driver_limits(band.w0, band.dw, band.nw)
        (llo, lhi), (ilo, ihi) = limits(tables, "liquid"), limits(tables, "ice")
        maps = (band_map(llo, lhi, B, B, w), band_map(ilo, ihi, ilo.size, B, w))
        draws = [grid_optics(liquid[j], ice[j], thickness, maps) for j in range(liquid.shape[0])]

    def one(objects):
        taus, omegas, gs = ([tau_gas, tr], [z, om_r], [z, g_r])
        for t, o, g in objects:
            taus, omegas, gs = taus + [t], omegas + [o], gs + [g]
        tau, omega, g = orc.add_optics(taus, omegas, gs)
        up, dn = orc.sw_fluxes(omega, g, tau, col["mu0"], 0.5, alb, alb, col["tsi"], solar)
        beam = direct_beam(tau, omega, g, col["mu0"], col["tsi"], solar)
        return tuple(np.array([orc.integrate_row(r, band.dw) for r in a]) for a in (beam, up, dn))

    def mean(results):
        out = []
        for k in range(3):
            total = results[0][k].copy()
            for r in results[1:]:
                total = total + r[k]
            out.append(total / float(len(results)))
        return dict(direct=out[0], up_int=out[1], dn_int=out[2])

    aerosol = [(aer[0], aer[1], aer[2])]
    sets = [mean([one([])]), mean([one(aerosol)])]
    if draws:
        clouds = [[(d[0], d[1], d[2]), (d[3], d[4], d[5])] for d in draws]
        sets.append(mean([one(c) for c in clouds]))
        sets.append(mean([one(aerosol + c) for c in clouds]))
    return tuple(sets)
