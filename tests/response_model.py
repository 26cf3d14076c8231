"""grt_pipeline_run_sky_weighted's definition restated in numpy: from a level's spectral rows [V][n] the sums
X_k = sum_i (t_i r_k(i)) F_i under responses (first, weights_list), t_i the trapezoid weight of the whole band, and the
actinic row (S/mu0 + (D - S)/mu_dif) + U/mu_dif.  The oracle's solvers supply the upward and downward spectra,
direct_beam_model.direct_beam the beam; a cloud set's spectra are the mean over its draws in order (the sums are linear in
them).  test_response_model.py holds it against the oracle's own trapezoid and against the case where the actinic flux is
the beam's alone."""
import numpy as np

from aerosol_model import oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from direct_beam_model import direct_beam
from pipeline_support import _solve, limits

MU_DIF = 0.5                     # driver.c:110


def trapezoid_weights(n, dw):
    """t_i: dw, dw/2 at the points 0 and n - 1."""
    t = np.full(n, float(dw))
    t[0] = t[-1] = 0.5 * dw
    return t


def weighted_rows(rows, dw, first, weights_list):
    """[R][V]: X_k of every level of rows [V][n], each term formed as F (t r)."""
    rows = np.asarray(rows, dtype=np.float64)
    t = trapezoid_weights(rows.shape[1], dw)
    out = np.empty((len(weights_list), rows.shape[0]))
    for k, (f, r) in enumerate(zip(first, weights_list)):
        r = np.asarray(r, dtype=np.float64)
        span = slice(int(f), int(f) + r.size)
        assert 0 <= span.start and span.stop <= rows.shape[1]
        out[k] = np.sum(rows[:, span] * (t[span] * r), axis=1)
    return out


def actinic(direct, down, up, mu0, mu_dif=MU_DIF):
    """The actinic flux from three finished rows, in the documented order."""
    return (direct / mu0 + (down - direct) / mu_dif) + up / mu_dif


def mean_in_order(arrays):
    """The draws 0 .. S - 1 added in order, then one division by S."""
    total = arrays[0].copy()
    for a in arrays[1:]:
        total = total + a
    return total / float(len(arrays))


def oracle_spectral_sets(orc, lib, band, col, lw, tables, liquid, ice, thickness, x, optics, emis, alb, solar):
    """The four sets of one column and band, in bit order (clean, aerosol, cloud, both), each a dict of the level spectra
    up, dn [V][n] and -- shortwave -- direct [V][n]: the objects combined as test_gpu_pipeline_sky.py's oracle_sky combines
    them (add_optics of gas, Rayleigh, then the aerosol, then liquid and ice), the oracle's solver and the restated beam per
    draw, the mean over the draws in order.  liquid / ice [S][3][B][L], optics [3][L][NA] on the grid x."""
    L = col["p"].size - 1
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    aer = oracle_aerosol_optics(orc, band, x, optics)
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
        up, dn = _solve(orc, band, col, lw, tau, omega, g, emis, alb, solar)
        out = dict(up=up, dn=dn)
        if not lw:
            out["direct"] = direct_beam(tau, omega, g, col["mu0"], col["tsi"], solar)
        return out

    def mean(results):
        return {k: mean_in_order([r[k] for r in results]) for k in results[0]}

    aerosol = [(aer[0], aer[1], aer[2])]
    clouds = [[(d[0], d[1], d[2]), (d[3], d[4], d[5])] for d in draws]
    return (mean([one([])]), mean([one(aerosol)]), mean([one(c) for c in clouds]), mean([one(aerosol + c) for c in clouds]))


def weighted_set(spectra, dw, first, weights_list, mu0=None):
    """One set's weighted rows [R][V] per row group from its level spectra (oracle_spectral_sets): up, dn and -- where the
    set has a beam -- direct and actinic (mu0: the column's)."""
    out = {k: weighted_rows(spectra[k], dw, first, weights_list) for k in spectra}
    if "direct" in out:
        out["actinic"] = actinic(out["direct"], out["dn"], out["up"], mu0)
    return out
