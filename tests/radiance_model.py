"""Longwave radiances at viewing angles restated in numpy for grt_pipeline_run_sky_radiances' tests.  The four streams of the
reference's longwave solver are radiances at the Gauss-Legendre secants -c1[s] (longwave.c:160-168); a radiance at secant
m is the same recurrence with c1[s] replaced by -m.  Per grid point, in lw_kernel's expressions and order: t_j = tau_j (1 -
omega_j) (longwave.c:252), e_j = exp(min((-m) t_j, 700)); downward from I = 0, I <- (1 - e_j) P_j + I e_j with P_j =
effective_planck(B(T_layer j), B(T_level j + 1), t_j): the downward radiance at the surface; the surface, I <- emis
B(T_surf) + (1 - emis) I (:202); upward with P_j from T_level j: the upward radiance at the top.  W m-2 sr-1 per cm-1.
Then the oracle's trapezoid and, for cloud sets, the mean over the draws in order.  test_radiance_model.py holds the
restatement against the oracle's own solver: the c2-weighted sum over the four stream secants is its flux."""
import numpy as np

from aerosol_model import oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from lw_jacobian_model import MAX_EXP_ARG, PLANCK_C1, PLANCK_C2, STREAM_C1, STREAM_C2, planck
from pipeline_support import limits

STREAM_SECANTS = tuple(-c for c in STREAM_C1)


def effective_planck(bc, be, tau):
    """longwave.c:100-118 with the two Planck values supplied by the caller."""
    a, b = 0.193, 0.013
    return (bc + (a * tau + b * tau * tau) * be) / (1.0 + a * tau + b * tau * tau)


def radiances(tau, omega, emis, t_surf, t_layers, t_levels, w, secants):
    """-> [A][2][n]: per secant the upward radiance at the top and the downward one at the surface, from a set's combined
    tau, omega [L][n], the emissivity [n], the temperatures and the grid's wavenumbers w [n]."""
    tau, omega, emis, w = (np.asarray(a, dtype=np.float64) for a in (tau, omega, emis, w))
    t = tau * (1.0 - omega)                                                # longwave.c:252
    L, n = t.shape
    bs = planck(t_surf, w)
    down_p = [effective_planck(planck(t_layers[j], w), planck(t_levels[j + 1], w), t[j]) for j in range(L)]
    up_p = [effective_planck(planck(t_layers[j], w), planck(t_levels[j], w), t[j]) for j in range(L)]
    out = np.zeros((len(secants), 2, n))
    for k, m in enumerate(secants):
        c1 = -float(m)
        ext = [np.exp(np.minimum(c1 * t[j], MAX_EXP_ARG)) for j in range(L)]
        beam = np.zeros(n)
        for j in range(L):
            beam = (1.0 - ext[j]) * down_p[j] + beam * ext[j]
        out[k, 1] = beam
        beam = emis * bs + (1 - emis) * beam
        for j in range(L - 1, -1, -1):
            beam = (1.0 - ext[j]) * up_p[j] + beam * ext[j]
        out[k, 0] = beam
    return out


def brightness(rad, w):
    """planck() solved for T: c2 w / log1p(c1 w^3 / I), +0.0 where I <= 0; rad [..][n], w [n]."""
    rad = np.asarray(rad, dtype=np.float64)
    w = np.broadcast_to(np.asarray(w, dtype=np.float64), rad.shape)
    out = np.zeros(rad.shape)
    lit = rad > 0.0
    out[lit] = PLANCK_C2 * w[lit] / np.log1p((PLANCK_C1 * w[lit] * w[lit] * w[lit]) / rad[lit])
    return out


def stream_sum(four):
    """((0 + c2[0] R_0) + c2[1] R_1) + c2[2] R_2) + c2[3] R_3 of radiances at the four stream secants, four [4][..]."""
    f = np.zeros(np.asarray(four[0]).shape)
    for s in range(4):
        f = f + STREAM_C2[s] * four[s]
    return f


def trapezoid(orc, rows, dw):
    """The oracle's trapezoid (driver.c:302-326) of every row of rows [..][n] -> [..]."""
    rows = np.asarray(rows)
    flat = rows.reshape(-1, rows.shape[-1])
    return np.array([orc.integrate_row(r, dw) for r in flat]).reshape(rows.shape[:-1])


def oracle_radiance_sets(orc, lib, band, col, tables, liquid, ice, thickness, x, optics, emis, secants):
    """The four sets of one column of the longwave band, in bit order (clean, aerosol, cloud, both), each a dict of
    rad [A][2][n] (the first draw's), integ [A][2] (the mean over the draws), largest [A][2] (each row's largest value at a
    point, over the draws), up, dn [V][n] (the oracle's own spectral fluxes of the first draw): the objects combined
    exactly as lw_jacobian_model.oracle_jacobian_sets combines them (add_optics of gas, Rayleigh, then the aerosol, then liquid and ice), per draw the restatement above integrated with
    the oracle's trapezoid, then the mean over the draws s = 0 .. S - 1 in order.  liquid / ice [S][3][B][L] (None: no
    cloud sets asked for: two sets), optics [3][L][NA] on the grid x (None: no aerosol sets: the clean set and, with
    clouds, the cloud set)."""
    L = col["p"].size - 1
    w = band.w0 + np.arange(band.nw) * band.dw                             # longwave.c:246
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    draws = []
    if liquid is not None:
        B = liquid.shape[2]
        lim = driver_limits(band.w0, band.dw, band.nw)
        (llo, lhi), (ilo, ihi) = limits(tables, "liquid"), limits(tables, "ice")
        maps = (band_map(llo, lhi, B, B, lim), band_map(ilo, ihi, ilo.size, B, lim))
        draws = [grid_optics(liquid[j], ice[j], thickness, maps) for j in range(liquid.shape[0])]

    def one(objects):
        taus, omegas, gs = ([tau_gas, tr], [z, om_r], [z, g_r])
        for t, o, g in objects:
            taus, omegas, gs = taus + [t], omegas + [o], gs + [g]
        tau, omega, g = orc.add_optics(taus, omegas, gs)
        up, dn = orc.lw_fluxes(band.w0, band.dw, col["t_surf"], col["t_layer"], col["t"], tau, omega, emis)
        rad = radiances(tau, omega, emis, col["t_surf"], col["t_layer"], col["t"], w, secants)
        return dict(rad=rad, integ=trapezoid(orc, rad, band.dw), up=up, dn=dn)

    def mean(results):
        total = results[0]["integ"].copy()
        for r in results[1:]:
            total = total + r["integ"]
        largest = np.max([np.abs(r["rad"]).max(axis=-1) for r in results], axis=0)
        return dict(results[0], integ=total / float(len(results)) if len(results) > 1 else total, largest=largest)

    sets = [mean([one([])])]
    aerosol = []
    if optics is not None:
        aer = oracle_aerosol_optics(orc, band, x, optics)
        aerosol = [(aer[0], aer[1], aer[2])]
        sets.append(mean([one(aerosol)]))
    if draws:
        clouds = [[(d[0], d[1], d[2]), (d[3], d[4], d[5])] for d in draws]
        sets.append(mean([one(c) for c in clouds]))
        if optics is not None:
            sets.append(mean([one(aerosol + c) for c in clouds]))
    return tuple(sets)
