"""The surface-temperature Jacobian of the longwave solver, dF_up(level)/dT_surf, restated in numpy for
grt_pipeline_run_sky_jacobian's tests.  The surface enters each of the four streams once (longwave.c:202, I_s = emis
B(T_surf) + (1 - emis) I_s), every layer above multiplies the stream by exp(c1[s] t), t = tau (1 - omega) (:177-183,
:252), and nothing else in the upward sweep depends on T_surf: D_s = emis dB/dT at the surface, D_s <- D_s exp(c1[s] t_j)
layer by layer, J = sum_s c2[s] D_s, with dB/dT = B (x/T) e/(e - 1), x = c2 w/T, e = exp(x), 0 where planck_law clamps x
(:68-94).  Then the oracle's trapezoid and, for cloud sets, the mean over the subcolumns in order.
test_lw_jacobian_model.py holds the restatement against central differences of the oracle's own solver."""
import numpy as np

from aerosol_model import oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from pipeline_support import limits

MAX_EXP_ARG = 700.0          # grtcode_config.h:41
PLANCK_C1, PLANCK_C2 = 1.1910429526245744e-8, 1.4387773538277202          # longwave.c:70-71
STREAM_C1 = (-14.402613260847248, -3.0302159969901132, -1.4925584280108841, -1.0746123148178333)    # longwave.c:160-168
STREAM_C2 = (0.07587638482015649, 0.676114979733751, 1.3726594476601073, 1.0169418413757783)


def planck(T, w):
    """B(T, w) [n] as planck_law forms it, W m-2 per cm-1 per steradian-weight of the streams."""
    w = np.asarray(w, dtype=np.float64)
    e = np.exp(np.minimum(PLANCK_C2 * w / T, MAX_EXP_ARG))
    return (PLANCK_C1 * w * w * w) / (e - 1.0)


def planck_derivative(T, w):
    """dB/dT (T, w) [n]: B (x/T) e/(e - 1); 0 where planck_law clamps x."""
    w = np.asarray(w, dtype=np.float64)
    x = PLANCK_C2 * w / T
    e = np.exp(np.minimum(x, MAX_EXP_ARG))
    return np.where(x > MAX_EXP_ARG, 0.0, planck(T, w) * (x / T) * (e / (e - 1.0)))


def surface_jacobian(tau, omega, emis, t_surf, w):
    """dF_up/dT_surf at every level and grid point, [V][n], levels top first, W m-2 K-1 per cm-1, from a set's combined
    tau, omega [L][n], the emissivity [n] and the grid's wavenumbers w [n]."""
    tau, omega, emis = (np.asarray(a, dtype=np.float64) for a in (tau, omega, emis))
    t = tau * (1.0 - omega)                                                # longwave.c:252
    L = t.shape[0]
    seed = emis * planck_derivative(t_surf, w)
    D = [seed.copy() for _ in range(4)]
    out = np.zeros((L + 1, t.shape[1]))

    def flux():
        f = np.zeros(t.shape[1])
        for s in range(4):
            f = f + STREAM_C2[s] * D[s]
        return f

    out[L] = flux()
    for j in range(L - 1, -1, -1):
        for s in range(4):
            D[s] = D[s] * np.exp(np.minimum(STREAM_C1[s] * t[j], MAX_EXP_ARG))
        out[j] = flux()
    return out


def trapezoid(orc, rows, dw):
    """The oracle's trapezoid (driver.c:302-326) of every row of rows [V][n] -> [V]."""
    return np.array([orc.integrate_row(r, dw) for r in rows])


def three(jac_int, user_level):
    """The three rows of GrtSurfaceJacobian.jacobian_fluxes_dev from the integrated levels [V]."""
    return np.array([jac_int[0], jac_int[-1], jac_int[user_level] if user_level >= 0 else 0.0])


def surface_closed_form(emis, t_surf, w, dw):
    """The surface row in closed form: numpy's trapezoid of emis dB/dT (c2[0] + c2[1] + c2[2] + c2[3])."""
    f = np.asarray(emis, dtype=np.float64) * planck_derivative(t_surf, w) * (
        STREAM_C2[0] + STREAM_C2[1] + STREAM_C2[2] + STREAM_C2[3])
    return float(np.sum(0.5 * (f[1:] + f[:-1])) * dw)


def oracle_jacobian_sets(orc, lib, band, col, tables, liquid, ice, thickness, x, optics, emis):
    """The four sets of one column of the longwave band, in bit order (clean, aerosol, cloud, both), each a dict of
    jacobian, up_int, dn_int [V]: the objects combined exactly as direct_beam_model.oracle_direct_sets combines them
    (add_optics of gas, Rayleigh, then the aerosol, then liquid and ice), per subcolumn the restatement above and the
    oracle's solver, each integrated with the oracle's trapezoid, then the mean over the subcolumns s = 0 .. S - 1 in
    order.  liquid / ice [S][3][B][L] (None: no cloud sets asked for: two sets), optics [3][L][NA] on the grid x."""
    L = col["p"].size - 1
    w = band.w0 + np.arange(band.nw) * band.dw                             # longwave.c:246
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    aer = oracle_aerosol_optics(orc, band, x, optics)
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
        jac = surface_jacobian(tau, omega, emis, col["t_surf"], w)
        return tuple(trapezoid(orc, a, band.dw) for a in (jac, up, dn))

    def mean(results):
        out = []
        for k in range(3):
            total = results[0][k].copy()
            for r in results[1:]:
                total = total + r[k]
            out.append(total / float(len(results)))
        return dict(jacobian=out[0], up_int=out[1], dn_int=out[2])

    aerosol = [(aer[0], aer[1], aer[2])]
    sets = [mean([one([])]), mean([one(aerosol)])]
    if draws:
        clouds = [[(d[0], d[1], d[2]), (d[3], d[4], d[5])] for d in draws]
        sets.append(mean([one(c) for c in clouds]))
        sets.append(mean([one(aerosol + c) for c in clouds]))
    return tuple(sets)
