"""grt_pipeline_run_ck_fluxes in numpy, for the tests, written from grt_ext.h's definitions: the rows whose class sums are the
sources (the sums themselves are kdist_correlated_model.mapped_rows'), the solve of every g-point on the class means -- the
longwave restated with lw_jacobian_model.planck's constants, STREAM_C1 / STREAM_C2 and radiance_model.effective_planck, the
shortwave by the oracle's sw_fluxes on g-point arrays [L][g-points] -- and the sequential sum of a bin's classes."""
import numpy as np

from kdist_correlated_model import mapped_rows
from lw_jacobian_model import MAX_EXP_ARG, STREAM_C1, STREAM_C2, planck
from radiance_model import effective_planck

MB_TO_ATM = float(np.float32(0.000986923))      # the pipeline's constant is a float
C_AIR = 2.147822334314468e+25


def wavenumbers(w0, dw, n):
    """w0 + i dw, one product and one sum per point, as the solvers form it"""
    return w0 + np.arange(n, dtype=np.float64) * dw


def rayleigh_one(w):
    """rayleigh.c:38-39 with n = 1, operation for operation (no transcendental: the device's bits)"""
    W = w * 1.e-4
    return (1.0 * 1.e-20 * W * W * W * W) / (0.268675 * 1.e5 * (9.38076E2 - 10.8426 * W * W))


def air_columns(p):
    """molecules cm-2 of every layer from the level pressures [V] in mb, as the pipeline stages them"""
    return C_AIR * np.abs(p[:-1] * MB_TO_ATM - p[1:] * MB_TO_ATM)


def lw_rows(cols, w, emis):
    """[ncol][2 V + 1][n]: Planck at the levels, the layers and the surface, then the emissivity (emis [n] or [ncol][n])"""
    emis = np.broadcast_to(np.asarray(emis, dtype=np.float64), (len(cols), w.size))
    return np.array([[planck(T, w) for T in c["t"]] + [planck(T, w) for T in c["t_layer"]] + [planck(c["t_surf"], w), e]
                     for c, e in zip(cols, emis)])


def sw_rows(ncol, w, solar, alb_dir, alb_dif):
    """[ncol][4][n]: the Rayleigh cross-section, the solar curve, the direct and the diffuse albedo"""
    ad = np.broadcast_to(np.asarray(alb_dir, dtype=np.float64), (ncol, w.size))
    af = np.broadcast_to(np.asarray(alb_dif, dtype=np.float64), (ncol, w.size))
    return np.array([[rayleigh_one(w), np.asarray(solar, dtype=np.float64), ad[c], af[c]] for c in range(ncol)])


def source_sums(rows, map_, dw, edges, K):
    """the class sums of the rows [ncol][R][n] under map_ [ncol][n]: [ncol][R][bins][K]"""
    return mapped_rows(rows, map_, dw, edges, K)[2]


def lw_solve(weight, tau, source):
    """weight [...], tau [L][...], source [2 V + 1][...] -> up, down [V][...] in W m-2 per class; +0.0 where weight is 0"""
    weight, tau, source = (np.asarray(a, dtype=np.float64) for a in (weight, tau, source))
    L = tau.shape[0]
    V = L + 1
    live = weight > 0.0
    W = np.where(live, weight, 1.0)
    t, S = tau / W, source / W
    up, dn = np.zeros((V,) + weight.shape), np.zeros((V,) + weight.shape)
    beams = [np.zeros(weight.shape) for _ in range(4)]

    def step(val, tl):
        f = np.zeros(weight.shape)
        for s in range(4):
            e = np.exp(np.minimum(STREAM_C1[s] * tl, MAX_EXP_ARG))
            beams[s] = (1.0 - e) * val + beams[s] * e
            f = f + STREAM_C2[s] * beams[s]
        return f

    for j in range(L):
        dn[j + 1] = step(effective_planck(S[V + j], S[j + 1], t[j]), t[j]) * W
    f = np.zeros(weight.shape)
    for s in range(4):
        beams[s] = S[2 * V] * S[2 * V - 1] + (1 - S[2 * V]) * beams[s]
        f = f + STREAM_C2[s] * beams[s]
    up[L] = f * W
    for j in range(L - 1, -1, -1):
        up[j] = step(effective_planck(S[V + j], S[j], t[j]), t[j]) * W
    return np.where(live, up, 0.0), np.where(live, dn, 0.0)


def sw_solve(orc, weight, tau, source, n_layer, mu_dir, tsi, mu_dif=0.5):
    """weight [...], tau [L][...], source [4][...] of ONE column -> up, down [V][...]: the oracle's shortwave on the live
    g-points, the class SUM of the solar curve as its solar term; +0.0 for empty classes and for a night column"""
    weight, tau, source = (np.asarray(a, dtype=np.float64) for a in (weight, tau, source))
    L = tau.shape[0]
    shape = weight.shape
    w1, t2, s2 = weight.reshape(-1), tau.reshape(L, -1), source.reshape(4, -1)
    up, dn = np.zeros((L + 1, w1.size)), np.zeros((L + 1, w1.size))
    live = w1 > 0.0
    if mu_dir > 0.0 and live.any():
        W = w1[live]
        tg = t2[:, live] / W
        tr = (np.asarray(n_layer, dtype=np.float64)[:, None] * s2[0, live][None, :]) / W
        tt = tg + tr
        u, d = orc.sw_fluxes(tr / tt, np.zeros_like(tt), tt, float(mu_dir), mu_dif, s2[2, live] / W, s2[3, live] / W,
                             float(tsi), s2[1, live])
        up[:, live], dn[:, live] = u, d
    return up.reshape((L + 1,) + shape), dn.reshape((L + 1,) + shape)


def bin_sums(flux):
    """[..., K] -> [...]: (((+0.0 + f[0]) + f[1]) + ...) + f[K - 1]"""
    flux = np.asarray(flux, dtype=np.float64)
    return np.cumsum(np.concatenate((np.zeros(flux.shape[:-1] + (1,)), flux), axis=-1), axis=-1)[..., -1]
