"""Channel transmittance profiles and contribution functions restated in numpy for grt_pipeline_run_sky_weighting's tests,
for the upward radiance at the top of the atmosphere.  Per grid point and viewing secant m, in radiance_model.radiances'
expressions: t_j = tau_j (1 - omega_j), e_j = exp(min((-m) t_j, 700)); the level-to-space transmittance T_0 = 1, T_{j+1} =
T_j e_j (level 0 the top, level V - 1 the surface); P_j = effective_planck(B(T_layer j), B(T_level j), t_j), the upward
sweep's; I_dn, the downward radiance at the surface, as radiances() forms it; and the V + 1 contribution rows K_j = ((1 -
e_j) P_j) T_j for layer j = 0 .. L - 1, K_L = (emis B(T_surf)) T_L, K_{L+1} = ((1 - emis) I_dn) T_L, whose sum is the
upward radiance at the top up to rounding.  A channel's value is channel_model.channel_mean of a row; a cloud set's the mean
over its draws in order.  test_weighting_model.py holds the restatement against radiance_model and the oracle's solver."""
import numpy as np

from aerosol_model import oracle_aerosol_optics
from channel_model import channel_mean, sign_ratio
from cloud_bands import band_map, driver_limits, grid_optics
from lw_jacobian_model import MAX_EXP_ARG, planck
from pipeline_support import limits
from radiance_model import effective_planck


def weighting(tau, omega, emis, t_surf, t_layers, t_levels, w, secants):
    """-> (T [A][V][n], K [A][V + 1][n]) from a set's combined tau, omega [L][n], the emissivity [n], the temperatures and
    the grid's wavenumbers w [n]."""
    tau, omega, emis, w = (np.asarray(a, dtype=np.float64) for a in (tau, omega, emis, w))
    t = tau * (1.0 - omega)                                                # longwave.c:252
    L, n = t.shape
    V = L + 1
    bs = planck(t_surf, w)
    down_p = [effective_planck(planck(t_layers[j], w), planck(t_levels[j + 1], w), t[j]) for j in range(L)]
    up_p = [effective_planck(planck(t_layers[j], w), planck(t_levels[j], w), t[j]) for j in range(L)]
    T = np.zeros((len(secants), V, n))
    K = np.zeros((len(secants), V + 1, n))
    for k, m in enumerate(secants):
        c1 = -float(m)
        beam = np.zeros(n)
        T[k, 0] = 1.0
        for j in range(L):
            e = np.exp(np.minimum(c1 * t[j], MAX_EXP_ARG))
            K[k, j] = ((1.0 - e) * up_p[j]) * T[k, j]
            beam = (1.0 - e) * down_p[j] + beam * e
            T[k, j + 1] = T[k, j] * e
        K[k, L] = (emis * bs) * T[k, L]
        K[k, L + 1] = ((1 - emis) * beam) * T[k, L]
    return T, K


def closure_bound(K):
    """What the sum of the V + 1 rows may miss the upward radiance by, per point: 4 (L + 2) 2^-52 sum |rows| -- each of the
    L + 2 terms carries a handful of roundings.  K [..][V + 1][n] -> [..][n]."""
    rows = K.shape[-2]
    return 4.0 * rows * 2.0 ** -52 * np.abs(K).sum(axis=-2)


def oracle_weighting_points(orc, lib, band, col, tables, liquid, ice, thickness, x, optics, emis, secants):
    """radiance_model.oracle_radiance_sets' four sets of one column (the same objects combined in the same order), each the
    list over its draws of weighting()'s (T, K) at every point."""
    L = col["p"].size - 1
    w = band.w0 + np.arange(band.nw) * band.dw
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
        return weighting(tau, omega, emis, col["t_surf"], col["t_layer"], col["t"], w, secants)

    sets = [[one([])]]
    aerosol = []
    if optics is not None:
        aer = oracle_aerosol_optics(orc, band, x, optics)
        aerosol = [(aer[0], aer[1], aer[2])]
        sets.append([one(aerosol)])
    if draws:
        clouds = [[(d[0], d[1], d[2]), (d[3], d[4], d[5])] for d in draws]
        sets.append([one(c) for c in clouds])
        if optics is not None:
            sets.append([one(aerosol + c) for c in clouds])
    return tuple(sets)


def channel_sets(points, first, weights):
    """oracle_weighting_points' sets for an instrument: each a dict of trans [A][V][C] and contrib [A][V + 1][C] --
    channel_mean of every draw's rows, then the mean over the draws s = 0 .. S - 1 in order, one division --, largest [A][V
    + 1], each contribution row's largest magnitude at a point over the draws (a transmittance row's is 1), and closure
    [A][C], closure_bound of every draw carried through |W| / sum W, the mean over the draws."""
    out = []
    absolute = [np.abs(np.asarray(x, dtype=np.float64)) for x in weights]
    ratio = sign_ratio(weights)

    def carried(K):
        return channel_mean(closure_bound(K), first, absolute) * ratio       # sum |W| bound / sum W

    for draws in points:
        S = len(draws)
        trans = channel_mean(draws[0][0], first, weights)
        contrib = channel_mean(draws[0][1], first, weights)
        closure = carried(draws[0][1])
        for T, K in draws[1:]:
            trans = trans + channel_mean(T, first, weights)
            contrib = contrib + channel_mean(K, first, weights)
            closure = closure + carried(K)
        if S > 1:
            trans, contrib, closure = trans / float(S), contrib / float(S), closure / float(S)
        largest = np.max([np.abs(K).max(axis=-1) for T, K in draws], axis=0)
        out.append(dict(trans=trans, contrib=contrib, largest=largest, closure=closure))
    return tuple(out)
