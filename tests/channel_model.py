"""Instrument channels restated in numpy for grt_pipeline_run_sky_channels' tests.  A channel is the grid points first ..
first + count - 1 with the weights W_k; its radiance is the weighted mean (sum_k W_k I_k) / (sum_k W_k) of the spectral
radiance I of radiance_model.py, sum_k W_k added in index order; its brightness temperature is planck() solved for T at the
channel centre, T = c2 v / log1p(c1 v^3 / R), +0.0 where R <= 0.  A cloud set's channel radiance is the mean over its draws
of the draws' channel radiances, s = 0 .. S - 1 in order, then one division by S."""
import numpy as np

from aerosol_model import oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from lw_jacobian_model import PLANCK_C1, PLANCK_C2
from pipeline_support import limits
from radiance_model import radiances

BLOCK = 128                    # points of a solver block


def weight_sum(weights):
    """sum_k W_k in index order, as the library's host code adds it."""
    s = 0.0
    for x in np.asarray(weights, dtype=np.float64):
        s += float(x)
    return s


def channel_mean(rows, first, weights):
    """rows [..][n] -> [..][C]: per channel c the weighted mean of rows[.., first[c] : first[c] + len(weights[c])]."""
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros(rows.shape[:-1] + (len(weights),))
    for c, (f, w) in enumerate(zip(first, weights)):
        w = np.asarray(w, dtype=np.float64)
        out[..., c] = (rows[..., int(f):int(f) + w.size] * w).sum(axis=-1) / weight_sum(w)
    return out


def magnitude(rows, first, weights):
    """... and sum_k |W_k I_k| / sum_k W_k: what an error of so many ulps of the additions is measured in."""
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros(rows.shape[:-1] + (len(weights),))
    for c, (f, w) in enumerate(zip(first, weights)):
        w = np.asarray(w, dtype=np.float64)
        out[..., c] = np.abs(rows[..., int(f):int(f) + w.size] * w).sum(axis=-1) / weight_sum(w)
    return out


def sign_ratio(weights):
    """sum |W| / sum W per channel -> [C]: how much a weighted mean can magnify a per-point error."""
    return np.array([np.abs(np.asarray(w, dtype=np.float64)).sum() / weight_sum(w) for w in weights])


def centroid(first, weights, w0, dw):
    """sum_k W_k w_i / sum_k W_k with w_i = w0 + i dw -> [C]."""
    out = []
    for f, w in zip(first, weights):
        w = np.asarray(w, dtype=np.float64)
        s = 0.0
        for k in range(w.size):
            s += float(w[k]) * (w0 + float(int(f) + k) * dw)
        out.append(s / weight_sum(w))
    return np.array(out)


def channel_brightness(R, center):
    """R [..][C], center [C] -> [..][C]: c2 v / log1p(c1 v^3 / R), +0.0 where R <= 0."""
    R = np.asarray(R, dtype=np.float64)
    v = np.broadcast_to(np.asarray(center, dtype=np.float64), R.shape)
    out = np.zeros(R.shape)
    lit = R > 0.0
    out[lit] = PLANCK_C2 * v[lit] / np.log1p((PLANCK_C1 * v[lit] * v[lit] * v[lit]) / R[lit])
    return out


def pair_count(first, counts, n):
    """The (channel, BLOCK-point block) pairs in which a channel has a point: sum_c (last block - first block + 1)."""
    total = 0
    for f, k in zip(first, counts):
        f, k = int(f), int(k)
        assert 0 <= f and k >= 1 and f + k <= n
        total += (f + k - 1) // BLOCK - f // BLOCK + 1
    return total


def oracle_channel_sets(orc, lib, band, col, tables, liquid, ice, thickness, x, optics, emis, secants, first, weights):
    """radiance_model.oracle_radiance_sets' four sets of one column (the same objects combined in the same order), each a
    dict of chan [A][2][C] -- channel_mean of every draw's radiances, then the mean over the draws in order --, largest
    [A][2], each row's largest radiance at a point over the draws, absolute [A][2], sum_i |I(i)| of each row, the mean over
    the draws (times dw: the magnitude of the row's trapezoid), and rad [A][2][n], the first draw's radiances."""
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
        return radiances(tau, omega, emis, col["t_surf"], col["t_layer"], col["t"], w, secants)

    def mean(rads):
        total = channel_mean(rads[0], first, weights)
        for r in rads[1:]:
            total = total + channel_mean(r, first, weights)
        largest = np.max([np.abs(r).max(axis=-1) for r in rads], axis=0)
        absolute = np.sum([np.abs(r).sum(axis=-1) for r in rads], axis=0) / float(len(rads))
        return dict(chan=total / float(len(rads)) if len(rads) > 1 else total, largest=largest, rad=rads[0],
                    absolute=absolute)

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
