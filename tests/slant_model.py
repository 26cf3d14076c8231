"""The shortwave solver with a sun cosine per layer for the direct beam, restated in numpy for the tests of
grt_pipeline_run_sky_zeniths_slant: shortwave.c:86-329 -- the delta-scaling (:86-89), both Eddington solutions of a layer
with the optical-depth clamp (:114-207, gammas :228-230), the two adding sweeps (:272-302) and the level fluxes
(:305-328) -- then the scaling by solar_flux mu0 and the total solar irradiance (:401-405, :447-451).  The one change:
in layer j the direct-beam solution takes mu_layer[j] where the reference takes mu_dir.  The diffuse solution (mu_dif),
the sweeps, the level expressions and the scale solar x mu0 are the reference's.  The direct beam itself is
direct_beam_model.pure_transmission's running product, which broadcasts an [L][1] cosine.

test_slant_model.py pins the restatement to the oracle's solver with every layer at one cosine, for each of
pipeline_support.MU0 and for optics with clouds and an aerosol among the layers: the largest difference measured there is
1.2e-15 of the column's largest flux, and the test bounds it at ten times that, 1.2e-14."""
import numpy as np

from direct_beam_model import MAX_EXP_ARG, pure_transmission

PIN_MEASURED = 1.2e-15      # the largest difference to the oracle's solver, of the column's largest flux (test_slant_model.py)
PIN_BOUND = 10.0 * PIN_MEASURED


def delta_scaling(omega, g, tau):
    """shortwave.c:86-89 -> omega_s, g_s, tau_s"""
    f = g * g
    return (1.0 - f) * omega / (1.0 - omega * f), g / (g + 1.0), tau * (1.0 - omega * f)


def eddington(os, ts, mu, gs, with_pure):
    """R, T (and T_pure) [L][n] of layers os, ts, gs [L][n] for a beam of cosine mu (a scalar or [L][1]): :114-207 with the
    gammas of :228-230; with_pure mirrors T_pure != NULL (T = max(T, T_pure))."""
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), os.shape)
    gamma1 = 0.25 * (7.0 - os * (4.0 + 3.0 * gs))
    gamma2 = -0.25 * (1.0 - os * (4.0 - 3.0 * gs))
    gamma3 = 0.25 * (2.0 - 3.0 * gs * mu)
    gamma4 = 1.0 - gamma3
    alpha1 = gamma1 * gamma4 + gamma2 * gamma3
    alpha2 = gamma1 * gamma3 + gamma2 * gamma4
    with np.errstate(all="ignore"):
        k = np.sqrt(gamma1 * gamma1 - gamma2 * gamma2)
        first = (1.0 / mu > k) & (ts / mu > MAX_EXP_ARG)
        second = ~first & (ts * k > MAX_EXP_ARG)
        t = np.where(first, MAX_EXP_ARG * mu, np.where(second, MAX_EXP_ARG / k, ts))
        tp, tm, tkm, tkp = np.exp(t / mu), np.exp(-t / mu), np.exp(-t * k), np.exp(t * k)
        r_cons = (1.0 / (1.0 + gamma1 * t)) * (gamma1 * t + (gamma3 - gamma1 * mu) * (1.0 - tm))
        front = os / ((1.0 - k * k * mu * mu) * ((k + gamma1) * tkp + (k - gamma1) * tkm))
        r_abs = front * ((1.0 - k * mu) * (alpha2 + k * gamma3) * tkp - (1.0 + k * mu) * (alpha2 - k * gamma3) * tkm
                         - 2.0 * k * (gamma3 - alpha2 * mu) * tm)
        t_abs = tm * (1.0 - front * ((1.0 + k * mu) * (alpha1 + k * gamma4) * tkp - (1.0 - k * mu) * (alpha1 - k * gamma4) * tkm
                                     - 2.0 * k * (gamma4 + alpha1 * mu) * tp))
        R = np.where(os >= 1.0, r_cons, r_abs)
        T = np.where(os >= 1.0, 1.0 - r_cons, t_abs)
        pure = tm
        empty = tp <= 1.0                                   # :149-158
        R, T, pure = np.where(empty, 0.0, R), np.where(empty, 1.0, T), np.where(empty, 1.0, pure)
        none = os <= 0.0                                    # :114-123
        e = np.exp(-ts / mu)
        R, T, pure = np.where(none, 0.0, R), np.where(none, e, T), np.where(none, e, pure)
    if with_pure:
        T = np.where(pure > T, pure, T)
    return R, T, pure


def sw_fluxes(omega, g, tau, mu_layer, mu_dif, alb_dir, alb_dif, tsi, solar, mu0):
    """up, dn, direct [V][n] (levels top first, W m-2 per cm-1) of a column of optics omega, g, tau [L][n] whose direct
    beam has the cosine mu_layer[j] ([L], or a scalar: every layer) in layer j, under the flux scale solar x mu0."""
    omega, g, tau = (np.asarray(a, dtype=np.float64) for a in (omega, g, tau))
    L, n = tau.shape
    mul = np.broadcast_to(np.asarray(mu_layer, dtype=np.float64).reshape(-1, 1), (L, 1))
    os, gs, ts = delta_scaling(omega, g, tau)
    Rdir, Tdir, _ = eddington(os, ts, mul, gs, True)
    Rdif, Tdif, _ = eddington(os, ts, mu_dif, gs, False)
    Tpure = pure_transmission(tau, omega, g, mul)
    V = L + 1
    # :272-289, from the surface up
    Rdir_dn, Rdif_dn = np.empty((V, n)), np.empty((V, n))
    Rdir_dn[L], Rdif_dn[L] = alb_dir, alb_dif
    for i in range(L - 1, -1, -1):
        A = Tpure[i]
        B = 1.0 / (1.0 - Rdif[i] * Rdif_dn[i + 1])
        Rdir_dn[i] = Rdir[i] + (A * Rdir_dn[i + 1] + (Tdir[i] - A) * Rdif_dn[i + 1]) * Tdif[i] * B
        Rdif_dn[i] = Rdif[i] + Tdif[i] * Tdif[i] * Rdif_dn[i + 1] * B
    # :294-302, from the top down
    Rdif_up = np.empty((L, n))
    Rdif_up[0] = Rdif[0]
    for i in range(1, L):
        B = 1.0 / (1.0 - Rdif[i] * Rdif_up[i - 1])
        Rdif_up[i] = Rdif[i] + Tdif[i] * Tdif[i] * Rdif_up[i - 1] * B
    # :305-328
    R, T, D = np.empty((V, n)), np.empty((V, n)), np.empty((V, n))
    dir_beam, dif_beam = np.ones(n), np.zeros(n)
    R[0], T[0], D[0] = dir_beam * Rdir_dn[0], dir_beam, dir_beam
    for i in range(1, V):
        if i > 1:
            C = 1.0 / (1.0 - Rdif[i - 1] * Rdif_up[i - 2])
            dif_beam = (dir_beam * Rdir[i - 1] * Rdif_up[i - 2] + dif_beam) * Tdif[i - 1] * C + dir_beam * (Tdir[i - 1] - Tpure[i - 1])
        else:
            dif_beam = dir_beam * (Tdir[i - 1] - Tpure[i - 1])
        dir_beam = dir_beam * Tpure[i - 1]
        B = 1.0 / (1.0 - Rdif_dn[i] * Rdif_up[i - 1])
        R[i] = (dir_beam * Rdir_dn[i] + dif_beam * Rdif_dn[i]) * B
        T[i] = dir_beam * (1.0 + Rdir_dn[i] * Rdif_up[i - 1] * B) + dif_beam * B
        D[i] = dir_beam
    scale = np.asarray(solar, dtype=np.float64) * mu0                      # :401-405, :447-451
    return tsi * (R * scale), tsi * (T * scale), tsi * (D * scale)
