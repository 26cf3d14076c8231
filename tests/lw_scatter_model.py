"""The longwave scattering correction (grt_ext.h: grt_pipeline_run_sky_scattering, grt_lw_scatter_levels) restated on the
CPU: in float64 numpy, operation for operation what k_longwave_scatter.hip computes, and in mpmath at 50 digits; with
them a dense solve of the same two-stream boundary-value problem, and the list of cases the kernel is held to.

Everything works on arrays whose LAST axis is the layer (top first); any leading axes are points.

    delta = F[tau, omega, g] - F[tau (1 - omega), 0, 0]        (two_stream_fluxes, twice; scatter_delta)
"""
import numpy as np

D = 1.66
K2_MIN = 1e-12
MAX_EXP = 700.0
PLANCK_C1 = 1.1910429526245744e-8
PLANCK_C2 = 1.4387773538277202


# ---- float64 ------------------------------------------------------------------------------------------------------ #
def planck(T, w):
    """planck_dev.h: planck()"""
    e = np.minimum(PLANCK_C2 * w / T, MAX_EXP)
    return (PLANCK_C1 * w * w * w) / (np.exp(e) - 1.0)


def effective_planck(bc, be, tau):
    """longwave_dev.h: effective_planck()"""
    a, b = 0.193, 0.013
    return (bc + (a * tau + b * tau * tau) * be) / (1.0 + a * tau + b * tau * tau)


def layer(tau, omega, g, pu, pd):
    """two_stream_layer: R, T, S_up, S_down, eps"""
    g1 = D * (1.0 - omega * (1.0 + g) / 2.0)
    g2 = D * omega * (1.0 - g) / 2.0
    k = np.sqrt(np.maximum((g1 - g2) * (g1 + g2), K2_MIN))
    x = np.minimum(k * tau, MAX_EXP)
    e = np.exp(-x)
    E = -np.expm1(-2.0 * x)
    m = -np.expm1(-x)
    den = k * (1.0 + e * e) + g1 * E
    R = g2 * E / den
    T = 2.0 * k * e / den
    eps = (k * m * m + (g1 - g2) * E) / den
    return R, T, eps * np.pi * pu, eps * np.pi * pd, eps


def sources(tau, omega, t_layers, t_levels, w):
    """The effective Planck terms of the upward and the downward source, [..., L]; t_layers [..., L], t_levels [..., L + 1]
    and w broadcast against the points."""
    ta = tau * (1.0 - omega)
    bc = planck(t_layers, w)
    return (effective_planck(bc, planck(t_levels[..., :-1], w), ta),
            effective_planck(bc, planck(t_levels[..., 1:], w), ta))


def adding(R, T, su, sd, A_L, U_L):
    """adding_up then adding_down: (F_up, F_down), each [..., L + 1]"""
    L = R.shape[-1]
    shape = np.broadcast(R[..., 0], A_L, U_L).shape
    A = np.empty(shape + (L + 1,))
    U = np.empty(shape + (L + 1,))
    A[..., L] = A_L
    U[..., L] = U_L
    for j in range(L - 1, -1, -1):
        beta = 1.0 / (1.0 - A[..., j + 1] * R[..., j])
        A[..., j] = R[..., j] + T[..., j] * T[..., j] * A[..., j + 1] * beta
        U[..., j] = su[..., j] + T[..., j] * (U[..., j + 1] + A[..., j + 1] * sd[..., j]) * beta
    fu = np.empty_like(A)
    fd = np.empty_like(A)
    fd[..., 0] = 0.0
    fu[..., 0] = U[..., 0]
    for j in range(L):
        beta = 1.0 / (1.0 - A[..., j + 1] * R[..., j])
        fd[..., j + 1] = (T[..., j] * fd[..., j] + R[..., j] * U[..., j + 1] + sd[..., j]) * beta
        fu[..., j + 1] = A[..., j + 1] * fd[..., j + 1] + U[..., j + 1]
    return fu, fd


def two_stream_fluxes(tau, omega, g, pu, pd, emis, bs):
    R, T, su, sd, _ = layer(tau, omega, g, pu, pd)
    return adding(R, T, su, sd, 1.0 - emis, emis * np.pi * bs)


def scatter_delta(tau, omega, g, t_layers, t_levels, t_surf, emis, w):
    """-> delta_up, delta_down, flux_up, flux_down, each [..., L + 1]: the correction and the scattering solve's own fluxes.
    tau, omega, g, t_layers [..., L], t_levels [..., L + 1]; t_surf, emis, w [...] (everything broadcasts over the points)"""
    tau, omega, g = (np.asarray(x, dtype=np.float64) for x in (tau, omega, g))
    t_surf, emis, w = (np.asarray(x, dtype=np.float64) for x in (t_surf, emis, w))
    pu, pd = sources(tau, omega, np.asarray(t_layers), np.asarray(t_levels), w[..., None])
    bs = planck(t_surf, w)
    fu, fd = two_stream_fluxes(tau, omega, g, pu, pd, emis, bs)
    zero = np.zeros_like(tau)
    au, ad = two_stream_fluxes(tau * (1.0 - omega), zero, zero, pu, pd, emis, bs)
    return fu - au, fd - ad, fu, fd


def dense_fluxes(R, T, su, sd, A_L, U_L):
    """One column (1-D arrays [L]): the 2 V boundary-value equations solved at once.  Unknowns F_up_0 .. F_up_L, then
    F_down_0 .. F_down_L."""
    L = len(R)
    V = L + 1
    M = np.zeros((2 * V, 2 * V))
    rhs = np.zeros(2 * V)
    up, dn = (lambda i: i), (lambda i: V + i)
    M[0, dn(0)] = 1.0                                                   # F_down_0 = 0
    row = 1
    for j in range(L):
        M[row, up(j)] = 1.0; M[row, dn(j)] = -R[j]; M[row, up(j + 1)] = -T[j]; rhs[row] = su[j]; row += 1
        M[row, dn(j + 1)] = 1.0; M[row, dn(j)] = -T[j]; M[row, up(j + 1)] = -R[j]; rhs[row] = sd[j]; row += 1
    M[row, up(L)] = 1.0; M[row, dn(L)] = -A_L; rhs[row] = U_L
    x = np.linalg.solve(M, rhs)
    return x[:V], x[V:]


# ---- mpmath, 50 digits ---------------------------------------------------------------------------------------------- #
def mp_scatter_delta(tau, omega, g, t_layers, t_levels, t_surf, emis, w, dps=50):
    """One column (sequences of L floats, scalars): scatter_delta in mpmath -> four lists of V mpf"""
    import mpmath as mp
    with mp.workdps(dps):
        f = mp.mpf
        pi = mp.pi
        Dm = f("1.66")
        c1, c2 = f(PLANCK_C1), f(PLANCK_C2)
        w = f(float(w))

        def B(T):
            e = min(c2 * w / f(float(T)), f(700))
            return c1 * w * w * w / (mp.exp(e) - 1)

        def peff(bc, be, t):
            a, b = f(0.193), f(0.013)
            return (bc + (a * t + b * t * t) * be) / (1 + a * t + b * t * t)

        def lay(t, o, gg, pu, pd):
            g1 = Dm * (1 - o * (1 + gg) / 2)
            g2 = Dm * o * (1 - gg) / 2
            k = mp.sqrt(max((g1 - g2) * (g1 + g2), f(K2_MIN)))
            x = min(k * t, f(700))
            e = mp.exp(-x)
            E = -mp.expm1(-2 * x)
            m = -mp.expm1(-x)
            den = k * (1 + e * e) + g1 * E
            eps = (k * m * m + (g1 - g2) * E) / den
            return g2 * E / den, 2 * k * e / den, eps * pi * pu, eps * pi * pd

        L = len(tau)
        emis_m = f(float(emis))

        def solve(ts, os_, gs, pus, pds):
            lay_ = [lay(ts[j], os_[j], gs[j], pus[j], pds[j]) for j in range(L)]
            A = [None] * (L + 1)
            U = [None] * (L + 1)
            A[L] = 1 - emis_m
            U[L] = emis_m * pi * B(t_surf)
            for j in range(L - 1, -1, -1):
                R, T, su, sd = lay_[j]
                beta = 1 / (1 - A[j + 1] * R)
                A[j] = R + T * T * A[j + 1] * beta
                U[j] = su + T * (U[j + 1] + A[j + 1] * sd) * beta
            fu, fd = [U[0]], [f(0)]
            for j in range(L):
                R, T, su, sd = lay_[j]
                beta = 1 / (1 - A[j + 1] * R)
                fd.append((T * fd[j] + R * U[j + 1] + sd) * beta)
                fu.append(A[j + 1] * fd[j + 1] + U[j + 1])
            return fu, fd

        ts = [f(float(x)) for x in tau]
        os_ = [f(float(x)) for x in omega]
        gs = [f(float(x)) for x in g]
        ta = [t * (1 - o) for t, o in zip(ts, os_)]
        pus = [peff(B(t_layers[j]), B(t_levels[j]), ta[j]) for j in range(L)]
        pds = [peff(B(t_layers[j]), B(t_levels[j + 1]), ta[j]) for j in range(L)]
        fu, fd = solve(ts, os_, gs, pus, pds)
        zero = [f(0)] * L
        au, ad = solve(ta, zero, zero, pus, pds)
        return ([a - b for a, b in zip(fu, au)], [a - b for a, b in zip(fd, ad)], fu, fd)


# ---- the cases ------------------------------------------------------------------------------------------------------ #
def case_list(L, seed=20260):
    """The point cases the kernel is compared on, for columns of L layers: dict(tau, omega, g [N][L], emis [N],
    no_scatter [N] bool -- omega is 0 in every layer).  Random ordinary columns (tau 1e-6 .. 100, omega <= 0.98, any g,
    emis 0.5 .. 1); tau = 0 in one layer and in all; tau down to 1e-300 and up to 1e5; omega in {0, 1 - 1e-9, 1} with
    emis >= 0.5; g in {-1, 0, 1}; emis in {0, 1} with omega <= 0.98.  Not among them: omega = 1 in every layer over
    emis = 0, a conservative atmosphere over a mirror with nothing that emits -- ill-conditioned at 2e-6."""
    rng = np.random.default_rng(seed + L)
    rows = []

    def ordinary():
        return (10.0 ** rng.uniform(-6, 2, L), rng.uniform(0, 0.98, L), rng.uniform(-1, 1, L), rng.uniform(0.5, 1.0))

    def add(tau=None, omega=None, g=None, emis=None):
        t, o, gg, e = ordinary()
        pick = lambda given, own: own if given is None else np.broadcast_to(np.asarray(given, dtype=np.float64), (L,)).copy()
        rows.append((pick(tau, t), pick(omega, o), pick(g, gg), e if emis is None else float(emis)))

    for _ in range(12):
        add()
    t = ordinary()[0]
    t[rng.integers(L)] = 0.0
    add(tau=t)                                          # tau = 0 in a layer
    add(tau=0.0)                                        # ... in all layers
    add(tau=0.0, omega=0.0)
    for tiny in (1e-300, 1e-100, 1e-8):
        add(tau=tiny)
        t = ordinary()[0]
        t[rng.integers(L)] = tiny
        add(tau=t)
    for big in (1e3, 1e5):
        add(tau=big)
        t = ordinary()[0]
        t[rng.integers(L)] = big
        add(tau=t)
    for _ in range(3):
        add(omega=0.0)                                  # nothing scatters: delta is exactly 0
    add(omega=0.0, g=1.0)
    add(omega=0.0, tau=1e5)
    for om in (1.0 - 1e-9, 1.0):
        add(omega=om, g=0.0, emis=0.5)
        add(omega=om, emis=0.9)
        o = ordinary()[1]
        o[rng.integers(L)] = om
        add(omega=o)
    for gg in (-1.0, 0.0, 1.0):
        add(g=gg)
        add(g=gg, omega=0.98)
    for em in (0.0, 1.0):
        add(emis=em)
        add(emis=em, tau=10.0 ** rng.uniform(-2, 1, L))
    tau, omega, g, emis = (np.array(x) for x in zip(*rows))
    return dict(tau=tau, omega=omega, g=g, emis=emis, no_scatter=(omega == 0.0).all(axis=1))


def temperatures(L, ncol, seed=7):
    """ncol columns' layer, level and surface temperatures: cold aloft, warm below, the surface a few K off the lowest level"""
    rng = np.random.default_rng(seed + 31 * L)
    t_levels = np.sort(rng.uniform(190.0, 300.0, (ncol, L + 1)), axis=1)
    t_layers = 0.5 * (t_levels[:, :-1] + t_levels[:, 1:]) + rng.uniform(-1.0, 1.0, (ncol, L))
    t_surf = t_levels[:, -1] + rng.uniform(-3.0, 8.0, ncol)
    return t_layers, t_levels, t_surf


def kernel_inputs(ncol, L, nw, w0=500.0, dw=1.0):
    """The kernel test's arrays: point i of column c takes case (i + 7 c) % N of case_list(L) -> dict(tau, omega, g
    [ncol][L][nw], emis [ncol][nw], t_layers, t_levels, t_surf, w [nw], case [ncol][nw], no_scatter [ncol][nw])"""
    cl = case_list(L)
    N = len(cl["emis"])
    case = (np.arange(nw)[None, :] + 7 * np.arange(ncol)[:, None]) % N
    t_layers, t_levels, t_surf = temperatures(L, ncol)
    out = dict(case=case, emis=np.ascontiguousarray(cl["emis"][case]), no_scatter=cl["no_scatter"][case],
               t_layers=t_layers, t_levels=t_levels, t_surf=t_surf, w=w0 + dw * np.arange(nw), w0=w0, dw=dw)
    for k in ("tau", "omega", "g"):
        out[k] = np.ascontiguousarray(np.transpose(cl[k][case], (0, 2, 1)))        # [ncol][nw][L] -> [ncol][L][nw]
    return out


def model_on_inputs(inp):
    """scatter_delta on kernel_inputs' arrays -> delta_up, delta_down, flux_up, flux_down, each [ncol][V][nw]"""
    pts = lambda x: np.transpose(x, (0, 2, 1))                                      # [ncol][L][nw] -> [ncol][nw][L]
    res = scatter_delta(pts(inp["tau"]), pts(inp["omega"]), pts(inp["g"]), inp["t_layers"][:, None, :],
                        inp["t_levels"][:, None, :], inp["t_surf"][:, None], inp["emis"], inp["w"][None, :])
    return tuple(np.ascontiguousarray(np.transpose(x, (0, 2, 1))) for x in res)
