"""What the batched pipeline's GPU tests (test_gpu_pipeline*.py, test_gpu_solver_shapes.py, test_gpu_subcolumn_shapes.py)
share, once each: the oracle's column-by-column restatements of the reference driver, the bands and cloud tables the
cases run on, their inputs, the four base entry points behind one call, a module's cache of oracle results, and the
checks more than one module makes.  A plain module: a test module imports what it
uses, the module fixtures (bands, tables, solver_bands) included, so each file shows what it depends on.  pytest does
not rewrite the asserts of a plain module: the ones here carry their own messages."""
import ctypes as C
import math

import numpy as np
import pytest

from cloud_bands import band_map, band_optics, driver_limits, grid_optics
from cloud_model import synthetic_tables
from grtcode_amd import api, synthetic as syn
from scenario import Band

GRAVITY, CP = 9.80665, 1004.64       # grt_ext.h: GRT_GRAVITY, GRT_SPECIFIC_HEAT_AIR
LEVEL_KEYS = ("lw_up", "lw_down", "sw_up", "sw_down")
KEYS = LEVEL_KEYS + ("lw_heating", "sw_heating", "fluxes")
SETS = ("lw_liquid", "lw_ice", "sw_liquid", "sw_ice")
LIQUID_EDGES = [10.0, 90.0, 170.0, 260.0, 350.0, 1800.0, 4200.0]                      # 6 liquid bands
ICE_EDGES = [10.0, 120.0, 230.0, 330.0, 1500.0, 3000.0, 4400.0, 6000.0, 9000.0]       # 8 ice bands


# ---- bands and inputs -------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def bands(request, tmp_path_factory):
    """The longwave and the shortwave band most cases run on, written once per test module."""
    root = tmp_path_factory.mktemp(request.module.__name__)
    lw = Band(str(root / "lw"), 1.0, 400.0, 1.0, 3000)
    sw = Band(str(root / "sw"), 1.0, 5000.0, 10.0, 3000, sw=True)
    return lw, sw


def make_shape_bands(ns, lw_w0, sw_w0):
    """A module fixture: per grid length n of ns a (longwave, shortwave) pair of n points at 1 and 10 cm-1 that starts at
    lw_w0 / sw_w0 (one wavenumber, or one per n)."""
    @pytest.fixture(scope="module")
    def fixture(request, tmp_path_factory):
        root = tmp_path_factory.mktemp(request.module.__name__ + "_shapes")
        out = {}
        for n in ns:
            lw0, sw0 = (w[n] if isinstance(w, dict) else w for w in (lw_w0, sw_w0))
            out[n] = (Band(str(root / f"lw{n}"), lw0, lw0 + (n - 1) * 1.0, 1.0, 300),
                      Band(str(root / f"sw{n}"), sw0, sw0 + (n - 1) * 10.0, 10.0, 300, sw=True))
            assert out[n][0].nw == n and out[n][1].nw == n
        return out
    return fixture


def _setup(bands, device, V, fast=0):
    """Gas optics (tuned to the form `fast`, Band.gas_optics), surface and sun of a (longwave, shortwave) pair of bands,
    either of which may be None."""
    lwb, swb = bands
    go_lw, _ = lwb.gas_optics(device, V, fast=fast) if lwb is not None else (None, None)
    go_sw, grid_sw = swb.gas_optics(device, V, fast=fast) if swb is not None else (None, None)
    emis = np.full(lwb.nw, 0.98) if lwb is not None else None
    alb = np.full(swb.nw, 0.2) if swb is not None else None
    solar = api.create_solar_flux(grid_sw, swb.files["solar"]) if swb is not None else None
    return go_lw, go_sw, emis, alb, solar


def _sentinel(device, n):
    """A device buffer of n doubles, each -7.25: what a refused call must leave."""
    buf = api.DeviceBuffer(device, 8 * n)
    fill = np.full(n, -7.25)
    api.check(api.load_library().grt_host_to_device(device, buf.ptr, fill.ctypes.data_as(C.c_void_p), C.c_size_t(8 * n)))
    return buf


def _deterministic(lib, on):
    api.check(lib.grt_set_deterministic(1 if on else -1))


# ---- clouds ------------------------------------------------------------------------------------------------------------ #
@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """Synthetic cloud parametrisations: more ice bands than liquid ones, and a gap after liquid band 1."""
    root = tmp_path_factory.mktemp("cloud_tables")
    (root / "i").mkdir()
    _, t = synthetic_tables(str(root), seed=4, band_edges=LIQUID_EDGES)
    _, ti = synthetic_tables(str(root / "i"), seed=9, band_edges=ICE_EDGES)
    t["ice"] = ti["ice"]
    t["liquid"]["Band_limits_upr"][1] = np.float64(np.float32(150.0))
    return t


def limits(t, phase):
    return t[phase]["Band_limits_lwr"].copy(), t[phase]["Band_limits_upr"].copy()


def subcolumn_clouds(cols, tables, seed, S, clear=False):
    """Cloud fields of each column -- overcast, partial and clear layers, liquid-only (low) and ice-only (high) ones --,
    layer thickness, and S draws of its band optics per pass, drawn as a driver with num_subcolumns = S draws them: per
    column, S longwave draws, then S shortwave draws.  Optics sets [ncol][S][3][B][L]."""
    L = cols[0]["p"].size - 1
    rng = np.random.default_rng(seed)
    out = {k: [] for k in SETS}
    th = []
    for c, col in enumerate(cols):
        cf = np.where(rng.random(L) < 0.5, rng.random(L), 0.0)
        cf[L - 3 - c % 4] = 1.0                                     # overcast
        cf[2] = 0.0                                                 # clear
        lwc = np.where(cf > 0, 0.2 * rng.random(L), 0.0)
        iwc = np.where(cf > 0, 0.03 * rng.random(L), 0.0)
        lwc[np.arange(L) < L // 3] = 0.0                            # ice only aloft
        iwc[L - 2:] = 0.0                                           # liquid only at the bottom
        cf[(lwc + iwc) == 0.0] = 0.0
        if clear:
            cf[:], lwc[:], iwc[:] = 0.0, 0.0, 0.0
        overlap = np.exp(-np.abs(np.diff(np.log(col["p"][1:] + col["p"][:-1]))) / 0.5)
        th.append(29.3 * col["t_layer"] * np.log(col["p"][1:] / col["p"][:-1]))          # m (hypsometric)
        draw = np.random.default_rng(seed * 7 + c).random
        for kl, ki in (("lw_liquid", "lw_ice"), ("sw_liquid", "sw_ice")):                 # two passes, S draws each
            draws = [band_optics(tables, draw, cf, lwc, iwc, overlap, 10.0, col["t_layer"]) for _ in range(S)]
            out[kl].append(np.array([d[0] for d in draws]))
            out[ki].append(np.array([d[1] for d in draws]))
    return dict(thickness=np.array(th), **{k: np.array(v) for k, v in out.items()})


def cloud_columns(cols, tables, seed, clear=False):
    """subcolumn_clouds' fields with one draw per pass, as the single-subcolumn entry points take them: optics sets
    [ncol][3][B][L].  At most four columns: the overcast layer of column c is layer L - 3 - c."""
    assert len(cols) <= 4
    return {k: (v[:, 0] if k in SETS else v) for k, v in subcolumn_clouds(cols, tables, seed, 1, clear=clear).items()}


def pick(cl, columns=None, subcolumns=None):
    """The cloud inputs of some columns (in that order) and some subcolumns of each (in that order)."""
    columns = range(cl["thickness"].shape[0]) if columns is None else list(columns)
    out = {"thickness": cl["thickness"][columns]}
    for k in SETS:
        a = cl[k][columns]
        out[k] = a if subcolumns is None else a[:, list(subcolumns)]
    return out


def make(tables, cl):
    return api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), cl["thickness"], *[cl[k] for k in SETS])


def few_layer_clouds(cols, tables, seed, clear=False):
    """cloud_columns' fields for columns of fewer layers than it places its overcast and clear layers in: every layer
    cloudy (liquid and ice) in the first two columns, clear in the third, half cover in the fourth."""
    L = cols[0]["p"].size - 1
    th, sets = [], {k: [] for k in SETS}
    for c, col in enumerate(cols):
        cf = np.full(L, 0.0 if clear else (1.0, 1.0, 0.0, 0.5)[c % 4])
        lwc, iwc = np.where(cf > 0, 0.15, 0.0), np.where(cf > 0, 0.02, 0.0)
        overlap = np.exp(-np.abs(np.diff(np.log(col["p"][1:] + col["p"][:-1]))) / 0.5)
        th.append(29.3 * col["t_layer"] * np.log(col["p"][1:] / col["p"][:-1]))
        draw = np.random.default_rng(seed * 7 + c).random
        for pre in ("lw", "sw"):
            a, b = band_optics(tables, draw, cf, lwc, iwc, overlap, 10.0, col["t_layer"])
            sets[pre + "_liquid"].append(a)
            sets[pre + "_ice"].append(b)
    return dict(thickness=np.array(th), **{k: np.array(v) for k, v in sets.items()})


def clouds_for(cols, tables, seed, clear=False):
    L = cols[0]["p"].size - 1
    if L >= 6:
        return cloud_columns(cols, tables, seed, clear=clear)
    return few_layer_clouds(cols, tables, seed, clear=clear)


# ---- the four base entry points ------------------------------------------------------------------------------------------ #
ENTRIES = ("run", "run_profiles", "run_allsky", "run_allsky_profiles")


def run_entry(pipe, entry, gcols, gclouds, ncol):
    """-> dict(six=[ncol][12] of the set the entry is about (all-sky for the all-sky forms), clear=[ncol][12] or None,
    prof=profiles dict of that set or None)."""
    if entry == "run":
        pipe.run(gcols)
        return dict(six=pipe.fluxes(ncol), clear=None, prof=None, clear_prof=None)
    if entry == "run_profiles":
        pipe.run_profiles(gcols)
        p = pipe.profiles(ncol)
        return dict(six=p["fluxes"], clear=None, prof=p, clear_prof=None)
    if entry == "run_allsky":
        pipe.run_allsky(gcols, gclouds)
        clear, cloudy = pipe.allsky_fluxes(ncol)
        return dict(six=cloudy, clear=clear, prof=None, clear_prof=None)
    pipe.run_allsky_profiles(gcols, gclouds)
    clear, cloudy = pipe.allsky_profiles(ncol)
    return dict(six=cloudy["fluxes"], clear=clear["fluxes"], prof=cloudy, clear_prof=clear)


# ---- the oracle, column by column -------------------------------------------------------------------------------------- #
def heating(up, dn, p):
    """K day-1 of every layer from level fluxes [.., V] and level pressures [V] in mb, levels top first."""
    net = dn - up
    return (GRAVITY / CP) * ((net[..., :-1] - net[..., 1:]) / (100.0 * (p[1:] - p[:-1]))) * 86400.0


def six(up_int, dn_int, user_level):
    """The six rows of grt_pipeline_run's layout from the integrated level fluxes [V]."""
    u = user_level
    return np.array([up_int[0], up_int[-1], up_int[u] if u >= 0 else 0.0,
                     dn_int[0], dn_int[-1], dn_int[u] if u >= 0 else 0.0])


def _solve(orc, band, col, lw, tau, omega, g, emis, alb, solar):
    if lw:
        return orc.lw_fluxes(band.w0, band.dw, col["t_surf"], col["t_layer"], col["t"], tau, omega, emis)
    return orc.sw_fluxes(omega, g, tau, col["mu0"], 0.5, alb, alb, col["tsi"], solar)


def _integrals(orc, band, up, dn):
    return (np.array([orc.integrate_row(r, band.dw) for r in up]), np.array([orc.integrate_row(r, band.dw) for r in dn]))


def oracle_column(orc, lib, band, col, lw, emis=None, alb=None, solar=None, user_level=-1):
    """driver.c:360-424 + 285-356 for one column and band: gas and Rayleigh through add_optics, the solver, the
    -integrated rows."""
    L = col["p"].size - 1
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)
    tau, omega, g = orc.add_optics([tau_gas, tr], [z, om_r], [z, g_r])
    up, dn = _solve(orc, band, col, lw, tau, omega, g, emis, alb, solar)
    rows = [up[0], up[-1], up[user_level] if user_level >= 0 else None,
            dn[0], dn[-1], dn[user_level] if user_level >= 0 else None]
    integ = [orc.integrate_row(r, band.dw) if r is not None else 0.0 for r in rows]
    return dict(tau_gas=tau_gas, tau=tau, omega=omega, g=g, up=up, dn=dn, integ=np.array(integ))


def _cloudy_column(orc, lib, band, col, tables, B):
    """What the subcolumns of one column and band share: the cloud bands' maps onto the driver's band-limit array (no
    cloud where no band lies) and the gas and Rayleigh optics.  -> maps, a function of one subcolumn's (liquid, ice
    [3][B][L], thickness) that gives add_optics of {gas, Rayleigh, liquid, ice}: tau, omega, g."""
    L = col["p"].size - 1
    w = driver_limits(band.w0, band.dw, band.nw)
    (llo, lhi), (ilo, ihi) = limits(tables, "liquid"), limits(tables, "ice")
    maps = (band_map(llo, lhi, B, B, w), band_map(ilo, ihi, ilo.size, B, w))
    tau_gas = band.oracle_tau(orc, orc, lib, col)
    tr, om_r, g_r = orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw)
    z = np.zeros_like(tau_gas)

    def combine(liquid, ice, thickness):
        lt, lo, lg, it, io, ig = grid_optics(liquid, ice, thickness, maps)      # tau = extinction x thickness
        return orc.add_optics([tau_gas, tr, lt, it], [z, om_r, lo, io], [z, g_r, lg, ig])
    return maps, combine


def oracle_allsky_levels(orc, lib, band, col, lw, tables, liquid, ice, thickness, emis=None, alb=None, solar=None):
    """driver.c:474-597 for one column and band with liquid / ice [3][B][L]: the cloud objects of cloud_optics' spreading,
    add_optics of four objects, the solver.  The spectra of every level are kept: up, dn [V][nw], and their integrals
    up_int, dn_int [V]; tau, omega, g and the band maps too."""
    maps, combine = _cloudy_column(orc, lib, band, col, tables, liquid.shape[1])
    tau, omega, g = combine(liquid, ice, thickness)
    up, dn = _solve(orc, band, col, lw, tau, omega, g, emis, alb, solar)
    up_int, dn_int = _integrals(orc, band, up, dn)
    return dict(tau=tau, omega=omega, g=g, maps=maps, up=up, dn=dn, up_int=up_int, dn_int=dn_int)


def oracle_allsky_column(orc, lib, band, col, lw, tables, liquid, ice, thickness, emis=None, alb=None, solar=None,
                         user_level=-1):
    """oracle_allsky_levels and its -integrated six rows, integ."""
    w = oracle_allsky_levels(orc, lib, band, col, lw, tables, liquid, ice, thickness, emis, alb, solar)
    return dict(w, integ=six(w["up_int"], w["dn_int"], user_level))


def oracle_subcolumns(orc, lib, band, col, lw, tables, liquid, ice, thickness, emis=None, alb=None, solar=None):
    """driver.c:503-589 for one column and band with liquid / ice [S][3][B][L]: per subcolumn the cloud objects, add_optics
    of {gas, Rayleigh, liquid, ice}, the solver; the up and down fluxes summed, divided by S; every level integrated."""
    L, S = col["p"].size - 1, liquid.shape[0]
    maps, combine = _cloudy_column(orc, lib, band, col, tables, liquid.shape[2])
    up_sum = np.zeros((L + 1, band.nw))
    dn_sum = np.zeros((L + 1, band.nw))
    for j in range(S):
        tau, omega, g = combine(liquid[j], ice[j], thickness)
        up, dn = _solve(orc, band, col, lw, tau, omega, g, emis, alb, solar)
        up_sum += up
        dn_sum += dn
    up_sum /= float(S)
    dn_sum /= float(S)
    up_int, dn_int = _integrals(orc, band, up_sum, dn_sum)
    return dict(up_int=up_int, dn_int=dn_int, up=up_sum, dn=dn_sum)


def spectral_rows(w, user_level):
    """[6][nw]: the six rows of output_fluxes without -integrated from an oracle result's level spectra up, dn [V][nw]."""
    up, dn = w["up"], w["dn"]
    z = np.zeros(up.shape[1])
    return np.array([up[0], up[-1], up[user_level] if user_level >= 0 else z,
                     dn[0], dn[-1], dn[user_level] if user_level >= 0 else z])


def oracle_rows(orc, lib, band, col, lw, user_level, cloud=None, tables=None, emis=None, alb=None, solar=None):
    """[6][nw]: the six rows of output_fluxes without -integrated, from the oracle's spectra (clear or all-sky)"""
    if cloud is None:
        w = oracle_column(orc, lib, band, col, lw, emis, alb, solar, user_level)
    else:
        w = oracle_allsky_levels(orc, lib, band, col, lw, tables, *cloud, emis, alb, solar)
    return spectral_rows(w, user_level)


def block_edges(n):
    """bins that start or end on a 128-point block boundary or one point either side, and one-interval bins at both ends"""
    e = {0, 1, n - 2, n - 1}
    for k in (128, 256):
        e |= {k - 1, k, k + 1}
    return np.array(sorted(x for x in e if 0 <= x <= n - 1), dtype=np.int32)


@pytest.fixture(scope="module")
def oracle_cache():
    """The oracle's results of one test module, one per key: cached(oracle_cache, key, make).  The oracle is the expensive
    part of a parity case; a key names everything its result depends on (kind, band, column, cloud or aerosol input)."""
    return {}


def cached(cache, key, make):
    if key not in cache:
        cache[key] = make()
    return cache[key]


# ---- checks ------------------------------------------------------------------------------------------------------------ #
def check_levels(got, c, key, col, want_up, want_dn, closure=False):
    """One column, band and set of a profile form: levels against the oracle's, the heating-rate formula and, closure=True,
    energy closure: the column's absorbed flux is the net flux at the top minus the net flux at the surface."""
    up, dn, hr = got[key + "_up"][c], got[key + "_down"][c], got[key + "_heating"][c]
    for name, a, want in (("up", up, want_up), ("down", dn, want_dn)):
        err = np.max(np.abs(a - want))
        assert err < 1e-9, f"{key} {name}: {err} W m-2 from the oracle"
    hmax = np.abs(hr).max()
    assert hmax > 0.0, f"{key}: no heating"
    err = np.max(np.abs(hr - heating(up, dn, col["p"])))
    assert err <= 1e-12 * hmax, f"{key} heating: {err} from the formula on its own levels, largest {hmax}"
    err = np.max(np.abs(hr - heating(want_up, want_dn, col["p"])))
    assert err <= 1e-6 * hmax, f"{key} heating: {err} from the formula on the oracle's levels, largest {hmax}"
    if closure:
        absorbed = np.sum(hr * 100.0 * (col["p"][1:] - col["p"][:-1]) * CP / (GRAVITY * 86400.0))
        fmax = max(np.abs(up).max(), np.abs(dn).max())
        err = abs(absorbed - ((dn[0] - up[0]) - (dn[-1] - up[-1])))
        assert err <= 1e-12 * fmax, f"{key} closure: {err} W m-2, largest flux {fmax}"


# ---- the solver kernels' edge shapes (test_gpu_solver_shapes.py, test_gpu_subcolumn_shapes.py) -------------------------- #
SOLVER_NS = (2, 3, 64, 65, 128, 129, 257)
# first wavenumber of each grid: whole grids inside one cloud band (lw 100-101 cm-1: liquid band 1, sw 2000-2010 cm-1),
# grids across the gap behind liquid band 1 (lw 140-203, 148-150 cm-1) and past the last ice band (sw 8990-9010 cm-1)
LW_W0 = {2: 100.0, 3: 148.0, 64: 140.0, 65: 1.0, 128: 1.0, 129: 100.0, 257: 1.0}
SW_W0 = {2: 2000.0, 3: 8990.0, 64: 1000.0, 65: 1.0, 128: 3000.0, 129: 100.0, 257: 1000.0}
MU0 = (1.0, 0.5, 0.05, 1e-3)       # 0.5 = mu_dif: the two beams share t/mu; 1e-3 clamps tau/mu at 700 in most layers
TRAP_ULPS = 64                      # bound on the partial-sum tree's depth at these n (derived from the code, not measured)
LEVEL_TOL = 1e-10                   # of the column's largest flux
solver_bands = make_shape_bands(SOLVER_NS, LW_W0, SW_W0)


def columns(V):
    cols = [syn.profile(500 + V + c, V) for c in range(len(MU0))]
    for c, mu in zip(cols, MU0):
        c["mu0"] = mu
    return cols


def surface(n, seed):
    """Emissivity and albedo with 0 and 1 at some points (both ends at n = 2)."""
    rng = np.random.default_rng(seed)
    emis, alb = rng.uniform(0.3, 1.0, n), rng.uniform(0.0, 0.7, n)
    emis[0], emis[-1], alb[0], alb[-1] = 0.0, 1.0, 1.0, 0.0
    if n > 3:
        emis[n // 2], alb[n // 2] = 1.0, 0.0
    return emis, alb


def user_index(kind, L):
    return {"-1": -1, "0": 0, "1": 1, "L-1": L - 1, "L": L}[kind]


def exact_trapezoid(f, dw):
    f = [float(x) for x in f]
    pts = [0.5 * f[0]] + f[1:-1] + [0.5 * f[-1]]
    return dw * math.fsum(pts), dw * math.fsum(abs(x) for x in f)


def assert_trapezoid(got, f, dw, what):
    ref, mag = exact_trapezoid(f, dw)
    assert abs(got - ref) <= TRAP_ULPS * 2.0 ** -52 * mag, (what, got, ref, mag)
