"""grt_pipeline_run_sky_zeniths_slant: grt_pipeline_run_sky_zeniths_direct with a sun cosine per layer for the direct beam.
(1) reduction: with every layer's cosine the angle's cos_zenith every output has grt_pipeline_run_sky_zeniths_direct's
bits in the deterministic mode, with and without a GrtZenithSurface_t, through the zenith instances of the solver and the
shared-layer kernel's; (2) oracle: with one layer its cosine is the whole geometry -- the oracle column under that cosine,
times cos_zenith over it; (3) model: cosines drawn per layer, and those of a spherical planet, against slant_model's
restatement; (4) physics: the direct beam of a low sun gains at every level; (5) indexing; (6) refusals.  The shapes are
test_gpu_sky_zenith_shapes.py's, the chunk the slant instances'."""
import ctypes as C

import numpy as np
import pytest

from aerosol_model import oracle_aerosol_optics
from cloud_bands import band_map, driver_limits, grid_optics
from direct_beam_model import three
from grtcode_amd import api, geometry
from pipeline_support import LEVEL_TOL, SOLVER_NS, _deterministic, _sentinel, limits, make, user_index
from pipeline_support import solver_bands as bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from sky_zenith_support import (AEROSOL, ALL, BOTH, CLEAN, CLOUD, NAMES, POOL, aerosols_of, angles, positions, positive_zero,
                                run_sky, run_sky_zeniths)
from slant_model import sw_fluxes as model_fluxes
from surface_support import host_rows
from test_gpu_sky_zeniths_direct import Case, run_zd

pytestmark = pytest.mark.gpu

assert api.GRT_ZENITH_CHUNK_SLANT == api.GRT_ZENITH_CHUNK_SLANT_SURFACE      # (one set of angle counts serves both)
ZN = api.GRT_ZENITH_CHUNK_SLANT
ZS = (1, ZN - 1, ZN, ZN + 1, 2 * ZN + 1)
NS = (2, 65, 129, 257)
RADIUS = geometry.EARTH_RADIUS

# grid length, levels, angles, draws, sets, user level, where the night samples are, knots
CASES = [(2, 2, ZS[0], 1, CLEAN, "-1", "none", 2), (65, 3, ZS[1], 2, AEROSOL, "0", "none", 3),
         (129, 16, ZS[2], 3, CLOUD, "L", "some", 9), (257, 2, ZS[3], 1, BOTH, "1", "last_chunk", 2),
         (65, 16, ZS[4], 2, ALL, "L-1", "last_chunk", 3), (129, 3, ZS[3], 3, ALL, "1", "some", 9),
         (257, 16, ZS[2], 2, ALL, "-1", "all", 3), (2, 3, ZS[4], 1, ALL, "0", "some", 2)]
assert {c[0] for c in CASES} == set(NS) <= set(SOLVER_NS) and {c[1] for c in CASES} == {2, 3, 16}
assert {c[2] for c in CASES} == set(ZS) and {c[3] for c in CASES} == {1, 2, 3}
assert {c[4] for c in CASES} >= {CLEAN, AEROSOL, CLOUD, BOTH, ALL} and {c[5] for c in CASES} == {"-1", "0", "1", "L-1", "L"}
assert {c[6] for c in CASES} == {"none", "some", "last_chunk", "all"}


def run_zs(pipe, x, sets, mu, wt, cosines, gsurf, direct, profiles, gcols=None, gclouds=None, gaer=None, ncol=None):
    """grt_pipeline_run_sky_zeniths_slant -> one dict, run_zd()'s keys (cosines None: slant == NULL)."""
    gsky, keep = api.make_sky(gclouds or x.gclouds, gaer or x.gaer, x.S, sets)
    gz, keep_z = api.make_zeniths(mu, wt)
    gslant = None
    if cosines is not None:
        gslant, keep_s = api.make_zenith_slant(cosines)
    pipe.run_sky_zeniths_slant(gcols or x.gcols, gsky, gz, gslant, gsurface=gsurf, direct=direct, profiles=profiles)
    n = x.ncol if ncol is None else ncol
    if profiles:
        return pipe.sky_zenith_direct_profiles(n, keep["nsets"], mu.shape[1])
    return pipe.sky_zenith_direct_fluxes(n, keep["nsets"], mu.shape[1])


def flat(mu, L, night=np.nan):
    """[ncol][Z][L]: every layer at the angle's own cosine; a night angle's entries `night` (they are not read)."""
    out = np.repeat(mu[:, :, None], L, axis=2)
    out[~(mu > 0.0)] = night
    return out


def drawn(mu, L, seed):
    """[ncol][Z][L] from POOL, another draw per (column, angle, layer): some layers clamp tau/mu at 700 and their neighbours
    do not; a night angle's entries are NaN."""
    rng = np.random.default_rng(seed)
    out = np.asarray(POOL)[rng.integers(0, len(POOL), mu.shape + (L,))]
    out[~(mu > 0.0)] = np.nan
    return out


def spherical(x, mu):
    """grt_slant_cosines over the hypsometric heights of the batch's columns."""
    h = np.stack([geometry.level_heights(col["p"], col["t_layer"]) for col in x.cols])
    return geometry.slant_cosines(RADIUS, h, mu)


def set_optics(name, orc, lib, x, c):
    """The draws of set `name` of column c of the shortwave band: [(tau, omega, g)], the objects combined as
    sky_zenith_support.oracle_sky combines them."""
    band, col, tables = x.swb, x.cols[c], x.tables
    L = col["p"].size - 1
    gas = x.__dict__.setdefault("gas_of_column", {})         # (the oracle's gas optics of a column: once per batch)
    if c not in gas:
        gas[c] = (band.oracle_tau(orc, orc, lib, col),) + tuple(orc.rayleigh(L, col["p"], band.w0, band.dw, band.nw))
    tau_gas, tr, om_r, g_r = gas[c]
    z = np.zeros_like(tau_gas)
    taus, omegas, gs = [tau_gas, tr], [z, om_r], [z, g_r]
    if name in ("aerosol", "both"):
        aer = oracle_aerosol_optics(orc, band, x.xs[1], x.f[1][c])
        taus, omegas, gs = taus + [aer[0]], omegas + [aer[1]], gs + [aer[2]]
    draws = [None]
    if name in ("cloud", "both"):
        liquid, ice = x.cl["sw_liquid"][c], x.cl["sw_ice"][c]
        B = liquid.shape[2]
        w = driver_limits(band.w0, band.dw, band.nw)
        (llo, lhi), (ilo, ihi) = limits(tables, "liquid"), limits(tables, "ice")
        maps = (band_map(llo, lhi, B, B, w), band_map(ilo, ihi, ilo.size, B, w))
        draws = [grid_optics(liquid[j], ice[j], x.cl["thickness"][c], maps) for j in range(liquid.shape[0])]
    out = []
    for d in draws:
        t, o, g = (taus, omegas, gs) if d is None else (taus + [d[0], d[3]], omegas + [d[1], d[4]], gs + [d[2], d[5]])
        out.append(orc.add_optics(t, o, g))
    return out


def reference(orc, x, c, optics, mu0, cosines, alb_dir, alb_dif, oracle_under=None):
    """up_int, dn_int, direct [V] of column c under mu0 with the layer cosines `cosines` [L]: per draw slant_model's solver
    -- oracle_under (one layer: its cosine): the oracle's solver under that cosine, times mu0 over it -- each level
    integrated with the oracle's trapezoid, then the mean over the draws in order."""
    col, band = x.cols[c], x.swb
    total = None
    for tau, omega, g in optics:
        if oracle_under is None:
            fields = model_fluxes(omega, g, tau, cosines, 0.5, alb_dir, alb_dif, col["tsi"], x.solar, mu0)
        else:
            up, dn = orc.sw_fluxes(omega, g, tau, oracle_under, 0.5, alb_dir, alb_dif, col["tsi"], x.solar)
            fields = (up * (mu0 / oracle_under), dn * (mu0 / oracle_under))
        rows = [np.array([orc.integrate_row(r, band.dw) for r in a]) for a in fields]
        total = rows if total is None else [a + b for a, b in zip(total, rows)]
    return [a / float(len(optics)) for a in total]


def check_reference(orc, lib, x, case, sets, mu, cosines, with_surface, user_level, six_rows, prof, oracle):
    """(2), (3): the first and the last day angle of the first and the last column, every set."""
    grid = api.create_spectral_grid(x.swb.w0, x.swb.wn, x.swb.dw)
    for c in sorted({0, x.ncol - 1}):
        days = [k for k in range(mu.shape[1]) if mu[c, k] > 0.0]
        for name, at in positions(sets).items():
            optics = set_optics(name, orc, lib, x, c)
            for k in sorted({days[0], days[-1]} if days else ()):
                alb_dir = host_rows(lib, grid, case.xa, case.knots[c, k:k + 1])[0] if with_surface else x.alb
                want = reference(orc, x, c, optics, mu[c, k], cosines[c, k], alb_dir, x.alb,
                                 oracle_under=cosines[c, k, 0] if oracle else None)
                ff = max(np.abs(want[0]).max(), np.abs(want[1]).max())
                want6 = np.concatenate([three(want[0], user_level), three(want[1], user_level)])
                errs = [np.max(np.abs(six_rows["angle_fluxes"][c, at, k] - want6)),
                        np.max(np.abs(prof["angle_fluxes"][c, at, k] - want6)),
                        np.max(np.abs(prof["angle_up"][c, at, k] - want[0])),
                        np.max(np.abs(prof["angle_down"][c, at, k] - want[1]))]
                if not oracle:
                    errs += [np.max(np.abs(six_rows["angle_direct"][c, at, k] - three(want[2], user_level))),
                             np.max(np.abs(prof["angle_direct"][c, at, k] - three(want[2], user_level))),
                             np.max(np.abs(prof["angle_direct_levels"][c, at, k] - want[2]))]
                print("oracle" if oracle else "model", "column", c, "angle", k, name, "errors", errs, "of", LEVEL_TOL * ff)
                assert ff > 0.0 and max(errs) <= LEVEL_TOL * ff, (c, k, name, errs, ff)


@pytest.mark.parametrize("n,V,Z,S,sets,ul,night,nk", CASES,
                         ids=[f"n{n}-V{V}-Z{Z}-S{S}-sets{s}-ul{u}-night_{w}-knots{q}" for n, V, Z, S, s, u, w, q in CASES])
def test_reduction_oracle_and_model_at_edge_shapes(bands, tables, oracle, lib, device, monkeypatch, n, V, Z, S, sets, ul, night, nk):
    """(1), (2) and (3): deterministic mode, fast = 0, three columns."""
    L, user_level = V - 1, user_index(ul, V - 1)
    case = Case(bands, tables, device, n, V, Z, S, nk)
    x = case.x
    mu = angles(x.ncol, Z, night, ZN)
    wt = np.array([[0.25 + 0.125 * ((c + 3 * k) % 5) for k in range(Z)] for c in range(x.ncol)])
    A = case.pipeline(user_level, False, in_force=False)
    _deterministic(lib, True)
    try:
        # ---- (1) every layer at the angle's own cosine: grt_pipeline_run_sky_zeniths_direct's bits ---------------------- #
        same = flat(mu, L)
        for gsurf in (case.gsurf, None):
            want = {p: run_zd(A, x, sets, mu, wt, gsurf, True, p) for p in (False, True)}
            for value in ("0", "1", None):
                if value is not None:
                    monkeypatch.setenv("GRT_ZENITH_SHARED", value)
                got = {p: run_zs(A, x, sets, mu, wt, same, gsurf, True, p) for p in (False, True)}
                bare = run_zs(A, x, sets, mu, wt, same, gsurf, False, False)
                if value is not None:
                    monkeypatch.delenv("GRT_ZENITH_SHARED")
                for p in (False, True):
                    assert set(got[p]) == set(want[p])
                    for key in want[p]:
                        assert np.array_equal(got[p][key], want[p][key]), (gsurf is not None, value, p, key)
                # (without a GrtZenithDirect_t the instances still carry the direct beam; its rows are not returned)
                assert "direct" not in bare and "angle_direct" not in bare
                for key in bare:
                    assert np.array_equal(bare[key], want[False][key]), (gsurf is not None, value, key)
            # slant == NULL is that call
            none = run_zs(A, x, sets, mu, wt, None, gsurf, True, True)
            for key in want[True]:
                assert np.array_equal(none[key], want[True][key]), (gsurf is not None, key)
        # two sweeps: the six-row form's rows are the profile form's
        cosines = drawn(mu, L, 3 * n + Z)
        prof = run_zs(A, x, sets, mu, wt, cosines, case.gsurf, True, True)
        six_rows = run_zs(A, x, sets, mu, wt, cosines, case.gsurf, True, False)
        monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
        s2 = run_zs(A, x, sets, mu, wt, cosines, case.gsurf, True, False)
        monkeypatch.delenv("GRT_SW_TWO_SWEEPS")
        for key in ("fluxes", "angle_fluxes", "direct", "angle_direct"):
            assert np.array_equal(s2[key], prof[key]), key
        # the solver's zenith instances and the shared-layer kernel's: the same bits under cosines per layer too
        for value in ("0", "1"):
            monkeypatch.setenv("GRT_ZENITH_SHARED", value)
            s1 = run_zs(A, x, sets, mu, wt, cosines, case.gsurf, True, False)
            monkeypatch.delenv("GRT_ZENITH_SHARED")
            for key in six_rows:
                assert np.array_equal(s1[key], six_rows[key]), (value, key)
        for out in (six_rows, prof):
            for key in [q for q in out if q.startswith("angle_")]:
                assert positive_zero(np.moveaxis(out[key], 2, 1)[~(mu > 0.0)]), key
        # ---- (2) one layer: the oracle column under the layer's cosine; (3) more: slant_model ---------------------------- #
        check_reference(oracle, lib, x, case, sets, mu, cosines, True, user_level, six_rows, prof, oracle=V == 2)
        if V > 2:
            # a spherical planet's cosines over the columns' own heights, the surface in force under every angle
            real = spherical(x, mu)
            prof = run_zs(A, x, sets, mu, wt, real, None, True, True)
            six_rows = run_zs(A, x, sets, mu, wt, real, None, True, False)
            check_reference(oracle, lib, x, case, sets, mu, real, False, user_level, six_rows, prof, oracle=False)
    finally:
        _deterministic(lib, False)
    A.destroy()
    x.destroy()


# ---- (4) physics ----------------------------------------------------------------------------------------------------- #
def test_a_low_sun_keeps_more_of_its_direct_beam(bands, tables, lib, device):
    """Real heights, cos_zenith in {0.05, 1e-3, 1}: every layer's cosine on the sphere is at least the angle's own, so the
    direct beam at every level is at least the plane-parallel run's, and more at the surface wherever that is not 0; under
    an overhead sun the two runs agree bit for bit."""
    n, V, S = 129, 16, 2
    case = Case(bands, tables, device, n, V, 3, S, 3)
    x = case.x
    mu = np.array([[0.05, 1e-3, 1.0], [1e-3, 1.0, 0.05], [1.0, 0.05, 1e-3]])
    cosines = spherical(x, mu)
    assert np.all(cosines[mu == 1.0] == 1.0) and np.all(cosines >= mu[:, :, None])
    pipe = case.pipeline(5, False)
    _deterministic(lib, True)
    try:
        for profiles in (False, True):
            plane = run_zd(pipe, x, ALL, mu, None, case.gsurf, True, profiles)
            sphere = run_zs(pipe, x, ALL, mu, None, cosines, case.gsurf, True, profiles)
            overhead = mu == 1.0
            for key in plane:
                if key.startswith("angle_"):
                    a, b = (np.moveaxis(o[key], 2, 1) for o in (sphere, plane))
                    assert np.array_equal(a[overhead], b[overhead]), key
            for key in ("angle_direct", "angle_direct_levels") if profiles else ("angle_direct",):
                a, b = (np.moveaxis(o[key], 2, 1)[~overhead] for o in (sphere, plane))
                assert np.all(a >= b), key
                surface = (slice(None), slice(None), -1 if key == "angle_direct_levels" else 1)
                lit = b[surface] != 0.0
                assert np.all(a[surface][lit] > b[surface][lit]), key
                # (the top of the atmosphere is the scale alone)
                assert np.array_equal(a[:, :, 0], b[:, :, 0]), key
            horizon = np.moveaxis(sphere["angle_direct"], 2, 1)[mu == 1e-3][:, 0, 1]
            flat_horizon = np.moveaxis(plane["angle_direct"], 2, 1)[mu == 1e-3][:, 0, 1]
            print("clean-sky surface direct beam at mu0 = 1e-3: sphere", horizon, "plane", flat_horizon)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    x.destroy()


# ---- (5) indexing ---------------------------------------------------------------------------------------------------- #
def test_indexing(bands, tables, lib, device):
    """Permuting the angles together with their cosine rows (and knots) permutes the output rows; a column alone has the
    bits it has in its batch; a subset of the set mask gives each set the bits of the four-set run; the longwave rows are
    grt_pipeline_run_sky's."""
    n, V, Z, S, nk = 129, 16, ZN + 1, 2, 3
    case = Case(bands, tables, device, n, V, Z, S, nk)
    x = case.x
    ncol, L = x.ncol, V - 1
    mu = angles(ncol, Z, "none", ZN)
    mu[2, 2] = -0.1
    cosines = drawn(mu, L, 17)
    pipe = case.pipeline(V - 2, False, in_force=False)
    _deterministic(lib, True)
    try:
        full = {p: run_zs(pipe, x, ALL, mu, None, cosines, case.gsurf, True, p) for p in (False, True)}
        order = np.array([(3 * k + 1) % Z for k in range(Z)])
        assert sorted(order) == list(range(Z))
        gperm, keep_perm = api.make_zenith_surface(case.xa, case.knots[:, order])
        for p in (False, True):
            got = run_zs(pipe, x, ALL, mu[:, order], None, cosines[:, order], gperm, True, p)
            for key in [q for q in got if q.startswith("angle_")]:
                assert np.array_equal(got[key], full[p][key][:, :, order]), (p, key)
        for sets in (CLEAN, AEROSOL, CLOUD, BOTH, AEROSOL | CLOUD):
            part = run_zs(pipe, x, sets, mu, None, cosines, case.gsurf, True, True)
            for name, at in positions(sets).items():
                for key in part:
                    assert np.array_equal(part[key][:, at], full[True][key][:, NAMES.index(name)]), (sets, name, key)
        for c in (0, ncol - 1):
            g1, keep1 = api.make_columns([x.cols[c]], MOL_ORDER, cfc_order=(0, 1))
            gc1, keep_c1 = make(tables, {k: v[c:c + 1] for k, v in x.cl.items()})
            ga1, keep_a1 = aerosols_of(tuple(f[c:c + 1] for f in x.f), x.xs)
            gs1, keep_s1 = api.make_zenith_surface(case.xa, case.knots[c:c + 1])
            for p in (False, True):
                one = run_zs(pipe, x, ALL, mu[c:c + 1], None, cosines[c:c + 1], gs1, True, p, gcols=g1, gclouds=gc1, gaer=ga1,
                             ncol=1)
                for key in one:
                    assert np.array_equal(one[key][0], full[p][key][c]), (c, p, key)
        sky = run_sky(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, ncol, True)
        for key in ("lw_up", "lw_down", "lw_heating"):
            assert np.array_equal(full[True][key], sky[key]), key
        assert np.array_equal(full[False]["fluxes"][:, :, :6], run_sky(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, ncol, False)["fluxes"][:, :, :6])
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    x.destroy()


def test_a_pipeline_without_a_shortwave_band(bands, tables, lib, device):
    """It runs the longwave and writes +0.0 to every shortwave and direct output."""
    n, V, Z, S = 65, 3, 3, 2
    case = Case(bands, tables, device, n, V, Z, S, 3)
    x = case.x
    ncol = x.ncol
    mu = angles(ncol, Z, "none", ZN)
    pipe = api.Pipeline(x.go_lw, None, ncol, 0, x.emis, None, None, spectral=False)
    want = api.Pipeline(x.go_lw, None, ncol, 0, x.emis, None, None, spectral=False)
    _deterministic(lib, True)
    try:
        for p in (False, True):
            got = run_zs(pipe, x, ALL, mu, None, drawn(mu, V - 1, 5), case.gsurf, True, p)
            sky = run_sky(want, x.gcols, x.gclouds, x.gaer, S, ALL, ncol, p)
            for key in [k for k in got if k.startswith("angle_") or k in ("direct", "direct_levels")]:
                assert positive_zero(got[key]), (p, key)
            for key in sky:
                assert np.array_equal(got[key], sky[key]), (p, key)
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    want.destroy()
    x.destroy()


# ---- (6) refusals ---------------------------------------------------------------------------------------------------- #
def test_refused_inputs(bands, tables, lib, device):
    """Each refusal returns GRTCODE_VALUE_ERR with sentinel-filled outputs untouched; afterwards
    grt_pipeline_run_sky_zeniths gives the bits it gave before."""
    n, V, Z, S, nk = 65, 3, 3, 2, 3
    case = Case(bands, tables, device, n, V, Z, S, nk)
    x = case.x
    ncol, L = x.ncol, V - 1
    pipe, mat = case.pipeline(-1, False), case.pipeline(-1, True)
    mu = angles(ncol, Z, "none", ZN)
    good = drawn(mu, L, 9)
    _deterministic(lib, True)
    before = {p: run_sky_zeniths(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, mu, None, ncol, p) for p in (False, True)}
    rows = (4 * V, 2 * (V - 1), 12, Z * 6, Z * 2 * V, 3, V, Z * 3, Z * V)
    sizes = [4 * r * (ncol + 1) for r in rows]
    bufs = [_sentinel(device, k) for k in sizes]

    def call(gsky, gz, gslant, gsurf, gdirect, form, gcols=None, on=None):
        gz.zenith_fluxes_dev = bufs[3].ptr
        gz.zenith_level_fluxes_dev = bufs[4].ptr if form == "profile" else None
        outs = [b.ptr for b in bufs[:3]] if form == "profile" else [None, None, bufs[2].ptr]
        return lib.grt_pipeline_run_sky_zeniths_slant((on or pipe).p, C.byref(gcols or x.gcols),
                                                      None if gsky is None else C.byref(gsky), C.byref(gz),
                                                      None if gslant is None else C.byref(gslant),
                                                      None if gsurf is None else C.byref(gsurf),
                                                      None if gdirect is None else C.byref(gdirect), *outs)

    def direct_of(form, which=(0, 1, 2, 3)):
        ptrs = [bufs[5 + k].ptr if k in which and (form == "profile" or k in (0, 2)) else None for k in range(4)]
        return api.GrtZenithDirect(ptrs[0], ptrs[1], ptrs[2], ptrs[3])

    def refused(cosines=good, gsurf=case.gsurf, direct=True, sets=ALL, cos=mu, weight=None, gclouds=x.gclouds, S_=S,
                which=(0, 1, 2, 3), forms=("profile", "six"), levels_in_six=None, gcols=None, null_array=False, on=None):
        gsky, ks = api.make_sky(gclouds, x.gaer, S_, sets)
        for form in forms:
            gz, kz = api.make_zeniths(cos, weight)
            gslant, keep_s = (None, None) if cosines is None else api.make_zenith_slant(cosines)
            if null_array:
                gslant.layer_cos_zenith = None
            gdirect = direct_of(form, which) if direct else None
            if levels_in_six is not None:
                setattr(gdirect, levels_in_six, bufs[6].ptr if levels_in_six == "direct_level_fluxes_dev" else bufs[8].ptr)
            with pytest.raises(api.GrtError) as e:
                api.check(call(gsky, gz, gslant, gsurf, gdirect, form, gcols, on))
            assert e.value.code == api.VALUE_ERR, e.value
        (on or pipe).sync()
        for b, k in zip(bufs, sizes):
            assert np.all(b.to_host((k,)) == -7.25)

    try:
        # ---- everything grt_pipeline_run_sky_zeniths_direct refuses (test_gpu_sky_zeniths_direct.py has the whole list)
        refused(sets=16)
        refused(gclouds=None)
        refused(S_=0)
        m = mu.copy()
        m[1, 1] = 1.0 + 1e-12
        refused(cos=m)
        w = np.ones_like(mu)
        w[0, 2] = -1e-300
        refused(weight=w)
        big, keep_big = api.make_columns(x.cols + x.cols[:1], MOL_ORDER, cfc_order=(0, 1))
        refused(gcols=big)
        refused(which=())
        for field in ("direct_level_fluxes_dev", "zenith_direct_level_fluxes_dev"):
            refused(forms=("six",), levels_in_six=field)
        g, k = api.make_zenith_surface(case.xa, case.knots.copy())
        k["direct_albedo"][1, 1, 1] = 1.0 + 1e-12
        refused(gsurf=g)
        g, k = api.make_zenith_surface(case.xa, case.knots)
        g.albedo_num_points = 1
        refused(gsurf=g)
        # (slant == NULL is grt_pipeline_run_sky_zeniths_direct: surface and direct both NULL is refused there)
        refused(cosines=None, gsurf=None, direct=False)
        # ---- a NULL array; a day sample's layer cosine that is not finite, is <= 0 or is > 1
        refused(null_array=True)
        for bad, where in ((np.nan, (0, 0, 0)), (np.inf, (1, 1, L - 1)), (-np.inf, (2, 0, 1)), (0.0, (ncol - 1, Z - 1, L - 1)),
                           (-0.0, (0, 1, 0)), (-1e-300, (1, 2, 1)), (1.0 + 1e-12, (2, 2, 0)), (-0.5, (1, 0, 0))):
            c = good.copy()
            c[where] = bad
            refused(cosines=c)
            refused(cosines=c, gsurf=None, direct=False, forms=("six",))
        # ---- a pipeline in the materialised form
        refused(on=mat)
        refused(on=mat, gsurf=None, direct=False)
        # ---- afterwards: the bits of before; a night sample's cosines are not read; an accepted call writes what it was given
        for p in (False, True):
            after = run_sky_zeniths(pipe, x.gcols, x.gclouds, x.gaer, S, ALL, mu, None, ncol, p)
            for key in after:
                assert np.array_equal(after[key], before[p][key]), (p, key)
        night = mu.copy()
        night[1, 1], night[0, 2] = -0.5, 0.0
        c = good.copy()
        c[1, 1], c[0, 2] = (np.nan, -3.0), (7.0, np.inf)
        gsky, ks = api.make_sky(x.gclouds, x.gaer, S, ALL)
        gz, kz = api.make_zeniths(night)
        gslant, keep_s = api.make_zenith_slant(c)
        api.check(call(gsky, gz, gslant, None, direct_of("profile", which=(0, 2)), "profile"))
        pipe.sync()
        for at, r in ((5, 3), (7, Z * 3)):
            got = bufs[at].to_host((ncol + 1, 4 * r))
            assert np.all(np.isfinite(got[:ncol])) and np.all(got[:ncol] != -7.25) and np.all(got[ncol] == -7.25)
        for at in (6, 8):
            assert np.all(bufs[at].to_host((sizes[at],)) == -7.25)
    finally:
        _deterministic(lib, False)
    for b in bufs:
        b.free()
    pipe.destroy()
    mat.destroy()
    x.destroy()
