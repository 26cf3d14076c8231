"""grt_pipeline_run_zeniths: the clear-clean set under several sun angles per column on one gas-optics pass.  Every day
angle's six rows and level fluxes against the oracle's column run with that cos(zenith), night angles exactly zero, the
weighted mean against numpy's sum of the oracle rows, fused and materialised form; one run in the production arithmetic
against the project's flux contract; in the deterministic mode the bit-for-bit identities with grt_pipeline_run and
grt_pipeline_run_profiles fed one angle at a time; and what the call refuses."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api
from pipeline_support import (_deterministic, _sentinel, _setup, cached, check_levels, heating, oracle_column,
                              six)
from pipeline_support import bands, oracle_cache  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from test_gpu_pipeline_production import FLUX_TOL, note, varied_columns
from test_gpu_solver_shapes import LEVEL_TOL

pytestmark = pytest.mark.gpu

V, NCOL = 16, 3
L = V - 1
ANGLES = (1.0, 0.5, 0.05, 1e-3, -0.2)       # 0.5 = mu_dif; 1e-3 clamps tau/mu at 700; one night sample
Z = len(ANGLES)


def case_columns():
    return varied_columns(860, V, NCOL)


def case_angles():
    """[NCOL][Z]: the angles in another order per column, and weights that do not sum to one."""
    mu = np.array([np.roll(ANGLES, c) for c in range(NCOL)])
    w = np.array([[0.05 + 0.1 * ((3 * c + 2 * k) % 7) for k in range(Z)] for c in range(NCOL)])
    return mu, w


def oracle_angle(cache, oracle, lib, band, c, col, mu, surface, user_level):
    """oracle_column of the shortwave band for column c under cos(zenith) mu, its level integrals added."""
    emis, alb, solar = surface

    def make():
        w = oracle_column(oracle, lib, band, dict(col, mu0=mu), False, emis, alb, solar, user_level)
        w["up_int"] = np.array([oracle.integrate_row(r, band.dw) for r in w["up"]])
        w["dn_int"] = np.array([oracle.integrate_row(r, band.dw) for r in w["dn"]])
        return w
    return cached(cache, ("sw", c, mu, user_level), make)


def check_six_rows(got6, w, user_level, what):
    ff = max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
    assert ff > 0.0, what
    err = np.max(np.abs(got6 - w["integ"]))
    assert err <= LEVEL_TOL * ff, f"{what}: six rows {err} W m-2 from the oracle, largest flux {ff}"
    assert np.array_equal(w["integ"], six(w["up_int"], w["dn_int"], user_level)), what


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
@pytest.mark.parametrize("user_level", [-1, 5], ids=["one_sweep", "two_sweeps"])
def test_every_angle_and_the_mean_match_the_oracle(bands, oracle_cache, oracle, lib, device, user_level, spectral):
    lwb, swb = bands
    cols = case_columns()
    mu, wt = case_angles()
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V, fast=0)
    surface = (emis, alb, solar)
    pipe = api.Pipeline(go_lw, go_sw, NCOL, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gcols.cos_zenith = None                      # (the entry point does not read it)
    for weights in (None, wt):
        gz, keep_z = api.make_zeniths(mu, weights)
        coef = weights if weights is not None else np.full((NCOL, Z), 1.0 / Z)
        pipe.run_zeniths(gcols, gz)
        fluxes, angles = pipe.zenith_fluxes(NCOL, Z)
        pipe.run_zeniths(gcols, gz, profiles=True)
        prof = pipe.zenith_profiles(NCOL, Z)
        for c, col in enumerate(cols):
            lw = cached(oracle_cache, ("lw", c, user_level), lambda: oracle_column(
                oracle, lib, lwb, col, True, emis, alb, solar, user_level))
            ff = max(abs(oracle.integrate_row(r, lwb.dw)) for r in list(lw["up"]) + list(lw["dn"]))
            assert np.max(np.abs(fluxes[c, :6] - lw["integ"])) <= LEVEL_TOL * ff
            mean6, mean_up, mean_dn, bound = np.zeros(6), np.zeros(V), np.zeros(V), 0.0
            for k in range(Z):
                what = f"column {c} angle {k} (mu {mu[c, k]})"
                if mu[c, k] <= 0.0:
                    assert np.all(angles[c, k] == 0.0) and np.all(prof["angle_fluxes"][c, k] == 0.0), what
                    assert np.all(prof["angle_up"][c, k] == 0.0) and np.all(prof["angle_down"][c, k] == 0.0), what
                    continue
                w = oracle_angle(oracle_cache, oracle, lib, swb, c, col, mu[c, k], surface, user_level)
                check_six_rows(angles[c, k], w, user_level, what)
                check_six_rows(prof["angle_fluxes"][c, k], w, user_level, what + " profile form")
                up, dn = prof["angle_up"][:, k], prof["angle_down"][:, k]
                own = {"sw_up": up, "sw_down": dn, "sw_heating": heating(up, dn, col["p"])}
                check_levels(own, c, "sw", col, w["up_int"], w["dn_int"])
                bound += coef[c, k] * LEVEL_TOL * max(np.abs(w["up_int"]).max(), np.abs(w["dn_int"]).max())
                mean6 += coef[c, k] * w["integ"]
                mean_up += coef[c, k] * w["up_int"]
                mean_dn += coef[c, k] * w["dn_int"]
            assert np.max(np.abs(fluxes[c, 6:] - mean6)) <= bound, (c, weights is None)
            assert np.max(np.abs(prof["fluxes"][c, 6:] - mean6)) <= bound, (c, weights is None)
            check_levels(prof, c, "sw", col, mean_up, mean_dn)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_production_form_meets_the_flux_contract(bands, oracle_cache, oracle, lib, device):
    """fast = 3 (the arithmetic a new gas-optics object runs) against the oracle at 1e-3 W m-2."""
    lwb, swb = bands
    cols = case_columns()
    mu, wt = case_angles()
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V, fast=3)
    pipe = api.Pipeline(go_lw, go_sw, NCOL, -1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gz, keep_z = api.make_zeniths(mu, wt)
    pipe.run_zeniths(gcols, gz)
    fluxes, angles = pipe.zenith_fluxes(NCOL, Z)
    assert go_lw.last_launch()["fast"] == 3 and go_sw.last_launch()["fast"] == 3
    worst = 0.0
    for c, col in enumerate(cols):
        mean6 = np.zeros(6)
        for k in range(Z):
            if mu[c, k] <= 0.0:
                assert np.all(angles[c, k] == 0.0)
                continue
            w = oracle_angle(oracle_cache, oracle, lib, swb, c, col, mu[c, k], (emis, alb, solar), -1)
            worst = max(worst, note(lib, "run_zeniths", "flux_w_m2", np.max(np.abs(angles[c, k] - w["integ"])), FLUX_TOL))
            mean6 += wt[c, k] * w["integ"]
        worst = max(worst, note(lib, "run_zeniths", "flux_w_m2", np.max(np.abs(fluxes[c, 6:] - mean6)), FLUX_TOL))
    print(f"run_zeniths, production form: worst flux error {worst:.3e} W m-2 (bound {FLUX_TOL})")
    assert worst <= FLUX_TOL
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def day_columns(cols, mu_k):
    """The columns under one angle each; a night sample's column runs under 1.0 and is not compared."""
    return [dict(col, mu0=(m if m > 0.0 else 1.0)) for col, m in zip(cols, mu_k)]


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
@pytest.mark.parametrize("user_level", [-1, 5], ids=["one_sweep", "two_sweeps"])
def test_bit_identities(bands, lib, device, monkeypatch, user_level, spectral):
    cols = case_columns()
    mu, wt = case_angles()
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V, fast=0)
    pipe = api.Pipeline(go_lw, go_sw, NCOL, user_level, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gz, keep_z = api.make_zeniths(mu, wt)
    _deterministic(lib, True)
    try:
        pipe.run_zeniths(gcols, gz)
        fluxes, angles = pipe.zenith_fluxes(NCOL, Z)
        pipe.run_zeniths(gcols, gz, profiles=True)
        prof = pipe.zenith_profiles(NCOL, Z)
        # each angle's rows are grt_pipeline_run's (run_profiles') fed that angle; the longwave rows are run's
        for k in range(Z):
            g1, k1 = api.make_columns(day_columns(cols, mu[:, k]), MOL_ORDER, cfc_order=(0, 1))
            pipe.run(g1)
            one = pipe.fluxes(NCOL)
            pipe.run_profiles(g1)
            p1 = pipe.profiles(NCOL)
            assert np.array_equal(fluxes[:, :6], one[:, :6]) and np.array_equal(prof["fluxes"][:, :6], p1["fluxes"][:, :6])
            assert np.array_equal(prof["lw_up"], p1["lw_up"]) and np.array_equal(prof["lw_heating"], p1["lw_heating"])
            day = mu[:, k] > 0.0
            assert np.array_equal(angles[day, k], one[day, 6:]), k
            assert np.array_equal(prof["angle_up"][day, k], p1["sw_up"][day]), k
            assert np.array_equal(prof["angle_down"][day, k], p1["sw_down"][day]), k
            assert np.array_equal(prof["angle_fluxes"][day, k], p1["fluxes"][day, 6:]), k
            assert np.all(angles[~day, k] == 0.0) and np.all(prof["angle_up"][~day, k] == 0.0)
            # Z = 1 without weights is run (run_profiles)
            gz1, kz1 = api.make_zeniths(np.where(day, mu[:, k], 1.0)[:, None])
            pipe.run_zeniths(gcols, gz1)
            f1, a1 = pipe.zenith_fluxes(NCOL, 1)
            assert np.array_equal(f1, one) and np.array_equal(a1[:, 0], one[:, 6:]), k
            pipe.run_zeniths(gcols, gz1, profiles=True)
            z1 = pipe.zenith_profiles(NCOL, 1)
            assert all(np.array_equal(z1[key], p1[key]) for key in p1), k
        # the mean is the fold of the angles' rows in order, each product rounded
        acc = wt[:, 0, None] * angles[:, 0]
        for k in range(1, Z):
            acc = acc + wt[:, k, None] * angles[:, k]
        assert np.array_equal(fluxes[:, 6:], acc)
        # the shared-layer kernel and the zenith instance of the six-row solver
        monkeypatch.setenv("GRT_ZENITH_SHARED", "0")
        pipe.run_zeniths(gcols, gz)
        f0, a0 = pipe.zenith_fluxes(NCOL, Z)
        monkeypatch.delenv("GRT_ZENITH_SHARED")
        assert np.array_equal(f0, fluxes) and np.array_equal(a0, angles)
        # a column alone is the column in its batch
        for c in range(NCOL):
            g1, k1 = api.make_columns([cols[c]], MOL_ORDER, cfc_order=(0, 1))
            gz1, kz1 = api.make_zeniths(mu[c: c + 1], wt[c: c + 1])
            pipe.run_zeniths(g1, gz1)
            f1, a1 = pipe.zenith_fluxes(1, Z)
            assert np.array_equal(f1[0], fluxes[c]) and np.array_equal(a1[0], angles[c]), c
            pipe.run_zeniths(g1, gz1, profiles=True)
            z1 = pipe.zenith_profiles(1, Z)
            assert all(np.array_equal(z1[key][0], prof[key][c]) for key in prof), c
        # permuting the angles permutes the per-angle outputs
        order = [3, 0, 4, 2, 1]
        gzp, kzp = api.make_zeniths(mu[:, order], wt[:, order])
        pipe.run_zeniths(gcols, gzp)
        fp, ap = pipe.zenith_fluxes(NCOL, Z)
        assert np.array_equal(ap, angles[:, order]) and np.array_equal(fp[:, :6], fluxes[:, :6])
        pipe.run_zeniths(gcols, gzp, profiles=True)
        pp = pipe.zenith_profiles(NCOL, Z)
        assert np.array_equal(pp["angle_up"], prof["angle_up"][:, order])
        assert np.array_equal(pp["angle_down"], prof["angle_down"][:, order])
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_longwave_only_pipeline_zeroes_the_shortwave(bands, lib, device):
    cols = case_columns()
    mu, wt = case_angles()
    go_lw, _, emis, _, _ = _setup((bands[0], None), device, V, fast=0)
    pipe = api.Pipeline(go_lw, None, NCOL, -1, emis, None, None, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    gz, keep_z = api.make_zeniths(mu, wt)
    pipe.run_zeniths(gcols, gz, profiles=True)
    prof = pipe.zenith_profiles(NCOL, Z)
    pipe.run(gcols)
    # (up at the top and the surface, down at the surface; down at the top and, without a user level, its rows are zeros)
    assert np.array_equal(prof["fluxes"], pipe.fluxes(NCOL)) and np.all(prof["fluxes"][:, [0, 1, 4]] > 0.0)
    assert all(np.all(prof[k] == 0.0) for k in ("sw_up", "sw_down", "sw_heating", "angle_fluxes", "angle_up", "angle_down"))
    pipe.destroy()
    go_lw.destroy()


def test_refusals_leave_the_outputs_untouched(bands, lib, device):
    cols = case_columns()
    mu, wt = case_angles()
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V, fast=0)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    sizes = {"levels": NCOL * 4 * V, "heating": NCOL * 2 * L, "fluxes": NCOL * 12, "angles": NCOL * Z * 6,
             "angle_levels": NCOL * Z * 2 * V}
    for spectral in (False, True):
        pipe = api.Pipeline(go_lw, go_sw, NCOL, 0, emis, alb, solar, spectral=spectral)
        bufs = {k: _sentinel(device, n) for k, n in sizes.items()}

        def call(gz, profile, gc=gcols, per_angle=True, outputs=True):
            gz.zenith_fluxes_dev = bufs["angles"].ptr if per_angle else None
            gz.zenith_level_fluxes_dev = bufs["angle_levels"].ptr if (per_angle and profile) else None
            ptrs = [bufs["levels"].ptr if profile else None, bufs["heating"].ptr if profile else None,
                    bufs["fluxes"].ptr if outputs else None]
            return lib.grt_pipeline_run_zeniths(pipe.p, C.byref(gc), C.byref(gz), *ptrs)

        def bad_mu(value):
            m = mu.copy()
            m[1, 2] = value
            return api.make_zeniths(m, wt)

        def bad_weight(value):
            w = wt.copy()
            w[2, 4] = value
            return api.make_zeniths(mu, w)

        refused = []
        for profile in (False, True):
            for zcount in (0, -3, api.GRT_MAX_ZENITHS + 1):
                gz, kz = api.make_zeniths(mu, wt)
                gz.num_zeniths = zcount
                refused.append(("Z", zcount, call(gz, profile)))
            gz, kz = api.make_zeniths(mu, wt)
            gz.cos_zenith = None
            refused.append(("cos_zenith NULL", profile, call(gz, profile)))
            for value in (np.nan, 1.0 + 1e-12, 2.0):
                gz, kz = bad_mu(value)
                refused.append(("mu", value, call(gz, profile)))
            for value in (np.nan, -1e-300, -1.0):
                gz, kz = bad_weight(value)
                refused.append(("weight", value, call(gz, profile)))
            for ncol in (0, NCOL + 1):
                few = api.GrtColumns()
                C.memmove(C.byref(few), C.byref(gcols), C.sizeof(few))
                few.ncol = ncol
                gz, kz = api.make_zeniths(mu, wt)
                refused.append(("ncol", ncol, call(gz, profile, gc=few)))
        gz, kz = api.make_zeniths(mu, wt)
        refused.append(("no output", None, call(gz, False, per_angle=False, outputs=False)))
        gz, kz = api.make_zeniths(mu, wt)
        gz.zenith_fluxes_dev, gz.zenith_level_fluxes_dev = None, bufs["angle_levels"].ptr
        refused.append(("angle levels in the six-row form", None,
                        lib.grt_pipeline_run_zeniths(pipe.p, C.byref(gcols), C.byref(gz), None, None, bufs["fluxes"].ptr)))
        assert all(rc == api.VALUE_ERR for _, _, rc in refused), [r for r in refused if r[2] != api.VALUE_ERR]
        pipe.sync()
        for k, n in sizes.items():
            assert np.all(bufs[k].to_host((n,)) == -7.25), k
        # the angles' own rows alone: neither the longwave nor the mean is formed
        gz, kz = api.make_zeniths(mu, wt)
        assert call(gz, False, outputs=False) == api.SUCCESS
        pipe.sync()
        assert np.all(bufs["fluxes"].to_host((sizes["fluxes"],)) == -7.25)
        got = bufs["angles"].to_host((NCOL, Z, 6))
        assert not np.any(got == -7.25) and np.all(got[mu > 0.0][:, [0, 1, 3, 4]] > 0.0) and np.all(got[mu <= 0.0] == 0.0)
        for b in bufs.values():
            b.free()
        pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
