"""grt_pipeline_run_sky_zeniths in the production arithmetic (fast = 3): the case and the margins of the sky sets'
production test (test_gpu_pipeline_sky.py) -- four columns of 16 levels, two cloud draws, the aerosol on
AEROSOL_GRID, all four sets; fluxes and level fluxes within 1e-3 W m-2 of the oracle, heating rates within the bound that
follows from it -- under Z = 3 sun angles per column, one of them a night sample: every day angle's rows of every set,
and the mean."""
import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID, aerosol_fields
from grtcode_amd import api, synthetic as syn
from pipeline_support import CP, GRAVITY, _setup, heating, make, subcolumn_clouds
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from sky_zenith_support import ALL, NAMES, aerosols_of, oracle_set, positive_zero, run_sky_zeniths, six

pytestmark = pytest.mark.gpu

FLUX_TOL = 1e-3       # W m-2
V1, UL1, S, Z = 16, 5, 2, 3
CLOUD_SEED, AEROSOL_SEED = 81, 83


def test_production_form_matches_the_oracle_per_angle_and_in_the_mean(bands, tables, oracle, lib, device):
    cols = []
    for c, fp in enumerate((1.0, 0.9, 1.03, 0.8)):
        col = syn.profile(320 + c, V1)
        col["p"] = col["p"] * fp
        cols.append(col)
    ncol, L = len(cols), V1 - 1
    mu = np.array([[0.6, 1.0, -0.2], [0.0, 0.3, 0.05], [1.0, -1.0, 0.6], [0.05, 0.3, 0.0]])
    assert mu.shape == (ncol, Z) and np.all(np.sum(mu <= 0.0, axis=1) == 1)
    wt = np.array([[0.5, 0.25, 0.25]] * ncol)
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1, fast=3)
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, CLOUD_SEED + 1, S)
    gclouds, keep_clouds = make(tables, cl)
    grids = (AEROSOL_GRID, AEROSOL_GRID)
    f = (aerosol_fields(ncol, L, AEROSOL_GRID, AEROSOL_SEED + 2, lw=True),
         aerosol_fields(ncol, L, AEROSOL_GRID, AEROSOL_SEED + 3, lw=False))
    gaer, keep_aer = aerosols_of(f, grids)
    prof = run_sky_zeniths(pipe, gcols, gclouds, gaer, S, ALL, mu, wt, ncol, True)
    six_rows = run_sky_zeniths(pipe, gcols, gclouds, gaer, S, ALL, mu, wt, ncol, False)
    assert go_lw.last_launch()["fast"] == 3 and go_sw.last_launch()["fast"] == 3
    swb = bands[1]
    worst = {"angle_flux": 0.0, "angle_level": 0.0, "mean_flux": 0.0, "mean_level": 0.0, "heating_of_bound": 0.0}
    for c, col in enumerate(cols):
        mass = 100.0 * (col["p"][1:] - col["p"][:-1]) / GRAVITY
        bound = 4.0 * FLUX_TOL / (CP * mass) * 86400.0
        for at, name in enumerate(NAMES):
            mean_up, mean_dn = np.zeros(V1), np.zeros(V1)
            for k in range(Z):
                if not mu[c, k] > 0.0:
                    for out in (six_rows["angle_fluxes"], prof["angle_fluxes"], prof["angle_up"], prof["angle_down"]):
                        assert positive_zero(out[c, at, k]), (c, name, k)
                    continue
                w = oracle_set(name, oracle, lib, swb, dict(col, mu0=mu[c, k]), tables, cl["sw_liquid"][c], cl["sw_ice"][c],
                               cl["thickness"][c], AEROSOL_GRID, f[1][c], emis, alb, solar)
                want = six(w["up_int"], w["dn_int"], UL1)
                worst["angle_flux"] = max(worst["angle_flux"], np.max(np.abs(six_rows["angle_fluxes"][c, at, k] - want)),
                                          np.max(np.abs(prof["angle_fluxes"][c, at, k] - want)))
                worst["angle_level"] = max(worst["angle_level"], np.max(np.abs(prof["angle_up"][c, at, k] - w["up_int"])),
                                           np.max(np.abs(prof["angle_down"][c, at, k] - w["dn_int"])))
                mean_up += wt[c, k] * w["up_int"]
                mean_dn += wt[c, k] * w["dn_int"]
            # (the weights add up to 1: the mean of values within FLUX_TOL is within FLUX_TOL)
            want = six(mean_up, mean_dn, UL1)
            worst["mean_flux"] = max(worst["mean_flux"], np.max(np.abs(six_rows["fluxes"][c, at, 6:] - want)),
                                     np.max(np.abs(prof["fluxes"][c, at, 6:] - want)))
            worst["mean_level"] = max(worst["mean_level"], np.max(np.abs(prof["sw_up"][c, at] - mean_up)),
                                      np.max(np.abs(prof["sw_down"][c, at] - mean_dn)))
            d = np.abs(prof["sw_heating"][c, at] - heating(mean_up, mean_dn, col["p"]))
            worst["heating_of_bound"] = max(worst["heating_of_bound"], np.max(d / bound))
    print("production form under three angles, worst:", worst)
    assert max(worst["angle_flux"], worst["angle_level"], worst["mean_flux"], worst["mean_level"]) <= FLUX_TOL, worst
    assert worst["heating_of_bound"] <= 1.0, worst
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
