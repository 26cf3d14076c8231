"""grt_pipeline_run_sky_zeniths_direct in the production arithmetic (fast = 3): test_gpu_sky_zeniths_production.py's case
and margin -- four columns of 16 levels, two cloud draws, the aerosol on AEROSOL_GRID, all four sets, within 1e-3 W m-2 of
the oracle -- under Z = GRT_ZENITH_CHUNK + 1 angles per column, one of them a night sample, with a direct albedo per
(column, angle) and every angle's direct beam: every day angle's rows of every set, the direct ones included."""
import numpy as np
import pytest

from aerosol_model import AEROSOL_GRID, aerosol_fields
from direct_beam_model import three
from grtcode_amd import api, surfaces, synthetic as syn
from pipeline_support import _setup, make, subcolumn_clouds
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER
from sky_zenith_support import ALL, NAMES, aerosols_of, positive_zero
from surface_support import host_rows
from test_gpu_sky_zeniths_direct import oracle_set_direct

pytestmark = pytest.mark.gpu

FLUX_TOL = 1e-3       # W m-2
V1, UL1, S = 16, 5, 2
Z = api.GRT_ZENITH_CHUNK + 1
CLOUD_SEED, AEROSOL_SEED = 81, 83


def test_production_form_matches_the_oracle_per_angle(bands, tables, oracle, lib, device):
    cols = []
    for c, fp in enumerate((1.0, 0.9, 1.03, 0.8)):
        col = syn.profile(320 + c, V1)
        col["p"] = col["p"] * fp
        cols.append(col)
    ncol, L = len(cols), V1 - 1
    pool = (0.6, 1.0, 0.3, 0.05, 0.85, 0.15)
    mu = np.array([[pool[(k + c) % len(pool)] for k in range(Z)] for c in range(ncol)])
    for c in range(ncol):
        mu[c, (2 * c + 1) % Z] = (-0.2, 0.0)[c % 2]
    assert np.all(np.sum(mu <= 0.0, axis=1) == 1)
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V1, fast=3)
    swb = bands[1]
    pipe = api.Pipeline(go_lw, go_sw, ncol, UL1, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = subcolumn_clouds(cols, tables, CLOUD_SEED + 1, S)
    gclouds, keep_clouds = make(tables, cl)
    f = (aerosol_fields(ncol, L, AEROSOL_GRID, AEROSOL_SEED + 2, lw=True),
         aerosol_fields(ncol, L, AEROSOL_GRID, AEROSOL_SEED + 3, lw=False))
    gaer, keep_aer = aerosols_of(f, (AEROSOL_GRID, AEROSOL_GRID))
    # open water under every angle, a little darker in the near infrared: three knots inside the band
    xa = np.array([swb.w0 + 0.2 * (swb.wn - swb.w0), swb.w0 + 0.5 * (swb.wn - swb.w0), swb.w0 + 0.8 * (swb.wn - swb.w0)])
    knots = surfaces.ocean_direct_albedo(mu)[:, :, None] * np.array([0.8, 1.0, 1.1])[None, None, :]
    gsurf, keep_surf = api.make_zenith_surface(xa, knots)
    gsky, keep_sky = api.make_sky(gclouds, gaer, S, ALL)
    got = {}
    for p in (False, True):
        gz, keep_z = api.make_zeniths(mu)
        pipe.run_sky_zeniths_direct(gcols, gsky, gz, gsurface=gsurf, direct=True, profiles=p)
        got[p] = pipe.sky_zenith_direct_profiles(ncol, 4, Z) if p else pipe.sky_zenith_direct_fluxes(ncol, 4, Z)
    assert go_lw.last_launch()["fast"] == 3 and go_sw.last_launch()["fast"] == 3
    grid = api.create_spectral_grid(swb.w0, swb.wn, swb.dw)
    worst = {"angle_flux": 0.0, "angle_level": 0.0, "angle_direct": 0.0, "angle_direct_level": 0.0}
    # (the oracle is the expensive part: the first and the last column of the batch, every set and angle of each)
    for c, col in ((0, cols[0]), (ncol - 1, cols[ncol - 1])):
        for at, name in enumerate(NAMES):
            for k in range(Z):
                if not mu[c, k] > 0.0:
                    for out in got.values():
                        for key in [q for q in out if q.startswith("angle_")]:
                            assert positive_zero(out[key][c, at, k]), (c, name, k, key)
                    continue
                alb_dir = host_rows(lib, grid, xa, knots[c, k:k + 1])[0]
                w = oracle_set_direct(name, oracle, lib, swb, dict(col, mu0=mu[c, k]), tables, cl["sw_liquid"][c],
                                      cl["sw_ice"][c], cl["thickness"][c], AEROSOL_GRID, f[1][c], alb_dir, alb, solar)
                want6 = np.concatenate([three(w["up_int"], UL1), three(w["dn_int"], UL1)])
                want3 = three(w["direct"], UL1)
                for out in got.values():
                    worst["angle_flux"] = max(worst["angle_flux"], np.max(np.abs(out["angle_fluxes"][c, at, k] - want6)))
                    worst["angle_direct"] = max(worst["angle_direct"], np.max(np.abs(out["angle_direct"][c, at, k] - want3)))
                prof = got[True]
                worst["angle_level"] = max(worst["angle_level"], np.max(np.abs(prof["angle_up"][c, at, k] - w["up_int"])),
                                           np.max(np.abs(prof["angle_down"][c, at, k] - w["dn_int"])))
                worst["angle_direct_level"] = max(worst["angle_direct_level"],
                                                  np.max(np.abs(prof["angle_direct_levels"][c, at, k] - w["direct"])))
    print("production form, a direct albedo per angle and the direct beam, worst:", worst)
    assert max(worst.values()) <= FLUX_TOL, worst
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
