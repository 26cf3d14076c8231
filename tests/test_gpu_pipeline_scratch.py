"""The device buffers a pipeline allocates on demand (GrtScratch: the park block, the level, bin and subcolumn partial sums,
the flux sums, the spread block, the surface rows) and its keyed tables, across calls on one live object: a sequence of
calls that makes each of them first appear and then be replaced by a larger one, and the same calls in reverse, when
every buffer is already large enough and is reused.  After each call the outputs are, bit for bit, those of a fresh
pipeline that made that call alone: what earlier calls left on the object does not reach a result.  Deterministic mode,
both pipeline forms, the smallest shape at which every buffer exists: three solver blocks per band, V = 3, two columns."""
import numpy as np
import pytest

from aerosol_model import aerosol_fields
from grtcode_amd import api
from pipeline_support import SETS, _deterministic, columns, limits, make_shape_bands
from pipeline_support import tables  # noqa: F401  (module fixture)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

V, N, NCOL = 3, 257, 2
L = V - 1
bands = make_shape_bands((N,), 1.0, 1000.0)


def drawn_clouds(S, seed, B=6):
    """Band tables [NCOL][S][3][B][L]: every other (subcolumn, layer) cloudy, the rest clear."""
    rng = np.random.default_rng(seed)
    cloudy = ((np.arange(S)[:, None] + np.arange(L)[None, :]) % 2 == 0)[None, :, None, :]
    out = {}
    for k in SETS:
        ext = np.where(cloudy, 10.0 ** rng.uniform(-5.0, -2.0, (NCOL, S, B, L)), 0.0)
        alb = np.where(cloudy, rng.uniform(0.0, 0.9999, (NCOL, S, B, L)), 0.0)
        asy = np.where(cloudy, rng.uniform(0.0, 0.95, (NCOL, S, B, L)), 0.0)
        out[k] = np.ascontiguousarray(np.stack([ext, alb, asy], axis=2))
    return out


def flat(*sets):
    """(clear, second set) dicts or arrays as one dict of arrays"""
    out = {}
    for s, x in enumerate(sets):
        for key, a in (x.items() if isinstance(x, dict) else [("fluxes", x)]):
            out[f"{s}.{key}"] = a
    return out


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "mat"])
def test_history_on_the_object_does_not_reach_a_result(bands, tables, lib, device, monkeypatch, spectral):
    lwb, swb = bands[N]
    go_lw, _ = lwb.gas_optics(device, V)
    go_sw, grid_sw = swb.gas_optics(device, V)
    solar = api.create_solar_flux(grid_sw, swb.files["solar"])
    emis, alb = np.full(N, 0.98), np.full(N, 0.2)
    cols = columns(V)[:NCOL]
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    thickness = np.array([29.3 * c["t_layer"] * np.log(c["p"][1:] / c["p"][:-1]) for c in cols])
    lims = limits(tables, "liquid"), limits(tables, "ice")
    cl = drawn_clouds(3, 17)
    clouds = {S: api.make_clouds(*lims, thickness, *[np.ascontiguousarray(cl[k][:, :S]) for k in SETS]) for S in (1, 3)}
    one = api.make_clouds(*lims, thickness, *[np.ascontiguousarray(cl[k][:, 0]) for k in SETS])
    lw_x, sw_x = np.array([20.0, 90.0, 200.0, 300.0]), np.array([1200.0, 2000.0, 3000.0])
    aer = api.make_aerosols(lw=(lw_x, aerosol_fields(NCOL, L, lw_x, 3, True)),
                            sw=(sw_x, aerosol_fields(NCOL, L, sw_x, 4, False)))
    rng = np.random.default_rng(23)
    e_x, a_x = np.array([50.0, 120.0, 240.0]), np.array([1100.0, 1900.0, 2500.0, 3400.0])
    surf_emis = api.make_surface(NCOL, emissivity=(e_x, rng.uniform(0.5, 1.0, (NCOL, 3))))
    surf_all = api.make_surface(NCOL, emissivity=(e_x, rng.uniform(0.5, 1.0, (NCOL, 3))),
                                albedo=(a_x, rng.uniform(0.0, 0.6, (NCOL, 4)), rng.uniform(0.0, 0.6, (NCOL, 4))))
    few = dict(lw_edges=[0, 100, N - 1], sw_edges=[0, N - 1])
    more = dict(lw_edges=[0, 1, 127, 128, 129, 200, N - 1], sw_edges=[3, 64, 128, 192, 250])

    def subcolumns(S, profile, two_sweeps=False):
        def step(pipe):
            if two_sweeps:
                monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
            try:
                pipe.run_subcolumns(gcols, clouds[S][0], S, profiles=profile)
            finally:
                monkeypatch.delenv("GRT_SW_TWO_SWEEPS", raising=False)
            return flat(*(pipe.subcolumn_profiles(NCOL) if profile else pipe.subcolumn_fluxes(NCOL)))
        return step

    def aerosols(pipe):
        pipe.run_aerosols(gcols, aer[0])
        return flat(*pipe.aerosol_fluxes(NCOL))

    def allsky(pipe):
        pipe.run_allsky(gcols, one[0])
        return flat(*pipe.allsky_fluxes(NCOL))

    def spectral_bins(pipe):
        pipe.run_spectral(gcols, None, **few)
        return pipe.spectral(NCOL)

    def band_profiles(pipe):
        pipe.run_band_profiles(gcols, one[0], **more)
        return pipe.band_profiles(NCOL)

    def surface(gsurface):
        def step(pipe):
            pipe.set_surface(gsurface[0])
            pipe.run(gcols)
            out = {"fluxes": pipe.fluxes(NCOL)}
            pipe.set_surface(None)
            return out
        return step

    steps = [("S1-six", subcolumns(1, False)), ("S3-six-two-sweeps", subcolumns(3, False, two_sweeps=True)),
             ("S1-profile", subcolumns(1, True)), ("S3-profile", subcolumns(3, True)),
             ("aerosols", aerosols), ("allsky", allsky), ("spectral-bins", spectral_bins), ("band-profiles", band_profiles),
             ("surface-emissivity", surface(surf_emis)), ("surface-all", surface(surf_all))]

    def create():
        return api.Pipeline(go_lw, go_sw, NCOL, -1, emis, alb, solar, spectral=spectral)

    pipe = create()
    _deterministic(lib, True)
    try:
        want = {}
        for name, step in steps:                       # every buffer appears, then is replaced by a larger one
            fresh = create()
            want[name] = step(fresh)
            fresh.destroy()
            got = step(pipe)
            assert got.keys() == want[name].keys() and len(got) > 0
            for key in got:
                assert np.all(np.isfinite(got[key])), (name, key)
                assert np.array_equal(got[key], want[name][key]), ("growing", name, key)
        for name, step in reversed(steps):             # every buffer is large enough already and is reused
            got = step(pipe)
            for key in got:
                assert np.array_equal(got[key], want[name][key]), ("shrinking", name, key)
        # (the subcolumn calls above left the materialised form's spread block at its six arrays before the aerosol pass
        # ran; on an object that has seen no clouds it appears with three and the all-sky pass replaces it)
        pipe.destroy()
        pipe = create()
        for name in ("aerosols", "allsky", "aerosols"):
            got = dict(steps)[name](pipe)
            for key in got:
                assert np.array_equal(got[key], want[name][key]), ("spread block", name, key)
        # the steps are not one another's: a wrong placement that gave every call the same rows would pass the above
        assert not np.array_equal(want["S1-six"]["1.fluxes"], want["S3-six-two-sweeps"]["1.fluxes"])
        assert not np.array_equal(want["aerosols"]["1.fluxes"], want["allsky"]["1.fluxes"])
        assert not np.array_equal(want["surface-emissivity"]["fluxes"], want["surface-all"]["fluxes"])
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
