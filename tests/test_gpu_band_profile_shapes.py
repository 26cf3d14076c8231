"""grt_pipeline_run_band_profiles at the shapes where a block-wise sum goes wrong: grids of one and two lanes, one block,
an exact multiple of the 128-point solver block and one live lane past it, bins that start and end on a block boundary
and one point either side, one-interval bins at both ends, two levels and 61, columns of one launch whose direct beam is
clamped and whose is not -- both forms, clear sky and all-sky, every bin against the oracle within LEVEL_TOL of the
column's largest flux."""
import numpy as np
import pytest

from grtcode_amd import api
from pipeline_support import (LEVEL_TOL, SOLVER_NS, block_edges, clouds_for, columns, exact_trapezoid, make,
                              oracle_allsky_levels, oracle_column, surface)
from pipeline_support import solver_bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

BANDS = (("lw", True), ("sw", False))


@pytest.mark.parametrize("V", [2, 61])
@pytest.mark.parametrize("n", SOLVER_NS)
def test_band_profiles_at_edge_shapes(solver_bands, tables, oracle, lib, device, n, V):
    pair = solver_bands[n]
    cols = columns(V)
    ncol = len(cols)
    go_lw, _ = pair[0].gas_optics(device, V)
    go_sw, grid_sw = pair[1].gas_optics(device, V)
    emis, _ = surface(n, 1 + n)
    _, alb = surface(n, 2 + n)
    solar = api.create_solar_flux(grid_sw, pair[1].files["solar"])
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    cl = clouds_for(cols, tables, 30 + V)
    gclouds, keep_clouds = make(tables, cl)
    edges = block_edges(n)
    assert edges.size >= 2
    want = {}
    for bi, (key, lw) in enumerate(BANDS):
        for c, col in enumerate(cols):
            want[bi, c, 0] = oracle_column(oracle, lib, pair[bi], col, lw, emis, alb, solar)
            want[bi, c, 1] = oracle_allsky_levels(oracle, lib, pair[bi], col, lw, tables, cl[key + "_liquid"][c],
                                                  cl[key + "_ice"][c], cl["thickness"][c], emis, alb, solar)
    for spectral in (False, True):
        pipe = api.Pipeline(go_lw, go_sw, ncol, -1, emis, alb, solar, spectral=spectral)
        assert edges.size - 1 <= pipe.band_profile_bin_limit()
        pipe.run_band_profiles(gcols, gclouds, edges, edges)
        got = pipe.band_profiles(ncol)
        for bi, (key, lw) in enumerate(BANDS):
            dw = pair[bi].dw
            assert got[key + "_up"].shape == (ncol, 2, edges.size - 1, V)
            for c in range(ncol):
                for s in range(2):
                    w = want[bi, c, s]
                    # the column's largest (integrated) flux, as test_gpu_solver_shapes.py scales LEVEL_TOL
                    scale = max(abs(exact_trapezoid(r, dw)[0]) for rows in (w["up"], w["dn"]) for r in rows)
                    assert scale > 0.0
                    for name, rows in ((key + "_up", w["up"]), (key + "_down", w["dn"])):
                        for b in range(edges.size - 1):
                            ref = np.array([exact_trapezoid(r[edges[b]:edges[b + 1] + 1], dw)[0] for r in rows])
                            err = np.max(np.abs(got[name][c, s, b] - ref))
                            assert err <= LEVEL_TOL * scale, (name, spectral, c, s, b, err, scale)
        pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
