"""grt_pipeline_run_band_profiles in the PRODUCTION arithmetic (fast = 3), next to test_gpu_pipeline_production.py and
with its inputs, oracle results and bounds: every bin of every level within FLUX_TOL (1e-3 W m-2) of the oracle's level
spectra integrated over the bin -- a bin is a partial sum of the broadband value that bound is set for --, every bin's
heating rates within the bound derived from it, 4 FLUX_TOL g/(c_p 100 dp) 86400 K day-1, and within FORMULA_TOL of the
formula on the call's own levels; fused and materialised form, clear-sky and all-sky set."""
import numpy as np
import pytest

from pipeline_support import CP, GRAVITY, block_edges, exact_trapezoid, heating, make
from pipeline_support import bands, oracle_cache, tables  # noqa: F401  (module fixtures)
from test_gpu_pipeline_production import BANDS, FLUX_TOL, FORMULA_TOL, V1, assert_production, check_tau_gas, note
from test_gpu_pipeline_production import p1  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spectral", [False, True], ids=["fused", "materialised"])
def test_run_band_profiles_matches_the_oracle(p1, tables, lib, device, spectral):
    entry = "run_band_profiles"
    pipe = p1.open(spectral)
    gclouds, keep_clouds = make(tables, p1.cl)
    edges = [block_edges(b.nw) for b in p1.bands]
    pipe.run_band_profiles(p1.gcols, gclouds, *edges)
    got = pipe.band_profiles(p1.ncol)
    assert_production(p1.go_lw, p1.go_sw)
    check_tau_gas(lib, entry, device, pipe, p1.bands, p1.ncol, V1 - 1, lambda bi, c: p1.clear(bi, c)["tau_gas"])
    for bi, (key, lw) in enumerate(BANDS):
        band, e = p1.bands[bi], edges[bi]
        assert got[key + "_up"].shape == (p1.ncol, 2, e.size - 1, V1)
        for c, col in enumerate(p1.cols):
            p = col["p"]
            bound = 4.0 * FLUX_TOL * GRAVITY / (CP * 100.0 * (p[1:] - p[:-1])) * 86400.0
            for s in range(2):
                w = p1.allsky(bi, c) if s == 1 else p1.clear(bi, c)
                for b in range(e.size - 1):
                    what = f"{key} column {c} set {s} bin {b}"
                    want = {d: np.array([exact_trapezoid(r[e[b]:e[b + 1] + 1], band.dw)[0] for r in w[d]])
                            for d in ("up", "dn")}
                    up, dn, hr = (got[key + x][c, s, b] for x in ("_up", "_down", "_heating"))
                    for name, a, ref in (("up", up, want["up"]), ("down", dn, want["dn"])):
                        err = note(lib, entry, "bin_level_flux_w_m2", np.max(np.abs(a - ref)), FLUX_TOL)
                        assert err <= FLUX_TOL, f"{what} {name}: {err} W m-2 from the oracle at level {np.argmax(np.abs(a - ref))}"
                    d = np.abs(hr - heating(want["up"], want["dn"], p))
                    note(lib, entry, "heating_of_its_bound", np.max(d / bound), 1.0)
                    j = int(np.argmax(d / bound))
                    assert np.all(d <= bound), f"{what}: heating {d[j]} K day-1 from the oracle in layer {j}, bound {bound[j]}"
                    hmax = np.abs(hr).max()
                    assert hmax > 0.0, what
                    err = np.max(np.abs(hr - heating(up, dn, p)))
                    assert err <= FORMULA_TOL * hmax, f"{what}: heating {err} from the formula on its own levels, largest {hmax}"
    p1.close()
