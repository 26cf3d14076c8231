"""grt_clouds_band_optics / grt_clouds_bands (grtcode_amd/csrc/host/grt_clouds.c): the clouds library's optics per band,
what the batched pipeline's all-sky pass takes, against cloud_optics() itself and against the numpy restatement.  Host
code only: no GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cloud_bands import band_map, band_optics, driver_limits, spread_bands
from cloud_model import LibcRand, cloud_optics, synthetic_tables
from grtcode_amd.dumpfile import write_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "grtcode_amd", "csrc", "host", "grt_clouds.c")
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def clouds(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("clouds_bands") / "libclouds_bands_test.so")
    r = subprocess.run(["gcc", "-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra",
                        "-I" + os.path.join(ROOT, "include"), SRC, "-o", so, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lib = C.CDLL(so)
    lib.cloud_optics.argtypes = [dp, C.c_int, C.c_int, dp, dp, dp, dp, C.c_double, dp] + [dp] * 6
    lib.grt_clouds_band_optics.argtypes = [C.c_int, dp, dp, dp, dp, C.c_double, dp, dp, dp]
    lib.grt_clouds_bands.argtypes = [C.c_int, C.POINTER(C.c_int), dp, dp]
    return lib


def ptr(a):
    return a.ctypes.data_as(dp)


def tables_with(root, seed, liquid_edges, ice_edges, gaps=()):
    """Synthetic parameter files with the liquid and the ice bands of their own; gaps: (phase, band, new upper limit)."""
    for sub in ("l", "i"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    paths, tables = synthetic_tables(root + "/l", seed=seed, band_edges=liquid_edges)
    _, other = synthetic_tables(root + "/i", seed=seed + 1, band_edges=ice_edges)
    tables["ice"] = other["ice"]
    for phase, band, upper in gaps:
        tables[phase]["Band_limits_upr"][band] = np.float64(np.float32(upper))
    for k in ("ice", "liquid"):
        write_dump(paths[k], tables[k])
    return paths, tables


def columns(L, k, rng):
    cf = np.where(rng.random(L) < 0.6, rng.random(L), 0.0)
    cf[1 + k] = 1.0
    cf[2 + k] = 0.0
    lwc = np.where(cf > 0, 0.3 * rng.random(L), 0.0)
    iwc = np.where(cf > 0, 0.05 * rng.random(L), 0.0)
    iwc[5] = 0.0                                                    # liquid-only, and an ice-only layer
    lwc[6] = 0.0
    t = np.linspace(205.0, 290.0, L)
    overlap = np.exp(-np.abs(np.diff(np.linspace(0.0, 12.0, L))) / 2.0)
    return cf, lwc, iwc, t, overlap


CASES = [
    # (liquid band edges, ice band edges, gaps)
    (None, None, ()),
    ([10.0, 200.0, 900.0, 2500.0], [10.0, 150.0, 700.0, 1800.0, 2600.0, 3500.0], ()),       # more ice bands than liquid
    ([10.0, 400.0, 1200.0, 2400.0], [10.0, 300.0, 1000.0, 2400.0],
     (("liquid", 0, 350.0), ("ice", 1, 800.0), ("liquid", 1, 1000.0))),                     # gaps between bands
]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_band_optics_spread_is_cloud_optics(tmp_path, clouds, case):
    liquid_edges, ice_edges, gaps = CASES[case]
    seed = 5 + case
    paths, tables = tables_with(str(tmp_path), seed, liquid_edges if liquid_edges else np.linspace(10.0, 3000.0, 7),
                                ice_edges if ice_edges else np.linspace(10.0, 3000.0, 7), gaps)
    assert clouds.initialize_clouds_lib(paths["beta"].encode(), paths["ice"].encode(), paths["liquid"].encode()) == 0
    try:
        B = tables["liquid"]["Band_limits_lwr"].size
        L, n = 12, 301
        w = driver_limits(1.0, 10.0, n)
        rng = np.random.default_rng(seed)
        rand = LibcRand()
        for col in range(3):                                        # several columns, each a longwave and a shortwave call
            cf, lwc, iwc, t, overlap = columns(L, col, rng)
            args = (ptr(cf), ptr(lwc), ptr(iwc), ptr(overlap), 10.0, ptr(t))
            for call in range(2):
                s = 1000 * case + 10 * col + call
                rand.seed(s)
                want = [np.full((L, n), -5.0) for _ in range(6)]
                assert clouds.cloud_optics(ptr(w), n, L, *args, *[ptr(a) for a in want]) == 0
                after_grid = rand()
                rand.seed(s)
                liq, ice = np.full((3, B, L), np.nan), np.full((3, B, L), np.nan)
                assert clouds.grt_clouds_band_optics(L, *args, ptr(liq), ptr(ice)) == 0
                assert rand() == after_grid                         # the same number of draws
                got = spread_bands(tables, liq, ice, w, out=[np.full((L, n), -5.0) for _ in range(6)])
                for a, b in zip(got, want):
                    assert np.array_equal(a, b)
                rand.seed(s)
                m_liq, m_ice = band_optics(tables, rand, cf, lwc, iwc, overlap, 10.0, t)
                assert np.allclose(liq, m_liq, rtol=1e-13, atol=0.0) and np.allclose(ice, m_ice, rtol=1e-13, atol=0.0)
                rand.seed(s)
                model = cloud_optics(tables, rand, w, cf, lwc, iwc, overlap, 10.0, t, out=[np.full((L, n), -5.0) for _ in range(6)])
                for a, b in zip(got, model):
                    assert np.allclose(a, b, rtol=1e-13, atol=0.0)
                assert np.any(liq[0] > 0.0) and np.any(ice[0] > 0.0)
                assert np.all(liq[0][:, 6] == 0.0)                  # the ice-only layer
        if gaps:
            # points that no band covers keep the caller's values in cloud_optics: the maps say -1 there
            lo, hi = tables["liquid"]["Band_limits_lwr"], tables["liquid"]["Band_limits_upr"]
            m = band_map(lo, hi, B, B, w)
            assert np.any(m < 0)
            assert np.all(got[0][:, m < 0] == -5.0)
    finally:
        assert clouds.finalize_clouds_lib() == 0


def test_bands_returns_the_rounded_limits(tmp_path, clouds):
    edges = [10.1, 200.3, 900.7, 2500.9]
    paths, tables = tables_with(str(tmp_path), 3, edges, [10.1, 150.2, 700.3, 1800.4, 2600.6])
    assert clouds.initialize_clouds_lib(paths["beta"].encode(), paths["ice"].encode(), paths["liquid"].encode()) == 0
    try:
        for ice, want in ((0, edges), (1, [10.1, 150.2, 700.3, 1800.4, 2600.6])):
            nb = C.c_int()
            assert clouds.grt_clouds_bands(ice, C.byref(nb), None, None) == 0
            assert nb.value == len(want) - 1
            lo, hi = np.zeros(nb.value), np.zeros(nb.value)
            assert clouds.grt_clouds_bands(ice, C.byref(nb), ptr(lo), ptr(hi)) == 0
            f32 = np.asarray(want, dtype=np.float32).astype(np.float64)
            assert np.array_equal(lo, f32[:-1]) and np.array_equal(hi, f32[1:])
            assert not np.array_equal(lo, np.asarray(want[:-1]))     # rounded: not the decimal values
    finally:
        assert clouds.finalize_clouds_lib() == 0
