"""grt_cloud_sampler_run: the band optics of cloud subcolumns sampled on the device, held bit for bit to the numpy
restatement (cloud_bands.band_optics) fed the same draws in the same order, to the host library (grt_clouds_band_optics)
after the same srand, and -- generator mode -- to the numpy Philox4x32-10; the generator's independence of batch, offset
and subcolumn count, its statistics, and the refusals.  The sampler alone: no gas optics.

Bit equality is the requirement: both sides do IEEE double + - x / with no contraction."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from cloud_model import LibcRand
from cloud_sampler_support import (edge_fields, expected_tables, libc_uniforms, philox_uniforms, plant_edges)
from grtcode_amd import api
from grtcode_amd.dumpfile import write_dump
from pipeline_support import _sentinel
from pipeline_support import tables  # noqa: F401  (module fixture: more ice bands than liquid ones, a gap between bands)

pytestmark = pytest.mark.gpu

NCOL = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def sampler(tables, device):
    gm, keep = api.make_cloud_model(tables)
    sp = api.CloudSampler(device, gm)
    yield sp
    sp.destroy()


def fields_of(f, S, **kw):
    return api.make_cloud_fields(f["cf"], f["lwc"], f["iwc"], f["ov"], temperature=f["t"], num_subcolumns=S, **kw)


@pytest.fixture(scope="module")
def uniform_cases(tables):
    """Per layer count: the fields, three subcolumns of draws with the edge values planted, and the expected tables --
    made once, shared by the S = 1 and S = 3 cases (S = 1 is the first subcolumn's draws)."""
    cache = {}
    B = tables["liquid"]["Band_limits_lwr"].size

    def get(L):
        if L not in cache:
            f = edge_fields(NCOL, L, 100 + L)
            u = plant_edges(np.random.default_rng(200 + L).random((NCOL, 2, 3, B, 2 * L - 1)), f)
            cache[L] = (f, u, expected_tables(tables, f, u))
        return cache[L]
    return get


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 130])
def test_uniforms_mode_is_band_optics_bit_for_bit(tables, sampler, uniform_cases, L, S):
    f, u, want = uniform_cases(L)
    gf, keep = fields_of(f, S, uniforms=u[:, :, :S])
    got = sampler.run(gf)
    assert got.shape == (4, S, NCOL, 3, want.shape[4], L)
    assert np.array_equal(got, want[:, :S])
    if L >= 63:
        # the cases the fields and the planted draws are there for
        kinds = (np.arange(L)[None, :] + np.arange(NCOL)[:, None]) % 6              # edge_fields' layer kinds
        at = lambda a, kind: a[np.broadcast_to((kinds == kind)[:, None, None, :], a.shape)]   # a [ncol][3][B][L]
        for k in range(4):
            assert np.all(at(got[k, 0][:, :1], 1) > 0.0)            # overcast with water: every band's draw is cloudy
            assert np.all(at(got[k, 0], 3) == 0.0)                  # clear
            assert np.all(at(got[k, 0], 5) == 0.0)                  # cloudy with no water at all
            assert np.all(at(got[k, 0], 2 if k % 2 else 4) == 0.0)  # no ice in liquid-only layers, no liquid in ice-only ones
            assert np.any(at(got[k, 0], 4 if k % 2 else 2) > 0.0)
        assert u[0, 0, 0, 0, 2] == 1.0 - f["cf"][0, 2] and got[0, 0, 0, 1, 0, 2] == 0.0       # rank == 1 - cf: not cloudy
        assert got[0, 0, 0, 1, 1, 0] > 0.0 and got[0, 0, 0, 1, 2, 0] > 0.0                    # ranks 1.25 and 1.0: cloudy


def test_a_radius_outside_every_size_regime_gives_no_liquid(tables, sampler, uniform_cases):
    f, u, _ = uniform_cases(2)
    assert tables["liquid"]["Effective_Radius_limits_upr"].max() < 40.0
    want = expected_tables(tables, f, u[:, :, :1], liquid_radius=40.0)
    gf, keep = fields_of(f, 1, uniforms=u[:, :, :1], liquid_radius=40.0)
    got = sampler.run(gf)
    assert np.array_equal(got, want)
    assert np.all(got[0] == 0.0) and np.all(got[2] == 0.0) and np.any(got[1] > 0.0)


@pytest.fixture(scope="module")
def clouds_library(tables, tmp_path_factory):
    """grt_clouds.c, compiled as tests/test_clouds_band_optics.py compiles it, loaded with the module's tables."""
    root = tmp_path_factory.mktemp("clouds_sampler_library")
    so = str(root / "libclouds_sampler_test.so")
    src = os.path.join(ROOT, "grtcode_amd", "csrc", "host", "grt_clouds.c")
    r = subprocess.run(["gcc", "-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wextra",
                        "-I" + os.path.join(ROOT, "include"), src, "-o", so, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    lib = C.CDLL(so)
    lib.grt_clouds_band_optics.argtypes = [C.c_int, dp, dp, dp, dp, C.c_double, dp, dp, dp]
    paths = {}
    for k in ("beta", "ice", "liquid"):
        paths[k] = str(root / f"{k}.dump")
        write_dump(paths[k], tables[k])
    assert lib.initialize_clouds_lib(paths["beta"].encode(), paths["ice"].encode(), paths["liquid"].encode()) == 0
    yield lib
    assert lib.finalize_clouds_lib() == 0


def test_the_host_library_after_the_same_srand(tables, sampler, clouds_library):
    L, S, n = 5, 2, 4321
    B = tables["liquid"]["Band_limits_lwr"].size
    f = edge_fields(NCOL, L, 7)
    rand = LibcRand()
    rand.seed(n)
    u = libc_uniforms(rand, NCOL, S, B, L)
    gf, keep = fields_of(f, S, uniforms=u)
    got = sampler.run(gf)
    rand.seed(n)
    ptr = lambda a: np.ascontiguousarray(a).ctypes.data_as(dp)
    for c in range(NCOL):                                           # the driver's order: column, pass, subcolumn
        for p in range(2):
            for s in range(S):
                liq, ice = np.full((3, B, L), np.nan), np.full((3, B, L), np.nan)
                assert clouds_library.grt_clouds_band_optics(L, ptr(f["cf"][c]), ptr(f["lwc"][c]), ptr(f["iwc"][c]),
                                                             ptr(f["ov"][c]), 10.0, ptr(f["t"][c]), ptr(liq), ptr(ice)) == 0
                assert np.array_equal(got[2 * p, s, c], liq), (c, p, s)
                assert np.array_equal(got[2 * p + 1, s, c], ice), (c, p, s)
    assert np.any(got[0] > 0.0) and np.any(got[1] > 0.0)


@pytest.mark.parametrize("L", [2, 65])
def test_generator_mode_is_the_numpy_philox(tables, sampler, L):
    S, seed, offset = 2, (0x9abcdef0 << 32) | 0x12345678, 1000
    B = tables["liquid"]["Band_limits_lwr"].size
    f = edge_fields(NCOL, L, 300 + L)
    gf, keep = fields_of(f, S, seed=seed, column_offset=offset)
    got = sampler.run(gf)
    want = expected_tables(tables, f, philox_uniforms(seed, offset, NCOL, S, B, L))
    assert np.array_equal(got, want)
    assert np.any(got[0] > 0.0) and not np.array_equal(got[0], got[2])          # the passes draw apart


def test_generator_depends_on_seed_and_global_column_alone(tables, sampler):
    L = 65
    f = edge_fields(4, L, 41)
    part = lambda cols: {k: v[cols] for k, v in f.items()}
    whole = sampler.run(fields_of(f, 2, seed=77)[0])
    first = sampler.run(fields_of(part(slice(0, 2)), 2, seed=77)[0])
    second = sampler.run(fields_of(part(slice(2, 4)), 2, seed=77, column_offset=2)[0])
    assert np.array_equal(whole[:, :, :2], first) and np.array_equal(whole[:, :, 2:], second)
    five = sampler.run(fields_of(f, 5, seed=77)[0])
    assert np.array_equal(five[:, :2], whole)                                   # subcolumn s of S = 2 and of S = 5
    assert not np.array_equal(five[:, 2], five[:, 3])
    other = sampler.run(fields_of(f, 2, seed=78)[0])
    assert not np.array_equal(other, whole)


def test_generator_statistics(tables, sampler):
    L, S = 64, 64
    B = tables["liquid"]["Band_limits_lwr"].size
    f = dict(cf=np.full((1, L), 0.3), lwc=np.full((1, L), 0.1), iwc=np.full((1, L), 0.01), t=np.full((1, L), 250.0),
             ov=np.zeros((1, L - 1)))
    got = sampler.run(fields_of(f, S, seed=2024)[0])
    cloudy = got[0, :, 0, 1] > 0.0                                  # [S][B][L]: the liquid's albedo is set where cloudy
    n = S * B * L
    bound = 5.0 * np.sqrt(0.3 * 0.7 / n)                            # 5 sigma of a binomial share; 0.015 at B = 6
    share = cloudy.mean()
    print(f"cloudy share {share:.5f} of {n} cells, bound 0.3 +- {bound:.5f}")
    assert cloudy.size == n and abs(share - 0.3) <= bound
    # overlap 1, one cloud fraction: every layer takes the first layer's rank -- a sample is cloudy everywhere or nowhere
    f["ov"][:] = 1.0
    got = sampler.run(fields_of(f, S, seed=2024)[0])
    for k in (0, 2):
        per_sample = (got[k, :, 0, 1] > 0.0).sum(axis=-1)           # [S][B]
        assert np.all((per_sample == 0) | (per_sample == L))
        assert np.any(per_sample == 0) and np.any(per_sample == L)


def test_refusals_leave_the_output_untouched(tables, sampler, lib, device):
    L, S = 4, 2
    B = tables["liquid"]["Band_limits_lwr"].size
    f = edge_fields(NCOL, L, 9)
    n = 4 * S * NCOL * 3 * B * L
    out = _sentinel(device, n)

    def refused(gf, sp=sampler.p, ptr=out.ptr):
        with pytest.raises(api.GrtError) as e:
            api.check(lib.grt_cloud_sampler_run(sp, C.byref(gf) if gf is not None else None, ptr))
        assert e.value.code == api.VALUE_ERR

    good, keep = fields_of(f, S)
    refused(good, sp=None)
    refused(None)
    refused(good, ptr=None)
    for field in ("cloud_fraction", "liquid_content", "ice_content", "temperature", "overlap"):
        gf, k = fields_of(f, S)
        setattr(gf, field, None)
        refused(gf)
    for bad_s in (0, -1, api.GRT_MAX_SUBCOLUMNS + 1):
        gf, k = fields_of(f, S)
        gf.num_subcolumns = bad_s
        refused(gf)
    for attr in ("ncol", "num_layers"):
        gf, k = fields_of(f, S)
        setattr(gf, attr, 0)
        refused(gf)
    for key, value in (("cf", -0.01), ("cf", 1.0 + 1e-12), ("cf", np.nan), ("cf", np.inf), ("lwc", -1e-9), ("lwc", np.inf),
                       ("lwc", np.nan), ("iwc", -1e-9), ("iwc", np.inf), ("iwc", np.nan)):
        g = {k: v.copy() for k, v in f.items()}
        g[key][NCOL - 1, L - 1] = value
        refused(fields_of(g, S)[0])
    api.device_synchronize(device)
    assert np.all(out.to_host((n,)) == -7.25)
    # ... and a cloudy layer with no water at all is NOT refused: zero optics, as in the library
    g = {k: v.copy() for k, v in f.items()}
    g["cf"][:], g["lwc"][:], g["iwc"][:] = 1.0, 0.0, 0.0
    api.check(lib.grt_cloud_sampler_run(sampler.p, C.byref(fields_of(g, S)[0]), out.ptr))
    api.device_synchronize(device)
    assert np.all(out.to_host((n,)) == 0.0)
    out.free()
