"""grt_pipeline_run_cloud_fields: the batched pipeline's subcolumn all-sky pass with the cloud tables sampled on the
device from cloud fields.  In the deterministic mode it must equal, bit for bit, grt_pipeline_run_subcolumns fed the
tables grt_cloud_sampler_run returns for the same fields (that entry point is held to the oracle by
test_gpu_pipeline_subcolumns.py and test_gpu_subcolumn_shapes.py; test_gpu_cloud_sampler.py holds the tables to the
clouds library): both output forms, both pipeline forms, draws from the caller and from the generator, cloud-free
fields; the buffer the two share stays clean for the entry points that upload tables; the refusals."""
import ctypes as C

import numpy as np
import pytest

from cloud_sampler_support import SETS, pipeline_fields
from grtcode_amd import api, synthetic as syn
from pipeline_support import KEYS, _deterministic, _sentinel, _setup, limits
from pipeline_support import bands, tables  # noqa: F401  (module fixtures)
from scenario import MOL_ORDER

pytestmark = pytest.mark.gpu

# max_columns 4 with 3 columns: the shortwave's two-sweep forms park one subcolumn of the batch per launch, so the
# subcolumn solver runs in S launches
V, NCOL, S, MAX_COLUMNS, USER_LEVEL = 16, 3, 3, 4, 6


@pytest.fixture(scope="module")
def sampler(tables, device):
    gm, keep = api.make_cloud_model(tables)
    sp = api.CloudSampler(device, gm)
    yield sp
    sp.destroy()


def fields_of(f, mode, B, temperature=True):
    L = f["cf"].shape[1]
    u = np.random.default_rng(5).random((NCOL, 2, S, B, 2 * L - 1)) if mode == "uniforms" else None
    return api.make_cloud_fields(f["cf"], f["lwc"], f["iwc"], f["ov"], temperature=f["t"] if temperature else None,
                                 thickness=f["th"], num_subcolumns=S, seed=99, column_offset=17, uniforms=u)[0]


def flat(pipe, profiles):
    if not profiles:
        return np.concatenate(pipe.subcolumn_fluxes(NCOL), axis=1)
    out = pipe.subcolumn_profiles(NCOL)
    return np.concatenate([np.concatenate([out[s][k].reshape(NCOL, -1) for k in KEYS], axis=1) for s in range(2)], axis=1)


@pytest.mark.parametrize("mode", ["uniforms", "generator"])
@pytest.mark.parametrize("spectral", [False, True])
def test_cloud_fields_is_run_subcolumns_on_the_sampler_tables(bands, tables, sampler, lib, device, spectral, mode):
    cols = [syn.profile(610 + c, V) for c in range(NCOL)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, MAX_COLUMNS, USER_LEVEL, emis, alb, solar, spectral=spectral)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    B = tables["liquid"]["Band_limits_lwr"].size
    _deterministic(lib, True)
    try:
        results = {}
        for clear in (False, True):
            f = pipeline_fields(cols, 61, clear=clear)
            # (draws from the caller: fields without temperatures, so the columns' layer temperatures are taken)
            gf = fields_of(f, mode, B, temperature=mode == "generator")
            made = sampler.run(fields_of(f, mode, B))               # [4][S][ncol][3][B][L]
            assert clear == (not np.any(made))
            gclouds, kc = api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), f["th"],
                                          *[made[k].transpose(1, 0, 2, 3, 4) for k in range(len(SETS))])
            assert kc["subcolumns"] == S
            for profiles in (False, True):
                pipe.run_cloud_fields(gcols, sampler, gf, profiles=profiles)
                got = flat(pipe, profiles)
                pipe.run_subcolumns(gcols, gclouds, S, profiles=profiles)
                want = flat(pipe, profiles)
                assert np.array_equal(got, want), (clear, profiles)
                results[clear, profiles] = got
        for profiles in (False, True):
            cloudy, none = results[False, profiles], results[True, profiles]
            h = cloudy.shape[1] // 2
            if not profiles:
                # cloud-free fields: the clear-sky rows but for the mean's roundings -- S equal values added (S - 1
                # roundings) and divided by S (one more): S 2^-53 relative, to first order
                assert np.all(np.abs(none[:, h:] - none[:, :h]) <= S * 2.0 ** -52 * np.abs(none[:, :h]))
            assert np.array_equal(cloudy[:, :h], none[:, :h])
            assert np.max(np.abs(cloudy[:, h:] - cloudy[:, :h])) > 1e-3
    finally:
        _deterministic(lib, False)
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_the_shared_cloud_buffer_stays_clean_and_the_kernel_is_timed(bands, tables, sampler, lib, device):
    cols = [syn.profile(620 + c, V) for c in range(NCOL)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, MAX_COLUMNS, USER_LEVEL, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    B = tables["liquid"]["Band_limits_lwr"].size
    f = pipeline_fields(cols, 62)
    gf = fields_of(f, "generator", B)
    made = sampler.run(gf)
    one, k1 = api.make_clouds(limits(tables, "liquid"), limits(tables, "ice"), f["th"], *[made[k][1] for k in range(4)])
    _deterministic(lib, True)
    try:
        pipe.run_allsky(gcols, one)
        before = np.concatenate(pipe.allsky_fluxes(NCOL), axis=1)
        api.profile_enable(True)
        api.profile_read(api.CLOUD_SAMPLER_TAG, reset=True)
        pipe.run_cloud_fields(gcols, sampler, gf)
        means = np.concatenate(pipe.subcolumn_fluxes(NCOL), axis=1)
        ms, launches = api.profile_read(api.CLOUD_SAMPLER_TAG)
        api.profile_enable(False)
        assert launches == 1 and ms > 0.0
        pipe.run_allsky(gcols, one)
        after = np.concatenate(pipe.allsky_fluxes(NCOL), axis=1)
    finally:
        api.profile_enable(False)
        _deterministic(lib, False)
    assert np.array_equal(after, before)
    assert np.array_equal(means[:, :12], before[:, :12]) and not np.array_equal(means[:, 12:], before[:, 12:])
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()


def test_refusals_through_the_pipeline(bands, tables, sampler, lib, device):
    cols = [syn.profile(630 + c, V) for c in range(NCOL)]
    go_lw, go_sw, emis, alb, solar = _setup(bands, device, V)
    pipe = api.Pipeline(go_lw, go_sw, MAX_COLUMNS, USER_LEVEL, emis, alb, solar, spectral=False)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    B = tables["liquid"]["Band_limits_lwr"].size
    f = pipeline_fields(cols, 63)
    sizes = (8 * V, 4 * (V - 1), 24)
    outs = [_sentinel(device, MAX_COLUMNS * n) for n in sizes]

    def refused(gf, gc=gcols, sp=sampler.p, level_ptr=outs[0].ptr, fluxes_ptr=outs[2].ptr):
        with pytest.raises(api.GrtError) as e:
            api.check(lib.grt_pipeline_run_cloud_fields(pipe.p, C.byref(gc), sp, C.byref(gf) if gf is not None else None,
                                                        level_ptr, outs[1].ptr, fluxes_ptr))
        assert e.value.code == api.VALUE_ERR

    good = fields_of(f, "generator", B)
    refused(good, level_ptr=None, fluxes_ptr=None)                  # both outputs NULL
    refused(good, sp=None)
    refused(None)
    two_cols, k2 = api.make_columns(cols[:2], MOL_ORDER, cfc_order=(0, 1))
    refused(good, gc=two_cols)                                      # ncol mismatch
    refused(good, gc=two_cols, level_ptr=None)
    five = [syn.profile(640 + c, V) for c in range(MAX_COLUMNS + 1)]
    five_cols, k5 = api.make_columns(five, MOL_ORDER, cfc_order=(0, 1))
    f5 = pipeline_fields(five, 64)
    refused(api.make_cloud_fields(f5["cf"], f5["lwc"], f5["iwc"], f5["ov"], thickness=f5["th"], num_subcolumns=S)[0],
            gc=five_cols)                                           # more columns than max_columns
    short = {k: np.ascontiguousarray(v[:, :-1]) for k, v in f.items()}
    refused(fields_of(short, "generator", B))                       # layer count mismatch
    for field in ("thickness", "cloud_fraction", "overlap"):
        gf = fields_of(f, "generator", B)
        setattr(gf, field, None)
        refused(gf)
    for bad_s in (0, api.GRT_MAX_SUBCOLUMNS + 1):
        gf = fields_of(f, "generator", B)
        gf.num_subcolumns = bad_s
        refused(gf)
    g = {k: v.copy() for k, v in f.items()}
    g["cf"][1, 4] = 1.5
    refused(fields_of(g, "generator", B))
    g = {k: v.copy() for k, v in f.items()}
    g["iwc"][2, 0] = -1.0
    refused(fields_of(g, "generator", B))
    pipe.sync()
    for buf, n in zip(outs, sizes):
        assert np.all(buf.to_host((MAX_COLUMNS * n,)) == -7.25)
        buf.free()
    pipe.destroy()
    go_lw.destroy()
    go_sw.destroy()
