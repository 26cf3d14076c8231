"""Cost of grt_pipeline_run_cloud_fields against grt_pipeline_run_subcolumns with ready-made tables on the G1 workload
(grtcode_amd.workload: 64 columns, 61 levels, the bench's grids and line lists, fast = 3), and of what the device sampler
replaces: the host library's grt_clouds_band_optics, once per column, pass and subcolumn.

Five alternating repetitions of these steps on one pipeline, S = 1 and 8:
  sub_S / subprof_S          grt_pipeline_run_subcolumns, six-row / profile form, fed the tables the sampler made for the
                             same fields (so both steps solve the same clouds): the yardstick
  fields_S / fieldsprof_S    grt_pipeline_run_cloud_fields, six-row / profile form, generator mode
Per step: the wall time, synchronised, and the sampler kernel's time by HIP-event profile tag 16.  The target: a
cloud-fields step does not exceed its yardstick by more than the yardstick's spread (max - min).
--host-only: only the host library's timing (no GPU needed): 64 columns x 2 passes x 8 subcolumns calls at 60 layers.
Result: profiles/pipeline_cloud_fields_timing.json (or the path given).

    python scripts/time_pipeline_cloud_fields.py [--reps 5] [--host-only] [--out profiles/pipeline_cloud_fields_timing.json]
"""
import ctypes
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

from pipeline_timing import ROOT, Session  # (first: it puts the repository root on sys.path)
from grtcode_amd import api
from grtcode_amd.dumpfile import write_dump

sys.path.insert(0, os.path.join(ROOT, "tests"))
from cloud_model import synthetic_tables  # noqa: E402

COUNTS = (1, 8)
LIQUID_EDGES = [10.0, 350.0, 700.0, 1200.0, 2000.0, 3500.0, 8000.0, 20000.0, 50000.0]          # pipeline_timing's bands
ICE_EDGES = [10.0, 250.0, 500.0, 800.0, 1300.0, 2200.0, 4000.0, 9000.0, 18000.0, 30000.0, 52000.0]


def model_tables(root, liquid_edges=LIQUID_EDGES, ice_edges=ICE_EDGES):
    os.makedirs(os.path.join(root, "i"), exist_ok=True)
    _, t = synthetic_tables(root, seed=4, band_edges=liquid_edges)
    _, ti = synthetic_tables(os.path.join(root, "i"), seed=9, band_edges=ice_edges)
    t["ice"] = ti["ice"]
    return t


def fields(p, tl, seed=1):
    """Cloud in about a third of the layers, liquid in the lower half, ice in the upper half."""
    ncol, L = tl.shape
    rng = np.random.default_rng(seed)
    cf = np.where(rng.random((ncol, L)) < 1.0 / 3.0, 0.1 + 0.9 * rng.random((ncol, L)), 0.0)
    low = np.arange(L)[None, :] >= L // 2
    lwc = np.where((cf > 0) & low, 0.2 * rng.random((ncol, L)), 0.0)
    iwc = np.where((cf > 0) & ~low, 0.03 * rng.random((ncol, L)), 0.0)
    overlap = np.exp(-np.abs(np.diff(np.log(p[:, 1:] + p[:, :-1]), axis=1)) / 0.5)
    return dict(cf=cf, lwc=lwc, iwc=iwc, ov=overlap, th=29.3 * tl * np.log(p[:, 1:] / p[:, :-1]), t=tl)


def host_library_ms(tables, ncol=64, S=8, L=60, reps=5):
    """Median wall time of ncol x 2 x S calls of grt_clouds_band_optics (grt_clouds.c, gcc -O2) at L layers."""
    dp = ctypes.POINTER(ctypes.c_double)
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libclouds_timing.so")
        subprocess.check_call(["gcc", "-std=gnu99", "-O2", "-ffp-contract=off", "-fPIC", "-shared",
                               "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "grtcode_amd", "csrc", "host", "grt_clouds.c"), "-o", so, "-lm"])
        paths = {}
        for k in ("beta", "ice", "liquid"):
            paths[k] = os.path.join(tmp, k + ".dump")
            write_dump(paths[k], tables[k])
        lib = ctypes.CDLL(so)
        lib.grt_clouds_band_optics.argtypes = [ctypes.c_int, dp, dp, dp, dp, ctypes.c_double, dp, dp, dp]
        assert lib.initialize_clouds_lib(paths["beta"].encode(), paths["ice"].encode(), paths["liquid"].encode()) == 0
        B = tables["liquid"]["Band_limits_lwr"].size
        p = np.tile(np.linspace(1.0, 1000.0, L + 1), (ncol, 1))
        f = fields(p, np.tile(np.linspace(210.0, 290.0, L), (ncol, 1)))
        liq, ice = np.zeros((3, B, L)), np.zeros((3, B, L))
        ptr = lambda a: a.ctypes.data_as(dp)
        rows = [[np.ascontiguousarray(f[k][c]) for k in ("cf", "lwc", "iwc", "ov", "t")] for c in range(ncol)]
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            for cf, lwc, iwc, ov, t in rows:
                for _call in range(2 * S):
                    lib.grt_clouds_band_optics(L, ptr(cf), ptr(lwc), ptr(iwc), ptr(ov), 10.0, ptr(t), ptr(liq), ptr(ice))
            ms.append(1e3 * (time.perf_counter() - t0))
        lib.finalize_clouds_lib()
    return {"bands": int(B), "num_x": int(tables["beta"]["x"].size), "calls": ncol * 2 * S, "layers": L,
            "median_ms": float(np.median(ms)), "samples_ms": ms,
            "table_megabytes": 8e-6 * 4 * ncol * S * 3 * B * L}


def host_cost():
    with tempfile.TemporaryDirectory() as tmp:
        return {"synthetic_6_bands": host_library_ms(model_tables(os.path.join(tmp, "a"), np.linspace(10.0, 3000.0, 7),
                                                                  np.linspace(10.0, 3000.0, 7))),
                "synthetic_8_liquid_10_ice_bands": host_library_ms(model_tables(os.path.join(tmp, "b")))}


def main():
    if "--host-only" in sys.argv:
        import json
        print(json.dumps(host_cost()))
        return
    s = Session("pipeline_cloud_fields_timing.json", lambda ap: ap.add_argument("--host-only", action="store_true"))
    pipe, gcols, lib, C = s.pipe, s.gcols, s.lib, api.C
    with tempfile.TemporaryDirectory() as tmp:
        tables = model_tables(tmp)
    gm, keep_model = api.make_cloud_model(tables)
    sampler = api.CloudSampler(s.device, gm)
    f = fields(s.keep["p"], s.keep["tl"])
    limits = lambda ph: (keep_model[ph]["band_lo"], keep_model[ph]["band_hi"])
    gfields, gclouds = {}, {}
    for n in COUNTS:
        gfields[n] = api.make_cloud_fields(f["cf"], f["lwc"], f["iwc"], f["ov"], temperature=f["t"], thickness=f["th"],
                                           num_subcolumns=n, seed=2024)[0]
        made = sampler.run(gfields[n])
        gclouds[n] = api.make_clouds(limits("liquid"), limits("ice"), f["th"],
                                     *[np.ascontiguousarray(made[k].transpose(1, 0, 2, 3, 4)) for k in range(4)])
    out = s.buffer(api.GRT_ALLSKY_FLUXES_PER_COLUMN)
    levels, heating, prof_out = s.profile_outputs(2)

    def step(mode):
        kind, _, n = mode.partition("_")
        ptrs = (levels.ptr, heating.ptr, prof_out.ptr) if kind.endswith("prof") else (None, None, out.ptr)
        if kind.startswith("sub"):
            api.check(lib.grt_pipeline_run_subcolumns(pipe.p, C.byref(gcols), C.byref(gclouds[int(n)][0]), int(n), *ptrs))
        else:
            api.check(lib.grt_pipeline_run_cloud_fields(pipe.p, C.byref(gcols), sampler.p, C.byref(gfields[int(n)]), *ptrs))

    pairs = [(f"{a}_{n}", f"{b}_{n}") for n in COUNTS for a, b in (("sub", "fields"), ("subprof", "fieldsprof"))]
    modes = [m for pair in pairs for m in pair]
    samples, median, spread = s.measure(modes, step, {"sampler_ms": api.CLOUD_SAMPLER_TAG})
    verdict = {new: {"yardstick_ms": median[old]["wall_ms"], "yardstick_spread_ms": spread[old]["wall_ms"],
                     "cloud_fields_ms": median[new]["wall_ms"], "sampler_kernel_ms": median[new]["sampler_ms"],
                     "within_spread": median[new]["wall_ms"] <= median[old]["wall_ms"] + spread[old]["wall_ms"]}
               for old, new in pairs}
    result = {"workload": s.workload + "; cloud in about a third of the layers; 8 liquid and 10 ice bands",
              "reps": s.args.reps, "order": ", ".join(modes) + " alternating; medians over the repetitions",
              "median": median, "spread": spread, "samples": samples, "verdict": verdict, "host_library": host_cost(),
              "target": "cloud_fields_ms <= yardstick_ms + yardstick_spread_ms"}
    sampler.destroy()
    s.finish(result, ("verdict", "host_library"))


if __name__ == "__main__":
    main()
