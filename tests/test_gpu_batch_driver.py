"""§8(f)-1, data-adapter side: examples/rfmip_batch_driver.c -- RFMIP-style columns (Pa, layer mole fractions for
H2O/O3, global means for the rest, zenith angle in degrees; rfmip-irf/src/rfmip-irf.c:175-325) from a flat dump,
through the batched device pipeline from plain C linked against the static archives -- against the oracle."""
import os
import subprocess

import numpy as np
import pytest

from grtcode_amd import api
from scenario import Band
from driver_support import batch_flags, build_example, col_lines, rfmip_like_columns, run_driver, write_grtc_dump
from pipeline_support import oracle_column

pytestmark = pytest.mark.gpu


def test_batched_c_driver_matches_oracle(tmp_path, oracle, lib):
    V, ncol = 13, 7
    cols, raw = rfmip_like_columns(ncol, V)
    swb = Band(str(tmp_path / "data"), 1.0, 6000.0, 2.0, 8000, sw=True)
    lwb = Band(str(tmp_path / "lw_view"), 1.0, 2000.0, 1.0, 0, sw=True)
    lwb.par, lwb.h2o_dir, lwb.files, lwb.tab = swb.par, swb.h2o_dir, swb.files, swb.tab
    lwb.lines = {m: {k: a[(ln["v0"] >= lwb.w0) & (ln["v0"] <= lwb.wn)] for k, a in ln.items()}
                 for m, ln in swb.lines.items()}
    dump = write_grtc_dump(str(tmp_path / "columns.bin"), ncol, V, raw)
    exe = build_example("rfmip_batch_driver", str(tmp_path / "rfmip_batch_driver"), backtrace=True)
    args = [exe, swb.par, swb.files["solar"], dump, *batch_flags(swb, ("1", "2000", "1"), ("1", "6000", "2"), 3)]
    r = run_driver(args)
    assert r.returncode == 0, r.stderr[-3000:]
    # soak (GRT_TEST_REPEAT_DRIVER=N): a crash on the way in or out shows its backtrace; in the deterministic mode the
    # whole C driver's output repeats to the last digit
    first = None
    for _ in range(int(os.environ.get("GRT_TEST_REPEAT_DRIVER", 2))):
        again = run_driver(args, env=dict(os.environ, GRT_DETERMINISTIC="1"))
        assert again.returncode == 0, again.stderr[-3000:]
        first = first or again.stdout
        assert again.stdout == first
    got = col_lines(r.stdout)
    assert sorted(got) == list(range(ncol))
    grid_sw = api.create_spectral_grid(swb.w0, swb.wn, swb.dw)
    solar = api.create_solar_flux(grid_sw, swb.files["solar"])
    worst = 0.0
    for c, col in enumerate(cols):
        emis, alb = np.full(lwb.nw, col["emis"]), np.full(swb.nw, col["alb"])
        w = oracle_column(oracle, lib, lwb, col, True, emis)
        worst = max(worst, np.max(np.abs(got[c][:4] - w["integ"][[0, 1, 3, 4]])))
        if col["mu0"] > 0:
            w = oracle_column(oracle, lib, swb, col, False, emis, alb, solar)
            worst = max(worst, np.max(np.abs(got[c][4:] - w["integ"][[0, 1, 3, 4]])))
        else:
            assert np.all(got[c][4:] == 0.0)                          # night: no shortwave (driver.c:706)
    print(f"batched C driver, {ncol} columns: worst flux difference {worst:.2e} W m-2")
    assert worst < 1e-4

    # ---- the same run as THREE ranks (one process each, sharing this GPU), 7 columns -> blocks of 3, 3, 1, flux blocks
    # gathered to rank 0 through the library's C entry points grt_multi_* (SURVEY §8e).  File transport here: RCCL wants
    # one GPU per rank (below: RCCL at world size 1).
    rdv = tmp_path / "rdv"
    rdv.mkdir()
    procs = [subprocess.Popen(args + ["-ranks", "3", "-rank", str(k), "-rendezvous", str(rdv), "-transport", "files"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(os.environ, GRT_MULTI_TIMEOUT="300")) for k in range(3)]
    outs = [p.communicate(timeout=900) for p in procs]
    for k, p in enumerate(procs):
        assert p.returncode == 0, (k, outs[k][1][-2000:])
    sharded = col_lines(outs[0][0])
    assert sorted(sharded) == list(range(ncol))
    assert not any(l.startswith("col ") for k in (1, 2) for l in outs[k][0].splitlines())     # only rank 0 reports
    for c in range(ncol):
        assert np.max(np.abs(sharded[c] - got[c])) < 1e-7          # a column's fluxes do not depend on its shard (atomics: ~1e-9)

    # ---- RCCL transport, world size 1: communicator through the rendezvous directory, ncclGather on the library stream
    rdv1 = tmp_path / "rdv1"
    rdv1.mkdir()
    r = subprocess.run(args + ["-ranks", "1", "-rank", "0", "-rendezvous", str(rdv1)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]                      # (-ranks 1: no communicator is made)
    from grtcode_amd import multi
    import ctypes as C
    m = multi.Multi(multi.RCCL, 0, 0, 1, str(rdv1))
    assert (rdv1 / "rccl_unique_id.bin").stat().st_size == 128
    block = np.arange(5 * 12, dtype=np.float64).reshape(5, 12)
    src, dst = api.DeviceBuffer(0, block.nbytes), api.DeviceBuffer(0, block.nbytes)
    api.check(lib.grt_host_to_device(0, src.ptr, block.ctypes.data_as(C.c_void_p), block.nbytes))
    m.gather_fluxes(src.ptr.value, 5, dst.ptr.value, True)
    assert m.max(3.25) == 3.25                                       # (synchronises the stream)
    assert np.array_equal(dst.to_host((5, 12)), block)
    m.destroy()
    assert not (rdv1 / "rccl_unique_id.bin").exists()               # rank 0 clears the id: the directory can be reused
    src.free()
    dst.free()
