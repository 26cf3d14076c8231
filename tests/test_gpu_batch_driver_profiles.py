"""examples/rfmip_batch_driver.c -profiles: level fluxes and heating rates of every column through the C driver, on one
rank and gathered from three (grt_multi_gather_rows, file transport)."""
import os
import subprocess

import numpy as np
import pytest

from scenario import Band
from driver_support import batch_flags, build_example, rfmip_like_columns, run_driver, write_grtc_dump

pytestmark = pytest.mark.gpu


def parse(stdout):
    """{column: {"col": [8], "lev": [V][4], "lay": [L][2]}} from the driver's lines, in the order they came."""
    out, cur = {}, None
    for line in stdout.splitlines():
        head, _, vals = line.partition(":")
        kind, _, idx = head.partition(" ")
        if kind not in ("col", "lev", "lay"):
            continue
        v = [float(x) for x in vals.split()]
        if kind == "col":
            cur = out.setdefault(int(idx), {"col": np.array(v), "lev": [], "lay": []})
        else:
            assert cur is not None and len(cur[kind]) == int(idx), line
            cur[kind].append(v)
    return {c: {k: np.array(x) for k, x in d.items()} for c, d in out.items()}


def test_driver_prints_level_fluxes_and_heating_rates(tmp_path):
    V, ncol = 13, 7
    L = V - 1
    cols, raw = rfmip_like_columns(ncol, V)
    swb = Band(str(tmp_path / "data"), 1.0, 6000.0, 2.0, 8000, sw=True)
    dump = write_grtc_dump(str(tmp_path / "columns.bin"), ncol, V, raw)
    exe = build_example("rfmip_batch_driver", str(tmp_path / "rfmip_batch_driver"), backtrace=True)
    args = [exe, swb.par, swb.files["solar"], dump, *batch_flags(swb, ("1", "2000", "1"), ("1", "6000", "2"), 3)]
    env = dict(os.environ, GRT_DETERMINISTIC="1")
    plain = run_driver(args, env=env)
    assert plain.returncode == 0, plain.stderr[-3000:]
    prof = run_driver(args + ["-profiles"], env=env)
    assert prof.returncode == 0, prof.stderr[-3000:]
    assert not any(l.startswith(("lev ", "lay ")) for l in plain.stdout.splitlines())     # opt-in
    col_lines = [l for l in plain.stdout.splitlines() if l.startswith("col ")]
    assert len(col_lines) == ncol
    assert [l for l in prof.stdout.splitlines() if l.startswith("col ")] == col_lines
    got = parse(prof.stdout)
    assert sorted(got) == list(range(ncol))
    for c, col in enumerate(cols):
        g = got[c]
        assert g["lev"].shape == (V, 4) and g["lay"].shape == (L, 2)
        rlut, rlus, rldt, rlds, rsut, rsus, rsdt, rsds = g["col"]
        top, sfc = g["lev"][0], g["lev"][L]
        assert top[0] == rlut and top[1] == rldt and sfc[0] == rlus and sfc[1] == rlds         # longwave: the same doubles
        want = np.array([rsut, rsdt, rsus, rsds])
        have = np.array([top[2], top[3], sfc[2], sfc[3]])
        assert np.all(np.abs(have - want) <= 1e-12 * max(1.0, np.abs(want).max()))          # shortwave: two sweeps
        assert np.all(np.isfinite(g["lay"])) and np.abs(g["lay"][:, 0]).max() > 0.0
        if col["mu0"] <= 0:
            assert np.all(g["lev"][:, 2:] == 0.0) and np.all(g["lay"][:, 1] == 0.0)         # night: no shortwave
        else:
            assert np.all(g["lev"][:, 3] > 0.0) and np.abs(g["lay"][:, 1]).max() > 0.0

    # the same run as three ranks, the rows gathered to rank 0 through grt_multi_gather_rows (file transport)
    rdv = tmp_path / "rdv"
    rdv.mkdir()
    procs = [subprocess.Popen(args + ["-profiles", "-ranks", "3", "-rank", str(k), "-rendezvous", str(rdv), "-transport", "files"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(env, GRT_MULTI_TIMEOUT="300")) for k in range(3)]
    outs = [p.communicate(timeout=900) for p in procs]
    for k, p in enumerate(procs):
        assert p.returncode == 0, (k, outs[k][1][-2000:])
    assert not any(parse(outs[k][0]) for k in (1, 2))                                       # only rank 0 reports
    sharded = parse(outs[0][0])
    assert sorted(sharded) == list(range(ncol))
    for c in range(ncol):
        for k in ("col", "lev", "lay"):
            a, b = sharded[c][k], got[c][k]
            assert a.shape == b.shape
            # a column's numbers do not depend on its shard (gas-optics launch shapes differ with the batch: ~1e-9)
            assert np.all(np.abs(a - b) <= 1e-7 * max(1.0, np.abs(b).max())), (c, k)
