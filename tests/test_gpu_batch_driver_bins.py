"""examples/rfmip_batch_driver.c -bin-width: every column's fluxes integrated over wavenumber bins through the C driver,
on one rank and gathered from three (grt_multi_gather_rows, file transport)."""
import os
import subprocess

import numpy as np
import pytest

from scenario import Band
from driver_support import batch_flags, build_example, rfmip_like_columns, run_driver, write_grtc_dump

pytestmark = pytest.mark.gpu

GRIDS = {"lwbin": (1.0, 2000.0, 1.0), "swbin": (1.0, 6000.0, 2.0)}      # w0, wn, dw of the two bands the driver runs


def bin_lines(stdout):
    """the lines after each col line that belong to it: {column: {"col": line, "lwbin": [lines], "swbin": [lines]}}"""
    out, cur = {}, None
    for line in stdout.splitlines():
        head = line.partition(":")[0]
        kind, _, idx = head.partition(" ")
        if kind == "col":
            cur = out.setdefault(int(idx), {"col": line, "lwbin": [], "swbin": []})
        elif kind in ("lwbin", "swbin"):
            assert cur is not None and len(cur[kind]) == int(idx), line
            cur[kind].append(line)
    return out


def values(line):
    return np.array([float(x) for x in line.partition(":")[2].split()])


def test_driver_prints_bins_on_one_and_three_ranks(tmp_path):
    V, ncol, width = 9, 5, 50.0
    cols, raw = rfmip_like_columns(ncol, V)
    swb = Band(str(tmp_path / "data"), 1.0, 6000.0, 2.0, 6000, sw=True)
    dump = write_grtc_dump(str(tmp_path / "columns.bin"), ncol, V, raw)
    exe = build_example("rfmip_batch_driver", str(tmp_path / "rfmip_batch_driver"), backtrace=True)
    (lw0, lwn, lwd), (sw0, swn, swd) = GRIDS["lwbin"], GRIDS["swbin"]
    # one column per batch: every gas-optics launch has the same shape on one rank and on three, so that the deterministic
    # mode makes the lines of the two runs the same text
    args = [exe, swb.par, swb.files["solar"], dump,
            *batch_flags(swb, (str(lw0), str(lwn), str(lwd)), (str(sw0), str(swn), str(swd)), 1)]
    env = dict(os.environ, GRT_DETERMINISTIC="1")
    plain = run_driver(args, env=env)
    assert plain.returncode == 0, plain.stderr[-3000:]
    binned = run_driver(args + ["-bin-width", str(width)], env=env)
    assert binned.returncode == 0, binned.stderr[-3000:]
    assert not any(l.startswith(("lwbin ", "swbin ")) for l in plain.stdout.splitlines())      # opt-in
    got = bin_lines(binned.stdout)
    assert sorted(got) == list(range(ncol))
    assert [got[c]["col"] for c in range(ncol)] == [l for l in plain.stdout.splitlines() if l.startswith("col ")]
    for c, col in enumerate(cols):
        broadband = values(got[c]["col"])
        for kind, k in (("lwbin", 0), ("swbin", 4)):
            w0, wn, dw = GRIDS[kind]
            n = int(round((wn - w0) / dw)) + 1
            step = int(round(width / dw))
            rows = np.array([values(l) for l in got[c][kind]])
            nb = (n - 1 + step - 1) // step
            assert rows.shape == (nb, 6), kind
            # bin limits: every `step` points from the first, the last bin ends at the last point, adjacent bins share
            # their edge
            assert rows[0, 0] == w0 and rows[-1, 1] == w0 + (n - 1) * dw
            assert np.array_equal(rows[1:, 0], rows[:-1, 1])
            assert np.allclose(rows[:-1, 1] - rows[:-1, 0], step * dw, rtol=0, atol=1e-9)
            assert 0 < rows[-1, 1] - rows[-1, 0] <= step * dw + 1e-9
            # the bins add up to the col line's four values of the band
            total = rows[:, 2:].sum(axis=0)
            want = broadband[k:k + 4]
            assert np.all(np.abs(total - want) <= 1e-12 * np.abs(rows[:, 2:]).sum(axis=0)), (c, kind)
        if col["mu0"] <= 0:
            assert np.all(rows[:, 2:] == 0.0)                                             # night: no shortwave
        else:
            assert np.all(rows[:, 4] > 0.0)                                              # sunlit: shortwave down at TOA

    # the same run as three ranks, the bins gathered to rank 0 through grt_multi_gather_rows (file transport)
    rdv = tmp_path / "rdv"
    rdv.mkdir()
    procs = [subprocess.Popen(args + ["-bin-width", str(width), "-ranks", "3", "-rank", str(k), "-rendezvous", str(rdv),
                                      "-transport", "files"],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                              env=dict(env, GRT_MULTI_TIMEOUT="300")) for k in range(3)]
    outs = [p.communicate(timeout=900) for p in procs]
    for k, p in enumerate(procs):
        assert p.returncode == 0, (k, outs[k][1][-2000:])
    assert not any(bin_lines(outs[k][0]) for k in (1, 2))                                    # only rank 0 reports

    def results(text):
        return [l for l in text.splitlines() if l.startswith(("col ", "lwbin ", "swbin "))]
    assert results(outs[0][0]) == results(binned.stdout)
