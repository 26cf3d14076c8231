"""grt_multi_gather_rows (include/grt_ext.h): the gather of grt_multi_gather_fluxes for rows of any width -- e.g. the
level fluxes and heating rates of grt_pipeline_run_profiles, 4 V + 2 (V - 1) doubles per column -- through the file
transport, one fresh process per rank (no GPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RANK = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from grtcode_amd import multi
rank, world, ncol, width, rdv = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
m = multi.Multi(multi.FILES, 0, rank, world, rdv)
first, count = m.shard(ncol)
per = -(-ncol // world)


def block(cols, w, step):
    return np.array([[1000.0 * c + 0.5 * k + 0.125 * step for k in range(w)] for c in cols], dtype=np.float64).reshape(len(cols), w)


for step in range(2):                                 # two gathers in a row: one call's files never meet the next's
    local = block(range(first, first + count), width, step)
    out = np.full((per * world, width), -1.0) if rank == 0 else None
    m.gather_rows(local.ctypes.data if count else 0, ncol, width, out.ctypes.data if rank == 0 else 0, False)
    if rank == 0:
        assert np.array_equal(out[:ncol], block(range(ncol), width, step)), step
        assert np.all(out[ncol:] == 0.0)
# rows of 12: grt_multi_gather_fluxes and grt_multi_gather_rows(..., 12, ...) deliver the same bytes
local = block(range(first, first + count), 12, 7)
got = []
for use_rows in (False, True):
    out = np.full((per * world, 12), -1.0) if rank == 0 else None
    args = (local.ctypes.data if count else 0, ncol)
    if use_rows:
        m.gather_rows(*args, 12, out.ctypes.data if rank == 0 else 0, False)
    else:
        m.gather_fluxes(*args, out.ctypes.data if rank == 0 else 0, False)
    got.append(out)
if rank == 0:
    assert got[0].tobytes() == got[1].tobytes()
    assert np.array_equal(got[0][:ncol], block(range(ncol), 12, 7))
assert m.max(1.0 + rank) == float(world)
m.destroy()
print("rank", rank, "ok")
"""


def _run_ranks(tmp_path, world, ncol, width):
    script = tmp_path / "rank.py"
    script.write_text(RANK % {"root": ROOT})
    rdv = tmp_path / "rdv"
    rdv.mkdir()
    env = dict(os.environ, GRT_MULTI_TIMEOUT="120")
    env.pop("GRT_MULTI_JOB", None)
    procs = [subprocess.Popen([sys.executable, str(script), str(r), str(world), str(ncol), str(width), str(rdv)],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env) for r in range(world)]
    for r, p in enumerate(procs):
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, (r, out, err[-2000:])
        assert f"rank {r} ok" in out
    assert os.listdir(rdv) == []


@pytest.mark.parametrize("world,ncol", [(2, 5), (3, 7), (3, 2)])
def test_profile_rows_reach_rank_zero_in_column_order(tmp_path, world, ncol):
    """Rows of 4 V + 2 (V - 1) = 242 doubles (V = 61): uneven shards (3 + 2, 3 + 3 + 1) and an empty one (1 + 1 + 0)."""
    V = 61
    _run_ranks(tmp_path, world, ncol, 4 * V + 2 * (V - 1))


ONE_RANK = r"""
import sys
import numpy as np
sys.path.insert(0, %(root)r)
from grtcode_amd import multi
use_rows, rdv = sys.argv[1] == "1", sys.argv[2]
m = multi.Multi(multi.FILES, 0, 1, 2, rdv)
first, count = m.shard(5)
local = np.arange(count * 12, dtype=np.float64).reshape(count, 12) + 0.25
if use_rows:
    m.gather_rows(local.ctypes.data, 5, 12, 0, False)
else:
    m.gather_fluxes(local.ctypes.data, 5, 0, False)
m.destroy()
"""


def test_gather_fluxes_is_gather_rows_of_twelve_on_disk(tmp_path):
    """Rank 1 alone (a gather needs no two ranks alive at once): what it leaves for rank 0 -- the exchange file's name and
    its bytes -- is the same whether it called grt_multi_gather_fluxes or grt_multi_gather_rows with rows of 12."""
    script = tmp_path / "one.py"
    script.write_text(ONE_RANK % {"root": ROOT})
    seen = []
    for use_rows in ("0", "1"):
        rdv = tmp_path / f"rdv{use_rows}"
        rdv.mkdir()
        env = dict(os.environ, GRT_MULTI_TIMEOUT="30")
        env.pop("GRT_MULTI_JOB", None)
        p = subprocess.run([sys.executable, str(script), use_rows, str(rdv)], capture_output=True, text=True, timeout=120,
                           env=env)
        assert p.returncode == 0, p.stderr[-2000:]
        seen.append({name: (rdv / name).read_bytes() for name in sorted(os.listdir(rdv))})
    assert seen[0] == seen[1]
    blocks = [name for name in seen[0] if name.startswith("fluxes_")]
    assert blocks == ["fluxes_0_0_rank1.bin"]
    got = np.frombuffer(seen[0][blocks[0]], dtype=np.float64)
    assert np.array_equal(got, np.arange(2 * 12, dtype=np.float64) + 0.25)      # rank 1 of 5 columns over 2: 2 rows
