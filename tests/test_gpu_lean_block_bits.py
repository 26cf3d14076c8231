"""The lean first pass (mp_lean_block.inc) bit for bit: changes to the block that only remove instructions leave every
sum and every rounding where it was, so in deterministic mode -- which fixes the order of the sums -- the optical depths
after the first pass and the gather are the bits recorded from the commit named in tests/golden/lean_first_pass_bits.npz
(tests/golden/make_lean_first_pass_bits.py wrote it).  Four grids, one per path of the block; what every line list holds
is said in tests/lean_block_cases.py."""
import os

import numpy as np
import pytest

import lean_block_cases as cases
from grtcode_amd import api
from test_gpu_gas_optics import tau_close
from test_gpu_moment_kernel import LEAN_TOL

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lean_first_pass_bits.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        assert int(z["seed"]) == cases.SEED
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def deterministic_tau(lib, device, tmp_path_factory):
    """The deterministic result of every grid, computed once: {name: (tau [2][3][321], tile ranges)}."""
    api.check(lib.grt_set_deterministic(1))
    try:
        return {name: cases.first_pass_tau(cases.band_of(tmp_path_factory.mktemp(name), name), device) for name in cases.GRIDS}
    finally:
        api.check(lib.grt_set_deterministic(-1))


@pytest.mark.parametrize("name", list(cases.GRIDS))
def test_line_list_holds_what_the_block_has_to_meet(name, deterministic_tau):
    rungs = cases.line_rungs(name)
    w0 = cases.GRIDS[name][0]
    v0 = np.array([r["v0"] for r in rungs])
    cell = np.floor(v0 - w0 + 0.5).astype(int)
    assert len(rungs) % 128 != 0
    assert np.count_nonzero((cell >= 60) & (cell <= 64)) == 0                                # empty cells
    assert np.count_nonzero(cell < 60) % 2 == 1
    # a row of 32 consecutive lines that spans three cells and more, wherever the rows begin
    sparse = np.flatnonzero((cell >= 100) & (cell < 140))
    assert np.all(cell[sparse[32:]] - cell[sparse[:-32]] >= 3)
    assert sum(r["s0"] == 0.0 for r in rungs) == 1
    half = np.abs((v0 - w0) % 1.0 - 0.5) < 1e-5
    assert np.count_nonzero(half) == 1 and rungs[int(np.flatnonzero(half)[0])]["delta"] == 0.0
    on_point = np.abs(v0 - w0 - cell) <= 2e-6
    assert 64 < np.count_nonzero(on_point) < 128                                            # a full raw batch and a partial one
    ranges = deterministic_tau[name][1]
    print(f"{name}: {len(rungs)} lines, tile ranges {ranges.tolist()}")
    assert ranges.shape == ((cases.NCELL + cases.TILE - 1) // cases.TILE, 2)
    assert ranges[1, 0] == np.count_nonzero(cell < 60) and ranges[1, 0] % 2 == 1 and ranges[1, 1] > ranges[1, 0]


@pytest.mark.parametrize("name", list(cases.GRIDS))
def test_first_pass_bits_are_the_recorded_ones(name, golden, deterministic_tau):
    got, want = deterministic_tau[name][0], golden["tau_" + name]
    assert got.shape == want.shape == (2, 3, cases.NCELL) and got.dtype == want.dtype == np.float64
    differ = np.argwhere(got != want)
    print(f"{name} ({cases.GRIDS[name][3]}): {len(differ)} of {got.size} values differ from commit {golden['commit']}"
          + (f"; first at (column, layer, point) {differ[0].tolist()}: {got[tuple(differ[0])]!r} != {want[tuple(differ[0])]!r}, "
             f"largest difference {max(tau_close(got[c], want[c]) for c in range(2)):.2e} of a layer's largest value" if len(differ) else ""))
    assert np.array_equal(got, want)


@pytest.mark.parametrize("name", list(cases.GRIDS))
def test_scheduler_order_agrees_with_the_fixed_one(name, lib, device, tmp_path, deterministic_tau):
    """The default mode: the same sums in the scheduler's order (four waves share a tile's lines)."""
    api.check(lib.grt_set_deterministic(0))
    try:
        free, _ = cases.first_pass_tau(cases.band_of(tmp_path, name), device)
    finally:
        api.check(lib.grt_set_deterministic(-1))
    det = deterministic_tau[name][0]
    err = max(tau_close(free[c], det[c]) for c in range(2))
    print(f"{name}: default mode against deterministic {err:.2e} (bound {LEAN_TOL:.1e})")
    assert err < LEAN_TOL
