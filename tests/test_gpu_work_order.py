"""The lockstep work order (grtcode_amd/csrc/grt_work_order.h) on the device: placement affects speed only.

A band of 300 grid points at 1 cm-1 in 64-cell tiles -- five tiles, the last one 44 cells short -- with about 2 000 lines
and 3 layers, so that a launch has 15 workgroups a column: no multiple of the 8 XCDs the ids are dealt to.  Every form
that walks the order runs here: the ring kernel in the reference's operation order (fast = 0, 1e-11 of a layer's largest
tau against the oracle, as everywhere in the suite) and the two-pass cell-moment form (fast = 3, 2e-6: its fp32 far
field), with equal line slices (tune(nslice=2): the slices add to tau with atomics), with the launch's work list
(slices left to the library) and, in the deterministic mode, in its phase launches of non-overlapping tiles."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api, synthetic as syn
from scenario import Band, MOL_ORDER, RUN_TO_RUN_FUSED
from test_gpu_gas_optics import tau_close

pytestmark = pytest.mark.gpu

V, NCOL, TILE = 4, 3, 64
ORACLE_TOL = {0: 1e-11, 3: 2e-6}
# one column of a batch against the same column launched alone, default mode: the reference-order form sums in fp64 only
# (tests/test_gpu_batch.py); the fused form's atomics land in the scheduler's order (scenario.RUN_TO_RUN_FUSED)
BATCH_TOL = {0: 1e-13, 3: RUN_TO_RUN_FUSED}


@pytest.fixture(scope="module")
def case(tmp_path_factory, oracle, lib):
    band = Band(str(tmp_path_factory.mktemp("work_order")), 600.0, 899.0, 1.0, 2000)
    assert band.nw == 300 and -(-band.nw // TILE) == 5 and band.nw % TILE != 0
    cols = [syn.profile(40 + c, V) for c in range(NCOL)]
    want = [band.oracle_tau(oracle, oracle, lib, col) for col in cols]
    return band, cols, want


def batch_tau(lib, device, band, cols, fast, nslice=0):
    """tau [len(cols)][layers][nw] of ONE launch over these columns, and what the launch was."""
    go, _ = band.gas_optics(device, V, from_file=False)
    go.tune(tile=TILE, nslice=nslice, fast=fast)
    gcols, keep = api.make_columns(cols, MOL_ORDER, cfc_order=(0, 1))
    buf = api.DeviceBuffer(device, 8 * len(cols) * (V - 1) * band.nw)
    api.check(lib.grt_optical_depth_batch(C.byref(go.c), C.byref(gcols), buf.ptr))
    tau = buf.to_host((len(cols), V - 1, band.nw)).copy()
    info = go.last_launch()
    buf.free()
    go.destroy()
    assert (info["fast"], info["tile"], info["columns_per_launch"]) == (fast, TILE, len(cols)), info
    return tau, info


@pytest.mark.parametrize("fast", [0, 3])
def test_one_column_of_fifteen_workgroups(case, lib, device, fast):
    band, cols, want = case
    tau, info = batch_tau(lib, device, band, cols[:1], fast, nslice=1)
    assert info["nslice"] == 1, info
    assert tau_close(tau[0], want[0]) < ORACLE_TOL[fast]


@pytest.mark.parametrize("mode", ["as_run", "deterministic"])
@pytest.mark.parametrize("fast", [0, 3])
def test_columns_of_one_launch_equal_the_columns_launched_alone(case, lib, device, fast, mode):
    band, cols, want = case
    if mode == "deterministic":
        api.check(lib.grt_set_deterministic(1))
    try:
        bitwise = bool(lib.grt_deterministic())
        together, _ = batch_tau(lib, device, band, cols, fast, nslice=1)
        for c in range(NCOL):
            alone, _ = batch_tau(lib, device, band, cols[c:c + 1], fast, nslice=1)
            if bitwise:
                assert np.array_equal(together[c], alone[0]), (c, tau_close(together[c], alone[0]))
            else:
                assert tau_close(together[c], alone[0]) < BATCH_TOL[fast], c
            assert tau_close(together[c], want[c]) < ORACLE_TOL[fast], c
    finally:
        if mode == "deterministic":
            api.check(lib.grt_set_deterministic(-1))


@pytest.mark.parametrize("fast,nslice", [(0, 2), (3, 2), (3, 0)], ids=["ring_two_slices", "two_pass_two_slices", "two_pass_work_list"])
def test_one_column_in_line_slices_and_by_the_work_list(case, lib, device, fast, nslice):
    band, cols, want = case
    tau, info = batch_tau(lib, device, band, cols[:1], fast, nslice=nslice)
    if not lib.grt_deterministic():         # (the deterministic mode takes one slice per tile and no work list)
        assert info["nslice"] == (2 if nslice == 2 else 1), info
    assert tau_close(tau[0], want[0]) < ORACLE_TOL[fast]
