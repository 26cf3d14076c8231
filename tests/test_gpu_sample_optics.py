"""sample_optics (optics.c:237-302): a destination grid's points take a finer source grid's values at the same wavenumbers.
Against a numpy model of the reference's counts -- including the wn = NULL count of n + 1 points, which the reference
writes one element past the destination row with and the port clamps -- and, where the reference build exists, against
the reference's own sample_optics on host objects."""
import ctypes as C
import math

import numpy as np
import pytest

from grtcode_amd import api

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
L = 3
SOURCE = (100.0, 228.0, 0.5)                     # n = 257
DESTS = {                                        # factor 1, 2 and 5 against SOURCE, starting on and off its first point
    1: (100.0, 228.0, 0.5),
    2: (110.0, 220.0, 1.0),
    5: (105.0, 225.0, 2.5),
}


def point_index(grid, w):
    """grid_point_index (spectral_grid.c:71-83): (code, index)."""
    if w < grid.w0 or w > grid.wn:
        return api.RANGE_ERR, None
    i = int(math.floor((w - grid.w0) / grid.dw + 0.5))
    if abs(grid.w0 + i * grid.dw - w) > grid.dw * 1e-5:
        return api.VALUE_ERR, None
    return api.SUCCESS, i


def model(dest_grid, src_grid, w0, wn, layers=(L, L)):
    """The reference's checks and counts: (code, lo_d, lo_s, factor, number of points written).  The reference writes
    n_d points; the port writes no more than the destination row holds."""
    if layers[0] != layers[1]:
        return api.VALUE_ERR, None
    lower, upper, lo_d, hi_d = dest_grid.w0, dest_grid.wn, 0, dest_grid.n
    if w0 is not None:
        rc, lo_d = point_index(dest_grid, w0)
        if rc:
            return rc, None
        lower = w0
    rc, lo_s = point_index(src_grid, lower)
    if rc:
        return rc, None
    if wn is not None:
        rc, hi_d = point_index(dest_grid, wn)
        if rc:
            return rc, None
        upper = wn
    rc, hi_s = point_index(src_grid, upper)
    if rc:
        return rc, None
    if upper < lower:
        return api.RANGE_ERR, None
    n_d, n_s = hi_d - lo_d + 1, hi_s - lo_s + 1
    if n_d > n_s or n_d < 2 or (n_s - 1) % (n_d - 1) != 0:
        return api.VALUE_ERR, None
    return api.SUCCESS, (lo_d, lo_s, (n_s - 1) // (n_d - 1), min(n_d, dest_grid.n - lo_d))


def source_optics(device, grid, seed=5):
    rng = np.random.default_rng(seed)
    sets = (rng.uniform(0.0, 3.0, (L, grid.n)), rng.uniform(0.0, 1.0, (L, grid.n)), rng.uniform(-1.0, 1.0, (L, grid.n)))
    o = api.OpticsObject(L, grid, device)
    o.update(*sets)
    return o, sets


def expected(dest_grid, src_sets, lo_d, lo_s, factor, count):
    out = []
    for s in src_sets:
        d = np.full((L, dest_grid.n), SENTINEL)
        d[:, lo_d: lo_d + count] = s[:, lo_s: lo_s + factor * (count - 1) + 1: factor] if factor else s[:, lo_s: lo_s + 1]
        out.append(d)
    return out


def run_case(device, src, src_sets, dest_grid, w0, wn):
    """(code, dest's three arrays after the call, the model's code and arrays)."""
    want_rc, counts = model(dest_grid, src.c.grid, w0, wn)
    dest = api.OpticsObject(L, dest_grid, device)
    fill = np.full((L, dest_grid.n), SENTINEL)
    dest.update(fill, fill, fill)
    try:
        api.sample_optics(dest, src, w0, wn)
        rc = api.SUCCESS
    except api.GrtError as e:
        rc = e.code
    got = dest.read()
    dest.destroy()
    return rc, got, want_rc, (expected(dest_grid, src_sets, *counts) if counts else None), counts


def wavenumbers(grid, *idx):
    return [grid.w0 + i * grid.dw for i in idx]


CASES = []
for f, (a, b, dw) in DESTS.items():
    n = int(math.ceil((b - a) / dw)) + 1
    for w0, wn in ((None, None), ("lo", None), (None, "hi"), ("lo", "hi"), ("last2", None), ("last", None)):
        CASES.append((f, w0, wn))


@pytest.mark.parametrize("factor,w0,wn", CASES)
def test_values_and_untouched_points_follow_the_reference_counts(device, factor, w0, wn):
    src_grid = api.create_spectral_grid(*SOURCE)
    src, sets = source_optics(device, src_grid)
    dg = api.create_spectral_grid(*DESTS[factor])
    pick = {None: None, "lo": dg.w0 + 3 * dg.dw, "hi": dg.w0 + (dg.n - 4) * dg.dw,
            "last2": dg.w0 + (dg.n - 2) * dg.dw, "last": dg.w0 + (dg.n - 1) * dg.dw}
    rc, got, want_rc, want, counts = run_case(device, src, sets, dg, pick[w0], pick[wn])
    assert rc == want_rc, (rc, want_rc, counts)
    if want is None:
        assert all(np.all(x == SENTINEL) for x in got)          # a refused call writes nothing
    else:
        for g, w in zip(got, want):
            assert np.array_equal(g, w)
        lo_d, lo_s, f, count = counts
        assert count >= 1
        if wn is not None and w0 is not None:
            assert f == factor                                  # explicit ends: the true ratio of the grids
    src.destroy()


def test_wn_null_is_clamped_to_the_destination_row(device):
    """With wn = NULL the reference counts n_d = n - lo_d + 1 points, one more than the destination row holds.  Where it
    accepts the grids (the last two destination points: (n_s - 1) % (n_d - 1) == 0 with factor 5 -> counted factor 4), the
    port writes the row's own points and leaves the next layer's row alone."""
    src_grid = api.create_spectral_grid(*SOURCE)
    src, sets = source_optics(device, src_grid)
    dg = api.create_spectral_grid(*DESTS[5])
    w0 = dg.w0 + (dg.n - 5) * dg.dw                             # five points left: n_d = 6, n_s = 21 -> factor 4
    rc, got, want_rc, want, counts = run_case(device, src, sets, dg, w0, None)
    assert rc == want_rc == api.SUCCESS
    lo_d, lo_s, f, count = counts
    assert (f, count, dg.n - lo_d) == (4, 5, 5)                 # the reference would write a sixth point
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
        assert np.all(g[1:, 0] == SENTINEL) and np.all(g[:, :lo_d] == SENTINEL)   # next layer's first point kept
    src.destroy()


def test_refusals(device):
    src_grid = api.create_spectral_grid(*SOURCE)
    src, sets = source_optics(device, src_grid)
    dg = api.create_spectral_grid(*DESTS[2])
    cases = [
        (dg, 110.5, 150.0, api.VALUE_ERR),           # off the destination grid
        (dg, 110.0, 150.25, api.VALUE_ERR),
        (dg, 100.0, 150.0, api.RANGE_ERR),           # outside the destination grid
        (dg, 110.0, 221.0, api.RANGE_ERR),
        (dg, 150.0, 120.0, api.RANGE_ERR),           # wn < w0
        (dg, 150.0, 150.0, api.VALUE_ERR),           # w0 == wn: one point, n_d < 2 (the reference divides by zero)
        (api.create_spectral_grid(100.0, 228.0, 0.25), 100.0, 110.0, api.VALUE_ERR),     # finer than the source
        (api.create_spectral_grid(100.0, 228.0, 0.75), 100.75, 130.0, api.VALUE_ERR),   # not on the source's points
        (api.create_spectral_grid(90.0, 240.0, 1.0), None, None, api.RANGE_ERR),         # wider than the source
        (api.create_spectral_grid(90.0, 240.0, 1.0), 120.0, 230.0, api.RANGE_ERR),
    ]
    for grid, w0, wn, code in cases:
        rc, got, want_rc, _, _ = run_case(device, src, sets, grid, w0, wn)
        assert rc == want_rc == code, (grid.w0, grid.dw, w0, wn, rc, want_rc)
        assert all(np.all(x == SENTINEL) for x in got)
    other = api.OpticsObject(L + 1, dg, device)                 # different layer counts
    with pytest.raises(api.GrtError) as e:
        api.sample_optics(other, src, 110.0, 150.0)
    assert e.value.code == api.VALUE_ERR
    other.destroy()
    src.destroy()


def test_against_the_reference_build(ref, device):
    """The reference's own sample_optics on host objects: same return codes, same values.  Only with both ends given and
    wn > w0 -- with wn = NULL the reference writes past its row, and with w0 == wn it divides by zero."""
    from oracle.bindings import RefOptics
    src_grid = api.create_spectral_grid(*SOURCE)
    src, sets = source_optics(device, src_grid)
    rsrc = ref._optics(ref.grid(*SOURCE), *sets)
    checked = 0
    for dspec in list(DESTS.values()) + [(100.0, 228.0, 0.25), (100.0, 226.0, 1.5), (90.0, 240.0, 1.0)]:
        dg = api.create_spectral_grid(*dspec)
        rg = ref.grid(*dspec)
        for i0, i1 in ((0, dg.n - 1), (1, dg.n - 2), (3, 10), (0, 1), (dg.n - 2, dg.n - 1), (2, 2 + (dg.n - 3) // 2)):
            for w0, wn in ((dg.w0 + i0 * dg.dw, dg.w0 + i1 * dg.dw), (dg.w0 + i0 * dg.dw + 0.3 * dg.dw, dg.w0 + i1 * dg.dw)):
                if not wn > w0:
                    continue
                rc, got, want_rc, _, _ = run_case(device, src, sets, dg, w0, wn)
                fill = np.full((L, dg.n), SENTINEL)
                rdest = ref._optics(rg, fill, fill, fill)
                rrc = ref.lib.sample_optics(C.byref(rdest), C.byref(rsrc), C.byref(C.c_double(w0)),
                                            C.byref(C.c_double(wn)))
                rgot = ref._read_optics(rdest)
                ref.lib.destroy_optics(C.byref(rdest))
                assert rc == rrc == want_rc, (dspec, w0, wn, rc, rrc, want_rc)
                for a, b in zip(got, rgot):
                    assert np.array_equal(a, b)
                checked += rc == api.SUCCESS
    assert checked >= 10
    ref.lib.destroy_optics(C.byref(rsrc))
    src.destroy()
