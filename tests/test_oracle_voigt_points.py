"""The point set of tests/voigt_points.py (CPU): that it is what the GPU test needs, and that the oracle's per-point
entry orc_voigt_xy is the reference's own rfm_voigt_line_shape at every one of its points.

The reference takes a grid and two widths, not (x, y).  With alpha = (double)0.832554611f its REPWID (RFM_voigt.c:94) is
exactly 1.0f; with centre 0 and a single point at w = x its X (:165) is x, and with gamma = y its Y (:95) is y.  What it
returns is RSQRPI*REPWID*K (:278: the fp32 product of the two constants, widened, times the double K) -- the oracle's K
is held to it by forming that same product, which is exact where a division by the scaling would round a second time --
and K itself in the pure-Lorentz branch (:103).  The bound is that of the Voigt fixture in tests/test_oracle_golden.py:
every double equal."""
import numpy as np
import pytest

import voigt_points as vp

F = np.float32


@pytest.fixture(scope="module")
def pts():
    return vp.build()


def test_point_set_is_fp32_and_mostly_away_from_the_limits(pts):
    x, y, adj = pts["x"], pts["y"], pts["adjacent"]
    assert x.dtype == F and y.dtype == F and x.size == y.size
    print(f"{x.size} points, {np.unique(y).size} values of y, {int(adj.sum())} limit-adjacent")
    assert 3e4 <= x.size <= 2 ** 18
    assert 0 < adj.sum() < 0.10 * x.size
    # every special y is there
    for c in (F(0.000001), F(8.425), F(6.8)):
        assert all(np.any(y == v) for v in (vp.steps(c, -1), c, vp.steps(c, 1)))
    assert np.any(y == 0) and np.any(y == F(1.5)) and np.any(y == vp.steps(F(70.55), -1)) and np.any(y == F(70.55))


def test_every_region_is_hit_away_from_the_limits(pts):
    code, adj = pts["code"], pts["adjacent"]
    counts = {name: int(np.sum((code == k) & ~adj)) for k, name in enumerate(vp.NAMES)}
    print(counts)
    assert set(counts) == {"lorentz", "far", "1", "2", "3", "4in", "4out"}
    assert min(counts.values()) >= 500, counts


def test_every_applicable_limit_is_straddled(pts):
    # both of a limit's branches occur among the points within two steps of it, at some y, for each pair of neighbours
    code, adj, cand, across = pts["code"], pts["adjacent"], pts["cand"], pts["across"]
    assert np.all(cand[np.arange(code.size), code]) and np.all(across[cand])
    assert np.all(across[~adj].sum(axis=1) == 1) and np.all(across[adj].sum(axis=1) >= 2)
    # only a square-root limit (XLIM0, XLIM1) leaves a choice: the fused form's may be a step off
    loose = cand.sum(axis=1) >= 2
    assert 500 <= loose.sum() < adj.sum() and np.all(cand[loose][:, [0, 1]].any(axis=1))
    pairs = set()
    for row, c in zip(across[adj], code[adj]):
        pairs |= {(int(c), int(o)) for o in np.nonzero(row)[0] if o != c}
    for a, b in ((0, 1), (1, 2), (2, 3), (2, 4), (2, 5), (3, 4), (4, 5)):
        assert (a, b) in pairs and (b, a) in pairs, (a, b)


def test_numpy_branches_are_the_oracles(oracle, pts):
    # the forced formula of the branch numpy chose is the one the oracle's own tests choose
    x, y, code = pts["x"], pts["y"], pts["code"]
    free = oracle.voigt_xy(x, y, -1)
    forced = np.zeros_like(free)
    for k in range(7):
        m = code == k
        forced[m] = oracle.voigt_xy(x[m], y[m], k)
    assert np.array_equal(free, forced)


def test_oracle_points_equal_the_reference_function(oracle, ref, pts):
    x, y, code = pts["x"], pts["y"], pts["code"]
    sqrln2 = F(0.832554611)
    alpha = np.float64(sqrln2)
    repwid = F(np.float64(sqrln2) / alpha)
    assert repwid == F(1.0)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    wres = 1.0
    assert np.array_equal(((x64 + 0 * wres - 0.0) * np.float64(repwid)).astype(F), x)      # :165
    assert np.array_equal((np.float64(repwid) * y64).astype(F), y)                          # :95
    got = oracle.voigt_xy(x, y, -1)
    want = np.array([ref.voigt(float(a), 1, wres, 0.0, float(b), float(alpha))[0] for a, b in zip(x64, y64)])
    scale = np.where(code == 6, 1.0, np.float64(vp.RSQRPI * repwid))                        # :278 (none at :103)
    assert np.all(np.isfinite(want)) and np.all(want >= 0) and np.all(want[y > 0] > 0)       # (y = 0: no Lorentz part, K = 0 beyond region 4)
    same = scale * got == want
    assert np.all(same), (int((~same).sum()), x[~same][:5], y[~same][:5])
