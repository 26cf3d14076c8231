"""The device's Voigt code point by point (grt_debug_voigt_points): every variant of voigt_class / voigt_near the line
kernels instantiate -- the class-specialised code and the packed-register region 4 of the production instance among them
-- at the 48 000 fp32 points of tests/voigt_points.py, against the oracle's per-point formulas (orc_voigt_xy, itself held
to the reference's compiled function by tests/test_oracle_voigt_points.py).  One launch per variant.

  variant 0 (reference operation order): the oracle's double, bit for bit, everywhere but in region 4's outer sums, whose
      exp(-x^2) comes from the device library instead of glibc (<= 5e-16 relative, the bound of tests/test_gpu_voigt.py);
  variants 1-4 (fused arithmetic): |K - oracle| <= 5e-6 oracle and <= 1e-6 K_oracle(0, y), the project's two bounds for
      it (tests/test_gpu_voigt.py); within 4 fp32 steps of a limit that is a square root (XLIM0, XLIM1: the fused form
      takes the hardware's, a step off at the most) against the better of the formulas on either side of that limit; next
      to the other limits (6.8 - y, 2.4 y, 18.1 y + 1.65: the same fp32 operations on the device and in numpy) against the
      reference's own branch, like anywhere else;
  variants 2-4: the class chosen is the one numpy fp32 works out from the limits, next to the limits without a root too
      (either neighbour's next to a square-root limit);
  variant 4 against 3: the same bits in classes 1 and 2 (the claim in gas_optics_dev.h that the packed form does the
      same operations in the same order per half).

Variants 2-4 are never handed a point beyond XLIM0 or a pure-Lorentz y by their callers: they are judged at the points
whose branch, or whose neighbour's across a limit, is one of regions 1-4, and what lies beyond XLIM0 within 4 steps
against region 1, which their class 0 evaluates there."""
import numpy as np
import pytest

import voigt_points as vp
from grtcode_amd import api

pytestmark = pytest.mark.gpu

REL, PEAK = 5e-6, 1e-6          # tests/test_gpu_voigt.py: pointwise, and of the line's peak
EXP_ULPS = 5e-16                # ocml's exp against glibc's, ibid.


@pytest.fixture(scope="module")
def pts(oracle):
    p = vp.build()
    x, y = p["x"], p["y"]
    p["free"] = oracle.voigt_xy(x, y, -1)
    p["forced"] = np.stack([oracle.voigt_xy(x, y, k) for k in range(7)])
    p["peak"] = oracle.voigt_xy(np.zeros_like(x), y, -1)
    assert np.array_equal(p["free"], p["forced"][p["code"], np.arange(x.size)])
    for a in p.values():
        a.setflags(write=False)
    return p


@pytest.fixture(scope="module")
def runs(device, pts):
    """(K, cls) of every variant: five launches."""
    return [api.debug_voigt_points(device, v, pts["x"], pts["y"]) for v in range(5)]


def report(tag, pts, mask, **errs):
    """The worst of each error within each branch, with its point."""
    for k, name in enumerate(vp.NAMES):
        m = np.nonzero(mask & (pts["code"] == k))[0]
        if m.size:
            worst = []
            for what, err in errs.items():
                j = m[np.argmax(err[m])]
                worst.append(f"{what} {err[j]:.3e} at ({pts['x'][j]:.9g}, {pts['y'][j]:.9g})")
            print(f"{tag}, region {name:7s} {m.size:6d} points: worst " + "; ".join(worst))


def fused_errors(K, pts, cand):
    """Per point: is it within both bounds of one of its candidate formulas, and its smaller error against them, as a
    fraction of the formula's value and of the peak."""
    with np.errstate(all="ignore"):      # (a formula forced far outside its region may overflow: never a candidate there)
        d = np.abs(K[None, :] - pts["forced"])
        rel = np.where(d == 0, 0.0, d / pts["forced"])
        peak = d / pts["peak"][None, :]
        ok = (d <= REL * pts["forced"]) & (d <= PEAK * pts["peak"][None, :]) & cand.T
        big = np.where(cand.T, np.maximum(rel / REL, peak / PEAK), np.inf)
    best = np.argmin(big, axis=0)
    cols = np.arange(K.size)
    return ok.any(axis=0), rel[best, cols], peak[best, cols]


def test_reference_order_equals_the_oracle(pts, runs):
    K, cls = runs[0]
    want, outer = pts["free"], pts["code"] == 5
    assert np.all(cls == -1)
    same = K == want
    print(f"variant 0: {int(same.sum())} of {K.size} points bit-equal; {int((~same & outer).sum())} of {int(outer.sum())} "
          "points of region 4's outer sums differ in the last bits")
    bad = ~same & ~outer
    assert not bad.any(), (int(bad.sum()), pts["x"][bad][:5], pts["y"][bad][:5], pts["code"][bad][:5])
    # (y = 0 leaves exp(-x^2) alone, subnormal at |x| = 26.8 and zero beyond 27.3: there the spacing of the subnormal
    # doubles, 2^-1074, is the least two exponentials can differ by -- added to the bound, nothing next to a normal value)
    d = np.abs(K - want)
    report("variant 0", pts, outer, relative=np.where(outer & (want > 0), d / np.where(want > 0, want, 1.0), 0.0))
    assert np.all(d[outer] <= EXP_ULPS * want[outer] + 2.0 ** -1074)


@pytest.mark.parametrize("variant", [1, 2, 3, 4])
def test_fused_arithmetic_is_within_the_project_bounds(pts, runs, variant):
    K, cls = runs[variant]
    cand, mask = pts["cand"], np.ones(K.size, dtype=bool)
    if variant >= 2:
        code, adj = pts["code"], pts["adjacent"]
        mask = (code != 6) & ~((code == 0) & ~adj)
        cand = cand.copy()
        cand[:, 1] |= cand[:, 0]          # beyond XLIM0 class 0 evaluates region 1
        cand[:, 0] = False
    assert np.all(np.isfinite(K))
    ok, rel, peak = fused_errors(K, pts, cand)
    report(f"variant {variant} away from limits", pts, mask & ~pts["adjacent"], pointwise=rel, of_peak=peak)
    report(f"variant {variant} limit-adjacent  ", pts, mask & pts["adjacent"], pointwise=rel, of_peak=peak)
    print(f"variant {variant}: worst {rel[mask].max():.3e} pointwise, {peak[mask].max():.3e} of the peak, over {int(mask.sum())} points")
    bad = mask & ~ok
    assert not bad.any(), (int(bad.sum()), pts["x"][bad][:5], pts["y"][bad][:5], pts["code"][bad][:5], rel[bad][:5], peak[bad][:5])


@pytest.mark.parametrize("variant", [2, 3, 4])
def test_class_is_the_one_the_limits_give(pts, runs, variant):
    K, cls = runs[variant]
    split = variant >= 3
    allowed = np.zeros((cls.size, 4), dtype=bool)
    for k in range(7):
        c = int(vp.classes(np.array([k]), split)[0])
        allowed[:, c] |= pts["cand"][:, k]
    assert cls.min() >= 0 and cls.max() <= (3 if split else 2)
    assert np.all(allowed[~pts["adjacent"]].sum(axis=1) == 1)
    good = allowed[np.arange(cls.size), cls]
    print(f"variant {variant}: classes {np.bincount(cls, minlength=4).tolist()}; at limit-adjacent points "
          f"{int((cls != vp.classes(pts['code'], split))[pts['adjacent']].sum())} take the neighbour's")
    assert good.all(), (int((~good).sum()), pts["x"][~good][:5], pts["y"][~good][:5], cls[~good][:5])
    assert np.all(np.bincount(cls, minlength=4)[: 4 if split else 3] >= 500)


def test_packed_region_4_gives_the_scalar_bits(pts, runs):
    (K3, c3), (K4, c4) = runs[3], runs[4]
    assert np.array_equal(c3, c4)
    m = (c3 == 1) | (c3 == 2)
    differ = m & (K3 != K4)
    worst = float(np.max(np.abs(K3[m] - K4[m]) / np.where(K3[m] != 0, np.abs(K3[m]), 1.0)))
    print(f"packed against scalar region 4: {int(differ.sum())} of {int(m.sum())} points differ, worst {worst:.3e} relative")
    assert int((c3 == 1).sum()) >= 500 and int((c3 == 2).sum()) >= 500
    assert not differ.any(), (int(differ.sum()), worst, pts["x"][differ][:5], pts["y"][differ][:5])
    assert np.array_equal(K3[~m], K4[~m])          # the other classes: the same code
