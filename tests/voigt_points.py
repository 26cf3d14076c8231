"""The (x, y) plane of the Voigt function, point by point: the point set tests/test_oracle_voigt_points.py and
tests/test_gpu_voigt_points.py share, with the reference's branch of every point worked out in numpy fp32
(RFM_voigt.c:97-126, :168-257).

Branch codes (those of orc_voigt_xy's `force`): 0 far wing (|x| >= XLIM0), 1-3 Humlicek regions 1-3, 4 / 5 region 4's
inner / outer sums, 6 pure Lorentz (y >= 70.55).

  y: 100 log-spaced values from 1e-8 to 70.5; 0; 1e-6f, 8.425f and 6.8f with their two fp32 neighbours each (the
     thresholds of :122, :111 and the sign change of XLIM2); 1.5 (Y0 of region 4); the fp32 number just below 70.55;
     and, for the pure-Lorentz branch, 70.55f, its upper neighbour, 100 and 1000.
  x, per y: 0; 280 log-spaced values from 1e-4 to XLIM0(y), every third one negated as well; every limit XLIM0-XLIM4
     that is positive, computed the reference's way and narrowed to fp32, at offsets of -2 ... +2 fp32 steps (the
     offsets -1 and +1 negated as well); 8 log-spaced values beyond XLIM0 up to 33 000, the reach of the committed
     fixture (three negated as well).  The Lorentz values of y take the log-spaced values up to 33 000 instead.

A point is LIMIT-ADJACENT when |x| lies within 4 fp32 steps of a limit that applies at its y: one with different
branches 5 steps below and 5 steps above it; `across` holds its own branch and the one across that limit.  `cand` holds
the branches a point may be judged against: its own, and the one across a limit it is adjacent to IF that limit is a
square root (XLIM0, XLIM1, and XLIM2 where y <= 1e-6 makes it XLIM0) -- the fused form takes those from the hardware
square root, one fp32 step off at the most, while 6.8 - y, 2.4 y and 18.1 y + 1.65 are the same two fp32 operations on the
device and here, so that next to them the device must take the reference's branch, to the last step."""
import numpy as np

F = np.float32
NAMES = ("far", "1", "2", "3", "4in", "4out", "lorentz")      # by branch code; the labels of test_fixture_reaches_every_region
ADJ_STEPS = 4
RSQRPI = F(0.56418958)
SEED = 20240607


def steps(x, k):
    """The fp32 number k steps above (below: k < 0) the positive fp32 x."""
    x = np.asarray(x, dtype=F)
    out = (x.view(np.int32) + np.int32(k)).view(F)
    assert np.all(x > 0) and np.all(out > 0) and np.all(np.isfinite(out))
    return out


def limits(y):
    """XLIM0 ... XLIM4 [5, n] in fp32, the reference's way: fp32 polynomials, the roots in double and narrowed."""
    y = np.asarray(y, dtype=F)
    with np.errstate(invalid="ignore"):
        x0 = np.sqrt((F(15100.0) + y * (F(40.0) - y * F(3.6))).astype(np.float64)).astype(F)
        x1 = np.where(y >= F(8.425), F(0.0), np.sqrt((F(164.0) - y * (F(4.3) + y * F(1.8))).astype(np.float64)).astype(F))
    x2 = F(6.8) - y
    x3 = F(2.4) * y
    x4 = F(18.1) * y + F(1.65)
    tiny = y <= F(0.000001)
    x1 = np.where(tiny, x0, x1)
    x2 = np.where(tiny, x0, x2)
    out = np.stack([x0, x1, x2, x3, x4]).astype(F)
    assert out.dtype == F
    return out


def branch(x, y):
    """The branch code the reference's tests choose at fp32 (x, y)."""
    x, y = np.asarray(x, dtype=F), np.asarray(y, dtype=F)
    a = np.abs(x)
    x0, x1, x2, x3, x4 = limits(y)
    return np.select([y >= F(70.55), a >= x0, a >= x1, a >= x2, a < x3, a <= x4], [6, 0, 1, 2, 3, 4], default=5).astype(np.int32)


def classes(code, split):
    """voigt_class's answer for a branch code: 0 regions 1-3 (and what lies beyond them), 1 / 2 region 4's inner / outer
    sums; split: region 3 is class 3."""
    code = np.asarray(code)
    cls = np.select([code == 4, code == 5, (code == 3) & split], [1, 2, 3], default=0)
    return cls.astype(np.int32)


def _y_values():
    ys = list(np.logspace(np.log10(1e-8), np.log10(70.5), 100).astype(F))
    ys.append(F(0.0))
    for c in (F(0.000001), F(8.425), F(6.8)):
        ys += [steps(c, -1)[()], c, steps(c, 1)[()]]
    ys.append(F(1.5))
    ys.append(steps(F(70.55), -1)[()])
    near = np.unique(np.array(ys, dtype=F))
    lorentz = np.array([F(70.55), steps(F(70.55), 1)[()], F(100.0), F(1000.0)], dtype=F)
    assert near.max() < F(70.55)
    return near, lorentz


def build():
    """The point set: dict of x, y (fp32), code (the reference's branch), adjacent (bool), across and cand (bool [n, 7]:
    the branches on either side of the limits a point is adjacent to; those it may be judged against)."""
    near, lorentz = _y_values()
    rng = np.random.default_rng(SEED)
    xs, ys = [], []
    for y in near:
        lim = limits(np.array([y], dtype=F))[:, 0]
        x0 = float(lim[0])
        # (each value moved at random within its own log step: every y meets other values of x; the ends stay)
        e = np.linspace(-4.0, np.log10(x0), 280)
        e[1:-1] += rng.uniform(-0.5, 0.5, 278) * (e[1] - e[0])
        body = (10.0 ** e).astype(F)
        beyond = np.logspace(np.log10(1.05 * x0), np.log10(33000.0), 8).astype(F)
        px = [np.array([0.0], dtype=F), body, -body[::3], beyond, -beyond[::3]]
        for L in lim:
            if L > 0:
                at = np.concatenate([steps(L, k).reshape(1) if k else np.array([L], dtype=F) for k in range(-2, 3)])
                px += [at, -at[[1, 3]]]
        px = np.concatenate(px).astype(F)
        xs.append(px)
        ys.append(np.full(px.size, y, dtype=F))
    body = np.logspace(-4.0, np.log10(33000.0), 200).astype(F)
    for y in lorentz:
        px = np.concatenate([np.array([0.0], dtype=F), body, -body[::3]]).astype(F)
        xs.append(px)
        ys.append(np.full(px.size, y, dtype=F))
    x, y = np.concatenate(xs), np.concatenate(ys)
    assert x.dtype == F and y.dtype == F
    code = branch(x, y)

    # limit-adjacent: |x| within 4 steps of a limit with different branches 5 steps to either side of it
    a = np.abs(x)
    ai = a.view(np.int32).astype(np.int64)
    lim = limits(y)
    cand = np.zeros((x.size, 7), dtype=bool)
    cand[np.arange(x.size), code] = True
    across = cand.copy()
    adjacent = np.zeros(x.size, dtype=bool)
    for which, L in enumerate(lim):
        ok = (L > 0) & (y < F(70.55))
        Ls = np.where(ok, L, F(1.0))
        below, above = branch(steps(Ls, -5), y), branch(steps(Ls, 5), y)
        hit = ok & (below != above) & (np.abs(ai - Ls.view(np.int32).astype(np.int64)) <= ADJ_STEPS)
        adjacent |= hit
        across[np.nonzero(hit)[0], below[hit]] = True
        across[np.nonzero(hit)[0], above[hit]] = True
        root = hit & ((which <= 1) | ((which == 2) & (y <= F(0.000001))))
        cand[np.nonzero(root)[0], below[root]] = True
        cand[np.nonzero(root)[0], above[root]] = True
    return {"x": x, "y": y, "code": code, "adjacent": adjacent, "across": across, "cand": cand}
