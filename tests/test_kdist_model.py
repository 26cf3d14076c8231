"""kdist_model.py's restatement of the k-distribution reduction, and grtcode_amd.kdist, against what pins them down, on the
CPU: an independent loop in plain Python reproduces the model bit for bit; over contiguous bins the sums over the classes are
the trapezoid integrals of the weight and of weight x tau; and on a ramp, whose k(g) is the ramp itself, cumulative and
k_of_g return it to within one class.  That is what keeps test_gpu_kdist.py from judging the kernel against a wrong
reference."""
import math

import numpy as np

from grtcode_amd import kdist
from kdist_model import kdist_row, same_bits
from pipeline_support import exact_trapezoid


def loop_row(tau, dw, edges, class_edges, weight):
    """the definition of grt_ext.h, point by point in Python floats"""
    K, nb = len(class_edges) + 1, len(edges) - 1
    points = [[0] * K for _ in range(nb)]
    wsum = [[0.0] * K for _ in range(nb)]
    tsum = [[0.0] * K for _ in range(nb)]
    for b in range(nb):
        for i in range(edges[b], edges[b + 1] + 1):
            w = 0.5 * dw if i in (edges[b], edges[b + 1]) else dw
            W = w if weight is None else w * float(weight[i])
            T = W * float(tau[i])
            k = sum(1 for e in class_edges if float(e) <= float(tau[i]))
            points[b][k] += 1
            wsum[b][k] = wsum[b][k] + W
            tsum[b][k] = tsum[b][k] + T
    return np.array(points, dtype=np.int32), np.array(wsum), np.array(tsum)


def test_the_model_is_the_definition_bit_for_bit():
    rng = np.random.default_rng(11)
    n = 97
    tau = 10.0 ** rng.uniform(-5.0, 3.0, n)
    tau[[3, 40]] = [0.0, -1.0]
    s = rng.uniform(0.0, 2.0, n)
    s[[7, 8, 60]] = 0.0
    class_edges = np.logspace(-4.0, 2.0, 13)
    tau[[20, 21]] = class_edges[[0, 5]]                # on an edge: the upper class
    edges = [0, 1, 30, 31, 96]
    for weight in (None, s):
        got = kdist_row(tau, 0.3, edges, class_edges, weight)
        want = loop_row(tau, 0.3, edges, class_edges, weight)
        assert np.array_equal(got[0], want[0])
        assert same_bits(got[1], want[1]) and same_bits(got[2], want[2])
        assert got[0].sum(axis=1).tolist() == [2, 30, 2, 66]
    # +0.0 in an empty class, and in a class whose terms are all -0.0 (the sum starts from +0.0)
    p, w, t = kdist_row(np.array([-1.0, -2.0, -3.0]), 1.0, [0, 2], [1.0], np.zeros(3))
    assert p.tolist() == [[3, 0]]
    assert same_bits(w, np.zeros((1, 2))) and same_bits(t, np.zeros((1, 2)))


def test_the_classes_add_up_to_the_trapezoid():
    """The sums over the classes against exact_trapezoid, to (m + 2) 2^-53 relative, m the bin's points: a sum of m
    non-negative terms of two roundings each.  (dw is a power of two here, so that the terms s_i tau_i the exact trapezoid
    is given are the device's T_i but for that factor: the bound then covers the comparison rigorously.)"""
    rng = np.random.default_rng(5)
    n, dw = 700, 0.5
    tau = 10.0 ** rng.uniform(-6.0, 2.0, n)
    s = rng.uniform(0.0, 3.0, n)
    s[rng.integers(0, n, 40)] = 0.0
    class_edges = np.logspace(-5.0, 1.0, 31)
    edges = [0, 1, 128, 129, 400, 699]
    for weight in (None, s):
        sw = np.ones(n) if weight is None else weight
        _points, w, t = kdist_row(tau, dw, edges, class_edges, weight)
        for b in range(len(edges) - 1):
            lo, hi = edges[b], edges[b + 1]
            m = hi - lo + 1
            for got, f in ((w[b], sw[lo:hi + 1]), (t[b], (sw * tau)[lo:hi + 1])):
                ref, _mag = exact_trapezoid(f, dw)
                assert abs(math.fsum(got) - ref) <= (m + 2) * 2.0 ** -53 * ref, (b, math.fsum(got), ref)
        # contiguous bins: the bins add up to the bin over their union
        _p1, w1, t1 = kdist_row(tau, dw, [0, n - 1], class_edges, weight)
        for part, whole in ((w, w1), (t, t1)):
            a, c = math.fsum(part.ravel()), math.fsum(whole.ravel())
            assert abs(a - c) <= (n + 2) * 2.0 ** -52 * c


def test_cumulative_and_k_of_g_on_a_ramp():
    """tau rises linearly with the grid index: g(tau) is linear, so k(g) is the ramp itself.  Both functions against that
    closed form, to within one class width (a class's points count as its mean)."""
    n, dw = 2001, 1.0
    tau = np.linspace(1.0, 3.0, n)
    K = 41
    class_edges = np.linspace(1.0, 3.0, K + 1)[1:-1]
    width = 2.0 / K
    _points, w, t = kdist_row(tau, dw, [0, n - 1], class_edges)
    g = kdist.cumulative(w)[0]
    assert g[-1] == 1.0 and np.all(np.diff(g) > 0.0)
    upper = np.concatenate((class_edges, [3.0]))                    # the upper edge of every class
    assert np.max(np.abs(g - (upper - 1.0) / 2.0)) <= width / 2.0   # g = (tau - 1)/2 on the ramp: one class is width/2 of g
    g_edges = np.linspace(0.0, 1.0, 17)
    k = kdist.k_of_g(w, t, g_edges)[0]
    mid = 1.0 + 2.0 * 0.5 * (g_edges[1:] + g_edges[:-1])            # the ramp's mean over each g-interval
    assert k.shape == (16,)
    assert np.max(np.abs(k - mid)) <= width
    # the intervals' means, weighted with their widths, are the bin's mean
    assert abs(np.sum(k * np.diff(g_edges)) - t.sum() / w.sum()) <= 1e-12
    # leading axes are kept, and a g-edge inside a class splits it in proportion: one class, two halves of the same mean
    k2 = kdist.k_of_g(np.array([[[2.0]], [[4.0]]]), np.array([[[6.0]], [[4.0]]]), [0.0, 0.5, 1.0])
    assert k2.shape == (2, 1, 2) and k2[:, 0].tolist() == [[3.0, 3.0], [1.0, 1.0]]
