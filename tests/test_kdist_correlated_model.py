"""kdist_correlated_model.py against kdist_model.py and against itself, and grtcode_amd.kdist.correlated_k_of_g (no GPU
needed): with a key row the row's own reduction is grt_kdist_rows'; the counts and weight sums do not depend on the values;
perfectly correlated layers give proportional sums and k(g); the g-interval means add up; map entries that name no class
are counted nowhere.

Bounds: equality everywhere but in the sum rule of correlated_k_of_g, whose (K + G) 2^-52 of the value is the rounding of the
K-term cumulative sums and of the G differences and products that rebuild the total -- not a measured value."""
import numpy as np
import pytest

from grtcode_amd import kdist
from kdist_correlated_model import KEY_ROW, KEY_SUM, class_map, key_rows, mapped_rows
from kdist_model import kdist_row, same_bits

DW = 0.37


def log_uniform(shape, seed):
    return 10.0 ** np.random.default_rng(seed).uniform(-6.0, 2.0, shape)


def test_the_sum_key_adds_the_rows_in_order_from_plus_zero():
    x = np.array([[[1e16, -0.0], [1.0, -0.0], [-1e16, -0.0], [1.0, -0.0]]])
    key = key_rows(x, KEY_SUM)
    # ((0 + 1e16) + 1) - 1e16 + 1 = 1, not 2; and +0.0 + -0.0 ... stays +0.0
    assert key[0, 0] == 1.0 and not np.signbit(key[0, 1])
    assert same_bits(key_rows(x, KEY_ROW, 2), x[:, 2, :])


@pytest.mark.parametrize("weighted", [False, True])
def test_the_key_rows_own_reduction_is_the_plain_one(weighted):
    G, R, n, K = 2, 4, 300, 17
    x = log_uniform((G, R, n), 1)
    ce = np.logspace(-5.0, 1.0, K - 1)
    s = np.random.default_rng(2).uniform(0.0, 3.0, n) if weighted else None
    edges = [0, 40, 41, 299]
    for r in (0, R - 1):
        m = class_map(x, KEY_ROW, ce, r)
        assert m.dtype == np.uint16 and m.shape == (G, n)
        points, weight, tau = mapped_rows(x, m, DW, edges, K, s)
        for g in range(G):
            want = kdist_row(x[g, r], DW, edges, ce, s)
            assert np.array_equal(points[g], want[0])
            assert same_bits(weight[g], want[1]) and same_bits(tau[g, r], want[2])


def test_points_and_weight_do_not_depend_on_the_values():
    G, R, n, K = 2, 3, 200, 9
    x = log_uniform((G, R, n), 3)
    ce = np.logspace(-5.0, 1.0, K - 1)
    m = class_map(x, KEY_SUM, ce)
    edges = [0, 99, 199]
    a = mapped_rows(x, m, DW, edges, K)
    b = mapped_rows(log_uniform((G, R, n), 4), m, DW, edges, K)
    assert np.array_equal(a[0], b[0]) and same_bits(a[1], b[1]) and not same_bits(a[2], b[2])
    assert a[0].sum() == G * (100 + 101)


def test_perfectly_correlated_layers():
    """tau_l = c_l tau_ref with c_l a power of two: every product is exact, so the sums are c_l times the reference's bit
    for bit, and so is k(g)."""
    n, K, ref = 500, 33, 1
    c = np.array([0.25, 1.0, 8.0, 2.0 ** -20])
    base = log_uniform(n, 5)
    x = (c[:, None] * base[None, :])[None]
    ce = np.logspace(-5.0, 1.0, K - 1)
    s = np.random.default_rng(6).uniform(0.5, 2.0, n)
    edges = [0, 250, 499]
    m = class_map(x, KEY_ROW, ce, ref)
    _points, weight, tau = mapped_rows(x, m, DW, edges, K, s)
    g_edges = np.linspace(0.0, 1.0, 9)
    kg = kdist.correlated_k_of_g(weight, tau, g_edges)
    assert kg.shape == (1, c.size, 2, 8)
    for l in range(c.size):
        assert same_bits(tau[0, l], c[l] * tau[0, ref])
        assert same_bits(kg[0, l], c[l] * kg[0, ref])
    assert np.all(np.diff(kg[0, ref], axis=-1) > 0.0), "k(g) of the key layer rises with g"


def test_correlated_k_of_g():
    G, R, n, K = 2, 3, 400, 21
    x = log_uniform((G, R, n), 7)
    ce = np.logspace(-5.0, 1.0, K - 1)
    m = class_map(x, KEY_SUM, ce)
    edges = [0, 150, 399]
    _points, weight, tau = mapped_rows(x, m, DW, edges, K)
    g_edges = np.array([0.0, 0.1, 0.35, 0.6, 0.9, 1.0])
    NG = g_edges.size - 1
    kg = kdist.correlated_k_of_g(weight, tau, g_edges)
    assert kg.shape == (G, R, 2, NG)
    # equal to k_of_g row by row
    for r in range(R):
        assert same_bits(kg[:, r], kdist.k_of_g(weight, tau[:, r], g_edges))
    # the interval means, weighted with the widths, add up to the bin mean of every row
    total = (kg * np.diff(g_edges)).sum(axis=-1)
    want = tau.sum(axis=-1) / weight.sum(axis=-1)[:, None, :]
    assert np.all(np.abs(total - want) <= (K + NG) * 2.0 ** -52 * np.abs(want))
    # g-edges on the cumulative class edges of a bin give that bin's class means
    g, b = 1, 0
    w = weight[g, b]
    keep = w > 0.0
    own = np.concatenate(([0.0], kdist.cumulative(w)[keep]))
    own[-1] = 1.0
    got = kdist.correlated_k_of_g(weight[g:g + 1, b:b + 1], tau[g:g + 1, :, b:b + 1], own)
    mean = tau[g, :, b][:, keep] / w[keep]
    # (a class mean comes back as a difference of two cumulative sums over a difference of two g: each cumulative sum is
    # off by at most K roundings of the row's total, so the quotient by 2 (K + 2) 2^-52 total / width, twice that to spare
    # the interpolation's own few roundings)
    bound = 4 * (K + 2) * 2.0 ** -52 * (tau[g, :, b].sum(axis=-1) / w.sum())[:, None] / np.diff(own)[None, :]
    assert got.shape == (1, R, 1, int(keep.sum())) and np.all(np.abs(got[0, :, 0] - mean) <= bound)
    # shapes
    with pytest.raises(ValueError):
        kdist.correlated_k_of_g(weight, tau[:, 0], g_edges)
    with pytest.raises(ValueError):
        kdist.correlated_k_of_g(weight[:, :1], tau, g_edges)
    with pytest.raises(ValueError):
        kdist.correlated_k_of_g(weight[..., :-1], tau, g_edges)
    with pytest.raises(ValueError):
        kdist.correlated_k_of_g(weight[0, 0], tau[0, :, 0], g_edges)


def test_map_entries_that_name_no_class_are_counted_nowhere():
    G, R, n, K = 1, 2, 50, 5
    x = log_uniform((G, R, n), 8)
    m = class_map(x, KEY_SUM, np.logspace(-4.0, 1.0, K - 1))
    good = mapped_rows(x, m, DW, [0, 49], K)
    bad = m.copy()
    bad[0, [3, 17, 30]] = [K, K + 1, 0xffff]
    points, weight, tau = mapped_rows(x, bad, DW, [0, 49], K)
    assert points.shape == (G, 1, K) and points.sum() == n - 3 and good[0].sum() == n
    keep = np.ones(n, dtype=bool)
    keep[[3, 17, 30]] = False
    sub = mapped_rows(x[:, :, keep], m[:, keep], 1.0, [0, 46], K)
    assert np.array_equal(points, sub[0])
    assert weight.sum() < good[1].sum() and np.all(tau <= good[2])
