"""The host staging of grt_pipeline_set_surface (no GPU needed): each grid point's entry of the surface grid and the
columns' slope and intercept entries.  The rows formed from them in NumPy, multiply then add as a kernel thread does, must
be the library's own host interpolate_to_grid(..., linear_sample, constant_extrapolation) bit for bit."""
import numpy as np
import pytest

from grtcode_amd import api
from surface_support import host_rows, same_bits, staged, thread_rows

# band grids of 2, 3 and 129 points: a longwave-like one at 1 cm-1, a shortwave-like one at 10 cm-1, and one whose first
# point and step are not representable, so that w0 + i dw rounds
BANDS = {"lw": (100.0, 1.0), "sw": (2000.0, 10.0), "fine": (100.3, 0.1)}
NS_POINTS = (2, 3, 129)


def band_grid(band, n):
    w0, dw = BANDS[band]
    g = api.create_spectral_grid(w0, w0 + (n - 1) * dw, dw)
    g.n = n                         # (ceil((wn - w0)/dw) + 1 may round one up on the fine grid: the points asked for)
    return g


def surface_grid(case, ns, g):
    """The surface grid x [ns] of a case on the band grid g."""
    lo, hi = g.w0, g.w0 + (g.n - 1) * g.dw
    span = max(hi - lo, g.dw)
    if case == "wholly below":
        return np.linspace(lo - 50.0, lo - 0.25, ns)
    if case == "wholly above":
        return np.linspace(hi + 0.25, hi + 80.0, ns)
    if case == "knot on a grid point":
        wk = g.w0 + np.float64(np.uint64(min(1, g.n - 1))) * g.dw              # the point's own double
        above = wk + np.linspace(0.0, 0.41 * span + 1.0, ns if ns == 2 else ns - 1)
        return above if ns == 2 else np.concatenate(([wk - 0.37 * span - 1.0], above))
    if case == "ends on grid points":
        return np.linspace(lo, hi, ns)                                          # w = x[0] and w = x[ns-1]
    assert case in ("across", "constant")
    return np.linspace(lo - 0.3 * span - 0.5, hi - 0.2 * span, ns) if g.n > 2 else np.linspace(lo - 0.5, lo + 0.5 * g.dw, ns)


CASES = ("across", "wholly below", "wholly above", "knot on a grid point", "ends on grid points", "constant")


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("ns", [2, 5])
@pytest.mark.parametrize("n", NS_POINTS)
@pytest.mark.parametrize("band", list(BANDS))
def test_staged_rows_are_the_host_interpolation(lib, band, n, ns, case):
    g = band_grid(band, n)
    x = surface_grid(case, ns, g)
    assert np.all(np.diff(x) > 0)
    ncol = 3
    rng = np.random.default_rng(1000 * n + 10 * ns + len(case))
    values = rng.uniform(0.0, 1.0, (ncol, ns))
    values[0, 0], values[1, -1], values[2, ns - 2] = 0.0, 1.0, 1.0
    if case == "constant":
        values[:] = np.array([0.0, 1.0, 0.6180339887498949])[:, None]
    assert case == "constant" or np.all(values[:, ns - 2] != values[:, ns - 1])
    want = host_rows(lib, g, x, values)
    entry, tables = staged(lib, g, x, values)
    assert entry.min() >= 0 and entry.max() <= ns
    got = thread_rows(g, entry, tables)
    assert same_bits(got, want), np.max(np.abs(got - want))
    # the tables themselves: the two constant ranges, and linear_sample's two expressions per interval
    assert np.all(tables[:, 0, 0] == 0.0) and same_bits(tables[:, 0, 1], values[:, 0])
    assert np.all(tables[:, ns, 0] == 0.0) and same_bits(tables[:, ns, 1], values[:, ns - 2])
    m = (values[:, 1:] - values[:, :-1]) / (x[1:] - x[:-1])
    assert same_bits(tables[:, 1:ns, 0], m) and same_bits(tables[:, 1:ns, 1], values[:, :-1] - m * x[:-1])
    # the named edges
    w = g.w0 + np.arange(n, dtype=np.uint64).astype(np.float64) * g.dw
    if case == "wholly below":
        assert np.all(entry == ns) and same_bits(want, np.repeat(values[:, ns - 2: ns - 1], n, axis=1))
    if case == "wholly above":
        assert np.all(entry == 0) and same_bits(want, np.repeat(values[:, :1], n, axis=1))
    if case == "knot on a grid point":
        k, j = min(1, n - 1), (1 if ns > 2 else 0)
        assert w[k] == x[j] and entry[k] == j                  # w = x[j]: interval j - 1 (entry j), or y[0] for j = 0
    if case == "ends on grid points":
        assert entry[0] == 0 and entry[-1] == ns - 1           # w = x[0]: y[0]; w = x[ns-1]: the last interval
    if case == "constant":
        assert np.all(tables[:, :, 0] == 0.0) and same_bits(got, np.repeat(values[:, :1], n, axis=1))


def test_entry_map_follows_the_three_rules(lib):
    """x[j] < w <= x[j+1] on a grid whose points are all exactly representable."""
    g = api.create_spectral_grid(100.0, 198.0, 2.0)
    x = np.array([95.0, 120.0, 121.0, 160.0, 180.0])
    entry, _ = staged(lib, g, x, np.zeros((1, x.size)))
    w = 100.0 + 2.0 * np.arange(g.n)
    want = np.array([0 if v <= x[0] else (x.size if v > x[-1] else 1 + int(np.searchsorted(x, v, side="left")) - 1)
                     for v in w], dtype=np.int32)
    assert np.array_equal(entry, want)
    assert entry[10] == 1 and entry[11] == 3 and entry[30] == 3 and entry[40] == 4 and entry[41] == 5
