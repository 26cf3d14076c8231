"""grt_slant_cosines and geometry.level_heights (no GPU needed): the layer cosines of the straight ray that reaches the
column's lowest level.  An overhead sun gives 1.0 in every layer; a flat planet copies mu0 bit for bit; on a sphere the
slant path through all layers, sum_j dz_j/mu_j, is the chord from the top level to the lowest one; the cosines grow with
height; every refusal; the hypsometric heights against their formula."""
import ctypes as C

import numpy as np
import pytest

from grtcode_amd import api, geometry

RADIUS = 6.371e6
MUS = (1.0, 0.5, 0.05, 1e-3, 0.0)
LEVELS = (2, 3, 16, 60)
# each term dz/mu of the path carries about six roundings (two squares, two differences, two roots, the sum a + b, rt + rb,
# the quotient: ~6 x 1.1e-16 relative) and at most 59 positive terms are added (another 59 x 1.1e-16 at the very worst):
# below 1e-14 together, two orders under the bound
CHORD_TOL = 1e-12


def heights(V, ncol=2, top=80e3, seed=3):
    """[ncol][V] m, top first, strictly descending: uneven layers, the second column's surface 1500 m up."""
    rng = np.random.default_rng(seed + V)
    out = np.empty((ncol, V))
    for c in range(ncol):
        cuts = np.sort(rng.uniform(0.0, 1.0, V - 2)) if V > 2 else np.empty(0)
        frac = np.concatenate([[1.0], cuts[::-1], [0.0]])
        out[c] = 1500.0 * c + frac * (top - 1500.0 * c)
    assert np.all(np.diff(out, axis=1) < 0.0)
    return out


def test_overhead_sun_gives_one_in_every_layer():
    for V in LEVELS:
        h = heights(V)
        got = geometry.slant_cosines(RADIUS, h, np.ones((2, 3)))
        assert got.shape == (2, 3, V - 1) and np.all(got == 1.0)


def test_flat_planet_copies_mu0_bit_for_bit():
    mu = np.array([[1.0, 0.5, 0.05, 1e-3, 0.0, 0.3333333333333333], [0.999, 1e-300, 0.7, 0.2, 5e-324, 1.0]])
    for V in LEVELS:
        got = geometry.slant_cosines(0.0, heights(V), mu)
        want = np.repeat(mu[:, :, None], V - 1, axis=2)
        assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("V", LEVELS)
def test_the_slant_path_is_the_chord(V):
    h = heights(V)
    mu = np.array([MUS, MUS[::-1]])
    got = geometry.slant_cosines(RADIUS, h, mu)
    assert np.all(np.isfinite(got)) and np.all(got > 0.0) and np.all(got <= 1.0)
    dz = -np.diff(h, axis=1)
    for c in range(2):
        r0, rtop = RADIUS + h[c, -1], RADIUS + h[c, 0]
        for k, mu0 in enumerate(mu[c]):
            path = float(np.sum(dz[c] / got[c, k]))
            s2 = r0 * r0 * (1.0 - mu0 * mu0)
            chord = float(np.sqrt(rtop * rtop - s2) - r0 * mu0)
            err = abs(path - chord) / chord
            print("V", V, "column", c, "mu0", mu0, "air mass", path / dz[c].sum(), "relative error", err)
            assert err <= CHORD_TOL, (V, c, mu0, err)
            # (at the horizon a spherical planet's air mass is tens, not 1/mu0)
            if mu0 <= 1e-3:
                assert path / dz[c].sum() < 60.0


@pytest.mark.parametrize("V", LEVELS[1:])
def test_cosines_grow_with_height(V):
    mu = np.array([[0.5, 0.05, 1e-3, 0.0, 0.999]] * 2)
    got = geometry.slant_cosines(RADIUS, heights(V), mu)
    # (top layer first: every layer's cosine is above that of the layer below it, and all are above mu0)
    assert np.all(np.diff(got, axis=2) < 0.0)
    assert np.all(got > mu[:, :, None])


def test_an_angle_below_the_horizon_gets_zeros():
    got = geometry.slant_cosines(RADIUS, heights(3), np.array([[-0.2, 0.5], [1.0, -1.0]]))
    assert np.all(got[0, 0] == 0.0) and np.all(got[1, 1] == 0.0) and np.all(got[0, 1] > 0.5) and np.all(got[1, 0] == 1.0)


def test_refusals(lib):
    h, mu = heights(3), np.array([[0.5, 0.1], [1.0, 0.3]])
    out = np.full((2, 2, 2), -7.25)
    p = api.c_double_p

    def call(radius=RADIUS, ncol=2, V=3, Z=2, hh=h, mm=mu, oo=out):
        return lib.grt_slant_cosines(C.c_double(radius), ncol, V, Z, None if hh is None else hh.ctypes.data_as(p),
                                     None if mm is None else mm.ctypes.data_as(p), None if oo is None else oo.ctypes.data_as(p))

    assert call() == 0 and np.all(out > 0.0)
    out[:] = -7.25
    bad_h = [h.copy() for _ in range(4)]
    bad_h[0][0, 1] = bad_h[0][0, 0]                  # not strictly descending: equal
    bad_h[1][1] = bad_h[1][1, ::-1]                  # ascending
    bad_h[2][1, 2] = np.nan
    bad_h[3][0, 0] = np.inf
    bad_mu = [mu.copy() for _ in range(3)]
    bad_mu[0][0, 1] = 1.0 + 1e-12
    bad_mu[1][1, 0] = -1.0 - 1e-12
    bad_mu[2][1, 1] = np.nan
    cases = [dict(radius=-1.0), dict(radius=-1e-300), dict(radius=np.inf), dict(radius=np.nan), dict(hh=None), dict(mm=None),
             dict(oo=None), dict(ncol=0), dict(V=1), dict(Z=0)]
    cases += [dict(hh=b) for b in bad_h] + [dict(mm=b) for b in bad_mu]
    for kw in cases:
        with pytest.raises(api.GrtError) as e:
            api.check(call(**kw))
        # (a NULL pointer is the library's GRTCODE_NULL_ERR, as at every entry point)
        null = any(k in kw and kw[k] is None for k in ("hh", "mm", "oo"))
        assert e.value.code == (api.NULL_ERR if null else api.VALUE_ERR), kw
        assert np.all(out == -7.25), kw
    with pytest.raises(api.GrtError):
        geometry.slant_cosines(-1.0, h, mu)
    with pytest.raises(ValueError):
        geometry.slant_cosines(RADIUS, h[0], mu)


def test_level_heights_against_the_formula():
    p = np.array([[0.1, 10.0, 300.0, 1000.0], [0.2, 20.0, 250.0, 850.0]])
    t = np.array([[230.0, 215.0, 270.0], [240.0, 220.0, 280.0]])
    z = geometry.level_heights(p, t, surface_height=np.array([[0.0], [1500.0]]))
    assert z.shape == p.shape and np.all(np.diff(z, axis=1) < 0.0)
    assert np.array_equal(z[:, -1], [0.0, 1500.0])
    for c in range(2):
        for j in range(3):
            dz = geometry.RD * t[c, j] / geometry.G0 * np.log(p[c, j + 1] / p[c, j])
            assert abs((z[c, j] - z[c, j + 1]) - dz) <= 1e-12 * z[c, 0]
    assert (geometry.RD, geometry.G0) == (287.05, 9.80665)
    one = geometry.level_heights(p[0], t[0])
    assert one.shape == (4,) and np.array_equal(one, geometry.level_heights(p, t)[0])
    for bad in (0.0, -1.0, np.nan):
        q = p.copy()
        q[1, 2] = bad
        with pytest.raises(ValueError):
            geometry.level_heights(q, t)
