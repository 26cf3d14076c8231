"""The band each grid point takes in grt_pipeline_run_allsky's per-point cloud maps (no GPU needed): the host's
grt_cloud_band_map against cloud_bands.band_map, the NumPy restatement of the reference's band rule that
test_clouds_band_optics.py judges against the clouds library."""
import ctypes as C

import numpy as np
import pytest

from cloud_bands import band_map, driver_limits

c_double_p = C.POINTER(C.c_double)

# what the pipeline hands over for a grid of 50 points 100, 102, .. 198 cm-1: 98, 101, 103, .. 197 (all exactly representable)
W = driver_limits(100.0, 2.0, 50)
# name -> (lo, hi, own bands, bands looped over, points)
CASES = {
    "bands inside the grid": ([98.0, 120.5, 150.2], [120.5, 150.2, 190.0], 3, 3, W),
    "limits exactly on grid values": ([101.0, 131.0, 171.0], [131.0, 171.0, 197.0], 3, 3, W),
    "first band starts above w[0]": ([110.4, 140.0], [140.0, 300.0], 2, 2, W),
    "last band ends below w[n-1]": ([10.0, 120.0], [120.0, 160.6], 2, 2, W),
    "more own bands than looped over": ([50.0, 115.0, 140.0, 170.0, 185.0], [115.0, 140.0, 170.0, 185.0, 400.0], 5, 3, W),
    "a band that covers no point": ([90.0, 111.2, 111.8], [111.2, 111.8, 250.0], 3, 3, W),
    "gap between two bands": ([100.0, 150.0], [130.0, 180.0], 2, 2, W),
    "all bands below the grid": ([1.0, 20.0], [20.0, 60.0], 2, 2, W),
    "all bands above the grid": ([500.0, 600.0], [600.0, 700.0], 2, 2, W),
    "one band": ([120.0], [160.0], 1, 1, W),
    "two points": ([0.5, 4.0], [4.0, 9.0], 2, 2, driver_limits(2.0, 5.0, 2)),
    "two points, both in the last band": ([0.0, 0.0], [0.0, 1.0e4], 2, 2, driver_limits(2.0, 5.0, 2)),
    "a grid that starts at zero": ([0.0, 3.0], [3.0, 20.0], 2, 2, driver_limits(0.0, 1.0, 12)),
}


def host_map(lib, lo, hi, own, nb, w):
    lo, hi, w = (np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi, w))
    idx = np.full(w.size, 77, dtype=np.int32)
    lib.grt_cloud_band_map.restype = None
    lib.grt_cloud_band_map(lo.ctypes.data_as(c_double_p), hi.ctypes.data_as(c_double_p), C.c_int(own), C.c_int(nb),
                           w.ctypes.data_as(c_double_p), C.c_int(w.size), idx.ctypes.data_as(C.POINTER(C.c_int)))
    return idx


@pytest.mark.parametrize("name", list(CASES))
def test_band_map_equals_the_restatement(lib, name):
    lo, hi, own, nb, w = CASES[name]
    got = host_map(lib, lo, hi, own, nb, w)
    want = band_map(lo, hi, own, nb, w)
    assert np.array_equal(got, want)
    # the named edges
    if name == "limits exactly on grid values":
        assert got[1] == 0 and w[1] == 101.0          # a lower limit on a point: the point is the band's first
        assert got[15] == 0 and got[16] == 1 and w[16] == 131.0    # an upper limit on a point: the point is the next band's
    if name == "first band starts above w[0]":
        assert np.all(got[:7] == 0)                   # band 0 reaches down to the first point
    if name == "last band ends below w[n-1]":
        assert np.all(got[-5:] == 1)                  # band own - 1 reaches up to the last point
    if name == "more own bands than looped over":
        assert got.max() == 2 and np.any(got == -1)   # the bands not looped over leave their points without one
    if name == "a band that covers no point":
        assert not np.any(got == 1)
    if name == "gap between two bands":
        assert np.any(got == -1)
    if name == "all bands below the grid":
        assert np.all(got == 1)
    if name == "all bands above the grid":
        assert got[-1] == 1 and np.all(got[:-1] == 0)


def test_band_map_on_the_driver_limits_of_the_bench_grids(lib):
    """The limits of a parametrisation with more ice than liquid bands, on grids shaped like the workload's."""
    liquid_lo = np.array([10.0, 250.0, 550.0, 780.0, 990.0, 1200.0, 1400.0])
    liquid_hi = np.append(liquid_lo[1:], 2200.0)
    ice_lo = np.linspace(10.0, 3000.0, 10)[:-1]
    ice_hi = np.linspace(10.0, 3000.0, 10)[1:]
    for w0, dw, n in ((1.0, 1.0, 3000), (1.0, 0.1, 4001), (820.0, 0.5, 700)):
        w = driver_limits(w0, dw, n)
        assert np.array_equal(host_map(lib, liquid_lo, liquid_hi, 7, 7, w), band_map(liquid_lo, liquid_hi, 7, 7, w))
        assert np.array_equal(host_map(lib, ice_lo, ice_hi, 9, 7, w), band_map(ice_lo, ice_hi, 9, 7, w))
