"""lw_scatter_kernel through grt_lw_scatter_levels against the float64 model (tests/lw_scatter_model.py, itself held to
mpmath by tests/test_lw_scatter_model.py): grids at the wave and workgroup edges, the shortest and an ordinary column,
one and several columns, on the model's case list -- ordinary columns; tau = 0 in a layer and in all; tau from 1e-300 to
1e5; omega in {0, 1 - 1e-9, 1}; g in {-1, 0, 1}; emis in {0, 1}.

Bounds, as fractions of the column's largest flux at the point: 1e-12 for the scattering solve's own fluxes -- what
tests/test_gpu_optics_solvers.py holds the existing solvers to --, twice that for the correction, a difference of two such
solves.  Exactly: +0.0 at every level of a point none of whose layers scatters, and in the downward correction at the top
everywhere.  Nothing is NaN or infinite.  Measured on an MI355X: worst 1.9e-15 in each of the four outputs."""
import numpy as np
import pytest

import lw_scatter_model as m
from grtcode_amd import api

pytestmark = pytest.mark.gpu

FLUX_TOL = 1e-12
DELTA_TOL = 2 * FLUX_TOL


@pytest.mark.parametrize("ncol", (1, 3))
@pytest.mark.parametrize("V", (2, 3, 16))
@pytest.mark.parametrize("nw", (1, 2, 64, 65, 128, 129, 257))
def test_kernel_against_the_model(device, nw, V, ncol):
    inp = m.kernel_inputs(ncol, V - 1, nw)
    want = m.model_on_inputs(inp)
    have = api.lw_scatter_levels(device, inp["tau"], inp["omega"], inp["g"], inp["t_layers"], inp["t_levels"],
                                 inp["t_surf"], inp["emis"], inp["w0"], inp["dw"], fluxes=True)
    scale = np.maximum(np.abs(want[2]).max(axis=1), np.abs(want[3]).max(axis=1))[:, None, :]       # [ncol][1][nw]
    assert (scale > 0).all()
    names = ("delta_up", "delta_down", "flux_up", "flux_down")
    for name, h, w_ in zip(names, have, want):
        assert h.shape == (ncol, V, nw) and np.isfinite(h).all(), name
        err = (np.abs(h - w_) / scale).max()
        print(f"{name}: worst {err:.2e} of scale")
    for name, h, w_, tol in zip(names, have, want, (DELTA_TOL, DELTA_TOL, FLUX_TOL, FLUX_TOL)):
        assert (np.abs(h - w_) <= tol * scale).all(), name
    # exactly +0.0 where nothing scatters, and in the downward correction at the top
    quiet = np.broadcast_to(inp["no_scatter"][:, None, :], have[0].shape)
    assert quiet.any() or nw < 40
    for h in have[:2]:
        assert (h[quiet] == 0.0).all() and not np.signbit(h[quiet]).any()
    assert (have[1][:, 0] == 0.0).all() and not np.signbit(have[1][:, 0]).any()
    assert (have[3][:, 0] == 0.0).all()


def test_omega_and_g_may_be_left_out(device):
    """omega NULL and g NULL are zeros: nothing scatters, and the solve is the absorption twin's"""
    inp = m.kernel_inputs(2, 4, 130)
    du, dd, fu, fd = api.lw_scatter_levels(device, inp["tau"], None, None, inp["t_layers"], inp["t_levels"], inp["t_surf"],
                                           inp["emis"], inp["w0"], inp["dw"], fluxes=True)
    zero = np.zeros_like(inp["tau"])
    eu, ed, gu, gd = api.lw_scatter_levels(device, inp["tau"], zero, zero, inp["t_layers"], inp["t_levels"], inp["t_surf"],
                                           inp["emis"], inp["w0"], inp["dw"], fluxes=True)
    for a, b in ((du, eu), (dd, ed), (fu, gu), (fd, gd)):
        assert np.array_equal(a, b)
    assert not du.any() and not dd.any()
    # without the fluxes the differences are the same doubles
    du2, dd2 = api.lw_scatter_levels(device, inp["tau"], None, None, inp["t_layers"], inp["t_levels"], inp["t_surf"],
                                     inp["emis"], inp["w0"], inp["dw"])
    assert np.array_equal(du, du2) and np.array_equal(dd, dd2)
