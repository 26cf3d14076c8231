"""The sweep kernels (k_gas_optics_sweep.hip) on the cases of tests/sweep_cases.py, against the oracle: grids of 1 to 27
bins (bin_sweep_kernel<0> clips a bin's right-hand wavenumbers at the last bin: `j + nbin >= bins.n - 1`, see
tests/test_oracle_sweep_shapes.py), line_sweep with lines up to the top of the grid, every shape of the last bin, line
counts at which first_true_wave changes shape (64, 64^2), and pressure shifts that reorder neighbours by many places
(sweep_sort_kernel's reach).

Bounds: the module-wide one of tests/test_gpu_sweep_methods.py, 1e-11 of each layer's largest optical depth, and for the
small cases a bin-by-bin one on the same terms (sweep_cases.bin_failures, where it is derived).  If one bin misses by
about 6e-8 of one line, compare that line's fp32 y = (float)(repwid gamma) from debug_line_prep and oracle.line_prep: a
two-ulp fp64 difference can flip an fp32 rounding.  Then move the line, not the bound."""
import numpy as np
import pytest

import sweep_cases as sc
from grtcode_amd import api, synthetic as syn
from test_gpu_gas_optics import tau_close
from test_gpu_sweep_methods import run

pytestmark = pytest.mark.gpu
TOL = 1e-11


def close(got, want, what):
    err = tau_close(got, want)
    print(f"{what}: {err:.2e} of the layer's largest optical depth")
    return err < TOL


@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("m,dw,extra", sc.SHORT_CASES)
def test_short_grids(tmp_path, oracle, lib, device, m, dw, extra, method):
    if sc.short_refused(m, dw, extra):
        with pytest.raises(api.GrtError):
            api.create_spectral_grid(sc.W0, sc.upper_end(sc.short_points(m, dw, extra), dw), dw)
        return
    short, long_, col = sc.short_pair(str(tmp_path), m, dw, extra)
    want = short.oracle_tau(oracle, oracle, lib, col, method=method)
    got = run(short, device, col, method)
    assert want.max() > 0.0 and close(got, want, "short grid")
    assert not sc.bin_failures(got, want, dw)
    # embedded in its partner of 40 more bins: the same lines reach the same bins (the LDS adds are unordered: not to the bit)
    got_long = run(long_, device, col, method)
    assert close(got_long, long_.oracle_tau(oracle, oracle, lib, col, method=method), "long grid")
    k = sc.embedded_points(m, dw, extra)
    assert close(got[:, :k], got_long[:, :k], "short grid in the long one")


@pytest.mark.parametrize("dw,npts", sc.TOP_CASES)
def test_line_sweep_with_lines_up_to_the_top_of_the_grid(tmp_path, oracle, lib, device, dw, npts):
    """The reference indexes bin `n` for lines within 25 cm-1 of the top; the product and the oracle skip that bin."""
    band, col = sc.top_case(str(tmp_path), dw, npts)
    sc.top_witness(oracle, lib, band, col)
    got = run(band, device, col, sc.LINE_SWEEP)
    assert close(got, band.oracle_tau(oracle, oracle, lib, col, method=sc.LINE_SWEEP), f"dw {dw}, {npts} points")


@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("ppb,last", sc.SHAPE_CASES)
def test_bin_shapes(tmp_path, oracle, lib, device, ppb, last, method):
    band, col = sc.shape_case(str(tmp_path), ppb, last, method)

    def shape(go):
        b = go.c.bins
        assert (b.ppb, b.last_ppb, b.do_interp, b.do_last_interp) == (ppb, last, int(ppb > 3), int(last > 3))
        assert b.n == 40 + (last < ppb) and b.num_wpoints == sc.shape_points(ppb, last)
    got = run(band, device, col, method, inspect=shape)
    assert close(got, band.oracle_tau(oracle, oracle, lib, col, method=method), f"ppb {ppb}, last bin of {last}")


@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("clustered", [False, True])
@pytest.mark.parametrize("n", sc.COUNT_N)
def test_line_counts(tmp_path, oracle, lib, device, n, clustered, method):
    band, col = sc.count_case(str(tmp_path), n, clustered)
    assert band.lines[syn.CO2]["v0"].size == n
    want = band.oracle_tau(oracle, oracle, lib, col, method=method)
    got = run(band, device, col, method)
    assert want.max() > 0.0 and close(got, want, f"{n} lines")
    if n <= 65:
        assert not sc.bin_failures(got, want, sc.COUNT_DW)


@pytest.mark.parametrize("method", sc.METHODS)
@pytest.mark.parametrize("spacing", sc.REORDER_SPACINGS)
def test_shifts_that_reorder_neighbours_by_many_places(tmp_path, oracle, lib, device, spacing, method):
    band, col = sc.reorder_case(str(tmp_path), spacing)
    sc.reorder_witness(oracle, lib, band, col)
    want = band.oracle_tau(oracle, oracle, lib, col, method=method)
    got = run(band, device, col, method)
    assert close(got, want, "reordered lines")
    assert not sc.bin_failures(got, want, sc.REORDER_DW)


def test_short_grid_in_the_batched_pipeline(tmp_path, oracle, lib, device):
    m, dw, extra = sc.PIPELINE_SHORT
    V = 4
    band, _, _ = sc.short_pair(str(tmp_path), m, dw, extra)
    go, grid = band.gas_optics(device, V, from_file=False, method=sc.WAVENUMBER_SWEEP)
    assert go.c.bins.n == 25
    cols = [syn.profile(c, V) for c in (4, 5)]
    pipe = api.Pipeline(go, None, len(cols), -1, np.full(band.nw, 0.98), None, None)
    gcols, keep = api.make_columns(cols, band.mols)
    pipe.run(gcols)
    pipe.fluxes(len(cols))
    tau = api.device_to_host(device, pipe.views(0)["tau_gas"], (len(cols), V - 1, band.nw))
    for c, col in enumerate(cols):
        assert close(tau[c], band.oracle_tau(oracle, oracle, lib, col, method=sc.WAVENUMBER_SWEEP), f"column {c}")
    pipe.destroy()
    go.destroy()
