"""The line kernels in spectral windows, point by point (far_wing_cases.py: two clusters of 32 lines 60 cm-1 apart).

Every other parity test of the line kernels divides the error by a layer's largest optical depth or a rung's peak; the far
field of the fused forms -- cell moments, their shift to parent cells, the near-field radius, region 1 folded into the
moments, the cut at the window's edge -- is small against either by construction.  Here every point at 130 Doppler widths
and more from EVERY line (beyond every XLIM0: the oracle is a plain Lorentzian there) is judged against its own value,

    |got - want| <= E want + 2^-53,      and exactly zero where the oracle is zero,

with E = 1e-9 for the reference order and the sweep methods (against the oracle's same method) and, for the fused forms,
far_wing_cases.fused_bound: a sum of named terms from the oracle's x_min and covering, about 1e-5 far from the clusters
and 9e-5 at 130 Doppler widths.  tests/test_far_wing_cases.py holds the witnesses that the case has such points (on the
CPU); the worst cases go to far_wing_parity.json, next to parity_full_g1.json (test_gpu_parity_production.record)."""
import pytest

from grtcode_amd import api
from far_wing_cases import E_STRICT, GRIDS, WindowCase, case_name
from line_ladder import X_WING, judge_wings
from test_gpu_gas_optics import tau_close
from test_gpu_moment_kernel import FAST_TOL, check_layer_norm, fused_forms, run
from test_gpu_parity_production import record
from test_gpu_sweep_methods import LINE_SWEEP, WAVENUMBER_SWEEP
from test_gpu_sweep_methods import run as run_sweep

pytestmark = pytest.mark.gpu
FUSED = ("moment kernel", "ring kernel", "two-pass, lean loop", "two-pass, general loop")
_cases = {}


@pytest.fixture
def case_of(tmp_path_factory, oracle, lib):
    """The window case of a grid, built once for the module and left unchanged."""
    def get(w0, dw):
        if (w0, dw) not in _cases:
            _cases[w0, dw] = WindowCase(str(tmp_path_factory.mktemp("window")), oracle, lib, w0, dw)
        return _cases[w0, dw]
    return get


def judge(case, got, want, E, what, report):
    """One form on the case's wing points (and the oracle's zeros): its failures as text; its worst cases into `report`."""
    wing = (case.x_min >= X_WING) & (want != 0.0)
    layers, bad = judge_wings(got, want, E, wing, want == 0.0, f"{case.name}, {what}")
    report[what] = dict(of_bound=[e["of_bound"] for e in layers], rel=[e["rel"] for e in layers],
                        points=[e["points"] for e in layers], of_layer_max=case.layer_norm(got, want).tolist())
    return bad


def launched(case, device, fast, tile=0, nslice=0):
    """The case through one form: (optical depths, what last_launch says of the launch)."""
    V = case.col["p"].size
    go, grid = case.band.gas_optics(device, V, from_file=False)
    go.tune(tile=tile, nslice=nslice, fast=fast)
    case.band.set_column(go, case.col)
    opt = api.OpticsObject(V - 1, grid, device)
    go.calculate_optical_depth(case.col["p"], case.col["t"], opt)
    tau, info = opt.read()[0], go.last_launch()
    opt.destroy()
    go.destroy()
    # (where the one-pass form's shape does not apply -- wide windows -- fast = 1 is the ring kernel itself)
    assert info["fast"] == fast or (fast, info["fast"]) == (1, 2), info
    return tau, info


@pytest.mark.parametrize("w0,dw", GRIDS, ids=[case_name(*g) for g in GRIDS])
def test_every_form_point_by_point_in_the_window(case_of, oracle, lib, device, w0, dw):
    """Every form on one grid: 1 cm-1 at 70 cm-1 (the far-infrared series) and at 30 000 cm-1 (region 2 in the lean loop),
    0.125 cm-1 (the lean loop's finest grid), 0.05, 0.02 and 0.005 cm-1 (the cell hierarchy) and 0.002 cm-1 (the wave-shared
    tree gather: reference order and production form only, as in test_windows_bit_exact_through_production_kernels)."""
    case = case_of(w0, dw)
    band, col, report = case.band, case.col, {}
    strict = run(band, device, col, 0)
    bad = judge(case, strict, case.want, E_STRICT, "reference order", report)
    if dw > 0.002:
        for method, name in ((WAVENUMBER_SWEEP, "wavenumber sweep"), (LINE_SWEEP, "line sweep")):
            bad += judge(case, run_sweep(band, device, col, method), case.want_sweep(oracle, lib, method), E_STRICT, name, report)
        forms = fused_forms(band, device, col)
        for got, name in zip(forms, FUSED):
            bad += judge(case, got, case.want, case.E, name, report)
    lean, info = launched(case, device, 3)
    report["launch"] = {key: int(info[key]) for key in ("tile", "nslice", "tree_levels", "halo")}
    if dw <= 0.002:
        bad += judge(case, lean, case.want, case.E, FUSED[2], report)
    assert (info["tree_levels"] > 0) == (dw <= 0.05), info      # the cell hierarchy ran where the windows are wide
    record(case.name, report, file="far_wing_parity.json")
    assert not bad, "\n".join(bad)
    # the old metric stays on
    assert tau_close(strict, case.want) < 1e-11
    if dw > 0.002:
        check_layer_norm(band, device, col, case.want, forms)
    else:
        assert tau_close(lean, case.want) < FAST_TOL


@pytest.mark.parametrize("tile,nslice", [(64, 1), (256, 3)])
@pytest.mark.parametrize("w0,dw", [(1000.0, 0.125), (700.0, 0.02)], ids=["1000_0.125", "700_0.02"])
def test_launch_splits_inside_the_gap_and_the_staircases(case_of, device, w0, dw, tile, nslice):
    """Tiles of 64 and 256 points, one and three line slices: tile and halo edges fall inside the gap and the staircases,
    the slices' sums meet in global memory.  The production form and the one-pass form, same bounds."""
    case = case_of(w0, dw)
    report, bad, norms = {}, [], []
    for fast, name in ((3, FUSED[2]), (1, FUSED[0])):
        got, info = launched(case, device, fast, tile=tile, nslice=nslice)
        bad += judge(case, got, case.want, case.E, name, report)
        report[name]["launch"] = {key: int(info[key]) for key in ("fast", "tile", "nslice", "tree_levels", "halo")}
        if info["tree_levels"] == 0 and info["fast"] == fast:      # the split asked for is the split that ran
            slices = 1 if api.load_library().grt_deterministic() else nslice
            assert (info["tile"], info["nslice"]) == (tile, slices), info
        norms.append(tau_close(got, case.want))
    record(f"{case.name}_tile{tile}_nslice{nslice}", report, file="far_wing_parity.json")
    assert not bad, "\n".join(bad)
    assert max(norms) < FAST_TOL, norms
