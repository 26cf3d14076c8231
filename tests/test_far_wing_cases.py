"""Witnesses of the window case (far_wing_cases.py), from the oracle alone: what keeps tests/test_gpu_far_wings.py from
passing emptily.  On every grid the case must have exact zeros between the clusters, wing points large enough to be judged
against their own value, wing points the layer norm cannot see, a staircase of window ends, and no wing point inside any
line's region 1."""
import numpy as np
import pytest

from far_wing_cases import E_VOIGT, E_SERIES, E_AMPLITUDE, GAP, GRIDS, PER_CLUSTER, STAIRS, WindowCase, case_name, fused_bound
from line_ladder import FLOOR, X_WING, judge_wings

FAST_TOL = 2e-6                             # the fused forms' bound of the layer norm (tests/test_gpu_moment_kernel.py)
BOTTOM = (3, 4, 5, 6)                       # the four bottom layers of the seven; the two top ones are too thin to judge


@pytest.fixture(scope="module", params=GRIDS, ids=[case_name(*g) for g in GRIDS])
def case(request, tmp_path_factory, oracle, lib):
    w0, dw = request.param
    return WindowCase(str(tmp_path_factory.mktemp("window")), oracle, lib, w0, dw)


def test_layers_and_lines(case):
    assert case.want.shape == (7, case.band.nw) and case.band.nw == int(round(85.0 / case.dw)) + 1
    assert sum(ln["v0"].size for ln in case.band.lines.values()) == 2 * PER_CLUSTER


def test_zero_gap(case):
    """Between 40 and 45 cm-1 above the first point no window reaches: exact zeros in every layer (4 points at 1 cm-1, 40
    at 0.125, a hundred at 0.05, a thousand at 0.005)."""
    gap = case.between(*GAP)
    zeros = np.sum(gap[None, :] & (case.want == 0.0) & (case.covering == 0), axis=1)
    assert np.all(zeros >= int(round(5.0 / case.dw)) - 1), zeros


def test_judged_share(case):
    """In the four bottom layers 99 % of the wing points and more are judged by E -- 6e-6 where it is smallest: Voigt,
    amplitude and series terms and a few lines' roundings -- and not by the floor."""
    assert E_VOIGT + E_AMPLITUDE + E_SERIES < 6e-6 < fused_bound(1e9, 4)
    for j in BOTTOM:
        wj = case.wing[j]
        assert wj.sum() >= 0.5 * case.band.nw, (j, wj.sum())
        share = np.mean(6e-6 * case.want[j, wj] >= FLOOR)
        assert share >= 0.99, (j, share)


def test_invisible_share(case):
    """What the case is for: on the grids finer than 1 cm-1, in layers 3 and 4, 90 % of the wing points and more lie below
    FAST_TOL of the layer's largest optical depth -- wrong by their own size, they pass the layer norm."""
    for j in (3, 4) if case.dw < 1.0 else ():     # (a 1 cm-1 grid resolves no line core: its layer maxima are wing values)
        wj = case.wing[j]
        share = np.mean(case.want[j, wj] < FAST_TOL * case.want[j].max())
        assert share >= 0.90, (j, share)


def test_staircase(case):
    """Between 35 and 40 cm-1 the first cluster's windows end one after another: covering falls from all 32 lines, never
    rises, and is zero beyond; on the grids of 0.125 cm-1 and finer it takes eight distinct values and more.  Strengths
    span a factor of ten, so one line more or less changes such a point by 1/320 of its value at the least."""
    stairs = case.between(*STAIRS)
    beyond = case.between(GAP[0] + 1.5 * case.dw, GAP[1] - 1.5 * case.dw)
    for j in range(case.want.shape[0]):
        cov = case.covering[j, stairs]
        assert cov.max() == PER_CLUSTER and np.all(np.diff(cov) <= 0), (j, cov)
        assert np.all(case.covering[j, beyond] == 0)
        if case.dw <= 0.125:
            assert cov.min() < 8 and np.unique(cov).size >= 8, (j, np.unique(cov))
        # the staircase is judged: its points above zero are wing points in the bottom layers
        if j in BOTTOM:
            assert np.any(case.wing[j, stairs] & (case.covering[j, stairs] < PER_CLUSTER))
    s0 = np.concatenate([ln["s0"] for ln in case.band.lines.values()])
    assert s0.max() / s0.min() <= 10.0


def test_a_doubled_far_field_passes_the_layer_norm_and_fails_point_by_point(case):
    """The two metrics on the oracle's own optical depths with the far field doubled -- every wing point more than 5 cm-1
    from every line centre, which is what a gather or a parent cell wrong by a factor of two would do: on the grids finer
    than 1 cm-1 the layer norm of layers 3 and 4 stays inside FAST_TOL, and the pointwise judgement fails in every layer
    that has such points."""
    v0 = np.concatenate([ln["v0"] for ln in case.band.lines.values()])
    far = case.wing & (np.min(np.abs(case.w[None, :] - v0[:, None]), axis=0) > 5.0)[None, :]
    got = np.where(far, 2.0 * case.want, case.want)
    layers, bad = judge_wings(got, case.want, case.E, case.wing, case.want == 0.0, case.name + ", far field doubled")
    assert np.all(far.sum(axis=1) > 0.3 * case.band.nw)
    assert len(bad) == case.want.shape[0] and all(e["of_bound"] > 1e3 for e in layers[2:]), bad
    if case.dw < 1.0:
        assert np.all(case.layer_norm(got)[[3, 4]] < FAST_TOL), case.layer_norm(got)
    # and the oracle against itself passes
    assert judge_wings(case.want, case.want, case.E, case.wing, case.want == 0.0, case.name)[1] == []


def test_excluded_points(case):
    """No wing point within 130 Doppler widths of ANY line in its layer: XLIM0 never exceeds 123.4 (RFM_voigt.c:109), so
    the oracle is a plain Lorentzian at every judged point; and the bound there is the issue's 1e-5 to 9e-5."""
    assert np.all(case.x_min[case.wing] >= X_WING)
    assert np.all(case.covering[case.wing] >= 1) and case.covering.max() <= 2 * PER_CLUSTER
    E = case.E[case.wing]
    assert 5.8e-6 < E.min() and E.max() < 1e-4, (E.min(), E.max())
