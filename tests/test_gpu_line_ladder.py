"""The line kernels over HITRAN's parameter ranges, line by line (line_ladder.py: one isolated line per rung, judged against
its own peak).  The other parity modules draw every line from synthetic.line_list (strengths 1e-27 .. 1e-20, ordinary
widths, energies below 4000 cm-1, shifts within 0.02 cm-1/atm) and compare over each layer's LARGEST optical depth, which
one strong line sets; here the parameters go where a real HITRAN file goes, and a weak line wrong by its own size fails.

Every ladder runs every form against the oracle, rung by rung:
    reference order (fast = 0), wavenumber sweep, line sweep                  1e-11 of the rung's peak
    moment kernel (1), ring kernel (2), two-pass lean (3), two-pass general (3, GRT_LEAN=0)   FAST_TOL (2e-6)
    lean loop against general loop    LEAN_TOL;       moment kernel against ring kernel    BETWEEN_TOL
each plus the floor 2^-53, and the layer-norm assertions of test_gpu_moment_kernel.py as well.  A rung's points at 130 Doppler
widths and more from its shifted centre are also judged one by one against their OWN value (Ladder.wing_failures: 1e-9 for the
first row, far_wing_cases.fused_bound with one covering line for the second), and every ladder states, from the oracle, the
least share of those points that lie above the floor (min_judged: the thin top layers of an ordinary line do not).  The columns run from 1e-6 mb
and 150 K at the top to 3 atm and 340 K at the bottom.  The ladders (line_ladder.LADDERS): 1 cm-1 from 70 cm-1 (the first
rungs lie below 0.7 T: the series for 1 - e^x of the lean loop, kTfFarir), 0.05 cm-1 from 700 cm-1 (the cell hierarchy),
1 cm-1 from 30 000 cm-1 (a grid step is tens of Doppler widths: the lean loop evaluates Humlicek region 2 itself), and
0.125 cm-1 from 1000 cm-1 (the finest grid whose first pass is the lean loop: shifts of more than a grid step there).

The witnesses -- that a ladder really has rungs on both sides of a branch -- come from the oracle and the parity hooks
(debug_line_strengths), never from a kernel's output."""
import numpy as np
import pytest

from far_wing_cases import E_STRICT, fused_bound
from line_ladder import (LADDERS, SPACING, X_WING, Ladder, bare_band, column, complete, judged_share, layer_means, lines_of,
                         mark, rung)
from test_gpu_moment_kernel import BETWEEN_TOL, FAST_TOL, LEAN_TOL, check_layer_norm, fused_forms, run
from test_gpu_sweep_methods import LINE_SWEEP, WAVENUMBER_SWEEP
from test_gpu_sweep_methods import run as run_sweep

pytestmark = pytest.mark.gpu
STRICT_TOL = 1e-11
KINDS = list(LADDERS)
# the loader's range test on the strength scaled by 2^96 (grt_line_store.c, pack_lean): 2^-100 <= s 2^96 <= 2^100
LEAN_S_MIN, LEAN_S_MAX = 2.0 ** -196, 2.0 ** 4


def wing_points(lad, oracle, lib, col, want, min_judged):
    """The ladder's wing points from the oracle (Ladder.locate); at least `min_judged` of them are large enough for the
    fused forms' E to judge them above the floor -- the witness that the pointwise judgement is not empty.  The shares the
    oracle gives, the same to two digits on all four grids (the thin top layers put an ordinary line's wings below 2^-53
    whatever the ladder; the bottom layers are judged to 0.55 - 1.00): strengths 0.21 (six of its twelve rungs are weaker
    than anything can judge; 1e-30 to 1e-16 and the pair at the top of the lean range are judged), energies 0.32 - 0.33,
    widths 0.45 (not the pure Doppler rungs: exact zeros there), centres 0.44, shifts 0.40 - 0.46, file 0.43."""
    x = lad.locate(oracle, lib, col)
    wing = (x >= X_WING) & (want != 0.0)
    share = judged_share(want, wing, fused_bound(x, 1.0)[wing])
    print(f"wing points: {int(wing.sum())}, {share:.3f} of them judged above the floor (at least {min_judged})")
    assert share >= min_judged, (share, min_judged)


def check_ladder(lad, device, oracle, lib, col, min_judged, from_file=False):
    """Every form on the ladder, rung by rung and on the rungs' far wings point by point; then the layer norm."""
    band = lad.band
    want = band.oracle_tau(oracle, oracle, lib, col)
    assert np.all(np.isfinite(want))
    wing_points(lad, oracle, lib, col, want, min_judged)
    strict = run(band, device, col, 0, from_file=from_file)
    bad = lad.rung_failures(strict, want, STRICT_TOL, "reference order")
    bad += lad.wing_failures(strict, want, E_STRICT, "reference order")
    for method, name in ((WAVENUMBER_SWEEP, "wavenumber sweep"), (LINE_SWEEP, "line sweep")):
        want_sweep = band.oracle_tau(oracle, oracle, lib, col, method=method)
        got = run_sweep(band, device, col, method, from_file=from_file)
        bad += lad.rung_failures(got, want_sweep, STRICT_TOL, name)
        bad += lad.wing_failures(got, want_sweep, E_STRICT, name)
    forms = fused_forms(band, device, col, from_file=from_file)
    mp, ring, lean, two = forms
    for got, name in ((mp, "moment kernel"), (ring, "ring kernel"), (lean, "two-pass, lean loop"),
                      (two, "two-pass, general loop")):
        bad += lad.rung_failures(got, want, FAST_TOL, name)
        bad += lad.wing_failures(got, want, fused_bound, name)
    bad += lad.rung_failures(lean, two, LEAN_TOL, "lean loop against general loop", peak_of=want)
    bad += lad.rung_failures(mp, ring, BETWEEN_TOL, "moment kernel against ring kernel", peak_of=want)
    assert not bad, "\n".join(bad)
    check_layer_norm(band, device, col, want, forms, from_file=from_file)


def rescale_factor(oracle, lib, r):
    """What the loader multiplies rung r's tabulated strength by (parse_HITRAN_file.c:372-384), from the oracle."""
    q296 = np.array([lib.Q(r["mol"], 296.0, r["iso"])])
    return oracle.rescale_strengths(np.ones(1), np.array([r["en"]]), np.array([r["v0"]]), q296)[0]


@pytest.mark.parametrize("kind", KINDS)
def test_strengths_from_1e_45_to_1e_16_and_across_the_lean_range(tmp_path, oracle, lib, device, kind):
    """Branch: the loader's range test on the rescaled strength (pack_lean: inside, the lean loop takes the line with its
    strength as an fp32 number scaled by 2^96; outside -- zero included -- the line is flagged and general_block takes it),
    and the fp32 amplitude of the lean loop (mantissa/exponent pairs put together by ldexpf), which may underflow.  Raw
    strengths over HITRAN's range, exact zero, and a pair of rungs 0.4 % to either side of each end of the range -- the
    upper pair by way of a lower-state energy of 8000 cm-1, as a real list would get there."""
    rungs = [rung(f"s0 {s:g}", s0=s) for s in (1e-45, 1e-40, 1e-35, 1e-30, 1e-25, 1e-20, 1e-16, 0.0)]
    ends = [(LEAN_S_MIN * (1.0 - 2.0 ** -8), 0.0), (LEAN_S_MIN * (1.0 + 2.0 ** -8), 0.0),
            (LEAN_S_MAX * (1.0 - 2.0 ** -8), 8000.0), (LEAN_S_MAX * (1.0 + 2.0 ** -8), 8000.0)]
    rungs += [rung(f"rescaled {s:.4g}", en=en) for s, en in ends]
    lad = Ladder(str(tmp_path), kind, rungs)
    assert lad.K % 2 == 0                                   # (an even store: no padding line in the lean records)
    for r, (s, _) in zip(lad.rungs[8:], ends):
        r["s0"] = s / rescale_factor(oracle, lib, r)
    lad.set_lines()
    col = column(8)
    # witness: the device store's rescaled strengths, in the merged store's order -- the rungs'
    go, _ = lad.band.gas_optics(device, col["p"].size, from_file=False)
    s = go.debug_line_strengths()
    go.destroy()
    assert s.size == lad.K and np.allclose(s[8:], [e[0] for e in ends], rtol=1e-12, atol=0.0), s
    near = lambda x, end: abs(x / end - 1.0) < 0.01
    assert any(x < LEAN_S_MIN and near(x, LEAN_S_MIN) for x in s) and any(x >= LEAN_S_MIN and near(x, LEAN_S_MIN) for x in s)
    assert any(x <= LEAN_S_MAX and near(x, LEAN_S_MAX) for x in s) and any(x > LEAN_S_MAX and near(x, LEAN_S_MAX) for x in s)
    assert s[7] == 0.0 and np.all((s[:7] > LEAN_S_MIN) & (s[:7] < LEAN_S_MAX))
    check_ladder(lad, device, oracle, lib, col, 0.18)


@pytest.mark.parametrize("kind", KINDS)
def test_lower_state_energies_from_unknown_to_20000(tmp_path, oracle, lib, device, kind):
    """Branch: e^(c2 E/T) in the lean loop -- the exponent split off exactly and applied with ldexpf, where the fp32
    amplitude can underflow in the cold top layer (150 K) and is largest in the warm bottom one (340 K) -- and, through
    the rescaling by e^(-c2 E/296), the loader's range test from the high side (E = 20 000 multiplies a strength by
    e^97).  E = -1 is HITRAN's "unknown".  Each energy with a strong and a weak line."""
    rungs = [rung(f"E {en:g} s0 {s:g}", en=en, s0=s) for en in (-1.0, 0.0, 4000.0, 10000.0, 15000.0, 20000.0)
             for s in (1e-19, 1e-27)] + [rung("ordinary")]
    lad = Ladder(str(tmp_path), kind, rungs)
    assert lad.K % 2 == 1                                   # (an odd store: the lean records end in a line of padding)
    check_ladder(lad, device, oracle, lib, column(9), 0.29)


WIDTHS = [("self width 0", 0.07, 0.0), ("air width 0", 0.0, 0.3), ("pure Doppler", 0.0, 0.0), ("air width .0001", 0.0001, 0.35),
          ("air 1.0 self 2.0", 1.0, 2.0), ("ordinary widths", 0.07, 0.35)]


@pytest.mark.parametrize("kind", KINDS)
def test_widths_from_none_to_broad_on_and_off_grid_points(tmp_path, oracle, lib, device, kind):
    """Branch: the hand-over of lines with y <= 1e-6 to the general loop inside a wave (exc, xl_mask in lean_block;
    RFM_voigt.c:122-126 for y = 0) -- by a width of zero, and by the thin top layers with ordinary widths --, y >= 8.425
    and >= 70.55 (no near-centre points, no region 1) under 3 atm with widths of 1 and 2 cm-1/atm.  Centres exactly on
    grid points (x = 0), half a step off (the halfway mark: guard) and 0.3 of a step off, without shift."""
    rungs = [rung(f"{name}, {off} of a step off", yair=ya, yself=ys, off=off, delta=0.0)
             for off in (0.0, 0.5, 0.3) for name, ya, ys in WIDTHS]
    rungs.append(rung("pure Doppler, strong, on a grid point", yair=0.0, yself=0.0, off=0.0, delta=0.0, s0=1e-18))
    lad = Ladder(str(tmp_path), kind, rungs)
    col = column(8)
    # witness: y = sqrt(ln 2) gamma/alpha from the oracle's line preparation -- zero, below 1e-6 with a width that is not
    # zero (at 100 cm-1, where Doppler widths are smallest, that takes the air width of .0001), above it, and broad
    _, gamma, alpha = lad.prepared(oracle, lib, col)
    y = np.sqrt(np.log(2.0)) * gamma / alpha
    assert np.any(y == 0.0) and np.any((y > 0.0) & (y <= 1e-6)) and np.any((y > 1e-6) & (y < 1.0)), y
    assert np.any((y >= 8.425) & (y < 70.55)), y.max()
    assert kind == "ultraviolet" or np.any(y >= 70.55), y.max()         # (Doppler widths of 0.04 cm-1 there: y up to 41)
    if kind != "far_infrared":      # the thin top layers do it with ordinary widths
        ordinary = [k for k, r in enumerate(lad.rungs) if r["yair"] > 0.05 and 0.3 < r["yself"] < 0.4]
        assert len(ordinary) == 3 and np.any(y[:, ordinary] <= 1e-6) and np.any(y[:, ordinary] > 1e-6), y[:, ordinary]
    check_ladder(lad, device, oracle, lib, col, 0.40)


@pytest.mark.parametrize("kind", KINDS)
def test_centres_on_inside_and_outside_the_guard_band(tmp_path, oracle, lib, device, kind):
    """Branch: the hand-over of lines whose SHIFTED centre comes within 1e-5 of a grid step of the halfway mark between two
    grid points (guard in lean_block: there the fp32 sum of offset and shift cannot decide kernels.c:431-432's floor).
    In one chosen layer the shifted centre sits on the mark, 3e-6 of a step to either side (inside the band) and 1e-4
    (outside): without shift (every layer), with delta = 0.02 for the bottom layer and -0.015 for a middle one.  Wide
    lines (0.1 and 0.5 cm-1/atm): in the bottom layers a window one point off shows at its edge, where a Lorentzian of
    half-width 0.3 is still 1e-4 of its peak."""
    col = column(9)
    L = col["p"].size - 1
    _, pavg, _ = layer_means(oracle, col)
    eps = np.array([0.0, 3e-6, -3e-6, 1e-4, -1e-4])
    w0, dw, _ = LADDERS[kind]
    groups = [(0.0, 0), (0.02, L - 1), (-0.015, L // 2)]
    rungs = []
    for delta, j in groups:
        d32 = float(np.float32(delta))
        for e in eps:
            k = len(rungs)
            rungs.append(rung(f"delta {delta}, {e:g} of a step from the mark in layer {j}", yair=0.1, yself=0.5, delta=delta,
                              v0=mark(kind, k, 0.5) - d32 * pavg[j] + e * dw))
    lad = Ladder(str(tmp_path), kind, rungs)
    assert lad.K % 2 == 1
    # witness: the oracle's shifted centres (bit-exact on the device: test_line_prep_and_windows_bit_exact), in grid steps
    vnn, _, _ = lad.prepared(oracle, lib, col)
    u = (vnn - w0) / dw
    from_mark = u - np.floor(u) - 0.5
    for g, (delta, j) in enumerate(groups):
        d = from_mark[j, 5 * g:5 * g + 5]
        assert np.allclose(d, eps, rtol=0.0, atol=1e-8), (delta, j, d)      # on, inside (1e-5) and outside, either side
    check_ladder(lad, device, oracle, lib, col, 0.40)


@pytest.mark.parametrize("kind", KINDS)
def test_shifts_of_a_tenth_per_atmosphere(tmp_path, oracle, lib, device, kind):
    """Branch: kf in lean_block -- the shifted centre's grid point is the unshifted one's plus floor(offset + shift + 1/2),
    more than one step away -- and kernels.c:433, a centre carried off the grid.  delta = +-0.1:
      * on the 0.05 cm-1 ladder the centre moves several grid steps in the bottom layers and a fraction of one in the top
        ones, and the first rung's centre leaves the grid in the bottom layer only (a loader keeps no line below the grid's
        first point, and 0.1 cm-1/atm does not carry one over half a step of 1 cm-1: on the other ladders that rung stays on
        the grid, its window clipped).  Windows of 500 points a side go through the cell hierarchy, whose first pass is
        the general loop;
      * the 0.125 cm-1 ladder is there for the lean loop itself: a workgroup takes it where the store's widest line stays
        below 0.3 of a grid step (kEtaSevenPoints, near_radius), so every rung is narrow (0.01 and 0.02 cm-1/atm) and the
        shift exceeds a grid step where the Lorentz width is a fifth of one."""
    w0, dw, _ = LADDERS[kind]
    narrow = dict(yair=0.01, yself=0.02) if kind == "eighth" else {}
    rungs = [rung("at the grid's first point, shifted downward", v0=w0 + 0.4 * dw, delta=-0.1)]
    rungs += [rung(f"delta {d}, {off} of a step off", delta=d, off=off) for d in (0.1, -0.1) for off in (0.0, 0.5, 0.3)]
    rungs += [rung("ordinary"), rung("delta 0.05", delta=0.05)]
    lad = Ladder(str(tmp_path), kind, [dict(r, **narrow) for r in rungs])
    assert lad.K % 2 == 1
    col = column(8)
    vnn, gamma, alpha = lad.prepared(oracle, lib, col)
    c = np.floor((vnn - w0) / dw + 0.5)                                     # kernels.c:431-432
    moved = np.abs(c[:, 1:7] - c[0, 1:7])
    if kind == "fine":
        assert np.all(c[:2, 0] == 0.0) and np.all(c[-1:, 0] < 0.0), c[:, 0]     # witness: on the grid at the top, off it below
        assert moved.max() >= 2.0, moved                                        # witness: more than one grid step
        want = lad.band.oracle_tau(oracle, oracle, lib, col)
        assert np.all(lad.per_rung(want)[-1:, 0] == 0.0) and np.all(lad.per_rung(want)[:2, 0] > 0.0)
    if kind == "eighth":
        # witness: a layer whose every line is narrower than 0.25 of a grid step (340/296 K at most widen it to 0.3: the
        # lean loop's condition), with centres moved a whole step and more, either way
        # -- and whose region 1 (123.4 Doppler widths, RFM_voigt.c:109) ends within the seven points at the top of the band
        lean_layers = np.all(gamma / dw <= 0.25, axis=1)
        reach = 123.4 * np.max(alpha / vnn, axis=1) * (lad.band.wn + 25.0) / (np.sqrt(np.log(2.0)) * dw) + 0.51
        lean_layers &= reach < 4.0
        assert np.any(lean_layers & np.any(c[:, 1:4] - c[0, 1:4] >= 2.0, axis=1)), (gamma / dw, reach, moved)
        assert np.any(lean_layers & np.any(c[:, 4:7] - c[0, 4:7] <= -1.0, axis=1)), (gamma / dw, reach, moved)
    check_ladder(lad, device, oracle, lib, col, 0.36)


UNUSUAL = [dict(), dict(yself=0.0), dict(yair=0.0), dict(yair=0.0, yself=0.0), dict(s0=0.0), dict(s0=1e-20, en=20000.0),
           dict(en=-1.0, s0=1e-19), dict(delta=0.1), dict(off=0.5, delta=0.0), dict(nexp=0.123456), dict(s0=1e-40),
           dict(yair=1.0, yself=2.0), dict()]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [97, 130])
def test_a_crowded_wave_of_ordinary_and_unusual_lines(tmp_path, oracle, lib, device, kind, n):
    """Branch: one wave of the lean loop holding lines that stay in it and lines it hands to general_block (xl_mask: any
    pattern of lanes and halves), 97 or 130 lines of one cell -- ordinary ones between lines without a width, without
    strength, with a strength outside the lean range, on the halfway mark, with an exponent that is not tabulated.
    The lines overlap: layer norm only."""
    band = bare_band(str(tmp_path), kind, SPACING)
    offs = np.linspace(-0.45, 0.45, n)
    rungs = []
    for i in range(n):
        r = rung(f"line {i}", **dict(dict(off=float(offs[i])), **UNUSUAL[i % len(UNUSUAL)]))
        rungs.append(complete(r, i, None))
        rungs[-1]["v0"] = mark(kind, 0, rungs[-1]["off"])
    rungs.sort(key=lambda r: r["v0"])
    band.lines = lines_of(rungs)
    col = column(7)
    want = band.oracle_tau(oracle, oracle, lib, col)
    assert np.all(np.isfinite(want))
    check_layer_norm(band, device, col, want, fused_forms(band, device, col))


@pytest.mark.parametrize("kind", KINDS)
def test_the_same_through_a_hitran_file(tmp_path, oracle, lib, device, kind):
    """Branch: the HITRAN reader (grt_hitran.c) on the fields as a real file writes them at the ends of their ranges --
    '.0001', '0.000', '-1.0000', '-.100000', '1.000E-45' -- and from there the same hand-overs as above; the oracle gets
    what the text holds (read_back_par_values)."""
    w0, dw, _ = LADDERS[kind]
    rungs = [rung("air width .0001", yair=0.0001), rung("self width 0.000", yself=0.0), rung("E -1.0000", en=-1.0, s0=1e-19),
             rung("delta -.100000", delta=-0.1), rung("s0 1.000E-45", s0=1e-45), rung("s0 1e-16", s0=1e-16),
             rung("on a grid point", off=0.0, delta=0.0), rung("on the halfway mark", off=0.5, delta=0.0),
             rung("E 15000", en=15000.0, s0=1e-24)]
    lad = Ladder(str(tmp_path), kind, rungs)
    lad.through_file(str(tmp_path / "par"))
    held = {m: ln for m, ln in lad.band.lines.items()}
    flat = lambda key: np.concatenate([held[m][key] for m in held])
    assert np.float32(0.0001) in flat("yair") and 0.0 in flat("yself") and -1.0 in flat("en")
    assert np.float32(-0.1) in flat("delta") and 1e-45 in flat("s0") and 1e-16 in flat("s0")
    with open(lad.band.par) as f:
        text = f.read()
    for field in (".0001", "0.000", "-1.0000", "-.100000", "1.000E-45"):
        assert field in text, field
    check_ladder(lad, device, oracle, lib, column(8), 0.38, from_file=True)
