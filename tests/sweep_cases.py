"""Cases for the two sweep methods (k_gas_optics_sweep.hip, the oracle's orc_bin_sweep / orc_line_sweep) outside what the
seeded bands of tests/test_gpu_sweep_methods.py reach: grids of a few bins, lines up to the top of the grid, every shape
of the last bin, line counts at which the wave-collective searches change shape, and shifts that reorder neighbours.
Shared by tests/test_oracle_sweep_shapes.py (CPU) and tests/test_gpu_sweep_shapes.py (device).

Every band here holds lines only -- no continua, CFCs or collision pairs -- so that a bin's optical depth is the sum of
its lines' terms and can be judged bin by bin.  Grids start at W0 = 500 cm-1; columns are syn.profile(.., 4) (three
layers, 0.01 mb to 1 atm) unless a case says otherwise.

A bin is `ppb = floor(1/dw) + 1` grid points (spectral_bin.c:52), so it is ppb*dw wide: 2, 2, 1.5, 1.2, 1.25, 1.1 cm-1
for dw = 2, 1, 0.5, 0.3, 0.25, 0.1."""
import os

import numpy as np

from grtcode_amd import synthetic as syn
from scenario import MOLTAB, Band

W0 = 500.0
WAVENUMBER_SWEEP, LINE_SWEEP = 0, 1
METHODS = (WAVENUMBER_SWEEP, LINE_SWEEP)
FLOOR = 2.0 ** -53                      # an optical depth below it changes no transmittance by an ulp (line_ladder.py)
F32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)


def ppb_of(dw):
    return int(np.floor(1.0 / dw) + 1)


def shape_of(dw, npts):
    """(ppb, last_ppb, do_interp, do_last_interp, n) of a grid, as spectral_bin.c:52-68 forms them."""
    ppb = ppb_of(dw)
    last = npts % ppb or ppb
    return ppb, last, int(ppb > 3), int(last > 3), npts // ppb + (ppb != last)


def upper_end(npts, dw):
    """A grid's upper wavenumber for create_spectral_grid, n = ceil((wn - w0)/dw) + 1: the last point -- lines above wn
    are not loaded -- or, where the rounding of (npts - 1) dw / dw tips the ceiling, the nearest double below it that
    does not.  One point: wn = w0, which the constructor refuses."""
    wn = W0 + (npts - 1) * dw
    while npts > 1 and int(np.ceil((wn - W0) / dw)) + 1 != npts:
        wn = np.nextafter(wn, W0)
    assert W0 + (npts - 1) * dw - wn < 1e-9
    return float(wn)


def bare_band(root, npts, dw, mols):
    band = Band(root, W0, upper_end(npts, dw), dw, 0, mols=mols, with_ctm=False, with_cfc=False, with_cia=False)
    assert band.nw == npts, (band.nw, npts)
    return band


def set_lines(band, lines):
    """The band's line lists; every centre within [w0, wn], outside which the product loads no line."""
    for ln in lines.values():
        assert ln["v0"].size == 0 or (ln["v0"].min() >= band.w0 and ln["v0"].max() <= band.wn)
    band.lines = lines


def lines_with_centres(mol, v0, seed, delta=None):
    """syn.line_list's parameters on the given (ascending) centres, every isotopologue in turn, as a .par file holds them."""
    v0 = np.asarray(v0, dtype=np.float64)
    assert np.all(np.diff(v0) >= 0.0)
    ln = syn.line_list(mol, v0.size, 1.0, 2.0, seed)
    ln["v0"] = v0
    if delta is not None:
        ln["delta"] = F32(delta)
    ln["iso"] = (1 + (np.arange(v0.size) * 7 + mol) % MOLTAB[mol][1]).astype(np.int32)
    return syn.read_back_par_values({mol: ln})[mol]


def spread(rng, n, lo, hi):
    return np.sort(np.round(rng.uniform(lo, hi, n), 6).clip(lo, hi))


def bin_starts(dw, npts):
    return np.arange(0, npts, ppb_of(dw))


def per_bin(a, dw, npts):
    """Largest |a| of every (layer, bin): [L][n]."""
    return np.maximum.reduceat(np.abs(a), bin_starts(dw, npts), axis=1)


def bin_failures(got, want, dw, tol=1e-11):
    """got against want bin by bin: max |got - want| over a bin <= tol x the oracle's largest value in that bin + 2^-53.
    Derived, not measured: every term is non-negative except the three-point quadratic, whose weights stay within
    [-0.125, 1]; at most 130 terms a bin; S(T), gamma and alpha agree to 1e-13
    (test_gpu_gas_optics.py::test_line_prep_and_windows_bit_exact) -- about 1e-12.  Returns what is out of bounds."""
    npts = want.shape[1]
    peak, err = per_bin(want, dw, npts), per_bin(got - want, dw, npts)
    live = peak > 0.0
    worst = float(np.max(np.where(live, np.maximum(err - FLOOR, 0.0) / np.where(live, peak, 1.0), 0.0)))
    print(f"worst bin {worst:.2e} of its peak (bound {tol:.1e})")
    return [f"layer {i} bin {j}: error {err[i, j]:.3e}, peak {peak[i, j]:.3e}" for i, j in np.argwhere(err > tol * peak + FLOOR)]


# ---- (a) short grids: 1, 2, 3 bins and the three counts around nbin_remote = 25 ------------------------------------- #
SHORT_BINS = (1, 2, 3, 25, 26, 27)
SHORT_DW = (2.0, 1.0, 0.3, 0.25)            # ppb 1, 2, 4, 5
SHORT_MOLS = [syn.H2O, syn.CO2]
SHORT_LINES = 37
#: (whole bins m, dw, extra points past the last whole bin: 0 or 1)
SHORT_CASES = [(m, dw, extra) for m in SHORT_BINS for dw in SHORT_DW for extra in ((0, 1) if ppb_of(dw) > 1 else (0,))]
#: the 25-bin dw 0.25 grid of (a), for the pipeline case
PIPELINE_SHORT = (25, 0.25, 0)


def short_points(m, dw, extra):
    return m * ppb_of(dw) + extra


def short_refused(m, dw, extra):
    """The one case of (a) with a single grid point (one bin of one point): create_spectral_grid wants wn > w0."""
    return short_points(m, dw, extra) < 2


def short_pair(root, m, dw, extra):
    """The short grid and its partner: same w0 and dw, 40 more whole bins counted from the short grid's last whole bin,
    the same lines -- whose unshifted centres lie 0.1 cm-1 inside the short grid's first and last point (|delta| <= 0.02
    under at most 1.1 atm: no shifted centre leaves it).  Returns (short band, long band, column)."""
    ppb, npts = ppb_of(dw), short_points(m, dw, extra)
    short = bare_band(os.path.join(root, "short"), npts, dw, SHORT_MOLS)
    long_ = bare_band(os.path.join(root, "long"), (m + 40) * ppb, dw, SHORT_MOLS)
    rng = np.random.default_rng(1000 * m + int(100 * dw) + extra)
    lo, hi = W0 + 0.1, W0 + (npts - 1) * dw - 0.1
    assert hi > lo
    lines = {mol: lines_with_centres(mol, spread(rng, SHORT_LINES, lo, hi), seed=31 + m) for mol in SHORT_MOLS}
    col = syn.profile(40 + m, 4)
    assert np.all(np.abs(np.concatenate([ln["delta"] for ln in lines.values()])) <= 0.02)
    assert col["p"].max() * 0.000986923 < 1.1
    set_lines(short, lines)
    set_lines(long_, {mol: dict(ln) for mol, ln in lines.items()})
    return short, long_, col


def embedded_points(m, dw, extra):
    """The short grid's points that its partner must reproduce: all of them, but for the single point of the last bin of
    an m ppb + 1 grid (in the long grid that point opens a whole bin, with other interpolation wavenumbers)."""
    return m * ppb_of(dw)


# ---- (b) line_sweep with lines up to the top of the grid ------------------------------------------------------------ #
TOP_CASES = [(1.0, 80), (1.0, 81), (0.25, 200), (0.25, 201)]       # 40 whole bins; a multiple of ppb and one point more
TOP_MOLS = [syn.H2O, syn.CO2, syn.O3]


def top_case(root, dw, npts):
    """300 lines over the whole grid: 240 anywhere, 40 within 25 cm-1 of the last point, 20 within 1.5 cm-1 of it."""
    band = bare_band(root, npts, dw, TOP_MOLS)
    rng = np.random.default_rng(int(1000 * dw) + npts)
    last = W0 + (npts - 1) * dw
    v = np.concatenate([rng.uniform(W0, last, 240), rng.uniform(last - 24.9, last, 40), rng.uniform(last - 1.4, last - 0.05, 20)])
    v = np.round(rng.permutation(v), 6).clip(W0, band.wn)
    set_lines(band, {mol: lines_with_centres(mol, np.sort(v[k::3]), seed=51) for k, mol in enumerate(TOP_MOLS)})
    return band, syn.profile(52, 4)


def shifted_centres(oracle, lib, band, col):
    """oracle.line_prep's shifted centres of every molecule of the band: {mol: [L][N]}."""
    p_atm = col["p"] * np.float64(np.float32(0.000986923))
    n, pavg, tavg = oracle.layer_means(p_atm, col["t"])
    out = {}
    for m in band.oracle_inputs(oracle, lib, col)["mols"]:
        ps, _ = oracle.species_means(p_atm, m["x"], n)
        out[m["id"]] = oracle.line_prep(m["lines"], m["mass"], m["num_iso"], pavg, tavg, ps, m["q"])[0]
    return out


def top_witness(oracle, lib, band, col):
    """Every layer has at least 20 shifted centres within 1.5 cm-1 of the last grid point and 60 within 25 cm-1."""
    v = np.concatenate(list(shifted_centres(oracle, lib, band, col).values()), axis=1)
    last = band.w0 + (band.nw - 1) * band.dw
    assert np.all(np.sum(last - v <= 1.5, axis=1) >= 20) and np.all(np.sum(last - v <= 25.0, axis=1) >= 60)


# ---- (c) bin shapes --------------------------------------------------------------------------------------------------- #
SHAPE_DW = {1: 2.0, 2: 1.0, 3: 0.5, 4: 0.3, 5: 0.25, 11: 0.1}
#: (ppb, last_ppb): every last_ppb of 1, 2, 3, 4 and ppb that exists; 40 whole bins, and the last one where it is shorter
SHAPE_CASES = [(ppb, last) for ppb in SHAPE_DW for last in sorted({1, 2, 3, 4, ppb}) if last <= ppb]
#: the eight that tests/golden/live_reference.npz pins to the reference build
SHAPE_GOLDEN = [(5, 2), (5, 3), (5, 4), (5, 5), (4, 3), (4, 4), (11, 4), (1, 1)]
SHAPE_MOLS = [syn.H2O, syn.CO2, syn.O3]


def shape_points(ppb, last):
    return 40 * ppb + (last if last < ppb else 0)


def shape_case(root, ppb, last, method):
    """300 lines; for line_sweep they stay 26.5 cm-1 below the top of the grid, where the reference defines it."""
    dw, npts = SHAPE_DW[ppb], shape_points(ppb, last)
    assert shape_of(dw, npts)[:2] == (ppb, last) and 40 <= shape_of(dw, npts)[4] <= 45
    band = bare_band(root, npts, dw, SHAPE_MOLS)
    top = band.wn - (26.5 if method == LINE_SWEEP else 0.0)
    rng = np.random.default_rng(100 * ppb + last)
    set_lines(band, {mol: lines_with_centres(mol, spread(rng, 100, W0, top), seed=61) for mol in SHAPE_MOLS})
    return band, syn.profile(60 + ppb, 4)


# ---- (d) line counts at which first_true_wave changes shape (64, 64^2) ---------------------------------------------------- #
COUNT_N = (1, 2, 63, 64, 65, 4095, 4096, 4097)
COUNT_DW, COUNT_POINTS = 0.5, 180           # ppb 3: 60 bins of 1.5 cm-1, 500 to 589.5 cm-1
COUNT_BIN = 20                              # the one bin of the clustered form: 530 to 531 cm-1, 58.5 cm-1 from the top


def count_case(root, n, clustered):
    """One molecule with exactly n lines: over the whole grid, or all inside bin COUNT_BIN -- then every other bin has
    all its lines to one side."""
    band = bare_band(root, COUNT_POINTS, COUNT_DW, [syn.CO2])
    rng = np.random.default_rng(7 * n + clustered)
    b0 = W0 + COUNT_BIN * ppb_of(COUNT_DW) * COUNT_DW
    lo, hi = (b0 + 0.1, b0 + 0.9) if clustered else (W0, band.wn)
    set_lines(band, {syn.CO2: lines_with_centres(syn.CO2, spread(rng, n, lo, hi), seed=71)})
    return band, syn.profile(70, 4)


# ---- (e) shifts that reorder neighbours by many places -------------------------------------------------------------------- #
REORDER_DW, REORDER_POINTS = 0.25, 150      # ppb 5: 30 bins of 1.25 cm-1


#: cm-1 between neighbours: 0.002, where the whole cluster lies within any shift, and 0.03, where the lines that swap in
#: the bottom layer (shifts of +-0.157 cm-1 under 1.57 atm) lie up to 0.31 cm-1 apart -- the full width of
#: sweep_sort_kernel's reach, 2 dmax |pavg|, and twice what half of it would cover
REORDER_SPACINGS = (0.002, 0.03)


def reorder_case(root, spacing):
    """40 CO2 lines `spacing` apart, delta = +0.1 / -0.1 in runs of one (12 lines), two (8) and five (20), under
    line_ladder.column(8): 1e-6 mb to 3 atm."""
    import line_ladder
    band = bare_band(root, REORDER_POINTS, REORDER_DW, [syn.CO2])
    sign = np.concatenate([np.tile([1.0, -1.0], 6), np.tile([1.0, 1.0, -1.0, -1.0], 2), np.tile([1.0] * 5 + [-1.0] * 5, 2)])
    assert sign.size == 40
    centres = np.round(518.0 + spacing * np.arange(40), 6)
    set_lines(band, {syn.CO2: lines_with_centres(syn.CO2, centres, seed=81, delta=0.1 * sign)})
    return band, line_ladder.column(8)


def reorder_witness(oracle, lib, band, col):
    """The top layer's shifted centres are ascending as listed; in the bottom layer some line sorts more than four places
    from where it is listed, and some pair that swaps lies more than 0.9 of the largest possible distance apart, twice
    the largest shift, unless the whole cluster is narrower than that."""
    v = shifted_centres(oracle, lib, band, col)[syn.CO2]
    v0 = band.lines[syn.CO2]["v0"]
    assert np.all(np.diff(v[0]) > 0.0)
    rank = np.argsort(np.argsort(v[-1], kind="stable"), kind="stable")
    assert np.max(np.abs(rank - np.arange(rank.size))) > 4
    swapped = np.triu(v[-1][:, None] > v[-1][None, :], 1)                # [j][k], j < k: j sorts after k
    apart = np.where(swapped, v0[None, :] - v0[:, None], 0.0).max()
    assert apart > 0.9 * min(2.0 * np.abs(v[-1] - v0).max(), v0[-1] - v0[0])
