"""The cases of tests/test_gpu_lean_block_bits.py and of tests/golden/make_lean_first_pass_bits.py, which recorded their
expected bits: four grids of 321 points at 1 cm-1, one per path of the lean block (mp_lean_block.inc), seeded line lists
of three molecules without continua, two columns of three layers (top-of-atmosphere, mid, surface pressure), cell tiles
of 64, one line slice.

Every list holds, cell by cell (cell c: the grid point w0 + c):
    cells 60 .. 64      no line at all (empty cells), and an ODD number of lines below them: the tile that begins at cell
                        64 begins on an odd line index (its line range reaches a cell or two below the tile, for the
                        pressure shifts: the gap is wider than that);
    cells 100 .. 139    a few lines per cell: a row of 32 consecutive lines spans three cells and more (the `odd` path);
    cell 150            one line 4e-6 of a grid step beyond the half-way mark to cell 151, without pressure shift: handed
                        to general_block in every layer; and one line with zeroed strength;
    cells 200 .. 249    two lines per cell ON the grid point, without pressure shift: a hundred core points where a grid
                        step is many Doppler widths -- one full batch of the raw queue and a partial one;
    elsewhere           `per_cell` lines per cell, up to 0.48 of a grid step from the grid point.
The number of lines is no multiple of 128."""
import numpy as np

from grtcode_amd import api, synthetic as syn
from line_ladder import MOLS, complete, lines_of
from scenario import Band

NCELL = 321
TILE = 64
#: name -> (first wavenumber, lines per cell, shortwave tables, what the block does there)
GRIDS = {
    "far_infrared": (1.0, 300, False, "NARROW, single, kTfLreg"),
    "two_cell_rows": (2000.0, 30, False, "two-cell rows, kTfLreg"),
    "region_two": (12000.0, 30, True, "general near field with region 2"),
    "ultraviolet": (45000.0, 30, True, "kTfCorrected with fold, kTfNcOne/kTfNcThree, core points through the raw queue"),
}
SEED = 20261020


def line_rungs(name):
    """The grid's lines in the order of their centres, as line_ladder's completed rungs."""
    w0, per_cell, _, _ = GRIDS[name]
    rng = np.random.default_rng(SEED + sorted(GRIDS).index(name))
    cells = []
    for c in range(NCELL):
        if 60 <= c <= 64:
            n = 0
        elif 100 <= c < 140:
            n = 8 if per_cell > 100 else 5
        elif 200 <= c < 250:
            n = 0
        else:
            n = per_cell
        cells.append(np.full(n, c))
    cell = np.concatenate(cells)
    off = rng.uniform(-0.48, 0.48, cell.size)
    off = np.where(cell == 0, np.abs(off), np.where(cell == NCELL - 1, -np.abs(off), off))      # (every line on the grid: none is dropped)
    if np.count_nonzero(cell < 60) % 2 == 0:                     # an odd number of lines below the empty cells
        cell, off = np.append(cell, 10), np.append(off, 0.1)
    on_grid = np.repeat(np.arange(200, 250), 2)
    cell = np.concatenate([cell, on_grid, [150, 150]])
    off = np.concatenate([off, np.tile([0.0, 1e-6], 50), [0.5 + 4e-6, 0.2]])
    n = cell.size
    if n % 128 == 0:
        cell, off, n = np.append(cell, 300), np.append(off, -0.3), n + 1
    par = dict(s0=10.0 ** rng.uniform(-24.0, -20.0, n), yair=np.round(rng.uniform(0.02, 0.10, n), 4),
               yself=np.round(rng.uniform(0.1, 0.5, n), 3), en=np.round(rng.uniform(0.0, 3000.0, n), 4),
               nexp=np.round(rng.uniform(0.4, 0.8, n), 2), delta=np.round(rng.uniform(-0.01, 0.0, n), 4))
    unshifted = (off == 0.0) | (off == 1e-6) | (off == 0.5 + 4e-6)
    par["delta"][unshifted] = 0.0
    par["s0"][(cell == 150) & (off == 0.2)] = 0.0
    v0 = w0 + cell + off
    order = np.argsort(v0, kind="stable")
    return [complete({k: float(a[j]) for k, a in par.items()}, i, float(v0[j])) for i, j in enumerate(order)]


def band_of(root, name):
    w0, _, sw, _ = GRIDS[name]
    band = Band(str(root), w0, w0 + NCELL - 1, 1.0, 0, mols=MOLS, sw=sw, with_ctm=False, with_cfc=False, with_cia=False)
    rungs = line_rungs(name)
    assert len(rungs) % 128 != 0
    band.lines = lines_of(rungs)
    return band


def columns():
    """Two columns of four levels: layers at top-of-atmosphere, mid and surface pressure."""
    out = []
    for seed in (3, 5):
        col = syn.profile(seed, 4)
        col["p"] = np.array([0.01, 0.1, 300.0, 1013.25])
        t = np.array([210.0, 230.0, 260.0, 295.0]) + (0.0 if seed == 3 else -12.5)
        col["t"] = t
        col["t_layer"] = 0.5 * (t[:-1] + t[1:])
        col["t_surf"] = float(t[-1])
        out.append(col)
    return out


def first_pass_tau(band, device):
    """tau of the lines [column][layer][point] in the two-pass form (lean first pass plus the gather), and the line ranges of
    its cell tiles."""
    taus, ranges = [], None
    for col in columns():
        V = col["p"].size
        go, grid = band.gas_optics(device, V, from_file=False)
        go.tune(tile=TILE, nslice=1, fast=3)
        band.set_column(go, col)
        opt = api.OpticsObject(V - 1, grid, device)
        go.calculate_optical_depth(col["p"], col["t"], opt)
        taus.append(opt.read()[0])
        info = go.last_launch()
        assert info["fast"] == 3 and info["tile"] == TILE and info["nslice"] == 1 and info["tree_levels"] == 0, info
        ranges = go.tile_items()[1]
        opt.destroy()
        go.destroy()
    return np.array(taus), ranges
