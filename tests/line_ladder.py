"""Ladders of isolated lines: one line per rung, 60 cm-1 apart, windows of 25 cm-1 to either side and no continua, so every
grid point sees at most one line and rung k owns the 60 cm-1 of grid around it.  A rung is then judged on its own terms,

    max |got - want| <= tol * peak(layer, rung) + 2^-53,

peak being the oracle's largest value in the rung's window -- not on the terms of the layer's strongest line (tau_close).
The floor is derived, not measured: an optical depth below 2^-53 changes no transmittance e^-tau by an ulp; it also keeps a
line whose fp32 amplitude underflows on the device from counting as an error.  A window the oracle fills with zeros must be
all zeros on the device.  Support for tests/test_gpu_line_ladder.py."""
import os

import numpy as np

from grtcode_amd import synthetic as syn
from scenario import MOLTAB, Band

SPACING = 60.0                              # cm-1 between rungs; rung k is centred 30 cm-1 above the start of its 60
FLOOR = 2.0 ** -53
# The far wing, point by point.  A point at x = |w - centre| sqrt(ln 2)/alpha >= X_WING Doppler widths of EVERY line lies
# beyond every line's XLIM0 (at most 123.4, RFM_voigt.c:109), where the oracle is a plain Lorentzian: no region 1, no
# near-centre arithmetic, nothing a kernel adds and takes back.  There each point is judged against ITSELF,
#     |got - want| <= E want + 2^-53,
# where the peak norms above and tau_close divide by something orders of magnitude larger.
X_WING = 130.0
SQRT_LN2 = float(np.sqrt(np.log(2.0)))


def judge_wings(got, want, E, wing, zero, what):
    """`got` against `want` on the points `wing` ([L][n], want != 0 there), each within E (a number or [L][n]) of its own
    value plus the floor; on the points `zero` (want == 0 there) got is zero.  Returns (per layer: dict of the worst
    error in units of its bound, the worst plain relative error and the number of points; failures as text, one line
    per layer with its worst point)."""
    E = np.broadcast_to(np.asarray(E, dtype=np.float64), want.shape)
    layers, bad = [], []
    for j in range(want.shape[0]):
        i = np.flatnonzero(wing[j])
        entry = dict(points=int(i.size), of_bound=0.0, rel=0.0)
        if not np.all(np.isfinite(got[j])):
            bad.append(f"{what}: layer {j}: not finite")
            entry["of_bound"] = entry["rel"] = float("inf")
        elif i.size:
            err = np.abs(got[j, i] - want[j, i])
            size = np.abs(want[j, i])
            ratio = err / (E[j, i] * size + FLOOR)
            k = int(np.argmax(ratio))
            entry.update(of_bound=float(ratio[k]), rel=float(np.max(err / size)), at=int(i[k]))
            if ratio[k] > 1.0:
                bad.append(f"{what}: layer {j}: {int(np.sum(ratio > 1.0))} of {i.size} wing points out of bounds, worst at "
                           f"point {i[k]}: got {got[j, i[k]]:.9e}, want {want[j, i[k]]:.9e}, off by {err[k] / size[k]:.3e} "
                           f"of it (bound {E[j, i[k]]:.3e}, {ratio[k]:.2f} of bound and floor)")
        nz = np.flatnonzero(zero[j] & (got[j] != 0.0))
        if nz.size:
            bad.append(f"{what}: layer {j}: {nz.size} points not zero where the oracle is, first at point {nz[0]}: "
                       f"{got[j, nz[0]]:.3e}")
        layers.append(entry)
    worst = max(e["of_bound"] for e in layers)
    print(f"{what}: worst wing point {worst:.3f} of its bound, {max(e['rel'] for e in layers):.2e} of its own value")
    return layers, bad


def judged_share(want, wing, E):
    """The share of the wing points that E can judge at all: E want at or above the floor."""
    return float(np.mean(E * np.abs(want[wing]) >= FLOOR)) if np.any(wing) else 0.0
MOLS = [syn.H2O, syn.CO2, syn.O3]           # rung k belongs to MOLS[k % 3]: the slots interleave in the merged store
F32_KEYS = ("yair", "yself", "en", "nexp", "delta")     # what the loaders keep as floats (parse_HITRAN_file.c:197-212)
#: an ordinary line, as synthetic.line_list draws them; `off`: the centre's offset from the rung's grid point [grid steps]
ORDINARY = dict(s0=1e-21, yair=0.07, yself=0.35, en=300.0, nexp=0.65, delta=-0.004, off=0.3)
#: the ladders: (first wavenumber, grid step, shortwave tables)
LADDERS = {"far_infrared": (70.0, 1.0, False), "fine": (700.0, 0.05, False), "ultraviolet": (30000.0, 1.0, True),
           "eighth": (1000.0, 0.125, False)}


def rung(name, **kw):
    return dict(ORDINARY, name=name, **kw)


def mark(kind, k, off):
    """The wavenumber `off` grid steps above the grid point at the middle of rung k's 60 cm-1."""
    w0, dw, _ = LADDERS[kind]
    return w0 + (int(round((0.5 + k) * SPACING / dw)) + off) * dw


def column(levels=8, seed=3):
    """syn.profile with the top at 1e-6 mb, the bottom at 3 atm, and 150 K (top) to 340 K (bottom)."""
    col = syn.profile(seed, levels)
    col["p"] = np.geomspace(1e-6, 3.0 * 1013.25, levels)
    col["t"] = np.linspace(150.0, 340.0, levels)
    col["t_layer"] = 0.5 * (col["t"][:-1] + col["t"][1:])
    col["t_surf"] = float(col["t"][-1])
    return col


def layer_means(oracle, col):
    """(n, pavg [atm], tavg) of the column's layers, as Band.oracle_inputs forms them."""
    return oracle.layer_means(col["p"] * np.float64(np.float32(0.000986923)), col["t"])


def bare_band(root, kind, span):
    """`span` cm-1 of a ladder's grid (its name, or another grid's (first wavenumber, step, shortwave tables)) with lines of
    MOLS only: no continua, CFCs or collision pairs, no lines yet."""
    w0, dw, sw = LADDERS[kind] if isinstance(kind, str) else kind
    return Band(root, w0, w0 + span, dw, 0, mols=MOLS, sw=sw, with_ctm=False, with_cfc=False, with_cia=False)


def complete(r, i, v0):
    """Line i of a list: its molecule and isotopologue, the float parameters rounded as the loaders keep them."""
    r = dict(r, mol=MOLS[i % len(MOLS)])
    for key in F32_KEYS:
        r[key] = float(np.float32(r[key]))
    r.setdefault("v0", v0)
    r["iso"] = 1 + (7 * i + r["mol"]) % MOLTAB[r["mol"]][1]
    return r


def lines_of(rungs):
    """Band.lines of completed rungs, which are in the order of their centres."""
    out = {}
    for m in MOLS:
        mine = [r for r in rungs if r["mol"] == m]
        out[m] = {key: np.array([r[key] for r in mine], dtype=np.float64) for key in ("v0", "s0") + F32_KEYS}
        out[m]["iso"] = np.array([r["iso"] for r in mine], dtype=np.int32)
    return out


class Ladder:
    def __init__(self, root, kind, rungs):
        """rungs: dicts of line parameters (rung()); a rung without "v0" is centred `off` grid steps from its grid point."""
        self.w0, self.dw, _ = LADDERS[kind]
        self.K = len(rungs)
        self.band = bare_band(root, kind, SPACING * self.K)
        self.rungs = [complete(r, k, mark(kind, k, r["off"])) for k, r in enumerate(rungs)]
        self.set_lines()
        nw = self.band.nw
        # rung k owns the grid points from 60 k to 60 (k + 1) cm-1 above w0 (the last rung: to the end of the grid)
        self.starts = np.array([int(np.ceil(SPACING * k / self.dw - 1e-9)) for k in range(self.K)])
        assert self.starts[0] == 0 and self.starts[-1] < nw and np.all(np.diff(self.starts) > 0)

    def set_lines(self):
        """The rungs as the band's per-molecule line lists (Band.lines), in rung order -- which is the order of centres."""
        v0 = [r["v0"] for r in self.rungs]
        assert all(b > a for a, b in zip(v0, v0[1:]))
        for k, r in enumerate(self.rungs):
            # the window (25 cm-1 about the grid point nearest the shifted centre; a shift of |delta| cm-1/atm under at
            # most 3 atm) stays inside the rung's 60 cm-1 -- or is clipped by the grid's own ends
            reach = 25.0 + self.dw + 3.0 * abs(r["delta"])
            assert k == 0 or r["v0"] - reach > self.w0 + SPACING * k, r
            assert k == self.K - 1 or r["v0"] + reach < self.w0 + SPACING * (k + 1), r
        self.band.lines = lines_of(self.rungs)

    def through_file(self, directory):
        """Write the lines as a HITRAN .par file into `directory` (a fresh one: the parsed-file cache is keyed by path),
        point the band at it and keep for the oracle what the text format holds."""
        os.makedirs(directory)
        self.band.par = os.path.join(directory, "ladder.par")
        syn.write_hitran_par(self.band.par, self.band.lines)
        self.band.lines = syn.read_back_par_values(self.band.lines)

    def prepared(self, oracle, lib, col):
        """The oracle's per-layer line quantities, [layer][rung]: shifted centre, Lorentz and Doppler half-widths."""
        n, pavg, tavg = layer_means(oracle, col)
        p_atm = col["p"] * np.float64(np.float32(0.000986923))
        vnn, gamma, alpha = (np.zeros((pavg.size, self.K)) for _ in range(3))
        for m in self.band.oracle_inputs(oracle, lib, col)["mols"]:
            ps, _ = oracle.species_means(p_atm, m["x"], n)
            v, _, g, a = oracle.line_prep(m["lines"], m["mass"], m["num_iso"], pavg, tavg, ps, m["q"])
            sel = [k for k, r in enumerate(self.rungs) if r["mol"] == m["id"]]
            vnn[:, sel], gamma[:, sel], alpha[:, sel] = v, g, a
        return vnn, gamma, alpha

    # -- the far wing, point by point ---------------------------------------------------------------------------------- #
    def locate(self, oracle, lib, col):
        """Every grid point's distance from its rung's shifted centre in Doppler widths, [L][n], from the oracle's line
        preparation: every point sees one line only, its rung's.  Kept for wing_failures."""
        vnn, _, alpha = self.prepared(oracle, lib, col)
        owner = np.searchsorted(self.starts, np.arange(self.band.nw), side="right") - 1
        w = self.w0 + self.dw * np.arange(self.band.nw)
        self.x = np.abs(w[None, :] - vnn[:, owner]) * SQRT_LN2 / alpha[:, owner]
        return self.x

    def wing_failures(self, got, want, E, what):
        """got against want on the rungs' points at X_WING Doppler widths and more from the rung's own shifted centre
        (locate), each within E(x_min, covering) -- a function, or a number -- of its own value plus the floor; zero where
        the oracle is zero there.  One line a point: covering = 1."""
        far = self.x >= X_WING
        bound = E(self.x, np.ones(self.x.shape)) if callable(E) else E
        return judge_wings(got, want, bound, far & (want != 0.0), far & (want == 0.0), what + ", wing points")[1]

    # -- the per-rung metric ------------------------------------------------------------------------------------------- #
    def per_rung(self, a):
        """Largest |a| of every (layer, rung): [L][K]."""
        return np.maximum.reduceat(np.abs(a), self.starts, axis=1)

    def rung_failures(self, got, want, tol, what, peak_of=None):
        """got against want rung by rung; `peak_of`: the oracle's optical depths where `want` is another form's.
        Prints the worst error in units of the rung's peak (after the floor); returns what is out of bounds, as text."""
        if not np.all(np.isfinite(got)):
            where = np.argwhere(np.maximum.reduceat(~np.isfinite(got), self.starts, axis=1))
            return [f"{what}: layer {j} rung {k} ({self.rungs[k]['name']}): not finite" for j, k in where]
        peak = self.per_rung(want if peak_of is None else peak_of)
        err = self.per_rung(got - want)
        live = peak > 0.0
        worst = float(np.max(np.where(live, np.maximum(err - FLOOR, 0.0) / np.where(live, peak, 1.0), 0.0)))
        print(f"{what}: worst rung {worst:.2e} of its peak (bound {tol:.1e})")
        out = [f"{what}: layer {j} rung {k} ({self.rungs[k]['name']}): error {err[j, k]:.3e}, peak {peak[j, k]:.3e}, "
               f"{err[j, k] / max(peak[j, k], 1e-300):.2e} of it (bound {tol:.1e})"
               for j, k in np.argwhere(err > tol * peak + FLOOR)]
        if peak_of is None:
            out += [f"{what}: layer {j} rung {k} ({self.rungs[k]['name']}): not zero where the oracle is"
                    for j, k in np.argwhere(~live & (self.per_rung(got) != 0.0))]
        return out
