"""The far wings, point by point: two clusters of ordinary lines 60 cm-1 apart with a spectral window between them.

Every other parity metric of the line kernels divides the error by something large -- a layer's largest optical depth
(tau_close), a rung's peak (line_ladder) -- and the far field of the fused forms (cell moments, their shift to parent cells,
the near-field radius, region 1 folded into the moments, the cut at the window's edge) is small against a peak by
construction.  Here 32 lines lie 10 to 15 cm-1 above the grid's first point and 32 lie 70 to 75 cm-1 above it, with windows
of 25 cm-1 to either side, so that between the clusters
  * the first cluster's wings fall off over 20 cm-1, the windows ending one after another between 35 and 40 cm-1
    (a staircase of 32 steps: a line dropped or kept a point too long shows as 1/320 of the value there or more);
  * nothing at all reaches the points from 40 to 45 cm-1 (exact zeros in the oracle);
  * the second cluster's windows open one after another between 45 and 50 cm-1;
and in the thin layers nearly every such point lies below FAST_TOL of its layer's maximum.  Each point at X_WING Doppler
widths and more from EVERY line is judged against its own value (line_ladder.judge_wings).

Everything here comes from the oracle (layer_means, species_means, line_prep, line_sample with its windows), nothing from
a kernel's output.  Support for tests/test_far_wing_cases.py (the witnesses, on the CPU) and tests/test_gpu_far_wings.py."""
import numpy as np

from line_ladder import SQRT_LN2, X_WING, bare_band, column, complete, layer_means, lines_of

#: (first wavenumber, grid step): the far-infrared series of the lean loop, region 2 inside the lean loop, the finest grid
#: whose first pass is the lean loop, the cell hierarchy (three depths), the wave-shared tree gather
GRIDS = [(70.0, 1.0), (30000.0, 1.0), (1000.0, 0.125), (700.0, 0.05), (700.0, 0.02), (700.0, 0.005), (700.0, 0.002)]
SPAN = 85.0
CLUSTERS = ((10.0, 15.0), (70.0, 75.0))     # cm-1 above the grid's first point
PER_CLUSTER = 32
GAP = (40.0, 45.0)                          # no window reaches these points
STAIRS = (35.0, 40.0)                       # the first cluster's windows end here, one after another

# ---- the bound E of |got - want| <= E want + 2^-53, term by term ------------------------------------------------------- #
#: reference order (fast = 0) and the sweep methods, against the oracle's same method: BOUNDS[0]["pointwise_rel"] of
#: tests/test_gpu_parity_production.py
E_STRICT = 1e-9
#: the fused Voigt, pointwise: the class of the Lorentzian and region-1 evaluations in fp32 (tests/test_gpu_voigt.py)
E_VOIGT = 5e-6
#: the lean loop's fp32 amplitude (mp_lean_block.inc, header comment)
E_AMPLITUDE = 2e-7
#: what the moment series leaves out with seven-point near fields, of the far-wing value (gas_optics_mp_dev.h, near_radius;
#: tests/test_moment_series.py); the 8- and 12-term series of wider near fields stay below 1e-7
E_SERIES = 6e-7
#: sequential fp32 sums of positive terms, one rounding of 2^-24 per line that covers the point; the higher moments add at
#: most sum_k 0.128^k = 0.147 of that (near_radius: |z|/(R + 1) <= 0.128)
E_SUM_PER_LINE = 1.15 * 2.0 ** -24
#: region 1 carried on by the moments beyond a line's XLIM0, where the reference is back at the Lorentzian: 1.5/x^2 of the
#: line's value there (gas_optics_mp_dev.h, near_radius; BOUNDS[3] of tests/test_gpu_parity_production.py names the same
#: departure); the nearest line bounds it for the sum
FOLD_EXCESS = 1.5


def fused_bound(x_min, covering):
    """E of the fused forms at points x_min >= X_WING Doppler widths from the nearest line, covered by `covering` lines."""
    return E_VOIGT + E_AMPLITUDE + E_SERIES + E_SUM_PER_LINE * covering + FOLD_EXCESS / np.maximum(x_min, X_WING) ** 2


def case_name(w0, dw):
    return f"{w0:g}_{dw:g}"


def window_band(root, w0, dw, seed=1):
    """The bare band (line_ladder.bare_band: lines of MOLS only, no continua, CFCs or collision pairs) from w0 to w0 + 85
    with the two clusters of 32 lines; every parameter from one default_rng(seed)."""
    band = bare_band(root, (w0, dw, w0 > 3000.0), SPAN)
    rng = np.random.default_rng(seed)
    n = PER_CLUSTER * len(CLUSTERS)
    centres = np.round(np.sort(np.concatenate([rng.uniform(w0 + lo, w0 + hi, PER_CLUSTER) for lo, hi in CLUSTERS])), 6)
    assert np.all(np.diff(centres) > 0.0)
    par = dict(s0=10.0 ** rng.uniform(-20.0, -19.0, n), yair=rng.uniform(0.05, 0.1, n), yself=rng.uniform(0.3, 0.5, n),
               en=rng.uniform(100.0, 1500.0, n), nexp=np.round(rng.uniform(0.5, 0.8, n), 2), delta=rng.uniform(-0.02, 0.02, n))
    lines = [complete({key: float(par[key][i]) for key in par}, i, float(centres[i])) for i in range(n)]
    band.lines = lines_of(lines)
    return band


class WindowCase:
    """window_band on line_ladder.column(8) with the oracle's optical depths (`want`) and, per (layer, point): x_min (the
    distance from the nearest shifted centre in ITS Doppler widths), covering (how many lines' windows hold the point) and
    wing (x_min >= X_WING and want > 0)."""

    def __init__(self, root, oracle, lib, w0, dw, seed=1):
        self.w0, self.dw, self.name = w0, dw, case_name(w0, dw)
        self.band = band = window_band(root, w0, dw, seed)
        self.col = col = column(8)
        self.w = w0 + dw * np.arange(band.nw)
        n, pavg, tavg = layer_means(oracle, col)
        p_atm = col["p"] * np.float64(np.float32(0.000986923))
        L, nw = pavg.size, band.nw
        self.x_min = np.full((L, nw), np.inf)
        self.covering = np.zeros((L, nw), dtype=np.int64)
        lines_only = np.zeros((L, nw))
        for m in band.oracle_inputs(oracle, lib, col)["mols"]:
            ps, ns = oracle.species_means(p_atm, m["x"], n)
            vnn, snn, gamma, alpha = oracle.line_prep(m["lines"], m["mass"], m["num_iso"], pavg, tavg, ps, m["q"])
            tau, s, e = oracle.line_sample(vnn, snn, gamma, alpha, ns, w0, dw, nw, windows=True)
            lines_only += tau
            for j in range(L):
                for l in range(vnn.shape[1]):
                    np.minimum(self.x_min[j], np.abs(self.w - vnn[j, l]) * (SQRT_LN2 / alpha[j, l]), out=self.x_min[j])
                    if s[j, l] <= e[j, l]:
                        self.covering[j, s[j, l]:e[j, l] + 1] += 1
        self.want = band.oracle_tau(oracle, oracle, lib, col)
        # (the band has nothing but its lines; the molecules' sums in another order)
        assert np.allclose(self.want, lines_only, rtol=1e-13, atol=0.0) and np.all(np.isfinite(self.want))
        # (no optical depth outside every window; inside one, a line without a Lorentz width to speak of underflows)
        assert np.all(self.want >= 0.0) and not np.any((self.want != 0.0) & (self.covering == 0))
        self.wing = (self.x_min >= X_WING) & (self.want > 0.0)
        self.E = fused_bound(self.x_min, self.covering)
        self._sweeps = {}

    def between(self, lo, hi):
        """The grid points from w0 + lo to w0 + hi, as a mask."""
        return (self.w >= self.w0 + lo) & (self.w <= self.w0 + hi)

    def want_sweep(self, oracle, lib, method):
        """The oracle's optical depths by a sweep method (computed once)."""
        if method not in self._sweeps:
            self._sweeps[method] = self.band.oracle_tau(oracle, oracle, lib, self.col, method=method)
        return self._sweeps[method]

    def layer_norm(self, got, want=None):
        """tau_close's metric, per layer: the largest error over the layer's largest optical depth."""
        want = self.want if want is None else want
        return np.max(np.abs(got - want), axis=1) / np.maximum(np.max(np.abs(want), axis=1), 1e-300)
