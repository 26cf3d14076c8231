"""What a live pipeline keeps between calls -- the scratch blocks of grt_scratch_need (GRT_SCRATCH_..., one per band), the
pinned staging buffers (GrtStaging) and the keyed device tables (GrtKeyedTable, kdist_table) -- reaches no result, at every
entry point: test_gpu_pipeline_scratch.py's proof for the entry points merged since it was written.

Every family of entry points runs a list of steps on one live object, each step also on a fresh object that makes that
call alone: all outputs finite, non-empty and equal bit for bit (deterministic mode, fast = 0, both pipeline forms).  The
steps start small and cross their chunk edges (Z, T, A 1 -> chunk + 1; S 1 -> 3; bins x K 1 x 2 -> 5 x 65; six rows ->
profiles; 1 -> 2 columns; one channel or response -> several that overlap), so that every buffer first appears and is then
replaced by a larger one; after each step grt_debug_pipeline_holdings' report (api.Pipeline.holdings) is held to COVERAGE
below, which names for every slot, staging buffer and keyed table the steps at which it appears and grows, or says why its
size is fixed per object.  Then the steps run backwards: no capacity moves (reuse) and the results are the recorded ones.
At the end one call per family on the grown object is held to that family's own reference (the oracle through
response_model, slant_model, surface_tiles_support, channel_model, radiance_model and ck_flux_model, with the tolerances of
the family's test module), since two equally wrong results are equal too.  The mixed test interleaves all families and
the steps of test_gpu_pipeline_scratch.py on one object.  Further tests: every keyed table under keys of equal length and
other content (A, B, A) and of another length; the entry points that share a slot in both orders; a surface in force
across a call with a GrtZenithSurface_t; two calls of different entry points queued with nothing between them, the second
of which replaces a block or a staging buffer the first one reads.

The shape: 257 grid points (three solver blocks, the last one ragged), V = 4 (at V = 3 the six-row and the level forms
have the same row counts), max_columns 2.

Before any of this ran on a device, every size formula of grt_scratch_need and grt_staging_reserve (grt_pipeline.c,
grt_pipeline_solve.c, grt_pipeline_inputs.c) was checked on paper against what its launch and its finishing kernel index:
[max_cols][slots][rows][nblocks] against grt_launch_reduce_partials' C rows x nblocks, grt_launch_subcolumn_mean's
C x S x rows x nblocks, the zenith and tile mean kernels' C x Z (T) x S x rows x nblocks, the channel, weighting and
response finishing kernels' C x S x (A x 2 | A x R | G V) x pairs; the staging needs against the offsets the stage functions
hand on.  Each holds for C <= max_cols with the slot count the entry point passes.

COVERAGE is checked against grt_pipeline_internal.h by a test without the gpu mark: a slot added to the header without
a line here, and so without a step, fails on a machine with no GPU.

Wall time of each test on an MI355X (pytest --durations, the call alone, fused / materialised form, in seconds): base
family 0.05 / 0.03, sky family 0.10 / 0.12, sun angles and tiles 0.26 / 0.08, longwave radiances 0.05 / 0.06,
k-distributions 0.04 / 0.04, all families interleaved 0.18 / 0.20, keyed tables 0.06 / 0.07, shared slots 0.09 / 0.12, surface in
force 0.01 / 0.01, two calls queued 0.01 / 0.01; the module's inputs (bands, gas optics, sampler) are made once, in 0.3 s.
The whole module: 2.6 s."""
import copy
import ctypes as C
import os
import re

import numpy as np
import pytest

from aerosol_model import aerosol_fields
from channel_model import oracle_channel_sets
from cloud_sampler_support import pipeline_fields
from grtcode_amd import api
from kdist_correlated_model import KEY_ROW, KEY_SUM, class_map
from pipeline_support import SETS, _deterministic, limits, make, make_shape_bands, pick
from pipeline_support import oracle_cache, tables  # noqa: F401  (module fixtures)
from radiance_model import oracle_radiance_sets
from response_model import oracle_spectral_sets, weighted_set
from scenario import MOL_ORDER
from sky_zenith_support import AEROSOL, ALL, CLEAN, NAMES, aerosols_of, angles, positions, run_sky, run_sky_zeniths
from test_gpu_ck_fluxes import Case as CkCase, assert_solve, assert_sums
from test_gpu_pipeline_channels import Instrument, check_model, edge_instrument, run_chan
from test_gpu_pipeline_radiances import check_integrated, run_rad, secants_of
from test_gpu_pipeline_scratch import flat
from test_gpu_pipeline_tiles import LEVEL_TOL as TILE_TOL, Inputs as TileInputs
from test_gpu_pipeline_weighted import LEVEL_TOL as WEIGHTED_TOL, check_against_model, run_weighted
from test_gpu_pipeline_weighting import run_wt
from test_gpu_sky_zeniths_direct import Case, run_zd
from test_gpu_sky_zeniths_slant import check_reference, drawn, flat as flat_cosines, run_zs
from surface_tiles_support import run_sky_tiles

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "grtcode_amd", "csrc", "host", "grt_pipeline_internal.h")
KERNELS = os.path.join(ROOT, "grtcode_amd", "csrc", "grt_kernels.h")

N, V, NCOL, S3, NK = 257, 4, 2, 3, 3
L = V - 1
USER_LEVEL = -1
ZN, TN = api.GRT_ZENITH_CHUNK, api.GRT_TILE_CHUNK
AN = int(re.search(r"#define GRT_RADIANCE_CHUNK (\d+)", open(KERNELS).read()).group(1))
Z5, T5, A5 = ZN + 1, TN + 1, AN + 1
bands = make_shape_bands((N,), 1.0, 1000.0)


# ---- the header's names ------------------------------------------------------------------------------------------------ #
def header_names():
    """(scratch slots, staging buffers, keyed tables) as grt_pipeline_internal.h declares them, in its order: the
    enumerators before GRT_SCRATCH_COUNT, the GrtStaging members of struct GrtPipeline, the GrtKeyedTable and GrtKdistTable
    members of GrtBand."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    enum = re.search(r"enum\s*\{([^}]*\bGRT_SCRATCH_COUNT\b[^}]*)\}", src).group(1)
    scratch = [n for n in re.findall(r"\bGRT_SCRATCH_\w+\b", enum) if n != "GRT_SCRATCH_COUNT"]
    band = re.search(r"typedef struct GrtBand\s*\{(.*?)\}\s*GrtBand;", src, re.S).group(1)
    keyed = re.findall(r"\b(?:GrtKeyedTable|GrtKdistTable)\s+(\w+)\s*;", band)
    pipe = re.search(r"struct GrtPipeline\s*\{(.*?)\};", src, re.S).group(1)
    staging = re.findall(r"\bGrtStaging\s+(\w+)\s*;", pipe)
    return scratch, staging, keyed


# ---- the steps, by family (the names COVERAGE speaks of) ---------------------------------------------------------------- #
FAMILIES = {
    # test_gpu_pipeline_scratch.py's steps
    "base": ("sub-S1-six", "sub-S3-six-two-sweeps", "sub-S1-profile", "sub-S3-profile", "aerosols", "allsky",
             "spectral-bins", "band-profiles", "surface-emissivity", "surface-all"),
    "sky": ("sky-six-c1", "sky-six-S1", "sky-six-S3", "sky-profile-S3", "direct-six-S1", "direct-profile-S3",
            "direct-own-levels", "jacobian-six-S1", "jacobian-profile-S3", "jacobian-own-levels", "scatter-six-S1",
            "scatter-profile-S3", "scatter-own-levels", "weighted-R1-S1", "weighted-R5-S3", "cloud-fields-S1-six",
            "cloud-fields-S3-profile"),
    "zeniths": ("zeniths-Z1-c1", "zeniths-Z5", "zeniths-Z5-profile", "sky-zeniths-Z1-S1", "sky-zeniths-Z5-S3-profile",
                "zen-direct-Z1", "zen-surface-Z1-knots2", "zen-direct-Z5-S3-profile-surface", "zen-own-levels-Z1",
                "zen-own-levels-Z5", "slant-Z1", "slant-Z5-S3-profile-surface", "tiles-T1-c1", "tiles-T5-S3"),
    "radiances": ("radiances-A1-c1", "radiances-A5-S3", "radiances-alone-A5-S3", "channels-C1-A1", "channels-C9-A5-S3",
                  "weighting-C1-A1-trans", "weighting-C9-A5-S3"),
    "kdist": ("kdist-K2-b1", "kdist-K65-b5-weight", "kdist-corr-kept", "kdist-corr-scratch", "ck-K2-b1", "ck-K65-b5-kept",
              "ck-own-sums-K2-b1", "ck-own-sums-K65-b5"),
}
FUSED_ONLY = {"slant-Z1", "slant-Z5-S3-profile-surface"}        # (the materialised form refuses the layer cosines)
ALL_STEPS = {s for names in FAMILIES.values() for s in names}
# (two entry points on the same columns and the same single cloud draw: nothing says that their results differ)
SAME_CALL = {frozenset(("sub-S1-six", "allsky"))}

# ---- the coverage table -------------------------------------------------------------------------------------------------- #
# One line per (name, bands, forms): kind -- scratch (capacity in doubles, per band), staging (capacity in doubles, per
# object; bands "-") or table (length of the stored key in bytes, per band) --, the bands (lw, sw, both) and pipeline forms
# (fused, mat, both) the line speaks of, the steps at which it appears (the first of them that runs on an object makes it
# appear), the steps at which it moves afterwards in its family's pass (a scratch or staging block grows; a key's length
# changes, either way), and -- for a block whose size is fixed per object, or a key whose length no family pass changes --
# the word "fixed" and why.  A name may take several lines.
CREATION = "creation"


def row(kind, name, bands_, forms, appears, grows="", fixed=""):
    return dict(kind=kind, name=name, bands=bands_, forms=forms, appears=tuple(appears.split()), grows=tuple(grows.split()),
                fixed=fixed)


CLOUD_FIRST = "sub-S1-six sky-six-S1 sky-zeniths-Z1-S1 radiances-A5-S3"
CLOUD_MORE = "sub-S3-six-two-sweeps sky-six-S3 sky-zeniths-Z5-S3-profile"
AEROSOL_FIRST = "aerosols sky-six-c1 sky-zeniths-Z1-S1 radiances-A1-c1"
COVERAGE = [
    row("scratch", "GRT_SCRATCH_PARK", "sw", "fused", "sub-S3-six-two-sweeps sky-profile-S3 zeniths-Z5-profile",
        fixed="fixed: [max_cols][2 V + 5 L][n], of max_cols, V and n alone"),
    row("scratch", "GRT_SCRATCH_LEVEL_PARTIALS", "lw", "fused", "sub-S1-profile sky-profile-S3 zeniths-Z5-profile",
        fixed="fixed: [max_cols][2 V][nblocks]"),
    row("scratch", "GRT_SCRATCH_LEVEL_PARTIALS", "sw", "fused", "sub-S1-profile sky-profile-S3",
        fixed="fixed: [max_cols][2 V][nblocks] (under sun angles the shortwave's levels go to GRT_SCRATCH_ZEN_PARTIALS)"),
    # 4 L n + 3 x objects x max_cols L n: the aerosol alone 3 arrays, liquid and ice 6, all three 9
    row("scratch", "GRT_SCRATCH_SPREAD", "both", "mat", "sub-S1-six sky-six-c1 sky-zeniths-Z1-S1 radiances-A1-c1",
        "sky-six-S1 radiances-A5-S3"),
    row("scratch", "GRT_SCRATCH_BIN_PARTIALS", "both", "both", "spectral-bins", "band-profiles"),
    row("scratch", "GRT_SCRATCH_SUB_PARTIALS", "lw", "fused", "sub-S1-six sky-six-S3 radiances-A5-S3 sky-zeniths-Z5-S3-profile",
        "sub-S3-six-two-sweeps sub-S3-profile sky-profile-S3"),
    row("scratch", "GRT_SCRATCH_SUB_PARTIALS", "sw", "fused", "sub-S1-six sky-six-S3 radiances-A5-S3",
        "sub-S3-six-two-sweeps sub-S3-profile sky-profile-S3"),
    row("scratch", "GRT_SCRATCH_FLUX_SUM", "lw", "mat", "sub-S1-six sky-six-S3 radiances-A5-S3 sky-zeniths-Z5-S3-profile",
        fixed="fixed: [2][max_cols][V][n]"),
    row("scratch", "GRT_SCRATCH_FLUX_SUM", "sw", "mat", "sub-S1-six sky-six-S3 radiances-A5-S3",
        fixed="fixed: [2][max_cols][V][n]"),
    row("scratch", "GRT_SCRATCH_SURF_ROWS", "lw", "both", "surface-emissivity", fixed="fixed: [max_cols][n]"),
    row("scratch", "GRT_SCRATCH_SURF_ROWS", "sw", "both", "surface-all", fixed="fixed: [max_cols][n]"),
    row("scratch", "GRT_SCRATCH_SURF_ROWS_DIF", "sw", "both", "surface-all", fixed="fixed: [max_cols][n]"),
    row("scratch", "GRT_SCRATCH_ZEN_PARTIALS", "sw", "both", "zeniths-Z1-c1",
        "zeniths-Z5 zeniths-Z5-profile sky-zeniths-Z5-S3-profile"),
    row("scratch", "GRT_SCRATCH_DIRECT_PARTIALS", "sw", "fused", "direct-six-S1", "direct-profile-S3"),
    row("scratch", "GRT_SCRATCH_DIRECT_PARTIALS", "lw", "fused", "jacobian-six-S1", "jacobian-profile-S3"),
    row("scratch", "GRT_SCRATCH_DIRECT_BEAM", "sw", "mat", "direct-six-S1 zen-direct-Z1",
        fixed="fixed: [max_cols][V][n] at both call sites (direct_rows_d points into it)"),
    row("scratch", "GRT_SCRATCH_DIRECT_BEAM", "lw", "mat", "jacobian-six-S1", fixed="fixed: [max_cols][V][n]"),
    row("scratch", "GRT_SCRATCH_DIRECT_SUM", "sw", "mat", "direct-profile-S3", fixed="fixed: [max_cols][V][n]"),
    row("scratch", "GRT_SCRATCH_DIRECT_SUM", "lw", "mat", "jacobian-profile-S3", fixed="fixed: [max_cols][V][n]"),
    row("scratch", "GRT_SCRATCH_DIRECT_LEVELS", "sw", "both", "direct-own-levels weighted-R1-S1 zen-own-levels-Z1",
        fixed="fixed: [max_cols][GRT_SKY_MAX_SETS][V] for its three users"),
    row("scratch", "GRT_SCRATCH_DIRECT_LEVELS", "lw", "both", "jacobian-own-levels",
        fixed="fixed: [max_cols][GRT_SKY_MAX_SETS][V]"),
    row("scratch", "GRT_SCRATCH_RADIANCE_PARTIALS", "lw", "both", "radiances-A1-c1", "radiances-A5-S3"),
    row("scratch", "GRT_SCRATCH_CHANNEL_PARTIALS", "lw", "both", "channels-C1-A1", "channels-C9-A5-S3"),
    row("scratch", "GRT_SCRATCH_WEIGHTING_PARTIALS", "lw", "both", "weighting-C1-A1-trans", "weighting-C9-A5-S3"),
    row("scratch", "GRT_SCRATCH_KDIST_MAP", "both", "both", "kdist-corr-scratch",
        fixed="fixed: [max_cols][n] unsigned shorts for both entry points"),
    row("scratch", "GRT_SCRATCH_CK_WEIGHT", "both", "both", "ck-own-sums-K2-b1", "ck-own-sums-K65-b5"),
    row("scratch", "GRT_SCRATCH_CK_TAU", "both", "both", "ck-own-sums-K2-b1", "ck-own-sums-K65-b5"),
    row("scratch", "GRT_SCRATCH_CK_SOURCE", "both", "both", "ck-own-sums-K2-b1", "ck-own-sums-K65-b5"),
    row("scratch", "GRT_SCRATCH_TILE_ROWS", "both", "both", "tiles-T1-c1", "tiles-T5-S3"),
    row("scratch", "GRT_SCRATCH_TILE_ROWS_DIF", "sw", "both", "tiles-T1-c1", "tiles-T5-S3"),
    row("scratch", "GRT_SCRATCH_TILE_PARTIALS", "both", "both", "tiles-T1-c1", "tiles-T5-S3"),
    row("scratch", "GRT_SCRATCH_RESPONSE_PARTIALS", "both", "both", "weighted-R1-S1", "weighted-R5-S3"),
    row("scratch", "GRT_SCRATCH_SCATTER_PARK", "lw", "both", "scatter-six-S1",
        fixed="fixed: grt_scatter_park_doubles(max_cols, V, n)"),
    row("scratch", "GRT_SCRATCH_SCATTER_PARTIALS", "lw", "both", "scatter-six-S1", "scatter-profile-S3"),
    row("scratch", "GRT_SCRATCH_SCATTER_LEVELS", "lw", "both", "scatter-own-levels",
        fixed="fixed: [max_cols][GRT_SKY_MAX_SETS][2][V]"),
    row("scratch", "GRT_SCRATCH_ZEN_DIRECT_PARTIALS", "sw", "both", "zen-direct-Z1", "zen-direct-Z5-S3-profile-surface"),
    row("scratch", "GRT_SCRATCH_ZEN_DIRECT_LEVELS", "sw", "both", "zen-own-levels-Z1", "zen-own-levels-Z5"),
    row("scratch", "GRT_SCRATCH_ZEN_SURF_ROWS", "sw", "mat", "zen-surface-Z1-knots2", fixed="fixed: [2][max_cols][n]"),
    row("scratch", "GRT_SCRATCH_ZEN_SLANT", "sw", "fused", "slant-Z1", "slant-Z5-S3-profile-surface"),
    row("staging", "small", "-", "both", CREATION, fixed="fixed: the per-column inputs of max_cols columns, reserved at creation"),
    row("staging", "cloud", "-", "both", CLOUD_FIRST + " tiles-T5-S3", CLOUD_MORE),
    row("staging", "aer", "-", "both", AEROSOL_FIRST + " tiles-T5-S3", "sky-six-S1"),
    row("staging", "surf", "-", "both", "surface-emissivity", "surface-all"),
    row("staging", "zen", "-", "both", "zeniths-Z1-c1", fixed="fixed: 3 max_cols GRT_MAX_ZENITHS"),
    row("staging", "rad", "-", "both", "radiances-A1-c1", fixed="fixed: max_cols GRT_MAX_VIEW_ANGLES"),
    row("staging", "tile", "-", "both", "tiles-T1-c1", "tiles-T5-S3"),
    row("staging", "zen_surf", "-", "both", "zen-surface-Z1-knots2", "zen-direct-Z5-S3-profile-surface"),
    row("table", "cloud_map", "both", "both", CLOUD_FIRST + " tiles-T5-S3",
        fixed="fixed: the family passes use one parametrisation (6 liquid, 8 ice bands); test_keyed_tables changes it"),
    row("table", "aer_map", "both", "both", AEROSOL_FIRST + " tiles-T5-S3", "sky-six-S1"),
    row("table", "bin_table", "both", "both", "spectral-bins", "band-profiles"),
    row("table", "kdist_table", "both", "both", "kdist-K2-b1",
        "kdist-K65-b5-weight kdist-corr-kept ck-K2-b1 ck-K65-b5-kept ck-own-sums-K2-b1 ck-own-sums-K65-b5"),
    row("table", "surf_map", "lw", "both", "surface-emissivity",
        fixed="fixed: the family passes use one emissivity grid; test_keyed_tables changes it"),
    row("table", "surf_map", "sw", "both", "surface-all",
        fixed="fixed: the family passes use one albedo grid; test_keyed_tables changes it"),
    row("table", "channel_table", "lw", "both", "channels-C1-A1", "channels-C9-A5-S3 weighting-C1-A1-trans weighting-C9-A5-S3"),
    row("table", "tile_map", "both", "both", "tiles-T1-c1",
        fixed="fixed: the family passes use one pair of tile grids; test_keyed_tables changes it"),
    row("table", "response_table", "both", "both", "weighted-R1-S1", "weighted-R5-S3"),
    row("table", "zen_surf_map", "sw", "both", "zen-surface-Z1-knots2", "zen-direct-Z5-S3-profile-surface"),
]


def test_coverage_table_names_exactly_what_the_header_declares():
    scratch, staging, keyed = header_names()
    assert scratch and len(set(scratch)) == len(scratch) and staging and keyed
    for kind, names in (("scratch", scratch), ("staging", staging), ("table", keyed)):
        have = {r["name"] for r in COVERAGE if r["kind"] == kind}
        assert have == set(names), (kind, "missing", sorted(set(names) - have), "extra", sorted(have - set(names)))
    for r in COVERAGE:
        what = (r["name"], r["bands"], r["forms"])
        assert r["kind"] in ("scratch", "staging", "table") and r["forms"] in ("fused", "mat", "both"), what
        assert r["bands"] in (("-",) if r["kind"] == "staging" else ("lw", "sw", "both")), what
        assert r["appears"], what
        assert set(r["appears"]) | set(r["grows"]) <= ALL_STEPS | {CREATION}, what
        # a step, or "fixed" and its reason -- never both, never neither
        assert bool(r["grows"]) != bool(r["fixed"]), what
        assert not r["fixed"] or (r["fixed"].startswith("fixed: ") and len(r["fixed"]) > 12), what
        if r["forms"] != "both":
            assert not set(r["appears"]) & FUSED_ONLY or r["forms"] == "fused", what
    # no (name, band, form) is spoken of twice
    seen = set()
    for r in COVERAGE:
        for b in (("lw", "sw") if r["bands"] == "both" else (r["bands"],)):
            for f in (("fused", "mat") if r["forms"] == "both" else (r["forms"],)):
                assert (r["kind"], r["name"], b, f) not in seen, (r["name"], b, f)
                seen.add((r["kind"], r["name"], b, f))


# ---- what an object holds ------------------------------------------------------------------------------------------------ #
def holdings(pipe):
    """{(kind, name, band): capacity or key length}: api.Pipeline.holdings() under the header's names."""
    scratch, staging, keyed = header_names()
    s, g, k = pipe.holdings()
    assert s.shape == (2, len(scratch)) and g.shape == (len(staging),) and k.shape == (2, len(keyed)), (s.shape, g.shape, k.shape)
    out = {}
    for bi, b in enumerate(("lw", "sw")):
        out.update({("scratch", name, b): int(s[bi, j]) for j, name in enumerate(scratch)})
        out.update({("table", name, b): int(k[bi, j]) for j, name in enumerate(keyed)})
    out.update({("staging", name, "-"): int(g[j]) for j, name in enumerate(staging)})
    return out


def covered(key, form):
    """The table's word on one (kind, name, band) in one pipeline form: (appears, grows, fixed), or None: the table says
    that this form, or this band, never has it."""
    for r in COVERAGE:
        if (r["kind"], r["name"]) == key[:2] and r["bands"] in (key[2], "both", "-") and r["forms"] in (form, "both"):
            return set(r["appears"]), set(r["grows"]), bool(r["fixed"])
    return None


def judge(step, form, before, after, strict):
    """What the table does not allow in the move from `before` to `after` over one step.  strict (a family's own pass):
    a slot marked as appearing went 0 -> x, one marked as growing went x -> y > x (a key: to another length), a fixed one
    kept its size, nothing else moved.  Not strict (families interleaved: which of a slot's steps comes first differs): a
    slot moves only at a step the table names for it, appears at the first of its steps, and a fixed one never moves."""
    problems = []
    for key in sorted(after):
        b, a = before[key], after[key]
        word = covered(key, form)
        if word is None:
            if a != 0:
                problems.append((step, key, b, a, "the table says this form or band never has it"))
            continue
        appears, grows, fixed = word
        smaller = a < b and key[0] != "table"
        if a != b:
            if smaller:
                problems.append((step, key, b, a, "shrank"))
            elif b == 0 and step not in appears and (strict or step not in grows):
                problems.append((step, key, b, a, "appeared at a step the table does not name for it"))
            elif b > 0 and fixed:
                problems.append((step, key, b, a, "a fixed size moved"))
            elif b > 0 and step not in grows and (strict or step not in appears):
                problems.append((step, key, b, a, "moved at a step the table does not name for it"))
        else:
            if b == 0 and step in appears:
                problems.append((step, key, b, a, "did not appear"))
            elif strict and step in grows:
                problems.append((step, key, b, a, "did not move"))
    return problems


def same_capacities(a, b):
    """the scratch and staging capacities (a key's length follows the last call's key)"""
    return {k: v for k, v in a.items() if k[0] != "table"} == {k: v for k, v in b.items() if k[0] != "table"}


# ---- the inputs ------------------------------------------------------------------------------------------------------------ #
class World:
    """The batch every step draws on: test_gpu_sky_zeniths_direct.py's Case at this module's shape (columns, surface, three
    cloud draws, aerosols, per-angle knots), test_gpu_pipeline_tiles.py's tiles on the same columns, the cloud sampler, and
    the same inputs cut down to one column, one draw and a two-point aerosol grid."""

    def __init__(self, bands, tables, lib, device):
        self.lib, self.device, self.tables = lib, device, tables
        self.case = Case(bands, tables, device, N, V, Z5, S3, NK, ncol=NCOL)
        x = self.x = self.case.x
        self.xt = TileInputs(bands, tables, device, lib, N, V, S3, T5, "free", (3, 4), ncol=NCOL)
        for k in SETS:
            assert np.array_equal(self.xt.cl[k], x.cl[k])           # (the same columns, clouds and aerosols)
        self.keep = []
        self.gcols = {NCOL: x.gcols, 1: self.held(api.make_columns(x.cols[:1], MOL_ORDER, cfc_order=(0, 1)))}
        self._clouds, self._aer = {}, {}
        self.small_x = tuple(np.array([g[0], g[-1]]) for g in x.xs)
        self.small_f = tuple(aerosol_fields(1, L, g, 70 + bi, lw=bi == 0) for bi, g in enumerate(self.small_x))
        gm = self.held(api.make_cloud_model(tables))
        self.sampler = api.CloudSampler(device, gm)
        self.fields = pipeline_fields(x.cols, 61)
        self.mu = {Z: angles(NCOL, Z, "none", ZN) for Z in (1, Z5)}
        self.sec = {A: secants_of(NCOL, A) for A in (1, A5)}

    def held(self, pair):
        self.keep.append(pair)
        return pair[0]

    def gclouds(self, ncol, S):
        if (ncol, S) not in self._clouds:
            self._clouds[ncol, S] = self.held(make(self.tables, pick(self.x.cl, columns=range(ncol), subcolumns=range(S))))
        return self._clouds[ncol, S]

    def gaer(self, ncol, small=False):
        if (ncol, small) not in self._aer:
            self._aer[ncol, small] = self.held(aerosols_of(self.small_f, self.small_x) if small else
                                               aerosols_of(tuple(f[:ncol] for f in self.x.f), self.x.xs))
        return self._aer[ncol, small]

    def view(self, ncol, S):
        """x with ncol columns and S draws, for the helpers that read their inputs from it"""
        v = copy.copy(self.x)
        v.ncol, v.S, v.cols = ncol, S, self.x.cols[:ncol]
        v.gcols, v.gclouds, v.gaer = self.gcols[ncol], self.gclouds(ncol, S), self.gaer(ncol)
        return v

    def create(self, spectral, max_columns=NCOL):
        x = self.x
        return api.Pipeline(x.go_lw, x.go_sw, max_columns, USER_LEVEL, x.emis, x.alb, x.solar, spectral=spectral)

    def destroy(self):
        self.sampler.destroy()
        self.x.destroy()
        self.xt.destroy()


@pytest.fixture(scope="module")
def world(bands, tables, lib, device):
    w = World(bands, tables, lib, device)
    yield w
    w.destroy()


def stacked(per_set):
    return {k: np.stack([s[k] for s in per_set], axis=1) for k in per_set[0]}


# ---- the steps ------------------------------------------------------------------------------------------------------------- #
def base_steps(w, monkeypatch):
    g2 = w.gcols[NCOL]
    rng = np.random.default_rng(23)
    e_x, a_x = np.array([50.0, 120.0, 240.0]), np.array([1100.0, 1900.0, 2500.0, 3400.0])
    surf_emis = w.held(api.make_surface(NCOL, emissivity=(e_x, rng.uniform(0.5, 1.0, (NCOL, 3)))))
    surf_all = w.held(api.make_surface(NCOL, emissivity=(e_x, rng.uniform(0.5, 1.0, (NCOL, 3))),
                                       albedo=(a_x, rng.uniform(0.0, 0.6, (NCOL, 4)), rng.uniform(0.0, 0.6, (NCOL, 4)))))
    few = dict(lw_edges=[0, 100, N - 1], sw_edges=[0, N - 1])
    more = dict(lw_edges=[0, 1, 127, 128, 129, 200, N - 1], sw_edges=[3, 64, 128, 192, 250])

    def subcolumns(S, profile, two_sweeps=False):
        def step(pipe):
            if two_sweeps:
                monkeypatch.setenv("GRT_SW_TWO_SWEEPS", "1")
            try:
                pipe.run_subcolumns(g2, w.gclouds(NCOL, S), S, profiles=profile)
            finally:
                monkeypatch.delenv("GRT_SW_TWO_SWEEPS", raising=False)
            return flat(*(pipe.subcolumn_profiles(NCOL) if profile else pipe.subcolumn_fluxes(NCOL)))
        return step

    def aerosols(pipe):
        pipe.run_aerosols(g2, w.gaer(NCOL))
        return flat(*pipe.aerosol_fluxes(NCOL))

    def allsky(pipe):
        pipe.run_allsky(g2, w.gclouds(NCOL, 1))
        return flat(*pipe.allsky_fluxes(NCOL))

    def spectral_bins(pipe):
        pipe.run_spectral(g2, None, **few)
        return pipe.spectral(NCOL)

    def band_profiles(pipe):
        pipe.run_band_profiles(g2, w.gclouds(NCOL, 1), **more)
        return pipe.band_profiles(NCOL)

    def surface(gsurface):
        def step(pipe):
            pipe.set_surface(gsurface)
            pipe.run(g2)
            out = {"fluxes": pipe.fluxes(NCOL)}
            pipe.set_surface(None)
            return out
        return step

    return [subcolumns(1, False), subcolumns(3, False, two_sweeps=True), subcolumns(1, True), subcolumns(3, True), aerosols,
            allsky, spectral_bins, band_profiles, surface(surf_emis), surface(surf_all)]


def several_responses(seed):
    """test_gpu_pipeline_weighted.py's five on this grid: all ones on the whole grid (it overlaps every other), a Gaussian and
    a box across a block's edge, a single point, random weights of both signs up to the last point."""
    rng = np.random.default_rng(seed)
    x = np.arange(-45, 46)
    weights = [np.ones(N), 3.0 * np.exp(-0.5 * (x / 15.0) ** 2), np.ones(16), np.array([0.7]), rng.uniform(-1.0, 2.0, 77)]
    first = [0, N // 2 - 45, 120, 200, N - 77]
    assert all(f + r.size <= N for f, r in zip(first, weights))
    return first, weights


def sky_steps(w):
    lib = w.lib

    def sky_out(pipe, ncol, nsets, profiles):
        return pipe.sky_profiles(ncol, nsets) if profiles else dict(fluxes=pipe.sky_fluxes(ncol, nsets))

    def sky(ncol, S, sets, profiles, small=False):
        def step(pipe):
            return run_sky(pipe, w.gcols[ncol], w.gclouds(ncol, S), w.gaer(ncol, small), S, sets, ncol, profiles)
        return step

    def third(which, S, profiles, own=False):
        """run_sky_direct or run_sky_jacobian; own: the profile form without the levels output, the three rows alone"""
        def step(pipe):
            gsky, keep = api.make_sky(w.gclouds(NCOL, S), w.gaer(NCOL), S, ALL)
            nsets = keep["nsets"]
            if not own:
                getattr(pipe, "run_sky_" + which)(w.gcols[NCOL], gsky, profiles=profiles)
                extra = getattr(pipe, f"sky_{which}_profiles" if profiles else f"sky_{which}_fluxes")(NCOL, nsets)
                return dict(sky_out(pipe, NCOL, nsets, profiles), **(extra if profiles else {which: extra}))
            ptrs, _ = pipe._sky_ptrs(gsky, True)
            three = pipe._buffer(f"sky_profiles.{which}", 8 * pipe.max_columns * nsets * 3)
            struct = (api.GrtDirectBeam if which == "direct" else api.GrtSurfaceJacobian)(three.ptr, None)
            api.check(getattr(lib, "grt_pipeline_run_sky_" + which)(pipe.p, C.byref(w.gcols[NCOL]), C.byref(gsky),
                                                                      C.byref(struct), *ptrs))
            out = sky_out(pipe, NCOL, nsets, True)
            out[which] = getattr(pipe, f"sky_{which}_fluxes")(NCOL, nsets, profiles=True)
            return out
        return step

    def scatter(S, profiles, own=False):
        def step(pipe):
            gsky, keep = api.make_sky(w.gclouds(NCOL, S), w.gaer(NCOL), S, ALL)
            nsets = keep["nsets"]
            if not own:
                pipe.run_sky_scattering(w.gcols[NCOL], gsky, profiles=profiles)
                extra = pipe.sky_scatter_profiles(NCOL, nsets) if profiles else dict(scatter=pipe.sky_scatter_fluxes(NCOL, nsets))
                return dict(sky_out(pipe, NCOL, nsets, profiles), **extra)
            ptrs, _ = pipe._sky_ptrs(gsky, True)
            six = pipe._buffer("sky_profiles.scatter", 8 * pipe.max_columns * nsets * 6)
            api.check(lib.grt_pipeline_run_sky_scattering(pipe.p, C.byref(w.gcols[NCOL]), C.byref(gsky), *ptrs, None, six.ptr))
            return dict(sky_out(pipe, NCOL, nsets, True), scatter=pipe.sky_scatter_fluxes(NCOL, nsets, profiles=True))
        return step

    def weighted(S, resp):
        def step(pipe):
            prof, wt = run_weighted(pipe, w.gcols[NCOL], w.gclouds(NCOL, S), w.gaer(NCOL), S, ALL, NCOL, resp[0], resp[1])
            return dict(prof, **wt)
        return step

    def cloud_fields(S, profiles):
        f = w.fields

        def step(pipe):
            gf, keep = api.make_cloud_fields(f["cf"], f["lwc"], f["iwc"], f["ov"], temperature=f["t"], thickness=f["th"],
                                             num_subcolumns=S, seed=99, column_offset=17)
            pipe.run_cloud_fields(w.gcols[NCOL], w.sampler, gf, profiles=profiles)
            return flat(*(pipe.subcolumn_profiles(NCOL) if profiles else pipe.subcolumn_fluxes(NCOL)))
        return step

    one = [([100], [np.linspace(0.5, 2.0, 40)])] * 2                # one response a band, across a block's edge
    w.five = [several_responses(5 + bi) for bi in range(2)]
    return [sky(1, 1, AEROSOL, False, small=True), sky(NCOL, 1, ALL, False), sky(NCOL, 3, ALL, False), sky(NCOL, 3, ALL, True),
            third("direct", 1, False), third("direct", 3, True), third("direct", 1, True, own=True),
            third("jacobian", 1, False), third("jacobian", 3, True), third("jacobian", 1, True, own=True),
            scatter(1, False), scatter(3, True), scatter(1, True, own=True), weighted(1, one), weighted(3, w.five),
            cloud_fields(1, False), cloud_fields(3, True)]


def zenith_steps(w):
    lib, case = w.lib, w.case
    xa2, knots2 = case.xa[:2], np.ascontiguousarray(case.knots[:, :1, :2])
    surf2 = w.held(api.make_zenith_surface(xa2, knots2))
    # (the staging buffer of the per-angle knots is reserved for GRT_MAX_ZENITHS angles: only many more knots outgrow it)
    xa40 = np.linspace(case.xa[0], case.xa[-1], 40)
    surf40 = w.held(api.make_zenith_surface(xa40, np.random.default_rng(41).uniform(0.02, 0.9, (NCOL, Z5, xa40.size))))
    w.cosines = {Z: drawn(w.mu[Z], L, 3 * N + Z) for Z in (1, Z5)}

    def zeniths(ncol, Z, profiles):
        def step(pipe):
            gz, keep = api.make_zeniths(w.mu[Z][:ncol])
            pipe.run_zeniths(w.gcols[ncol], gz, profiles=profiles)
            if profiles:
                return pipe.zenith_profiles(ncol, Z)
            fluxes, per_angle = pipe.zenith_fluxes(ncol, Z)
            return dict(fluxes=fluxes, angle_fluxes=per_angle)
        return step

    def sky_zeniths(Z, S, profiles):
        def step(pipe):
            return run_sky_zeniths(pipe, w.gcols[NCOL], w.gclouds(NCOL, S), w.gaer(NCOL), S, ALL, w.mu[Z], None, NCOL, profiles)
        return step

    def direct(Z, S, gsurf, profiles):
        def step(pipe):
            return run_zd(pipe, w.view(NCOL, S), ALL, w.mu[Z], None, gsurf, True, profiles)
        return step

    def own_levels(Z):
        """the profile form with every angle's three rows and their mean, and neither levels output"""
        def step(pipe):
            gsky, keep = api.make_sky(w.gclouds(NCOL, 1), w.gaer(NCOL), 1, ALL)
            gz, keep_z = api.make_zeniths(w.mu[Z])
            gdirect, ptrs = pipe._zenith_direct_outputs(gsky, gz, True, True)
            gdirect.direct_level_fluxes_dev, gdirect.zenith_direct_level_fluxes_dev = None, None
            api.check(lib.grt_pipeline_run_sky_zeniths_direct(pipe.p, C.byref(w.gcols[NCOL]), C.byref(gsky), C.byref(gz), None,
                                                              C.byref(gdirect), *ptrs))
            name, nsets = "sky_zenith_direct_profiles", keep["nsets"]
            out = stacked(pipe._read_profiles(name, nsets, NCOL))
            out["direct"] = pipe.buffers[name + ".direct"].to_host((NCOL, nsets, 3))
            out["angle_direct"] = pipe.buffers[name + ".angle_direct"].to_host((NCOL, nsets, Z, 3))
            out["angle_fluxes"] = pipe.buffers[name + ".angles"].to_host((NCOL, nsets, Z, 6))
            return out
        return step

    def slant(Z, S, gsurf, profiles):
        def step(pipe):
            return run_zs(pipe, w.view(NCOL, S), ALL, w.mu[Z], None, w.cosines[Z], gsurf, True, profiles)
        return step

    def tiles(ncol, T, S, sets):
        def step(pipe):
            gt, keep = w.xt.gtiles(order=range(T), columns_=range(ncol))
            return run_sky_tiles(pipe, w.gcols[ncol], w.gclouds(ncol, S), w.gaer(ncol), S, sets, gt, ncol)
        return step

    return [zeniths(1, 1, False), zeniths(NCOL, Z5, False), zeniths(NCOL, Z5, True), sky_zeniths(1, 1, False),
            sky_zeniths(Z5, 3, True), direct(1, 1, None, False), direct(1, 1, surf2, False), direct(Z5, 3, surf40, True),
            own_levels(1), own_levels(Z5), slant(1, 1, None, False), slant(Z5, 3, surf40, True), tiles(1, 1, 1, CLEAN),
            tiles(NCOL, T5, 3, ALL)]


def radiance_steps(w):
    band = w.x.lwb
    w.one_channel = Instrument([100], [np.linspace(0.5, 2.0, 40)])           # across a block's edge
    w.channels = edge_instrument(N, band.dw, False, True)[0]                  # several that overlap, one the whole grid
    assert w.channels.C >= 9

    def radiances(ncol, A, S, sets, points, fluxes=True):
        def step(pipe):
            return run_rad(pipe, w.gcols[ncol], w.gclouds(ncol, S), w.gaer(ncol), S, sets, ncol, w.sec[A][:ncol],
                           spectral=points, bright=points, fluxes=fluxes)
        return step

    def channels(A, S, inst):
        def step(pipe):
            return run_chan(pipe, w.gcols[NCOL], w.gclouds(NCOL, S), w.gaer(NCOL), S, ALL, NCOL, w.sec[A], inst)
        return step

    def weighting(A, S, inst, contribution):
        def step(pipe):
            return run_wt(pipe, w.gcols[NCOL], w.gclouds(NCOL, S), w.gaer(NCOL), S, ALL, NCOL, w.sec[A], inst,
                          contribution=contribution)
        return step

    return [radiances(1, 1, 1, AEROSOL, True), radiances(NCOL, A5, 3, ALL, False), radiances(NCOL, A5, 3, ALL, False, fluxes=False),
            channels(1, 1, w.one_channel), channels(A5, 3, w.channels), weighting(1, 1, w.one_channel, False),
            weighting(A5, 3, w.channels, True)]


CK_SMALL = dict(class_edges=np.array([1e-2]), lw_edges=[0, N - 1], sw_edges=[3, 250])
CK_LARGE = dict(class_edges=np.logspace(-6.0, 2.0, 64), lw_edges=[0, 1, 127, 128, 200, N - 1], sw_edges=[3, 64, 128, 129, 192, 250])


def dropped(out):
    """a run's nested dict as one flat dict, what the call did not write left out"""
    return {f"{b}.{k}": a for b, d in out.items() for k, a in d.items() if a is not None}


def kdist_steps(w):
    lib = w.lib
    g2 = w.gcols[NCOL]
    weight = (np.linspace(0.5, 1.5, N), np.linspace(2.0, 0.25, N))

    def kdist(args, weights=(None, None)):
        def step(pipe):
            pipe.run_kdist(g2, args["class_edges"], lw_edges=args["lw_edges"], sw_edges=args["sw_edges"], lw_weight=weights[0],
                           sw_weight=weights[1])
            return dropped(pipe.kdist(NCOL))
        return step

    def correlated(keep_map):
        def step(pipe):
            pipe.run_kdist_correlated(g2, CK_LARGE["class_edges"], lw_edges=CK_LARGE["lw_edges"], sw_edges=CK_LARGE["sw_edges"],
                                      lw_key=("sum",), sw_key=("layer", V - 2), keep_map=keep_map)
            return dropped(pipe.kdist_correlated(NCOL))
        return step

    def ck(args, keep_map):
        def step(pipe):
            pipe.run_ck_fluxes(g2, args["class_edges"], lw_edges=args["lw_edges"], sw_edges=args["sw_edges"], lw_key=("sum",),
                               sw_key=("layer", V - 2), keep_map=keep_map)
            return dropped(pipe.ck_fluxes(NCOL))
        return step

    def ck_own_sums(args):
        """the call without the weight, tau and source outputs: the class sums stay in pipeline scratch"""
        def step(pipe):
            ce = np.ascontiguousarray(args["class_edges"], dtype=np.float64)
            K = ce.size + 1
            gk = api.GrtCkFluxes()
            gk.num_classes, gk.class_edges = K, ce.ctypes.data_as(api.c_double_p)
            keep, shapes = [], {}
            for name, b, edges, key in (("lw", gk.lw, args["lw_edges"], (api.KDIST_KEY_SUM, 0)),
                                        ("sw", gk.sw, args["sw_edges"], (api.KDIST_KEY_ROW, V - 2))):
                e = np.ascontiguousarray(edges, dtype=np.int32)
                keep.append(e)
                b.edges, b.num_bins = e.ctypes.data_as(api.c_int_p), e.size - 1
                b.key.kind, b.key.layer = key
                count = pipe.max_columns * b.num_bins * K
                b.flux_up_dev = pipe._buffer(f"own.{name}.up", 8 * count * V).ptr
                b.flux_down_dev = pipe._buffer(f"own.{name}.down", 8 * count * V).ptr
                b.bin_up_dev = pipe._buffer(f"own.{name}.bin_up", 8 * pipe.max_columns * b.num_bins * V).ptr
                b.bin_down_dev = pipe._buffer(f"own.{name}.bin_down", 8 * pipe.max_columns * b.num_bins * V).ptr
                shapes[name] = {"up": (NCOL, V, b.num_bins, K), "down": (NCOL, V, b.num_bins, K),
                                "bin_up": (NCOL, V, b.num_bins), "bin_down": (NCOL, V, b.num_bins)}
            api.check(lib.grt_pipeline_run_ck_fluxes(pipe.p, C.byref(g2), C.byref(gk)))
            pipe.sync()
            return {f"{name}.{k}": pipe.buffers[f"own.{name}.{k}"].to_host(sh) for name, d in shapes.items() for k, sh in d.items()}
        return step

    return [kdist(CK_SMALL), kdist(CK_LARGE, weight), correlated(True), correlated(False), ck(CK_SMALL, False), ck(CK_LARGE, True),
            ck_own_sums(CK_SMALL), ck_own_sums(CK_LARGE)]


def steps_of(w, family, monkeypatch, form):
    made = {"base": lambda: base_steps(w, monkeypatch), "sky": lambda: sky_steps(w), "zeniths": lambda: zenith_steps(w),
            "radiances": lambda: radiance_steps(w), "kdist": lambda: kdist_steps(w)}[family]()
    assert len(made) == len(FAMILIES[family])
    return [(name, step) for name, step in zip(FAMILIES[family], made) if form == "fused" or name not in FUSED_ONLY]


# ---- the passes ------------------------------------------------------------------------------------------------------------- #
def compare(got, want, what):
    assert got.keys() == want.keys() and len(got) > 0, (what, sorted(got), sorted(want))
    for key in got:
        assert got[key].size > 0 and np.all(np.isfinite(got[key])), (what, key)
        assert np.array_equal(got[key], want[key]), (what, key)


def history(w, spectral, steps, strict):
    """The growing pass and the reverse pass of `steps` on one live object -> (the object, every step's recorded result).
    The caller holds the grown object to its references and destroys it."""
    form = "mat" if spectral else "fused"
    pipe = w.create(spectral)
    held = holdings(pipe)
    for key, v in held.items():
        assert (v > 0) == (key[:2] == ("staging", "small")), ("at creation", key, v)
    want, problems, moves = {}, [], []
    for name, step in steps:                            # every buffer appears, then is replaced by a larger one
        fresh = w.create(spectral)
        want[name] = step(fresh)
        fresh.destroy()
        compare(step(pipe), want[name], ("growing", form, name))
        now = holdings(pipe)
        moves += [(name, key, held[key], now[key]) for key in sorted(now) if now[key] != held[key]]
        problems += judge(name, form, held, now, strict)
        held = now
    for m in moves:
        print(form, *m)
    assert not problems, problems
    for name, step in reversed(steps):                  # every buffer is large enough already and is reused
        compare(step(pipe), want[name], ("reverse", form, name))
        assert same_capacities(holdings(pipe), held), ("reverse", form, name)
    # the steps are not one another's: a wrong placement that gave every call the same rows would pass the above
    names = [name for name, _ in steps]
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            if frozenset((a, b)) in SAME_CALL:
                continue
            if {k: v.shape for k, v in want[a].items()} == {k: v.shape for k, v in want[b].items()}:
                assert any(not np.array_equal(want[a][k], want[b][k]) for k in want[a]), (a, b)
    return pipe, want, held


def every_slot_of_the_form_appeared(held, form, names):
    """the table's lines of this form whose steps ran: all of them hold something now"""
    for key, v in held.items():
        word = covered(key, form)
        if word is not None and word[0] & (set(names) | {CREATION}):
            assert v > 0, (form, key)


FORMS = pytest.mark.parametrize("spectral", [False, True], ids=["fused", "mat"])


@pytest.mark.gpu
@FORMS
def test_base_family(world, lib, monkeypatch, spectral):
    form = "mat" if spectral else "fused"
    steps = steps_of(world, "base", monkeypatch, form)
    _deterministic(lib, True)
    try:
        pipe, want, held = history(world, spectral, steps, True)
        every_slot_of_the_form_appeared(held, form, FAMILIES["base"])
        pipe.destroy()
    finally:
        _deterministic(lib, False)


# ---- ground truth, one call per family on the grown object ---------------------------------------------------------------- #
def sky_truth(w, pipe, oracle):
    """run_sky_weighted, all four sets of three draws: the weighted rows against response_model on the oracle's spectra, and
    the call's own level rows against the same spectra under the trapezoid's weights"""
    x = w.x
    prof, wt = run_weighted(pipe, x.gcols, x.gclouds, x.gaer, S3, ALL, NCOL, w.five[0], w.five[1])
    for bi, (band, key, lw) in enumerate(((x.lwb, "lw", True), (x.swb, "sw", False))):
        for c, col in enumerate(x.cols):
            spectra = oracle_spectral_sets(oracle, w.lib, band, col, lw, w.tables, x.cl[key + "_liquid"][c], x.cl[key + "_ice"][c],
                                           x.cl["thickness"][c], x.xs[bi], x.f[bi][c], x.emis, x.alb, x.solar)
            for k in range(4):
                check_against_model(wt, c, k, key, band, col, spectra[k], w.five[bi], WEIGHTED_TOL, 0.0, "history")
                whole = weighted_set({q: spectra[k][q] for q in ("up", "dn")}, band.dw, [0], [np.ones(band.nw)])
                ff = max(np.abs(whole["up"]).max(), np.abs(whole["dn"]).max())
                for name, q in ((key + "_up", "up"), (key + "_down", "dn")):
                    err = np.max(np.abs(prof[name][c, k] - whole[q][0]))
                    assert err <= WEIGHTED_TOL * ff, (name, c, k, err, ff)


def zenith_truth(w, pipe, oracle, oracle_cache, spectral):
    """The per-angle rows and direct beam under Z5 angles, three draws and a per-angle albedo against slant_model fed by the
    oracle (fused form: cosines drawn per layer; materialised form: every layer at the angle's own, the plane-parallel
    call); every tile's rows against the oracle over the tile's surface."""
    x, mu = w.x, w.mu[Z5]
    if spectral:
        cosines = flat_cosines(mu, L)
        got = {p: run_zd(pipe, x, ALL, mu, None, w.case.gsurf, True, p) for p in (False, True)}
    else:
        cosines = w.cosines[Z5]
        got = {p: run_zs(pipe, x, ALL, mu, None, cosines, w.case.gsurf, True, p) for p in (False, True)}
    check_reference(oracle, w.lib, x, w.case, ALL, mu, cosines, True, USER_LEVEL, got[False], got[True], oracle=False)
    xt = w.xt
    tiles = xt.tiles(pipe, ALL)
    for c in range(NCOL):
        for at, name in enumerate(NAMES):
            for t in (0, T5 - 1):
                want, largest = xt.oracle_rows(oracle, oracle_cache, name, c, t, USER_LEVEL)
                for bi in (0, 1):
                    err = np.max(np.abs(tiles["tiles"][c, at, t, 6 * bi:6 * bi + 6] - want[6 * bi:6 * bi + 6]))
                    assert largest[bi] > 0.0 and err <= TILE_TOL * largest[bi], (c, name, t, bi, err, largest[bi])


def radiance_truth(w, pipe, oracle):
    """run_sky_channels at A5 angles, three draws, the overlapping instrument: the channel values against channel_model and
    the call's integrated radiances against radiance_model, both fed by the oracle"""
    x, inst, sec = w.x, w.channels, w.sec[A5]
    got = run_chan(pipe, x.gcols, x.gclouds, x.gaer, S3, ALL, NCOL, sec, inst)
    whole = [i for i, (f, wt) in enumerate(zip(inst.first, inst.weights)) if f == 0 and wt.size == N][0]
    for c, col in enumerate(x.cols):
        args = (oracle, w.lib, x.lwb, col, w.tables, x.cl["lw_liquid"][c], x.cl["lw_ice"][c], x.cl["thickness"][c], x.xs[0],
                x.f[0][c], x.emis, sec[c])
        want, rad = oracle_channel_sets(*args, inst.first, inst.weights), oracle_radiance_sets(*args)
        for k in range(4):
            check_model(got, c, k, want[k], inst, whole, x.lwb, "history")
            check_integrated(got, c, k, rad[k], x.lwb, "history")


def kdist_truth(w, pipe, oracle):
    """run_ck_fluxes with kept maps: the map against kdist_correlated_model, the class sums against it and ck_flux_model on
    the tau_gas the pipeline shows, the fluxes against ck_flux_model's solve of the device's own sums"""
    x = w.x
    k = object.__new__(CkCase)
    k.__dict__.update(bands=(x.lwb, x.swb), device=w.device, V=V, L=L, ncol=NCOL, cols=x.cols, emis=x.emis, alb=x.alb,
                      solar=x.solar)
    ce, K = CK_LARGE["class_edges"], CK_LARGE["class_edges"].size + 1
    pipe.run_ck_fluxes(x.gcols, ce, lw_edges=CK_LARGE["lw_edges"], sw_edges=CK_LARGE["sw_edges"], lw_key=("sum",),
                       sw_key=("layer", V - 2), keep_map=True)
    out = pipe.ck_fluxes(NCOL)
    for bi, name in enumerate(("lw", "sw")):
        edges = np.array(CK_LARGE[name + "_edges"], dtype=np.int32)
        m = class_map(k.tau_gas(pipe, bi), KEY_SUM if bi == 0 else KEY_ROW, ce, V - 2)
        assert np.array_equal(out[name]["map"], m), name
        assert_sums(k, out[name], bi, m, edges, K, pipe=pipe)
        assert_solve(k, oracle, out[name], bi)


@pytest.mark.gpu
@FORMS
def test_sky_family(world, oracle, lib, monkeypatch, spectral):
    form = "mat" if spectral else "fused"
    steps = steps_of(world, "sky", monkeypatch, form)
    _deterministic(lib, True)
    try:
        pipe, want, held = history(world, spectral, steps, True)
        every_slot_of_the_form_appeared(held, form, FAMILIES["sky"])
        sky_truth(world, pipe, oracle)
        assert same_capacities(holdings(pipe), held)
        pipe.destroy()
    finally:
        _deterministic(lib, False)


@pytest.mark.gpu
@FORMS
def test_sun_angles_and_tiles_family(world, oracle, oracle_cache, lib, monkeypatch, spectral):
    form = "mat" if spectral else "fused"
    steps = steps_of(world, "zeniths", monkeypatch, form)
    _deterministic(lib, True)
    try:
        pipe, want, held = history(world, spectral, steps, True)
        every_slot_of_the_form_appeared(held, form, FAMILIES["zeniths"])
        zenith_truth(world, pipe, oracle, oracle_cache, spectral)
        assert same_capacities(holdings(pipe), held)
        pipe.destroy()
    finally:
        _deterministic(lib, False)


@pytest.mark.gpu
@FORMS
def test_longwave_radiance_family(world, oracle, lib, monkeypatch, spectral):
    form = "mat" if spectral else "fused"
    steps = steps_of(world, "radiances", monkeypatch, form)
    _deterministic(lib, True)
    try:
        pipe, want, held = history(world, spectral, steps, True)
        every_slot_of_the_form_appeared(held, form, FAMILIES["radiances"])
        # without flux rows the radiance kernel stands in the solver's place: the same radiances
        assert np.array_equal(want["radiances-alone-A5-S3"]["radiances"], want["radiances-A5-S3"]["radiances"])
        radiance_truth(world, pipe, oracle)
        assert same_capacities(holdings(pipe), held)
        pipe.destroy()
    finally:
        _deterministic(lib, False)


@pytest.mark.gpu
@FORMS
def test_k_distribution_family(world, oracle, lib, monkeypatch, spectral):
    form = "mat" if spectral else "fused"
    steps = steps_of(world, "kdist", monkeypatch, form)
    _deterministic(lib, True)
    try:
        pipe, want, held = history(world, spectral, steps, True)
        every_slot_of_the_form_appeared(held, form, FAMILIES["kdist"])
        # maps kept and maps in scratch: the same sums; the class sums kept and in scratch: the same fluxes
        for key, a in want["kdist-corr-scratch"].items():
            assert np.array_equal(a, want["kdist-corr-kept"][key]), key
        for small, own in (("ck-K2-b1", "ck-own-sums-K2-b1"), ("ck-K65-b5-kept", "ck-own-sums-K65-b5")):
            for key, a in want[own].items():
                assert np.array_equal(a, want[small][key]), (own, key)
        kdist_truth(world, pipe, oracle)
        assert same_capacities(holdings(pipe), held)
        pipe.destroy()
    finally:
        _deterministic(lib, False)


@pytest.mark.gpu
@FORMS
def test_all_families_interleaved_on_one_object(world, lib, monkeypatch, spectral):
    """One step of each family in turn, each family's own order kept, test_gpu_pipeline_scratch.py's steps among them."""
    form = "mat" if spectral else "fused"
    lists = [steps_of(world, family, monkeypatch, form) for family in FAMILIES]
    steps = [lst[i] for i in range(max(len(lst) for lst in lists)) for lst in lists if i < len(lst)]
    assert len(steps) == sum(len(lst) for lst in lists)
    _deterministic(lib, True)
    try:
        pipe, want, held = history(world, spectral, steps, False)
        # every slot, staging buffer and keyed table the table gives this form holds something now
        for key, v in held.items():
            assert (v > 0) == (covered(key, form) is not None), (form, key, v)
        pipe.destroy()
    finally:
        _deterministic(lib, False)


# ---- keyed tables ---------------------------------------------------------------------------------------------------------- #
def alternation(w, spectral, what, tables_, call, A, B, other):
    """A, B, A -- keys of equal length and other content -- then a key of another length on one object; every result is a
    fresh object's, A's and B's differ, and the stored key lengths follow."""
    pipe = w.create(spectral)
    solo, lengths = {}, {}
    for name, variant in (("A", A), ("B", B), ("other", other)):
        fresh = w.create(spectral)
        solo[name] = call(fresh, variant)
        fresh.destroy()
    assert any(not np.array_equal(solo["A"][k], solo["B"][k]) for k in solo["A"]), (what, "A and B give the same result")
    for name, variant in (("A", A), ("B", B), ("A", A), ("other", other), ("A", A)):
        compare(call(pipe, variant), solo[name], (what, name))
        now = holdings(pipe)
        lengths.setdefault(name, [now[key] for key in tables_])
        assert lengths[name] == [now[key] for key in tables_] and min(lengths[name]) > 0, (what, name)
    assert lengths["A"] == lengths["B"] and lengths["A"] != lengths["other"], (what, lengths)
    pipe.destroy()


@pytest.mark.gpu
@FORMS
def test_keyed_tables_follow_their_keys(world, lib, spectral):
    w, x, xt, case = world, world.x, world.xt, world.case
    g2 = w.gcols[NCOL]
    both = lambda name: [("table", name, "lw"), ("table", name, "sw")]          # noqa: E731
    _deterministic(lib, True)
    try:
        # the aerosol grid
        def aerosols(pipe, grids):
            f = tuple(aerosol_fields(NCOL, L, g, 60 + bi, lw=bi == 0) for bi, g in enumerate(grids))
            ga, keep = aerosols_of(f, grids)
            pipe.run_aerosols(g2, ga)
            return flat(*pipe.aerosol_fluxes(NCOL))
        alternation(w, spectral, "aerosol grid", both("aer_map"), aerosols, x.xs, tuple(g + 0.37 * (g[1] - g[0]) for g in x.xs),
                    tuple(g[:5] for g in x.xs))

        # the surface grid
        rng = np.random.default_rng(29)
        emis, adir, adif = rng.uniform(0.5, 1.0, (NCOL, 4)), rng.uniform(0.0, 0.6, (NCOL, 4)), rng.uniform(0.0, 0.6, (NCOL, 4))
        e_x, a_x = np.array([50.0, 120.0, 180.0, 240.0]), np.array([1100.0, 1900.0, 2500.0, 3400.0])

        def surface(pipe, grids):
            k = grids[0].size
            gs, keep = api.make_surface(NCOL, emissivity=(grids[0], emis[:, :k]), albedo=(grids[1], adir[:, :k], adif[:, :k]))
            pipe.set_surface(gs)
            pipe.run(g2)
            out = {"fluxes": pipe.fluxes(NCOL)}
            pipe.set_surface(None)
            return out
        alternation(w, spectral, "surface grid", both("surf_map"), surface, (e_x, a_x), (e_x + 9.5, a_x + 95.0), (e_x[:3], a_x[:3]))

        # the tile grid
        def tiles(pipe, grids):
            k = (grids[0].size, grids[1].size)
            gt, keep = api.make_surface_tiles(NCOL, xt.ts, fraction=xt.fr, emissivity=(grids[0], xt.ke[..., :k[0]]),
                                              albedo=(grids[1], xt.kd[..., :k[1]], xt.kf[..., :k[1]]))
            return run_sky_tiles(pipe, g2, w.gclouds(NCOL, 1), w.gaer(NCOL), 1, CLEAN, gt, NCOL)
        alternation(w, spectral, "tile grid", both("tile_map"), tiles, (xt.xe, xt.xa), (xt.xe + 9.5, xt.xa + 95.0),
                    (xt.xe[:2], xt.xa[:2]))

        # the per-angle albedo grid
        def zenith_surface(pipe, grid):
            gs, keep = api.make_zenith_surface(grid, np.ascontiguousarray(case.knots[..., :grid.size]))
            return run_zd(pipe, w.view(NCOL, 1), CLEAN, w.mu[Z5], None, gs, True, False)
        alternation(w, spectral, "per-angle albedo grid", [("table", "zen_surf_map", "sw")], zenith_surface, case.xa,
                    case.xa + 95.0, case.xa[:2])

        # the cloud band limits (another upper limit of liquid band 1 moves the gap behind it; seven ice bands for eight)
        def clouds(pipe, lims):
            cl = pick(x.cl, subcolumns=[0])
            gc, keep = api.make_clouds(lims[0], lims[1], cl["thickness"], *[cl[k] for k in SETS])
            pipe.run_allsky(g2, gc)
            return flat(*pipe.allsky_fluxes(NCOL))
        liquid, ice = limits(w.tables, "liquid"), limits(w.tables, "ice")
        moved = (liquid[0], liquid[1].copy())
        moved[1][1] = 165.0
        alternation(w, spectral, "cloud band limits", both("cloud_map"), clouds, (liquid, ice), (moved, ice),
                    (liquid, (ice[0][:7], ice[1][:7])))

        # the bin edges
        def bins(pipe, edges):
            pipe.run_spectral(g2, None, lw_edges=edges[0], sw_edges=edges[1])
            out = pipe.spectral(NCOL)
            return {k: out[k] for k in ("lw_bins", "sw_bins", "fluxes")}
        alternation(w, spectral, "bin edges", both("bin_table"), bins, ([0, 100, N - 1], [0, 128, N - 1]),
                    ([0, 101, N - 1], [0, 127, N - 1]), ([0, 1, 127, 128, N - 1], [3, 64, 250]))

        # the channel set
        def channels(pipe, inst):
            return run_chan(pipe, g2, w.gclouds(NCOL, 1), w.gaer(NCOL), 1, CLEAN, NCOL, w.sec[1], inst, fluxes=False)
        weights = [np.linspace(0.5, 2.0, 40), np.ones(3)]
        alternation(w, spectral, "channel set", [("table", "channel_table", "lw")], channels, Instrument([100, 7], weights),
                    Instrument([101, 7], weights), Instrument([100, 7, 250], weights + [np.ones(5)]))

        # the response set
        def responses(pipe, resp):
            return run_weighted(pipe, g2, w.gclouds(NCOL, 1), w.gaer(NCOL), 1, CLEAN, NCOL, resp, resp)[1]
        alternation(w, spectral, "response set", both("response_table"), responses, ([100, 7], weights), ([101, 7], weights),
                    ([100, 7, 250], weights + [np.ones(5)]))

        # the class edges, without and with a weight
        def kdist(pipe, v):
            pipe.run_kdist(g2, v[0], lw_edges=CK_LARGE["lw_edges"], sw_edges=CK_LARGE["sw_edges"], lw_weight=v[1], sw_weight=v[1])
            return dropped(pipe.kdist(NCOL))
        ce, wt = np.logspace(-4.0, 1.0, 6), np.linspace(0.5, 1.5, N)
        alternation(w, spectral, "class edges", both("kdist_table"), kdist, (ce, None), (1.5 * ce, None), (ce[:4], None))
        alternation(w, spectral, "class edges under a weight", both("kdist_table"), kdist, (ce, wt), (ce, wt[::-1].copy()), (ce, None))
    finally:
        _deterministic(lib, False)


# ---- shared slots, a surface in force, two calls in flight ---------------------------------------------------------------- #
@pytest.mark.gpu
@FORMS
def test_entry_points_that_share_a_slot_in_both_orders(world, lib, monkeypatch, spectral):
    """Each pair on fresh objects, a then b and b then a: the later call finds the block the other made, every result is
    the call's own, and both orders leave the shared block at the larger of the two needs."""
    form = "mat" if spectral else "fused"
    steps = {name: step for family in FAMILIES for name, step in steps_of(world, family, monkeypatch, form)}
    pairs = [("zeniths-Z5", "sky-zeniths-Z1-S1", ("GRT_SCRATCH_ZEN_PARTIALS", "sw")),
             ("zeniths-Z1-c1", "sky-zeniths-Z5-S3-profile", ("GRT_SCRATCH_ZEN_PARTIALS", "sw")),
             ("direct-own-levels", "weighted-R1-S1", ("GRT_SCRATCH_DIRECT_LEVELS", "sw")),
             ("direct-own-levels", "zen-own-levels-Z5", ("GRT_SCRATCH_DIRECT_LEVELS", "sw")),
             ("weighted-R5-S3", "zen-own-levels-Z1", ("GRT_SCRATCH_DIRECT_LEVELS", "sw")),
             ("kdist-corr-scratch", "ck-K2-b1", ("GRT_SCRATCH_KDIST_MAP", "lw")),
             ("scatter-six-S1", "scatter-profile-S3", ("GRT_SCRATCH_SCATTER_PARTIALS", "lw")),
             # (the third row group: the shortwave's direct beam, the longwave's Jacobian, three rows and V)
             ("direct-six-S1", "direct-profile-S3", ("GRT_SCRATCH_DIRECT_BEAM" if spectral else "GRT_SCRATCH_DIRECT_PARTIALS", "sw")),
             ("jacobian-six-S1", "jacobian-profile-S3", ("GRT_SCRATCH_DIRECT_BEAM" if spectral else "GRT_SCRATCH_DIRECT_PARTIALS", "lw"))]
    if spectral:
        pairs.append(("direct-six-S1", "zen-direct-Z1", ("GRT_SCRATCH_DIRECT_BEAM", "sw")))
    _deterministic(lib, True)
    try:
        solo, need = {}, {}
        for name in {n for a, b, _ in pairs for n in (a, b)}:
            fresh = world.create(spectral)
            solo[name] = steps[name](fresh)
            need[name] = holdings(fresh)
            fresh.destroy()
        for a, b, (slot, band) in pairs:
            key = ("scratch", slot, band)
            ends = []
            for first, second in ((a, b), (b, a)):
                pipe = world.create(spectral)
                compare(steps[first](pipe), solo[first], (first, "before", second))
                assert holdings(pipe) == need[first]
                compare(steps[second](pipe), solo[second], (second, "after", first))
                ends.append(holdings(pipe)[key])
                compare(steps[first](pipe), solo[first], (first, "again after", second))
                assert holdings(pipe)[key] == ends[-1]
                pipe.destroy()
            assert ends[0] == ends[1] == max(need[a][key], need[b][key]), (a, b, key, ends, need[a][key], need[b][key])
            assert max(need[a][key], need[b][key]) > 0, (a, b, key)
    finally:
        _deterministic(lib, False)


@pytest.mark.gpu
@FORMS
def test_a_surface_in_force_outlives_a_call_with_a_surface_per_angle(world, lib, spectral):
    w, case = world, world.case
    g2 = w.gcols[NCOL]
    gs, keep = api.make_surface(NCOL, albedo=(case.xa, case.other, case.dif))
    _deterministic(lib, True)
    try:
        fresh = w.create(spectral)
        fresh.set_surface(gs)
        fresh.run(g2)
        want = fresh.fluxes(NCOL)
        fresh.set_surface(None)
        fresh.run(g2)
        without = fresh.fluxes(NCOL)
        fresh.destroy()
        assert not np.array_equal(want[:, 6:], without[:, 6:])
        fresh = w.create(spectral)
        angles_want = run_zd(fresh, w.view(NCOL, S3), ALL, w.mu[Z5], None, case.gsurf, True, False)
        fresh.destroy()
        pipe = w.create(spectral)
        pipe.set_surface(gs)
        rows = {k: v for k, v in holdings(pipe).items() if "SURF_ROWS" in k[1]}
        got = run_zd(pipe, w.view(NCOL, S3), ALL, w.mu[Z5], None, case.gsurf, True, False)
        # (the per-angle albedo is the direct beam's; the diffuse one is the surface's in force: not the fresh object's rows)
        assert np.all(np.isfinite(got["angle_fluxes"])) and not np.array_equal(got["angle_fluxes"], angles_want["angle_fluxes"])
        now = holdings(pipe)
        assert {k: now[k] for k in rows} == {**rows, ("scratch", "GRT_SCRATCH_ZEN_SURF_ROWS", "sw"): 2 * NCOL * N if spectral else 0}
        pipe.run(g2)
        assert np.array_equal(pipe.fluxes(NCOL), want)
        pipe.set_surface(None)
        compare(run_zd(pipe, w.view(NCOL, S3), ALL, w.mu[Z5], None, case.gsurf, True, False), angles_want, "surface cleared")
        pipe.destroy()
    finally:
        _deterministic(lib, False)


@pytest.mark.gpu
@FORMS
def test_two_calls_queued_back_to_back(world, lib, spectral):
    """Nothing waits and nothing is read between the two calls of a pair; the second replaces a scratch block (the angles'
    partial sums) or a staging buffer (the aerosol tables) that the first one's kernels read.  Both results are the solo
    ones."""
    w = world
    g2 = w.gcols[NCOL]

    def zeniths_small(pipe):
        gz, keep = api.make_zeniths(w.mu[1])
        pipe.run_zeniths(g2, gz)
        return keep

    def zeniths_read(pipe):
        fluxes, per_angle = pipe.zenith_fluxes(NCOL, 1)
        return dict(fluxes=fluxes, angle_fluxes=per_angle)

    def sky_zeniths_large(pipe):
        gsky, keep = api.make_sky(w.gclouds(NCOL, 3), w.gaer(NCOL), 3, ALL)
        gz, keep_z = api.make_zeniths(w.mu[Z5])
        pipe.run_sky_zeniths(g2, gsky, gz, profiles=True)
        return keep, keep_z

    def sky_zeniths_read(pipe):
        return pipe.sky_zenith_profiles(NCOL, 4, Z5)

    def aerosols_small(pipe):
        pipe.run_aerosols(w.gcols[1], w.gaer(1, small=True))

    def aerosols_read(pipe):
        return flat(*pipe.aerosol_fluxes(1))

    def sky_large(pipe):
        gsky, keep = api.make_sky(w.gclouds(NCOL, 1), w.gaer(NCOL), 1, ALL)
        pipe.run_sky(g2, gsky)
        return keep

    def sky_read(pipe):
        return dict(fluxes=pipe.sky_fluxes(NCOL, 4))

    _deterministic(lib, True)
    try:
        for what, key, (run_a, read_a), (run_b, read_b) in (
                ("scratch block", ("scratch", "GRT_SCRATCH_ZEN_PARTIALS", "sw"), (zeniths_small, zeniths_read),
                 (sky_zeniths_large, sky_zeniths_read)),
                ("staging buffer", ("staging", "aer", "-"), (aerosols_small, aerosols_read), (sky_large, sky_read))):
            solo = []
            for run, read in ((run_a, read_a), (run_b, read_b)):
                fresh = w.create(spectral)
                keep = run(fresh)
                solo.append(read(fresh))
                fresh.destroy()
            pipe = w.create(spectral)
            keep_a = run_a(pipe)
            first = holdings(pipe)[key]
            keep_b = run_b(pipe)                     # (queued behind it: no sync, no read)
            assert holdings(pipe)[key] > first > 0, (what, first, holdings(pipe)[key])
            compare(read_b(pipe), solo[1], (what, "second call"))
            compare(read_a(pipe), solo[0], (what, "first call"))
            del keep_a, keep_b
            pipe.destroy()
    finally:
        _deterministic(lib, False)
