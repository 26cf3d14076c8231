"""grt_pipeline_run_sky_weighted's C ABI: exported and declared with its seven arguments, GrtResponses_t field for field the
ctypes structure, at most 256 responses per band, grt_response_pair_count on hand cases and on everything the entry point
refuses in a band's four fields, no new profile tag, and the Python methods (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_run_sky_weighted_is_exported(lib):
    for name in ("grt_pipeline_run_sky_weighted", "grt_response_pair_count", "grt_pipeline_response_block_limit"):
        assert name in api.EXPORTS and hasattr(lib, name), name
    assert "GrtResponses" in dir(api)
    assert list(lib.grt_pipeline_run_sky_weighted.argtypes) == [C.c_void_p, C.POINTER(api.GrtColumns), C.POINTER(api.GrtSky),
                                                                C.POINTER(api.GrtResponses), C.c_void_p, C.c_void_p,
                                                                C.c_void_p]
    assert list(lib.grt_response_pair_count.argtypes) == [C.POINTER(api.GrtResponses), C.c_int, C.c_longlong]
    assert lib.grt_response_pair_count.restype == C.c_longlong
    assert list(lib.grt_pipeline_response_block_limit.argtypes) == [C.c_void_p, C.c_int]


def test_the_declarations():
    src = header("include", "grt_ext.h")
    m = re.search(r"EXTERN int grt_pipeline_run_sky_weighted\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_sky_weighted is not declared in grt_ext.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 7
    assert args[0].startswith("GrtPipeline_t *") and args[1].startswith("GrtColumns_t const *")
    assert args[2].startswith("GrtSky_t const *") and args[3].startswith("GrtResponses_t const *")
    assert args[4:] == ["fp_t *level_fluxes_dev", "fp_t *heating_dev", "fp_t *fluxes_dev"]
    m = re.search(r"EXTERN long long grt_response_pair_count\(([^;]*)\);", src)
    assert m, "grt_response_pair_count is not declared in grt_ext.h"
    args = [" ".join(a.split()) for a in re.sub(r"/\*.*?\*/", "", m.group(1)).split(",")]
    assert args == ["GrtResponses_t const *responses", "int band", "long long num_points"]
    m = re.search(r"EXTERN int grt_pipeline_response_block_limit\(([^;]*)\);", src)
    assert m and [" ".join(a.split()) for a in m.group(1).split(",")] == ["GrtPipeline_t const *pipeline", "int band"]


def test_the_struct_layout_matches_ctypes():
    src = header("include", "grt_ext.h")
    body = re.search(r"typedef struct GrtResponses\s*\{(.*?)\}\s*GrtResponses_t;", src, re.S)
    assert body, "GrtResponses_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if d.strip()]
    assert decls == ["int lw_num_responses", "int const *lw_first", "int const *lw_offset", "fp_t const *lw_weights",
                     "int sw_num_responses", "int const *sw_first", "int const *sw_offset", "fp_t const *sw_weights",
                     "fp_t *weighted_levels_dev", "fp_t *actinic_levels_dev"]
    names = [d.split("*")[-1].split()[-1] for d in decls]
    assert [f[0] for f in api.GrtResponses._fields_] == names
    band = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_double)]
    assert [f[1] for f in api.GrtResponses._fields_] == band + band + [C.c_void_p, C.c_void_p]
    assert C.sizeof(api.GrtResponses) == 80
    assert [getattr(api.GrtResponses, n).offset for n in names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72]


def test_the_constants_and_the_tags():
    src = header("include", "grt_ext.h")
    assert re.findall(r"#define GRT_MAX_RESPONSES (\d+)", src) == ["256"]
    assert api.GRT_MAX_RESPONSES == 256
    # the finishing kernels count under GRT_TAG_BAND_PROFILES: the header's tags are still exactly 1 .. 37
    numbers = [int(v) for v in re.findall(r"GRT_TAG_\w+ = (\d+)", src)]
    assert sorted(numbers) == list(range(1, 38))
    assert re.findall(r"GRT_TAG_BAND_PROFILES = (\d+)", src) == ["14"] and api.TAG_BAND_PROFILES == 14


def pairs(lw=None, sw=None, band=1, n=257):
    g, keep = api.make_responses(lw=lw, sw=sw)
    return api.response_pair_count(g, band, n)


def test_pair_count_on_hand_cases(lib):
    one = np.ones(1)
    for band, kw in ((0, "lw"), (1, "sw")):
        assert pairs(**{kw: ([5], [one])}, band=band) == 1                       # one point
        assert pairs(**{kw: ([127], [np.ones(2)])}, band=band) == 2              # the points 127 .. 128
        assert pairs(**{kw: ([0], [np.ones(257)])}, band=band) == 3              # the whole grid of 257
        assert pairs(**{kw: ([0, 127, 128, 0], [np.ones(257), np.ones(2), one, np.ones(128)])}, band=band) == 3 + 2 + 1 + 1
        assert pairs(**{kw: ([256], [one])}, band=band) == 1
        # negative weights, repeats and overlaps are responses like any other
        assert pairs(**{kw: ([3, 3], [-np.ones(4), np.ones(4)])}, band=band) == 2
    # a band without responses has no pairs; the other band's fields are not looked at
    assert pairs(sw=([5], [one]), band=0) == 0
    assert pairs(lw=([900], [one]), sw=([5], [one]), band=1) == 1


def test_pair_count_refuses_what_the_entry_point_refuses(lib):
    one = np.ones(1)
    assert lib.grt_response_pair_count(None, 1, 257) == -1
    g, keep = api.make_responses(sw=([5], [one]))
    for band in (-1, 2):
        assert api.response_pair_count(g, band, 257) == -1
    for n in (0, -3):
        assert api.response_pair_count(g, 1, n) == -1
    assert pairs(sw=([-1], [one])) == -1                                         # first < 0
    assert pairs(sw=([256], [np.ones(2)])) == -1                                 # first + count > n
    assert pairs(sw=([257], [one])) == -1
    for bad in (np.nan, np.inf, -np.inf):
        assert pairs(sw=([3], [np.array([1.0, bad, 1.0])])) == -1
    for count in (-1, api.GRT_MAX_RESPONSES + 1):
        g, keep = api.make_responses(sw=([5], [one]))
        g.sw_num_responses = count
        assert api.response_pair_count(g, 1, 257) == -1
    assert pairs(sw=(np.arange(api.GRT_MAX_RESPONSES), [one] * api.GRT_MAX_RESPONSES)) == api.GRT_MAX_RESPONSES
    for field in ("sw_first", "sw_offset", "sw_weights"):
        g, keep = api.make_responses(sw=([5], [one]))
        setattr(g, field, None)
        assert api.response_pair_count(g, 1, 257) == -1, field
    g, keep = api.make_responses(sw=([5, 9], [np.ones(2), np.ones(3)]))
    keep["sw_offset"][0] = 1                                                     # offset[0] != 0
    assert api.response_pair_count(g, 1, 257) == -1
    keep["sw_offset"][:] = [0, 2, 2]                                             # not strictly increasing
    assert api.response_pair_count(g, 1, 257) == -1
    keep["sw_offset"][:] = [0, 3, 2]
    assert api.response_pair_count(g, 1, 257) == -1
    keep["sw_offset"][:] = [0, 2, 5]
    assert api.response_pair_count(g, 1, 257) == 2


def test_python_has_the_weighted_calls():
    for name in ("run_sky_weighted", "sky_weighted", "response_block_limit"):
        assert callable(getattr(api.Pipeline, name))
    assert callable(api.make_responses) and callable(api.response_pair_count)
    from grtcode_amd import responses
    for name in ("tabulated", "band", "photon_weight", "erythemal", "join"):
        assert callable(getattr(responses, name))
    g, keep = api.make_responses(lw=([1, 2], [np.ones(3), np.ones(4)]))
    assert g.lw_num_responses == 2 and g.sw_num_responses == 0 and not g.sw_first
    assert list(keep["lw_offset"]) == [0, 3, 7] and list(keep["lw_counts"]) == [3, 4]
