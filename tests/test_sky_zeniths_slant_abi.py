"""grt_pipeline_run_sky_zeniths_slant's C ABI (no GPU needed): the two symbols and their arguments against the header, the
grt_sizeof kind and the ctypes struct in the header's field order, the chunk constants of the shared-layer kernel's slant
instances, the semantics the header must state, and make_zenith_slant's shapes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from grtcode_amd import api, geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def fields_of(src, tag):
    body = re.search(rf"typedef struct {tag}\s*\{{(.*?)\}}\s*{tag}_t;", src, re.S)
    assert body, f"{tag}_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";")]
    return [re.search(r"(\w+)$", d).group(1) for d in decls if d]


def test_the_entry_points_are_exported_and_declared(lib):
    for name in ("grt_pipeline_run_sky_zeniths_slant", "grt_slant_cosines"):
        assert name in api.EXPORTS and hasattr(lib, name), name
    assert len(lib.grt_pipeline_run_sky_zeniths_slant.argtypes) == 10
    src = header("include", "grt_ext.h")
    m = re.search(r"EXTERN int grt_pipeline_run_sky_zeniths_slant\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_sky_zeniths_slant is not declared in grt_ext.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert len(args) == 10
    kinds = ("GrtColumns_t", "GrtSky_t", "GrtZeniths_t", "GrtZenithSlant_t", "GrtZenithSurface_t", "GrtZenithDirect_t")
    for a, kind in zip(args[1:7], kinds):
        assert a.startswith(kind + " const *"), a
    assert all(a.startswith("fp_t *") for a in args[7:])
    m = re.search(r"EXTERN int grt_slant_cosines\(([^;]*)\);", src)
    assert m, "grt_slant_cosines is not declared in grt_ext.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert [a.rsplit(" ", 1)[0] for a in args] == ["double", "int", "int", "int", "double const", "double const", "double"]
    assert len(lib.grt_slant_cosines.argtypes) == 7


def test_size_and_layout(lib):
    src = header("include", "grt_ext.h")
    kinds = [k.strip() for k in re.search(r"enum grt_struct_kind\s*\{(.*?)\}", src, re.S).group(1).replace("= 0", "").split(",")]
    more = re.search(r"enum grt_struct_kind_more\s*\{\s*GRT_ZENITH_SURFACE = GRT_LW_SCATTER \+ 1, GRT_ZENITH_DIRECT\s*\}", src)
    slant = re.search(r"enum grt_struct_kind_slant\s*\{\s*GRT_ZENITH_SLANT = GRT_ZENITH_DIRECT \+ 1\s*\}", src)
    assert more and slant and kinds[-1] == "GRT_LW_SCATTER"
    assert api.GRT_ZENITH_SLANT == len(kinds) + 2 == api.GRT_ZENITH_DIRECT + 1
    assert lib.grt_sizeof(api.GRT_ZENITH_SLANT) == C.sizeof(api.GrtZenithSlant) == C.sizeof(C.c_void_p)
    assert fields_of(src, "GrtZenithSlant") == [f[0] for f in api.GrtZenithSlant._fields_] == ["layer_cos_zenith"]
    assert api.GrtZenithSlant._fields_[0][1] is api.c_double_p
    # (the kinds before it keep their sizes)
    assert lib.grt_sizeof(api.GRT_ZENITH_SURFACE) == C.sizeof(api.GrtZenithSurface)
    assert lib.grt_sizeof(api.GRT_ZENITH_DIRECT) == C.sizeof(api.GrtZenithDirect)
    assert lib.grt_sizeof(api.GRT_ZENITH_SLANT + 1) == 0


def test_chunk_constants_and_the_kernel_join():
    src = header("grtcode_amd", "csrc", "grt_kernels.h")
    for name in ("GRT_ZENITH_CHUNK_SLANT", "GRT_ZENITH_CHUNK_SLANT_SURFACE"):
        m = re.search(rf"#define {name}\s+(\d+)\b", src)
        assert m and int(m.group(1)) == getattr(api, name) and getattr(api, name) in (2, 4), name
    body = re.search(r"typedef struct GrtZenithSlantArgs\s*\{(.*?)\}\s*GrtZenithSlantArgs;", src, re.S)
    assert body and re.search(r"double const \*mu_layer;", body.group(1))
    assert re.search(r"GrtZenithSlantArgs const \*zenith_slant;", src)
    hip = header("grtcode_amd", "csrc", "hip", "k_shortwave.hip")
    assert re.search(r"static_assert\(!has<GrtZenithSlantArgs, Joins\.\.\.> \|\| \(has<GrtZenithArgs, Joins\.\.\.>", hip)


def test_the_header_states_the_semantics():
    src = " ".join(re.sub(r"\n \*", " ", header("include", "grt_ext.h")).split())
    for sentence in (
            "For column c, angle k and layer j (top layer first), the caller gives layer_cos_zenith[c][k][j] in (0, 1].",
            "In layer j the direct-beam solution uses that value wherever it uses mu_dir today.",
            "That covers eddington<true>, its gamma3, the optical-depth clamp, T_pure and so the running direct beam.",
            "The diffuse solution (mu_dif), the adding sweeps and the level expressions are untouched.",
            "The flux scale stays solar * cos_zenith[c][k].",
            "cos_zenith <= 0 stays a night sample: +0.0, nothing solved, the angle's layer cosines not read.",
            "Not covered: a sun below the horizon that still lights upper layers"):
        assert sentence in src, sentence


def test_make_zenith_slant_shapes():
    cosines = np.random.default_rng(5).uniform(0.01, 1.0, (4, 5, 6))
    gs, keep = api.make_zenith_slant(cosines)
    assert keep["shape"] == (4, 5, 6)
    assert np.array_equal(np.ctypeslib.as_array(gs.layer_cos_zenith, shape=(4, 5, 6)), cosines)
    for bad in (cosines[0], cosines[0, 0], cosines[None]):
        with pytest.raises(ValueError):
            api.make_zenith_slant(bad)
    assert callable(api.Pipeline.run_sky_zeniths_slant)
    assert callable(geometry.slant_cosines) and callable(geometry.level_heights)
