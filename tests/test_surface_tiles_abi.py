"""grt_pipeline_run_sky_tiles' C ABI: exported and declared with its five arguments, its three profile tags, its limits and
a ctypes struct in the header's field order and size (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

from grtcode_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_run_sky_tiles_is_exported(lib):
    assert "grt_pipeline_run_sky_tiles" in api.EXPORTS
    assert hasattr(lib, "grt_pipeline_run_sky_tiles")
    assert len(lib.grt_pipeline_run_sky_tiles.argtypes) == 5


def test_tags_and_limits_equal_the_headers():
    src = header("include", "grt_ext.h")
    for name, value, want in (("TILE_LW", api.TAG_TILE_LW, 35), ("TILE_SW", api.TAG_TILE_SW, 36),
                              ("TILE_MEAN", api.TAG_TILE_MEAN, 37)):
        assert re.findall(rf"GRT_TAG_{name} = (\d+)", src) == [str(want)] and value == want, name
    assert api.TAG_CK_SW == 34
    numbers = [int(v) for v in re.findall(r"GRT_TAG_\w+ = (\d+)", src)]
    assert sorted(numbers) == list(range(1, 38))
    m = re.search(r"#define GRT_MAX_TILES\s+(\d+)\b", src)
    assert m and int(m.group(1)) == api.GRT_MAX_TILES == 16
    kernels = header("grtcode_amd", "csrc", "grt_kernels.h")
    chunks = re.findall(r"#define GRT_TILE_CHUNK(?:_\w+)?\s+(\d+)\b", kernels)
    assert len(chunks) == 4 and {int(c) for c in chunks} == {api.GRT_TILE_CHUNK} and api.GRT_TILE_CHUNK in (2, 4, 8)
    for name in ("grt_launch_lw_tiles", "grt_launch_sw_tiles", "grt_launch_tile_mean", "grt_tile_chunk"):
        assert re.search(rf"\bint {name}\(", kernels), name


def test_run_sky_tiles_is_declared_and_the_struct_matches():
    src = header("include", "grt_ext.h")
    m = re.search(r"EXTERN int grt_pipeline_run_sky_tiles\(([^;]*)\);", src)
    assert m, "grt_pipeline_run_sky_tiles is not declared in grt_ext.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(args) == 5
    assert args[1].startswith("GrtColumns_t const *") and args[2].startswith("GrtSky_t const *")
    assert args[3].startswith("GrtSurfaceTiles_t const *") and args[4].startswith("fp_t *")
    body = re.search(r"typedef struct GrtSurfaceTiles\s*\{(.*?)\}\s*GrtSurfaceTiles_t;", src, re.S)
    assert body, "GrtSurfaceTiles_t is not declared in grt_ext.h"
    names = []
    for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";"):
        names += [re.search(r"(\w+)$", part.strip()).group(1) for part in d.split(",") if part.strip()]
    assert names == [f[0] for f in api.GrtSurfaceTiles._fields_]
    ints = {"num_tiles", "num_emissivity_points", "num_albedo_points"}
    for n, t in api.GrtSurfaceTiles._fields_:
        assert t is (C.c_int if n in ints else C.c_void_p if n == "tile_fluxes_dev" else api.c_double_p), n
    # an int, two pointers, two ints, six pointers: 4 (+ 4) + 16 + 8 + 48 bytes where pointers and doubles take eight
    assert C.sizeof(api.GrtSurfaceTiles) == 80
    assert api.GrtSurfaceTiles.num_emissivity_points.offset == 24 and api.GrtSurfaceTiles.tile_fluxes_dev.offset == 72


def test_python_pipeline_has_the_tile_calls():
    for name in ("run_sky_tiles", "sky_tile_fluxes"):
        assert callable(getattr(api.Pipeline, name))
    t_surf = np.full((2, 3), 280.0)
    grid = np.array([10.0, 20.0, 40.0])
    gt, keep = api.make_surface_tiles(2, t_surf, fraction=np.full((2, 3), 0.25), emissivity=(grid, np.full((2, 3, 3), 0.9)),
                                      albedo=(grid[:2], np.full((2, 3, 2), 0.1)))
    assert gt.num_tiles == 3 and keep["shape"] == (2, 3) and keep["num_points"] == (3, 2)
    assert gt.num_emissivity_points == 3 and gt.num_albedo_points == 2 and not gt.diffuse_albedo and not gt.tile_fluxes_dev
    gt, keep = api.make_surface_tiles(2, t_surf)
    assert gt.num_tiles == 3 and keep["num_points"] == (0, 0) and not gt.fraction and not gt.emissivity
