"""The C ABI of the longwave scattering correction: grt_pipeline_run_sky_scattering and grt_lw_scatter_levels exported and
declared with their argument lists, GrtLwScatter_t field for field the ctypes structure and grt_sizeof's size, the two
profile tags, the kernel in the build and in liblongwave.a, the shared device code in its header, the Python calls, and the
refusals the host decides before it needs a device (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from grtcode_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def text(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def declared_args(name):
    m = re.search(r"EXTERN int %s\(([^;]*)\);" % name, text("include", "grt_ext.h"))
    assert m, f"{name} is not declared in grt_ext.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_the_functions_are_exported_and_declared(lib):
    for name in ("grt_pipeline_run_sky_scattering", "grt_lw_scatter_levels"):
        assert name in api.EXPORTS and hasattr(lib, name), name
    assert declared_args("grt_pipeline_run_sky_scattering") == [
        "GrtPipeline_t *pipeline", "GrtColumns_t const *columns", "GrtSky_t const *sky", "fp_t *level_fluxes_dev",
        "fp_t *heating_dev", "fp_t *fluxes_dev", "fp_t *scatter_levels_dev", "fp_t *scatter_dev"]
    assert list(lib.grt_pipeline_run_sky_scattering.argtypes) == [C.c_void_p, C.POINTER(api.GrtColumns),
                                                                  C.POINTER(api.GrtSky)] + [C.c_void_p] * 5
    assert declared_args("grt_lw_scatter_levels") == ["Device_t device", "GrtLwScatter_t const *scatter"]
    assert list(lib.grt_lw_scatter_levels.argtypes) == [C.c_int, C.POINTER(api.GrtLwScatter)]


def test_the_struct_layout_matches_ctypes_and_grt_sizeof(lib):
    body = re.search(r"typedef struct GrtLwScatter\s*\{(.*?)\}\s*GrtLwScatter_t;", text("include", "grt_ext.h"), re.S)
    assert body, "GrtLwScatter_t is not declared in grt_ext.h"
    decls = [d.strip() for d in re.sub(r"/\*.*?\*/", "", body.group(1), flags=re.S).split(";") if d.strip()]
    assert decls == ["int ncol", "int num_levels", "long long n", "fp_t w0, dw", "fp_t const *tau_dev, *omega_dev, *g_dev",
                     "fp_t const *layer_temperature_dev, *level_temperature_dev, *surface_temperature_dev",
                     "fp_t const *emissivity_dev", "fp_t *delta_up_dev, *delta_down_dev", "fp_t *flux_up_dev, *flux_down_dev"]
    names = ["ncol", "num_levels", "n", "w0", "dw", "tau_dev", "omega_dev", "g_dev", "layer_temperature_dev",
             "level_temperature_dev", "surface_temperature_dev", "emissivity_dev", "delta_up_dev", "delta_down_dev",
             "flux_up_dev", "flux_down_dev"]
    assert [f[0] for f in api.GrtLwScatter._fields_] == names
    assert [getattr(api.GrtLwScatter, n).offset for n in names] == [0, 4] + list(range(8, 8 + 8 * 14, 8))
    assert C.sizeof(api.GrtLwScatter) == 120
    assert re.search(r"GRT_CLOUD_FIELDS, GRT_LW_SCATTER\s*\}", text("include", "grt_ext.h"))
    assert lib.grt_sizeof(api.GRT_LW_SCATTER) == C.sizeof(api.GrtLwScatter)
    assert lib.grt_sizeof(api.GRT_CLOUD_FIELDS) == C.sizeof(api.GrtCloudFields)


def test_the_tags_continue_the_list():
    header = text("include", "grt_ext.h")
    assert re.findall(r"GRT_TAG_TILE_MEAN = (\d+)", header) == ["37"]
    assert len(re.findall(r"GRT_TAG_SCATTER_LW = GRT_TAG_TILE_MEAN \+ 1,\s*GRT_TAG_SCATTER_FINISH\s*\}", header)) == 1
    assert api.TAG_TILE_MEAN == 37 and api.TAG_SCATTER_LW == 38 and api.TAG_SCATTER_FINISH == 39


def test_the_kernel_is_where_it_belongs():
    assert "k_longwave_scatter.hip" in build.HIP_SRC
    assert build.ARCHIVES["liblongwave.a"] == ["k_longwave", "k_longwave_scatter"]
    members = subprocess.run(["ar", "t", os.path.join(build.LIB, "liblongwave.a")], check=True, capture_output=True,
                             text=True).stdout.split()
    assert sorted(members) == ["k_longwave.o", "k_longwave_scatter.o"]
    sc = text("grtcode_amd", "csrc", "hip", "k_longwave_scatter.hip")
    lw = text("grtcode_amd", "csrc", "hip", "k_longwave.hip")
    dev = text("grtcode_amd", "csrc", "hip", "longwave_dev.h")
    assert len(re.findall(r"__global__[^\n]*void lw_scatter_kernel\(", sc)) == 1
    assert "#pragma clang fp contract(off)" in sc and "#pragma clang fp contract(off)" in dev
    # what both files must say alike is said once, in the header both include
    for once in (r"__device__[^\n]*double effective_planck\(", r"__device__[^\n]*double absorption_tau\(", r"struct LwPoint\b"):
        assert len(re.findall(once, dev)) == 1, once
        assert not re.findall(once, lw) and not re.findall(once, sc), once
    for src in (lw, sc):
        assert '#include "longwave_dev.h"' in src and '#include "planck_dev.h"' in src
    for used in ("LwPoint<", "effective_planck(", "planck(", "LevelSink<"):
        assert used in sc, used
    # no per-thread arrays in the kernel: its sweeps carry scalars
    body = sc[sc.index("void lw_scatter_kernel("):]
    body = body[:body.index("\n}\n")]
    assert not re.findall(r"\bdouble\s+\w+\[", body)
    kernels = text("grtcode_amd", "csrc", "grt_kernels.h")
    for name in ("GrtScatterArgs", "grt_launch_lw_scatter", "grt_scatter_args_ok", "GrtScatterArgs const *scatter",
                 "grt_launch_scatter_add"):
        assert name in kernels, name
    assert re.search(r"scatter_ok = in\.scatter == nullptr \|\|", kernels)


def test_python_has_the_calls():
    for name in ("run_sky_scattering", "sky_scatter_fluxes", "sky_scatter_profiles"):
        assert callable(getattr(api.Pipeline, name)), name
    assert callable(api.lw_scatter_levels)


def test_refusals_that_need_no_device(lib):
    # the kernel-level entry decides its arguments before it looks at the device
    assert lib.grt_lw_scatter_levels(0, None) == api.VALUE_ERR
    fake = C.c_void_p(0x1000)

    def full():
        sc = api.GrtLwScatter(ncol=1, num_levels=3, n=8, w0=500.0, dw=1.0)
        for f in ("tau_dev", "omega_dev", "g_dev", "layer_temperature_dev", "level_temperature_dev",
                  "surface_temperature_dev", "emissivity_dev", "delta_up_dev", "delta_down_dev"):
            setattr(sc, f, fake)
        return sc

    for f in ("tau_dev", "layer_temperature_dev", "level_temperature_dev", "surface_temperature_dev", "emissivity_dev",
              "delta_up_dev", "delta_down_dev"):
        sc = full()
        setattr(sc, f, None)
        assert lib.grt_lw_scatter_levels(0, C.byref(sc)) == api.VALUE_ERR, f
    for f, v in (("ncol", 0), ("ncol", 65536), ("num_levels", 1), ("n", 0), ("dw", 0.0), ("dw", float("nan")),
                 ("dw", float("inf")), ("flux_up_dev", fake), ("flux_down_dev", fake)):
        sc = full()
        setattr(sc, f, v)
        assert lib.grt_lw_scatter_levels(0, C.byref(sc)) == api.VALUE_ERR, (f, v)
    # the pipeline entry: the pipeline and the columns are looked at first, then the scatter outputs
    cols, sky = api.GrtColumns(), api.GrtSky()
    args = [None] * 5
    assert lib.grt_pipeline_run_sky_scattering(None, C.byref(cols), C.byref(sky), *args) == api.NULL_ERR
    assert lib.grt_pipeline_run_sky_scattering(fake, None, C.byref(sky), *args) == api.NULL_ERR
    # both scatter outputs NULL; scatter_levels_dev in the six-row form
    assert lib.grt_pipeline_run_sky_scattering(fake, C.byref(cols), C.byref(sky), None, None, fake, None, None) == api.VALUE_ERR
    assert lib.grt_pipeline_run_sky_scattering(fake, C.byref(cols), C.byref(sky), None, None, fake, fake, fake) == api.VALUE_ERR
