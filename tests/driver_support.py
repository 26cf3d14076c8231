"""What the driver tests share: building an example with gcc, running it, the input files the examples read (column text
format, GRTC dump) and the output they write (col lines, text flux file), and the columns the oracle is fed for them."""
import json
import os
import struct
import subprocess

import numpy as np

from grtcode_amd import synthetic as syn
from scenario import MOL_ORDER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "grtcode_amd", "lib")
ARCHIVES = ["-lgrtcode_hip_ext", "-lshortwave", "-llongwave", "-lgas_optics", "-lgrtcode_utilities"]
GM = {syn.CO2: 4.0e-4, syn.CH4: 1.8e-6, syn.N2O: 3.3e-7, syn.CO: 1.0e-7, syn.O2: 0.209}     # mole fractions
NAME = {syn.H2O: "H2O", syn.CO2: "CO2", syn.O3: "O3", syn.N2O: "N2O", syn.CO: "CO", syn.CH4: "CH4", syn.O2: "O2"}


def build_example(name, out, *, shared=False, backtrace=False):
    """examples/<name>.c -> the executable `out`: against the static archives (what a C caller of the reference-shaped API
    links), or with shared=True against libgrtcode_hip.so; backtrace=True makes a fatal signal print where it happened."""
    link = (["-lgrtcode_hip", "-lm", "-Wl,-rpath," + LIBDIR] if shared else
            [*ARCHIVES, "-L/opt/rocm/lib", "-lamdhip64", "-lstdc++", "-lm", "-Wl,-rpath,/opt/rocm/lib"])
    debug = ["-g", "-Wall", "-DGRT_BACKTRACE", "-rdynamic"] if backtrace else ["-Wall"]
    r = subprocess.run(["gcc", "-std=gnu99", "-O2", *debug, "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "examples", name + ".c"), "-L" + LIBDIR, *link, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run_driver(args, env=None, timeout=600):
    """Run the C driver once; if it dies on a signal, the failure report carries its stderr (the driver is built with
    -DGRT_BACKTRACE and prints its own backtrace there).  A driver that died is not started again."""
    r = subprocess.run(args, capture_output=True, text=True, timeout=timeout, env=env)
    if r.returncode < 0:
        raise AssertionError(f"driver died on signal {-r.returncode}\n{r.stderr[-6000:]}")
    return r


def col_lines(stdout):
    """{column: its values} from the "col <i>: ..." lines of rfmip_batch_driver"""
    got = {}
    for line in stdout.splitlines():
        if line.startswith("col "):
            head, vals = line.split(":")
            got[int(head.split()[1])] = np.array([float(x) for x in vals.split()])
    return got


def batch_flags(swb, lw, sw, chunk):
    """rfmip_batch_driver's options after its three positional arguments: continua, the two CFCs with their ppmv, the CIA
    pairs, the two grids (w0, wn, dw as the test writes them), -chunk and the production arithmetic"""
    return ["-h2o-ctm", swb.h2o_dir, "-o3-ctm", swb.files["o3_ctm"],
            "-CFC-11", swb.files["cfc11"], "2.3e-4", "-CFC-12", swb.files["cfc12"], "5.2e-4",
            "-N2-N2", swb.files["cia_n2n2"], "-O2-N2", swb.files["cia_o2n2"], "-O2-O2", swb.files["cia_o2o2"],
            "-w-lw", lw[0], "-W-lw", lw[1], "-r-lw", lw[2], "-w-sw", sw[0], "-W-sw", sw[1], "-r-sw", sw[2],
            "-chunk", str(chunk), "-fast", "3"]


def write_column(path, v):
    rows = [("level_pressure", v["level_pressure_mb"]), ("level_temperature", v["level_temperature"]),
            ("layer_pressure", v["layer_pressure_mb"]), ("layer_temperature", v["layer_temperature"]),
            ("surface_temperature", [v["surface_temperature"]]), ("solar_zenith_angle", [v["solar_zenith_angle_deg"]]),
            ("toa_solar_irradiance", [v["toa_solar_irradiance"]])]
    rows += [(k, v["abundance"][k]) for k in ("H2O", "CO2", "O3", "N2O", "CO", "CH4", "O2", "CFC11", "CFC12")]
    with open(path, "w") as f:
        for name, vals in rows:
            f.write(name + ": " + " ".join(repr(float(x)) for x in vals) + "\n")


def write_grtc_dump(path, ncol, V, raw):
    """the flat dump rfmip_batch_driver reads: magic, ncol, nlev, the five global means, then the columns"""
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", 0x47525443, ncol, V))
        f.write(np.array([GM[syn.CO2], GM[syn.CH4], GM[syn.N2O], GM[syn.CO], GM[syn.O2]]).tobytes())
        f.write(raw.astype("<f8").tobytes())
    return path


def parse_output(path, with_time=False):
    """The text flux file of the driver.h applications: {(column, name): values}, or {(time, column, name): values}."""
    out = {}
    for line in open(path):
        if line.startswith("#"):
            continue
        t, c, name, count, *vals = line.split()
        if with_time:
            out[(int(t), int(c), name)] = np.array([float(x) for x in vals])
        else:
            assert int(count) == len(vals)
            out[(int(c), name)] = np.array([float(x) for x in vals])
    return out


def layers_to_levels(ab, p, pl):
    """rfmip-irf.c:295-308"""
    L = pl.size
    out = np.zeros(L + 1)
    out[0], out[L] = ab[0] * 1e6, ab[L - 1] * 1e6
    for k in range(1, L):
        out[k] = 1e6 * (ab[k - 1] + (ab[k] - ab[k - 1]) * (p[k] - pl[k - 1]) / (pl[k] - pl[k - 1]))
    return out


def as_column(v):
    """The column the drivers build from a column text file (basic-circ-test.c semantics) as the checker wants it."""
    p, pl = np.array(v["level_pressure_mb"]), np.array(v["layer_pressure_mb"])
    L = pl.size

    def to_levels(ab):                                  # basic-circ-test.c:51-66
        ab = np.array(ab)
        out = np.zeros(L + 1)
        out[0], out[L] = ab[0] * 1e6, ab[L - 1] * 1e6
        for i in range(1, L):
            out[i] = (ab[i - 1] + (ab[i] - ab[i - 1]) * (p[i] - pl[i - 1]) / (pl[i] - pl[i - 1])) * 1e6
        return out
    ppmv = {m: to_levels(v["abundance"][NAME[m]]) for m in MOL_ORDER}
    ppmv[syn.N2] = np.full(L + 1, 0.781e6)
    mu0 = float(np.cos(2.0 * np.pi * v["solar_zenith_angle_deg"] / 360.0))
    return dict(p=p, t=np.array(v["level_temperature"]), t_layer=np.array(v["layer_temperature"]),
                t_surf=v["surface_temperature"], ppmv=ppmv, mu0=mu0, tsi=v["toa_solar_irradiance"] / mu0,
                cfc_ppmv={0: to_levels(v["abundance"]["CFC11"]), 1: to_levels(v["abundance"]["CFC12"])})


def circ1_column():
    """CIRC case 1 (the numbers of circ/src/circ1.h, held in tests/golden): the checker's column and the raw values"""
    v = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_test_vectors.json")))["circ1"]
    return as_column(v), v


def rfmip_like_columns(n, V):
    cols, raw = [], []
    for c in range(n):
        base = syn.profile(c, V)
        p_pa = base["p"] * 100.0
        play_pa = 0.5 * (p_pa[:-1] + p_pa[1:])
        h2o_lay = 0.5e-6 * (base["ppmv"][syn.H2O][:-1] + base["ppmv"][syn.H2O][1:])
        o3_lay = 0.5e-6 * (base["ppmv"][syn.O3][:-1] + base["ppmv"][syn.O3][1:])
        sza = [20.0, 55.0, 100.0, 70.0, 0.0][c % 5]                  # column 2 of every five is a night column
        tsi, emis, alb = 1360.0, 0.97, 0.12
        raw.append(np.concatenate([p_pa, play_pa, base["t"], base["t_layer"],
                                   [base["t_surf"], emis, alb, sza, tsi], h2o_lay, o3_lay]))
        # what the driver must make of it (rfmip-irf.c:186,295-308,318-325)
        p, pl = p_pa * 0.01, play_pa * 0.01
        ppmv = {m: np.full(V, x * 1e6) for m, x in GM.items()}
        ppmv[syn.H2O], ppmv[syn.O3] = layers_to_levels(h2o_lay, p, pl), layers_to_levels(o3_lay, p, pl)
        ppmv[syn.N2] = np.full(V, 0.781e6)
        cols.append(dict(p=p, t=base["t"], t_layer=base["t_layer"], t_surf=base["t_surf"], ppmv=ppmv,
                         mu0=float(np.cos(2.0 * np.pi * sza / 360.0)), tsi=tsi,
                         cfc_ppmv={0: np.full(V, 2.3e-4), 1: np.full(V, 5.2e-4)}, emis=emis, alb=alb))
    return cols, np.concatenate(raw)
