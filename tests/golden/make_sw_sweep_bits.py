"""Record tests/golden/sw_sweep_bits.npz: every output of tests/sw_sweep_cases.py's runs -- the pipeline's entry points that
reach a kernel of k_shortwave.hip, on a shortwave-only pipeline (the tiles: both bands) in both forms --, in deterministic
mode, from the library of the commit that is checked out: the bits that tests/test_gpu_sw_sweep_bits.py holds every later
k_shortwave.hip to.  Needs the GPU.

    python tests/golden/make_sw_sweep_bits.py [--library PATH] [--commit HASH] [--out FILE]

--library: a libgrtcode_hip.so built from another commit (then say which with --commit); default: this tree's library and
`git rev-parse HEAD`."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--library")
    ap.add_argument("--commit")
    ap.add_argument("--out", default=os.path.join(HERE, "sw_sweep_bits.npz"))
    args = ap.parse_args()
    from grtcode_amd import api
    import sw_sweep_cases as cases
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    if args.library:
        os.environ["GRT_LIB_PATH"] = os.path.abspath(args.library)      # (every object of api loads the same library)
    lib = api.load_library()
    device = api.create_device(0)
    api.check(lib.grt_set_deterministic(1))
    with tempfile.TemporaryDirectory() as tmp:
        inp = cases.Inputs(tmp)
        got = cases.run_all(inp, device)
        again = cases.run_all(inp, device)
    assert got.keys() == again.keys()
    for name, a in got.items():
        assert np.array_equal(a, again[name]), name
        assert np.all(np.isfinite(a)) and np.any(a != 0.0), name
        print(f"{name}: shape {a.shape}, largest magnitude {np.abs(a).max():.6e}")
    out = {"commit": np.array(commit), "seed": np.array(cases.SEED)}
    out.update(got)
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(got)} arrays, commit {commit}")


if __name__ == "__main__":
    main()
