"""Record tests/golden/lean_first_pass_bits.npz: the optical depths of tests/lean_block_cases.py's four grids after the lean
first pass and the gather, in deterministic mode, from the library of the commit that is checked out -- the bits that
tests/test_gpu_lean_block_bits.py holds every later first pass to.  Needs the GPU.

    python tests/golden/make_lean_first_pass_bits.py [--library PATH] [--commit HASH] [--out FILE]

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
    ap.add_argument("--out", default=os.path.join(HERE, "lean_first_pass_bits.npz"))
    args = ap.parse_args()
    from grtcode_amd import api
    import lean_block_cases as cases
    commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    if args.library:
        os.environ["GRT_LIB_PATH"] = os.path.abspath(args.library)      # (every object of api loads the same library)
    lib = api.load_library()
    device = api.create_device(0)
    api.check(lib.grt_set_deterministic(1))
    out = {"commit": np.array(commit), "seed": np.array(cases.SEED)}
    with tempfile.TemporaryDirectory() as tmp:
        for name in cases.GRIDS:
            band = cases.band_of(os.path.join(tmp, name), name)
            tau, ranges = cases.first_pass_tau(band, device)
            again, _ = cases.first_pass_tau(band, device)
            assert np.array_equal(tau, again), name
            assert np.all(np.isfinite(tau)) and np.all(tau.max(axis=2) > 0.0), name
            print(f"{name}: {sum(a['v0'].size for a in band.lines.values())} lines, tile ranges {ranges.tolist()}, "
                  f"largest tau per layer {tau.max(axis=2).tolist()}")
            out["tau_" + name] = tau
    np.savez_compressed(args.out, **out)
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, commit {commit}")


if __name__ == "__main__":
    main()
