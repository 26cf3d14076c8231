#!/usr/bin/env python3
"""How many vector instructions one lean block costs (no GPU needed).

    scripts/lean_block_count.py [--root TREE] [--json]

The lean first pass fills the vector pipe, so its time follows the number of vector wave instructions
a block of 128 lines issues.  This compiles grtcode_amd/csrc/hip/k_gas_optics_mp.hip of TREE (default: this checkout)
device-only to assembly with build.py's HIPFLAGS and prints one table per instance of gas_optics_lean_kernel (NARROW =
true: the longwave band's, false: the shortwave band's):

  * registers: VGPRs, spilled SGPRs, scratch bytes per lane (the compiler's kernel-resource-usage remarks);
  * vector instructions by class, counted by mnemonic prefix, for two stretches of the line loop that
    mp_lean_block.inc marks with assembly comments (`; lean block: begin`, `: core points`, `: end`):
        block    the block proper, from the loop's head to the push of its core points into the raw queue,
        loop     the whole loop body, to the request for the next block's records (queues, drain_raw and the
                 class formulas behind it included);
    and for each stretch two counts:
        main     along the CHEAPEST path through the stretch's control flow (every conditional branch taken to its
                 cheaper side, no loop walked twice): what every block issues at least -- the rare branches (lines handed
                 to general_block, lanes outside their row's two cells, region 1 beyond the near field, a raw queue that is
                 full) are not on it, nor is the dearer side of a choice the tile's flags make;
        static   every instruction between the two comments as the file lays them out, rare branches included.

The loop's head is the last label before the `begin` comment (the scheduler moves the block's first instructions ahead
of the comment).  Classes: DPP (any mnemonic with a _dpp suffix), lane read/write (v_readlane, v_writelane,
v_readfirstlane), packed fp32 (v_pk_), fp64 (_f64), compare (v_cmp), select (v_cndmask), convert (v_cvt_ and the
roundings and exponent moves that run at the same rate: v_rndne_, v_floor_, v_ceil_, v_trunc_, v_fract_, v_ldexp_,
v_frexp_), transcendental (v_rcp_, v_rsq_, v_sqrt_, v_exp_, v_log_, v_sin_, v_cos_), other fp32 (_f32), other (every
other v_).  tests/test_lean_block_count.py holds the counts to profiles/lean_block_count_after.txt."""
import argparse
import heapq
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SOURCE = os.path.join("grtcode_amd", "csrc", "hip", "k_gas_optics_mp.hip")
KERNEL = "gas_optics_lean_kernel"
INSTANCES = {"ILb1E": "gas_optics_lean_kernel<true> (longwave)", "ILb0E": "gas_optics_lean_kernel<false> (shortwave)"}
MARK = {"begin": "; lean block: begin", "core": "; lean block: core points", "end": "; lean block: end"}
CLASSES = ["packed fp32", "other fp32", "fp64", "compare", "select", "convert", "transcendental", "DPP", "lane read/write",
           "other"]
CONVERT = ("v_cvt_", "v_rndne_", "v_floor_", "v_ceil_", "v_trunc_", "v_fract_", "v_ldexp_", "v_frexp_")
TRANSCENDENTAL = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_exp_", "v_log_", "v_sin_", "v_cos_")
LANE = ("v_readlane", "v_writelane", "v_readfirstlane")


def classify(mnemonic):
    """The class of a vector instruction, None for anything that is not one."""
    m = mnemonic
    if not m.startswith("v_"):
        return None
    if "_dpp" in m:
        return "DPP"
    if m.startswith(LANE):
        return "lane read/write"
    if m.startswith("v_pk_"):
        return "packed fp32" if "_f32" in m else "other"
    if m.startswith("v_cmp"):
        return "compare"
    if m.startswith("v_cndmask"):
        return "select"
    if m.startswith(CONVERT):
        return "convert"
    if m.startswith(TRANSCENDENTAL):
        return "transcendental"
    if "_f64" in m:
        return "fp64"
    if "_f32" in m:
        return "other fp32"
    return "other"


def compile_assembly(root, workdir):
    """-> (assembly text, remarks text) of TREE's k_gas_optics_mp.hip under build.py's flags."""
    from grtcode_amd.build import HIPFLAGS, ROOT as BUILD_ROOT
    flags = [f.replace(BUILD_ROOT, root) for f in HIPFLAGS]
    out = os.path.join(workdir, "k_gas_optics_mp.s")
    r = subprocess.run(["hipcc"] + flags + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                           os.path.join(root, SOURCE), "-o", out],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout)
        raise RuntimeError("hipcc failed")
    with open(out) as f:
        return f.read(), r.stdout


def resources(remarks):
    """{instance key: {vgprs, sgpr_spills, scratch_bytes}} from the compiler's remarks."""
    out, key = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: +(Function Name|VGPRs|SGPRs Spill|ScratchSize \[bytes/lane\]): +(\S+)", line)
        if not m:
            continue
        what, value = m.groups()
        if what == "Function Name":
            key = next((k for k in INSTANCES if KERNEL + k in value), None)
            if key is not None:
                out[key] = {}
        elif key is not None:
            out[key][{"VGPRs": "vgprs", "SGPRs Spill": "sgpr_spills"}.get(what, "scratch_bytes")] = int(value)
    return out


def function_lines(assembly, key):
    """The lines of the instance's body, comments stripped but for the block's marks."""
    lines, inside = [], False
    for raw in assembly.splitlines():
        if not inside:
            inside = re.match(r"^_Z\w*" + KERNEL + key + r"\w*:", raw) is not None
            continue
        if raw.startswith(".Lfunc_end"):
            break
        text = raw.strip()
        if text in MARK.values():
            lines.append(text)
            continue
        text = text.split(";")[0].strip()
        if text and not text.startswith(".") or re.match(r"^\.LBB\w+:$", text):
            lines.append(text)
    if not lines:
        raise RuntimeError(f"no {KERNEL}{key} in the assembly")
    return lines


def tally(instructions):
    t = dict.fromkeys(CLASSES, 0)
    for ins in instructions:
        c = classify(ins.split()[0])
        if c is not None:
            t[c] += 1
    return t


def cheapest_path(lines, start, stop):
    """Instructions along the path from line `start` to line `stop` that issues the fewest vector instructions.
    Basic blocks end at labels, branches and the stop line; a conditional branch has two ways on, s_branch one."""
    label_at = {ln[:-1]: i for i, ln in enumerate(lines) if ln.endswith(":")}
    leaders = sorted(set([start, stop] + list(label_at.values())
                         + [i + 1 for i, ln in enumerate(lines) if ln.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_setpc"))]))
    leaders = [i for i in leaders if i < len(lines)]
    nxt = {a: b for a, b in zip(leaders, leaders[1:])}
    blocks = {}
    for a in leaders:
        b = nxt.get(a, len(lines))
        body = [ln for ln in lines[a:b] if not ln.endswith(":") and ln not in MARK.values()]
        last = body[-1] if body else ""
        succ = []
        if last.startswith(("s_cbranch", "s_branch")):
            succ.append(label_at[last.split()[-1]])
        if not last.startswith(("s_branch", "s_endpgm", "s_setpc")) and b < len(lines):
            succ.append(b)
        blocks[a] = (body, sum(classify(ln.split()[0]) is not None for ln in body), succ)
    best, heap = {start: (0, None)}, [(0, start)]
    while heap:
        cost, a = heapq.heappop(heap)
        if a == stop:
            break
        if cost > best[a][0]:
            continue
        for s in blocks[a][2]:
            c = cost + blocks[a][1]
            if s not in best or c < best[s][0]:
                best[s] = (c, a)
                heapq.heappush(heap, (c, s))
    if stop not in best:
        raise RuntimeError("the stretch's end cannot be reached from its head")
    path, a = [], best[stop][1]
    while a is not None:
        path.append(a)
        a = best[a][1]
    return [ln for a in reversed(path) for ln in blocks[a][0]]


def count_instance(assembly, key):
    lines = function_lines(assembly, key)
    at = {name: lines.index(text) for name, text in MARK.items()}
    head = max(i for i, ln in enumerate(lines[:at["begin"]]) if ln.endswith(":"))
    out = {}
    for stretch, stop in (("block", at["core"]), ("loop", at["end"])):
        static = [ln for ln in lines[head:stop] if not ln.endswith(":") and ln not in MARK.values()]
        out[stretch] = {"main": tally(cheapest_path(lines, head, stop)), "static": tally(static)}
    return out


def count(root=ROOT):
    """{instance key: {vgprs, sgpr_spills, scratch_bytes, block: {main, static}, loop: {main, static}}}"""
    workdir = tempfile.mkdtemp(prefix="lean_block_count_")
    try:
        assembly, remarks = compile_assembly(root, workdir)
    finally:
        shutil.rmtree(workdir, ignore_errors=True)
    res = resources(remarks)
    return {key: dict(res[key], **count_instance(assembly, key)) for key in INSTANCES}


def render(counts):
    out = []
    for key, title in INSTANCES.items():
        c = counts[key]
        out.append(f"== {title} ==")
        out.append(f"{key} VGPRs: {c['vgprs']}")
        out.append(f"{key} spilled SGPRs: {c['sgpr_spills']}")
        out.append(f"{key} scratch bytes per lane: {c['scratch_bytes']}")
        out.append(f"{'vector instructions':<24}{'block main':>12}{'block static':>14}{'loop main':>12}{'loop static':>13}")
        cols = [c["block"]["main"], c["block"]["static"], c["loop"]["main"], c["loop"]["static"]]
        for cls in CLASSES:
            out.append(f"{cls:<24}{cols[0][cls]:>12}{cols[1][cls]:>14}{cols[2][cls]:>12}{cols[3][cls]:>13}")
        out.append(f"{'total':<24}{sum(cols[0].values()):>12}{sum(cols[1].values()):>14}{sum(cols[2].values()):>12}{sum(cols[3].values()):>13}")
        out.append(f"{key} main-path vector instructions, block: {sum(cols[0].values())}")
        out.append(f"{key} main-path vector instructions, loop: {sum(cols[2].values())}")
        out.append(f"{key} main-path lane reads/writes, loop: {cols[2]['lane read/write']}")
        out.append("")
    return "\n".join(out)


def parse(text):
    """The figures a rendered table states outright: {instance key: {what: number}}."""
    out = {}
    for key, what, value in re.findall(r"^(ILb[01]E) ([^:]+): (\d+)$", text, flags=re.M):
        out.setdefault(key, {})[what] = int(value)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--root", default=ROOT, help="the tree whose kernel is counted (default: this checkout)")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    counts = count(os.path.abspath(args.root))
    print(json.dumps(counts, indent=1) if args.json else render(counts))


if __name__ == "__main__":
    main()
