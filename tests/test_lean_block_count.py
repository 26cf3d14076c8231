"""A ratchet on what one lean block costs: scripts/lean_block_count.py compiles the first pass for gfx950 and counts the
vector instructions of the lean block; the counts may not rise above those written into profiles/lean_block_count_after.txt
(when a change lowers them, that file is written again).  No GPU needed; skipped where there is no hipcc."""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import lean_block_count  # noqa: E402

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc: nothing to compile with")
RECORD = os.path.join(ROOT, "profiles", "lean_block_count_after.txt")


@pytest.fixture(scope="module")
def counts():
    c = lean_block_count.count()
    print(lean_block_count.render(c))
    return c


@pytest.fixture(scope="module")
def recorded():
    with open(RECORD) as f:
        return lean_block_count.parse(f.read())


def test_the_rendered_table_reads_back(counts):
    back = lean_block_count.parse(lean_block_count.render(counts))
    for key, c in counts.items():
        assert back[key]["VGPRs"] == c["vgprs"] and back[key]["spilled SGPRs"] == c["sgpr_spills"]
        assert back[key]["main-path vector instructions, block"] == sum(c["block"]["main"].values())


@pytest.mark.parametrize("key", list(lean_block_count.INSTANCES))
def test_registers(counts, key):
    assert counts[key]["scratch_bytes"] == 0
    assert counts[key]["vgprs"] <= 128


@pytest.mark.parametrize("key", list(lean_block_count.INSTANCES))
@pytest.mark.parametrize("stretch", ["block", "loop"])
def test_main_path_is_no_longer_than_recorded(counts, recorded, key, stretch):
    got = sum(counts[key][stretch]["main"].values())
    want = recorded[key][f"main-path vector instructions, {stretch}"]
    print(f"{lean_block_count.INSTANCES[key]}, {stretch}: {got} vector instructions on the main path (recorded {want})")
    assert got <= want


@pytest.mark.parametrize("key", list(lean_block_count.INSTANCES))
def test_lane_reads_and_writes_of_the_loop_are_no_more_than_recorded(counts, recorded, key):
    """The loop's scalars do not all fit the scalar registers: what the compiler parks in a vector register's lanes and
    reads back on the main path is held to the recorded number (DESIGN.md §3.1 says why it is not zero)."""
    assert counts[key]["loop"]["main"]["lane read/write"] <= recorded[key]["main-path lane reads/writes, loop"]
    assert counts[key]["sgpr_spills"] <= recorded[key]["spilled SGPRs"]
