"""The work order of the line kernels (grtcode_amd/csrc/grt_work_order.h), walked on the host through the library's
grt_work_order -- the very function decode_work calls on the device.

Two properties, for every shape:
  * the nb = ngroups*per_group workgroup ids map onto every (group, rem) pair exactly once;
  * locality: the workgroup ids of one residue b % 8 go to one XCD, in order, and about 128 of them are resident there at
    a time.  The items of any 128 consecutive ids of a residue must span at most two groups wherever that is possible at
    all -- and otherwise no more groups than a contiguous run of work items of that length has to touch.

The second bound, worked out rather than observed: n consecutive ids of a residue are 8 apart, so under any order that
deals every group to all eight XCDs they cover n items of a run of W = 8 (n - 1) + 1 consecutive items of the group-major
list, and a run of W items that starts on a group's last item touches (W + per_group - 2) // per_group + 1 groups.  With
n = 128 that is two for per_group >= 1 016 (every batched launch: 60 layers x 64 columns = 3 840) and more below: a group of
8 workgroups has one workgroup per XCD, so 128 ids of a residue touch 128 groups under ANY bijection -- "at most two"
cannot hold for the small shapes of the table, and the bound below is what replaces it there.  The large shapes are here
so that "at most two" itself is asserted."""
import ctypes as C

import pytest

RESIDENT = 128      # workgroups resident on an XCD: 32 CUs x 4
XCDS = 8

# (ngroups, per_group, what the shape is there for)
SHAPES = [
    (1, 1, "smallest case"),
    (1, 7, "nb not a multiple of 8"),
    (5, 3, "nb not a multiple of 8"),
    (13, 60, "longwave-like group count"),
    (196, 8, "shortwave-like group count"),
    (7, 1, "per_group below 8"),
    (13, 1016, "smallest per_group at which 128 resident workgroups span two groups"),
    (5, 3840, "a batched launch: 60 layers x 64 columns per group"),
]


def walk(lib, ngroups, per_group):
    lib.grt_work_order.restype = None
    lib.grt_work_order.argtypes = [C.c_uint] * 4 + [C.POINTER(C.c_uint)] * 2
    nb = ngroups * per_group
    group, rem = C.c_uint(), C.c_uint()
    out = []
    for b in range(nb):
        lib.grt_work_order(nb, per_group, ngroups, b, C.byref(group), C.byref(rem))
        out.append((group.value, rem.value))
    return out


@pytest.mark.parametrize("shape", SHAPES, ids=[f"{g}x{p}" for g, p, _ in SHAPES])
def test_every_item_once_and_resident_workgroups_share_groups(lib, shape):
    ngroups, per_group, _ = shape
    items = walk(lib, ngroups, per_group)
    assert sorted(items) == [(g, r) for g in range(ngroups) for r in range(per_group)]
    for x in range(XCDS):
        groups = [g for g, _ in items[x::XCDS]]         # this XCD's workgroups, in dispatch order
        for k in range(max(len(groups) - RESIDENT, 0) + 1):
            window = groups[k:k + RESIDENT]
            if not window:
                continue
            run = XCDS * (len(window) - 1) + 1
            bound = (run + per_group - 2) // per_group + 1
            if per_group >= XCDS * (RESIDENT - 1):
                assert bound <= 2
            assert len(set(window)) <= bound, (x, k)


def test_every_xcd_takes_an_eighth_of_every_group(lib):
    """What the lockstep order is for: whatever a group costs, each XCD gets its share of it (to within one workgroup)."""
    for ngroups, per_group in ((13, 60), (5, 3840), (196, 8), (5, 3)):
        items = walk(lib, ngroups, per_group)
        for g in range(ngroups):
            counts = [sum(1 for gg, _ in items[x::XCDS] if gg == g) for x in range(XCDS)]
            assert max(counts) - min(counts) <= 1 and sum(counts) == per_group, (ngroups, per_group, g, counts)
