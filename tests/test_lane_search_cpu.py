"""Pins for the tree searches' shared shape (csrc/lane_search.h, csrc/split_front.h): the
workspace size every *_gpu entry point reports, and the resources of the lane-refill kernels
and of the split front end's kernels in the built library.  No GPU: a query with a null
workspace returns before any HIP call, and the resources are read from the code objects'
metadata."""
import ctypes
import re

import pytest

import test_trunk_isa_cpu as isa

nat = pytest.importorskip("az_native")

NS = (0, 1, 1024, 16384, 16385, 1 << 24)
# Bytes reported by the library of the commit before the searches shared their front end,
# recorded from that library: {(max_empties or depth, split_plies): bytes for every n of NS}.
SOLVE = {
    (0, 0): (256, 256, 256, 256, 256, 256),
    (0, 1): (256, 3072, 90368, 1442048, 1442048, 1442048),
    (0, 2): (256, 3072, 135424, 270592, 270592, 270592),
    (1, 0): (256, 256, 256, 256, 256, 256),
    (1, 1): (256, 3072, 90368, 1442048, 1442048, 1442048),
    (1, 2): (256, 3072, 135424, 270592, 270592, 270592),
    (8, 0): (256, 256, 256, 256, 256, 256),
    (8, 1): (256, 3072, 405760, 6488320, 6488320, 6488320),
    (8, 2): (256, 5632, 2928896, 5857536, 5857536, 5857536),
    (12, 0): (256, 256, 256, 256, 256, 256),
    (12, 1): (256, 3072, 585984, 9371904, 9371904, 9371904),
    (12, 2): (256, 8192, 6533376, 13066496, 13066496, 13066496),
    (14, 0): (256, 256, 256, 256, 256, 256),
    (14, 1): (256, 3072, 676096, 10813696, 10813696, 10813696),
    (14, 2): (256, 10752, 8876288, 17752320, 17752320, 17752320),
}
DEEP = {
    (0, 0): (256, 256, 256, 256, 256, 256),
    (0, 1): (256, 3584, 94464, 1507584, 1507584, 1507584),
    (0, 2): (256, 3584, 141568, 282880, 282880, 282880),
    (1, 0): (256, 256, 256, 256, 256, 256),
    (1, 1): (256, 3584, 94464, 1507584, 1507584, 1507584),
    (1, 2): (256, 3584, 141568, 282880, 282880, 282880),
    (12, 0): (256, 256, 256, 256, 256, 256),
    (12, 1): (256, 3584, 612608, 9797888, 9797888, 9797888),
    (12, 2): (256, 8704, 6830336, 13660416, 13660416, 13660416),
    (16, 0): (256, 256, 256, 256, 256, 256),
    (16, 1): (256, 3584, 801024, 12812544, 12812544, 12812544),
    (16, 2): (256, 15360, 12105984, 24211712, 24211712, 24211712),
    (20, 0): (256, 256, 256, 256, 256, 256),
    (20, 1): (256, 3584, 989440, 15827200, 15827200, 15827200),
    (20, 2): (256, 20480, 18888960, 37777664, 37777664, 37777664),
}
SEARCH = {
    (1, 0): (256, 256, 256, 256, 256, 256),
    (1, 1): (256, 256, 256, 256, 256, 256),
    (1, 2): (256, 256, 256, 256, 256, 256),
    (2, 0): (256, 256, 256, 256, 256, 256),
    (2, 1): (256, 4096, 1601792, 25624832, 25624832, 25624832),
    (2, 2): (256, 256, 256, 256, 256, 256),
    (6, 0): (256, 256, 256, 256, 256, 256),
    (6, 1): (256, 4096, 1601792, 25624832, 25624832, 25624832),
    (6, 2): (256, 53760, 52898048, 52898048, 52898048, 52898048),
    (10, 0): (256, 256, 256, 256, 256, 256),
    (10, 1): (256, 4096, 1601792, 25624832, 25624832, 25624832),
    (10, 2): (256, 53760, 52898048, 52898048, 52898048, 52898048),
}
LEAF = {0: 256, 1: 1024, 65: 2304, 4096: 82176}


def query(fn, *args):
    need = ctypes.c_size_t(1)
    assert fn(*args, ctypes.byref(need), None) == nat.AZ_OK
    return need.value


def check_table(table, size_of):
    assert len(table) in (12, 15)
    for (param, split), want in table.items():
        got = tuple(size_of(n, param, split) for n in NS)
        assert got == want, (param, split, got, want)


def test_solve_workspace_bytes():
    check_table(SOLVE, lambda n, e, split: query(
        nat.lib.oth_solve_gpu, None, None, n, e, 100, split, None, None, None, None))


def test_solve_deep_workspace_bytes():
    check_table(DEEP, lambda n, e, split: query(
        nat.lib.oth_solve_deep_gpu, None, None, n, e, -65, 65, 100, split, None, None, None, None))


def test_search_workspace_bytes():
    check_table(SEARCH, lambda n, d, split: query(
        nat.lib.oth_search_gpu, None, None, n, d, 100, split, None, None, None, None))


def test_leaf_solve_workspace_bytes():
    for rows, want in LEAF.items():
        assert query(nat.lib.az_leaf_solve_gpu, None, None, rows, 12, 100, None) == want, rows


# name pattern: (block, frame bytes, {frames: LDS bytes}, vector registers of the commit before
# the kernels shared their loop, recorded from that library)
LANE_KERNELS = {
    r"7k_solveILi(\d+)E": (128, 20, {7: 17920, 11: 28160, 13: 33280}, 60),
    r"8k_searchILi(\d+)E": (128, 24, {3: 9216, 6: 18432, 9: 27648}, 61),
    r"12k_solve_deepILi(\d+)E": (64, 28, {11: 19712, 15: 26880, 19: 34048}, 91),
    r"12k_leaf_solveE": (64, 28, {11: 19712}, 94),
}


@pytest.fixture(scope="module")
def notes():
    return {k: v for k, v in isa.kernel_notes(isa.LIB).items() if not k.endswith(".kd")}


@isa.needs_tools
@pytest.mark.parametrize("pattern", list(LANE_KERNELS))
def test_lane_kernels_keep_their_resources(notes, pattern):
    block, frame_bytes, lds, vgprs = LANE_KERNELS[pattern]
    found = {}
    for k, n in notes.items():
        m = re.search(pattern, k)
        if m:
            found[int(m.group(1)) if m.groups() else 11] = n
    assert sorted(found) == sorted(lds), sorted(found)
    for nf, n in found.items():
        assert lds[nf] == nf * block * frame_bytes
        assert n["group_segment_fixed_size"] == lds[nf], (pattern, nf, n)
        assert n["private_segment_fixed_size"] == 0, (pattern, nf, n)
        assert n.get("vgpr_spill_count", 0) == 0, (pattern, nf, n)
        assert n["vgpr_count"] + n.get("agpr_count", 0) <= vgprs, (pattern, nf, n)
        assert n["max_flat_workgroup_size"] == block, (pattern, nf, n)


@isa.needs_tools
@pytest.mark.parametrize("part", ["expand", "combine", "finish"])
def test_split_front_kernels_use_no_lds_and_no_scratch(notes, part):
    found = {k: n for k, n in notes.items() if re.search(r"k_(split|deep)_" + part, k)}
    assert found, part
    for k, n in found.items():
        assert n["group_segment_fixed_size"] == 0, (k, n)
        assert n["private_segment_fixed_size"] == 0, (k, n)
        assert n.get("vgpr_spill_count", 0) == 0, (k, n)
