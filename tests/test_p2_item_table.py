"""The P2 item table (mi_p2_item_table: host only).

P2 of the articulated substep sums each link's record (four float4 slots) with its descendants'
records, in descendant-list order. In the paired kernel the work items are the (link, slot) pairs,
links ranked by descendant count, longest first, dealt to the 32 lanes of a half in passes
(mi_pair.hpp pair_p2_composites). The host entry ranks the links (p2_link_order), packs the order
into 64-bit words (p2_pack) and reads every item back out of the words (p2_item -> p2_unpack),
all mi_topo.hpp; the kernel reads its items out of the same words, built by the same functions
at compile time, through p2_unpack, and a static_assert next to it holds its indexing to p2_item
for every pass and lane. So the ranking, the packing and the decode are what this file sees; that
the kernel's fold then gives the bits it gave before is held by tests/test_gpu_phase_share.py
(recorded arrays) on the GPU. The table is also defined for 64 lanes (no kernel uses that width:
the one-env-per-wave kernels keep lane = link). Checked for the Humanoid, Ant and Cartpole link
trees and a chain of 33 links (the largest tree mi_sim_create accepts), on both widths:
  * every (link, slot) is held exactly once; a lane holds at most one item per pass (the table has
    one entry per pass and lane); a lane's items all have slot lane & 3 (what the kernel assumes);
  * items come longest list first: in pass-major, lane-minor order the descendant counts never rise;
  * the record reads of any lane (one per descendant and item) are at most
    ceil(total reads / lanes) + the longest single list;
  * a numpy restatement of the fold over the table gives, on random float32 records, arrays
    bit-equal to the lane = link fold (own record, then the descendants in increasing index order,
    a left fold) that the kernels ran before the table. Both folds walk the same lists, so beyond
    the coverage check this shows only that a slot's sum does not depend on the other slots."""
import ctypes as C

import numpy as np
import pytest

from omniisaacgymenvs_amd import native as N
from omniisaacgymenvs_amd.robots.model import load_robot

TREES = {name: np.asarray(load_robot(name).parent, np.int32) for name in ("Humanoid", "Ant", "Cartpole")}
TREES["chain33"] = np.arange(-1, 32, dtype=np.int32)
CASES = [(name, w) for name in TREES for w in (32, 64)]


def table(parent, lanes):
    lib = N.load_library()
    L = int(parent.size)
    passes = C.c_int32(-1)
    par = np.ascontiguousarray(parent, np.int32)
    pp = par.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.mi_p2_item_table(pp, L, lanes, None, 0, C.byref(passes)) == 0
    assert passes.value == -(-4 * L // lanes)
    items = np.full(passes.value * lanes, -7, np.int32)
    assert lib.mi_p2_item_table(pp, L, lanes, items.ctypes.data_as(C.POINTER(C.c_int32)), items.size,
                                C.byref(passes)) == 0
    return items.reshape(passes.value, lanes)


def descendants(parent):
    """desc[l]: descendants of l in increasing index order (mi_sim_create's desc_list)."""
    L = parent.size
    out = [[] for _ in range(L)]
    for c in range(1, L):
        x = parent[c]
        while x >= 0:
            out[x].append(c)
            x = parent[x]
    return [sorted(d) for d in out]


@pytest.mark.parametrize("name,lanes", CASES)
def test_table_covers_every_item_once_and_is_balanced(name, lanes):
    parent = TREES[name]
    L = int(parent.size)
    assert parent[0] == -1 and all(0 <= parent[l] < l for l in range(1, L))
    desc = descendants(parent)
    tab = table(parent, lanes)
    held = tab[tab >= 0]
    assert sorted(held.tolist()) == list(range(4 * L)), "every (link, slot) exactly once"
    assert set(np.unique(tab[tab < 0]).tolist()) <= {-1}
    for p in range(tab.shape[0]):
        for ln in range(lanes):
            if tab[p, ln] >= 0:
                assert tab[p, ln] % 4 == ln % 4, "a lane works on slot lane & 3"
    counts = [len(desc[it // 4]) for it in tab.reshape(-1) if it >= 0]
    assert all(a >= b for a, b in zip(counts, counts[1:])), "longest list first"
    assert (tab.reshape(-1)[:4 * L] >= 0).all(), "no idle lane ahead of an item"
    reads = np.array([sum(len(desc[it // 4]) for it in tab[:, ln] if it >= 0) for ln in range(lanes)])
    total, longest = 4 * sum(len(d) for d in desc), max(len(d) for d in desc)
    assert reads.sum() == total
    print(f"[p2-items] {name} L {L} lanes {lanes}: passes {tab.shape[0]}, reads per lane max {reads.max()} "
          f"(lane = link: {4 * longest}), total {total}, bound {-(-total // lanes) + longest}")
    assert reads.max() <= -(-total // lanes) + longest


@pytest.mark.parametrize("name,lanes", CASES)
def test_fold_over_the_table_is_bit_equal_to_the_link_fold(name, lanes):
    parent = TREES[name]
    L = int(parent.size)
    desc = descendants(parent)
    rng = np.random.default_rng(5)
    # magnitudes spread over several binades, so that a different order of the additions rounds differently
    recs = (rng.standard_normal((L, 4, 4)) * 10.0 ** rng.integers(-3, 4, (L, 4, 4))).astype(np.float32)
    want = np.empty_like(recs)
    for l in range(L):            # lane = link: the four slots together, descendants in list order
        acc = recs[l].copy()
        for d in desc[l]:
            acc = acc + recs[d]
        want[l] = acc
    assert want.dtype == np.float32
    got = np.full_like(recs, np.nan)
    for p, row in enumerate(table(parent, lanes)):
        for ln, it in enumerate(row):
            if it < 0:
                continue
            l, s = divmod(int(it), 4)
            acc = recs[l, s].copy()
            for d in desc[l]:
                acc = acc + recs[d, s]
            got[l, s] = acc
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if L > 2:
        # the check can tell orders apart: the reversed fold differs somewhere
        rev = np.stack([recs[l] + sum((recs[d] for d in reversed(desc[l])), np.zeros((4, 4), np.float32))
                        for l in range(L)])
        assert not np.array_equal(rev.view(np.uint32), want.view(np.uint32))


def test_bad_arguments_are_refused():
    lib = N.load_library()
    par = TREES["Ant"]
    pp = par.ctypes.data_as(C.POINTER(C.c_int32))
    n = C.c_int32(0)
    small = np.zeros(8, np.int32)
    assert lib.mi_p2_item_table(pp, par.size, 48, None, 0, C.byref(n)) != 0          # lanes
    assert lib.mi_p2_item_table(pp, 0, 32, None, 0, C.byref(n)) != 0                 # L
    assert lib.mi_p2_item_table(pp, par.size, 32, small.ctypes.data_as(C.POINTER(C.c_int32)), small.size,
                                C.byref(n)) != 0                                     # room
    bad = np.array([-1, 2, 0], np.int32)                                             # a parent after its child
    assert lib.mi_p2_item_table(bad.ctypes.data_as(C.POINTER(C.c_int32)), 3, 32, None, 0, C.byref(n)) != 0
