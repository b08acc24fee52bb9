"""The item schedule of the persistent key-side attention backward (csrc/ar_attn_sched.hpp, exported for the host as
ar_attn_bwd_grouped_run): every workgroup derives a fixed contiguous run of (batch, key head, 128-key block) items from its index alone.
No kernel is launched here."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from auto_round_amd import _lib

    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def _runs(lib, items, wgs):
    out = []
    for blk in range(wgs):
        first, count = ctypes.c_int64(-1), ctypes.c_int64(-1)
        assert lib.ar_attn_bwd_grouped_run(items, wgs, blk, ctypes.byref(first), ctypes.byref(count)) == 0
        out.append((first.value, count.value))
    return out


# (items, key blocks per (batch, key head), CUs): the grid is min(items, CUs)
CASES = [(8, 4, 256), (324, 9, 256), (1024, 16, 256), (4096, 16, 256), (1, 1, 256), (18, 3, 256), (1000, 8, 304), (37, 37, 8), (2048, 32, 512)]


@pytest.mark.parametrize("items,n_kb,cus", CASES)
def test_every_item_once_in_balanced_contiguous_runs(lib, items, n_kb, cus):
    wgs = min(items, cus)
    runs = _runs(lib, items, wgs)
    seen = [0] * items
    for first, count in runs:
        assert count >= 1 and 0 <= first and first + count <= items
        for i in range(first, first + count):
            seen[i] += 1
    assert seen == [1] * items                                           # every item assigned exactly once
    lengths = [c for _, c in runs]
    assert max(lengths) - min(lengths) <= 1                              # run lengths differ by at most one
    # (contiguity holds by construction once every run is one range of the item numbering, in which a (batch, key head) owns n_kb
    # consecutive numbers; checked from the owner map, not from the runs: the key blocks a workgroup holds of one (batch, key head)
    # have no foreign block between them, and a (batch, key head) is spread over no more workgroups than its size forces)
    owner = [None] * items
    for wg, (first, count) in enumerate(runs):
        for i in range(first, first + count):
            owner[i] = wg
    for g in range(items // n_kb):
        mine = owner[g * n_kb:(g + 1) * n_kb]
        for wg in set(mine):
            at = [k for k, o in enumerate(mine) if o == wg]
            assert at[-1] - at[0] + 1 == len(at)
        assert len(set(mine)) <= (n_kb + min(lengths) - 2) // min(lengths) + 1


@pytest.mark.parametrize("items,n_kb,cus", [c for c in CASES if min(c[0], c[2]) % 8 == 0])
def test_workgroups_of_one_xcd_hold_neighbouring_runs(lib, items, n_kb, cus):
    """workgroups go to the 8 XCDs round-robin: those with the same index % 8 take one contiguous span of the items, so the key blocks
    of a (batch, key head), which stream the same Q / dO rows, share an L2"""
    wgs = min(items, cus)
    runs = _runs(lib, items, wgs)
    for x in range(8):
        mine = sorted(runs[blk] for blk in range(x, wgs, 8))
        for (f0, c0), (f1, _) in zip(mine, mine[1:]):
            assert f0 + c0 == f1
        assert mine[0][0] == sum(c for blk in range(wgs) if blk % 8 < x for c in [runs[blk][1]])


def test_refuses_nonsense(lib):
    first, count = ctypes.c_int64(), ctypes.c_int64()
    for items, wgs, blk in ((0, 1, 0), (8, 0, 0), (8, 9, 0), (8, 4, 4), (8, 4, -1)):
        assert lib.ar_attn_bwd_grouped_run(items, wgs, blk, ctypes.byref(first), ctypes.byref(count)) == -1
