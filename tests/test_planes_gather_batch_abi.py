"""hsrans_decode_device_planes_gather_batch without a device: the entries are exported with the header's argument counts, the structs mirror
the header, the workspace bound is its formula, and hsrans_planes_gather_batch_tasks — the host-side cut of the merge over rows of mixed
element sizes — is a short Python model's: C_r and slot_r as the header lays the workspace out, each row's tasks taken from
hsrans_planes_gather_tasks on that row alone."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASK = 4096


def _up(v, a):
    return (v + a - 1) // a * a


SIGNATURES = {
    # name: (restype, number of arguments)
    "hsrans_planes_gather_set_create": (ctypes.c_int, 5),
    "hsrans_planes_gather_set_destroy": (None, 1),
    "hsrans_planes_gather_batch_workspace_bytes": (ctypes.c_size_t, 3),
    "hsrans_decode_device_planes_gather_batch": (ctypes.c_int, 9),
    "hsrans_planes_gather_set_status": (ctypes.c_int, 4),
    "hsrans_planes_gather_set_info": (ctypes.c_int, 2),
    "hsrans_planes_gather_batch_tasks": (ctypes.c_size_t, 7),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_the_entries_are_exported_with_their_signatures(name):
    lib = H.load_library()
    assert hasattr(lib, name), f"{name} is not exported"
    restype, n_args = SIGNATURES[name]
    fn = getattr(lib, name)
    assert fn.restype is restype
    assert len(fn.argtypes) == n_args


def test_the_binding_has_the_headers_argument_counts():
    hdr = open(os.path.join(ROOT, "include", "hsrans_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name, (_, n_args) in SIGNATURES.items():
        m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, hdr)
        assert m, f"{name} is not declared in include/hsrans_hip.h"
        assert len(m.group(1).split(",")) == n_args, name
    # (the eighth entry of the interface is the handle's type)
    assert re.search(r"typedef struct hsrans_planes_gather_set hsrans_planes_gather_set;", hdr)


def test_the_structs_mirror_the_header():
    T = api.PlanesGatherBatchTask
    assert ctypes.sizeof(T) == 48
    assert [n for n, _ in T._fields_] == ["src", "work_pos", "plane_step", "dst_delta", "lo", "hi", "member", "reserved"]
    assert [getattr(T, n).offset for n, _ in T._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert ctypes.sizeof(api.MemberRange) == 32
    assert ctypes.sizeof(api.PlanesGatherSetInfo) == 24
    assert [n for n, _ in api.PlanesGatherSetInfo._fields_] == ["members", "coded", "stored", "rows", "merge_tasks", "launches"]
    for name in ("planes_gather_batch_workspace_bytes", "planes_gather_batch_tasks", "PlanesGatherSet", "PlanesGatherBatchTask", "PlanesGatherSetInfo"):
        assert hasattr(H, name), name
    for name in ("make_planes_gather_set", "decode_device_planes_gather_batch", "planes_gather_set_status"):
        assert callable(getattr(H.Context, name)), name
    assert callable(H.PlanesGatherSet.info)


@pytest.mark.parametrize("W", [2, 4, 8])
def test_the_workspace_bound_is_its_formula(W):
    counts, totals = [0, 1, 2, 7, 64, 4097], [0, 1, 15, 16, 255, 256, 257, 4096, 70_001, 1_000_003]
    for count in counts:
        for total in totals:
            got = H.planes_gather_batch_workspace_bytes(W, count, total)
            assert got == _up(W * (total + 30 * count), 256), (count, total)


@pytest.mark.parametrize("W", [0, 1, 3, 16])
def test_the_workspace_bound_refuses_other_element_sizes(W):
    assert H.planes_gather_batch_workspace_bytes(W, 4, 1000) == 0


def test_the_workspace_bound_refuses_an_overflow():
    assert H.planes_gather_batch_workspace_bytes(2, 0, 2**63 - 256) == 2**64 - 512
    assert H.planes_gather_batch_workspace_bytes(2, 0, 2**63) == 0           # the product wraps
    assert H.planes_gather_batch_workspace_bytes(2, 0, 2**63 - 100) == 0     # the rounding up wraps
    assert H.planes_gather_batch_workspace_bytes(8, 2**32 - 1, 2**64 - 1) == 0  # the sum wraps
    assert H.planes_gather_batch_workspace_bytes(8, 1, 2**61) == 0


# ---- the cut of the merge ----
def model_tasks(rows, itemsizes, elements):
    """(src, work_pos, plane_step, dst_delta mod 2^64, lo, hi, member) per task, from the single call's cut of each row alone"""
    out, at = [], 0
    for m, off, n, dst in rows:
        slot = _up(off % 16 + n, 16) if n else 0
        for src, work_pos, delta, lo, hi in H.planes_gather_tasks([(off, n, dst)], elements[m]):
            out.append((int(src), at + int(work_pos), slot, int(delta), int(lo), int(hi), m))
        at += itemsizes[m] * slot
    return out, at


ITEMSIZES = [4, 2, 8, 2, 4, 8]  # (shuffled: no order among the members' element sizes)
ELEMENTS = [300_007, 70_001, 20_003, 5_000, 4_097, 100_000]


def _rows():
    rows = [(2, 5, 0, 0)]  # an empty row: no task, no workspace
    k = 0
    for phase in (0, 1, 15):
        for n in (1, 15, 16, 17, 4095, 4097):
            m = k % 6 if ELEMENTS[k % 6] >= 32 + phase + n else 0
            rows.append((m, 32 + phase, n, 1000 * k + 3))
            k += 1
    rows += [(m, ELEMENTS[m] - n, n, 7) for m, n in ((1, 1), (3, 17), (4, 4097), (5, 4097))]  # rows that end with their tensors
    rows += [(0, 100_000, 200_007, 0), (3, 0, 5_000, 1 << 40), (4, ELEMENTS[4], 0, 9)]
    random.Random(5).shuffle(rows)
    return rows


ROWS = _rows()


def test_the_cut_is_the_models():
    want, work = model_tasks(ROWS, ITEMSIZES, ELEMENTS)
    got = H.planes_gather_batch_tasks(ROWS, ITEMSIZES, ELEMENTS)
    assert got.shape == (len(want), 7) and len(want) > len(ROWS)
    assert [tuple(int(v) for v in row) for row in got] == want
    assert {int(m) for m in got[:, 6]} == set(range(6)), "members of every element size take part"
    # what the layout means: the sub-slots of a task's planes lie inside the call's workspace, rows do not share them
    assert all(int(t[1]) % 16 == 0 and int(t[2]) % 16 == 0 for t in got)
    assert max(int(t[1]) + (ITEMSIZES[int(t[6])] - 1) * int(t[2]) + int(t[5]) for t in got) <= work
    assert work <= H.planes_gather_batch_workspace_bytes(8, len(ROWS), sum(r[2] for r in ROWS))


@pytest.mark.parametrize("row", sorted(set(ROWS)), ids=lambda r: "m%d_o%d_n%d" % r[:3])
def test_the_cut_of_one_row_is_the_single_calls(row):
    m, off, n, dst = row
    single = H.planes_gather_tasks([(off, n, dst)], ELEMENTS[m])
    got = H.planes_gather_batch_tasks([row], ITEMSIZES, ELEMENTS)
    assert got.shape[0] == single.shape[0]
    assert np.array_equal(got[:, [0, 1, 3, 4, 5]], single)
    assert all(int(t[2]) == _up(off % 16 + n, 16) and int(t[6]) == m for t in got)


def _raw_count(rows, itemsizes, elements, reserved=0):
    L = H.load_library()
    arr = (api.MemberRange * max(len(rows), 1))()
    for k, (m, off, n, dst) in enumerate(rows):
        arr[k].member, arr[k].offset, arr[k].length, arr[k].dst_offset, arr[k].reserved = m, off, n, dst, reserved
    sizes, elems = (ctypes.c_uint32 * len(itemsizes))(*itemsizes), (ctypes.c_uint64 * len(elements))(*elements)
    return L.hsrans_planes_gather_batch_tasks(arr, len(rows), sizes, elems, len(itemsizes), None, 0)


def test_the_cut_returns_the_count_alone_with_no_capacity():
    want, _ = model_tasks(ROWS, ITEMSIZES, ELEMENTS)
    assert _raw_count(ROWS, ITEMSIZES, ELEMENTS) == len(want)
    assert H.planes_gather_batch_tasks(ROWS, ITEMSIZES, ELEMENTS, capacity=0).shape == (0, 7)
    got = H.planes_gather_batch_tasks(ROWS, ITEMSIZES, ELEMENTS, capacity=3)
    assert [tuple(int(v) for v in row) for row in got] == want[:3]


def test_the_cut_refuses_what_the_call_refuses():
    good = [(1, 16, 100, 0), (5, 0, 10, 0)]
    assert _raw_count(good, ITEMSIZES, ELEMENTS) == 2
    assert _raw_count([(6, 0, 1, 0)], ITEMSIZES, ELEMENTS) == 0, "member >= members"
    assert _raw_count(good + [(6, 0, 0, 0)], ITEMSIZES, ELEMENTS) == 0, "... of an empty row too"
    assert _raw_count(good, ITEMSIZES, ELEMENTS, reserved=1) == 0, "reserved != 0"
    assert _raw_count([(1, ELEMENTS[1] - 4, 4, 0)], ITEMSIZES, ELEMENTS) == 1
    assert _raw_count(good + [(1, ELEMENTS[1] - 4, 5, 0)], ITEMSIZES, ELEMENTS) == 0, "a row one element beyond its member"
    assert _raw_count([(3, ELEMENTS[3] + 1, 0, 0)], ITEMSIZES, ELEMENTS) == 0
    assert _raw_count([(3, ELEMENTS[3], 1, 0)], ITEMSIZES, ELEMENTS) == 0
    assert _raw_count([(1, ELEMENTS[3], 1, 0)], ITEMSIZES, ELEMENTS) == 1, "a row is measured against its own member"
    assert _raw_count(good, [4, 2, 8, 2, 4, 3], ELEMENTS) == 0, "an element size that is not 2, 4 or 8"
    L = H.load_library()
    assert L.hsrans_planes_gather_batch_tasks(None, 3, None, None, 0, None, 0) == 0  # no rows where some are counted


def test_the_cut_refuses_a_launch_of_2_to_the_31_tasks():
    """the bound hsrans_decode_device_planes_gather_batch refuses by: a launch has fewer than 2^31 workgroups (the count alone: nothing is
    written); reached by arithmetic on huge element counts, over members of different element sizes"""
    sizes, huge = [2, 8], [1 << 44, 1 << 44]
    assert _raw_count([(0, 0, (2**31 - 1) * TASK, 0)], sizes, huge) == 2**31 - 1
    assert _raw_count([(0, 0, 2**31 * TASK, 0)], sizes, huge) == 0
    assert _raw_count([(1, 1, (2**31 - 1) * TASK, 0)], sizes, huge) == 0                         # the phase makes one task more
    assert _raw_count([(0, 0, 2**30 * TASK, 0), (1, 0, 2**30 * TASK, 0)], sizes, huge) == 0      # the total counts, not a row or a member
    assert _raw_count([(0, 0, 2**30 * TASK, 0), (1, 16, (2**30 - 1) * TASK, 0)], sizes, huge) == 2**31 - 1
