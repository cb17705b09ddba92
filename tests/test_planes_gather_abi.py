"""hsrans_decode_device_planes_gather without a device: the entries are exported with the header's argument counts, the structs mirror the
header, the workspace bound is its formula, and hsrans_planes_gather_tasks — the host-side cut of the merge — is a short Python model's."""
import ctypes
import os
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
    "hsrans_planes_gather_create": (ctypes.c_int, 5),
    "hsrans_planes_gather_destroy": (None, 1),
    "hsrans_planes_gather_workspace_bytes": (ctypes.c_size_t, 3),
    "hsrans_decode_device_planes_gather": (ctypes.c_int, 9),
    "hsrans_planes_gather_status": (ctypes.c_int, 4),
    "hsrans_planes_gather_info": (ctypes.c_int, 2),
    "hsrans_planes_gather_tasks": (ctypes.c_size_t, 5),
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
    assert re.search(r"typedef struct hsrans_planes_gather hsrans_planes_gather;", hdr)


def test_the_structs_mirror_the_header():
    assert ctypes.sizeof(api.Range) == 24
    assert ctypes.sizeof(api.PlanesGatherTask) == 32
    assert [api.PlanesGatherTask.src.offset, api.PlanesGatherTask.work_pos.offset, api.PlanesGatherTask.dst_delta.offset, api.PlanesGatherTask.lo.offset,
            api.PlanesGatherTask.hi.offset] == [0, 8, 16, 24, 28]
    assert ctypes.sizeof(api.PlanesGatherInfo) == 20
    assert [n for n, _ in api.PlanesGatherInfo._fields_] == ["coded", "stored", "rows", "merge_tasks", "launches"]
    for name in ("planes_gather_workspace_bytes", "planes_gather_tasks", "PlanesGather"):
        assert hasattr(H, name), name
    for name in ("make_planes_gather", "decode_device_planes_gather", "planes_gather_status"):
        assert callable(getattr(H.Context, name)), name


@pytest.mark.parametrize("W", [2, 4, 8])
def test_the_workspace_bound_is_its_formula(W):
    counts, totals = [0, 1, 2, 7, 64, 4097], [0, 1, 15, 16, 255, 256, 257, 4096, 70_001, 1_000_003]
    for count in counts:
        for total in totals:
            got = H.planes_gather_workspace_bytes(W, count, total)
            assert got == W * _up(total + 30 * count, 256) and got % 256 == 0, (count, total)
    for total in totals:
        row = [H.planes_gather_workspace_bytes(W, c, total) for c in counts]
        assert row == sorted(row), total
    for count in counts:
        col = [H.planes_gather_workspace_bytes(W, count, t) for t in totals]
        assert col == sorted(col), count


@pytest.mark.parametrize("W", [0, 1, 3, 16])
def test_the_workspace_bound_refuses_other_element_sizes(W):
    assert H.planes_gather_workspace_bytes(W, 4, 1000) == 0


# ---- the cut of the merge ----
def model_tasks(ranges, elements):
    """(src, work_pos, dst_delta mod 2^64, lo, hi) per task; None: a range beyond the tensor"""
    out, at = [], 0
    for off, n, dst in ranges:
        if off > elements or n > elements - off:
            return None
        phase, first = off % 16, off - off % 16
        for src in range(first, off + n if n else first, TASK):
            out.append((src, at + src - first, (dst - off) % 2**64, phase if src == first else 0, min(TASK, off + n - src)))
        at += _up(phase + n, 16) if n else 0
    return out


ELEMENTS = 300_007  # not a multiple of 16
LENGTHS = [1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 5]
CASES = [[(16 * 100 + phase, n, 3)] for phase in (0, 1, 15) for n in LENGTHS]
CASES += [
    [(ELEMENTS - n, n, 0)] for n in (1, 7, 17, 4097)  # ending on the tensor's last element
] + [
    [(5, 0, 0)], [(ELEMENTS, 0, 9)], [],              # empty ranges: no task
    [(0, 0, 0), (31, 4097, 100), (7, 0, 5), (16, 16, 0), (ELEMENTS - 3, 3, 50_000), (15, 2 * 4096 + 5, 7)],  # a list: B_r runs on past empty ranges
    [(4096 * 3 + 1, 20, 0), (4096 * 3 + 1, 20, 1 << 40)],  # the same elements twice
    [(100_000, 200_007, 0)],
]


@pytest.mark.parametrize("ranges", CASES, ids=[str(k) for k in range(len(CASES))])
def test_the_cut_is_the_models(ranges):
    want = model_tasks(ranges, ELEMENTS)
    got = H.planes_gather_tasks(ranges, ELEMENTS)
    assert got.shape == (len(want), 5)
    assert [tuple(int(v) for v in row) for row in got] == want
    # what the model's tasks mean: they tile each range in order, on the source's 16-element grid
    k = 0
    at = 0
    for off, n, dst in ranges:
        if n == 0:
            continue
        pos = off
        while pos < off + n:
            src, work_pos, delta, lo, hi = (int(v) for v in got[k])
            assert src % 16 == 0 and work_pos % 16 == 0 and lo < 16 and lo < hi <= TASK
            assert src + lo == pos, "the tasks of a range tile it in order"
            assert lo == (off % 16 if pos == off else 0)
            assert hi == TASK or src + hi == off + n, "only a range's last task is short"
            assert delta == (dst - off) % 2**64
            assert work_pos - at == src - (off - off % 16), "an element lies at B_r + phase + i of its region"
            pos = src + hi
            k += 1
        assert pos == off + n
        at += _up(off % 16 + n, 16)
    assert k == got.shape[0]
    assert at <= sum(n for _, n, _ in ranges) + 30 * len(ranges)  # what hsrans_planes_gather_workspace_bytes allows for


def test_the_cut_refuses_a_range_beyond_the_tensor():
    L = H.load_library()
    for bad in ([(ELEMENTS, 1, 0)], [(ELEMENTS + 1, 0, 0)], [(0, ELEMENTS + 1, 0)], [(0, 16, 0), (ELEMENTS - 15, 16, 0)], [(2**64 - 8, 16, 0)]):
        assert model_tasks(bad, ELEMENTS) is None
        assert H.planes_gather_tasks(bad, ELEMENTS).shape == (0, 5)
        arr = np.asarray(bad, np.uint64)
        assert L.hsrans_planes_gather_tasks(arr.ctypes.data, arr.shape[0], ELEMENTS, None, 0) == 0
    assert L.hsrans_planes_gather_tasks(None, 3, ELEMENTS, None, 0) == 0  # no ranges where some are counted


def test_the_cut_refuses_a_launch_of_2_to_the_31_tasks():
    """the bound hsrans_decode_device_planes_gather refuses by: a launch has fewer than 2^31 workgroups (the count alone: nothing is written)"""
    L = H.load_library()
    huge = 1 << 44

    def count(rows):
        arr = np.asarray(rows, np.uint64)
        return L.hsrans_planes_gather_tasks(arr.ctypes.data, arr.shape[0], huge, None, 0)

    assert count([(0, (2**31 - 1) * TASK, 0)]) == 2**31 - 1
    assert count([(0, 2**31 * TASK, 0)]) == 0
    assert count([(1, (2**31 - 1) * TASK, 0)]) == 0                      # the phase makes one task more
    assert count([(0, 2**30 * TASK, 0), (0, 2**30 * TASK, 0)]) == 0      # the total counts, not a range
    assert count([(0, 2**30 * TASK, 0), (16, (2**30 - 1) * TASK, 0)]) == 2**31 - 1


def test_the_cut_writes_no_more_than_capacity():
    ranges = [(3, 3 * 4096, 0)]
    assert H.planes_gather_tasks(ranges, ELEMENTS).shape[0] == 4
    got = H.planes_gather_tasks(ranges, ELEMENTS, capacity=2)
    assert got.shape[0] == 2 and np.array_equal(got, H.planes_gather_tasks(ranges, ELEMENTS)[:2])
