"""hsrans_decode_device_planes_gather_batch_indirect without a device: the four entries are exported with the header's argument counts, the
new info struct mirrors the header (and the host-rows call's keeps its 24 bytes), the control workspace's size function meets its contract
on a grid of arguments, and null handles are refused before any device call."""
import ctypes
import os
import re

import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = 2

SIGNATURES = {
    # name: (restype, number of arguments)
    "hsrans_planes_gather_batch_indirect_workspace_bytes": (ctypes.c_size_t, 3),
    "hsrans_decode_device_planes_gather_batch_indirect": (ctypes.c_int, 12),
    "hsrans_planes_gather_set_refused": (ctypes.c_int, 3),
    "hsrans_planes_gather_set_indirect_info": (ctypes.c_int, 5),
}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hsrans_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_the_entries_are_exported_with_the_headers_argument_counts(name):
    lib = H.load_library()
    assert hasattr(lib, name), f"{name} is not exported"
    restype, n_args = SIGNATURES[name]
    fn = getattr(lib, name)
    assert fn.restype is restype
    assert len(fn.argtypes) == n_args
    m = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, _header())
    assert m, f"{name} is not declared in include/hsrans_hip.h"
    assert len(m.group(1).split(",")) == n_args


def test_the_info_struct_mirrors_the_header():
    m = re.search(r"typedef struct hsrans_planes_gather_set_indirect_info_t\s*\{(.*?)\}\s*hsrans_planes_gather_set_indirect_info_t;", _header(), flags=re.S)
    assert m, "hsrans_planes_gather_set_indirect_info_t is not declared"
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip() for f in re.sub(r"^\s*uint32_t", "", decl.strip()).split(",")]
    assert fields == ["members", "coded", "stored", "max_rows", "merge_grid", "launches", "set_launches"]
    assert all(d.strip().startswith("uint32_t") for d in m.group(1).split(";") if d.strip())
    assert [n for n, _ in api.PlanesGatherSetIndirectInfo._fields_] == fields
    assert ctypes.sizeof(api.PlanesGatherSetIndirectInfo) == 4 * len(fields)
    # the struct the host-rows call reports through is as it was
    assert ctypes.sizeof(api.PlanesGatherSetInfo) == 24
    for name in ("planes_gather_batch_indirect_workspace_bytes", "PlanesGatherSetIndirectInfo"):
        assert hasattr(H, name) and name in H.__all__, name
    for name in ("decode_device_planes_gather_batch_indirect", "planes_gather_set_refused"):
        assert callable(getattr(H.Context, name)), name
    assert callable(H.PlanesGatherSet.indirect_info)


COUNTS = [0, 1, 2, 3, 7, 64, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 4097, 10_000, 100_000, 1_000_003]
CODED = [0, 1, 2, 7, 8, 64, 1000, 65_535, 65_536]


@pytest.mark.parametrize("W", [2, 4, 8])
def test_the_workspace_function_meets_its_contract(W):
    size = H.planes_gather_batch_indirect_workspace_bytes
    grid = {(k, c): size(k, W, c) for k in CODED for c in COUNTS}
    assert all(g > 0 and g % 256 == 0 for g in grid.values()), grid
    for k in CODED:  # non-decreasing in max_count ...
        got = [grid[k, c] for c in COUNTS]
        assert got == sorted(got), (k, got)
    for c in COUNTS:  # ... and in coded_planes
        got = [grid[k, c] for k in CODED]
        assert got == sorted(got), (c, got)
    for (k, c), g in grid.items():
        # a header, first_task[max_count + 1], C_r and the first gather row per row, max_count * W rows of 32 bytes ...
        control = 256 + 4 * (c + 1) + 8 * c + 4 * c + 32 * c * W
        assert g >= control + (H.gather_batch_workspace_bytes(k, c * W) if k else 0), (k, c)  # ... and the set's own workspace behind them
        assert g == size(k, W, c)  # pure
    # no coded plane: the set's part is left out
    assert all(grid[0, c] < grid[1, c] and grid[0, c] < 256 + 512 + (16 + 32 * W) * c + 1024 for c in COUNTS)
    last = (1 << 31) // W - 1  # the largest count whose rows stay below 2^31
    for k in (0, 7):
        assert size(k, W, last) >= grid[k, COUNTS[-1]]
        assert size(k, W, last + 1) == 0
        assert size(k, W, 0xFFFFFFFF) == 0
    assert size(65_537, W, 10) == 0 and size(0xFFFFFFFF, W, 10) == 0


@pytest.mark.parametrize("W", [0, 1, 3, 5, 6, 16])
def test_the_workspace_function_refuses_other_element_sizes(W):
    for k in (0, 1, 9):
        for c in (0, 1, 1000):
            assert H.planes_gather_batch_indirect_workspace_bytes(k, W, c) == 0


def test_null_handles_are_refused_without_a_device():
    L = H.load_library()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf) + 255 & ~255
    info = api.PlanesGatherSetIndirectInfo()
    assert L.hsrans_decode_device_planes_gather_batch_indirect(None, None, p, None, 1, p, 64, p, 512, p, 4096, None) == E_ARG
    assert L.hsrans_decode_device_planes_gather_batch_indirect(None, None, None, None, 0, None, 0, None, 0, None, 0, None) == E_ARG
    assert L.hsrans_planes_gather_set_refused(None, None, None) == E_ARG
    assert L.hsrans_planes_gather_set_indirect_info(None, 1, 64, 512, ctypes.byref(info)) == E_ARG
    assert L.hsrans_planes_gather_set_indirect_info(None, 1, 64, 512, None) == E_ARG
