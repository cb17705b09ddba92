"""hsrans_decode_device_planes_gather_indirect without a device: the four entries are exported with the header's argument counts, the new
info struct mirrors the header, the control workspace's size function meets its contract, and null handles are refused before any device call."""
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
    "hsrans_planes_gather_indirect_workspace_bytes": (ctypes.c_size_t, 2),
    "hsrans_decode_device_planes_gather_indirect": (ctypes.c_int, 13),
    "hsrans_planes_gather_refused": (ctypes.c_int, 3),
    "hsrans_planes_gather_indirect_info": (ctypes.c_int, 5),
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
    m = re.search(r"typedef struct hsrans_planes_gather_indirect_info_t\s*\{(.*?)\}\s*hsrans_planes_gather_indirect_info_t;", _header(), flags=re.S)
    assert m, "hsrans_planes_gather_indirect_info_t is not declared"
    fields = [f.strip() for decl in m.group(1).split(";") if decl.strip() for f in re.sub(r"^\s*uint32_t", "", decl.strip()).split(",")]
    assert fields == ["coded", "stored", "max_rows", "merge_grid", "launches", "set_launches"]
    assert all(d.strip().startswith("uint32_t") for d in m.group(1).split(";") if d.strip())
    assert [n for n, _ in api.PlanesGatherIndirectInfo._fields_] == fields
    assert ctypes.sizeof(api.PlanesGatherIndirectInfo) == 4 * len(fields)
    # the struct the host-ranges call reports through is as it was
    assert ctypes.sizeof(api.PlanesGatherInfo) == 20
    for name in ("planes_gather_indirect_workspace_bytes", "PlanesGatherIndirectInfo"):
        assert hasattr(H, name), name
    for name in ("decode_device_planes_gather_indirect", "planes_gather_refused"):
        assert callable(getattr(H.Context, name)), name
    assert callable(H.PlanesGather.indirect_info)


SWEEP = [0, 1, 2, 3, 7, 64, 255, 256, 257, 1023, 1024, 1025, 4096, 4097, 10_000, 100_000, 1_000_003]


@pytest.mark.parametrize("W", [2, 4, 8])
def test_the_workspace_function_meets_its_contract(W):
    got = [H.planes_gather_indirect_workspace_bytes(W, c) for c in SWEEP]
    assert all(g > 0 and g % 256 == 0 for g in got), got
    assert got == sorted(got)
    for c, g in zip(SWEEP, got):
        # behind the header, the prefix, B_r and the rows lies the set's own workspace, sized for all planes coded
        rows_and_prefix = 32 * c * W + 8 * c + 4 * (c + 1)
        assert g >= H.gather_batch_workspace_bytes(W, c * W) + rows_and_prefix, c
    last = (1 << 31) // W - 1  # the largest count whose rows stay below 2^31
    assert H.planes_gather_indirect_workspace_bytes(W, last) >= got[-1]
    assert H.planes_gather_indirect_workspace_bytes(W, last + 1) == 0
    assert H.planes_gather_indirect_workspace_bytes(W, 0xFFFFFFFF) == 0


@pytest.mark.parametrize("W", [0, 1, 3, 5, 16])
def test_the_workspace_function_refuses_other_element_sizes(W):
    for c in (0, 1, 1000):
        assert H.planes_gather_indirect_workspace_bytes(W, c) == 0


def test_null_handles_are_refused_without_a_device():
    L = H.load_library()
    buf = (ctypes.c_uint8 * 4096)()
    p = ctypes.addressof(buf) + 255 & ~255
    info = api.PlanesGatherIndirectInfo()
    assert L.hsrans_decode_device_planes_gather_indirect(None, None, p, None, 1, 16, p, 64, p, 512, p, 4096, None) == E_ARG
    assert L.hsrans_decode_device_planes_gather_indirect(None, None, None, None, 0, 0, None, 0, None, 0, None, 0, None) == E_ARG
    assert L.hsrans_planes_gather_refused(None, None, None) == E_ARG
    assert L.hsrans_planes_gather_indirect_info(None, 1, 16, 64, ctypes.byref(info)) == E_ARG
    assert L.hsrans_planes_gather_indirect_info(None, 1, 16, 64, None) == E_ARG
