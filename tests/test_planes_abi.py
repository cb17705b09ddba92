"""The byte-plane layer without a device: the new entries are exported with their signatures, the size functions are the layout's
arithmetic, the host split / merge are the layout (plane p = byte p of every element, in memory order), and coding a bf16 tensor's
planes apart is smaller than coding its bytes as they lie."""
import ctypes
import os
import re

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

MT = H.MT
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _up256(v):
    return (v + 255) & ~255


SIGNATURES = {
    # name: (restype, number of arguments)
    "hsrans_planes_capacity": (ctypes.c_size_t, 3),
    "hsrans_planes_workspace_bytes": (ctypes.c_size_t, 2),
    "hsrans_planes_split": (ctypes.c_int, 4),
    "hsrans_planes_merge": (ctypes.c_int, 4),
    "hsrans_planes_split_device": (ctypes.c_int, 6),
    "hsrans_planes_merge_device": (ctypes.c_int, 6),
    "hsrans_encode_device_planes": (ctypes.c_size_t, 16),
    "hsrans_planes_create": (ctypes.c_int, 4),
    "hsrans_planes_destroy": (None, 1),
    "hsrans_decode_device_planes": (ctypes.c_int, 9),
    "hsrans_planes_status": (ctypes.c_int, 4),
    "hsrans_planes_info": (ctypes.c_int, 2),
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
    for macro in ("#define HSRANS_PLANES_MAX 8", "#define HSRANS_PLANES_STORE_INCOMPRESSIBLE 1u"):
        assert macro in hdr


def test_the_descriptor_mirrors_the_header():
    # 6 x u32, u64 elements, 8 + 8 x u64, u64 frame_length: no padding anywhere
    assert ctypes.sizeof(api.PlanesDesc) == 24 + 8 + 64 + 64 + 8
    assert api.PlanesDesc.elements.offset == 24 and api.PlanesDesc.offset.offset == 32 and api.PlanesDesc.length.offset == 96
    assert api.PlanesDesc.frame_length.offset == 160
    assert ctypes.sizeof(api.PlanesInfo) == 12
    assert api.PLANES_MAX == 8 and api.PLANES_STORE_INCOMPRESSIBLE == 1
    for name in ("planes_capacity", "planes_workspace_bytes", "planes_split", "planes_merge", "PlanesDesc", "Planes"):
        assert hasattr(H, name), name
    for name in ("planes_split_device", "planes_merge_device", "encode_device_planes", "make_planes", "decode_device_planes", "planes_status"):
        assert callable(getattr(H.Context, name)), name


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("states", [32, 64])
@pytest.mark.parametrize("n", [1, 15, 255, 256, 257, 65536, 1_000_003])
def test_the_size_functions_are_the_layouts_arithmetic(W, states, n):
    assert H.planes_capacity(W, states, n) == W * _up256(H.capacity(MT, states, n))
    assert H.planes_workspace_bytes(W, n) == W * _up256(n)


@pytest.mark.parametrize("W", [0, 1, 3, 16])
def test_the_size_functions_refuse_other_element_sizes(W):
    assert H.planes_capacity(W, 64, 1000) == 0
    assert H.planes_workspace_bytes(W, 1000) == 0


@pytest.mark.parametrize("W", [2, 4, 8])
def test_the_size_functions_refuse_no_elements_and_other_state_counts(W):
    assert H.planes_capacity(W, 64, 0) == 0
    assert H.planes_workspace_bytes(W, 0) == 0
    assert H.planes_capacity(W, 16, 1000) == 0


DTYPES = {2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 1025])
def test_host_split_and_merge_are_the_layout(W, n):
    rng = np.random.default_rng(1000 * W + n)
    a = rng.integers(0, 256, n * W, dtype=np.uint8).view(DTYPES[W])
    planes = H.planes_split(a)
    assert len(planes) == W
    rows = a.view(np.uint8).reshape(-1, W)
    for p in range(W):
        assert planes[p].dtype == np.uint8 and planes[p].shape == (n,)
        assert np.array_equal(planes[p], rows[:, p]), p
    back = H.planes_merge(planes, W)
    assert np.array_equal(back, a.view(np.uint8))
    assert np.array_equal(back, np.stack(planes, axis=1).reshape(-1))  # numpy's interleave


def test_host_split_and_merge_refuse_other_element_sizes():
    lib = H.load_library()
    buf = np.zeros(64, np.uint8)
    ptrs = (ctypes.c_void_p * 16)(*[buf.ctypes.data] * 16)
    for W in (0, 1, 3, 16):
        assert lib.hsrans_planes_split(W, buf.ctypes.data, 4, ptrs) == 2
        assert lib.hsrans_planes_merge(W, ptrs, 4, buf.ctypes.data) == 2
    assert lib.hsrans_planes_split(2, None, 4, ptrs) == 2
    assert lib.hsrans_planes_merge(2, None, 4, buf.ctypes.data) == 2
    with pytest.raises(H.HsransError):
        H.planes_split(np.zeros(8, np.uint8))
    with pytest.raises(H.HsransError):
        H.planes_merge([np.zeros(8, np.uint8)] * 2, 4)


def _bf16_bytes(n, seed):
    """n standard-normal values truncated to bf16: the upper two bytes of their fp32 (little-endian memory order)"""
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    return (x.view(np.uint32) >> 16).astype(np.uint16)


def test_planes_coded_apart_are_smaller_than_the_bytes_as_they_lie():
    a = _bf16_bytes(1 << 20, seed=17)
    together = H.encode(MT, 64, 11, a.view(np.uint8), block_size=1 << 16, independent_blocks=True).size
    apart = [H.encode(MT, 64, 11, p, block_size=1 << 16, independent_blocks=True).size for p in H.planes_split(a)]
    print(f"interleaved {together} bytes; planes {apart} = {sum(apart)} bytes ({sum(apart) / together:.4f})")
    assert sum(apart) < together
