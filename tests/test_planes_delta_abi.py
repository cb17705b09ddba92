"""Tensors coded against a base, without a device: the host statement of the rule — hsrans_planes_split_delta is the split of a ^ b,
hsrans_planes_merge_delta its inverse, also over the base itself — with their refusals, and the new entries exported with the header's
argument counts and listed in the binding's signature table."""
import ctypes

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import _abi

E_ARG = 2
NP_UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
SIZES = [1, 15, 16, 17, 1025]

# name -> (restype, number of arguments), as include/hsrans_hip.h declares them
SIGNATURES = {
    "hsrans_planes_split_delta": (ctypes.c_int, 5),
    "hsrans_planes_merge_delta": (ctypes.c_int, 5),
    "hsrans_planes_split_delta_device": (ctypes.c_int, 7),
    "hsrans_planes_merge_delta_device": (ctypes.c_int, 7),
    "hsrans_encode_device_planes_delta": (ctypes.c_size_t, 18),
    "hsrans_decode_device_planes_delta": (ctypes.c_int, 11),
    "hsrans_encode_device_planes_delta_batch": (ctypes.c_int, 10),
    "hsrans_decode_device_planes_delta_batch": (ctypes.c_int, 11),
    "hsrans_decode_device_planes_gather_delta": (ctypes.c_int, 11),
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_the_entries_are_exported_and_in_the_signature_table(name):
    lib = H.load_library()
    assert hasattr(lib, name), f"{name} is not exported"
    restype, n_args = SIGNATURES[name]
    assert name in _abi.SIGNATURES, name
    assert _abi.SIGNATURES[name][0] is restype and len(_abi.SIGNATURES[name][1]) == n_args
    fn = getattr(lib, name)
    assert fn.restype is restype and len(fn.argtypes) == n_args


def test_the_python_names_exist():
    assert callable(H.planes_split_delta) and callable(H.planes_merge_delta)
    for method in ("planes_split_delta_device", "planes_merge_delta_device", "encode_device_planes_delta", "decode_device_planes_delta",
                   "encode_device_planes_delta_batch", "decode_device_planes_delta_batch", "decode_device_planes_gather_delta"):
        assert callable(getattr(H.Context, method)), method


def _pair(W, n):
    rng = np.random.default_rng(W * 1000 + n)
    a = rng.integers(0, 256, n * W, dtype=np.uint8).view(NP_UINT[W])
    b = rng.integers(0, 256, n * W, dtype=np.uint8).view(NP_UINT[W])
    return a, b


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_the_host_split_is_the_split_of_the_xor(W, n):
    a, b = _pair(W, n)
    got = H.planes_split_delta(a, b)
    want = (a ^ b).view(np.uint8).reshape(-1, W)
    assert len(got) == W
    for p in range(W):
        assert got[p].dtype == np.uint8 and np.array_equal(got[p], want[:, p]), p
    # ... which is what the plain split gives for a ^ b, and the plain split of `a` against a base of zeros
    for p, plane in enumerate(H.planes_split(a ^ b)):
        assert np.array_equal(got[p], plane), p
    for p, plane in enumerate(H.planes_split_delta(a, np.zeros_like(a))):
        assert np.array_equal(plane, a.view(np.uint8).reshape(-1, W)[:, p]), p


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_the_host_merge_is_its_inverse(W, n):
    a, b = _pair(W, n)
    planes = H.planes_split_delta(a, b)
    assert np.array_equal(H.planes_merge_delta(planes, b), a.view(np.uint8))
    assert np.array_equal(H.planes_merge(planes, W), (a ^ b).view(np.uint8))  # the plain merge gives the residue
    # in place: the output is the base's own buffer
    L = H.load_library()
    buf = b.copy()
    ptrs = (ctypes.c_void_p * W)(*[p.ctypes.data for p in planes])
    assert L.hsrans_planes_merge_delta(W, ptrs, buf.ctypes.data, n, buf.ctypes.data) == 0
    assert np.array_equal(buf, a)


def test_the_host_functions_refuse_bad_arguments():
    L = H.load_library()
    a, b = _pair(4, 64)
    out = np.full(4 * 64 + 8, 0xA5, np.uint8)
    planes = [np.full(64 + 8, 0xA5, np.uint8) for _ in range(4)]
    ptrs = (ctypes.c_void_p * 8)(*[p.ctypes.data for p in planes])
    holed = (ctypes.c_void_p * 8)(planes[0].ctypes.data, None, planes[2].ctypes.data, planes[3].ctypes.data)
    for W in (0, 1, 3, 5, 16):
        assert L.hsrans_planes_split_delta(W, a.ctypes.data, b.ctypes.data, 64, ptrs) == E_ARG, W
        assert L.hsrans_planes_merge_delta(W, ptrs, b.ctypes.data, 64, out.ctypes.data) == E_ARG, W
    assert L.hsrans_planes_split_delta(4, None, b.ctypes.data, 64, ptrs) == E_ARG
    assert L.hsrans_planes_split_delta(4, a.ctypes.data, None, 64, ptrs) == E_ARG
    assert L.hsrans_planes_split_delta(4, a.ctypes.data, b.ctypes.data, 64, None) == E_ARG
    assert L.hsrans_planes_split_delta(4, a.ctypes.data, b.ctypes.data, 64, holed) == E_ARG
    assert L.hsrans_planes_merge_delta(4, ptrs, None, 64, out.ctypes.data) == E_ARG
    assert L.hsrans_planes_merge_delta(4, ptrs, b.ctypes.data, 64, None) == E_ARG
    assert L.hsrans_planes_merge_delta(4, None, b.ctypes.data, 64, out.ctypes.data) == E_ARG
    assert L.hsrans_planes_merge_delta(4, holed, b.ctypes.data, 64, out.ctypes.data) == E_ARG
    assert np.all(out == 0xA5) and all(np.all(p == 0xA5) for p in planes)
    # the wrappers: a base of another shape
    with pytest.raises(H.HsransError):
        H.planes_split_delta(a, b[:-1])
    with pytest.raises(H.HsransError):
        H.planes_split_delta(a, b.view(np.uint16))
    with pytest.raises(H.HsransError):
        H.planes_merge_delta(H.planes_split(a)[:3], b)
