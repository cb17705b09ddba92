"""Tensors coded against a base as a zigzag difference, without a device: the host statement of the rule — hsrans_planes_split_diff is the
split of z = zigzag(a - b), the elements read as little-endian unsigned integers, hsrans_planes_merge_diff its inverse, also over the base
itself — on random pairs and on the pairs where a carry or a borrow runs through the element (planes_diff_cases.py), with their refusals,
and the nine new entries exported with the header's argument counts and listed in the binding's signature table."""
import ctypes

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import _abi
from planes_diff_cases import NP_UINT, carry_cases, planes_of, planted, unzigzag, zigzag

E_ARG = 2
SIZES = [1, 15, 16, 17, 1025]

# name -> (restype, number of arguments), as include/hsrans_hip.h declares them: each its _delta twin's
SIGNATURES = {
    "hsrans_planes_split_diff": (ctypes.c_int, 5),
    "hsrans_planes_merge_diff": (ctypes.c_int, 5),
    "hsrans_planes_split_diff_device": (ctypes.c_int, 7),
    "hsrans_planes_merge_diff_device": (ctypes.c_int, 7),
    "hsrans_encode_device_planes_diff": (ctypes.c_size_t, 18),
    "hsrans_decode_device_planes_diff": (ctypes.c_int, 11),
    "hsrans_encode_device_planes_diff_batch": (ctypes.c_int, 10),
    "hsrans_decode_device_planes_diff_batch": (ctypes.c_int, 11),
    "hsrans_decode_device_planes_gather_diff": (ctypes.c_int, 11),
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
    twin = name.replace("_diff", "_delta")  # the same argument list, type for type
    assert _abi.SIGNATURES[name] == _abi.SIGNATURES[twin], twin


def test_the_python_names_exist():
    assert callable(H.planes_split_diff) and callable(H.planes_merge_diff)
    for method in ("planes_split_diff_device", "planes_merge_diff_device", "encode_device_planes_diff", "decode_device_planes_diff",
                   "encode_device_planes_diff_batch", "decode_device_planes_diff_batch", "decode_device_planes_gather_diff"):
        assert callable(getattr(H.Context, method)), method


def test_the_numpy_rule_is_the_written_rule():
    """the reference every test leans on, against the rule worked by hand in Python integers"""
    for W in (2, 4, 8):
        a, b = carry_cases(W)
        mod = 1 << (8 * W)
        want = []
        for x, y in zip(a.tolist(), b.tolist()):
            d = (x - y) % mod
            want.append(((d << 1) ^ (0 - (d >> (8 * W - 1)))) % mod)
        z = zigzag(a, b)
        assert z.dtype == a.dtype and z.tolist() == want, W
        assert want[0] == 2 and want[1] == mod - 1 and want[2] == 2  # d = +1, d = 2^(8 W - 1), d = +1
        assert np.array_equal(unzigzag(z, b), a), W


def _pair(W, n):
    rng = np.random.default_rng(W * 1000 + n)
    a = rng.integers(0, 256, n * W, dtype=np.uint8).view(NP_UINT[W])
    b = rng.integers(0, 256, n * W, dtype=np.uint8).view(NP_UINT[W])
    return a, b


def _check_split_and_merge(a, b):
    W, n = a.itemsize, a.size
    want = planes_of(zigzag(a, b))
    got = H.planes_split_diff(a, b)
    assert len(got) == W
    for p in range(W):
        assert got[p].dtype == np.uint8 and np.array_equal(got[p], want[p]), p
    # ... which is what the plain split gives for z; against a base of zeros z is the element doubled, or its complement doubled plus one
    for p, plane in enumerate(H.planes_split(zigzag(a, b))):
        assert np.array_equal(got[p], plane), p
    assert np.array_equal(H.planes_merge_diff(got, b), a.view(np.uint8))
    assert np.array_equal(H.planes_merge(got, W), zigzag(a, b).view(np.uint8))  # the plain merge gives z
    # in place: the output is the base's own buffer
    L = H.load_library()
    buf = b.copy()
    ptrs = (ctypes.c_void_p * W)(*[p.ctypes.data for p in got])
    assert L.hsrans_planes_merge_diff(W, ptrs, buf.ctypes.data, n, buf.ctypes.data) == 0
    assert np.array_equal(buf, a)


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_the_host_split_is_the_split_of_z_and_the_merge_inverts_it(W, n):
    _check_split_and_merge(*_pair(W, n))


@pytest.mark.parametrize("W", [2, 4, 8])
def test_the_host_rule_on_the_carry_cases(W):
    a, b, starts = planted(W, 7)
    ca, cb = carry_cases(W)
    assert all(np.array_equal(a[s: s + ca.size], ca) and np.array_equal(b[s: s + cb.size], cb) for s in starts)
    _check_split_and_merge(a, b)
    _check_split_and_merge(ca, cb)


def test_a_tensor_against_itself_is_all_zero_planes_and_xor_is_another_rule():
    a, b = _pair(2, 1025)
    assert all(not p.any() for p in H.planes_split_diff(a, a))
    one_ulp = (a + np.uint16(1)).astype(np.uint16)
    assert all(np.all(p == (2 if k == 0 else 0)) for k, p in enumerate(H.planes_split_diff(one_ulp, a)))  # z = 2 whatever carries
    assert any(not np.array_equal(x, y) for x, y in zip(H.planes_split_diff(a, b), H.planes_split_delta(a, b)))


def test_the_host_functions_refuse_what_the_delta_ones_refuse():
    L = H.load_library()
    a, b = _pair(4, 64)
    out = np.full(4 * 64 + 8, 0xA5, np.uint8)
    planes = [np.full(64 + 8, 0xA5, np.uint8) for _ in range(4)]
    ptrs = (ctypes.c_void_p * 8)(*[p.ctypes.data for p in planes])
    holed = (ctypes.c_void_p * 8)(planes[0].ctypes.data, None, planes[2].ctypes.data, planes[3].ctypes.data)
    split_calls = [(W, a.ctypes.data, b.ctypes.data, 64, ptrs) for W in (0, 1, 3, 5, 16)]
    split_calls += [(4, None, b.ctypes.data, 64, ptrs), (4, a.ctypes.data, None, 64, ptrs), (4, a.ctypes.data, b.ctypes.data, 64, None),
                    (4, a.ctypes.data, b.ctypes.data, 64, holed)]
    merge_calls = [(W, ptrs, b.ctypes.data, 64, out.ctypes.data) for W in (0, 1, 3, 5, 16)]
    merge_calls += [(4, ptrs, None, 64, out.ctypes.data), (4, ptrs, b.ctypes.data, 64, None), (4, None, b.ctypes.data, 64, out.ctypes.data),
                    (4, holed, b.ctypes.data, 64, out.ctypes.data)]
    for args in split_calls:
        assert L.hsrans_planes_split_diff(*args) == L.hsrans_planes_split_delta(*args) == E_ARG, args[0]
    for args in merge_calls:
        assert L.hsrans_planes_merge_diff(*args) == L.hsrans_planes_merge_delta(*args) == E_ARG, args[0]
    assert np.all(out == 0xA5) and all(np.all(p == 0xA5) for p in planes)
    # the wrappers: a base of another shape
    with pytest.raises(H.HsransError):
        H.planes_split_diff(a, b[:-1])
    with pytest.raises(H.HsransError):
        H.planes_split_diff(a, b.view(np.uint16))
    with pytest.raises(H.HsransError):
        H.planes_merge_diff(H.planes_split(a)[:3], b)
