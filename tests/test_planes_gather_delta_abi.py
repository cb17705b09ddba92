"""The delta forms of the indirect and the many-frame byte-plane gathers, without a device: the five entries are exported with the header's
argument counts and listed in the binding's signature table, the Context methods exist, and null handles are refused before anything
touches a device."""
import ctypes

import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import _abi

E_ARG = 2

# name -> (restype, number of arguments), as include/hsrans_hip.h declares them
SIGNATURES = {
    "hsrans_planes_base_set_create": (ctypes.c_int, 5),
    "hsrans_planes_base_set_destroy": (None, 1),
    "hsrans_decode_device_planes_gather_indirect_delta": (ctypes.c_int, 15),
    "hsrans_decode_device_planes_gather_batch_delta": (ctypes.c_int, 10),
    "hsrans_decode_device_planes_gather_batch_indirect_delta": (ctypes.c_int, 13),
}
# each delta entry takes its plain twin's arguments and the base's
TWINS = {
    "hsrans_decode_device_planes_gather_indirect_delta": ("hsrans_decode_device_planes_gather_indirect", 2),
    "hsrans_decode_device_planes_gather_batch_delta": ("hsrans_decode_device_planes_gather_batch", 1),
    "hsrans_decode_device_planes_gather_batch_indirect_delta": ("hsrans_decode_device_planes_gather_batch_indirect", 1),
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


@pytest.mark.parametrize("name", sorted(TWINS))
def test_a_delta_entry_takes_its_twins_arguments_and_the_base(name):
    twin, more = TWINS[name]
    assert len(_abi.SIGNATURES[name][1]) == len(_abi.SIGNATURES[twin][1]) + more


def test_the_header_declares_them():
    import os

    text = open(os.path.join(os.path.dirname(os.path.abspath(H.__file__)), "..", "include", "hsrans_hip.h")).read()
    for name in SIGNATURES:
        assert f" {name}(" in text, name
    assert "typedef struct hsrans_planes_base_set hsrans_planes_base_set;" in text


def test_the_python_names_exist():
    assert H.PlanesBaseSet._destroy == "hsrans_planes_base_set_destroy"
    assert H.PlanesBaseSet.__mro__[1] is H.PlanesGatherSet.__mro__[1], "on the shared handle base"
    for method in ("make_planes_base_set", "decode_device_planes_gather_indirect_delta", "decode_device_planes_gather_batch_delta",
                   "decode_device_planes_gather_batch_indirect_delta"):
        assert callable(getattr(H.Context, method)), method


def test_destroying_nothing_is_harmless():
    H.load_library().hsrans_planes_base_set_destroy(None)


def test_null_handles_are_refused_without_a_device():
    L = H.load_library()
    h = ctypes.c_void_p()
    ptrs, sizes = (ctypes.c_void_p * 1)(), (ctypes.c_size_t * 1)()
    assert L.hsrans_planes_base_set_create(None, None, ptrs, sizes, ctypes.byref(h)) == E_ARG
    assert L.hsrans_planes_base_set_create(None, None, ptrs, sizes, None) == E_ARG
    assert not h.value
    assert L.hsrans_decode_device_planes_gather_indirect_delta(None, None, None, None, 0, 0, None, 0, None, 0, None, 0, None, 0, None) == E_ARG
    assert L.hsrans_decode_device_planes_gather_batch_delta(None, None, None, None, 0, None, 0, None, 0, None) == E_ARG
    assert L.hsrans_decode_device_planes_gather_batch_indirect_delta(None, None, None, None, None, 0, None, 0, None, 0, None, 0, None) == E_ARG
