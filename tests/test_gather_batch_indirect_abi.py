"""hsrans_decode_device_gather_batch_indirect's host side, without a GPU: the four exported symbols and their declarations, the workspace
size (a pure function), the refusals that need no device, and the Python mirror — signatures, and the type checks that come before any C
call."""
import ctypes
import inspect
import os
import re

import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

E_ARG = 2
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hsrans_hip.h")
SYMBOLS = {"hsrans_gather_batch_workspace_bytes": 2, "hsrans_decode_device_gather_batch_indirect": 10, "hsrans_gather_set_refused": 3,
           "hsrans_gather_set_indirect_info": 4}


def test_symbols_and_signatures():
    L = H.load_library()
    for name, n_args in SYMBOLS.items():
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == n_args, name


def test_header_declares_them():
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    decl = {name: re.search(r"(\w+)\s+" + name + r"\s*\(([^;]*)\)\s*;", text) for name in SYMBOLS}
    for name, n_args in SYMBOLS.items():
        assert decl[name] is not None, name
        assert len(decl[name].group(2).split(",")) == n_args, (name, decl[name].group(2))
    assert decl["hsrans_gather_batch_workspace_bytes"].group(1) == "size_t"
    args = " ".join(decl["hsrans_decode_device_gather_batch_indirect"].group(2).split()).replace(" ,", ",")  # (a comment stood in front of the comma)
    assert args == ("hsrans_ctx *ctx, hsrans_gather_set *set, const hsrans_member_range *d_ranges, const uint32_t *d_count, uint32_t max_count, "
                    "void *d_dst, size_t dst_capacity, void *d_workspace, size_t workspace_bytes, void *hip_stream")
    assert " ".join(decl["hsrans_gather_set_refused"].group(2).split()) == "hsrans_ctx *ctx, hsrans_gather_set *set, void *hip_stream"
    assert " ".join(decl["hsrans_gather_set_indirect_info"].group(2).split()) == \
        "const hsrans_gather_set *set, uint32_t max_count, size_t dst_capacity, hsrans_gather_set_info_t *info"
    # behind hsrans_decode_device_gather_batch
    assert text.index("hsrans_decode_device_gather_batch(") < text.index("hsrans_decode_device_gather_batch_indirect(")


def test_workspace_bytes():
    counts = (0, 1, 2, 63, 64, 65, 1000, 1 << 16, (1 << 20) + 1, 1 << 28, (1 << 32) - 1)
    members = (1, 2, 63, 64, 65, 1023, 1024, 1025, 1500, 65_535, 65_536)
    table = {}
    for m in members:
        for n in counts:
            w = H.gather_batch_workspace_bytes(m, n)
            assert w > 0 and w % 256 == 0, (m, n, w)
            assert w >= 4 * (2 * n + 1) and w >= 4 * 3 * m, (m, n, w)  # perm[] and first_task[]; three words per member
            assert w == H.load_library().hsrans_gather_batch_workspace_bytes(m, n)
            table[m, n] = w
    for i, m in enumerate(members):  # non-decreasing in both arguments
        for j, n in enumerate(counts):
            assert i == 0 or table[m, n] >= table[members[i - 1], n]
            assert j == 0 or table[m, n] >= table[m, counts[j - 1]]
    for n in counts:
        assert H.gather_batch_workspace_bytes(0, n) == 0
        assert H.gather_batch_workspace_bytes(65_537, n) == 0 and H.gather_batch_workspace_bytes((1 << 32) - 1, n) == 0
    assert H.gather_batch_workspace_bytes(10, 1 << 20) < 3 * 4 * (1 << 20)  # two words per range and a header, nothing of another order


def test_null_handles_and_pointers_are_argument_errors():
    """refused on the host before anything touches a device (the non-null values are never dereferenced: the handles come first)"""
    L = H.load_library()
    ws = H.gather_batch_workspace_bytes(4, 4)
    fake = 0x1000
    # (ctx, set, d_ranges, d_count, max_count, d_dst, dst_capacity, d_workspace, workspace_bytes, hip_stream)
    assert L.hsrans_decode_device_gather_batch_indirect(None, None, None, None, 4, None, 0, None, 0, None) == E_ARG
    assert L.hsrans_decode_device_gather_batch_indirect(None, fake, fake, None, 4, fake, 16, fake, ws, None) == E_ARG  # no context
    assert L.hsrans_decode_device_gather_batch_indirect(fake, None, fake, None, 4, fake, 16, fake, ws, None) == E_ARG  # no set
    assert L.hsrans_gather_set_refused(None, None, None) == E_ARG
    assert L.hsrans_gather_set_refused(fake, None, None) == E_ARG
    info = api.GatherSetInfo()
    assert L.hsrans_gather_set_indirect_info(None, 4, 16, ctypes.byref(info)) == E_ARG
    assert L.hsrans_gather_set_indirect_info(None, 4, 16, None) == E_ARG


def test_python_mirror():
    sig = inspect.signature(api.Context.decode_device_gather_batch_indirect)
    assert list(sig.parameters) == ["self", "gset", "d_ranges", "d_dst", "count", "max_count", "workspace", "stream"]
    for name in ("count", "max_count", "workspace", "stream"):
        assert sig.parameters[name].default is None
    assert list(inspect.signature(api.Context.gather_set_refused).parameters) == ["self", "gset", "stream"]
    assert inspect.signature(api.Context.gather_set_refused).parameters["stream"].default is None
    assert list(inspect.signature(api.GatherSet.indirect_info).parameters) == ["self", "max_count", "dst_capacity"]
    assert list(inspect.signature(api.gather_batch_workspace_bytes).parameters) == ["members", "max_count"]
    assert H.gather_batch_workspace_bytes is api.gather_batch_workspace_bytes and "gather_batch_workspace_bytes" in H.__all__


class _NoCalls:
    """stands in for the library: any C call fails the test"""

    def __getattr__(self, name):
        raise AssertionError("C call " + name)


class _FakeCuda:
    """a CPU tensor that says it is on the GPU: the wrappers' checks read attributes only"""

    def __init__(self, t):
        self.t = t
        self.is_cuda = True

    def __getattr__(self, name):
        return getattr(self.t, name)


def test_wrappers_refuse_bad_tensors_before_any_c_call():
    ctx = object.__new__(api.Context)
    ctx.L = _NoCalls()
    gset = object.__new__(api.GatherSet)
    gset.handle, gset.dplans = None, [None] * 3
    stream = object()  # (given, so that torch is not asked for a current stream)
    dst = torch.zeros(64, dtype=torch.uint8)
    good = _FakeCuda(torch.zeros((8, 4), dtype=torch.int64))

    def refused(d_ranges, count=None):
        with pytest.raises(TypeError):
            ctx.decode_device_gather_batch_indirect(gset, d_ranges, dst, count=count, stream=stream)

    refused(torch.zeros((8, 4), dtype=torch.int64))                             # not on the GPU
    refused(_FakeCuda(torch.zeros((8, 3), dtype=torch.int64)))                  # the single call's shape
    refused(_FakeCuda(torch.zeros((32,), dtype=torch.int64)))
    refused(_FakeCuda(torch.zeros((8, 4), dtype=torch.int32)))                  # wrongly typed
    refused(_FakeCuda(torch.zeros((8, 4), dtype=torch.float64)))
    refused(_FakeCuda(torch.zeros((8, 8), dtype=torch.int64)[:, :4]))           # not contiguous
    refused(_FakeCuda(torch.zeros((4, 8), dtype=torch.int64).t()))
    refused(good, count=torch.zeros((), dtype=torch.int32))                     # count: not on the GPU
    refused(good, count=_FakeCuda(torch.zeros((), dtype=torch.int64)))          # wrongly typed
    refused(good, count=_FakeCuda(torch.zeros((2,), dtype=torch.int32)))        # not a scalar
