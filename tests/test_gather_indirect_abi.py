"""hsrans_decode_device_gather_indirect's host side, without a GPU: the two exported symbols, the workspace size (a pure function), the
refusals that need no device, and the Python mirror's signature."""
import inspect

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

E_ARG = 2


def test_symbols():
    L = H.load_library()
    assert hasattr(L, "hsrans_decode_device_gather_indirect") and hasattr(L, "hsrans_gather_workspace_bytes")


def test_workspace_bytes():
    last = 0
    for n in (0, 1, 2, 3, 62, 63, 64, 65, 1000, 1 << 16, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 1 << 28, (1 << 32) - 1):
        w = H.gather_workspace_bytes(n)
        assert w > 0 and w % 256 == 0 and w >= 4 * (n + 1), (n, w)
        assert w >= last, (n, w, last)  # non-decreasing
        last = w
        assert w == H.load_library().hsrans_gather_workspace_bytes(n)
    assert H.gather_workspace_bytes(1 << 20) < 2 * 4 * (1 << 20)  # first_task and a header, nothing of another order


def test_null_handles_and_pointers_are_argument_errors():
    """refused on the host before anything touches a device (the non-null values are never dereferenced: the context comes first)"""
    L = H.load_library()
    ws = H.gather_workspace_bytes(4)
    # (ctx, dplan, d_stream, stream_length, d_ranges, d_count, max_count, d_dst, dst_capacity, d_workspace, workspace_bytes, hip_stream)
    assert L.hsrans_decode_device_gather_indirect(None, None, None, 0, None, None, 4, None, 0, None, 0, None) == E_ARG
    fake = 0x1000  # an aligned non-null value
    assert L.hsrans_decode_device_gather_indirect(None, fake, fake, 16, fake, None, 4, fake, 16, fake, ws, None) == E_ARG  # no context
    assert L.hsrans_decode_device_gather_indirect(fake, None, fake, 16, fake, None, 4, fake, 16, fake, ws, None) == E_ARG  # no plan


def test_python_mirror():
    sig = inspect.signature(api.Context.decode_device_gather_indirect)
    assert list(sig.parameters) == ["self", "dplan", "d_stream", "d_ranges", "d_dst", "count", "max_count", "workspace", "stream_length", "stream"]
    for name in ("count", "max_count", "workspace", "stream_length", "stream"):
        assert sig.parameters[name].default is None
    assert H.gather_workspace_bytes is api.gather_workspace_bytes and "gather_workspace_bytes" in H.__all__
    L = H.load_library()
    assert len(L.hsrans_decode_device_gather_indirect.argtypes) == 12
