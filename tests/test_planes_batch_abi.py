"""hsrans_*_device_planes_batch without a device: the symbols and the Python names, the two pure host functions (the workspace of many
tensors, the task prefix of the one split / merge launch) and the refusals every entry makes before it touches a device."""
import ctypes

import hypersonic_rans_amd as H
from hypersonic_rans_amd import _abi, api

E_ARG = 2
SYMBOLS = ["hsrans_planes_batch_workspace_bytes", "hsrans_planes_batch_tasks", "hsrans_encode_device_planes_batch", "hsrans_planes_set_create",
           "hsrans_planes_set_destroy", "hsrans_planes_set_info", "hsrans_decode_device_planes_batch", "hsrans_planes_set_status"]


def test_the_symbols_and_the_python_names_are_there():
    L = H.load_library()
    for name in SYMBOLS:
        assert getattr(L, name) is not None and name in _abi.SIGNATURES, name
    for name in ("planes_batch_workspace_bytes", "planes_batch_tasks", "PlanesSet"):
        assert hasattr(H, name) and name in H.__all__, name
    for name in ("encode_device_planes_batch", "make_planes_set", "decode_device_planes_batch", "planes_set_status"):
        assert callable(getattr(H.Context, name)), name
    assert H.PlanesSet._destroy == "hsrans_planes_set_destroy" and issubclass(H.PlanesSet, api._Handle)
    # the structures as the C side lays them out (static_assert in hsrans_capi_planes_batch.cpp)
    assert ctypes.sizeof(api.PlanesMember) == 240 and ctypes.sizeof(api.PlanesSetInfo) == 32 and ctypes.sizeof(api.PlanesBatchStats) == 16


def test_the_workspace_is_the_sum_of_the_members():
    shapes = [(2, 1), (2, 17), (4, 4097), (8, 65536), (2, 2 * 65536 + 77), (4, 4096), (8, 255), (2, 256), (4, 257)]
    want = sum(H.planes_workspace_bytes(W, n) for W, n in shapes)
    assert want > 0 and H.planes_batch_workspace_bytes([W for W, _ in shapes], [n for _, n in shapes]) == want
    for W, n in shapes:
        assert H.planes_batch_workspace_bytes([W], [n]) == H.planes_workspace_bytes(W, n) == W * ((n + 255) // 256 * 256)
    # a member's region starts at the sum of the earlier ones: every prefix is the prefix's own value
    for k in range(1, len(shapes) + 1):
        assert H.planes_batch_workspace_bytes([W for W, _ in shapes[:k]], [n for _, n in shapes[:k]]) == sum(H.planes_workspace_bytes(W, n) for W, n in shapes[:k])


def test_the_workspace_is_zero_for_what_no_call_takes():
    assert H.planes_batch_workspace_bytes([], []) == 0
    assert H.planes_batch_workspace_bytes([2, 3, 4], [16, 16, 16]) == 0      # a bad element size
    assert H.planes_batch_workspace_bytes([2, 1], [16, 16]) == 0
    assert H.planes_batch_workspace_bytes([2, 4], [16, 0]) == 0              # a member without elements
    assert H.planes_batch_workspace_bytes([2], [(1 << 64) - 1]) == 0         # up256 wraps
    assert H.planes_batch_workspace_bytes([8], [1 << 62]) == 0               # elem_size * up256 wraps
    assert H.planes_batch_workspace_bytes([8, 8, 8], [1 << 60] * 3) == 0     # the sum wraps
    assert H.planes_batch_workspace_bytes([8], [1 << 60]) == 1 << 63         # (each member alone does not)
    L = H.load_library()
    one = (ctypes.c_uint32 * 1)(2)
    n = (ctypes.c_size_t * 1)(16)
    assert L.hsrans_planes_batch_workspace_bytes(None, n, 1) == 0 and L.hsrans_planes_batch_workspace_bytes(one, None, 1) == 0
    assert L.hsrans_planes_batch_workspace_bytes(one, n, 0) == 0 and L.hsrans_planes_batch_workspace_bytes(one, n, 1) == 512


def test_a_member_has_the_tasks_of_its_single_launch():
    for n in (1, 15, 16, 4095, 4096, 4097):
        assert H.planes_batch_tasks([n]) == (1, [0, 1]), n
    for n in (8192, 8193):
        assert H.planes_batch_tasks([n]) == (2, [0, 2]), n
    for n in (1, 16, 255, 4096, 4111, 4112, 8191, 8192, 65536, 2 * 65536 + 77, 1_000_003, 1 << 30):
        assert H.planes_batch_tasks([n])[0] == max(1, -(-(n // 16) // 256)), n


def test_the_prefix_and_the_total_of_a_mixed_list():
    elements = [1, 17, 4097, 65536, 2 * 65536 + 77, 65536 + 5, 3 * 65536 + 9, 4096]
    tasks = [1, 1, 1, 16, 33, 16, 48, 1]  # max(1, ceil(floor(n / 16) / 256))
    total, first = H.planes_batch_tasks(elements)
    assert total == sum(tasks) and first == [sum(tasks[:k]) for k in range(len(tasks) + 1)]
    # without the prefix: the total alone
    L = H.load_library()
    assert L.hsrans_planes_batch_tasks((ctypes.c_size_t * 8)(*elements), 8, None) == sum(tasks)


def test_the_tasks_are_zero_for_what_no_launch_takes():
    assert H.planes_batch_tasks([]) == (0, [])
    assert H.planes_batch_tasks([16, 0, 16]) == (0, [])              # a member without elements
    assert H.planes_batch_tasks([(1 << 42) + 1]) == (0, [])          # more than a single launch takes
    assert H.planes_batch_tasks([1 << 42])[0] == 1 << 30
    assert H.planes_batch_tasks([1 << 42, 1 << 42]) == (0, [])       # 2^31 tasks
    assert H.planes_batch_tasks([1 << 42, (1 << 42) - 4096])[0] == (1 << 31) - 1
    L = H.load_library()
    assert L.hsrans_planes_batch_tasks(None, 1, None) == 0
    assert L.hsrans_planes_batch_tasks((ctypes.c_size_t * 1)(16), 0, None) == 0


def test_every_entry_refuses_null_handles_without_a_device():
    L = H.load_library()
    fake = ctypes.c_void_p(0x1000)  # never dereferenced: every call below is refused before it looks at it
    members = (api.PlanesMember * 2)()
    for m in members:
        m.frame_length, m.rc, m.desc.elem_size = 7, 7, 7
    stats = api.PlanesBatchStats(9, 9, 9, 9)
    handles = (ctypes.c_void_p * 16)(*([0x1000] * 16))
    assert L.hsrans_encode_device_planes_batch(None, members, 2, fake, 1 << 20, None, handles, ctypes.byref(stats)) == E_ARG
    assert not any(handles) and all(m.frame_length == 0 and bytes(m.desc) == bytes(api.PlanesDesc()) for m in members)
    assert (stats.launches, stats.members, stats.planes, stats.stored) == (0, 0, 0, 0)
    assert L.hsrans_encode_device_planes_batch(fake, None, 2, fake, 1 << 20, None, None, None) == E_ARG
    assert L.hsrans_encode_device_planes_batch(fake, members, 0, fake, 1 << 20, None, None, None) == E_ARG
    descs = (api.PlanesDesc * 1)()
    plans = (ctypes.c_void_p * 8)()
    out = ctypes.c_void_p(0x1000)
    assert L.hsrans_planes_set_create(None, descs, plans, 1, ctypes.byref(out)) == E_ARG and not out.value
    assert L.hsrans_planes_set_create(fake, None, plans, 1, ctypes.byref(out)) == E_ARG
    assert L.hsrans_planes_set_create(fake, descs, None, 1, ctypes.byref(out)) == E_ARG
    assert L.hsrans_planes_set_create(fake, descs, plans, 0, ctypes.byref(out)) == E_ARG
    assert L.hsrans_planes_set_create(fake, descs, plans, 1, None) == E_ARG
    info = api.PlanesSetInfo()
    assert L.hsrans_planes_set_info(None, ctypes.byref(info)) == E_ARG and L.hsrans_planes_set_info(fake, None) == E_ARG
    arr = (ctypes.c_void_p * 1)(0x1000)
    lens = (ctypes.c_size_t * 1)(16)
    assert L.hsrans_decode_device_planes_batch(None, fake, arr, lens, arr, lens, fake, 256, None) == E_ARG
    assert L.hsrans_decode_device_planes_batch(fake, None, arr, lens, arr, lens, fake, 256, None) == E_ARG
    assert L.hsrans_planes_set_status(None, fake, None, None) == E_ARG and L.hsrans_planes_set_status(fake, None, None, None) == E_ARG
    L.hsrans_planes_set_destroy(None)
