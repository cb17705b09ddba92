"""hsrans_pack_device and hsrans_planes_pack_device without a device: the five entries are exported with the header's argument counts, the
two stream-layer size functions against a numpy model, the frame layout on hand-made descriptors (the formulae of include/hsrans_hip.h,
idempotence, a 0 for every broken rule), and both device entries refusing a NULL context before they touch a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import _abi, api

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hsrans_hip.h")
E_ARG = 2
C = H.PACK_CHUNK
ENTRIES = {"hsrans_pack_layout": 3, "hsrans_pack_tasks": 3, "hsrans_pack_device": 7, "hsrans_planes_pack_layout": 4, "hsrans_planes_pack_device": 10}
MAX_ITEMS = 524288


def up16(v):
    return (int(v) + 15) // 16 * 16


@pytest.fixture(scope="module")
def L():
    return api.load_library()


def test_the_five_entries_are_exported_with_the_headers_argument_counts(L):
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    for name, n_args in ENTRIES.items():
        params = re.search(r"\b" + name + r"\s*\(([^()]*)\)\s*;", text).group(1)
        assert len(params.split(",")) == n_args == len(_abi.SIGNATURES[name][1]), name
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == n_args, name


def test_the_chunk_is_the_headers():
    value = int(re.search(r"^#define HSRANS_PACK_CHUNK (\d+)", open(HEADER).read(), flags=re.M).group(1))
    assert C == value and C >= 4096 and C & (C - 1) == 0


def _model(lengths):
    padded = np.array([up16(v) for v in lengths], dtype=np.uint64)
    offsets = np.concatenate([[0], np.cumsum(padded)]).astype(np.uint64)
    first = np.concatenate([[0], np.cumsum((padded + np.uint64(C - 1)) // np.uint64(C))]).astype(np.uint64)
    return offsets, first


def test_layout_and_tasks_match_a_numpy_model():
    rng = np.random.default_rng(23)
    edges = [1, 15, 16, 17, C - 1, C, C + 1]
    sets = [edges, edges[::-1], [1], [C + 1, 1, C, 17, 2 * C], list(rng.integers(1, 5 * C, 200)) + edges, list(rng.integers(1, 49, 300)), [1 << 33, 3, (1 << 33) + 1]]
    for lengths in sets:
        offsets, first = _model(lengths)
        total, got = H.pack_layout(lengths)
        assert total == int(offsets[-1]) and got == [int(v) for v in offsets], lengths[:8]
        tasks, got_first = H.pack_tasks(lengths)
        assert tasks == int(first[-1]) and got_first == [int(v) for v in first], lengths[:8]
    # the arrays are optional: the totals alone
    arr = (ctypes.c_size_t * len(edges))(*edges)
    lib = api.load_library()
    assert lib.hsrans_pack_layout(arr, len(edges), None) == int(_model(edges)[0][-1]) and lib.hsrans_pack_tasks(arr, len(edges), None) == int(_model(edges)[1][-1])


def test_layout_and_tasks_return_zero_for_what_no_call_takes(L):
    big = 1 << 63
    refused = [[], [0], [5, 0, 7], [1] * (MAX_ITEMS + 1), [big, big], [2 ** 64 - 1], [2 ** 64 - 16, 16]]
    for lengths in refused:
        assert H.pack_layout(lengths) == (0, []) and H.pack_tasks(lengths) == (0, []), len(lengths)
    # ... straight through the C entries too, which get the 524,289 items and must write nothing
    n = MAX_ITEMS + 1
    arr = (ctypes.c_size_t * n)(*([1] * n))
    offsets, first = (ctypes.c_uint64 * 4)(7, 7, 7, 7), (ctypes.c_uint32 * 4)(7, 7, 7, 7)
    assert L.hsrans_pack_layout(arr, n, offsets) == 0 and L.hsrans_pack_tasks(arr, n, first) == 0
    assert L.hsrans_pack_layout(None, 3, offsets) == 0 and L.hsrans_pack_tasks(None, 3, first) == 0
    assert L.hsrans_pack_layout(arr, 0, offsets) == 0 and L.hsrans_pack_tasks(arr, 0, first) == 0
    two = (ctypes.c_size_t * 2)(big, big)
    assert L.hsrans_pack_layout(two, 2, offsets) == 0 and L.hsrans_pack_tasks(two, 2, first) == 0
    assert list(offsets) == [7] * 4 and list(first) == [7] * 4
    assert H.pack_layout([1] * MAX_ITEMS)[0] == 16 * MAX_ITEMS and H.pack_tasks([1] * MAX_ITEMS)[0] == MAX_ITEMS  # the limit itself is taken
    # a layout that fits and a task total that does not: 2^31 chunks
    assert H.pack_layout([C << 31])[0] == C << 31 and H.pack_tasks([C << 31]) == (0, [])
    assert H.pack_tasks([(C << 31) - C + 1]) == (0, []) and H.pack_tasks([(C << 31) - C])[0] == (1 << 31) - 1


def _desc(W, elements, lengths, offsets, stored_mask=0, frame_length=None):
    d = api.PlanesDesc()
    d.elem_size, d.states, d.bits, d.block_size, d.index_interval, d.stored_mask, d.elements = W, 64, 11, 1 << 16, 32, stored_mask, elements
    for p in range(W):
        d.offset[p], d.length[p] = offsets[p], lengths[p]
    d.frame_length = max(o + n for o, n in zip(offsets, lengths)) if frame_length is None else frame_length
    return d


def _hand_made():
    """W of 2, 4 and 8; stored planes (length == elements) and coded ones; source offsets as an encoder leaves them, compacted, and in
    another order than the planes'"""
    return [
        _desc(2, 65539, [65539, 30001], [0, 69888], stored_mask=0b01),                                   # an encoder's frame: one stored, one coded
        _desc(4, 4096, [1000, 17, 4096, 3333], [5120, 0, 1024, 9216 + 16], stored_mask=0b0100),        # planes out of order
        _desc(8, 1000, [1000, 999, 1, 15, 16, 17, 700, 1000], [16 * 70 * p for p in (7, 0, 3, 1, 2, 6, 5, 4)], stored_mask=0b10000001),
        _desc(2, 17, [17, 17], [32, 0], stored_mask=0b11, frame_length=4096),                            # every plane stored, a roomy frame
        _desc(2, 5, [3, 2], [0, 16]),                                                                     # already packed
    ]


def _expected(descs):
    outs, bases = [], [0]
    for d in descs:
        at, offsets = 0, []
        for p in range(d.elem_size):
            offsets.append(at)
            at += up16(d.length[p])
        outs.append((offsets, offsets[-1] + d.length[d.elem_size - 1]))
        bases.append(bases[-1] + at)
    return outs, bases


def test_the_frame_layout_follows_its_formulae_and_is_idempotent():
    descs = _hand_made()
    outs, bases, total = H.planes_pack_layout(descs)
    want, want_bases = _expected(descs)
    assert total == want_bases[-1] and bases == want_bases and len(outs) == len(descs)
    for d, o, (offsets, frame_length) in zip(descs, outs, want):
        W = d.elem_size
        assert list(o.offset)[:W] == offsets and o.frame_length == frame_length and list(o.offset)[W:] == [0] * (8 - W)
        assert list(o.length) == list(d.length)
        for field in ("elem_size", "states", "bits", "block_size", "index_interval", "stored_mask", "elements"):
            assert getattr(o, field) == getattr(d, field), field
    assert all(b % 16 == 0 for b in bases)
    again, bases2, total2 = H.planes_pack_layout(outs)
    assert [bytes(d) for d in again] == [bytes(d) for d in outs] and bases2 == bases and total2 == total
    assert bytes(outs[4]) == bytes(descs[4])  # (a packed descriptor is its own layout)
    # each member alone: its own total is its share of the arena
    for k, d in enumerate(descs):
        one, b, t = H.planes_pack_layout([d])
        assert bytes(one[0]) == bytes(outs[k]) and b == [0, bases[k + 1] - bases[k]] and t == b[1]


def test_the_frame_layout_writes_in_place_and_takes_null_outputs(L):
    descs = _hand_made()
    K = len(descs)
    want, _, total = H.planes_pack_layout(descs)
    arr = (api.PlanesDesc * K)(*descs)
    assert L.hsrans_planes_pack_layout(arr, K, None, None) == total
    assert [bytes(d) for d in arr] == [bytes(d) for d in descs]
    assert L.hsrans_planes_pack_layout(arr, K, arr, None) == total
    assert [bytes(d) for d in arr] == [bytes(d) for d in want]


def test_the_frame_layout_returns_zero_for_each_broken_rule(L):
    good = _hand_made()[1]

    def changed(**kw):
        d = api.PlanesDesc.from_buffer_copy(good)
        for key, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, key)[v[0]] = v[1]
            else:
                setattr(d, key, v)
        return d

    broken = {
        "elem_size 3": changed(elem_size=3), "elem_size 1": changed(elem_size=1), "elem_size 16": changed(elem_size=16), "elem_size 0": changed(elem_size=0),
        "an offset that is no multiple of 16": changed(offset=(1, 8)),
        "a length of 0": changed(length=(3, 0)),
        "two planes overlap": changed(offset=(1, 5120 + 512)),
        "a plane begins in another's last 16 bytes": changed(offset=(1, 5120 + 992)),  # plane 0 ends at 6120
        "a frame_length below the last byte": changed(frame_length=9216 + 16 + 3333 - 1),
        "an offset + length that wraps": changed(offset=(2, 2 ** 64 - 16)),
    }
    for why, d in broken.items():
        outs = (api.PlanesDesc * 2)()
        bases = (ctypes.c_uint64 * 3)(7, 7, 7)
        assert L.hsrans_planes_pack_layout((api.PlanesDesc * 2)(good, d), 2, outs, bases) == 0, why
        assert bytes(outs) == bytes((api.PlanesDesc * 2)()) and list(bases) == [7, 7, 7], why
        assert H.planes_pack_layout([d, good]) == ([], [], 0), why
    assert H.planes_pack_layout([changed(frame_length=9216 + 16 + 3333)])[2] != 0  # (the last byte itself is enough)
    assert H.planes_pack_layout([]) == ([], [], 0) and H.planes_pack_layout([good] * 65537) == ([], [], 0)
    assert L.hsrans_planes_pack_layout(None, 1, None, None) == 0 and L.hsrans_planes_pack_layout((api.PlanesDesc * 1)(good), 0, None, None) == 0
    assert H.planes_pack_layout([good] * 65536)[2] == 65536 * H.planes_pack_layout([good])[2]  # the limit itself is taken
    huge = _desc(2, 1 << 62, [2 ** 63, 2 ** 63], [0, 2 ** 63])  # two planes whose sum no size_t holds
    assert H.planes_pack_layout([huge]) == ([], [], 0)
    half = _desc(2, 1 << 62, [2 ** 62, 2 ** 62], [0, 2 ** 62])
    assert H.planes_pack_layout([half])[2] == 2 ** 63 and H.planes_pack_layout([half, half]) == ([], [], 0)  # ... nor two members' sum


def test_the_device_entries_refuse_a_null_context_before_any_device(L):
    lengths = (ctypes.c_size_t * 2)(100, 200)
    srcs = (ctypes.c_void_p * 2)(0x10000, 0x20000)  # (never dereferenced: the context is looked at first)
    assert L.hsrans_pack_device(None, srcs, lengths, 2, 0x100000, 1 << 20, None) == E_ARG
    descs = (api.PlanesDesc * 2)(*_hand_made()[:2])
    frame_lengths = (ctypes.c_size_t * 2)(descs[0].frame_length, descs[1].frame_length)
    outs = (api.PlanesDesc * 2)(*_hand_made()[:2])
    assert L.hsrans_planes_pack_device(None, descs, srcs, frame_lengths, 2, 0x100000, 1 << 20, None, outs, None) == E_ARG
    assert bytes(outs) == bytes((api.PlanesDesc * 2)())  # on refusal out_descs is zeroed
