"""hsrans_*_device_planes: tensors of 2-, 4- and 8-byte elements coded as byte planes.  The two kernels alone against numpy; every plane
of a frame against its single call (hsrans_encode_device), the host encoder and the oracle's decode; the rule for stored planes; frames
decoded back to the tensor, with coded, stored and mixed planes; refusals that launch nothing and write nothing."""
import ctypes

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api, synth

pytestmark = pytest.mark.gpu

MT = H.MT
E_ARG = 2
SENTINEL = 0xA5
TORCH_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
NP_UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
N_MAX = 1_000_003


# ---- inputs: numpy arrays of 2-, 4- or 8-byte items, made once ----
@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(29)
    x = rng.standard_normal(N_MAX).astype(np.float32)
    ramp = (np.arange(N_MAX, dtype=np.uint64) << np.uint64(8)) | rng.integers(0, 256, N_MAX, dtype=np.uint64)  # noise in the low byte
    mixed = (rng.integers(0, 256, N_MAX, dtype=np.uint16) | (np.abs(rng.standard_normal(N_MAX) * 3).astype(np.uint16) << 8)).astype(np.uint16)
    return {
        "bf16": (x.view(np.uint32) >> 16).astype(np.uint16),  # truncated to bf16
        "fp16": x.astype(np.float16).view(np.uint16),
        "fp32": x.view(np.uint32),
        "i64": ramp,
        "uniform": synth.uniform_bytes(2 * N_MAX, seed=31).view(np.uint16),  # every plane incompressible
        "mixed": mixed,  # plane 0 uniform, plane 1 small values: exactly one plane worth coding
    }


def _tensor(a, name=None):
    """The device tensor of a numpy array of unsigned items: bf16 / fp16 / fp32 under their torch dtypes, the rest as signed integers."""
    t = torch.from_numpy(np.ascontiguousarray(a).view({2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize])).cuda()
    real = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}.get(name)
    return t.view(real) if real is not None else t


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _full(n):
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")


def _untouched(t):
    return bool((t == SENTINEL).all().item())


def _buffers(W, states, n, extra=0):
    return _full(H.planes_capacity(W, states, n) + extra), _full(H.planes_workspace_bytes(W, n) + extra)


# ---- the kernels alone ----
SIZES = [1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097, 2 * 65536 + 77]
PAD = 64  # sentinel bytes behind every destination


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_the_split_kernel_equals_numpy(gpu_ctx, W, n):
    raw = np.random.default_rng(W * 1_000_000 + n).integers(0, 256, n * W, dtype=np.uint8)
    d_in = _tensor(raw.view(NP_UINT[W]))
    planes = [_full(n + PAD) for _ in range(W)]
    gpu_ctx.planes_split_device(d_in, planes, elements=n)
    torch.cuda.synchronize()
    rows = raw.reshape(-1, W)
    for p in range(W):
        got = planes[p].cpu().numpy()
        assert np.array_equal(got[:n], rows[:, p]), p
        assert np.all(got[n:] == SENTINEL), p


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_the_merge_kernel_equals_numpys_interleave(gpu_ctx, W, n):
    rng = np.random.default_rng(W * 2_000_000 + n)
    planes = [rng.integers(0, 256, n, dtype=np.uint8) for _ in range(W)]
    d_planes = [torch.from_numpy(p).cuda() for p in planes]
    pad_items = PAD // W
    out = _full((n + pad_items) * W).view(TORCH_INT[W])
    gpu_ctx.planes_merge_device(d_planes, out, elements=n)
    torch.cuda.synchronize()
    got = _bytes(out)
    assert np.array_equal(got[: n * W], np.stack(planes, axis=1).reshape(-1))
    assert np.all(got[n * W:] == SENTINEL)


def test_the_kernel_entries_refuse_bad_arguments(gpu_ctx):
    n = 1024
    L, ctx = gpu_ctx.L, gpu_ctx.handle
    el = _full(8 * n + 16)
    pl = [_full(n + 16) for _ in range(8)]
    ptrs = lambda ts: (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])  # noqa: E731
    bad = [
        (None, 2, el.data_ptr(), n, ptrs(pl)),                  # no context
        (ctx, 3, el.data_ptr(), n, ptrs(pl)),                   # element size
        (ctx, 16, el.data_ptr(), n, ptrs(pl)),
        (ctx, 2, el.data_ptr(), 0, ptrs(pl)),                   # no elements
        (ctx, 2, el.data_ptr() + 4, n, ptrs(pl)),               # alignment of the element buffer
        (ctx, 2, el.data_ptr(), n, ptrs([pl[0], pl[1][8:]])),   # ... of a plane
        (ctx, 2, el.data_ptr(), n, ptrs([pl[0], pl[0]])),       # two planes on one range
        (ctx, 2, el.data_ptr(), n, ptrs([pl[0], el[16:]])),     # a plane inside the element buffer
        (ctx, 4, el.data_ptr(), n, None),                       # no plane array
    ]
    for c, W, e, count, pp in bad:
        assert L.hsrans_planes_split_device(c, W, e, count, pp, None) == E_ARG, (W, count)
        assert L.hsrans_planes_merge_device(c, W, pp, count, e, None) == E_ARG, (W, count)
    torch.cuda.synchronize()
    assert _untouched(el) and all(_untouched(t) for t in pl)


# ---- encode ----
# (input, states, bits, index_interval, block_size, elements): every element size, both state counts, bits 10 / 11 / 13 / 15, with and without checkpoints
CASES = [
    ("bf16", 64, 11, 32, 1 << 16, 1_000_003),
    ("bf16", 32, 10, 0, 1 << 16, 1),
    ("bf16", 64, 13, 0, 1 << 14, 65536),
    ("fp16", 64, 13, 32, 1 << 16, 17),
    ("fp16", 32, 15, 0, 1 << 14, 1025),
    ("fp16", 32, 11, 32, 1 << 16, 2 * 65536 + 77),
    ("fp32", 64, 11, 32, 1 << 16, 2 * 65536 + 77),
    ("fp32", 32, 11, 32, 1 << 14, 65536),
    ("fp32", 64, 15, 0, 1 << 16, 1025),
    ("fp32", 64, 10, 0, 1 << 16, 1),
    ("i64", 64, 11, 32, 1 << 14, 65536),
    ("i64", 32, 13, 0, 1 << 16, 17),
    ("i64", 64, 10, 32, 1 << 16, 2 * 65536 + 77),  # (uniform planes in 16 KiB blocks at 10 bits outgrow hsrans_capacity: the single call fails too)
    ("i64", 64, 11, 0, 1 << 16, 1_000_003),
]
CASE_IDS = [f"{c[0]}-s{c[1]}-b{c[2]}-i{c[3]}-n{c[5]}" for c in CASES]


def _encode(ctx, a, name, states, bits, interval, block, store, want_plans=True):
    t = _tensor(a, name)
    frame, work = _buffers(a.itemsize, states, a.size)
    n, desc, plans = ctx.encode_device_planes(t, frame, work, states=states, bits=bits, block_size=block, index_interval=interval,
                                              store_incompressible=store, want_plans=want_plans)
    return t, frame, work, n, desc, plans


def _single(ctx, plane, states, bits, interval, block):
    """hsrans_encode_device of one plane's bytes: (stream, plan blob)"""
    d_in = torch.from_numpy(np.ascontiguousarray(plane)).cuda()
    d_out = _full(H.capacity(MT, states, plane.size))
    m, p = ctx.encode_device(MT, states, bits, d_in, d_out, block_size=block, index_interval=interval, want_plan=True)
    return d_out[:m].cpu().numpy(), ctx.read_device_plan(p)


def _check_desc(desc, W, states, bits, interval, block, n):
    assert (desc.elem_size, desc.states, desc.bits, desc.block_size, desc.index_interval, desc.elements) == (W, states, bits, block, interval, n)
    stride = H.planes_capacity(W, states, n) // W
    for p in range(api.PLANES_MAX):
        assert desc.offset[p] == (p * stride if p < W else 0), p
        assert (desc.length[p] != 0) == (p < W), p
    assert desc.frame_length == desc.offset[W - 1] + desc.length[W - 1]


def _reference_decodes(plane, states, block):
    """Whether the reference's mt_ decoder takes the plane's stream at all.  It rejects a stream in which no block carries a histogram
    (every block one symbol; a one-symbol file is the plain case), its own encoder's included, and inputs shorter than a group less one
    byte are undefined behaviour in it (tests/test_gpu_parity.py, tests/test_host_format.py): the oracle returns 0
    for both.  Such planes are still checked against the single call, the host encoder and the oracle's plan executor."""
    return plane.size >= states - 1 and any(np.unique(plane[b: b + block]).size > 1 for b in range(0, plane.size, block))


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_every_coded_plane_is_its_single_calls_stream(gpu_ctx, oracle, inputs, case):
    name, states, bits, interval, block, n = case
    a = inputs[name][:n]
    W = a.itemsize
    t, frame, work, total, desc, plans = _encode(gpu_ctx, a, name, states, bits, interval, block, store=False)
    _check_desc(desc, W, states, bits, interval, block, n)
    assert total == desc.frame_length and desc.stored_mask == 0 and all(p is not None for p in plans)
    got = frame.cpu().numpy()
    rows = a.view(np.uint8).reshape(-1, W)
    for p in range(W):
        plane = np.ascontiguousarray(rows[:, p])
        mine = got[desc.offset[p]: desc.offset[p] + desc.length[p]]
        want, want_plan = _single(gpu_ctx, plane, states, bits, interval, block)
        assert desc.length[p] == want.size and np.array_equal(mine, want), p
        assert np.array_equal(mine, H.encode(MT, states, bits, plane, block_size=block, independent_blocks=True)), p
        if _reference_decodes(plane, states, block):
            r, back = oracle.decode(MT, states, bits, mine, n)
            assert r == n and np.array_equal(back, plane), p
        blob = gpu_ctx.read_device_plan(plans[p])
        assert np.array_equal(blob, want_plan), p
        r, back = oracle.exec_plan(blob, mine, n)  # (every length: the oracle's plan executor over the plan the call returned)
        assert r == n and np.array_equal(back, plane), p
        end = desc.offset[p + 1] if p + 1 < W else got.size
        assert np.all(got[desc.offset[p] + desc.length[p]: end] == SENTINEL), p  # nothing written past a plane's stream


def test_without_plans_the_frame_is_the_same(gpu_ctx, inputs):
    a = inputs["fp32"][:65536 + 5]
    _, frame, _, total, desc, plans = _encode(gpu_ctx, a, "fp32", 64, 11, 32, 1 << 16, store=True)
    _, frame2, _, total2, desc2, plans2 = _encode(gpu_ctx, a, "fp32", 64, 11, 32, 1 << 16, store=True, want_plans=False)
    assert plans2 == [None] * 4 and total2 == total and bytes(desc2) == bytes(desc)
    for p in range(4):
        lo, hi = desc.offset[p], desc.offset[p] + desc.length[p]
        assert torch.equal(frame[lo:hi], frame2[lo:hi]), p


# ---- stored planes ----
def _stored_rule(ctx, a, states, bits, block):
    """bit p set exactly when plane p's single call gives a stream no shorter than the plane"""
    rows = a.view(np.uint8).reshape(-1, a.itemsize)
    lengths = [_single(ctx, rows[:, p], states, bits, 0, block)[0].size for p in range(a.itemsize)]
    return sum(1 << p for p, m in enumerate(lengths) if m >= a.size), lengths


def test_fp32_stores_its_mantissa_planes(gpu_ctx, inputs):
    n = 2 * 65536 + 77
    a = inputs["fp32"][:n]
    _, frame, _, total, desc, plans = _encode(gpu_ctx, a, "fp32", 64, 11, 32, 1 << 16, store=True)
    want_mask, lengths = _stored_rule(gpu_ctx, a, 64, 11, 1 << 16)
    assert desc.stored_mask == want_mask
    assert desc.stored_mask & 0b0011 == 0b0011 and not desc.stored_mask & 0b1000  # (plane 2, ~7.97 bits, sits at the edge: either)
    rows = a.view(np.uint8).reshape(-1, 4)
    got = frame.cpu().numpy()
    for p in range(4):
        stored = bool(desc.stored_mask >> p & 1)
        assert (plans[p] is None) == stored, p
        assert desc.length[p] == (n if stored else lengths[p]), p
        if stored:
            assert np.array_equal(got[desc.offset[p]: desc.offset[p] + n], rows[:, p]), p
    assert total == desc.frame_length == desc.offset[3] + desc.length[3]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_plane_is_stored_exactly_when_its_stream_is_no_shorter(gpu_ctx, inputs, case):
    name, states, bits, interval, block, n = case
    a = inputs[name][:n]
    _, _, _, _, desc, plans = _encode(gpu_ctx, a, name, states, bits, interval, block, store=True)
    want_mask, _ = _stored_rule(gpu_ctx, a, states, bits, block)
    assert desc.stored_mask == want_mask
    assert [p is None for p in plans] == [bool(want_mask >> k & 1) for k in range(a.itemsize)]


def test_uniform_bytes_are_all_stored(gpu_ctx, inputs):
    a = inputs["uniform"][: 2 * 65536 + 77]
    t, frame, work, total, desc, plans = _encode(gpu_ctx, a, "uniform", 64, 11, 32, 1 << 16, store=True)
    assert desc.stored_mask == 0b11 and plans == [None, None]
    planes = gpu_ctx.make_planes(desc, plans)
    assert planes.info() == {"coded": 0, "stored": 2, "launches": 1}
    out = torch.zeros_like(t)
    gpu_ctx.decode_device_planes(planes, frame, out, work)
    assert gpu_ctx.planes_status(planes) == [0, 0]
    assert torch.equal(out.view(torch.uint8), t.view(torch.uint8))
    planes.close()


# ---- decode ----
def _round_trip(ctx, a, name, states, bits, interval, block, store):
    t, frame, work, total, desc, plans = _encode(ctx, a, name, states, bits, interval, block, store)
    planes = ctx.make_planes(desc, plans)
    work2 = _full(work.numel())  # (a workspace of its own: the decode needs nothing the encode left)
    out = torch.zeros_like(t)
    ctx.decode_device_planes(planes, frame, out, work2)
    assert ctx.planes_status(planes) == [0] * a.itemsize
    assert torch.equal(out.view(torch.uint8), t.view(torch.uint8))
    return planes, plans


@pytest.mark.parametrize("store", [False, True], ids=["coded", "store"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_frame_decodes_to_the_tensor(gpu_ctx, inputs, case, store):
    name, states, bits, interval, block, n = case
    planes, plans = _round_trip(gpu_ctx, inputs[name][:n], name, states, bits, interval, block, store)
    info = planes.info()
    coded = [p for p in plans if p is not None]
    assert info["coded"] == len(coded) and info["stored"] == len(plans) - len(coded)
    planes.close()
    if coded:  # the batch the object holds is hsrans_dplan_batch_create's over the coded planes
        batch = gpu_ctx.make_batch(coded)
        assert info["launches"] == batch.info()["launches"] + 1
        batch.close()
    else:
        assert info["launches"] == 1


def test_exactly_one_coded_plane(gpu_ctx, inputs):
    planes, plans = _round_trip(gpu_ctx, inputs["mixed"][: 3 * 65536 + 9], "mixed", 64, 11, 32, 1 << 16, store=True)
    assert plans[0] is None and plans[1] is not None
    assert planes.info()["coded"] == 1 and planes.info()["stored"] == 1
    planes.close()


def test_two_decodes_back_to_back_on_one_stream(gpu_ctx, inputs):
    a = inputs["fp32"][: 2 * 65536 + 77]
    t, frame, work, total, desc, plans = _encode(gpu_ctx, a, "fp32", 64, 11, 32, 1 << 16, store=True)
    planes = gpu_ctx.make_planes(desc, plans)
    s = torch.cuda.Stream()
    out1, out2 = torch.zeros_like(t), torch.zeros_like(t)
    s.wait_stream(torch.cuda.current_stream())
    gpu_ctx.decode_device_planes(planes, frame, out1, work, stream=s)
    gpu_ctx.decode_device_planes(planes, frame, out2, work, stream=s)
    assert gpu_ctx.planes_status(planes, stream=s) == [0, 0, 0, 0]
    assert torch.equal(out1.view(torch.uint8), t.view(torch.uint8)) and torch.equal(out2.view(torch.uint8), t.view(torch.uint8))
    planes.close()


def test_a_compacted_frame_decodes(gpu_ctx, inputs):
    """offsets need only be non-overlapping multiples of 16: the planes moved next to each other, in another order"""
    a = inputs["bf16"][: 65536 + 3]
    t, frame, work, total, desc, plans = _encode(gpu_ctx, a, "bf16", 64, 11, 32, 1 << 16, store=True)
    up16 = lambda v: (v + 15) & ~15  # noqa: E731
    packed = _full(up16(desc.length[0]) + up16(desc.length[1]))
    moved = api.PlanesDesc.from_buffer_copy(desc)
    moved.offset[1], moved.offset[0] = 0, up16(desc.length[1])
    for p in range(2):
        packed[moved.offset[p]: moved.offset[p] + desc.length[p]] = frame[desc.offset[p]: desc.offset[p] + desc.length[p]]
    moved.frame_length = moved.offset[0] + desc.length[0]
    planes = gpu_ctx.make_planes(moved, plans)
    out = torch.zeros_like(t)
    gpu_ctx.decode_device_planes(planes, packed, out, work)
    assert gpu_ctx.planes_status(planes) == [0, 0]
    assert torch.equal(out.view(torch.uint8), t.view(torch.uint8))
    planes.close()


# ---- refusals ----
def test_the_encoder_refuses_before_it_launches(gpu_ctx, inputs):
    n = 4096
    a = inputs["fp32"][:n]
    t = _tensor(a, "fp32")
    W, L, ctx = 4, gpu_ctx.L, gpu_ctx.handle
    cap, wb = H.planes_capacity(W, 64, n), H.planes_workspace_bytes(W, n)
    frame, work = _full(cap + 32), _full(wb + 32)
    shared = _full(cap + wb)
    ok = dict(ctx=ctx, W=W, states=64, bits=11, d_in=t.data_ptr(), n=n, d_frame=frame.data_ptr(), cap=cap, block=1 << 16, interval=32, flags=1,
              d_work=work.data_ptr(), wb=wb, desc=True)
    bad = [
        dict(ctx=None), dict(desc=False),
        dict(W=1), dict(W=3), dict(W=16),
        dict(states=48), dict(states=16),
        dict(bits=9), dict(bits=16),
        dict(block=0), dict(block=100),
        dict(interval=6),
        dict(n=0), dict(n=1 << 45),  # (the buffers stay as they are: a count the single call could not take either)
        dict(flags=2), dict(flags=0x80000001),
        dict(d_in=t.data_ptr() + 4), dict(d_frame=frame.data_ptr() + 8), dict(d_work=work.data_ptr() + 1),
        dict(d_in=None), dict(d_frame=None), dict(d_work=None),
        dict(cap=cap - 1), dict(wb=wb - 1),
        dict(d_frame=shared.data_ptr(), d_work=shared.data_ptr() + cap - 256),       # the workspace begins inside the frame
        dict(d_frame=shared.data_ptr(), d_in=shared.data_ptr() + cap - 16),          # the elements begin inside the frame
        dict(d_work=shared.data_ptr(), d_in=shared.data_ptr() + 256),                # the elements lie inside the workspace
    ]
    for change in bad:
        k = dict(ok, **change)
        desc = api.PlanesDesc()
        handles = (ctypes.c_void_p * 8)()
        r = L.hsrans_encode_device_planes(k["ctx"], k["W"], k["states"], k["bits"], k["d_in"], k["n"], k["d_frame"], k["cap"], k["block"], k["interval"], k["flags"],
                                          k["d_work"], k["wb"], None, ctypes.byref(desc) if k["desc"] else None, handles)
        assert r == 0, change
        assert not any(handles), change
        assert bytes(desc) == bytes(api.PlanesDesc()), change
    torch.cuda.synchronize()
    assert _untouched(frame) and _untouched(work) and _untouched(shared)
    # ... and through the wrapper, which raises
    with pytest.raises(H.HsransError):
        gpu_ctx.encode_device_planes(t, frame[: cap - 256], work)
    with pytest.raises(H.HsransError):
        gpu_ctx.encode_device_planes(torch.zeros(64, dtype=torch.uint8, device="cuda"), frame, work)
    torch.cuda.synchronize()
    assert _untouched(frame) and _untouched(work)


def test_the_decoder_and_the_object_refuse_bad_arguments(gpu_ctx, inputs):
    n = 65536 + 1
    a = inputs["bf16"][:n]
    t, frame, work, total, desc, plans = _encode(gpu_ctx, a, "bf16", 64, 11, 32, 1 << 16, store=False)
    W, L, ctx = 2, gpu_ctx.L, gpu_ctx.handle

    # -- hsrans_planes_create --
    def create(d, pl):
        arr = (ctypes.c_void_p * 8)(*[None if p is None else p.handle.value for p in pl])
        h = ctypes.c_void_p()
        rc = L.hsrans_planes_create(ctx, ctypes.byref(d) if d is not None else None, arr, ctypes.byref(h))
        assert (rc == 0) == bool(h.value)
        if h.value:
            L.hsrans_planes_destroy(h)
        return rc

    def changed(**fields):
        d = api.PlanesDesc.from_buffer_copy(desc)
        for key, v in fields.items():
            if isinstance(v, tuple):
                getattr(d, key)[v[0]] = v[1]
            else:
                setattr(d, key, v)
        return d

    assert create(desc, plans) == 0
    assert create(None, plans) == E_ARG
    assert create(desc, [plans[0], None]) == E_ARG                      # a coded plane without its plan
    assert create(changed(stored_mask=1), plans) == E_ARG               # a stored plane with one
    assert create(desc, [plans[0], plans[0]]) == E_ARG                  # one plan twice (and not plane 1's stream)
    assert create(changed(elem_size=3), plans) == E_ARG
    assert create(changed(states=32), plans) == E_ARG                   # not the plans' states
    assert create(changed(bits=12), plans) == E_ARG
    assert create(changed(elements=n - 1), plans) == E_ARG
    assert create(changed(offset=(1, desc.offset[1] + 8)), plans) == E_ARG   # not a multiple of 16
    assert create(changed(offset=(1, 16)), plans) == E_ARG                   # inside plane 0
    assert create(changed(frame_length=desc.frame_length - 1), plans) == E_ARG
    assert create(changed(stored_mask=4), plans) == E_ARG               # a plane the elements do not have

    # -- hsrans_decode_device_planes --
    planes = gpu_ctx.make_planes(desc, plans)
    out = _full(W * n + 32)
    work2 = _full(work.numel() + 32)
    joined = _full(2 * W * n + work.numel())
    ok = dict(ctx=ctx, planes=planes.handle, d_frame=frame.data_ptr(), fl=frame.numel(), d_out=out.data_ptr(), oc=W * n, d_work=work2.data_ptr(), wb=work.numel())
    bad = [
        dict(ctx=None), dict(planes=None),
        dict(d_frame=None), dict(d_out=None), dict(d_work=None),
        dict(d_frame=frame.data_ptr() + 4), dict(d_out=out.data_ptr() + 8), dict(d_work=work2.data_ptr() + 2),
        dict(fl=desc.frame_length - 1), dict(oc=W * n - 1), dict(wb=work.numel() - 1),
        dict(d_out=joined.data_ptr(), d_work=joined.data_ptr() + (W * n & ~15) - 16),   # the workspace begins inside the output
        dict(d_out=frame.data_ptr() + 256, oc=W * n),                                   # the output lies inside the frame
        dict(d_work=frame.data_ptr()),                                                  # the workspace lies on the frame
    ]
    before = frame.clone()
    for change in bad:
        k = dict(ok, **change)
        rc = L.hsrans_decode_device_planes(k["ctx"], k["planes"], k["d_frame"], k["fl"], k["d_out"], k["oc"], k["d_work"], k["wb"], None)
        assert rc == E_ARG, change
    torch.cuda.synchronize()
    assert _untouched(out) and _untouched(work2) and _untouched(joined) and torch.equal(frame, before)
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.decode_device_planes(planes, frame, out[: W * n - 16].view(torch.bfloat16), work2)
    assert e.value.code == E_ARG
    # what was refused still decodes
    good = torch.zeros_like(t)
    gpu_ctx.decode_device_planes(planes, frame, good, work2)
    assert gpu_ctx.planes_status(planes) == [0, 0]
    assert torch.equal(good.view(torch.uint8), t.view(torch.uint8))
    planes.close()
