"""hsrans_*_device_planes_batch: many tensors' frames of byte planes in one call.  Every member of a call against its single call
(hsrans_encode_device_planes: frame bytes, descriptor, stored planes, plan blobs) over a set that holds the task and tail edges of the
one-launch kernels and every element size at once; a launch count that does not grow with the members; sets decoded back to their
tensors and against the single decode; refusals that launch nothing and write nothing."""
import ctypes

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api, synth

pytestmark = pytest.mark.gpu

E_ARG = 2
SENTINEL = 0xA5
PAD = 64  # sentinel bytes behind every frame, workspace and output
N_MAX = 3 * 65536 + 9
DEFAULTS = dict(states=64, bits=11, block_size=1 << 16, index_interval=32, store_incompressible=True)
# (input, elements): 1 task with only a tail; a lane and a tail; one full workgroup and a tail element; 16 full workgroups of 8-byte elements;
# 33 workgroups, the last nearly empty, and a tail; every plane stored; one plane stored and one coded; exactly one full workgroup, no tail
SET = [("bf16", 1), ("fp16", 17), ("fp32", 4097), ("i64", 65536), ("bf16", 2 * 65536 + 77), ("uniform", 65536 + 5), ("mixed", 3 * 65536 + 9), ("fp32", 4096)]


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(43)
    x = rng.standard_normal(N_MAX).astype(np.float32)
    ramp = (np.arange(N_MAX, dtype=np.uint64) << np.uint64(8)) | rng.integers(0, 256, N_MAX, dtype=np.uint64)
    mixed = (rng.integers(0, 256, N_MAX, dtype=np.uint16) | (np.abs(rng.standard_normal(N_MAX) * 3).astype(np.uint16) << 8)).astype(np.uint16)
    return {
        "bf16": (x.view(np.uint32) >> 16).astype(np.uint16),
        "fp16": x.astype(np.float16).view(np.uint16),
        "fp32": x.view(np.uint32),
        "i64": ramp,
        "uniform": synth.uniform_bytes(2 * N_MAX, seed=47).view(np.uint16),  # every plane incompressible
        "mixed": mixed,  # plane 0 uniform, plane 1 small values: exactly one plane worth coding (the "mixed" input of test_gpu_planes.py)
    }


def _tensor(a, name=None):
    t = torch.from_numpy(np.ascontiguousarray(a).view({2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize])).cuda()
    real = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}.get(name)
    return t.view(real) if real is not None else t


def _full(n):
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")


def _untouched(t):
    return bool((t == SENTINEL).all().item())


def _settings(options, k):
    return dict(DEFAULTS, **(options[k] or {})) if options is not None else dict(DEFAULTS)


def _members(inputs, spec):
    return [(name, inputs[name][:n]) for name, n in spec]


def _buffers(members, options=None):
    """fresh sentinel-filled frames (capacity + PAD each) and one workspace (+ PAD) for a call over `members`"""
    frames = [_full(H.planes_capacity(a.itemsize, _settings(options, k)["states"], a.size) + PAD) for k, (_, a) in enumerate(members)]
    work = _full(H.planes_batch_workspace_bytes([a.itemsize for _, a in members], [a.size for _, a in members]) + PAD)
    return frames, work


def _encode_batch(ctx, members, options=None, stats=None, want_plans=True):
    tensors = [_tensor(a, name) for name, a in members]
    frames, work = _buffers(members, options)
    caps = [f[: f.numel() - PAD] for f in frames]
    got = ctx.encode_device_planes_batch(tensors, caps, work[: work.numel() - PAD], options=options, want_plans=want_plans, stats=stats, **DEFAULTS)
    return tensors, frames, work, got


def _encode_single(ctx, name, a, s):
    """the member's single call: (frame with PAD sentinel bytes behind it, frame_length, desc, plans)"""
    t = _tensor(a, name)
    frame = _full(H.planes_capacity(a.itemsize, s["states"], a.size) + PAD)
    work = _full(H.planes_workspace_bytes(a.itemsize, a.size))
    n, desc, plans = ctx.encode_device_planes(t, frame[: frame.numel() - PAD], work, **s)
    return frame, n, desc, plans


def _assert_member_is_its_single_call(ctx, name, a, s, frame, got):
    n, desc, plans = got
    want_frame, want_n, want_desc, want_plans = _encode_single(ctx, name, a, s)
    W = a.itemsize
    assert n == want_n == desc.frame_length and bytes(desc) == bytes(want_desc), name
    assert desc.stored_mask == want_desc.stored_mask and [p is None for p in plans] == [p is None for p in want_plans] == [bool(desc.stored_mask >> p & 1) for p in range(W)]
    mine, want = frame.cpu().numpy(), want_frame.cpu().numpy()
    assert np.array_equal(mine, want), name  # every byte of the capacity and of the pad behind it
    assert np.all(mine[mine.size - PAD:] == SENTINEL), name
    for p in range(W):
        if plans[p] is not None:  # nothing behind a coded plane's data (a stored plane lies over its stream's first bytes, as in the single call)
            end = desc.offset[p + 1] if p + 1 < W else mine.size
            assert np.all(mine[desc.offset[p] + desc.length[p]: end] == SENTINEL), (name, p)
            assert np.array_equal(ctx.read_device_plan(plans[p]), ctx.read_device_plan(want_plans[p])), (name, p)


@pytest.fixture(scope="module")
def encoded(gpu_ctx, inputs):
    """the mixed set encoded once with the default settings: what the encode and the decode tests share"""
    members = _members(inputs, SET)
    stats = {}
    tensors, frames, work, got = _encode_batch(gpu_ctx, members, stats=stats)
    return dict(members=members, tensors=tensors, frames=frames, work=work, got=got, stats=stats)


# ---- encode ----
def test_every_member_is_its_single_call(gpu_ctx, encoded):
    for k, (name, a) in enumerate(encoded["members"]):
        _assert_member_is_its_single_call(gpu_ctx, name, a, DEFAULTS, encoded["frames"][k], encoded["got"][k])
    work = encoded["work"]
    assert _untouched(work[work.numel() - PAD:])
    masks = [g[1].stored_mask for g in encoded["got"]]
    assert masks[5] == 0b11 and masks[6] == 0b01  # all planes stored; one stored and one coded
    st = encoded["stats"]
    assert st["members"] == len(SET) and st["planes"] == sum(a.itemsize for _, a in encoded["members"]) and st["stored"] == sum(bin(m).count("1") for m in masks)


def test_the_launches_do_not_grow_with_the_members(gpu_ctx, inputs, encoded):
    members = _members(inputs, SET * 4)
    stats = {}
    tensors, frames, work, got = _encode_batch(gpu_ctx, members, stats=stats)
    assert len(members) == 32 and stats["members"] == 32 and stats["planes"] == 4 * encoded["stats"]["planes"] and stats["stored"] == 4 * encoded["stats"]["stored"]
    assert stats["launches"] == encoded["stats"]["launches"]
    for k in range(32):  # the repeats are the first eight again, byte for byte
        first = encoded["got"][k % 8]
        assert got[k][0] == first[0] and bytes(got[k][1]) == bytes(first[1]), k
        assert torch.equal(frames[k], encoded["frames"][k % 8]), k


def test_members_with_settings_of_their_own(gpu_ctx, inputs):
    members = _members(inputs, SET)
    other = dict(states=32, bits=13, index_interval=0)
    options = [other, None, other, None, dict(bits=13), dict(store_incompressible=False), other, dict(block_size=1 << 14, index_interval=0)]
    tensors, frames, work, got = _encode_batch(gpu_ctx, members, options=options)
    for k, (name, a) in enumerate(members):
        _assert_member_is_its_single_call(gpu_ctx, name, a, _settings(options, k), frames[k], got[k])
    assert got[5][1].stored_mask == 0 and got[0][1].states == 32 and got[7][1].block_size == 1 << 14
    assert _untouched(work[work.numel() - PAD:])


def test_without_plans_the_frames_are_the_same(gpu_ctx, encoded):
    tensors, frames, work, got = _encode_batch(gpu_ctx, encoded["members"], want_plans=False)
    for k in range(len(SET)):
        assert got[k][2] == [None] * encoded["members"][k][1].itemsize and bytes(got[k][1]) == bytes(encoded["got"][k][1]), k
        assert torch.equal(frames[k], encoded["frames"][k]), k


def test_three_hundred_small_members(gpu_ctx, inputs):
    """more members than a workgroup has lanes: the member search runs over a prefix of 300 entries"""
    members = [("bf16", inputs["bf16"][37 * k: 37 * k + 512]) for k in range(300)]  # one KiB each
    stats = {}
    tensors, frames, work, got = _encode_batch(gpu_ctx, members, stats=stats)
    assert stats["members"] == 300 and stats["planes"] == 600
    for k in (0, 299):
        _assert_member_is_its_single_call(gpu_ctx, "bf16", members[k][1], DEFAULTS, frames[k], got[k])
    pset = gpu_ctx.make_planes_set([g[1] for g in got], [g[2] for g in got])
    outs = [torch.zeros_like(t) for t in tensors]
    gpu_ctx.decode_device_planes_batch(pset, frames, outs, _full(pset.info()["work_bytes"]))
    assert gpu_ctx.planes_set_status(pset) == [0] * 300
    assert all(torch.equal(o.view(torch.uint8), t.view(torch.uint8)) for o, t in zip(outs, tensors))
    pset.close()


# ---- decode ----
def _padded_outputs(tensors):
    """an output per tensor inside a sentinel-filled buffer of PAD bytes more: (buffers, the tensors to decode into)"""
    bufs = [_full(t.numel() * t.element_size() + PAD) for t in tensors]
    return bufs, [b[: b.numel() - PAD].view(t.dtype) for b, t in zip(bufs, tensors)]


def _decode_and_check(ctx, pset, frames, tensors, stream=None):
    bufs, outs = _padded_outputs(tensors)
    work = _full(pset.info()["work_bytes"] + PAD)
    ctx.decode_device_planes_batch(pset, frames, outs, work[: work.numel() - PAD], stream=stream)
    assert ctx.planes_set_status(pset, stream=stream) == [0] * len(tensors)
    for k, (b, o, t) in enumerate(zip(bufs, outs, tensors)):
        assert torch.equal(o.view(torch.uint8), t.view(torch.uint8)), k
        assert _untouched(b[b.numel() - PAD:]), k
    assert _untouched(work[work.numel() - PAD:])
    return outs


def test_the_set_decodes_to_the_tensors_and_to_the_single_decodes(gpu_ctx, encoded):
    got, frames, tensors = encoded["got"], encoded["frames"], encoded["tensors"]
    pset = gpu_ctx.make_planes_set([g[1] for g in got], [g[2] for g in got])
    info = pset.info()
    coded = [p for g in got for p in g[2] if p is not None]
    planes = sum(t.element_size() for t in tensors)
    assert info["members"] == len(SET) and info["coded"] == len(coded) and info["stored"] == planes - len(coded)
    assert info["merge_tasks"] == H.planes_batch_tasks([t.numel() for t in tensors])[0]
    assert info["work_bytes"] == H.planes_batch_workspace_bytes([t.element_size() for t in tensors], [t.numel() for t in tensors])
    outs = _decode_and_check(gpu_ctx, pset, frames, tensors)
    pset.close()
    batch = gpu_ctx.make_batch(coded)  # the batch the set held is hsrans_dplan_batch_create's over all coded planes
    assert info["launches"] == batch.info()["launches"] + 1
    batch.close()
    for k, (n, desc, plans) in enumerate(got):  # ... and every member as hsrans_decode_device_planes decodes it
        single = gpu_ctx.make_planes(desc, plans)
        out = torch.zeros_like(tensors[k])
        gpu_ctx.decode_device_planes(single, frames[k], out, _full(H.planes_workspace_bytes(desc.elem_size, desc.elements)))
        assert gpu_ctx.planes_status(single) == [0] * desc.elem_size
        assert torch.equal(out.view(torch.uint8), outs[k].view(torch.uint8)), k
        single.close()


def test_two_decodes_back_to_back_on_one_stream(gpu_ctx, encoded):
    got, frames, tensors = encoded["got"], encoded["frames"], encoded["tensors"]
    pset = gpu_ctx.make_planes_set([g[1] for g in got], [g[2] for g in got])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    work = _full(pset.info()["work_bytes"])
    outs1, outs2 = [torch.zeros_like(t) for t in tensors], [torch.zeros_like(t) for t in tensors]
    s.wait_stream(torch.cuda.current_stream())
    gpu_ctx.decode_device_planes_batch(pset, frames, outs1, work, stream=s)
    gpu_ctx.decode_device_planes_batch(pset, frames, outs2, work, stream=s)
    assert gpu_ctx.planes_set_status(pset, stream=s) == [0] * len(tensors)
    for a, b, t in zip(outs1, outs2, tensors):
        assert torch.equal(a.view(torch.uint8), t.view(torch.uint8)) and torch.equal(b.view(torch.uint8), t.view(torch.uint8))
    pset.close()


def test_a_set_of_one_member(gpu_ctx, inputs):
    members = _members(inputs, [("fp32", 2 * 65536 + 77)])
    tensors, frames, work, got = _encode_batch(gpu_ctx, members)
    _assert_member_is_its_single_call(gpu_ctx, "fp32", members[0][1], DEFAULTS, frames[0], got[0])
    pset = gpu_ctx.make_planes_set([got[0][1]], [got[0][2]])
    assert pset.info()["members"] == 1
    _decode_and_check(gpu_ctx, pset, frames, tensors)
    pset.close()


def test_a_set_whose_planes_are_all_stored_has_no_batch(gpu_ctx, inputs):
    members = _members(inputs, [("uniform", 65536 + 5), ("uniform", 17), ("uniform", 4096)])
    tensors, frames, work, got = _encode_batch(gpu_ctx, members)
    assert [g[1].stored_mask for g in got] == [0b11] * 3 and all(g[2] == [None, None] for g in got)
    pset = gpu_ctx.make_planes_set([g[1] for g in got], [g[2] for g in got])
    info = pset.info()
    assert (info["coded"], info["stored"], info["launches"]) == (0, 6, 1)
    _decode_and_check(gpu_ctx, pset, frames, tensors)
    pset.close()


# ---- refusals ----
def _c_members(rows):
    arr = (api.PlanesMember * len(rows))()
    for e, r in zip(arr, rows):
        e.elem_size, e.states, e.bits, e.block_size, e.index_interval, e.flags = r["W"], r["states"], r["bits"], r["block"], r["interval"], r["flags"]
        e.d_in, e.elements, e.d_frame, e.frame_capacity = r["d_in"], r["n"], r["d_frame"], r["cap"]
        e.frame_length, e.rc, e.desc.elem_size = 7, 7, 7  # (what a refusal must reset)
    return arr


def _refused(L, ctx, rows, d_work, wb):
    arr = _c_members(rows)
    handles = (ctypes.c_void_p * (8 * len(rows)))(*([1] * (8 * len(rows))))
    stats = api.PlanesBatchStats()
    rc = L.hsrans_encode_device_planes_batch(ctx, arr, len(rows), d_work, wb, None, handles, ctypes.byref(stats))
    zero = bytes(api.PlanesDesc())
    return rc == E_ARG and not any(handles) and all(e.frame_length == 0 and bytes(e.desc) == zero for e in arr) and stats.launches == 0, arr


def test_the_encoder_refuses_before_it_launches(gpu_ctx, inputs):
    n, W, L, ctx = 4096, 4, gpu_ctx.L, gpu_ctx.handle
    tensors = [_tensor(inputs["fp32"][k * n: (k + 1) * n], "fp32") for k in range(3)]
    cap, wb = H.planes_capacity(W, 64, n), 3 * H.planes_workspace_bytes(W, n)
    frames = [_full(cap + 32) for _ in range(3)]
    work = _full(wb + 32)
    shared = _full(2 * cap + wb)
    good = [dict(W=W, states=64, bits=11, block=1 << 16, interval=32, flags=1, d_in=t.data_ptr(), n=n, d_frame=f.data_ptr(), cap=cap) for t, f in zip(tensors, frames)]
    single_call = [
        dict(W=1), dict(W=3), dict(W=16), dict(states=48), dict(states=16), dict(bits=9), dict(bits=16), dict(block=0), dict(block=100), dict(interval=6),
        dict(n=0), dict(n=1 << 45), dict(flags=2), dict(flags=0x80000001), dict(d_in=None), dict(d_frame=None), dict(cap=cap - 1),
    ]
    for at in (0, 2):  # each of the single call's refusals in the first and in the last member
        aligned = [dict(d_in=tensors[at].data_ptr() + 4), dict(d_frame=frames[at].data_ptr() + 8)]
        for change in single_call + aligned:
            rows = [dict(r) for r in good]
            rows[at].update(change)
            ok, arr = _refused(L, ctx, rows, work.data_ptr(), wb)
            assert ok, (at, change)
            assert [e.rc for e in arr] == [E_ARG if k == at else 0 for k in range(3)], (at, change)
    call = [
        (good, dict(d_work=None)), (good, dict(d_work=work.data_ptr() + 1)), (good, dict(wb=wb - 1)),   # the workspace: unset, unaligned, one byte short
        ([good[0], dict(good[1], d_frame=frames[0].data_ptr() + 256), good[2]], {}),                   # two members' frames overlap
        ([good[0], good[1], dict(good[2], d_frame=shared.data_ptr(), d_in=shared.data_ptr() + cap - 16)], {}),  # a member's elements inside its own frame
        ([dict(good[0], d_frame=shared.data_ptr()), dict(good[1], d_in=shared.data_ptr() + 512), good[2]], {}),  # a frame on another member's input
        ([dict(good[0], d_frame=shared.data_ptr()), good[1], good[2]], dict(d_work=shared.data_ptr() + cap - 256)),  # the workspace begins inside a frame
        ([dict(good[0], d_in=shared.data_ptr() + 256), good[1], good[2]], dict(d_work=shared.data_ptr())),  # a member's elements inside the workspace
    ]
    for rows, change in call:
        k = dict(dict(d_work=work.data_ptr(), wb=wb), **change)
        ok, arr = _refused(L, ctx, rows, k["d_work"], k["wb"])
        assert ok, change
    torch.cuda.synchronize()
    assert all(_untouched(f) for f in frames) and _untouched(work) and _untouched(shared)
    # through the wrapper, which raises and names the member
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.encode_device_planes_batch(tensors, [frames[0], frames[1][: cap - 256], frames[2]], work)
    assert e.value.code == E_ARG and e.value.rcs == [0, E_ARG, 0] and "member 1" in str(e.value)
    torch.cuda.synchronize()
    assert all(_untouched(f) for f in frames) and _untouched(work)
    # what was refused still encodes, and round-trips
    got = gpu_ctx.encode_device_planes_batch(tensors, [f[:cap] for f in frames], work[:wb])
    pset = gpu_ctx.make_planes_set([g[1] for g in got], [g[2] for g in got])
    _decode_and_check(gpu_ctx, pset, frames, tensors)
    pset.close()


def test_more_planes_than_the_codec_batch_takes(gpu_ctx, inputs):
    """65,536 planes is the codec batch's limit; element sizes are even, so the first call beyond it has 65,538"""
    K, L, ctx = 32769, gpu_ctx.L, gpu_ctx.handle
    t = _tensor(inputs["bf16"][:1], "bf16")  # (inputs may share memory: every member reads the same element)
    cap, region = H.planes_capacity(2, 64, 1), H.planes_workspace_bytes(2, 1)
    frames, work = _full(K * cap), _full(K * region)
    row = dict(W=2, states=64, bits=11, block=1 << 16, interval=0, flags=1, d_in=t.data_ptr(), n=1, cap=cap)
    rows = [dict(row, d_frame=frames.data_ptr() + k * cap) for k in range(K)]
    ok, _ = _refused(L, ctx, rows, work.data_ptr(), work.numel())
    assert ok
    torch.cuda.synchronize()
    assert _untouched(frames) and _untouched(work)


def test_the_set_and_the_decoder_refuse_bad_arguments(gpu_ctx, encoded):
    got, frames, tensors = encoded["got"][1:4], encoded["frames"][1:4], encoded["tensors"][1:4]  # fp16 17, fp32 4097, i64 65536
    descs, plans = [g[1] for g in got], [g[2] for g in got]
    L, ctx = gpu_ctx.L, gpu_ctx.handle
    with pytest.raises(H.HsransError) as e:  # one plan under two members
        gpu_ctx.make_planes_set([descs[2], descs[1], descs[2]], [plans[2], plans[1], plans[2]])
    assert e.value.code == E_ARG
    assert any(p is not None for p in plans[2])  # (the ramp's high bytes are coded: the set above held them twice)
    coded_at = [p is not None for p in plans[2]].index(True)
    with pytest.raises(H.HsransError) as e:  # a member hsrans_planes_create refuses: a coded plane without its plan
        gpu_ctx.make_planes_set(descs, [plans[0], plans[1], [None if p == coded_at else d for p, d in enumerate(plans[2])]])
    assert e.value.code == E_ARG

    pset = gpu_ctx.make_planes_set(descs, plans)
    wb = pset.info()["work_bytes"]
    bufs, outs = _padded_outputs(tensors)
    work = _full(wb + PAD)
    before = [f.clone() for f in frames]
    sizes = [t.numel() * t.element_size() for t in tensors]
    ok = dict(ctx=ctx, set=pset.handle, frames=[f.data_ptr() for f in frames], fl=[f.numel() for f in frames], outs=[o.data_ptr() for o in outs], oc=list(sizes),
              d_work=work.data_ptr(), wb=wb)

    def with_(key, k, v):
        return {key: [v if j == k else x for j, x in enumerate(ok[key])]}

    bad = [
        dict(ctx=None), dict(set=None), dict(d_work=None), dict(d_work=work.data_ptr() + 2), dict(wb=wb - 1),   # ... a short workspace
        with_("frames", 0, None), with_("outs", 2, None), with_("frames", 1, frames[1].data_ptr() + 4), with_("outs", 0, outs[0].data_ptr() + 8),
        with_("fl", 2, descs[2].frame_length - 1), with_("oc", 0, sizes[0] - 1), with_("oc", 2, sizes[2] - 1),  # a short frame, a short out_capacity
        with_("outs", 0, frames[2].data_ptr() + 256),                                                          # an output inside another member's frame
        with_("outs", 1, outs[2].data_ptr() + 1024),                                                           # two outputs overlap
        dict(d_work=frames[2].data_ptr()),                                                                     # the workspace lies on a frame
        dict(d_work=bufs[2].data_ptr() + 4096),                                                                # ... inside an output
    ]
    for change in bad:
        k = dict(ok, **change)
        arrays = [(ctypes.c_void_p * 3)(*k["frames"]), (ctypes.c_size_t * 3)(*k["fl"]), (ctypes.c_void_p * 3)(*k["outs"]), (ctypes.c_size_t * 3)(*k["oc"])]
        assert L.hsrans_decode_device_planes_batch(k["ctx"], k["set"], *arrays, k["d_work"], k["wb"], None) == E_ARG, change
    assert L.hsrans_decode_device_planes_batch(ctx, pset.handle, None, (ctypes.c_size_t * 3)(*ok["fl"]), (ctypes.c_void_p * 3)(*ok["outs"]), (ctypes.c_size_t * 3)(*ok["oc"]),
                                               work.data_ptr(), wb, None) == E_ARG
    torch.cuda.synchronize()
    assert all(_untouched(b) for b in bufs) and _untouched(work) and all(torch.equal(f, b) for f, b in zip(frames, before))
    with pytest.raises(H.HsransError) as e:  # through the wrapper: an output too small
        gpu_ctx.decode_device_planes_batch(pset, frames, [outs[0], outs[1][:-4], outs[2]], work[:wb])
    assert e.value.code == E_ARG
    # what was refused still decodes
    _decode_and_check(gpu_ctx, pset, frames, tensors)
    pset.close()
