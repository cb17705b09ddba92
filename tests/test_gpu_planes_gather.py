"""hsrans_decode_device_planes_gather: element ranges of a frame of byte planes that stays compressed.  Every expected value is a numpy slice
of the ORIGINAL array; the output and the workspace are pre-filled with a sentinel and compared whole — the output against the ranges'
elements and nothing else, the workspace against the layout the header promises (so no byte outside the ranges' slots is written)."""
import ctypes

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api, synth

pytestmark = pytest.mark.gpu

E_ARG = 2
SENTINEL = 0xA5
N = 300_007  # 5 blocks of 64 KiB per plane; not a multiple of 16
BLOCK = 1 << 16
NP_INT = {2: np.int16, 4: np.int32, 8: np.int64}
TORCH_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def _up(v, a):
    return (v + a - 1) // a * a


# ---- inputs (as tests/test_gpu_planes.py makes them) and their frames, made once ----
@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(29)
    x = rng.standard_normal(N).astype(np.float32)
    ramp = (np.arange(N, dtype=np.uint64) << np.uint64(8)) | rng.integers(0, 256, N, dtype=np.uint64)  # noise in the low byte
    mixed = (rng.integers(0, 256, N, dtype=np.uint16) | (np.abs(rng.standard_normal(N) * 3).astype(np.uint16) << 8)).astype(np.uint16)
    return {
        "bf16": (x.view(np.uint32) >> 16).astype(np.uint16),
        "fp32": x.view(np.uint32),
        "i64": ramp,
        "uniform": synth.uniform_bytes(2 * N, seed=31).view(np.uint16),  # every plane stored
        "mixed": mixed,  # exactly one coded plane
    }


def _full(n):
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")


class Frame:
    def __init__(self, ctx, a, states, bits, interval, store):
        self.a, self.W = a, a.itemsize
        self.t = torch.from_numpy(np.ascontiguousarray(a).view(NP_INT[self.W])).cuda()
        self.frame = _full(H.planes_capacity(self.W, states, a.size))
        work = _full(H.planes_workspace_bytes(self.W, a.size))
        _, self.desc, self.plans = ctx.encode_device_planes(self.t, self.frame, work, states=states, bits=bits, block_size=BLOCK, index_interval=interval,
                                                            store_incompressible=store)
        self.planes = ctx.make_planes(self.desc, self.plans)
        self.pg = ctx.make_planes_gather(self.planes, self.frame)
        self.coded = [p for p in range(self.W) if self.plans[p] is not None]
        self.rows = a.view(np.uint8).reshape(-1, self.W)  # rows[i, p] = plane p's byte of element i


# (input, states, bits, index_interval, store incompressible planes)
FRAMES = {
    "bf16-coded": ("bf16", 64, 11, 32, False),
    "bf16-store": ("bf16", 64, 11, 32, True),
    "fp32-coded": ("fp32", 64, 11, 32, False),
    "fp32-store": ("fp32", 64, 11, 32, True),
    "fp32-s32-b13": ("fp32", 32, 13, 32, True),  # another gather kind
    "fp32-i0": ("fp32", 64, 11, 0, True),        # no checkpoints: a chain per block
    "i64-coded": ("i64", 64, 11, 32, False),
    "i64-store": ("i64", 64, 11, 32, True),
    "uniform": ("uniform", 64, 11, 32, True),
    "mixed": ("mixed", 64, 11, 32, True),
}


@pytest.fixture(scope="module")
def frames(gpu_ctx, inputs):
    made = {}

    def get(key):
        if key not in made:
            name, states, bits, interval, store = FRAMES[key]
            made[key] = Frame(gpu_ctx, inputs[name], states, bits, interval, store)
        return made[key]

    yield get
    for f in made.values():
        f.pg.close()
        f.planes.close()


# ---- the range list: (offset, length, destination rule); "al": the destination's byte address is 16-aligned against the source's 16-element
# grid (dst_offset - offset a multiple of 16: whole blocks leave as 16-byte stores), "el": it is only element-aligned (dst_offset - offset odd) ----
SHAPES = [
    (0, 1, "al"),                 # element 0
    (N - 1, 1, "el"),             # the last element (of a tensor that ends inside a 16-element block)
    (16 * 50 + 1, 15, "al"),      # phase 1
    (16 * 70 + 15, 16, "el"),     # phase 15
    (4096, 17, "al"),             # phase 0
    (10_001, 4095, "el"),         # phase 1
    (20_015, 4097, "al"),         # phase 15, two tasks
    (123, 0, "el"),               # empty
    (60_000, 70_001, "el"),       # crosses two mt_ block boundaries; 18 tasks
    (20_000, 300, "al"),          # overlaps (20_015, 4097) in the source
    (N - 70, 70, "al"),           # whole blocks, then a tail that ends with the tensor
    (32, 16, "el"), (48, 16, "al"),  # exactly one aligned block each
]


def _ranges(shapes=SHAPES, first=0):
    """destinations packed in list order, each moved up to the next offset that meets its rule; returns (ranges, output elements)"""
    out, at = [], first
    for off, n, rule in shapes:
        want = off % 16 if rule == "al" else (off + 1) % 2
        while at % 16 != want if rule == "al" else at % 2 != want:
            at += 1
        out.append((off, n, at))
        at += n
    return out, at


def _expected_out(f, ranges, out_elements):
    want = np.full(out_elements * f.W, SENTINEL, np.uint8)
    flat = f.a.view(np.uint8)
    for off, n, dst in ranges:
        want[dst * f.W: (dst + n) * f.W] = flat[off * f.W: (off + n) * f.W]
    return want


def _layout(ranges):
    """[(B_r, phase)] per range and the sum of the slots: the header's workspace layout"""
    at, out = 0, []
    for off, n, _ in ranges:
        out.append((at, off % 16))
        at += _up(off % 16 + n, 16) if n else 0
    return out, at


def _expected_work(f, ranges, work_bytes):
    want = np.full(work_bytes, SENTINEL, np.uint8)
    slots, total = _layout(ranges)
    stride = _up(total, 256)
    for p in f.coded:
        for (off, n, _), (b, phase) in zip(ranges, slots):
            want[p * stride + b + phase: p * stride + b + phase + n] = f.rows[off: off + n, p]
    return want, f.W * stride


def _gather(ctx, f, ranges, out_elements, pg=None, stream=None, extra=0):
    out = _full(out_elements * f.W)
    total = sum(n for _, n, _ in ranges)
    work = _full(H.planes_gather_workspace_bytes(f.W, len(ranges), total) + 256 + extra)
    ctx.decode_device_planes_gather(pg or f.pg, ranges, out.view(TORCH_INT[f.W]), work, stream=stream)
    return out, work


def _check(ctx, f, ranges, out_elements, out, work, pg=None, stream=None):
    assert ctx.planes_gather_status(pg or f.pg, stream=stream) == [0] * f.W
    assert np.array_equal(out.cpu().numpy(), _expected_out(f, ranges, out_elements))
    want_work, need = _expected_work(f, ranges, work.numel())
    assert need <= work.numel() - 256
    assert np.array_equal(work.cpu().numpy(), want_work)


@pytest.mark.parametrize("key", sorted(FRAMES))
def test_one_call_over_the_range_list(gpu_ctx, frames, key):
    f = frames(key)
    name, states, bits, interval, store = FRAMES[key]
    if key == "uniform":
        assert f.coded == []
    if key == "mixed":
        assert f.coded == [1]
    if not store:
        assert len(f.coded) == f.W
    ranges, n_out = _ranges()
    # both store paths are in the list: destinations whose byte address is 16-aligned and ones that are only element-aligned
    assert any((dst - off) % 16 == 0 and n >= 32 for off, n, dst in ranges) and any((dst - off) % 2 == 1 and n >= 32 for off, n, dst in ranges)
    out, work = _gather(gpu_ctx, f, ranges, n_out + 5)
    _check(gpu_ctx, f, ranges, n_out + 5, out, work)
    info = f.pg.info()
    assert info["coded"] == len(f.coded) and info["stored"] == f.W - len(f.coded)
    assert info["rows"] == len(ranges) * len(f.coded)
    assert info["merge_tasks"] == H.planes_gather_tasks(ranges, N).shape[0]
    if not f.coded:
        assert info["launches"] == 1


@pytest.mark.parametrize("key", ["bf16-store", "fp32-coded", "i64-store", "mixed"])
def test_the_launches_are_the_sets_plus_the_merge(gpu_ctx, frames, key):
    """the same rows through a gather set of the test's own over the coded planes: its launches + 1, and the same workspace bytes"""
    f = frames(key)
    ranges, n_out = _ranges()
    out, work = _gather(gpu_ctx, f, ranges, n_out)
    torch.cuda.synchronize()
    slots, total = _layout(ranges)
    stride = _up(total, 256)
    streams = [f.frame[f.desc.offset[p]: f.desc.offset[p] + f.desc.length[p]] for p in f.coded]
    gset = gpu_ctx.make_gather_set([f.plans[p] for p in f.coded], streams)
    rows = [(k, off, n, p * stride + b + phase) for (off, n, _), (b, phase) in zip(ranges, slots) for k, p in enumerate(f.coded)]
    work2 = _full(work.numel())
    gpu_ctx.decode_device_gather_batch(gset, rows, work2)
    assert gpu_ctx.gather_set_status(gset) == [0] * len(f.coded)
    assert f.pg.info()["launches"] == gset.info()["launches"] + 1
    assert torch.equal(work, work2)
    gset.close()


@pytest.mark.parametrize("key", ["bf16-store", "fp32-coded", "fp32-i0", "i64-store", "uniform"])
def test_one_range_over_the_whole_tensor_is_the_whole_decode(gpu_ctx, frames, key):
    f = frames(key)
    whole = torch.zeros_like(f.t)
    gpu_ctx.decode_device_planes(f.planes, f.frame, whole, _full(H.planes_workspace_bytes(f.W, N)))
    assert gpu_ctx.planes_status(f.planes) == [0] * f.W
    out, work = _gather(gpu_ctx, f, [(0, N, 0)], N + 3)
    _check(gpu_ctx, f, [(0, N, 0)], N + 3, out, work)
    assert torch.equal(out[: N * f.W], whole.view(torch.uint8)) and torch.equal(whole, f.t)


@pytest.mark.parametrize("key", ["bf16-store", "fp32-store", "i64-coded"])
def test_shuffled_rows(gpu_ctx, frames, key):
    f = frames(key)
    picked = np.random.default_rng(7).permutation(N // 1000)[:64]
    ranges = [(int(r) * 1000, 1000, k * 1000) for k, r in enumerate(picked)]
    out, work = _gather(gpu_ctx, f, ranges, 64_000)
    _check(gpu_ctx, f, ranges, 64_000, out, work)
    table = f.a[: N // 1000 * 1000].reshape(-1, 1000)
    assert np.array_equal(out.cpu().numpy().view(f.a.dtype).reshape(64, 1000), table[picked])


def test_a_compacted_frame_gathers_the_same(gpu_ctx, frames):
    """offsets need only be non-overlapping multiples of 16: the planes moved next to each other, in another order"""
    f = frames("bf16-store")
    desc = f.desc
    up16 = lambda v: (v + 15) & ~15  # noqa: E731
    packed = _full(up16(desc.length[0]) + up16(desc.length[1]))
    moved = api.PlanesDesc.from_buffer_copy(desc)
    moved.offset[1], moved.offset[0] = 0, up16(desc.length[1])
    for p in range(2):
        packed[moved.offset[p]: moved.offset[p] + desc.length[p]] = f.frame[desc.offset[p]: desc.offset[p] + desc.length[p]]
    moved.frame_length = moved.offset[0] + desc.length[0]
    planes = gpu_ctx.make_planes(moved, f.plans)
    pg = gpu_ctx.make_planes_gather(planes, packed)
    ranges, n_out = _ranges()
    out, work = _gather(gpu_ctx, f, ranges, n_out, pg=pg)
    _check(gpu_ctx, f, ranges, n_out, out, work, pg=pg)
    pg.close()
    planes.close()


def test_two_calls_back_to_back_and_the_planes_object_still_decodes(gpu_ctx, frames):
    f = frames("fp32-store")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    r1, n1 = _ranges()
    r2, n2 = _ranges(SHAPES[::-1], first=11)
    with torch.cuda.stream(s):
        out1, work1 = _gather(gpu_ctx, f, r1, n1, stream=s)
        out2, work2 = _gather(gpu_ctx, f, r2, n2, stream=s)
        _check(gpu_ctx, f, r2, n2, out2, work2, stream=s)
        _check(gpu_ctx, f, r1, n1, out1, work1, stream=s)
    # the planes object the gather object borrows is as it was
    whole = torch.zeros_like(f.t)
    gpu_ctx.decode_device_planes(f.planes, f.frame, whole, _full(H.planes_workspace_bytes(f.W, N)))
    assert gpu_ctx.planes_status(f.planes) == [0] * f.W
    assert torch.equal(whole, f.t)


def test_empty_calls_write_nothing(gpu_ctx, frames):
    f = frames("fp32-store")
    L = gpu_ctx.L
    out, work = _full(4096), _full(4096)
    args = (out.data_ptr(), out.numel(), work.data_ptr(), work.numel(), None)
    assert L.hsrans_decode_device_planes_gather(gpu_ctx.handle, f.pg.handle, None, 0, *args) == 0
    empty = np.asarray([(5, 0, 0), (N, 0, 1024), (0, 0, 7)], np.uint64)
    assert L.hsrans_decode_device_planes_gather(gpu_ctx.handle, f.pg.handle, empty.ctypes.data, 3, *args) == 0
    gpu_ctx.decode_device_planes_gather(f.pg, [], out.view(torch.int32), work)
    assert gpu_ctx.planes_gather_status(f.pg) == [0] * 4
    assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all())
    info = f.pg.info()
    assert (info["rows"], info["merge_tasks"], info["launches"]) == (0, 0, 0)


def test_the_call_and_the_object_refuse_bad_arguments(gpu_ctx, frames, inputs):
    f = frames("fp32-store")
    W, L, ctx = 4, gpu_ctx.L, gpu_ctx.handle
    other = H.Context(0)

    # -- hsrans_planes_gather_create --
    def create(c, planes, d_frame, length, want_out=True):
        h = ctypes.c_void_p()
        rc = L.hsrans_planes_gather_create(c, planes, d_frame, length, ctypes.byref(h) if want_out else None)
        assert (rc == 0) == bool(h.value)
        if h.value:
            L.hsrans_planes_gather_destroy(h)
        return rc

    fp, fl = f.frame.data_ptr(), f.frame.numel()
    assert create(ctx, f.planes.handle, fp, fl) == 0
    assert create(ctx, f.planes.handle, fp, f.desc.frame_length) == 0
    assert create(None, f.planes.handle, fp, fl) == E_ARG
    assert create(ctx, None, fp, fl) == E_ARG
    assert create(ctx, f.planes.handle, None, fl) == E_ARG
    assert create(ctx, f.planes.handle, fp, fl, want_out=False) == E_ARG
    assert create(other.handle, f.planes.handle, fp, fl) == E_ARG          # a planes object of another context
    assert create(ctx, f.planes.handle, fp + 8, fl - 8) == E_ARG          # a misaligned frame
    assert create(ctx, f.planes.handle, fp, f.desc.frame_length - 1) == E_ARG

    # -- hsrans_decode_device_planes_gather --
    ranges = [(100, 5000, 0), (7, 0, 3), (N - 9, 9, 5003)]
    n_out = 5012
    need = W * _up(_layout(ranges)[1], 256)
    out, work = _full(W * n_out + 32), _full(need + 32)
    joined = _full(W * n_out + need + 64)
    # a gather object of another context, over planes of that context
    o_t, o_frame, o_work = f.t.clone(), _full(f.frame.numel()), _full(H.planes_workspace_bytes(W, N))
    _, o_desc, o_plans = other.encode_device_planes(o_t, o_frame, o_work)
    o_planes = other.make_planes(o_desc, o_plans)
    o_pg = other.make_planes_gather(o_planes, o_frame)

    def arr(rows):
        return np.ascontiguousarray(np.asarray(rows, dtype=np.uint64).reshape(-1, 3))

    ok = dict(ctx=ctx, pg=f.pg.handle, ranges=arr(ranges), count=3, d_out=out.data_ptr(), oc=W * n_out, d_work=work.data_ptr(), wb=need)
    big = 1 << 62
    bad = [
        dict(ctx=None), dict(pg=None), dict(ranges=None), dict(d_out=None), dict(d_work=None),
        dict(pg=o_pg.handle),                                                  # a gather object of another context
        dict(ctx=other.handle),
        dict(d_out=out.data_ptr() + 8), dict(d_work=work.data_ptr() + 4),      # alignment
        dict(ranges=arr([(N, 1, 0)]), count=1),                                # beyond the tensor
        dict(ranges=arr([(N - 4, 5, 0)]), count=1),
        dict(ranges=arr([(N + 1, 0, 0)]), count=1),
        dict(ranges=arr([(2**64 - 2, 4, 0)]), count=1),                        # offset + length overflows
        dict(oc=W * n_out - 1),                                                # beyond the output
        dict(ranges=arr([(0, 16, n_out - 15)]), count=1),
        dict(ranges=arr([(0, 16, 2**64 - 8)]), count=1),                       # dst_offset + length overflows
        dict(ranges=arr([(0, 16, big)]), count=1),                             # (dst_offset + length) * elem_size overflows
        dict(wb=need - 1),                                                     # below this call's layout
        dict(wb=0),
        dict(d_out=joined.data_ptr(), d_work=joined.data_ptr() + (W * n_out & ~15) - 16),  # the workspace begins inside the output
        dict(d_out=f.frame.data_ptr() + 256),                                  # the output lies inside the frame
        dict(d_work=f.frame.data_ptr()),                                       # the workspace lies on the frame
    ]
    before = f.frame.clone()
    for change in bad:
        k = dict(ok, **change)
        r = k["ranges"]
        rc = L.hsrans_decode_device_planes_gather(k["ctx"], k["pg"], None if r is None else r.ctypes.data, k["count"], k["d_out"], k["oc"], k["d_work"], k["wb"], None)
        assert rc == E_ARG, {n: v for n, v in change.items() if n != "ranges"}
    # count * elem_size at 2^31: refused before the ranges are read (the pointer is never followed that far)
    one = arr([(0, 0, 0)])
    assert L.hsrans_decode_device_planes_gather(ctx, f.pg.handle, one.ctypes.data, (1 << 31) // W, out.data_ptr(), W * n_out, work.data_ptr(), need, None) == E_ARG
    torch.cuda.synchronize()
    for t in (out, work, joined):
        assert bool((t == SENTINEL).all())
    assert torch.equal(f.frame, before)
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.decode_device_planes_gather(f.pg, ranges, out[: W * n_out - 16].view(torch.int32), work)
    assert e.value.code == E_ARG
    # the wrapper's own refusals: an output tensor of another element size, a workspace that is not bytes
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_planes_gather(f.pg, ranges, out.view(torch.int16), work)
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_planes_gather(f.pg, ranges, out.view(torch.int32), work.view(torch.int32))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all())
    # what was refused still gathers
    good, gwork = _gather(gpu_ctx, f, ranges, n_out)
    _check(gpu_ctx, f, ranges, n_out, good, gwork)
    o_pg.close()
    o_planes.close()
