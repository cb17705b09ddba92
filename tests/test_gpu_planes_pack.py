"""hsrans_pack_device and hsrans_planes_pack_device: many streams, or many frames of byte planes, into one exact-size arena in one launch.
Every arena is pre-filled with a sentinel and has PAD sentinel bytes behind it; every source has sentinel bytes behind its length, so a pad
that is copied instead of written as zero shows.  The stream layer against a numpy model at the chunk's and the 16-byte unit's edges and
over tables that make the item search work; then real streams and real frames decoded, gathered and repacked from the arena's slices."""
import ctypes

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api, synth

pytestmark = pytest.mark.gpu

E_ARG = 2
SENTINEL = 0xA5
PAD = 64
C = H.PACK_CHUNK
DEFAULTS = dict(states=64, bits=11, block_size=1 << 16, index_interval=32, store_incompressible=True)
NP_INT = {2: np.int16, 4: np.int32, 8: np.int64}


def up16(v):
    return (int(v) + 15) // 16 * 16


def _full(n):
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")


def _untouched(t):
    return bool((t == SENTINEL).all().item())


# ---- layer 1 against a numpy model ----
def _sources(lengths, seed, only16=False):
    """one buffer that holds every item at a 16-byte aligned offset — with only16 at an odd multiple of 16 of a 256-byte aligned buffer —
    random bytes over its length and the sentinel everywhere else.  Returns (device buffer, host copy, the items' offsets in it)."""
    rng = np.random.default_rng(seed)
    at, starts = 16 if only16 else 0, []
    for n in lengths:
        starts.append(at)
        at += ((up16(n) + 31) // 32 * 32 + 32) if only16 else up16(n) + 16  # (sentinel behind every item; with only16 every start stays an odd multiple of 16)
    host = np.full(at + PAD, SENTINEL, np.uint8)
    for s, n in zip(starts, lengths):
        host[s: s + n] = rng.integers(0, 256, n, dtype=np.uint8)
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 256 == 0 and (not only16 or all(s % 32 == 16 for s in starts))
    return buf, host, starts


def _pack_and_check(ctx, lengths, seed, only16=False):
    buf, host, starts = _sources(lengths, seed, only16)
    total, offsets = H.pack_layout(lengths)
    assert total == sum(up16(n) for n in lengths)
    arena = _full(total + PAD)
    got = ctx.pack_device([buf[s:] for s in starts], lengths, arena[:total])
    assert got == offsets
    torch.cuda.synchronize()
    mine = arena.cpu().numpy()
    want = np.zeros(total, np.uint8)  # the pads are zero, whatever lies behind the sources
    for s, n, o in zip(starts, lengths, offsets):
        want[o: o + n] = host[s: s + n]
    assert np.array_equal(mine[:total], want)
    assert np.all(mine[total:] == SENTINEL)  # nothing behind offsets[count]
    assert np.array_equal(buf.cpu().numpy(), host)  # (the sources are only read)


@pytest.mark.parametrize("length", [1, 15, 16, 17, C - 1, C, C + 1, 2 * C + 5])
def test_one_item_of_each_edge_length(gpu_ctx, length):
    _pack_and_check(gpu_ctx, [length], seed=length)


def test_the_item_search(gpu_ctx):
    _pack_and_check(gpu_ctx, [C + 1, 1, C, 17, 2 * C], seed=3)  # items of 2, 1, 1, 1 and 2 tasks
    _pack_and_check(gpu_ctx, [2 * C + 5], seed=4)               # count = 1: nothing to search
    rng = np.random.default_rng(5)
    _pack_and_check(gpu_ctx, [int(v) for v in rng.integers(1, 49, 300)], seed=6)  # more items than a workgroup has lanes, one task each
    _pack_and_check(gpu_ctx, [C + 1, 1, C, 17, 2 * C, 33], seed=7, only16=True)    # sources that are only 16-byte aligned


def test_real_streams_decode_from_the_arena(gpu_ctx):
    rng = np.random.default_rng(11)
    sizes = [(H.RAW, 65536 + 5, {"index_interval": 32}), (H.MT, 3 * 65536 + 77, {"block_size": 1 << 16, "index_interval": 32}),
             (H.MT, 4095, {"block_size": 1 << 14, "index_interval": 4})]
    data = [np.clip(rng.standard_normal(n) * 20 + 128, 0, 255).astype(np.uint8) for _, n, _ in sizes]
    d_in = [torch.from_numpy(a).cuda() for a in data]
    d_out = [_full(H.capacity(c, 64, n)) for c, n, _ in sizes]
    lengths, plans = gpu_ctx.encode_device_batch([(c, 64, 11, d_in[k], d_out[k], o) for k, (c, _, o) in enumerate(sizes)], want_plans=True)
    assert all(p is not None for p in plans) and all(0 < n <= d.numel() for n, d in zip(lengths, d_out))
    total, offsets = H.pack_layout(lengths)
    assert total < sum(d.numel() for d in d_out)
    arena = _full(total + PAD)
    assert gpu_ctx.pack_device(d_out, lengths, arena[:total]) == offsets
    batch = gpu_ctx.make_batch(plans)
    outs = [torch.zeros_like(t) for t in d_in]
    gpu_ctx.decode_device_batch(batch, [arena[offsets[k]: offsets[k] + lengths[k]] for k in range(3)], outs)
    assert gpu_ctx.batch_status(batch) == [0, 0, 0]
    for k in range(3):
        assert torch.equal(outs[k], d_in[k]), k
        assert torch.equal(arena[offsets[k]: offsets[k] + lengths[k]], d_out[k][: lengths[k]]), k
        assert not arena[offsets[k] + lengths[k]: offsets[k + 1]].any(), k
    assert _untouched(arena[total:])
    batch.close()


# ---- frames ----
def _tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(NP_INT[a.itemsize])).cuda()


class Frames:
    """five tensors encoded in one call, and their frames packed into one arena"""

    def __init__(self, ctx):
        rng = np.random.default_rng(17)
        x = rng.standard_normal(65536 + 3).astype(np.float32)
        self.arrays = [
            (x.view(np.uint32) >> 16).astype(np.uint16),                                                                    # bf16: one stored, one coded plane
            x[:4096].view(np.uint32).copy(),                                                                                # fp32
            (np.arange(1000, dtype=np.uint64) << np.uint64(8)) | rng.integers(0, 256, 1000, dtype=np.uint64),               # an 8-byte ramp
            synth.uniform_bytes(2 * 5000, seed=19).view(np.uint16),                                                         # every plane stored
            (x[:17].view(np.uint32) >> 16).astype(np.uint16),                                                               # 17 elements
        ]
        self.tensors = [_tensor(a) for a in self.arrays]
        self.frames = [_full(H.planes_capacity(a.itemsize, 64, a.size)) for a in self.arrays]
        work = _full(H.planes_batch_workspace_bytes([a.itemsize for a in self.arrays], [a.size for a in self.arrays]))
        got = ctx.encode_device_planes_batch(self.tensors, self.frames, work, **DEFAULTS)
        self.descs, self.plans = [g[1] for g in got], [g[2] for g in got]
        self.want_descs, self.bases, self.total = H.planes_pack_layout(self.descs)
        self.buf = _full(self.total + PAD)
        self.arena = self.buf[: self.total]
        self.packed_descs, self.slices = ctx.planes_pack_device(self.descs, self.frames, self.arena)
        torch.cuda.synchronize()


@pytest.fixture(scope="module")
def packed(gpu_ctx):
    return Frames(gpu_ctx)


def _decode_set(ctx, descs, plans, frames, tensors, stream=None):
    pset = ctx.make_planes_set(descs, plans)
    bufs = [_full(t.numel() * t.element_size() + PAD) for t in tensors]
    outs = [b[: b.numel() - PAD].view(t.dtype) for b, t in zip(bufs, tensors)]
    work = _full(pset.info()["work_bytes"])
    ctx.decode_device_planes_batch(pset, frames, outs, work, stream=stream)
    status = ctx.planes_set_status(pset, stream=stream)
    pset.close()
    assert status == [0] * len(tensors)
    for k, (b, o, t) in enumerate(zip(bufs, outs, tensors)):
        assert torch.equal(o.view(torch.uint8), t.view(torch.uint8)), k
        assert _untouched(b[b.numel() - PAD:]), k


def test_the_arena_holds_every_plane_where_the_layout_says(gpu_ctx, packed):
    f = packed
    assert f.descs[0].stored_mask == 0b01 and f.descs[3].stored_mask == 0b11 and all(any(p is not None for p in f.plans[k]) for k in (0, 1, 2))
    assert f.total == sum(up16(d.length[p]) for d in f.descs for p in range(d.elem_size)) < sum(d.frame_length for d in f.descs)
    assert [bytes(d) for d in f.packed_descs] == [bytes(d) for d in f.want_descs]
    arena = f.buf.cpu().numpy()
    covered = np.zeros(f.total, bool)
    for k, (src, dst) in enumerate(zip(f.descs, f.packed_descs)):
        frame = f.frames[k].cpu().numpy()
        assert f.slices[k].data_ptr() == f.arena.data_ptr() + f.bases[k] and f.slices[k].numel() == dst.frame_length and f.bases[k] % 16 == 0
        for p in range(src.elem_size):
            at, n = f.bases[k] + dst.offset[p], src.length[p]
            assert np.array_equal(arena[at: at + n], frame[src.offset[p]: src.offset[p] + n]), (k, p)
            assert not arena[at + n: at + up16(n)].any(), (k, p)
            covered[at: at + up16(n)] = True
    assert covered.all() and np.all(arena[f.total:] == SENTINEL)


def test_the_set_decodes_from_the_arenas_slices(gpu_ctx, packed):
    _decode_set(gpu_ctx, packed.packed_descs, packed.plans, packed.slices, packed.tensors)
    assert _untouched(packed.buf[packed.total:])


def _gather_rows(f):
    """a fixed list of rows (member, offset, length, dst_offset) over all five members, their destinations side by side on 16-byte steps"""
    shapes = {0: [(0, 1), (65536 + 2, 1), (4090, 4100), (65536 - 20, 23)], 1: [(17, 300), (4095, 1), (0, 4096)], 2: [(1, 998), (999, 1)], 3: [(123, 4000), (4999, 1)],
              4: [(0, 17), (16, 1), (5, 7)]}
    rows, at = [], 0
    for i in range(4):
        for k in range(5):
            if i < len(shapes[k]):
                W = f.arrays[k].itemsize
                offset, length = shapes[k][i]
                rows.append((k, offset, length, at // W))
                at = up16(at + length * W)
    return rows, at


def test_the_gathers_read_the_arena_as_they_read_the_frames(gpu_ctx, packed):
    f = packed
    rows, out_bytes = _gather_rows(f)
    want = np.full(out_bytes, SENTINEL, np.uint8)
    for k, offset, length, dst in rows:
        W = f.arrays[k].itemsize
        want[dst * W: (dst + length) * W] = f.arrays[k][offset: offset + length].view(np.uint8)
    d_rows = torch.from_numpy(np.asarray([(o, n, d, k) for k, o, n, d in rows], np.int64)).cuda()
    wb = H.planes_gather_batch_workspace_bytes(8, len(rows), sum(r[2] for r in rows)) + 256
    results = []
    for descs, frames in ((f.descs, f.frames), (f.packed_descs, f.slices)):
        pset = gpu_ctx.make_planes_set(descs, f.plans)
        pgs = gpu_ctx.make_planes_gather_set(pset, frames)
        out, out_indirect = _full(out_bytes), _full(out_bytes)
        gpu_ctx.decode_device_planes_gather_batch(pgs, rows, out, _full(wb))
        gpu_ctx.decode_device_planes_gather_batch_indirect(pgs, d_rows, out_indirect, _full(wb))
        assert gpu_ctx.planes_gather_set_refused(pgs) == 0 and gpu_ctx.planes_gather_set_status(pgs) == [0] * 5
        results.append((out.cpu().numpy(), out_indirect.cpu().numpy()))
        pgs.close()
        pset.close()
    (unpacked, unpacked_indirect), (from_arena, from_arena_indirect) = results
    assert np.array_equal(unpacked, want) and np.array_equal(unpacked_indirect, want)
    assert np.array_equal(from_arena, unpacked) and np.array_equal(from_arena_indirect, unpacked_indirect)


def test_one_member_decodes_from_its_slice(gpu_ctx, packed):
    f = packed
    for k in (0, 2):
        planes = gpu_ctx.make_planes(f.packed_descs[k], f.plans[k])
        out = torch.zeros_like(f.tensors[k])
        gpu_ctx.decode_device_planes(planes, f.slices[k], out, _full(H.planes_workspace_bytes(f.arrays[k].itemsize, f.arrays[k].size)))
        assert gpu_ctx.planes_status(planes) == [0] * f.arrays[k].itemsize
        assert torch.equal(out.view(torch.uint8), f.tensors[k].view(torch.uint8)), k
        planes.close()


def test_the_survivors_of_an_arena_pack_into_another(gpu_ctx, packed):
    f = packed
    keep = [0, 2, 4]
    descs, plans, tensors = [f.packed_descs[k] for k in keep], [f.plans[k] for k in keep], [f.tensors[k] for k in keep]
    sources = [f.slices[k] for k in keep]
    assert all(s.data_ptr() % 16 == 0 for s in sources) and any(s.data_ptr() % 256 != 0 for s in sources)
    total = H.planes_pack_layout(descs)[2]
    assert total == sum(f.bases[k + 1] - f.bases[k] for k in keep)
    second = _full(total + PAD)
    descs2, slices2 = gpu_ctx.planes_pack_device(descs, sources, second[:total])
    assert [bytes(d) for d in descs2] == [bytes(d) for d in descs]  # (the layout is idempotent)
    _decode_set(gpu_ctx, descs2, plans, slices2, tensors)
    direct = _full(total + PAD)
    descs3, _ = gpu_ctx.planes_pack_device([f.descs[k] for k in keep], [f.frames[k] for k in keep], direct[:total])
    assert [bytes(d) for d in descs3] == [bytes(d) for d in descs2]
    assert torch.equal(second, direct) and _untouched(second[total:])


def test_two_packs_and_a_decode_queued_on_a_side_stream(gpu_ctx, packed):
    f = packed
    first, second = _full(f.total + PAD), _full(f.total + PAD)
    pset = gpu_ctx.make_planes_set(f.packed_descs, f.plans)
    outs = [torch.zeros_like(t) for t in f.tensors]
    work = _full(pset.info()["work_bytes"])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    descs1, slices1 = gpu_ctx.planes_pack_device(f.descs, f.frames, first[: f.total], stream=side)
    descs2, slices2 = gpu_ctx.planes_pack_device(descs1, slices1, second[: f.total], stream=side)
    gpu_ctx.decode_device_planes_batch(pset, slices2, outs, work, stream=side)
    assert gpu_ctx.planes_set_status(pset, stream=side) == [0] * 5
    pset.close()
    for k, (o, t) in enumerate(zip(outs, f.tensors)):
        assert torch.equal(o.view(torch.uint8), t.view(torch.uint8)), k
    assert torch.equal(first, f.buf) and torch.equal(second, f.buf)


# ---- refusals ----
def test_refusals_launch_nothing(gpu_ctx, packed):
    f, L, ctx = packed, gpu_ctx.L, gpu_ctx.handle
    K = 5
    arena = _full(f.total + PAD)
    shared = _full(2 * f.total + int(f.descs[0].frame_length) + 1024)
    before = [fr.clone() for fr in f.frames]
    ok = dict(descs=list(f.descs), frames=[fr.data_ptr() for fr in f.frames], fl=[fr.numel() for fr in f.frames], count=K, arena=arena.data_ptr(), cap=f.total)

    def with_(key, k, v):
        return {key: [v if j == k else x for j, x in enumerate(ok[key])]}

    overlapping = api.PlanesDesc.from_buffer_copy(f.descs[1])
    overlapping.offset[1] = overlapping.offset[0]
    inside = shared.data_ptr() + up16(f.total) + 256
    room = up16(int(f.descs[4].frame_length)) + 4096
    assert room - 16 + f.total <= shared.numel()
    bad = {
        "a misaligned source": with_("frames", 2, f.frames[2].data_ptr() + 8),
        "a misaligned arena": dict(arena=arena.data_ptr() + 8),
        "a capacity one byte short": dict(cap=f.total - 1),
        "an arena inside a frame": dict(with_("frames", 0, shared.data_ptr()), **with_("fl", 0, shared.numel()), arena=shared.data_ptr() + 512),
        "a frame inside the arena": dict(with_("frames", 0, inside), **with_("fl", 0, int(f.descs[0].frame_length)), arena=shared.data_ptr(), cap=shared.numel()),
        "a frame whose last 16 bytes are the arena's first": dict(with_("frames", 4, shared.data_ptr()), **with_("fl", 4, room), arena=shared.data_ptr() + room - 16),
        "a frame length one byte short": with_("fl", 3, int(f.descs[3].frame_length) - 1),
        "a descriptor with overlapping planes": with_("descs", 1, overlapping),
        "count 0": dict(count=0),
        "a NULL frame": with_("frames", 1, None), "a NULL arena": dict(arena=None),
    }
    zero = bytes((api.PlanesDesc * K)())
    for why, change in bad.items():
        k = dict(ok, **change)
        outs = (api.PlanesDesc * K)(*f.descs)  # (what a refusal must zero)
        bases = (ctypes.c_uint64 * (K + 1))()
        rc = L.hsrans_planes_pack_device(ctx, (api.PlanesDesc * K)(*k["descs"]), (ctypes.c_void_p * K)(*k["frames"]), (ctypes.c_size_t * K)(*k["fl"]), k["count"], k["arena"],
                                         k["cap"], None, outs, bases)
        assert rc == E_ARG, why
        assert k["count"] == 0 or bytes(outs) == zero, why
    # layer 1's own
    src = _full(4096 + PAD)
    one = dict(srcs=[src.data_ptr(), src.data_ptr() + 1024], lengths=[1000, 17], count=2, arena=arena.data_ptr(), cap=1008 + 32)
    bad1 = {
        "a misaligned source": dict(srcs=[src.data_ptr(), src.data_ptr() + 1028]), "a NULL source": dict(srcs=[None, src.data_ptr()]),
        "a misaligned arena": dict(arena=arena.data_ptr() + 4), "a capacity one byte short": dict(cap=1008 + 31), "a length of 0": dict(lengths=[1000, 0]),
        "the arena on a source": dict(arena=src.data_ptr() + 2048 - 1024, cap=2048), "the arena's last bytes on a source": dict(arena=src.data_ptr() + 2048, srcs=[src.data_ptr(), src.data_ptr() + 3072]),
        "count 0": dict(count=0), "a NULL arena": dict(arena=None),
    }
    for why, change in bad1.items():
        k = dict(one, **change)
        assert L.hsrans_pack_device(ctx, (ctypes.c_void_p * 2)(*k["srcs"]), (ctypes.c_size_t * 2)(*k["lengths"]), k["count"], k["arena"], k["cap"], None) == E_ARG, why
    assert L.hsrans_pack_device(ctx, None, (ctypes.c_size_t * 2)(1000, 17), 2, arena.data_ptr(), 2048, None) == E_ARG
    assert L.hsrans_pack_device(ctx, (ctypes.c_void_p * 2)(*one["srcs"]), None, 2, arena.data_ptr(), 2048, None) == E_ARG
    torch.cuda.synchronize()
    assert _untouched(arena) and _untouched(shared) and _untouched(src) and all(torch.equal(a, b) for a, b in zip(f.frames, before))
    # through the wrapper, which raises
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.planes_pack_device(f.descs, f.frames, arena[: f.total - 1])
    assert e.value.code == E_ARG
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.pack_device([src, src[1024:]], [1000, 17], arena[: 1008 + 31])
    assert e.value.code == E_ARG
    with pytest.raises(H.HsransError) as e:  # a length beyond its tensor never reaches the kernel
        gpu_ctx.pack_device([src[:1000], src[1024: 1024 + 16]], [1000, 17], arena[:2048])
    assert e.value.code == E_ARG
    with pytest.raises(TypeError):  # numel() must be bytes: an arena, a source or a frame of another dtype
        gpu_ctx.pack_device([src, src[1024:]], [1000, 17], arena[:2048].view(torch.int32))
    with pytest.raises(TypeError):
        gpu_ctx.pack_device([src[:1024].view(torch.int16), src[1024:]], [1000, 17], arena[:2048])
    with pytest.raises(TypeError):
        gpu_ctx.planes_pack_device(f.descs, [f.frames[0].view(torch.int16)] + f.frames[1:], arena[: f.total])
    torch.cuda.synchronize()
    assert _untouched(arena)
    # what was refused still packs
    descs, _ = gpu_ctx.planes_pack_device(f.descs, f.frames, arena[: f.total])
    assert [bytes(d) for d in descs] == [bytes(d) for d in f.want_descs] and torch.equal(arena, f.buf)
