"""hsrans_decode_device_planes_gather_batch: element ranges of many frames of byte planes, of 2-, 4- and 8-byte elements, in one call.  Every
expected value is a numpy slice of the ORIGINAL arrays; the output and the workspace are pre-filled with a sentinel and compared whole —
the output against the rows' elements and nothing else, the workspace against the layout the header promises (so no byte outside the coded
planes' sub-slots is written).  The frames and the sets are made once for the module."""
import ctypes
import random

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api, synth

pytestmark = pytest.mark.gpu

E_ARG = 2
SENTINEL = 0xA5
BLOCK = 1 << 16
N_BIG = 70_001    # two mt_ blocks of 64 KiB per plane; ends inside a 16-element block
N_SMALL = 20_003
NP_INT = {2: np.int16, 4: np.int32, 8: np.int64}
TORCH_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}


def _up(v, a):
    return (v + a - 1) // a * a


def _full(n):
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")


class Member:
    """one tensor, its frame and — for the single-call comparison — its own planes and gather objects"""

    def __init__(self, ctx, a, states=64, bits=11, interval=32, store=True):
        self.a, self.W, self.N = a, a.itemsize, a.size
        self.t = torch.from_numpy(np.ascontiguousarray(a).view(NP_INT[self.W])).cuda()
        self.frame = _full(H.planes_capacity(self.W, states, a.size))
        work = _full(H.planes_workspace_bytes(self.W, a.size))
        _, self.desc, self.plans = ctx.encode_device_planes(self.t, self.frame, work, states=states, bits=bits, block_size=BLOCK, index_interval=interval,
                                                            store_incompressible=store)
        self.coded = [p for p in range(self.W) if self.plans[p] is not None]
        self.rows = a.view(np.uint8).reshape(-1, self.W)  # rows[i, p] = plane p's byte of element i
        self._single = None
        self.ctx = ctx

    def single(self):
        if self._single is None:
            planes = self.ctx.make_planes(self.desc, self.plans)
            self._single = (planes, self.ctx.make_planes_gather(planes, self.frame))
        return self._single[1]

    def close(self):
        if self._single is not None:
            self._single[1].close()
            self._single[0].close()


class Set:
    def __init__(self, ctx, members):
        self.members = members
        self.pset = ctx.make_planes_set([m.desc for m in members], [m.plans for m in members])
        self.pgs = ctx.make_planes_gather_set(self.pset, [m.frame for m in members])
        self.itemsizes, self.elements = [m.W for m in members], [m.N for m in members]

    def close(self):
        self.pgs.close()
        self.pset.close()
        for m in self.members:
            m.close()


@pytest.fixture(scope="module")
def sets(gpu_ctx):
    rng = np.random.default_rng(29)
    x = rng.standard_normal(N_BIG).astype(np.float32)
    bf16, fp32 = (x.view(np.uint32) >> 16).astype(np.uint16), x.view(np.uint32)
    ramp = (np.arange(N_SMALL, dtype=np.uint64) << np.uint64(8)) | rng.integers(0, 256, N_SMALL, dtype=np.uint64)  # noise in the low byte
    main = Set(gpu_ctx, [
        Member(gpu_ctx, bf16, store=False),                 # 0: all planes coded
        Member(gpu_ctx, bf16),                              # 1: incompressible planes stored
        Member(gpu_ctx, fp32, states=32, bits=13),          # 2: another gather kind
        Member(gpu_ctx, fp32[:N_SMALL].copy(), interval=0),  # 3: no checkpoints
        Member(gpu_ctx, ramp),                              # 4: 8-byte elements
        Member(gpu_ctx, synth.uniform_bytes(2 * N_SMALL, seed=31).view(np.uint16)),  # 5: every plane stored
    ])
    stored = Set(gpu_ctx, [
        Member(gpu_ctx, synth.uniform_bytes(2 * N_SMALL, seed=33).view(np.uint16)),
        Member(gpu_ctx, synth.uniform_bytes(4 * 5_001, seed=35).view(np.uint32)),
        Member(gpu_ctx, synth.uniform_bytes(8 * 3_001, seed=37).view(np.uint64)),
    ])
    assert len(main.members[0].coded) == 2 and 0 < len(main.members[1].coded) < 2 and main.members[5].coded == []
    assert 0 < len(main.members[2].coded) < 4 and 0 < len(main.members[4].coded) < 8
    assert all(m.coded == [] for m in stored.members)
    yield {"main": main, "stored": stored}
    main.close()
    stored.close()


# ---- the row list: the SHAPES of tests/test_gpu_planes_gather.py scaled to a tensor of N elements: (offset, length, destination rule);
# "al": the destination's byte address is 16-aligned against the source's 16-element grid (dst_offset - offset a multiple of 16: whole blocks
# leave as 16-byte stores), "el": it is only element-aligned (dst_offset - offset odd) ----
def _shapes(N):
    half = N // 2 // 16 * 16
    return [
        (0, 1, "al"),                      # element 0
        (N - 1, 1, "el"),                  # the last element (of a tensor that ends inside a 16-element block)
        (16 * 50 + 1, 15, "al"),           # phase 1
        (16 * 70 + 15, 16, "el"),          # phase 15
        (4096, 17, "al"),                  # phase 0
        (5_001, 4095, "el"),               # phase 9
        (half - 1, 4097, "al"),            # phase 15, two tasks
        (123, 0, "el"),                    # empty
        (N - 10_001, 10_001, "el"),        # N_BIG: crosses the mt_ block boundary at 65,536; three tasks; ends with the tensor
        (half - 16, 300, "al"),            # overlaps the two-task row in the source
        (N - 70, 70, "al"),                # whole blocks, then a tail that ends with the tensor
        (32, 16, "el"), (48, 16, "al"),    # exactly one aligned block each
    ]


def _rows(s, members, first=0, flip=0):
    """the shapes dealt over `members` in interleaved order (no two adjacent rows of one member), the rule of every other member flipped;
    destinations packed in list order, in bytes, each moved up to the next element of its member that meets its rule.
    Returns (rows (member, offset, length, dst_offset), output bytes)."""
    out, at = [], first
    n_shapes = len(_shapes(N_BIG))
    for i in range(n_shapes):
        for j, m in enumerate(members):
            off, n, rule = _shapes(s.elements[m])[i]
            if (j + flip) % 2:
                rule = "el" if rule == "al" else "al"
            W = s.itemsizes[m]
            dst = -(-at // W)
            while (dst - off) % 16 != 0 if rule == "al" else (dst - off) % 2 != 1:
                dst += 1
            out.append((m, off, n, dst))
            at = (dst + n) * W
    return out, _up(at, 16)


def _expected_out(s, rows, out_bytes):
    want = np.full(out_bytes, SENTINEL, np.uint8)
    for m, off, n, dst in rows:
        W = s.itemsizes[m]
        want[dst * W: (dst + n) * W] = s.members[m].a.view(np.uint8)[off * W: (off + n) * W]
    return want


def _layout(s, rows):
    """[(C_r, slot_r, phase)] per row and the sum of W * slot: the header's workspace layout"""
    at, out = 0, []
    for m, off, n, _ in rows:
        slot = _up(off % 16 + n, 16) if n else 0
        out.append((at, slot, off % 16))
        at += s.itemsizes[m] * slot
    return out, at


def _expected_work(s, rows, work_bytes):
    want = np.full(work_bytes, SENTINEL, np.uint8)
    slots, total = _layout(s, rows)
    for (m, off, n, _), (c, slot, phase) in zip(rows, slots):
        for p in s.members[m].coded:
            want[c + p * slot + phase: c + p * slot + phase + n] = s.members[m].rows[off: off + n, p]
    return want, _up(total, 256)


def _gather(ctx, s, rows, out_bytes, stream=None):
    out = _full(out_bytes)
    work = _full(H.planes_gather_batch_workspace_bytes(max(s.itemsizes), len(rows), sum(r[2] for r in rows)) + 256)
    ctx.decode_device_planes_gather_batch(s.pgs, rows, out, work, stream=stream)
    return out, work


def _check(ctx, s, rows, out_bytes, out, work, stream=None):
    assert ctx.planes_gather_set_status(s.pgs, stream=stream) == [0] * len(s.members)
    assert np.array_equal(out.cpu().numpy(), _expected_out(s, rows, out_bytes))
    want_work, need = _expected_work(s, rows, work.numel())
    assert need <= work.numel() - 256
    assert np.array_equal(work.cpu().numpy(), want_work)


MAIN = [0, 1, 2, 4, 5]  # member 3 has no row at all in the main list
ALL = [5, 3, 0, 4, 2, 1]


def test_the_row_list_is_what_it_claims(sets):
    s = sets["main"]
    rows, _ = _rows(s, MAIN)
    assert {r[0] for r in rows} == set(MAIN) and all(a[0] != b[0] for a, b in zip(rows, rows[1:]))
    assert any(n == 0 for _, _, n, _ in rows)
    assert any(off < BLOCK < off + n for m, off, n, _ in rows if s.elements[m] == N_BIG), "a row crosses the mt_ block boundary"
    for W in (2, 4, 8):  # both store paths, for every element size
        mine = [(off, n, dst) for m, off, n, dst in rows if s.itemsizes[m] == W and n >= 32]
        assert any((dst - off) % 16 == 0 for off, n, dst in mine) and any((dst - off) % 2 == 1 for off, n, dst in mine)
    assert {off % 16 for _, off, n, _ in rows if n} >= {0, 1, 15}


def test_the_output_is_the_rows_elements_and_nothing_else(gpu_ctx, sets):
    s = sets["main"]
    rows, n_out = _rows(s, MAIN)
    out, work = _gather(gpu_ctx, s, rows, n_out + 48)
    _check(gpu_ctx, s, rows, n_out + 48, out, work)  # (the workspace too: the header's layout, and the sentinel everywhere else)


def test_it_is_the_single_calls_byte_for_byte(gpu_ctx, sets):
    s = sets["main"]
    rows, n_out = _rows(s, MAIN)
    out, _ = _gather(gpu_ctx, s, rows, n_out)
    single = _full(n_out)
    for m in MAIN:
        mine = [(off, n, dst) for k, off, n, dst in rows if k == m]
        W = s.itemsizes[m]
        work = _full(H.planes_gather_workspace_bytes(W, len(mine), sum(r[1] for r in mine)))
        gpu_ctx.decode_device_planes_gather(s.members[m].single(), mine, single.view(TORCH_INT[W]), work)
        assert gpu_ctx.planes_gather_status(s.members[m].single()) == [0] * W
    assert gpu_ctx.planes_gather_set_status(s.pgs) == [0] * 6
    assert torch.equal(out, single)
    # ... and a row's merge tasks are the single call's for it
    for m, off, n, dst in rows:
        got = H.planes_gather_batch_tasks([(m, off, n, dst)], s.itemsizes, s.elements)
        assert np.array_equal(got[:, [0, 1, 3, 4, 5]], H.planes_gather_tasks([(off, n, dst)], s.elements[m]))


def test_shuffled_rows_give_the_same_output(gpu_ctx, sets):
    s = sets["main"]
    rows, n_out = _rows(s, ALL)
    out, work = _gather(gpu_ctx, s, rows, n_out)
    _check(gpu_ctx, s, rows, n_out, out, work)
    shuffled = list(rows)
    random.Random(11).shuffle(shuffled)
    out2, work2 = _gather(gpu_ctx, s, shuffled, n_out)
    _check(gpu_ctx, s, shuffled, n_out, out2, work2)
    assert torch.equal(out, out2)


def test_the_launches_are_the_sets_plus_one_however_many_rows(gpu_ctx, sets):
    s = sets["main"]
    rows, n_out = _rows(s, ALL)
    out, work = _gather(gpu_ctx, s, rows, n_out)
    torch.cuda.synchronize()
    info = s.pgs.info()
    coded = [(m, p) for m, mem in enumerate(s.members) for p in mem.coded]
    planes = sum(s.itemsizes)
    assert (info["members"], info["coded"], info["stored"]) == (6, len(coded), planes - len(coded))
    assert info["rows"] == sum(len(s.members[m].coded) for m, _, n, _ in rows if n)
    assert info["merge_tasks"] == H.planes_gather_batch_tasks(rows, s.itemsizes, s.elements).shape[0]
    # the same gather rows through a gather set of the test's own over all coded planes: its launches + 1, and the same workspace bytes
    streams = [s.members[m].frame[s.members[m].desc.offset[p]: s.members[m].desc.offset[p] + s.members[m].desc.length[p]] for m, p in coded]
    gset = gpu_ctx.make_gather_set([s.members[m].plans[p] for m, p in coded], streams)
    slots, total = _layout(s, rows)
    grows = [(coded.index((m, p)), off, n, c + p * slot + phase) for (m, off, n, _), (c, slot, phase) in zip(rows, slots) if n for p in s.members[m].coded]
    work2 = _full(work.numel())
    gpu_ctx.decode_device_gather_batch(gset, grows, work2)
    assert gpu_ctx.gather_set_status(gset) == [0] * len(coded)
    assert info["launches"] == gset.info()["launches"] + 1 and 2 <= info["launches"] <= 7
    assert torch.equal(work, work2)
    gset.close()
    # ten times the rows, all members in use: not one launch more
    many, at = [], 0
    for rep in range(10):
        more, at = _rows(s, ALL, first=at, flip=rep)
        many += more
    out10, work10 = _gather(gpu_ctx, s, many, at)
    _check(gpu_ctx, s, many, at, out10, work10)
    info10 = s.pgs.info()
    assert info10["launches"] == info["launches"]
    assert info10["rows"] == 10 * info["rows"] and info10["merge_tasks"] == 10 * info["merge_tasks"]


def test_an_all_stored_set_makes_one_launch(gpu_ctx, sets):
    s = sets["stored"]
    shapes = [(0, 1), (15, 17), (1000, 2001), (3_001 - 40, 40), (77, 0), (16, 16)]
    rows, at = [], 0
    for i, (off, n) in enumerate(shapes):
        for m in (2, 0, 1):
            W = s.itemsizes[m]
            dst = -(-at // W) + (i + m) % 3
            rows.append((m, off, n, dst))
            at = (dst + n) * W
    at = _up(at, 16)
    out, work = _gather(gpu_ctx, s, rows, at + 16)
    _check(gpu_ctx, s, rows, at + 16, out, work)  # (status settles the stream and reports OK; the workspace is all sentinel)
    assert bool((work == SENTINEL).all())
    info = s.pgs.info()
    assert (info["members"], info["coded"], info["stored"]) == (3, 0, 14)
    assert (info["rows"], info["launches"]) == (0, 1)
    assert info["merge_tasks"] == H.planes_gather_batch_tasks(rows, s.itemsizes, s.elements).shape[0]


def test_whole_tensor_rows_are_the_whole_decode(gpu_ctx, sets):
    s = sets["main"]
    outs = [torch.zeros_like(m.t) for m in s.members]
    gpu_ctx.decode_device_planes_batch(s.pset, [m.frame for m in s.members], outs, _full(s.pset.info()["work_bytes"]))
    assert gpu_ctx.planes_set_status(s.pset) == [0] * 6
    rows, at = [], 0
    for m in ALL:
        dst = _up(at, 16) // s.itemsizes[m]
        rows.append((m, 0, s.elements[m], dst))
        at = (dst + s.elements[m]) * s.itemsizes[m]
    at = _up(at, 16)
    out, work = _gather(gpu_ctx, s, rows, at)
    _check(gpu_ctx, s, rows, at, out, work)
    for m, _, n, dst in rows:
        W = s.itemsizes[m]
        assert torch.equal(out[dst * W: (dst + n) * W], outs[m].view(torch.uint8)) and torch.equal(outs[m], s.members[m].t)


def test_two_calls_back_to_back_and_the_planes_set_still_decodes(gpu_ctx, sets):
    s = sets["main"]
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    r1, n1 = _rows(s, MAIN)
    r2, n2 = _rows(s, ALL[::-1], first=22, flip=1)
    with torch.cuda.stream(st):
        out1, work1 = _gather(gpu_ctx, s, r1, n1, stream=st)
        out2, work2 = _gather(gpu_ctx, s, r2, n2, stream=st)
        _check(gpu_ctx, s, r2, n2, out2, work2, stream=st)
        _check(gpu_ctx, s, r1, n1, out1, work1, stream=st)
    # the planes set the gather set borrows is as it was
    outs = [torch.zeros_like(m.t) for m in s.members]
    gpu_ctx.decode_device_planes_batch(s.pset, [m.frame for m in s.members], outs, _full(s.pset.info()["work_bytes"]))
    assert gpu_ctx.planes_set_status(s.pset) == [0] * 6
    assert all(torch.equal(o, m.t) for o, m in zip(outs, s.members))


def _call(ctx, pgs, rows, out, out_bytes, work, work_bytes, reserved=0, handle=None):
    arr = (api.MemberRange * max(len(rows), 1))()
    for k, (m, off, n, dst) in enumerate(rows):
        arr[k].member, arr[k].offset, arr[k].length, arr[k].dst_offset, arr[k].reserved = m, off, n, dst, reserved
    return ctx.L.hsrans_decode_device_planes_gather_batch(handle if handle is not None else ctx.handle, pgs.handle, arr if rows else None, len(rows), out, out_bytes,
                                                          work, work_bytes, None)


def test_empty_calls_write_nothing_and_launch_nothing(gpu_ctx, sets):
    s = sets["main"]
    out, work = _full(4096), _full(4096)
    assert _call(gpu_ctx, s.pgs, [], out.data_ptr(), 4096, work.data_ptr(), 4096) == 0
    info = s.pgs.info()
    assert (info["rows"], info["merge_tasks"], info["launches"]) == (0, 0, 0)
    assert _call(gpu_ctx, s.pgs, [(0, 5, 0, 0), (4, N_SMALL, 0, 512), (5, 0, 0, 7)], out.data_ptr(), 4096, work.data_ptr(), 4096) == 0
    gpu_ctx.decode_device_planes_gather_batch(s.pgs, [], out, work)
    assert gpu_ctx.planes_gather_set_status(s.pgs) == [0] * 6
    assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all())
    info = s.pgs.info()
    assert (info["rows"], info["merge_tasks"], info["launches"]) == (0, 0, 0)


def test_the_call_refuses_bad_arguments_and_writes_nothing(gpu_ctx, sets):
    s = sets["main"]
    rows = [(0, 100, 5000, 0), (4, 7, 0, 3), (4, N_SMALL - 9, 9, 1300), (2, 31, 40, 2700)]
    need = _up(_layout(s, rows)[1], 256)
    n_out = 2740 * 4
    out, work = _full(n_out + 32), _full(need + 32)
    joined = _full(n_out + need + 64)
    o, w = out.data_ptr(), work.data_ptr()
    frame = s.members[2].frame
    before = frame.clone()
    # an object of another context, over a set of that context
    other = H.Context(0)
    o_member = Member(other, s.members[4].a[:5_000].copy())
    o_set = Set(other, [o_member])

    def call(rows=rows, d_out=o, oc=n_out, d_work=w, wb=need, **kw):
        pgs = kw.pop("pgs", s.pgs)
        return _call(gpu_ctx, pgs, rows, d_out, oc, d_work, wb, **kw)

    # the same row passes for the 2-byte member and fails for the 8-byte one: its destination ends one element beyond out_capacity
    cap8 = (100 + 16) * 8
    refused = [
        call(rows=[(6, 0, 1, 0)]), call(rows=rows + [(6, 0, 0, 0)]),                     # member = members
        call(reserved=1),
        call(rows=[(1, N_BIG - 4, 5, 0)]), call(rows=[(3, N_SMALL, 1, 0)]),              # one element beyond its member
        call(rows=[(4, N_SMALL + 1, 0, 0)]), call(rows=[(0, 2**64 - 2, 4, 0)]),
        call(rows=[(4, 0, 16, 100)], oc=cap8 - 8),                                       # one 8-byte element beyond out_capacity
        call(rows=[(0, 0, 16, 2**64 - 8)]), call(rows=[(4, 0, 16, 1 << 62)]),            # dst_offset + length, and its bytes, overflow
        call(wb=need - 1), call(wb=0),                                                   # one byte below this call's need
        call(d_out=o + 8), call(d_work=w + 4), call(d_out=None), call(d_work=None),      # alignment and null pointers
        call(d_out=frame.data_ptr() + 256),                                              # the output lies inside a frame
        call(d_work=s.members[5].frame.data_ptr()),                                      # the workspace lies on a frame
        call(d_out=joined.data_ptr(), d_work=joined.data_ptr() + n_out - 16),            # the workspace begins inside the output
        call(pgs=o_set.pgs), call(handle=other.handle),                                  # an object of another context
        gpu_ctx.L.hsrans_decode_device_planes_gather_batch(gpu_ctx.handle, s.pgs.handle, None, 3, o, n_out, w, need, None),
        gpu_ctx.L.hsrans_decode_device_planes_gather_batch(gpu_ctx.handle, None, None, 0, o, n_out, w, need, None),
    ]
    assert refused == [E_ARG] * len(refused), refused
    torch.cuda.synchronize()
    for t in (out, work, joined):
        assert bool((t == SENTINEL).all())
    assert torch.equal(frame, before)
    # ... and through the wrapper: an output that ends 16 bytes early, a workspace that is not bytes
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.decode_device_planes_gather_batch(s.pgs, rows, out[: n_out - 16], work)
    assert e.value.code == E_ARG
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_planes_gather_batch(s.pgs, rows, out[:n_out], work.view(torch.int32))
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all())
    # what was refused by one element or one byte passes without it
    assert call(rows=[(4, 0, 16, 100)], oc=cap8) == 0
    assert call(rows=[(0, 0, 16, 100)], oc=cap8 - 8) == 0
    assert call() == 0
    assert gpu_ctx.planes_gather_set_status(s.pgs) == [0] * 6
    want = _expected_out(s, [(0, 0, 16, 100), (4, 0, 16, 100)] + rows, out.numel())
    # (rows' first member-0 row overwrites bytes 0 .. 10,000 last, as the calls ran)
    assert np.array_equal(out.cpu().numpy(), want)
    o_set.close()


def test_create_refuses_bad_frames(gpu_ctx, sets):
    s = sets["main"]
    frames = [m.frame for m in s.members]
    lengths = [int(m.desc.frame_length) for m in s.members]
    gpu_ctx.make_planes_gather_set(s.pset, frames, lengths).close()  # exactly the descriptors' lengths will do
    short = list(lengths)
    short[3] -= 1
    room = _full(frames[1].numel() + 32)
    at = (8 - room.data_ptr()) % 16
    moved = list(frames)
    moved[1] = room[at: at + frames[1].numel()].copy_(frames[1])  # the same frame, 8 bytes off the 16-byte grid
    assert moved[1].data_ptr() % 16 == 8
    for fr, ln in [(frames, short), (moved, None), (frames[:5], None), (frames + [frames[0]], None)]:
        with pytest.raises(H.HsransError) as e:
            gpu_ctx.make_planes_gather_set(s.pset, fr, ln)
        assert e.value.code == E_ARG
    # ... and the C entry its null arguments and a set of another context
    L, h = gpu_ctx.L, ctypes.c_void_p()
    fp, fl = api._tensor_arrays(frames)
    other = H.Context(0)
    assert L.hsrans_planes_gather_set_create(None, s.pset.handle, fp, fl, ctypes.byref(h)) == E_ARG
    assert L.hsrans_planes_gather_set_create(gpu_ctx.handle, None, fp, fl, ctypes.byref(h)) == E_ARG
    assert L.hsrans_planes_gather_set_create(gpu_ctx.handle, s.pset.handle, None, fl, ctypes.byref(h)) == E_ARG
    assert L.hsrans_planes_gather_set_create(gpu_ctx.handle, s.pset.handle, fp, None, ctypes.byref(h)) == E_ARG
    assert L.hsrans_planes_gather_set_create(gpu_ctx.handle, s.pset.handle, fp, fl, None) == E_ARG
    assert L.hsrans_planes_gather_set_create(other.handle, s.pset.handle, fp, fl, ctypes.byref(h)) == E_ARG
    assert not h.value
