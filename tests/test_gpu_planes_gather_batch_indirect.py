"""hsrans_decode_device_planes_gather_batch_indirect: element ranges of many frames of byte planes, the rows in DEVICE memory.  Tensors, frames,
sets, row list and sentinel method are tests/test_gpu_planes_gather_batch.py's: every expected value is a numpy slice of the ORIGINAL arrays;
the output and the data workspace are pre-filled with a sentinel and compared whole — the output against the rows' elements and nothing else,
the workspace against the host call's row-major layout.  The control workspace is never inspected."""
import ctypes

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api
from test_gpu_planes_gather_batch import (ALL, MAIN, N_BIG, N_SMALL, SENTINEL, Member, Set, _expected_out, _expected_work, _full, _layout, _rows, _shapes,  # noqa: F401
                                          _up, sets)

pytestmark = pytest.mark.gpu

E_ARG, E_DEVICE = 2, 5
GARBAGE = 0xDEADBEEFDEADBEEF  # rows that are never read: far outside every tensor, a member no set has, reserved bits set
ROUND = 2048                  # rows of one round of the cut at its two rows a thread; the tests hold for any batch factor up to 2


def _dev_rows(rows, n=None, reserved=None):
    """(rows, 4) int64 on the device in hsrans_member_range's layout: `rows` ((member, offset, length, dst_offset)), then garbage up to `n`;
    reserved: {row: its reserved word}, 0 elsewhere"""
    arr = np.full((max(n or 0, len(rows)), 4), GARBAGE, np.uint64)
    for k, (m, off, length, dst) in enumerate(rows):
        arr[k] = np.asarray([off, length, dst, m | ((reserved or {}).get(k, 0) << 32)], np.uint64)
    return torch.from_numpy(arr.view(np.int64)).cuda()


def _count(n):
    return torch.from_numpy(np.asarray([n], np.uint32).view(np.int32)).cuda()


def _coded(s):
    return sum(len(m.coded) for m in s.members)


class Call:
    """one indirect call's buffers: out and d_work full of the sentinel (d_work 256 bytes longer than any rows can need), a control workspace"""

    def __init__(self, s, out_bytes, max_count, total_elements, work_bytes=None):
        self.s, self.max_count = s, max_count
        self.out = _full(out_bytes)
        self.work = _full(H.planes_gather_batch_workspace_bytes(max(s.itemsizes), max_count, total_elements) + 256 if work_bytes is None else work_bytes)
        self.ws = torch.empty(H.planes_gather_batch_indirect_workspace_bytes(_coded(s), max(s.itemsizes), max_count), dtype=torch.uint8, device="cuda")
        assert self.ws.numel() > 0

    def run(self, ctx, d_rows, count=None, stream=None):
        got = ctx.decode_device_planes_gather_batch_indirect(self.s.pgs, d_rows, self.out, self.work, count=count, max_count=self.max_count, workspace=self.ws, stream=stream)
        assert got is self.ws

    def check(self, rows):
        """out and d_work whole: `rows` gathered, every other byte the sentinel ([]: nothing written)"""
        assert np.array_equal(self.out.cpu().numpy(), _expected_out(self.s, rows, self.out.numel()))
        want, need = _expected_work(self.s, rows, self.work.numel())
        assert need <= self.work.numel()
        assert np.array_equal(self.work.cpu().numpy(), want)

    def untouched(self):
        return bool((self.out == SENTINEL).all()) and bool((self.work == SENTINEL).all())

    def refill(self):
        self.out.fill_(SENTINEL)
        self.work.fill_(SENTINEL)


def _clean(ctx, s, stream=None):
    assert ctx.planes_gather_set_refused(s.pgs, stream=stream) == 0
    assert ctx.planes_gather_set_status(s.pgs, stream=stream) == [0] * len(s.members)


def _host(ctx, s, rows, like):
    """the host-rows call into buffers the size of `like`'s"""
    out, work = _full(like.out.numel()), _full(like.work.numel())
    ctx.decode_device_planes_gather_batch(s.pgs, rows, out, work)
    return out, work


def _total(rows):
    return sum(r[2] for r in rows)


@pytest.fixture(scope="module")
def many(sets):
    """about 4,500 rows over all members of the main set — lengths 0..40, six rows of 5,000 elements (two tasks each) — with packed destinations,
    16-byte aligned against the source's grid in even rows and only element-aligned in odd ones; made once, never changed"""
    s = sets["main"]
    rng = np.random.default_rng(53)
    rows, at = [], 0
    for k in range(4_500):
        m = int(rng.integers(0, len(s.members)))
        n = 5_000 if k % 750 == 300 else int(rng.integers(0, 41))
        off = int(rng.integers(0, s.elements[m] - n + 1))
        W = s.itemsizes[m]
        dst = -(-at // W)
        while (dst - off) % 16 != 0 if k % 2 == 0 else (dst - off) % 2 != 1:
            dst += 1
        rows.append((m, off, n, dst))
        at = (dst + n) * W
    return rows, _up(at, 16)


@pytest.mark.parametrize("order", ["sizes up", "sizes down"])
def test_the_row_list_on_the_main_set(gpu_ctx, sets, order):
    s = sets["main"]
    members = MAIN if order == "sizes up" else MAIN[::-1]  # element sizes 2 2 4 8 2, and 2 8 4 2 2
    rows, n_out = _rows(s, members)
    c = Call(s, n_out + 48, len(rows), _total(rows))
    c.run(gpu_ctx, _dev_rows(rows))
    _clean(gpu_ctx, s)
    c.check(rows)
    host_out, host_work = _host(gpu_ctx, s, rows, c)
    assert gpu_ctx.planes_gather_set_status(s.pgs) == [0] * 6
    assert torch.equal(c.out, host_out) and torch.equal(c.work, host_work)
    # what the call launches: the planes cut, the set's cut and its launches, the merge
    info = s.pgs.indirect_info(len(rows), c.out.numel(), c.work.numel())
    coded = [(m, p) for m, mem in enumerate(s.members) for p in mem.coded]
    assert (info["members"], info["coded"], info["stored"]) == (6, len(coded), sum(s.itemsizes) - len(coded))
    assert info["max_rows"] == len(rows) * 8
    assert 1 <= info["merge_grid"] <= len(rows) + c.work.numel() // (2 * 4096)
    streams = [s.members[m].frame[s.members[m].desc.offset[p]: s.members[m].desc.offset[p] + s.members[m].desc.length[p]] for m, p in coded]
    gset = gpu_ctx.make_gather_set([s.members[m].plans[p] for m, p in coded], streams)
    set_info = gset.indirect_info(info["max_rows"], c.work.numel())
    gset.close()
    assert info["set_launches"] == set_info["launches"] + 1 and info["launches"] == info["set_launches"] + 2


def test_an_all_stored_set_makes_two_kernels_and_leaves_the_workspace(gpu_ctx, sets):
    s = sets["stored"]
    shapes = [(0, 1), (15, 17), (1000, 2001), (3_001 - 40, 40), (77, 0), (16, 16)]
    rows, at = [], 0
    for i, (off, n) in enumerate(shapes):
        for m in (2, 0, 1):
            W = s.itemsizes[m]
            dst = -(-at // W) + (i + m) % 3
            rows.append((m, off, n, dst))
            at = (dst + n) * W
    c = Call(s, _up(at, 16) + 16, len(rows), _total(rows))
    c.run(gpu_ctx, _dev_rows(rows))
    _clean(gpu_ctx, s)
    c.check(rows)
    assert bool((c.work == SENTINEL).all())
    info = s.pgs.indirect_info(len(rows), c.out.numel(), c.work.numel())
    assert (info["members"], info["coded"], info["stored"]) == (3, 0, 14)
    assert (info["max_rows"], info["set_launches"], info["launches"]) == (0, 0, 2)
    assert H.planes_gather_batch_indirect_workspace_bytes(0, 8, len(rows)) == c.ws.numel() < H.planes_gather_batch_indirect_workspace_bytes(1, 8, len(rows))


def test_a_count_below_max_count_reads_no_row_beyond_it(gpu_ctx, sets):
    s = sets["main"]
    rows, n_out = _rows(s, ALL)
    c = Call(s, n_out, len(rows) + 9, _total(rows))
    for n in (7, len(rows), 1, 0):
        c.refill()
        c.run(gpu_ctx, _dev_rows(rows[:n], n=len(rows) + 9), count=_count(n))
        _clean(gpu_ctx, s)
        c.check(rows[:n])
    # only empty rows, at and inside their members' ends: nothing is written
    empty = [(0, 5, 0, 0), (4, N_SMALL, 0, 512), (5, 0, 0, 7), (2, N_BIG, 0, n_out // 4)]
    c.refill()
    c.run(gpu_ctx, _dev_rows(empty, n=len(rows) + 9), count=_count(len(empty)))
    _clean(gpu_ctx, s)
    c.check([])
    assert c.untouched()


def test_more_rows_than_two_rounds_of_the_cut(gpu_ctx, sets, many):
    s = sets["main"]
    rows, n_out = many
    assert len(rows) > 2 * ROUND and {r[0] for r in rows} == set(range(6))
    assert sum(1 for r in rows if r[2] == 0) > 50 and sum(1 for r in rows if r[2] == 5_000) == 6
    tasks = H.planes_gather_batch_tasks(rows, s.itemsizes, s.elements)
    assert tasks.shape[0] == sum(1 for r in rows if r[2]) + 6  # the long rows give two tasks each
    c = Call(s, n_out, len(rows), _total(rows))
    c.run(gpu_ctx, _dev_rows(rows))
    _clean(gpu_ctx, s)
    c.check(rows)
    host_out, host_work = _host(gpu_ctx, s, rows, c)
    assert torch.equal(c.out, host_out) and torch.equal(c.work, host_work)


GOOD = [(0, 100, 5000, 0), (4, 7, 0, 3), (4, N_SMALL - 9, 9, 1300), (2, 31, 40, 2700)]
GOOD_OUT = 2740 * 4  # bytes


def test_what_only_the_device_can_see_is_refused_there(gpu_ctx, sets, many):
    s = sets["main"]
    long_rows, long_out = many
    long_rows = long_rows[: ROUND + 400]
    big = 1 << 62
    # name: (the offending row, reserved)
    bad_rows = {
        "member = members": ((6, 0, 1, 0), 0),
        "an empty row of a member the set has not": ((6, 0, 0, 0), 0),
        "member 2^32 - 1": ((0xFFFFFFFF, 0, 1, 0), 0),
        "reserved != 0": ((0, 0, 1, 0), 1),
        "reserved != 0 on an empty row": ((0, 0, 0, 0), 0x80000000),
        "beyond its member": ((1, N_BIG - 4, 5, 0), 0),
        "beyond a member of another size": ((3, N_SMALL, 1, 0), 0),
        "an empty row beyond its member": ((4, N_SMALL + 1, 0, 0), 0),
        "offset + length wraps": ((0, 2**64 - 2, 4, 0), 0),
        "one 8-byte element beyond the output": ((4, 0, 16, GOOD_OUT // 8 - 15), 0),
        "dst_offset + length wraps": ((0, 0, 16, 2**64 - 8), 0),
        "(dst_offset + length) * elem_size wraps": ((4, 0, 16, big), 0),
    }
    places = ["first", "last", "a later round"]
    hit = set()
    for k, (name, (bad, reserved)) in enumerate(bad_rows.items()):
        place = places[k % 3]
        hit.add(place)
        if place == "a later round":  # behind more good rows than one round of the cut takes
            rows, at, out_bytes = long_rows, ROUND + 300, long_out
        else:
            rows, at, out_bytes = GOOD, 0 if place == "first" else len(GOOD), GOOD_OUT
        if name == "one 8-byte element beyond the output":
            bad = (4, 0, 16, out_bytes // 8 - 15)
        listed = rows[:at] + [bad] + rows[at:]
        c = Call(s, out_bytes, len(listed), _total(rows) + 16)
        c.run(gpu_ctx, _dev_rows(listed, reserved={at: reserved}))
        assert gpu_ctx.planes_gather_set_refused(s.pgs) == E_DEVICE, name
        assert gpu_ctx.planes_gather_set_refused(s.pgs) == 0, name  # once
        assert gpu_ctx.planes_gather_set_status(s.pgs) == [0] * 6, name
        assert c.untouched(), name
        # a good call on the same workspaces is bit-exact
        c.run(gpu_ctx, _dev_rows(GOOD, n=len(listed)), count=_count(len(GOOD)))
        _clean(gpu_ctx, s)
        c.check(GOOD)
    assert hit == set(places)
    # the count word, and a data workspace one 256-byte step too small for these rows
    need = _up(_layout(s, GOOD)[1], 256)
    assert need > 256
    for name, count, work_bytes in (("a count above max_count", len(GOOD) + 1, None), ("a count of 2^32 - 1", 0xFFFFFFFF, None), ("the rows do not fit d_work", len(GOOD), need - 256)):
        c = Call(s, GOOD_OUT, len(GOOD), _total(GOOD), work_bytes=work_bytes)
        c.run(gpu_ctx, _dev_rows(GOOD), count=_count(count))
        assert gpu_ctx.planes_gather_set_refused(s.pgs) == E_DEVICE, name
        assert gpu_ctx.planes_gather_set_refused(s.pgs) == 0, name
        assert gpu_ctx.planes_gather_set_status(s.pgs) == [0] * 6, name
        assert c.untouched(), name
    # ... and exactly enough of it passes, as does the 2-byte row whose 8-byte twin ended beyond the output
    c = Call(s, GOOD_OUT, len(GOOD), _total(GOOD), work_bytes=need)
    c.run(gpu_ctx, _dev_rows(GOOD))
    _clean(gpu_ctx, s)
    c.check(GOOD)
    c = Call(s, GOOD_OUT, 1, 16)
    c.run(gpu_ctx, _dev_rows([(0, 0, 16, GOOD_OUT // 8 - 15)]))
    _clean(gpu_ctx, s)
    c.check([(0, 0, 16, GOOD_OUT // 8 - 15)])


def test_graph_replays_read_the_rows_anew(gpu_ctx, sets):
    """one captured call; before every replay the rows and the count are overwritten in place.  Nothing of a replay may leak into the next: not
    its prefix, not its refusal."""
    s = sets["main"]
    a, n_a = _rows(s, MAIN)
    b, n_b = _rows(s, [3, 5, 4], first=22, flip=1)
    ROWS = max(len(a), len(b)) + 5
    total, n_out = max(_total(a), _total(b)), max(n_a, n_b) + 64
    c, direct = Call(s, n_out, ROWS, total), Call(s, n_out, ROWS, total)
    d_rows, d_count = _dev_rows([], n=ROWS), _count(ROWS)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            c.run(gpu_ctx, d_rows, count=d_count, stream=side)
    torch.cuda.synchronize()
    assert c.untouched()  # capturing runs nothing
    replays = (("rows A", a, 0), ("rows B: another count, other members", b, 0), ("a refused row among A", a[:9] + [(1, N_BIG, 1, 0)] + a[9:20], E_DEVICE),
               ("rows A again", a, 0), ("count 0", [], 0))
    for name, rows, expect in replays:
        d_rows.copy_(_dev_rows(rows, n=ROWS))
        d_count.copy_(_count(len(rows)))
        c.refill()
        g.replay()
        torch.cuda.synchronize()
        assert gpu_ctx.planes_gather_set_refused(s.pgs) == expect, name
        assert gpu_ctx.planes_gather_set_refused(s.pgs) == 0, name  # reported once
        assert gpu_ctx.planes_gather_set_status(s.pgs) == [0] * 6
        if expect:
            assert c.untouched(), name
            continue
        c.check(rows)
        direct.refill()
        direct.run(gpu_ctx, _dev_rows(rows, n=ROWS), count=_count(len(rows)))
        _clean(gpu_ctx, s)
        assert torch.equal(c.out, direct.out) and torch.equal(c.work, direct.work), name


def test_two_calls_in_flight_on_two_streams(gpu_ctx, sets):
    s = sets["main"]
    r1, n1 = _rows(s, MAIN)
    r2, n2 = _rows(s, ALL[::-1], first=22, flip=1)
    c1, c2 = Call(s, n1, len(r1), _total(r1)), Call(s, n2, len(r2) + 3, _total(r2) + 100)
    d1, d2, k2 = _dev_rows(r1), _dev_rows(r2, n=len(r2) + 3), _count(len(r2))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        c1.run(gpu_ctx, d1, stream=s1)
    with torch.cuda.stream(s2):
        c2.run(gpu_ctx, d2, count=k2, stream=s2)
    s1.synchronize()
    s2.synchronize()
    _clean(gpu_ctx, s)
    c1.check(r1)
    c2.check(r2)
    # the objects are as they were: the host-rows call still gives the same bytes
    host_out, host_work = _host(gpu_ctx, s, r1, c1)
    assert gpu_ctx.planes_gather_set_status(s.pgs) == [0] * 6
    assert torch.equal(host_out, c1.out) and torch.equal(host_work, c1.work)


def test_the_call_refuses_bad_arguments_on_the_host(gpu_ctx, sets):
    s = sets["main"]
    L, ctx = gpu_ctx.L, gpu_ctx.handle
    other = H.Context(0)
    MAXC = len(GOOD) + 1
    need_work = H.planes_gather_batch_workspace_bytes(8, MAXC, _total(GOOD))
    need_ws = H.planes_gather_batch_indirect_workspace_bytes(_coded(s), 8, MAXC)
    out, work, ws = _full(GOOD_OUT + 32), _full(need_work + 32), _full(need_ws + 512)
    joined = _full(GOOD_OUT + need_work + need_ws + 1024)
    d_rows, d_count = _dev_rows(GOOD, n=MAXC + 1), torch.from_numpy(np.asarray([len(GOOD), 0], np.int32)).cuda()
    # an object of another context, over a set of that context
    o_set = Set(other, [Member(other, s.members[4].a[:5_000].copy())])
    frame = s.members[2].frame

    ok = dict(ctx=ctx, pgs=s.pgs.handle, d_rows=d_rows.data_ptr(), d_count=d_count.data_ptr(), max_count=MAXC, d_out=out.data_ptr(), oc=GOOD_OUT, d_work=work.data_ptr(),
              wb=need_work, d_ws=ws.data_ptr(), wsb=need_ws)
    assert ok["d_ws"] % 256 == 0 and ok["d_rows"] % 8 == 0
    jp = joined.data_ptr()
    j_work = jp + _up(GOOD_OUT, 256)
    j_ws = j_work + _up(need_work, 256)
    bad = [
        dict(ctx=None), dict(pgs=None), dict(d_rows=None), dict(d_out=None), dict(d_work=None), dict(d_ws=None),
        dict(pgs=o_set.pgs.handle), dict(ctx=other.handle),                              # an object of another context
        dict(d_out=out.data_ptr() + 8), dict(d_work=work.data_ptr() + 4),                 # alignment
        dict(d_rows=d_rows.data_ptr() + 4), dict(d_count=d_count.data_ptr() + 2), dict(d_ws=ws.data_ptr() + 128),
        dict(wsb=need_ws - 1), dict(wsb=0),                                               # below the size function
        dict(max_count=(1 << 31) // 8),                                                   # ... which returns 0
        dict(d_out=frame.data_ptr() + 256), dict(d_work=s.members[5].frame.data_ptr()), dict(d_ws=s.members[0].frame.data_ptr()),  # on a frame
        dict(d_out=jp, d_work=jp + (GOOD_OUT & ~15) - 16),                                # the data workspace begins inside the output
        dict(d_out=jp, d_work=j_work, d_ws=j_work + (need_work & ~255) - 256),           # the control workspace begins inside the data workspace
        dict(d_out=jp, d_ws=jp + 256),                                                    # ... inside the output
        dict(d_rows=jp + 64, d_out=jp),                                                   # the rows lie in the output
        dict(d_count=j_work + 16, d_work=j_work),                                         # the count lies in the data workspace
        dict(d_rows=j_ws + 8, d_ws=j_ws), dict(d_count=j_ws + need_ws - 4, d_ws=j_ws),    # ... in the control workspace
    ]

    def call(k):
        return L.hsrans_decode_device_planes_gather_batch_indirect(k["ctx"], k["pgs"], k["d_rows"], k["d_count"], k["max_count"], k["d_out"], k["oc"], k["d_work"], k["wb"],
                                                                   k["d_ws"], k["wsb"], None)

    before = frame.clone()
    for change in bad:
        assert call(dict(ok, **change)) == E_ARG, change
    assert call(dict(ok, max_count=0)) == 0  # nothing to do, nothing queued
    torch.cuda.synchronize()
    for t in (out, work, joined):
        assert bool((t == SENTINEL).all())
    assert torch.equal(frame, before)
    _clean(gpu_ctx, s)
    info = api.PlanesGatherSetIndirectInfo()
    assert L.hsrans_planes_gather_set_indirect_info(s.pgs.handle, (1 << 31) // 8, GOOD_OUT, need_work, ctypes.byref(info)) == E_ARG
    # the wrapper's own refusals
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_planes_gather_batch_indirect(s.pgs, d_rows, out, work.view(torch.int32))
    with pytest.raises(TypeError):
        gpu_ctx.decode_device_planes_gather_batch_indirect(s.pgs, d_rows.view(-1), out, work)
    with pytest.raises(TypeError):
        gpu_ctx.decode_device_planes_gather_batch_indirect(s.pgs, d_rows[:, :3].contiguous(), out, work)
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.decode_device_planes_gather_batch_indirect(s.pgs, d_rows, out, work, max_count=MAXC, workspace=ws[:1024])
    assert e.value.code == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all())
    # what was refused still gathers, with the very arguments of `ok`
    assert call(ok) == 0
    _clean(gpu_ctx, s)
    assert np.array_equal(out.cpu().numpy(), _expected_out(s, GOOD, out.numel()))
    assert np.array_equal(work.cpu().numpy(), _expected_work(s, GOOD, work.numel())[0])
    o_set.close()
