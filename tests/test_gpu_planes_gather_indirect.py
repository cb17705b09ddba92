"""hsrans_decode_device_planes_gather_indirect: element ranges of a frame of byte planes, the ranges in DEVICE memory.  Tensors, frames, range
list and sentinel method are tests/test_gpu_planes_gather.py's: every expected value is a numpy slice of the ORIGINAL array; the output and
the data workspace are pre-filled with a sentinel and compared whole — the output against the ranges' elements and nothing else, the
workspace against the layout the header promises at the host-known stride up256(max_elements + 30 max_count).  The control workspace is
never inspected."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from test_gpu_planes_gather import FRAMES, N, SENTINEL, SHAPES, TORCH_INT, _expected_out, _full, _gather, _layout, _ranges, _up, frames, inputs  # noqa: F401

pytestmark = pytest.mark.gpu

E_ARG, E_DEVICE = 2, 5
GARBAGE = 0xDEADBEEFDEADBEEF  # rows that are never read: far outside every tensor


def _rows(ranges, rows=None):
    """(rows, 3) int64 on the device: `ranges`, then garbage up to `rows`"""
    arr = np.full((max(rows or 0, len(ranges)), 3), GARBAGE, np.uint64)
    if len(ranges):
        arr[: len(ranges)] = np.asarray(ranges, np.uint64).reshape(-1, 3)
    return torch.from_numpy(arr.view(np.int64)).cuda()


def _count(n):
    return torch.from_numpy(np.asarray([n], np.uint32).view(np.int32)).cuda()


def _stride(max_count, max_elements):
    return _up(max_elements + 30 * max_count, 256)


def _expected_work(f, ranges, work_bytes, stride):
    want = np.full(work_bytes, SENTINEL, np.uint8)
    slots, total = _layout(ranges)
    assert total <= stride
    for p in f.coded:
        for (off, n, _), (b, phase) in zip(ranges, slots):
            want[p * stride + b + phase: p * stride + b + phase + n] = f.rows[off: off + n, p]
    return want


class Call:
    """one indirect call's buffers: out and d_work full of the sentinel (d_work 256 bytes longer than it must be), a control workspace"""

    def __init__(self, f, out_elements, max_count, max_elements):
        self.f, self.max_count, self.max_elements = f, max_count, max_elements
        self.out = _full(out_elements * f.W)
        self.need_work = H.planes_gather_workspace_bytes(f.W, max_count, max_elements)
        assert self.need_work == f.W * _stride(max_count, max_elements)
        self.work = _full(self.need_work + 256)
        self.ws = torch.empty(H.planes_gather_indirect_workspace_bytes(f.W, max_count), dtype=torch.uint8, device="cuda")

    def run(self, ctx, d_ranges, count=None, stream=None, pg=None):
        got = ctx.decode_device_planes_gather_indirect(pg or self.f.pg, d_ranges, self.out.view(TORCH_INT[self.f.W]), self.work[: self.need_work], count=count,
                                                       max_count=self.max_count, max_elements=self.max_elements, workspace=self.ws, stream=stream)
        assert got is self.ws

    def check(self, ranges):
        """out and d_work whole: `ranges` gathered, every other byte the sentinel ([]: nothing written)"""
        out_elements = self.out.numel() // self.f.W
        assert np.array_equal(self.out.cpu().numpy(), _expected_out(self.f, ranges, out_elements))
        assert np.array_equal(self.work.cpu().numpy(), _expected_work(self.f, ranges, self.work.numel(), _stride(self.max_count, self.max_elements)))

    def refill(self):
        self.out.fill_(SENTINEL)
        self.work.fill_(SENTINEL)


def _clean(ctx, f, stream=None):
    assert ctx.planes_gather_refused(f.pg, stream=stream) == 0
    assert ctx.planes_gather_status(f.pg, stream=stream) == [0] * f.W


@pytest.mark.parametrize("key", sorted(FRAMES))
def test_the_range_list_on_every_frame(gpu_ctx, frames, key):
    f = frames(key)
    ranges, n_out = _ranges()
    total = sum(n for _, n, _ in ranges)
    c = Call(f, n_out + 5, len(ranges), total)
    c.run(gpu_ctx, _rows(ranges))
    _clean(gpu_ctx, f)
    c.check(ranges)
    host_out, _ = _gather(gpu_ctx, f, ranges, n_out + 5)
    assert torch.equal(c.out, host_out)
    info = f.pg.indirect_info(len(ranges), total, c.out.numel())
    assert info["coded"] == len(f.coded) and info["stored"] == f.W - len(f.coded) and info["max_rows"] == len(ranges) * len(f.coded)
    assert 1 <= info["merge_grid"] <= len(ranges) + _stride(len(ranges), total) // 4096
    if key == "uniform":
        assert f.coded == [] and info["set_launches"] == 0 and info["launches"] == 2
    else:
        streams = [f.frame[f.desc.offset[p]: f.desc.offset[p] + f.desc.length[p]] for p in f.coded]
        gset = gpu_ctx.make_gather_set([f.plans[p] for p in f.coded], streams)
        set_info = gset.indirect_info(len(ranges) * len(f.coded), f.W * _stride(len(ranges), total))
        gset.close()
        assert info["set_launches"] == set_info["launches"] + 1 and info["launches"] == info["set_launches"] + 2


@pytest.mark.parametrize("key", ["bf16-store", "fp32-coded"])
def test_a_count_below_max_count_reads_no_row_beyond_it(gpu_ctx, frames, key):
    f = frames(key)
    ranges, n_out = _ranges()
    total = sum(n for _, n, _ in ranges)
    c = Call(f, n_out, 40, total)
    for n in (5, len(ranges), 1, 0):
        c.refill()
        c.run(gpu_ctx, _rows(ranges[:n], rows=40), count=_count(n))
        _clean(gpu_ctx, f)
        c.check(ranges[:n])
    # only empty ranges: nothing is written
    empty = [(5, 0, 0), (N, 0, n_out), (0, 0, 7)]
    c.refill()
    c.run(gpu_ctx, _rows(empty, rows=40), count=_count(3))
    _clean(gpu_ctx, f)
    c.check([])
    assert bool((c.out == SENTINEL).all()) and bool((c.work == SENTINEL).all())


@pytest.mark.parametrize("key", ["bf16-store", "fp32-i0", "i64-coded", "uniform"])
def test_one_range_over_the_whole_tensor_is_the_whole_decode(gpu_ctx, frames, key):
    f = frames(key)
    whole = torch.zeros_like(f.t)
    gpu_ctx.decode_device_planes(f.planes, f.frame, whole, _full(H.planes_workspace_bytes(f.W, N)))
    assert gpu_ctx.planes_status(f.planes) == [0] * f.W
    c = Call(f, N + 3, 1, N)
    c.run(gpu_ctx, _rows([(0, N, 0)]))
    _clean(gpu_ctx, f)
    c.check([(0, N, 0)])
    assert torch.equal(c.out[: N * f.W], whole.view(torch.uint8)) and torch.equal(whole, f.t)


@pytest.mark.parametrize("key", ["bf16-store", "fp32-coded"])
def test_ten_thousand_short_rows_make_every_workgroup_loop(gpu_ctx, frames, key):
    f = frames(key)
    ROWS, LEN = 10_000, 40
    offsets = np.random.default_rng(41).integers(0, N - LEN + 1, ROWS)
    ranges, at = [], 0
    for k, off in enumerate(int(o) for o in offsets):
        # even rows: the destination 16-aligned against the source's grid (16-byte stores); odd rows: only element-aligned
        while (at - off) % 16 != 0 if k % 2 == 0 else (at - off) % 2 != 1:
            at += 1
        ranges.append((off, LEN, at))
        at += LEN
    c = Call(f, at, ROWS, ROWS * LEN)
    info = f.pg.indirect_info(ROWS, ROWS * LEN, c.out.numel())
    tasks = H.planes_gather_tasks(ranges, N).shape[0]
    assert tasks > 4 * info["merge_grid"], (tasks, info)  # what the inputs are chosen for: every workgroup of the merge loops
    assert ROWS > 4 * 1024                                 # ... and the cut runs several rounds
    c.run(gpu_ctx, _rows(ranges))
    _clean(gpu_ctx, f)
    c.check(ranges)


def test_ranges_made_on_the_device_with_a_device_computed_count(gpu_ctx, frames):
    f = frames("fp32-store")
    ROWS, LEN = 64, 1000
    c = Call(f, ROWS * LEN, ROWS, ROWS * LEN)
    torch.cuda.synchronize()
    # a "router": the table rows whose first element is positive, in table order — rows, count and the call on one stream, nothing waited
    # for and nothing copied to the host in between (a stable sort compacts the picked rows to the front)
    table = f.t[: N // LEN * LEN].view(-1, LEN)
    mask = table[: ROWS * 2, 0] > 0
    order = torch.argsort((~mask).to(torch.int8), stable=True)[:ROWS]
    d_count = mask.sum().clamp(max=ROWS).to(torch.int32).reshape(1)
    k = torch.arange(ROWS, device="cuda")
    used = k < d_count
    d_ranges = torch.stack([torch.where(used, order * LEN, -1), torch.where(used, LEN, -1), torch.where(used, k * LEN, -1)], dim=1).contiguous()
    c.run(gpu_ctx, d_ranges, count=d_count)
    _clean(gpu_ctx, f)
    n = int(d_count.item())
    rows = f.a[: N // LEN * LEN].view(np.int32).reshape(-1, LEN)
    want_picked = np.nonzero(rows[:ROWS * 2, 0] > 0)[0][:ROWS]
    assert 8 < n == want_picked.size
    c.check([(int(r) * LEN, LEN, k * LEN) for k, r in enumerate(want_picked)])


@pytest.mark.parametrize("key", ["bf16-store", "fp32-coded", "uniform"])
def test_graph_replays_read_the_ranges_anew(gpu_ctx, frames, key):
    """one captured call; before every replay the rows and the count are overwritten in place.  Nothing of a replay may leak into the next:
    not its prefix, not its refusal."""
    f = frames(key)
    ROWS, LEN, MAX_ELEMENTS = 400, 100, 60_000
    rng = np.random.default_rng(77)
    full = [(int(o), LEN, k * (LEN + 2) + (k % 2)) for k, o in enumerate(rng.integers(0, N - LEN, ROWS))]
    c = Call(f, 64_000, ROWS, MAX_ELEMENTS)
    d_ranges, d_count = _rows([], rows=ROWS), _count(ROWS)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            c.run(gpu_ctx, d_ranges, count=d_count, stream=side)
    torch.cuda.synchronize()
    c.check([])  # capturing runs nothing
    replays = (("the full list", full, 0), ("150 rows", full[100:250], 0), ("count 0", [], 0),
               ("one refused row", full[:50] + [(N - 5, 10, 0)] + full[50:100], E_DEVICE), ("the full list reversed", full[::-1], 0),
               ("one long range", [(1000, 50_001, 3)], 0))
    for name, ranges, expect in replays:
        d_ranges.copy_(_rows(ranges, rows=ROWS))
        d_count.copy_(_count(len(ranges)))
        c.refill()
        g.replay()
        torch.cuda.synchronize()
        c.check(ranges if expect == 0 else [])
        assert gpu_ctx.planes_gather_refused(f.pg) == expect, name
        assert gpu_ctx.planes_gather_refused(f.pg) == 0, name  # reported once
        assert gpu_ctx.planes_gather_status(f.pg) == [0] * f.W


def test_what_only_the_device_can_see_is_refused_there(gpu_ctx, frames):
    f = frames("fp32-store")
    W = f.W
    good = [(100, 5000, 0), (7, 0, 3), (N - 9, 9, 5003)]
    n_out, total = 5012, 5009
    big = 1 << 62
    # (rows, count word or None, max_elements)
    cases = {
        "beyond the tensor": ([(N - 4, 5, 0)], None, total),
        "an empty range beyond the tensor": ([(N + 1, 0, 0)], None, total),
        "offset + length wraps": ([(2**64 - 2, 4, 0)], None, total),
        "dst_offset + length wraps": ([(0, 16, 2**64 - 8)], None, total),
        "beyond the output": ([(0, 16, n_out - 15)], None, total),
        "(dst_offset + length) * elem_size wraps": ([(0, 16, big)], None, total),
        "a count above max_count": (good, 5, total),
        "a count of 2^32 - 1": (good, 0xFFFFFFFF, total),
        "the slots do not fit the stride": (good, None, 1000),
        "a bad row behind good ones": (good + [(N, 1, 0)], None, total),
    }
    for name, (rows, count, max_elements) in cases.items():
        c = Call(f, n_out, 4, max_elements)
        c.run(gpu_ctx, _rows(rows, rows=4), count=None if count is None and len(rows) == 4 else _count(len(rows) if count is None else count))
        assert gpu_ctx.planes_gather_refused(f.pg) == E_DEVICE, name
        assert gpu_ctx.planes_gather_refused(f.pg) == 0, name  # once
        assert gpu_ctx.planes_gather_status(f.pg) == [0] * W, name
        c.check([])
        assert bool((c.out == SENTINEL).all()) and bool((c.work == SENTINEL).all()), name
        # the next good call is bit-exact
        ok = Call(f, n_out, 4, total)
        ok.run(gpu_ctx, _rows(good, rows=4), count=_count(3))
        _clean(gpu_ctx, f)
        ok.check(good)


def test_the_call_refuses_bad_arguments_on_the_host(gpu_ctx, frames):
    f = frames("fp32-store")
    W, L, ctx = 4, gpu_ctx.L, gpu_ctx.handle
    other = H.Context(0)
    ranges = [(100, 5000, 0), (7, 0, 3), (N - 9, 9, 5003)]
    n_out, total, MAXC = 5012, 5009, 4
    need_work, need_ws = H.planes_gather_workspace_bytes(W, MAXC, total), H.planes_gather_indirect_workspace_bytes(W, MAXC)
    out, work, ws = _full(W * n_out + 32), _full(need_work + 32), _full(need_ws + 512)
    joined = _full(W * n_out + need_work + need_ws + 1024)
    d_ranges, d_count = _rows(ranges, rows=MAXC + 1), torch.from_numpy(np.asarray([3, 3], np.int32)).cuda()
    # a gather object of another context, over planes of that context
    o_t, o_frame, o_work = f.t.clone(), _full(f.frame.numel()), _full(H.planes_workspace_bytes(W, N))
    _, o_desc, o_plans = other.encode_device_planes(o_t, o_frame, o_work)
    o_planes = other.make_planes(o_desc, o_plans)
    o_pg = other.make_planes_gather(o_planes, o_frame)

    ok = dict(ctx=ctx, pg=f.pg.handle, d_ranges=d_ranges.data_ptr(), d_count=d_count.data_ptr(), max_count=MAXC, max_elements=total, d_out=out.data_ptr(), oc=W * n_out,
              d_work=work.data_ptr(), wb=need_work, d_ws=ws.data_ptr(), wsb=need_ws)
    assert ok["d_ws"] % 256 == 0 and ok["d_ranges"] % 8 == 0
    jp = joined.data_ptr()
    j_work = jp + _up(W * n_out, 256)
    j_ws = j_work + _up(need_work, 256)
    bad = [
        dict(ctx=None), dict(pg=None), dict(d_ranges=None), dict(d_out=None), dict(d_work=None), dict(d_ws=None),
        dict(pg=o_pg.handle), dict(ctx=other.handle),                                   # a gather object of another context
        dict(d_out=out.data_ptr() + 8), dict(d_work=work.data_ptr() + 4),                # alignment
        dict(d_ranges=d_ranges.data_ptr() + 4), dict(d_count=d_count.data_ptr() + 2), dict(d_ws=ws.data_ptr() + 128),
        dict(wsb=need_ws - 1), dict(wsb=0), dict(wb=need_work - 1), dict(wb=0),          # below the size functions
        dict(max_count=(1 << 31) // W), dict(max_elements=2**64 - 64),                   # a size function returns 0
        dict(d_out=f.frame.data_ptr() + 256), dict(d_work=f.frame.data_ptr()), dict(d_ws=f.frame.data_ptr()),  # on the frame
        dict(d_out=jp, d_work=jp + (W * n_out & ~15) - 16),                              # the workspace begins inside the output
        dict(d_out=jp, d_work=j_work, d_ws=j_work + (need_work & ~255) - 256),          # the control workspace begins inside the data workspace
        dict(d_out=jp, d_ws=jp + 256),                                                   # ... inside the output
        dict(d_ranges=jp + 64, d_out=jp),                                                # the ranges lie in the output
        dict(d_count=j_work + 16, d_work=j_work),                                        # the count lies in the data workspace
        dict(d_ranges=j_ws + 8, d_ws=j_ws), dict(d_count=j_ws + need_ws - 4, d_ws=j_ws),  # ... in the control workspace
    ]

    def call(k):
        return L.hsrans_decode_device_planes_gather_indirect(k["ctx"], k["pg"], k["d_ranges"], k["d_count"], k["max_count"], k["max_elements"], k["d_out"], k["oc"],
                                                             k["d_work"], k["wb"], k["d_ws"], k["wsb"], None)

    before = f.frame.clone()
    for change in bad:
        assert call(dict(ok, **change)) == E_ARG, change
    assert call(dict(ok, max_count=0)) == 0  # nothing to do, nothing queued
    torch.cuda.synchronize()
    for t in (out, work, joined):
        assert bool((t == SENTINEL).all())
    assert torch.equal(f.frame, before)
    _clean(gpu_ctx, f)
    # the wrapper's own refusals
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_planes_gather_indirect(f.pg, d_ranges, out.view(torch.int16), work)
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_planes_gather_indirect(f.pg, d_ranges, out.view(torch.int32), work.view(torch.int32))
    with pytest.raises(TypeError):
        gpu_ctx.decode_device_planes_gather_indirect(f.pg, d_ranges.view(-1), out.view(torch.int32), work)
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.decode_device_planes_gather_indirect(f.pg, d_ranges, out.view(torch.int32), work[:1024], max_count=MAXC, max_elements=total)
    assert e.value.code == E_ARG
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((work == SENTINEL).all())
    # what was refused still gathers, with the very arguments of `ok`
    assert call(ok) == 0
    _clean(gpu_ctx, f)
    assert np.array_equal(out.cpu().numpy()[: W * n_out], _expected_out(f, ranges, n_out))
    assert np.array_equal(work.cpu().numpy(), _expected_work(f, ranges, work.numel(), _stride(MAXC, total)))
    # max_elements left to the wrapper: what d_work can hold
    c = Call(f, n_out, 3, total)
    gpu_ctx.decode_device_planes_gather_indirect(f.pg, _rows(ranges), c.out.view(torch.int32), c.work[: c.need_work])
    _clean(gpu_ctx, f)
    assert np.array_equal(c.out.cpu().numpy(), _expected_out(f, ranges, n_out))
    o_pg.close()
    o_planes.close()


def test_two_calls_in_flight_on_two_streams(gpu_ctx, frames):
    f = frames("fp32-store")
    r1, n1 = _ranges()
    r2, n2 = _ranges(SHAPES[::-1], first=11)
    total = sum(n for _, n, _ in r1)
    c1, c2 = Call(f, n1, len(r1), total), Call(f, n2, len(r2) + 3, total + 100)
    d1, d2, k2 = _rows(r1), _rows(r2, rows=len(r2) + 3), _count(len(r2))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        c1.run(gpu_ctx, d1, stream=s1)
    with torch.cuda.stream(s2):
        c2.run(gpu_ctx, d2, count=k2, stream=s2)
    s1.synchronize()
    s2.synchronize()
    _clean(gpu_ctx, f)
    c1.check(r1)
    c2.check(r2)
    # the objects are as they were: the host-ranges call and the whole decode still give the tensor
    host_out, _ = _gather(gpu_ctx, f, r1, n1)
    assert gpu_ctx.planes_gather_status(f.pg) == [0] * f.W
    assert torch.equal(host_out, c1.out)
    whole = torch.zeros_like(f.t)
    gpu_ctx.decode_device_planes(f.planes, f.frame, whole, _full(H.planes_workspace_bytes(f.W, N)))
    assert gpu_ctx.planes_status(f.planes) == [0] * f.W
    assert torch.equal(whole, f.t)
