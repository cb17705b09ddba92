"""hsrans_decode_device_gather_indirect on the GPU, bit-exact: the ranges are in device memory, the device cuts them into tasks, and the
bytes land where hsrans_decode_device_gather puts them for the same ranges — and nowhere else.  Expected bytes are always the encoder's
input, data[offset : offset + length].  Every gather writes into a buffer filled with 0xCC that has 4 KiB of canary in front of and
behind the destination; the WHOLE buffer is compared, so a byte written outside a range fails the case.  Inputs the device refuses
(kStatusBadRange) must leave the destination entirely alone and show up in the plan's status exactly once."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth

import test_gpu_gather as G

pytestmark = pytest.mark.gpu

N, BLOCK, CANARY, CONTAINERS = G.N, G.BLOCK, G.CANARY, G.CONTAINERS
E_ARG, E_FORMAT, E_DEVICE = 2, 3, 5
GARBAGE = np.array([0xFFFFFFFFFFFFFFF0, 0x7FFFFFFFFFFFFFFF, 0xDEADBEEFDEADBEEF], np.uint64)  # a row no call may act on


@pytest.fixture(scope="module")
def datasets():
    out = {}
    for name, d in (("nonstat", synth.nonstationary(N)), ("zipf", synth.enwik8_shaped(N, seed=11))):
        d = d.copy()
        d[G.FILL_BLOCK * BLOCK:(G.FILL_BLOCK + 1) * BLOCK] = 0x41
        out[name] = d
    return out


def _device_ranges(ranges, rows=None):
    """(n, 3) uint64 -> a CUDA int64 tensor of `rows` >= n rows; the rows behind n hold garbage"""
    ranges = np.asarray(ranges, np.uint64).reshape(-1, 3)
    rows = ranges.shape[0] if rows is None else rows
    full = np.tile(GARBAGE, (max(rows, 1), 1))
    full[:ranges.shape[0]] = ranges
    return torch.from_numpy(full.view(np.int64)).cuda()


def _want(size, ranges, data):
    want = np.full(size, 0xCC, np.uint8)
    for off, length, dst in ranges:
        want[int(dst):int(dst + length)] = data[int(off):int(off + length)]
    return want


def _explain(got, want, ranges):
    bad = int(np.argmax(got != want))
    row = int(np.searchsorted(ranges[:, 2], bad, side="right")) - 1 if len(ranges) else -1
    return f"first wrong byte at destination {bad} (of {want.size}), range {row}: {ranges[max(row, 0)].tolist() if len(ranges) else None}, got {got[bad]} want {want[bad]}"


def _indirect_and_check(ctx, dplan, d_stream, m, data, src, packing="packed", misalign=0, with_count=True, spare_rows=0, against_host=True):
    """one indirect gather of the (offset, length) pairs `src`; compares the whole destination buffer, canaries included, with the data and
    with what decode_device_gather leaves for the same ranges"""
    ranges, size = G._layout(src, packing, base_align=misalign)
    n = ranges.shape[0]
    want = _want(size, ranges, data)
    backing = torch.full((size + 16,), 0xCC, dtype=torch.uint8, device="cuda")
    d_dst = backing[misalign:misalign + size]
    d_ranges = _device_ranges(ranges, n + spare_rows)
    count = torch.tensor(n, dtype=torch.int32, device="cuda") if with_count else None
    ctx.decode_device_gather_indirect(dplan, d_stream, d_ranges, d_dst, count=count, max_count=(n + spare_rows) if with_count else n, stream_length=m)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got, want), _explain(got, want, ranges)
    whole = backing.cpu().numpy()
    assert np.all(whole[size + misalign:] == 0xCC) and np.all(whole[:misalign] == 0xCC)
    assert ctx.status(dplan) == 0
    if against_host:
        backing2 = torch.full((size + 16,), 0xCC, dtype=torch.uint8, device="cuda")
        ctx.decode_device_gather(dplan, d_stream, ranges, backing2[misalign:misalign + size], stream_length=m)
        torch.cuda.synchronize()
        assert torch.equal(backing, backing2)
    return ranges


@pytest.mark.parametrize("bits", (11, 12, 14, 15))
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("kind", CONTAINERS)
def test_matrix(gpu_ctx, datasets, kind, states, bits):
    data = datasets["nonstat" if states == 64 else "zipf"]
    s, plan = G._encode(gpu_ctx, kind, states, bits, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = G._upload(s)
    rng = np.random.default_rng(200_000 * CONTAINERS.index(kind) + 100 * states + bits)
    src = G._random_src(rng, 1100, N)
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, src, "packed")                                 # random ranges, back to back
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, G._explicit_src(N, states), "gaps")            # the explicit ones, canary between them
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, G._explicit_src(N, states), "packed", misalign=1)
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, src[:300], "aligned", with_count=False)        # the word-store path; count = NULL
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, [(0, N)], "packed", misalign=3)                # one range = the whole stream


@pytest.mark.parametrize("states,bits", ((64, 11), (32, 12), (64, 14)))
def test_raw_without_index(gpu_ctx, datasets, states, bits):
    data = datasets["zipf"][:600_011]
    s, plan = G._encode(gpu_ctx, "raw", states, bits, data)
    assert H.plan_chain_count(plan) == 1
    dplan = gpu_ctx.make_device_plan(plan)
    _indirect_and_check(gpu_ctx, dplan, G._upload(s), s.size, data, [(300_000, 5000)], "packed")
    _indirect_and_check(gpu_ctx, dplan, G._upload(s), s.size, data, [(299_999, 4097), (0, 3), (data.size - 5, 5)], "gaps", misalign=1)


@pytest.mark.parametrize("states,bits,interval", ((64, 11, 32), (32, 12, 32), (64, 14, 0)))
def test_plan_written_on_the_device(gpu_ctx, datasets, states, bits, interval):
    data = datasets["nonstat"]
    d_in = torch.from_numpy(data).cuda()
    d_out = torch.empty(H.capacity(H.MT, states, data.size), dtype=torch.uint8, device="cuda")
    m, dplan = gpu_ctx.encode_device(H.MT, states, bits, d_in, d_out, block_size=BLOCK, index_interval=interval, want_plan=True)
    rng = np.random.default_rng(17 + bits)
    _indirect_and_check(gpu_ctx, dplan, d_out, m, data, G._random_src(rng, 400, N) + G._explicit_src(N, states), "packed")
    _indirect_and_check(gpu_ctx, dplan, d_out, m, data, G._explicit_src(N, states), "aligned")


def test_plan_from_an_indexing_decode(gpu_ctx, datasets):
    data = datasets["nonstat"]
    s = H.encode(H.MT, 64, 11, data, block_size=BLOCK)
    d_stream = G._upload(s)
    base = gpu_ctx.make_device_plan_from_stream(H.MT, 64, 11, d_stream, s.size, N)
    out = torch.zeros(N, dtype=torch.uint8, device="cuda")
    indexed = gpu_ctx.decode_device_indexing(base, d_stream, out, 32, stream_length=s.size)
    rng = np.random.default_rng(15)
    _indirect_and_check(gpu_ctx, base, d_stream, s.size, data, G._random_src(rng, 200, N), "packed")
    _indirect_and_check(gpu_ctx, indexed, d_stream, s.size, data, G._random_src(rng, 400, N) + G._explicit_src(N, 64), "packed")


def test_counts(gpu_ctx, datasets):
    """*d_count below max_count: the rows behind it hold garbage and are never read; 0: nothing happens; NULL: max_count rows"""
    data = datasets["zipf"]
    s, plan = G._encode(gpu_ctx, "mt32", 64, 11, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = G._upload(s)
    rng = np.random.default_rng(41)
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, G._random_src(rng, 333, N), "packed", spare_rows=700)
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, G._random_src(rng, 1, N), "packed", spare_rows=5000)
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, [], "packed", spare_rows=100, against_host=False)  # *d_count == 0
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, G._random_src(rng, 77, N), "packed", with_count=False)
    # only empty ranges: a launch without a task
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, [(5, 0), (N, 0), (0, 0)], "gaps")


@pytest.mark.parametrize("kind,states,bits", (("raw32", 64, 11), ("mt", 32, 12)))
def test_more_tasks_than_the_grid_has_waves(gpu_ctx, datasets, kind, states, bits):
    data = datasets["nonstat"]
    s, plan = G._encode(gpu_ctx, kind, states, bits, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = G._upload(s)
    # 100 % of the stream in 4 KiB ranges
    src = [(o, min(4096, N - o)) for o in range(0, N, 4096)]
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, src, "packed")
    _indirect_and_check(gpu_ctx, dplan, d_stream, s.size, data, src, "packed", misalign=1)
    # A grid far smaller than the task total: the host sizes it from max_count + dst_capacity / L, so many long ranges aimed at ONE small
    # destination window make a small grid with many tasks.  All ranges keep the same dst_offset - offset, so overlapping destinations
    # receive the same bytes whichever task writes them.
    rng = np.random.default_rng(8)
    L = H.gather_segment(N, H.plan_chain_count(plan), states, 32 if kind == "raw32" else 0)  # (mt_ without checkpoints: a block, not a power of two)
    w0, W, count = 500_001, 24 * L, 200
    assert w0 + W <= N
    lens = rng.integers(W // 4, W, count)
    offs = w0 + (rng.random(count) * (W - lens)).astype(np.int64)
    ranges = np.stack([offs, lens, offs - w0 + CANARY], axis=1).astype(np.uint64)
    tasks = H.gather_tasks(N, H.plan_chain_count(plan), states, 32 if kind == "raw32" else 0, ranges).shape[0]
    size = W + 2 * CANARY
    assert tasks > 4 * (count + size // L), (tasks, count, size, L)  # several rounds of the strided loop for every wave of the grid
    lo, hi = int(offs.min()), int((offs + lens).max())
    want = np.full(size, 0xCC, np.uint8)
    want[lo - w0 + CANARY:hi - w0 + CANARY] = data[lo:hi]
    covered = np.zeros(size, bool)
    for off, length, dst in ranges:
        covered[int(dst):int(dst + length)] = True
    assert covered[lo - w0 + CANARY:hi - w0 + CANARY].all()  # (the union is one interval: `want` above is exact)
    d_dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device_gather_indirect(dplan, d_stream, _device_ranges(ranges), d_dst, stream_length=s.size)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got, want), _explain(got, want, ranges[:0])
    assert gpu_ctx.status(dplan) == 0
    # range by range, each through a call of its own into a buffer of its own
    for off, length, dst in ranges[::20]:
        one = np.array([[off, length, CANARY]], np.uint64)
        d_one = torch.full((int(length) + 2 * CANARY,), 0xCC, dtype=torch.uint8, device="cuda")
        gpu_ctx.decode_device_gather_indirect(dplan, d_stream, _device_ranges(one), d_one, stream_length=s.size)
        torch.cuda.synchronize()
        assert np.array_equal(d_one.cpu().numpy(), _want(d_one.numel(), one, data))
    assert gpu_ctx.status(dplan) == 0


def test_ranges_made_on_the_device(gpu_ctx, datasets):
    """the ranges come out of torch kernels on the same stream and never visit the host; nothing is synchronised before the gather"""
    data = datasets["zipf"]
    s, plan = G._encode(gpu_ctx, "raw32", 64, 11, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = G._upload(s)
    rng = np.random.default_rng(23)
    PAGE, LEN, count = 1000, 3001, 500
    pages = rng.integers(0, (N - LEN) // PAGE, count).astype(np.int64)
    d_dst = torch.full((count * LEN + 2 * CANARY,), 0xCC, dtype=torch.uint8, device="cuda")
    workspace = torch.empty(H.gather_workspace_bytes(count), dtype=torch.uint8, device="cuda")
    d_pages = torch.from_numpy(pages).cuda()
    torch.cuda.synchronize()
    # a "page table" lookup on the GPU: offset = page * PAGE + 7, fixed length, destinations back to back behind the canary
    d_off = d_pages * PAGE + 7
    d_len = torch.full_like(d_off, LEN)
    d_pos = torch.arange(count, dtype=torch.int64, device="cuda") * LEN + CANARY
    d_ranges = torch.stack([d_off, d_len, d_pos], dim=1).contiguous()
    d_count = (d_pages >= 0).sum().to(torch.int32)  # = count, computed on the device as well
    gpu_ctx.decode_device_gather_indirect(dplan, d_stream, d_ranges, d_dst, count=d_count, workspace=workspace, stream_length=s.size)
    torch.cuda.synchronize()
    ranges = np.stack([pages * PAGE + 7, np.full(count, LEN), np.arange(count) * LEN + CANARY], axis=1).astype(np.uint64)
    got, want = d_dst.cpu().numpy(), _want(d_dst.numel(), ranges, data)
    assert np.array_equal(got, want), _explain(got, want, ranges)
    assert gpu_ctx.status(dplan) == 0


@pytest.mark.parametrize("kind,states,bits", (("raw32", 64, 11), ("mt", 64, 14)))
def test_graph_replays_read_the_ranges_anew(gpu_ctx, datasets, kind, states, bits):
    """one captured call (two kernel nodes in a line); before every replay the ranges and the count are overwritten in place"""
    data = datasets["nonstat"]
    s, plan = G._encode(gpu_ctx, kind, states, bits, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = G._upload(s)
    ROWS, SIZE = 600, 12_000_000
    rng = np.random.default_rng(77)
    d_ranges = _device_ranges(np.zeros((0, 3), np.uint64), ROWS)
    d_count = torch.zeros((), dtype=torch.int32, device="cuda")
    d_dst = torch.full((SIZE,), 0xCC, dtype=torch.uint8, device="cuda")
    workspace = torch.empty(H.gather_workspace_bytes(ROWS), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            gpu_ctx.decode_device_gather_indirect(dplan, d_stream, d_ranges, d_dst, count=d_count, max_count=ROWS, workspace=workspace, stream=side, stream_length=s.size)
    torch.cuda.synchronize()
    assert bool((d_dst == 0xCC).all())  # capturing runs nothing
    totals = []
    for src in (G._random_src(rng, 500, N // 8)[:500], [(0, 1), (N - 1, 1), (7 * BLOCK - 1, 2)], [(1_000_001, 3_000_000 - 1_000_001)],
                [(o, l) for o, l in G._random_src(rng, ROWS, N) if l <= 8192][:ROWS], []):
        ranges, size = G._layout(src, "packed")
        assert size <= SIZE and ranges.shape[0] <= ROWS
        totals.append(H.gather_tasks(N, H.plan_chain_count(plan), states, 32 if kind == "raw32" else 0, ranges).shape[0])
        d_ranges.copy_(_device_ranges(ranges, ROWS))
        d_count.fill_(ranges.shape[0])
        d_dst.fill_(0xCC)
        g.replay()
        torch.cuda.synchronize()
        got, want = d_dst.cpu().numpy(), _want(SIZE, ranges, data)
        assert np.array_equal(got, want), _explain(got, want, ranges)
        assert gpu_ctx.status(dplan) == 0
    assert len(set(totals)) >= 4, totals  # the replays differ in their task totals


def test_device_refusals(gpu_ctx, datasets):
    """what only the device can see: nothing is gathered, the status reports it once, the next call is fine"""
    data = datasets["zipf"][:400_003]
    n = data.size
    s, plan = G._encode(gpu_ctx, "raw32", 64, 11, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = G._upload(s)
    CAP = 20_000
    backing = torch.full((CAP + 2 * CANARY,), 0xCC, dtype=torch.uint8, device="cuda")
    d_dst = backing[CANARY:CANARY + CAP]
    good = [(0, 100, 0), (5000, 3000, 200), (n - 10, 10, 19_990)]

    def refused(ranges, count=None, max_count=None):
        rows = np.asarray(ranges, np.uint64).reshape(-1, 3)
        d_count = None if count is None else torch.tensor(count, dtype=torch.int32, device="cuda")
        gpu_ctx.decode_device_gather_indirect(dplan, d_stream, _device_ranges(rows, max(rows.shape[0], max_count or 0)), d_dst, count=d_count,
                                              max_count=max_count, stream_length=s.size)
        torch.cuda.synchronize()
        assert bool((backing == 0xCC).all())
        assert gpu_ctx.status(dplan) == E_DEVICE
        assert gpu_ctx.status(dplan) == 0
        # ... and the plan is as good as before
        gpu_ctx.decode_device_gather_indirect(dplan, d_stream, _device_ranges(good), d_dst, stream_length=s.size)
        torch.cuda.synchronize()
        assert np.array_equal(d_dst.cpu().numpy(), _want(CAP, np.array(good, np.uint64), data)) and gpu_ctx.status(dplan) == 0
        assert bool((backing[:CANARY] == 0xCC).all()) and bool((backing[CANARY + CAP:] == 0xCC).all())
        d_dst.fill_(0xCC)

    refused(good[:2] + [(n - 10, 11, 300)])                         # a range past the decoded length (the valid ones in front of it: not gathered either)
    refused([(n + 1, 0, 0)])
    refused([(0, 100, 0), (5000, 10_000, 10_001)])                  # dst_offset + length past dst_capacity
    refused([(0, 1, CAP)])
    refused([(2 ** 64 - 8, 16, 0)] + good)                          # offset + length wraps
    refused([(8, 2 ** 64 - 4, 0)])
    refused([(0, 16, 2 ** 64 - 8)])                                 # dst_offset + length wraps
    refused(good, count=4, max_count=3)                             # *d_count > max_count
    refused(good, count=-1, max_count=3)                            # (as uint32: 2^32 - 1)


def test_host_refusals_leave_the_destination_alone(gpu_ctx, datasets):
    data = datasets["zipf"][:400_003]
    s, plan = G._encode(gpu_ctx, "raw32", 64, 11, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = G._upload(s)
    d_dst = torch.full((20_000,), 0xCC, dtype=torch.uint8, device="cuda")
    d_ranges = _device_ranges([(0, 100, 0), (5000, 3000, 200)])
    need = H.gather_workspace_bytes(2)
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0

    def refused(code, dp=dplan, stream=d_stream, m=s.size, ranges=d_ranges, workspace=ws, **kw):
        with pytest.raises(H.HsransError) as e:
            gpu_ctx.decode_device_gather_indirect(dp, stream, ranges, d_dst, workspace=workspace, stream_length=m, **kw)
        assert e.value.code == code, (e.value.code, code)
        torch.cuda.synchronize()
        assert bool((d_dst == 0xCC).all())

    refused(E_ARG, workspace=ws[:need - 256])                        # a short workspace
    refused(E_ARG, workspace=ws[:4])
    refused(E_ARG, workspace=ws[64:64 + need])                       # a misaligned one
    # misaligned ranges (no int64 tensor starts in the middle of a word: the C entry directly)
    rc = gpu_ctx.L.hsrans_decode_device_gather_indirect(gpu_ctx.handle, dplan.handle, d_stream.data_ptr(), s.size, d_ranges.data_ptr() + 4, None, 1, d_dst.data_ptr(),
                                                        d_dst.numel(), ws.data_ptr(), ws.numel(), None)
    assert rc == E_ARG
    refused(E_ARG, stream=d_stream[8:], m=s.size)                    # a misaligned stream
    refused(E_FORMAT, m=s.size - 2)                                  # a wrong stream length
    refused(E_FORMAT, m=s.size + 16)
    sb, pb = G._encode(gpu_ctx, "block", 64, 11, data)               # block_ without checkpoints: a walk plan, no entry points
    refused(E_FORMAT, dp=gpu_ctx.make_device_plan(pb), stream=G._upload(sb), m=sb.size)
    # max_count == 0: fine, nothing queued
    gpu_ctx.decode_device_gather_indirect(dplan, d_stream, d_ranges, d_dst, max_count=0, workspace=ws, stream_length=s.size)
    torch.cuda.synchronize()
    assert bool((d_dst == 0xCC).all()) and gpu_ctx.status(dplan) == 0


def test_two_streams_two_workspaces(gpu_ctx, datasets):
    """nothing orders the calls of the two streams: each has its own workspace and destination"""
    data = datasets["zipf"]
    s, plan = G._encode(gpu_ctx, "raw32", 64, 12, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = G._upload(s)
    rng = np.random.default_rng(13)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    jobs = []
    for k in range(8):
        ranges, size = G._layout(G._random_src(rng, 600, N), "packed")
        jobs.append((ranges, size, _device_ranges(ranges), torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")))
    workspaces = [torch.empty(H.gather_workspace_bytes(600), dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for k, (ranges, size, d_ranges, d_dst) in enumerate(jobs):  # (calls of ONE stream share its workspace: they run in order)
        gpu_ctx.decode_device_gather_indirect(dplan, d_stream, d_ranges, d_dst, workspace=workspaces[k % 2], stream_length=s.size, stream=streams[k % 2])
    torch.cuda.synchronize()
    for ranges, size, d_ranges, d_dst in jobs:
        got, want = d_dst.cpu().numpy(), _want(size, ranges, data)
        assert np.array_equal(got, want), _explain(got, want, ranges)
    assert gpu_ctx.status(dplan) == 0


def test_a_million_ranges(gpu_ctx, datasets):
    """max_count above 2^20: k_gather_cut's workgroup loops over the ranges 1025 times, k_gather_ranges searches a prefix of 2^20 + 6 entries"""
    data = datasets["nonstat"]
    s, plan = G._encode(gpu_ctx, "raw32", 64, 11, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = G._upload(s)
    rng = np.random.default_rng(2)
    count = (1 << 20) + 5
    lens = rng.integers(0, 4, count).astype(np.int64)  # 0 .. 3 bytes: a quarter of the ranges has no task
    offs = rng.integers(0, N - 3, count).astype(np.int64)
    ends = np.cumsum(lens)
    dsts = ends - lens + CANARY
    total = int(ends[-1])
    want = np.full(total + 2 * CANARY, 0xCC, np.uint8)
    want[CANARY:CANARY + total] = data[np.repeat(offs, lens) + (np.arange(total) - np.repeat(ends - lens, lens))]
    d_ranges = torch.from_numpy(np.stack([offs, lens, dsts], axis=1)).cuda()
    d_dst = torch.full((want.size,), 0xCC, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device_gather_indirect(dplan, d_stream, d_ranges, d_dst, stream_length=s.size)
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), want)
    assert gpu_ctx.status(dplan) == 0
