"""hsrans_decode_device_gather_batch_indirect on the GPU, bit-exact: the ranges of MANY streams are in device memory, the device checks,
sorts and cuts them, and the bytes land where hsrans_decode_device_gather_batch puts them for the same rows — and nowhere else.  Expected
bytes are always the encoder's input, data[member][offset : offset + length].  Every gather writes into a buffer filled with 0xCC that has
4 KiB of canary in front of and behind the destination; the WHOLE buffer is compared, so a byte written outside a range, or taken from the
wrong member, fails the case.  Every member's status and the set's own refusal word must stay 0 unless the case says otherwise; rows the
device refuses must leave the destination entirely alone and show up in gather_set_refused exactly once."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from test_gpu_gather import _encode, _upload
from test_gpu_gather_batch import CANARY, MEMBERS, N, N_RAW, _altered_member, _explicit_src, _layout, _random_src, _Set, _want

pytestmark = pytest.mark.gpu

E_ARG, E_DEVICE = 2, 5
GARBAGE = np.array([0xFFFFFFFFFFFFFFF0, 0x7FFFFFFFFFFFFFFF, 0xDEADBEEFDEADBEEF, 0xFFFFFFFF], np.uint64)  # a row no call may act on: member 2^32 - 1
K = len(MEMBERS)


@pytest.fixture(scope="module")
def ten(gpu_ctx):
    return _Set(gpu_ctx)


def _device_rows(ranges, rows=None, reserved=0):
    """(n, 4) rows (member, offset, length, dst_offset) -> a CUDA int64 tensor of `rows` >= n rows in the layout of hsrans_member_range:
    (offset, length, dst_offset, member | reserved << 32); the rows behind n hold garbage"""
    ranges = np.asarray(ranges, np.uint64).reshape(-1, 4)
    rows = ranges.shape[0] if rows is None else rows
    full = np.tile(GARBAGE, (max(rows, 1), 1))
    full[:ranges.shape[0], :3] = ranges[:, 1:]
    full[:ranges.shape[0], 3] = ranges[:, 0] | np.uint64(reserved << 32)
    return torch.from_numpy(full.view(np.int64)).cuda()


def _explain(got, want, ranges):
    bad = int(np.argmax(got != want))
    hit = [r.tolist() for r in ranges if int(r[3]) <= bad < int(r[3] + r[2])][:3]
    return f"first wrong byte at destination {bad} (of {want.size}), got {got[bad]} want {want[bad]}; ranges (member, offset, length, dst) there: {hit}"


def _clean(ctx, gset):
    assert ctx.gather_set_status(gset) == [0] * len(gset.dplans)
    assert ctx.gather_set_refused(gset) == 0


def _indirect_and_check(ctx, gset, data, src, packing="packed", misalign=0, with_count=True, spare_rows=0, against_host=True):
    """one indirect gather of the (member, offset, length) triples `src`; compares the whole destination buffer, canaries included, with
    the data and byte for byte with what decode_device_gather_batch leaves for the same rows"""
    ranges, size = _layout(src, packing, base_align=misalign)
    n = ranges.shape[0]
    want = _want(data, ranges, size)
    backing = torch.full((size + 16,), 0xCC, dtype=torch.uint8, device="cuda")
    d_dst = backing[misalign:misalign + size]
    d_ranges = _device_rows(ranges, n + spare_rows)
    count = torch.tensor(n, dtype=torch.int32, device="cuda") if with_count else None
    ctx.decode_device_gather_batch_indirect(gset, d_ranges, d_dst, count=count, max_count=(n + spare_rows) if with_count else n)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got, want), _explain(got, want, ranges)
    whole = backing.cpu().numpy()
    assert np.all(whole[size + misalign:] == 0xCC) and np.all(whole[:misalign] == 0xCC)
    _clean(ctx, gset)
    if against_host:
        backing2 = torch.full((size + 16,), 0xCC, dtype=torch.uint8, device="cuda")
        ctx.decode_device_gather_batch(gset, ranges, backing2[misalign:misalign + size])
        torch.cuda.synchronize()
        assert torch.equal(backing, backing2)
    return ranges


def _all_explicit(ten):
    return [t for m, (_, states, _) in enumerate(MEMBERS) for t in _explicit_src(m, ten.data[m].size, states)]


def test_whole_buffer(gpu_ctx, ten):
    rng = np.random.default_rng(2025)
    src = _random_src(rng, 600, ten.data)
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, src + _all_explicit(ten), "packed")
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, _all_explicit(ten), "gaps")
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, _all_explicit(ten) + src[:100], "packed", misalign=1)
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, src[:300] + _all_explicit(ten), "aligned")  # the word-store path
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, src[:300], "aligned", misalign=1)


def test_info_describes_the_launches(gpu_ctx, ten):
    before = ten.gset.info()
    info = ten.gset.indirect_info(1000, 5_000_000)
    assert info["members"] == K and info["kind_members"] == before["kind_members"]
    assert info["launches"] == sum(1 for k in range(6) if info["kind_members"][k]) <= 6
    assert info["kind_tasks"] == [0] * 6 and info["kind_entries"] == [0] * 6
    for k in range(6):
        if info["kind_members"][k]:
            assert info["kind_grid"][k] >= 1 and info["kind_waves"][k] in (1, 2, 4, 8, 16) and 0 < info["kind_lds_bytes"][k] <= 160 * 1024
        else:
            assert info["kind_grid"][k] == info["kind_waves"][k] == info["kind_lds_bytes"][k] == 0
    assert ten.gset.indirect_info(0, 5_000_000)["launches"] == 0
    # an indirect call does not write the last host-ranges call's record
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, [(0, 0, 100), (9, 5, 70)], against_host=False)
    assert ten.gset.info() == before


def test_counts(gpu_ctx, ten):
    """*d_count below max_count: the rows behind it hold garbage and are never read; 0: nothing happens; NULL: max_count rows"""
    rng = np.random.default_rng(41)
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, _random_src(rng, 333, ten.data), spare_rows=700)
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, _random_src(rng, 1, ten.data), spare_rows=5000)
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, [], spare_rows=100, against_host=False)  # *d_count == 0
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, _random_src(rng, 77, ten.data), with_count=False)
    # only empty ranges: launches without a task
    _indirect_and_check(gpu_ctx, ten.gset, ten.data, [(2, 5, 0), (9, N_RAW, 0), (0, N, 0), (4, 0, 0)], "gaps")


@pytest.mark.parametrize("spare_rows", (0, 40_000))  # (few possible tasks: small workgroups; many: the largest)
def test_unit_edges_of_the_shared_kinds(gpu_ctx, ten, spare_rows):
    """a unit is `waves` consecutive tasks of one member: task counts around the multiples of `waves`, which indirect_info reports for the
    call's max_count and dst_capacity (the same for every call here).  A one-byte range is exactly one task whatever its member's segment
    length; the host's cut of the same rows confirms the count."""
    rng = np.random.default_rng(5)
    SIZE, ROWS = 1 << 18, 48 + spare_rows
    info = ten.gset.indirect_info(ROWS, SIZE)
    shared_kinds = sorted(k for k in set(ten.kinds) if k >= 3)
    assert len(shared_kinds) >= 2

    def ones(member, tasks):
        return [(member, int(o), 1) for o in rng.integers(0, ten.data[member].size, tasks)]

    def run(src, packing="packed", kind=None, tasks=None):
        ranges, size = _layout(src, packing)
        assert size <= SIZE and ranges.shape[0] <= 48
        d_dst = _run_fixed(gpu_ctx, ten, ranges, SIZE, ROWS)
        d_host = torch.full((SIZE,), 0xCC, dtype=torch.uint8, device="cuda")
        gpu_ctx.decode_device_gather_batch(ten.gset, ranges, d_host)
        torch.cuda.synchronize()
        assert torch.equal(d_dst, d_host)
        if kind is not None:
            assert ten.gset.info()["kind_tasks"][kind] == tasks

    for kind in shared_kinds:
        mine = [m for m in range(K) if ten.kinds[m] == kind]
        m, waves = mine[0], info["kind_waves"][kind]
        assert waves in (1, 2, 4, 8, 16)
        print("kind", kind, "max_count", ROWS, "waves", waves)
        for tasks in (waves - 1, waves, waves + 1, 3 * waves):
            if tasks:
                run(ones(m, tasks), kind=kind, tasks=tasks)
        if len(mine) >= 2:  # two members of the kind in one call: 1 and waves + 1 tasks
            run(ones(mine[1], 1) + ones(m, waves + 1), kind=kind, tasks=waves + 2)
            run(ones(m, waves + 1) + ones(mine[1], 1), "gaps", kind=kind, tasks=waves + 2)
        run([(m, int(rng.integers(0, ten.data[m].size - 5000)), int(rng.integers(1, 5000))) for _ in range(40)])  # all ranges on one member
    run([(m, 1000 + 37 * m, 333) for m in range(K)], "gaps")  # one range per member


def _run_fixed(ctx, ten, ranges, size, max_count):
    """rows `ranges` with *d_count = their number and exactly max_count rows, into a buffer of exactly `size` bytes: whole buffer, status"""
    want = _want(ten.data, ranges, size)
    d_dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    count = torch.tensor(ranges.shape[0], dtype=torch.int32, device="cuda")
    ctx.decode_device_gather_batch_indirect(ten.gset, _device_rows(ranges, max_count), d_dst, count=count, max_count=max_count)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got, want), _explain(got, want, ranges)
    _clean(ctx, ten.gset)
    return d_dst


def test_a_set_of_1500_members(gpu_ctx, ten):
    """the ten plans repeated: the scan over the members' positions crosses its 1024-wide round"""
    members = [k % K for k in range(1500)]
    big = gpu_ctx.make_gather_set([ten.dplans[m] for m in members], [ten.d_streams[m] for m in members], [ten.sizes[m] for m in members])
    data = [ten.data[m] for m in members]
    info = big.indirect_info(1000, 1 << 20)
    assert info["members"] == 1500 and sum(info["kind_members"]) == 1500
    rng = np.random.default_rng(19)
    chosen = [0, 1023, 1024, 1499] + [int(m) for m in rng.integers(0, 1500, 200)]
    src = _random_src(rng, 400, data, members=chosen) + [(m, 1000 + m, 2000) for m in (0, 1023, 1024, 1499)]
    _indirect_and_check(gpu_ctx, big, data, src, "packed")
    _indirect_and_check(gpu_ctx, big, data, [(m, 7, 5000) for m in (1499, 1024, 1023, 0)], "gaps", misalign=1, spare_rows=50)
    _clean(gpu_ctx, ten.gset)


def test_more_tasks_than_the_grid_has_waves(gpu_ctx, ten):
    """many long ranges aimed at one small window per member: the grids are sized from max_count and dst_capacity, so every wave loops.
    All ranges of a member keep one dst_offset - offset, so overlapping destinations receive the same bytes whichever task writes them."""
    indexed = [m for m in range(K) if MEMBERS[m][0] in ("raw32", "mt32", "block32")]  # (a checkpoint every 32 groups: L is the 4 KiB floor)
    private = next(m for m in indexed if ten.kinds[m] < 3)
    shared = next(m for m in indexed if ten.kinds[m] >= 3)
    pair = [private, shared]
    gset = gpu_ctx.make_gather_set([ten.dplans[m] for m in pair], [ten.d_streams[m] for m in pair], [ten.sizes[m] for m in pair])
    data = [ten.data[m] for m in pair]
    rng = np.random.default_rng(8)
    L, count = 4096, 200
    W = 24 * L
    size = 2 * W + 3 * CANARY
    rows, spans = [], []
    for k, w0 in enumerate((100_001, 150_003)):
        assert w0 + W <= N
        lens = rng.integers(W // 2, W, count)
        offs = w0 + (rng.random(count) * (W - lens)).astype(np.int64)
        base = CANARY + k * (W + CANARY)
        rows.append(np.stack([np.full(count, k), offs, lens, offs - w0 + base], axis=1))
        spans.append((int(offs.min()), int((offs + lens).max()), w0, base))
    ranges = np.concatenate(rows).astype(np.uint64)
    ranges = ranges[rng.permutation(ranges.shape[0])]
    want = np.full(size, 0xCC, np.uint8)
    covered = np.zeros(size, bool)
    for m, off, length, dst in ranges.tolist():
        covered[dst:dst + length] = True
    for k, (lo, hi, w0, base) in enumerate(spans):
        want[lo - w0 + base:hi - w0 + base] = data[k][lo:hi]
        assert covered[lo - w0 + base:hi - w0 + base].all()  # (the union is one interval: `want` is exact)
    assert covered.sum() == sum(hi - lo for lo, hi, _, _ in spans)
    d_host = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device_gather_batch(gset, ranges, d_host)  # the yardstick, and the host's count of the tasks
    host = gset.info()
    info = gset.indirect_info(ranges.shape[0], size)
    for m in pair:
        k = ten.kinds[m]
        print("kind", k, "tasks", host["kind_tasks"][k], "grid", info["kind_grid"][k], "waves", info["kind_waves"][k])
        assert host["kind_tasks"][k] > 4 * info["kind_grid"][k] * info["kind_waves"][k], (k, host, info)
    d_dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device_gather_batch_indirect(gset, _device_rows(ranges), d_dst)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert np.array_equal(got, want), _explain(got, want, ranges)
    assert torch.equal(d_dst, d_host)
    _clean(gpu_ctx, gset)


def test_a_quarter_of_a_million_ranges(gpu_ctx, ten):
    """2^18 + 5 ranges of 0 .. 3 bytes over all ten members: 257 rounds of the cut's passes, and a quarter of the ranges has no task"""
    rng = np.random.default_rng(2)
    count = (1 << 18) + 5
    lens = rng.integers(0, 4, count).astype(np.int64)
    members = rng.integers(0, K, count).astype(np.int64)
    offs = rng.integers(0, N_RAW - 3, count).astype(np.int64)
    ends = np.cumsum(lens)
    starts = ends - lens
    total = int(ends[-1])
    want = np.full(total + 2 * CANARY, 0xCC, np.uint8)
    for m in range(K):
        sel = members == m
        n_m = int(lens[sel].sum())
        within = np.arange(n_m) - np.repeat(np.cumsum(lens[sel]) - lens[sel], lens[sel])
        want[CANARY + np.repeat(starts[sel], lens[sel]) + within] = ten.data[m][np.repeat(offs[sel], lens[sel]) + within]
    d_ranges = torch.from_numpy(np.stack([offs, lens, starts + CANARY, members], axis=1)).cuda()
    d_dst = torch.full((want.size,), 0xCC, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device_gather_batch_indirect(ten.gset, d_ranges, d_dst)
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), want)
    _clean(gpu_ctx, ten.gset)


def test_ranges_made_on_the_device(gpu_ctx, ten):
    """the rows come out of torch kernels on the same stream and never visit the host; nothing is synchronised before the gather"""
    rng = np.random.default_rng(23)
    PAGE, LEN, count = 1000, 3001, 500
    pages = rng.integers(0, (N_RAW - LEN) // PAGE, count).astype(np.int64)
    d_dst = torch.full((count * LEN + 2 * CANARY,), 0xCC, dtype=torch.uint8, device="cuda")
    workspace = torch.empty(H.gather_batch_workspace_bytes(K, count), dtype=torch.uint8, device="cuda")
    d_pages = torch.from_numpy(pages).cuda()
    torch.cuda.synchronize()
    # a "page table" lookup on the GPU: the member is the page's number modulo the members, the offset its place in that member
    d_member = d_pages % K
    d_off = d_pages * PAGE + 7
    d_len = torch.full_like(d_off, LEN)
    d_pos = torch.arange(count, dtype=torch.int64, device="cuda") * LEN + CANARY
    d_ranges = torch.stack([d_off, d_len, d_pos, d_member], dim=1).contiguous()
    d_count = (d_pages >= 0).sum().to(torch.int32)  # = count, computed on the device as well
    got_ws = gpu_ctx.decode_device_gather_batch_indirect(ten.gset, d_ranges, d_dst, count=d_count, workspace=workspace)
    assert got_ws is workspace
    torch.cuda.synchronize()
    ranges = np.stack([pages % K, pages * PAGE + 7, np.full(count, LEN), np.arange(count) * LEN + CANARY], axis=1).astype(np.uint64)
    got, want = d_dst.cpu().numpy(), _want(ten.data, ranges, d_dst.numel())
    assert np.array_equal(got, want), _explain(got, want, ranges)
    _clean(gpu_ctx, ten.gset)


def test_graph_replays_read_the_ranges_anew(gpu_ctx, ten):
    """one captured call; before every replay the rows and the count are overwritten in place.  Nothing of a replay may leak into the next:
    not its counters, not its refusal."""
    ROWS, SIZE = 400, 6_000_000
    rng = np.random.default_rng(77)
    d_ranges = _device_rows(np.zeros((0, 4), np.uint64), ROWS)
    d_count = torch.zeros((), dtype=torch.int32, device="cuda")
    d_dst = torch.full((SIZE,), 0xCC, dtype=torch.uint8, device="cuda")
    workspace = torch.empty(H.gather_batch_workspace_bytes(K, ROWS), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            gpu_ctx.decode_device_gather_batch_indirect(ten.gset, d_ranges, d_dst, count=d_count, max_count=ROWS, workspace=workspace, stream=side)
    torch.cuda.synchronize()
    assert bool((d_dst == 0xCC).all())  # capturing runs nothing
    private = next(m for m in range(K) if ten.kinds[m] < 3)
    shared = next(m for m in range(K) if ten.kinds[m] >= 3)
    good = _random_src(rng, ROWS, ten.data)
    replays = (("all kinds", good, 0), ("one private-kind member", _random_src(rng, 150, ten.data, members=[private]), 0),
               ("one shared-kind member", _random_src(rng, 150, ten.data, members=[shared]), 0), ("count 0", [], 0),
               ("a refused row", good[:50] + [(9, N_RAW - 5, 6)] + good[50:100], E_DEVICE), ("all kinds again", good[::-1][:300], 0),
               ("one shared-kind member again", [(shared, 0, 70_000)], 0))
    for name, src, expect in replays:
        ranges, size = _layout(src, "packed")
        assert size <= SIZE and ranges.shape[0] <= ROWS
        d_ranges.copy_(_device_rows(ranges, ROWS))
        d_count.fill_(ranges.shape[0])
        d_dst.fill_(0xCC)
        g.replay()
        torch.cuda.synchronize()
        got = d_dst.cpu().numpy()
        want = _want(ten.data, ranges, SIZE) if expect == 0 else np.full(SIZE, 0xCC, np.uint8)
        assert np.array_equal(got, want), name + ": " + _explain(got, want, ranges)
        assert gpu_ctx.gather_set_refused(ten.gset) == expect, name
        _clean(gpu_ctx, ten.gset)  # (reported once)


def test_device_refusals(gpu_ctx, ten):
    """what only the device can see: nothing is gathered, the set's word reports it once, no member's status moves, the next call is fine"""
    CAP = 20_000
    backing = torch.full((CAP + 2 * CANARY,), 0xCC, dtype=torch.uint8, device="cuda")
    d_dst = backing[CANARY:CANARY + CAP]
    good = [(0, 0, 100, 0), (5, 5000, 3000, 200), (9, N_RAW - 10, 10, 19_990), (3, 70_000, 4097, 4000)]

    def refused(ranges, count=None, max_count=None, reserved=0):
        rows = np.asarray(ranges, np.uint64).reshape(-1, 4)
        d_count = None if count is None else torch.tensor(count, dtype=torch.int32, device="cuda")
        gpu_ctx.decode_device_gather_batch_indirect(ten.gset, _device_rows(rows, max(rows.shape[0], max_count or 0), reserved=reserved), d_dst, count=d_count,
                                                    max_count=max_count)
        torch.cuda.synchronize()
        assert bool((backing == 0xCC).all())
        assert gpu_ctx.gather_set_status(ten.gset) == [0] * K  # no member plan's word is touched
        assert gpu_ctx.gather_set_refused(ten.gset) == E_DEVICE
        assert gpu_ctx.gather_set_refused(ten.gset) == 0
        # ... and the set is as good as before
        gpu_ctx.decode_device_gather_batch_indirect(ten.gset, _device_rows(good), d_dst)
        torch.cuda.synchronize()
        assert np.array_equal(d_dst.cpu().numpy(), _want(ten.data, np.array(good, np.uint64), CAP))
        assert bool((backing[:CANARY] == 0xCC).all()) and bool((backing[CANARY + CAP:] == 0xCC).all())
        _clean(gpu_ctx, ten.gset)
        d_dst.fill_(0xCC)

    refused(good + [(K, 0, 100, 300)])                                 # member == members
    refused([(K, 0, 0, 0)])                                            # ... even for an empty range
    refused(good[:1], reserved=1)                                      # reserved == 1
    refused(good + [(9, 200_000, 10, 300)])                            # an offset the 300,007-byte members have, the 100,003-byte one has not
    refused([(9, N_RAW - 10, 11, 300)])
    refused([(0, 0, 100, 0), (3, 5000, 10_000, 10_001)])               # dst_offset + length past dst_capacity
    refused([(4, 0, 1, CAP)])
    refused([(2, 2 ** 64 - 8, 16, 0)] + good)                          # offset + length wraps
    refused([(2, 8, 2 ** 64 - 4, 0)])
    refused([(2, 0, 16, 2 ** 64 - 8)])                                 # dst_offset + length wraps
    refused(good, count=len(good) + 1, max_count=len(good))            # *d_count = max_count + 1
    refused(good, count=-1, max_count=len(good))                       # (as uint32: 2^32 - 1)
    refused(good + [(1, N, 1, 0)])                                     # a bad row behind good ones: those are not gathered either


def test_host_refusals_leave_the_destination_alone(gpu_ctx, ten):
    d_dst = torch.full((20_000,), 0xCC, dtype=torch.uint8, device="cuda")
    d_ranges = _device_rows([(0, 0, 100, 0), (5, 5000, 3000, 200)])
    d_count = torch.tensor([2, 2], dtype=torch.int32, device="cuda")
    need = H.gather_batch_workspace_bytes(K, 2)
    ws = torch.empty(need + 512, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 256 == 0
    L = gpu_ctx.L

    def idle():
        torch.cuda.synchronize()
        assert bool((d_dst == 0xCC).all())
        _clean(gpu_ctx, ten.gset)

    def refused(gset=ten.gset, workspace=ws, **kw):
        with pytest.raises(H.HsransError) as e:
            gpu_ctx.decode_device_gather_batch_indirect(gset, d_ranges, d_dst, workspace=workspace, **kw)
        assert e.value.code == E_ARG, e.value.code
        idle()

    refused(workspace=ws[:need - 256])                               # a short workspace
    refused(workspace=ws[:4])                                        # a tiny one
    refused(workspace=ws[64:64 + need])                              # a misaligned one
    # misaligned rows and a misaligned count (no tensor starts in the middle of a word: the C entry directly)
    s = torch.cuda.current_stream().cuda_stream
    assert L.hsrans_decode_device_gather_batch_indirect(gpu_ctx.handle, ten.gset.handle, d_ranges.data_ptr() + 4, None, 1, d_dst.data_ptr(), d_dst.numel(), ws.data_ptr(),
                                                        ws.numel(), s) == E_ARG
    assert L.hsrans_decode_device_gather_batch_indirect(gpu_ctx.handle, ten.gset.handle, d_ranges.data_ptr(), d_count.data_ptr() + 2, 2, d_dst.data_ptr(), d_dst.numel(),
                                                        ws.data_ptr(), ws.numel(), s) == E_ARG
    assert L.hsrans_decode_device_gather_batch_indirect(gpu_ctx.handle, ten.gset.handle, None, None, 2, d_dst.data_ptr(), d_dst.numel(), ws.data_ptr(), ws.numel(), s) == E_ARG
    assert L.hsrans_decode_device_gather_batch_indirect(gpu_ctx.handle, ten.gset.handle, d_ranges.data_ptr(), None, 2, None, d_dst.numel(), ws.data_ptr(), ws.numel(), s) == E_ARG
    assert L.hsrans_decode_device_gather_batch_indirect(gpu_ctx.handle, ten.gset.handle, d_ranges.data_ptr(), None, 2, d_dst.data_ptr(), d_dst.numel(), None, ws.numel(), s) == E_ARG
    idle()
    # a set of a second context
    other = H.Context(0)
    so, po = _encode(other, "raw32", 64, 11, ten.data[0][:50_000])
    theirs = other.make_gather_set([other.make_device_plan(po)], [_upload(so)], [so.size])
    refused(gset=theirs)
    assert L.hsrans_gather_set_refused(gpu_ctx.handle, theirs.handle, s) == E_ARG
    # max_count == 0: fine, nothing queued
    gpu_ctx.decode_device_gather_batch_indirect(ten.gset, d_ranges, d_dst, max_count=0, workspace=ws)
    idle()
    # ... and the same arguments with rows in use are fine
    gpu_ctx.decode_device_gather_batch_indirect(ten.gset, d_ranges, d_dst, count=d_count[:1], workspace=ws)
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), _want(ten.data, np.array([(0, 0, 100, 0), (5, 5000, 3000, 200)], np.uint64), 20_000))
    _clean(gpu_ctx, ten.gset)


def test_two_streams_two_workspaces_one_set(gpu_ctx, ten):
    """nothing orders the calls of the two streams: each has its own workspace and destination"""
    rng = np.random.default_rng(13)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    jobs = []
    for k in range(8):
        ranges, size = _layout(_random_src(rng, 400, ten.data), "packed")
        jobs.append((ranges, size, _device_rows(ranges), torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")))
    workspaces = [torch.empty(H.gather_batch_workspace_bytes(K, 400), dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for k, (ranges, size, d_ranges, d_dst) in enumerate(jobs):  # (calls of ONE stream share its workspace: they run in order)
        gpu_ctx.decode_device_gather_batch_indirect(ten.gset, d_ranges, d_dst, workspace=workspaces[k % 2], stream=streams[k % 2])
    torch.cuda.synchronize()
    for ranges, size, d_ranges, d_dst in jobs:
        got, want = d_dst.cpu().numpy(), _want(ten.data, ranges, size)
        assert np.array_equal(got, want), _explain(got, want, ranges)
    _clean(gpu_ctx, ten.gset)


def test_altered_histogram_reaches_its_members_status_only(gpu_ctx):
    """three members with host-built tables, the middle one over a stream whose histogram is not its plan's: the workgroup that serves that
    member's first unit raises that member's status; the others' stay 0, the set's refusal word stays 0, and every member's bytes are right"""
    ms = [_altered_member(gpu_ctx, "raw32", 64, 11, 70 + k) for k in range(3)]
    gset = gpu_ctx.make_gather_set([m[4] for m in ms], [ms[0][2], ms[1][3], ms[2][2]], [m[1] for m in ms])
    assert sum(gset.indirect_info(8, 1 << 16)["kind_members"][3:]) == 3
    ranges, size = _layout([(0, 1000, 4096), (1, 150_001, 4096), (2, N - 4096, 4096), (1, 5, 20_000)], "gaps")
    d_dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device_gather_batch_indirect(gset, _device_rows(ranges), d_dst)
    torch.cuda.synchronize()
    assert gpu_ctx.gather_set_refused(gset) == 0
    codes = gpu_ctx.gather_set_status(gset)
    assert codes == [0, E_DEVICE, 0], codes
    # (member 1's workgroups decode with its plan's own table, which the stream's counts never enter: its bytes are the input's too)
    assert np.array_equal(d_dst.cpu().numpy(), _want([m[0] for m in ms], ranges, size))
    assert gpu_ctx.gather_set_status(gset) == [0, 0, 0] and gpu_ctx.gather_set_refused(gset) == 0


def test_altered_histogram_of_a_member_that_builds_its_table(gpu_ctx):
    """a member whose waves build their table from the stream's counts: the altered count breaks the sum, the wave raises the member's
    status and returns before it writes anything; the member beside it is untouched by that"""
    good, other = _altered_member(gpu_ctx, "raw32", 64, 11, 80), _altered_member(gpu_ctx, "mt", 64, 11, 81)
    gset = gpu_ctx.make_gather_set([good[4], other[4]], [good[2], other[3]], [good[1], other[1]])
    info = gset.indirect_info(8, 1 << 16)
    assert sum(info["kind_members"][:3]) == 1 and sum(info["kind_members"][3:]) == 1, info
    ranges, size = _layout([(0, 1000, 4096), (1, 1000, 4096), (1, 7, 100)], "gaps")  # (member 1's ranges lie in its first block: the altered counts)
    d_dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device_gather_batch_indirect(gset, _device_rows(ranges), d_dst)
    torch.cuda.synchronize()
    assert gpu_ctx.gather_set_refused(gset) == 0
    codes = gpu_ctx.gather_set_status(gset)
    assert codes == [0, E_DEVICE], codes
    assert np.array_equal(d_dst.cpu().numpy(), _want([good[0]], ranges[:1], size))  # member 0's bytes, and 0xCC everywhere else
    assert gpu_ctx.gather_set_status(gset) == [0, 0] and gpu_ctx.gather_set_refused(gset) == 0
