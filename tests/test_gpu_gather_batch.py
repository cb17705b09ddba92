"""hsrans_decode_device_gather_batch on the GPU, bit-exact: byte ranges of MANY streams that stay compressed in device memory land where
the caller wants them, and nowhere else, in one launch per table layout.  Expected bytes are always the encoder's input,
data[member][offset : offset + length].  Every gather writes into a buffer filled with 0xCC that has 4 KiB of canary in front of and
behind the destination (and, in the 'gaps' layout, between the ranges); the WHOLE buffer is compared, so a byte written outside a range —
or taken from the wrong member: every member holds other bytes — fails the case; every member's status must stay 0.
A member whose stream does not carry its plan's histogram has its own tests at the end: that member's status says so, no other's."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth
from test_gpu_gather import _encode, _upload

pytestmark = pytest.mark.gpu

N = 300_007  # a multiple of neither 64 nor 32: every stream ends in a masked group
N_RAW = 100_003
BLOCK = 1 << 16
FILL_BLOCK = 2  # block [2 * 64 KiB, 3 * 64 KiB) holds one symbol only: a single-symbol fill block in the mt_ members
CANARY = 4096
# (container, states, bits); the last one is a raw stream without an index: one chain
MEMBERS = (("raw32", 64, 11), ("raw32", 64, 12), ("raw32", 32, 12), ("rawdev", 64, 14), ("raw32", 64, 15), ("mt", 64, 11), ("mt32", 64, 12), ("mt", 32, 14),
           ("block32", 64, 15), ("raw", 64, 11))


class _Set:
    """the ten members: their data, streams, device plans, the gather set over them and each member's kind (found by asking, not assumed)"""

    def __init__(self, ctx):
        self.data, self.sizes, self.d_streams, self.dplans = [], [], [], []
        for k, (kind, states, bits) in enumerate(MEMBERS):
            n = N_RAW if kind == "raw" else N
            d = (synth.nonstationary(n, seed=40 + k) if states == 64 else synth.enwik8_shaped(n, seed=40 + k)).copy()
            if n > (FILL_BLOCK + 1) * BLOCK:
                d[FILL_BLOCK * BLOCK:(FILL_BLOCK + 1) * BLOCK] = 0x41 + k
            s, plan = _encode(ctx, kind, states, bits, d)
            self.data.append(d)
            self.sizes.append(s.size)
            self.d_streams.append(_upload(s))
            self.dplans.append(ctx.make_device_plan(plan))
        assert H.plan_chain_count(plan) == 1  # the last member: a raw stream without an index
        self.gset = ctx.make_gather_set(self.dplans, self.d_streams, self.sizes)
        self.kinds = []
        scratch = torch.zeros(64, dtype=torch.uint8, device="cuda")
        for m in range(len(MEMBERS)):
            ctx.decode_device_gather_batch(self.gset, [(m, 0, 1, 0)], scratch)
            info = self.gset.info()
            assert info["launches"] == 1 and sum(info["kind_tasks"]) == 1
            self.kinds.append(info["kind_tasks"].index(1))
        torch.cuda.synchronize()
        assert ctx.gather_set_status(self.gset) == [0] * len(MEMBERS)


@pytest.fixture(scope="module")
def ten(gpu_ctx):
    return _Set(gpu_ctx)


def _layout(src, packing, base_align=0):  # (test_gpu_gather's has no member column)
    """(member, offset, length) triples -> (N, 4) rows (member, offset, length, dst_offset) and the buffer size.  packing: 'packed' = back to
    back behind the front canary (most destinations misaligned against their source); 'aligned' = every dst_offset congruent to its offset
    modulo 4 (gaps of < 4 bytes); 'gaps' = 4 KiB of canary between ranges."""
    rows, pos = [], CANARY
    for m, off, length in src:
        if packing == "aligned":
            pos += (off - pos - base_align) % 4
        rows.append((m, off, length, pos))
        pos += length + (CANARY if packing == "gaps" else 0)
    return np.array(rows, np.uint64).reshape(-1, 4), pos + CANARY


def _want(data, ranges, size):
    want = np.full(size, 0xCC, np.uint8)
    for m, off, length, dst in ranges.tolist():
        want[dst:dst + length] = data[m][off:off + length]
    return want


def _gather_and_check(ctx, gset, data, src, packing="packed", misalign=0):
    """one batch gather of the (member, offset, length) triples `src`; compares the whole destination buffer, canaries included"""
    ranges, size = _layout(src, packing, base_align=misalign)
    want = _want(data, ranges, size)
    backing = torch.full((size + 16,), 0xCC, dtype=torch.uint8, device="cuda")
    d_dst = backing[misalign:misalign + size]  # (misalign: a destination base that is not even 2-byte aligned)
    ctx.decode_device_gather_batch(gset, ranges, d_dst)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    if not np.array_equal(got, want):
        bad = int(np.argmax(got != want))
        row = int(np.searchsorted(ranges[:, 3], bad, side="right")) - 1
        raise AssertionError(f"first wrong byte at destination {bad} (of {size}), range {row}: {ranges[max(row, 0)].tolist()}, got {got[bad]} want {want[bad]}")
    whole = backing.cpu().numpy()
    assert np.all(whole[size + misalign:] == 0xCC) and np.all(whole[:misalign] == 0xCC)
    assert ctx.gather_set_status(gset) == [0] * len(gset.dplans)
    return ranges, d_dst


def _random_src(rng, count, data, members=None):
    members = list(range(len(data))) if members is None else members
    src = []
    for _ in range(count):
        m = int(rng.choice(members))
        n = data[m].size
        length = min(int(2.0 ** rng.uniform(0, 16)), n)  # 1 B .. 64 KiB, every magnitude alike
        src.append((m, int(rng.integers(0, n - length + 1)), length))
    return src


def _explicit_src(m, n, states):
    b0 = BLOCK  # a block boundary (mt_) and a checkpoint boundary
    f0, f1 = FILL_BLOCK * BLOCK, (FILL_BLOCK + 1) * BLOCK
    src = [
        (0, 1), (0, 5000),                                                              # offset 0
        (n - 1, 1), (n - 17, 17), (n - 30_001, 30_001),                                 # ending at decoded_len, inside the masked tail
        (b0 - 1, 2), (b0 - 1, 4099), (b0, states), (b0 - states, 2 * states),           # across a block boundary
        (77_777, 9000), (77_777, 9000),                                                 # the same source twice
        (50_003, 0),                                                                    # an empty range among the others
    ]
    if n > f1:
        src += [(f0 + 100, 1), (f0 + 3, 30_001), (f0, BLOCK), (f0 - 5000, 12_000), (f1 - 11, 6000)]  # inside and across the fill block
    return [(m, off, length) for off, length in src]


def _all_explicit(ten):
    return [t for m, (_, states, _) in enumerate(MEMBERS) for t in _explicit_src(m, ten.data[m].size, states)]


def test_kinds_present(ten):
    info = ten.gset.info()
    assert info["members"] == len(MEMBERS) and sum(info["kind_members"]) == len(MEMBERS)
    assert sum(1 for k in range(3) if info["kind_members"][k]) >= 2, info      # at least two kinds with a table per wave ...
    assert sum(1 for k in range(3, 6) if info["kind_members"][k]) >= 2, info   # ... and two with one per workgroup
    print("kinds of the ten members:", ten.kinds)  # (which kind a plan gets is gather_shape's decision: reported, not asserted)
    for k in range(6):
        assert info["kind_members"][k] == ten.kinds.count(k)


def test_whole_buffer(gpu_ctx, ten):
    rng = np.random.default_rng(2024)
    src = _random_src(rng, 600, ten.data)
    _gather_and_check(gpu_ctx, ten.gset, ten.data, src + _all_explicit(ten), "packed")     # 600 random ranges and the explicit edges, back to back
    _gather_and_check(gpu_ctx, ten.gset, ten.data, _all_explicit(ten), "gaps")             # the explicit ones, canary between them
    _gather_and_check(gpu_ctx, ten.gset, ten.data, _all_explicit(ten) + src[:100], "packed", misalign=1)
    _gather_and_check(gpu_ctx, ten.gset, ten.data, src[:300] + _all_explicit(ten), "aligned")  # the word-store path
    _gather_and_check(gpu_ctx, ten.gset, ten.data, src[:300], "aligned", misalign=1)


def test_equals_the_single_calls(gpu_ctx, ten):
    rng = np.random.default_rng(7)
    src = _random_src(rng, 600, ten.data) + _all_explicit(ten)
    ranges, d_batch = _gather_and_check(gpu_ctx, ten.gset, ten.data, src, "packed")
    d_single = torch.full_like(d_batch, 0xCC)
    for m in range(len(MEMBERS)):
        mine = ranges[ranges[:, 0] == m][:, 1:]
        gpu_ctx.decode_device_gather(ten.dplans[m], ten.d_streams[m], mine, d_single, stream_length=ten.sizes[m])
    torch.cuda.synchronize()
    assert torch.equal(d_batch, d_single)
    for m in range(len(MEMBERS)):
        assert gpu_ctx.status(ten.dplans[m]) == 0  # a member stays usable alone


def test_members_used_unevenly(gpu_ctx, ten):
    rng = np.random.default_rng(11)
    for m in (0, 5, 8, 9):  # all ranges on one member
        _gather_and_check(gpu_ctx, ten.gset, ten.data, _random_src(rng, 120, ten.data, members=[m]), "packed")
    # one range on each member: a shared-kind workgroup is then mostly padding
    _gather_and_check(gpu_ctx, ten.gset, ten.data, [(m, 1000 + 37 * m, 333) for m in range(len(MEMBERS))], "gaps")
    info = ten.gset.info()
    for k in range(3, 6):
        assert info["kind_entries"][k] == info["kind_waves"][k] * ten.kinds.count(k) and info["kind_tasks"][k] == ten.kinds.count(k)
    # a member of a shared kind with 3 * waves + 1 tasks: its run ends in a padded workgroup
    m = next(m for m in range(len(MEMBERS)) if ten.kinds[m] >= 3 and MEMBERS[m][0] == "raw32")
    kind, seg = ten.kinds[m], 4096  # (a checkpoint every 32 groups: L is the 4 KiB floor)
    _gather_and_check(gpu_ctx, ten.gset, ten.data, [(m, 0, 13 * seg)], "packed")
    waves = ten.gset.info()["kind_waves"][kind]
    assert waves in (1, 2, 4, 8, 16) and (3 * waves + 1) * seg < N
    _gather_and_check(gpu_ctx, ten.gset, ten.data, [(m, 0, (3 * waves + 1) * seg), ((m + 1) % 10, 5, 70)], "packed", misalign=1)
    info = ten.gset.info()
    assert info["kind_waves"][kind] == waves and info["kind_tasks"][kind] - (ten.kinds[(m + 1) % 10] == kind) == 3 * waves + 1
    assert info["kind_entries"][kind] == 4 * waves + waves * (ten.kinds[(m + 1) % 10] == kind)
    # a set of one member
    for m in (3, 6):
        one = gpu_ctx.make_gather_set([ten.dplans[m]], [ten.d_streams[m]], [ten.sizes[m]])
        src = [(0, off, length) for _, off, length in _random_src(rng, 60, ten.data, members=[m]) + _explicit_src(m, ten.data[m].size, MEMBERS[m][1])]
        _gather_and_check(gpu_ctx, one, [ten.data[m]], src, "packed")
        assert one.info()["launches"] == 1
    # the same plan and stream as two members
    for m in (1, 7):
        twice = gpu_ctx.make_gather_set([ten.dplans[m]] * 2, [ten.d_streams[m]] * 2, [ten.sizes[m]] * 2)
        src = [(int(rng.integers(0, 2)), off, length) for _, off, length in _random_src(rng, 80, ten.data, members=[m])]
        _gather_and_check(gpu_ctx, twice, [ten.data[m]] * 2, src, "packed")
    assert gpu_ctx.gather_set_status(ten.gset) == [0] * len(MEMBERS)  # the plans were members of other sets meanwhile


def test_one_launch_per_kind(gpu_ctx, ten):
    rng = np.random.default_rng(13)
    _gather_and_check(gpu_ctx, ten.gset, ten.data, _random_src(rng, 300, ten.data), "packed")
    info = ten.gset.info()
    assert info["launches"] == len(set(ten.kinds)) <= 6
    assert info["launches"] == sum(1 for t in info["kind_tasks"] if t)
    for k in range(6):
        assert (info["kind_tasks"][k] != 0) == (k in ten.kinds)
        if info["kind_tasks"][k]:
            assert info["kind_grid"][k] * info["kind_waves"][k] >= info["kind_entries"][k] >= info["kind_tasks"][k] and info["kind_lds_bytes"][k] > 0
    for kind in sorted(set(ten.kinds)):  # the ranges touch members of one kind only: one launch
        _gather_and_check(gpu_ctx, ten.gset, ten.data, _random_src(rng, 60, ten.data, members=[m for m in range(len(MEMBERS)) if ten.kinds[m] == kind]), "packed")
        info = ten.gset.info()
        assert info["launches"] == 1 and [k for k in range(6) if info["kind_tasks"][k]] == [kind]
    two = sorted(set(ten.kinds))[:2]
    _gather_and_check(gpu_ctx, ten.gset, ten.data, _random_src(rng, 60, ten.data, members=[m for m in range(len(MEMBERS)) if ten.kinds[m] in two]), "packed")
    assert ten.gset.info()["launches"] == 2


def test_refusals_leave_the_destination_alone(gpu_ctx, ten):
    d_dst = torch.full((20_000,), 0xCC, dtype=torch.uint8, device="cuda")
    L = H.load_library()

    def untouched():
        torch.cuda.synchronize()
        assert bool((d_dst == 0xCC).all())

    def refused(ranges, code=2):
        with pytest.raises(H.HsransError) as e:
            gpu_ctx.decode_device_gather_batch(ten.gset, ranges, d_dst)
        assert e.value.code == code, (e.value.code, code)
        untouched()

    good = (0, 0, 100, 0)
    refused([good, (len(MEMBERS), 0, 100, 200)])                      # member == members
    refused([good, (4, N - 10, 11, 200)])                             # one byte beyond a member's decoded length
    refused([good, (9, N_RAW - 10, 11, 200)])
    refused([good, (9, N_RAW + 1, 0, 200)])
    refused([good, (3, 5000, 10_000, 10_001)])                        # dst_offset + length == dst_capacity + 1
    refused([good, (3, 0, 1, 20_000)])
    from hypersonic_rans_amd import api
    rows = (api.MemberRange * 2)(api.MemberRange(0, 100, 0, 0, 0), api.MemberRange(0, 100, 200, 1, 1))  # reserved != 0
    s = torch.cuda.current_stream()
    assert L.hsrans_decode_device_gather_batch(gpu_ctx.handle, ten.gset.handle, rows, 2, d_dst.data_ptr(), d_dst.numel(), s.cuda_stream) == 2
    untouched()
    assert L.hsrans_decode_device_gather_batch(gpu_ctx.handle, ten.gset.handle, None, 2, d_dst.data_ptr(), d_dst.numel(), s.cuda_stream) == 2
    # nothing to do: fine, nothing launched, nothing written
    gpu_ctx.decode_device_gather_batch(ten.gset, np.zeros((0, 4), np.uint64), d_dst)
    assert ten.gset.info()["launches"] == 0
    gpu_ctx.decode_device_gather_batch(ten.gset, [(2, 5, 0, 0), (9, N_RAW, 0, 20_000), (0, N, 0, 7)], d_dst)
    assert ten.gset.info()["launches"] == 0
    untouched()
    assert gpu_ctx.gather_set_status(ten.gset) == [0] * len(MEMBERS)
    # create: a block_ plan without checkpoints has no entry points; a stream length off by one
    sb, pb = _encode(gpu_ctx, "block", 64, 11, ten.data[0])
    for dplans, streams, lengths, code in (([ten.dplans[0], gpu_ctx.make_device_plan(pb)], [ten.d_streams[0], _upload(sb)], [ten.sizes[0], sb.size], 3),
                                           ([ten.dplans[0], ten.dplans[1]], [ten.d_streams[0], ten.d_streams[1]], [ten.sizes[0], ten.sizes[1] - 1], 3),
                                           ([ten.dplans[0], ten.dplans[1]], [ten.d_streams[0], ten.d_streams[1]], [ten.sizes[0] + 1, ten.sizes[1]], 3),
                                           ([ten.dplans[0]], [ten.d_streams[0][8:]], [ten.sizes[0]], 2)):      # a misaligned stream
        with pytest.raises(H.HsransError) as e:
            gpu_ctx.make_gather_set(dplans, streams, lengths)
        assert e.value.code == code, (e.value.code, code)


def test_two_sets_on_two_streams(gpu_ctx, ten):
    """two sets of one context, their gathers queued alternately on two torch streams, one synchronise: the task lists go through the
    context's one buffer, and single gathers of a member run in between"""
    first = ten.gset
    order = [7, 2, 9, 0, 4]
    second = gpu_ctx.make_gather_set([ten.dplans[m] for m in order], [ten.d_streams[m] for m in order], [ten.sizes[m] for m in order])
    second_data = [ten.data[m] for m in order]
    rng = np.random.default_rng(17)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    jobs = []
    for k in range(8):
        gset, data = (first, ten.data) if k % 2 == 0 else (second, second_data)
        ranges, size = _layout(_random_src(rng, 400, data), "packed")
        jobs.append((gset, data, ranges, size, torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")))
    single_ranges = np.array([(100, 50_000, 0)], np.uint64)
    d_single = torch.full((50_000,), 0xCC, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for k, (gset, data, ranges, size, d_dst) in enumerate(jobs):
        scratch = ranges.copy()
        gpu_ctx.decode_device_gather_batch(gset, scratch, d_dst, stream=streams[k % 2])
        scratch[:] = 0  # `ranges` is read before the call returns: the caller may reuse it
        if k == 3:
            gpu_ctx.decode_device_gather(ten.dplans[0], ten.d_streams[0], single_ranges, d_single, stream_length=ten.sizes[0], stream=streams[0])
    torch.cuda.synchronize()
    for gset, data, ranges, size, d_dst in jobs:
        assert np.array_equal(d_dst.cpu().numpy(), _want(data, ranges, size))
    assert np.array_equal(d_single.cpu().numpy(), ten.data[0][100:50_100])
    assert gpu_ctx.gather_set_status(first) == [0] * len(MEMBERS) and gpu_ctx.gather_set_status(second) == [0] * len(order)


def _first_hist_off(plan):
    """where the stream keeps the counts the plan's first piece decodes with"""
    return int(H.api.plan_tables(plan)[2][0]["hist_off"])


def _altered_member(ctx, kind, states, bits, seed):
    """(data, stream length, the good device copy of the stream, one with a count of its first histogram flipped, device plan)"""
    data = synth.nonstationary(N, seed=seed).copy()
    s, plan = _encode(ctx, kind, states, bits, data)
    bad = _upload(s)
    bad[_first_hist_off(plan) + 40] ^= 0x5A
    return data, s.size, _upload(s), bad, ctx.make_device_plan(plan)


def test_altered_histogram_reaches_its_members_status_only(gpu_ctx):
    """three members with host-built tables, the middle one over a stream whose histogram is not its plan's: the first workgroup of that
    member's run raises that member's status, reported once; the others' statuses stay 0 and every member's bytes are right"""
    ms = [_altered_member(gpu_ctx, "raw32", 64, 11, 70 + k) for k in range(3)]
    gset = gpu_ctx.make_gather_set([m[4] for m in ms], [ms[0][2], ms[1][3], ms[2][2]], [m[1] for m in ms])
    assert sum(gset.info()["kind_members"][3:]) == 3
    ranges, size = _layout([(0, 1000, 4096), (1, 150_001, 4096), (2, N - 4096, 4096)], "gaps")
    d_dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device_gather_batch(gset, ranges, d_dst)
    torch.cuda.synchronize()
    codes = gpu_ctx.gather_set_status(gset)
    assert codes[0] == 0 and codes[2] == 0 and codes[1] != 0, codes
    # (member 1's workgroups decode with its plan's own table, which the stream's counts never enter: its bytes are the input's too)
    assert np.array_equal(d_dst.cpu().numpy(), _want([m[0] for m in ms], ranges, size))
    assert gpu_ctx.gather_set_status(gset) == [0, 0, 0]  # (reported once, then cleared, like hsrans_dplan_status)


def test_altered_histogram_of_a_member_that_builds_its_table(gpu_ctx):
    """a member whose waves build their table from the stream's counts (MEMBERS' mt_ 64 x 11): the altered count breaks the sum, the wave
    raises the member's status and returns before it writes anything; the member beside it is untouched by that"""
    good, other = _altered_member(gpu_ctx, "raw32", 64, 11, 80), _altered_member(gpu_ctx, "mt", 64, 11, 81)
    gset = gpu_ctx.make_gather_set([good[4], other[4]], [good[2], other[3]], [good[1], other[1]])
    info = gset.info()
    assert sum(info["kind_members"][:3]) == 1 and sum(info["kind_members"][3:]) == 1, info
    ranges, size = _layout([(0, 1000, 4096), (1, 1000, 4096)], "gaps")  # (member 1's range lies in its first block: the altered counts)
    d_dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device_gather_batch(gset, ranges, d_dst)
    torch.cuda.synchronize()
    codes = gpu_ctx.gather_set_status(gset)
    assert codes[0] == 0 and codes[1] != 0, codes
    assert np.array_equal(d_dst.cpu().numpy(), _want([good[0]], ranges[:1], size))  # member 0's bytes, and 0xCC everywhere else
    assert gpu_ctx.gather_set_status(gset) == [0, 0]
