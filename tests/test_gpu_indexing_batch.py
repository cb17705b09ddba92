"""hsrans_decode_device_indexing_batch: the first decode of many streams in one call.  Every member — block_ walk plans and mt_ base plans,
32 and 64 states, 10-15 bits, different intervals, the reference's own block ends — gets what hsrans_decode_device_indexing gives it alone:
the bytes (against the CPU oracle), the plan blob (against hsrans_index_build and against the single call), the launch.  The number of
kernels launched does not grow with the number of members; a member that fails on the device fails alone; what is refused is refused
before anything is written; both assembly paths agree."""
import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth
from oracle_lib import BLOCK, MT

pytestmark = pytest.mark.gpu

CANARY = 64


@pytest.fixture(scope="module")
def zipf():
    return synth.enwik8_shaped(1 << 20, seed=11)


@pytest.fixture(scope="module")
def nonstat():
    return synth.nonstationary(3_000_000)


def _runs(zipf):
    """tests/test_gpu_block_indexing.py's: text with long runs of one byte in it — single-symbol blocks between coded ones and next to each other"""
    return np.concatenate([zipf[:100_000], np.full(300_000, 7, np.uint8), zipf[100_000:200_000], np.full(150_000, 9, np.uint8), np.full(150_000, 3, np.uint8),
                           zipf[200_000:300_037]])


# (container, states, bits, data, length, block size (None: the reference's encoder), interval)
SPECS = ((H.BLOCK, 64, 11, "zipf", 300_000, 65536, 32),       # baseline
         (H.BLOCK, 32, 11, "zipf", 300_000, 65536, 4),        # hundreds of chains per block
         (H.BLOCK, 64, 13, "nonstat", 1_000_003, 32768, 32),  # 3-byte tail
         (H.BLOCK, 64, 11, "zipf", 40_000, 65536, 32),        # one coded block: shared_hist == 1
         (H.BLOCK, 64, 12, "runs", 900_037, 65536, 32),       # fill blocks, alone and in runs; the 12-bit layout
         (H.BLOCK, 64, 15, "zipf", 300_000, 65536, 64),       # widest table
         (H.MT, 64, 11, "zipf", 300_000, 65536, 32),          # mt_ member
         (H.MT, 32, 13, "nonstat", 1_000_003, 65536, 8),      # mt_, 32 states
         (H.BLOCK, 64, 11, "zipf", 1 << 20, None, 64),        # the reference's block ends
         (H.BLOCK, 32, 13, "nonstat", 3_000_000, None, 64))


class Case:
    def __init__(self, spec, s, want, want_plan):
        self.container, self.states, self.bits, _, self.n, _, self.interval = spec
        self.s, self.want, self.want_plan = s, want, want_plan


@pytest.fixture(scope="module")
def cases(gpu_ctx, oracle, ref, zipf, nonstat):
    """per member of the mixed batch: its stream, the oracle's decode of it and hsrans_index_build's blob — computed once, never changed"""
    out = []
    for spec in SPECS:
        container, states, bits, src, n, block, interval = spec
        d = (zipf if src == "zipf" else nonstat if src == "nonstat" else _runs(zipf))[:n]
        s = ref.encode(BLOCK, states, bits, d) if block is None else H.encode(container, states, bits, d, block_size=block)
        r, want = oracle.decode(BLOCK if container == H.BLOCK else MT, states, bits, s, n)
        assert r == n and np.array_equal(want, d)
        want.setflags(write=False)
        out.append(Case(spec, s, want, gpu_ctx.index_build(container, states, bits, s, interval)))
    return out


def _upload(s):
    import torch

    return torch.from_numpy(np.concatenate([s, np.zeros((-s.size) % 16, np.uint8)])).cuda()


def _member(ctx, c, d_in=None):
    """(base plan, d_stream, the output with its canary behind it)"""
    import torch

    d_in = _upload(c.s) if d_in is None else d_in
    base = ctx.make_device_plan_from_stream(c.container, c.states, c.bits, d_in, c.s.size, c.n)
    out = torch.full((c.n + CANARY,), 0xCC, dtype=torch.uint8, device="cuda")
    return base, d_in, out


def _batch(ctx, cs, stats=None):
    ms = [_member(ctx, c) for c in cs]
    plans = ctx.decode_device_indexing_batch([(base, d_in, out[:c.n], c.interval, c.s.size) for c, (base, d_in, out) in zip(cs, ms)], stats=stats)
    return ms, plans


def _check_member(ctx, c, base, d_in, out, indexed, single=True):
    import torch

    got = out.cpu().numpy()
    assert np.array_equal(got[:c.n], c.want) and bool((got[c.n:] == 0xCC).all())
    blob = ctx.read_device_plan(indexed, capacity=c.want_plan.size + 4096)
    assert np.array_equal(blob, c.want_plan)
    again = torch.zeros(c.n, dtype=torch.uint8, device="cuda")
    ctx.decode_device(indexed, d_in, again, stream_length=c.s.size)
    assert ctx.status(indexed) == 0 and np.array_equal(again.cpu().numpy(), c.want)
    if single:  # the single call on the same base plan and stream: the same blob, the same launch
        again.zero_()
        alone = ctx.decode_device_indexing(base, d_in, again, c.interval, stream_length=c.s.size)
        assert np.array_equal(ctx.read_device_plan(alone, capacity=c.want_plan.size + 4096), blob)
        assert np.array_equal(again.cpu().numpy(), c.want)
        again.zero_()
        ctx.decode_device(alone, d_in, again, stream_length=c.s.size)
        assert alone.launch_info() == indexed.launch_info() and np.array_equal(again.cpu().numpy(), c.want)
    twin = ctx.make_device_plan(c.want_plan)  # the same blob through the host's group builder: the same launch
    again.zero_()
    ctx.decode_device(twin, d_in, again, stream_length=c.s.size)
    assert ctx.status(twin) == 0 and np.array_equal(again.cpu().numpy(), c.want)
    print("launch of the batch's plan", indexed.launch_info(), "of the hsrans_index_build blob", twin.launch_info())
    assert indexed.launch_info() == twin.launch_info()
    return blob


@pytest.fixture(scope="module")
def mixed(gpu_ctx, cases):
    """the ONE call with the ten members"""
    stats = {}
    ms, plans = _batch(gpu_ctx, cases, stats)
    return ms, plans, stats


def test_the_mixed_batch_is_one_call_of_at_most_seven_launches(mixed):
    _, plans, stats = mixed
    print(stats)
    assert len(plans) == len(SPECS) == 10 and all(p is not None for p in plans)
    assert stats["walk_members"] == 8 and stats["mt_members"] == 2 and 1 <= stats["launches"] <= 7


@pytest.mark.parametrize("k", range(len(SPECS)))
def test_the_mixed_batch(gpu_ctx, cases, mixed, k):
    """Member k of the one call (the table above): bytes, blob, status, the single call's plan and launch, and the launch of the plan
    hsrans_dplan_create makes from the hsrans_index_build blob (k = 7, mt_ in 16 blocks with 256 chains each at interval 8, is the member
    whose blocks are cut into 4 parts by their own chain counts where the average checkpoints per block would give 3)."""
    ms, plans, _ = mixed
    base, d_in, out = ms[k]
    _check_member(gpu_ctx, cases[k], base, d_in, out, plans[k])
    assert gpu_ctx.status(base) == 0
    if k == 3:
        hdr, _, _ = H.api.plan_tables(cases[3].want_plan)
        assert hdr["shared_hist"] == 1 and hdr["n_chains"] > 1


def test_launch_count_does_not_grow_with_the_members(gpu_ctx, cases):
    c = cases[0]
    launches, blobs = [], []
    for k in (4, 24):
        stats = {}
        ms, plans = _batch(gpu_ctx, [c] * k, stats)  # (every member its own upload, base plan and output)
        assert len({m[1].data_ptr() for m in ms}) == k and len({m[2].data_ptr() for m in ms}) == k
        assert stats["walk_members"] == k and stats["mt_members"] == 0 and stats["tasks"] == k
        launches.append(stats["launches"])
        for (base, d_in, out), indexed in zip(ms, plans):
            blobs.append(_check_member(gpu_ctx, c, base, d_in, out, indexed, single=False))
    assert launches[0] == launches[1] and 1 <= launches[0] <= 7, launches
    assert all(np.array_equal(b, blobs[0]) for b in blobs)


@pytest.mark.parametrize("states", (32, 64))
def test_a_member_that_fails_fails_alone(gpu_ctx, zipf, cases, states):
    import torch

    good = cases[0]
    # tests/test_gpu_block_indexing.py's: 196 blocks against room for 64; one count of the second block's histogram flipped
    d_many = zipf[:200_000]
    s_many = H.encode(H.BLOCK, states, 11, d_many, block_size=1024, out_capacity=400_000)
    d_flip = zipf[:300_000]
    s_flip = H.encode(H.BLOCK, states, 11, d_flip, block_size=65536)
    _, _, pc = H.api.plan_tables(gpu_ctx.index_build(H.BLOCK, states, 11, s_flip, 32))
    hists = sorted(set(int(h) for h in pc[(pc["flags"] & 2) == 0]["hist_off"]))
    assert len(hists) > 2
    bad = s_flip.copy()
    bad[hists[1] + 2] ^= 0x40
    b0, in0, out0 = _member(gpu_ctx, good)
    in1 = _upload(s_many)
    b1 = gpu_ctx.make_device_plan_from_stream(H.BLOCK, states, 11, in1, s_many.size, d_many.size)
    out1 = torch.zeros(d_many.size, dtype=torch.uint8, device="cuda")
    in2, in2_bad = _upload(s_flip), _upload(bad)
    b2 = gpu_ctx.make_device_plan_from_stream(H.BLOCK, states, 11, in2, s_flip.size, d_flip.size)
    out2 = torch.zeros(d_flip.size, dtype=torch.uint8, device="cuda")
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.decode_device_indexing_batch([(b0, in0, out0[:good.n], good.interval, good.s.size), (b1, in1, out1, 32, s_many.size), (b2, in2_bad, out2, 32, bad.size)])
    err = e.value
    assert err.codes == [0, 3, 5] and err.code == 3
    assert err.plans[0] is not None and err.plans[1] is None and err.plans[2] is None
    _check_member(gpu_ctx, good, b0, in0, out0, err.plans[0], single=False)
    assert np.array_equal(out1.cpu().numpy(), d_many)  # the walk itself went through
    for base, d_in, size, out, d in ((b0, in0, good.s.size, out0[:good.n], good.want), (b1, in1, s_many.size, out1, d_many), (b2, in2, s_flip.size, out2, d_flip)):
        assert gpu_ctx.status(base) == 0
        out.zero_()
        gpu_ctx.decode_device(base, d_in, out, stream_length=size)
        assert gpu_ctx.status(base) == 0 and np.array_equal(out.cpu().numpy(), d)


def test_refusals_write_nothing(gpu_ctx, zipf, cases):
    import torch

    c = cases[0]
    a, b = _member(gpu_ctx, c), _member(gpu_ctx, c)
    spare = _member(gpu_ctx, c)[2]
    indexed = gpu_ctx.decode_device_indexing(_member(gpu_ctx, c)[0], a[1], spare[:c.n], c.interval, stream_length=c.s.size)
    spare.fill_(0xCC)
    d_raw = zipf[:300_000]
    s_raw = H.encode(H.RAW, 64, 11, d_raw)
    raw, in_raw = gpu_ctx.make_device_plan(H.plan_build(H.RAW, 64, 11, s_raw)), _upload(s_raw)
    # one buffer that holds member a's stream at its front and, from byte 16 on, what would be member b's output: a write over a read
    in_a = _upload(c.s)
    shared = torch.full((16 + c.n + CANARY,), 0xCC, dtype=torch.uint8, device="cuda")
    assert in_a.numel() > 16 and in_a.numel() < shared.numel()
    shared[:in_a.numel()] = in_a
    shared_before = shared.clone()

    def m(base, d_in, out, interval=c.interval, length=c.s.size):
        return (base, d_in, out[:c.n], interval, length)

    for what, members in (("one dplan named twice", [m(a[0], a[1], a[2]), m(a[0], a[1], b[2])]),
                          ("two members sharing an output", [m(a[0], a[1], a[2]), m(b[0], b[1], a[2])]),
                          ("an interval of 6", [m(a[0], a[1], a[2]), m(b[0], b[1], b[2], interval=6)]),
                          ("a member that is already indexed", [m(a[0], a[1], a[2]), m(indexed, b[1], b[2])]),
                          ("a raw base plan", [m(a[0], a[1], a[2]), (raw, in_raw, spare[:d_raw.size], 32, s_raw.size)]),
                          ("an output lying over another member's stream", [m(a[0], shared[:in_a.numel()], a[2]), m(b[0], b[1], shared[16:])])):
        stats = {}
        with pytest.raises(H.HsransError) as e:
            gpu_ctx.decode_device_indexing_batch(members, stats=stats)
        assert e.value.code == 2 and e.value.codes == [2, 2] and e.value.plans == [None, None], what
        assert stats["launches"] == 0, what
        for out in (a[2], b[2], spare):
            assert bool((out == 0xCC).all()), what
        assert torch.equal(shared, shared_before), what
    # ... and the same members, well formed, go through
    plans = gpu_ctx.decode_device_indexing_batch([m(a[0], a[1], a[2]), m(b[0], b[1], b[2])])
    for (base, d_in, out), p in zip((a, b), plans):
        _check_member(gpu_ctx, c, base, d_in, out, p, single=False)
    # ... and so do two members, each with a base plan and an output of its own, that read ONE uploaded stream: reads may share
    p, q = _member(gpu_ctx, c, in_a), _member(gpu_ctx, c, in_a)
    assert p[1].data_ptr() == q[1].data_ptr() and p[0] is not q[0] and p[2].data_ptr() != q[2].data_ptr()
    plans = gpu_ctx.decode_device_indexing_batch([m(p[0], in_a, p[2]), m(q[0], in_a, q[2])])
    for (base, d_in, out), indexed in zip((p, q), plans):
        _check_member(gpu_ctx, c, base, d_in, out, indexed, single=False)


def test_both_assembly_paths(cases, monkeypatch):
    """HSRANS_INDEX_ASSEMBLE_ON_HOST=1: the single call's body member by member — the same blobs, the same bytes, no batch launch"""
    monkeypatch.setenv("HSRANS_INDEX_ASSEMBLE_ON_HOST", "1")
    ctx = H.Context(0)  # (the switch is read when the context is made)
    cs = [cases[0], cases[4], cases[6]]
    stats = {}
    ms, plans = _batch(ctx, cs, stats)
    assert stats["launches"] == 0 and stats["walk_members"] == 2 and stats["mt_members"] == 1
    for c, (base, d_in, out), indexed in zip(cs, ms, plans):
        _check_member(ctx, c, base, d_in, out, indexed, single=False)
