"""hsrans_encode_device_batch: many raw / mt_ streams encoded on the GPU by one launch per kernel kind.  Every member against its
single call (hsrans_encode_device_raw / hsrans_encode_device: stream bytes, length, device plan) and the host encoder; plans decoded
back through the batch decoder; refusals that launch nothing; a failing member that leaves the others alone; launch counts that do not
grow with the member count; context reuse."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth
from hypersonic_rans_amd.api import hist_from_counts

pytestmark = pytest.mark.gpu

RAW, MT = H.RAW, H.MT
E_ARG, E_DEVICE = 2, 5
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def corpus():
    return synth.enwik8_shaped(4 << 20, seed=23)


def _dev(data):
    return torch.from_numpy(np.ascontiguousarray(data)).cuda()


def _out(container, states, n, extra=0):
    return torch.full((H.capacity(container, states, n) + extra,), SENTINEL, dtype=torch.uint8, device="cuda")


def _single(ctx, container, states, bits, d_in, opts, want_plan):
    """The member's single call: (stream bytes, DevicePlan or None)."""
    d_out = _out(container, states, d_in.numel())
    if container == RAW:
        r = ctx.encode_device_raw(states, bits, d_in, d_out, hist=opts.get("hist"), index_interval=opts.get("index_interval", 0),
                                  index_groups=opts.get("index_groups"), want_device_plan=want_plan)
        n, p = (r if want_plan else (r, None))
        if p is not None and not p.handle.value:  # (no index: the single call returns no plan)
            p = None
    else:
        r = ctx.encode_device(MT, states, bits, d_in, d_out, block_size=opts["block_size"], index_interval=opts.get("index_interval", 0), want_plan=want_plan)
        n, p = (r if want_plan else (r, None))
    return d_out[:n].cpu().numpy(), p


def _host(container, states, bits, data, opts):
    if container == RAW:
        return H.encode(RAW, states, bits, data, hist=opts.get("hist"))
    return H.encode(MT, states, bits, data, block_size=opts["block_size"], independent_blocks=True)


def _plan_bytes(ctx, p):
    return None if p is None else ctx.read_device_plan(p)


def _run(ctx, specs, corpus, want_plans=True, stats=None):
    """specs: (container, states, bits, offset, length, opts).  Returns (members, lengths, plans, outputs)."""
    members, ins, outs = [], [], []
    for container, states, bits, off, n, opts in specs:
        d_in = _dev(corpus[off: off + n])
        d_out = _out(container, states, n)
        ins.append(d_in)
        outs.append(d_out)
        members.append((container, states, bits, d_in, d_out, opts))
    r = ctx.encode_device_batch(members, want_plans=want_plans, stats=stats)
    lengths, plans = r if want_plans else (r, [None] * len(specs))
    return members, lengths, plans, outs


def test_every_member_equals_its_single_call(gpu_ctx, corpus):
    big = 3 << 20
    groups = H.index_boundaries(64, 11, big, gpu_ctx)
    hist = H.make_hist(corpus[7: 7 + 65536], 12)
    specs = [
        (RAW, 64, 11, 0, 1, {}),
        (RAW, 32, 10, 5, 31, {}),
        (RAW, 64, 12, 9, 63, {"index_interval": 4}),
        (RAW, 32, 13, 100, 64, {}),
        (RAW, 64, 14, 200, 65, {"index_interval": 4}),
        (RAW, 32, 15, 300, 4095, {"index_interval": 32}),
        (RAW, 64, 11, 400, 65536, {"index_interval": 4}),
        (RAW, 32, 11, 500, 1_000_003, {"index_interval": 32}),
        (RAW, 64, 11, 0, big, {"index_groups": groups}),
        (RAW, 64, 12, 7, 65536, {"hist": hist, "index_interval": 32}),
        (RAW, 32, 14, 600, 1_000_003, {}),
        (RAW, 64, 10, 700, 4095, {}),
        (MT, 64, 11, 800, 1, {"block_size": 1 << 14}),
        (MT, 32, 12, 900, 31, {"block_size": 1 << 16}),
        (MT, 64, 13, 1000, 63, {"block_size": 1 << 14, "index_interval": 4}),
        (MT, 32, 10, 1100, 64, {"block_size": 1 << 16, "index_interval": 4}),
        (MT, 64, 15, 1200, 65, {"block_size": 1 << 14}),
        (MT, 32, 14, 1300, 4095, {"block_size": 1 << 16, "index_interval": 32}),
        (MT, 64, 11, 1400, 65536, {"block_size": 1 << 14, "index_interval": 4}),
        (MT, 32, 11, 1500, 1_000_003, {"block_size": 1 << 16, "index_interval": 32}),
        (MT, 64, 12, 1600, big, {"block_size": 1 << 16, "index_interval": 32}),
        (MT, 64, 11, 1700, 1_000_003, {"block_size": 1 << 21}),  # one block larger than the input
        (MT, 32, 15, 1800, 65536, {"block_size": 1 << 14}),
        (MT, 64, 10, 1900, big, {"block_size": 1 << 14}),
    ]
    stats = {}
    members, lengths, plans, outs = _run(gpu_ctx, specs, corpus, stats=stats)
    assert stats["raw_members"] == 12 and stats["mt_members"] == 12
    for k, (container, states, bits, off, n, opts) in enumerate(specs):
        data = corpus[off: off + n]
        got = outs[k][: lengths[k]].cpu().numpy()
        want, want_plan = _single(gpu_ctx, container, states, bits, members[k][3], opts, True)
        assert lengths[k] == want.size, (k, lengths[k], want.size)
        assert np.array_equal(got, want), k
        assert np.all(outs[k][lengths[k]:].cpu().numpy() == SENTINEL), k  # nothing written past the stream
        assert np.array_equal(got, _host(container, states, bits, data, opts)), k
        assert (plans[k] is None) == (want_plan is None), k
        if want_plan is not None:
            assert np.array_equal(_plan_bytes(gpu_ctx, plans[k]), _plan_bytes(gpu_ctx, want_plan)), k


@pytest.mark.parametrize("container", [RAW, MT])
def test_round_trip_through_the_batch_decoder(gpu_ctx, corpus, container):
    K, n = 32, 1 << 20
    sizes = [n] * K
    specs = []
    for k in range(K):
        opts = ({"index_groups": H.index_boundaries_batch(64, 11, sizes, k, gpu_ctx)} if container == RAW
                else {"block_size": 1 << 16, "index_interval": 32})
        specs.append((container, 64, 11, k * 97, n, opts))
    members, lengths, plans, outs = _run(gpu_ctx, specs, corpus)
    assert all(p is not None for p in plans)
    streams = [outs[k][: lengths[k]] for k in range(K)]
    backs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(K)]
    batch = gpu_ctx.make_batch(plans)
    gpu_ctx.decode_device_batch(batch, streams, backs, stream_lengths=lengths)
    torch.cuda.synchronize()
    assert gpu_ctx.batch_status(batch) == [0] * K
    for k in range(K):
        assert torch.equal(backs[k], members[k][3]), k
    for k in range(K):  # each plan alone as well
        back = torch.zeros(n, dtype=torch.uint8, device="cuda")
        gpu_ctx.decode_device(plans[k], streams[k], back, stream_length=lengths[k])
        torch.cuda.synchronize()
        assert gpu_ctx.status(plans[k]) == 0
        assert torch.equal(back, members[k][3]), k


def test_many_small_raw_members(gpu_ctx, corpus):
    rng = np.random.default_rng(515)
    specs = []
    for k in range(512):
        n = int(rng.integers(1, 65537))
        off = int(rng.integers(0, corpus.size - n))
        specs.append((RAW, 64 if k % 2 else 32, 10 + k % 6, off, n, {}))
    stats = {}
    members, lengths, plans, outs = _run(gpu_ctx, specs, corpus, want_plans=False, stats=stats)
    assert stats["raw_members"] == 512 and stats["launches"] == 4  # histograms, coding wavefronts of 64 and 32 states, copy
    for k, (container, states, bits, off, n, opts) in enumerate(specs):
        assert np.array_equal(outs[k][: lengths[k]].cpu().numpy(), _host(RAW, states, bits, corpus[off: off + n], opts)), k


def _bad_hist(bits):
    counts = np.zeros(256, np.int64)
    counts[:4] = 1 << (bits - 2)
    counts[0] += 1  # sums to 2^bits + 1
    return hist_from_counts(counts)


def _refusal_cases(corpus):
    """(name, build) where build() returns the list of members of one call (two good ones plus the bad one)."""
    n = 5000
    good = lambda: [(RAW, 64, 11, _dev(corpus[:n]), _out(RAW, 64, n)), (MT, 64, 11, _dev(corpus[:n]), _out(MT, 64, n), {"block_size": 1 << 14})]
    data = corpus[n: 2 * n]

    def member(container=RAW, states=64, bits=11, d_in=None, d_out=None, **opts):
        d_in = _dev(data) if d_in is None else d_in
        d_out = _out(container, states, d_in.numel()) if d_out is None else d_out
        return (container, states, bits, d_in, d_out, opts)

    def misaligned_in():
        buf = _dev(corpus[: n + 16])
        return good() + [member(d_in=buf[1: 1 + n])]

    def misaligned_out():
        buf = _out(RAW, 64, n, extra=16)
        return good() + [member(d_out=buf[1:])]

    def short_out():
        return good() + [member(d_out=torch.full((H.capacity(RAW, 64, n) - 1,), SENTINEL, dtype=torch.uint8, device="cuda"))]

    def overlapping_outputs():
        shared = _out(MT, 64, n)
        return good() + [member(d_out=shared), member(container=MT, d_out=shared, block_size=1 << 14)]

    def output_over_input():
        m = good()
        victim = m[0][4]  # an input that lies inside another member's output
        return m + [member(d_in=victim[:n])]

    return [
        ("block_ member", lambda: good() + [member(container=H.BLOCK, block_size=1 << 14)]),
        ("16 states", lambda: good() + [member(states=16)]),
        ("bits 9", lambda: good() + [member(bits=9)]),
        ("bits 16", lambda: good() + [member(bits=16)]),
        ("misaligned d_in", misaligned_in),
        ("misaligned d_out", misaligned_out),
        ("out_capacity one byte short", short_out),
        ("length 0", lambda: good() + [member(length=0)]),
        ("mt_ block_size 0", lambda: good() + [member(container=MT, block_size=0)]),
        ("mt_ block_size not a multiple of 64", lambda: good() + [member(container=MT, block_size=1000)]),
        ("raw block_size", lambda: good() + [member(block_size=64)]),
        ("index_interval % 4", lambda: good() + [member(index_interval=6)]),
        ("non-ascending index_groups", lambda: good() + [member(index_groups=[8, 4])]),
        ("hist not summing to 2^bits", lambda: good() + [member(hist=_bad_hist(11))]),
        ("overlapping outputs", overlapping_outputs),
        ("output overlapping an input", output_over_input),
    ]


@pytest.mark.parametrize("case", range(16))
def test_refusals_launch_nothing(gpu_ctx, corpus, case):
    name, build = _refusal_cases(corpus)[case]
    members = build()
    before = [m[4].cpu().numpy().copy() for m in members]
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.encode_device_batch(members, want_plans=True)
    assert e.value.code == E_ARG, name
    assert e.value.lengths == [0] * len(members) and e.value.plans == [None] * len(members), name
    torch.cuda.synchronize()
    for m, b in zip(members, before):
        assert np.array_equal(m[4].cpu().numpy(), b), name


def test_a_failing_member_leaves_the_others_alone(gpu_ctx, corpus):
    n = 200_000
    data = corpus[:n]
    counts = np.array(H.make_hist(data, 11).symbolCount, np.int64)
    present = np.flatnonzero(np.bincount(data, minlength=256))
    keep = int(np.argmax(counts))
    lost = int([p for p in present if p != keep][-1])  # a byte that occurs gets no slot
    counts[keep] += counts[lost]
    counts[lost] = 0
    specs = [
        (RAW, 64, 11, 0, n, {"index_interval": 32}),
        (MT, 64, 11, 3000, n, {"block_size": 1 << 16, "index_interval": 32}),
        (RAW, 64, 11, 0, n, {"hist": hist_from_counts(counts), "index_interval": 32}),
        (RAW, 32, 12, 5000, n, {}),
        (MT, 32, 13, 7000, n, {"block_size": 1 << 14}),
    ]
    members = [(c, s, b, _dev(corpus[o: o + m]), _out(c, s, m), opts) for c, s, b, o, m, opts in specs]
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.encode_device_batch(members, want_plans=True)
    assert e.value.code == E_DEVICE and "member 2" in str(e.value)
    lengths, plans = e.value.lengths, e.value.plans
    assert lengths[2] == 0 and plans[2] is None
    for k in (0, 1, 3, 4):
        c, s, b, d_in, d_out, opts = members[k]
        want, want_plan = _single(gpu_ctx, c, s, b, d_in, opts, True)
        assert lengths[k] == want.size and np.array_equal(d_out[: lengths[k]].cpu().numpy(), want), k
        assert (plans[k] is None) == (want_plan is None), k
        if want_plan is not None:
            assert np.array_equal(_plan_bytes(gpu_ctx, plans[k]), _plan_bytes(gpu_ctx, want_plan)), k


def test_launch_count_does_not_grow_with_the_member_count(gpu_ctx, corpus):
    seen = []
    for K in (2, 16, 128):
        specs = []
        for k in range(K):
            n = 3000 + 17 * k
            specs.append((RAW, 64, 11, k * 11, n, {"index_interval": 4}) if k % 2 == 0 else (MT, 64, 11, k * 13, n, {"block_size": 1 << 10, "index_interval": 4}))
        stats = {}
        members, lengths, plans, outs = _run(gpu_ctx, specs, corpus, stats=stats)
        assert all(v > 0 for v in lengths)
        seen.append(stats["launches"])
    # raw histograms, mt_ histograms, raw coding, mt_ coding, mt_ gather, raw copy, mt_ plans
    assert seen == [7, 7, 7], seen


def test_context_reuse(gpu_ctx, corpus):
    small = [(RAW, 64, 11, 0, 70_000, {"index_interval": 32}), (MT, 32, 12, 100, 90_000, {"block_size": 1 << 14, "index_interval": 4}),
             (RAW, 32, 13, 200, 5_000, {})]
    large = [(RAW, 64, 11, 300, 2_500_000, {"index_interval": 32}), (MT, 64, 11, 400, 3_500_000, {"block_size": 1 << 16, "index_interval": 32}),
             (MT, 32, 14, 500, 1_500_000, {"block_size": 1 << 14})]

    def outcome(specs):
        members, lengths, plans, outs = _run(gpu_ctx, specs, corpus)
        return [(outs[k][: lengths[k]].cpu().numpy(), _plan_bytes(gpu_ctx, plans[k])) for k in range(len(specs))]

    def same(a, b):
        assert len(a) == len(b)
        for (sa, pa), (sb, pb) in zip(a, b):
            assert np.array_equal(sa, sb)
            assert (pa is None) == (pb is None) and (pa is None or np.array_equal(pa, pb))

    first = outcome(small)
    singles = [_single(gpu_ctx, c, s, b, _dev(corpus[o: o + n]), opts, True) for c, s, b, o, n, opts in small]
    same(first, [(st, _plan_bytes(gpu_ctx, p)) for st, p in singles])
    big = outcome(large)  # the context's encode buffers grow
    same(outcome(small), first)
    same(outcome(large), big)
