"""hsrans_encode_device_ex_batch: many block_ / carried-state mt_ streams encoded on the GPU by one launch per kernel kind.  Every member
against its single call (hsrans_encode_device_ex: stream bytes, length, plan blob, device plan) and the host encoder; device plans
decoded back through the batch decoder; a launch count that does not grow with the member count; refusals that launch nothing; a plan
that does not fit failing alone; context reuse.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth
from hypersonic_rans_amd.api import EncodeExBatchStats, EncodeExMember, EncodeOpts, ENC_INDEPENDENT_BLOCKS

pytestmark = pytest.mark.gpu

RAW, BLOCK, MT = H.RAW, H.BLOCK, H.MT
E_ARG = 2
SENTINEL = 0xA5
EXTRA = 64
# the adaptive policy's unit, 1 << MinBlockSize (hsrans_host.cpp reference_policy): mt_ 2^16; block_ by states and bits 10..15
_MIN64, _MIN32 = (20, 19, 16, 17, 17, 16), (20, 19, 15, 17, 17, 18)


def walk_unit(container, states, bits):
    return 1 << 16 if container == MT else 1 << (_MIN64 if states == 64 else _MIN32)[bits - 10]


@pytest.fixture(scope="module")
def zipf():
    return synth.enwik8_shaped(1 << 20, seed=11)


@pytest.fixture(scope="module")
def nonstat():
    return synth.nonstationary(3_000_000)


@pytest.fixture(scope="module")
def runs(zipf):
    return np.concatenate([np.full(70_000, 7, np.uint8), zipf[:100_000], np.full(200_000, 200, np.uint8), zipf[:33]])


def _dev(data):
    return torch.from_numpy(np.ascontiguousarray(data)).cuda()


def _out(container, states, n):
    """(the whole tensor, the view the encoder is given): EXTRA sentinel bytes lie behind out_capacity"""
    cap = H.capacity(container, states, n)
    whole = torch.full((cap + EXTRA,), SENTINEL, dtype=torch.uint8, device="cuda")
    return whole, whole[:cap]


def _indexed(opts):
    return bool(opts.get("index_interval")) or opts.get("index_groups") is not None


def _single(ctx, container, states, bits, d_in, opts):
    """The member's single call: (stream bytes, plan blob or None, whether it returned a device plan)."""
    _, d_out = _out(container, states, d_in.numel())
    r = ctx.encode_device_ex(container, states, bits, d_in, d_out, want_plan=True, want_device_plan=True, **opts)
    if not isinstance(r, tuple):
        return d_out[:r].cpu().numpy(), None, False
    n, plan, dplan = r
    return d_out[:n].cpu().numpy(), plan, bool(dplan.handle.value)


def _host(container, states, bits, data, opts):
    r = H.encode(container, states, bits, data, **opts)
    return r if isinstance(r, tuple) else (r, None)


def _run(ctx, specs, stats=None, want_device_plans=True):
    """specs: (container, states, bits, data, opts).  Returns (lengths, plans, dplans, ins, wholes)."""
    ins = [_dev(s[3]) for s in specs]
    outs = [_out(s[0], s[1], s[3].size) for s in specs]
    members = [(s[0], s[1], s[2], ins[k], outs[k][1], s[4]) for k, s in enumerate(specs)]
    r = ctx.encode_device_ex_batch(members, want_plans=True, want_device_plans=want_device_plans, stream=None, stats=stats)
    lengths, plans = r[0], r[1]
    return lengths, plans, (r[2] if want_device_plans else None), ins, [w for w, _ in outs]


def _check_against_single_and_host(ctx, specs, lengths, plans, dplans, ins, wholes):
    for k, (container, states, bits, data, opts) in enumerate(specs):
        what = (k, container, states, bits, data.size, {n: v for n, v in opts.items() if n != "index_groups"})
        got = wholes[k].cpu().numpy()
        stream, plan, has_dplan = _single(ctx, container, states, bits, ins[k], opts)
        host_stream, host_plan = _host(container, states, bits, data, opts)
        assert lengths[k] == stream.size == host_stream.size, what
        assert np.array_equal(got[: lengths[k]], stream) and np.array_equal(stream, host_stream), what
        assert (got[lengths[k]:] == SENTINEL).all(), what
        if _indexed(opts):
            assert plans[k] is not None and np.array_equal(plans[k], plan) and np.array_equal(plan, host_plan), what
        else:
            assert plans[k] is None and plan is None, what
        assert (dplans[k] is not None) == has_dplan, what


def _member_mix(zipf, nonstat, runs):
    specs = []
    combos = ((BLOCK, 32), (BLOCK, 64), (MT, 32), (MT, 64))
    for i, (container, S) in enumerate(combos):  # the short lengths, every bit width
        for j, n in enumerate((1, S - 5, S, S + 1, 4095)):
            at = 1000 * (5 * i + j)
            specs.append((container, S, 10 + (5 * i + j) % 6, zipf[at: at + n], {}))
    for container, S, bits in ((BLOCK, 32, 12), (MT, 64, 11)):  # around the walk's unit
        unit = walk_unit(container, S, bits)
        for n in (unit - S, unit - 1, unit + 1, unit + S + 3):
            specs.append((container, S, bits, np.resize(nonstat, n), {}))
    specs.append((BLOCK, 64, 10, nonstat, {}))  # several adaptive blocks
    specs.append((MT, 64, 12, runs, {}))  # single-symbol blocks
    specs.append((BLOCK, 32, 13, np.full(300_000, 42, np.uint8), {}))
    part = zipf[:300_000]
    specs.append((BLOCK, 64, 11, part, {"block_size": 4096}))  # fixed blocks, carried states
    specs.append((MT, 32, 12, part, {"block_size": 65536}))
    specs.append((MT, 64, 10, part, {"block_size": 65536 + 64}))
    specs.append((MT, 64, 11, zipf[: 2 * 65536 + 64 - 7], {"block_size": 65536}))  # a remainder shorter than a group: merged
    specs.append((BLOCK, 32, 14, zipf[: 2 * 4096 + 32 - 7], {"block_size": 4096}))
    specs.append((MT, 64, 11, zipf, {"block_size": 65536, "independent_blocks": True, "index_groups": H.index_boundaries(64, 11, zipf.size)}))
    specs.append((BLOCK, 64, 12, zipf[:500_000], {"index_interval": 4}))
    specs.append((MT, 32, 11, zipf, {"index_interval": 32}))
    specs.append((MT, 64, 13, part, {"block_size": 65536, "index_interval": 32}))
    specs.append((BLOCK, 64, 11, zipf, {"index_groups": H.index_boundaries(64, 11, zipf.size)}))  # listed checkpoints, carried states
    specs.append((MT, 32, 12, zipf, {"block_size": 65536, "index_groups": H.index_boundaries(32, 12, zipf.size)}))
    return specs


def test_every_member_equals_its_single_call_and_the_host_encoder(gpu_ctx, zipf, nonstat, runs):
    specs = _member_mix(zipf, nonstat, runs)
    assert len(specs) >= 40
    stats = {}
    lengths, plans, dplans, ins, wholes = _run(gpu_ctx, specs, stats)
    assert stats["block_members"] == sum(s[0] == BLOCK for s in specs) and stats["mt_members"] == sum(s[0] == MT for s in specs)
    assert 1 <= stats["launches"] <= 5 and stats["blocks"] >= len(specs) and stats["units"] >= len(specs)
    _check_against_single_and_host(gpu_ctx, specs, lengths, plans, dplans, ins, wholes)


def test_round_trip_through_the_batch_decoder(gpu_ctx):
    corpus = synth.enwik8_shaped(4 << 20, seed=23)
    n = 1 << 20
    specs = [((BLOCK if k < 16 else MT), 64, 11, corpus[k * 98304: k * 98304 + n], {"index_interval": 32}) for k in range(32)]
    lengths, plans, dplans, ins, wholes = _run(gpu_ctx, specs)
    assert all(p is not None for p in dplans)
    streams = [wholes[k][: lengths[k]] for k in range(32)]
    outs = [torch.zeros(n, dtype=torch.uint8, device="cuda") for _ in range(32)]
    batch = gpu_ctx.make_batch(dplans)
    gpu_ctx.decode_device_batch(batch, streams, outs)
    assert gpu_ctx.batch_status(batch) == [0] * 32
    for k in range(32):
        assert torch.equal(outs[k], ins[k]), k
    for k in range(32):  # each plan alone
        outs[k].zero_()
        gpu_ctx.decode_device(dplans[k], streams[k], outs[k])
        assert gpu_ctx.status(dplans[k]) == 0 and torch.equal(outs[k], ins[k]), k


def test_the_launch_count_does_not_grow_with_the_member_count(gpu_ctx, zipf):
    def mix(K, adaptive):
        # (the adaptive mt_ members are longer than the walk's unit, 2^16: they have whole units for the cost launch)
        four = [(MT, 64, 11, {} if adaptive else {"block_size": 8192}), (MT, 32, 12, {} if adaptive else {"block_size": 4096}),
                (MT, 64, 10, {"block_size": 4096}), (BLOCK, 32, 13, {"index_interval": 32} if adaptive else {"block_size": 4096, "index_interval": 32})]
        return [(c, S, bits, zipf[997 * k: 997 * k + 70_000 + 64 * k], opts) for k in range(K) for c, S, bits, opts in (four[k % 4],)]

    counts = {}
    for K in (4, 64):
        stats = {}
        _run(gpu_ctx, mix(K, True), stats, want_device_plans=False)
        counts[K] = stats["launches"]
    assert counts[4] == counts[64] and counts[4] <= 5
    stats = {}
    _run(gpu_ctx, mix(8, False), stats, want_device_plans=False)
    assert stats["launches"] == counts[4] - 1  # no member walks the adaptive policy: no unit costs


def _good(zipf):
    return [(BLOCK, 64, 11, zipf[:50_000], {}), (MT, 32, 12, zipf[1000:41_000], {"index_interval": 32}), (MT, 64, 10, zipf[:30_000], {"block_size": 4096})]


REFUSALS = ("raw", "independent_interval", "independent_no_index", "bits", "states", "misaligned_in", "misaligned_out", "capacity", "block_size", "interval", "length",
            "outputs_overlap", "output_over_input")


@pytest.mark.parametrize("case", REFUSALS)
def test_refusals_launch_nothing(gpu_ctx, zipf, case):
    specs = _good(zipf)
    ins = [_dev(s[3]) for s in specs]
    outs = [_out(s[0], s[1], s[3].size) for s in specs]
    members = [(s[0], s[1], s[2], ins[k], outs[k][1], s[4]) for k, s in enumerate(specs)]
    n = 40_000
    d_in = _dev(np.concatenate([zipf[:n], zipf[:16]]))
    whole, d_out = _out(MT, 64, n + 16)
    watched = [w for w, _ in outs] + [whole]
    bad = {"raw": (RAW, 64, 11, d_in[:n], d_out),
           "independent_interval": (MT, 64, 11, d_in[:n], d_out, {"block_size": 65536, "independent_blocks": True, "index_interval": 32}),
           "independent_no_index": (MT, 64, 11, d_in[:n], d_out, {"block_size": 65536, "independent_blocks": True}),
           "bits": (MT, 64, 9, d_in[:n], d_out),
           "states": (MT, 48, 11, d_in[:n], d_out),
           "misaligned_in": (MT, 64, 11, d_in[1: n + 1], d_out),
           "misaligned_out": (MT, 64, 11, d_in[:n], whole[1: 1 + d_out.numel()]),
           "capacity": (MT, 64, 11, d_in[:n], d_out[: H.capacity(MT, 64, n) - 1]),
           "block_size": (MT, 64, 11, d_in[:n], d_out, {"block_size": 100}),
           "interval": (MT, 64, 11, d_in[:n], d_out, {"index_interval": 6}),
           "length": (MT, 64, 11, d_in[:n], d_out, {"length": 0}),
           "outputs_overlap": (MT, 32, 12, d_in[:n], outs[1][0][16:]),
           "output_over_input": (MT, 64, 11, d_in[:n], None)}[case]
    if case == "output_over_input":  # the new member's output lies over member 0's input
        room = torch.full((50_000 + H.capacity(MT, 64, n),), SENTINEL, dtype=torch.uint8, device="cuda")
        room[:50_000] = ins[0]
        members[0] = members[0][:3] + (room[:50_000],) + members[0][4:]
        bad = bad[:4] + (room[: H.capacity(MT, 64, n)],)
        watched.append(room)
    before = [w.clone() for w in watched]
    stats = {}
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.encode_device_ex_batch(members[:2] + [bad] + members[2:], want_plans=True, want_device_plans=True, stats=stats)
    assert e.value.code == E_ARG and e.value.lengths == [0] * 4 and e.value.rcs == [E_ARG] * 4
    assert e.value.plans == [None] * 4 and e.value.device_plans == [None] * 4
    assert stats["launches"] == 0
    torch.cuda.synchronize()
    for w, b in zip(watched, before):
        assert torch.equal(w, b)
    for w, _ in outs:
        assert bool((w == SENTINEL).all())


def _ctypes_call(ctx, rows, want_device_plans=False):
    """rows: (container, states, bits, d_in, d_out, EncodeOpts or None), straight to the C entry.  Returns (rc, members, handles, stats)."""
    arr = (EncodeExMember * len(rows))()
    for k, (container, states, bits, d_in, d_out, opts) in enumerate(rows):
        e = arr[k]
        e.container, e.states, e.bits = container, states, bits
        e.d_in, e.length, e.d_out, e.out_capacity = d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_out.numel()
        if opts is not None:
            e.opts = ctypes.pointer(opts)
    handles = (ctypes.c_void_p * len(rows))()
    stats = EncodeExBatchStats()
    s = torch.cuda.current_stream()
    rc = ctx.L.hsrans_encode_device_ex_batch(ctx.handle, arr, len(rows), ctypes.c_void_p(s.cuda_stream), handles if want_device_plans else None, ctypes.byref(stats))
    return rc, arr, handles, stats


def test_two_members_sharing_one_opts_are_refused(gpu_ctx, zipf):
    ins = [_dev(zipf[:30_000]), _dev(zipf[5000:45_000])]
    outs = [_out(MT, 64, t.numel()) for t in ins]
    shared = EncodeOpts(4096, 0, None, 0, 0, 0, 0, None, 0)
    rc, arr, _, stats = _ctypes_call(gpu_ctx, [(MT, 64, 11, ins[k], outs[k][1], shared) for k in range(2)])
    assert rc == E_ARG and [m.stream_length for m in arr] == [0, 0] and [m.rc for m in arr] == [E_ARG] * 2 and stats.launches == 0
    torch.cuda.synchronize()
    assert all(bool((w == SENTINEL).all()) for w, _ in outs)
    # (each with an opts object of its own: accepted)
    own = [EncodeOpts(4096, 0, None, 0, 0, 0, 0, None, 0) for _ in range(2)]
    rc, arr, _, stats = _ctypes_call(gpu_ctx, [(MT, 64, 11, ins[k], outs[k][1], own[k]) for k in range(2)])
    assert rc == 0 and all(m.stream_length > 0 and m.rc == 0 for m in arr) and stats.launches > 0


def test_a_plan_that_does_not_fit_fails_alone(gpu_ctx, zipf):
    datas = [zipf[:200_000], zipf[100_000:400_000], zipf[300_000:450_000]]
    spec = [(BLOCK, 64, 11), (MT, 64, 12), (MT, 32, 11)]
    ins = [_dev(d) for d in datas]
    singles = [_single(gpu_ctx, c, S, bits, ins[k], {"index_interval": 32}) for k, (c, S, bits) in enumerate(spec)]
    outs = [_out(c, S, datas[k].size) for k, (c, S, bits) in enumerate(spec)]
    bufs = [np.zeros(singles[k][1].size - (8 if k == 1 else 0), np.uint8) for k in range(3)]  # member 1: 8 bytes short of what its plan needs
    opts = [EncodeOpts(0, 32, bufs[k].ctypes.data, bufs[k].size, 77, 0, 0, None, 0) for k in range(3)]
    rc, arr, handles, stats = _ctypes_call(gpu_ctx, [spec[k] + (ins[k], outs[k][1], opts[k]) for k in range(3)], want_device_plans=True)
    try:
        assert rc == E_ARG
        assert arr[1].rc == E_ARG and arr[1].stream_length == 0 and opts[1].plan_size == 0 and not handles[1]
        torch.cuda.synchronize()
        assert bool((outs[1][0] == SENTINEL).all())
        for k in (0, 2):
            stream, plan, _ = singles[k]
            got = outs[k][0].cpu().numpy()
            assert arr[k].rc == 0 and arr[k].stream_length == stream.size and np.array_equal(got[: stream.size], stream) and (got[stream.size:] == SENTINEL).all()
            assert opts[k].plan_size == plan.size and np.array_equal(bufs[k], plan) and handles[k]
    finally:
        for h in handles:
            if h:
                gpu_ctx.L.hsrans_dplan_destroy(ctypes.c_void_p(h))


def test_context_reuse(gpu_ctx, zipf, nonstat, runs):
    big = [(BLOCK, 64, 10, nonstat[:1_500_000], {"index_interval": 32}), (MT, 64, 12, runs, {}), (MT, 32, 11, zipf, {"block_size": 65536, "index_interval": 4}),
           (BLOCK, 32, 12, zipf[:70_000], {"index_groups": H.index_boundaries(32, 12, 70_000)}), (MT, 64, 11, zipf[:4095], {})]
    small = [(MT, 64, 11, zipf[:9000], {"index_interval": 32}), (BLOCK, 32, 15, zipf[:63], {})]

    def results(specs):
        lengths, plans, dplans, ins, wholes = _run(gpu_ctx, specs)
        return lengths, [None if p is None else p.tobytes() for p in plans], [w.cpu().numpy().tobytes() for w in wholes]

    first, first_small = results(big), results(small)
    d_in = _dev(zipf[:300_000])
    _, d_out = _out(BLOCK, 64, d_in.numel())
    n1, plan1 = gpu_ctx.encode_device_ex(BLOCK, 64, 11, d_in, d_out, index_interval=32, want_plan=True)
    assert results(small) == first_small
    raw_out = _out(RAW, 64, d_in.numel())[1]
    mt_out = _out(MT, 64, d_in.numel())[1]
    gpu_ctx.encode_device_batch([(RAW, 64, 11, d_in, raw_out), (MT, 64, 11, d_in, mt_out, {"block_size": 65536})])
    assert results(big) == first
    _, d_out2 = _out(BLOCK, 64, d_in.numel())
    n2, plan2 = gpu_ctx.encode_device_ex(BLOCK, 64, 11, d_in, d_out2, index_interval=32, want_plan=True)
    assert n1 == n2 and np.array_equal(plan1, plan2) and torch.equal(d_out[:n1], d_out2[:n2])
