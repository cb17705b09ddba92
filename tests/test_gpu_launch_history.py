"""Ticket-drawing launches past their counter sets, and overlapped.

Four launch paths hand work out through 64-bit ticket counters in device memory that are never reset: the uniform-interval raw launch
(k_decode_persist: run_persistent / run_persistent_pair), the grouped launch with more groups than workgroups (run_grouped, launch info
`dynamic_groups`), its batch twin, and the plans the device encoders and the first-decode indexing pass build.  Each relies on "a launch
draws exactly H tickets, so ticket % H is this launch's own order whatever the counter has seen before"; a plan owns kCounterSets sets of
counters and launch k takes set k % kCounterSets, so that launches may overlap (include/hsrans_hip.h).  The first kCounterSets launches of a
plan each see a zeroed set: only launch kCounterSets + 1 meets a counter that is not zero.  Every case here launches ONE plan
2 * kCounterSets + 3 times (every set reused twice, set 0 three times), serially, from four streams at once, from a captured graph, after
a launch that reported a bad histogram, through a batch, a queue, the host-pointer entry's refilled plan and a rank's sub-runs in one launch.

The first test needs no GPU: it measures the inputs (never a kernel): the shapes are ticket shapes under the default geometry.  Every GPU
case repeats that assertion from the launch info of the real launch.  Every "want" is the oracle's decode of the stream; every output
buffer has 4096 guard bytes of 0xCC behind it and is filled with a poison value that changes from launch to launch; bytes are compared on
the device."""
import functools
import hashlib
import os
import re

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api, synth
from oracle_lib import BLOCK, MT, RAW

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
GUARD = 4096


def _counter_sets():
    with open(os.path.join(ROOT, "hypersonic_rans_amd", "csrc", "hsrans_kernels.h")) as f:
        return int(re.search(r"^constexpr uint32_t kCounterSets = (\d+);", f.read(), re.M).group(1))


SETS = _counter_sets()
LAUNCHES = 2 * SETS + 3

# ---- the shapes: the smallest at which the kernels draw tickets ----
N_RAW = 3_000_003
RAW_CASES = [(states, bits, interval) for interval in (32, 4) for states in (64, 32) for bits in (11, 13, 15)]
N_GROUPED, BLOCK_SIZE, INTERVAL = 9_000_000, 1 << 13, 4
GROUPED_CASES = [(container, states, bits) for container in (MT, BLOCK) for states, bits in ((64, 11), (64, 12), (64, 15), (32, 11))]
BATCH_SIZES = [2_300_000 + 100_003 * k for k in range(4)]
BATCH_CONTAINERS = (MT, BLOCK, MT, BLOCK)
# (the 6,000,000-byte shape in 64 KiB blocks of test_a_ranks_sub_runs_announce_their_completion has 89 groups: a rank's launch of it is static,
# grid 44 and 46, and draws nothing.  The smallest round size at which BOTH ranks' launches have clearly more groups than the 512 workgroups
# of a 12-bit grouped launch, in the 8 KiB blocks of the grouped cases: 681 and 674 groups)
SUB_RUNS = (MT, 64, 12, 12_000_000, 1 << 13, 4)
SUB_WORLD, SUB_PARTS = 2, 3
NAMES = {RAW: "raw", BLOCK: "block", MT: "mt"}
raw_id = lambda c: f"raw-{c[0]}-{c[1]}-g{c[2]}"
grouped_id = lambda c: f"{NAMES[c[0]]}-{c[1]}-{c[2]}"


@functools.lru_cache(maxsize=None)
def raw_case(states, bits, interval):
    d = synth.nonstationary(N_RAW, seed=700 + states + bits)
    s, plan = H.encode(H.RAW, states, bits, d, index_interval=interval)
    return d, s, plan


@functools.lru_cache(maxsize=None)
def block_case(container, states, bits, n=N_GROUPED, block=BLOCK_SIZE, interval=INTERVAL, seed=77):
    d = synth.nonstationary(n, seed=seed)
    if interval:
        s, plan = H.encode(container, states, bits, d, index_interval=interval, block_size=block)
    else:
        s = H.encode(container, states, bits, d, block_size=block)
        plan = H.plan_build(container, states, bits, s)
    return d, s, plan


@functools.lru_cache(maxsize=None)
def sub_run_case():
    container, states, bits, n, block, interval = SUB_RUNS
    d = synth.nonstationary(n, seed=5)
    s, plan = H.encode(container, states, bits, d, index_interval=interval, block_size=block)
    return d, s, plan


def rank_slices(plan):
    """the plan of each rank's whole run of chains (what a sharded decode launches when one launch decodes all of a rank's sub-runs)"""
    from hypersonic_rans_amd import sharded
    return [H.plan_slice(plan, first, count) for first, count in sharded.ShardLayout(plan, SUB_WORLD, parts=SUB_PARTS).runs]


_wants = {}


def oracle_bytes(oracle, container, states, bits, stream, plan, data):
    """the oracle's decode of the stream (its plan executor where the reference's decoder refuses the file), computed once per stream"""
    key = (container, states, bits, data.size, hashlib.sha256(stream).digest())
    if key not in _wants:
        r, want = oracle.decode(container, states, bits, stream, data.size)
        if r != data.size:
            r, want = oracle.exec_plan(plan, stream, data.size)
        assert r == data.size and np.array_equal(want[:r], data)
        want = want[:data.size]
        want.setflags(write=False)
        _wants[key] = want
    return _wants[key]


# ---- what a plan is to the launcher ----
def _header(plan):
    return api.plan_tables(plan)[0]


def _kind(hdr):
    return {k: hdr[k] for k in ("container", "states", "bits", "flags", "decoded_len", "n_chains", "n_pieces", "shared_hist", "interval")}


def static_total(n_chains, states, info):
    """static_shares (csrc/hsrans_launch.cpp) from the launch info: the chains the waves of a uniform-interval launch decode without a
    ticket; the rest, n_chains - static_total, go through the queues (two runs per wave at 32 states)"""
    grid, waves, weights = info["grid"], info["waves_per_block"], info["class_weights"]
    W, runs = grid * waves, 2 if states == 32 else 1
    per_class = waves // 4 if waves >= 4 else 1
    classes = waves // per_class
    first_half = (grid + 1) // 2
    wg = [sum(n_chains * weights[hf * 4 + k] // (1000 * W * runs) * per_class * runs for k in range(4) if k < classes) for hf in range(2)]
    return first_half * wg[0] + (grid - first_half) * wg[1]


def assert_raw_draws_tickets(case, hdr, info):
    """a uniform-interval launch whose queues hand out at least 500 chains (and, at 64 states, whose static runs are not empty)"""
    states, bits, interval = case
    assert hdr["interval"] == interval and hdr["states"] == states and hdr["n_chains"] == info["chains"], (case, hdr, info)
    assert info["shared_table"] == 1 and info["chains_per_wave"] == 1 and info["table_mode"] == (4 if bits == 15 else 3) and info["waves_per_block"] == 16, (case, info)
    st = static_total(hdr["n_chains"], states, info)
    assert 0 <= st <= hdr["n_chains"] and hdr["n_chains"] - st >= 500, (case, hdr["n_chains"], st, info)
    if states == 64:
        assert st > 0, (case, hdr["n_chains"], info)
    return st


def group_count(plan):
    """the groups dplan_fill makes of a block_/mt_ plan with single-piece chains: consecutive chains of one histogram, and runs of
    single-symbol blocks; (groups, fewest chains of a coded group that is neither the first nor the last, chain each group begins at, any fill)"""
    hdr, cf, pieces = api.plan_tables(plan)
    assert hdr["n_pieces"] == hdr["n_chains"] and np.array_equal(cf, np.arange(hdr["n_chains"] + 1))
    fill = (pieces["flags"] & 2) != 0
    hist = pieces["hist_off"]
    joins = np.zeros(hdr["n_chains"], bool)
    joins[1:] = (fill[1:] & fill[:-1]) | (~fill[1:] & ~fill[:-1] & (hist[1:] == hist[:-1]))
    begins = np.flatnonzero(~joins)
    counts = np.diff(np.append(begins, hdr["n_chains"]))
    coded = np.flatnonzero(~fill[begins])
    inner = counts[coded[1:-1]]
    return begins.size, int(inner.min()) if inner.size else 0xFFFFFFFF, begins, bool(fill.any())


def grouped_facts(plan):
    """LaunchFacts of a block_/mt_ plan with an index, as dplan_fill and dplan_launch fill them (no group of these plans is long enough
    to be cut into parts: 32 chains a block)"""
    hdr = _header(plan)
    n_groups, fewest, begins, any_fill = group_count(plan)
    lean = hdr["states"] == 64
    dealt = lean and not any_fill and api.dealt_shares(np.append(begins, hdr["n_chains"]), hdr["decoded_len"] // 64, bits=hdr["bits"])[0]
    return dict(n_groups=n_groups, groups_lean=int(lean), spread_min_block=fewest if lean else 0, tickets=1, dealt=int(dealt))


def assert_grouped_draws_tickets(plan, info):
    """the grouped launch with more groups than workgroups: every group behind the first round is a ticket"""
    n_groups = group_count(plan)[0]
    assert info["dynamic_groups"] == 1 and info["spread"] == 0 and n_groups > info["grid"], (n_groups, info)
    return n_groups


def test_the_shapes_are_ticket_shapes():
    """Measured on the inputs alone (hsrans_launch_choice at the default geometry, 256 CUs): raw plans take k_decode_persist<3> (<4> at 15
    bits) with 729 .. 23,438 chains behind the static runs; the grouped plans take k_decode_grouped with dynamic_groups == 1 and more groups
    than workgroups; the batch members' groups together exceed the grid a grouped launch of that many groups gets; each rank's run of the
    sub-run case takes k_decode_grouped<3, true, true> with dynamic_groups == 1 (681 and 674 groups for 512 workgroups)."""
    assert SETS >= 2
    for case in RAW_CASES:
        states, bits, interval = case
        hdr = _header(raw_case(*case)[2])
        name, info = api.launch_choice(_kind(hdr), persistent=1, table_mode=4 if bits == 15 else 3)
        assert name == f"hsrans::k_decode_persist<{4 if bits == 15 else 3}>", (case, name, info)
        assert_raw_draws_tickets(case, hdr, info)
    for case in GROUPED_CASES:
        container, states, bits = case
        plan = block_case(*case)[2]
        name, info = api.launch_choice(_kind(_header(plan)), **grouped_facts(plan))
        assert name == f"hsrans::k_decode_grouped<{4 if bits >= 13 else 3}, {'true' if states == 64 else 'false'}, false>", (case, name, info)
        assert_grouped_draws_tickets(plan, info)
    groups = chains = 0
    for k, (container, n) in enumerate(zip(BATCH_CONTAINERS, BATCH_SIZES)):
        plan = block_case(container, 64, 11, n, seed=900 + k)[2]
        assert -(-n // BLOCK_SIZE) >= 281
        groups, chains = groups + group_count(plan)[0], chains + _header(plan)["n_chains"]
    _, info = api.launch_choice(dict(container=MT, states=64, bits=11, decoded_len=sum(BATCH_SIZES), n_chains=chains, n_pieces=chains), n_groups=groups, groups_lean=1, tickets=1)
    assert groups > info["grid"], (groups, info)
    for rank, part in enumerate(rank_slices(sub_run_case()[2])):
        name, info = api.launch_choice(_kind(_header(part)), parts=1, n_parts=SUB_PARTS, **grouped_facts(part))
        assert name == "hsrans::k_decode_grouped<3, true, true>", (rank, name, info)
        assert_grouped_draws_tickets(part, info)


# ---- on the GPU ----
def _upload(stream):
    import torch
    return torch.from_numpy(np.concatenate([stream, np.zeros((-stream.size) % 16 + 16, np.uint8)])).cuda()


def _poison(launch):
    v = (0x35 + 0x47 * launch) & 0xFF
    return v if v != 0xCC else 0x33


def _new_buf(n, launch=0):
    import torch
    buf = torch.full((n + GUARD,), 0xCC, dtype=torch.uint8, device="cuda")
    buf[:n].fill_(_poison(launch))
    return buf


def _check_buf(buf, d_want, what):
    """the oracle's bytes and the guard intact, compared on the device"""
    import torch
    n = d_want.numel()
    if not torch.equal(buf[:n], d_want):
        wrong = (buf[:n] != d_want).nonzero()
        at = int(wrong[0])
        raise AssertionError(f"{what}: {wrong.numel()} of {n} bytes differ from the oracle, the first at {at}: got {int(buf[at])} want {int(d_want[at])}")
    assert bool((buf[n:] == 0xCC).all()), f"{what}: wrote behind the output"


class Member:
    """a stream on the device, the oracle's bytes beside it, and its device plan"""

    def __init__(self, ctx, oracle, container, states, bits, data, stream, plan, dplan=None, d_in=None):
        import torch
        self.ctx, self.container, self.plan, self.stream, self.n, self.m = ctx, container, plan, stream, data.size, stream.size
        self.want = oracle_bytes(oracle, container, states, bits, stream, plan, data)
        self.d_want = torch.from_numpy(self.want.copy()).cuda()
        self.d_in = _upload(stream) if d_in is None else d_in
        self.dplan = ctx.make_device_plan(plan) if dplan is None else dplan
        self.buf = _new_buf(self.n)
        self.launches = 0

    def launch(self, what="", d_in=None, stream=None, buf=None, check=True):
        """one launch into the poisoned buffer: status 0, the oracle's bytes, the guard intact"""
        k = self.launches
        self.launches += 1
        buf = self.buf if buf is None else buf
        buf[:self.n].fill_(_poison(k))
        self.ctx.decode_device(self.dplan, self.d_in if d_in is None else d_in, buf[:self.n], stream=stream, stream_length=self.m)
        if check:
            what = f"{what} launch {k + 1} of this plan (launch % {SETS} == {k % SETS})"
            assert self.ctx.status(self.dplan) == 0, what
            _check_buf(buf, self.d_want, what)

    def assert_draws_tickets(self, case=None):
        info = self.dplan.launch_info()
        if self.container == RAW:
            assert_raw_draws_tickets(case, _header(self.plan), info)
        else:
            assert_grouped_draws_tickets(self.plan, info)
        return info


def _raw_member(ctx, oracle, case):
    states, bits, interval = case
    return Member(ctx, oracle, RAW, states, bits, *raw_case(*case))


def _block_member(ctx, oracle, case):
    container, states, bits = case[:3]
    return Member(ctx, oracle, container, states, bits, *block_case(*case))


THREE = [("raw", (64, 11, 32)), ("raw", (32, 11, 32)), ("grouped", (MT, 64, 11))]
FOUR = THREE + [("grouped", (BLOCK, 64, 11))]
plan_id = lambda p: raw_id(p[1]) if p[0] == "raw" else grouped_id(p[1])


def _member(ctx, oracle, which):
    kind, case = which
    return (_raw_member if kind == "raw" else _block_member)(ctx, oracle, case), (case if kind == "raw" else None)


# 1. past the sets
@gpu
@pytest.mark.parametrize("case", RAW_CASES, ids=raw_id)
def test_raw_plan_past_its_counter_sets(gpu_ctx, oracle, case):
    """k_decode_persist: every queue head of every set is reused twice, set 0 three times"""
    m = _raw_member(gpu_ctx, oracle, case)
    for _ in range(LAUNCHES):
        m.launch(raw_id(case))
    m.assert_draws_tickets(case)


@gpu
@pytest.mark.parametrize("case", GROUPED_CASES, ids=grouped_id)
def test_grouped_plan_past_its_counter_sets(gpu_ctx, oracle, case):
    """k_decode_grouped with dynamic_groups == 1: ticket % n_groups on a counter that has seen two launches"""
    m = _block_member(gpu_ctx, oracle, case)
    for _ in range(LAUNCHES):
        m.launch(grouped_id(case))
    m.assert_draws_tickets()


# 2. plans built on the device
@gpu
@pytest.mark.parametrize("builder", ("encode_device-mt", "encode_device_ex-mt", "encode_device_ex-block", "indexing-mt", "indexing-block"))
def test_device_built_plan_past_its_counter_sets(gpu_ctx, oracle, builder):
    """the group lists and ticket counters the device encoders and the first-decode indexing pass lay out themselves"""
    import torch
    how, name = builder.split("-")
    container = MT if name == "mt" else BLOCK
    n = N_GROUPED
    if how == "indexing":
        d, s, _ = block_case(container, 64, 11, interval=0)
        _, s4, plan = block_case(container, 64, 11)  # (the encoder's plan of the same stream bytes: what the oracle's plan executor may need)
        assert np.array_equal(s, s4)
        d_in = _upload(s)
        base = gpu_ctx.make_device_plan_from_stream(container, 64, 11, d_in, s.size, n)
        first = _new_buf(n)
        dplan = gpu_ctx.decode_device_indexing(base, d_in, first[:n], INTERVAL, stream_length=s.size)
        m = Member(gpu_ctx, oracle, container, 64, 11, d, s, plan, dplan=dplan, d_in=d_in)
        _check_buf(first, m.d_want, f"{builder}: the first decode")
    else:
        d = block_case(container, 64, 11)[0]
        kw = dict(independent_blocks=True) if how == "encode_device" else {}
        s, plan = H.encode(container, 64, 11, d, index_interval=INTERVAL, block_size=BLOCK_SIZE, **kw)
        cap = H.capacity(container, 64, n)
        d_out = torch.zeros(cap + 32, dtype=torch.uint8, device="cuda")
        d_src = torch.from_numpy(d).cuda()
        if how == "encode_device":
            size, dplan = gpu_ctx.encode_device(container, 64, 11, d_src, d_out[:cap], block_size=BLOCK_SIZE, index_interval=INTERVAL, want_plan=True)
        else:
            size, dplan = gpu_ctx.encode_device_ex(container, 64, 11, d_src, d_out[:cap], block_size=BLOCK_SIZE, index_interval=INTERVAL, want_device_plan=True)
        assert size == s.size and torch.equal(d_out[:size].cpu(), torch.from_numpy(s)), builder
        m = Member(gpu_ctx, oracle, container, 64, 11, d, s, plan, dplan=dplan, d_in=d_out)
    for _ in range(LAUNCHES):
        m.launch(builder)
    m.assert_draws_tickets()


# 3. overlap
@gpu
@pytest.mark.parametrize("which", THREE, ids=plan_id)
def test_launches_of_one_plan_overlap_on_four_streams(gpu_ctx, oracle, which):
    """what include/hsrans_hip.h promises: launches of ONE device plan on several streams, each with its own output, fewer than
    kCounterSets of them in flight (four streams: at most four)"""
    import torch
    m, case = _member(gpu_ctx, oracle, which)
    bufs = [_new_buf(m.n, k) for k in range(LAUNCHES)]
    streams = [torch.cuda.Stream() for _ in range(4)]
    for s in streams:
        s.wait_stream(torch.cuda.current_stream())
    for k, buf in enumerate(bufs):
        gpu_ctx.decode_device(m.dplan, m.d_in, buf[:m.n], stream=streams[k % 4], stream_length=m.m)
    torch.cuda.synchronize()
    assert gpu_ctx.status(m.dplan) == 0
    for k, buf in enumerate(bufs):
        _check_buf(buf, m.d_want, f"{plan_id(which)} launch {k + 1} (launch % {SETS} == {k % SETS}) on stream {k % 4}")
    m.assert_draws_tickets(case)


# 4. graph
@gpu
@pytest.mark.parametrize("which", THREE, ids=plan_id)
def test_a_captured_launch_keeps_its_counter_set_across_replays(gpu_ctx, oracle, which):
    """a graph node's counters are the set the capture took: five replays, an eager launch of the same plan between them"""
    import torch
    m, case = _member(gpu_ctx, oracle, which)
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            gpu_ctx.decode_device(m.dplan, m.d_in, m.buf[:m.n], stream=side, stream_length=m.m)
    torch.cuda.synchronize()
    eager = _new_buf(m.n)
    for replay in range(5):
        m.buf[:m.n].fill_(_poison(replay))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert gpu_ctx.status(m.dplan) == 0, replay
        _check_buf(m.buf, m.d_want, f"{plan_id(which)} replay {replay + 1}")
        m.launch(f"{plan_id(which)} between replays:", buf=eager)
    m.assert_draws_tickets(case)


# 5. after a reported failure
def _damaged(m):
    """the stream with one histogram count changed: the corruptions test_failure_modes (raw) and
    test_many_small_block_streams_share_one_launch (mt_, block_) apply and know to end in a status word"""
    bad = m.d_in.clone()
    if m.container == RAW:
        bad[16] ^= 1
    else:
        bad[400] ^= 0x11
    return bad


@gpu
@pytest.mark.parametrize("which", FOUR, ids=plan_id)
def test_good_launches_behind_one_that_reported_a_bad_histogram(gpu_ctx, oracle, which):
    """the draw count of a launch whose histogram check failed: kCounterSets + 1 launches later its counter set comes round again"""
    import torch
    m, case = _member(gpu_ctx, oracle, which)
    for _ in range(4):
        m.launch(plan_id(which))
    m.launch(d_in=_damaged(m), check=False)
    assert gpu_ctx.status(m.dplan) != 0, "a changed histogram count went unreported"
    assert bool((m.buf[m.n:] == 0xCC).all()), "the failing launch wrote behind the output"
    assert gpu_ctx.status(m.dplan) == 0  # (reported once, then cleared)
    # two refused calls: neither launches, neither writes
    m.buf[:m.n].fill_(0x77)
    shifted = torch.zeros(m.d_in.numel() + 16, dtype=torch.uint8, device="cuda")
    shifted[1:1 + m.d_in.numel()] = m.d_in
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device(m.dplan, shifted[1:], m.buf[:m.n], stream_length=m.m)
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device(m.dplan, m.d_in, m.buf[:m.n - 1], stream_length=m.m)
    torch.cuda.synchronize()
    assert bool((m.buf[:m.n] == 0x77).all()) and bool((m.buf[m.n:] == 0xCC).all()), "a refused call wrote"
    assert gpu_ctx.status(m.dplan) == 0
    for _ in range(SETS + 1):
        m.launch(f"{plan_id(which)} behind the failure:")
    m.assert_draws_tickets(case)


# 6. batch and queue
@gpu
def test_grouped_batch_and_queue_past_their_counter_sets(gpu_ctx, oracle):
    """the grouped batch launch's own tickets (k_decode_grouped_batch), and a Queue's cached batch"""
    import torch
    ms = [Member(gpu_ctx, oracle, c, 64, 11, *block_case(c, 64, 11, n, seed=900 + k)) for k, (c, n) in enumerate(zip(BATCH_CONTAINERS, BATCH_SIZES))]
    batch = gpu_ctx.make_batch([m.dplan for m in ms])
    info = batch.info()
    # (the launch's own group count, and the same number recounted from the plans: what the CPU test holds above the default geometry's grid)
    assert info["launches"] == 1 and info["grouped_members"] == 4 and info["solo_members"] == 0 and info["direct_members"] == 0 and info["groups"] > info["grid"] > 0, info
    assert info["groups"] == sum(group_count(m.plan)[0] for m in ms), info

    def launch(k, d_ins=None):
        for m in ms:
            m.buf[:m.n].fill_(_poison(k))
        gpu_ctx.decode_device_batch(batch, d_ins or [m.d_in for m in ms], [m.buf[:m.n] for m in ms], stream_lengths=[m.m for m in ms])
        torch.cuda.synchronize()
        return gpu_ctx.batch_status(batch)

    def check(k, what, skip=None):
        for i, m in enumerate(ms):
            if i != skip:
                _check_buf(m.buf, m.d_want, f"{what} {k + 1} ({what} % {SETS} == {k % SETS}), member {i}")

    for k in range(LAUNCHES):
        assert launch(k) == [0] * 4, k
        check(k, "batch launch")
    codes = launch(LAUNCHES, [_damaged(m) if i == 1 else m.d_in for i, m in enumerate(ms)])
    assert codes[1] != 0 and codes[0] == codes[2] == codes[3] == 0, codes
    check(LAUNCHES, "batch launch", skip=1)
    assert bool((ms[1].buf[ms[1].n:] == 0xCC).all()), "the failing member wrote behind its output"
    for k in range(LAUNCHES + 1, LAUNCHES + SETS + 2):
        assert launch(k) == [0] * 4, k
        check(k, "batch launch")
    batch.close()
    # the same members through a queue: its batch is made once and launched again by every later flush
    q = api.Queue(gpu_ctx, max_members=4)
    for k in range(LAUNCHES):
        for m in ms:
            m.buf[:m.n].fill_(_poison(k))
            q.submit(m.dplan, m.d_in, m.buf[:m.n], stream_length=m.m)
        q.flush()
        torch.cuda.synchronize()
        for m in ms:
            assert gpu_ctx.status(m.dplan) == 0, k
        check(k, "queue round")
    st = q.stats()
    assert st["batches_reused"] == LAUNCHES - 1 and st["batches_made"] == 1, st
    q.close()


# 7. the host-pointer entry's refilled plan
@gpu
def test_host_entry_refills_its_plan_with_the_other_kind_on_every_call(gpu_ctx, oracle):
    """hsrans_decode_host: one device plan per context, refilled on every call (dplan_arena zeroes heads and epoch); then the context's
    cached index of a plan-less stream, launched kCounterSets + 2 times.  The entry decodes into a staging buffer of the context's that
    nobody can poison from outside, and bytes a launch leaves undecoded would still be there from the call before: so between the plan-less
    calls another stream of the same size is decoded with its plan (which leaves the cached index alone) and overwrites that buffer.
    The launch info of the context's own plans cannot be read from outside, so this case carries no ticket-shape assertion of its own: its
    streams are those of case 1 (raw 64/11/32 and mt 64/11, held to drawing tickets there and in the CPU test), its cached index is the
    same stream's blocks with a checkpoint every 64 groups, and that it draws tickets was seen once, when this case failed at plan-less
    call kCounterSets + 2 against a build without the modulo (CHANGELOG.md).  A change of the geometry that ends that is caught in case 1."""
    raw = (RAW, 64, 11) + raw_case(64, 11, 32)
    mt = (MT, 64, 11) + block_case(MT, 64, 11)
    other = (BLOCK, 64, 11) + block_case(BLOCK, 64, 11, seed=78)
    wants = [oracle_bytes(oracle, *c[:3], c[4], c[5], c[3]) for c in (raw, mt, other)]
    assert other[3].size == mt[3].size and int((wants[2] != wants[1]).sum()) > mt[3].size // 2  # (the other stream's bytes really are others)

    def call(k, which, with_plan, what):
        container, states, bits, d, s, plan = (raw, mt, other)[which]
        r, got = gpu_ctx.decode_host(container, states, bits, s, d.size, plan=plan if with_plan else None)
        assert r == d.size, (what, k, r)
        assert np.array_equal(got, wants[which]), f"{what} {k + 1} ({NAMES[container]}): first wrong byte at {int(np.argmax(got != wants[which]))}"

    for k in range(LAUNCHES):
        call(k, k & 1, True, "call")
    chains = None
    for k in range(SETS + 3):
        call(k, 1, False, "plan-less call")
        if chains is None:
            chains = gpu_ctx.host_index_chains()
        assert chains > 0 and gpu_ctx.host_index_chains() == chains, (k, chains)  # (from the second call on the cached index is what launches)
        call(k, 2, True, "call between plan-less calls")


# 8. sub-runs in one launch
@gpu
def test_a_ranks_sub_runs_in_one_grouped_launch_past_the_counter_sets(gpu_ctx, oracle, monkeypatch):
    """k_decode_grouped<3, true, true> with tickets: a rank's three sub-runs in one launch of more groups than workgroups, so that the groups
    behind the first round are drawn and the sub-runs are signalled on the dynamic path; the rank's plan is launched again and again.
    Nothing here waits on a completion word or reads one (test_a_ranks_sub_runs_announce_their_completion covers the words): what is
    checked is the bytes of the rank's range, its status and that nothing outside the range is written."""
    import torch
    from hypersonic_rans_amd import sharded
    monkeypatch.setenv("HSRANS_SHARD_ONE_LAUNCH", "1")
    container, states, bits = SUB_RUNS[:3]
    d, stream, plan = sub_run_case()
    d_want = torch.from_numpy(oracle_bytes(oracle, container, states, bits, stream, plan, d).copy()).cuda()
    slices = rank_slices(plan)
    for rank in range(SUB_WORLD):
        dec = sharded.ShardedDecoder(gpu_ctx, plan, parts=SUB_PARTS, world=SUB_WORLD, rank=rank)
        assert bool(dec.c.info["one_launch"]) and dec.c.whole_plan() is not None
        d_window = dec.upload_window(stream, "cuda")
        out = dec.alloc_out("cuda")
        b, e = dec.ranges[rank]
        b, e = b - dec.out_base, e - dec.out_base
        assert 0 <= b < e <= out.numel()
        for k in range(LAUNCHES):
            out.fill_(_poison(k))
            torch.cuda.synchronize()
            dec.step(d_window, out, gather=False)
            torch.cuda.synchronize()
            dec.check()
            what = f"rank {rank} step {k + 1} (step % {SETS} == {k % SETS})"
            assert torch.equal(out[b:e], d_want[b + dec.out_base:e + dec.out_base]), f"{what}: {int((out[b:e] != d_want[b + dec.out_base:e + dec.out_base]).sum())} bytes of the rank's range differ from the oracle"
            assert bool((out[:b] == _poison(k)).all()) and bool((out[e:] == _poison(k)).all()), f"{what}: wrote outside the rank's range"
        info = dec.launch_info()
        assert info["chains"] == _header(slices[rank])["n_chains"], (rank, info)
        assert_grouped_draws_tickets(slices[rank], info)
