"""Decode and encode kernels on streams at the extreme word rates (tests/rate_inputs.py): nearly every lane takes a 16-bit word in nearly
every group (the most the LDS stream ring, the re-base once per 4 groups, the gather's non-storing skip and the one-chain kernel's
producer/consumer ring ever see), no lane takes a word for groups on end (adjacent checkpoints on ONE stream word: a chain whose window
is empty), and both in turn at lengths that are no multiple of 4 groups.

The first test needs no GPU: it measures the inputs (never a kernel) against the floors that make them extreme, and runs every one of them
through the host SIMD decoders (hsrans_decode_cpu, which re-base their cursors in blocks too).  Every GPU case compares the GPU's bytes with the
oracle's decode of the same stream, writes into a buffer with 0xCC guard bytes behind it, asserts status 0, launches its plan twice and
asserts from the launch info that the kernel it is about is the one that ran."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api, synth
from oracle_lib import BLOCK, MT, RAW

import rate_inputs as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu
GUARD = 4096


# ---- the inputs, made once per process (the encoders run on the host) ----
@functools.lru_cache(maxsize=None)
def raw_case(kind, n, states, bits, index=None):
    """(data, stream, plan) of a raw input under hot_hist; index: None (one chain), an interval, or "wave" (hsrans_index_boundaries, MI355X)"""
    if index is None:
        d, s = R.encode_raw(kind, n, states, bits, seed=bits + states)
        return d, s, H.plan_build(H.RAW, states, bits, s)
    kw = dict(index_groups=H.index_boundaries(states, bits, n, None)) if index == "wave" else dict(index_interval=index)
    d, (s, plan) = R.encode_raw(kind, n, states, bits, seed=bits + states, **kw)
    return d, s, plan


@functools.lru_cache(maxsize=None)
def mixed_case(container, states, bits, n, block, interval, fill=()):
    d = R.mixed_blocks(n, block, bits, seed=bits + states + container, fill_blocks=fill)
    if interval:
        s, plan = H.encode(container, states, bits, d, index_interval=interval, block_size=block)
    else:
        s = H.encode(container, states, bits, d, block_size=block)
        plan = H.plan_build(container, states, bits, s)
    return d, s, plan


def oracle_bytes(oracle, container, states, bits, stream, plan, data):
    """the oracle's decode of the stream (its plan executor where the reference's decoder refuses the file): the bytes the GPU must give"""
    r, want = oracle.decode(container, states, bits, stream, data.size)
    if r != data.size:
        r, want = oracle.exec_plan(plan, stream, data.size)
    assert r == data.size and np.array_equal(want, data)
    return want


# ---- every input of the GPU cases below, for the CPU test ----
SINGLE = [(kind, n, states, bits) for kind in ("hot", "cold", "alternating") for n in (200_003, (1 << 20) + 65) for states in (32, 64) for bits in (10, 11, 12, 14)]
N_INDEXED = 3_000_003
INDEXED = [(kind, N_INDEXED, states, bits, index) for kind in ("cold", "alternating") for states in (32, 64) for bits in (11, 13, 15) for index in (4, 32, "wave")]
N_BUILD = 400_037
BUILD = [(kind, N_BUILD, states, bits, 4) for kind in ("hot", "alternating") for states in (32, 64) for bits in (11, 15)]
N_BATCH = 2_000_003
N_GATHER, N_GATHER_RAW, N_TAIL = 300_007, 100_003, 1_000_003
GATHER_BITS = (11, 12, 14, 15)
GATHER_RAW = [("alternating", N_GATHER_RAW, states, bits, None) for states in (32, 64) for bits in GATHER_BITS] + \
             [("alternating", N_GATHER, states, bits, 32) for states in (32, 64) for bits in GATHER_BITS]
N_ENC = 300_007
ENC_RAW = [(kind, N_ENC, states, bits, index) for kind in ("hot", "cold", "alternating") for states in (32, 64) for bits in (11, 15) for index in (None, 4)]

DEALT = [(c, 64, 11, (4 << 20) + 1, 1 << 17, 4) for c in (MT, BLOCK)]
DEALT_RANK = [(MT, 64, bits, 8_000_001, 1 << 18, 4) for bits in (13, 14)]
SPREAD = (MT, 64, 11, 8_000_001, 1 << 18, 4, (3, 17))
DYNAMIC = (MT, 64, 11, 9_000_000, 1 << 13, 4)
STATIC = [(MT, 64, bits, 8_000_001, 1 << 18, 4) for bits in (12, 15)]
NON_LEAN = (MT, 32, 11, 2_000_001, 1 << 16, 4)
PRIVATE = [(c, states, bits, 600_001, 1 << 16, 0) for c in (MT, BLOCK) for states in (32, 64) for bits in (11, 15)]
RECORDING = [(c, 64, bits, 2_000_001, 1 << 16, 0) for c in (MT, BLOCK) for bits in (11, 14)]
GROUPED_BATCH = [(c, 64, 11, 700_001 + 100_000 * k, 1 << 15, (4, 32)[k]) for c in (MT, BLOCK) for k in (0, 1)]
GATHER_MIXED = [(c, states, bits, N_GATHER, 1 << 16, 32) for c in (MT, BLOCK) for states in (32, 64) for bits in GATHER_BITS]
WINDOW = (MT, 64, 11, 2_000_001, 1 << 16, 4)
PIPELINE = (MT, 64, 11, 8_000_001, 1 << 18, 4)
SUB_RUNS = (MT, 64, 11, 24_000_000, 1 << 18, 8)
ENC_MIXED = [(c, 64, 11, 1_000_003, block, 4) for c in (MT, BLOCK) for block in (1 << 14, 1 << 17)]
PLANES_N, PLANES_BLOCK = 300_001, 1 << 16
# the table of the issue: both containers and state counts at every width, a checkpoint every 4 groups
TABLE = [(c, states, bits, 600_001, block, 4) for c in (MT, BLOCK) for states in (32, 64)
         for bits, block in ((10, 1 << 16), (11, 1 << 16), (12, 1 << 16), (13, 1 << 17), (14, 1 << 17), (15, 1 << 18))]

RAW_INPUTS = [c + (None,) for c in SINGLE] + INDEXED + BUILD + GATHER_RAW + ENC_RAW + [("hot", N_TAIL, 64, 11, None)] + \
             [(kind, N_BATCH, 64, bits, index) for kind in ("hot", "cold", "alternating") for bits in (11, 13, 14, 15) for index in ("wave", 32)] + \
             [(kind, N_BATCH, 32, 11, index) for kind in ("hot", "cold", "alternating") for index in ("wave", 32)]
MIXED_INPUTS = DEALT + DEALT_RANK + [SPREAD, DYNAMIC, NON_LEAN, WINDOW, PIPELINE, SUB_RUNS] + STATIC + PRIVATE + RECORDING + GROUPED_BATCH + GATHER_MIXED + ENC_MIXED + TABLE


def _cpu_decoders_agree(container, states, bits, stream, plan, want):
    for level in range(api.cpu_level() + 1):
        for threads in (1, 4):
            for p in (None, plan):
                r, got = api.decode_cpu(container, states, bits, stream, want.size, plan=p, level=level, threads=threads)
                assert r == want.size and np.array_equal(got, want), (container, states, bits, want.size, level, threads, p is not None)


def test_the_inputs_are_extreme_and_the_host_decoders_agree_on_them(oracle):
    """The floors, measured on the inputs alone.  A symbol of frequency 1 of 2^bits costs `bits` bits, so: a raw_hot stream is longer than
    n * bits / 8; the hot stretches of a mixed_blocks stream cost at least `bits` bits a byte (what is left of the stream after 520 bytes a block
    for its header, states and histogram, over the hot bytes: the cold rest only adds to it).  A chain that takes no word begins and ends on one
    stream word: a plan with a checkpoint every 4 groups over cold, alternating or mixed data holds at least 100 such pairs of neighbours
    (measured: 141 .. 29,537 per mixed plan, 407 .. 20,173 per raw plan; the hot bytes cost 0.9 .. 5.2 bits more than `bits`).  Longer chains get
    no floor: even the cold symbol costs a fraction of a bit, so 64 lanes together take a word every few groups at 11 bits, every few dozen
    at 15."""
    seen = set()
    for kind, n, states, bits, index in RAW_INPUTS:
        if (kind, n, states, bits, index) in seen:
            continue
        seen.add((kind, n, states, bits, index))
        d, s, plan = raw_case(kind, n, states, bits, index)
        if kind == "hot":
            assert s.size > n * bits // 8, (kind, n, states, bits)
        elif index == 4:
            assert R.equal_neighbours(plan) >= 100, (kind, n, states, bits, index, R.equal_neighbours(plan))
        _cpu_decoders_agree(H.RAW, states, bits, s, plan, oracle_bytes(oracle, RAW, states, bits, s, plan, d))
    for case in MIXED_INPUTS:
        if case in seen:
            continue
        seen.add(case)
        _mixed_floors(oracle, case, *mixed_case(*case))
    # the inputs the device encoders get, as the host encoder codes them in independent blocks (what encode_device and the planes' encoder write)
    for case in [c for c in ENC_MIXED if c[0] == MT] + [(MT, 64, 11, PLANES_N, PLANES_BLOCK, 4)]:
        container, states, bits, n, block, interval = case
        d = planes_low() if n == PLANES_N else mixed_case(*case)[0]
        s, plan = H.encode(container, states, bits, d, index_interval=interval, block_size=block, independent_blocks=True)
        _mixed_floors(oracle, case, d, s, plan)
    high = planes_high()
    s, plan = H.encode(MT, 64, 11, high, index_interval=4, block_size=PLANES_BLOCK, independent_blocks=True)
    assert R.equal_neighbours(plan) >= 100
    _cpu_decoders_agree(MT, 64, 11, s, plan, oracle_bytes(oracle, MT, 64, 11, s, plan, high))
    raw_case.cache_clear()  # (this test alone touches every input: a few hundred megabytes the GPU cases need not inherit)
    mixed_case.cache_clear()


def planes_low():
    return R.mixed_blocks(PLANES_N, PLANES_BLOCK, 11, seed=9)


def planes_high():
    return R.raw_cold(PLANES_N, seed=10)


def _mixed_floors(oracle, case, d, s, plan):
    container, states, bits, n, block, interval = case[:6]
    fill = case[6] if len(case) > 6 else ()
    assert s.size <= H.capacity(container, states, n)
    hot = R.mixed_hot_bytes(n, block, bits, fill)
    cost = (s.size - 520 * -(-n // block)) * 8 / hot
    assert cost >= bits, (case, cost)
    if interval == 4:
        assert R.equal_neighbours(plan) >= 100, (case, R.equal_neighbours(plan))
    want = oracle_bytes(oracle, container, states, bits, s, plan, d)
    if not api.plan_tables(plan)[0]["flags"] & 1:  # (a block_ stream without an index has a walk plan: its one chain follows the inline headers)
        r, by_plan = oracle.exec_plan(plan, s, n)
        assert r == n and np.array_equal(by_plan, want), case
    _cpu_decoders_agree(container, states, bits, s, plan, want)


# ---- on the GPU ----
def _upload(stream):
    import torch
    return torch.from_numpy(np.concatenate([stream, np.zeros((-stream.size) % 16 + 16, np.uint8)])).cuda()


def _decode_twice(ctx, plan_or_dplan, stream, want, d_in=None):
    """two launches of one device plan into a buffer with guard bytes behind it: status 0, the oracle's bytes, the guard intact; returns
    the launch info"""
    import torch
    dplan = plan_or_dplan if isinstance(plan_or_dplan, api.DevicePlan) else ctx.make_device_plan(plan_or_dplan)
    d_in = _upload(stream) if d_in is None else d_in
    n = want.size
    buf = torch.full((n + GUARD,), 0xCC, dtype=torch.uint8, device="cuda")
    for launch in range(2):
        buf[:n].fill_(0xCC if launch else 0)
        ctx.decode_device(dplan, d_in, buf[:n], stream_length=stream.size)
        assert ctx.status(dplan) == 0, launch
        got = buf.cpu().numpy()
        assert np.array_equal(got[:n], want), (launch, int(np.argmax(got[:n] != want)))
        assert (got[n:] == 0xCC).all(), "wrote behind the output"
    return dplan.launch_info()


@gpu
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits", (10, 11, 12, 14))
def test_one_chain_kernel(gpu_ctx, oracle, states, bits):
    """k_decode_single (launch info: one workgroup of two waves): the producer wave's ring at the most words a group takes, at none, and
    going from one to the other"""
    for kind, n, s_, b_ in SINGLE:
        if (s_, b_) != (states, bits):
            continue
        d, s, plan = raw_case(kind, n, states, bits)
        assert H.plan_chain_count(plan) == 1
        info = _decode_twice(gpu_ctx, plan, s, oracle_bytes(oracle, RAW, states, bits, s, plan, d))
        assert (info["grid"], info["waves_per_block"], info["chains"]) == (1, 2, 1), (kind, n, info)


@gpu
def test_one_chain_on_the_general_kernel_in_a_child_process():
    """HSRANS_SINGLE_FAST=0 (read once per process): the same streams on one wave of the general kernel, against the oracle"""
    code = r"""
import sys, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r + '/tests')
import hypersonic_rans_amd as H
import test_gpu_rate_extremes as T
from oracle_lib import Oracle, RAW
ctx, oracle = H.Context(0), Oracle()
for kind, n, states, bits in T.SINGLE:
    d, s, plan = T.raw_case(kind, n, states, bits)
    info = T._decode_twice(ctx, plan, s, T.oracle_bytes(oracle, RAW, states, bits, s, plan, d))
    assert (info['grid'], info['waves_per_block']) == (1, 1), (kind, n, states, bits, info)
print('ok')
""" % (ROOT, ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, HSRANS_SINGLE_FAST="0"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok" in r.stdout, (r.stdout[-500:], r.stderr[-1500:])


@gpu
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits", (11, 13, 15))
def test_raw_plans_with_an_index_on_idle_and_alternating_streams(gpu_ctx, oracle, states, bits):
    """k_decode_direct (one chain per wave), k_decode_persist (a uniform interval), k_decode_dual (13-15 bits: two chains per wave) and the
    32-state pair loop, where whole chains take no word (`limit == start`) and where the ring goes from idle to full rate inside a chain"""
    for kind in ("cold", "alternating"):
        for index in (4, 32, "wave"):
            d, s, plan = raw_case(kind, N_INDEXED, states, bits, index)
            info = _decode_twice(gpu_ctx, plan, s, oracle_bytes(oracle, RAW, states, bits, s, plan, d))
            assert info["shared_table"] == 1 and info["chains"] == H.plan_chain_count(plan) and info["waves_per_block"] == 16, (kind, index, info)
            assert info["table_mode"] == (4 if bits == 15 else 3), (kind, index, info)
            # (two chains per wave: 64 states, 13 bits and more, a plan with one chain per wave; the same widths with a uniform interval: k_decode_persist)
            assert info["chains_per_wave"] == (2 if states == 64 and bits >= 13 and index == "wave" else 1), (kind, index, info)


def _mixed_on_device(ctx, oracle, case):
    d, s, plan = mixed_case(*case)
    container, states, bits = case[:3]
    return _decode_twice(ctx, plan, s, oracle_bytes(oracle, container, states, bits, s, plan, d))


@gpu
@pytest.mark.parametrize("case", DEALT, ids=("mt", "block"))
def test_dealt_launch(gpu_ctx, oracle, case):
    """k_decode_dealt<true, false>: 32 blocks, 16,384 chains"""
    info = _mixed_on_device(gpu_ctx, oracle, case)
    assert info["spread"] == 2 and info["table_mode"] == 3, info


@gpu
@pytest.mark.parametrize("case", DEALT_RANK, ids=("13", "14"))
def test_dealt_launch_with_rank_tables(gpu_ctx, oracle, case):
    """k_decode_dealt_rank<13> and <14>"""
    info = _mixed_on_device(gpu_ctx, oracle, case)
    assert info["spread"] == 2 and info["table_mode"] == 4, info


@gpu
def test_spread_launch(gpu_ctx, oracle):
    """k_decode_spread<3, false>: two single-symbol blocks keep the plan off the dealt launch"""
    info = _mixed_on_device(gpu_ctx, oracle, SPREAD)
    assert info["spread"] == 1 and info["waves_per_block"] == 16 and info["dynamic_groups"] == 0, info


@gpu
def test_grouped_launch_with_tickets(gpu_ctx, oracle):
    """k_decode_grouped<3, true, false> handing blocks out through its ticket counter: 1,099 blocks for 1,024 workgroups"""
    info = _mixed_on_device(gpu_ctx, oracle, DYNAMIC)
    assert info["dynamic_groups"] == 1 and info["waves_per_block"] == 8 and info["grid"] < 1099 and info["spread"] == 0, info


@gpu
@pytest.mark.parametrize("case", STATIC, ids=("12", "15"))
def test_grouped_launch_in_static_order(gpu_ctx, oracle, case):
    """k_decode_grouped<3, true, false> (12 bits) and <4, true, false> (15 bits): fewer groups than workgroups, no ticket counter"""
    info = _mixed_on_device(gpu_ctx, oracle, case)
    assert info["dynamic_groups"] == 0 and info["spread"] == 0 and info["shared_table"] == 1 and info["table_mode"] == (3 if case[2] == 12 else 4), info
    assert info["waves_per_block"] == 16 and info["grid"] < 512, info


@gpu
def test_grouped_launch_of_a_32_state_stream(gpu_ctx, oracle):
    """the grouped kernel that is not lean: 32 states"""
    info = _mixed_on_device(gpu_ctx, oracle, NON_LEAN)
    assert info["spread"] == 0 and info["shared_table"] == 1 and info["dynamic_groups"] == 0 and info["table_mode"] == 3 and info["waves_per_block"] == 16, info


@gpu
@pytest.mark.parametrize("case", PRIVATE, ids=lambda c: f"{('raw', 'block', 'mt')[c[0]]}-{c[1]}-{c[2]}")
def test_streams_without_an_index_and_a_table_per_wave(gpu_ctx, oracle, case):
    """un-indexed mt_ and block_ streams: every wave builds the table of its block (mt_) / one wave walks the inline headers (block_)"""
    container, states, bits, n = case[:4]
    d, s, plan = mixed_case(*case)
    want = oracle_bytes(oracle, container, states, bits, s, plan, d)
    for _ in range(2):
        r, got = gpu_ctx.decode_host(container, states, bits, s, n)
        assert r == n and np.array_equal(got, want), int(np.argmax(got != want))
    info = _decode_twice(gpu_ctx, plan, s, want)
    assert info["shared_table"] == 0 and info["spread"] == 0 and info["dynamic_groups"] == 0, info
    assert info["walk"] == (1 if container == BLOCK else 0) and info["table_mode"] == PRIVATE_KIND[bits], info


# ---- the recording passes ----
@gpu
@pytest.mark.parametrize("interval", (4, 32))
@pytest.mark.parametrize("case", RECORDING, ids=lambda c: f"{('raw', 'block', 'mt')[c[0]]}-{c[2]}")
def test_first_decode_records_the_index(gpu_ctx, oracle, case, interval):
    """decode_device_indexing on un-indexed mixed streams: the recording pass's bytes, the plan it leaves (hsrans_index_build's, byte for byte)
    and a second decode with that plan"""
    import torch
    container, states, bits, n, block = case[:5]
    d, s, plan = mixed_case(*case)
    want = oracle_bytes(oracle, container, states, bits, s, plan, d)
    d_in = _upload(s)
    base = gpu_ctx.make_device_plan_from_stream(container, states, bits, d_in, s.size, n)
    first = torch.full((n + GUARD,), 0xCC, dtype=torch.uint8, device="cuda")
    indexed = gpu_ctx.decode_device_indexing(base, d_in, first[:n], interval, stream_length=s.size)
    got = first.cpu().numpy()
    assert np.array_equal(got[:n], want) and (got[n:] == 0xCC).all()
    _, s2, want_plan = mixed_case(container, states, bits, n, block, interval)  # (the encoder's plan of the same stream bytes)
    assert np.array_equal(s2, s)
    assert np.array_equal(gpu_ctx.read_device_plan(indexed, capacity=want_plan.size + 4096), want_plan)
    assert np.array_equal(gpu_ctx.index_build(container, states, bits, s, interval), want_plan)  # (the index pass alone, from a host copy)
    info = _decode_twice(gpu_ctx, indexed, s, want, d_in=d_in)
    assert info["chains"] == H.plan_chain_count(want_plan) and info["shared_table"] == 1, info


@gpu
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits", (11, 15))
def test_index_build_on_hot_and_alternating_streams(gpu_ctx, oracle, states, bits):
    """hsrans_index_build / hsrans_index_build_at on raw streams at full rate (the library records a raw stream's checkpoints with its host
    decoder): the encoder's plan byte for byte, and both plans decode on the GPU"""
    for kind in ("hot", "alternating"):
        d, s, want_plan = raw_case(kind, N_BUILD, states, bits, 4)
        want = oracle_bytes(oracle, RAW, states, bits, s, want_plan, d)
        plan = gpu_ctx.index_build(H.RAW, states, bits, s, 4)
        assert np.array_equal(plan, want_plan), kind
        groups = [4, 8, 1000, 1004, 4000, (N_BUILD // states // 4 - 1) * 4]
        at = gpu_ctx.index_build_at(H.RAW, states, bits, s, groups)
        assert np.array_equal(at, api.index_build_host(H.RAW, states, bits, s, groups)) and H.plan_chain_count(at) == len(groups) + 1
        for p in (plan, at):
            info = _decode_twice(gpu_ctx, p, s, want)
            assert info["chains"] == H.plan_chain_count(p) and info["shared_table"] == 1, info


@gpu
def test_first_decode_of_four_streams_in_one_call(gpu_ctx, oracle):
    """decode_device_indexing_batch: four members, two of them mixed streams at 14 bits (their hot stretches at the most words a group takes)"""
    import torch
    members, wants, plans = [], [], []
    for k, case in enumerate(RECORDING):
        container, states, bits, n, block = case[:5]
        d, s, plan = mixed_case(*case)
        wants.append(oracle_bytes(oracle, container, states, bits, s, plan, d))
        d_in = _upload(s)
        base = gpu_ctx.make_device_plan_from_stream(container, states, bits, d_in, s.size, n)
        members.append((base, d_in, torch.full((n,), 0xCC, dtype=torch.uint8, device="cuda"), (4, 32)[k % 2], s.size))
        plans.append(mixed_case(container, states, bits, n, block, (4, 32)[k % 2])[2])
    stats = {}
    indexed = gpu_ctx.decode_device_indexing_batch(members, stats=stats)
    for k, m in enumerate(members):
        assert np.array_equal(m[2].cpu().numpy(), wants[k]), k
        assert np.array_equal(gpu_ctx.read_device_plan(indexed[k], capacity=plans[k].size + 4096), plans[k]), k
        _decode_twice(gpu_ctx, indexed[k], mixed_case(*RECORDING[k])[1], wants[k], d_in=m[1])


# ---- batch ----
def _batch_members(ctx, oracle, specs):
    import torch
    ms = []
    for container, states, bits, d, s, plan in specs:
        ms.append({"stream": s, "want": oracle_bytes(oracle, container, states, bits, s, plan, d), "d_in": _upload(s),
                   "buf": torch.full((d.size + GUARD,), 0xCC, dtype=torch.uint8, device="cuda"), "dplan": ctx.make_device_plan(plan)})
    return ms


def _launch_batch_twice(ctx, batch, ms):
    import torch
    for launch in range(2):
        for m in ms:
            m["buf"][:m["want"].size].fill_(0xA5 if launch else 0)
        ctx.decode_device_batch(batch, [m["d_in"] for m in ms], [m["buf"][:m["want"].size] for m in ms], stream_lengths=[m["stream"].size for m in ms])
        torch.cuda.synchronize()
        assert ctx.batch_status(batch) == [0] * len(ms)
        for i, m in enumerate(ms):
            got, n = m["buf"].cpu().numpy(), m["want"].size
            assert np.array_equal(got[:n], m["want"]), f"member {i} differs from the oracle (launch {launch})"
            assert (got[n:] == 0xCC).all(), f"member {i} wrote behind its output"


def _raw_batch_specs(states, bits_of, index):
    specs = []
    for k, kind in enumerate(("hot", "cold", "alternating")):
        d, s, plan = raw_case(kind, N_BATCH, states, bits_of[k], index)
        specs.append((RAW, states, bits_of[k], d, s, plan))
    text = synth.enwik8_shaped(N_BATCH, seed=77)
    kw = dict(index_groups=H.index_boundaries(states, bits_of[3], N_BATCH, None)) if index == "wave" else dict(index_interval=index)
    s, plan = H.encode(H.RAW, states, bits_of[3], text, **kw)
    specs.append((RAW, states, bits_of[3], text, s, plan))
    return specs


@gpu
@pytest.mark.parametrize("index", ("wave", 32))
def test_batch_of_equal_streams_one_launch(gpu_ctx, oracle, index):
    """the one-chain-per-wave batch kernel: a stream at full rate, an idle one, an alternating one and text, side by side in one launch"""
    ms = _batch_members(gpu_ctx, oracle, _raw_batch_specs(64, (11,) * 4, index))
    batch = gpu_ctx.make_batch([m["dplan"] for m in ms])
    info = batch.info()
    assert info["launches"] == 1 and info["direct_members"] == 4 and info["solo_members"] == 0, info
    _launch_batch_twice(gpu_ctx, batch, ms)


@gpu
@pytest.mark.parametrize("index", ("wave", 32))
def test_batch_of_32_state_streams(gpu_ctx, oracle, index):
    """k_decode_batch_pair: a slot's run as two halves side by side"""
    ms = _batch_members(gpu_ctx, oracle, _raw_batch_specs(32, (11,) * 4, index))
    batch = gpu_ctx.make_batch([m["dplan"] for m in ms])
    info = batch.info()
    assert info["launches"] == 1 and info["direct_members"] == 4 and info["solo_members"] == 0, info
    _launch_batch_twice(gpu_ctx, batch, ms)


@gpu
@pytest.mark.parametrize("index", ("wave", 32))
def test_batch_of_wide_histogram_streams(gpu_ctx, oracle, index):
    """the two-chain batch kernels: the 8-byte table at 13 bits, the rank table at 14 and 15 — a launch for each table kind"""
    ms = _batch_members(gpu_ctx, oracle, _raw_batch_specs(64, (13,) * 4, index) + _raw_batch_specs(64, (14, 15, 14, 15), index))
    batch = gpu_ctx.make_batch([m["dplan"] for m in ms])
    info = batch.info()
    assert info["launches"] == 2 and info["direct_members"] == 8 and info["solo_members"] == 0, info
    _launch_batch_twice(gpu_ctx, batch, ms)


@gpu
def test_batch_of_block_streams_one_grouped_launch(gpu_ctx, oracle):
    """the grouped batch launch: mt_ and block_ members in 32 KiB blocks"""
    ms = _batch_members(gpu_ctx, oracle, [(c[0], c[1], c[2]) + mixed_case(*c) for c in GROUPED_BATCH])
    batch = gpu_ctx.make_batch([m["dplan"] for m in ms])
    info = batch.info()
    assert info["launches"] == 1 and info["grouped_members"] == 4 and info["solo_members"] == 0 and info["direct_members"] == 0, info
    _launch_batch_twice(gpu_ctx, batch, ms)


# ---- gather ----
CANARY = 4096


def _gather_kind(ctx, dplan, d_stream, m):
    """the gather kind of a plan (its decode-table layout), found by asking a set of this one member"""
    info = ctx.make_gather_set([dplan], [d_stream], [m]).info()
    assert sum(info["kind_members"]) == 1
    return info["kind_members"].index(1)


def _rows(src):
    """([member,] offset, length) -> ([member,] offset, length, destination), back to back behind a canary; and the buffer's size"""
    rows, pos = [], CANARY
    for r in src:
        rows.append(tuple(r) + (pos,))
        pos += r[-1]
    return rows, pos + CANARY


def _random_src(rng, count, n, longest):
    lens = np.minimum((2.0 ** rng.uniform(0, np.log2(longest), count)).astype(np.int64), n)
    offs = (rng.random(count) * (n - lens + 1)).astype(np.int64)
    return [(int(o), int(l)) for o, l in zip(offs, lens)]


def _edge_src(hot, cold):
    """ranges that begin and end inside the hot stretch [hot), inside the cold stretch [cold) behind it, and across the edge between them"""
    (hb, he), (cb, ce) = hot, cold
    assert he - hb >= 64 and ce - cb >= 64 and he == cb
    return [(hb + 3, he - hb - 7), (hb + (he - hb) // 2, 1), (cb + 5, ce - cb - 9), (cb + (ce - cb) // 2, 2), (he - 40, 80), (he - 1, 2), (hb + 1, ce - hb - 2)]


def _raw_edges(n, seed):
    st = R.hot_stretches(n, seed)
    for k in range(len(st) - 1):
        if st[k][1] - st[k][0] >= 1000 and st[k + 1][0] - st[k][1] >= 1000:
            return _edge_src(st[k], (st[k][1], st[k + 1][0]))
    raise AssertionError("no long hot stretch in front of a long cold one")


def _mixed_edges(n, block, bits):
    lo = block  # block 1
    b, e = R.mixed_stretch(1, min(block, n - lo), block, bits)
    assert lo + block - (lo + e) >= 1000
    return _edge_src((lo + b, lo + e), (lo + e, lo + block))


def _check_dst(got, want, rows):
    if not np.array_equal(got, want):
        bad = int(np.argmax(got != want))
        dsts = np.array([r[-1] for r in rows])
        row = int(np.searchsorted(dsts, bad, side="right")) - 1
        raise AssertionError(f"first wrong byte at destination {bad} (of {want.size}), range {row}: {rows[max(row, 0)]}, got {got[bad]} want {want[bad]}")


def _gather_both_ways(ctx, dplan, d_stream, m, data, src):
    """the ranges through decode_device_gather and through decode_device_gather_indirect: whole destination buffers, canaries included"""
    import torch
    rows, size = _rows(src)
    want = np.full(size, 0xCC, np.uint8)
    for off, length, dst in rows:
        want[dst:dst + length] = data[off:off + length]
    for launch in range(2):
        dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
        ctx.decode_device_gather(dplan, d_stream, rows, dst, stream_length=m)
        torch.cuda.synchronize()
        _check_dst(dst.cpu().numpy(), want, rows)
        assert ctx.status(dplan) == 0
    dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    d_rows = torch.from_numpy(np.array(rows, np.int64).reshape(-1, 3)).cuda()
    ctx.decode_device_gather_indirect(dplan, d_stream, d_rows, dst, stream_length=m)
    torch.cuda.synchronize()
    _check_dst(dst.cpu().numpy(), want, rows)
    assert ctx.status(dplan) == 0


def _gather_member(ctx, container, states, bits, index):
    """(data, stream, plan, explicit ranges) of one cell of the gather matrix"""
    if container == RAW:
        n = N_GATHER if index else N_GATHER_RAW
        d, s, plan = raw_case("alternating", n, states, bits, index)
        return d, s, plan, _raw_edges(n, bits + states)
    d, s, plan = mixed_case(container, states, bits, N_GATHER, 1 << 16, 32)
    return d, s, plan, _mixed_edges(N_GATHER, 1 << 16, bits)


PRIVATE_KIND = {10: 0, 11: 0, 12: 1, 13: 2, 14: 2, 15: 2}  # a table per wave: 4 bytes a slot, the same with freq - 1, a byte a slot and 256 records
GATHER_CELLS = [(RAW, None), (RAW, 32), (MT, 32), (BLOCK, 32)]
SHARED_KIND = {11: 3, 12: 3, 14: 4, 15: 4}  # raw plans carry a host-built table: the 8-byte one, the rank table from 14 bits


@gpu
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits", GATHER_BITS)
@pytest.mark.parametrize("container,index", GATHER_CELLS, ids=("raw", "raw32", "mt32", "block32"))
def test_gather_matrix(gpu_ctx, oracle, container, index, states, bits):
    """k_gather / k_gather_ranges, both table placements: 300 random ranges and the ranges around the edge of a hot stretch; a range in a cold
    stretch behind a hot one is reached through gather_advance / the non-storing skip at both rates"""
    d, s, plan, edges = _gather_member(gpu_ctx, container, states, bits, index)
    want = oracle_bytes(oracle, container, states, bits, s, plan, d)
    dplan, d_stream = gpu_ctx.make_device_plan(plan), _upload(s)
    kind = _gather_kind(gpu_ctx, dplan, d_stream, s.size)
    # (a raw plan with an index carries a host-built table, one per workgroup; every other plan's waves build their own)
    assert kind == (SHARED_KIND[bits] if container == RAW and index else PRIVATE_KIND[bits]), kind
    rng = np.random.default_rng(1000 * container + 10 * states + bits)
    src = _random_src(rng, 300, d.size, 1 << (14 if index is None else 17)) + edges
    _gather_both_ways(gpu_ctx, dplan, d_stream, s.size, want, src)


@gpu
def test_gather_of_the_tail_of_a_hot_stream_without_an_index(gpu_ctx, oracle):
    """the last 100 bytes of 1,000,003: the longest run of gather_advance at full rate (15,623 groups decoded and not stored)"""
    d, s, plan = raw_case("hot", N_TAIL, 64, 11)
    want = oracle_bytes(oracle, RAW, 64, 11, s, plan, d)
    dplan, d_stream = gpu_ctx.make_device_plan(plan), _upload(s)
    assert H.plan_chain_count(plan) == 1 and _gather_kind(gpu_ctx, dplan, d_stream, s.size) == 0
    _gather_both_ways(gpu_ctx, dplan, d_stream, s.size, want, [(N_TAIL - 100, 100)])


@gpu
def _spilled_member(ctx, monkeypatch):
    """a raw plan whose decode table stays in global memory (HSRANS_TABLE_SPILL=1, read when a device plan is made): the sixth gather kind"""
    d, s, plan, edges = _gather_member(ctx, RAW, 64, 15, 32)
    monkeypatch.setenv("HSRANS_TABLE_SPILL", "1")
    dplan = ctx.make_device_plan(plan)
    monkeypatch.delenv("HSRANS_TABLE_SPILL")
    return d, s, plan, edges, dplan


@gpu
def test_gather_with_the_table_in_global_memory(gpu_ctx, oracle, monkeypatch):
    d, s, plan, edges, dplan = _spilled_member(gpu_ctx, monkeypatch)
    want = oracle_bytes(oracle, RAW, 64, 15, s, plan, d)
    d_stream = _upload(s)
    assert _gather_kind(gpu_ctx, dplan, d_stream, s.size) == 5
    _gather_both_ways(gpu_ctx, dplan, d_stream, s.size, want, _random_src(np.random.default_rng(5), 300, d.size, 1 << 17) + edges)


@gpu
def test_gather_set_with_a_member_of_every_kind(gpu_ctx, oracle, monkeypatch):
    """k_gather_set / k_set_ranges: one member per table layout (all six kinds: the five the matrix above reaches and the table in global
    memory), ranges on the host and on the device"""
    import torch
    d, s, plan, edges, dplan = _spilled_member(gpu_ctx, monkeypatch)
    d_stream = _upload(s)
    by_kind = {_gather_kind(gpu_ctx, dplan, d_stream, s.size): (oracle_bytes(oracle, RAW, 64, 15, s, plan, d), s.size, dplan, d_stream, edges, 32)}
    for container, index in GATHER_CELLS:
        for states in (64, 32):
            for bits in GATHER_BITS:
                d, s, plan, edges = _gather_member(gpu_ctx, container, states, bits, index)
                dplan, d_stream = gpu_ctx.make_device_plan(plan), _upload(s)
                kind = _gather_kind(gpu_ctx, dplan, d_stream, s.size)
                if kind not in by_kind:
                    by_kind[kind] = (oracle_bytes(oracle, container, states, bits, s, plan, d), s.size, dplan, d_stream, edges, index)
    assert sorted(by_kind) == list(range(6)), sorted(by_kind)
    members = [by_kind[k] for k in range(6)]
    gset = gpu_ctx.make_gather_set([m[2] for m in members], [m[3] for m in members], [m[1] for m in members])
    assert gset.info()["kind_members"] == [1] * 6
    rng = np.random.default_rng(6)
    src = []
    for k, m in enumerate(members):
        src += [(k,) + r for r in _random_src(rng, 60, m[0].size, 1 << (14 if m[5] is None else 16)) + m[4]]
    order = rng.permutation(len(src))
    rows, size = _rows([src[i] for i in order])
    want = np.full(size, 0xCC, np.uint8)
    for k, off, length, dst in rows:
        want[dst:dst + length] = members[k][0][off:off + length]
    for launch in range(2):
        dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
        gpu_ctx.decode_device_gather_batch(gset, rows, dst)
        torch.cuda.synchronize()
        _check_dst(dst.cpu().numpy(), want, rows)
        assert gpu_ctx.gather_set_status(gset) == [0] * 6
        info = gset.info()
        assert info["launches"] == 6 and all(info["kind_tasks"]), info
    dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
    d_rows = torch.from_numpy(np.array([(off, length, at, k) for k, off, length, at in rows], np.int64)).cuda()
    gpu_ctx.decode_device_gather_batch_indirect(gset, d_rows, dst)
    torch.cuda.synchronize()
    _check_dst(dst.cpu().numpy(), want, rows)
    assert gpu_ctx.gather_set_status(gset) == [0] * 6 and gpu_ctx.gather_set_refused(gset) == 0
    assert gset.info()["launches"] == 6


# ---- the rest ----
@gpu
def test_window_and_ranges_decode_over_slices_of_a_mixed_plan(gpu_ctx, oracle):
    """decode_device_window / decode_device_ranges: every rank of three holds its window of the stream (and of the output) only"""
    import torch
    from hypersonic_rans_amd import sharded
    container, states, bits, n = WINDOW[:4]
    d, stream, plan = mixed_case(*WINDOW)
    want = oracle_bytes(oracle, container, states, bits, stream, plan, d)
    buf = torch.full((n + GUARD,), 0xCC, dtype=torch.uint8, device="cuda")
    for first, count in sharded.shard_chains(plan, 3):
        (hb, he), (bb, be) = H.plan_stream_ranges(plan, first, count)
        lo = bb & ~15
        window = torch.full((be - lo + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        window[bb - lo: be - lo] = torch.from_numpy(stream[bb:be]).cuda()
        dplan = gpu_ctx.make_device_plan(H.plan_slice(plan, first, count))
        for _ in range(2):
            gpu_ctx.decode_device_window(dplan, window, lo, be - lo, buf[:n])
            assert gpu_ctx.status(dplan) == 0
        assert dplan.launch_info()["chains"] == count
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n], want) and (got[n:] == 0xCC).all()
    layout = sharded.ShardLayout(plan, 3, parts=2)
    for rank in range(3):
        b, e = layout.ranges[rank]
        lo, hi = layout.windows[rank]
        window = torch.full((hi - lo + 16,), 0xEE, dtype=torch.uint8, device="cuda")
        window[:hi - lo] = torch.from_numpy(stream[lo:hi]).cuda()
        buf = torch.full((GUARD + e - b + GUARD,), 0xCC, dtype=torch.uint8, device="cuda")
        for f, c in layout.sub_runs[rank]:
            dplan = gpu_ctx.make_device_plan(H.plan_slice(plan, f, c))
            for _ in range(2):
                gpu_ctx.decode_device_ranges(dplan, window, lo, hi - lo, buf[GUARD:GUARD + e - b], b, e - b)
                assert gpu_ctx.status(dplan) == 0
            assert dplan.launch_info()["chains"] == c
        got = buf.cpu().numpy()
        assert np.array_equal(got[GUARD:GUARD + e - b], want[b:e]), rank
        assert (got[:GUARD] == 0xCC).all() and (got[GUARD + e - b:] == 0xCC).all(), f"rank {rank} wrote outside its output window"


@gpu
def test_pipelined_host_decode_in_three_slices(gpu_ctx, oracle):
    import torch
    from hypersonic_rans_amd import pipeline
    container, states, bits, n = PIPELINE[:4]
    d, stream, plan = mixed_case(*PIPELINE)
    want = oracle_bytes(oracle, container, states, bits, stream, plan, d)
    host_stream = torch.from_numpy(stream).pin_memory()
    host_out = torch.full((n + GUARD,), 0xCC, dtype=torch.uint8).pin_memory()
    dec = pipeline.PipelinedHostDecoder(gpu_ctx, plan, n_slices=3)
    for launch in range(2):
        host_out[:n].fill_(0x33)
        dec.decode(host_stream, host_out[:n])
        got = host_out.numpy()
        assert np.array_equal(got[:n], want) and (got[n:] == 0xCC).all(), launch
    dec.close()


@gpu
def test_a_ranks_sub_runs_in_one_dealt_launch(gpu_ctx, oracle, monkeypatch):
    """k_decode_dealt<true, true>: a rank's four sub-runs in one launch, each announced by its completion word; a second stream copies every
    sub-run away as soon as its word fires"""
    import torch
    from hypersonic_rans_amd import sharded
    monkeypatch.setenv("HSRANS_SHARD_ONE_LAUNCH", "1")
    container, states, bits, n = SUB_RUNS[:4]
    d, stream, plan = mixed_case(*SUB_RUNS)
    want = torch.from_numpy(oracle_bytes(oracle, container, states, bits, stream, plan, d)).cuda()
    world, parts = 2, 4
    side = torch.cuda.Stream()
    for rank in range(world):
        dec = sharded.ShardedDecoder(gpu_ctx, plan, parts=parts, world=world, rank=rank)
        assert bool(dec.c.info["one_launch"])
        d_window = dec.upload_window(stream, "cuda")
        out = dec.alloc_out("cuda")
        for rep in range(2):
            out.fill_(0xA5)
            copy = torch.full_like(out, 0x5A)
            torch.cuda.synchronize()
            dec.step(d_window, out, gather=False)
            for k in reversed(range(parts)) if rep & 1 else range(parts):
                b, e = dec.layout.sub_ranges[rank][k]
                if e > b:
                    dec.c.wait_part(k, side)
                    with torch.cuda.stream(side):
                        copy[b:e].copy_(out[b:e], non_blocking=True)
            side.synchronize()
            b, e = dec.ranges[rank]
            assert torch.equal(copy[b:e], want[b:e]), (rank, rep)
            torch.cuda.synchronize()
            dec.check()
            other = out.clone()
            other[b:e] = 0xA5
            assert bool((other == 0xA5).all()), f"rank {rank} wrote outside its range"
        assert dec.launch_info()["spread"] == 2


@gpu
@pytest.mark.parametrize("store", (False, True), ids=("coded", "store"))
def test_planes_of_a_tensor_whose_byte_planes_are_extreme(gpu_ctx, oracle, store):
    """uint16 elements: the low-byte plane is mixed_blocks data, the high-byte plane idle; the frame's coded planes against the oracle, the
    round trip, and element ranges through decode_device_planes_gather"""
    import torch
    n, block = PLANES_N, PLANES_BLOCK
    low, high = planes_low(), planes_high()
    a = (low.astype(np.uint16) | (high.astype(np.uint16) << 8)).astype(np.uint16)
    t = torch.from_numpy(a.view(np.int16)).cuda()
    frame = torch.full((H.planes_capacity(2, 64, n),), 0xA5, dtype=torch.uint8, device="cuda")
    work = torch.full((H.planes_workspace_bytes(2, n),), 0xA5, dtype=torch.uint8, device="cuda")
    total, desc, plans = gpu_ctx.encode_device_planes(t, frame, work, states=64, bits=11, block_size=block, index_interval=4, store_incompressible=store)
    assert all(p is not None for p in plans)  # (both planes compress: neither is stored)
    host_frame = frame.cpu().numpy()
    for p, plane in enumerate((low, high)):
        s = host_frame[desc.offset[p]:desc.offset[p] + desc.length[p]]
        r, back = oracle.decode(MT, 64, 11, s, n)
        assert r == n and np.array_equal(back, plane), p
    planes = gpu_ctx.make_planes(desc, plans)
    info = planes.info()
    assert info["coded"] == 2 and info["stored"] == 0
    out = torch.full((n + GUARD,), -1, dtype=torch.int16, device="cuda")
    for launch in range(2):
        out[:n].fill_(0)
        gpu_ctx.decode_device_planes(planes, frame, out[:n], torch.full_like(work, 0xA5))
        assert gpu_ctx.planes_status(planes) == [0, 0]
        got = out.cpu().numpy().view(np.uint16)
        assert np.array_equal(got[:n], a) and (got[n:] == 0xFFFF).all(), launch
    pg = gpu_ctx.make_planes_gather(planes, frame)
    rng = np.random.default_rng(50)
    b, e = R.mixed_stretch(1, block, block, 11)
    src = _random_src(rng, 43, n, 1 << 14) + _edge_src((block + b, block + e), (block + e, 2 * block))
    assert len(src) == 50
    ranges, at = [], 16
    for off, length in src:
        ranges.append((off, length, at))
        at += length
    want = np.full(at + 16, 0xA5A5, np.uint16)
    for off, length, dst in ranges:
        want[dst:dst + length] = a[off:off + length]
    d_out = torch.full((2 * (at + 16),), 0xA5, dtype=torch.uint8, device="cuda")
    g_work = torch.full((H.planes_gather_workspace_bytes(2, len(ranges), sum(r[1] for r in ranges)) + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    for launch in range(2):
        gpu_ctx.decode_device_planes_gather(pg, ranges, d_out.view(torch.int16), g_work)
        assert gpu_ctx.planes_gather_status(pg) == [0, 0]
        assert np.array_equal(d_out.cpu().numpy().view(np.uint16), want), launch
    assert pg.info()["rows"] == 2 * len(ranges)
    pg.close()
    planes.close()


# ---- the encoders at the same extremes ----
@gpu
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits", (11, 15))
def test_raw_encoder_on_the_device(gpu_ctx, oracle, states, bits):
    """encode_device_raw under hot_hist: every lane emits a word at every step of a hot stretch, none in the cold rest; stream and plan byte
    for byte the host encoder's, and the device-built plan decodes"""
    import torch
    hist = R.hot_hist(bits)
    for kind in ("hot", "cold", "alternating"):
        for index in (None, 4):
            d, s, plan = raw_case(kind, N_ENC, states, bits, index)
            want = oracle_bytes(oracle, RAW, states, bits, s, plan, d)
            d_in = torch.from_numpy(d).cuda()
            d_out = torch.full((R.raw_room(N_ENC) + GUARD,), 0xCC, dtype=torch.uint8, device="cuda")
            if index is None:
                m = gpu_ctx.encode_device_raw(states, bits, d_in, d_out[:R.raw_room(N_ENC)], hist=hist)
                dplan = gpu_ctx.make_device_plan(plan)
            else:
                m, got_plan, dplan = gpu_ctx.encode_device_raw(states, bits, d_in, d_out[:R.raw_room(N_ENC)], hist=hist, index_interval=index, want_plan=True,
                                                               want_device_plan=True)
                assert np.array_equal(got_plan, plan), (kind, index)
            got = d_out.cpu().numpy()
            assert m == s.size and np.array_equal(got[:m], s), (kind, index, m, s.size)
            assert (got[R.raw_room(N_ENC):] == 0xCC).all()
            stream_dev = torch.cat([d_out[:m], torch.zeros((-m) % 16 + 16, dtype=torch.uint8, device="cuda")])
            info = _decode_twice(gpu_ctx, dplan, s, want, d_in=stream_dev)
            assert info["chains"] == H.plan_chain_count(plan), info


@gpu
@pytest.mark.parametrize("container", (MT, BLOCK), ids=("mt", "block"))
@pytest.mark.parametrize("block", (1 << 14, 1 << 17))
def test_container_encoders_on_the_device(gpu_ctx, oracle, container, block):
    """encode_device (mt_, independent blocks) and encode_device_ex on mixed_blocks data: byte for byte the host encoder's stream and plan;
    the device-built plans decode"""
    import torch
    n, bits, interval = 1_000_003, 11, 4
    d = mixed_case(container, 64, bits, n, block, interval)[0]
    d_in = torch.from_numpy(d).cuda()
    cap = H.capacity(container, 64, n)
    runs = [("ex", dict())]
    if container == MT:
        runs.append(("plain", dict(independent_blocks=True)))
    for name, kw in runs:
        s, plan = H.encode(container, 64, bits, d, index_interval=interval, block_size=block, **kw)
        want = oracle_bytes(oracle, container, 64, bits, s, plan, d)
        d_out = torch.full((cap + GUARD,), 0xCC, dtype=torch.uint8, device="cuda")
        if name == "ex":
            m, got_plan, dplan = gpu_ctx.encode_device_ex(container, 64, bits, d_in, d_out[:cap], block_size=block, index_interval=interval, want_plan=True,
                                                          want_device_plan=True)
        else:
            m, dplan = gpu_ctx.encode_device(container, 64, bits, d_in, d_out[:cap], block_size=block, index_interval=interval, want_plan=True)
            got_plan = gpu_ctx.read_device_plan(dplan, capacity=plan.size + 4096)
        got = d_out.cpu().numpy()
        assert m == s.size and np.array_equal(got[:m], s), (name, m, s.size)
        assert (got[cap:] == 0xCC).all()
        assert np.array_equal(got_plan, plan), name
        info = _decode_twice(gpu_ctx, dplan, s, want, d_in=d_out)
        assert info["chains"] == H.plan_chain_count(plan) and info["shared_table"] == 1, info
