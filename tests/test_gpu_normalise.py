"""The count normalisation of every GPU encoder (csrc/enc_normalise.h: the reference's heap sort replayed in registers, its three
extraction forms, its two heap builds, the closed-form steal and charity passes) on blocks DESIGNED for it (normalise_inputs.py): every
depth of the sort, tied and untied cuts on either side of each change of extraction form, many steal passes, deep charity.

A wrong tie or a wrong lane gives counts that still sum to 2^bits and a stream our own decoder still reads back, so every test here compares
with the host encoder byte for byte (its normalisation is pinned to the oracle on every designed block and to the real reference on the
boundary ones: test_normalise_host.py); the oracle's decoder must also give the input back.

The sites that normalise: k_encode_blocks<S, 4096> and <S, 2048> (encode_device) and k_encode_blocks_batch, with the parallel heap build in
LDS; k_encode_raw<S> and k_encode_raw_batch<S>, with the register build (heap_sift<>); k_unit_costs and k_unit_costs_batch
(unit_costs_body) for the adaptive walk of encode_device_ex and block_choices_device.  The chain kernels code with the counts the walk
hands them, and of the unit-cost kernels' normalisation only the cost reaches the host: a wrong tie there shows where it turns a decision
of the walk, not otherwise (there is no entry that returns the costs)."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
import normalise_inputs as N
from oracle_lib import BLOCK, MT, RAW

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
CHUNK_BLOCKS_PER_CU = 11  # hsrans_encode.hip chunk_variant: more than 11 x CUs blocks in a launch take the 2 KiB-chunk kernel


def _dev(data):
    return torch.from_numpy(np.ascontiguousarray(data)).cuda()


def _out(container, states, n):
    return torch.full((H.capacity(container, states, n),), SENTINEL, dtype=torch.uint8, device="cuda")


def test_designed_blocks_reach_what_they_claim():
    """(on the arithmetic alone, before any GPU result is looked at; the same check as the host test's)"""
    N.check_coverage()


# ---- what went wrong, in the words of the design -------------------------------------------------------------------------------------
def mt_blocks(stream, states):
    """(offset, counts or None for a single-symbol block) of every block image of an mt_ stream"""
    out, o = [], 16
    while o + 8 <= stream.size:
        v = int(stream[o: o + 8].view("<u8")[0])
        if v >> 63:
            out.append((o, None))
            o += 8
            continue
        if o + 16 + 4 * states + 512 > stream.size:
            break
        skip = int(stream[o + 8: o + 16].view("<u8")[0])
        out.append((o, stream[o + 16 + 4 * states: o + 16 + 4 * states + 512].view("<u2").astype(np.int64)))
        o += 16 + 2 * (skip + 1)
    return out


def first_difference(got, want, states, blocks, bits):
    """names the first block whose image differs: its class from `arith` and where the two histograms differ (symbol: gpu / host)"""
    n = min(got.size, want.size)
    at = int(np.argmax(got[:n] != want[:n])) if (got[:n] != want[:n]).any() else n
    host = mt_blocks(want, states)
    k = max(0, sum(1 for o, _ in host if o <= at) - 1)
    text = f"streams of {got.size} / {want.size} bytes differ first at byte {at}, in block {k}"
    if k < len(blocks):
        raw = np.bincount(blocks[k], minlength=256)
        kind, take, jf, tie = N.arith(raw, blocks[k].size, bits)
        text += f" ({blocks[k].size} bytes, {int((raw != 0).sum())} symbols: {kind} take={take} j/full={jf} {'TIED' if tie else 'untied'} cut)"
    try:
        gpu = mt_blocks(got, states)
        a, b = gpu[k][1], host[k][1]
        where = np.nonzero(a != b)[0]
        text += f"; histograms differ at {len(where)} symbols: " + ", ".join(f"{s}: {a[s]} / {b[s]}" for s in where[:12]) + (" (sum %d)" % a.sum())
    except Exception as e:  # (a stream too broken to walk)
        text += f"; the GPU stream's block headers cannot be walked ({type(e).__name__})"
    return text


_cache = {}


def host_mt(states, bits, size):
    key = ("host", states, bits, size)
    if key not in _cache:
        d = N.blocks(bits, size)
        _cache[key] = H.encode(MT, states, bits, d.concatenated(), block_size=size, independent_blocks=True, index_interval=4)
    return _cache[key]


def gpu_mt(ctx, states, bits, size):
    """(stream, plan) of encode_device on the setting's concatenated blocks, checkpoints every 4 groups"""
    key = ("gpu", states, bits, size)
    if key not in _cache:
        data = N.blocks(bits, size).concatenated()
        d_in, d_out = _dev(data), _out(MT, states, data.size)
        m, dplan = ctx.encode_device(MT, states, bits, d_in, d_out, block_size=size, index_interval=4, want_plan=True)
        _cache[key] = (d_out[:m].cpu().numpy(), ctx.read_device_plan(dplan))
    return _cache[key]


# ---- encode_device: k_encode_blocks<S, 4096>, the parallel LDS heap build --------------------------------------------------------------
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits,size", N.SETTINGS)
def test_independent_blocks(gpu_ctx, oracle, states, bits, size):
    d = N.blocks(bits, size)
    data = d.concatenated()
    want, want_plan = host_mt(states, bits, size)
    got, got_plan = gpu_mt(gpu_ctx, states, bits, size)
    assert got.size == want.size and np.array_equal(got, want), first_difference(got, want, states, d.data, bits)
    assert got_plan.size == want_plan.size and np.array_equal(got_plan, want_plan), (states, bits, size)
    r, back = oracle.decode(MT, states, bits, got, data.size)
    assert r == data.size and np.array_equal(back, data), (states, bits, size)


@pytest.mark.parametrize("states", (32, 64))
def test_independent_blocks_in_2k_chunks(gpu_ctx, oracle, states):
    """more blocks than 11 x CUs in one launch: k_encode_blocks<S, 2048> normalises too — every 4160-byte block of every width, at 11 bits"""
    threshold = CHUNK_BLOCKS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    blocks = [b for bits in range(10, 16) for b in N.blocks(bits, 4160).data[:-1]]
    blocks = (blocks * (threshold // len(blocks) + 1))[: threshold + 64]
    assert len(blocks) > threshold
    data = np.concatenate(blocks)
    want = H.encode(MT, states, 11, data, block_size=4160, independent_blocks=True)
    d_in, d_out = _dev(data), _out(MT, states, data.size)
    m = gpu_ctx.encode_device(MT, states, 11, d_in, d_out, block_size=4160)
    got = d_out[:m].cpu().numpy()
    assert got.size == want.size and np.array_equal(got, want), first_difference(got, want, states, blocks, 11)
    r, back = oracle.decode(MT, states, 11, got, data.size)
    assert r == data.size and np.array_equal(back, data)


@pytest.mark.parametrize("bits", (10, 15))
def test_a_block_whose_counts_float32_does_not_hold(gpu_ctx, oracle, bits):
    """2^25 + 64 bytes in one block, an odd dominant count above 2^24: (float)count rounds before the scale does"""
    data = N.huge_block()
    kind, take, _, tie = N.arith(np.bincount(data, minlength=256), data.size, bits)
    assert kind != "none" and take > 0 and tie, (kind, take, tie)
    want = H.encode(MT, 64, bits, data, block_size=N.HUGE, independent_blocks=True)
    d_in, d_out = _dev(data), _out(MT, 64, data.size)
    m = gpu_ctx.encode_device(MT, 64, bits, d_in, d_out, block_size=N.HUGE)
    got = d_out[:m].cpu().numpy()
    assert got.size == want.size and np.array_equal(got, want), first_difference(got, want, 64, [data], bits)
    r, back = oracle.decode(MT, 64, bits, got, data.size)
    assert r == data.size and np.array_equal(back, data)


# ---- encode_device_raw: k_encode_raw<S>, the register heap build (heap_sift<>) ----------------------------------------------------------
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits", N.RAW_BITS)
def test_raw_streams_of_one_designed_block(gpu_ctx, oracle, states, bits):
    subset = N.raw_subset(bits)
    kinds = {(kind, take) for _, (kind, take, _, _) in subset}
    assert {("steal", t) for t in N.BOUNDARY_TAKES} <= kinds and ("steal", 1) in kinds and ("none", 0) in kinds, sorted(kinds)
    assert {("charity", t) for t in N.RAW_CHARITY_TAKES} <= kinds and len(subset) <= 24, sorted(kinds)
    for block, info in subset:
        want = H.encode(RAW, states, bits, block)
        d_in, d_out = _dev(block), _out(RAW, states, block.size)
        m = gpu_ctx.encode_device_raw(states, bits, d_in, d_out)
        got = d_out[:m].cpu().numpy()
        if not (got.size == want.size and np.array_equal(got, want)):
            a, b = got[16: 16 + 512].view("<u2").astype(np.int64), want[16: 16 + 512].view("<u2").astype(np.int64)
            where = np.nonzero(a != b)[0] if got.size >= 528 else []
            pytest.fail(f"S={states} bits={bits} {block.size} bytes, class {info}: {got.size} / {want.size} bytes; histograms (gpu / host) differ at "
                        + ", ".join(f"{s}: {a[s]} / {b[s]}" for s in where[:12]))
        r, back = oracle.decode(RAW, states, bits, got, block.size)
        assert r == block.size and np.array_equal(back, block), (states, bits, info)


# ---- block_choices_device and encode_device_ex: k_unit_costs and k_encode_chain<S> -----------------------------------------------------
def gpu_ex(ctx, container, states, bits, size, block_size):
    key = ("ex", container, states, bits, size, block_size)
    if key not in _cache:
        data = N.blocks(bits, size).concatenated()
        d_in, d_out = _dev(data), _out(container, states, data.size)
        m = ctx.encode_device_ex(container, states, bits, d_in, d_out, block_size=block_size)
        _cache[key] = d_out[:m].cpu().numpy()
    return _cache[key]


@pytest.mark.parametrize("container", (BLOCK, MT))
@pytest.mark.parametrize("states", (32, 64))
def test_block_choices_and_carried_state_streams(gpu_ctx, oracle, container, states):
    for bits, size in N.SETTINGS:
        d = N.blocks(bits, size)
        data = d.concatenated()
        d_in = _dev(data)
        for block_size in (size, 0):
            what = (container, states, bits, size, block_size)
            want = H.block_choices(container, states, bits, data, block_size=block_size)
            got = gpu_ctx.block_choices_device(container, states, bits, d_in, block_size=block_size)
            assert got.size == want.size, what
            for field in ("begin", "end", "single", "symbol", "counts"):
                same = got[field] == want[field] if field != "counts" else (got[field] == want[field]).all(axis=1)
                k = int(np.argmin(same))
                assert same.all(), (what, field, f"choice {k}", N.describe(d, k) if block_size and k < len(d.data) else "", got[field][k], want[field][k])
            stream = gpu_ex(gpu_ctx, container, states, bits, size, block_size)
            host = H.encode(container, states, bits, data, block_size=block_size)
            assert stream.size == host.size and np.array_equal(stream, host), (what, int(np.argmax(stream[:host.size] != host[:stream.size])))
            r, back = oracle.decode(container, states, bits, stream, data.size)
            assert r == data.size and np.array_equal(back, data), what


# ---- the batch forms: k_encode_blocks_batch, k_encode_chain_batch, k_unit_costs_batch ---------------------------------------------------
def test_batch_members_equal_their_single_calls(gpu_ctx):
    """one call: every setting as an mt_ member (k_encode_blocks_batch), and the raw kernel's blocks as raw members (k_encode_raw_batch has
    the register heap build too)"""
    specs = [(32 if k % 2 else 64, bits, size) for k, (bits, size) in enumerate(N.SETTINGS)]
    raws = [(32 if k % 2 else 64, bits, block, info) for bits in N.RAW_BITS for k, (block, info) in enumerate(N.raw_subset(bits))]
    ins = [_dev(N.blocks(bits, size).concatenated()) for _, bits, size in specs] + [_dev(block) for _, _, block, _ in raws]
    outs = [_out(MT, spec[0], d_in.numel()) for spec, d_in in zip(specs, ins)] + [_out(RAW, states, block.size) for states, _, block, _ in raws]
    members = [(MT, states, bits, ins[k], outs[k], {"block_size": size, "index_interval": 4}) for k, (states, bits, size) in enumerate(specs)]
    members += [(RAW, states, bits, ins[len(specs) + k], outs[len(specs) + k]) for k, (states, bits, _, _) in enumerate(raws)]
    lengths, plans = gpu_ctx.encode_device_batch(members, want_plans=True)
    for k, (states, bits, size) in enumerate(specs):
        want, want_plan = gpu_mt(gpu_ctx, states, bits, size)
        got = outs[k][: lengths[k]].cpu().numpy()
        assert got.size == want.size and np.array_equal(got, want), first_difference(got, want, states, N.blocks(bits, size).data, bits)
        assert np.array_equal(gpu_ctx.read_device_plan(plans[k]), want_plan), (states, bits, size)
    for k, (states, bits, block, info) in enumerate(raws):
        got = outs[len(specs) + k][: lengths[len(specs) + k]].cpu().numpy()
        want = H.encode(RAW, states, bits, block)  # (what the single call gives: test_raw_streams_of_one_designed_block)
        assert got.size == want.size and np.array_equal(got, want), (states, bits, block.size, info)


def test_ex_batch_members_equal_their_single_calls(gpu_ctx):
    """block_size 0: the adaptive walk's unit costs, for every member in one launch of k_unit_costs_batch (unit_costs_body)"""
    specs = []
    for k, (bits, size) in enumerate(N.SETTINGS):
        specs.append((MT if k % 2 else BLOCK, 32 if k % 4 < 2 else 64, bits, size, 0))
        specs.append((BLOCK if k % 2 else MT, 64 if k % 4 < 2 else 32, bits, size, size if k % 3 else 0))
    ins = [_dev(N.blocks(bits, size).concatenated()) for _, _, bits, size, _ in specs]
    outs = [_out(c, states, d_in.numel()) for (c, states, _, _, _), d_in in zip(specs, ins)]
    members = [(c, states, bits, ins[k], outs[k], {"block_size": block_size}) for k, (c, states, bits, size, block_size) in enumerate(specs)]
    lengths = gpu_ctx.encode_device_ex_batch(members)
    for k, (c, states, bits, size, block_size) in enumerate(specs):
        want = gpu_ex(gpu_ctx, c, states, bits, size, block_size)
        got = outs[k][: lengths[k]].cpu().numpy()
        assert got.size == want.size and np.array_equal(got, want), (specs[k], int(np.argmax(got[:want.size] != want[:got.size])))
        assert np.array_equal(want, H.encode(c, states, bits, N.blocks(bits, size).concatenated(), block_size=block_size)), specs[k]
