"""hsrans_encode_host_pipelined: host bytes in, an mt_ stream (and plan) in host memory out, encoded on the GPU slice by slice with the
PCIe legs overlapped — byte for byte against the host encoder (hsrans_encode_ex, independent blocks) and against hsrans_encode_device on
the same bytes in HBM, for pinned and pageable buffers, decoded back by hsrans_decode_host_pipelined and by the oracle's mt_ decoder."""
import ctypes

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth
from oracle_lib import MT

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def zipf():
    return synth.enwik8_shaped(32 << 20, seed=17)


def host_buf(n, pinned, fill=None, data=None):
    """a CPU uint8 buffer of n bytes: a pinned torch tensor or a pageable numpy array"""
    if pinned:
        t = torch.empty(n, dtype=torch.uint8).pin_memory()
        if data is not None:
            t.copy_(torch.from_numpy(np.ascontiguousarray(data)))
        elif fill is not None:
            t.fill_(fill)
        return t
    a = np.empty(n, np.uint8)
    if data is not None:
        a[:] = data
    elif fill is not None:
        a[:] = fill
    return a


def as_np(buf):
    return buf.numpy() if isinstance(buf, torch.Tensor) else buf


def pipelined(ctx, states, bits, data, block, interval=0, n_slices=0, pin_in=True, pin_out=True):
    """stream (np), plan (np or None); checks that nothing past the stream's end was written"""
    src = host_buf(data.size, pin_in, data=data)
    out = host_buf(H.capacity(MT, states, data.size), pin_out, fill=SENTINEL)
    m, plan = ctx.encode_host_pipelined(states, bits, src, out, block_size=block, index_interval=interval, n_slices=n_slices)
    o = as_np(out)
    assert np.all(o[m:] == SENTINEL), "bytes past the returned length were written"
    return o[:m].copy(), plan


def host_encoder(states, bits, data, block, interval=0):
    r = H.encode(MT, states, bits, data, block_size=block, index_interval=interval, independent_blocks=True)
    return r if isinstance(r, tuple) else (r, None)


def check_identical(ctx, states, bits, data, block, interval, n_slices):
    want, want_plan = host_encoder(states, bits, data, block, interval)
    got, plan = pipelined(ctx, states, bits, data, block, interval, n_slices)
    assert got.size == want.size and np.array_equal(got, want), (states, bits, block, interval, n_slices, data.size)
    if interval:
        assert plan is not None and np.array_equal(plan, want_plan), ("plan", states, bits, block, interval, n_slices, data.size)
    else:
        assert plan is None


# (states, bits, block, interval, n_slices, length): every state count and width, three block sizes (one an odd multiple of 64), the
# slicings 0 / 1 / 2 / 3 / 7, lengths that are not multiples of the block or of the state count
CASES = [
    (64, 11, 1 << 16, 0, 0, 32 << 20),
    (64, 11, 1 << 16, 32, 0, (32 << 20) - 12345),
    (64, 10, 1 << 16, 4, 3, 5_000_017),
    (32, 12, 1 << 18, 32, 2, 9_999_999),
    (32, 14, 64 * 1001, 0, 7, 7_654_321),
    (64, 15, 64 * 1001, 32, 7, 3_000_037),
    (64, 14, 1 << 18, 0, 1, 2_621_440),
    (32, 11, 1 << 16, 4, 3, 1_000_003),
    (32, 15, 1 << 16, 32, 0, 4_194_303),
    (64, 12, 64 * 1001, 4, 2, 6_400_065),
]


@pytest.mark.parametrize("states,bits,block,interval,n_slices,length", CASES)
def test_byte_identical_to_the_host_encoder(gpu_ctx, zipf, states, bits, block, interval, n_slices, length):
    check_identical(gpu_ctx, states, bits, zipf[:length], block, interval, n_slices)


@pytest.mark.parametrize("interval", [0, 4, 32])
@pytest.mark.parametrize("n_slices", [0, 1, 3])
def test_input_smaller_than_one_block(gpu_ctx, zipf, interval, n_slices):
    for states, length in ((64, 40_001), (32, 31), (64, 65)):
        check_identical(gpu_ctx, states, 11, zipf[:length], 1 << 16, interval, n_slices)


@pytest.mark.parametrize("interval", [0, 4, 32])
@pytest.mark.parametrize("n_slices", [0, 2, 7])
def test_single_symbol_blocks(gpu_ctx, zipf, interval, n_slices):
    """constant runs: single-symbol blocks (marker only, one fill chain each) inside and at the ends of slices"""
    b = 1 << 16
    data = np.concatenate([np.full(3 * b, 7, np.uint8), zipf[: 2 * b + 999], np.full(4 * b - 999, 200, np.uint8), zipf[: b + 5],
                           np.full(2 * b + 77, 9, np.uint8)])
    for states in (32, 64):
        check_identical(gpu_ctx, states, 12, data, b, interval, n_slices)


@pytest.mark.parametrize("interval", [0, 4, 32])
@pytest.mark.parametrize("n_slices", [0, 3, 7])
def test_exactly_one_coded_block(gpu_ctx, zipf, interval, n_slices):
    """one block carries a histogram, every other is a single-symbol block: the plan's shared_hist / aux_off case"""
    b = 1 << 16
    data = np.concatenate([np.full(3 * b, 1, np.uint8), zipf[:b], np.full(3 * b + 4321, 2, np.uint8)])
    for states in (32, 64):
        check_identical(gpu_ctx, states, 11, data, b, interval, n_slices)


def test_identical_to_the_device_encoder_at_256_mib(gpu_ctx):
    n = 256 << 20
    data = synth.enwik8_shaped(n, seed=23)
    d_in = torch.from_numpy(data).cuda()
    d_out = torch.empty(H.capacity(MT, 64, n), dtype=torch.uint8, device="cuda")
    m, dplan = gpu_ctx.encode_device(MT, 64, 11, d_in, d_out, block_size=1 << 16, index_interval=32, want_plan=True)
    want = d_out[:m].cpu().numpy()
    want_plan = gpu_ctx.read_device_plan(dplan, capacity=H.load_library().hsrans_plan_capacity(MT, 64, n, 32, 1 << 16))
    del d_in, d_out
    got, plan = pipelined(gpu_ctx, 64, 11, data, 1 << 16, 32, 0)
    assert got.size == m and np.array_equal(got, want)
    assert np.array_equal(plan, want_plan)
    got0, plan0 = pipelined(gpu_ctx, 64, 11, data, 1 << 16, 0, 0)
    assert plan0 is None and np.array_equal(got0, want)


def test_pinned_pageable_and_mixed_buffers_give_the_same_bytes(gpu_ctx, zipf):
    data = zipf[: 20_000_003]
    want, want_plan = host_encoder(64, 11, data, 1 << 16, 32)
    for pin_in, pin_out in ((True, True), (False, False), (True, False), (False, True)):
        got, plan = pipelined(gpu_ctx, 64, 11, data, 1 << 16, 32, 4, pin_in=pin_in, pin_out=pin_out)
        assert np.array_equal(got, want) and np.array_equal(plan, want_plan), (pin_in, pin_out)


@pytest.mark.parametrize("states", [32, 64])
def test_round_trip_through_the_decode_pipeline_and_the_oracle(gpu_ctx, oracle, zipf, states):
    data = zipf[: 12_345_679]
    stream, plan = pipelined(gpu_ctx, states, 11, data, 1 << 16, 32, 5)
    s = host_buf(stream.size, True, data=stream)
    back = host_buf(data.size, True, fill=0)
    assert gpu_ctx.decode_host_pipelined(MT, states, 11, s, back, plan) == data.size
    assert np.array_equal(back.numpy(), data)
    r, out = oracle.decode(MT, states, 11, stream, data.size)
    assert r == data.size and np.array_equal(out, data)


def _raw_call(ctx, container, states, bits, data, out, block, interval=0, flags=1, plan=None, plan_capacity=None, groups=None, n_slices=0):
    opts = H.api.EncodeOpts(block, interval, plan.ctypes.data if plan is not None else None,
                            (plan.size if plan is not None else 0) if plan_capacity is None else plan_capacity, 0, flags, 0,
                            groups.ctypes.data if groups is not None else None, groups.size if groups is not None else 0)
    n = H.load_library().hsrans_encode_host_pipelined(ctx.handle, container, states, bits, data.ctypes.data, data.size, out.ctypes.data, out.size,
                                                      ctypes.byref(opts), n_slices)
    return n, opts.plan_size


def test_refusals_leave_out_untouched(gpu_ctx, zipf):
    data = np.ascontiguousarray(zipf[:1_000_000])
    cap = H.capacity(MT, 64, data.size)
    out = np.full(cap, SENTINEL, np.uint8)
    pcap = H.load_library().hsrans_plan_capacity(MT, 64, data.size, 32, 1 << 16)
    plan = np.full(pcap, SENTINEL, np.uint8)
    groups = np.array([64, 128], np.uint64)
    refused = [
        dict(container=H.RAW), dict(container=H.BLOCK), dict(flags=0), dict(flags=3), dict(block=0), dict(block=1000), dict(block=(1 << 30) + 64),
        dict(states=16), dict(bits=16), dict(bits=9), dict(interval=6, plan=plan), dict(interval=32), dict(groups=groups, plan=plan),
        dict(out=out[: cap - 1]), dict(interval=32, plan=plan, plan_capacity=64),
        dict(interval=32, plan=plan, plan_capacity=int(pcap // 8)),
    ]
    for kw in refused:
        args = dict(container=MT, states=64, bits=11, data=data, out=out, block=1 << 16)
        args.update(kw)
        n, psize = _raw_call(gpu_ctx, **args)
        assert n == 0 and psize == 0, kw
        assert np.all(out == SENTINEL), kw
        assert np.all(plan == SENTINEL), kw
    # the refused plan capacity is exactly what the host encoder refuses as well: one byte less than the plan it writes
    _, want_plan = host_encoder(64, 11, data, 1 << 16, 32)
    small = np.full(want_plan.size - 1, SENTINEL, np.uint8)
    n, _ = _raw_call(gpu_ctx, MT, 64, 11, data, out, 1 << 16, interval=32, plan=small)
    assert n == 0 and np.all(out == SENTINEL) and np.all(small == SENTINEL)
    exact = np.full(want_plan.size, SENTINEL, np.uint8)
    n, psize = _raw_call(gpu_ctx, MT, 64, 11, data, out, 1 << 16, interval=32, plan=exact)
    assert n != 0 and psize == want_plan.size and np.array_equal(exact, want_plan)


def test_tight_plan_capacity_with_single_symbol_blocks(gpu_ctx, zipf):
    """a plan buffer of exactly the plan's size, smaller than the bound that takes every block as coded, is accepted"""
    b = 1 << 16
    data = np.concatenate([np.full(5 * b, 3, np.uint8), zipf[: 3 * b + 17]])
    want, want_plan = host_encoder(64, 11, data, b, 32)
    out = np.full(H.capacity(MT, 64, data.size), SENTINEL, np.uint8)
    exact = np.full(want_plan.size, SENTINEL, np.uint8)
    n, psize = _raw_call(gpu_ctx, MT, 64, 11, data, out, b, interval=32, plan=exact, n_slices=3)
    assert n == want.size and np.array_equal(out[:n], want) and np.array_equal(exact, want_plan) and psize == want_plan.size
    assert np.all(out[n:] == SENTINEL)


def test_context_reuse_interleaved_with_pipelined_decodes(gpu_ctx, zipf):
    for k, (length, states, interval, n_slices) in enumerate([(9_000_001, 64, 32, 0), (300_000, 32, 4, 3), (20_000_000, 64, 0, 5),
                                                              (9_000_001, 64, 32, 0), (1_234_567, 32, 32, 7)]):
        data = zipf[k * 1000: k * 1000 + length]
        want, want_plan = host_encoder(states, 11, data, 1 << 16, interval)
        got, plan = pipelined(gpu_ctx, states, 11, data, 1 << 16, interval, n_slices)
        assert np.array_equal(got, want) and (interval == 0 or np.array_equal(plan, want_plan)), k
        idx = want_plan if interval else host_encoder(states, 11, data, 1 << 16, 32)[1]
        s = host_buf(got.size, True, data=got)
        back = host_buf(data.size, True, fill=0)
        assert gpu_ctx.decode_host_pipelined(MT, states, 11, s, back, idx) == data.size and np.array_equal(back.numpy(), data), k
