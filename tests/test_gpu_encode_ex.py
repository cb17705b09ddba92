"""hsrans_encode_device_ex: every format hsrans_encode_ex writes, on the GPU — block_ and mt_ with the reference's adaptive blocks or fixed
blocks, the states carried from block to block — byte for byte against the host encoder (and, where recorded, the real reference),
plans included, decoded back on the device."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth
from oracle_lib import BLOCK, MT

pytestmark = pytest.mark.gpu

ZIPF_PREFIXES = (65537, 65560, 65599, 65600, 131073, 524300)
# the adaptive policy's unit, 1 << MinBlockSize (hsrans_host.cpp reference_policy): mt_ 2^16; block_ by states and bits 10..15
_MIN64, _MIN32 = (20, 19, 16, 17, 17, 16), (20, 19, 15, 17, 17, 18)


def walk_unit(container, states, bits):
    return 1 << 16 if container == MT else 1 << (_MIN64 if states == 64 else _MIN32)[bits - 10]


def short_last_block(container, states, bits, n):
    """The documented deviation: where the reference leaves a last block shorter than one group, the product merges it."""
    unit = walk_unit(container, states, bits)
    target = ((n - 1) & ~(states - 1)) & ~(unit - 1)
    if target > unit:
        target -= unit
    return target > 0 and n - target < states


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
    d = torch.zeros(max(int(data.size), 1), dtype=torch.uint8, device="cuda")
    if data.size:
        d[: data.size] = torch.from_numpy(np.ascontiguousarray(data)).cuda()
    return d[: data.size] if data.size else d


def device_encode(ctx, container, states, bits, data, **kw):
    d_in = _dev(data)
    d_out = torch.full((H.capacity(container, states, data.size),), 0xA5, dtype=torch.uint8, device="cuda")
    r = ctx.encode_device_ex(container, states, bits, d_in, d_out, **kw)
    m = r[0] if isinstance(r, tuple) else r
    return (d_out[:m].cpu().numpy(),) + (tuple(r[1:]) if isinstance(r, tuple) else ())


def sweep_inputs(zipf, nonstat, runs, container, states, bits):
    unit = walk_unit(container, states, bits)
    yield from ((f"zipf[:{n}]", zipf[:n]) for n in ZIPF_PREFIXES)
    yield "zipf", zipf
    yield "nonstat", nonstat
    yield "runs", runs
    yield "one symbol", np.full(300_000, 42, np.uint8)
    yield "n < S", zipf[: states - 5]
    for n in (unit - states, unit - 1, unit + 1, unit + states + 3):
        if 0 < n <= 3 * (1 << 20):
            yield f"unit{n:+d}", np.resize(nonstat, n)


RECORDED = {65537, 65560, 65599, 65600, 131073, 524300}


@pytest.mark.parametrize("container", (BLOCK, MT))
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits", (10, 11, 12, 13, 14, 15))
def test_adaptive_blocks_match_the_host_encoder(gpu_ctx, ref, zipf, nonstat, runs, container, states, bits):
    for name, data in sweep_inputs(zipf, nonstat, runs, container, states, bits):
        host = H.encode(container, states, bits, data, block_size=0)
        (dev,) = device_encode(gpu_ctx, container, states, bits, data, block_size=0)
        assert dev.size == host.size and np.array_equal(dev, host), (name, container, states, bits, dev.size, host.size)
        recorded = (name.startswith("zipf[:") and data.size in RECORDED) or name == "nonstat"
        if recorded:
            want = ref.encode(container, states, bits, data)
            if not np.array_equal(host, want):
                assert short_last_block(container, states, bits, data.size), (name, container, states, bits)


@pytest.mark.parametrize("container", (BLOCK, MT))
@pytest.mark.parametrize("states", (32, 64))
def test_the_walk_cuts_non_stationary_data_into_blocks(gpu_ctx, nonstat, runs, container, states):
    for data in (nonstat, runs):
        dev, = device_encode(gpu_ctx, container, states, 11, data)
        assert np.array_equal(dev, H.encode(container, states, 11, data))
        if container == MT:
            assert H.plan_chain_count(H.plan_build(container, states, 11, dev)) > 1


@pytest.mark.parametrize("container", (BLOCK, MT))
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("block_size", (4096, 65536, 65536 + 64))
def test_fixed_blocks_with_carried_states(gpu_ctx, zipf, nonstat, container, states, block_size):
    for data in (zipf, nonstat[:1_500_000], zipf[: 2 * block_size + states - 7]):  # (the last: a remainder shorter than S, merged)
        host = H.encode(container, states, 12, data, block_size=block_size)
        (dev,) = device_encode(gpu_ctx, container, states, 12, data, block_size=block_size)
        assert np.array_equal(dev, host), (container, states, block_size, data.size)


def _decode_checks(ctx, container, states, bits, data, stream, plan, dplan):
    d_stream = _dev(np.concatenate([stream, np.zeros((-stream.size) % 16 + 16, np.uint8)]))
    for p in (dplan, ctx.make_device_plan(plan), ctx.make_device_plan(H.plan_build(container, states, bits, stream))):
        d_back = torch.zeros(data.size, dtype=torch.uint8, device="cuda")
        ctx.decode_device(p, d_stream, d_back, stream_length=stream.size)
        torch.cuda.synchronize()
        assert ctx.status(p) == 0
        assert np.array_equal(d_back.cpu().numpy(), data)


@pytest.mark.parametrize("container", (BLOCK, MT))
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("index", ("i16", "i32", "groups"))
@pytest.mark.parametrize("block_size", (0, 65536))
def test_plans_match_the_host_encoder_and_decode(gpu_ctx, nonstat, container, states, index, block_size):
    bits, data = 11, nonstat
    kw = dict(index_groups=H.index_boundaries(states, bits, data.size, gpu_ctx)) if index == "groups" else dict(index_interval=int(index[1:]))
    host, hplan = H.encode(container, states, bits, data, block_size=block_size, **kw)
    dev, plan, dplan = device_encode(gpu_ctx, container, states, bits, data, block_size=block_size, want_plan=True, want_device_plan=True, **kw)
    assert np.array_equal(dev, host)
    assert np.array_equal(plan, hplan)
    _decode_checks(gpu_ctx, container, states, bits, data, dev, plan, dplan)


@pytest.mark.parametrize("kind", ("config2", "nonstationary"))
@pytest.mark.parametrize("container", (BLOCK, MT))
def test_100_mb(gpu_ctx, kind, container):
    states, bits, n = 64, 11, 100_000_000
    data = synth.enwik8_shaped(n, seed=7) if kind == "config2" else synth.nonstationary(n)
    groups = H.index_boundaries(states, bits, n, gpu_ctx)
    host, hplan = H.encode(container, states, bits, data, index_groups=groups)
    dev, plan, dplan = device_encode(gpu_ctx, container, states, bits, data, index_groups=groups, want_plan=True, want_device_plan=True)
    assert np.array_equal(dev, host)
    assert np.array_equal(plan, hplan)
    d_stream = _dev(np.concatenate([dev, np.zeros((-dev.size) % 16 + 16, np.uint8)]))
    d_back = torch.zeros(n, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(dplan, d_stream, d_back, stream_length=dev.size)
    torch.cuda.synchronize()
    assert gpu_ctx.status(dplan) == 0 and np.array_equal(d_back.cpu().numpy(), data)


@pytest.mark.parametrize("states", (32, 64))
def test_delegation_to_the_raw_and_independent_encoders(gpu_ctx, zipf, states):
    data = zipf
    d_in = _dev(data)
    a = torch.zeros(H.capacity(H.RAW, states, data.size), dtype=torch.uint8, device="cuda")
    b = torch.zeros_like(a)
    m1 = gpu_ctx.encode_device_ex(H.RAW, states, 12, d_in, a)
    m2 = gpu_ctx.encode_device_raw(states, 12, d_in, b)
    assert m1 == m2 and torch.equal(a[:m1], b[:m2])
    a = torch.zeros(H.capacity(MT, states, data.size), dtype=torch.uint8, device="cuda")
    b = torch.zeros_like(a)
    m1 = gpu_ctx.encode_device_ex(MT, states, 12, d_in, a, block_size=1 << 15, independent_blocks=True)
    m2 = gpu_ctx.encode_device(MT, states, 12, d_in, b, block_size=1 << 15)
    assert m1 == m2 and torch.equal(a[:m1], b[:m2])
    # independent blocks with an index: the chain kernel with fresh states per block, stream and plan as the host's
    host, hplan = H.encode(MT, states, 12, data, block_size=1 << 15, independent_blocks=True, index_interval=16)
    dev, plan = device_encode(gpu_ctx, MT, states, 12, data, block_size=1 << 15, independent_blocks=True, index_interval=16, want_plan=True)
    assert np.array_equal(dev, host) and np.array_equal(plan, hplan)


def test_refusals_leave_the_output_alone(gpu_ctx, zipf):
    data = zipf[:200_000]
    d_in = _dev(data)
    cap = H.capacity(MT, 64, data.size)
    d_out = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    big_in = torch.zeros(data.size + 16, dtype=torch.uint8, device="cuda")
    big_in[1: 1 + data.size] = d_in
    cases = [
        dict(container=MT, states=64, bits=11, d_in=d_in, d_out=d_out[:cap], independent_blocks=True),  # independent needs block_size
        dict(container=BLOCK, states=64, bits=11, d_in=d_in, d_out=d_out[:cap], block_size=4096, independent_blocks=True),
        dict(container=MT, states=64, bits=9, d_in=d_in, d_out=d_out[:cap]),
        dict(container=MT, states=16, bits=11, d_in=d_in, d_out=d_out[:cap]),
        dict(container=MT, states=64, bits=11, d_in=big_in[1: 1 + data.size], d_out=d_out[:cap]),  # unaligned input
        dict(container=MT, states=64, bits=11, d_in=d_in, d_out=d_out[1: 1 + cap]),  # unaligned output
        dict(container=MT, states=64, bits=11, d_in=d_in, d_out=d_out[: cap - 1]),  # short capacity
        dict(container=MT, states=64, bits=11, d_in=d_in, d_out=d_out[:cap], block_size=100),  # not a multiple of 64
        # listed checkpoints with fixed blocks of 5 groups: checkpoints are taken between sets of four groups (documented limit)
        dict(container=MT, states=64, bits=11, d_in=d_in, d_out=d_out[:cap], block_size=320, index_groups=np.arange(4, 400, 4, dtype=np.uint64), want_plan=True),
    ]
    for kw in cases:
        c, s, b, i, o = kw.pop("container"), kw.pop("states"), kw.pop("bits"), kw.pop("d_in"), kw.pop("d_out")
        with pytest.raises(H.HsransError):
            gpu_ctx.encode_device_ex(c, s, b, i, o, **kw)
        torch.cuda.synchronize()
        assert bool((d_out == 0xA5).all()), kw
        # the context still works
        host = H.encode(MT, 64, 11, data)
        (dev,) = device_encode(gpu_ctx, MT, 64, 11, data)
        assert np.array_equal(dev, host)
