"""hsrans_decode_device_gather on the GPU, bit-exact: arbitrary byte ranges of a stream that stays compressed in device memory land where
the caller wants them, and nowhere else.  Expected bytes are always the encoder's input, data[offset : offset + length].  Every gather
writes into a buffer filled with 0xCC that has 4 KiB of canary in front of and behind the destination (and in every gap between
ranges); the WHOLE buffer is compared, so a byte written outside a range fails the case; the plan's status word must stay 0."""
import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth

pytestmark = pytest.mark.gpu

N = 3_000_001  # not a multiple of 64 (nor of 32): the stream ends in a masked group
BLOCK = 1 << 16
FILL_BLOCK = 5  # mt_ block [5 * 64 KiB, 6 * 64 KiB) holds one symbol only: a single-symbol fill block
CANARY = 4096
CONTAINERS = ("raw32", "rawdev", "mt", "mt32", "block32")


@pytest.fixture(scope="module")
def datasets():
    out = {}
    for name, d in (("nonstat", synth.nonstationary(N)), ("zipf", synth.enwik8_shaped(N, seed=11))):
        d = d.copy()
        d[FILL_BLOCK * BLOCK:(FILL_BLOCK + 1) * BLOCK] = 0x41
        out[name] = d
    return out


def _upload(stream):
    return torch.from_numpy(np.concatenate([stream, np.zeros((-stream.size) % 16, np.uint8)])).cuda()


def _encode(ctx, kind, states, bits, data):
    if kind == "raw32":
        s, plan = H.encode(H.RAW, states, bits, data, index_interval=32)
    elif kind == "rawdev":
        s, plan = H.encode(H.RAW, states, bits, data, index_groups=H.index_boundaries(states, bits, data.size, ctx))
    elif kind == "raw":
        s = H.encode(H.RAW, states, bits, data)
        plan = H.plan_build(H.RAW, states, bits, s)
    elif kind == "mt":
        s = H.encode(H.MT, states, bits, data, block_size=BLOCK)
        plan = H.plan_build(H.MT, states, bits, s)
    elif kind == "mt32":
        s, plan = H.encode(H.MT, states, bits, data, block_size=BLOCK, index_interval=32)
    elif kind == "block32":
        s, plan = H.encode(H.BLOCK, states, bits, data, index_interval=32)
    elif kind == "block":
        s = H.encode(H.BLOCK, states, bits, data)
        plan = H.plan_build(H.BLOCK, states, bits, s)
    else:
        raise AssertionError(kind)
    return s, plan


def _layout(src, packing, base_align=0):
    """(offset, length) pairs -> (N, 3) ranges and the buffer size.  packing: 'packed' = back to back behind the front canary (most
    destinations misaligned against their source); 'aligned' = every dst_offset congruent to its offset modulo 4 (gaps of < 4 bytes);
    'gaps' = 4 KiB of canary between ranges."""
    rows, pos = [], CANARY
    for off, length in src:
        if packing == "aligned":
            pos += (off - pos - base_align) % 4
        rows.append((off, length, pos))
        pos += length + (CANARY if packing == "gaps" else 0)
    return np.array(rows, np.uint64).reshape(-1, 3), pos + CANARY


def _gather_and_check(ctx, dplan, d_stream, m, data, src, packing="packed", misalign=0, check_status=True):
    """one gather of the (offset, length) pairs `src`; compares the whole destination buffer, canaries included"""
    ranges, size = _layout(src, packing, base_align=misalign)
    want = np.full(size, 0xCC, np.uint8)
    for off, length, dst in ranges:
        want[int(dst):int(dst + length)] = data[int(off):int(off + length)]
    backing = torch.full((size + 16,), 0xCC, dtype=torch.uint8, device="cuda")
    d_dst = backing[misalign:misalign + size]  # (misalign: a destination base that is not even 2-byte aligned)
    ctx.decode_device_gather(dplan, d_stream, ranges, d_dst, stream_length=m)
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    if not np.array_equal(got, want):
        bad = int(np.argmax(got != want))
        row = int(np.searchsorted(ranges[:, 2], bad, side="right")) - 1
        raise AssertionError(f"first wrong byte at destination {bad} (of {size}), range {row}: {ranges[max(row, 0)].tolist()}, got {got[bad]} want {want[bad]}")
    assert np.all(backing.cpu().numpy()[size + misalign:] == 0xCC) and np.all(backing.cpu().numpy()[:misalign] == 0xCC)
    if check_status:
        assert ctx.status(dplan) == 0
    return ranges


def _random_src(rng, count, n):
    lens = np.minimum((2.0 ** rng.uniform(0, 18, count)).astype(np.int64), n)  # 1 B .. 256 KiB, every magnitude alike
    offs = (rng.random(count) * (n - lens + 1)).astype(np.int64)
    return [(int(o), int(l)) for o, l in zip(offs, lens)]


def _explicit_src(n, states):
    b0 = 7 * BLOCK  # a block boundary (mt_) and a checkpoint boundary
    f0, f1 = FILL_BLOCK * BLOCK, (FILL_BLOCK + 1) * BLOCK
    return [
        (0, 1), (0, 5000), (0, 77_777),                            # offset 0
        (n - 1, 1), (n - 17, 17), (n - 70_001, 70_001),            # ending at decoded_len, inside the masked tail
        (b0 - 1, 1), (b0 - 1, 2), (b0 - 1, 4099), (b0 + 1, 1), (b0 + 1, 9000), (b0, states), (b0 - states, 2 * states),  # around a block boundary
        (f0 + 100, 1), (f0 + 3, 30_001), (f0, BLOCK), (f0 - 5000, 12_000), (f1 - 11, 6000), (f0 - 70_000, 3 * BLOCK),     # inside and across the fill block
        (123_457, 31_000), (123_457, 31_000),                      # the same source twice
        (1_000_003, 0),                                            # an empty range among the others
    ]


@pytest.mark.parametrize("bits", (11, 12, 14, 15))
@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("kind", CONTAINERS)
def test_matrix(gpu_ctx, datasets, kind, states, bits):
    data = datasets["nonstat" if states == 64 else "zipf"]
    s, plan = _encode(gpu_ctx, kind, states, bits, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = _upload(s)
    rng = np.random.default_rng(100_000 * CONTAINERS.index(kind) + 100 * states + bits)
    src = _random_src(rng, 1100, N)
    _gather_and_check(gpu_ctx, dplan, d_stream, s.size, data, src, "packed")                      # >= 1,000 random ranges, back to back
    _gather_and_check(gpu_ctx, dplan, d_stream, s.size, data, _explicit_src(N, states), "gaps")   # the explicit ones, canary between them
    _gather_and_check(gpu_ctx, dplan, d_stream, s.size, data, _explicit_src(N, states), "packed", misalign=1)
    _gather_and_check(gpu_ctx, dplan, d_stream, s.size, data, src[:300], "aligned")               # the word-store path
    # one range = the whole stream: the same bytes decode_device gives
    whole = torch.zeros(N, dtype=torch.uint8, device="cuda")
    gpu_ctx.decode_device(dplan, d_stream, whole, stream_length=s.size)
    torch.cuda.synchronize()
    assert np.array_equal(whole.cpu().numpy(), data)
    _gather_and_check(gpu_ctx, dplan, d_stream, s.size, data, [(0, N)], "packed")
    _gather_and_check(gpu_ctx, dplan, d_stream, s.size, data, [(0, N)], "packed", misalign=3)


@pytest.mark.parametrize("states,bits", ((64, 11), (32, 12), (64, 14)))
def test_raw_without_index(gpu_ctx, datasets, states, bits):
    """one chain: every task decodes from the stream's first byte, and is correct"""
    data = datasets["zipf"][:600_011]
    s, plan = _encode(gpu_ctx, "raw", states, bits, data)
    assert H.plan_chain_count(plan) == 1
    dplan = gpu_ctx.make_device_plan(plan)
    _gather_and_check(gpu_ctx, dplan, _upload(s), s.size, data, [(300_000, 5000)], "packed")
    _gather_and_check(gpu_ctx, dplan, _upload(s), s.size, data, [(299_999, 4097), (0, 3), (data.size - 5, 5)], "gaps", misalign=1)


@pytest.mark.parametrize("states,bits,interval", ((64, 11, 32), (32, 12, 32), (64, 14, 0)))
def test_plan_written_on_the_device(gpu_ctx, datasets, states, bits, interval):
    """the GPU encoder's plan (no host copy of it exists): the chain that holds a byte is found on the device"""
    data = datasets["nonstat"]
    d_in = torch.from_numpy(data).cuda()
    d_out = torch.empty(H.capacity(H.MT, states, data.size), dtype=torch.uint8, device="cuda")
    m, dplan = gpu_ctx.encode_device(H.MT, states, bits, d_in, d_out, block_size=BLOCK, index_interval=interval, want_plan=True)
    rng = np.random.default_rng(7 + bits)
    _gather_and_check(gpu_ctx, dplan, d_out, m, data, _random_src(rng, 400, N) + _explicit_src(N, states), "packed")
    _gather_and_check(gpu_ctx, dplan, d_out, m, data, _explicit_src(N, states), "aligned")


def test_plan_from_an_indexing_decode(gpu_ctx, datasets):
    data = datasets["nonstat"]
    s = H.encode(H.MT, 64, 11, data, block_size=BLOCK)
    d_stream = _upload(s)
    base = gpu_ctx.make_device_plan_from_stream(H.MT, 64, 11, d_stream, s.size, N)
    out = torch.zeros(N, dtype=torch.uint8, device="cuda")
    indexed = gpu_ctx.decode_device_indexing(base, d_stream, out, 32, stream_length=s.size)
    rng = np.random.default_rng(5)
    _gather_and_check(gpu_ctx, base, d_stream, s.size, data, _random_src(rng, 200, N), "packed")
    _gather_and_check(gpu_ctx, indexed, d_stream, s.size, data, _random_src(rng, 400, N) + _explicit_src(N, 64), "packed")


def test_refusals_leave_the_destination_alone(gpu_ctx, datasets):
    data = datasets["zipf"][:400_003]
    s, plan = _encode(gpu_ctx, "raw32", 64, 11, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = _upload(s)
    d_dst = torch.full((20_000,), 0xCC, dtype=torch.uint8, device="cuda")

    def refused(dp, stream, m, ranges, code):
        with pytest.raises(H.HsransError) as e:
            gpu_ctx.decode_device_gather(dp, stream, ranges, d_dst, stream_length=m)
        assert e.value.code == code, (e.value.code, code)
        torch.cuda.synchronize()
        assert bool((d_dst == 0xCC).all())

    refused(dplan, d_stream, s.size, [(0, 100, 0), (data.size - 10, 11, 200)], 2)   # a range past the decoded length
    refused(dplan, d_stream, s.size, [(data.size + 1, 0, 0)], 2)
    refused(dplan, d_stream, s.size, [(0, 100, 0), (5000, 10_000, 10_001)], 2)      # the destination is too small
    refused(dplan, d_stream, s.size, [(0, 1, 20_000)], 2)
    refused(dplan, d_stream, s.size - 2, [(0, 100, 0)], 3)                          # a wrong stream length
    refused(dplan, d_stream, s.size + 16, [(0, 100, 0)], 3)
    sb, pb = _encode(gpu_ctx, "block", 64, 11, data)                                # block_ without checkpoints: no entry points
    refused(gpu_ctx.make_device_plan(pb), _upload(sb), sb.size, [(0, 100, 0)], 3)
    # nothing to do: fine, nothing launched, nothing written
    gpu_ctx.decode_device_gather(dplan, d_stream, np.zeros((0, 3), np.uint64), d_dst, stream_length=s.size)
    gpu_ctx.decode_device_gather(dplan, d_stream, [(5, 0, 0), (data.size, 0, 20_000)], d_dst, stream_length=s.size)
    torch.cuda.synchronize()
    assert bool((d_dst == 0xCC).all()) and gpu_ctx.status(dplan) == 0


def test_two_gathers_queued_back_to_back(gpu_ctx, datasets):
    """different range lists, one stream, no synchronisation in between: the first launch's task list must not be overwritten under it"""
    data = datasets["nonstat"]
    s, plan = _encode(gpu_ctx, "mt32", 64, 11, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = _upload(s)
    rng = np.random.default_rng(99)
    jobs = []
    for k in range(6):  # (six: the lists together are larger than one region of the context's task buffer)
        ranges, size = _layout(_random_src(rng, 1500 + 100 * k, N), "packed")
        jobs.append((ranges, size, torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")))
    for ranges, size, d_dst in jobs:
        scratch = ranges.copy()
        gpu_ctx.decode_device_gather(dplan, d_stream, scratch, d_dst, stream_length=s.size)
        scratch[:] = 0  # `ranges` is read before the call returns: the caller may reuse it
    torch.cuda.synchronize()
    assert gpu_ctx.status(dplan) == 0
    for ranges, size, d_dst in jobs:
        want = np.full(size, 0xCC, np.uint8)
        for off, length, dst in ranges:
            want[int(dst):int(dst + length)] = data[int(off):int(off + length)]
        assert np.array_equal(d_dst.cpu().numpy(), want)


def test_gathers_on_two_streams(gpu_ctx, datasets):
    data = datasets["zipf"]
    s, plan = _encode(gpu_ctx, "raw32", 64, 12, data)
    dplan = gpu_ctx.make_device_plan(plan)
    d_stream = _upload(s)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    jobs = []
    for k in range(8):
        ranges, size = _layout(_random_src(rng, 600, N), "packed")
        d_dst = torch.full((size,), 0xCC, dtype=torch.uint8, device="cuda")
        jobs.append((ranges, size, d_dst))
    torch.cuda.synchronize()
    for k, (ranges, size, d_dst) in enumerate(jobs):
        gpu_ctx.decode_device_gather(dplan, d_stream, ranges, d_dst, stream_length=s.size, stream=streams[k % 2])
    torch.cuda.synchronize()
    for ranges, size, d_dst in jobs:
        want = np.full(size, 0xCC, np.uint8)
        for off, length, dst in ranges:
            want[int(dst):int(dst + length)] = data[int(off):int(off + length)]
        assert np.array_equal(d_dst.cpu().numpy(), want)
    assert gpu_ctx.status(dplan) == 0


def test_altered_histogram_sets_the_status_and_the_plans_table_decodes(gpu_ctx):
    """A stream that does not carry the histogram the plan's host-built table was made from (one count flipped in the device copy):
    the first workgroup's first wave compares the stream's counts with the plan's copy and raises the status, reported once; the
    workgroups decode with the plan's own table, which the stream's counts never enter, so the gathered bytes are still the input's."""
    data = synth.enwik8_shaped(300_011, seed=21)
    s, plan = _encode(gpu_ctx, "raw32", 64, 11, data)
    dplan = gpu_ctx.make_device_plan(plan)
    bad = _upload(s)
    bad[int(H.api.plan_tables(plan)[2][0]["hist_off"]) + 40] ^= 0x5A  # one count of the histogram every piece of this plan decodes with
    assert sum(gpu_ctx.make_gather_set([dplan], [bad], [s.size]).info()["kind_members"][3:]) == 1  # a kind with a host-built table
    _gather_and_check(gpu_ctx, dplan, bad, s.size, data, [(1000, 4096), (150_001, 4096), (data.size - 4096, 4096)], "gaps", check_status=False)
    assert gpu_ctx.status(dplan) != 0
    assert gpu_ctx.status(dplan) == 0  # (reported once, then cleared)
