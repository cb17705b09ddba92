"""hsrans_decode_device_indexing on block_ streams: the first decode of a stream that only exists in device memory — planned from its
head (hsrans_dplan_create_from_device_stream(HSRANS_BLOCK)), walked by one wavefront that also records block headers, entry states and
checkpoints — leaves the indexed plan behind, assembled on the device (k_walk_index_count / k_walk_index_fill).  That plan is byte for
byte the one hsrans_index_build makes from a host copy of the stream, launches like it, and serves the gather entry.  Bytes against the
CPU oracle (block_rANS32x64_16w_decode.cpp:15-128)."""
import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import synth
from oracle_lib import BLOCK

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zipf():
    return synth.enwik8_shaped(1 << 20, seed=11)


@pytest.fixture(scope="module")
def nonstat():
    return synth.nonstationary(3_000_000)


def _upload(s):
    import torch

    return torch.from_numpy(np.concatenate([s, np.zeros((-s.size) % 16, np.uint8)])).cuda()


def _first_decode(ctx, states, bits, s, n, interval):
    """(d_stream, base plan, output with 64 canary bytes behind it, indexed plan)"""
    import torch

    d_in = _upload(s)
    base = ctx.make_device_plan_from_stream(H.BLOCK, states, bits, d_in, s.size, n)
    assert np.array_equal(ctx.read_device_plan(base, capacity=1 << 16), H.plan_build(H.BLOCK, states, bits, s))
    first = torch.full((n + 64,), 0xCC, dtype=torch.uint8, device="cuda")
    indexed = ctx.decode_device_indexing(base, d_in, first[:n], interval, stream_length=s.size)
    return d_in, base, first, indexed


def _check(ctx, oracle, states, bits, s, d, interval, quirk=False):
    import torch

    n = d.size
    r0, want = oracle.decode(BLOCK, states, bits, s, n)
    assert r0 == n and (quirk or np.array_equal(want, d))
    d_in, base, first, indexed = _first_decode(ctx, states, bits, s, n, interval)
    assert np.array_equal(first[:n].cpu().numpy(), want) and bool((first[n:] == 0xCC).all())
    want_plan = ctx.index_build(H.BLOCK, states, bits, s, interval)
    assert np.array_equal(ctx.read_device_plan(indexed, capacity=want_plan.size + 4096), want_plan)
    again = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ctx.decode_device(indexed, d_in, again, stream_length=s.size)
    assert ctx.status(indexed) == 0 and np.array_equal(again.cpu().numpy(), want)
    twin = ctx.make_device_plan(want_plan)  # the same blob through the host's group builder: the same launch
    again.zero_()
    ctx.decode_device(twin, d_in, again, stream_length=s.size)
    assert ctx.status(twin) == 0 and np.array_equal(again.cpu().numpy(), want)
    assert indexed.launch_info() == twin.launch_info()
    # three ranges in one gather: unaligned, across a block edge (the first piece with another histogram), the last bytes
    _, _, pc = H.api.plan_tables(want_plan)
    coded = pc[(pc["flags"] & 2) == 0]
    later = coded[coded["hist_off"] != coded["hist_off"][0]]
    edge = int(later["out_off"][0]) if later.size else n // 2
    ranges = [(12_345, 1_001, 0), (edge - 100, 300, 1_001), (n - 77, 77, 1_301)]
    dst = torch.full((1_378 + 16,), 0xCC, dtype=torch.uint8, device="cuda")
    ctx.decode_device_gather(indexed, d_in, ranges, dst, stream_length=s.size)
    got = dst.cpu().numpy()
    assert ctx.status(indexed) == 0 and bool((got[1_378:] == 0xCC).all())
    for off, length, at in ranges:
        assert np.array_equal(got[at:at + length], want[off:off + length]), (off, length)
    return want_plan


def _runs(zipf):
    """text with long runs of one byte in it: in fixed blocks of 64 KiB, single-symbol blocks between coded ones and next to each other"""
    return np.concatenate([zipf[:100_000], np.full(300_000, 7, np.uint8), zipf[100_000:200_000], np.full(150_000, 9, np.uint8), np.full(150_000, 3, np.uint8),
                           zipf[200_000:300_037]])


# (data, length, bits, block size, interval): a handful of blocks and a tail; hundreds of chains per block (the per-block loop beyond one
# wavefront's lanes, the cut into parts); many blocks of changing statistics; a 3-byte tail; one coded block (shared_hist); the widest
# table; single-symbol blocks between coded ones and in runs (one fill group per run)
CASES = (("zipf", 300_000, 11, 65536, 32), ("zipf", 300_000, 11, 65536, 4), ("nonstat", 2_000_000, 11, 65536, 32), ("nonstat", 1_000_003, 13, 32768, 32),
         ("zipf", 40_000, 11, 65536, 32), ("zipf", 300_000, 15, 65536, 64), ("runs", 900_037, 11, 65536, 32))


def _data(src, n, zipf, nonstat):
    return (zipf if src == "zipf" else nonstat if src == "nonstat" else _runs(zipf))[:n]


@pytest.mark.parametrize("states,case", [(st, c) for c in range(len(CASES)) for st in (32, 64) if (st, CASES[c][2]) != (32, 15)])  # (the widest table: 64 states only)
def test_first_decode_of_a_block_stream_leaves_the_index_behind(gpu_ctx, oracle, zipf, nonstat, states, case):
    src, n, bits, block, interval = CASES[case]
    d = _data(src, n, zipf, nonstat)
    s = H.encode(H.BLOCK, states, bits, d, block_size=block)
    plan = _check(gpu_ctx, oracle, states, bits, s, d, interval)
    hdr, _, pc = H.api.plan_tables(plan)
    if src == "runs":
        fill = (pc["flags"] & 2) != 0
        assert int(fill.sum()) > 2 and bool((fill[1:] & fill[:-1]).any()) and bool((fill[1:] & ~fill[:-1]).any())  # alone and next to each other
    if case == 4:
        assert hdr["shared_hist"] == 1 and hdr["n_chains"] > 1


@pytest.mark.parametrize("states", (32, 64))
@pytest.mark.parametrize("bits", (11, 13))
@pytest.mark.parametrize("src,n", (("nonstat", 3_000_000), ("zipf", 1 << 20), ("zipf", 524_300)))
def test_streams_of_the_reference(gpu_ctx, oracle, ref, zipf, nonstat, states, bits, src, n):
    """the reference's adaptive block ends; 524,300 is a length whose last bytes the reference itself mis-decodes"""
    d = (zipf if src == "zipf" else nonstat)[:n]
    s = ref.encode(BLOCK, states, bits, d)
    _check(gpu_ctx, oracle, states, bits, s, d, 64, quirk=n == 524_300)


@pytest.mark.parametrize("states", (32, 64))
def test_both_assembly_paths(oracle, zipf, nonstat, monkeypatch, states):
    """HSRANS_INDEX_ASSEMBLE_ON_HOST=1: the records come down and the host writes the blob — the same blob, the same bytes"""
    monkeypatch.setenv("HSRANS_INDEX_ASSEMBLE_ON_HOST", "1")
    ctx = H.Context(0)  # (the switch is read when the context is made)
    for case in (0, 2, 4, 6):
        src, n, bits, block, interval = CASES[case]
        d = _data(src, n, zipf, nonstat)
        s = H.encode(H.BLOCK, states, bits, d, block_size=block)
        _check(ctx, oracle, states, bits, s, d, interval)


@pytest.mark.parametrize("states", (32, 64))
def test_block_list_overflow_still_decodes(gpu_ctx, zipf, states):
    """more blocks than decoded_len / 4096 + 16: no plan (as hsrans_index_build), but the walk itself went through"""
    import torch

    d = zipf[:200_000]
    s = H.encode(H.BLOCK, states, 11, d, block_size=1024, out_capacity=400_000)  # (520 bytes of header a block: more than the default capacity)
    d_in = _upload(s)
    base = gpu_ctx.make_device_plan_from_stream(H.BLOCK, states, 11, d_in, s.size, d.size)
    out = torch.zeros(d.size, dtype=torch.uint8, device="cuda")
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_indexing(base, d_in, out, 32, stream_length=s.size)
    assert np.array_equal(out.cpu().numpy(), d)
    out.zero_()
    gpu_ctx.decode_device(base, d_in, out, stream_length=s.size)
    assert gpu_ctx.status(base) == 0 and np.array_equal(out.cpu().numpy(), d)


@pytest.mark.parametrize("states", (32, 64))
def test_refusals_and_a_flipped_histogram_count(gpu_ctx, zipf, states):
    import torch

    d = zipf[:300_000]
    s = H.encode(H.BLOCK, states, 11, d, block_size=65536)
    d_in, base, first, indexed = _first_decode(gpu_ctx, states, 11, s, d.size, 32)
    # arguments: an interval that is not a multiple of 4, a plan that has checkpoints already, a raw stream planned on the device
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_indexing(base, d_in, first[:d.size], 6, stream_length=s.size)
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_indexing(indexed, d_in, first[:d.size], 32, stream_length=s.size)
    with pytest.raises(H.HsransError):
        gpu_ctx.make_device_plan_from_stream(H.RAW, states, 11, d_in, s.size, d.size)
    # one count of the SECOND block's histogram: its sum is no longer 2^bits — a device error, no plan, the status word cleared
    _, _, pc = H.api.plan_tables(gpu_ctx.index_build(H.BLOCK, states, 11, s, 32))
    hists = sorted(set(int(h) for h in pc[(pc["flags"] & 2) == 0]["hist_off"]))
    assert len(hists) > 2
    bad = s.copy()
    bad[hists[1] + 2] ^= 0x40
    d_bad = _upload(bad)
    out = torch.zeros(d.size, dtype=torch.uint8, device="cuda")
    with pytest.raises(H.HsransError):
        gpu_ctx.decode_device_indexing(base, d_bad, out, 32, stream_length=bad.size)
    assert gpu_ctx.status(base) == 0
    gpu_ctx.decode_device(base, d_in, out, stream_length=s.size)
    assert gpu_ctx.status(base) == 0 and np.array_equal(out.cpu().numpy(), d)
