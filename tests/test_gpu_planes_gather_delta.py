"""The delta forms of the indirect and the many-frame byte-plane gathers: hsrans_decode_device_planes_gather_indirect_delta,
hsrans_decode_device_planes_gather_batch_delta, hsrans_decode_device_planes_gather_batch_indirect_delta and hsrans_planes_base_set.
Sizes, settings, the row list and the sentinel method are tests/test_gpu_planes_delta.py's: tensors of BIG = 2 * 65536 + 77 elements, 64
states, 11 bits, 64 KiB blocks, interval 32; `_rows(first)` — every length at every phase of the 16-element grid and a row that ends with
the tensor, packed from element 0 (16-byte stores) and from element 1 (element-wide stores).  Every expected value is a numpy slice of the
ORIGINAL arrays, or what hsrans_decode_device_planes_gather_delta writes for the same rows; every destination and workspace sits in a
sentinel-filled buffer with PAD bytes behind it."""
import ctypes
import random

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api, synth
from test_gpu_planes_delta import BIG, PAD, SENTINEL, TORCH_INT, Refusals, _bytes, _full, _rows, _settings, _tensor, _untouched

pytestmark = pytest.mark.gpu

E_ARG, E_DEVICE = 2, 5
DEFAULTS = _settings(64, 11, 32, 1 << 16, True)
GARBAGE = 0xDEADBEEFDEADBEEF  # rows beyond the count: never read


def _up(v, a):
    return (v + a - 1) // a * a


def _bf16(x):
    return (x.view(np.uint32) >> 16).astype(np.uint16)


@pytest.fixture(scope="module")
def arrays():
    """name -> (tensor, base): a fine-tune next to its base, tuned = base * (1 + 0.01 * N(0, 1)); made once and never changed"""
    rng = np.random.default_rng(29)
    base = rng.standard_normal(BIG).astype(np.float32)
    tuned = (base * (1 + 0.01 * rng.standard_normal(BIG))).astype(np.float32)
    tuned2 = (base * (1 + 0.01 * rng.standard_normal(BIG))).astype(np.float32)
    ramp = np.arange(BIG, dtype=np.uint64) << np.uint64(8)
    pairs = {
        "bf16": (_bf16(tuned), _bf16(base)),
        "bf16-second": (_bf16(tuned2), _bf16(base)),
        "bf16-noisy": (_bf16(tuned) ^ rng.integers(0, 256, BIG, dtype=np.uint16), _bf16(base)),  # the low byte of the residue is uniform
        "fp16": (tuned.astype(np.float16).view(np.uint16), base.astype(np.float16).view(np.uint16)),
        "fp32": (tuned.view(np.uint32), base.view(np.uint32)),
        "fp32-alone": (tuned2.view(np.uint32), None),
        "i64": (ramp + rng.integers(0, 1000, BIG, dtype=np.uint64), ramp + rng.integers(0, 1000, BIG, dtype=np.uint64)),
        "uniform": (synth.uniform_bytes(2 * BIG, seed=31).view(np.uint16), _bf16(base)),
        "bf16-same": (_bf16(base), _bf16(base)),
    }
    for a, b in pairs.values():
        a.setflags(write=False)
        if b is not None:
            b.setflags(write=False)
    return pairs


def _dtype_name(name):
    return name.split("-")[0] if name.split("-")[0] in ("bf16", "fp16", "fp32") and name != "bf16-noisy" else None


def _dev_ranges(ranges, n=None):
    """(rows, 3) int64 on the device in hsrans_range's layout, then garbage up to `n`"""
    arr = np.full((max(n or 0, len(ranges)), 3), GARBAGE, np.uint64)
    for k, g in enumerate(ranges):
        arr[k] = np.asarray(g, np.uint64)
    return torch.from_numpy(arr.view(np.int64)).cuda()


def _dev_rows(rows, n=None):
    """(rows, 4) int64 on the device in hsrans_member_range's layout: `rows` ((member, offset, length, dst_offset)), then garbage up to `n`"""
    arr = np.full((max(n or 0, len(rows)), 4), GARBAGE, np.uint64)
    for k, (m, off, length, dst) in enumerate(rows):
        arr[k] = np.asarray([off, length, dst, m], np.uint64)
    return torch.from_numpy(arr.view(np.int64)).cuda()


def _count(n):
    return torch.from_numpy(np.asarray([n], np.uint32).view(np.int32)).cuda()


# ---------------------------------------------------------------------------------------------------------------------
# 1. one frame, ranges on the device
# ---------------------------------------------------------------------------------------------------------------------
SINGLE = {"bf16-stored-plane": ("bf16-noisy", True), "fp32-coded": ("fp32", False), "i64": ("i64", True)}


class Single:
    def __init__(self, ctx, a, b, name, store):
        self.a, self.b, self.W = a, b, a.itemsize
        self.t, self.base = _tensor(a, name), _tensor(b, name)
        self.frame = _full(H.planes_capacity(self.W, 64, a.size) + PAD)
        work = _full(H.planes_workspace_bytes(self.W, a.size))
        _, self.desc, self.plans = ctx.encode_device_planes_delta(self.t, self.base, self.frame[:-PAD], work, **_settings(64, 11, 32, 1 << 16, store))
        self.planes = ctx.make_planes(self.desc, self.plans)
        self.pg = ctx.make_planes_gather(self.planes, self.frame[:-PAD])


@pytest.fixture(scope="module")
def singles(gpu_ctx, arrays):
    made = {}

    def get(key):
        if key not in made:
            name, store = SINGLE[key]
            made[key] = Single(gpu_ctx, arrays[name][0], arrays[name][1], _dtype_name(name), store)
        return made[key]

    yield get
    for s in made.values():
        s.pg.close()
        s.planes.close()


@pytest.mark.parametrize("counted", [True, False], ids=["count-on-the-device", "count-none"])
@pytest.mark.parametrize("first", [0, 1], ids=["from-element-0", "from-element-1"])
@pytest.mark.parametrize("key", sorted(SINGLE))
def test_the_single_indirect_delta_gathers_the_tensors_rows(gpu_ctx, singles, key, first, counted):
    s = singles(key)
    W = s.W
    if key == "bf16-stored-plane":
        assert s.desc.stored_mask == 0b01
    elif key == "fp32-coded":
        assert s.desc.stored_mask == 0
    rows, n_out = _rows(first)
    assert rows[-1][0] + rows[-1][1] == BIG
    assert rows[0][2] == first and all(((dst - off) * W) % 16 == (0 if first == 0 else W) for off, n, dst in rows)
    out_bytes = (n_out + 5) * W
    # the host-ranges delta call: its regions lie up256(sum of slots) apart
    stride = _up(sum(_up(off % 16 + n, 16) for off, n, _ in rows), 256)
    host_out, host_work = _full(out_bytes + PAD), _full(W * stride + PAD)
    gpu_ctx.decode_device_planes_gather_delta(s.pg, rows, s.base, host_out[:out_bytes].view(TORCH_INT[W]), host_work[:-PAD])
    assert gpu_ctx.planes_gather_status(s.pg) == [0] * W
    # the indirect one, shaped to the same regions: up256(max_elements + 30 max_count) == stride
    max_count = len(rows) + 3 if counted else len(rows)
    max_elements = stride - 30 * max_count
    assert H.planes_gather_workspace_bytes(W, max_count, max_elements) == W * stride
    out, work = _full(out_bytes + PAD), _full(W * stride + PAD)
    ws_bytes = H.planes_gather_indirect_workspace_bytes(W, max_count)
    ws = _full(ws_bytes + PAD)
    got = gpu_ctx.decode_device_planes_gather_indirect_delta(s.pg, _dev_ranges(rows, n=max_count), s.base, out[:out_bytes].view(TORCH_INT[W]), work[:-PAD],
                                                             count=_count(len(rows)) if counted else None, max_count=max_count, max_elements=max_elements,
                                                             workspace=ws[:ws_bytes])
    assert got.data_ptr() == ws.data_ptr()
    assert gpu_ctx.planes_gather_refused(s.pg) == 0
    assert gpu_ctx.planes_gather_status(s.pg) == [0] * W
    want = np.full(out.numel(), SENTINEL, np.uint8)
    flat = s.a.view(np.uint8)
    for off, n, dst in rows:
        want[dst * W: (dst + n) * W] = flat[off * W: (off + n) * W]
    assert np.array_equal(out.cpu().numpy(), want)  # numpy's rows of the TENSOR, everything else untouched
    assert torch.equal(out, host_out) and torch.equal(work, host_work)  # ... and the host-ranges delta call's bytes, workspace included
    assert _untouched(work[-PAD:]) and _untouched(ws[-PAD:])
    assert np.array_equal(_bytes(s.base), s.b.view(np.uint8))  # the base is as it was
    # the plain twin writes the same workspace: the residue's plane bytes
    plain_out, plain_work = _full(out_bytes + PAD), _full(W * stride + PAD)
    gpu_ctx.decode_device_planes_gather_indirect(s.pg, _dev_ranges(rows, n=max_count), plain_out[:out_bytes].view(TORCH_INT[W]), plain_work[:-PAD],
                                                 count=_count(len(rows)) if counted else None, max_count=max_count, max_elements=max_elements, workspace=ws[:ws_bytes])
    assert gpu_ctx.planes_gather_refused(s.pg) == 0
    assert torch.equal(plain_work, work)


# ---------------------------------------------------------------------------------------------------------------------
# 2 - 5. many frames
# ---------------------------------------------------------------------------------------------------------------------
# (input, base: None, "own", or the name of the member whose base tensor it shares)
MEMBERS = [
    ("bf16", "own"),
    ("fp16", "own"),
    ("fp32", "own"),
    ("i64", "own"),
    ("bf16-second", "bf16"),  # the very same base tensor as member 0
    ("fp32-alone", None),
    ("uniform", "own"),       # uniform bytes against a Gaussian base: every plane stored
    ("bf16-same", "own"),     # the tensor equals its base: the residue is zero
]
K = len(MEMBERS)
NO_BASE = 5


class World:
    def __init__(self, ctx, arrays):
        self.ctx = ctx
        self.arrays = [arrays[name][0] for name, _ in MEMBERS]
        self.base_arrays = [arrays[name][1] for name, _ in MEMBERS]
        self.W = [a.itemsize for a in self.arrays]
        self.tensors = [_tensor(a, _dtype_name(name)) for a, (name, _) in zip(self.arrays, MEMBERS)]
        own = {}
        self.bases = []
        for (name, kind), b in zip(MEMBERS, self.base_arrays):
            if kind is None:
                self.bases.append(None)
            elif kind == "own":
                own[name] = _tensor(b, _dtype_name(name))
                self.bases.append(own[name])
            else:
                self.bases.append(own[kind])
        self.frames = [_full(H.planes_capacity(a.itemsize, 64, a.size) + PAD) for a in self.arrays]
        work = _full(H.planes_batch_workspace_bytes(self.W, [a.size for a in self.arrays]))
        got = ctx.encode_device_planes_delta_batch(self.tensors, self.bases, [f[:-PAD] for f in self.frames], work, **DEFAULTS)
        self.descs, self.plans = [g[1] for g in got], [g[2] for g in got]
        self.pset = ctx.make_planes_set(self.descs, self.plans)
        self.pgs = ctx.make_planes_gather_set(self.pset, [f[:-PAD] for f in self.frames])
        self.bs = ctx.make_planes_base_set(self.pgs, self.bases)
        self.none = ctx.make_planes_base_set(self.pgs, [None] * K)
        self.planes = [ctx.make_planes(d, p) for d, p in zip(self.descs, self.plans)]
        self.pg = [ctx.make_planes_gather(p, f[:-PAD]) for p, f in zip(self.planes, self.frames)]
        self.base_before = [None if b is None else b.clone() for b in self.bases]

    def close(self):
        for h in [self.bs, self.none] + self.pg + self.planes + [self.pgs, self.pset]:
            h.close()

    # ---- rows: every member's _rows(first) in a region of its own of one output, all rows shuffled ----
    def rows(self, first, seed, members=range(K)):
        rows, at = [], 0
        for m in members:
            mine, n_out = _rows(first)
            rows += [(m, off, n, at // self.W[m] + dst) for off, n, dst in mine]
            at = _up(at + (n_out + 1) * self.W[m], 128)
        random.Random(seed).shuffle(rows)
        return rows, at

    def expected(self, rows, out_bytes, residue=False):
        want = np.full(out_bytes, SENTINEL, np.uint8)
        for m, off, n, dst in rows:
            W = self.W[m]
            a = self.arrays[m] if not residue or self.base_arrays[m] is None else self.arrays[m] ^ self.base_arrays[m]
            want[dst * W: (dst + n) * W] = a.view(np.uint8)[off * W: (off + n) * W]
        return want

    def work_bytes(self, rows, max_count=None):
        return H.planes_gather_batch_workspace_bytes(8, max_count or len(rows), sum(r[2] for r in rows))

    def clean(self):
        assert self.ctx.planes_gather_set_refused(self.pgs) == 0
        assert self.ctx.planes_gather_set_status(self.pgs) == [0] * K

    def bases_unchanged(self):
        return all(b is None or torch.equal(b, before) for b, before in zip(self.bases, self.base_before))


@pytest.fixture(scope="module")
def world(gpu_ctx, arrays):
    w = World(gpu_ctx, arrays)
    yield w
    w.close()


class Buffers:
    """out and d_work of one call, each with PAD sentinel bytes behind it; for the indirect forms a control workspace likewise"""

    def __init__(self, w, out_bytes, work_bytes, max_count=None):
        self.out_bytes, self.work_bytes = out_bytes, work_bytes
        self.out, self.work = _full(out_bytes + PAD), _full(work_bytes + PAD)
        if max_count is not None:
            self.ws_bytes = H.planes_gather_batch_indirect_workspace_bytes(w.pgs.coded, w.pgs.max_itemsize, max_count)
            assert self.ws_bytes > 0
            self.ws = _full(self.ws_bytes + PAD)

    def args(self):
        return self.out[:self.out_bytes], self.work[:self.work_bytes]

    def pads_untouched(self):
        return _untouched(self.out[-PAD:]) and _untouched(self.work[-PAD:]) and (not hasattr(self, "ws") or _untouched(self.ws[-PAD:]))

    def untouched(self):
        return _untouched(self.out) and _untouched(self.work) and (not hasattr(self, "ws") or _untouched(self.ws[-PAD:]))

    def refill(self):
        self.out.fill_(SENTINEL)
        self.work.fill_(SENTINEL)


def test_the_fixture_is_what_it_claims(world):
    w = world
    assert w.bases[0] is w.bases[4] and w.bases[NO_BASE] is None
    assert sorted(set(w.W)) == [2, 4, 8]
    assert w.descs[6].stored_mask == 0b11, "uniform bytes against a Gaussian base: every plane stored"
    assert np.array_equal(w.arrays[7], w.base_arrays[7])
    rows, _ = w.rows(0, 3)
    assert [r[0] for r in rows] != sorted(r[0] for r in rows) and {r[0] for r in rows} == set(range(K))


@pytest.mark.parametrize("first", [0, 1], ids=["from-element-0", "from-element-1"])
def test_the_batch_delta_gathers_every_members_rows(gpu_ctx, world, first):
    w = world
    rows, out_bytes = w.rows(first, 3 + first)
    for m, off, n, dst in rows:
        assert ((dst - off) * w.W[m]) % 16 == (0 if first == 0 else w.W[m])
    b = Buffers(w, out_bytes, w.work_bytes(rows))
    gpu_ctx.decode_device_planes_gather_batch_delta(w.pgs, w.bs, rows, *b.args())
    w.clean()
    info = w.pgs.info()
    assert np.array_equal(b.out.cpu().numpy(), w.expected(rows, out_bytes + PAD))  # numpy's rows of the TENSORS and nothing else
    assert b.pads_untouched() and w.bases_unchanged()
    # every member's rows by decode_device_planes_gather_delta on its own gather object (without a base: decode_device_planes_gather)
    single = _full(out_bytes + PAD)
    for m in range(K):
        W = w.W[m]
        mine = [(off, n, dst) for k, off, n, dst in rows if k == m]
        work = _full(H.planes_gather_workspace_bytes(W, len(mine), sum(r[1] for r in mine)))
        view = single[:out_bytes].view(TORCH_INT[W])
        if w.bases[m] is None:
            gpu_ctx.decode_device_planes_gather(w.pg[m], mine, view, work)
        else:
            gpu_ctx.decode_device_planes_gather_delta(w.pg[m], mine, w.bases[m], view, work)
        assert gpu_ctx.planes_gather_status(w.pg[m]) == [0] * W
    assert torch.equal(b.out, single)
    # the plain call on the same rows: the residues, the same workspace bytes, the same info; the member without a base gets the same rows
    p = Buffers(w, out_bytes, w.work_bytes(rows))
    gpu_ctx.decode_device_planes_gather_batch(w.pgs, rows, *p.args())
    w.clean()
    assert w.pgs.info() == info
    assert np.array_equal(p.out.cpu().numpy(), w.expected(rows, out_bytes + PAD, residue=True))
    assert torch.equal(p.work, b.work)
    for m, off, n, dst in rows:
        if m == NO_BASE:
            assert torch.equal(p.out[dst * 4: (dst + n) * 4], b.out[dst * 4: (dst + n) * 4])


def _indirect(ctx, w, base_set, b, d_rows, count, max_count, stream=None):
    out, work = b.args()
    if base_set is None:
        got = ctx.decode_device_planes_gather_batch_indirect(w.pgs, d_rows, out, work, count=count, max_count=max_count, workspace=b.ws[:b.ws_bytes], stream=stream)
    else:
        got = ctx.decode_device_planes_gather_batch_indirect_delta(w.pgs, base_set, d_rows, out, work, count=count, max_count=max_count, workspace=b.ws[:b.ws_bytes],
                                                                   stream=stream)
    assert got.data_ptr() == b.ws.data_ptr()


@pytest.mark.parametrize("first", [0, 1], ids=["from-element-0", "from-element-1"])
def test_the_batch_indirect_delta_is_the_host_rows_call(gpu_ctx, world, first):
    w = world
    rows, out_bytes = w.rows(first, 5 + first)
    ROWS = len(rows) + 4
    wb = w.work_bytes(rows, ROWS)
    host = Buffers(w, out_bytes, wb)
    gpu_ctx.decode_device_planes_gather_batch_delta(w.pgs, w.bs, rows, *host.args())
    w.clean()
    assert np.array_equal(host.out.cpu().numpy(), w.expected(rows, out_bytes + PAD))
    for count, max_count in ((_count(len(rows)), ROWS), (None, len(rows))):
        b = Buffers(w, out_bytes, wb, max_count)
        _indirect(gpu_ctx, w, w.bs, b, _dev_rows(rows, n=ROWS), count, max_count)
        w.clean()
        assert torch.equal(b.out, host.out) and torch.equal(b.work, host.work)
        assert b.pads_untouched() and w.bases_unchanged()
        # what *_indirect_info says of the plain call holds for this one: the launches are the same kernels but the merge
        info = w.pgs.indirect_info(max_count, out_bytes, wb)
        assert info["launches"] == info["set_launches"] + 2
    # one bad row among good ones — a range one element beyond its member: nothing is written, and the refusal is reported once
    bad = rows[:40] + [(2, BIG - 4, 5, 0)] + rows[40:]
    b = Buffers(w, out_bytes, w.work_bytes(bad, ROWS), ROWS)
    _indirect(gpu_ctx, w, w.bs, b, _dev_rows(bad, n=ROWS), _count(len(bad)), ROWS)
    assert gpu_ctx.planes_gather_set_refused(w.pgs) == E_DEVICE
    assert gpu_ctx.planes_gather_set_refused(w.pgs) == 0
    assert gpu_ctx.planes_gather_set_status(w.pgs) == [0] * K
    assert b.untouched()


def test_an_all_null_base_set_gives_the_plain_calls(gpu_ctx, world):
    w = world
    rows, out_bytes = w.rows(0, 7)
    ROWS = len(rows)
    wb = w.work_bytes(rows)
    plain, delta = Buffers(w, out_bytes, wb), Buffers(w, out_bytes, wb)
    gpu_ctx.decode_device_planes_gather_batch(w.pgs, rows, *plain.args())
    gpu_ctx.decode_device_planes_gather_batch_delta(w.pgs, w.none, rows, *delta.args())
    w.clean()
    assert np.array_equal(plain.out.cpu().numpy(), w.expected(rows, out_bytes + PAD, residue=True))
    assert torch.equal(plain.out, delta.out) and torch.equal(plain.work, delta.work)
    plain, delta = Buffers(w, out_bytes, wb, ROWS), Buffers(w, out_bytes, wb, ROWS)
    _indirect(gpu_ctx, w, None, plain, _dev_rows(rows), None, ROWS)
    _indirect(gpu_ctx, w, w.none, delta, _dev_rows(rows), None, ROWS)
    w.clean()
    assert np.array_equal(plain.out.cpu().numpy(), w.expected(rows, out_bytes + PAD, residue=True))
    assert torch.equal(plain.out, delta.out) and torch.equal(plain.work, delta.work)
    assert delta.pads_untouched()


def test_a_captured_batch_indirect_delta_reads_the_rows_anew(gpu_ctx, world):
    """one captured call, a single line of kernels on a side stream; before every replay the rows and the count are overwritten in place"""
    w = world
    a, n_a = w.rows(0, 11)
    c, n_c = w.rows(1, 13, members=[6, 3, 5, 0])
    ROWS = max(len(a), len(c)) + 3
    out_bytes = max(n_a, n_c)
    wb = max(w.work_bytes(a, ROWS), w.work_bytes(c, ROWS))
    cap, direct = Buffers(w, out_bytes, wb, ROWS), Buffers(w, out_bytes, wb, ROWS)
    d_rows, d_count = _dev_rows([], n=ROWS), _count(ROWS)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            _indirect(gpu_ctx, w, w.bs, cap, d_rows, d_count, ROWS, stream=side)
    torch.cuda.synchronize()
    assert cap.untouched()  # capturing runs nothing
    for name, rows in (("rows A", a), ("rows C: another count, other members", c), ("rows A again", a)):
        d_rows.copy_(_dev_rows(rows, n=ROWS))
        d_count.copy_(_count(len(rows)))
        cap.refill()
        g.replay()
        torch.cuda.synchronize()
        w.clean()
        assert np.array_equal(cap.out.cpu().numpy(), w.expected(rows, out_bytes + PAD)), name
        direct.refill()
        _indirect(gpu_ctx, w, w.bs, direct, _dev_rows(rows, n=ROWS), _count(len(rows)), ROWS)
        w.clean()
        assert torch.equal(cap.out, direct.out) and torch.equal(cap.work, direct.work), name
        assert cap.pads_untouched()


# ---------------------------------------------------------------------------------------------------------------------
# 6. refusals (ctypes): nothing written, sentinels intact
# ---------------------------------------------------------------------------------------------------------------------
RANGES = [(16, 1000, 0), (3, 50, 1000)]


class Refused:
    """tests/test_gpu_planes_delta.py's small fp32 tensor with its base, delta frame and buffers; two gather sets over the frame; and `big`:
    a base with room behind it, so that every window laid over it stays inside one allocation"""

    def __init__(self, ctx, inputs):
        self.r = r = Refusals(ctx, inputs)
        self.pgs = ctx.make_planes_gather_set(r.pset, [r.good_frame])
        self.pgs2 = ctx.make_planes_gather_set(r.pset, [r.good_frame])
        self.wb1 = H.planes_gather_workspace_bytes(4, 2, 1050)
        self.ws1 = H.planes_gather_indirect_workspace_bytes(4, 2)
        self.wbk = H.planes_gather_batch_workspace_bytes(4, 2, 1050)
        self.wsk = H.planes_gather_batch_indirect_workspace_bytes(self.pgs.coded, 4, 2)
        assert 0 < self.wb1 <= r.wb and 0 < self.wbk <= r.wb and self.ws1 > 512 and self.wsk > 512
        self.ws = _full(max(self.ws1, self.wsk) + PAD)
        room = r.bytes + max(self.wb1, self.wbk, self.ws1, self.wsk) + 4096
        assert r.shared.numel() >= 4096 + r.bytes and r.shared.numel() >= max(self.ws1, self.wsk, self.wb1, self.wbk) + 512
        self.big = _full(room)
        self.big[: r.bytes] = r.base_buf[: r.bytes]
        # valid ranges / rows INSIDE the base, 1024 bytes in
        self.big[1024: 1024 + 48] = _dev_ranges(RANGES).view(torch.uint8).flatten()
        self.big[2048: 2048 + 64] = _dev_rows([(0,) + g for g in RANGES]).view(torch.uint8).flatten()
        self.big_before = self.big.clone()
        self.base_view = r.base_buf[: r.bytes].view(torch.float32)
        self.bs = ctx.make_planes_base_set(self.pgs, [self.base_view])
        self.bs2 = ctx.make_planes_base_set(self.pgs2, [self.base_view])
        self.bs_big = ctx.make_planes_base_set(self.pgs, [self.big[: r.bytes].view(torch.float32)])
        self.d_ranges, self.d_rows = _dev_ranges(RANGES), _dev_rows([(0,) + g for g in RANGES])
        self.ranges_before, self.rows_before = self.d_ranges.clone(), self.d_rows.clone()

    def untouched(self):
        return (self.r.untouched() and _untouched(self.ws) and torch.equal(self.big, self.big_before) and torch.equal(self.d_ranges, self.ranges_before)
                and torch.equal(self.d_rows, self.rows_before))

    def close(self):
        for h in (self.bs, self.bs2, self.bs_big, self.pgs, self.pgs2, self.r.pg, self.r.pset, self.r.planes):
            h.close()


@pytest.fixture(scope="module")
def refused(gpu_ctx):
    rng = np.random.default_rng(29)
    base = rng.standard_normal(4096).astype(np.float32)
    tuned = (base * (1 + 0.01 * rng.standard_normal(4096))).astype(np.float32)
    f = Refused(gpu_ctx, {"fp32": (tuned.view(np.uint32), base.view(np.uint32))})
    yield f
    f.close()


def _want(f):
    r = f.r
    want = np.full(r.bytes, SENTINEL, np.uint8)
    flat = _bytes(r.t)
    want[: 4 * 1000] = flat[4 * 16: 4 * 1016]
    want[4 * 1000: 4 * 1050] = flat[4 * 3: 4 * 53]
    return want


def test_the_single_indirect_delta_refuses_a_bad_base_and_every_aliasing(gpu_ctx, refused):
    f, r, L = refused, refused.r, gpu_ctx.L
    sh, fr, big = r.shared.data_ptr(), r.good_frame.data_ptr(), f.big.data_ptr()
    other = H.Context(0)

    def call(d_base, base_bytes, d_out=None, d_work=None, wb=None, d_ws=None, d_ranges=-1, ctx=gpu_ctx.handle):
        return L.hsrans_decode_device_planes_gather_indirect_delta(ctx, r.pg.handle, f.d_ranges.data_ptr() if d_ranges == -1 else d_ranges, None, 2, 1050, d_base, base_bytes,
                                                                   d_out or r.out.data_ptr(), r.bytes, d_work or r.work.data_ptr(), f.wb1 if wb is None else wb,
                                                                   d_ws or f.ws.data_ptr(), f.ws1, None)

    refusals = {
        "no base": call(None, r.bytes),
        "a base 8 bytes off the 16-byte grid": call(r.base + 8, r.bytes),
        "a base one byte short": call(r.base, r.bytes - 1),
        "the ranges' elements are not enough: the base is the whole tensor": call(r.base, 4 * 1050),
        "the base 16 bytes into the output": call(sh + 4096 + 16, r.bytes, d_out=sh + 4096),
        "the output 16 bytes into the base": call(big, r.bytes, d_out=big + 16),
        "the output exactly on the base": call(big, r.bytes, d_out=big),
        "the workspace inside the base": call(big, r.bytes, d_work=big + 256),
        "the base inside the workspace": call(sh + 256, r.bytes, d_work=sh),
        "the control workspace inside the base": call(big, r.bytes, d_ws=big + 256),
        "the base inside the control workspace": call(sh + 256, r.bytes, d_ws=sh),
        "the ranges inside the base": call(big, r.bytes, d_ranges=big + 1024),
        "the base inside the frame the object is bound to": call(fr + 256, r.bytes),
        "the base on the frame": call(fr, r.bytes),
        # the plain twin's own refusals come back from the delta entry
        "a misaligned output": call(r.base, r.bytes, d_out=r.out.data_ptr() + 8),
        "a workspace one byte short": call(r.base, r.bytes, wb=f.wb1 - 1),
        "no ranges": call(r.base, r.bytes, d_ranges=None),
        "another context": call(r.base, r.bytes, ctx=other.handle),
    }
    assert refusals == {k: E_ARG for k in refusals}, refusals
    assert gpu_ctx.planes_gather_refused(r.pg) == 0
    assert f.untouched()
    # with everything in order the very same call gathers
    out, work = _full(r.bytes), _full(f.wb1)
    assert call(r.base, r.bytes, d_out=out.data_ptr(), d_work=work.data_ptr()) == 0
    assert gpu_ctx.planes_gather_refused(r.pg) == 0 and gpu_ctx.planes_gather_status(r.pg) == [0] * 4
    assert np.array_equal(out.cpu().numpy(), _want(f))
    assert _untouched(f.ws[-PAD:])
    f.ws.fill_(SENTINEL)


def test_the_base_set_refuses_bad_bases(gpu_ctx, refused):
    f, r, L = refused, refused.r, gpu_ctx.L
    fr = r.good_frame.data_ptr()
    h = ctypes.c_void_p()
    other = H.Context(0)

    def create(d_base, base_bytes, ctx=gpu_ctx.handle, pgs=f.pgs.handle, out=ctypes.byref(h), arrays=True):
        ptrs, sizes = (ctypes.c_void_p * 1)(d_base), (ctypes.c_size_t * 1)(base_bytes)
        return L.hsrans_planes_base_set_create(ctx, pgs, ptrs if arrays else None, sizes, out)

    refusals = {
        "no context": create(r.base, r.bytes, ctx=None),
        "no gather set": create(r.base, r.bytes, pgs=None),
        "no bases": create(r.base, r.bytes, arrays=False),
        "no sizes": L.hsrans_planes_base_set_create(gpu_ctx.handle, f.pgs.handle, (ctypes.c_void_p * 1)(r.base), None, ctypes.byref(h)),
        "no result": create(r.base, r.bytes, out=None),
        "a set of another context": create(r.base, r.bytes, ctx=other.handle),
        "a base 8 bytes off the 16-byte grid": create(r.base + 8, r.bytes),
        "a base one byte short": create(r.base, r.bytes - 1),
        "a base inside the member's frame": create(fr + 256, r.bytes),
        "a base that ends inside the frame": create(fr - r.bytes + 16, r.bytes),
    }
    assert refusals == {k: E_ARG for k in refusals}, refusals
    assert not h.value
    L.hsrans_planes_base_set_destroy(None)
    # exactly enough bytes will do, and so will no base at all
    assert create(r.base, r.bytes) == 0 and h.value
    L.hsrans_planes_base_set_destroy(h)
    assert create(None, 0) == 0 and h.value
    L.hsrans_planes_base_set_destroy(h)
    # the wrapper: one base per member, of the member's shape
    for bases in ([], [f.base_view, f.base_view], [f.base_view[:-1]], [f.base_view.view(torch.int16)], [f.base_view.cpu()]):
        with pytest.raises(H.HsransError) as e:
            gpu_ctx.make_planes_base_set(f.pgs, bases)
        assert e.value.code == E_ARG
    with pytest.raises(H.HsransError) as e:
        gpu_ctx.decode_device_planes_gather_batch_delta(f.pgs, f.bs2, [(0,) + g for g in RANGES], r.out[: r.bytes], r.work[: f.wbk])
    assert e.value.code == E_ARG
    assert f.untouched()


def test_the_batch_deltas_refuse_a_bad_base_set_and_every_aliasing(gpu_ctx, refused):
    f, r, L = refused, refused.r, gpu_ctx.L
    big = f.big.data_ptr()
    rows = (api.MemberRange * 2)()
    for k, (off, n, dst) in enumerate(RANGES):
        rows[k].member, rows[k].offset, rows[k].length, rows[k].dst_offset, rows[k].reserved = 0, off, n, dst, 0
    other = H.Context(0)

    def host(bs, d_out=None, d_work=None, wb=None, pgs=None, ctx=gpu_ctx.handle, ranges=rows):
        return L.hsrans_decode_device_planes_gather_batch_delta(ctx, (pgs or f.pgs).handle, bs and bs.handle, ranges, 2, d_out or r.out.data_ptr(), r.bytes,
                                                                d_work or r.work.data_ptr(), f.wbk if wb is None else wb, None)

    def device(bs, d_out=None, d_work=None, d_ws=None, d_rows=-1, pgs=None, ctx=gpu_ctx.handle, ws_bytes=None):
        return L.hsrans_decode_device_planes_gather_batch_indirect_delta(ctx, (pgs or f.pgs).handle, bs and bs.handle, f.d_rows.data_ptr() if d_rows == -1 else d_rows, None, 2,
                                                                         d_out or r.out.data_ptr(), r.bytes, d_work or r.work.data_ptr(), f.wbk, d_ws or f.ws.data_ptr(),
                                                                         f.wsk if ws_bytes is None else ws_bytes, None)

    refusals = {}
    for name, call in (("host rows", host), ("device rows", device)):
        refusals.update({
            f"{name}: no base set": call(None),
            f"{name}: a base set of another gather set": call(f.bs2),
            f"{name}: a gather set the base set is not of": call(f.bs, pgs=f.pgs2),
            f"{name}: another context": call(f.bs, ctx=other.handle),
            f"{name}: the output 16 bytes into the base": call(f.bs_big, d_out=big + 16),
            f"{name}: the output exactly on the base": call(f.bs_big, d_out=big),
            f"{name}: the workspace inside the base": call(f.bs_big, d_work=big + 256),
            # the plain twin's own refusals come back from the delta entry
            f"{name}: a misaligned output": call(f.bs, d_out=r.out.data_ptr() + 8),
            f"{name}: no workspace": L.hsrans_decode_device_planes_gather_batch_delta(gpu_ctx.handle, f.pgs.handle, f.bs.handle, rows, 2, r.out.data_ptr(), r.bytes, None,
                                                                                     f.wbk, None) if call is host else
            L.hsrans_decode_device_planes_gather_batch_indirect_delta(gpu_ctx.handle, f.pgs.handle, f.bs.handle, f.d_rows.data_ptr(), None, 2, r.out.data_ptr(), r.bytes,
                                                                      None, f.wbk, f.ws.data_ptr(), f.wsk, None),
        })
    refusals.update({
        "host rows: a workspace one byte below the rows' need": host(f.bs, wb=_up(4 * (1008 + 64), 256) - 1),
        "host rows: no rows": host(f.bs, ranges=None),
        "device rows: the control workspace inside the base": device(f.bs_big, d_ws=big + 256),
        "device rows: the rows inside the base": device(f.bs_big, d_rows=big + 2048),
        "device rows: a control workspace one byte short": device(f.bs, ws_bytes=f.wsk - 1),
        "device rows: no rows": device(f.bs, d_rows=None),
    })
    assert refusals == {k: E_ARG for k in refusals}, refusals
    assert gpu_ctx.planes_gather_set_refused(f.pgs) == 0
    assert f.untouched()
    # with everything in order both gather, into buffers of their own
    for call in (host, device):
        out, work = _full(r.bytes), _full(f.wbk)
        assert call(f.bs, d_out=out.data_ptr(), d_work=work.data_ptr()) == 0
        assert gpu_ctx.planes_gather_set_refused(f.pgs) == 0 and gpu_ctx.planes_gather_set_status(f.pgs) == [0]
        assert np.array_equal(out.cpu().numpy(), _want(f))
    assert _untouched(f.ws[-PAD:])
    f.ws.fill_(SENTINEL)
