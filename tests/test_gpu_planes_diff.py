"""hsrans_*_device_planes_diff: tensors coded against a base as a zigzag difference.  The invariant is what every test here leans on: a diff
frame of `in` against `base` is, byte for byte, the ordinary frame of z = zigzag(in - base), the elements read as little-endian unsigned
integers — so the expected frame, descriptor and plans are always what encode_device_planes gives for a PRECOMPUTED z (numpy:
planes_diff_cases.zigzag), and the expected tensor is always a numpy array.  The fixture is test_gpu_planes_delta.py's, built the same
way: `base` 1,000,003 standard-normal fp32 values (seed 29), `tuned` = base * (1 + 0.01 * standard_normal) from the same generator.
Every destination is pre-filled with a sentinel, has sentinel bytes behind it, and is compared whole.

Unlike the XOR kernels these can go wrong in their arithmetic: the carry cases (planes_diff_cases.carry_cases) are planted as the first
elements, inside a full block, in the tail and as the last elements, for the kernels alone and for the range merge's heads and tails.

The size test's figures, measured on an MI355X: see test_the_diff_frame_is_well_below_the_delta_frame's docstring."""
import ctypes

import numpy as np
import pytest
import torch

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api
from planes_diff_cases import CARRY_N, NP_UINT, carry_cases, planes_of, planted, zigzag

pytestmark = pytest.mark.gpu

E_ARG = 2
SENTINEL = 0xA5
PAD = 64  # sentinel bytes behind every destination
N_MAX = 1_000_003
BIG = 2 * 65536 + 77
NP_INT = {2: np.int16, 4: np.int32, 8: np.int64}
TORCH_INT = {2: torch.int16, 4: torch.int32, 8: torch.int64}
REAL = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}


# ---- inputs: name -> (in, base), numpy arrays of unsigned 2-, 4- or 8-byte items, made once and never changed ----
@pytest.fixture(scope="module")
def inputs():
    rng = np.random.default_rng(29)
    base = rng.standard_normal(N_MAX).astype(np.float32)
    tuned = (base * (1 + 0.01 * rng.standard_normal(N_MAX))).astype(np.float32)
    ramp = np.arange(N_MAX, dtype=np.uint64) << np.uint64(8)
    bf16 = lambda x: (x.view(np.uint32) >> 16).astype(np.uint16)  # noqa: E731  (truncated to bf16: the top 16 bits)
    pairs = {
        "bf16": (bf16(tuned), bf16(base)),
        "fp16": (tuned.astype(np.float16).view(np.uint16), base.astype(np.float16).view(np.uint16)),
        "fp32": (tuned.view(np.uint32), base.view(np.uint32)),
        "i64": (ramp + rng.integers(0, 1000, N_MAX, dtype=np.uint64), ramp + rng.integers(0, 1000, N_MAX, dtype=np.uint64)),
    }
    # the gather's frame with a stored plane: the low byte of z is uniform, the high byte small (drawn last: the pairs above are the delta test's)
    pairs["bf16-noisy"] = (bf16(tuned) ^ rng.integers(0, 256, N_MAX, dtype=np.uint16), bf16(base))
    for a, b in pairs.values():
        a.setflags(write=False)
        b.setflags(write=False)
    return pairs


def _tensor(a, name=None):
    """The device tensor of a numpy array of unsigned items: bf16 / fp16 / fp32 under their torch dtypes, the rest as signed integers."""
    t = torch.from_numpy(np.ascontiguousarray(a).view(NP_INT[a.itemsize]).copy()).cuda()
    real = REAL.get(name)
    return t.view(real) if real is not None else t


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def _full(n):
    return torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")


def _untouched(t):
    return bool((t == SENTINEL).all().item())


def _padded(a, name=None):
    """(buffer, view): the array's bytes in a device buffer with PAD sentinel bytes behind them, and the view over the array's elements"""
    raw = np.ascontiguousarray(a).view(np.uint8)
    buf = _full(raw.size + PAD)
    buf[: raw.size] = torch.from_numpy(raw.copy()).cuda()
    view = buf[: raw.size].view(TORCH_INT[a.itemsize])
    return buf, (view.view(REAL[name]) if name in REAL else view)


def _buffers(W, states, n):
    return _full(H.planes_capacity(W, states, n) + PAD), _full(H.planes_workspace_bytes(W, n) + PAD)


# ---- 1. the kernels alone ----
SIZES = [1, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097, BIG]


def _random_pair(W, n, salt):
    rng = np.random.default_rng(salt * 10_000_000 + W * 1_000_000 + n)
    return rng.integers(0, 256, n * W, dtype=np.uint8).view(NP_UINT[W]), rng.integers(0, 256, n * W, dtype=np.uint8).view(NP_UINT[W])


def _check_split(ctx, a, b):
    W, n = a.itemsize, a.size
    d_in, d_base = _tensor(a), _tensor(b)
    planes = [_full(n + PAD) for _ in range(W)]
    ctx.planes_split_diff_device(d_in, d_base, planes)
    torch.cuda.synchronize()
    want = planes_of(zigzag(a, b))
    for p in range(W):
        got = planes[p].cpu().numpy()
        assert np.array_equal(got[:n], want[p]), p
        assert np.all(got[n:] == SENTINEL), p
    assert np.array_equal(_bytes(d_in), a.view(np.uint8)) and np.array_equal(_bytes(d_base), b.view(np.uint8))


def _check_merge(ctx, a, b, in_place):
    W, n = a.itemsize, a.size
    want = planes_of(zigzag(a, b))
    d_planes = [torch.from_numpy(want[p]).cuda() for p in range(W)]
    base_buf, d_base = _padded(b)
    if in_place:
        out_buf, out = base_buf, d_base
    else:
        out_buf = _full(n * W + PAD)
        out = out_buf[: n * W].view(TORCH_INT[W])
    ctx.planes_merge_diff_device(d_planes, d_base, out)
    torch.cuda.synchronize()
    got = out_buf.cpu().numpy()
    assert np.array_equal(got[: n * W], a.view(np.uint8))
    assert np.all(got[n * W:] == SENTINEL)
    if not in_place:
        assert np.array_equal(base_buf.cpu().numpy()[: n * W], b.view(np.uint8)) and _untouched(base_buf[n * W:])
    for p in range(W):
        assert np.array_equal(d_planes[p].cpu().numpy(), want[p]), p


@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_the_split_kernel_equals_numpys_split_of_z(gpu_ctx, W, n):
    _check_split(gpu_ctx, *_random_pair(W, n, 1))


@pytest.mark.parametrize("in_place", [False, True], ids=["apart", "in-place"])
@pytest.mark.parametrize("W", [2, 4, 8])
@pytest.mark.parametrize("n", SIZES)
def test_the_merge_kernel_undoes_numpys_z(gpu_ctx, W, n, in_place):
    _check_merge(gpu_ctx, *_random_pair(W, n, 2), in_place)


# ---- 2. the carry cases: first elements, a full block, the tail, last elements ----
@pytest.mark.parametrize("W", [2, 4, 8])
def test_the_kernels_carry_and_borrow_within_an_element_and_never_beyond(gpu_ctx, W):
    a, b, starts = planted(W, 11)
    ca, cb = carry_cases(W)
    assert starts[0] == 0 and starts[1] + ca.size <= CARRY_N // 16 * 16 <= starts[2] and starts[3] + ca.size == CARRY_N
    assert all(np.array_equal(a[s: s + ca.size], ca) and np.array_equal(b[s: s + cb.size], cb) for s in starts)
    z = zigzag(ca, cb)
    assert z[0] == 2 and z[1] == np.iinfo(z.dtype).max and z[2] == 2
    _check_split(gpu_ctx, a, b)
    _check_merge(gpu_ctx, a, b, False)
    _check_merge(gpu_ctx, a, b, True)


# ---- 3. frame identity, 4. round trip ----
# (input, states, bits, index_interval, block_size, elements)
CASES = [
    ("bf16", 64, 11, 32, 1 << 16, N_MAX),
    ("fp16", 32, 13, 0, 1 << 14, 1025),
    ("fp32", 64, 11, 32, 1 << 16, BIG),
    ("i64", 64, 11, 32, 1 << 14, 65536),
    ("bf16", 64, 11, 32, 1 << 16, 1),
    ("fp32", 64, 11, 32, 1 << 16, 17),
]
CASE_IDS = [f"{c[0]}-s{c[1]}-b{c[2]}-i{c[3]}-n{c[5]}" for c in CASES]


def _settings(states, bits, interval, block, store):
    return dict(states=states, bits=bits, block_size=block, index_interval=interval, store_incompressible=store)


class Encoded:
    """One tensor encoded twice: by the diff call against its base, and by the plain call from a precomputed z"""

    def __init__(self, ctx, a, b, name, settings):
        self.a, self.b, self.W, self.n = a, b, a.itemsize, a.size
        self.z = zigzag(a, b)
        self.t, self.base = _tensor(a, name), _tensor(b, name)
        states = settings["states"]
        self.frame, self.work = _buffers(self.W, states, self.n)
        self.total, self.desc, self.plans = ctx.encode_device_planes_diff(self.t, self.base, self.frame[:-PAD], self.work[:-PAD], **settings)
        self.plain_frame, plain_work = _buffers(self.W, states, self.n)
        self.plain_total, self.plain_desc, self.plain_plans = ctx.encode_device_planes(_tensor(self.z), self.plain_frame[:-PAD], plain_work[:-PAD], **settings)


@pytest.mark.parametrize("store", [False, True], ids=["coded", "store"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_a_diff_frame_is_the_plain_frame_of_z_and_decodes_to_the_tensor(gpu_ctx, inputs, case, store):
    name, states, bits, interval, block, n = case
    a, b = inputs[name][0][:n], inputs[name][1][:n]
    e = Encoded(gpu_ctx, a, b, name, _settings(states, bits, interval, block, store))
    W = e.W
    # -- the frame, the descriptor, the plans
    assert e.total == e.plain_total == e.desc.frame_length
    assert bytes(e.desc) == bytes(e.plain_desc)
    assert (e.desc.elem_size, e.desc.elements) == (W, n)  # (the frame names neither its base nor its rule: nothing else to find in it)
    got, want = e.frame.cpu().numpy(), e.plain_frame.cpu().numpy()
    for p in range(W):
        lo, hi = e.desc.offset[p], e.desc.offset[p] + e.desc.length[p]
        assert np.array_equal(got[lo:hi], want[lo:hi]), p
        end = e.desc.offset[p + 1] if p + 1 < W else got.size - PAD
        # nothing written past a plane's stream (a stored plane lies over the stream that did not shrink: there, what the plain call leaves)
        assert np.all(got[hi:end] == SENTINEL) if not e.desc.stored_mask >> p & 1 else np.array_equal(got[hi:end], want[hi:end]), p
        assert (e.plans[p] is None) == (e.plain_plans[p] is None) == bool(e.desc.stored_mask >> p & 1), p
        if e.plans[p] is not None:
            assert np.array_equal(gpu_ctx.read_device_plan(e.plans[p]), gpu_ctx.read_device_plan(e.plain_plans[p])), p
    if not store:
        assert e.desc.stored_mask == 0
    assert _untouched(e.work[-PAD:]) and _untouched(e.frame[-PAD:])
    assert np.array_equal(_bytes(e.t), a.view(np.uint8)) and np.array_equal(_bytes(e.base), b.view(np.uint8))  # inputs unchanged
    # -- the decodes
    planes = gpu_ctx.make_planes(e.desc, e.plans)
    plain = gpu_ctx.make_planes(e.plain_desc, e.plain_plans)
    assert planes.info() == plain.info()  # coded, stored and the launches of one decode
    frame = e.frame[:-PAD]
    # into an output of its own
    out_buf, work = _full(n * W + PAD), _full(e.work.numel())
    gpu_ctx.decode_device_planes_diff(planes, frame, e.base, out_buf[: n * W].view(e.t.dtype), work[:-PAD])
    assert gpu_ctx.planes_status(planes) == [0] * W
    assert np.array_equal(out_buf.cpu().numpy()[: n * W], a.view(np.uint8)) and _untouched(out_buf[n * W:]) and _untouched(work[-PAD:])
    assert np.array_equal(_bytes(e.base), b.view(np.uint8))
    # in place, over a copy of the base
    copy_buf, copy = _padded(b, name)
    gpu_ctx.decode_device_planes_diff(planes, frame, copy, copy, work[:-PAD])
    assert gpu_ctx.planes_status(planes) == [0] * W
    assert np.array_equal(copy_buf.cpu().numpy()[: n * W], a.view(np.uint8)) and _untouched(copy_buf[n * W:])
    # the plain decode of the same frame gives z: intended
    res_buf = _full(n * W + PAD)
    gpu_ctx.decode_device_planes(planes, frame, res_buf[: n * W].view(e.t.dtype), work[:-PAD])
    assert gpu_ctx.planes_status(planes) == [0] * W
    assert np.array_equal(res_buf.cpu().numpy()[: n * W], e.z.view(np.uint8)) and _untouched(res_buf[n * W:])
    planes.close()
    plain.close()


def _same_frame(desc, frame, want_desc, want_frame):
    if bytes(desc) != bytes(want_desc):
        return False
    return all(torch.equal(frame[desc.offset[p]: desc.offset[p] + desc.length[p]], want_frame[desc.offset[p]: desc.offset[p] + desc.length[p]])
               for p in range(desc.elem_size))


# ---- 5. size: the test that makes the point ----
def test_the_diff_frame_is_well_below_the_delta_frame(gpu_ctx, inputs):
    """The bf16 fixture, 64 states, 11 bits, interval 32, 64 KiB blocks, stored planes allowed.  Coded by the library's HOST encoder, plane by
    plane with the same settings, the XOR residue comes to 464,404 + 18,844 = 483,248 bytes and z to 385,312 + 144 = 385,456: ratio 0.798.
    The bound of 0.85 leaves room for nothing but a changed normalisation.  The frames are compared by the sum of their planes' lengths
    and as hsrans_planes_pack_device lays them out (an unpacked frame_length holds plane 1's fixed offset and says nothing about size).
    Measured on an MI355X: delta planes 464,404 + 18,844 = 483,248 bytes (0.2416 of the tensor), diff planes 385,312 + 144 = 385,456 bytes
    (0.1927 of the tensor), none stored: ratio 0.7976 — the host encoder's figures to the byte; packed frames 483,260 and 385,456 bytes."""
    a, b = inputs["bf16"]
    settings = _settings(64, 11, 32, 1 << 16, True)
    e = Encoded(gpu_ctx, a, b, "bf16", settings)
    t, base = _tensor(a, "bf16"), _tensor(b, "bf16")
    frame, work = _buffers(2, 64, a.size)
    _, delta_desc, _ = gpu_ctx.encode_device_planes_delta(t, base, frame[:-PAD], work[:-PAD], **settings)
    packed = lambda d: H.planes_pack_layout([d])[0][0].frame_length  # noqa: E731
    coded = lambda d: sum(d.length[p] for p in range(d.elem_size))  # noqa: E731
    print(f"\nbf16 fixture, {a.size} elements: delta planes {[delta_desc.length[p] for p in range(2)]} = {coded(delta_desc)} bytes "
          f"({coded(delta_desc) / (2 * a.size):.4f} of the tensor), diff planes {[e.desc.length[p] for p in range(2)]} = {coded(e.desc)} bytes "
          f"({coded(e.desc) / (2 * a.size):.4f} of the tensor), ratio {coded(e.desc) / coded(delta_desc):.4f}; packed frames {packed(delta_desc)} and "
          f"{packed(e.desc)}, ratio {packed(e.desc) / packed(delta_desc):.4f}; stored masks {delta_desc.stored_mask} / {e.desc.stored_mask}")
    assert coded(e.desc) < 0.85 * coded(delta_desc)
    assert packed(e.desc) < 0.85 * packed(delta_desc)


# ---- 6. batch ----
# (input, elements, base: None, "own", or "shared" (members with it share ONE base buffer), options)
MEMBERS = [
    ("bf16", 65536 + 3, "shared", dict(bits=11, index_interval=32)),
    ("fp32", 4097, None, dict(bits=12, index_interval=0)),
    ("bf16", 65536 + 3, "shared", dict(bits=13, index_interval=16, states=32)),  # the very same base as member 0
    ("i64", 40_000, "own", dict(bits=11, index_interval=32, block_size=1 << 14)),
    ("fp16", 17, None, dict(bits=10, index_interval=0, store_incompressible=False)),
    ("fp32", BIG, "own", dict(bits=11, index_interval=32)),
]
DEFAULTS = dict(states=64, bits=11, block_size=1 << 16, index_interval=32, store_incompressible=True)


class Batch:
    def __init__(self, ctx, inputs):
        self.arrays, self.base_arrays, self.tensors, self.bases = [], [], [], []
        shared = None
        for name, n, kind, _ in MEMBERS:
            a, b = inputs[name][0][:n], inputs[name][1][:n]
            self.arrays.append(a)
            self.base_arrays.append(None if kind is None else b)
            self.tensors.append(_tensor(a, name))
            if kind == "shared":
                shared = _tensor(b, name) if shared is None else shared
            self.bases.append(None if kind is None else shared if kind == "shared" else _tensor(b, name))
        self.options = [m[3] for m in MEMBERS]
        self.settings = [dict(DEFAULTS, **o) for o in self.options]
        self.frames = [_full(H.planes_capacity(a.itemsize, s["states"], a.size) + PAD) for a, s in zip(self.arrays, self.settings)]
        self.work_bytes = H.planes_batch_workspace_bytes([a.itemsize for a in self.arrays], [a.size for a in self.arrays])
        self.work = _full(self.work_bytes + PAD)
        self.stats = {}
        self.got = ctx.encode_device_planes_diff_batch(self.tensors, self.bases, [f[:-PAD] for f in self.frames], self.work[:-PAD], options=self.options,
                                                       stats=self.stats, **DEFAULTS)
        self.descs, self.plans = [g[1] for g in self.got], [g[2] for g in self.got]


@pytest.fixture(scope="module")
def batch(gpu_ctx, inputs):
    return Batch(gpu_ctx, inputs)


def test_every_batch_member_equals_its_single_call(gpu_ctx, batch):
    f = batch
    assert f.bases[0] is f.bases[2] and f.bases[1] is None and f.bases[4] is None
    assert sorted({a.itemsize for a in f.arrays}) == [2, 4, 8]
    assert f.stats["members"] == len(MEMBERS) and f.stats["planes"] == sum(a.itemsize for a in f.arrays)
    for k, (total, desc, plans) in enumerate(f.got):
        a, W = f.arrays[k], f.arrays[k].itemsize
        frame, work = _buffers(W, f.settings[k]["states"], a.size)
        if f.bases[k] is None:
            want_total, want_desc, want_plans = gpu_ctx.encode_device_planes(f.tensors[k], frame[:-PAD], work[:-PAD], **f.settings[k])
        else:
            want_total, want_desc, want_plans = gpu_ctx.encode_device_planes_diff(f.tensors[k], f.bases[k], frame[:-PAD], work[:-PAD], **f.settings[k])
        assert total == want_total and _same_frame(desc, f.frames[k], want_desc, frame), k
        got, want = f.frames[k].cpu().numpy(), frame.cpu().numpy()
        for p in range(W):
            assert (plans[p] is None) == (want_plans[p] is None), (k, p)
            if plans[p] is not None:
                assert np.array_equal(gpu_ctx.read_device_plan(plans[p]), gpu_ctx.read_device_plan(want_plans[p])), (k, p)
            hi, end = desc.offset[p] + desc.length[p], desc.offset[p + 1] if p + 1 < W else got.size
            assert np.all(got[hi:end] == SENTINEL) if plans[p] is not None else np.array_equal(got[hi:end], want[hi:end]), (k, p)  # (as the single call leaves it)
    assert _untouched(f.work[-PAD:])
    for k, a in enumerate(f.arrays):  # inputs and bases unchanged
        assert np.array_equal(_bytes(f.tensors[k]), a.view(np.uint8)), k
        assert f.bases[k] is None or np.array_equal(_bytes(f.bases[k]), f.base_arrays[k].view(np.uint8)), k


def test_the_batch_decode_restores_every_member(gpu_ctx, batch):
    f = batch
    pset = gpu_ctx.make_planes_set(f.descs, f.plans)
    in_place = 3  # a member with a base of its own
    assert MEMBERS[in_place][2] == "own"
    bufs, outs, bases = [], [], list(f.bases)
    for k, a in enumerate(f.arrays):
        if k == in_place:
            buf, view = _padded(f.base_arrays[k], MEMBERS[k][0])
            bases[k] = view
        else:
            buf = _full(a.size * a.itemsize + PAD)
            view = buf[: a.size * a.itemsize].view(f.tensors[k].dtype)
        bufs.append(buf)
        outs.append(view)
    work = _full(pset.info()["work_bytes"] + PAD)
    frames = [fr[:-PAD] for fr in f.frames]
    gpu_ctx.decode_device_planes_diff_batch(pset, frames, bases, outs, work[:-PAD])
    assert gpu_ctx.planes_set_status(pset) == [0] * len(MEMBERS)
    for k, a in enumerate(f.arrays):
        got = bufs[k].cpu().numpy()
        assert np.array_equal(got[: a.size * a.itemsize], a.view(np.uint8)), k
        assert np.all(got[a.size * a.itemsize:] == SENTINEL), k
        assert f.bases[k] is None or np.array_equal(_bytes(f.bases[k]), f.base_arrays[k].view(np.uint8)), k
    assert _untouched(work[-PAD:])
    # each member against its single call's decode (a member without a base: the plain one)
    for k, a in enumerate(f.arrays):
        planes = gpu_ctx.make_planes(f.descs[k], f.plans[k])
        out = torch.zeros_like(f.tensors[k])
        own_work = _full(H.planes_workspace_bytes(a.itemsize, a.size))
        if f.bases[k] is None:
            gpu_ctx.decode_device_planes(planes, frames[k], out, own_work)
        else:
            gpu_ctx.decode_device_planes_diff(planes, frames[k], f.bases[k], out, own_work)
        assert gpu_ctx.planes_status(planes) == [0] * a.itemsize
        assert np.array_equal(_bytes(out), bufs[k].cpu().numpy()[: a.size * a.itemsize]), k
        planes.close()
    # the plain batch decode of the same frames: z
    plain = [torch.zeros_like(t) for t in f.tensors]
    gpu_ctx.decode_device_planes_batch(pset, frames, plain, work[:-PAD])
    assert gpu_ctx.planes_set_status(pset) == [0] * len(MEMBERS)
    for k, (a, b) in enumerate(zip(f.arrays, f.base_arrays)):
        assert np.array_equal(_bytes(plain[k]), (a if b is None else zigzag(a, b)).view(np.uint8)), k
    pset.close()


# ---- 7. gather ----
class Gathered:
    def __init__(self, ctx, a, b, name, store):
        self.e = Encoded(ctx, a, b, name, _settings(64, 11, 32, 1 << 16, store))
        self.planes = ctx.make_planes(self.e.desc, self.e.plans)
        self.pg = ctx.make_planes_gather(self.planes, self.e.frame[:-PAD])

    def close(self):
        self.pg.close()
        self.planes.close()


GATHERED = {"bf16-stored-plane": ("bf16-noisy", True), "fp32-coded": ("fp32", False), "i64-coded": ("i64", False)}


@pytest.fixture(scope="module")
def gathered(gpu_ctx, inputs):
    made = {}

    def get(key):
        if key not in made:
            name, store = GATHERED[key]
            made[key] = Gathered(gpu_ctx, inputs[name][0][:BIG], inputs[name][1][:BIG], name if name in REAL else None, store)
        return made[key]

    yield get
    for g in made.values():
        g.close()


def _rows(first):
    """(offset, length, dst_offset): every length at every phase of the source's 16-element grid, then a row that ends with the tensor.  The
    destinations are packed from element `first`, each moved up to the next element that lies `first` elements off the source's grid: from
    element 0 every whole block's byte address is 16-aligned (16-byte stores), from element 1 none is (element-wide stores)."""
    rows, at, off = [], first, 16 * 40

    def place(offset, length):
        nonlocal at
        at += (offset + first - at) % 16
        rows.append((offset, length, at))
        at += length

    for phase in (0, 1, 8, 15):
        for length in (1, 15, 17, 4096, 4096 + 3):
            place(off + phase, length)
            off += 16 * ((phase + length) // 16 + 3)
    place(BIG - 4099, 4099)
    return rows, at


def _check_gather(ctx, g, rows, n_out):
    e, W = g.e, g.e.W
    out = _full((n_out + 5) * W + PAD)
    work = _full(H.planes_gather_workspace_bytes(W, len(rows), sum(n for _, n, _ in rows)) + PAD)
    ctx.decode_device_planes_gather_diff(g.pg, rows, e.base, out[: (n_out + 5) * W].view(TORCH_INT[W]), work[:-PAD])
    assert ctx.planes_gather_status(g.pg) == [0] * W
    want = np.full(out.numel(), SENTINEL, np.uint8)
    flat = e.a.view(np.uint8)
    for off, n, dst in rows:
        want[dst * W: (dst + n) * W] = flat[off * W: (off + n) * W]
    assert np.array_equal(out.cpu().numpy(), want)  # each range the slice of `in`; everything else untouched
    assert _untouched(work[-PAD:])
    assert np.array_equal(_bytes(e.base), e.b.view(np.uint8))
    info = g.pg.info()
    # the plain gather of the same rows: z's rows, by the same launches
    plain = _full(out.numel())
    ctx.decode_device_planes_gather(g.pg, rows, plain[: (n_out + 5) * W].view(TORCH_INT[W]), work[:-PAD])
    assert ctx.planes_gather_status(g.pg) == [0] * W
    flat = e.z.view(np.uint8)
    for off, n, dst in rows:
        want[dst * W: (dst + n) * W] = flat[off * W: (off + n) * W]
    assert np.array_equal(plain.cpu().numpy(), want)
    assert g.pg.info() == info


@pytest.mark.parametrize("first", [0, 1], ids=["from-element-0", "from-element-1"])
@pytest.mark.parametrize("key", sorted(GATHERED))
def test_gathered_ranges_are_numpys_slices_of_the_tensor(gpu_ctx, gathered, key, first):
    g = gathered(key)
    e, W = g.e, g.e.W
    if key == "bf16-stored-plane":
        assert e.desc.stored_mask == 0b01 and e.plans[0] is None and e.plans[1] is not None
    else:
        assert e.desc.stored_mask == 0 and all(p is not None for p in e.plans)
    rows, n_out = _rows(first)
    assert rows[-1][0] + rows[-1][1] == BIG and all(off + n <= BIG for off, n, _ in rows)
    # ranges start and end off the 16-element grid; the store path of every whole block: 16-byte stores from element 0, element-wide from element 1
    assert any(off % 16 for off, _, _ in rows) and any((off + n) % 16 for off, n, _ in rows)
    assert rows[0][2] == first and all(((dst - off) * W) % 16 == (0 if first == 0 else W) for off, n, dst in rows)
    _check_gather(gpu_ctx, g, rows, n_out)


@pytest.mark.parametrize("W", [2, 4, 8])
def test_the_gathers_heads_and_tails_carry_within_an_element(gpu_ctx, W):
    """the carry cases in a frame of their own: as a range's head (elements 1 .. 15 of a block), inside full blocks with either store path,
    and as a range's tail"""
    a, b, starts = planted(W, 13)
    L = carry_cases(W)[0].size
    g = Gathered(gpu_ctx, a, b, None, False)
    rows = [(0, CARRY_N, 0), (1, CARRY_N - 1, 97), (33, 20, 200 + 1), (starts[2], L, 240 + 3), (CARRY_N - L, L, 270)]
    assert starts[1] == 32 and 33 + 20 > 48  # the third range: a head over the planted block's elements, then a tail, no whole block
    try:
        _check_gather(gpu_ctx, g, rows, 280)
    finally:
        g.close()


# ---- 8. refusals: each its delta twin's ----
def _ptrs(values, size=None):
    return (ctypes.c_void_p * (size or len(values)))(*values)


def _sizes(values):
    return (ctypes.c_size_t * len(values))(*values)


class Refusals:
    """a small fp32 tensor, its base, a diff frame of it and every buffer a call takes, with room around them"""

    def __init__(self, ctx, inputs):
        n = self.n = 4096
        a, b = inputs["fp32"][0][:n], inputs["fp32"][1][:n]
        self.a, self.b = a, b
        self.W, self.bytes = 4, 4 * n
        self.t = _tensor(a, "fp32")
        self.base_buf = _full(4 * n + 64)
        self.base_buf[: 4 * n] = torch.from_numpy(np.ascontiguousarray(b).view(np.uint8).copy()).cuda()
        self.base = self.base_buf.data_ptr()
        self.base_before = self.base_buf.clone()
        self.cap, self.wb = H.planes_capacity(4, 64, n), H.planes_workspace_bytes(4, n)
        self.frame, self.work, self.out = _full(self.cap + 64), _full(self.wb + 64), _full(4 * n + 64)
        self.shared = _full(self.cap + self.wb + 4 * n)  # for the overlaps: nothing in it may change
        good_frame, good_work = _full(self.cap), _full(self.wb)
        _, self.desc, self.plans = ctx.encode_device_planes_diff(self.t, self.base_buf[: 4 * n].view(torch.float32), good_frame, good_work, store_incompressible=False)
        self.good_frame = good_frame
        self.frame_before = good_frame.clone()
        self.planes = ctx.make_planes(self.desc, self.plans)
        _, desc2, plans2 = ctx.encode_device_planes_diff(self.t, self.base_buf[: 4 * n].view(torch.float32), _full(self.cap), good_work, store_incompressible=False)
        assert bytes(desc2) == bytes(self.desc)
        self.pset = ctx.make_planes_set([desc2], [plans2])  # (plans of its own: the same frame)
        self.pg = ctx.make_planes_gather(self.planes, good_frame)

    def untouched(self):
        torch.cuda.synchronize()
        return (_untouched(self.frame) and _untouched(self.work) and _untouched(self.out) and _untouched(self.shared) and torch.equal(self.base_buf, self.base_before)
                and torch.equal(self.good_frame, self.frame_before))


@pytest.fixture(scope="module")
def refusals(gpu_ctx, inputs):
    r = Refusals(gpu_ctx, inputs)
    yield r
    r.pg.close()
    r.pset.close()
    r.planes.close()


def _bad_bases(r, d_out=None):
    """(d_base, base_bytes, why) that every entry refuses; with d_out also the overlaps of an output and the base"""
    bad = [
        (None, r.bytes, "no base"),
        (r.base + 4, r.bytes, "a misaligned base"),
        (r.base, r.bytes - 1, "short base_bytes"),
    ]
    if d_out is not None:
        bad += [
            (d_out + 16, r.bytes, "the base 16 bytes into the output"),
            (d_out - 16, r.bytes, "the output 16 bytes into the base"),
        ]
    return bad


def test_the_kernel_entries_refuse_a_bad_base(gpu_ctx, refusals):
    r, L, ctx = refusals, gpu_ctx.L, gpu_ctx.handle
    planes = [_full(r.n + 16) for _ in range(4)]
    pp = _ptrs([p.data_ptr() for p in planes], 8)
    el = r.shared.data_ptr() + 256  # (room in front of it for a base that begins 16 bytes earlier)
    for d_base, _, why in _bad_bases(r)[:2] + [(planes[1].data_ptr(), 0, "the base on a plane"), (planes[2].data_ptr() + r.n - 16, 0, "the base ends on a plane")]:
        assert L.hsrans_planes_split_diff_device(ctx, 4, r.t.data_ptr(), d_base, r.n, pp, None) == E_ARG, why
        assert L.hsrans_planes_merge_diff_device(ctx, 4, pp, d_base, r.n, el, None) == E_ARG, why
    for d_base, why in [(el + 16, "the base 16 bytes into the output"), (el - 16, "the output 16 bytes into the base")]:
        assert L.hsrans_planes_merge_diff_device(ctx, 4, pp, d_base, r.n, el, None) == E_ARG, why
    assert L.hsrans_planes_split_diff_device(None, 4, r.t.data_ptr(), r.base, r.n, pp, None) == E_ARG
    assert L.hsrans_planes_split_diff_device(ctx, 3, r.t.data_ptr(), r.base, r.n, pp, None) == E_ARG
    assert L.hsrans_planes_merge_diff_device(ctx, 4, pp, r.base, 0, el, None) == E_ARG
    assert r.untouched() and all(_untouched(p) for p in planes)


def _encode_diff(L, r, ctx, d_base, base_bytes, d_frame=None, d_work=None, d_in=None):
    desc, handles = api.PlanesDesc(), (ctypes.c_void_p * 8)()
    got = L.hsrans_encode_device_planes_diff(ctx, 4, 64, 11, d_in or r.t.data_ptr(), d_base, base_bytes, r.n, d_frame or r.frame.data_ptr(), r.cap, 1 << 16, 32, 1,
                                             d_work or r.work.data_ptr(), r.wb, None, ctypes.byref(desc), handles)
    return got, bytes(desc) == bytes(api.PlanesDesc()) and not any(handles)


def test_the_encoder_refuses_a_bad_base(gpu_ctx, refusals):
    r, L, ctx = refusals, gpu_ctx.L, gpu_ctx.handle
    for d_base, base_bytes, why in _bad_bases(r):
        assert _encode_diff(L, r, ctx, d_base, base_bytes) == (0, True), why
    sh = r.shared.data_ptr()
    assert _encode_diff(L, r, ctx, sh + r.cap - 16, r.bytes, d_frame=sh) == (0, True)           # the base begins inside the frame
    assert _encode_diff(L, r, ctx, sh, r.bytes, d_frame=sh + r.bytes - 16) == (0, True)        # the frame begins inside the base
    assert _encode_diff(L, r, ctx, sh + 256, r.bytes, d_work=sh) == (0, True)                   # the base lies inside the workspace
    assert _encode_diff(L, r, ctx, sh, r.bytes + 4096, d_work=sh + r.bytes + 256) == (0, True)  # ... meets it only over base_bytes
    # all the plain call's refusals stay: a few of them
    assert _encode_diff(L, r, None, r.base, r.bytes) == (0, True)
    assert _encode_diff(L, r, ctx, r.base, r.bytes, d_in=r.t.data_ptr() + 4) == (0, True)
    assert _encode_diff(L, r, ctx, r.base, r.bytes, d_frame=r.frame.data_ptr() + 8) == (0, True)
    assert r.untouched()
    with pytest.raises(H.HsransError):
        gpu_ctx.encode_device_planes_diff(r.t, r.t[:-1], r.frame, r.work)  # a base of another element count
    with pytest.raises(H.HsransError):
        gpu_ctx.encode_device_planes_diff(r.t, r.t.view(torch.int16), r.frame, r.work)  # ... of another element size
    with pytest.raises(H.HsransError):
        gpu_ctx.encode_device_planes_diff(r.t, None, r.frame, r.work)
    assert r.untouched()


def test_the_batch_encoder_refuses_a_bad_base(gpu_ctx, refusals):
    r, L, ctx = refusals, gpu_ctx.L, gpu_ctx.handle

    frame1, frame2, work2 = _full(r.cap), _full(r.cap), _full(2 * r.wb)

    def call(bases, base_bytes, null_arrays=False):
        m = (api.PlanesMember * 2)()
        frames = [frame1.data_ptr(), frame2.data_ptr()]
        for k in range(2):
            m[k].elem_size, m[k].states, m[k].bits, m[k].block_size, m[k].index_interval, m[k].flags = 4, 64, 11, 1 << 16, 32, 1
            m[k].d_in, m[k].elements, m[k].d_frame, m[k].frame_capacity = r.t.data_ptr(), r.n, frames[k], r.cap
        handles = (ctypes.c_void_p * 16)()
        rc = L.hsrans_encode_device_planes_diff_batch(ctx, m, None if null_arrays else _ptrs(bases), None if null_arrays else _sizes(base_bytes), 2,
                                                      work2.data_ptr(), 2 * r.wb, None, handles, None)
        made = [h for h in handles if h]
        for h in made:
            L.hsrans_dplan_destroy(h)
        return rc, all(m[k].frame_length == 0 and bytes(m[k].desc) == bytes(api.PlanesDesc()) for k in range(2)) and not made

    for d_base, base_bytes, why in _bad_bases(r)[1:]:  # (a NULL entry is a member without a base)
        assert call([r.base, d_base], [r.bytes, base_bytes]) == (E_ARG, True), why
        assert call([d_base, None], [base_bytes, 0]) == (E_ARG, True), why
    assert call([r.base, r.base], [r.bytes, r.bytes], null_arrays=True) == (E_ARG, True)
    assert call([frame1.data_ptr() + 256, None], [r.bytes, 0]) == (E_ARG, True)       # member 0's base inside its frame
    assert call([None, frame1.data_ptr() + 256], [0, r.bytes]) == (E_ARG, True)       # member 1's base inside member 0's frame
    assert call([work2.data_ptr() + 512, None], [r.bytes, 0]) == (E_ARG, True)        # a base inside the workspace
    assert r.untouched() and _untouched(frame1) and _untouched(frame2) and _untouched(work2)
    assert call([r.base, None], [r.bytes, 0]) == (0, False)                           # what was refused encodes


def _decode_diff(L, r, ctx, d_base, base_bytes, d_out=None, d_work=None, d_frame=None):
    return L.hsrans_decode_device_planes_diff(ctx, r.planes.handle, d_frame or r.good_frame.data_ptr(), r.good_frame.numel(), d_base, base_bytes,
                                              d_out or r.out.data_ptr(), r.bytes, d_work or r.work.data_ptr(), r.wb, None)


def test_the_decoders_refuse_a_bad_base(gpu_ctx, refusals):
    r, L, ctx = refusals, gpu_ctx.L, gpu_ctx.handle
    sh = r.shared.data_ptr()
    out = sh + 4096  # an output with room in front of it
    for d_base, base_bytes, why in _bad_bases(r, d_out=out):
        assert _decode_diff(L, r, ctx, d_base, base_bytes, d_out=out) == E_ARG, why
    assert _decode_diff(L, r, ctx, sh + 256, r.bytes, d_work=sh) == E_ARG                  # the base inside the workspace
    fr = r.good_frame.data_ptr()
    assert _decode_diff(L, r, ctx, fr + 256, r.bytes) == E_ARG                             # the base inside the frame (two reads, refused all the same)
    assert _decode_diff(L, r, ctx, fr, r.bytes) == E_ARG                                   # ... on its start
    assert _decode_diff(L, r, ctx, fr + r.good_frame.numel() - 16, r.bytes) == E_ARG       # ... on its last 16 bytes
    assert _decode_diff(L, r, ctx, sh, r.bytes + 4096, d_frame=sh + r.bytes + 256) == E_ARG  # ... meeting it only over base_bytes
    assert _decode_diff(L, r, ctx, out, r.bytes - 16, d_out=out) == E_ARG                  # in place, but the base is shorter than the tensor
    assert _decode_diff(L, r, None, r.base, r.bytes) == E_ARG
    assert _decode_diff(L, r, ctx, r.base, r.bytes, d_out=r.out.data_ptr() + 8) == E_ARG   # the plain call's refusals stay

    def batch_call(d_base, base_bytes, d_out, d_work=None, null_arrays=False):
        return L.hsrans_decode_device_planes_diff_batch(ctx, r.pset.handle, _ptrs([r.good_frame.data_ptr()]), _sizes([r.good_frame.numel()]),
                                                        None if null_arrays else _ptrs([d_base]), None if null_arrays else _sizes([base_bytes]), _ptrs([d_out]),
                                                        _sizes([r.bytes]), d_work or r.work.data_ptr(), r.wb, None)

    for d_base, base_bytes, why in _bad_bases(r, d_out=out)[1:]:
        assert batch_call(d_base, base_bytes, out) == E_ARG, why
    assert batch_call(r.base, r.bytes, out, null_arrays=True) == E_ARG
    assert batch_call(sh + 256, r.bytes, r.out.data_ptr(), d_work=sh) == E_ARG
    assert batch_call(fr + 256, r.bytes, r.out.data_ptr()) == E_ARG                         # the base inside the member's frame
    assert batch_call(fr + r.good_frame.numel() - 16, r.bytes, r.out.data_ptr()) == E_ARG
    assert batch_call(out, r.bytes - 16, out) == E_ARG
    assert r.untouched()
    # what was refused still decodes, apart and in place; a NULL entry of the batch's array is a member without a base
    want = r.a.view(np.uint8)
    good, own_work = _full(r.bytes), _full(r.wb)
    assert _decode_diff(L, r, ctx, r.base, r.bytes, d_out=good.data_ptr(), d_work=own_work.data_ptr()) == 0
    assert gpu_ctx.planes_status(r.planes) == [0] * 4 and np.array_equal(good.cpu().numpy(), want)
    own = r.base_buf[: r.bytes].clone()
    assert batch_call(own.data_ptr(), r.bytes, own.data_ptr(), d_work=own_work.data_ptr()) == 0
    assert gpu_ctx.planes_set_status(r.pset) == [0] and np.array_equal(own.cpu().numpy(), want)
    assert batch_call(None, 0, good.data_ptr(), d_work=own_work.data_ptr()) == 0
    assert gpu_ctx.planes_set_status(r.pset) == [0]
    assert np.array_equal(good.cpu().numpy(), zigzag(r.a, r.b).view(np.uint8))


def test_the_gather_refuses_a_bad_base_and_every_aliasing(gpu_ctx, refusals):
    r, L, ctx = refusals, gpu_ctx.L, gpu_ctx.handle
    ranges = np.array([[16, 1000, 0], [3, 50, 1000]], np.uint64)
    wb = H.planes_gather_workspace_bytes(4, 2, 1050)
    assert wb <= r.wb
    sh = r.shared.data_ptr()

    def call(d_base, base_bytes, d_out=None, d_work=None):
        return L.hsrans_decode_device_planes_gather_diff(ctx, r.pg.handle, ranges.ctypes.data, 2, d_base, base_bytes, d_out or r.out.data_ptr(), r.bytes,
                                                         d_work or r.work.data_ptr(), wb, None)

    for d_base, base_bytes, why in _bad_bases(r, d_out=sh + 4096):
        assert call(d_base, base_bytes, d_out=sh + 4096) == E_ARG, why
    assert call(sh, 2 * r.bytes, d_out=sh + r.bytes) == E_ARG      # the output inside the base
    assert call(sh, r.bytes, d_out=sh) == E_ARG                    # the output exactly on the base: the gather has no in-place form
    assert call(sh + 256, r.bytes, d_work=sh) == E_ARG             # the base inside the workspace
    fr = r.good_frame.data_ptr()
    assert call(fr + 256, r.bytes) == E_ARG                        # the base inside the frame the object is bound to
    assert call(fr, r.bytes) == E_ARG
    assert call(fr + r.good_frame.numel() - 16, r.bytes) == E_ARG
    assert call(r.base, 4 * 1050) == E_ARG                         # the ranges' elements are not enough: the base is the whole tensor
    assert r.untouched()
    out, own_work = _full(r.bytes), _full(wb)
    assert call(r.base, r.bytes, d_out=out.data_ptr(), d_work=own_work.data_ptr()) == 0
    assert gpu_ctx.planes_gather_status(r.pg) == [0] * 4
    want = np.full(r.bytes, SENTINEL, np.uint8)
    flat = r.a.view(np.uint8)
    want[: 4 * 1000] = flat[4 * 16: 4 * 1016]
    want[4 * 1000: 4 * 1050] = flat[4 * 3: 4 * 53]
    assert np.array_equal(out.cpu().numpy(), want)
