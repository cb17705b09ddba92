"""hsrans_decode_device_gather_batch's host side, without a GPU: the exported symbols, the ctypes mirrors of its structs, the refusal of null
arguments, and the pure function that cuts the ranges of many members into ONE kind's launch (hsrans_gather_batch_tasks) — against
hsrans_gather_tasks per range and per member, which is what the single call of each member runs."""
import ctypes

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

# (decoded_len, n_chains, states, interval, kind): kinds 0 and 2 keep a table per wave, 3 and 4 one per workgroup
MEMBERS = [
    (300_007, 147, 64, 32, 3),
    (300_007, 147, 64, 32, 0),
    (300_007, 293, 32, 32, 3),     # L = 4096: four checkpoint intervals of 32 x 32 bytes
    (1_000_003, 16, 64, 0, 4),     # no uniform interval: L from the mean chain length
    (300_007, 147, 64, 32, 2),
    (100_003, 1, 64, 0, 3),        # one chain
    (500_000, 245, 64, 32, 3),     # never asked for
]


def _ranges(seed, count=300, members=MEMBERS, skip=(6,)):
    rng = np.random.default_rng(seed)
    rows = []
    for _ in range(count):
        m = int(rng.choice([k for k in range(len(members)) if k not in skip]))
        n = members[m][0]
        length = min(int(2.0 ** rng.uniform(0, 16)), n) if rng.random() > 0.05 else 0
        off = int(rng.integers(0, n - length + 1))
        rows.append((m, off, length, int(rng.integers(0, 1 << 40))))
    return rows


def _single(member, rows):
    """H.gather_tasks of one member's ranges, in range order"""
    d, c, s, iv, _ = member
    return H.gather_tasks(d, c, s, iv, [(o, ln, dst) for _, o, ln, dst in rows])


def test_symbols_and_struct_sizes():
    L = H.load_library()
    for name in ("hsrans_gather_set_create", "hsrans_gather_set_destroy", "hsrans_decode_device_gather_batch", "hsrans_gather_set_status", "hsrans_gather_set_info",
                 "hsrans_gather_batch_tasks"):
        assert hasattr(L, name), name
    assert ctypes.sizeof(api.MemberRange) == 32 and ctypes.sizeof(api.GatherBatchTask) == 32 and ctypes.sizeof(api.GatherMember) == 24


def test_null_arguments_are_refused_without_a_device():
    L = H.load_library()
    out = ctypes.c_void_p(0x1234)
    one = (ctypes.c_void_p * 1)(None)
    length = (ctypes.c_size_t * 1)(16)
    assert L.hsrans_gather_set_create(None, one, one, length, 1, ctypes.byref(out)) == 2 and out.value is None
    assert L.hsrans_gather_set_create(None, None, None, None, 1, None) == 2
    r = (api.MemberRange * 1)(api.MemberRange(0, 1, 0, 0, 0))
    assert L.hsrans_decode_device_gather_batch(None, None, r, 1, None, 0, None) == 2
    assert L.hsrans_gather_set_status(None, None, None, None) == 2
    assert L.hsrans_gather_set_info(None, None) == 2
    L.hsrans_gather_set_destroy(None)


@pytest.mark.parametrize("kind", (0, 2))
@pytest.mark.parametrize("waves", (1, 4))
def test_private_kinds_are_the_single_cut_per_range(kind, waves):
    rows = _ranges(kind)
    got = H.gather_batch_tasks(MEMBERS, rows, kind, waves)
    want = []
    for row in rows:
        if MEMBERS[row[0]][4] == kind:
            want += [(b, e, d, row[0]) for b, e, d in _single(MEMBERS[row[0]], [row]).tolist()]
    assert len(want) > 20
    assert got.tolist() == [list(w) for w in want]


@pytest.mark.parametrize("kind", (3, 4))
@pytest.mark.parametrize("waves", (1, 4, 16))
def test_shared_kinds_are_sorted_by_member_and_padded(kind, waves):
    rows = _ranges(10 + kind)
    got = H.gather_batch_tasks(MEMBERS, rows, kind, waves)
    assert got.shape[0] > 0 and got.shape[0] % waves == 0
    members = got[:, 3].astype(np.int64)
    assert np.all(members.reshape(-1, waves) == members.reshape(-1, waves)[:, :1])  # every run of `waves` entries has one member
    assert np.all(np.diff(members) >= 0)                                             # sorted by member
    padding = (got[:, 0] == 0) & (got[:, 1] == 0)
    assert np.all(got[padding, 2] == 0)
    present = sorted(set(members.tolist()))
    assert present == sorted({r[0] for r in rows if MEMBERS[r[0]][4] == kind and r[2] > 0})  # a member without ranges (6) or of another kind: no entry
    assert 6 not in present
    for m in present:
        mine = got[(members == m) & ~padding]
        want = _single(MEMBERS[m], [r for r in rows if r[0] == m])   # stable: the member's ranges in range order
        assert np.array_equal(mine[:, :3], want), m
        assert int(padding[members == m].sum()) == (-want.shape[0]) % waves < waves
        run = got[members == m]
        assert not ((run[:, 0] == 0) & (run[:, 1] == 0))[:want.shape[0]].any()  # the padding stands behind the member's tasks
    if waves == 1:
        assert not padding.any()


def test_every_kind_of_one_call_together_holds_every_task_once():
    rows = _ranges(99)
    total = sum(_single(MEMBERS[r[0]], [r]).shape[0] for r in rows)
    seen = 0
    for kind in range(6):
        got = H.gather_batch_tasks(MEMBERS, rows, kind, 4)
        seen += int(((got[:, 0] != 0) | (got[:, 1] != 0)).sum())
        if kind in (1, 5):
            assert got.shape[0] == 0  # no member of that kind
    assert seen == total


def test_members_cut_at_their_own_segment_length():
    """a checkpoint every 32 groups is 1 KiB at 32 states and 2 KiB at 64: both are raised to the 4 KiB floor, in four and in two intervals;
    a checkpoint every 128 groups at 64 states cuts at 8 KiB — three members of one kind, each cut as its single call cuts it"""
    members = [(300_007, 293, 32, 32, 3), (300_007, 37, 64, 128, 3), (300_007, 147, 64, 32, 3)]
    assert [H.gather_segment(*m[:4]) for m in members] == [4096, 8192, 4096]
    rows = [(0, 1000, 20_000, 0), (1, 1000, 20_000, 50_000), (2, 1000, 20_000, 100_000)]
    got = H.gather_batch_tasks(members, rows, 3, 1)
    for m in range(3):
        mine = got[got[:, 3] == m]
        assert np.array_equal(mine[:, :3], _single(members[m], [rows[m]]))
        L = H.gather_segment(*members[m][:4])
        assert all(int(b) // L == (int(e) - 1) // L for b, e in mine[:, :2].tolist())
    assert (got[:, 3] == 0).sum() == 6 and (got[:, 3] == 1).sum() == 3 and (got[:, 3] == 2).sum() == 6


def test_capacity_protocol():
    L = H.load_library()
    rows = _ranges(5, count=60)
    for kind, waves in ((0, 4), (3, 4)):
        full = H.gather_batch_tasks(MEMBERS, rows, kind, waves)
        n = full.shape[0]
        assert n > 8
        assert np.array_equal(H.gather_batch_tasks(MEMBERS, rows, kind, waves, capacity=5), full[:5])
        mem = (api.GatherMember * len(MEMBERS))(*[api.GatherMember(*m) for m in MEMBERS])
        rr = (api.MemberRange * len(rows))(*[api.MemberRange(o, ln, d, m, 0) for m, o, ln, d in rows])
        short = np.full((n, 4), 0xCCCCCCCCCCCCCCCC, np.uint64)  # 32-byte rows
        assert L.hsrans_gather_batch_tasks(mem, len(MEMBERS), rr, len(rows), kind, waves, short.ctypes.data, 3) == n  # still the need
        assert np.array_equal(short[:3, :3], full[:3, :3]) and np.all(short[3:] == 0xCCCCCCCCCCCCCCCC)                # and not overrun
        assert L.hsrans_gather_batch_tasks(mem, len(MEMBERS), rr, len(rows), kind, waves, None, 0) == n


def test_refusals():
    ok = [(0, 0, 100, 0), (1, 5, 100, 200)]
    assert H.gather_batch_tasks(MEMBERS, ok, 3, 4).shape[0] == 4 and H.gather_batch_tasks(MEMBERS, ok, 0, 4).shape[0] == 1
    for kind in (0, 3):
        assert H.gather_batch_tasks(MEMBERS, ok + [(len(MEMBERS), 0, 1, 0)], kind, 4).shape[0] == 0        # member == n_members
        assert H.gather_batch_tasks(MEMBERS, ok + [(0, 300_007 - 9, 10, 0)], kind, 4).shape[0] == 0        # one byte beyond decoded_len
        assert H.gather_batch_tasks(MEMBERS, ok + [(1, 300_008, 0, 0)], kind, 4).shape[0] == 0
        assert H.gather_batch_tasks(MEMBERS, ok + [(0, 8, (1 << 64) - 4, 0)], kind, 4).shape[0] == 0       # offset + length wraps
        assert H.gather_batch_tasks(MEMBERS, ok, kind, 0).shape[0] == 0                                    # waves == 0
    assert H.gather_batch_tasks(MEMBERS, ok, 6, 4).shape[0] == 0                                           # no such kind
    assert H.gather_batch_tasks(MEMBERS, ok + [(0, 300_007 - 10, 10, 0)], 3, 4).shape[0] == 4              # ending at decoded_len is fine
    assert H.gather_batch_tasks(MEMBERS, [], 3, 4).shape[0] == 0
    L = H.load_library()
    mem = (api.GatherMember * 1)(api.GatherMember(1000, 4, 64, 0, 0))
    assert L.hsrans_gather_batch_tasks(mem, 1, None, 1, 0, 4, None, 0) == 0                                # null ranges, count > 0
