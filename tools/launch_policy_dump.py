#!/usr/bin/env python3
"""Print what the decode launch policy (csrc/hsrans_launch.cpp) answers over a fixed grid of inputs:  launch_policy_dump.py > OUT

No GPU: every call goes through a library entry that takes ctx = NULL (the MI355X defaults, 256 CUs and 160 KiB of LDS) —
hsrans_launch_choice, hsrans_index_boundaries, hsrans_index_boundaries_batch, hsrans_dealt_shares, hsrans_batch_deal.  Run it on two builds
and compare the outputs byte for byte (cmp): a refactor of the policy must leave them identical.  (The gather and batch launch shapes have no
entry that works without a device: tests/test_launch_policy.py sweeps them in a stand-alone program.)

The grid:
  * the plan kinds and fact sets of tests/test_launch_choice.py;
  * raw plans of 8..15 bits, 32 / 64 states, 1, 2, 63, 4096, 47104 and 2^20 chains, index intervals 0 / 8 / 32; the same chain counts as lean
    grouped plans and as plans whose waves build their own tables;
  * the indexes of hsrans_index_boundaries[_batch], the dealing of hsrans_dealt_shares at 11 / 13 / 14 bits, hsrans_batch_deal;
  * the named class lists of tests/test_geometry_domain.py under every HSRANS_*_WEIGHTS knob, with HSRANS_WAVES_PER_WG 4 / 8 / 16.
Arrays are printed as length, SHA-1 and their first and last values."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import hypersonic_rans_amd as H  # noqa: E402
from hypersonic_rans_amd import api  # noqa: E402

BITS = range(8, 16)
STATES = (32, 64)
CHAINS = (1, 2, 63, 4096, 47104, 1 << 20)
INTERVALS = (0, 8, 32)
NAMED = {"flat": (1000,) * 8, "steep": (3000, 2000, 1000, 500, 500, 400, 300, 300), "reversed": (300, 300, 400, 500, 500, 1000, 2000, 3000),
         "edge": (100, 100, 100, 3000, 100, 100, 1500, 3000)}
KNOBS = ("SLOT_WEIGHTS", "SLOT_WEIGHTS4", "DIRECT_WEIGHTS", "DIRECT_WEIGHTS4", "DIRECT_WEIGHTS6", "DIRECT_WEIGHTS3", "DIRECT_WEIGHTS_PAIR", "DUAL_WEIGHTS",
         "DUAL_WEIGHTS_WIDE", "DEALT_WEIGHTS", "BATCH_WEIGHTS")
MERGEABLE_WITH_HIST = 2 | 4
WALK = 1


def arr(a):
    a = np.ascontiguousarray(a)
    ends = list(a.reshape(-1)[:4]) + list(a.reshape(-1)[-4:])
    return "n=%d sha1=%s ends=%s" % (a.size, hashlib.sha1(a.tobytes()).hexdigest(), [int(x) for x in ends])


def choice(what, plan, **facts):
    try:
        name, info = api.launch_choice(plan, **facts)
        print(what, "->", name, " ".join("%s=%s" % (k, info[k]) for k in sorted(info)))
    except (NotImplementedError, ValueError, H.HsransError) as e:
        print(what, "->", type(e).__name__)


def raw(states, bits, n_chains, interval=0, decoded_len=100_000_000):
    return dict(container=H.RAW, states=states, bits=bits, flags=MERGEABLE_WITH_HIST, decoded_len=decoded_len, n_chains=n_chains, n_pieces=n_chains, shared_hist=1,
                interval=interval)


def raw_facts(states, bits, interval):
    if interval == 0:
        return dict(persistent=1, table_mode=4 if states == 64 and bits >= 14 else 3, dual=int(states == 64 and bits >= 13))
    return dict(persistent=1, table_mode=4 if bits == 15 else 3)


def blocks(bits, size, block, interval, container=H.MT, states=64):
    lengths = [min(block, size - lo) for lo in range(0, size, block)]
    begin = np.concatenate([[0], np.cumsum([-(-n // (interval * states)) for n in lengths])]).astype(np.uint32)
    n = int(begin[-1])
    return dict(container=container, states=states, bits=bits, flags=0, decoded_len=size, n_chains=n, n_pieces=n, interval=interval), begin


def lean(plan, block_begin, groups_per_block, *, coded_blocks_only=True, **more):
    dealt = coded_blocks_only and api.dealt_shares(block_begin, plan["decoded_len"] // 64, bits=plan["bits"])[0]
    fewest = int(np.diff(block_begin)[:-1].min()) if block_begin.size > 2 else 0
    return dict(n_groups=(len(block_begin) - 1) * groups_per_block, groups_lean=1, spread_min_block=fewest, tickets=1, dealt=int(dealt), **more)


def dealing(what, begin, total_groups, bits):
    try:
        ok, share, split = api.dealt_shares(begin, total_groups, bits=bits)
        print(what, "-> ok=%d begin %s split %s" % (ok, arr(share), arr(split)))
    except H.HsransError as e:
        print(what, "->", type(e).__name__)


def kernel_table_rows():
    few, many = blocks(11, 24_000_000, 1 << 18, 8), blocks(11, 1 << 30, 1 << 18, 16)
    choice("row direct 11", raw(64, 11, 8192), persistent=1, table_mode=3)
    choice("row dual 13", raw(64, 13, 8192), persistent=1, table_mode=3, dual=1)
    choice("row dual 14", raw(64, 14, 8192), persistent=1, table_mode=4, dual=1)
    choice("row persist", raw(64, 11, 24415, interval=64), persistent=1, table_mode=3)
    choice("row grouped many", many[0], **lean(*many, 1))
    choice("row dealt", few[0], **lean(*few, 8))
    choice("row spread", few[0], **lean(*few, 8, coded_blocks_only=False))
    choice("row single", dict(container=H.RAW, states=64, bits=11, decoded_len=1 << 20, n_chains=1, n_pieces=1, shared_hist=1), single_valid=1, single_ring_entries=2048)
    choice("row walk", dict(container=H.BLOCK, states=64, bits=11, flags=WALK, decoded_len=1 << 20, n_chains=1, n_pieces=1))
    for bits in (12, 13, 14):
        plan, begin = blocks(bits, 24_000_000, 1 << 18, 8)
        choice("row dealt forced %d" % bits, plan, **dict(lean(plan, begin, 8), dealt=1))
    for coded in (True, False):
        choice("row index pass coded=%d" % coded, dict(few[0], shared_hist=0), **dict(lean(*few, 8, coded_blocks_only=coded, index_pass=1), dealt=1))
    choice("row single index pass", dict(container=H.RAW, states=64, bits=11, decoded_len=1 << 20, n_chains=1, n_pieces=1), single_valid=1, single_ring_entries=2048, index_pass=1)
    for (plan, begin), per_block, coded in ((few, 8, True), (few, 8, False), (many, 1, True), (blocks(13, 1 << 30, 1 << 18, 16), 1, True)):
        for n_parts in (0, 1, 4, 16, 17):
            choice("row parts %d bits %d coded=%d n=%d" % (per_block, plan["bits"], coded, n_parts), plan, **lean(plan, begin, per_block, coded_blocks_only=coded, parts=1, n_parts=n_parts))
    choice("row parts not lean", few[0], **dict(lean(*few, 8, parts=1, n_parts=4), groups_lean=0, spread_min_block=0, dealt=0))
    choice("row parts raw", raw(64, 11, 8192), persistent=1, table_mode=3, parts=1, n_parts=4)
    choice("row parts mt", dict(few[0], n_chains=92, n_pieces=92, interval=0), parts=1, n_parts=2)
    choice("row bad states", dict(container=H.RAW, states=48, bits=11, n_chains=1, n_pieces=1))


def the_grid(tag):
    for states in STATES:
        for bits in BITS:
            for n in CHAINS:
                for interval in INTERVALS:
                    size = max(n, 1) * states * (interval if interval else 32)
                    choice("%s raw S=%d b=%d n=%d G=%d" % (tag, states, bits, n, interval), raw(states, bits, n, interval, size), **raw_facts(states, bits, interval))
                    choice("%s calib S=%d b=%d n=%d G=%d" % (tag, states, bits, n, interval), raw(states, bits, n, interval, size), calibrating=1, **raw_facts(states, bits, interval))
                # waves build their own tables: mt_ without an index, and as an index pass
                own = dict(container=H.MT, states=states, bits=bits, flags=0, decoded_len=n * 65536, n_chains=n, n_pieces=n)
                choice("%s own S=%d b=%d n=%d" % (tag, states, bits, n), own)
                choice("%s own pass S=%d b=%d n=%d" % (tag, states, bits, n), own, index_pass=1)
                # grouped: n chains in groups of up to 512
                for interval in INTERVALS[1:]:
                    groups = max(1, n // 512)
                    plan = dict(container=H.MT, states=states, bits=bits, flags=0, decoded_len=n * states * interval, n_chains=n, n_pieces=n, interval=interval)
                    for lean_ in (0, 1):
                        for tickets in (0, 1):
                            choice("%s grouped S=%d b=%d n=%d G=%d lean=%d t=%d" % (tag, states, bits, n, interval, lean_, tickets), plan, n_groups=groups, groups_lean=lean_,
                                   tickets=tickets, spread_min_block=min(n, 512) if lean_ else 0)
                    begin = np.minimum(np.arange(groups + 1, dtype=np.uint64) * 512, n).astype(np.uint32)
                    begin[-1] = n
                    for b in (11, 13, 14) if bits == 11 and states == 64 else ():
                        dealing("%s deal b=%d n=%d G=%d" % (tag, b, n, interval), begin, n * interval, b)
                        choice("%s dealt b=%d n=%d G=%d" % (tag, b, n, interval), dict(plan, bits=b), n_groups=groups, groups_lean=1, tickets=1, spread_min_block=min(n, 512), dealt=1)
            for bits in BITS:
                for size in (64, 4096, 3_000_000, 12_000_000, 100_000_000, 1 << 30):
                    print("%s index S=%d b=%d size=%d ->" % (tag, states, bits, size), arr(H.index_boundaries(states, bits, size)))
                for sizes in ([3_000_000] * 4, [3_000_000, 2_000_000, 3_000_000, 1_000_003], [100_000_000], [4096, 0, 1 << 26]):
                    for member in range(len(sizes)):
                        print("%s batch index S=%d b=%d sizes=%s m=%d ->" % (tag, states, bits, sizes, member), arr(api.index_boundaries_batch(states, bits, sizes, member)))


def dealings(tag):
    for bits in (11, 13, 14):
        for size, block, interval in ((24_000_000, 1 << 18, 8), (3_000_000, 1 << 16, 4), (1 << 30, 1 << 18, 16), (100_000_000, 1 << 20, 32), (128 << 20, 1 << 18, 8), (6_000_000, 1 << 17, 4)):
            plan, begin = blocks(bits, size, block, interval)
            dealing("%s deal b=%d size=%d block=%d G=%d" % (tag, bits, size, block, interval), begin, size // 64, bits)
        for n_blocks in (1, 2, 92, 1023):
            begin = (np.arange(n_blocks + 1, dtype=np.uint64) * 47104 // n_blocks).astype(np.uint32)
            dealing("%s deal b=%d blocks=%d of 47104" % (tag, bits, n_blocks), begin, 47104 * 8, bits)


def batch_deals(tag):
    rng = np.random.default_rng(7)
    uniform = [np.arange(0, 46875 + 1, 16, dtype=np.uint64) for _ in range(4)]
    ragged = [np.concatenate([[0], np.cumsum(rng.integers(4, 200, n))]).astype(np.uint64) for n in (100, 3000, 8192, 1)]
    own = [np.concatenate([[0], H.index_boundaries(64, 11, 12_000_000).astype(np.uint64), [12_000_000 // 64]]) for _ in range(2)]
    for what, starts in (("uniform", uniform), ("ragged", ragged), ("own index", own)):
        for grid, waves in ((512, 16), (256, 16), (1024, 8), (511, 16), (2, 4)):
            for name, ws in [("default", None)] + list(NAMED.items()):
                try:
                    imb, slots = api.batch_deal(starts, grid, waves, ws)
                    print("%s batch deal %s %dx%d %s -> imbalance %r slots %s" % (tag, what, grid, waves, name, imb, arr(slots)))
                except H.HsransError as e:
                    print("%s batch deal %s %dx%d %s -> %s" % (tag, what, grid, waves, name, type(e).__name__))


def main():
    kernel_table_rows()
    the_grid("default")
    dealings("default")
    batch_deals("default")
    for waves in (4, 8, 16):
        os.environ["HSRANS_WAVES_PER_WG"] = str(waves)
        for knob in KNOBS:
            for name, ws in NAMED.items():
                os.environ["HSRANS_" + knob] = ",".join(str(w) for w in ws)
                tag = "W=%d %s=%s" % (waves, knob, name)
                kernel_table_rows_under(tag)
                del os.environ["HSRANS_" + knob]
        del os.environ["HSRANS_WAVES_PER_WG"]


def kernel_table_rows_under(tag):
    """a thinner grid for the knobs: every launch kind once per table width, the two indexes, the dealing"""
    for states, bits in ((64, 11), (64, 12), (64, 13), (64, 14), (64, 15), (32, 11)):
        for n in (63, 1463, 8192, 47104):
            choice("%s direct S=%d b=%d n=%d" % (tag, states, bits, n), raw(states, bits, n, 0, 3_000_003), **raw_facts(states, bits, 0))
        for interval in (4, 32):
            n = -(-(3_000_003 // states) // interval)
            choice("%s persist S=%d b=%d G=%d" % (tag, states, bits, interval), raw(states, bits, n, interval, 3_000_003), **raw_facts(states, bits, interval))
        print("%s index S=%d b=%d ->" % (tag, states, bits), arr(H.index_boundaries(states, bits, 12_000_000)), arr(H.index_boundaries(states, bits, 3_000_000)))
        sizes = [3_000_000, 2_000_000, 3_000_000, 1_000_003]
        print("%s batch index S=%d b=%d ->" % (tag, states, bits), " ".join(arr(api.index_boundaries_batch(states, bits, sizes, m)) for m in range(4)))
    for bits, size, block, interval in ((11, 9_000_000, 1 << 13, 4), (11, 3_000_000, 1 << 16, 4), (11, 6_000_000, 1 << 17, 4), (15, 6_000_000, 1 << 17, 4), (13, 3_000_000, 1 << 16, 4),
                                        (14, 3_000_000, 1 << 16, 4)):
        plan, begin = blocks(bits, size, block, interval)
        choice("%s grouped b=%d size=%d" % (tag, bits, size), plan, n_groups=len(begin) - 1, groups_lean=1, tickets=1)
        choice("%s spread b=%d size=%d" % (tag, bits, size), plan, n_groups=len(begin) - 1, groups_lean=1, tickets=1, spread_min_block=int(np.diff(begin)[:-1].min()))
        if bits in (11, 13, 14):
            dealing("%s deal b=%d size=%d" % (tag, bits, size), begin, size // 64, bits)
            choice("%s dealt b=%d size=%d" % (tag, bits, size), plan, n_groups=len(begin) - 1, groups_lean=1, tickets=1, spread_min_block=int(np.diff(begin)[:-1].min()), dealt=1)


if __name__ == "__main__":
    main()
