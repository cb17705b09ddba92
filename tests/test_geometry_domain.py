"""Every share rule of the decode launches, at class lengths and workgroup shapes off the defaults: pure host arithmetic, no GPU.

A launch is shaped by numbers that differ from machine to machine: the eight per-mille class lengths (nine HSRANS_*_WEIGHTS lists,
HSRANS_DEALT_WEIGHTS, HSRANS_BATCH_WEIGHTS), the waves per workgroup, the dealt launch's gap.  They decide which wave decodes which chains and
nothing else, so whatever they are the waves' chain ranges must cut [0, n_chains) into disjoint, ascending pieces.  This file holds a plain
Python model of each rule, written from the comments of csrc/hsrans_kernels.h, hsrans_kernels.hip and the kernels' headers — never by asking
the library for the answer — and feeds it what hsrans_launch_choice reports (grid, waves_per_block, class_weights) under the knobs.

THE DOMAIN of a list of class lengths (csrc/hsrans_tuning.h): eight values, every one of them 100 .. 3000 as written — the bounds
tests/test_gpu_calibrate.py holds hsrans_ctx_calibrate's fits to.  read_tuning ignores any other list as a whole.  Two lists that read_tuning took as they stood before:
  HSRANS_SLOT_WEIGHTS=3000,3000,1000,1000,0,0,0,0  is rejected for its zero half: the cumulative table of the grid's second half ends in 0,
      so k_decode_grouped's weighted split (count * cum[k] / cum[waves], the divisor 0 taken as 1) gives every wave of those workgroups the
      share [0, 0) and their blocks are never decoded; k_decode_dealt divides by that entry.  (test_a_zero_half_loses_a_blocks_chains shows
      it on the model.)
  HSRANS_DEALT_WEIGHTS=60000 x 8  is rejected for its size: 16 waves x 6000 wrap the table's uint16_t entries, the table is no longer
      non-decreasing and the kernel's wave shares are not the ones the host dealt.  (test_unbounded_lengths_wrap_the_table)
A zero CLASS beside live ones is safe in every kernel (an empty share skips its run: `first >= last` in kernels_grouped.h, `while (i < last)`
in kernels_spread.h, `have` in kernels_dealt.h, a run_len of 0 in kernels_persist.h), but lies outside the domain all the same."""
import os

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

LO, HI = 100, 3000
CLASS_LISTS = ("SLOT_WEIGHTS", "SLOT_WEIGHTS4", "DIRECT_WEIGHTS", "DIRECT_WEIGHTS4", "DIRECT_WEIGHTS6", "DIRECT_WEIGHTS3", "DIRECT_WEIGHTS_PAIR", "DUAL_WEIGHTS",
               "DUAL_WEIGHTS_WIDE")
FLAT = (1000,) * 8
STEEP = (3000, 2000, 1000, 500, 500, 400, 300, 300)
REVERSED = STEEP[::-1]
EDGE = (100, 100, 100, 3000, 100, 100, 1500, 3000)
NAMED = {"flat": FLAT, "steep": STEEP, "reversed": REVERSED, "edge": EDGE}
ZERO_HALF = (3000, 3000, 1000, 1000, 0, 0, 0, 0)
HUGE = (60000,) * 8
SPREAD_MAX_SHARE, DEALT_GRID, NO_SPLIT = 127, 512, 0xFFFF
CUS = 256  # the default geometry (ctx = NULL): an MI355X

text = lambda ws: ",".join(str(w) for w in ws)
in_domain = lambda ws: len(ws) >= 8 and all(LO <= w <= HI for w in ws[:8])
rescaled = lambda ws: [w * 8000 // sum(ws[:8]) for w in ws[:8]]


def random_lists(count, seed=2026):
    """lists inside the domain: half of them as any eight values of 100 .. 3000, half of them cut to a sum of 8000 like the calibrator's"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        ws = [int(w) for w in rng.integers(LO, HI + 1, 8)]
        if len(out) % 2:
            ws = [max(LO, min(HI, w * 8000 // sum(ws))) for w in ws]
        out.append(tuple(ws))
    return out


# ---- the model ----
def per_class_of(waves):
    return waves // 4 if waves >= 4 else 1


def cum_table(weights, waves):
    """[half of the grid][wave]: w / 10 per wave of class wave / (waves / 4) (the fourth class takes what is left), 17 entries, flat behind `waves`"""
    pc = per_class_of(waves)
    out = np.zeros((2, 17), np.int64)
    for hf in range(2):
        for k in range(16):
            out[hf][k + 1] = out[hf][k] + (weights[hf * 4 + min(3, k // pc)] // 10 if k < waves else 0)
    return out


def assert_table(cum, waves, what):
    for hf in range(2):
        assert (np.diff(cum[hf]) >= 0).all(), (what, "a cumulative table falls", cum[hf])
        assert 1 <= cum[hf][waves] <= 0xFFFF and cum[hf][16] == cum[hf][waves], (what, "last entry", cum[hf])


def assert_partition(first, last, lo, hi, what):
    """ranges in wave order: each begins where the one before ended, the first at lo, the last ends at hi"""
    first, last = np.asarray(first, np.int64), np.asarray(last, np.int64)
    assert first.size and first[0] == lo and last[-1] == hi, (what, int(first[0]), int(last[-1]), lo, hi)
    assert (last >= first).all() and (first[1:] == last[:-1]).all(), (what, "ranges overlap or leave a gap")


def static_shares(n_chains, states, grid, waves, weights):
    """PersistentArgs' static shares: run_len[class] = n_chains * w / (1000 * W * runs per wave) whole chains"""
    W, runs, pc = grid * waves, 2 if states == 32 else 1, per_class_of(waves)
    classes, fh = waves // pc, (grid + 1) // 2
    run_len, class_off, wg = [0] * 8, [0] * 8, [0, 0]
    for hf in range(2):
        off = 0
        for k in range(4):
            run_len[hf * 4 + k] = n_chains * weights[hf * 4 + k] // (1000 * W * runs) if k < classes else 0
            class_off[hf * 4 + k] = off
            off += run_len[hf * 4 + k] * pc * runs
        wg[hf] = off
    return dict(run_len=run_len, class_off=class_off, wg_chains=wg, half_base=[0, fh * wg[0]], static_total=fh * wg[0] + (grid - fh) * wg[1], runs=runs)


def static_ranges(st, grid, waves):
    """run_persistent[_pair]: wave w of workgroup blk starts at half_base + workgroups before it in its half + its class's offset + the waves of
    its class before it"""
    pc, fh = per_class_of(waves), (grid + 1) // 2
    w = np.arange(grid * waves)
    blk, wv = w // waves, w % waves
    half = (blk >= fh).astype(np.int64)
    cls = half * 4 + wv // pc
    q0 = np.array(st["run_len"])[cls] * st["runs"]
    first = np.array(st["half_base"])[half] + (blk - half * fh) * np.array(st["wg_chains"])[half] + np.array(st["class_off"])[cls] + (wv % pc) * q0
    return first, first + q0


def spread_share_begin(n_chains, b, grid, w1, w2):
    fh = (grid + 1) // 2
    b = np.asarray(b, np.int64)
    cum = np.where(b <= fh, b * w1, fh * w1 + (b - fh) * w2)
    return n_chains * cum // (fh * w1 + (grid - fh) * w2)


def wave_split(count, cum_half, waves, weighted=True):
    """a workgroup's `count` chains over its waves: count * cum[k] / cum[waves], or evenly"""
    k = np.arange(waves + 1)
    return count * cum_half[:waves + 1] // cum_half[waves] if weighted else count * k // waves


def dealt_wave_split(count, split, gap, cum_half):
    """run_dealt: the split is made over count + gap virtual positions (the gap stands for the second prologue of the wave that straddles the
    share's block boundary) and mapped back"""
    two = split < count
    g = gap if two else 0
    v = cum_half[:17] * (count + g) // cum_half[16]
    s = min(split, count)
    return np.where(v < s, v, np.where(v < s + g, s, v - g))


def boundaries(units, weights_of_chain):
    """cut `units` units of 4 groups at units * cum / all; every chain at least one unit; stop at the total"""
    wt = np.asarray(weights_of_chain, np.int64)
    k = np.arange(wt.size - 1)
    b = units * np.cumsum(wt)[:-1] // int(wt.sum())
    b = np.maximum.accumulate(np.concatenate([[1], b - k]))[1:] + k  # b[k] = max(b[k], b[k - 1] + 1), b[-1] = 0
    return b[b < units] * 4


def direct_boundaries(states, total_groups, info):
    """one chain per wave slot of the launch `info` describes (two at 32 states and in the two-chain launch), at most one per 32 groups"""
    grid, waves = info["grid"], info["waves_per_block"]
    rpw = 2 if states == 32 or info["chains_per_wave"] == 2 else 1
    units = total_groups // 4
    chains = min(grid * waves * rpw, units // 8 or 1)
    if chains <= 1:
        return np.zeros(0, np.int64)
    w = np.arange(chains) // rpw
    cls = (w // waves >= (grid + 1) // 2) * 4 + np.minimum(w % waves // per_class_of(waves), 3)
    return boundaries(units, np.array(info["class_weights"])[cls])


def batch_apportion(totals, pairs):
    n = [1 if t and k < pairs else 0 for k, t in enumerate(totals)]
    for _ in range(pairs - sum(n)):
        best = max((m for m in range(len(n)) if n[m]), key=lambda m: (totals[m] / n[m], -m), default=None)
        if best is None:
            break
        n[best] += 1
    return n


def batch_boundaries(totals, member, grid, waves, weights, per_slot=1):
    n = batch_apportion(totals, grid - (grid + 1) // 2)[member]
    units = totals[member] // 4
    chains = min(n * 2 * waves * per_slot, units // 8 or 1)
    if chains <= 1:
        return np.zeros(0, np.int64)
    slot = np.arange(chains) // per_slot
    cls = (slot // waves >= n) * 4 + np.minimum(slot % waves // per_class_of(waves), 3)
    return boundaries(units, np.array(weights)[cls])


# ---- the kinds (the shapes of tests/test_gpu_geometry.py, as plan headers) ----
def raw(states, bits, n_chains, interval=0, n=3_000_003):
    return dict(container=H.RAW, states=states, bits=bits, flags=2 | 4, decoded_len=n, n_chains=n_chains, n_pieces=n_chains, shared_hist=1, interval=interval)


def persist_kind(states, bits, interval, n=3_000_003):
    return raw(states, bits, -(-(n // states) // interval), interval, n), dict(persistent=1, table_mode=4 if bits == 15 else 3)


def direct_facts(states, bits):
    return dict(persistent=1, table_mode=4 if states == 64 and bits >= 14 else 3, dual=int(states == 64 and bits >= 13))


def blocks(bits, size, block, interval, states=64):
    lengths = [min(block, size - lo) for lo in range(0, size, block)]
    begin = np.concatenate([[0], np.cumsum([-(-n // (interval * states)) for n in lengths])]).astype(np.uint32)
    n = int(begin[-1])
    return dict(container=H.MT, states=states, bits=bits, flags=0, decoded_len=size, n_chains=n, n_pieces=n, interval=interval), begin


PERSIST = [(64, 11, 32), (64, 11, 4), (64, 15, 32), (64, 15, 4), (32, 11, 32), (32, 11, 4)]
DIRECT = [(64, 11), (64, 12), (64, 13), (64, 14), (64, 15), (32, 11)]
DIRECT_SIZES = (12_000_000, 3_000_000)
GROUPED = [blocks(11, 9_000_000, 1 << 13, 4), blocks(11, 3_000_000, 1 << 16, 4), blocks(11, 6_000_000, 1 << 17, 4), blocks(15, 6_000_000, 1 << 17, 4)]
DEALT = blocks(11, 3_000_000, 1 << 16, 4)  # 11,719 chains in 46 blocks
WAVES = (4, 8, 12, 16)


def set_lists(monkeypatch, ws, waves=None):
    for name in CLASS_LISTS + ("DEALT_WEIGHTS", "BATCH_WEIGHTS"):
        monkeypatch.setenv("HSRANS_" + name, text(ws))
    if waves is not None:
        monkeypatch.setenv("HSRANS_WAVES_PER_WG", str(waves))


def check_every_rule(ws, waves, what, boundaries_too=True):
    """the properties, for the environment as it is set now"""
    # 1. uniform-interval launches: the static runs cut [0, static_total), static_total <= n_chains
    for case in PERSIST:
        plan, facts = persist_kind(*case)
        name, info = api.launch_choice(plan, **facts)
        assert "k_decode_persist" in name, (what, case, name)
        st = static_shares(plan["n_chains"], case[0], info["grid"], info["waves_per_block"], info["class_weights"])
        assert 0 <= st["static_total"] <= plan["n_chains"], (what, case, st)
        assert_partition(*static_ranges(st, info["grid"], info["waves_per_block"]), 0, st["static_total"], (what, case))
    # 2. one chain per wave: the index is ascending, every chain a unit of 4 groups at least, the last boundary below the total; the waves' runs
    # of its chains cut [0, n_chains)
    for states, bits in DIRECT if boundaries_too else ():
        for size in DIRECT_SIZES:
            groups = H.index_boundaries(states, bits, size)
            total = size // states
            _, info = api.launch_choice(raw(states, bits, 1 << 30, n=size), **direct_facts(states, bits))
            assert np.array_equal(groups, direct_boundaries(states, total, info)), (what, states, bits, size, "the index is not the model's")
            assert groups.size and groups[0] >= 4 and (np.diff(groups.astype(np.int64)) >= 4).all() and (groups % 4 == 0).all() and groups[-1] < total // 4 * 4, (what, states, bits, size)
            n = groups.size + 1
            _, info = api.launch_choice(raw(states, bits, n, n=size), **direct_facts(states, bits))
            W = info["grid"] * info["waves_per_block"]
            if states == 64 and info["chains_per_wave"] == 1:
                R = -(-n // W)
                w = np.arange(W)
                assert_partition(np.minimum(w * R, n), np.minimum(w * R + R, n), 0, n, (what, states, bits, size))
            else:
                assert n <= 2 * W, (what, states, bits, size, n, W)
    # 3. grouped: the table of the launch's own waves, and the wave split of a block of any size (weighted from 8 chains a wave on)
    for plan, begin in GROUPED:
        name, info = api.launch_choice(plan, n_groups=len(begin) - 1, groups_lean=1, tickets=1)
        assert "k_decode_grouped" in name and info["spread"] == 0, (what, name, info)
        w = info["waves_per_block"]
        cum = cum_table(info["class_weights"], w)
        assert_table(cum, w, (what, "grouped", info))
        for count in (1, w - 1, 8 * w - 1, 8 * w, 8 * w + 1, 256, 2048, 65535, 1 << 20):
            for hf in range(2):
                s = wave_split(count, cum[hf], w, count >= 8 * w)
                assert_partition(s[:-1], s[1:], 0, count, (what, "grouped", count, hf))
    # 4. spread (always 512 x 16): workgroups' shares, none above kSpreadMaxShare, and the waves' parts of them
    for n_chains, min_block in ((11_719, 256), (40_000, 1024), (65_024, 1024)):
        plan = dict(DEALT[0], n_chains=n_chains, n_pieces=n_chains)
        name, info = api.launch_choice(plan, n_groups=50, groups_lean=1, tickets=1, spread_min_block=min_block)
        if info["spread"] != 1:  # (the launcher keeps the grouped launch where a share could overrun the LDS records: never at 22.9 chains a workgroup)
            assert n_chains != 11_719, (what, info)
            continue
        assert name == "hsrans::k_decode_spread<3, false>" and (info["grid"], info["waves_per_block"]) == (2 * CUS, 16), (what, name, info)
        cum = cum_table(info["class_weights"], 16)
        assert_table(cum, 16, (what, "spread"))
        c = spread_share_begin(n_chains, np.arange(info["grid"] + 1), info["grid"], int(cum[0][16]), int(cum[1][16]))
        assert_partition(c[:-1], c[1:], 0, n_chains, (what, "spread shares"))
        assert np.diff(c).max() <= SPREAD_MAX_SHARE and np.diff(c).max() < min_block, (what, int(np.diff(c).max()))
        for b in (0, 1, 255, 256, 511):
            s = wave_split(int(c[b + 1] - c[b]), cum[int(b >= 256)], 16)
            assert_partition(s[:-1], s[1:], 0, int(c[b + 1] - c[b]), (what, "spread waves", b))
    # 5. dealt (always 512 x 16): begin[513], split[512]; a share in two blocks at the most; the waves' parts under the gap
    plan, begin = DEALT
    for bits in (11, 13, 14):
        ok, share, split = api.dealt_shares(begin, plan["decoded_len"] // 64, bits=bits)
        assert ok, (what, bits, "the dealing refuses 11,719 chains in 46 blocks")
        name, info = api.launch_choice(dict(plan, bits=bits), n_groups=len(begin) - 1, groups_lean=1, tickets=1, spread_min_block=256, dealt=1)
        assert info["spread"] == 2 and (info["grid"], info["waves_per_block"]) == (DEALT_GRID, 16), (what, name, info)
        cum = cum_table(info["class_weights"], 16)
        assert_table(cum, 16, (what, "dealt"))
        share = share.astype(np.int64)
        assert_partition(share[:-1], share[1:], 0, plan["n_chains"], (what, "dealt shares"))
        blk_of = np.repeat(np.arange(begin.size - 1), np.diff(begin))
        gap = (int(os.environ.get("HSRANS_DEALT_GAP_GROUPS", 17)) + plan["interval"] // 2) // plan["interval"]
        for b in range(DEALT_GRID):
            c0, c1 = int(share[b]), int(share[b + 1])
            if c1 == c0:
                continue
            touched = np.unique(blk_of[c0:c1])
            assert touched.size <= 2, (what, "a dealt share in three blocks", b)
            sp = int(split[b])
            if touched.size == 2:
                assert 0 < sp < c1 - c0 and blk_of[c0 + sp - 1] == touched[0] and blk_of[c0 + sp] == touched[1], (what, b, sp)
            else:
                assert sp == NO_SPLIT or sp >= c1 - c0, (what, b, sp)
            s = dealt_wave_split(c1 - c0, sp, gap, cum[int(b >= DEALT_GRID // 2)])
            assert_partition(s[:-1], s[1:], 0, c1 - c0, (what, "dealt waves", b))
    # 6. batch: four members' indexes
    if boundaries_too:
        for states, bits in ((64, 11), (64, 13), (32, 11)):
            sizes = [3_000_000] * 4
            for member in (0, 3):
                groups = api.index_boundaries_batch(states, bits, sizes, member)
                total = sizes[member] // states
                assert groups.size and groups[0] >= 4 and (np.diff(groups.astype(np.int64)) >= 4).all() and (groups % 4 == 0).all() and groups[-1] < total // 4 * 4, (what, states, bits)


# ---- the properties ----
@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("name", NAMED)
def test_every_share_rule_under_the_named_lists(monkeypatch, name, waves):
    set_lists(monkeypatch, NAMED[name], waves)
    check_every_rule(NAMED[name], waves, (name, waves))


@pytest.mark.parametrize("waves", WAVES)
def test_every_share_rule_under_random_lists_of_the_domain(monkeypatch, waves):
    """200 seeded lists per shape; the two index rules (slower: 8,192 chains each) under every fifth"""
    for k, ws in enumerate(random_lists(200, seed=waves)):
        assert in_domain(ws)
        set_lists(monkeypatch, ws, waves)
        check_every_rule(ws, waves, (ws, waves), boundaries_too=k % 5 == 0)


@pytest.mark.parametrize("gap", (0, 1, 17, 1000))
def test_the_dealt_gap_keeps_the_waves_parts_a_partition(monkeypatch, gap):
    monkeypatch.setenv("HSRANS_DEALT_GAP_GROUPS", str(gap))
    for ws in NAMED.values():
        set_lists(monkeypatch, ws)
        check_every_rule(ws, 16, (ws, gap), boundaries_too=False)


def test_a_zero_half_loses_a_blocks_chains():
    """why ZERO_HALF is outside the domain: under the rule as the kernel has it (a divisor of 0 counts as 1) no wave of a workgroup of the
    grid's second half takes a chain of its block"""
    cum = cum_table(ZERO_HALF, 16)
    assert cum[1][16] == 0
    with pytest.raises(AssertionError):
        assert_table(cum, 16, "zero half")
    s = 256 * cum[1] // max(1, int(cum[1][16]))
    assert s[16] == 0  # 256 chains, none decoded


def test_unbounded_lengths_wrap_the_table():
    """why HUGE is outside the domain: 16 x 6000 in uint16_t entries"""
    cum = cum_table(HUGE, 16)
    assert cum[0][16] == 96000 > 0xFFFF
    assert (np.diff(cum[0].astype(np.uint16).astype(np.int64)) < 0).any()
    assert cum_table((HI,) * 8, 16)[0][16] == 4800  # the domain's largest table


# ---- the domain, enforced by read_tuning ----
def _facts_of(kind):
    if kind == "persist":
        return persist_kind(64, 11, 4)
    if kind == "persist-small":  # 1,465 chains: a grid of 92 workgroups, not above the CUs
        return persist_kind(64, 11, 32)
    if kind == "persist-pair":
        return persist_kind(32, 11, 4)
    if kind.startswith("direct"):
        _, states, bits, chains = kind.split("-")
        return raw(int(states), int(bits), int(chains)), direct_facts(int(states), int(bits))
    if kind == "grouped-small":  # 46 groups: a grid not above the CUs
        return DEALT[0], dict(n_groups=46, groups_lean=1, tickets=1)
    if kind == "spread":
        return DEALT[0], dict(n_groups=50, groups_lean=1, tickets=1, spread_min_block=256)
    if kind.startswith("dealt"):
        return dict(DEALT[0], bits=int(kind.split("-")[1])), dict(n_groups=46, groups_lean=1, tickets=1, spread_min_block=256, dealt=1)
    raise KeyError(kind)


# the liveness table: list -> (environment beside it, a plan kind whose class_weights name the list)
LIVE = {
    "SLOT_WEIGHTS": ({}, "persist"),
    "SLOT_WEIGHTS4": ({}, "persist-small"),   # and grouped plans of up to 256 groups ("grouped-small")
    "DIRECT_WEIGHTS": ({}, "direct-64-11-8192"),
    "DIRECT_WEIGHTS4": ({}, "direct-64-11-1463"),
    "DIRECT_WEIGHTS6": ({"HSRANS_WAVES_PER_WG": "12"}, "direct-64-11-6144"),  # and, on the default geometry, the dealt launch at 13 / 14 bits
    "DIRECT_WEIGHTS3": ({"HSRANS_WAVES_PER_WG": "12"}, "direct-64-11-1463"),
    "DIRECT_WEIGHTS_PAIR": ({}, "persist-pair"),
    "DUAL_WEIGHTS": ({}, "direct-64-13-8192"),
    "DUAL_WEIGHTS_WIDE": ({}, "direct-64-15-8192"),
    "DEALT_WEIGHTS": ({}, "dealt-11"),
}
MORE_LIVE = [("SLOT_WEIGHTS4", {}, "grouped-small"), ("DIRECT_WEIGHTS6", {}, "dealt-13"), ("DIRECT_WEIGHTS6", {}, "dealt-14"), ("DIRECT_WEIGHTS", {}, "dealt-11"),
             ("DIRECT_WEIGHTS", {}, "direct-64-12-8192"), ("DIRECT_WEIGHTS_PAIR", {}, "direct-32-11-8192"), ("DUAL_WEIGHTS_WIDE", {}, "direct-64-14-8192"),
             ("DIRECT_WEIGHTS", {}, "spread")]


def _weights_under(monkeypatch, env, kind):
    with monkeypatch.context() as m:
        for k, v in env.items():
            m.setenv(k, v)
        return api.launch_choice(_facts_of(kind)[0], **_facts_of(kind)[1])[1]["class_weights"]


@pytest.mark.parametrize("name,env,kind", [(n,) + LIVE[n] for n in LIVE] + MORE_LIVE)
def test_every_list_reaches_a_launch(monkeypatch, name, env, kind):
    """no list is dead: each changes the class_weights of one kind at least — and an accepted list arrives unchanged"""
    default = _weights_under(monkeypatch, env, kind)
    got = _weights_under(monkeypatch, dict(env, **{"HSRANS_" + name: text(STEEP)}), kind)
    assert got == list(STEEP) != default, (name, kind, got, default)
    if kind.startswith("dealt"):  # (three lists reach the dealt launch: the direct launch's, its rank-table twin's at 13 / 14 bits, and its own over both)
        return
    for other in CLASS_LISTS + ("DEALT_WEIGHTS",):  # ... and no other list does
        if other != name:
            assert _weights_under(monkeypatch, dict(env, **{"HSRANS_" + other: text(EDGE)}), kind) == default, (name, other, kind)


REJECTED = {"a zero half": ZERO_HALF, "unbounded": HUGE, "a class of 99": (99,) + STEEP[1:], "a class of 3001": STEEP[:7] + (3001,), "a zero class": (0,) + STEEP[1:],
            "seven values": STEEP[:7], "all zero": (0,) * 8}


@pytest.mark.parametrize("why", REJECTED)
def test_a_list_outside_the_domain_leaves_the_defaults(monkeypatch, why):
    ws = REJECTED[why]
    assert not in_domain(ws)
    sizes = [3_000_000] * 4
    want = {n: _weights_under(monkeypatch, *LIVE[n]) for n in LIVE}
    want_index = H.index_boundaries(64, 11, 12_000_000)
    want_batch = api.index_boundaries_batch(64, 11, sizes, 1)
    want_dealt = api.dealt_shares(DEALT[1], DEALT[0]["decoded_len"] // 64)
    for name, (env, kind) in LIVE.items():
        assert _weights_under(monkeypatch, dict(env, **{"HSRANS_" + name: text(ws)}), kind) == want[name], (why, name)
    monkeypatch.setenv("HSRANS_DIRECT_WEIGHTS", text(ws))
    assert np.array_equal(H.index_boundaries(64, 11, 12_000_000), want_index), why
    monkeypatch.setenv("HSRANS_BATCH_WEIGHTS", text(ws))
    assert np.array_equal(api.index_boundaries_batch(64, 11, sizes, 1), want_batch), why
    monkeypatch.setenv("HSRANS_DEALT_WEIGHTS", text(ws))
    got = api.dealt_shares(DEALT[1], DEALT[0]["decoded_len"] // 64)
    assert got[0] == want_dealt[0] and np.array_equal(got[1], want_dealt[1]) and np.array_equal(got[2], want_dealt[2]), why


def test_accepted_lists_arrive_unchanged_or_rescaled_to_8000(monkeypatch):
    doubled, ragged = tuple(2 * w for w in FLAT), (100, 100, 100, 100, 100, 100, 100, 3000)
    assert rescaled(doubled) == list(FLAT) and rescaled(ragged) == [216] * 7 + [6486] and rescaled(STEEP) == list(STEEP)
    for ws in (STEEP, EDGE, doubled, ragged):
        assert in_domain(ws)
        for name, (env, kind) in LIVE.items():
            want = list(ws) if name == "DEALT_WEIGHTS" else rescaled(ws)  # (HSRANS_DEALT_WEIGHTS and HSRANS_BATCH_WEIGHTS are taken as written)
            assert _weights_under(monkeypatch, dict(env, **{"HSRANS_" + name: text(ws)}), kind) == want, (name, ws)
    # the two knobs without a launch info on the host: the index they cut is the model's under the list as written
    sizes = [3_000_000, 2_000_000, 3_000_000, 1_000_003]
    for ws in (STEEP, REVERSED, doubled):
        monkeypatch.setenv("HSRANS_BATCH_WEIGHTS", text(ws))
        for member in range(4):
            want = batch_boundaries([n // 64 for n in sizes], member, 2 * CUS, 16, ws)
            assert np.array_equal(api.index_boundaries_batch(64, 11, sizes, member), want), (ws, member)
    monkeypatch.delenv("HSRANS_BATCH_WEIGHTS")
    default = api.index_boundaries_batch(64, 11, sizes, 0)
    assert not np.array_equal(default, batch_boundaries([n // 64 for n in sizes], 0, 2 * CUS, 16, STEEP))
    monkeypatch.setenv("HSRANS_DEALT_WEIGHTS", text(STEEP))
    ok, begin, _ = api.dealt_shares(DEALT[1], DEALT[0]["decoded_len"] // 64)
    shares = np.diff(begin[:DEALT_GRID + 1].astype(np.int64))
    assert ok and abs(shares[:256].mean() / shares[256:].mean() - 6500 / 1500) < 0.2, (shares[:256].mean(), shares[256:].mean())


def test_the_spread_launch_names_the_lengths_its_table_was_made_from(monkeypatch):
    """k_decode_spread's table comes from the one-chain-per-wave launch's lengths, whatever the grouped shape's are"""
    plan, facts = _facts_of("spread")
    name, info = api.launch_choice(plan, **facts)
    default = info["class_weights"]
    assert name == "hsrans::k_decode_spread<3, false>" and info["spread"] == 1, (name, info)
    monkeypatch.setenv("HSRANS_SLOT_WEIGHTS", text(STEEP))
    monkeypatch.setenv("HSRANS_SLOT_WEIGHTS4", text(STEEP))
    assert api.launch_choice(plan, **facts)[1]["class_weights"] == default
    monkeypatch.setenv("HSRANS_DIRECT_WEIGHTS", text(REVERSED))
    name, info = api.launch_choice(plan, **facts)
    assert name == "hsrans::k_decode_spread<3, false>" and info["class_weights"] == list(REVERSED), (name, info)
    monkeypatch.setenv("HSRANS_SPREAD", "0")  # the grouped launch of the same plan keeps the grouped shape's
    name, info = api.launch_choice(plan, **facts)
    assert "k_decode_grouped" in name and info["class_weights"] == list(STEEP), (name, info)


def test_the_waves_knob_gives_the_raw_launches_their_grids(monkeypatch):
    """HSRANS_WAVES_PER_WG = 4 / 8 / 12: 1536 x 4, 1024 x 8, 512 x 12; the class lengths count at 12 and 16 waves only"""
    for waves, grid in ((4, 1536), (8, 1024), (12, 512), (16, 512)):
        monkeypatch.setenv("HSRANS_WAVES_PER_WG", str(waves))
        for kind in ("persist", "persist-pair", "direct-64-11-100000"):
            _, info = api.launch_choice(*[_facts_of(kind)[0]], **_facts_of(kind)[1])
            assert (info["grid"], info["waves_per_block"]) == (grid, waves), (kind, waves, info)
            assert (info["class_weights"] == list(FLAT)) == (waves < 12), (kind, waves, info)
