"""Every launch path at class lengths and workgroup shapes off the defaults, on the GPU.

The numbers that shape a launch — the class lengths, the waves per workgroup, the dealt launch's gap, minimum and store policy, the grouped
launch's priority table, the gather's segment floor, a calibration — decide which wave decodes which chains and nothing else: the bytes must be
the oracle's whatever they are.  Every case sets its knobs with monkeypatch, makes a FRESH context after that (tuning is read when a context, a
plan, a batch is made) and everything else under it; "want" is the oracle's decode of the stream; the output has 4096 guard bytes of 0xCC behind
it and a poison fill, is compared on the device, the status is 0 and every case launches twice.  Every case then proves from the launch info
(and the kernel's name, hsrans_launch_choice on the case's own context) that its knob shaped the launch, and that this info is not the
default's.  Four knobs leave no trace in any launch info — HSRANS_GROUP_PRIO, HSRANS_GROUP_PRIO_CLASS, HSRANS_DEALT_GAP_GROUPS (kernel
parameters only) and HSRANS_HPIPE_DIRECT: their cases assert the launch kind they ride on, and the last one the pipeline's own trace line.

Only lists inside the domain of csrc/hsrans_tuning.h run here (tests/test_geometry_domain.py holds every share rule to it on the host); the
first test, which needs no GPU, checks that and the launch each shape takes on the default geometry."""
import functools

import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api, synth
from oracle_lib import BLOCK, MT, RAW
from test_geometry_domain import FLAT, NAMED, REVERSED, STEEP, direct_facts, in_domain, text
from test_gpu_dealt import shifting
from test_gpu_launch_history import GUARD, Member, _check_buf, _header, _kind, _poison, block_case, group_count, oracle_bytes, raw_case, static_total

gpu = pytest.mark.gpu
LISTS = sorted(NAMED)
NAMES = {RAW: "raw", BLOCK: "block", MT: "mt"}
PRIO_CLASS = "1000,0,500,0,1000,0,500,0,300,700"


# ---- streams, made once ----
@functools.lru_cache(maxsize=None)
def direct_data(n, seed=5):
    return synth.enwik8_shaped(n, seed=seed)


def direct_case(ctx, states, bits, n, seed=5):
    """a raw stream with one chain per wave slot of the launch `ctx` would give it (the stream's bytes do not depend on the index)"""
    d = direct_data(n, seed)
    groups = H.index_boundaries(states, bits, n, ctx)
    s, plan = H.encode(H.RAW, states, bits, d, index_groups=groups)
    return d, s, plan


@functools.lru_cache(maxsize=None)
def weighted_case(container, big, bits=12):
    """Groups of at least 8 x waves chains, so that k_decode_grouped splits them over the waves by class weight, and a short last block that it
    splits evenly.  12 bits: neither the dealt nor the spread launch takes such a plan.  A device plan cuts the blocks of a plan with fewer than
    3 groups per CU into parts of 64 chains and more until it has that many (group_parts_of, csrc/hsrans_kernels.h), so blocks of 8 x 16 = 128
    chains (a 9 MB stream) end as groups of 64, never weighted.  The smallest plans that keep weighted groups:
    big: 24 blocks of 1 MiB (4,096 chains each, cut into 31 parts of 132) and one of 79 chains: 745 groups, a grid of 512, above the CUs
         (HSRANS_SLOT_WEIGHTS); weighted at 16 and at 12 waves.  25 MB: 3 x 256 groups x 128 chains x 256 bytes is what it takes
    small: 100 blocks of 127 chains (too short to cut) and one of 50: 101 groups, a grid below the CUs (HSRANS_SLOT_WEIGHTS4); weighted at 12
         waves (96 chains).  At 16 waves no plan with a grid below the CUs keeps a group of 128 chains: its split is the even one."""
    block = 1 << 20 if big else 127 * 256
    n = (24 * block + 79 * 256 - 100) if big else (100 * block + 50 * 256 - 100)
    d = shifting(n, seed=41 + big, period=block)
    s, plan = H.encode(container, 64, bits, d, index_interval=4, block_size=block)
    return d, s, plan


@functools.lru_cache(maxsize=None)
def spread_case(container):
    """64 KiB blocks, a checkpoint every 4 groups, single-symbol blocks among them: not dealt"""
    d = synth.nonstationary(4_000_000, seed=77)
    s, plan = H.encode(container, 64, 11, d, index_interval=4, block_size=1 << 16)
    return d, s, plan


@functools.lru_cache(maxsize=None)
def dealt_case(container, bits):
    """3,000,000 bytes in 64 KiB blocks with a histogram each: 11,719 chains in 46 blocks"""
    d = shifting(3_000_000, seed=bits + 4, period=1 << 16)
    s, plan = H.encode(container, 64, bits, d, index_interval=4, block_size=1 << 16)
    return d, s, plan


def group_sizes(plan, cus=256):
    """the groups of a device plan: group_count's, each cut into parts of at least 64 chains while there are fewer than 3 groups per CU
    (group_parts_of / group_parts_max_of / index_block_part, csrc/hsrans_kernels.h)"""
    begins = group_count(plan)[2]
    counts = np.diff(np.append(begins, _header(plan)["n_chains"]))
    k_max = -(-3 * cus // counts.size) if counts.size < 3 * cus else 1
    out = []
    for c in counts:
        parts = max(1, min(int(c) // 64, k_max))
        out += [int(c) * (p + 1) // parts - int(c) * p // parts for p in range(parts)]
    return out


def facts_of(plan, ctx=None):
    """LaunchFacts of a plan as dplan_fill and dplan_launch fill them"""
    hdr = _header(plan)
    if hdr["container"] == RAW:
        if hdr["interval"]:
            return dict(persistent=1, table_mode=4 if hdr["bits"] == 15 else 3)
        return direct_facts(hdr["states"], hdr["bits"])
    n_groups, fewest, begins, any_fill = group_count(plan)
    n_groups = len(group_sizes(plan))
    lean = hdr["states"] == 64
    dealt = lean and not any_fill and api.dealt_shares(np.append(begins, hdr["n_chains"]), hdr["decoded_len"] // 64, ctx, bits=hdr["bits"])[0]
    return dict(n_groups=n_groups, groups_lean=int(lean), spread_min_block=fewest if lean else 0, tickets=1, dealt=int(dealt))


def choice(plan, ctx=None):
    return api.launch_choice(_kind(_header(plan)), ctx, **facts_of(plan, ctx))


def setenv(monkeypatch, env):
    for k, v in env.items():
        assert "WEIGHTS" not in k or in_domain([int(x) for x in v.split(",")]), (k, v)  # only lists inside the domain reach the GPU
        monkeypatch.setenv("HSRANS_" + k, str(v))


def decode_twice(ctx, oracle, plan_of, default, kernel, expect, what):
    """plan_of(ctx) -> (container, states, bits, data, stream, plan); two launches against the oracle, then the proof from the launch info"""
    container, states, bits, d, s, plan = plan_of(ctx)
    m = Member(ctx, oracle, container, states, bits, d, s, plan)
    for _ in range(2):
        m.launch(what)
    info = m.dplan.launch_info()
    name, chosen = choice(plan, ctx)
    assert chosen == info, (what, "the launch is not the one hsrans_launch_choice names", chosen, info)
    assert name == kernel, (what, name, info)
    for key, want in expect.items():
        assert info[key] == want, (what, key, info)
    if default is not None:
        assert (name, info) != default, (what, "the knob left the launch as the defaults make it", info)
    return info


# ---- the cases ----
# 1. uniform-interval raw: (states, bits, interval, knob); interval 32 gives a grid below the CUs (92 and 184 workgroups): HSRANS_SLOT_WEIGHTS4
PERSIST = [(64, 11, 4, "SLOT_WEIGHTS"), (64, 15, 4, "SLOT_WEIGHTS"), (32, 11, 4, "DIRECT_WEIGHTS_PAIR"), (64, 11, 32, "SLOT_WEIGHTS4"), (64, 15, 32, "SLOT_WEIGHTS4"),
           (32, 11, 32, "SLOT_WEIGHTS4")]
PERSIST_WAVES = [(64, 11, 4), (64, 15, 4), (32, 11, 4)]
WAVES_GRID = {4: 1536, 8: 1024, 12: 512, 16: 512}
# 2. one chain per wave: (states, bits, size, knob, environment beside it)
DIRECT = [(64, 11, 12_000_000, "DIRECT_WEIGHTS", {}), (64, 12, 12_000_000, "DIRECT_WEIGHTS", {}), (64, 13, 12_000_000, "DUAL_WEIGHTS", {}),
          (64, 14, 12_000_000, "DUAL_WEIGHTS_WIDE", {}), (64, 15, 12_000_000, "DUAL_WEIGHTS_WIDE", {}), (32, 11, 12_000_000, "DIRECT_WEIGHTS_PAIR", {}),
          (64, 11, 3_000_000, "DIRECT_WEIGHTS4", {}), (64, 11, 12_000_000, "DIRECT_WEIGHTS6", {"WAVES_PER_WG": 12}), (64, 11, 3_000_000, "DIRECT_WEIGHTS3", {"WAVES_PER_WG": 12})]


def direct_kernel(states, bits):
    return f"hsrans::k_decode_dual<{3 if bits == 13 else 4}>" if states == 64 and bits >= 13 else "hsrans::k_decode_direct<3>"


def persist_plan(states, bits, interval):
    return lambda ctx: (RAW, states, bits) + raw_case(states, bits, interval)


def test_the_lists_are_inside_the_domain_and_the_shapes_take_their_launches(monkeypatch):
    """no GPU: hsrans_launch_choice at the default geometry (256 CUs) for every shape below, under the knobs of its case"""
    for ws in NAMED.values():
        assert in_domain(ws) and sum(ws) == 8000 and min(ws) >= 100
    for states, bits, interval, knob in PERSIST:
        plan = raw_case(states, bits, interval)[2]
        default = choice(plan)
        with monkeypatch.context() as mp:
            setenv(mp, {knob: text(STEEP)})
            name, info = choice(plan)
        assert name == default[0] == f"hsrans::k_decode_persist<{4 if bits == 15 else 3}>" and info["class_weights"] == list(STEEP) != default[1]["class_weights"], (knob, name, info)
        assert 0 < static_total(info["chains"], states, info) <= info["chains"] or states == 32
    for states, bits, n, knob, env in DIRECT:
        with monkeypatch.context() as mp:
            setenv(mp, env)
            default = choice(direct_case(None, states, bits, n)[2])
            setenv(mp, {knob: text(STEEP)})
            plan = direct_case(None, states, bits, n)[2]
            name, info = choice(plan)
        assert name == direct_kernel(states, bits) and info["class_weights"] == list(STEEP) != default[1]["class_weights"], (knob, name, info)
        if states == 64 and bits <= 12:  # 12 MB: 5,859 chains, in both halves of the grid; 3 MB: 1,464 chains, a grid not above the CUs
            assert (info["grid"] <= 256) == (n == 3_000_000) and info["chains"] == (1_464 if n == 3_000_000 else 5_859), (knob, info)
    for container in (MT, BLOCK):
        for big, knob in ((1, "SLOT_WEIGHTS"), (0, "SLOT_WEIGHTS4")):
            for waves in (16, 12):
                plan = weighted_case(container, big)[2]
                with monkeypatch.context() as mp:
                    setenv(mp, {knob: text(STEEP), "WAVES_PER_WG": waves})
                    name, info = choice(plan)
                counts = np.array(group_sizes(plan))
                assert name == "hsrans::k_decode_grouped<3, true, false>" and info["spread"] == 0 and info["waves_per_block"] == waves and info["class_weights"] == list(STEEP), (name, info)
                assert (info["grid"], counts.size) == ((512, 745) if big else (101, 101)) and info["dynamic_groups"] == big, (info, counts.size)
                assert ((counts[:-1] >= 8 * waves).all() or (not big and waves == 16)) and counts[-1] < 8 * waves, (info, counts)
        name, info = choice(block_case(container, 64, 11)[2])
        assert name == "hsrans::k_decode_grouped<3, true, false>" and info["dynamic_groups"] == 1, (name, info)
        name, info = choice(spread_case(container)[2])
        assert name == "hsrans::k_decode_spread<3, false>" and info["spread"] == 1, (name, info)
        for bits in (11, 13, 14):
            name, info = choice(dealt_case(container, bits)[2])
            assert name == ("hsrans::k_decode_dealt<true, false>" if bits == 11 else f"hsrans::k_decode_dealt_rank<{bits}u, false>") and info["spread"] == 2, (name, info)
            assert info["chains"] == 11_719 and group_count(dealt_case(container, bits)[2])[0] == 46
    plan = dealt_case(MT, 11)[2]
    with monkeypatch.context() as mp:
        setenv(mp, {"DEALT_WT": 0})
        assert choice(plan)[0] == "hsrans::k_decode_dealt<false, false>"
        setenv(mp, {"DEALT_MIN_CHAINS": 100_000})
        assert choice(plan)[1]["spread"] != 2


# 1.
@gpu
@pytest.mark.parametrize("ws", LISTS)
@pytest.mark.parametrize("case", PERSIST, ids=lambda c: f"{c[0]}-{c[1]}-g{c[2]}")
def test_uniform_interval_launch_under_class_lengths(monkeypatch, oracle, case, ws):
    states, bits, interval, knob = case
    default = choice(raw_case(states, bits, interval)[2])
    setenv(monkeypatch, {knob: text(NAMED[ws])})
    ctx = H.Context(0)
    info = decode_twice(ctx, oracle, persist_plan(states, bits, interval), default, f"hsrans::k_decode_persist<{4 if bits == 15 else 3}>",
                        dict(class_weights=list(NAMED[ws]), waves_per_block=16), (case, ws))
    assert static_total(info["chains"], states, info) <= info["chains"]


@gpu
@pytest.mark.parametrize("waves", (4, 8, 12))
@pytest.mark.parametrize("case", PERSIST_WAVES, ids=lambda c: f"{c[0]}-{c[1]}-g{c[2]}")
def test_uniform_interval_launch_at_other_workgroup_shapes(monkeypatch, oracle, case, waves):
    states, bits, interval = case
    default = choice(raw_case(*case)[2])
    setenv(monkeypatch, {"WAVES_PER_WG": waves, "SLOT_WEIGHTS": text(STEEP), "DIRECT_WEIGHTS_PAIR": text(STEEP)})
    ctx = H.Context(0)
    decode_twice(ctx, oracle, persist_plan(*case), default, f"hsrans::k_decode_persist<{4 if bits == 15 else 3}>",
                 dict(waves_per_block=waves, grid=WAVES_GRID[waves] if bits == 11 else {4: 768}.get(waves, 512), class_weights=list(STEEP if waves == 12 else FLAT)), (case, waves))


# 2.
@gpu
@pytest.mark.parametrize("ws", LISTS)
@pytest.mark.parametrize("case", DIRECT, ids=lambda c: f"{c[0]}-{c[1]}-{c[2]}-{c[3]}")
def test_one_chain_per_wave_under_class_lengths(monkeypatch, oracle, case, ws):
    """the index is cut by the context under the list, and the launch names the list"""
    states, bits, n, knob, env = case
    setenv(monkeypatch, env)
    default = choice(direct_case(None, states, bits, n)[2])
    setenv(monkeypatch, {knob: text(NAMED[ws])})
    ctx = H.Context(0)
    info = decode_twice(ctx, oracle, lambda c: (RAW, states, bits) + direct_case(c, states, bits, n), default, direct_kernel(states, bits),
                        dict(class_weights=list(NAMED[ws]), waves_per_block=env.get("WAVES_PER_WG", 16)), (case, ws))
    assert info["chains"] <= info["grid"] * info["waves_per_block"] * (2 if states == 32 or info["chains_per_wave"] == 2 else 1), info


@gpu
@pytest.mark.parametrize("waves", (4, 8))
def test_one_chain_per_wave_at_other_workgroup_shapes(monkeypatch, oracle, waves):
    default = choice(direct_case(None, 64, 11, 12_000_000)[2])
    setenv(monkeypatch, {"WAVES_PER_WG": waves, "DIRECT_WEIGHTS": text(STEEP)})
    ctx = H.Context(0)
    decode_twice(ctx, oracle, lambda c: (RAW, 64, 11) + direct_case(c, 64, 11, 12_000_000), default, "hsrans::k_decode_direct<3>",
                 dict(waves_per_block=waves, grid=-(-5_859 // waves), class_weights=list(FLAT)), waves)


@gpu
@pytest.mark.parametrize("states,bits,knob", [(64, 11, "DIRECT_WEIGHTS"), (64, 13, "DUAL_WEIGHTS"), (32, 11, "DIRECT_WEIGHTS_PAIR")])
def test_an_index_cut_under_one_list_decodes_under_another(monkeypatch, oracle, states, bits, knob):
    """a plan is portable: its chains need not fit the classes of the waves that decode them"""
    n = 12_000_000
    default = choice(direct_case(None, states, bits, n)[2])
    with monkeypatch.context() as mp:
        setenv(mp, {knob: text(STEEP)})
        case = direct_case(None, states, bits, n)
    assert not np.array_equal(api.plan_tables(case[2])[2]["steps"], api.plan_tables(direct_case(None, states, bits, n)[2])[2]["steps"])
    setenv(monkeypatch, {knob: text(REVERSED)})
    ctx = H.Context(0)
    decode_twice(ctx, oracle, lambda c: (RAW, states, bits) + case, default, direct_kernel(states, bits), dict(class_weights=list(REVERSED)), (states, bits))


# 3.
@gpu
@pytest.mark.parametrize("waves", (16, 12))
@pytest.mark.parametrize("big", (1, 0), ids=("745-groups", "101-groups"))
@pytest.mark.parametrize("container,ws", [(MT, ws) for ws in LISTS] + [(BLOCK, "steep"), (BLOCK, "edge")], ids=lambda v: NAMES.get(v, v) if isinstance(v, int) else v)
def test_grouped_launch_with_the_weighted_split(monkeypatch, oracle, container, ws, big, waves):
    default = choice(weighted_case(container, big)[2])
    setenv(monkeypatch, {"SLOT_WEIGHTS" if big else "SLOT_WEIGHTS4": text(NAMED[ws]), "WAVES_PER_WG": waves})
    ctx = H.Context(0)
    decode_twice(ctx, oracle, lambda c: (container, 64, 12) + weighted_case(container, big), default, "hsrans::k_decode_grouped<3, true, false>",
                 dict(class_weights=list(NAMED[ws]), waves_per_block=waves, spread=0, grid=512 if big else 101, dynamic_groups=big), (NAMES[container], big, ws, waves))


@gpu
@pytest.mark.parametrize("env", ({"GROUP_PRIO": 1000}, {"GROUP_PRIO_CLASS": PRIO_CLASS}), ids=("prio-1000", "prio-class"))
@pytest.mark.parametrize("container", (MT, BLOCK), ids=("mt", "block"))
def test_grouped_launch_under_the_priority_knobs(monkeypatch, oracle, container, env):
    """tickets drawn (9,000,000 bytes in 8 KiB blocks: an even split, classes [0..7] of the table), and the weighted plan (classes [8..9]).  The
    priority is a kernel parameter that no launch info shows: what is asserted is the launch it rides on."""
    setenv(monkeypatch, env)
    ctx = H.Context(0)
    decode_twice(ctx, oracle, lambda c: (container, 64, 11) + block_case(container, 64, 11), None, "hsrans::k_decode_grouped<3, true, false>",
                 dict(dynamic_groups=1, spread=0, waves_per_block=8), (NAMES[container], env))
    decode_twice(ctx, oracle, lambda c: (container, 64, 12) + weighted_case(container, 1), None, "hsrans::k_decode_grouped<3, true, false>",
                 dict(dynamic_groups=1, spread=0, waves_per_block=16), (NAMES[container], env, "weighted"))


# 4.
@gpu
@pytest.mark.parametrize("container,ws", [(MT, ws) for ws in LISTS] + [(BLOCK, "steep")])
def test_spread_launch_under_class_lengths(monkeypatch, oracle, container, ws):
    default = choice(spread_case(container)[2])
    setenv(monkeypatch, {"DIRECT_WEIGHTS": text(NAMED[ws]), "SLOT_WEIGHTS": text(FLAT)})
    ctx = H.Context(0)
    decode_twice(ctx, oracle, lambda c: (container, 64, 11) + spread_case(container), default, "hsrans::k_decode_spread<3, false>",
                 dict(spread=1, class_weights=list(NAMED[ws]), grid=512, waves_per_block=16), (NAMES[container], ws))


# 5.
def dealt_kernel(bits, wt=True):
    return f"hsrans::k_decode_dealt<{'true' if wt else 'false'}, false>" if bits == 11 else f"hsrans::k_decode_dealt_rank<{bits}u, false>"


@gpu
@pytest.mark.parametrize("ws", LISTS)
@pytest.mark.parametrize("container,bits", [(MT, 11), (MT, 13), (MT, 14), (BLOCK, 11)])
def test_dealt_launch_under_class_lengths(monkeypatch, oracle, container, bits, ws):
    default = choice(dealt_case(container, bits)[2])
    setenv(monkeypatch, {"DEALT_WEIGHTS": text(NAMED[ws])})
    ctx = H.Context(0)
    decode_twice(ctx, oracle, lambda c: (container, 64, bits) + dealt_case(container, bits), default, dealt_kernel(bits),
                 dict(spread=2, class_weights=list(NAMED[ws]), grid=512, waves_per_block=16), (NAMES[container], bits, ws))


@gpu
def test_dealt_launch_with_nt_stores(monkeypatch, oracle):
    """HSRANS_DEALT_WT=0: a kernel of its own"""
    default = choice(dealt_case(MT, 11)[2])
    setenv(monkeypatch, {"DEALT_WT": 0})
    ctx = H.Context(0)
    decode_twice(ctx, oracle, lambda c: (MT, 64, 11) + dealt_case(MT, 11), default, "hsrans::k_decode_dealt<false, false>", dict(spread=2), "nt")


@gpu
@pytest.mark.parametrize("gap", (0, 1000))
@pytest.mark.parametrize("bits", (11, 14))
def test_dealt_launch_under_the_gap(monkeypatch, oracle, bits, gap):
    """0: no second prologue is counted; 1000 groups = 250 chains of this plan: more than any share holds.  (The gap is a kernel parameter
    that no launch info shows; tests/test_geometry_domain.py holds the waves' parts under it to a partition.)"""
    setenv(monkeypatch, {"DEALT_GAP_GROUPS": gap, "DEALT_WEIGHTS": text(STEEP)})
    ctx = H.Context(0)
    decode_twice(ctx, oracle, lambda c: (MT, 64, bits) + dealt_case(MT, bits), None, dealt_kernel(bits), dict(spread=2, class_weights=list(STEEP)), (bits, gap))


@gpu
def test_a_plan_below_the_dealt_minimum_falls_back(monkeypatch, oracle):
    default = choice(dealt_case(MT, 11)[2])
    setenv(monkeypatch, {"DEALT_MIN_CHAINS": 100_000})
    ctx = H.Context(0)
    container, states, bits, d, s, plan = (MT, 64, 11) + dealt_case(MT, 11)
    m = Member(ctx, oracle, container, states, bits, d, s, plan)
    for _ in range(2):
        m.launch("below the minimum")
    info = m.dplan.launch_info()
    assert default[1]["spread"] == 2 and info["spread"] != 2 and info != default[1], info


# 6.
BATCH_SIZES = [3_000_000] * 4


def batch_members(ctx, oracle, states, bits, index_ctx=None):
    ms = []
    for k, n in enumerate(BATCH_SIZES):
        d = direct_data(n, seed=60 + k)
        groups = api.index_boundaries_batch(states, bits, BATCH_SIZES, k, index_ctx or ctx)
        s, plan = H.encode(H.RAW, states, bits, d, index_groups=groups)
        ms.append(Member(ctx, oracle, RAW, states, bits, d, s, plan))
    return ms


def batch_twice(ctx, ms, what):
    import torch
    batch = ctx.make_batch([m.dplan for m in ms])
    for k in range(2):
        for m in ms:
            m.buf[:m.n].fill_(_poison(k))
        ctx.decode_device_batch(batch, [m.d_in for m in ms], [m.buf[:m.n] for m in ms], stream_lengths=[m.m for m in ms])
        torch.cuda.synchronize()
        assert ctx.batch_status(batch) == [0] * len(ms), what
        for i, m in enumerate(ms):
            _check_buf(m.buf, m.d_want, f"{what}: launch {k + 1}, member {i}")
    info = batch.info()
    batch.close()
    assert info["launches"] == 1 and info["direct_members"] == len(ms) and info["solo_members"] == 0 and info["grouped_members"] == 0, (what, info)
    return info


@gpu
@pytest.mark.parametrize("ws,other", (("steep", "reversed"), ("reversed", "steep")))
def test_batch_launch_under_class_lengths(monkeypatch, oracle, ws, other):
    default = None
    if ws == "steep":
        ctx = H.Context(0)
        default = batch_twice(ctx, batch_members(ctx, oracle, 64, 11), "defaults")
    setenv(monkeypatch, {"BATCH_WEIGHTS": text(NAMED[ws])})
    ctx = H.Context(0)
    ms = batch_members(ctx, oracle, 64, 11)
    info = batch_twice(ctx, ms, ws)
    assert info["class_weights"] == list(NAMED[ws]) and (info["grid"], info["block"]) == (512, 1024), info
    assert default is None or default["class_weights"] != info["class_weights"]
    # a batch made under the other list over the same streams' plans (remade on its context: a device plan belongs to one)
    setenv(monkeypatch, {"BATCH_WEIGHTS": text(NAMED[other])})
    ctx2 = H.Context(0)
    ms2 = [Member(ctx2, oracle, RAW, 64, 11, direct_data(m.n, seed=60 + k), m.stream, m.plan) for k, m in enumerate(ms)]
    info = batch_twice(ctx2, ms2, f"{ws} plans under {other}")
    assert info["class_weights"] == list(NAMED[other]), info


@gpu
@pytest.mark.parametrize("states,bits,block", ((64, 13, 1024), (32, 11, 1024)))
def test_wide_and_paired_batch_launches_under_class_lengths(monkeypatch, oracle, states, bits, block):
    setenv(monkeypatch, {"BATCH_WEIGHTS": text(STEEP)})
    ctx = H.Context(0)
    info = batch_twice(ctx, batch_members(ctx, oracle, states, bits), (states, bits))
    assert info["class_weights"] == list(STEEP) and info["block"] == block, info


# 7.
N_GATHER = 1_000_003
FLOORS = {64: (256, 1024), 1000: (1024, 1024), 65536: (65536, 65536)}  # floor -> segment of the raw plan (256-byte chains), of the mt_ plan (1,024-byte chains)
DEFAULT_SEGMENT = 4096
RANGES = [(255, 3), (65_535, 2), (1, 1), (N_GATHER - 70_001, 70_001), (500_000, 0), (131_071, 66_000), (7, 1_000)]  # crosses a border of every segment length; single byte; to the last byte; empty


@functools.lru_cache(maxsize=None)
def gather_case(container):
    d = synth.nonstationary(N_GATHER, seed=88)
    if container == RAW:
        s, plan = H.encode(H.RAW, 64, 11, d, index_interval=4)
    else:
        s, plan = H.encode(H.MT, 64, 11, d, index_interval=16, block_size=1 << 16)
    return d, s, plan


def packed(ranges, first=3):
    out, at = [], first
    for off, n in ranges:
        out.append((off, n, at))
        at += n + 5
    return out, at


def tasks_of(ranges, segment):
    """a range is cut at the absolute multiples of the segment length"""
    return sum((off + n - 1) // segment - off // segment + 1 for off, n in ranges if n)


def check_gather(dst, want, ranges, what):
    import torch
    expect = torch.full_like(dst, 0xCC)
    expect[:dst.numel() - GUARD] = 0x5A
    for off, n, at in ranges:
        expect[at:at + n] = want[off:off + n]
    assert torch.equal(dst, expect), (what, int((dst != expect).sum()), "bytes differ from the oracle's slices or the poison")


@gpu
@pytest.mark.parametrize("floor", sorted(FLOORS))
@pytest.mark.parametrize("container", (RAW, MT), ids=("raw", "mt"))
def test_gather_under_the_segment_floor(monkeypatch, oracle, container, floor):
    import torch
    segment = FLOORS[floor][container == MT]
    setenv(monkeypatch, {"GATHER_MIN_SEGMENT": floor})
    ctx = H.Context(0)
    m = Member(ctx, oracle, container, 64, 11, *gather_case(container))
    ranges, total = packed(RANGES)

    def fresh():
        dst = torch.full((total + GUARD,), 0xCC, dtype=torch.uint8, device="cuda")
        dst[:total] = 0x5A
        return dst

    for k in range(2):
        dst = fresh()
        ctx.decode_device_gather(m.dplan, m.d_in, ranges, dst[:total], stream_length=m.m)
        assert ctx.status(m.dplan) == 0
        check_gather(dst, m.d_want, ranges, ("gather", k))
        dst = fresh()
        d_ranges = torch.tensor(ranges, dtype=torch.int64, device="cuda")
        ctx.decode_device_gather_indirect(m.dplan, m.d_in, d_ranges, dst[:total], stream_length=m.m)
        assert ctx.status(m.dplan) == 0
        check_gather(dst, m.d_want, ranges, ("indirect", k))
    # the proof: the same plan as the one member of a gather set, whose info counts the tasks of its last gather
    gset = ctx.make_gather_set([m.dplan], [m.d_in], [m.m])
    dst = fresh()
    ctx.decode_device_gather_batch(gset, [(0,) + r for r in ranges], dst[:total])
    assert ctx.gather_set_status(gset) == [0]
    check_gather(dst, m.d_want, ranges, "set")
    tasks = sum(gset.info()["kind_tasks"])
    gset.close()
    assert tasks == tasks_of(RANGES, segment) != tasks_of(RANGES, DEFAULT_SEGMENT), (tasks, segment)


@gpu
def test_a_gather_set_whose_members_were_made_under_different_floors(monkeypatch, oracle):
    import torch
    ranges, total = packed(RANGES + RANGES)
    members, rows = [], []
    for k, (container, floor) in enumerate(((RAW, 64), (MT, 65536))):
        with monkeypatch.context() as mp:
            setenv(mp, {"GATHER_MIN_SEGMENT": floor})
            ctx = H.Context(0) if k == 0 else ctx
            members.append(Member(ctx, oracle, container, 64, 11, *gather_case(container)))  # (a floor is read when a device plan is made)
        rows += [(k,) + r for r in ranges[k * len(RANGES):(k + 1) * len(RANGES)]]
    gset = ctx.make_gather_set([m.dplan for m in members], [m.d_in for m in members], [m.m for m in members])
    for k in range(2):
        dst = torch.full((total + GUARD,), 0xCC, dtype=torch.uint8, device="cuda")
        dst[:total] = 0x5A
        ctx.decode_device_gather_batch(gset, rows, dst[:total])
        assert ctx.gather_set_status(gset) == [0, 0]
        expect = torch.full_like(dst, 0xCC)
        expect[:total] = 0x5A
        for member, off, n, at in rows:
            expect[at:at + n] = members[member].d_want[off:off + n]
        assert torch.equal(dst, expect), k
    tasks = sum(gset.info()["kind_tasks"])
    gset.close()
    assert tasks == tasks_of(RANGES, 256) + tasks_of(RANGES, 65536) != 2 * tasks_of(RANGES, DEFAULT_SEGMENT), tasks


@gpu
@pytest.mark.parametrize("floor", (64, 65536))
def test_planes_gather_under_the_segment_floor(monkeypatch, floor):
    """element ranges of a small bf16 frame; expected: slices of the array.  The proof: the planes' plans as a gather set of the test's own"""
    import torch
    n, block, interval = 300_007, 1 << 16, 32  # 2,048-byte chains: segments of 2,048 and 65,536 bytes (4,096 by default)
    segment = {64: 2048, 65536: 65536}[floor]
    rng = np.random.default_rng(29)
    a = (rng.standard_normal(n).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    setenv(monkeypatch, {"GATHER_MIN_SEGMENT": floor})
    ctx = H.Context(0)
    t = torch.from_numpy(a.view(np.int16)).cuda()
    frame = torch.full((H.planes_capacity(2, 64, n),), 0xA5, dtype=torch.uint8, device="cuda")
    work = torch.full((H.planes_workspace_bytes(2, n),), 0xA5, dtype=torch.uint8, device="cuda")
    _, desc, plans = ctx.encode_device_planes(t, frame, work, states=64, bits=11, block_size=block, index_interval=interval, store_incompressible=False)
    planes = ctx.make_planes(desc, plans)
    pg = ctx.make_planes_gather(planes, frame)
    shapes = [(2047, 3), (65_535, 2), (1, 1), (n - 70_001, 70_001), (500, 0), (131_071, 66_000)]
    ranges, total = packed(shapes, first=1)
    for k in range(2):
        out = torch.full((2 * total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        gwork = torch.full((H.planes_gather_workspace_bytes(2, len(ranges), sum(c for _, c in shapes)) + 256,), 0xA5, dtype=torch.uint8, device="cuda")
        ctx.decode_device_planes_gather(pg, ranges, out[:2 * total].view(torch.int16), gwork)
        assert ctx.planes_gather_status(pg) == [0, 0]
        want = np.full(2 * total + GUARD, 0xA5, np.uint8)
        for off, c, at in ranges:
            want[2 * at:2 * (at + c)] = a[off:off + c].view(np.uint8)
        assert np.array_equal(out.cpu().numpy(), want), k
    streams = [frame[desc.offset[p]:desc.offset[p] + desc.length[p]] for p in range(2)]
    gset = ctx.make_gather_set([plans[p] for p in range(2)], streams)
    dst = torch.zeros(2 * total + 64, dtype=torch.uint8, device="cuda")
    ctx.decode_device_gather_batch(gset, [(p, off, c, p * total + at) for off, c, at in ranges for p in range(2)], dst)
    assert ctx.gather_set_status(gset) == [0, 0]
    tasks = sum(gset.info()["kind_tasks"])
    for h in (gset, pg, planes):
        h.close()
    assert tasks == 2 * tasks_of(shapes, segment) != 2 * tasks_of(shapes, DEFAULT_SEGMENT), (tasks, segment)


# 8.
@gpu
def test_every_launch_kind_after_each_calibration(oracle):
    """one context: hsrans_ctx_calibrate, then two hsrans_ctx_calibrate_runs; after each the direct (index cut by the calibrated context),
    spread, dealt and batch shapes decode to the oracle's bytes with lengths inside the calibrator's bounds"""
    ctx = H.Context(0)
    n = 12_000_000
    inside = lambda ws: len(ws) == 8 and all(100 <= w <= 3000 for w in ws) and abs(sum(ws) - 8000) <= 8
    rep = None
    for step in range(3):
        r = ctx.calibrate(bits=11, iterations=3) if step == 0 else ctx.calibrate_runs(bits=11, copies=2 * step, iterations=3)
        assert inside(r["class_weights"]), (step, r)
        rep = rep or r
        info = decode_twice(ctx, oracle, lambda c: (RAW, 64, 11) + direct_case(c, 64, 11, n), None, "hsrans::k_decode_direct<3>", {}, ("direct", step))
        assert info["class_weights"] == rep["class_weights"], (step, info, rep)  # (the one-stream fit stays the launch's own set)
        info = decode_twice(ctx, oracle, lambda c: (MT, 64, 11) + spread_case(MT), None, "hsrans::k_decode_spread<3, false>", dict(spread=1), ("spread", step))
        assert info["class_weights"] == rep["class_weights"], (step, info, rep)
        info = decode_twice(ctx, oracle, lambda c: (MT, 64, 11) + dealt_case(MT, 11), None, "hsrans::k_decode_dealt<true, false>", dict(spread=2), ("dealt", step))
        assert inside(info["class_weights"]), (step, info)
        info = batch_twice(ctx, batch_members(ctx, oracle, 64, 11), ("batch", step))
        assert inside(info["class_weights"]), (step, info)


# 9.
@gpu
def test_host_pipeline_storing_straight_into_page_locked_output(monkeypatch, oracle, capfd):
    import torch
    from hypersonic_rans_amd import pipeline
    setenv(monkeypatch, {"HPIPE_DIRECT": 1, "HPIPE_TRACE": 1})
    ctx = H.Context(0)
    d, s, plan = dealt_case(MT, 11)
    want = oracle_bytes(oracle, MT, 64, 11, s, plan, d)
    host_in = torch.from_numpy(s.copy()).pin_memory()
    host_out = torch.full((d.size + GUARD,), 0xCC, dtype=torch.uint8).pin_memory()
    dec = pipeline.PipelinedHostDecoder(ctx, plan)
    for k in range(2):
        host_out[:d.size].fill_(_poison(k))
        dec.decode(host_in, host_out[:d.size])
        got = host_out.numpy()
        assert np.array_equal(got[:d.size], want), (k, int(np.argmax(got[:d.size] != want)))
        assert (got[d.size:] == 0xCC).all(), "wrote behind the output"
    dec.close()
    err = capfd.readouterr().err
    assert err.count("hpipe direct") == 2 and "hpipe staged" not in err, err
