"""Which kernel a single-plan decode launch runs (hsrans_launch_choice = choose_launch in csrc/hsrans_kernels.hip): pure host logic, no GPU,
ctx = NULL (the MI355X defaults: 256 CUs, 160 KiB of LDS).

One case per row of DESIGN.md §5's kernel table that a single-plan launch can reach (the batch kernels and the planners are launched
elsewhere), then the edges the launcher's code writes down.  The expected names and shapes are DESIGN.md's and what the GPU tests assert of
hsrans_dplan_launch_info after a launch (tests/test_gpu_dealt.py, test_gpu_configs.py, test_gpu_parity.py); the LDS sizes are DESIGN.md's
sums: a wave's stream ring is 4 x 512 B + a 512 B mirror, an 8-byte table 8 << bits, a spread share's piece records (127 + 1) x 48 B."""
import numpy as np
import pytest

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

RING = 4 * 512 + 512
LDS_LIMIT = 160 * 1024
MERGEABLE_WITH_HIST = 2 | 4  # a raw plan with an index: kPlanMergeable | kPlanHasHist
WALK = 1


def raw(bits, n_chains, interval=0, decoded_len=100_000_000):
    return dict(container=H.RAW, states=64, bits=bits, flags=MERGEABLE_WITH_HIST, decoded_len=decoded_len, n_chains=n_chains, n_pieces=n_chains, shared_hist=1,
                interval=interval)


def blocks(bits, size, block, interval, container=H.MT):
    """header fields of a block_/mt_ plan of `size` bytes in blocks of `block` bytes with a checkpoint every `interval` groups, and its blocks as
    chain ranges"""
    lengths = [min(block, size - lo) for lo in range(0, size, block)]
    begin = np.concatenate([[0], np.cumsum([-(-n // (interval * 64)) for n in lengths])]).astype(np.uint32)
    n = int(begin[-1])
    return dict(container=container, states=64, bits=bits, flags=0, decoded_len=size, n_chains=n, n_pieces=n, interval=interval), begin


def lean(plan, block_begin, groups_per_block, *, coded_blocks_only=True, **more):
    """the facts of a lean grouped plan; dealt = what hsrans_dealt_shares says of its blocks (a plan with a single-symbol block has no dealing)"""
    dealt = coded_blocks_only and api.dealt_shares(block_begin, plan["decoded_len"] // 64, bits=plan["bits"])[0]
    return dict(n_groups=(len(block_begin) - 1) * groups_per_block, groups_lean=1, spread_min_block=int(np.diff(block_begin)[:-1].min()), tickets=1, dealt=int(dealt), **more)


# 24 MB in 256 KiB blocks, a checkpoint every 8 groups (tests/test_gpu_dealt.py's first case): 92 blocks of 512 chains for 512 workgroups
FEW_LARGE = blocks(11, 24_000_000, 1 << 18, 8)
# 2^30 bytes in 256 KiB blocks (the grouped launch's home ground): 4,096 blocks, 16 per CU
MANY = blocks(11, 1 << 30, 1 << 18, 16)

ROWS = [
    # plan kind, header, facts, kernel, grid, waves, what else the launch info says
    ("raw 11 bits, one chain per wave", raw(11, 8192), dict(persistent=1, table_mode=3), "hsrans::k_decode_direct<3>", 512, 16, dict(lds_bytes=16 * RING + (8 << 11))),
    ("raw 13 bits", raw(13, 8192), dict(persistent=1, table_mode=3, dual=1), "hsrans::k_decode_dual<3>", 256, 16, dict(chains_per_wave=2, lds_bytes=32 * RING + (8 << 13))),
    ("raw 14 bits", raw(14, 8192), dict(persistent=1, table_mode=4, dual=1), "hsrans::k_decode_dual<4>", 256, 16, dict(chains_per_wave=2, table_mode=4)),
    ("raw, uniform interval", raw(11, 24415, interval=64), dict(persistent=1, table_mode=3), "hsrans::k_decode_persist<3>", 512, 16, {}),
    ("lean grouped, 16 blocks per CU", MANY[0], lean(*MANY, 1), "hsrans::k_decode_grouped<3, true, false>", 4 * 256, 8, dict(dynamic_groups=1, spread=0)),
    ("lean grouped, few large blocks, dealt", FEW_LARGE[0], lean(*FEW_LARGE, 8), "hsrans::k_decode_dealt<true, false>", 512, 16,
     dict(spread=2, dynamic_groups=0, lds_bytes=16 * RING + 2 * (8 << 11) + 2048)),
    ("the same with a single-symbol block", FEW_LARGE[0], lean(*FEW_LARGE, 8, coded_blocks_only=False), "hsrans::k_decode_spread<3, false>", 512, 16,
     dict(spread=1, dynamic_groups=0, lds_bytes=16 * RING + 2 * (8 << 11) + 128 * 48)),
    ("raw without an index", dict(container=H.RAW, states=64, bits=11, decoded_len=1 << 20, n_chains=1, n_pieces=1, shared_hist=1), dict(single_valid=1, single_ring_entries=2048),
     "hsrans::k_decode_single", 1, 2, {}),
    ("block_ walk", dict(container=H.BLOCK, states=64, bits=11, flags=WALK, decoded_len=1 << 20, n_chains=1, n_pieces=1), {}, "hsrans::k_decode<0, false>", 1, 1, dict(walk=1)),
]


@pytest.mark.parametrize("kind,plan,facts,kernel,grid,waves,more", ROWS, ids=[r[0] for r in ROWS])
def test_kernel_table_rows(kind, plan, facts, kernel, grid, waves, more):
    name, info = api.launch_choice(plan, **facts)
    assert name == kernel, (name, info)
    assert (info["grid"], info["waves_per_block"], info["block"]) == (grid, waves, waves * 64), info
    assert info["chains"] == plan["n_chains"]
    assert info["lds_bytes"] <= LDS_LIMIT, info
    for key, want in more.items():
        assert info[key] == want, (key, info)


def test_the_dealt_row_has_a_dealing_and_the_single_symbol_row_has_none():
    assert lean(*FEW_LARGE, 8)["dealt"] == 1 and lean(*FEW_LARGE, 8, coded_blocks_only=False)["dealt"] == 0
    assert lean(*MANY, 1)["dealt"] == 0  # (a block and more per workgroup slot: the grouped launch's)


def test_twelve_bits_never_take_the_dealt_launch():
    plan, begin = blocks(12, 24_000_000, 1 << 18, 8)
    name, info = api.launch_choice(plan, **dict(lean(plan, begin, 8), dealt=1))
    assert info["spread"] != 2 and name == "hsrans::k_decode_grouped<3, true, false>", (name, info)  # (two 32 KiB tables twice per CU: no spread launch either)
    assert info["lds_bytes"] <= LDS_LIMIT


@pytest.mark.parametrize("bits", (13, 14))
def test_wide_histograms_are_dealt_only_with_dealt_wide(bits, monkeypatch):
    plan, begin = blocks(bits, 24_000_000, 1 << 18, 8)
    facts = dict(lean(plan, begin, 8), dealt=1)
    name, info = api.launch_choice(plan, **facts)
    assert name == f"hsrans::k_decode_dealt_rank<{bits}u, false>" and info["spread"] == 2 and (info["grid"], info["waves_per_block"]) == (512, 16), (name, info)
    assert info["table_mode"] == 4 and info["lds_bytes"] <= LDS_LIMIT
    monkeypatch.setenv("HSRANS_DEALT_WIDE", "0")
    name, info = api.launch_choice(plan, **facts)
    assert name == "hsrans::k_decode_grouped<4, true, false>" and info["spread"] == 0, (name, info)
    assert info["lds_bytes"] <= LDS_LIMIT


def test_an_index_pass_takes_neither_the_dealt_nor_the_spread_nor_the_single_launch():
    plan, begin = FEW_LARGE
    for coded in (True, False):
        name, info = api.launch_choice(dict(plan, shared_hist=0), **dict(lean(plan, begin, 8, coded_blocks_only=coded, index_pass=1), dealt=1))
        assert name == "hsrans::k_decode<0, false>" and info["spread"] == 0 and info["dynamic_groups"] == 0, (name, info)
    single = dict(container=H.RAW, states=64, bits=11, decoded_len=1 << 20, n_chains=1, n_pieces=1)
    name, info = api.launch_choice(single, single_valid=1, single_ring_entries=2048, index_pass=1)
    assert name == "hsrans::k_decode<0, false>" and (info["grid"], info["waves_per_block"]) == (1, 1), (name, info)


def test_sub_runs_take_the_kernels_that_count_them():
    """a sharded decode's sub-runs in one launch (tests/test_gpu_parity.py asserts spread == 2 of such a launch)"""
    for (plan, begin), per_block, coded, kernel in ((FEW_LARGE, 8, True, "hsrans::k_decode_dealt<true, true>"), (FEW_LARGE, 8, False, "hsrans::k_decode_spread<3, true>"),
                                                    (MANY, 1, True, "hsrans::k_decode_grouped<3, true, true>"), (blocks(13, 1 << 30, 1 << 18, 16), 1, True, "hsrans::k_decode_grouped<4, true, true>")):
        free, _ = api.launch_choice(plan, **lean(plan, begin, per_block, coded_blocks_only=coded))
        name, info = api.launch_choice(plan, **lean(plan, begin, per_block, coded_blocks_only=coded, parts=1, n_parts=4))
        assert name == kernel and free != name, (name, info)
        assert info["lds_bytes"] <= LDS_LIMIT


def test_sub_runs_with_a_kernel_that_cannot_count_them_are_not_supported():
    plan, begin = FEW_LARGE
    with pytest.raises(NotImplementedError):  # groups that are not lean
        api.launch_choice(plan, **dict(lean(plan, begin, 8, parts=1, n_parts=4), groups_lean=0, spread_min_block=0, dealt=0))
    with pytest.raises(NotImplementedError):  # a plan without groups
        api.launch_choice(raw(11, 8192), persistent=1, table_mode=3, parts=1, n_parts=4)
    with pytest.raises(NotImplementedError):
        api.launch_choice(dict(plan, n_chains=92, n_pieces=92, interval=0), parts=1, n_parts=2)  # mt_ without an index


@pytest.mark.parametrize("n_parts", (0, 17))
def test_sub_runs_of_an_invalid_number_are_refused(n_parts):
    plan, begin = FEW_LARGE
    for coded in (True, False):
        with pytest.raises(ValueError):
            api.launch_choice(plan, **lean(plan, begin, 8, coded_blocks_only=coded, parts=1, n_parts=n_parts))
    api.launch_choice(plan, **lean(plan, begin, 8, parts=1, n_parts=16))  # (the most there can be)


def test_bad_arguments():
    with pytest.raises(H.HsransError):
        api.launch_choice(dict(container=H.RAW, states=48, bits=11, n_chains=1, n_pieces=1))
