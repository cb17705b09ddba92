"""Inputs at the two extremes of the stream's word rate (a plain module: numpy only, seeded, deterministic).

A rANS state takes a 16-bit word from the stream whenever the symbol it decoded had a small frequency: a symbol of frequency 1 of 2^bits
costs `bits` bits, so a lane that decodes such symbols takes a word in (nearly) every group; a symbol that holds (nearly) all of the
probability costs a small fraction of a bit, so the lanes that decode it take no word for groups on end (whole chains between two checkpoints
begin and end on one stream word).  The decode kernels move their stream cursors by arguments about how many words a group can take (the LDS
stream ring, the re-base once per 4 groups, the gather's non-storing skip, the producer/consumer ring of the one-chain kernel); these inputs
sit at both ends of that range and switch between them.

`hot_hist(bits)` is a histogram made by the caller (raw streams take one): count 1 for the symbols 0..254, the rest for 255.  Under it
`raw_hot` costs `bits` bits a byte, `raw_cold` next to nothing, and `raw_alternating` goes from one to the other at lengths that are no
multiple of anything.  block_ and mt_ streams make their histograms from the data: `mixed_blocks` is data whose own histograms come out
that way, block by block."""
from __future__ import annotations

import numpy as np

import hypersonic_rans_amd as H
from hypersonic_rans_amd import api

HOT_SYMBOLS = 255  # the symbols 0..254 of hot_hist; 255 is the cold one


def hot_hist(bits: int):
    counts = np.ones(256, np.int64)
    counts[255] = (1 << bits) - 255
    return api.hist_from_counts(counts)


def raw_hot(n: int, seed: int) -> np.ndarray:
    """bytes of 0..254 only: `bits` bits a byte under hot_hist(bits)"""
    return np.random.default_rng(seed).integers(0, HOT_SYMBOLS, n, dtype=np.uint8)


def raw_cold(n: int, seed: int) -> np.ndarray:
    """all 255, one byte in about 2000 another symbol: many groups on end without a word"""
    rng = np.random.default_rng(seed)
    d = np.full(n, 255, np.uint8)
    pos = np.nonzero(rng.random(n) < 1.0 / 2000)[0]
    d[pos] = rng.integers(0, HOT_SYMBOLS, pos.size, dtype=np.uint8)
    return d


def hot_stretches(n: int, seed: int) -> list:
    """the (begin, end) of raw_alternating's hot stretches: lengths 1..3000 at gaps 1..6000"""
    rng = np.random.default_rng(seed ^ 0x5EED)
    out, pos = [], 0
    while True:
        pos += int(rng.integers(1, 6001))
        length = int(rng.integers(1, 3001))
        if pos + length > n:
            return out
        out.append((pos, pos + length))
        pos += length


def raw_alternating(n: int, seed: int) -> np.ndarray:
    """raw_cold with hot stretches of random length at random gaps: idle to full rate and back inside one chain and across checkpoints"""
    d = raw_cold(n, seed)
    rng = np.random.default_rng(seed + 1)
    for b, e in hot_stretches(n, seed):
        d[b:e] = rng.integers(0, HOT_SYMBOLS, e - b, dtype=np.uint8)
    return d


RAW_KINDS = {"hot": raw_hot, "cold": raw_cold, "alternating": raw_alternating}


def raw_room(n: int) -> int:
    """room for a raw stream under hot_hist: the data expands (up to 15 bits a byte)"""
    return 2 * n + 4096


def encode_raw(kind: str, n: int, states: int, bits: int, seed: int, **index):
    """(data, what H.encode returns) of a raw input under hot_hist(bits); `index`: index_interval / index_groups"""
    d = RAW_KINDS[kind](n, seed)
    return d, H.encode(H.RAW, states, bits, d, hist=hot_hist(bits), out_capacity=raw_room(n), **index)


def mixed_stretch(k: int, length: int, block: int, bits: int):
    """(begin, end) of block k's hot stretch inside the block, or None where the block is too short for one"""
    r = max(1, block >> bits)
    if length < HOT_SYMBOLS * r:
        return None
    begin = (977 * k + 13) % (length - HOT_SYMBOLS * r + 1)
    return begin, begin + HOT_SYMBOLS * r


def mixed_blocks(n: int, block: int, bits: int, seed: int, fill_blocks=()) -> np.ndarray:
    """Data whose blocks of `block` bytes give block_/mt_ the extreme histogram: block k is its dominant symbol (37k + 5) & 255 but for one hot
    stretch that holds every other symbol r = max(1, block >> bits) times, shuffled: each of those normalises to frequency 1 (`bits` bits), the
    rest of the block costs next to nothing.  Blocks in `fill_blocks` (and a last block too short for a stretch) hold their symbol only."""
    rng = np.random.default_rng(seed)
    d = np.empty(n, np.uint8)
    r = max(1, block >> bits)
    for k, lo in enumerate(range(0, n, block)):
        length = min(block, n - lo)
        dominant = (37 * k + 5) & 255
        d[lo:lo + length] = dominant
        where = mixed_stretch(k, length, block, bits)
        if k in fill_blocks or where is None:
            continue
        others = np.repeat(np.delete(np.arange(256, dtype=np.uint8), dominant), r)
        rng.shuffle(others)
        d[lo + where[0]:lo + where[1]] = others
    return d


def mixed_hot_bytes(n: int, block: int, bits: int, fill_blocks=()) -> int:
    total = 0
    for k, lo in enumerate(range(0, n, block)):
        where = mixed_stretch(k, min(block, n - lo), block, bits)
        if k not in fill_blocks and where is not None:
            total += where[1] - where[0]
    return total


def equal_neighbours(plan) -> int:
    """pairs of adjacent pieces of a plan that begin at the same stream word: the chain between them took no word at all"""
    _, _, pieces = api.plan_tables(plan)
    w = pieces["words_off"]
    return int(np.count_nonzero(w[1:] == w[:-1]))
