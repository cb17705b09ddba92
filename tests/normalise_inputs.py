"""Blocks whose byte counts are DESIGNED to take the count normalisation (hist.cpp:103-199; hsrans_host.cpp normalize_counts; on the GPU
csrc/enc_normalise.h) through every depth of its heap sort, with and without a tie at the cut, and through many steal passes and charity
extractions (a plain module: numpy only, seeded, deterministic, no GPU).

The normalisation scales the 256 byte counts of a block to 2^bits, then repairs the rounding: too large a sum is taken back in "steal"
passes, too small a one handed out in "charity" passes, and the last pass of either stops part-way through the symbols sorted by count.
Which symbols lie before that cut is all the sort decides; where the counts on both sides of the cut are EQUAL, the order the reference's
heap sort happens to give equal counts decides the histogram.  A wrong tie gives counts that still sum to 2^bits and still decode.

`arith` restates the arithmetic (not the sort) to say what a histogram asks of the sort; it chooses inputs and proves coverage and never
checks a result.  The families below draw histograms; `blocks(bits, B)` keeps one block of bytes per distinct (kind, take, tie) class of a
setting, and `check_coverage` is the list of classes the settings together must reach."""
from __future__ import annotations

import functools

import numpy as np

# (bits, block size).  4160 = 65 * 64 is no power of two, so the scale factor rounds at every width (at 4096 and bits >= 12 it is an integer
# and nothing is ever adjusted); 4096 and 65536 only where the factor is a fraction.
# From 13 bits on a block of 4160 bytes cannot end its steal at take 0 or 1 (see _wanted_classes), and at 12 bits it cannot need 64 charity
# extractions (only counts of 33..64 round down, by less than 1/2 each, and 126 of them fill the block): those widths get a second, longer
# block size (a factor of 0.39, so rare symbols are floored to 1 as they are at 10 bits), with few draws.
WIDE = {12: 10432, 13: 20800, 14: 41600, 15: 83200}
SETTINGS = tuple((bits, 4160) for bits in range(10, 16)) + ((10, 4096), (11, 4096), (10, 65536)) + tuple(WIDE.items())
DRAWS = 1200  # per family and setting
RAW_BITS, RAW_CHARITY_TAKES = (10, 12, 15), (1, 2, 64)  # raw_subset: the widths the raw kernel is run at, the charity depths it gets there
BOUNDARY_TAKES = (2, 65, 66, 129, 130, 193, 194)  # besides "0 or 1": the extractions on either side of a change of extraction form


def scaled_counts(raw, size: int, bits: int) -> np.ndarray:
    """the counts before the repair: float32 scale, + 0.5, truncation to uint16, floor at 1 for a symbol that occurs (rows of `raw`)"""
    raw = np.asarray(raw, dtype=np.int64)
    factor = np.float32(1 << bits) / np.float32(size)
    c = ((raw.astype(np.float32) * factor).astype(np.float32) + np.float32(0.5)).astype(np.uint16).astype(np.int64)
    c[(c == 0) & (raw != 0)] = 1
    return c


def arith_many(raw, size: int, bits: int):
    """`arith` of every row of `raw` (N x 256): arrays kind (0 none, 1 steal, 2 charity), take, j_or_full, tie"""
    c = scaled_counts(np.atleast_2d(raw), size, bits)
    target = 1 << bits
    s = c.sum(axis=1)
    m = (c >= 2).sum(axis=1)
    kind = np.where(s == target, 0, np.where(s > target, 1, 2))
    # steal: pass j takes one from each of the m_j symbols with count >= j + 1 while more than m_j are missing
    e = np.where(kind == 1, s - target, 0)
    j = np.ones(len(c), np.int64)
    mj = m.copy()
    while True:
        more = e > mj
        if not more.any():
            break
        e = np.where(more, e - mj, e)
        j = np.where(more, j + 1, j)
        mj = np.where(more, (c >= (j + 1)[:, None]).sum(axis=1), mj)
    steal_take = mj - e
    # charity: the m symbols with count >= 2 each get full = (e - 1) / m, the e - full m largest one more
    ec = np.where(kind == 2, target - s, 1)
    full = (ec - 1) // np.maximum(m, 1)
    charity_take = ec - full * m
    take = np.where(kind == 1, steal_take, np.where(kind == 2, charity_take, 0))
    srt = -np.sort(-c, axis=1)
    rows = np.arange(len(c))
    inside = (take >= 1) & (take <= 255)
    tie = inside & (srt[rows, np.clip(take - 1, 0, 255)] == srt[rows, np.clip(take, 0, 255)])
    return kind, take, np.where(kind == 1, j, np.where(kind == 2, full, 0)), tie


KINDS = ("none", "steal", "charity")


def arith(raw, size: int, bits: int):
    """(kind, take, j_or_full, tie) of one histogram of `size` bytes: kind "none" (the scaled counts already sum to 2^bits), "steal" or
    "charity"; take = the entries the sort has to deliver; j = the steal passes, full = the whole charity rounds; tie = the sorted scaled
    counts at positions take - 1 and take are equal, so the sort's order of equal counts decides the histogram"""
    kind, take, jf, tie = arith_many(np.asarray(raw)[None, :], size, bits)
    return KINDS[int(kind[0])], int(take[0]), int(jf[0]), bool(tie[0])


# ---- histogram families: 256 raw counts that sum to `size`, on a random permutation of the symbols --------------------------------------
def _place(rng, counts) -> np.ndarray:
    raw = np.zeros(256, np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    raw[rng.permutation(256)[: counts.size]] = counts
    return raw


def dirichlet_multinomial(rng, size: int, bits: int) -> np.ndarray:
    """2..256 symbols, concentration 10^U(-1.5, 1.5)"""
    k = int(rng.integers(2, 257))
    alpha = 10.0 ** rng.uniform(-1.5, 1.5)
    p = rng.dirichlet(np.full(k, alpha))
    return _place(rng, rng.multinomial(size, p / p.sum()))


def _solve_last_level(size, fixed, n_last):
    """a value v >= 1 with fixed + n_last * v == size, or None"""
    rem = size - fixed
    if rem < n_last or rem % n_last:
        return None
    return rem // n_last


def few_level(rng, size: int, bits: int) -> np.ndarray:
    """1..3 distinct count values: runs of equal counts, so ties at most cuts"""
    while True:
        levels = int(rng.integers(1, 4))
        k = int(rng.integers(max(2, levels), 257))
        if levels == 1:
            divisors = [d for d in range(2, 257) if size % d == 0]
            k = int(rng.choice(divisors))
            return _place(rng, np.full(k, size // k))
        cuts = np.sort(rng.choice(np.arange(1, k), levels - 1, replace=False))
        n = np.diff(np.concatenate([[0], cuts, [k]]))
        top = max(2, 2 * size // k)
        start = rng.integers(1, top, levels - 1)
        for step in range(int(n[-1])):  # one of n_last consecutive values of the second-last level makes the last one whole
            vals = start.copy()
            vals[-1] += step
            v = _solve_last_level(size, int((n[:-1] * vals).sum()), int(n[-1]))
            if v is not None and v not in vals and len(set(vals.tolist())) == levels - 1:
                return _place(rng, np.repeat(np.concatenate([vals, [v]]), n))


def heavy_plus_singles(rng, size: int, bits: int) -> np.ndarray:
    """1..4 equal heavy symbols plus r symbols of count 1..3: scaled, the small ones are floored to 1 and many steal passes take it back"""
    while True:
        h = int(rng.integers(1, 5))
        r = int(rng.integers(0, 257 - h))
        small = rng.integers(1, int(rng.integers(1, 4)) + 1, r)
        extra = (size - int(small.sum())) % h
        if r + extra + h > 256 or int(small.sum()) + extra + h > size:
            continue
        small = np.concatenate([small, np.ones(extra, np.int64)])
        heavy = (size - int(small.sum())) // h
        return _place(rng, np.concatenate([np.full(h, heavy), small]))


def near_half(rng, size: int, bits: int) -> np.ndarray:
    """counts whose scaled value has a fractional part in [0.25, 0.5) (all rounded down: a large deficit) or in [0.5, 0.8) (all rounded up:
    a large surplus); one more symbol takes what is left of the block"""
    factor = float(1 << bits) / size
    lo, hi = ((0.25, 0.5), (0.5, 0.8))[int(rng.integers(0, 2))]
    k = int(rng.integers(2, 257))
    top = max(4, int(2.5 * size / k))
    r = np.arange(1, top + 1)
    frac = r * factor - np.floor(r * factor)
    cand = r[(frac >= lo) & (frac < hi)]
    if cand.size == 0:
        cand = r
    counts = rng.choice(cand, k - 1)
    while int(counts.sum()) >= size:
        counts = counts[: counts.size // 2]
    return _place(rng, np.concatenate([counts, [size - int(counts.sum())]]))


FAMILIES = (dirichlet_multinomial, few_level, heavy_plus_singles, near_half)


def tied_runs(rng, size: int, bits: int, takes, rows_each: int) -> np.ndarray:
    """The directed construction for a class the seeded families miss: for each wanted `take`, rows of n > take symbols of ONE count a — a
    run of equal counts that spans the cut, each rounding by the same amount, so the sum is off by about n times that amount —, w symbols of
    count 1, and one symbol with what is left of the block.  (rows_each * len(takes)) x 256 counts; the caller keeps the rows that `arith`
    puts in the class it wants."""
    take = np.repeat(np.asarray(takes, dtype=np.int64), rows_each)
    rows = take.size
    n = take + 1 + (rng.random(rows) * (256 - take - 1) * rng.random(rows)).astype(np.int64)  # (take + 1 .. 256, the short runs more often)
    w = np.where(rng.random(rows) < 0.4, 0, (rng.random(rows) * np.maximum(256 - n - 1, 0)).astype(np.int64))
    a = 1 + (rng.random(rows) * np.maximum((size - w) // n - 1, 0) * rng.random(rows)).astype(np.int64)
    rest = size - n * a - w
    cols = np.arange(256)[None, :]
    raw = np.where(cols < n[:, None], a[:, None], np.where(cols < (n + w)[:, None], 1, 0))
    good = (rest >= 0) & ((rest == 0) | (n + w <= 255))
    at = np.minimum(n + w, 255)
    raw[np.arange(rows), at] += np.where(good & (rest > 0), rest, 0)
    return rng.permuted(raw[good & (raw.sum(axis=1) == size)], axis=1)


def _shuffled_block(rng, raw) -> np.ndarray:
    block = np.repeat(np.arange(256, dtype=np.uint8), raw)
    rng.shuffle(block)
    return block


class Designed:
    """the blocks of one setting: `data[k]` (bytes), `raw[k]` (its counts), `info[k]` = arith of it; the last block is the short one"""

    def __init__(self, bits, size, data, raw, info):
        self.bits, self.size, self.data, self.raw, self.info = bits, size, data, raw, info

    def concatenated(self) -> np.ndarray:
        return np.concatenate(self.data)

    def pick(self, kind, take=None, tie=None, best=None):
        """index of a whole block of that class (best = "j": the one with the largest j_or_full; "take": the largest take), or None"""
        hits = [k for k, i in enumerate(self.info[:-1]) if i[0] == kind and (take is None or i[1] == take) and (tie is None or i[3] == tie)]
        if not hits:
            return None
        if best == "j":
            return max(hits, key=lambda k: (self.info[k][2], -k))
        if best == "take":
            return max(hits, key=lambda k: (self.info[k][1], -k))
        return hits[0]


def _wanted_classes(bits: int, size: int):
    """(kind, take, tie or None) a setting holds whatever the draws gave (see check_coverage): made by tied_runs where they are missing.
    Every width has a tied cut on either side of each change of extraction form; one setting has every steal depth, one every charity depth.
    A block of 4160 bytes ends its steal at take 0 or 1 at 10..12 bits only.  From 13 bits on it scales by 1.97 or more, so every symbol that
    occurs has a count >= 2 and is one of the m that can give, none is floored to 1, and each adds less than 1/2 to the sum by its rounding:
    the surplus e is at most m / 2, there is one steal pass, and it spares take = m - e >= m / 2 symbols.  take = 1 needs m = 2 and e = 1;
    two EQUAL counts have an even sum, 2^bits is even, so e is even; two unequal ones would both have to round up by exactly 1/2, and
    128 a / 65 is never a whole number and a half.  Those widths have the WIDE block sizes for it."""
    wanted = []
    if size == 4160:
        wanted += [("steal", t, True) for t in ((1,) if bits <= 12 else ()) + BOUNDARY_TAKES]
    if bits in RAW_BITS and size == WIDE.get(bits, 4160):
        wanted += [("charity", t, None) for t in RAW_CHARITY_TAKES]
    if WIDE.get(bits) == size:
        wanted += [("steal", 0, None), ("steal", 1, True), ("steal", 1, False), ("steal", 2, True)]
    if (bits, size) == (13, 4160):
        wanted += [("steal", t, None) for t in range(0, 249)]
    if (bits, size) == (11, 4160):
        wanted += [("charity", t, None) for t in range(1, 101)]
    return wanted


@functools.lru_cache(maxsize=None)
def blocks(bits: int, size: int) -> Designed:
    """One shuffled block of `size` bytes per distinct (kind, take, tie) class the families reach at this setting — of the draws of a steal
    class the one with the most passes — plus further blocks whose scaled counts already sum to 2^bits, blocks of exactly 2 and exactly 256
    symbols, the directed constructions, and a short last block of size // 2 + 7 bytes."""
    rng = np.random.default_rng([bits, size, 0x4E4F524D])
    draws = DRAWS if size <= 4160 else DRAWS // 4 if size == 65536 else DRAWS // 40  # (a 64 KiB block costs 16 times a 4 KiB one to code)
    raws = np.stack([family(rng, size, bits) for family in FAMILIES for _ in range(draws)])
    assert (raws.sum(axis=1) == size).all() and (raws >= 0).all()
    kind, take, jf, tie = arith_many(raws, size, bits)
    symbols = (raws != 0).sum(axis=1)
    chosen = {}
    for k in range(len(raws)):
        key = (KINDS[kind[k]], int(take[k]), bool(tie[k]))
        if key not in chosen or (kind[k] == 1 and jf[k] > jf[chosen[key]]):
            chosen[key] = k
    extras = list(np.nonzero(kind == 0)[0][:4]) + list(np.nonzero(symbols == 2)[0][:2]) + list(np.nonzero(symbols == 256)[0][:2])
    keep = list(dict.fromkeys(sorted(chosen.values()) + [int(k) for k in extras]))
    out_raw = [raws[k] for k in keep]

    def missing():
        return [w for w in _wanted_classes(bits, size) if not any(c[0] == w[0] and c[1] == w[1] and w[2] in (None, c[2]) for c in chosen)]

    for _ in range(3):
        lacking = missing()
        if not lacking:
            break
        made = tied_runs(rng, size, bits, [w[1] for w in lacking], 3000)
        mk, mt, _, mtie = arith_many(made, size, bits)
        for k in range(len(made)):
            key = (KINDS[mk[k]], int(mt[k]), bool(mtie[k]))
            if key not in chosen and any(w[0] == key[0] and w[1] == key[1] and w[2] in (None, key[2]) for w in lacking):
                chosen[key] = -1
                out_raw.append(made[k])
    data = [_shuffled_block(rng, r) for r in out_raw]
    short = size // 2 + 7
    out_raw.append(_place(rng, rng.multinomial(short, rng.dirichlet(np.full(200, 0.5)))))
    data.append(_shuffled_block(rng, out_raw[-1]))
    info = [arith(r, int(r.sum()), bits) for r in out_raw]
    return Designed(bits, size, data, out_raw, info)


def all_settings():
    return [blocks(bits, size) for bits, size in SETTINGS]


def check_coverage() -> dict:
    """Asserts, on `arith` alone, that the designed blocks reach what the tests claim to reach; returns the census."""
    steal, charity = set(), set()
    none_blocks, two, full = 0, 0, 0
    by_bits = {}
    for d in all_settings():
        for raw, (kind, take, jf, tie) in zip(d.raw[:-1], d.info[:-1]):
            assert int(raw.sum()) == d.size
            if kind == "steal":
                steal.add(take)
                by_bits.setdefault(d.bits, []).append((take, jf, tie))
            elif kind == "charity":
                charity.add(take)
            else:
                none_blocks += 1
            n = int((raw != 0).sum())
            two += n == 2
            full += n == 256
    missing = [t for t in range(0, 249) if t not in steal]
    assert not missing, f"steal takes never reached: {missing}"
    assert any(t >= 252 for t in steal), sorted(steal)[-3:]
    missing = [t for t in range(1, 101) if t not in charity]
    assert not missing, f"charity takes never reached: {missing}"
    for bits in range(10, 16):
        seen = by_bits.get(bits, [])
        tied = {t for t, _, tie in seen if tie}
        untied = {t for t, _, tie in seen if not tie}
        assert 1 in tied, (bits, "no tied cut at take 1")
        assert 0 in untied or 1 in untied, bits
        lacking = [t for t in BOUNDARY_TAKES if t not in tied]
        assert not lacking, (bits, "boundary takes without a tied cut", lacking)
        both = [t for t in (1,) + BOUNDARY_TAKES if t in untied or (t == 1 and 0 in untied)]
        assert len(both) >= 4, (bits, "boundary takes with an untied cut too", both)
    for bits in (10, 11, 12):
        assert any(jf >= 2 and take > 0 and tie for take, jf, tie in by_bits[bits]), (bits, "no tied cut after several steal passes")
    assert any(jf >= 16 and take > 0 and tie for take, jf, tie in by_bits[10]), "no tied cut after 16 steal passes at 10 bits"
    assert none_blocks >= 10 and two >= 1 and full >= 1, (none_blocks, two, full)
    return {"steal": steal, "charity": charity, "none": none_blocks, "two": two, "full": full,
            "max_j": max(jf for seen in by_bits.values() for _, jf, _ in seen), "blocks": sum(len(d.data) for d in all_settings())}


# ---- subsets: the blocks that go to the recorded reference, and the ones the one-wavefront raw kernel gets one launch each ----------------
def boundary_picks(d: Designed, both: bool = True) -> list:
    """indices of d's steal blocks at takes 0, 1 and BOUNDARY_TAKES: the tied one and (with `both`) the untied one, where d has them"""
    out = []
    for take in (0, 1) + BOUNDARY_TAKES:
        ties = (True, False) if both else ((True,) if d.pick("steal", take, True) is not None else (False,))
        out += [d.pick("steal", take, tie) for tie in ties]
    return [k for k in out if k is not None]


def extreme_picks(d: Designed) -> list:
    """the most steal passes, the deepest steal, the deepest charity, the most whole charity rounds, and a block that needs no repair"""
    out = [d.pick("steal", best="j"), d.pick("steal", best="take"), d.pick("charity", best="take"), d.pick("charity", best="j"), d.pick("none")]
    return [k for k in out if k is not None]


def reference_subset() -> list:
    """(bits, block) of every setting's boundary and extreme blocks: what tests/golden/make_golden.py asks the real reference about"""
    out = []
    for d in all_settings():
        for k in dict.fromkeys(boundary_picks(d) + extreme_picks(d)):
            out.append((d.bits, d.data[k]))
    assert len(out) <= 300, len(out)
    return out


def raw_subset(bits: int) -> list:
    """(block, info) for the raw kernel (its own heap build, in registers): the steal boundary takes, charity takes 1, 2, 64 and the largest,
    the most steal passes, one block that needs no repair — from the 4160-byte setting, and the wide one where it has what that one lacks"""
    out, seen = [], set()
    for d in [blocks(bits, 4160)] + ([blocks(bits, WIDE[bits])] if bits in WIDE else []):
        picks = boundary_picks(d, both=False) + [d.pick("charity", t) for t in RAW_CHARITY_TAKES] + [d.pick("charity", best="take"), d.pick("steal", best="j"), d.pick("none")]
        for k in picks:
            if k is not None and d.info[k][:2] + d.info[k][3:] not in seen:
                seen.add(d.info[k][:2] + d.info[k][3:])
                out.append((d.data[k], d.info[k]))
    return out


def describe(d: Designed, k: int) -> str:
    kind, take, jf, tie = d.info[k]
    return f"block {k} of setting bits={d.bits} B={d.size}: {kind} take={take} {'j' if kind == 'steal' else 'full'}={jf} {'TIED' if tie else 'untied'} cut, {int((d.raw[k] != 0).sum())} symbols"


HUGE = (1 << 25) + 64


@functools.lru_cache(maxsize=None)
def huge_block() -> np.ndarray:
    """One block of 2^25 + 64 bytes, where (float)count is no longer exact: an odd dominant count above 2^24 (float32 rounds it to a multiple
    of 2) and 255 symbols on two levels, each count of which float32 still holds exactly; shuffled in runs of 64 bytes (a full shuffle of 32 MiB
    costs more than everything else the test does)."""
    rng = np.random.default_rng(0x4855_4745)
    dominant = (1 << 24) + 4_000_001
    rest = HUGE - dominant
    low = 50_001
    while (rest - 127 * low) % 128:
        low += 1
    raw = _place(rng, [dominant] + [(rest - 127 * low) // 128] * 128 + [low] * 127)
    assert int(raw.sum()) == HUGE and HUGE % 64 == 0
    runs = np.repeat(np.arange(256, dtype=np.uint8), raw).reshape(-1, 64)
    return runs[rng.permutation(len(runs))].reshape(-1)
