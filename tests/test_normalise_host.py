"""The host library's count normalisation (hsrans_host.cpp normalize_counts) on histograms DESIGNED for it (normalise_inputs.py): every
depth of the reference's heap sort with and without a tie at the cut, many steal passes, deep charity.  Against the plain-C oracle on every
block; against the real reference's recorded make_hist on the boundary and extreme blocks."""
import numpy as np
import pytest

import hypersonic_rans_amd as H
import normalise_inputs as N


def test_designed_blocks_reach_what_they_claim():
    """on the arithmetic alone, before any result is looked at: every steal depth 0..248 and one >= 252, every charity depth 1..100, a tied
    cut on either side of each change of extraction form at every width, tied cuts after several (and after 16) steal passes, blocks that
    need no repair, blocks of 2 and of 256 symbols"""
    census = N.check_coverage()
    assert census["max_j"] >= 52 and census["blocks"] >= 3000, census


@pytest.mark.parametrize("bits,size", N.SETTINGS)
def test_host_histograms_are_the_oracles(oracle, bits, size):
    d = N.blocks(bits, size)
    for k, block in enumerate(d.data):
        got = np.asarray(H.make_hist(block, bits).symbolCount, dtype=np.int64)
        want = np.asarray(oracle.make_hist(block, bits).symbolCount, dtype=np.int64)
        assert np.array_equal(got, want), (N.describe(d, k), np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
        assert int(got.sum()) == 1 << bits, N.describe(d, k)
        assert (got[d.raw[k] != 0] >= 1).all() and (got[d.raw[k] == 0] == 0).all(), N.describe(d, k)


def test_host_histograms_are_the_real_references(ref):
    subset = N.reference_subset()
    assert 100 <= len(subset) <= 300
    for bits, block in subset:
        want, _ = ref.make_hist(block, bits)
        got = np.asarray(H.make_hist(block, bits).symbolCount, dtype=np.uint16)
        assert np.array_equal(got, want), (bits, N.arith(np.bincount(block, minlength=256), block.size, bits))
