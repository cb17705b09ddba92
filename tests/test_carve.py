"""csrc/hsrans_carve.h on its own: the overlap rule of the batch entries (spans_disjoint) and the layout carver (Carve, up256) that every
entry packing many parts into one buffer uses.  A stand-alone program, compiled by the host compiler with nothing but that header (so the
header needs no HIP), checks on seeded random cases

  1. spans_disjoint against an all-pairs check of the stated rule (false exactly when two non-empty spans intersect and at least one of them
     is a write), up to 12 spans in a 64-byte address range so that touching, nested, identical and empty spans all occur;
  2. the same against the rule as hsrans_encode_device_batch stated it before the rule had one home: the outputs pairwise, then every
     input against every output (non-empty spans only) — written out here, not taken from the library;
  3. Carve::take / close at 256 against off_k = off_{k-1} + up256(size_{k-1}), and mixed alignments (16, 256, 512) against align_up by hand.

The program runs under AddressSanitizer and UBSan where the host compiler has them (it loads nothing into Python)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hypersonic_rans_amd", "csrc")

PROGRAM = r"""
#include "hsrans_carve.h"

#include <stdio.h>

static uint64_t rng_state;
static uint32_t rnd(uint32_t n) // [0, n)
{
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 11) % n);
}

static bool meet(const Span &a, const Span &b) { return a.lo < a.hi && b.lo < b.hi && a.lo < b.hi && b.lo < a.hi; }

// the rule, pair by pair
static bool rule_all_pairs(const std::vector<Span> &s)
{
  for (size_t i = 0; i < s.size(); i++)
    for (size_t j = i + 1; j < s.size(); j++)
      if (meet(s[i], s[j]) && (s[i].write || s[j].write))
        return false;
  return true;
}

// the encoders' rule as it was stated per entry: no two outputs overlap, no output overlaps an input
static bool rule_outputs_then_inputs(const std::vector<Span> &outs, const std::vector<Span> &ins)
{
  for (size_t i = 0; i < outs.size(); i++)
    for (size_t j = i + 1; j < outs.size(); j++)
      if (outs[i].lo < outs[j].hi && outs[j].lo < outs[i].hi)
        return false;
  for (const Span &in : ins)
    for (const Span &out : outs)
      if (in.lo < out.hi && out.lo < in.hi)
        return false;
  return true;
}

static Span random_span(bool may_be_empty, bool write)
{
  const uint32_t lo = rnd(64), len = may_be_empty ? rnd(64 - lo + 1) : 1 + rnd(64 - lo);
  return Span{(uintptr_t)lo, (uintptr_t)(lo + len), write};
}

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int main()
{
  rng_state = 0x9E3779B97F4A7C15ull;
  // 1. against the rule over all pairs
  unsigned refused = 0, accepted = 0, touching = 0, nested = 0, identical = 0, empty = 0, shared_reads = 0;
  for (int c = 0; c < 6000; c++)
  {
    std::vector<Span> s(rnd(13));
    for (Span &sp : s)
      sp = random_span(true, rnd(3) == 0);
    for (size_t i = 0; i < s.size(); i++)
    {
      empty += s[i].lo == s[i].hi;
      for (size_t j = i + 1; j < s.size(); j++)
      {
        touching += s[i].lo < s[i].hi && s[j].lo < s[j].hi && (s[i].hi == s[j].lo || s[j].hi == s[i].lo);
        identical += s[i].lo < s[i].hi && s[i].lo == s[j].lo && s[i].hi == s[j].hi;
        nested += meet(s[i], s[j]) && ((s[i].lo < s[j].lo && s[j].hi < s[i].hi) || (s[j].lo < s[i].lo && s[i].hi < s[j].hi));
        shared_reads += meet(s[i], s[j]) && !s[i].write && !s[j].write;
      }
    }
    const bool want = rule_all_pairs(s);
    std::vector<Span> sorted = s;
    const bool got = spans_disjoint(sorted);
    if (got != want || sorted.size() != s.size())
    {
      printf("case %d: spans_disjoint says %d, the rule %d\n", c, (int)got, (int)want);
      for (const Span &sp : s)
        printf("  [%u, %u) %s\n", (unsigned)sp.lo, (unsigned)sp.hi, sp.write ? "write" : "read");
      return 1;
    }
    (want ? accepted : refused)++;
  }
  if (refused < 500 || accepted < 500 || !touching || !nested || !identical || !empty || !shared_reads)
  {
    printf("the generator misses a kind of case: refused %u accepted %u touching %u nested %u identical %u empty %u shared reads %u\n", refused, accepted, touching,
           nested, identical, empty, shared_reads);
    return 1;
  }
  printf("rule: %u refused, %u accepted (touching %u, nested %u, identical %u, empty %u, reads sharing %u)\n", refused, accepted, touching, nested, identical, empty,
         shared_reads);

  // 2. against the encoders' rule as stated per entry, non-empty spans
  unsigned refused2 = 0, accepted2 = 0;
  for (int c = 0; c < 6000; c++)
  {
    const uint32_t members = 1 + rnd(6);
    std::vector<Span> outs, ins, all;
    for (uint32_t k = 0; k < members; k++)
    {
      outs.push_back(random_span(false, true));
      ins.push_back(random_span(false, false));
      if (rnd(4) == 0)
        outs.back().hi = outs.back().lo + 1 + rnd(3); // (short outputs: more batches that pass)
      all.push_back(outs.back());
      all.push_back(ins.back());
    }
    const bool want = rule_outputs_then_inputs(outs, ins);
    if (spans_disjoint(all) != want)
    {
      printf("case %d of the encoders' rule: spans_disjoint says %d, the rule %d\n", c, (int)!want, (int)want);
      return 1;
    }
    (want ? accepted2 : refused2)++;
  }
  if (refused2 < 300 || accepted2 < 300)
  {
    printf("the encoders' generator is lopsided: refused %u accepted %u\n", refused2, accepted2);
    return 1;
  }
  printf("encoders' rule: %u refused, %u accepted\n", refused2, accepted2);

  // 3. the carver
  for (size_t v = 0; v < 5000; v++)
    if (up256(v) != (v + 255) / 256 * 256 || up16(v) != (v + 15) / 16 * 16)
    {
      printf("up256 / up16 of %zu\n", v);
      return 1;
    }
  for (int c = 0; c < 4000; c++)
  {
    const uint32_t n = 1 + rnd(10);
    Carve a, b;
    size_t closed = 0, by_hand = 0; // the closed form at 256; the cursor of the mixed alignments
    for (uint32_t k = 0; k < n; k++)
    {
      const size_t size = rnd(4) == 0 ? 0 : rnd(3) == 0 ? 256 * (size_t)rnd(20) : rnd(5000);
      if (a.take(size) != closed || a.at != closed + size)
      {
        printf("case %d: region %u at 256\n", c, k);
        return 1;
      }
      closed += up256(size);
      const size_t align = rnd(3) == 0 ? 16 : rnd(2) ? 256 : 512, here = align_up(by_hand, align);
      if (b.take(size, align) != here || b.at != here + size)
      {
        printf("case %d: region %u at %zu\n", c, k, align);
        return 1;
      }
      by_hand = here + size;
    }
    const size_t last = rnd(2) ? 256 : 512;
    if (a.close() != closed || a.at != closed || a.close() != closed || b.close(last) != align_up(by_hand, last))
    {
      printf("case %d: close\n", c);
      return 1;
    }
  }
  printf("carve ok\n");
  return 0;
}
"""


def test_overlap_rule_and_layout_carver(tmp_path):
    src = tmp_path / "carve_check.cpp"
    exe = tmp_path / "carve_check"
    src.write_text(PROGRAM)
    base = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:  # a host compiler without the sanitizer runtimes: the same program, plain
        r = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert r.returncode == 0 and r.stdout.rstrip().endswith("carve ok"), (r.stdout[-2000:], r.stderr[-3000:])


def _sources():
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".cpp", ".h", ".hip")):
            with open(os.path.join(CSRC, name)) as f:
                yield name, f.read()


def test_one_rounding_one_carver_one_overlap_rule():
    """What hsrans_carve.h replaced stays replaced: one definition of up256, no rounding to 256 spelled out elsewhere, no local take, and no
    overlap check of a batch file's own."""
    import re

    definitions = [name for name, text in _sources() if re.search(r"\bup256\s*(=\s*\[|\(size_t \w+\)\s*\{)", text)]
    assert definitions == ["hsrans_carve.h"], definitions
    for name, text in _sources():
        if name == "hsrans_carve.h":
            continue
        assert "+ 255) & ~" not in text and "/ 256 * 256" not in text, name
        assert not re.search(r"\btake\s*=\s*\[|\bsize_t take\(", text), name
        if "batch" in name:
            assert not re.search(r"\branges_disjoint\b|\bdisjoint\(|bool spans_disjoint", text), name
