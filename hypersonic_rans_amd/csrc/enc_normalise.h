// enc_normalise.h — the reference's count normalisation on one wavefront: the heap sort replayed in registers, adjust_counts.
// Part of the one encoder translation unit hsrans_encode.hip (which includes the parts in dependency order and holds the launchers).
#ifndef HSRANS_ENC_NORMALISE_H
#define HSRANS_ENC_NORMALISE_H

namespace hsrans
{
namespace
{

// ---- hist.cpp:16-215: the heap sort ---------------------------------------------------------------------------------
// The reference sorts the symbols by count with a textbook heap sort; the order of EQUAL counts that sort happens to
// produce decides which symbols are adjusted, so the sort is replayed exactly (hsrans_host.cpp heap_sift) — but as
// wave-uniform code: the heap lives in five registers by tree level (entries count << 8 | symbol),
//   A: nodes 0..62 (levels 0-5, lane = node), B: 63..126 (level 6), C: 127..190, D: 191..254 (level 7), E: node 255,
// read with v_readlane and written with a one-lane select, all control flow scalar.  ~4x faster than one lane walking LDS.
struct Heap
{
  uint32_t A, B, C, D, E;
};

// one lane of a register takes a wave-uniform value (v_cmp + v_cndmask: as cheap as v_writelane through M0, and the
// compiler keeps track of the hazards)
__device__ __forceinline__ uint32_t write_lane(uint32_t value, uint32_t lane, uint32_t reg) { return lane_id() == lane ? value : reg; }

template <int LEVEL>
__device__ __forceinline__ uint32_t heap_get(const Heap &h, uint32_t i)
{
  if constexpr (LEVEL <= 5)
    return __builtin_amdgcn_readlane(h.A, i);
  else if constexpr (LEVEL == 6)
    return __builtin_amdgcn_readlane(h.B, i - 63);
  else if constexpr (LEVEL == 7)
    return i < 191 ? __builtin_amdgcn_readlane(h.C, i - 127) : __builtin_amdgcn_readlane(h.D, i - 191);
  else
    return h.E;
}

template <int LEVEL>
__device__ __forceinline__ void heap_set(Heap &h, uint32_t i, uint32_t v)
{
  if constexpr (LEVEL <= 5)
    h.A = write_lane(v, i, h.A);
  else if constexpr (LEVEL == 6)
    h.B = write_lane(v, i - 63, h.B);
  else if constexpr (LEVEL == 7)
  {
    if (i < 191)
      h.C = write_lane(v, i - 127, h.C);
    else
      h.D = write_lane(v, i - 191, h.D);
  }
  else
    h.E = v;
}

// `val` belongs at node `root` (on level LEVEL) or below it; n = heap size
template <int LEVEL>
__device__ __forceinline__ void heap_sift(Heap &h, uint32_t root, uint32_t n, uint32_t val)
{
  if constexpr (LEVEL == 8)
    heap_set<8>(h, root, val);
  else
  {
    const uint32_t l = 2 * root + 1;
    if (l >= n)
    {
      heap_set<LEVEL>(h, root, val);
      return;
    }
    uint32_t big = l;
    uint32_t vb = heap_get<LEVEL + 1>(h, l);
    if constexpr (LEVEL + 1 < 8)
      if (l + 1 < n)
      {
        const uint32_t ar = heap_get<LEVEL + 1>(h, l + 1);
        if ((ar >> 8) > (vb >> 8)) // the right child only wins when strictly larger
        {
          big = l + 1;
          vb = ar;
        }
      }
    if ((vb >> 8) > (val >> 8))
    {
      heap_set<LEVEL>(h, root, vb);
      heap_sift<LEVEL + 1>(h, big, n, val);
    }
    else
      heap_set<LEVEL>(h, root, val);
  }
}

template <int LEVEL>
__device__ __forceinline__ void heap_build_level(Heap &h, uint32_t first, uint32_t last)
{
  for (uint32_t i = last + 1; i-- > first;)
    heap_sift<LEVEL>(h, i, 256, heap_get<LEVEL>(h, i));
}

// ---- the extraction as straight-line scalar code -----------------------------------------------------------------------------
// One extraction is one sift of the heap's last entry down from the root, every step depends on the one before, and the wavefront
// pays about 2.3 ns per instruction whatever it is (tools/microbench/lone_wave.hip) — so this is written for its instruction count
// (the compiler's form of heap_sift<> above spends 22-24 instructions a level).  Bottom-up: walk down the path of the larger
// children to its end WITHOUT looking at the entry to place (8 instructions a level: two v_readlane, "right wins only when its
// count is strictly larger" as one s_or + s_cmp on count << 8 | symbol, two s_cselect), then find from the bottom where the entry
// belongs (it came from the bottom: usually one compare), then move the path up by one (s_mov m0 + v_writelane per level).
// Same heap as heap_sift<0>: the counts along the path never grow, so "the first node whose larger child is not larger than the
// entry" is found from either end.  Lanes: A holds nodes 0..62 (lane = node), B nodes 63..126 (lane = node - 63), C 127..190,
// D 191..254; cK = lane of the path's node on level K (level 7: 0..63 in C, 64..127 in D), bK = that node's entry.
#define HSRANS_HEAP_PICK_AT(REG, L, R, BN, CN) /* children at lanes L, R of REG: the larger one's entry -> BN, its lane -> CN */                    \
  "v_readlane_b32 %[sl], " REG ", " L "\n\t"                                                                                                      \
  "v_readlane_b32 %[sr], " REG ", " R "\n\t"                                                                                                      \
  "s_or_b32 " BN ", %[sl], 0xff\n\t"                                                                                                              \
  "s_cmp_gt_u32 %[sr], " BN "\n\t"                                                                                                                \
  "s_cselect_b32 " BN ", %[sr], %[sl]\n\t"                                                                                                        \
  "s_cselect_b32 " CN ", " R ", " L "\n\t"
#define HSRANS_HEAP_PICK(REG, BN, CN) HSRANS_HEAP_PICK_AT(REG, "%[l]", "%[r]", BN, CN)
#define HSRANS_HEAP_DOWN_A(CK, BN, CN) /* node at lane CK of A (levels 1..4): children at lanes 2 CK + 1, 2 CK + 2 of A */                        \
  "s_lshl1_add_u32 %[l], " CK ", 1\n\t"                                                                                                           \
  "s_add_u32 %[r], %[l], 1\n\t" HSRANS_HEAP_PICK("%[A]", BN, CN)
#define HSRANS_HEAP_HEAD /* the entry's compare key, levels 0..4 */                                                                           \
  "s_or_b32 %[vmax], %[val], 0xff\n\t" HSRANS_HEAP_PICK_AT("%[A]", "1", "2", "%[b1]", "%[c1]") HSRANS_HEAP_DOWN_A("%[c1]", "%[b2]", "%[c2]")         \
      HSRANS_HEAP_DOWN_A("%[c2]", "%[b3]", "%[c3]") HSRANS_HEAP_DOWN_A("%[c3]", "%[b4]", "%[c4]") HSRANS_HEAP_DOWN_A("%[c4]", "%[b5]", "%[c5]")
#define HSRANS_HEAP_CLIMB_FROM(K, BK, BNEXT, LOWER) /* the path ends on level K: does the entry go there? (else try level K - 1) */                \
  "bottom" K "_%=:\n\t"                                                                                                                           \
  "s_cmp_gt_u32 " BK ", %[vmax]\n\t"                                                                                                              \
  "s_cbranch_scc0 " LOWER "_%=\n\t"                                                                                                               \
  "s_mov_b32 " BNEXT ", %[val]\n\t"                                                                                                               \
  "s_branch w" K "_%=\n\t"
#define HSRANS_HEAP_WRITE_A(K, CK, BNEXT) "w" K "_%=:\n\ts_mov_b32 m0, " CK "\n\tv_writelane_b32 %[A], " BNEXT ", m0\n\t"
#define HSRANS_HEAP_WRITES /* levels 5 .. 0 take the entry of the level below (or the entry to place) */                                          \
  HSRANS_HEAP_WRITE_A("5", "%[c5]", "%[b6]") HSRANS_HEAP_WRITE_A("4", "%[c4]", "%[b5]") HSRANS_HEAP_WRITE_A("3", "%[c3]", "%[b4]")                \
  HSRANS_HEAP_WRITE_A("2", "%[c2]", "%[b3]") HSRANS_HEAP_WRITE_A("1", "%[c1]", "%[b2]")                                                           \
  "w0_%=:\n\tv_writelane_b32 %[A], %[b1], 0\n\t"                                                                                                  \
  "s_branch done_%=\n\t"
#define HSRANS_HEAP_CLIMBS /* the rarer ends of the climb */                                                                                       \
  HSRANS_HEAP_CLIMB_FROM("5", "%[b5]", "%[b6]", "bottom4") HSRANS_HEAP_CLIMB_FROM("4", "%[b4]", "%[b5]", "bottom3")                               \
  HSRANS_HEAP_CLIMB_FROM("3", "%[b3]", "%[b4]", "bottom2") HSRANS_HEAP_CLIMB_FROM("2", "%[b2]", "%[b3]", "bottom1")                               \
  HSRANS_HEAP_CLIMB_FROM("1", "%[b1]", "%[b2]", "bottom0")                                                                                        \
  "bottom0_%=:\n\t"                                                                                                                               \
  "s_mov_b32 %[b1], %[val]\n\t"                                                                                                                   \
  "s_branch w0_%=\n\t"                                                                                                                            \
  "done_%=:"
struct HeapScratch // (scalar temporaries of one extraction; the register allocator places them)
{
  uint32_t vmax, l, r, sl, sr, c1, c2, c3, c4, c5, c6, c7, b1, b2, b3, b4, b5, b6, b7;
};
#define HSRANS_HEAP_OPERANDS                                                                                                                       \
  [A] "+v"(h.A), [B] "+v"(h.B), [C] "+v"(h.C), [D] "+v"(h.D), [vmax] "=&s"(t.vmax), [l] "=&s"(t.l), [r] "=&s"(t.r), [sl] "=&s"(t.sl), \
      [sr] "=&s"(t.sr), [c1] "=&s"(t.c1), [c2] "=&s"(t.c2), [c3] "=&s"(t.c3), [c4] "=&s"(t.c4), [c5] "=&s"(t.c5), [c6] "=&s"(t.c6), [c7] "=&s"(t.c7),  \
      [b1] "=&s"(t.b1), [b2] "=&s"(t.b2), [b3] "=&s"(t.b3), [b4] "=&s"(t.b4), [b5] "=&s"(t.b5), [b6] "=&s"(t.b6), [b7] "=&s"(t.b7)

// heap of n entries, 127 <= n <= 255 (levels 0..6 whole, level 7 up to node n - 1): the maximum leaves, `val` (the entry that was at
// node n) is sifted down from the root
__device__ __forceinline__ void heap_extract_high(Heap &h, uint32_t n, uint32_t val)
{
  HeapScratch t;
  const uint32_t n7 = n - 127; // nodes of level 7 in the heap: their lanes in C / D (as 0..127) are below this
  asm volatile(HSRANS_HEAP_HEAD
               // level 5 (A, nodes 31..62) -> level 6 (B): children at lanes 2 c - 62, 2 c - 61
               "s_lshl1_add_u32 %[l], %[c5], -62\n\t"
               "s_add_u32 %[r], %[l], 1\n\t" HSRANS_HEAP_PICK("%[B]", "%[b6]", "%[c6]")
               // level 6 (B, lane c) -> level 7: children are level-7 entries 2 c and 2 c + 1 (C: 0..63, D: 64..127), if still in the heap
               "s_lshl_b32 %[l], %[c6], 1\n\t"
               "s_cmp_ge_u32 %[l], %[n7]\n\t"
               "s_cbranch_scc1 bottom6_%=\n\t"
               "s_add_u32 %[r], %[l], 1\n\t"
               "s_cmp_lt_u32 %[c6], 32\n\t"
               "s_cbranch_scc0 fromD_%=\n\t"
               "v_readlane_b32 %[sl], %[C], %[l]\n\t"
               "v_readlane_b32 %[sr], %[C], %[r]\n\t"
               "s_branch pick7_%=\n\t"
               "fromD_%=:\n\t"
               "s_sub_u32 %[b7], %[l], 64\n\t"
               "v_readlane_b32 %[sl], %[D], %[b7]\n\t"
               "s_add_u32 %[b7], %[b7], 1\n\t"
               "v_readlane_b32 %[sr], %[D], %[b7]\n\t"
               "pick7_%=:\n\t"
               "s_cmp_lt_u32 %[r], %[n7]\n\t" // the right child may already be out of the heap: then it never wins
               "s_cselect_b32 %[sr], %[sr], 0\n\t"
               "s_or_b32 %[b7], %[sl], 0xff\n\t"
               "s_cmp_gt_u32 %[sr], %[b7]\n\t"
               "s_cselect_b32 %[b7], %[sr], %[sl]\n\t"
               "s_cselect_b32 %[c7], %[r], %[l]\n\t"
               // the path ends on level 7: the common case first, straight down through the writes
               "s_cmp_gt_u32 %[b7], %[vmax]\n\t"
               "s_cbranch_scc0 bottom6_%=\n\t"
               "s_cmp_lt_u32 %[c7], 64\n\t"
               "s_cbranch_scc1 w7C_%=\n\t"
               "s_sub_u32 m0, %[c7], 64\n\t"
               "v_writelane_b32 %[D], %[val], m0\n\t"
               "s_branch w6_%=\n\t"
               "w7C_%=:\n\t"
               "s_mov_b32 m0, %[c7]\n\t"
               "v_writelane_b32 %[C], %[val], m0\n\t"
               "w6_%=:\n\t"
               "s_mov_b32 m0, %[c6]\n\t"
               "v_writelane_b32 %[B], %[b7], m0\n\t" HSRANS_HEAP_WRITES HSRANS_HEAP_CLIMB_FROM("6", "%[b6]", "%[b7]", "bottom5") HSRANS_HEAP_CLIMBS
               : HSRANS_HEAP_OPERANDS
               : [val] "s"(val), [n7] "s"(n7)
               : "scc");
}

// heap of n entries, 63 <= n <= 126 (levels 0..5 whole, level 6 up to node n - 1)
__device__ __forceinline__ void heap_extract_mid(Heap &h, uint32_t n, uint32_t val)
{
  HeapScratch t;
  const uint32_t n6 = n - 63; // nodes of level 6 in the heap: their lanes in B are below this
  asm volatile(HSRANS_HEAP_HEAD
               // level 5 (A, nodes 31..62) -> level 6 (B): children at lanes 2 c - 62, 2 c - 61, if still in the heap
               "s_lshl1_add_u32 %[l], %[c5], -62\n\t"
               "s_cmp_ge_u32 %[l], %[n6]\n\t"
               "s_cbranch_scc1 bottom5_%=\n\t"
               "s_add_u32 %[r], %[l], 1\n\t"
               "v_readlane_b32 %[sl], %[B], %[l]\n\t"
               "v_readlane_b32 %[sr], %[B], %[r]\n\t"
               "s_cmp_lt_u32 %[r], %[n6]\n\t"
               "s_cselect_b32 %[sr], %[sr], 0\n\t"
               "s_or_b32 %[b6], %[sl], 0xff\n\t"
               "s_cmp_gt_u32 %[sr], %[b6]\n\t"
               "s_cselect_b32 %[b6], %[sr], %[sl]\n\t"
               "s_cselect_b32 %[c6], %[r], %[l]\n\t"
               "s_cmp_gt_u32 %[b6], %[vmax]\n\t"
               "s_cbranch_scc0 bottom5_%=\n\t"
               "s_mov_b32 %[b7], %[val]\n\t"
               "s_mov_b32 m0, %[c6]\n\t"
               "v_writelane_b32 %[B], %[b7], m0\n\t" HSRANS_HEAP_WRITES HSRANS_HEAP_CLIMBS
               : HSRANS_HEAP_OPERANDS
               : [val] "s"(val), [n6] "s"(n6)
               : "scc");
}
// heap of n entries, 1 <= n <= 62 (every node in A; more than 192 of the 256 symbols extracted: near-uniform bytes): every level
// looks whether its children are still in the heap
#define HSRANS_HEAP_DOWN_CHECKED(K, CK, BN, CN) /* node at lane CK of A on level K: children 2 CK + 1, 2 CK + 2 if below n */                    \
  "s_lshl1_add_u32 %[l], " CK ", 1\n\t"                                                                                                           \
  "s_cmp_ge_u32 %[l], %[n]\n\t"                                                                                                                   \
  "s_cbranch_scc1 bottom" K "_%=\n\t"                                                                                                             \
  "s_add_u32 %[r], %[l], 1\n\t"                                                                                                                   \
  "v_readlane_b32 %[sl], %[A], %[l]\n\t"                                                                                                          \
  "v_readlane_b32 %[sr], %[A], %[r]\n\t"                                                                                                          \
  "s_cmp_lt_u32 %[r], %[n]\n\t"                                                                                                                   \
  "s_cselect_b32 %[sr], %[sr], 0\n\t"                                                                                                             \
  "s_or_b32 " BN ", %[sl], 0xff\n\t"                                                                                                              \
  "s_cmp_gt_u32 %[sr], " BN "\n\t"                                                                                                                \
  "s_cselect_b32 " BN ", %[sr], %[sl]\n\t"                                                                                                        \
  "s_cselect_b32 " CN ", %[r], %[l]\n\t"
__device__ __forceinline__ void heap_extract_low(Heap &h, uint32_t n, uint32_t val)
{
  HeapScratch t;
  asm volatile("s_or_b32 %[vmax], %[val], 0xff\n\t"
               "s_mov_b32 %[c1], 0\n\t" // (the root, as the lane the first step starts from)
               HSRANS_HEAP_DOWN_CHECKED("0", "%[c1]", "%[b1]", "%[c1]") HSRANS_HEAP_DOWN_CHECKED("1", "%[c1]", "%[b2]", "%[c2]")
               HSRANS_HEAP_DOWN_CHECKED("2", "%[c2]", "%[b3]", "%[c3]") HSRANS_HEAP_DOWN_CHECKED("3", "%[c3]", "%[b4]", "%[c4]")
               HSRANS_HEAP_DOWN_CHECKED("4", "%[c4]", "%[b5]", "%[c5]")
               // level 5 (nodes 31..62) has no children below 62: the path ends here at the latest
               "s_cmp_gt_u32 %[b5], %[vmax]\n\t"
               "s_cbranch_scc0 bottom4_%=\n\t"
               "s_mov_b32 %[b6], %[val]\n\t" HSRANS_HEAP_WRITES HSRANS_HEAP_CLIMBS
               : HSRANS_HEAP_OPERANDS
               : [val] "s"(val), [n] "s"(n)
               : "scc");
}
#undef HSRANS_HEAP_DOWN_CHECKED
#undef HSRANS_HEAP_PICK_AT
#undef HSRANS_HEAP_PICK
#undef HSRANS_HEAP_DOWN_A
#undef HSRANS_HEAP_HEAD
#undef HSRANS_HEAP_CLIMB_FROM
#undef HSRANS_HEAP_WRITE_A
#undef HSRANS_HEAP_WRITES
#undef HSRANS_HEAP_CLIMBS
#undef HSRANS_HEAP_OPERANDS


// Heap sort of L.order (count << 8 | symbol) as far as the adjustment needs it: the `take` largest entries in the order
// the reference's sort puts them at the top of its array.  Returns, per lane, a 4-bit mask of its symbols (4 * lane + k)
// that are among them.
template <bool PARALLEL_BUILD, class LDS> // (the raw format's kernel keeps the register form: its one wavefront does this once per 100 MB, and the LDS form costs its pass 6 % through the register allocation)
__device__ __forceinline__ uint32_t heap_take_largest(LDS &L, uint32_t lane, uint32_t take)
{
  Heap h;
  if constexpr (PARALLEL_BUILD)
  // The BUILD of the heap (the sort's first phase: sift nodes 127 ... 0 down, in that order) has a level's nodes working on
  // disjoint subtrees, and a node only needs the levels below it finished: all nodes of a level sift at once, one per lane, in
  // LDS — 2 + 3 + ... + 8 dependent steps instead of 128 sifts one after the other — and give the heap the serial order gives.
  // The extractions that follow depend on one another and stay in the registers.
  {
    uint32_t *ord = L.order;
    auto sift = [&](uint32_t root) { // (per lane; comparisons as heap_sift below: by count, the right child only wins when strictly larger)
      const uint32_t val = ord[root];
      uint32_t i = root;
      while (true)
      {
        const uint32_t l = 2 * i + 1;
        if (l >= 256)
          break;
        uint32_t big = l, vb = ord[l];
        if (l + 1 < 256)
        {
          const uint32_t ar = ord[l + 1];
          if ((ar >> 8) > (vb >> 8))
            big = l + 1, vb = ar;
        }
        if ((vb >> 8) <= (val >> 8))
          break;
        ord[i] = vb;
        i = big;
      }
      ord[i] = val;
    };
    if (lane == 0)
      sift(127); // the only level-7 node with a child
    wave_sync();
    sift(63 + lane); // level 6: nodes 63 .. 126
    wave_sync();
    for (uint32_t first = 31; ; first = (first - 1) / 2) // levels 5 .. 0: nodes first .. 2 * first
    {
      if (lane <= first)
        sift(first + lane);
      wave_sync();
      if (first == 0)
        break;
    }
  }
  h.A = L.order[lane < 63 ? lane : 62];
  h.B = L.order[63 + lane];
  h.C = L.order[127 + lane];
  h.D = L.order[191 + lane < 255 ? 191 + lane : 254];
  h.E = __builtin_amdgcn_readfirstlane(L.order[255]);
  if constexpr (!PARALLEL_BUILD)
  {
    heap_sift<7>(h, 127, 256, heap_get<7>(h, 127)); // the only level-7 node with a child
    heap_build_level<6>(h, 63, 126);
    heap_build_level<5>(h, 31, 62);
    heap_build_level<4>(h, 15, 30);
    heap_build_level<3>(h, 7, 14);
    heap_build_level<2>(h, 3, 6);
    heap_build_level<1>(h, 1, 2);
    heap_build_level<0>(h, 0, 0);
  }
  if (take == 0)
    return 0;
  // `take` extractions; i + 1 = the heap's size before the next one, whose last entry (node i) is the one sifted down.  Nothing is
  // recorded per extraction: what was taken is what is no longer among the heap's first i + 1 nodes (every symbol is in it once).
  uint32_t i = 255;
  heap_extract_high(h, i, h.E);
  i--, take--;
  auto run = [&](uint32_t lowest, auto &&extract) { // nodes i ... lowest leave the heap, as long as extractions are wanted
    uint32_t todo = take < i + 1 - lowest ? take : i + 1 - lowest;
    take -= todo;
    for (; todo != 0; todo--, i--)
      extract(i);
  };
  run(191, [&](uint32_t k) { heap_extract_high(h, k, __builtin_amdgcn_readlane(h.D, k - 191)); });
  run(127, [&](uint32_t k) { heap_extract_high(h, k, __builtin_amdgcn_readlane(h.C, k - 127)); });
  run(63, [&](uint32_t k) { heap_extract_mid(h, k, __builtin_amdgcn_readlane(h.B, k - 63)); });
  run(1, [&](uint32_t k) { heap_extract_low(h, k, __builtin_amdgcn_readlane(h.A, k)); }); // (more than 192 of the 256 symbols: near-uniform bytes)
  const uint32_t left = take != 0 ? 0 : i + 1; // (take still wanted with one node left: the root goes too)
  uint8_t *rem = (uint8_t *)L.table;         // (the table's space, not yet in use)
  ((uint32_t *)rem)[lane] = 0;
  wave_sync();
  if (lane < 63 && lane < left)
    rem[h.A & 0xFF] = 1;
  if (63 + lane < left)
    rem[h.B & 0xFF] = 1;
  if (127 + lane < left)
    rem[h.C & 0xFF] = 1;
  if (191 + lane < left) // (nodes 191 .. 254; node 255 left with the first extraction)
    rem[h.D & 0xFF] = 1;
  wave_sync();
  const uint32_t m4 = ((const uint32_t *)rem)[lane];
  const uint32_t taken = ~((m4 & 1) | ((m4 >> 7) & 2) | ((m4 >> 14) & 4) | ((m4 >> 21) & 8)) & 0xFu;
  return taken;
}

// The reference's fix-up of the scaled counts (hist.cpp:103-199; hsrans_host.cpp normalize_counts).  It sorts the symbols
// by count (heap sort) and then runs "steal" passes (sum too large: every symbol with count >= 2 gives one, smallest
// first, until the sum fits) or "charity" passes (sum too small: every symbol with count >= 2 gets one, largest first).
// Only the LAST pass depends on the order, and only through which symbols are on which side of one cut in the sorted
// array; everything else follows from the counts alone:
//   steal:   pass j takes one from every symbol with original count >= j + 1 (m_j of them) while more than m_j are still
//            missing; the final pass J takes from the e_J smallest of those m_J, i.e. from all of them except the
//            m_J - e_J largest of the sort;
//   charity: the symbols with count >= 2 (m of them, their number never changes) each get F = (e - 1) / m, then the
//            e - F * m largest of the sort get one more.
// So the heap sort only has to deliver its largest few entries (heap_take_largest), in exactly the order the reference's
// sort would put them (ties!).  Counts stay in registers: sc[k] is symbol 4 * lane + k.
template <bool PARALLEL_BUILD, class LDS>
__device__ __forceinline__ void adjust_counts(LDS &L, uint32_t lane, uint32_t (&sc)[4], uint32_t sum, uint32_t target)
{
  auto count_ge = [&](uint32_t t) {
    uint32_t n = 0;
    for (uint32_t k = 0; k < 4; k++)
      n += ballot_count(sc[k] >= t);
    return n;
  };
  // (skipping the sort when the cut between taken and spared symbols does not fall inside a run of equal counts — a bisection over
  // ballots finds that out — was measured: no gain, the sort is no longer what a block waits for)
  const uint32_t m = count_ge(2); // >= 1: 256 counts <= 1 cannot come from counts that scale to 2^bits >= 1024
  if (sum > target)
  {
    uint32_t e = sum - target, j = 1, mj = m;
    while (e > mj) // terminates: the symbols can give sum - 256 > e in total
    {
      e -= mj;
      j++;
      mj = count_ge(j + 1);
    }
    const uint32_t spared = heap_take_largest<PARALLEL_BUILD>(L, lane, mj - e);
    for (uint32_t k = 0; k < 4; k++)
    {
      const uint32_t c = sc[k];
      uint32_t give = c >= 2 ? (c - 1 < j - 1 ? c - 1 : j - 1) : 0;
      give += c >= j + 1 && !((spared >> k) & 1) ? 1 : 0;
      sc[k] = c - give;
    }
  }
  else
  {
    const uint32_t e = target - sum;
    const uint32_t full = (e - 1) / m;
    const uint32_t lucky = heap_take_largest<PARALLEL_BUILD>(L, lane, e - full * m);
    for (uint32_t k = 0; k < 4; k++)
      sc[k] += (sc[k] >= 2 ? full : 0) + ((lucky >> k) & 1);
  }
}

} // namespace
} // namespace hsrans

#endif
