// enc_pass.h — one wavefront codes one block or stream: encode_body and its stages; k_encode_blocks, k_encode_raw.
// Part of the one encoder translation unit hsrans_encode.hip (which includes the parts in dependency order and holds the launchers).
#ifndef HSRANS_ENC_PASS_H
#define HSRANS_ENC_PASS_H

namespace hsrans
{
namespace
{

template <uint32_t CHUNK>
struct ChunkT
{
  uint4 q[CHUNK / 1024];
};
template <uint32_t CHUNK>
__device__ __forceinline__ ChunkT<CHUNK> chunk_load(const uint8_t *in, uint64_t begin, uint64_t end, uint32_t c, uint32_t lane)
{
  ChunkT<CHUNK> r;
  const uint64_t at = begin + (uint64_t)c * CHUNK;
  if (at + CHUNK <= end) // (wave-uniform; all but a block's last chunk: plain loads instead of guarded ones)
  {
#pragma unroll
    for (uint32_t k = 0; k < CHUNK / 1024; k++)
      r.q[k] = *(const uint4 *)(in + at + k * 1024 + lane * 16);
    return r;
  }
#pragma unroll
  for (uint32_t k = 0; k < CHUNK / 1024; k++)
    r.q[k] = load16_guarded(in, at + k * 1024 + lane * 16, end);
  return r;
}
template <uint32_t CHUNK>
__device__ __forceinline__ void chunk_to_lds(WaveLdsT<CHUNK> &L, const ChunkT<CHUNK> &r, uint32_t c, uint32_t lane)
{
#pragma unroll
  for (uint32_t k = 0; k < CHUNK / 1024; k++)
    *(uint4 *)(L.stage + (c & 1) * CHUNK + k * 1024 + lane * 16) = r.q[k];
}

// one group, general form: lanes whose byte does not exist (the file's last, partial group) keep their state
template <uint32_t S, uint32_t CHUNK>
__device__ __forceinline__ void encode_group_slow(uint32_t &x, WaveLdsT<CHUNK> &L, uint32_t group_off, uint32_t valid, uint32_t &p, uint32_t lane, uint32_t byte_in_group)
{
  constexpr uint32_t kRing = 2 * CHUNK;
  const bool active = lane < S && byte_in_group < valid;
  const uint32_t sym = L.stage[(group_off + byte_in_group) & (kRing - 1)];
  const uint4 e = L.table[sym];
  const bool emit = active && x >= e.x;
  const unsigned long long mask = __builtin_amdgcn_ballot_w64(emit);
  const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
  p -= 2 * (uint32_t)__builtin_popcountll(mask);
  uint32_t v = x;
  if (emit)
  {
    *(uint16_t *)((uint8_t *)L.order + ((p + 2 * rank) & (kOutRing - 1))) = (uint16_t)x; // lane S-1's word goes last in memory (rANS32x64_16w.cpp:65-99)
    v = x >> 16;
  }
  const uint32_t q = __umulhi(v, e.z) >> (e.w >> 24);
  const uint32_t nx = __umul24(q, e.w) + v + e.y;
  x = active ? nx : x;
}

// Four whole groups (a set: groups 4t+3 ... 4t, coded in that order) with their table entries already in registers.
//
// ONE wavefront codes a block and every state is one dependent chain, so the wavefront is alone on its issue port and pays about
// 2.1-2.4 ns for EVERY instruction, whatever it is (tools/microbench/lone_wave.hip: dependent or independent VALU, SALU, s_nop and
// s_waitcnt alike) — the pass costs its instruction count.  Hence one asm statement per set (nothing of the compiler's between the
// groups) and per group the 14 instructions below: the cursor counts words (no shift of the popcount), the ring address is an
// add-shift and an and-or, lanes that emit nothing write to their own sink word through a select of the ADDRESS (two writes of
// EXEC around the store cost three instructions and their hazards), the renormalisation shift is the select itself
// (v_cndmask_b32_sdwa with src1_sel:WORD_1), the table's shift count is read out of byte 3 of its word by the shift.
// `pw`: word offset (from the slot) of the lowest word written; `ring`: LDS address of the emitted-word ring (kOutRing-aligned);
// `sink`: this lane's sink address.  S == 32: only lanes 0..31 hold states; EXEC is narrowed to them for the set.
#define HSRANS_ENC_GROUP(EX, EY, EZ, EW)                                                                                                  \
  "v_cmp_ge_u32 vcc, %[x], " EX "\n\t"                                                                                                    \
  "s_bcnt1_i32_b64 %[n], vcc\n\t" /* (also the wait state a VALU read of VCC as an operand needs after a VALU write of it) */            \
  "v_mbcnt_lo_u32_b32 %[r], vcc_lo, 0\n\t"                                                                                                \
  "v_mbcnt_hi_u32_b32 %[r], vcc_hi, %[r]\n\t"                                                                                             \
  "s_sub_u32 %[pw], %[pw], %[n]\n\t"                                                                                                      \
  "v_add_lshl_u32 %[r], %[r], %[pw], 1\n\t"                                                                                               \
  "v_and_or_b32 %[r], %[r], %[mask], %[ring]\n\t"                                                                                         \
  "v_cndmask_b32 %[r], %[sink], %[r], vcc\n\t"                                                                                            \
  "ds_write_b16 %[r], %[x]\n\t"                                                                                                           \
  "v_cndmask_b32_sdwa %[x], %[x], %[x], vcc dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:WORD_1\n\t"                       \
  "v_mul_hi_u32 %[q], %[x], " EZ "\n\t"                                                                                                   \
  "v_lshrrev_b32_sdwa %[q], " EW ", %[q] dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD\n\t"                          \
  "v_mul_u32_u24 %[q], %[q], " EW "\n\t"                                                                                                  \
  "v_add3_u32 %[x], %[x], " EY ", %[q]\n\t"
template <uint32_t S>
__device__ __forceinline__ void encode_set_fast(uint32_t &x, const uint4 (&e)[4], uint32_t ring, uint32_t sink, uint32_t &pw)
{
  uint32_t r, q, n;
  unsigned long long saved_exec = 0;
  if constexpr (S == 64)
    asm volatile(HSRANS_ENC_GROUP("%[x3]", "%[y3]", "%[z3]", "%[w3]") HSRANS_ENC_GROUP("%[x2]", "%[y2]", "%[z2]", "%[w2]")
                 HSRANS_ENC_GROUP("%[x1]", "%[y1]", "%[z1]", "%[w1]") HSRANS_ENC_GROUP("%[x0]", "%[y0]", "%[z0]", "%[w0]")
                 : [x] "+v"(x), [pw] "+s"(pw), [r] "=&v"(r), [q] "=&v"(q), [n] "=&s"(n)
                 : [x0] "v"(e[0].x), [y0] "v"(e[0].y), [z0] "v"(e[0].z), [w0] "v"(e[0].w), [x1] "v"(e[1].x), [y1] "v"(e[1].y), [z1] "v"(e[1].z), [w1] "v"(e[1].w),
                   [x2] "v"(e[2].x), [y2] "v"(e[2].y), [z2] "v"(e[2].z), [w2] "v"(e[2].w), [x3] "v"(e[3].x), [y3] "v"(e[3].y), [z3] "v"(e[3].z), [w3] "v"(e[3].w),
                   [ring] "v"(ring), [sink] "v"(sink), [mask] "s"(kOutRing - 1)
                 : "vcc", "scc", "memory");
  else
    asm volatile("s_mov_b64 %[ex], exec\n\ts_and_b64 exec, exec, %[lanes]\n\t" //
                 HSRANS_ENC_GROUP("%[x3]", "%[y3]", "%[z3]", "%[w3]") HSRANS_ENC_GROUP("%[x2]", "%[y2]", "%[z2]", "%[w2]")
                 HSRANS_ENC_GROUP("%[x1]", "%[y1]", "%[z1]", "%[w1]") HSRANS_ENC_GROUP("%[x0]", "%[y0]", "%[z0]", "%[w0]") //
                 "s_mov_b64 exec, %[ex]"
                 : [x] "+v"(x), [pw] "+s"(pw), [r] "=&v"(r), [q] "=&v"(q), [n] "=&s"(n), [ex] "=&s"(saved_exec)
                 : [x0] "v"(e[0].x), [y0] "v"(e[0].y), [z0] "v"(e[0].z), [w0] "v"(e[0].w), [x1] "v"(e[1].x), [y1] "v"(e[1].y), [z1] "v"(e[1].z), [w1] "v"(e[1].w),
                   [x2] "v"(e[2].x), [y2] "v"(e[2].y), [z2] "v"(e[2].z), [w2] "v"(e[2].w), [x3] "v"(e[3].x), [y3] "v"(e[3].y), [z3] "v"(e[3].z), [w3] "v"(e[3].w),
                   [ring] "v"(ring), [sink] "v"(sink), [mask] "s"(kOutRing - 1), [lanes] "s"(0xFFFFFFFFull)
                 : "vcc", "scc", "memory");
  // (an asm statement with several outputs returns a struct; when a member of it lives across basic blocks the instruction selector
  // exports the WHOLE struct in registers of one kind — scalar ones here, and the states cannot be copied into those.  These two empty
  // statements, one output each, give the states and the cursor values of their own inside the block.  No instructions.)
  asm volatile("" : "+v"(x));
  asm volatile("" : "+s"(pw));
}
#undef HSRANS_ENC_GROUP

// the 8-byte image of a single-symbol block (mt_rANS32x64_16w_encode.cpp:289-295)
__device__ __forceinline__ uint64_t marker_word(uint32_t size, uint32_t sym) { return (uint64_t)size | ((uint64_t)1 << 63) | ((uint64_t)sym << 54); }

// ---- the headers in front of the words (`words`: where the lowest word was written) ----
__device__ __forceinline__ void write_counts(uint8_t *h, const uint32_t (&sc)[4], uint32_t lane) // [counts 256 x u16]
{
  for (uint32_t k = 0; k < 4; k++)
    *(uint16_t *)(h + 2 * (lane * 4 + k)) = (uint16_t)sc[k];
}
template <uint32_t S>
__device__ __forceinline__ void write_states(uint8_t *h, uint32_t x, uint32_t lane) // [states S x u32]
{
  if (lane < S)
    ((U32a2 *)(h + 4 * lane))->v = x;
}
// the raw stream's: [n u64][total u64][counts 256 x u16][states S x u32] (rANS32x64_16w.cpp:150-166); the image is the finished stream
template <uint32_t S>
__device__ __forceinline__ void write_raw_header(const EncParams &ep, uint8_t *words, uint32_t words_bytes, uint32_t ck_left, const uint32_t (&sc)[4], uint32_t x, uint32_t lane)
{
  constexpr uint32_t kRawHeader = 16 + 512 + 4 * S;
  uint8_t *h = words - kRawHeader;
  const uint64_t total = (uint64_t)kRawHeader + words_bytes;
  if (lane == 0)
  {
    ((U64a2 *)h)->v = ep.n;
    ((U64a2 *)(h + 8))->v = total;
    ep.image_bytes[0] = total;
    ep.image_off[0] = 0;
    ep.result[0] = total;
    ep.result[1] = total <= ep.out_cap ? 1 : 0;
    ep.result[2] = ck_left; // (listed checkpoints that were not met: 0 unless the list was not what the host validated)
  }
  write_counts(h + 16, sc, lane);
  write_states<S>(h + 16 + 512, x, lane);
}
// a block_ block's: [size u64][counts 256 x u16] (block_rANS32x64_16w_encode.cpp; hsrans_host.cpp encode())
__device__ __forceinline__ void write_block_header(const EncParams &ep, const uint32_t b, uint8_t *words, uint32_t size, const uint8_t *slot_end, const uint32_t (&sc)[4], uint32_t lane)
{
  uint8_t *hb = words - (8 + 512);
  if (lane == 0)
  {
    ((U64a2 *)hb)->v = (uint64_t)size;
    ep.image_bytes[b] = (uint64_t)(slot_end - hb);
  }
  write_counts(hb + 8, sc, lane);
}
// an mt_ block's: [size u64][skip u64][states S x u32][counts 256 x u16]
template <uint32_t S>
__device__ __forceinline__ void write_mt_header(const EncParams &ep, const uint32_t b, uint8_t *words, uint32_t size, uint32_t words_bytes, const uint8_t *slot_end, const uint32_t (&sc)[4],
                                                uint32_t x, uint32_t lane)
{
  constexpr uint32_t kHeader = 16 + 4 * S + 512;
  uint8_t *h = words - kHeader;
  // skip: uint16 units from the state array to the next block header, minus one; the last block's is one less
  // (hsrans_host.cpp encode(); mt_rANS32x64_16w_encode.cpp:149,277)
  const uint64_t skip = (uint64_t)(4 * S + 512 + words_bytes) / 2 - 1 - (b + 1 == ep.n_blocks ? 1 : 0);
  if (lane == 0)
  {
    ((U64a2 *)h)->v = (uint64_t)size;
    ((U64a2 *)(h + 8))->v = skip;
    ep.image_bytes[b] = (uint64_t)(slot_end - h);
  }
  write_states<S>(h + 16, x, lane);
  write_counts(h + 16 + 4 * S, sc, lane);
}

// the coder's table {x_max, bias, rcp, cmpl | shift << 24} from the normalised counts
template <class LDS>
__device__ __forceinline__ void write_table(uint32_t bits, LDS &L, uint32_t lane, const uint32_t (&sc)[4], uint32_t part)
{
  const uint32_t target = 1u << bits;
  // exclusive prefix over the 256 counts: lane-local then across lanes
  uint32_t cum = wave_inclusive_scan(part, lane) - part;
  for (uint32_t k = 0; k < 4; k++)
  {
    // x' = x + bias + (x / freq) * (2^bits - freq), the division as multiply-high by a rounded-up reciprocal (exact for
    // x < 2^31, which renormalisation guarantees)
    const uint32_t freq = sc[k];
    uint4 e;
    e.x = freq << (31 - bits); // emit when x >= ((2^15 >> bits) << 16) * freq
    if (freq < 2)
    {
      e.y = cum + target - 1; // rcp = 2^32 - 1 gives x - 1 for freq == 1
      e.z = 0xFFFFFFFFu;
      e.w = target - freq;
      if (freq == 0)
        e.x = 0xFFFFFFFFu;
    }
    else
    {
      const uint32_t shift = 32 - __clz(freq - 1); // smallest shift with freq <= 1 << shift
      e.y = cum;
      // ceil(2^(shift + 31) / freq), in [2^31, 2^32): by one correctly rounded double division — the quotient is an integer or at least
      // 2^-15 away from one (freq <= 2^15), the rounding error below 2^-21 — instead of a 64-bit integer division in software
      e.z = (uint32_t)__builtin_ceil(__builtin_ldexp(1.0, (int)shift + 31) / (double)freq);
      e.w = (target - freq) | ((shift - 1) << 24);
    }
    L.table[lane * 4 + k] = e;
    cum += freq;
  }
}

// ---- byte histogram by the coding wavefront itself: kSubHists copies laid out [symbol][copy], copy = lane & 7 ----
// (a lane's counter sits in bank 8 * (symbol % 4) + copy: lanes of different copies never meet in a bank)
__device__ __forceinline__ void count16(uint32_t *mine, const uint4 &d)
{
  const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
  for (uint32_t k = 0; k < 16; k++)
    atomicAdd(&mine[((w[k >> 2] >> (8 * (k & 3))) & 0xFF) * kSubHists], 1u);
}
template <uint32_t CHUNK>
__device__ __forceinline__ void count_own_bytes(const uint8_t *in, uint64_t begin, uint64_t end, uint32_t size, WaveLdsT<CHUNK> &L, uint32_t lane, uint32_t (&raw)[4])
{
  uint32_t *sub = (uint32_t *)L.table;
  for (uint32_t k = lane; k < kSubHists * 256 / 4; k += 64)
    ((uint4 *)sub)[k] = make_uint4(0, 0, 0, 0);
  wave_sync();
  uint32_t *mine = sub + (lane & (kSubHists - 1));
  uint32_t off = lane * 16;
  for (; off + 3 * 1024 + 16 <= size; off += 4096) // four loads in flight
  {
    uint4 d[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      d[u] = *(const uint4 *)(in + begin + off + u * 1024);
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      count16(mine, d[u]);
  }
  for (; off < size; off += 1024)
  {
    const uint4 d = load16_guarded(in, begin + off, end);
    const uint32_t have = size - off < 16 ? size - off : 16;
    if (have == 16)
      count16(mine, d);
    else
    {
      const uint32_t w[4] = {d.x, d.y, d.z, d.w};
      for (uint32_t k = 0; k < have; k++)
        atomicAdd(&mine[((w[k >> 2] >> (8 * (k & 3))) & 0xFF) * kSubHists], 1u);
    }
  }
  wave_sync();
  for (uint32_t k = 0; k < 4; k++) // symbol 4 * lane + k: its kSubHists copies are 32 bytes in a row
  {
    const uint4 lo = ((const uint4 *)sub)[(lane * 4 + k) * 2], hi = ((const uint4 *)sub)[(lane * 4 + k) * 2 + 1];
    raw[k] = lo.x + lo.y + lo.z + lo.w + hi.x + hi.y + hi.z + hi.w;
  }
  wave_sync();
}

// ---- the rings ----
// emitted words: [p, flushed_to) of the slot is still in the LDS ring only; a whole segment leaves with one 8-byte store per lane
struct OutRing
{
  const uint8_t *ring; // L.order
  uint8_t *slot;
  uint32_t lane;
  uint32_t lds, sink;  // LDS addresses of the ring and of this lane's sink word (encode_set_fast)
  uint32_t flushed_to; // (a multiple of kOutSeg: encode_slot_bytes)
  uint32_t flush_at;   // a segment is complete when the cursor is at or below this word

  __device__ __forceinline__ void flush_segment()
  {
    flushed_to -= kOutSeg;
    const uint2 v = *(const uint2 *)(ring + ((flushed_to & (kOutRing - 1)) + lane * 8));
    *(uint2 *)(slot + flushed_to + lane * 8) = v;
  }
  __device__ __forceinline__ void drain(uint32_t p) const // the ring's rest (less than two segments), word by word
  {
    for (uint32_t o = p + 2 * lane; o < flushed_to; o += 128)
      *(uint16_t *)(slot + o) = *(const uint16_t *)(ring + (o & (kOutRing - 1)));
  }
};

// One wavefront's job.  RAW = false: block b of an mt_ stream with independent blocks (own histogram, own header).
// RAW = true: a whole raw stream (rANS32x64_16w.cpp:34-166 is ONE dependent chain per coder state, so one wavefront is all the
// format has work for): the counts come from the caller or from k_raw_histogram, checkpoints may sit at listed groups, and the
// image in the slot is the finished stream [n][total][counts][states][words].
// CHAIN = true: block b of ep.chain_blocks, one step of k_encode_chain's walk: the states come in through *carry_x and leave
// through it, the counts are the walk's (given_counts[b]), listed checkpoints are absolute groups counted down in *carry_ck.
template <uint32_t S, bool RAW, uint32_t CHUNK, bool CHAIN = false>
__device__ __forceinline__ void encode_body(const EncParams &ep, const uint32_t b, WaveLdsT<CHUNK> &L, const uint32_t lane, uint32_t *carry_x = nullptr,
                                            uint32_t *carry_ck = nullptr)
{
  constexpr uint32_t kChunk = CHUNK, kRing = 2 * CHUNK;
  using Chunk = ChunkT<CHUNK>;
  const uint64_t begin = CHAIN ? ep.chain_blocks[b].begin : RAW ? 0 : (uint64_t)b * ep.block;
  const uint64_t end = CHAIN ? ep.chain_blocks[b].end : RAW || b + 1 == ep.n_blocks ? ep.n : begin + ep.block;
  const uint32_t size = (uint32_t)(end - begin);
  const uint8_t *in = ep.in;
  const uint64_t slot_bytes = CHAIN ? ep.chain_blocks[b].slot_bytes : ep.slot_bytes;
  uint8_t *slot_end = CHAIN ? ep.scratch + ep.chain_blocks[b].slot_end : ep.scratch + (uint64_t)(b + 1) * ep.slot_bytes;

  const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
  uint32_t raw[4] = {0, 0, 0, 0};
  if constexpr (RAW)
  {
    bool missing = false;
    for (uint32_t k = 0; k < 4; k++) // byte counts of the whole input (k_raw_histogram); with given_counts they only say which symbols occur
    {
      raw[k] = ep.given_counts ? ep.given_counts[lane * 4 + k] : ep.raw_counts[lane * 4 + k];
      missing |= raw[k] == 0 && ep.raw_counts[lane * 4 + k] != 0;
    }
    if (__builtin_amdgcn_ballot_w64(missing) != 0) // a symbol of the input has no slot in the caller's histogram: not encodable (hsrans_host.cpp put_group returns 0 too)
    {
      if (lane == 0)
      {
        ep.image_bytes[0] = 0;
        ep.result[0] = 0;
        ep.result[1] = 0;
        ep.result[2] = 0;
      }
      return;
    }
  }
  else if constexpr (CHAIN)
  {
    const uint32_t single = ep.chain_blocks[b].single;
    if (single != 0) // single-symbol block: only the marker word, states untouched (mt_rANS32x64_16w_encode.cpp:289-295)
    {
      if (lane == 0)
      {
        ((U64a2 *)(slot_end - 8))->v = marker_word(size, single & 0xFF);
        ep.image_bytes[b] = 8;
      }
      return;
    }
    for (uint32_t k = 0; k < 4; k++) // the walk's normalised counts (hsrans_host.cpp reference_blocks / fixed_blocks)
      raw[k] = ep.given_counts[(uint64_t)b * 256 + lane * 4 + k];
  }
  else
  {
    if (ep.raw_counts != nullptr) // counted by k_block_histograms, a workgroup per block, before this kernel
    {
      const uint4 v = ((const uint4 *)(ep.raw_counts + (uint64_t)b * 256))[lane];
      raw[0] = v.x, raw[1] = v.y, raw[2] = v.z, raw[3] = v.w;
    }
    else
      count_own_bytes(in, begin, end, size, L, lane, raw);
    uint32_t present = 0;
    for (uint32_t k = 0; k < 4; k++)
      present += raw[k] != 0;
    const uint32_t distinct = wave_sum(present);
    if (distinct == 1) // single-symbol block: only the marker word (mt_rANS32x64_16w_encode.cpp:289-295)
    {
      if (present)
      {
        uint32_t sym = lane * 4;
        for (uint32_t k = 0; k < 4; k++)
          if (raw[k])
            sym = lane * 4 + k;
        ((U64a2 *)(slot_end - 8))->v = marker_word(size, sym);
        ep.image_bytes[b] = 8;
        ep.chain_count[b] = 1;
      }
      return;
    }
  }

  const uint64_t t1 = __builtin_amdgcn_s_memrealtime();
  // ---- normalisation (hist.cpp:16-215; hsrans_host.cpp normalize_counts) ----
  const uint32_t target = 1u << ep.bits;
  const float factor = (float)target / (float)(uint64_t)size;
  uint32_t sc[4];
  uint32_t part = 0;
  const bool normalised = (RAW || CHAIN) && ep.given_counts != nullptr; // the caller's hist_t: already sums to 2^bits (checked on the host)
  for (uint32_t k = 0; k < 4; k++)
  {
    const float v = __fmul_rn((float)raw[k], factor); // one rounding per operation, like the reference's build
    uint32_t c = (uint32_t)(uint16_t)__fadd_rn(v, 0.5f);
    if (c == 0 && raw[k] != 0)
      c = 1;
    if (normalised)
      c = raw[k];
    sc[k] = c;
    part += c;
    L.order[lane * 4 + k] = (c << 8) | (lane * 4 + k);
  }
  const uint32_t sum = wave_sum(part);
  wave_sync();
  // (a block whose scaled counts sum above the target replays ~130 extractions of the heap sort, the others a handful; raising those
  // wavefronts' priority — s_setprio 3 — where two share a SIMD was measured: their normalisation 56 -> 49 us at the 90th percentile,
  // the kernel's length unchanged, 138 us: not kept)
  if constexpr (!CHAIN) // (a chain's counts are normalised by the walk)
    if (sum != target && !normalised)
    {
      adjust_counts<!RAW>(L, lane, sc, sum, target);
      part = sc[0] + sc[1] + sc[2] + sc[3];
    }
  write_table(ep.bits, L, lane, sc, part);

  const uint64_t t2 = __builtin_amdgcn_s_memrealtime();
  // ---- backward rANS pass over the block (rANS32x64_16w.cpp:34-166) ----
  // The block's bytes pass through an LDS ring of two chunks (byte r of the block at ring offset r mod kRing) with a third
  // chunk on its way in registers; symbols and their table entries are fetched one and two sets (of four groups) ahead of
  // the set being coded, so that the state update is the only dependent chain.
  const uint32_t byte_in_group = enc_lane_to_byte(lane) & (S - 1);
  uint32_t x = CHAIN ? *carry_x : 1u << 15;
  uint8_t *slot = slot_end - slot_bytes; // the block's scratch slot; words are written from its end downwards
  uint32_t p = (uint32_t)slot_bytes;     // byte offset (from `slot`) of the lowest word written so far
  // (asking for this first input ahead of the normalisation, which uses neither the ring nor these registers, was measured: nothing)
  const uint32_t n_chunks = (size + kChunk - 1) / kChunk;
  chunk_to_lds(L, chunk_load<CHUNK>(in, begin, end, n_chunks - 1, lane), n_chunks - 1, lane);
  if (n_chunks >= 2)
    chunk_to_lds(L, chunk_load<CHUNK>(in, begin, end, n_chunks - 2, lane), n_chunks - 2, lane);
  Chunk pre{};
  if (n_chunks >= 3)
    pre = chunk_load<CHUNK>(in, begin, end, n_chunks - 3, lane);
  wave_sync();

  // sidecar checkpoints (hsrans_host.cpp encode(): after group gr of the block is coded, gr % interval == 0, gr != 0, the
  // group whole): the decoder's states and read cursor when it is about to start group gr
  const uint32_t whole_groups = size / S;
  auto checkpoint_at = [&](uint64_t ck) {
    if (lane < S)
      ep.ck_states[ck * S + lane] = x;
    if (lane == 0)
      ep.ck_pos[ck] = (uint32_t)slot_bytes - p;
  };
  auto checkpoint = [&](uint32_t gr) { checkpoint_at((CHAIN ? (uint64_t)ep.chain_blocks[b].ck_base : (uint64_t)b * ep.max_ck) + (gr / ep.interval - 1)); };
  if (!RAW && !CHAIN && lane == 0)
    ep.chain_count[b] = 1 + (ep.interval != 0 && whole_groups >= 1 ? (whole_groups - 1) / ep.interval : 0);
  // RAW with listed checkpoints (ascending group indices, multiples of 4; hsrans_host.cpp encode(): `wanted`): the list is walked
  // from its end; entries at or behind the last whole group are never checkpoints
  // CHAIN: the host keeps only the entries that are checkpoints (inside a coded block, not its first group, below the file's last
  // whole group) and this block's are the highest ones left; ck_want is relative to the block's first group g_first
  const uint64_t g_first = begin / S;
  uint32_t ck_left = CHAIN ? *carry_ck : RAW && ep.ck_groups ? ep.n_ck_groups : 0;
  while (!CHAIN && ck_left != 0 && ep.ck_groups[ck_left - 1] >= whole_groups)
    ck_left--;
  auto want_of = [&](uint32_t left) -> uint32_t {
    if (left == 0)
      return 0;
    const uint64_t g = ep.ck_groups[left - 1];
    return CHAIN ? (g > g_first ? (uint32_t)(g - g_first) : 0) : (uint32_t)g;
  };
  uint32_t ck_want = want_of(ck_left); // (0 is never asked for)
  auto listed = [&](uint32_t gr) {
    if (!(RAW || CHAIN) || gr != ck_want || gr == 0)
      return;
    checkpoint_at(ck_left - 1);
    ck_left--;
    ck_want = want_of(ck_left);
  };

  OutRing out{(const uint8_t *)L.order, slot, lane, (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint8_t *)L.order,
              (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) uint32_t *)L.sink + 4 * lane, (uint32_t)slot_bytes, 0};

  uint32_t g = (size + S - 1) / S; // groups of the block still to code; group i covers bytes [i*S, i*S+S)
  if (size % S != 0)               // only the file's last group can be partial
  {
    g--;
    encode_group_slow<S, CHUNK>(x, L, g * S, size - g * S, p, lane, byte_in_group);
  }
  while (g % 4 != 0)
  {
    g--;
    encode_group_slow<S, CHUNK>(x, L, g * S, S, p, lane, byte_in_group);
  }
  wave_sync();
  if (p + kOutSeg <= out.flushed_to) // (at most four groups so far: at most one segment)
    out.flush_segment();

  if (ep.interval != 0 && g != 0 && g % ep.interval == 0 && g < whole_groups)
    checkpoint(g);
  if (g < whole_groups)
    listed(g);

  constexpr uint32_t kSetBytes = 4 * S;
  constexpr uint32_t kSetsPerChunk = kChunk / kSetBytes;
  const uint8_t *my_byte = L.stage + byte_in_group;
  auto read_syms = [&](int32_t t, uint32_t(&s)[4]) { // t < 0 wraps inside the ring: harmless, never coded
    const uint32_t off = (uint32_t)t * kSetBytes;
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
      s[k] = my_byte[(off + k * S) & (kRing - 1)];
  };
  auto read_entries = [&](const uint32_t(&s)[4], uint4(&e)[4]) {
#pragma unroll
    for (uint32_t k = 0; k < 4; k++)
      e[k] = L.table[s[k]];
  };
  auto chunk_finished = [&](uint32_t c) { // every group of chunk c is coded: its ring half takes the chunk two further down
    if (c < 2)
      return;
    chunk_to_lds(L, pre, c - 2, lane);
    if (c >= 3)
      pre = chunk_load<CHUNK>(in, begin, end, c - 3, lane);
    wave_sync();
  };
  if ((uint64_t)g * S <= (uint64_t)(n_chunks - 1) * kChunk) // the groups coded one by one above were all of the last chunk
    chunk_finished(n_chunks - 1);

  // What else happens after a set — a checkpoint, a chunk of input used up — happens at sets known in advance: `event` is the next
  // such set below, and the loop pays one compare per set for all of it (the wavefront pays for every instruction, see above)
  const uint32_t ck_sets = ep.interval != 0 ? ep.interval / (ep.interval % 4 == 0 ? 4 : ep.interval % 2 == 0 ? 2 : 1) : 0; // 4 t % interval == 0  <=>  t % ck_sets == 0
  uint32_t pw = __builtin_amdgcn_readfirstlane(p >> 1); // the cursor in words
  int32_t t = (int32_t)(g / 4) - 1;
  // the next set (<= t) that ends a chunk whose ring half is wanted / that a checkpoint follows / that a listed checkpoint follows; -1: none
  int32_t ev_chunk = t >= (int32_t)(2 * kSetsPerChunk) ? (int32_t)((uint32_t)t / kSetsPerChunk * kSetsPerChunk) : -1;
  int32_t ev_ck = ck_sets != 0 && t >= (int32_t)ck_sets ? (int32_t)((uint32_t)t / ck_sets * ck_sets) : -1;
  auto listed_set = [&]() { return (RAW || CHAIN) && ck_want != 0 && (int32_t)(ck_want / 4) <= t ? (int32_t)(ck_want / 4) : -1; };
  int32_t ev_listed = listed_set();
  auto max3 = [](int32_t a, int32_t b, int32_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); };
  int32_t event = max3(ev_chunk, ev_ck, ev_listed);
  auto set_events = [&]() { // set t (groups 4t .. 4t+3) is coded and something is due after it
    p = pw << 1;
    if (t == ev_ck)
    {
      checkpoint((uint32_t)(4 * t));
      ev_ck = t > (int32_t)ck_sets ? t - (int32_t)ck_sets : -1; // (never after set 0: group 0 starts no chain of its own)
    }
    if ((RAW || CHAIN) && t == ev_listed)
    {
      listed((uint32_t)(4 * t));
      ev_listed = listed_set();
      if (ev_listed == t)
        ev_listed = -1;
    }
    if (t == ev_chunk)
    {
      chunk_finished((uint32_t)t / kSetsPerChunk);
      ev_chunk = t >= (int32_t)(3 * kSetsPerChunk) ? t - (int32_t)kSetsPerChunk : -1;
    }
    event = max3(ev_chunk, ev_ck, ev_listed);
  };

  out.flush_at = (out.flushed_to - kOutSeg) >> 1;
  uint32_t sa[4], sb[4];
  uint4 ea[4], eb[4];
  read_syms(t, sa);
  read_entries(sa, ea);
  read_syms(t - 1, sb);
  // one wait per set: everything fetched during the last set (this set's entries, the next set's symbols) has had a whole set to arrive;
  // said here, the compiler drops the five finer waits it would spread over the set (each a slot of the wavefront's issue port)
  auto lds_arrived = [] {
    __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0)
    __builtin_amdgcn_sched_barrier(0);  // (nothing moves above it: a use scheduled ahead of it would get a wait of its own)
  };
  auto after_set = [&]() { // (both unlikely: a taken branch costs the lone wavefront a refill of its instruction buffer, the straight path must be the common one)
    if (__builtin_expect(pw <= out.flush_at, 0))
    {
      out.flush_segment();
      out.flush_at -= kOutSeg >> 1;
    }
    if (__builtin_expect(t == event, 0))
      set_events();
  };
  if (t >= 0 && (t & 1) == 0) // an odd number of sets: one set ahead of the loop, which then runs two sets a turn and never leaves in the middle
  {
    lds_arrived();
    read_entries(sb, eb);
    read_syms(t - 2, sa);
    encode_set_fast<S>(x, ea, out.lds, out.sink, pw);
    after_set();
    --t;
    for (uint32_t k = 0; k < 4; k++)
      ea[k] = eb[k], sb[k] = sa[k];
  }
  while (t >= 0)
  {
    lds_arrived();
    read_entries(sb, eb);
    read_syms(t - 2, sa);
    encode_set_fast<S>(x, ea, out.lds, out.sink, pw);
    after_set();
    --t;
    lds_arrived();
    read_entries(sa, ea);
    read_syms(t - 2, sb);
    encode_set_fast<S>(x, eb, out.lds, out.sink, pw);
    after_set();
    --t;
  }
  p = pw << 1;

  const uint64_t t3 = __builtin_amdgcn_s_memrealtime();
  if (ep.stamps && lane == 0)
  {
    ep.stamps[b * 4 + 0] = t0;
    ep.stamps[b * 4 + 1] = t1;
    ep.stamps[b * 4 + 2] = t2;
    ep.stamps[b * 4 + 3] = t3;
  }
  const uint32_t words_bytes = (uint32_t)slot_bytes - p;
  if constexpr (CHAIN)
  {
    *carry_x = x;
    *carry_ck = ck_left;
    if (ep.block_states != nullptr && lane < S)
      ep.block_states[(uint64_t)b * S + lane] = x;
  }
  wave_sync();
  out.drain(p);
  if constexpr (RAW)
    write_raw_header<S>(ep, slot + p, words_bytes, ck_left, sc, x, lane);
  else if (CHAIN && !ep.chain_mt)
    write_block_header(ep, b, slot + p, size, slot_end, sc, lane);
  else
    write_mt_header<S>(ep, b, slot + p, size, words_bytes, slot_end, sc, x, lane);
}

template <uint32_t S, uint32_t CHUNK>
__global__ void __launch_bounds__(64) k_encode_blocks(EncParams ep)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[]; // one wavefront per workgroup: its LDS starts at address 0, so every LDS address of the pass is a constant plus the lane's part
  const uint32_t lane = lane_id();
  const uint32_t b = blockIdx.x;
  if (b >= ep.n_blocks)
    return;
  encode_body<S, false, CHUNK>(ep, b, *(WaveLdsT<CHUNK> *)lds_raw, lane);
}

template <uint32_t S>
__global__ void __launch_bounds__(64) k_encode_raw(EncParams ep)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  encode_body<S, true, kChunkFew>(ep, 0, *(WaveLdsT<kChunkFew> *)lds_raw, lane_id());
}

} // namespace
} // namespace hsrans

#endif
