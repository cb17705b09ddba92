// enc_place.h — around the coding pass: histograms, unit summaries and costs, scan, plan, gather and copy; the chain kernels.
// Part of the one encoder translation unit hsrans_encode.hip (which includes the parts in dependency order and holds the launchers).
#ifndef HSRANS_ENC_PLACE_H
#define HSRANS_ENC_PLACE_H

namespace hsrans
{
namespace
{

// ---- raw streams: K_hist (wide) -> K_raw (one wavefront) -> K_copy (wide) -----------------------------------------------
// byte counts of the whole input into counts[256] (zeroed by the launcher): per-workgroup LDS histograms (the sub-histogram layout
// of the block encoder), one global atomic per symbol and workgroup
// (workgroup `wg` of `n_wg` that share the input: the body of k_raw_histogram and of k_raw_histogram_batch)
__device__ __forceinline__ void raw_histogram_body(const uint8_t *in, uint64_t n, uint32_t *counts, uint32_t wg, uint32_t n_wg)
{
  constexpr uint32_t kSubStride = 257; // dwords between copies: copy c of symbol s sits in bank (c + s) % 32, not all in bank s % 32
  __shared__ uint32_t sub[kSubHists * kSubStride];
  for (uint32_t k = threadIdx.x; k < kSubHists * kSubStride; k += 256)
    sub[k] = 0;
  __syncthreads();
  uint32_t *mine = sub + (threadIdx.x & (kSubHists - 1)) * kSubStride;
  for (uint64_t off = ((uint64_t)wg * 256 + threadIdx.x) * 16; off < n; off += (uint64_t)n_wg * 4096)
  {
    const uint4 d = load16_guarded(in, off, n);
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
    const uint32_t have = n - off < 16 ? (uint32_t)(n - off) : 16;
    for (uint32_t k = 0; k < have; k++)
      atomicAdd(&mine[(w[k >> 2] >> (8 * (k & 3))) & 0xFF], 1u);
  }
  __syncthreads();
  uint32_t v = 0;
  for (uint32_t c = 0; c < kSubHists; c++)
    v += sub[c * kSubStride + threadIdx.x];
  if (v)
    atomicAdd(&counts[threadIdx.x], v);
}
__global__ void __launch_bounds__(256) k_raw_histogram(const uint8_t *in, uint64_t n, uint32_t *counts) { raw_histogram_body(in, n, counts, blockIdx.x, gridDim.x); }

// byte counts of every block of an mt_ encode, a workgroup per block: counts[b][256].  The coding wavefront used to count its own
// block (33 us of its ~270 at 64 KiB, 130 us at 256 KiB: 64 lanes of LDS atomics); 256 threads per block and every CU at it take
// a few microseconds for the whole input, and the block is in L2 when the coding wavefront reads it again.
__device__ __forceinline__ void block_histograms_body(EncParams ep, const uint32_t b, uint32_t *counts)
{
  // 32 copies of the histogram, copy = lane & 31, laid out [symbol][copy]: a lane's counter is ALWAYS in bank (lane & 31), whatever the
  // symbol, so the 32 lanes the LDS serves at a time never meet in a bank (the [copy][symbol] layout of round 4, copies 257 dwords apart,
  // put a counter in bank (copy + symbol) % 32: 64 random symbols per instruction, about five to a bank — 31.7 us per 100 MB); equal
  // bytes only meet from lanes 32 apart, which the LDS serves one after the other anyway
  // (23.7 us per 100 MB.  Fewer copies to fit more workgroups on a CU — 24: 6 per CU, all 1,526 blocks in one round — measured slower:
  // 27.3 us with 24, 26.5 us with 16: it is the atomics, not the tail of the grid)
  constexpr uint32_t kCopies = 32;
  __shared__ uint32_t sub[256 * kCopies];
  const uint64_t begin = (uint64_t)b * ep.block;
  const uint64_t end = b + 1 == ep.n_blocks ? ep.n : begin + ep.block;
  for (uint32_t k = threadIdx.x; k < 256 * kCopies; k += 256)
    sub[k] = 0;
  __syncthreads();
  uint32_t *mine = sub + (threadIdx.x & (kCopies - 1));
  auto count16 = [&](const uint4 &d) {
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
      atomicAdd(&mine[((w[k >> 2] >> (8 * (k & 3))) & 0xFF) * kCopies], 1u);
  };
  uint64_t off = begin + threadIdx.x * 16;
  for (; off + 3 * 4096 + 16 <= end; off += 4 * 4096) // four loads in flight per thread
  {
    uint4 d[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      d[u] = *(const uint4 *)(ep.in + off + u * 4096);
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      count16(d[u]);
  }
  for (; off < end; off += 4096)
  {
    const uint4 d = load16_guarded(ep.in, off, end);
    const uint32_t have = end - off < 16 ? (uint32_t)(end - off) : 16;
    if (have == 16)
      count16(d);
    else
    {
      const uint32_t w[4] = {d.x, d.y, d.z, d.w};
      for (uint32_t k = 0; k < have; k++)
        atomicAdd(&mine[((w[k >> 2] >> (8 * (k & 3))) & 0xFF) * kCopies], 1u);
    }
  }
  __syncthreads();
  uint32_t v = 0;
  for (uint32_t c = 0; c < kCopies; c++) // (thread t sums symbol t's copies starting at copy t: the 32 lanes served together read 32 banks)
    v += sub[threadIdx.x * kCopies + ((threadIdx.x + c) & (kCopies - 1))];
  counts[(uint64_t)b * 256 + threadIdx.x] = v;
}
__global__ void __launch_bounds__(256) k_block_histograms(EncParams ep, uint32_t *counts) { block_histograms_body(ep, blockIdx.x, counts); }

// the unit summaries of the block walk (hsrans_host.h UnitSummary: counts[256], run_len, run_sym, fresh_cost; 1040 bytes), a workgroup per unit
// of ep.block symbols: k_block_histograms' counting, and per thread the highest position whose byte differs from the unit's last
// byte (one compare per byte; the run that ends the unit starts behind the highest of them)
// (unit `b`: the body of k_unit_summaries_batch, and k_unit_summaries' own text below: called from that kernel it compiles to other code —
// two instructions more, the rest in another order — and hsrans_encode_device_ex keeps its kernels' code, so the kernel keeps its body)
__device__ __forceinline__ void unit_summaries_body(const EncParams &ep, const uint32_t b, uint8_t *summaries)
{
  constexpr uint32_t kCopies = 32;
  __shared__ uint32_t sub[256 * kCopies];
  __shared__ uint32_t differ;
  const uint64_t begin = (uint64_t)b * ep.block;
  const uint64_t end = b + 1 == ep.n_blocks ? ep.n : begin + ep.block;
  const uint32_t last = ep.in[end - 1];
  for (uint32_t k = threadIdx.x; k < 256 * kCopies; k += 256)
    sub[k] = 0;
  if (threadIdx.x == 0)
    differ = 0;
  __syncthreads();
  uint32_t *mine = sub + (threadIdx.x & (kCopies - 1));
  uint32_t my_differ = 0; // 1 + offset (from begin) of the highest byte seen that is not `last`; 0: none
  auto count = [&](const uint4 &d, uint64_t off, uint32_t have) {
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
      if (k < have)
      {
        const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xFF;
        atomicAdd(&mine[c * kCopies], 1u);
        my_differ = c != last ? (uint32_t)(off - begin) + k + 1 : my_differ; // (offsets ascend per thread)
      }
  };
  uint64_t off = begin + threadIdx.x * 16;
  for (; off + 3 * 4096 + 16 <= end; off += 4 * 4096)
  {
    uint4 d[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      d[u] = *(const uint4 *)(ep.in + off + u * 4096);
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      count(d[u], off + u * 4096, 16);
  }
  for (; off < end; off += 4096)
    count(load16_guarded(ep.in, off, end), off, end - off < 16 ? (uint32_t)(end - off) : 16);
  if (my_differ)
    atomicMax(&differ, my_differ);
  __syncthreads();
  uint32_t v = 0;
  for (uint32_t c = 0; c < kCopies; c++)
    v += sub[threadIdx.x * kCopies + ((threadIdx.x + c) & (kCopies - 1))];
  uint32_t *out = (uint32_t *)(summaries + (uint64_t)b * kUnitSummaryBytes);
  out[threadIdx.x] = v;
  if (threadIdx.x == 0)
  {
    out[256] = (uint32_t)(end - begin) - differ;
    out[257] = last;
    out[258] = 0; // fresh_cost: k_unit_costs
    out[259] = 0;
  }
}
__global__ void __launch_bounds__(256) k_unit_summaries(EncParams ep, uint8_t *summaries)
{
  constexpr uint32_t kCopies = 32;
  __shared__ uint32_t sub[256 * kCopies];
  __shared__ uint32_t differ;
  const uint32_t b = blockIdx.x;
  const uint64_t begin = (uint64_t)b * ep.block;
  const uint64_t end = b + 1 == ep.n_blocks ? ep.n : begin + ep.block;
  const uint32_t last = ep.in[end - 1];
  for (uint32_t k = threadIdx.x; k < 256 * kCopies; k += 256)
    sub[k] = 0;
  if (threadIdx.x == 0)
    differ = 0;
  __syncthreads();
  uint32_t *mine = sub + (threadIdx.x & (kCopies - 1));
  uint32_t my_differ = 0; // 1 + offset (from begin) of the highest byte seen that is not `last`; 0: none
  auto count = [&](const uint4 &d, uint64_t off, uint32_t have) {
    const uint32_t w[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (uint32_t k = 0; k < 16; k++)
      if (k < have)
      {
        const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xFF;
        atomicAdd(&mine[c * kCopies], 1u);
        my_differ = c != last ? (uint32_t)(off - begin) + k + 1 : my_differ; // (offsets ascend per thread)
      }
  };
  uint64_t off = begin + threadIdx.x * 16;
  for (; off + 3 * 4096 + 16 <= end; off += 4 * 4096)
  {
    uint4 d[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      d[u] = *(const uint4 *)(ep.in + off + u * 4096);
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      count(d[u], off + u * 4096, 16);
  }
  for (; off < end; off += 4096)
    count(load16_guarded(ep.in, off, end), off, end - off < 16 ? (uint32_t)(end - off) : 16);
  if (my_differ)
    atomicMax(&differ, my_differ);
  __syncthreads();
  uint32_t v = 0;
  for (uint32_t c = 0; c < kCopies; c++)
    v += sub[threadIdx.x * kCopies + ((threadIdx.x + c) & (kCopies - 1))];
  uint32_t *out = (uint32_t *)(summaries + (uint64_t)b * kUnitSummaryBytes);
  out[threadIdx.x] = v;
  if (threadIdx.x == 0)
  {
    out[256] = (uint32_t)(end - begin) - differ;
    out[257] = last;
    out[258] = 0; // fresh_cost: k_unit_costs
    out[259] = 0;
  }
}

// The adaptive walk's per-unit term (hsrans_host.cpp unit_fresh_cost): the unit's counts normalised at the unit size — the coding
// wavefront's normalisation, one rounding per operation and the heap sort's tie order, which is normalize_counts bit for bit — and its
// code length under them, sum of counts[s] * log2f(fresh[s] / 2^bits) with the logarithms from the host's table, each product and
// each difference rounded on its own (__fmul_rn / __fsub_rn: no contraction), subtracted in symbol order.  A wavefront per whole
// unit; the host keeps only the old histogram's term of _CanExtendHist.  (A short last unit is never a candidate: 0.)
struct UnitCostLds
{
  uint32_t order[256]; // heap_take_largest's sort, as in WaveLdsT
  uint4 table[256];    // (its scratch)
  float prod[256];
};
// (unit `u`: the body of k_unit_costs_batch, and k_unit_costs' own text below, kept there for the same reason as k_unit_summaries')
__device__ __forceinline__ void unit_costs_body(const EncParams &ep, const uint32_t lane, const uint32_t u, uint8_t *summaries, const float *log_table)
{
  __shared__ UnitCostLds L;
  uint32_t *sw = (uint32_t *)(summaries + (uint64_t)u * kUnitSummaryBytes);
  if ((uint64_t)(u + 1) * ep.block > ep.n)
  {
    if (lane == 0)
      sw[258] = 0;
    return;
  }
  const uint32_t target = 1u << ep.bits;
  const float factor = (float)target / (float)ep.block;
  uint32_t raw[4], sc[4], part = 0;
  for (uint32_t k = 0; k < 4; k++)
  {
    raw[k] = sw[lane * 4 + k];
    const float v = __fmul_rn((float)raw[k], factor);
    uint32_t c = (uint32_t)(uint16_t)__fadd_rn(v, 0.5f);
    if (c == 0 && raw[k] != 0)
      c = 1;
    sc[k] = c;
    part += c;
    L.order[lane * 4 + k] = (c << 8) | (lane * 4 + k);
  }
  const uint32_t sum = wave_sum(part);
  wave_sync();
  if (sum != target)
    adjust_counts<true>(L, lane, sc, sum, target);
  for (uint32_t k = 0; k < 4; k++)
    L.prod[lane * 4 + k] = raw[k] != 0 ? __fmul_rn((float)raw[k], log_table[sc[k]]) : 0.0f;
  wave_sync();
  if (lane == 0)
  {
    float cost = (float)(2 * 256 + ep.S * 4 + 8 * 2) * 0.5f;
    for (uint32_t k = 0; k < 256; k++)
      if (sw[k] != 0)
        cost = __fsub_rn(cost, L.prod[k]);
    ((float *)sw)[258] = cost;
  }
}
__global__ void __launch_bounds__(64) k_unit_costs(EncParams ep, uint8_t *summaries, const float *log_table)
{
  __shared__ UnitCostLds L;
  const uint32_t lane = lane_id(), u = blockIdx.x;
  uint32_t *sw = (uint32_t *)(summaries + (uint64_t)u * kUnitSummaryBytes);
  if ((uint64_t)(u + 1) * ep.block > ep.n)
  {
    if (lane == 0)
      sw[258] = 0;
    return;
  }
  const uint32_t target = 1u << ep.bits;
  const float factor = (float)target / (float)ep.block;
  uint32_t raw[4], sc[4], part = 0;
  for (uint32_t k = 0; k < 4; k++)
  {
    raw[k] = sw[lane * 4 + k];
    const float v = __fmul_rn((float)raw[k], factor);
    uint32_t c = (uint32_t)(uint16_t)__fadd_rn(v, 0.5f);
    if (c == 0 && raw[k] != 0)
      c = 1;
    sc[k] = c;
    part += c;
    L.order[lane * 4 + k] = (c << 8) | (lane * 4 + k);
  }
  const uint32_t sum = wave_sum(part);
  wave_sync();
  if (sum != target)
    adjust_counts<true>(L, lane, sc, sum, target);
  for (uint32_t k = 0; k < 4; k++)
    L.prod[lane * 4 + k] = raw[k] != 0 ? __fmul_rn((float)raw[k], log_table[sc[k]]) : 0.0f;
  wave_sync();
  if (lane == 0)
  {
    float cost = (float)(2 * 256 + ep.S * 4 + 8 * 2) * 0.5f;
    for (uint32_t k = 0; k < 256; k++)
      if (sw[k] != 0)
        cost = __fsub_rn(cost, L.prod[k]);
    ((float *)sw)[258] = cost;
  }
}

// (Round 4 also built single-pass placement — the coding wavefront learns its image's position by a decoupled look-back over status
// words (memory-side atomics: the XCDs' L2s are not coherent) and copies the image itself, no scan and gather kernels — and took it
// out again: the blocks of one launch all finish at about the same time, so nearly every look-back walks the whole chain of own
// sizes, 64 per round trip: 0.302 ms against 0.283 for 100 MB in 64 KiB blocks, 0.348 against 0.277 in 32 KiB blocks.)
// ---- K_scan: one workgroup ----------------------------------------------------------------------------------------
// exclusive prefix of `v` over the 1024 threads of the workgroup, plus the workgroup total in *total
__device__ __forceinline__ uint64_t wg_exclusive_scan(uint64_t v, uint64_t *wave_tot, uint64_t *total)
{
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint64_t incl = v;
  for (int d = 1; d < 64; d <<= 1)
  {
    const uint64_t o = __shfl_up(incl, d, 64);
    if ((int)lane >= d)
      incl += o;
  }
  __syncthreads(); // wave_tot may still be read by the previous call
  if (lane == 63)
    wave_tot[wave] = incl;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (uint32_t w = 0; w < 16; w++)
  {
    before += w < wave ? wave_tot[w] : 0;
    all += wave_tot[w];
  }
  *total = all;
  return before + incl - v;
}

// CARRIED (hsrans_encode_host_pipelined): the blocks are one slice of a longer stream.  The stream position, chain count, coded-block
// count and last histogram position come in through *carry and leave through it, so that image_off / chain_off are the absolute ones
// of the whole stream; result[5] is the slice's first byte.  The file header is not written (the caller writes it after the last
// slice), and a slice that is not the stream's last gives its last coded block the skip of a block with a successor (encode_body
// took it for the stream's last block).
template <bool CARRIED = false>
__device__ __forceinline__ void scan_images_body(EncParams ep, EncCarry *carry = nullptr, uint32_t last_slice = 1)
{
  __shared__ uint64_t wave_tot[16];
  uint64_t bytes_before = CARRIED ? carry->bytes_before : 16; // file header
  uint64_t chains_before = CARRIED ? carry->chains_before : 0, coded_blocks = CARRIED ? carry->coded_blocks : 0, last_hist = 0;
  const uint64_t slice_base = bytes_before;
  constexpr uint64_t kNone = ~(uint64_t)0;
  uint64_t my_last = kNone; // highest non-single block this thread has seen
  for (uint32_t base = 0; base < ep.n_blocks; base += 1024)
  {
    const uint32_t i = base + threadIdx.x;
    const bool have = i < ep.n_blocks;
    const uint64_t bytes = have ? ep.image_bytes[i] : 0;
    const uint64_t chains = have ? ep.chain_count[i] : 0;
    uint64_t t_bytes, t_chains, t_coded;
    const uint64_t off = wg_exclusive_scan(bytes, wave_tot, &t_bytes);
    const uint64_t coff = wg_exclusive_scan(chains, wave_tot, &t_chains);
    (void)wg_exclusive_scan(have && bytes != 8 ? 1 : 0, wave_tot, &t_coded);
    if (have)
    {
      ep.image_off[i] = bytes_before + off;
      ep.chain_off[i] = (uint32_t)(chains_before + coff);
      if (bytes != 8)
        my_last = bytes_before + off + 16 + 4 * (uint64_t)ep.S; // where this block's counts will be
    }
    bytes_before += t_bytes;
    chains_before += t_chains;
    coded_blocks += t_coded;
  }
  // any thread's candidate will do when there is exactly one coded block (the only case the value is used in)
  __shared__ uint64_t hist_s;
  if (threadIdx.x == 0)
    hist_s = CARRIED ? carry->last_hist : 0;
  __syncthreads();
  if (my_last != kNone)
    atomicMax((unsigned long long *)&hist_s, (unsigned long long)my_last);
  __syncthreads();
  last_hist = hist_s;
  if (threadIdx.x == 0)
  {
    const uint64_t total = bytes_before;
    if constexpr (CARRIED)
    {
      const uint32_t b = ep.n_blocks - 1;
      const uint64_t bytes = ep.image_bytes[b];
      if (last_slice == 0 && bytes != 8)
      {
        U64a2 *skip = (U64a2 *)(ep.scratch + (uint64_t)(b + 1) * ep.slot_bytes - bytes + 8);
        skip->v = skip->v + 1;
      }
      carry->bytes_before = total;
      carry->chains_before = chains_before;
      carry->coded_blocks = coded_blocks;
      carry->last_hist = last_hist;
      ep.result[0] = total;
      ep.result[1] = 1;
      ep.result[2] = chains_before;
      ep.result[3] = coded_blocks;
      ep.result[4] = last_hist;
      ep.result[5] = slice_base;
    }
    else
    {
      ep.result[0] = total;
      ep.result[1] = total <= ep.out_cap ? 1 : 0;
      if (ep.fits)
        *ep.fits = total <= ep.out_cap ? 1 : 0;
      ep.result[2] = chains_before;
      ep.result[3] = coded_blocks;
      ep.result[4] = last_hist;
      if (total <= ep.out_cap)
      {
        ((uint64_t *)ep.out)[0] = ep.n;
        ((uint64_t *)ep.out)[1] = total;
      }
    }
  }
}
__global__ void __launch_bounds__(1024) k_scan_images(EncParams ep) { scan_images_body(ep); }
__global__ void __launch_bounds__(1024) k_scan_images_carried(EncParams ep, EncCarry *carry, uint32_t last_slice) { scan_images_body<true>(ep, carry, last_slice); }

// ---- K_plan: the sidecar plan of the stream (hsrans_plan.h), one wavefront per block --------------------------------
// Writes exactly what the host encoder emits for the same layout (hsrans_host.cpp encode(), "sidecar plan"): single-piece
// chains in output order — per coded block one chain from the block header's states plus one per checkpoint, per
// single-symbol block one fill chain — and the Group records of the grouped decode launch (one group per block).
// HEADS (hsrans_encode_host_pipelined): the images are gone from ep.scratch by the time the plan is written; what the plan reads of
// them — a coded block's first 16 + 4 S bytes, a single-symbol block's 8-byte marker — was kept by K_gather at ep.scratch + b (16 + 4 S).
template <bool HEADS = false>
__device__ __forceinline__ void plan_blocks_body(EncParams ep, const uint32_t b)
{
  const uint32_t lane = threadIdx.x, S = ep.S;
  const uint32_t nc = ep.n_chains;
  uint32_t *chain_first = (uint32_t *)(ep.plan + plan_chain_first_off());
  Piece *pieces = (Piece *)(ep.plan + plan_pieces_off(nc));
  uint32_t *states = (uint32_t *)(ep.plan + plan_states_off(nc, nc));
  const uint64_t begin = (uint64_t)b * ep.block;
  const uint64_t end = b + 1 == ep.n_blocks ? ep.n : begin + ep.block;
  const uint64_t bytes = ep.image_bytes[b], at = ep.image_off[b];
  const uint32_t c0 = ep.chain_off[b], count = ep.chain_count[b];
  const bool single = bytes == 8;
  const uint64_t header = 16 + 4 * (uint64_t)S + 512;
  const uint64_t hist_off = at + 16 + 4 * (uint64_t)S;
  const uint64_t whole_file = ep.n / S; // whole groups of the file (rANS32x64_16w.cpp:220)
  const uint8_t *image = HEADS ? ep.scratch + (uint64_t)b * (16 + 4 * (uint64_t)S) : ep.scratch + (uint64_t)(b + 1) * ep.slot_bytes - bytes;
  if (b == 0 && lane == 0)
    chain_first[nc] = nc;
  for (uint32_t k = lane; k < count; k += 64)
  {
    Piece p{};
    p.flags = kPieceChainStart;
    p.state_idx = c0 + k;
    if (single)
    {
      p.out_off = begin;
      p.hist_off = (image[6] >> 6) | ((uint64_t)(image[7] & 0x3F) << 2); // bits 54..61 of the marker
      p.fill_len = end - begin;
      p.flags |= kPieceFill;
    }
    else
    {
      const uint64_t g_first = begin / S, g_end = (end - 1) / S + 1;
      const uint64_t g0 = g_first + (uint64_t)k * ep.interval;
      const uint64_t g1 = k + 1 < count ? g0 + ep.interval : g_end;
      p.words_off = k == 0 ? at + header : at + bytes - ep.ck_pos[(uint64_t)b * ep.max_ck + (k - 1)];
      p.out_off = g0 * S;
      p.hist_off = hist_off;
      const uint64_t stop = g1 < whole_file ? g1 : whole_file;
      p.steps = (uint32_t)(stop > g0 ? stop - g0 : 0);
      p.tail = (uint16_t)(k + 1 == count && end == ep.n ? ep.n - whole_file * S : 0);
    }
    pieces[c0 + k] = p;
    chain_first[c0 + k] = c0 + k;
  }
  // start states: chain 0 from the block header (2-byte aligned in the image), the others from the checkpoint slots
  for (uint32_t k = 0; k < count; k++)
    if (lane < S)
    {
      uint32_t v = 0;
      if (!single)
        v = k == 0 ? ((const U32a2 *)(image + 16 + 4 * lane))->v : ep.ck_states[((uint64_t)b * ep.max_ck + (k - 1)) * S + lane];
      states[(uint64_t)(c0 + k) * S + lane] = v;
    }
  if (ep.groups != nullptr && lane < ep.group_split)
  {
    // one Group per part: a block is cut into up to group_split parts of >= 128 chains; the parts that are not needed
    // (short last block, single-symbol block) stay empty
    const uint32_t by_size = group_parts_of(count, ep.group_split); // (hsrans_kernels.h)
    const uint32_t k = single || by_size < 1 ? 1 : by_size;
    Group g{};
    g.flags = single ? kGroupFill : kGroupMergeable;
    g.hist_off = single ? 0 : hist_off;
    if (lane < k)
    {
      const uint32_t lo = (uint32_t)((uint64_t)count * lane / k), hi = (uint32_t)((uint64_t)count * (lane + 1) / k);
      g.begin = c0 + lo;
      g.piece0 = c0 + lo; // (k_plan_blocks: chain c is piece c, state set c)
      g.count = hi - lo;
      g.words_end = hi < count ? at + bytes - ep.ck_pos[(uint64_t)b * ep.max_ck + (hi - 1)] : at + bytes;
    }
    else
    {
      g.begin = c0;
      g.piece0 = c0;
      g.count = 0;
      g.flags = kGroupFill;
      g.words_end = at + bytes;
    }
    ((Group *)ep.groups)[(uint64_t)b * ep.group_split + lane] = g;
  }
}
__global__ void __launch_bounds__(64) k_plan_blocks(EncParams ep) { plan_blocks_body(ep, blockIdx.x); }
__global__ void __launch_bounds__(64) k_plan_blocks_carried(EncParams ep) { plan_blocks_body<true>(ep, blockIdx.x); }

// ---- K_gather: one workgroup per block image; source and destination are only 2-byte aligned -------------------------
struct __attribute__((packed, aligned(2))) U128a2
{
  uint32_t v[4];
};

// sum of `v` over the 256 threads of the workgroup (every thread gets it); `slot`: 4 words of LDS of the caller's
__device__ __forceinline__ uint64_t wg_sum(uint64_t v, uint64_t *slot)
{
  for (int d = 32; d >= 1; d >>= 1)
    v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0)
    slot[threadIdx.x >> 6] = v;
  __syncthreads();
  return slot[0] + slot[1] + slot[2] + slot[3];
}

// Up to this many blocks, every workgroup of K_gather adds up the image sizes in front of its own block itself (n / 256 loads per
// thread out of L2, two reductions) and the scan kernel with its launch is not run at all: K_scan is one workgroup's worth of latency
// (13.5 us at 1,526 blocks) on the path of every encode.  Beyond it the reads grow with the square of the block count: K_scan again.
constexpr uint32_t kSelfScanBlocks = kEncSelfScanBlocks;

// CARRIED (hsrans_encode_host_pipelined): K_scan has run (k_scan_images_carried); the slice's images go to ep.out + (image_off[b] -
// image_off[0]), the slice's own staging buffer, and with `heads` each block's first 16 + 4 S bytes (all of a single-symbol block's 8)
// also to heads + b (16 + 4 S), for the plan written after the last slice (k_plan_blocks_carried)
template <bool CARRIED = false>
__device__ __forceinline__ void gather_images_body(EncParams ep, const uint32_t b, uint8_t *heads = nullptr)
{
  const uint64_t bytes = ep.image_bytes[b];
  uint64_t off;
  if constexpr (CARRIED)
  {
    off = ep.image_off[b] - ep.image_off[0];
    if (heads != nullptr)
    {
      const uint64_t keep = 16 + 4 * (uint64_t)ep.S;
      const uint8_t *src = ep.scratch + (uint64_t)(b + 1) * ep.slot_bytes - bytes;
      uint8_t *dst = heads + (uint64_t)b * keep;
      for (uint64_t i = threadIdx.x * 2; i < (bytes < keep ? bytes : keep); i += 512)
        *(uint16_t *)(dst + i) = *(const uint16_t *)(src + i);
    }
  }
  else if (ep.n_blocks <= kSelfScanBlocks)
  {
    __shared__ uint64_t red[5][4];
    uint64_t before = 0, total = 0, chains_before = 0, chains = 0, coded = 0;
    for (uint32_t i = threadIdx.x; i < ep.n_blocks; i += 256)
    {
      const uint64_t by = ep.image_bytes[i];
      const uint64_t ch = ep.chain_count[i];
      total += by;
      chains += ch;
      coded += by != 8 ? 1 : 0;
      before += i < b ? by : 0;
      chains_before += i < b ? ch : 0;
    }
    before = wg_sum(before, red[0]);
    total = 16 + wg_sum(total, red[1]); // (16: the file header)
    chains_before = wg_sum(chains_before, red[2]);
    chains = wg_sum(chains, red[3]);
    coded = wg_sum(coded, red[4]);
    off = 16 + before;
    const bool fits = total <= ep.out_cap;
    if (threadIdx.x == 0)
    {
      ep.image_off[b] = off;
      ep.chain_off[b] = (uint32_t)chains_before;
      if (bytes != 8 && coded == 1) // the one coded block of the stream says where its counts are (read in that case only)
        ep.result[4] = off + 16 + 4 * (uint64_t)ep.S;
      if (b + 1 == ep.n_blocks)
      {
        ep.result[0] = total;
        ep.result[1] = fits ? 1 : 0;
        ep.result[2] = chains;
        ep.result[3] = coded;
        if (fits)
        {
          ((uint64_t *)ep.out)[0] = ep.n;
          ((uint64_t *)ep.out)[1] = total;
        }
      }
    }
    if (!fits)
      return;
  }
  else
  {
    if (*ep.fits == 0)
      return;
    off = ep.image_off[b];
  }
  const uint8_t *src = ep.scratch + (uint64_t)(b + 1) * ep.slot_bytes - bytes;
  uint8_t *dst = ep.out + off;
  // head: up to the first 16-byte boundary of dst
  uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
  if (head > bytes)
    head = bytes;
  for (uint64_t i = threadIdx.x * 2; i < head; i += 512)
    *(uint16_t *)(dst + i) = *(const uint16_t *)(src + i);
  const uint64_t body = (bytes - head) / 16;
  uint64_t i = threadIdx.x;
  for (; i + 3 * 256 < body; i += 4 * 256) // four loads in flight per thread
  {
    U128a2 v[4];
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      v[u] = *(const U128a2 *)(src + head + (i + u * 256) * 16);
#pragma unroll
    for (uint32_t u = 0; u < 4; u++)
      *(uint4 *)(dst + head + (i + u * 256) * 16) = make_uint4(v[u].v[0], v[u].v[1], v[u].v[2], v[u].v[3]);
  }
  for (; i < body; i += 256)
  {
    const U128a2 v = *(const U128a2 *)(src + head + i * 16);
    *(uint4 *)(dst + head + i * 16) = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  }
  for (uint64_t k = head + body * 16 + threadIdx.x * 2; k < bytes; k += 512)
    *(uint16_t *)(dst + k) = *(const uint16_t *)(src + k);
}
__global__ void __launch_bounds__(256) k_gather_images(EncParams ep) { gather_images_body(ep, blockIdx.x); }
__global__ void __launch_bounds__(256) k_gather_images_carried(EncParams ep, uint8_t *heads) { gather_images_body<true>(ep, blockIdx.x, heads); }

// the one image of a raw encode (the whole stream), copied by workgroups wg of n_wg (k_copy_image: the whole grid)
__device__ __forceinline__ void copy_image_body(EncParams ep, const uint32_t wg, const uint32_t n_wg)
{
  if (ep.result[1] == 0)
    return;
  const uint64_t bytes = ep.image_bytes[0];
  const uint8_t *src = ep.scratch + ep.slot_bytes - bytes; // 2-byte aligned; ep.out is 16-byte aligned
  const uint64_t body = bytes / 16;
  for (uint64_t i = (uint64_t)wg * 256 + threadIdx.x; i < body; i += (uint64_t)n_wg * 256)
  {
    const U128a2 v = *(const U128a2 *)(src + i * 16);
    *(uint4 *)(ep.out + i * 16) = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  }
  if (wg == 0)
    for (uint64_t i = body * 16 + threadIdx.x * 2; i < bytes; i += 512)
      *(uint16_t *)(ep.out + i) = *(const uint16_t *)(src + i);
}
__global__ void __launch_bounds__(256) k_copy_image(EncParams ep) { copy_image_body(ep, blockIdx.x, gridDim.x); }

// ---- chain encodes: block_ / mt_ streams whose coder states run through every block ----------------------------------------
// The reference carries the states from block to block (mt_rANS32x64_16w_encode.cpp:220-222, the block_ encoders alike), so the
// whole input is ONE dependent chain per state: one wavefront codes the blocks back to front (encode_body<CHAIN>), each into a
// slot of its own, then adds up the image sizes and writes the file header; K_gather_chain moves the images into place.
// (the body of k_encode_chain_batch: the chain loop, the placement scan and the header write — k_encode_chain's own text below, kept there
// for the same reason as k_unit_summaries')
template <uint32_t S>
__device__ __forceinline__ void encode_chain_body(const EncParams &ep, WaveLdsT<kChunkFew> &L, const uint32_t lane)
{
  uint32_t x = 1u << 15;
  uint32_t ck_left = ep.ck_groups ? ep.n_ck_groups : 0;
  for (uint32_t b = ep.n_blocks; b-- > 0;)
  {
    if (ep.chain_independent)
      x = 1u << 15;
    encode_body<S, false, kChunkFew, true>(ep, b, L, lane, &x, &ck_left);
    wave_sync(); // (the next block rebuilds the table and the rings this one read; its image sizes are read below)
  }
  // placement: image b at the file header plus the images in front of it
  const uint64_t head = 16 + (ep.chain_mt ? 0 : 4 * (uint64_t)S);
  uint64_t at = head;
  for (uint32_t base = 0; base < ep.n_blocks; base += 64)
  {
    const uint32_t i = base + lane;
    const uint64_t v = i < ep.n_blocks ? ep.image_bytes[i] : 0;
    uint64_t incl = v;
    for (int d = 1; d < 64; d <<= 1)
    {
      const uint64_t o = __shfl_up(incl, d, 64);
      if ((int)lane >= d)
        incl += o;
    }
    if (i < ep.n_blocks)
      ep.image_off[i] = at + incl - v;
    at += __shfl(incl, 63, 64);
  }
  const uint64_t total = at;
  const bool fits = total <= ep.out_cap;
  if (lane == 0)
  {
    ep.result[0] = total;
    ep.result[1] = fits ? 1 : 0;
    ep.result[2] = ck_left; // (listed checkpoints that were not met: 0 unless the list was not what the host filtered)
    if (fits)
    {
      ((uint64_t *)ep.out)[0] = ep.n;
      ((uint64_t *)ep.out)[1] = total;
    }
  }
  if (fits && !ep.chain_mt && lane < S) // block_: the states after the first block follow the file header
    ((uint32_t *)(ep.out + 16))[lane] = x;
}
template <uint32_t S>
__global__ void __launch_bounds__(64) k_encode_chain(EncParams ep)
{
  extern __shared__ __attribute__((aligned(16))) uint8_t lds_raw[];
  const uint32_t lane = lane_id();
  WaveLdsT<kChunkFew> &L = *(WaveLdsT<kChunkFew> *)lds_raw;
  uint32_t x = 1u << 15;
  uint32_t ck_left = ep.ck_groups ? ep.n_ck_groups : 0;
  for (uint32_t b = ep.n_blocks; b-- > 0;)
  {
    if (ep.chain_independent)
      x = 1u << 15;
    encode_body<S, false, kChunkFew, true>(ep, b, L, lane, &x, &ck_left);
    wave_sync(); // (the next block rebuilds the table and the rings this one read; its image sizes are read below)
  }
  // placement: image b at the file header plus the images in front of it
  const uint64_t head = 16 + (ep.chain_mt ? 0 : 4 * (uint64_t)S);
  uint64_t at = head;
  for (uint32_t base = 0; base < ep.n_blocks; base += 64)
  {
    const uint32_t i = base + lane;
    const uint64_t v = i < ep.n_blocks ? ep.image_bytes[i] : 0;
    uint64_t incl = v;
    for (int d = 1; d < 64; d <<= 1)
    {
      const uint64_t o = __shfl_up(incl, d, 64);
      if ((int)lane >= d)
        incl += o;
    }
    if (i < ep.n_blocks)
      ep.image_off[i] = at + incl - v;
    at += __shfl(incl, 63, 64);
  }
  const uint64_t total = at;
  const bool fits = total <= ep.out_cap;
  if (lane == 0)
  {
    ep.result[0] = total;
    ep.result[1] = fits ? 1 : 0;
    ep.result[2] = ck_left; // (listed checkpoints that were not met: 0 unless the list was not what the host filtered)
    if (fits)
    {
      ((uint64_t *)ep.out)[0] = ep.n;
      ((uint64_t *)ep.out)[1] = total;
    }
  }
  if (fits && !ep.chain_mt && lane < S) // block_: the states after the first block follow the file header
    ((uint32_t *)(ep.out + 16))[lane] = x;
}

// copies image b of a chain encode to its place, part `part` of `parts`; source and destination are 2-byte aligned
// (the body of k_gather_chain — b = blockIdx.x, cut into gridDim.y parts — and of k_gather_chain_batch)
__device__ __forceinline__ void gather_chain_body(const EncParams &ep, const uint32_t b, const uint32_t part, const uint32_t parts)
{
  if (ep.result[1] == 0)
    return;
  const uint64_t bytes = ep.image_bytes[b];
  const uint8_t *src = ep.scratch + ep.chain_blocks[b].slot_end - bytes;
  uint8_t *dst = ep.out + ep.image_off[b];
  uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
  if (head > bytes)
    head = bytes;
  const uint64_t body = (bytes - head) / 16;
  if (part == 0)
    for (uint64_t i = threadIdx.x * 2; i < head; i += 512)
      *(uint16_t *)(dst + i) = *(const uint16_t *)(src + i);
  const uint64_t lo = body * part / parts, hi = body * (part + 1) / parts;
  for (uint64_t i = lo + threadIdx.x; i < hi; i += 256)
  {
    const U128a2 v = *(const U128a2 *)(src + head + i * 16);
    *(uint4 *)(dst + head + i * 16) = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  }
  if (part + 1 == parts)
    for (uint64_t k = head + body * 16 + threadIdx.x * 2; k < bytes; k += 512)
      *(uint16_t *)(dst + k) = *(const uint16_t *)(src + k);
}
__global__ void __launch_bounds__(256) k_gather_chain(EncParams ep) { gather_chain_body(ep, blockIdx.x, blockIdx.y, gridDim.y); }

} // namespace
} // namespace hsrans

#endif
