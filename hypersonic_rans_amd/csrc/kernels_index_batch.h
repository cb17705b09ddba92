// kernels_index_batch.h — the first decode of MANY streams in one call (hsrans_decode_device_indexing_batch): k_index_pass_batch, the recording
// pass with one wavefront per task — a block_ member's walk, or one block of an mt_ base plan — and the batch forms of the four assembly kernels
// of kernels_walk.h, which read their member's arguments from a table in device memory.
// Part of the one device translation unit hsrans_kernels.hip (which includes the parts in dependency order and holds the host-side launcher).
#ifndef HSRANS_KERNELS_INDEX_BATCH_H
#define HSRANS_KERNELS_INDEX_BATCH_H

namespace hsrans
{

// ---------------------------------------------------------------------------------------------------------------
// The recording pass: blockDim.x = 64, workgroup b runs task b = {member, chain} of a list the host ordered by descending work (workgroups
// are dispatched in index order: the longest walk starts first).  LDS: [ring][table], the private branch of k_decode with one wave; the
// launch's dynamic LDS is sized for the widest table among its members.  The task and the member's record are uniform: scalar loads, once;
// the KParams the shared device functions read (run_block_walk, run_planned_chain) is formed from the record in registers — the fields of
// an index-build pass, nothing else is set.
// ---------------------------------------------------------------------------------------------------------------
template <int MODE>
__global__ void __launch_bounds__(1024) __attribute__((amdgpu_num_sgpr(80))) k_index_pass_batch(const IndexPassTask *tasks, const IndexPassMember *members)
{
  extern __shared__ u32x4 smem_v[];
  uint8_t *smem = (uint8_t *)smem_v;

  const IndexPassTask t = tasks[blockIdx.x];
  const IndexPassMember m = members[t.member];
  KParams kp{};
  kp.stream = m.stream;
  kp.stream_len = m.stream_len;
  kp.out = m.out;
  kp.out_cap = m.out_cap;
  kp.plan = m.plan;
  kp.status = m.status;
  kp.ckpt_states = m.ck_states;
  kp.ckpt_words = m.ck_words;
  kp.ckpt_interval = m.interval;
  kp.walk_blocks = m.walk_blocks;
  kp.walk_states = m.walk_states;
  kp.walk_count = m.walk_count;
  kp.walk_max_blocks = m.walk_max_blocks;

  const PlanView pv = plan_view(kp.plan);
  WaveCtx c;
  wave_ctx_begin(c, kp.stream, kp.stream_len, 0, kp.out, kp.out_cap, kp.status, pv.hdr->bits, pv.hdr->states);
  c.rings = smem;
  c.table = smem + kWaveRingBytes;
  c.table_b = c.table;
  c.gtable = nullptr;
  c.scratch_cnt = (uint16_t *)c.rings;
  c.scratch_cum = (uint16_t *)(c.rings + 512);
  if (pv.hdr->flags & kPlanWalk)
    run_block_walk<MODE>(c, pv, kp);
  else if (t.chain < pv.hdr->n_chains)
    run_planned_chain<MODE, false>(c, pv, t.chain, kp);
}

// ---------------------------------------------------------------------------------------------------------------
// The assembly: the bodies of k_index_count / k_index_fill / k_walk_index_count / k_walk_index_fill (kernels_walk.h) for member
// blockIdx.x of a table of their argument structs.
//   count   one workgroup of 1,024 per member; it also leaves the member's status word (its base plan's, behind the pass) in
//           status_out[member], so that the words of all members come down in one copy
//   fill    grid = members x blocks: the wavefronts of row blockIdx.x stride over the member's blocks
// ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_index_count_batch(const IndexArgs *args, const uint32_t *const *status_of, uint32_t *status_out)
{
  if (threadIdx.x == 0)
    status_out[blockIdx.x] = *status_of[blockIdx.x];
  index_count(args[blockIdx.x]);
}

__global__ void __launch_bounds__(64) k_index_fill_batch(const IndexArgs *args)
{
  const IndexArgs &a = args[blockIdx.x];
  const uint32_t n = a.n_base;
  for (uint32_t ch = blockIdx.y; ch < n; ch += gridDim.y)
    index_fill(a, ch);
}

__global__ void __launch_bounds__(1024) k_walk_index_count_batch(const WalkIndexArgs *args, const uint32_t *const *status_of, uint32_t *status_out)
{
  if (threadIdx.x == 0)
    status_out[blockIdx.x] = *status_of[blockIdx.x];
  walk_index_count(args[blockIdx.x]);
}

__global__ void __launch_bounds__(64) k_walk_index_fill_batch(const WalkIndexArgs *args)
{
  walk_index_fill(args[blockIdx.x], blockIdx.y, gridDim.y);
}

} // namespace hsrans

#endif // HSRANS_KERNELS_INDEX_BATCH_H
