// block_reduce.hpp -- the reductions the trainer's kernels share: the last-arriving-block ticket (the project's one
// piece of memory-ordering code), the halving LDS sum tree, and the fold of per-block partials in block order.
// The ticket (cdna_hip_programming.md, "In-launch split-K reduction"). A grid reduces in ONE launch: every block
// writes its partial to the workspace and draws a ticket from a counter in device memory; the block that draws
// blocks - 1 knows every other has published and finishes the reduction alone. In order: every wave drains its stores
// (s_waitcnt vmcnt(0)) and the block meets at a barrier, so that thread 0's release covers the whole block's partial;
// thread 0 releases at agent scope, waits, and adds 1 to the counter (relaxed, agent scope); the thread that drew
// blocks - 1 acquires at agent scope and waits: every partial is visible to its block, which puts the counter back to
// 0 for the next launch (or the replay of a captured graph; no memset). No block ever waits on another: one that is not
// last just exits, so the grid cannot deadlock whatever part of it is resident. No float atomics: the last block reads
// the partials in a fixed order, so the result does not depend on arrival order and is the same bits every call.
#pragma once
#include <hip/hip_runtime.h>

namespace upkie {

// Thread 0's part, behind the block's drained stores and barrier: true in the one block of `blocks` that arrives last.
__device__ __forceinline__ bool ticket_draw(unsigned* ticket, int blocks) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (drawn != (unsigned)(blocks - 1)) return false;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  return true;
}

// For a kernel whose whole last block goes on: every thread of a block calls it behind the partial's stores; true in
// every thread of the last block (the counter back to 0), false elsewhere. `flag`: one word of the block's LDS.
template <class Word>
__device__ __forceinline__ bool ticket_last_block(unsigned* ticket, int blocks, Word* flag) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) *flag = ticket_draw(ticket, blocks) ? 1 : 0;
  __syncthreads();
  if (*flag == 0) return false;
  if (threadIdx.x == 0) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return true;
}

// Sums the THREADS words of each LDS array into its word 0 by a fixed halving tree (word t += word t + h, h = THREADS / 2
// ... 1; several arrays share the barriers). Every thread has written its word t and calls this; then all may read word 0.
template <int THREADS, class... T>
__device__ __forceinline__ void lds_tree_sum(int tid, T*... lds) {
  for (int h = THREADS / 2; h > 0; h >>= 1) {
    __syncthreads();
    if (tid < h) ((lds[tid] += lds[tid + h]), ...);
  }
  __syncthreads();
}

// p[0] + p[stride] + ... + p[(grid - 1) stride], added in that order from 0.f: one word of `grid` per-block partials,
// 32 loads in flight at a time.
__device__ __forceinline__ float fold_in_block_order(const float* p, int grid, int stride) {
  float s = 0.f;
  int b = 0;
  for (; b + 32 <= grid; b += 32) {
    float x[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) x[k] = p[(size_t)(b + k) * stride];
#pragma unroll
    for (int k = 0; k < 32; ++k) s += x[k];
  }
  for (; b < grid; ++b) s += p[(size_t)b * stride];
  return s;
}

}  // namespace upkie
