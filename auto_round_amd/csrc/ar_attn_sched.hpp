// ar_attn_sched.hpp -- the item schedule of the persistent key-side attention backward (csrc/ar_attn_exact.hip, k_xattn_bwd<.., GRP>).
// Host and device compile the same function: the host only sizes the grid, every workgroup derives its own fixed run from its index,
// and nothing is communicated between workgroups.
//
// An item is (batch, key head, block of 128 keys), numbered item = (batch * key_heads + key_head) * key_blocks + key_block, so the items
// of one (batch, key head) are neighbours.  Run r of n_runs is the contiguous range [first, first + count): the first items % n_runs runs
// are one item longer than the rest, so run lengths differ by at most one and every item belongs to exactly one run.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AR_SCHED_HD __host__ __device__ __forceinline__
#else
#define AR_SCHED_HD inline
#endif

namespace ar {

AR_SCHED_HD void xattn_group_run(int run, int n_runs, int items, int& first, int& count) {
    const int q = items / n_runs, r = items % n_runs;
    first = run * q + (run < r ? run : r);
    count = q + (run < r ? 1 : 0);
}

// workgroup index -> run.  Workgroups go to the 8 XCDs round-robin (index % 8); the workgroups of one XCD take NEIGHBOURING runs, so the
// key blocks of one (batch, key head) -- which stream the same Q / dO rows, head after head at about the same time -- meet in one L2
// (the rule of xattn_map).  A permutation of [0, n_runs) either way.
AR_SCHED_HD int xattn_group_run_of_block(int block, int n_runs) {
    if (n_runs & 7) return block;
    return (block & 7) * (n_runs >> 3) + (block >> 3);
}

}  // namespace ar
