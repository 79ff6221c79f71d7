// jobs.hpp -- the job grid of a launch that covers several tensors: ONE table layout, ONE append, ONE block-to-job scan.
//
// A multi-tensor kernel (adam.hip, sparse_adam.hip, the apply kernels of densify.hip and mcmc.hip, the observer and the int8
// pass of qat.hip) gets its tensors as a by-value table and gives each a contiguous range of workgroups:
//     job j owns blocks [first_block[j], first_block[j] + nblocks[j]),   grid = the sum of nblocks
// The launcher keeps what is its own: how many workgroups a tensor wants, the cap, and which tensors it leaves out.
//
// Not this: CbJobs of qat.hip. Its three jobs are fixed and chosen by POSITION (scales, rotations, features), an absent one
// stays in the table with a sentinel first_block so that it is never selected. It has no count and no append.
#pragma once
#include "common.hpp"

namespace c3dgs {

template <class T, int MAX>
struct JobTable {
    T t[MAX];
    int first_block[MAX];
    int nblocks[MAX];
    int n = 0;

    int grid() const { return n ? first_block[n - 1] + nblocks[n - 1] : 0; }
    // one more job, of `want` workgroups clamped to [1, cap]; the caller keeps n below MAX
    void add(const T& job, long long want, int cap)
    {
        first_block[n] = grid();
        nblocks[n] = (int)(want < 1 ? 1 : (want > cap ? cap : want));
        t[n++] = job;
    }
};

// the job that owns this workgroup: the last one whose first block is not past it
template <class T, int MAX>
__device__ __forceinline__ int job_of_block(const JobTable<T, MAX>& jobs)
{
    int j = 0;
#pragma unroll
    for (int k = 1; k < MAX; k++)
        if (k < jobs.n && (int)blockIdx.x >= jobs.first_block[k]) j = k;
    return j;
}

// the table of c3dgs_rows_apply and c3dgs_mcmc_apply (densify.hip, mcmc.hip)
using RowsJobs = JobTable<c3dgs_rows_tensor, C3DGS_ROWS_MAX_TENSORS>;

} // namespace c3dgs
