// pfmscan_sites.hpp -- what the two site-profile translation units share (pfmscan_sites.hip: one motif, per-group rows;
// pfmscan_sites_lib.hip: a library, long accumulators): the validity keys, their reductions and the verdict.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <climits>
#include <cstdint>

#include "pfmscan_ctx.hpp"

namespace pfmscan {

constexpr int SITE_VERDICT_BLOCK = 1024;
constexpr int64_t SITE_NONE = INT64_MAX;

__device__ inline int64_t site_block_min(int64_t v, int64_t *sh)
{
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (t < s) sh[t] = min(sh[t], sh[t + s]);
        __syncthreads();
    }
    const int64_t m = sh[0];
    __syncthreads();
    return m;
}

// record (off, len), off already relative to the buffer, lies inside it
__device__ inline bool site_inside(int64_t off, int64_t len, int64_t n_pos)
{
    return off >= 0 && len >= 0 && off <= n_pos && len <= n_pos - off;
}

// verdict[0] = the smallest bad flat element index, verdict[1] = the first lane of the check kernel that found a broken table
static __global__ __launch_bounds__(SITE_VERDICT_BLOCK) void k_site_verdict(const int64_t *__restrict__ blk_cells, int64_t n_cells,
                                                                           const int64_t *__restrict__ blk_check, int64_t n_check,
                                                                           int64_t *__restrict__ verdict)
{
    __shared__ int64_t sh[SITE_VERDICT_BLOCK];
    int64_t m = SITE_NONE;
    for (int64_t i = threadIdx.x; i < n_cells; i += SITE_VERDICT_BLOCK) m = min(m, blk_cells[i]);
    m = site_block_min(m, sh);
    if (threadIdx.x == 0) verdict[0] = m;
    m = SITE_NONE;
    for (int64_t i = threadIdx.x; i < n_check; i += SITE_VERDICT_BLOCK) m = min(m, blk_check[i]);
    m = site_block_min(m, sh);
    if (threadIdx.x == 0) verdict[1] = m;
}

// pfmscan_sites.hip
int site_shape(pfmscan_ctx *ctx, bool rows, int dtype, int32_t m, int32_t flank);
// v[0..1] as k_site_verdict wrote them -> status; cell_base is added to the reported element index
int site_verdict(pfmscan_ctx *ctx, const int64_t *v, int64_t cell_base, int64_t *first_bad);

}  // namespace pfmscan
