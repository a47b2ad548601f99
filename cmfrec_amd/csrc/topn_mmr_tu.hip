// topn_mmr_tu.hip -- the instantiations and the launch of the MMR re-ranking kernel (topn_mmr_kernels.hpp).  A unit of its own
// beside topn_tu.hip and topn_filter_tu.hip, so that the families compile side by side.
#include <algorithm>
#include "topn_mmr_kernels.hpp"

namespace cmfhip {

namespace {

template <int Q>
int launch_mmr(hipStream_t st, int num_cus, const TopnMmrParams<real_t> &P, int max_groups)
{
    const size_t smem = topnm_lds_bytes(P.pool, sizeof(real_t));
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_mmr_kernel<real_t, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    // workgroups per CU: what the registers and this pool's LDS allow
    int per_cu = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, topn_mmr_kernel<real_t, Q>, TOPNM_TH, smem) != hipSuccess || per_cu < 1) per_cu = 1;
    int grid = (int)std::min<long>((long)P.nu, (long)num_cus * per_cu);
    if (max_groups > 0) grid = std::min(grid, max_groups);
    hipLaunchKernelGGL((topn_mmr_kernel<real_t, Q>), dim3(grid), dim3(TOPNM_TH), smem, st, P);
    HIP_CHECK(hipGetLastError());
    return grid;
}

}  // namespace

int topn_mmr_launch(hipStream_t st, int num_cus, const TopnMmrParams<real_t> &P, int max_groups)
{
    static_assert(TOPNM_QMAX == 9, "one case per tile count of topnm_q");
    switch (topnm_q(P.pool)) {
    case 1: return launch_mmr<1>(st, num_cus, P, max_groups);
    case 3: return launch_mmr<3>(st, num_cus, P, max_groups);
    case 6: return launch_mmr<6>(st, num_cus, P, max_groups);
    default: return launch_mmr<9>(st, num_cus, P, max_groups);
    }
}

}  // namespace cmfhip
