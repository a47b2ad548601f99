// topn_explain_tu.hip -- the instantiations and the launch of the explanation kernel (topn_explain_kernels.hpp).  A unit of its
// own beside topn_mmr_tu.hip; the row solvers of chol_kernels.hpp, whose diagonal-tile step the kernel borrows, are not
// instantiated here.
#include <algorithm>
#include "topn_explain_kernels.hpp"

namespace cmfhip {

namespace {

template <int Q>
int launch_explain(hipStream_t st, int num_cus, const TopnExplainParams<real_t> &P, int max_groups)
{
    const size_t smem = topnx_layout(P.k + (P.bias ? 1 : 0), P.n_top, P.sr, sizeof(real_t)).bytes;
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_explain_kernel<real_t, Q>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    // workgroups per CU: what the registers and this shape's LDS allow
    int per_cu = 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, topn_explain_kernel<real_t, Q>, TOPNX_TH, smem) != hipSuccess || per_cu < 1) per_cu = 1;
    int grid = (int)std::min<long>((long)P.nu, (long)num_cus * per_cu);
    if (max_groups > 0) grid = std::min(grid, max_groups);
    hipLaunchKernelGGL((topn_explain_kernel<real_t, Q>), dim3(grid), dim3(TOPNX_TH), smem, st, P);
    HIP_CHECK(hipGetLastError());
    return grid;
}

}  // namespace

int topn_explain_launch(hipStream_t st, int num_cus, const TopnExplainParams<real_t> &P, int max_groups)
{
    static_assert(TOPNX_QMAX == 9, "one case per tile count of topnx_q");
    switch (topnx_q(P.k + (P.bias ? 1 : 0))) {
    case 1: return launch_explain<1>(st, num_cus, P, max_groups);
    case 3: return launch_explain<3>(st, num_cus, P, max_groups);
    case 6: return launch_explain<6>(st, num_cus, P, max_groups);
    default: return launch_explain<9>(st, num_cus, P, max_groups);
    }
}

}  // namespace cmfhip
