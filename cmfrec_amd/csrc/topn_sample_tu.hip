// topn_sample_tu.hip -- the instantiations and the launch of the sampling kernels (topn_sample_kernels.hpp).  A unit of its own
// beside topn_tu.hip, which holds the host side of the call: the ranking units compile as they did.
#include <algorithm>
#include "topn_sample_kernels.hpp"

namespace cmfhip {

namespace {

template <int NUT, bool LSE>
int launch_sample(hipStream_t st, int num_cus, int blocks_per_cu, const TopnSampleParams<real_t> &P)
{
    const size_t smem = topnsm_lds_bytes(NUT, P.k, P.n_top, sizeof(real_t), LSE);
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_sample_kernel<real_t, NUT, LSE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = (P.nu + 16 * NUT - 1) / (16 * NUT);
    const int grid = std::min(tiles, num_cus * blocks_per_cu);
    hipLaunchKernelGGL((topn_sample_kernel<real_t, NUT, LSE>), dim3(grid), dim3(TOPNW_TH), smem, st, P);
    HIP_CHECK(hipGetLastError());
    return grid;
}

template <bool LSE>
int launch_sample_tiles(hipStream_t st, int num_cus, int nut, int blocks_per_cu, const TopnSampleParams<real_t> &P)
{
    static_assert(TOPNW_MAX_NUT == 4, "one case per tile count");
    switch (nut) {
    case 1: return launch_sample<1, LSE>(st, num_cus, blocks_per_cu, P);
    case 2: return launch_sample<2, LSE>(st, num_cus, blocks_per_cu, P);
    case 3: return launch_sample<3, LSE>(st, num_cus, blocks_per_cu, P);
    default:
        // (four tiles with the log-partition's state do not fit the registers in double precision: topnsm_max_tiles)
        if constexpr (topnsm_max_tiles(sizeof(real_t), LSE) >= 4) return launch_sample<4, LSE>(st, num_cus, blocks_per_cu, P);
        else return launch_sample<3, LSE>(st, num_cus, blocks_per_cu, P);
    }
}

}  // namespace

int topn_sample_launch(hipStream_t st, int num_cus, int nut, int blocks_per_cu, const TopnSampleParams<real_t> &P, real_t *out_scores)
{
    const int grid = P.out_lse != nullptr ? launch_sample_tiles<true>(st, num_cus, nut, blocks_per_cu, P)
                                          : launch_sample_tiles<false>(st, num_cus, nut, blocks_per_cu, P);
    if (out_scores != nullptr) {
        hipLaunchKernelGGL(topn_sample_scores_kernel<real_t>, dim3((unsigned)((P.nu + 15) / 16), (unsigned)P.n_top), dim3(64), 0, st, P, out_scores);
        HIP_CHECK(hipGetLastError());
    }
    return grid;
}

}  // namespace cmfhip
