// topn_filter_tu.hip -- the instantiations and launches of the half-precision filter (topn_filter_kernels.hpp).  A unit of its own
// beside topn_tu.hip, so that the two compile side by side.
#include <algorithm>
#include "topn_filter.hpp"

namespace cmfhip {

void topn_filter_build_image(hipStream_t st, int num_cus, const real_t *dB, size_t ldb, int n, int k, const real_t *dbias, TopnFilterImage &img)
{
    img.ready = img.usable = false;
    if (!img.ev0) { HIP_CHECK(hipEventCreate(&img.ev0)); HIP_CHECK(hipEventCreate(&img.ev1)); }
    img.mx.alloc_at_least(2);
    HIP_CHECK(hipEventRecord(img.ev0, st));
    HIP_CHECK(hipMemsetAsync(img.mx.ptr, 0, 2 * sizeof(unsigned), st));
    const size_t cells = (size_t)n * (size_t)k;
    const unsigned grid = (unsigned)std::min<size_t>((cells + 255) / 256, (size_t)num_cus * 8);
    hipLaunchKernelGGL(topn_filter_absmax_kernel<real_t>, dim3(grid), dim3(256), 0, st, dB, ldb, n, k, dbias, img.mx.ptr);
    HIP_CHECK(hipGetLastError());
    unsigned mx[2] = {0, 0};
    img.mx.download(mx, 2, st);
    HIP_CHECK(hipStreamSynchronize(st));
    img.ready = true;
    // (a bias of 2^100 and more could carry a key past the floats)
    if (topnf_out_of_range(mx[0]) || mx[1] >= ((unsigned)(127 + 100) << 23)) return;
    img.sb = topnf_scale_exp(mx[0]);
    const size_t kh = (size_t)topnf_kh(k);
    img.Bh.alloc_at_least((size_t)n * kh);
    img.nb.alloc_at_least((size_t)n);
    img.db.alloc_at_least((size_t)n);
    const unsigned rows = (unsigned)std::min<size_t>(((size_t)n + 3) / 4, (size_t)num_cus * 8);
    hipLaunchKernelGGL(topn_filter_image_kernel<real_t>, dim3(rows), dim3(256), 0, st, dB, ldb, n, k, img.sb, img.Bh.ptr, img.nb.ptr, img.db.ptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(img.ev1, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipEventElapsedTime(&img.build_ms, img.ev0, img.ev1));
    img.usable = true;
}

int topn_filter_pick_tiles(int nu, int k, int m, int num_cus, int forced, int *blocks_per_cu)
{
    int best = 1, best_bpc = 1;
    double best_cost = 0;
    for (int nut = 1; nut <= TOPNF_MAX_NUT; nut <<= 1) {
        const size_t smem = topnf_lds_bytes(nut, k, m);
        if (smem > TOPNF_LDS_MAX) break;
        const int bpc = (int)std::min<size_t>(TOPNF_LDS_MAX / smem, (size_t)(2048 / TOPNF_TH));
        const long tiles = ((long)nu + 16 * nut - 1) / (16 * nut), slots = (long)num_cus * bpc;
        const long share = std::min<long>(bpc, (tiles + num_cus - 1) / num_cus);
        const double cost = (double)((tiles + slots - 1) / slots) * share * (nut + 0.5);
        if (nut == 1 || (forced > 0 ? nut <= forced : cost <= best_cost)) { best = nut; best_bpc = bpc; best_cost = cost; }
    }
    *blocks_per_cu = best_bpc;
    return best;
}

namespace {

template <int NUT>
int launch_filter(hipStream_t st, int num_cus, const TopnFilterParams<real_t> &P, int blocks_per_cu)
{
    const size_t smem = topnf_lds_bytes(NUT, P.k, P.m);
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_filter_kernel<real_t, NUT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = (P.nu + 16 * NUT - 1) / (16 * NUT);
    const int grid = std::min(tiles, num_cus * blocks_per_cu);
    hipLaunchKernelGGL((topn_filter_kernel<real_t, NUT>), dim3(grid), dim3(TOPNF_TH), smem, st, P);
    return grid;
}

}  // namespace

int topn_filter_launch(hipStream_t st, int num_cus, const TopnFilterParams<real_t> &P, int forced_tiles, int *users_per_wg)
{
    int bpc = 1, grid = 0;
    const int nut = topn_filter_pick_tiles(P.nu, P.k, P.m, num_cus, forced_tiles, &bpc);
    switch (nut) {
    case 1: grid = launch_filter<1>(st, num_cus, P, bpc); break;
    case 2: grid = launch_filter<2>(st, num_cus, P, bpc); break;
    case 4: grid = launch_filter<4>(st, num_cus, P, bpc); break;
    default: grid = launch_filter<8>(st, num_cus, P, bpc); break;
    }
    HIP_CHECK(hipGetLastError());
    *users_per_wg = 16 * nut;
    return grid;
}

void topn_filter_launch_keys(hipStream_t st, int num_cus, const TopnFilterParams<real_t> &P)
{
    const size_t smem = topnf_lds_bytes(1, P.k, P.m);
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_filter_keys_kernel<real_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int grid = std::min((P.nu + 15) / 16, num_cus * 2);
    hipLaunchKernelGGL(topn_filter_keys_kernel<real_t>, dim3(grid), dim3(TOPNF_TH), smem, st, P);
    HIP_CHECK(hipGetLastError());
}

void topn_filter_refine(hipStream_t st, int num_cus, const TopnRefineParams<real_t> &P, bool wide)
{
    const int grid = std::min((P.nu + TOPNF_REFINE_NW - 1) / TOPNF_REFINE_NW, num_cus * 8);
    if (wide) hipLaunchKernelGGL((topn_filter_refine_kernel<real_t, true>), dim3(grid), dim3(64 * TOPNF_REFINE_NW), 0, st, P);
    else hipLaunchKernelGGL((topn_filter_refine_kernel<real_t, false>), dim3(grid), dim3(64 * TOPNF_REFINE_NW), 0, st, P);
    HIP_CHECK(hipGetLastError());
}

void topn_filter_certify(hipStream_t st, const real_t *scores, int nu, int n_top, const float *tau, const int *state, int *certified)
{
    hipLaunchKernelGGL(topn_filter_certify_kernel<real_t>, dim3((unsigned)((nu + 255) / 256)), dim3(256), 0, st, scores, nu, n_top, tau, state,
                       certified);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cmfhip
