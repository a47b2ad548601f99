// newrows_naz_tu.hip -- the one translation unit that instantiates newrows_naz_kernels.hpp: the right-hand sides of a batch of new
// rows under NA_as_zero (session.hip, newrows_run_naz).  Declarations: newrows.hpp.
#include "newrows.hpp"
#include "newrows_naz_kernels.hpp"

namespace cmfhip {

int naz_launch_rhs(hipStream_t st, int num_cus, const NazRhsParams<real_t> &P, int max_waves)
{
    const int waves = launch_naz_rhs_kernels<real_t>(st, num_cus, P, max_waves);
    HIP_CHECK(hipGetLastError());
    return waves;
}

void naz_launch_pad_rows(hipStream_t st, const real_t *src, size_t lds, int off, int cols, real_t scale, int ones_col, real_t *dst, size_t ldd,
                         size_t rows)
{
    if (rows == 0 || ldd == 0) return;
    hipLaunchKernelGGL(naz_pad_rows_kernel<real_t>, dim3((unsigned)std::min<size_t>((rows * ldd + 255) / 256, 1 << 16)), dim3(256), 0, st, src, lds,
                       off, cols, scale, ones_col, dst, ldd, rows);
    HIP_CHECK(hipGetLastError());
}

void naz_launch_weight_corrections(hipStream_t st, const real_t *w, size_t nnz, real_t *g, real_t *z)
{
    if (nnz == 0) return;
    hipLaunchKernelGGL(naz_weight_corrections_kernel<real_t>, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, w, nnz, g, z);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cmfhip
