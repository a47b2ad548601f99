// launch_dense.hip -- launch unit of the dense layer: the GEMM and Gramian kernels of dense_kernels.hpp, trtri / potrs.
#include "launch.hpp"

namespace cmfhip {

// ------------------------------------------------------------------------------------------
// dense contractions
template <bool TRANSA>
void launch_gemm(const DeviceInfo &dev, int M, int N, int K, real_t alpha, const real_t *A, size_t lda,
                        const real_t *B, size_t ldb, real_t *C, size_t ldc)
{
    if (M <= 0 || N <= 0) return;
    // C[M, N] = alpha * op(A) B, all row-major: the dense contractions of the side-information path (w U C, U^T A, I D, the
    // rotations of the low-rank path).  Round 3: the library's own MFMA kernel (dense_kernels.hpp, gemm_mfma_kernel) -- the
    // matrix cores under an LDS-staged 128 x 128 tile, split over K with an ordered reduction where M x N alone would leave
    // CUs idle (U^T A: 512 x 256 outputs over 1.5 M rows).  Round 6: the only GEMM of the library -- the rocBLAS alternative
    // (CMFREC_HIP_GEMM_OWN=0, rounds 3-5) went with the link against it; cmfrec_hip_gemm_probe still times rocBLAS beside it
    // when that library can be loaded at run time (a measurement tool, not a path).
    {
        DeviceInfo &d = const_cast<DeviceInfo &>(dev);
        const int bm = (M + GEMM_BM - 1) / GEMM_BM, bn = (N + GEMM_BN - 1) / GEMM_BN;
        int nsplit = 1;
        if ((long long)bm * bn < 2LL * dev.num_cus && K >= 4096)
            // (chunks of at least 256: config 3's I^T B -- 64 x 128 outputs over 10,677 rows -- ran as 11 workgroups of 1024 rows each,
            //  204 us per call on 11 of 256 CUs; round 5: 42 workgroups)
            nsplit = (int)std::min<long long>((K + 255) / 256, std::max<long long>(1, (4LL * dev.num_cus) / ((long long)bm * bn)));
        int kchunk = (std::max(K, 1) + nsplit - 1) / nsplit;
        kchunk = (kchunk + GEMM_BK - 1) / GEMM_BK * GEMM_BK;
        nsplit = (std::max(K, 1) + kchunk - 1) / kchunk;
        const dim3 grid(bn, bm, nsplit);
        if (nsplit == 1) {
            hipLaunchKernelGGL((gemm_mfma_kernel<real_t, TRANSA>), grid, dim3(256), 0, dev.stream, M, N, K, kchunk, alpha, A, lda, B, ldb, C, ldc,
                               (size_t)0);
        } else {
            const size_t ss = (size_t)M * N;
            d.gemm_ws.alloc_at_least(ss * nsplit);
            hipLaunchKernelGGL((gemm_mfma_kernel<real_t, TRANSA>), grid, dim3(256), 0, dev.stream, M, N, K, kchunk, alpha, A, lda, B, ldb,
                               d.gemm_ws.ptr, (size_t)N, ss);
            hipLaunchKernelGGL(gemm_splitk_reduce_kernel<real_t>, dim3((unsigned)((ss + 255) / 256)), dim3(256), 0, dev.stream, d.gemm_ws.ptr, ss,
                               nsplit, M, N, C, ldc);
        }
        HIP_CHECK(hipGetLastError());
        return;
    }
}
template void launch_gemm<false>(const DeviceInfo &, int, int, int, real_t, const real_t *, size_t, const real_t *, size_t, real_t *, size_t);
template void launch_gemm<true>(const DeviceInfo &, int, int, int, real_t, const real_t *, size_t, const real_t *, size_t, real_t *, size_t);

// ------------------------------------------------------------------------------------------
// Gramian  out[k,k] = scale * B[:, :k]^T B[:, :k] + add_diag * I
void launch_gram(const DeviceInfo &dev, GramWorkspace &ws, const real_t *B, size_t ldb, int n, int k,
                        real_t *out, real_t scale, real_t add_diag)
{
    if (k <= 64) {
        // two workgroups per CU: 27.9 + 7.1 us for the two stages on C2's 359 k x 50 / 160 k x 50 matrices, against 35.8 + 5.1 (one),
        // 33.0 + 12.3 (four), 36.5 + 17.6 (eight) -- profiles/r03/r03_bo_gram_blocks.txt
        int nblocks = std::max(1, std::min(dev.num_cus * 2, (n + 127) / 128));
        int rpb = std::max(1, (n + nblocks - 1) / nblocks);         // (n == 0: one block of no rows, out = add_diag * I)
        nblocks = (n + rpb - 1) / rpb;
        if (nblocks < 1) nblocks = 1;
        size_t need = (size_t)nblocks * k * k;
        if (ws.partial.n < need) ws.partial.alloc(need);
        // double precision, 48 < k <= 52: the live columns of the last block on the vector ALU (dense_kernels.hpp)
        const int rem = (sizeof(real_t) == 8 && k > 48 && k <= 52) ? k - 48 : 0;
        switch (rem) {
#define CMF_GRAM_REM(R) case R: hipLaunchKernelGGL((gram_mfma_partial_kernel<real_t, R>), dim3(nblocks), dim3(256), 0, dev.stream, B, ldb, n, k, rpb, ws.partial.ptr); break;
            CMF_GRAM_REM(1) CMF_GRAM_REM(2) CMF_GRAM_REM(3) CMF_GRAM_REM(4)
#undef CMF_GRAM_REM
            default: hipLaunchKernelGGL((gram_mfma_partial_kernel<real_t, 0>), dim3(nblocks), dim3(256), 0, dev.stream, B, ldb, n, k, rpb, ws.partial.ptr); break;
        }
        hipLaunchKernelGGL(gram_reduce_kernel<real_t>, dim3((k * k + GRAM_RED_ENT - 1) / GRAM_RED_ENT), dim3(256), 0, dev.stream,
                           ws.partial.ptr, nblocks, k * k, out, scale, add_diag, k);
    } else {
        // k > 64: out = scale * B^T B through the split-K GEMM (both operands the same matrix: 4 x the triangle's flops in
        // the rare k > 64 set-ups, no extra kernel), then the diagonal shift; both triangles are filled
        launch_gemm<true>(dev, k, k, n, scale, B, ldb, B, ldb, out, (size_t)k);
        if (add_diag != 0)
            hipLaunchKernelGGL(add_diag_kernel<real_t>, dim3((k + 255) / 256), dim3(256), 0, dev.stream, out, k, 0, k, add_diag);
    }
    HIP_CHECK(hipGetLastError());
}

// Linv [k, k] := (R^T)^-1 of the row-major upper factor R (dense_kernels.hpp, trtri_from_upper_kernel): R and the rows being built
// staged in LDS while 2 k (k + 1) elements fit (static limit 48 KiB, raised to 96 KiB on request), in global memory beyond.
void launch_trtri(const DeviceInfo &dev, const real_t *R, int k, real_t *Linv)
{
    const size_t tr_smem = (size_t)2 * k * (k + 1) * sizeof(real_t);
    if (tr_smem <= 96 * 1024) {
        auto kern = trtri_from_upper_kernel<real_t, true>;
        if (tr_smem > 48 * 1024) HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tr_smem));
        hipLaunchKernelGGL(kern, dim3(1), dim3(256), tr_smem, dev.stream, R, k, Linv);
    } else {
        hipLaunchKernelGGL((trtri_from_upper_kernel<real_t, false>), dim3(1), dim3(256), 0, dev.stream, R, k, Linv);
    }
    HIP_CHECK(hipGetLastError());
}

// X := X (R^T R)^-1 for the row-major [rows, k] block X (ld = ldx) and the row-major upper Cholesky factor R [k, k] of a
// shared matrix: the multi-right-hand-side posv of optimizeA Case 3 (common.c:3171-3175).  Round 4: no library call -- the
// inverse of the shared matrix once (L^-1 = R^-T by one workgroup, column per thread; M^-1 = L^-T L^-1 by the library's own
// GEMM), then the rows times it as one tall GEMM on the matrix cores (rounds 1-3: two rocBLAS trsm over all rows).
void launch_potrs_rows(const DeviceInfo &dev, int rows, int k, const real_t *R, real_t *X, size_t ldx)
{
    if (rows <= 0 || k <= 0) return;
    DeviceInfo &d = const_cast<DeviceInfo &>(dev);
    d.potrs_inv.alloc_at_least((size_t)2 * k * k);
    d.potrs_tmp.alloc_at_least((size_t)rows * k);
    real_t *Linv = d.potrs_inv.ptr, *Minv = d.potrs_inv.ptr + (size_t)k * k;
    launch_trtri(dev, R, k, Linv);
    launch_gemm<true>(dev, k, k, k, (real_t)1, Linv, (size_t)k, Linv, (size_t)k, Minv, (size_t)k);
    launch_gemm<false>(dev, rows, k, k, (real_t)1, X, ldx, Minv, (size_t)k, d.potrs_tmp.ptr, (size_t)k);
    if (sizeof(real_t) == 4) {
        // Single precision: one step of iterative refinement with the matrix itself.  The product with an explicit inverse carries
        // an error of cond(M) eps where the two triangular solves of the reference's posv are backward stable; x1 = x0 +
        // (b - x0 M) M^-1 brings the residual back to the level of the solves (the right-hand sides are still in X here).
        // M = R^T R from the factor; three tall products instead of one, on rows x k x k flops -- nothing beside the half-step's gather.
        d.potrs_ref.alloc_at_least((size_t)k * k + (size_t)rows * k);
        real_t *Mfull = d.potrs_ref.ptr, *Res = d.potrs_ref.ptr + (size_t)k * k;
        hipLaunchKernelGGL(upper_only_kernel<real_t>, grid1d((size_t)k * k), dim3(256), 0, dev.stream, R, k, Linv);       // (Linv is free again)
        launch_gemm<true>(dev, k, k, k, (real_t)1, Linv, (size_t)k, Linv, (size_t)k, Mfull, (size_t)k);                    // R^T R
        launch_gemm<false>(dev, rows, k, k, (real_t)1, d.potrs_tmp.ptr, (size_t)k, Mfull, (size_t)k, Res, (size_t)k);      // x0 M
        hipLaunchKernelGGL(residual_rows_kernel<real_t>, grid1d((size_t)rows * k), dim3(256), 0, dev.stream, Res, (size_t)k, X, ldx, (size_t)rows, k);   // b - x0 M
        launch_gemm<false>(dev, rows, k, k, (real_t)1, Res, (size_t)k, Minv, (size_t)k, X, ldx);                           // (b - x0 M) M^-1 -> X
        hipLaunchKernelGGL(add_rows_kernel<real_t>, grid1d((size_t)rows * k), dim3(256), 0, dev.stream, X, ldx, d.potrs_tmp.ptr, (size_t)k, (size_t)rows, k);
        HIP_CHECK(hipGetLastError());
        return;
    }
    HIP_CHECK(hipMemcpy2DAsync(X, ldx * sizeof(real_t), d.potrs_tmp.ptr, (size_t)k * sizeof(real_t), (size_t)k * sizeof(real_t), (size_t)rows,
                               hipMemcpyDeviceToDevice, dev.stream));
}

}  // namespace cmfhip
