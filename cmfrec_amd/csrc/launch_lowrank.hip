// launch_lowrank.hip -- launch unit of the low-rank row updates (lowrank_kernels.hpp) and of the symmetric eigen-decomposition
// they rest on (eig_kernels.hpp), with the entry point that runs the decomposition on its own (cmfrec_hip_sym_eig).
#include "launch.hpp"
#include "lowrank_kernels.hpp"
#include "eig_kernels.hpp"

namespace cmfhip {

// Enqueues the decomposition of the kc x kc matrix Minit on the eigen stream, behind `after` (an event of the main stream:
// what produced Minit), and records E.ev behind it.
void issue_eig(DeviceInfo &d, EigCache &E, const real_t *Minit, int kc, hipEvent_t after)
{
    E.W.alloc_at_least((size_t)kc * kc); E.V.alloc_at_least((size_t)kc * kc);
    E.Q.alloc_at_least((size_t)kc * kc); E.Qt.alloc_at_least((size_t)kc * kc); E.Lam.alloc_at_least((size_t)kc);
    if (!E.ev) HIP_CHECK(hipEventCreateWithFlags(&E.ev, hipEventDisableTiming));
    HIP_CHECK(hipStreamWaitEvent(d.eig_stream(), after, 0));
    // default: Householder tridiagonalisation + implicit QL with the rotations applied row-parallel (eig_kernels.hpp);
    // CMFREC_HIP_EIG=jacobi takes the one-workgroup Jacobi kernel (on-device cross-check; also the fallback should a QL iteration
    // ever fail to converge: the status word is read back the first time a matrix of this size goes through a cache)
    static bool ql_bad = false;
    bool done = false;
    if (!ql_bad && !switches().eig_jacobi && kc <= EIG_MAX_N) {
        E.D.alloc_at_least((size_t)kc); E.E.alloc_at_least((size_t)kc); E.Tau.alloc_at_least((size_t)kc);
        if (E.info.n < 1) { E.info.alloc(1); HIP_CHECK(hipMemsetAsync(E.info.ptr, 0, sizeof(int), d.eig_stream())); }
        hipLaunchKernelGGL(eig_tridiag_kernel<real_t>, dim3(1), dim3(EIG_TRIDIAG_THREADS), 0, d.eig_stream(), Minit, kc, E.W.ptr, E.D.ptr, E.E.ptr, E.Tau.ptr);
        const bool wide = kc > 288;                          // rows of the eigenvector matrix per workgroup: 64, or 32 (LDS: kc rows doubles)
        const int rows = wide ? 32 : 64;
        const size_t smem = ((size_t)kc * rows + 4 * (size_t)kc) * sizeof(double);
        auto kern = wide ? eig_ql_rows_kernel<real_t, 32> : eig_ql_rows_kernel<real_t, 64>;
        static thread_local bool attr_set[MAX_DEVICES][2] = {{false}};
        bool &as = attr_set[std::min(std::max(d.device, 0), MAX_DEVICES - 1)][wide ? 1 : 0];
        if (!as) { HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024)); as = true; }
        hipLaunchKernelGGL(kern, dim3((kc + rows - 1) / rows), dim3(64), smem, d.eig_stream(), kc, E.W.ptr, E.D.ptr, E.E.ptr, E.Tau.ptr, E.Q.ptr,
                           E.Qt.ptr, (size_t)kc, E.Lam.ptr, E.info.ptr);
        HIP_CHECK(hipGetLastError());
        done = true;
        if (E.checked_kc != kc) {
            int h_info = 0;
            HIP_CHECK(hipMemcpyAsync(&h_info, E.info.ptr, sizeof(int), hipMemcpyDeviceToHost, d.eig_stream()));
            HIP_CHECK(hipStreamSynchronize(d.eig_stream()));
            E.checked_kc = kc;
            if (h_info != 0) { ql_bad = true; done = false; }
        }
    }
    if (!done)
        hipLaunchKernelGGL(jacobi_eig_kernel<real_t>, dim3(1), dim3(1024), 0, d.eig_stream(), Minit, kc, E.W.ptr, E.V.ptr, E.Q.ptr, E.Qt.ptr,
                           (size_t)kc, E.Lam.ptr, 30, sizeof(real_t) == 4 ? 1e-9 : 1e-13);
    E.kind = done ? 3 : 2;
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(E.ev, d.eig_stream()));
}

// Collective Cholesky half-step (mode CHOL_COLLECTIVE, dense side information on every row of the block) with the rows of
// few entries solved by the low-rank update of a diagonalised shared matrix instead of a k_t^3 / 3 factorisation per row
// (config 5's users: 20 entries against k_t = 257 unknowns).  c: the call as launch_chol would take it (right-hand sides
// w U C already in the rows, c.Minit = w C^T C); Um: the block's rows of U; k: the factors shared with X; rows_b: rows of
// the opposing matrix.  Returns -1 when the path does not apply (the caller launches as usual), else the return code.
// CMFREC_HIP_LOWRANK=0 switches it off, =1 forces it whenever the shapes allow (tests).
// mine: this side's cache (NULL: the scratch's own, never fresh); next / kc_next: the other side's cache with its matrix in
// next->M, decomposed behind this one for the half-step that follows (NULL: nothing to prefetch).
int launch_collective_lowrank(const DeviceInfo &dev, LowRankScratch &S, CholCall c, const SparseShard &X, const real_t *Cm,
                                     const SideOperand &Um, int p_self, real_t w, int k, int rows_b, EigCache *mine,
                                     EigCache *next, int kc_next)
{
    const int lr_sw = switches().lowrank;       // CMFREC_HIP_LOWRANK: 0 / 1 force the path off / on
    const int kt = c.kt, kc = c.kc, k_side_self = c.koff;
    // rows of up to lr_max entries: the s x s system is at most half the k_t x k_t one (and 8 blocks in single, 4 in double)
    const int lr_type_max = (sizeof(real_t) == 4) ? 128 : 64;
    const int lr_max = (kt >= 256 && lr_type_max >= 128) ? 128 : (kt >= 128 ? 64 : 32);
    const int n_full = X.rows_longer_than(lr_max, X.nrows);          // positions [0, n_full): full factorisation
    const int n_light = X.nrows - n_full;
    const bool lr_ok = lr_sw != 0 && c.mode == CHOL_COLLECTIVE && c.Mfull == nullptr && c.X2 == nullptr &&
                       !X.weighted() &&
                       !c.scale_bias_const && !dev.nonneg_now && !c.nonneg && dev.l1_now == (real_t)0 && dev.l1_last_now == (real_t)0 &&
                       c.rows_with_u >= X.nrows && !c.rhs_prefilled_all && kt <= 320 && kt >= 64 && kc > 0 && p_self > 0 &&
                       // the penalty must be a multiple of the identity on the rotated block: the last unknown's own lambda
                       // (a bias) has to sit outside of it
                       (kt - 1 >= kc || c.lam_last == c.lam) &&
                       (lr_sw == 1 || (n_light >= 32768 && kt >= 96));
    S.last_rows = 0; S.last_eig = 0;
    if (!lr_ok || n_light <= 0) return -1;
    hipStream_t st = dev.stream;
    const int ngr = (kt + 15) / 16;
    const size_t ldbt = (size_t)16 * ngr;
    S.Ct.alloc_at_least((size_t)p_self * kc);
    S.Bt.alloc_at_least((size_t)rows_b * ldbt + 64);
    S.R.alloc_at_least((size_t)X.nrows * kc);
    S.T.alloc_at_least((size_t)n_light * kc);
    EigCache &E = mine ? *mine : S.own;
    if (mine) mine->wanted = true;
    // w C^T C = Q L Q^T on the eigen stream, beside the full factorisations of the longer rows (which do not need it and are
    // enqueued first: see EigCache)
    {
        DeviceInfo &d = const_cast<DeviceInfo &>(dev);
        d.ensure_aux();
        const bool have = mine != nullptr && mine->fresh && mine->ev != nullptr;
        const bool ahead = next != nullptr && kc_next > 0;
        if (!have || ahead) {
            if (!d.eig_fork) HIP_CHECK(hipEventCreateWithFlags(&d.eig_fork, hipEventDisableTiming));
            HIP_CHECK(hipEventRecord(d.eig_fork, st));
        }
        c.row_limit = n_full;
        const int rc = (n_full > 0) ? launch_chol(dev, c, &X) : 0;
        if (rc) return rc;
        if (!have) {
            issue_eig(d, E, c.Minit, kc, d.eig_fork);
            if (mine) mine->fresh = true;          // (c.Minit is the session's w C^T C of this side as it stands)
        }
        if (ahead) {
            issue_eig(d, *next, next->M.ptr, kc_next, d.eig_fork);
            next->fresh = true;
        }
        S.last_eig = E.kind;
        S.last_rows = n_light;
        HIP_CHECK(hipStreamWaitEvent(st, E.ev, 0));
    }
    // C~ = C Q ;  B~ = [B(:, :k) Q(k_side:, :) | B(:, k:)] ;  R = w U C~ (natural row order)
    launch_gemm<false>(dev, p_self, kc, kc, (real_t)1, Cm, (size_t)kc, E.Q.ptr, (size_t)kc, S.Ct.ptr, (size_t)kc);
    launch_gemm<false>(dev, rows_b, kc, k, (real_t)1, c.B, c.ldb, E.Q.ptr + (size_t)k_side_self * kc, (size_t)kc, S.Bt.ptr, ldbt);
    if (kt > kc)
        hipLaunchKernelGGL(copy_cols_kernel<real_t>, grid1d((size_t)rows_b * (kt - kc)), dim3(256), 0, st, S.Bt.ptr, ldbt, kc, c.B, c.ldb, k,
                           kt - kc, (size_t)rows_b);
    side_times(dev, Um, X.nrows, kc, p_self, w, S.Ct.ptr, S.R.ptr, (size_t)kc);
    LrParams<real_t> L;
    L.A = c.A; L.lda = c.lda; L.pre = S.R.ptr; L.ldpre = (size_t)kc;
    L.Tc = S.T.ptr; L.ldt = (size_t)kc; L.pos0 = n_full;
    L.Bt = S.Bt.ptr; L.ldbt = ldbt; L.lam_eig = E.Lam.ptr;
    L.kt = kt; L.kc = kc; L.koff = k_side_self; L.rotated = 1;
    L.indptr = X.p.ptr; L.indices = X.i.ptr; L.values = X.v.ptr; L.bias_sub = c.bias_sub;
    L.lam = c.lam; L.lam_last = c.lam_last;
    L.scale_lam = c.scale_lam ? 1 : 0; L.scale_lam_sideinfo = c.scale_lam_sideinfo ? 1 : 0;
    L.scale_bias_const = 0; L.p_side = p_self; L.collective = 1;
    if (dev.row_counter.n < ROW_COUNTER_INTS) const_cast<DeviceInfo &>(dev).row_counter.alloc(ROW_COUNTER_INTS);
    HIP_CHECK(hipMemsetAsync(dev.row_counter.ptr + 8, 0, 4 * sizeof(int), st));
    // rows sorted by length: (64, 128] entries -> 8 blocks (single precision only), (32, 64] -> 4, the rest -> 2
    const int n_gt64 = X.rows_longer_than(64, X.nrows), n_gt32 = X.rows_longer_than(32, X.nrows);
    auto lr_launch = [&](auto kern, int nb_, int wps, int first, int last, int counter) {
        if (last <= first) return;
        LrParams<real_t> Lc = L;
        Lc.row_first = first; Lc.nrows = last; Lc.counter = dev.row_counter.ptr + 8 + counter;
        const size_t smem = 4 * lowrank_lds_elems<real_t>(nb_) * sizeof(real_t);
        if (smem > 48 * 1024)
            HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        const int grid = std::min((last - first + 3) / 4, dev.num_cus * wps);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, Lc, X.desc.ptr);
    };
    // (two wavefronts per SIMD at least: a single wave cannot keep the matrix pipe issuing, see gramk_kernels.hpp)
#ifdef CMFREC_HIP_FLOAT
    lr_launch(lowrank_rows_kernel<real_t, 8, 2>, 8, 2, n_full, std::max(n_full, n_gt64), 0);
    lr_launch(lowrank_rows_kernel<real_t, 4, 3>, 4, 3, std::max(n_full, n_gt64), std::max(n_full, n_gt32), 1);
#else
    lr_launch(lowrank_rows_kernel<real_t, 4, 2>, 4, 2, std::max(n_full, n_gt64), std::max(n_full, n_gt32), 1);
#endif
#ifdef CMFREC_HIP_FLOAT
    lr_launch(lowrank_rows_kernel<real_t, 2, 4>, 2, 4, std::max(n_full, n_gt32), X.nrows, 2);
#else
    lr_launch(lowrank_rows_kernel<real_t, 2, 3>, 2, 3, std::max(n_full, n_gt32), X.nrows, 2);
#endif
    HIP_CHECK(hipGetLastError());
    // x[:kc] = Q x~[:kc]: one GEMM over the light rows (in processing order), then back to their rows
    launch_gemm<false>(dev, n_light, kc, kc, (real_t)1, S.T.ptr, (size_t)kc, E.Qt.ptr, (size_t)kc, S.R.ptr, (size_t)kc);
    hipLaunchKernelGGL(scatter_rows_kernel<real_t>, grid1d((size_t)n_light * kc), dim3(256), 0, st, c.A, c.lda, X.desc.ptr, n_full, S.R.ptr,
                       (size_t)kc, kc, (size_t)n_light);
    HIP_CHECK(hipGetLastError());
    return 0;
}

// Plain closed-form rows (factors_closed_form, common.c:978-1070: no side information) with few entries against many unknowns: the
// row's matrix is lam_i I + sum_j B_j B_j^T -- already diagonal plus a rank-s update, so the low-rank kernel applies without any
// rotation (lowrank_kernels.hpp, !rotated / !collective): an s x s system instead of a k_t^3 / 3 factorisation.  Config 3's users
// (k_t = 129, double): 38 % of the rows hold at most 64 entries.  -1 when the path does not apply.
#ifndef CMF_LR_MAX_F64
#define CMF_LR_MAX_F64 96      // 64: the four-block build only (the A/B build of round 5)
#endif
int launch_plain_lowrank(const DeviceInfo &dev, const CholCall &c, const SparseShard &X)
{
    const int lr_sw = switches().lowrank;       // CMFREC_HIP_LOWRANK: 0 / 1 force the path off / on
    const int kt = c.kt;
    // (double precision, k_t >= 128: rows of 65..96 entries on a six-block build, 21 tiles at one wavefront per SIMD -- the full
    //  path costs such a row the 36-tile rank-k update, a 133 KB round trip through HBM and the eight-block factorisation)
    const int lr_type_max = (sizeof(real_t) == 4) ? 128 : 64;
    const int lr_max = (kt >= 256 && lr_type_max >= 128) ? 128 : (kt >= 128 ? (sizeof(real_t) == 8 ? CMF_LR_MAX_F64 : 64) : 32);
    const int n_rows = X.n_nonempty;                                  // rows without entries stay as they are (common.c:3270)
    const int n_full = X.rows_longer_than(lr_max, n_rows);
    const int n_light = n_rows - n_full;
    const bool ok = lr_sw != 0 && !X.weighted() && c.koff == 0 && c.X2 == nullptr && !c.rhs_only &&
                    c.values_override == nullptr && !c.nonneg && !dev.nonneg_now && dev.l1_now == (real_t)0 && dev.l1_last_now == (real_t)0 &&
                    kt <= 320 && (lr_sw == 1 ? kt >= 40 : (kt >= 96 && n_light >= 2048));
    if (!ok || n_light <= 0) return -1;
    CholCall cf = c;
    cf.row_limit = n_full;
    const int rc = (n_full > 0) ? launch_chol(dev, cf, &X) : 0;
    if (rc) return rc;
    hipStream_t st = dev.stream;
    LrParams<real_t> L;
    L.A = c.A; L.lda = c.lda; L.pre = nullptr; L.ldpre = 0; L.Tc = nullptr; L.ldt = 0; L.pos0 = n_full;
    L.Bt = c.B; L.ldbt = c.ldb; L.lam_eig = nullptr;
    L.kt = kt; L.kc = 0; L.koff = 0; L.rotated = 0;
    L.indptr = X.p.ptr; L.indices = X.i.ptr; L.values = X.v.ptr; L.bias_sub = c.bias_sub;
    L.lam = c.lam; L.lam_last = c.lam_last;
    L.scale_lam = c.scale_lam ? 1 : 0; L.scale_lam_sideinfo = 0; L.scale_bias_const = c.scale_bias_const ? 1 : 0; L.p_side = 0; L.collective = 0;
    if (dev.row_counter.n < ROW_COUNTER_INTS) const_cast<DeviceInfo &>(dev).row_counter.alloc(ROW_COUNTER_INTS);
    HIP_CHECK(hipMemsetAsync(dev.row_counter.ptr + 8, 0, 4 * sizeof(int), st));
    const int n_gt64 = X.rows_longer_than(64, n_rows), n_gt32 = X.rows_longer_than(32, n_rows);
    auto lr_launch = [&](auto kern, int nb_, int wps, int first, int last, int counter) {
        if (last <= first) return;
        LrParams<real_t> Lc = L;
        Lc.row_first = first; Lc.nrows = last; Lc.counter = dev.row_counter.ptr + 8 + counter;
        const size_t smem = 4 * lowrank_lds_elems<real_t>(nb_) * sizeof(real_t);
        if (smem > 48 * 1024)
            HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        const int grid = std::min((last - first + 3) / 4, dev.num_cus * wps);
        poison_lds(st, dev.num_cus);
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, Lc, X.desc.ptr);
    };
#ifdef CMFREC_HIP_FLOAT
    lr_launch(lowrank_rows_kernel<real_t, 8, 2>, 8, 2, n_full, std::max(n_full, n_gt64), 0);
    lr_launch(lowrank_rows_kernel<real_t, 4, 3>, 4, 3, std::max(n_full, n_gt64), std::max(n_full, n_gt32), 1);
    lr_launch(lowrank_rows_kernel<real_t, 2, 4>, 2, 4, std::max(n_full, n_gt32), n_rows, 2);
#else
    if (lr_max > 64) lr_launch(lowrank_rows_kernel<real_t, 6, 1>, 6, 1, n_full, std::max(n_full, n_gt64), 0);
    lr_launch(lowrank_rows_kernel<real_t, 4, 2>, 4, 2, std::max(n_full, n_gt64), std::max(n_full, n_gt32), 1);
    lr_launch(lowrank_rows_kernel<real_t, 2, 3>, 2, 3, std::max(n_full, n_gt32), n_rows, 2);
#endif
    HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace cmfhip

using namespace cmfhip;

// The symmetric eigen-decomposition of the low-rank path on its own (tests/test_gpu_operators.py::test_sym_eig,
// tools/microbench/eig_probe.py): A [n, n] symmetric -> Q [n, n] (Q[i][c] = component i of eigenvector c), lam [n] (clamped at
// zero); method 0 = tridiagonalisation + QL (eig_kernels.hpp), 1 = the one-workgroup Jacobi kernel.  ms: device time of `reps` runs.
extern "C" int cmfrec_hip_sym_eig(int n, const real_t *A, real_t *Q, real_t *lam, int method, int reps, double *ms)
{
    return guarded([&]() {
        if (n < 2 || n > EIG_MAX_N) { g_last_error = "cmfrec_hip_sym_eig: 2 <= n <= 320"; return 2; }
        DeviceInfo dev;
        init_device(dev, -1);
        DevBuf<real_t> dA, dQ, dQt, dL;
        DevBuf<double> W, V, D, E, Tau;
        DevBuf<int> info;
        const size_t nn = (size_t)n * n;
        dA.upload(A, nn, dev.stream); dQ.alloc(nn); dQt.alloc(nn); dL.alloc((size_t)n);
        W.alloc(nn); V.alloc(nn); D.alloc((size_t)n); E.alloc((size_t)n); Tau.alloc((size_t)n); info.alloc(1);
        HIP_CHECK(hipMemsetAsync(info.ptr, 0, sizeof(int), dev.stream));
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
        const bool wide = n > 288;
        const int rows = wide ? 32 : 64;
        const size_t smem = ((size_t)n * rows + 4 * (size_t)n) * sizeof(double);
        auto kern = wide ? eig_ql_rows_kernel<real_t, 32> : eig_ql_rows_kernel<real_t, 64>;
        HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        for (int r = 0; r < std::max(reps, 1) + 1; r++) {
            if (r == 1) HIP_CHECK(hipEventRecord(e0, dev.stream));
            if (method == 0 || method == 2) {        // (2: only the tridiagonalisation inside the timed runs -- where the time goes)
                hipLaunchKernelGGL(eig_tridiag_kernel<real_t>, dim3(1), dim3(EIG_TRIDIAG_THREADS), 0, dev.stream, dA.ptr, n, W.ptr, D.ptr, E.ptr, Tau.ptr);
                if (method == 0 || r == 0)
                    hipLaunchKernelGGL(kern, dim3((n + rows - 1) / rows), dim3(64), smem, dev.stream, n, W.ptr, D.ptr, E.ptr, Tau.ptr, dQ.ptr, dQt.ptr,
                                       (size_t)n, dL.ptr, info.ptr);
            } else
                hipLaunchKernelGGL(jacobi_eig_kernel<real_t>, dim3(1), dim3(1024), 0, dev.stream, dA.ptr, n, W.ptr, V.ptr, dQ.ptr, dQt.ptr, (size_t)n,
                                   dL.ptr, 30, sizeof(real_t) == 4 ? 1e-9 : 1e-13);
            HIP_CHECK(hipGetLastError());
        }
        HIP_CHECK(hipEventRecord(e1, dev.stream));
        HIP_CHECK(hipEventSynchronize(e1));
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
        if (ms) *ms = (double)t / std::max(reps, 1);
        int h_info = 0;
        HIP_CHECK(hipMemcpyAsync(&h_info, info.ptr, sizeof(int), hipMemcpyDeviceToHost, dev.stream));
        dQ.download(Q, nn, dev.stream); dL.download(lam, (size_t)n, dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        if (h_info != 0) { g_last_error = "cmfrec_hip_sym_eig: a QL iteration did not converge"; return 4; }
        return 0;
    });
}
