/*
 * cmfrec_hip.h -- C ABI of the MI355X-native ALS factor-update path behind cmfrec's interface.
 *
 * One shared object per precision, like the reference (setup.py:389-412 builds wrapper_double /
 * wrapper_float from the same sources):
 *     libcmfrec_hip_double.so : real_t = double        libcmfrec_hip_float.so : real_t = float
 * (compile the including translation unit with -DCMFREC_HIP_FLOAT for the float library).
 * int_t is the 32-bit `int` of the reference's default build (src/cmfrec.h:300-305); CSR/CSC
 * offsets are size_t (src/cmfrec.h:991).  Dense matrices are row-major; missing optional pointers
 * are NULL and optional sizes 0 (include/cmfrec.h.in:238-241).
 *
 * Three levels, from the outside in:
 *   1. the two drop-in fit entry points, byte-for-byte the reference's positional signatures;
 *   2. the operator boundary: one factor update with host buffers (what the reference's internal
 *      optimizeA* functions compute), used by the parity tests;
 *   3. a device-resident session (factors + CSR/CSC stay in HBM across half-iterations), which is
 *      what level 1 drives and what bench.py times.
 *
 * Return codes (include/cmfrec.h.in:210-213): 0 ok, 1 out of memory (host or device), 2 invalid or
 * unsupported input, 3 interrupted.  Additionally 4 = HIP runtime failure (no usable gfx950
 * device, kernel launch error); there is NO CPU fallback.
 */
#ifndef CMFREC_HIP_H
#define CMFREC_HIP_H
#include <stddef.h>
#include <stdint.h>
#include <stdbool.h>

#ifdef CMFREC_HIP_FLOAT
typedef float real_t;
#else
typedef double real_t;
#endif
typedef int int_t;

#ifdef __cplusplus
extern "C" {
#endif

/* ============================ level 1: drop-in fit entry points ============================ */

/* Replaces fit_collective_implicit_als, /root/reference/src/cmfrec.h:1893-1921 (body
 * src/collective.c:9375-10207; documented in include/cmfrec.h.in:927-959).
 * Supported: CG / PCG / Cholesky, optionally with DENSE side information U[m_u, p] / II[n_i, q] without NaN
 * (m_u, n_i may exceed m, n: A, B then have max(m, m_u) / max(n, n_i) rows, src/collective.c:9437-9440) (k_user, k_item, k_main, w_main, w_user, w_item as the reference): Cholesky
 * (optimizeA_collective_implicit, src/collective.c:5971-6244) or block CG / PCG
 * (collective_block_cg_implicit, :2905-3303).  No adjust_weight.
 * or SPARSE side information as COO triplets (U_row / U_col / U_sp / nnz_U and the I_* twins; missing = absent, rows
 * within X's; collective.c:1849-2131 / :2905-3303 with u_vec_sp); nonneg / nonneg_C / nonneg_D with max_cd_steps
 * (solve_nonneg, common.c:2131-2179; k_t <= 140 / 199), l1_lam (solve_elasticnet, :2228-2294) and the per-matrix
 * lam_unique / l1_lam_unique (entries 2..5: A, B, C, D; :9793-9809, :9855-10016); dense U / II with NaN (= missing) under the
 * plain Cholesky solver; precompute_for_predictions; NA_as_zero_U / NA_as_zero_I (sparse U / I whose absent entries are zeros,
 * on the rows / columns of X): the dense route on the zero-filled matrix up to CMFREC_HIP_ZEROFILL_MAX_GB (default 8 GB), on the
 * triplets themselves beyond it (single device; cmfrec_hip_session_set_sideinfo_sparse_zeros).  Anything else returns 2. */
int_t fit_collective_implicit_als(
    real_t *A, real_t *B,
    real_t *C, real_t *D,
    bool reset_values, int_t seed,
    real_t *U_colmeans, real_t *I_colmeans,
    int_t m, int_t n, int_t k,
    int_t ixA[], int_t ixB[], real_t *X, size_t nnz,
    real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique,
    real_t *U, int_t m_u, int_t p,
    real_t *II, int_t n_i, int_t q,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    int_t I_row[], int_t I_col[], real_t *I_sp, size_t nnz_I,
    bool NA_as_zero_U, bool NA_as_zero_I,
    int_t k_main, int_t k_user, int_t k_item,
    real_t w_main, real_t w_user, real_t w_item,
    real_t *w_main_multiplier,
    real_t alpha, bool adjust_weight, bool apply_log_transf,
    int_t niter, int nthreads,
    bool verbose, bool handle_interrupt,
    bool use_cg, int_t max_cg_steps, bool precondition_cg, bool finalize_chol,
    bool nonneg, int_t max_cd_steps, bool nonneg_C, bool nonneg_D,
    bool precompute_for_predictions,
    real_t *precomputedBtB,
    real_t *precomputedBeTBe,
    real_t *precomputedBeTBeChol,
    real_t *precomputedCtUbias);

/* Replaces fit_collective_explicit_als, /root/reference/src/cmfrec.h:1851-1892 (body
 * src/collective.c:7263-9370; include/cmfrec.h.in:885-926).
 * Supported: sparse X with missing-as-NA, biases/centering/scale_lam,
 * CG / PCG or Cholesky, optional DENSE side information U[m_u, p] / II[n_i, q] without NaN (m_u, n_i may exceed
 * m, n: rows known from side information only are fitted to it alone and get a zero bias, :4967-5101, :8296)
 * (Cholesky: collective_closed_form_block, src/collective.c:1223-1847; CG: collective_block_cg, :2134-2903),
 * k_main/k_user/k_item, w_user/w_item; also SPARSE side information as COO triplets (missing = absent, rows within
 * X's; collective_closed_form_block / collective_block_cg with u_vec_sp, :1636-1653, :1719-1731, :2609-2621); nonneg /
 * nonneg_C / nonneg_D with max_cd_steps (solve_nonneg, common.c:2131-2179), l1_lam (solve_elasticnet) and the per-matrix
 * lam_unique / l1_lam_unique (user bias, item bias, A, B, C, D; :8178-8219, :8367-8423, :8649-8654, :8820-8825, :9066-9238);
 * add_implicit_features with Ai, Bi, w_implicit (:8448-8534, :1704-1771, :2301-2304, :2624-2643, :2862-2868; Cholesky or
 * CG / PCG, dense or no side information inside X, not with nonneg / L1 / precompute_for_predictions); dense U / II with
 * NaN (= missing) under the Cholesky solver with unscaled lambda; scale_bias_const (scaling_biasA / scaling_biasB are
 * outputs); observation weights (weight, one per entry of X; src/common.c:1098-1291, :679-723); NA_as_zero_X on sparse X for
 * the model without side information (optimizeA Case 3, src/common.c:3118-3205; src/collective.c:8573-8600); dense X
 * (Xfull [m, n], NaN = missing, weight [m, n]) for the model without side information, with the reference's choice of solver
 * per half-step (optimizeA Cases 1-2, src/common.c:2787-3116); NA_as_zero_U / NA_as_zero_I (sparse U / I whose absent entries
 * are zeros, on the rows / columns of X): the dense route on the zero-filled matrix up to CMFREC_HIP_ZEROFILL_MAX_GB (default
 * 8 GB), on the triplets themselves beyond it (single device; cmfrec_hip_session_set_sideinfo_sparse_zeros).  Anything else
 * returns 2. */
int_t fit_collective_explicit_als(
    real_t *biasA, real_t *biasB,
    real_t *A, real_t *B,
    real_t *C, real_t *D,
    real_t *Ai, real_t *Bi,
    bool add_implicit_features,
    bool reset_values, int_t seed,
    real_t *glob_mean,
    real_t *U_colmeans, real_t *I_colmeans,
    int_t m, int_t n, int_t k,
    int_t ixA[], int_t ixB[], real_t *X, size_t nnz,
    real_t *Xfull,
    real_t *weight,
    bool user_bias, bool item_bias, bool center,
    real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique,
    bool scale_lam, bool scale_lam_sideinfo, bool scale_bias_const,
    real_t *scaling_biasA, real_t *scaling_biasB,
    real_t *U, int_t m_u, int_t p,
    real_t *II, int_t n_i, int_t q,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    int_t I_row[], int_t I_col[], real_t *I_sp, size_t nnz_I,
    bool NA_as_zero_X, bool NA_as_zero_U, bool NA_as_zero_I,
    int_t k_main, int_t k_user, int_t k_item,
    real_t w_main, real_t w_user, real_t w_item, real_t w_implicit,
    int_t niter, int nthreads,
    bool verbose, bool handle_interrupt,
    bool use_cg, int_t max_cg_steps, bool precondition_cg, bool finalize_chol,
    bool nonneg, int_t max_cd_steps, bool nonneg_C, bool nonneg_D,
    bool precompute_for_predictions,
    bool include_all_X,
    real_t *B_plus_bias,
    real_t *precomputedBtB,
    real_t *precomputedTransBtBinvBt,
    real_t *precomputedBtXbias,
    real_t *precomputedBeTBeChol,
    real_t *precomputedBiTBi,
    real_t *precomputedTransCtCinvCt,
    real_t *precomputedCtCw,
    real_t *precomputedCtUbias);

/* ============================ level 2: operator boundary (host buffers) ==================== */

/* One iALS half-step; replaces optimizeA_implicit, src/cmfrec.h:1014-1027 / src/common.c:3305-3421.
 * A[m,lda] in/out, B[n,ldb]; the k solved columns start at A / B.  BtB_out (k*k) optional. */
int cmfrec_hip_optimizeA_implicit(
    real_t *A, size_t lda, const real_t *B, size_t ldb,
    int_t m, int_t n, int_t k,
    const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
    real_t lam,
    bool use_cg, bool precondition_cg, int_t max_cg_steps,
    real_t *BtB_out);

/* One explicit-feedback half-step on sparse X (missing = NA, unweighted); replaces optimizeA
 * Case 4, src/cmfrec.h:986-1008 / src/common.c:3209-3302.  bias_sub (length n, optional) is
 * subtracted from the stored values on the fly, replacing the host sweeps collective.c:8566-8570 /
 * :8750-8754. */
int cmfrec_hip_optimizeA_explicit(
    real_t *A, size_t lda, const real_t *B, size_t ldb,
    int_t m, int_t n, int_t k,
    const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
    const real_t *bias_sub,
    real_t lam, real_t lam_last, bool scale_lam, bool scale_bias_const,
    bool use_cg, bool precondition_cg, int_t max_cg_steps);

/* The same with observation weights (optimizeA Case 4 with weight != NULL, src/common.c:3268-3299 -> the weighted branches
 * of factors_closed_form :985-1012 and factors_explicit_cg / _pcg :1126-1135, :1162-1171, :1222-1254): weight[nnz] in the
 * entry order of Xcsr; wsum[m] (optional) = the lambda multipliers of scale_lam the driver passes (wsumA,
 * src/collective.c:7978-8008), NULL = every row's own sum of weights.  weight == NULL: cmfrec_hip_optimizeA_explicit. */
int cmfrec_hip_optimizeA_explicit_weighted(
    real_t *A, size_t lda, const real_t *B, size_t ldb,
    int_t m, int_t n, int_t k,
    const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr, const real_t *weight, const real_t *wsum,
    const real_t *bias_sub,
    real_t lam, real_t lam_last, bool scale_lam, bool scale_bias_const,
    bool use_cg, bool precondition_cg, int_t max_cg_steps);

/* Dense full side-information update (the C / D step); replaces optimizeA Case 1,
 * src/common.c:2793-2991.  do_B: Xfull is [n, ldX] and used transposed (common.c:2852-2855). */
int cmfrec_hip_optimizeA_dense_full(
    real_t *A, size_t lda, const real_t *B, size_t ldb,
    int_t m, int_t n, int_t k,
    const real_t *Xfull, size_t ldX, bool do_B,
    real_t lam, real_t lam_last, bool scale_lam);

/* Collective (block-system) half-step with dense full U, Cholesky; replaces optimizeA_collective
 * general branch, src/cmfrec.h:1646-1683 / src/collective.c:5566-5968 ->
 * collective_closed_form_block (:1223-1847). */
int cmfrec_hip_optimizeA_collective(
    real_t *A, size_t lda, const real_t *B, size_t ldb, const real_t *C,
    int_t m, int_t m_u, int_t n, int_t p,
    int_t k, int_t k_main, int_t k_user, int_t k_item,
    const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
    const real_t *bias_sub,
    const real_t *U,
    real_t lam, real_t w_user, real_t lam_last,
    bool scale_lam, bool scale_lam_sideinfo);

/* Factors of rows that were not part of the fit, one batched pass (level 2 under the two drop-in entry points below):
 * the closed-form row update of the fit with B (and C) fixed -- collective_factors_warm / _cold and their implicit
 * twins, src/collective.c:3309-4087.  X: COO (ixA, ixB, X, nnz) or CSR (Xcsr_*, m_x+1 offsets), values already
 * shifted by the global mean / scaled by alpha; biasB is subtracted inside the gather.  U raw, U_colmeans subtracted on
 * the device.  A is [max(m_x, m_u), k_user+k+k_main], biasA (optional) one value per row.  lam_x: what the implicit
 * model puts on the diagonal of the X block (see factors_collective_implicit_multiple below); BtB_pre (implicit,
 * lam included) and TransCtCinvCt_pre ([p, k_user+k]) replace the matrices otherwise rebuilt from B and C. */
int cmfrec_hip_factors_multiple(
    real_t *A, real_t *biasA, int_t m_x, int_t m_u, int_t p, const real_t *U, const real_t *U_colmeans,
    const int_t ixA[], const int_t ixB[], const real_t *X, size_t nnz,
    const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
    const real_t *B, int_t n, const real_t *C, const real_t *biasB,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t lam_bias, real_t lam_x, real_t w_user,
    bool implicit, bool scale_lam, bool scale_lam_sideinfo, bool scale_bias_const,
    const real_t *BtB_pre, const real_t *TransCtCinvCt_pre,
    /* sparse side information instead of U (NULL): COO triplets or CSR over the m_u rows, missing = absent */
    const int_t U_row[], const int_t U_col[], const real_t *U_sp, size_t nnz_U,
    const size_t U_csr_p[], const int_t U_csr_i[], const real_t *U_csr,
    bool nonneg /* solve_nonneg instead of the Cholesky solves, 10 (k_user+k+k_main[+1]) sweeps at most */);
int cmfrec_hip_factors_multiple_l1(
    real_t *A, real_t *biasA, int_t m_x, int_t m_u, int_t p, const real_t *U, const real_t *U_colmeans,
    const int_t ixA[], const int_t ixB[], const real_t *X, size_t nnz,
    const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
    const real_t *B, int_t n, const real_t *C, const real_t *biasB,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t lam_bias, real_t lam_x, real_t w_user,
    bool implicit, bool scale_lam, bool scale_lam_sideinfo, bool scale_bias_const,
    const real_t *BtB_pre, const real_t *TransCtCinvCt_pre,
    /* sparse side information instead of U (NULL): COO triplets or CSR over the m_u rows, missing = absent */
    const int_t U_row[], const int_t U_col[], const real_t *U_sp, size_t nnz_U,
    const size_t U_csr_p[], const int_t U_csr_i[], const real_t *U_csr,
    bool nonneg /* solve_nonneg instead of the Cholesky solves, 10 (k_user+k+k_main[+1]) sweeps at most */,
    /* L1 penalty of the row systems / of the bias unknown, after the w_main rescaling (solve_elasticnet,
     * /root/reference/src/common.c:2228-2294; collective.c:3571-3931); TransCtCinvCt_pre must be NULL */
    real_t l1_lam, real_t l1_lam_bias);
/* The same with the remaining inputs of the explicit model's new rows (implicit: they must be NULL):
 * weight: observation weights of sparse X, one per entry in the order of the triplets / of Xcsr; every entry's rank-1 term
 *   and right-hand side are weighted, and under scale_lam the row's lambda multiplier is the sum of its weights
 *   (src/common.c:693-715; a row whose sum is below the type's epsilon comes out as zeros).
 * Xfull [m_x, n], NaN = not observed, instead of the sparse forms (both: return 2), weight_full [m_x, n] its weights, read
 *   only where Xfull is present.  The block is compacted on the device into the triplets of its present entries
 *   (dense_rows_device.hpp), glob_mean_full subtracted there, in blocks of rows of at most 1 GB; a row solves on its present
 *   entries, a row of NaN is a row without observations.
 * Bi [n, k+k_main]: implicit features.  Every row system gets BiTBi on the X block and w_implicit * sum_{j observed} Bi_j
 *   on the right-hand side (src/collective.c:1704-1707, :1757-1771), rows without observations included (no "cold"
 *   solution).  BiTBi_pre replaces w_implicit_gram * Bi^T Bi, built on the device otherwise -- two weights because the
 *   reference's batch driver builds the matrix before the row function divides w_implicit by w_main (:11016-11020, :3706-3714).
 * TransBtBinvBt_pre [n, k+k_main (+1 with biasA)]: without weights, nonneg, L1, side information and Bi the rows of Xfull
 *   without a NaN are (x - glob_mean_full - biasB)^T TransBtBinvBt (src/common.c:736-758), whatever lambda it was built with. */
int cmfrec_hip_factors_multiple_ex(
    real_t *A, real_t *biasA, int_t m_x, int_t m_u, int_t p, const real_t *U, const real_t *U_colmeans,
    const int_t ixA[], const int_t ixB[], const real_t *X, size_t nnz,
    const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
    const real_t *B, int_t n, const real_t *C, const real_t *biasB,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t lam_bias, real_t lam_x, real_t w_user,
    bool implicit, bool scale_lam, bool scale_lam_sideinfo, bool scale_bias_const,
    const real_t *BtB_pre, const real_t *TransCtCinvCt_pre,
    const int_t U_row[], const int_t U_col[], const real_t *U_sp, size_t nnz_U,
    const size_t U_csr_p[], const int_t U_csr_i[], const real_t *U_csr,
    bool nonneg, real_t l1_lam, real_t l1_lam_bias,
    const real_t *weight, const real_t *Xfull, const real_t *weight_full, real_t glob_mean_full,
    const real_t *Bi, real_t w_implicit, real_t w_implicit_gram, const real_t *BiTBi_pre,
    const real_t *TransBtBinvBt_pre);

/* Replace factors_collective_explicit_multiple / factors_collective_implicit_multiple,
 * /root/reference/src/cmfrec.h:2004-2047 and :2048-2071 (bodies src/collective.c:10865-11174, :11176-11340): same
 * positional parameters, same return codes (0 ok, 1 out of memory, 2 invalid / unsupported).  Supported: sparse X
 * (COO or CSR), dense U without NaN (rows beyond m get the side-information-only solution, rows beyond m_u the plain
 * one), user bias, lam_unique, scale_lam / scale_lam_sideinfo / scale_bias_const, w_main / w_user, alpha and
 * apply_log_transf; sparse side information (COO or CSR; not together with scale_lam_sideinfo in the explicit
 * version); nonneg (solve_nonneg on every row system) and L1 penalties (not both).  The explicit version also takes
 * Xfull [m, n] with NaN = missing instead of the sparse forms (both: 2), weight (per triplet, in the order of Xcsr, or
 * [m, n] with Xfull) and Bi with add_implicit_features (BiTBi read when given, else w_implicit Bi^T Bi built on the
 * device; the right-hand side carries w_implicit / w_main, as in the reference) -- see cmfrec_hip_factors_multiple_ex.
 * Returned with 2: NA_as_zero_X / _U, binary side information, NaN in U, and the combinations in which the reference's
 * own rows are not the solution of the model: weights of a sparse X with side information or
 * implicit features together with glob_mean / biasB; a dense row without observations together with U and U_colmeans.
 * Of the precomputed matrices BtB (implicit), TransCtCinvCt, TransBtBinvBt (complete dense rows of the model without
 * side information) and BiTBi are read -- the ones that change the result; the others (BtB of the explicit model
 * among them) are rebuilt on the device from B and C.
 * Two details of the reference that are kept: (1) without a precomputed BtB the implicit version puts the lam of the
 * call, *not* lam / w_main, on the diagonal of the X block (collective.c:11270-11280) while the k_user block gets
 * lam / w_main; (2) the side-information-only solution of the explicit version under scale_lam_sideinfo scales lam by
 * p on all but the last of the k_user+k unknowns (:3397-3411). */
int_t factors_collective_explicit_multiple(
    real_t *A, real_t *biasA, int_t m,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U, bool NA_as_zero_X,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *Ub, int_t m_ubin, int_t pbin,
    real_t *C, real_t *Cb,
    real_t glob_mean, real_t *biasB,
    real_t *U_colmeans,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *Xfull, int_t n,
    real_t *weight,
    real_t *B,
    real_t *Bi, bool add_implicit_features,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique,
    bool scale_lam, bool scale_lam_sideinfo,
    bool scale_bias_const, real_t scaling_biasA,
    real_t w_main, real_t w_user, real_t w_implicit,
    int_t n_max, bool include_all_X,
    real_t *BtB, real_t *TransBtBinvBt, real_t *BtXbias, real_t *BeTBeChol, real_t *BiTBi,
    real_t *TransCtCinvCt, real_t *CtCw, real_t *CtUbias, real_t *B_plus_bias,
    int nthreads);

int_t factors_collective_implicit_multiple(
    real_t *A, int_t m,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *B, int_t n,
    real_t *C,
    real_t *U_colmeans,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t l1_lam, real_t alpha, real_t w_main, real_t w_user,
    real_t w_main_multiplier,
    bool apply_log_transf,
    real_t *BeTBe, real_t *BtB, real_t *BeTBeChol, real_t *CtUbias,
    int nthreads);

/* The same half-step with SPARSE side information: U as CSR over its m_u rows (missing attributes are simply absent,
 * !NA_as_zero_U).  Explicit (implicit = false: collective_closed_form_block, src/collective.c:1223-1847) or implicit
 * model (collective_closed_form_block_implicit, :1849-2131), Cholesky.  A is overwritten ([m, lda], first
 * k_user+k+k_main columns). */
int cmfrec_hip_optimizeA_collective_sparse(
    real_t *A, size_t lda, const real_t *B, size_t ldb, const real_t *C,
    int_t m, int_t m_u, int_t n, int_t p,
    int_t k, int_t k_main, int_t k_user, int_t k_item,
    const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
    const real_t *bias_sub,
    const size_t Ucsr_p[], const int_t Ucsr_i[], const real_t *Ucsr,
    real_t lam, real_t w_user, real_t lam_last,
    bool scale_lam, bool scale_lam_sideinfo, bool implicit);

/* ============================ level 3: device-resident session ============================= */

typedef struct cmfrec_hip_session cmfrec_hip_session;

typedef struct cmfrec_hip_model {
    int32_t implicit;                 /* 1: iALS (optimizeA_implicit), 0: explicit (optimizeA / _collective) */
    int32_t m, n, k;                  /* global sizes, shared factors */
    int32_t k_main, k_user, k_item;
    int32_t user_bias, item_bias;     /* explicit only: bias rides as an extra column (collective.c:7651-7663) */
    int32_t scale_lam, scale_lam_sideinfo;
    int32_t use_cg, precondition_cg, max_cg_steps;
    int32_t p, q, m_u, n_i;           /* dense side info widths / rows (0 = none) */
    real_t lam, w_user, w_item;
    /* row-block shard owned by this process (single GPU: [0,m) and [0,n)) */
    int32_t row_begin, row_end, col_begin, col_end;
    /* m, n are the rows of A and B.  Side information may describe more users / items than X has rows / columns
     * (m_u > m_x: the reference's m_max = max(m, m_u), src/collective.c:7332-7335): then m_x / n_x give the shape
     * of X; 0 = same as m / n.  Rows beyond m_x are solved from their side information alone. */
    int32_t m_x, n_x;
} cmfrec_hip_model;

/* device < 0: use the current HIP device. Returns NULL on failure (see cmfrec_hip_last_error). */
cmfrec_hip_session *cmfrec_hip_session_create(const cmfrec_hip_model *model, int device);
void cmfrec_hip_session_destroy(cmfrec_hip_session *s);
const char *cmfrec_hip_last_error(void);
/* return code (1 out of memory, 2 invalid input, 4 HIP failure) that goes with the last NULL from cmfrec_hip_session_create */
int cmfrec_hip_last_error_code(void);

/* CSR of the local user rows [row_begin,row_end) (indptr rebased to 0, column ids global) and CSC
 * of the local item columns [col_begin,col_end) (row ids global).  Host buffers; copied to HBM. */
int cmfrec_hip_session_set_X(cmfrec_hip_session *s,
                             const size_t *csr_p, const int_t *csr_i, const real_t *csr_v,
                             const size_t *csc_p, const int_t *csc_i, const real_t *csc_v);
/* Same from the COO triplet (host buffers): CSR and CSC are built in HBM by a stable sort, i.e. with the
 * entry order of coo_to_csr_and_csc (src/helpers.c:1375-1491); values become (x - subtract) * alpha on the
 * way (centring src/common.c:3603-3613; confidence src/collective.c:9606-9611).  Only for sessions that own
 * all rows and columns. */
/* Multi-GPU overlap (optional, after set_X with the same CSR): cut the local rows of A into `nparts` contiguous parts
 * with their own processing orders.  update('A') then finishes part after part and records one event per part;
 * stream_wait_part makes another stream (the one the all-gather of that part is issued on) wait for it, so the
 * collective of a finished part runs beside the kernels of the following ones.  Sessions without user side
 * information only.  nparts <= 1 removes the split. */
int cmfrec_hip_session_set_A_parts(cmfrec_hip_session *s, const size_t *csr_p, const int_t *csr_i,
                                   const real_t *csr_v, int nparts);
int cmfrec_hip_session_nparts(cmfrec_hip_session *s);
int cmfrec_hip_session_part_range(cmfrec_hip_session *s, int part, int *begin, int *end);   /* local row offsets */
int cmfrec_hip_session_stream_wait_part(cmfrec_hip_session *s, int part, void *stream);

int cmfrec_hip_session_set_X_coo(cmfrec_hip_session *s, const int_t *row, const int_t *col, const real_t *val,
                                 size_t nnz, real_t subtract, real_t alpha);
/* The same with observation weights (explicit model): weight[nnz], one per entry, travels through the same stable sort as
 * the values (weightR / weightC of coo_to_csr_and_csc, src/helpers.c:1375-1491).  Every row solver then weights the entry's
 * rank-1 term and right-hand side (src/common.c:985-1012, :1126-1135, :1162-1171, :1246-1254), scale_lam multiplies lambda by
 * the row's sum of weights (:679-723; src/collective.c:7978-8008) and init_biases takes weighted means (src/common.c:4180-4205,
 * :4672-4692, :4826-4847).  weight == NULL: as cmfrec_hip_session_set_X_coo.  Returns 2 for the implicit model.
 * cmfrec_hip_session_set_X_weighted: the same from host CSR + CSC with their weights in the same entry order. */
int cmfrec_hip_session_set_X_coo_weighted(cmfrec_hip_session *s, const int_t *row, const int_t *col, const real_t *val,
                                          const real_t *weight, size_t nnz, real_t subtract, real_t alpha);
int cmfrec_hip_session_set_X_weighted(cmfrec_hip_session *s,
                                      const size_t *csr_p, const int_t *csr_i, const real_t *csr_v, const real_t *csr_w,
                                      const size_t *csc_p, const int_t *csc_i, const real_t *csc_v, const real_t *csc_w);
/* One shard from a COO triplet already resident in HBM (device pointers): which = 'r': CSR of the local rows, d_key = row -
   row_begin, d_other = global column; 'c': CSC of the local columns, d_key = column - col_begin, d_other = global row.
   Multi-GPU set-up path (the triplets come out of an all-to-all between the ranks); no reference counterpart: the
   reference converts on the host (src/helpers.c:1375-1491). */
int cmfrec_hip_session_set_X_coo_device(cmfrec_hip_session *s, int which, const int_t *d_key, const int_t *d_other,
                                        const real_t *d_val, size_t nnz, real_t subtract, real_t alpha);
/* NA_as_zero for the main matrix (explicit model, sparse X whose absent entries are zeros; plain model on one device): from
 * here on every update('A' / 'B') is optimizeA Case 3 (src/common.c:3118-3205) -- one shared matrix opp^T opp + lambda (x rows
 * under scale_lam), right-hand sides sum_j x_j opp_j over the row's entries plus the constant -sum over ALL opposing rows of
 * (their bias + glob_mean [when center]) x row (src/collective.c:8573-8600, :8756-8787), one factorisation and a triangular
 * solve for every row, with or without entries.  A side with dense complete side information on exactly the rows of X:
 * optimizeA_collective's factorised block matrix (src/collective.c:5607-5617, :5700-5716), closed form only.  X must have been
 * set uncentred. */
int cmfrec_hip_session_set_NA_as_zero_X(cmfrec_hip_session *s, int on, int center, real_t glob_mean);
/* Rows of A (which = 'A') or B ('B') that every update of that matrix leaves at ZERO, bias included, instead of solving them:
 * with NA_as_zero_U / NA_as_zero_I the reference does not solve a row that has neither an entry of X nor an entry of the side
 * information (collective_closed_form_block, src/collective.c:1262-1271; _implicit: :1876-1884), while the zero-filled dense
 * matrix the fit runs on (fit.hip, ZeroFilledSide) would.  count = 0 clears the list. */
int cmfrec_hip_session_set_zero_rows(cmfrec_hip_session *s, int which, const int_t *rows, int count);
/* Rows of A ('A') or B ('B') that take the CLOSED FORM in every update of that matrix, also when the update runs CG for the
 * others: a dense X whose half-step (optimizeA Case 2, src/common.c:2992-3116) has rows missing fewer than 2 k entries (closed form
 * from the precomputed B^T B, factors_closed_form :662, :759-790) next to rows missing more (the solver asked for).  mask: one byte
 * per row of the matrix, non-zero = closed form; NULL clears it.  A CG update then solves every row by CG, keeps a copy, solves
 * every row in closed form and puts the copy back for the rows whose byte is zero.
 * 'C' / 'D' (round 5): the attributes of DENSE side information with NaN, which the session holds as the sparse matrix of its
 * present, centred values (cmfrec_hip_session_set_sideinfo_sparse).  The reference's dense C / D update (optimizeA Cases 1-2 on
 * the transposed matrix, src/common.c:2793-3116) treats an attribute by the number of values it misses; one byte per attribute:
 * 0 = the solver asked for, 1 = closed form (fewer than 2 (k_side + k) missing values, :759-790; the complete attributes of a
 * matrix with at least 75 % complete ones), 2 = CG from zero with k_side + k steps (the other attributes of such a matrix,
 * :2953-2985).  fit_collective_*_als sets them (fit.hip, DenseNanSide::rules). */
int cmfrec_hip_session_set_closed_form_rows(cmfrec_hip_session *s, int which, const unsigned char *mask);
/* The lambda multipliers of the rows of A ('A') / B ('B') under scale_lam, instead of the rows' own sums of weights: a dense X
 * under scale_lam, where a row that misses fewer than 2 k entries keeps the n lam of a complete row (its matrix is the precomputed
 * B^T B + n lam I minus the missing rows, src/common.c:759-790, :3031-3032) while the others take lam times their present entries.
 * The session must hold X with observation weights (unit weights for this use); call after the bias start values.  mult: one
 * value per row of the matrix.
 * 'C' / 'D' (round 5): the multipliers of the attributes of dense side information with NaN under scale_lam (the same rule:
 * the rows of U x lam for an attribute that misses fewer than 2 (k_side + k) values, its present values otherwise); the
 * session puts unit weights on its attribute-major copy of the sparse side information. */
int cmfrec_hip_session_set_lambda_multipliers(cmfrec_hip_session *s, int which, const real_t *mult);
/* Bias start values of the explicit model from the resident X, as initialize_biases_twosided /
 * _onesided (src/common.c:4410-4909, 4265-4289; call sites src/collective.c:8166-8220): written to the
 * session's bias vectors and the bias columns of A / B.  Call after set_X* and set_factors. */
int cmfrec_hip_session_init_biases(cmfrec_hip_session *s, real_t lam_user, real_t lam_item);
/* Copies the resident CSR (which = 'r') or CSC ('c') back: indptr[rows+1], indices[nnz], values[nnz],
 * order[rows] = rows in processing order.  NULL = skip. */
int cmfrec_hip_session_get_X(cmfrec_hip_session *s, int which, size_t *indptr, int_t *indices, real_t *values,
                             int_t *order);
/* Full factor matrices A[m, k_user+k+k_main], B[n, k_item+k+k_main] (+ biasA[m], biasB[n] when the
 * model has them; C[p,k_user+k], D[q,k_item+k]); host buffers.  NULL = leave unchanged. */
int cmfrec_hip_session_set_factors(cmfrec_hip_session *s, const real_t *A, const real_t *B,
                                   const real_t *biasA, const real_t *biasB,
                                   const real_t *C, const real_t *D);
int cmfrec_hip_session_get_factors(cmfrec_hip_session *s, real_t *A, real_t *B,
                                   real_t *biasA, real_t *biasB, real_t *C, real_t *D);
/* Dense side information, already centred by column (host does column means like
 * common.c:4911-4997): U rows [0,m_u), II rows [0,n_i). */
int cmfrec_hip_session_set_sideinfo(cmfrec_hip_session *s, const real_t *U, const real_t *II);
/* Non-negativity constraints: nonneg for A and B, nonneg_C / nonneg_D for the side-information factors.  The closed-form
 * row systems are then solved by the reference's cyclic coordinate descent (solve_nonneg, src/common.c:2131-2179,
 * at most max_cd_steps sweeps, 0 = until converged) and the CG is switched off for that matrix (common.c:725, :2781).
 * The k_t x k_t system lives in LDS: k_t <= 140 (double) / 199 (single). */
/* Row-block shards of the explicit / collective model (one session per GPU): side information restricted to
   the rows of the block -- U_local = rows [row_begin, min(row_end, m_u)) of U, I_local = rows [col_begin, min(col_end, n_i))
   of I (already centred) -- and the C / D update (optimizeA Case 1, src/common.c:2793-2991) cut in two:
   _partial leaves [F_loc^T F_loc | U_loc^T F_loc] in a device buffer (cmfrec_hip_session_device_ptr(s, 'P', &elems, NULL)),
   the caller all-reduces it over the ranks, _finish adds lambda and solves -- the same small system on every rank. */
int cmfrec_hip_session_set_sideinfo_local(cmfrec_hip_session *s, const real_t *U_local, const real_t *I_local);
int cmfrec_hip_session_sideinfo_partial(cmfrec_hip_session *s, int which /* 'C' | 'D' */);
int cmfrec_hip_session_sideinfo_finish(cmfrec_hip_session *s, int which /* 'C' | 'D' */);
int cmfrec_hip_session_set_nonneg(cmfrec_hip_session *s, int nonneg, int nonneg_C, int nonneg_D, int max_cd_steps);
/* Implicit features of the explicit model (add_implicit_features of fit_collective_explicit_als,
 * /root/reference/src/collective.c:7269, :8448-8534): Ai [m, k+k_main] and Bi [n, k+k_main] factorise the binary
 * "was observed" pattern of X with weight w_implicit (already divided by w_main).  After this call the session's
 * updates 'b' (Bi from A) and 'a' (Ai from B) exist, iterate() runs them between D and B like the reference, and the
 * A / B updates carry the extra term (collective.c:1704-1707, :1757-1771).  Ai / Bi may be NULL (start values are never
 * read by the closed-form updates).  Ai / Bi are always closed-form; A / B run Cholesky or the block CG like the rest of
 * the model.  Whole-matrix sessions, dense or no side information. */
int cmfrec_hip_session_set_implicit_features(cmfrec_hip_session *s, real_t w_implicit, const real_t *Ai, const real_t *Bi);
int cmfrec_hip_session_get_implicit_features(cmfrec_hip_session *s, real_t *Ai, real_t *Bi);

/* scale_bias_const of the explicit model (/root/reference/src/collective.c:7555, :8110-8160): rows solved without side
 * information keep the bias' lambda as given (lam_unique[0] / [1], which the caller has multiplied by scaling_biasA /
 * scaling_biasB) instead of scaling it by the row's count (common.c:679-723). */
int cmfrec_hip_session_set_scale_bias_const(cmfrec_hip_session *s, int on);

/* Per-matrix penalties (lam_unique / l1_lam_unique of the fit entry points, /root/reference/src/collective.c:430):
 * six values each in the order user bias, item bias, A, B, C, D, already divided by w_main.  Either pointer may be NULL
 * (that family keeps the scalar of the model / of set_l1).  The A / B updates use [2] / [3] and, for a fitted bias, [0] /
 * [1] on the last unknown (:8649-8654, :8820-8825); C / D use [4] / w_user, [5] / w_item (:8367, :8418); the implicit
 * model ignores [0], [1]. */
int cmfrec_hip_session_set_lam_unique(cmfrec_hip_session *s, const real_t *lam_unique, const real_t *l1_lam_unique,
                                      int max_cd_steps);

/* L1 penalty (one value for every matrix: A, B and the bias columns take l1_lam, C / D l1_lam / w_user, / w_item;
 * scaled per row like lambda).  Systems are then solved by solve_elasticnet (src/common.c:2228-2294), or by
 * solve_nonneg with the penalty on the right-hand side where a non-negativity constraint applies; no CG. */
int cmfrec_hip_session_set_l1(cmfrec_hip_session *s, real_t l1_lam, int max_cd_steps);
/* SPARSE side information as COO triplets (which = 'U': [m_u, p], 'I': [n_i, q]; missing = absent, no centring):
 * CSR by row and CSC by attribute are built on the device.  Cholesky updates: the row's attributes are a second gather
 * source of the row kernel; CG / PCG: a second gathered term of the block CG (generic kernel).  m_u <= rows of X. */
int cmfrec_hip_session_set_sideinfo_sparse(cmfrec_hip_session *s, int which, const int_t *row, const int_t *col,
                                           const real_t *val, size_t nnz);
/* SPARSE side information whose ABSENT ENTRIES ARE ZEROS (NA_as_zero_U / NA_as_zero_I), on every row of the factor matrix
 * (the model's m_u = m / n_i = n; rows without triplets are rows of zeros).  colmeans [p] / [q]: the column means over ALL
 * rows, subtracted from every cell, absent ones included (NULL: none).  The session then behaves as after
 * cmfrec_hip_session_set_sideinfo on the zero-filled, centred dense matrix -- every solver and option of dense side
 * information -- but keeps the triplets alone: the products with that matrix run as sparse products plus a rank-one
 * correction (side_zeros_kernels.hpp), work and memory proportional to nnz.  Triplets that repeat a position add up.
 * Returns 2 on a row-block shard (local side information, parts of A, cmfrec_hip_session_sideinfo_partial): those keep to
 * the dense matrix. */
int cmfrec_hip_session_set_sideinfo_sparse_zeros(cmfrec_hip_session *s, int which /* 'U' | 'I' */, const int_t *row,
                                                 const int_t *col, const real_t *val, size_t nnz, const real_t *colmeans);
/* The two products of that form alone, host buffers: U~ = U_sparse - 1 colmeans^T of `rows` rows and p attributes,
 *   UM  [count, kc] = alpha (U~ M)[first : first + count, :]   when M [p, kc] is given (else NULL),
 *   UtF [p, kc]     = U~^T F[:, :kc]                            when F [rows, ldF] is given (else NULL).
 * kc <= 320.  Bitwise reproducible: no floating-point atomics, every sum in a fixed order. */
int cmfrec_hip_side_zeros_products(int_t rows, int_t p, int_t kc, const int_t *row, const int_t *col, const real_t *val,
                                   size_t nnz, const real_t *colmeans, const real_t *M, real_t alpha, int_t first,
                                   int_t count, real_t *UM, const real_t *F, size_t ldF, real_t *UtF);

/* One update of the local block, asynchronous on the session stream. which: 'A','B','C','D'.
 * use_cholesky != 0 forces the Cholesky solver for this call (finalize_chol). */
int cmfrec_hip_session_update(cmfrec_hip_session *s, int which, int use_cholesky);
/* niter full ALS iterations in the reference's order C, D, B, A (collective.c:8334-8898 /
 * :9827-10045) on a single-GPU session. */
int cmfrec_hip_session_iterate(cmfrec_hip_session *s, int niter, int finalize_chol);
int cmfrec_hip_session_sync(cmfrec_hip_session *s);

/* Device pointers for torch.distributed / RCCL plumbing (factor all-gather between half-steps).
 * which 'A'/'B': the [rows, ld] matrix incl. the bias column; returns NULL if unknown. */
void *cmfrec_hip_session_device_ptr(cmfrec_hip_session *s, int which, size_t *rows, size_t *ld);
void *cmfrec_hip_session_stream(cmfrec_hip_session *s);
/* To be called after the local block of `which` was refreshed on all ranks (after the all-gather):
 * refreshes what is derived from the full matrix (bias vectors). */
int cmfrec_hip_session_after_gather(cmfrec_hip_session *s, int which);
/* The "precompute_for_predictions" epilogue of the fit drivers (src/collective.c:8936-9249, 10056-10115) from
 * the resident factors.  Host buffers, NULL = skip.  With kp = k + k_main (+1 with a user bias, explicit),
 * kc = k_user + k, kq = k_user + kp:  BtB[kp, kp] (implicit: + lam I);  explicit only: TransBtBinvBt[n, kp],
 * TransCtCinvCt[p, kc];  with user side information: CtCw[kc, kc] (explicit), BeTBe[kq, kq] (implicit),
 * BeTBeChol[kq, kq] (upper triangle = the factor R, M = R^T R).
 * include_all_X (explicit model): use all max(n, n_i) rows of B, else the n columns X has (collective.c:9013).
 * last_step_cholesky: whether the last iteration of the fit used the Cholesky solver (use_cg=false or
 * finalize_chol).  It only matters for quirk Q9 of the reference, which this library reproduces: in the implicit
 * model with user side information, after a CG last step, BeTBe / BeTBeChol carry the UNWEIGHTED C^T C when
 * w_user != 1 (src/collective.c:10077 tests `w_user == 1.` where `!=` was meant); see DESIGN.md, Parity. */
int cmfrec_hip_session_precompute(cmfrec_hip_session *s, int last_step_cholesky, int include_all_X, real_t *BtB,
                                  real_t *TransBtBinvBt, real_t *BeTBe, real_t *BeTBeChol, real_t *CtCw,
                                  real_t *TransCtCinvCt);

/* HIP-event time (ms) and launch count of the row-update kernels of `which` ('A' or 'B') since
 * the last reset; synchronises the stream. */
int cmfrec_hip_session_kernel_time(cmfrec_hip_session *s, int which, double *ms, long *launches);
/* Per-kernel figures of the CG row-update launches of `which`.  Rows are scheduled in six nnz bins,
 * one persistent launch each: bin 1: 257..2048 nnz (8 waves/row), 2: 129..256 (4 waves/row),
 * 3: 65..128 (2 waves/row), 4: 33..64 (1 wave/row), 5: 1..32 (1 wave/row, half tiles, double-buffered
 * gather); bin 0: rows > 2048 nnz, whose CG passes are
 * split over many workgroups (one launch pair per pass; the figure covers the whole sequence).
 * ms = summed HIP-event time of that bin's launches since the last reset. */
int cmfrec_hip_session_bin_stats(cmfrec_hip_session *s, int which, int bin, double *ms, long *launches,
                                 long *rows, unsigned long long *nnz);
/* 1 if the launches of that bin run beside other kernels (few split rows on the second stream; every bin of a block
 * that is updated in parts): their event timings then include the neighbours' work and are not a kernel duration. */
int cmfrec_hip_session_bin_overlaps(cmfrec_hip_session *s, int which, int bin);
/* How the split rows (> 1024 entries) of that side are solved: 0 none, 1 streamed once per CG pass, 2 read once, CG on the
 * row's own Gramian (chosen when few split rows share an opposing row, e.g. a rank's item block of a multi-GPU run). */
int cmfrec_hip_session_vh_mode(cmfrec_hip_session *s, int which);
/* rows of X's CSR ('A') / CSC ('B') shard with at least this many entries are "split rows": their entries are stored sorted
   by the opposing index (a permutation of the row's sums) and take the split-row kernels (1025; double precision: 513 where
   the split rows go through their own Gramian) */
int cmfrec_hip_session_vh_min(cmfrec_hip_session *s, int which);
/* the most recent collective Cholesky half-step: rows solved by the low-rank kernels (0: path not taken) and the
   eigen-decomposition behind them (3 tridiagonalisation + implicit QL, 2 the one-workgroup Jacobi kernel; CMFREC_HIP_EIG=jacobi forces 2) */
int cmfrec_hip_session_lowrank_info(cmfrec_hip_session *s, int *rows, int *eig);
void cmfrec_hip_session_reset_timers(cmfrec_hip_session *s);

/* Batched top-N (the step after the path; the reference ranks one user per call: topN, src/common.c:5127-5380).
 * score(u, i) = A_u . B_i (+ biasB[i]) over the k columns starting at A / B (skip k_user / k_item by offsetting the
 * pointers), items in the user's exclusion list (CSR over the nu users, each list sorted ascending; NULL = none)
 * are skipped, the n_top best item ids per user are returned in descending score (ties: lower id first), -1 where
 * fewer than n_top items remain.  out_scores (optional) holds the scores as defined above; the reference adds
 * glob_mean + biasA[u] afterwards, which does not change the order.  k <= 272 (every width the library fits),
 * n_top <= min(128, n); beyond that return code 2.  k <= 64 runs the register-resident kernel, wider models the MFMA kernel
 * (CMFREC_HIP_TOPN=wide: that one for every k).  One call = one ranker (below) made, used once and destroyed: B is uploaded
 * on every call. */
int cmfrec_hip_topN_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k,
                          const real_t *biasB, const size_t excl_p[], const int_t excl_i[], int_t n_top,
                          int_t *out_ids, real_t *out_scores);

/* A ranking handle that keeps the item side on the device: ranking a user base in batches uploads B once, not once per batch.
 * create: B [n, ldb], the k scored columns start at B (skip k_item by offsetting the pointer) and are uploaded packed; biasB
 * optional; device < 0: the current device.  NULL on failure (cmfrec_hip_last_error / cmfrec_hip_last_error_code).
 * topN: the semantics, limits and return codes of cmfrec_hip_topN_batch for nu users A [nu, lda]; uploads the users' factors
 * and exclusion lists, ranks, downloads.  The handle's device buffers are reused from call to call and grow on demand; calls on
 * one handle must not overlap.
 * kernel_ms: HIP-event time of the ranking kernel of the most recent topN call (return code 2 before the first).
 * launch_shape: how that kernel was launched -- users that share one pass over the items (16 for the register-resident kernel,
 * 16 to 64 for the MFMA kernel, by what fits the LDS) and workgroups; the items are streamed once per 16..64 users. */
typedef struct cmfrec_hip_ranker cmfrec_hip_ranker;
cmfrec_hip_ranker *cmfrec_hip_ranker_create(const real_t *B, size_t ldb, int_t n, int_t k, const real_t *biasB, int device);
int cmfrec_hip_ranker_topN(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu,
                           const size_t excl_p[], const int_t excl_i[], int_t n_top,
                           int_t *out_ids, real_t *out_scores);
/* Top-N over per-user candidate lists (the batch form of the reference's include_ix, src/common.c:5134-5260): user u is ranked
 * over the items of its own list, cand_i[cand_p[u] .. cand_p[u + 1]) (CSR over the nu users, required), and gets exactly what
 * cmfrec_hip_ranker_topN returns with every item outside the list in the user's exclusion list: the same score, order, tie rule
 * (lower id first, whatever the order of the list), -1 / -inf filling and limits (code 2 beyond them; cand_p == NULL: code 2).
 * Each list is ascending and free of duplicates, like the exclusion lists; an unsorted list or one with duplicates gives an
 * unspecified tie order or a repeated id.  An id outside [0, n) never enters (decided on the device).  A list may be empty, shorter
 * or longer than n_top.  excl_p / excl_i (optional, as in ranker_topN) may come along -- the reference refuses both on one user,
 * the batch form takes both: a candidate that is also in the user's exclusion list is dropped.
 * One wavefront ranks one user at a time from the handle's packed copy of B and gathers only the listed rows (every k <= 272
 * on the same kernel, topn_cand_kernels.hpp); a score has the value cmfrec_hip_score_pairs returns for the same two rows with
 * biasA = NULL and glob_mean = 0.  kernel_ms / launch_shape report that kernel after such a call: the wavefronts of a workgroup
 * (a wavefront holds one user at a time) and the workgroups.  cmfrec_hip_topN_candidates_batch is create, one such call, destroy. */
int cmfrec_hip_ranker_topN_candidates(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu,
                                      const size_t cand_p[], const int_t cand_i[],
                                      const size_t excl_p[], const int_t excl_i[], int_t n_top,
                                      int_t *out_ids, real_t *out_scores);
int cmfrec_hip_topN_candidates_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k,
                                     const real_t *biasB, const size_t cand_p[], const int_t cand_i[],
                                     const size_t excl_p[], const int_t excl_i[], int_t n_top,
                                     int_t *out_ids, real_t *out_scores);
/* Ranks of held-out items: for user u and every t of its held-out list held_i[held_p[u] .. held_p[u + 1]) (CSR over the nu users,
 * required, held_p[0] = 0; each list ascending and free of duplicates),
 *   out_rank = #{ i in [0, n) : i not in the user's exclusion list, score(u, i) not NaN, score(u, i) before score(u, t) }
 * in the order of cmfrec_hip_ranker_topN (higher score first, then lower id): the 0-based place of t in the user's full ranking;
 * the user's other held-out items count like any item.  out_rank = -1 where t is outside [0, n), in the user's exclusion list,
 * or scores NaN (decided on the device).  out_scores (optional) [held_p[nu]]: score(u, t), NaN where out_rank = -1.  out_pool
 * (optional) [nu]: the number of items of the user's ranking (not excluded, not NaN).  No n_top limit: every place up to n - 1
 * is counted.  excl_p / excl_i as in ranker_topN (each list ascending; a repeated id counts once).
 * One pass over the items per workgroup of 16..64 users on the MFMA, as the wide top-N kernel (topn_rank_kernels.hpp), for every
 * k <= 272; a user with more held-out items than one pass holds (by what fits the LDS, 1024 at the most) costs its workgroup
 * further passes.  A score has the bits the wide top-N kernel gives the pair: with CMFREC_HIP_TOPN=wide,
 * topN(...)[u, out_rank] == t and the scores are equal bit for bit wherever out_rank < n_top; against the default top-N kernel
 * of k <= 64 the two agree up to rounding (a near tie may swap neighbours).  All results are integer counts and do not depend on
 * the launch shape.  Code 2 when held_p == NULL (and, for ranks_batch, k > 272); the outputs are then untouched.
 * kernel_ms / launch_shape report the rank kernel after such a call (its threshold and exclusion steps included): users per
 * workgroup and workgroups.  Top-N, candidate and rank calls may be interleaved on one handle.
 * cmfrec_hip_ranks_batch is create, one such call, destroy. */
int cmfrec_hip_ranker_ranks(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu,
                            const size_t held_p[], const int_t held_i[],
                            const size_t excl_p[], const int_t excl_i[],
                            int_t *out_rank, real_t *out_scores, int_t *out_pool);
int cmfrec_hip_ranks_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k,
                           const real_t *biasB, const size_t held_p[], const int_t held_i[],
                           const size_t excl_p[], const int_t excl_i[],
                           int_t *out_rank, real_t *out_scores, int_t *out_pool);
/* Neighbours of the ranker's own rows ("items like this item"; a ranker over the user factors: "users like this user").
 * query_ids [nq]: rows of the ranker's matrix, each in [0, n); only the ids are uploaded, the query tile is gathered from the
 * resident rows.  metric: 0 = dot product, score(q, i) = B_q . B_i -- without the bias, even when the ranker holds one;
 * 1 = cosine, score(q, i) = ((B_q . B_i) * rn[i]) * rn[q], two multiplications in that order, rn[i] = 1 / sqrt(sum_f B[i, f]^2)
 * (IEEE square root and division, made by the first cosine call of a ranker and resident from then on; inverse_norms downloads
 * them).  A row whose sum of squares is zero, NaN or infinite has rn = NaN: it is nobody's neighbour and, as a query, has none.
 * The query itself is skipped; excl_p / excl_i (optional): further exclusion lists, CSR over the nq queries, each ascending, as
 * in ranker_topN.  Order, ties (lower id first), -1 / -inf filling and limits are those of ranker_topN.  Every k <= 272 runs the
 * MFMA kernel's body (topn_similar_kernels.hpp).  Code 2 with a message, decided on the host with the outputs untouched: a
 * query id outside [0, n) or query_ids == NULL, a metric other than 0 / 1, exclusion lists that are not a CSR, k > 272 or
 * n_top > min(128, n).  nq == 0: code 0, nothing written.  kernel_ms / launch_shape report the neighbour kernel after such a
 * call (the norm kernel is outside the timed interval).  Neighbour, top-N, candidate and rank calls may be interleaved on one
 * handle.  cmfrec_hip_similar_batch is create (without a bias), one such call, destroy. */
int cmfrec_hip_ranker_similar(cmfrec_hip_ranker *r, const int_t *query_ids, int_t nq, int metric,
                              const size_t excl_p[], const int_t excl_i[], int_t n_top,
                              int_t *out_ids, real_t *out_scores);
int cmfrec_hip_similar_batch(const real_t *B, size_t ldb, int_t n, int_t k, const int_t *query_ids, int_t nq, int metric,
                             const size_t excl_p[], const int_t excl_i[], int_t n_top, int_t *out_ids, real_t *out_scores);
/* Deep lists and next pages: top-N without the limit of 128, and "items 21-40" without ranking the first 20 again.
 * topN_deep: the n_top best of every user for any 1 <= n_top <= n (k <= 272 as everywhere; otherwise code 2, "needs k <= 272 and
 * 1 <= n_top <= n", before anything touches the device).  Order, tie rule (lower id first), -1 / -inf filling, exclusion lists, NaN
 * rule and out_scores == NULL are those of cmfrec_hip_ranker_topN.  The [nu, n_top] result is built on the device in pages: page p
 * is one pass of the MFMA kernel's body (topn_after_kernels.hpp) that admits only the pairs strictly behind the last (score, id) of
 * page p - 1 in the total order, read from the result itself -- no host round trip between the pages, one download at the end.  The
 * result does not depend on the page length (128 by default; CMFREC_HIP_TOPN_PAGE = 1 .. 512 is a test hook).  Every k runs the MFMA
 * kernel: a score has the bits cmfrec_hip_ranker_ranks and the MFMA top-N kernel give the pair, so for n_top <= 128 the result is
 * that of cmfrec_hip_ranker_topN for k > 64 (for every k under CMFREC_HIP_TOPN=wide) bit for bit.  kernel_ms: the interval around
 * all the pages; launch_shape: the last page's.  pages: the launches and the page length of the most recent topN_deep call on the
 * handle (code 2 before the first).  cmfrec_hip_topN_deep_batch is create, one topN_deep call, destroy.
 * topN_after: the next n_top <= min(128, n) items of every user strictly behind its cursor (after_scores[u], after_ids[u]) --
 * [nu] each, typically the last column of the previous page; both NULL: the first page (one without the other: code 2).  A cursor
 * of (+inf, -1) starts at the top; the (-inf, -1) an exhausted user's page ends with gives -1 / -inf throughout; so does a NaN
 * cursor score.  The cursor's item need not be rankable: it may have been excluded since.  The cursor compares score bits, so the
 * scores must come from this route: topN_after, topN_deep, ranker_ranks, or ranker_topN on the MFMA kernel (k > 64, or
 * CMFREC_HIP_TOPN=wide).  The default kernel of k <= 64 rounds a score differently in the last bits: with a cursor from it, an item
 * that nearly ties with the cursor's may be returned again or left out.
 * Deep, next-page, top-N, candidate, rank and neighbour calls may be interleaved on one handle. */
int cmfrec_hip_ranker_topN_deep(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu,
                                const size_t excl_p[], const int_t excl_i[], int_t n_top,
                                int_t *out_ids, real_t *out_scores);
int cmfrec_hip_ranker_topN_after(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu,
                                 const size_t excl_p[], const int_t excl_i[],
                                 const int_t *after_ids, const real_t *after_scores, int_t n_top,
                                 int_t *out_ids, real_t *out_scores);
int cmfrec_hip_topN_deep_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k,
                               const real_t *biasB, const size_t excl_p[], const int_t excl_i[], int_t n_top,
                               int_t *out_ids, real_t *out_scores);
int cmfrec_hip_ranker_pages(cmfrec_hip_ranker *r, int *pages, int *page_len);
int cmfrec_hip_ranker_inverse_norms(cmfrec_hip_ranker *r, real_t *out);
int cmfrec_hip_ranker_kernel_ms(cmfrec_hip_ranker *r, double *ms);
int cmfrec_hip_ranker_launch_shape(cmfrec_hip_ranker *r, int *users_per_workgroup, int *workgroups);

/* The full ranking of a few users across the whole device.  The MFMA ranking kernel gives a whole pass
 * over the items to the workgroup that owns a tile of 16..64 users, so a request of one user runs on one compute unit.  With the
 * split setting on, the items of a full ranking are cut into slices, every (user tile, slice) is a workgroup of its own, and a
 * second kernel on the same stream merges the slices' lists per user.
 * set_split: slices = -1 off (the default: exactly the launches of a handle that never heard of it), 0 = the number
 * cmfrec_hip_topn_split_plan chooses per call, >= 1 = that many, held to what the planner allows.  The setting affects the full
 * ranking only: cmfrec_hip_ranker_topN without candidates and cmfrec_hip_newrows_topN.  Candidate lists, topN_deep / topN_after,
 * ranks, metrics and similar ignore it.  With the setting on, EVERY k takes the MFMA arithmetic, also k <= 64: ids and scores are
 * bit for bit those of the unsplit MFMA kernel (CMFREC_HIP_TOPN=wide for k <= 64) whatever the number of slices; against the
 * register-resident kernel of k <= 64 the scores agree up to rounding.  Limits and return codes as cmfrec_hip_ranker_topN.
 * slices: the item slices of the most recent ranking launch on the handle, 1 when it was not split (return code 2 before the
 * first call).  cmfrec_hip_ranker_kernel_ms spans the slice pass and the merge; cmfrec_hip_ranker_launch_shape's workgroups are
 * those of the slice pass (user-tile workgroups times slices).
 * cmfrec_hip_newrows_set_split: the same setting for the ranker inside a new-rows handle, made now or later.
 * cmfrec_hip_topn_split_plan: the planner, host arithmetic only (no device is touched): for nu users, n items, k factors and lists
 * of n_top on a device of num_cus compute units and elements of sizeof_real bytes (4 or 8), requested = 0 to choose or >= 1 to
 * ask: *slices >= 1 and *slice_items, a multiple of 128 with slices * slice_items >= n > (slices - 1) * slice_items.  It splits
 * only while the user tiles alone leave workgroup slots of the device empty, and never into slices shorter than a measured
 * minimum.  Return code 2 for arguments outside cmfrec_hip_ranker_topN's limits. */
int cmfrec_hip_ranker_set_split(cmfrec_hip_ranker *r, int slices);
int cmfrec_hip_ranker_slices(cmfrec_hip_ranker *r, int *slices);
int cmfrec_hip_topn_split_plan(int_t nu, int_t n, int_t k, int_t n_top, int num_cus, size_t sizeof_real, int requested,
                               int *slices, int *slice_items);
void cmfrec_hip_ranker_destroy(cmfrec_hip_ranker *r);

/* New rows against a model that stays on the device: factors and top-N of users who were not part of the fit, batch after
 * batch, without uploading B (C, Bi, biasB, the precomputed matrices) or rebuilding the Gramians per call, and -- for the ranking --
 * without the factors or the users' own items leaving the device.  The handle sits at the level of
 * factors_collective_explicit_multiple / factors_collective_implicit_multiple (which are create, factors, destroy): the fields
 * carry the reference's names and go through the same rescaling (lam_unique, scaling_biasA, the division by w_main, ...); what
 * those two refuse the handle refuses, with the same messages and return codes.
 * model: B [max(n, n_max) with include_all_X, else n; k_item+k+k_main]; C [p, k_user+k] or NULL; user_bias: the rows have a bias
 *   unknown (the drop-in call: biasA given); Bi [n, k+k_main] with add_implicit_features.  implicit = 1 reads alpha,
 *   w_main_multiplier, apply_log_transf and BtB, and not glob_mean, biasB, Bi, the scale_* flags, lam_unique or TransBtBinvBt.  Of the
 *   precomputed matrices BtB (implicit), TransBtBinvBt, BiTBi and TransCtCinvCt are read when not NULL.  Everything is copied to
 *   the device by create; the caller's arrays may go away afterwards.
 * batch: X as triplets (X, ixA, ixB, nnz), CSR (Xcsr_*, m+1 offsets) or Xfull [m, n] with NaN = not observed (explicit model);
 *   weight in the form of X; U [m_u, p] dense, or sparse as triplets / CSR; values as the caller has them (the handle subtracts
 *   glob_mean, applies log / alpha).  Rows out: max(m, m_u).
 * create: NULL on failure (cmfrec_hip_last_error / cmfrec_hip_last_error_code); device < 0: the current device.
 * factors: A [max(m, m_u), k_user+k+k_main], biasA one value per row (explicit model with user_bias; may be NULL).
 * topN: solves the batch like factors, then ranks its rows [0, max(m, m_u)) straight from the device factors -- columns
 *   [k_user, k_user+k+k_main) against the columns of B from k_item, + biasB -- with the semantics, limits and return codes of
 *   cmfrec_hip_ranker_topN (k+k_main <= 272, n_top <= min(128, items): otherwise 2, and the handle stays usable).  Rows that only
 *   have attributes are ranked like the rest.  exclude_seen: every row skips the items of its own X (sparse, or the present
 *   entries of Xfull); excl_p / excl_i: further lists per row in the ranker's form (CSR over the batch's rows, each sorted
 *   ascending); both: their union.  out_ids / out_scores [rows, n_top]; A / biasA optional outputs -- NULL: the factors never
 *   leave the device.  The ranker is made by the first topN call from the device copy of the items and holds a second, packed
 *   copy of their scored columns (ldb = the ranking kernels' padded width, as in cmfrec_hip_ranker_create).
 * topN_candidates: topN over each row's candidate list, cand_p / cand_i (CSR over the batch's rows, required, each list ascending
 *   and free of duplicates), with the semantics of cmfrec_hip_ranker_topN_candidates; exclude_seen and excl_p / excl_i as in topN
 *   -- a candidate among the row's own items or in its list is dropped.  The batch is solved exactly as in topN; the candidate
 *   lists are uploaded, nothing else enters or leaves the device.  What topN refuses is refused with the same message.
 * ranks: the ranks of each row's held-out items held_p / held_i (CSR over the batch's rows, required), with the semantics of
 *   cmfrec_hip_ranker_ranks; exclude_seen and excl_p / excl_i as in topN -- a held-out item among the row's own items or in its
 *   list gets -1.  The batch is solved exactly as in topN; the held-out lists go up, out_rank / out_scores [held_p[rows]] and
 *   out_pool [rows] (the last two optional) come down.  What topN refuses is refused with the same message.
 * impute: the explicit model's imputation of a dense batch (impute_X_collective_explicit below, without the per-call model work):
 *   solves the batch like factors, then Xout [m, n] = batch->Xfull with every NaN replaced by
 *   A_r . B_c + glob_mean + biasA[r] + biasB[c] from the device factors (columns [k_user, k_user+k+k_main) against the columns of
 *   B from k_item, its first n rows); every present entry keeps its bits.  Xout may be batch->Xfull itself.  The fill runs block of rows by
 *   block of rows on the matrix cores and skips the rows (and tiles) without a NaN; a batch without any NaN is copied without
 *   solving.  A / biasA: optional outputs as in topN.  Return code 2, with a message, and the handle stays usable: an implicit
 *   model, a batch whose X is not Xfull, m <= 0; whatever factors refuses for the batch is refused with the same message.
 * predict: solves the batch like factors, then scores the n_pairs chosen pairs (row[i], col[i]) straight from the device factors,
 *   the resident items and their bias, with the rule of cmfrec_hip_scorer_predict below (explicit or implicit by the model):
 *   row indexes the batch's rows [0, max(m, m_u)), col the items [0, n) -- [0, max(n, n_max)) with include_all_X; a pair outside
 *   gets the fallback value.  A / biasA optional outputs as in topN.  What factors refuses for the batch is refused with the same
 *   message and code, out is left alone and the handle stays usable.  The return codes of factors (0, 1, 2, 3).
 * kernel_ms: HIP-event times of the most recent call -- its solve phase (uploads of the batch, shard build, row solves; 0 after
 *   an impute call that found no NaN) and, after a topN, the ranking kernel, after an impute, the fill kernel summed over the
 *   blocks, after a predict, the scoring kernel summed over the blocks (0 after a factors call); 2 before the first call.
 * Missing-as-zero models (the explicit model; cmfrec_hip_newrows_model_ex and cmfrec_hip_newrows_create_ex below).  NA_as_zero_X: every one of
 *   the n cells of a row of a SPARSE batch counts, an absent one as a zero of weight 1 with the target -glob_mean - biasB_j; a dense
 *   Xfull batch ignores the field, as the reference does.  NA_as_zero_U: an absent attribute of a SPARSE U is a zero (minus its
 *   column mean).  The handle builds B^T B, C^T C, BtXbias and CtUbias itself on the device (items beyond n, with include_all_X,
 *   count with glob_mean only).  Without observation weights every row of such a batch shares one matrix: the batch is one
 *   gather-sum over the triplets and one product with that matrix's inverse.  Refused with code 2 (per batch: the handle stays
 *   usable): either field with nonneg, an L1 penalty, implicit features, scale_bias_const or the implicit model; NA_as_zero_X
 *   with a sparse U whose absent entries are missing (NA_as_zero_U = 0), with weights together with side information, or with
 *   dense U on other rows than the batch's (m_u != m).
 * Calls on one handle must not overlap; a handle belongs to the device it was made on. */
typedef struct cmfrec_hip_newrows_model {
    int32_t implicit;
    int32_t n, n_max, include_all_X;
    int32_t p;
    int32_t user_bias, add_implicit_features;
    int32_t k, k_user, k_item, k_main;
    int32_t scale_lam, scale_lam_sideinfo, scale_bias_const;
    int32_t nonneg, apply_log_transf;
    real_t glob_mean, lam, l1_lam, scaling_biasA, w_main, w_user, w_implicit, alpha, w_main_multiplier;
    const real_t *B, *C, *U_colmeans, *biasB, *Bi;
    const real_t *lam_unique, *l1_lam_unique;            /* the reference's six values each, or NULL */
    const real_t *BtB, *TransBtBinvBt, *BiTBi, *TransCtCinvCt;
} cmfrec_hip_newrows_model;
/* The model with the missing-as-zero options behind it: `base` first, so the struct is cmfrec_hip_newrows_model with the two fields at
 * its end; cmfrec_hip_newrows_model itself keeps its layout for the callers compiled against it.  0 / 0: cmfrec_hip_newrows_create. */
typedef struct cmfrec_hip_newrows_model_ex {
    cmfrec_hip_newrows_model base;
    int32_t NA_as_zero_X, NA_as_zero_U;
} cmfrec_hip_newrows_model_ex;
typedef struct cmfrec_hip_newrows_batch {
    int32_t m, m_u;
    const real_t *U;
    const int_t *U_row, *U_col; const real_t *U_sp; size_t nnz_U;
    const size_t *U_csr_p; const int_t *U_csr_i; const real_t *U_csr;
    const real_t *X; const int_t *ixA, *ixB; size_t nnz;
    const size_t *Xcsr_p; const int_t *Xcsr_i; const real_t *Xcsr;
    const real_t *Xfull;
    const real_t *weight;
} cmfrec_hip_newrows_batch;
typedef struct cmfrec_hip_newrows cmfrec_hip_newrows;
int cmfrec_hip_sizeof_newrows_model(void);
cmfrec_hip_newrows *cmfrec_hip_newrows_create(const cmfrec_hip_newrows_model *model, int device);
int cmfrec_hip_newrows_factors(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, real_t *A, real_t *biasA);
int cmfrec_hip_newrows_topN(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, int exclude_seen,
                            const size_t excl_p[], const int_t excl_i[], int_t n_top,
                            int_t *out_ids, real_t *out_scores, real_t *A, real_t *biasA);
int cmfrec_hip_newrows_topN_candidates(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch,
                                       const size_t cand_p[], const int_t cand_i[], int exclude_seen,
                                       const size_t excl_p[], const int_t excl_i[], int_t n_top,
                                       int_t *out_ids, real_t *out_scores, real_t *A, real_t *biasA);
int cmfrec_hip_newrows_ranks(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch,
                             const size_t held_p[], const int_t held_i[], int exclude_seen,
                             const size_t excl_p[], const int_t excl_i[],
                             int_t *out_rank, real_t *out_scores, int_t *out_pool, real_t *A, real_t *biasA);
int cmfrec_hip_newrows_impute(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, real_t *Xout, real_t *A, real_t *biasA);
int cmfrec_hip_newrows_predict(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, const int_t *row, const int_t *col,
                               size_t n_pairs, real_t *out, real_t *A, real_t *biasA);
int cmfrec_hip_newrows_kernel_ms(cmfrec_hip_newrows *h, double *solve_ms, double *rank_ms);
int cmfrec_hip_newrows_set_split(cmfrec_hip_newrows *h, int slices);   /* see cmfrec_hip_ranker_set_split */
void cmfrec_hip_newrows_destroy(cmfrec_hip_newrows *h);
/* One-shot form of a missing-as-zero batch: cmfrec_hip_newrows_create, one cmfrec_hip_newrows_factors, destroy -- the level-2
 * call beside cmfrec_hip_factors_multiple_ex for models with NA_as_zero_X / NA_as_zero_U set.  The codes of factors.
 * create_ex: cmfrec_hip_newrows_create with the two options; every other call of the handle is the same. */
/* naz_launch_waves: the wavefronts of the most recent launch of the missing-as-zero right-hand-side kernel on this handle (0: none
 * yet) -- what the test hook CMFREC_HIP_NAZ_WAVES caps (measurement and tests, like cmfrec_hip_evalset_launch_waves). */
int cmfrec_hip_newrows_naz_launch_waves(cmfrec_hip_newrows *h, int *waves);
int cmfrec_hip_sizeof_newrows_model_ex(void);
cmfrec_hip_newrows *cmfrec_hip_newrows_create_ex(const cmfrec_hip_newrows_model_ex *model, int device);
int cmfrec_hip_factors_multiple_naz(const cmfrec_hip_newrows_model_ex *model, const cmfrec_hip_newrows_batch *batch, real_t *A, real_t *biasA);

/* Replaces impute_X_collective_explicit, /root/reference/src/cmfrec.h:2071-2103 (body src/collective.c:11351-11544; the Python class's
 * CMF.transform): the NaN of Xfull [m, n] replaced in place by the predictions from the factors of its rows -- the same
 * positional parameters, the same return codes.  It is cmfrec_hip_newrows_create, one cmfrec_hip_newrows_impute, destroy; what
 * factors_collective_explicit_multiple refuses (NA_as_zero_U, Ub / Cb, ...) is refused here with the same messages.  A matrix
 * without NaN returns 0 untouched.  The precomputed matrices are read as in factors_collective_explicit_multiple. */
int_t impute_X_collective_explicit(
    int_t m, bool user_bias,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *Ub, int_t m_ubin, int_t pbin,
    real_t *C, real_t *Cb,
    real_t glob_mean, real_t *biasB,
    real_t *U_colmeans,
    real_t *Xfull, int_t n,
    real_t *weight,
    real_t *B,
    real_t *Bi, bool add_implicit_features,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique,
    bool scale_lam, bool scale_lam_sideinfo,
    bool scale_bias_const, real_t scaling_biasA,
    real_t w_main, real_t w_user, real_t w_implicit,
    int_t n_max, bool include_all_X,
    real_t *BtB,
    real_t *TransBtBinvBt,
    real_t *BeTBeChol,
    real_t *BiTBi,
    real_t *TransCtCinvCt,
    real_t *CtCw,
    real_t *CtUbias,
    real_t *B_plus_bias,
    int nthreads);

/* Predictions for chosen (row, col) pairs with both factor matrices resident on the device (the evaluation loop after a fit:
 * millions of pairs against one model).  With a = A[row, 0 .. kk) and b = B[col, 0 .. kk) -- A and B point at the first scored
 * column: skip k_user / k_item by offsetting the pointers, kk = k + k_main --
 *   explicit:  row in [0, m) and col in [0, n):  a . b + biasA[row] + biasB[col] + glob_mean   (a missing bias adds nothing)
 *              otherwise:                        glob_mean + (biasA[row] if 0 <= row < m) + (biasB[col] if 0 <= col < n)
 *   implicit:  row in [0, m) and col in [0, n):  a . b;   otherwise NaN
 * The dot product is accumulated in the working precision, in an order that depends on kk alone: a pair's bits do not depend on
 * its position in the call, on the other pairs or on the block size.  Pairs out of range are decided on the device.
 * create: uploads the kk scored columns of A [m, lda] and B [n, ldb] packed and zero-padded to 16 bytes, and the biases (each
 *   optional); implicit != 0 selects the implicit rule (biases and glob_mean are then ignored, given or not: a . b alone); device < 0: the
 *   current device.  NULL on failure (cmfrec_hip_last_error / cmfrec_hip_last_error_code): 2 for m, n or kk < 1, a leading
 *   dimension below kk or a missing matrix.
 * predict: out[i] for the pairs (row[i], col[i]), i < n_pairs; the pairs go up and the values come down in blocks of at most 2^24
 *   pairs (CMFREC_HIP_PREDICT_BLOCK: test hook for that size).  The handle's buffers are reused and grow on demand; n_pairs = 0
 *   returns 0.  Calls on one handle must not overlap.
 * kernel_ms: HIP-event time of the scoring kernel over the blocks of the most recent predict call (2 before the first). */
typedef struct cmfrec_hip_scorer cmfrec_hip_scorer;
cmfrec_hip_scorer *cmfrec_hip_scorer_create(const real_t *A, size_t lda, int_t m, const real_t *B, size_t ldb, int_t n, int_t kk,
                                            const real_t *biasA, const real_t *biasB, real_t glob_mean, int implicit, int device);
int cmfrec_hip_scorer_predict(cmfrec_hip_scorer *s, const int_t *row, const int_t *col, size_t n_pairs, real_t *out);
int cmfrec_hip_scorer_kernel_ms(cmfrec_hip_scorer *s, double *ms);
void cmfrec_hip_scorer_destroy(cmfrec_hip_scorer *s);

/* Squared and absolute error on held-out pairs, reduced on the device.  An evaluation set -- row, col,
 * the held-out value x and an optional weight per pair -- goes to the device once and stays there; an evaluation then is the
 * scoring kernel of cmfrec_hip_scorer_predict ending in a reduction instead of a store, and a download of this one record.
 * With p the prediction of a pair (the value cmfrec_hip_scorer_predict returns for it, bit for bit), in double precision in
 * either library  e = (double)p - (double)x  and  w = weight ? (double)weight : 1.  Two classes of pairs:
 *   [0] scored:    row in [0, m) and col in [0, n)
 *   [1] fallback:  explicit rule, the pair outside the model, p the fallback value
 * and per class n (pairs), sum_w, sum_we = sum w e, sum_wabs = sum w |e|, sum_wsq = sum w e^2, max_abs = max |e|.  n_skipped: the
 * pairs that add to nothing else -- x is NaN, or, under the implicit rule, the pair is outside the model (its prediction is NaN by
 * definition).  Only NaN skips a pair: an infinite x is counted as it is.  n[0] + n[1] + n_skipped = n_pairs.  The sums are added in
 * an order that depends on the device, the launch shape and the order of the pairs, not on the run: the same call returns the
 * same bytes (no atomics).  cmfrec_amd.metrics.error_metrics turns a record into RMSE, MAE, the mean signed error.
 * evalset_create: uploads the four arrays whole (weight optional); n_pairs = 0 is legal; device < 0: the current device.  NULL
 *   on failure: 2 for a NaN, infinite or negative weight and for a missing row / col / x with n_pairs > 0, 1 when the device has no
 *   room.  The indices are not checked: the kernel decides them as it does for predictions.  The order of the pairs is free; pairs
 *   sorted by row are scored faster (section 3.8).
 * evalset_kernel_ms: HIP-event time of both kernels of the most recent evaluation of the set (2 before the first).
 * evalset_launch_waves: the wavefronts of the scoring launch of the most recent evaluation (0 for a set without pairs; 2 before
 *   the first): what CMFREC_HIP_EVAL_WAVES below caps.
 * scorer_errors: against the scorer's resident matrices, biases, mean and rule; 2 when the set lives on another device.
 * session_errors: against the session's factors as they are on the device (the columns behind k_user / k_item, k + k_main wide,
 *   biasA / biasB where the model has them, the implicit rule for an implicit model); glob_mean is the caller's, the session does
 *   not own one.  Launched on the session's stream behind the updates queued there; synchronises; changes nothing in the session.
 *   2 for a session that does not own all rows and for a set on another device.
 * One set may serve any number of scorers and sessions, one call at a time.
 * CMFREC_HIP_EVAL_WAVES (read per call): at most that many wavefronts, rounded up to whole workgroups, in the scoring launch, so
 *   that a small set gives a wavefront several chunks (test hook; 0: by occupancy). */
typedef struct cmfrec_hip_errors {      /* all classes: [0] scored, [1] fallback */
    uint64_t n[2]; uint64_t n_skipped;
    double sum_w[2], sum_we[2], sum_wabs[2], sum_wsq[2], max_abs[2];
} cmfrec_hip_errors;
typedef struct cmfrec_hip_evalset cmfrec_hip_evalset;
cmfrec_hip_evalset *cmfrec_hip_evalset_create(const int_t *row, const int_t *col, const real_t *x, const real_t *weight, size_t n_pairs,
                                              int device);
int cmfrec_hip_evalset_kernel_ms(cmfrec_hip_evalset *e, double *ms);
int cmfrec_hip_evalset_launch_waves(cmfrec_hip_evalset *e, size_t *waves);
void cmfrec_hip_evalset_destroy(cmfrec_hip_evalset *e);
int cmfrec_hip_scorer_errors(cmfrec_hip_scorer *s, cmfrec_hip_evalset *e, cmfrec_hip_errors *out);
int cmfrec_hip_session_errors(cmfrec_hip_session *s, cmfrec_hip_evalset *e, real_t glob_mean, cmfrec_hip_errors *out);

/* Going back to an earlier iterate.  snapshot: a second set of device buffers, allocated on first use,
 * takes everything cmfrec_hip_session_get_factors and _get_implicit_features return -- A, B, the biases, C, D, Ai, Bi -- by
 * device-to-device copies on the session's stream, behind the updates queued there; a later snapshot overwrites it.  restore:
 * the copies the other way round; the factors then are bit for bit those of the snapshot, and the next update starts from them.
 * Neither synchronises.  2 with a message: restore without a snapshot, and either call on a session that does not own all rows
 * (a shard of a multi-device fit), as cmfrec_hip_session_errors. */
int cmfrec_hip_session_snapshot(cmfrec_hip_session *s);
int cmfrec_hip_session_restore(cmfrec_hip_session *s);

/* Validation while fitting: a held-out set is evaluated where the factors are, between the iterations
 * of fit_collective_explicit_als / fit_collective_implicit_als, and the fit may stop early and return its best iterate.  The
 * signatures of those two functions do not change: the monitor is handed over beforehand,
 *   cmfrec_hip_fit_set_monitor(&mon);  fit_collective_explicit_als(...);
 * It is kept per thread (the struct is copied, the arrays it points to are the caller's) and is consumed by the next of the two
 * fit calls on that thread, whatever that call returns; NULL clears it.  A fit without a monitor runs exactly as before.
 *   evalset      a resident held-out set (cmfrec_hip_evalset_create, the fit's precision), evaluated as
 *                cmfrec_hip_session_errors does: the biases and the global mean of the explicit model, the implicit rule; or
 *   rankset      a resident ranking set (cmfrec_hip_rankset_create below) with its cut-off k_at, evaluated as
 *                cmfrec_hip_session_ranking does.  Exactly one of the two.
 *   metric       what is watched.  From an evalset, both classes of the record together as cmfrec_amd.metrics.error_metrics
 *                forms them: CMFREC_HIP_WATCH_RMSE  sqrt(S(w e^2) / S(w)),  CMFREC_HIP_WATCH_MAE  S(w |e|) / S(w); lower is better.
 *                From a rankset, sum / count of the record: CMFREC_HIP_WATCH_HIT, _PRECISION, _RECALL, _AP, _NDCG, _RR, _AUC
 *                (higher is better) and _MEAN_RANK (lower is better); NaN where no user counts
 *   every        evaluate after iterations every, 2 every, ... (1-based) and after the last one; < 1 counts as 1
 *   patience     stop once that many evaluations in a row have not improved; <= 0: never stop (monitor only)
 *   min_delta    an evaluation improves when it beats the best so far by more than this (the first one always does); NaN never does
 *   restore_best != 0: every improvement takes a cmfrec_hip_session_snapshot, and when the loop ends -- stopped or run to niter --
 *                on a later iterate than the best one, cmfrec_hip_session_restore runs right after the loop, before anything reads
 *                the factors: A, B, the biases, C, D, Ai, Bi and every precompute_for_predictions output then come from the best
 *                iterate.  0: the last iterate is returned, stopped or not.
 *   values       [niter] out, optional: the watched value per iteration, NaN where the iteration was not evaluated or not run
 *   records      [niter] out, optional, with an evalset: the full record per evaluated iteration (the others are zeroed)
 *   rank_records [niter] out, optional, with a rankset: the same
 *   iters_run    out, optional: the iterations that ran;  best_iter  out, optional: the 0-based iteration of the best evaluation,
 *                -1 when none improved (every value NaN)
 * finalize_chol keeps its meaning: the Cholesky pass belongs to iteration niter - 1 alone; a fit that stops before it does not
 * add one, and a fit that ran it but restores an earlier iterate returns conjugate-gradient factors.  An interrupt (return 3)
 * leaves the iterate it was at; iters_run and best_iter are still written.
 * Refused with 2 and a message (cmfrec_hip_last_error), before the fit writes to any of its outputs: niter < 1; an unknown metric;
 * CMFREC_HIP_DEVICES naming several devices or CMFREC_HIP_SHARDED=1 (the sharded driver and every fit that would fall back from
 * it); both sets or none; a metric that does not belong to the set; a set on another device than the fit's; an evalset without a
 * single pair inside the m x n of X whose value is not NaN; a rankset with k + k_main > 272, with a user beyond the rows of X, or
 * in which no user has a held-out item inside the n items that its exclusion list leaves (no user with T > 0).
 * verbose prints the watched value per evaluated iteration.
 * cmfrec_hip_early_stop_step is that rule alone, host only, for the loop above and for tests.  The caller zeroes the struct, sets
 * every / patience / min_delta / higher_is_better and best_iter = -1.  With value == NULL it returns CMFREC_HIP_STEP_EVALUATE when
 * 0-based iteration `iter` of `niter` is one to evaluate, else 0.  With a value it books the evaluation and returns a mask of
 * CMFREC_HIP_STEP_IMPROVED (best / best_iter updated, misses = 0) and CMFREC_HIP_STEP_STOP (misses has reached patience). */
#define CMFREC_HIP_WATCH_RMSE 0
#define CMFREC_HIP_WATCH_MAE 1
#define CMFREC_HIP_WATCH_HIT 2          /* 2 .. 9: from a rankset, the metric's place in cmfrec_hip_rank_record + 2 */
#define CMFREC_HIP_WATCH_PRECISION 3
#define CMFREC_HIP_WATCH_RECALL 4
#define CMFREC_HIP_WATCH_AP 5
#define CMFREC_HIP_WATCH_NDCG 6
#define CMFREC_HIP_WATCH_RR 7
#define CMFREC_HIP_WATCH_AUC 8
#define CMFREC_HIP_WATCH_MEAN_RANK 9
#define CMFREC_HIP_STEP_IMPROVED 1
#define CMFREC_HIP_STEP_STOP 2
#define CMFREC_HIP_STEP_EVALUATE 4
typedef struct cmfrec_hip_rankset cmfrec_hip_rankset;          /* the ranking set and its record: described below */
typedef struct cmfrec_hip_rank_record {
    double sum[8]; uint64_t count[8]; uint64_t users;
} cmfrec_hip_rank_record;
typedef struct cmfrec_hip_fit_monitor {
    cmfrec_hip_evalset *evalset;
    cmfrec_hip_rankset *rankset;
    int metric, k_at, every, patience, restore_best;
    double min_delta;
    double *values;
    cmfrec_hip_errors *records;
    cmfrec_hip_rank_record *rank_records;
    int *iters_run, *best_iter;
} cmfrec_hip_fit_monitor;
typedef struct cmfrec_hip_early_stop {
    int every, patience, higher_is_better;
    double min_delta;
    double best;
    int best_iter, misses;
} cmfrec_hip_early_stop;
int cmfrec_hip_fit_set_monitor(const cmfrec_hip_fit_monitor *monitor);

/* The ranking metrics of held-out items, reduced on the device (rank_metrics_kernels.hpp).  A ranking set
 * -- nu user ids, their held-out lists (CSR over the nu users) and, optionally, their exclusion lists (CSR over the nu users, each
 * list sorted ascending, as cmfrec_hip_ranker_ranks takes them) -- goes to the device once and stays there.  An evaluation ranks
 * the held-out items (topn_rank_kernel, the ranks cmfrec_hip_ranker_ranks returns, bit for bit) and reduces them where they are:
 * per user exactly the quantities of cmfrec_amd.metrics.ranking_metrics at cut-off k_at -- hit, precision, recall, ap, ndcg, rr,
 * auc, mean_rank, in this order -- and over the users one record: per metric the float64 sum over the users that count and their
 * number (a user without a valid held-out item counts nowhere, a user whose pool holds nothing but its held-out items not in
 * auc), and `users`, the users with a valid held-out item.  A mean is sum / count.  The NDCG discounts and ideal sums come from
 * two tables the host computes in float64 with libm's log2, as NumPy forms them; the sums are added in an order that depends on the
 * device and the launch, not on the run: the same call returns the same bytes (no atomics).
 * The place of a rank among a user's own ranks is counted, not sorted: the work per user grows with the square of its list
 * (fine for the tens to hundreds of held-out items of an evaluation; a list of tens of thousands makes its user the launch's tail).
 * rankset_create: NULL on failure (cmfrec_hip_last_error_code: 2 for lists that are not a CSR or a negative user id, 1 for no room).
 * ranker_metrics: A [m, lda] on the host, the rows of the set's users are taken from it (2 for a user id >= m); per_user [nu, 8]
 *   and out_rank [held_p[nu]] optional outputs.  2 when the set lives on another device than the ranker.
 * CMFREC_HIP_RANKMETRIC_WAVES (read per call): at most that many wavefronts, rounded up to whole workgroups, in the metric launch,
 *   so that a small set gives a wavefront several users in a row (test hook; 0: one wavefront per user up to what the device runs).
 * cmfrec_hip_rank_record (declared above, before the monitor that points to it): double sum[8]; uint64_t count[8]; uint64_t users. */
cmfrec_hip_rankset *cmfrec_hip_rankset_create(const int_t *users, int_t nu, const size_t *held_p, const int_t *held_i,
                                              const size_t *excl_p, const int_t *excl_i, int device);
void cmfrec_hip_rankset_destroy(cmfrec_hip_rankset *set);
int cmfrec_hip_ranker_metrics(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t m, cmfrec_hip_rankset *set, int k_at,
                              cmfrec_hip_rank_record *out, double *per_user, int_t *out_rank);
/* session_ranking: the counterpart of cmfrec_hip_session_errors -- the record of the session's factors as they are on the device
 * (the columns behind k_user / k_item, k + k_main wide; an explicit model's item bias is added to the scores as
 * cmfrec_hip_ranker_create's biasB is).  The rows of the set's users are gathered on the device; a ranker the session owns takes B
 * by a device-to-device column copy into its padded layout on every call, no host round trip.  Waits for the updates queued on
 * the session's stream; changes nothing in the session.  2: a session that does not own all rows, k + k_main > 272, a set on
 * another device, a user id beyond the rows of A. */
int cmfrec_hip_session_ranking(cmfrec_hip_session *s, cmfrec_hip_rankset *set, int k_at, cmfrec_hip_rank_record *out);
int cmfrec_hip_early_stop_step(cmfrec_hip_early_stop *st, int iter, int niter, const double *value);

/* Replace predict_X_old_collective_explicit / _implicit and predict_X_new_collective_explicit / _implicit of the reference's
 * src/cmfrec.h (bodies src/collective.c:11797-12069 over predict_multiple, src/common.c:5066-5110) -- the same positional
 * parameters, the same return codes; nthreads is accepted and ignored.
 * _old: the pairs against factors the caller holds: a scorer (above) created, used once, destroyed; A [m, k_user+k+k_main],
 *   B [n_max (n), k_item+k+k_main]; m = 0 or n = 0 is legal (that side is not read: every pair gets the fallback value), a negative
 *   size, k + k_main < 1 or a missing array returns 2.  _new: the factors of a batch of new rows, then the pairs from them (row indexes the batch's
 *   rows, m = max(m_new, m_u)): cmfrec_hip_newrows_create, one cmfrec_hip_newrows_predict, destroy -- the argument mapping,
 *   refusals and messages of factors_collective_*_multiple; a refused call leaves predicted untouched.
 * Two deliberate differences from the reference: the dot product runs over k + k_main factors, as the
 * model, topN and the imputation define a prediction (the reference's predict_multiple stops after k; equal for k_main = 0); and
 * a negative row / col is treated like one beyond the end (the reference's fallback reads biasA[row] / biasB[col] for it). */
int_t predict_X_old_collective_explicit(
    int_t row[], int_t col[], real_t *predicted, size_t n_predict,
    real_t *A, real_t *biasA,
    real_t *B, real_t *biasB,
    real_t glob_mean,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    int_t m, int_t n_max,
    int nthreads);
int_t predict_X_old_collective_implicit(
    int_t row[], int_t col[], real_t *predicted, size_t n_predict,
    real_t *A,
    real_t *B,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    int_t m, int_t n,
    int nthreads);
int_t predict_X_new_collective_explicit(
    int_t m_new,
    int_t row[], int_t col[], real_t *predicted, size_t n_predict,
    int nthreads,
    bool user_bias,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U, bool NA_as_zero_X,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *Ub, int_t m_ubin, int_t pbin,
    real_t *C, real_t *Cb,
    real_t glob_mean, real_t *biasB,
    real_t *U_colmeans,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *Xfull, int_t n,
    real_t *weight,
    real_t *B,
    real_t *Bi, bool add_implicit_features,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique,
    bool scale_lam, bool scale_lam_sideinfo,
    bool scale_bias_const, real_t scaling_biasA,
    real_t w_main, real_t w_user, real_t w_implicit,
    int_t n_max, bool include_all_X,
    real_t *BtB,
    real_t *TransBtBinvBt,
    real_t *BtXbias,
    real_t *BeTBeChol,
    real_t *BiTBi,
    real_t *TransCtCinvCt,
    real_t *CtCw,
    real_t *CtUbias,
    real_t *B_plus_bias);
int_t predict_X_new_collective_implicit(
    int_t m_new,
    int_t row[], int_t col[], real_t *predicted, size_t n_predict,
    int nthreads,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *B, int_t n,
    real_t *C,
    real_t *U_colmeans,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t l1_lam, real_t alpha, real_t w_main, real_t w_user,
    real_t w_main_multiplier,
    bool apply_log_transf,
    real_t *BeTBe,
    real_t *BtB,
    real_t *BeTBeChol,
    real_t *CtUbias);

/* Replace precompute_collective_explicit / precompute_collective_implicit, /root/reference/src/cmfrec.h:1922-1960 (bodies
 * src/collective.c:10209-10485, :10487-10566): the matrices the prediction functions reuse, from factors the caller holds -- the
 * same positional parameters, the same return codes.  Host buffers in and out; the Gramians run on the library's MFMA kernels,
 * the solves with many right-hand sides (TransBtBinvBt, TransCtCinvCt) on the row Cholesky kernel, BeTBeChol on the small
 * factorisation kernel.  As in the reference the symmetric outputs carry their upper triangle (row-major), the strictly lower
 * part is zero.  extra_precision (the reference's second summation order) is accepted and ignored. */
int_t precompute_collective_explicit(
    real_t *B, int_t n, int_t n_max, bool include_all_X,
    real_t *C, int_t p,
    real_t *Bi, bool add_implicit_features,
    real_t *biasB, real_t glob_mean, bool NA_as_zero_X,
    real_t *U_colmeans, bool NA_as_zero_U,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    bool user_bias,
    bool nonneg,
    real_t lam, real_t *lam_unique,
    bool scale_lam, bool scale_lam_sideinfo,
    bool scale_bias_const, real_t scaling_biasA,
    real_t w_main, real_t w_user, real_t w_implicit,
    real_t *B_plus_bias,
    real_t *BtB,
    real_t *TransBtBinvBt,
    real_t *BtXbias,
    real_t *BeTBeChol,
    real_t *BiTBi,
    real_t *TransCtCinvCt,
    real_t *CtCw,
    real_t *CtUbias);
int_t precompute_collective_implicit(
    real_t *B, int_t n,
    real_t *C, int_t p,
    real_t *U_colmeans, bool NA_as_zero_U,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t w_main, real_t w_user, real_t w_main_multiplier,
    bool nonneg,
    bool extra_precision,
    real_t *BtB,
    real_t *BeTBe,
    real_t *BeTBeChol,
    real_t *CtUbias);

/* Replace topN_old_collective_explicit / topN_old_collective_implicit, /root/reference/src/cmfrec.h:2104-2127 (bodies
 * src/collective.c:11546-11613 over topN, src/common.c:5127-5380): the n_top best items of ONE user whose factors exist, with an
 * include list or an exclude list, scores (+ glob_mean + the user's bias) on request.  Same argument checks and return codes.
 * Scores of the candidates on the device, a stable descending radix sort; ties go to the earlier candidate (the lower item id
 * without an include list) where the reference's qsort leaves their order open.  Many users at once: cmfrec_hip_topN_batch. */
int_t topN_old_collective_explicit(
    real_t *a_vec, real_t a_bias,
    real_t *A, real_t *biasA, int_t row_index,
    real_t *B,
    real_t *biasB,
    real_t glob_mean,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    int_t *include_ix, int_t n_include,
    int_t *exclude_ix, int_t n_exclude,
    int_t *outp_ix, real_t *outp_score,
    int_t n_top, int_t n, int_t n_max, bool include_all_X, int nthreads);
int_t topN_old_collective_implicit(
    real_t *a_vec,
    real_t *A, int_t row_index,
    real_t *B,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    int_t *include_ix, int_t n_include,
    int_t *exclude_ix, int_t n_exclude,
    int_t *outp_ix, real_t *outp_score,
    int_t n_top, int_t n, int nthreads);

/* Runs the on-device self-test of the cross-lane primitives (DPP / permlane swaps) the row kernels
 * are built on; returns the number of mismatching lanes (0 = ok), negative = HIP failure. */
int cmfrec_hip_selftest_lanes(void);
/* timing / agreement probe of the dense contraction C[M, N] = op(A) B (transa: A stored [K, M]) on random operands: ms per call of
   the library's own MFMA kernel and of rocBLAS (loaded at run time if it is there; -1 and a plain reference kernel otherwise),
   largest difference of the two results relative to the largest entry */
int cmfrec_hip_gemm_probe(int M, int N, int K, int transa, int reps, double *ms_own, double *ms_rocblas, double *max_rel_diff);
/* timing probe of the compaction of a dense batch of new rows (dense_rows_device.hpp) on a seeded [rows, n] block with the given
   fraction of present entries: device-event milliseconds per run of the count kernel and of the write kernel over `reps` runs
   after a warm-up run each; nnz: the present entries found */
int cmfrec_hip_dense_rows_probe(int rows, int n, double present, int reps, double *ms_count, double *ms_write, size_t *nnz);
/* The symmetric eigen-decomposition the low-rank row path runs once per half-step on w C^T C (replaces what the reference gets
 * from a k_t x k_t dposv per row, src/collective.c:1823, for rows of few entries): A [n, n] symmetric (2 <= n <= 320) ->
 * Q [n, n] with Q[i][c] = component i of eigenvector c, lam [n] clamped at zero.  method 0: Householder tridiagonalisation +
 * implicit QL (the default of the path), 1: one-workgroup Jacobi (cross-check).  ms: device milliseconds per run over `reps`. */
int cmfrec_hip_sym_eig(int n, const real_t *A, real_t *Q, real_t *lam, int method, int reps, double *ms);
/* One operation of the dense layer on its own, through the launch helpers the library itself uses (test entry point).  Row-major
 * host images with explicit leading dimensions; the operand of an image starts `off` elements into it (the image is that much
 * longer), so that its 16-byte alignment on the device is the caller's choice.  The whole image of C -- those elements and the
 * padding of every row included -- is uploaded before the operation and downloaded after it.
 *   op 0 / 1 : C[m, n] = s1 * A B with A [m, k] / s1 * A^T B with A stored [k, m]; B [k, n]
 *   op 2     : C[k, k] = s1 * B[:n, :k]^T B[:n, :k] + s2 * I                                       (ldc == k, k >= 1)
 *   op 3     : C[n, n] := its upper Cholesky factor in place, the strict lower triangle untouched  (ldc == n, n >= 1)
 *   op 4     : C[n, n] = (R^T)^-1 for the upper factor R = A [n, n]                                (lda == ldc == n, n >= 1)
 *   op 5     : C[m, :k] := C (R^T R)^-1 for the upper factor R = A [k, k]                          (lda == k, ldc >= k)
 * Returns 2 on negative sizes or offsets, a leading dimension below the row length, or a missing operand. */
int cmfrec_hip_dense_op(int op, int m, int n, int k, real_t s1, real_t s2, const real_t *A, size_t lda, int offA,
                        const real_t *B, size_t ldb, int offB, real_t *C, size_t ldc, int offC);

/* The fill kernel of the imputation on its own, through the launch helper cmfrec_hip_newrows_impute uses (test entry point):
 *   X[r, c] = isnan(X[r, c]) ? sum_{f < kk} A[r * lda + f] B[c * ldb + f] + glob_mean + biasA[r] + biasB[c] : X[r, c]
 * in place on the row-major X[m, ldx], kk <= 272.  Host images, each uploaded as it is (m * lda, n * ldb, m * ldx elements from
 * the pointer, the padding of every row included); X is downloaded whole.  A and B point at the first used column.  biasA
 * (optional): m values -- or, where it points into the image of A, that column of the image (stride lda: the layout of the
 * new-rows handle, whose factor rows end in their bias).  biasB (optional): n values.  row_missing (optional): one count per
 * row; a row whose count is 0 is neither read nor written.  Returns 2 on negative sizes, kk > 272, a leading dimension below the
 * row length or a missing operand. */
int cmfrec_hip_impute_dense(int m, int n, int kk, const real_t *A, size_t lda, const real_t *biasA, const real_t *B, size_t ldb,
                            const real_t *biasB, real_t glob_mean, real_t *X, size_t ldx, const int *row_missing);

/* The scoring kernel of the chosen pairs on its own, through the launch helper every prediction path uses (test entry point):
 * the rule of cmfrec_hip_scorer_predict on host images that are uploaded as they are.  A is the image of the row factors,
 * offA + m * lda elements whose operand [m, lda] starts offA elements in (so that its 16-byte alignment on the device is the
 * caller's choice: aligned operands with even pitches are fetched 16 bytes per lane, the others element by element, with the same
 * bits); B likewise.  biasA (optional): m values -- or, where it points into the image of A, that column of the image (stride
 * lda).  biasB (optional): n values.  Returns 2 on negative sizes or offsets, kk < 1, a leading dimension below kk or a missing
 * operand. */
int cmfrec_hip_score_pairs(int m, int n, int kk, const real_t *A, size_t lda, int offA, const real_t *biasA, const real_t *B, size_t ldb,
                           int offB, const real_t *biasB, real_t glob_mean, int implicit, const int_t *row, const int_t *col, size_t n_pairs,
                           real_t *out);

/* The two kernels of the error reduction on their own (test entry point), beside cmfrec_hip_score_pairs and with its arguments
 * and return codes: the same host images, uploaded as they are, then x [n_pairs], weight [n_pairs] or NULL (2 for a NaN, infinite
 * or negative one), pred [n_pairs] or NULL -- the prediction of every pair as the kernel formed it, skipped pairs included -- and
 * out, the record (all zeros for n_pairs = 0). */
int cmfrec_hip_pair_errors(int m, int n, int kk, const real_t *A, size_t lda, int offA, const real_t *biasA, const real_t *B, size_t ldb,
                           int offB, const real_t *biasB, real_t glob_mean, int implicit, const int_t *row, const int_t *col, size_t n_pairs,
                           const real_t *x, const real_t *weight, real_t *pred, cmfrec_hip_errors *out);

/* Start values as the reference's random_parallel draws them (src/helpers.c:927-1043; xoshiro256++
 * seeded by splitmix64, truncated ziggurat normals or uniforms, scaled 2^-7): A <- stream(seed),
 * B <- the stream jumped once.  Host-only.  Returns 1 if the ziggurat tables are NumPy's exact
 * constants, 0 if they were recomputed (<= 1 ulp apart). */
int cmfrec_hip_random_parallel(real_t *A, size_t sizeA, real_t *B, size_t sizeB, int_t seed, bool normal);

/* The point-to-point schedule MultiDev::exchange issues for one half-step (direct placement): the operations of all
 * D devices for the block boundaries bb[0 .. D], five ints each -- {device, peer, send (1) / receive (0), first row, rows} -- in
 * issue order, at most `cap` of them written to `out`.  Host-only, no device needed: lets a test check that every send has its
 * matching receive with the same count and that the received blocks tile the replica.  Returns the number of operations. */
int cmfrec_hip_exchange_plan(int D, const int *bb, int *out, int cap);

/* Build info: sizeof(real_t), and the gfx target the kernels were compiled for. */
int cmfrec_hip_sizeof_real(void);
/* sizeof(cmfrec_hip_model) as compiled: lets a binding verify its mirror of the struct before the first call. */
int cmfrec_hip_sizeof_model(void);
const char *cmfrec_hip_build_info(void);
/* The CMFREC_HIP_* environment switches are read when a session is created; this reads them again for the
 * sessions that already exist (bench.py's pass with the nnz bins in line). */
void cmfrec_hip_reload_switches(void);

#ifdef __cplusplus
}
#endif
#endif
