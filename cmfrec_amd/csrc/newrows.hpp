// newrows.hpp -- what the units behind the new-rows handle share (cmfrec_hip_newrows_*, include/cmfrec_hip.h): the
// device-resident model of a batch of new rows and its batch run (session.hip), the ranking of device factors against device
// items (topn_tu.hip), the C entry points and the rescaling rules of the two drop-in functions (fit.hip).  No kernels.
#pragma once
#include "device_base.hpp"

struct cmfrec_hip_ranker;

namespace cmfhip {

// The model side of cmfrec_hip_factors_multiple_ex's arguments (the rescaling of the drop-in functions applied): what does not
// change from batch to batch.
struct NewRowsModelArgs {
    const real_t *B = nullptr;                 // [n, k_item + k + k_main]
    int_t n = 0;
    const real_t *C = nullptr;                 // [p, k_user + k], null: no side information in any batch
    int_t p = 0;
    const real_t *U_colmeans = nullptr;
    const real_t *biasB = nullptr;
    int_t k = 0, k_user = 0, k_item = 0, k_main = 0;
    bool user_bias = false;                    // a bias unknown in every row system (the one-shot calls: biasA given)
    real_t lam = 0, lam_bias = 0, lam_x = 0, w_user = 1;
    bool implicit = false, scale_lam = false, scale_lam_sideinfo = false, scale_bias_const = false;
    const real_t *BtB_pre = nullptr, *TransCtCinvCt_pre = nullptr;
    bool nonneg = false;
    real_t l1_lam = 0, l1_lam_bias = 0;
    const real_t *Bi = nullptr;                // [n_Bi, k + k_main]
    int_t n_Bi = 0;
    real_t w_implicit = 1, w_implicit_gram = 1;
    const real_t *BiTBi_pre = nullptr;
    const real_t *TransBtBinvBt_pre = nullptr; // [n_TB, k + k_main (+ 1)]
    int_t n_TB = 0;
    // missing-as-zero models: an absent entry of a sparse X / of a sparse U is a zero.  glob_mean and
    // n_x (the items that carry a bias: the rest of B's rows count with the mean only) enter the constant of the right-hand sides.
    bool NA_as_zero_X = false, NA_as_zero_U = false;
    real_t glob_mean = 0;
    int_t n_x = 0;
};

// The batch side: everything that depends on X, U, the weights or Xfull.
struct NewRowsBatchArgs {
    int_t m_x = 0, m_u = 0;
    int_t n = 0;                               // items of this batch: bound of X's indices, columns of Xfull (<= the model's n)
    const real_t *U = nullptr;                 // [m_u, p]
    const int_t *U_row = nullptr, *U_col = nullptr; const real_t *U_sp = nullptr; size_t nnz_U = 0;
    const size_t *U_csr_p = nullptr; const int_t *U_csr_i = nullptr; const real_t *U_csr = nullptr;
    const int_t *ixA = nullptr, *ixB = nullptr; const real_t *X = nullptr; size_t nnz = 0;
    const size_t *Xcsr_p = nullptr; const int_t *Xcsr_i = nullptr; const real_t *Xcsr = nullptr;
    const real_t *weight = nullptr, *Xfull = nullptr, *weight_full = nullptr;
    real_t glob_mean_full = 0;
    bool allow_TransCtCinvCt = true;           // the drop-in functions do not hand that matrix on with a dense X
};

struct NewRowsState;

// session.hip.  create / run report through g_last_error and the ABI's return codes; both throw HipError on a HIP failure
// (call them inside guarded()).  run leaves the factors on the device ([rows, ldA], the bias in the last column) and downloads
// them where A / biasA are given.
NewRowsState *newrows_state_create(const NewRowsModelArgs &M, int device, int *rc);
void newrows_state_destroy(NewRowsState *s);
int newrows_state_run(NewRowsState *s, const NewRowsBatchArgs &bt, real_t *A, real_t *biasA);
struct NewRowsView {
    int device = 0;
    const real_t *dA = nullptr; size_t ldA = 0; int rows = 0;     // factors of the last batch
    const real_t *dB = nullptr; size_t ldB = 0; int n = 0;        // the resident items (all columns), their bias or null
    const real_t *dbiasB = nullptr;
};
NewRowsView newrows_state_view(const NewRowsState *s);
// Exclusion lists of the last batch's rows for the ranking kernels, on the device: the items of each row's own X (seen), the
// caller's lists (host CSR over the rows, each sorted), or their union; every list sorted ascending.  Both null: *dp = null.
int newrows_state_exclusions(NewRowsState *s, bool seen, const size_t *excl_p, const int_t *excl_i, const size_t **dp, const int **di);
int newrows_state_solve_ms(NewRowsState *s, double *ms);
// Imputation of a dense batch (bt.Xfull [m_x, n] with NaN): Xout [m_x, n] = Xfull with every NaN replaced by the prediction from
// the batch's factors; Xout may be bt.Xfull.  A batch without any NaN is copied without solving (*solved = false).  fill_ms: the
// HIP-event time of the fill kernel over the blocks of the last impute call.
int newrows_state_impute(NewRowsState *s, const NewRowsBatchArgs &bt, real_t *Xout, real_t *A, real_t *biasA, bool *solved);
double newrows_state_fill_ms(const NewRowsState *s);
// the wavefronts of the last launch of the missing-as-zero right-hand-side kernel (0: none yet; what CMFREC_HIP_NAZ_WAVES caps)
int newrows_state_naz_waves(const NewRowsState *s);

// newrows_naz_tu.hip: the kernels of newrows_naz_kernels.hpp behind plain functions (the one unit that instantiates them)
template <typename T> struct NazRhsParams;
int naz_launch_rhs(hipStream_t st, int num_cus, const NazRhsParams<real_t> &P, int max_waves);     // the wavefronts of the task launch
void naz_launch_pad_rows(hipStream_t st, const real_t *src, size_t lds, int off, int cols, real_t scale, int ones_col, real_t *dst, size_t ldd,
                         size_t rows);
void naz_launch_weight_corrections(hipStream_t st, const real_t *w, size_t nnz, real_t *g, real_t *z);

// topn_tu.hip: a ranker over items that are on the device already (packed copy, ldb = topnw_kp(k)), and a ranking call on
// device factors with device exclusion lists -- cmfrec_hip_ranker_topN without its uploads.  The caller has synchronised the
// stream that wrote dA / the lists.
cmfrec_hip_ranker *ranker_create_from_device(const real_t *dB, size_t ldb, int_t n, int_t k, const real_t *dbiasB, int device);
int ranker_topN_device(cmfrec_hip_ranker *r, const char *fn, const real_t *dA, size_t lda, int_t nu, const size_t *dexcl_p,
                       const int *dexcl_i, int_t n_top, int_t *out_ids, real_t *out_scores);
// the same over each row's candidate list (host CSR over the nu rows, uploaded here; topn_cand_kernels.hpp)
int ranker_topN_candidates_device(cmfrec_hip_ranker *r, const char *fn, const real_t *dA, size_t lda, int_t nu, const size_t cand_p[],
                                  const int_t cand_i[], const size_t *dexcl_p, const int *dexcl_i, int_t n_top, int_t *out_ids,
                                  real_t *out_scores);
// the ranks of each row's held-out items (host CSR over the nu rows, uploaded here; topn_rank_kernels.hpp); out_rank / out_scores
// [held_p[nu]], out_pool [nu], the last two optional
int ranker_ranks_device(cmfrec_hip_ranker *r, const char *fn, const real_t *dA, size_t lda, int_t nu, const size_t held_p[],
                        const int_t held_i[], const size_t *dexcl_p, const int *dexcl_i, int_t *out_rank, real_t *out_scores,
                        int_t *out_pool);
int ranker_check_limits(const char *fn, int_t k, int_t n_top, int_t n);
// topn_tu.hip: the ranking metrics of a resident set (cmfrec_hip_rankset_*, rank_metrics_kernels.hpp) against factors that are on
// the device, through a ranker the caller owns (*owned: null before the first call; cmfrec_hip_ranker_destroy it), and what a fit
// asks of the set it is to watch.  Both report through g_last_error and throw HipError (call inside guarded()).
int rankset_run_on_factors(cmfrec_hip_ranker **owned, cmfrec_hip_rankset *set, const char *fn, int device, const real_t *dA, size_t ldA, int_t m,
                           const real_t *dB, size_t ldB, int_t n, int_t kk, const real_t *dbiasB, int k_at, cmfrec_hip_rank_record *out);
int rankset_usable(cmfrec_hip_rankset *set, const char *fn, int device, int_t m, int_t n, int_t kk, int k_at);

// predict_tu.hip: the scoring of chosen (row, col) pairs against operands that are on the device already -- the stream, the
// pair buffers and the timing of cmfrec_hip_scorer_predict without its factor uploads.  dA [m, lda] / dB [n, ldb] point at the
// first scored column; dbiasA: m values with stride ldbiasA, or null.  Throws HipError (call inside guarded()); the caller has
// synchronised the stream that wrote the operands.
struct PairScorer;
PairScorer *pair_scorer_create(int device);
void pair_scorer_destroy(PairScorer *ps);
int pair_scorer_run(PairScorer *ps, const real_t *dA, size_t lda, int_t m, const real_t *dbiasA, size_t ldbiasA, const real_t *dB, size_t ldb,
                    int_t n, int_t kk, const real_t *dbiasB, real_t glob_mean, bool implicit, const int_t *row, const int_t *col,
                    size_t n_pairs, real_t *out);
double pair_scorer_ms(const PairScorer *ps);               // the kernel over the blocks of the last run

// predict_tu.hip: the error record of a resident evaluation set (cmfrec_hip_evalset_*) against operands that are on the device
// already, with pair_scorer_run's operand arguments: the two kernels on stream st behind what is queued there, one
// synchronisation, the record in *out.  device / num_cus: the operands' device (the set must live there, otherwise 2 with fn's
// name in the message).  dpred: the predictions too ([n_pairs] on the device), or null.  Throws HipError.
int evalset_run(cmfrec_hip_evalset *e, const char *fn, int device, int num_cus, hipStream_t st, const real_t *dA, size_t lda, int_t m,
                const real_t *dbiasA, size_t ldbiasA, const real_t *dB, size_t ldb, int_t n, int_t kk, const real_t *dbiasB, real_t glob_mean,
                bool implicit, real_t *dpred, cmfrec_hip_errors *out);
// what a fit asks of the set it is to watch (cmfrec_hip_fit_set_monitor), before it writes anything: the set lives on `device`
// (< 0: the current one) and at least one pair lies inside [0, m) x [0, n) with a value that is not NaN -- one download of the
// set's three arrays.  0, or 2 with fn's name in the message.  Throws HipError.
int evalset_usable(cmfrec_hip_evalset *e, const char *fn, int device, int_t m, int_t n);

}  // namespace cmfhip
