// fit_inputs.hpp -- what the two fit drivers (fit.hip) make of the caller's arrays before a session exists: the forms side
// information is taken in (SideInput over ZeroFilledSide / SparseZerosSide / DenseNanSide), the dense X as COO (DenseX), the
// global mean.  Host only: nothing of HIP is included, so the same code compiles into a stand-alone program under
// AddressSanitizer / UBSan (tests/c_caller/fit_inputs_san.cpp) -- it indexes arrays with indices the caller supplied.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/cmfrec_hip.h"

namespace cmfit {

#ifdef CMFREC_HIP_FLOAT
const real_t EPS_T = FLT_EPSILON;
#else
const real_t EPS_T = DBL_EPSILON;
#endif

// Dense side information with missing values (NaN).  The reference centres the present entries of each column
// (center_by_cols, common.c:4938-4997) and then uses, for every row / column, only what is present -- the same
// arithmetic as its sparse-side-information route run on the centred values (collective.c:1566-1653: the C^T C block
// and the right-hand side over the present attributes, lambda scaled by their count; optimizeA Case 2 for C / D).  So
// such a matrix is handed to the sparse route as COO triplets of its centred present entries.
struct DenseNanSide {
    std::vector<int_t> row, col;
    std::vector<real_t> val;
    std::vector<int_t> na_col;                  // missing values per attribute
    int_t n_rows = 0;
    // What the reference's dense C / D update (optimizeA Cases 1-2 on the transposed matrix, common.c:2793-3116) does differently
    // from the sparse one, per attribute.  An attribute that misses fewer than 2 kc values is solved from the precomputed Gramian
    // minus the missing rows (factors_closed_form :759-790, ahead of the CG branch at :884): in closed form whatever use_cg says
    // (mask 1), under scale_lam with the n_rows x lam of a complete attribute (:3031-3032 / :2832).  When at least 75 % of the
    // attributes are complete (helpers.c:151-250) those share one factorisation (mask 1) and the ones that miss 2 kc values or
    // more are redone by CG from zero with kc steps (mask 2; Case 1's fix-up loop, :2953-2985).  Mask 0: the solver asked for.
    void rules(int_t kc, bool scale_lam, std::vector<unsigned char> &mask, std::vector<real_t> &mult) const
    {
        const int_t p = (int_t)na_col.size();
        int_t with_na = 0;
        bool any_few = false;
        for (int_t c = 0; c < p; c++) { with_na += (na_col[c] > 0); any_few = any_few || (na_col[c] > 0 && na_col[c] < 2 * kc); }
        const bool near = (p - with_na) >= (int_t)((real_t)0.75 * (real_t)p);
        mask.resize((size_t)p);
        for (int_t c = 0; c < p; c++) mask[c] = (na_col[c] < 2 * kc) ? 1 : (near ? 2 : 0);
        mult.clear();
        if (scale_lam && any_few) {
            mult.resize((size_t)p);
            for (int_t c = 0; c < p; c++)
                mult[c] = (na_col[c] < 2 * kc) ? (real_t)n_rows : (na_col[c] < n_rows ? (real_t)(n_rows - na_col[c]) : (real_t)1);
        }
    }
    bool convert(const real_t *M, int_t rows, int_t cols, real_t *means)
    {
        bool any = false;
        for (size_t e = 0; e < (size_t)rows * cols && !any; e++) any = std::isnan(M[e]);
        if (!any) return false;
        std::vector<double> sum((size_t)cols, 0.0);
        std::vector<size_t> cnt((size_t)cols, 0);
        for (int_t r = 0; r < rows; r++)
            for (int_t c = 0; c < cols; c++) {
                const real_t v = M[(size_t)r * cols + c];
                if (!std::isnan(v)) { sum[c] += v; cnt[c]++; }
            }
        for (int_t c = 0; means && c < cols; c++) means[c] = (real_t)(sum[c] / (double)cnt[c]);
        n_rows = rows; na_col.resize((size_t)cols);
        for (int_t c = 0; c < cols; c++) na_col[c] = rows - (int_t)cnt[c];
        for (int_t r = 0; r < rows; r++)
            for (int_t c = 0; c < cols; c++) {
                const real_t v = M[(size_t)r * cols + c];
                if (std::isnan(v)) continue;
                row.push_back(r); col.push_back(c); val.push_back(means ? v - means[c] : v);
            }
        return true;
    }
};

// NA_as_zero_U / NA_as_zero_I: a sparse side-information matrix whose absent entries are ZEROS is the dense matrix holding those
// zeros, on every row of X (rows of X beyond the last row of the triplets are zero rows: the column means divide by all of
// them).  The reference reaches the same numbers by other operations -- optimizeA Case 3 for C / D with the column means as a
// rank-one correction (collective.c:8354-8386, common.c:3116-3205), the full w C^T C block plus a constant -w C^T colmeans on
// every right-hand side (collective.c:1277-1457, :5790-5800, :5823-5836; block CG: :2292-2298) -- and agrees with the dense
// route on the zero-filled matrix to 1e-15, closed form and CG, both models (tests/test_oracle_vs_ref.py).  So that is what the
// fit runs, in one of two forms.  Up to CMFREC_HIP_ZEROFILL_MAX_GB the triplets are scattered into a [rows of X, cols] matrix here
// and take the dense path, GEMMs and all; cost: rows x cols numbers of host and device memory instead of the triplets.  Beyond it
// (single device) the triplets themselves go to the session (SparseZerosSide below, cmfrec_hip_session_set_sideinfo_sparse_zeros):
// the same dense path with its two products by that matrix taken as sparse products plus the column means' rank-one term.  More
// rows of side information than X has: refused (the reference treats the rows beyond X differently from its dense branch,
// nothing pins them).
struct ZeroFilledSide {
    std::vector<real_t> dense;
    // Size limit of the zero-filled matrix: it exists three times (here, as the centred copy, on the device).  Beyond
    // CMFREC_HIP_ZEROFILL_MAX_GB (default 8 GB per copy; realistic sparse side information of 1e6..1e7 rows x 1e3..1e4 columns
    // is 8e9..8e11 bytes) build() returns 3 and the fit takes the sparse form; a multi-device fit, whose row-block shards need
    // the dense matrix, answers with a controlled "not implemented at this size" instead of a bad_alloc / hipErrorOutOfMemory
    // late in the fit.  Read per fit: a tiny value sends any problem down the sparse form (tests, tools/bench_side_zeros.py).
    static double max_bytes()
    {
        const char *e = getenv("CMFREC_HIP_ZEROFILL_MAX_GB");
        const double gb = (e != nullptr && atof(e) > 0) ? atof(e) : 8.0;
        return gb * 1e9;
    }
    // 0 ok, 1 triplets missing / out of range, 2 more rows than X, 3 larger than the limit above.  Triplets that repeat a
    // position are SUMMED (the reference's COO -> CSR keeps both and its sums add both: the same numbers).
    int build(int_t rows_x, int_t rows_side, int_t cols, const int_t *r, const int_t *c, const real_t *v, size_t nnz)
    {
        if (rows_side > rows_x) return 2;
        if (!r || !c || !v || cols <= 0) return 1;
        if ((double)rows_x * (double)cols * (double)sizeof(real_t) > max_bytes()) return 3;
        dense.assign((size_t)rows_x * (size_t)cols, (real_t)0);
        for (size_t e = 0; e < nnz; e++) {
            if (r[e] < 0 || r[e] >= rows_side || c[e] < 0 || c[e] >= cols) return 1;
            dense[(size_t)r[e] * (size_t)cols + (size_t)c[e]] += v[e];
        }
        return 0;
    }
};
// ... the sparse form: the triplets as they came (validated; positions given twice add up in the products as they do in the
// scatter above) and the column means over ALL rows of X, summed in double -- what center_cols computes of the zero-filled matrix.
struct SparseZerosSide {
    bool on = false;
    const int_t *row = nullptr, *col = nullptr;
    const real_t *val = nullptr;
    size_t nnz = 0;
    std::vector<real_t> means;           // empty: the caller asked for no centring (no colmeans output)
    // 0 ok, 1 triplets missing / out of range, 4 NaN among the values
    int take(int_t rows_x, int_t rows_side, int_t cols, const int_t *r, const int_t *c, const real_t *v, size_t n, real_t *means_out)
    {
        if (!r || !c || !v || cols <= 0) return 1;
        std::vector<double> sum((size_t)cols, 0.0);
        for (size_t e = 0; e < n; e++) {
            if (r[e] < 0 || r[e] >= rows_side || c[e] < 0 || c[e] >= cols) return 1;
            if (std::isnan(v[e])) return 4;
            sum[(size_t)c[e]] += (double)v[e];
        }
        if (means_out != nullptr) {
            means.resize((size_t)cols);
            for (int_t j = 0; j < cols; j++) means_out[j] = means[(size_t)j] = (real_t)(sum[(size_t)j] / (double)rows_x);
        }
        row = r; col = c; val = v; nnz = n; on = true;
        return 0;
    }
    const real_t *colmeans() const { return means.empty() ? nullptr : means.data(); }
};
// ... with one exception the reference makes: a row with neither an entry of X nor an entry of the side information is not solved
// but set to zero, bias included (collective_closed_form_block, collective.c:1262-1271; _implicit: :1876-1884).  The list of
// those rows, for cmfrec_hip_session_set_zero_rows.
inline std::vector<int_t> rows_without_data(int_t rows, const int_t *ix_x, size_t nnz, const int_t *ix_side, size_t nnz_side)
{
    std::vector<char> has((size_t)rows, 0);
    for (size_t e = 0; e < nnz; e++) if (ix_x[e] >= 0 && ix_x[e] < rows) has[(size_t)ix_x[e]] = 1;
    for (size_t e = 0; ix_side != nullptr && e < nnz_side; e++) if (ix_side[e] >= 0 && ix_side[e] < rows) has[(size_t)ix_side[e]] = 1;
    std::vector<int_t> out;
    for (int_t r = 0; r < rows; r++) if (!has[(size_t)r]) out.push_back(r);
    return out;
}
// precomputedCtUbias of the reference's epilogue (collective.c:9244-9252, :10115-10123): -w C^T colmeans
inline void fill_CtUbias(real_t *out, const real_t *C, const real_t *colmeans, int_t p, int_t kc, real_t w)
{
    if (!out || !C || !colmeans) return;
    for (int_t f = 0; f < kc; f++) {
        double acc = 0;
        for (int_t j = 0; j < p; j++) acc += (double)C[(size_t)j * kc + f] * (double)colmeans[j];
        out[f] = (real_t)(-(double)w * acc);
    }
}

// column means of sparse side information are reported like the reference does (common.c:4976-4990); the fit itself runs on
// the values as given (the centred copy center_by_cols makes is not the one coo_to_csr_and_csc reads, collective.c:6541-6558)
inline void sparse_colmeans(const int_t *col, const real_t *val, size_t nnz, int_t cols, real_t *means)
{
    if (!means) return;
    std::vector<double> sum((size_t)cols, 0.0);
    std::vector<size_t> cnt((size_t)cols, 0);
    for (size_t e = 0; e < nnz; e++) { sum[col[e]] += val[e]; cnt[col[e]]++; }
    for (int_t c = 0; c < cols; c++) means[c] = (real_t)(sum[c] / (double)cnt[c]);
}

// Dense X (Xfull [m, n] row-major, NaN = missing; weight, if given, dense too) -> the COO of its present entries in row-major
// order, which is the order every running mean of the reference's dense branches takes them in (common.c:3463-3490,
// :4152-4180), plus what optimizeA's case selection needs (helpers.c:151-250): a half-step is "full" when no row (column) has
// a missing entry and "near dense" when at least 75 % of them have none.
struct DenseX {
    std::vector<int_t> row, col;
    std::vector<real_t> val, w;
    bool full = false, near_row = false, near_col = false;
    std::vector<int_t> na_row, na_col;          // missing entries per row / column
    void convert(const real_t *Xfull, const real_t *weight, int_t m, int_t n)
    {
        na_row.assign((size_t)m, 0); na_col.assign((size_t)n, 0);
        size_t present = 0;
        for (int_t r = 0; r < m; r++)
            for (int_t c = 0; c < n; c++) {
                const bool na = std::isnan(Xfull[(size_t)r * n + c]);
                na_row[r] += na; na_col[c] += na; present += !na;
            }
        row.reserve(present); col.reserve(present); val.reserve(present);
        if (weight) w.reserve(present);
        for (int_t r = 0; r < m; r++)
            for (int_t c = 0; c < n; c++) {
                const real_t x = Xfull[(size_t)r * n + c];
                if (std::isnan(x)) continue;
                row.push_back(r); col.push_back(c); val.push_back(x);
                if (weight) w.push_back(weight[(size_t)r * n + c]);
            }
        full = (present == (size_t)m * (size_t)n);
        if (!full) {
            int_t with_na = 0;
            for (int_t r = 0; r < m; r++) with_na += (na_row[r] > 0);
            near_row = (m - with_na) >= (int)(0.75 * (double)m);
            with_na = 0;
            for (int_t c = 0; c < n; c++) with_na += (na_col[c] > 0);
            near_col = (n - with_na) >= (int_t)((real_t)0.75 * (real_t)n);
        }
    }
};

// ---- side information: column means + centering, common.c:4938-4997 (only when the means are asked for) ----
inline void center_cols(const real_t *M, int rows, int cols, real_t *means, std::vector<real_t> &out)
{
    out.assign(M, M + (size_t)rows * cols);
    if (means == nullptr) return;                                     // no centring asked for (common.c:4938)
    for (int c = 0; c < cols; c++) means[c] = 0;
    for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) means[c] += M[(size_t)r * cols + c];
    for (int c = 0; c < cols; c++) means[c] /= (double)rows;
    for (int r = 0; r < rows; r++) for (int c = 0; c < cols; c++) out[(size_t)r * cols + c] -= means[c];
}

// One side of side information -- U on the rows of X or I on its columns -- as the two fit drivers see it: what the caller
// passed, rewritten in place by the two stages of the intake, and the converters' storage the rewritten pointers point into.  The
// drivers' own checks sit between and after the stages and read these fields; a refusal comes back as its message (empty: go on).
struct SideInput {
    const real_t *dense;                 // [rows, cols] row-major, or NULL
    int_t rows, cols;
    const int_t *row, *col;              // COO triplets (absent = missing, or = zero under naz)
    const real_t *val;
    size_t nnz;
    real_t *colmeans;                    // output; NULL: no centring asked for
    const char *name;                    // "U" / "I": the words that differ in the messages
    const char *more_rows_than;          // "X" / "X has columns"
    const char *shape_words;             // "rows of X x p" / "columns of X x q"
    ZeroFilledSide zf;
    SparseZerosSide sz;
    DenseNanSide nan;
    std::vector<int_t> zero_rows;        // rows of X with neither an entry nor side information (naz only)
    std::vector<real_t> centred;         // the dense matrix minus its column means (center())
    bool naz = false;                    // NA_as_zero_U / _I applied: sparse triplets whose absent entries are zeros
    bool had_dense = false;              // before the NaN stage: dense or sparse-zeros (the prediction matrices of a dense side)
    bool nan_side = false;               // dense with NaN, now the triplets of its centred present entries

    bool sparse() const { return dense == nullptr && nnz > 0; }
    bool present() const { return dense != nullptr || nnz > 0 || sz.on; }
    bool beyond(int_t rows_x) const { return (dense != nullptr || nnz > 0) && rows > rows_x; }
    std::string index_message() const { return std::string("cmfrec_hip: ") + name + " index out of range."; }

    // Stage 1, NA_as_zero_U / _I: sparse side information whose absent entries are zeros -> the dense route on the zero-filled
    // matrix (ZeroFilledSide), or, past its size limit on a single device, the same route on the triplets (SparseZerosSide).
    // rows_x: rows of X on this side; ix_x / nnz_x: its entries' indices on this side.
    std::string zero_fill(bool flag, int_t rows_x, const int_t *ix_x, size_t nnz_x, bool sparse_zeros_ok)
    {
        naz = flag && dense == nullptr && nnz > 0;
        if (!naz) return "";
        const std::string N(name);
        zero_rows = rows_without_data(rows_x, ix_x, nnz_x, row, nnz);
        int e = zf.build(rows_x, rows, cols, row, col, val, nnz);
        if (e == 3 && sparse_zeros_ok && (e = sz.take(rows_x, rows, cols, row, col, val, nnz, colmeans)) == 4)
            return "cmfrec_hip: NA_as_zero_" + N + " beyond CMFREC_HIP_ZEROFILL_MAX_GB: NaN among the values of " + N + " is not implemented.";
        if (e == 2) return "cmfrec_hip: NA_as_zero_" + N + " with more rows of " + N + " than " + more_rows_than + " is not implemented.";
        if (e == 3)
            return "cmfrec_hip: NA_as_zero_" + N + " on several devices runs on the zero-filled dense matrix (" + shape_words + "), which is larger than "
                   "CMFREC_HIP_ZEROFILL_MAX_GB (default 8) here: not implemented at this size.";
        if (e) return index_message();
        if (!sz.on) dense = zf.dense.data();
        rows = rows_x; nnz = 0; row = col = nullptr; val = nullptr;
        return "";
    }
    // Stage 2: dense side information with NaN -> the sparse route on its centred present entries; else the column means of
    // sparse triplets (whose columns are in range: the drivers refuse the others afterwards).
    void take_nan()
    {
        had_dense = (dense != nullptr) || sz.on;
        if (dense && rows > 0 && cols > 0 && nan.convert(dense, rows, cols, colmeans)) {
            dense = nullptr; row = nan.row.data(); col = nan.col.data(); val = nan.val.data(); nnz = nan.val.size(); nan_side = true;
        } else if (dense == nullptr && nnz > 0 && row && col && val) {
            bool ok = true;
            for (size_t e = 0; e < nnz && ok; e++) ok = (col[e] >= 0 && col[e] < cols);
            if (ok) sparse_colmeans(col, val, nnz, cols, colmeans);
        }
    }
    // after the NaN stage nothing is left of this side.  `any_nan_side`: NaN on EITHER side -- so a U that runs on the triplets
    // beyond the zero-fill limit (no dense pointer, no count left) is "empty" too once I has NaN; kept as it is.
    bool nothing_present(bool any_nan_side) const { return any_nan_side && nnz == 0 && nan.row.empty() && had_dense && dense == nullptr; }
    // sparse: COO triplets with rows inside X.  The drivers test both sides in one condition, ahead of either side's indices.
    bool bad_triplets(int_t rows_x) const { return sparse() && (rows > rows_x || !row || !col || !val); }
    bool index_out_of_range() const
    {
        for (size_t e = 0; sparse() && e < nnz; e++)
            if (row[e] < 0 || row[e] >= rows || col[e] < 0 || col[e] >= cols) return true;
        return false;
    }
    void drop_if_absent() { if (!present()) { rows = 0; cols = 0; } }
    void center() { if (dense) center_cols(dense, rows, cols, colmeans, centred); }
    const real_t *centred_or_null() const { return dense ? centred.data() : nullptr; }
};
inline SideInput user_side(const real_t *U, int_t m_u, int_t p, const int_t *r, const int_t *c, const real_t *v, size_t nnz, real_t *colmeans)
{
    return SideInput{U, m_u, p, r, c, v, nnz, colmeans, "U", "X", "rows of X x p"};
}
inline SideInput item_side(const real_t *II, int_t n_i, int_t q, const int_t *r, const int_t *c, const real_t *v, size_t nnz, real_t *colmeans)
{
    return SideInput{II, n_i, q, r, c, v, nnz, colmeans, "I", "X has columns", "columns of X x q"};
}

// ---- global mean, common.c:3494-3524 + :3603 (nthreads selects running mean vs sum / count) ----
// the entries unweighted, in the order given
inline real_t mean_of_entries(const real_t *X, size_t nnz, int nthreads)
{
    double xsum = 0;
    if (nthreads >= 8) {
        for (size_t e = 0; e < nnz; e++) xsum += X[e];
        return (real_t)(xsum / (double)nnz);
    }
    size_t cnt = 0;
    for (size_t e = 0; e < nnz; e++) xsum += (X[e] - xsum) / (double)(++cnt);
    return (real_t)xsum;
}
// weighted running mean, common.c:3574-3584.  With 8 threads or more the reference divides the UNWEIGHTED sum of X by
// the sum of the weights (:3561-3571) -- not a mean, but the number a caller with nthreads >= 8 receives (Python:
// nthreads = -1 on a host of 8 cores or more), so it is reproduced (fixture g23).
// (one of the two places this stood took the quotient through real_t, double and real_t again where the other took it to real_t
//  at once: checked, real_t -> double -> real_t returns the same real_t, so the two were one function)
inline real_t weighted_mean_of_entries(const real_t *X, const real_t *weight, size_t nnz, int nthreads)
{
    double xsum = 0, wsum = 2.220446049250313e-16;
    if (nthreads >= 8) {
        wsum = 0;
        for (size_t e = 0; e < nnz; e++) { xsum += (double)X[e]; wsum += (double)weight[e]; }
        return (real_t)(xsum / wsum);
    }
    for (size_t e = 0; e < nnz; e++) { wsum += (double)weight[e]; xsum += (((double)X[e] - xsum) * (double)weight[e]) / wsum; }
    return (real_t)xsum;
}
// the mean of the entries finished per case.  NA_as_zero_X: the mean over all m x n cells -- the mean of the entries x nnz / (m n)
// (common.c:3494-3523), with weights DIVIDED by the weights' share of all cells, wsum / (wsum + m n - nnz), as the reference does
// (:3590-3594; the sum of the weights there is a compensated sum, helpers.c:1691-1707); the stored values stay as they are
// (:3600-3607), the mean enters every right-hand side instead (collective.c:8573-8600, :8756-8787).  Otherwise: not below zero for
// the non-negative model (:3604-3605).  A mean below sqrt(eps) counts as zero.
inline real_t global_mean(const real_t *X, const real_t *weight, size_t nnz, int_t m, int_t n, int nthreads, bool NA_as_zero_X, bool nonneg)
{
    real_t gm = weight ? weighted_mean_of_entries(X, weight, nnz, nthreads) : mean_of_entries(X, nnz, nthreads);
    if (NA_as_zero_X && weight) {
        double err = 0, res = 0;
        for (size_t e = 0; e < nnz; e++) { const double diff = (double)weight[e] - err; const double temp = res + diff; err = (temp - res) - diff; res = temp; }
        const long double wl = (long double)res;
        gm = (real_t)((long double)gm / (wl / (wl + ((long double)m * (long double)n - (long double)nnz))));
    } else if (NA_as_zero_X)
        gm = (real_t)((long double)gm * ((long double)nnz / ((long double)m * (long double)n)));
    else if (nonneg)
        gm = std::max(gm, (real_t)0);
    if (std::fabs(gm) < std::sqrt(EPS_T)) gm = 0;
    return gm;
}

}  // namespace cmfit
