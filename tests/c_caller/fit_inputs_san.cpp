// The host-only intake of the two fit drivers (cmfrec_amd/csrc/fit_inputs.hpp) as a stand-alone program for AddressSanitizer and
// UBSan: the tiny cases of tests/test_fit_refusals_host.py -- the bad inputs among them: indices out of range, NULL triplets,
// repeated positions, all-NaN columns, more rows of side information than X -- through SideInput in the drivers' order, then the
// global mean in its four cases.  Every array is a heap block of exactly its length, so a read or write past it is reported.
// CPU only; build and run once per precision, from the repository root:
//   clang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all [-DCMFREC_HIP_FLOAT]
//       tests/c_caller/fit_inputs_san.cpp -o fit_inputs_san && ./fit_inputs_san
#include <cstdio>
#include <cstring>

#include "../../cmfrec_amd/csrc/fit_inputs.hpp"

using namespace cmfit;

static int failures = 0;
static void expect(bool ok, const char *what)
{
    if (!ok) { failures++; fprintf(stderr, "FAILED: %s\n", what); }
}

struct Triplets { std::vector<int_t> row, col; std::vector<real_t> val; bool null_row = false; };
static const real_t NaN = std::nan("");

// the sequence both drivers run on their two sides (without the driver-specific checks in between); "" when the intake goes through
static std::string intake(int_t m, int_t n, const std::vector<int_t> &ixA, const std::vector<int_t> &ixB, const std::vector<real_t> *U, int_t m_u,
                          const Triplets *Us, bool naz_U, const std::vector<real_t> *II, int_t n_i, const Triplets *Is, bool naz_I, bool centre,
                          std::vector<real_t> *means_U = nullptr)
{
    const int_t p = 2, q = 2;
    std::vector<real_t> cmU((size_t)p, -1), cmI((size_t)q, -1);
    SideInput su = user_side(U ? U->data() : nullptr, m_u, p, Us && !Us->null_row ? Us->row.data() : nullptr, Us ? Us->col.data() : nullptr,
                             Us ? Us->val.data() : nullptr, Us ? Us->col.size() : 0, centre ? cmU.data() : nullptr);
    SideInput si = item_side(II ? II->data() : nullptr, n_i, q, Is && !Is->null_row ? Is->row.data() : nullptr, Is ? Is->col.data() : nullptr,
                             Is ? Is->val.data() : nullptr, Is ? Is->col.size() : 0, centre ? cmI.data() : nullptr);
    std::string r = su.zero_fill(naz_U, m, ixA.data(), ixA.size(), true);
    if (r.empty()) r = si.zero_fill(naz_I, n, ixB.data(), ixB.size(), true);
    if (!r.empty()) return r;
    su.take_nan(); si.take_nan();
    if (su.nothing_present(su.nan_side || si.nan_side)) return "U empty";
    if (su.bad_triplets(m) || si.bad_triplets(n)) return "COO";
    su.drop_if_absent(); si.drop_if_absent();
    if (su.index_out_of_range()) return su.index_message();
    if (si.index_out_of_range()) return si.index_message();
    su.center(); si.center();
    for (int side = 0; side < 2; side++) {                       // what the session hand-over reads
        const SideInput &s = side ? si : su;
        double acc = 0;
        for (size_t e = 0; s.sparse() && e < s.nnz; e++) acc += (double)s.row[e] + (double)s.col[e] + (std::isnan(s.val[e]) ? 0 : (double)s.val[e]);
        for (size_t e = 0; s.dense && e < (size_t)s.rows * s.cols; e++) acc += (double)s.centred[e];
        for (size_t e = 0; s.sz.on && e < s.sz.nnz; e++) acc += (double)s.sz.val[e];
        for (int_t z : s.zero_rows) expect(z >= 0 && z < (side ? n : m), "zero row inside X");
        std::vector<unsigned char> mask; std::vector<real_t> mult;
        if (!s.nan.na_col.empty()) { s.nan.rules(4, true, mask, mult); expect(mask.size() == 2, "one rule per attribute"); }
        expect(acc == acc, "finite hand-over");
    }
    if (means_U) *means_U = cmU;
    return "";
}

int main()
{
    const int_t m = 4, n = 3;
    const std::vector<int_t> ixA = {0, 1, 2, 3, 0}, ixB = {0, 1, 2, 0, 2};
    const std::vector<real_t> X = {1, 2, 3, 4, 5}, W = {1, 2, 1, (real_t)0.5, 1};
    std::vector<real_t> U = {1, 2, 3, 4, 5, 6, 7, 8}, I = {1, 2, 3, 4, 5, 6};
    std::vector<real_t> U_nan = U, U_all(8, NaN), I_all(6, NaN), U_col_nan = U;
    U_nan[2] = NaN;
    for (int r = 0; r < 4; r++) U_col_nan[(size_t)r * 2 + 1] = NaN;                // one attribute without a present entry
    const Triplets good_U = {{0, 1, 3}, {0, 1, 0}, {1, 2, 3}}, good_I = {{0, 2}, {1, 0}, {(real_t)1.5, -2}};
    const Triplets bad_col = {{0, 1, 3}, {0, 5, 0}, {1, 2, 3}}, bad_row = {{0, -1, 3}, {0, 1, 0}, {1, 2, 3}}, huge = {{0, 2147483647, 3}, {0, 1, 0}, {1, 2, 3}};
    const Triplets repeated = {{1, 1, 1}, {0, 0, 0}, {1, 2, 3}}, nan_val = {{0, 1, 3}, {0, 1, 0}, {1, NaN, 3}};
    Triplets null_row = good_U; null_row.null_row = true;
    const std::string ixU = "cmfrec_hip: U index out of range.", ixI = "cmfrec_hip: I index out of range.";
    std::vector<real_t> means;

    for (int pass = 0; pass < 2; pass++) {                                         // the zero-filled form, then the triplets beyond the limit
        if (pass) setenv("CMFREC_HIP_ZEROFILL_MAX_GB", "1e-9", 1);
        for (int centre = 0; centre < 2; centre++) {
            expect(intake(m, n, ixA, ixB, nullptr, 4, &good_U, true, nullptr, 3, &good_I, true, centre) == "", "naz U and I");
            expect(intake(m, n, ixA, ixB, nullptr, 3, &good_U, true, nullptr, 0, nullptr, false, centre) == ixU, "naz U: a row at rows_side");
            expect(intake(m, n, ixA, ixB, nullptr, 4, &repeated, true, nullptr, 0, nullptr, false, centre, &means) == "", "naz U: repeated positions");
            expect(!centre || (means[0] == (real_t)1.5 && means[1] == 0), "repeated positions add up in the column means");
            expect(intake(m, n, ixA, ixB, nullptr, 4, &bad_col, true, nullptr, 0, nullptr, false, centre) == ixU, "naz U: column out of range");
            expect(intake(m, n, ixA, ixB, nullptr, 4, &bad_row, true, nullptr, 0, nullptr, false, centre) == ixU, "naz U: negative row");
            expect(intake(m, n, ixA, ixB, nullptr, 4, &huge, true, nullptr, 0, nullptr, false, centre) == ixU, "naz U: row INT_MAX");
            expect(intake(m, n, ixA, ixB, nullptr, 4, &null_row, true, nullptr, 0, nullptr, false, centre) == ixU, "naz U: NULL rows");
            expect(intake(m, n, ixA, ixB, nullptr, 0, nullptr, false, nullptr, 3, &bad_col, true, centre) == ixI, "naz I: column out of range");
            expect(intake(m, n, ixA, ixB, nullptr, 5, &good_U, true, nullptr, 0, nullptr, false, centre)
                       == "cmfrec_hip: NA_as_zero_U with more rows of U than X is not implemented.", "naz U: rows_side > rows_x");
            expect(intake(m, n, ixA, ixB, nullptr, 0, nullptr, false, nullptr, 4, &good_I, true, centre)
                       == "cmfrec_hip: NA_as_zero_I with more rows of I than X has columns is not implemented.", "naz I: rows_side > rows_x");
            expect(intake(m, n, ixA, ixB, nullptr, 4, &nan_val, true, nullptr, 0, nullptr, false, centre)
                       == (pass ? "cmfrec_hip: NA_as_zero_U beyond CMFREC_HIP_ZEROFILL_MAX_GB: NaN among the values of U is not implemented." : ""), "naz U: NaN value");
        }
    }
    unsetenv("CMFREC_HIP_ZEROFILL_MAX_GB");
    for (int centre = 0; centre < 2; centre++) {
        expect(intake(m, n, ixA, ixB, &U, 4, nullptr, false, &I, 3, nullptr, false, centre) == "", "dense U and I");
        expect(intake(m, n, ixA, ixB, &U, 4, nullptr, false, nullptr, 3, &good_I, false, centre) == "", "dense U, sparse I");
        expect(intake(m, n, ixA, ixB, &U_nan, 4, nullptr, false, &I, 3, nullptr, false, centre) == "", "NaN in U");
        expect(intake(m, n, ixA, ixB, &U_col_nan, 4, nullptr, false, nullptr, 0, nullptr, false, centre) == "", "an all-NaN column of U");
        expect(intake(m, n, ixA, ixB, &U_all, 4, nullptr, false, nullptr, 0, nullptr, false, centre) == "U empty", "all-NaN U");
        expect(intake(m, n, ixA, ixB, nullptr, 0, nullptr, false, &I_all, 3, nullptr, false, centre) == "", "all-NaN I goes on");
        expect(intake(m, n, ixA, ixB, nullptr, 4, &bad_col, false, nullptr, 0, nullptr, false, centre) == ixU, "sparse U: column out of range");
        expect(intake(m, n, ixA, ixB, nullptr, 4, &huge, false, nullptr, 0, nullptr, false, centre) == ixU, "sparse U: row INT_MAX");
        expect(intake(m, n, ixA, ixB, nullptr, 4, &bad_row, false, nullptr, 3, &bad_col, false, centre) == ixU, "U before I");
        expect(intake(m, n, ixA, ixB, nullptr, 4, &null_row, false, nullptr, 0, nullptr, false, centre) == "COO", "sparse U: NULL rows");
        expect(intake(m, n, ixA, ixB, nullptr, 5, &good_U, false, nullptr, 0, nullptr, false, centre) == "COO", "sparse U: rows beyond X");
        expect(intake(m, n, ixA, ixB, nullptr, 4, &bad_col, false, nullptr, 3, &null_row, false, centre) == "COO", "shape before indices");
    }
    // X with indices out of range beside naz: rows_without_data skips them (the drivers refuse them later)
    expect(intake(m, n, {0, 9, -3, 3, 0}, {0, 1, 7, 0, 2}, nullptr, 4, &good_U, true, nullptr, 3, &good_I, true, true) == "", "naz with bad X indices");

    // the global mean: four cases x the two reductions; checked against the sums written out
    const double sumX = 15, sumW = 5.5;
    for (int nthreads : {1, 8})
        for (int naz = 0; naz < 2; naz++) {
            const real_t plain = global_mean(X.data(), nullptr, X.size(), m, n, nthreads, naz, false);
            const real_t weighted = global_mean(X.data(), W.data(), X.size(), m, n, nthreads, naz, false);
            const double want = naz ? sumX / 12 : sumX / 5;
            const double wmean = nthreads >= 8 ? sumX / sumW : (1 * 1 + 2 * 2 + 3 * 1 + 4 * 0.5 + 5 * 1) / sumW;
            const double wwant = naz ? wmean / (sumW / (sumW + 12 - 5)) : wmean;
            expect(std::fabs((double)plain - want) < 1e-6 && std::fabs((double)weighted - wwant) < 1e-6, "global mean");
        }
    const std::vector<real_t> neg = {-1, -2, -3, -4, -5}, tiny = {(real_t)1e-12, 0, 0, 0, 0};
    expect(global_mean(neg.data(), nullptr, 5, m, n, 1, false, true) == 0 && global_mean(neg.data(), W.data(), 5, m, n, 8, false, true) == 0, "nonneg clamp");
    expect(global_mean(neg.data(), nullptr, 5, m, n, 1, false, false) == -3, "running mean");
    expect(global_mean(tiny.data(), nullptr, 5, m, n, 1, false, false) == 0 && global_mean(tiny.data(), W.data(), 5, m, n, 1, true, false) == 0, "flush below sqrt(eps)");
    expect(mean_of_entries(X.data(), 1, 1) == 1 && weighted_mean_of_entries(X.data(), W.data(), 1, 8) == 1, "one entry");

    // the dense X as COO and the epilogue's -w C^T colmeans
    std::vector<real_t> Xf = {1, NaN, 3, 4, 5, 6, NaN, NaN, NaN, 10, 11, 12}, Wf(12, 2);
    DenseX dx; dx.convert(Xf.data(), Wf.data(), m, n);
    expect(dx.val.size() == 8 && dx.w.size() == 8 && dx.na_row[2] == 3 && dx.na_col[1] == 2 && !dx.full, "dense X");
    std::vector<real_t> C = {1, 2, 3, 4}, cm = {1, -1}, outv(2, 0);
    fill_CtUbias(outv.data(), C.data(), cm.data(), 2, 2, (real_t)0.5);
    expect(outv[0] == 1 && outv[1] == 1, "CtUbias");

    printf("fit_inputs_san (%s): %s\n", sizeof(real_t) == 4 ? "float" : "double", failures ? "FAILED" : "all checks passed");
    return failures ? 1 : 0;
}
