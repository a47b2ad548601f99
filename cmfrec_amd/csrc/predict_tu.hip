// predict_tu.hip -- predictions for chosen (row, col) pairs: cmfrec_hip_score_pairs (the kernel alone, test entry point), the
// cmfrec_hip_scorer_* handle (both factor matrices resident), the pair scorer cmfrec_hip_newrows_predict runs on device factors
// (newrows.hpp) and predict_X_old_collective_explicit / _implicit.  A translation unit of its own, like topn_tu.hip.  Every
// path launches through launch_score_pairs (predict_kernels.hpp).  The error of the predictions on a resident held-out set
// (cmfrec_hip_evalset_*, cmfrec_hip_scorer_errors, cmfrec_hip_pair_errors, and evalset_run for cmfrec_hip_session_errors in
// session.hip) launches through launch_score_errors (predict_error_kernels.hpp).
#include <algorithm>
#include <cmath>
#include <vector>
#include "device_base.hpp"
#include "newrows.hpp"
#include "predict_kernels.hpp"
#include "predict_error_kernels.hpp"

using namespace cmfhip;

namespace cmfhip {

// what a scoring call needs beside its operands: a stream, the device copies of a block of pairs and of its results, the
// events around the kernel.  The buffers are reused from call to call and grow on demand.
struct PairScorer {
    int device = 0, num_cus = 256;
    hipStream_t stream = nullptr;
    DevBuf<int> row, col;
    DevBuf<real_t> out;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double ms = 0;                             // the kernel over the blocks of the last call
    bool timed = false;
    void open(int dev)
    {
        open_device(dev, &device, &num_cus, &stream);
        HIP_CHECK(hipEventCreate(&ev0));
        HIP_CHECK(hipEventCreate(&ev1));
    }
    ~PairScorer()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

constexpr size_t PREDICT_BLOCK_MAX = (size_t)1 << 24;

// P: the operands on the device; row / col / out: the caller's host arrays.  Block by block: indices up, kernel, values down.
static int score_blocks(PairScorer &ps, ScoreParams<real_t> P, const int_t *row, const int_t *col, size_t n_pairs, real_t *out)
{
    DeviceScope scope(ps.device);
    switches_mut().reload();
    size_t block = PREDICT_BLOCK_MAX;
    if (switches().predict_block > 0) block = std::min<size_t>((size_t)switches().predict_block, PREDICT_BLOCK_MAX);
    block = std::min(block, n_pairs);
    ps.ms = 0;
    ps.row.alloc_at_least(block); ps.col.alloc_at_least(block); ps.out.alloc_at_least(block);
    for (size_t p0 = 0; p0 < n_pairs; p0 += block) {
        const size_t nb = std::min(block, n_pairs - p0);
        ps.row.upload(row + p0, nb, ps.stream);
        ps.col.upload(col + p0, nb, ps.stream);
        P.row = ps.row.ptr; P.col = ps.col.ptr; P.out = ps.out.ptr; P.n_pairs = nb;
        HIP_CHECK(hipEventRecord(ps.ev0, ps.stream));
        launch_score_pairs(ps.stream, ps.num_cus, P);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(ps.ev1, ps.stream));
        ps.out.download(out + p0, nb, ps.stream);
        HIP_CHECK(hipStreamSynchronize(ps.stream));
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, ps.ev0, ps.ev1));
        ps.ms += (double)t;
    }
    ps.timed = true;
    return 0;
}

PairScorer *pair_scorer_create(int device)
{
    PairScorer *ps = new PairScorer();
    try {
        ps->open(device);
    } catch (...) {
        delete ps;
        throw;
    }
    return ps;
}

void pair_scorer_destroy(PairScorer *ps) { delete ps; }

int pair_scorer_run(PairScorer *ps, const real_t *dA, size_t lda, int_t m, const real_t *dbiasA, size_t ldbiasA, const real_t *dB, size_t ldb,
                    int_t n, int_t kk, const real_t *dbiasB, real_t glob_mean, bool implicit, const int_t *row, const int_t *col,
                    size_t n_pairs, real_t *out)
{
    ScoreParams<real_t> P;
    P.A = dA; P.lda = lda; P.m = m; P.B = dB; P.ldb = ldb; P.n = n; P.kk = kk;
    P.biasA = dbiasA; P.ldbiasA = ldbiasA; P.biasB = dbiasB; P.glob_mean = glob_mean; P.implicit = implicit ? 1 : 0;
    return score_blocks(*ps, P, row, col, n_pairs, out);
}

double pair_scorer_ms(const PairScorer *ps) { return ps->ms; }

}  // namespace cmfhip

// a held-out set resident on the device, with the records of its evaluations' wavefronts and the events around their kernels
struct cmfrec_hip_evalset {
    int device = 0, num_cus = 256;
    hipStream_t stream = nullptr;              // the uploads; an evaluation runs on the stream of whoever owns the factors
    size_t n_pairs = 0;
    DevBuf<int> row, col;
    DevBuf<real_t> x, weight;
    DevBuf<cmfrec_hip_errors> partials;        // one record per wavefront of the launch, then the final one; grows on demand
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double ms = 0;
    size_t waves = 0;                          // wavefronts of the most recent evaluation's scoring launch
    bool timed = false;
    ~cmfrec_hip_evalset()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

namespace cmfhip {

// the one host pass over the weights: each finite and >= 0
static bool weights_ok(const real_t *w, size_t n)
{
    for (size_t i = 0; i < n; i++)
        if (!(w[i] >= (real_t)0) || w[i] > std::numeric_limits<real_t>::max()) return false;
    return true;
}

// the body of cmfrec_hip_evalset_create; the arrays have been checked
static void evalset_fill(cmfrec_hip_evalset &e, const int_t *row, const int_t *col, const real_t *x, const real_t *weight, size_t n_pairs, int device)
{
    open_device(device, &e.device, &e.num_cus, &e.stream);
    HIP_CHECK(hipEventCreate(&e.ev0));
    HIP_CHECK(hipEventCreate(&e.ev1));
    e.n_pairs = n_pairs;
    if (n_pairs == 0) return;
    e.row.upload(row, n_pairs, e.stream);
    e.col.upload(col, n_pairs, e.stream);
    e.x.upload(x, n_pairs, e.stream);
    if (weight) e.weight.upload(weight, n_pairs, e.stream);
    HIP_CHECK(hipStreamSynchronize(e.stream));     // the caller's arrays may go away
}

int evalset_usable(cmfrec_hip_evalset *e, const char *fn, int device, int_t m, int_t n)
{
    if (e == nullptr) {
        g_last_error = std::string(fn) + ": the monitor has no evaluation set";
        return 2;
    }
    if (device < 0) HIP_CHECK(hipGetDevice(&device));
    if (e->device != device) {
        g_last_error = std::string(fn) + ": the evaluation set lives on device " + std::to_string(e->device) + ", the fit runs on device " +
                       std::to_string(device);
        return 2;
    }
    bool any = false;
    if (e->n_pairs > 0) {
        DeviceScope scope(e->device);
        std::vector<int> row(e->n_pairs), col(e->n_pairs);
        std::vector<real_t> x(e->n_pairs);
        e->row.download(row.data(), e->n_pairs, e->stream);
        e->col.download(col.data(), e->n_pairs, e->stream);
        e->x.download(x.data(), e->n_pairs, e->stream);
        HIP_CHECK(hipStreamSynchronize(e->stream));
        for (size_t i = 0; i < e->n_pairs && !any; i++)
            any = row[i] >= 0 && row[i] < m && col[i] >= 0 && col[i] < n && !std::isnan(x[i]);
    }
    if (!any) {
        g_last_error = std::string(fn) + ": the evaluation set has no pair inside X with a value: nothing to watch";
        return 2;
    }
    return 0;
}

int evalset_run(cmfrec_hip_evalset *e, const char *fn, int device, int num_cus, hipStream_t st, const real_t *dA, size_t lda, int_t m,
                const real_t *dbiasA, size_t ldbiasA, const real_t *dB, size_t ldb, int_t n, int_t kk, const real_t *dbiasB, real_t glob_mean,
                bool implicit, real_t *dpred, cmfrec_hip_errors *out)
{
    if (e == nullptr || out == nullptr) {
        g_last_error = std::string(fn) + ": invalid arguments";
        return 2;
    }
    if (e->device != device) {
        g_last_error = std::string(fn) + ": the evaluation set lives on device " + std::to_string(e->device) + ", the factors on device " +
                       std::to_string(device);
        return 2;
    }
    DeviceScope scope(device);
    memset(out, 0, sizeof *out);
    e->ms = 0;
    e->waves = 0;
    e->timed = true;
    if (e->n_pairs == 0) return 0;
    ScoreParams<real_t> P;
    P.A = dA; P.lda = lda; P.m = m; P.B = dB; P.ldb = ldb; P.n = n; P.kk = kk;
    P.biasA = dbiasA; P.ldbiasA = ldbiasA; P.biasB = dbiasB; P.glob_mean = glob_mean; P.implicit = implicit ? 1 : 0;
    P.row = e->row.ptr; P.col = e->col.ptr; P.n_pairs = e->n_pairs;
    ErrorParams<real_t> E;
    E.x = e->x.ptr; E.weight = e->weight.ptr; E.pred = dpred;
    const char *cap = getenv("CMFREC_HIP_EVAL_WAVES");               // test hook, read per call
    const int max_waves = (cap != nullptr && cap[0] != 0) ? atoi(cap) : 0;
    const size_t waves = launch_score_errors(st, num_cus, max_waves, P, E, true);
    e->waves = waves;
    e->partials.alloc_at_least(waves + 1);
    E.partials = e->partials.ptr;
    HIP_CHECK(hipEventRecord(e->ev0, st));
    launch_score_errors(st, num_cus, max_waves, P, E, false);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(e->ev1, st));
    HIP_CHECK(hipMemcpyAsync(out, e->partials.ptr + waves, sizeof *out, hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, e->ev0, e->ev1));
    e->ms = (double)t;
    return 0;
}

}  // namespace cmfhip

struct cmfrec_hip_scorer {
    PairScorer ps;
    int m = 0, n = 0, kk = 0;
    size_t ld = 0;                             // columns of both packed matrices: kk rounded up to the 16-byte piece, the rest zero
    DevBuf<real_t> A, B, biasA, biasB;
    bool has_biasA = false, has_biasB = false;
    real_t glob_mean = 0;
    bool implicit = false;
};

extern "C" {

int cmfrec_hip_score_pairs(int m, int n, int kk, const real_t *A, size_t lda, int offA, const real_t *biasA, const real_t *B, size_t ldb,
                           int offB, const real_t *biasB, real_t glob_mean, int implicit, const int_t *row, const int_t *col, size_t n_pairs,
                           real_t *out)
{
    return guarded([&]() {
        auto bad = [](const char *what) { g_last_error = std::string("cmfrec_hip_score_pairs: ") + what; return 2; };
        if (m < 0 || n < 0 || offA < 0 || offB < 0) return bad("sizes and offsets >= 0");
        if (kk < 1) return bad("kk >= 1");
        if ((m > 0 && (!A || lda < (size_t)kk)) || (n > 0 && (!B || ldb < (size_t)kk)) || (n_pairs > 0 && (!row || !col || !out)))
            return bad("a missing operand or a leading dimension below the row length");
        if (n_pairs == 0) return 0;
        PairScorer ps;
        ps.open(-1);
        DevBuf<real_t> dA, dB, dba, dbb;
        const size_t na = m > 0 ? (size_t)offA + (size_t)m * lda : 0, nb = n > 0 ? (size_t)offB + (size_t)n * ldb : 0;
        if (na) dA.upload(A, na, ps.stream);
        if (nb) dB.upload(B, nb, ps.stream);
        const bool strided = biasA != nullptr && na > 0 && biasA >= A && biasA < A + na;
        if (biasA && !strided && m > 0) dba.upload(biasA, (size_t)m, ps.stream);
        if (biasB && n > 0) dbb.upload(biasB, (size_t)n, ps.stream);
        ScoreParams<real_t> P;
        P.A = na ? dA.ptr + offA : nullptr; P.lda = lda; P.m = m;
        P.B = nb ? dB.ptr + offB : nullptr; P.ldb = ldb; P.n = n; P.kk = kk;
        P.biasA = strided ? dA.ptr + (biasA - A) : dba.ptr; P.ldbiasA = strided ? lda : 1;
        P.biasB = dbb.ptr; P.glob_mean = glob_mean; P.implicit = implicit ? 1 : 0;
        return score_blocks(ps, P, row, col, n_pairs, out);
    });
}

// the body of cmfrec_hip_scorer_create.  min_rows: 1 for the handle's own contract; 0 for predict_X_old_*, where a side without
// rows is legal and every pair then gets the fallback value (that side's matrix and bias are not read and may be NULL)
static cmfrec_hip_scorer *scorer_create(const char *fn, int_t min_rows, const real_t *A, size_t lda, int_t m, const real_t *B, size_t ldb, int_t n,
                                        int_t kk, const real_t *biasA, const real_t *biasB, real_t glob_mean, int implicit, int device)
{
    cmfrec_hip_scorer *s = nullptr;
    const int rc = guarded([&]() {
        if (m < min_rows || n < min_rows || kk <= 0 || (m > 0 && (A == nullptr || lda < (size_t)kk)) ||
            (n > 0 && (B == nullptr || ldb < (size_t)kk))) {
            g_last_error = std::string(fn) + ": invalid arguments (A [m, lda] and B [n, ldb] with m, n >= " + (min_rows ? "1" : "0") +
                           ", kk >= 1 and lda, ldb >= kk)";
            return 2;
        }
        s = new cmfrec_hip_scorer();
        s->ps.open(device);
        hipStream_t st = s->ps.stream;
        constexpr int Ve = score_ve<real_t>();
        s->m = m; s->n = n; s->kk = kk; s->ld = (size_t)((kk + Ve - 1) / Ve) * Ve;
        s->A.alloc((size_t)m * s->ld);
        s->B.alloc((size_t)n * s->ld);
        if (s->ld != (size_t)kk) {
            if (m > 0) HIP_CHECK(hipMemsetAsync(s->A.ptr, 0, s->A.n * sizeof(real_t), st));
            if (n > 0) HIP_CHECK(hipMemsetAsync(s->B.ptr, 0, s->B.n * sizeof(real_t), st));
        }
        if (m > 0) upload_columns(s->A.ptr, s->ld, A, lda, (size_t)m, (size_t)kk, st);
        if (n > 0) upload_columns(s->B.ptr, s->ld, B, ldb, (size_t)n, (size_t)kk, st);
        // (the implicit rule knows no bias and no mean: none is kept, so that none can reach the kernel)
        s->implicit = implicit != 0;
        s->has_biasA = biasA != nullptr && m > 0 && !s->implicit; s->has_biasB = biasB != nullptr && n > 0 && !s->implicit;
        if (s->has_biasA) s->biasA.upload(biasA, (size_t)m, st);
        if (s->has_biasB) s->biasB.upload(biasB, (size_t)n, st);
        s->glob_mean = s->implicit ? (real_t)0 : glob_mean;
        HIP_CHECK(hipStreamSynchronize(st));       // the caller's matrices may go away
        return 0;
    });
    g_last_rc = rc;
    if (rc != 0) {
        delete s;
        return nullptr;
    }
    return s;
}

cmfrec_hip_scorer *cmfrec_hip_scorer_create(const real_t *A, size_t lda, int_t m, const real_t *B, size_t ldb, int_t n, int_t kk,
                                            const real_t *biasA, const real_t *biasB, real_t glob_mean, int implicit, int device)
{
    return scorer_create("cmfrec_hip_scorer_create", 1, A, lda, m, B, ldb, n, kk, biasA, biasB, glob_mean, implicit, device);
}

int cmfrec_hip_scorer_predict(cmfrec_hip_scorer *s, const int_t *row, const int_t *col, size_t n_pairs, real_t *out)
{
    return guarded([&]() {
        if (s == nullptr || (n_pairs > 0 && (!row || !col || !out))) {
            g_last_error = "cmfrec_hip_scorer_predict: invalid arguments";
            return 2;
        }
        if (n_pairs == 0) return 0;
        ScoreParams<real_t> P;
        P.A = s->A.ptr; P.lda = s->ld; P.m = s->m; P.B = s->B.ptr; P.ldb = s->ld; P.n = s->n; P.kk = s->kk;
        P.biasA = s->has_biasA ? s->biasA.ptr : nullptr; P.ldbiasA = 1; P.biasB = s->has_biasB ? s->biasB.ptr : nullptr;
        P.glob_mean = s->glob_mean; P.implicit = s->implicit ? 1 : 0;
        return score_blocks(s->ps, P, row, col, n_pairs, out);
    });
}

int cmfrec_hip_scorer_kernel_ms(cmfrec_hip_scorer *s, double *ms)
{
    if (s == nullptr || ms == nullptr || !s->ps.timed) {
        g_last_error = "cmfrec_hip_scorer_kernel_ms: no predict call with pairs on this handle yet";
        return 2;
    }
    *ms = s->ps.ms;
    return 0;
}

void cmfrec_hip_scorer_destroy(cmfrec_hip_scorer *s)
{
    if (s == nullptr) return;
    int cur = -1;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != s->ps.device && hipSetDevice(s->ps.device) == hipSuccess;
    delete s;
    if (sw) (void)hipSetDevice(cur);
}

cmfrec_hip_evalset *cmfrec_hip_evalset_create(const int_t *row, const int_t *col, const real_t *x, const real_t *weight, size_t n_pairs,
                                              int device)
{
    cmfrec_hip_evalset *e = nullptr;
    const int rc = guarded([&]() {
        if (n_pairs > 0 && (!row || !col || !x)) {
            g_last_error = "cmfrec_hip_evalset_create: row, col and x are required";
            return 2;
        }
        if (weight && !weights_ok(weight, n_pairs)) {
            g_last_error = "cmfrec_hip_evalset_create: a weight is negative, NaN or infinite";
            return 2;
        }
        e = new cmfrec_hip_evalset();
        evalset_fill(*e, row, col, x, weight, n_pairs, device);
        return 0;
    });
    g_last_rc = rc;
    if (rc != 0) {
        delete e;
        return nullptr;
    }
    return e;
}

int cmfrec_hip_evalset_kernel_ms(cmfrec_hip_evalset *e, double *ms)
{
    if (e == nullptr || ms == nullptr || !e->timed) {
        g_last_error = "cmfrec_hip_evalset_kernel_ms: no evaluation of this set yet";
        return 2;
    }
    *ms = e->ms;
    return 0;
}

int cmfrec_hip_evalset_launch_waves(cmfrec_hip_evalset *e, size_t *waves)
{
    if (e == nullptr || waves == nullptr || !e->timed) {
        g_last_error = "cmfrec_hip_evalset_launch_waves: no evaluation of this set yet";
        return 2;
    }
    *waves = e->waves;
    return 0;
}

void cmfrec_hip_evalset_destroy(cmfrec_hip_evalset *e)
{
    if (e == nullptr) return;
    int cur = -1;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != e->device && hipSetDevice(e->device) == hipSuccess;
    delete e;
    if (sw) (void)hipSetDevice(cur);
}

int cmfrec_hip_scorer_errors(cmfrec_hip_scorer *s, cmfrec_hip_evalset *e, cmfrec_hip_errors *out)
{
    return guarded([&]() {
        if (s == nullptr) {
            g_last_error = "cmfrec_hip_scorer_errors: invalid arguments";
            return 2;
        }
        return evalset_run(e, "cmfrec_hip_scorer_errors", s->ps.device, s->ps.num_cus, s->ps.stream, s->A.ptr, s->ld, s->m,
                           s->has_biasA ? s->biasA.ptr : nullptr, 1, s->B.ptr, s->ld, s->n, s->kk, s->has_biasB ? s->biasB.ptr : nullptr,
                           s->glob_mean, s->implicit, nullptr, out);
    });
}

int cmfrec_hip_pair_errors(int m, int n, int kk, const real_t *A, size_t lda, int offA, const real_t *biasA, const real_t *B, size_t ldb,
                           int offB, const real_t *biasB, real_t glob_mean, int implicit, const int_t *row, const int_t *col, size_t n_pairs,
                           const real_t *x, const real_t *weight, real_t *pred, cmfrec_hip_errors *out)
{
    return guarded([&]() {
        auto bad = [](const char *what) { g_last_error = std::string("cmfrec_hip_pair_errors: ") + what; return 2; };
        if (m < 0 || n < 0 || offA < 0 || offB < 0) return bad("sizes and offsets >= 0");
        if (kk < 1) return bad("kk >= 1");
        if ((m > 0 && (!A || lda < (size_t)kk)) || (n > 0 && (!B || ldb < (size_t)kk)) || (n_pairs > 0 && (!row || !col || !x)) || !out)
            return bad("a missing operand or a leading dimension below the row length");
        if (weight && !weights_ok(weight, n_pairs)) return bad("a weight is negative, NaN or infinite");
        cmfrec_hip_evalset e;
        evalset_fill(e, row, col, x, weight, n_pairs, -1);
        hipStream_t st = e.stream;
        DevBuf<real_t> dA, dB, dba, dbb, dpred;
        const size_t na = m > 0 ? (size_t)offA + (size_t)m * lda : 0, nb = n > 0 ? (size_t)offB + (size_t)n * ldb : 0;
        if (n_pairs > 0) {
            if (na) dA.upload(A, na, st);
            if (nb) dB.upload(B, nb, st);
        }
        const bool strided = biasA != nullptr && na > 0 && biasA >= A && biasA < A + na;
        if (n_pairs > 0 && biasA && !strided && m > 0) dba.upload(biasA, (size_t)m, st);
        if (n_pairs > 0 && biasB && n > 0) dbb.upload(biasB, (size_t)n, st);
        if (pred) dpred.alloc(n_pairs);
        const int rc = evalset_run(&e, "cmfrec_hip_pair_errors", e.device, e.num_cus, st, na ? dA.ptr + offA : nullptr, lda, m,
                                   strided ? dA.ptr + (biasA - A) : dba.ptr, strided ? lda : 1, nb ? dB.ptr + offB : nullptr, ldb, n, kk,
                                   dbb.ptr, glob_mean, implicit != 0, dpred.ptr, out);
        if (rc == 0 && pred && n_pairs > 0) {
            dpred.download(pred, n_pairs, st);
            HIP_CHECK(hipStreamSynchronize(st));
        }
        return rc;
    });
}

// scorer created, used once, destroyed
static int_t predict_old(const char *fn, int_t row[], int_t col[], real_t *predicted, size_t n_predict, real_t *A, real_t *biasA, real_t *B,
                         real_t *biasB, real_t glob_mean, int_t k, int_t k_user, int_t k_item, int_t k_main, int_t m, int_t n, bool implicit)
{
    if (n_predict == 0) return 0;
    // (m = 0 or n = 0 is legal, as in the reference: every pair is then out of range and gets the fallback value)
    if (!row || !col || !predicted || (m > 0 && !A) || (n > 0 && !B) || k < 0 || k_main < 0 || k_user < 0 || k_item < 0 || k + k_main < 1 || m < 0 ||
        n < 0) {
        g_last_error = std::string(fn) + ": invalid arguments";
        fprintf(stderr, "cmfrec_hip: %s\n", g_last_error.c_str());
        return 2;
    }
    const int_t kk = k + k_main;
    cmfrec_hip_scorer *s = scorer_create(fn, 0, A ? A + k_user : nullptr, (size_t)(k_user + kk), m, B ? B + k_item : nullptr, (size_t)(k_item + kk), n,
                                         kk, biasA, biasB, glob_mean, implicit ? 1 : 0, -1);
    if (s == nullptr) return g_last_rc > 3 ? 1 : (g_last_rc ? g_last_rc : 1);
    const int rc = cmfrec_hip_scorer_predict(s, row, col, n_predict, predicted);
    cmfrec_hip_scorer_destroy(s);
    return rc > 3 ? 1 : rc;
}

int_t predict_X_old_collective_explicit(
    int_t row[], int_t col[], real_t *predicted, size_t n_predict,
    real_t *A, real_t *biasA,
    real_t *B, real_t *biasB,
    real_t glob_mean,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    int_t m, int_t n_max,
    int nthreads)
{
    (void)nthreads;
    return predict_old("predict_X_old_collective_explicit", row, col, predicted, n_predict, A, biasA, B, biasB, glob_mean, k, k_user, k_item,
                       k_main, m, n_max, false);
}

int_t predict_X_old_collective_implicit(
    int_t row[], int_t col[], real_t *predicted, size_t n_predict,
    real_t *A,
    real_t *B,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    int_t m, int_t n,
    int nthreads)
{
    (void)nthreads;
    return predict_old("predict_X_old_collective_implicit", row, col, predicted, n_predict, A, nullptr, B, nullptr, (real_t)0, k, k_user, k_item,
                       k_main, m, n, true);
}

}  // extern "C"
