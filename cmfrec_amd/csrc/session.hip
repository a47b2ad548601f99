// session.hip -- device-resident ALS session (level 3 of include/cmfrec_hip.h) and the
// operator-level entry points with host buffers (level 2).  The row solvers and the dense layer are reached through
// launch.hpp (launch_cg.hip, launch_chol.hip, launch_lowrank.hip, launch_dense.hip); of the kernels only the preprocessing
// (coo_device.hpp, dense_rows_device.hpp, side_zeros_kernels.hpp, impute_kernels.hpp) and small dense helpers are built here.
//
// The session owns the state the reference's fit drivers keep on the host
// (/root/reference/src/collective.c:7651-7677, :9468-9473): the factor matrices in the
// "[rows, k_tot + bias]" layout, the bias vectors, CSR and CSC copies of X, side information and
// the small k x k work matrices -- all resident in HBM for the whole fit.
#include "launch.hpp"
#include "coo_device.hpp"
#include "dense_rows_device.hpp"
#include "side_zeros_kernels.hpp"
#include "impute_kernels.hpp"
#include "newrows.hpp"
#include "newrows_naz_kernels.hpp"
#include <dlfcn.h>
#include <functional>
#include <limits>
#include <memory>
#include <new>

namespace cmfhip {

thread_local std::string g_last_error;
thread_local int g_last_rc = 0;      // return code that goes with g_last_error where the entry point returns a pointer

// out[count, kc] = alpha U[:count, :] M,  M [p, kc]
void side_times(const DeviceInfo &dev, const SideOperand &u, int count, int kc, int p, real_t alpha, const real_t *M, real_t *out,
                       size_t ldo)
{
    if (u.zeros != nullptr) sz_times(dev, *u.zeros, u.first, count, kc, alpha, M, (size_t)kc, out, ldo);
    else launch_gemm<false>(dev, count, kc, p, alpha, u.dense, (size_t)p, M, (size_t)kc, out, ldo);
}
// out[p, kc] = U[:rows, :]^T F[:rows, :kc]   (sparse-as-zeros: all its rows)
void side_transposed_times(const DeviceInfo &dev, const SideOperand &u, int rows, int kc, int p, const real_t *F, size_t ldF,
                                  real_t *out, size_t ldo)
{
    if (u.zeros != nullptr) sz_transposed_times(dev, *u.zeros, kc, F, ldF, out, ldo);
    else launch_gemm<true>(dev, p, kc, rows, (real_t)1, u.dense, (size_t)p, F, ldF, out, ldo);
}

void open_device(int device, int *device_id, int *num_cus, hipStream_t *stream)
{
    switches_mut().reload();           // the environment switches, once per session / operator call (device_base.hpp, Switches)
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0) {
        g_last_error = "cmfrec_hip: no HIP device available (this library has no CPU fallback)";
        fprintf(stderr, "%s\n", g_last_error.c_str());
        throw HipError{4};
    }
    if (device >= 0) HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipGetDevice(device_id));
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, *device_id));
    *num_cus = prop.multiProcessorCount;
    HIP_CHECK(hipStreamCreateWithFlags(stream, hipStreamNonBlocking));
}

void init_device(DeviceInfo &dev, int device)
{
    open_device(device, &dev.device, &dev.num_cus, &dev.stream);
}

}  // namespace cmfhip

using namespace cmfhip;

struct cmfrec_hip_session {
    cmfrec_hip_model mdl;
    DeviceInfo dev;
    int k_totA = 0, k_totB = 0, has_bias = 0;
    size_t ldA = 0, ldB = 0;
    DevBuf<real_t> A, B, biasA, biasB, C, D, U, II;
    SparseShard Xr, Xc;
    // sparse side information (missing = absent): CSR by user / item for the factor updates, CSC by attribute for C / D
    SparseShard Usr, Usc, Isr, Isc;
    bool sparseU = false, sparseI = false;
    // sparse side information whose ABSENT ENTRIES ARE ZEROS (cmfrec_hip_session_set_sideinfo_sparse_zeros): the same two shards and
    // the column means, standing in for the dense U / II in every product (SideOperand)
    SideZeros zerosU, zerosI;
    SideOperand side_operand(bool isU)
    {
        SideOperand o;
        SideZeros &z = isU ? zerosU : zerosI;
        if (z.on()) o.zeros = &z; else o.dense = isU ? U.ptr : II.ptr;
        return o;
    }
    // non-negativity constraints (solve_nonneg instead of the Cholesky solve; they switch the CG off for that matrix)
    bool nonneg = false, nonneg_C = false, nonneg_D = false;
    int max_cd_steps = 100;
    // implicit features of the explicit model (add_implicit_features): Ai [m, k+k_main], Bi [n, k+k_main] factorise the
    // binary "was observed" matrix alongside X (collective.c:8448-8534); Cholesky-type solves only
    bool implicit_feats = false;
    real_t w_implicit = 1;
    DevBuf<real_t> Ai, Bi, bitbi, bitbi_full, ones;
    // segment tables of the two-stage right-hand-side gather of the Ai / Bi updates ([0]: rows of X, [1]: columns)
    struct GatherSegs { DevBuf<int> seg_row, seg_off, row_first; int nseg = 0; } gsegs[2];
    DevBuf<real_t> gpartial, grhs;
    // per-matrix penalties, the reference's lam_unique / l1_lam_unique order (collective.c:430): user bias, item bias, A, B,
    // C, D -- after the w_main rescaling.  Scalar lam / l1_lam fill all six.
    real_t lam6[6] = {0, 0, 0, 0, 0, 0}, l16[6] = {0, 0, 0, 0, 0, 0};
    bool scale_bias_const = false;   // explicit model: the bias' lambda is not scaled row by row (lam6[0], [1] carry a constant factor)
    // NA_as_zero for the main matrix (explicit model without side information): absent entries of X are zeros.  Every
    // half-step is optimizeA Case 3 (common.c:3118-3205): one shared matrix, the stored values uncentred, and the constant
    // -sum over all opposing rows of (their bias + naz_mean) x row on every right-hand side (collective.c:8573-8600, :8756-8787)
    bool naz_X = false, naz_center = false;
    real_t x_subtract = 0;        // what the most recent set_X_coo* subtracted from the values (cmfrec_hip_session_set_NA_as_zero_X checks it)
    real_t naz_mean = 0;
    DevBuf<real_t> naz_part, naz_vec, naz_M, naz_rhs;
    // ... with observation weights (update_factor_naz_weighted): per entry w - 1 and the right-hand-side bracket, a zero array in
    // the place of the values for the CG kernels
    DevBuf<real_t> naz_g, naz_xt, naz_zero;
    DevBuf<real_t> naz_mult;            // NA_as_zero_X with sparse side information: the rows' lambda multiplier (every cell counts)
    DevBuf<int> zrowsA, zrowsB;   // rows every update of A / B leaves at zero (cmfrec_hip_session_set_zero_rows)
    int n_zrowsA = 0, n_zrowsB = 0;
    DevBuf<unsigned char> cfmaskA, cfmaskB;   // rows that take the closed form inside a CG update (cmfrec_hip_session_set_closed_form_rows)
    // ... and the attributes of dense side information with NaN (C / D updates): 1 = closed form, 2 = CG from zero with k_side + k steps
    DevBuf<unsigned char> cfmaskC, cfmaskD;
    bool cfC_any[3] = {false, false, false}, cfD_any[3] = {false, false, false};   // which mask values occur
    bool has_cfA = false, has_cfB = false;
    DevBuf<real_t> cf_keep;
    real_t l1_lam = 0;              // L1 penalty (after the w_main rescaling); C / D use l1_lam / w_user, / w_item
    // optional split of the local rows of A into contiguous parts, each with its own processing order: an A-step then
    // finishes part by part (one event each), so the all-gather of a finished part overlaps the rest of the step
    std::vector<std::unique_ptr<SparseShard>> XrParts;
    std::vector<int> partBegin;          // nparts + 1 local row offsets
    std::vector<hipEvent_t> partEv;
    DevBuf<real_t> gram, ctc, betbe, ucA, ucB;
    // low-rank row updates (lowrank_kernels.hpp): eigenvectors / values of w C^T C, rotated C and opposing factors,
    // rotated right-hand sides and solutions
    LowRankScratch lr;
    EigCache eigA, eigB;          // eigenvectors of w_user C^T C (A-steps) / w_item D^T D (B-steps), see EigCache
    // row-block shards of the explicit / collective model (distributed.py): U / I hold only the rows of this
    // rank's block, and the C / D update is split into partial sums over the local rows (side_part: [kc x kc | p x kc]),
    // an all-reduce by the caller, and the identical small solve on every rank
    bool side_local = false;
    DevBuf<real_t> side_part;
    GramWorkspace gws;
    // cmfrec_hip_session_snapshot / _restore: a second copy of A, B, biasA, biasB, C, D, Ai, Bi, allocated on first use
    DevBuf<real_t> snap[8];
    bool has_snapshot = false;
    cmfrec_hip_ranker *ranker = nullptr;  // cmfrec_hip_session_ranking: the session's own ranker, refreshed from B where it lives
    std::vector<EventPair> evA, evB;     // whole half-steps
    BinTimers binA, binB;                // row-update kernel launches per nnz bin

    hipEvent_t new_event()
    {
        hipEvent_t e;
        HIP_CHECK(hipEventCreate(&e));
        return e;
    }
    ~cmfrec_hip_session()
    {
        for (auto &p : evA) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        for (auto &p : evB) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        binA.clear(); binB.clear();
        for (auto e : partEv) (void)hipEventDestroy(e);
        if (ranker) cmfrec_hip_ranker_destroy(ranker);
    }
};

static void trim_events(std::vector<EventPair> &v)
{
    constexpr size_t CAP = 2048;
    if (v.size() < CAP) return;
    for (size_t e = 0; e < CAP / 2; e++) { (void)hipEventDestroy(v[e].a); (void)hipEventDestroy(v[e].b); }
    v.erase(v.begin(), v.begin() + CAP / 2);
}

extern "C" {

int cmfrec_hip_sizeof_real(void) { return (int)sizeof(real_t); }
int cmfrec_hip_sizeof_model(void) { return (int)sizeof(cmfrec_hip_model); }
const char *cmfrec_hip_build_info(void)
{
#ifdef CMFREC_HIP_FLOAT
    return "cmfrec_hip float gfx950";
#else
    return "cmfrec_hip double gfx950";
#endif
}
const char *cmfrec_hip_last_error(void) { return g_last_error.c_str(); }
void cmfrec_hip_reload_switches(void) { switches_mut().reload(); }

cmfrec_hip_session *cmfrec_hip_session_create(const cmfrec_hip_model *model, int device)
{
    cmfrec_hip_session *s = nullptr;
    int rc = guarded([&]() {
        const cmfrec_hip_model &m = *model;
        if (m.m <= 0 || m.n <= 0 || m.k < 0 || m.row_begin < 0 || m.row_end > m.m || m.col_begin < 0 ||
            m.col_end > m.n || m.row_begin > m.row_end || m.col_begin > m.col_end) {
            g_last_error = "cmfrec_hip: invalid model sizes";
            return 2;
        }
        if (m.implicit && (m.user_bias || m.item_bias)) {
            g_last_error = "cmfrec_hip: the implicit model has no biases";
            return 2;
        }
        if ((m.k_user && !m.p) || (m.k_item && !m.q)) {
            g_last_error = "cmfrec_hip: k_user / k_item need side information";
            return 2;
        }
        if ((m.p > 0 && m.m_u > m.m) || (m.q > 0 && m.n_i > m.n) || m.m_x > m.m || m.n_x > m.n) {
            g_last_error = "cmfrec_hip: m / n must be the rows of A / B: max(m_x, m_u) and max(n_x, n_i)";
            return 2;
        }
        s = new cmfrec_hip_session();
        s->mdl = m;
        init_device(s->dev, device);
        s->k_totA = m.k_user + m.k + m.k_main;
        s->k_totB = m.k_item + m.k + m.k_main;
        s->has_bias = (m.user_bias || m.item_bias) ? 1 : 0;
        s->ldA = (size_t)(s->k_totA + s->has_bias);
        s->ldB = (size_t)(s->k_totB + s->has_bias);
        s->A.alloc((size_t)m.m * s->ldA);
        s->B.alloc((size_t)m.n * s->ldB);
        HIP_CHECK(hipMemsetAsync(s->A.ptr, 0, s->A.n * sizeof(real_t), s->dev.stream));
        HIP_CHECK(hipMemsetAsync(s->B.ptr, 0, s->B.n * sizeof(real_t), s->dev.stream));
        if (s->has_bias) {
            s->biasA.alloc(m.m);
            s->biasB.alloc(m.n);
            HIP_CHECK(hipMemsetAsync(s->biasA.ptr, 0, (size_t)m.m * sizeof(real_t), s->dev.stream));
            HIP_CHECK(hipMemsetAsync(s->biasB.ptr, 0, (size_t)m.n * sizeof(real_t), s->dev.stream));
        }
        int kmax = std::max(s->k_totA, s->k_totB) + 1;
        for (int e = 0; e < 6; e++) s->lam6[e] = s->mdl.lam;
        s->gram.alloc((size_t)kmax * kmax);
        s->ctc.alloc((size_t)kmax * kmax);
        s->betbe.alloc((size_t)kmax * kmax);
        if (m.p > 0) s->C.alloc((size_t)m.p * (m.k_user + m.k));
        if (m.q > 0) s->D.alloc((size_t)m.q * (m.k_item + m.k));
        if (m.p > 0 && m.use_cg) s->ucA.alloc((size_t)std::max(1, m.m_u) * (m.k_user + m.k));     // U C of the block CG
        if (m.q > 0 && m.use_cg) s->ucB.alloc((size_t)std::max(1, m.n_i) * (m.k_item + m.k));
        return 0;
    });
    g_last_rc = rc;
    if (rc != 0) {
        delete s;
        return nullptr;
    }
    return s;
}
int cmfrec_hip_last_error_code(void) { return g_last_rc; }

void cmfrec_hip_session_destroy(cmfrec_hip_session *s)
{
    if (!s) return;
    (void)hipStreamSynchronize(s->dev.stream);
    delete s;
}

static int weights_allowed(const cmfrec_hip_session *s, const char *fn)
{
    if (s->mdl.implicit) { g_last_error = std::string(fn) + ": observation weights belong to the explicit model"; return 2; }
    return 0;
}

// NA_as_zero_X with observation weights: an absent entry is a zero of weight one, so the rows' lambda multipliers under scale_lam
// count them (wsumA / wsumB, collective.c:7991-8022).  Kept in SparseShard::wsum_naz beside the plain sums of the weights and
// rebuilt whenever the flag is switched on or X is uploaded again (the plain sums stay what the ordinary weighted updates and
// cmfrec_hip_session_set_lambda_multipliers('A' / 'B') use).
static void refresh_naz_multipliers(cmfrec_hip_session *s)
{
    if (!s->naz_X || !s->Xr.weighted()) { s->Xr.wsum_naz.release(); s->Xc.wsum_naz.release(); return; }
    HIP_CHECK(hipSetDevice(s->dev.device));
    hipStream_t st = s->dev.stream;
    s->Xr.wsum_naz.alloc_at_least((size_t)s->Xr.nrows); s->Xc.wsum_naz.alloc_at_least((size_t)s->Xc.nrows);
    hipLaunchKernelGGL(naz_wsum_kernel<real_t>, grid1d((size_t)s->Xr.nrows), dim3(256), 0, st, s->Xr.p.ptr, s->Xr.w.ptr, s->Xr.nrows,
                       s->mdl.n, s->Xr.wsum_naz.ptr);
    hipLaunchKernelGGL(naz_wsum_kernel<real_t>, grid1d((size_t)s->Xc.nrows), dim3(256), 0, st, s->Xc.p.ptr, s->Xc.w.ptr, s->Xc.nrows,
                       s->mdl.m, s->Xc.wsum_naz.ptr);
    HIP_CHECK(hipGetLastError());
}

int cmfrec_hip_session_set_X_weighted(cmfrec_hip_session *s, const size_t *csr_p, const int_t *csr_i, const real_t *csr_v,
                                      const real_t *csr_w, const size_t *csc_p, const int_t *csc_i, const real_t *csc_v,
                                      const real_t *csc_w)
{
    return guarded([&]() {
        if ((csr_w != nullptr) != (csc_w != nullptr)) { g_last_error = "cmfrec_hip_session_set_X_weighted: weights for both orientations or none"; return 2; }
        if (csr_w != nullptr) { const int rc = weights_allowed(s, "cmfrec_hip_session_set_X_weighted"); if (rc) return rc; }
        HIP_CHECK(hipSetDevice(s->dev.device));
        s->Xr.opp_row_bytes_hint = s->Xc.opp_row_bytes_hint = (size_t)(s->mdl.k + s->mdl.k_main) * sizeof(real_t);
        shard_from_csr(s->Xr, s->mdl.row_end - s->mdl.row_begin, csr_p, csr_i, csr_v, s->mdl.n, s->dev.stream, csr_w);
        shard_from_csr(s->Xc, s->mdl.col_end - s->mdl.col_begin, csc_p, csc_i, csc_v, s->mdl.m, s->dev.stream, csc_w);
        refresh_naz_multipliers(s);
        return 0;
    });
}

int cmfrec_hip_session_set_X(cmfrec_hip_session *s, const size_t *csr_p, const int_t *csr_i, const real_t *csr_v,
                             const size_t *csc_p, const int_t *csc_i, const real_t *csc_v)
{
    return cmfrec_hip_session_set_X_weighted(s, csr_p, csr_i, csr_v, nullptr, csc_p, csc_i, csc_v, nullptr);
}

int cmfrec_hip_session_set_A_parts(cmfrec_hip_session *s, const size_t *csr_p, const int_t *csr_i, const real_t *csr_v,
                                   int nparts)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const int nrows = s->mdl.row_end - s->mdl.row_begin;
        s->XrParts.clear(); s->partBegin.clear();
        for (auto e : s->partEv) (void)hipEventDestroy(e);
        s->partEv.clear();
        if (nparts <= 1) return 0;
        if (s->mdl.p > 0) { g_last_error = "cmfrec_hip_session_set_A_parts: not with user side information"; return 2; }
        if (s->Xr.weighted()) { g_last_error = "cmfrec_hip_session_set_A_parts: not with observation weights"; return 2; }
        // no host CSR given: cut the resident one (shards built on the device)
        std::vector<size_t> hp; std::vector<int_t> hi; std::vector<real_t> hv;
        if (csr_p == nullptr) {
            if (s->Xr.nrows != nrows) { g_last_error = "cmfrec_hip_session_set_A_parts: set X first"; return 2; }
            hp.resize((size_t)nrows + 1); hi.resize(std::max<size_t>(s->Xr.nnz, 1)); hv.resize(std::max<size_t>(s->Xr.nnz, 1));
            s->Xr.p.download(hp.data(), (size_t)nrows + 1, s->dev.stream);
            s->Xr.i.download(hi.data(), s->Xr.nnz, s->dev.stream);
            s->Xr.v.download(hv.data(), s->Xr.nnz, s->dev.stream);
            HIP_CHECK(hipStreamSynchronize(s->dev.stream));
            csr_p = hp.data(); csr_i = hi.data(); csr_v = hv.data();
        }
        nparts = std::min(nparts, std::max(1, nrows));
        const int step = (nrows + nparts - 1) / nparts;
        for (int c = 0; c <= nparts; c++) s->partBegin.push_back(std::min(c * step, nrows));
        std::vector<size_t> pp;
        for (int c = 0; c < nparts; c++) {
            const int r0 = s->partBegin[c], r1 = s->partBegin[c + 1];
            pp.resize((size_t)(r1 - r0) + 1);
            for (int r = r0; r <= r1; r++) pp[r - r0] = csr_p[r] - csr_p[r0];
            s->XrParts.emplace_back(new SparseShard());
            s->XrParts.back()->is_part = true;
            s->XrParts.back()->opp_row_bytes_hint = (size_t)(s->mdl.k + s->mdl.k_main) * sizeof(real_t);
            shard_from_csr(*s->XrParts.back(), r1 - r0, pp.data(), csr_i + csr_p[r0], csr_v + csr_p[r0], s->mdl.n, s->dev.stream);
            HIP_CHECK(hipStreamSynchronize(s->dev.stream));              // pp is reused
            hipEvent_t e;
            HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            s->partEv.push_back(e);
        }
        return 0;
    });
}

int cmfrec_hip_session_part_range(cmfrec_hip_session *s, int part, int *begin, int *end)
{
    if (part < 0 || part >= (int)s->XrParts.size()) return 2;
    if (begin) *begin = s->partBegin[part];
    if (end) *end = s->partBegin[part + 1];
    return 0;
}

int cmfrec_hip_session_nparts(cmfrec_hip_session *s) { return (int)s->XrParts.size(); }

int cmfrec_hip_session_stream_wait_part(cmfrec_hip_session *s, int part, void *stream)
{
    return guarded([&]() {
        if (part < 0 || part >= (int)s->partEv.size()) { g_last_error = "cmfrec_hip_session_stream_wait_part: no such part"; return 2; }
        HIP_CHECK(hipStreamWaitEvent((hipStream_t)stream, s->partEv[part], 0));
        return 0;
    });
}

// weight: one observation weight per entry (explicit model), or null
int cmfrec_hip_session_set_X_coo_weighted(cmfrec_hip_session *s, const int_t *row, const int_t *col, const real_t *val,
                                          const real_t *weight, size_t nnz, real_t subtract, real_t alpha)
{
    return guarded([&]() {
        const cmfrec_hip_model &m = s->mdl;
        if (m.row_begin != 0 || m.row_end != m.m || m.col_begin != 0 || m.col_end != m.n) {
            g_last_error = "cmfrec_hip_session_set_X_coo: only for sessions that own all rows and columns";
            return 2;
        }
        if (weight != nullptr) { const int rc = weights_allowed(s, "cmfrec_hip_session_set_X_coo_weighted"); if (rc) return rc; }
        HIP_CHECK(hipSetDevice(s->dev.device));
        DevBuf<int> dr, dc; DevBuf<real_t> dv, dw;
        dr.upload(row, nnz, s->dev.stream); dc.upload(col, nnz, s->dev.stream); dv.upload(val, nnz, s->dev.stream);
        if (weight != nullptr) dw.upload(weight, nnz, s->dev.stream);
        s->Xr.opp_row_bytes_hint = s->Xc.opp_row_bytes_hint = (size_t)(m.k + m.k_main) * sizeof(real_t);
        s->x_subtract = subtract;
        shard_from_coo(s->Xr, m.m, m.n, dr.ptr, dc.ptr, dv.ptr, nnz, subtract, alpha, s->dev.stream, dw.ptr);
        shard_from_coo(s->Xc, m.n, m.m, dc.ptr, dr.ptr, dv.ptr, nnz, subtract, alpha, s->dev.stream, dw.ptr);
        refresh_naz_multipliers(s);
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        return 0;
    });
}

int cmfrec_hip_session_set_X_coo(cmfrec_hip_session *s, const int_t *row, const int_t *col, const real_t *val,
                                 size_t nnz, real_t subtract, real_t alpha)
{
    return cmfrec_hip_session_set_X_coo_weighted(s, row, col, val, nullptr, nnz, subtract, alpha);
}

// One shard from a COO triplet that already lives in HBM (multi-GPU set-up: the triplets come out of the
// all-to-all exchange of the ranks' blocks, distributed.py): which = 'r' -> CSR of the local rows (d_key = row - row_begin,
// d_other = global column), 'c' -> CSC of the local columns (d_key = column - col_begin, d_other = global row).
// x := (x - subtract) * alpha as in cmfrec_hip_session_set_X_coo.  The pointers are device pointers.
int cmfrec_hip_session_set_X_coo_device(cmfrec_hip_session *s, int which, const int_t *d_key, const int_t *d_other,
                                        const real_t *d_val, size_t nnz, real_t subtract, real_t alpha)
{
    return guarded([&]() {
        const cmfrec_hip_model &m = s->mdl;
        if (which != 'r' && which != 'c') { g_last_error = "cmfrec_hip_session_set_X_coo_device: which must be 'r' or 'c'"; return 2; }
        HIP_CHECK(hipSetDevice(s->dev.device));
        s->Xr.opp_row_bytes_hint = s->Xc.opp_row_bytes_hint = (size_t)(m.k + m.k_main) * sizeof(real_t);
        if (which == 'r') shard_from_coo(s->Xr, m.row_end - m.row_begin, m.n, d_key, d_other, d_val, nnz, subtract, alpha, s->dev.stream);
        else shard_from_coo(s->Xc, m.col_end - m.col_begin, m.m, d_key, d_other, d_val, nnz, subtract, alpha, s->dev.stream);
        refresh_naz_multipliers(s);       // (this upload carries no weights: the multipliers of a weighted predecessor go)
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        return 0;
    });
}

int cmfrec_hip_session_init_biases(cmfrec_hip_session *s, real_t lam_user, real_t lam_item)
{
    return guarded([&]() {
        const cmfrec_hip_model &m = s->mdl;
        if (m.implicit || !s->has_bias) { g_last_error = "cmfrec_hip_session_init_biases: the model has no biases"; return 2; }
        if (m.row_begin != 0 || m.row_end != m.m || m.col_begin != 0 || m.col_end != m.n) {
            g_last_error = "cmfrec_hip_session_init_biases: only for sessions that own all rows and columns";
            return 2;
        }
        HIP_CHECK(hipSetDevice(s->dev.device));
        hipStream_t st = s->dev.stream;
        // under scale_lam_sideinfo the rows that have side information count its attributes too (wsumA / wsumB,
        // collective.c:8071-8104).  For sparse side information the reference adds `U_csr_p[row+1] - U_csr[row]` there -- an
        // index minus a value (:8086): nothing to pin, so that combination is refused
        if ((s->Xr.weighted() || s->Xc.weighted()) && (m.scale_lam_sideinfo || s->scale_bias_const)) {
            g_last_error = "cmfrec_hip: bias start values with observation weights and scale_lam_sideinfo / scale_bias_const are not implemented";
            return 2;
        }
        if (m.scale_lam_sideinfo && ((s->sparseU && m.user_bias) || (s->sparseI && m.item_bias))) {
            g_last_error = "cmfrec_hip: bias start values with scale_lam_sideinfo and sparse side information are not defined by the reference";
            return 2;
        }
        auto sweep = [&](const SparseShard &X, const real_t *other, real_t lam_b, int user_rule, real_t *bias) {
            const bool users = (&X == &s->Xr);
            if (X.weighted()) {                                           // common.c:4180-4205, :4672-4692, :4826-4847
                const int onesided = (m.user_bias != m.item_bias) ? 1 : 0;
                const real_t *wd = m.scale_lam ? X.wsum.ptr : nullptr;
                if (X.n_long > 0)
                    hipLaunchKernelGGL(bias_sweep_weighted_long_kernel, dim3(X.n_long), dim3(64), 0, st, X.p.ptr, X.i.ptr, X.v.ptr, X.w.ptr,
                                       other, X.order.ptr, X.n_long, lam_b, wd, onesided, bias);
                if (X.nrows > X.n_long)
                    hipLaunchKernelGGL(bias_sweep_weighted_kernel, dim3((X.nrows - X.n_long + 63) / 64), dim3(64), 0, st, X.p.ptr, X.i.ptr,
                                       X.v.ptr, X.w.ptr, other, X.order.ptr, X.n_long, X.nrows, lam_b, wd, onesided, bias);
                return;
            }
            const int extra = m.scale_lam_sideinfo ? (users ? m.p : m.q) : 0, extra_rows = users ? m.m_u : m.n_i;
            if (X.n_long > 0)
                hipLaunchKernelGGL(bias_sweep_long_kernel, dim3(X.n_long), dim3(64), 0, st, X.p.ptr, X.i.ptr, X.v.ptr, other,
                                   X.order.ptr, X.n_long, lam_b, (int)m.scale_lam, user_rule, bias, extra, extra_rows);
            if (X.nrows > X.n_long)
                hipLaunchKernelGGL(bias_sweep_kernel, dim3((X.nrows - X.n_long + 63) / 64), dim3(64), 0, st, X.p.ptr, X.i.ptr,
                                   X.v.ptr, other, X.order.ptr, X.n_long, X.nrows, lam_b, (int)m.scale_lam, user_rule, bias, extra,
                                   extra_rows);
        };
        if (m.user_bias && !m.item_bias) {                                // collective.c:8166-8185
            sweep(s->Xr, nullptr, lam_user, 0, s->biasA.ptr);
        } else if (m.item_bias && !m.user_bias) {                         // :8187-8204 (only when the B-step uses CG)
            if (m.use_cg) sweep(s->Xc, nullptr, lam_item, 0, s->biasB.ptr);
        } else {                                                          // common.c:4410-4909, five sweeps, items first
            HIP_CHECK(hipMemsetAsync(s->biasA.ptr, 0, (size_t)m.m * sizeof(real_t), st));
            HIP_CHECK(hipMemsetAsync(s->biasB.ptr, 0, (size_t)m.n * sizeof(real_t), st));
            for (int it = 0; it < 5; it++) {
                sweep(s->Xc, s->biasA.ptr, lam_item, 0, s->biasB.ptr);
                sweep(s->Xr, s->biasB.ptr, lam_user, 1, s->biasA.ptr);
            }
        }
        if (m.user_bias)
            hipLaunchKernelGGL(col_insert_kernel<real_t>, grid1d(m.m), dim3(256), 0, st, s->A.ptr, s->ldA, m.m, s->k_totA, s->biasA.ptr);
        if (m.item_bias)
            hipLaunchKernelGGL(col_insert_kernel<real_t>, grid1d(m.n), dim3(256), 0, st, s->B.ptr, s->ldB, m.n, s->k_totB, s->biasB.ptr);
        HIP_CHECK(hipGetLastError());
        return 0;
    });
}

int cmfrec_hip_session_get_X(cmfrec_hip_session *s, int which, size_t *indptr, int_t *indices, real_t *values,
                             int_t *order)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const SparseShard &X = (which == 'r' || which == 'R') ? s->Xr : s->Xc;
        if (indptr) X.p.download(indptr, (size_t)X.nrows + 1, s->dev.stream);
        if (indices) X.i.download(indices, X.nnz, s->dev.stream);
        if (values) X.v.download(values, X.nnz, s->dev.stream);
        if (order) X.order.download(order, (size_t)X.nrows, s->dev.stream);
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        return 0;
    });
}

static void upload_padded(cmfrec_hip_session *s, const real_t *host, size_t rows, int cols, real_t *dst, size_t ldd)
{
    if (!host || rows == 0) return;
    if ((size_t)cols == ldd) {
        HIP_CHECK(hipMemcpyAsync(dst, host, rows * cols * sizeof(real_t), hipMemcpyHostToDevice, s->dev.stream));
    } else {
        HIP_CHECK(hipMemcpy2DAsync(dst, ldd * sizeof(real_t), host, (size_t)cols * sizeof(real_t),
                                   (size_t)cols * sizeof(real_t), rows, hipMemcpyHostToDevice, s->dev.stream));
    }
}
static void download_padded(cmfrec_hip_session *s, real_t *host, size_t rows, int cols, const real_t *src, size_t lds)
{
    if (!host || rows == 0) return;
    if ((size_t)cols == lds) {
        HIP_CHECK(hipMemcpyAsync(host, src, rows * cols * sizeof(real_t), hipMemcpyDeviceToHost, s->dev.stream));
    } else {
        HIP_CHECK(hipMemcpy2DAsync(host, (size_t)cols * sizeof(real_t), src, lds * sizeof(real_t),
                                   (size_t)cols * sizeof(real_t), rows, hipMemcpyDeviceToHost, s->dev.stream));
    }
}

int cmfrec_hip_session_set_factors(cmfrec_hip_session *s, const real_t *A, const real_t *B, const real_t *biasA,
                                   const real_t *biasB, const real_t *C, const real_t *D)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const cmfrec_hip_model &m = s->mdl;
        hipStream_t st = s->dev.stream;
        s->eigA.fresh = false; s->eigB.fresh = false;
        upload_padded(s, A, m.m, s->k_totA, s->A.ptr, s->ldA);
        upload_padded(s, B, m.n, s->k_totB, s->B.ptr, s->ldB);
        if (s->has_bias) {
            // bias column of the [rows, k_tot+1] layout: the bias itself or ones (collective.c:8283-8317)
            if (biasA && m.user_bias) s->biasA.upload(biasA, m.m, st);
            if (biasB && m.item_bias) s->biasB.upload(biasB, m.n, st);
            if (m.user_bias)
                hipLaunchKernelGGL(col_insert_kernel<real_t>, grid1d(m.m), dim3(256), 0, st, s->A.ptr, s->ldA, m.m, s->k_totA, s->biasA.ptr);
            else
                hipLaunchKernelGGL(col_fill_kernel<real_t>, grid1d(m.m), dim3(256), 0, st, s->A.ptr, s->ldA, m.m, s->k_totA, (real_t)1);
            if (m.item_bias)
                hipLaunchKernelGGL(col_insert_kernel<real_t>, grid1d(m.n), dim3(256), 0, st, s->B.ptr, s->ldB, m.n, s->k_totB, s->biasB.ptr);
            else
                hipLaunchKernelGGL(col_fill_kernel<real_t>, grid1d(m.n), dim3(256), 0, st, s->B.ptr, s->ldB, m.n, s->k_totB, (real_t)1);
            HIP_CHECK(hipGetLastError());
        }
        if (C && m.p > 0) s->C.upload(C, (size_t)m.p * (m.k_user + m.k), st);
        if (D && m.q > 0) s->D.upload(D, (size_t)m.q * (m.k_item + m.k), st);
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}

int cmfrec_hip_session_get_factors(cmfrec_hip_session *s, real_t *A, real_t *B, real_t *biasA, real_t *biasB,
                                   real_t *C, real_t *D)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const cmfrec_hip_model &m = s->mdl;
        hipStream_t st = s->dev.stream;
        download_padded(s, A, m.m, s->k_totA, s->A.ptr, s->ldA);
        download_padded(s, B, m.n, s->k_totB, s->B.ptr, s->ldB);
        if (biasA && m.user_bias) s->biasA.download(biasA, m.m, st);
        if (biasB && m.item_bias) s->biasB.download(biasB, m.n, st);
        if (C && m.p > 0) s->C.download(C, (size_t)m.p * (m.k_user + m.k), st);
        if (D && m.q > 0) s->D.download(D, (size_t)m.q * (m.k_item + m.k), st);
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}

int cmfrec_hip_session_set_sideinfo(cmfrec_hip_session *s, const real_t *U, const real_t *II)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const cmfrec_hip_model &m = s->mdl;
        if (U && m.p > 0) { s->U.upload(U, (size_t)m.m_u * m.p, s->dev.stream); s->zerosU.clear(); }
        if (II && m.q > 0) { s->II.upload(II, (size_t)m.n_i * m.q, s->dev.stream); s->zerosI.clear(); }
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        return 0;
    });
}

// Row-block shards: U holds the rows [row_begin, min(row_end, m_u)) only, I the rows [col_begin, min(col_end, n_i)).
int cmfrec_hip_session_set_sideinfo_local(cmfrec_hip_session *s, const real_t *U_local, const real_t *I_local)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const cmfrec_hip_model &m = s->mdl;
        const int ru = std::max(0, std::min(m.row_end, m.m_u) - m.row_begin), ri = std::max(0, std::min(m.col_end, m.n_i) - m.col_begin);
        if (U_local && m.p > 0 && ru > 0) s->U.upload(U_local, (size_t)ru * m.p, s->dev.stream);
        if (I_local && m.q > 0 && ri > 0) s->II.upload(I_local, (size_t)ri * m.q, s->dev.stream);
        s->side_local = true;
        s->zerosU.clear(); s->zerosI.clear();          // (a row block runs on the dense matrix alone)
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        return 0;
    });
}

// C / D update of a row-block shard, first half (optimizeA Case 1, common.c:2793-2991, split over the ranks): the partial
// sums over the LOCAL rows of the factor matrix F (A for 'C', B for 'D') that carry side information,
//   side_part = [ F_loc^T F_loc  (kc x kc) | U_loc^T F_loc  (p x kc) ],
// for the caller to all-reduce (cmfrec_hip_session_device_ptr(s, 'P')).  Dense side information only.
int cmfrec_hip_session_sideinfo_partial(cmfrec_hip_session *s, int which)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const cmfrec_hip_model &m = s->mdl;
        const DeviceInfo &dev = s->dev;
        const bool isC = (which == 'C');
        const int p = isC ? m.p : m.q;
        if ((which != 'C' && which != 'D') || p <= 0 || (isC ? s->sparseU : s->sparseI) || (isC ? s->zerosU : s->zerosI).on()) {
            g_last_error = "cmfrec_hip_session_sideinfo_partial: dense side information on that side is required";
            return 2;
        }
        const int rows_u = isC ? m.m_u : m.n_i, begin = isC ? m.row_begin : m.col_begin, end = isC ? m.row_end : m.col_end;
        const int local = std::max(0, std::min(end, rows_u) - begin);
        const int kc = (isC ? m.k_user : m.k_item) + m.k;
        const real_t *F = (isC ? s->A.ptr : s->B.ptr) + (size_t)begin * (isC ? s->ldA : s->ldB);
        const size_t ldF = isC ? s->ldA : s->ldB;
        const real_t *Um = (isC ? s->U.ptr : s->II.ptr) + (s->side_local ? (size_t)0 : (size_t)begin * p);
        s->side_part.alloc_at_least((size_t)kc * kc + (size_t)p * kc);
        HIP_CHECK(hipMemsetAsync(s->side_part.ptr, 0, ((size_t)kc * kc + (size_t)p * kc) * sizeof(real_t), dev.stream));
        if (local > 0) {
            launch_gram(dev, s->gws, F, ldF, local, kc, s->side_part.ptr, (real_t)1, (real_t)0);
            launch_gemm<true>(dev, p, kc, local, (real_t)1, Um, (size_t)p, F, ldF, s->side_part.ptr + (size_t)kc * kc, (size_t)kc);
        }
        return 0;
    });
}

// ... second half, on the all-reduced sums: C := (U^T F) (F^T F + lam I)^-1, the same on every rank
int cmfrec_hip_session_sideinfo_finish(cmfrec_hip_session *s, int which)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const cmfrec_hip_model &m = s->mdl;
        const DeviceInfo &dev = s->dev;
        const bool isC = (which == 'C');
        const int p = isC ? m.p : m.q;
        if ((which != 'C' && which != 'D') || p <= 0 || (isC ? s->sparseU : s->sparseI) || (isC ? s->zerosU : s->zerosI).on()) {
            g_last_error = "cmfrec_hip_session_sideinfo_finish: dense side information on that side is required";
            return 2;
        }
        const int rows_u = isC ? m.m_u : m.n_i;
        const int kc = (isC ? m.k_user : m.k_item) + m.k;
        real_t *Cm = isC ? s->C.ptr : s->D.ptr;
        (isC ? s->eigA : s->eigB).fresh = false;
        const real_t w = isC ? m.w_user : m.w_item;
        const bool scale_lam = m.scale_lam || m.scale_lam_sideinfo;
        const real_t lam = s->lam6[isC ? 4 : 5] / w;                                               // collective.c:8367, :8418
        const real_t diag = scale_lam ? lam * (real_t)rows_u : lam;                                // common.c:2832
        HIP_CHECK(hipMemcpyAsync(s->gram.ptr, s->side_part.ptr, (size_t)kc * kc * sizeof(real_t), hipMemcpyDeviceToDevice, dev.stream));
        hipLaunchKernelGGL(add_diag_kernel<real_t>, dim3((kc + 255) / 256), dim3(256), 0, dev.stream, s->gram.ptr, kc, 0, kc, diag);
        HIP_CHECK(hipMemcpyAsync(Cm, s->side_part.ptr + (size_t)kc * kc, (size_t)p * kc * sizeof(real_t), hipMemcpyDeviceToDevice, dev.stream));
        struct Scope {                                            // nonneg_C / nonneg_D, L1 on C / D as in cmfrec_hip_session_update
            const DeviceInfo &d;
            Scope(const DeviceInfo &d_, bool nn, int steps, real_t l1, real_t sc) : d(d_) { d.nonneg_now = nn; d.max_cd_steps = steps; d.l1_now = l1; d.l1_last_now = l1; d.l1_scale = sc; }
            ~Scope() { d.nonneg_now = false; d.l1_now = 0; d.l1_last_now = 0; d.l1_scale = 1; }
        } scope(dev, isC ? s->nonneg_C : s->nonneg_D, s->max_cd_steps, s->l16[isC ? 4 : 5] / w, scale_lam ? (real_t)rows_u : (real_t)1);
        CholCall c{Cm, (size_t)kc, nullptr, 0, kc, 0, nullptr, s->gram.ptr, 0, 0, 0, 0, 0, false, false, false, CHOL_PREFILLED};
        return launch_chol(dev, c, nullptr, p);                                                    // common.c:2872-2875
    });
}

int cmfrec_hip_session_set_nonneg(cmfrec_hip_session *s, int nonneg, int nonneg_C, int nonneg_D, int max_cd_steps)
{
    s->nonneg = nonneg != 0; s->nonneg_C = nonneg_C != 0; s->nonneg_D = nonneg_D != 0;
    s->max_cd_steps = max_cd_steps;
    return 0;
}

int cmfrec_hip_session_set_implicit_features(cmfrec_hip_session *s, real_t w_implicit, const real_t *Ai, const real_t *Bi)
{
    return guarded([&]() {
        const cmfrec_hip_model &m = s->mdl;
        HIP_CHECK(hipSetDevice(s->dev.device));
        if (m.implicit) { g_last_error = "cmfrec_hip: add_implicit_features belongs to the explicit-feedback model"; return 2; }
        if (m.row_begin != 0 || m.row_end != m.m || m.col_begin != 0 || m.col_end != m.n || !s->XrParts.empty()) {
            g_last_error = "cmfrec_hip: add_implicit_features: sharded sessions are not built";
            return 2;
        }
        if ((m.m_x > 0 && m.m_x < m.m) || (m.n_x > 0 && m.n_x < m.n)) {
            g_last_error = "cmfrec_hip: add_implicit_features: side information must not cover rows / columns beyond X";
            return 2;
        }
        if (s->Xr.p.ptr == nullptr || s->Xc.p.ptr == nullptr) {
            g_last_error = "cmfrec_hip: add_implicit_features: set X first";
            return 2;
        }
        if (!(w_implicit > 0)) { g_last_error = "cmfrec_hip: w_implicit must be positive"; return 2; }
        const int kk = m.k + m.k_main;
        const int ktmax = std::max(s->k_totA, s->k_totB) + 1;
        s->Ai.alloc((size_t)m.m * kk); s->Bi.alloc((size_t)m.n * kk);
        s->bitbi.alloc((size_t)kk * kk); s->bitbi_full.alloc((size_t)ktmax * ktmax);
        const size_t nnz = s->Xr.nnz;
        s->ones.alloc(std::max<size_t>(nnz, 1));
        std::vector<real_t> one(std::max<size_t>(nnz, 1), (real_t)1);
        HIP_CHECK(hipMemcpyAsync(s->ones.ptr, one.data(), one.size() * sizeof(real_t), hipMemcpyHostToDevice, s->dev.stream));
        if (Ai) HIP_CHECK(hipMemcpyAsync(s->Ai.ptr, Ai, (size_t)m.m * kk * sizeof(real_t), hipMemcpyHostToDevice, s->dev.stream));
        else HIP_CHECK(hipMemsetAsync(s->Ai.ptr, 0, (size_t)m.m * kk * sizeof(real_t), s->dev.stream));
        if (Bi) HIP_CHECK(hipMemcpyAsync(s->Bi.ptr, Bi, (size_t)m.n * kk * sizeof(real_t), hipMemcpyHostToDevice, s->dev.stream));
        else HIP_CHECK(hipMemsetAsync(s->Bi.ptr, 0, (size_t)m.n * kk * sizeof(real_t), s->dev.stream));
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        // segments of up to GSUM_SEG entries per row, in row order
        size_t max_seg = 0;
        for (int o = 0; o < 2; o++) {
            const SparseShard &X = o == 0 ? s->Xr : s->Xc;
            std::vector<size_t> hp((size_t)X.nrows + 1);
            X.p.download(hp.data(), hp.size(), s->dev.stream);
            HIP_CHECK(hipStreamSynchronize(s->dev.stream));
            std::vector<int> srow, soff, rfirst((size_t)X.nrows + 1, 0);
            for (int r = 0; r < X.nrows; r++) {
                rfirst[r] = (int)srow.size();
                for (size_t off = 0; off < hp[r + 1] - hp[r]; off += GSUM_SEG) { srow.push_back(r); soff.push_back((int)off); }
            }
            rfirst[X.nrows] = (int)srow.size();
            auto &G = s->gsegs[o];
            G.nseg = (int)srow.size();
            G.seg_row.upload(srow.data(), std::max<size_t>(srow.size(), 1), s->dev.stream);
            G.seg_off.upload(soff.data(), std::max<size_t>(soff.size(), 1), s->dev.stream);
            G.row_first.upload(rfirst.data(), rfirst.size(), s->dev.stream);
            HIP_CHECK(hipStreamSynchronize(s->dev.stream));
            max_seg = std::max(max_seg, srow.size());
        }
        s->gpartial.alloc(std::max<size_t>(max_seg, 1) * kk);
        s->grhs.alloc((size_t)std::max(m.m, m.n) * kk);
        s->w_implicit = w_implicit;
        s->implicit_feats = true;
        return 0;
    });
}

int cmfrec_hip_session_get_implicit_features(cmfrec_hip_session *s, real_t *Ai, real_t *Bi)
{
    return guarded([&]() {
        const cmfrec_hip_model &m = s->mdl;
        if (!s->implicit_feats) { g_last_error = "cmfrec_hip: the session has no implicit features"; return 2; }
        HIP_CHECK(hipSetDevice(s->dev.device));
        const int kk = m.k + m.k_main;
        if (Ai) HIP_CHECK(hipMemcpyAsync(Ai, s->Ai.ptr, (size_t)m.m * kk * sizeof(real_t), hipMemcpyDeviceToHost, s->dev.stream));
        if (Bi) HIP_CHECK(hipMemcpyAsync(Bi, s->Bi.ptr, (size_t)m.n * kk * sizeof(real_t), hipMemcpyDeviceToHost, s->dev.stream));
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        return 0;
    });
}

int cmfrec_hip_session_set_NA_as_zero_X(cmfrec_hip_session *s, int on, int center, real_t glob_mean)
{
    return guarded([&]() {
        if (on && s->mdl.implicit) { g_last_error = "cmfrec_hip_session_set_NA_as_zero_X: explicit model only"; return 2; }
        // the mean enters through the right-hand-side constant: an X that was uploaded centred would count it twice; the weighted
        // and the sharded forms are not built (the updates would refuse them one by one)
        if (on && (s->x_subtract != (real_t)0 || s->mdl.row_begin != 0 || s->mdl.row_end != s->mdl.m ||
                   s->mdl.col_begin != 0 || s->mdl.col_end != s->mdl.n)) {
            g_last_error = "cmfrec_hip_session_set_NA_as_zero_X: X must have been set uncentred (subtract = 0) on the whole row and "
                           "column range";
            return 2;
        }
        s->naz_X = on != 0; s->naz_center = center != 0; s->naz_mean = glob_mean;
        refresh_naz_multipliers(s);
        return 0;
    });
}

int cmfrec_hip_session_set_zero_rows(cmfrec_hip_session *s, int which, const int_t *rows, int count)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        if (which != 'A' && which != 'B') { g_last_error = "cmfrec_hip_session_set_zero_rows: which must be 'A' or 'B'"; return 2; }
        const int limit = which == 'A' ? s->mdl.m : s->mdl.n;
        for (int e = 0; e < count; e++)
            if (rows == nullptr || rows[e] < 0 || rows[e] >= limit) { g_last_error = "cmfrec_hip_session_set_zero_rows: row out of range"; return 2; }
        DevBuf<int> &buf = which == 'A' ? s->zrowsA : s->zrowsB;
        (which == 'A' ? s->n_zrowsA : s->n_zrowsB) = std::max(count, 0);
        if (count > 0) {
            std::vector<int> h(rows, rows + count);
            buf.alloc_at_least((size_t)count);
            HIP_CHECK(hipMemcpyAsync(buf.ptr, h.data(), (size_t)count * sizeof(int), hipMemcpyHostToDevice, s->dev.stream));
            HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        }
        return 0;
    });
}

int cmfrec_hip_session_set_closed_form_rows(cmfrec_hip_session *s, int which, const unsigned char *mask)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        if (which == 'C' || which == 'D') {
            // attributes of DENSE side information with NaN, which the session holds as the sparse matrix of its present values: what
            // the reference's dense C / D update does per attribute inside a CG update (0: CG as asked for, 1: closed form, 2: CG from
            // zero with k_side + k steps; fit.hip, DenseNanSide::rules)
            const bool isC = which == 'C';
            const size_t rows = (size_t)(isC ? s->mdl.p : s->mdl.q);
            bool *any = isC ? s->cfC_any : s->cfD_any;
            any[0] = any[1] = any[2] = false;
            if (mask == nullptr) return 0;
            if (!(isC ? s->sparseU : s->sparseI)) { g_last_error = "cmfrec_hip_session_set_closed_form_rows: 'C' / 'D' need sparse side information on that side"; return 2; }
            for (size_t r = 0; r < rows; r++) {
                if (mask[r] > 2) { g_last_error = "cmfrec_hip_session_set_closed_form_rows: mask values 0, 1, 2"; return 2; }
                any[mask[r]] = true;
            }
            DevBuf<unsigned char> &buf = isC ? s->cfmaskC : s->cfmaskD;
            buf.alloc_at_least(rows);
            HIP_CHECK(hipMemcpyAsync(buf.ptr, mask, rows, hipMemcpyHostToDevice, s->dev.stream));
            HIP_CHECK(hipStreamSynchronize(s->dev.stream));
            return 0;
        }
        if (which != 'A' && which != 'B') { g_last_error = "cmfrec_hip_session_set_closed_form_rows: which must be 'A', 'B', 'C' or 'D'"; return 2; }
        const size_t rows = (size_t)(which == 'A' ? s->mdl.m : s->mdl.n);
        (which == 'A' ? s->has_cfA : s->has_cfB) = (mask != nullptr);
        if (mask != nullptr) {
            DevBuf<unsigned char> &buf = which == 'A' ? s->cfmaskA : s->cfmaskB;
            buf.alloc_at_least(rows);
            HIP_CHECK(hipMemcpyAsync(buf.ptr, mask, rows, hipMemcpyHostToDevice, s->dev.stream));
            HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        }
        return 0;
    });
}

int cmfrec_hip_session_set_lambda_multipliers(cmfrec_hip_session *s, int which, const real_t *mult)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        if (mult != nullptr && (which == 'C' || which == 'D')) {
            // attributes of dense side information with NaN under scale_lam (DenseNanSide::rules): unit weights on the attribute-major
            // shard of the present values (a multiplication by one: the unweighted numbers bit for bit) carry the multipliers
            SparseShard &Us = which == 'C' ? s->Usc : s->Isc;
            if (!(which == 'C' ? s->sparseU : s->sparseI) || Us.nnz == 0) {
                g_last_error = "cmfrec_hip_session_set_lambda_multipliers: 'C' / 'D' need sparse side information on that side";
                return 2;
            }
            Us.w.alloc_at_least(Us.nnz);
            hipLaunchKernelGGL(fill_kernel<real_t>, grid1d(Us.nnz), dim3(256), 0, s->dev.stream, Us.w.ptr, Us.nnz, (real_t)1);
            HIP_CHECK(hipGetLastError());
            Us.wsum.upload(mult, (size_t)Us.nrows, s->dev.stream);
            HIP_CHECK(hipStreamSynchronize(s->dev.stream));
            return 0;
        }
        if ((which != 'A' && which != 'B') || mult == nullptr) { g_last_error = "cmfrec_hip_session_set_lambda_multipliers: which must be 'A', 'B', 'C' or 'D', mult non-null"; return 2; }
        SparseShard &X = which == 'A' ? s->Xr : s->Xc;
        if (!X.weighted() || s->mdl.implicit) {
            g_last_error = "cmfrec_hip_session_set_lambda_multipliers: the explicit model with observation weights on X (unit weights will do)";
            return 2;
        }
        X.wsum.upload(mult, (size_t)X.nrows, s->dev.stream);
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        return 0;
    });
}

int cmfrec_hip_session_set_scale_bias_const(cmfrec_hip_session *s, int on)
{
    s->scale_bias_const = on != 0;
    return 0;
}

int cmfrec_hip_session_set_lam_unique(cmfrec_hip_session *s, const real_t *lam_unique, const real_t *l1_lam_unique, int max_cd_steps)
{
    if (lam_unique) for (int e = 0; e < 6; e++) s->lam6[e] = lam_unique[e];
    if (l1_lam_unique) {
        for (int e = 0; e < 6; e++) s->l16[e] = l1_lam_unique[e];
        s->max_cd_steps = max_cd_steps;
    }
    return 0;
}

int cmfrec_hip_session_set_l1(cmfrec_hip_session *s, real_t l1_lam, int max_cd_steps)
{
    s->l1_lam = l1_lam;
    for (int e = 0; e < 6; e++) s->l16[e] = l1_lam;
    s->max_cd_steps = max_cd_steps;
    return 0;
}

int cmfrec_hip_session_set_sideinfo_sparse(cmfrec_hip_session *s, int which, const int_t *row, const int_t *col,
                                           const real_t *val, size_t nnz)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const cmfrec_hip_model &m = s->mdl;
        const bool isU = (which == 'U');
        const int rows = isU ? m.m_u : m.n_i, cols = isU ? m.p : m.q;
        if ((which != 'U' && which != 'I') || rows <= 0 || cols <= 0 || nnz == 0) {
            g_last_error = "cmfrec_hip_session_set_sideinfo_sparse: needs 'U' / 'I', the model's m_u, p / n_i, q and entries";
            return 2;
        }
        if (rows > (isU ? (m.m_x > 0 ? m.m_x : m.m) : (m.n_x > 0 ? m.n_x : m.n)) || m.row_begin != 0 || m.row_end != m.m ||
            m.col_begin != 0 || m.col_end != m.n) {
            g_last_error = "cmfrec_hip: sparse side information: rows beyond X and sharded sessions are not supported";
            return 2;
        }
        DevBuf<int> dr, dc; DevBuf<real_t> dv;
        dr.upload(row, nnz, s->dev.stream); dc.upload(col, nnz, s->dev.stream); dv.upload(val, nnz, s->dev.stream);
        // CSR over ALL rows of the factor matrix (rows beyond m_u / n_i are empty), CSC over the attributes
        shard_from_coo(isU ? s->Usr : s->Isr, isU ? m.m : m.n, cols, dr.ptr, dc.ptr, dv.ptr, nnz, (real_t)0, (real_t)1, s->dev.stream);
        shard_from_coo(isU ? s->Usc : s->Isc, cols, rows, dc.ptr, dr.ptr, dv.ptr, nnz, (real_t)0, (real_t)1, s->dev.stream);
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        (isU ? s->sparseU : s->sparseI) = true;
        (isU ? s->zerosU : s->zerosI).clear();          // (the shards just rebuilt were that form's)
        return 0;
    });
}

// Sparse side information whose ABSENT ENTRIES ARE ZEROS (NA_as_zero_U / _I) on every row of the factor matrix: the session keeps
// the triplets in both orientations and the column means, and every product with the dense centred matrix U - 1 colmeans^T --
// right-hand sides, block CG, low-rank rows, the C / D update -- is taken on them (side_times / side_transposed_times,
// side_zeros_kernels.hpp).  The solvers downstream see the same operands as with cmfrec_hip_session_set_sideinfo on the
// zero-filled centred matrix.  Whole-matrix sessions with m_u = m (n_i = n); row-block shards keep to the dense matrix.
int cmfrec_hip_session_set_sideinfo_sparse_zeros(cmfrec_hip_session *s, int which, const int_t *row, const int_t *col,
                                                 const real_t *val, size_t nnz, const real_t *colmeans)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const cmfrec_hip_model &m = s->mdl;
        const bool isU = (which == 'U');
        const int rows = isU ? m.m_u : m.n_i, cols = isU ? m.p : m.q;
        if ((which != 'U' && which != 'I') || rows <= 0 || cols <= 0 || nnz == 0 || !row || !col || !val) {
            g_last_error = "cmfrec_hip_session_set_sideinfo_sparse_zeros: needs 'U' / 'I', the model's m_u, p / n_i, q and entries";
            return 2;
        }
        if (m.row_begin != 0 || m.row_end != m.m || m.col_begin != 0 || m.col_end != m.n || s->side_local || !s->XrParts.empty()) {
            g_last_error = "cmfrec_hip_session_set_sideinfo_sparse_zeros: row-block shards (local side information, parts of A, partial "
                           "C / D sums) need the dense matrix: cmfrec_hip_session_set_sideinfo_local";
            return 2;
        }
        if (rows != (isU ? m.m : m.n)) {
            g_last_error = "cmfrec_hip_session_set_sideinfo_sparse_zeros: the side information must cover every row of the factor matrix "
                           "(m_u = m / n_i = n): rows without entries are rows of zeros";
            return 2;
        }
        if (cols > 0 && (isU ? m.k_user : m.k_item) + m.k > SZ_MAX_WIDTH) {
            g_last_error = "cmfrec_hip_session_set_sideinfo_sparse_zeros: at most 320 factors shared with the side information";
            return 2;
        }
        for (size_t e = 0; e < nnz; e++)
            if (row[e] < 0 || row[e] >= rows || col[e] < 0 || col[e] >= cols) {
                g_last_error = "cmfrec_hip_session_set_sideinfo_sparse_zeros: index out of range";
                return 2;
            }
        DevBuf<int> dr, dc; DevBuf<real_t> dv;
        dr.upload(row, nnz, s->dev.stream); dc.upload(col, nnz, s->dev.stream); dv.upload(val, nnz, s->dev.stream);
        SparseShard &by_row = isU ? s->Usr : s->Isr, &by_col = isU ? s->Usc : s->Isc;
        shard_from_coo(by_row, rows, cols, dr.ptr, dc.ptr, dv.ptr, nnz, (real_t)0, (real_t)1, s->dev.stream);
        shard_from_coo(by_col, cols, rows, dc.ptr, dr.ptr, dv.ptr, nnz, (real_t)0, (real_t)1, s->dev.stream);
        (isU ? s->zerosU : s->zerosI).build(&by_row, &by_col, colmeans, s->dev.stream);
        (isU ? s->sparseU : s->sparseI) = false;
        (isU ? s->U : s->II).release();
        (isU ? s->eigA : s->eigB).fresh = false;
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        return 0;
    });
}

// The two products of that form alone, host buffers in and out (what the session's helpers launch, for callers who want the
// products and for the tests): U~ = U_sparse - 1 colmeans^T over `rows` rows and p attributes,
//     UM  [count, kc] = alpha (U~ M)[first : first + count, :]      when M [p, kc] is given
//     UtF [p, kc]     = U~^T F[:, :kc]                               when F [rows, ldF] is given
int cmfrec_hip_side_zeros_products(int_t rows, int_t p, int_t kc, const int_t *row, const int_t *col, const real_t *val, size_t nnz,
                                   const real_t *colmeans, const real_t *M, real_t alpha, int_t first, int_t count, real_t *UM,
                                   const real_t *F, size_t ldF, real_t *UtF)
{
    return guarded([&]() {
        if (rows <= 0 || p <= 0 || kc <= 0 || kc > SZ_MAX_WIDTH || nnz == 0 || !row || !col || !val || (M != nullptr && UM == nullptr) ||
            (F != nullptr && (UtF == nullptr || ldF < (size_t)kc)) || (M != nullptr && (first < 0 || count < 0 || first > rows - count))) {
            g_last_error = "cmfrec_hip_side_zeros_products: invalid sizes (kc <= 320, rows first .. first + count inside the matrix, ldF >= kc)";
            return 2;
        }
        for (size_t e = 0; e < nnz; e++)
            if (row[e] < 0 || row[e] >= rows || col[e] < 0 || col[e] >= p) {
                g_last_error = "cmfrec_hip_side_zeros_products: index out of range";
                return 2;
            }
        DeviceInfo dev;
        init_device(dev, -1);
        hipStream_t st = dev.stream;
        DevBuf<int> dr, dc; DevBuf<real_t> dv;
        dr.upload(row, nnz, st); dc.upload(col, nnz, st); dv.upload(val, nnz, st);
        SparseShard by_row, by_col;
        SideZeros Z;
        shard_from_coo(by_row, rows, p, dr.ptr, dc.ptr, dv.ptr, nnz, (real_t)0, (real_t)1, st);
        shard_from_coo(by_col, p, rows, dc.ptr, dr.ptr, dv.ptr, nnz, (real_t)0, (real_t)1, st);
        Z.build(&by_row, &by_col, colmeans, st);
        SideOperand u;
        u.zeros = &Z;
        if (M != nullptr && count > 0) {
            DevBuf<real_t> dM, dO;
            dM.upload(M, (size_t)p * kc, st);
            dO.alloc((size_t)count * kc);
            side_times(dev, u.from_row(first, p), count, kc, p, alpha, dM.ptr, dO.ptr, (size_t)kc);
            dO.download(UM, (size_t)count * kc, st);
            HIP_CHECK(hipStreamSynchronize(st));
        }
        if (F != nullptr) {
            DevBuf<real_t> dF, dO;
            dF.upload(F, (size_t)rows * ldF, st);
            dO.alloc((size_t)p * kc);
            side_transposed_times(dev, u, rows, kc, p, dF.ptr, ldF, dO.ptr, (size_t)kc);
            dO.download(UtF, (size_t)p * kc, st);
            HIP_CHECK(hipStreamSynchronize(st));
        }
        return 0;
    });
}

// ---- one half-step of the ALS loop on the local block -------------------------------------
// What a half-step reads of the session by side, picked once: "self" = the matrix being updated (A when isA, B otherwise; its side
// information U, C), "opp" = the fixed one.  The drivers below take their side-dependent values from here and pick none themselves.
struct HalfStepSide {
    const bool isA;
    real_t *const self, *const opp;
    const size_t ld_self, ld_opp;
    const int k_side_self, k_side_opp;          // k_user / k_item
    const int k_tot_opp;                        // columns of opp in front of its bias column
    const real_t *const oppx;                   // opp + k_side_opp: the columns X refers to
    const int p_self;                           // attributes of this side's side information
    const int rows_self, rows_opp;              // rows of the two matrices (m / n)
    const int rows_x_self, rows_x_opp;          // ... that X has (m_x / n_x where set): update_factor's Gramian and block systems
    const int rows_u, begin;                    // rows with side information; first row of the local block
    const SparseShard &X, &Us;                  // X by rows of self; sparse side information by rows of self
    const real_t *const Cm;                     // C / D
    const SideOperand Um, Um_blk;               // U / I (dense, or sparse with zeros); ... from the local block's first row
    const real_t w;                             // w_user / w_item
    const bool sparse_side;
    const bool self_bias, opp_bias;
    const real_t *const bias;                   // the opposing biases when that side has them (fused "X - bias", :8566-8570, :8750-8754)
    // lam_unique[2] / [3] for A / B; the bias, when fitted, takes lam_unique[0] / [1] (collective.c:8649-8654, :8820-8825); the
    // implicit model fits none
    const real_t lam_self, lam_last_self;
    const int kk, ks, kc, kt;                   // k + k_main; + the bias; k_side + k (the columns C has); k_side + ks
    // NA_as_zero_X: the constant of the opposing biases and the mean exists; the mean when X is centred, else zero
    const bool has_cst;
    const real_t mean;
    const real_t *const Fi;                     // the opposing side's implicit factors [rows_opp, kk], nullptr without implicit features
    cmfrec_hip_session::GatherSegs &G;          // segments of the gather-sum over X
    real_t *const uc;                           // U C of the block CG
    BinTimers *const bins;
    EigCache *const eig_mine, *const eig_next;  // eigenvectors of this side's w C^T C, and of the side whose half-step comes next ...
    const real_t *const Cm_next;                // ... with what its prefetch reads of that side: D / C, q / p, k_item / k_user + k, w
    const int p_next, kc_next;
    const real_t w_next;
    const bool sparse_side_next;

    HalfStepSide(cmfrec_hip_session *s, bool isA_)
        : isA(isA_), self(isA ? s->A.ptr : s->B.ptr), opp(isA ? s->B.ptr : s->A.ptr), ld_self(isA ? s->ldA : s->ldB),
          ld_opp(isA ? s->ldB : s->ldA), k_side_self(isA ? s->mdl.k_user : s->mdl.k_item),
          k_side_opp(isA ? s->mdl.k_item : s->mdl.k_user), k_tot_opp(isA ? s->k_totB : s->k_totA), oppx(opp + k_side_opp),
          p_self(isA ? s->mdl.p : s->mdl.q), rows_self(isA ? s->mdl.m : s->mdl.n), rows_opp(isA ? s->mdl.n : s->mdl.m),
          rows_x_self(isA ? (s->mdl.m_x > 0 ? s->mdl.m_x : s->mdl.m) : (s->mdl.n_x > 0 ? s->mdl.n_x : s->mdl.n)),
          rows_x_opp(isA ? (s->mdl.n_x > 0 ? s->mdl.n_x : s->mdl.n) : (s->mdl.m_x > 0 ? s->mdl.m_x : s->mdl.m)),
          rows_u(isA ? s->mdl.m_u : s->mdl.n_i), begin(isA ? s->mdl.row_begin : s->mdl.col_begin), X(isA ? s->Xr : s->Xc),
          Us(isA ? s->Usr : s->Isr), Cm(isA ? s->C.ptr : s->D.ptr), Um(s->side_operand(isA)),
          Um_blk(Um.from_row(s->side_local ? 0 : begin, p_self)), w(isA ? s->mdl.w_user : s->mdl.w_item),
          sparse_side(isA ? s->sparseU : s->sparseI), self_bias(isA ? s->mdl.user_bias : s->mdl.item_bias),
          opp_bias(isA ? s->mdl.item_bias : s->mdl.user_bias), bias(opp_bias ? (isA ? s->biasB.ptr : s->biasA.ptr) : nullptr),
          lam_self(s->lam6[isA ? 2 : 3]), lam_last_self((!s->mdl.implicit && self_bias) ? s->lam6[isA ? 0 : 1] : lam_self),
          kk(s->mdl.k + s->mdl.k_main), ks(kk + (self_bias ? 1 : 0)), kc(k_side_self + s->mdl.k), kt(k_side_self + ks),
          has_cst(opp_bias || s->naz_center), mean(s->naz_center ? s->naz_mean : (real_t)0),
          Fi(s->implicit_feats ? (isA ? s->Bi.ptr : s->Ai.ptr) : nullptr), G(s->gsegs[isA ? 0 : 1]),
          uc(isA ? s->ucA.ptr : s->ucB.ptr), bins(isA ? &s->binA : &s->binB), eig_mine(isA ? &s->eigA : &s->eigB),
          eig_next(isA ? &s->eigB : &s->eigA), Cm_next(isA ? s->D.ptr : s->C.ptr), p_next(isA ? s->mdl.q : s->mdl.p),
          kc_next(k_side_opp + s->mdl.k), w_next(isA ? s->mdl.w_item : s->mdl.w_user),
          sparse_side_next(isA ? s->sparseI : s->sparseU)
    {
    }
};

// Explicit model: rows that exist only in the side information (beyond the shape of X) are fitted to it alone,
//   a[:kc] = (C^T C + (lam / w) (p if scale_lam) I)^-1 C^T u     (optimizeA Case 1 on U[m_x:], collective.c:4967-5101)
// their remaining unknowns are zero under Cholesky (A was zeroed) and left alone under CG.
static int solve_sideinfo_only_rows(cmfrec_hip_session *s, const HalfStepSide &v, bool chol, int first, int count)
{
    if (count <= 0) return 0;
    const cmfrec_hip_model &m = s->mdl;
    const DeviceInfo &dev = s->dev;
    const int p_self = v.p_self, kc = v.kc;
    const bool scale_lam = m.scale_lam || m.scale_lam_sideinfo;                                    // :7465
    real_t *rows = v.self + (size_t)(v.begin + first) * v.ld_self;
    if (chol) HIP_CHECK(hipMemsetAsync(rows, 0, (size_t)count * v.ld_self * sizeof(real_t), dev.stream));
    launch_gram(dev, s->gws, v.Cm, (size_t)kc, p_self, kc, s->betbe.ptr, (real_t)1,
                (v.lam_self / v.w) * (real_t)(scale_lam ? p_self : 1));                                           // common.c:2824-2832
    side_times(dev, v.Um_blk.from_row(first, p_self), count, kc, p_self, (real_t)1, v.Cm, rows, v.ld_self);   // common.c:2847-2855
    CholCall c{rows, v.ld_self, nullptr, 0, kc, 0, nullptr, s->betbe.ptr, 0, 0, 0, 0, 0, false, false, false, CHOL_PREFILLED};
    return launch_chol(dev, c, nullptr, count);                                                    // common.c:2872-2875
}

// sum of the rows of F (leading dimension ldf; Bi / Ai, or the factors themselves) at every row's observed positions, by the
// two-stage segmented gather-sum; result in dst [rows, kk].  Returns false when the tables / widths do not allow it (the caller
// then gathers inside the row kernel).
static bool launch_gsum(cmfrec_hip_session *s, const HalfStepSide &v, const real_t *F, size_t ldf, int kk, real_t *dst, int rows)
{
    if (kk > 64 * GSUM_MAXC || dst == nullptr) return false;
    hipStream_t st = s->dev.stream;
    if (v.G.nseg > 0)
        hipLaunchKernelGGL(gather_sum_segments_kernel<real_t>, dim3((v.G.nseg + 3) / 4), dim3(256), 0, st, v.X.p.ptr, v.X.i.ptr, F, ldf, kk,
                           v.G.seg_row.ptr, v.G.seg_off.ptr, v.G.nseg, s->gpartial.ptr);
    hipLaunchKernelGGL(gather_sum_rows_kernel<real_t>, dim3((rows + 3) / 4), dim3(256), 0, st, s->gpartial.ptr, v.G.row_first.ptr, rows, kk,
                       dst, (size_t)kk);
    HIP_CHECK(hipGetLastError());
    return true;
}

// ---- launch groups the half-steps share ----
// the opposing matrix' bias column is fixed to 1 while this one's bias is fitted (collective.c:8538-8543, :8728-8732)
static void fill_fixed_bias_column(cmfrec_hip_session *s, const HalfStepSide &v)
{
    if (!v.self_bias) return;
    hipLaunchKernelGGL(col_fill_kernel<real_t>, grid1d(v.rows_opp), dim3(256), 0, s->dev.stream, v.opp, v.ld_opp, v.rows_opp, v.k_tot_opp,
                       (real_t)1);
}

// Bi^T Bi of the opposing implicit factors (rows of them) into s->bitbi [kk, kk]: times w_implicit when weighted; into_gram adds it
// onto the first k + k_main unknowns of s->gram [ks, ks] (collective.c:1704-1707)
static void launch_implicit_gram(cmfrec_hip_session *s, const HalfStepSide &v, int rows, bool weighted, bool into_gram)
{
    launch_gram(s->dev, s->gws, v.Fi, (size_t)v.kk, rows, v.kk, s->bitbi.ptr, weighted ? s->w_implicit : (real_t)1, (real_t)0);
    if (into_gram)
        hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)v.kk * v.kk), dim3(256), 0, s->dev.stream, s->bitbi.ptr, v.kk, (real_t)1,
                           s->gram.ptr, v.ks, 0);
}

// w_i times the gather-sum (s->grhs) onto the columns behind k_side of the right-hand sides (:1757-1771)
static void add_implicit_rhs(cmfrec_hip_session *s, const HalfStepSide &v, real_t *rhs, size_t ld)
{
    hipLaunchKernelGGL(add_cols_scaled_kernel<real_t>, grid1d((size_t)v.X.nrows * v.kk), dim3(256), 0, s->dev.stream, rhs, ld, v.k_side_self,
                       s->grhs.ptr, v.kk, s->w_implicit, (size_t)v.X.nrows);
}

// the implicit-features term of the lane <-> unknown CG kernel (it gathers Bi_j at the row's entries itself unless c.gsum is set)
static void set_implicit_term(const cmfrec_hip_session *s, const HalfStepSide &v, CgCall &c)
{
    c.Bi = v.Fi; c.BiTBi = s->bitbi.ptr; c.ki = v.kk; c.w_imp = s->w_implicit;
}

// sparse side information: the row's attributes as the second gather source of the launch
static void set_sparse_side(const HalfStepSide &v, CholCall &c)
{
    c.X2 = &v.Us; c.B2 = v.Cm; c.ldb2 = (size_t)v.kc; c.kc2 = v.kc; c.w2 = v.w;
}
static void set_sparse_side(const HalfStepSide &v, CgCall &c)
{
    c.X2 = &v.Us; c.C2 = v.Cm;
}

// ---- ... and the ones of the main matrix missing-as-zero ----
static int naz_check_side_rows(int rows_u, int rows_self)
{
    if (rows_u == rows_self) return 0;
    g_last_error = "cmfrec_hip: NA_as_zero_X with side information: side information on exactly the rows / columns of X";
    return 2;
}

// sum of the opposing implicit factors at the row's observed positions into s->grhs
static int naz_implicit_gsum(cmfrec_hip_session *s, const HalfStepSide &v)
{
    if (launch_gsum(s, v, v.Fi, (size_t)v.kk, v.kk, s->grhs.ptr, v.X.nrows)) return 0;
    g_last_error = "cmfrec_hip: NA_as_zero_X with implicit features: k + k_main too wide for the gather-sum";
    return 2;
}

// cst = - sum over ALL opposing rows of (bias + mean) x row into s->naz_vec [ks] (:3152-3157 / :5815-5821), added onto every row of
// add_to [rows_self, ks] when that is given.  nullptr when there is neither an opposing bias nor centring.
static const real_t *naz_constant(cmfrec_hip_session *s, const HalfStepSide &v, real_t *add_to = nullptr, size_t ld_add = 0)
{
    if (!v.has_cst) return nullptr;
    hipStream_t st = s->dev.stream;
    const int ks = v.ks, nb = (v.rows_opp + COLSUM_ROWS - 1) / COLSUM_ROWS;
    s->naz_part.alloc_at_least((size_t)nb * ks); s->naz_vec.alloc_at_least((size_t)ks);
    hipLaunchKernelGGL(weighted_colsum_partial_kernel<real_t>, dim3(nb), dim3(256), 0, st, v.oppx, v.ld_opp, v.rows_opp, ks, v.bias, v.mean,
                       s->naz_part.ptr);
    hipLaunchKernelGGL(colsum_finish_kernel<real_t>, grid1d(ks), dim3(256), 0, st, s->naz_part.ptr, nb, ks, (real_t)-1, s->naz_vec.ptr);
    if (add_to != nullptr)
        hipLaunchKernelGGL(add_rowvec_kernel<real_t>, grid1d((size_t)v.rows_self * ks), dim3(256), 0, st, add_to, ld_add, (size_t)v.rows_self, ks,
                           s->naz_vec.ptr);
    return s->naz_vec.ptr;
}

// sum_j x_j opp_j over every row's entries by the gather-only launch of the row Cholesky kernel (tgemm_sp_dense, :3145-3151 /
// :5753-5762), x_j from values_override when given, added into dst, which the caller has zeroed
static int naz_gather_rhs_into(cmfrec_hip_session *s, const HalfStepSide &v, real_t *dst, size_t ld, const real_t *values_override = nullptr)
{
    CholCall c{dst, ld, v.oppx, v.ld_opp, v.ks, 0, nullptr, s->gram.ptr, 0, 0, 0, v.lam_self, v.lam_last_self, false, false, false, CHOL_NAZ};
    c.rhs_only = true; c.values_override = values_override;
    return launch_chol(s->dev, c, &v.X);
}

// ... into s->naz_rhs [rows_self, ks], grown and zeroed here
static int naz_gather_rhs(cmfrec_hip_session *s, const HalfStepSide &v, const real_t *values_override = nullptr)
{
    s->naz_rhs.alloc_at_least((size_t)v.rows_self * v.ks);
    HIP_CHECK(hipMemsetAsync(s->naz_rhs.ptr, 0, (size_t)v.rows_self * v.ks * sizeof(real_t), s->dev.stream));
    return naz_gather_rhs_into(s, v, s->naz_rhs.ptr, (size_t)v.ks, values_override);
}

// a zero array of at least nnz entries, in the place of the values for the CG kernels
static const real_t *naz_zeros(cmfrec_hip_session *s, size_t nnz)
{
    nnz = std::max<size_t>(nnz, 1);
    if (s->naz_zero.n < nnz) {
        s->naz_zero.alloc(nnz);
        HIP_CHECK(hipMemsetAsync(s->naz_zero.ptr, 0, nnz * sizeof(real_t), s->dev.stream));
    }
    return s->naz_zero.ptr;
}

// observation weights: per entry w_j - 1 into s->naz_g and the right-hand-side bracket w_j x_j - (w_j - 1)(mean + bias_j) into s->naz_xt
static void naz_entry_transform(cmfrec_hip_session *s, const HalfStepSide &v)
{
    const size_t nnz = v.X.nnz;
    s->naz_g.alloc_at_least(std::max<size_t>(nnz, 1)); s->naz_xt.alloc_at_least(std::max<size_t>(nnz, 1));
    if (nnz > 0)
        hipLaunchKernelGGL(naz_entry_transform_kernel<real_t>, grid1d(nnz), dim3(256), 0, s->dev.stream, v.X.v.ptr, v.X.w.ptr, v.X.i.ptr, nnz,
                           v.bias, v.mean, s->naz_g.ptr, s->naz_xt.ptr);
}

// NA_as_zero_X on a side with SPARSE side information (missing = absent; round 5): no matrix is shared by the rows any more -- each
// adds the rank-1 terms of its own attributes -- so the reference solves row by row (collective_closed_form_block's general
// branch with prefer_BtB, collective.c:1534-1846):
//     M_i   = blockdiag(0, B^T B) + w sum_u c_u c_u^T + lam mult_i I,   mult_i = n (+ the row's attributes under scale_lam_sideinfo)
//     rhs_i = [w sum_u u_iu c_u ; sum_j x_j b_j + cst]
// on the two-source build of the row Cholesky kernel: B^T B embedded as the matrix every row starts from (Mfull), the entries of X
// right-hand side only, the attributes as the second gather source with their rank-1 terms, the constant prefilled.  Closed
// form only (the block CG with NA_as_zero_X, collective.c:2134-2903, is not restated).
static int update_factor_naz_sparse_side(cmfrec_hip_session *s, const HalfStepSide &v, bool chol)
{
    const cmfrec_hip_model &m = s->mdl;
    const DeviceInfo &dev = s->dev;
    hipStream_t st = dev.stream;
    if (int rc = naz_check_side_rows(v.rows_u, v.rows_self)) return rc;
    const int ks = v.ks, kt = v.kt;
    fill_fixed_bias_column(s, v);
    launch_gram(dev, s->gws, v.oppx, v.ld_opp, v.rows_opp, ks, s->gram.ptr, (real_t)1, (real_t)0);
    // implicit features (round 6, fixture g37): w_i Bi^T Bi on the first k + k_main unknowns of the X block (collective.c:1704-1707;
    // the block CG keeps it apart, unweighted: :2301-2304, :2626-2629), w_i times the sum of the opposing implicit factors at the
    // row's observed positions in the right-hand side (:1757-1771)
    if (v.Fi != nullptr) {
        launch_implicit_gram(s, v, v.rows_opp, chol, chol);
        if (chol)
            if (int rc = naz_implicit_gsum(s, v)) return rc;
    }
    // mult_i = n: every cell of the row counts
    const bool scaled = m.scale_lam || m.scale_lam_sideinfo;
    auto fill_mult = [&]() {
        if (!scaled) return;
        s->naz_mult.alloc_at_least((size_t)v.rows_self);
        hipLaunchKernelGGL(fill_kernel<real_t>, grid1d((size_t)v.rows_self), dim3(256), 0, st, s->naz_mult.ptr, (size_t)v.rows_self, (real_t)v.rows_opp);
    };
    if (!chol) {
        // Block CG (round 6; collective_block_cg with NA_as_zero_X and u_vec_sp, collective.c:2134-2903): the X block of every row's
        // system is the shared B^T B (:2430-2445 first residual, :2700-2760 the products), its right-hand side sum_j x_j b_j + cst;
        // the row's attributes gather rows of C.  On the lane <-> unknown kernel: B^T B as its shared matrix (CgParams::gx), the
        // right-hand side of the X block as the per-row constant of the first residual, the entries of X with rank-1 weight zero.
        if (int rc = naz_gather_rhs(s, v)) return rc;
        naz_constant(s, v, s->naz_rhs.ptr, (size_t)ks);
        const real_t *zeros = naz_zeros(s, v.X.nnz);
        fill_mult();
        HIP_CHECK(hipGetLastError());
        CgCall c{v.self, v.ld_self, v.oppx, v.ld_opp, ks, nullptr, nullptr, v.lam_self, v.lam_last_self, scaled, false, m.max_cg_steps, false,
                 (bool)m.precondition_cg};
        c.koff = v.k_side_self; c.kc = v.kc; c.w_side = v.w; c.rows_with_u = v.rows_u; c.p_side = v.p_self;
        c.scale_lam_sideinfo = (bool)m.scale_lam_sideinfo;
        set_sparse_side(v, c);
        c.Gx = s->gram.ptr; c.rconst_x = s->naz_rhs.ptr; c.ldr_x = (size_t)ks;
        c.values_override = zeros; c.weights_override = zeros;
        if (scaled) c.wsum_override = s->naz_mult.ptr;
        c.gx_all_rows = v.has_cst;                         // rows with neither entries nor attributes: solved from the constant, zero without it
        if (v.Fi != nullptr) set_implicit_term(s, v, c);   // (the kernel gathers Bi_j at the row's entries itself)
        return launch_cg(dev, c, v.X);
    }
    s->naz_M.alloc_at_least((size_t)kt * kt);
    hipLaunchKernelGGL(betbe_base_kernel<real_t>, grid1d((size_t)kt * kt), dim3(256), 0, st, s->gram.ptr, ks, v.k_side_self, (real_t)0, s->naz_M.ptr);
    // right-hand sides start from [0 ; cst]
    HIP_CHECK(hipMemset2DAsync(v.self, v.ld_self * sizeof(real_t), 0, (size_t)kt * sizeof(real_t), (size_t)v.rows_self, st));
    naz_constant(s, v, v.self + v.k_side_self, v.ld_self);
    if (v.Fi != nullptr) add_implicit_rhs(s, v, v.self, v.ld_self);
    fill_mult();
    HIP_CHECK(hipGetLastError());
    CholCall c{v.self, v.ld_self, v.oppx, v.ld_opp, kt, v.k_side_self, nullptr, nullptr, v.kc, v.rows_u, v.p_self, v.lam_self, v.lam_last_self,
               scaled, (bool)m.scale_lam_sideinfo, false, CHOL_COLLECTIVE, s->naz_M.ptr};
    set_sparse_side(v, c);
    c.rhs_prefilled_all = true; c.x_rhs_only = true;
    if (scaled) c.mult_override = s->naz_mult.ptr;
    return launch_chol(dev, c, &v.X);
}

// One half-step of the explicit model with the main matrix missing-as-zero (see cmfrec_hip_session::naz_X).
// Without side information on this side: optimizeA Case 3 (common.c:3116-3205).  With dense, complete side information that
// covers exactly the rows of X: optimizeA_collective with bufferBeTBeChol (collective.c:5566-5968, :5607-5617) -- every row
// shares  blockdiag(0, B^T B) + w C^T C + lam mult I  (mult = n + p | n | 1, :4787-4799, :5700-5716), right-hand sides
// X B + w U C + the bias / mean constant on the columns behind k_user (:5753-5770, :5815-5821), one factorisation (:5715) and
// the substitutions of collective_closed_form_block's first branch (:1364-1460).
static int update_factor_naz(cmfrec_hip_session *s, const HalfStepSide &v, bool chol)
{
    const cmfrec_hip_model &m = s->mdl;
    const DeviceInfo &dev = s->dev;
    hipStream_t st = dev.stream;
    const int p_self = v.p_self, rows_self = v.rows_self, rows_opp = v.rows_opp;
    if (s->scale_bias_const || dev.nonneg_now || dev.l1_now != (real_t)0 ||
        dev.l1_last_now != (real_t)0 || m.row_begin != 0 || m.row_end != m.m || m.col_begin != 0 || m.col_end != m.n ||
        s->Xr.weighted() || s->side_local) {
        g_last_error = "cmfrec_hip: NA_as_zero_X: the explicit model on one device without weights, nonneg / L1, "
                       "scale_bias_const, incomplete side information";
        return 2;
    }
    // implicit features (round 5): the model without side information -- the reference runs those half-steps through
    // optimizeA_collective's general branch (collective.c:8612 / :8783 -> :1534-1846 with prefer_BtB), which without side
    // information is ONE matrix for all rows, B^T B + w_i Bi^T Bi + lam mult I, and right-hand sides X B + w_i sum_{observed} Bi_j
    // + the constant: the shared-matrix half-step below with two more terms.  Closed form (the block CG is not restated).
    // (use_cg: the reference takes its closed-form Case 1 here whatever the solver asked for -- collective.c:5121-5130 -- and returns
    //  the same numbers bit for bit)
    // (round 6, fixture g37: with side information too -- dense: the shared block matrix takes w_i Bi^T Bi on its X block and the
    //  right-hand sides the gather-sum like below; sparse: update_factor_naz_sparse_side)
    if (p_self > 0 && v.sparse_side) return update_factor_naz_sparse_side(s, v, chol);
    // (m > m_u takes optimizeA Case 3 for the rows beyond in the reference -- its build corrupts the heap there, so nothing
    //  pins that branch)
    if (p_self > 0)
        if (int rc = naz_check_side_rows(v.rows_u, rows_self)) return rc;
    // (use_cg changes nothing here, like in Case 3: collective_closed_form_block takes the factorised block matrix before it looks
    //  at the solver, collective.c:1364-1460 -- the reference's fit with use_cg = true returns the closed-form numbers, g20)
    (void)chol;
    if (p_self == 0 && v.k_side_self != 0) {
        g_last_error = "cmfrec_hip: NA_as_zero_X: k_user / k_item without side information on that side";
        return 2;
    }
    const real_t lam_self = v.lam_self, lam_last_self = v.lam_last_self;
    const int ks = v.ks, kc = v.kc, kt = v.kt;
    fill_fixed_bias_column(s, v);
    // shared matrix: opp^T opp + diag(lam .. lam, lam_last), x rows_opp (+ p with side information on this side under
    // scale_lam_sideinfo) under scale_lam (common.c:3128-3138; collective.c:4787-4799)
    const real_t mult = (p_self > 0 && m.scale_lam_sideinfo) ? (real_t)(rows_opp + p_self)
                        : ((m.scale_lam || m.scale_lam_sideinfo) ? (real_t)rows_opp : (real_t)1);
    launch_gram(dev, s->gws, v.oppx, v.ld_opp, rows_opp, ks, s->gram.ptr, (real_t)1, lam_self * mult);
    if (lam_last_self != lam_self)
        hipLaunchKernelGGL(add_diag_kernel<real_t>, dim3(1), dim3(64), 0, st, s->gram.ptr, ks, ks - 1, ks, (lam_last_self - lam_self) * mult);
    // + w_i Bi^T Bi on the first k + k_main unknowns (:1704-1707): weighted and added whatever the solver
    if (v.Fi != nullptr) launch_implicit_gram(s, v, rows_opp, true, true);
    real_t *Msh = s->gram.ptr;                // the matrix the rows share, [kt, kt]
    if (p_self > 0) {
        launch_gram(dev, s->gws, v.Cm, (size_t)kc, p_self, kc, s->ctc.ptr, v.w, (real_t)0);        // :5658-5668
        s->naz_M.alloc_at_least((size_t)kt * kt);
        hipLaunchKernelGGL(naz_block_matrix_kernel<real_t>, grid1d((size_t)kt * kt), dim3(256), 0, st, s->gram.ptr, ks, s->ctc.ptr, kc, v.k_side_self,
                           lam_self * mult, s->naz_M.ptr);
        Msh = s->naz_M.ptr;
    }
    // right-hand sides: sum_j x_j opp_j over the row's entries (tgemm_sp_dense, :3145-3151 / :5753-5762), left by the row kernel in
    // the rows of self themselves, with side information aside in naz_rhs [rows, ks] ...
    real_t *rhs = v.self;
    const size_t ld_r = v.ld_self;
    HIP_CHECK(hipMemset2DAsync(rhs, ld_r * sizeof(real_t), 0, (size_t)kt * sizeof(real_t), (size_t)rows_self, st));
    if (int rc = p_self > 0 ? naz_gather_rhs(s, v) : naz_gather_rhs_into(s, v, rhs, ld_r)) return rc;
    if (p_self > 0) {
        // ... w U C on the first k_side + k columns, the gathered part behind k_side
        side_times(dev, v.Um, rows_self, kc, p_self, v.w, v.Cm, rhs, ld_r);
        hipLaunchKernelGGL(add_cols_scaled_kernel<real_t>, grid1d((size_t)rows_self * ks), dim3(256), 0, st, rhs, ld_r, v.k_side_self, s->naz_rhs.ptr, ks,
                           (real_t)1, (size_t)rows_self);
    }
    if (v.Fi != nullptr) {
        // ... w_i times the sum of the opposing implicit factors at the row's observed positions (:1757-1771)
        if (int rc = naz_implicit_gsum(s, v)) return rc;
        add_implicit_rhs(s, v, rhs, ld_r);
    }
    // ... plus the constant of the opposing biases and the mean (:3152-3157 / :5815-5821)
    naz_constant(s, v, rhs + v.k_side_self, ld_r);
    // one factorisation, all rows (with and without entries) through the triangular solves (:3171-3175 / :5715, :1455-1458)
    hipLaunchKernelGGL(potrf_upper_kernel<real_t>, dim3(1), dim3(256), 0, st, Msh, kt);
    HIP_CHECK(hipGetLastError());
    launch_potrs_rows(dev, rows_self, kt, Msh, v.self, v.ld_self);
    return 0;
}

// ... WITH observation weights on a side that carries DENSE side information (round 5): a row with entries leaves the shared
// factorisation (collective.c:1367-1372 wants weight == NULL || nnz == 0) for collective_closed_form_block's general branch,
//     M_i   = w C^T C (+) B^T B + sum_j (w_j - 1) b_j b_j^T + lam mult_i I,   mult_i = sum of the row's weights + absent entries (+ p)
//     rhs_i = [w U C ; sum_j (w_j x_j - (w_j - 1)(mean + bias_j)) b_j + cst]
// on the row Cholesky kernel's collective mode: w C^T C for the rows with side information (all of them), blockdiag(0, B^T B) as the
// matrix every row starts from, the entries' weight pairs as they are (entry_pairs), the right-hand sides prefilled.  Closed form.
static int update_factor_naz_weighted_side(cmfrec_hip_session *s, const HalfStepSide &v, bool chol)
{
    const cmfrec_hip_model &m = s->mdl;
    const DeviceInfo &dev = s->dev;
    hipStream_t st = dev.stream;
    // has_side == false (round 6, fixture g39): no side information on this side, but implicit features -- the reference still takes its
    // collective route (collective.c:8612, :8783), whose rows without entries are zeroed unless the bias / mean constant exists
    // (:1258-1268); every row then counts as "with side information" of zero attributes
    const int p_self = v.p_self, rows_self = v.rows_self;
    const bool has_side = p_self > 0;
    const int rows_u = has_side ? v.rows_u : rows_self;
    if (int rc = naz_check_side_rows(rows_u, rows_self)) return rc;
    // sparse side information (missing = absent; round 6, fixture g36): the row's attributes as the second gather source instead of the
    // shared w C^T C / w U C (collective.c:1636-1653 / :2292-2298 beside the weight branches)
    const bool sparse_side = has_side && v.sparse_side;
    const bool dense_side = has_side && !sparse_side;
    const int ks = v.ks, kc = has_side ? v.kc : 0, kt = v.kt;
    fill_fixed_bias_column(s, v);
    launch_gram(dev, s->gws, v.oppx, v.ld_opp, v.rows_opp, ks, s->gram.ptr, (real_t)1, (real_t)0);
    // implicit features: w_i Bi^T Bi on the first k + k_main unknowns of the X block (closed form: inside the matrix every row starts
    // from; block CG: the kernel's own product with the unweighted matrix), w_i times the gather-sum of the opposing implicit factors in
    // the right-hand sides (closed form; the CG kernel gathers them itself)
    if (v.Fi != nullptr) {
        launch_implicit_gram(s, v, v.rows_opp, chol, chol);
        if (chol)
            if (int rc = naz_implicit_gsum(s, v)) return rc;
    }
    s->naz_M.alloc_at_least((size_t)kt * kt);
    hipLaunchKernelGGL(betbe_base_kernel<real_t>, grid1d((size_t)kt * kt), dim3(256), 0, st, s->gram.ptr, ks, v.k_side_self, (real_t)0, s->naz_M.ptr);
    const bool scaled = m.scale_lam || m.scale_lam_sideinfo;
    if (!chol) {
        // Block CG (round 6; fixture g35).  The rows WITH entries: collective_block_cg with NA_as_zero_X and weights (collective.c:2446-2493
        // first residual, :2700-2760 products) -- the shared B^T B, the corrections (w_j - 1) b_j b_j^T of the row's entries, the dense
        // side-information block through C^T C and U C -- on the lane <-> unknown kernel (CgParams::gx).  The rows WITHOUT entries run
        // the same CG from their side information and the constant: the reference factorises the shared block matrix for them only
        // when the caller hands it the buffers of precompute_for_predictions (filled_BtB, :5702-5716), which this model does not offer.
        if (dense_side) {
            launch_gram(dev, s->gws, v.Cm, (size_t)kc, p_self, kc, s->ctc.ptr, (real_t)1, (real_t)0);                 // C^T C, unweighted
            side_times(dev, v.Um, rows_self, kc, p_self, (real_t)1, v.Cm, v.uc, (size_t)kc);   // U C
        }
        naz_entry_transform(s, v);
        if (int rc = naz_gather_rhs(s, v, s->naz_xt.ptr)) return rc;
        naz_constant(s, v, s->naz_rhs.ptr, (size_t)ks);
        const real_t *zeros = naz_zeros(s, v.X.nnz);
        HIP_CHECK(hipGetLastError());
        CgCall c{v.self, v.ld_self, v.oppx, v.ld_opp, ks, nullptr, nullptr, v.lam_self, v.lam_last_self, scaled, false, m.max_cg_steps, false,
                 (bool)m.precondition_cg};
        c.koff = v.k_side_self; c.kc = kc; c.w_side = v.w; c.rows_with_u = rows_u; c.p_side = p_self;
        if (sparse_side) set_sparse_side(v, c);
        else if (has_side) { c.CtC = s->ctc.ptr; c.UC = v.uc; }
        if (v.Fi != nullptr) set_implicit_term(s, v, c);
        c.scale_lam_sideinfo = (bool)m.scale_lam_sideinfo;
        c.Gx = s->gram.ptr; c.rconst_x = s->naz_rhs.ptr; c.ldr_x = (size_t)ks;
        c.values_override = zeros; c.weights_override = s->naz_g.ptr;                // (the multipliers: X.wsum_naz, launch_cg)
        c.gx_all_rows = v.has_cst;
        return launch_cg(dev, c, v.X);
    }
    if (dense_side) launch_gram(dev, s->gws, v.Cm, (size_t)kc, p_self, kc, s->ctc.ptr, v.w, (real_t)0);
    // right-hand sides start from [w U C ; cst]  (sparse side information: [0 ; cst], the attributes are gathered by the row kernel)
    HIP_CHECK(hipMemset2DAsync(v.self, v.ld_self * sizeof(real_t), 0, (size_t)kt * sizeof(real_t), (size_t)rows_self, st));
    if (dense_side) side_times(dev, v.Um, rows_self, kc, p_self, v.w, v.Cm, v.self, v.ld_self);
    if (v.Fi != nullptr) add_implicit_rhs(s, v, v.self, v.ld_self);
    naz_constant(s, v, v.self + v.k_side_self, v.ld_self);
    naz_entry_transform(s, v);
    HIP_CHECK(hipGetLastError());
    CholCall c{v.self, v.ld_self, v.oppx, v.ld_opp, kt, v.k_side_self, nullptr, dense_side ? s->ctc.ptr : nullptr, kc, rows_u, p_self, v.lam_self,
               v.lam_last_self, scaled, (bool)m.scale_lam_sideinfo, false, CHOL_COLLECTIVE, s->naz_M.ptr};
    c.rhs_prefilled_all = true; c.entry_pairs = true; c.values_override = s->naz_xt.ptr; c.weights_override = s->naz_g.ptr;
    if (sparse_side) set_sparse_side(v, c);
    if (scaled) c.mult_override = v.X.wsum_naz.ptr;      // sum of the row's weights + its absent entries (cmfrec_hip_session_set_NA_as_zero_X)
    return launch_chol(dev, c, &v.X);
}

// The same half-step WITH observation weights and without side information (optimizeA Case 4 with NA_as_zero && weight,
// common.c:3209-3302; driver collective.c:8573-8600 + :8680-8717, :8756-8787 + :8847-8876): an absent entry is a zero of weight
// one, so every row's system is the shared opp^T opp plus the correction of its present entries,
//     M_i   = opp^T opp + sum_j (w_j - 1) opp_j opp_j^T + diag(lam_i .. lam_i, lam_last_i)
//     rhs_i = sum_j [w_j x_j - (w_j - 1)(mean + bias_j)] opp_j + cst,    cst = - sum over ALL opposing rows of (bias + mean) x row
// (factors_closed_form :846-907; factors_explicit_cg_NA_as_zero_weighted :1293-1441), lam_i = lam x (sum of the row's weights +
// number of its absent entries) under scale_lam.  Closed form: the row Cholesky kernel in its CHOL_NAZ_W mode (B^T B as the
// initial matrix, the corrections on the matrix cores).  CG: the right-hand sides by the gather-only launch, then the tiled CG
// kernels of the explicit model with the shared matrix in LDS (GRAMX builds), weights w - 1 and zero values --
//     r = rhs_i - M_i a,   Ap = M_i p
// are the reference's :1321-1371 / :1391-1406 regrouped.  Rows without entries are solved when cst exists (:3270-3271).
static int update_factor_naz_weighted(cmfrec_hip_session *s, const HalfStepSide &v, bool chol)
{
    const cmfrec_hip_model &m = s->mdl;
    const DeviceInfo &dev = s->dev;
    hipStream_t st = dev.stream;
    if (dev.nonneg_now || dev.l1_now != (real_t)0 || dev.l1_last_now != (real_t)0 || s->side_local) {
        g_last_error = "cmfrec_hip: NA_as_zero_X with observation weights: the model without nonneg / L1";
        return 2;
    }
    if (v.p_self > 0 || s->implicit_feats) return update_factor_naz_weighted_side(s, v, chol);
    const int rows_self = v.rows_self, ks = v.ks;
    const real_t *opp = v.oppx;               // the columns X refers to (the other side may carry k_item / k_user)
    const SparseShard &X = v.X;
    const real_t lam_self = v.lam_self, lam_last_self = v.lam_last_self;
    if (!chol && ks > 64 && !m.precondition_cg) {
        g_last_error = "cmfrec_hip: NA_as_zero_X with observation weights under CG: at most 64 unknowns per row (the preconditioned solver takes more)";
        return 2;
    }
    fill_fixed_bias_column(s, v);
    launch_gram(dev, s->gws, opp, v.ld_opp, v.rows_opp, ks, s->gram.ptr, (real_t)1, (real_t)0);   // :3233-3236, no diagonal
    // cst (bias_BtX) and the per-entry pairs
    const bool has_cst = v.has_cst;
    const real_t *cst = naz_constant(s, v);
    naz_entry_transform(s, v);
    HIP_CHECK(hipGetLastError());
    if (chol) {
        // right-hand sides start from cst (or zero), every row that is solved is overwritten
        const int nsolve = has_cst ? X.nrows : X.n_nonempty;
        s->naz_rhs.alloc_at_least((size_t)rows_self * ks);
        hipLaunchKernelGGL(set_rowvec_kernel<real_t>, grid1d((size_t)rows_self * ks), dim3(256), 0, st, s->naz_rhs.ptr, (size_t)ks, (size_t)rows_self, ks, cst);
        // (rows without entries and without cst keep their factors: the kernel solves into naz_rhs, copied back below for the solved rows)
        CholCall c{s->naz_rhs.ptr, (size_t)ks, opp, v.ld_opp, ks, 0, nullptr, s->gram.ptr, 0, 0, 0, lam_self, lam_last_self, m.scale_lam != 0, false,
                   s->scale_bias_const, CHOL_NAZ_W};
        c.values_override = s->naz_xt.ptr; c.weights_override = s->naz_g.ptr; c.rhs_prefilled_all = true; c.all_rows = has_cst;
        int rc = launch_chol(dev, c, &X);
        if (rc) return rc;
        hipLaunchKernelGGL(copy_rows_by_order_kernel<real_t>, grid1d((size_t)nsolve * ks), dim3(256), 0, st, s->naz_rhs.ptr, (size_t)ks, v.self, v.ld_self,
                           X.order.ptr, nsolve, ks);
        HIP_CHECK(hipGetLastError());
        return 0;
    }
    // CG: rhs_i by the gather-only launch (sum_j xt_j opp_j) + cst ...
    if (int rc = naz_gather_rhs(s, v, s->naz_xt.ptr)) return rc;
    if (has_cst)
        hipLaunchKernelGGL(add_rowvec_kernel<real_t>, grid1d((size_t)rows_self * ks), dim3(256), 0, st, s->naz_rhs.ptr, (size_t)ks, (size_t)rows_self, ks, cst);
    // ... then the tiled kernels: shared matrix in LDS, rank-1 weights w - 1, values zero
    CgCall c{v.self, v.ld_self, opp, v.ld_opp, ks, nullptr, nullptr, lam_self, lam_last_self, m.scale_lam != 0, s->scale_bias_const, m.max_cg_steps, false};
    c.Gx = s->gram.ptr; c.rconst_x = s->naz_rhs.ptr; c.ldr_x = (size_t)ks;
    c.values_override = naz_zeros(s, X.nnz); c.weights_override = s->naz_g.ptr;
    // precondition_cg (round 6; factors_explicit_pcg_NA_as_zero_weighted, common.c:1443-1613): the lane <-> unknown kernel with the
    // shared matrix, its diagonal in the Jacobi preconditioner, the rows without entries in the same launch when the constant exists
    c.precond = m.precondition_cg != 0; c.gx_all_rows = c.precond && has_cst;
    int rc = launch_cg(dev, c, X);
    if (rc) return rc;
    if (!c.precond && has_cst && X.nrows > X.n_nonempty) {
        const int cnt = X.nrows - X.n_nonempty;
        hipLaunchKernelGGL(cg_shared_matrix_rows_kernel<real_t>, dim3((cnt + 3) / 4), dim3(256), 0, st, v.self, v.ld_self, X.order.ptr + X.n_nonempty, cnt, ks,
                           s->gram.ptr, cst, lam_self, lam_last_self, m.scale_lam ? X.wsum_naz.ptr : nullptr, s->scale_bias_const ? 1 : 0, m.max_cg_steps);
        HIP_CHECK(hipGetLastError());
    }
    return 0;
}

static int update_factor(cmfrec_hip_session *s, bool isA, bool chol, int part = -1)
{
    // "self" = matrix being updated, "opp" = the fixed one
    const HalfStepSide v(s, isA);
    if (s->naz_X && !s->mdl.implicit && s->Xr.weighted()) return update_factor_naz_weighted(s, v, chol);
    if (s->naz_X && !s->mdl.implicit) return update_factor_naz(s, v, chol);
    const cmfrec_hip_model &m = s->mdl;
    const DeviceInfo &dev = s->dev;
    hipStream_t st = dev.stream;
    const size_t ld_self = v.ld_self, ld_opp = v.ld_opp;
    const int rows_opp = v.rows_x_opp;        // rows of the opposing matrix that X refers to (the Gramian's rows)
    const int k_side_self = v.k_side_self, p_self = v.p_self, begin = v.begin;
    const real_t *oppx = v.oppx;
    const SparseShard &X = (part >= 0) ? *s->XrParts[part] : v.X;
    const bool sbc = s->scale_bias_const && !m.implicit;      // rows without side information: common.c:679-723
    const real_t lam_self = v.lam_self, lam_last_self = v.lam_last_self;
    real_t *self_blk = v.self + (size_t)(begin + (part >= 0 ? s->partBegin[part] : 0)) * ld_self;
    if (part >= 0 && (!isA || p_self > 0)) {
        g_last_error = "cmfrec_hip: row parts are only built for A-steps without side information";
        return 2;
    }
    const int kk = v.kk, kc = v.kc, rows_u = v.rows_u;
    const int rows_x_self = v.rows_x_self;                    // rows of this matrix X has
    const real_t w = v.w;
    const bool scale_lam = m.scale_lam || m.scale_lam_sideinfo;                                     // :7465

    // the X block of a block-CG system: the implicit model's Gramian, or the explicit model's fixed bias column and fused "X - bias"
    auto block_cg_call = [&](bool scale_bias_const) {
        const real_t *bias_sub_cg = nullptr;
        int kx = kk;
        if (m.implicit) {
            launch_gram(dev, s->gws, oppx, ld_opp, rows_opp, kk, s->gram.ptr, (real_t)1, (real_t)0);
        } else {
            fill_fixed_bias_column(s, v);
            HIP_CHECK(hipGetLastError());
            kx = v.ks;
            bias_sub_cg = v.bias;
        }
        CgCall c{self_blk, ld_self, oppx, ld_opp, kx, bias_sub_cg, m.implicit ? s->gram.ptr : nullptr, lam_self, lam_last_self, scale_lam,
                 scale_bias_const, m.max_cg_steps, (bool)m.implicit, (bool)m.precondition_cg};
        c.koff = k_side_self; c.kc = kc; c.w_side = w; c.p_side = p_self; c.scale_lam_sideinfo = (bool)m.scale_lam_sideinfo;
        return c;
    };
    // ... and its implicit-features term (collective.c:2301-2304, :2624-2643, :2862-2868; round 6: with u_vec_sp too): the unweighted
    // Bi^T Bi apart, the right-hand-side term by the gather-sum where the tables allow it
    auto add_implicit_term_cg = [&](CgCall &c) {
        if (v.Fi == nullptr || m.implicit) return;
        launch_implicit_gram(s, v, rows_opp, false, false);
        set_implicit_term(s, v, c);
        if (part < 0 && launch_gsum(s, v, v.Fi, (size_t)kk, kk, s->grhs.ptr, X.nrows)) c.gsum = s->grhs.ptr;
    };

    if (p_self > 0 && v.sparse_side) {
        // sparse side information (missing = absent): the row's attributes are a second gather source of the same
        // Cholesky launch (collective.c:1636-1653, :1719-1731 / :2003-2021) or of the lane <-> unknown CG kernel
        if (!chol) {
            // block CG / PCG with the attributes as a second gathered term (collective_block_cg u_vec_sp branches,
            // collective.c:2292-2298, :2609-2621, :2847-2860; implicit: :2993-2999 ff.), generic kernel
            CgCall c = block_cg_call(false);          // (scale_bias_const: not with sparse side information)
            c.rows_with_u = rows_u;
            set_sparse_side(v, c);
            add_implicit_term_cg(c);
            return launch_cg_any(dev, c, X, nullptr);
        }
        if (m.implicit) {
            if (X.nrows) HIP_CHECK(hipMemsetAsync(self_blk, 0, (size_t)X.nrows * ld_self * sizeof(real_t), st));   // :6018-6019
            const int kt = k_side_self + kk;
            launch_gram(dev, s->gws, oppx, ld_opp, rows_opp, kk, s->gram.ptr, (real_t)1, lam_self);
            hipLaunchKernelGGL(betbe_base_kernel<real_t>, grid1d(kt * kt), dim3(256), 0, st, s->gram.ptr, kk, k_side_self, lam_self,
                               s->betbe.ptr);
            CholCall c{self_blk, ld_self, oppx, ld_opp, kt, k_side_self, nullptr, nullptr, kc, rows_u, p_self, lam_self,
                       lam_last_self, false, false, false, CHOL_COLLECTIVE_IMPLICIT, s->betbe.ptr};
            set_sparse_side(v, c);
            return launch_chol(dev, c, &X);
        }
        // (the explicit model's closed form: below, after the implicit-features term it may carry)
    }
    // rows of the local block with side information, and those of them that X has (explicit model: rows beyond X are not part of
    // the block system, solve_sideinfo_only_rows)
    const int local_u = std::max(0, std::min(rows_u - begin, X.nrows));
    const int local_x = std::max(0, std::min(rows_x_self - begin, X.nrows));
    if (p_self > 0 && !chol) {
        // block CG on the collective system, dense full side information: collective_block_cg (explicit,
        // collective.c:2134-2903) / collective_block_cg_implicit (:2905-3303), prefer_CtC branch
        launch_gram(dev, s->gws, v.Cm, (size_t)kc, p_self, kc, s->ctc.ptr, (real_t)1, (real_t)0);   // C^T C, unweighted
        side_times(dev, v.Um_blk, local_u, kc, p_self, (real_t)1, v.Cm, v.uc, (size_t)kc);   // U C
        CgCall c = block_cg_call(sbc);
        const int local_u_main = m.implicit ? local_u : std::min(local_u, local_x);
        c.CtC = s->ctc.ptr; c.UC = v.uc; c.rows_with_u = local_u_main;
        add_implicit_term_cg(c);
        int rc = launch_cg_any(dev, c, X, nullptr);
        if (rc) return rc;
        return solve_sideinfo_only_rows(s, v, false, local_u_main, local_u - local_u_main);
    }
    if (m.implicit && p_self > 0) {
        // optimizeA_collective_implicit, Cholesky, dense full side information (collective.c:5971-6244)
        const int kt = k_side_self + kk;
        launch_gram(dev, s->gws, oppx, ld_opp, rows_opp, kk, s->gram.ptr, (real_t)1, lam_self);     // :6056-6061
        hipLaunchKernelGGL(betbe_base_kernel<real_t>, grid1d(kt * kt), dim3(256), 0, st, s->gram.ptr, kk, k_side_self, lam_self,
                           s->betbe.ptr);                                                           // :6121-6135
        launch_gram(dev, s->gws, v.Cm, (size_t)kc, p_self, kc, s->ctc.ptr, w, (real_t)0);          // :6138-6160
        if (X.nrows) HIP_CHECK(hipMemsetAsync(self_blk, 0, (size_t)X.nrows * ld_self * sizeof(real_t), st));   // :6018-6019
        side_times(dev, v.Um_blk, local_u, kc, p_self, w, v.Cm, self_blk, ld_self);   // :6163-6168
        CholCall c{self_blk, ld_self, oppx, ld_opp, kt, k_side_self, nullptr, s->ctc.ptr, kc, local_u,
                   p_self, lam_self, lam_last_self, false, false, false, CHOL_COLLECTIVE_IMPLICIT, s->betbe.ptr};
        return launch_chol(dev, c, &X);
    }
    if (m.implicit) {
        // optimizeA_implicit, common.c:3305-3421 (the Gramian once per half-step: parts > 0 reuse it)
        if (part <= 0)
            launch_gram(dev, s->gws, oppx, ld_opp, rows_opp, kk, s->gram.ptr, (real_t)1, chol ? lam_self : (real_t)0);
        if (chol) {
            if (X.nrows) HIP_CHECK(hipMemsetAsync(self_blk, 0, (size_t)X.nrows * ld_self * sizeof(real_t), st)); // :3334
            CholCall c{self_blk + k_side_self, ld_self, oppx, ld_opp, kk, 0, nullptr,
                       s->gram.ptr, 0, 0, 0, lam_self, lam_last_self, false, false, false, CHOL_IMPLICIT};
            return launch_chol(dev, c, &X);
        }
        CgCall c{self_blk + k_side_self, ld_self, oppx, ld_opp, kk, nullptr, s->gram.ptr,
                 lam_self, lam_last_self, false, false, m.max_cg_steps, true, (bool)m.precondition_cg};
        return launch_cg_any(dev, c, X, v.bins);
    }

    // ---- explicit ----
    // the opposing matrix' bias column is fixed to 1 while this one's bias is fitted (collective.c:8538-8543, :8728-8732)
    fill_fixed_bias_column(s, v);
    HIP_CHECK(hipGetLastError());
    const real_t *bias_sub = v.bias;                                        // fused "X - bias" (:8566-8570, :8750-8754)
    const int ksolve = v.ks, kt = v.kt;
    // implicit features: w_i Bi^T Bi joins the X block of every row's matrix (collective.c:1704-1707) and
    // w_i sum_{j observed} Bi_j its right-hand side (:1757-1771).  The second gather source of the Cholesky launch reads
    // the same sparsity pattern with unit values from Bi, right-hand side only.
    const real_t *Fi = chol ? v.Fi : nullptr;
    if (Fi != nullptr) {
        launch_implicit_gram(s, v, rows_opp, true, false);
        hipLaunchKernelGGL(embed_block_kernel<real_t>, grid1d(kt * kt), dim3(256), 0, st, s->bitbi.ptr, kk, k_side_self,
                           kt, s->bitbi_full.ptr);
        HIP_CHECK(hipGetLastError());
    }
    auto add_implicit_term = [&](CholCall &c) {
        if (Fi == nullptr) return;
        c.Mfull = s->bitbi_full.ptr;
        if (part < 0 && launch_gsum(s, v, Fi, (size_t)kk, kk, s->grhs.ptr, X.nrows)) {
            // the right-hand-side term by the segmented gather-sum, added to the (zeroed / w U C) rows the launch then starts
            // from: the row kernel gathers X only (first version: Bi as a second gather source of the same launch, c3 +
            // implicit features A-step 34.4 ms, B-step 20.5 ms)
            add_implicit_rhs(s, v, self_blk, ld_self);
            c.rhs_prefilled_all = true;
            return;
        }
        c.X2 = &X; c.values2 = s->ones.ptr; c.B2 = Fi; c.ldb2 = (size_t)kk; c.kc2 = kk; c.koff2 = k_side_self;
        c.w2 = s->w_implicit; c.w2_syr_zero = true; c.rows2 = X.nrows;
    };
    if (p_self > 0 && v.sparse_side) {
        // sparse side information, closed form: the row's attributes as the second gather source (collective.c:1636-1653, :1719-1731);
        // round 6: together with the implicit-features term (its right-hand side by the segmented gather-sum)
        if (X.nrows) HIP_CHECK(hipMemsetAsync(self_blk, 0, (size_t)X.nrows * ld_self * sizeof(real_t), st));   // :4817-4822
        CholCall c{self_blk, ld_self, oppx, ld_opp, kt, k_side_self, bias_sub, nullptr, kc, rows_u, p_self, lam_self,
                   lam_last_self, scale_lam, (bool)m.scale_lam_sideinfo, false, CHOL_COLLECTIVE};
        add_implicit_term(c);
        if (c.X2 != nullptr) {
            g_last_error = "cmfrec_hip: implicit features with sparse side information: k + k_main beyond the gather-sum's width";
            return 2;
        }
        set_sparse_side(v, c);
        return launch_chol(dev, c, &X);
    }
    if (p_self > 0) {
        // optimizeA_collective general branch, Cholesky (collective.c:5566-5968)
        launch_gram(dev, s->gws, v.Cm, (size_t)kc, p_self, kc, s->ctc.ptr, w, (real_t)0);          // :5658-5668
        if (X.nrows) HIP_CHECK(hipMemsetAsync(self_blk, 0, (size_t)X.nrows * ld_self * sizeof(real_t), st));   // :4817-4822
        side_times(dev, v.Um_blk, local_u, kc, p_self, w, v.Cm, self_blk, ld_self);   // :5768-5773
        const int local_u_main = std::min(local_u, local_x);              // rows beyond X: solve_sideinfo_only_rows
        CholCall c{self_blk, ld_self, oppx, ld_opp, kt, k_side_self, bias_sub, s->ctc.ptr, kc, local_u_main,
                   p_self, lam_self, lam_last_self, scale_lam, (bool)m.scale_lam_sideinfo, sbc, CHOL_COLLECTIVE};
        add_implicit_term(c);
        // rows with few entries against many unknowns: low-rank path (lowrank_kernels.hpp)
        if (Fi == nullptr && !sbc && local_u_main == X.nrows && part < 0) {
            // the other side's w D^T D, if its next half-step will want the eigenvectors and they are not there yet: decomposed
            // behind this side's (EigCache)
            EigCache *next = v.eig_next;
            if (next->wanted && !next->fresh && v.p_next > 0 && !v.sparse_side_next) {
                next->M.alloc_at_least((size_t)v.kc_next * v.kc_next);
                launch_gram(dev, s->gws, v.Cm_next, (size_t)v.kc_next, v.p_next, v.kc_next, next->M.ptr, v.w_next, (real_t)0);
            } else {
                next = nullptr;
            }
            const int rc_lr = launch_collective_lowrank(dev, s->lr, c, X, v.Cm, v.Um_blk, p_self, w, m.k, v.rows_opp, v.eig_mine, next,
                                                        v.kc_next);
            if (rc_lr >= 0) return rc_lr;
        }
        int rc = launch_chol(dev, c, &X);
        if (rc) return rc;
        return solve_sideinfo_only_rows(s, v, true, local_u_main, local_u - local_u_main);
    }
    if (Fi != nullptr) {
        // without side information on this side the reference still takes optimizeA_collective (collective.c:8612, :8783)
        if (X.nrows) HIP_CHECK(hipMemsetAsync(self_blk, 0, (size_t)X.nrows * ld_self * sizeof(real_t), st));   // :4817-4822
        CholCall c{self_blk, ld_self, oppx, ld_opp, ksolve, 0, bias_sub, nullptr, 0, 0, 0,
                   lam_self, lam_last_self, scale_lam, false, false, CHOL_COLLECTIVE};
        add_implicit_term(c);
        return launch_chol(dev, c, &X);
    }
    if (chol) {
        CholCall c{self_blk + k_side_self, ld_self, oppx, ld_opp, ksolve, 0, bias_sub, nullptr, 0, 0, 0,
                   lam_self, lam_last_self, scale_lam, false, sbc, CHOL_EXPLICIT};
        return launch_chol(dev, c, &X);
    }
    CgCall c{self_blk + k_side_self, ld_self, oppx, ld_opp, ksolve, bias_sub, nullptr,
             lam_self, lam_last_self, scale_lam, sbc, m.max_cg_steps, false, (bool)m.precondition_cg};
    // block CG with the implicit-features term (collective_block_cg without side information on this side,
    // collective.c:2624-2643, :2862-2868): generic kernel; rows without entries are zeroed (:1258-1268)
    add_implicit_term_cg(c);
    return launch_cg_any(dev, c, X, v.bins);
}

// Ai / Bi update: optimizeA Case 3 on the binary indicator of X (collective.c:8448-8534; common.c:3116-3205): one
// shared matrix F^T F + lam/w_i (x rows of F under scale_lam), right-hand sides sum_{j observed} F_j
static int update_implicit_feats(cmfrec_hip_session *s, bool isAi)
{
    const cmfrec_hip_model &m = s->mdl;
    const DeviceInfo &dev = s->dev;
    const HalfStepSide v(s, isAi);
    const int kk = v.kk;
    real_t *self = isAi ? s->Ai.ptr : s->Bi.ptr;
    const real_t *F = v.oppx;                                                // B_bias + k_item / A_bias + k_user
    const size_t ldf = v.ld_opp;
    const int rows_f = v.rows_opp, rows_self = v.rows_self;
    const SparseShard &X = v.X;
    const bool scale_lam = m.scale_lam || m.scale_lam_sideinfo;
    const real_t lam = (v.lam_self / s->w_implicit) * (scale_lam ? (real_t)rows_f : (real_t)1);   // :8469, :8510
    launch_gram(dev, s->gws, F, ldf, rows_f, kk, s->gram.ptr, (real_t)1, lam);
    HIP_CHECK(hipMemsetAsync(self, 0, (size_t)rows_self * kk * sizeof(real_t), dev.stream));
    CholCall c{self, (size_t)kk, F, ldf, kk, 0, nullptr, s->gram.ptr, 0, 0, 0, lam, lam, false, false, false, CHOL_NAZ};
    c.values_override = s->ones.ptr;
    if (dev.nonneg_now || dev.l1_now != (real_t)0 || dev.l1_last_now != (real_t)0)
        return launch_chol(dev, c, &X);             // coordinate descent: per row on the assembled system
    // one factorisation of the shared matrix, the row kernel only gathers the right-hand sides (first version: the
    // matrix factorised once per row -- c1 + implicit features 8 ms for Bi + Ai)
    // ... first by the row kernel itself (rhs_only, still the path of wider systems), whose staging loop made the longest
    // row the critical path (Bi at the C1 shape 4.5 ms); now a two-stage segmented gather-sum
    if (!launch_gsum(s, v, F, ldf, kk, self, rows_self)) {
        c.rhs_only = true;
        int rc = launch_chol(dev, c, &X);
        if (rc) return rc;
    }
    hipLaunchKernelGGL(potrf_upper_kernel<real_t>, dim3(1), dim3(256), 0, dev.stream, s->gram.ptr, kk);
    HIP_CHECK(hipGetLastError());
    launch_potrs_rows(dev, rows_self, kk, s->gram.ptr, self, (size_t)kk);
    return 0;
}

// C / D update: optimizeA Case 1 with do_B (common.c:2793-2991; Q6: always the transposed gemm)
static int update_sideinfo(cmfrec_hip_session *s, bool isC, bool chol, int cg_steps = -1)
{
    const cmfrec_hip_model &m = s->mdl;
    const DeviceInfo &dev = s->dev;
    const int p = isC ? m.p : m.q;
    if (p <= 0) return 0;
    (isC ? s->eigA : s->eigB).fresh = false;
    const int rows_u = isC ? m.m_u : m.n_i;
    const int kc = (isC ? m.k_user : m.k_item) + m.k;
    real_t *Cm = isC ? s->C.ptr : s->D.ptr;
    const SideOperand Um = s->side_operand(isC);
    const real_t *F = isC ? s->A.ptr : s->B.ptr;
    const size_t ldF = isC ? s->ldA : s->ldB;
    const real_t w = isC ? m.w_user : m.w_item;
    const bool scale_lam = m.scale_lam || m.scale_lam_sideinfo;
    real_t lam = s->lam6[isC ? 4 : 5] / w;                                                                    // collective.c:8367, :8418
    if (isC ? s->sparseU : s->sparseI) {
        // sparse side information: optimizeA Case 4 on its CSC -- one row of C per attribute, gathered from the
        // first k_side+k columns of the factor matrix (collective.c:8354-8386; attributes nobody has stay untouched)
        const SparseShard &Uc = isC ? s->Usc : s->Isc;
        if (!chol) {
            CgCall cg{Cm, (size_t)kc, F, ldF, kc, nullptr, nullptr, lam, lam, scale_lam, false, cg_steps > 0 ? cg_steps : m.max_cg_steps, false,
                      (bool)m.precondition_cg};
            return launch_cg_any(dev, cg, Uc);
        }
        CholCall c{Cm, (size_t)kc, F, ldF, kc, 0, nullptr, nullptr, 0, 0, 0, lam, lam, scale_lam, false, false, CHOL_EXPLICIT};
        return launch_chol(dev, c, &Uc);
    }
    real_t diag = scale_lam ? lam * (real_t)rows_u : lam;                                          // common.c:2832
    launch_gram(dev, s->gws, F, ldF, rows_u, kc, s->gram.ptr, (real_t)1, diag);                    // common.c:2824
    side_transposed_times(dev, Um, rows_u, kc, p, F, ldF, Cm, (size_t)kc);                         // common.c:2852-2855
    CholCall c{Cm, (size_t)kc, nullptr, 0, kc, 0, nullptr, s->gram.ptr, 0, 0, 0, 0, 0, false, false, false, CHOL_PREFILLED};
    return launch_chol(dev, c, nullptr, p);                                                        // common.c:2872-2875
}

// The matrices the reference keeps for predictions on new data (the step after the path),
// from the factors resident in the session:
//   implicit (epilogue of fit_collective_implicit_als, src/collective.c:10056-10115):
//     BtB = B^T B + lam I;  with user side information  BeTBe = blockdiag(lam I, BtB) + w C^T C  and its Cholesky factor
//   explicit (epilogue of fit_collective_explicit_als, :8936-9249), Bp = [B(:, k_item:) | 1 if user_bias]:
//     BtB = Bp^T Bp;  TransBtBinvBt = Bp (BtB + lam (n if scale_lam) I)^-1;  CtCw = w C^T C;
//     TransCtCinvCt = C (C^T C + lam (p if scale_lam) / w I)^-1;
//     BeTBeChol = chol(blockdiag(0, BtB) + CtCw + lam mult I),  mult = p + n | n | 1
// Host output buffers, NULL = skip; square matrices are complete (both triangles) except the Cholesky factors
// (upper triangle R, M = R^T R; the strict lower triangle holds the lower triangle of M).
int cmfrec_hip_session_precompute(cmfrec_hip_session *s, int last_step_cholesky, int include_all_X, real_t *BtB,
                                  real_t *TransBtBinvBt, real_t *BeTBe, real_t *BeTBeChol, real_t *CtCw,
                                  real_t *TransCtCinvCt)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        cmfrec_hip_model m = s->mdl;
        // rows of B that enter: n_max with include_all_X (explicit model only), else the columns of X (collective.c:9013-9016)
        if (!(include_all_X && !m.implicit) && m.n_x > 0) m.n = m.n_x;
        const DeviceInfo &dev = s->dev;
        hipStream_t st = dev.stream;
        const int kk = m.k + m.k_main, ub = (!m.implicit && m.user_bias) ? 1 : 0;
        const int kp = kk + ub, kc = m.k_user + m.k, kq = m.k_user + kp;
        const bool scale_lam = m.scale_lam || m.scale_lam_sideinfo;
        DevBuf<real_t> Bp, G, M, T1;
        Bp.alloc((size_t)m.n * kp); G.alloc((size_t)kp * kp);
        hipLaunchKernelGGL(copy_mat_kernel<real_t>, grid1d((size_t)m.n * kk), dim3(256), 0, st, s->B.ptr + m.k_item, s->ldB, Bp.ptr,
                           (size_t)kp, (size_t)m.n, kk);
        if (ub) hipLaunchKernelGGL(col_fill_kernel<real_t>, grid1d(m.n), dim3(256), 0, st, Bp.ptr, (size_t)kp, m.n, kk, (real_t)1);
        // lam_unique[2] for the users' systems, the bias' own lam_unique[0] as a correction of the last diagonal entry
        // (collective.c:9066-9074, :9225-9238).  Implicit model: the Gramian keeps the lambda of the last A-step when that ran
        // Cholesky (lam_unique[2]), else the epilogue adds the scalar lam (:10062-10075).
        const real_t lamA = m.implicit ? (last_step_cholesky ? s->lam6[2] : m.lam) : s->lam6[2];
        const real_t lam_bias_diff = ub ? s->lam6[0] - s->lam6[2] : (real_t)0;
        launch_gram(dev, s->gws, Bp.ptr, (size_t)kp, m.n, kp, G.ptr, (real_t)1, m.implicit ? lamA : (real_t)0);
        if (BtB) G.download(BtB, (size_t)kp * kp, st);
        if (TransBtBinvBt && !m.implicit) {                               // collective.c:9034-9082
            M.alloc((size_t)kp * kp);
            HIP_CHECK(hipMemcpyAsync(M.ptr, G.ptr, (size_t)kp * kp * sizeof(real_t), hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(kp), dim3(256), 0, st, M.ptr, kp, 0, kp,
                               lamA * (real_t)(m.scale_lam ? m.n : 1));
            if (lam_bias_diff != 0)
                hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(1), dim3(256), 0, st, M.ptr, kp, kp - 1, kp,
                                   lam_bias_diff * (real_t)(m.scale_lam ? m.n : 1));
            CholCall c{Bp.ptr, (size_t)kp, nullptr, 0, kp, 0, nullptr, M.ptr, 0, 0, 0, 0, 0, false, false, false, CHOL_PREFILLED};
            int rc = launch_chol(dev, c, nullptr, m.n);
            if (rc) return rc;
            Bp.download(TransBtBinvBt, (size_t)m.n * kp, st);
        }
        if (m.p > 0) {
            const real_t w = m.w_user;
            DevBuf<real_t> CtC, Cc;
            CtC.alloc((size_t)kc * kc);
            launch_gram(dev, s->gws, s->C.ptr, (size_t)kc, m.p, kc, CtC.ptr, (real_t)1, (real_t)0);
            if (TransCtCinvCt && !m.implicit) {                           // :9083-9142
                M.alloc((size_t)kc * kc); Cc.alloc((size_t)m.p * kc);
                HIP_CHECK(hipMemcpyAsync(M.ptr, CtC.ptr, (size_t)kc * kc * sizeof(real_t), hipMemcpyDeviceToDevice, st));
                HIP_CHECK(hipMemcpyAsync(Cc.ptr, s->C.ptr, (size_t)m.p * kc * sizeof(real_t), hipMemcpyDeviceToDevice, st));
                hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(kc), dim3(256), 0, st, M.ptr, kc, 0, kc,
                                   lamA * (real_t)(m.scale_lam ? m.p : 1) / w);
                CholCall c{Cc.ptr, (size_t)kc, nullptr, 0, kc, 0, nullptr, M.ptr, 0, 0, 0, 0, 0, false, false, false, CHOL_PREFILLED};
                int rc = launch_chol(dev, c, nullptr, m.p);
                if (rc) return rc;
                Cc.download(TransCtCinvCt, (size_t)m.p * kc, st);
            }
            if (CtCw) {                                                   // w C^T C
                T1.alloc((size_t)kc * kc);
                HIP_CHECK(hipMemsetAsync(T1.ptr, 0, (size_t)kc * kc * sizeof(real_t), st));
                hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kc * kc), dim3(256), 0, st, CtC.ptr, kc, w, T1.ptr, kc, 0);
                T1.download(CtCw, (size_t)kc * kc, st);
                HIP_CHECK(hipStreamSynchronize(st));
            }
            if (BeTBe || BeTBeChol) {                                     // :9184-9243 / :10073-10110
                M.alloc((size_t)kq * kq);
                HIP_CHECK(hipMemsetAsync(M.ptr, 0, (size_t)kq * kq * sizeof(real_t), st));
                hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kp * kp), dim3(256), 0, st, G.ptr, kp, (real_t)1, M.ptr, kq, m.k_user);
                // Quirk Q9 (reference behaviour, reproduced on purpose -- see DESIGN.md "Parity"): in the implicit model
                // whose last iteration ran CG (no finalize_chol) the epilogue scales the cached C^T C by w_user only `if (w_user == 1.)`
                // (src/collective.c:10077, the test is inverted), so for w_user != 1 the UNWEIGHTED C^T C ends up in
                // BeTBe / BeTBeChol.  With Cholesky (or w_user == 1) the weighted matrix comes out, as intended.
                const real_t w_betbe = (m.implicit && !last_step_cholesky) ? (real_t)1 : w;
                hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kc * kc), dim3(256), 0, st, CtC.ptr, kc, w_betbe, M.ptr, kq, 0);
                if (m.implicit) {                                         // lam is already inside G; the k_user block gets its own
                    if (m.k_user) hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(m.k_user), dim3(256), 0, st, M.ptr, kq, 0, m.k_user, lamA);
                } else {
                    const real_t mult = m.scale_lam_sideinfo ? (real_t)(m.p + m.n) : (scale_lam ? (real_t)m.n : (real_t)1);
                    hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(kq), dim3(256), 0, st, M.ptr, kq, 0, kq, lamA * mult);
                    if (lam_bias_diff != 0)
                        hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(1), dim3(256), 0, st, M.ptr, kq, kq - 1, kq, lam_bias_diff * mult);
                }
                if (BeTBe) M.download(BeTBe, (size_t)kq * kq, st);
                if (BeTBeChol) {
                    hipLaunchKernelGGL(potrf_upper_kernel<real_t>, dim3(1), dim3(256), 0, st, M.ptr, kq);
                    M.download(BeTBeChol, (size_t)kq * kq, st);
                }
            }
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}

int cmfrec_hip_session_after_gather(cmfrec_hip_session *s, int which)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const cmfrec_hip_model &m = s->mdl;
        hipStream_t st = s->dev.stream;
        if (m.implicit || !s->has_bias) return 0;
        if (which == 'B') {
            if (m.item_bias)     // collective.c:8723-8725
                hipLaunchKernelGGL(col_extract_kernel<real_t>, grid1d(m.n), dim3(256), 0, st, s->B.ptr, s->ldB, m.n, s->k_totB, s->biasB.ptr);
            if (m.user_bias)     // collective.c:8728-8732
                hipLaunchKernelGGL(col_fill_kernel<real_t>, grid1d(m.n), dim3(256), 0, st, s->B.ptr, s->ldB, m.n, s->k_totB, (real_t)1);
        } else if (which == 'A') {
            if (m.user_bias)     // collective.c:8882-8884
                hipLaunchKernelGGL(col_extract_kernel<real_t>, grid1d(m.m), dim3(256), 0, st, s->A.ptr, s->ldA, m.m, s->k_totA, s->biasA.ptr);
            if (m.item_bias)     // collective.c:8538-8543 (done at the top of the next iteration in the reference)
                hipLaunchKernelGGL(col_fill_kernel<real_t>, grid1d(m.m), dim3(256), 0, st, s->A.ptr, s->ldA, m.m, s->k_totA, (real_t)1);
        }
        HIP_CHECK(hipGetLastError());
        return 0;
    });
}

int cmfrec_hip_session_update(cmfrec_hip_session *s, int which, int use_cholesky)
{
    return guarded([&]() {
        HIP_CHECK(hipSetDevice(s->dev.device));
        const bool isAB = (which == 'A' || which == 'B'), isImp = (which == 'a' || which == 'b');
        const bool nn = (isAB || isImp) ? s->nonneg : (which == 'C' ? s->nonneg_C : s->nonneg_D);
        // l1_lam_unique order: user bias, item bias, A, B, C, D (collective.c:8652-8654, :8823-8825, :8369-8423, :8472-8516)
        const bool ub = !s->mdl.implicit && s->mdl.user_bias, ib = !s->mdl.implicit && s->mdl.item_bias;
        const real_t l1 = which == 'A' ? s->l16[2] : which == 'B' ? s->l16[3] : which == 'a' ? s->l16[2] / s->w_implicit
                          : which == 'b' ? s->l16[3] / s->w_implicit
                          : (which == 'C' ? s->l16[4] / s->mdl.w_user : s->l16[5] / s->mdl.w_item);
        const real_t l1_last = which == 'A' ? s->l16[ub ? 0 : 2] : which == 'B' ? s->l16[ib ? 1 : 3] : l1;
        const bool chol = use_cholesky || !s->mdl.use_cg || nn || l1 != 0 || l1_last != 0;   // common.c:725, :2781, :3320: no CG with nonneg / L1
        struct SolveScope {                                           // the closed-form launches of this update
            const DeviceInfo &d;
            SolveScope(const DeviceInfo &d_, bool on, int steps, real_t l1_, real_t l1l, real_t sc) : d(d_)
            { d.nonneg_now = on; d.max_cd_steps = steps; d.l1_now = l1_; d.l1_last_now = l1l; d.l1_scale = sc; }
            ~SolveScope() { d.nonneg_now = false; d.l1_now = 0; d.l1_last_now = 0; d.l1_scale = 1; }
        } scope(s->dev, nn, s->max_cd_steps, l1, l1_last,
                // the dense C / D update scales lambda -- and the penalty -- by the number of rows of U / I (common.c:2832, :2882)
                // the Ai / Bi update (Case 3) by the rows of the fixed matrix (common.c:3131, :3182)
                ((which == 'C' || which == 'D' || isImp) && (s->mdl.scale_lam || s->mdl.scale_lam_sideinfo))
                    ? (real_t)(which == 'C' ? s->mdl.m_u : which == 'D' ? s->mdl.n_i : which == 'a' ? s->mdl.n : s->mdl.m)
                    : (real_t)1);
        if (which == 'A' || which == 'B') {
            EventPair ev{s->new_event(), s->new_event()};
            HIP_CHECK(hipEventRecord(ev.a, s->dev.stream));
            int rc = 0;
            if (which == 'A' && !s->XrParts.empty()) {
                for (int c = 0; c < (int)s->XrParts.size() && rc == 0; c++) {
                    rc = update_factor(s, true, chol, c);
                    HIP_CHECK(hipEventRecord(s->partEv[c], s->dev.stream));
                }
            } else {
                rc = update_factor(s, which == 'A', chol);
                if (rc == 0 && !chol && (which == 'A' ? s->has_cfA : s->has_cfB)) {
                    // rows of this half-step that the reference solves in closed form next to the CG rows
                    // (cmfrec_hip_session_set_closed_form_rows): CG results aside, closed form over all rows, CG rows back
                    const bool isA = which == 'A';
                    real_t *self = isA ? s->A.ptr : s->B.ptr;
                    const size_t ld = isA ? s->ldA : s->ldB, rows = (size_t)(isA ? s->mdl.m : s->mdl.n);
                    s->cf_keep.alloc_at_least(rows * ld);
                    HIP_CHECK(hipMemcpyAsync(s->cf_keep.ptr, self, rows * ld * sizeof(real_t), hipMemcpyDeviceToDevice, s->dev.stream));
                    rc = update_factor(s, isA, true);
                    if (rc != 0) {
                        // the closed-form pass failed part-way: put the CG results back whole rather than leave a mix of zeroed
                        // and half-solved rows behind the error code
                        HIP_CHECK(hipMemcpyAsync(self, s->cf_keep.ptr, rows * ld * sizeof(real_t), hipMemcpyDeviceToDevice, s->dev.stream));
                    } else {
                        hipLaunchKernelGGL(restore_rows_kernel<real_t>, grid1d(rows * ld), dim3(256), 0, s->dev.stream, self, s->cf_keep.ptr, ld, rows,
                                           (isA ? s->cfmaskA : s->cfmaskB).ptr);
                        HIP_CHECK(hipGetLastError());
                    }
                }
            }
            if (rc == 0 && (which == 'A' ? s->n_zrowsA : s->n_zrowsB) > 0) {
                // rows the reference does not solve under NA_as_zero_U / _I (cmfrec_hip_session_set_zero_rows): the unknowns of
                // the row, its own bias included; a bias column fixed to 1 stays
                const bool isA = which == 'A';
                const bool self_bias = !s->mdl.implicit && (isA ? s->mdl.user_bias : s->mdl.item_bias);
                const int ncols = (isA ? s->k_totA : s->k_totB) + (self_bias ? 1 : 0), cnt = isA ? s->n_zrowsA : s->n_zrowsB;
                hipLaunchKernelGGL(zero_rows_kernel<real_t>, grid1d((size_t)cnt * ncols), dim3(256), 0, s->dev.stream, isA ? s->A.ptr : s->B.ptr,
                                   isA ? s->ldA : s->ldB, ncols, (isA ? s->zrowsA : s->zrowsB).ptr, cnt);
                HIP_CHECK(hipGetLastError());
            }
            HIP_CHECK(hipEventRecord(ev.b, s->dev.stream));
            (which == 'A' ? s->evA : s->evB).push_back(ev);
            // long-lived sessions: the timing events are a window over the most recent updates, not an unbounded log
            trim_events(which == 'A' ? s->evA : s->evB);
            for (auto &v : (which == 'A' ? s->binA : s->binB).ev) trim_events(v);
            return rc;
        }
        if (which == 'C' || which == 'D') {
            if (s->side_local) {
                // the session holds the side information of its row block only: the whole-matrix update would read rows it
                // does not have -- the sharded form is sideinfo_partial + all-reduce + sideinfo_finish
                g_last_error = "cmfrec_hip_session_update: C / D of a session with local side information go through "
                               "cmfrec_hip_session_sideinfo_partial / _finish";
                return 2;
            }
            const bool isC = which == 'C';
            int rc = update_sideinfo(s, isC, chol);
            const bool *any = isC ? s->cfC_any : s->cfD_any;
            if (rc == 0 && !chol && (isC ? s->sparseU : s->sparseI) && (any[1] || any[2])) {
                // dense side information with NaN (cmfrec_hip_session_set_closed_form_rows 'C' / 'D'): next to the CG attributes the
                // reference solves some in closed form (mask 1) and some by CG from zero with k_side + k steps (mask 2)
                real_t *Cm = isC ? s->C.ptr : s->D.ptr;
                const int kc = (isC ? s->mdl.k_user : s->mdl.k_item) + s->mdl.k;
                const size_t rows = (size_t)(isC ? s->mdl.p : s->mdl.q), ld = (size_t)kc;
                const unsigned char *mask = (isC ? s->cfmaskC : s->cfmaskD).ptr;
                hipStream_t st = s->dev.stream;
                s->cf_keep.alloc_at_least(rows * ld);
                for (int value = 1; value <= 2 && rc == 0; value++) {
                    if (!any[value]) continue;
                    HIP_CHECK(hipMemcpyAsync(s->cf_keep.ptr, Cm, rows * ld * sizeof(real_t), hipMemcpyDeviceToDevice, st));
                    if (value == 2) HIP_CHECK(hipMemsetAsync(Cm, 0, rows * ld * sizeof(real_t), st));
                    rc = value == 1 ? update_sideinfo(s, isC, true) : update_sideinfo(s, isC, false, kc);
                    if (rc != 0) { HIP_CHECK(hipMemcpyAsync(Cm, s->cf_keep.ptr, rows * ld * sizeof(real_t), hipMemcpyDeviceToDevice, st)); break; }
                    hipLaunchKernelGGL(keep_rows_unless_kernel<real_t>, grid1d(rows * ld), dim3(256), 0, st, Cm, s->cf_keep.ptr, ld, rows, mask,
                                       (unsigned char)value);
                    HIP_CHECK(hipGetLastError());
                }
            }
            return rc;
        }
        if ((which == 'a' || which == 'b') && s->implicit_feats) return update_implicit_feats(s, which == 'a');
        g_last_error = "cmfrec_hip: unknown update target";
        return 2;
    });
}

int cmfrec_hip_session_iterate(cmfrec_hip_session *s, int niter, int finalize_chol)
{
    const cmfrec_hip_model &m = s->mdl;
    if (m.row_begin != 0 || m.row_end != m.m || m.col_begin != 0 || m.col_end != m.n) {
        g_last_error = "cmfrec_hip: iterate() needs a session that owns all rows (use update()+all-gather on shards)";
        return 2;
    }
    for (int it = 0; it < niter; it++) {
        // collective.c:8336-8340 / :9829-9830
        int chol = (finalize_chol && m.use_cg && it == niter - 1) ? 1 : 0;
        int rc;
        if (m.p > 0 && (rc = cmfrec_hip_session_update(s, 'C', chol))) return rc;
        if (m.q > 0 && (rc = cmfrec_hip_session_update(s, 'D', chol))) return rc;
        if (s->implicit_feats) {                                              // collective.c:8448-8534: Bi, then Ai
            if ((rc = cmfrec_hip_session_update(s, 'b', 1))) return rc;
            if ((rc = cmfrec_hip_session_update(s, 'a', 1))) return rc;
        }
        if ((rc = cmfrec_hip_session_update(s, 'B', chol))) return rc;
        if ((rc = cmfrec_hip_session_after_gather(s, 'B'))) return rc;
        if ((rc = cmfrec_hip_session_update(s, 'A', chol))) return rc;
        if ((rc = cmfrec_hip_session_after_gather(s, 'A'))) return rc;
    }
    return 0;
}

// the error of the current factors' predictions on a resident held-out set (predict_tu.hip, evalset_run): reads A, B and the
// biases where they are, behind the updates queued on the session's stream; writes nothing of the session's
int cmfrec_hip_session_errors(cmfrec_hip_session *s, cmfrec_hip_evalset *e, real_t glob_mean, cmfrec_hip_errors *out)
{
    return guarded([&]() {
        if (s == nullptr) {
            g_last_error = "cmfrec_hip_session_errors: invalid arguments";
            return 2;
        }
        const cmfrec_hip_model &m = s->mdl;
        if (m.row_begin != 0 || m.row_end != m.m || m.col_begin != 0 || m.col_end != m.n) {
            g_last_error = "cmfrec_hip_session_errors: needs a session that owns all rows";
            return 2;
        }
        if (m.k + m.k_main < 1) {
            g_last_error = "cmfrec_hip_session_errors: k + k_main >= 1";
            return 2;
        }
        const bool implicit = m.implicit != 0;
        return evalset_run(e, "cmfrec_hip_session_errors", s->dev.device, s->dev.num_cus, s->dev.stream, s->A.ptr + m.k_user, s->ldA, m.m,
                           (!implicit && m.user_bias) ? s->biasA.ptr : nullptr, 1, s->B.ptr + m.k_item, s->ldB, m.n, m.k + m.k_main,
                           (!implicit && m.item_bias) ? s->biasB.ptr : nullptr, implicit ? (real_t)0 : glob_mean, implicit, nullptr, out);
    });
}

// the ranking metrics of the current factors on a resident ranking set (topn_tu.hip, rankset_run_on_factors): the listed users' rows
// of A are gathered on the device, the session's ranker takes B (and the item bias of an explicit model that has one) by a
// device-to-device copy, then the rank kernel and the reduction run; writes nothing of the session's
int cmfrec_hip_session_ranking(cmfrec_hip_session *s, cmfrec_hip_rankset *set, int k_at, cmfrec_hip_rank_record *out)
{
    const char *fn = "cmfrec_hip_session_ranking";
    return guarded([&]() {
        if (s == nullptr) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        const cmfrec_hip_model &m = s->mdl;
        if (m.row_begin != 0 || m.row_end != m.m || m.col_begin != 0 || m.col_end != m.n) {
            g_last_error = std::string(fn) + ": needs a session that owns all rows";
            return 2;
        }
        if (m.k + m.k_main < 1) {
            g_last_error = std::string(fn) + ": k + k_main >= 1";
            return 2;
        }
        HIP_CHECK(hipSetDevice(s->dev.device));
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));          // the ranker has a stream of its own
        return rankset_run_on_factors(&s->ranker, set, fn, s->dev.device, s->A.ptr + m.k_user, s->ldA, m.m, s->B.ptr + m.k_item, s->ldB, m.n,
                                      m.k + m.k_main, (!m.implicit && m.item_bias) ? s->biasB.ptr : nullptr, k_at, out);
    });
}

// A second copy of everything cmfrec_hip_session_get_factors / _get_implicit_features return -- A and B in their padded layout
// (the bias column rides in them), the bias vectors, C, D, Ai, Bi -- so that a fit can go back to its best iterate.  The copies
// are device to device on the session's stream, behind the updates queued there.  What an update derives from the factors
// (Gramians, U C, the eigenvectors of C^T C) is rebuilt by the update that needs it; the cached eigenvectors are marked stale.
static int snapshot_copy(cmfrec_hip_session *s, const char *fn, bool restore)
{
    return guarded([&]() {
        if (s == nullptr) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        const cmfrec_hip_model &m = s->mdl;
        if (m.row_begin != 0 || m.row_end != m.m || m.col_begin != 0 || m.col_end != m.n || s->side_local) {
            g_last_error = std::string(fn) + ": needs a session that owns all rows";
            return 2;
        }
        if (restore && !s->has_snapshot) {
            g_last_error = std::string(fn) + ": no snapshot has been taken";
            return 2;
        }
        HIP_CHECK(hipSetDevice(s->dev.device));
        hipStream_t st = s->dev.stream;
        DevBuf<real_t> *live[8] = {&s->A, &s->B, &s->biasA, &s->biasB, &s->C, &s->D, &s->Ai, &s->Bi};
        for (int e = 0; e < 8; e++) {
            DevBuf<real_t> &cur = *live[e], &snap = s->snap[e];
            if (restore && snap.n != cur.n) {                 // (implicit features switched on after the snapshot, for instance)
                g_last_error = std::string(fn) + ": the session's matrices have changed shape since the snapshot";
                return 2;
            }
            if (!restore && snap.n != cur.n) snap.alloc(cur.n);
            if (cur.n == 0) continue;
            HIP_CHECK(hipMemcpyAsync(restore ? cur.ptr : snap.ptr, restore ? snap.ptr : cur.ptr, cur.n * sizeof(real_t),
                                     hipMemcpyDeviceToDevice, st));
        }
        if (restore) { s->eigA.fresh = false; s->eigB.fresh = false; }
        else s->has_snapshot = true;
        return 0;
    });
}
int cmfrec_hip_session_snapshot(cmfrec_hip_session *s) { return snapshot_copy(s, "cmfrec_hip_session_snapshot", false); }
int cmfrec_hip_session_restore(cmfrec_hip_session *s) { return snapshot_copy(s, "cmfrec_hip_session_restore", true); }

int cmfrec_hip_session_sync(cmfrec_hip_session *s)
{
    return guarded([&]() {
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        return 0;
    });
}

void *cmfrec_hip_session_device_ptr(cmfrec_hip_session *s, int which, size_t *rows, size_t *ld)
{
    switch (which) {
        case 'A': if (rows) *rows = s->mdl.m; if (ld) *ld = s->ldA; return s->A.ptr;
        case 'B': if (rows) *rows = s->mdl.n; if (ld) *ld = s->ldB; return s->B.ptr;
        // (whoever asks for C / D may write to it: the cached eigenvectors are not trusted afterwards)
        case 'C': if (rows) *rows = s->mdl.p; if (ld) *ld = s->mdl.k_user + s->mdl.k; s->eigA.fresh = false; return s->C.ptr;
        case 'D': if (rows) *rows = s->mdl.q; if (ld) *ld = s->mdl.k_item + s->mdl.k; s->eigB.fresh = false; return s->D.ptr;
        case 'a': if (rows) *rows = s->mdl.m; if (ld) *ld = 1; return s->biasA.ptr;
        case 'b': if (rows) *rows = s->mdl.n; if (ld) *ld = 1; return s->biasB.ptr;
        case 'P': if (rows) *rows = s->side_part.n; if (ld) *ld = 1; return s->side_part.ptr;   // partial sums of the C / D update
    }
    return nullptr;
}

void *cmfrec_hip_session_stream(cmfrec_hip_session *s) { return (void *)s->dev.stream; }

int cmfrec_hip_session_kernel_time(cmfrec_hip_session *s, int which, double *ms, long *launches)
{
    return guarded([&]() {
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        auto &v = (which == 'A') ? s->evA : s->evB;
        double tot = 0;
        for (auto &p : v) {
            float t = 0;
            HIP_CHECK(hipEventElapsedTime(&t, p.a, p.b));
            tot += t;
        }
        if (ms) *ms = tot;
        if (launches) *launches = (long)v.size();
        return 0;
    });
}

int cmfrec_hip_session_bin_stats(cmfrec_hip_session *s, int which, int bin, double *ms, long *launches,
                                 long *rows, unsigned long long *nnz)
{
    return guarded([&]() {
        if (bin < 0 || bin >= NBINS) return 2;
        HIP_CHECK(hipStreamSynchronize(s->dev.stream));
        BinTimers &bt = (which == 'A') ? s->binA : s->binB;
        const SparseShard &X = (which == 'A') ? s->Xr : s->Xc;
        double tot = 0;
        for (auto &p : bt.ev[bin]) {
            float t = 0;
            HIP_CHECK(hipEventElapsedTime(&t, p.a, p.b));
            tot += t;
        }
        if (ms) *ms = tot;
        // with row parts every half-step launches each bin once per part: report half-steps, not launches
        const long per_step = (which == 'A' && !s->XrParts.empty()) ? (long)s->XrParts.size() : 1;
        if (launches) *launches = (long)bt.ev[bin].size() / per_step;
        if (rows) *rows = X.bin_rows[bin];
        if (nnz) *nnz = X.bin_nnz[bin];
        return 0;
    });
}

int cmfrec_hip_session_bin_overlaps(cmfrec_hip_session *s, int which, int bin)
{
    const SparseShard &X = (which == 'A') ? s->Xr : s->Xc;
    if (which == 'A' && !s->XrParts.empty()) return 1;                    // the bins of a part alternate between two streams
    if (cg_bin_streams() > 1) return 1;                                    // the bins of a half-step run side by side (launch_cg_S)
    // (the Gramian path stays in line, launch_cg_S)
    const bool gram_in_line = cmfrec_hip_session_vh_mode(s, which) == 2 && true;
    return (bin == BIN_VHEAVY && X.vh_runs_aside(s->dev.num_cus) && !gram_in_line) ? 1 : 0;
}

// The most recent collective Cholesky half-step of the session: rows solved by the low-rank kernels (0: the path was not taken)
// and the eigen-decomposition behind them (3 tridiagonalisation + QL, 2 the one-workgroup Jacobi kernel)
int cmfrec_hip_session_lowrank_info(cmfrec_hip_session *s, int *rows, int *eig)
{
    if (rows) *rows = s->lr.last_rows;
    if (eig) *eig = s->lr.last_eig;
    return 0;
}

// rows of the CSR ('A') / CSC ('B') shard with at least this many entries are split rows (their entries are kept sorted by
// opposing index, SparseShard::vh_min)
int cmfrec_hip_session_vh_min(cmfrec_hip_session *s, int which)
{
    return ((which == 'A') ? s->Xr : s->Xc).vh_min;
}

int cmfrec_hip_session_vh_mode(cmfrec_hip_session *s, int which)
{
    const SparseShard &X = (which == 'A') ? s->Xr : s->Xc;
    if (X.bin_rows[BIN_VHEAVY] <= 0) return 0;
    const bool gram = (switches().vh != 0) ? switches().vh == 2 : X.prefer_gram((size_t)(s->mdl.k + s->mdl.k_main) * sizeof(real_t));
    return (gram && s->mdl.k + s->mdl.k_main <= 16 * GRAM_NTT) ? 2 : 1;
}

void cmfrec_hip_session_reset_timers(cmfrec_hip_session *s)
{
    (void)hipStreamSynchronize(s->dev.stream);
    s->binA.clear(); s->binB.clear();
    for (auto *v : {&s->evA, &s->evB}) {
        for (auto &p : *v) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
        v->clear();
    }
}

// ============================ level 2: operators with host buffers ============================

int cmfrec_hip_optimizeA_implicit(real_t *A, size_t lda, const real_t *B, size_t ldb, int_t m, int_t n, int_t k,
                                  const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr, real_t lam,
                                  bool use_cg, bool precondition_cg, int_t max_cg_steps, real_t *BtB_out)
{
    return guarded([&]() {
        DeviceInfo dev;
        init_device(dev, -1);
        DevBuf<real_t> dA, dB, dG;
        GramWorkspace gws;
        SparseShard X;
        dA.upload(A, (size_t)m * lda, dev.stream);
        dB.upload(B, (size_t)n * ldb, dev.stream);
        dG.alloc((size_t)k * k);
        X.opp_row_bytes_hint = (size_t)k * sizeof(real_t);
        shard_from_csr(X, m, Xcsr_p, Xcsr_i, Xcsr, n, dev.stream);
        launch_gram(dev, gws, dB.ptr, ldb, n, k, dG.ptr, (real_t)1, use_cg ? (real_t)0 : lam);
        int rc;
        if (use_cg) {
            CgCall c{dA.ptr, lda, dB.ptr, ldb, k, nullptr, dG.ptr, lam, lam, false, false, max_cg_steps, true, precondition_cg};
            rc = launch_cg_any(dev, c, X);
        } else {
            // common.c:3334 zeroes m*k - (lda-k) elements from A
            HIP_CHECK(hipMemsetAsync(dA.ptr, 0, ((size_t)m * lda - (lda - (size_t)k)) * sizeof(real_t), dev.stream));
            CholCall c{dA.ptr, lda, dB.ptr, ldb, k, 0, nullptr, dG.ptr, 0, 0, 0, lam, lam, false, false, false, CHOL_IMPLICIT};
            rc = launch_chol(dev, c, &X);
        }
        dA.download(A, (size_t)m * lda, dev.stream);
        if (BtB_out) dG.download(BtB_out, (size_t)k * k, dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        return rc;
    });
}

int cmfrec_hip_optimizeA_explicit(real_t *A, size_t lda, const real_t *B, size_t ldb, int_t m, int_t n, int_t k,
                                  const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
                                  const real_t *bias_sub, real_t lam, real_t lam_last, bool scale_lam,
                                  bool scale_bias_const, bool use_cg, bool precondition_cg, int_t max_cg_steps)
{
    return cmfrec_hip_optimizeA_explicit_weighted(A, lda, B, ldb, m, n, k, Xcsr_p, Xcsr_i, Xcsr, nullptr, nullptr, bias_sub, lam, lam_last,
                                                  scale_lam, scale_bias_const, use_cg, precondition_cg, max_cg_steps);
}

int cmfrec_hip_optimizeA_explicit_weighted(real_t *A, size_t lda, const real_t *B, size_t ldb, int_t m, int_t n, int_t k,
                                           const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr, const real_t *weight,
                                           const real_t *wsum, const real_t *bias_sub, real_t lam, real_t lam_last, bool scale_lam,
                                           bool scale_bias_const, bool use_cg, bool precondition_cg, int_t max_cg_steps)
{
    return guarded([&]() {
        DeviceInfo dev;
        init_device(dev, -1);
        DevBuf<real_t> dA, dB, dbias;
        SparseShard X;
        dA.upload(A, (size_t)m * lda, dev.stream);
        dB.upload(B, (size_t)n * ldb, dev.stream);
        if (bias_sub) dbias.upload(bias_sub, n, dev.stream);
        X.opp_row_bytes_hint = (size_t)k * sizeof(real_t);
        shard_from_csr(X, m, Xcsr_p, Xcsr_i, Xcsr, n, dev.stream, weight);
        if (weight != nullptr && wsum != nullptr && X.weighted()) {      // the driver's multipliers instead of the rows' own sums
            X.wsum.upload(wsum, (size_t)m, dev.stream);
            HIP_CHECK(hipStreamSynchronize(dev.stream));
        }
        int rc;
        if (use_cg) {
            CgCall c{dA.ptr, lda, dB.ptr, ldb, k, bias_sub ? dbias.ptr : nullptr, nullptr, lam, lam_last, scale_lam,
                     scale_bias_const, max_cg_steps, false, precondition_cg};
            rc = launch_cg_any(dev, c, X);
        } else {
            CholCall c{dA.ptr, lda, dB.ptr, ldb, k, 0, bias_sub ? dbias.ptr : nullptr, nullptr, 0, 0, 0, lam, lam_last,
                       scale_lam, false, scale_bias_const, CHOL_EXPLICIT};
            rc = launch_chol(dev, c, &X);
        }
        dA.download(A, (size_t)m * lda, dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        return rc;
    });
}

int cmfrec_hip_optimizeA_dense_full(real_t *A, size_t lda, const real_t *B, size_t ldb, int_t m, int_t n, int_t k,
                                    const real_t *Xfull, size_t ldX, bool do_B, real_t lam, real_t lam_last,
                                    bool scale_lam)
{
    return guarded([&]() {
        if (lam != lam_last) { g_last_error = "cmfrec_hip: dense_full supports lam_last == lam only"; return 2; }
        DeviceInfo dev;
        init_device(dev, -1);
        DevBuf<real_t> dA, dB, dX, dG;
        GramWorkspace gws;
        dA.alloc((size_t)m * lda);
        HIP_CHECK(hipMemsetAsync(dA.ptr, 0, dA.n * sizeof(real_t), dev.stream));
        dB.upload(B, (size_t)n * ldb, dev.stream);
        size_t xrows = do_B ? (size_t)n : (size_t)m;
        dX.upload(Xfull, xrows * ldX, dev.stream);
        dG.alloc((size_t)k * k);
        launch_gram(dev, gws, dB.ptr, ldb, n, k, dG.ptr, (real_t)1, scale_lam ? lam * (real_t)n : lam);
        if (do_B) launch_gemm<true>(dev, m, k, n, (real_t)1, dX.ptr, ldX, dB.ptr, ldb, dA.ptr, lda);
        else      launch_gemm<false>(dev, m, k, n, (real_t)1, dX.ptr, ldX, dB.ptr, ldb, dA.ptr, lda);
        CholCall c{dA.ptr, lda, nullptr, 0, k, 0, nullptr, dG.ptr, 0, 0, 0, 0, 0, false, false, false, CHOL_PREFILLED};
        int rc = launch_chol(dev, c, nullptr, m);
        // only the k solved columns are written back (padding columns are never touched by the reference)
        std::vector<real_t> tmp((size_t)m * lda);
        dA.download(tmp.data(), (size_t)m * lda, dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        for (int r = 0; r < m; r++) memcpy(A + (size_t)r * lda, tmp.data() + (size_t)r * lda, (size_t)k * sizeof(real_t));
        return rc;
    });
}

// (cmfrec_hip_topN_batch and the ranking handle: topn_tu.hip)

// ---- the reference's stand-alone entry points for the prediction matrices and the ranking, under their own names and with
// ---- their own signatures (round 6; src/cmfrec.h:1922-1960, :2104-2127) ------------------------------------------------------
// Host buffers in and out like the fit entry points.  The Gramians run on the library's MFMA kernels, the solves with many
// right-hand sides on the row Cholesky kernel (CHOL_PREFILLED), the factorisation of the small block matrix on potrf_upper_kernel.
// Like the reference (syrk / potrf with one triangle referenced, src/collective.c:10345-10470) the symmetric outputs carry their
// UPPER triangle (row-major), the strictly lower part is zero.
static void zero_strictly_lower(real_t *M, int n)
{
    if (M == nullptr) return;
    for (int i = 1; i < n; i++) for (int j = 0; j < i; j++) M[(size_t)i * n + j] = 0;
}
// out[kd, kd] = scale * X[:, :kd]^T X[:, :kd] over `rows` rows (X on the host, leading dimension ldx, first used column at X)
static void host_gram(const DeviceInfo &dev, GramWorkspace &gws, const real_t *X, size_t ldx, int rows, int kd, real_t scale, DevBuf<real_t> &dX,
                      DevBuf<real_t> &out)
{
    dX.upload(X, (size_t)rows * ldx, dev.stream);
    out.alloc_at_least((size_t)kd * kd);
    launch_gram(dev, gws, dX.ptr, ldx, rows, kd, out.ptr, scale, (real_t)0);
}

int_t precompute_collective_implicit(
    real_t *B, int_t n, real_t *C, int_t p, real_t *U_colmeans, bool NA_as_zero_U,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t w_main, real_t w_user, real_t w_main_multiplier,
    bool nonneg, bool extra_precision,
    real_t *BtB, real_t *BeTBe, real_t *BeTBeChol, real_t *CtUbias)
{
    (void)extra_precision;                                  // (the two summation orders of the reference; one here)
    return guarded([&]() {
        if (B == nullptr || BtB == nullptr || n <= 0 || k + k_main <= 0) { g_last_error = "precompute_collective_implicit: B, BtB and n > 0 are required"; return 2; }
        if (p > 0 && (C == nullptr || BeTBe == nullptr)) { g_last_error = "precompute_collective_implicit: p > 0 needs C and BeTBe"; return 2; }
        if (w_main_multiplier != (real_t)1) w_main *= w_main_multiplier;       // collective.c:10501-10507
        if (w_main != (real_t)1) { lam /= w_main; w_user /= w_main; }
        DeviceInfo dev;
        init_device(dev, -1);
        GramWorkspace gws;
        hipStream_t st = dev.stream;
        const int kk = k + k_main, ktB = k_item + kk, kc = k_user + k, kq = k_user + kk;
        DevBuf<real_t> dB, dC, G, CtC, M;
        dB.upload(B, (size_t)n * ktB, st);
        G.alloc((size_t)kk * kk);
        launch_gram(dev, gws, dB.ptr + k_item, (size_t)ktB, n, kk, G.ptr, (real_t)1, lam);      // B^T B + lam I (:10509-10515)
        G.download(BtB, (size_t)kk * kk, st);
        if (p > 0) {
            host_gram(dev, gws, C, (size_t)kc, p, kc, w_user, dC, CtC);                            // w C^T C (:10523-10543)
            M.alloc((size_t)kq * kq);
            HIP_CHECK(hipMemsetAsync(M.ptr, 0, (size_t)kq * kq * sizeof(real_t), st));
            hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kk * kk), dim3(256), 0, st, G.ptr, kk, (real_t)1, M.ptr, kq, k_user);
            hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kc * kc), dim3(256), 0, st, CtC.ptr, kc, (real_t)1, M.ptr, kq, 0);
            if (k_user) hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(k_user), dim3(256), 0, st, M.ptr, kq, 0, k_user, lam);   // :10545-10546
            M.download(BeTBe, (size_t)kq * kq, st);
            if (BeTBeChol != nullptr && !nonneg) {                                                 // :10548-10555
                hipLaunchKernelGGL(potrf_upper_kernel<real_t>, dim3(1), dim3(256), 0, st, M.ptr, kq);
                M.download(BeTBeChol, (size_t)kq * kq, st);
            }
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        zero_strictly_lower(BtB, kk);
        if (p > 0) {
            zero_strictly_lower(BeTBe, kq);
            if (BeTBeChol != nullptr && !nonneg) zero_strictly_lower(BeTBeChol, kq);
            if (C != nullptr && CtUbias != nullptr && U_colmeans != nullptr && NA_as_zero_U)       // :10557-10564
                for (int f = 0; f < kc; f++) {
                    double acc = 0;
                    for (int_t j = 0; j < p; j++) acc += (double)C[(size_t)j * kc + f] * (double)U_colmeans[j];
                    CtUbias[f] = (real_t)(-(double)w_user * acc);
                }
        }
        return 0;
    });
}

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
    real_t *BtB, real_t *TransBtBinvBt, real_t *BtXbias, real_t *BeTBeChol, real_t *BiTBi,
    real_t *TransCtCinvCt, real_t *CtCw, real_t *CtUbias)
{
    return guarded([&]() {
        if (B == nullptr || n <= 0) { g_last_error = "precompute_collective_explicit: B and n > 0 are required"; return 2; }
        if (user_bias && B_plus_bias == nullptr) { g_last_error = "precompute_collective_explicit: user_bias needs the B_plus_bias buffer"; return 2; }
        if ((TransBtBinvBt != nullptr || BeTBeChol != nullptr || (Bi != nullptr && add_implicit_features)) && BtB == nullptr) {
            g_last_error = "precompute_collective_explicit: the matrices derived from BtB need the BtB buffer";
            return 2;
        }
        if (n_max == 0) n_max = n;                                                 // collective.c:10240-10241
        if (include_all_X) n = n_max;
        const int k_main_i = k_main;
        real_t lam_last = lam;
        if (lam_unique != nullptr) { lam_last = lam_unique[user_bias ? 0 : 2]; lam = lam_unique[2]; }    // :10245-10249
        if (w_main != (real_t)1) { lam /= w_main; lam_last /= w_main; w_user /= w_main; w_implicit /= w_main; }
        real_t lam_B = lam, lam_last_B = lam_last, lam_C = lam;
        if (scale_lam || scale_lam_sideinfo) {                                      // :10263-10277
            const real_t multiplier = (real_t)(n + (scale_lam_sideinfo ? p : 0));
            lam *= multiplier;
            lam_C *= (real_t)p;
            lam_last *= scale_bias_const ? scaling_biasA : multiplier;
            lam_B = lam; lam_last_B = lam_last;
        }
        const int ktB0 = k_item + k + k_main;
        const real_t *Bh = B;
        if (user_bias) {                                                            // append_ones_last_col, :10279-10300
            for (int_t c = 0; c < n_max; c++) {
                memcpy(B_plus_bias + (size_t)c * (ktB0 + 1), B + (size_t)c * ktB0, (size_t)ktB0 * sizeof(real_t));
                B_plus_bias[(size_t)c * (ktB0 + 1) + ktB0] = 1;
            }
            k_main++;
            Bh = B_plus_bias;
        }
        const int kk = k + k_main, ktB = k_item + kk, kc = k_user + k, kq = k_user + kk, kki = k + k_main_i;
        if (NA_as_zero_X && BtXbias != nullptr) {                                   // :10302-10342
            std::vector<double> acc((size_t)kk, 0.);
            if (n_max > n && glob_mean != (real_t)0)
                for (int_t c = n; c < n_max; c++) for (int f = 0; f < kk; f++) acc[f] -= (double)glob_mean * (double)Bh[(size_t)c * ktB + k_item + f];
            if (biasB != nullptr || glob_mean != (real_t)0)
                for (int_t c = 0; c < n; c++) {
                    const double coef = -((biasB != nullptr ? (double)biasB[c] : 0.) + (double)glob_mean);
                    for (int f = 0; f < kk; f++) acc[f] += coef * (double)Bh[(size_t)c * ktB + k_item + f];
                }
            for (int f = 0; f < kk; f++) BtXbias[f] = (real_t)acc[f];
        }
        DeviceInfo dev;
        init_device(dev, -1);
        GramWorkspace gws;
        hipStream_t st = dev.stream;
        DevBuf<real_t> dB, dBi, dC, G, Gi, CtC, M, Bp, Cc;
        if (BtB != nullptr) {                                                       // :10344-10351
            dB.upload(Bh, (size_t)n_max * ktB, st);
            G.alloc((size_t)kk * kk);
            launch_gram(dev, gws, dB.ptr + k_item, (size_t)ktB, n, kk, G.ptr, (real_t)1, (real_t)0);
            G.download(BtB, (size_t)kk * kk, st);
        }
        const bool with_bi = Bi != nullptr && add_implicit_features;
        if (with_bi) {                                                              // :10353-10360
            if (BiTBi == nullptr) { g_last_error = "precompute_collective_explicit: add_implicit_features needs the BiTBi buffer"; return 2; }
            host_gram(dev, gws, Bi, (size_t)kki, n, kki, w_implicit, dBi, Gi);
            Gi.download(BiTBi, (size_t)kki * kki, st);
        }
        if (TransBtBinvBt != nullptr && !nonneg && !add_implicit_features) {        // :10362-10386
            M.alloc((size_t)kk * kk); Bp.alloc((size_t)n * kk);
            HIP_CHECK(hipMemcpyAsync(M.ptr, G.ptr, (size_t)kk * kk * sizeof(real_t), hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(kk), dim3(256), 0, st, M.ptr, kk, 0, kk - 1, lam_B);
            hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(1), dim3(256), 0, st, M.ptr, kk, kk - 1, kk, lam_last_B);
            hipLaunchKernelGGL(copy_mat_kernel<real_t>, grid1d((size_t)n * kk), dim3(256), 0, st, dB.ptr + k_item, (size_t)ktB, Bp.ptr, (size_t)kk, (size_t)n, kk);
            CholCall c{Bp.ptr, (size_t)kk, nullptr, 0, kk, 0, nullptr, M.ptr, 0, 0, 0, 0, 0, false, false, false, CHOL_PREFILLED};
            const int rc = launch_chol(dev, c, nullptr, n);
            if (rc) return rc;
            Bp.download(TransBtBinvBt, (size_t)n * kk, st);
        }
        const bool with_c = p > 0 && C != nullptr;
        if (with_c && CtCw != nullptr) {                                            // :10388-10421
            host_gram(dev, gws, C, (size_t)kc, p, kc, (real_t)1, dC, CtC);
            if (TransCtCinvCt != nullptr && !add_implicit_features && !nonneg) {
                M.alloc((size_t)kc * kc); Cc.alloc((size_t)p * kc);
                HIP_CHECK(hipMemcpyAsync(M.ptr, CtC.ptr, (size_t)kc * kc * sizeof(real_t), hipMemcpyDeviceToDevice, st));
                HIP_CHECK(hipMemcpyAsync(Cc.ptr, dC.ptr, (size_t)p * kc * sizeof(real_t), hipMemcpyDeviceToDevice, st));
                hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(kc), dim3(256), 0, st, M.ptr, kc, 0, kc, lam_C / w_user);
                CholCall c{Cc.ptr, (size_t)kc, nullptr, 0, kc, 0, nullptr, M.ptr, 0, 0, 0, 0, 0, false, false, false, CHOL_PREFILLED};
                const int rc = launch_chol(dev, c, nullptr, p);
                if (rc) return rc;
                Cc.download(TransCtCinvCt, (size_t)p * kc, st);
            }
            if (w_user != (real_t)1) {                                              // :10419-10420 (in place, stays on the device for the block matrix)
                DevBuf<real_t> T1;
                T1.alloc((size_t)kc * kc);
                HIP_CHECK(hipMemsetAsync(T1.ptr, 0, (size_t)kc * kc * sizeof(real_t), st));
                hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kc * kc), dim3(256), 0, st, CtC.ptr, kc, w_user, T1.ptr, kc, 0);
                HIP_CHECK(hipMemcpyAsync(CtC.ptr, T1.ptr, (size_t)kc * kc * sizeof(real_t), hipMemcpyDeviceToDevice, st));
                HIP_CHECK(hipStreamSynchronize(st));
            }
            CtC.download(CtCw, (size_t)kc * kc, st);
        }
        if (BeTBeChol != nullptr && (C != nullptr || add_implicit_features) && !nonneg) {      // :10423-10461
            M.alloc((size_t)kq * kq);
            HIP_CHECK(hipMemsetAsync(M.ptr, 0, (size_t)kq * kq * sizeof(real_t), st));
            hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kk * kk), dim3(256), 0, st, G.ptr, kk, (real_t)1, M.ptr, kq, k_user);
            if (with_c && CtCw != nullptr)
                hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kc * kc), dim3(256), 0, st, CtC.ptr, kc, (real_t)1, M.ptr, kq, 0);
            else if (with_c) {
                host_gram(dev, gws, C, (size_t)kc, p, kc, w_user, dC, CtC);
                hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kc * kc), dim3(256), 0, st, CtC.ptr, kc, (real_t)1, M.ptr, kq, 0);
            }
            if (with_bi) hipLaunchKernelGGL(add_block_kernel<real_t>, grid1d((size_t)kki * kki), dim3(256), 0, st, Gi.ptr, kki, (real_t)1, M.ptr, kq, k_user);
            hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(kq), dim3(256), 0, st, M.ptr, kq, 0, kq - 1, lam);           // add_to_diag2
            hipLaunchKernelGGL(add_diag_kernel<real_t>, grid1d(1), dim3(256), 0, st, M.ptr, kq, kq - 1, kq, lam_last);
            hipLaunchKernelGGL(potrf_upper_kernel<real_t>, dim3(1), dim3(256), 0, st, M.ptr, kq);
            M.download(BeTBeChol, (size_t)kq * kq, st);
        }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
        zero_strictly_lower(BtB, kk);
        if (with_bi) zero_strictly_lower(BiTBi, kki);
        if (with_c && CtCw != nullptr) zero_strictly_lower(CtCw, kc);
        if (BeTBeChol != nullptr && (C != nullptr || add_implicit_features) && !nonneg) zero_strictly_lower(BeTBeChol, kq);
        if (C != nullptr && CtUbias != nullptr && p > 0 && U_colmeans != nullptr && NA_as_zero_U)      // :10463-10470
            for (int f = 0; f < kc; f++) {
                double acc = 0;
                for (int_t j = 0; j < p; j++) acc += (double)C[(size_t)j * kc + f] * (double)U_colmeans[j];
                CtUbias[f] = (real_t)(-(double)w_user * acc);
            }
        return 0;
    });
}

// topN (src/common.c:5127-5380) for one user: scores of the candidate items on the device (one thread per item), a stable radix
// sort by descending score (rocPRIM; ties: the earlier candidate, i.e. the lower item id without an include list), the first n_top.
static int topn_one_user(const real_t *a_vec, int_t k_user, const real_t *B, int_t k_item, const real_t *biasB, real_t glob_mean, real_t biasA,
                         int_t k, int_t k_main, int_t *include_ix, int_t n_include, int_t *exclude_ix, int_t n_exclude, int_t *outp_ix,
                         real_t *outp_score, int_t n_top, int_t n)
{
    auto bad = [&](const char *msg) { g_last_error = msg; fprintf(stderr, "%s\n", msg); return 2; };
    if (a_vec == nullptr || B == nullptr || outp_ix == nullptr) return bad("topN: a_vec, B and outp_ix are required");
    if (include_ix != nullptr && exclude_ix != nullptr) return bad("Cannot pass both 'include_ix' and 'exclude_ix'.");
    if (n_top <= 0) return bad("'n_top' must be greater than zero.");
    if (exclude_ix != nullptr && n_exclude > n - n_top) return bad("Number of rankeable entities is less than 'n_top'");
    if (include_ix != nullptr && n_include > n) return bad("Number of entities to include is larger than 'n'.");
    if (include_ix != nullptr) for (int_t i = 0; i < n_include; i++) if (include_ix[i] < 0 || include_ix[i] >= n) return bad("'include_ix' contains invalid entries");
    if (exclude_ix != nullptr) for (int_t i = 0; i < n_exclude; i++) if (exclude_ix[i] < 0 || exclude_ix[i] >= n) return bad("'exclude_ix' contains invalid entries");
    for (int_t f = 0; f < k_user + k + k_main; f++) if (std::isnan((double)a_vec[f])) return bad("The latent factors contain NAN values");
    if (std::isnan((double)biasA)) return bad("The bias is a NAN value");
    const int k_pred = k + k_main, ktB = k_item + k + k_main;
    std::vector<int> cand;
    if (include_ix != nullptr) cand.assign(include_ix, include_ix + n_include);
    else {
        std::vector<char> out((size_t)n, 0);
        if (exclude_ix != nullptr) for (int_t i = 0; i < n_exclude; i++) out[(size_t)exclude_ix[i]] = 1;
        cand.reserve((size_t)n);
        for (int_t i = 0; i < n; i++) if (!out[(size_t)i]) cand.push_back((int)i);
    }
    const int ncand = (int)cand.size();
    if (ncand < n_top) return bad("Number of rankeable entities is less than 'n_top'");
    DeviceInfo dev;
    init_device(dev, -1);
    hipStream_t st = dev.stream;
    DevBuf<real_t> da, dB, dbias, sc_in, sc_out;
    DevBuf<int> id_in, id_out;
    DevBuf<unsigned char> tmp;
    da.upload(a_vec + k_user, (size_t)k_pred, st);
    dB.upload(B, (size_t)n * ktB, st);
    if (biasB != nullptr) dbias.upload(biasB, (size_t)n, st);
    id_in.upload(cand.data(), (size_t)ncand, st);
    sc_in.alloc((size_t)ncand); sc_out.alloc((size_t)ncand); id_out.alloc((size_t)ncand);
    hipLaunchKernelGGL(topn_one_user_scores_kernel<real_t>, grid1d((size_t)ncand), dim3(256), 0, st, da.ptr, k_pred, dB.ptr + k_item, (size_t)ktB,
                       biasB != nullptr ? dbias.ptr : nullptr, id_in.ptr, ncand, sc_in.ptr);
    HIP_CHECK(hipGetLastError());
    size_t bytes = 0;
    HIP_CHECK(rocprim::radix_sort_pairs_desc(nullptr, bytes, sc_in.ptr, sc_out.ptr, id_in.ptr, id_out.ptr, (size_t)ncand, 0, 8 * sizeof(real_t), st));
    tmp.alloc(std::max<size_t>(bytes, 1));
    HIP_CHECK(rocprim::radix_sort_pairs_desc(tmp.ptr, bytes, sc_in.ptr, sc_out.ptr, id_in.ptr, id_out.ptr, (size_t)ncand, 0, 8 * sizeof(real_t), st));
    std::vector<real_t> hs((size_t)n_top);
    std::vector<int> hi((size_t)n_top);
    id_out.download(hi.data(), (size_t)n_top, st);
    sc_out.download(hs.data(), (size_t)n_top, st);
    HIP_CHECK(hipStreamSynchronize(st));
    for (int_t i = 0; i < n_top; i++) {
        outp_ix[i] = hi[(size_t)i];
        if (outp_score != nullptr) outp_score[i] = hs[(size_t)i] + (glob_mean + biasA);          // common.c:5349-5358
    }
    return 0;
}

int_t topN_old_collective_explicit(
    real_t *a_vec, real_t a_bias, real_t *A, real_t *biasA, int_t row_index, real_t *B, real_t *biasB, real_t glob_mean,
    int_t k, int_t k_user, int_t k_item, int_t k_main, int_t *include_ix, int_t n_include, int_t *exclude_ix, int_t n_exclude,
    int_t *outp_ix, real_t *outp_score, int_t n_top, int_t n, int_t n_max, bool include_all_X, int nthreads)
{
    (void)nthreads;
    return guarded([&]() {
        if (include_all_X || n == 0) n = n_max;                                                   // collective.c:11560-11561
        if (a_vec != nullptr)
            return topn_one_user(a_vec, k_user, B, k_item, biasB, glob_mean, a_bias, k, k_main, include_ix, n_include, exclude_ix, n_exclude, outp_ix, outp_score, n_top, n);
        if (A == nullptr) { g_last_error = "topN_old_collective_explicit: a_vec or A is required"; return 2; }
        return topn_one_user(A + (size_t)row_index * (size_t)(k_user + k + k_main), k_user, B, k_item, biasB, glob_mean,
                             biasA == nullptr ? (real_t)0 : biasA[row_index], k, k_main, include_ix, n_include, exclude_ix, n_exclude, outp_ix,
                             outp_score, n_top, n);
    });
}

int_t topN_old_collective_implicit(
    real_t *a_vec, real_t *A, int_t row_index, real_t *B, int_t k, int_t k_user, int_t k_item, int_t k_main,
    int_t *include_ix, int_t n_include, int_t *exclude_ix, int_t n_exclude, int_t *outp_ix, real_t *outp_score, int_t n_top, int_t n, int nthreads)
{
    return topN_old_collective_explicit(a_vec, (real_t)0, A, nullptr, row_index, B, nullptr, (real_t)0, k, k_user, k_item, k_main, include_ix, n_include,
                                        exclude_ix, n_exclude, outp_ix, outp_score, n_top, n, n, false, nthreads);
}

int cmfrec_hip_optimizeA_collective(real_t *A, size_t lda, const real_t *B, size_t ldb, const real_t *C, int_t m,
                                    int_t m_u, int_t n, int_t p, int_t k, int_t k_main, int_t k_user, int_t k_item,
                                    const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
                                    const real_t *bias_sub, const real_t *U, real_t lam, real_t w_user,
                                    real_t lam_last, bool scale_lam, bool scale_lam_sideinfo)
{
    return guarded([&]() {
        if (m_u > m) { g_last_error = "cmfrec_hip: m_u > m is not supported"; return 2; }
        DeviceInfo dev;
        init_device(dev, -1);
        const int kc = k_user + k, kt = k_user + k + k_main;
        DevBuf<real_t> dA, dB, dC, dU, dG, dbias;
        GramWorkspace gws;
        SparseShard X;
        dA.upload(A, (size_t)m * lda, dev.stream);
        dB.upload(B, (size_t)n * ldb, dev.stream);
        dC.upload(C, (size_t)p * kc, dev.stream);
        dU.upload(U, (size_t)m_u * p, dev.stream);
        if (bias_sub) dbias.upload(bias_sub, n, dev.stream);
        dG.alloc((size_t)kc * kc);
        X.opp_row_bytes_hint = (size_t)k * sizeof(real_t);
        shard_from_csr(X, m, Xcsr_p, Xcsr_i, Xcsr, n, dev.stream);
        launch_gram(dev, gws, dC.ptr, (size_t)kc, p, kc, dG.ptr, w_user, (real_t)0);
        // collective.c:4817-4822 zeroes max(m,m_u)*lda - (lda-k_totA) elements
        HIP_CHECK(hipMemsetAsync(dA.ptr, 0, ((size_t)m * lda - (lda - (size_t)kt)) * sizeof(real_t), dev.stream));
        launch_gemm<false>(dev, m_u, kc, p, w_user, dU.ptr, (size_t)p, dC.ptr, (size_t)kc, dA.ptr, lda);
        CholCall c{dA.ptr, lda, dB.ptr + k_item, ldb, kt, k_user, bias_sub ? dbias.ptr : nullptr, dG.ptr, kc, m_u, p,
                   lam, lam_last, (bool)(scale_lam || scale_lam_sideinfo), scale_lam_sideinfo, false, CHOL_COLLECTIVE};
        LowRankScratch lrs;
        int rc = (m_u >= m) ? launch_collective_lowrank(dev, lrs, c, X, dC.ptr, SideOperand{dU.ptr}, p, w_user, k, n) : -1;
        if (rc < 0) rc = launch_chol(dev, c, &X);
        dA.download(A, (size_t)m * lda, dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        return rc;
    });
}

// Collective half-step with SPARSE side information (U given as CSR over the m_u rows that have any): the branches of
// collective_closed_form_block (collective.c:1223-1847) / collective_closed_form_block_implicit (:1849-2131) with
// u_vec == NULL, u_vec_sp != NULL, !NA_as_zero_U: the row's present attributes add  w * C_j C_j^T  to the upper-left
// [k_user+k]^2 block (:1636-1653, :2003-2011) and  w * u_j C_j  to the right-hand side (:1719-1731, :2013-2021); under
// scale_lam_sideinfo lambda is also multiplied by their number (:1338-1346).  Both gathers -- rows of B through X, rows of
// C through U -- run through the same staging ring and matrix-core rank-1 updates of one kernel launch.
int cmfrec_hip_optimizeA_collective_sparse(real_t *A, size_t lda, const real_t *B, size_t ldb, const real_t *C, int_t m,
                                           int_t m_u, int_t n, int_t p, int_t k, int_t k_main, int_t k_user, int_t k_item,
                                           const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
                                           const real_t *bias_sub, const size_t Ucsr_p[], const int_t Ucsr_i[],
                                           const real_t *Ucsr, real_t lam, real_t w_user, real_t lam_last, bool scale_lam,
                                           bool scale_lam_sideinfo, bool implicit)
{
    return guarded([&]() {
        if (m_u > m) { g_last_error = "cmfrec_hip: m_u > m is not supported here"; return 2; }
        DeviceInfo dev;
        init_device(dev, -1);
        const int kc = k_user + k, kk = k + k_main, kt = k_user + kk;
        DevBuf<real_t> dA, dB, dC, dG, dM, dbias;
        GramWorkspace gws;
        SparseShard X, Us;
        dA.alloc((size_t)m * lda);
        HIP_CHECK(hipMemsetAsync(dA.ptr, 0, dA.n * sizeof(real_t), dev.stream));          // collective.c:4817-4822, :6018-6019
        dB.upload(B, (size_t)n * ldb, dev.stream);
        dC.upload(C, (size_t)p * kc, dev.stream);
        if (bias_sub) dbias.upload(bias_sub, n, dev.stream);
        X.opp_row_bytes_hint = (size_t)k * sizeof(real_t);
        shard_from_csr(X, m, Xcsr_p, Xcsr_i, Xcsr, n, dev.stream);
        std::vector<size_t> up((size_t)m + 1);
        for (int r = 0; r <= m; r++) up[r] = Ucsr_p[std::min(r, m_u)];
        shard_from_csr(Us, m, up.data(), Ucsr_i, Ucsr, p, dev.stream);
        int rc;
        if (implicit) {
            dG.alloc((size_t)kk * kk); dM.alloc((size_t)kt * kt);
            launch_gram(dev, gws, dB.ptr + k_item, ldb, n, kk, dG.ptr, (real_t)1, lam);
            hipLaunchKernelGGL(betbe_base_kernel<real_t>, grid1d((size_t)kt * kt), dim3(256), 0, dev.stream, dG.ptr, kk, k_user, lam,
                               dM.ptr);
            CholCall c{dA.ptr, lda, dB.ptr + k_item, ldb, kt, k_user, nullptr, nullptr, kc, m_u, p, lam, lam, false, false, false,
                       CHOL_COLLECTIVE_IMPLICIT, dM.ptr};
            c.X2 = &Us; c.B2 = dC.ptr; c.ldb2 = (size_t)kc; c.kc2 = kc; c.w2 = w_user;
            rc = launch_chol(dev, c, &X);
        } else {
            CholCall c{dA.ptr, lda, dB.ptr + k_item, ldb, kt, k_user, bias_sub ? dbias.ptr : nullptr, nullptr, kc, m_u, p, lam,
                       lam_last, (bool)(scale_lam || scale_lam_sideinfo), scale_lam_sideinfo, false, CHOL_COLLECTIVE};
            c.X2 = &Us; c.B2 = dC.ptr; c.ldb2 = (size_t)kc; c.kc2 = kc; c.w2 = w_user;
            rc = launch_chol(dev, c, &X);
        }
        std::vector<real_t> tmp((size_t)m * lda);
        dA.download(tmp.data(), (size_t)m * lda, dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        for (int r = 0; r < m; r++) memcpy(A + (size_t)r * lda, tmp.data() + (size_t)r * lda, (size_t)kt * sizeof(real_t));
        return rc;
    });
}

// what cmfrec_hip_factors_multiple_ex adds to the arguments of cmfrec_hip_factors_multiple_l1 (include/cmfrec_hip.h)
struct NewRowsExtra {
    const real_t *weight = nullptr;            // sparse X: one per entry, in the order of the triplets / of Xcsr
    const real_t *Xfull = nullptr;             // [m_x, n], NaN = not observed
    const real_t *weight_full = nullptr;       // [m_x, n], read where Xfull is present
    real_t glob_mean_full = 0;                 // subtracted from the present entries of Xfull on the device
    const real_t *Bi = nullptr;                // [n, k + k_main]
    real_t w_implicit = 1, w_implicit_gram = 1;
    const real_t *BiTBi_pre = nullptr;         // [k + k_main]^2, w_implicit_gram included
    const real_t *TransBtBinvBt_pre = nullptr; // [n, k + k_main (+ 1 with a bias)]
};

// Factors of rows that were not part of the fit, all of them in one pass (the step after the path):
// factors_collective_explicit_multiple (collective.c:10865-11174) / factors_collective_implicit_multiple
// (:11176-11340) restricted to sparse X (COO or CSR, values already transformed: minus the global mean, times
// alpha) and dense side information without missing values.  Per row (collective_factors_warm :3555-3964,
// collective_factors_cold :3309-3440, the *_implicit twins :3442-3553, :3966-4087) this is the closed-form row
// update of the fit with B (and C) fixed:
//   explicit, no U:       factors_closed_form on [B | 1]            -> Cholesky mode EXPLICIT
//   explicit, U, nnz > 0: collective_closed_form_block              -> mode COLLECTIVE
//   explicit, U, nnz = 0: "cold" (C^T C + (lam/w)(p if scale_lam_sideinfo) I)^-1 C^T u, bias 0; the last of the
//                         k_user+k unknowns keeps the unscaled lam/w (scale_bias_const := scale_lam_sideinfo in the
//                         call at :3397-3411); with TransCtCinvCt given it is u^T TransCtCinvCt (:3380-3386)
//   implicit:             factors_implicit_chol / collective_closed_form_block_implicit -> modes IMPLICIT /
//                         COLLECTIVE_IMPLICIT; lam_x is what sits on the diagonal of the X block (the reference adds
//                         the *unscaled* lam there when it builds BtB itself, :11270-11280, and lam / w_main on the
//                         k_user block), BtB_pre (lam included) replaces B^T B + lam_x I when given.
// l1_lam / l1_lam_bias: the L1 penalty of the row systems and of the bias unknown (solve_elasticnet instead of the Cholesky
// substitution, common.c:2228-2294; collective_factors_warm / _cold hand them down like lam / lam_bias, collective.c:3571-3931,
// :3321-3400), already divided by w_main.  Rows that only have side information take l1_lam / w_user (:3395).
// The work is split in two (newrows.hpp): NewRowsState holds what belongs to the model -- the device copies of B (with its ones
// column), biasB, C, the column means, Bi, the Gramians and the precomputed matrices, the stream and the workspaces -- and is
// built once; newrows_state_run does what depends on the batch and leaves the factors on the device.  The three one-shot entry
// points below are "state made, one batch, state destroyed"; the handle of fit.hip (cmfrec_hip_newrows_*) keeps the state.
}  // extern "C"

namespace cmfhip {

struct NewRowsState {
    DeviceInfo dev;                            // (first: its stream outlives the buffers below)
    GramWorkspace gws;
    NewRowsModelArgs M;                        // the scalars; the host pointers are not read after create
    int ub = 0, kc = 0, kk = 0, kt = 0, ktA = 0, kT = 0;
    size_t ldB = 0, ldA = 0;
    bool l1on = false, have_C = false, have_means = false, have_Bi = false, have_T = false, have_TB = false;
    // model side, built once (w_user C^T C and the matrix of the rows without observations: on the first batch that needs them)
    DevBuf<real_t> dB, dbias, dC, dmeans, dG, dM, dCtC, dMcold, dT, dTB, dBi, dBiG, dBiFull;
    bool ctc_built = false, cold_built = false;
    // batch side: reused from call to call, grown on demand (the shards are rebuilt: their layout belongs to the batch)
    DevBuf<real_t> dA, dU, dcold, dTBout, dba, dXb, dWb;
    DevBuf<int> dmiss;
    std::unique_ptr<SparseShard> Xs, Us;
    int rows = 0;                              // rows of the last batch, 0: none yet
    // exclusion lists of the last batch's rows for the ranking kernels (newrows_state_exclusions)
    DevBuf<size_t> ep, ep_in;
    DevBuf<int> ei, ei_in;
    DevBuf<unsigned char> sort_tmp;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the solve phase of the last batch
    bool timed = false;
    // imputation (newrows_state_impute): does dXb still hold the caller's whole batch (one block, not centred), the events around
    // a block's fill kernel and their sum over the blocks of the last impute call
    bool xb_resident = false;
    hipEvent_t ev2 = nullptr, ev3 = nullptr;
    double fill_ms = 0;
    // missing-as-zero models (newrows_run_naz): the padded operand copies of the right-hand-side kernel, B^T B with the ones column
    // and no diagonal, the constant rows [CtUbias | BtXbias] of the rows with / without side information -- built by create -- and
    // the shared matrices with their inverses, each built by the first batch that needs it
    struct NazInverse {
        DevBuf<real_t> M, R, Linv, Minv;
        int k = 0;
        bool built = false;
    };
    bool naz = false, naz_has_cst = false;
    int kx = 0;
    size_t ldBx = 0, ldCw = 0;
    DevBuf<real_t> dBx, dCw, dBtB, dc_side, dc_plain, dc_u;   // [kt] each: [CtUbias | BtXbias], [0 | BtXbias], [CtUbias | 0]
    int naz_last_waves = 0;
    NazInverse inv_side, inv_plain, inv_cold;
    real_t inv_side_mult = 0;                  // the lambda multiplier inv_side was built with (dense U under scale_lam_sideinfo: n + p)
    DevBuf<real_t> drhs, dtmp, dres, dg, dz, dpart, dUC, dcold2;
    DevBuf<NazTask> dtasks;
    DevBuf<NazFinishRow> dfin;
    std::vector<NazTask> tasks;
    std::vector<NazFinishRow> fin;
    ~NewRowsState()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (ev2) (void)hipEventDestroy(ev2);
        if (ev3) (void)hipEventDestroy(ev3);
    }
};

// rows per device block of a dense batch: its device copy (and the weights') stays within 1 GB
static long long newrows_block_rows(int n, bool weighted, int m_x)
{
    const size_t per_row = (size_t)n * sizeof(real_t) * (weighted ? 2 : 1);
    long long block_rows = (long long)std::max<size_t>(1, ((size_t)1 << 30) / std::max<size_t>(per_row, 1));
    if (switches().newrows_block_rows > 0) block_rows = switches().newrows_block_rows;     // test hook
    return std::min<long long>(block_rows, m_x);
}

// the three refusals about the form of X and its weights, in front of everything else (a batch without rows included)
static int newrows_form_check(bool implicit, bool Bi, const NewRowsBatchArgs &bt)
{
    auto bad = [](const char *what) { g_last_error = std::string("cmfrec_hip_factors_multiple: ") + what; return 2; };
    if (implicit && (bt.weight || bt.Xfull || bt.weight_full || Bi)) return bad("observation weights, dense X and implicit features belong to the explicit model");
    if (bt.Xfull && (bt.nnz > 0 || bt.Xcsr_p)) return bad("X given both as a dense and as a sparse matrix");
    if ((bt.weight_full && !bt.Xfull) || (bt.weight && bt.Xfull)) return bad("the weights must have the form of X (weight with sparse X, weight_full with Xfull)");
    return 0;
}

// ---- missing-as-zero models: NA_as_zero_X / NA_as_zero_U of a batch of new rows -----------------------
// Per row, with every one of the n cells counted (an absent one a zero of weight 1, its target -glob_mean - biasB_j) and an
// absent attribute of a sparse U a zero minus its column mean:
//     M   = blockdiag(0, B~^T B~) + w_user C^T C + diag(lam mult)          B~ = [B | 1] with a user bias
//     rhs = [CtUbias | BtXbias] + sum_X coef_j B~_j (+) sum_U u_c w_user C_c,   BtXbias = -sum_all (glob_mean + biasB_j) B~_j,
//     CtUbias = -w_user C^T colmeans
// Without observation weights M is the same for every row: the batch is newrows_naz_kernels.hpp's gather-sum and one product
// with the inverse the model keeps.  With weights a row adds sum_obs (w_j - 1) b_j b_j^T: the row Cholesky kernel on the base B~^T B~.
// The model side, once per handle: the padded copies, B~^T B~, the constants.
static void newrows_naz_model_side(NewRowsState &S)
{
    const NewRowsModelArgs &M = S.M;
    DeviceInfo &dev = S.dev;
    hipStream_t st = dev.stream;
    const int ub = S.ub, kk = S.kk, kc = S.kc, kt = S.kt, n = M.n, kx = kk + ub;
    S.naz = true; S.kx = kx;
    S.ldBx = naz_padded_ld<real_t>(kx);
    S.dBx.alloc((size_t)n * S.ldBx);
    naz_launch_pad_rows(st, S.dB.ptr, S.ldB, M.k_item, kk, (real_t)1, ub ? kk : -1, S.dBx.ptr, S.ldBx, (size_t)n);
    if (S.have_C) {
        S.ldCw = naz_padded_ld<real_t>(kc);
        S.dCw.alloc((size_t)M.p * S.ldCw);
        naz_launch_pad_rows(st, S.dC.ptr, (size_t)kc, 0, kc, M.w_user, -1, S.dCw.ptr, S.ldCw, (size_t)M.p);
    }
    S.dc_side.alloc((size_t)kt); S.dc_plain.alloc((size_t)kt); S.dc_u.alloc((size_t)kt);
    HIP_CHECK(hipMemsetAsync(S.dc_side.ptr, 0, (size_t)kt * sizeof(real_t), st));
    HIP_CHECK(hipMemsetAsync(S.dc_u.ptr, 0, (size_t)kt * sizeof(real_t), st));
    HIP_CHECK(hipMemsetAsync(S.dc_plain.ptr, 0, (size_t)kt * sizeof(real_t), st));
    if (M.NA_as_zero_X) {
        const real_t *Bx = S.dB.ptr + M.k_item;
        S.dBtB.alloc((size_t)kx * kx);
        launch_gram(dev, S.gws, Bx, S.ldB, n, kx, S.dBtB.ptr, (real_t)1, (real_t)0);
        // BtXbias: the items that carry a bias, then the items beyond them with the mean alone (include_all_X)
        S.naz_has_cst = M.glob_mean != (real_t)0 || S.dbias.ptr != nullptr;
        if (S.naz_has_cst) {
            const int n_b = std::max(0, std::min<int>(M.n_x > 0 ? M.n_x : n, n));
            const int nb1 = (n_b + COLSUM_ROWS - 1) / COLSUM_ROWS, nb2 = (n - n_b + COLSUM_ROWS - 1) / COLSUM_ROWS;
            DevBuf<real_t> part;
            part.alloc((size_t)std::max(nb1 + nb2, 1) * kx);
            if (nb1 > 0)
                hipLaunchKernelGGL(weighted_colsum_partial_kernel<real_t>, dim3(nb1), dim3(256), 0, st, Bx, S.ldB, n_b, kx, S.dbias.ptr, M.glob_mean,
                                   part.ptr);
            if (nb2 > 0)
                hipLaunchKernelGGL(weighted_colsum_partial_kernel<real_t>, dim3(nb2), dim3(256), 0, st, Bx + (size_t)n_b * S.ldB, S.ldB, n - n_b, kx,
                                   (const real_t *)nullptr, M.glob_mean, part.ptr + (size_t)nb1 * kx);
            hipLaunchKernelGGL(colsum_finish_kernel<real_t>, grid1d(kx), dim3(256), 0, st, part.ptr, nb1 + nb2, kx, (real_t)-1, S.dc_plain.ptr + M.k_user);
            HIP_CHECK(hipGetLastError());
            HIP_CHECK(hipMemcpyAsync(S.dc_side.ptr + M.k_user, S.dc_plain.ptr + M.k_user, (size_t)kx * sizeof(real_t), hipMemcpyDeviceToDevice, st));
            HIP_CHECK(hipStreamSynchronize(st));   // part goes away
        }
    }
    if (M.NA_as_zero_U && S.have_C && S.have_means) {
        // CtUbias = -w_user C^T colmeans, added onto the first k_user + k columns of the rows with side information
        DevBuf<real_t> ctu;
        ctu.alloc((size_t)kc);
        launch_gemm<false>(dev, 1, kc, M.p, -M.w_user, S.dmeans.ptr, (size_t)M.p, S.dC.ptr, (size_t)kc, ctu.ptr, (size_t)kc);
        hipLaunchKernelGGL(add_rowvec_kernel<real_t>, grid1d((size_t)kc), dim3(256), 0, st, S.dc_side.ptr, (size_t)kt, (size_t)1, kc, ctu.ptr);
        hipLaunchKernelGGL(add_rowvec_kernel<real_t>, grid1d((size_t)kc), dim3(256), 0, st, S.dc_u.ptr, (size_t)kt, (size_t)1, kc, ctu.ptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));
    }
}

// I.M [k, k] holds a symmetric positive definite matrix: its inverse through the library's own potrf / trtri, kept in I.Minv
static void newrows_naz_invert(DeviceInfo &dev, NewRowsState::NazInverse &I, int k)
{
    hipStream_t st = dev.stream;
    const size_t kk2 = (size_t)k * k;
    I.R.alloc(kk2); I.Linv.alloc(kk2); I.Minv.alloc(kk2);
    HIP_CHECK(hipMemcpyAsync(I.R.ptr, I.M.ptr, kk2 * sizeof(real_t), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(potrf_upper_kernel<real_t>, dim3(1), dim3(256), 0, st, I.R.ptr, k);
    HIP_CHECK(hipGetLastError());
    launch_trtri(dev, I.R.ptr, k, I.Linv.ptr);
    launch_gemm<true>(dev, k, k, k, (real_t)1, I.Linv.ptr, (size_t)k, I.Linv.ptr, (size_t)k, I.Minv.ptr, (size_t)k);
    I.k = k; I.built = true;
}

// out[rows, k] (ld = ldo) = rhs[rows, k] M^-1: the product with the explicit inverse and one step of refinement with the matrix
// itself, x1 = x0 + (b - x0 M) M^-1, which brings the error of the product (cond(M) eps) back to that of two triangular solves
static void newrows_naz_apply(NewRowsState &S, const NewRowsState::NazInverse &I, const real_t *rhs, size_t ldr, int rows, real_t *out, size_t ldo)
{
    if (rows <= 0) return;
    DeviceInfo &dev = S.dev;
    const int k = I.k;
    S.dtmp.alloc_at_least((size_t)rows * k); S.dres.alloc_at_least((size_t)rows * k);
    launch_gemm<false>(dev, rows, k, k, (real_t)1, rhs, ldr, I.Minv.ptr, (size_t)k, out, ldo);
    launch_gemm<false>(dev, rows, k, k, (real_t)1, out, ldo, I.M.ptr, (size_t)k, S.dres.ptr, (size_t)k);
    hipLaunchKernelGGL(residual_rows_kernel<real_t>, grid1d((size_t)rows * k), dim3(256), 0, dev.stream, S.dres.ptr, (size_t)k, rhs, ldr, (size_t)rows, k);
    launch_gemm<false>(dev, rows, k, k, (real_t)1, S.dres.ptr, (size_t)k, I.Minv.ptr, (size_t)k, S.dtmp.ptr, (size_t)k);
    hipLaunchKernelGGL(add_rows_kernel<real_t>, grid1d((size_t)rows * k), dim3(256), 0, dev.stream, out, ldo, S.dtmp.ptr, (size_t)k, (size_t)rows, k);
    HIP_CHECK(hipGetLastError());
}

// the task list of the right-hand-side kernel from the rows' lengths (host), uploaded into S.dtasks / S.dfin; returns the slots
static size_t newrows_naz_tasks(NewRowsState &S, int rows, const std::vector<size_t> *lenX, const std::vector<size_t> *lenU, int rows_u)
{
    S.tasks.clear(); S.fin.clear();
    size_t slots = 0;
    for (int r = 0; r < rows; r++) {
        const int nx = lenX ? (int)(((*lenX)[r] + NAZ_SEG - 1) / NAZ_SEG) : 0;
        const int nu = (lenU && r < rows_u) ? (int)(((*lenU)[r] + NAZ_SEG - 1) / NAZ_SEG) : 0;
        const int tot = nx + nu;
        if (tot == 0) continue;
        const bool direct = tot == 1;
        const int slot0 = (int)slots;
        for (int sg = 0; sg < nx; sg++) S.tasks.push_back(NazTask{r, direct ? 2 : 0, sg, slot0 + sg});
        for (int sg = 0; sg < nu; sg++) S.tasks.push_back(NazTask{r, 1 | (direct ? 2 : 0), sg, slot0 + nx + sg});
        if (!direct) { S.fin.push_back(NazFinishRow{r, slot0, nx, nu}); slots += (size_t)tot; }
    }
    hipStream_t st = S.dev.stream;
    if (!S.tasks.empty()) S.dtasks.upload(S.tasks.data(), S.tasks.size(), st);
    if (!S.fin.empty()) S.dfin.upload(S.fin.data(), S.fin.size(), st);
    return slots;
}

// The batch side.  Xs / Us: the shards newrows_state_run has built (Us: sparse U, or empty); lenX / lenU: the rows' lengths on the
// host; m_u / p: as newrows_state_run has reduced them (0 without side information in the batch); dense: dU holds the centred
// dense U.  naz_x: NA_as_zero_X applies to this batch (a sparse X).  Leaves the factors in S.dA.
static int newrows_run_naz(NewRowsState &S, SparseShard &Xs, SparseShard &Us, const std::vector<size_t> &lenX, const std::vector<size_t> &lenU,
                           int m_max, int m_u, int p, bool spU, bool naz_x)
{
    const NewRowsModelArgs &M = S.M;
    auto bad = [](const char *what) { g_last_error = std::string("cmfrec_hip_factors_multiple: ") + what; return 2; };
    DeviceInfo &dev = S.dev;
    hipStream_t st = dev.stream;
    const int ub = S.ub, kc = S.kc, kt = S.kt, kx = S.kx, k_user = M.k_user, n = M.n;
    const size_t ldA = S.ldA, ldB = S.ldB;
    const bool scaled = M.scale_lam || M.scale_lam_sideinfo;
    const real_t lam = M.lam, lam_bias = M.lam_bias;
    const int max_waves = switches().naz_waves;
    const bool side = p > 0 && m_u > 0;
    NazRhsParams<real_t> P;
    P.Bx = S.dBx.ptr; P.ldbx = S.ldBx; P.kx = kx; P.koff_x = k_user;
    P.biasB = S.dbias.ptr; P.glob_mean = M.glob_mean;
    // The constant of a row: BtXbias belongs to a sparse X under NA_as_zero_X, CtUbias to a sparse U under NA_as_zero_U -- a dense
    // U is centred before it is multiplied and knows no absent entry, and an ordinary X (or a dense Xfull) has no constant
    const bool ctu = spU && M.NA_as_zero_U;
    P.c_side = naz_x ? (ctu ? S.dc_side.ptr : S.dc_plain.ptr) : (ctu ? S.dc_u.ptr : nullptr);
    P.c_plain = naz_x ? S.dc_plain.ptr : nullptr;
    P.rows_side = side ? std::min(m_u, m_max) : 0;
    P.n_bias = (int)(M.n_x > 0 ? M.n_x : M.n);
    P.kt = kt; P.rows = m_max;
    P.gwidth = std::max(kx, S.have_C ? kc : 0);
    if (spU) { P.up = Us.p.ptr; P.ui = Us.i.ptr; P.uv = Us.v.ptr; P.Cw = S.dCw.ptr; P.ldcw = S.ldCw; P.kc = kc; }
    auto run_rhs = [&](bool with_x, real_t *rhs, size_t ld) {
        if (with_x) { P.xp = Xs.p.ptr; P.xi = Xs.i.ptr; P.xv = Xs.v.ptr; P.xw = Xs.weighted() ? Xs.w.ptr : nullptr; }
        const size_t slots = newrows_naz_tasks(S, m_max, with_x ? &lenX : nullptr, spU ? &lenU : nullptr, m_u);
        P.ldp = (size_t)std::max(kx, kc);
        S.dpart.alloc_at_least(std::max<size_t>(slots, 1) * P.ldp);
        P.partial = S.dpart.ptr;
        P.tasks = S.dtasks.ptr; P.ntasks = (int)S.tasks.size(); P.fin = S.dfin.ptr; P.nfin = (int)S.fin.size();
        P.rhs = rhs; P.ld = ld;
        poison_lds(st, dev.num_cus);              // test hook (the kernel has no LDS: nothing may depend on it)
        S.naz_last_waves = naz_launch_rhs(st, dev.num_cus, P, max_waves);
    };
    auto ensure_CtC = [&]() {
        if (S.ctc_built) return;
        S.dCtC.alloc((size_t)kc * kc);
        launch_gram(dev, S.gws, S.dC.ptr, (size_t)kc, p, kc, S.dCtC.ptr, M.w_user, (real_t)0);
        S.ctc_built = true;
    };
    if (!naz_x) {
        // NA_as_zero_U with an ordinary X: the rows with entries through the collective row solver with the shared w_user C^T C as
        // its side block and the right-hand sides of the side block from the kernel's second source + CtUbias; the rows without
        // any entry ("cold") share w_user C^T C + lam I
        ensure_CtC();
        run_rhs(false, S.dA.ptr, ldA);
        if (!S.inv_cold.built) {
            S.inv_cold.M.alloc((size_t)kc * kc);
            HIP_CHECK(hipMemcpyAsync(S.inv_cold.M.ptr, S.dCtC.ptr, (size_t)kc * kc * sizeof(real_t), hipMemcpyDeviceToDevice, st));
            hipLaunchKernelGGL(add_diag_kernel<real_t>, dim3((kc + 255) / 256), dim3(256), 0, st, S.inv_cold.M.ptr, kc, 0, kc, lam);
            newrows_naz_invert(dev, S.inv_cold, kc);
        }
        S.dcold.alloc_at_least((size_t)m_u * kc); S.dcold2.alloc_at_least((size_t)m_u * kc);
        HIP_CHECK(hipMemcpy2DAsync(S.dcold.ptr, (size_t)kc * sizeof(real_t), S.dA.ptr, ldA * sizeof(real_t), (size_t)kc * sizeof(real_t), (size_t)m_u,
                                   hipMemcpyDeviceToDevice, st));
        newrows_naz_apply(S, S.inv_cold, S.dcold.ptr, (size_t)kc, m_u, S.dcold2.ptr, (size_t)kc);
        CholCall c{S.dA.ptr, ldA, S.dB.ptr + M.k_item, ldB, kt, k_user, S.dbias.ptr, S.dCtC.ptr, kc, m_u, p, lam, lam_bias, M.scale_lam, false,
                   M.scale_bias_const, CHOL_COLLECTIVE};
        if (int rc = launch_chol(dev, c, &Xs)) return rc;
        hipLaunchKernelGGL(cold_select_kernel<real_t>, dim3(m_u), dim3(64), 0, st, S.dA.ptr, ldA, kt, kc, S.dcold2.ptr, Xs.p.ptr, m_u);
        HIP_CHECK(hipGetLastError());
        return 0;
    }
    if (Xs.weighted()) {
        // observation weights, no side information: every row's matrix is B~^T B~ + sum_obs (w_j - 1) b_j b_j^T + lam mult, mult =
        // sum of the row's weights + its absent cells.  The right-hand sides are the kernel's (its per-entry coefficients); the row
        // Cholesky kernel adds the corrections onto the base matrix and solves in place.
        if (side) return bad("NA_as_zero_X with observation weights together with side information is not supported");
        run_rhs(true, S.dA.ptr, ldA);
        S.dg.alloc_at_least(Xs.nnz); S.dz.alloc_at_least(Xs.nnz);
        naz_launch_weight_corrections(st, Xs.w.ptr, Xs.nnz, S.dg.ptr, S.dz.ptr);
        Xs.wsum_naz.alloc_at_least((size_t)m_max);
        hipLaunchKernelGGL(naz_wsum_kernel<real_t>, grid1d((size_t)m_max), dim3(256), 0, st, Xs.p.ptr, Xs.w.ptr, m_max, n, Xs.wsum_naz.ptr);
        HIP_CHECK(hipGetLastError());
        CholCall c{S.dA.ptr + k_user, ldA, S.dB.ptr + M.k_item, ldB, kx, 0, nullptr, S.dBtB.ptr, 0, 0, 0, lam, lam_bias, scaled, false,
                   M.scale_bias_const, CHOL_NAZ_W};
        c.values_override = S.dz.ptr; c.weights_override = S.dg.ptr; c.rhs_prefilled_all = true; c.all_rows = S.naz_has_cst;
        if (int rc = launch_chol(dev, c, &Xs)) return rc;
        if (scaled && !S.naz_has_cst) {
            hipLaunchKernelGGL(zero_weightless_rows_kernel<real_t>, dim3(m_max), dim3(64), 0, st, Xs.p.ptr, Xs.wsum_naz.ptr, m_max, 0,
                               std::numeric_limits<real_t>::epsilon(), S.dA.ptr, ldA, kt);
            HIP_CHECK(hipGetLastError());
        }
        return 0;
    }
    // the shared-matrix route
    if (side && !spU && m_u != m_max)
        return bad("NA_as_zero_X with dense U: side information on exactly the rows of the batch (m_u == m)");
    if (side && spU && !M.NA_as_zero_U)
        return bad("NA_as_zero_X with a sparse U whose absent entries are missing is not supported (NA_as_zero_U)");
    const int rows_side = P.rows_side;
    auto diag = [&](real_t *Gd, real_t mult, bool keep_last) {         // Gd [kx, kx] = B~^T B~ + lam mult I, the last unknown's own lambda
        HIP_CHECK(hipMemcpyAsync(Gd, S.dBtB.ptr, (size_t)kx * kx * sizeof(real_t), hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(add_diag_kernel<real_t>, dim3((kx + 255) / 256), dim3(256), 0, st, Gd, kx, 0, kx, lam * mult);
        const real_t last = (ub ? lam_bias : lam) * (keep_last ? (real_t)1 : mult);
        if (last != lam * mult) hipLaunchKernelGGL(add_diag_kernel<real_t>, dim3(1), dim3(64), 0, st, Gd, kx, kx - 1, kx, last - lam * mult);
    };
    const real_t mult_side = (M.scale_lam_sideinfo && !spU) ? (real_t)(n + p) : (scaled ? (real_t)n : (real_t)1);
    if (rows_side > 0 && (!S.inv_side.built || S.inv_side_mult != mult_side)) {
        ensure_CtC();
        const real_t mult = mult_side;
        DevBuf<real_t> Gd;
        Gd.alloc((size_t)kx * kx);
        diag(Gd.ptr, mult, false);
        S.inv_side.M.alloc((size_t)kt * kt);
        hipLaunchKernelGGL(naz_block_matrix_kernel<real_t>, grid1d((size_t)kt * kt), dim3(256), 0, st, Gd.ptr, kx, S.dCtC.ptr, kc, k_user, lam * mult,
                           S.inv_side.M.ptr);
        HIP_CHECK(hipGetLastError());
        newrows_naz_invert(dev, S.inv_side, kt);
        S.inv_side_mult = mult_side;
        HIP_CHECK(hipStreamSynchronize(st));       // Gd goes away
    }
    if (rows_side < m_max && !S.inv_plain.built) {
        const real_t mult = scaled ? (real_t)n : (real_t)1;
        DevBuf<real_t> Gd;
        Gd.alloc((size_t)kx * kx);
        diag(Gd.ptr, mult, M.scale_bias_const);
        S.inv_plain.M.alloc((size_t)kt * kt);
        hipLaunchKernelGGL(betbe_base_kernel<real_t>, grid1d((size_t)kt * kt), dim3(256), 0, st, Gd.ptr, kx, k_user, lam * mult, S.inv_plain.M.ptr);
        HIP_CHECK(hipGetLastError());
        newrows_naz_invert(dev, S.inv_plain, kt);
        HIP_CHECK(hipStreamSynchronize(st));
    }
    S.drhs.alloc_at_least((size_t)m_max * kt);
    run_rhs(true, S.drhs.ptr, (size_t)kt);
    if (side && !spU) {
        // dense U (centred already) joins the right-hand sides as U (w_user C)
        S.dUC.alloc_at_least((size_t)m_u * kc);
        launch_gemm<false>(dev, m_u, kc, p, M.w_user, S.dU.ptr, (size_t)p, S.dC.ptr, (size_t)kc, S.dUC.ptr, (size_t)kc);
        hipLaunchKernelGGL(add_cols_scaled_kernel<real_t>, grid1d((size_t)m_u * kc), dim3(256), 0, st, S.drhs.ptr, (size_t)kt, 0, S.dUC.ptr, kc, (real_t)1,
                           (size_t)m_u);
        HIP_CHECK(hipGetLastError());
    }
    newrows_naz_apply(S, S.inv_side, S.drhs.ptr, (size_t)kt, rows_side, S.dA.ptr, ldA);
    newrows_naz_apply(S, S.inv_plain, S.drhs.ptr + (size_t)rows_side * kt, (size_t)kt, m_max - rows_side, S.dA.ptr + (size_t)rows_side * ldA, ldA);
    return 0;
}

NewRowsState *newrows_state_create(const NewRowsModelArgs &M, int device, int *rc)
{
    auto bad = [&](const char *what) -> NewRowsState * {
        g_last_error = std::string("cmfrec_hip_factors_multiple: ") + what;
        *rc = 2;
        return nullptr;
    };
    *rc = 0;
    if (M.implicit && M.Bi) return bad("observation weights, dense X and implicit features belong to the explicit model");
    if (!M.B || M.n <= 0 || M.k < 0 || M.k_user < 0 || M.k_item < 0 || M.k_main < 0 || M.p < 0 || (M.implicit && M.user_bias))
        return bad("invalid arguments");
    if (M.Bi && ((size_t)M.k + (size_t)M.k_main == 0)) return bad("implicit features without factors");
    if (M.BiTBi_pre && !M.Bi) return bad("BiTBi without Bi");
    const bool l1on = M.l1_lam != (real_t)0 || (M.user_bias && M.l1_lam_bias != (real_t)0);
    if (l1on && M.TransCtCinvCt_pre) return bad("TransCtCinvCt cannot be used with an L1 penalty (collective.c:3378)");
    std::unique_ptr<NewRowsState> sp(new NewRowsState);
    NewRowsState &S = *sp;
    S.M = M;
    init_device(S.dev, device);
    DeviceInfo &dev = S.dev;
    hipStream_t st = dev.stream;
    const int ub = S.ub = M.user_bias ? 1 : 0;
    // non-negative factors: every row system goes through solve_nonneg with the reference's sweep limit for new rows, 10 x the
    // number of unknowns (collective.c:3401, :3800-3931, :4041-4054)
    dev.nonneg_now = M.nonneg;
    dev.max_cd_steps = 10 * (M.k_user + M.k + M.k_main + ub);
    S.l1on = l1on;
    dev.l1_now = M.l1_lam;
    dev.l1_last_now = ub ? M.l1_lam_bias : M.l1_lam;
    dev.l1_scale = 1;
    const int kc = S.kc = M.k_user + M.k, kk = S.kk = M.k + M.k_main, kt = S.kt = M.k_user + kk + ub, ktA = S.ktA = M.k_user + kk;
    S.kT = kk + ub;
    const size_t ldb_host = (size_t)(M.k_item + kk), ldB = S.ldB = ldb_host + ub;
    S.ldA = (size_t)kt;
    const int n = M.n;
    S.dB.alloc((size_t)n * ldB);
    HIP_CHECK(hipMemcpy2DAsync(S.dB.ptr, ldB * sizeof(real_t), M.B, ldb_host * sizeof(real_t), ldb_host * sizeof(real_t),
                               (size_t)n, hipMemcpyHostToDevice, st));
    if (ub) hipLaunchKernelGGL(col_fill_kernel<real_t>, grid1d(n), dim3(256), 0, st, S.dB.ptr, ldB, n, (int)ldb_host, (real_t)1);
    if (M.biasB) S.dbias.upload(M.biasB, (size_t)n, st);
    // implicit features: w_i Bi^T Bi joins the X block of every row's matrix (collective.c:1704-1707), w_i sum_{j observed} Bi_j
    // its right-hand side (:1757-1771); the matrix term carries the weight of the batch driver (:11016-11020), the right-hand
    // side the one the row function rescales by w_main (:3706-3714)
    if (M.Bi) {
        if (M.n_Bi <= 0 || M.n_Bi > n) return bad("invalid arguments");
        S.have_Bi = true;
        S.dBi.upload(M.Bi, (size_t)M.n_Bi * kk, st);
        S.dBiG.alloc((size_t)kk * kk);
        if (M.BiTBi_pre) S.dBiG.upload(M.BiTBi_pre, S.dBiG.n, st);
        else launch_gram(dev, S.gws, S.dBi.ptr, (size_t)kk, M.n_Bi, kk, S.dBiG.ptr, M.w_implicit_gram, (real_t)0);
        S.dBiFull.alloc((size_t)kt * kt);
        hipLaunchKernelGGL(embed_block_kernel<real_t>, grid1d((size_t)kt * kt), dim3(256), 0, st, S.dBiG.ptr, kk, M.k_user, kt, S.dBiFull.ptr);
    }
    if (M.C && M.p > 0) {
        S.have_C = true;
        S.dC.upload(M.C, (size_t)M.p * kc, st);
        if (M.U_colmeans) { S.have_means = true; S.dmeans.upload(M.U_colmeans, (size_t)M.p, st); }
        if (M.TransCtCinvCt_pre) { S.have_T = true; S.dT.upload(M.TransCtCinvCt_pre, (size_t)M.p * kc, st); }
    }
    if (M.implicit) {
        S.dG.alloc((size_t)kk * kk);
        if (M.BtB_pre) S.dG.upload(M.BtB_pre, (size_t)kk * kk, st);
        else launch_gram(dev, S.gws, S.dB.ptr + M.k_item, ldB, n, kk, S.dG.ptr, (real_t)1, M.lam_x);
        if (S.have_C) {
            S.dM.alloc((size_t)ktA * ktA);
            hipLaunchKernelGGL(betbe_base_kernel<real_t>, grid1d((size_t)ktA * ktA), dim3(256), 0, st, S.dG.ptr, kk, M.k_user, M.lam,
                               S.dM.ptr);
        }
    }
    if (M.TransBtBinvBt_pre && M.n_TB > 0) { S.have_TB = true; S.dTB.upload(M.TransBtBinvBt_pre, (size_t)M.n_TB * S.kT, st); }
    if (M.NA_as_zero_X || M.NA_as_zero_U) {
        if (M.implicit || M.Bi || M.nonneg || l1on) return bad("NA_as_zero belongs to the explicit model without implicit features, nonneg or an L1 penalty");
        if (kt > (sizeof(real_t) == 8 ? 256 : 272)) return bad("NA_as_zero: at most 256 (double) / 272 (single precision) unknowns per row");
        newrows_naz_model_side(S);
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventCreate(&S.ev0));
    HIP_CHECK(hipEventCreate(&S.ev1));
    HIP_CHECK(hipEventCreate(&S.ev2));
    HIP_CHECK(hipEventCreate(&S.ev3));
    HIP_CHECK(hipStreamSynchronize(st));       // the caller's matrices may go away
    S.M.B = S.M.C = S.M.U_colmeans = S.M.biasB = S.M.BtB_pre = S.M.TransCtCinvCt_pre = S.M.Bi = S.M.BiTBi_pre = S.M.TransBtBinvBt_pre = nullptr;
    return sp.release();
}

void newrows_state_destroy(NewRowsState *s)
{
    if (s == nullptr) return;
    int cur = -1;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != s->dev.device && hipSetDevice(s->dev.device) == hipSuccess;
    delete s;
    if (sw) (void)hipSetDevice(cur);
}

NewRowsView newrows_state_view(const NewRowsState *s)
{
    NewRowsView v;
    v.device = s->dev.device;
    v.dA = s->dA.ptr; v.ldA = s->ldA; v.rows = s->rows;
    v.dB = s->dB.ptr; v.ldB = s->ldB; v.n = s->M.n;
    v.dbiasB = s->dbias.ptr;
    return v;
}

int newrows_state_solve_ms(NewRowsState *s, double *ms)
{
    if (!s->timed) return 2;
    DeviceScope scope(s->dev.device);
    HIP_CHECK(hipEventSynchronize(s->ev1));
    float t = 0;
    HIP_CHECK(hipEventElapsedTime(&t, s->ev0, s->ev1));
    *ms = (double)t;
    return 0;
}

int newrows_state_run(NewRowsState *sp, const NewRowsBatchArgs &bt, real_t *A, real_t *biasA)
{
    NewRowsState &S = *sp;
    const NewRowsModelArgs &M = S.M;
    auto bad = [](const char *what) { g_last_error = std::string("cmfrec_hip_factors_multiple: ") + what; return 2; };
    const bool implicit = M.implicit, nonneg = M.nonneg, scale_lam = M.scale_lam, scale_lam_sideinfo = M.scale_lam_sideinfo,
               scale_bias_const = M.scale_bias_const, l1on = S.l1on, Bi = S.have_Bi;
    const real_t lam = M.lam, lam_bias = M.lam_bias, w_user = M.w_user, l1_lam = M.l1_lam, l1_lam_bias = M.l1_lam_bias;
    const int k_user = M.k_user, n = bt.n;
    const real_t *weight = bt.weight, *Xfull = bt.Xfull, *weight_full = bt.weight_full, *U = bt.U, *X = bt.X;
    const int_t *ixA = bt.ixA, *ixB = bt.ixB;
    const size_t *Xcsr_p = bt.Xcsr_p, *U_csr_p = bt.U_csr_p;
    size_t nnz = bt.nnz;
    int m_x = bt.m_x, m_u = bt.m_u, p = M.p;
    S.rows = 0;
    S.xb_resident = false;
    if (int frc = newrows_form_check(implicit, false, bt)) return frc;
    if (Xfull) { nnz = 0; ixA = nullptr; ixB = nullptr; X = nullptr; weight = nullptr; }
    if (m_x <= 0 || (!Xfull && !Xcsr_p && nnz == 0)) weight = nullptr;
    // sparse side information (COO or CSR over m_u rows, missing = absent): second gather source of the row kernel
    const bool spU = (U == nullptr && p > 0 && ((bt.nnz_U > 0 && bt.U_row && bt.U_col && bt.U_sp) || U_csr_p));
    const int m_max = std::max(m_x, (p > 0 && (U || spU)) ? m_u : 0);
    if (m_max <= 0) return 0;
    if (n <= 0 || n > M.n || (Bi && n > M.n_Bi) || (p > 0 && (U || spU) && !S.have_C) || (nnz > 0 && !Xcsr_p && (!ixA || !ixB || !X)))
        return bad("invalid arguments");
    if (spU && !implicit && scale_lam_sideinfo)
        return bad("sparse side information with scale_lam_sideinfo is not supported "
                   "(the reference scales the rows without observations differently, collective.c:3397-3411)");
    if (!(p > 0 && (U || spU))) { p = 0; m_u = 0; }
    // index validation on the host, before anything reaches the device (the fit entry points do the same,
    // fit.hip): a row id outside [0, m_x) or an item id outside [0, n) would corrupt device memory silently
    // (the missing-as-zero routes want the rows' lengths on the host for their task list: counted in the same pass)
    std::vector<size_t> lenX, lenU;
    const bool want_len = S.naz && ((M.NA_as_zero_X && !Xfull) || (M.NA_as_zero_U && spU));
    if (want_len) { lenX.assign((size_t)m_max, 0); lenU.assign((size_t)m_max, 0); }
    if (Xcsr_p) {
        const size_t nz = Xcsr_p[m_x];
        for (int r = 0; r < m_x; r++) if (Xcsr_p[r] > Xcsr_p[r + 1]) return bad("Xcsr_p is not non-decreasing");
        if (nz > 0 && (!bt.Xcsr_i || !bt.Xcsr)) return bad("Xcsr_i / Xcsr missing");
        for (size_t e = 0; e < nz; e++) if (bt.Xcsr_i[e] < 0 || bt.Xcsr_i[e] >= n) return bad("item index of X outside [0, n)");
        if (want_len) for (int r = 0; r < m_x; r++) lenX[r] = Xcsr_p[r + 1] - Xcsr_p[r];
    } else if (want_len) {
        for (size_t e = 0; e < nnz; e++) {
            if (ixA[e] < 0 || ixA[e] >= m_x || ixB[e] < 0 || ixB[e] >= n) return bad("row / item index of X outside [0, m_x) x [0, n)");
            lenX[ixA[e]]++;
        }
    } else {
        for (size_t e = 0; e < nnz; e++)
            if (ixA[e] < 0 || ixA[e] >= m_x || ixB[e] < 0 || ixB[e] >= n) return bad("row / item index of X outside [0, m_x) x [0, n)");
    }
    if (spU) {
        if (U_csr_p) {
            const size_t nz = U_csr_p[m_u];
            for (int r = 0; r < m_u; r++) if (U_csr_p[r] > U_csr_p[r + 1]) return bad("U_csr_p is not non-decreasing");
            if (nz > 0 && (!bt.U_csr_i || !bt.U_csr)) return bad("U_csr_i / U_csr missing");
            for (size_t e = 0; e < nz; e++) if (bt.U_csr_i[e] < 0 || bt.U_csr_i[e] >= p) return bad("attribute index of U outside [0, p)");
            if (want_len) for (int r = 0; r < m_u; r++) lenU[r] = U_csr_p[r + 1] - U_csr_p[r];
        } else {
            for (size_t e = 0; e < bt.nnz_U; e++) {
                if (bt.U_row[e] < 0 || bt.U_row[e] >= m_u || bt.U_col[e] < 0 || bt.U_col[e] >= p) return bad("row / attribute index of U outside [0, m_u) x [0, p)");
                if (want_len) lenU[bt.U_row[e]]++;
            }
        }
    }
    DeviceScope scope(S.dev.device);
    switches_mut().reload();
    DeviceInfo &dev = S.dev;
    GramWorkspace &gws = S.gws;
    hipStream_t st = dev.stream;
    const int ub = S.ub, kc = S.kc, kk = S.kk, kt = S.kt, ktA = S.ktA, kT = S.kT;
    const size_t ldB = S.ldB, ldA = S.ldA;
    DevBuf<real_t> &dA = S.dA, &dC = S.dC, &dU = S.dU;
    S.Xs.reset(new SparseShard);
    S.Us.reset(new SparseShard);
    SparseShard &Xs = *S.Xs, &Us = *S.Us;
    HIP_CHECK(hipEventRecord(S.ev0, st));
    dA.alloc_at_least((size_t)m_max * ldA);
    HIP_CHECK(hipMemsetAsync(dA.ptr, 0, (size_t)m_max * ldA * sizeof(real_t), st));
    auto empty_shard = [&]() {
        std::vector<size_t> pp((size_t)m_max + 1, 0);
        shard_from_csr(Xs, m_max, pp.data(), nullptr, nullptr, n, st);
    };
    // dense X: the block is compacted on the device into the triplets of its present entries (dense_rows_device.hpp), in
    // blocks of rows so that its device copy (and the weights') stays within a budget; with TransBtBinvBt and nothing that
    // changes the row systems, the rows without a missing entry are  x^T TransBtBinvBt  (common.c:736-758)
    const bool use_TB = Xfull != nullptr && S.have_TB && n == M.n_TB && !weight_full && !nonneg && !l1on && p == 0 && !Bi;
    if (Xfull) {
        const long long block_rows = newrows_block_rows(n, weight_full != nullptr, m_x);
        S.xb_resident = block_rows >= m_x && !use_TB;
        S.dmiss.alloc_at_least((size_t)m_x);
        if (use_TB) S.dTBout.alloc_at_least((size_t)m_x * kT);
        DevBuf<real_t> &dXb = S.dXb, &dWb = S.dWb;
        std::vector<std::unique_ptr<DenseRowsCoo>> parts;
        size_t total = 0;
        for (long long r0 = 0; r0 < m_x; r0 += block_rows) {
            const int rows = (int)std::min<long long>(block_rows, m_x - r0);
            dXb.upload(Xfull + (size_t)r0 * n, (size_t)rows * n, st);
            if (weight_full) dWb.upload(weight_full + (size_t)r0 * n, (size_t)rows * n, st);
            parts.emplace_back(new DenseRowsCoo);
            dense_rows_to_coo(dXb.ptr, weight_full ? dWb.ptr : nullptr, rows, n, (int)r0, bt.glob_mean_full, S.dmiss.ptr + r0,
                              *parts.back(), st);
            total += parts.back()->nnz;
            if (use_TB) {
                hipLaunchKernelGGL(dense_rows_center_kernel<real_t>, grid1d(std::min<size_t>((size_t)rows * n, (size_t)1 << 22)), dim3(256), 0,
                                   st, dXb.ptr, (size_t)rows, n, bt.glob_mean_full, S.dbias.ptr, S.dmiss.ptr + r0);
                HIP_CHECK(hipGetLastError());
                launch_gemm<false>(dev, rows, kT, n, (real_t)1, dXb.ptr, (size_t)n, S.dTB.ptr, (size_t)kT, S.dTBout.ptr + (size_t)r0 * kT,
                                   (size_t)kT);
                HIP_CHECK(hipStreamSynchronize(st));
            }
        }
        if (total == 0) empty_shard();
        else if (parts.size() == 1) {
            DenseRowsCoo &c = *parts[0];
            shard_from_coo(Xs, m_max, n, c.row.ptr, c.col.ptr, c.val.ptr, total, (real_t)0, (real_t)1, st, weight_full ? c.wt.ptr : nullptr);
            HIP_CHECK(hipStreamSynchronize(st));
        } else {
            DenseRowsCoo all;
            all.row.alloc(total); all.col.alloc(total); all.val.alloc(total);
            if (weight_full) all.wt.alloc(total);
            size_t at = 0;
            for (auto &c : parts) {
                if (c->nnz == 0) continue;
                HIP_CHECK(hipMemcpyAsync(all.row.ptr + at, c->row.ptr, c->nnz * sizeof(int), hipMemcpyDeviceToDevice, st));
                HIP_CHECK(hipMemcpyAsync(all.col.ptr + at, c->col.ptr, c->nnz * sizeof(int), hipMemcpyDeviceToDevice, st));
                HIP_CHECK(hipMemcpyAsync(all.val.ptr + at, c->val.ptr, c->nnz * sizeof(real_t), hipMemcpyDeviceToDevice, st));
                if (weight_full) HIP_CHECK(hipMemcpyAsync(all.wt.ptr + at, c->wt.ptr, c->nnz * sizeof(real_t), hipMemcpyDeviceToDevice, st));
                at += c->nnz;
            }
            HIP_CHECK(hipStreamSynchronize(st));
            parts.clear();
            shard_from_coo(Xs, m_max, n, all.row.ptr, all.col.ptr, all.val.ptr, total, (real_t)0, (real_t)1, st, weight_full ? all.wt.ptr : nullptr);
            HIP_CHECK(hipStreamSynchronize(st));
        }
    } else if (Xcsr_p) {
        std::vector<size_t> pp((size_t)m_max + 1);
        for (int r = 0; r <= m_max; r++) pp[r] = Xcsr_p[std::min(r, m_x)];
        shard_from_csr(Xs, m_max, pp.data(), bt.Xcsr_i, bt.Xcsr, n, st, Xcsr_p[m_x] > 0 ? weight : nullptr);
    } else if (nnz == 0) {
        empty_shard();
    } else {
        DevBuf<int> dr, dc; DevBuf<real_t> dv, dw;
        dr.upload(ixA, std::max<size_t>(nnz, 1), st); dc.upload(ixB, std::max<size_t>(nnz, 1), st);
        dv.upload(X, std::max<size_t>(nnz, 1), st);
        if (weight) dw.upload(weight, nnz, st);
        shard_from_coo(Xs, m_max, n, dr.ptr, dc.ptr, dv.ptr, nnz, (real_t)0, (real_t)1, st, weight ? dw.ptr : nullptr);
        HIP_CHECK(hipStreamSynchronize(st));
    }
    if (spU) {
        if (U_csr_p) {
            std::vector<size_t> up((size_t)m_max + 1);
            for (int r = 0; r <= m_max; r++) up[r] = U_csr_p[std::min(r, m_u)];
            shard_from_csr(Us, m_max, up.data(), bt.U_csr_i, bt.U_csr, p, st);
        } else {
            DevBuf<int> dr, dc; DevBuf<real_t> dv;
            dr.upload(bt.U_row, bt.nnz_U, st); dc.upload(bt.U_col, bt.nnz_U, st); dv.upload(bt.U_sp, bt.nnz_U, st);
            shard_from_coo(Us, m_max, p, dr.ptr, dc.ptr, dv.ptr, bt.nnz_U, (real_t)0, (real_t)1, st);
            HIP_CHECK(hipStreamSynchronize(st));
        }
    } else if (p > 0) {
        dU.upload(U, (size_t)m_u * p, st);
        if (S.have_means)
            hipLaunchKernelGGL(sub_colmeans_kernel<real_t>, grid1d((size_t)m_u * p), dim3(256), 0, st, dU.ptr, (size_t)m_u, p,
                               S.dmeans.ptr);
    }
    // w_user C^T C of the rows with dense side information: the model's, built by the first batch that has such rows
    auto ensure_CtC = [&]() {
        if (S.ctc_built) return;
        S.dCtC.alloc((size_t)kc * kc);
        launch_gram(dev, gws, dC.ptr, (size_t)kc, p, kc, S.dCtC.ptr, w_user, (real_t)0);
        S.ctc_built = true;
    };
    const real_t *opp = S.dB.ptr + M.k_item;
    const real_t *bias_sub = S.dbias.ptr;
    int rc = 0;
    // missing-as-zero models: a sparse X under NA_as_zero_X, a sparse U under NA_as_zero_U (a dense Xfull ignores the first, as
    // the reference does, collective.c:3621-3632; a dense U knows no absent entry)
    const bool naz_x = S.naz && M.NA_as_zero_X && !Xfull, naz_u = S.naz && M.NA_as_zero_U && spU && m_u > 0;
    if (naz_x || naz_u) {
        rc = newrows_run_naz(S, Xs, Us, lenX, lenU, m_max, m_u, p, spU, naz_x);
    } else if (implicit) {
        if (p == 0) {
            CholCall c{dA.ptr + k_user, ldA, opp, ldB, kk, 0, nullptr, S.dG.ptr, 0, 0, 0, lam, lam, false, false, false,
                       CHOL_IMPLICIT};
            rc = launch_chol(dev, c, &Xs);
        } else if (spU) {
            CholCall c{dA.ptr, ldA, opp, ldB, ktA, k_user, nullptr, nullptr, kc, m_u, p, lam, lam, false, false, false,
                       CHOL_COLLECTIVE_IMPLICIT, S.dM.ptr};
            c.X2 = &Us; c.B2 = dC.ptr; c.ldb2 = (size_t)kc; c.kc2 = kc; c.w2 = w_user;
            rc = launch_chol(dev, c, &Xs);
        } else {
            ensure_CtC();
            launch_gemm<false>(dev, m_u, kc, p, w_user, dU.ptr, (size_t)p, dC.ptr, (size_t)kc, dA.ptr, ldA);
            CholCall c{dA.ptr, ldA, opp, ldB, ktA, k_user, nullptr, S.dCtC.ptr, kc, m_u, p, lam, lam, false, false, false,
                       CHOL_COLLECTIVE_IMPLICIT, S.dM.ptr};
            rc = launch_chol(dev, c, &Xs);
        }
    } else if (Bi) {
        // with implicit features every row goes through the block solver, the model without side information included
        // (collective.c:3759-3760), and a row without observations is not a "cold" row (:3655-3659): one launch.  Rows that
        // the kernel treats as rows with side information take the block solver's rules for the last unknown's lambda
        // and the L1 penalty (:1349-1354); that is every row except those beyond a dense U.
        const bool all_u = p == 0 || spU || m_u >= m_max;
        bool sbc = scale_bias_const;
        if (!all_u) {
            if (l1on && scale_bias_const && (scale_lam || scale_lam_sideinfo))
                return bad("implicit features with an L1 penalty, scale_bias_const and dense side "
                           "information for fewer rows than the batch is not supported");
            sbc = false;
        }
        if (p > 0 && !spU) {
            ensure_CtC();
            launch_gemm<false>(dev, m_u, kc, p, w_user, dU.ptr, (size_t)p, dC.ptr, (size_t)kc, dA.ptr, ldA);
        }
        if (Xs.nnz > 0)
            hipLaunchKernelGGL(implicit_rhs_rows_kernel<real_t>, grid1d((size_t)m_max * 64), dim3(256), 0, st, Xs.p.ptr, Xs.i.ptr, S.dBi.ptr, kk,
                               M.w_implicit, m_max, dA.ptr, ldA, k_user);
        HIP_CHECK(hipGetLastError());
        CholCall c{dA.ptr, ldA, opp, ldB, kt, k_user, bias_sub, (p > 0 && !spU) ? S.dCtC.ptr : nullptr, p > 0 ? kc : 0,
                   all_u ? m_max : m_u, p, lam, lam_bias, (bool)(scale_lam || scale_lam_sideinfo),
                   (bool)(scale_lam_sideinfo && !spU), sbc, CHOL_COLLECTIVE};
        c.Mfull = S.dBiFull.ptr; c.rhs_prefilled_all = true;
        if (spU) { c.X2 = &Us; c.B2 = dC.ptr; c.ldb2 = (size_t)kc; c.kc2 = kc; c.w2 = w_user; c.rows2 = m_u; }
        rc = launch_chol(dev, c, &Xs);
    } else if (p == 0) {
        CholCall c{dA.ptr + k_user, ldA, opp, ldB, kk + ub, 0, bias_sub, nullptr, 0, 0, 0, lam, lam_bias,
                   (bool)(scale_lam || scale_lam_sideinfo), false, scale_bias_const, CHOL_EXPLICIT};
        rc = launch_chol(dev, c, &Xs);
    } else if (spU) {
        // rows with attributes but no observations come out of the same launch: without scale_lam_sideinfo the
        // "cold" solution (collective.c:3309-3440 with u_vec_sp) is the block system with an empty X part
        CholCall c{dA.ptr, ldA, opp, ldB, kt, k_user, bias_sub, nullptr, kc, m_u, p, lam, lam_bias, scale_lam, false,
                   scale_bias_const, CHOL_COLLECTIVE};
        c.X2 = &Us; c.B2 = dC.ptr; c.ldb2 = (size_t)kc; c.kc2 = kc; c.w2 = w_user;
        rc = launch_chol(dev, c, &Xs);
    } else {
        ensure_CtC();
        launch_gemm<false>(dev, m_u, kc, p, w_user, dU.ptr, (size_t)p, dC.ptr, (size_t)kc, dA.ptr, ldA);
        CholCall c{dA.ptr, ldA, opp, ldB, kt, k_user, bias_sub, S.dCtC.ptr, kc, m_u, p, lam, lam_bias,
                   (bool)(scale_lam || scale_lam_sideinfo), scale_lam_sideinfo, scale_bias_const, CHOL_COLLECTIVE};
        rc = launch_chol(dev, c, &Xs);
        if (rc == 0) {
            // cold rows
            S.dcold.alloc_at_least((size_t)m_u * kc);
            if (S.have_T && bt.allow_TransCtCinvCt) {
                launch_gemm<false>(dev, m_u, kc, p, (real_t)1, dU.ptr, (size_t)p, S.dT.ptr, (size_t)kc, S.dcold.ptr, (size_t)kc);
            } else {
                const real_t lc = lam / w_user;
                if (!S.cold_built) {
                    S.dMcold.alloc((size_t)kc * kc);
                    launch_gram(dev, gws, dC.ptr, (size_t)kc, p, kc, S.dMcold.ptr, (real_t)1, scale_lam_sideinfo ? lc * (real_t)p : lc);
                    if (scale_lam_sideinfo)
                        hipLaunchKernelGGL(add_diag_kernel<real_t>, dim3(1), dim3(64), 0, st, S.dMcold.ptr, kc, kc - 1, kc,
                                           lc - lc * (real_t)p);
                    S.cold_built = true;
                }
                launch_gemm<false>(dev, m_u, kc, p, (real_t)1, dU.ptr, (size_t)p, dC.ptr, (size_t)kc, S.dcold.ptr, (size_t)kc);
                CholCall cc{S.dcold.ptr, (size_t)kc, nullptr, 0, kc, 0, nullptr, S.dMcold.ptr, 0, 0, 0, 0, 0, false, false, false,
                            CHOL_PREFILLED};
                // factors_closed_form on C with l1_lam / w_user, scaled by p like lam except on the last unknown (collective.c:3385-3400)
                dev.l1_last_now = l1_lam / w_user;
                dev.l1_now = scale_lam_sideinfo ? dev.l1_last_now * (real_t)p : dev.l1_last_now;
                rc = launch_chol(dev, cc, nullptr, m_u);
                dev.l1_now = l1_lam; dev.l1_last_now = ub ? l1_lam_bias : l1_lam;
            }
            hipLaunchKernelGGL(cold_select_kernel<real_t>, dim3(m_u), dim3(64), 0, st, dA.ptr, ldA, kt, kc, S.dcold.ptr,
                               Xs.p.ptr, m_u);
        }
    }
    HIP_CHECK(hipGetLastError());
    if (rc) return rc;
    if (!implicit && !naz_x && Xs.weighted() && (scale_lam || scale_lam_sideinfo)) {
        hipLaunchKernelGGL(zero_weightless_rows_kernel<real_t>, dim3(m_max), dim3(64), 0, st, Xs.p.ptr, Xs.wsum.ptr, m_max, p > 0 ? m_u : 0,
                           std::numeric_limits<real_t>::epsilon(), dA.ptr, ldA, kt);
        HIP_CHECK(hipGetLastError());
    }
    if (use_TB) {
        hipLaunchKernelGGL(dense_rows_select_complete_kernel<real_t>, grid1d(std::min<size_t>((size_t)m_x * kT, (size_t)1 << 22)), dim3(256), 0, st,
                           dA.ptr, ldA, k_user, S.dTBout.ptr, kT, S.dmiss.ptr, (size_t)m_x);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(S.ev1, st));
    S.timed = true;
    S.rows = m_max;
    // the factors stay on the device (dA, the bias in its last column); the copies to the host are the caller's choice
    if (A)
        HIP_CHECK(hipMemcpy2DAsync(A, (size_t)ktA * sizeof(real_t), dA.ptr, ldA * sizeof(real_t), (size_t)ktA * sizeof(real_t),
                                   (size_t)m_max, hipMemcpyDeviceToHost, st));
    if (ub && biasA) {
        S.dba.alloc_at_least((size_t)m_max);
        hipLaunchKernelGGL(col_extract_kernel<real_t>, grid1d(m_max), dim3(256), 0, st, dA.ptr, ldA, m_max, ktA, S.dba.ptr);
        S.dba.download(biasA, (size_t)m_max, st);
    }
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// ---- imputation: the NaN of a dense batch replaced by the model's predictions -------------------------------------------------
// impute_X_collective_explicit (collective.c:11351-11544): the factors of the batch's rows (newrows_state_run), then block of
// rows by block of rows -- the budget of the dense batch -- the caller's X on the device, impute_fill_kernel on it with the
// device factors (the bias in the last column of their rows), the resident items and the per-row counts of missing entries the
// compaction left in S.dmiss, and the block back to Xout (which may be bt.Xfull itself).  The kernel must see the caller's
// values: the block the run left in S.dXb is kept only when the batch was one block and the TransBtBinvBt route did not centre
// it; otherwise every block is uploaded again.  A batch without any NaN is copied without solving (:11427); *solved says which.
int newrows_state_impute(NewRowsState *sp, const NewRowsBatchArgs &bt, real_t *Xout, real_t *A, real_t *biasA, bool *solved)
{
    NewRowsState &S = *sp;
    *solved = false;
    S.fill_ms = 0;
    const int m = bt.m_x, n = bt.n;
    const real_t *Xfull = bt.Xfull;
    if (S.M.implicit || !Xfull || m <= 0 || n <= 0 || n > S.M.n || !Xout) {
        g_last_error = "cmfrec_hip_newrows_impute: invalid arguments";
        return 2;
    }
    const size_t total = (size_t)m * (size_t)n;
    size_t e = 0;
    while (e < total && !std::isnan(Xfull[e])) e++;
    if (e == total) {
        if (Xout != Xfull) memcpy(Xout, Xfull, total * sizeof(real_t));
        return 0;
    }
    if (int rc = newrows_state_run(sp, bt, A, biasA)) return rc;
    *solved = true;
    DeviceScope scope(S.dev.device);
    hipStream_t st = S.dev.stream;
    const long long block_rows = newrows_block_rows(n, bt.weight_full != nullptr, m);
    const bool resident = S.xb_resident && block_rows >= m;
    ImputeParams<real_t> P;
    P.X = S.dXb.ptr; P.ldx = (size_t)n; P.n = n;
    P.lda = S.ldA; P.B = S.dB.ptr + S.M.k_item; P.ldb = S.ldB; P.kk = S.kk;
    P.ldbias = S.ldA; P.biasB = S.dbias.ptr; P.glob_mean = bt.glob_mean_full;
    P.tiles_per_block = 0;
    for (long long r0 = 0; r0 < m; r0 += block_rows) {
        const int rows = (int)std::min<long long>(block_rows, m - r0);
        if (!resident) S.dXb.upload(Xfull + (size_t)r0 * n, (size_t)rows * n, st);
        P.X = S.dXb.ptr; P.rows = rows;
        P.A = S.dA.ptr + (size_t)r0 * S.ldA + S.M.k_user;
        P.biasA = S.ub ? S.dA.ptr + (size_t)r0 * S.ldA + S.ktA : nullptr;
        P.row_missing = S.dmiss.ptr + r0;
        HIP_CHECK(hipEventRecord(S.ev2, st));
        launch_impute_fill(S.dev, st, P);
        HIP_CHECK(hipEventRecord(S.ev3, st));
        S.dXb.download(Xout + (size_t)r0 * n, (size_t)rows * n, st);
        HIP_CHECK(hipStreamSynchronize(st));
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, S.ev2, S.ev3));
        S.fill_ms += (double)t;
    }
    S.xb_resident = false;                     // (the block holds the filled values now)
    return 0;
}

double newrows_state_fill_ms(const NewRowsState *s) { return s->fill_ms; }
int newrows_state_naz_waves(const NewRowsState *s) { return s->naz_last_waves; }

// ---- exclusion lists of the last batch's rows ---------------------------------------------------
// row pointers of the union: the row's own entries, then the caller's list
__global__ void seen_union_ptr_kernel(const size_t *__restrict__ xp, const size_t *__restrict__ lp, int rows, size_t *__restrict__ out)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r <= rows) out[r] = xp[r] + lp[r];
}

// one wavefront per row: the item ids of the row's entries, then those of the caller's list
__global__ void __launch_bounds__(64)
seen_union_fill_kernel(const size_t *__restrict__ xp, const int *__restrict__ xi, const size_t *__restrict__ lp,
                       const int *__restrict__ li, const size_t *__restrict__ op, int rows, int *__restrict__ out)
{
    const int r = blockIdx.x;
    if (r >= rows) return;
    const size_t x0 = xp[r], nx = xp[r + 1] - x0, l0 = lp[r], nl = lp[r + 1] - l0, o0 = op[r];
    for (size_t e = threadIdx.x; e < nx; e += 64) out[o0 + e] = xi[x0 + e];
    for (size_t e = threadIdx.x; e < nl; e += 64) out[o0 + nx + e] = li[l0 + e];
}

int newrows_state_exclusions(NewRowsState *sp, bool seen, const size_t *excl_p, const int_t *excl_i, const size_t **dp, const int **di)
{
    NewRowsState &S = *sp;
    *dp = nullptr; *di = nullptr;
    const int rows = S.rows;
    if (rows <= 0 || (!seen && !excl_p)) return 0;
    auto bad = [](const char *what) { g_last_error = std::string("cmfrec_hip_newrows_topN: ") + what; return 2; };
    const int n = S.M.n;
    size_t nl = 0;
    if (excl_p) {
        nl = excl_p[rows];
        if (nl > 0 && !excl_i) return bad("invalid arguments");
        for (int r = 0; r < rows; r++) if (excl_p[r] > excl_p[r + 1]) return bad("excl_p is not non-decreasing");
    }
    DeviceScope scope(S.dev.device);
    hipStream_t st = S.dev.stream;
    if (!seen) {                                   // the caller's lists as they are (sorted by contract, like the ranker's)
        S.ep.upload(excl_p, (size_t)rows + 1, st);
        S.ei.alloc_at_least(std::max<size_t>(nl, 1));
        if (nl > 0) S.ei.upload(excl_i, nl, st);
        HIP_CHECK(hipStreamSynchronize(st));
        *dp = S.ep.ptr; *di = S.ei.ptr;
        return 0;
    }
    // The shard keeps a row's entries in the order of the triplets (that order fixes the sums of the row's system); the ranking
    // kernels search a sorted list.  So: a second CSR of item ids -- the shard's row pointers (or theirs plus the lists'), the ids
    // copied (or concatenated), each row's ids sorted by a segmented radix sort.  An id in both lists stays twice: the search
    // is a lower bound.
    const SparseShard &Xs = *S.Xs;
    const size_t total = Xs.nnz + nl;
    if (total >= ((size_t)1 << 31)) return bad("more than 2^31 excluded entries in one batch");
    const size_t *ptr = Xs.p.ptr;
    const int *keys_in = Xs.i.ptr;
    if (nl > 0) {
        S.ep_in.upload(excl_p, (size_t)rows + 1, st);
        S.ei_in.alloc_at_least(total);
        DevBuf<int> dl;
        dl.upload(excl_i, nl, st);
        S.ep.alloc_at_least((size_t)rows + 1);
        hipLaunchKernelGGL(seen_union_ptr_kernel, grid1d((size_t)rows + 1), dim3(256), 0, st, Xs.p.ptr, S.ep_in.ptr, rows, S.ep.ptr);
        hipLaunchKernelGGL(seen_union_fill_kernel, dim3(rows), dim3(64), 0, st, Xs.p.ptr, Xs.i.ptr, S.ep_in.ptr, dl.ptr, S.ep.ptr, rows,
                           S.ei_in.ptr);
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipStreamSynchronize(st));       // dl goes away
        ptr = S.ep.ptr; keys_in = S.ei_in.ptr;
    }
    S.ei.alloc_at_least(std::max<size_t>(total, 1));
    if (total > 0) {
        unsigned bits = 1;
        while (bits < 32 && (1ull << bits) < (unsigned long long)n) bits++;
        size_t bytes = 0;
        HIP_CHECK(rocprim::segmented_radix_sort_keys(nullptr, bytes, keys_in, S.ei.ptr, (unsigned)total, (unsigned)rows, ptr, ptr + 1, 0u, bits, st));
        S.sort_tmp.alloc_at_least(bytes + 16);
        HIP_CHECK(rocprim::segmented_radix_sort_keys(S.sort_tmp.ptr, bytes, keys_in, S.ei.ptr, (unsigned)total, (unsigned)rows, ptr, ptr + 1, 0u, bits, st));
    }
    HIP_CHECK(hipStreamSynchronize(st));
    *dp = ptr; *di = S.ei.ptr;
    return 0;
}

}  // namespace cmfhip

extern "C" {

static int factors_multiple_impl(real_t *A, real_t *biasA, int_t m_x, int_t m_u, int_t p, const real_t *U,
                                 const real_t *U_colmeans, const int_t ixA[], const int_t ixB[], const real_t *X,
                                 size_t nnz, const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
                                 const real_t *B, int_t n, const real_t *C, const real_t *biasB, int_t k, int_t k_user,
                                 int_t k_item, int_t k_main, real_t lam, real_t lam_bias, real_t lam_x, real_t w_user,
                                 bool implicit, bool scale_lam, bool scale_lam_sideinfo, bool scale_bias_const,
                                 const real_t *BtB_pre, const real_t *TransCtCinvCt_pre,
                                 const int_t U_row[], const int_t U_col[], const real_t *U_sp, size_t nnz_U,
                                 const size_t U_csr_p[], const int_t U_csr_i[], const real_t *U_csr, bool nonneg,
                                 real_t l1_lam, real_t l1_lam_bias, const NewRowsExtra &ex)
{
    return guarded([&]() {
        NewRowsBatchArgs bt;
        bt.m_x = m_x; bt.m_u = m_u; bt.n = n; bt.U = U;
        bt.U_row = U_row; bt.U_col = U_col; bt.U_sp = U_sp; bt.nnz_U = nnz_U; bt.U_csr_p = U_csr_p; bt.U_csr_i = U_csr_i; bt.U_csr = U_csr;
        bt.ixA = ixA; bt.ixB = ixB; bt.X = X; bt.nnz = nnz; bt.Xcsr_p = Xcsr_p; bt.Xcsr_i = Xcsr_i; bt.Xcsr = Xcsr;
        bt.weight = ex.weight; bt.Xfull = ex.Xfull; bt.weight_full = ex.weight_full; bt.glob_mean_full = ex.glob_mean_full;
        if (int frc = newrows_form_check(implicit, ex.Bi != nullptr, bt)) return frc;
        const bool side = p > 0 && (U || (nnz_U > 0 && U_row && U_col && U_sp) || U_csr_p);
        if (std::max(m_x, side ? m_u : 0) <= 0) return 0;          // a batch without rows
        if (!A) {
            g_last_error = "cmfrec_hip_factors_multiple: invalid arguments";
            return 2;
        }
        NewRowsModelArgs M;
        M.B = B; M.n = n; M.C = side ? C : nullptr; M.p = p; M.U_colmeans = (side && U) ? U_colmeans : nullptr; M.biasB = biasB;
        M.k = k; M.k_user = k_user; M.k_item = k_item; M.k_main = k_main; M.user_bias = biasA != nullptr;
        M.lam = lam; M.lam_bias = lam_bias; M.lam_x = lam_x; M.w_user = w_user;
        M.implicit = implicit; M.scale_lam = scale_lam; M.scale_lam_sideinfo = scale_lam_sideinfo; M.scale_bias_const = scale_bias_const;
        M.BtB_pre = BtB_pre; M.TransCtCinvCt_pre = TransCtCinvCt_pre; M.nonneg = nonneg; M.l1_lam = l1_lam; M.l1_lam_bias = l1_lam_bias;
        M.Bi = ex.Bi; M.n_Bi = n; M.w_implicit = ex.w_implicit; M.w_implicit_gram = ex.w_implicit_gram; M.BiTBi_pre = ex.BiTBi_pre;
        M.TransBtBinvBt_pre = ex.Xfull ? ex.TransBtBinvBt_pre : nullptr; M.n_TB = n;
        int rc = 0;
        NewRowsState *s = newrows_state_create(M, -1, &rc);
        if (s == nullptr) return rc;
        std::unique_ptr<NewRowsState, void (*)(NewRowsState *)> hold(s, newrows_state_destroy);
        return newrows_state_run(s, bt, A, biasA);
    });
}

int cmfrec_hip_factors_multiple(real_t *A, real_t *biasA, int_t m_x, int_t m_u, int_t p, const real_t *U,
                                const real_t *U_colmeans, const int_t ixA[], const int_t ixB[], const real_t *X,
                                size_t nnz, const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
                                const real_t *B, int_t n, const real_t *C, const real_t *biasB, int_t k, int_t k_user,
                                int_t k_item, int_t k_main, real_t lam, real_t lam_bias, real_t lam_x, real_t w_user,
                                bool implicit, bool scale_lam, bool scale_lam_sideinfo, bool scale_bias_const,
                                const real_t *BtB_pre, const real_t *TransCtCinvCt_pre,
                                const int_t U_row[], const int_t U_col[], const real_t *U_sp, size_t nnz_U,
                                const size_t U_csr_p[], const int_t U_csr_i[], const real_t *U_csr, bool nonneg)
{
    return factors_multiple_impl(A, biasA, m_x, m_u, p, U, U_colmeans, ixA, ixB, X, nnz, Xcsr_p, Xcsr_i, Xcsr, B, n, C, biasB, k,
                                 k_user, k_item, k_main, lam, lam_bias, lam_x, w_user, implicit, scale_lam, scale_lam_sideinfo,
                                 scale_bias_const, BtB_pre, TransCtCinvCt_pre, U_row, U_col, U_sp, nnz_U, U_csr_p, U_csr_i, U_csr,
                                 nonneg, (real_t)0, (real_t)0, NewRowsExtra());
}

int cmfrec_hip_factors_multiple_l1(real_t *A, real_t *biasA, int_t m_x, int_t m_u, int_t p, const real_t *U,
                                   const real_t *U_colmeans, const int_t ixA[], const int_t ixB[], const real_t *X,
                                   size_t nnz, const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
                                   const real_t *B, int_t n, const real_t *C, const real_t *biasB, int_t k, int_t k_user,
                                   int_t k_item, int_t k_main, real_t lam, real_t lam_bias, real_t lam_x, real_t w_user,
                                   bool implicit, bool scale_lam, bool scale_lam_sideinfo, bool scale_bias_const,
                                   const real_t *BtB_pre, const real_t *TransCtCinvCt_pre,
                                   const int_t U_row[], const int_t U_col[], const real_t *U_sp, size_t nnz_U,
                                   const size_t U_csr_p[], const int_t U_csr_i[], const real_t *U_csr, bool nonneg,
                                   real_t l1_lam, real_t l1_lam_bias)
{
    return factors_multiple_impl(A, biasA, m_x, m_u, p, U, U_colmeans, ixA, ixB, X, nnz, Xcsr_p, Xcsr_i, Xcsr, B, n, C, biasB, k,
                                 k_user, k_item, k_main, lam, lam_bias, lam_x, w_user, implicit, scale_lam, scale_lam_sideinfo,
                                 scale_bias_const, BtB_pre, TransCtCinvCt_pre, U_row, U_col, U_sp, nnz_U, U_csr_p, U_csr_i, U_csr,
                                 nonneg, l1_lam, l1_lam_bias, NewRowsExtra());
}

int cmfrec_hip_factors_multiple_ex(real_t *A, real_t *biasA, int_t m_x, int_t m_u, int_t p, const real_t *U,
                                   const real_t *U_colmeans, const int_t ixA[], const int_t ixB[], const real_t *X,
                                   size_t nnz, const size_t Xcsr_p[], const int_t Xcsr_i[], const real_t *Xcsr,
                                   const real_t *B, int_t n, const real_t *C, const real_t *biasB, int_t k, int_t k_user,
                                   int_t k_item, int_t k_main, real_t lam, real_t lam_bias, real_t lam_x, real_t w_user,
                                   bool implicit, bool scale_lam, bool scale_lam_sideinfo, bool scale_bias_const,
                                   const real_t *BtB_pre, const real_t *TransCtCinvCt_pre,
                                   const int_t U_row[], const int_t U_col[], const real_t *U_sp, size_t nnz_U,
                                   const size_t U_csr_p[], const int_t U_csr_i[], const real_t *U_csr, bool nonneg,
                                   real_t l1_lam, real_t l1_lam_bias,
                                   const real_t *weight, const real_t *Xfull, const real_t *weight_full, real_t glob_mean_full,
                                   const real_t *Bi, real_t w_implicit, real_t w_implicit_gram, const real_t *BiTBi_pre,
                                   const real_t *TransBtBinvBt_pre)
{
    NewRowsExtra ex;
    ex.weight = weight; ex.Xfull = Xfull; ex.weight_full = weight_full; ex.glob_mean_full = glob_mean_full;
    ex.Bi = Bi; ex.w_implicit = w_implicit; ex.w_implicit_gram = w_implicit_gram; ex.BiTBi_pre = BiTBi_pre;
    ex.TransBtBinvBt_pre = TransBtBinvBt_pre;
    return factors_multiple_impl(A, biasA, m_x, m_u, p, U, U_colmeans, ixA, ixB, X, nnz, Xcsr_p, Xcsr_i, Xcsr, B, n, C, biasB, k,
                                 k_user, k_item, k_main, lam, lam_bias, lam_x, w_user, implicit, scale_lam, scale_lam_sideinfo,
                                 scale_bias_const, BtB_pre, TransCtCinvCt_pre, U_row, U_col, U_sp, nnz_U, U_csr_p, U_csr_i, U_csr,
                                 nonneg, l1_lam, l1_lam_bias, ex);
}

}  // extern "C"

// ---- on-device self-test of the cross-lane primitives (lanes.hpp) -----------------------------
namespace cmfhip {
__global__ void lanes_selftest_kernel(real_t *out)
{
    const int lane = threadIdx.x;
    const real_t x = (real_t)(lane * 3 + 1);
    const real_t y = (real_t)(1000 + lane);
    real_t *o = out + lane;
    o[0 * 64] = lanes::xor1(x);
    o[1 * 64] = lanes::xor2(x);
    o[2 * 64] = lanes::xor4(x);
    o[3 * 64] = lanes::xor8(x);
    o[4 * 64] = lanes::recv_xor4(x, y);
    o[5 * 64] = lanes::recv_xor8(x, y);
    o[6 * 64] = lanes::tswap32_add(x, y);
    o[7 * 64] = lanes::tswap16_add(x, y);
    o[8 * 64] = lanes::bcast8<0>(x);
    o[9 * 64] = lanes::bcast8<3>(x);
    o[10 * 64] = lanes::bcast8<5>(x);
    o[11 * 64] = lanes::bcast8<7>(x);
    o[12 * 64] = lanes::wave_sum(x);
    real_t v[8];
    for (int i = 0; i < 8; i++) v[i] = (real_t)(lane + 100 * i);
    o[13 * 64] = treduce8_low<real_t>(v, lane);
    o[14 * 64] = treduce8_high<real_t>(v, lane);
    o[15 * 64] = lanes::half_mirror(x);
    o[16 * 64] = (real_t)lanes::bcast8<6>(lane * 5 + 2);
}
}  // namespace cmfhip

// Timing probe of the dense contraction C[M, N] = op(A) B on the device (tools/microbench/gemm_probe.py): milliseconds per call of
// the library's own MFMA kernel and -- when librocblas can be loaded at run time; the shared objects are not linked against it since
// round 6 -- of rocBLAS on the same operands, and the largest difference between their results relative to the largest entry
// (ms_rocblas = -1 and the difference against a plain one-thread-per-output kernel when the library is not there).
// transa != 0: A is stored [K, M].
namespace cmfhip {
template <typename T>
__global__ void gemm_naive_kernel(int M, int N, int K, int transa, const T *__restrict__ A, size_t lda, const T *__restrict__ B, size_t ldb,
                                  T *__restrict__ C, size_t ldc)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (size_t)M * N) return;
    const int i = (int)(e / N), j = (int)(e % N);
    double acc = 0;
    for (int q = 0; q < K; q++) acc += (double)(transa ? A[(size_t)q * lda + i] : A[(size_t)i * lda + q]) * (double)B[(size_t)q * ldb + j];
    C[(size_t)i * ldc + j] = (T)acc;
}
struct RocBlasProbe {          // (measurement tool only)
    typedef int (*create_t)(void **);
    typedef int (*destroy_t)(void *);
    typedef int (*set_stream_t)(void *, hipStream_t);
    typedef int (*gemm_t)(void *, int, int, int, int, int, const real_t *, const real_t *, int, const real_t *, int, const real_t *, real_t *, int);
    create_t create = nullptr; destroy_t destroy = nullptr; set_stream_t set_stream = nullptr; gemm_t gemm = nullptr;
    RocBlasProbe()
    {
        void *lib = dlopen("librocblas.so.5", RTLD_NOW | RTLD_LOCAL);
        if (!lib) lib = dlopen("librocblas.so", RTLD_NOW | RTLD_LOCAL);
        if (!lib) return;
        create = (create_t)dlsym(lib, "rocblas_create_handle"); destroy = (destroy_t)dlsym(lib, "rocblas_destroy_handle");
        set_stream = (set_stream_t)dlsym(lib, "rocblas_set_stream");
        gemm = (gemm_t)dlsym(lib, sizeof(real_t) == 4 ? "rocblas_sgemm" : "rocblas_dgemm");
    }
    bool ok() const { return create && destroy && set_stream && gemm; }
};
}  // namespace cmfhip
extern "C" int cmfrec_hip_gemm_probe(int M, int N, int K, int transa, int reps, double *ms_own, double *ms_rocblas, double *max_rel_diff)
{
    return guarded([&]() {
        DeviceInfo dev;
        init_device(dev, -1);
        DevBuf<real_t> A, B, C1, C2;
        A.alloc((size_t)M * K); B.alloc((size_t)K * N); C1.alloc((size_t)M * N); C2.alloc((size_t)M * N);
        std::vector<real_t> ha((size_t)M * K), hb((size_t)K * N);
        unsigned long long x = 88172645463325252ull;
        auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (real_t)((double)(x >> 11) / 9007199254740992.0 - 0.5); };
        for (auto &v : ha) v = rnd();
        for (auto &v : hb) v = rnd();
        A.upload(ha.data(), ha.size(), dev.stream); B.upload(hb.data(), hb.size(), dev.stream);
        const size_t lda = transa ? (size_t)M : (size_t)K;
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
        static const RocBlasProbe rb;
        void *h = nullptr;
        const bool have_lib = rb.ok() && rb.create(&h) == 0 && rb.set_stream(h, dev.stream) == 0;
        auto run = [&](bool own, real_t *C, double *ms) {
            const real_t one = 1, zero = 0;
            for (int r = 0; r < reps + 1; r++) {
                if (r == 1) HIP_CHECK(hipEventRecord(e0, dev.stream));
                if (!own)   // row-major C is the column-major C^T = B^T op(A)^T: first operand B, second operand A with the flag inverted
                    (void)rb.gemm(h, 111 /* none */, transa ? 112 /* transpose */ : 111, N, M, K, &one, B.ptr, N, A.ptr, (int)lda, &zero, C, N);
                else if (transa) launch_gemm<true>(dev, M, N, K, (real_t)1, A.ptr, lda, B.ptr, (size_t)N, C, (size_t)N);
                else launch_gemm<false>(dev, M, N, K, (real_t)1, A.ptr, lda, B.ptr, (size_t)N, C, (size_t)N);
            }
            HIP_CHECK(hipEventRecord(e1, dev.stream));
            HIP_CHECK(hipEventSynchronize(e1));
            float t = 0;
            HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
            if (ms) *ms = (double)t / std::max(reps, 1);
        };
        run(true, C1.ptr, ms_own);
        if (have_lib) run(false, C2.ptr, ms_rocblas);
        else {
            if (ms_rocblas) *ms_rocblas = -1.0;
            hipLaunchKernelGGL(gemm_naive_kernel<real_t>, grid1d((size_t)M * N), dim3(256), 0, dev.stream, M, N, K, transa, A.ptr, lda, B.ptr, (size_t)N,
                               C2.ptr, (size_t)N);
            HIP_CHECK(hipGetLastError());
        }
        std::vector<real_t> h1((size_t)M * N), h2((size_t)M * N);
        C1.download(h1.data(), h1.size(), dev.stream); C2.download(h2.data(), h2.size(), dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        if (h) (void)rb.destroy(h);
        double mx = 0, df = 0;
        for (size_t e = 0; e < h1.size(); e++) { mx = std::max(mx, std::fabs((double)h2[e])); df = std::max(df, std::fabs((double)h1[e] - (double)h2[e])); }
        if (max_rel_diff) *max_rel_diff = df / std::max(mx, 1e-300);
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        return 0;
    });
}

// Timing probe of the dense batch's compaction (tools/microbench/dense_rows_probe.py): a seeded [rows, n] block with the given
// fraction of present entries, the count pass and the scan + write pass timed with device events over `reps` runs after one
// warm-up run each (milliseconds per run); nnz: present entries found.
extern "C" int cmfrec_hip_dense_rows_probe(int rows, int n, double present, int reps, double *ms_count, double *ms_write, size_t *nnz)
{
    return guarded([&]() {
        if (rows <= 0 || n <= 0 || reps <= 0) { g_last_error = "cmfrec_hip_dense_rows_probe: rows, n, reps > 0"; return 2; }
        DeviceInfo dev;
        init_device(dev, -1);
        hipStream_t st = dev.stream;
        std::vector<real_t> h((size_t)rows * n);
        unsigned long long x = 88172645463325252ull;
        const real_t nan = std::numeric_limits<real_t>::quiet_NaN();
        for (auto &v : h) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            const double u = (double)(x >> 11) / 9007199254740992.0;
            v = (u < present) ? (real_t)(1.0 + 4.0 * u) : nan;
        }
        DevBuf<real_t> dX; DevBuf<int> dmiss; DevBuf<unsigned> cnt;
        dX.upload(h.data(), h.size(), st); dmiss.alloc((size_t)rows); cnt.alloc((size_t)rows + 1);
        hipEvent_t e0, e1;
        HIP_CHECK(hipEventCreate(&e0)); HIP_CHECK(hipEventCreate(&e1));
        const dim3 grid((unsigned)((rows + DENSE_ROWS_WAVES - 1) / DENSE_ROWS_WAVES)), block(64 * DENSE_ROWS_WAVES);
        float t = 0;
        for (int r = 0; r < reps + 1; r++) {
            if (r == 1) HIP_CHECK(hipEventRecord(e0, st));
            hipLaunchKernelGGL(dense_rows_count_kernel<real_t>, grid, block, 0, st, dX.ptr, rows, n, cnt.ptr, dmiss.ptr);
        }
        HIP_CHECK(hipEventRecord(e1, st)); HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
        if (ms_count) *ms_count = (double)t / reps;
        DenseRowsCoo out;
        dense_rows_to_coo(dX.ptr, nullptr, rows, n, 0, (real_t)0, dmiss.ptr, out, st);          // the triplets' buffers (and one whole conversion)
        DevBuf<size_t> off; off.alloc((size_t)rows + 1);
        {
            auto in = rocprim::make_transform_iterator(cnt.ptr, u32_to_size());
            DevBuf<unsigned char> tmp; size_t bytes = 0;
            HIP_CHECK(hipMemsetAsync(cnt.ptr + rows, 0, sizeof(unsigned), st));
            HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, off.ptr, (size_t)0, (size_t)rows + 1, rocprim::plus<size_t>(), st));
            tmp.alloc(bytes + 16);
            HIP_CHECK(rocprim::exclusive_scan(tmp.ptr, bytes, in, off.ptr, (size_t)0, (size_t)rows + 1, rocprim::plus<size_t>(), st));
            HIP_CHECK(hipStreamSynchronize(st));
        }
        for (int r = 0; r < reps + 1; r++) {
            if (r == 1) HIP_CHECK(hipEventRecord(e0, st));
            if (out.nnz)
                hipLaunchKernelGGL(dense_rows_write_kernel<real_t>, grid, block, 0, st, dX.ptr, (const real_t *)nullptr, rows, n, 0, (real_t)0, off.ptr,
                                   out.row.ptr, out.col.ptr, out.val.ptr, (real_t *)nullptr);
        }
        HIP_CHECK(hipEventRecord(e1, st)); HIP_CHECK(hipEventSynchronize(e1));
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventElapsedTime(&t, e0, e1));
        if (ms_write) *ms_write = (double)t / reps;
        if (nnz) *nnz = out.nnz;
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        return 0;
    });
}


// The dense layer on its own (tests/test_gpu_dense_ops.py): one operation through the launch helpers the library itself uses --
// launch_gemm<false / true>, launch_gram, the potrf_upper_kernel launch of the shared-matrix half-steps, launch_trtri and
// launch_potrs_rows -- on host images with explicit leading dimensions.  Each device buffer is a copy of its host image, whose
// first `off` elements precede the operand (the operand starts at image + off: alignment is the caller's choice); the whole
// image of C, those elements and the padding of every row included, is uploaded before the operation and downloaded after it.
//   op 0 / 1 : C[m, n] = s1 * A B with A [m, k] / s1 * A^T B with A stored [k, m]; B [k, n]
//   op 2     : C[k, k] = s1 * B[:n, :k]^T B[:n, :k] + s2 * I                                       (ldc == k)
//   op 3     : C[n, n] := its upper Cholesky factor in place, the strict lower triangle untouched  (ldc == n)
//   op 4     : C[n, n] = (R^T)^-1 for the upper factor R = A [n, n]                                (lda == ldc == n)
//   op 5     : C[m, :k] := C (R^T R)^-1 for the upper factor R = A [k, k]                          (lda == k, ldc >= k)
extern "C" int cmfrec_hip_dense_op(int op, int m, int n, int k, real_t s1, real_t s2, const real_t *A, size_t lda, int offA,
                                   const real_t *B, size_t ldb, int offB, real_t *C, size_t ldc, int offC)
{
    return guarded([&]() {
        if (op < 0 || op > 5) { g_last_error = "cmfrec_hip_dense_op: op is 0 .. 5"; return 2; }
        if (m < 0 || n < 0 || k < 0 || offA < 0 || offB < 0 || offC < 0) { g_last_error = "cmfrec_hip_dense_op: sizes and offsets >= 0"; return 2; }
        // rows and live columns of the three images for this operation (0 rows: the operand is not used)
        size_t ra = 0, ca = 0, rb = 0, cb = 0, rc = 0, cc = 0;
        bool tight_a = false, tight_c = false;
        switch (op) {
            case 0: ra = m; ca = k; rb = k; cb = n; rc = m; cc = n; break;
            case 1: ra = k; ca = m; rb = k; cb = n; rc = m; cc = n; break;
            case 2: rb = n; cb = k; rc = k; cc = k; tight_c = true; break;
            case 3: rc = n; cc = n; tight_c = true; break;
            case 4: ra = n; ca = n; rc = n; cc = n; tight_a = tight_c = true; break;
            default: ra = k; ca = k; rc = m; cc = k; tight_a = true; break;
        }
        if ((op == 2 && k < 1) || ((op == 3 || op == 4) && n < 1)) { g_last_error = "cmfrec_hip_dense_op: an empty matrix"; return 2; }
        if ((ra && (lda < ca || (tight_a && lda != ca))) || (rb && ldb < cb) || (rc && (ldc < cc || (tight_c && ldc != cc)))) {
            g_last_error = "cmfrec_hip_dense_op: a leading dimension below the row length (or not equal to it where the kernel takes none)";
            return 2;
        }
        if ((ra && ca && !A) || (rb && cb && !B) || (rc && cc && !C)) { g_last_error = "cmfrec_hip_dense_op: a missing operand"; return 2; }
        DeviceInfo dev;
        init_device(dev, -1);
        hipStream_t st = dev.stream;
        const size_t na = ra ? (size_t)offA + ra * lda : 0, nb = rb ? (size_t)offB + rb * ldb : 0, nc = rc ? (size_t)offC + rc * ldc : 0;
        DevBuf<real_t> dA, dB, dC;
        if (na && A) dA.upload(A, na, st);
        if (nb && B) dB.upload(B, nb, st);
        if (nc && C) dC.upload(C, nc, st);
        const real_t *pa = dA.ptr ? dA.ptr + offA : nullptr, *pb = dB.ptr ? dB.ptr + offB : nullptr;
        real_t *pc = dC.ptr ? dC.ptr + offC : nullptr;
        GramWorkspace gws;
        switch (op) {
            case 0: launch_gemm<false>(dev, m, n, k, s1, pa, lda, pb, ldb, pc, ldc); break;
            case 1: launch_gemm<true>(dev, m, n, k, s1, pa, lda, pb, ldb, pc, ldc); break;
            case 2: launch_gram(dev, gws, pb, ldb, n, k, pc, s1, s2); break;
            case 3: hipLaunchKernelGGL(potrf_upper_kernel<real_t>, dim3(1), dim3(256), 0, st, pc, n); break;
            case 4: launch_trtri(dev, pa, n, pc); break;
            default: launch_potrs_rows(dev, m, k, pa, pc, ldc); break;
        }
        HIP_CHECK(hipGetLastError());
        if (nc && C) dC.download(C, nc, st);
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}

// The fill kernel of the imputation on its own (tests/test_gpu_impute.py), through the launch helper newrows_state_impute uses:
// X[m, ldx] is filled in place where it holds NaN.  Host images, each uploaded as it is (m * lda, n * ldb, m * ldx elements
// from the pointer, the padding of the rows included), X downloaded whole.  biasA: m values, or -- where it points into the
// image of A -- the column of that image it points at (stride lda: the layout of the new-rows state, whose factor rows end in
// their bias).  row_missing: optional, one count per row; 0 leaves the row alone.
extern "C" int cmfrec_hip_impute_dense(int m, int n, int kk, const real_t *A, size_t lda, const real_t *biasA, const real_t *B, size_t ldb,
                                       const real_t *biasB, real_t glob_mean, real_t *X, size_t ldx, const int *row_missing)
{
    return guarded([&]() {
        auto bad = [](const char *what) { g_last_error = std::string("cmfrec_hip_impute_dense: ") + what; return 2; };
        if (m < 0 || n < 0 || kk < 0 || kk > IMPUTE_KMAX) return bad("sizes >= 0 and kk <= 272");
        if (m == 0 || n == 0) return 0;
        if (!X || ldx < (size_t)n || (kk > 0 && (!A || !B || lda < (size_t)kk || ldb < (size_t)kk))) return bad("a missing operand or a leading dimension below the row length");
        DeviceInfo dev;
        init_device(dev, -1);
        hipStream_t st = dev.stream;
        DevBuf<real_t> dA, dB, dX, dba, dbb;
        DevBuf<int> dmiss;
        if (kk > 0) { dA.upload(A, (size_t)m * lda, st); dB.upload(B, (size_t)n * ldb, st); }
        dX.upload(X, (size_t)m * ldx, st);
        const bool strided = biasA != nullptr && kk > 0 && biasA >= A && biasA < A + (size_t)m * lda;
        if (biasA && !strided) dba.upload(biasA, (size_t)m, st);
        if (biasB) dbb.upload(biasB, (size_t)n, st);
        if (row_missing) dmiss.upload(row_missing, (size_t)m, st);
        ImputeParams<real_t> P;
        P.X = dX.ptr; P.ldx = ldx; P.rows = m; P.n = n;
        P.A = dA.ptr; P.lda = lda; P.B = dB.ptr; P.ldb = ldb; P.kk = kk;
        P.biasA = !biasA ? nullptr : (strided ? dA.ptr + (biasA - A) : dba.ptr); P.ldbias = strided ? lda : 1;
        P.biasB = dbb.ptr; P.glob_mean = glob_mean; P.row_missing = dmiss.ptr; P.tiles_per_block = 0;
        launch_impute_fill(dev, st, P);
        dX.download(X, (size_t)m * ldx, st);
        HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    });
}

#ifdef CMF_CG_TICKS
// (instrumented builds only; not part of include/cmfrec_hip.h) copies the 32 tick sums to `out` and clears them
extern "C" int cmfrec_hip_debug_cg_ticks(unsigned long long *out)
{
    unsigned long long *buf = cg_ticks_buffer();
    HIP_CHECK(hipDeviceSynchronize());
    HIP_CHECK(hipMemcpy(out, buf, 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    HIP_CHECK(hipMemset(buf, 0, 32 * sizeof(unsigned long long)));
    return 0;
}
#endif

extern "C" int cmfrec_hip_selftest_lanes(void)
{
    int bad = -1;
    int rc = guarded([&]() {
        DeviceInfo dev;
        init_device(dev, -1);
        DevBuf<real_t> d;
        d.alloc(17 * 64);
        hipLaunchKernelGGL(lanes_selftest_kernel, dim3(1), dim3(64), 0, dev.stream, d.ptr);
        HIP_CHECK(hipGetLastError());
        std::vector<real_t> h(17 * 64);
        d.download(h.data(), h.size(), dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        auto X = [](int l) { return (double)(l * 3 + 1); };
        auto Y = [](int l) { return (double)(1000 + l); };
        bad = 0;
        for (int l = 0; l < 64; l++) {
            double e[17];
            e[0] = X(l ^ 1); e[1] = X(l ^ 2); e[2] = X(l ^ 4); e[3] = X(l ^ 8);
            e[4] = (l & 4) ? Y(l ^ 4) : X(l ^ 4);
            e[5] = (l & 8) ? Y(l ^ 8) : X(l ^ 8);
            e[6] = (l < 32) ? X(l) + X(l + 32) : Y(l - 32) + Y(l);
            e[7] = (l & 16) ? Y(l - 16) + Y(l) : X(l) + X(l + 16);
            e[8] = X((l & ~7) | 0); e[9] = X((l & ~7) | 3); e[10] = X((l & ~7) | 5); e[11] = X((l & ~7) | 7);
            double s = 0; for (int j = 0; j < 64; j++) s += X(j);
            e[12] = s;
            { int b = l & 7; double t = 0; for (int j = 0; j < 8; j++) t += (double)(((l & ~7) | j) + 100 * b); e[13] = t; }
            { int b = l >> 3; double t = 0; for (int j = 0; j < 8; j++) t += (double)(((l & 7) | (j << 3)) + 100 * b); e[14] = t; }
            e[15] = X(l ^ 7);
            e[16] = (double)(((l & ~7) | 6) * 5 + 2);
            for (int c = 0; c < 17; c++)
                if ((double)h[c * 64 + l] != e[c]) {
                    if (bad < 8) fprintf(stderr, "lanes selftest: case %d lane %d got %g expected %g\n", c, l, (double)h[c * 64 + l], e[c]);
                    bad++;
                }
        }
        return 0;
    });
    return rc ? -rc : bad;
}
