// device.hpp -- host-side device plumbing for the ALS path: HBM buffers, CSR shards with the
// nnz-binned row schedule, and the call descriptions of the row-update launchers (launch.hpp declares the launchers).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/cmfrec_hip.h"
#include "device_base.hpp"
#include "cg_kernels.hpp"
#include "chol_kernels.hpp"
#include "dense_kernels.hpp"
#include "gram_cg_kernels.hpp"
#include "topn_kernels.hpp"

namespace cmfhip {

// Rows are scheduled longest-first inside nnz bins; every bin is a persistent launch whose teams
// stride over the sorted list, which balances the heavy-tailed row lengths the reference handles
// with `omp schedule(dynamic)` (common.c:3259,3349).  A row of a bin with W waves per row keeps its
// gathered tiles in registers when it has <= 64*W non-zeros.
constexpr int MAX_DEVICES = 16;   // per-device caches of launch attributes
constexpr int NBINS = 6;
constexpr int BIN_VHEAVY = 0;   // > 1024 nnz : every CG pass split over many workgroups (vh_* kernels); measured on C2: 2048 -> 5.05, 1024 -> 4.93, 512 -> 5.11 ms
constexpr int BIN_HEAVY = 1;    // 257..1024  : 8 waves / row (double: register-resident up to 512 nnz, else re-streamed; single: two tiles per wave, resident)
constexpr int BIN_MED4 = 2;     // 129..256   : 4 waves / row
constexpr int BIN_MED2 = 3;     // 65..128    : 2 waves / row
constexpr int BIN_LIGHT = 4;    // 33..64     : 1 wave / row, 4 rows / workgroup
constexpr int BIN_TINY = 5;     // 1..32      : 1 wave / row, half-size tiles, double-buffered gather
constexpr int BIN_MIN_NNZ[NBINS] = {1025, 257, 129, 65, 33, 1};
// The boundary of the split rows is a property of the shard (SparseShard::vh_min).  Single precision: 1025 -- the 8-wave kernel
// keeps two tiles per wave and nothing else, so the boundary cannot move up.  Double precision: an 8-wave team keeps 512
// entries in registers and re-streams the second tile of longer rows on every pass (1.7x the algorithmic bytes measured on
// that bin in round 2); since the split rows' Gramian kernel does the last column block of k = 50 on the vector ALU (round 3),
// cutting at 513 is the faster split WHERE THE GRAMIAN PATH TAKES THE SPLIT ROWS: C2 4.36 -> 4.16 ms (513), 4.24 (769), 4.34
// (385) -- profiles/r03_c; where they are streamed (C1: small opposing matrices, many references) 1025 stays better (2.48
// against 2.65 ms).  CMFREC_HIP_VH_MIN overrides.
inline int vh_min_env()
{
    const int v = switches().vh_min;
    return v > 0 ? std::min(sizeof(real_t) == 4 ? BIN_MIN_NNZ[BIN_VHEAVY] : (1 << 30), std::max(258, v)) : 0;
}

struct SparseShard {
    int nrows = 0;
    size_t nnz = 0;
    int vh_min = BIN_MIN_NNZ[BIN_VHEAVY];       // rows of at least this many entries are split rows (build_bins)
    size_t opp_row_bytes_hint = 50 * sizeof(real_t);   // bytes of a gathered row (k x sizeof), for the choice of vh_min; set before the build
    int bin_of(long long l) const
    {
        if (l >= vh_min) return BIN_VHEAVY;
        for (int b = 1; b < NBINS; b++)
            if (l >= BIN_MIN_NNZ[b]) return b;
        return -1;   // empty row
    }
    static bool gram_pays(double vh_nnz, int n_other_, size_t opp_bytes_per_row)
    {
        // Round 6: always.  Rounds 3-5 streamed the split rows of double precision once per CG pass where they share their opposing
        // rows often enough to live in cache (more than 40 references per opposing row, or 3.5 with a matrix below 100 MB: C1).  Measured
        // again on C1 with the slice kernel as it stands (remainder columns on the vector ALU, the boundary at 513): 2.24 -> 1.86 ms per
        // iteration, its item step 1.31 -> 0.93 (profiles/r06/r06_n_c1_split_rows_sweep.txt); the streamed path stays behind
        // CMFREC_HIP_VH=stream, for k > 64 and for block systems.
        (void)vh_nnz; (void)opp_bytes_per_row;
        return sizeof(real_t) == 4 || n_other_ > 0;
    }
    DevBuf<size_t> p;
    DevBuf<int> i;
    DevBuf<real_t> v;
    // observation weights of the explicit model (empty: none): one per entry in the order of `v`, and per row the multiplier
    // of lambda under scale_lam -- the sum of the row's weights, 1 for a row without entries (wsumA / wsumB of the driver,
    // collective.c:7978-8008; summed in double, entry by entry, as there)
    DevBuf<real_t> w, wsum;
    // NA_as_zero_X with observation weights: the multipliers of that model -- sum of the row's weights + number of its ABSENT entries
    // (collective.c:7991-8022) -- in a buffer of their own, rebuilt by the session whenever X or the flag changes (round 6; they
    // used to overwrite wsum in place, which a second upload of X or switching the flag off left stale)
    DevBuf<real_t> wsum_naz;
    bool weighted() const { return w.ptr != nullptr && nnz > 0; }
    DevBuf<int> order;       // row ids sorted by nnz descending: [bin 0 | bin 1 | ... | bin 4 | empty rows]
    DevBuf<RowDesc> desc;    // same order: {row, nnz, CSR offset}
    int bin_rows[NBINS] = {0, 0, 0, 0, 0, 0};
    int bin_first[NBINS] = {0, 0, 0, 0, 0, 0};
    size_t bin_nnz[NBINS] = {0, 0, 0, 0, 0, 0};
    int n_nonempty = 0, n_empty = 0;
    int max_nnz = 0;
    int n_long = 0;          // rows with more than LONG_ROW entries (they lead the processing order)
    int n_gt96 = 0;          // rows with more than 96 entries (the six-block low-rank build of double precision, launch_lowrank.hip)
    int n_gt16 = 0;          // rows with more than 16 entries: the rest of the tiny bin goes two rows per wavefront
    int n_gt512 = 0;         // rows with more than 512 entries (single precision: the 257..512 part of the heavy bin runs on 4-wave teams)
    int n_gt_low[4] = {0, 0, 0, 0};   // rows with more than CG_NT_LOW * 8 W entries, W = 1, 2, 4, 8 (48 / 96 / 192 / 384): where a length bin's launch by tile size begins
    bool is_part = false;    // one of several parts of a block that are updated one after the other (session.hip)
    int n_other = 0;         // rows of the opposing matrix the entries refer to
    // Split rows: read their gathered rows once and run the CG on the row's own Gramian (gram_cg_kernels.hpp, one wavefront
    // per slice: c4shard's item rows 2.31 -> 1.57 ms, BASELINE config 4 on one GPU 40.6 -> 21.8 ms, C2's items 0.89 ->
    // 0.73 ms), or stream them once per CG pass (sorted entries, one slice of the opposing matrix per XCD).  Single
    // precision always takes the Gramian (the matrix cores outrun any gather).  In double precision v_mfma_f64_16x16x4 is no
    // faster than the VALU, and streaming wins once the split rows of a launch share their opposing rows often enough to live
    // in cache: C2's items (15 references per opposing row, a 144 MB opposing matrix) still favour the Gramian; C1
    // (MovieLens-10M-shaped: 4 / 28 MB opposing matrices, 100+ references) did not in round 3 -- 1.29 against 1.06 ms for its A-step --
    // and does since (gram_pays above: round 6).
    // `opp_bytes_per_row` = k x sizeof(real_t) of the launch.  CMFREC_HIP_VH=gram / stream force one.
    bool prefer_gram(size_t opp_bytes_per_row) const { return gram_pays((double)bin_nnz[0], n_other, opp_bytes_per_row); }
    // few split rows (less than about one round of workgroups per CG pass): their launch sequence is a chain of
    // latencies and runs on the second stream beside the other bins
    bool vh_runs_aside(int num_cus) const
    {
        return bin_rows[0] > 0 && n_chunks <= 4 * num_cus;
    }
    static constexpr int LONG_ROW = 1024;
    // rows (they lead the processing order) with more than `maxlen` entries, for the nnz-bin boundaries 32 .. 1024
    int rows_longer_than(int maxlen, int cap) const
    {
        int n;
        if (maxlen >= max_nnz) n = 0;
        else if (maxlen >= LONG_ROW) n = n_long;
        else if (maxlen >= 256) n = bin_first[BIN_MED4];
        else if (maxlen >= 128) n = bin_first[BIN_MED2];
        else if (maxlen >= 96) n = n_gt96;
        else if (maxlen >= 64) n = bin_first[BIN_LIGHT];
        else if (maxlen >= 32) n = bin_first[BIN_TINY];
        else n = n_nonempty;
        return std::min(n, cap);
    }
    // split-row work list and CG state of the very heavy rows (cg_kernels.hpp, VhState)
    int n_chunks = 0;
    DevBuf<int> vh_chunk_row, vh_chunk_start, vh_chunk_cnt, vh_chunk_off, vh_launch, vh_done;
    DevBuf<VhWork> vh_work;
    int n_launch = 0;
    DevBuf<real_t> vh_r, vh_p, vh_r_old, vh_part;
    // Gramian path of the very heavy rows (gram_cg_kernels.hpp): slices of <= GRAM_SLICE non-zeros
    static constexpr int GRAM_SLICE = 2048;
    int slice_len = GRAM_SLICE;          // entries per slice of this shard (build_bins)
    int n_slices = 0;
    DevBuf<int> sl_vrow, sl_first, sl_count, row_sl_off;
    std::vector<int> h_row_sl_off;       // host copy of row_sl_off (batching of the two-kernel Cholesky mode)
    DevBuf<real_t> gram_part;
    mutable DevBuf<real_t> chol_part;    // partial normal matrices of the slices (wave-per-row Cholesky kernel), sized on first use

    void upload(int nrows_, const size_t *hp, const int *hi, const real_t *hv, hipStream_t st, const real_t *hw = nullptr)
    {
        nrows = nrows_;
        nnz = hp[nrows] - hp[0];
        std::vector<size_t> p0(nrows + 1);
        for (int r = 0; r <= nrows; r++) p0[r] = hp[r] - hp[0];
        p.upload(p0.data(), nrows + 1, st);
        i.upload(hi + hp[0], nnz, st);
        v.upload(hv + hp[0], nnz, st);
        w.release(); wsum.release();
        if (hw != nullptr && nnz > 0) {
            w.upload(hw + hp[0], nnz, st);
            std::vector<real_t> ws((size_t)nrows);
            for (int r = 0; r < nrows; r++) {
                double acc_w = 0;
                for (size_t e = hp[r]; e < hp[r + 1]; e++) acc_w += hw[e];
                ws[r] = (hp[r + 1] > hp[r]) ? (real_t)acc_w : (real_t)1;
            }
            wsum.upload(ws.data(), (size_t)nrows, st);
            HIP_CHECK(hipStreamSynchronize(st));
        }
        std::vector<int> ord(nrows);
        std::iota(ord.begin(), ord.end(), 0);
        auto len = [&](int r) { return (long long)(p0[r + 1] - p0[r]); };
        std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return len(a) > len(b); });
        std::vector<RowDesc> dsc(nrows);
        std::vector<unsigned> lens(nrows);
        for (int q = 0; q < nrows; q++) {
            const int r = ord[q];
            dsc[q].row = r; dsc[q].nnz = (int)len(r); dsc[q].st = (unsigned long long)p0[r];
            lens[q] = (unsigned)len(r);
        }
        order.upload(ord.data(), nrows, st);
        desc.upload(dsc.data(), nrows, st);
        build_bins(lens.data(), st);
        HIP_CHECK(hipStreamSynchronize(st));   // host staging vectors go out of scope
    }

    // split-row work list: chunks (row-contiguous, the order their partials are added in) and the
    // workgroup -> chunk map of the pass kernel (empty: identity)
    void set_vh_chunks(const std::vector<int> &c_row, const std::vector<int> &c_start, const std::vector<int> &c_cnt,
                       const std::vector<int> &c_off, std::vector<int> launch, hipStream_t st)
    {
        n_chunks = (int)c_row.size();
        if (launch.empty()) { launch.resize(n_chunks); std::iota(launch.begin(), launch.end(), 0); }
        n_launch = (int)launch.size();
        vh_chunk_row.upload(c_row.data(), c_row.size(), st);
        vh_chunk_start.upload(c_start.data(), c_start.size(), st);
        vh_chunk_cnt.upload(c_cnt.data(), c_cnt.size(), st);
        vh_chunk_off.upload(c_off.data(), c_off.size(), st);
        vh_launch.upload(launch.data(), launch.size(), st);
        vh_part.alloc((size_t)n_chunks * 64);
        // resolved work items of the pass kernel (the split rows lead the processing order: desc[vi] is row vi of them)
        const int nvh = (int)c_off.size() - 1;
        std::vector<RowDesc> hd((size_t)std::max(nvh, 1));
        HIP_CHECK(hipMemcpyAsync(hd.data(), desc.ptr, (size_t)nvh * sizeof(RowDesc), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<VhWork> work(launch.size());
        for (size_t b = 0; b < launch.size(); b++) {
            VhWork &w = work[b];
            const int c = launch[b];
            w.pad_ = 0;
            if (c < 0) { w.vi = -1; w.row = 0; w.cnt = 0; w.chunk = 0; w.st = 0; continue; }
            w.vi = c_row[c]; w.row = hd[w.vi].row; w.cnt = c_cnt[c]; w.chunk = c;
            w.st = hd[w.vi].st + (unsigned long long)c_start[c];
        }
        vh_work.upload(work.data(), work.size(), st);
        HIP_CHECK(hipStreamSynchronize(st));
    }

    // nnz bins, split-row work list and CG state from the row lengths in processing order (descending)
    void build_bins(const unsigned *lens_sorted, hipStream_t st)
    {
        for (int b = 0; b < NBINS; b++) { bin_rows[b] = 0; bin_nnz[b] = 0; }
        n_empty = 0; n_long = 0; n_gt16 = 0; n_gt96 = 0; n_gt512 = 0; n_slices = 0; h_row_sl_off.assign(1, 0);
        n_gt_low[0] = n_gt_low[1] = n_gt_low[2] = n_gt_low[3] = 0;
        std::vector<int> c_row, c_first, c_cnt, c_off(1, 0);
        std::vector<int> s_row, s_first, s_count, s_off(1, 0);
        // few split rows (C2's users: 50 rows, 65 k entries): short slices, so that their Gramian kernels -- which run in line
        // with the other bins, see launch_cg_S -- have a few hundred wavefronts to spread over instead of a few dozen
        // where the split rows begin (see vh_min_env above): double precision cuts at 513 when the rows above that go through
        // their Gramian, at 1025 otherwise
        vh_min = BIN_MIN_NNZ[BIN_VHEAVY];
        if (vh_min_env() > 0) vh_min = vh_min_env();
        else if (sizeof(real_t) == 8) {
            double nnz513 = 0;
            for (int q = 0; q < nrows && lens_sorted[q] >= 513u; q++) nnz513 += (double)lens_sorted[q];
            const bool gram = (switches().vh != 0) ? switches().vh == 2 : gram_pays(nnz513, n_other, opp_row_bytes_hint);
            // (Round 5: 385 / 321 / 258 for a shard whose split rows hold 40 % of the entries -- C2's items -- move the eight-wave bin's rows
            //  to the slice kernel, 87 against 115-126 ps per entry: in line the two bins gain 0.035 ms together, side by side on two streams
            //  the half-step does not change, 3.285 / 3.298 against 3.293 / 3.286 ms; profiles/r05/r05_l_split_boundary.txt, r05_m_*)
            if (gram && opp_row_bytes_hint <= 16 * 4 * sizeof(real_t)) vh_min = 513;
        }
        long long vh_total = 0;
        for (int q = 0; q < nrows && (long long)lens_sorted[q] >= vh_min; q++) vh_total += (long long)lens_sorted[q];
        slice_len = (vh_total < (long long)GRAM_SLICE * 1024) ? 256 : GRAM_SLICE;
        for (int q = 0; q < nrows; q++) {
            const long long l = (long long)lens_sorted[q];
            if (l > LONG_ROW) n_long++;
            if (l > 16) n_gt16++;
            if (l > 96) n_gt96++;
            if (l > 512) n_gt512++;
            for (int w = 0; w < 4; w++) if (l > (long long)CG_NT_LOW * 8 * (1 << w)) n_gt_low[w]++;
            const int b = bin_of(l);
            if (b < 0) { n_empty++; continue; }
            if (b == BIN_VHEAVY) {
                const int CHN = TILE * VH_CHUNK_TILES;
                for (long long f = 0; f < l; f += CHN) {
                    c_row.push_back(bin_rows[b]); c_first.push_back((int)f); c_cnt.push_back((int)std::min<long long>(CHN, l - f));
                }
                c_off.push_back((int)c_row.size());
                // equal slices, multiples of 16 non-zeros (one staging round)
                const int nsl = (int)((l + slice_len - 1) / slice_len);
                const int per = (int)((((l + nsl - 1) / nsl) + 15) / 16 * 16);
                for (long long f = 0; f < l; f += per) {
                    s_row.push_back(bin_rows[b]); s_first.push_back((int)f); s_count.push_back((int)std::min<long long>(per, l - f));
                }
                s_off.push_back((int)s_row.size());
            }
            bin_rows[b]++; bin_nnz[b] += (size_t)l;
        }
        int acc = 0;
        for (int b = 0; b < NBINS; b++) { bin_first[b] = acc; acc += bin_rows[b]; }
        n_nonempty = acc;
        max_nnz = nrows ? (int)lens_sorted[0] : 0;
        if (bin_rows[BIN_VHEAVY]) {
            const int nvh = bin_rows[BIN_VHEAVY];
            set_vh_chunks(c_row, c_first, c_cnt, c_off, std::vector<int>(), st);      // row order; finalize_vheavy() refines it
            vh_done.alloc(nvh); vh_r_old.alloc(nvh);
            vh_r.alloc((size_t)nvh * 64); vh_p.alloc((size_t)nvh * 64);
            n_slices = (int)s_row.size();
            sl_vrow.upload(s_row.data(), s_row.size(), st);
            sl_first.upload(s_first.data(), s_first.size(), st);
            sl_count.upload(s_count.data(), s_count.size(), st);
            row_sl_off.upload(s_off.data(), s_off.size(), st);
            h_row_sl_off = s_off;
            gram_part.alloc((size_t)n_slices * GRAM_PART);
        }
        HIP_CHECK(hipStreamSynchronize(st));
    }
};

struct DeviceInfo {
    int device = 0;
    int num_cus = 256;
    hipStream_t stream = nullptr;
    DevBuf<real_t> cg_gfull, cg_rconst;   // block systems on the tiled CG kernels: weighted Gramian (k x k) and per-row constants
    DevBuf<real_t> tile_init;       // initial matrices of a Cholesky launch in tile-linear layout (chol_wave_kernels.hpp, tile_pack_kernel)
    DevBuf<int> row_counter;        // work counters of the dynamically scheduled row kernels (zeroed before each launch)
    DevBuf<real_t> potrs_inv, potrs_tmp;   // launch_potrs_rows: L^-1 and M^-1 of the shared matrix; the product before it replaces the rows
    DevBuf<real_t> potrs_ref;              // ... single precision: the matrix itself and the residuals of the refinement step
    DevBuf<real_t> gemm_ws;         // partial products of the split-K GEMMs (launch_dense.hip, launch_gemm)
    // second stream + events for two row kernels that may overlap (heavy-row teams beside light-row teams); created on
    // first use, owned here
    hipStream_t aux_stream = nullptr;
    hipEvent_t fork_ev = nullptr, join_ev = nullptr;
    // third stream for the eigen-decomposition of the low-rank path (one workgroup, overlaps the row kernels of both other streams)
    hipStream_t eig_stream_ = nullptr;
    hipEvent_t eig_fork = nullptr;
    hipStream_t eig_stream()
    {
        if (!eig_stream_) HIP_CHECK(hipStreamCreateWithFlags(&eig_stream_, hipStreamNonBlocking));
        return eig_stream_;
    }
    // solver option of the update in progress (set by the session around a half-step): closed-form rows are solved by
    // the non-negative coordinate descent instead of the Cholesky factorisation
    mutable bool nonneg_now = false;
    mutable int max_cd_steps = 100;
    mutable real_t l1_now = 0;      // L1 penalty of the update in progress (already divided by w_user / w_item for C / D)
    mutable real_t l1_last_now = 0; // ... of the last unknown (the bias' own penalty under l1_lam_unique)
    mutable real_t l1_scale = 1;    // ... times this for the launches whose lambda is scaled by a row count on the host
    DeviceInfo() = default;
    DeviceInfo(const DeviceInfo &) = delete;
    DeviceInfo &operator=(const DeviceInfo &) = delete;
    ~DeviceInfo()
    {
        if (eig_fork) (void)hipEventDestroy(eig_fork);
        if (eig_stream_) (void)hipStreamDestroy(eig_stream_);
        if (fork_ev) (void)hipEventDestroy(fork_ev);
        if (join_ev) (void)hipEventDestroy(join_ev);
        for (int i = 0; i < MAX_BIN_STREAMS; i++) {
            if (bin_join[i]) (void)hipEventDestroy(bin_join[i]);
            if (i > 0 && bin_streams[i]) (void)hipStreamDestroy(bin_streams[i]);
        }
        if (aux_stream) (void)hipStreamDestroy(aux_stream);
        if (stream) (void)hipStreamDestroy(stream);
    }
    void ensure_aux()
    {
        if (aux_stream) return;
        HIP_CHECK(hipStreamCreateWithFlags(&aux_stream, hipStreamNonBlocking));
        HIP_CHECK(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
        HIP_CHECK(hipEventCreateWithFlags(&join_ev, hipEventDisableTiming));
    }
    // further streams for the nnz bins of a half-step running side by side (launch_cg_S): bin_streams[0] is aux_stream
    static constexpr int MAX_BIN_STREAMS = 5;
    hipStream_t bin_streams[MAX_BIN_STREAMS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t bin_join[MAX_BIN_STREAMS] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    void ensure_bin_streams(int n)
    {
        ensure_aux();
        bin_streams[0] = aux_stream;
        if (!bin_join[0]) HIP_CHECK(hipEventCreateWithFlags(&bin_join[0], hipEventDisableTiming));
        for (int i = 1; i < n && i < MAX_BIN_STREAMS; i++) {
            if (!bin_streams[i]) HIP_CHECK(hipStreamCreateWithFlags(&bin_streams[i], hipStreamNonBlocking));
            if (!bin_join[i]) HIP_CHECK(hipEventCreateWithFlags(&bin_join[i], hipEventDisableTiming));
        }
    }
};

// HIP-event pairs around the launches of one nnz bin (0 heavy, 1 medium, 2 light) on the stream
// the kernel runs on; read back by cmfrec_hip_session_kernel_time.
struct EventPair { hipEvent_t a, b; };
struct BinTimers {
    std::vector<EventPair> ev[NBINS]; // per nnz bin (bin 0 = whole split-row sequence of the very heavy rows)
    void clear()
    {
        for (auto &v : ev) {
            for (auto &p : v) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
            v.clear();
        }
    }
};

// partial Gramians of launch_gram
struct GramWorkspace {
    DevBuf<real_t> partial;
};

// ------------------------------------------------------------------------------------------
// CG row updates
struct CgCall {
    real_t *A; size_t lda;
    const real_t *B; size_t ldb;
    int k;
    const real_t *bias_sub;
    const real_t *BtB;       // implicit only
    real_t lam, lam_last;
    bool scale_lam, scale_bias_const;
    int max_cg_steps;
    bool implicit;
    bool precond = false;
    // block system with dense side information (A points at the first unknown, koff of them precede the X block)
    int koff = 0, kc = 0;
    const real_t *CtC = nullptr, *UC = nullptr;
    real_t w_side = 0;
    int rows_with_u = 0, p_side = 0;
    bool scale_lam_sideinfo = false;
    // ... or sparse side information: the row's attributes (X2, CSR over the same rows) gather rows of C2[*, kc]
    const SparseShard *X2 = nullptr;
    const real_t *C2 = nullptr;
    // implicit features of the explicit model: Bi [*, ki], BiTBi = Bi^T Bi (unweighted), weight w_imp
    const real_t *Bi = nullptr, *BiTBi = nullptr;
    int ki = 0;
    real_t w_imp = 0;
    const real_t *gsum = nullptr;     // [rows, ki]: sum of the rows of Bi at each row's observed positions (segmented gather-sum), or null
    int skip_first = 0;               // generic kernel: the first positions of the processing order are solved elsewhere (launch_cg.hip, launch_cg_wide)
    // explicit model on the tiled kernels with a matrix every row shares and a per-row constant in the first residual (GRAMX builds):
    // NA_as_zero_X with observation weights (session.hip, update_factor_naz_weighted) -- Gx [k, k], rconst_x [rows, ldr_x], and the
    // entries' values / weights read from these arrays (CSR order of X) instead of the shard's own
    const real_t *Gx = nullptr, *rconst_x = nullptr;
    size_t ldr_x = 0;
    const real_t *values_override = nullptr, *weights_override = nullptr;
    bool gx_all_rows = false;         // ... with the preconditioner (generic kernel): the rows without entries are part of the launch
    const real_t *wsum_override = nullptr;   // lambda's per-row multipliers under scale_lam instead of the rows' own counts / sums
};

enum class CgVariant { Auto, Generic };
CgVariant cg_variant_from_env();

// layout of DeviceInfo::row_counter: [0, 64) the Cholesky kernels' counters, then CG_NCOUNTERS padded counters per nnz bin
constexpr int NCOUNTER_SETS = 2 * NBINS + 2;   // one set per nnz bin + spares for bins that run as two launches (NBINS, NBINS + 1; NBINS + 2 + bin)
constexpr size_t ROW_COUNTER_INTS = 64 + (size_t)NCOUNTER_SETS * CG_NCOUNTERS * CG_COUNTER_STRIDE;
inline size_t cg_counter_offset(int bin) { return 64 + (size_t)bin * CG_NCOUNTERS * CG_COUNTER_STRIDE; }

// CMFREC_HIP_CG_TEAMS (test hook): a launch of the dynamically scheduled row kernels with fewer teams than rows AND fewer than
// CG_NCOUNTERS.  The kernels hand out the positions nteams + j + CG_NCOUNTERS c from counter j = team mod CG_NCOUNTERS, which
// reaches every position only when all counters are in use (or no row is left to claim: what an uncapped launch guarantees).  So
// the capped launch gets its own descriptor array with the rows, in their order, at the positions its teams do reach -- 0 ..
// nteams-1, then nteams + j + CG_NCOUNTERS c for j < nteams -- and whatever at the others, which no team reads; the kernels stay as
// they are.  Host round trip and a synchronise behind the launch (release): a test hook, not a path of a fit.
struct CappedDesc {
    RowDesc *dev = nullptr;
    int nrows = 0;
    void build(const RowDesc *desc_dev, int count, int nteams, hipStream_t st)
    {
        std::vector<RowDesc> h((size_t)count);
        HIP_CHECK(hipMemcpyAsync(h.data(), desc_dev, (size_t)count * sizeof(RowDesc), hipMemcpyDeviceToHost, st));
        HIP_CHECK(hipStreamSynchronize(st));
        const int per_round = nteams;                       // positions reached per round of CG_NCOUNTERS
        const int rest = count - nteams;                    // rows beyond every team's first
        const int last = nteams + ((rest - 1) / per_round) * CG_NCOUNTERS + (rest - 1) % per_round;
        nrows = last + 1;
        RowDesc none; none.row = 0; none.nnz = 0; none.st = 0;
        std::vector<RowDesc> out((size_t)nrows, none);
        for (int i = 0; i < count; i++) {
            const int pos = (i < nteams) ? i : nteams + ((i - nteams) / per_round) * CG_NCOUNTERS + (i - nteams) % per_round;
            out[(size_t)pos] = h[(size_t)i];
        }
        HIP_CHECK(hipMalloc((void **)&dev, (size_t)nrows * sizeof(RowDesc)));
        HIP_CHECK(hipMemcpyAsync(dev, out.data(), (size_t)nrows * sizeof(RowDesc), hipMemcpyHostToDevice, st));
        HIP_CHECK(hipStreamSynchronize(st));                // (`out` leaves scope)
    }
    void release(hipStream_t st)
    {
        if (dev == nullptr) return;
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipFree(dev));
        dev = nullptr;
    }
};
// the grid of such a launch and whether it needs the array above (teams per workgroup: RPB, or the tiny kernel's four wavefronts)
inline bool cg_teams_cap(int &grid, int teams_per_block, int count)
{
    const int cap = switches().cg_teams;
    if (cap <= 0) return false;
    grid = std::min(grid, (cap + teams_per_block - 1) / teams_per_block);
    const int nteams = grid * teams_per_block;
    return nteams < CG_NCOUNTERS && nteams < count;
}

// split rows of this launch on the Gramian path?  (CMFREC_HIP_VH=stream / gram force one; k > 64 and block systems stream)
template <bool GRAMX>
inline bool vh_takes_gram(int k, const SparseShard &X)
{
    if (GRAMX || k > 16 * GRAM_NTT) return false;
    return (switches().vh != 0) ? switches().vh == 2 : X.prefer_gram((size_t)k * sizeof(real_t));
}

// number of streams the nnz bins of a half-step are spread over (CMFREC_HIP_BINS_PAR; 1 = one after the other)
inline int cg_bin_streams()
{
    const int n = switches().bins_par;  // C2: 4.19 (1) / 3.99 (2) / 4.21 (3) / 4.11 (4) / 4.30 (6) ms per iteration, profiles/r03_d
    return std::min(std::max(n, 1), DeviceInfo::MAX_BIN_STREAMS + 1);
}

inline dim3 grid1d(size_t n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }

}  // namespace cmfhip
