// launch_chol.hip -- launch unit of the closed-form row updates: the wave-per-row kernels (chol_wave_kernels.hpp), the
// producer / consumer pair of gramk_kernels.hpp, the CG on the summed partials (gram_cg_wide_kernels.hpp) and the
// workgroup-per-row kernel (chol_kernels.hpp) are instantiated here and nowhere else.  The low-rank rows are launch_lowrank.hip.
// (chol_rows_kernel stays in one object with the wave kernels: compiled in a unit of its own its builds come out with other
// register and spill counts, profiles/session_split.)
#include "launch.hpp"
#include "chol_wave_kernels.hpp"
#include "gramk_kernels.hpp"
#include "gram_cg_wide_kernels.hpp"

namespace cmfhip {

#ifndef CMF_PARTS_NP
#define CMF_PARTS_NP 2             // wavefronts per row of chol_parts_producer_kernel: 2 = halves of 18 tiles (default), 4 = quarters of 9 (measured on par with the round-2 producer)
#define CMF_PARTS_PD 2             // steps of four gathered rows in flight per wavefront (quarters: 4)
#define CMF_PARTS_WPS 2            // wavefronts per SIMD
#endif

// A row update that goes through partial matrices in HBM (the two-kernel wave path and the gramk pair of launch_chol): a
// producer kernel over work items, then a kernel over the rows that takes a row's partials.  Work items [0, n_slices) are the
// slices of the split rows -- positions < n_heavy of the processing order, SparseShard::sl_* -- and item n_slices + i is the
// whole row at position n_heavy + i.
// chol_part_scratch fills SL (slice tables, counts) and sizes the scratch X.chol_part: part_elems elements for each of at most
// max(batch, slices of the longest split row) items; that number is returned.
static size_t chol_part_scratch(const SparseShard &X, int n_heavy, int total, int batch, size_t part_elems, CholSlices<real_t> &SL)
{
    const int nsl = n_heavy > 0 ? X.n_slices : 0;
    if (n_heavy > 0) {
        SL.vrow = X.sl_vrow.ptr; SL.first = X.sl_first.ptr; SL.count = X.sl_count.ptr; SL.row_off = X.row_sl_off.ptr;
    }
    SL.n_slices = nsl; SL.n_heavy = n_heavy;
    const std::vector<int> &ho = X.h_row_sl_off;
    int max_row_items = 1;
    for (int r = 0; r < n_heavy; r++) max_row_items = std::max(max_row_items, ho[r + 1] - ho[r]);
    const size_t cap_items = (size_t)std::min<long long>((long long)nsl + (total - n_heavy), std::max(batch, max_row_items));
    if (X.chol_part.n < cap_items * part_elems) X.chol_part.alloc(cap_items * part_elems);
    SL.part = X.chol_part.ptr;
    return cap_items;
}
// The batches: run_batch(item0, item1, row0, row1, ctr) for the split rows in whole rows, then for the other positions in runs
// of cap_items; ctr and ctr + 1 are the batch's two work counters, zeroed here (the pairs cycle through [4, 60) of
// DeviceInfo::row_counter).
template <typename RunBatch>
static void chol_part_batches(const DeviceInfo &dev, const SparseShard &X, int n_heavy, int total, size_t cap_items, RunBatch run_batch)
{
    const int nsl = n_heavy > 0 ? X.n_slices : 0;
    const std::vector<int> &ho = X.h_row_sl_off;
    int ctr = 4;
    auto counted_batch = [&](int item0, int item1, int row0, int row1) {
        if (ctr + 2 > 60) ctr = 4;
        HIP_CHECK(hipMemsetAsync(dev.row_counter.ptr + ctr, 0, 2 * sizeof(int), dev.stream));
        run_batch(item0, item1, row0, row1, ctr);
        ctr += 2;
    };
    for (int r = 0; r < n_heavy;) {                 // split rows: whole rows per batch
        int r1 = r + 1;
        while (r1 < n_heavy && ho[r1 + 1] - ho[r] <= (int)cap_items) r1++;
        counted_batch(ho[r], ho[r1], r, r1);
        r = r1;
    }
    for (int r = n_heavy; r < total; r += (int)cap_items) {   // the others: item n_slices + i <-> position n_heavy + i
        const int r1 = (int)std::min<long long>(total, (long long)r + (long long)cap_items);
        counted_batch(nsl + (r - n_heavy), nsl + (r1 - n_heavy), r, r1);
    }
}

// X may be null for CHOL_PREFILLED (then nrows_prefilled rows are solved in natural order)
int launch_chol(const DeviceInfo &dev, const CholCall &c, const SparseShard *X, int nrows_prefilled)
{
    if (X != nullptr && c.mode == CHOL_EXPLICIT && c.row_limit < 0 && c.cg_wide == nullptr) {
        const int rc_lr = launch_plain_lowrank(dev, c, *X);      // rows with few entries against many unknowns (-1: not applicable)
        if (rc_lr >= 0) return rc_lr;
    }
    CholParams<real_t> P;
    P.A = c.A; P.lda = c.lda; P.B = c.B; P.ldb = c.ldb; P.kt = c.kt; P.koff = c.koff;
    P.indptr = X ? X->p.ptr : nullptr; P.indices = X ? X->i.ptr : nullptr; P.values = X ? X->v.ptr : nullptr;
    P.bias_sub = c.bias_sub;
    // observation weights of the explicit model ride on the shard (SparseShard::w / wsum)
    const bool weighted = X != nullptr && X->weighted() && (c.mode == CHOL_EXPLICIT || c.mode == CHOL_COLLECTIVE) && c.values_override == nullptr;
    if (weighted) { P.weights = X->w.ptr; P.wsum = X->wsum.ptr; }
    if (c.mode == CHOL_NAZ_W) { P.weights = c.weights_override; P.wsum = X->wsum_naz.ptr; }
    if (c.mult_override != nullptr) P.wsum = c.mult_override;
    P.x_rhs_only = c.x_rhs_only ? 1 : 0;
    if (c.entry_pairs) { P.entry_pairs = 1; P.weights = c.weights_override; }
    P.order = X ? X->order.ptr : nullptr;
    if (c.mode == CHOL_PREFILLED) P.nrows = nrows_prefilled;
    else if (c.mode == CHOL_COLLECTIVE || c.mode == CHOL_COLLECTIVE_IMPLICIT || (c.mode == CHOL_NAZ_W && c.all_rows)) P.nrows = X->nrows;   // empty rows too
    else P.nrows = X->n_nonempty;                                                // non-empty rows
    if (c.row_limit >= 0) P.nrows = std::min(P.nrows, c.row_limit);
    P.Minit = c.Minit; P.Mfull = c.Mfull; P.kc = c.kc; P.rows_with_u = c.rows_with_u; P.p_side = c.p_side;
    P.lam = c.lam; P.lam_last = c.lam_last;
    P.scale_lam = c.scale_lam; P.scale_lam_sideinfo = c.scale_lam_sideinfo; P.scale_bias_const = c.scale_bias_const;
    P.mode = c.mode;
    if (c.X2) {
        P.indptr2 = c.X2->p.ptr; P.indices2 = c.X2->i.ptr; P.values2 = c.values2 ? c.values2 : c.X2->v.ptr;
        P.B2 = c.B2; P.ldb2 = c.ldb2; P.kc2 = c.kc2; P.w2 = c.w2; P.koff2 = c.koff2; P.w2_syr_zero = c.w2_syr_zero ? 1 : 0; P.rows_src2 = c.rows2;
    }
    P.values_override = c.values_override; P.rhs_only = c.rhs_only ? 1 : 0; P.rhs_prefilled_all = c.rhs_prefilled_all ? 1 : 0;
    const bool l1on = dev.l1_now != (real_t)0 || dev.l1_last_now != (real_t)0;
    const bool nonneg = c.nonneg || dev.nonneg_now;
    P.nonneg = nonneg ? 1 : 0; P.max_cd_steps = (dev.nonneg_now || l1on) ? dev.max_cd_steps : c.max_cd_steps;
    // PREFILLED launches carry their lambda inside the prefilled matrix, scaled on the host (common.c:2832-2833): their L1
    // penalty takes the same factor (solve_elasticnet_batch / solve_nonneg_batch calls, :2876-2902)
    const real_t l1_mult = (c.mode == CHOL_PREFILLED || c.mode == CHOL_NAZ) ? dev.l1_scale : (real_t)1;
    P.l1 = dev.l1_now * l1_mult; P.l1_last = dev.l1_last_now * l1_mult;
    if (P.nrows <= 0) return 0;
    const int T = chol_tiles(c.kt);
    const size_t smem_nonneg = (nonneg || l1on) ? ((size_t)c.kt * c.kt + 2 * (size_t)c.kt + 64) * sizeof(real_t) : 0;
    if (smem_nonneg > 160 * 1024) {
        g_last_error = "cmfrec_hip: nonneg: the k_t x k_t system must fit the 160 KB of LDS (k_t <= 140 in double, 199 in single precision)";
        return 2;
    }
    if (T > 17 || (sizeof(real_t) == 8 && T > 16)) {
        g_last_error = "cmfrec_hip: Cholesky path: k_t too large for the register-resident normal matrix "
                       "(k_t <= 256 in double, <= 272 in single precision)";
        return 2;
    }
    if (dev.row_counter.n < ROW_COUNTER_INTS) const_cast<DeviceInfo &>(dev).row_counter.alloc(ROW_COUNTER_INTS);
    HIP_CHECK(hipMemsetAsync(dev.row_counter.ptr, 0, 4 * sizeof(int), dev.stream));   // [0, 4): first launches of this call
    P.counter = dev.row_counter.ptr;
    P.row_first = 0;
    const bool two_src = c.X2 != nullptr || c.mode == CHOL_NAZ || c.mode == CHOL_NAZ_W || c.x_rhs_only || c.entry_pairs;   // (that build only)
    // Rows of up to WAVE_ROW_MAX entries: one wavefront per row, the matrix in its registers (chol_wave_kernels.hpp).
    // The rows beyond (they lead the processing order) stay with the workgroup-per-row kernel below; the two launches
    // run side by side on two streams.  CMFREC_HIP_CHOL=rows keeps everything on the workgroup-per-row kernel (A/B
    // switch and on-device cross-check).
    {
        const int chol_sw = switches().chol;        // 1: rows, 2: noslices
        const bool border = (c.kt > 16) && ((c.kt - 1) % 16 == 0);
        const int nbw = (c.kt - (border ? 1 : 0) + 15) / 16;
        const bool wave_ok = X != nullptr && !two_src && !nonneg && !l1on && !c.rhs_only && nbw <= 8 && !weighted &&
                             (c.mode == CHOL_EXPLICIT || c.mode == CHOL_IMPLICIT || c.mode == CHOL_COLLECTIVE ||
                              c.mode == CHOL_COLLECTIVE_IMPLICIT) &&
                             chol_sw != 1;
        if (wave_ok) {
            // rows beyond 1024 entries: sliced (their slice tables are the ones of the split-row CG path, SparseShard::sl_*);
            // CMFREC_HIP_CHOL=noslices leaves them to the workgroup-per-row kernel (A/B switch)
            const bool sliced = chol_sw != 2;
            const int n_heavy = std::min(X->bin_rows[BIN_VHEAVY], P.nrows);
            const int total = P.nrows;
            DeviceInfo &d = const_cast<DeviceInfo &>(dev);
            // one launch of the wave kernel over the positions [first, last) of the processing order (or over work items)
            auto wave_launch = [&](int wmode, int first, int last, int counter, const CholSlices<real_t> &SL, hipStream_t st) {
                if (last <= first) return;
                CholParams<real_t> W = P;
                W.row_first = first; W.nrows = last; W.counter = dev.row_counter.ptr + counter;
                auto wlaunch = [&](auto kern, int nb_, int wps) {
                    poison_lds(st, dev.num_cus);      // test hook, launch_cg.hip
                    const size_t smem = 4 * (wmode == 1 ? chol_wave_lds_elems_producer(nb_) : chol_wave_lds_elems<real_t>(nb_)) * sizeof(real_t);
                    const int grid = std::min((last - first + 3) / 4, dev.num_cus * wps);
                    if (smem > 48 * 1024)
                        HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
                    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, W, X->desc.ptr, SL);
                };
                // <16-blocks, border, gather steps in flight, wavefronts per SIMD, overflow tiles, mode>
#define WAVE_KERN_M(nb_, pd, wps, nov, wm) (border ? chol_wave_kernel<real_t, nb_, true, pd, wps, nov, wm, false> : chol_wave_kernel<real_t, nb_, false, pd, wps, nov, wm, false>)
#define WAVE_KERN(nb_, pd, wps, nov) \
    (wmode == 1 ? WAVE_KERN_M(nb_, pd, wps, nov, 1) : wmode == 2 ? WAVE_KERN_M(nb_, pd, wps, nov, 2) : WAVE_KERN_M(nb_, pd, wps, nov, 0))
#ifdef CMFREC_HIP_FLOAT
                if (nbw <= 2) wlaunch(WAVE_KERN(2, 4, 4, 0), 2, 4);
                else if (nbw <= 4) wlaunch(WAVE_KERN(4, 4, 2, 0), 4, 2);
                else if (nbw <= 6) wlaunch(WAVE_KERN(6, 3, 2, 0), 6, 2);
                else wlaunch(WAVE_KERN(8, 2, 1, 0), 8, 1);
#else
                if (nbw <= 2) wlaunch(WAVE_KERN(2, 4, 3, 0), 2, 3);
                else if (nbw <= 4) wlaunch(WAVE_KERN(4, 3, 2, 0), 4, 2);
                else if (nbw <= 6) wlaunch(WAVE_KERN(6, 2, 1, 0), 6, 1);
                // 7 and 8 blocks in double: two kernels, see below
                // Round 5: one wavefront per SIMD issues a double-precision MFMA every ~130 cycles, two keep the pipe busy (35-38 against
                // 75 TFLOP/s, profiles/r05/r05_za_mfma_f64_occupancy.txt).  Where every unknown of the tiles is gathered (koff = 0,
                // k_t = 128 / 129: config 3) the rank-k update is done by TWO wavefronts per row with 18 tiles each, four workgroups
                // of 128 threads per CU (chol_parts_producer_kernel; config 3 15.10 -> 14.75-14.84 ms, r05_ze); the other shapes and
                // -DCMF_WAVE_PROD_ONE_WAVE keep the round-2 producer (one wavefront per row and SIMD, 32 + 4 tiles in two sweeps).
                else if (wmode == 1) {
                    const bool fullq = c.koff == 0 && c.kt - (border ? 1 : 0) == 128;
#ifdef CMF_WAVE_PROD_ONE_WAVE
                    const bool parts = false;
#else
                    const bool parts = fullq;
#endif
                    if (!parts) wlaunch(WAVE_KERN_M(8, 3, 1, 32, 1), 8, 1);      // 32 tiles per sweep
                    else if (switches().parts_coop && CMF_PARTS_NP == 2) {
                        // Round 6: the row's two wavefronts share ONE gather through LDS (chol_parts_coop_kernels.hpp, chol_wg_tu.hip):
                        // config 3 12.97 -> 12.80 ms, the partials bit for bit the same (CMFREC_HIP_PARTS_COOP=0: round 5's kernel)
                        poison_lds(st, dev.num_cus);
                        HIP_CHECK(launch_chol_parts_coop(dev.num_cus, border, switches().parts_coop == 3 ? 3 : 4, st, W, X->desc.ptr, SL));
                    }
                    else {
                        poison_lds(st, dev.num_cus);
                        constexpr int NPQ = CMF_PARTS_NP;
                        auto kern = border ? chol_parts_producer_kernel<real_t, 8, true, CMF_PARTS_PD, CMF_PARTS_WPS, true, NPQ>
                                           : chol_parts_producer_kernel<real_t, 8, false, CMF_PARTS_PD, CMF_PARTS_WPS, true, NPQ>;
                        const int grid = std::min(last - first, dev.num_cus * CMF_PARTS_WPS * 4 / NPQ);
                        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * NPQ), 0, st, W, X->desc.ptr, SL);
                    }
                }
                else if (switches().chol_wg) {
                    // Round 6: the factorisation by one workgroup of TWO wavefronts per row, the 36 tiles dealt to them, four rows per CU in
                    // flight (chol_wg_kernels.hpp) instead of one wavefront per row and SIMD with 263 spilled registers: config 3
                    // 14.2 -> 13.0 ms (profiles/r06/r06_j_*).  CMFREC_HIP_CHOL_WG=4: four wavefronts per row, two rows per CU (14.0);
                    // =0: the one-wavefront build below (A/B switch and on-device cross-check).
                    poison_lds(st, dev.num_cus);
                    HIP_CHECK(launch_chol_wg8(dev.num_cus, border, switches().chol_wg == 2 ? 2 : 4, st, W, X->desc.ptr, SL));       // chol_wg_tu.hip
                }
                else wlaunch((border ? chol_wave_kernel<real_t, 8, true, 1, 1, 6, 2, true> : chol_wave_kernel<real_t, 8, false, 1, 1, 6, 2, true>), 8, 1);
#endif
#undef WAVE_KERN
#undef WAVE_KERN_M
                HIP_CHECK(hipGetLastError());
            };
            const int nb_inst = nbw <= 2 ? 2 : nbw <= 4 ? 4 : nbw <= 6 ? 6 : 8;
            const size_t part_elems = chol_wave_part_elems(nb_inst);
            CholSlices<real_t> SLT;
            if (n_heavy > 0) {
                SLT.vrow = X->sl_vrow.ptr; SLT.first = X->sl_first.ptr; SLT.count = X->sl_count.ptr; SLT.row_off = X->row_sl_off.ptr;
                SLT.n_slices = X->n_slices;
            }
            SLT.n_heavy = n_heavy;
            SLT.dbg_skip = switches().debug_skip;
            const bool cg_wide = c.cg_wide != nullptr;
            if ((sizeof(real_t) == 8 && nbw > 6) || cg_wide) {
                // (cg_wide: the second kernel is the CG on the summed partials, gram_cg_wide_kernels.hpp -- every precision and width)
                // Two kernels (7 and 8 blocks in double: 28 / 36 tiles of 8 registers + the factorisation's temporaries exceed
                // what one kernel can keep in registers -- hipcc emits the accumulator-file form of the MFMAs at one wave per
                // SIMD, 256 registers for all MFMA destinations).  The producer build runs every row's rank-k update at full
                // MFMA rate (no spills, three gather steps in flight) and leaves the raw tiles in HBM, the second build adds the
                // initial matrix and factorises.  76 KB per work item each way; batches bound the scratch buffer.
                const int BATCH = 32768;
                const size_t cap_items = chol_part_scratch(*X, n_heavy, total, BATCH, part_elems, SLT);
                // the launch's initial matrices once, in the tile layout of the partials (the row kernel then adds them like a
                // partial, 16 values per round trip, instead of 144 dependent loads per row)
                if (!cg_wide) {
                    const bool fullm = (c.mode == CHOL_IMPLICIT);
                    const real_t *M1 = fullm ? c.Minit : c.Mfull, *M2 = fullm ? nullptr : c.Minit;
                    const size_t tl = (size_t)36 * 256;
                    if (M1 != nullptr || (M2 != nullptr && c.kc > 0)) d.tile_init.alloc_at_least(2 * tl);
                    if (M1 != nullptr) {
                        hipLaunchKernelGGL(tile_pack_kernel<real_t>, dim3((unsigned)((tl + 255) / 256)), dim3(256), 0, dev.stream, M1, c.kt, 8, d.tile_init.ptr);
                        SLT.init1 = d.tile_init.ptr;
                    }
                    if (M2 != nullptr && c.kc > 0) {
                        hipLaunchKernelGGL(tile_pack_kernel<real_t>, dim3((unsigned)((tl + 255) / 256)), dim3(256), 0, dev.stream, M2, c.kc, 8, d.tile_init.ptr + tl);
                        SLT.init2 = d.tile_init.ptr + tl;
                    }
                }
                auto run_batch = [&](int item0, int item1, int row0, int row1, int ctr) {
                    CholSlices<real_t> SL = SLT;
                    SL.part_base = item0;
                    wave_launch(1, item0, item1, ctr, SL, dev.stream);
                    if (cg_wide) {
                        WideCgParams<real_t> Wp;
                        Wp.part = SL.part; Wp.part_base = item0; Wp.NB = nb_inst; Wp.border = border ? 1 : 0;
                        Wp.row_off = X->row_sl_off.ptr; Wp.n_heavy = n_heavy; Wp.n_slices = SL.n_slices;
                        Wp.row_first = row0; Wp.row_last = row1;
                        const size_t smem = gcw_lds_elems<real_t>(c.kt) * sizeof(real_t);
                        auto kern = gram_cg_wide_kernel<real_t>;
                        HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
                        const int per_cu = std::max(1, (int)((size_t)160 * 1024 / smem));
                        poison_lds(dev.stream, dev.num_cus);
                        hipLaunchKernelGGL(kern, dim3(std::min(row1 - row0, dev.num_cus * per_cu)), dim3(64 * GCW_NW), smem, dev.stream, *c.cg_wide, Wp);
                        HIP_CHECK(hipGetLastError());
                    } else
                    wave_launch(2, row0, row1, ctr + 1, SL, dev.stream);
                };
                chol_part_batches(dev, *X, n_heavy, total, cap_items, run_batch);
                return 0;
            }
            const bool two = n_heavy > 0 && total > n_heavy;
            if (two) {
                d.ensure_aux();
                HIP_CHECK(hipEventRecord(d.fork_ev, dev.stream));
                HIP_CHECK(hipStreamWaitEvent(d.aux_stream, d.fork_ev, 0));
            }
            hipStream_t heavy_stream = two ? d.aux_stream : dev.stream;
            CholSlices<real_t> none;
            int rc_heavy = 0;
            if (n_heavy > 0 && sliced) {
                CholSlices<real_t> SL = SLT;
                const size_t need = (size_t)X->n_slices * part_elems;
                if (X->chol_part.n < need) X->chol_part.alloc(need);
                SL.part = X->chol_part.ptr;
                wave_launch(1, 0, X->n_slices, 1, SL, heavy_stream);       // partial Gramians of the slices
                wave_launch(2, 0, n_heavy, 3, SL, heavy_stream);           // their rows: sum, factorise, solve
            }
            wave_launch(0, n_heavy, total, 2, none, dev.stream);          // everything up to 1024 entries
            if (n_heavy > 0 && !sliced) {
                CholParams<real_t> H = P;
                H.nrows = n_heavy;
                // (on the stream the call was issued on: the k_t <= 64 variant of the row kernel forks onto the auxiliary one itself)
                rc_heavy = launch_chol_rows(dev, c, X, H, two_src, smem_nonneg);
            } else if (two) {
                HIP_CHECK(hipEventRecord(d.join_ev, d.aux_stream));
                HIP_CHECK(hipStreamWaitEvent(dev.stream, d.join_ev, 0));
            }
            return rc_heavy;
        }
        if (c.cg_wide != nullptr) {
            // the wide CG (launch_cg_wide) exists only as the second kernel of the wave path above: falling through would hand
            // its rows a factorisation without a word -- other numbers than the reference's CG
            g_last_error = "cmfrec_hip: internal: the Gramian CG beyond 64 unknowns needs the wave-per-row producer (weights, nonneg, L1 or "
                           "CMFREC_HIP_CHOL=rows keep it off)";
            return 2;
        }
    }
#ifdef CMFREC_HIP_FLOAT
    {
        // 17-block rows (k_t = 257 .. 272, config 5's item step): the rank-k update by gramk_producer_kernel (four independent
        // wavefronts per row or slice, operands straight from the gather), the partial matrices through HBM, the factorisation
        // and the substitutions by gramk_consumer_kernel (four wavefronts per row, two rows per CU).  CMFREC_HIP_GRAMK=0 keeps
        // the 16-wavefront row kernel with its own LDS-staged rank-k loop (A/B switch and cross-check).
        const bool gk_off = switches().gramk == 0;
        const bool gk_ok = X != nullptr && T == 17 && !two_src && c.koff == 0 && !weighted && !c.rhs_only && c.values_override == nullptr &&
                           (c.mode == CHOL_EXPLICIT || c.mode == CHOL_COLLECTIVE) && !nonneg && !l1on && !gk_off;
        if (gk_ok) {
            DeviceInfo &d = const_cast<DeviceInfo &>(dev);
            const int total = P.nrows;
            const int n_heavy = std::min(X->bin_rows[BIN_VHEAVY], total);
            CholSlices<real_t> SLT;
            const int batch_env = switches().gramk_batch;
            const int BATCH = batch_env > 0 ? batch_env : 32768;                      // x 158 KB = 5.2 GB of partials
            // (Tried: two half-size buffers with the consumer of a batch on the second stream beside the producer of the next
            // one -- c5 shard 146.3 against 145.8 ms / iteration in line, profiles/r03: not kept.)
            const size_t cap_items = chol_part_scratch(*X, n_heavy, total, BATCH, (size_t)GK_PART, SLT);
            // the launch's initial matrices once, in the tile layout of the partials (the consumer adds them like a partial)
            const real_t *init1 = nullptr, *init2 = nullptr;
            {
                const size_t tl = (size_t)GK_NT * 256;
                if (c.Mfull != nullptr || (c.Minit != nullptr && c.kc > 0)) d.tile_init.alloc_at_least(2 * tl);
                if (c.Mfull != nullptr) {
                    hipLaunchKernelGGL(tile_pack_lane_kernel<real_t>, dim3((unsigned)((tl + 255) / 256)), dim3(256), 0, dev.stream, c.Mfull, c.kt, GK_NB,
                                       d.tile_init.ptr);
                    init1 = d.tile_init.ptr;
                }
                if (c.Minit != nullptr && c.kc > 0) {
                    hipLaunchKernelGGL(tile_pack_lane_kernel<real_t>, dim3((unsigned)((tl + 255) / 256)), dim3(256), 0, dev.stream, c.Minit, c.kc, GK_NB,
                                       d.tile_init.ptr + tl);
                    init2 = d.tile_init.ptr + tl;
                }
            }
            int rc_all = 0;
            // two persistent workgroups per CU fill the register file; a few slots stay open so that the small launches of
            // another stream (the eigen-decomposition chain of the low-rank rows, EigCache) are dispatched beside a batch
            // instead of behind it
            const int gk_open = GK_OPEN_SLOTS;
            const int gk_grid = std::max(2 * dev.num_cus - gk_open, dev.num_cus / 2);
            auto run_batch = [&](int item0, int item1, int row0, int row1, int ctr) {
                real_t *part = SLT.part;
                CholSlices<real_t> SL = SLT;
                SL.part_base = item0;
                CholParams<real_t> W = P;
                W.row_first = item0; W.nrows = item1; W.counter = dev.row_counter.ptr + ctr;
                if (item1 > item0) {
                    poison_lds(dev.stream, dev.num_cus);
                    hipLaunchKernelGGL(gramk_producer_kernel<real_t>, dim3(std::min(item1 - item0, gk_grid)), dim3(256), 0, dev.stream, W,
                                       X->desc.ptr, SL);
                    HIP_CHECK(hipGetLastError());
                }
                CholParams<real_t> H = P;
                H.row_first = row0; H.nrows = row1; H.counter = dev.row_counter.ptr + ctr + 1;
                H.gk_part = part; H.gk_row_off = X->row_sl_off.ptr; H.gk_n_heavy = n_heavy; H.gk_n_slices = SLT.n_slices; H.gk_base = item0;
                H.gk_stride = (size_t)GK_PART; H.gk_init1 = init1; H.gk_init2 = init2;
                if (row1 > row0) {
                    poison_lds(dev.stream, dev.num_cus);
                    hipLaunchKernelGGL(gramk_consumer_kernel<real_t>, dim3(std::min(row1 - row0, gk_grid)), dim3(256), 0, dev.stream, H);
                    HIP_CHECK(hipGetLastError());
                }
            };
            chol_part_batches(dev, *X, n_heavy, total, cap_items, run_batch);
            return rc_all;
        }
    }
#endif
    return launch_chol_rows(dev, c, X, P, two_src, smem_nonneg);
}

// the workgroup-per-row kernel over the positions [P.row_first, P.nrows) of the processing order
int launch_chol_rows(const DeviceInfo &dev, const CholCall &c, const SparseShard *X, CholParams<real_t> P, bool two_src,
                            size_t smem_nonneg)
{
    const int T = chol_tiles(c.kt);
#ifdef CMF_CHOL_DEBUG
    P.dbg = switches().debug_skip;
    if (switches().debug_ticks && T >= 16) {
        // phase timers of the widest kernel: printed (and reset) by the launch that follows, i.e. per half-step
        static unsigned long long *d_ticks = nullptr;
        unsigned long long h[8];
        if (d_ticks == nullptr) { HIP_CHECK(hipMalloc((void **)&d_ticks, sizeof(h))); HIP_CHECK(hipMemset(d_ticks, 0, sizeof(h))); }
        else {
            HIP_CHECK(hipDeviceSynchronize());
            HIP_CHECK(hipMemcpy(h, d_ticks, sizeof(h), hipMemcpyDeviceToHost));
            if (h[5] > 0)
                fprintf(stderr, "chol_rows ticks/row: setup %.0f rank-k|trailing %.0f init %.0f diag+wait %.0f panel %.0f back %.0f  (rows %llu, nnz/row %.0f)\n",
                        (double)h[0] / h[5], (double)h[1] / h[5], (double)h[2] / h[5], (double)h[3] / h[5], (double)h[7] / h[5], (double)h[4] / h[5], h[5],
                        (double)h[6] / h[5]);
            HIP_CHECK(hipMemset(d_ticks, 0, sizeof(h)));
        }
        P.tstamp = d_ticks;
    }
#endif
    // the two-source build (sparse side information) only where it is asked for
#define CHOL_KERN(a, b, c_, d) (two_src ? chol_rows_kernel<real_t, a, b, c_, d, true> : chol_rows_kernel<real_t, a, b, c_, d, false>)
    hipStream_t run_on = dev.stream;
    auto launch = [&](auto kern, int ntt, int nw, int ch, int wgs) {
        size_t smem = std::max(chol_lds_elems<real_t>(ntt, ch) * sizeof(real_t), smem_nonneg);
        int grid = std::min(P.nrows - P.row_first, dev.num_cus * wgs);
        if (grid <= 0) return;
        if (smem > 48 * 1024)
            HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        poison_lds(run_on, dev.num_cus);          // test hook, launch_cg.hip
        hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), smem, run_on, P);
    };
    // <16-blocks per dimension, wavefronts per workgroup, gathered rows per round, waves per SIMD>
    if (T <= 4) {
        // k_t <= 64: the whole system is 10 tiles.  Rows of 129 non-zeros and more (they lead the processing order) get
        // a four-wave workgroup, the others a two-wave one: with few gathered rows the per-row latency chain dominates
        // and more rows in flight per CU win (C2 A-step 20.9 -> 12.8 ms).  The two launches overlap on two streams, so
        // the light rows fill the CUs while the heaviest rows finish.
        const int total = P.nrows;
        const int nheavy = (X != nullptr) ? std::min(total, X->bin_first[BIN_MED2]) : total;
        DeviceInfo &d = const_cast<DeviceInfo &>(dev);
        const bool two = nheavy > 0 && total > nheavy;
        if (two) {
            d.ensure_aux();
            HIP_CHECK(hipEventRecord(d.fork_ev, dev.stream));
            HIP_CHECK(hipStreamWaitEvent(d.aux_stream, d.fork_ev, 0));
        }
        if (nheavy > 0) {
            P.nrows = nheavy;
            launch(CHOL_KERN(4, 4, 16, 2), 4, 4, 16, 2);
        }
        if (total > nheavy) {
            P.row_first = nheavy; P.nrows = total; P.counter = dev.row_counter.ptr + 1;
            if (two) run_on = d.aux_stream;
            launch(CHOL_KERN(4, 2, 16, 2), 4, 2, 16, 4);
            if (two) {
                HIP_CHECK(hipEventRecord(d.join_ev, d.aux_stream));
                HIP_CHECK(hipStreamWaitEvent(dev.stream, d.join_ev, 0));
            }
        }
    }
    else if (T <= 6) launch(CHOL_KERN(6, 8, 32, 1), 6, 8, 32, 1);
    else if (T <= 9) launch(CHOL_KERN(9, 8, 32, 1), 9, 8, 32, 1);
#ifdef CMFREC_HIP_FLOAT
    else if (T <= 12) launch(CHOL_KERN(12, 8, 32, 1), 12, 8, 32, 1);
    else if (T <= 16) launch(CHOL_KERN(16, 16, 16, 1), 16, 16, 16, 1);
    // k = 256 + bias (BASELINE config 5).  Two workgroups per CU do not pay here: at the 128 VGPRs that allows the
    // kernel spills (c5 share 1.6 -> 4.0 s per A-step; the same on 9 tiles in double: 22.6 -> 25.6 ms).
    else {
        // The rows the producer / consumer pair of launch_chol does not take (weights, non-negativity, L1, a second gather
        // source): 16 wavefronts per row (10 tile slots per wave; the 8-wave build spilled ~500 registers: c5 shard B-step
        // 377 -> 274 ms), 32 gathered rows per round (half the barriers and staging rounds of the rank-k update: 272 -> 219 ms).
        // The build is register-starved either way (128 VGPRs at 16 waves, ~1 KB of scratch per lane).
        launch(CHOL_KERN(17, 16, 32, 1), 17, 16, 32, 1);
    }
#else
    else if (T <= 12) launch(CHOL_KERN(12, 8, 16, 1), 12, 8, 16, 1);
    else launch(CHOL_KERN(16, 8, 16, 1), 16, 8, 16, 1);
#endif
#undef CHOL_KERN
    HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace cmfhip
