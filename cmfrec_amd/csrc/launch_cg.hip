// launch_cg.hip -- launch unit of the CG row updates: every instantiation of cg_kernels.hpp (the register-tiled bins, the tiny
// rows, the split rows' pass / update pair, the lane <-> unknown kernel) and of gram_cg_kernels.hpp's gram_slice / gram_cg
// kernels lives in this object.  launch_cg() and launch_cg_any() are what the host units call (launch.hpp).
#include "launch.hpp"
#include "gram_cg_wide_kernels.hpp"     // (gcw_lds_elems: launch_cg_wide asks whether the wide kernel of launch_chol.hip fits)

namespace cmfhip {

CgVariant cg_variant_from_env() { return switches().cg_generic ? CgVariant::Generic : CgVariant::Auto; }

// Test hook (CMFREC_HIP_POISON_LDS=1, tests/test_gpu_operators.py): fill the LDS of every CU with NaN patterns in front of the
// launches of the CG row update, so that a kernel that reads LDS it has not written -- found once in gram_cg_kernel: 0 x stale
// LDS, NaN only when the previous tenant left a NaN pattern there, i.e. on some boxes in some runs -- fails every time.
__global__ void __launch_bounds__(256) poison_lds_kernel(int words)
{
    extern __shared__ unsigned int poison_words[];
    volatile unsigned int *w = poison_words;
    for (int e = threadIdx.x; e < words; e += 256) w[e] = 0xFFFFFFFFu;       // NaN as float and as either half of a double
}
void poison_lds(hipStream_t st, int num_cus)
{
    if (!switches().poison_lds) return;
    constexpr int BYTES = 80 * 1024;                                         // two workgroups cover the 160 KB of a CU
    static thread_local bool attr_set = false;
    if (!attr_set) {
        HIP_CHECK(hipFuncSetAttribute((const void *)poison_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BYTES));
        attr_set = true;
    }
    hipLaunchKernelGGL(poison_lds_kernel, dim3(num_cus * 4), dim3(256), BYTES, st, BYTES / 4);
    HIP_CHECK(hipGetLastError());
}

template <int S, bool IMPLICIT, int W, int RPB, bool GRAMX = false, int NRES_ = 0, int NTSEL = 0>
inline void launch_cg_bin(const DeviceInfo &dev, CgParams<real_t> P, int first, int count, BinTimers *tm, int bin, hipStream_t st, int counter_set = -1)
{
    if (count <= 0) return;
    EventPair ev{nullptr, nullptr};
    if (tm) {
        HIP_CHECK(hipEventCreate(&ev.a));
        HIP_CHECK(hipEventCreate(&ev.b));
        HIP_CHECK(hipEventRecord(ev.a, st));
    }
    poison_lds(st, dev.num_cus);
    P.order += first;
    P.desc += first;
    P.nrows = count;
    P.counter = dev.row_counter.ptr + cg_counter_offset(counter_set >= 0 ? counter_set : bin);          // zeroed by launch_cg_S
    constexpr int threads = 64 * W * RPB;
    size_t smem = (((IMPLICIT || GRAMX) ? (size_t)gram_elems<real_t>(S) : 0) + (size_t)RPB * 2 * W * 64) * sizeof(real_t);
    auto kern = cg_rows_kernel<real_t, S, IMPLICIT, W, RPB, GRAMX, NRES_, NTSEL>;
    // per device: the dynamic-LDS attribute and the occupancy belong to the device the kernel was loaded on
    static thread_local int bpc_dev[MAX_DEVICES] = {0};
    int &blocks_per_cu = bpc_dev[std::min(std::max(dev.device, 0), MAX_DEVICES - 1)];
    if (blocks_per_cu == 0) {
        if (smem > 48 * 1024)
            HIP_CHECK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        int nb = 0;
        HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, threads, smem));
        blocks_per_cu = std::max(1, nb);
    }
    int teams_needed = (count + RPB - 1) / RPB;
    int grid = std::min(teams_needed, dev.num_cus * blocks_per_cu);
    CappedDesc capped;
    if (cg_teams_cap(grid, RPB, count)) {
        capped.build(P.desc, count, grid * RPB, st);
        P.desc = capped.dev;
        P.nrows = capped.nrows;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(threads), smem, st, P);
    HIP_CHECK(hipGetLastError());
    capped.release(st);
    if (tm) {
        HIP_CHECK(hipEventRecord(ev.b, st));
        tm->ev[bin].push_back(ev);
    }
}

// The rows of at most 32 entries: one row per wavefront (cg_rows_tiny_kernel).  Two rows per wavefront (round 5, cg_rows_pair_kernel)
// issued 15 % fewer vector instructions per row but read its Gramian from LDS in every pass and a pair cost its longer row -- C2 3.375
// against 3.348 ms (profiles/r05/r05_e_*, r05_w_*); removed in round 6, the sources are in the history (git log -- cmfrec_amd/csrc/cg_pair_kernels.hpp).
template <int S, bool IMPLICIT, bool GRAMX = false>
inline void launch_cg_tiny(const DeviceInfo &dev, CgParams<real_t> P, int first, int count, BinTimers *tm, hipStream_t st, int n_gt16)
{
    if (count <= 0) return;
    EventPair ev{nullptr, nullptr};
    if (tm) {
        HIP_CHECK(hipEventCreate(&ev.a));
        HIP_CHECK(hipEventCreate(&ev.b));
        HIP_CHECK(hipEventRecord(ev.a, st));
    }
    poison_lds(st, dev.num_cus);
    // One launch for the bin (a second launch for the rows of <= 16 entries costs more in launch tails beside the other bins than
    // the shorter tile saves, profiles/r04/r04_z2); the kernels take the 16-slot tile where the rows allow it.
    constexpr bool tiny16_on = true;
    const int count_le16 = std::min(count, std::max(0, first + count - std::max(first, n_gt16)));
    size_t smem = ((IMPLICIT || GRAMX) ? (size_t)gram_elems<real_t>(S) : 0) * sizeof(real_t);
    const int di = std::min(std::max(dev.device, 0), MAX_DEVICES - 1);
    CgParams<real_t> P1 = P;
    P1.order += first;
    P1.desc += first;
    P1.nrows = count;
    P1.counter = dev.row_counter.ptr + cg_counter_offset(BIN_TINY);
    {
        const bool mixed = tiny16_on && count_le16 > 0;
        auto kern = mixed ? cg_rows_tiny_kernel<real_t, S, IMPLICIT, GRAMX, 0> : cg_rows_tiny_kernel<real_t, S, IMPLICIT, GRAMX, 4>;
        static thread_local int bpc_dev[MAX_DEVICES][2] = {{0}};
        int &blocks_per_cu = bpc_dev[di][mixed ? 1 : 0];
        if (blocks_per_cu == 0) {
            int nb = 0;
            HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, smem));
            blocks_per_cu = std::max(1, nb);
        }
        int grid = std::min((count + 3) / 4, dev.num_cus * blocks_per_cu);
        CappedDesc capped;
        if (cg_teams_cap(grid, 4, count)) {
            capped.build(P1.desc, count, grid * 4, st);
            P1.desc = capped.dev;
            P1.nrows = capped.nrows;
        }
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), smem, st, P1);
        capped.release(st);
    }
    HIP_CHECK(hipGetLastError());
    if (tm) {
        HIP_CHECK(hipEventRecord(ev.b, st));
        tm->ev[BIN_TINY].push_back(ev);
    }
}

// very heavy rows: one (pass, update) launch pair per CG pass
template <int S, bool IMPLICIT, bool GRAMX = false>
inline void launch_cg_vheavy(const DeviceInfo &dev_, CgParams<real_t> P, const SparseShard &X, BinTimers *tm, hipStream_t st)
{
    const int nvh = X.bin_rows[BIN_VHEAVY];
    if (nvh <= 0) return;
    struct { hipStream_t stream; int num_cus; } dev{st, dev_.num_cus};      // everything below launches on `st`
    EventPair ev{nullptr, nullptr};
    if (tm) {
        HIP_CHECK(hipEventCreate(&ev.a));
        HIP_CHECK(hipEventCreate(&ev.b));
        HIP_CHECK(hipEventRecord(ev.a, dev.stream));
    }
    // Default: read the gathered rows once and run the CG on the row's own Gramian (gram_cg_kernels.hpp); CMFREC_HIP_VH=stream
    // takes the launch pair per CG pass below (also the on-device cross-check of the Gramian path, and the only path for
    // k > 64 and for block systems).
    if (vh_takes_gram<GRAMX>(P.k, X)) {
        // one gather: Gramian slices on the matrix cores, then CG on the k x k system (gram_cg_kernels.hpp)
        GramParams<real_t> G;
        G.sl_vrow = X.sl_vrow.ptr; G.sl_first = X.sl_first.ptr; G.sl_count = X.sl_count.ptr; G.row_sl_off = X.row_sl_off.ptr;
        G.part = X.gram_part.ptr; G.n_slices = X.n_slices; G.nvh = nvh;
        P.nrows = nvh;
#ifdef CMF_CG_DEBUG
        if (switches().debug_ticks) {
            static unsigned long long *d_t = nullptr;
            unsigned long long h[4];
            if (d_t == nullptr) { HIP_CHECK(hipMalloc((void **)&d_t, sizeof(h))); HIP_CHECK(hipMemset(d_t, 0, sizeof(h))); }
            else {
                HIP_CHECK(hipDeviceSynchronize());
                HIP_CHECK(hipMemcpy(h, d_t, sizeof(h), hipMemcpyDeviceToHost));
                if (h[1] > 0)
                    fprintf(stderr, "gram_wave: %.0f ticks per wave, %llu waves, %llu slices, %llu nnz: %.1f ticks per nnz and wave\n",
                            (double)h[0] / h[1], h[1], h[2], h[3], (double)h[0] / (double)h[3]);
                HIP_CHECK(hipMemset(d_t, 0, sizeof(h)));
            }
            G.ticks = d_t;
        }
#endif
        // slice partials: one wavefront per slice straight from the gather (gram_wave_kernel), or the LDS-staged workgroup
        // kernel (CMFREC_HIP_GRAM_KERNEL=slice)
        poison_lds(dev.stream, dev.num_cus);
        const bool slice_kernel = switches().gram_slice;
        if (slice_kernel)
            hipLaunchKernelGGL((gram_slice_kernel<real_t, IMPLICIT>), dim3(std::min(X.n_slices, dev.num_cus * 2)), dim3(64 * GRAM_NW), 0,
                           dev.stream, P, G);
        else {
            // double precision, 48 < k <= 52 (k = 50): the two to four columns of the last block as vector products instead of
            // four matrix-core tiles per slab
            const dim3 gw(std::min((X.n_slices + 3) / 4, dev.num_cus * 4));
            const int rem = (sizeof(real_t) == 8) ? P.k - 16 * (GRAM_NTT - 1) : 0;
            launch_gram_wave(gw, dev.stream, P, G, IMPLICIT, rem);       // gram_wave_tu.hip: built with its own scheduler
        }
        poison_lds(dev.stream, dev.num_cus);
        hipLaunchKernelGGL((gram_cg_kernel<real_t, IMPLICIT>), dim3(std::min(nvh, dev.num_cus * 8)), dim3(256), 0, dev.stream, P, G);
        HIP_CHECK(hipGetLastError());
        if (tm) {
            HIP_CHECK(hipEventRecord(ev.b, dev.stream));
            tm->ev[BIN_VHEAVY].push_back(ev);
        }
        return;
    }
    VhState<real_t> V;
    V.r = X.vh_r.ptr; V.p = X.vh_p.ptr; V.r_old = X.vh_r_old.ptr; V.done = X.vh_done.ptr; V.part = X.vh_part.ptr;
    V.chunk_row = X.vh_chunk_row.ptr; V.chunk_start = X.vh_chunk_start.ptr; V.chunk_cnt = X.vh_chunk_cnt.ptr;
    V.chunk_off = X.vh_chunk_off.ptr; V.launch = X.vh_launch.ptr; V.work = X.vh_work.ptr;
    V.nvh = nvh; V.nchunks = X.n_chunks; V.nlaunch = X.n_launch;
    P.nrows = nvh;
    poison_lds(dev.stream, dev.num_cus);
    const dim3 gp(X.n_launch), bp(64 * VH_CHUNK_TILES), gu(nvh), bu(64 * VH_UPD_WAVES);
    hipLaunchKernelGGL((vh_pass_kernel<real_t, S, IMPLICIT, 0>), gp, bp, 0, dev.stream, P, V);
    hipLaunchKernelGGL((vh_update_kernel<real_t, IMPLICIT, 0, GRAMX>), gu, bu, 0, dev.stream, P, V);
    for (int step = 0; step < P.max_cg_steps; step++) {
        hipLaunchKernelGGL((vh_pass_kernel<real_t, S, IMPLICIT, 1>), gp, bp, 0, dev.stream, P, V);
        hipLaunchKernelGGL((vh_update_kernel<real_t, IMPLICIT, 1, GRAMX>), gu, bu, 0, dev.stream, P, V);
    }
    HIP_CHECK(hipGetLastError());
    if (tm) {
        HIP_CHECK(hipEventRecord(ev.b, dev.stream));
        tm->ev[BIN_VHEAVY].push_back(ev);
    }
}

// A length bin of double-precision rows as two launches by tile size (cg_kernels.hpp, NTSEL): the rows of more than 48 W entries lead
// the bin's processing order and keep two wavefronts per SIMD, the others run on the build that fits three.  One event pair around
// both; the second launch on its own counter set.  CMFREC_HIP_NT_SPLIT=0: one launch (A/B switch).
template <int S, bool IMPLICIT, int W, int RPB, bool GRAMX>
inline void launch_cg_bin_by_tile(const DeviceInfo &dev, const CgParams<real_t> &P, const SparseShard &X, int first, int count, BinTimers *tm, int bin,
                                  hipStream_t st)
{
    // (double precision: not the two-wave teams -- a workgroup of two wavefronts with its own copy of the Gramian, 28 KB, fits five
    //  times into the 160 KB of LDS, not the six that three wavefronts per SIMD would be: measured 4-7 % slower as two launches, r05_u)
#ifdef CMFREC_HIP_FLOAT
    constexpr bool by_tile = S >= CMF_CG_NT_MIN_S && CMF_CG_NT_F32 && W <= 4;
#else
    // (round 6: the eight-wave teams too -- their rows of 257..384 entries on the build for 5 / 6 entries per lane group, 168 registers:
    //  the workgroup no longer owns every register of its CU, the neighbouring stream's workgroups fit beside it)
    constexpr bool by_tile = S >= CMF_CG_NT_MIN_S && S <= CG_NTSEL_MAX_S && (W == 1 || W == 4 || W == 8);
#endif
    if (count <= 0) return;
#ifndef CMFREC_HIP_FLOAT
    // Two resident tiles per wavefront (cg_rows_kernel, NRES_ = 2) for the rows of 5 or 6 entries per lane group of the two- and the
    // eight-wave bins: 65..96 entries on ONE wavefront (four rows per workgroup share a Gramian copy; no barrier, no exchange), 257..384
    // on FOUR (two rows in flight per CU, half the per-wavefront fixed work per row).  W NRES is what it was, so a row keeps its tile
    // and differs only in the order its tile partials are added.  The upper ranges stay on their teams, the two-wave one as a launch
    // of the bodies for 7 and 8 entries (CMFREC_HIP_NT_SPLIT=0: of every body, as that switch has it everywhere -- the same bits).
    // CMFREC_HIP_TWO_TILES=0: the routing before; 2 / 3: only the two- / the eight-wave bin's rows move (A/B switch).
    // (block systems with S = 7: those two instantiations keep 16-44 bytes of scratch per lane and stay where they were)
    constexpr bool two_tiles = S >= CMF_CG_NT_MIN_S && S <= CG_NTSEL_MAX_S && (W == 2 || W == 8) && RPB == 1 && !(GRAMX && S == CG_NTSEL_MAX_S);
    if constexpr (two_tiles) {
        const int tt = switches().two_tiles;
        if (tt == 1 || tt == (W == 2 ? 2 : 3)) {
            const int n_hi = std::min(count, std::max(0, X.n_gt_low[W == 2 ? 1 : 3] - first));
            EventPair ev{nullptr, nullptr};
            if (tm) { HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b)); HIP_CHECK(hipEventRecord(ev.a, st)); }
            if (switches().nt_split) launch_cg_bin<S, IMPLICIT, W, 1, GRAMX, 0, 2>(dev, P, first, n_hi, nullptr, bin, st);
            else launch_cg_bin<S, IMPLICIT, W, 1, GRAMX>(dev, P, first, n_hi, nullptr, bin, st);
            launch_cg_bin<S, IMPLICIT, W / 2, (W == 2) ? 4 : 1, GRAMX, 2, 1>(dev, P, first + n_hi, count - n_hi, nullptr, bin, st, NBINS + 2 + bin);
            if (tm) { HIP_CHECK(hipEventRecord(ev.b, st)); tm->ev[bin].push_back(ev); }
            return;
        }
    }
#endif
    if constexpr (by_tile) {
        if (switches().nt_split) {
            const int n_hi = std::min(count, std::max(0, X.n_gt_low[W == 1 ? 0 : W == 2 ? 1 : W == 4 ? 2 : 3] - first));
            EventPair ev{nullptr, nullptr};
            if (tm) { HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b)); HIP_CHECK(hipEventRecord(ev.a, st)); }
            launch_cg_bin<S, IMPLICIT, W, RPB, GRAMX, 0, 2>(dev, P, first, n_hi, nullptr, bin, st);
            launch_cg_bin<S, IMPLICIT, W, RPB, GRAMX, 0, 1>(dev, P, first + n_hi, count - n_hi, nullptr, bin, st, NBINS + 2 + bin);
            if (tm) { HIP_CHECK(hipEventRecord(ev.b, st)); tm->ev[bin].push_back(ev); }
            return;
        }
    }
    launch_cg_bin<S, IMPLICIT, W, RPB, GRAMX>(dev, P, first, count, tm, bin, st);
}

// one of the register-tiled bins (8 / 4 / 2 / 1 wavefronts per row)
template <int S, bool IMPLICIT, bool GRAMX>
inline void launch_cg_any_bin(const DeviceInfo &dev, const CgParams<real_t> &P, const SparseShard &X, BinTimers *tm, int bin, hipStream_t st)
{
    const int first = X.bin_first[bin], count = X.bin_rows[bin];
    switch (bin) {
        case BIN_HEAVY:
#ifdef CMFREC_HIP_FLOAT
            {
                // single precision: rows of 257..512 entries on four waves with two resident tiles each (cg_rows_kernel, NRES_),
                // the longer ones on eight; one event pair around both launches, the second on a spare counter set
                const int n_long8 = std::min(count, std::max(0, X.n_gt512 - first));
                EventPair ev{nullptr, nullptr};
                if (tm) { HIP_CHECK(hipEventCreate(&ev.a)); HIP_CHECK(hipEventCreate(&ev.b)); HIP_CHECK(hipEventRecord(ev.a, st)); }
                launch_cg_bin<S, IMPLICIT, 8, 1, GRAMX>(dev, P, first, n_long8, nullptr, bin, st);
                launch_cg_bin<S, IMPLICIT, 4, 1, GRAMX, 2>(dev, P, first + n_long8, count - n_long8, nullptr, bin, st, NBINS);
                if (tm) { HIP_CHECK(hipEventRecord(ev.b, st)); tm->ev[bin].push_back(ev); }
                break;
            }
            // (double precision: rows of 257..384 entries on six-wave teams were measured slower -- 0.245 -> 0.27 ms for C2's items,
            //  0.184 -> 0.203 for its users, profiles/r04/r04_u -- a second launch per bin costs more than the idle waves)
#endif
            launch_cg_bin_by_tile<S, IMPLICIT, 8, 1, GRAMX>(dev, P, X, first, count, tm, bin, st); break;
        case BIN_MED4: launch_cg_bin_by_tile<S, IMPLICIT, 4, 1, GRAMX>(dev, P, X, first, count, tm, bin, st); break;
        case BIN_MED2: launch_cg_bin_by_tile<S, IMPLICIT, 2, 1, GRAMX>(dev, P, X, first, count, tm, bin, st); break;
        default: launch_cg_bin_by_tile<S, IMPLICIT, 1, 4, GRAMX>(dev, P, X, first, count, tm, bin, st); break;
    }
}

template <int S, bool IMPLICIT, bool GRAMX = false>
inline void launch_cg_S(const DeviceInfo &dev, const CgParams<real_t> &P, const SparseShard &X, BinTimers *tm)
{
    // Few split rows (less than about one round of workgroups per pass: the users of C2) make their launch sequence --
    // 2 kernels per CG pass -- a chain of latencies, 0.08 ms with next to no work; it then runs on the second stream
    // beside the other bins.  Many split rows (the items of C2) fill the chip by themselves and stay in line.
    if (dev.row_counter.n < ROW_COUNTER_INTS) const_cast<DeviceInfo &>(dev).row_counter.alloc(ROW_COUNTER_INTS);
    HIP_CHECK(hipMemsetAsync(dev.row_counter.ptr, 0, ROW_COUNTER_INTS * sizeof(int), dev.stream));   // work counters of the bins
    // (The Gramian path is two launches, not two per pass, and its slices are short when the rows are few: it stays in line.)
    const bool vh_aside = X.bin_rows[BIN_VHEAVY] > 0 && X.vh_runs_aside(dev.num_cus) && !vh_takes_gram<GRAMX>(P.k, X);
    // A shard that is one of several parts of a block (multi-GPU overlap, session.hip) has a quarter of the rows per
    // launch, so ramp-up and tail of every bin weigh four times as much: its bins alternate between the two streams,
    // the next bin fills the CUs the previous one is vacating.  (Not for whole blocks: there the per-bin event timings
    // feed the roofline report and must not overlap.)
    const bool alt = X.is_part;
    DeviceInfo &d = const_cast<DeviceInfo &>(dev);
    // Round 3: the bins of a half-step side by side.  Every bin is a persistent launch whose teams claim rows from a counter, so
    // a launch that shares the chip with its neighbours just takes its rows as workgroups become resident; what disappears are
    // the ramp-up and the tail of six launches per half-step, during which most CUs idle (C2: 4.36 -> 4.09 ms with two streams).
    // CMFREC_HIP_BINS_PAR = number of streams (1: in line as before; default cg_bin_streams()).  The per-bin events then
    // measure overlapping spans.
    const int npar = cg_bin_streams();
    if (npar > 1 && !(vh_aside || alt)) {
        d.ensure_bin_streams(npar - 1);
        hipStream_t ss[DeviceInfo::MAX_BIN_STREAMS + 1];
        ss[0] = dev.stream;
        for (int i = 1; i < npar; i++) ss[i] = d.bin_streams[i - 1];
        HIP_CHECK(hipEventRecord(d.fork_ev, dev.stream));
        for (int i = 1; i < npar; i++) HIP_CHECK(hipStreamWaitEvent(ss[i], d.fork_ev, 0));
        // Bins onto streams: longest estimated bin first, each to the stream with the least work so far (LPT), so that the
        // streams end together and no bin's tail runs alone.  Estimate = entries + a per-row share in entry equivalents, fitted
        // to the in-line times of the bins of C2 (profiles/r03_f, both half-steps: ~10.5 M entries per ms everywhere, plus ~12 ns
        // per row of an 8-wave team, ~1 ns per row of the tiny bin, < 1 ns elsewhere).
        static const double row_equiv[NBINS] = {0.0, 126.0, 7.0, 7.0, 0.0, 11.5};
        double cost[NBINS], load[DeviceInfo::MAX_BIN_STREAMS + 1] = {0, 0, 0, 0, 0, 0};
        int order_b[NBINS];
        for (int b = 0; b < NBINS; b++) {
            cost[b] = (double)X.bin_nnz[b] + row_equiv[b] * (double)X.bin_rows[b];
            order_b[b] = b;
        }
        std::sort(order_b, order_b + NBINS, [&](int a, int b2) { return cost[a] > cost[b2]; });
        for (int q = 0; q < NBINS; q++) {
            const int b = order_b[q];
            if (X.bin_rows[b] <= 0) continue;
            int si = 0;
            for (int i = 1; i < npar; i++) if (load[i] < load[si]) si = i;
            load[si] += cost[b];
            if (b == BIN_VHEAVY) launch_cg_vheavy<S, IMPLICIT, GRAMX>(dev, P, X, tm, ss[si]);
            else if (b == BIN_TINY) launch_cg_tiny<S, IMPLICIT, GRAMX>(dev, P, X.bin_first[BIN_TINY], X.bin_rows[BIN_TINY], tm, ss[si], X.n_gt16);
            else launch_cg_any_bin<S, IMPLICIT, GRAMX>(dev, P, X, tm, b, ss[si]);
        }
        for (int i = 1; i < npar; i++) {
            HIP_CHECK(hipEventRecord(d.bin_join[i - 1], ss[i]));
            HIP_CHECK(hipStreamWaitEvent(dev.stream, d.bin_join[i - 1], 0));
        }
        return;
    }
    if (vh_aside || alt) {
        d.ensure_aux();
        HIP_CHECK(hipEventRecord(d.fork_ev, dev.stream));
        HIP_CHECK(hipStreamWaitEvent(d.aux_stream, d.fork_ev, 0));
    }
    hipStream_t s0 = dev.stream, s1 = alt ? d.aux_stream : dev.stream;
    launch_cg_vheavy<S, IMPLICIT, GRAMX>(dev, P, X, tm, (vh_aside || (alt && X.is_part)) ? d.aux_stream : dev.stream);
    // then longest rows first: they are the longest-running teams
    launch_cg_any_bin<S, IMPLICIT, GRAMX>(dev, P, X, tm, BIN_HEAVY, s0);
    launch_cg_any_bin<S, IMPLICIT, GRAMX>(dev, P, X, tm, BIN_MED4, s1);
    launch_cg_any_bin<S, IMPLICIT, GRAMX>(dev, P, X, tm, BIN_MED2, s0);
    launch_cg_any_bin<S, IMPLICIT, GRAMX>(dev, P, X, tm, BIN_LIGHT, s1);
    launch_cg_tiny<S, IMPLICIT, GRAMX>(dev, P, X.bin_first[BIN_TINY], X.bin_rows[BIN_TINY], tm, s0, X.n_gt16);
    if (vh_aside || alt) {
        HIP_CHECK(hipEventRecord(d.join_ev, d.aux_stream));
        HIP_CHECK(hipStreamWaitEvent(dev.stream, d.join_ev, 0));
    }
}

template <int NF, bool IMPLICIT>
inline void launch_cg_generic(const DeviceInfo &dev, CgParams<real_t> P, const SparseShard &X, int first = 0, bool all_rows = false)
{
    int count = (P.kc > 0 || P.Bi != nullptr || all_rows) ? X.nrows : X.n_nonempty;   // rows without entries still have side information / get zeroed
    if (count <= first) return;
    // rows of 129 non-zeros and more (they lead the processing order): a workgroup per row -- sixteen wavefronts for the
    // rows beyond 1024 non-zeros (the longest row is the critical path of the launch: C1's items with implicit features
    // 31 -> 13 ms), four for the others; the rest: a wavefront per row
    const int nteam = std::min(count, X.bin_first[BIN_MED2]);
    const int nvh = std::min(nteam, X.bin_rows[BIN_VHEAVY]);
    poison_lds(dev.stream, dev.num_cus);
    if (nvh > first) {
        P.row_first = first; P.nrows = nvh;
        hipLaunchKernelGGL((cg_rows_generic_kernel<real_t, NF, IMPLICIT, 16>), dim3(std::min(nvh - first, dev.num_cus * 2)), dim3(1024), 0,
                           dev.stream, P);
    }
    if (nteam > std::max(nvh, first)) {
        P.row_first = std::max(nvh, first); P.nrows = nteam;
        hipLaunchKernelGGL((cg_rows_generic_kernel<real_t, NF, IMPLICIT, 4>), dim3(std::min(nteam - P.row_first, dev.num_cus * 8)), dim3(256), 0,
                           dev.stream, P);
    }
    if (count > std::max(nteam, first)) {
        P.row_first = std::max(nteam, first); P.nrows = count;
        int grid = std::min((count - P.row_first + 3) / 4, dev.num_cus * 8);
        hipLaunchKernelGGL((cg_rows_generic_kernel<real_t, NF, IMPLICIT, 1>), dim3(grid), dim3(256), 0, dev.stream, P);
    }
    HIP_CHECK(hipGetLastError());
}

#ifdef CMF_CG_TICKS
// 8 kernel families x 4 sums (cg_kernels.hpp, CgParams::ticks); one buffer per process, read and cleared by cmfrec_hip_debug_cg_ticks
unsigned long long *cg_ticks_buffer()
{
    static unsigned long long *buf = nullptr;
    if (buf == nullptr) {
        HIP_CHECK(hipMalloc((void **)&buf, 32 * sizeof(unsigned long long)));
        HIP_CHECK(hipMemset(buf, 0, 32 * sizeof(unsigned long long)));
    }
    return buf;
}
#endif

int launch_cg(const DeviceInfo &dev, const CgCall &c, const SparseShard &X, BinTimers *tm)
{
    CgParams<real_t> P;
    P.A = c.A; P.lda = c.lda; P.B = c.B; P.ldb = c.ldb; P.k = c.k;
    P.indptr = X.p.ptr; P.indices = X.i.ptr; P.values = X.v.ptr;
    P.bias_sub = c.bias_sub; P.order = X.order.ptr; P.desc = X.desc.ptr; P.nrows = 0; P.BtB = c.BtB;
    if (!c.implicit && X.weighted()) { P.weights = X.w.ptr; P.wsum = X.wsum.ptr; }
    P.lam = c.lam; P.lam_last = c.lam_last;
    P.scale_lam = c.scale_lam; P.scale_bias_const = c.scale_bias_const;
    P.max_cg_steps = c.max_cg_steps;
    P.precond = c.precond ? 1 : 0;
    P.koff = c.koff; P.kc = c.kc; P.CtC = c.CtC; P.UC = c.UC; P.w_side = c.w_side;
    P.rows_with_u = c.rows_with_u; P.p_side = c.p_side; P.scale_lam_sideinfo = c.scale_lam_sideinfo ? 1 : 0;
    if (c.X2) { P.indptr2 = c.X2->p.ptr; P.indices2 = c.X2->i.ptr; P.values2 = c.X2->v.ptr; P.C2 = c.C2; }
    P.Bi = c.Bi; P.BiTBi = c.BiTBi; P.ki = c.ki; P.w_imp = c.w_imp;
#ifdef CMF_CG_DEBUG
    P.dbg = switches().debug_skip;
#endif
#ifdef CMF_CG_TICKS
    P.ticks = cg_ticks_buffer();
#endif
    const int S = (c.k + 7) / 8;
    if (c.values_override != nullptr) P.values = c.values_override;
    if (c.weights_override != nullptr) { P.weights = c.weights_override; P.wsum = X.wsum_naz.ptr; }     // (NA_as_zero_X with weights only)
    if (c.wsum_override != nullptr) P.wsum = c.wsum_override;
    if (c.Gx != nullptr && (c.kc > 0 || c.X2 != nullptr || c.Bi != nullptr)) {
        // block systems whose X block is a matrix every row shares (NA_as_zero_X: collective_block_cg's NA_as_zero_X branches with the
        // precomputed B^T B, collective.c:2430-2445, :2700-2760): the lane <-> unknown kernel with CgParams::gx, every row of the launch
        if (c.implicit || c.skip_first != 0) {
            g_last_error = "cmfrec_hip: block CG with a shared matrix: the explicit model";
            return 2;
        }
        P.BtB = c.Gx; P.rconst = c.rconst_x; P.ldr = c.ldr_x; P.gx = c.gx_all_rows ? 2 : 1;   // 2: the constant of the biases / the mean exists
        const int NFb = (c.koff + c.k + 63) / 64;
        switch (NFb) {
            case 1: launch_cg_generic<1, false>(dev, P, X, 0, true); return 0;
            case 2: launch_cg_generic<2, false>(dev, P, X, 0, true); return 0;
            case 3: launch_cg_generic<3, false>(dev, P, X, 0, true); return 0;
            default: break;
        }
        g_last_error = "cmfrec_hip: block CG with a shared matrix: at most 192 unknowns per row";
        return 2;
    }
    if (c.Gx != nullptr && c.precond) {
        // ... with the Jacobi preconditioner (factors_explicit_pcg_NA_as_zero_weighted, common.c:1443-1613): the lane <-> unknown kernel
        // with the shared matrix and the per-row constant (CgParams::gx), any width it takes
        if (c.implicit || c.kc > 0 || c.Bi != nullptr || c.koff != 0 || c.skip_first != 0 || c.X2 != nullptr) {
            g_last_error = "cmfrec_hip: preconditioned CG with a shared matrix: plain explicit rows";
            return 2;
        }
        P.BtB = c.Gx; P.rconst = c.rconst_x; P.ldr = c.ldr_x; P.gx = 1;
        const int NFx = (c.k + 63) / 64;
        switch (NFx) {
            case 1: launch_cg_generic<1, false>(dev, P, X, 0, c.gx_all_rows); return 0;
            case 2: launch_cg_generic<2, false>(dev, P, X, 0, c.gx_all_rows); return 0;
            case 3: launch_cg_generic<3, false>(dev, P, X, 0, c.gx_all_rows); return 0;
            default: break;
        }
        g_last_error = "cmfrec_hip: preconditioned CG with a shared matrix: at most 192 unknowns per row";
        return 2;
    }
    if (c.Gx != nullptr) {
        // shared matrix + per-row constant on the GRAMX builds (no block structure: the explicit model's own lambda rules apply)
        if (c.implicit || c.precond || S > 8 || c.kc > 0 || c.Bi != nullptr || c.koff != 0 || c.skip_first != 0) {
            g_last_error = "cmfrec_hip: CG with a shared matrix: plain explicit rows of at most 64 unknowns, no preconditioner";
            return 2;
        }
        P.BtB = c.Gx; P.rconst = c.rconst_x; P.ldr = c.ldr_x;
#define CMF_XCASE(SS) case SS: launch_cg_S<SS, false, true>(dev, P, X, tm); break;
        switch (S) {
            CMF_XCASE(1) CMF_XCASE(2) CMF_XCASE(3) CMF_XCASE(4)
            CMF_XCASE(5) CMF_XCASE(6) CMF_XCASE(7) CMF_XCASE(8)
        }
#undef CMF_XCASE
        HIP_CHECK(hipGetLastError());
        return 0;
    }
    // Block systems (dense side information on EVERY row of the launch and / or implicit features, no k_user offset) on the
    // tiled kernels: the weighted Gramian w C^T C + w_i Bi^T Bi acts on the unknowns like the implicit model's B^T B, the row's
    // constant w (U C)_row + w_i sum Bi_j joins the first residual (GRAMX builds, cg_kernels.hpp).  Rows without entries
    // (still solved from their side information / zeroed) go through the generic kernel afterwards.
    const bool block = (c.kc > 0 || c.Bi != nullptr);
    const bool tiled_block = block && cg_variant_from_env() != CgVariant::Generic && !c.implicit && c.koff == 0 && !c.precond && c.skip_first == 0 &&
                             S <= 8 && c.X2 == nullptr && (c.kc == 0 || (c.rows_with_u >= X.nrows && c.CtC != nullptr && c.UC != nullptr)) &&
                             (c.Bi == nullptr || (c.gsum != nullptr && c.BiTBi != nullptr)) && c.kc <= c.k && c.ki <= c.k;
    if (tiled_block) {
        DeviceInfo &d = const_cast<DeviceInfo &>(dev);
        d.cg_gfull.alloc_at_least((size_t)c.k * c.k);
        d.cg_rconst.alloc_at_least((size_t)std::max(X.nrows, 1) * c.k);
        hipLaunchKernelGGL(block_gram_kernel<real_t>, dim3((c.k * c.k + 255) / 256), dim3(256), 0, dev.stream, c.CtC, c.kc, c.w_side, c.BiTBi,
                           c.ki, c.w_imp, c.k, d.cg_gfull.ptr);
        hipLaunchKernelGGL(block_rconst_kernel<real_t>, dim3((unsigned)(((size_t)X.nrows * c.k + 255) / 256)), dim3(256), 0, dev.stream, c.UC, c.kc,
                           c.w_side, c.gsum, c.ki, c.w_imp, c.k, (size_t)X.nrows, d.cg_rconst.ptr);
        P.BtB = d.cg_gfull.ptr; P.rconst = d.cg_rconst.ptr; P.ldr = (size_t)c.k;
#define CMF_BCASE(SS) case SS: launch_cg_S<SS, false, true>(dev, P, X, tm); break;
        switch (S) {
            CMF_BCASE(1) CMF_BCASE(2) CMF_BCASE(3) CMF_BCASE(4)
            CMF_BCASE(5) CMF_BCASE(6) CMF_BCASE(7) CMF_BCASE(8)
        }
#undef CMF_BCASE
        if (X.nrows > X.n_nonempty) {
            // rows without entries: solved from their side information alone / zeroed (collective.c:1258-1268), one wavefront per row
            CgParams<real_t> Pe = P;
            Pe.BtB = c.BtB; Pe.rconst = nullptr;
            Pe.row_first = X.n_nonempty; Pe.nrows = X.nrows;
            const int cnt = X.nrows - X.n_nonempty;
            const int NFe = (c.koff + c.k + 63) / 64;
            const int grid = std::min((cnt + 3) / 4, dev.num_cus * 8);
            switch (NFe) {
                case 1: hipLaunchKernelGGL((cg_rows_generic_kernel<real_t, 1, false, 1>), dim3(grid), dim3(256), 0, dev.stream, Pe); break;
                default: hipLaunchKernelGGL((cg_rows_generic_kernel<real_t, 2, false, 1>), dim3(grid), dim3(256), 0, dev.stream, Pe); break;
            }
        }
        HIP_CHECK(hipGetLastError());
        return 0;
    }
    // the Jacobi-preconditioned variants (not a default anywhere in the reference) and the remaining block systems run on the
    // generic kernel
    const bool generic = cg_variant_from_env() == CgVariant::Generic || S > 8 || c.precond || c.kc > 0 || c.Bi != nullptr || c.skip_first > 0;
    if (!generic) {
#define CMF_CASE(SS)                                                        \
    case SS:                                                                \
        if (c.implicit) launch_cg_S<SS, true>(dev, P, X, tm);               \
        else            launch_cg_S<SS, false>(dev, P, X, tm);              \
        return 0;
        switch (S) {
            CMF_CASE(1) CMF_CASE(2) CMF_CASE(3) CMF_CASE(4)
            CMF_CASE(5) CMF_CASE(6) CMF_CASE(7) CMF_CASE(8)
        }
#undef CMF_CASE
    }
    const int NF = (c.koff + c.k + 63) / 64;
#define CMF_GCASE(NN)                                                       \
    case NN:                                                                \
        if (c.implicit) launch_cg_generic<NN, true>(dev, P, X, c.skip_first);  \
        else            launch_cg_generic<NN, false>(dev, P, X, c.skip_first); \
        return 0;
    switch (NF) {
        CMF_GCASE(1) CMF_GCASE(2) CMF_GCASE(3) CMF_GCASE(4) CMF_GCASE(5)
    }
#undef CMF_GCASE
    g_last_error = "cmfrec_hip: CG path supports k <= 320 per solved matrix";
    return 2;
}

// CG of the explicit model beyond 64 unknowns (k_t <= 129): through the row's Gramian (gram_cg_wide_kernels.hpp) instead of the
// lane <-> unknown kernel.  -1: not applicable (the caller takes launch_cg).  CMFREC_HIP_CG_KERNEL=generic keeps the generic kernel
// (A/B switch and on-device cross-check).
int launch_cg_wide(const DeviceInfo &dev, const CgCall &c, const SparseShard &X)
{
    const bool border = (c.k > 16) && ((c.k - 1) % 16 == 0);
    const int nbw = (c.k - (border ? 1 : 0) + 15) / 16;
    if (c.implicit || c.k <= 64 || nbw > 8 || c.precond || c.X2 != nullptr || c.Bi != nullptr || c.koff != 0 || X.weighted() ||
        dev.nonneg_now || dev.l1_now != (real_t)0 || dev.l1_last_now != (real_t)0 ||      // (launch_chol's wave path is off then)
        cg_variant_from_env() == CgVariant::Generic || switches().chol == 1 ||
        (c.kc > 0 && (c.CtC == nullptr || c.UC == nullptr || c.kc > c.k)) || gcw_lds_elems<real_t>(c.k) * sizeof(real_t) > (size_t)160 * 1024)
        return -1;
    CgParams<real_t> P;
    P.A = c.A; P.lda = c.lda; P.B = c.B; P.ldb = c.ldb; P.k = c.k;
    P.indptr = X.p.ptr; P.indices = X.i.ptr; P.values = X.v.ptr;
    P.bias_sub = c.bias_sub; P.order = X.order.ptr; P.desc = X.desc.ptr; P.nrows = 0; P.BtB = nullptr;
    P.lam = c.lam; P.lam_last = c.lam_last;
    P.scale_lam = c.scale_lam; P.scale_bias_const = c.scale_bias_const;
    P.max_cg_steps = c.max_cg_steps; P.precond = 0;
    P.koff = 0; P.kc = c.kc; P.CtC = c.CtC; P.UC = c.UC; P.w_side = c.w_side;
    P.rows_with_u = c.rows_with_u; P.p_side = c.p_side; P.scale_lam_sideinfo = c.scale_lam_sideinfo ? 1 : 0;
    // The Gramian costs k_t / 8 times the products of the CG's four passes per entry and saves three of the four gathers and the
    // generic kernel's wave-wide reduction per gathered row: it pays on the long rows (config 3's items under CG: 18.1 -> 6.8 ms)
    // and loses on the short ones (its users, 143 entries per row on average: 8.6 -> 15.8 ms).  So the rows beyond 256 entries --
    // they lead the processing order -- take it, the others stay on the lane <-> unknown kernel (CgCall::skip_first).
    const int n_wide = X.rows_longer_than(256, X.n_nonempty);
    if (n_wide <= 0) return -1;
    CholCall cc{c.A, c.lda, c.B, c.ldb, c.k, 0, c.bias_sub, nullptr, 0, 0, 0, c.lam, c.lam_last, c.scale_lam, c.scale_lam_sideinfo,
                c.scale_bias_const, CHOL_EXPLICIT};
    cc.cg_wide = &P;
    cc.row_limit = n_wide;
    int rc = launch_chol(dev, cc, &X);                    // positions [0, n_wide)
    if (rc) return rc;
    CgCall rest = c;
    rest.skip_first = n_wide;
    return launch_cg(dev, rest, X, nullptr);              // the shorter rows, and a block system's rows without entries
}
int launch_cg_any(const DeviceInfo &dev, const CgCall &c, const SparseShard &X, BinTimers *tm)
{
    const int rc = launch_cg_wide(dev, c, X);
    return rc >= 0 ? rc : launch_cg(dev, c, X, tm);
}

}  // namespace cmfhip
