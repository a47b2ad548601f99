// topn_cand_kernels.hpp -- batched top-N over per-user candidate lists: topn_cand_kernel.
//
// The batch form of the reference's include_ix: user u is ranked over its own list L_u (CSR over the users, each list ascending
// and free of duplicates) and gets exactly what topn_kernel / topn_wide_kernel would return with every item outside L_u in its
// exclusion list -- score(u, i) = A_u . B_i (+ biasB[i]), descending, ties to the lower id, -1 / -inf where fewer than n_top
// remain, a NaN score never enters, an id outside [0, n) never enters.  An exclusion list may come along: a candidate in it is dropped.
//
//   wavefront  = one user at a time, handed out by a work counter in device memory (one vector atomic per user by lane 0) in
//                the order of `order`, the users by descending list length (the host sorts them): the lists are of very
//                different lengths, a stride would leave the launch waiting for the wavefront that drew the long ones, and a
//                long list that starts last is the whole tail of the launch
//   user side  : the user's row sits in registers for the whole list, in the piece <-> lane map of score_pairs_kernel
//                (predict_kernels.hpp): G = score_group_width(k) lanes per candidate, lane g of a group holds pieces g, g + G, ...
//                (at most three pieces: G < 64 covers the row in one round)
//   item side  : a step scores 64 / G candidates, each group gathering its candidate's row of the ranker's packed B 16 bytes per
//                lane (ldb = topnw_kp(k): rows 16-byte aligned, whole pieces); SCORE_STEPS steps are in flight -- their row
//                loads, then the arithmetic -- and their ids were loaded one round of steps ahead, so a round waits for one
//                dependent load, not two
//   score      : the products of score_pairs_kernel in its order, its butterfly (score_group_sum), then + biasB[i] (+ 0, the
//                scorer's glob_mean): the value cmfrec_hip_score_pairs returns for the same two rows with biasA = NULL and
//                glob_mean = 0, whatever the candidate's place in its list, the user's place in the batch or the launch shape
//   selection  : per wavefront in LDS a sorted list of NP = max(32, pow2(n_top)) entries and TOPNC_SLOTS candidate slots.  Lane 0 of
//                a group offers its score if it is not below the user's current n_top-th best (-inf until the first merge) and,
//                then, not in the exclusion list (binary search); the offers of a step take consecutive slots (ballot and prefix
//                count, no atomics).  When the slots are full, and at the end of the list: the slots are sorted (bitonic, as wide
//                as they are filled), folded into the list by the first stage of a bitonic merge of (list descending |
//                candidates ascending), whose better half alone is kept, and the merge is finished -- topn_wide_kernel's
//                scheme.  Offers that found no slot are made again after the merge, against the new threshold.  The order
//                (score descending, id ascending) is total, so which offer took which slot does not show in the result.
// Static LDS, vector stores only; the wavefronts of a workgroup never meet (no __syncthreads).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "predict_kernels.hpp"
#include "topn_kernels.hpp"

namespace cmfhip {

constexpr int TOPNC_NW = 4;                   // wavefronts per workgroup
constexpr int TOPNC_TH = 64 * TOPNC_NW;
constexpr int TOPNC_SLOTS = 128;              // candidate slots per wavefront
constexpr int TOPNC_LS = TOPN_NMAX + TOPNC_SLOTS;
constexpr int TOPNC_KMAX = 272;               // the widest row the register copy of the user is sized for

__host__ __device__ inline int topnc_np(int n_top) { int np = 32; while (np < n_top) np <<= 1; return np; }

template <typename T>
struct TopnCandParams {
    const T *A; size_t lda; int nu;          // users' factors, first used column
    const T *B; size_t ldb; int n, k;        // item factors: ldb = topnw_kp(k), columns [k, ldb) zero, rows 16-byte aligned
    const T *biasB;                          // or null
    const size_t *cand_p; const int *cand_i; // per-user candidate lists, each ascending and free of duplicates
    const size_t *excl_p; const int *excl_i; // per-user exclusion lists, each sorted ascending; or null
    int n_top;
    int *out_ids; T *out_scores;             // [nu, n_top]; out_scores may be null
    unsigned *next;                          // work counter, zero before the launch
    const int *order;                        // the users in the order they are handed out (longest list first)
};

// what one wavefront's LDS operations wrote is read by its other lanes after this
__device__ __forceinline__ void topnc_lds_sync()
{
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// The c (1 .. TOPNC_SLOTS) filled slots csc / cid (the free ones hold -inf) into the sorted list sc / id [NP]; the slots are
// left free.  Returns the score of the n_top-th best (-inf while the list is shorter).  Wave-uniform.
template <typename T>
__device__ __forceinline__ T topnc_merge(T *sc, int *id, T *csc, int *cid, int NP, int ntop, int c, int lane)
{
    const T NEG = -INFINITY;
    int W = 1;
    while (W < c) W <<= 1;                                                   // <= TOPNC_SLOTS
    for (int size = 2; size <= W; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = lane; e < W / 2; e += 64) {
                const int i = 2 * e - (e & (stride - 1)), j = i + stride;
                const bool up = ((i & size) == 0) || (size == W);            // final merge: best first everywhere
                const T si = csc[i], sj = csc[j]; const int ii = cid[i], ij = cid[j];
                const bool swap = up ? topn_before(sj, ij, si, ii) : topn_before(si, ii, sj, ij);
                if (swap) { csc[i] = sj; csc[j] = si; cid[i] = ij; cid[j] = ii; }
            }
            topnc_lds_sync();
        }
    }
    // (list descending | -inf ... | the NP best candidates ascending) is bitonic; the first stage of its merge leaves the better
    // of list[NP - 1 - j] and candidate j in the list half, which holds the best NP and is bitonic again
    for (int j = lane; j < W; j += 64) {
        if (j < NP) {
            const int i = NP - 1 - j;
            const T sl = sc[i], sb = csc[j]; const int il = id[i], ib = cid[j];
            if (topn_before(sb, ib, sl, il)) { sc[i] = sb; id[i] = ib; }
        }
        csc[j] = NEG; cid[j] = 0x7fffffff;
    }
    topnc_lds_sync();
    for (int stride = NP >> 1; stride > 0; stride >>= 1) {
        for (int e = lane; e < NP / 2; e += 64) {
            const int i = 2 * e - (e & (stride - 1)), j = i + stride;
            const T si = sc[i], sj = sc[j]; const int ii = id[i], ij = id[j];
            if (topn_before(sj, ij, si, ii)) { sc[i] = sj; sc[j] = si; id[i] = ij; id[j] = ii; }
        }
        topnc_lds_sync();
    }
    for (int e = ntop + lane; e < NP; e += 64) { sc[e] = NEG; id[e] = 0x7fffffff; }       // keep the best n_top
    topnc_lds_sync();
    return sc[ntop - 1];
}

template <typename T, int G>
__global__ void __launch_bounds__(TOPNC_TH)
topn_cand_kernel(const TopnCandParams<T> P)
{
    constexpr int Ve = 16 / (int)sizeof(T), PS = 64 / G, U = SCORE_STEPS;
    // pieces per lane: a group narrower than the wavefront covers its row in one round
    constexpr int R = G < 64 ? 1 : ((TOPNC_KMAX + Ve - 1) / Ve + 63) / 64;
    __shared__ T ssc[TOPNC_NW][TOPNC_LS];                          // per wavefront: [0, NP) sorted list, [NP, NP + SLOTS) candidates
    __shared__ int sid[TOPNC_NW][TOPNC_LS];
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int kk = P.k, ntop = P.n_top, NP = topnc_np(ntop);
    const int rounds = ((kk + Ve - 1) / Ve + G - 1) / G;           // <= R (the host checks k <= TOPNC_KMAX)
    const T NEG = -INFINITY;
    T *sc = ssc[wave]; int *id = sid[wave];
    T *csc = sc + NP; int *cid = id + NP;
    for (int e = lane; e < TOPNC_LS; e += 64) { sc[e] = NEG; id[e] = 0x7fffffff; }
    topnc_lds_sync();
    // (the loops over users, steps and rounds are wavefront-uniform: all 64 lanes reach the cross-lane moves of the butterfly)
    for (;;) {
        int u = 0;
        if (lane == 0) u = (int)atomicAdd(P.next, 1u);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= P.nu) break;
        u = P.order[u];
        const T *arow = P.A + (size_t)u * P.lda;
        T a[R][Ve];
#pragma unroll
        for (int rd = 0; rd < R; rd++) score_load_piece<T, false>(arow, (rd * G + g) * Ve, kk, a[rd]);   // zeros past kk
        const size_t beg = P.cand_p[u], end = P.cand_p[u + 1];
        const size_t xb = P.excl_p != nullptr ? P.excl_p[u] : 0, xe = P.excl_p != nullptr ? P.excl_p[u + 1] : 0;
        T thr = NEG;                                               // score of the current n_top-th best
        int cnt = 0;                                               // filled slots
        int cn[U];                                                 // the ids of the next round of steps
#pragma unroll
        for (int s = 0; s < U; s++) {
            const size_t pos = beg + (size_t)(s * PS + sub);
            cn[s] = pos < end ? P.cand_i[pos] : -1;
        }
        for (size_t c0 = beg; c0 < end; c0 += (size_t)(PS * U)) {
            int cc[U];
            bool ok[U];
            const T *pb[U];
            T bb[U], acc[U];
#pragma unroll
            for (int s = 0; s < U; s++) {
                cc[s] = cn[s];
                const size_t pos = c0 + (size_t)(PS * U + s * PS + sub);
                cn[s] = pos < end ? P.cand_i[pos] : -1;
            }
#pragma unroll
            for (int s = 0; s < U; s++) {
                ok[s] = cc[s] >= 0 && cc[s] < P.n;                 // an id out of range is decided here: none of its lanes loads
                pb[s] = P.B + (size_t)(ok[s] ? cc[s] : 0) * P.ldb;
                bb[s] = (g == 0 && ok[s] && P.biasB != nullptr) ? P.biasB[cc[s]] : (T)0;
                acc[s] = (T)0;
            }
#pragma unroll
            for (int rd = 0; rd < R; rd++) {
                if (rd < rounds) {
                    const int e0 = (rd * G + g) * Ve;
                    T b[U][Ve];
#pragma unroll
                    for (int s = 0; s < U; s++) {
                        if (ok[s] && e0 < kk) score_load_piece<T, true>(pb[s], e0, kk, b[s]);
                        else {
#pragma unroll
                            for (int e = 0; e < Ve; e++) b[s][e] = (T)0;
                        }
                    }
#pragma unroll
                    for (int s = 0; s < U; s++)
#pragma unroll
                        for (int e = 0; e < Ve; e++) {
                            const bool in = e0 + e < kk;
                            acc[s] = fma(in ? a[rd][e] : (T)0, in ? b[s][e] : (T)0, acc[s]);
                        }
                }
            }
            T sv[U];
#pragma unroll
            for (int s = 0; s < U; s++) {
                sv[s] = score_group_sum<G>(acc[s]);
                if (P.biasB != nullptr) sv[s] += bb[s];
                sv[s] += (T)0;                                     // the scorer's "+ glob_mean" at zero (-0 becomes +0 there too)
            }
#pragma unroll
            for (int s = 0; s < U; s++) {
                const int item = cc[s];
                bool pend = g == 0 && ok[s] && sv[s] >= thr;       // NaN never enters
                if (pend && P.excl_p != nullptr) {                 // sorted list of the user: binary search
                    size_t lo = xb, hi = xe;
                    while (lo < hi) {
                        const size_t mid = (lo + hi) >> 1;
                        if (P.excl_i[mid] < item) lo = mid + 1; else hi = mid;
                    }
                    if (lo < xe && P.excl_i[lo] == item) pend = false;
                }
                for (;;) {
                    const unsigned long long mask = __ballot(pend);
                    if (mask == 0) break;                          // uniform
                    const int pos = cnt + __popcll(mask & ((1ull << lane) - 1ull));
                    if (pend && pos < TOPNC_SLOTS) { csc[pos] = sv[s]; cid[pos] = item; pend = false; }
                    cnt = min(TOPNC_SLOTS, cnt + (int)__popcll(mask));
                    if (cnt == TOPNC_SLOTS) {
                        topnc_lds_sync();
                        thr = topnc_merge(sc, id, csc, cid, NP, ntop, cnt, lane);
                        cnt = 0;
                        pend = pend && sv[s] >= thr;               // the offers without a slot, against the new threshold
                    }
                }
            }
        }
        topnc_lds_sync();
        if (cnt > 0) (void)topnc_merge(sc, id, csc, cid, NP, ntop, cnt, lane);
        for (int j = lane; j < ntop; j += 64) {
            const T s = sc[j];
            P.out_ids[(size_t)u * ntop + j] = (s == NEG) ? -1 : id[j];
            if (P.out_scores != nullptr) P.out_scores[(size_t)u * ntop + j] = s;
        }
        for (int e = lane; e < NP; e += 64) { sc[e] = NEG; id[e] = 0x7fffffff; }         // the next user starts from an empty list
        topnc_lds_sync();
    }
}

// wavefronts resident per CU by the kernel's own register and LDS use, in workgroups
template <typename T, int G>
inline int topn_cand_blocks_per_cu()
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, topn_cand_kernel<T, G>, TOPNC_TH, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    return per_cu;
}

// Launches the kernel on P.nu users (device pointers; P.next zeroed on st by the caller's memset before this).  max_waves > 0
// caps the wavefronts of the launch, rounded up to whole workgroups.  Returns the grid.
template <typename T>
inline int launch_topn_cand(hipStream_t st, int num_cus, const TopnCandParams<T> &P, int max_waves)
{
    const int G = score_group_width<T>(P.k);
    int per_cu = 4;
    switch (G) {
    case 1: per_cu = topn_cand_blocks_per_cu<T, 1>(); break;
    case 2: per_cu = topn_cand_blocks_per_cu<T, 2>(); break;
    case 4: per_cu = topn_cand_blocks_per_cu<T, 4>(); break;
    case 8: per_cu = topn_cand_blocks_per_cu<T, 8>(); break;
    case 16: per_cu = topn_cand_blocks_per_cu<T, 16>(); break;
    case 32: per_cu = topn_cand_blocks_per_cu<T, 32>(); break;
    default: per_cu = topn_cand_blocks_per_cu<T, 64>(); break;
    }
    long grid = std::min<long>(((long)P.nu + TOPNC_NW - 1) / TOPNC_NW, (long)num_cus * per_cu);
    if (max_waves > 0) grid = std::min<long>(grid, ((long)max_waves + TOPNC_NW - 1) / TOPNC_NW);
    const dim3 gr((unsigned)grid), th(TOPNC_TH);
    switch (G) {
    case 1: hipLaunchKernelGGL((topn_cand_kernel<T, 1>), gr, th, 0, st, P); break;
    case 2: hipLaunchKernelGGL((topn_cand_kernel<T, 2>), gr, th, 0, st, P); break;
    case 4: hipLaunchKernelGGL((topn_cand_kernel<T, 4>), gr, th, 0, st, P); break;
    case 8: hipLaunchKernelGGL((topn_cand_kernel<T, 8>), gr, th, 0, st, P); break;
    case 16: hipLaunchKernelGGL((topn_cand_kernel<T, 16>), gr, th, 0, st, P); break;
    case 32: hipLaunchKernelGGL((topn_cand_kernel<T, 32>), gr, th, 0, st, P); break;
    default: hipLaunchKernelGGL((topn_cand_kernel<T, 64>), gr, th, 0, st, P); break;
    }
    return (int)grid;
}

}  // namespace cmfhip
