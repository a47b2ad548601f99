// topn_split_kernels.hpp -- the full ranking of a FEW users spread over the whole device.
//
// topn_wide_kernel (topn_wide_kernels.hpp) gives the whole pass over the items to the workgroup that owns the user tile: one
// user, or any batch of up to 16 * NUT users, is one workgroup on one CU.  Here the item range is cut into slices and the grid is
// (user-tile workgroups) x (slices):
//
//   slice pass   topn_split_kernel = topn_wide_body under a fourth policy whose item_begin / item_end are the slice
//                [blockIdx.y * slice_items, ...) -- slice_items a multiple of TOPNW_ITEMS, so a slice starts on a round boundary and
//                a lane meets the items it would meet in the unsplit pass.  Item ids stay global (bias, exclusion lists and output
//                ids need no offset).  Slice s writes every user's sorted list to row block s of a scratch array
//                [slices][nu][n_top] of scores and ids: the order of topn_wide_kernel (score descending, lower id first), -inf / -1
//                where the slice had fewer admissible items, NaN never entered.
//   merge        topn_split_merge_kernel: one workgroup per user folds the `slices` lists into the final n_top.  Wavefront w
//                takes the lists w, w + NW, ... one after the other: a list that is sorted descending against the running list
//                (sorted descending, NP = max(32, pow2(n_top)) entries in LDS) is the first stage of a bitonic merge -- the better
//                of running[NP - 1 - j] and list[j] stays -- and log2(NP) compare-exchange stages finish it, exactly the fold of
//                topn_wide_body.  A list whose best entry does not beat the running n_top-th is skipped.  Then the wavefronts'
//                lists are folded pairwise (log2(NW) levels, a workgroup barrier each).  No atomics, no inter-workgroup
//                communication: the kernel simply runs behind the slice pass on the same stream.
//
// The score of a pair is the same MFMA sequence over k in whichever slice the item lies, and the order is total (ids are unique),
// so the best n_top of the union of the slices' best n_top is the unsplit list: bit for bit, ids and scores, for every slice count.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topn_wide_kernels.hpp"

namespace cmfhip {

constexpr int TOPNSP_MERGE_NW = 16;           // wavefronts of a merge workgroup, at most (a power of two)
constexpr int TOPNSP_MAX_SLICES = 4096;       // what a caller can ask for (the grid's y extent and the scratch stay small)

template <typename T>
struct TopnSplitParams : TopnWideParams<T> {  // out_ids / out_scores: the scratch [slices][nu][n_top], both non-null
    int slice_items;                          // a multiple of TOPNW_ITEMS; slice s = items [s * slice_items, min(n, (s + 1) * slice_items))
    int s0, s1;                               // the workgroup's slice: filled in by the kernel, not by the host
};

template <typename T>
struct TopnSplitPolicy : TopnWidePolicy<T> {
    using Params = TopnSplitParams<T>;
    static __device__ __forceinline__ int item_begin(const Params &P) { return P.s0; }
    static __device__ __forceinline__ int item_end(const Params &P) { return P.s1; }
};

template <typename T, int NUT>
__global__ void __launch_bounds__(TOPNW_TH)
topn_split_kernel(const TopnSplitParams<T> P0)
{
    TopnSplitParams<T> P = P0;
    const size_t block = (size_t)blockIdx.y * (size_t)P.nu * (size_t)P.n_top;
    P.s0 = (int)min((long long)blockIdx.y * P.slice_items, (long long)P.n);
    P.s1 = (int)min((long long)P.s0 + P.slice_items, (long long)P.n);
    P.out_ids += block;
    P.out_scores += block;
    topn_wide_body<T, NUT, TopnSplitPolicy<T>>(P);
}

template <typename T>
struct TopnMergeParams {
    const T *part_scores; const int *part_ids;   // [slices][nu][n_top]
    int slices, nu, n_top;
    int *out_ids; T *out_scores;                 // [nu, n_top]; out_scores may be null
};

__host__ __device__ inline int topnsp_merge_waves(int slices)
{
    int nw = 1;
    while (nw < slices && nw < TOPNSP_MERGE_NW) nw <<= 1;
    return nw;
}
__host__ __device__ inline size_t topnsp_merge_lds_bytes(int nw, int n_top, size_t sizeof_real)
{
    return (size_t)nw * topnw_np(n_top) * (sizeof_real + sizeof(int));
}

// running list (sc, id) [NP] in LDS, sorted descending <- the best NP of it and of a second sorted list whose entry j this lane
// holds in (ms[q], mi[q]) for j = lane + 64 q.  One wavefront; NP / 64 <= Q.
template <typename T, int Q>
__device__ __forceinline__ void topnsp_fold(T *sc, int *id, int NP, int lane, const T (&ms)[Q], const int (&mi)[Q])
{
#pragma unroll
    for (int q = 0; q < Q; q++) {
        const int j = lane + 64 * q;
        if (j < NP) {
            const int i = NP - 1 - j;
            if (topn_before(ms[q], mi[q], sc[i], id[i])) { sc[i] = ms[q]; id[i] = mi[q]; }
        }
    }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    for (int stride = NP >> 1; stride > 0; stride >>= 1) {
        for (int e = lane; e < NP / 2; e += 64) {
            const int i = 2 * e - (e & (stride - 1)), j = i + stride;
            const T si = sc[i], sj = sc[j]; const int ii = id[i], ij = id[j];
            if (topn_before(sj, ij, si, ii)) { sc[i] = sj; sc[j] = si; id[i] = ij; id[j] = ii; }
        }
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    }
}

// grid = nu workgroups of 64 * topnsp_merge_waves(slices) threads; LDS topnsp_merge_lds_bytes
template <typename T>
__global__ void __launch_bounds__(64 * TOPNSP_MERGE_NW)
topn_split_merge_kernel(const TopnMergeParams<T> P)
{
    constexpr int Q = TOPN_NMAX / 64;                               // list entries per lane (n_top <= TOPN_NMAX = NP at most)
    extern __shared__ __attribute__((aligned(16))) unsigned char topnsp_smem[];
    const int ntop = P.n_top, NP = topnw_np(ntop);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int u = blockIdx.x;
    T *ssc = reinterpret_cast<T *>(topnsp_smem);                    // [nw][NP]
    int *sid = reinterpret_cast<int *>(ssc + nw * NP);              // [nw][NP]
    T *sc = ssc + wave * NP; int *id = sid + wave * NP;
    const T NEG = -INFINITY;
    for (int e = lane; e < NP; e += 64) { sc[e] = NEG; id[e] = 0x7fffffff; }
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const size_t ld = (size_t)P.nu * (size_t)ntop;                  // between two slices' blocks
    const size_t row = (size_t)u * (size_t)ntop;
    T ms[Q]; int mi[Q];
    auto load = [&](int s) {
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int j = lane + 64 * q;
            const bool has = s < P.slices && j < ntop;
            ms[q] = has ? P.part_scores[(size_t)s * ld + row + j] : NEG;
            mi[q] = has ? P.part_ids[(size_t)s * ld + row + j] : 0x7fffffff;
        }
    };
    load(wave);
    for (int s = wave; s < P.slices; s += nw) {                     // wave-uniform
        T cs[Q]; int ci[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) { cs[q] = ms[q]; ci[q] = mi[q]; }
        load(s + nw);                                               // the next list is on its way during the fold
        // the list's best entry (lane 0's first) against the running n_top-th best: nothing to gain, nothing to do
        const T bs = __shfl(cs[0], 0); const int bi = __shfl(ci[0], 0);
        if (!topn_before(bs, bi, sc[ntop - 1], id[ntop - 1])) continue;
        topnsp_fold<T, Q>(sc, id, NP, lane, cs, ci);
    }
    for (int step = 1; step < nw; step <<= 1) {                     // uniform over the workgroup
        __syncthreads();
        if ((wave & (2 * step - 1)) == 0 && wave + step < nw) {
            const T *osc = sc + step * NP; const int *oid = id + step * NP;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int j = lane + 64 * q;
                ms[q] = j < NP ? osc[j] : NEG;
                mi[q] = j < NP ? oid[j] : 0x7fffffff;
            }
            topnsp_fold<T, Q>(sc, id, NP, lane, ms, mi);
        }
    }
    if (wave == 0) {
        for (int j = lane; j < ntop; j += 64) {
            const T sv = sc[j];
            P.out_ids[row + j] = (sv == NEG) ? -1 : id[j];
            if (P.out_scores != nullptr) P.out_scores[row + j] = sv;
        }
    }
}

}  // namespace cmfhip
