// topn_wide_kernels.hpp -- batched top-N scoring for every width the library fits (k <= 272), on the matrix cores.
//
// Same semantics as topn_kernel (topn_kernels.hpp): score(u, i) = A_u . B_i (+ biasB[i]), the items of the user's sorted
// exclusion list skipped, the n_top best ids per user in descending score (ties: lower id first), -1 / -inf where fewer remain,
// a NaN score never enters.  topn_kernel holds one item's row in registers per thread and stops at 64 factors; here a tile of
// users against a tile of items is a small matrix product on the 16x16x4 MFMA of the working type (exact f32 / f64), with a
// run-time loop over k (DESIGN.md "Top-N for wide models").
//
//   workgroup  = TOPNW_NW wavefronts, 16 * NUT users (NUT = 1..4 user tiles, chosen on the host by what fits the LDS)
//   user side  : the tile's factors sit in LDS, zero-padded to KS columns (KS * sizeof(T) = 16 bytes times an odd number, so the
//                16 users of one ds_read_b128 fall into 16 different 16-byte slots of the 256-byte bank row)
//   item side  : a round is 16 items per wavefront; a wavefront streams ITS 16 item rows from global memory (16 bytes per lane
//                along the row, B zero-padded to a multiple of the chunk by the ranker) and scores them against all NUT user
//                tiles, so one fetch of an item element serves 16 * NUT users
//   operands   : MFMA step e of a chunk takes factor  chunk * 4V + (lane >> 4) * V + e  for both operands (V = 16 bytes /
//                sizeof(T)): a common permutation of the factor index, which the product does not see
//   results    : lane l holds item (l & 15) against users MfmaAcc<T>::row_of(l, r) of each tile -- the f32 and f64 C/D maps differ
//   lists      : per user in LDS a sorted list of NP = max(32, pow2(n_top)) entries and TOPNW_CAND candidate slots.  A score enters
//                the candidates only if it beats the user's current n_top-th best and (then) is not in the exclusion list.  A
//                wavefront per user sorts the candidates (bitonic), folds them into the list by the first stage of a bitonic
//                merge of (list descending | candidates ascending) -- whose better half alone is kept -- and finishes the merge.
//                Candidates that found no free slot stay in their lane's registers and are offered again after the merge (the
//                threshold has risen by then); which of them got a slot first does not change the result, the order is total.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense_kernels.hpp"
#include "topn_kernels.hpp"

namespace cmfhip {

constexpr int TOPNW_NW = 8;                   // wavefronts per workgroup (two per SIMD)
constexpr int TOPNW_TH = 64 * TOPNW_NW;
constexpr int TOPNW_ITEMS = 16 * TOPNW_NW;    // items per round
constexpr int TOPNW_CAND = 32;                // candidate slots per user
constexpr int TOPNW_KMAX = 272;               // the widest model the library fits (single precision; 256 in double)
constexpr int TOPNW_MAX_NUT = 4;
constexpr size_t TOPNW_LDS_MAX = 160 * 1024;

// factors per chunk = one 16-byte load per lane times the four lane groups
__host__ __device__ constexpr int topnw_chunk(size_t sizeof_real) { return (int)(64 / sizeof_real); }
// columns of the packed, zero-padded item matrix
__host__ __device__ inline int topnw_kp(int k, size_t sizeof_real) { const int ch = topnw_chunk(sizeof_real); return (k + ch - 1) / ch * ch; }
// LDS row stride of the user factors: KP plus one 16-byte slot
__host__ __device__ inline int topnw_ks(int k, size_t sizeof_real) { return topnw_kp(k, sizeof_real) + (int)(16 / sizeof_real); }
__host__ __device__ inline int topnw_np(int n_top) { int np = 32; while (np < n_top) np <<= 1; return np; }
__host__ __device__ inline size_t topnw_lds_bytes(int nut, int k, int n_top, size_t sizeof_real)
{
    const size_t ut = 16 * (size_t)nut, ls = (size_t)topnw_np(n_top) + TOPNW_CAND;
    return ut * topnw_ks(k, sizeof_real) * sizeof_real + ut * ls * (sizeof_real + sizeof(int)) + ut * (sizeof_real + sizeof(int)) +
           2 * sizeof(int);
}

template <typename T>
struct TopnWideParams {
    const T *A; size_t lda; int nu;          // users' factors, first used column
    const T *B; size_t ldb; int n, k;        // item factors: ldb >= topnw_kp(k), columns [k, kp) zero, rows 16-byte aligned
    const T *biasB;                          // or null
    const size_t *excl_p; const int *excl_i; // per-user exclusion lists, each sorted ascending; or null
    int n_top;
    int *out_ids; T *out_scores;             // [nu, n_top]; out_scores may be null
};

// What topn_wide_body leaves to its caller (topn_wide_kernel below, topn_similar_kernel in topn_similar_kernels.hpp,
// topn_after_kernel in topn_after_kernels.hpp): where the
// user tile comes from, what turns an accumulator into a score, and one more reason to skip a pair.  Everything is resolved at
// compile time; `xs` is the policy's own LDS behind the body's (extra bytes: the host adds them to topnw_lds_bytes).
//   Params                         the fields the body reads: nu, B, ldb, n, k, excl_p, excl_i, n_top, out_ids, out_scores
//   fill_users(P, As, xs, ...)     As [UT][KS] <- the tile's factors, zero beyond k and beyond the tile's nu_t users (all threads,
//                                  in front of the body's barrier); xs <- whatever score / admit read
//   item_value(P, item, live)      per lane and round: what the score needs of the lane's item
//   score(acc, iv, xs, UT, u)      the score of user u of the tile against that item
//   admit(xs, UT, u, item, score)  false: the pair is skipped -- asked once per pair, ahead of the exclusion list, not again
//                                  when a candidate is offered a second time
//   out_stride(P)                  elements between two users' rows of out_ids / out_scores
//   item_begin(P), item_end(P)     the items [begin, end) the workgroup ranks: 0 and P.n, but for a slice of the items
//                                  (topn_split_kernels.hpp) -- begin a multiple of TOPNW_ITEMS, so the rows keep their lanes
template <typename T>
struct TopnWidePolicy {
    using Params = TopnWideParams<T>;
    static __device__ __forceinline__ void fill_users(const Params &P, T *As, unsigned char *, int u0, int nu_t, int UT, int KS, int tid)
    {
        for (int e = tid; e < UT * KS; e += TOPNW_TH) {
            const int u = e / KS, f = e % KS;
            As[e] = (u < nu_t && f < P.k) ? P.A[(size_t)(u0 + u) * P.lda + f] : T(0);
        }
    }
    static __device__ __forceinline__ T item_value(const Params &P, int item, bool live) { return (P.biasB != nullptr && live) ? P.biasB[item] : T(0); }
    static __device__ __forceinline__ T score(T acc, T bias, const unsigned char *, int, int) { return acc + bias; }
    static __device__ __forceinline__ bool admit(const unsigned char *, int, int, int, T) { return true; }
    static __device__ __forceinline__ size_t out_stride(const Params &P) { return (size_t)P.n_top; }
    static __device__ __forceinline__ int item_begin(const Params &) { return 0; }
    static __device__ __forceinline__ int item_end(const Params &P) { return P.n; }
};

template <typename T, int NUT, typename POL>
__device__ __forceinline__ void topn_wide_body(const typename POL::Params P)
{
    using Acc = MfmaAcc<T>;
    using vec = typename Acc::vec;
    constexpr int V = 16 / sizeof(T);                               // factors per 16-byte load
    constexpr int CH = 4 * V;                                       // factors per chunk
    typedef T ldv __attribute__((ext_vector_type(V)));
    constexpr int UT = 16 * NUT;
    constexpr int PF = 4;                                           // item-row loads in flight per lane
    extern __shared__ __attribute__((aligned(16))) unsigned char topnw_smem[];
    const int k = P.k, ntop = P.n_top;
    const int KS = topnw_ks(k, sizeof(T)), nchunk = topnw_kp(k, sizeof(T)) / CH;
    const int NP = topnw_np(ntop), LS = NP + TOPNW_CAND;
    T *As = reinterpret_cast<T *>(topnw_smem);                      // [UT][KS]
    T *ssc = As + UT * KS;                                          // [UT][LS]: [0, NP) sorted list, [NP, LS) candidates
    T *thr = ssc + UT * LS;                                         // [UT] score of the current n_top-th best (-inf until full)
    int *sid = reinterpret_cast<int *>(thr + UT);                   // [UT][LS]
    int *cnt = sid + UT * LS;                                       // [UT] candidates offered since the last merge
    int *flag = cnt + UT;                                           // [2] "a lane still holds a candidate", alternating
    unsigned char *xs = reinterpret_cast<unsigned char *>(flag + 2);   // the policy's own (8-byte aligned: UT * LS + UT + 2 ints)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const int i0 = POL::item_begin(P), i1 = POL::item_end(P);       // the items of this workgroup's pass
    const T NEG = -INFINITY;
    int turn = 0;                                                   // merges so far (uniform): which flag is live
    if (tid < 2) flag[tid] = 0;
    for (int u0 = blockIdx.x * UT; u0 < P.nu; u0 += gridDim.x * UT) {
        const int nu_t = min(UT, P.nu - u0);
        __syncthreads();
        POL::fill_users(P, As, xs, u0, nu_t, UT, KS, tid);
        for (int e = tid; e < UT * LS; e += TOPNW_TH) { ssc[e] = NEG; sid[e] = 0x7fffffff; }
        if (tid < UT) { cnt[tid] = 0; thr[tid] = NEG; }
        __syncthreads();
        const T *arow = As + col * KS + grp * V;
        // the item rows arrive through a ring of PF loads in flight per lane: a chunk's load is issued PF chunks ahead, and the
        // first PF of the NEXT round before this round's filter and merge, so those overlap the fetch
        auto item_row = [&](int c0) { return P.B + (size_t)min(c0 + 16 * wave + col, P.n - 1) * P.ldb + grp * V; };
        const T *brow = item_row(i0);
        ldv bq[PF];
#pragma unroll
        for (int p = 0; p < PF; p++) bq[p] = *reinterpret_cast<const ldv *>(brow + min(p, nchunk - 1) * CH);
        for (int c0 = i0; c0 < i1; c0 += TOPNW_ITEMS) {
            const int item = c0 + 16 * wave + col;
            const bool live = item < i1;
            const auto iv = POL::item_value(P, item, live);
            vec acc[NUT];
#pragma unroll
            for (int t = 0; t < NUT; t++) acc[t] = vec{0, 0, 0, 0};
            auto score_chunk = [&](const ldv &b, int c) {
#pragma unroll
                for (int t = 0; t < NUT; t++) {
                    const ldv a = *reinterpret_cast<const ldv *>(arow + t * 16 * KS + c * CH);
#pragma unroll
                    for (int e = 0; e < V; e++) acc[t] = Acc::mma(a[e], b[e], acc[t]);
                }
            };
            int c = 0;
            for (; c + PF <= nchunk; c += PF) {
#pragma unroll
                for (int p = 0; p < PF; p++) {
                    const ldv b = bq[p];
                    bq[p] = *reinterpret_cast<const ldv *>(brow + min(c + p + PF, nchunk - 1) * CH);   // (past the end: a repeat, unused)
                    score_chunk(b, c + p);
                }
            }
#pragma unroll
            for (int p = 0; p < PF - 1; p++)
                if (c + p < nchunk) score_chunk(bq[p], c + p);                   // uniform
            brow = item_row(c0 + TOPNW_ITEMS);
#pragma unroll
            for (int p = 0; p < PF; p++) bq[p] = *reinterpret_cast<const ldv *>(brow + min(p, nchunk - 1) * CH);
            // filter: bit (4 t + r) of `pend` = this lane still has to offer its score for user 16 t + row_of(lane, r)
            unsigned pend = 0;
#pragma unroll
            for (int t = 0; t < NUT; t++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int u = 16 * t + Acc::row_of(lane, r);
                    acc[t][r] = POL::score(acc[t][r], iv, xs, UT, u);
                    if (live && u < nu_t && acc[t][r] >= thr[u] && POL::admit(xs, UT, u, item, acc[t][r])) {   // NaN never enters
                        bool skip = false;
                        if (P.excl_p != nullptr) {                               // sorted list of the user: binary search
                            const size_t end = P.excl_p[u0 + u + 1];
                            size_t lo = P.excl_p[u0 + u], hi = end;
                            while (lo < hi) {
                                const size_t mid = (lo + hi) >> 1;
                                if (P.excl_i[mid] < item) lo = mid + 1; else hi = mid;
                            }
                            skip = (lo < end) && (P.excl_i[lo] == item);
                        }
                        if (!skip) pend |= 1u << (4 * t + r);
                    }
                }
            }
            bool more;
            do {
#pragma unroll
                for (int t = 0; t < NUT; t++) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const unsigned bit = 1u << (4 * t + r);
                        if (pend & bit) {
                            const int u = 16 * t + Acc::row_of(lane, r);
                            if (!(acc[t][r] >= thr[u])) pend &= ~bit;            // the threshold has passed it meanwhile
                            else {
                                const int pos = atomicAdd(&cnt[u], 1);
                                if (pos < TOPNW_CAND) {
                                    ssc[u * LS + NP + pos] = acc[t][r];
                                    sid[u * LS + NP + pos] = item;
                                    pend &= ~bit;
                                }
                            }
                        }
                    }
                }
                if (pend) flag[turn & 1] = 1;
                __syncthreads();
                if (tid == 0) flag[(turn + 1) & 1] = 0;
                // merge: one wavefront per user
                for (int u = wave; u < nu_t; u += TOPNW_NW) {
                    const int c = min(cnt[u], TOPNW_CAND);
                    if (c == 0) continue;                                        // wave-uniform
                    T *sc = ssc + u * LS; int *id = sid + u * LS;
                    T *csc = sc + NP; int *cid = id + NP;
                    int W = 1;
                    while (W < c) W <<= 1;                                       // <= TOPNW_CAND
                    // candidates, best first (the free slots hold -inf)
                    for (int size = 2; size <= W; size <<= 1) {
                        for (int stride = size >> 1; stride > 0; stride >>= 1) {
                            if (lane < W / 2) {
                                const int i = 2 * lane - (lane & (stride - 1)), j = i + stride;
                                const bool up = ((i & size) == 0) || (size == W);
                                const T si = csc[i], sj = csc[j]; const int ii = cid[i], ij = cid[j];
                                const bool swap = up ? topn_before(sj, ij, si, ii) : topn_before(si, ii, sj, ij);
                                if (swap) { csc[i] = sj; csc[j] = si; cid[i] = ij; cid[j] = ii; }
                            }
                            __builtin_amdgcn_wave_barrier();
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        }
                    }
                    // (list descending | -inf ... | candidates ascending) is bitonic; the first stage of its merge leaves the
                    // better of list[NP - 1 - j] and candidate j in the list half, which holds the best NP and is bitonic again
                    if (lane < W) {
                        const int i = NP - 1 - lane;
                        const T sl = sc[i], sb = csc[lane]; const int il = id[i], ib = cid[lane];
                        if (topn_before(sb, ib, sl, il)) { sc[i] = sb; id[i] = ib; }
                        csc[lane] = NEG; cid[lane] = 0x7fffffff;
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
                    for (int e = ntop + lane; e < NP; e += 64) { sc[e] = NEG; id[e] = 0x7fffffff; }   // keep the best n_top
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    if (lane == 0) { cnt[u] = 0; thr[u] = sc[ntop - 1]; }
                }
                more = flag[turn & 1] != 0;
                turn++;
                __syncthreads();
            } while (more);
        }
        const size_t ldo = POL::out_stride(P);
        for (int e = tid; e < nu_t * ntop; e += TOPNW_TH) {
            const int u = e / ntop, j = e % ntop;
            const T sv = ssc[u * LS + j];
            P.out_ids[(size_t)(u0 + u) * ldo + j] = (sv == NEG) ? -1 : sid[u * LS + j];
            if (P.out_scores != nullptr) P.out_scores[(size_t)(u0 + u) * ldo + j] = sv;
        }
    }
}

template <typename T, int NUT>
__global__ void __launch_bounds__(TOPNW_TH)
topn_wide_kernel(const TopnWideParams<T> P)
{
    topn_wide_body<T, NUT, TopnWidePolicy<T>>(P);
}

}  // namespace cmfhip
