// topn_rank_kernels.hpp -- the place of held-out items in each user's full ranking, counted on the device (DESIGN.md "Ranks of
// held-out items").
//
//   score(u, i) = A_u . B_i (+ biasB[i])   -- the bits topn_wide_kernel computes for that pair
//   rank(u, t)  = #{ i in [0, n) : i not in excl(u), score(u, i) not NaN, topn_before(score(u, i), i, score(u, t), t) }
//   pool(u)     = #{ i in [0, n) : i not in excl(u), score(u, i) not NaN }
//   rank = -1 (score NaN) for t outside [0, n), t in excl(u), score(u, t) NaN
//
// Tiling and product are those of topn_wide_kernel (topn_wide_kernels.hpp): TOPNW_NW wavefronts, 16 * NUT users with their
// factors in LDS at stride topnw_ks, a wavefront streams its 16 item rows per round through the four-deep ring, chunks in
// ascending order into a zero accumulator, then + bias.  The product loop is repeated here, not shared: topn_wide_kernel's
// instruction stream stays what it was, and the exact test (tests/test_gpu_ranks.py) keeps the two in step.
//
// In place of the lists and merges, per user in LDS: a slice of up to TS held-out items, their scores ("thresholds") sorted by
// (score desc, id asc), and one counter per threshold.  A pass over the items for one slice:
//   1. thresholds: a "diagonal" product.  Lane column c of a wavefront fetches the row of the item that user 16 t + c holds in
//      slot j, the A operand is the user tile as in the streaming pass, and of the 16 x 16 result only element (c, c) is read:
//      the same chunk order and MFMA chain as the streaming pass gives that pair (an element of an MFMA result is a function of
//      its own row and column alone).  1/16 of the matrix pipe's width, on lists that are short against n.
//   2. sort: bitonic network over the padded slice (TSP = power of two) of all the tile's users at once; invalid targets
//      (id -1) go last, nv[u] = valid ones.
//   3. exclusions: every item of the user's exclusion list is scored by the same diagonal product and taken OUT of the counter
//      the streaming pass will put it in (and out of the pool): the work is the sum of the list lengths, the streaming pass
//      tests nothing per score.  An excluded item that equals a threshold marks that target (rank -1).  A list is ascending; a
//      repeated id is taken out once.
//   4. stream: a score's position among the user's sorted thresholds is p = #{ j : threshold j comes before it or is it }; it
//      counts for every threshold from p on, so counter[p] is bumped.  p == nv (beats none, the common case): nothing, decided
//      by one LDS read and one compare against the user's last threshold, as the top-N kernel's filter.  p == 0 (beats all): a
//      per-lane register, added to counter[0] once at the end of the pass.  A NaN score takes one off the user's pool (n to
//      begin with) through an LDS atomic: a user row of NaN pays n atomics, every other user a handful.
//   5. ranks = prefix sums of the counters, written through the targets' slots.
// All results are integer counts: they do not depend on NUT, TS, the grid or the order of the LDS atomics.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense_kernels.hpp"
#include "topn_kernels.hpp"
#include "topn_wide_kernels.hpp"

namespace cmfhip {

constexpr int TOPNR_TS_MAX = 1024;            // thresholds per user and pass at the most
constexpr int TOPNR_MARK = 1 << 30;           // bit of a slot: the target is in the user's exclusion list

__host__ __device__ inline int topnr_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }
// per user beside the factors: tsp thresholds (score, id, slot, counter), the last threshold's score again, and nv, pool, held
// length, exclusion length
__host__ __device__ inline size_t topnr_lds_bytes(int nut, int k, int tsp, size_t sizeof_real)
{
    const size_t ut = 16 * (size_t)nut;
    return ut * topnw_ks(k, sizeof_real) * sizeof_real + ut * tsp * (sizeof_real + 3 * sizeof(int)) + ut * sizeof_real +
           ut * 4 * sizeof(int) + 2 * sizeof(int);
}

template <typename T>
struct TopnRankParams {
    const T *A; size_t lda; int nu;          // users' factors, first used column
    const T *B; size_t ldb; int n, k;        // the ranker's packed item factors (as TopnWideParams)
    const T *biasB;                          // or null
    const size_t *held_p; const int *held_i; // per-user held-out lists (CSR over the users)
    const size_t *excl_p; const int *excl_i; // per-user exclusion lists, each sorted ascending; or null
    int ts, tsp;                             // held-out items per user and pass; the padded slice (power of two >= ts)
    int *out_rank; T *out_scores;            // [held_p[nu]]; out_scores may be null
    int *out_pool;                           // [nu] or null
};

template <typename T, int NUT>
__global__ void __launch_bounds__(TOPNW_TH)
topn_rank_kernel(const TopnRankParams<T> P)
{
    using Acc = MfmaAcc<T>;
    using vec = typename Acc::vec;
    constexpr int V = 16 / sizeof(T);
    constexpr int CH = 4 * V;
    typedef T ldv __attribute__((ext_vector_type(V)));
    constexpr int UT = 16 * NUT;
    constexpr int PF = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char topnr_smem[];
    const int k = P.k, TS = P.ts, TSP = P.tsp;
    const int KS = topnw_ks(k, sizeof(T)), nchunk = topnw_kp(k, sizeof(T)) / CH;
    T *As = reinterpret_cast<T *>(topnr_smem);                      // [UT][KS]
    T *tsc = As + UT * KS;                                          // [UT][TSP] thresholds, sorted after step 2
    T *tlast = tsc + UT * TSP;                                      // [UT] score of the user's last valid threshold; +inf: none
    int *tid_ = reinterpret_cast<int *>(tlast + UT);                // [UT][TSP] their items; -1: not a valid target
    int *tslot = tid_ + UT * TSP;                                   // [UT][TSP] place in the slice (| TOPNR_MARK); -1: padding
    int *cnt = tslot + UT * TSP;                                    // [UT][TSP]
    int *nv = cnt + UT * TSP;                                       // [UT] valid thresholds
    int *pool = nv + UT;                                            // [UT]
    int *hlen = pool + UT;                                          // [UT] held-out items of the user
    int *elen = hlen + UT;                                          // [UT] its exclusion list's length
    int *mx = elen + UT;                                            // [2] the tile's longest held-out / exclusion list
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;

    // the diagonal product: element (col, col) of (user tile t) x (the 16 item rows `row` of the lanes' columns), in the lanes
    // that hold it (one per column); the chunk order of the streaming pass
    auto diagonal = [&](int t, int row, bool &mine) -> T {
        const T *arow = As + (16 * t + col) * KS + grp * V;
        const T *brow = P.B + (size_t)row * P.ldb + grp * V;
        vec acc = vec{0, 0, 0, 0};
        for (int c = 0; c < nchunk; c++) {
            const ldv a = *reinterpret_cast<const ldv *>(arow + c * CH);
            const ldv b = *reinterpret_cast<const ldv *>(brow + c * CH);
#pragma unroll
            for (int e = 0; e < V; e++) acc = Acc::mma(a[e], b[e], acc);
        }
        T s = T(0);
        mine = false;
#pragma unroll
        for (int r = 0; r < 4; r++)
            if (Acc::row_of(lane, r) == col) { s = acc[r]; mine = true; }
        return s;
    };
    // does (s, item) come before threshold j of user u
    auto before = [&](T s, int item, int u, int j) -> bool {
        const T x = tsc[u * TSP + j];
        return (s > x) || (s == x && item < tid_[u * TSP + j]);
    };
    // #{ j < nvu : threshold j comes before (s, item) or is it }, for 0 < that < nvu known
    auto position = [&](T s, int item, int u, int nvu) -> int {
        int lo = 1, hi = nvu - 1;                                   // threshold 0 does not come after it, threshold nvu - 1 does
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (before(s, item, u, mid)) hi = mid; else lo = mid + 1;
        }
        return lo;                                                  // the first threshold it comes before
    };

    for (int u0 = blockIdx.x * UT; u0 < P.nu; u0 += gridDim.x * UT) {
        const int nu_t = min(UT, P.nu - u0);
        __syncthreads();
        for (int e = tid; e < UT * KS; e += TOPNW_TH) {
            const int u = e / KS, f = e % KS;
            As[e] = (u < nu_t && f < k) ? P.A[(size_t)(u0 + u) * P.lda + f] : T(0);
        }
        if (tid < 2) mx[tid] = 0;
        __syncthreads();
        if (tid < UT) {
            int hl = 0, el = 0;
            if (tid < nu_t) {
                hl = (int)(P.held_p[u0 + tid + 1] - P.held_p[u0 + tid]);
                if (P.excl_p != nullptr) el = (int)(P.excl_p[u0 + tid + 1] - P.excl_p[u0 + tid]);
            }
            hlen[tid] = hl; elen[tid] = el;
            atomicMax(&mx[0], hl); atomicMax(&mx[1], el);
        }
        __syncthreads();
        const int max_h = mx[0], max_e = mx[1];
        for (int s0 = 0; s0 == 0 || s0 < max_h; s0 += TS) {
            const int ts_t = min(TS, max_h - s0);                   // slots in use in this pass (0: a tile without held-out items)
            __syncthreads();
            for (int e = tid; e < UT * TSP; e += TOPNW_TH) { tsc[e] = T(0); tid_[e] = -1; tslot[e] = -1; cnt[e] = 0; }
            if (tid < UT) { nv[tid] = 0; pool[tid] = P.n; }         // the pool: n, minus the NaN scores, minus the excluded items
            __syncthreads();
            // 1. thresholds
            for (int w = wave; w < NUT * ts_t; w += TOPNW_NW) {
                const int t = w / ts_t, j = w % ts_t, u = 16 * t + col;
                const bool has = u < nu_t && s0 + j < hlen[u];
                const int item = has ? P.held_i[P.held_p[u0 + u] + s0 + j] : -1;
                const bool inr = item >= 0 && item < P.n;
                bool mine;
                T s = diagonal(t, inr ? item : 0, mine);
                if (mine && has) {
                    if (P.biasB != nullptr && inr) s += P.biasB[item];
                    const bool ok = inr && !(s != s);
                    tsc[u * TSP + j] = s; tid_[u * TSP + j] = ok ? item : -1; tslot[u * TSP + j] = j;
                    if (ok) atomicAdd(&nv[u], 1);
                }
            }
            __syncthreads();
            // 2. sort: valid targets first, by (score desc, id asc)
            for (int size = 2; size <= TSP; size <<= 1) {
                for (int stride = size >> 1; stride > 0; stride >>= 1) {
                    for (int e = tid; e < UT * (TSP / 2); e += TOPNW_TH) {
                        const int u = e / (TSP / 2), q = e % (TSP / 2);
                        const int i = u * TSP + 2 * q - (q & (stride - 1)), j = i + stride;
                        const bool up = ((2 * q - (q & (stride - 1))) & size) == 0;
                        const T si = tsc[i], sj = tsc[j]; const int ii = tid_[i], ij = tid_[j];
                        const bool j_first = ij >= 0 && (ii < 0 || topn_before(sj, ij, si, ii));
                        const bool i_first = ii >= 0 && (ij < 0 || topn_before(si, ii, sj, ij));
                        if (up ? j_first : i_first) {
                            tsc[i] = sj; tsc[j] = si; tid_[i] = ij; tid_[j] = ii;
                            const int a = tslot[i]; tslot[i] = tslot[j]; tslot[j] = a;
                        }
                    }
                    __syncthreads();
                }
            }
            if (tid < UT) tlast[tid] = nv[tid] > 0 ? tsc[tid * TSP + nv[tid] - 1] : T(INFINITY);     // (read after step 3's barrier)
            // 3. the exclusion lists: out of the counters they will be streamed into
            for (int w = wave; w < NUT * max_e; w += TOPNW_NW) {
                const int t = w / max_e, j = w % max_e, u = 16 * t + col;
                const bool has = u < nu_t && j < elen[u];
                int item = -1;
                if (has) {
                    const size_t at = P.excl_p[u0 + u] + j;
                    item = P.excl_i[at];
                    if (j > 0 && P.excl_i[at - 1] == item) item = -1;                    // a repeated id: once
                }
                const bool inr = item >= 0 && item < P.n;
                bool mine;
                T s = diagonal(t, inr ? item : 0, mine);
                if (mine && inr) {
                    if (P.biasB != nullptr) s += P.biasB[item];
                    if (!(s != s)) {
                        atomicSub(&pool[u], 1);
                        const int nvu = nv[u];
                        if (nvu > 0 && !before(s, item, u, 0)) {                         // else p == 0: target of none
                            const int p = before(s, item, u, nvu - 1) ? position(s, item, u, nvu) : nvu;
                            if (tid_[u * TSP + p - 1] == item) atomicOr(&tslot[u * TSP + p - 1], TOPNR_MARK);
                            if (p < nvu) atomicSub(&cnt[u * TSP + p], 1);
                        } else if (nvu > 0) atomicSub(&cnt[u * TSP], 1);
                    }
                }
            }
            __syncthreads();
            // 4. stream the items (the product loop of topn_wide_kernel)
            int beat_all[NUT][4];
#pragma unroll
            for (int t = 0; t < NUT; t++)
#pragma unroll
                for (int r = 0; r < 4; r++) beat_all[t][r] = 0;
            const T *arow = As + col * KS + grp * V;
            auto item_row = [&](int c0) { return P.B + (size_t)min(c0 + 16 * wave + col, P.n - 1) * P.ldb + grp * V; };
            const T *brow = item_row(0);
            ldv bq[PF];
#pragma unroll
            for (int p = 0; p < PF; p++) bq[p] = *reinterpret_cast<const ldv *>(brow + min(p, nchunk - 1) * CH);
            for (int c0 = 0; c0 < P.n; c0 += TOPNW_ITEMS) {
                const int item = c0 + 16 * wave + col;
                const bool live = item < P.n;
                // (a lane past the last item adds NaN: its scores take the NaN exit below and count nowhere)
                const T bias = live ? (P.biasB != nullptr ? P.biasB[item] : T(0)) : T(NAN);
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
                        bq[p] = *reinterpret_cast<const ldv *>(brow + min(c + p + PF, nchunk - 1) * CH);
                        score_chunk(b, c + p);
                    }
                }
#pragma unroll
                for (int p = 0; p < PF - 1; p++)
                    if (c + p < nchunk) score_chunk(bq[p], c + p);
                brow = item_row(c0 + TOPNW_ITEMS);
#pragma unroll
                for (int p = 0; p < PF; p++) bq[p] = *reinterpret_cast<const ldv *>(brow + min(p, nchunk - 1) * CH);
#pragma unroll
                for (int t = 0; t < NUT; t++) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int u = 16 * t + Acc::row_of(lane, r);
                        const T s = acc[t][r] + bias;
                        if (!(s < tlast[u])) {                      // else, the common case: after every threshold -- counts nowhere
                            if (s != s) {
                                if (live) atomicSub(&pool[u], 1);   // a NaN score is not in the ranking
                            } else {
                                const int nvu = nv[u];              // (a padding user beyond nu_t: no thresholds, nothing written)
                                if (nvu > 0 && before(s, item, u, nvu - 1)) {
                                    if (before(s, item, u, 0)) beat_all[t][r]++;
                                    else atomicAdd(&cnt[u * TSP + position(s, item, u, nvu)], 1);
                                }
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < NUT; t++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int u = 16 * t + Acc::row_of(lane, r);
                    if (beat_all[t][r]) atomicAdd(&cnt[u * TSP], beat_all[t][r]);
                }
            }
            __syncthreads();
            // 5. prefix sums, out through the slots
            if (tid < nu_t) {
                const int u = tid, nvu = nv[u];
                const size_t base = P.held_p[u0 + u] + s0;
                int run = 0;
                for (int j = 0; j < TSP; j++) {
                    const int sl = tslot[u * TSP + j];
                    if (j < nvu) run += cnt[u * TSP + j];
                    if (sl < 0) continue;
                    const bool ok = j < nvu && !(sl & TOPNR_MARK);
                    const size_t at = base + (sl & (TOPNR_MARK - 1));
                    P.out_rank[at] = ok ? run : -1;
                    if (P.out_scores != nullptr) P.out_scores[at] = ok ? tsc[u * TSP + j] : T(NAN);
                }
                if (s0 == 0 && P.out_pool != nullptr) P.out_pool[u0 + u] = pool[u];
            }
        }
    }
}

}  // namespace cmfhip
