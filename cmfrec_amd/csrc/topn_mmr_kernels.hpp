// topn_mmr_kernels.hpp -- diversified top-N: maximal marginal relevance (MMR, Carbonell & Goldstein) over a per-user shortlist
// that is on the device already.
//
// Per user a pool of M <= 128 (id, score) pairs in pool order.  A pair whose id is outside [0, n) or whose score is not finite is
// invalid and never picked (the -1 / -inf a short top-N list ends with).  Over the valid pairs
//   rel_i    = (s_i - s_min) / (s_max - s_min), 0 for all when s_max == s_min
//   sim(i,j) = (b_i . b_j) * inv_i * inv_j over the k factor columns (no bias); inv = the ranker's inverse row norm, 0 for a row
//              that has none (row_rnorm_kernel's NaN), so such a row is similar to nothing
//   pick 1   = the valid pair of the largest rel; pick t + 1 = the valid, unpicked pair of the largest
//              v_i = theta * rel_i - (1 - theta) * max_{j picked} sim(i, j); equal values go to the earlier pool position
// out_ids / out_scores [n_top]: the picked ids and their scores as they came in; out_mmr (optional): v at the pick, theta * rel for the
// first; -1 / -inf once the valid pairs have run out.
// rel is a monotone image of the score that rounding can flatten (two scores one ulp apart, far from s_min), so the picks that
// are by rel alone -- the first of every call, all of them when theta == 1 -- compare the scores themselves: theta == 1 returns the
// valid pairs in descending score, earlier position first, exactly.
//
//   workgroup : TOPNM_NW = 4 wavefronts, one user at a time; users by a static stride over the grid (every user costs the same)
//   Gramian   : the MP x MP products (MP = M rounded up to 16) as NT (NT + 1) / 2 upper-triangle 16 x 16 tiles, NT = MP / 16, dealt
//               round-robin to the wavefronts (tile t to wavefront t % 4: at most Q = 9 each at M = 128), accumulators in
//               registers, on the 16x16x4 MFMA of the working type.  A slot beyond the last tile recomputes tile (0, 0) and is
//               dropped: no branch inside the product loop
//   staging   : the pool's rows are gathered by id from the ranker's packed, zero-padded B in chunks of 128 bytes per row, 16
//               bytes per thread, into two LDS buffers (row stride 144 bytes = 16 x 9: the 16 rows of one ds_read_b128 fall into
//               16 different slots); chunk c + 1 is in flight in registers while chunk c is multiplied: a row is read from memory
//               once per user.  Both MFMA operands take factor  chunk + half * 4V + (lane >> 4) * V + e  at step e: the common
//               permutation of the factor index that topn_wide_kernels.hpp uses
//   table     : the tiles leave the accumulators scaled, (acc * inv_min(i,j)) * inv_max(i,j) -- the same bits on both sides of
//               the diagonal --, into an MP x MP table in LDS that takes the place of the staging buffers; row stride MP + 1, so
//               that the mirrored store of an off-diagonal tile (16 lanes, one column) spreads over the banks
//   greedy    : thread i < MP owns pair i (validity, score, rel, running max sim in registers).  Per pick: the value, a DPP
//               butterfly for the wavefront's maximum and one for the earliest position that holds it (lanes::wave_fold), one
//               LDS exchange across the wavefronts (two alternating slots: one barrier per pick), the owner writes the output,
//               every thread reads its entry of the picked pair's table row (contiguous) into its running maximum
// No atomics; nothing depends on the grid.  Every LDS word that is read was written in the same user's pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits>

#include "device_base.hpp"
#include "dense_kernels.hpp"
#include "lanes.hpp"
#include "topn_wide_kernels.hpp"

namespace cmfhip {

constexpr int TOPNM_NW = 4;                    // wavefronts per workgroup
constexpr int TOPNM_TH = 64 * TOPNM_NW;
constexpr int TOPNM_POOL_MAX = 128;
constexpr int TOPNM_CHUNK_BYTES = 128;         // of a row per staging chunk: two MFMA groups of 4 V factors
constexpr int TOPNM_ROW_BYTES = TOPNM_CHUNK_BYTES + 16;
constexpr int TOPNM_QMAX = 9;                  // tiles per wavefront at M = 128: 36 / 4
constexpr size_t TOPNM_LDS_MAX = 160 * 1024;

__host__ __device__ inline int topnm_mp(int pool) { return (pool + 15) / 16 * 16; }
// tiles per wavefront the kernel is instantiated for: the least of 1, 3, 6, 9 that holds ceil(NT (NT + 1) / 2 / 4)
__host__ __device__ inline int topnm_q(int pool)
{
    const int nt = topnm_mp(pool) / 16;
    return nt <= 2 ? 1 : (nt <= 4 ? 3 : (nt <= 6 ? 6 : TOPNM_QMAX));
}
// the fixed head: inv [128], the two exchanges' values [2][4] each, the rows' ids [128], the picks' positions [2][4]
__host__ __device__ inline size_t topnm_head_bytes(size_t sizeof_real)
{
    return (TOPNM_POOL_MAX + 16) * sizeof_real + (TOPNM_POOL_MAX + 8) * sizeof(int);
}
// ... and behind it the staging buffers, then in their place the table
__host__ __device__ inline size_t topnm_lds_bytes(int pool, size_t sizeof_real)
{
    const size_t mp = (size_t)topnm_mp(pool);
    const size_t stage = 2 * mp * TOPNM_ROW_BYTES, table = (mp * (mp + 1) * sizeof_real + 15) / 16 * 16;
    return topnm_head_bytes(sizeof_real) + (stage > table ? stage : table);
}

template <typename T>
struct TopnMmrParams {
    const T *B; size_t ldb; int n, k;        // item factors: ldb >= topnw_kp(k), columns [k, kp) zero, rows 16-byte aligned
    const T *rn;                             // [n] row_rnorm_kernel's inverse norms
    const int *pool_ids; const T *pool_scores;   // [nu, pool]
    int nu, pool;
    T theta; int n_top;
    int *out_ids; T *out_scores; T *out_mmr; // [nu, n_top]; out_mmr may be null
};

template <typename T, int Q>
__global__ void __launch_bounds__(TOPNM_TH)
topn_mmr_kernel(const TopnMmrParams<T> P)
{
    using Acc = MfmaAcc<T>;
    using vec = typename Acc::vec;
    constexpr int V = 16 / sizeof(T);                               // factors per 16-byte load
    typedef T ldv __attribute__((ext_vector_type(V)));
    constexpr int CW = TOPNM_CHUNK_BYTES / sizeof(T);               // factors per chunk
    constexpr int RS = TOPNM_ROW_BYTES / sizeof(T);                 // staging row stride
    constexpr int PIECES = TOPNM_CHUNK_BYTES / 16;                  // 16-byte pieces of a row per chunk
    constexpr int NLD = TOPNM_POOL_MAX * PIECES / TOPNM_TH;         // pieces per thread and chunk at M = 128
    constexpr int NONE = 0x7fffffff;
    extern __shared__ __attribute__((aligned(16))) unsigned char topnm_smem[];
    T *sinv = reinterpret_cast<T *>(topnm_smem);                    // [128] inverse norm of the pair's row, 0: similar to nothing
    T *redv = sinv + TOPNM_POOL_MAX;                                // [2][4] the wavefronts' best value of a pick, alternating
    T *redm = redv + 8;                                             // [2][4] their largest s and largest -s
    int *rowid = reinterpret_cast<int *>(redm + 8);                 // [128] row of B, -1: stage zeros
    int *redp = rowid + TOPNM_POOL_MAX;                             // [2][4] ... and its position
    T *body = reinterpret_cast<T *>(redp + 8);                      // staging [2][MP][RS], then table [MP][MP + 1]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, grp = lane >> 4;
    const int M = P.pool, MP = topnm_mp(M), NT = MP / 16, MS = MP + 1;
    const int ntiles = NT * (NT + 1) / 2;
    const int kp = topnw_kp(P.k, sizeof(T)), nck = (kp + CW - 1) / CW;
    const T NEG = -INFINITY, POS = INFINITY;
    auto larger = [](T x, T y) { return x > y ? x : y; };
    auto smaller = [](T x, T y) { return x < y ? x : y; };
    // slot q of this wavefront: tile wave + 4 q of the upper triangle in row-major order -> first rows of its two row blocks
    int offa[Q], offb[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        int bi = 0, rem = wave + TOPNM_NW * q;
        if (rem >= ntiles) rem = 0;
        while (rem >= NT - bi) { rem -= NT - bi; bi++; }
        offa[q] = 16 * bi; offb[q] = 16 * (bi + rem);
    }
    for (int u = blockIdx.x; u < P.nu; u += gridDim.x) {
        __syncthreads();                                            // the user before is done with the table and the exchanges
        int id = -1;
        T s = NEG;
        if (tid < M) { id = P.pool_ids[(size_t)u * M + tid]; s = P.pool_scores[(size_t)u * M + tid]; }
        const bool valid = id >= 0 && id < P.n && s > NEG && s < POS;   // (a NaN fails both)
        T inv = 0;
        if (valid) { const T r = P.rn[id]; inv = (r > T(0) && r < POS) ? r : T(0); }
        if (tid < MP) { rowid[tid] = valid ? id : -1; sinv[tid] = inv; }
        {   // (+ 0: one zero, so that the folds' operands commute bit for bit)
            const T hi = lanes::wave_fold(valid ? s + T(0) : NEG, larger), lo = lanes::wave_fold(valid ? T(0) - s : NEG, larger);
            if (lane == 0) { redm[wave] = hi; redm[4 + wave] = lo; }
        }
        __syncthreads();
        const T smax = larger(larger(redm[0], redm[1]), larger(redm[2], redm[3]));
        const T smin = -larger(larger(redm[4], redm[5]), larger(redm[6], redm[7]));
        const T span = smax - smin;
        const T rel = (valid && span > T(0)) ? (s - smin) / span : T(0);

        // ---- the Gramian of the pool's rows
        vec acc[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) acc[q] = vec{0, 0, 0, 0};
        ldv g[NLD];
        auto gather = [&](int c) {
#pragma unroll
            for (int j = 0; j < NLD; j++) {
                const int e = tid + j * TOPNM_TH, row = e / PIECES, c0 = c * CW + (e % PIECES) * V;
                ldv v;
#pragma unroll
                for (int i = 0; i < V; i++) v[i] = T(0);
                if (row < MP) {
                    const int rid = rowid[row];
                    if (rid >= 0 && c0 < kp) v = *reinterpret_cast<const ldv *>(P.B + (size_t)rid * P.ldb + c0);
                }
                g[j] = v;
            }
        };
        auto stage = [&](T *buf) {
#pragma unroll
            for (int j = 0; j < NLD; j++) {
                const int e = tid + j * TOPNM_TH, row = e / PIECES;
                if (row < MP) *reinterpret_cast<ldv *>(buf + row * RS + (e % PIECES) * V) = g[j];
            }
        };
        gather(0);
        stage(body);
        __syncthreads();
        for (int c = 0; c < nck; c++) {
            const T *buf = body + (c & 1) * MP * RS;
            if (c + 1 < nck) gather(c + 1);
#pragma unroll
            for (int h = 0; h < CW / (4 * V); h++) {
                const T *base = buf + col * RS + h * 4 * V + grp * V;
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const ldv a = *reinterpret_cast<const ldv *>(base + offa[q] * RS);
                    const ldv b = *reinterpret_cast<const ldv *>(base + offb[q] * RS);
#pragma unroll
                    for (int e = 0; e < V; e++) acc[q] = Acc::mma(a[e], b[e], acc[q]);
                }
            }
            if (c + 1 < nck) stage(body + ((c + 1) & 1) * MP * RS);
            __syncthreads();
        }
        // ---- the similarity table, in the staging buffers' place (the loop's last barrier: nobody reads them any more)
        T *tab = body;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            if (wave + TOPNM_NW * q < ntiles) {                     // wave-uniform
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = offa[q] + Acc::row_of(lane, r), j = offb[q] + col;
                    const T x = sinv[min(i, j)], y = sinv[max(i, j)];
                    const T v = (x != T(0) && y != T(0)) ? (acc[q][r] * x) * y : T(0);
                    tab[i * MS + j] = v;
                    if (offa[q] != offb[q]) tab[j * MS + i] = v;
                }
            }
        }
        __syncthreads();

        // ---- the greedy picks
        const T theta = P.theta, omt = T(1) - theta;
        const bool by_score = theta == T(1);
        const size_t o = (size_t)u * (size_t)P.n_top;
        bool avail = valid;
        T msim = NEG;                                               // largest similarity to a picked pair (read from the second pick on)
        int t = 0;
        for (; t < P.n_top; t++) {
            const T v = t == 0 ? theta * rel : theta * rel - omt * msim;
            T key = (t == 0 || by_score) ? s : v;
            if (!(key == key)) key = -std::numeric_limits<T>::max();   // (never met with finite factors: the pair stays pickable)
            key = avail ? key + T(0) : NEG;
            const T best = lanes::wave_fold(key, larger);
            const T first = lanes::wave_fold((avail && key == best) ? T(tid) : T(NONE), smaller);
            const int slot = (t & 1) * 4;
            if (lane == 0) { redv[slot + wave] = best; redp[slot + wave] = first < T(TOPNM_TH) ? (int)first : NONE; }
            __syncthreads();
            T wb = redv[slot];
            int wp = redp[slot];
#pragma unroll
            for (int w = 1; w < TOPNM_NW; w++) {                    // a later wavefront holds later positions: it needs more to win
                const T b = redv[slot + w];
                const int p = redp[slot + w];
                if (p != NONE && (wp == NONE || b > wb)) { wb = b; wp = p; }
            }
            if (wp == NONE) break;                                  // (uniform) the valid pairs have run out
            if (tid == wp) {
                avail = false;
                P.out_ids[o + t] = id; P.out_scores[o + t] = s;
                if (P.out_mmr != nullptr) P.out_mmr[o + t] = v;
            }
            if (tid < MP) msim = larger(tab[wp * MS + tid], msim);
        }
        for (int e = t + tid; e < P.n_top; e += TOPNM_TH) {
            P.out_ids[o + e] = -1; P.out_scores[o + e] = NEG;
            if (P.out_mmr != nullptr) P.out_mmr[o + e] = NEG;
        }
    }
}

// topn_mmr_kernel over P.nu pools on st (instantiated in topn_mmr_tu.hip): a persistent grid of as many workgroups as the device
// holds at the pool's LDS size, at most one per user, at most max_groups where that is > 0 (CMFREC_HIP_MMR_GROUPS); returns the grid
int topn_mmr_launch(hipStream_t st, int num_cus, const TopnMmrParams<real_t> &P, int max_groups);

}  // namespace cmfhip
