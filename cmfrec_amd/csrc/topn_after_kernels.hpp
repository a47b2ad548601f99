// topn_after_kernels.hpp -- the next n_top best items of every user behind a per-user cursor: pages of a ranking, and through
// pages chained on the device any n_top <= n (DESIGN.md "Deep lists and next pages").
//
// topn_after_kernel is topn_wide_body (topn_wide_kernels.hpp: tiling, item streaming, MFMA product, candidate slots, bitonic
// merge, output) under a third policy:
//   users   : topn_wide_kernel's -- the tile's factors from A, the score acc + bias: the bits topn_wide_kernel gives the pair
//   cursor  : (cur_scores[u * cur_ld], cur_ids[u * cur_ld]) per user, read from device memory into the policy's LDS; a pair
//             (s, item) is offered only if topn_before(cursor, (s, item)) -- the cursor is strictly ahead of it in the total
//             order (higher score first, then lower id).  No special cases:
//               (+inf, -1)   admits every pair: the first page (also what cur_scores == null stands for)
//               (-inf, -1)   what an exhausted user's previous page ends with: admits only scores of -inf, which are written as
//                            -1 / -inf like an empty position, so every later position is -1 / -inf
//               NaN score    admits nothing
//             The cursor's item itself need not be rankable (it may have been excluded since).
//   output  : n_top columns per user with the row stride out_ld: a page writes its columns of a wider [nu, out_ld] result
//   LDS     : the body's, then the cursor scores and ids of the tile's 16 * NUT users
// The cursor compares score bits: it must come from this body's scores (this kernel, topn_wide_kernel, topn_rank_kernel).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topn_wide_kernels.hpp"

namespace cmfhip {

constexpr int TOPNA_PAGE_MAX = 512;           // the longest page (list of NP = 512 entries per user)

// the policy's LDS per user tile
__host__ __device__ constexpr size_t topna_extra_bytes(size_t sizeof_real) { return 16 * (sizeof_real + sizeof(int)); }
__host__ __device__ inline size_t topna_lds_bytes(int nut, int k, int n_top, size_t sizeof_real)
{
    return topnw_lds_bytes(nut, k, n_top, sizeof_real) + (size_t)nut * topna_extra_bytes(sizeof_real);
}

template <typename T>
struct TopnAfterParams {
    const T *A; size_t lda; int nu;          // as TopnWideParams
    const T *B; size_t ldb; int n, k;
    const T *biasB;
    const size_t *excl_p; const int *excl_i;
    int n_top;                               // length of the page
    int *out_ids; T *out_scores;             // first column of the page; rows out_ld apart; out_scores may be null
    size_t out_ld;
    const T *cur_scores; const int *cur_ids; // one cursor per user, cur_ld elements apart; both null: every user starts at the top
    size_t cur_ld;
};

template <typename T>
struct TopnAfterPolicy {
    using Params = TopnAfterParams<T>;
    static __device__ __forceinline__ void fill_users(const Params &P, T *As, unsigned char *xs, int u0, int nu_t, int UT, int KS, int tid)
    {
        T *cs = reinterpret_cast<T *>(xs);                           // [UT] (beyond the tile: never read, the body asks u < nu_t first)
        int *ci = reinterpret_cast<int *>(cs + UT);                  // [UT]
        if (tid < UT) {
            const bool has = P.cur_scores != nullptr && tid < nu_t;
            cs[tid] = has ? P.cur_scores[(size_t)(u0 + tid) * P.cur_ld] : T(INFINITY);
            ci[tid] = has ? P.cur_ids[(size_t)(u0 + tid) * P.cur_ld] : -1;
        }
        for (int e = tid; e < UT * KS; e += TOPNW_TH) {
            const int u = e / KS, f = e % KS;
            As[e] = (u < nu_t && f < P.k) ? P.A[(size_t)(u0 + u) * P.lda + f] : T(0);
        }
    }
    static __device__ __forceinline__ T item_value(const Params &P, int item, bool live) { return (P.biasB != nullptr && live) ? P.biasB[item] : T(0); }
    static __device__ __forceinline__ T score(T acc, T bias, const unsigned char *, int, int) { return acc + bias; }
    static __device__ __forceinline__ bool admit(const unsigned char *xs, int UT, int u, int item, T s)
    {
        const T *cs = reinterpret_cast<const T *>(xs);
        return topn_before(cs[u], reinterpret_cast<const int *>(cs + UT)[u], s, item);
    }
    static __device__ __forceinline__ size_t out_stride(const Params &P) { return P.out_ld; }
    static __device__ __forceinline__ int item_begin(const Params &) { return 0; }
    static __device__ __forceinline__ int item_end(const Params &P) { return P.n; }
};

template <typename T, int NUT>
__global__ void __launch_bounds__(TOPNW_TH)
topn_after_kernel(const TopnAfterParams<T> P)
{
    topn_wide_body<T, NUT, TopnAfterPolicy<T>>(P);
}

}  // namespace cmfhip
