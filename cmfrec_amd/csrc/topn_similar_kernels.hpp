// topn_similar_kernels.hpp -- neighbours of the ranker's own rows: "which items are like this item" by dot product or cosine.
//
// topn_similar_kernel is topn_wide_body (topn_wide_kernels.hpp: tiling, item streaming, MFMA product, candidate slots, bitonic
// merge, output) under another policy (DESIGN.md "Similar items and users"):
//   query tile : gathered from the resident B by query_ids[u0 + u], 16 bytes per thread, unscaled; the columns [k, KS) are zero
//                (B's own padding, and the tile's last 16-byte slot); no factor matrix is uploaded
//   score      : dot    -- the accumulator as it is (no bias, even when the ranker holds one)
//                cosine -- (acc * rn[item]) * rn[query]: two multiplications, in that order
//   self       : item == query_ids[u] is skipped ahead of the exclusion list
//   LDS        : the body's, then rn[query] and the query id of the tile's 16 * NUT users
// rn = row_rnorm_kernel's inverse norms.  A row whose sum of squares is zero, NaN or infinite has rn = NaN; a NaN score never
// enters a list, so such a row is nobody's neighbour and, as a query, has none.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topn_wide_kernels.hpp"

namespace cmfhip {

constexpr int TOPNS_DOT = 0, TOPNS_COSINE = 1;
constexpr int TOPNS_NORM_TH = 256;            // threads of row_rnorm_kernel: four lanes per row, 64 rows per workgroup

__host__ __device__ inline size_t topns_lds_bytes(int nut, int k, int n_top, size_t sizeof_real)
{
    return topnw_lds_bytes(nut, k, n_top, sizeof_real) + 16 * (size_t)nut * (sizeof_real + sizeof(int));
}

// rn[i] = 1 / sqrt(sum_f B[i, f]^2), IEEE square root and division (no approximate rsqrt).  B [n, ldb]: the ranker's packed
// matrix, kp = topnw_kp(k) columns read, [k, kp) zero, rows 16-byte aligned.  Four lanes per row, 16 bytes per lane and step:
// lane g adds the squares of the 16-byte pieces g, g + 4, g + 8, ... in ascending order (one fma each), then
// (s0 + s1) + (s2 + s3) -- an order that the row alone decides, not the launch.
template <typename T>
__global__ void __launch_bounds__(TOPNS_NORM_TH)
row_rnorm_kernel(const T *__restrict__ B, size_t ldb, int n, int kp, T *__restrict__ rn)
{
    constexpr int V = 16 / sizeof(T);
    typedef T ldv __attribute__((ext_vector_type(V)));
    const size_t row = (size_t)blockIdx.x * (TOPNS_NORM_TH / 4) + (threadIdx.x >> 2);
    const int g = threadIdx.x & 3;
    T s = 0;
    if (row < (size_t)n) {
        const T *b = B + row * ldb + g * V;
        for (int f = 0; f < kp; f += 4 * V) {
            const ldv v = *reinterpret_cast<const ldv *>(b + f);
#pragma unroll
            for (int e = 0; e < V; e++) {
                if constexpr (sizeof(T) == 8) s = __builtin_fma(v[e], v[e], s);
                else s = __builtin_fmaf(v[e], v[e], s);
            }
        }
    }
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    if (g == 0 && row < (size_t)n) {
        T r;
        if constexpr (sizeof(T) == 8) r = __builtin_sqrt(s); else r = __builtin_sqrtf(s);
        rn[row] = (s > T(0) && s < T(INFINITY)) ? T(1) / r : T(NAN);
    }
}

template <typename T>
struct TopnSimilarParams {
    const int *query_ids; int nu;            // rows of B that ask, each in [0, n)
    const T *B; size_t ldb; int n, k;        // as TopnWideParams
    const T *rn;                             // [n] inverse norms (cosine), or null (dot)
    const size_t *excl_p; const int *excl_i; // per-query exclusion lists, each sorted ascending; or null
    int n_top;
    int *out_ids; T *out_scores;             // [nu, n_top]; out_scores may be null
};

template <typename T, int METRIC>
struct TopnSimilarPolicy {
    using Params = TopnSimilarParams<T>;
    struct None {};
    static __device__ __forceinline__ void fill_users(const Params &P, T *As, unsigned char *xs, int u0, int nu_t, int UT, int KS, int tid)
    {
        constexpr int V = 16 / sizeof(T);
        typedef T ldv __attribute__((ext_vector_type(V)));
        T *rnq = reinterpret_cast<T *>(xs);                          // [UT] (NaN-free filler beyond the tile: never offered)
        int *qid = reinterpret_cast<int *>(rnq + UT);                // [UT] (-1 beyond the tile)
        if (tid < UT) {
            const int q = tid < nu_t ? P.query_ids[u0 + tid] : -1;
            qid[tid] = q;
            if constexpr (METRIC == TOPNS_COSINE) rnq[tid] = q >= 0 ? P.rn[q] : T(0);
            else rnq[tid] = T(0);
        }
        const int pieces = KS / V;                                   // per row; the last one is the padding slot
        for (int e = tid; e < UT * pieces; e += TOPNW_TH) {
            const int u = e / pieces, p = e % pieces;
            ldv v;
#pragma unroll
            for (int i = 0; i < V; i++) v[i] = T(0);
            if (u < nu_t && p < pieces - 1) v = *reinterpret_cast<const ldv *>(P.B + (size_t)P.query_ids[u0 + u] * P.ldb + p * V);
            *reinterpret_cast<ldv *>(As + u * KS + p * V) = v;
        }
    }
    static __device__ __forceinline__ auto item_value(const Params &P, int item, bool live)
    {
        if constexpr (METRIC == TOPNS_COSINE) return live ? P.rn[item] : T(0);
        else return None{};
    }
    static __device__ __forceinline__ T score(T acc, T rni, const unsigned char *xs, int, int u) { return (acc * rni) * reinterpret_cast<const T *>(xs)[u]; }
    static __device__ __forceinline__ T score(T acc, None, const unsigned char *, int, int) { return acc; }
    static __device__ __forceinline__ bool admit(const unsigned char *xs, int UT, int u, int item, T)
    {
        return reinterpret_cast<const int *>(reinterpret_cast<const T *>(xs) + UT)[u] != item;
    }
    static __device__ __forceinline__ size_t out_stride(const Params &P) { return (size_t)P.n_top; }
    static __device__ __forceinline__ int item_begin(const Params &) { return 0; }
    static __device__ __forceinline__ int item_end(const Params &P) { return P.n; }
};

template <typename T, int NUT, int METRIC>
__global__ void __launch_bounds__(TOPNW_TH)
topn_similar_kernel(const TopnSimilarParams<T> P)
{
    topn_wide_body<T, NUT, TopnSimilarPolicy<T, METRIC>>(P);
}

}  // namespace cmfhip
