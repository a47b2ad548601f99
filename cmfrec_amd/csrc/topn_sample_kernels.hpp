// topn_sample_kernels.hpp -- stochastic top-N: n items per user drawn without replacement with probability proportional to
// exp(score / T) (Plackett-Luce), as the top-n of  key = score + T * g,  g one standard Gumbel variable per (user, item) pair, and
// on request the per-user log-partition  lse[u] = log sum_i exp(score_ui / T)  (DESIGN.md section 3.21).
//
// topn_sample_kernel is topn_wide_body (topn_wide_kernels.hpp: tiling, item streaming, MFMA product, candidate slots, bitonic
// merge, output) with its extension hooks on, under TopnSamplePolicy<T, LSE>:
//   noise      : counter-based.  h = splitmix64(seed ^ (u * 0x9E3779B97F4A7C15 + i)), u the user's place in the call's batch;
//                U = ((h >> 11) + 1/2) 2^-53 (double) or ((h >> 40) + 1/2) 2^-24 (single), an exact rational strictly inside
//                (0, 1); g = -log(-log U) in the working precision.  For U > 1/2 (top bit of h set) neither format holds U, but
//                both hold w = 1 - U = ((~h >> 11 or 40) + 1/2) 2^-53 or -24 exactly, and -log U = -log1p(-w).
//   lazy       : the hash is integer work and runs for every pair; the two logarithms do not.  With z = the leading one-bits of
//                h, 1 - U >= 2^-(z + 1) (the bit behind the run is zero; where the run fills the mantissa the 1/2 holds U off 1),
//                and -log U >= 1 - U, so  g <= (z + 1) ln 2  exactly.  TOPNSM_BOUND_C = 2^-10 on top covers the rounding of the
//                two library logarithms (a few units in the last place of 1 + |g| <= 39: below 2^-17 in single precision) and of
//                (z + 1) ln 2 itself.  key and bound are the same fma(T, ., score), which does not decrease in its middle
//                argument, so bound < threshold proves key < threshold: the pair is dropped with its logarithms unevaluated
//                (its key is NaN, which the body's threshold test never admits).  The threshold logic is the body's.
//   lse        : LSE = true.  Per lane and per user of its accumulator a running reference m (single precision) and a sum
//                (double) of exp((score - m) / T), the exponential in single precision (v_exp_f32) in both builds; a score above
//                m moves m there and rescales the sum.  Excluded pairs take no part: wavefront 0 walks the tile's sorted
//                exclusion lists one round ahead of the items (a cursor and the next excluded id per user in LDS) and leaves a
//                128-bit mask per user and round, double-buffered between the body's barriers; a pair costs one LDS word.
//                At the end of a tile: a butterfly over the 16 lanes that share a user, the wavefronts' partials through LDS,
//                merged in wavefront order by one thread per user; lse = m / T + log(sum) in double.  No atomics.
//                LSE = false compiles all of it out; the policy then has no LDS of its own.
//   scores     : the list carries keys.  topn_sample_scores_kernel recomputes the n_top scores per user behind it: a wavefront
//                per 16 users and list position runs the body's MFMA sequence (same operands per step, same chunk order, the
//                zero padding included) on the 16 (user, item) pairs as the diagonal of a 16 x 16 tile, then + bias -- the bits
//                topn_wide_kernel gives for the pair.  n_top / (items / 16) of the ranking's MFMAs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_base.hpp"
#include "topn_wide_kernels.hpp"

namespace cmfhip {

constexpr unsigned long long TOPNSM_GOLDEN = 0x9E3779B97F4A7C15ull;   // the user stride of the counter; splitmix64's increment
constexpr double TOPNSM_LN2 = 0.693147180559945309417232121458;
constexpr double TOPNSM_BOUND_C = 0x1p-10;                            // slack of the lazy bound (see above)

// LDS of the policy per user of the tile (LSE only): cursor 8, wavefront sums 8 NW, wavefront references 4 NW, next id 4, masks 32
__host__ __device__ constexpr size_t topnsm_extra_per_user(bool lse) { return lse ? 8 + 8 * TOPNW_NW + 4 * TOPNW_NW + 4 + 2 * 16 : 0; }
// user tiles per workgroup at most: in double precision the 48 registers of four tiles' log-partition state would spill
__host__ __device__ constexpr int topnsm_max_tiles(size_t sizeof_real, bool lse) { return (lse && sizeof_real == 8) ? 3 : TOPNW_MAX_NUT; }
__host__ __device__ inline size_t topnsm_lds_bytes(int nut, int k, int n_top, size_t sizeof_real, bool lse)
{
    return topnw_lds_bytes(nut, k, n_top, sizeof_real) + 16 * (size_t)nut * topnsm_extra_per_user(lse);
}

__host__ __device__ __forceinline__ unsigned long long topnsm_splitmix64(unsigned long long x)
{
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__device__ __forceinline__ unsigned long long topnsm_hash(unsigned long long seed, int user, int item)
{
    return topnsm_splitmix64(seed ^ ((unsigned long long)user * TOPNSM_GOLDEN + (unsigned long long)item));
}

// g <= this, for every h, in the arithmetic of topnsm_gumbel
template <typename T>
__device__ __forceinline__ T topnsm_gumbel_bound(unsigned long long h)
{
    const unsigned long long nh = ~h;
    const int z = nh ? __builtin_clzll(nh) : 64;
    return (T)(z + 1) * (T)TOPNSM_LN2 + (T)TOPNSM_BOUND_C;
}

__device__ __forceinline__ double topnsm_gumbel(unsigned long long h, double)
{
    double L;
    if (h >> 63) L = -log1p(-(((double)(~h >> 11) + 0.5) * 0x1p-53));
    else L = -log(((double)(h >> 11) + 0.5) * 0x1p-53);
    return -log(L);
}
__device__ __forceinline__ float topnsm_gumbel(unsigned long long h, float)
{
    float L;
    if (h >> 63) L = -log1pf(-(((float)(unsigned)(~h >> 40) + 0.5f) * 0x1p-24f));
    else L = -logf(((float)(unsigned)(h >> 40) + 0.5f) * 0x1p-24f);
    return -logf(L);
}

template <typename T> __device__ __forceinline__ T topnsm_fma(T a, T b, T c);
template <> __device__ __forceinline__ double topnsm_fma<double>(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <> __device__ __forceinline__ float topnsm_fma<float>(float a, float b, float c) { return __builtin_fmaf(a, b, c); }

template <typename T>
struct TopnSampleParams {
    const T *A; size_t lda; int nu;          // as TopnWideParams
    const T *B; size_t ldb; int n, k;
    const T *biasB;
    const size_t *excl_p; const int *excl_i;
    int n_top;
    int *out_ids; T *out_scores;             // [nu, n_top]: the ids and their KEYS (the body's list)
    T temperature;                           // > 0 (temperature 0 is topn_wide_kernel's call)
    float inv_t;                             // 1 / temperature
    unsigned long long seed;
    double *out_lse;                         // [nu] (LSE)
};

// one log-sum-exp partial: sum of exp((score - m) / T) over what has been added
struct TopnSampleLse {
    float m; double s;
    template <typename T>
    __device__ __forceinline__ void add(T score, float inv_t)
    {
        if (score > (T)m) {                                          // a new reference (the first score finds m = -inf, s = 0)
            const float mn = (float)score;
            s *= (double)__expf((float)((T)m - (T)mn) * inv_t);
            m = mn;
        }
        s += (double)__expf((float)(score - (T)m) * inv_t);
    }
    __device__ __forceinline__ void merge(float m2, double s2, float inv_t)
    {
        const float M = fmaxf(m, m2);
        const double e1 = (m == M) ? 1.0 : (double)__expf((m - M) * inv_t), e2 = (m2 == M) ? 1.0 : (double)__expf((m2 - M) * inv_t);
        s = s * e1 + s2 * e2;
        m = M;
    }
};

template <typename T, bool LSE>
struct TopnSamplePolicy {
    using Params = TopnSampleParams<T>;
    template <int NUT> struct TileState {
        TopnSampleLse l[LSE ? 4 * NUT : 1];
        __device__ __forceinline__ TileState()
        {
#pragma unroll
            for (int j = 0; j < (LSE ? 4 * NUT : 1); j++) { l[j].m = -INFINITY; l[j].s = 0.0; }
        }
    };
    // the policy's LDS (LSE): [UT] cursors, [NW][UT] sums, [NW][UT] references, [UT] next ids, [2][UT][4] mask words
    struct Lds {
        size_t *cur; double *wsum; float *wm; int *nxt; unsigned *mask;
        __device__ __forceinline__ Lds(unsigned char *xs, int UT)
        {
            cur = reinterpret_cast<size_t *>(xs);
            wsum = reinterpret_cast<double *>(cur + UT);
            wm = reinterpret_cast<float *>(wsum + TOPNW_NW * UT);
            nxt = reinterpret_cast<int *>(wm + TOPNW_NW * UT);
            mask = reinterpret_cast<unsigned *>(nxt + UT);
        }
    };
    // thread u < UT: the mask of user u for the items [c_begin, c_begin + TOPNW_ITEMS) into buffer (c_begin / TOPNW_ITEMS) & 1
    static __device__ __forceinline__ void build_mask(const Params &P, const Lds &L, int UT, int u, int u0, int nu_t, int c_begin)
    {
        unsigned *m = L.mask + ((size_t)((c_begin / TOPNW_ITEMS) & 1) * UT + u) * 4;
        m[0] = 0; m[1] = 0; m[2] = 0; m[3] = 0;
        const int c_end = c_begin + TOPNW_ITEMS;
        int id = L.nxt[u];
        if (id >= c_end) return;                                     // (also: no list, a list that has run out, beyond the tile)
        size_t c = L.cur[u];
        const size_t end = P.excl_p[u0 + u + 1];
        while (id < c_end) {
            if (id >= c_begin) m[(id - c_begin) >> 5] |= 1u << ((id - c_begin) & 31);
            c++;
            id = c < end ? P.excl_i[c] : 0x7fffffff;
        }
        L.cur[u] = c; L.nxt[u] = id;
    }
    static __device__ __forceinline__ void fill_users(const Params &P, T *As, unsigned char *xs, int u0, int nu_t, int UT, int KS, int tid)
    {
        for (int e = tid; e < UT * KS; e += TOPNW_TH) {
            const int u = e / KS, f = e % KS;
            As[e] = (u < nu_t && f < P.k) ? P.A[(size_t)(u0 + u) * P.lda + f] : T(0);
        }
        if constexpr (LSE) {
            if (tid < UT) {
                const Lds L(xs, UT);
                size_t c = 0;
                int id = 0x7fffffff;
                if (P.excl_p != nullptr && tid < nu_t) {
                    c = P.excl_p[u0 + tid];
                    if (c < P.excl_p[u0 + tid + 1]) id = P.excl_i[c];
                }
                L.cur[tid] = c; L.nxt[tid] = id;
                build_mask(P, L, UT, tid, u0, nu_t, 0);
            }
        }
    }
    static __device__ __forceinline__ void round_begin(const Params &P, unsigned char *xs, int c0, int u0, int nu_t, int UT, int tid)
    {
        if constexpr (LSE) {
            if (tid < UT && c0 + TOPNW_ITEMS < P.n) build_mask(P, Lds(xs, UT), UT, tid, u0, nu_t, c0 + TOPNW_ITEMS);
        }
    }
    static __device__ __forceinline__ T item_value(const Params &P, int item, bool live) { return (P.biasB != nullptr && live) ? P.biasB[item] : T(0); }
    // the key of the pair, or NaN where its bound shows it below thr; j = 4 t + r names the lane's accumulator
    template <int NUT>
    static __device__ __forceinline__ T pair_key(const Params &P, TileState<NUT> &ts, int j, T acc, T bias, unsigned char *xs, int UT, int u, int user,
                                                 int item, bool ok, T thr)
    {
        const T s = acc + bias;
        if (!ok) return T(NAN);
        if constexpr (LSE) {
            bool in = s > T(-INFINITY);                                // (NaN and -inf add nothing)
            if (P.excl_p != nullptr) {
                const int idx = item & (TOPNW_ITEMS - 1);
                const unsigned w = Lds(xs, UT).mask[((size_t)((item / TOPNW_ITEMS) & 1) * UT + u) * 4 + (idx >> 5)];
                in = in && !((w >> (idx & 31)) & 1u);
            }
            if (in) ts.l[j].add(s, P.inv_t);
        }
        const unsigned long long h = topnsm_hash(P.seed, user, item);
        if (!(topnsm_fma<T>(P.temperature, topnsm_gumbel_bound<T>(h), s) >= thr)) return T(NAN);
        return topnsm_fma<T>(P.temperature, topnsm_gumbel(h, T(0)), s);
    }
    template <int NUT>
    static __device__ __forceinline__ void tile_end(const Params &P, TileState<NUT> &ts, unsigned char *xs, int u0, int nu_t, int UT, int tid)
    {
        if constexpr (LSE) {
            const Lds L(xs, UT);
            const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
            for (int j = 0; j < 4 * NUT; j++) {
                TopnSampleLse &l = ts.l[j];
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) {
                    const float m2 = __shfl_xor(l.m, d);
                    const double s2 = __shfl_xor(l.s, d);
                    l.merge(m2, s2, P.inv_t);
                }
                if ((lane & 15) == 0) {
                    const int u = 16 * (j >> 2) + MfmaAcc<T>::row_of(lane, j & 3);
                    L.wm[wave * UT + u] = l.m; L.wsum[wave * UT + u] = l.s;
                }
            }
            __syncthreads();
            if (tid < nu_t) {
                TopnSampleLse l{L.wm[tid], L.wsum[tid]};
                for (int w = 1; w < TOPNW_NW; w++) l.merge(L.wm[w * UT + tid], L.wsum[w * UT + tid], P.inv_t);
                P.out_lse[u0 + tid] = l.s > 0.0 ? (double)l.m / (double)P.temperature + log(l.s) : -INFINITY;
            }
        }
    }
    static __device__ __forceinline__ bool admit(const unsigned char *, int, int, int, T) { return true; }
    static __device__ __forceinline__ size_t out_stride(const Params &P) { return (size_t)P.n_top; }
    static __device__ __forceinline__ int item_begin(const Params &) { return 0; }
    static __device__ __forceinline__ int item_end(const Params &P) { return P.n; }
};

template <typename T, int NUT, bool LSE>
__global__ void __launch_bounds__(TOPNW_TH)
topn_sample_kernel(const TopnSampleParams<T> P)
{
    topn_wide_body<T, NUT, TopnSamplePolicy<T, LSE>, true>(P);
}

// out_sc[u, j] = the score of (u, P.out_ids[u, j]) with topn_wide_kernel's bits, -inf where the id is -1.
// grid (ceil(nu / 16), n_top), one wavefront each.
template <typename T>
__global__ void __launch_bounds__(64)
topn_sample_scores_kernel(const TopnSampleParams<T> P, T *__restrict__ out_sc)
{
    using Acc = MfmaAcc<T>;
    using vec = typename Acc::vec;
    constexpr int V = 16 / sizeof(T), CH = 4 * V;
    typedef T ldv __attribute__((ext_vector_type(V)));
    const int lane = threadIdx.x, col = lane & 15, grp = lane >> 4;
    const int j = blockIdx.y, ut = blockIdx.x * 16 + col;
    const int u = min(ut, P.nu - 1);
    const int id = P.out_ids[(size_t)u * P.n_top + j];
    const int nchunk = topnw_kp(P.k, sizeof(T)) / CH;
    const T *arow = P.A + (size_t)u * P.lda;
    const T *brow = P.B + (size_t)max(id, 0) * P.ldb + grp * V;
    vec acc = vec{0, 0, 0, 0};
    for (int c = 0; c < nchunk; c++) {
        const ldv b = *reinterpret_cast<const ldv *>(brow + c * CH);
#pragma unroll
        for (int e = 0; e < V; e++) {
            const int f = c * CH + grp * V + e;
            acc = Acc::mma(f < P.k ? arow[f] : T(0), b[e], acc);
        }
    }
    if (ut >= P.nu) return;
    const T bias = (P.biasB != nullptr && id >= 0) ? P.biasB[id] : T(0);
#pragma unroll
    for (int r = 0; r < 4; r++)
        if (Acc::row_of(lane, r) == col) out_sc[(size_t)u * P.n_top + j] = id >= 0 ? acc[r] + bias : T(-INFINITY);
}

// The sampling kernel and the score kernel behind it on st; nut / blocks_per_cu as pick_user_tiles gave them for
// topnsm_extra_per_user(lse) bytes per user.  out_lse != null asks for the log-partition.  Returns the ranking grid.
int topn_sample_launch(hipStream_t st, int num_cus, int nut, int blocks_per_cu, const TopnSampleParams<real_t> &P, real_t *out_scores);

}  // namespace cmfhip
