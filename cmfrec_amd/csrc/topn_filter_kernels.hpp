// topn_filter_kernels.hpp -- the certified half-precision filter in front of the exact ranking.
//
// The full ranking scores every (user, item) pair in the working precision and throws all but n_top of them away.  Here the pass
// over the items runs on v_mfma_f32_16x16x32_f16 against a half-precision image of the item factors and keeps, per user, the M best
// KEYS -- a key is the half-precision score plus a bound on everything that separates it from the score the exact kernels
// compute, so  key(u, j) >= score(u, j)  for every pair.  The M ids are then rescored exactly (topn_filter_refine_kernel, with the
// arithmetic of the kernel the unfiltered call would run, bit for bit), and the user is certified when its n_top-th exact score is
// strictly above tau[u], the M-th key: no item outside the shortlist can score higher.
//
//   image      : topn_filter_image_kernel, once per ranker.  Bh [n][kh] halves, kh = k rounded up to 32, columns [k, kh) zero;
//                Bh = half(B * 2^sb), one power of two for the matrix (its largest |entry| lands in [2^13, 2^14)), halves below the
//                smallest normal flushed to zero (the matrix instruction never sees a subnormal).  Per item two floats, rounded
//                upwards: nb = |b~|, db = |b - b~|, b~ = Bh * 2^-sb, measured in double from the values themselves -- rounding,
//                flushing and clamping are all inside db.
//   workgroup  = TOPNF_NW wavefronts, 16 * NUT users (NUT = 1, 2, 4 or 8 user tiles, chosen on the host by what fits the LDS: a
//                factor takes two bytes here, so twice the exact kernel's tiles fit)
//   user side  : a wavefront per user row converts it on the fly with the row's OWN power of two (topnf_convert_row), measures
//                na = |a~| and da = |a - a~| the same way and leaves the halves in LDS, rows KS = kh + 8 halves apart (16 bytes times
//                an odd number: the 16 users of one ds_read_b128 fall into different 16-byte slots).  A row with a non-finite
//                entry, or one of 2^41 and more, is skipped: its keys are NaN, which never enter, and its state is 0.
//   item side  : a round is 16 items per wavefront; a wavefront streams ITS 16 image rows, 16 bytes (8 halves) per lane, PF loads
//                in flight, and scores them against all NUT user tiles: one MFMA per tile and 32 factors.  Lane l holds factors
//                32 c + 8 (l >> 4) + 0..7 of chunk c for both operands -- whatever factor the hardware pairs with an element, it
//                is the same for both, and the product does not see a common permutation.
//   results    : lane l holds item (l & 15) against users 16 t + 4 (l >> 4) + r of tile t, r = 0..3 (the f32 C/D map)
//   key        : s = acc * 2^-(sa + sb);  e0 = na (db + C nb) + (da + W (na + da)) (nb + db),  C = 2 (kh + 8) 2^-22 (the sum inside
//                the matrix instruction, truncation assumed at every addition),  W = (kh + 8) * 2 u (the rounding of the exact
//                kernels themselves, u the unit roundoff of the working precision);
//                key = s + bias + ((e0 + 2^-21 (|s| + |bias| + e0)) (1 + 2^-20) + 2^-120)   -- the second term covers rounding the
//                bias to float, the two additions and the exact kernels' final addition, the factor every rounding of e0 itself,
//                the constant every underflow.
//   lists      : topn_wide_body's scheme on float keys: per user in LDS a sorted list of M entries and TOPNF_CAND candidate slots; a
//                key enters the candidates only if it is not below the user's current M-th best and (then) the item is not in the
//                exclusion list; a wavefront per user sorts the candidates, folds them in by the first stage of a bitonic merge and
//                finishes the merge; what found no slot is offered again against the raised threshold.
//   output     : per user tau = the M-th key (-inf while the list is not full), and the M ids (free slots 0x7fffffff)
//   refinement : topn_filter_refine_kernel, a wavefront per user.  The user's row sits zero-padded in LDS; the M shortlisted rows
//                of the ranker's packed B are scored 16 at a time.  WIDE: the 16x16x4 MFMA chain of topn_wide_body -- the user in
//                all 16 rows of the A operand, the 16 items in the columns, the same chunks in the same order, then + bias --, so
//                a score has the bits topn_wide_kernel gives it.  Otherwise (k <= 64 on the default route): topn_kernel's sum,
//                s = bias; s += a[f] * b[f] over 64 zero-padded factors in order.  The M (score, id) pairs are sorted by the
//                ranking's total order (bitonic, in LDS) and the first n_top written.
// topn_filter_keys_kernel is the same body with the selection replaced by a store of every key (a probe for tests).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "topn_kernels.hpp"
#include "topn_wide_kernels.hpp"

namespace cmfhip {

constexpr int TOPNF_NW = 8;                   // wavefronts per workgroup
constexpr int TOPNF_TH = 64 * TOPNF_NW;
constexpr int TOPNF_ITEMS = 16 * TOPNF_NW;    // items per round
constexpr int TOPNF_CAND = 32;                // candidate slots per user
constexpr int TOPNF_KMAX = 272;
constexpr int TOPNF_ROW_REGS = (TOPNF_KMAX + 63) / 64;   // values of a row per lane while it is converted
constexpr int TOPNF_MAX_NUT = 8;
constexpr int TOPNF_NTOP_MAX = 64;            // longer lists take the exact route
constexpr int TOPNF_M_MIN = 32, TOPNF_M_MAX = 128;
constexpr int TOPNF_EXP_MAX = 40;             // a row whose largest |entry| is 2^41 or more is not filtered
constexpr size_t TOPNF_LDS_MAX = 160 * 1024;
constexpr int TOPNF_FREE = 0x7fffffff;        // id of a free shortlist slot

typedef _Float16 topnf_h8 __attribute__((ext_vector_type(8)));
typedef float topnf_f4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int topnf_kh(int k) { return (k + 31) / 32 * 32; }
__host__ __device__ inline int topnf_ks(int k) { return topnf_kh(k) + 8; }
// shortlist length: max(32, pow2(2 n_top)), at most 128; forced (32 .. 128, test hook) rounds up to a power of two and is held
// to n_top at least
__host__ __device__ inline int topnf_m(int n_top, int forced)
{
    const int want = (forced >= TOPNF_M_MIN && forced <= TOPNF_M_MAX) ? (forced > n_top ? forced : n_top) : 2 * n_top;
    int m = TOPNF_M_MIN;
    while (m < want && m < TOPNF_M_MAX) m <<= 1;
    return m;
}
__host__ __device__ inline size_t topnf_lds_bytes(int nut, int k, int m)
{
    const size_t ut = 16 * (size_t)nut, ls = (size_t)m + TOPNF_CAND;
    return ut * topnf_ks(k) * sizeof(_Float16) + ut * sizeof(topnf_f4) + ut * ls * (sizeof(float) + sizeof(int)) +
           ut * (sizeof(float) + sizeof(int)) + 2 * sizeof(int);
}
// the scale 2^sexp that brings a largest |entry| of float bits `mbits` into [2^13, 2^14); a zero or tiny row stops at 2^54
__host__ __device__ inline int topnf_scale_exp(unsigned mbits)
{
    const int e = (int)(mbits >> 23) - 127;
    const int s = 13 - e;
    return s > 54 ? 54 : s;
}
__host__ __device__ inline bool topnf_out_of_range(unsigned mbits) { return mbits >= ((unsigned)(127 + TOPNF_EXP_MAX + 1) << 23); }   // inf, NaN too

template <typename T>
struct TopnFilterParams {
    const T *A; size_t lda; int nu;          // users' factors, first used column
    const _Float16 *Bh; int n, k;            // the image [n][topnf_kh(k)], rows 16-byte aligned
    const float *nb, *db; int sb;            // per item |b~| and |b - b~| (rounded upwards), the image's scale exponent
    const T *biasB;                          // or null
    const size_t *excl_p; const int *excl_i; // per-user exclusion lists, each sorted ascending; or null
    int m;                                   // shortlist length: a power of two, 32 .. 128
    int *short_ids;                          // [nu][m], free slots TOPNF_FREE
    float *tau; int *state;                  // [nu] the m-th key; 1 = filtered, 0 = skipped (non-finite or out of range)
    float *keys;                             // probe only: [nu][n]
};

__device__ __forceinline__ void topnf_lds_sync()
{
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// a non-negative double as a float that is not below it
__device__ __forceinline__ float topnf_up(double x)
{
    float f = (float)x;
    if ((double)f < x) f = __uint_as_float(__float_as_uint(f) + 1u);
    return f;
}

__device__ __forceinline__ double topnf_pow2(int e) { return __longlong_as_double((long long)(1023 + e) << 52); }

// One wavefront turns a row of k values into halves: dst[0 .. ncol) <- half(src * 2^sexp), zero beyond k, halves below the
// smallest normal flushed, the product held to +-2^15.  OWN: sexp is chosen from the row's largest |entry| (else it is given).
// nrm / dlt: |row~| and |row - row~| of row~ = dst * 2^-sexp, rounded upwards.  Returns false, with a row of zeros, for a row with a
// non-finite entry or one of 2^41 and more.  ncol <= 64 * TOPNF_ROW_REGS.  Wave-uniform.
template <typename T, bool OWN>
__device__ __forceinline__ bool topnf_convert_row(const T *src, int k, int ncol, int &sexp, _Float16 *dst, int lane, float &nrm, float &dlt)
{
    T v[TOPNF_ROW_REGS];
    unsigned mbits = 0;
#pragma unroll
    for (int i = 0; i < TOPNF_ROW_REGS; i++) {
        const int f = lane + 64 * i;
        v[i] = f < k ? src[f] : T(0);
        mbits = max(mbits, __float_as_uint(fabsf((float)v[i])));             // (a NaN's bits lie above infinity's)
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mbits = max(mbits, (unsigned)__shfl_xor((int)mbits, o));
    const bool ok = !topnf_out_of_range(mbits);
    if (OWN) sexp = topnf_scale_exp(mbits);
    const double sc = topnf_pow2(sexp), isc = topnf_pow2(-sexp);
    double n2 = 0, d2 = 0;
#pragma unroll
    for (int i = 0; i < TOPNF_ROW_REGS; i++) {
        const int f = lane + 64 * i;
        _Float16 h = (_Float16)0.0f;
        if (ok) {
            const double x = fmin(fmax((double)v[i] * sc, -32768.0), 32768.0);
            h = (_Float16)(float)x;
            if (fabsf((float)h) < 6.103515625e-05f) h = (_Float16)0.0f;      // below 2^-14: subnormal as a half
            const double t = (double)(float)h * isc, d = (double)v[i] - t;
            n2 += t * t; d2 += d * d;
        }
        if (f < ncol) dst[f] = h;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { n2 += __shfl_xor(n2, o); d2 += __shfl_xor(d2, o); }
    nrm = topnf_up(sqrt(n2) * (1.0 + 0x1p-30));
    dlt = topnf_up(sqrt(d2) * (1.0 + 0x1p-30));
    return ok;
}

// the largest |entry| of B [n, ldb] (columns [0, k)) and of bias [n] (or null) as float bits: out[0], out[1], zero before the launch
template <typename T>
__global__ void __launch_bounds__(256)
topn_filter_absmax_kernel(const T *__restrict__ B, size_t ldb, int n, int k, const T *__restrict__ bias, unsigned *out)
{
    unsigned mb = 0, mbias = 0;
    const size_t cells = (size_t)n * (size_t)k;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < cells; e += (size_t)gridDim.x * blockDim.x) {
        const size_t i = e / (size_t)k, f = e % (size_t)k;
        mb = max(mb, __float_as_uint(fabsf((float)B[i * ldb + f])));
        if (f == 0 && bias != nullptr) mbias = max(mbias, __float_as_uint(fabsf((float)bias[i])));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mb = max(mb, (unsigned)__shfl_xor((int)mb, o));
        mbias = max(mbias, (unsigned)__shfl_xor((int)mbias, o));
    }
    if ((threadIdx.x & 63) == 0) { atomicMax(&out[0], mb); atomicMax(&out[1], mbias); }
}

// the image: a wavefront per item row
template <typename T>
__global__ void __launch_bounds__(256)
topn_filter_image_kernel(const T *__restrict__ B, size_t ldb, int n, int k, int sb, _Float16 *__restrict__ Bh, float *__restrict__ nb,
                         float *__restrict__ db)
{
    const int lane = threadIdx.x & 63, kh = topnf_kh(k);
    const int waves = (int)(gridDim.x * (blockDim.x >> 6));
    for (int i = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); i < n; i += waves) {
        float nrm, dlt;
        int s = sb;
        (void)topnf_convert_row<T, false>(B + (size_t)i * ldb, k, kh, s, Bh + (size_t)i * kh, lane, nrm, dlt);
        if (lane == 0) { nb[i] = nrm; db[i] = dlt; }
    }
}

template <typename T, int NUT, bool PROBE>
__device__ __forceinline__ void topn_filter_body(const TopnFilterParams<T> P)
{
    constexpr int UT = 16 * NUT;
    constexpr int PF = 4;                                           // image-row loads in flight per lane
    extern __shared__ __attribute__((aligned(16))) unsigned char topnf_smem[];
    const int k = P.k, M = P.m;
    const int KS = topnf_ks(k), nchunk = topnf_kh(k) / 32, LS = M + TOPNF_CAND;
    _Float16 *As = reinterpret_cast<_Float16 *>(topnf_smem);        // [UT][KS]
    topnf_f4 *upar = reinterpret_cast<topnf_f4 *>(As + UT * KS);    // [UT] {2^-(sa + sb), na, da + W (na + da), -}
    float *ssc = reinterpret_cast<float *>(upar + UT);              // [UT][LS]: [0, M) sorted list, [M, LS) candidates
    float *thr = ssc + UT * LS;                                     // [UT] the current M-th best key (-inf until full)
    int *sid = reinterpret_cast<int *>(thr + UT);                   // [UT][LS]
    int *cnt = sid + UT * LS;                                       // [UT] candidates offered since the last merge
    int *flag = cnt + UT;                                           // [2] "a lane still holds a candidate", alternating
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int col = lane & 15, grp = lane >> 4;
    const float NEG = -INFINITY;
    const float cacc = (float)(2 * (topnf_kh(k) + 8)) * 0x1p-22f;                                   // C
    const float cwrk = (float)(topnf_kh(k) + 8) * (sizeof(T) == 8 ? 0x1p-52f : 0x1p-23f);           // W
    int turn = 0;
    if (tid < 2) flag[tid] = 0;
    for (int u0 = blockIdx.x * UT; u0 < P.nu; u0 += gridDim.x * UT) {
        const int nu_t = min(UT, P.nu - u0);
        __syncthreads();
        for (int u = wave; u < UT; u += TOPNF_NW) {                 // wave-uniform
            float na = 0, da = 0;
            int sa = 0;
            bool ok = false;
            if (u < nu_t) ok = topnf_convert_row<T, true>(P.A + (size_t)(u0 + u) * P.lda, k, KS, sa, As + u * KS, lane, na, da);
            else
                for (int f = lane; f < KS; f += 64) As[u * KS + f] = (_Float16)0.0f;
            if (lane == 0) {
                // (sa + sb lies in [-54, 108]: the factor is a normal float; NaN for a row that is skipped)
                const float mu = ok ? (float)topnf_pow2(-(sa + P.sb)) : __uint_as_float(0x7fc00000u);
                upar[u] = topnf_f4{mu, na, da + cwrk * (na + da), 0.0f};
                if (!PROBE && u < nu_t) P.state[u0 + u] = ok ? 1 : 0;
            }
        }
        if (!PROBE) {
            for (int e = tid; e < UT * LS; e += TOPNF_TH) { ssc[e] = NEG; sid[e] = TOPNF_FREE; }
            if (tid < UT) { cnt[tid] = 0; thr[tid] = NEG; }
        }
        __syncthreads();
        const _Float16 *arow = As + col * KS + grp * 8;
        const int kh = topnf_kh(k);
        auto item_row = [&](int c0) { return P.Bh + (size_t)min(c0 + 16 * wave + col, P.n - 1) * kh + grp * 8; };
        const _Float16 *brow = item_row(0);
        topnf_h8 bq[PF];
#pragma unroll
        for (int p = 0; p < PF; p++) bq[p] = *reinterpret_cast<const topnf_h8 *>(brow + min(p, nchunk - 1) * 32);
        for (int c0 = 0; c0 < P.n; c0 += TOPNF_ITEMS) {
            const int item = c0 + 16 * wave + col;
            const bool live = item < P.n;
            const float nbj = live ? P.nb[item] : 0.0f, dbj = live ? P.db[item] : 0.0f;
            const float bj = (live && P.biasB != nullptr) ? (float)P.biasB[item] : 0.0f;
            const float pj = dbj + cacc * nbj, qj = nbj + dbj;
            topnf_f4 acc[NUT];
#pragma unroll
            for (int t = 0; t < NUT; t++) acc[t] = topnf_f4{0, 0, 0, 0};
            auto score_chunk = [&](const topnf_h8 &b, int c) {
#pragma unroll
                for (int t = 0; t < NUT; t++) {
                    const topnf_h8 a = *reinterpret_cast<const topnf_h8 *>(arow + t * 16 * KS + c * 32);
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[t], 0, 0, 0);
                }
            };
            int c = 0;
            for (; c + PF <= nchunk; c += PF) {
#pragma unroll
                for (int p = 0; p < PF; p++) {
                    const topnf_h8 b = bq[p];
                    bq[p] = *reinterpret_cast<const topnf_h8 *>(brow + min(c + p + PF, nchunk - 1) * 32);   // (past the end: a repeat, unused)
                    score_chunk(b, c + p);
                }
            }
#pragma unroll
            for (int p = 0; p < PF - 1; p++)
                if (c + p < nchunk) score_chunk(bq[p], c + p);                   // uniform
            brow = item_row(c0 + TOPNF_ITEMS);
#pragma unroll
            for (int p = 0; p < PF; p++) bq[p] = *reinterpret_cast<const topnf_h8 *>(brow + min(p, nchunk - 1) * 32);
            // keys; bit (4 t + r) of `pend` = this lane still has to offer its key for user 16 t + 4 grp + r
            unsigned pend = 0;
#pragma unroll
            for (int t = 0; t < NUT; t++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int u = 16 * t + 4 * grp + r;
                    const topnf_f4 up = upar[u];
                    const float s = acc[t][r] * up[0];
                    const float e0 = fmaf(up[1], pj, up[2] * qj);
                    const float key = (s + bj) + ((e0 + 0x1p-21f * (fabsf(s) + fabsf(bj) + e0)) * (1.0f + 0x1p-20f) + 0x1p-120f);
                    acc[t][r] = key;
                    if (PROBE) {
                        if (live && u < nu_t) P.keys[(size_t)(u0 + u) * (size_t)P.n + item] = key;
                    } else if (live && u < nu_t && key >= thr[u]) {              // NaN never enters
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
            if (PROBE) continue;
            bool more;
            do {
#pragma unroll
                for (int t = 0; t < NUT; t++) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const unsigned bit = 1u << (4 * t + r);
                        if (pend & bit) {
                            const int u = 16 * t + 4 * grp + r;
                            if (!(acc[t][r] >= thr[u])) pend &= ~bit;            // the threshold has passed it meanwhile
                            else {
                                const int pos = atomicAdd(&cnt[u], 1);
                                if (pos < TOPNF_CAND) {
                                    ssc[u * LS + M + pos] = acc[t][r];
                                    sid[u * LS + M + pos] = item;
                                    pend &= ~bit;
                                }
                            }
                        }
                    }
                }
                if (pend) flag[turn & 1] = 1;
                __syncthreads();
                if (tid == 0) flag[(turn + 1) & 1] = 0;
                for (int u = wave; u < nu_t; u += TOPNF_NW) {                    // merge: one wavefront per user
                    const int nc = min(cnt[u], TOPNF_CAND);
                    if (nc == 0) continue;                                       // wave-uniform
                    float *sc = ssc + u * LS; int *id = sid + u * LS;
                    float *csc = sc + M; int *cid = id + M;
                    int W = 1;
                    while (W < nc) W <<= 1;                                      // <= TOPNF_CAND <= M
                    for (int size = 2; size <= W; size <<= 1) {                  // candidates, best first (free slots hold -inf)
                        for (int stride = size >> 1; stride > 0; stride >>= 1) {
                            if (lane < W / 2) {
                                const int i = 2 * lane - (lane & (stride - 1)), j = i + stride;
                                const bool up = ((i & size) == 0) || (size == W);
                                const float si = csc[i], sj = csc[j]; const int ii = cid[i], ij = cid[j];
                                const bool swap = up ? topn_before(sj, ij, si, ii) : topn_before(si, ii, sj, ij);
                                if (swap) { csc[i] = sj; csc[j] = si; cid[i] = ij; cid[j] = ii; }
                            }
                            topnf_lds_sync();
                        }
                    }
                    // (list descending | -inf ... | candidates ascending) is bitonic: the first stage of its merge leaves the
                    // better of list[M - 1 - j] and candidate j in the list half, which holds the best M and is bitonic again
                    if (lane < W) {
                        const int i = M - 1 - lane;
                        const float sl = sc[i], sb = csc[lane]; const int il = id[i], ib = cid[lane];
                        if (topn_before(sb, ib, sl, il)) { sc[i] = sb; id[i] = ib; }
                        csc[lane] = NEG; cid[lane] = TOPNF_FREE;
                    }
                    topnf_lds_sync();
                    for (int stride = M >> 1; stride > 0; stride >>= 1) {
                        if (lane < M / 2) {                                      // M / 2 <= 64
                            const int i = 2 * lane - (lane & (stride - 1)), j = i + stride;
                            const float si = sc[i], sj = sc[j]; const int ii = id[i], ij = id[j];
                            if (topn_before(sj, ij, si, ii)) { sc[i] = sj; sc[j] = si; id[i] = ij; id[j] = ii; }
                        }
                        topnf_lds_sync();
                    }
                    if (lane == 0) { cnt[u] = 0; thr[u] = sc[M - 1]; }
                }
                more = flag[turn & 1] != 0;
                turn++;
                __syncthreads();
            } while (more);
        }
        if (PROBE) continue;
        // the shortlists and tau
        for (int e = tid; e < nu_t * M; e += TOPNF_TH) {
            const int u = e / M, j = e % M;
            P.short_ids[(size_t)(u0 + u) * (size_t)M + j] = sid[u * LS + j];
        }
        if (tid < nu_t) P.tau[u0 + tid] = ssc[tid * LS + M - 1];
    }
}

template <typename T, int NUT>
__global__ void __launch_bounds__(TOPNF_TH)
topn_filter_kernel(const TopnFilterParams<T> P)
{
    topn_filter_body<T, NUT, false>(P);
}

template <typename T>
__global__ void __launch_bounds__(TOPNF_TH)
topn_filter_keys_kernel(const TopnFilterParams<T> P)
{
    topn_filter_body<T, 1, true>(P);
}

constexpr int TOPNF_REFINE_NW = 4;           // wavefronts (users at a time) per workgroup of the refinement
constexpr int TOPNF_ROW = 288;               // a user's zero-padded row: topnw_kp of the widest model, 16-byte slots

template <typename T>
struct TopnRefineParams {
    const T *A; size_t lda; int nu;          // users' factors, first used column
    const T *B; size_t ldb; int n, k;        // the ranker's packed items: ldb = topnw_kp(k), columns [k, ldb) zero
    const T *biasB;                          // or null
    const int *short_ids; int m;             // [nu][m] shortlists of topn_filter_kernel
    int n_top;
    int *out_ids; T *out_scores;             // [nu, n_top]
};

template <typename T, bool WIDE>
__global__ void __launch_bounds__(64 * TOPNF_REFINE_NW)
topn_filter_refine_kernel(const TopnRefineParams<T> P)
{
    using Acc = MfmaAcc<T>;
    constexpr int V = 16 / sizeof(T), CH = 4 * V;
    typedef T ldv __attribute__((ext_vector_type(V)));
    __shared__ __attribute__((aligned(16))) T rows[TOPNF_REFINE_NW][TOPNF_ROW];
    __shared__ T ssc[TOPNF_REFINE_NW][TOPNF_M_MAX];
    __shared__ int sid[TOPNF_REFINE_NW][TOPNF_M_MAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int k = P.k, M = P.m, ntop = P.n_top;
    const T NEG = -INFINITY;
    T *arow = rows[wave], *sc = ssc[wave];
    int *id = sid[wave];
    const int waves = (int)gridDim.x * TOPNF_REFINE_NW;
    for (int u = (int)blockIdx.x * TOPNF_REFINE_NW + wave; u < P.nu; u += waves) {    // wave-uniform
        for (int f = lane; f < TOPNF_ROW; f += 64) arow[f] = f < k ? P.A[(size_t)u * P.lda + f] : T(0);
        topnf_lds_sync();
        const int *sl = P.short_ids + (size_t)u * (size_t)M;
        if (WIDE) {
            const int col = lane & 15, grp = lane >> 4, nchunk = topnw_kp(k, sizeof(T)) / CH;
            for (int j0 = 0; j0 < M; j0 += 16) {
                const int item = sl[j0 + col];
                const bool live = item >= 0 && item < P.n;
                const T *brow = P.B + (size_t)(live ? item : 0) * P.ldb + grp * V;
                typename Acc::vec acc = {0, 0, 0, 0};
                for (int c = 0; c < nchunk; c++) {
                    const ldv b = *reinterpret_cast<const ldv *>(brow + c * CH);
                    const ldv a = *reinterpret_cast<const ldv *>(arow + c * CH + grp * V);
#pragma unroll
                    for (int e = 0; e < V; e++) acc = Acc::mma(a[e], b[e], acc);
                }
                // (all 16 rows of the tile hold this user: every r of every lane group has the score; lanes 0..15 write theirs)
                const T s = acc[0] + ((P.biasB != nullptr && live) ? P.biasB[item] : T(0));
                if (grp == 0) {
                    const bool in = live && s == s;                              // a NaN never enters
                    sc[j0 + col] = in ? s : NEG; id[j0 + col] = in ? item : TOPNF_FREE;
                }
            }
        } else {
            for (int j = lane; j < M; j += 64) {
                const int item = sl[j];
                const bool live = item >= 0 && item < P.n;
                const T *brow = P.B + (size_t)(live ? item : 0) * P.ldb;
                T b[TOPN_KMAX];
#pragma unroll
                for (int f = 0; f < TOPN_KMAX; f++) b[f] = (f < k) ? brow[f] : T(0);
                T s = (P.biasB != nullptr && live) ? P.biasB[item] : T(0);
#pragma unroll
                for (int f = 0; f < TOPN_KMAX; f++) s += arow[f] * b[f];
                const bool in = live && s == s;
                sc[j] = in ? s : NEG; id[j] = in ? item : TOPNF_FREE;
            }
        }
        topnf_lds_sync();
        for (int size = 2; size <= M; size <<= 1) {                              // best first
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                if (lane < M / 2) {                                              // M / 2 <= 64
                    const int i = 2 * lane - (lane & (stride - 1)), j = i + stride;
                    const bool up = (i & size) == 0;
                    const T si = sc[i], sj = sc[j]; const int ii = id[i], ij = id[j];
                    const bool swap = up ? topn_before(sj, ij, si, ii) : topn_before(si, ii, sj, ij);
                    if (swap) { sc[i] = sj; sc[j] = si; id[i] = ij; id[j] = ii; }
                }
                topnf_lds_sync();
            }
        }
        for (int j = lane; j < ntop; j += 64) {                                  // (n_top <= M)
            const T sv = sc[j];
            P.out_ids[(size_t)u * ntop + j] = (sv == NEG) ? -1 : id[j];
            P.out_scores[(size_t)u * ntop + j] = sv;
        }
        topnf_lds_sync();
    }
}

// certified[u] = the user was filtered, and its shortlist was not full or its n_top-th exact score lies strictly above tau[u]
template <typename T>
__global__ void __launch_bounds__(256)
topn_filter_certify_kernel(const T *__restrict__ scores, int nu, int n_top, const float *__restrict__ tau, const int *__restrict__ state,
                           int *__restrict__ certified)
{
    const int u = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (u >= nu) return;
    const float t = tau[u];
    certified[u] = (state[u] == 1 && (t == -INFINITY || (double)scores[(size_t)u * n_top + n_top - 1] > (double)t)) ? 1 : 0;
}

}  // namespace cmfhip
