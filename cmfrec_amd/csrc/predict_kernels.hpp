// predict_kernels.hpp -- the predicted value of chosen (row, col) pairs: score_pairs_kernel and its launch helper
// launch_score_pairs, the one way to it (cmfrec_hip_score_pairs, the scorer handle, cmfrec_hip_newrows_predict and the four
// predict_X_* names: predict_tu.hip).  DESIGN.md section 3.8.  The kernel's loop is score_chunks, which score_errors_kernel
// (predict_error_kernels.hpp) runs too: "stores" below is the epilogue of this kernel, ScoreStore.
//
//   explicit:  row in [0, m) and col in [0, n):  a . b + biasA[row] + biasB[col] + glob_mean   (a missing bias adds nothing)
//              otherwise:                        glob_mean + (biasA[row] if row in [0, m)) + (biasB[col] if col in [0, n))
//   implicit:  a . b, otherwise NaN (biasA, biasB and glob_mean are not read, whether given or not)
// with a = A[row * lda + 0 .. kk), b = B[col * ldb + 0 .. kk).
//
// Work split.  A row of kk elements is cut into 16-byte pieces of Ve = 16 / sizeof(T) elements.  A group of G lanes owns a pair,
// G the power of two that covers the pieces (at most 64); lane g of the group takes pieces g, g + G, ... and accumulates their
// products in element order with fused multiply-adds, the elements past kk as zeros.  An xor butterfly over the G lanes (DPP
// inside 16-lane rows, permlane swaps across them: lanes.hpp) leaves the sum in every lane of the group: every level adds the
// same two values in both partner lanes, so a pair's bits depend on kk and on the two rows, not on the group, the wavefront or
// the position of the pair in the call.  Lane 0 of the group adds biasA, biasB, glob_mean in that order and stores.
// A wavefront handles 64 / G pairs per step and SCORE_STEPS steps at once: the index loads of all steps, then the 2 * SCORE_STEPS
// independent 16-byte loads of a round, then the arithmetic -- the kernel was expected to wait on gather latency, not on the ALUs (DESIGN.md 3.8 reads the measurement).
// A pair out of range is decided here (no host pass over row / col); none of its lanes loads from A or B.
//
// Load width.  VA / VB say that the pointer and the leading dimension of A / B are multiples of 16 bytes: a piece is then one
// 16-byte load (the row's last piece whole: its elements past kk, which belong to the image, are replaced by zeros).  Otherwise
// the same lane <-> element map is fetched element by element.  The arithmetic is the same code on the same values: the bits of a
// prediction do not depend on the width.  No LDS, no atomics, vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <limits>

#include "lanes.hpp"

namespace cmfhip {

template <typename T>
struct ScoreParams {
    const T *A = nullptr; size_t lda = 0; int m = 0;       // [m, lda], from the first scored column
    const T *B = nullptr; size_t ldb = 0; int n = 0;       // [n, ldb]
    int kk = 0;
    const T *biasA = nullptr; size_t ldbiasA = 1;          // biasA[row * ldbiasA] (a column of A's image: ldbiasA = lda), or null
    const T *biasB = nullptr;                              // biasB[col], or null
    T glob_mean = 0;
    const int *row = nullptr, *col = nullptr;
    T *out = nullptr;
    size_t n_pairs = 0;
    int implicit = 0;                                      // the fallback rule: NaN instead of glob_mean + the biases in range
};

constexpr int SCORE_TH = 256;          // threads per workgroup
constexpr int SCORE_STEPS = 4;         // steps in flight per wavefront

template <typename T> constexpr int score_ve() { return 16 / (int)sizeof(T); }

// lanes per pair for rows of kk elements
template <typename T> inline int score_group_width(int kk)
{
    const int pieces = (kk + score_ve<T>() - 1) / score_ve<T>();
    int G = 1;
    while (G < pieces && G < 64) G *= 2;
    return G;
}

// one piece of a row into registers.  The wide form brings the elements past kk of the row's last piece along as they are in
// the image; the arithmetic replaces them by zeros after the wait, so that nothing between the loads of a round depends on one.
template <typename T, bool VEC>
__device__ __forceinline__ void score_load_piece(const T *p, int e0, int kk, T (&v)[16 / sizeof(T)])
{
    constexpr int Ve = 16 / (int)sizeof(T);
    if constexpr (VEC) {
        typedef T Vec __attribute__((ext_vector_type(Ve)));
        const Vec x = *reinterpret_cast<const Vec *>(p + e0);
#pragma unroll
        for (int e = 0; e < Ve; e++) v[e] = x[e];
    } else {
#pragma unroll
        for (int e = 0; e < Ve; e++) v[e] = (e0 + e < kk) ? p[e0 + e] : (T)0;
    }
}

// sum over the G lanes of a group (G consecutive lanes, aligned to G), the same bits in each of them
template <int G, typename T>
__device__ __forceinline__ T score_group_sum(T v)
{
    if constexpr (G >= 2) v += lanes::xor1(v);
    if constexpr (G >= 4) v += lanes::xor2(v);
    if constexpr (G >= 8) v += lanes::qxor4(v);
    if constexpr (G >= 16) v += lanes::xor8(v);
    if constexpr (G >= 32) v = lanes::tswap16_add(v, v);
    if constexpr (G >= 64) v = lanes::tswap32_add(v, v);
    return v;
}

// The wavefront's loop over its chunks of (64 / G) * SCORE_STEPS pairs, shared by score_pairs_kernel and score_errors_kernel
// (predict_error_kernels.hpp): the prediction of a pair is the same code in both.  What happens to it is the epilogue's business:
//   epi.begin(u, i, mine)    before the index loads of step u are waited for; mine: this lane is lane 0 of the group of the live pair i
//   epi.middle(u, i, mine)   after the last round's arithmetic, in front of the butterflies (the registers of the pieces are free again)
//   epi.end(u, i, ok, res)   on that lane alone, after the butterfly: ok = the pair is inside the model, res = its prediction
// Returns the wavefront's index and the number of wavefronts of the launch through wave / nwaves.
template <typename T, int G, bool VA, bool VB, typename Epi>
__device__ __forceinline__ void score_chunks(const ScoreParams<T> &P, Epi &epi, size_t &wave, size_t &nwaves)
{
    constexpr int Ve = 16 / (int)sizeof(T), PS = 64 / G, U = SCORE_STEPS;
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
    wave = (size_t)blockIdx.x * (SCORE_TH / 64) + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    nwaves = (size_t)gridDim.x * (SCORE_TH / 64);
    constexpr size_t per_chunk = (size_t)PS * U;
    const size_t chunks = (P.n_pairs + per_chunk - 1) / per_chunk;
    const int kk = P.kk;
    const int rounds = ((kk + Ve - 1) / Ve + G - 1) / G;
    // (chunks, rounds and the loop over them are wavefront-uniform: all 64 lanes reach the cross-lane moves of the butterfly)
    for (size_t c = wave; c < chunks; c += nwaves) {
        size_t pr[U];
        int rr[U], cc[U];
        bool live[U], ok[U];
        const T *pa[U], *pb[U];
        T ba[U], bb[U], acc[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            pr[u] = c * per_chunk + (size_t)(u * PS + sub);
            live[u] = pr[u] < P.n_pairs;
            rr[u] = live[u] ? P.row[pr[u]] : -1;
            cc[u] = live[u] ? P.col[pr[u]] : -1;
            epi.begin(u, pr[u], g == 0 && live[u]);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const bool ra = rr[u] >= 0 && rr[u] < P.m, cb = cc[u] >= 0 && cc[u] < P.n;
            ok[u] = ra && cb;
            pa[u] = P.A + (size_t)(ok[u] ? rr[u] : 0) * P.lda;
            pb[u] = P.B + (size_t)(ok[u] ? cc[u] : 0) * P.ldb;
            // the biases of the side that is in range: needed by the explicit model's scored pair and by its fallback alike
            // (the implicit rule knows no bias: none is loaded)
            const bool need = g == 0 && live[u] && !P.implicit;
            ba[u] = (need && ra && P.biasA) ? P.biasA[(size_t)rr[u] * P.ldbiasA] : (T)0;
            bb[u] = (need && cb && P.biasB) ? P.biasB[cc[u]] : (T)0;
            acc[u] = (T)0;
        }
        for (int rd = 0; rd < rounds; rd++) {
            const int e0 = (rd * G + g) * Ve;
            T a[U][Ve], b[U][Ve];
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (ok[u] && e0 < kk) {
                    score_load_piece<T, VA>(pa[u], e0, kk, a[u]);
                    score_load_piece<T, VB>(pb[u], e0, kk, b[u]);
                } else {
#pragma unroll
                    for (int e = 0; e < Ve; e++) { a[u][e] = (T)0; b[u][e] = (T)0; }
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int e = 0; e < Ve; e++) {
                    const bool in = e0 + e < kk;
                    acc[u] = fma(in ? a[u][e] : (T)0, in ? b[u][e] : (T)0, acc[u]);
                }
        }
#pragma unroll
        for (int u = 0; u < U; u++) epi.middle(u, pr[u], g == 0 && live[u]);
#pragma unroll
        for (int u = 0; u < U; u++) {
            const T dot = score_group_sum<G>(acc[u]);
            if (g == 0 && live[u]) {
                T res;
                if (ok[u]) {
                    res = dot;
                    if (!P.implicit) {
                        if (P.biasA) res += ba[u];
                        if (P.biasB) res += bb[u];
                        res += P.glob_mean;
                    }
                } else if (P.implicit) {
                    res = std::numeric_limits<T>::quiet_NaN();
                } else {
                    res = P.glob_mean;
                    if (P.biasA && rr[u] >= 0 && rr[u] < P.m) res += ba[u];
                    if (P.biasB && cc[u] >= 0 && cc[u] < P.n) res += bb[u];
                }
                epi.end(u, pr[u], ok[u], res);
            }
        }
    }
}

template <typename T>
struct ScoreStore {
    T *out;
    __device__ __forceinline__ void begin(int, size_t, bool) {}
    __device__ __forceinline__ void middle(int, size_t, bool) {}
    __device__ __forceinline__ void end(int, size_t i, bool, T res) { out[i] = res; }
};

template <typename T, int G, bool VA, bool VB>
__global__ __launch_bounds__(SCORE_TH) void score_pairs_kernel(const ScoreParams<T> P)
{
    ScoreStore<T> epi{P.out};
    size_t wave, nwaves;
    score_chunks<T, G, VA, VB>(P, epi, wave, nwaves);
}

// grid-stride launch: as many workgroups as are resident at once (by the kernel's own register use: 5 to 7 wavefronts per SIMD),
// so that every wavefront gets the same share of the steps
template <typename K, typename T>
inline void launch_score_kernel(K kernel, hipStream_t st, size_t blocks, int num_cus, const ScoreParams<T> &P)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, SCORE_TH, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    const int grid = (int)std::min<size_t>(blocks, (size_t)num_cus * (size_t)per_cu);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(SCORE_TH), 0, st, P);
}

template <typename T, int G>
inline void launch_score_width(hipStream_t st, size_t blocks, int num_cus, const ScoreParams<T> &P, bool va, bool vb)
{
    if (va && vb) launch_score_kernel(score_pairs_kernel<T, G, true, true>, st, blocks, num_cus, P);
    else if (va) launch_score_kernel(score_pairs_kernel<T, G, true, false>, st, blocks, num_cus, P);
    else if (vb) launch_score_kernel(score_pairs_kernel<T, G, false, true>, st, blocks, num_cus, P);
    else launch_score_kernel(score_pairs_kernel<T, G, false, false>, st, blocks, num_cus, P);
}

// may this operand be fetched 16 bytes at a time?  Its pointer and its row pitch are multiples of 16 bytes.  The image then holds
// the last piece of every row whole: device images start on a 16-byte boundary, so the operand starts a whole number of pieces
// into a row whose length is a whole number of pieces and at least kk.
template <typename T> inline bool score_wide_ok(const T *p, size_t ld)
{
    return ((uintptr_t)p % 16) == 0 && (ld * sizeof(T)) % 16 == 0;
}

// Launches the kernel on P.n_pairs pairs (device pointers; nothing is launched for none).  The caller has checked kk >= 1,
// lda / ldb >= kk and that A / B are there when m / n > 0.
template <typename T>
inline void launch_score_pairs(hipStream_t st, int num_cus, const ScoreParams<T> &P)
{
    if (P.n_pairs == 0) return;
    const int G = score_group_width<T>(P.kk);
    const size_t per_chunk = (size_t)(64 / G) * SCORE_STEPS, per_block = per_chunk * (SCORE_TH / 64);
    const size_t blocks = (P.n_pairs + per_block - 1) / per_block;
    const bool va = P.m > 0 && score_wide_ok(P.A, P.lda), vb = P.n > 0 && score_wide_ok(P.B, P.ldb);
    switch (G) {
    case 1: launch_score_width<T, 1>(st, blocks, num_cus, P, va, vb); break;
    case 2: launch_score_width<T, 2>(st, blocks, num_cus, P, va, vb); break;
    case 4: launch_score_width<T, 4>(st, blocks, num_cus, P, va, vb); break;
    case 8: launch_score_width<T, 8>(st, blocks, num_cus, P, va, vb); break;
    case 16: launch_score_width<T, 16>(st, blocks, num_cus, P, va, vb); break;
    case 32: launch_score_width<T, 32>(st, blocks, num_cus, P, va, vb); break;
    default: launch_score_width<T, 64>(st, blocks, num_cus, P, va, vb); break;
    }
}

}  // namespace cmfhip
