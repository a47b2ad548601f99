// newrows_naz_kernels.hpp -- right-hand sides of a batch of new rows under NA_as_zero: the value-weighted
// gather-sum over two sources, naz_rhs_kernel, its second pass naz_rhs_finish_kernel and the launch helper launch_naz_rhs_kernels.
// Instantiated in newrows_naz_tu.hip only.
//
// Per row r of the batch, with the constant row c (c_side for the rows that have side information, c_plain for the others):
//     rhs[r, koff_x + f] = c[koff_x + f] + sum over the row's entries j of X of  coef_j * Bx[j, f]      f < kx
//     rhs[r, f]         += sum over the row's attributes a of U of              u_a    * Cw[a, f]      f < kc
// coef_j = x_j, or with observation weights  w_j x_j - (w_j - 1)(glob_mean + biasB_j), computed per entry here.
// Bx / Cw are padded device copies of the operand rows: a row starts on a 16-byte boundary and is a whole number of 16-byte
// pieces long, zeros behind its last column.
//
// Work split (the model is predict_kernels.hpp).  A row of `width` elements is cut into 16-byte pieces of Ve elements; a group of
// G lanes owns an entry, G the power of two that covers the pieces of the wider source (at most 64; beyond 64 pieces the
// columns are taken in windows of 64 pieces, one pass over the entries per window).  A wavefront has 64 / G entries per step
// and NAZ_STEPS steps in flight: the index / value loads of all steps, the 16-byte loads of all steps, then the fused
// multiply-adds in step order.  Group `sub` takes the entries sub, sub + 64 / G, ... of its task in that order, so a lane's sum
// has a fixed order; an xor butterfly over the lane bits above the group adds the 64 / G group sums, the same two values in both
// partner lanes of every level.  One wavefront takes one task: a row's entries of one source up to NAZ_SEG; a longer row is cut
// into segments of NAZ_SEG entries from its start.  A row with exactly one task is written at once (c + sum); the others leave
// partial sums that naz_rhs_finish_kernel adds in order: c, the segments of X, the segments of U.  So a row's bits depend on
// its own entries, on G (the model's widths) and on NAZ_SEG -- not on the other rows, their order, or the number of wavefronts
// of the launch (CMFREC_HIP_NAZ_WAVES).  No LDS, no atomics, vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>

#include "lanes.hpp"

namespace cmfhip {

constexpr int NAZ_TH = 256;            // threads per workgroup
constexpr int NAZ_STEPS = 4;           // steps in flight per wavefront
constexpr int NAZ_SEG = 256;           // entries of one task

// one task: `row`'s entries [seg * NAZ_SEG, ...) of source `src` (0: X, 1: U); direct: the row's only task; slot: where its
// partial sum goes otherwise
struct NazTask {
    int row, src_direct, seg, slot;
};
// a row of the second pass: its partial sums are the slots [slot0, slot0 + nx) of X, then [slot0 + nx, slot0 + nx + nu) of U
struct NazFinishRow {
    int row, slot0, nx, nu;
};

template <typename T>
struct NazRhsParams {
    // source 0: X against the padded item rows
    const size_t *xp = nullptr; const int *xi = nullptr; const T *xv = nullptr; const T *xw = nullptr;
    const T *Bx = nullptr; size_t ldbx = 0; int kx = 0, koff_x = 0;
    const T *biasB = nullptr; int n_bias = 0; T glob_mean = 0;   // read with weights only; the items [0, n_bias) carry a bias
    // source 1: U against the padded rows of w_user C (null: none)
    const size_t *up = nullptr; const int *ui = nullptr; const T *uv = nullptr;
    const T *Cw = nullptr; size_t ldcw = 0; int kc = 0;
    const T *c_side = nullptr, *c_plain = nullptr; int rows_side = 0;      // [kt] each, null = zeros
    T *rhs = nullptr; size_t ld = 0; int kt = 0; int rows = 0;
    const NazTask *tasks = nullptr; int ntasks = 0;
    T *partial = nullptr; size_t ldp = 0;                   // [slots, ldp], ldp >= max(kx, kc)
    const NazFinishRow *fin = nullptr; int nfin = 0;
    int gwidth = 0;                                         // the width that chooses G: the model's wider source, whatever the batch holds
};

template <typename T> constexpr int naz_ve() { return 16 / (int)sizeof(T); }

// lanes per entry for rows of `width` elements
template <typename T> inline int naz_group_width(int width)
{
    const int pieces = (width + naz_ve<T>() - 1) / naz_ve<T>();
    int G = 1;
    while (G < pieces && G < 64) G *= 2;
    return G;
}
template <typename T> inline size_t naz_padded_ld(int width) { return (size_t)((width + naz_ve<T>() - 1) / naz_ve<T>() * naz_ve<T>()); }

// sum over the 64 / G groups of a wavefront (lanes with equal lane & (G - 1)), the same bits in each of them
template <int G, typename T>
__device__ __forceinline__ T naz_cross_group_sum(T v)
{
    if constexpr (G <= 1) v += lanes::xor1(v);
    if constexpr (G <= 2) v += lanes::xor2(v);
    if constexpr (G <= 4) v += lanes::xor4(v);
    if constexpr (G <= 8) v += lanes::xor8(v);
    if constexpr (G <= 16) v = lanes::tswap16_add(v, v);
    if constexpr (G <= 32) v = lanes::tswap32_add(v, v);
    return v;
}

// rhs[r, :] = the row's constant, for every row of the batch (the rows without entries keep it)
template <typename T>
__global__ void naz_rhs_init_kernel(const NazRhsParams<T> P)
{
    const size_t total = (size_t)P.rows * (size_t)P.kt;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int r = (int)(e / (size_t)P.kt), f = (int)(e % (size_t)P.kt);
        const T *c = r < P.rows_side ? P.c_side : P.c_plain;
        P.rhs[(size_t)r * P.ld + f] = c != nullptr ? c[f] : T(0);
    }
}

template <typename T, int G>
__global__ __launch_bounds__(NAZ_TH) void naz_rhs_kernel(const NazRhsParams<T> P)
{
    constexpr int Ve = 16 / (int)sizeof(T), PS = 64 / G, U = NAZ_STEPS;
    typedef T Vec __attribute__((ext_vector_type(Ve)));
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
    const int wave = blockIdx.x * (NAZ_TH / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nwaves = gridDim.x * (NAZ_TH / 64);
    // (the tasks, their lengths and the windows are wavefront-uniform: all 64 lanes reach the cross-lane moves)
    for (int t = wave; t < P.ntasks; t += nwaves) {
        const NazTask tk = P.tasks[t];
        const int row = tk.row, src = tk.src_direct & 1;
        const bool direct = (tk.src_direct & 2) != 0;
        const size_t *ptr = src ? P.up : P.xp;
        const int *idx = src ? P.ui : P.xi;
        const T *val = src ? P.uv : P.xv;
        const T *wt = src ? nullptr : P.xw;
        const T *F = src ? P.Cw : P.Bx;
        const size_t ldf = src ? P.ldcw : P.ldbx;
        const int width = src ? P.kc : P.kx, col0 = src ? 0 : P.koff_x;
        const size_t e0 = ptr[row] + (size_t)tk.seg * NAZ_SEG;
        const int len = (int)min((size_t)NAZ_SEG, ptr[row + 1] - e0);
        const T *c = row < P.rows_side ? P.c_side : P.c_plain;
        for (int w0 = 0; w0 < width; w0 += G * Ve) {
            const int f0 = w0 + g * Ve;
            const bool cols = f0 < width;                  // (f0 + Ve <= ldf then: the padded row holds the whole piece)
            T acc[Ve];
#pragma unroll
            for (int e = 0; e < Ve; e++) acc[e] = T(0);
            for (int j0 = 0; j0 < len; j0 += PS * U) {
                int id[U];
                T cf[U];
                bool live[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int j = j0 + u * PS + sub;
                    live[u] = j < len;
                    id[u] = live[u] ? idx[e0 + j] : 0;
                    cf[u] = live[u] ? val[e0 + j] : T(0);
                    if (wt != nullptr && live[u]) {
                        const T w = wt[e0 + j];
                        const T shift = P.glob_mean + ((P.biasB != nullptr && id[u] < P.n_bias) ? P.biasB[id[u]] : T(0));
                        cf[u] = w * cf[u] - (w - T(1)) * shift;
                    }
                }
                Vec v[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if (live[u] && cols) {
                        v[u] = *reinterpret_cast<const Vec *>(F + (size_t)id[u] * ldf + f0);
                    } else {
#pragma unroll
                        for (int e = 0; e < Ve; e++) v[u][e] = T(0);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++)
#pragma unroll
                    for (int e = 0; e < Ve; e++) acc[e] = fma(cf[u], v[u][e], acc[e]);
            }
#pragma unroll
            for (int e = 0; e < Ve; e++) acc[e] = naz_cross_group_sum<G>(acc[e]);
            if (sub == 0 && cols) {
#pragma unroll
                for (int e = 0; e < Ve; e++) {
                    const int f = f0 + e;
                    if (f >= width) continue;
                    if (direct) P.rhs[(size_t)row * P.ld + col0 + f] = (c != nullptr ? c[col0 + f] : T(0)) + acc[e];
                    else P.partial[(size_t)tk.slot * P.ldp + f] = acc[e];
                }
            }
        }
    }
}

// second pass: the rows with more than one task, one wavefront per row, lane <-> column
template <typename T>
__global__ __launch_bounds__(NAZ_TH) void naz_rhs_finish_kernel(const NazRhsParams<T> P)
{
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (NAZ_TH / 64) + (int)(threadIdx.x >> 6), nwaves = gridDim.x * (NAZ_TH / 64);
    for (int i = wave; i < P.nfin; i += nwaves) {
        const NazFinishRow fr = P.fin[i];
        const T *c = fr.row < P.rows_side ? P.c_side : P.c_plain;
        for (int f = lane; f < P.kt; f += 64) {
            T acc = c != nullptr ? c[f] : T(0);
            const int fx = f - P.koff_x;
            if (fx >= 0 && fx < P.kx)
                for (int s = 0; s < fr.nx; s++) acc += P.partial[(size_t)(fr.slot0 + s) * P.ldp + fx];
            if (f < P.kc)
                for (int s = 0; s < fr.nu; s++) acc += P.partial[(size_t)(fr.slot0 + fr.nx + s) * P.ldp + f];
            P.rhs[(size_t)fr.row * P.ld + f] = acc;
        }
    }
}

// dst[r, f] = scale * src[r, off + f] for f < cols, 1 at f == ones_col (if >= 0), zeros up to ldd: the padded operand copies
template <typename T>
__global__ void naz_pad_rows_kernel(const T *__restrict__ src, size_t lds, int off, int cols, T scale, int ones_col, T *__restrict__ dst,
                                    size_t ldd, size_t rows)
{
    const size_t total = rows * ldd;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / ldd; const int f = (int)(e % ldd);
        dst[e] = f < cols ? scale * src[r * lds + off + f] : (f == ones_col ? T(1) : T(0));
    }
}

// per entry of a weighted X: g[e] = w[e] - 1 (the rank-1 weight of its correction of the shared matrix), z[e] = 0
template <typename T>
__global__ void naz_weight_corrections_kernel(const T *__restrict__ w, size_t nnz, T *__restrict__ g, T *__restrict__ z)
{
    const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    g[e] = w[e] - T(1);
    z[e] = T(0);
}

template <typename T, int G>
inline int launch_naz_rhs_width(hipStream_t st, int num_cus, const NazRhsParams<T> &P, int max_waves)
{
    auto kernel = naz_rhs_kernel<T, G>;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, NAZ_TH, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    size_t blocks = ((size_t)P.ntasks + NAZ_TH / 64 - 1) / (NAZ_TH / 64);
    blocks = std::min<size_t>(blocks, (size_t)num_cus * (size_t)per_cu);
    if (max_waves > 0) blocks = std::min<size_t>(blocks, (size_t)(max_waves + NAZ_TH / 64 - 1) / (NAZ_TH / 64));
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(NAZ_TH), 0, st, P);
    return (int)blocks * (NAZ_TH / 64);
}

// The three launches on P.rows rows: the constants, the tasks, the rows of the second pass.  max_waves > 0: at most that many
// wavefronts (rounded up to whole workgroups) take the tasks (test hook CMFREC_HIP_NAZ_WAVES).  Returns the wavefronts of the
// launch of naz_rhs_kernel (0: no task).
template <typename T>
inline int launch_naz_rhs_kernels(hipStream_t st, int num_cus, const NazRhsParams<T> &P, int max_waves)
{
    int waves = 0;
    if (P.rows <= 0) return waves;
    const size_t total = (size_t)P.rows * (size_t)P.kt;
    hipLaunchKernelGGL(naz_rhs_init_kernel<T>, dim3((unsigned)std::min<size_t>((total + 255) / 256, 1 << 16)), dim3(256), 0, st, P);
    if (P.ntasks > 0) {
        switch (naz_group_width<T>(std::max(P.gwidth, std::max(P.kx, P.kc)))) {
        case 1: waves = launch_naz_rhs_width<T, 1>(st, num_cus, P, max_waves); break;
        case 2: waves = launch_naz_rhs_width<T, 2>(st, num_cus, P, max_waves); break;
        case 4: waves = launch_naz_rhs_width<T, 4>(st, num_cus, P, max_waves); break;
        case 8: waves = launch_naz_rhs_width<T, 8>(st, num_cus, P, max_waves); break;
        case 16: waves = launch_naz_rhs_width<T, 16>(st, num_cus, P, max_waves); break;
        case 32: waves = launch_naz_rhs_width<T, 32>(st, num_cus, P, max_waves); break;
        default: waves = launch_naz_rhs_width<T, 64>(st, num_cus, P, max_waves); break;
        }
    }
    if (P.nfin > 0) {
        size_t blocks = ((size_t)P.nfin + NAZ_TH / 64 - 1) / (NAZ_TH / 64);
        if (max_waves > 0) blocks = std::min<size_t>(blocks, (size_t)(max_waves + NAZ_TH / 64 - 1) / (NAZ_TH / 64));
        hipLaunchKernelGGL(naz_rhs_finish_kernel<T>, dim3((unsigned)blocks), dim3(NAZ_TH), 0, st, P);
    }
    return waves;
}

}  // namespace cmfhip
