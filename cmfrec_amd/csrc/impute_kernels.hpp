// impute_kernels.hpp -- the missing entries of a dense block of rows, filled in place from the factors, on the matrix cores.
//
// impute_X_collective_explicit (reference src/collective.c:11351-11544) ends in "keep what is present, predict what is NaN":
//   X[r, c] = isnan(X[r, c]) ? sum_{f < kk} A[r, f] B[c, f] + glob_mean + biasA[r] + biasB[c] : X[r, c]
// Here that is one kernel on a row-major block X[rows, ldx]: the tile product A B^T on the 16x16x4 MFMA of the working type,
// fused with the test and the store, so that the predictions of the present entries are never formed and never written
// (DESIGN.md section 3.7).  It skips what the reference's TODO at :11392 names: rows without a missing entry.
//
//   workgroup  = IMPUTE_NW wavefronts on 16 * NUT rows (NUT = 1, 2 or 4 row tiles -- 1 or 2 in single precision --, chosen on the host by rows and LDS) and a run
//                of column tiles; its rows' factors sit in LDS, zero-padded to KS columns by index (nothing outside [0, kk) of a
//                factor row is read), KS * sizeof(T) = 16 bytes times an odd number as in topn_wide_kernels.hpp
//   wavefront  : one column tile of CW = 128 bytes / sizeof(T) columns at a time (16 in double, 2 x 16 in single precision)
//                against all NUT row tiles
//   X layout   : lane l touches column (l mod CW) of the rows (l / CW) + (64 / CW) i of a row tile: every load and every store
//                instruction of a wavefront covers whole 128-byte runs along a row, 4 rows (double) or 2 rows (single) each
//   skipping   : a row whose count of missing entries is 0 (row_missing, optional) is never loaded; a wavefront reads its X tiles
//                first and votes: no NaN in any of them -> no item load, no product, no store; otherwise the product runs for the
//                row tiles that hold a NaN only, and only the lanes whose entry was NaN store
//   operands   : MFMA step e of a chunk takes factor  chunk * 4V + (lane >> 4) * V + e  of the row (lane & 15) for both operands
//                (V = 16 bytes / sizeof(T)): the rows' from LDS in one 16-byte read, the items' straight from global memory in one
//                16-byte load along k (the tail of a row by element, masked by index)
//   results    : lane l holds column (l & 15) of the rows MfmaAcc<T>::row_of(l, r).  In double precision that IS the X layout;
//                in single precision the accumulator map gives 64-byte runs, so the two 16-column halves of a tile go through a
//                wavefront-private LDS tile [16][IMPUTE_SCR_LD] and come back in the X layout
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dense_kernels.hpp"
#include "dense_rows_device.hpp"
#include "launch.hpp"

namespace cmfhip {

constexpr int IMPUTE_NW = 4;                    // wavefronts per workgroup (one per SIMD)
constexpr int IMPUTE_TH = 64 * IMPUTE_NW;
constexpr int IMPUTE_KMAX = 272;                // the widest model the library fits
// row tiles per workgroup: at most 16 X entries per lane and round (4 x 4 in double, 2 x 8 in single precision)
__host__ __device__ constexpr int impute_max_nut(size_t sizeof_real) { return sizeof_real == 8 ? 4 : 2; }
constexpr size_t IMPUTE_LDS_TARGET = 48 * 1024; // three workgroups per CU
constexpr int IMPUTE_SCR_LD = 36;               // row stride of the single-precision exchange tile (4 rows apart = 16 banks apart)

// columns of a row's factors in LDS: kk rounded up to the chunk of 64 bytes, plus one 16-byte slot
__host__ __device__ inline int impute_ks(int kk, size_t sizeof_real)
{
    const int ch = (int)(64 / sizeof_real);
    return (kk + ch - 1) / ch * ch + (int)(16 / sizeof_real);
}
__host__ __device__ inline size_t impute_lds_bytes(int nut, int kk, size_t sizeof_real)
{
    return (size_t)16 * nut * impute_ks(kk, sizeof_real) * sizeof_real +
           (sizeof_real == 4 ? (size_t)IMPUTE_NW * 16 * IMPUTE_SCR_LD * sizeof_real : 0);
}
// row tiles per workgroup: as many as the rows fill and the LDS target holds (one always fits: 35 KB at kk = 272 in double)
inline int impute_pick_nut(int rows, int kk, size_t sizeof_real)
{
    int nut = std::min(rows <= 16 ? 1 : (rows <= 32 ? 2 : 4), impute_max_nut(sizeof_real));
    while (nut > 1 && impute_lds_bytes(nut, kk, sizeof_real) > IMPUTE_LDS_TARGET) nut >>= 1;
    return nut;
}

template <typename T>
struct ImputeParams {
    T *X; size_t ldx; int rows, n;           // the block, filled in place
    const T *A; size_t lda;                  // the rows' factors, first used column
    const T *B; size_t ldb; int kk;          // the items' factors, first used column; kk = k + k_main
    const T *biasA; size_t ldbias;           // or null; the bias of row r at biasA[r * ldbias]
    const T *biasB;                          // or null
    T glob_mean;
    const int *row_missing;                  // or null; 0: the row holds no NaN and is left alone
    int tiles_per_block;                     // column tiles of one workgroup (blockIdx.y)
};

template <typename T, int NUT>
__global__ void __launch_bounds__(IMPUTE_TH)
impute_fill_kernel(const ImputeParams<T> P)
{
    using Acc = MfmaAcc<T>;
    using vec = typename Acc::vec;
    constexpr int V = 16 / sizeof(T);                               // factors per 16-byte load
    constexpr int CH = 4 * V;                                       // factors per chunk
    constexpr int CW = 128 / sizeof(T);                             // columns of a wavefront's tile
    constexpr int NS = CW / 16;                                     // its 16-column halves
    constexpr int RI = 64 / CW;                                     // rows per X instruction
    constexpr int NI = 16 / RI;                                     // X entries per lane and row tile
    constexpr int UT = 16 * NUT;
    typedef T ldv __attribute__((ext_vector_type(V)));
    extern __shared__ __attribute__((aligned(16))) unsigned char impute_smem[];
    const int kk = P.kk, KS = impute_ks(kk, sizeof(T)), nchunk = (KS - V) / CH;
    T *As = reinterpret_cast<T *>(impute_smem);                     // [UT][KS]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (uniform to the compiler too)
    const int col = lane & 15, grp = lane >> 4;
    const int xcol = lane % CW, xrow = lane / CW;
    const int r0 = blockIdx.x * UT, nr = min(UT, P.rows - r0);
    // bit (NI t + i) of `live`: the lane's i-th row of row tile t exists and has something missing
    unsigned live = 0;
#pragma unroll
    for (int t = 0; t < NUT; t++)
#pragma unroll
        for (int i = 0; i < NI; i++) {
            const int row = 16 * t + xrow + RI * i;
            if (row < nr && (P.row_missing == nullptr || P.row_missing[r0 + row] != 0)) live |= 1u << (NI * t + i);
        }
    if (__ballot(live != 0) == 0) return;                           // (every wavefront sees all rows: the whole workgroup)
    for (int e = tid; e < UT * KS; e += IMPUTE_TH) {
        const int u = e / KS, f = e % KS;
        As[e] = (u < nr && f < kk) ? P.A[(size_t)(r0 + u) * P.lda + f] : T(0);
    }
    __syncthreads();
    const T *arow = As + col * KS + grp * V;
    const int ntiles = (P.n + CW - 1) / CW;
    const int ct0 = blockIdx.y * P.tiles_per_block, ct1 = min(ntiles, ct0 + P.tiles_per_block);
    for (int ct = ct0 + wave; ct < ct1; ct += IMPUTE_NW) {          // (no workgroup barrier below: the trip counts differ)
        const int c0 = ct * CW, xc = c0 + xcol;
        const bool colok = xc < P.n;
        T xv[NUT][NI];
#pragma unroll
        for (int t = 0; t < NUT; t++)
#pragma unroll
            for (int i = 0; i < NI; i++) {
                xv[t][i] = T(0);
                if (colok && ((live >> (NI * t + i)) & 1u)) xv[t][i] = P.X[(size_t)(r0 + 16 * t + xrow + RI * i) * P.ldx + xc];
            }
        unsigned nan = 0;
        bool any[NUT], any_tile = false;
#pragma unroll
        for (int t = 0; t < NUT; t++) {
            unsigned mine = 0;
#pragma unroll
            for (int i = 0; i < NI; i++) if (dense_is_nan(xv[t][i])) mine |= 1u << (NI * t + i);
            nan |= mine;
            any[t] = __ballot(mine != 0) != 0;                      // wave-uniform
            any_tile |= any[t];
        }
        if (!any_tile) continue;
        // the product: the 16 (2 x 16) item rows of this tile, 16 bytes per lane along k, one chunk ahead
        const T *brow[NS];
#pragma unroll
        for (int s = 0; s < NS; s++) brow[s] = P.B + (size_t)min(c0 + 16 * s + col, P.n - 1) * P.ldb;
        auto item_chunk = [&](int c, ldv (&b)[NS]) {
            const int f0 = c * CH + grp * V;
#pragma unroll
            for (int s = 0; s < NS; s++) {
                if (f0 + V <= kk) __builtin_memcpy(&b[s], brow[s] + f0, sizeof(ldv));       // (rows of B are not 16-byte aligned)
                else {
#pragma unroll
                    for (int e = 0; e < V; e++) b[s][e] = (f0 + e < kk) ? brow[s][f0 + e] : T(0);
                }
            }
        };
        vec acc[NUT][NS];
#pragma unroll
        for (int t = 0; t < NUT; t++)
#pragma unroll
            for (int s = 0; s < NS; s++) acc[t][s] = vec{0, 0, 0, 0};
        ldv bcur[NS], bnext[NS];
        item_chunk(0, bcur);
        for (int c = 0; c < nchunk; c++) {
            if (c + 1 < nchunk) item_chunk(c + 1, bnext);
#pragma unroll
            for (int t = 0; t < NUT; t++) {
                if (!any[t]) continue;
                const ldv a = *reinterpret_cast<const ldv *>(arow + t * 16 * KS + c * CH);
#pragma unroll
                for (int e = 0; e < V; e++)
#pragma unroll
                    for (int s = 0; s < NS; s++) acc[t][s] = Acc::mma(a[e], bcur[s][e], acc[t][s]);
            }
#pragma unroll
            for (int s = 0; s < NS; s++) bcur[s] = bnext[s];
        }
        const T bB = (P.biasB != nullptr && colok) ? P.biasB[xc] : T(0);
#pragma unroll
        for (int t = 0; t < NUT; t++) {
            if (!any[t]) continue;
            T out[NI];
            if constexpr (NS == 1) {                                // row_of(l, i) = (l >> 4) + 4 i = xrow + RI i
#pragma unroll
                for (int i = 0; i < NI; i++) out[i] = acc[t][0][i];
            } else {
                T *scr = As + UT * KS + wave * 16 * IMPUTE_SCR_LD;
#pragma unroll
                for (int s = 0; s < NS; s++)
#pragma unroll
                    for (int r = 0; r < 4; r++) scr[Acc::row_of(lane, r) * IMPUTE_SCR_LD + 16 * s + col] = acc[t][s][r];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
                for (int i = 0; i < NI; i++) out[i] = scr[(xrow + RI * i) * IMPUTE_SCR_LD + xcol];
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
#pragma unroll
            for (int i = 0; i < NI; i++) {
                if (!((nan >> (NI * t + i)) & 1u)) continue;
                T v = out[i] + P.glob_mean;
                if (P.biasA != nullptr) v += P.biasA[(size_t)(r0 + 16 * t + xrow + RI * i) * P.ldbias];
                v += bB;
                P.X[(size_t)(r0 + 16 * t + xrow + RI * i) * P.ldx + xc] = v;
            }
        }
    }
}

template <typename T, int NUT>
inline void launch_impute_fill_nut(const DeviceInfo &dev, hipStream_t st, ImputeParams<T> P)
{
    constexpr int CW = 128 / sizeof(T);
    const size_t smem = impute_lds_bytes(NUT, P.kk, sizeof(T));
    HIP_CHECK(hipFuncSetAttribute((const void *)impute_fill_kernel<T, NUT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const long row_blocks = ((long)P.rows + 16 * NUT - 1) / (16 * NUT);
    const long ntiles = ((long)P.n + CW - 1) / CW;
    // column groups: enough workgroups for eight per CU, at least IMPUTE_NW tiles each (one per wavefront)
    long groups = std::max<long>(1, ((long)dev.num_cus * 8 + row_blocks - 1) / row_blocks);
    groups = std::min<long>(std::min<long>(groups, (ntiles + IMPUTE_NW - 1) / IMPUTE_NW), 65535);
    long per = (ntiles + groups - 1) / groups;
    per = (per + IMPUTE_NW - 1) / IMPUTE_NW * IMPUTE_NW;
    groups = (ntiles + per - 1) / per;
    P.tiles_per_block = (int)per;
    poison_lds(st, dev.num_cus);
    hipLaunchKernelGGL((impute_fill_kernel<T, NUT>), dim3((unsigned)row_blocks, (unsigned)groups), dim3(IMPUTE_TH), smem, st, P);
    HIP_CHECK(hipGetLastError());
}

// the launch of the fill on a block that is on the device (P.tiles_per_block is set here)
template <typename T>
inline void launch_impute_fill(const DeviceInfo &dev, hipStream_t st, const ImputeParams<T> &P)
{
    if (P.rows <= 0 || P.n <= 0) return;
    switch (impute_pick_nut(P.rows, P.kk, sizeof(T))) {
        case 1: launch_impute_fill_nut<T, 1>(dev, st, P); break;
        case 2: launch_impute_fill_nut<T, 2>(dev, st, P); break;
        default:
            if constexpr (impute_max_nut(sizeof(T)) >= 4) launch_impute_fill_nut<T, 4>(dev, st, P);
            break;
    }
}

}  // namespace cmfhip
