// subspace_kernels.hpp -- the subspace (iALS++) half-step: block Gauss-Seidel on a row's normal equations, 16 unknowns at a time.
// DESIGN.md section 3.22 derives the arithmetic; tests/subspace_reference.py restates it in NumPy.
//
// The row's system is W a = r with W = G0 + D + sum_j g_j b_j b_j^T and r = sum_j y_j b_j (implicit: G0 = B^T B, g_j = the stored
// value alpha x_j, y_j = g_j + 1; explicit: no G0, g_j = 1, y_j = x_j - bias_sub[j]; D = diag(lam .. lam, lam_last)).  With
// yhat_j = a . b_j kept per entry, one step on the block pi of 16 consecutive unknowns is
//     grad = G0[pi, :] a + D_pi a_pi + sum_j (g_j yhat_j - y_j) b_j[pi]          ( = (W a - r)[pi] )
//     H    = G0[pi, pi] + D_pi + sum_j g_j b_j[pi] b_j[pi]^T                      ( = W[pi, pi], unit diagonal on the padding )
//     d    = -H^-1 grad ;  a_pi += d ;  yhat_j += b_j[pi] . d
// and a half-step is `sweeps` passes over the blocks in ascending order.
//
// Work split.  A team of NW wavefronts owns a row at a time and strides over the positions [row_first, row_end) of the shard's
// processing order (longest rows first): NW = 1 for rows of up to SUB_WAVE_ROW entries, four teams to a workgroup, which never
// meet at a barrier; NW = 4, one workgroup, for longer rows.  Every sum has one order, fixed by the row and the team width: no
// atomics, and a half-step returns the same bytes twice.
// Data movement.  The block's operand b_j[pi] is 16 elements per entry (128 / 64 bytes): PL = 8 / 4 lanes fetch one entry, 16 bytes
// each (VEC; element by element where the opposing matrix is not 16-byte aligned), into a slab S [entry][SUB_LDS] in LDS.  The
// row's yhat, g and y live in LDS beside it.  A row of up to `cap` entries is resident: the slab gathered for H is the one the
// yhat update reads.  A longer row goes through the same loops in chunks of `cap` entries: its yhat lives in the global slice
// yhat[st .. st + nnz) (st: the row's CSR offset), g and y are formed again per chunk, the block is gathered twice.
// Matrix pipe.  H is accumulated four entries per v_mfma_{f64,f32}_16x16x4: lane (q, i) = (lane >> 4, lane & 15) feeds
// g_e S[e][i] and S[e][i] of entry e = 4 s + q as the A and B operands.  The gradient is vector code in the same loop: one FMA per
// step into the lane's partial over q, summed by two permlane swaps.  G0[pi, :] a is read down G0's columns (G0 is symmetric,
// so 16 lanes read 16 consecutive elements), the columns dealt over q and the team's wavefronts.  chol_diag_block
// (chol_kernels.hpp) factorises H and leaves inv(R) in LDS; d = -inv(R) (inv(R)^T grad) is two 16-term dot products on 16 lanes.  A
// pivot that is not positive makes the hardware rsq return NaN: the row comes out NaN, no other row is touched.
// Phase 0.  yhat_j = a . b_j over the full width by 16 lanes per entry, 16 bytes per lane and round (as predict_kernels.hpp
// gathers), summed inside the 16-lane row by DPP.
#pragma once
#include <hip/hip_runtime.h>

#include "cg_kernels.hpp"
#include "chol_kernels.hpp"
#include "lanes.hpp"
#include "predict_kernels.hpp"

namespace cmfhip {

template <typename T>
struct SubspaceParams {
    T *A = nullptr; size_t lda = 0;            // row r -> A + r * lda: its k unknowns, in and out
    const T *B = nullptr; size_t ldb = 0;      // opposing rows, the first k columns
    int k = 0;
    const int *indices = nullptr; const T *values = nullptr;
    const T *bias_sub = nullptr;               // explicit: y_j = x_j - bias_sub[idx_j], or null
    const T *G0 = nullptr;                     // implicit: B^T B [k, k] without lambda; explicit: null
    T lam = 0, lam_last = 0;
    int implicit = 0;
    int sweeps = 1;
    int cap = 0;                               // entries of a row that stay in LDS (a multiple of 4, at most the team's maximum)
    const RowDesc *desc = nullptr;             // the processing order: {row, nnz, CSR offset}
    int row_first = 0, row_end = 0;            // its positions this launch handles
    T *yhat = nullptr;                         // [nnz of the shard]: yhat of the rows beyond cap
};

constexpr int SUB_TH = 256;            // threads of a workgroup
constexpr int SUB_WAVE_ROW = 64;       // rows of up to this many entries go to one wavefront
constexpr int SUB_LDS = 17;            // leading dimension of the slab: the yhat update reads S[e][c] with e across the lanes
template <int NW> constexpr int subspace_cap_max() { return NW == 1 ? 64 : 320; }
template <typename T> constexpr int subspace_slot() { return 16 * CholMfma<T>::LDR > 256 ? 16 * CholMfma<T>::LDR : 256; }
// LDS elements of one team: slab, yhat / g / y, the row's unknowns (kp = k rounded up to 16), inv(R), the other wavefronts' tiles,
// every wavefront's gradient partial, then grad | inv(R)^T grad | d
template <typename T, int NW> constexpr size_t subspace_team_elems(int kp)
{
    return (size_t)subspace_cap_max<NW>() * (SUB_LDS + 3) + (size_t)kp + subspace_slot<T>() + (size_t)(NW - 1) * 256 + (size_t)NW * 16 + 48;
}

template <typename T, int NW, bool VEC>
__global__ void __launch_bounds__(SUB_TH)
subspace_rows_kernel(const SubspaceParams<T> P)
{
    using Mf = CholMfma<T>;
    using vec = typename Mf::vec;
    constexpr int CAPMAX = subspace_cap_max<NW>();
    constexpr int NT = 64 * NW, TEAMS = SUB_TH / NT;
    constexpr int Ve = 16 / (int)sizeof(T), PL = 16 / Ve;      // elements of a 16-byte piece; lanes per entry of a slab
    constexpr int LDR = Mf::LDR;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int k = P.k, nb = (k + 15) / 16, kp = 16 * nb;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // wavefront of the workgroup
    const int team_in_block = wv / NW, wave = wv % NW;
    const int lane = threadIdx.x & 63, tid = wave * 64 + lane;
    const int q = lane >> 4, i = lane & 15;
    T *S = reinterpret_cast<T *>(smem_raw) + (size_t)team_in_block * subspace_team_elems<T, NW>(kp);
    T *ysh = S + (size_t)CAPMAX * SUB_LDS, *gsh = ysh + CAPMAX, *tsh = gsh + CAPMAX;
    T *a_s = tsh + CAPMAX;
    T *slot = a_s + kp;
    T *hpart = slot + subspace_slot<T>();
    T *gpart = hpart + (NW - 1) * 256;
    T *v16 = gpart + NW * 16;
    const int cap = P.cap;

    // the team's writes to LDS and to its yhat slice become visible to its other lanes (NW = 1: the teams of a workgroup run
    // different numbers of rows and never meet at a barrier)
    auto team_sync = [&]() {
        if constexpr (NW == 1) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        } else {
            __syncthreads();
        }
    };
    auto entry_gy = [&](size_t pos, int idx, T &g, T &y) {
        const T x = P.values[pos];
        if (P.implicit) { g = x; y = x + T(1); }
        else { g = T(1); y = (P.bias_sub != nullptr) ? x - P.bias_sub[idx] : x; }
    };

    const int nteams = (int)gridDim.x * TEAMS;
    for (int pos = P.row_first + (int)blockIdx.x * TEAMS + team_in_block; pos < P.row_end; pos += nteams) {
        const RowDesc d = P.desc[pos];
        const int nnz = d.nnz;
        const size_t st = (size_t)d.st;
        T *arow = P.A + (size_t)d.row * P.lda;
        const bool resident = nnz <= cap;
        for (int e = tid; e < kp; e += NT) a_s[e] = (e < k) ? arow[e] : T(0);
        team_sync();

        // the slab of block bi for the entries [c0, c0 + cn) of the row; rows [cn, cn4) of it are zeros
        auto gather_slab = [&](int c0, int cn, int cn4, int bi) {
            const int pl = tid % PL, eg = tid / PL;
            const int col = 16 * bi + pl * Ve;
#pragma unroll 2
            for (int e0 = 0; e0 < cn4; e0 += NT / PL) {
                const int e = e0 + eg;
                T b[Ve];
#pragma unroll
                for (int x = 0; x < Ve; x++) b[x] = T(0);
                if (e < cn && col < k) {
                    const int idx = P.indices[st + (size_t)(c0 + e)];
                    score_load_piece<T, VEC>(P.B + (size_t)idx * P.ldb, col, k, b);
                }
                if (e < cn4) {
#pragma unroll
                    for (int x = 0; x < Ve; x++) S[e * SUB_LDS + pl * Ve + x] = (col + x < k) ? b[x] : T(0);
                }
            }
        };

        // ---- phase 0: yhat_j = a . b_j, 16 lanes per entry; the entries' g and y of a resident row ----
        for (int j0 = 0; j0 < nnz; j0 += NT / 16) {
            const int j = j0 + (tid >> 4);
            const bool live = j < nnz;
            const int idx = live ? P.indices[st + (size_t)j] : 0;
            const T *bp = P.B + (size_t)idx * P.ldb;
            T acc = T(0);
            for (int e0 = i * Ve; e0 < k; e0 += 16 * Ve) {
                T b[Ve];
                if (live) {
                    score_load_piece<T, VEC>(bp, e0, k, b);
                } else {
#pragma unroll
                    for (int x = 0; x < Ve; x++) b[x] = T(0);
                }
#pragma unroll
                for (int x = 0; x < Ve; x++) acc = fma((e0 + x < k) ? b[x] : T(0), a_s[e0 + x], acc);
            }
            acc = lanes::row_sum16(acc);
            if (live && i == 0) {
                if (resident) {
                    T g, y;
                    entry_gy(st + (size_t)j, idx, g, y);
                    ysh[j] = acc; gsh[j] = g; tsh[j] = y;
                } else {
                    P.yhat[st + (size_t)j] = acc;
                }
            }
        }
        if (resident && tid < ((nnz + 3) & ~3) - nnz) { ysh[nnz + tid] = T(0); gsh[nnz + tid] = T(0); tsh[nnz + tid] = T(0); }
        team_sync();

        for (int sw = 0; sw < P.sweeps; sw++) {
            for (int bi = 0; bi < nb; bi++) {
                // ---- H on the matrix pipe, the gradient beside it ----
                vec hacc = vec{0, 0, 0, 0};
                T gacc = T(0);
                for (int c0 = 0; c0 < nnz; c0 += cap) {
                    const int cn = min(cap, nnz - c0), cn4 = (cn + 3) & ~3;
                    gather_slab(c0, cn, cn4, bi);
                    if (!resident) {
                        for (int e = tid; e < cn4; e += NT) {
                            T g = T(0), y = T(0), yh = T(0);
                            if (e < cn) {
                                const size_t p = st + (size_t)(c0 + e);
                                entry_gy(p, P.indices[p], g, y);
                                yh = P.yhat[p];
                            }
                            ysh[e] = yh; gsh[e] = g; tsh[e] = y;
                        }
                    }
                    team_sync();
                    for (int s = wave; s < cn4 / 4; s += NW) {
                        const int e = 4 * s + q;
                        const T sv = S[e * SUB_LDS + i], g = gsh[e];
                        const T cj = fma(g, ysh[e], -tsh[e]);
                        hacc = Mf::mma(g * sv, sv, hacc);
                        gacc = fma(cj, sv, gacc);
                    }
                    if (!resident) team_sync();           // the next chunk overwrites the slab and the entries' arrays
                }
                // G0[pi, :] a down the columns of G0: column c = 4 wave + q, then every 4 NW-th
                if (P.G0 != nullptr && 16 * bi + i < k)
                    for (int c = 4 * wave + q; c < k; c += 4 * NW) gacc = fma(P.G0[(size_t)c * k + 16 * bi + i], a_s[c], gacc);
                gacc = lanes::tswap16_add(gacc, gacc);
                gacc = lanes::tswap32_add(gacc, gacc);
                if constexpr (NW > 1) {
                    if (wave > 0) {
#pragma unroll
                        for (int r = 0; r < 4; r++) hpart[(wave - 1) * 256 + r * 64 + lane] = hacc[r];
                    }
                    if (lane < 16) gpart[wave * 16 + lane] = gacc;
                    __syncthreads();
                }
                if (wave == 0) {
                    if constexpr (NW > 1) {
                        gacc = gpart[i];
#pragma unroll
                        for (int w = 1; w < NW; w++) {
                            gacc += gpart[w * 16 + i];
#pragma unroll
                            for (int r = 0; r < 4; r++) hacc[r] += hpart[(w - 1) * 256 + r * 64 + lane];
                        }
                    }
                    // + G0[pi, pi] + D_pi, unit diagonal on the padding
                    const int uj = 16 * bi + i;
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int ui = 16 * bi + Mf::row_of(lane, r);
                        T add = T(0);
                        if (ui < k && uj < k) {
                            if (P.G0 != nullptr) add = P.G0[(size_t)ui * k + uj];
                            if (ui == uj) add += (ui == k - 1) ? P.lam_last : P.lam;
                        } else if (ui == uj) {
                            add = T(1);
                        }
                        hacc[r] += add;
                    }
                    if (uj < k) gacc = fma((uj == k - 1) ? P.lam_last : P.lam, a_s[uj], gacc);
                    if (lane < 16) v16[lane] = gacc;
                    chol_diag_block<T>(hacc, slot, lane, min(16, k - 16 * bi));
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    // d = -inv(R) (inv(R)^T grad)
                    T t = T(0);
#pragma unroll
                    for (int c = 0; c < 16; c++) t = fma(slot[c * LDR + i], v16[c], t);
                    if (lane < 16) v16[16 + lane] = t;
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                    __builtin_amdgcn_wave_barrier();
                    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                    T dl = T(0);
#pragma unroll
                    for (int c = 0; c < 16; c++) dl = fma(slot[i * LDR + c], v16[16 + c], dl);
                    if (lane < 16) {
                        v16[32 + lane] = -dl;
                        if (uj < k) a_s[uj] -= dl;
                    }
                }
                team_sync();
                // ---- yhat_j += b_j[pi] . d : a lane per entry ----
                for (int c0 = 0; c0 < nnz; c0 += cap) {
                    const int cn = min(cap, nnz - c0);
                    if (!resident) {
                        gather_slab(c0, cn, cn, bi);
                        team_sync();
                    }
                    for (int e = tid; e < cn; e += NT) {
                        T acc = T(0);
#pragma unroll
                        for (int c = 0; c < 16; c++) acc = fma(S[e * SUB_LDS + c], v16[32 + c], acc);
                        if (resident) ysh[e] += acc;
                        else P.yhat[st + (size_t)(c0 + e)] += acc;
                    }
                    if (!resident) team_sync();
                }
                team_sync();
            }
        }
        for (int e = tid; e < k; e += NT) arow[e] = a_s[e];
        team_sync();                                       // the next row overwrites a_s
    }
}

}  // namespace cmfhip
