// topn_explain_kernels.hpp -- why an item was recommended: the score of a (user, target) pair split into one term per item of
// the user's history.
//
// Per user u: W_u = G0 + diag + sum_j g_j b_j b_j^T over the history (b_j the ranker's resident row, [b_j, 1] with a bias
// unknown), a_u = W_u^-1 sum_j y_j b_j, and for a target t
//   c_tj = y_j * b_t^T W_u^-1 b_j,     total_t = sum_j c_tj = b_t . a_u,
// the n_top largest c_tj in descending order, equal values to the earlier history position, -1 / -inf behind a short history.
// A pivot of W_u that is not positive: NaN totals and contributions, ids -1, for that user alone.
//
//   workgroup : TOPNX_NW = 4 wavefronts, one user at a time, users by a static stride over the grid; no atomics, nothing
//               depends on the grid
//   1 build   : the history in slabs of SR = 32 (16 where the LDS is short) rows, gathered by id from the packed B 16 bytes
//               per thread into LDS [SR][KS]; the NT (NT + 1) / 2 upper-triangle 16 x 16 tiles of sum g b b^T (NT = tiles of
//               the k + bias unknowns) are dealt round-robin to the wavefronts (tile t to wavefront t % 4, at most Q = 9 each)
//               and accumulated in registers on the 16x16x4 MFMA of the working type: four history rows per step, operand a
//               = g_h * row_h[16 bi + col], operand b = row_h[16 bj + col].  With a bias, column k of a staged row is one.
//               G0 (device copy) and the diagonal join as the tiles leave the accumulators for LDS; the padding unknowns
//               beyond k + bias get a unit diagonal
//   2 factor  : W = R^T R in LDS on the packed upper-triangle tiles, [16][17] each, blocked and right-looking: wavefront 0
//               factorises and inverts the diagonal tile (chol_diag_block of chol_kernels.hpp; inv(R_kk) stays, [16][LDR]),
//               the panel tiles X_j = inv(R_kk)^T W_kj and the trailing tiles W_ij -= X_i^T X_j are MFMAs dealt to the
//               wavefronts, operands read from the tiles in LDS
//   3 solve   : up to 16 targets per tile: their rows are gathered straight into Z [KW][16] (factor-major), then
//               R^T R Z = B_T^T by blocked forward and backward substitution in place: Z_k <- inv(R_kk)^(T) Z_k by wavefront
//               0, Z_j -= R_kj^T Z_k (forward) / R_jk Z_k (backward) dealt to the wavefronts, all on the MFMA.  Further
//               tiles of targets reuse the factor
//   4 history : per target tile a second pass over the history slabs: wavefront w < SR / 16 forms P = B_hist[16, KW] . Z on
//               the MFMA and leaves y_j * P in LDS; wavefront w then owns the targets w, w + 4, w + 8, w + 12: lane 0..3
//               adds that target's column in double, in history order; all lanes offer the slab's values that reach the
//               target's current n_top-th best to topnc_merge (topn_cand_kernels.hpp) against the target's sorted list in
//               LDS, keyed (value descending, history position ascending)
//   5 store   : plain vector stores; a position becomes the item id there
// Every LDS word that is read was written in the same user's pass.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_base.hpp"
#include "dense_kernels.hpp"
#include "lanes.hpp"
#include "chol_kernels.hpp"
#include "topn_wide_kernels.hpp"
#include "topn_cand_kernels.hpp"

namespace cmfhip {

constexpr int TOPNX_NW = 4;                    // wavefronts per workgroup
constexpr int TOPNX_TH = 64 * TOPNX_NW;
constexpr int TOPNX_KMAX = 128;                // unknowns, the bias included
constexpr int TOPNX_NTOP_MAX = 64;
constexpr int TOPNX_QMAX = 9;                  // tiles per wavefront at 128 unknowns: 36 / 4
constexpr int TOPNX_LD = 17;                   // row stride of a 16 x 16 tile of W in LDS
constexpr int TOPNX_ZS = 16;                   // row stride of Z
constexpr int TOPNX_PS = 17;                   // row stride of the slab's contributions
constexpr size_t TOPNX_LDS_MAX = 160 * 1024;

__host__ __device__ inline int topnx_nt(int ku) { return (ku + 15) / 16; }
// tiles per wavefront the kernel is instantiated for: the least of 1, 3, 6, 9 that holds ceil(NT (NT + 1) / 2 / 4)
__host__ __device__ inline int topnx_q(int ku)
{
    const int nt = topnx_nt(ku);
    return nt <= 2 ? 1 : (nt <= 4 ? 3 : (nt <= 6 ? 6 : TOPNX_QMAX));
}
// tile (bi, bj), bj >= bi, of the packed upper triangle
__host__ __device__ inline int topnx_tile(int bi, int bj, int nt) { return bi * nt - bi * (bi - 1) / 2 + (bj - bi); }

// where the pieces lie in the dynamic LDS, in elements of T from its start (ints behind the Ts)
struct TopnxLayout {
    size_t w, inv, z, slab, pbuf, lsc, csc, sy, sg;       // T
    size_t lid, cid, rowid, flag;                         // int, from the start of the int part
    size_t t_elems, bytes;
};
__host__ __device__ inline TopnxLayout topnx_layout(int ku, int n_top, int sr, size_t sizeof_real)
{
    const size_t nt = (size_t)topnx_nt(ku), kw = 16 * nt, v = 16 / sizeof_real, ks = kw + v;
    const size_t ldr = sizeof_real == 8 ? 17 : 20, np = (size_t)topnc_np(n_top);
    TopnxLayout L;
    size_t o = 0;
    L.w = o;    o += nt * (nt + 1) / 2 * 16 * TOPNX_LD;
    L.inv = o;  o += nt * 16 * ldr;
    L.z = o;    o += kw * TOPNX_ZS;
    L.slab = o; o += (size_t)sr * ks;
    L.pbuf = o; o += (size_t)sr * TOPNX_PS;
    L.lsc = o;  o += 16 * np;
    L.csc = o;  o += TOPNX_NW * 64;
    L.sy = o;   o += (size_t)sr;
    L.sg = o;   o += (size_t)sr;
    L.t_elems = (o + 1) / 2 * 2;
    size_t i = 0;
    L.lid = i;   i += 16 * np;
    L.cid = i;   i += TOPNX_NW * 64;
    L.rowid = i; i += (size_t)sr;
    L.flag = i;  i += 1;
    L.bytes = L.t_elems * sizeof_real + i * sizeof(int);
    return L;
}
// rows per slab: 32, or 16 where 32 do not fit beside the factor
__host__ __device__ inline int topnx_slab_rows(int ku, int n_top, size_t sizeof_real)
{
    return topnx_layout(ku, n_top, 32, sizeof_real).bytes <= TOPNX_LDS_MAX ? 32 : 16;
}

template <typename T>
struct TopnExplainParams {
    const T *B; size_t ldb; int n, k;        // item factors: ldb = topnw_kp(k), columns [k, ldb) zero, rows 16-byte aligned
    int nu, bias, n_top, sr;                 // bias: one more unknown, every row [b, 1]; sr = topnx_slab_rows
    const size_t *hist_p; const int *hist_i; const T *hist_g, *hist_y;   // CSR over the users (ids checked by the host)
    const size_t *targ_p; const int *targ_i;
    const T *G0;                             // [k, k] row-major on the device, or null
    T diag, diag_bias; const T *diag_u, *diag_bias_u;   // diag_u / diag_bias_u [nu] replace diag / diag_bias, or null
    T *out_total; int *out_ids; T *out_contrib;   // [targ_p[nu]], [targ_p[nu], n_top] x 2
};

template <typename T, int Q>
__global__ void __launch_bounds__(TOPNX_TH)
topn_explain_kernel(const TopnExplainParams<T> P)
{
    using Acc = MfmaAcc<T>;
    using vec = typename Acc::vec;
    constexpr int V = 16 / sizeof(T);
    typedef T ldv __attribute__((ext_vector_type(V)));
    constexpr int LD = TOPNX_LD, TS = 16 * TOPNX_LD, ZS = TOPNX_ZS, PS = TOPNX_PS, LDR = CholMfma<T>::LDR, INVS = 16 * LDR;
    constexpr int NONE = 0x7fffffff;
    extern __shared__ __attribute__((aligned(16))) unsigned char topnx_smem[];
    const int k = P.k, ku = k + (P.bias ? 1 : 0), NT = topnx_nt(ku), KW = 16 * NT, KS = KW + V, PR = KW / V;
    const int kp = topnw_kp(k, sizeof(T)), SR = P.sr, ntop = P.n_top, NP = topnc_np(ntop);
    const int ntiles = NT * (NT + 1) / 2;
    const TopnxLayout L = topnx_layout(ku, ntop, SR, sizeof(T));
    T *tb = reinterpret_cast<T *>(topnx_smem);
    int *ib = reinterpret_cast<int *>(tb + L.t_elems);
    T *Wt = tb + L.w, *invR = tb + L.inv, *Z = tb + L.z, *slab = tb + L.slab, *pbuf = tb + L.pbuf;
    T *lsc = tb + L.lsc, *sy = tb + L.sy, *sg = tb + L.sg;
    int *lid = ib + L.lid, *rowid = ib + L.rowid, *flag = ib + L.flag;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, grp = lane >> 4;
    T *csc = tb + L.csc + wave * 64;
    int *cid = ib + L.cid + wave * 64;
    const T NEG = -INFINITY, POS = INFINITY;

    // slot q of this wavefront: tile wave + 4 q of the upper triangle in row-major order -> first columns of its two blocks
    int offa[Q], offb[Q];
#pragma unroll
    for (int q = 0; q < Q; q++) {
        int bi = 0, rem = wave + TOPNX_NW * q;
        if (rem >= ntiles) rem = 0;
        while (rem >= NT - bi) { rem -= NT - bi; bi++; }
        offa[q] = 16 * bi; offb[q] = 16 * (bi + rem);
    }
    // the rows rowid[0 .. rows) into dst, 16 bytes per thread: row r to dst + r * KS, or (TO_Z) as column r of Z
    auto gather = [&](int rows, bool to_z) {
        for (int e = tid; e < rows * PR; e += TOPNX_TH) {
            const int row = e / PR, c0 = (e % PR) * V, rid = rowid[row];
            const bool live = rid >= 0 && rid < P.n;
            ldv v;
#pragma unroll
            for (int i = 0; i < V; i++) v[i] = T(0);
            if (live && c0 < kp) v = *reinterpret_cast<const ldv *>(P.B + (size_t)rid * P.ldb + c0);
            if (P.bias && live) {
#pragma unroll
                for (int i = 0; i < V; i++)
                    if (c0 + i == k) v[i] = T(1);
            }
            if (to_z) {
#pragma unroll
                for (int i = 0; i < V; i++) Z[(c0 + i) * ZS + row] = v[i];
            } else {
                *reinterpret_cast<ldv *>(slab + row * KS + c0) = v;
            }
        }
    };

    for (int u = blockIdx.x; u < P.nu; u += gridDim.x) {
        const size_t tbeg = P.targ_p[u], tend = P.targ_p[u + 1];
        if (tbeg == tend) continue;                                 // (uniform) nothing to explain
        const size_t hbeg = P.hist_p[u];
        const int hlen = (int)(P.hist_p[u + 1] - hbeg);
        __syncthreads();                                            // the user before is done with every buffer
        if (tid == 0) *flag = 0;

        // ---- 1: W_u
        vec acc[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) acc[q] = vec{0, 0, 0, 0};
        for (int s0 = 0; s0 < hlen; s0 += SR) {
            const int nh = min(SR, hlen - s0);
            if (tid < SR) {
                const bool in = tid < nh;
                rowid[tid] = in ? P.hist_i[hbeg + s0 + tid] : -1;
                sg[tid] = in ? P.hist_g[hbeg + s0 + tid] : T(0);
            }
            __syncthreads();
            gather(SR, false);
            __syncthreads();
            const int steps = (nh + 3) / 4;
            for (int s = 0; s < steps; s++) {
                const int h = 4 * s + grp;
                const T gs = sg[h];
                const T *rowp = slab + h * KS + col;
#pragma unroll
                for (int q = 0; q < Q; q++) acc[q] = Acc::mma(gs * rowp[offa[q]], rowp[offb[q]], acc[q]);
            }
            __syncthreads();
        }
        const T dg = P.diag_u != nullptr ? P.diag_u[u] : P.diag, db = P.diag_bias_u != nullptr ? P.diag_bias_u[u] : P.diag_bias;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int t = wave + TOPNX_NW * q;
            if (t < ntiles) {                                       // wave-uniform
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int i = Acc::row_of(lane, r), gi = offa[q] + i, gj = offb[q] + col;
                    T v = acc[q][r];
                    if (P.G0 != nullptr && gi < k && gj < k) v += P.G0[(size_t)gi * k + gj];
                    if (gi == gj) v += gi < k ? dg : (gi < ku ? db : T(1));
                    Wt[t * TS + i * LD + col] = v;
                }
            }
        }
        __syncthreads();

        // ---- 2: W = R^T R
        for (int kb = 0; kb < NT; kb++) {
            T *inv = invR + kb * INVS;
            if (wave == 0) {
                const T *D = Wt + topnx_tile(kb, kb, NT) * TS;
                vec d;
#pragma unroll
                for (int r = 0; r < 4; r++) d[r] = D[Acc::row_of(lane, r) * LD + col];
                chol_diag_block<T>(d, inv, lane, 16);
                topnc_lds_sync();
                const T x = inv[col * LDR + col];                   // 1 / sqrt(pivot): NaN or inf where a pivot is not positive
                if (__ballot(!(x > T(0) && x < POS)) != 0 && lane == 0) *flag = 1;
            }
            __syncthreads();
            for (int bj = kb + 1 + wave; bj < NT; bj += TOPNX_NW) {
                T *X = Wt + topnx_tile(kb, bj, NT) * TS;
                vec c = vec{0, 0, 0, 0};
#pragma unroll
                for (int s = 0; s < 4; s++) c = Acc::mma(inv[(4 * s + grp) * LDR + col], X[(4 * s + grp) * LD + col], c);
#pragma unroll
                for (int r = 0; r < 4; r++) X[Acc::row_of(lane, r) * LD + col] = c[r];
            }
            __syncthreads();
            const int nrem = NT - kb - 1;
            for (int t = wave; t < nrem * (nrem + 1) / 2; t += TOPNX_NW) {
                int ri = 0, rem = t;
                while (rem >= nrem - ri) { rem -= nrem - ri; ri++; }
                const int bi = kb + 1 + ri, bj = bi + rem;
                const T *Xi = Wt + topnx_tile(kb, bi, NT) * TS, *Xj = Wt + topnx_tile(kb, bj, NT) * TS;
                T *C = Wt + topnx_tile(bi, bj, NT) * TS;
                vec c;
#pragma unroll
                for (int r = 0; r < 4; r++) c[r] = C[Acc::row_of(lane, r) * LD + col];
#pragma unroll
                for (int s = 0; s < 4; s++) c = Acc::mma(-Xi[(4 * s + grp) * LD + col], Xj[(4 * s + grp) * LD + col], c);
#pragma unroll
                for (int r = 0; r < 4; r++) C[Acc::row_of(lane, r) * LD + col] = c[r];
            }
            __syncthreads();
        }
        const bool bad = *flag != 0;

        for (size_t t0 = tbeg; t0 < tend; t0 += 16) {
            const int nt = (int)min((size_t)16, tend - t0);
            // ---- 3: Z = W^-1 B_T^T
            if (tid < 16) rowid[tid] = tid < nt ? P.targ_i[t0 + tid] : -1;
            for (int e = tid; e < 16 * NP; e += TOPNX_TH) { lsc[e] = NEG; lid[e] = NONE; }
            __syncthreads();
            gather(16, true);
            __syncthreads();
            for (int kb = 0; kb < NT; kb++) {                       // forward: R^T Y = B_T^T
                const T *inv = invR + kb * INVS;
                T *Zk = Z + 16 * kb * ZS;
                if (wave == 0) {
                    vec c = vec{0, 0, 0, 0};
#pragma unroll
                    for (int s = 0; s < 4; s++) c = Acc::mma(inv[(4 * s + grp) * LDR + col], Zk[(4 * s + grp) * ZS + col], c);
#pragma unroll
                    for (int r = 0; r < 4; r++) Zk[Acc::row_of(lane, r) * ZS + col] = c[r];
                }
                __syncthreads();
                for (int bj = kb + 1 + wave; bj < NT; bj += TOPNX_NW) {
                    const T *Rkj = Wt + topnx_tile(kb, bj, NT) * TS;
                    T *Zj = Z + 16 * bj * ZS;
                    vec c;
#pragma unroll
                    for (int r = 0; r < 4; r++) c[r] = Zj[Acc::row_of(lane, r) * ZS + col];
#pragma unroll
                    for (int s = 0; s < 4; s++) c = Acc::mma(-Rkj[(4 * s + grp) * LD + col], Zk[(4 * s + grp) * ZS + col], c);
#pragma unroll
                    for (int r = 0; r < 4; r++) Zj[Acc::row_of(lane, r) * ZS + col] = c[r];
                }
                __syncthreads();
            }
            for (int kb = NT - 1; kb >= 0; kb--) {                  // backward: R Z = Y
                const T *inv = invR + kb * INVS;
                T *Zk = Z + 16 * kb * ZS;
                if (wave == 0) {
                    vec c = vec{0, 0, 0, 0};
#pragma unroll
                    for (int s = 0; s < 4; s++) c = Acc::mma(inv[col * LDR + 4 * s + grp], Zk[(4 * s + grp) * ZS + col], c);
#pragma unroll
                    for (int r = 0; r < 4; r++) Zk[Acc::row_of(lane, r) * ZS + col] = c[r];
                }
                __syncthreads();
                for (int bj = wave; bj < kb; bj += TOPNX_NW) {
                    const T *Rjk = Wt + topnx_tile(bj, kb, NT) * TS;
                    T *Zj = Z + 16 * bj * ZS;
                    vec c;
#pragma unroll
                    for (int r = 0; r < 4; r++) c[r] = Zj[Acc::row_of(lane, r) * ZS + col];
#pragma unroll
                    for (int s = 0; s < 4; s++) c = Acc::mma(-Rjk[col * LD + 4 * s + grp], Zk[(4 * s + grp) * ZS + col], c);
#pragma unroll
                    for (int r = 0; r < 4; r++) Zj[Acc::row_of(lane, r) * ZS + col] = c[r];
                }
                __syncthreads();
            }

            // ---- 4: the history against Z
            const int tsum = wave + TOPNX_NW * (lane & 3);          // lanes 0..3: the target whose total this lane adds up
            double tot = 0;
            T thr[4] = {NEG, NEG, NEG, NEG};                        // the n_top-th best of target wave + 4 q so far
            for (int s0 = 0; s0 < hlen; s0 += SR) {
                const int nh = min(SR, hlen - s0);
                if (tid < SR) {
                    const bool in = tid < nh;
                    rowid[tid] = in ? P.hist_i[hbeg + s0 + tid] : -1;
                    sy[tid] = in ? P.hist_y[hbeg + s0 + tid] : T(0);
                }
                __syncthreads();
                gather(SR, false);
                __syncthreads();
                if (16 * wave < SR) {                               // wave-uniform
                    vec c = vec{0, 0, 0, 0};
                    const T *ap = slab + (16 * wave + col) * KS + grp, *zp = Z + grp * ZS + col;
                    for (int s = 0; s < KW / 4; s++) c = Acc::mma(ap[4 * s], zp[4 * s * ZS], c);
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int i = 16 * wave + Acc::row_of(lane, r);
                        pbuf[i * PS + col] = sy[i] * c[r];
                    }
                }
                __syncthreads();
                if (lane < 4 && tsum < nt)
                    for (int h = 0; h < nh; h++) tot += (double)pbuf[h * PS + tsum];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int t = wave + TOPNX_NW * q;
                    if (t < nt) {                                   // wave-uniform
                        const T v = lane < nh ? pbuf[min(lane, SR - 1) * PS + t] : NEG;
                        const bool offer = lane < nh && v >= thr[q];
                        if (__ballot(offer) != 0) {
                            csc[lane] = offer ? v : NEG;
                            cid[lane] = offer ? s0 + lane : NONE;
                            topnc_lds_sync();
                            thr[q] = topnc_merge(lsc + t * NP, lid + t * NP, csc, cid, NP, ntop, nh, lane);
                        }
                    }
                }
            }
            // ---- 5
            topnc_lds_sync();
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int t = wave + TOPNX_NW * q;
                if (t < nt) {
                    const size_t o = (t0 + t) * (size_t)ntop;
                    for (int j = lane; j < ntop; j += 64) {
                        const T s = lsc[t * NP + j];
                        const int pos = lid[t * NP + j];
                        const bool pad = bad || s == NEG;
                        P.out_ids[o + j] = pad ? -1 : P.hist_i[hbeg + pos];
                        P.out_contrib[o + j] = bad ? T(NAN) : s;
                    }
                }
            }
            if (lane < 4 && tsum < nt) P.out_total[t0 + tsum] = bad ? T(NAN) : (T)tot;
            __syncthreads();                                        // the next tile of targets writes Z and the lists
        }
    }
}

// topn_explain_kernel over P.nu users on st (instantiated in topn_explain_tu.hip): a persistent grid of as many workgroups as
// the device holds at this shape's LDS size, at most one per user, at most max_groups where that is > 0
// (CMFREC_HIP_EXPLAIN_GROUPS); returns the grid
int topn_explain_launch(hipStream_t st, int num_cus, const TopnExplainParams<real_t> &P, int max_groups);

}  // namespace cmfhip
