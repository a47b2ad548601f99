// objective_kernels.hpp -- the components of the training objective of the factors as they are on the device
// (cmfrec_hip_session_objective: objective_tu.hip).
//
//   objective_items_kernel   one workgroup: the first work item of every row of X's CSR, from indptr
//   objective_rows_kernel    one pass over the CSR: the data term over the stored entries and the penalty sums of A, B and the biases
//   gram_f64acc_kernel       slab partials of M^T M on the shared columns, accumulated in double on v_mfma_f64_16x16x4
//   gram_inner_kernel        <A^T A, B^T B> tile pair by tile pair, from the two sets of slab partials
//   objective_reduce_kernel  one workgroup: the wavefronts' records and the tile pairs' products, in index order
//
// Work items of objective_rows_kernel.  A row of X with l entries is cut into max(1, ceil(l / seg)) items of seg entries (seg =
// OBJ_SEGMENT, or the test hook's); a row without entries keeps one, so that its norms are counted.  item_off[r] is the first item of
// row r (objective_items_kernel), item_off[m] their number.  Behind them come ceil(n / (64 / G)) items that hold 64 / G rows of B
// each and read no entry of X: B's penalty sums need its rows and the column orientation's indptr alone.  A wavefront takes the items
// wave, wave + nwaves, ...; it finds an item's row by bisection over item_off (wavefront-uniform, scalar loads).
//
// Lanes.  A row of kk = k + k_main elements is cut into 16-byte pieces of Ve elements; a group of G lanes, G the power of two that
// covers the pieces up to 64, holds a row with C pieces per lane (C > 1 beyond 64 pieces: kk <= 272 needs 2 in single, 3 in double
// precision).  Every one of the 64 / G groups of a wavefront keeps a copy of the owning row a_i in registers; group q takes the
// entries q, q + 64 / G, ... of the item, two steps in flight: the index, value and weight loads of both, then their 2 C gathers of
// 16 bytes per lane, then the arithmetic.  The partial dot products are fused multiply-adds in element order in the working
// precision, summed over the group by the xor butterfly of predict_kernels.hpp (DPP inside 16-lane rows, permlane swaps across
// them).  The residual is formed in the working precision (single: exactly in double, rounded once), its square and every sum in
// double, in the registers of lane 0 of the group.  The wavefront that holds a row's first item adds the row's penalty sums: every
// lane of group 0 the squares of its own pieces, lane 0 the columns in front of the shared ones, the last column and the bias.
//
// After its last item a wavefront folds the 64 lanes' sums (lanes::wave_fold: the same bits in every lane) and lane 0 writes one
// record of OBJ_FIELDS values; every wavefront of the launch writes one.  objective_reduce_kernel adds the records in an order that
// is a function of the wavefront index alone.  No atomics, no LDS in the row kernel: the same call on the same device returns the
// same bytes.
#pragma once
#include "../../include/cmfrec_hip.h"
#include "predict_kernels.hpp"

namespace cmfhip {

constexpr int OBJ_TH = 256;            // threads per workgroup of the row kernel
constexpr int OBJ_SEGMENT = 2048;      // entries per work item of a long row
constexpr int OBJ_ITEMS_TH = 1024;     // objective_items_kernel: one workgroup
constexpr int OBJ_REDUCE_TH = 256;
// a record: n (a 64-bit count), sum_w, data, then {sq, scaled sq, last-column sq, scaled last-column sq} of A, {sq, scaled sq} of
// biasA, the same six of B / biasB -- the leading fields of cmfrec_hip_objective, whose last one is allpairs
constexpr int OBJ_FIELDS = 15;
static_assert(sizeof(cmfrec_hip_objective) == (OBJ_FIELDS + 1) * 8, "cmfrec_hip_objective has padding");

// one side of the model: its matrix, its bias, the indptr of X by its rows and lambda's per-row multipliers
template <typename T>
struct ObjSide {
    const T *F = nullptr; size_t ld = 0;   // [rows, ld]
    int rows = 0, k_side = 0;              // k_side columns (k_user / k_item) in front of the shared ones
    const T *bias = nullptr;               // [rows] or null
    const size_t *p = nullptr;             // [rows + 1]
    const T *wsum = nullptr;               // [rows]: the rows' weight sums (1 for an empty row), or null: the entry counts
};

template <typename T>
struct ObjParams {
    ObjSide<T> a, b;
    int kk = 0;
    const int *idx = nullptr;              // CSR of X by the rows of a: opposing index, value, weight (or null)
    const T *v = nullptr, *w = nullptr;
    const unsigned long long *item_off = nullptr;   // [a.rows + 1]
    int seg = OBJ_SEGMENT;
    double *records = nullptr;             // [wavefronts of the launch][OBJ_FIELDS]
};

__host__ __device__ inline unsigned long long obj_row_items(size_t len, int seg)
{
    return len ? (unsigned long long)((len + (size_t)seg - 1) / (size_t)seg) : 1ull;
}

// item_off[r] = sum over the rows before r of their items, item_off[rows] = all of them.  Thread t owns a contiguous run of rows; the
// runs' totals are scanned through LDS.
__global__ __launch_bounds__(OBJ_ITEMS_TH) void objective_items_kernel(const size_t *p, int rows, int seg, unsigned long long *item_off)
{
    __shared__ unsigned long long tot[OBJ_ITEMS_TH];
    const int t = threadIdx.x;
    const long long per = ((long long)rows + OBJ_ITEMS_TH - 1) / OBJ_ITEMS_TH;
    const long long r0 = std::min<long long>((long long)t * per, rows), r1 = std::min<long long>(r0 + per, rows);
    unsigned long long mine = 0;
    for (long long r = r0; r < r1; r++) mine += obj_row_items(p[r + 1] - p[r], seg);
    tot[t] = mine;
    __syncthreads();
    for (int d = 1; d < OBJ_ITEMS_TH; d <<= 1) {
        const unsigned long long below = t >= d ? tot[t - d] : 0ull;
        __syncthreads();
        tot[t] += below;
        __syncthreads();
    }
    unsigned long long at = tot[t] - mine;
    for (long long r = r0; r < r1; r++) {
        item_off[r] = at;
        at += obj_row_items(p[r + 1] - p[r], seg);
    }
    if (t == OBJ_ITEMS_TH - 1) item_off[rows] = tot[t];
}

// the C pieces of the row at `row` (its first shared column) that lane g of a group holds; elements past kk are zeros
template <typename T, int G, int C, bool VEC>
__device__ __forceinline__ void obj_load_row(const T *row, int g, int kk, bool live, T (&x)[C][16 / sizeof(T)])
{
    constexpr int Ve = 16 / (int)sizeof(T);
#pragma unroll
    for (int c = 0; c < C; c++) {
        const int e0 = (c * G + g) * Ve;
        if (live && e0 < kk) {
            score_load_piece<T, VEC>(row, e0, kk, x[c]);
#pragma unroll
            for (int e = 0; e < Ve; e++) x[c][e] = (e0 + e < kk) ? x[c][e] : (T)0;
        } else {
#pragma unroll
            for (int e = 0; e < Ve; e++) x[c][e] = (T)0;
        }
    }
}

// the penalty sums of one row, in the lanes of the group that holds it (x: the lane's pieces of the shared columns)
struct ObjNorms {
    double sq = 0, sq_s = 0, last = 0, last_s = 0, bsq = 0, bsq_s = 0;
};
template <typename T, int C>
__device__ __forceinline__ void obj_add_norms(ObjNorms &N, const ObjSide<T> &S, int r, int g, int kk, const T (&x)[C][16 / sizeof(T)])
{
    constexpr int Ve = 16 / (int)sizeof(T);
    const size_t len = S.p[r + 1] - S.p[r];
    const double mult = S.wsum ? (double)S.wsum[r] : (len ? (double)len : 1.);
    double sq = 0;
#pragma unroll
    for (int c = 0; c < C; c++)
#pragma unroll
        for (int e = 0; e < Ve; e++) sq += (double)x[c][e] * (double)x[c][e];
    if (g == 0) {
        const T *row = S.F + (size_t)r * S.ld;
        for (int q = 0; q < S.k_side; q++) sq += (double)row[q] * (double)row[q];
        const double l = (double)row[S.k_side + kk - 1], b = S.bias ? (double)S.bias[r] : 0.;
        N.last += l * l; N.last_s += mult * (l * l);
        N.bsq += b * b; N.bsq_s += mult * (b * b);
    }
    N.sq += sq; N.sq_s += mult * sq;
}

template <typename T, bool IMPLICIT, int G, int C, bool VEC>
__global__ __launch_bounds__(OBJ_TH) void objective_rows_kernel(const ObjParams<T> P)
{
    constexpr int Ve = 16 / (int)sizeof(T), PS = 64 / G;
    const int lane = threadIdx.x & 63, g = lane & (G - 1), sub = lane / G;
    const unsigned long long wave = (unsigned long long)blockIdx.x * (OBJ_TH / 64) +
                                    (unsigned long long)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned long long nwaves = (unsigned long long)gridDim.x * (OBJ_TH / 64);
    const int kk = P.kk, m = P.a.rows, n = P.b.rows;
    const unsigned long long items_a = P.item_off[m], items_b = (unsigned long long)((n + PS - 1) / PS);
    unsigned long long cnt = 0;
    double sum_w = 0, data = 0;
    ObjNorms NA, NB;
    // (the items, the rows they belong to and the trip counts below are wavefront-uniform: all 64 lanes reach every butterfly)
    for (unsigned long long t = wave; t < items_a + items_b; t += nwaves) {
        if (t >= items_a) {
            const long long r = (long long)(t - items_a) * PS + sub;
            const bool live = r < (long long)n;
            T b[C][Ve];
            obj_load_row<T, G, C, VEC>(P.b.F + (size_t)(live ? r : 0) * P.b.ld + P.b.k_side, g, kk, live, b);
            if (live) obj_add_norms<T, C>(NB, P.b, (int)r, g, kk, b);
            continue;
        }
        int lo = 0, hi = m;                                   // item_off[lo] <= t < item_off[hi]
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (P.item_off[mid] <= t) lo = mid; else hi = mid;
        }
        const int i = lo;
        const unsigned long long s = t - P.item_off[i];
        const size_t row_end = P.a.p[i + 1], first = P.a.p[i] + (size_t)s * (size_t)P.seg;
        const size_t last = std::min(row_end, first + (size_t)P.seg);
        T a[C][Ve];
        obj_load_row<T, G, C, VEC>(P.a.F + (size_t)i * P.a.ld + P.a.k_side, g, kk, true, a);
        if (s == 0 && sub == 0) obj_add_norms<T, C>(NA, P.a, i, g, kk, a);
        const T bias_a = (!IMPLICIT && P.a.bias) ? P.a.bias[i] : (T)0;
        for (size_t e = first; e < last; e += 2 * PS) {
            size_t q[2];
            bool live[2];
            int j[2];
            T x[2], w[2], bias_b[2], b[2][C][Ve], dot[2];
#pragma unroll
            for (int u = 0; u < 2; u++) {
                q[u] = e + (size_t)(u * PS + sub);
                live[u] = q[u] < last;
                j[u] = live[u] ? P.idx[q[u]] : 0;
                x[u] = live[u] ? P.v[q[u]] : (T)0;
                w[u] = (live[u] && !IMPLICIT && P.w) ? P.w[q[u]] : (T)1;
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                obj_load_row<T, G, C, VEC>(P.b.F + (size_t)j[u] * P.b.ld + P.b.k_side, g, kk, live[u], b[u]);
                bias_b[u] = (live[u] && g == 0 && !IMPLICIT && P.b.bias) ? P.b.bias[j[u]] : (T)0;
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                T acc = (T)0;
#pragma unroll
                for (int c = 0; c < C; c++)
#pragma unroll
                    for (int ee = 0; ee < Ve; ee++) acc = fma(a[c][ee], b[u][c][ee], acc);
                dot[u] = score_group_sum<G>(acc);
            }
#pragma unroll
            for (int u = 0; u < 2; u++) {
                if (!(live[u] && g == 0)) continue;
                cnt++;
                if constexpr (IMPLICIT) {
                    const T r = (T)1 - dot[u];
                    const double rd = (double)r, sd = (double)dot[u];
                    sum_w += 1.;
                    data += (1. + (double)x[u]) * (rd * rd) - sd * sd;
                } else {
                    T r;
                    if constexpr (sizeof(T) == 4) r = (T)((((double)x[u] - (double)bias_a) - (double)bias_b[u]) - (double)dot[u]);
                    else r = ((x[u] - bias_a) - bias_b[u]) - dot[u];
                    const double rd = (double)r, wd = (double)w[u];
                    sum_w += wd;
                    data += wd * (rd * rd);
                }
            }
        }
    }
    auto add = [](double p, double q) { return p + q; };
    double rec[OBJ_FIELDS];
    rec[0] = __longlong_as_double((long long)lanes::wave_sum_u64(cnt));
    rec[1] = lanes::wave_fold(sum_w, add); rec[2] = lanes::wave_fold(data, add);
    const ObjNorms *NN[2] = {&NA, &NB};
#pragma unroll
    for (int side = 0; side < 2; side++) {
        rec[3 + 6 * side] = lanes::wave_fold(NN[side]->sq, add); rec[4 + 6 * side] = lanes::wave_fold(NN[side]->sq_s, add);
        rec[5 + 6 * side] = lanes::wave_fold(NN[side]->last, add); rec[6 + 6 * side] = lanes::wave_fold(NN[side]->last_s, add);
        rec[7 + 6 * side] = lanes::wave_fold(NN[side]->bsq, add); rec[8 + 6 * side] = lanes::wave_fold(NN[side]->bsq_s, add);
    }
    if (lane == 0)
#pragma unroll
        for (int f = 0; f < OBJ_FIELDS; f++) P.records[wave * OBJ_FIELDS + f] = rec[f];
}

// ---- <A^T A, B^T B> in double ----------------------------------------------------------------------------------------------------
// gram_f64acc_kernel: workgroup (x, y) owns the slab x of `slab` rows (a multiple of 4) and the tile row y of M^T M; its four
// wavefronts take the 16 x 16 tiles (y, J), J = y + wave, y + wave + 4, ... of the upper triangle.  One v_mfma_f64_16x16x4 consumes
// four rows: lane l converts M[r + (l >> 4)][16 y + (l & 15)] and M[r + (l >> 4)][16 J + (l & 15)] to double (zeros past the rows
// of the slab and past kk), so a product of two single-precision values is exact and only the accumulation rounds.  The tile goes
// out as the accumulator's four registers, lane-linear: part[(x * pairs + pair(y, J)) * 256 + 64 reg + lane] -- the same element
// of the tile at the same place for A and for B, which is all the inner product needs.
constexpr int GRAM64_TH = 256;
__host__ __device__ inline int gram64_tiles(int kk) { return (kk + 15) / 16; }
__host__ __device__ inline int gram64_pair(int nt, int I, int J) { return I * nt - I * (I - 1) / 2 + (J - I); }
__host__ __device__ inline int gram64_pairs(int nt) { return nt * (nt + 1) / 2; }

template <typename T>
__global__ __launch_bounds__(GRAM64_TH) void gram_f64acc_kernel(const T *M, size_t ld, int rows, int kk, int slab, double *part)
{
    typedef double vec4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int nt = gram64_tiles(kk), I = blockIdx.y;
    const long long r0 = (long long)blockIdx.x * slab, r1 = std::min<long long>(rows, r0 + slab);
    const int ci = I * 16 + (lane & 15);
    for (int J = I + wv; J < nt; J += GRAM64_TH / 64) {
        const int cj = J * 16 + (lane & 15);
        vec4 acc = {0., 0., 0., 0.};
#pragma unroll 4
        for (long long rb = r0; rb < r1; rb += 4) {
            const long long r = rb + (lane >> 4);
            const bool in = r < r1;
            const double x = (in && ci < kk) ? (double)M[(size_t)r * ld + ci] : 0.;
            const double y = (in && cj < kk) ? (double)M[(size_t)r * ld + cj] : 0.;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(x, y, acc, 0, 0, 0);
        }
        double *out = part + ((size_t)blockIdx.x * gram64_pairs(nt) + gram64_pair(nt, I, J)) * 256;
#pragma unroll
        for (int reg = 0; reg < 4; reg++) out[reg * 64 + lane] = acc[reg];
    }
}

// workgroup = tile pair: thread e adds the slabs' partials of its element in slab order for both matrices and multiplies; a tile off
// the diagonal stands for its mirror image too.  The 256 products are added by thread 0 in element order: pair_dot[pair].
__global__ __launch_bounds__(256) void gram_inner_kernel(const double *part_a, int slabs_a, const double *part_b, int slabs_b, int nt,
                                                         double *pair_dot)
{
    __shared__ double prod[256];
    const int pair = blockIdx.x, pairs = gram64_pairs(nt), e = threadIdx.x;
    int I = 0, rest = pair;
    while (rest >= nt - I) { rest -= nt - I; I++; }
    double ga = 0, gb = 0;
    for (int s = 0; s < slabs_a; s++) ga += part_a[((size_t)s * pairs + pair) * 256 + e];
    for (int s = 0; s < slabs_b; s++) gb += part_b[((size_t)s * pairs + pair) * 256 + e];
    prod[e] = (rest == 0 ? 1. : 2.) * (ga * gb);
    __syncthreads();
    if (e == 0) {
        double tot = 0;
        for (int q = 0; q < 256; q++) tot += prod[q];
        pair_dot[pair] = tot;
    }
}

// records[0 .. nrec) and pair_dot[0 .. npairs) -> out[OBJ_FIELDS + 1]: thread t takes the records t, t + 256, ... in ascending order,
// then one thread per field the 256 results in ascending order; field 0 is a count and travels as its 64 bits.  One more thread
// adds the tile pairs' products in index order (npairs = 0: the explicit model, allpairs = 0).
__global__ __launch_bounds__(OBJ_REDUCE_TH) void objective_reduce_kernel(const double *records, size_t nrec, const double *pair_dot,
                                                                         int npairs, double *out)
{
    __shared__ double part[OBJ_FIELDS][OBJ_REDUCE_TH];
    auto combine = [](int f, double p, double q) {
        if (f > 0) return p + q;
        return __longlong_as_double((long long)((unsigned long long)__double_as_longlong(p) + (unsigned long long)__double_as_longlong(q)));
    };
    const int t = threadIdx.x;
    double acc[OBJ_FIELDS];
#pragma unroll
    for (int f = 0; f < OBJ_FIELDS; f++) acc[f] = 0.;          // (the bits of a zero count too)
    for (size_t r = (size_t)t; r < nrec; r += OBJ_REDUCE_TH)
#pragma unroll
        for (int f = 0; f < OBJ_FIELDS; f++) acc[f] = combine(f, acc[f], records[r * OBJ_FIELDS + f]);
#pragma unroll
    for (int f = 0; f < OBJ_FIELDS; f++) part[f][t] = acc[f];
    __syncthreads();
    if (t < OBJ_FIELDS) {
        double v = 0.;
        for (int s = 0; s < OBJ_REDUCE_TH; s++) v = combine(t, v, part[t][s]);
        out[t] = v;
    } else if (t == OBJ_FIELDS) {
        double v = 0.;
        for (int q = 0; q < npairs; q++) v += pair_dot[q];
        out[OBJ_FIELDS] = v;
    }
}

}  // namespace cmfhip
