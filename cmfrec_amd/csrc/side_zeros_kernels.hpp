// side_zeros_kernels.hpp -- the two products of sparse side information whose ABSENT ENTRIES ARE ZEROS (NA_as_zero_U / _I),
// taken on the triplets instead of on the zero-filled dense matrix.
//
// The session multiplies by dense side information in two forms only (session.hip, side_times / side_transposed_times):
//     U M    M [p, kc]       right-hand sides w U C, the U C of the block CG, the rotated w U C Q of the low-rank rows
//     U^T F  F [rows, ldF]   the C / D update
// With U~ = U_sparse - 1 mu^T (mu: column sums over ALL rows divided by the rows) both have a sparse form,
//     U~ M    = SpMM(U_csr, M)    - 1 (mu^T M)      one kc-vector per call  (sz_colsum: weights mu, matrix M)
//     U~^T F  = SpMM^T(U_csc, F)  - mu (1^T F)      one kc-vector per call  (sz_colsum: no weights, matrix F)
// so the work is nnz x kc instead of rows x p x kc and no rows x p matrix exists anywhere.
//
// Mapping (both products): lanes run along kc, so the gather of one row of M / F is one contiguous read per entry.  A group of
// 16 / 32 / 64 lanes owns one item -- four / two rows per wavefront for kc <= 16 / 32, one wavefront per row beyond, each lane
// holding up to five accumulators (kc <= 320) -- and walks the item's entries in order, four gathers in flight.
//   row side:        item = one row of U;  out[r - first, :] = alpha (sum_e u_e M[col_e, :] - c)
//   attribute side:  item = one SEGMENT of an attribute's column.  Most attributes have a few entries, some (a flag nearly every
//                    row carries) have as many as there are rows: a column is cut into segments of
//                        SZ_UNIT = 512 entries
//                    A column of one segment is finished by its own group (out[a, :] = sum - mu_a s); the segments of a longer
//                    column store partial sums, and sz_cols_finish_kernel adds a column's partials in segment order.
// No floating-point atomics anywhere, every sum has a fixed order: the same call returns the same bits.  Duplicated positions
// add up (the triplets are not merged); an item without entries yields its correction term alone.  No LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <vector>

#include "device.hpp"

namespace cmfhip {

constexpr int SZ_UNIT = 512;             // entries per segment of an attribute's column
constexpr int SZ_MAX_WIDTH = 320;        // widest kc: five accumulators per lane
constexpr int SZ_COLSUM_SEGS = 4096;     // at most this many row segments in a column-sum (sz_colsum): four wavefronts per SIMD

struct SzSeg {                           // one work item of the attribute side
    unsigned long long beg;              // first entry (offset into the column-major shard)
    int len;                             // entries, <= SZ_UNIT
    int col;                             // the attribute
    int slot;                            // < 0: the column's only segment, finished in place; else the row of `partial` it fills
    int pad_;
};
struct SzLong {                          // an attribute of several segments: partial rows [first, first + nparts)
    int col, first, nparts;
};

// acc[c] += sum over the entries e in [beg, end), in order, of val[e] * Mat[idx[e], j + c * LANES]
template <typename T, int LANES, int NJ>
__device__ __forceinline__ void sz_gather(const int *__restrict__ idx, const T *__restrict__ val, size_t beg, size_t end,
                                          const T *__restrict__ Mat, size_t ld, int j, int width, T (&acc)[NJ])
{
    size_t e = beg;
    for (; e + 4 <= end; e += 4) {
        const int i0 = idx[e], i1 = idx[e + 1], i2 = idx[e + 2], i3 = idx[e + 3];
        const T u0 = val[e], u1 = val[e + 1], u2 = val[e + 2], u3 = val[e + 3];
        T g0[NJ], g1[NJ], g2[NJ], g3[NJ];
#pragma unroll
        for (int c = 0; c < NJ; c++) {
            const int jj = j + c * LANES;
            const bool in = jj < width;
            g0[c] = in ? Mat[(size_t)i0 * ld + jj] : (T)0;
            g1[c] = in ? Mat[(size_t)i1 * ld + jj] : (T)0;
            g2[c] = in ? Mat[(size_t)i2 * ld + jj] : (T)0;
            g3[c] = in ? Mat[(size_t)i3 * ld + jj] : (T)0;
        }
#pragma unroll
        for (int c = 0; c < NJ; c++) {
            acc[c] = fma(u0, g0[c], acc[c]);
            acc[c] = fma(u1, g1[c], acc[c]);
            acc[c] = fma(u2, g2[c], acc[c]);
            acc[c] = fma(u3, g3[c], acc[c]);
        }
    }
    for (; e < end; e++) {
        const int i0 = idx[e];
        const T u0 = val[e];
#pragma unroll
        for (int c = 0; c < NJ; c++) {
            const int jj = j + c * LANES;
            if (jj < width) acc[c] = fma(u0, Mat[(size_t)i0 * ld + jj], acc[c]);
        }
    }
}

// Row side.  indptr / idx / val: the row-major shard; cvec: mu^T M [kc] or null (no column means); rows [first, first + count).
template <typename T, int LANES, int NJ>
__global__ void __launch_bounds__(256) sz_rows_kernel(const size_t *__restrict__ indptr, const int *__restrict__ idx,
                                                      const T *__restrict__ val, const T *__restrict__ M, size_t ldm, int kc,
                                                      const T *__restrict__ cvec, T alpha, int first, int count,
                                                      T *__restrict__ out, size_t ldo)
{
    constexpr int GROUPS = 256 / LANES;
    const int j = threadIdx.x % LANES;
    const long long item = (long long)blockIdx.x * GROUPS + threadIdx.x / LANES;
    if (item >= count) return;
    const size_t r = (size_t)first + (size_t)item;
    T acc[NJ];
#pragma unroll
    for (int c = 0; c < NJ; c++) acc[c] = (T)0;
    sz_gather<T, LANES, NJ>(idx, val, indptr[r], indptr[r + 1], M, ldm, j, kc, acc);
#pragma unroll
    for (int c = 0; c < NJ; c++) {
        const int jj = j + c * LANES;
        if (jj < kc) out[(size_t)item * ldo + jj] = alpha * (acc[c] - (cvec != nullptr ? cvec[jj] : (T)0));
    }
}

// Attribute side, first pass.  idx / val: the column-major shard (idx = rows of F); svec: 1^T F [kc] (read with mu only).
template <typename T, int LANES, int NJ>
__global__ void __launch_bounds__(256) sz_cols_kernel(const SzSeg *__restrict__ segs, int nseg, const int *__restrict__ idx,
                                                      const T *__restrict__ val, const T *__restrict__ F, size_t ldf, int kc,
                                                      const T *__restrict__ mu, const T *__restrict__ svec, T *__restrict__ out,
                                                      size_t ldo, T *__restrict__ partial)
{
    constexpr int GROUPS = 256 / LANES;
    const int j = threadIdx.x % LANES;
    const long long item = (long long)blockIdx.x * GROUPS + threadIdx.x / LANES;
    if (item >= nseg) return;
    const SzSeg sg = segs[item];
    T acc[NJ];
#pragma unroll
    for (int c = 0; c < NJ; c++) acc[c] = (T)0;
    sz_gather<T, LANES, NJ>(idx, val, (size_t)sg.beg, (size_t)sg.beg + (size_t)sg.len, F, ldf, j, kc, acc);
    const T m = (sg.slot < 0 && mu != nullptr) ? mu[sg.col] : (T)0;
#pragma unroll
    for (int c = 0; c < NJ; c++) {
        const int jj = j + c * LANES;
        if (jj >= kc) continue;
        if (sg.slot < 0) out[(size_t)sg.col * ldo + jj] = acc[c] - (mu != nullptr ? m * svec[jj] : (T)0);
        else partial[(size_t)sg.slot * kc + jj] = acc[c];
    }
}

// ... second pass: the attributes of several segments, partials added in segment order
template <typename T>
__global__ void __launch_bounds__(256) sz_cols_finish_kernel(const SzLong *__restrict__ longs, int nlong, const T *__restrict__ partial,
                                                             int kc, const T *__restrict__ mu, const T *__restrict__ svec,
                                                             T *__restrict__ out, size_t ldo)
{
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)nlong * kc) return;
    const SzLong L = longs[t / kc];
    const int j = (int)(t % kc);
    T acc = (T)0;
    for (int q = 0; q < L.nparts; q++) acc += partial[(size_t)(L.first + q) * kc + j];
    out[(size_t)L.col * ldo + j] = acc - (mu != nullptr ? mu[L.col] * svec[j] : (T)0);
}

// Column sums  out[j] = sum_r wgt[r] X[r, j]  (wgt null: ones), in two passes of fixed order: one wavefront per (segment of
// seg_rows rows, 64 columns) on four interleaved chains, then one thread per column over the segments.
template <typename T>
__global__ void __launch_bounds__(256) sz_colsum_partial_kernel(const T *__restrict__ X, size_t ld, int rows, int width,
                                                                const T *__restrict__ wgt, int seg_rows, int nseg, T *__restrict__ part)
{
    const int seg = blockIdx.x * 4 + (threadIdx.x >> 6), j = blockIdx.y * 64 + (threadIdx.x & 63);
    if (seg >= nseg || j >= width) return;
    const int r0 = seg * seg_rows, r1 = min(rows, r0 + seg_rows);
    T a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    int r = r0;
    for (; r + 4 <= r1; r += 4) {
        const T x0 = X[(size_t)r * ld + j], x1 = X[(size_t)(r + 1) * ld + j], x2 = X[(size_t)(r + 2) * ld + j], x3 = X[(size_t)(r + 3) * ld + j];
        if (wgt != nullptr) {
            a0 = fma(wgt[r], x0, a0); a1 = fma(wgt[r + 1], x1, a1); a2 = fma(wgt[r + 2], x2, a2); a3 = fma(wgt[r + 3], x3, a3);
        } else {
            a0 += x0; a1 += x1; a2 += x2; a3 += x3;
        }
    }
    for (; r < r1; r++) a0 = wgt != nullptr ? fma(wgt[r], X[(size_t)r * ld + j], a0) : a0 + X[(size_t)r * ld + j];
    part[(size_t)seg * width + j] = (a0 + a1) + (a2 + a3);
}

template <typename T>
__global__ void __launch_bounds__(256) sz_colsum_finish_kernel(const T *__restrict__ part, int nseg, int width, T *__restrict__ out)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= width) return;
    T acc = (T)0;
    for (int q = 0; q < nseg; q++) acc += part[(size_t)q * width + j];
    out[j] = acc;
}

// ---- host side ----------------------------------------------------------------------------
// One side's sparse-as-zeros operand: the two orientations (owned by the caller), the column means and the work buffers.
struct SideZeros {
    const SparseShard *csr = nullptr, *csc = nullptr;     // by row [rows] / by attribute [p]
    int rows = 0, p = 0;
    bool has_mu = false;
    DevBuf<real_t> mu;                                    // [p]
    DevBuf<SzSeg> segs;
    DevBuf<SzLong> longs;
    int nseg = 0, nlong = 0, npart = 0;
    DevBuf<real_t> vec, colsum_part, col_part;            // mu^T M / 1^T F; partials of sz_colsum; partials of the long columns
    bool on() const { return csr != nullptr; }
    void clear() { csr = csc = nullptr; rows = p = 0; has_mu = false; nseg = nlong = npart = 0; }

    // after both shards are built: the attribute side's segment table from the column-major row pointers
    void build(const SparseShard *by_row, const SparseShard *by_col, const real_t *colmeans, hipStream_t st)
    {
        csr = by_row; csc = by_col; rows = by_row->nrows; p = by_col->nrows;
        has_mu = colmeans != nullptr;
        if (has_mu) mu.upload(colmeans, (size_t)p, st);
        std::vector<size_t> hp((size_t)p + 1);
        by_col->p.download(hp.data(), (size_t)p + 1, st);
        HIP_CHECK(hipStreamSynchronize(st));
        std::vector<SzSeg> hs; std::vector<SzLong> hl;
        hs.reserve((size_t)p + by_col->nnz / SZ_UNIT);
        npart = 0;
        for (int a = 0; a < p; a++) {
            const size_t len = hp[(size_t)a + 1] - hp[a];
            if (len <= (size_t)SZ_UNIT) { hs.push_back(SzSeg{(unsigned long long)hp[a], (int)len, a, -1, 0}); continue; }
            const int parts = (int)((len + SZ_UNIT - 1) / SZ_UNIT);
            hl.push_back(SzLong{a, npart, parts});
            for (int q = 0; q < parts; q++) {
                const size_t b = hp[a] + (size_t)q * SZ_UNIT;
                hs.push_back(SzSeg{(unsigned long long)b, (int)std::min<size_t>(SZ_UNIT, hp[(size_t)a + 1] - b), a, npart + q, 0});
            }
            npart += parts;
        }
        nseg = (int)hs.size(); nlong = (int)hl.size();
        segs.upload(hs.data(), hs.size(), st);
        if (nlong) longs.upload(hl.data(), hl.size(), st);
        HIP_CHECK(hipStreamSynchronize(st));               // (the host vectors go out of scope)
    }
};

// out[j] = sum_r wgt[r] X[r, j], j < width
inline void sz_colsum(const DeviceInfo &dev, SideZeros &Z, const real_t *X, size_t ld, int rows, int width, const real_t *wgt, real_t *out)
{
    const int seg_rows = std::max(64, (rows + SZ_COLSUM_SEGS - 1) / SZ_COLSUM_SEGS);
    const int nseg = std::max(1, (rows + seg_rows - 1) / seg_rows);
    Z.colsum_part.alloc_at_least((size_t)nseg * width);
    hipLaunchKernelGGL(sz_colsum_partial_kernel<real_t>, dim3((nseg + 3) / 4, (width + 63) / 64), dim3(256), 0, dev.stream, X, ld, rows, width,
                       wgt, seg_rows, nseg, Z.colsum_part.ptr);
    hipLaunchKernelGGL(sz_colsum_finish_kernel<real_t>, dim3((width + 255) / 256), dim3(256), 0, dev.stream, Z.colsum_part.ptr, nseg, width, out);
    HIP_CHECK(hipGetLastError());
}

// launches kern<real_t, LANES, NJ> for the width: GROUPS items per workgroup of 256 threads
#define SZ_DISPATCH(kern, width, items, ...)                                                                                          \
    do {                                                                                                                              \
        const long long it_ = (items);                                                                                                \
        auto go_ = [&](auto k_, int lanes_) {                                                                                         \
            const int groups_ = 256 / lanes_;                                                                                         \
            hipLaunchKernelGGL(k_, dim3((unsigned)((it_ + groups_ - 1) / groups_)), dim3(256), 0, dev.stream, __VA_ARGS__);           \
        };                                                                                                                            \
        if ((width) <= 16) go_(kern<real_t, 16, 1>, 16);                                                                              \
        else if ((width) <= 32) go_(kern<real_t, 32, 1>, 32);                                                                         \
        else if ((width) <= 64) go_(kern<real_t, 64, 1>, 64);                                                                         \
        else if ((width) <= 128) go_(kern<real_t, 64, 2>, 64);                                                                        \
        else if ((width) <= 192) go_(kern<real_t, 64, 3>, 64);                                                                        \
        else if ((width) <= 256) go_(kern<real_t, 64, 4>, 64);                                                                        \
        else go_(kern<real_t, 64, 5>, 64);                                                                                            \
    } while (0)

// out[r - first, :kc] = alpha (U~ M)[r, :],  r in [first, first + count);  M [p, kc] with leading dimension ldm
inline void sz_times(const DeviceInfo &dev, SideZeros &Z, int first, int count, int kc, real_t alpha, const real_t *M, size_t ldm,
                     real_t *out, size_t ldo)
{
    if (count <= 0 || kc <= 0) return;
    const real_t *cvec = nullptr;
    if (Z.has_mu) {
        Z.vec.alloc_at_least((size_t)kc);
        sz_colsum(dev, Z, M, ldm, Z.p, kc, Z.mu.ptr, Z.vec.ptr);
        cvec = Z.vec.ptr;
    }
    const SparseShard &S = *Z.csr;
    SZ_DISPATCH(sz_rows_kernel, kc, count, S.p.ptr, S.i.ptr, S.v.ptr, M, ldm, kc, cvec, alpha, first, count, out, ldo);
    HIP_CHECK(hipGetLastError());
}

// out[a, :kc] = (U~^T F)[a, :] over the first `rows_f` rows of F (the rows of U);  a < p
inline void sz_transposed_times(const DeviceInfo &dev, SideZeros &Z, int kc, const real_t *F, size_t ldf, real_t *out, size_t ldo)
{
    if (Z.p <= 0 || kc <= 0) return;
    const real_t *svec = nullptr;
    if (Z.has_mu) {
        Z.vec.alloc_at_least((size_t)kc);
        sz_colsum(dev, Z, F, ldf, Z.rows, kc, nullptr, Z.vec.ptr);
        svec = Z.vec.ptr;
    }
    if (Z.npart) Z.col_part.alloc_at_least((size_t)Z.npart * kc);
    const SparseShard &S = *Z.csc;
    const real_t *mu = Z.has_mu ? Z.mu.ptr : nullptr;
    SZ_DISPATCH(sz_cols_kernel, kc, Z.nseg, Z.segs.ptr, Z.nseg, S.i.ptr, S.v.ptr, F, ldf, kc, mu, svec, out, ldo, Z.col_part.ptr);
    if (Z.nlong)
        hipLaunchKernelGGL(sz_cols_finish_kernel<real_t>, dim3((unsigned)(((size_t)Z.nlong * kc + 255) / 256)), dim3(256), 0, dev.stream,
                           Z.longs.ptr, Z.nlong, Z.col_part.ptr, kc, mu, svec, out, ldo);
    HIP_CHECK(hipGetLastError());
}

}  // namespace cmfhip
