// dense_rows_device.hpp -- the present entries of a dense batch of new rows as a device COO.
//
// factors_collective_explicit_multiple takes the new rows' X as a dense [rows, n] block with NaN for "not observed"
// (Xfull, collective.c:11108-11115); a row is then solved on its present entries (common.c:1038-1055,
// collective.c:1671-1690, :1724-1733).  The block is uploaded as it is and compacted here into the triplets
// (row, column, x - glob_mean, weight) of its present entries, in row-major order, together with every row's number of
// missing entries; shard_from_coo's stable sort keeps that order, so the result does not change from run to run.
//
// Two passes, one wavefront per row, consecutive lanes on consecutive columns:
//   1. count: per chunk of 64 columns a ballot of "present" and its population count;
//   2. an exclusive scan of the counts over the rows, then the write pass: lane's slot = row offset + the chunks' running
//      total + the number of present lanes below it in the ballot (mbcnt).
// No atomics.  The weights are read only where X is present (their payload elsewhere is the caller's NaN or garbage).
#pragma once
#include "coo_device.hpp"

namespace cmfhip {

constexpr int DENSE_ROWS_WAVES = 4;       // rows (wavefronts) per workgroup
constexpr int DENSE_ROWS_UNROLL = 4;      // chunks of 64 columns in flight per wavefront

// (bit test: independent of how the translation unit's floating-point flags treat NaN comparisons)
__device__ __forceinline__ bool dense_is_nan(double v) { return ((unsigned long long)__double_as_longlong(v) & 0x7fffffffffffffffull) > 0x7ff0000000000000ull; }
__device__ __forceinline__ bool dense_is_nan(float v) { return ((unsigned)__float_as_int(v) & 0x7fffffffu) > 0x7f800000u; }

// lanes below this one whose bit is set in a wavefront ballot
__device__ __forceinline__ int ballot_prefix(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

template <typename T>
__global__ void __launch_bounds__(64 * DENSE_ROWS_WAVES)
dense_rows_count_kernel(const T *__restrict__ X, int rows, int n, unsigned *__restrict__ present, int *__restrict__ missing)
{
    const int row = blockIdx.x * DENSE_ROWS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;                        // (the whole wavefront)
    const T *x = X + (size_t)row * (size_t)n;
    int cnt = 0;
    for (int c0 = 0; c0 < n; c0 += 64 * DENSE_ROWS_UNROLL) {
        bool here[DENSE_ROWS_UNROLL];
#pragma unroll
        for (int u = 0; u < DENSE_ROWS_UNROLL; u++) {
            const int col = c0 + 64 * u + lane;
            here[u] = (col < n) && !dense_is_nan(x[min(col, n - 1)]);
        }
#pragma unroll
        for (int u = 0; u < DENSE_ROWS_UNROLL; u++) cnt += __popcll(__ballot(here[u]));
    }
    if (lane == 0) { present[row] = (unsigned)cnt; missing[row] = n - cnt; }
}

// row_off: exclusive scan of `present`, relative to the block's first entry; row0: the block's first row in the batch
template <typename T>
__global__ void __launch_bounds__(64 * DENSE_ROWS_WAVES)
dense_rows_write_kernel(const T *__restrict__ X, const T *__restrict__ W, int rows, int n, int row0, T subtract,
                        const size_t *__restrict__ row_off, int *__restrict__ out_row, int *__restrict__ out_col,
                        T *__restrict__ out_val, T *__restrict__ out_wt)
{
    const int row = blockIdx.x * DENSE_ROWS_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const T *x = X + (size_t)row * (size_t)n;
    const T *w = (W != nullptr) ? W + (size_t)row * (size_t)n : nullptr;
    const size_t last = row_off[row + 1];           // (bound of this row's slots: nothing is written at or beyond it)
    size_t slot0 = row_off[row];
    for (int c0 = 0; c0 < n; c0 += 64 * DENSE_ROWS_UNROLL) {
        T v[DENSE_ROWS_UNROLL];
        bool here[DENSE_ROWS_UNROLL];
#pragma unroll
        for (int u = 0; u < DENSE_ROWS_UNROLL; u++) {
            const int col = c0 + 64 * u + lane;
            v[u] = x[min(col, n - 1)];
            here[u] = (col < n) && !dense_is_nan(v[u]);
        }
#pragma unroll
        for (int u = 0; u < DENSE_ROWS_UNROLL; u++) {
            const int col = c0 + 64 * u + lane;
            const unsigned long long mask = __ballot(here[u]);
            const size_t slot = slot0 + (size_t)ballot_prefix(mask);
            if (here[u] && slot < last) {
                out_row[slot] = row0 + row;
                out_col[slot] = col;
                out_val[slot] = v[u] - subtract;
                if (w != nullptr) out_wt[slot] = w[col];
            }
            slot0 += (size_t)__popcll(mask);
        }
    }
}

// complete rows as the operand of the TransBtBinvBt product (common.c:741-746 after preprocess_vec, collective.c:6337-6388):
// x - glob_mean - biasB[col] in place; rows with a missing entry become zeros (their products are not used)
template <typename T>
__global__ void dense_rows_center_kernel(T *__restrict__ X, size_t rows, int n, T subtract, const T *__restrict__ bias,
                                         const int *__restrict__ missing)
{
    const size_t total = rows * (size_t)n;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / (size_t)n; const int c = (int)(e % (size_t)n);
        X[e] = (missing[r] == 0) ? X[e] - subtract - (bias != nullptr ? bias[c] : T(0)) : T(0);
    }
}

// A[r, off : off + kk] = src[r, :] for the rows without a missing entry
template <typename T>
__global__ void dense_rows_select_complete_kernel(T *__restrict__ A, size_t lda, int off, const T *__restrict__ src, int kk,
                                                  const int *__restrict__ missing, size_t rows)
{
    const size_t total = rows * (size_t)kk;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / (size_t)kk; const int f = (int)(e % (size_t)kk);
        if (missing[r] == 0) A[r * lda + off + f] = src[e];
    }
}

// implicit-features term of the right-hand sides (collective.c:1757-1771, Xones = 1 on the row's observed items):
// A[r, off + f] += w * sum_{j in row r} Bi[j, f], the entries in CSR order; one wavefront per row, lane <-> column
template <typename T>
__global__ void __launch_bounds__(256)
implicit_rhs_rows_kernel(const size_t *__restrict__ indptr, const int *__restrict__ indices, const T *__restrict__ Bi, int kk,
                         T w, int rows, T *__restrict__ A, size_t lda, int off)
{
    const int row = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (row >= rows) return;
    const size_t st = indptr[row], en = indptr[row + 1];
    if (en == st) return;
    for (int f = lane; f < kk; f += 64) {
        T acc = T(0);
        for (size_t e = st; e < en; e++) acc += Bi[(size_t)indices[e] * kk + f];
        A[(size_t)row * lda + off + f] += w * acc;
    }
}

// rows whose weights sum to (almost) nothing under scale_lam come out as zeros (common.c:712, collective.c:1324-1329):
// rows with entries, |wsum| < eps, and -- rows_keep -- no side information of their own
template <typename T>
__global__ void zero_weightless_rows_kernel(const size_t *__restrict__ indptr, const T *__restrict__ wsum, int rows, int rows_keep,
                                            T eps, T *__restrict__ A, size_t lda, int kt)
{
    const int r = blockIdx.x;
    if (r >= rows || r < rows_keep || indptr[r + 1] == indptr[r] || !(fabs((double)wsum[r]) < (double)eps)) return;
    for (int e = threadIdx.x; e < kt; e += blockDim.x) A[(size_t)r * lda + e] = T(0);
}

struct DenseRowsCoo {
    DevBuf<int> row, col;
    DevBuf<real_t> val, wt;
    size_t nnz = 0;
};

// One block of rows: dX [rows, n] (and dW, or null) in HBM -> out (global row ids row0 + r), d_missing[rows].
// Returns after the block's entry count has reached the host.
inline void dense_rows_to_coo(const real_t *dX, const real_t *dW, int rows, int n, int row0, real_t subtract, int *d_missing,
                              DenseRowsCoo &out, hipStream_t st)
{
    DevBuf<unsigned> cnt; DevBuf<size_t> off; DevBuf<unsigned char> tmp;
    cnt.alloc((size_t)rows + 1); off.alloc((size_t)rows + 1);
    HIP_CHECK(hipMemsetAsync(cnt.ptr, 0, ((size_t)rows + 1) * sizeof(unsigned), st));
    const dim3 grid((unsigned)((rows + DENSE_ROWS_WAVES - 1) / DENSE_ROWS_WAVES)), block(64 * DENSE_ROWS_WAVES);
    hipLaunchKernelGGL(dense_rows_count_kernel<real_t>, grid, block, 0, st, dX, rows, n, cnt.ptr, d_missing);
    HIP_CHECK(hipGetLastError());
    auto in = rocprim::make_transform_iterator(cnt.ptr, u32_to_size());
    size_t bytes = 0;
    HIP_CHECK(rocprim::exclusive_scan(nullptr, bytes, in, off.ptr, (size_t)0, (size_t)rows + 1, rocprim::plus<size_t>(), st));
    tmp.alloc(bytes + 16);
    HIP_CHECK(rocprim::exclusive_scan(tmp.ptr, bytes, in, off.ptr, (size_t)0, (size_t)rows + 1, rocprim::plus<size_t>(), st));
    size_t total = 0;
    HIP_CHECK(hipMemcpyAsync(&total, off.ptr + rows, sizeof(size_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    out.nnz = total;
    out.row.alloc(total); out.col.alloc(total); out.val.alloc(total);
    if (dW != nullptr) out.wt.alloc(total);
    if (total) {
        hipLaunchKernelGGL(dense_rows_write_kernel<real_t>, grid, block, 0, st, dX, dW, rows, n, row0, subtract, off.ptr, out.row.ptr,
                           out.col.ptr, out.val.ptr, dW != nullptr ? out.wt.ptr : nullptr);
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipStreamSynchronize(st));            // cnt / off / tmp are released here
}

}  // namespace cmfhip
