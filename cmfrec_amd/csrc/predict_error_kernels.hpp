// predict_error_kernels.hpp -- the error of the predictions on held-out (row, col, x[, weight]) pairs, reduced on the device:
// score_errors_kernel, reduce_error_partials and their launch helper launch_score_errors (the evaluation set of
// cmfrec_hip_evalset_*, cmfrec_hip_scorer_errors, cmfrec_hip_session_errors and cmfrec_hip_pair_errors: predict_tu.hip).
// DESIGN.md section 3.11.
//
// The prediction p of a pair is score_pairs_kernel's, bit for bit: both kernels run score_chunks (predict_kernels.hpp), the
// same loads, fused multiply-adds and butterfly, and differ in the epilogue alone.  Here lane 0 of the pair's group forms, in
// double precision whatever T is,  e = (double)p - (double)x[i]  and  w = weight ? (double)weight[i] : 1,  and adds the pair to
// one of two classes kept in its own registers:
//   class 0 "scored":    row and col inside the model
//   class 1 "fallback":  explicit rule, the pair outside the model, p the fallback value
// per class n (64-bit count), sum_w, sum_we = sum w e, sum_wabs = sum w |e|, sum_wsq = sum w e^2 and max_abs = max |e|.  A pair
// whose x is NaN and, under the implicit rule, a pair outside the model (its prediction is NaN by definition) adds to n_skipped
// and to nothing else; an infinite x is a value like any other.  pred (optional): p is stored too, skipped pairs included.
//
// After its last chunk a wavefront folds the 64 lanes' accumulators with an xor butterfly (DPP inside 16-lane rows, permlane
// swaps across them; the lanes that are not lane 0 of a group carry zeros) -- every level combines the same two values in both
// partner lanes, so all lanes end with the same bits -- and lane 0 writes the wavefront's record to partials[wave] with ordinary
// vector stores: every wavefront of the launch writes one, those without a chunk a record of zeros.  reduce_error_partials,
// one workgroup, combines the records in an order that is a function of the wavefront index alone: thread t takes the records
// t, t + 256, ... in ascending order, then one thread per field takes the 256 threads' results in ascending order.  No atomics of
// any kind and no LDS in the first kernel: the same call on the same device and grid returns the same bytes.
#pragma once
#include "../../include/cmfrec_hip.h"
#include "predict_kernels.hpp"

namespace cmfhip {

// a record is 13 fields of 8 bytes, in the order of cmfrec_hip_errors: three counts, eight sums, two maxima
constexpr int ERR_FIELDS = 13, ERR_COUNTS = 3, ERR_SUMS = 8;
static_assert(sizeof(cmfrec_hip_errors) == ERR_FIELDS * 8, "cmfrec_hip_errors has padding");
constexpr int ERR_REDUCE_TH = 256;

template <typename T>
struct ErrorParams {
    const T *x = nullptr;                  // [n_pairs]
    const T *weight = nullptr;             // [n_pairs] or null
    T *pred = nullptr;                     // [n_pairs] or null
    cmfrec_hip_errors *partials = nullptr; // one record per wavefront of the launch, then the final record
};

// the epilogue of score_chunks: x and the weight of a step's pairs are asked for with the step's indices, the sums are the lane's own
template <typename T>
struct ScoreErrors {
    const ErrorParams<T> &E;
    const int implicit;
    unsigned long long n0 = 0, n1 = 0, nskip = 0;
    double w0 = 0, we0 = 0, wabs0 = 0, wsq0 = 0, max0 = 0;
    double w1 = 0, we1 = 0, wabs1 = 0, wsq1 = 0, max1 = 0;
    T xs[SCORE_STEPS], ws[SCORE_STEPS];
    __device__ __forceinline__ ScoreErrors(const ErrorParams<T> &E_, int implicit_) : E(E_), implicit(implicit_) {}
    __device__ __forceinline__ void begin(int u, size_t i, bool mine)
    {
        xs[u] = mine ? E.x[i] : (T)0;
    }
    // (the weights are asked for once the pieces' registers are free: four more values per lane through the rounds would cost a
    // wavefront per SIMD in double precision)
    __device__ __forceinline__ void middle(int u, size_t i, bool mine)
    {
        ws[u] = (mine && E.weight) ? E.weight[i] : (T)1;
    }
    __device__ __forceinline__ void end(int u, size_t i, bool ok, T res)
    {
        if (E.pred) E.pred[i] = res;
        const double x = (double)xs[u], w = (double)ws[u];
        const double e = (double)res - x, ae = fabs(e);
        if (x != x || (!ok && implicit)) {
            nskip++;
        } else if (ok) {
            n0++; w0 += w; we0 += w * e; wabs0 += w * ae; wsq0 += w * (e * e); max0 = fmax(max0, ae);
        } else {
            n1++; w1 += w; we1 += w * e; wabs1 += w * ae; wsq1 += w * (e * e); max1 = fmax(max1, ae);
        }
    }
};

template <typename T, int G, bool VA, bool VB>
__global__ __launch_bounds__(SCORE_TH) void score_errors_kernel(const ScoreParams<T> P, const ErrorParams<T> E)
{
    ScoreErrors<T> epi(E, P.implicit);
    size_t wave, nwaves;
    score_chunks<T, G, VA, VB>(P, epi, wave, nwaves);
    // (every wavefront of the launch arrives here with all 64 lanes, whether it had a chunk or not)
    auto add = [](double a, double b) { return a + b; };
    auto mx = [](double a, double b) { return fmax(a, b); };
    cmfrec_hip_errors r;
    r.n[0] = lanes::wave_sum_u64(epi.n0); r.n[1] = lanes::wave_sum_u64(epi.n1); r.n_skipped = lanes::wave_sum_u64(epi.nskip);
    r.sum_w[0] = lanes::wave_fold(epi.w0, add); r.sum_w[1] = lanes::wave_fold(epi.w1, add);
    r.sum_we[0] = lanes::wave_fold(epi.we0, add); r.sum_we[1] = lanes::wave_fold(epi.we1, add);
    r.sum_wabs[0] = lanes::wave_fold(epi.wabs0, add); r.sum_wabs[1] = lanes::wave_fold(epi.wabs1, add);
    r.sum_wsq[0] = lanes::wave_fold(epi.wsq0, add); r.sum_wsq[1] = lanes::wave_fold(epi.wsq1, add);
    r.max_abs[0] = lanes::wave_fold(epi.max0, mx); r.max_abs[1] = lanes::wave_fold(epi.max1, mx);
    if ((threadIdx.x & 63) == 0) E.partials[wave] = r;
}

// field f of two records combined: a count, a sum or a maximum.  The fields travel as their 64 bits.
__device__ __forceinline__ unsigned long long err_combine(int f, unsigned long long a, unsigned long long b)
{
    if (f < ERR_COUNTS) return a + b;
    const double x = __longlong_as_double((long long)a), y = __longlong_as_double((long long)b);
    return (unsigned long long)__double_as_longlong(f < ERR_COUNTS + ERR_SUMS ? x + y : fmax(x, y));
}

// partials[0 .. nrec) -> partials[nrec]; one workgroup of ERR_REDUCE_TH threads
__global__ __launch_bounds__(ERR_REDUCE_TH) void reduce_error_partials(cmfrec_hip_errors *partials, size_t nrec)
{
    __shared__ unsigned long long part[ERR_FIELDS][ERR_REDUCE_TH];
    const unsigned long long *raw = reinterpret_cast<const unsigned long long *>(partials);
    const int t = threadIdx.x;
    unsigned long long acc[ERR_FIELDS];
#pragma unroll
    for (int f = 0; f < ERR_FIELDS; f++) acc[f] = 0;        // (the bits of 0.0 too)
    for (size_t r = (size_t)t; r < nrec; r += ERR_REDUCE_TH)
#pragma unroll
        for (int f = 0; f < ERR_FIELDS; f++) acc[f] = err_combine(f, acc[f], raw[r * ERR_FIELDS + f]);
#pragma unroll
    for (int f = 0; f < ERR_FIELDS; f++) part[f][t] = acc[f];
    __syncthreads();
    if (t < ERR_FIELDS) {
        unsigned long long v = 0;
        for (int s = 0; s < ERR_REDUCE_TH; s++) v = err_combine(t, v, part[t][s]);
        reinterpret_cast<unsigned long long *>(partials)[nrec * ERR_FIELDS + t] = v;
    }
}

template <typename K, typename T>
inline size_t launch_errors_kernel(K kernel, hipStream_t st, size_t blocks, int num_cus, int max_waves, const ScoreParams<T> &P,
                                   const ErrorParams<T> &E, bool dry)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, SCORE_TH, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    size_t grid = std::min<size_t>(blocks, (size_t)num_cus * (size_t)per_cu);
    if (max_waves > 0) grid = std::min<size_t>(grid, ((size_t)max_waves + SCORE_TH / 64 - 1) / (SCORE_TH / 64));
    if (!dry) hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(SCORE_TH), 0, st, P, E);
    return grid * (SCORE_TH / 64);
}

template <typename T, int G>
inline size_t launch_errors_width(hipStream_t st, size_t blocks, int num_cus, int max_waves, const ScoreParams<T> &P, const ErrorParams<T> &E,
                                  bool va, bool vb, bool dry)
{
    if (va && vb) return launch_errors_kernel(score_errors_kernel<T, G, true, true>, st, blocks, num_cus, max_waves, P, E, dry);
    if (va) return launch_errors_kernel(score_errors_kernel<T, G, true, false>, st, blocks, num_cus, max_waves, P, E, dry);
    if (vb) return launch_errors_kernel(score_errors_kernel<T, G, false, true>, st, blocks, num_cus, max_waves, P, E, dry);
    return launch_errors_kernel(score_errors_kernel<T, G, false, false>, st, blocks, num_cus, max_waves, P, E, dry);
}

// The scoring launch over P.n_pairs >= 1 pairs (P.out is not used) and, behind it, the reduction of its records into
// E.partials[waves]; returns waves, the wavefronts of the launch.  max_waves > 0 caps them (rounded up to whole workgroups).
// dry: nothing is launched -- the caller sizes E.partials (waves + 1 records) from the return value first.  The same checks as
// launch_score_pairs are the caller's.
template <typename T>
inline size_t launch_score_errors(hipStream_t st, int num_cus, int max_waves, const ScoreParams<T> &P, const ErrorParams<T> &E, bool dry)
{
    const int G = score_group_width<T>(P.kk);
    const size_t per_chunk = (size_t)(64 / G) * SCORE_STEPS, per_block = per_chunk * (SCORE_TH / 64);
    const size_t blocks = (P.n_pairs + per_block - 1) / per_block;
    const bool va = P.m > 0 && score_wide_ok(P.A, P.lda), vb = P.n > 0 && score_wide_ok(P.B, P.ldb);
    size_t waves;
    switch (G) {
    case 1: waves = launch_errors_width<T, 1>(st, blocks, num_cus, max_waves, P, E, va, vb, dry); break;
    case 2: waves = launch_errors_width<T, 2>(st, blocks, num_cus, max_waves, P, E, va, vb, dry); break;
    case 4: waves = launch_errors_width<T, 4>(st, blocks, num_cus, max_waves, P, E, va, vb, dry); break;
    case 8: waves = launch_errors_width<T, 8>(st, blocks, num_cus, max_waves, P, E, va, vb, dry); break;
    case 16: waves = launch_errors_width<T, 16>(st, blocks, num_cus, max_waves, P, E, va, vb, dry); break;
    case 32: waves = launch_errors_width<T, 32>(st, blocks, num_cus, max_waves, P, E, va, vb, dry); break;
    default: waves = launch_errors_width<T, 64>(st, blocks, num_cus, max_waves, P, E, va, vb, dry); break;
    }
    if (!dry) hipLaunchKernelGGL(reduce_error_partials, dim3(1), dim3(ERR_REDUCE_TH), 0, st, E.partials, waves);
    return waves;
}

}  // namespace cmfhip
