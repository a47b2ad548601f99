// rank_metrics_kernels.hpp -- the ranking metrics of held-out items reduced on the device (cmfrec_hip_rankset_*,
// cmfrec_hip_ranker_metrics, cmfrec_hip_session_ranking: topn_tu.hip).
//
// Input: what topn_rank_kernel leaves on the device -- per held-out entry its 0-based rank in the user's full ranking (-1: the item
// is outside the model or excluded) and per user the pool size P -- and the held-out lists' CSR offsets.  Per user exactly the
// quantities of cmfrec_amd.metrics.ranking_metrics at cut-off k: with r_1 < ... < r_T the valid ranks and h = #{r_j < k}
//   hit h > 0, precision h / k, recall h / T, ap sum_{r_j < k} j / (r_j + 1) / min(k, T), ndcg sum_{r_j < k} disc[r_j] / ideal[min(k, T)],
//   rr 1 / (r_1 + 1), auc 1 - sum_j (r_j - (j - 1)) / (T (P - T)), mean_rank sum r_j / T.
// T = 0 leaves the user out of every metric, P = T out of auc alone.  disc[r] = 1 / log2(r + 2) for r < k and ideal[c] = the sum of
// the first c of them are tables computed by the host in float64 with libm's log2 (not the device's), as NumPy forms them: where
// NumPy's log2 is libm's too, every TERM of a sum equals NumPy's bit for bit and only the order of the additions differs; a NumPy
// built on another vector library may differ in the last bit of a discount, which the tests' bound has room for.
//
// rank_metrics_kernel: one wavefront per user, grid-stride over the users.  The lanes take the user's entries 64 at a time.  The
// place j of a rank among the user's own ranks is 1 + the number of the user's valid ranks that are smaller (equal ranks -- an
// item listed twice -- in list order, as NumPy's stable sort leaves them): every 64 ranks of the list are held one per lane and
// passed round by __shfl, so a list of any length needs no buffer (the cross-lane reads are the LDS crossbar's, no LDS is
// allocated).  The price: a list of L entries costs ceil(L / 64)^2 rounds of 64 cross-lane reads per lane and reads its ranks
// ceil(L / 64) times from L1 / L2 -- 1,024 reads per lane at L = 200, 16,384 at L = 1,000, quadratic beyond: one user with tens of
// thousands of held-out items would be the tail of the launch.  Held-out lists of an evaluation are tens to hundreds of items; a
// sort in LDS per user is what longer lists would need.  The user's sums are folded by a butterfly (lanes::wave_fold), the
// user's eight values are formed by every lane alike and added to the wavefront's record: per metric the float64 sum over its users and the number of users that contributed.  One
// record per wavefront, then rank_metrics_reduce -- one workgroup, thread t takes records t, t + 256, ... in ascending order, then
// one thread per field takes the 256 results in ascending order -- writes the final record behind them.  No atomics: the same
// call on the same device and grid returns the same bytes.
#pragma once
#include "../../include/cmfrec_hip.h"
#include "lanes.hpp"

namespace cmfhip {

constexpr int RANKM_METRICS = 8;                       // hit, precision, recall, ap, ndcg, rr, auc, mean_rank
constexpr int RANKM_FIELDS = 2 * RANKM_METRICS + 1;    // the sums, the counts, the users with T > 0
static_assert(sizeof(cmfrec_hip_rank_record) == RANKM_FIELDS * 8, "cmfrec_hip_rank_record has padding");
constexpr int RANKM_TH = 256, RANKM_REDUCE_TH = 256;

struct RankMetricParams {
    const int *ranks = nullptr;          // [held_p[nu]]
    const int *pool = nullptr;           // [nu]
    const size_t *held_p = nullptr;      // [nu + 1]
    int nu = 0, k_at = 1;
    const double *disc = nullptr;        // [k_at]
    const double *ideal = nullptr;       // [k_at + 1]
    double *per_user = nullptr;          // [nu, 8] or null: NaN where the user does not count
    cmfrec_hip_rank_record *partials = nullptr;   // one record per wavefront of the launch, then the final one
};

__global__ __launch_bounds__(RANKM_TH) void rank_metrics_kernel(const RankMetricParams P)
{
    const int lane = threadIdx.x & 63;
    const size_t wave = ((size_t)blockIdx.x * RANKM_TH + threadIdx.x) >> 6, nwaves = ((size_t)gridDim.x * RANKM_TH) >> 6;
    auto add = [](double a, double b) { return a + b; };
    double sum[RANKM_METRICS];
    unsigned long long cnt[RANKM_METRICS], users = 0;
#pragma unroll
    for (int f = 0; f < RANKM_METRICS; f++) { sum[f] = 0; cnt[f] = 0; }
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    for (size_t u = wave; u < (size_t)P.nu; u += nwaves) {
        const size_t lo = P.held_p[u], len = P.held_p[u + 1] - lo;
        const size_t chunks = (len + 63) / 64;
        unsigned long long T = 0, h = 0;
        double s_ap = 0, s_ndcg = 0, s_auc = 0, s_rank = 0;
        int first = 0x7fffffff;
        for (size_t q = 0; q < chunks; q++) {                       // my entry of this round: q * 64 + lane
            const size_t e = q * 64 + (size_t)lane;
            const int r = e < len ? P.ranks[lo + e] : -1;
            unsigned long long smaller = 0;
            for (size_t c = 0; c < chunks; c++) {                   // against every entry of the list, 64 at a time
                const size_t o = c * 64 + (size_t)lane;
                const int v = o < len ? P.ranks[lo + o] : -1;
                for (int s = 0; s < 64; s++) {
                    const int w = __shfl(v, s);
                    smaller += (w >= 0 && (w < r || (w == r && c * 64 + (size_t)s < e))) ? 1u : 0u;
                }
            }
            if (r >= 0) {
                const unsigned long long j = smaller + 1;
                T++;
                first = min(first, r);
                s_rank += (double)r;
                s_auc += (double)((long long)r - (long long)(j - 1));
                if (r < P.k_at) { h++; s_ap += (double)j / ((double)r + 1.0); s_ndcg += P.disc[r]; }
            }
        }
        T = lanes::wave_sum_u64(T); h = lanes::wave_sum_u64(h);
        s_ap = lanes::wave_fold(s_ap, add); s_ndcg = lanes::wave_fold(s_ndcg, add);
        s_auc = lanes::wave_fold(s_auc, add); s_rank = lanes::wave_fold(s_rank, add);
        first = (int)lanes::wave_fold((double)first, [](double a, double b) { return fmin(a, b); });   // (an int is exact as a double)
        double v[RANKM_METRICS];
        if (T > 0) {
            const double Tf = (double)T, k = (double)P.k_at;
            const unsigned long long cut = T < (unsigned long long)P.k_at ? T : (unsigned long long)P.k_at;
            const long long rest = (long long)P.pool[u] - (long long)T;
            v[0] = h > 0 ? 1.0 : 0.0;
            v[1] = (double)h / k;
            v[2] = (double)h / Tf;
            v[3] = s_ap / (double)cut;
            v[4] = s_ndcg / P.ideal[cut];
            v[5] = 1.0 / ((double)first + 1.0);
            v[6] = rest != 0 ? 1.0 - s_auc / (Tf * (double)rest) : nan;
            v[7] = s_rank / Tf;
            users++;
#pragma unroll
            for (int f = 0; f < RANKM_METRICS; f++)
                if (v[f] == v[f]) { sum[f] += v[f]; cnt[f]++; }
        } else {
#pragma unroll
            for (int f = 0; f < RANKM_METRICS; f++) v[f] = nan;
        }
        if (P.per_user != nullptr && lane < RANKM_METRICS) {
            double mine = v[0];
#pragma unroll
            for (int f = 1; f < RANKM_METRICS; f++) mine = lane == f ? v[f] : mine;
            P.per_user[u * RANKM_METRICS + (size_t)lane] = mine;
        }
    }
    if (lane == 0) {
        cmfrec_hip_rank_record rec;
#pragma unroll
        for (int f = 0; f < RANKM_METRICS; f++) { rec.sum[f] = sum[f]; rec.count[f] = cnt[f]; }
        rec.users = users;
        P.partials[wave] = rec;
    }
}

// field f of two records combined: a float64 sum or a count.  The fields travel as their 64 bits.
__device__ __forceinline__ unsigned long long rankm_combine(int f, unsigned long long a, unsigned long long b)
{
    if (f >= RANKM_METRICS) return a + b;
    return (unsigned long long)__double_as_longlong(__longlong_as_double((long long)a) + __longlong_as_double((long long)b));
}

// partials[0 .. nrec) -> partials[nrec]; one workgroup of RANKM_REDUCE_TH threads
__global__ __launch_bounds__(RANKM_REDUCE_TH) void rank_metrics_reduce(cmfrec_hip_rank_record *partials, size_t nrec)
{
    __shared__ unsigned long long part[RANKM_FIELDS][RANKM_REDUCE_TH];
    const unsigned long long *raw = reinterpret_cast<const unsigned long long *>(partials);
    const int t = threadIdx.x;
    unsigned long long acc[RANKM_FIELDS];
#pragma unroll
    for (int f = 0; f < RANKM_FIELDS; f++) acc[f] = 0;      // (the bits of 0.0 too)
    for (size_t r = (size_t)t; r < nrec; r += RANKM_REDUCE_TH)
#pragma unroll
        for (int f = 0; f < RANKM_FIELDS; f++) acc[f] = rankm_combine(f, acc[f], raw[r * RANKM_FIELDS + f]);
#pragma unroll
    for (int f = 0; f < RANKM_FIELDS; f++) part[f][t] = acc[f];
    __syncthreads();
    if (t < RANKM_FIELDS) {
        unsigned long long v = 0;
        for (int s = 0; s < RANKM_REDUCE_TH; s++) v = rankm_combine(t, v, part[t][s]);
        reinterpret_cast<unsigned long long *>(partials)[nrec * RANKM_FIELDS + t] = v;
    }
}

// the wavefronts of a launch over nu users: one per user up to what the device holds at once; max_waves > 0 caps them (rounded up
// to whole workgroups)
inline size_t rank_metrics_waves(int nu, int num_cus, int max_waves)
{
    const size_t per_block = RANKM_TH / 64;
    size_t blocks = std::min<size_t>(((size_t)std::max(nu, 1) + per_block - 1) / per_block, (size_t)num_cus * 8);
    if (max_waves > 0) blocks = std::min<size_t>(blocks, ((size_t)max_waves + per_block - 1) / per_block);
    return blocks * per_block;
}

// both kernels on stream st; P.partials holds waves + 1 records (waves = rank_metrics_waves of the same arguments)
inline void launch_rank_metrics(hipStream_t st, size_t waves, const RankMetricParams &P)
{
    hipLaunchKernelGGL(rank_metrics_kernel, dim3((unsigned)(waves / (RANKM_TH / 64))), dim3(RANKM_TH), 0, st, P);
    hipLaunchKernelGGL(rank_metrics_reduce, dim3(1), dim3(RANKM_REDUCE_TH), 0, st, P.partials, waves);
}

}  // namespace cmfhip
