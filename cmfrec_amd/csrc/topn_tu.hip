// topn_tu.hip -- the ranking entry points: cmfrec_hip_ranker_* (the item factors stay on the device between calls) and
// cmfrec_hip_topN_batch (one ranker for one call).  A translation unit of its own, like chol_wg_tu.hip: the wide kernel's
// instantiations stay out of session.hip's compile.
//
// Routing: k <= TOPN_KMAX (64) launches topn_kernel, the kernel of every release so far; beyond that -- or for every k under
// CMFREC_HIP_TOPN=wide, a cross-check and A/B switch -- topn_wide_kernel (topn_wide_kernels.hpp).  A call with candidate lists
// (cmfrec_hip_ranker_topN_candidates and its kin) launches topn_cand_kernel (topn_cand_kernels.hpp) for every k.  A rank call
// (cmfrec_hip_ranker_ranks and its kin) launches topn_rank_kernel (topn_rank_kernels.hpp) for every k.  A neighbour call
// (cmfrec_hip_ranker_similar and its kin) launches topn_similar_kernel (topn_similar_kernels.hpp) for every k: the wide
// kernel's body with the query tile gathered from the resident rows.  A deep or next-page call (cmfrec_hip_ranker_topN_deep /
// _topN_after) launches topn_after_kernel (topn_after_kernels.hpp) for every k, once per page: the wide kernel's body behind a
// per-user cursor.  A ranker whose split setting is on (cmfrec_hip_ranker_set_split) sends the full ranking, for every k, to the MFMA
// arithmetic: topn_wide_kernel itself where the planner (cmfrec_hip_topn_split_plan) leaves the items whole, else
// topn_split_kernel over slices of the items and topn_split_merge_kernel behind it (topn_split_kernels.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include "device_base.hpp"
#include "newrows.hpp"
#include "topn_wide_kernels.hpp"
#include "topn_split_kernels.hpp"
#include "topn_similar_kernels.hpp"
#include "topn_after_kernels.hpp"
#include "topn_cand_kernels.hpp"
#include "topn_rank_kernels.hpp"
#include "rank_metrics_kernels.hpp"

using namespace cmfhip;

namespace cmfhip { void poison_lds(hipStream_t st, int num_cus); }   // launch_cg.hip (launch.hpp): test hook, CMFREC_HIP_POISON_LDS=1

struct cmfrec_hip_ranker {
    struct Device { int device = 0, num_cus = 256; hipStream_t stream = nullptr; } dev;
    int n = 0, k = 0;
    size_t ldb = 0;                          // columns of the packed item matrix on the device: topnw_kp(k), columns [k, ldb) zero
    bool has_bias = false;
    DevBuf<real_t> B, bias;                  // uploaded once
    DevBuf<real_t> A, sc;                    // per call; they grow on demand
    DevBuf<size_t> ep;
    DevBuf<int> ei, ids;
    DevBuf<size_t> cp;                       // candidate lists of a candidate call
    DevBuf<int> ci, corder;                  // ... and the users by descending list length
    DevBuf<unsigned> next;                   // work counter of topn_cand_kernel
    DevBuf<int> pool;                        // per-user pool of a rank call (its held-out lists use cp / ci, its ranks ids)
    DevBuf<real_t> rn;                       // inverse row norms of B: made by the first cosine call, resident from then on
    bool has_rn = false;
    DevBuf<int> qid;                         // query ids of a neighbour call
    DevBuf<real_t> cur_s;                    // the caller's cursors of a next-page call
    DevBuf<int> cur_i;
    int last_pages = 0, last_page_len = 0;   // launches and page length of the last deep call
    hipEvent_t ev0 = nullptr, ev1 = nullptr; // around the ranking kernel of the last call
    bool timed = false;
    int last_users = 0, last_grid = 0;       // users per workgroup and workgroups of that launch
    int split = -1;                          // cmfrec_hip_ranker_set_split: -1 off, 0 the planner's choice, >= 1 that many slices
    int last_slices = 1;                     // item slices of the last ranking launch
    DevBuf<real_t> part_sc;                  // the slices' lists of a split call: [slices][nu][n_top]
    DevBuf<int> part_id;
    ~cmfrec_hip_ranker()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (dev.stream) (void)hipStreamDestroy(dev.stream);
    }
};

namespace {

constexpr const char *LIMITS = "needs k <= 272 and n_top <= min(128, n)";
constexpr const char *RANK_LIMITS = "needs k <= 272";
constexpr const char *DEEP_LIMITS = "needs k <= 272 and 1 <= n_top <= n";

// User tiles per workgroup of the wide kernel (DESIGN.md "Top-N for wide models"): as many as the LDS holds beside the lists,
// unless fewer finish the nu users in fewer or cheaper waves of workgroups.  A workgroup's time per item round is about
// (nut + 1/2) -- its MFMAs and the item fetch they share -- times the workgroups that share its CU.
// CMFREC_HIP_TOPN_TILES (test hook) asks for a number of tiles; it is clamped to what fits.
// extra_per_tile: LDS bytes per user tile beyond topnw_lds_bytes (the neighbour kernel's ids and inverse norms).
int pick_user_tiles(int nu, int k, int n_top, int num_cus, int *blocks_per_cu, size_t extra_per_tile = 0, size_t sizeof_real = sizeof(real_t))
{
    const int forced = switches().topn_tiles;
    int best = 1, best_bpc = 1;
    double best_cost = 0;
    for (int nut = 1; nut <= TOPNW_MAX_NUT; nut++) {
        const size_t smem = topnw_lds_bytes(nut, k, n_top, sizeof_real) + nut * extra_per_tile;
        if (smem > TOPNW_LDS_MAX) break;
        const int bpc = (int)std::min<size_t>(TOPNW_LDS_MAX / smem, (size_t)(2048 / TOPNW_TH));
        const long tiles = ((long)nu + 16 * nut - 1) / (16 * nut), slots = (long)num_cus * bpc;
        const long share = std::min<long>(bpc, (tiles + num_cus - 1) / num_cus);
        const double cost = (double)((tiles + slots - 1) / slots) * share * (nut + 0.5);
        if (nut == 1 || (forced > 0 ? nut <= forced : cost <= best_cost)) { best = nut; best_bpc = bpc; best_cost = cost; }
    }
    *blocks_per_cu = best_bpc;
    return best;
}

template <int NUT>
int launch_wide(const cmfrec_hip_ranker::Device &dev, const TopnWideParams<real_t> &P, int blocks_per_cu)
{
    const size_t smem = topnw_lds_bytes(NUT, P.k, P.n_top, sizeof(real_t));
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_wide_kernel<real_t, NUT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = (P.nu + 16 * NUT - 1) / (16 * NUT);
    const int grid = std::min(tiles, dev.num_cus * blocks_per_cu);
    hipLaunchKernelGGL((topn_wide_kernel<real_t, NUT>), dim3(grid), dim3(TOPNW_TH), smem, dev.stream, P);
    return grid;
}

// Item slices of a full ranking: the user tiles of pick_user_tiles fill `tiles` of the device's
// num_cus * blocks_per_cu workgroup slots; while slots stay empty the items are cut so that tiles * slices fills them, but never
// into slices of fewer than TOPNSP_MIN_ROUNDS rounds of TOPNW_ITEMS items -- below that the slice pass costs what it saves (the
// user tile is loaded, every slice's list is written, merged and read again).  requested >= 1 asks for that many slices and is
// held to the rounds there are and to TOPNSP_MAX_SLICES.  The slices are equal but for the last: slice_items = rounds per slice
// * TOPNW_ITEMS, slices = what that leaves non-empty.
// PROVISIONAL: TOPNSP_MIN_ROUNDS and the use of every LDS-limited slot are to be set from tools/bench_topn_split.py's table.
constexpr long TOPNSP_MIN_ROUNDS = 4;

void plan_split(int nu, int n, int k, int n_top, int num_cus, size_t sizeof_real, int requested, int *slices, int *slice_items)
{
    const long rounds = std::max<long>(1, ((long)n + TOPNW_ITEMS - 1) / TOPNW_ITEMS);
    long want = requested;
    if (requested <= 0) {
        int bpc = 1;
        const int nut = pick_user_tiles(nu, k, n_top, num_cus, &bpc, 0, sizeof_real);
        const long tiles = ((long)nu + 16 * nut - 1) / (16 * nut), slots = (long)num_cus * bpc;
        want = tiles >= slots ? 1 : std::min(slots / tiles, std::max<long>(1, rounds / TOPNSP_MIN_ROUNDS));
    }
    want = std::max<long>(1, std::min<long>(want, std::min<long>(rounds, TOPNSP_MAX_SLICES)));
    const long per = (rounds + want - 1) / want;
    *slices = (int)((rounds + per - 1) / per);
    *slice_items = (int)std::min<long>(per * TOPNW_ITEMS, ((long)0x7fffffff / TOPNW_ITEMS) * TOPNW_ITEMS);
}

// the slice pass and the merge of a split ranking: P.out_ids / P.out_scores are the scratch, `out` the call's result
template <int NUT>
int launch_split(const cmfrec_hip_ranker::Device &dev, const TopnSplitParams<real_t> &P, int blocks_per_cu, int slices,
                 const TopnMergeParams<real_t> &M)
{
    const size_t smem = topnw_lds_bytes(NUT, P.k, P.n_top, sizeof(real_t));
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_split_kernel<real_t, NUT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = (P.nu + 16 * NUT - 1) / (16 * NUT);
    const int grid = std::min(tiles, dev.num_cus * blocks_per_cu);
    hipLaunchKernelGGL((topn_split_kernel<real_t, NUT>), dim3(grid, slices), dim3(TOPNW_TH), smem, dev.stream, P);
    HIP_CHECK(hipGetLastError());
    const int nw = topnsp_merge_waves(slices);
    hipLaunchKernelGGL(topn_split_merge_kernel<real_t>, dim3(P.nu), dim3(64 * nw), topnsp_merge_lds_bytes(nw, P.n_top, sizeof(real_t)),
                       dev.stream, M);
    return grid * slices;
}

template <int NUT, int METRIC>
int launch_similar(const cmfrec_hip_ranker::Device &dev, const TopnSimilarParams<real_t> &P, int blocks_per_cu)
{
    const size_t smem = topns_lds_bytes(NUT, P.k, P.n_top, sizeof(real_t));
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_similar_kernel<real_t, NUT, METRIC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = (P.nu + 16 * NUT - 1) / (16 * NUT);
    const int grid = std::min(tiles, dev.num_cus * blocks_per_cu);
    hipLaunchKernelGGL((topn_similar_kernel<real_t, NUT, METRIC>), dim3(grid), dim3(TOPNW_TH), smem, dev.stream, P);
    return grid;
}

template <int NUT>
int launch_after(const cmfrec_hip_ranker::Device &dev, const TopnAfterParams<real_t> &P, int blocks_per_cu)
{
    const size_t smem = topna_lds_bytes(NUT, P.k, P.n_top, sizeof(real_t));
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_after_kernel<real_t, NUT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = (P.nu + 16 * NUT - 1) / (16 * NUT);
    const int grid = std::min(tiles, dev.num_cus * blocks_per_cu);
    hipLaunchKernelGGL((topn_after_kernel<real_t, NUT>), dim3(grid), dim3(TOPNW_TH), smem, dev.stream, P);
    return grid;
}

template <int METRIC>
int launch_similar_tiles(const cmfrec_hip_ranker::Device &dev, const TopnSimilarParams<real_t> &P, int nut, int blocks_per_cu)
{
    switch (nut) {
    case 1: return launch_similar<1, METRIC>(dev, P, blocks_per_cu);
    case 2: return launch_similar<2, METRIC>(dev, P, blocks_per_cu);
    case 3: return launch_similar<3, METRIC>(dev, P, blocks_per_cu);
    default: return launch_similar<4, METRIC>(dev, P, blocks_per_cu);
    }
}

// the inverse norms of the ranker's rows, made on its stream the first time they are asked for (the caller holds the DeviceScope)
void ensure_inverse_norms(cmfrec_hip_ranker *r)
{
    if (r->has_rn) return;
    r->rn.alloc_at_least((size_t)r->n);
    const int rows = TOPNS_NORM_TH / 4;
    hipLaunchKernelGGL(row_rnorm_kernel<real_t>, dim3((unsigned)((r->n + rows - 1) / rows)), dim3(TOPNS_NORM_TH), 0, r->dev.stream, r->B.ptr,
                       r->ldb, r->n, (int)r->ldb, r->rn.ptr);
    HIP_CHECK(hipGetLastError());
    r->has_rn = true;
}

// User tiles per workgroup and slice length of the rank kernel (DESIGN.md "Ranks of held-out items"): the longest held-out list
// decides how many passes over the items a tile may need; per tile count the cost of a pass is pick_user_tiles' model.  Among
// the tile counts the one with the least passes x cost wins, the larger on a tie.  CMFREC_HIP_TOPN_TILES clamps the tiles,
// CMFREC_HIP_RANK_SLICE the slice (test hooks).  Returns 0 tiles when not even one threshold per user fits (cannot happen for
// k <= TOPNW_KMAX).
int pick_rank_shape(int nu, int k, size_t max_held, int num_cus, int *ts, int *tsp, int *blocks_per_cu)
{
    const int forced = switches().topn_tiles, slice = switches().rank_slice;
    int best = 0;
    double best_cost = 0;
    for (int nut = 1; nut <= TOPNW_MAX_NUT; nut++) {
        if (forced > 0 && nut > forced && best > 0) break;
        int cap = 0;                                                          // the largest padded slice that fits
        for (int p = 1; p <= TOPNR_TS_MAX && topnr_lds_bytes(nut, k, p, sizeof(real_t)) <= TOPNW_LDS_MAX; p <<= 1) cap = p;
        if (cap == 0) break;
        int s = cap;
        if (slice > 0) s = std::min(s, slice);
        const int need = (int)std::min<size_t>((size_t)s, std::max<size_t>(max_held, 1));
        const int pad = topnr_pow2(need);
        const size_t smem = topnr_lds_bytes(nut, k, pad, sizeof(real_t));
        const int bpc = (int)std::min<size_t>(TOPNW_LDS_MAX / smem, (size_t)(2048 / TOPNW_TH));
        const long tiles = ((long)nu + 16 * nut - 1) / (16 * nut), slots = (long)num_cus * bpc;
        const long share = std::min<long>(bpc, (tiles + num_cus - 1) / num_cus);
        const double passes = (double)((std::max<size_t>(max_held, 1) + s - 1) / s);
        const double cost = passes * (double)((tiles + slots - 1) / slots) * share * (nut + 0.5);
        if (best == 0 || (forced > 0 ? nut <= forced : cost <= best_cost)) { best = nut; best_cost = cost; *ts = need; *tsp = pad; *blocks_per_cu = bpc; }
    }
    return best;
}

template <int NUT>
int launch_rank(const cmfrec_hip_ranker::Device &dev, const TopnRankParams<real_t> &P, int blocks_per_cu)
{
    const size_t smem = topnr_lds_bytes(NUT, P.k, P.tsp, sizeof(real_t));
    HIP_CHECK(hipFuncSetAttribute((const void *)topn_rank_kernel<real_t, NUT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = (P.nu + 16 * NUT - 1) / (16 * NUT);
    const int grid = std::min(tiles, dev.num_cus * blocks_per_cu);
    hipLaunchKernelGGL((topn_rank_kernel<real_t, NUT>), dim3(grid), dim3(TOPNW_TH), smem, dev.stream, P);
    return grid;
}

int check_n_top(const char *fn, int_t n_top, int_t n)
{
    if (n_top > TOPN_NMAX || n_top > n) {
        g_last_error = std::string(fn) + ": " + LIMITS;
        return 2;
    }
    return 0;
}

// the ranking of nu users whose factors dA [nu, lda] and exclusion lists are on the device already: the launch, the timing
// events and the download of cmfrec_hip_ranker_topN (the caller holds the DeviceScope and has checked the limits)
// dcand_p != null: over each user's candidate list (device CSR) on topn_cand_kernel
int rank_device(cmfrec_hip_ranker *r, const real_t *dA, size_t lda, int_t nu, const size_t *dexcl_p, const int *dexcl_i, int_t n_top,
                int_t *out_ids, real_t *out_scores, const size_t *dcand_p = nullptr, const int *dcand_i = nullptr)
{
    const cmfrec_hip_ranker::Device &dev = r->dev;
    const int k = r->k;
    r->ids.alloc_at_least((size_t)nu * n_top);
    if (out_scores) r->sc.alloc_at_least((size_t)nu * n_top);
    if (dcand_p) {
        r->next.alloc_at_least(1);
        HIP_CHECK(hipMemsetAsync(r->next.ptr, 0, sizeof(unsigned), dev.stream));
    }
    // a split ranker: the full ranking of every k on the MFMA arithmetic, over as many item slices as the planner gives it
    const bool split = dcand_p == nullptr && r->split >= 0;
    int slices = 1, slice_items = 0;
    if (split) plan_split(nu, r->n, k, n_top, dev.num_cus, sizeof(real_t), r->split, &slices, &slice_items);
    if (slices > 1) {
        r->part_sc.alloc_at_least((size_t)slices * (size_t)nu * (size_t)n_top);
        r->part_id.alloc_at_least((size_t)slices * (size_t)nu * (size_t)n_top);
    }
    r->last_slices = slices;
    HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
    if (dcand_p) {
        TopnCandParams<real_t> P;
        P.A = dA; P.lda = lda; P.nu = nu; P.B = r->B.ptr; P.ldb = r->ldb; P.n = r->n; P.k = k;
        P.biasB = r->has_bias ? r->bias.ptr : nullptr;
        P.cand_p = dcand_p; P.cand_i = dcand_i;
        P.excl_p = dexcl_p; P.excl_i = dexcl_p ? dexcl_i : nullptr;
        P.n_top = n_top; P.out_ids = r->ids.ptr; P.out_scores = out_scores ? r->sc.ptr : nullptr;
        P.next = r->next.ptr; P.order = r->corder.ptr;
        r->last_grid = launch_topn_cand(dev.stream, dev.num_cus, P, switches().topn_cand_waves);
        r->last_users = TOPNC_NW;
    } else if (slices > 1) {
        TopnSplitParams<real_t> P;
        P.A = dA; P.lda = lda; P.nu = nu; P.B = r->B.ptr; P.ldb = r->ldb; P.n = r->n; P.k = k;
        P.biasB = r->has_bias ? r->bias.ptr : nullptr;
        P.excl_p = dexcl_p; P.excl_i = dexcl_p ? dexcl_i : nullptr;
        P.n_top = n_top; P.out_ids = r->part_id.ptr; P.out_scores = r->part_sc.ptr;
        P.slice_items = slice_items; P.s0 = P.s1 = 0;
        TopnMergeParams<real_t> M;
        M.part_scores = r->part_sc.ptr; M.part_ids = r->part_id.ptr; M.slices = slices; M.nu = nu; M.n_top = n_top;
        M.out_ids = r->ids.ptr; M.out_scores = out_scores ? r->sc.ptr : nullptr;
        int bpc = 1;
        const int nut = pick_user_tiles(nu, k, n_top, dev.num_cus, &bpc);
        switch (nut) {
        case 1: r->last_grid = launch_split<1>(dev, P, bpc, slices, M); break;
        case 2: r->last_grid = launch_split<2>(dev, P, bpc, slices, M); break;
        case 3: r->last_grid = launch_split<3>(dev, P, bpc, slices, M); break;
        default: r->last_grid = launch_split<4>(dev, P, bpc, slices, M); break;
        }
        r->last_users = 16 * nut;
    } else if (k <= TOPN_KMAX && !switches().topn_wide && !split) {
        TopnParams<real_t> P;
        P.A = dA; P.lda = lda; P.nu = nu; P.B = r->B.ptr; P.ldb = r->ldb; P.n = r->n; P.k = k;
        P.biasB = r->has_bias ? r->bias.ptr : nullptr;
        P.excl_p = dexcl_p; P.excl_i = dexcl_p ? dexcl_i : nullptr;
        P.n_top = n_top; P.out_ids = r->ids.ptr; P.out_scores = out_scores ? r->sc.ptr : nullptr;
        const size_t smem = topn_lds_bytes(sizeof(real_t));
        HIP_CHECK(hipFuncSetAttribute((const void *)topn_kernel<real_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        const int tiles = (nu + TOPN_UT - 1) / TOPN_UT;
        hipLaunchKernelGGL(topn_kernel<real_t>, dim3(std::min(tiles, dev.num_cus * 2)), dim3(TOPN_TH), smem, dev.stream, P);
        r->last_users = TOPN_UT; r->last_grid = std::min(tiles, dev.num_cus * 2);
    } else {
        TopnWideParams<real_t> P;
        P.A = dA; P.lda = lda; P.nu = nu; P.B = r->B.ptr; P.ldb = r->ldb; P.n = r->n; P.k = k;
        P.biasB = r->has_bias ? r->bias.ptr : nullptr;
        P.excl_p = dexcl_p; P.excl_i = dexcl_p ? dexcl_i : nullptr;
        P.n_top = n_top; P.out_ids = r->ids.ptr; P.out_scores = out_scores ? r->sc.ptr : nullptr;
        int bpc = 1;
        const int nut = pick_user_tiles(nu, k, n_top, dev.num_cus, &bpc);
        switch (nut) {
        case 1: r->last_grid = launch_wide<1>(dev, P, bpc); break;
        case 2: r->last_grid = launch_wide<2>(dev, P, bpc); break;
        case 3: r->last_grid = launch_wide<3>(dev, P, bpc); break;
        default: r->last_grid = launch_wide<4>(dev, P, bpc); break;
        }
        r->last_users = 16 * nut;
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(r->ev1, dev.stream));
    r->timed = true;
    r->ids.download(out_ids, (size_t)nu * n_top, dev.stream);
    if (out_scores) r->sc.download(out_scores, (size_t)nu * n_top, dev.stream);
    HIP_CHECK(hipStreamSynchronize(dev.stream));
    return 0;
}

// Page length of a deep list (DESIGN.md "Deep lists and next pages"): 128, the list size the wide kernel has been measured at,
// and longer only where a longer page was measured at least 10 % faster at n_top = 500 and 1000 -- double precision 256 around
// k = 128 and 512 around k = 256, single precision 256 around k = 272; the ranges' ends lie midway between the measured widths.
// A list that one page of 128 holds runs as that page.  CMFREC_HIP_TOPN_PAGE (test hook, 1 .. TOPNA_PAGE_MAX, read per call) asks
// for any other length; the length is cut down to what one user tile fits beside the factors.  The result does not depend on it.
int default_page_len(int k)
{
    if (sizeof(real_t) == 8) return k >= 192 ? 512 : (k >= 96 ? 256 : 128);
    return k >= 192 ? 256 : 128;
}

int pick_page_len(int k, int_t n_top)
{
    const char *v = getenv("CMFREC_HIP_TOPN_PAGE");
    const int asked = (v != nullptr && v[0] != 0) ? atoi(v) : 0;
    int len = (asked >= 1 && asked <= TOPNA_PAGE_MAX) ? asked : (n_top <= 128 ? 128 : default_page_len(k));
    while (len > 32 && topna_lds_bytes(1, k, len, sizeof(real_t)) > TOPNW_LDS_MAX) len = topnw_np(len) / 2;
    return (int)std::min<int_t>(len, n_top);
}

// The n_top best of nu users behind their cursors, in pages of page_len on topn_after_kernel, for every k (the register-resident
// topn_kernel of k <= 64 rounds otherwise, and a cursor compares bits).  The whole [nu, n_top] result lives in r->ids / r->sc;
// page p is one launch that writes the columns [p * page_len, ...) and reads its cursors from the column in front of them -- no
// host round trip between the pages, one download at the end.  The first page's cursors: dcur_s / dcur_i [nu], or null (every
// user starts at the top).  The timing events enclose all the pages.  Returns the launches in *pages.
// (the caller holds the DeviceScope and has checked the limits; the factors and exclusion lists are on the device)
int rank_device_deep(cmfrec_hip_ranker *r, const real_t *dA, size_t lda, int_t nu, const size_t *dexcl_p, const int *dexcl_i, int_t n_top,
                     int page_len, const real_t *dcur_s, const int *dcur_i, int_t *out_ids, real_t *out_scores, int *pages)
{
    const cmfrec_hip_ranker::Device &dev = r->dev;
    const size_t cells = (size_t)nu * (size_t)n_top;
    r->ids.alloc_at_least(cells);
    r->sc.alloc_at_least(cells);                                         // (the next page's cursors, wanted by the caller or not)
    TopnAfterParams<real_t> P;
    P.A = dA; P.lda = lda; P.nu = nu; P.B = r->B.ptr; P.ldb = r->ldb; P.n = r->n; P.k = r->k;
    P.biasB = r->has_bias ? r->bias.ptr : nullptr;
    P.excl_p = dexcl_p; P.excl_i = dexcl_p ? dexcl_i : nullptr;
    P.out_ld = (size_t)n_top;
    poison_lds(dev.stream, dev.num_cus);                                 // (the policy's LDS too is written before it is read)
    HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
    int launches = 0;
    for (int_t first = 0; first < n_top; first += page_len, launches++) {
        P.n_top = (int)std::min<int_t>(page_len, n_top - first);
        P.out_ids = r->ids.ptr + first; P.out_scores = r->sc.ptr + first;
        if (first == 0) { P.cur_scores = dcur_s; P.cur_ids = dcur_s ? dcur_i : nullptr; P.cur_ld = 1; }
        else { P.cur_scores = r->sc.ptr + first - 1; P.cur_ids = r->ids.ptr + first - 1; P.cur_ld = (size_t)n_top; }
        int bpc = 1;
        const int nut = pick_user_tiles(nu, r->k, P.n_top, dev.num_cus, &bpc, topna_extra_bytes(sizeof(real_t)));
        switch (nut) {
        case 1: r->last_grid = launch_after<1>(dev, P, bpc); break;
        case 2: r->last_grid = launch_after<2>(dev, P, bpc); break;
        case 3: r->last_grid = launch_after<3>(dev, P, bpc); break;
        default: r->last_grid = launch_after<4>(dev, P, bpc); break;
        }
        r->last_users = 16 * nut;
        HIP_CHECK(hipGetLastError());
    }
    HIP_CHECK(hipEventRecord(r->ev1, dev.stream));
    r->timed = true;
    r->last_slices = 1;
    r->ids.download(out_ids, cells, dev.stream);
    if (out_scores) r->sc.download(out_scores, cells, dev.stream);
    HIP_CHECK(hipStreamSynchronize(dev.stream));
    if (pages) *pages = launches;
    return 0;
}

// the candidate lists of a call (host CSR over the nu users) into the ranker's buffers; 2 with a message for lists that are not a CSR
int upload_candidates(cmfrec_hip_ranker *r, const char *fn, int_t nu, const size_t cand_p[], const int_t cand_i[])
{
    bool bad = cand_p == nullptr;
    for (int_t u = 0; !bad && u < nu; u++) bad = cand_p[u] > cand_p[u + 1];
    if (bad || (cand_p[nu] > 0 && cand_i == nullptr)) {
        g_last_error = std::string(fn) + ": invalid arguments";
        return 2;
    }
    // the order the kernel hands the users out in: longest list first (a long list that starts last is the launch's tail)
    std::vector<int> order((size_t)nu);
    for (int_t u = 0; u < nu; u++) order[u] = u;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cand_p[a + 1] - cand_p[a] > cand_p[b + 1] - cand_p[b]; });
    r->corder.upload(order.data(), (size_t)nu, r->dev.stream);
    HIP_CHECK(hipStreamSynchronize(r->dev.stream));          // `order` goes away
    r->cp.upload(cand_p, (size_t)nu + 1, r->dev.stream);
    r->ci.alloc_at_least(std::max<size_t>(cand_p[nu], 1));
    if (cand_p[nu] > 0) r->ci.upload(cand_i, cand_p[nu], r->dev.stream);
    return 0;
}

// the held-out lists of a call (host CSR over the nu users) into the ranker's buffers; 2 with a message for lists that are not a
// CSR; *max_held = the longest list
int upload_held(cmfrec_hip_ranker *r, const char *fn, int_t nu, const size_t held_p[], const int_t held_i[], size_t *max_held)
{
    bool bad = held_p == nullptr;
    size_t longest = 0;
    for (int_t u = 0; !bad && u < nu; u++) {
        bad = held_p[u] > held_p[u + 1];
        if (!bad) longest = std::max(longest, held_p[u + 1] - held_p[u]);
    }
    if (bad || longest > (size_t)0x7fffffff || (held_p[nu] > held_p[0] && held_i == nullptr)) {
        g_last_error = std::string(fn) + ": invalid arguments";
        return 2;
    }
    r->cp.upload(held_p, (size_t)nu + 1, r->dev.stream);
    r->ci.alloc_at_least(std::max<size_t>(held_p[nu], 1));
    if (held_p[nu] > 0) r->ci.upload(held_i, held_p[nu], r->dev.stream);
    *max_held = longest;
    return 0;
}

// the ranks of nu users whose factors dA [nu, lda], held-out lists (r->cp / r->ci, total entries) and exclusion lists are on the
// device: the launch, the timing events (around topn_rank_kernel, whose threshold and exclusion steps are part of it) and the
// download.  Nothing is written to the outputs before the kernel has run.
// dheld_p / dheld_i: the held-out lists where they are (null: the ranker's own r->cp / r->ci, filled by upload_held).  stay: the
// ranks and the pool stay on the device (r->ids, r->pool) for rank_metrics_kernel behind the launch; nothing is downloaded and
// the stream is not waited for.
int ranks_device(cmfrec_hip_ranker *r, const real_t *dA, size_t lda, int_t nu, size_t total, size_t max_held, const size_t *dexcl_p,
                 const int *dexcl_i, int_t *out_rank, real_t *out_scores, int_t *out_pool, const size_t *dheld_p = nullptr,
                 const int *dheld_i = nullptr, bool stay = false)
{
    const cmfrec_hip_ranker::Device &dev = r->dev;
    r->ids.alloc_at_least(std::max<size_t>(total, 1));
    if (out_scores) r->sc.alloc_at_least(std::max<size_t>(total, 1));
    if (out_pool || stay) r->pool.alloc_at_least((size_t)nu);
    TopnRankParams<real_t> P;
    P.A = dA; P.lda = lda; P.nu = nu; P.B = r->B.ptr; P.ldb = r->ldb; P.n = r->n; P.k = r->k;
    P.biasB = r->has_bias ? r->bias.ptr : nullptr;
    P.held_p = dheld_p ? dheld_p : r->cp.ptr; P.held_i = dheld_p ? dheld_i : r->ci.ptr;
    P.excl_p = dexcl_p; P.excl_i = dexcl_p ? dexcl_i : nullptr;
    P.out_rank = r->ids.ptr; P.out_scores = out_scores ? r->sc.ptr : nullptr; P.out_pool = (out_pool || stay) ? r->pool.ptr : nullptr;
    int bpc = 1;
    const int nut = pick_rank_shape(nu, r->k, max_held, dev.num_cus, &P.ts, &P.tsp, &bpc);
    if (nut == 0) {
        g_last_error = "cmfrec_hip_ranker_ranks: the model does not fit the rank kernel's LDS";
        return 2;
    }
    HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
    switch (nut) {
    case 1: r->last_grid = launch_rank<1>(dev, P, bpc); break;
    case 2: r->last_grid = launch_rank<2>(dev, P, bpc); break;
    case 3: r->last_grid = launch_rank<3>(dev, P, bpc); break;
    default: r->last_grid = launch_rank<4>(dev, P, bpc); break;
    }
    r->last_users = 16 * nut;
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(r->ev1, dev.stream));
    r->timed = true;
    r->last_slices = 1;
    if (stay) return 0;
    r->ids.download(out_rank, total, dev.stream);
    if (out_scores) r->sc.download(out_scores, total, dev.stream);
    if (out_pool) r->pool.download(out_pool, (size_t)nu, dev.stream);
    HIP_CHECK(hipStreamSynchronize(dev.stream));
    return 0;
}

}  // namespace

// a ranking set resident on the device: user ids, held-out lists, exclusion lists; and what its evaluations need beside them --
// the two NDCG tables of the last cut-off, the gathered rows of the users, the per-user values, the wavefronts' records
struct cmfrec_hip_rankset {
    int device = 0, num_cus = 256;
    hipStream_t stream = nullptr;              // the uploads; an evaluation runs on the ranker's stream
    int nu = 0;
    size_t total = 0, max_held = 0;
    bool has_excl = false;
    std::vector<int> users_host, held_host, excl_host;     // host copies: the gather of cmfrec_hip_ranker_metrics, rankset_usable
    std::vector<size_t> held_p_host, excl_p_host;
    int max_user = -1;
    DevBuf<int> users, held_i, excl_i;
    DevBuf<size_t> held_p, excl_p;
    int table_k = 0;                           // the cut-off disc / ideal were made for (0: none yet)
    DevBuf<double> disc, ideal, per_user;
    DevBuf<real_t> A;                          // [nu, k] rows of the set's users
    DevBuf<cmfrec_hip_rank_record> partials;
    ~cmfrec_hip_rankset() { if (stream) (void)hipStreamDestroy(stream); }
};

namespace cmfhip {

// The metrics of a set whose users' factors dA [nu, lda] are on the device, on the ranker's stream: the rank kernel, then the
// reduction; one synchronisation.  per_user [nu, 8] / out_rank [total]: optional host outputs.
int rankset_run(cmfrec_hip_ranker *r, cmfrec_hip_rankset *set, const char *fn, const real_t *dA, size_t lda, int k_at,
                cmfrec_hip_rank_record *out, double *per_user, int_t *out_rank)
{
    if (r == nullptr || set == nullptr || out == nullptr || dA == nullptr || k_at < 1 || lda < (size_t)r->k) {
        g_last_error = std::string(fn) + ": invalid arguments";
        return 2;
    }
    if (set->device != r->dev.device) {
        g_last_error = std::string(fn) + ": the ranking set lives on device " + std::to_string(set->device) + ", the items on device " +
                       std::to_string(r->dev.device);
        return 2;
    }
    DeviceScope scope(r->dev.device);
    switches_mut().reload();
    hipStream_t st = r->dev.stream;
    memset(out, 0, sizeof *out);
    if (set->nu == 0) return 0;
    if (set->table_k != k_at) {
        // the discounts and the ideal sums as NumPy forms them: 1 / log2(j + 1) for j = 1 .. k, and their running sums
        std::vector<double> disc((size_t)k_at), ideal((size_t)k_at + 1, 0.0);
        for (int j = 1; j <= k_at; j++) { disc[j - 1] = 1.0 / std::log2((double)j + 1.0); ideal[j] = ideal[j - 1] + disc[j - 1]; }
        set->disc.upload(disc.data(), disc.size(), st);
        set->ideal.upload(ideal.data(), ideal.size(), st);
        HIP_CHECK(hipStreamSynchronize(st));                 // the vectors go away
        set->table_k = k_at;
    }
    if (int rc = ranks_device(r, dA, lda, set->nu, set->total, set->max_held, set->has_excl ? set->excl_p.ptr : nullptr,
                              set->has_excl ? set->excl_i.ptr : nullptr, nullptr, nullptr, nullptr, set->held_p.ptr, set->held_i.ptr, true))
        return rc;
    const char *cap = getenv("CMFREC_HIP_RANKMETRIC_WAVES");            // test hook, read per call
    const int max_waves = (cap != nullptr && cap[0] != 0) ? atoi(cap) : 0;
    const size_t waves = rank_metrics_waves(set->nu, r->dev.num_cus, max_waves);
    set->partials.alloc_at_least(waves + 1);
    if (per_user) set->per_user.alloc_at_least((size_t)set->nu * RANKM_METRICS);
    RankMetricParams P;
    P.ranks = r->ids.ptr; P.pool = r->pool.ptr; P.held_p = set->held_p.ptr; P.nu = set->nu; P.k_at = k_at;
    P.disc = set->disc.ptr; P.ideal = set->ideal.ptr; P.per_user = per_user ? set->per_user.ptr : nullptr; P.partials = set->partials.ptr;
    launch_rank_metrics(st, waves, P);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out, set->partials.ptr + waves, sizeof *out, hipMemcpyDeviceToHost, st));
    if (per_user) set->per_user.download(per_user, (size_t)set->nu * RANKM_METRICS, st);
    if (out_rank && set->total > 0) r->ids.download(out_rank, set->total, st);
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// dst [nu, k] = the rows users[0 .. nu) of src [., lds], columns [0, k)
__global__ void gather_user_rows_kernel(real_t *__restrict__ dst, const real_t *__restrict__ src, size_t lds, const int *__restrict__ users,
                                        int nu, int k)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nu * (size_t)k) return;
    const size_t u = i / (size_t)k, c = i % (size_t)k;
    dst[i] = src[(size_t)users[u] * lds + c];
}

// what a fit asks of the set it is to watch before it writes anything (cmfrec_hip_fit_set_monitor): the set lives on `device`
// (< 0: the current one), kk fits the rank kernel, every user is a row of A, and at least one user has a held-out item inside
// [0, n) that its exclusion list does not take away (T > 0) -- from the set's host copies.  0, or 2 with fn's name in the message.
int rankset_usable(cmfrec_hip_rankset *set, const char *fn, int device, int_t m, int_t n, int_t kk, int k_at)
{
    if (set == nullptr || k_at < 1) {
        g_last_error = std::string(fn) + ": the monitor needs a ranking set and k_at >= 1";
        return 2;
    }
    if (device < 0) HIP_CHECK(hipGetDevice(&device));
    if (set->device != device) {
        g_last_error = std::string(fn) + ": the ranking set lives on device " + std::to_string(set->device) + ", the fit runs on device " +
                       std::to_string(device);
        return 2;
    }
    if (kk > TOPNW_KMAX) {
        g_last_error = std::string(fn) + ": a ranking watch " + RANK_LIMITS + " (k + k_main)";
        return 2;
    }
    if (set->max_user >= m) {
        g_last_error = std::string(fn) + ": the ranking set names user " + std::to_string(set->max_user) + ", X has " + std::to_string(m) + " rows";
        return 2;
    }
    for (int u = 0; u < set->nu; u++)
        for (size_t e = set->held_p_host[u]; e < set->held_p_host[u + 1]; e++) {
            const int item = set->held_host[e];
            if (item < 0 || item >= n) continue;
            if (set->has_excl && std::binary_search(set->excl_host.begin() + set->excl_p_host[u], set->excl_host.begin() + set->excl_p_host[u + 1], item))
                continue;
            return 0;
        }
    g_last_error = std::string(fn) + ": no user of the ranking set has a held-out item that can be ranked: nothing to watch";
    return 2;
}

// The metrics of a set against factors that are on the device (cmfrec_hip_session_ranking): A [m, ldA] and B [n, ldB] point at the
// first ranked column, kk wide.  *owned: a ranker the caller keeps between calls -- made from B on the first call, refreshed
// from B on every later one by a device-to-device column copy into its padded layout (topnw_kp), no host round trip.  The users'
// rows are gathered on the device.  The caller has synchronised the stream that wrote the factors.
int rankset_run_on_factors(cmfrec_hip_ranker **owned, cmfrec_hip_rankset *set, const char *fn, int device, const real_t *dA, size_t ldA, int_t m,
                           const real_t *dB, size_t ldB, int_t n, int_t kk, const real_t *dbiasB, int k_at, cmfrec_hip_rank_record *out)
{
    if (owned == nullptr || set == nullptr || out == nullptr || k_at < 1) {
        g_last_error = std::string(fn) + ": invalid arguments";
        return 2;
    }
    if (kk > TOPNW_KMAX) {
        g_last_error = std::string(fn) + ": " + RANK_LIMITS;
        return 2;
    }
    if (set->device != device) {
        g_last_error = std::string(fn) + ": the ranking set lives on device " + std::to_string(set->device) + ", the factors on device " +
                       std::to_string(device);
        return 2;
    }
    if (set->max_user >= m) {
        g_last_error = std::string(fn) + ": the ranking set names user " + std::to_string(set->max_user) + ", A has " + std::to_string(m) + " rows";
        return 2;
    }
    cmfrec_hip_ranker *r = *owned;
    if (r == nullptr) {
        r = *owned = cmfrec_hip_ranker_create(dB, ldB, n, kk, dbiasB, device);
        if (r == nullptr) return g_last_rc ? g_last_rc : 4;
    } else {
        DeviceScope scope(device);
        upload_columns(r->B.ptr, r->ldb, dB, ldB, (size_t)n, (size_t)kk, r->dev.stream);
        r->has_rn = false;                                   // (norms of the rows that were)
        if (dbiasB) r->bias.upload(dbiasB, (size_t)n, r->dev.stream);
    }
    memset(out, 0, sizeof *out);
    if (set->nu == 0) return 0;
    DeviceScope scope(device);
    set->A.alloc_at_least((size_t)set->nu * (size_t)kk);
    const size_t cells = (size_t)set->nu * (size_t)kk;
    hipLaunchKernelGGL(gather_user_rows_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, r->dev.stream, set->A.ptr, dA, ldA,
                       set->users.ptr, set->nu, (int)kk);
    HIP_CHECK(hipGetLastError());
    return rankset_run(r, set, fn, set->A.ptr, (size_t)kk, k_at, out, nullptr, nullptr);
}

}  // namespace cmfhip

static_assert(TOPNC_KMAX == TOPNW_KMAX, "topn_cand_kernel holds a user's row of the widest model in registers");

extern "C" {

cmfrec_hip_ranker *cmfrec_hip_ranker_create(const real_t *B, size_t ldb, int_t n, int_t k, const real_t *biasB, int device)
{
    cmfrec_hip_ranker *r = nullptr;
    const int rc = guarded([&]() {
        if (B == nullptr || n <= 0 || k <= 0 || ldb < (size_t)k) {
            g_last_error = "cmfrec_hip_ranker_create: invalid arguments";
            return 2;
        }
        if (k > TOPNW_KMAX) {
            g_last_error = std::string("cmfrec_hip_ranker_create: ") + LIMITS;
            return 2;
        }
        r = new cmfrec_hip_ranker();
        open_device(device, &r->dev.device, &r->dev.num_cus, &r->dev.stream);
        r->n = n; r->k = k; r->ldb = (size_t)topnw_kp(k, sizeof(real_t));
        r->B.alloc((size_t)n * r->ldb);
        if (r->ldb != (size_t)k) HIP_CHECK(hipMemsetAsync(r->B.ptr, 0, r->B.n * sizeof(real_t), r->dev.stream));
        upload_columns(r->B.ptr, r->ldb, B, ldb, (size_t)n, (size_t)k, r->dev.stream);
        r->has_bias = biasB != nullptr;
        if (biasB) r->bias.upload(biasB, (size_t)n, r->dev.stream);
        HIP_CHECK(hipEventCreate(&r->ev0));
        HIP_CHECK(hipEventCreate(&r->ev1));
        HIP_CHECK(hipStreamSynchronize(r->dev.stream));      // the caller's B may go away
        return 0;
    });
    g_last_rc = rc;
    if (rc != 0) {
        delete r;
        return nullptr;
    }
    return r;
}

int cmfrec_hip_ranker_topN(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t excl_p[], const int_t excl_i[],
                           int_t n_top, int_t *out_ids, real_t *out_scores)
{
    return guarded([&]() {
        if (r == nullptr || nu <= 0 || n_top <= 0 || !A || !out_ids || lda < (size_t)r->k || (excl_p != nullptr && excl_i == nullptr && excl_p[nu] > 0)) {
            g_last_error = "cmfrec_hip_ranker_topN: invalid arguments";
            return 2;
        }
        if (int rc = check_n_top("cmfrec_hip_ranker_topN", n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        const cmfrec_hip_ranker::Device &dev = r->dev;
        const int k = r->k;
        r->A.alloc_at_least((size_t)nu * k);
        upload_columns(r->A.ptr, (size_t)k, A, lda, (size_t)nu, (size_t)k, dev.stream);
        if (excl_p) {
            r->ep.upload(excl_p, (size_t)nu + 1, dev.stream);
            r->ei.alloc_at_least(std::max<size_t>(excl_p[nu], 1));
            if (excl_p[nu] > 0) r->ei.upload(excl_i, excl_p[nu], dev.stream);
        }
        return rank_device(r, r->A.ptr, (size_t)k, nu, excl_p ? r->ep.ptr : nullptr, excl_p ? r->ei.ptr : nullptr, n_top, out_ids, out_scores);
    });
}

int cmfrec_hip_ranker_topN_candidates(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t cand_p[], const int_t cand_i[],
                                      const size_t excl_p[], const int_t excl_i[], int_t n_top, int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_ranker_topN_candidates";
    return guarded([&]() {
        if (r == nullptr || nu <= 0 || n_top <= 0 || !A || !out_ids || !cand_p || lda < (size_t)r->k ||
            (excl_p != nullptr && excl_i == nullptr && excl_p[nu] > 0)) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        const cmfrec_hip_ranker::Device &dev = r->dev;
        const int k = r->k;
        if (int rc = upload_candidates(r, fn, nu, cand_p, cand_i)) return rc;
        r->A.alloc_at_least((size_t)nu * k);
        upload_columns(r->A.ptr, (size_t)k, A, lda, (size_t)nu, (size_t)k, dev.stream);
        if (excl_p) {
            r->ep.upload(excl_p, (size_t)nu + 1, dev.stream);
            r->ei.alloc_at_least(std::max<size_t>(excl_p[nu], 1));
            if (excl_p[nu] > 0) r->ei.upload(excl_i, excl_p[nu], dev.stream);
        }
        return rank_device(r, r->A.ptr, (size_t)k, nu, excl_p ? r->ep.ptr : nullptr, excl_p ? r->ei.ptr : nullptr, n_top, out_ids, out_scores,
                           r->cp.ptr, r->ci.ptr);
    });
}

int cmfrec_hip_ranker_topN_deep(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t excl_p[], const int_t excl_i[],
                                int_t n_top, int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_ranker_topN_deep";
    return guarded([&]() {
        if (r != nullptr && (n_top < 1 || n_top > r->n)) {
            g_last_error = std::string(fn) + ": " + DEEP_LIMITS;
            return 2;
        }
        if (r == nullptr || nu <= 0 || !A || !out_ids || lda < (size_t)r->k || (excl_p != nullptr && excl_i == nullptr && excl_p[nu] > 0)) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        const cmfrec_hip_ranker::Device &dev = r->dev;
        const int k = r->k;
        r->A.alloc_at_least((size_t)nu * k);
        upload_columns(r->A.ptr, (size_t)k, A, lda, (size_t)nu, (size_t)k, dev.stream);
        if (excl_p) {
            r->ep.upload(excl_p, (size_t)nu + 1, dev.stream);
            r->ei.alloc_at_least(std::max<size_t>(excl_p[nu], 1));
            if (excl_p[nu] > 0) r->ei.upload(excl_i, excl_p[nu], dev.stream);
        }
        const int len = pick_page_len(k, n_top);
        int pages = 0;
        if (int rc = rank_device_deep(r, r->A.ptr, (size_t)k, nu, excl_p ? r->ep.ptr : nullptr, excl_p ? r->ei.ptr : nullptr, n_top, len, nullptr,
                                      nullptr, out_ids, out_scores, &pages))
            return rc;
        r->last_pages = pages; r->last_page_len = len;
        return 0;
    });
}

int cmfrec_hip_ranker_topN_after(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t excl_p[], const int_t excl_i[],
                                 const int_t *after_ids, const real_t *after_scores, int_t n_top, int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_ranker_topN_after";
    return guarded([&]() {
        if (r == nullptr || nu <= 0 || n_top <= 0 || !A || !out_ids || lda < (size_t)r->k || (after_ids == nullptr) != (after_scores == nullptr) ||
            (excl_p != nullptr && excl_i == nullptr && excl_p[nu] > 0)) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        const cmfrec_hip_ranker::Device &dev = r->dev;
        const int k = r->k;
        r->A.alloc_at_least((size_t)nu * k);
        upload_columns(r->A.ptr, (size_t)k, A, lda, (size_t)nu, (size_t)k, dev.stream);
        if (excl_p) {
            r->ep.upload(excl_p, (size_t)nu + 1, dev.stream);
            r->ei.alloc_at_least(std::max<size_t>(excl_p[nu], 1));
            if (excl_p[nu] > 0) r->ei.upload(excl_i, excl_p[nu], dev.stream);
        }
        if (after_ids) {
            r->cur_s.upload(after_scores, (size_t)nu, dev.stream);
            r->cur_i.upload(after_ids, (size_t)nu, dev.stream);
        }
        return rank_device_deep(r, r->A.ptr, (size_t)k, nu, excl_p ? r->ep.ptr : nullptr, excl_p ? r->ei.ptr : nullptr, n_top, (int)n_top,
                                after_ids ? r->cur_s.ptr : nullptr, after_ids ? r->cur_i.ptr : nullptr, out_ids, out_scores, nullptr);
    });
}

int cmfrec_hip_ranker_pages(cmfrec_hip_ranker *r, int *pages, int *page_len)
{
    if (r == nullptr || r->last_pages == 0) {
        g_last_error = "cmfrec_hip_ranker_pages: no deep ranking call on this handle yet";
        return 2;
    }
    if (pages) *pages = r->last_pages;
    if (page_len) *page_len = r->last_page_len;
    return 0;
}

int cmfrec_hip_ranker_ranks(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t held_p[], const int_t held_i[],
                            const size_t excl_p[], const int_t excl_i[], int_t *out_rank, real_t *out_scores, int_t *out_pool)
{
    const char *fn = "cmfrec_hip_ranker_ranks";
    return guarded([&]() {
        if (r == nullptr || nu <= 0 || !A || !held_p || lda < (size_t)r->k || (held_p[nu] > 0 && !out_rank) ||
            (excl_p != nullptr && excl_i == nullptr && excl_p[nu] > 0)) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        const cmfrec_hip_ranker::Device &dev = r->dev;
        const int k = r->k;
        size_t max_held = 0;
        if (int rc = upload_held(r, fn, nu, held_p, held_i, &max_held)) return rc;
        r->A.alloc_at_least((size_t)nu * k);
        upload_columns(r->A.ptr, (size_t)k, A, lda, (size_t)nu, (size_t)k, dev.stream);
        if (excl_p) {
            r->ep.upload(excl_p, (size_t)nu + 1, dev.stream);
            r->ei.alloc_at_least(std::max<size_t>(excl_p[nu], 1));
            if (excl_p[nu] > 0) r->ei.upload(excl_i, excl_p[nu], dev.stream);
        }
        return ranks_device(r, r->A.ptr, (size_t)k, nu, held_p[nu], max_held, excl_p ? r->ep.ptr : nullptr, excl_p ? r->ei.ptr : nullptr,
                            out_rank, out_scores, out_pool);
    });
}

cmfrec_hip_rankset *cmfrec_hip_rankset_create(const int_t *users, int_t nu, const size_t *held_p, const int_t *held_i,
                                              const size_t *excl_p, const int_t *excl_i, int device)
{
    const char *fn = "cmfrec_hip_rankset_create";
    cmfrec_hip_rankset *set = nullptr;
    const int rc = guarded([&]() {
        bool bad = nu < 0 || (nu > 0 && (users == nullptr || held_p == nullptr));
        size_t longest = 0;
        int max_user = -1;
        for (int_t u = 0; !bad && u < nu; u++) {
            bad = users[u] < 0 || held_p[u] > held_p[u + 1] || (excl_p != nullptr && excl_p[u] > excl_p[u + 1]);
            if (!bad) { longest = std::max(longest, held_p[u + 1] - held_p[u]); max_user = std::max(max_user, (int)users[u]); }
        }
        if (!bad && nu > 0)
            bad = held_p[0] != 0 || longest > (size_t)0x7fffffff || (held_p[nu] > 0 && held_i == nullptr) ||
                  (excl_p != nullptr && (excl_p[0] != 0 || (excl_p[nu] > 0 && excl_i == nullptr)));
        if (bad) {
            g_last_error = std::string(fn) + ": invalid arguments (user ids >= 0; held-out and exclusion lists a CSR over the users)";
            return 2;
        }
        set = new cmfrec_hip_rankset();
        open_device(device, &set->device, &set->num_cus, &set->stream);
        set->nu = nu; set->max_held = longest; set->max_user = max_user;
        if (nu == 0) return 0;
        set->total = held_p[nu];
        set->users_host.assign(users, users + nu);
        set->held_p_host.assign(held_p, held_p + nu + 1);
        if (set->total > 0) set->held_host.assign(held_i, held_i + set->total);
        if (excl_p) {
            set->excl_p_host.assign(excl_p, excl_p + nu + 1);
            if (excl_p[nu] > 0) set->excl_host.assign(excl_i, excl_i + excl_p[nu]);
        }
        set->users.upload(set->users_host.data(), (size_t)nu, set->stream);
        set->held_p.upload(held_p, (size_t)nu + 1, set->stream);
        set->held_i.alloc(std::max<size_t>(set->total, 1));
        if (set->total > 0) set->held_i.upload(held_i, set->total, set->stream);
        set->has_excl = excl_p != nullptr;
        if (excl_p) {
            set->excl_p.upload(excl_p, (size_t)nu + 1, set->stream);
            set->excl_i.alloc(std::max<size_t>(excl_p[nu], 1));
            if (excl_p[nu] > 0) set->excl_i.upload(excl_i, excl_p[nu], set->stream);
        }
        HIP_CHECK(hipStreamSynchronize(set->stream));        // the caller's arrays may go away
        return 0;
    });
    g_last_rc = rc;
    if (rc != 0) {
        delete set;
        return nullptr;
    }
    return set;
}

void cmfrec_hip_rankset_destroy(cmfrec_hip_rankset *set)
{
    if (set == nullptr) return;
    (void)hipSetDevice(set->device);
    delete set;
}

int cmfrec_hip_ranker_metrics(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t m, cmfrec_hip_rankset *set, int k_at,
                              cmfrec_hip_rank_record *out, double *per_user, int_t *out_rank)
{
    const char *fn = "cmfrec_hip_ranker_metrics";
    return guarded([&]() {
        if (r == nullptr || set == nullptr || A == nullptr || out == nullptr || k_at < 1 || lda < (size_t)r->k) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        if (set->max_user >= m) {
            g_last_error = std::string(fn) + ": the ranking set names user " + std::to_string(set->max_user) + ", A has " + std::to_string(m) + " rows";
            return 2;
        }
        if (set->device != r->dev.device) return rankset_run(r, set, fn, A, lda, k_at, out, per_user, out_rank);   // (refused there)
        DeviceScope scope(r->dev.device);
        const size_t k = (size_t)r->k;
        std::vector<real_t> rows((size_t)set->nu * k);
        for (int u = 0; u < set->nu; u++) memcpy(rows.data() + (size_t)u * k, A + (size_t)set->users_host[u] * lda, k * sizeof(real_t));
        set->A.alloc_at_least(std::max<size_t>(rows.size(), 1));
        if (!rows.empty()) HIP_CHECK(hipMemcpyAsync(set->A.ptr, rows.data(), rows.size() * sizeof(real_t), hipMemcpyHostToDevice, r->dev.stream));
        HIP_CHECK(hipStreamSynchronize(r->dev.stream));      // `rows` goes away
        return rankset_run(r, set, fn, set->A.ptr, k, k_at, out, per_user, out_rank);
    });
}

int cmfrec_hip_ranker_similar(cmfrec_hip_ranker *r, const int_t *query_ids, int_t nq, int metric, const size_t excl_p[], const int_t excl_i[],
                              int_t n_top, int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_ranker_similar";
    return guarded([&]() {
        if (r == nullptr || nq < 0 || n_top <= 0 || (nq > 0 && (!query_ids || !out_ids))) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        if (metric != TOPNS_DOT && metric != TOPNS_COSINE) {
            g_last_error = std::string(fn) + ": metric must be 0 (dot product) or 1 (cosine), got " + std::to_string(metric);
            return 2;
        }
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        for (int_t q = 0; q < nq; q++)
            if (query_ids[q] < 0 || query_ids[q] >= r->n) {
                g_last_error = std::string(fn) + ": query id " + std::to_string(query_ids[q]) + " (entry " + std::to_string(q) +
                               ") is not a row of the ranker's " + std::to_string(r->n);
                return 2;
            }
        if (excl_p != nullptr) {
            bool bad = false;
            for (int_t q = 0; !bad && q < nq; q++) bad = excl_p[q] > excl_p[q + 1];
            if (bad || (excl_p[nq] > 0 && excl_i == nullptr)) {
                g_last_error = std::string(fn) + ": invalid arguments (the exclusion lists are not a CSR over the queries)";
                return 2;
            }
        }
        if (nq == 0) return 0;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        const cmfrec_hip_ranker::Device &dev = r->dev;
        r->qid.upload(query_ids, (size_t)nq, dev.stream);
        if (excl_p) {
            r->ep.upload(excl_p, (size_t)nq + 1, dev.stream);
            r->ei.alloc_at_least(std::max<size_t>(excl_p[nq], 1));
            if (excl_p[nq] > 0) r->ei.upload(excl_i, excl_p[nq], dev.stream);
        }
        if (metric == TOPNS_COSINE) ensure_inverse_norms(r);             // outside the timed interval
        r->ids.alloc_at_least((size_t)nq * n_top);
        if (out_scores) r->sc.alloc_at_least((size_t)nq * n_top);
        TopnSimilarParams<real_t> P;
        P.query_ids = r->qid.ptr; P.nu = nq; P.B = r->B.ptr; P.ldb = r->ldb; P.n = r->n; P.k = r->k;
        P.rn = metric == TOPNS_COSINE ? r->rn.ptr : nullptr;
        P.excl_p = excl_p ? r->ep.ptr : nullptr; P.excl_i = excl_p ? r->ei.ptr : nullptr;
        P.n_top = n_top; P.out_ids = r->ids.ptr; P.out_scores = out_scores ? r->sc.ptr : nullptr;
        int bpc = 1;
        const int nut = pick_user_tiles(nq, r->k, n_top, dev.num_cus, &bpc, 16 * (sizeof(real_t) + sizeof(int)));
        poison_lds(dev.stream, dev.num_cus);                             // (the policy's LDS too is written before it is read)
        HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
        r->last_grid = metric == TOPNS_COSINE ? launch_similar_tiles<TOPNS_COSINE>(dev, P, nut, bpc) : launch_similar_tiles<TOPNS_DOT>(dev, P, nut, bpc);
        r->last_users = 16 * nut;
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipEventRecord(r->ev1, dev.stream));
        r->timed = true;
        r->last_slices = 1;
        r->ids.download(out_ids, (size_t)nq * n_top, dev.stream);
        if (out_scores) r->sc.download(out_scores, (size_t)nq * n_top, dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        return 0;
    });
}

int cmfrec_hip_ranker_inverse_norms(cmfrec_hip_ranker *r, real_t *out)
{
    return guarded([&]() {
        if (r == nullptr || out == nullptr) {
            g_last_error = "cmfrec_hip_ranker_inverse_norms: invalid arguments";
            return 2;
        }
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        ensure_inverse_norms(r);
        r->rn.download(out, (size_t)r->n, r->dev.stream);
        HIP_CHECK(hipStreamSynchronize(r->dev.stream));
        return 0;
    });
}

int cmfrec_hip_ranker_kernel_ms(cmfrec_hip_ranker *r, double *ms)
{
    return guarded([&]() {
        if (r == nullptr || ms == nullptr || !r->timed) {
            g_last_error = "cmfrec_hip_ranker_kernel_ms: no ranking call on this handle yet";
            return 2;
        }
        HIP_CHECK(hipEventSynchronize(r->ev1));
        float t = 0;
        HIP_CHECK(hipEventElapsedTime(&t, r->ev0, r->ev1));
        *ms = (double)t;
        return 0;
    });
}

int cmfrec_hip_ranker_set_split(cmfrec_hip_ranker *r, int slices)
{
    if (r == nullptr || slices < -1) {
        g_last_error = "cmfrec_hip_ranker_set_split: invalid arguments (-1: off, 0: the planner's choice, >= 1: that many slices)";
        return 2;
    }
    r->split = slices;
    return 0;
}

int cmfrec_hip_ranker_slices(cmfrec_hip_ranker *r, int *slices)
{
    if (r == nullptr || slices == nullptr || !r->timed) {
        g_last_error = "cmfrec_hip_ranker_slices: no ranking call on this handle yet";
        return 2;
    }
    *slices = r->last_slices;
    return 0;
}

int cmfrec_hip_topn_split_plan(int_t nu, int_t n, int_t k, int_t n_top, int num_cus, size_t sizeof_real, int requested, int *slices,
                               int *slice_items)
{
    if (nu <= 0 || n <= 0 || k <= 0 || k > TOPNW_KMAX || n_top <= 0 || n_top > TOPN_NMAX || n_top > n || num_cus <= 0 ||
        (sizeof_real != 4 && sizeof_real != 8) || requested < 0 || slices == nullptr || slice_items == nullptr) {
        g_last_error = std::string("cmfrec_hip_topn_split_plan: invalid arguments (") + LIMITS + "; sizeof_real 4 or 8; requested >= 0)";
        return 2;
    }
    plan_split(nu, n, k, n_top, num_cus, sizeof_real, requested, slices, slice_items);
    return 0;
}

int cmfrec_hip_ranker_launch_shape(cmfrec_hip_ranker *r, int *users_per_workgroup, int *workgroups)
{
    if (r == nullptr || !r->timed) {
        g_last_error = "cmfrec_hip_ranker_launch_shape: no ranking call on this handle yet";
        return 2;
    }
    if (users_per_workgroup) *users_per_workgroup = r->last_users;
    if (workgroups) *workgroups = r->last_grid;
    return 0;
}

void cmfrec_hip_ranker_destroy(cmfrec_hip_ranker *r)
{
    delete r;
}

int cmfrec_hip_topN_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k,
                          const real_t *biasB, const size_t excl_p[], const int_t excl_i[], int_t n_top,
                          int_t *out_ids, real_t *out_scores)
{
    if (nu <= 0 || n <= 0 || k <= 0 || n_top <= 0 || !A || !B || !out_ids) {
        g_last_error = "cmfrec_hip_topN_batch: invalid arguments";
        return 2;
    }
    if (k > TOPNW_KMAX || n_top > TOPN_NMAX || n_top > n) {
        g_last_error = std::string("cmfrec_hip_topN_batch: ") + LIMITS;
        return 2;
    }
    cmfrec_hip_ranker *r = cmfrec_hip_ranker_create(B, ldb, n, k, biasB, -1);
    if (r == nullptr) return g_last_rc;
    const int rc = cmfrec_hip_ranker_topN(r, A, lda, nu, excl_p, excl_i, n_top, out_ids, out_scores);
    cmfrec_hip_ranker_destroy(r);
    return rc;
}

int cmfrec_hip_topN_deep_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k,
                               const real_t *biasB, const size_t excl_p[], const int_t excl_i[], int_t n_top,
                               int_t *out_ids, real_t *out_scores)
{
    if (nu <= 0 || n <= 0 || k <= 0 || !A || !B) {
        g_last_error = "cmfrec_hip_topN_deep_batch: invalid arguments";
        return 2;
    }
    if (k > TOPNW_KMAX || n_top < 1 || n_top > n) {
        g_last_error = std::string("cmfrec_hip_topN_deep_batch: ") + DEEP_LIMITS;
        return 2;
    }
    if (!out_ids) {
        g_last_error = "cmfrec_hip_topN_deep_batch: invalid arguments";
        return 2;
    }
    cmfrec_hip_ranker *r = cmfrec_hip_ranker_create(B, ldb, n, k, biasB, -1);
    if (r == nullptr) return g_last_rc;
    const int rc = cmfrec_hip_ranker_topN_deep(r, A, lda, nu, excl_p, excl_i, n_top, out_ids, out_scores);
    cmfrec_hip_ranker_destroy(r);
    return rc;
}

int cmfrec_hip_topN_candidates_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k,
                                     const real_t *biasB, const size_t cand_p[], const int_t cand_i[], const size_t excl_p[],
                                     const int_t excl_i[], int_t n_top, int_t *out_ids, real_t *out_scores)
{
    if (nu <= 0 || n <= 0 || k <= 0 || n_top <= 0 || !A || !B || !out_ids || !cand_p) {
        g_last_error = "cmfrec_hip_topN_candidates_batch: invalid arguments";
        return 2;
    }
    if (k > TOPNW_KMAX || n_top > TOPN_NMAX || n_top > n) {
        g_last_error = std::string("cmfrec_hip_topN_candidates_batch: ") + LIMITS;
        return 2;
    }
    cmfrec_hip_ranker *r = cmfrec_hip_ranker_create(B, ldb, n, k, biasB, -1);
    if (r == nullptr) return g_last_rc;
    const int rc = cmfrec_hip_ranker_topN_candidates(r, A, lda, nu, cand_p, cand_i, excl_p, excl_i, n_top, out_ids, out_scores);
    cmfrec_hip_ranker_destroy(r);
    return rc;
}

int cmfrec_hip_similar_batch(const real_t *B, size_t ldb, int_t n, int_t k, const int_t *query_ids, int_t nq, int metric, const size_t excl_p[],
                             const int_t excl_i[], int_t n_top, int_t *out_ids, real_t *out_scores)
{
    if (n <= 0 || k <= 0 || nq < 0 || n_top <= 0 || !B) {
        g_last_error = "cmfrec_hip_similar_batch: invalid arguments";
        return 2;
    }
    if (k > TOPNW_KMAX || n_top > TOPN_NMAX || n_top > n) {
        g_last_error = std::string("cmfrec_hip_similar_batch: ") + LIMITS;
        return 2;
    }
    cmfrec_hip_ranker *r = cmfrec_hip_ranker_create(B, ldb, n, k, nullptr, -1);
    if (r == nullptr) return g_last_rc;
    const int rc = cmfrec_hip_ranker_similar(r, query_ids, nq, metric, excl_p, excl_i, n_top, out_ids, out_scores);
    cmfrec_hip_ranker_destroy(r);
    return rc;
}

int cmfrec_hip_ranks_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k, const real_t *biasB,
                           const size_t held_p[], const int_t held_i[], const size_t excl_p[], const int_t excl_i[],
                           int_t *out_rank, real_t *out_scores, int_t *out_pool)
{
    if (nu <= 0 || n <= 0 || k <= 0 || !A || !B || !held_p) {
        g_last_error = "cmfrec_hip_ranks_batch: invalid arguments";
        return 2;
    }
    if (k > TOPNW_KMAX) {
        g_last_error = std::string("cmfrec_hip_ranks_batch: ") + RANK_LIMITS;
        return 2;
    }
    cmfrec_hip_ranker *r = cmfrec_hip_ranker_create(B, ldb, n, k, biasB, -1);
    if (r == nullptr) return g_last_rc;
    const int rc = cmfrec_hip_ranker_ranks(r, A, lda, nu, held_p, held_i, excl_p, excl_i, out_rank, out_scores, out_pool);
    cmfrec_hip_ranker_destroy(r);
    return rc;
}

}  // extern "C"

namespace cmfhip {

int ranker_check_limits(const char *fn, int_t k, int_t n_top, int_t n)
{
    if (k > TOPNW_KMAX || k <= 0) {
        g_last_error = std::string(fn) + ": " + LIMITS;
        return 2;
    }
    return check_n_top(fn, n_top, n);
}

cmfrec_hip_ranker *ranker_create_from_device(const real_t *dB, size_t ldb, int_t n, int_t k, const real_t *dbiasB, int device)
{
    // (uploads are hipMemcpyDefault copies: the same create serves items that are on the device already)
    return cmfrec_hip_ranker_create(dB, ldb, n, k, dbiasB, device);
}

int ranker_topN_device(cmfrec_hip_ranker *r, const char *fn, const real_t *dA, size_t lda, int_t nu, const size_t *dexcl_p,
                       const int *dexcl_i, int_t n_top, int_t *out_ids, real_t *out_scores)
{
    return guarded([&]() {
        if (r == nullptr || nu <= 0 || n_top <= 0 || !dA || !out_ids || lda < (size_t)r->k) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        return rank_device(r, dA, lda, nu, dexcl_p, dexcl_i, n_top, out_ids, out_scores);
    });
}

int ranker_topN_candidates_device(cmfrec_hip_ranker *r, const char *fn, const real_t *dA, size_t lda, int_t nu, const size_t cand_p[],
                                  const int_t cand_i[], const size_t *dexcl_p, const int *dexcl_i, int_t n_top, int_t *out_ids,
                                  real_t *out_scores)
{
    return guarded([&]() {
        if (r == nullptr || nu <= 0 || n_top <= 0 || !dA || !out_ids || !cand_p || lda < (size_t)r->k) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        if (int rc = upload_candidates(r, fn, nu, cand_p, cand_i)) return rc;
        return rank_device(r, dA, lda, nu, dexcl_p, dexcl_i, n_top, out_ids, out_scores, r->cp.ptr, r->ci.ptr);
    });
}

int ranker_ranks_device(cmfrec_hip_ranker *r, const char *fn, const real_t *dA, size_t lda, int_t nu, const size_t held_p[],
                        const int_t held_i[], const size_t *dexcl_p, const int *dexcl_i, int_t *out_rank, real_t *out_scores,
                        int_t *out_pool)
{
    return guarded([&]() {
        if (r == nullptr || nu <= 0 || !dA || !held_p || lda < (size_t)r->k || (held_p[nu] > 0 && !out_rank)) {
            g_last_error = std::string(fn) + ": invalid arguments";
            return 2;
        }
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        size_t max_held = 0;
        if (int rc = upload_held(r, fn, nu, held_p, held_i, &max_held)) return rc;
        return ranks_device(r, dA, lda, nu, held_p[nu], max_held, dexcl_p, dexcl_i, out_rank, out_scores, out_pool);
    });
}

}  // namespace cmfhip
