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
// topn_split_kernel over slices of the items and topn_split_merge_kernel behind it (topn_split_kernels.hpp).  A ranker whose filter
// is on (cmfrec_hip_ranker_set_filter) sends cmfrec_hip_ranker_topN of n_top <= 64 through topn_filter_kernel (topn_filter_kernels.hpp,
// launched from topn_filter_tu.hip), topn_filter_refine_kernel over the shortlists -- with the arithmetic of the kernel the call
// would run unfiltered -- and topn_filter_certify_kernel; the users that are not certified take the route above in a second batch.
// A diversified call (cmfrec_hip_ranker_rerank_mmr / _topN_diverse) launches topn_mmr_kernel (topn_mmr_kernels.hpp, from
// topn_mmr_tu.hip) over per-user pools that are on the device: the caller's, or the lists the full ranking above left there.
// A sampling call (cmfrec_hip_ranker_topN_sample) launches topn_sample_kernel -- the wide kernel's body under a policy that adds
// Gumbel noise to the scores -- and topn_sample_scores_kernel behind it (topn_sample_kernels.hpp, from topn_sample_tu.hip), for
// every k; temperature 0 launches topn_wide_kernel.  It reads none of the handle's split or filter settings.
// An explanation call (cmfrec_hip_ranker_explain) launches topn_explain_kernel (topn_explain_kernels.hpp, from topn_explain_tu.hip)
// over per-user histories and target lists; it reads the resident rows and none of the handle's split or filter settings.
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
#include "topn_filter.hpp"
#include "topn_mmr_kernels.hpp"
#include "topn_explain_kernels.hpp"
#include "topn_sample_kernels.hpp"
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
    int filter = 0;                          // cmfrec_hip_ranker_set_filter: 0 off, 1 the half-precision filter
    TopnFilterImage fimg;                    // the image of B, built when the filter is switched on
    DevBuf<int> f_short, f_state, f_cert;    // shortlists [nu][m], per-user state and certificate of a filtered call
    DevBuf<float> f_tau, f_keys;
    int fs_users = 0, fs_filtered = 0, fs_certified = 0;   // of the last cmfrec_hip_ranker_topN
    bool fs_valid = false;
    hipEvent_t fev[4] = {nullptr, nullptr, nullptr, nullptr};   // around the filter, the refinement and the certificate
    float f_ms[3] = {0, 0, 0};
    DevBuf<int> mmr_ids;                     // the result of a diversified call: [nu][n_top] (its pools use ids / sc)
    DevBuf<real_t> mmr_sc, mmr_v;
    DevBuf<size_t> x_hp, x_tp;               // an explanation call: histories and targets (CSR over the users) ...
    DevBuf<int> x_hi, x_ti;
    DevBuf<real_t> sm_keys;                  // a sampling call: the keys of the lists (their ids and scores: ids / sc) ...
    DevBuf<double> sm_lse;                   // ... and the users' log-partitions
    DevBuf<real_t> x_g, x_y, x_g0, x_du, x_dbu, x_tot;   // ... their coefficients, G0, the per-user diagonals, the totals (lists: ids / sc)
    const real_t *item_bias() const { return has_bias ? bias.ptr : nullptr; }
    ~cmfrec_hip_ranker()
    {
        for (hipEvent_t e : fev)
            if (e) (void)hipEventDestroy(e);
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        if (dev.stream) (void)hipStreamDestroy(dev.stream);
    }
};

namespace {

constexpr const char *LIMITS = "needs k <= 272 and n_top <= min(128, n)";
constexpr const char *RANK_LIMITS = "needs k <= 272";
constexpr const char *DEEP_LIMITS = "needs k <= 272 and 1 <= n_top <= n";
constexpr const char *EXPLAIN_LIMITS = "needs k + bias <= 128 and 1 <= n_top <= 64";
constexpr const char *SAMPLE_LIMITS = "needs k <= 272, 1 <= n_top <= min(128, n) and a finite temperature >= 0 whose inverse is finite";
constexpr const char *MMR_LIMITS = "needs k <= 272, 1 <= n_top <= pool <= min(128, n) and 0 <= theta <= 1";

// User tiles per workgroup of the wide kernel (DESIGN.md "Top-N for wide models"): as many as the LDS holds beside the lists,
// unless fewer finish the nu users in fewer or cheaper waves of workgroups.  A workgroup's time per item round is about
// (nut + 1/2) -- its MFMAs and the item fetch they share -- times the workgroups that share its CU.
// CMFREC_HIP_TOPN_TILES (test hook) asks for a number of tiles; it is clamped to what fits.
// extra_per_tile: LDS bytes per user tile beyond topnw_lds_bytes (the neighbour kernel's ids and inverse norms).
// max_nut: a kernel that cannot take all TOPNW_MAX_NUT tiles (the sampling kernel with its log-partition, in double precision).
int pick_user_tiles(int nu, int k, int n_top, int num_cus, int *blocks_per_cu, size_t extra_per_tile = 0, size_t sizeof_real = sizeof(real_t),
                    int max_nut = TOPNW_MAX_NUT)
{
    const int forced = switches().topn_tiles;
    int best = 1, best_bpc = 1;
    double best_cost = 0;
    for (int nut = 1; nut <= max_nut; nut++) {
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

// the run-time tile count as a compile-time one: f(std::integral_constant<int, NUT>) for NUT = nut
template <class F>
int with_tiles(int nut, F &&f)
{
    static_assert(TOPNW_MAX_NUT == 4, "one case per tile count");
    switch (nut) {
    case 1: return f(std::integral_constant<int, 1>());
    case 2: return f(std::integral_constant<int, 2>());
    case 3: return f(std::integral_constant<int, 3>());
    default: return f(std::integral_constant<int, 4>());
    }
}

// One launch of a kernel that takes nut user tiles per workgroup and smem bytes of LDS: a workgroup per tile group of P.nu users,
// at most blocks_per_cu per CU, times grid_y (the item slices of the split kernel).  Returns the grid's first dimension.
template <class Params>
int launch_tiled(const cmfrec_hip_ranker::Device &dev, void (*kernel)(Params), int nut, size_t smem, const Params &P, int blocks_per_cu,
                 int grid_y = 1)
{
    HIP_CHECK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
    const int tiles = (P.nu + 16 * nut - 1) / (16 * nut);
    const int grid = std::min(tiles, dev.num_cus * blocks_per_cu);
    hipLaunchKernelGGL(kernel, dim3(grid, grid_y), dim3(TOPNW_TH), smem, dev.stream, P);
    HIP_CHECK(hipGetLastError());
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

int refuse(const char *fn, const std::string &why)
{
    g_last_error = std::string(fn) + ": " + why;
    return 2;
}

int check_n_top(const char *fn, int_t n_top, int_t n)
{
    return (n_top > TOPN_NMAX || n_top > n) ? refuse(fn, LIMITS) : 0;
}

// what every call over a batch of users refuses as "invalid arguments": no handle, no users, factors narrower than the model,
// exclusion offsets that promise indices that are not there (the order of an exclusion list is the caller's business)
bool bad_users(const cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t *excl_p = nullptr, const int_t *excl_i = nullptr)
{
    return r == nullptr || nu <= 0 || !A || lda < (size_t)r->k || (excl_p != nullptr && excl_i == nullptr && excl_p[nu] > 0);
}

// lists over `count` users or queries are a CSR: offsets that do not decrease, indices where there is an entry; *longest = the
// longest list
bool csr_ok(const size_t *p, const int_t *i, int_t count, size_t *longest = nullptr)
{
    if (p == nullptr) return false;
    size_t len = 0;
    for (int_t u = 0; u < count; u++) {
        if (p[u] > p[u + 1]) return false;
        len = std::max(len, p[u + 1] - p[u]);
    }
    if (longest) *longest = len;
    return p[count] == 0 || i != nullptr;
}

void upload_csr(DevBuf<size_t> &dp, DevBuf<int> &di, const size_t *p, const int_t *i, int_t count, hipStream_t st)
{
    dp.upload(p, (size_t)count + 1, st);
    di.alloc_at_least(std::max<size_t>(p[count], 1));
    if (p[count] > 0) di.upload(i, p[count], st);
}

// the users of a call, on the device: factors dA [nu, lda] (null in a neighbour call, whose users are rows of B) and their
// exclusion lists, both null where the call has none
struct RankUsers {
    const real_t *dA; size_t lda; int_t nu;
    const size_t *excl_p; const int *excl_i;
};

// the factors of a call's users from the host (or wherever A is) into r->A, packed
RankUsers stage_users(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu)
{
    const size_t k = (size_t)r->k;
    r->A.alloc_at_least((size_t)nu * k);
    upload_columns(r->A.ptr, k, A, lda, (size_t)nu, k, r->dev.stream);
    return RankUsers{r->A.ptr, k, nu, nullptr, nullptr};
}

// ... and their exclusion lists (host CSR over users.nu, or null) into r->ep / r->ei
void stage_exclusions(cmfrec_hip_ranker *r, RankUsers &users, const size_t *excl_p, const int_t *excl_i)
{
    if (excl_p == nullptr) return;
    upload_csr(r->ep, r->ei, excl_p, excl_i, users.nu, r->dev.stream);
    users.excl_p = r->ep.ptr; users.excl_i = r->ei.ptr;
}

// The fields the kernels' parameter structs have in common, filled from the ranker and the call; a struct without one of the
// groups (the neighbour kernel has no user factors, the refinement no exclusions) does not call that group's function.
template <class P> void set_items(P &p, const cmfrec_hip_ranker *r) { p.B = r->B.ptr; p.ldb = r->ldb; p.n = r->n; p.k = r->k; }
template <class P> void set_users(P &p, const RankUsers &u) { p.A = u.dA; p.lda = u.lda; p.nu = u.nu; }
template <class P> void set_exclusions(P &p, const RankUsers &u) { p.excl_p = u.excl_p; p.excl_i = u.excl_p ? u.excl_i : nullptr; }
template <class P> void set_lists(P &p, const cmfrec_hip_ranker *r, int_t n_top, bool want_scores)
{
    p.n_top = n_top; p.out_ids = r->ids.ptr; p.out_scores = want_scores ? r->sc.ptr : nullptr;
}

// the parameters of a kernel that scores the users against every item: all of the above but the lists
template <class P>
P ranking_params(const cmfrec_hip_ranker *r, const RankUsers &users)
{
    P p;
    set_items(p, r); p.biasB = r->item_bias();
    set_users(p, users); set_exclusions(p, users);
    return p;
}

// the end of the interval that cmfrec_hip_ranker_kernel_ms reports, and what _launch_shape and _slices say of its last launch
void end_timed(cmfrec_hip_ranker *r, int users_per_workgroup, int grid, int slices)
{
    HIP_CHECK(hipEventRecord(r->ev1, r->dev.stream));
    r->timed = true;
    r->last_users = users_per_workgroup; r->last_grid = grid; r->last_slices = slices;
}

// the call's result comes down and the stream is waited for.  more / out_more: a third array of the call (the pools of a rank
// call, the certificates of a filtered one), null where there is none or the caller does not want it
void download_and_wait(cmfrec_hip_ranker *r, size_t cells, int_t *out_ids, real_t *out_scores, const DevBuf<int> *more = nullptr,
                       int *out_more = nullptr, size_t n_more = 0)
{
    hipStream_t st = r->dev.stream;
    r->ids.download(out_ids, cells, st);
    if (out_scores) r->sc.download(out_scores, cells, st);
    if (out_more) more->download(out_more, n_more, st);
    HIP_CHECK(hipStreamSynchronize(st));
}

// the ranking of users who are on the device already: the launch, the timing events and the download of cmfrec_hip_ranker_topN
// (the caller holds the DeviceScope and has checked the limits)
// dcand_p != null: over each user's candidate list (device CSR) on topn_cand_kernel
// stay: ids and scores stay on the device (r->ids, r->sc) for the kernel behind the launch; nothing is downloaded and the stream
// is not waited for
int rank_device(cmfrec_hip_ranker *r, const RankUsers &users, int_t n_top, int_t *out_ids, real_t *out_scores,
                const size_t *dcand_p = nullptr, const int *dcand_i = nullptr, bool stay = false)
{
    const bool want_scores = out_scores != nullptr || stay;
    const cmfrec_hip_ranker::Device &dev = r->dev;
    const int k = r->k;
    const int_t nu = users.nu;
    const size_t cells = (size_t)nu * n_top;
    r->ids.alloc_at_least(cells);
    if (want_scores) r->sc.alloc_at_least(cells);
    if (dcand_p) {
        r->next.alloc_at_least(1);
        HIP_CHECK(hipMemsetAsync(r->next.ptr, 0, sizeof(unsigned), dev.stream));
    }
    // a split ranker: the full ranking of every k on the MFMA arithmetic, over as many item slices as the planner gives it
    const bool split = dcand_p == nullptr && r->split >= 0;
    int slices = 1, slice_items = 0;
    if (split) plan_split(nu, r->n, k, n_top, dev.num_cus, sizeof(real_t), r->split, &slices, &slice_items);
    if (slices > 1) {
        r->part_sc.alloc_at_least((size_t)slices * cells);
        r->part_id.alloc_at_least((size_t)slices * cells);
    }
    HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
    int users_per_workgroup = 0, grid = 0;
    if (dcand_p) {
        auto P = ranking_params<TopnCandParams<real_t>>(r, users);
        set_lists(P, r, n_top, want_scores);
        P.cand_p = dcand_p; P.cand_i = dcand_i;
        P.next = r->next.ptr; P.order = r->corder.ptr;
        grid = launch_topn_cand(dev.stream, dev.num_cus, P, switches().topn_cand_waves);
        users_per_workgroup = TOPNC_NW;
    } else if (slices > 1) {
        // the slice pass writes every slice's list into the scratch, the merge makes the call's result of them
        auto P = ranking_params<TopnSplitParams<real_t>>(r, users);
        P.n_top = n_top; P.out_ids = r->part_id.ptr; P.out_scores = r->part_sc.ptr;
        P.slice_items = slice_items; P.s0 = P.s1 = 0;
        TopnMergeParams<real_t> M;
        M.part_scores = r->part_sc.ptr; M.part_ids = r->part_id.ptr; M.slices = slices; M.nu = nu;
        set_lists(M, r, n_top, want_scores);
        int bpc = 1;
        const int nut = pick_user_tiles(nu, k, n_top, dev.num_cus, &bpc);
        grid = slices * with_tiles(nut, [&](auto t) {
            const int tiles = launch_tiled(dev, topn_split_kernel<real_t, t()>, t(), topnw_lds_bytes(t(), k, n_top, sizeof(real_t)), P, bpc, slices);
            const int nw = topnsp_merge_waves(slices);
            hipLaunchKernelGGL(topn_split_merge_kernel<real_t>, dim3(nu), dim3(64 * nw), topnsp_merge_lds_bytes(nw, n_top, sizeof(real_t)),
                               dev.stream, M);
            return tiles;
        });
        users_per_workgroup = 16 * nut;
    } else if (k <= TOPN_KMAX && !switches().topn_wide && !split) {
        auto P = ranking_params<TopnParams<real_t>>(r, users);
        set_lists(P, r, n_top, want_scores);
        const size_t smem = topn_lds_bytes(sizeof(real_t));
        HIP_CHECK(hipFuncSetAttribute((const void *)topn_kernel<real_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        grid = std::min((nu + TOPN_UT - 1) / TOPN_UT, dev.num_cus * 2);
        hipLaunchKernelGGL(topn_kernel<real_t>, dim3(grid), dim3(TOPN_TH), smem, dev.stream, P);
        users_per_workgroup = TOPN_UT;
    } else {
        auto P = ranking_params<TopnWideParams<real_t>>(r, users);
        set_lists(P, r, n_top, want_scores);
        int bpc = 1;
        const int nut = pick_user_tiles(nu, k, n_top, dev.num_cus, &bpc);
        grid = with_tiles(nut, [&](auto t) {
            return launch_tiled(dev, topn_wide_kernel<real_t, t()>, t(), topnw_lds_bytes(t(), k, n_top, sizeof(real_t)), P, bpc);
        });
        users_per_workgroup = 16 * nut;
    }
    HIP_CHECK(hipGetLastError());
    end_timed(r, users_per_workgroup, grid, slices);
    if (!stay) download_and_wait(r, cells, out_ids, out_scores);
    return 0;
}

// the image of the ranker's items, built on first use and again after the items changed; false: the filter cannot run on them
bool ensure_filter_image(cmfrec_hip_ranker *r)
{
    if (!r->fimg.ready)
        topn_filter_build_image(r->dev.stream, r->dev.num_cus, r->B.ptr, r->ldb, r->n, r->k, r->item_bias(), r->fimg);
    return r->fimg.usable;
}

// shortlist length of a filtered call: topnf_m; CMFREC_HIP_TOPN_FILTER_M (test hook, 32 .. 128, read per call) forces it
int filter_m(int_t n_top)
{
    const char *v = getenv("CMFREC_HIP_TOPN_FILTER_M");
    return topnf_m((int)n_top, (v != nullptr && v[0] != 0) ? atoi(v) : 0);
}

// the filter kernel's parameters over the image of the items; the outputs are the caller's to set
TopnFilterParams<real_t> filter_params(cmfrec_hip_ranker *r, const RankUsers &users, int m)
{
    TopnFilterParams<real_t> P;
    set_users(P, users); set_exclusions(P, users);
    P.Bh = r->fimg.Bh.ptr; P.n = r->n; P.k = r->k;
    P.nb = r->fimg.nb.ptr; P.db = r->fimg.db.ptr; P.sb = r->fimg.sb;
    P.biasB = r->item_bias(); P.m = m;
    P.short_ids = nullptr; P.tau = nullptr; P.state = nullptr; P.keys = nullptr;
    return P;
}

// The filtered ranking of users who are on the device: topn_filter_kernel leaves a shortlist of m ids
// and the bound tau per user, topn_filter_refine_kernel ranks the shortlists with the scores of the kernel rank_device would
// launch for this ranker (the same routing), topn_filter_certify_kernel compares.  ids / scores come down for every user,
// certified [nu] says whose are final.
int rank_device_filtered(cmfrec_hip_ranker *r, const RankUsers &users, int_t n_top, int_t *out_ids, real_t *out_scores, int *certified)
{
    const cmfrec_hip_ranker::Device &dev = r->dev;
    const int_t nu = users.nu;
    const int m = filter_m(n_top);
    const size_t cells = (size_t)nu * (size_t)n_top;
    r->ids.alloc_at_least(cells);
    r->sc.alloc_at_least(cells);
    r->f_short.alloc_at_least((size_t)nu * (size_t)m);
    r->f_state.alloc_at_least((size_t)nu);
    r->f_cert.alloc_at_least((size_t)nu);
    r->f_tau.alloc_at_least((size_t)nu);
    for (hipEvent_t &e : r->fev)
        if (!e) HIP_CHECK(hipEventCreate(&e));
    TopnFilterParams<real_t> F = filter_params(r, users, m);
    F.short_ids = r->f_short.ptr; F.tau = r->f_tau.ptr; F.state = r->f_state.ptr;
    HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
    HIP_CHECK(hipEventRecord(r->fev[0], dev.stream));
    int users_per_workgroup = 0;
    const int grid = topn_filter_launch(dev.stream, dev.num_cus, F, switches().topn_tiles, &users_per_workgroup);
    HIP_CHECK(hipEventRecord(r->fev[1], dev.stream));
    TopnRefineParams<real_t> P;
    set_items(P, r); P.biasB = r->item_bias();
    set_users(P, users);
    set_lists(P, r, n_top, true);
    P.short_ids = r->f_short.ptr; P.m = m;
    topn_filter_refine(dev.stream, dev.num_cus, P, !(r->k <= TOPN_KMAX && !switches().topn_wide));
    HIP_CHECK(hipEventRecord(r->fev[2], dev.stream));
    topn_filter_certify(dev.stream, r->sc.ptr, nu, n_top, r->f_tau.ptr, r->f_state.ptr, r->f_cert.ptr);
    HIP_CHECK(hipEventRecord(r->fev[3], dev.stream));
    end_timed(r, users_per_workgroup, grid, 1);
    download_and_wait(r, cells, out_ids, out_scores, &r->f_cert, certified, (size_t)nu);
    for (int s = 0; s < 3; s++) HIP_CHECK(hipEventElapsedTime(&r->f_ms[s], r->fev[s], r->fev[s + 1]));
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

// The n_top best of the users behind their cursors, in pages of page_len on topn_after_kernel, for every k (the register-resident
// topn_kernel of k <= 64 rounds otherwise, and a cursor compares bits).  The whole [nu, n_top] result lives in r->ids / r->sc;
// page p is one launch that writes the columns [p * page_len, ...) and reads its cursors from the column in front of them -- no
// host round trip between the pages, one download at the end.  The first page's cursors: dcur_s / dcur_i [nu], or null (every
// user starts at the top).  The timing events enclose all the pages.  Returns the launches in *pages.
// (the caller holds the DeviceScope and has checked the limits; the users are on the device)
int rank_device_deep(cmfrec_hip_ranker *r, const RankUsers &users, int_t n_top, int page_len, const real_t *dcur_s, const int *dcur_i,
                     int_t *out_ids, real_t *out_scores, int *pages)
{
    const cmfrec_hip_ranker::Device &dev = r->dev;
    const size_t cells = (size_t)users.nu * (size_t)n_top;
    r->ids.alloc_at_least(cells);
    r->sc.alloc_at_least(cells);                                         // (the next page's cursors, wanted by the caller or not)
    auto P = ranking_params<TopnAfterParams<real_t>>(r, users);
    P.out_ld = (size_t)n_top;
    poison_lds(dev.stream, dev.num_cus);                                 // (the policy's LDS too is written before it is read)
    HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
    int launches = 0, nut = 1, grid = 0;
    for (int_t first = 0; first < n_top; first += page_len, launches++) {
        P.n_top = (int)std::min<int_t>(page_len, n_top - first);
        P.out_ids = r->ids.ptr + first; P.out_scores = r->sc.ptr + first;
        if (first == 0) { P.cur_scores = dcur_s; P.cur_ids = dcur_s ? dcur_i : nullptr; P.cur_ld = 1; }
        else { P.cur_scores = r->sc.ptr + first - 1; P.cur_ids = r->ids.ptr + first - 1; P.cur_ld = (size_t)n_top; }
        int bpc = 1;
        nut = pick_user_tiles(users.nu, r->k, P.n_top, dev.num_cus, &bpc, topna_extra_bytes(sizeof(real_t)));
        grid = with_tiles(nut, [&](auto t) {
            return launch_tiled(dev, topn_after_kernel<real_t, t()>, t(), topna_lds_bytes(t(), P.k, P.n_top, sizeof(real_t)), P, bpc);
        });
    }
    end_timed(r, 16 * nut, grid, 1);
    download_and_wait(r, cells, out_ids, out_scores);
    if (pages) *pages = launches;
    return 0;
}

// the candidate lists of a call (host CSR over the nu users) into the ranker's buffers; 2 with a message for lists that are not a CSR
int upload_candidates(cmfrec_hip_ranker *r, const char *fn, int_t nu, const size_t cand_p[], const int_t cand_i[])
{
    if (!csr_ok(cand_p, cand_i, nu)) return refuse(fn, "invalid arguments");
    // the order the kernel hands the users out in: longest list first (a long list that starts last is the launch's tail)
    std::vector<int> order((size_t)nu);
    for (int_t u = 0; u < nu; u++) order[u] = u;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cand_p[a + 1] - cand_p[a] > cand_p[b + 1] - cand_p[b]; });
    r->corder.upload(order.data(), (size_t)nu, r->dev.stream);
    HIP_CHECK(hipStreamSynchronize(r->dev.stream));          // `order` goes away
    upload_csr(r->cp, r->ci, cand_p, cand_i, nu, r->dev.stream);
    return 0;
}

// the held-out lists of a call (host CSR over the nu users) into the ranker's buffers; 2 with a message for lists that are not a
// CSR; *max_held = the longest list
int upload_held(cmfrec_hip_ranker *r, const char *fn, int_t nu, const size_t held_p[], const int_t held_i[], size_t *max_held)
{
    if (!csr_ok(held_p, held_i, nu, max_held) || *max_held > (size_t)0x7fffffff) return refuse(fn, "invalid arguments");
    upload_csr(r->cp, r->ci, held_p, held_i, nu, r->dev.stream);
    return 0;
}

// the ranks of users who are on the device, as are their held-out lists (total entries, the longest max_held): the launch, the
// timing events (around topn_rank_kernel, whose threshold and exclusion steps are part of it) and the download.  Nothing is
// written to the outputs before the kernel has run.
// dheld_p / dheld_i: the held-out lists where they are (null: the ranker's own r->cp / r->ci, filled by upload_held).  stay: the
// ranks and the pool stay on the device (r->ids, r->pool) for rank_metrics_kernel behind the launch; nothing is downloaded and
// the stream is not waited for.
int ranks_device(cmfrec_hip_ranker *r, const RankUsers &users, size_t total, size_t max_held, int_t *out_rank, real_t *out_scores,
                 int_t *out_pool, const size_t *dheld_p = nullptr, const int *dheld_i = nullptr, bool stay = false)
{
    const cmfrec_hip_ranker::Device &dev = r->dev;
    r->ids.alloc_at_least(std::max<size_t>(total, 1));
    if (out_scores) r->sc.alloc_at_least(std::max<size_t>(total, 1));
    if (out_pool || stay) r->pool.alloc_at_least((size_t)users.nu);
    auto P = ranking_params<TopnRankParams<real_t>>(r, users);
    P.held_p = dheld_p ? dheld_p : r->cp.ptr; P.held_i = dheld_p ? dheld_i : r->ci.ptr;
    P.out_rank = r->ids.ptr; P.out_scores = out_scores ? r->sc.ptr : nullptr; P.out_pool = (out_pool || stay) ? r->pool.ptr : nullptr;
    int bpc = 1;
    const int nut = pick_rank_shape(users.nu, r->k, max_held, dev.num_cus, &P.ts, &P.tsp, &bpc);
    if (nut == 0) return refuse("cmfrec_hip_ranker_ranks", "the model does not fit the rank kernel's LDS");
    HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
    const int grid = with_tiles(nut, [&](auto t) {
        return launch_tiled(dev, topn_rank_kernel<real_t, t()>, t(), topnr_lds_bytes(t(), P.k, P.tsp, sizeof(real_t)), P, bpc);
    });
    end_timed(r, 16 * nut, grid, 1);
    if (!stay) download_and_wait(r, total, out_rank, out_scores, &r->pool, out_pool, (size_t)users.nu);
    return 0;
}

// what a diversified call refuses beyond "invalid arguments" (DESIGN.md section 3.19), before a device is touched
int check_mmr(const char *fn, int_t k, int_t n, int_t pool, int_t n_top, double theta)
{
    const bool ok = k <= TOPNW_KMAX && n_top >= 1 && n_top <= pool && pool <= TOPNM_POOL_MAX && pool <= n && theta >= 0.0 && theta <= 1.0;
    return ok ? 0 : refuse(fn, MMR_LIMITS);
}

// The MMR pass over the pools that are on the device, r->ids / r->sc [nu, pool]: the launch, the timing events and the download.
// CMFREC_HIP_MMR_GROUPS (test hook, read per call) caps the workgroups, so that a small batch gives one of them many users.
// (the caller holds the DeviceScope and has checked the limits)
int mmr_device(cmfrec_hip_ranker *r, int_t nu, int_t pool, double theta, int_t n_top, int_t *out_ids, real_t *out_scores, real_t *out_mmr)
{
    const cmfrec_hip_ranker::Device &dev = r->dev;
    const size_t cells = (size_t)nu * (size_t)n_top;
    ensure_inverse_norms(r);                                             // outside the timed interval
    r->mmr_ids.alloc_at_least(cells);
    r->mmr_sc.alloc_at_least(cells);
    if (out_mmr) r->mmr_v.alloc_at_least(cells);
    TopnMmrParams<real_t> P;
    set_items(P, r);
    P.rn = r->rn.ptr;
    P.pool_ids = r->ids.ptr; P.pool_scores = r->sc.ptr; P.nu = nu; P.pool = pool;
    P.theta = (real_t)theta; P.n_top = n_top;
    P.out_ids = r->mmr_ids.ptr; P.out_scores = r->mmr_sc.ptr; P.out_mmr = out_mmr ? r->mmr_v.ptr : nullptr;
    const char *cap = getenv("CMFREC_HIP_MMR_GROUPS");
    const int max_groups = (cap != nullptr && cap[0] != 0) ? atoi(cap) : 0;
    poison_lds(dev.stream, dev.num_cus);                                 // (every LDS word the kernel reads it has written)
    HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
    const int grid = topn_mmr_launch(dev.stream, dev.num_cus, P, max_groups);
    end_timed(r, 1, grid, 1);
    r->mmr_ids.download(out_ids, cells, dev.stream);
    r->mmr_sc.download(out_scores, cells, dev.stream);
    if (out_mmr) r->mmr_v.download(out_mmr, cells, dev.stream);
    HIP_CHECK(hipStreamSynchronize(dev.stream));
    return 0;
}

// what an explanation call refuses, before a device is touched: 0, or 2 with the message set
int check_explain(const char *fn, int_t n, int_t k, const cmfrec_hip_explain_args *a)
{
    if (a == nullptr || a->nu <= 0 || !a->hist_p || !a->targ_p) return refuse(fn, std::string("invalid arguments; ") + EXPLAIN_LIMITS);
    const int_t nu = a->nu;
    if (k + (a->bias ? 1 : 0) > TOPNX_KMAX || a->n_top < 1 || a->n_top > TOPNX_NTOP_MAX) return refuse(fn, EXPLAIN_LIMITS);
    if (a->G0 != nullptr && a->bias) return refuse(fn, "G0 together with a bias unknown is not supported");
    size_t longest = 0;
    if (!csr_ok(a->hist_p, a->hist_i, nu, &longest) || longest > (size_t)0x7fffff00)
        return refuse(fn, "invalid arguments (hist_p is not a CSR over the users: offsets that do not decrease)");
    if (!csr_ok(a->targ_p, a->targ_i, nu)) return refuse(fn, "invalid arguments (targ_p is not a CSR over the users: offsets that do not decrease)");
    if (a->hist_p[nu] > a->hist_p[0] && (!a->hist_g || !a->hist_y)) return refuse(fn, "invalid arguments (hist_g and hist_y are required)");
    if (a->targ_p[nu] > a->targ_p[0] && (!a->out_total || !a->out_ids || !a->out_contrib)) return refuse(fn, "invalid arguments (the outputs are required)");
    if (!(a->diag > 0.0) || (a->bias && a->diag_bias_u == nullptr && !(a->diag_bias > 0.0))) return refuse(fn, "diag (and diag_bias with a bias) must be > 0");
    if (a->diag_u != nullptr)
        for (int_t u = 0; u < nu; u++)
            if (!(a->diag_u[u] > (real_t)0)) return refuse(fn, "diag_u[" + std::to_string(u) + "] must be > 0");
    if (a->bias && a->diag_bias_u != nullptr)
        for (int_t u = 0; u < nu; u++)
            if (!(a->diag_bias_u[u] > (real_t)0)) return refuse(fn, "diag_bias_u[" + std::to_string(u) + "] must be > 0");
    for (size_t e = a->hist_p[0]; e < a->hist_p[nu]; e++)
        if (a->hist_i[e] < 0 || a->hist_i[e] >= n)
            return refuse(fn, "history id " + std::to_string(a->hist_i[e]) + " (entry " + std::to_string(e) + ") is not a row of the ranker's " + std::to_string(n));
    for (size_t e = a->targ_p[0]; e < a->targ_p[nu]; e++)
        if (a->targ_i[e] < 0 || a->targ_i[e] >= n)
            return refuse(fn, "target id " + std::to_string(a->targ_i[e]) + " (entry " + std::to_string(e) + ") is not a row of the ranker's " + std::to_string(n));
    return 0;
}

// The explanation pass: uploads, the launch, the timing events and the download.  CMFREC_HIP_EXPLAIN_GROUPS (test hook, read per
// call) caps the workgroups, so that a small batch gives one of them many users.  (the caller holds the DeviceScope and has
// checked the arguments)
int explain_device(cmfrec_hip_ranker *r, const cmfrec_hip_explain_args *a)
{
    const cmfrec_hip_ranker::Device &dev = r->dev;
    hipStream_t st = dev.stream;
    const int_t nu = a->nu;
    const size_t nh = a->hist_p[nu], nt = a->targ_p[nu], t_first = a->targ_p[0], cells = nt * (size_t)a->n_top;
    if (nt == t_first) return 0;                                         // no targets: nothing is written
    upload_csr(r->x_hp, r->x_hi, a->hist_p, a->hist_i, nu, st);
    upload_csr(r->x_tp, r->x_ti, a->targ_p, a->targ_i, nu, st);
    r->x_g.alloc_at_least(std::max<size_t>(nh, 1));
    r->x_y.alloc_at_least(std::max<size_t>(nh, 1));
    if (nh > 0) { r->x_g.upload(a->hist_g, nh, st); r->x_y.upload(a->hist_y, nh, st); }
    if (a->G0) r->x_g0.upload(a->G0, (size_t)r->k * r->k, st);
    if (a->diag_u) r->x_du.upload(a->diag_u, (size_t)nu, st);
    const bool bias_u = a->bias && a->diag_bias_u != nullptr;
    if (bias_u) r->x_dbu.upload(a->diag_bias_u, (size_t)nu, st);
    r->x_tot.alloc_at_least(nt);
    r->ids.alloc_at_least(cells);
    r->sc.alloc_at_least(cells);
    TopnExplainParams<real_t> P;
    set_items(P, r);
    P.nu = nu; P.bias = a->bias ? 1 : 0; P.n_top = a->n_top;
    P.sr = topnx_slab_rows(r->k + P.bias, a->n_top, sizeof(real_t));
    P.hist_p = r->x_hp.ptr; P.hist_i = r->x_hi.ptr; P.hist_g = r->x_g.ptr; P.hist_y = r->x_y.ptr;
    P.targ_p = r->x_tp.ptr; P.targ_i = r->x_ti.ptr;
    P.G0 = a->G0 ? r->x_g0.ptr : nullptr;
    P.diag = (real_t)a->diag; P.diag_bias = (real_t)a->diag_bias; P.diag_u = a->diag_u ? r->x_du.ptr : nullptr;
    P.diag_bias_u = bias_u ? r->x_dbu.ptr : nullptr;
    P.out_total = r->x_tot.ptr; P.out_ids = r->ids.ptr; P.out_contrib = r->sc.ptr;
    const char *cap = getenv("CMFREC_HIP_EXPLAIN_GROUPS");
    const int max_groups = (cap != nullptr && cap[0] != 0) ? atoi(cap) : 0;
    poison_lds(st, dev.num_cus);                                         // (every LDS word the kernel reads it has written)
    HIP_CHECK(hipEventRecord(r->ev0, st));
    const int grid = topn_explain_launch(st, dev.num_cus, P, max_groups);
    end_timed(r, 1, grid, 1);
    // (the targets of users [0, nu) are entries [targ_p[0], targ_p[nu]) of the outputs, as they are of targ_i)
    HIP_CHECK(hipMemcpyAsync(a->out_total + t_first, r->x_tot.ptr + t_first, (nt - t_first) * sizeof(real_t), hipMemcpyDeviceToHost, st));
    const size_t c0 = t_first * (size_t)a->n_top;
    HIP_CHECK(hipMemcpyAsync(a->out_ids + c0, r->ids.ptr + c0, (cells - c0) * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipMemcpyAsync(a->out_contrib + c0, r->sc.ptr + c0, (cells - c0) * sizeof(real_t), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    return 0;
}

// what a sampling call refuses beyond "invalid arguments" (DESIGN.md section 3.21), before a device is touched
int check_sample(const char *fn, int_t k, int_t n, int_t n_top, double temperature)
{
    if (k > TOPNW_KMAX || k <= 0 || n_top < 1 || n_top > TOPN_NMAX || n_top > n) return refuse(fn, SAMPLE_LIMITS);
    if (!(temperature >= 0.0) || !std::isfinite(temperature) || (temperature > 0.0 && !((real_t)temperature > 0 && std::isfinite((real_t)(1.0 / temperature)))))
        return refuse(fn, SAMPLE_LIMITS);
    return 0;
}

// The sampling pass over users that are on the device: the launches, the timing events and the download.  temperature == 0 is
// topn_wide_kernel itself -- the full ranking on the MFMA arithmetic for every k -- with the keys equal to the scores and a NaN
// log-partition.  The handle's split and filter settings play no part.  (the caller holds the DeviceScope and has checked the limits)
int sample_device(cmfrec_hip_ranker *r, const RankUsers &users, int_t n_top, double temperature, unsigned long long seed, bool with_lse,
                  int_t *out_ids, real_t *out_scores, real_t *out_keys, double *out_lse)
{
    const cmfrec_hip_ranker::Device &dev = r->dev;
    const int_t nu = users.nu;
    const size_t cells = (size_t)nu * n_top;
    const bool noise = temperature > 0.0;
    r->ids.alloc_at_least(cells);
    r->sc.alloc_at_least(cells);
    if (noise) r->sm_keys.alloc_at_least(cells);
    if (noise && with_lse) r->sm_lse.alloc_at_least((size_t)nu);
    int bpc = 1, nut = 1, grid = 0;
    poison_lds(dev.stream, dev.num_cus);                                 // (the policy's LDS too is written before it is read)
    HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
    if (!noise) {
        auto P = ranking_params<TopnWideParams<real_t>>(r, users);
        set_lists(P, r, n_top, true);
        nut = pick_user_tiles(nu, r->k, n_top, dev.num_cus, &bpc);
        grid = with_tiles(nut, [&](auto t) {
            return launch_tiled(dev, topn_wide_kernel<real_t, t()>, t(), topnw_lds_bytes(t(), r->k, n_top, sizeof(real_t)), P, bpc);
        });
    } else {
        auto P = ranking_params<TopnSampleParams<real_t>>(r, users);
        P.n_top = n_top; P.out_ids = r->ids.ptr; P.out_scores = r->sm_keys.ptr;
        P.temperature = (real_t)temperature; P.inv_t = (float)(1.0 / temperature); P.seed = seed;
        P.out_lse = with_lse ? r->sm_lse.ptr : nullptr;
        nut = pick_user_tiles(nu, r->k, n_top, dev.num_cus, &bpc, 16 * topnsm_extra_per_user(with_lse), sizeof(real_t),
                              topnsm_max_tiles(sizeof(real_t), with_lse));
        grid = topn_sample_launch(dev.stream, dev.num_cus, nut, bpc, P, r->sc.ptr);
    }
    end_timed(r, 16 * nut, grid, 1);
    download_and_wait(r, cells, out_ids, out_scores);                    // (and the stream is idle)
    if (out_keys) {
        if (noise) r->sm_keys.download(out_keys, cells, dev.stream);
        else r->sc.download(out_keys, cells, dev.stream);
    }
    if (with_lse && noise) r->sm_lse.download(out_lse, (size_t)nu, dev.stream);
    HIP_CHECK(hipStreamSynchronize(dev.stream));
    if (with_lse && !noise) std::fill(out_lse, out_lse + nu, std::nan(""));
    return 0;
}

// a ranker of its own on the current device for one call
template <class F>
int with_ranker(const real_t *B, size_t ldb, int_t n, int_t k, const real_t *biasB, F &&call)
{
    cmfrec_hip_ranker *r = cmfrec_hip_ranker_create(B, ldb, n, k, biasB, -1);
    if (r == nullptr) return g_last_rc;
    const int rc = call(r);
    cmfrec_hip_ranker_destroy(r);
    return rc;
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
    const RankUsers users{dA, lda, set->nu, set->has_excl ? set->excl_p.ptr : nullptr, set->has_excl ? set->excl_i.ptr : nullptr};
    if (int rc = ranks_device(r, users, set->total, set->max_held, nullptr, nullptr, nullptr, set->held_p.ptr, set->held_i.ptr, true)) return rc;
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
        r->fimg.ready = false;                               // (and their image)
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
    const char *fn = "cmfrec_hip_ranker_topN";
    return guarded([&]() {
        if (bad_users(r, A, lda, nu, excl_p, excl_i) || n_top <= 0 || !out_ids) return refuse(fn, "invalid arguments");
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        const size_t k = (size_t)r->k;
        RankUsers users = stage_users(r, A, lda, nu);
        stage_exclusions(r, users, excl_p, excl_i);
        r->fs_valid = true; r->fs_users = nu; r->fs_filtered = 0; r->fs_certified = 0;
        // the filter: n_top <= 64 of a ranker that is not split and whose items have an image; everything else as it always was
        if (r->filter != 1 || n_top > TOPNF_NTOP_MAX || r->split >= 0 || !ensure_filter_image(r))
            return rank_device(r, users, n_top, out_ids, out_scores);
        std::vector<int> cert((size_t)nu);
        if (int rc = rank_device_filtered(r, users, n_top, out_ids, out_scores, cert.data())) return rc;
        // the users without a certificate: one batch on the exact route, their rows scattered into the result
        std::vector<int_t> rest;
        for (int_t u = 0; u < nu; u++)
            if (!cert[u]) rest.push_back(u);
        r->fs_filtered = nu; r->fs_certified = nu - (int)rest.size();
        if (rest.empty()) return 0;
        const size_t nr = rest.size();
        std::vector<real_t> Ar(nr * k), sr(out_scores ? nr * (size_t)n_top : 0);
        std::vector<int_t> ir(nr * (size_t)n_top), xi;
        std::vector<size_t> xp(excl_p ? nr + 1 : 0, 0);
        for (size_t j = 0; j < nr; j++) {
            const int_t u = rest[j];
            memcpy(&Ar[j * k], A + (size_t)u * lda, k * sizeof(real_t));
            if (excl_p) {
                xi.insert(xi.end(), excl_i + excl_p[u], excl_i + excl_p[u + 1]);
                xp[j + 1] = xi.size();
            }
        }
        users = stage_users(r, Ar.data(), k, (int_t)nr);
        stage_exclusions(r, users, excl_p ? xp.data() : nullptr, xi.data());
        if (int rc = rank_device(r, users, n_top, ir.data(), out_scores ? sr.data() : nullptr))
            return rc;                                       // (rank_device has waited for the stream: the vectors may go)
        for (size_t j = 0; j < nr; j++) {
            memcpy(out_ids + (size_t)rest[j] * n_top, &ir[j * (size_t)n_top], (size_t)n_top * sizeof(int_t));
            if (out_scores) memcpy(out_scores + (size_t)rest[j] * n_top, &sr[j * (size_t)n_top], (size_t)n_top * sizeof(real_t));
        }
        return 0;
    });
}

int cmfrec_hip_ranker_set_filter(cmfrec_hip_ranker *r, int mode)
{
    return guarded([&]() {
        if (r == nullptr || (mode != 0 && mode != 1)) {
            g_last_error = "cmfrec_hip_ranker_set_filter: invalid arguments (0: off, 1: the half-precision filter)";
            return 2;
        }
        DeviceScope scope(r->dev.device);
        r->filter = mode;
        if (mode == 0) r->fimg.release();
        else (void)ensure_filter_image(r);
        return 0;
    });
}

int cmfrec_hip_ranker_filter_stats(cmfrec_hip_ranker *r, int *users, int *filtered, int *certified)
{
    if (r == nullptr || !r->fs_valid) {
        g_last_error = "cmfrec_hip_ranker_filter_stats: no cmfrec_hip_ranker_topN call on this handle yet";
        return 2;
    }
    if (users) *users = r->fs_users;
    if (filtered) *filtered = r->fs_filtered;
    if (certified) *certified = r->fs_certified;
    return 0;
}

int cmfrec_hip_ranker_filter_ms(cmfrec_hip_ranker *r, double ms[4])
{
    if (r == nullptr || ms == nullptr || r->filter != 1 || !r->fimg.ready) {
        g_last_error = "cmfrec_hip_ranker_filter_ms: the filter of this handle is off";
        return 2;
    }
    ms[0] = r->fimg.usable ? r->fimg.build_ms : 0.0;
    for (int s = 0; s < 3; s++) ms[s + 1] = r->fs_filtered > 0 ? r->f_ms[s] : 0.0;
    return 0;
}

int cmfrec_hip_ranker_filter_keys(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, float *keys_out)
{
    const char *fn = "cmfrec_hip_ranker_filter_keys";
    return guarded([&]() {
        if (bad_users(r, A, lda, nu) || !keys_out) return refuse(fn, "invalid arguments");
        if ((size_t)nu * (size_t)r->n > ((size_t)1 << 20)) return refuse(fn, "a probe for small shapes, needs nu * n <= 2^20");
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        if (r->filter != 1 || !ensure_filter_image(r)) return refuse(fn, "the filter of this handle is off, or its items have no image");
        const cmfrec_hip_ranker::Device &dev = r->dev;
        const size_t cells = (size_t)nu * (size_t)r->n;
        const RankUsers users = stage_users(r, A, lda, nu);
        r->f_keys.alloc_at_least(cells);
        TopnFilterParams<real_t> F = filter_params(r, users, TOPNF_M_MIN);
        F.keys = r->f_keys.ptr;
        topn_filter_launch_keys(dev.stream, dev.num_cus, F);
        r->f_keys.download(keys_out, cells, dev.stream);
        HIP_CHECK(hipStreamSynchronize(dev.stream));
        return 0;
    });
}

int cmfrec_hip_ranker_topN_candidates(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t cand_p[], const int_t cand_i[],
                                      const size_t excl_p[], const int_t excl_i[], int_t n_top, int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_ranker_topN_candidates";
    return guarded([&]() {
        if (bad_users(r, A, lda, nu, excl_p, excl_i) || n_top <= 0 || !out_ids || !cand_p) return refuse(fn, "invalid arguments");
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        if (int rc = upload_candidates(r, fn, nu, cand_p, cand_i)) return rc;
        RankUsers users = stage_users(r, A, lda, nu);
        stage_exclusions(r, users, excl_p, excl_i);
        return rank_device(r, users, n_top, out_ids, out_scores, r->cp.ptr, r->ci.ptr);
    });
}

int cmfrec_hip_ranker_topN_deep(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t excl_p[], const int_t excl_i[],
                                int_t n_top, int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_ranker_topN_deep";
    return guarded([&]() {
        if (r != nullptr && (n_top < 1 || n_top > r->n)) return refuse(fn, DEEP_LIMITS);
        if (bad_users(r, A, lda, nu, excl_p, excl_i) || !out_ids) return refuse(fn, "invalid arguments");
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        RankUsers users = stage_users(r, A, lda, nu);
        stage_exclusions(r, users, excl_p, excl_i);
        const int len = pick_page_len(r->k, n_top);
        int pages = 0;
        if (int rc = rank_device_deep(r, users, n_top, len, nullptr, nullptr, out_ids, out_scores, &pages)) return rc;
        r->last_pages = pages; r->last_page_len = len;
        return 0;
    });
}

int cmfrec_hip_ranker_topN_after(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t excl_p[], const int_t excl_i[],
                                 const int_t *after_ids, const real_t *after_scores, int_t n_top, int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_ranker_topN_after";
    return guarded([&]() {
        if (bad_users(r, A, lda, nu, excl_p, excl_i) || n_top <= 0 || !out_ids || (after_ids == nullptr) != (after_scores == nullptr))
            return refuse(fn, "invalid arguments");
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        RankUsers users = stage_users(r, A, lda, nu);
        stage_exclusions(r, users, excl_p, excl_i);
        if (after_ids) {
            r->cur_s.upload(after_scores, (size_t)nu, r->dev.stream);
            r->cur_i.upload(after_ids, (size_t)nu, r->dev.stream);
        }
        return rank_device_deep(r, users, n_top, (int)n_top, after_ids ? r->cur_s.ptr : nullptr, after_ids ? r->cur_i.ptr : nullptr, out_ids,
                                out_scores, nullptr);
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
        if (bad_users(r, A, lda, nu, excl_p, excl_i) || !held_p || (held_p[nu] > 0 && !out_rank)) return refuse(fn, "invalid arguments");
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        size_t max_held = 0;
        if (int rc = upload_held(r, fn, nu, held_p, held_i, &max_held)) return rc;
        RankUsers users = stage_users(r, A, lda, nu);
        stage_exclusions(r, users, excl_p, excl_i);
        return ranks_device(r, users, held_p[nu], max_held, out_rank, out_scores, out_pool);
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
        if (r == nullptr || nq < 0 || n_top <= 0 || (nq > 0 && (!query_ids || !out_ids))) return refuse(fn, "invalid arguments");
        if (metric != TOPNS_DOT && metric != TOPNS_COSINE)
            return refuse(fn, "metric must be 0 (dot product) or 1 (cosine), got " + std::to_string(metric));
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        for (int_t q = 0; q < nq; q++)
            if (query_ids[q] < 0 || query_ids[q] >= r->n)
                return refuse(fn, "query id " + std::to_string(query_ids[q]) + " (entry " + std::to_string(q) + ") is not a row of the ranker's " +
                                      std::to_string(r->n));
        if (excl_p != nullptr && !csr_ok(excl_p, excl_i, nq))
            return refuse(fn, "invalid arguments (the exclusion lists are not a CSR over the queries)");
        if (nq == 0) return 0;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        const cmfrec_hip_ranker::Device &dev = r->dev;
        r->qid.upload(query_ids, (size_t)nq, dev.stream);
        RankUsers queries{nullptr, 0, nq, nullptr, nullptr};
        stage_exclusions(r, queries, excl_p, excl_i);
        if (metric == TOPNS_COSINE) ensure_inverse_norms(r);             // outside the timed interval
        const size_t cells = (size_t)nq * n_top;
        r->ids.alloc_at_least(cells);
        if (out_scores) r->sc.alloc_at_least(cells);
        TopnSimilarParams<real_t> P;
        set_items(P, r); set_exclusions(P, queries); set_lists(P, r, n_top, out_scores != nullptr);
        P.query_ids = r->qid.ptr; P.nu = nq;
        P.rn = metric == TOPNS_COSINE ? r->rn.ptr : nullptr;
        int bpc = 1;
        const int nut = pick_user_tiles(nq, r->k, n_top, dev.num_cus, &bpc, 16 * (sizeof(real_t) + sizeof(int)));
        poison_lds(dev.stream, dev.num_cus);                             // (the policy's LDS too is written before it is read)
        HIP_CHECK(hipEventRecord(r->ev0, dev.stream));
        auto launch = [&](auto m) {
            return with_tiles(nut, [&](auto t) {
                return launch_tiled(dev, topn_similar_kernel<real_t, t(), m()>, t(), topns_lds_bytes(t(), P.k, P.n_top, sizeof(real_t)), P, bpc);
            });
        };
        const int grid = metric == TOPNS_COSINE ? launch(std::integral_constant<int, TOPNS_COSINE>()) : launch(std::integral_constant<int, TOPNS_DOT>());
        end_timed(r, 16 * nut, grid, 1);
        download_and_wait(r, cells, out_ids, out_scores);
        return 0;
    });
}

int cmfrec_hip_ranker_rerank_mmr(cmfrec_hip_ranker *r, int_t nu, int_t pool, const int_t *pool_ids, const real_t *pool_scores, double theta,
                                 int_t n_top, int_t *out_ids, real_t *out_scores, real_t *out_mmr)
{
    const char *fn = "cmfrec_hip_ranker_rerank_mmr";
    return guarded([&]() {
        if (r == nullptr || nu <= 0 || !pool_ids || !pool_scores || !out_ids || !out_scores)
            return refuse(fn, std::string("invalid arguments; ") + MMR_LIMITS);
        if (int rc = check_mmr(fn, r->k, r->n, pool, n_top, theta)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        const size_t cells = (size_t)nu * (size_t)pool;
        r->ids.upload(pool_ids, cells, r->dev.stream);
        r->sc.upload(pool_scores, cells, r->dev.stream);
        return mmr_device(r, nu, pool, theta, n_top, out_ids, out_scores, out_mmr);
    });
}

int cmfrec_hip_ranker_topN_diverse(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t excl_p[], const int_t excl_i[],
                                   int_t pool, double theta, int_t n_top, int_t *out_ids, real_t *out_scores, real_t *out_mmr)
{
    const char *fn = "cmfrec_hip_ranker_topN_diverse";
    return guarded([&]() {
        if (bad_users(r, A, lda, nu, excl_p, excl_i) || !out_ids || !out_scores) return refuse(fn, std::string("invalid arguments; ") + MMR_LIMITS);
        if (int rc = check_mmr(fn, r->k, r->n, pool, n_top, theta)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        RankUsers users = stage_users(r, A, lda, nu);
        stage_exclusions(r, users, excl_p, excl_i);
        // the pool: the full ranking of n_top = pool by the handle's exact route (a filtered handle's certified lists are these
        // lists bit for bit), left on the device
        if (int rc = rank_device(r, users, pool, nullptr, nullptr, nullptr, nullptr, true)) return rc;
        return mmr_device(r, nu, pool, theta, n_top, out_ids, out_scores, out_mmr);
    });
}

int cmfrec_hip_ranker_topN_sample(cmfrec_hip_ranker *r, const real_t *A, size_t lda, int_t nu, const size_t excl_p[], const int_t excl_i[],
                                  int_t n_top, double temperature, uint64_t seed, int with_lse, int_t *out_ids, real_t *out_scores,
                                  real_t *out_keys, double *out_lse)
{
    const char *fn = "cmfrec_hip_ranker_topN_sample";
    return guarded([&]() {
        if (bad_users(r, A, lda, nu, excl_p, excl_i) || !out_ids || (with_lse && !out_lse)) return refuse(fn, std::string("invalid arguments; ") + SAMPLE_LIMITS);
        if (int rc = check_sample(fn, r->k, r->n, n_top, temperature)) return rc;
        if (excl_p != nullptr && !csr_ok(excl_p, excl_i, nu)) return refuse(fn, "invalid arguments (the exclusion lists are not a CSR over the users)");
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        RankUsers users = stage_users(r, A, lda, nu);
        stage_exclusions(r, users, excl_p, excl_i);
        return sample_device(r, users, n_top, temperature, (unsigned long long)seed, with_lse != 0, out_ids, out_scores, out_keys, out_lse);
    });
}

int cmfrec_hip_ranker_explain(cmfrec_hip_ranker *r, const cmfrec_hip_explain_args *args)
{
    const char *fn = "cmfrec_hip_ranker_explain";
    return guarded([&]() {
        if (r == nullptr) return refuse(fn, std::string("invalid arguments; ") + EXPLAIN_LIMITS);
        if (int rc = check_explain(fn, r->n, r->k, args)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        return explain_device(r, args);
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
    const char *fn = "cmfrec_hip_topN_batch";
    if (nu <= 0 || n <= 0 || k <= 0 || n_top <= 0 || !A || !B || !out_ids) return refuse(fn, "invalid arguments");
    if (int rc = ranker_check_limits(fn, k, n_top, n)) return rc;
    return with_ranker(B, ldb, n, k, biasB, [&](cmfrec_hip_ranker *r) {
        return cmfrec_hip_ranker_topN(r, A, lda, nu, excl_p, excl_i, n_top, out_ids, out_scores);
    });
}

int cmfrec_hip_topN_deep_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k,
                               const real_t *biasB, const size_t excl_p[], const int_t excl_i[], int_t n_top,
                               int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_topN_deep_batch";
    if (nu <= 0 || n <= 0 || k <= 0 || !A || !B) return refuse(fn, "invalid arguments");
    if (k > TOPNW_KMAX || n_top < 1 || n_top > n) return refuse(fn, DEEP_LIMITS);
    if (!out_ids) return refuse(fn, "invalid arguments");
    return with_ranker(B, ldb, n, k, biasB, [&](cmfrec_hip_ranker *r) {
        return cmfrec_hip_ranker_topN_deep(r, A, lda, nu, excl_p, excl_i, n_top, out_ids, out_scores);
    });
}

int cmfrec_hip_topN_diverse_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k, const real_t *biasB,
                                  const size_t excl_p[], const int_t excl_i[], int_t pool, double theta, int_t n_top, int_t *out_ids,
                                  real_t *out_scores, real_t *out_mmr)
{
    const char *fn = "cmfrec_hip_topN_diverse_batch";
    if (nu <= 0 || n <= 0 || k <= 0 || !A || !B || !out_ids || !out_scores) return refuse(fn, std::string("invalid arguments; ") + MMR_LIMITS);
    if (int rc = check_mmr(fn, k, n, pool, n_top, theta)) return rc;
    return with_ranker(B, ldb, n, k, biasB, [&](cmfrec_hip_ranker *r) {
        return cmfrec_hip_ranker_topN_diverse(r, A, lda, nu, excl_p, excl_i, pool, theta, n_top, out_ids, out_scores, out_mmr);
    });
}

int cmfrec_hip_topN_sample_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k, const real_t *biasB,
                                 const size_t excl_p[], const int_t excl_i[], int_t n_top, double temperature, uint64_t seed, int with_lse,
                                 int_t *out_ids, real_t *out_scores, real_t *out_keys, double *out_lse)
{
    const char *fn = "cmfrec_hip_topN_sample_batch";
    if (nu <= 0 || n <= 0 || k <= 0 || !A || !B || !out_ids || (with_lse && !out_lse)) return refuse(fn, std::string("invalid arguments; ") + SAMPLE_LIMITS);
    if (int rc = check_sample(fn, k, n, n_top, temperature)) return rc;
    return with_ranker(B, ldb, n, k, biasB, [&](cmfrec_hip_ranker *r) {
        return cmfrec_hip_ranker_topN_sample(r, A, lda, nu, excl_p, excl_i, n_top, temperature, seed, with_lse, out_ids, out_scores, out_keys, out_lse);
    });
}

int cmfrec_hip_explain_batch(const real_t *B, size_t ldb, int_t n, int_t k, const cmfrec_hip_explain_args *args)
{
    const char *fn = "cmfrec_hip_explain_batch";
    if (n <= 0 || k <= 0 || !B) return refuse(fn, std::string("invalid arguments; ") + EXPLAIN_LIMITS);
    if (int rc = check_explain(fn, n, k, args)) return rc;
    return with_ranker(B, ldb, n, k, nullptr, [&](cmfrec_hip_ranker *r) { return cmfrec_hip_ranker_explain(r, args); });
}

int cmfrec_hip_topN_candidates_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k,
                                     const real_t *biasB, const size_t cand_p[], const int_t cand_i[], const size_t excl_p[],
                                     const int_t excl_i[], int_t n_top, int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_topN_candidates_batch";
    if (nu <= 0 || n <= 0 || k <= 0 || n_top <= 0 || !A || !B || !out_ids || !cand_p) return refuse(fn, "invalid arguments");
    if (int rc = ranker_check_limits(fn, k, n_top, n)) return rc;
    return with_ranker(B, ldb, n, k, biasB, [&](cmfrec_hip_ranker *r) {
        return cmfrec_hip_ranker_topN_candidates(r, A, lda, nu, cand_p, cand_i, excl_p, excl_i, n_top, out_ids, out_scores);
    });
}

int cmfrec_hip_similar_batch(const real_t *B, size_t ldb, int_t n, int_t k, const int_t *query_ids, int_t nq, int metric, const size_t excl_p[],
                             const int_t excl_i[], int_t n_top, int_t *out_ids, real_t *out_scores)
{
    const char *fn = "cmfrec_hip_similar_batch";
    if (n <= 0 || k <= 0 || nq < 0 || n_top <= 0 || !B) return refuse(fn, "invalid arguments");
    if (int rc = ranker_check_limits(fn, k, n_top, n)) return rc;
    return with_ranker(B, ldb, n, k, nullptr, [&](cmfrec_hip_ranker *r) {
        return cmfrec_hip_ranker_similar(r, query_ids, nq, metric, excl_p, excl_i, n_top, out_ids, out_scores);
    });
}

int cmfrec_hip_ranks_batch(const real_t *A, size_t lda, int_t nu, const real_t *B, size_t ldb, int_t n, int_t k, const real_t *biasB,
                           const size_t held_p[], const int_t held_i[], const size_t excl_p[], const int_t excl_i[],
                           int_t *out_rank, real_t *out_scores, int_t *out_pool)
{
    const char *fn = "cmfrec_hip_ranks_batch";
    if (nu <= 0 || n <= 0 || k <= 0 || !A || !B || !held_p) return refuse(fn, "invalid arguments");
    if (k > TOPNW_KMAX) return refuse(fn, RANK_LIMITS);
    return with_ranker(B, ldb, n, k, biasB, [&](cmfrec_hip_ranker *r) {
        return cmfrec_hip_ranker_ranks(r, A, lda, nu, held_p, held_i, excl_p, excl_i, out_rank, out_scores, out_pool);
    });
}

}  // extern "C"

namespace cmfhip {

int ranker_check_limits(const char *fn, int_t k, int_t n_top, int_t n)
{
    if (k > TOPNW_KMAX || k <= 0) return refuse(fn, LIMITS);
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
        if (bad_users(r, dA, lda, nu) || n_top <= 0 || !out_ids) return refuse(fn, "invalid arguments");
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        return rank_device(r, RankUsers{dA, lda, nu, dexcl_p, dexcl_i}, n_top, out_ids, out_scores);
    });
}

int ranker_topN_candidates_device(cmfrec_hip_ranker *r, const char *fn, const real_t *dA, size_t lda, int_t nu, const size_t cand_p[],
                                  const int_t cand_i[], const size_t *dexcl_p, const int *dexcl_i, int_t n_top, int_t *out_ids,
                                  real_t *out_scores)
{
    return guarded([&]() {
        if (bad_users(r, dA, lda, nu) || n_top <= 0 || !out_ids || !cand_p) return refuse(fn, "invalid arguments");
        if (int rc = check_n_top(fn, n_top, r->n)) return rc;
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        if (int rc = upload_candidates(r, fn, nu, cand_p, cand_i)) return rc;
        return rank_device(r, RankUsers{dA, lda, nu, dexcl_p, dexcl_i}, n_top, out_ids, out_scores, r->cp.ptr, r->ci.ptr);
    });
}

int ranker_ranks_device(cmfrec_hip_ranker *r, const char *fn, const real_t *dA, size_t lda, int_t nu, const size_t held_p[],
                        const int_t held_i[], const size_t *dexcl_p, const int *dexcl_i, int_t *out_rank, real_t *out_scores,
                        int_t *out_pool)
{
    return guarded([&]() {
        if (bad_users(r, dA, lda, nu) || !held_p || (held_p[nu] > 0 && !out_rank)) return refuse(fn, "invalid arguments");
        DeviceScope scope(r->dev.device);
        switches_mut().reload();
        size_t max_held = 0;
        if (int rc = upload_held(r, fn, nu, held_p, held_i, &max_held)) return rc;
        return ranks_device(r, RankUsers{dA, lda, nu, dexcl_p, dexcl_i}, held_p[nu], max_held, out_rank, out_scores, out_pool);
    });
}

}  // namespace cmfhip

