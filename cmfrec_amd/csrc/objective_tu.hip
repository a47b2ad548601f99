// objective_tu.hip -- the kernels of objective_kernels.hpp and their launches: one evaluation of the components of the training
// objective (objective_run, behind cmfrec_hip_session_objective), and the host function that composes the number from them
// (cmfrec_hip_objective_value).  DESIGN.md section 3.18.
#include <algorithm>
#include <cstdlib>

#include "objective.hpp"
#include "objective_kernels.hpp"

namespace cmfhip {

struct ObjectiveWorkspace {
    DevBuf<unsigned long long> item_off;
    DevBuf<double> records, part_a, part_b, pair_dot, out;
};

void objective_workspace_destroy(ObjectiveWorkspace *ws) { delete ws; }

namespace {

// CMFREC_HIP_OBJ_SEGMENT / CMFREC_HIP_OBJ_WAVES: test hooks, read per call
int env_int(const char *name)
{
    const char *v = getenv(name);
    return (v != nullptr && v[0] != 0) ? atoi(v) : 0;
}

template <typename K>
size_t launch_rows_kernel(K kernel, const ObjectiveCall &c, size_t items_bound, int max_waves, const ObjParams<real_t> &P, bool dry)
{
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, OBJ_TH, 0) != hipSuccess || per_cu < 1) per_cu = 4;
    size_t grid = std::min<size_t>((items_bound + OBJ_TH / 64 - 1) / (OBJ_TH / 64), (size_t)c.num_cus * (size_t)per_cu);
    if (max_waves > 0) grid = std::min<size_t>(grid, ((size_t)max_waves + OBJ_TH / 64 - 1) / (OBJ_TH / 64));
    grid = std::max<size_t>(grid, 1);
    if (!dry) hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(OBJ_TH), 0, c.stream, P);
    return grid * (OBJ_TH / 64);
}

template <bool IMPLICIT, bool VEC>
size_t launch_rows_width(int G, int C, const ObjectiveCall &c, size_t items_bound, int max_waves, const ObjParams<real_t> &P, bool dry)
{
#define OBJ_CASE(g, cc) return launch_rows_kernel(objective_rows_kernel<real_t, IMPLICIT, g, cc, VEC>, c, items_bound, max_waves, P, dry)
    switch (G) {
    case 1: OBJ_CASE(1, 1);
    case 2: OBJ_CASE(2, 1);
    case 4: OBJ_CASE(4, 1);
    case 8: OBJ_CASE(8, 1);
    case 16: OBJ_CASE(16, 1);
    case 32: OBJ_CASE(32, 1);
    default: break;
    }
    if (C == 1) OBJ_CASE(64, 1);
    if (C == 2) OBJ_CASE(64, 2);
    OBJ_CASE(64, 3);
#undef OBJ_CASE
}

// the wavefronts of the launch; dry: nothing is launched (the caller sizes the records first)
size_t launch_rows(const ObjectiveCall &c, size_t items_bound, int max_waves, const ObjParams<real_t> &P, bool dry)
{
    const int pieces = (c.kk + score_ve<real_t>() - 1) / score_ve<real_t>();
    const int G = score_group_width<real_t>(c.kk), C = std::max(1, (pieces + 63) / 64);
    const bool vec = score_wide_ok(P.a.F + P.a.k_side, P.a.ld) && score_wide_ok(P.b.F + P.b.k_side, P.b.ld);
    if (c.implicit) return vec ? launch_rows_width<true, true>(G, C, c, items_bound, max_waves, P, dry)
                               : launch_rows_width<true, false>(G, C, c, items_bound, max_waves, P, dry);
    return vec ? launch_rows_width<false, true>(G, C, c, items_bound, max_waves, P, dry)
               : launch_rows_width<false, false>(G, C, c, items_bound, max_waves, P, dry);
}

// slab partials of M^T M on kk columns: at most GRAM64_MAX_SLABS slabs of at least 1024 rows; returns their number
constexpr int GRAM64_MAX_SLABS = 128;
int launch_gram64(const ObjectiveCall &c, const real_t *M, size_t ld, int rows, DevBuf<double> &part)
{
    const int nt = gram64_tiles(c.kk);
    int slab = std::max(1024, (rows + GRAM64_MAX_SLABS - 1) / GRAM64_MAX_SLABS);
    slab = (slab + 3) / 4 * 4;
    const int slabs = (rows + slab - 1) / slab;
    part.alloc_at_least((size_t)slabs * gram64_pairs(nt) * 256);
    hipLaunchKernelGGL(gram_f64acc_kernel<real_t>, dim3((unsigned)slabs, (unsigned)nt), dim3(GRAM64_TH), 0, c.stream, M, ld, rows, c.kk, slab,
                       part.ptr);
    return slabs;
}

}  // namespace

int objective_run(ObjectiveWorkspace *&ws, const ObjectiveCall &c, cmfrec_hip_objective *out)
{
    if (ws == nullptr) ws = new ObjectiveWorkspace();
    const int seg = env_int("CMFREC_HIP_OBJ_SEGMENT") > 0 ? env_int("CMFREC_HIP_OBJ_SEGMENT") : OBJ_SEGMENT;
    const int max_waves = env_int("CMFREC_HIP_OBJ_WAVES");
    ObjParams<real_t> P;
    P.a.F = c.A; P.a.ld = c.ldA; P.a.rows = c.m; P.a.k_side = c.k_user; P.a.bias = c.biasA; P.a.p = c.csr_p; P.a.wsum = c.wsum_rows;
    P.b.F = c.B; P.b.ld = c.ldB; P.b.rows = c.n; P.b.k_side = c.k_item; P.b.bias = c.biasB; P.b.p = c.csc_p; P.b.wsum = c.wsum_cols;
    P.kk = c.kk; P.idx = c.csr_i; P.v = c.csr_v; P.w = c.csr_w; P.seg = seg;
    // (an upper bound of the work items is enough to size the launch: the kernel reads their number from item_off)
    const size_t items_bound = (size_t)c.m + c.nnz / (size_t)seg + (size_t)c.n;
    const size_t waves = launch_rows(c, items_bound, max_waves, P, true);
    ws->item_off.alloc_at_least((size_t)c.m + 1);
    ws->records.alloc_at_least(waves * OBJ_FIELDS);
    ws->out.alloc_at_least(OBJ_FIELDS + 1);
    P.item_off = ws->item_off.ptr; P.records = ws->records.ptr;
    hipLaunchKernelGGL(objective_items_kernel, dim3(1), dim3(OBJ_ITEMS_TH), 0, c.stream, c.csr_p, c.m, seg, ws->item_off.ptr);
    launch_rows(c, items_bound, max_waves, P, false);
    int npairs = 0;
    if (c.implicit) {
        // both Gramians anew on every evaluation: a precomputed one may be older than the last update of its matrix
        const int nt = gram64_tiles(c.kk);
        npairs = gram64_pairs(nt);
        const int slabs_a = launch_gram64(c, c.A + c.k_user, c.ldA, c.m, ws->part_a);
        const int slabs_b = launch_gram64(c, c.B + c.k_item, c.ldB, c.n, ws->part_b);
        ws->pair_dot.alloc_at_least((size_t)npairs);
        hipLaunchKernelGGL(gram_inner_kernel, dim3((unsigned)npairs), dim3(256), 0, c.stream, ws->part_a.ptr, slabs_a, ws->part_b.ptr, slabs_b,
                           nt, ws->pair_dot.ptr);
    }
    hipLaunchKernelGGL(objective_reduce_kernel, dim3(1), dim3(OBJ_REDUCE_TH), 0, c.stream, ws->records.ptr, waves, ws->pair_dot.ptr, npairs,
                       ws->out.ptr);
    HIP_CHECK(hipGetLastError());
    cmfrec_hip_objective rec;
    HIP_CHECK(hipMemcpyAsync(&rec, ws->out.ptr, sizeof rec, hipMemcpyDeviceToHost, c.stream));
    HIP_CHECK(hipStreamSynchronize(c.stream));
    *out = rec;
    return 0;
}

}  // namespace cmfhip

extern "C" {

/* the objective from its components (include/cmfrec_hip.h); host only */
double cmfrec_hip_objective_value(const cmfrec_hip_objective *rec, const double *lam6, double w_main, int scale_lam, int scale_bias_const)
{
    if (rec == nullptr || lam6 == nullptr) return 0. / 0.;
    const int s = scale_lam ? 1 : 0, sb = (scale_lam && !scale_bias_const) ? 1 : 0;
    const double penalty = lam6[2] * rec->normA[s] + lam6[3] * rec->normB[s] + lam6[0] * rec->normbiasA[sb] + lam6[1] * rec->normbiasB[sb];
    return 0.5 * w_main * (rec->data + rec->allpairs) + 0.5 * penalty;
}

}  // extern "C"
