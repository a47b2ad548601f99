// subspace_tu.hip -- the instantiations of subspace_rows_kernel (subspace_kernels.hpp) and their launch: launch_subspace, behind
// cmfrec_hip_session_set_subspace.  DESIGN.md section 3.22.
#include <algorithm>
#include <cstdlib>

#include "launch.hpp"
#include "subspace_kernels.hpp"

namespace cmfhip {

namespace {

// CMFREC_HIP_SUBSPACE_LDS_ROWS / CMFREC_HIP_SUBSPACE_WAVES: test hooks, read per call
int env_int(const char *name)
{
    const char *v = getenv(name);
    return (v != nullptr && v[0] != 0) ? atoi(v) : 0;
}

// the positions [first, end) of the processing order on teams of NW wavefronts
template <int NW, bool VEC>
int launch_rows(const DeviceInfo &dev, SubspaceParams<real_t> P, int first, int end, int cap_hook, int max_waves)
{
    if (end <= first) return 0;
    constexpr int TEAMS = SUB_TH / (64 * NW);
    const size_t smem = (size_t)TEAMS * subspace_team_elems<real_t, NW>((P.k + 15) / 16 * 16) * sizeof(real_t);
    if (smem > 64 * 1024) {
        g_last_error = "cmfrec_hip: the subspace solver fits k + k_main (+ 1) <= 272";
        return 2;
    }
    P.row_first = first; P.row_end = end;
    P.cap = subspace_cap_max<NW>();
    if (cap_hook > 0) P.cap = std::min(P.cap, std::max(4, cap_hook & ~3));
    auto kernel = subspace_rows_kernel<real_t, NW, VEC>;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, SUB_TH, smem) != hipSuccess || per_cu < 1) per_cu = 1;
    size_t grid = std::min<size_t>(((size_t)(end - first) + TEAMS - 1) / TEAMS, (size_t)dev.num_cus * (size_t)per_cu);
    if (max_waves > 0) grid = std::min<size_t>(grid, ((size_t)max_waves + SUB_TH / 64 - 1) / (SUB_TH / 64));
    hipLaunchKernelGGL(kernel, dim3((unsigned)std::max<size_t>(grid, 1)), dim3(SUB_TH), smem, dev.stream, P);
    return 0;
}

template <bool VEC>
int launch_both(const DeviceInfo &dev, const SubspaceParams<real_t> &P, const SparseShard &X, int cap_hook, int max_waves)
{
    // the rows of more than SUB_WAVE_ROW entries lead the processing order
    const int n_long = X.rows_longer_than(SUB_WAVE_ROW, X.n_nonempty);
    if (const int rc = launch_rows<4, VEC>(dev, P, 0, n_long, cap_hook, max_waves)) return rc;
    return launch_rows<1, VEC>(dev, P, n_long, X.n_nonempty, cap_hook, max_waves);
}

}  // namespace

int launch_subspace(const DeviceInfo &dev, const SubspaceCall &c, const SparseShard &X, DevBuf<real_t> &yhat)
{
    if (X.n_nonempty == 0) return 0;
    const int cap_hook = env_int("CMFREC_HIP_SUBSPACE_LDS_ROWS"), max_waves = env_int("CMFREC_HIP_SUBSPACE_WAVES");
    yhat.alloc_at_least(std::max<size_t>(X.nnz, 1));
    SubspaceParams<real_t> P;
    P.A = c.A; P.lda = c.lda; P.B = c.B; P.ldb = c.ldb; P.k = c.k;
    P.indices = X.i.ptr; P.values = X.v.ptr; P.bias_sub = c.bias_sub; P.G0 = c.G0;
    P.lam = c.lam; P.lam_last = c.lam_last; P.implicit = c.G0 != nullptr; P.sweeps = c.sweeps;
    P.desc = X.desc.ptr; P.yhat = yhat.ptr;
    const int rc = score_wide_ok(c.B, c.ldb) ? launch_both<true>(dev, P, X, cap_hook, max_waves) : launch_both<false>(dev, P, X, cap_hook, max_waves);
    if (rc) return rc;
    HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace cmfhip
