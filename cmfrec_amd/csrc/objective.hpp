// objective.hpp -- what session.hip asks of objective_tu.hip: one evaluation of the objective's components on factors and a CSR
// that are on the device (cmfrec_hip_session_objective).  No kernels here.
#pragma once
#include "device_base.hpp"

namespace cmfhip {

struct ObjectiveWorkspace;        // work items, records, Gramian partials: grows on demand, owned by the session

struct ObjectiveCall {
    int device = 0, num_cus = 0;
    hipStream_t stream = nullptr;
    bool implicit = false;
    int kk = 0;                                       // k + k_main: the columns both sides share
    const real_t *A = nullptr; size_t ldA = 0; int m = 0, k_user = 0; const real_t *biasA = nullptr;
    const real_t *B = nullptr; size_t ldB = 0; int n = 0, k_item = 0; const real_t *biasB = nullptr;
    size_t nnz = 0;
    const size_t *csr_p = nullptr; const int *csr_i = nullptr;      // X by rows: indptr [m + 1], item index, value, weight or null
    const real_t *csr_v = nullptr, *csr_w = nullptr;
    const real_t *wsum_rows = nullptr;                // lambda's multipliers of the rows under scale_lam, or null: their entry counts
    const size_t *csc_p = nullptr;                    // X by columns: indptr [n + 1] alone
    const real_t *wsum_cols = nullptr;
};

// Runs behind what is queued on c.stream, downloads the record and waits for it.  Throws HipError (call inside guarded()).
int objective_run(ObjectiveWorkspace *&ws, const ObjectiveCall &c, cmfrec_hip_objective *out);
void objective_workspace_destroy(ObjectiveWorkspace *ws);

}  // namespace cmfhip
