// fit.hip -- the two drop-in fit entry points (level 1 of include/cmfrec_hip.h).
//
// Host-side restatement of the driver logic of the reference's fit_collective_implicit_als
// (/root/reference/src/collective.c:9375-10207) and fit_collective_explicit_als (:7263-9370) for
// the supported option set: input validation, log transform, global mean (common.c:3423-3648), side-info column centering
// (common.c:4911-4997), start values; X := (X - mean)*alpha, COO -> CSR + CSC (stable, helpers.c:1375-1491)
// and the bias initialisation (common.c:4410-4909) run on the device (coo_device.hpp); the ALS loop
// order C -> D -> B -> A, which runs on the device-resident session (session.hip).  Every
// temporary is allocated and freed here; outputs are caller-allocated (cmfrec.h.in:240-241).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <csignal>
#include <cstdio>
#include <cstring>
#include <chrono>
#include <cstdlib>
#include <functional>
#include <vector>
#include <dlfcn.h>
#include <set>
#include <string>
#include <hip/hip_runtime.h>
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>          // types and prototypes only: the library is bound at run time, when a fit spans several devices
#define CMF_HAVE_RCCL 1
#else
#define CMF_HAVE_RCCL 0         // a ROCm install without the RCCL headers: the shards exchange by peer copies only
#endif

#include "../../include/cmfrec_hip.h"
#include "rng_host.hpp"
#include "exchange_plan.hpp"
#include "newrows.hpp"
#include "fit_inputs.hpp"

using namespace cmfit;

namespace {

// ---- SIGINT between half-steps (helpers.c:1493-1501, collective.c:9520-9531) -----------------
volatile sig_atomic_t g_stop = 0;
void on_sigint(int) { g_stop = 1; }
struct SigGuard {
    void (*old)(int) = nullptr;
    bool armed = false;
    explicit SigGuard(bool arm) : armed(arm)
    {
        // the flag is cleared for every fit, armed or not: the loops test it unconditionally, and a Ctrl-C handled by an
        // earlier fit must not end the next one at iteration 0 (the reference resets should_stop_procedure in its cleanup)
        g_stop = 0;
        if (arm) old = signal(SIGINT, on_sigint);
    }
    ~SigGuard() { if (armed) signal(SIGINT, old); }
};

// CMFREC_HIP_TIMING=1: wall-clock of the host phases of a fit on stderr
struct PhaseTimer {
    bool on = getenv("CMFREC_HIP_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void lap(const char *what)
    {
        if (!on) return;
        auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[cmfrec_hip timing] %-28s %9.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};

int fail(bool verbose, const char *msg)
{
    if (verbose) fprintf(stderr, "%s\n", msg);
    return 2;
}

// ---- validation while fitting (cmfrec_hip_fit_set_monitor, include/cmfrec_hip.h) -------------------------------------
// The monitor waits here, per thread, for the next fit call; take_monitor() at the top of both fit functions empties the slot on
// every path out of them.
struct FitMonitor {
    bool on = false;
    cmfrec_hip_fit_monitor m;
    real_t glob_mean = 0;        // the explicit fit's, set once it is known
    int returned = -1;           // run_loop: the 0-based iteration whose factors the session holds when the loop is over
};
thread_local FitMonitor g_monitor;
std::vector<int> devices_from_env();
bool sharded_fit_wanted(const std::vector<int> &devs);
FitMonitor take_monitor()
{
    FitMonitor out = g_monitor;
    g_monitor = FitMonitor();
    return out;
}
int refuse_monitor(bool verbose, const std::string &msg)
{
    cmfhip::g_last_error = msg;
    if (verbose) fprintf(stderr, "%s\n", msg.c_str());
    return 2;
}
// the refusals that need no session, before the fit writes to any output: 0 or 2
int check_monitor(const FitMonitor &mon, const char *fn, int_t m, int_t n, int_t kk, int_t niter, bool verbose)
{
    if (!mon.on) return 0;
    const std::string name(fn);
    if (niter < 1) return refuse_monitor(verbose, name + ": a monitor needs niter >= 1");
    const bool ranking = mon.m.rankset != nullptr;
    if ((mon.m.evalset != nullptr) == ranking)
        return refuse_monitor(verbose, name + ": the monitor needs an evaluation set or a ranking set, one of the two");
    if (ranking ? (mon.m.metric < CMFREC_HIP_WATCH_HIT || mon.m.metric > CMFREC_HIP_WATCH_MEAN_RANK)
                : (mon.m.metric != CMFREC_HIP_WATCH_RMSE && mon.m.metric != CMFREC_HIP_WATCH_MAE))
        return refuse_monitor(verbose, name + ": the monitor's metric must be CMFREC_HIP_WATCH_RMSE or _MAE with an evaluation set, "
                                              "CMFREC_HIP_WATCH_HIT .. _MEAN_RANK with a ranking set");
    const std::vector<int> devs = devices_from_env();
    if (sharded_fit_wanted(devs))
        return refuse_monitor(verbose, name + ": a monitor needs a fit on one device (CMFREC_HIP_DEVICES names several, or "
                                              "CMFREC_HIP_SHARDED is set)");
    const int device = devs.empty() ? -1 : devs[0];
    const int rc = cmfhip::guarded([&]() {
        return ranking ? cmfhip::rankset_usable(mon.m.rankset, fn, device, m, n, kk, mon.m.k_at) : cmfhip::evalset_usable(mon.m.evalset, fn, device, m, n);
    });
    if (rc && verbose) fprintf(stderr, "%s\n", cmfhip::g_last_error.c_str());
    return rc;
}
double watched_value(const cmfrec_hip_errors &r, int metric)
{
    const double sw = r.sum_w[0] + r.sum_w[1];
    if (sw == 0) return std::nan("");
    if (metric == CMFREC_HIP_WATCH_MAE) return (r.sum_wabs[0] + r.sum_wabs[1]) / sw;
    return std::sqrt((r.sum_wsq[0] + r.sum_wsq[1]) / sw);
}
double watched_value(const cmfrec_hip_rank_record &r, int metric)
{
    const int f = metric - CMFREC_HIP_WATCH_HIT;
    return r.count[f] ? r.sum[f] / (double)r.count[f] : std::nan("");
}
const char *watched_name(int metric)
{
    static const char *names[] = {"RMSE", "MAE", "hit", "precision", "recall", "AP", "NDCG", "RR", "AUC", "mean rank"};
    return names[metric];
}

// chol_A / chol_B: that half-step is a closed-form solve whatever use_cg says (dense X without weights whose rows / columns are
// all or nearly all complete: optimizeA Case 1, common.c:2787-2993)
// mon: the held-out set is evaluated between the iterations, and the loop may end early and go back to its best iterate
int run_loop(cmfrec_hip_session *s, const cmfrec_hip_model &mdl, int niter, bool finalize_chol, bool verbose, bool implicit_feats = false,
             bool chol_A = false, bool chol_B = false, FitMonitor *mon = nullptr)
{
    cmfrec_hip_early_stop es;
    memset(&es, 0, sizeof es);
    int ran = 0;
    bool snapshot_taken = false;
    if (mon) {
        es.every = mon->m.every; es.patience = mon->m.patience; es.min_delta = mon->m.min_delta; es.best_iter = -1;
        es.higher_is_better = (mon->m.rankset != nullptr && mon->m.metric != CMFREC_HIP_WATCH_MEAN_RANK) ? 1 : 0;
        for (int it = 0; it < niter && mon->m.values; it++) mon->m.values[it] = std::nan("");
        if (mon->m.records) memset(mon->m.records, 0, (size_t)niter * sizeof(cmfrec_hip_errors));
        if (mon->m.rank_records) memset(mon->m.rank_records, 0, (size_t)niter * sizeof(cmfrec_hip_rank_record));
    }
    // what the monitor reports however the loop ends; the best iterate comes back when the loop ended on a later one
    auto finish = [&](int rc) {
        if (!mon) return rc;
        if (mon->m.iters_run) *mon->m.iters_run = ran;
        if (mon->m.best_iter) *mon->m.best_iter = es.best_iter;
        mon->returned = ran - 1;
        if (rc == 0 && snapshot_taken && es.best_iter != ran - 1) {
            rc = cmfrec_hip_session_restore(s);
            mon->returned = es.best_iter;
        }
        return rc;
    };
    for (int it = 0; it < niter; it++) {
        if (g_stop) return finish(3);
        int chol = (finalize_chol && mdl.use_cg && it == niter - 1) ? 1 : 0;
        int rc;
        if (mdl.p > 0) { if (verbose) { printf("Updating C..."); fflush(stdout); }
            if ((rc = cmfrec_hip_session_update(s, 'C', chol))) return finish(rc); if (verbose) printf(" done\n"); }
        if (g_stop) return finish(3);
        if (mdl.q > 0) { if (verbose) { printf("Updating D..."); fflush(stdout); }
            if ((rc = cmfrec_hip_session_update(s, 'D', chol))) return finish(rc); if (verbose) printf(" done\n"); }
        if (g_stop) return finish(3);
        if (implicit_feats) {                                             // collective.c:8448-8534
            if (verbose) { printf("Updating Bi..."); fflush(stdout); }
            if ((rc = cmfrec_hip_session_update(s, 'b', 1))) return finish(rc);
            if (verbose) { printf(" done\nUpdating Ai..."); fflush(stdout); }
            if ((rc = cmfrec_hip_session_update(s, 'a', 1))) return finish(rc);
            if (verbose) printf(" done\n");
            if (g_stop) return finish(3);
        }
        if (verbose) { printf("Updating B..."); fflush(stdout); }
        if ((rc = cmfrec_hip_session_update(s, 'B', (chol || chol_B) ? 1 : 0))) return finish(rc);
        if ((rc = cmfrec_hip_session_after_gather(s, 'B'))) return finish(rc);
        if (verbose) { cmfrec_hip_session_sync(s); printf(" done\n"); }
        if (g_stop) return finish(3);
        if (verbose) { printf("Updating A..."); fflush(stdout); }
        if ((rc = cmfrec_hip_session_update(s, 'A', (chol || chol_A) ? 1 : 0))) return finish(rc);
        if ((rc = cmfrec_hip_session_after_gather(s, 'A'))) return finish(rc);
        if (verbose) { cmfrec_hip_session_sync(s); printf(" done\n\tCompleted ALS iteration %2d\n\n", it + 1); fflush(stdout); }
        ran = it + 1;
        if (mon && cmfrec_hip_early_stop_step(&es, it, niter, nullptr)) {
            double value;
            if (mon->m.rankset != nullptr) {
                cmfrec_hip_rank_record rec;
                if ((rc = cmfrec_hip_session_ranking(s, mon->m.rankset, mon->m.k_at, &rec))) return finish(rc);
                value = watched_value(rec, mon->m.metric);
                if (mon->m.rank_records) mon->m.rank_records[it] = rec;
            } else {
                cmfrec_hip_errors rec;
                if ((rc = cmfrec_hip_session_errors(s, mon->m.evalset, mon->glob_mean, &rec))) return finish(rc);
                value = watched_value(rec, mon->m.metric);
                if (mon->m.records) mon->m.records[it] = rec;
            }
            if (mon->m.values) mon->m.values[it] = value;
            const int step = cmfrec_hip_early_stop_step(&es, it, niter, &value);
            if (verbose) {
                printf("\tHeld-out %s after iteration %2d: %.6g%s\n\n", watched_name(mon->m.metric), it + 1, value,
                       (step & CMFREC_HIP_STEP_IMPROVED) ? " (best so far)" : "");
                fflush(stdout);
            }
            if ((step & CMFREC_HIP_STEP_IMPROVED) && mon->m.restore_best) {
                if ((rc = cmfrec_hip_session_snapshot(s))) return finish(rc);
                snapshot_taken = true;
            }
            if (step & CMFREC_HIP_STEP_STOP) {
                if (verbose) { printf("\tStopping early: no improvement in %d evaluations\n\n", es.patience); fflush(stdout); }
                break;
            }
        }
    }
    return finish(0);
}

// ---- several GPUs of one node behind the unchanged C signature ----------------------------------
// CMFREC_HIP_DEVICES="0,1,2,3" (HIP device ordinals, comma separated; an ordinal may repeat, which shards one device --
// that is how the path is tested on a single-GPU box).  One entry: that device instead of the current one.  Several:
// users are cut into equal contiguous blocks and items into nnz-balanced ones, every device owns one block of each, holds
// full replicas of A and B, updates its own rows, and the updated rows travel to the peers over xGMI
// (hipMemcpyPeerAsync, ordered by events; no host synchronisation inside the loop) -- the all-gather of distributed.py
// without torch.  Rows are independent given the opposing matrix and every device computes B^T B from identical
// replicas, so the factors are bit-for-bit those of the single-device fit as long as every row takes the same kernel path on
// the shard as on the whole matrix.  That holds for rows of at most 1024 entries (512 in double precision); for split rows the
// choice between the streaming and the Gramian path, and the slice length, follow the SHARD's statistics (device.hpp,
// prefer_gram / slice_len), so their sums may be taken in another order: equal to rounding, not to the bit
// (tests/test_gpu_multidevice.py has both cases).
std::vector<int> devices_from_env()
{
    std::vector<int> out;
    const char *e = getenv("CMFREC_HIP_DEVICES");
    if (e == nullptr) return out;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return out;
    const char *q = e;
    while (*q) {
        char *end = nullptr;
        const long v = strtol(q, &end, 10);
        if (end == q) break;
        if (v >= 0 && v < count) out.push_back((int)v);
        q = end;
        while (*q == ',' || *q == ' ') q++;
    }
    return out;
}

// RCCL for the exchange between the devices of one fit ("ncclAllGather ... or direct placement").  Bound with
// dlopen when the first multi-device fit asks for it -- a single-device caller never maps the library -- through the prototypes
// of <rccl/rccl.h> (decltype: nothing is declared by hand).
#if !CMF_HAVE_RCCL
// no RCCL headers on this install: enough of the interface for the code below to compile; load() never succeeds, so none of these
// is ever called and every multi-device fit exchanges by peer copies
typedef void *ncclComm_t;
enum ncclResult_t { ncclSuccess = 0, ncclSystemError = 2 };
enum ncclDataType_t { ncclFloat = 7, ncclDouble = 8 };
enum ncclRedOp_t { ncclSum = 0 };
ncclResult_t ncclCommInitAll(ncclComm_t *, int, const int *);
ncclResult_t ncclCommDestroy(ncclComm_t);
ncclResult_t ncclGroupStart();
ncclResult_t ncclGroupEnd();
ncclResult_t ncclSend(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
ncclResult_t ncclRecv(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t);
ncclResult_t ncclAllReduce(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t);
const char *ncclGetErrorString(ncclResult_t);
#endif
struct RcclApi {
    void *handle = nullptr;
    bool failed = false;        // a previous load found the library unusable: do not dlopen it again for every fit
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclSend) Send = nullptr;
    decltype(&ncclRecv) Recv = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    bool load()
    {
        if (handle) return true;
        if (failed || !CMF_HAVE_RCCL) return false;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            handle = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (handle) break;
        }
        if (!handle) { failed = true; return false; }
#define CMF_SYM(field, sym) field = reinterpret_cast<decltype(field)>(dlsym(handle, #sym)); if (!field) { dlclose(handle); handle = nullptr; failed = true; return false; }
        CMF_SYM(CommInitAll, ncclCommInitAll) CMF_SYM(CommDestroy, ncclCommDestroy) CMF_SYM(GroupStart, ncclGroupStart)
        CMF_SYM(GroupEnd, ncclGroupEnd) CMF_SYM(Send, ncclSend) CMF_SYM(Recv, ncclRecv) CMF_SYM(AllReduce, ncclAllReduce)
        CMF_SYM(GetErrorString, ncclGetErrorString)
#undef CMF_SYM
        return true;
    }
};
RcclApi &rccl() { static RcclApi api; return api; }
#ifdef CMFREC_HIP_FLOAT
const ncclDataType_t NCCL_REAL = ncclFloat;
#else
const ncclDataType_t NCCL_REAL = ncclDouble;
#endif

// acc[i] += x[i]: the partial sums of the C / D update when the shards exchange by copies (fixed order: shard 0, 1, 2 ...)
__global__ void add_into_kernel(real_t *__restrict__ acc, const real_t *__restrict__ x, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) acc[i] += x[i];
}

// The shards of one fit and what travels between them.  Two transports:
//   RCCL   (distinct devices; the default there): the updated row blocks go by DIRECT PLACEMENT -- one ncclGroup of
//          ncclSend / ncclRecv per half-step, every device sends its block to each peer and receives the peers' blocks straight
//          into its replica, all pairs at once (on an xGMI node every pair of GPUs has a link of its own: one hop on D - 1 links
//          instead of a ring's D - 1 steps on one); the partial sums of the C / D update by ncclAllReduce.  Every call is
//          enqueued on the owning session's stream: kernels -> exchange -> next kernels are ordered by the stream, the host
//          thread never waits inside the loop.
//   copies (an ordinal repeats, i.e. several shards on one device -- how the path runs on a single-GPU box -- or
//          CMFREC_HIP_EXCHANGE=copy): hipMemcpyPeerAsync ordered by events; the C / D partial sums are added on the first
//          shard's device in shard order and copied back.
struct MultiDev {
    std::vector<cmfrec_hip_session *> sess;
    std::vector<int> dev;
    std::vector<int> rb, cb;               // block boundaries of users / items (D + 1 each)
    std::vector<hipEvent_t> ev;            // per device: "my block has reached every peer"
    std::vector<ncclComm_t> comm;          // RCCL transport: one communicator per shard (empty: copies)
    real_t *stage = nullptr, *stage2 = nullptr;   // copies transport: partial sums on the first shard's device
    size_t stage_n = 0;
    std::string error;
    ~MultiDev()
    {
        for (auto e : ev) if (e) (void)hipEventDestroy(e);
        if (!comm.empty()) for (auto c : comm) if (c) (void)rccl().CommDestroy(c);
        if (stage) { (void)hipSetDevice(dev.empty() ? 0 : dev[0]); (void)hipFree(stage); (void)hipFree(stage2); }
        for (auto s : sess) if (s) cmfrec_hip_session_destroy(s);
    }
    bool use_rccl() const { return !comm.empty(); }
    // CMFREC_HIP_EXCHANGE = rccl | copy (default: rccl where the ordinals are distinct and librccl can be bound)
    int init_transport(bool verbose)
    {
        const char *e = getenv("CMFREC_HIP_EXCHANGE");
        const bool want_copy = e != nullptr && strcmp(e, "copy") == 0, want_rccl = e != nullptr && strcmp(e, "rccl") == 0;
        const bool distinct = std::set<int>(dev.begin(), dev.end()).size() == dev.size();
        if (want_copy || !distinct) {
            if (want_rccl) { error = "cmfrec_hip: CMFREC_HIP_EXCHANGE=rccl needs distinct device ordinals in CMFREC_HIP_DEVICES"; return 2; }
            return 0;
        }
        if (!rccl().load()) {
            if (want_rccl) { error = "cmfrec_hip: librccl could not be loaded"; return 4; }
            if (verbose) printf("cmfrec_hip: librccl not found, the shards exchange by peer copies\n");
            return 0;
        }
        comm.assign(dev.size(), nullptr);
        const ncclResult_t r = rccl().CommInitAll(comm.data(), (int)dev.size(), dev.data());
        if (r != ncclSuccess) {
            comm.clear();
            error = std::string("cmfrec_hip: ncclCommInitAll failed: ") + rccl().GetErrorString(r);
            if (want_rccl) return 4;
            if (verbose) printf("%s; the shards exchange by peer copies\n", error.c_str());
            error.clear();
        }
        return 0;
    }
    // block d of matrix `which` (updated on device d) reaches every other replica; every stream then holds all blocks
    int exchange(int which)
    {
        const int D = (int)sess.size();
        const std::vector<int> &bb = (which == 'A') ? rb : cb;
        if (use_rccl()) {
            if (D == 1) return 0;
            std::vector<real_t *> base(D); std::vector<size_t> ld(D); std::vector<hipStream_t> st(D);
            for (int d = 0; d < D; d++) {
                size_t rows = 0;
                base[d] = (real_t *)cmfrec_hip_session_device_ptr(sess[d], which, &rows, &ld[d]);
                st[d] = (hipStream_t)cmfrec_hip_session_stream(sess[d]);
            }
            ncclResult_t r = rccl().GroupStart();
            // the schedule is a pure function of the block boundaries (exchange_plan.hpp; tests/test_exchange_plan.py)
            for (const cmfhip::ExchangeOp &op : cmfhip::direct_placement_plan(bb)) {
                if (r != ncclSuccess) break;
                const int d = op.dev;
                real_t *ptr = base[d] + (size_t)op.first_row * ld[d];
                const size_t cnt = (size_t)op.rows * ld[d];
                r = op.send ? rccl().Send(ptr, cnt, NCCL_REAL, op.peer, comm[d], st[d]) : rccl().Recv(ptr, cnt, NCCL_REAL, op.peer, comm[d], st[d]);
            }
            const ncclResult_t r2 = rccl().GroupEnd();
            if (r != ncclSuccess || r2 != ncclSuccess) {
                error = std::string("cmfrec_hip: RCCL exchange failed: ") + rccl().GetErrorString(r != ncclSuccess ? r : r2);
                return 4;
            }
            return 0;
        }
        for (int d = 0; d < D; d++) {
            size_t rows = 0, ld = 0;
            real_t *src = (real_t *)cmfrec_hip_session_device_ptr(sess[d], which, &rows, &ld);
            hipStream_t st = (hipStream_t)cmfrec_hip_session_stream(sess[d]);
            if (hipSetDevice(dev[d]) != hipSuccess) return 4;
            const size_t off = (size_t)bb[d] * ld, bytes = (size_t)(bb[d + 1] - bb[d]) * ld * sizeof(real_t);
            for (int e = 0; e < D && bytes; e++) {
                if (e == d) continue;
                size_t r2 = 0, l2 = 0;
                real_t *dst = (real_t *)cmfrec_hip_session_device_ptr(sess[e], which, &r2, &l2);
                if (hipMemcpyPeerAsync(dst + off, dev[e], src + off, dev[d], bytes, st) != hipSuccess) return 4;
            }
            if (hipEventRecord(ev[d], st) != hipSuccess) return 4;
        }
        for (int e = 0; e < D; e++) {
            hipStream_t st = (hipStream_t)cmfrec_hip_session_stream(sess[e]);
            if (hipSetDevice(dev[e]) != hipSuccess) return 4;
            for (int d = 0; d < D; d++)
                if (d != e && hipStreamWaitEvent(st, ev[d], 0) != hipSuccess) return 4;
        }
        return 0;
    }
    // the shards' partial sums [F_loc^T F_loc | U_loc^T F_loc] of a C / D update (cmfrec_hip_session_sideinfo_partial) become
    // their total on every shard -- the same numbers everywhere, so that every replica solves the same small system
    int allreduce_partials(size_t count)
    {
        const int D = (int)sess.size();
        if (use_rccl()) {
            ncclResult_t r = rccl().GroupStart();
            for (int d = 0; d < D && r == ncclSuccess; d++) {
                size_t rows = 0, ld = 0;
                real_t *part = (real_t *)cmfrec_hip_session_device_ptr(sess[d], 'P', &rows, &ld);
                r = rccl().AllReduce(part, part, count, NCCL_REAL, ncclSum, comm[d], (hipStream_t)cmfrec_hip_session_stream(sess[d]));
            }
            const ncclResult_t r2 = rccl().GroupEnd();
            if (r != ncclSuccess || r2 != ncclSuccess) {
                error = std::string("cmfrec_hip: RCCL all-reduce failed: ") + rccl().GetErrorString(r != ncclSuccess ? r : r2);
                return 4;
            }
            return 0;
        }
        if (D == 1) return 0;
        // copies: everything through the first shard's stream, between two host synchronisations (the test transport)
        for (int d = 0; d < D; d++) { const int rc = cmfrec_hip_session_sync(sess[d]); if (rc) return rc; }
        if (hipSetDevice(dev[0]) != hipSuccess) return 4;
        if (stage_n < count) {
            if (stage) { (void)hipFree(stage); (void)hipFree(stage2); stage = stage2 = nullptr; }
            if (hipMalloc((void **)&stage, count * sizeof(real_t)) != hipSuccess || hipMalloc((void **)&stage2, count * sizeof(real_t)) != hipSuccess) return 1;
            stage_n = count;
        }
        hipStream_t st0 = (hipStream_t)cmfrec_hip_session_stream(sess[0]);
        for (int d = 0; d < D; d++) {
            size_t rows = 0, ld = 0;
            const real_t *part = (const real_t *)cmfrec_hip_session_device_ptr(sess[d], 'P', &rows, &ld);
            if (hipMemcpyPeerAsync(d == 0 ? stage : stage2, dev[0], part, dev[d], count * sizeof(real_t), st0) != hipSuccess) return 4;
            if (d > 0) hipLaunchKernelGGL(add_into_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st0, stage, stage2, count);
        }
        for (int d = 0; d < D; d++) {
            size_t rows = 0, ld = 0;
            real_t *part = (real_t *)cmfrec_hip_session_device_ptr(sess[d], 'P', &rows, &ld);
            if (hipMemcpyPeerAsync(part, dev[d], stage, dev[0], count * sizeof(real_t), st0) != hipSuccess) return 4;
        }
        if (hipStreamSynchronize(st0) != hipSuccess) return 4;
        return 0;
    }
};

// One session per entry of `devs`, each owning a block of users and a block of items and holding the block's entries of X
// ((x - subtract) * alpha): users in equal contiguous blocks, items in nnz-balanced contiguous ones.
// `configure` is called on every new session once its shards are built.
int build_shards(MultiDev &md, const std::vector<int> &devs, const cmfrec_hip_model &mdl, int_t m, int_t n, const int_t *ixA,
                 const int_t *ixB, const real_t *X, size_t nnz, real_t subtract, real_t alpha,
                 const std::function<int(cmfrec_hip_session *, int)> &configure)
{
    const int D = (int)devs.size();
    md.dev = devs;
    {
        const int rc = md.init_transport(false);
        if (rc) { fprintf(stderr, "%s\n", md.error.c_str()); return rc; }
    }
    md.rb.assign(D + 1, 0); md.cb.assign(D + 1, 0);
    const int step = (m + D - 1) / D;
    for (int d = 0; d <= D; d++) md.rb[d] = std::min(d * step, (int)m);
    {
        std::vector<size_t> cnt((size_t)n + 1, 0);
        for (size_t e = 0; e < nnz; e++) cnt[(size_t)ixB[e] + 1]++;
        for (int j = 0; j < n; j++) cnt[j + 1] += cnt[j];
        int j = 0;
        for (int d = 1; d < D; d++) {
            const double target = (double)nnz * d / D;
            while (j < n && (double)cnt[j] < target) j++;
            md.cb[d] = std::max(md.cb[d - 1], j);
        }
        md.cb[D] = n;
    }
    for (int d = 0; d < D; d++)
        for (int e = 0; e < D; e++)
            if (devs[d] != devs[e] && hipSetDevice(devs[d]) == hipSuccess) {
                int can = 0;
                if (hipDeviceCanAccessPeer(&can, devs[d], devs[e]) == hipSuccess && can) {
                    const hipError_t pe = hipDeviceEnablePeerAccess(devs[e], 0);
                    if (pe != hipSuccess) (void)hipGetLastError();            // already enabled
                }
            }
    md.sess.assign(D, nullptr); md.ev.assign(D, nullptr);
    std::vector<int_t> key, oth; std::vector<real_t> val;
    for (int d = 0; d < D; d++) {
        cmfrec_hip_model md_d = mdl;
        md_d.row_begin = md.rb[d]; md_d.row_end = md.rb[d + 1]; md_d.col_begin = md.cb[d]; md_d.col_end = md.cb[d + 1];
        md.sess[d] = cmfrec_hip_session_create(&md_d, devs[d]);
        if (!md.sess[d]) { const int ec = cmfrec_hip_last_error_code(); return ec ? ec : 1; }
        if (hipEventCreateWithFlags(&md.ev[d], hipEventDisableTiming) != hipSuccess) return 4;
        // the block's entries in COO order (the order the stable device sort keeps inside a row), staged through device buffers
        for (int side = 0; side < 2; side++) {
            const int lo = side == 0 ? md.rb[d] : md.cb[d], hi = side == 0 ? md.rb[d + 1] : md.cb[d + 1];
            const int_t *kk = side == 0 ? ixA : ixB, *oo = side == 0 ? ixB : ixA;
            key.clear(); oth.clear(); val.clear();
            for (size_t e = 0; e < nnz; e++)
                if (kk[e] >= lo && kk[e] < hi) { key.push_back(kk[e] - lo); oth.push_back(oo[e]); val.push_back(X[e]); }
            int_t *dk = nullptr, *d_o = nullptr; real_t *dv = nullptr;
            const size_t cntE = key.size();
            if (hipSetDevice(devs[d]) != hipSuccess) return 4;
            if (hipMalloc((void **)&dk, std::max<size_t>(cntE, 1) * sizeof(int_t)) != hipSuccess) return 1;
            if (hipMalloc((void **)&d_o, std::max<size_t>(cntE, 1) * sizeof(int_t)) != hipSuccess) { (void)hipFree(dk); return 1; }
            if (hipMalloc((void **)&dv, std::max<size_t>(cntE, 1) * sizeof(real_t)) != hipSuccess) { (void)hipFree(dk); (void)hipFree(d_o); return 1; }
            (void)hipMemcpy(dk, key.data(), cntE * sizeof(int_t), hipMemcpyHostToDevice);
            (void)hipMemcpy(d_o, oth.data(), cntE * sizeof(int_t), hipMemcpyHostToDevice);
            (void)hipMemcpy(dv, val.data(), cntE * sizeof(real_t), hipMemcpyHostToDevice);
            const int rc = cmfrec_hip_session_set_X_coo_device(md.sess[d], side == 0 ? 'r' : 'c', dk, d_o, dv, cntE, subtract, alpha);
            (void)hipFree(dk); (void)hipFree(d_o); (void)hipFree(dv);
            if (rc) return rc;
        }
        const int rc = configure(md.sess[d], d);
        if (rc) return rc;
    }
    return 0;
}

// C ('C') or D ('D') update of the collective model over the shards (optimizeA Case 1, common.c:2793-2991, with U / I cut into the
// same row blocks as A / B): every shard adds up  F_loc^T F_loc  and  U_loc^T F_loc  over ITS rows, the sums are made global
// (ncclAllReduce, or added in shard order by the copies transport), and every shard solves the same small system -- C / D stay
// identical replicas without ever being exchanged.
int multi_sideinfo_step(MultiDev &md, const cmfrec_hip_model &mdl, int which)
{
    const int D = (int)md.sess.size();
    const size_t pp = (size_t)(which == 'C' ? mdl.p : mdl.q), kc = (size_t)((which == 'C' ? mdl.k_user : mdl.k_item) + mdl.k);
    for (int d = 0; d < D; d++) { const int rc = cmfrec_hip_session_sideinfo_partial(md.sess[d], which); if (rc) return rc; }
    const int rc = md.allreduce_partials(kc * kc + pp * kc);
    if (rc) return rc;
    for (int d = 0; d < D; d++) { const int rc2 = cmfrec_hip_session_sideinfo_finish(md.sess[d], which); if (rc2) return rc2; }
    return 0;
}

// The ALS loop over the shards, both models: C, D (dense side information), then B, then A (collective.c:8334-8898, :9855-10022) --
// every device updates its block, the updated rows (a bias column rides in them, collective.c:8538-8543) reach the peers
// (MultiDev::exchange), and every replica splits the opposing bias off again (cmfrec_hip_session_after_gather).
int multi_loop(MultiDev &md, const cmfrec_hip_model &mdl, int niter, bool finalize_chol, bool verbose)
{
    const int D = (int)md.sess.size();
    if (verbose) {
        printf("Starting ALS optimization routine (%d device shards, exchange by %s)\n\n", D, md.use_rccl() ? "RCCL" : "peer copies");
        fflush(stdout);
    }
    for (int it = 0; it < niter; it++) {
        if (g_stop) return 3;
        const int chol = (finalize_chol && mdl.use_cg && it == niter - 1) ? 1 : 0;
        if (mdl.p > 0) { const int rc = multi_sideinfo_step(md, mdl, 'C'); if (rc) return rc; }
        if (mdl.q > 0) { const int rc = multi_sideinfo_step(md, mdl, 'D'); if (rc) return rc; }
        for (int pass = 0; pass < 2; pass++) {
            const int which = pass == 0 ? 'B' : 'A';
            for (int d = 0; d < D; d++) { const int rc = cmfrec_hip_session_update(md.sess[d], which, chol); if (rc) return rc; }
            int rc = md.exchange(which);
            if (rc == 4 && !md.error.empty()) fprintf(stderr, "%s\n", md.error.c_str());
            for (int d = 0; d < D && !rc; d++) rc = cmfrec_hip_session_after_gather(md.sess[d], which);
            if (rc) return rc;
            if (g_stop) return 3;
        }
        if (verbose) { for (int d = 0; d < D; d++) cmfrec_hip_session_sync(md.sess[d]); printf("\tCompleted ALS iteration %2d\n\n", it + 1); fflush(stdout); }
    }
    for (int d = 0; d < D; d++) { const int rc = cmfrec_hip_session_sync(md.sess[d]); if (rc) return rc; }
    return 0;
}

// the rows of the (centred) dense side information that belong to shard d: U rows [rb[d], min(rb[d+1], m_u)), I likewise
int set_sideinfo_shard(const MultiDev &md, cmfrec_hip_session *sd, int d, const real_t *Uc, int_t m_u, int_t p, const real_t *Ic, int_t n_i, int_t q)
{
    const real_t *Ul = (Uc && p > 0 && md.rb[d] < m_u) ? Uc + (size_t)md.rb[d] * p : nullptr;
    const real_t *Il = (Ic && q > 0 && md.cb[d] < n_i) ? Ic + (size_t)md.cb[d] * q : nullptr;
    if ((Uc && p > 0) || (Ic && q > 0)) return cmfrec_hip_session_set_sideinfo_local(sd, Ul, Il);
    return 0;
}

// several entries in CMFREC_HIP_DEVICES, or one entry together with CMFREC_HIP_SHARDED=1 (the sharded driver on a single
// shard: what a one-GPU box can run of the RCCL transport -- communicator, all-reduce -- tests/test_gpu_multidevice.py)
bool sharded_fit_wanted(const std::vector<int> &devs)
{
    if (devs.size() > 1) return true;
    const char *e = getenv("CMFREC_HIP_SHARDED");
    return devs.size() == 1 && e != nullptr && e[0] == '1';
}

int fail(bool verbose, const std::string &msg) { return fail(verbose, msg.c_str()); }

// the session of a fit, or why there is none (on stderr when verbose) and the code the fit returns
cmfrec_hip_session *create_session(const cmfrec_hip_model &mdl, int device, bool verbose, int &rc)
{
    cmfrec_hip_session *s = cmfrec_hip_session_create(&mdl, device);
    if (s) return s;
    if (verbose) fprintf(stderr, "%s\n", cmfrec_hip_last_error());
    const int ec = cmfrec_hip_last_error_code();
    rc = ec ? ec : 1;
    return nullptr;
}

// side information in whichever form the intake left it: the zero rows, the centred dense matrices, the triplets taken as zeros
// (beyond the zero-fill limit), the sparse triplets (as given, or the centred present entries of a dense matrix with NaN)
int hand_sides_to_session(cmfrec_hip_session *s, const SideInput &su, const SideInput &si)
{
    int rc = 0;
    if (!su.zero_rows.empty()) rc = cmfrec_hip_session_set_zero_rows(s, 'A', su.zero_rows.data(), (int)su.zero_rows.size());
    if (!rc && !si.zero_rows.empty()) rc = cmfrec_hip_session_set_zero_rows(s, 'B', si.zero_rows.data(), (int)si.zero_rows.size());
    if (!rc) rc = cmfrec_hip_session_set_sideinfo(s, su.centred_or_null(), si.centred_or_null());
    if (!rc && su.sz.on) rc = cmfrec_hip_session_set_sideinfo_sparse_zeros(s, 'U', su.sz.row, su.sz.col, su.sz.val, su.sz.nnz, su.sz.colmeans());
    if (!rc && si.sz.on) rc = cmfrec_hip_session_set_sideinfo_sparse_zeros(s, 'I', si.sz.row, si.sz.col, si.sz.val, si.sz.nnz, si.sz.colmeans());
    if (!rc && su.sparse()) rc = cmfrec_hip_session_set_sideinfo_sparse(s, 'U', su.row, su.col, su.val, su.nnz);
    if (!rc && si.sparse()) rc = cmfrec_hip_session_set_sideinfo_sparse(s, 'I', si.row, si.col, si.val, si.nnz);
    return rc;
}

// dense side information with NaN: the per-attribute rules of the dense C / D update (DenseNanSide::rules); kc: the width of C / D
int hand_nan_rules(cmfrec_hip_session *s, const SideInput &side, int which, int_t kc, bool scale_lam, bool use_cg)
{
    if (side.nan.na_col.empty() || !side.sparse()) return 0;
    std::vector<unsigned char> mask; std::vector<real_t> mult;
    side.nan.rules(kc, scale_lam, mask, mult);
    int rc = 0;
    if (use_cg) rc = cmfrec_hip_session_set_closed_form_rows(s, which, mask.data());
    if (!rc && !mult.empty()) rc = cmfrec_hip_session_set_lambda_multipliers(s, which, mult.data());
    return rc;
}

}  // namespace

extern "C" {

/* the exchange schedule of MultiDev::exchange as data (include/cmfrec_hip.h); host-only */
int cmfrec_hip_exchange_plan(int D, const int *bb, int *out, int cap)
{
    if (D < 1 || bb == nullptr) return -1;
    const std::vector<cmfhip::ExchangeOp> ops = cmfhip::direct_placement_plan(std::vector<int>(bb, bb + D + 1));
    for (size_t i = 0; i < ops.size() && (int)i < cap && out != nullptr; i++) {
        out[5 * i] = ops[i].dev; out[5 * i + 1] = ops[i].peer; out[5 * i + 2] = ops[i].send;
        out[5 * i + 3] = ops[i].first_row; out[5 * i + 4] = ops[i].rows;
    }
    return (int)ops.size();
}

/* validation while fitting (include/cmfrec_hip.h): the monitor of this thread's next fit call */
int cmfrec_hip_fit_set_monitor(const cmfrec_hip_fit_monitor *monitor)
{
    g_monitor = FitMonitor();
    if (monitor != nullptr) { g_monitor.on = true; g_monitor.m = *monitor; }
    return 0;
}

/* the rule of the monitor, host only: which iterations are evaluated, what improves, when to stop */
int cmfrec_hip_early_stop_step(cmfrec_hip_early_stop *st, int iter, int niter, const double *value)
{
    if (st == nullptr) return 0;
    if (value == nullptr) {
        const int every = st->every < 1 ? 1 : st->every;
        return ((iter + 1) % every == 0 || iter == niter - 1) ? CMFREC_HIP_STEP_EVALUATE : 0;
    }
    const double v = *value;
    bool improved = false;
    if (!std::isnan(v))
        improved = st->best_iter < 0 || (st->higher_is_better ? v > st->best + st->min_delta : v < st->best - st->min_delta);
    if (improved) {
        st->best = v; st->best_iter = iter; st->misses = 0;
        return CMFREC_HIP_STEP_IMPROVED;
    }
    st->misses++;
    return (st->patience > 0 && st->misses >= st->patience) ? CMFREC_HIP_STEP_STOP : 0;
}

/* Start values exactly as the reference's random_parallel (helpers.c:927-1043) draws them. */
int cmfrec_hip_random_parallel(real_t *A, size_t sizeA, real_t *B, size_t sizeB, int_t seed, bool normal)
{
    cmfrng::random_parallel<real_t>(A, sizeA, B, sizeB, seed, normal);
    return CMF_ZIGGURAT_TABLES_EXACT;
}

int_t fit_collective_implicit_als(
    real_t *A, real_t *B, real_t *C, real_t *D, bool reset_values, int_t seed,
    real_t *U_colmeans, real_t *I_colmeans, int_t m, int_t n, int_t k,
    int_t ixA[], int_t ixB[], real_t *X, size_t nnz,
    real_t lam, real_t *lam_unique, real_t l1_lam, real_t *l1_lam_unique,
    real_t *U, int_t m_u, int_t p, real_t *II, int_t n_i, int_t q,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    int_t I_row[], int_t I_col[], real_t *I_sp, size_t nnz_I,
    bool NA_as_zero_U, bool NA_as_zero_I, int_t k_main, int_t k_user, int_t k_item,
    real_t w_main, real_t w_user, real_t w_item, real_t *w_main_multiplier,
    real_t alpha, bool adjust_weight, bool apply_log_transf, int_t niter, int nthreads,
    bool verbose, bool handle_interrupt, bool use_cg, int_t max_cg_steps, bool precondition_cg,
    bool finalize_chol, bool nonneg, int_t max_cd_steps, bool nonneg_C, bool nonneg_D,
    bool precompute_for_predictions, real_t *precomputedBtB, real_t *precomputedBeTBe,
    real_t *precomputedBeTBeChol, real_t *precomputedCtUbias)
{

    (void)nthreads;
    FitMonitor mon = take_monitor();
    if (const int rc_mon = check_monitor(mon, "fit_collective_implicit_als", m, n, k + k_main, niter, verbose)) return rc_mon;
    // collective.c:9406-9435
    if (k_user && U == nullptr && nnz_U == 0) return fail(verbose, "Cannot pass 'k_user' without U data.");
    if (k_item && II == nullptr && nnz_I == 0) return fail(verbose, "Cannot pass 'k_item' without I data.");
    if (k_main && nnz == 0) return fail(verbose, "Cannot pass 'k_main' without X data.");
    if (nnz == 0) return fail(verbose, "cmfrec_hip: the implicit model needs at least one entry of X.");
    // side information, stage 1 (NA_as_zero_U / _I) and stage 2 (NaN in a dense matrix), U before I: SideInput, fit_inputs.hpp
    SideInput su = user_side(U, m_u, p, U_row, U_col, U_sp, nnz_U, U_colmeans), si = item_side(II, n_i, q, I_row, I_col, I_sp, nnz_I, I_colmeans);
    const bool sparse_zeros_ok = !sharded_fit_wanted(devices_from_env());
    std::string refusal = su.zero_fill(NA_as_zero_U, m, ixA, nnz, sparse_zeros_ok);
    if (refusal.empty()) refusal = si.zero_fill(NA_as_zero_I, n, ixB, nnz, sparse_zeros_ok);
    if (!refusal.empty()) return fail(verbose, refusal);
    su.take_nan(); si.take_nan();
    const bool nan_side = su.nan_side || si.nan_side;
    // (asymmetry, kept: only U is refused for having nothing left; an I without a present entry counts as no I)
    if (su.nothing_present(nan_side)) return fail(verbose, "cmfrec_hip: U has no present entries.");
    // side information: dense or sparse COO (missing = absent).  Sparse: rows within X.
    if (su.bad_triplets(m) || si.bad_triplets(n))
        return fail(verbose, "cmfrec_hip: sparse side information must be COO triplets with rows inside X.");
    su.drop_if_absent(); si.drop_if_absent();
    if (su.index_out_of_range()) return fail(verbose, su.index_message());
    if (si.index_out_of_range()) return fail(verbose, si.index_message());
    if ((l1_lam != 0 || l1_lam_unique) && (su.beyond(m) || si.beyond(n)))
        return fail(verbose, "cmfrec_hip: L1 together with side information beyond X is not implemented.");
    if (nonneg || nonneg_C || nonneg_D || l1_lam != 0 || l1_lam_unique) use_cg = false;    // collective.c:9568-9571 (any of them, unlike the explicit model)
    // For rows with few missing values the reference corrects a precomputed Gramian instead of summing the present entries
    // (factors_closed_form, common.c:762-790): the same solution with the Cholesky solver; under CG such attributes are solved in
    // closed form or restart from zero with k steps (:2958-2985) -- DenseNanSide::rules, handed to the session below.  The
    // non-negative / L1 solvers see another matrix layout -- not restated, so not offered.
    if (nan_side && (nonneg || nonneg_C || nonneg_D || l1_lam != 0 || l1_lam_unique))
        return fail(verbose, "cmfrec_hip: NaN in dense side information: not together with nonneg / L1.");
    if (precompute_for_predictions && precomputedBtB == nullptr)
        return fail(verbose, "cmfrec_hip: precompute_for_predictions needs the output buffers (cmfrec.h.in:760-778).");
    if (m <= 0 || n <= 0 || k + k_main <= 0) return fail(verbose, "cmfrec_hip: invalid dimensions.");
    for (size_t e = 0; e < nnz; e++)
        if (ixA[e] < 0 || ixA[e] >= m || ixB[e] < 0 || ixB[e] >= n) return fail(verbose, "cmfrec_hip: X index out of range.");
    real_t w_mult = 1;
    if (adjust_weight) {                                                  // collective.c:9776-9783
        w_mult = (real_t)((long double)nnz / (long double)((size_t)m * (size_t)n));
        w_main *= w_mult;
    }
    if (w_main_multiplier) *w_main_multiplier = w_mult;
    // per-matrix penalties: entries 2..5 = A, B, C, D (the bias slots are unused by this model, collective.c:9793-9809)
    real_t lam6[6], l16[6];
    for (int e = 0; e < 6; e++) { lam6[e] = lam_unique ? lam_unique[e] : lam; l16[e] = l1_lam_unique ? l1_lam_unique[e] : l1_lam; }
    if (w_main != (real_t)1) {                                            // collective.c:9786-9811
        lam /= w_main; l1_lam /= w_main; w_user /= w_main; w_item /= w_main;
        for (int e = 2; e < 6; e++) { lam6[e] /= w_main; l16[e] /= w_main; }
    }

    PhaseTimer tm;
    tm.lap("validate");
    SigGuard sig(handle_interrupt);
    std::vector<real_t> Xs;                                              // X is copied before edits (:9578-9599)
    if (apply_log_transf) {
        Xs.assign(X, X + nnz);
        for (auto &x : Xs) x = std::log(x);
    }
    tm.lap("log transform");

    su.center(); si.center();

    const int k_totA = k_user + k + k_main, k_totB = k_item + k + k_main;
    const int_t m_max = std::max(m, su.rows), n_max = std::max(n, si.rows);     // rows of A / B (collective.c:9437-9440)
    if (reset_values) {                                                  // :9750-9774
        const bool fill_B = si.present();
        cmfrng::random_parallel<real_t>(A, (size_t)m_max * k_totA, fill_B ? B : nullptr, fill_B ? (size_t)n_max * k_totB : 0, seed, false);
        if (use_cg) {
            if (!fill_B) memset(B, 0, (size_t)n_max * k_totB * sizeof(real_t));
            if (su.present()) memset(C, 0, (size_t)su.cols * (k_user + k) * sizeof(real_t));
            if (si.present()) memset(D, 0, (size_t)si.cols * (k_item + k) * sizeof(real_t));
        }
        // Cholesky: start values that are never read (the C / D / B steps run first) are left as passed, like the reference
    }
    if (!use_cg) finalize_chol = false;                                  // :9518
    tm.lap("start values");

    cmfrec_hip_model mdl;
    memset(&mdl, 0, sizeof mdl);
    mdl.implicit = 1; mdl.m = m_max; mdl.n = n_max; mdl.m_x = m; mdl.n_x = n;
    mdl.k = k; mdl.k_main = k_main; mdl.k_user = k_user; mdl.k_item = k_item;
    mdl.use_cg = use_cg; mdl.max_cg_steps = max_cg_steps; mdl.precondition_cg = precondition_cg; mdl.lam = lam;
    mdl.p = su.cols; mdl.q = si.cols; mdl.m_u = su.rows; mdl.n_i = si.rows; mdl.w_user = w_user; mdl.w_item = w_item;
    mdl.row_begin = 0; mdl.row_end = m_max; mdl.col_begin = 0; mdl.col_end = n_max;
    // the matrices for predictions, single device and shards alike (collective.c:10056-10115; also after an interrupt, :10034-10043)
    // (a monitored fit that returns an earlier iterate than niter - 1 returns one whose last A-step was not the Cholesky pass; a
    //  sharded fit has no monitor, check_monitor)
    auto epilogue = [&](cmfrec_hip_session *s) {
        const int last_chol = (!use_cg || (finalize_chol && niter > 0 && (!mon.on || mon.returned == niter - 1))) ? 1 : 0;
        const int rc2 = cmfrec_hip_session_precompute(s, last_chol, 0, precomputedBtB, nullptr, su.had_dense ? precomputedBeTBe : nullptr,
                                                      su.had_dense ? precomputedBeTBeChol : nullptr, nullptr, nullptr);
        if (su.naz && !rc2) fill_CtUbias(precomputedCtUbias, C, su.colmeans, su.cols, k_user + k, w_user);   // collective.c:9244-9252, :10115-10123
        return rc2;
    };
    // device selection without touching the signature: CMFREC_HIP_DEVICES (one ordinal: that device; several: row-block shards)
    const std::vector<int> devs = devices_from_env();
    // Sharded: the plain model and the one with DENSE side information (C / D by partial sums + all-reduce, multi_sideinfo_step),
    // all solvers, constraints and penalties; sparse side information and side information beyond the shape of X keep to the
    // first listed device.
    const bool multi_ok = sharded_fit_wanted(devs) && !su.sparse() && !si.sparse() && !su.sz.on && !si.sz.on && su.rows <= m && si.rows <= n &&
                          m >= (int_t)devs.size() && n >= (int_t)devs.size() && su.zero_rows.empty() && si.zero_rows.empty();
    if (devs.size() > 1 && !multi_ok && verbose)
        printf("cmfrec_hip: CMFREC_HIP_DEVICES lists %d devices; this configuration (sparse side information / side information beyond X) "
               "runs on the first\n", (int)devs.size());
    if (multi_ok) {
        MultiDev md;
        int rc_loop = build_shards(md, devs, mdl, m_max, n_max, ixA, ixB, apply_log_transf ? Xs.data() : X, nnz, (real_t)0, alpha,
                                   [&](cmfrec_hip_session *sd, int d) {
            int rc2 = set_sideinfo_shard(md, sd, d, su.centred_or_null(), su.rows, su.cols, si.centred_or_null(), si.rows, si.cols);
            if (!rc2 && (nonneg || nonneg_C || nonneg_D)) rc2 = cmfrec_hip_session_set_nonneg(sd, nonneg, nonneg_C, nonneg_D, (int)max_cd_steps);
            if (!rc2 && l1_lam != 0) rc2 = cmfrec_hip_session_set_l1(sd, l1_lam, (int)max_cd_steps);
            // (the shards always pass lam6, the single device below only when lam_unique / l1_lam_unique was given: left apart)
            if (!rc2) rc2 = cmfrec_hip_session_set_lam_unique(sd, lam6, l1_lam_unique ? l16 : nullptr, (int)max_cd_steps);
            if (!rc2) rc2 = cmfrec_hip_session_set_factors(sd, A, B, nullptr, nullptr, C, D);
            return rc2;
        });
        if (!rc_loop) rc_loop = multi_loop(md, mdl, (int)niter, finalize_chol, verbose);
        cmfrec_hip_session *s0 = md.sess.empty() ? nullptr : md.sess[0];
        if ((rc_loop == 0 || rc_loop == 3) && s0) {
            int rc2 = cmfrec_hip_session_get_factors(s0, A, B, nullptr, nullptr, C, D);
            if (rc2) rc_loop = rc2;
        }
        if ((rc_loop == 0 || rc_loop == 3) && s0 && precompute_for_predictions)
            if (const int rc2 = epilogue(s0)) rc_loop = rc2;
        if (verbose && rc_loop == 0) printf("ALS procedure terminated successfully\n");
        return rc_loop;
    }
    int rc = 0;
    cmfrec_hip_session *s = create_session(mdl, devs.empty() ? -1 : devs[0], verbose, rc);
    if (!s) return rc;
    tm.lap("session create");
    // X := alpha * X and COO -> CSR + CSC happen on the device (coo_device.hpp), same entry order as helpers.c:1375-1491
    rc = cmfrec_hip_session_set_X_coo(s, ixA, ixB, apply_log_transf ? Xs.data() : X, nnz, (real_t)0, alpha);
    std::vector<real_t>().swap(Xs);
    tm.lap("set_X_coo (upload, sort, bins)");
    if (!rc) rc = hand_sides_to_session(s, su, si);
    if (!rc) rc = hand_nan_rules(s, su, 'C', k_user + k, false, use_cg);
    if (!rc) rc = hand_nan_rules(s, si, 'D', k_item + k, false, use_cg);
    if (!rc && (nonneg || nonneg_C || nonneg_D)) rc = cmfrec_hip_session_set_nonneg(s, nonneg, nonneg_C, nonneg_D, (int)max_cd_steps);
    if (!rc && l1_lam != 0) rc = cmfrec_hip_session_set_l1(s, l1_lam, (int)max_cd_steps);
    if (!rc && (lam_unique || l1_lam_unique))
        rc = cmfrec_hip_session_set_lam_unique(s, lam_unique ? lam6 : nullptr, l1_lam_unique ? l16 : nullptr, (int)max_cd_steps);
    if (!rc) rc = cmfrec_hip_session_set_factors(s, A, B, nullptr, nullptr, C, D);
    if (verbose && !rc) { printf("Starting ALS optimization routine\n\n"); fflush(stdout); }
    if (tm.on) cmfrec_hip_session_sync(s);
    tm.lap("set_factors");
    int rc_loop = rc ? rc : run_loop(s, mdl, niter, finalize_chol, verbose, false, false, false, mon.on ? &mon : nullptr);
    if (tm.on) cmfrec_hip_session_sync(s);
    tm.lap("ALS iterations");
    if (rc_loop == 0 || rc_loop == 3) {
        int rc2 = cmfrec_hip_session_get_factors(s, A, B, nullptr, nullptr, C, D);
        if (rc2) rc_loop = rc2;
    }
    tm.lap("get_factors");
    if ((rc_loop == 0 || rc_loop == 3) && precompute_for_predictions) {
        if (verbose) { printf("Finishing precomputed matrices..."); fflush(stdout); }
        if (const int rc2 = epilogue(s)) rc_loop = rc2;
        if (verbose) printf("  done\n");
        tm.lap("precompute epilogue");
    }
    cmfrec_hip_session_destroy(s);
    tm.lap("session destroy");
    if (verbose && rc_loop == 0) printf("ALS procedure terminated successfully\n");
    return rc_loop;
}

int_t fit_collective_explicit_als(
    real_t *biasA, real_t *biasB, real_t *A, real_t *B, real_t *C, real_t *D, real_t *Ai, real_t *Bi,
    bool add_implicit_features, bool reset_values, int_t seed, real_t *glob_mean,
    real_t *U_colmeans, real_t *I_colmeans, int_t m, int_t n, int_t k,
    int_t ixA[], int_t ixB[], real_t *X, size_t nnz, real_t *Xfull, real_t *weight,
    bool user_bias, bool item_bias, bool center, real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique, bool scale_lam, bool scale_lam_sideinfo, bool scale_bias_const,
    real_t *scaling_biasA, real_t *scaling_biasB, real_t *U, int_t m_u, int_t p, real_t *II, int_t n_i, int_t q,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U, int_t I_row[], int_t I_col[], real_t *I_sp, size_t nnz_I,
    bool NA_as_zero_X, bool NA_as_zero_U, bool NA_as_zero_I, int_t k_main, int_t k_user, int_t k_item,
    real_t w_main, real_t w_user, real_t w_item, real_t w_implicit, int_t niter, int nthreads,
    bool verbose, bool handle_interrupt, bool use_cg, int_t max_cg_steps, bool precondition_cg, bool finalize_chol,
    bool nonneg, int_t max_cd_steps, bool nonneg_C, bool nonneg_D, bool precompute_for_predictions,
    bool include_all_X, real_t *B_plus_bias, real_t *precomputedBtB, real_t *precomputedTransBtBinvBt,
    real_t *precomputedBtXbias, real_t *precomputedBeTBeChol, real_t *precomputedBiTBi,
    real_t *precomputedTransCtCinvCt, real_t *precomputedCtCw, real_t *precomputedCtUbias)
{
    (void)max_cd_steps;
    (void)precomputedBiTBi;        // with add_implicit_features the prediction matrices are not produced here
    FitMonitor mon = take_monitor();
    if (const int rc_mon = check_monitor(mon, "fit_collective_explicit_als", m, n, k + k_main, niter, verbose)) return rc_mon;
    // collective.c:7308-7329
    if (k_user && U == nullptr && nnz_U == 0) return fail(verbose, "Cannot pass 'k_user' without U data.");
    if (k_item && II == nullptr && nnz_I == 0) return fail(verbose, "Cannot pass 'k_item' without I data.");
    if (k_main && Xfull == nullptr && nnz == 0) return fail(verbose, "Cannot pass 'k_main' without X data.");
    // side information, stage 1 (NA_as_zero_U / _I), U before I: SideInput, fit_inputs.hpp.  The dense-X and NA_as_zero_X checks below
    // read what it left; stage 2 (NaN in a dense matrix) follows them.
    SideInput su = user_side(U, m_u, p, U_row, U_col, U_sp, nnz_U, U_colmeans), si = item_side(II, n_i, q, I_row, I_col, I_sp, nnz_I, I_colmeans);
    const bool sparse_zeros_ok = !sharded_fit_wanted(devices_from_env());
    std::string refusal = su.zero_fill(NA_as_zero_U, m, ixA, nnz, sparse_zeros_ok);
    if (refusal.empty()) refusal = si.zero_fill(NA_as_zero_I, n, ixB, nnz, sparse_zeros_ok);
    if (!refusal.empty()) return fail(verbose, refusal);
    // Dense X: the rows of the present entries go through the same row kernels as a sparse X (a row's system is the sum over
    // its present entries either way: factors_closed_form, common.c:762-1075; factors_explicit_cg_dense, :1615-1749).  What the
    // reference's dense cases add is the CHOICE of solver (optimizeA Cases 1-2, common.c:2787-3116), followed here per
    // half-step.  Without weights: a half-step whose rows are all or nearly all complete is a closed-form solve whatever
    // use_cg says (Case 1; its rows with many missing entries run k CG steps from zero there, :2944-2983 -- the exact solution
    // in exact arithmetic -- and the closed form here); otherwise (Case 2) a row that misses fewer than twice as many entries
    // as its system has unknowns is solved in closed form from the precomputed B^T B (factors_closed_form, :662, :759-790:
    // that branch comes before the CG one), the others by the solver asked for.  A half-step that has rows of both kinds under
    // use_cg runs both solvers (dense_cf_A / _B).  With weights every row takes the solver asked for.
    DenseX dx;
    bool dense_chol_A = false, dense_chol_B = false;
    std::vector<unsigned char> dense_cf_A, dense_cf_B;
    std::vector<real_t> dense_mult_A, dense_mult_B;
    bool unit_weights = false;
    // With side information (round 6, fixture g33): the side that has it goes through optimizeA_collective, whose dense-X branches are the
    // same systems over the present entries (collective.c:5115-5565 shared factorisation + row-by-row corrections; :5566-5968 row by
    // row; lambda's multiplier n - cnt_NA_x = the number of present entries, :1296-1302, no precomputed matrix with lambda inside) with
    // this choice of solver: closed form whatever use_cg says when X is complete or nearly complete on that orientation and the side
    // information is dense or missing-as-zero (:5121-5130), the solver asked for otherwise.  The side without side information keeps
    // optimizeA's rules above.  Side information on exactly the rows / columns of X (the rows beyond it would take optimizeA's dense
    // cases on a sub-block, :4832-5099), complete (no NaN), no weights.
    const bool dense_side_A = Xfull && su.present(), dense_side_B = Xfull && si.present();
    const bool had_dense_X = Xfull != nullptr;
    if (Xfull) {
        if (add_implicit_features || NA_as_zero_X)
            return fail(verbose, "cmfrec_hip: dense X is implemented for the model without implicit features and NA_as_zero_X.");
        // (with weights the compiled reference corrupts its heap -- "free(): invalid pointer" on a dense X with holes, dense U and I and
        //  dense weights, either solver, both precisions -- so that combination has nothing to be pinned against)
        if ((dense_side_A || dense_side_B) && (weight || NA_as_zero_U || NA_as_zero_I))
            return fail(verbose, "cmfrec_hip: dense X with side information: not together with observation weights or NA_as_zero_U / _I.");
        if ((dense_side_A && su.rows != m) || (dense_side_B && si.rows != n))
            return fail(verbose, "cmfrec_hip: dense X with side information: U / I must have exactly the rows / columns of X.");
        if (m <= 0 || n <= 0) return fail(verbose, "cmfrec_hip: invalid dimensions.");
        dx.convert(Xfull, weight, m, n);
        if (dx.val.empty()) return fail(verbose, "cmfrec_hip: 'X' has all entries missing.");
        const int_t fewA = 2 * (k + k_main + (user_bias ? 1 : 0)), fewB = 2 * (k + k_main + (item_bias ? 1 : 0));
        // Under scale_lam a row that misses fewer than 2 k entries keeps the n lam of a complete row -- its matrix is the precomputed
        // B^T B + n lam I minus the missing rows (factors_closed_form, common.c:759-790 with BtB_has_diag; :3031-3032) -- while the
        // others take lam times their present entries.  Restated through the weighted kernels: unit weights (a multiplication by
        // one: the unweighted numbers bit for bit) and the per-row multipliers handed over after the bias start values
        // (cmfrec_hip_session_set_lambda_multipliers).
        if (!weight && (scale_lam || scale_lam_sideinfo)) {
            bool any = false;
            for (int_t r = 0; r < m && !any && !dense_side_A; r++) any = (dx.na_row[r] > 0 && dx.na_row[r] < fewA);
            for (int_t c = 0; c < n && !any && !dense_side_B; c++) any = (dx.na_col[c] > 0 && dx.na_col[c] < fewB);
            if (any) {
                // (a side with side information: the present entries, like a sparse X -- collective.c:1296-1302)
                dense_mult_A.resize((size_t)m); dense_mult_B.resize((size_t)n);
                for (int_t r = 0; r < m; r++) dense_mult_A[r] = (!dense_side_A && dx.na_row[r] < fewA) ? (real_t)n : (dx.na_row[r] < n ? (real_t)(n - dx.na_row[r]) : (real_t)1);
                for (int_t c = 0; c < n; c++) dense_mult_B[c] = (!dense_side_B && dx.na_col[c] < fewB) ? (real_t)m : (dx.na_col[c] < m ? (real_t)(m - dx.na_col[c]) : (real_t)1);
                // (the bias start values of a weighted session do not restate scale_lam_sideinfo / scale_bias_const: say so here,
                //  before anything is uploaded, and in terms of what the caller passed -- no weights)
                if ((scale_lam_sideinfo || scale_bias_const) && user_bias && item_bias && reset_values)
                    return fail(verbose, "cmfrec_hip: dense X whose rows / columns miss only a few entries, under scale_lam together with "
                                         "scale_lam_sideinfo / scale_bias_const and both biases, is not implemented (its per-row lambda "
                                         "multipliers ride on the weighted kernels, whose bias start values do not restate those options).");
                dx.w.assign(dx.val.size(), (real_t)1);
                unit_weights = true;
            }
        }
        ixA = dx.row.data(); ixB = dx.col.data(); X = dx.val.data(); nnz = dx.val.size();
        if (weight || unit_weights) weight = dx.w.data();
        if (!weight || unit_weights) {
            // Case 2 under use_cg: closed form for the rows that miss few entries, CG for the others (rows without any entry are zero)
            auto case2_chol = [&](const std::vector<int_t> &na, int_t other, int_t few, bool &mixed) {
                size_t n_few = 0, n_many = 0;
                for (int_t v : na) { if (v < few) n_few++; else if (v < other) n_many++; }
                mixed = (n_few > 0 && n_many > 0);
                return n_many == 0;
            };
            bool mixA = false, mixB = false;
            dense_chol_A = dx.full || dx.near_row || case2_chol(dx.na_row, n, fewA, mixA);
            dense_chol_B = dx.full || dx.near_col || case2_chol(dx.na_col, m, fewB, mixB);
            if (dense_side_A) { dense_chol_A = (dx.full || dx.near_row) && su.dense != nullptr; mixA = false; }
            if (dense_side_B) { dense_chol_B = (dx.full || dx.near_col) && si.dense != nullptr; mixB = false; }
            // a half-step with rows of both kinds under use_cg: the rows that miss few entries are marked for the closed form
            // (cmfrec_hip_session_set_closed_form_rows), the update runs both solvers
            if (use_cg && !nonneg && l1_lam == 0 && !l1_lam_unique) {
                if (!(dx.full || dx.near_row) && mixA) { dense_cf_A.resize((size_t)m); for (int_t r = 0; r < m; r++) dense_cf_A[r] = dx.na_row[r] < fewA; }
                if (!(dx.full || dx.near_col) && mixB) { dense_cf_B.resize((size_t)n); for (int_t c = 0; c < n; c++) dense_cf_B[c] = dx.na_col[c] < fewB; }
            }
        }
        Xfull = nullptr;
    }
    // NA_as_zero_X (sparse X whose absent entries are zeros): every half-step shares one matrix over its rows -- optimizeA Case 3
    // without side information on that side (common.c:3118-3205: closed form whatever use_cg says), optimizeA_collective with
    // the factorised shared block matrix (collective.c:5607-5617, :5700-5716) with dense complete side information
    if (NA_as_zero_X && (nonneg || l1_lam != 0 || l1_lam_unique ||
                         (scale_bias_const && (scale_lam || scale_lam_sideinfo) && (user_bias || item_bias))))
        return fail(verbose, "cmfrec_hip: NA_as_zero_X is implemented for the model without nonneg / L1 and scale_bias_const.");
    // the matrices for predictions (round 5): for the model without side information -- B_plus_bias, BtB, TransBtBinvBt as ever, plus
    // BtXbias, the constant every new row's right-hand side receives (collective.c:8938-8986)
    if (NA_as_zero_X && precompute_for_predictions && (su.present() || si.present() || add_implicit_features))
        return fail(verbose, "cmfrec_hip: NA_as_zero_X with precompute_for_predictions: the model without side information and implicit features.");
    // ... with implicit features (round 5): the model without side information and weights, closed form (optimizeA_collective's
    // general branch on a matrix all rows share, collective.c:8612 / :8783 -> :1534-1846)
    // (use_cg is accepted: the reference takes its closed-form Case 1 whatever the solver asked for, collective.c:5121-5130)
    // (round 6, fixture g37: with dense or sparse side information on exactly the rows / columns of X)
    // (and with observation weights: fixture g39)
    // ... with SPARSE side information (round 5): row by row on the shared B^T B plus the rank-1 terms of the row's own attributes
    // (collective_closed_form_block with prefer_BtB, collective.c:1534-1846) -- closed form, side information on exactly the rows /
    // columns of X, no weights
    if (NA_as_zero_X && (su.sparse() || si.sparse())) {
        if (NA_as_zero_U || NA_as_zero_I)
            return fail(verbose, "cmfrec_hip: NA_as_zero_X with sparse side information: not together with NA_as_zero_U / _I.");
        if ((su.sparse() && su.rows != m) || (si.sparse() && si.rows != n))
            return fail(verbose, "cmfrec_hip: NA_as_zero_X with side information: U / I must have exactly the rows / columns of X.");
    }
    // ... with observation weights (round 5): optimizeA Case 4's NA_as_zero + weight branches (common.c:3209-3302, :846-907,
    // :1293-1441) without side information; with DENSE complete side information the rows with entries leave the shared
    // factorisation for collective_closed_form_block's general branch (collective.c:1367-1372, :1534-1846), closed form.  Not
    // with start values for the biases: the reference's own (initialize_biases with NA_as_zero and weights) index the item biases
    // by row inside the item sweep (common.c:4727-4731).
    if (NA_as_zero_X && weight != nullptr) {
        if ((user_bias || item_bias) && reset_values)
            return fail(verbose, "cmfrec_hip: NA_as_zero_X with observation weights: pass start values for the biases (reset_values = false); "
                                 "the reference's own start values are not defined for this combination.");
        if (use_cg && !precondition_cg && k + k_main + 1 > 64)
            return fail(verbose, "cmfrec_hip: NA_as_zero_X with observation weights under CG: k + k_main + bias <= 64 (precondition_cg takes more).");
    }
    if (NA_as_zero_X && (su.dense || si.dense)) {
        // (use_cg is accepted: with a factorised shared block matrix the reference takes the closed form whatever the solver asked for)
        if ((su.dense && su.rows != m) || (si.dense && si.rows != n))
            return fail(verbose, "cmfrec_hip: NA_as_zero_X with side information: U / I must have exactly the rows / columns of X.");
        for (size_t e = 0; su.dense && e < (size_t)su.rows * (size_t)su.cols; e++)
            if (std::isnan(su.dense[e])) return fail(verbose, "cmfrec_hip: NA_as_zero_X with side information: NaN in U is not implemented.");
        for (size_t e = 0; si.dense && e < (size_t)si.rows * (size_t)si.cols; e++)
            if (std::isnan(si.dense[e])) return fail(verbose, "cmfrec_hip: NA_as_zero_X with side information: NaN in I is not implemented.");
    }
    // stage 2 of the intake: dense side information with NaN -> the sparse route on its centred present entries
    su.take_nan(); si.take_nan();
    const bool nan_side = su.nan_side || si.nan_side;
    // (asymmetry, kept: only U is refused for having nothing left; an I without a present entry counts as no I)
    if (su.nothing_present(nan_side)) return fail(verbose, "cmfrec_hip: U has no present entries.");
    // implicit features (Ai, Bi on the binary "was observed" matrix): closed-form solves, dense, sparse (round 6, fixture g32) or no
    // side information inside the shape of X, prediction matrices not produced
    if (add_implicit_features) {
        if (!Ai || !Bi) return fail(verbose, "cmfrec_hip: add_implicit_features needs the Ai and Bi outputs.");
        if (su.beyond(m) || si.beyond(n))
            return fail(verbose, "cmfrec_hip: implicit features with side information beyond X are not implemented.");
        if (precompute_for_predictions)
            return fail(verbose, "cmfrec_hip: implicit features: precompute_for_predictions is not implemented.");
        // the reference itself crashes on add_implicit_features with nonneg or an L1 penalty (its Ai / Bi updates are handed
        // a NULL thread-local buffer, collective.c:8487-8489): nothing to pin against, so not offered
        if (nonneg || l1_lam != 0 || l1_lam_unique)
            return fail(verbose, "cmfrec_hip: implicit features with nonneg / L1 are not implemented.");
        if (!(w_implicit > 0)) return fail(verbose, "cmfrec_hip: w_implicit must be positive.");
    }
    // side information: dense (no NaN) or sparse COO (missing = absent).  Sparse: Cholesky updates only, rows within X.
    if (su.bad_triplets(m) || si.bad_triplets(n))
        return fail(verbose, "cmfrec_hip: sparse side information must be COO triplets with rows inside X.");
    su.drop_if_absent(); si.drop_if_absent();
    if (su.index_out_of_range()) return fail(verbose, su.index_message());
    if (si.index_out_of_range()) return fail(verbose, si.index_message());
    if ((l1_lam != 0 || l1_lam_unique) && (su.beyond(m) || si.beyond(n)))
        return fail(verbose, "cmfrec_hip: L1 together with side information beyond X is not implemented.");
    if (nonneg || l1_lam != 0 || l1_lam_unique) use_cg = false;           // collective.c:7474-7479
    // For rows with few missing values the reference corrects a precomputed Gramian instead of summing the present entries
    // (factors_closed_form, common.c:762-790).  Unscaled lambda + Cholesky: the same solution.  Under scale_lam that Gramian
    // already carries lam x (all rows) (:3031-3032) and under CG such attributes are solved in closed form or restart from zero
    // with k steps (:2958-2985): per-attribute rules (DenseNanSide::rules, round 5) handed to the session below.  The
    // non-negative / L1 solvers see another matrix layout -- not restated, so not offered.
    if (nan_side && (nonneg || nonneg_C || nonneg_D || l1_lam != 0 || l1_lam_unique))
        return fail(verbose, "cmfrec_hip: NaN in dense side information: not together with nonneg / L1.");
    if (nan_side && had_dense_X)
        return fail(verbose, "cmfrec_hip: dense X with side information: NaN in U / I is not implemented.");
    if (precompute_for_predictions && precomputedBtB == nullptr)
        return fail(verbose, "cmfrec_hip: precompute_for_predictions needs the output buffers (cmfrec.h.in:760-778).");
    // observation weights (one per entry of X): every row solver and the start values of the biases take them; the lambda
    // multipliers of scale_lam become sums of weights (collective.c:7931-8008).  Not together with the options whose weight
    // bookkeeping is not restated: NaN side information, scale_lam_sideinfo, scale_bias_const.
    // (scale_lam_sideinfo with weights under NA_as_zero_X: the multiplier is the weights' sum + the absent entries + p, no start values)
    // Sparse side information (round 6): the row's attributes are the second gather source of the weighted row solvers, unweighted
    // themselves (collective.c:1636-1653 beside :1673-1699; block CG :2187-2208 beside :2292-2298) -- fixture g31.
    // (weights + sparse side information + scale_lam_sideinfo: the reference's multipliers add `U_csr_p[row+1] - U_csr[row]` -- a VALUE of
    //  U where its row pointer is meant, collective.c:8087, :8106 -- so there is no meaningful number to agree with: refused)
    if (weight && scale_lam_sideinfo && (su.sparse() || si.sparse()))
        return fail(verbose, "cmfrec_hip: observation weights with sparse side information under scale_lam_sideinfo are not implemented "
                             "(the reference's lambda multipliers for this combination read a value of U / I in place of a row pointer).");
    // (round 6, fixture g38: with implicit features too -- the weighted row solvers with the implicit-features term, whose own
    //  gather-sum and Ai / Bi updates take no weights, collective.c:1757-1771, :8449-8535)
    if (weight && (nan_side || (scale_lam_sideinfo && !NA_as_zero_X) ||
                   (scale_bias_const && scale_lam && (user_bias || item_bias))))
        return fail(verbose, "cmfrec_hip: observation weights together with NaN side information / scale_lam_sideinfo / "
                             "scale_bias_const are not implemented.");
    if (m <= 0 || n <= 0 || nnz == 0) return fail(verbose, "cmfrec_hip: invalid dimensions.");
    for (size_t e = 0; e < nnz; e++)
        if (ixA[e] < 0 || ixA[e] >= m || ixB[e] < 0 || ixB[e] >= n) return fail(verbose, "cmfrec_hip: X index out of range.");

    SigGuard sig(handle_interrupt);
    scale_lam = scale_lam || scale_lam_sideinfo;                          // :7465
    if (!use_cg) finalize_chol = false;                                   // :7481
    // per-matrix penalties, order: user bias, item bias, A, B, C, D (collective.c:430)
    real_t lam6[6], l16[6];
    for (int e = 0; e < 6; e++) { lam6[e] = lam_unique ? lam_unique[e] : lam; l16[e] = l1_lam_unique ? l1_lam_unique[e] : l1_lam; }
    if (w_main != (real_t)1) {                                            // :7497-7521
        lam /= w_main; l1_lam /= w_main; w_user /= w_main; w_item /= w_main; w_implicit /= w_main;
        for (int e = 0; e < 6; e++) { lam6[e] /= w_main; l16[e] /= w_main; }
    }
    const bool has_bias = user_bias || item_bias;
    // scale_bias_const: the biases' lambda is scaled by one constant -- the mean over the rows of (entries + attributes
    // counted under scale_lam_sideinfo) -- instead of row by row (collective.c:7555-7556, :8026-8048, :8071-8160)
    if (!scale_lam || !has_bias) scale_bias_const = false;
    if (scale_bias_const) {
        if (add_implicit_features || su.sparse() || si.sparse() || nan_side)
            return fail(verbose, "cmfrec_hip: scale_bias_const with implicit features / sparse or NaN side information is not implemented.");
        if (item_bias && !user_bias && !use_cg)
            return fail(verbose, "cmfrec_hip: scale_bias_const with only an item bias and the Cholesky solver: the reference leaves "
                                 "scaling_biasB unset (collective.c:7934).");
        if (!scaling_biasA || !scaling_biasB) return fail(verbose, "cmfrec_hip: scale_bias_const needs the scaling_biasA / scaling_biasB outputs.");
        auto mean_count = [&](const int_t *ix, int_t rows, int_t extra, int_t extra_rows) {
            std::vector<size_t> cnt((size_t)rows, 0);
            for (size_t e = 0; e < nnz; e++) cnt[ix[e]]++;
            double wmean = 0;
            for (int_t r = 0; r < rows; r++) {
                const real_t w = (real_t)(cnt[r] + (cnt[r] == 0)) + (real_t)((scale_lam_sideinfo && r < extra_rows) ? extra : 0);
                wmean += ((double)w - wmean) / (double)(r + 1);
            }
            return (real_t)wmean;
        };
        if (user_bias) { *scaling_biasA = mean_count(ixA, m, (su.dense || su.sz.on) ? su.cols : 0, su.rows); lam6[0] *= *scaling_biasA; l16[0] *= *scaling_biasA; }
        if (item_bias) { *scaling_biasB = mean_count(ixB, n, (si.dense || si.sz.on) ? si.cols : 0, si.rows); lam6[1] *= *scaling_biasB; l16[1] *= *scaling_biasB; }
    }
    const int k_totA = k_user + k + k_main, k_totB = k_item + k + k_main;
    const int_t m_max = std::max(m, su.rows), n_max = std::max(n, si.rows);      // rows of A / B (collective.c:7332-7335)

    // ---- global mean, common.c:3494-3524 + :3603 (nthreads selects running mean vs sum/cnt); the
    //      subtraction itself happens on the device while the CSR / CSC are built ----
    PhaseTimer tm;
    const real_t gm = center ? global_mean(X, weight, nnz, m, n, nthreads, NA_as_zero_X, nonneg) : (real_t)0;      // fit_inputs.hpp
    *glob_mean = gm;
    tm.lap("global mean");

    // ---- side information: column means + centering, common.c:4938-4997 ----
    su.center(); si.center();

    tm.lap("side info centring");
    // ---- factor start values, collective.c:8241-8274 ----
    if (reset_values) {
        const bool fill_B = (si.present() || add_implicit_features);
        cmfrng::random_parallel<real_t>(A, (size_t)m_max * k_totA, fill_B ? B : nullptr, fill_B ? (size_t)n_max * k_totB : 0, seed, true);
        if (nonneg) {                                                     // :8256-8263: non-negative start values
            for (size_t e = 0; e < (size_t)m_max * k_totA; e++) A[e] = std::fabs(A[e]);
            if (fill_B) for (size_t e = 0; e < (size_t)n_max * k_totB; e++) B[e] = std::fabs(B[e]);
        }
        if (use_cg) {
            if (!fill_B) memset(B, 0, (size_t)n_max * k_totB * sizeof(real_t));
            if (su.present()) memset(C, 0, (size_t)su.cols * (k_user + k) * sizeof(real_t));
            if (si.present()) memset(D, 0, (size_t)si.cols * (k_item + k) * sizeof(real_t));
        }
    }

    // dense X: rows / columns without a present entry are zero in the reference (optimizeA, common.c:2925-2929; factors_closed_form,
    // :667-677) -- factors and bias -- whereas the sparse path leaves such rows at their start values
    auto zero_empty_dense = [&]() {
        if (dx.na_row.empty()) return;
        // (a side with side information solves such rows from their attributes: optimizeA_collective, collective.c:1285-1331)
        for (int_t r = 0; r < m && !dense_side_A; r++) if (dx.na_row[r] == n) { memset(A + (size_t)r * k_totA, 0, (size_t)k_totA * sizeof(real_t)); if (biasA) biasA[r] = 0; }
        for (int_t c = 0; c < n && !dense_side_B; c++) if (dx.na_col[c] == m) { memset(B + (size_t)c * k_totB, 0, (size_t)k_totB * sizeof(real_t)); if (biasB) biasB[c] = 0; }
    };
    if (niter > 0) zero_empty_dense();
    cmfrec_hip_model mdl;
    memset(&mdl, 0, sizeof mdl);
    mdl.implicit = 0; mdl.m = m_max; mdl.n = n_max; mdl.m_x = m; mdl.n_x = n;
    mdl.k = k; mdl.k_main = k_main; mdl.k_user = k_user; mdl.k_item = k_item;
    mdl.user_bias = user_bias; mdl.item_bias = item_bias; mdl.scale_lam = scale_lam; mdl.scale_lam_sideinfo = scale_lam_sideinfo;
    mdl.use_cg = use_cg; mdl.max_cg_steps = max_cg_steps; mdl.precondition_cg = precondition_cg; mdl.p = su.cols; mdl.q = si.cols; mdl.m_u = su.rows; mdl.n_i = si.rows;
    mdl.lam = lam; mdl.w_user = w_user; mdl.w_item = w_item;
    mdl.row_begin = 0; mdl.row_end = m_max; mdl.col_begin = 0; mdl.col_end = n_max;
    const std::vector<int> devs = devices_from_env();                  // CMFREC_HIP_DEVICES: one ordinal = that device, several = row-block shards
    // Several devices: the plain model and the one with DENSE side information (biases, centring, CG / Cholesky, non-negativity,
    // L1, per-matrix penalties) as row-block shards that exchange the updated rows (MultiDev).  The bias start values are those
    // of the single-device driver: they are computed by a temporary session that holds the whole X on the first device (the
    // sweeps alternate over all rows and all columns, common.c:4410-4909), then handed to every shard.
    // (a dense X keeps to one device: its half-steps follow the reference's per-half-step choice of solver, dense_chol_A / _B,
    // and its empty rows are zeroed afterwards -- neither is part of multi_loop)
    const bool multi_ok = sharded_fit_wanted(devs) && !su.sparse() && !si.sparse() && !su.sz.on && !si.sz.on && su.rows <= m && si.rows <= n &&
                          !add_implicit_features && !NA_as_zero_X && !weight && dx.na_row.empty() && m >= (int_t)devs.size() && n >= (int_t)devs.size() &&
                          su.zero_rows.empty() && si.zero_rows.empty();
    if (devs.size() > 1 && !multi_ok && verbose)
        printf("cmfrec_hip: CMFREC_HIP_DEVICES lists %d devices; this configuration (sparse side information / side information beyond X / "
               "weights / implicit features / NA_as_zero / dense X) runs on the first\n", (int)devs.size());
    // the penalties and constraints of a session: the temporary bias session, every shard, the single device
    auto configure = [&](cmfrec_hip_session *sd) {
        int rc2 = 0;
        if (nonneg || nonneg_C || nonneg_D) rc2 = cmfrec_hip_session_set_nonneg(sd, nonneg, nonneg_C, nonneg_D, (int)max_cd_steps);
        if (!rc2 && l1_lam != 0) rc2 = cmfrec_hip_session_set_l1(sd, l1_lam, (int)max_cd_steps);
        if (!rc2 && (lam_unique || l1_lam_unique || scale_bias_const))
            rc2 = cmfrec_hip_session_set_lam_unique(sd, (lam_unique || scale_bias_const) ? lam6 : nullptr,
                                                    (l1_lam_unique || (scale_bias_const && l1_lam != 0)) ? l16 : nullptr, (int)max_cd_steps);
        if (!rc2 && scale_bias_const) rc2 = cmfrec_hip_session_set_scale_bias_const(sd, 1);
        return rc2;
    };
    // the biases' lambdas for their start values, clipped like common.c:4449-4452 (collective.c:8178, :8197, :8218-8219)
    const real_t lam_u = std::fabs(lam6[0]) < EPS_T ? EPS_T : lam6[0], lam_i = std::fabs(lam6[1]) < EPS_T ? EPS_T : lam6[1];
    // the matrices for predictions, single device and shards alike (collective.c:8936-9249)
    auto epilogue = [&](cmfrec_hip_session *s) {
        const int last_chol = (!use_cg || (finalize_chol && niter > 0)) ? 1 : 0;
        const int rc2 = cmfrec_hip_session_precompute(s, last_chol, include_all_X ? 1 : 0, precomputedBtB, precomputedTransBtBinvBt, nullptr,
                                                      su.had_dense ? precomputedBeTBeChol : nullptr, su.had_dense ? precomputedCtCw : nullptr,
                                                      su.had_dense ? precomputedTransCtCinvCt : nullptr);
        if (rc2) return rc2;
        if (su.naz) fill_CtUbias(precomputedCtUbias, C, su.colmeans, su.cols, k_user + k, w_user);   // collective.c:9244-9252, :10115-10123
        if (NA_as_zero_X && precomputedBtXbias != nullptr) {               // (never on the shards: multi_ok excludes NA_as_zero_X)
            // minus the sum over the items of (their bias + the mean) x their factors, the bias column as 1 (collective.c:8938-8986)
            const int_t kp = k + k_main + (user_bias ? 1 : 0);
            std::vector<double> acc((size_t)kp, 0.);
            if (item_bias || center)
                for (int_t c = 0; c < n; c++) {
                    const double coef = -((item_bias ? (double)biasB[c] : 0.) + (double)gm);
                    const real_t *b = B + (size_t)c * k_totB + k_item;
                    for (int_t f = 0; f < k + k_main; f++) acc[(size_t)f] += coef * (double)b[f];
                    if (user_bias) acc[(size_t)(kp - 1)] += coef;
                }
            for (int_t f = 0; f < kp; f++) precomputedBtXbias[f] = (real_t)acc[(size_t)f];
        }
        if (user_bias && B_plus_bias) {                                   // append_ones_last_col, :8908-8920
            for (int_t c = 0; c < n_max; c++) {
                memcpy(B_plus_bias + (size_t)c * (k_totB + 1), B + (size_t)c * k_totB, (size_t)k_totB * sizeof(real_t));
                B_plus_bias[(size_t)c * (k_totB + 1) + k_totB] = 1;
            }
        }
        return 0;
    };
    if (multi_ok) {
        int rc = 0;
        if (has_bias && reset_values) {
            cmfrec_hip_session *t = create_session(mdl, devs[0], verbose, rc);
            if (!t) return rc;
            rc = cmfrec_hip_session_set_X_coo_weighted(t, ixA, ixB, X, nullptr, nnz, gm, (real_t)1);
            if (!rc) rc = configure(t);          // (the sweeps need the attribute COUNTS under scale_lam_sideinfo, mdl.p / mdl.q, not U / I)
            if (!rc) rc = cmfrec_hip_session_set_factors(t, A, B, nullptr, nullptr, nullptr, nullptr);
            if (!rc) rc = cmfrec_hip_session_init_biases(t, lam_u, lam_i);
            if (!rc) rc = cmfrec_hip_session_get_factors(t, nullptr, nullptr, biasA, biasB, nullptr, nullptr);
            cmfrec_hip_session_destroy(t);
            if (rc) return rc;
        }
        MultiDev md;
        if (!rc) rc = build_shards(md, devs, mdl, m_max, n_max, ixA, ixB, X, nnz, gm, (real_t)1, [&](cmfrec_hip_session *sd, int d) {
            int rc2 = set_sideinfo_shard(md, sd, d, su.centred_or_null(), su.rows, su.cols, si.centred_or_null(), si.rows, si.cols);
            if (!rc2) rc2 = configure(sd);
            if (!rc2) rc2 = cmfrec_hip_session_set_factors(sd, A, B, has_bias ? biasA : nullptr, has_bias ? biasB : nullptr, C, D);
            return rc2;
        });
        int rc_loop = rc ? rc : multi_loop(md, mdl, (int)niter, finalize_chol, verbose);
        cmfrec_hip_session *s0 = md.sess.empty() ? nullptr : md.sess[0];
        if ((rc_loop == 0 || rc_loop == 3) && s0) {
            const int rc2 = cmfrec_hip_session_get_factors(s0, A, B, biasA, biasB, C, D);
            if (rc2) rc_loop = rc2;
        }
        if ((rc_loop == 0 || rc_loop == 3) && s0 && precompute_for_predictions)
            if (const int rc2 = epilogue(s0)) rc_loop = rc2;
        if (verbose && rc_loop == 0) printf("ALS procedure terminated successfully\n");
        return rc_loop;
    }
    int rc = 0;
    cmfrec_hip_session *s = create_session(mdl, devs.empty() ? -1 : devs[0], verbose, rc);
    if (!s) return rc;
    tm.lap("start values + session");
    // X - mean, COO -> CSR + CSC and the bias start values are computed on the device (coo_device.hpp)
    rc = cmfrec_hip_session_set_X_coo_weighted(s, ixA, ixB, X, weight, nnz, NA_as_zero_X ? (real_t)0 : gm, (real_t)1);
    if (!rc && NA_as_zero_X) rc = cmfrec_hip_session_set_NA_as_zero_X(s, 1, center ? 1 : 0, gm);
    tm.lap("set_X_coo (upload, sort, bins)");
    if (!rc && !dense_cf_A.empty()) rc = cmfrec_hip_session_set_closed_form_rows(s, 'A', dense_cf_A.data());
    if (!rc && !dense_cf_B.empty()) rc = cmfrec_hip_session_set_closed_form_rows(s, 'B', dense_cf_B.data());
    if (!rc) rc = hand_sides_to_session(s, su, si);
    if (!rc) rc = hand_nan_rules(s, su, 'C', k_user + k, scale_lam, use_cg);
    if (!rc) rc = hand_nan_rules(s, si, 'D', k_item + k, scale_lam, use_cg);
    if (!rc) rc = configure(s);
    if (!rc) rc = cmfrec_hip_session_set_factors(s, A, B, reset_values ? nullptr : biasA, reset_values ? nullptr : biasB, C, D);
    // Ai / Bi need no start values: their first update is a closed-form solve (collective.c:8236-8240)
    if (!rc && add_implicit_features) rc = cmfrec_hip_session_set_implicit_features(s, w_implicit, nullptr, nullptr);
    if (tm.on) cmfrec_hip_session_sync(s);
    tm.lap("side info + factors upload");
    if (!rc && has_bias && reset_values && NA_as_zero_X) {
        // bias start values, missing-as-zero branches (common.c:4207-4237 one-sided; :4453-4476, :4693-4710, :4849-4868
        // two-sided): O(nnz) running means per row and column, computed here on the host and handed over
        auto scaled_means = [&](const int_t *ix, int_t rows, int_t other) {       // running mean of the row's entries (COO order) x cnt / other
            std::vector<double> mean((size_t)rows, 0.); std::vector<size_t> cnt((size_t)rows, 0);
            for (size_t e = 0; e < nnz; e++) { const size_t r = (size_t)ix[e]; mean[r] += ((double)X[e] - mean[r]) / (double)(++cnt[r]); }
            std::vector<double> raw = mean;
            for (int_t r = 0; r < rows; r++) mean[r] *= (double)cnt[r] / (double)other;
            return std::make_tuple(mean, raw, cnt);
        };
        std::vector<real_t> bA((size_t)m_max, 0), bB((size_t)n_max, 0);
        if (user_bias && item_bias) {
            auto [meanA, rawA, cntA] = scaled_means(ixA, m, n);
            auto [meanB, rawB, cntB] = scaled_means(ixB, n, m);
            (void)rawA; (void)rawB; (void)cntA; (void)cntB;
            const double fB = (double)m / ((double)m + (double)lam_i * (scale_lam ? (double)m : 1.));
            const double fA = (double)n / ((double)n + (double)lam_u * (scale_lam ? (double)n : 1.));
            for (int iter = 0; iter < 5; iter++) {
                double bmean = 0;
                // (the reference averages biasA over `row < n` here, common.c:4697-4698; past m it reads beyond the array)
                if (iter > 0) for (int_t r = 0; r < std::min(m, n); r++) bmean += ((double)bA[r] - bmean) / (double)(r + 1);
                for (int_t c = 0; c < n; c++) bB[c] = (real_t)((meanB[c] - bmean - (double)gm) * fB);
                bmean = 0;
                if (iter > 0) for (int_t c = 0; c < n; c++) bmean += ((double)bB[c] - bmean) / (double)(c + 1);
                for (int_t r = 0; r < m; r++) bA[r] = (real_t)((meanA[r] - bmean - (double)gm) * fA);
            }
        } else if (user_bias || use_cg) {                                  // collective.c:8166-8204 (item bias alone: only with use_cg)
            const bool users = user_bias;
            const int_t rows = users ? m : n, other = users ? n : m;
            auto [mean, raw, cnt] = scaled_means(users ? ixA : ixB, rows, other);
            (void)mean;
            const double lam_b = users ? (double)lam_u : (double)lam_i;
            const double den = (double)other + lam_b * (scale_lam ? (double)other : 1.);
            std::vector<real_t> &b = users ? bA : bB;
            for (int_t r = 0; r < rows; r++) {
                if (cnt[r] > 0) {
                    double bm = raw[r];
                    bm -= (double)gm / ((double)cnt[r] / (double)other);
                    bm *= (double)cnt[r] / den;
                    b[r] = (real_t)bm;
                } else b[r] = (real_t)(-(double)gm / ((double)other / den));
            }
        }
        if (user_bias || item_bias) {
            memcpy(biasA, bA.data(), (size_t)m_max * sizeof(real_t)); memcpy(biasB, bB.data(), (size_t)n_max * sizeof(real_t));
            rc = cmfrec_hip_session_set_factors(s, nullptr, nullptr, user_bias ? biasA : nullptr, item_bias ? biasB : nullptr, nullptr, nullptr);
        }
    } else
    if (!rc && has_bias && reset_values)                                  // common.c:4410-4909
        rc = cmfrec_hip_session_init_biases(s, lam_u, lam_i);
    if (tm.on) cmfrec_hip_session_sync(s);
    tm.lap("bias init");
    // dense X under scale_lam: the rows' lambda multipliers (n for a row that misses few entries, its present entries otherwise)
    if (!rc && !dense_mult_A.empty()) rc = cmfrec_hip_session_set_lambda_multipliers(s, 'A', dense_mult_A.data());
    if (!rc && !dense_mult_B.empty()) rc = cmfrec_hip_session_set_lambda_multipliers(s, 'B', dense_mult_B.data());
    if (verbose && !rc) { printf("Starting ALS optimization routine\n\n"); fflush(stdout); }
    mon.glob_mean = gm;
    int rc_loop = rc ? rc : run_loop(s, mdl, niter, finalize_chol, verbose, add_implicit_features, dense_chol_A, dense_chol_B, mon.on ? &mon : nullptr);
    if (tm.on) cmfrec_hip_session_sync(s);
    tm.lap("ALS iterations");
    if (rc_loop == 0 || rc_loop == 3) {
        int rc2 = cmfrec_hip_session_get_factors(s, A, B, biasA, biasB, C, D);
        if (!rc2 && add_implicit_features) rc2 = cmfrec_hip_session_get_implicit_features(s, Ai, Bi);
        if (rc2) rc_loop = rc2;
    }
    if (rc_loop == 0 || rc_loop == 3) {                                   // no bias beyond the shape of X (collective.c:8296, :8923-8925)
        if (user_bias) for (int_t r = m; r < m_max; r++) biasA[r] = 0;
        if (item_bias) for (int_t c = n; c < n_max; c++) biasB[c] = 0;
        if (niter > 0) zero_empty_dense();
    }
    if ((rc_loop == 0 || rc_loop == 3) && precompute_for_predictions) {
        if (verbose) { printf("Finishing precomputed matrices..."); fflush(stdout); }
        if (const int rc2 = epilogue(s)) rc_loop = rc2;
        if (verbose) printf("  done\n");
    }
    cmfrec_hip_session_destroy(s);
    tm.lap("get_factors + precompute + destroy");
    if (verbose && rc_loop == 0) printf("ALS procedure terminated successfully\n");
    return rc_loop;
}

// ---- factors of new rows (the step after the path) -----------------------------------------------------
// Same positional signatures as the reference (src/cmfrec.h:2004-2071).  Supported: sparse X (COO or CSR, missing = not
// observed) or dense X (Xfull, NaN = not observed; compacted on the device), observation weights in either form, implicit
// features (Bi), dense U without NaN or sparse U, L1 penalties, non-negativity; no binary side information / NA_as_zero.
// Anything else returns 2 with a message on stderr.  The precomputed matrices of the reference's
// signature are optional accelerators there; here the small Gramians are rebuilt on the device from B and C (BtB of the
// implicit model, TransCtCinvCt, TransBtBinvBt and BiTBi are used when given, because they decide the result:
// collective.c:11270-11280, :3380, common.c:736-758, collective.c:1704-1707).
static int unsupported_multiple(const char *what)
{
    cmfhip::g_last_error = std::string("factors_collective_*_multiple: ") + what + " is not supported by the HIP build";
    fprintf(stderr, "cmfrec_hip: %s\n", cmfhip::g_last_error.c_str());
    return 2;
}

// the refusals of the missing-as-zero models of the new-rows handle
static int unsupported_naz(const char *what)
{
    cmfhip::g_last_error = std::string("cmfrec_hip_newrows: ") + what + " is not supported";
    return 2;
}

}  // extern "C"

// ---- the handle: a model of new rows resident on the device (cmfrec_hip_newrows_*, include/cmfrec_hip.h) ---------------------
// The rescaling rules of the two drop-in functions live here once: newrows_model_side is their model half (create), newrows_batch_side
// their batch half (factors / topN); the drop-in functions themselves are create, factors, destroy.
struct cmfrec_hip_newrows {
    cmfrec_hip_newrows_model mdl;              // the scalars; its pointers are cleared after create
    bool naz_X = false, naz_U = false;         // the missing-as-zero options (cmfrec_hip_newrows_create_ex)
    cmfhip::NewRowsState *state = nullptr;
    cmfrec_hip_ranker *ranker = nullptr;       // made by the first topN call
    int split = -1;                            // cmfrec_hip_newrows_set_split: handed to the ranker when it is made
    cmfhip::PairScorer *scorer = nullptr;      // made by the first predict call
    bool has_C = false, has_biasB = false, has_Bi = false, has_means = false;
    int_t n_sparse = 0;                        // rows of B a sparse batch may index (n_max with include_all_X), n: a dense one
    bool called = false, ranked = false;       // a solve on this handle; the last call ranked
    bool imputed = false, solved = true;       // the last call imputed; it solved (an impute call without any NaN does not)
    bool predicted = false;                    // the last call scored pairs
    ~cmfrec_hip_newrows()
    {
        cmfhip::pair_scorer_destroy(scorer);
        if (ranker) cmfrec_hip_ranker_destroy(ranker);
        cmfhip::newrows_state_destroy(state);
    }
};

namespace {

// Model half of factors_collective_explicit_multiple (factors_collective_explicit_single, collective.c:10611-10630;
// collective_factors_warm, :3694-3713) and of factors_collective_implicit_multiple (collective_factors_warm_implicit, :4000-4004).
int newrows_model_side(const cmfrec_hip_newrows_model &m, cmfhip::NewRowsModelArgs &M, int_t *n_sparse, bool naz_X = false, bool naz_U = false)
{
    const bool side = m.C != nullptr && m.p > 0;
    M.B = m.B; M.C = side ? m.C : nullptr; M.p = side ? m.p : 0; M.U_colmeans = side ? m.U_colmeans : nullptr;
    M.k = m.k; M.k_user = m.k_user; M.k_item = m.k_item; M.k_main = m.k_main;
    M.nonneg = m.nonneg != 0;
    if (m.implicit && (naz_X || naz_U)) return unsupported_naz("NA_as_zero of the implicit model");
    if (m.implicit) {
        // L1 penalty: rows with observations keep the l1_lam of the call (collective_factors_warm_implicit rescales lam and w_user by
        // w_main only, :4000-4004).
        // With side information the reference's own result is not finite (its elastic-net sweeps diverge on the block system of
        // collective_closed_form_block_implicit: +-inf in most rows of a seeded problem, tests/golden_cases.py) -- refused.
        if (m.l1_lam != 0 && side)
            return unsupported_multiple("L1 regularisation together with side information (the reference's result is not finite)");
        if (m.l1_lam != 0 && m.nonneg) return unsupported_multiple("L1 regularisation together with non-negativity");
        // BtB as the reference builds it when none is passed: + the lam of the call, before the w_main rescaling
        // (collective.c:11270-11280; not built for a single row without BeTBeChol either, where the row function does the same)
        real_t lam = m.lam, w_user = m.w_user;
        M.lam_x = lam;
        const real_t wm = m.w_main * m.w_main_multiplier;                       // collective_factors_warm_implicit, :4000-4004
        if (wm != 1) { lam /= wm; w_user /= wm; }
        M.implicit = true; M.n = m.n; *n_sparse = m.n;
        M.lam = lam; M.lam_bias = lam; M.w_user = w_user; M.l1_lam = m.l1_lam; M.l1_lam_bias = m.l1_lam;
        M.BtB_pre = m.BtB;
        return 0;
    }
    const bool Bi = m.add_implicit_features != 0;
    if (Bi && !m.Bi) return unsupported_multiple("add_implicit_features without Bi");
    // missing-as-zero models: what the handle does not solve under either option
    const bool naz = naz_X || naz_U;
    if (naz && m.nonneg) return unsupported_naz("NA_as_zero together with non-negativity");
    if (naz && (m.l1_lam != 0 || m.l1_lam_unique != nullptr)) return unsupported_naz("NA_as_zero together with an L1 penalty");
    if (naz && Bi) return unsupported_naz("NA_as_zero together with implicit features");
    if (naz && m.scale_bias_const) return unsupported_naz("NA_as_zero together with scale_bias_const");
    const bool ub = m.user_bias != 0;
    // factors_collective_explicit_single, collective.c:10611-10630
    real_t lam = m.lam, l1_lam = m.l1_lam, lam_bias = m.lam, l1_lam_bias = m.l1_lam, w_user = m.w_user, w_implicit = m.w_implicit;
    bool scale_bias_const = m.scale_bias_const != 0;
    const bool scale_any = m.scale_lam || m.scale_lam_sideinfo;
    if (m.lam_unique) { lam_bias = m.lam_unique[ub ? 0 : 2]; lam = m.lam_unique[2]; }
    if (m.l1_lam_unique) { l1_lam_bias = m.l1_lam_unique[ub ? 0 : 2]; l1_lam = m.l1_lam_unique[2]; }
    if (!ub) scale_bias_const = false;
    if (scale_any && scale_bias_const) { lam_bias *= m.scaling_biasA; l1_lam_bias *= m.scaling_biasA; }
    // BiTBi carries the w_implicit of the call (batch driver, :11016-11020), the right-hand side the rescaled one (:3706-3714)
    const real_t w_implicit_gram = w_implicit;
    if (m.w_main != 1) {                                                        // collective_factors_warm, :3694-3713
        w_user /= m.w_main; w_implicit /= m.w_main; lam /= m.w_main; lam_bias /= m.w_main; l1_lam /= m.w_main; l1_lam_bias /= m.w_main;
    }
    const bool l1on = l1_lam != 0 || (ub && l1_lam_bias != 0);
    if (l1on && m.nonneg) return unsupported_multiple("L1 regularisation together with non-negativity");
    // rows without side information and without a bias: the reference passes scale_lam where factors_closed_form
    // expects scale_bias_const (:3789-3799), so the last factor keeps the unscaled lam (not with implicit features: those
    // rows go through the block solver, :3759-3760)
    if (!ub && !Bi) scale_bias_const = scale_any;
    // B's rows: with dense X or implicit features the n columns of Xfull / rows of Bi bound the item indices
    const bool more = m.include_all_X && m.n_max > m.n;
    *n_sparse = (more && !Bi) ? m.n_max : m.n;
    M.n = more ? m.n_max : m.n;
    M.biasB = m.biasB; M.user_bias = ub;
    M.NA_as_zero_X = naz_X; M.NA_as_zero_U = naz_U; M.glob_mean = m.glob_mean; M.n_x = m.n;
    M.lam = lam; M.lam_bias = lam_bias; M.lam_x = lam; M.w_user = w_user;
    M.scale_lam = m.scale_lam != 0; M.scale_lam_sideinfo = m.scale_lam_sideinfo != 0; M.scale_bias_const = scale_bias_const;
    M.l1_lam = l1_lam; M.l1_lam_bias = l1_lam_bias;
    // (TransCtCinvCt: not with non-negativity or an L1 penalty, collective.c:3378)
    M.TransCtCinvCt_pre = (m.nonneg || l1on || !side) ? nullptr : m.TransCtCinvCt;
    if (Bi) { M.Bi = m.Bi; M.n_Bi = m.n; M.w_implicit = w_implicit; M.w_implicit_gram = w_implicit_gram; M.BiTBi_pre = m.BiTBi; }
    // TransBtBinvBt: complete dense rows of the model without side information (common.c:736-758, n_BtB == n); the batch decides
    // the rest (no weights, no side information in it)
    if (m.TransBtBinvBt && !m.nonneg && !l1on && !Bi && !more) { M.TransBtBinvBt_pre = m.TransBtBinvBt; M.n_TB = m.n; }
    return 0;
}

// Batch half: the refusals that depend on the batch, preprocess_vec's shift by the global mean (:6337-6388; dense X: on the
// device, the item bias: inside the gather) or the implicit model's log / alpha (:10802-10810, :4006-4016).  `vals` holds the
// transformed values while the batch runs.  1: a batch without rows (nothing to do), 0: run it, 2: refused.
int newrows_batch_side(const cmfrec_hip_newrows &h, const cmfrec_hip_newrows_batch &b, cmfhip::NewRowsBatchArgs &bt, std::vector<real_t> &vals_tmp)
{
    const cmfrec_hip_newrows_model &m = h.mdl;
    int_t mx = b.m, m_u = b.m_u;
    const real_t *U = h.has_C ? b.U : nullptr, *Xfull = b.Xfull, *weight = b.weight;
    const bool spU = h.has_C && (b.U == nullptr && (b.nnz_U || b.U_csr_p));
    if (Xfull && (b.nnz || b.Xcsr_p)) return unsupported_multiple("X both as a dense and as a sparse matrix");
    if (m.implicit && (Xfull || weight)) {
        cmfhip::g_last_error = "cmfrec_hip_factors_multiple: observation weights, dense X and implicit features belong to the explicit model";
        return 2;
    }
    if (!h.has_C && m.p > 0 && (b.U || b.nnz_U || b.U_csr_p)) {             // side information for a model without C
        cmfhip::g_last_error = "cmfrec_hip_factors_multiple: invalid arguments";
        return 2;
    }
    if (U == nullptr && !spU) m_u = 0;
    if (std::max(mx, m_u) <= 0) return 1;                                       // rows out: max(m, m_u), collective.c:11210
    if (mx <= 0) { Xfull = nullptr; weight = nullptr; }
    if (U) for (size_t e = 0; e < (size_t)m_u * (size_t)m.p; e++) if (std::isnan(U[e]))
        return (h.naz_X || h.naz_U) ? unsupported_naz("NA_as_zero together with missing values in a dense U")
                                                  : unsupported_multiple("missing values in U");
    const bool side = U != nullptr || spU;
    if (!m.implicit) {
        // The block solver's weighted right-hand side of sparse X is the NA_as_zero one, w x - (w - 1)(glob_mean + biasB), applied
        // to values that preprocess_vec has centred already (collective.c:1743-1753): with a mean or item biases the reference's
        // rows are not the solution of the weighted model.  Not restated.
        if (weight && !Xfull && (side || h.has_Bi) && (m.glob_mean != 0 || h.has_biasB))
            return unsupported_multiple("observation weights of sparse X together with glob_mean / biasB and side information or implicit "
                                        "features (the reference's right-hand side is not the weighted model's, collective.c:1743-1753)");
        // A dense row of NaN with side information reaches the side-information-only solution through collective_factors_warm,
        // which has centred u already and hands it on with the column means: they are subtracted twice (:3616, :3662-3677, :3337).
        if (Xfull && U && h.has_means && !h.has_Bi)
            for (int_t r = 0; r < std::min(mx, m_u); r++) {
                int_t c = 0;
                while (c < m.n && std::isnan(Xfull[(size_t)r * (size_t)m.n + c])) c++;
                if (c == m.n)
                    return unsupported_multiple("a dense row of X without any observation together with U and U_colmeans (the reference "
                                                "centres that row's side information twice, collective.c:3616, :3337)");
            }
    }
    const size_t nz = Xfull ? 0 : (b.Xcsr_p ? b.Xcsr_p[mx > 0 ? mx : 0] : b.nnz);
    const real_t *vals = b.Xcsr_p ? b.Xcsr : b.X;
    if (m.implicit) {
        if ((m.apply_log_transf || m.alpha != 1) && nz) {
            vals_tmp.assign(vals, vals + nz);
            if (m.apply_log_transf) for (size_t e = 0; e < nz; e++) vals_tmp[e] = std::log(vals_tmp[e]);   // :10802-10810
            if (m.alpha != 1) for (size_t e = 0; e < nz; e++) vals_tmp[e] *= m.alpha;                      // :4006-4016
            vals = vals_tmp.data();
        }
    } else if (m.glob_mean != 0 && nz && !h.naz_X) {
        // (under NA_as_zero_X the mean is part of every cell's target: it enters through the constant BtXbias, session.hip)
        vals_tmp.assign(vals, vals + nz);
        for (size_t e = 0; e < nz; e++) vals_tmp[e] -= m.glob_mean;
        vals = vals_tmp.data();
    }
    bt.m_x = mx; bt.m_u = m_u; bt.n = Xfull ? m.n : h.n_sparse;
    bt.U = U;
    if (spU) {
        bt.U_row = b.U_row; bt.U_col = b.U_col; bt.U_sp = b.U_sp; bt.nnz_U = b.nnz_U;
        bt.U_csr_p = b.U_csr_p; bt.U_csr_i = b.U_csr_i; bt.U_csr = b.U_csr;
    }
    bt.ixA = b.ixA; bt.ixB = b.ixB; bt.X = (b.Xcsr_p || Xfull) ? nullptr : vals; bt.nnz = Xfull ? 0 : b.nnz;
    bt.Xcsr_p = b.Xcsr_p; bt.Xcsr_i = b.Xcsr_i; bt.Xcsr = b.Xcsr_p ? vals : nullptr;
    bt.weight = Xfull ? nullptr : weight; bt.Xfull = Xfull; bt.weight_full = Xfull ? weight : nullptr;
    bt.glob_mean_full = m.glob_mean;
    // (a dense row of NaN reaches the side-information-only solution through collective_factors_warm, which does not hand
    //  TransCtCinvCt on, :3662-3677)
    bt.allow_TransCtCinvCt = Xfull == nullptr;
    return 0;
}

// the raw return code of the batch run (0 .. 4)
int newrows_solve(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, real_t *A, real_t *biasA, bool *empty)
{
    *empty = false;
    if (h == nullptr || batch == nullptr || h->state == nullptr) {
        cmfhip::g_last_error = "cmfrec_hip_newrows: invalid arguments";
        return 2;
    }
    return cmfhip::guarded([&]() {
        cmfhip::NewRowsBatchArgs bt;
        std::vector<real_t> vals_tmp;
        const int brc = newrows_batch_side(*h, *batch, bt, vals_tmp);
        if (brc == 1) { *empty = true; return 0; }
        if (brc) return brc;
        h->ranked = false; h->imputed = false; h->predicted = false;
        const int rc = cmfhip::newrows_state_run(h->state, bt, A, biasA);
        if (rc == 0) { h->called = true; h->solved = true; }
        return rc;
    });
}

}  // namespace

extern "C" {

int cmfrec_hip_sizeof_newrows_model(void) { return (int)sizeof(cmfrec_hip_newrows_model); }

int cmfrec_hip_sizeof_newrows_model_ex(void) { return (int)sizeof(cmfrec_hip_newrows_model_ex); }

}  // extern "C"

namespace {

cmfrec_hip_newrows *newrows_create(const cmfrec_hip_newrows_model *model, bool naz_X, bool naz_U, int device)
{
    cmfrec_hip_newrows *h = nullptr;
    const int rc = cmfhip::guarded([&]() {
        if (model == nullptr) {
            cmfhip::g_last_error = "cmfrec_hip_newrows_create: invalid arguments";
            return 2;
        }
        cmfhip::NewRowsModelArgs M;
        int_t n_sparse = 0;
        if (int mrc = newrows_model_side(*model, M, &n_sparse, naz_X, naz_U)) return mrc;
        h = new cmfrec_hip_newrows();
        h->mdl = *model;
        h->naz_X = naz_X; h->naz_U = naz_U;
        h->n_sparse = n_sparse;
        h->has_C = M.C != nullptr; h->has_biasB = M.biasB != nullptr; h->has_Bi = M.Bi != nullptr; h->has_means = M.U_colmeans != nullptr;
        int src = 0;
        h->state = cmfhip::newrows_state_create(M, device, &src);
        if (h->state == nullptr) return src ? src : 4;
        cmfrec_hip_newrows_model &m = h->mdl;
        m.B = m.C = m.U_colmeans = m.biasB = m.Bi = m.lam_unique = m.l1_lam_unique = m.BtB = m.TransBtBinvBt = m.BiTBi = m.TransCtCinvCt = nullptr;
        return 0;
    });
    cmfhip::g_last_rc = rc;
    if (rc != 0) {
        delete h;
        return nullptr;
    }
    return h;
}

}  // namespace

extern "C" {

cmfrec_hip_newrows *cmfrec_hip_newrows_create(const cmfrec_hip_newrows_model *model, int device)
{
    return newrows_create(model, false, false, device);
}

cmfrec_hip_newrows *cmfrec_hip_newrows_create_ex(const cmfrec_hip_newrows_model_ex *model, int device)
{
    return newrows_create(model ? &model->base : nullptr, model && model->NA_as_zero_X != 0, model && model->NA_as_zero_U != 0, device);
}

int cmfrec_hip_newrows_factors(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, real_t *A, real_t *biasA)
{
    bool empty = false;
    if (h != nullptr && batch != nullptr && A == nullptr && std::max(batch->m, batch->m_u) > 0) {
        cmfhip::g_last_error = "cmfrec_hip_newrows_factors: invalid arguments";
        return 2;
    }
    const int rc = newrows_solve(h, batch, A, biasA, &empty);
    return rc > 3 ? 1 : rc;
}

int cmfrec_hip_newrows_topN(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, int exclude_seen,
                            const size_t excl_p[], const int_t excl_i[], int_t n_top,
                            int_t *out_ids, real_t *out_scores, real_t *A, real_t *biasA)
{
    const char *fn = "cmfrec_hip_newrows_topN";
    if (h == nullptr || batch == nullptr || h->state == nullptr || n_top <= 0 || out_ids == nullptr) {
        cmfhip::g_last_error = std::string(fn) + ": invalid arguments";
        return 2;
    }
    const int_t kr = h->mdl.k + h->mdl.k_main;
    if (int rc = cmfhip::ranker_check_limits(fn, kr, n_top, cmfhip::newrows_state_view(h->state).n)) return rc;
    bool empty = false;
    if (int rc = newrows_solve(h, batch, A, biasA, &empty)) return rc;
    if (empty) return 0;
    const int rc = cmfhip::guarded([&]() {
        const cmfhip::NewRowsView v = cmfhip::newrows_state_view(h->state);
        if (h->ranker == nullptr) {
            h->ranker = cmfhip::ranker_create_from_device(v.dB + h->mdl.k_item, v.ldB, v.n, kr, v.dbiasB, v.device);
            if (h->ranker == nullptr) return cmfhip::g_last_rc ? cmfhip::g_last_rc : 4;
            (void)cmfrec_hip_ranker_set_split(h->ranker, h->split);
        }
        const size_t *dp = nullptr;
        const int *di = nullptr;
        if (int erc = cmfhip::newrows_state_exclusions(h->state, exclude_seen != 0, excl_p, excl_i, &dp, &di)) return erc;
        return cmfhip::ranker_topN_device(h->ranker, fn, v.dA + h->mdl.k_user, v.ldA, v.rows, dp, di, n_top, out_ids, out_scores);
    });
    if (rc == 0) h->ranked = true;
    return rc;
}

int cmfrec_hip_newrows_topN_candidates(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, const size_t cand_p[],
                                       const int_t cand_i[], int exclude_seen, const size_t excl_p[], const int_t excl_i[],
                                       int_t n_top, int_t *out_ids, real_t *out_scores, real_t *A, real_t *biasA)
{
    const char *fn = "cmfrec_hip_newrows_topN_candidates";
    if (h == nullptr || batch == nullptr || h->state == nullptr || n_top <= 0 || out_ids == nullptr || cand_p == nullptr) {
        cmfhip::g_last_error = std::string(fn) + ": invalid arguments";
        return 2;
    }
    const int_t kr = h->mdl.k + h->mdl.k_main;
    if (int rc = cmfhip::ranker_check_limits(fn, kr, n_top, cmfhip::newrows_state_view(h->state).n)) return rc;
    bool empty = false;
    if (int rc = newrows_solve(h, batch, A, biasA, &empty)) return rc;
    if (empty) return 0;
    const int rc = cmfhip::guarded([&]() {
        const cmfhip::NewRowsView v = cmfhip::newrows_state_view(h->state);
        if (h->ranker == nullptr) {
            h->ranker = cmfhip::ranker_create_from_device(v.dB + h->mdl.k_item, v.ldB, v.n, kr, v.dbiasB, v.device);
            if (h->ranker == nullptr) return cmfhip::g_last_rc ? cmfhip::g_last_rc : 4;
            (void)cmfrec_hip_ranker_set_split(h->ranker, h->split);
        }
        const size_t *dp = nullptr;
        const int *di = nullptr;
        if (int erc = cmfhip::newrows_state_exclusions(h->state, exclude_seen != 0, excl_p, excl_i, &dp, &di)) return erc;
        return cmfhip::ranker_topN_candidates_device(h->ranker, fn, v.dA + h->mdl.k_user, v.ldA, v.rows, cand_p, cand_i, dp, di, n_top,
                                                     out_ids, out_scores);
    });
    if (rc == 0) h->ranked = true;
    return rc;
}

int cmfrec_hip_newrows_ranks(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, const size_t held_p[], const int_t held_i[],
                             int exclude_seen, const size_t excl_p[], const int_t excl_i[], int_t *out_rank, real_t *out_scores,
                             int_t *out_pool, real_t *A, real_t *biasA)
{
    const char *fn = "cmfrec_hip_newrows_ranks";
    if (h == nullptr || batch == nullptr || h->state == nullptr || held_p == nullptr) {
        cmfhip::g_last_error = std::string(fn) + ": invalid arguments";
        return 2;
    }
    const int_t kr = h->mdl.k + h->mdl.k_main;
    if (int rc = cmfhip::ranker_check_limits(fn, kr, 1, cmfhip::newrows_state_view(h->state).n)) return rc;
    bool empty = false;
    if (int rc = newrows_solve(h, batch, A, biasA, &empty)) return rc;
    if (empty) return 0;
    const int rc = cmfhip::guarded([&]() {
        const cmfhip::NewRowsView v = cmfhip::newrows_state_view(h->state);
        if (h->ranker == nullptr) {
            h->ranker = cmfhip::ranker_create_from_device(v.dB + h->mdl.k_item, v.ldB, v.n, kr, v.dbiasB, v.device);
            if (h->ranker == nullptr) return cmfhip::g_last_rc ? cmfhip::g_last_rc : 4;
            (void)cmfrec_hip_ranker_set_split(h->ranker, h->split);
        }
        const size_t *dp = nullptr;
        const int *di = nullptr;
        if (int erc = cmfhip::newrows_state_exclusions(h->state, exclude_seen != 0, excl_p, excl_i, &dp, &di)) return erc;
        return cmfhip::ranker_ranks_device(h->ranker, fn, v.dA + h->mdl.k_user, v.ldA, v.rows, held_p, held_i, dp, di, out_rank,
                                           out_scores, out_pool);
    });
    if (rc == 0) h->ranked = true;
    return rc;
}

int cmfrec_hip_newrows_impute(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, real_t *Xout, real_t *A, real_t *biasA)
{
    auto bad = [](const char *what) { cmfhip::g_last_error = std::string("cmfrec_hip_newrows_impute: ") + what; return 2; };
    if (h == nullptr || batch == nullptr || h->state == nullptr || Xout == nullptr) return bad("invalid arguments");
    if (h->mdl.implicit) return bad("imputation belongs to the explicit model");
    if (batch->Xfull == nullptr || batch->nnz || batch->Xcsr_p) return bad("X must be a dense matrix (Xfull) with NaN for the entries to impute");
    if (batch->m <= 0) return bad("a batch without rows of X");
    return cmfhip::guarded([&]() {
        cmfhip::NewRowsBatchArgs bt;
        std::vector<real_t> vals_tmp;
        if (int brc = newrows_batch_side(*h, *batch, bt, vals_tmp)) return brc;      // (1, a batch without rows, is ruled out above)
        h->ranked = false; h->imputed = false; h->predicted = false;
        bool solved = false;
        const int rc = cmfhip::newrows_state_impute(h->state, bt, Xout, A, biasA, &solved);
        if (rc == 0) { h->called = true; h->imputed = true; h->solved = solved; }
        return rc;
    });
}

int cmfrec_hip_newrows_predict(cmfrec_hip_newrows *h, const cmfrec_hip_newrows_batch *batch, const int_t *row, const int_t *col,
                               size_t n_pairs, real_t *out, real_t *A, real_t *biasA)
{
    if (h == nullptr || batch == nullptr || h->state == nullptr || (n_pairs > 0 && (!row || !col || !out))) {
        cmfhip::g_last_error = "cmfrec_hip_newrows_predict: invalid arguments";
        return 2;
    }
    bool empty = false;
    if (int rc = newrows_solve(h, batch, A, biasA, &empty)) return rc > 3 ? 1 : rc;        // (the codes of _factors)
    const int rc = cmfhip::guarded([&]() {
        const cmfhip::NewRowsView v = cmfhip::newrows_state_view(h->state);
        if (h->scorer == nullptr) h->scorer = cmfhip::pair_scorer_create(v.device);
        const cmfrec_hip_newrows_model &m = h->mdl;
        const int_t kk = m.k + m.k_main, rows = empty ? 0 : v.rows;
        const bool ub = !m.implicit && v.ldA > (size_t)(m.k_user + kk);          // a factor row ends in its bias
        return cmfhip::pair_scorer_run(h->scorer, rows ? v.dA + m.k_user : nullptr, v.ldA, rows, (ub && rows) ? v.dA + m.k_user + kk : nullptr,
                                       v.ldA, v.dB + m.k_item, v.ldB, v.n, kk, m.implicit ? nullptr : v.dbiasB,
                                       m.implicit ? (real_t)0 : m.glob_mean, m.implicit != 0, row, col, n_pairs, out);
    });
    // (a batch without rows leaves newrows_solve before it clears what the call before left: what the last call was is set here)
    if (rc == 0) { h->called = true; h->ranked = false; h->imputed = false; h->predicted = true; if (empty) h->solved = false; }
    return rc > 3 ? 1 : rc;
}

int cmfrec_hip_newrows_set_split(cmfrec_hip_newrows *h, int slices)
{
    if (h == nullptr || slices < -1) {
        cmfhip::g_last_error = "cmfrec_hip_newrows_set_split: invalid arguments (-1: off, 0: the planner's choice, >= 1: that many slices)";
        return 2;
    }
    h->split = slices;
    return h->ranker ? cmfrec_hip_ranker_set_split(h->ranker, slices) : 0;
}

int cmfrec_hip_newrows_kernel_ms(cmfrec_hip_newrows *h, double *solve_ms, double *rank_ms)
{
    if (h == nullptr || h->state == nullptr || !h->called) {
        cmfhip::g_last_error = "cmfrec_hip_newrows_kernel_ms: no call on this handle yet";
        return 2;
    }
    return cmfhip::guarded([&]() {
        double s = 0, r = 0;
        if (h->solved) { if (int rc = cmfhip::newrows_state_solve_ms(h->state, &s)) return rc; }
        if (h->imputed) r = cmfhip::newrows_state_fill_ms(h->state);
        if (h->ranked) { if (int rc = cmfrec_hip_ranker_kernel_ms(h->ranker, &r)) return rc; }
        if (h->predicted) r = cmfhip::pair_scorer_ms(h->scorer);
        if (solve_ms) *solve_ms = s;
        if (rank_ms) *rank_ms = r;
        return 0;
    });
}

void cmfrec_hip_newrows_destroy(cmfrec_hip_newrows *h)
{
    delete h;
}

int cmfrec_hip_newrows_naz_launch_waves(cmfrec_hip_newrows *h, int *waves)
{
    if (h == nullptr || h->state == nullptr || waves == nullptr) {
        cmfhip::g_last_error = "cmfrec_hip_newrows_naz_launch_waves: invalid arguments";
        return 2;
    }
    *waves = cmfhip::newrows_state_naz_waves(h->state);
    return 0;
}

int cmfrec_hip_factors_multiple_naz(const cmfrec_hip_newrows_model_ex *model, const cmfrec_hip_newrows_batch *batch, real_t *A, real_t *biasA)
{
    if (model == nullptr || batch == nullptr) {
        cmfhip::g_last_error = "cmfrec_hip_factors_multiple_naz: invalid arguments";
        return 2;
    }
    cmfrec_hip_newrows *h = cmfrec_hip_newrows_create_ex(model, -1);
    if (h == nullptr) {
        const int ec = cmfrec_hip_last_error_code();
        return ec > 3 ? 1 : (ec ? ec : 1);
    }
    const int rc = cmfrec_hip_newrows_factors(h, batch, A, biasA);
    cmfrec_hip_newrows_destroy(h);
    return rc;
}

}  // extern "C"

namespace {

// the pairs of a predict_X_new_* call: row indexes the batch's rows, col the items
struct PredictPairs {
    const int_t *row, *col;
    size_t n;
    real_t *out;
};

// factors_collective_explicit_multiple, impute_X_collective_explicit (which is that call followed by the fill, collective.c:
// 11429-11463) and predict_X_new_collective_explicit (that call followed by predict_X_old_collective_explicit, :11913-11960):
// handle created, one batch, handle destroyed.  Ximpute: Xfull, filled in place; pairs: scored from the device factors; both
// null: the factors.
int_t explicit_multiple_dropin(
    real_t *Ximpute, const PredictPairs *pairs, bool user_bias,
    real_t *A, real_t *biasA, int_t m,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U, bool NA_as_zero_X,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *Ub, int_t m_ubin, int_t pbin,
    real_t *C, real_t *Cb,
    real_t glob_mean, real_t *biasB,
    real_t *U_colmeans,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *Xfull, int_t n,
    real_t *weight,
    real_t *B,
    real_t *Bi, bool add_implicit_features,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique,
    bool scale_lam, bool scale_lam_sideinfo,
    bool scale_bias_const, real_t scaling_biasA,
    real_t w_main, real_t w_user, real_t w_implicit,
    int_t n_max, bool include_all_X,
    real_t *BtB, real_t *TransBtBinvBt, real_t *BtXbias, real_t *BeTBeChol, real_t *BiTBi,
    real_t *TransCtCinvCt, real_t *CtCw, real_t *CtUbias, real_t *B_plus_bias,
    int nthreads)
{
    (void)m_ubin; (void)pbin; (void)Cb;
    (void)BtB; (void)BtXbias; (void)BeTBeChol; (void)CtCw; (void)CtUbias; (void)B_plus_bias;
    (void)nthreads;
    if (NA_as_zero_U || NA_as_zero_X) return unsupported_multiple("NA_as_zero");
    const bool spU = (U == nullptr && (nnz_U || U_csr_p));
    if (Ub) return unsupported_multiple("binary side information");
    if (Xfull && (nnz || Xcsr_p)) return unsupported_multiple("X both as a dense and as a sparse matrix");
    if (add_implicit_features && !Bi) return unsupported_multiple("add_implicit_features without Bi");
    if (U == nullptr && !spU) { m_u = 0; }
    if (std::max(m, m_u) <= 0 && !pairs) return 0;
    if (m <= 0) { Xfull = nullptr; weight = nullptr; }
    const bool side = U != nullptr || spU;
    // the model as this batch sees it: side information only where the batch has some, a bias unknown where biasA is asked for
    cmfrec_hip_newrows_model mdl;
    memset(&mdl, 0, sizeof mdl);
    mdl.n = n; mdl.n_max = n_max; mdl.include_all_X = include_all_X; mdl.p = side ? p : 0;
    mdl.user_bias = user_bias; mdl.add_implicit_features = add_implicit_features;
    mdl.k = k; mdl.k_user = k_user; mdl.k_item = k_item; mdl.k_main = k_main;
    mdl.scale_lam = scale_lam; mdl.scale_lam_sideinfo = scale_lam_sideinfo; mdl.scale_bias_const = scale_bias_const;
    mdl.nonneg = nonneg;
    mdl.glob_mean = glob_mean; mdl.lam = lam; mdl.l1_lam = l1_lam; mdl.scaling_biasA = scaling_biasA;
    mdl.w_main = w_main; mdl.w_user = w_user; mdl.w_implicit = w_implicit; mdl.alpha = 1; mdl.w_main_multiplier = 1;
    mdl.B = B; mdl.C = side ? C : nullptr; mdl.U_colmeans = U_colmeans; mdl.biasB = biasB; mdl.Bi = add_implicit_features ? Bi : nullptr;
    mdl.lam_unique = lam_unique; mdl.l1_lam_unique = l1_lam_unique;
    mdl.TransBtBinvBt = (Xfull && !side && !weight) ? TransBtBinvBt : nullptr; mdl.BiTBi = add_implicit_features ? BiTBi : nullptr;
    mdl.TransCtCinvCt = TransCtCinvCt;
    cmfrec_hip_newrows_batch bt;
    memset(&bt, 0, sizeof bt);
    bt.m = m; bt.m_u = m_u; bt.U = U;
    bt.U_row = U_row; bt.U_col = U_col; bt.U_sp = U_sp; bt.nnz_U = nnz_U; bt.U_csr_p = U_csr_p; bt.U_csr_i = U_csr_i; bt.U_csr = U_csr;
    bt.X = X; bt.ixA = ixA; bt.ixB = ixB; bt.nnz = nnz; bt.Xcsr_p = Xcsr_p; bt.Xcsr_i = Xcsr_i; bt.Xcsr = Xcsr;
    bt.Xfull = Xfull; bt.weight = weight;
    cmfrec_hip_newrows *h = cmfrec_hip_newrows_create(&mdl, -1);
    if (h == nullptr) {
        const int ec = cmfrec_hip_last_error_code();
        if (ec == 2) fprintf(stderr, "%s\n", cmfrec_hip_last_error());
        return ec > 3 ? 1 : (ec ? ec : 1);
    }
    bool empty = false;
    const int rc = Ximpute ? cmfrec_hip_newrows_impute(h, &bt, Ximpute, A, biasA)
                 : pairs ? cmfrec_hip_newrows_predict(h, &bt, pairs->row, pairs->col, pairs->n, pairs->out, A, biasA)
                         : newrows_solve(h, &bt, A, biasA, &empty);
    cmfrec_hip_newrows_destroy(h);
    if (rc == 2) fprintf(stderr, "%s\n", cmfrec_hip_last_error());
    return rc > 3 ? 1 : rc;
}

}  // namespace

extern "C" {

int_t factors_collective_explicit_multiple(
    real_t *A, real_t *biasA, int_t m,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U, bool NA_as_zero_X,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *Ub, int_t m_ubin, int_t pbin,
    real_t *C, real_t *Cb,
    real_t glob_mean, real_t *biasB,
    real_t *U_colmeans,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *Xfull, int_t n,
    real_t *weight,
    real_t *B,
    real_t *Bi, bool add_implicit_features,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique,
    bool scale_lam, bool scale_lam_sideinfo,
    bool scale_bias_const, real_t scaling_biasA,
    real_t w_main, real_t w_user, real_t w_implicit,
    int_t n_max, bool include_all_X,
    real_t *BtB, real_t *TransBtBinvBt, real_t *BtXbias, real_t *BeTBeChol, real_t *BiTBi,
    real_t *TransCtCinvCt, real_t *CtCw, real_t *CtUbias, real_t *B_plus_bias,
    int nthreads)
{
    return explicit_multiple_dropin(nullptr, nullptr, biasA != nullptr, A, biasA, m, U, m_u, p, NA_as_zero_U, NA_as_zero_X, nonneg, U_row, U_col, U_sp, nnz_U,
                                    U_csr_p, U_csr_i, U_csr, Ub, m_ubin, pbin, C, Cb, glob_mean, biasB, U_colmeans, X, ixA, ixB, nnz, Xcsr_p,
                                    Xcsr_i, Xcsr, Xfull, n, weight, B, Bi, add_implicit_features, k, k_user, k_item, k_main, lam, lam_unique,
                                    l1_lam, l1_lam_unique, scale_lam, scale_lam_sideinfo, scale_bias_const, scaling_biasA, w_main, w_user,
                                    w_implicit, n_max, include_all_X, BtB, TransBtBinvBt, BtXbias, BeTBeChol, BiTBi, TransCtCinvCt, CtCw,
                                    CtUbias, B_plus_bias, nthreads);
}

// impute_X_collective_explicit, reference src/cmfrec.h (body src/collective.c:11351-11544): Xfull's NaN replaced in place.  The
// reference returns 0 for a matrix without NaN before it looks at anything else (:11424-11427); so does this.
int_t impute_X_collective_explicit(
    int_t m, bool user_bias,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *Ub, int_t m_ubin, int_t pbin,
    real_t *C, real_t *Cb,
    real_t glob_mean, real_t *biasB,
    real_t *U_colmeans,
    real_t *Xfull, int_t n,
    real_t *weight,
    real_t *B,
    real_t *Bi, bool add_implicit_features,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique,
    bool scale_lam, bool scale_lam_sideinfo,
    bool scale_bias_const, real_t scaling_biasA,
    real_t w_main, real_t w_user, real_t w_implicit,
    int_t n_max, bool include_all_X,
    real_t *BtB,
    real_t *TransBtBinvBt,
    real_t *BeTBeChol,
    real_t *BiTBi,
    real_t *TransCtCinvCt,
    real_t *CtCw,
    real_t *CtUbias,
    real_t *B_plus_bias,
    int nthreads)
{
    if (Xfull == nullptr || m <= 0 || n <= 0) return 0;
    const size_t total = (size_t)m * (size_t)n;
    size_t e = 0;
    while (e < total && !std::isnan(Xfull[e])) e++;
    if (e == total) return 0;
    return explicit_multiple_dropin(Xfull, nullptr, user_bias, nullptr, nullptr, m, U, m_u, p, NA_as_zero_U, false, nonneg, U_row, U_col, U_sp, nnz_U,
                                    U_csr_p, U_csr_i, U_csr, Ub, m_ubin, pbin, C, Cb, glob_mean, biasB, U_colmeans, nullptr, nullptr, nullptr, 0,
                                    nullptr, nullptr, nullptr, Xfull, n, weight, B, Bi, add_implicit_features, k, k_user, k_item, k_main, lam,
                                    lam_unique, l1_lam, l1_lam_unique, scale_lam, scale_lam_sideinfo, scale_bias_const, scaling_biasA, w_main,
                                    w_user, w_implicit, n_max, include_all_X, BtB, TransBtBinvBt, nullptr, BeTBeChol, BiTBi, TransCtCinvCt,
                                    CtCw, CtUbias, B_plus_bias, nthreads);
}


}  // extern "C"

namespace {

// factors_collective_implicit_multiple and predict_X_new_collective_implicit (that call followed by
// predict_X_old_collective_implicit, collective.c:12024-12059): pairs null: the factors
int_t implicit_multiple_dropin(
    const PredictPairs *pairs,
    real_t *A, int_t m,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *B, int_t n,
    real_t *C,
    real_t *U_colmeans,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t l1_lam, real_t alpha, real_t w_main, real_t w_user,
    real_t w_main_multiplier,
    bool apply_log_transf,
    real_t *BeTBe, real_t *BtB, real_t *BeTBeChol, real_t *CtUbias,
    int nthreads)
{
    // a precomputed BeTBeChol without BtB means the caller's BtB is unknown: rebuild (equal for consistent inputs)
    (void)BeTBe; (void)BeTBeChol; (void)CtUbias; (void)nthreads;
    if (NA_as_zero_U) return unsupported_multiple("NA_as_zero");
    const bool spU = (U == nullptr && (nnz_U || U_csr_p));
    if (U == nullptr && !spU) m_u = 0;
    const bool side = U != nullptr || spU;
    cmfrec_hip_newrows_model mdl;
    memset(&mdl, 0, sizeof mdl);
    mdl.implicit = 1;
    mdl.n = n; mdl.n_max = n; mdl.p = side ? p : 0;
    mdl.k = k; mdl.k_user = k_user; mdl.k_item = k_item; mdl.k_main = k_main;
    mdl.nonneg = nonneg; mdl.apply_log_transf = apply_log_transf;
    mdl.lam = lam; mdl.l1_lam = l1_lam; mdl.scaling_biasA = 1; mdl.w_main = w_main; mdl.w_user = w_user; mdl.w_implicit = 1;
    mdl.alpha = alpha; mdl.w_main_multiplier = w_main_multiplier;
    mdl.B = B; mdl.C = side ? C : nullptr; mdl.U_colmeans = U_colmeans; mdl.BtB = BtB;
    // the model-side refusals come first, as they always have; then a batch without rows is no work
    {
        cmfhip::NewRowsModelArgs M;
        int_t ns = 0;
        if (int mrc = newrows_model_side(mdl, M, &ns)) return mrc;
    }
    if (std::max(m, m_u) <= 0 && !pairs) return 0;                              // rows out: max(m, m_u), collective.c:11210
    cmfrec_hip_newrows_batch bt;
    memset(&bt, 0, sizeof bt);
    bt.m = m; bt.m_u = m_u; bt.U = U;
    bt.U_row = U_row; bt.U_col = U_col; bt.U_sp = U_sp; bt.nnz_U = nnz_U; bt.U_csr_p = U_csr_p; bt.U_csr_i = U_csr_i; bt.U_csr = U_csr;
    bt.X = X; bt.ixA = ixA; bt.ixB = ixB; bt.nnz = nnz; bt.Xcsr_p = Xcsr_p; bt.Xcsr_i = Xcsr_i; bt.Xcsr = Xcsr;
    cmfrec_hip_newrows *h = cmfrec_hip_newrows_create(&mdl, -1);
    if (h == nullptr) {
        const int ec = cmfrec_hip_last_error_code();
        return ec > 3 ? 1 : (ec ? ec : 1);
    }
    bool empty = false;
    const int rc = pairs ? cmfrec_hip_newrows_predict(h, &bt, pairs->row, pairs->col, pairs->n, pairs->out, A, nullptr)
                         : newrows_solve(h, &bt, A, nullptr, &empty);
    cmfrec_hip_newrows_destroy(h);
    return rc > 3 ? 1 : rc;
}

}  // namespace

extern "C" {

int_t factors_collective_implicit_multiple(
    real_t *A, int_t m,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *B, int_t n,
    real_t *C,
    real_t *U_colmeans,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t l1_lam, real_t alpha, real_t w_main, real_t w_user,
    real_t w_main_multiplier,
    bool apply_log_transf,
    real_t *BeTBe, real_t *BtB, real_t *BeTBeChol, real_t *CtUbias,
    int nthreads)
{
    return implicit_multiple_dropin(nullptr, A, m, U, m_u, p, NA_as_zero_U, nonneg, U_row, U_col, U_sp, nnz_U, U_csr_p, U_csr_i, U_csr, X, ixA, ixB,
                                    nnz, Xcsr_p, Xcsr_i, Xcsr, B, n, C, U_colmeans, k, k_user, k_item, k_main, lam, l1_lam, alpha, w_main, w_user,
                                    w_main_multiplier, apply_log_transf, BeTBe, BtB, BeTBeChol, CtUbias, nthreads);
}

// predict_X_new_collective_explicit / _implicit, reference src/cmfrec.h (bodies src/collective.c:11861-12069): the factors of the
// batch's rows, then the chosen pairs from them -- here without the factors leaving the device.  row indexes the batch's rows
// [0, max(m_new, m_u)).  The argument mapping, the refusals and their messages are those of factors_collective_*_multiple.
int_t predict_X_new_collective_explicit(
    int_t m_new,
    int_t row[], int_t col[], real_t *predicted, size_t n_predict,
    int nthreads,
    bool user_bias,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U, bool NA_as_zero_X,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *Ub, int_t m_ubin, int_t pbin,
    real_t *C, real_t *Cb,
    real_t glob_mean, real_t *biasB,
    real_t *U_colmeans,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *Xfull, int_t n,
    real_t *weight,
    real_t *B,
    real_t *Bi, bool add_implicit_features,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t *lam_unique,
    real_t l1_lam, real_t *l1_lam_unique,
    bool scale_lam, bool scale_lam_sideinfo,
    bool scale_bias_const, real_t scaling_biasA,
    real_t w_main, real_t w_user, real_t w_implicit,
    int_t n_max, bool include_all_X,
    real_t *BtB,
    real_t *TransBtBinvBt,
    real_t *BtXbias,
    real_t *BeTBeChol,
    real_t *BiTBi,
    real_t *TransCtCinvCt,
    real_t *CtCw,
    real_t *CtUbias,
    real_t *B_plus_bias)
{
    const PredictPairs pairs = {row, col, n_predict, predicted};
    return explicit_multiple_dropin(nullptr, &pairs, user_bias, nullptr, nullptr, m_new, U, m_u, p, NA_as_zero_U, NA_as_zero_X, nonneg, U_row, U_col,
                                    U_sp, nnz_U, U_csr_p, U_csr_i, U_csr, Ub, m_ubin, pbin, C, Cb, glob_mean, biasB, U_colmeans, X, ixA, ixB, nnz,
                                    Xcsr_p, Xcsr_i, Xcsr, Xfull, n, weight, B, Bi, add_implicit_features, k, k_user, k_item, k_main, lam,
                                    lam_unique, l1_lam, l1_lam_unique, scale_lam, scale_lam_sideinfo, scale_bias_const, scaling_biasA, w_main,
                                    w_user, w_implicit, n_max, include_all_X, BtB, TransBtBinvBt, BtXbias, BeTBeChol, BiTBi, TransCtCinvCt,
                                    CtCw, CtUbias, B_plus_bias, nthreads);
}

int_t predict_X_new_collective_implicit(
    int_t m_new,
    int_t row[], int_t col[], real_t *predicted, size_t n_predict,
    int nthreads,
    real_t *U, int_t m_u, int_t p,
    bool NA_as_zero_U,
    bool nonneg,
    int_t U_row[], int_t U_col[], real_t *U_sp, size_t nnz_U,
    size_t U_csr_p[], int_t U_csr_i[], real_t *U_csr,
    real_t *X, int_t ixA[], int_t ixB[], size_t nnz,
    size_t *Xcsr_p, int_t *Xcsr_i, real_t *Xcsr,
    real_t *B, int_t n,
    real_t *C,
    real_t *U_colmeans,
    int_t k, int_t k_user, int_t k_item, int_t k_main,
    real_t lam, real_t l1_lam, real_t alpha, real_t w_main, real_t w_user,
    real_t w_main_multiplier,
    bool apply_log_transf,
    real_t *BeTBe,
    real_t *BtB,
    real_t *BeTBeChol,
    real_t *CtUbias)
{
    const PredictPairs pairs = {row, col, n_predict, predicted};
    return implicit_multiple_dropin(&pairs, nullptr, m_new, U, m_u, p, NA_as_zero_U, nonneg, U_row, U_col, U_sp, nnz_U, U_csr_p, U_csr_i, U_csr, X,
                                    ixA, ixB, nnz, Xcsr_p, Xcsr_i, Xcsr, B, n, C, U_colmeans, k, k_user, k_item, k_main, lam, l1_lam, alpha,
                                    w_main, w_user, w_main_multiplier, apply_log_transf, BeTBe, BtB, BeTBeChol, CtUbias, nthreads);
}

}  // extern "C"
