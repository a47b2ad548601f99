// device_base.hpp -- what every translation unit with C entry points shares: the error state and return codes, the run-time
// switches, a device buffer.  No kernels: a unit that includes only this compiles none but its own.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <new>
#include <string>

#include "../../include/cmfrec_hip.h"

namespace cmfhip {

extern thread_local std::string g_last_error;
extern thread_local int g_last_rc;     // return code that goes with g_last_error where the entry point returns a pointer

struct HipError {
    int code;       // C-ABI return code: 1 OOM, 4 HIP failure
};

inline void hip_check(hipError_t e, const char *what, const char *file, int line)
{
    if (e == hipSuccess) return;
    char buf[512];
    snprintf(buf, sizeof buf, "cmfrec_hip: %s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    g_last_error = buf;
    fprintf(stderr, "%s\n", buf);
    throw HipError{e == hipErrorOutOfMemory ? 1 : 4};
}
#define HIP_CHECK(x) ::cmfhip::hip_check((x), #x, __FILE__, __LINE__)

// body of a C entry point: HIP failures and bad_alloc become the ABI's return codes
inline int guarded(const std::function<int()> &f)
{
    try {
        return f();
    } catch (const HipError &e) {
        return e.code;
    } catch (const std::bad_alloc &) {
        g_last_error = "cmfrec_hip: host out of memory";
        return 1;
    }
}

// Run-time switches: the CMFREC_HIP_* environment variables are read ONCE PER SESSION -- when a session is
// created (every level-1 / level-2 entry point creates its own) or when cmfrec_hip_reload_switches() is called -- into this
// process-wide struct, instead of a getenv per launch path.  Each is an A/B switch or an on-device cross-check (another kernel
// for the same row systems, exercised by tests/test_gpu_switches.py and the tests that name it), a test hook, or a deployment
// setting (devices, exchange, size limit); none selects another model.
struct Switches {
    bool poison_lds = false;        // CMFREC_HIP_POISON_LDS: NaN patterns in LDS and fresh buffers in front of the launches (test hook)
    int vh_min = 0;                 // CMFREC_HIP_VH_MIN: where the split rows begin (0: by precision and path)
    int vh = 0;                     // CMFREC_HIP_VH: split rows 1 = stream (launch pair per CG pass), 2 = gram (one gather, CG on the row's Gramian); 0: by shape
    bool gram_slice = false;        // CMFREC_HIP_GRAM_KERNEL=slice: LDS-staged workgroup kernel for the slice partials
    int bins_par = 2;               // CMFREC_HIP_BINS_PAR: streams the nnz bins of a half-step are spread over (1: in line)
    bool nt_split = true;           // CMFREC_HIP_NT_SPLIT=0: a double-precision length bin as one launch instead of two by tile size
    int two_tiles = 1;              // CMFREC_HIP_TWO_TILES: double-precision rows of 65..96 / 257..384 entries on one / four wavefronts with two resident tiles each (1); 0 = on two- / eight-wave teams with one tile per wavefront (as before), 2 / 3 = only the first / the second range moves
    bool cg_generic = false;        // CMFREC_HIP_CG_KERNEL=generic: lane <-> unknown CG kernel everywhere
    int chol = 0;                   // CMFREC_HIP_CHOL: 1 = rows (workgroup-per-row kernel only), 2 = noslices
    int parts_coop = 1;             // CMFREC_HIP_PARTS_COOP: the rank-k update of those rows with ONE gather shared by the row's two wavefronts through LDS (chol_parts_coop_kernels.hpp; 3: three steps in flight instead of four); 0 = each wavefront gathers for itself (round 5)
    int chol_wg = 2;                // CMFREC_HIP_CHOL_WG: eight-block rows in double precision factorised by a workgroup of 2 (default) / 4 wavefronts per row (chol_wg_kernels.hpp); 0 = one wavefront per row (rounds 2-5)
    int gramk = -1;                 // CMFREC_HIP_GRAMK: 0 / 1 force the producer / consumer pair off / on (-1: by width)
    int gramk_batch = 0;            // CMFREC_HIP_GRAMK_BATCH: work items per batch (test hook: several batches on a small problem)
    int lowrank = -1;               // CMFREC_HIP_LOWRANK: 0 / 1 force the low-rank row kernel off / on (-1: by shape)
    bool topn_wide = false;         // CMFREC_HIP_TOPN=wide: the MFMA ranking kernel (topn_wide_kernels.hpp) for every k, not only beyond 64 (cross-check, A/B)
    int topn_tiles = 0;             // CMFREC_HIP_TOPN_TILES: user tiles per workgroup of that kernel, 1..4 (test hook; 0: by shape)
    int topn_cand_waves = 0;        // CMFREC_HIP_TOPN_CAND_WAVES: at most that many wavefronts (rounded up to whole workgroups) in a launch of the candidate-list ranking kernel (topn_cand_kernels.hpp), so that a small batch gives a wavefront several users (test hook; 0: by occupancy)
    int rank_slice = 0;             // CMFREC_HIP_RANK_SLICE: held-out items per user and pass of the rank kernel (topn_rank_kernels.hpp); test hook; 0: by what fits the LDS
    bool eig_jacobi = false;        // CMFREC_HIP_EIG=jacobi: the one-workgroup Jacobi kernel instead of tridiagonalisation + QL (cross-check)
    int debug_skip = 0;             // CMFREC_HIP_CG_SKIP / _CHOL_SKIP / _WAVE_SKIP (timing builds only: -DCMF_CG_DEBUG / -DCMF_CHOL_DEBUG)
    bool debug_ticks = false;       // CMFREC_HIP_GRAM_TICKS / _CHOL_TICKS (timing builds only)
    int cg_teams = 0;               // CMFREC_HIP_CG_TEAMS: at most that many teams (rounded up to whole workgroups) in a launch of the dynamically scheduled CG row kernels, so that a small problem gives a team several rows (test hook; 0: by occupancy)
    int newrows_block_rows = 0;     // CMFREC_HIP_NEWROWS_BLOCK_ROWS: rows per device block of a dense batch of new rows (test hook; 0: by the 1 GB budget)
    int predict_block = 0;          // CMFREC_HIP_PREDICT_BLOCK: pairs per upload / launch / download block of the pair scorer (test hook; 0: 2^24)
    int naz_waves = 0;              // CMFREC_HIP_NAZ_WAVES: at most that many wavefronts (rounded up to whole workgroups) in a launch of the NA_as_zero right-hand-side kernel of new rows (newrows_naz_kernels.hpp), so that one wavefront takes many rows in turn (test hook; 0: by occupancy)
    void reload()
    {
        auto str = [](const char *n) -> const char * { const char *v = getenv(n); return (v != nullptr && v[0] != 0) ? v : nullptr; };
        auto num = [&](const char *n, int dflt) -> int { const char *v = str(n); return v ? atoi(v) : dflt; };
        poison_lds = str("CMFREC_HIP_POISON_LDS") != nullptr;
        vh_min = num("CMFREC_HIP_VH_MIN", 0);
        const char *v = str("CMFREC_HIP_VH");
        vh = !v ? 0 : strcmp(v, "stream") == 0 ? 1 : strcmp(v, "gram") == 0 ? 2 : 1;       // (any other value streams, as before)
        v = str("CMFREC_HIP_GRAM_KERNEL"); gram_slice = v && strcmp(v, "slice") == 0;
        bins_par = num("CMFREC_HIP_BINS_PAR", 2);
        nt_split = num("CMFREC_HIP_NT_SPLIT", 1) != 0;
        two_tiles = num("CMFREC_HIP_TWO_TILES", 1);
        v = str("CMFREC_HIP_CG_KERNEL"); cg_generic = v && strcmp(v, "generic") == 0;
        v = str("CMFREC_HIP_CHOL"); chol = !v ? 0 : strcmp(v, "rows") == 0 ? 1 : strcmp(v, "noslices") == 0 ? 2 : 0;
        parts_coop = num("CMFREC_HIP_PARTS_COOP", 1);
        chol_wg = num("CMFREC_HIP_CHOL_WG", 2);
        if (chol_wg == 1) chol_wg = 2;
        gramk = num("CMFREC_HIP_GRAMK", -1);
        gramk_batch = num("CMFREC_HIP_GRAMK_BATCH", 0);
        lowrank = num("CMFREC_HIP_LOWRANK", -1);
        v = str("CMFREC_HIP_TOPN"); topn_wide = v && strcmp(v, "wide") == 0;
        topn_tiles = num("CMFREC_HIP_TOPN_TILES", 0);
        topn_cand_waves = num("CMFREC_HIP_TOPN_CAND_WAVES", 0);
        rank_slice = num("CMFREC_HIP_RANK_SLICE", 0);
        v = str("CMFREC_HIP_EIG"); eig_jacobi = v && strcmp(v, "jacobi") == 0;
        debug_skip = num("CMFREC_HIP_CG_SKIP", num("CMFREC_HIP_CHOL_SKIP", num("CMFREC_HIP_WAVE_SKIP", 0)));
        debug_ticks = str("CMFREC_HIP_GRAM_TICKS") != nullptr || str("CMFREC_HIP_CHOL_TICKS") != nullptr;
        cg_teams = num("CMFREC_HIP_CG_TEAMS", 0);
        newrows_block_rows = num("CMFREC_HIP_NEWROWS_BLOCK_ROWS", 0);
        predict_block = num("CMFREC_HIP_PREDICT_BLOCK", 0);
        naz_waves = num("CMFREC_HIP_NAZ_WAVES", 0);
    }
};
inline Switches &switches_mut() { static Switches sw; static bool first = (sw.reload(), true); (void)first; return sw; }
inline const Switches &switches() { return switches_mut(); }

template <typename T>
struct DevBuf {
    T *ptr = nullptr;
    size_t n = 0;
    bool owned = true;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release()
    {
        if (ptr && owned) (void)hipFree(ptr);
        ptr = nullptr;
        n = 0;
    }
    void alloc(size_t count)
    {
        release();
        n = count;
        owned = true;
        if (count) HIP_CHECK(hipMalloc((void **)&ptr, count * sizeof(T)));
        if (count && switches().poison_lds) {          // test hook (poison_lds below): device buffers too
            HIP_CHECK(hipMemset(ptr, 0xFF, count * sizeof(T)));
            HIP_CHECK(hipDeviceSynchronize());
        }
    }
    void alloc_at_least(size_t count)
    {
        if (n < count) alloc(count);
    }
    void upload(const T *host, size_t count, hipStream_t st)
    {
        if (count > n) alloc(count);
        // (hipMemcpyDefault: the source may also be device memory -- side information generated shard-wise in HBM, bench.py)
        if (count) HIP_CHECK(hipMemcpyAsync(ptr, host, count * sizeof(T), hipMemcpyDefault, st));
    }
    void download(T *host, size_t count, hipStream_t st) const
    {
        if (count) HIP_CHECK(hipMemcpyAsync(host, ptr, count * sizeof(T), hipMemcpyDeviceToHost, st));
    }
};

// rows x cols values from a host (or device) matrix with leading dimension ld into a device matrix with leading dimension dld
inline void upload_columns(real_t *dst, size_t dld, const real_t *src, size_t ld, size_t rows, size_t cols, hipStream_t st)
{
    if (ld == cols && dld == cols) HIP_CHECK(hipMemcpyAsync(dst, src, rows * cols * sizeof(real_t), hipMemcpyDefault, st));
    else HIP_CHECK(hipMemcpy2DAsync(dst, dld * sizeof(real_t), src, ld * sizeof(real_t), cols * sizeof(real_t), rows, hipMemcpyDefault, st));
}

// the calling thread's current device while a handle made on another one is used
struct DeviceScope {
    int prev = -1;
    explicit DeviceScope(int device)
    {
        int cur = -1;
        HIP_CHECK(hipGetDevice(&cur));
        if (cur != device) { HIP_CHECK(hipSetDevice(device)); prev = cur; }
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// reloads the switches, selects `device` (< 0: the current one), reports it and its CU count, creates a stream (session.hip)
void open_device(int device, int *device_id, int *num_cus, hipStream_t *stream);

}  // namespace cmfhip
