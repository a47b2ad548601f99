// launch.hpp -- what session.hip needs from the launch layer, and what the launch units need from each other: the
// descriptions of a launch and the launchers' declarations, no kernels.  The definitions -- and with them every instantiation
// of the row-solver, GEMM and Gramian kernels -- are in the launch units:
//   launch_cg.hip         launch_cg, launch_cg_wide, launch_cg_any, poison_lds, cg_ticks_buffer
//   launch_chol.hip       launch_chol (wave-per-row kernels, gramk pair, the wide Gramian-CG second kernel), launch_chol_rows
//   launch_lowrank.hip    issue_eig, launch_collective_lowrank, launch_plain_lowrank
//   launch_dense.hip      launch_gemm, launch_gram, launch_trtri, launch_potrs_rows
// (side_times / side_transposed_times, beside the preprocessing kernels they launch, and open_device / init_device are session.hip's.)
// One definition each, so the function-local state of the launchers (occupancy tables, attribute flags, tick buffers) exists
// once per library.
#pragma once
#include "device.hpp"

namespace cmfhip {

struct SideZeros;                           // side_zeros_kernels.hpp
template <typename T> struct CholSlices;    // chol_wave_kernels.hpp

// ---- dense layer (launch_dense.hip) --------------------------------------------------------
// C[M, N] = alpha * op(A) B, all row-major
template <bool TRANSA>
void launch_gemm(const DeviceInfo &dev, int M, int N, int K, real_t alpha, const real_t *A, size_t lda, const real_t *B, size_t ldb,
                 real_t *C, size_t ldc);
extern template void launch_gemm<false>(const DeviceInfo &, int, int, int, real_t, const real_t *, size_t, const real_t *, size_t, real_t *, size_t);
extern template void launch_gemm<true>(const DeviceInfo &, int, int, int, real_t, const real_t *, size_t, const real_t *, size_t, real_t *, size_t);
// out[k,k] = scale * B[:, :k]^T B[:, :k] + add_diag * I
void launch_gram(const DeviceInfo &dev, GramWorkspace &ws, const real_t *B, size_t ldb, int n, int k, real_t *out, real_t scale,
                 real_t add_diag);
void launch_trtri(const DeviceInfo &dev, const real_t *R, int k, real_t *Linv);
void launch_potrs_rows(const DeviceInfo &dev, int rows, int k, const real_t *R, real_t *X, size_t ldx);
void init_device(DeviceInfo &dev, int device);             // session.hip (open_device: device_base.hpp)

// ---- CG row updates (launch_cg.hip) --------------------------------------------------------
void poison_lds(hipStream_t st, int num_cus);              // test hook (CMFREC_HIP_POISON_LDS=1) in front of the row kernels' launches
int launch_cg(const DeviceInfo &dev, const CgCall &c, const SparseShard &X, BinTimers *tm = nullptr);
int launch_cg_wide(const DeviceInfo &dev, const CgCall &c, const SparseShard &X);
int launch_cg_any(const DeviceInfo &dev, const CgCall &c, const SparseShard &X, BinTimers *tm = nullptr);
#ifdef CMF_CG_TICKS
unsigned long long *cg_ticks_buffer();
#endif
// (gram_wave_tu.hip)
void launch_gram_wave(dim3 grid, hipStream_t st, const CgParams<real_t> &P, const GramParams<real_t> &G, bool implicit, int rem);

// ---- closed-form row updates (launch_chol.hip, launch_lowrank.hip) --------------------------
// (chol_wg_tu.hip: the four-wavefront factorisation of the eight-block rows, double precision)
hipError_t launch_chol_wg8(int num_cus, bool border, int waves_per_row, hipStream_t st, const CholParams<real_t> &W, const RowDesc *desc, const CholSlices<real_t> &SL);
hipError_t launch_chol_parts_coop(int num_cus, bool border, int depth, hipStream_t st, const CholParams<real_t> &W, const RowDesc *desc, const CholSlices<real_t> &SL);

struct CholCall {
    real_t *A; size_t lda;
    const real_t *B; size_t ldb;
    int kt, koff;
    const real_t *bias_sub;
    const real_t *Minit; int kc; int rows_with_u; int p_side;
    real_t lam, lam_last;
    bool scale_lam, scale_lam_sideinfo, scale_bias_const;
    int mode;
    const real_t *Mfull = nullptr;
    // second gather source (sparse side information): rows of B2[*, ldb2] selected by X2's entries, unknowns [0, kc2)
    const SparseShard *X2 = nullptr;
    const real_t *B2 = nullptr;
    size_t ldb2 = 0;
    int kc2 = 0;
    real_t w2 = 0;
    // non-negative factors: coordinate descent on the assembled system instead of the Cholesky solve
    bool nonneg = false;
    int max_cd_steps = 100;
    // second source placed at unknown koff2 and used for the right-hand side only (implicit-features term)
    int koff2 = 0;
    bool w2_syr_zero = false;
    int rows2 = -1;
    const real_t *values2 = nullptr;         // values of the second source (default: X2's own)
    const real_t *values_override = nullptr; // values of the first source (default: X's own)
    bool rhs_only = false;                   // CHOL_NAZ: gather the right-hand sides only
    bool rhs_prefilled_all = false;          // every row starts from the right-hand side left in A
    const real_t *weights_override = nullptr; // CHOL_NAZ_W: the entries' rank-1 weights (w - 1), CSR order of X
    bool x_rhs_only = false;                 // the entries of X add to the right-hand sides only (their Gramian is inside Mfull)
    bool entry_pairs = false;                // weights_override / values_override are the entries' rank-1 and right-hand-side weights
    const real_t *mult_override = nullptr;   // per-row lambda multipliers of the collective modes instead of the rows' lengths
    bool all_rows = false;                   // CHOL_NAZ_W: rows without entries are solved too (from the prefilled right-hand side)
    int row_limit = -1;                      // only the first row_limit positions of the processing order (the others are solved elsewhere)
    // CG on the row's Gramian instead of the factorisation (gram_cg_wide_kernels.hpp): the producer build of the wave kernel runs
    // every row's rank-k update, gram_cg_wide_kernel takes the partials; the parameters of the CG (explicit model)
    const CgParams<real_t> *cg_wide = nullptr;
};

// X may be null for CHOL_PREFILLED (then nrows_prefilled rows are solved in natural order)
int launch_chol(const DeviceInfo &dev, const CholCall &c, const SparseShard *X, int nrows_prefilled = 0);
// the workgroup-per-row kernel over the positions [P.row_first, P.nrows) of the processing order
int launch_chol_rows(const DeviceInfo &dev, const CholCall &c, const SparseShard *X, CholParams<real_t> P, bool two_src, size_t smem_nonneg);
int launch_plain_lowrank(const DeviceInfo &dev, const CholCall &c, const SparseShard &X);

// Eigenvectors / values of one side's shared matrix w C^T C (eig_kernels.hpp: tridiagonalisation + implicit QL, two launches
// of 1 and ceil(k_c / 64) workgroups -- a few milliseconds of mostly sequential work on a handful of CUs), so
//  * inside a half-step it is enqueued BEHIND the launches of the rows that do not need it (the producer / consumer batches of
//    the long rows), on the eigen stream, waiting only for an event recorded in front of them;
//  * a half-step also enqueues the decomposition the NEXT half-step of the other side will ask for (`wanted`: that side took
//    the low-rank path before), since C and D are final once their own updates have run (cmfrec's order C, D, B, A):
//    `fresh` says the cached vectors belong to the side matrix as it stands; every update / upload of C or D clears it.
// (Rounds 3-5 bound rocSOLVER's dsyevd here -- ~4000 launches per decomposition, 6 ms on an idle device and 33 ms beside the
//  persistent batches, profiles/r05/r05_zg_*; round 6 replaced it and the link against rocBLAS went with it.)
struct EigCache {
    DevBuf<double> W, V, D, E, Tau;
    DevBuf<int> info;
    DevBuf<real_t> Q, Qt, Lam, M;     // M: the matrix a prefetch decomposes (the half-step's own one lives in the session's ctc)
    hipEvent_t ev = nullptr;          // recorded behind the chain on the eigen stream
    bool fresh = false, wanted = false;
    int kind = 0;                     // 3 tridiagonalisation + QL (eig_kernels.hpp), 2 the one-workgroup Jacobi kernel
    int checked_kc = 0;               // the QL kernel's status word has been read back for this matrix size (once per size and cache)
    ~EigCache() { if (ev) (void)hipEventDestroy(ev); }
};

struct LowRankScratch {
    DevBuf<real_t> Ct, Bt, R, T;
    EigCache own;                 // callers without a cache per side (the stand-alone operator)
    int last_rows = 0;            // rows the low-rank kernels solved in the most recent launch (0: path not taken)
    int last_eig = 0;             // its eigen-decomposition: 3 tridiagonalisation + QL, 2 the one-workgroup Jacobi kernel
};

void issue_eig(DeviceInfo &d, EigCache &E, const real_t *Minit, int kc, hipEvent_t after);

// Side information as the half-steps multiply by it: the dense matrix (from the operand's first row), or the sparse matrix whose
// absent entries are zeros, centred by its column means (side_zeros_kernels.hpp).  No kernel reads U element by element: every
// use is one of the two products below, so the solvers downstream see the same operands either way.
struct SideOperand {
    const real_t *dense = nullptr;
    SideZeros *zeros = nullptr;
    int first = 0;                              // the operand's first row within `zeros`
    SideOperand from_row(int r, int p) const
    {
        SideOperand o = *this;
        if (o.dense != nullptr) o.dense += (size_t)r * p;
        o.first += r;
        return o;
    }
};
// out[count, kc] = alpha U[:count, :] M,  M [p, kc]   (session.hip)
void side_times(const DeviceInfo &dev, const SideOperand &u, int count, int kc, int p, real_t alpha, const real_t *M, real_t *out, size_t ldo);
// out[p, kc] = U[:rows, :]^T F[:rows, :kc]   (sparse-as-zeros: all its rows)
void side_transposed_times(const DeviceInfo &dev, const SideOperand &u, int rows, int kc, int p, const real_t *F, size_t ldF, real_t *out,
                           size_t ldo);

int launch_collective_lowrank(const DeviceInfo &dev, LowRankScratch &S, CholCall c, const SparseShard &X, const real_t *Cm,
                              const SideOperand &Um, int p_self, real_t w, int k, int rows_b, EigCache *mine = nullptr,
                              EigCache *next = nullptr, int kc_next = 0);

}  // namespace cmfhip
