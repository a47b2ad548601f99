// topn_filter.hpp -- what topn_tu.hip needs of the half-precision filter (topn_filter_kernels.hpp): the
// image of a ranker's item factors and the launches.  The kernels are instantiated in topn_filter_tu.hip only.
#pragma once
#include "device_base.hpp"
#include "topn_filter_kernels.hpp"

namespace cmfhip {

struct TopnFilterImage {
    DevBuf<_Float16> Bh;                     // [n][topnf_kh(k)]
    DevBuf<float> nb, db;                    // [n]
    DevBuf<unsigned> mx;                     // [2] float bits of the largest |B| and |bias|
    int sb = 0;
    bool ready = false;                      // built for the ranker's current factors
    bool usable = false;                     // ... and they were finite and in range: the filter may run
    float build_ms = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    void release()
    {
        Bh.release(); nb.release(); db.release(); mx.release();
        ready = usable = false;
    }
    ~TopnFilterImage()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

// Builds the image of dB [n, ldb] (device, columns [0, k)) and checks dbias [n] (device, or null) on st; waits for it.  A matrix
// with a non-finite entry or one of 2^41 and more, or such a bias, gets no image: img.usable stays false.
void topn_filter_build_image(hipStream_t st, int num_cus, const real_t *dB, size_t ldb, int n, int k, const real_t *dbias, TopnFilterImage &img);

// User tiles per workgroup (1, 2, 4 or 8) by what fits the LDS, as pick_user_tiles chooses for the exact kernel; forced > 0
// (CMFREC_HIP_TOPN_TILES) asks for at most that many.
int topn_filter_pick_tiles(int nu, int k, int m, int num_cus, int forced, int *blocks_per_cu);

// topn_filter_kernel over P.nu users; returns the grid, *users_per_wg = 16 * tiles
int topn_filter_launch(hipStream_t st, int num_cus, const TopnFilterParams<real_t> &P, int forced_tiles, int *users_per_wg);
// topn_filter_keys_kernel: P.keys [nu][n] <- every key
void topn_filter_launch_keys(hipStream_t st, int num_cus, const TopnFilterParams<real_t> &P);
// topn_filter_refine_kernel over P.nu shortlists; wide: the MFMA kernel's arithmetic, else the register-resident kernel's (k <= 64)
void topn_filter_refine(hipStream_t st, int num_cus, const TopnRefineParams<real_t> &P, bool wide);
void topn_filter_certify(hipStream_t st, const real_t *scores, int nu, int n_top, const float *tau, const int *state, int *certified);

}  // namespace cmfhip
