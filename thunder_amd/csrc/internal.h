// internal.h -- the thx:: functions one .hip defines and another calls.  The
// definer includes this header too, so a signature that drifts is a compile
// error; default arguments live here only.
#pragma once

#include "common.h"

namespace thx {

// ---- scan_mfma.hip: the FP32-MFMA global scan (algo 1)
int scan_mfma(const float* rotP, int nR, const float* traP, int nT, const float* dat,
              const float* ctf, const float* sigRcp, int nImg, int nPxl, const double* pR,
              const double* pT, int kIdx, int nK, float* wC, float* wR, float* wT,
              float* baseL, void* workspace, size_t wsBytes, hipStream_t stream);
size_t scan_mfma_workspace(int nImg, int nR, int nT, int nPxl);

// ---- scan_split.hip: the split-bf16 global scans (algo 2, 4)
int scan_split_algo(int algo, const float* rotP, int nR, const float* traP, int nT,
                    const float* dat, const float* ctf, const float* sigRcp, int nImg, int nPxl,
                    const double* pR, const double* pT, int kIdx, int nK, float* wC, float* wR,
                    float* wT, float* baseL, float guard, float* dvpOut, void* workspace,
                    size_t wsBytes, hipStream_t s);
size_t scan_split_workspace(int nImg, int nR, int nT, int nPxl);
float scan_guard_default();

// ---- local.hip: the 3D phase and what the driver needs around it
int launch_local_weights(const float* dvp, int nR, int nT, const double* pC, const double* pR,
                         const double* pT, float* wC, float* wR, float* wT, float* baseL, int nImg,
                         hipStream_t s, const int* act, const int* nAct);
int launch_local_weights_d(const float* dvp, int nR, int nT, int nD, const double* pC,
                           const double* pR, const double* pT, const double* pD, float* wC,
                           float* wR, float* wT, float* wD, float* baseL, int nImg, hipStream_t s,
                           const int* act, const int* nAct);
// One 3D phase, as the C-ABI entry points and the expectation driver describe it.
struct LocalPhase {
    // volume in volLayout (0 half-complex, 1 cells, 2 y-pair); a routed phase's
    // y-pair copy: the whole one, or the compact ball of radius ypairR > 0
    const float *vol = nullptr, *ypair = nullptr;
    int volLayout = 0, vdim = 0, pf = 0, ypairR = 0;
    // cloud and priors.  nD = 0: no CTF search; nD >= 1: CTF search over nD
    // defocus samples (ctf = ctfD[nImg][nD][nPxl], priors pD[nImg][nD], marginal wD)
    const double *quat = nullptr, *trans = nullptr;
    int nR = 0, nT = 0, nD = 0;
    const double *pC = nullptr, *pR = nullptr, *pT = nullptr, *pD = nullptr;
    const float *dat = nullptr, *ctf = nullptr, *sigRcp = nullptr;
    int nPxl = 0, idim = 0, nImg = 0;
    // pixel set and its visiting order (pxOrder NULL: set order)
    const int *iCol = nullptr, *iRow = nullptr, *pxOrder = nullptr;
    int nOrd = 0;
    // outputs; dvp (may be NULL) receives the materialised likelihoods
    float *wC = nullptr, *wR = nullptr, *wT = nullptr, *wD = nullptr, *baseL = nullptr, *dvp = nullptr;
    const thx_local_sel* sel = nullptr;     // selection (may be NULL)
    // driver extras, all optional.  evBeg / evEnd: recorded around the phase
    // kernel; routeOut (device): the routed phase's kernel choice; routeSample =
    // {list, count}: the images the route samples instead of the active list;
    // stepPlan = {order, plan} of step_plan_build instead of one built here
    hipEvent_t evBeg = nullptr, evEnd = nullptr;
    int* routeOut = nullptr;
    const int *const *routeSample = nullptr, *const *stepPlan = nullptr;
    void* workspace = nullptr;
    size_t wsBytes = 0;
    thx_stream_t stream = nullptr;
};
int local_phase_impl(const LocalPhase& ph);
size_t local_phase_workspace_planned(int nImg, int nR, int nT, int nVisit);
size_t step_plan_ints(int nImg);
bool step_plan_build(const int* pxOrder, int nOrd, const float* dat, const float* sigRcp, int nPxl,
                     int nImg, int nD, int* cOrd, int* plan, hipStream_t s, int* status);
bool phase_routed(int volLayout, int pf, int nPxl, int nD);

// ---- optimiser.hip: calVari (floors 0) into rows {k1 k2 k3 s0 s1 .} of vari nImg x 6
int pf_calvari_vari(int nImg, int mR, const double* quat, int mT, const double* trans,
                    double* vari, hipStream_t s);

// ---- twod.hip: MODE_2D projection and phase
int project2d_launch(const float* vol, int vdim, int pf, const double* rot, int rotStride, int nR,
                     const int* iCol, const int* iRow, int nPxl, float* rotP, hipStream_t s);
int local_phase2d_launch(const float* vol, int vdim, int pf, const int* cls, const double* rot,
                         int rotStride, int nR, const double* trans, int nT, const double* pC,
                         const double* pR, const double* pT, const float* dat, const float* ctf,
                         const float* sigRcp, const int* iCol, const int* iRow, int nPxl, int idim,
                         int nImg, float* wC, float* wR, float* wT, float* baseL, float* dvp,
                         const int* done, hipStream_t s, int nD = 0, const double* pD = nullptr,
                         float* wD = nullptr, const int* act = nullptr, const int* nAct = nullptr);

// ---- symmetry.hip
int pf_symmetrise_launch(int nImg, int mR, double* quat, int anchorMode, const double* anchor,
                         const double* symQ, int nSym, uint64_t seed, uint32_t stream,
                         const int* done, hipStream_t s);

// ---- order.hip: the phases' view order
size_t view_order_tmp_bytes(int nImg);
int view_order(int nImg, int mLR, const double* quat, unsigned* keys, unsigned* keysOut, int* idx,
               int* ord, void* tmp, size_t tmpBytes, hipStream_t s);

}  // namespace thx
