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
                         hipStream_t s, const int* act = nullptr, const int* nAct = nullptr);
int launch_local_weights_d(const float* dvp, int nR, int nT, int nD, const double* pC,
                           const double* pR, const double* pT, const double* pD, float* wC,
                           float* wR, float* wT, float* wD, float* baseL, int nImg, hipStream_t s,
                           const int* act = nullptr, const int* nAct = nullptr);
// evBeg / evEnd (may be NULL): recorded around the phase kernel; dvp (may be
// NULL): receives the materialised likelihoods
int local_phase_impl(const thx_local_sel* sel, hipEvent_t evBeg, hipEvent_t evEnd,
                     const float* vol, int volLayout, int vdim, int pf, const double* quat, int nR,
                     const double* trans, int nT, const double* pC, const double* pR,
                     const double* pT, const float* dat, const float* ctf, const float* sigRcp,
                     const int* iCol, const int* iRow, const int* pxOrder, int nOrd, int nPxl,
                     int idim, int nImg, float* wC, float* wR, float* wT, float* baseL, float* dvp,
                     void* workspace, size_t wsBytes, thx_stream_t stream, int nD = 0,
                     const double* pD = nullptr, float* wD = nullptr,
                     const float* ypair = nullptr, int* routeOut = nullptr,
                     const int* const* routeSample = nullptr, int ypairR = 0,
                     const int* const* stepPlan = nullptr);
size_t local_phase_workspace_planned(int nImg, int nR, int nT, int nVisit);
size_t step_plan_ints(int nImg);
bool step_plan_build(const int* pxOrder, int nOrd, const float* dat, const float* sigRcp, int nPxl,
                     int nImg, int nD, int* cOrd, int* plan, hipStream_t s, int* status);
bool phase_routed(int volLayout, int pf, int nPxl, int nD);

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
