// fft_plans.h -- the hipFFT plans and 3D transforms that reconstruct.hip makes
// and caches, shared with refresh.hip (the next round's projectee runs an
// inverse transform at box N and, on its fallback path, a forward transform
// at box pf N with the very plans the reconstruction of that box made).
// Defined in reconstruct.hip.
#pragma once
#include <hipfft/hipfft.h>

#include <mutex>

#include "common.h"

#define THX_FFT(call)                                                          \
    do {                                                                       \
        hipfftResult r_ = (call);                                              \
        if (r_ != HIPFFT_SUCCESS) {                                            \
            ::thx::set_error("%s:%d %s: hipfft error %d", __FILE__, __LINE__, \
                             #call, (int)r_);                                  \
            return THX_ERR_HIP;                                                \
        }                                                                      \
    } while (0)

namespace thx {

struct Plans {
    hipfftHandle c2r = 0, r2c = 0, r2cN = 0;
    hipfftHandle c2rX = 0, r2cX = 0;     // 1D batched along x (the column-pass transforms)
    float2* tw = nullptr;                // vdim twiddles exp(-2 pi i k / vdim)
    bool cols = false;                   // the column-pass transforms are available
    size_t work = 0;
};

// Plans per (device, vdim, N, stream), made once: creating a 512^3 hipFFT
// plan costs hundreds of ms, the transforms themselves ~0.6 ms.  A plan binds
// one stream and work area, so every stream has its own; calls on one stream
// take its entry's mutex (host threads sharing a stream), calls on different
// streams -- the two hemispheres, several GPUs -- run concurrently.  The
// cache's own mutex covers only the lookup.
struct PlanEntry {
    std::mutex mu;
    Plans p;
    bool made = false;
    unsigned* bits = nullptr;   // pinned host word: the balancing loop's read-back
};

// the entry for (current device, vdim, N, s), its plans made; returned locked
int cached_plans(int vdim, int N, hipStream_t s, PlanEntry** out, std::unique_lock<std::mutex>& lock);

// every plan of p that exists <- this work area (at least p.work bytes) and stream
int bind_plans(const Plans& p, void* work, hipStream_t s);

// The 3D C2R / R2C of box vdim with p's plans (method as thx_fft3d's); the
// caller has bound their work area and stream.  C is overwritten either way.
int c2r3d(const Plans& p, float2* C, float* rl, int vdim, hipStream_t s, int method = 0);
int r2c3d(const Plans& p, float* rl, float2* C, int vdim, hipStream_t s, int method = 0);

// batched 2D transforms of nK images of box vdim (hipFFT owns their work area)
struct Plans2 {
    hipfftHandle c2r = 0, r2c = 0;
};

// the plans for (current device, vdim, nK, s), bound to s; returned locked
int plans2d(int vdim, int nK, hipStream_t s, Plans2** out, std::unique_lock<std::mutex>& lock);

}  // namespace thx
