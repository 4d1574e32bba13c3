// round.hip -- what runs between two rounds on the top particles
// (Particle::rank1st, exported by thx_expectation_rank1st):
//   thx_rank1st_diff -- Particle::diffTopR / diffTopT / diffTopD / diffTopC
//                       (src/Particle.cpp:2004-2038) of every image;
//   thx_recentre     -- Optimiser::reCentreImg (src/Optimiser.cpp:6064-6090);
//   thx_class_count  -- the numerator of refreshClassDistr (:5386-5432);
//   thx_pf_score     -- Particle::compressR / calScore (src/Particle.cpp:647-678,
//                       1144-1147), the table's score and the grading weight.
// Nothing here synchronises or allocates; every pointer is a device pointer.
#include "common.h"

namespace {

// One thread per image.  Each difference is formed without contraction, in
// the order the reference's Eigen expressions spell out, then prev <- current.
__global__ void __launch_bounds__(256) k_rank1st_diff(
    int nImg, const double* __restrict__ topQ, double* __restrict__ prevQ,
    double* __restrict__ diffR, const double* __restrict__ topT, double* __restrict__ prevT,
    double* __restrict__ diffT, const double* __restrict__ topD, double* __restrict__ prevD,
    double* __restrict__ diffD, const int* __restrict__ cls, int* __restrict__ prevCls,
    int* __restrict__ sameC)
{
#pragma clang fp contract(off)
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nImg) return;
    if (topQ) {
        double dot = 0.0;
        for (int k = 0; k < 4; k++) {
            const double q = topQ[4 * (size_t)l + k];
            dot += prevQ[4 * (size_t)l + k] * q;
            prevQ[4 * (size_t)l + k] = q;
        }
        diffR[l] = 1.0 - fabs(dot);
    }
    if (topT) {
        const double tx = topT[2 * (size_t)l], ty = topT[2 * (size_t)l + 1];
        const double dx = prevT[2 * (size_t)l] - tx, dy = prevT[2 * (size_t)l + 1] - ty;
        diffT[l] = sqrt(dx * dx + dy * dy);
        prevT[2 * (size_t)l] = tx;
        prevT[2 * (size_t)l + 1] = ty;
    }
    if (topD) {
        const double d = topD[l];
        diffD[l] = fabs(prevD[l] - d);
        prevD[l] = d;
    }
    if (cls) {
        const int c = cls[l];
        sameC[l] = prevCls[l] == c;
        prevCls[l] = c;
    }
}

// reCentreImg's per-image state, one wave per image (4 images per block).
// Every lane reads t = topTrans[l] before any value of the image is written,
// and what replaces it is t - t (setTopT(topT() - tran)), which carries the
// read: no lane can see the zero.  The image pass (k_recentre_img) runs after
// this launch and reads the updated offS only.
__global__ void __launch_bounds__(256) k_recentre_state(int nImg, double* __restrict__ topTrans,
                                                        double* __restrict__ offS, int mLT,
                                                        double* __restrict__ trans,
                                                        double* __restrict__ prevTrans)
{
    const int l = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (l >= nImg) return;
    const double tx = topTrans[2 * (size_t)l], ty = topTrans[2 * (size_t)l + 1];
    if (trans) {
        double* T = trans + (size_t)l * mLT * 2;
        for (int e = lane; e < 2 * mLT; e += 64) T[e] -= (e & 1) ? ty : tx;
    }
    if (lane == 0) {
        offS[2 * (size_t)l] -= tx;
        offS[2 * (size_t)l + 1] -= ty;
        if (prevTrans) {
            prevTrans[2 * (size_t)l] -= tx;
            prevTrans[2 * (size_t)l + 1] -= ty;
        }
        topTrans[2 * (size_t)l] = tx - tx;
        topTrans[2 * (size_t)l + 1] = ty - ty;
    }
}

// imgFT[l] = oriFT[l] exp(-2 pi i (i rCol + j rRow)) on the whole stored
// half-plane [idim][idim/2+1] (translate(Image&, const Image&, ...), src/
// Image/ImageFunctions.cpp:269-284; IMAGE_FOR_EACH_PIXEL_FT: j in [-idim/2,
// idim/2), i in [0, idim/2]), rCol / rRow = the RFLOAT offset over idim.
// A streaming pass: block (x = image, y = chunk of RC_PER_BLOCK pixels), the
// lanes of a wave on consecutive float2 of the image's flat storage.
constexpr int RC_UNROLL = 4;
constexpr int RC_PER_BLOCK = 256 * RC_UNROLL;

__global__ void __launch_bounds__(256) k_recentre_img(int idim, const float2* __restrict__ oriFT,
                                                      float2* __restrict__ imgFT,
                                                      const double* __restrict__ offS)
{
    const int l = blockIdx.x;
    const int nc = idim / 2 + 1, per = idim * nc;
    const float rCol = (float)offS[2 * (size_t)l] / idim;
    const float rRow = (float)offS[2 * (size_t)l + 1] / idim;
    const float2* src = oriFT + (size_t)l * per;
    float2* dst = imgFT + (size_t)l * per;
    const int q0 = blockIdx.y * RC_PER_BLOCK + threadIdx.x;
    float2 v[RC_UNROLL];
#pragma unroll
    for (int u = 0; u < RC_UNROLL; u++) {
        const int q = q0 + u * 256;
        if (q < per) v[u] = src[q];
    }
#pragma unroll
    for (int u = 0; u < RC_UNROLL; u++) {
        const int q = q0 + u * 256;
        if (q >= per) continue;
        const int jj = q / nc, i = q - jj * nc;
        const int j = jj < idim / 2 ? jj : jj - idim;
        dst[q] = cmul(v[u], phase_shift(i, j, rCol, rRow));
    }
}

__global__ void __launch_bounds__(256) k_class_count(int nImg, const int* __restrict__ cls,
                                                     int nK, double* __restrict__ count)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nImg) return;
    const int k = cls[l];
    if (k >= 0 && k < nK) atomicAdd(count + k, 1.0);
}

// compressR of every image from its row {k1 k2 k3 s0 s1 sD} of vari:
// (k1 k2 k3)^(-1/6) in 3D, 1 / k1 in MODE_2D
__global__ void __launch_bounds__(256) k_pf_score(int nImg, const double* __restrict__ vari,
                                                  int twoD, double* __restrict__ score)
{
    const int l = blockIdx.x * 256 + threadIdx.x;
    if (l >= nImg) return;
    const double* v = vari + 6 * (size_t)l;
    score[l] = twoD ? 1.0 / v[0] : pow(v[0] * v[1] * v[2], -1.0 / 6);
}

}  // namespace

extern "C" int thx_rank1st_diff(int nImg, const double* topQuat, double* prevQuat, double* diffR,
                                const double* topTrans, double* prevTrans, double* diffT,
                                const double* topD, double* prevD, double* diffD, const int* cls,
                                int* prevCls, int* sameC, thx_stream_t stream)
{
    THX_CHECK_ARG(nImg >= 0, "thx_rank1st_diff: nImg < 0");
    THX_CHECK_ARG((!topQuat == !prevQuat) && (!topQuat == !diffR),
                  "thx_rank1st_diff: topQuat, prevQuat and diffR go together");
    THX_CHECK_ARG((!topTrans == !prevTrans) && (!topTrans == !diffT),
                  "thx_rank1st_diff: topTrans, prevTrans and diffT go together");
    THX_CHECK_ARG((!topD == !prevD) && (!topD == !diffD),
                  "thx_rank1st_diff: topD, prevD and diffD go together");
    THX_CHECK_ARG((!cls == !prevCls) && (!cls == !sameC),
                  "thx_rank1st_diff: cls, prevCls and sameC go together");
    if (nImg == 0 || !(topQuat || topTrans || topD || cls)) return THX_OK;
    THX_LAUNCH(k_rank1st_diff, dim3(thx::cdiv(nImg, 256)), dim3(256), 0, thx::as_stream(stream),
               nImg, topQuat, prevQuat, diffR, topTrans, prevTrans, diffT, topD, prevD, diffD, cls,
               prevCls, sameC);
    return THX_OK;
}

extern "C" int thx_recentre(int nImg, int idim, const float* oriFT, float* imgFT, double* topTrans,
                            double* offS, int mLT, double* trans, double* prevTrans,
                            thx_stream_t stream)
{
    THX_CHECK_ARG(nImg >= 0, "thx_recentre: nImg < 0");
    THX_CHECK_ARG(!imgFT || (idim >= 2 && idim % 2 == 0 && idim <= 8192),
                  "thx_recentre: idim must be even, 2 .. 8192");
    THX_CHECK_ARG(!trans || mLT > 0, "thx_recentre: a translation cloud needs mLT > 0");
    if (nImg == 0) return THX_OK;
    THX_CHECK_ARG(topTrans && offS, "thx_recentre: null topTrans or offS");
    THX_CHECK_ARG(!imgFT || (oriFT && oriFT != imgFT),
                  "thx_recentre: imgFT needs oriFT, in a buffer of its own");
    hipStream_t s = thx::as_stream(stream);
    THX_LAUNCH(k_recentre_state, dim3(thx::cdiv(nImg, 4)), dim3(256), 0, s, nImg, topTrans, offS,
               mLT, trans, prevTrans);
    if (!imgFT) return THX_OK;
    const long per = (long)idim * (idim / 2 + 1);
    THX_LAUNCH(k_recentre_img, dim3(nImg, thx::cdiv(per, RC_PER_BLOCK)), dim3(256), 0, s, idim,
               reinterpret_cast<const float2*>(oriFT), reinterpret_cast<float2*>(imgFT), offS);
    return THX_OK;
}

extern "C" int thx_class_count(int nImg, const int* cls, int nK, double* count,
                               thx_stream_t stream)
{
    THX_CHECK_ARG(nImg >= 0 && nK > 0, "thx_class_count: nImg < 0 or nK < 1");
    if (nImg == 0) return THX_OK;
    THX_CHECK_ARG(cls && count, "thx_class_count: null argument");
    THX_LAUNCH(k_class_count, dim3(thx::cdiv(nImg, 256)), dim3(256), 0, thx::as_stream(stream),
               nImg, cls, nK, count);
    return THX_OK;
}

extern "C" int thx_pf_score(int nImg, const double* vari, int twoD, double* score,
                            thx_stream_t stream)
{
    THX_CHECK_ARG(nImg >= 0 && (twoD == 0 || twoD == 1), "thx_pf_score: nImg < 0 or twoD not 0 / 1");
    if (nImg == 0) return THX_OK;
    THX_CHECK_ARG(vari && score, "thx_pf_score: null argument");
    THX_LAUNCH(k_pf_score, dim3(thx::cdiv(nImg, 256)), dim3(256), 0, thx::as_stream(stream), nImg,
               vari, twoD, score);
    return THX_OK;
}
