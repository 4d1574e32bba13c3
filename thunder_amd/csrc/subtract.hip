// subtract.hip -- the Subtract option after the last round (Optimiser::run,
// src/Optimiser.cpp:4163-4363): the per-image loop of saveSubtract
// (:8418-8537) with the poses saveDatabase writes for it (:8295-8361), and the
// region centre it recentres on (centroid(const Volume&),
// src/Image/ImageFunctions.cpp:37-62).  3D only, as the reference (:8444-8450).
//
//   per image l and copy s in [0, nSym] (s = 0: the pose itself; s > 0:
//   symmetry element s - 1), output plane s nImg + l:
//     rotC = rotB, or R_s^T rotB in FP64 (:8478-8488)
//     P    = Projector::project(Image&, rot) (src/Projector.cpp:167-183): the
//            stored pixels with i^2 + j^2 < r^2 (so j in [-r, r), i in [0, r];
//            the pixels with rint|.| = r stay in, unlike the spectrum table),
//            FP64 rotation -> FP32 coordinate, trilinear gather; 0 elsewhere;
//            translate(P, r, t - offS) on the same disc (:456-464,
//            src/Image/ImageFunctions.cpp:322-339)
//     diff = ori - P ctf on every stored pixel (:8493-8500; CTF_ON_THE_FLY:
//            the unscaled attributes unless dF is given)
//     diff *= exp(-2 pi i (i sx + j sy) / idim), (sx, sy) = -t + offS -
//            (rotC^T centre).xy, on every stored pixel, Nyquist row and column
//            included (:8502-8510, ImageFunctions.cpp:269-284)
//   then the backward transform scaled by 1 / idim^2 (FFT::bwExecutePlan,
//   src/FFT.cpp:346-360).
//
// The pass is write-bound: (1 + nSym) planes out per plane in.  One workgroup
// per image; the copies' FP64 matrices and recentring shifts are formed once
// into LDS (64 copies at a time), every thread owns stored pixels in storage
// order (coalesced float2 loads and stores), loads its ori pixel and evaluates
// the CTF and the first phase once, then loops over the copies.  No atomics, no
// host synchronisation: bit-identical from run to run.
//
// thx_region_centroid: FP64 sums of (i, j, k) u and u in a fixed-order tree --
// a thread adds its strided voxels in index order, the xor butterfly folds a
// wave, the waves and then the blocks are added in index order by one thread.
#include "common.h"
#include "fft_plans.h"
#include "volume.h"

namespace {

constexpr int SB_THREADS = 256;
constexpr int SB_COPIES = 64;           // copies whose matrices LDS holds at a time
constexpr int SB_FFT_BATCH = 512;       // planes per batched transform
constexpr int RC_THREADS = 256;
constexpr int RC_MAX_BLOCKS = 1024;

struct Copy {
    double m[6];        // columns 0, 1 of rotC (column-major, as quat_to_mat)
    float rCol, rRow;   // the recentring shift / idim
};

// quaternion(dvec4&, const dmat33&), src/Geometry/Euler.cpp:112-123; m column-major
THX_DEV void mat_to_quat(const double* m, double* q)
{
    const double a = m[0], b = m[4], c = m[8];
    q[0] = 0.5 * sqrt(fmax(0.0, 1 + a + b + c));
    q[1] = copysign(0.5 * sqrt(fmax(0.0, 1 + a - b - c)), m[5] - m[7]);    // R(2,1) - R(1,2)
    q[2] = copysign(0.5 * sqrt(fmax(0.0, 1 - a + b - c)), m[6] - m[2]);    // R(0,2) - R(2,0)
    q[3] = copysign(0.5 * sqrt(fmax(0.0, 1 - a - b + c)), m[1] - m[3]);    // R(1,0) - R(0,1)
}

__global__ void __launch_bounds__(SB_THREADS) k_subtract(
    const float2* __restrict__ vol, int vdim, int pf, int nK, long volStride,
    const float2* __restrict__ oriFT, const float* __restrict__ attr,
    const double* __restrict__ quat, const double* __restrict__ trans,
    const double* __restrict__ offS, const double* __restrict__ dF, const int* __restrict__ cls,
    int nImg, int idim, int r, const double* __restrict__ symR, int nSym,
    const double* __restrict__ centre, float2* __restrict__ diffFT, float2* __restrict__ modelFT,
    float2* __restrict__ diffWs, double* __restrict__ quatOut, double* __restrict__ shift)
{
    __shared__ Copy sCopy[SB_COPIES];
    const size_t l = blockIdx.x;
    const int tid = threadIdx.x;
    const int nc = idim / 2 + 1;
    const int per = idim * nc;
    const size_t plane = (size_t)per;
    const int k = cls ? cls[l] : 0;
    const double tx = trans[2 * l], ty = trans[2 * l + 1];
    const double ox = offS ? offS[2 * l] : 0.0, oy = offS ? offS[2 * l + 1] : 0.0;
    if (k < 0 || k >= nK) {
        // a class outside the projectee stack: no gather, the image's outputs are NaN
        const float2 nan2 = make_float2(__builtin_nanf(""), __builtin_nanf(""));
        for (int s = 0; s <= nSym; s++) {
            const size_t o = ((size_t)s * nImg + l) * plane;
            for (int q = tid; q < per; q += SB_THREADS) {
                if (diffFT) diffFT[o + q] = nan2;
                if (modelFT) modelFT[o + q] = nan2;
                if (diffWs) diffWs[o + q] = nan2;
            }
            if (quatOut && tid < 4) quatOut[((size_t)s * nImg + l) * 4 + tid] = __builtin_nan("");
        }
        if (shift && tid < 2) shift[2 * l + tid] = __builtin_nan("");
        return;
    }
    if (shift && tid == 0) {
        shift[2 * l] = tx - ox;
        shift[2 * l + 1] = ty - oy;
    }
    const float2* P = vol + (size_t)k * volStride;
    const float2* ori = oriFT + l * plane;
    const float* A = attr + 8 * l;
    const float dU = dF ? (float)(A[2] * dF[l]) : A[2], dV = dF ? (float)(A[3] * dF[l]) : A[3];
    // translate(): RFLOAT shift / nColRL (src/Image/ImageFunctions.cpp:322-339)
    const float nCol = (float)(tx - ox) / idim, nRow = (float)(ty - oy) / idim;
    // a gather further out than this would leave the projectee (a quaternion
    // that is not a unit one): such a pixel is NaN instead
    const float lim = (float)(vdim / 2 - 1);
    const int r2 = r * r;
    for (int s0 = 0; s0 <= nSym; s0 += SB_COPIES) {
        const int ns = nSym + 1 - s0 < SB_COPIES ? nSym + 1 - s0 : SB_COPIES;
        __syncthreads();
        if (tid < ns) {
            const int s = s0 + tid;
            const double q[4] = {quat[4 * l], quat[4 * l + 1], quat[4 * l + 2], quat[4 * l + 3]};
            double rotB[9], rotC[9];
            quat_to_mat(q, rotB);
            if (s == 0) {
#pragma unroll
                for (int e = 0; e < 9; e++) rotC[e] = rotB[e];
            } else {
                // rotC = R^T rotB: rotC(a, c) = sum_k R(k, a) rotB(k, c); R row-major
                const double* R = symR + 9 * (size_t)(s - 1);
#pragma unroll
                for (int c = 0; c < 3; c++)
#pragma unroll
                    for (int a = 0; a < 3; a++)
                        rotC[c * 3 + a] = R[a] * rotB[c * 3] + R[3 + a] * rotB[c * 3 + 1] +
                                          R[6 + a] * rotB[c * 3 + 2];
            }
            Copy cp;
#pragma unroll
            for (int e = 0; e < 6; e++) cp.m[e] = rotC[e];
            // regionTrans = (rotC^T centre).xy (:8502-8504)
            double gx = 0.0, gy = 0.0;
            if (centre) {
                gx = rotC[0] * centre[0] + rotC[1] * centre[1] + rotC[2] * centre[2];
                gy = rotC[3] * centre[0] + rotC[4] * centre[1] + rotC[5] * centre[2];
            }
            cp.rCol = (float)(-tx + ox - gx) / idim;
            cp.rRow = (float)(-ty + oy - gy) / idim;
            sCopy[tid] = cp;
            if (quatOut) mat_to_quat(rotC, quatOut + ((size_t)s * nImg + l) * 4);
        }
        __syncthreads();
        for (int q = tid; q < per; q += SB_THREADS) {
            const int jj = q / nc, i = q - jj * nc;
            const int j = jj < idim / 2 ? jj : jj - idim;
            const float2 o = ori[q];
            const bool in = i * i + j * j < r2;
            float c = 0.f;
            float2 ph1 = make_float2(1.f, 0.f);
            if (in) {
                c = ctf_at(A, dU, dV, i, j, idim);
                ph1 = phase_shift(i, j, nCol, nRow);
            }
            for (int s = 0; s < ns; s++) {
                float2 M = make_float2(0.f, 0.f);
                if (in) {
                    float x, y, z;
                    rot_coord(sCopy[s].m, i, j, pf, x, y, z);
                    float2 p = make_float2(__builtin_nanf(""), __builtin_nanf(""));
                    if (fabsf(x) < lim && fabsf(y) < lim && fabsf(z) < lim)
                        p = interp_ft(P, vdim, x, y, z);
                    const float2 pm = cmul(p, ph1);
                    M = make_float2(pm.x * c, pm.y * c);
                }
                const size_t at = ((size_t)(s0 + s) * nImg + l) * plane + q;
                if (modelFT) modelFT[at] = M;
                const float2 d = cmul(make_float2(o.x - M.x, o.y - M.y),
                                      phase_shift(i, j, sCopy[s].rCol, sCopy[s].rRow));
                if (diffFT) diffFT[at] = d;
                if (diffWs) diffWs[at] = d;
            }
        }
    }
}

// FFTW's c2r, which the reference runs, reads only the Hermitian part of
// columns 0 and N/2 (the recentring phase leaves column N/2 inconsistent for a
// fractional shift); how hipFFT reads an inconsistent column is its own
// choice, so the workspace copy gets that Hermitian part written out:
// v(j) <- (v(j) + conj v(-j)) / 2, rows 0 and N/2 real
__global__ void __launch_bounds__(256) k_hermitian_cols(float2* __restrict__ ft, size_t nPlane,
                                                        int N)
{
    const int nc = N / 2 + 1;
    const size_t each = (size_t)2 * nc, tot = each * nPlane;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < tot;
         q += (size_t)gridDim.x * blockDim.x) {
        const size_t pl = q / each;
        const int e = (int)(q % each), col = e < nc ? 0 : N / 2, jj = e < nc ? e : e - nc;
        float2* img = ft + pl * (size_t)N * nc;
        const size_t a = (size_t)jj * nc + col, b = (size_t)((N - jj) % N) * nc + col;
        const float2 va = img[a], vb = img[b];
        const float2 h = make_float2((va.x + vb.x) * 0.5f, (va.y - vb.y) * 0.5f);
        img[a] = h;                     // a == b for rows 0 and N/2: the real part
        if (a != b) img[b] = make_float2(h.x, -h.y);
    }
}

// after the C2R, in place: bwExecutePlan's 1 / N^2; centred: the reference's
// corner-origin image moved to the centred layout of an MRC stack (rl_index of
// preprocess.hip; for an even box the two layouts swap pixel pairs); the
// planes of an image whose class is outside [0, nK) are NaN
__global__ void __launch_bounds__(256) k_rl_finish(float* __restrict__ rl, size_t nPlane, int nImg,
                                                   int N, int centred, float scale,
                                                   const int* __restrict__ cls, int nK)
{
    const size_t half = (size_t)N * (N / 2), tot = half * nPlane;
    for (size_t q = blockIdx.x * (size_t)blockDim.x + threadIdx.x; q < tot;
         q += (size_t)gridDim.x * blockDim.x) {
        const size_t pl = q / half, p = q % half;
        const int jj = (int)(p / N), ii = (int)(p % N);
        float* img = rl + pl * (size_t)N * N;
        const size_t a = (size_t)jj * N + ii;
        const size_t b = (size_t)(jj + N / 2) * N + (centred ? (ii + N / 2) % N : ii);
        float va = img[a] * scale, vb = img[b] * scale;
        const int k = cls ? cls[pl % nImg] : 0;
        if (k < 0 || k >= nK) va = vb = __builtin_nanf("");
        img[a] = centred ? vb : va;
        img[b] = centred ? va : vb;
    }
}

// block b sums the voxels b T + t, b T + t + G T, ... (T threads, G blocks) into
// part[4][G] = sum i u, sum j u, sum k u, sum u
__global__ void __launch_bounds__(RC_THREADS) k_centroid_partial(const float* __restrict__ map,
                                                                 int N, double* __restrict__ part)
{
    __shared__ double sh[4][RC_THREADS / 64];
    const size_t n3 = (size_t)N * N * N;
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    for (size_t q = blockIdx.x * (size_t)RC_THREADS + threadIdx.x; q < n3;
         q += (size_t)gridDim.x * RC_THREADS) {
        const int i = signed_idx((int)(q % N), N), j = signed_idx((int)(q / N % N), N);
        const int k = signed_idx((int)(q / ((size_t)N * N)), N);
        const double u = (double)map[q];
        a[0] += i * u;
        a[1] += j * u;
        a[2] += k * u;
        a[3] += u;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int e = 0; e < 4; e++) {
        a[e] = wave_sum(a[e]);
        if (lane == 0) sh[e][wv] = a[e];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        double t = 0.0;
        for (int w = 0; w < RC_THREADS / 64; w++) t += sh[threadIdx.x][w];
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = t;
    }
}

__global__ void __launch_bounds__(64) k_centroid_final(const double* __restrict__ part, int nBlock,
                                                       double* __restrict__ centre)
{
    __shared__ double sh[4];
    if (threadIdx.x < 4) {
        double t = 0.0;
        for (int b = 0; b < nBlock; b++) t += part[(size_t)threadIdx.x * nBlock + b];
        sh[threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x < 3) centre[threadIdx.x] = sh[threadIdx.x] / sh[3];
}

int centroid_blocks(int N)
{
    const long n3 = (long)N * N * N;
    const long b = (n3 + RC_THREADS * 16 - 1) / (RC_THREADS * 16);
    return (int)(b < 1 ? 1 : b > RC_MAX_BLOCKS ? RC_MAX_BLOCKS : b);
}

bool box_ok(int N) { return N > 0 && N % 2 == 0 && N <= 4096; }

}  // namespace

int thx::hermitian_cols(float2* ft, size_t nPlane, int N, hipStream_t s)
{
    const size_t nCol = nPlane * (size_t)(N + 2);
    THX_LAUNCH(k_hermitian_cols, dim3(nCol > 2048 * 256 ? 2048 : thx::cdiv((long)nCol, 256)),
               dim3(256), 0, s, ft, nPlane, N);
    return THX_OK;
}

int thx::rl_finish(float* rl, size_t nPlane, int nImg, int N, int centred, float scale,
                   const int* cls, int nK, hipStream_t s)
{
    THX_LAUNCH(k_rl_finish, dim3(2048), dim3(256), 0, s, rl, nPlane, nImg, N, centred, scale, cls,
               nK);
    return THX_OK;
}

extern "C" size_t thx_region_centroid_workspace(int N)
{
    if (!box_ok(N)) return 0;
    return (size_t)4 * centroid_blocks(N) * sizeof(double) + 256;
}

extern "C" int thx_region_centroid(const float* map, int N, double* centre, void* workspace,
                                   size_t wsBytes, thx_stream_t stream)
{
    THX_CHECK_ARG(box_ok(N), "thx_region_centroid: N=%d must be even, in [2, 4096]", N);
    THX_CHECK_ARG(map && centre && workspace, "thx_region_centroid: null argument");
    THX_CHECK_ARG(wsBytes >= thx_region_centroid_workspace(N),
                  "thx_region_centroid: workspace %zu < %zu bytes", wsBytes,
                  thx_region_centroid_workspace(N));
    const int nb = centroid_blocks(N);
    thx::Carver cv(workspace, wsBytes);
    double* part = cv.take<double>((size_t)4 * nb);
    THX_LAUNCH(k_centroid_partial, dim3(nb), dim3(RC_THREADS), 0, thx::as_stream(stream), map, N,
               part);
    THX_LAUNCH(k_centroid_final, dim3(1), dim3(64), 0, thx::as_stream(stream), part, nb, centre);
    return THX_OK;
}

extern "C" size_t thx_subtract_workspace(int nImg, int idim, int nSym, int wantRL)
{
    if (nImg < 0 || idim <= 0 || idim % 2 || nSym < 0) return 0;
    if (!wantRL) return 0;
    return (size_t)(1 + nSym) * nImg * idim * (idim / 2 + 1) * sizeof(float2) + 256;
}

extern "C" int thx_subtract(const float* vol, int vdim, int pf, int nK, const float* oriFT,
                            const float* attr, const double* quat, const double* trans,
                            const double* offS, const double* dF, const int* cls, int nImg,
                            int idim, int r, const double* symR, int nSym, const double* centre,
                            float* diffFT, float* modelFT, float* diffRL, int centred,
                            double* quatOut, double* shift, void* workspace, size_t wsBytes,
                            thx_stream_t stream)
{
    THX_CHECK_ARG(vdim > 0 && vdim % 2 == 0 && pf > 0 && nK >= 1 && nImg >= 0,
                  "thx_subtract: bad sizes");
    THX_CHECK_ARG(idim > 0 && idim % 2 == 0, "thx_subtract: idim=%d must be even", idim);
    THX_CHECK_ARG(r >= 1 && r <= idim / 2 - 1, "thx_subtract: r=%d outside [1, idim/2-1]", r);
    THX_CHECK_ARG((long)r * pf < vdim / 2 - 1, "thx_subtract: r * pf reaches the projectee's edge");
    THX_CHECK_ARG(nSym >= 0, "thx_subtract: nSym=%d is negative", nSym);
    THX_CHECK_ARG(nSym == 0 || symR, "thx_subtract: symR is NULL with nSym=%d", nSym);
    THX_CHECK_ARG(diffFT || modelFT || diffRL || quatOut || shift,
                  "thx_subtract: every output is NULL");
    THX_CHECK_ARG((long)(1 + nSym) * nImg < (1l << 31), "thx_subtract: too many output planes");
    const size_t need = thx_subtract_workspace(nImg, idim, nSym, diffRL != nullptr);
    THX_CHECK_ARG(!diffRL || (workspace && wsBytes >= need),
                  "thx_subtract: workspace %zu < %zu bytes", workspace ? wsBytes : (size_t)0, need);
    if (nImg == 0) return THX_OK;
    THX_CHECK_ARG(vol && oriFT && attr && quat && trans, "thx_subtract: null argument");
    hipStream_t s = thx::as_stream(stream);
    const size_t per = (size_t)idim * (idim / 2 + 1);
    const size_t nPlane = (size_t)(1 + nSym) * nImg;
    thx::Carver cv(workspace, wsBytes);
    float2* ws = diffRL ? cv.take<float2>(nPlane * per) : nullptr;
    const long volStride = (long)(vdim / 2 + 1) * vdim * vdim;
    THX_LAUNCH(k_subtract, dim3(nImg), dim3(SB_THREADS), 0, s,
               reinterpret_cast<const float2*>(vol), vdim, pf, nK, volStride,
               reinterpret_cast<const float2*>(oriFT), attr, quat, trans, offS, dF, cls, nImg, idim,
               r, symR, nSym, centre, reinterpret_cast<float2*>(diffFT),
               reinterpret_cast<float2*>(modelFT), ws, quatOut, shift);
    if (!diffRL) return THX_OK;
    const size_t nCol = nPlane * (size_t)(idim + 2);
    THX_LAUNCH(k_hermitian_cols, dim3(nCol > 2048 * 256 ? 2048 : thx::cdiv((long)nCol, 256)),
               dim3(256), 0, s, ws, nPlane, idim);
    for (size_t p0 = 0; p0 < nPlane; p0 += SB_FFT_BATCH) {
        const int nb = nPlane - p0 < (size_t)SB_FFT_BATCH ? (int)(nPlane - p0) : SB_FFT_BATCH;
        // the batched 2D plans reconstruct.hip caches per (device, box, batch, stream)
        thx::Plans2* pl = nullptr;
        std::unique_lock<std::mutex> lk;
        THX_RET(thx::plans2d(idim, nb, s, &pl, lk));
        THX_FFT(hipfftExecC2R(pl->c2r, reinterpret_cast<hipfftComplex*>(ws + p0 * per),
                              diffRL + p0 * (size_t)idim * idim));
    }
    THX_LAUNCH(k_rl_finish, dim3(2048), dim3(256), 0, s, diffRL, nPlane, nImg, idim, centred,
               1.f / ((float)idim * idim), cls, nK);
    return THX_OK;
}
