// maptools.hip -- the reference's stand-alone map tools on device:
//   thx_vol_transform_rl  VOL_TRANSFORM_MAT_RL / SYMMETRIZE_RL (include/Geometry/
//                         Transformation.h:58-84, 139-163), thunder_alignZ's call
//                         (appsrc/thunder_alignZ.cpp:158-162)
//   thx_ft_resize         the Fourier crop / pad of thunder_resize (appsrc/thunder_resize.cpp:
//                         149-163)
//   thx_vol_resize        that tool's chain: fw, crop / pad, bw
//   thx_project_images    Projector::project(Image&, const dmat33&) (src/Projector.cpp:276-294)
//                         and FFT::bw per image (appsrc/thunder_project.cpp:187-204)
//   thx_vol_soft_mask     softMask(dst, src, r, ew, 0) (src/Functions/Mask.cpp:499-521), which is
//                         thunder_mask (appsrc/thunder_mask.cpp:143)
//
// The transform is a gather: one thread per output voxel, lanes along i (the stores are
// coalesced, the taps of neighbouring lanes are neighbours under any rotation, so L2 serves
// most of them); the matrix index is the same for every lane, so the matrices come through
// scalar loads (as in k_project3d); the matrices are added in index order inside the thread and
// dst is written once.  The squared norm that decides the ball is FP64 without fused
// multiply-add, in the reference's order: under a permutation matrix M x is exact and a lattice
// point at |x| = r is outside, as there.
// The projection is k_subtract's, without the CTF and the subtraction: one thread per stored
// pixel, the image index in blockIdx.y; its real-space images go through subtract.hip's
// Hermitian columns, the cached batched 2D plans and its scale / centring pass.
// No atomics anywhere: every entry is bit-identical from run to run.
#include <cmath>

#include "common.h"
#include "fft_plans.h"
#include "volume.h"

namespace {

constexpr int MT_THREADS = 256;
constexpr unsigned MT_BLOCKS = 2048;    // grid cap of the streaming kernels: eight blocks per CU
constexpr int MT_FFT_BATCH = 512;       // images per batched 2D transform (as subtract.hip)

// Volume::getByInterpolationRL's trilinear branch (src/Image/Volume.cpp:304-311): floor + 8
// weights (WG_TRI_INTERP_LINEAR), taps summed in box order k, j, i (getRL(w, x0), :482-489),
// negative indices wrapped (Volume::getRL)
THX_DEV float interp_rl(const float* __restrict__ src, int N, float x, float y, float z)
{
    const float fx = floorf(x), fy = floorf(y), fz = floorf(z);
    const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    const float dx = x - fx, dy = y - fy, dz = z - fz;
    const float vx[2] = {1.f - dx, dx};
    const float vy[2] = {1.f - dy, dy};
    const float vz[2] = {1.f - dz, dz};
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const size_t row = ((size_t)wrap_idx(z0 + k, N) * N + wrap_idx(y0 + j, N)) * N;
#pragma unroll
            for (int i = 0; i < 2; i++)
                acc += src[row + wrap_idx(x0 + i, N)] * (vx[i] * vy[j] * vz[k]);
        }
    return acc;
}

// the NEAREST_INTERP branch (:301-302): AROUND of each coordinate
THX_DEV float nearest_rl(const float* __restrict__ src, int N, float x, float y, float z)
{
    const int xi = (int)rintf(x), yi = (int)rintf(y), zi = (int)rintf(z);
    return src[((size_t)wrap_idx(zi, N) * N + wrap_idx(yi, N)) * N + wrap_idx(xi, N)];
}

// a b + c d + e f as the reference's compiler leaves it: three rounded products, added left to
// right.  Contraction is switched off here: the compiler's default would fuse them into
// multiply-adds (HIP's __dmul_rn / __dadd_rn are plain * and + and do not prevent that).
THX_DEV double dot3(double a, double b, double c, double d, double e, double f)
{
#pragma clang fp contract(off)
    return (a * b + c * d) + e * f;
}

// N^3 <= 2^30, so the flat index and its grid stride fit 32 bits.  Every tap index is wrapped
// into [0, N) and a coordinate passes the ball test only when |M x| < r <= N/2 - 1 (a NaN or
// huge matrix fails it), so no gather leaves src.
__global__ void __launch_bounds__(MT_THREADS) k_vol_transform(const float* __restrict__ src, int N,
                                                              const double* __restrict__ mat,
                                                              int nMat, double r2, int interp,
                                                              int addSrc, float* __restrict__ dst)
{
    const unsigned n = (unsigned)N, n3 = n * n * n;
    for (unsigned q = blockIdx.x * MT_THREADS + threadIdx.x; q < n3; q += gridDim.x * MT_THREADS) {
        const unsigned row = q / n;
        const double i = signed_idx((int)(q - row * n), N), j = signed_idx((int)(row % n), N),
                     k = signed_idx((int)(row / n), N);
        float acc = addSrc ? src[q] : 0.f;
        for (int m = 0; m < nMat; m++) {
            const double* M = mat + 9 * (size_t)m;      // the same for every lane: scalar loads
            const double x = dot3(M[0], i, M[1], j, M[2], k);
            const double y = dot3(M[3], i, M[4], j, M[5], k);
            const double z = dot3(M[6], i, M[7], j, M[8], k);
            if (!(dot3(x, x, y, y, z, z) < r2)) continue;
            acc += interp ? interp_rl(src, N, (float)x, (float)y, (float)z)
                          : nearest_rl(src, N, (float)x, (float)y, (float)z);
        }
        dst[q] = acc;
    }
}

// one thread per stored voxel of dst (box M): inside the common cube its value in src (box N)
__global__ void __launch_bounds__(MT_THREADS) k_ft_resize(const float2* __restrict__ src, int N,
                                                          float2* __restrict__ dst, int M)
{
    const long n = (long)(M / 2 + 1) * M * M;
    const int h = (N < M ? N : M) / 2;
    GRID_STRIDE(q, n)
    {
        int i, j, k;
        hc_coord(q, M, i, j, k);
        float2 v = make_float2(0.f, 0.f);
        if (i <= h && j >= -h && j < h && k >= -h && k < h)
            v = src[((size_t)wrap_idx(k, N) * N + wrap_idx(j, N)) * (N / 2 + 1) + i];
        dst[q] = v;
    }
}

__global__ void __launch_bounds__(MT_THREADS) k_scale(float* __restrict__ rl, long n, float scale)
{
    GRID_STRIDE(q, n) rl[q] = rl[q] * scale;
}

// image m = blockIdx.y, blockIdx.y + gridDim.y, ...: its FP64 matrix and shift are the same
// for every lane.  A coordinate beyond lim would leave the projectee: NaN instead of a gather.
__global__ void __launch_bounds__(MT_THREADS) k_project_images(
    const float2* __restrict__ vol, int vdim, int pf, const double* __restrict__ mat,
    const double* __restrict__ trans, int n, int N, int r, float2* __restrict__ imgFT,
    float2* __restrict__ imgWs)
{
    const int nc = N / 2 + 1, per = N * nc, r2 = r * r;
    const float lim = (float)(vdim / 2 - 1);
    for (int m = blockIdx.y; m < n; m += gridDim.y) {
        const double* M = mat + 9 * (size_t)m;
        const double mm[6] = {M[0], M[1], M[2], M[3], M[4], M[5]};
        // translate(): RFLOAT shift / nColRL, as k_trans_table
        const float rCol = trans ? (float)trans[2 * (size_t)m] / N : 0.f;
        const float rRow = trans ? (float)trans[2 * (size_t)m + 1] / N : 0.f;
        for (int q = blockIdx.x * MT_THREADS + threadIdx.x; q < per; q += gridDim.x * MT_THREADS) {
            const int jj = q / nc, i = q - jj * nc, j = signed_idx(jj, N);
            float2 v = make_float2(0.f, 0.f);
            if (i * i + j * j < r2) {
                float x, y, z;
                rot_coord(mm, i, j, pf, x, y, z);
                v = make_float2(__builtin_nanf(""), __builtin_nanf(""));
                if (fabsf(x) < lim && fabsf(y) < lim && fabsf(z) < lim) v = interp_ft(vol, vdim, x, y, z);
                if (trans) v = cmul(v, phase_shift(i, j, rCol, rRow));
            }
            const size_t at = (size_t)m * per + q;
            if (imgFT) imgFT[at] = v;
            if (imgWs) imgWs[at] = v;
        }
    }
}

// dst may be src: no __restrict__
__global__ void __launch_bounds__(MT_THREADS) k_vol_soft_mask(const float* src, int N, float r,
                                                              float ew, float* dst)
{
    const unsigned n = (unsigned)N, n3 = n * n * n;
    for (unsigned q = blockIdx.x * MT_THREADS + threadIdx.x; q < n3; q += gridDim.x * MT_THREADS) {
        const unsigned row = q / n;
        const int i = signed_idx((int)(q - row * n), N), j = signed_idx((int)(row % n), N),
                  k = signed_idx((int)(row / n), N);
        dst[q] = src[q] * soft_mask(sqrtf((float)(i * i + j * j + k * k)), r, ew);
    }
}

unsigned blocks(size_t n) { return thx::stream_blocks(n, MT_THREADS, MT_BLOCKS); }

struct ResizeWs {
    float* rl = nullptr;        // src's copy: the R2C may overwrite its input
    float2* A = nullptr;        // the transform at N
    float2* B = nullptr;        // the transform at M
    char* work = nullptr;       // hipFFT's work area, for the plans of N and then of M
    size_t bytes = 0;
};

ResizeWs carve_resize(void* ws, size_t cap, int N, int M)
{
    thx::Carver k(ws, cap);
    ResizeWs c;
    c.rl = k.take<float>((size_t)N * N * N);
    c.A = k.take<float2>(thx::ft_elems(N));
    c.B = k.take<float2>(thx::ft_elems(M));
    c.work = k.take<char>(thx::fft_reserve(N > M ? N : M));
    c.bytes = k.off + 256;
    return c;
}

size_t images_bytes(int n, int N) { return (size_t)n * N * (N / 2 + 1) * sizeof(float2) + 256; }

}  // namespace

extern "C" int thx_vol_transform_rl(const float* src, int N, const double* mat, int nMat, double r,
                                    int interp, int addSrc, float* dst, thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_vol_transform_rl: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(nMat >= 0, "thx_vol_transform_rl: nMat=%d is negative", nMat);
    THX_CHECK_ARG(r > 0.0 && r <= (double)(N / 2 - 1), "thx_vol_transform_rl: r=%g outside (0, N/2-1]", r);
    THX_CHECK_ARG(interp == 0 || interp == 1, "thx_vol_transform_rl: interp=%d is not 0 or 1", interp);
    THX_CHECK_ARG(src && dst, "thx_vol_transform_rl: src / dst is NULL");
    THX_CHECK_ARG(dst != src, "thx_vol_transform_rl: dst must not be src");
    THX_CHECK_ARG(nMat == 0 || mat, "thx_vol_transform_rl: mat is NULL with nMat=%d", nMat);
    THX_LAUNCH(k_vol_transform, dim3(blocks((size_t)N * N * N)), dim3(MT_THREADS), 0,
               thx::as_stream(stream), src, N, mat, nMat, r * r, interp, addSrc ? 1 : 0, dst);
    return THX_OK;
}

extern "C" int thx_ft_resize(const float* srcFT, int N, float* dstFT, int M, thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_ft_resize: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(thx::box_ok(M), "thx_ft_resize: M=%d must be even, in [16, 1024]", M);
    THX_CHECK_ARG(srcFT && dstFT, "thx_ft_resize: srcFT / dstFT is NULL");
    THX_CHECK_ARG(dstFT != srcFT, "thx_ft_resize: dstFT must not be srcFT");
    THX_LAUNCH(k_ft_resize, dim3(blocks(thx::ft_elems(M))), dim3(MT_THREADS), 0,
               thx::as_stream(stream), reinterpret_cast<const float2*>(srcFT), N,
               reinterpret_cast<float2*>(dstFT), M);
    return THX_OK;
}

extern "C" size_t thx_vol_resize_workspace(int N, int M)
{
    if (!thx::box_ok(N) || !thx::box_ok(M)) return 0;
    return carve_resize(nullptr, ~size_t(0), N, M).bytes;
}

extern "C" int thx_vol_resize(const float* src, int N, float* dst, int M, void* workspace,
                              size_t wsBytes, thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_vol_resize: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(thx::box_ok(M), "thx_vol_resize: M=%d must be even, in [16, 1024]", M);
    THX_CHECK_ARG(src && dst, "thx_vol_resize: src / dst is NULL");
    const ResizeWs c = carve_resize(workspace, wsBytes, N, M);
    THX_CHECK_ARG(workspace && wsBytes >= c.bytes, "thx_vol_resize: workspace %zu < %zu bytes",
                  workspace ? wsBytes : (size_t)0, c.bytes);
    hipStream_t s = thx::as_stream(stream);
    THX_HIP(hipMemcpyAsync(c.rl, src, sizeof(float) * N * N * N, hipMemcpyDeviceToDevice, s));
    // the plans of N, then those of M (the same entry when N == M): each entry is locked, bound
    // to the shared work area and used before the next is taken; the stream orders their use
    for (int inverse = 0; inverse < 2; inverse++) {
        const int box = inverse ? M : N;
        std::unique_lock<std::mutex> lk;
        thx::PlanEntry* pe = nullptr;
        THX_RET(thx::cached_plans(box, box / 2, s, &pe, lk));
        // the workspace query cannot ask hipFFT, so its share is a reserve: too small a one is
        // reported as what it is, a workspace that does not hold this box's plans
        THX_CHECK_ARG(pe->p.work <= thx::fft_reserve(box),
                      "thx_vol_resize: the workspace reserves %zu bytes for hipFFT's work area at "
                      "box %d, its plans need %zu",
                      thx::fft_reserve(box), box, pe->p.work);
        THX_RET(thx::bind_plans(pe->p, c.work, s));
        if (!inverse) {
            THX_RET(thx::r2c3d(pe->p, c.rl, c.A, N, s));
            THX_RET(thx_ft_resize(reinterpret_cast<const float*>(c.A), N,
                                  reinterpret_cast<float*>(c.B), M, stream));
            THX_RET(thx::hermitian_planes(c.B, M, s));
        } else {
            THX_RET(thx::c2r3d(pe->p, c.B, dst, M, s));
        }
    }
    THX_LAUNCH(k_scale, dim3(blocks((size_t)M * M * M)), dim3(MT_THREADS), 0, s, dst,
               (long)M * M * M, 1.f / ((float)M * (float)M * (float)M));
    return THX_OK;
}

extern "C" size_t thx_project_images_workspace(int n, int N)
{
    if (n < 0 || !thx::box_ok(N)) return 0;
    return images_bytes(n, N);
}

extern "C" int thx_project_images(const float* vol, int vdim, int pf, const double* mat,
                                  const double* trans, int n, int N, int r, float* imgFT,
                                  float* imgRL, int centred, void* workspace, size_t wsBytes,
                                  thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_project_images: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(pf >= 1 && (long)pf * N == vdim, "thx_project_images: vdim=%d is not pf N = %d x %d",
                  vdim, pf, N);
    THX_CHECK_ARG(n >= 0, "thx_project_images: n=%d is negative", n);
    THX_CHECK_ARG(r >= 1 && r <= N / 2 - 1, "thx_project_images: r=%d outside [1, N/2-1]", r);
    THX_CHECK_ARG(imgFT || imgRL, "thx_project_images: imgFT and imgRL are both NULL");
    const size_t need = imgRL ? images_bytes(n, N) : 0;
    THX_CHECK_ARG(!imgRL || (workspace && wsBytes >= need),
                  "thx_project_images: workspace %zu < %zu bytes", workspace ? wsBytes : (size_t)0,
                  need);
    if (n == 0) return THX_OK;
    THX_CHECK_ARG(vol && mat, "thx_project_images: vol / mat is NULL");
    hipStream_t s = thx::as_stream(stream);
    const size_t per = (size_t)N * (N / 2 + 1);
    thx::Carver cv(workspace, wsBytes);
    float2* ws = imgRL ? cv.take<float2>((size_t)n * per) : nullptr;
    THX_LAUNCH(k_project_images, dim3(blocks(per), n < 65535 ? n : 65535), dim3(MT_THREADS), 0, s,
               reinterpret_cast<const float2*>(vol), vdim, pf, mat, trans, n, N, r,
               reinterpret_cast<float2*>(imgFT), ws);
    if (!imgRL) return THX_OK;
    THX_RET(thx::hermitian_cols(ws, (size_t)n, N, s));
    for (size_t p0 = 0; p0 < (size_t)n; p0 += MT_FFT_BATCH) {
        const int nb = n - p0 < (size_t)MT_FFT_BATCH ? (int)(n - p0) : MT_FFT_BATCH;
        thx::Plans2* pl = nullptr;
        std::unique_lock<std::mutex> lk;
        THX_RET(thx::plans2d(N, nb, s, &pl, lk));
        THX_FFT(hipfftExecC2R(pl->c2r, reinterpret_cast<hipfftComplex*>(ws + p0 * per),
                              imgRL + p0 * (size_t)N * N));
    }
    return thx::rl_finish(imgRL, (size_t)n, n, N, centred, 1.f / ((float)N * N), nullptr, 1, s);
}

extern "C" int thx_vol_soft_mask(const float* src, int N, float r, float ew, float* dst,
                                 thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_vol_soft_mask: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(std::isfinite(r) && r >= 0.f, "thx_vol_soft_mask: r must be finite and >= 0");
    THX_CHECK_ARG(std::isfinite(ew) && ew > 0.f, "thx_vol_soft_mask: ew must be finite and > 0");
    THX_CHECK_ARG(src && dst, "thx_vol_soft_mask: src / dst is NULL");
    THX_LAUNCH(k_vol_soft_mask, dim3(blocks((size_t)N * N * N)), dim3(MT_THREADS), 0,
               thx::as_stream(stream), src, N, r, ew, dst);
    return THX_OK;
}
