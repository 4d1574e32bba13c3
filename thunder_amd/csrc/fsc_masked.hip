// fsc_masked.hip -- the masked / core-region branch of
// Model::compareTwoHemispheres (src/Model.cpp:411-567; 3D only, as there):
//
//   1. fscUnmask = FSC(A, B)                       (src/Functions/Spectrum.cpp:302-337)
//   2. t = resP(fscUnmask, 0.8, 1, 1, false)       (:339-363, the trailing result-- included;
//                                                   the threshold is the RFLOAT 0.8)
//   3. randomPhase (:365-386): a stored voxel q whose shell rint|(i, j, k)| is above t is
//      multiplied by exp(2 pi i u), u = draw 0 of the Philox stream (q >> 32, q & 0xffffffff,
//      tag), one tag for A and one for B (the reference draws from an urandom-seeded GSL
//      generator); written out of place, so it is also the copy the inverse transform needs
//   4. bw, softMask with bg = 0 (src/Functions/Mask.cpp:533-544: v (1 - (1 - alpha))), fw, for
//      the randomised pair -> fscRF, and for plain copies of A and B -> fscMask.  alpha is the
//      caller's map (_maskFSC) or softMask(mask, coreR, edge) (:466-487, _coreFSC) evaluated
//      in the multiply kernel, never materialised
//   5. fsc[u] = fscMask[u] for u < t + 2, else (fscMask[u] - fscRF[u]) / (1 - fscRF[u]); no
//      guard on that divisor, as in the reference (:555-561)
//
// Before each inverse transform the planes i = 0 and i = N/2 of the copy are replaced by
// their Hermitian part (z(j, k) + conj z(-j, -k)) / 2 -- all FFTW's c2r, which the reference
// runs, reads of them; random phases leave them inconsistent, and how hipFFT or the column
// passes read an inconsistent plane is their own choice (the precedent: subtract.hip).
//
// The shell sums are FP64 in a fixed order, without atomics (volume.h: shell_pass per block,
// sum_slots in the final block).  Everything is stream-ordered with no host round trip, and the
// whole call is bit-identical from run to run.
#include <cmath>

#include "common.h"
#include "fft_plans.h"
#include "volume.h"

namespace {

constexpr int FM_THREADS = 256;
constexpr int FM_WAVES = FM_THREADS / 64;
constexpr int FM_MAX_BLOCKS = 1024;     // four per CU; the final pass walks them in order
constexpr int FM_FINAL = 1024;          // threads of the final pass (3 nShell sums)
constexpr uint32_t FM_TAG_A = 0x72706841u;   // "rphA": counter word c of A's phase stream
constexpr uint32_t FM_TAG_B = 0x72706842u;   // "rphB"

// part[block][3][nShell] = the block's sums of Re(a conj b), |a|^2, |b|^2 per shell
__global__ void __launch_bounds__(FM_THREADS) k_shell_partial(const float2* __restrict__ A,
                                                              const float2* __restrict__ B, int N,
                                                              int nShell, double* __restrict__ part)
{
    extern __shared__ double sh[];      // [FM_WAVES][3][nShell]
    const int nc = N / 2 + 1;
    shell_pass<3, FM_WAVES>(sh, N, nShell, nShell, part, [=](long row, int i, int, double* s) {
        const float2 a = A[row * nc + i], b = B[row * nc + i];
        s[0] = (double)a.x * b.x + (double)a.y * b.y;
        s[1] = (double)a.x * a.x + (double)a.y * a.y;
        s[2] = (double)b.x * b.x + (double)b.y * b.y;
        return true;
    });
}

// one block: the slots in block order, the curve, and (thres != NULL) resP
__global__ void __launch_bounds__(FM_FINAL) k_shell_final(const double* __restrict__ part,
                                                          int nBlock, int nShell,
                                                          double* __restrict__ curve,
                                                          int* __restrict__ thres)
{
    extern __shared__ double acc[];     // [3][nShell], then the curve [nShell]
    double* cur = acc + 3 * nShell;
    for (int s = threadIdx.x; s < 3 * nShell; s += FM_FINAL)
        acc[s] = sum_slots<3>(part, nBlock, nShell, s);
    __syncthreads();
    for (int u = threadIdx.x; u < nShell; u += FM_FINAL) {
        const double ab = sqrt(acc[nShell + u] * acc[2 * nShell + u]);
        cur[u] = ab == 0.0 ? 0.0 : acc[u] / ab;
        curve[u] = cur[u];
    }
    __syncthreads();
    if (thres && threadIdx.x == 0) *thres = res_p(cur, nShell, 0.8f);
}

__global__ void __launch_bounds__(FM_THREADS) k_random_phase(const float2* __restrict__ src,
                                                             float2* __restrict__ dst, int N,
                                                             const int* __restrict__ thres,
                                                             uint64_t seed, uint32_t tag)
{
    const int nc = N / 2 + 1;
    const size_t n = (size_t)nc * N * N;
    const int t = *thres;
    for (size_t q = blockIdx.x * (size_t)FM_THREADS + threadIdx.x; q < n;
         q += (size_t)gridDim.x * FM_THREADS) {
        const int i = (int)(q % nc);
        const size_t jk = q / nc;
        const int j = signed_idx((int)(jk % N), N), k = signed_idx((int)(jk / N), N);
        float2 v = src[q];
        if (shell_of(i * i + j * j + k * k) > t) {
            Philox ph(seed, (uint32_t)(q >> 32), (uint32_t)q, tag);
            double sn, cs;
            sincospi(2.0 * ph.uniform(), &sn, &cs);
            v = cmul(v, make_float2((float)cs, (float)sn));
        }
        dst[q] = v;
    }
}

// planes i = 0 and i = N/2 of a half-complex volume <- their Hermitian part; one thread per
// pair (z(j, k), z(-j, -k)), the one at the lower address
__global__ void __launch_bounds__(FM_THREADS) k_hermitian_planes(float2* __restrict__ ft, int N)
{
    const int nc = N / 2 + 1;
    const size_t tot = (size_t)2 * N * N;
    const size_t e = blockIdx.x * (size_t)FM_THREADS + threadIdx.x;
    if (e >= tot) return;
    const int col = e < (size_t)N * N ? 0 : N / 2;
    const size_t r = e % ((size_t)N * N);
    const int jr = (int)(r % N), kr = (int)(r / N);
    const size_t a = ((size_t)kr * N + jr) * nc + col;
    const size_t b = ((size_t)((N - kr) % N) * N + (N - jr) % N) * nc + col;
    if (a > b) return;
    const float2 va = ft[a], vb = ft[b];
    const float2 h = make_float2((va.x + vb.x) * 0.5f, (va.y - vb.y) * 0.5f);
    ft[a] = h;                          // a == b for the self-paired points: the real part
    if (a != b) ft[b] = make_float2(h.x, -h.y);
}

// after the C2R, in place: bw's 1 / N^3, then softMask with bg = 0
__global__ void __launch_bounds__(FM_THREADS) k_mask_mul(float* __restrict__ rl,
                                                         const float* __restrict__ alpha, int N,
                                                         float coreR, float edge, float scale)
{
    const size_t n3 = (size_t)N * N * N;
    for (size_t q = blockIdx.x * (size_t)FM_THREADS + threadIdx.x; q < n3;
         q += (size_t)gridDim.x * FM_THREADS) {
        float al;
        if (alpha) {
            al = alpha[q];
        } else {
            const int i = signed_idx((int)(q % N), N), j = signed_idx((int)(q / N % N), N);
            const int k = signed_idx((int)(q / ((size_t)N * N)), N);
            const float u = sqrtf((float)(i * i + j * j + k * k));
            if (u > coreR + edge) al = 0.f;
            else if (u >= coreR) al = 0.5f + 0.5f * cosf((u - coreR) / edge * (float)M_PI);
            else al = 1.f;
        }
        rl[q] = rl[q] * scale * (1.f - (1.f - al));
    }
}

// cur = [unmasked, masked, randomised][nShell]
__global__ void k_fsc_combine(const double* __restrict__ cur, const int* __restrict__ thres,
                              int nShell, double* __restrict__ fsc, double* __restrict__ curves,
                              int* __restrict__ thresOut)
{
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nShell) return;
    const int t = *thres;
    const double m = cur[nShell + u], rf = cur[2 * nShell + u];
    fsc[u] = u < t + 2 ? m : (m - rf) / (1.0 - rf);
    if (curves)
        for (int c = 0; c < 3; c++) curves[c * nShell + u] = cur[c * nShell + u];
    if (thresOut && u == 0) *thresOut = t;
}

int shell_blocks(int N) { return thx::shell_blocks(N, FM_WAVES, FM_MAX_BLOCKS); }
unsigned stream_blocks(size_t n) { return thx::stream_blocks(n, FM_THREADS, 4096); }

struct Carved {
    double* part = nullptr;
    double* cur = nullptr;
    int* thres = nullptr;
    float2* CA = nullptr;
    float2* CB = nullptr;
    float* rl = nullptr;
    char* work = nullptr;
    size_t bytes = 0;
};

Carved carve(void* ws, size_t cap, int N, int nShell)
{
    thx::Carver k(ws, cap);
    Carved c;
    c.part = k.take<double>((size_t)shell_blocks(N) * 3 * nShell);
    c.cur = k.take<double>((size_t)3 * nShell);
    c.thres = k.take<int>(1);
    c.CA = k.take<float2>(thx::ft_elems(N));
    c.CB = k.take<float2>(thx::ft_elems(N));
    c.rl = k.take<float>((size_t)N * N * N);
    c.work = k.take<char>(thx::fft_reserve(N));
    c.bytes = k.off + 256;
    return c;
}

int shell_curve(const float2* A, const float2* B, int N, int nShell, double* part, double* curve,
                int* thres, hipStream_t s)
{
    const int nb = shell_blocks(N);
    THX_LAUNCH(k_shell_partial, dim3(nb), dim3(FM_THREADS), sizeof(double) * FM_WAVES * 3 * nShell, s,
               A, B, N, nShell, part);
    THX_LAUNCH(k_shell_final, dim3(1), dim3(FM_FINAL), sizeof(double) * 4 * nShell, s, part, nb,
               nShell, curve, thres);
    return THX_OK;
}

}  // namespace

int thx::hermitian_planes(float2* ft, int N, hipStream_t s)
{
    THX_LAUNCH(k_hermitian_planes, dim3(thx::cdiv((long)2 * N * N, FM_THREADS)), dim3(FM_THREADS), 0,
               s, ft, N);
    return THX_OK;
}

extern "C" size_t thx_fsc_masked_workspace(int N, int nShell)
{
    if (!thx::box_ok(N) || !thx::shells_ok(N, nShell)) return 0;
    return carve(nullptr, ~size_t(0), N, nShell).bytes;
}

extern "C" int thx_fsc_masked(const float* A, const float* B, int N, int nShell,
                              const float* alphaMask, float coreR, float edge,
                              unsigned long long seed, int method, double* fsc, double* curves,
                              int* thres, void* workspace, size_t wsBytes, thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_fsc_masked: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(thx::shells_ok(N, nShell), "thx_fsc_masked: nShell=%d outside [2, N/2]", nShell);
    THX_CHECK_ARG(method >= 0 && method <= 2, "thx_fsc_masked: method is 0, 1 or 2");
    THX_CHECK_ARG(method != 2 || (N & (N - 1)) == 0,
                  "thx_fsc_masked: the column passes need a power-of-two N");
    const bool core = coreR > 0.f;
    THX_CHECK_ARG(std::isfinite(coreR), "thx_fsc_masked: coreR is not finite");
    THX_CHECK_ARG(!(core && alphaMask), "thx_fsc_masked: alphaMask and coreR are exclusive");
    THX_CHECK_ARG(core || alphaMask, "thx_fsc_masked: neither alphaMask nor coreR > 0 is given");
    THX_CHECK_ARG(!core || (std::isfinite(edge) && edge > 0.f),
                  "thx_fsc_masked: the core mask needs a finite edge > 0");
    THX_CHECK_ARG(A && B && fsc, "thx_fsc_masked: A / B / fsc is NULL");
    const Carved c = carve(workspace, wsBytes, N, nShell);
    THX_CHECK_ARG(workspace && wsBytes >= c.bytes, "thx_fsc_masked: workspace %zu < %zu bytes",
                  workspace ? wsBytes : (size_t)0, c.bytes);
    hipStream_t s = thx::as_stream(stream);
    std::unique_lock<std::mutex> lk;
    thx::PlanEntry* pe = nullptr;
    THX_RET(thx::cached_plans(N, N / 2, s, &pe, lk));
    const thx::Plans& pl = pe->p;
    THX_CHECK_ARG(method != 2 || pl.cols, "thx_fsc_masked: no column passes for N=%d", N);
    THX_CHECK_ARG(pl.work <= thx::fft_reserve(N), "thx_fsc_masked: hipFFT's work area exceeds the reserve");
    THX_RET(thx::bind_plans(pl, c.work, s));
    const float2* A2 = reinterpret_cast<const float2*>(A);
    const float2* B2 = reinterpret_cast<const float2*>(B);
    const size_t nFT = thx::ft_elems(N), n3 = (size_t)N * N * N;
    const float scale = 1.f / ((float)N * (float)N * (float)N);
    THX_RET(shell_curve(A2, B2, N, nShell, c.part, c.cur, c.thres, s));
    for (int pass = 0; pass < 2; pass++) {      // 0: randomised -> cur[2], 1: plain -> cur[1]
        if (pass == 0) {
            THX_LAUNCH(k_random_phase, dim3(stream_blocks(nFT)), dim3(FM_THREADS), 0, s, A2, c.CA, N,
                       c.thres, (uint64_t)seed, FM_TAG_A);
            THX_LAUNCH(k_random_phase, dim3(stream_blocks(nFT)), dim3(FM_THREADS), 0, s, B2, c.CB, N,
                       c.thres, (uint64_t)seed, FM_TAG_B);
        } else {
            THX_HIP(hipMemcpyAsync(c.CA, A, nFT * sizeof(float2), hipMemcpyDeviceToDevice, s));
            THX_HIP(hipMemcpyAsync(c.CB, B, nFT * sizeof(float2), hipMemcpyDeviceToDevice, s));
        }
        for (float2* C : {c.CA, c.CB}) {
            THX_RET(thx::hermitian_planes(C, N, s));
            THX_RET(thx::c2r3d(pl, C, c.rl, N, s, method));
            THX_LAUNCH(k_mask_mul, dim3(stream_blocks(n3)), dim3(FM_THREADS), 0, s, c.rl, alphaMask,
                       N, coreR, edge, scale);
            THX_RET(thx::r2c3d(pl, c.rl, C, N, s, method));
        }
        THX_RET(shell_curve(c.CA, c.CB, N, nShell, c.part, c.cur + (pass == 0 ? 2 : 1) * nShell,
                            nullptr, s));
    }
    THX_LAUNCH(k_fsc_combine, dim3(thx::cdiv(nShell, 256)), dim3(256), 0, s, c.cur, c.thres, nShell,
               fsc, curves, thres);
    return THX_OK;
}
