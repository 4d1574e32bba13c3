// postprocess.hip -- what Postprocess::run (src/Postprocess.cpp:50-183) does after
// saveFSC(): the 0.143 resolution, mergeAB (:207-213), fscWeightingFilter
// (src/Functions/Filter.cpp:144-167), bFactorEst (src/Functions/Spectrum.cpp:414-453),
// sharpen (:402-412: bFactorFilter, Filter.cpp:29-44, then lowPassFilter, :69-92), the inverse
// transform and softMask with bg = 0.  The same filters are thunder_lowpass
// (appsrc/thunder_lowpass.cpp:146-150) and thunder_bfactor.
//
// The reference makes five read-modify-write sweeps of the merged half-complex map; here the
// halves are read twice and one half-complex map is written once:
//   pass 1  k_guinier_partial: |A + B| / 2 summed per shell (nothing else is written; the FSC
//           weight is constant on a shell, so it multiplies the shell's sum in the fit)
//   pass 2  k_ft_stream: (A + B) / 2, times the FSC weight, times exp(-0.5 b f^2), times the low
//           pass, each product rounded to FP32 as the reference's three sweeps round
//
// The shell index is rint(sqrt(i^2 + j^2 + k^2)) from the integer q2 (volume.h's shell_of).
// fscWeightingFilter's literal FP32 expression AROUND(NORM_3(i/N, j/N, k/N) N) gives the same
// index at every stored voxel for N = 48, 96, 100, 200, 250, 384, 400 and 500 (counted in
// numpy: zero differences; tests/postprocess_ref.py holds both forms and
// tests/test_postprocess.py compares them at N = 32, 48 and 100).
//
// The Guinier sums (one sum and one count per shell) are FP64 in a fixed order without atomics
// (volume.h: shell_pass per block, sum_slots in the final block).  The fit itself runs in FP64
// in that last block (the reference accumulates in RFLOAT).
// Everything is stream-ordered, nothing is allocated, nothing is read back.
#include <cmath>

#include "common.h"
#include "fft_plans.h"
#include "volume.h"

namespace {

constexpr int PP_THREADS = 256;
constexpr int PP_WAVES = PP_THREADS / 64;
constexpr int PP_MAX_BLOCKS = 1024;     // Guinier partials: four per CU, walked in order
constexpr int PP_FINAL = 1024;
constexpr unsigned PP_STREAM_BLOCKS = 2048;   // grid cap of the streaming kernels: eight
                                              // 256-thread blocks per CU (k_ft_stream holds five
                                              // at its 94 VGPRs, k_pp_scale_mask all eight)

// sqrt(max(0, 2 fsc / (1 + fsc))) as the reference's RFLOAT
THX_DEV float fsc_weight(double f) { return (float)sqrt(fmax(0.0, 2.0 * f / (1.0 + f))); }

struct StreamArgs {
    const float2* A;
    const float2* B;            // NULL: dst = A
    float2* dst;
    int N;
    const double* fsc;          // NULL: no FSC weight
    int nShell;
    float b;                    // the B-factor, or bDev[0] (a double) when bDev != NULL
    const double* bDev;
    float thres, ew;            // the low pass in 1 / box; thresDev: (float)*thresDev / N
    const int* thresDev;
    int lowPass;                // 0: no low pass
};

// one stored voxel: merge, FSC weight, B-factor factor, low pass, in the reference's order,
// every product rounded to FP32
THX_DEV float2 filter_voxel(float2 v, int i, int j, int k, float fN, const float* wtab,
                            int nShell, bool weigh, float b, float thres, float hi, float ew,
                            bool lowPass)
{
    if (weigh) {
        const int u = shell_of(i * i + j * j + k * k);
        const float w = u < nShell ? wtab[u] : 0.f;
        v = make_float2(v.x * w, v.y * w);
    }
    if (b == 0.f && !lowPass) return v;
    const float x = (float)i / fN, y = (float)j / fN, z = (float)k / fN;
    const float f2 = __fadd_rn(__fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y)), __fmul_rn(z, z));
    const float f = sqrtf(f2);
    if (lowPass && f > hi) return make_float2(0.f, 0.f);    // the stop band needs no exp
    if (b != 0.f) {
        const float e = (float)exp(-0.5 * (double)b * (double)f2);
        v = make_float2(v.x * e, v.y * e);
    }
    if (lowPass && !(f < thres)) {
        const float c = (float)(cos((double)(f - thres) * M_PI / (double)ew) / 2 + 0.5);
        v = make_float2(v.x * c, v.y * c);
    }
    return v;
}

// VEC consecutive stored voxels per lane (VEC = 2: 16-byte loads of the flat array, whose
// element count N^2 (N/2 + 1) is even; rows themselves are only 8-byte aligned, N/2 + 1
// being odd for N = 4m), lanes along i
template <int VEC>
__global__ void __launch_bounds__(PP_THREADS) k_ft_stream(const StreamArgs a)
{
    extern __shared__ float wtab[];     // [nShell] FSC weights
    const bool weigh = a.fsc != nullptr;
    if (weigh) {
        for (int u = threadIdx.x; u < a.nShell; u += PP_THREADS) wtab[u] = fsc_weight(a.fsc[u]);
        __syncthreads();
    }
    const int N = a.N, nc = N / 2 + 1;
    const float fN = (float)N;
    const float b = a.bDev ? (float)a.bDev[0] : a.b;
    const float thres = a.thresDev ? (float)(*a.thresDev) / fN : a.thres;
    const float hi = thres + a.ew;
    const bool lowPass = a.lowPass != 0;
    const size_t n = (size_t)nc * N * N / VEC;
    for (size_t p = blockIdx.x * (size_t)PP_THREADS + threadIdx.x; p < n;
         p += (size_t)gridDim.x * PP_THREADS) {
        float2 v[VEC];
        if (VEC == 2) {
            const float4 va = reinterpret_cast<const float4*>(a.A)[p];
            v[0] = make_float2(va.x, va.y);
            v[VEC - 1] = make_float2(va.z, va.w);
            if (a.B) {
                const float4 vb = reinterpret_cast<const float4*>(a.B)[p];
                v[0] = make_float2((v[0].x + vb.x) / 2, (v[0].y + vb.y) / 2);
                v[VEC - 1] = make_float2((v[VEC - 1].x + vb.z) / 2, (v[VEC - 1].y + vb.w) / 2);
            }
        } else {
            v[0] = a.A[p];
            if (a.B) {
                const float2 vb = a.B[p];
                v[0] = make_float2((v[0].x + vb.x) / 2, (v[0].y + vb.y) / 2);
            }
        }
        size_t row = p * VEC / nc;
        int i = (int)(p * VEC - row * nc);
#pragma unroll
        for (int e = 0; e < VEC; e++) {
            const int j = signed_idx((int)(row % N), N), k = signed_idx((int)(row / N), N);
            v[e] = filter_voxel(v[e], i, j, k, fN, wtab, a.nShell, weigh, b, thres, hi, a.ew,
                                lowPass);
            if (++i == nc) {
                i = 0;
                row++;
            }
        }
        if (VEC == 2)
            reinterpret_cast<float4*>(a.dst)[p] = make_float4(v[0].x, v[0].y, v[VEC - 1].x, v[VEC - 1].y);
        else
            a.dst[p] = v[0];
    }
}

// the fit's upper shell: nTab, or *rUdev clamped to [0, nTab]
THX_DEV int upper_shell(const int* rUdev, int nTab) { return rUdev ? min(max(*rUdev, 0), nTab) : nTab; }

// part[block][2][nTab] = the block's sums of |F| and of 1 over the stored voxels of shells
// [rL, rU); F = A, or (A + B) / 2 rounded to FP32 as mergeAB stores it
__global__ void __launch_bounds__(PP_THREADS) k_guinier_partial(const float2* __restrict__ A,
                                                                const float2* __restrict__ B,
                                                                int N, int rL, int nTab,
                                                                const int* __restrict__ rUdev,
                                                                double* __restrict__ part)
{
    extern __shared__ double sh[];      // [PP_WAVES][2][nTab]
    const int nc = N / 2 + 1;
    shell_pass<2, PP_WAVES>(sh, N, nTab, upper_shell(rUdev, nTab), part,
                            [=](long row, int i, int u, double* s) {
        if (u < rL) return false;
        float2 v = A[row * nc + i];
        if (B) {
            const float2 vb = B[row * nc + i];
            v = make_float2((v.x + vb.x) / 2, (v.y + vb.y) / 2);
        }
        s[0] = sqrt((double)v.x * v.x + (double)v.y * v.y);
        s[1] = 1.0;
        return true;
    });
}

// one block: the slots in block order, then the fit.  GSL's unweighted fit_linear:
// c1 = sum (x - mx)(y - my) / sum (x - mx)^2, c0 = my - c1 mx
__global__ void __launch_bounds__(PP_FINAL) k_guinier_fit(const double* __restrict__ part,
                                                          int nBlock, int N, int rL, int nTab,
                                                          const int* __restrict__ rUdev,
                                                          const double* __restrict__ w,
                                                          double* __restrict__ out,
                                                          double* __restrict__ guinier,
                                                          int* __restrict__ nFitOut)
{
    extern __shared__ double acc[];     // [2][nTab] sums and counts, then x and y
    for (int s = threadIdx.x; s < 2 * nTab; s += PP_FINAL)
        acc[s] = sum_slots<2>(part, nBlock, nTab, s);
    __syncthreads();
    const int rU = upper_shell(rUdev, nTab), n = rU - rL;
    __shared__ int bad;
    if (threadIdx.x == 0) bad = n < 2;
    __syncthreads();
    for (int u = rL + threadIdx.x; u < rU; u += PP_FINAL) {
        const double sum = acc[u] * (w ? w[u] : 1.0), cnt = acc[nTab + u];
        const float xf = (float)u / (float)N;
        if (!(cnt > 0.0) || !(sum > 0.0) || !(sum < INFINITY)) bad = 1;    // benign race: all write 1
        acc[u] = (double)__fmul_rn(xf, xf);
        acc[nTab + u] = (cnt > 0.0 && sum > 0.0) ? log(sum / cnt) : 0.0;
    }
    __syncthreads();
    if (guinier)
        for (int e = threadIdx.x; e < nTab; e += PP_FINAL) {
            const bool in = e < n;
            guinier[e] = in ? acc[rL + e] : 0.0;
            guinier[nTab + e] = in ? acc[nTab + rL + e] : 0.0;
        }
    if (threadIdx.x != 0) return;
    double c0 = 0.0, c1 = 0.0;
    if (!bad) {
        double mx = 0.0, my = 0.0;
        for (int u = rL; u < rU; u++) {
            mx += acc[u];
            my += acc[nTab + u];
        }
        mx /= n;
        my /= n;
        double sxx = 0.0, sxy = 0.0;
        for (int u = rL; u < rU; u++) {
            const double dx = acc[u] - mx;
            sxx += dx * dx;
            sxy += dx * (acc[nTab + u] - my);
        }
        c1 = sxy / sxx;
        c0 = my - c1 * mx;
    }
    out[0] = 2.0 * c1;
    out[1] = c0;
    out[2] = (double)(n > 0 ? n : 0);
    out[3] = bad ? 1.0 : 0.0;
    if (nFitOut) *nFitOut = n > 0 ? n : 0;
}

// the chain's small step between the FSC and pass 1: res = resP(fsc, 0.143, 1, 1, false), the
// FSC weight per shell as a double for the fit, and, with a given B-factor, the fit's outputs
__global__ void k_pp_prepare(const double* __restrict__ fsc, int nShell, int rL, double bIn,
                             int given, int* __restrict__ info, double* __restrict__ wd,
                             double* __restrict__ fit, double* __restrict__ guinier)
{
    for (int u = threadIdx.x; u < nShell; u += blockDim.x) {
        wd[u] = (double)fsc_weight(fsc[u]);
        if (given && guinier) guinier[u] = guinier[nShell + u] = 0.0;
    }
    if (threadIdx.x != 0) return;
    info[1] = res_p(fsc, nShell, 0.143f);
    info[2] = rL;
    if (given) {
        info[3] = 0;
        fit[0] = bIn;
        fit[1] = fit[2] = fit[3] = 0.0;
    }
}

// after the C2R, in place: bw's 1 / N^3, then softMask with bg = 0 (alpha NULL: the scale only)
__global__ void __launch_bounds__(PP_THREADS) k_pp_scale_mask(float* __restrict__ rl,
                                                              const float* __restrict__ alpha,
                                                              size_t n4, float scale)
{
    float4* r4 = reinterpret_cast<float4*>(rl);
    const float4* a4 = reinterpret_cast<const float4*>(alpha);
    for (size_t q = blockIdx.x * (size_t)PP_THREADS + threadIdx.x; q < n4;
         q += (size_t)gridDim.x * PP_THREADS) {
        float4 v = r4[q];
        v = make_float4(v.x * scale, v.y * scale, v.z * scale, v.w * scale);
        if (alpha) {
            const float4 al = a4[q];
            v = make_float4(v.x * (1.f - (1.f - al.x)), v.y * (1.f - (1.f - al.y)),
                            v.z * (1.f - (1.f - al.z)), v.w * (1.f - (1.f - al.w)));
        }
        r4[q] = v;
    }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
int guinier_blocks(int N) { return thx::shell_blocks(N, PP_WAVES, PP_MAX_BLOCKS); }
unsigned stream_blocks(size_t n) { return thx::stream_blocks(n, PP_THREADS, PP_STREAM_BLOCKS); }

size_t guinier_bytes(int N, int nTab) { return (size_t)guinier_blocks(N) * 2 * nTab * sizeof(double) + 256; }

int launch_stream(const StreamArgs& a, hipStream_t s)
{
    const size_t lds = a.fsc ? sizeof(float) * a.nShell : 0;
    const size_t n = thx::ft_elems(a.N);
    if (aligned16(a.A) && aligned16(a.dst) && (!a.B || aligned16(a.B)))
        THX_LAUNCH(k_ft_stream<2>, dim3(stream_blocks(n / 2)), dim3(PP_THREADS), lds, s, a);
    else
        THX_LAUNCH(k_ft_stream<1>, dim3(stream_blocks(n)), dim3(PP_THREADS), lds, s, a);
    return THX_OK;
}

int launch_guinier(const float2* A, const float2* B, int N, int rL, int nTab, const int* rUdev,
                   const double* w, double* out, double* guinier, int* nFitOut, double* part,
                   hipStream_t s)
{
    const int nb = guinier_blocks(N);
    THX_LAUNCH(k_guinier_partial, dim3(nb), dim3(PP_THREADS), sizeof(double) * PP_WAVES * 2 * nTab, s,
               A, B, N, rL, nTab, rUdev, part);
    THX_LAUNCH(k_guinier_fit, dim3(1), dim3(PP_FINAL), sizeof(double) * 2 * nTab, s, part, nb, N, rL,
               nTab, rUdev, w, out, guinier, nFitOut);
    return THX_OK;
}

struct Carved {
    double* part = nullptr;
    double* wd = nullptr;
    char* shared = nullptr;     // thx_fsc_masked's workspace, then C and hipFFT's work area
    size_t sharedBytes = 0;
    size_t bytes = 0;
};

Carved carve(void* ws, size_t cap, int N, int nShell)
{
    thx::Carver k(ws, cap);
    Carved c;
    c.part = k.take<double>((size_t)guinier_blocks(N) * 2 * nShell);
    c.wd = k.take<double>(nShell);
    c.sharedBytes = thx_fsc_masked_workspace(N, nShell);
    const size_t own = thx::ft_elems(N) * sizeof(float2) + 256 + thx::fft_reserve(N);
    if (c.sharedBytes < own) c.sharedBytes = own;
    c.shared = k.take<char>(c.sharedBytes);
    c.bytes = k.off + 256;
    return c;
}

}  // namespace

extern "C" int thx_ft_merge_weight(const float* A, const float* B, int N, const double* fsc,
                                   int nShell, float* dst, thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_ft_merge_weight: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(!fsc || thx::shells_ok(N, nShell), "thx_ft_merge_weight: nShell=%d outside [2, N/2]",
                  nShell);
    THX_CHECK_ARG(A && dst, "thx_ft_merge_weight: A / dst is NULL");
    StreamArgs a{};
    a.A = reinterpret_cast<const float2*>(A);
    a.B = reinterpret_cast<const float2*>(B);
    a.dst = reinterpret_cast<float2*>(dst);
    a.N = N;
    a.fsc = fsc;
    a.nShell = fsc ? nShell : 0;
    return launch_stream(a, thx::as_stream(stream));
}

extern "C" size_t thx_bfactor_est_workspace(int N, int rU)
{
    if (!thx::box_ok(N) || rU < 1 || rU > N / 2) return 0;
    return guinier_bytes(N, rU);
}

extern "C" int thx_bfactor_est(const float* F, int N, int rL, int rU, const int* rUdev,
                               const double* w, double* out, double* guinier, void* workspace,
                               size_t wsBytes, thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_bfactor_est: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(rU >= 1 && rU <= N / 2, "thx_bfactor_est: rU=%d outside [1, N/2]", rU);
    THX_CHECK_ARG(rL >= 0, "thx_bfactor_est: rL=%d is negative", rL);
    THX_CHECK_ARG(F && out, "thx_bfactor_est: F / out is NULL");
    const size_t need = guinier_bytes(N, rU);
    THX_CHECK_ARG(workspace && wsBytes >= need, "thx_bfactor_est: workspace %zu < %zu bytes",
                  workspace ? wsBytes : (size_t)0, need);
    thx::Carver k(workspace, wsBytes);
    double* part = k.take<double>((size_t)guinier_blocks(N) * 2 * rU);
    return launch_guinier(reinterpret_cast<const float2*>(F), nullptr, N, rL, rU, rUdev, w, out,
                          guinier, nullptr, part, thx::as_stream(stream));
}

extern "C" int thx_ft_sharpen(const float* src, int N, float bFactor, const double* bFactorDev,
                              float thres, const int* thresDev, float ew, float* dst,
                              thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_ft_sharpen: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(bFactorDev || std::isfinite(bFactor), "thx_ft_sharpen: bFactor is not finite");
    THX_CHECK_ARG(thresDev || std::isfinite(thres), "thx_ft_sharpen: thres is not finite");
    THX_CHECK_ARG(std::isfinite(ew), "thx_ft_sharpen: ew is not finite");
    THX_CHECK_ARG(src && dst, "thx_ft_sharpen: src / dst is NULL");
    StreamArgs a{};
    a.A = reinterpret_cast<const float2*>(src);
    a.dst = reinterpret_cast<float2*>(dst);
    a.N = N;
    a.b = bFactor;
    a.bDev = bFactorDev;
    a.thres = thres;
    a.thresDev = thresDev;
    a.ew = ew;
    a.lowPass = ew > 0.f && (thresDev || thres >= 0.f);
    return launch_stream(a, thx::as_stream(stream));
}

extern "C" size_t thx_postprocess_workspace(int N, int nShell, int wantAverage)
{
    (void)wantAverage;          // the average reuses the sharpened map's half-complex buffer
    if (!thx::box_ok(N) || !thx::shells_ok(N, nShell)) return 0;
    return carve(nullptr, ~size_t(0), N, nShell).bytes;
}

extern "C" int thx_postprocess(const float* A, const float* B, int N, int nShell,
                               const float* alphaMask, float pixelSize, float lowResA, float edgeFT,
                               double bFactorIn, unsigned long long seed, int method, double* fsc,
                               double* curves, int* info, double* fit, double* guinier,
                               float* average, float* sharp, void* workspace, size_t wsBytes,
                               thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_postprocess: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(thx::shells_ok(N, nShell), "thx_postprocess: nShell=%d outside [2, N/2]", nShell);
    THX_CHECK_ARG(method >= 0 && method <= 2, "thx_postprocess: method is 0, 1 or 2");
    THX_CHECK_ARG(method != 2 || (N & (N - 1)) == 0,
                  "thx_postprocess: the column passes need a power-of-two N");
    THX_CHECK_ARG(std::isfinite(pixelSize) && pixelSize > 0.f,
                  "thx_postprocess: pixelSize must be finite and > 0");
    THX_CHECK_ARG(std::isfinite(lowResA) && lowResA > 0.f,
                  "thx_postprocess: lowResA must be finite and > 0");
    THX_CHECK_ARG(std::isfinite(edgeFT), "thx_postprocess: edgeFT is not finite");
    THX_CHECK_ARG(!std::isinf(bFactorIn), "thx_postprocess: bFactorIn is infinite (NaN: estimate)");
    THX_CHECK_ARG(A && B && alphaMask, "thx_postprocess: A / B / alphaMask is NULL");
    THX_CHECK_ARG(fsc && info && fit && sharp, "thx_postprocess: fsc / info / fit / sharp is NULL");
    THX_CHECK_ARG(aligned16(alphaMask) && aligned16(sharp) && aligned16(average),
                  "thx_postprocess: alphaMask / sharp / average must be 16-byte aligned");
    // AROUND(resA2P(1 / lowResA, N, pixelSize)) in the reference's RFLOAT
    const float rLf = rintf((float)N * pixelSize / lowResA);
    THX_CHECK_ARG(rLf >= 0.f && rLf < 1e6f, "thx_postprocess: rL from pixelSize / lowResA is out of range");
    const int rL = (int)rLf;
    const Carved c = carve(workspace, wsBytes, N, nShell);
    THX_CHECK_ARG(workspace && wsBytes >= c.bytes, "thx_postprocess: workspace %zu < %zu bytes",
                  workspace ? wsBytes : (size_t)0, c.bytes);
    hipStream_t s = thx::as_stream(stream);
    const float2* A2 = reinterpret_cast<const float2*>(A);
    const float2* B2 = reinterpret_cast<const float2*>(B);
    THX_RET(thx_fsc_masked(A, B, N, nShell, alphaMask, 0.f, 0.f, seed, method, fsc, curves, info,
                           c.shared, c.sharedBytes, stream));
    const bool given = !std::isnan(bFactorIn);
    THX_LAUNCH(k_pp_prepare, dim3(1), dim3(256), 0, s, fsc, nShell, rL, given ? bFactorIn : 0.0,
               given ? 1 : 0, info, c.wd, fit, guinier);
    if (!given)
        THX_RET(launch_guinier(A2, B2, N, rL, nShell, info + 1, c.wd, fit, guinier, info + 3, c.part,
                               s));
    // the FSC is done with its workspace: the merged map and hipFFT's work area live there now
    float2* C = reinterpret_cast<float2*>(c.shared);
    char* work = c.shared + ((thx::ft_elems(N) * sizeof(float2) + 255) & ~size_t(255));
    std::unique_lock<std::mutex> lk;
    thx::PlanEntry* pe = nullptr;
    THX_RET(thx::cached_plans(N, N / 2, s, &pe, lk));
    const thx::Plans& pl = pe->p;
    THX_CHECK_ARG(method != 2 || pl.cols, "thx_postprocess: no column passes for N=%d", N);
    THX_CHECK_ARG(pl.work <= thx::fft_reserve(N), "thx_postprocess: hipFFT's work area exceeds the reserve");
    THX_RET(thx::bind_plans(pl, work, s));
    const size_t n3 = (size_t)N * N * N;
    const float scale = 1.f / ((float)N * (float)N * (float)N);
    for (int pass = 0; pass < (average ? 2 : 1); pass++) {      // 0: sharp, 1: the plain average
        StreamArgs a{};
        a.A = A2;
        a.B = B2;
        a.dst = C;
        a.N = N;
        if (pass == 0) {
            a.fsc = fsc;
            a.nShell = nShell;
            a.bDev = fit;
            a.thresDev = info + 1;
            a.ew = edgeFT / (float)N;
            a.lowPass = a.ew > 0.f;
        }
        THX_RET(launch_stream(a, s));
        THX_RET(thx::hermitian_planes(C, N, s));
        float* rl = pass == 0 ? sharp : average;
        THX_RET(thx::c2r3d(pl, C, rl, N, s, method));
        THX_LAUNCH(k_pp_scale_mask, dim3(stream_blocks(n3 / 4)), dim3(PP_THREADS), 0, s, rl,
                   pass == 0 ? alphaMask : nullptr, n3 / 4, scale);
    }
    return THX_OK;
}
