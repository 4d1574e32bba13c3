// refresh.hip -- the last stage of a round: the reconstructed reference of
// box N becomes the next round's projectee of box vdim = pf N, on device.
//
//   thx_ref_average: Model::compareTwoHemispheres' averaging
//             (src/Model.cpp:611-690): below the shell radius r both half
//             maps become (A + B) / 2 (QUAD_3(i, j, k) < r^2, :660-669; 2D
//             QUAD(i, j) < r^2, :647-656; everything for K > 1, :683-689),
//             then lowPassFilter (src/Functions/Filter.cpp:46-92) with
//             f = |(i, j, k)| / N: kept below thres, 0 above thres + ew,
//             times cos((f - thres) pi / ew) / 2 + 1 / 2 between (off in the
//             reference: OPTIMISER_SOLVENT_FLATTEN_LOW_PASS is not compiled
//             in, include/Config.h:173-181).
//   thx_projectee: Optimiser::solventFlatten (src/Optimiser.cpp:7768-7989,
//             OPTIMISER_SOLVENT_FLATTEN_MASK_ZERO: softMask with bg = 0,
//             src/Functions/Mask.cpp:499-521, or dst = src (1 - (1 - alpha)),
//             :533-544) followed by Model::refreshProj -> Projector::
//             setProjectee (src/Model.cpp:1013-1044, src/Projector.cpp:97-148):
//             VOL_PAD_RL (include/Image/ImageFunctions.h:176-192: voxel
//             (i, j, k), i, j, k in [-N/2, N/2), keeps its signed coordinate
//             in the pf N box), gridCorrection (src/Projector.cpp:524-606:
//             divided by TIK_RL(|r| / (pf nColRL)) with nColRL the PADDED box,
//             NIK_RL for nearest-neighbour interpolation), FFT::fw
//             (unnormalised).  The fw / bw pairs between those steps cancel
//             (bw divides by the size, fw does not), so what runs is at most
//             one inverse transform at N (Fourier-space input only) and one
//             forward transform at pf N.
//
// The forward transform has two forms with one results contract:
//   fallback: one fused kernel writes mask x correction x scale into the
//             padded real volume, then hipFFT's 3D R2C plan (any even box);
//   pruned:   (power-of-two vdim, 16 .. 512) the padded volume is zero outside
//             the wrapped central N^3 box, so it is never written and no
//             all-zero line is transformed.  Three passes of wave FFTs in LDS
//             (fft_lds.h):
//               x: the N^2 non-zero rows, two real rows per complex FFT
//                  (z = a + i b, A(k) = (Z(k) + conj Z(-k)) / 2, B(k) =
//                  (Z(k) - conj Z(-k)) / 2i), mask, correction and scale
//                  applied while loading        -> X [N][N][H], H = vdim/2+1
//               y: N slices, N rows in, vdim out -> Y [N][vdim][H]
//               z: every column, N rows in       -> dst [vdim][vdim][H]
//   No atomics; every output element is written by one thread from a fixed
//   butterfly order, so results are bit-identical from run to run.  Nothing
//   on this path waits for the device.
// Layouts: real-space maps [k][j][i] with the origin at index 0 and negative
// coordinates wrapped (Volume RL, thx_reconstruct's dst); Fourier maps
// half-complex [k][j][i <= box/2] (Volume FT = hipFFT's R2C layout).
#include <cmath>

#include "common.h"
#include "fft_lds.h"
#include "fft_plans.h"
#include "volume.h"

namespace {

constexpr int RF_CT = 16;       // columns per tile of the column passes
constexpr int RF_WAVES = 4;
constexpr int RF_THREADS = 64 * RF_WAVES;
constexpr int RF_RSTEP = RF_THREADS / RF_CT;

// 1 / TIK_RL(u / pv) (interp 0) or 1 / NIK_RL(u / pv) (interp 1), pv = pf vdim
THX_DEV float grid_corr(float u, float pv, int interp)
{
    const float x = (float)M_PI * (u / pv);
    const float j0 = x == 0.f ? 1.f : sinf(x) / x;
    return interp ? 1.f / j0 : 1.f / (j0 * j0);
}

// One voxel of the masked, corrected source: (i, j, k) signed, v its value,
// al its alpha (used when hasAlpha).  The same expression on both paths.
THX_DEV float refresh_value(float v, int i, int j, int k, float rMask, float edge, bool hasAlpha,
                            float al, float pv, int interp, float scale)
{
    const float u = sqrtf((float)(i * i + j * j + k * k));
    if (hasAlpha) v = v * (1.f - (1.f - al));
    else if (rMask > 0.f) v = v * soft_mask(u, rMask, edge);
    return v * grid_corr(u, pv, interp) * scale;
}

// ------------------------------------------------------- Fourier-side kernel
// One thread per stored voxel of nK maps [N][N][N/2+1] (mode3d) or images
// [N][N/2+1]; A, B in place; B may be NULL (no averaging).
__global__ void k_ref_average(float2* __restrict__ A, float2* __restrict__ B, int N, long per, long n,
                              float r, float thres, float ew, int mode3d)
{
    const long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const int nc = N / 2 + 1;
    const long e = q % per;
    const int i = (int)(e % nc);
    const long rest = e / nc;
    const int j = signed_idx((int)(rest % N), N);
    const int k = mode3d ? signed_idx((int)(rest / N), N) : 0;
    const int quad = i * i + j * j + k * k;
    float2 a = A[q];
    float2 b = B ? B[q] : a;
    if (B && (r < 0.f || (float)quad < r * r)) {
        a = make_float2((a.x + b.x) / 2.f, (a.y + b.y) / 2.f);
        b = a;
    }
    if (thres > 0.f) {
        const float fi = (float)i / (float)N, fj = (float)j / (float)N, fk = (float)k / (float)N;
        const float f = sqrtf(fi * fi + fj * fj + fk * fk);
        float m = 1.f;
        if (f < thres) m = 1.f;
        else if (f > thres + ew) m = 0.f;
        else m = cosf((f - thres) * (float)M_PI / ew) / 2.f + 0.5f;
        a = make_float2(a.x * m, a.y * m);
        b = make_float2(b.x * m, b.y * m);
    }
    A[q] = a;
    if (B) B[q] = b;
}

// ------------------------------------------------------------ fallback pads
// pad[vdim^3] (3D): the masked, corrected source at its signed coordinate, 0
// elsewhere.  Block (64, 4): x fastest, blockIdx.y over row groups, .z = slice.
__global__ void k_pad3(float* __restrict__ pad, const float* __restrict__ src,
                       const float* __restrict__ alpha, int N, int vdim, float rMask, float edge,
                       float pv, int interp, float scale)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, z = blockIdx.z;
    if (x >= vdim || y >= vdim) return;
    const int i = signed_idx(x, vdim), j = signed_idx(y, vdim), k = signed_idx(z, vdim);
    const int h = N / 2;
    float v = 0.f;
    if (i >= -h && i < h && j >= -h && j < h && k >= -h && k < h) {
        const size_t e = ((size_t)wrap_idx(k, N) * N + wrap_idx(j, N)) * N + wrap_idx(i, N);
        v = refresh_value(src[e], i, j, k, rMask, edge, alpha != nullptr, alpha ? alpha[e] : 0.f, pv,
                          interp, scale);
    }
    pad[((size_t)z * vdim + y) * vdim + x] = v;
}

// pad[nK][vdim^2] (2D, blockIdx.z = class): radial mask over |(i, j)|,
// correction |(i, j)| / (pf vdim)
__global__ void k_pad2(float* __restrict__ pad, const float* __restrict__ src, int N, int vdim,
                       float rMask, float edge, float pv, int interp, float scale)
{
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y, c = blockIdx.z;
    if (x >= vdim || y >= vdim) return;
    const int i = signed_idx(x, vdim), j = signed_idx(y, vdim);
    const int h = N / 2;
    float v = 0.f;
    if (i >= -h && i < h && j >= -h && j < h) {
        const size_t e = ((size_t)c * N + wrap_idx(j, N)) * N + wrap_idx(i, N);
        v = refresh_value(src[e], i, j, 0, rMask, edge, false, 0.f, pv, interp, scale);
    }
    pad[((size_t)c * vdim + y) * vdim + x] = v;
}

// ------------------------------------------------------------ pruned passes
// compact index of padded index p of a length-V line whose non-zero part is
// the wrapped central N: -1 where the line is zero
THX_DEV int compact_idx(int p, int N, int V)
{
    if (p < N / 2) return p;
    if (p >= V - N / 2) return p - (V - N);
    return -1;
}

template <int V>
constexpr size_t rf_row_lds() { return (size_t)(RF_WAVES * thx::fft_pitch<V>() + V) * sizeof(float2); }

template <int V>
constexpr size_t rf_col_lds() { return (size_t)(RF_CT * thx::fft_pitch<V>() + V) * sizeof(float2); }

template <int V>
THX_DEV const float2* rf_twiddles(float2* sTw, const float2* __restrict__ tw)
{
    for (int q = threadIdx.x; q < V; q += blockDim.x) sTw[q] = tw[q];
    return sTw;
}

// x pass: a wave takes the row pair (2 p, 2 p + 1) of the N^2 rows (zc, yc)
// of the source, X [row][H].
template <int V>
__global__ void __launch_bounds__(RF_THREADS) k_prune_x(float2* __restrict__ X,
                                                        const float* __restrict__ src,
                                                        const float* __restrict__ alpha, int N,
                                                        float rMask, float edge, float pv, int interp,
                                                        float scale, const float2* __restrict__ tw)
{
    extern __shared__ float2 sm[];
    constexpr int H = V / 2 + 1, P = thx::fft_pitch<V>();
    constexpr int NX = (V + 63) / 64, NH = (H + 63) / 64;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float2* stw = rf_twiddles<V>(sm + RF_WAVES * P, tw);
    __syncthreads();
    const long pair = (long)blockIdx.x * RF_WAVES + wv;
    if (pair >= (long)N * N / 2) return;
    float2* buf = sm + wv * P;
    const long row0 = 2 * pair;                     // N even: both rows in one slice
    const int zc = (int)(row0 / N), yc = (int)(row0 % N);
    const int k = signed_idx(zc, N), j0 = signed_idx(yc, N), j1 = signed_idx(yc + 1, N);
    const float* s0 = src + row0 * N;
    const float* a0 = alpha ? alpha + row0 * N : nullptr;
#pragma unroll
    for (int t = 0; t < NX; t++) {
        const int x = lane + 64 * t;
        if (x < V) {
            const int xc = compact_idx(x, N, V);
            float2 v = make_float2(0.f, 0.f);
            if (xc >= 0) {
                const int i = signed_idx(xc, N);
                v.x = refresh_value(s0[xc], i, j0, k, rMask, edge, alpha != nullptr,
                                    a0 ? a0[xc] : 0.f, pv, interp, scale);
                v.y = refresh_value(s0[N + xc], i, j1, k, rMask, edge, alpha != nullptr,
                                    a0 ? a0[N + xc] : 0.f, pv, interp, scale);
            }
            buf[thx::fft_slot<V>(x, 0)] = v;
        }
    }
    thx::wave_lds_sync();
    thx::wave_fft<V>(buf, 0, stw, -1.f, lane);
    float2* o0 = X + row0 * H;
    float2* o1 = o0 + H;
#pragma unroll
    for (int t = 0; t < NH; t++) {
        const int x = lane + 64 * t;
        if (x < H) {
            const float2 zk = buf[thx::fft_slot<V>(x, 0)];
            const float2 zm = buf[thx::fft_slot<V>(V - x, 0)];     // slot wraps V to 0
            o0[x] = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
            o1[x] = make_float2(0.5f * (zk.y + zm.y), 0.5f * (zm.x - zk.x));
        }
    }
}

// Column pass: a block takes a tile of RF_CT kx columns of one outer index
// (y pass: the slice zc; z pass: the row ky).  The NIN compact input rows go
// to their padded positions of a length-V column, the rest is zero; C2C
// forward; V rows out.
//   in  element (outer, r, kx): in  + outer * inOuter  + r * inRow  + kx
//   out element (outer, p, kx): out + outer * outOuter + p * outRow + kx
template <int V>
__global__ void __launch_bounds__(RF_THREADS) k_prune_col(float2* __restrict__ out,
                                                          const float2* __restrict__ in, int N,
                                                          int nOuter, long inOuter, long inRow, long outOuter,
                                                          long outRow, const float2* __restrict__ tw)
{
    extern __shared__ float2 sm[];
    constexpr int H = V / 2 + 1, P = thx::fft_pitch<V>(), NT = (H + RF_CT - 1) / RF_CT;
    constexpr int NR = V / RF_RSTEP;
    const int t = thx::xcd_tile(NT * nOuter);           // kx-neighbouring tiles on one XCD
    if (t < 0) return;
    float2* tile = sm;                                  // [RF_CT][P], column c rotated by c
    const float2* stw = rf_twiddles<V>(sm + RF_CT * P, tw);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int kx0 = (t % NT) * RF_CT, outer = t / NT;
    const int ncol = min(RF_CT, H - kx0);
    const int c = tid % RF_CT, rr = tid / RF_CT;
    const bool on = c < ncol;
    const float2* ibase = in + (size_t)outer * inOuter + kx0 + c;
    float2* obase = out + (size_t)outer * outOuter + kx0 + c;
    float2* col = tile + c * P;
    float2 v[NR];
#pragma unroll
    for (int i = 0; i < NR; i++) {
        const int rc = compact_idx(rr + i * RF_RSTEP, N, V);
        v[i] = on && rc >= 0 ? ibase[(size_t)rc * inRow] : make_float2(0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < NR; i++) col[thx::fft_slot<V>(rr + i * RF_RSTEP, c)] = v[i];
    __syncthreads();
    for (int cc = wv; cc < ncol; cc += RF_WAVES) thx::wave_fft<V>(tile + cc * P, cc, stw, -1.f, lane);
    __syncthreads();
    if (on) {
#pragma unroll
        for (int i = 0; i < NR; i++)
            obase[(size_t)(rr + i * RF_RSTEP) * outRow] = col[thx::fft_slot<V>(rr + i * RF_RSTEP, c)];
    }
}

template <int V>
int pruned_n(const float* src, const float* alpha, int N, float rMask, float edge, float pv,
             int interp, float scale, float2* X, float2* Y, float2* dst, const float2* tw,
             hipStream_t s)
{
    constexpr int H = V / 2 + 1, NT = (H + RF_CT - 1) / RF_CT;
    constexpr size_t lr = rf_row_lds<V>(), lc = rf_col_lds<V>();
    static std::atomic<unsigned> set[2];
    THX_RET(thx::set_max_lds(reinterpret_cast<const void*>(k_prune_x<V>), (int)lr, set[0]));
    THX_RET(thx::set_max_lds(reinterpret_cast<const void*>(k_prune_col<V>), (int)lc, set[1]));
    const dim3 b(RF_THREADS);
    const long pairs = (long)N * N / 2;
    hipLaunchKernelGGL((k_prune_x<V>), dim3(thx::cdiv(pairs, RF_WAVES)), b, lr, s, X, src, alpha, N,
                       rMask, edge, pv, interp, scale, tw);
    THX_LAUNCH_CHECK();
    // y: X [zc][yc][kx] -> Y [zc][ky][kx]
    hipLaunchKernelGGL((k_prune_col<V>), dim3((NT * N + 7) / 8 * 8), b, lc, s, Y, X, N, N, (long)N * H, (long)H,
                       (long)V * H, (long)H, tw);
    THX_LAUNCH_CHECK();
    // z: Y [zc][ky][kx] -> dst [kz][ky][kx]
    hipLaunchKernelGGL((k_prune_col<V>), dim3((NT * V + 7) / 8 * 8), b, lc, s, dst, Y, N, V, (long)H, (long)V * H,
                       (long)H, (long)V * H, tw);
    THX_LAUNCH_CHECK();
    return THX_OK;
}

bool pruned_ok(int vdim) { return vdim >= 16 && vdim <= 512 && (vdim & (vdim - 1)) == 0; }

// method 0's route on the boxes both paths serve (DESIGN.md 4b has the
// measurement behind it)
constexpr bool AUTO_PRUNED = true;

bool route_pruned(int vdim, int method) { return method == 2 || (method == 0 && AUTO_PRUNED && pruned_ok(vdim)); }

struct Carved {
    float2* ftCopy = nullptr;   // fromFT: the C2R's input (hipFFT overwrites it)
    float* rl = nullptr;        // fromFT: the real-space map
    char* workN = nullptr;
    float* pad = nullptr;       // fallback
    char* workV = nullptr;
    float2* X = nullptr;        // pruned
    float2* Y = nullptr;
    size_t bytes = 0;
};

Carved carve(void* ws, size_t cap, int N, int pf, bool pruned, bool fromFT)
{
    const int vdim = N * pf;
    const size_t H = vdim / 2 + 1;
    thx::Carver k(ws, cap);
    Carved c;
    if (fromFT) {
        c.ftCopy = k.take<float2>(thx::ft_elems(N));
        c.rl = k.take<float>((size_t)N * N * N);
        c.workN = k.take<char>(thx::fft_reserve(N));
    }
    if (pruned) {
        c.X = k.take<float2>((size_t)N * N * H);
        c.Y = k.take<float2>((size_t)N * vdim * H);
    } else {
        c.pad = k.take<float>((size_t)vdim * vdim * vdim);
        c.workV = k.take<char>(thx::fft_reserve(vdim));
    }
    c.bytes = k.off + 256;
    return c;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb)
{
    const char* x = static_cast<const char*>(a);
    const char* y = static_cast<const char*>(b);
    return x < y + nb && y < x + na;
}

bool shape_ok(int N, int pf) { return N >= 8 && N % 2 == 0 && pf >= 1 && (long)N * pf <= 2048; }

}  // namespace

extern "C" int thx_ref_average(float* A, float* B, int N, int nK, float r, float thres, float ew,
                               int mode3d, thx_stream_t stream)
{
    THX_CHECK_ARG(A && N >= 8 && N % 2 == 0 && N <= 2048 && nK > 0, "thx_ref_average: bad arguments");
    THX_CHECK_ARG(A != B, "thx_ref_average: A and B are the same map");
    THX_CHECK_ARG(std::isfinite(r) && std::isfinite(thres), "thx_ref_average: r / thres not finite");
    THX_CHECK_ARG(!(thres > 0.f) || (std::isfinite(ew) && ew > 0.f),
                  "thx_ref_average: the low-pass needs a finite ew > 0");
    const long per = mode3d ? (long)thx::ft_elems(N) : (long)N * (N / 2 + 1);
    const long n = per * nK;
    hipLaunchKernelGGL(k_ref_average, dim3(thx::cdiv(n, 256)), dim3(256), 0, thx::as_stream(stream),
                       reinterpret_cast<float2*>(A), reinterpret_cast<float2*>(B), N, per, n, r, thres,
                       ew, mode3d);
    THX_LAUNCH_CHECK();
    return THX_OK;
}

extern "C" size_t thx_projectee_workspace(int N, int pf, int method, int fromFT)
{
    if (!shape_ok(N, pf) || method < 0 || method > 2) return 0;
    if (method == 2 && !pruned_ok(N * pf)) return 0;
    return carve(nullptr, ~size_t(0), N, pf, route_pruned(N * pf, method), fromFT != 0).bytes;
}

extern "C" int thx_projectee(const float* src, int fromFT, int N, int pf, float rMask, float edge,
                             const float* alphaMask, int interp, float scale, float* dst, int method,
                             void* workspace, size_t wsBytes, thx_stream_t stream)
{
    THX_CHECK_ARG(src && dst, "thx_projectee: src / dst is NULL");
    THX_CHECK_ARG(shape_ok(N, pf), "thx_projectee: N must be even and >= 8, pf >= 1");
    THX_CHECK_ARG(method >= 0 && method <= 2, "thx_projectee: method is 0, 1 or 2");
    THX_CHECK_ARG(interp == 0 || interp == 1, "thx_projectee: interp is 0 (linear) or 1 (nearest)");
    THX_CHECK_ARG(std::isfinite(scale) && std::isfinite(rMask), "thx_projectee: scale / rMask not finite");
    const bool radial = rMask > 0.f;
    THX_CHECK_ARG(!(radial && alphaMask), "thx_projectee: rMask and alphaMask are exclusive");
    THX_CHECK_ARG(!radial || (std::isfinite(edge) && edge > 0.f),
                  "thx_projectee: the radial mask needs a finite edge > 0");
    const int vdim = N * pf;
    THX_CHECK_ARG(method != 2 || pruned_ok(vdim),
                  "thx_projectee: the pruned path needs a power-of-two pf N in [16, 512]");
    const bool pruned = route_pruned(vdim, method);
    const Carved c = carve(workspace, wsBytes, N, pf, pruned, fromFT != 0);
    THX_CHECK_ARG(workspace && wsBytes >= c.bytes, "thx_projectee: workspace too small");
    const size_t srcBytes = fromFT ? thx::ft_elems(N) * sizeof(float2) : sizeof(float) * N * N * N;
    const size_t dstBytes = thx::ft_elems(vdim) * sizeof(float2);
    THX_CHECK_ARG(!overlaps(dst, dstBytes, src, srcBytes), "thx_projectee: dst aliases src");
    THX_CHECK_ARG(!overlaps(dst, dstBytes, workspace, wsBytes), "thx_projectee: dst aliases the workspace");
    THX_CHECK_ARG(!alphaMask || !overlaps(dst, dstBytes, alphaMask, sizeof(float) * N * N * N),
                  "thx_projectee: dst aliases alphaMask");
    hipStream_t s = thx::as_stream(stream);
    const float pv = (float)pf * (float)vdim;
    const float* rl = src;
    if (fromFT) {
        // FFT::bw of the reference box: C2R, then 1 / N^3 (folded into scale)
        std::unique_lock<std::mutex> lk;
        thx::PlanEntry* pe = nullptr;
        THX_RET(thx::cached_plans(N, N / 2, s, &pe, lk));
        THX_CHECK_ARG(pe->p.work <= thx::fft_reserve(N), "thx_projectee: hipFFT's work area exceeds the reserve");
        THX_RET(thx::bind_plans(pe->p, c.workN, s));
        THX_HIP(hipMemcpyAsync(c.ftCopy, src, srcBytes, hipMemcpyDeviceToDevice, s));
        THX_RET(thx::c2r3d(pe->p, c.ftCopy, c.rl, N, s, 1));
        rl = c.rl;
        scale = scale / ((float)N * (float)N * (float)N);
    }
    std::unique_lock<std::mutex> lk;
    thx::PlanEntry* pe = nullptr;
    THX_RET(thx::cached_plans(vdim, N, s, &pe, lk));
    float2* out = reinterpret_cast<float2*>(dst);
    if (pruned) {
        const float2* tw = pe->p.tw;
        THX_CHECK_ARG(tw, "thx_projectee: no twiddle table for this box");
#define THX_PRUNED(V) \
    case V: return pruned_n<V>(rl, alphaMask, N, rMask, edge, pv, interp, scale, c.X, c.Y, out, tw, s)
        switch (vdim) {
            THX_PRUNED(16);
            THX_PRUNED(32);
            THX_PRUNED(64);
            THX_PRUNED(128);
            THX_PRUNED(256);
            THX_PRUNED(512);
            default: thx::set_error("thx_projectee: unsupported pruned box %d", vdim); return THX_ERR_ARG;
        }
#undef THX_PRUNED
    }
    THX_CHECK_ARG(pe->p.work <= thx::fft_reserve(vdim), "thx_projectee: hipFFT's work area exceeds the reserve");
    THX_RET(thx::bind_plans(pe->p, c.workV, s));
    hipLaunchKernelGGL(k_pad3, dim3(thx::cdiv(vdim, 64), thx::cdiv(vdim, 4), vdim), dim3(64, 4), 0, s, c.pad, rl, alphaMask, N, vdim,
                       rMask, edge, pv, interp, scale);
    THX_LAUNCH_CHECK();
    return thx::r2c3d(pe->p, c.pad, out, vdim, s, 1);
}

extern "C" size_t thx_projectee2d_workspace(int N, int pf, int nK, int fromFT)
{
    if (!shape_ok(N, pf) || nK <= 0) return 0;
    const int vdim = N * pf;
    thx::Carver k(nullptr, ~size_t(0));
    if (fromFT) {
        k.take<float2>((size_t)nK * N * (N / 2 + 1));
        k.take<float>((size_t)nK * N * N);
    }
    k.take<float>((size_t)nK * vdim * vdim);
    return k.off + 256;
}

extern "C" int thx_projectee2d(const float* src, int fromFT, int nK, int N, int pf, float rMask,
                               float edge, const float* alphaMask, int interp, float scale, float* dst,
                               void* workspace, size_t wsBytes, thx_stream_t stream)
{
    THX_CHECK_ARG(src && dst && nK > 0, "thx_projectee2d: bad arguments");
    THX_CHECK_ARG(shape_ok(N, pf), "thx_projectee2d: N must be even and >= 8, pf >= 1");
    // the reference aborts on a provided mask in MODE_2D (src/Optimiser.cpp:7933-7957)
    THX_CHECK_ARG(!alphaMask, "thx_projectee2d: a provided mask is 3D only");
    THX_CHECK_ARG(interp == 0 || interp == 1, "thx_projectee2d: interp is 0 (linear) or 1 (nearest)");
    THX_CHECK_ARG(std::isfinite(scale) && std::isfinite(rMask), "thx_projectee2d: scale / rMask not finite");
    THX_CHECK_ARG(!(rMask > 0.f) || (std::isfinite(edge) && edge > 0.f),
                  "thx_projectee2d: the radial mask needs a finite edge > 0");
    const size_t need = thx_projectee2d_workspace(N, pf, nK, fromFT);
    THX_CHECK_ARG(workspace && wsBytes >= need, "thx_projectee2d: workspace too small");
    const int vdim = N * pf;
    const size_t srcBytes = (fromFT ? sizeof(float2) * N * (N / 2 + 1) : sizeof(float) * N * N) * nK;
    const size_t dstBytes = sizeof(float2) * nK * vdim * (vdim / 2 + 1);
    THX_CHECK_ARG(!overlaps(dst, dstBytes, src, srcBytes), "thx_projectee2d: dst aliases src");
    THX_CHECK_ARG(!overlaps(dst, dstBytes, workspace, wsBytes), "thx_projectee2d: dst aliases the workspace");
    hipStream_t s = thx::as_stream(stream);
    thx::Carver k(workspace, wsBytes);
    const float* rl = src;
    if (fromFT) {
        float2* ftCopy = k.take<float2>((size_t)nK * N * (N / 2 + 1));
        float* r = k.take<float>((size_t)nK * N * N);
        std::unique_lock<std::mutex> lk;
        thx::Plans2* pl = nullptr;
        THX_RET(thx::plans2d(N, nK, s, &pl, lk));
        THX_HIP(hipMemcpyAsync(ftCopy, src, srcBytes, hipMemcpyDeviceToDevice, s));
        THX_FFT(hipfftExecC2R(pl->c2r, reinterpret_cast<hipfftComplex*>(ftCopy), r));
        rl = r;
        scale = scale / ((float)N * (float)N);
    }
    float* pad = k.take<float>((size_t)nK * vdim * vdim);
    hipLaunchKernelGGL(k_pad2, dim3(thx::cdiv(vdim, 64), thx::cdiv(vdim, 4), nK), dim3(64, 4), 0, s, pad,
                       rl, N, vdim, rMask, edge, (float)pf * (float)vdim, interp, scale);
    THX_LAUNCH_CHECK();
    std::unique_lock<std::mutex> lk;
    thx::Plans2* pl = nullptr;
    THX_RET(thx::plans2d(vdim, nK, s, &pl, lk));
    THX_FFT(hipfftExecR2C(pl->r2c, pad, reinterpret_cast<hipfftComplex*>(dst)));
    return THX_OK;
}
