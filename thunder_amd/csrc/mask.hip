// mask.hip -- mask generation on device: genMask / removeIsolatedPoint /
// extMask / softEdge (src/Functions/Mask.cpp:581-731) with the corner removal
// of thunder_genmask (appsrc/thunder_genmask.cpp:156-159).  autoMask's
// threshold search (:733-791) is not here.
//
//   threshold: mask = src > thres ? 1 : 0 (:699-704), a voxel with
//             i^2 + j^2 + k^2 >= (N/2)^2 counting as 0 first (removeCorners),
//             then removeIsolatedPoint (:581-610): a 1-voxel none of whose six
//             face neighbours inside the box is 1 becomes 0, judged on the
//             thresholded map (the reference's copy), not in place.
//   extend:   extMask (:612-640).  ext > 0: 1 wherever a 1-voxel lies at an
//             integer offset d with QUAD_3(d) < pow_2(ext); ext < 0: 0 wherever
//             a 0-voxel inside the box lies that close; other voxels keep their
//             value.  The reference scatters over the grid [-a, a)^3, a =
//             ceil|ext|; the offset -a never passes the strict test (a^2 >=
//             ext^2), so the footprint is the open ball and the gather over it
//             gives the same map.
//   soft edge: softEdge (:642-692).  d = the smallest NORM_3(d) < ew to a
//             1-voxel; a voxel with 0 < d < ew becomes 0.5 + 0.5 cos(d / ew pi),
//             the others keep their value.  d is the FP32 value of
//             sqrt(integer |d|^2) (the reference rounds gsl_hypot3 to RFLOAT),
//             so the minimum over integer |d|^2 is exact.
//   box faces: nothing wraps and nothing is written outside the box.  The
//             reference indexes linearly with its bounds checks compiled out
//             (IMG_VOL_BOUNDARY_NO_CHECK), so a footprint that crosses a face
//             writes into a neighbouring row or outside the array there; that
//             is an out-of-row write, not behaviour to reproduce.
//
// Maps are real [N][N][N], origin at index 0, negatives wrapped.  The two tests
// against ext^2 and ew are made once on the host, in the reference's types,
// into an integer limit L (|d|^2 < L passes): the device compares integers.
//
// No (2a+1)^3 taps: the binary predicate (== 1, or == 0 for the erosion) is
// packed to bits along x in CENTRED order (bit p of a row is i = p - N/2, so a
// row is one contiguous run and a face is the end of the row), one 64-bit word
// per wave through __ballot.  An output wave owns 64 x of one row; for every
// (dy, dz) with dy^2 + dz^2 < L it takes the three words around its own from
// LDS (a tile of 8 x 8 rows plus halo is staged once per block), forms the
// 64-bit window centred on its voxel and finds the nearest set bit within the
// x half-width hx (the largest with hx^2 + dy^2 + dz^2 < L; hx <= 31, tabulated
// per (dy, dz) in LDS) with one count-trailing-zeros and one count-leading-zeros.  About pi L row lookups per
// voxel; rows whose three words are empty are skipped wave-wide.  No atomics,
// no host synchronisation; every voxel is written by one thread from integer
// arithmetic, so results are bit-identical from run to run.
#include <cmath>

#include "common.h"
#include "volume.h"

namespace {

constexpr int MK_THREADS = 256;
constexpr int MK_WAVES = MK_THREADS / 64;
constexpr int MK_T = 8;                 // rows per tile edge (y and z)
constexpr int MK_LIMIT = 32;            // |ext|, ew at most
constexpr int MK_FAR = 1 << 30;

enum { MK_EXTEND = 0, MK_ERODE = 1, MK_SOFT = 2 };

int row_words(int N) { return (N + 63) / 64; }
size_t bits_bytes(int N) { return (size_t)N * N * row_words(N) * sizeof(uint64_t); }

// stored index of a centred coordinate p = i + N/2 (N even)
THX_DEV int stored_idx(int p, int N) { return p < N / 2 ? p + N / 2 : p - N / 2; }

// One wave per word: lane l is centred x = 64 w + l of centred row (yc, zc).
template <int ONES>
__global__ void __launch_bounds__(MK_THREADS) k_mask_pack(const float* __restrict__ src, int N,
                                                          int W, uint64_t* __restrict__ bits)
{
    const long total = (long)N * N * W;
    const long g = (long)blockIdx.x * MK_WAVES + (threadIdx.x >> 6);
    if (g >= total) return;
    const int lane = threadIdx.x & 63;
    const int w = (int)(g % W);
    const long row = g / W;
    const int yc = (int)(row % N), zc = (int)(row / N);
    const int xc = w * 64 + lane;
    bool on = false;
    if (xc < N) {
        const float v = src[((size_t)stored_idx(zc, N) * N + stored_idx(yc, N)) * N +
                            stored_idx(xc, N)];
        on = ONES ? v == 1.f : v == 0.f;
    }
    const uint64_t word = __ballot(on);
    if (lane == 0) bits[g] = word;
}

// dst = the thresholded map without its isolated points.  One thread per voxel
// in storage order; the six neighbours are thresholded again from src.
__global__ void __launch_bounds__(MK_THREADS) k_mask_threshold(const float* __restrict__ src, int N,
                                                               float thres, int removeCorners,
                                                               float* __restrict__ dst)
{
    const size_t n3 = (size_t)N * N * N;
    const size_t q = blockIdx.x * (size_t)MK_THREADS + threadIdx.x;
    if (q >= n3) return;
    const int h = N / 2;
    const int ii = (int)(q % N), jj = (int)(q / N % N), kk = (int)(q / ((size_t)N * N));
    const int i = ii < h ? ii : ii - N, j = jj < h ? jj : jj - N, k = kk < h ? kk : kk - N;
    auto on = [&](int a, int b, int c) {
        if (a < -h || a >= h || b < -h || b >= h || c < -h || c >= h) return false;
        // a corner voxel is set to 0 before the comparison (it passes a negative thres)
        if (removeCorners && a * a + b * b + c * c >= h * h) return 0.f > thres;
        return src[((size_t)wrap_idx(c, N) * N + wrap_idx(b, N)) * N + wrap_idx(a, N)] > thres;
    };
    float m = 0.f;
    if (on(i, j, k) && (on(i - 1, j, k) || on(i, j - 1, k) || on(i, j, k - 1) || on(i + 1, j, k) ||
                        on(i, j + 1, k) || on(i, j, k + 1)))
        m = 1.f;
    dst[q] = m;
}

// Block (w, ty, tz): the 64 x of word w of the MK_T x MK_T centred rows from
// (ty MK_T, tz MK_T).  am: the largest offset with am^2 < lim2 (the halo).
// sRow[(rz RY + ry) * 3 + c] = word w - 1 + c of centred row (y0 - am + ry,
// z0 - am + rz), 0 outside the box.
template <int MODE>
__global__ void __launch_bounds__(MK_THREADS) k_mask_ball(const float* __restrict__ src,
                                                          float* __restrict__ dst,
                                                          const uint64_t* __restrict__ bits, int N,
                                                          int W, int am, int lim2, float ew)
{
    extern __shared__ uint64_t sRow[];
    const int w = blockIdx.x, y0 = blockIdx.y * MK_T, z0 = blockIdx.z * MK_T;
    const int RY = MK_T + 2 * am;
    const int nWord = RY * RY * 3;
    for (int e = threadIdx.x; e < nWord; e += MK_THREADS) {
        const int c = e % 3, r = e / 3;
        const int yc = y0 - am + r % RY, zc = z0 - am + r / RY, ww = w - 1 + c;
        uint64_t v = 0;
        if (yc >= 0 && yc < N && zc >= 0 && zc < N && ww >= 0 && ww < W)
            v = bits[((size_t)zc * N + yc) * W + ww];
        sRow[e] = v;
    }
    // sHx[(dz + am) D + dy + am] = the largest hx with hx^2 < lim2 - dz^2 - dy^2 (at most
    // 1024: exact in FP32), -1 outside the disc
    const int D = 2 * am + 1;
    signed char* sHx = reinterpret_cast<signed char*>(sRow + nWord);
    for (int e = threadIdx.x; e < D * D; e += MK_THREADS) {
        const int dz = e / D - am, dy = e % D - am;
        const int rem = lim2 - dz * dz - dy * dy;
        sHx[e] = rem > 0 ? (signed char)((int)ceilf(sqrtf((float)rem)) - 1) : (signed char)-1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int xc = w * 64 + lane;
    const bool valid = xc < N;
    // the window of bits [x - 32, x + 31] starts at bit 32 + lane of (w-1, w) for
    // lane < 32, at bit lane - 32 of (w, w+1) otherwise; bit 32 of it is x
    const bool low = lane < 32;
    const int sh = (32 + lane) & 63;
    for (int t = wv; t < MK_T * MK_T; t += MK_WAVES) {
        const int ty = t % MK_T, tz = t / MK_T;
        const int yc = y0 + ty, zc = z0 + tz;
        if (yc >= N || zc >= N) continue;
        int best = MK_FAR;
        for (int dz = -am; dz <= am; dz++) {
            if (zc + dz < 0 || zc + dz >= N) continue;
            if (MODE != MK_SOFT && __all(best != MK_FAR || !valid)) break;
            const signed char* hxOf = sHx + (dz + am) * D + am;
            for (int dy = -am; dy <= am; dy++) {
                const int hx = hxOf[dy];
                if (hx < 0 || yc + dy < 0 || yc + dy >= N) continue;
                const uint64_t* row = sRow + ((tz + am + dz) * RY + (ty + am + dy)) * 3;
                const uint64_t A = row[0], B = row[1], C = row[2];
                if ((A | B | C) == 0) continue;
                const uint64_t lo = low ? A : B, hi = low ? B : C;
                const uint64_t win = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
                const unsigned right = (unsigned)(win >> 32) & ((2u << hx) - 1u);   // bit b: dx = b
                const unsigned left = hx ? (unsigned)win >> (32 - hx) : 0u;   // bit hx - 1: dx = -1
                int dx = MK_FAR;
                if (right) dx = __builtin_ctz(right);
                if (left) {
                    const int dl = hx - (31 - __builtin_clz(left));
                    dx = dl < dx ? dl : dx;
                }
                if (dx != MK_FAR) {
                    const int d2 = dx * dx + dy * dy + dz * dz;
                    best = d2 < best ? d2 : best;
                }
            }
        }
        if (!valid) continue;
        const size_t at = ((size_t)stored_idx(zc, N) * N + stored_idx(yc, N)) * N + stored_idx(xc, N);
        float v = src[at];
        if (MODE == MK_EXTEND) {
            if (best != MK_FAR) v = 1.f;
        } else if (MODE == MK_ERODE) {
            if (best != MK_FAR) v = 0.f;
        } else if (best != MK_FAR && best > 0) {
            const float d = (float)sqrt((double)best);
            v = 0.5f + 0.5f * cosf(d / ew * (float)M_PI);
        }
        dst[at] = v;
    }
}

// the smallest integer q that fails QUAD_3(d) < TSGSL_pow_2(ext) (a double
// against the RFLOAT square, :626, :635)
int limit_ext(float ext)
{
    const double e2 = (double)(float)((double)ext * (double)ext);
    int q = 0;
    while (q <= 3 * MK_LIMIT * MK_LIMIT && (double)q < e2) q++;
    return q;
}

// the smallest integer q that fails RFLOAT(NORM_3(d)) < ew (:668-670)
int limit_edge(float ew)
{
    int q = 0;
    while (q <= 3 * MK_LIMIT * MK_LIMIT && (float)std::sqrt((double)q) < ew) q++;
    return q;
}

// the largest a with a^2 < lim2 (lim2 >= 1)
int reach(int lim2)
{
    int a = 0;
    while ((a + 1) * (a + 1) < lim2) a++;
    return a;
}

template <int ONES>
int pack(const float* src, int N, uint64_t* bits, hipStream_t s)
{
    const int W = row_words(N);
    THX_LAUNCH(k_mask_pack<ONES>, dim3(thx::cdiv((long)N * N * W, MK_WAVES)), dim3(MK_THREADS), 0, s,
               src, N, W, bits);
    return THX_OK;
}

template <int MODE>
int ball(const float* src, float* dst, const uint64_t* bits, int N, int lim2, float ew, hipStream_t s)
{
    const int W = row_words(N), am = reach(lim2), RY = MK_T + 2 * am;
    // the rows (at most 70^2 24 B = 117600) and the half-width table (at most 63^2 B)
    const size_t lds = (size_t)RY * RY * 3 * sizeof(uint64_t) + (size_t)(2 * am + 1) * (2 * am + 1);
    static std::atomic<unsigned> ldsSet;
    if (lds > 64 * 1024)
        THX_RET(thx::set_max_lds(reinterpret_cast<const void*>(k_mask_ball<MODE>), 128 * 1024, ldsSet));
    THX_LAUNCH(k_mask_ball<MODE>, dim3(W, thx::cdiv(N, MK_T), thx::cdiv(N, MK_T)), dim3(MK_THREADS),
               lds, s, src, dst, bits, N, W, am, lim2, ew);
    return THX_OK;
}

int copy_map(const float* src, float* dst, int N, hipStream_t s)
{
    if (src != dst)
        THX_HIP(hipMemcpyAsync(dst, src, sizeof(float) * N * N * N, hipMemcpyDeviceToDevice, s));
    return THX_OK;
}

bool aliases(const float* a, const float* b, int N)
{
    const size_t n = (size_t)N * N * N;
    return a < b + n && b < a + n;
}

int extend_impl(const float* src, int N, float ext, float* dst, uint64_t* bits, hipStream_t s)
{
    if (ext == 0.f) return copy_map(src, dst, N, s);
    if (ext > 0.f) {
        THX_RET(pack<1>(src, N, bits, s));
        return ball<MK_EXTEND>(src, dst, bits, N, limit_ext(ext), 0.f, s);
    }
    THX_RET(pack<0>(src, N, bits, s));
    return ball<MK_ERODE>(src, dst, bits, N, limit_ext(ext), 0.f, s);
}

int soft_impl(const float* src, int N, float ew, float* dst, uint64_t* bits, hipStream_t s)
{
    if (!(ew > 0.f)) return copy_map(src, dst, N, s);
    THX_RET(pack<1>(src, N, bits, s));
    return ball<MK_SOFT>(src, dst, bits, N, limit_edge(ew), ew, s);
}

}  // namespace

extern "C" size_t thx_gen_mask_workspace(int N)
{
    if (!thx::box_ok(N)) return 0;
    return bits_bytes(N) + 256;
}

extern "C" int thx_mask_threshold(const float* src, int N, float thres, int removeCorners,
                                  float* dst, thx_stream_t stream)
{
    THX_CHECK_ARG(thx::box_ok(N), "thx_mask_threshold: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(src && dst, "thx_mask_threshold: src / dst is NULL");
    THX_CHECK_ARG(!aliases(src, dst, N), "thx_mask_threshold: dst aliases src");
    THX_CHECK_ARG(std::isfinite(thres), "thx_mask_threshold: thres is not finite");
    THX_LAUNCH(k_mask_threshold, dim3(thx::cdiv((long)N * N * N, MK_THREADS)), dim3(MK_THREADS), 0,
               thx::as_stream(stream), src, N, thres, removeCorners, dst);
    return THX_OK;
}

#define MK_CHECK_COMMON(name)                                                                    \
    THX_CHECK_ARG(thx::box_ok(N), name ": N=%d must be even, in [16, 1024]", N);                      \
    THX_CHECK_ARG(src && dst, name ": src / dst is NULL");                                       \
    THX_CHECK_ARG(src == dst || !aliases(src, dst, N), name ": dst overlaps src without being it"); \
    THX_CHECK_ARG(workspace && wsBytes >= thx_gen_mask_workspace(N),                             \
                  name ": workspace %zu < %zu bytes", workspace ? wsBytes : (size_t)0,           \
                  thx_gen_mask_workspace(N))

extern "C" int thx_mask_extend(const float* src, int N, float ext, float* dst, void* workspace,
                               size_t wsBytes, thx_stream_t stream)
{
    THX_CHECK_ARG(std::fabs(ext) <= (float)MK_LIMIT, "thx_mask_extend: |ext|=%g above %d",
                  (double)std::fabs(ext), MK_LIMIT);
    MK_CHECK_COMMON("thx_mask_extend");
    thx::Carver cv(workspace, wsBytes);
    return extend_impl(src, N, ext, dst, cv.take<uint64_t>(bits_bytes(N) / sizeof(uint64_t)),
                       thx::as_stream(stream));
}

extern "C" int thx_mask_soft_edge(const float* src, int N, float ew, float* dst, void* workspace,
                                  size_t wsBytes, thx_stream_t stream)
{
    THX_CHECK_ARG(ew <= (float)MK_LIMIT, "thx_mask_soft_edge: ew=%g above %d", (double)ew, MK_LIMIT);
    MK_CHECK_COMMON("thx_mask_soft_edge");
    thx::Carver cv(workspace, wsBytes);
    return soft_impl(src, N, ew, dst, cv.take<uint64_t>(bits_bytes(N) / sizeof(uint64_t)),
                     thx::as_stream(stream));
}

extern "C" int thx_gen_mask(const float* src, int N, float thres, float ext, float ew,
                            int removeCorners, float* dst, void* workspace, size_t wsBytes,
                            thx_stream_t stream)
{
    THX_CHECK_ARG(std::fabs(ext) <= (float)MK_LIMIT, "thx_gen_mask: |ext|=%g above %d",
                  (double)std::fabs(ext), MK_LIMIT);
    THX_CHECK_ARG(ew <= (float)MK_LIMIT, "thx_gen_mask: ew=%g above %d", (double)ew, MK_LIMIT);
    THX_CHECK_ARG(thx::box_ok(N), "thx_gen_mask: N=%d must be even, in [16, 1024]", N);
    THX_CHECK_ARG(src && dst, "thx_gen_mask: src / dst is NULL");
    THX_CHECK_ARG(!aliases(src, dst, N), "thx_gen_mask: dst aliases src");
    THX_CHECK_ARG(std::isfinite(thres), "thx_gen_mask: thres is not finite");
    THX_CHECK_ARG(workspace && wsBytes >= thx_gen_mask_workspace(N),
                  "thx_gen_mask: workspace %zu < %zu bytes", workspace ? wsBytes : (size_t)0,
                  thx_gen_mask_workspace(N));
    hipStream_t s = thx::as_stream(stream);
    thx::Carver cv(workspace, wsBytes);
    uint64_t* bits = cv.take<uint64_t>(bits_bytes(N) / sizeof(uint64_t));
    // the stages after the threshold read only their own voxel and the packed
    // bits, so they run in place on dst
    THX_LAUNCH(k_mask_threshold, dim3(thx::cdiv((long)N * N * N, MK_THREADS)), dim3(MK_THREADS), 0, s,
               src, N, thres, removeCorners, dst);
    THX_RET(extend_impl(dst, N, ext, dst, bits, s));
    return soft_impl(dst, N, ew, dst, bits, s);
}
