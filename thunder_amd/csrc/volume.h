// volume.h -- cubic half-complex maps [k][j][i <= N/2] (j, k wrapped): indices, shells,
// ordered shell sums, and the sizes the map-level entry points (fsc_masked, postprocess,
// refresh, mask, subtract) agree on.
//
// The shell sums are FP64 in a fixed order, without atomics: a wave takes whole rows (j, k)
// with its lanes along i, where the shell index never decreases, so a segmented scan sums the
// lanes of one shell and the segment's last lane adds the total to the wave's own LDS
// histogram (shell_pass); the block adds its waves' histograms in wave order into its slot of
// the workspace, and one block adds the slots in block order (sum_slots).  That order is what
// makes the callers bit-identical from run to run.
#pragma once
#include "common.h"

// signed coordinate of a wrapped index
THX_DEV int signed_idx(int a, int n) { return a < n / 2 ? a : a - n; }

// AROUND(NORM_3(i, j, k)) of an integer q2 = i^2 + j^2 + k^2 < 2^24: q2 is exact in FP32 and
// sqrt(q2) is at least 0.25 / (2 sqrt(q2)) > 1e-4 away from any half-integer ((m + 1/2)^2 is
// never an integer), far more than FP32's rounding at 887, so the FP32 root rounds to the
// same integer as the FP64 one
THX_DEV int shell_of(int q2) { return (int)rintf(sqrtf((float)q2)); }

// One block's pass over its rows of an N^3 half-complex map: part[blockIdx.x][NS][nTab] = its
// NS sums per shell, over the voxels of shells below rU (<= nTab) that voxel counts.
// voxel(row, i, u, s) loads stored voxel row (N / 2 + 1) + i of shell u and fills s[NS], or
// returns false (s untouched: not counted).  sh is the block's LDS, [WAVES][NS][nTab]; the
// block has 64 WAVES threads.
template <int NS, int WAVES, typename Voxel>
THX_DEV void shell_pass(double* sh, int N, int nTab, int rU, double* __restrict__ part, Voxel voxel)
{
    constexpr int THREADS = 64 * WAVES;
    for (int s = threadIdx.x; s < WAVES * NS * nTab; s += THREADS) sh[s] = 0.0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* mine = sh + (size_t)wv * NS * nTab;
    const int nc = N / 2 + 1;
    const long nRow = (long)N * N;
    for (long row = (long)blockIdx.x * WAVES + wv; row < nRow; row += (long)gridDim.x * WAVES) {
        const int j = signed_idx((int)(row % N), N), k = signed_idx((int)(row / N), N);
        const int c2 = j * j + k * k;
        for (int i0 = 0; i0 < nc; i0 += 64) {
            // the shell grows with i: nothing further along this row is below rU
            if (shell_of(i0 * i0 + c2) >= rU) break;
            const int i = i0 + lane;
            const int u = i < nc ? shell_of(i * i + c2) : 1 << 30;
            double s[NS];
#pragma unroll
            for (int e = 0; e < NS; e++) s[e] = 0.0;
            const bool in = u < rU && voxel(row, i, u, s);
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int uu = __shfl_up(u, o, 64);
                double t[NS];
#pragma unroll
                for (int e = 0; e < NS; e++) t[e] = __shfl_up(s[e], o, 64);
                if (lane >= o && uu == u) {
#pragma unroll
                    for (int e = 0; e < NS; e++) s[e] += t[e];
                }
            }
            const int un = __shfl_down(u, 1, 64);
            if ((lane == 63 || un != u) && in) {
#pragma unroll
                for (int e = 0; e < NS; e++) mine[e * nTab + u] += s[e];
            }
        }
    }
    __syncthreads();
    for (int s = threadIdx.x; s < NS * nTab; s += THREADS) {
        double t = 0.0;
        for (int w = 0; w < WAVES; w++) t += sh[(size_t)w * NS * nTab + s];
        part[(size_t)blockIdx.x * NS * nTab + s] = t;
    }
}

// entry s of the nBlock slots part[block][NS][nTab] of shell_pass, added in block order,
// sixteen loads in flight
template <int NS>
THX_DEV double sum_slots(const double* __restrict__ part, int nBlock, int nTab, int s)
{
    double t = 0.0;
    int b = 0;
    for (; b + 16 <= nBlock; b += 16) {
        double v[16];
#pragma unroll
        for (int e = 0; e < 16; e++) v[e] = part[(size_t)(b + e) * NS * nTab + s];
#pragma unroll
        for (int e = 0; e < 16; e++) t += v[e];
    }
    for (; b < nBlock; b++) t += part[(size_t)b * NS * nTab + s];
    return t;
}

// softMask's weight of the source (1 - w, bg = 0) at distance u
THX_DEV float soft_mask(float u, float r, float ew)
{
    if (u > r + ew) return 0.f;
    if (u >= r) return 1.f - (0.5f - 0.5f * cosf((u - r) / ew * (float)M_PI));
    return 1.f;
}

// resP(curve, thres, 1, 1, false) (src/Functions/Spectrum.cpp:339-363): the first shell from 1
// whose value is below thres, minus one (the trailing result--); thres is the reference's
// RFLOAT, widened for the compare
THX_DEV int res_p(const double* curve, int nShell, float thres)
{
    const double thr = (double)thres;
    int r = 1;
    for (; r < nShell; r++)
        if (curve[r] < thr) break;
    return r - 1;
}

namespace thx {

inline bool box_ok(int N) { return N >= 16 && N <= 1024 && N % 2 == 0; }
inline bool shells_ok(int N, int nShell) { return nShell >= 2 && nShell <= N / 2; }
inline size_t ft_elems(int N) { return (size_t)(N / 2 + 1) * N * N; }

// hipFFT's work area is known only once a plan exists, and the workspace
// query is host-only: reserve twice the transform's complex volume (the
// 3D real plans of rocFFT take one) and check at the call.
inline size_t fft_reserve(int N) { return 2 * ft_elems(N) * sizeof(float2); }

// grid of a shell_pass: eight rows per wave, at most cap blocks (walked in order afterwards)
inline int shell_blocks(int N, int waves, int cap)
{
    const long b = ((long)N * N + waves * 8 - 1) / (waves * 8);
    return (int)(b > cap ? cap : b);
}

// grid of a grid-stride kernel over n elements, capped (the caps are measured per file)
inline unsigned stream_blocks(size_t n, int threads, unsigned cap)
{
    const size_t b = (n + threads - 1) / threads;
    return (unsigned)(b > cap ? cap : b);
}

// planes i = 0 and i = N/2 of a half-complex volume <- their Hermitian part, before a C2R
// (fsc_masked.hip)
int hermitian_planes(float2* ft, int N, hipStream_t s);

// the same for nPlane half-complex images [N][N/2+1]: columns i = 0 and i = N/2 <- their
// Hermitian part, before a batched 2D C2R (subtract.hip)
int hermitian_cols(float2* ft, size_t nPlane, int N, hipStream_t s);

// after that C2R, in place on nPlane images [N][N]: times scale, and with centred the corner
// origin moved to the centred layout of an MRC stack; plane p is NaN when cls (may be NULL:
// class 0) has cls[p % nImg] outside [0, nK) (subtract.hip)
int rl_finish(float* rl, size_t nPlane, int nImg, int N, int centred, float scale, const int* cls,
              int nK, hipStream_t s);

}  // namespace thx
