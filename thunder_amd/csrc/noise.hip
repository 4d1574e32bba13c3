// noise.hip -- the noise model of Optimiser::maximization (src/Optimiser.cpp:
// 3405-3559) next to reconstructRef: the residual power spectra behind
// allReduceSigma (:6395-6709), the per-image norm of normCorrection
// (:6201-6393), initSigma (:5145-5243) and allocPreCal's sigRcpP expansion
// (:8060-8071), with the switches of include/Config.h as they stand
// (SIGMA_WHOLE_FREQUENCY, SIGMA_RANK1ST, CTF_ON_THE_FLY,
// RECENTRE_IMAGE_EACH_ITERATION, NORM_MASK, NORM_CORRECTION, REFRESH_SIGMA on;
// SIGMA_MASK, SIGMA_GRADING and CORRECT_SCALE off).
//
//   powerSpectrum(dst, img, r) (src/Functions/Spectrum.cpp:161-190): every
//     stored half-plane pixel (column 0 with j < 0 included) with
//     i^2+j^2 < r^2 and u = rint(|(i,j)|) < r adds |img|^2 to shell u; the
//     shell sum is divided by its pixel count.  thx_spectrum_pixels lists
//     that domain shell by shell, so a wave owns whole shells: it walks a
//     shell in chunks of 64 pixels, every lane summing its own pixels in
//     table order, and folds the 64 partial sums with the xor butterfly.  The
//     order of every addition is fixed by the table, so the spectra are
//     bit-identical from run to run -- no floating-point atomics anywhere.
//   the residual kernel: one workgroup per image, its waves take the shells
//     u = wave, wave + 4, ... (shell length grows with u, so interleaving
//     balances them).  Per pixel: FP64 rotation -> FP32 coordinate
//     (rot_coord), trilinear / bilinear gather of the class's projectee,
//     the a4 phases of t and t - offset, the CTF on the fly at (dU d, dV d),
//     then |img - M|^2, |ori - N|^2, |M|^2, |img|^2.  Pixels outside the disc
//     are never read.
//   the per-group sums and everything initSigma accumulates are FP64 and
//     added in image order by one thread per output element.
#include "common.h"

#include <cmath>

namespace {

constexpr int NS_THREADS = 256;
constexpr int NS_WAVES = NS_THREADS / 64;

// bilinear gather of Image::getByInterpolationFT (src/Image/Image.cpp:345-367)
// as in twod.hip: fold, floor, 4 taps in box order j, i
THX_DEV float2 interp2_ft(const float2* __restrict__ img, int vdim, float x, float y)
{
    const bool conj = !(x >= 0.f);
    if (conj) { x = -x; y = -y; }
    const float fx = floorf(x), fy = floorf(y);
    const int x0 = (int)fx, y0 = (int)fy;
    const float dx = x - fx, dy = y - fy;
    const float wx[2] = {1.f - dx, dx}, wy[2] = {1.f - dy, dy};
    const int nc = vdim / 2 + 1;
    float re = 0.f, im = 0.f;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const float2* row = img + (size_t)wrap_idx(y0 + j, vdim) * nc + x0;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const float w = wx[i] * wy[j];
            re += row[i].x * w;
            im += row[i].y * w;
        }
    }
    return make_float2(re, conj ? -im : im);
}

// sum of |img|^2 over table entries [b, e), one wave, fixed order; the
// roundings are spelled out (no FMA contraction), so every kernel that walks a
// shell gets the same bits
THX_DEV float shell_power(const float2* __restrict__ img, const int* __restrict__ iPxl, int b,
                          int e, int lane)
{
    float s = 0.f;
    for (int q = b + lane; q < e; q += 64) {
        const float2 v = img[iPxl[q]];
        s = __fadd_rn(s, __fadd_rn(__fmul_rn(v.x, v.x), __fmul_rn(v.y, v.y)));
    }
    return wave_sum(s);
}

__global__ void __launch_bounds__(NS_THREADS) k_power_spectrum(const float2* __restrict__ imgFT,
                                                               long per, int r,
                                                               const int* __restrict__ iPxl,
                                                               const int* __restrict__ shellStart,
                                                               float* __restrict__ ps)
{
    const size_t l = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float2* img = imgFT + l * per;
    for (int u = wv; u < r; u += NS_WAVES) {
        const int b = shellStart[u], e = shellStart[u + 1];
        const float s = shell_power(img, iPxl, b, e, lane);
        if (lane == 0) ps[l * r + u] = s / (float)(e - b);
    }
}

template <bool TWO_D>
__global__ void __launch_bounds__(NS_THREADS) k_residual(
    const float2* __restrict__ vol, int vdim, int pf, int nK, long volStride,
    const float2* __restrict__ imgFT, const float2* __restrict__ oriFT,
    const float* __restrict__ attr, const double* __restrict__ rot,
    const double* __restrict__ trans, const double* __restrict__ offS,
    const double* __restrict__ dF, const int* __restrict__ cls, int idim, long per, int r,
    const int* __restrict__ iCol, const int* __restrict__ iRow, const int* __restrict__ iPxl,
    const int* __restrict__ shellStart, float* __restrict__ spectra, double* __restrict__ norm,
    float rL2, float rN2)
{
    __shared__ double sMat[9];
    __shared__ double sNorm[NS_WAVES];
    const size_t l = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float* S = spectra + l * 4 * r;
    const int k = cls ? cls[l] : 0;
    if (k < 0 || k >= nK) {
        // a class outside the projectee stack: no gather, the image's outputs are NaN
        for (int q = tid; q < 4 * r; q += NS_THREADS)
            if (oriFT || q / r != 1) S[q] = __builtin_nanf("");
        if (norm && tid == 0) norm[l] = __builtin_nan("");
        return;
    }
    if (tid == 0) {
        if (TWO_D) {
            sMat[0] = rot[2 * l];
            sMat[1] = rot[2 * l + 1];
        } else {
            const double q[4] = {rot[4 * l], rot[4 * l + 1], rot[4 * l + 2], rot[4 * l + 3]};
            quat_to_mat(q, sMat);
        }
    }
    __syncthreads();
    const double mm[6] = {sMat[0], sMat[1], sMat[2], sMat[3], sMat[4], sMat[5]};
    const float2* P = vol + (size_t)k * volStride;
    const float2* img = imgFT + l * per;
    const float2* ori = oriFT ? oriFT + l * per : nullptr;
    const float* A = attr + 8 * l;
    const double d = dF ? dF[l] : 1.0;
    // CTF(dU d, dV d) (src/Optimiser.cpp:6537-6547); d = 1 leaves the attributes
    const float dU = dF ? (float)(A[2] * d) : A[2], dV = dF ? (float)(A[3] * d) : A[3];
    const double tx = trans[2 * l], ty = trans[2 * l + 1];
    const double ox = offS ? offS[2 * l] : 0.0, oy = offS ? offS[2 * l + 1] : 0.0;
    // translate(): RFLOAT shift / nColRL (src/Image/ImageFunctions.cpp:322-339)
    const float mCol = (float)tx / idim, mRow = (float)ty / idim;
    const float nCol = (float)(tx - ox) / idim, nRow = (float)(ty - oy) / idim;
    double nrm = 0.0;
    for (int u = wv; u < r; u += NS_WAVES) {
        const int b = shellStart[u], e = shellStart[u + 1];
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        for (int q = b + lane; q < e; q += 64) {
            const int ic = iCol[q], ir = iRow[q], ip = iPxl[q];
            float2 p;
            if (TWO_D) {
                const double nx = (double)(ic * pf), ny = (double)(ir * pf);
                p = interp2_ft(P, vdim, (float)(mm[0] * nx - mm[1] * ny),
                               (float)(mm[1] * nx + mm[0] * ny));
            } else {
                float x, y, z;
                rot_coord(mm, ic, ir, pf, x, y, z);
                p = interp_ft(P, vdim, x, y, z);
            }
            const float c = ctf_at(A, dU, dV, ic, ir, idim);
            const float2 pm = cmul(p, phase_shift(ic, ir, mCol, mRow));
            const float2 M = make_float2(pm.x * c, pm.y * c);
            const float2 v = img[ip];
            const float er = v.x - M.x, ei = v.y - M.y;
            const float res = er * er + ei * ei;
            s0 += res;
            s2 += M.x * M.x + M.y * M.y;
            s3 += v.x * v.x + v.y * v.y;
            if (ori) {
                const float2 pn = cmul(p, phase_shift(ic, ir, nCol, nRow));
                const float2 o = ori[ip];
                const float fr = o.x - pn.x * c, fi = o.y - pn.y * c;
                s1 += fr * fr + fi * fi;
            }
            if (norm) {
                // normCorrection's bound is on the pixel radius, not on the shell
                const float quad = (float)(ic * ic + ir * ir);
                if (quad >= rL2 && quad < rN2) nrm += (double)res;
            }
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        s3 = wave_sum(s3);
        if (lane == 0) {
            const float n = (float)(e - b);
            S[u] = s0 / n;
            if (ori) S[r + u] = s1 / n;
            S[2 * r + u] = s2 / n;
            S[3 * r + u] = s3 / n;
        }
    }
    if (norm) {
        nrm = wave_sum(nrm);
        if (lane == 0) sNorm[wv] = nrm;
        __syncthreads();
        if (tid == 0) {
            double t = 0.0;
            for (int w = 0; w < NS_WAVES; w++) t += sNorm[w];
            norm[l] = t;
        }
    }
}

// one thread per (group, column) of acc[3][nGroup][r+1]; images in index order
__global__ void __launch_bounds__(64) k_sigma_accumulate(const float* __restrict__ spectra,
                                                         const int* __restrict__ group, int nImg,
                                                         int r, int nGroup,
                                                         double* __restrict__ acc)
{
    const int q = blockIdx.x * 64 + threadIdx.x;
    if (q >= nGroup * (r + 1)) return;
    const int g = q / (r + 1), u = q % (r + 1);
    const size_t plane = (size_t)nGroup * (r + 1);
    double m = acc[q], n = acc[plane + q], s = acc[2 * plane + q];
    // the loop is one dependent chain per thread and so latency bound: the
    // loads of NA_DEPTH images are issued together, the additions stay in
    // index order
    constexpr int NA_DEPTH = 8;
    for (int l0 = 0; l0 < nImg; l0 += NA_DEPTH) {
        float v[NA_DEPTH][4];
        int gl[NA_DEPTH];
        const int uc = u < r ? u : r - 1;       // the weight column loads a valid one, unused
#pragma unroll
        for (int k = 0; k < NA_DEPTH; k++) {
            const int l = l0 + k < nImg ? l0 + k : nImg - 1;
            gl[k] = group ? group[l] : 0;
            const float* S = spectra + (size_t)l * 4 * r;
#pragma unroll
            for (int c = 0; c < 4; c++) v[k][c] = S[c * r + uc];
        }
        double t[NA_DEPTH];
#pragma unroll
        for (int k = 0; k < NA_DEPTH; k++) t[k] = sqrt((double)v[k][2] / (double)v[k][3]);
#pragma unroll
        for (int k = 0; k < NA_DEPTH; k++) {
            const bool in = l0 + k < nImg && gl[k] == g;
            const bool w = u == r;
            m += in ? (w ? 1.0 : (double)v[k][0] / 2) : 0.0;
            n += in ? (w ? 1.0 : (double)v[k][1] / 2) : 0.0;
            s += in ? (w ? 1.0 : t[k]) : 0.0;
        }
    }
    acc[q] = m;
    acc[plane + q] = n;
    acc[2 * plane + q] = s;
}

// avgSum[e] += sum_l oriFT[l][e] over every stored float, image order
__global__ void __launch_bounds__(256) k_init_avg(const float* __restrict__ oriFT, int nImg,
                                                  long perF, double* __restrict__ avgSum)
{
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    if (e >= perF) return;
    double a = avgSum[e];
    for (int l = 0; l < nImg; l++) a += (double)oriFT[(size_t)l * perF + e];
    avgSum[e] = a;
}

// psSum[u] += sum_l powerSpectrum(oriFT_l)[u]: one wave per shell, image order
__global__ void __launch_bounds__(64) k_init_ps(const float2* __restrict__ oriFT, int nImg,
                                                long per, const int* __restrict__ iPxl,
                                                const int* __restrict__ shellStart,
                                                double* __restrict__ psSum)
{
    const int u = blockIdx.x, lane = threadIdx.x;
    const int b = shellStart[u], e = shellStart[u + 1];
    double a = psSum[u];
    for (int l = 0; l < nImg; l++)
        a += (double)(shell_power(oriFT + (size_t)l * per, iPxl, b, e, lane) / (float)(e - b));
    if (lane == 0) psSum[u] = a;
}

__global__ void __launch_bounds__(256) k_sig_rcp_rows(const double* __restrict__ sigRcp, int nCol,
                                                      const int* __restrict__ group,
                                                      const int* __restrict__ iSig, int nPxl,
                                                      int nGroup, float* __restrict__ out)
{
    const size_t l = blockIdx.y;
    const int g = group ? group[l] : 0;
    const bool ok = g >= 0 && g < nGroup;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < nPxl; i += gridDim.x * 256) {
        const int u = iSig[i];
        out[l * nPxl + i] = ok && u >= 0 && u < nCol ? (float)sigRcp[(size_t)g * nCol + u]
                                                    : __builtin_nanf("");
    }
}

__global__ void __launch_bounds__(256) k_img_scale(float2* __restrict__ imgFT,
                                                   float2* __restrict__ oriFT,
                                                   const float* __restrict__ scale, long per)
{
    const size_t l = blockIdx.y;
    const float s = scale[l];
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < per; q += (long)gridDim.x * 256) {
        float2 v = imgFT[l * per + q];
        imgFT[l * per + q] = make_float2(v.x * s, v.y * s);
        if (oriFT) {
            v = oriFT[l * per + q];
            oriFT[l * per + q] = make_float2(v.x * s, v.y * s);
        }
    }
}

bool radius_ok(int idim, int r) { return idim > 0 && idim % 2 == 0 && r >= 1 && r <= idim / 2 - 1; }

template <bool TWO_D>
int residual_launch(const char* who, const float* vol, int vdim, int pf, int nK,
                    const float* imgFT, const float* oriFT, const float* attr, const double* rot,
                    const double* trans, const double* offS, const double* dF, const int* cls,
                    int nImg, int idim, int r, const int* iCol, const int* iRow, const int* iPxl,
                    const int* shellStart, float* spectra, double* norm, float rL, float rNorm,
                    thx_stream_t stream)
{
    THX_CHECK_ARG(vol && imgFT && attr && rot && trans && iCol && iRow && iPxl && shellStart &&
                      spectra,
                  "%s: null argument", who);
    THX_CHECK_ARG(vdim > 0 && vdim % 2 == 0 && pf > 0 && nK >= 1 && nImg >= 0, "%s: bad sizes", who);
    THX_CHECK_ARG(radius_ok(idim, r), "%s: r=%d outside [1, idim/2-1]", who, r);
    THX_CHECK_ARG((long)r * pf < vdim / 2 - 1, "%s: r * pf reaches the projectee's edge", who);
    // every pixel below rNorm has to lie in a shell below r: |(i,j)| < r - 1/2
    THX_CHECK_ARG(!norm || (rL >= 0.f && rNorm >= rL && rNorm <= r - 0.5f),
                  "%s: norm radii need 0 <= rL <= rNorm <= r - 1/2", who);
    if (nImg == 0) return THX_OK;
    const long per = (long)idim * (idim / 2 + 1);
    const long volStride = (long)(vdim / 2 + 1) * vdim * (TWO_D ? 1 : vdim);
    hipLaunchKernelGGL(k_residual<TWO_D>, dim3(nImg), dim3(NS_THREADS), 0, thx::as_stream(stream),
                       reinterpret_cast<const float2*>(vol), vdim, pf, nK, volStride,
                       reinterpret_cast<const float2*>(imgFT),
                       reinterpret_cast<const float2*>(oriFT), attr, rot, trans, offS, dF, cls,
                       idim, per, r, iCol, iRow, iPxl, shellStart, spectra, norm,
                       (float)((double)rL * rL), (float)((double)rNorm * rNorm));
    THX_LAUNCH_CHECK();
    return THX_OK;
}

// the pixels of shell u < r, in the reference's loop order (j outer, i inner)
template <typename F>
void for_shell_pixels(int r, F f)
{
    for (long j = -r; j < r; j++)
        for (long i = 0; i <= r; i++) {
            if (i * i + j * j >= (long)r * r) continue;
            const int u = (int)std::rint(std::hypot((double)i, (double)j));
            if (u < r) f((int)i, (int)j, u);
        }
}

}  // namespace

extern "C" int thx_spectrum_pixels(int idim, int r, int cap, int* iCol, int* iRow, int* iShell,
                                   int* iPxl, int* shellStart, int* nPxl)
{
    THX_CHECK_ARG(nPxl, "thx_spectrum_pixels: nPxl is NULL");
    THX_CHECK_ARG(radius_ok(idim, r), "thx_spectrum_pixels: r=%d outside [1, idim/2-1]", r);
    std::vector<int> start(r + 1, 0);
    for_shell_pixels(r, [&](int, int, int u) { start[u + 1]++; });
    for (int u = 0; u < r; u++) start[u + 1] += start[u];
    *nPxl = start[r];
    if (shellStart)
        for (int u = 0; u <= r; u++) shellStart[u] = start[u];
    if (!iCol && !iRow && !iShell && !iPxl) return THX_OK;
    THX_CHECK_ARG(cap >= start[r], "thx_spectrum_pixels: cap=%d too small (%d pixels)", cap,
                  start[r]);
    std::vector<int> at(start.begin(), start.end() - 1);
    const long nColFT = idim / 2 + 1;
    for_shell_pixels(r, [&](int i, int j, int u) {
        const int n = at[u]++;
        if (iCol) iCol[n] = i;
        if (iRow) iRow[n] = j;
        if (iShell) iShell[n] = u;
        if (iPxl) iPxl[n] = (int)((j >= 0 ? j : j + idim) * nColFT + i);
    });
    return THX_OK;
}

extern "C" int thx_power_spectrum(const float* imgFT, int nImg, int idim, int r, const int* iPxl,
                                  const int* shellStart, float* ps, thx_stream_t stream)
{
    THX_CHECK_ARG(imgFT && iPxl && shellStart && ps, "thx_power_spectrum: null argument");
    THX_CHECK_ARG(nImg >= 0 && radius_ok(idim, r), "thx_power_spectrum: bad sizes");
    if (nImg == 0) return THX_OK;
    hipLaunchKernelGGL(k_power_spectrum, dim3(nImg), dim3(NS_THREADS), 0, thx::as_stream(stream),
                       reinterpret_cast<const float2*>(imgFT), (long)idim * (idim / 2 + 1), r, iPxl,
                       shellStart, ps);
    THX_LAUNCH_CHECK();
    return THX_OK;
}

extern "C" int thx_residual_spectra(const float* vol, int vdim, int pf, int nK, const float* imgFT,
                                    const float* oriFT, const float* attr, const double* quat,
                                    const double* trans, const double* offS, const double* dF,
                                    const int* cls, int nImg, int idim, int r, const int* iCol,
                                    const int* iRow, const int* iPxl, const int* shellStart,
                                    float* spectra, double* norm, float rL, float rNorm,
                                    thx_stream_t stream)
{
    return residual_launch<false>("thx_residual_spectra", vol, vdim, pf, nK, imgFT, oriFT, attr,
                                  quat, trans, offS, dF, cls, nImg, idim, r, iCol, iRow, iPxl,
                                  shellStart, spectra, norm, rL, rNorm, stream);
}

extern "C" int thx_residual_spectra2d(const float* vol, int vdim, int pf, int nK,
                                      const float* imgFT, const float* oriFT, const float* attr,
                                      const double* rot, const double* trans, const double* offS,
                                      const double* dF, const int* cls, int nImg, int idim, int r,
                                      const int* iCol, const int* iRow, const int* iPxl,
                                      const int* shellStart, float* spectra, double* norm, float rL,
                                      float rNorm, thx_stream_t stream)
{
    return residual_launch<true>("thx_residual_spectra2d", vol, vdim, pf, nK, imgFT, oriFT, attr,
                                 rot, trans, offS, dF, cls, nImg, idim, r, iCol, iRow, iPxl,
                                 shellStart, spectra, norm, rL, rNorm, stream);
}

extern "C" int thx_sigma_accumulate(const float* spectra, const int* group, int nImg, int r,
                                    int nGroup, double* acc, thx_stream_t stream)
{
    THX_CHECK_ARG(spectra && acc, "thx_sigma_accumulate: null argument");
    THX_CHECK_ARG(nImg >= 0 && r >= 1 && nGroup >= 1 && (long)nGroup * (r + 1) < (1l << 30),
                  "thx_sigma_accumulate: bad sizes");
    if (nImg == 0) return THX_OK;
    hipLaunchKernelGGL(k_sigma_accumulate, dim3(thx::cdiv((long)nGroup * (r + 1), 64)), dim3(64), 0,
                       thx::as_stream(stream), spectra, group, nImg, r, nGroup, acc);
    THX_LAUNCH_CHECK();
    return THX_OK;
}

extern "C" int thx_sigma_finalise(const double* acc, int nGroup, int r, int nCol, double alpha,
                                  int grouped, double* sig, double* sigRcp)
{
    THX_CHECK_ARG(acc && sig && sigRcp, "thx_sigma_finalise: null argument");
    THX_CHECK_ARG(nGroup >= 1 && r >= 1 && nCol >= r + 1, "thx_sigma_finalise: need nCol >= r + 1");
    const size_t plane = (size_t)nGroup * (r + 1);
    std::vector<double> row[3];
    for (int g = 0; g < nGroup; g++) {
        // rows / counts; without grouping row 0 serves every group (:6653-6676)
        const int src = grouped ? g : 0;
        for (int q = 0; q < 3; q++) {
            const double* a = acc + q * plane + (size_t)src * (r + 1);
            row[q].assign(nCol - 1, 0.0);
            for (int u = 0; u < r; u++) row[q][u] = a[u] / a[r];
            for (int u = r; u < nCol - 1; u++) row[q][u] = row[q][r - 1];   // :6678-6684
        }
        for (int u = 0; u < nCol - 1; u++) {
            const double ratio = std::fmin(1.0, row[2][u]);
            const double s = ratio * row[0][u] + (1 - ratio) * alpha * row[1][u];
            sig[(size_t)g * nCol + u] = s;
            sigRcp[(size_t)g * nCol + u] = -0.5 / s;
        }
        sig[(size_t)g * nCol + nCol - 1] = 0.0;
        sigRcp[(size_t)g * nCol + nCol - 1] = 0.0;
    }
    return THX_OK;
}

extern "C" int thx_sigma_init_accumulate(const float* oriFT, int nImg, int idim, int r,
                                         const int* iPxl, const int* shellStart, double* avgSum,
                                         double* psSum, thx_stream_t stream)
{
    THX_CHECK_ARG(oriFT && iPxl && shellStart && avgSum && psSum,
                  "thx_sigma_init_accumulate: null argument");
    THX_CHECK_ARG(nImg >= 0 && radius_ok(idim, r), "thx_sigma_init_accumulate: bad sizes");
    if (nImg == 0) return THX_OK;
    const long per = (long)idim * (idim / 2 + 1);
    hipLaunchKernelGGL(k_init_avg, dim3(thx::cdiv(2 * per, 256)), dim3(256), 0,
                       thx::as_stream(stream), oriFT, nImg, 2 * per, avgSum);
    THX_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_init_ps, dim3(r), dim3(64), 0, thx::as_stream(stream),
                       reinterpret_cast<const float2*>(oriFT), nImg, per, iPxl, shellStart, psSum);
    THX_LAUNCH_CHECK();
    return THX_OK;
}

extern "C" int thx_sigma_init_finalise(const double* avgSum, const double* psSum, double nTotal,
                                       int idim, int r, int nGroup, int nCol, double* sig,
                                       double* sigRcp)
{
    THX_CHECK_ARG(avgSum && psSum && sig && sigRcp, "thx_sigma_init_finalise: null argument");
    THX_CHECK_ARG(radius_ok(idim, r) && nGroup >= 1 && nCol >= r + 1 && nTotal > 0,
                  "thx_sigma_init_finalise: bad sizes");
    // ringAverage(u, avg, re + im) (src/Functions/Spectrum.cpp:47-62): for
    // u < r <= idim/2 - 1 the ring is shell u of the table
    std::vector<double> ring(r, 0.0);
    std::vector<long> cnt(r, 0);
    const long nColFT = idim / 2 + 1;
    for_shell_pixels(r, [&](int i, int j, int u) {
        const size_t p = (size_t)((j >= 0 ? j : j + idim) * nColFT + i);
        ring[u] += (avgSum[2 * p] + avgSum[2 * p + 1]) / nTotal;
        cnt[u]++;
    });
    std::vector<double> s(nCol - 1);
    for (int u = 0; u < r; u++) {
        const double a = ring[u] / cnt[u];
        s[u] = (psSum[u] / nTotal - a * a) / 2;
    }
    for (int u = r; u < nCol - 1; u++) s[u] = s[r - 1];
    for (int g = 0; g < nGroup; g++) {
        for (int u = 0; u < nCol - 1; u++) {
            sig[(size_t)g * nCol + u] = s[u];
            sigRcp[(size_t)g * nCol + u] = -0.5 / s[u];
        }
        sig[(size_t)g * nCol + nCol - 1] = 0.0;
        sigRcp[(size_t)g * nCol + nCol - 1] = 0.0;
    }
    return THX_OK;
}

extern "C" int thx_sig_rcp_rows(const double* sigRcp, int nGroup, int nCol, const int* group,
                                const int* iSig, int nPxl, int nImg, float* out,
                                thx_stream_t stream)
{
    THX_CHECK_ARG(sigRcp && iSig && out, "thx_sig_rcp_rows: null argument");
    THX_CHECK_ARG(nGroup >= 1 && nCol >= 1 && nPxl >= 0 && nImg >= 0 && nImg <= 65535,
                  "thx_sig_rcp_rows: bad sizes (at most 65535 images per call)");
    if (nImg == 0 || nPxl == 0) return THX_OK;
    const unsigned gx = thx::cdiv(nPxl, 256) > 32 ? 32 : thx::cdiv(nPxl, 256);
    hipLaunchKernelGGL(k_sig_rcp_rows, dim3(gx, nImg), dim3(256), 0, thx::as_stream(stream), sigRcp,
                       nCol, group, iSig, nPxl, nGroup, out);
    THX_LAUNCH_CHECK();
    return THX_OK;
}

extern "C" int thx_img_scale(float* imgFT, float* oriFT, const float* scale, int nImg, int idim,
                             thx_stream_t stream)
{
    THX_CHECK_ARG(imgFT && scale, "thx_img_scale: null argument");
    THX_CHECK_ARG(nImg >= 0 && nImg <= 65535 && idim > 0 && idim % 2 == 0,
                  "thx_img_scale: bad sizes (at most 65535 images per call)");
    if (nImg == 0) return THX_OK;
    const long per = (long)idim * (idim / 2 + 1);
    const unsigned gx = thx::cdiv(per, 256) > 64 ? 64 : thx::cdiv(per, 256);
    hipLaunchKernelGGL(k_img_scale, dim3(gx, nImg), dim3(256), 0, thx::as_stream(stream),
                       reinterpret_cast<float2*>(imgFT), reinterpret_cast<float2*>(oriFT), scale,
                       per);
    THX_LAUNCH_CHECK();
    return THX_OK;
}
