// load.hip -- thx_pf_load: Particle::load (src/Particle.cpp:401-556), MODE_3D,
// for every image of a batch at once -- what Optimiser::loadParticles
// (src/Optimiser.cpp:5312-5384) does per image on the host when a run starts
// from a .thu table instead of a global search.  Every pointer is a device
// pointer, FP64; nothing synchronises with the host or is read back.
//
// One stream-ordered chain of three launches:
//   k_pf_load          the clouds, pT, pD and the defocus spread vari[5];
//   k_pf_balance_rot   pR = balanceWeight(PAR_R) of the rotation cloud (:496);
//   k_pf_calvari_vari  vari[0 .. 4] = calVari(PAR_R), calVari(PAR_T) (:499, :530)
// the last two being the expectation driver's own statistics (optimiser.hip).
//
// Where the draws come from (the reference draws from one gsl engine per
// thread, which fixes no layout): image l owns 8 lanes; lane j owns the
// counter stream (seed; l, stream_id, j) of common.h's Philox and the
// particles i = j (mod 8) of every set, in rising order.  With nR_j, nT_j, nD_j
// the lane's share of the mR rotations, mT translations and mD defocus
// factors (n_j = (n + 7 - j) / 8), its counter's fourth word runs
//   [0, 4 nR_j)        rotations, four uniforms each: two Box-Muller pairs
//                      (g0, g1), (g2, g3) -- k_pf_perturb's layout;
//   then 2 nT_j        translations, one pair (gx, gy) each;
//   then 2 nD_j        defocus factors, one pair each, the cosine branch kept;
//   then nR_j          the rotations' sign uniforms, one each.
// So image l's result depends on its own row and (seed, l, stream_id) only,
// not on nImg or on the launch's shape.
#include "internal.h"
#include "pf_group.h"
#include "symmetry.h"

namespace {

__global__ void __launch_bounds__(256) k_pf_load(
    int nImg, int mR, int mT, int mD, const double* __restrict__ topQuat,
    const double* __restrict__ k, const double* __restrict__ topTrans,
    const double* __restrict__ sd, const double* __restrict__ topD, const double* __restrict__ sdD,
    uint64_t seed, uint32_t stream, double* __restrict__ quat, double* __restrict__ trans,
    double* __restrict__ pT, double* __restrict__ d, double* __restrict__ pD,
    double* __restrict__ vari)
{
    const int l = (int)((blockIdx.x * 256l + threadIdx.x) / GROUP);
    const int lane = threadIdx.x % GROUP;
    if (l >= nImg) return;
    const int nRj = (mR + GROUP - 1 - lane) / GROUP;
    const int nTj = (mT + GROUP - 1 - lane) / GROUP;
    const int nDj = (mD + GROUP - 1 - lane) / GROUP;
    Philox rng(seed, (uint32_t)l, stream, (uint32_t)lane);
    Philox sgn(seed, (uint32_t)l, stream, (uint32_t)lane);
    sgn.ctr.w = 4u * nRj + 2u * nTj + 2u * nDj;

    // ---- rotations (:462-489): r_i = pert_i (+-q), pert ~ sampleACG(k1, k2, k3)
    // (a normalised N(0, diag(1, k1, k2, k3)), DirectionalStat.cpp:39-62, 78-91;
    // the k as given: PERTURB_K_MAX caps perturb's, not these), the sign by
    // gsl_ran_flat(-1, 1) >= 0; no symmetry copy (left to the search)
    double* Q = quat + (size_t)l * mR * 4;
    const double q[4] = {topQuat[4 * (size_t)l], topQuat[4 * (size_t)l + 1],
                         topQuat[4 * (size_t)l + 2], topQuat[4 * (size_t)l + 3]};
    const double sd1 = sqrt(k[3 * (size_t)l]), sd2 = sqrt(k[3 * (size_t)l + 1]);
    const double sd3 = sqrt(k[3 * (size_t)l + 2]);
    for (int i = lane; i < mR; i += GROUP) {
        const double2 g0 = rng.gauss2(), g1 = rng.gauss2();
        double p[4] = {g0.x, g0.y * sd1, g1.x * sd2, g1.y * sd3};
        const double nn = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3]);
        for (int c = 0; c < 4; c++) p[c] /= nn;
        const double s = -1.0 + 2.0 * sgn.uniform() >= 0.0 ? 1.0 : -1.0;
        const double sq[4] = {s * q[0], s * q[1], s * q[2], s * q[3]};
        double r[4];
        thx::sym_qmul(p, sq, r);            // quaternion_mul(part, pert, +-q)
        for (int c = 0; c < 4; c++) Q[4 * i + c] = r[c];
    }

    // ---- translations (:509-530): t_i = topT + (g0 s0, g1 s1)
    // (gsl_ran_bivariate_gaussian, rho 0), pT = balanceWeight(PAR_T)
    double* Tr = trans + (size_t)l * mT * 2;
    const double tx = topTrans[2 * (size_t)l], ty = topTrans[2 * (size_t)l + 1];
    const double s0 = sd[2 * (size_t)l], s1 = sd[2 * (size_t)l + 1];
    for (int i = lane; i < mT; i += GROUP) {
        const double2 g = rng.gauss2();
        Tr[2 * i] = tx + g.x * s0;
        Tr[2 * i + 1] = ty + g.y * s1;
    }
    // ---- defocus factors (:539-551): d_i = topD + g sD, pD = balanceWeight(PAR_D)
    double* D = d + (size_t)l * mD;
    if (mD > 0) {
        const double d0 = topD[l], sD = sdD[l];
        for (int i = lane; i < mD; i += GROUP) D[i] = d0 + rng.gauss2().x * sD;
    }
    thx::wave_mem_sync();
    balance_trans(Tr, pT + (size_t)l * mT, mT, lane);
    double vD = 0.0;
    if (mD > 0) {
        balance_d(D, mD, lane, pD + (size_t)l * mD);
        vD = defocus_sd(D, mD, lane);
    }
    if (vari && lane == 0) vari[6 * (size_t)l + 5] = vD;
}

}  // namespace

extern "C" int thx_pf_load(int nImg, int mR, int mT, int mD, const double* topQuat,
                           const double* k, const double* topTrans, const double* sd,
                           const double* topD, const double* sdD, unsigned long long seed,
                           unsigned stream_id, double* quat, double* trans, double* pR, double* pT,
                           double* d, double* pD, double* vari, thx_stream_t stream)
{
    THX_CHECK_ARG(nImg >= 0, "thx_pf_load: nImg < 0");
    THX_CHECK_ARG(mR > 0 && mT > 0 && mD >= 0,
                  "thx_pf_load: mR=%d, mT=%d must be positive, mD=%d not negative", mR, mT, mD);
    THX_CHECK_ARG((!topD == !sdD) && (!topD == !d) && (!topD == !pD),
                  "thx_pf_load: topD, sdD, d and pD go together");
    if (nImg == 0) return THX_OK;
    THX_CHECK_ARG(topQuat && k && topTrans && sd && quat && trans && pR && pT,
                  "thx_pf_load: null argument");
    THX_CHECK_ARG((mD > 0) == (topD != nullptr),
                  "thx_pf_load: topD, sdD, d and pD are given if and only if mD > 0");
    hipStream_t s = thx::as_stream(stream);
    THX_LAUNCH(k_pf_load, dim3(thx::cdiv((long)nImg * GROUP, 256)), dim3(256), 0, s, nImg, mR, mT,
               mD, topQuat, k, topTrans, sd, topD, sdD, (uint64_t)seed, (uint32_t)stream_id, quat,
               trans, pT, d, pD, vari);
    THX_RET(thx_pf_balance_rot(nImg, mR, quat, pR, stream));
    if (vari) THX_RET(thx::pf_calvari_vari(nImg, mR, quat, mT, trans, vari, s));
    return THX_OK;
}
