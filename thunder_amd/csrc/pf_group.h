// pf_group.h -- the particle statistics' lane group (device): one image per
// GROUP lanes, its sums and sample moments, and the closed-form priors of
// Particle::balanceWeight for translations and defocus factors.  Shared by
// the expectation driver (optimiser.hip) and Particle::load (load.hip).
#pragma once

#include "common.h"

// Particle statistics run one image per GROUP lanes (8 images per wave): the
// 4x4 algebra is repeated by every lane anyway, so narrower groups mean
// fewer waves for the same latency-bound FP64 chains, and each lane's 16
// register-resident particles give the fixed point's quadratic forms ILP.
// Measured on 12 500 x 125 (tools/pf_bench.py, profiles/r02_pf_group_ab.jsonl):
// calVari 0.145 / 0.105 ms at GROUP 16 / 8 on 3-degree clouds, 32 and 64 slower.
constexpr int GROUP = 8;

// v from another lane of the row by DPP (both 32-bit halves)
template <int CTRL>
THX_DEV double dpp_d(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    // every lane's source lies inside its row: no 'old' operand to initialise
    const int lo = __builtin_amdgcn_mov_dpp((int)(unsigned)b, CTRL, 0xf, 0xf, true);
    const int hi = __builtin_amdgcn_mov_dpp((int)(unsigned)(b >> 32), CTRL, 0xf, 0xf, true);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}

// Sum over the GROUP lanes of an image, the same value in every lane.  For
// GROUP 8 by DPP (quad pairs, quad halves, then the row's half mirror pairs
// the two quads): VALU moves instead of three dependent ds_bpermute rounds
// per value, 11 values per fixed-point pass.
THX_DEV double group_sum(double v)
{
    if constexpr (GROUP == 8) {
        v += dpp_d<0xb1>(v);    // quad_perm [1, 0, 3, 2]
        v += dpp_d<0x4e>(v);    // quad_perm [2, 3, 0, 1]
        v += dpp_d<0x141>(v);   // row_half_mirror: lane i <-> 7 - i of its 8
        return v;
    }
#pragma unroll
    for (int o = GROUP / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Mean and sum of squared deviations from it (gsl_stats_mean, and what
// gsl_stats_sd_m divides by n - 1) of each of the C interleaved components
// of the n samples x[C i + c], over the GROUP lanes of an image: every lane
// gets both.  The callers floor and divide, each in its own way.
template <int C>
THX_DEV void group_moments(const double* x, int n, int lane, double* mean, double* ss)
{
    for (int c = 0; c < C; c++) mean[c] = 0.0;
    for (int i = lane; i < n; i += GROUP)
        for (int c = 0; c < C; c++) mean[c] += x[C * i + c];
    for (int c = 0; c < C; c++) mean[c] = group_sum(mean[c]) / n;
    for (int c = 0; c < C; c++) ss[c] = 0.0;
    for (int i = lane; i < n; i += GROUP)
        for (int c = 0; c < C; c++) ss[c] += (x[C * i + c] - mean[c]) * (x[C * i + c] - mean[c]);
    for (int c = 0; c < C; c++) ss[c] = group_sum(ss[c]);
}

// Particle::balanceWeight(PAR_T) (src/Particle.cpp:2342-2375) of the set
// Tr[mT][2] the group's lanes have written and synchronised on: pT = 1 / pdf
// normalised, with the floors sample sd >= 1e-6 (sd = 1 for a single
// particle) and pdf >= 1e-300.
THX_DEV void balance_trans(const double* Tr, double* pTl, int mT, int lane)
{
    double mu[2], ss[2];
    group_moments<2>(Tr, mT, lane, mu, ss);
    const double b0 = fmax(1e-6, mT > 1 ? sqrt(ss[0] / (mT - 1)) : 1.0);
    const double b1 = fmax(1e-6, mT > 1 ? sqrt(ss[1] / (mT - 1)) : 1.0);
    double tot = 0.0;
    for (int i = lane; i < mT; i += GROUP) {
        const double u = (Tr[2 * i] - mu[0]) / b0, v = (Tr[2 * i + 1] - mu[1]) / b1;
        const double p = exp(-(u * u + v * v) / 2) / (2 * M_PI * b0 * b1);
        const double x = 1.0 / fmax(p, 1e-300);
        pTl[i] = x;
        tot += x;
    }
    tot = group_sum(tot);
    for (int i = lane; i < mT; i += GROUP) pTl[i] /= tot;
}

// Particle::calVari(PAR_D) (src/Particle.cpp:1120-1141): gsl_stats_sd of the
// mD samples, 0 for a single one; every lane gets it.
THX_DEV double defocus_sd(const double* D, int mD, int lane)
{
    double m, v;
    group_moments<1>(D, mD, lane, &m, &v);
    return mD > 1 ? sqrt(v / (mD - 1)) : 0.0;
}

// balanceWeight(PAR_D) (src/Particle.cpp:2374-2409): w_i = 1 / N(d_i - m; s)
// with the sample mean m and s = gsl_stats_sd_m (n - 1), 1 when s == 0
// (one sample, or all equal); normW.
THX_DEV void balance_d(const double* D, int mD, int lane, double* pD)
{
    double m, v;
    group_moments<1>(D, mD, lane, &m, &v);
    const double sd = mD > 1 ? sqrt(v / (mD - 1)) : 0.0;
    double tot = 0.0;
    for (int i = lane; i < mD; i += GROUP) {
        const double u = (D[i] - m) / sd;
        const double x = sd == 0.0 ? 1.0 : 1.0 / (exp(-0.5 * u * u) / (sd * sqrt(2 * M_PI)));
        pD[i] = x;
        tot += x;
    }
    tot = group_sum(tot);
    for (int i = lane; i < mD; i += GROUP) pD[i] /= tot;
}
