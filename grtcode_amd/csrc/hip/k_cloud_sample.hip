// k_cloud_sample.hip -- cloud subcolumns sampled on the device (grt_ext.h: grt_cloud_sampler_run).
// One sample (column, pass, subcolumn, band) is the clouds library's sample_subcolumn followed by its pade_band of liquid
// and ice for every layer (grt_clouds.c: sample_subcolumn, beta_lookup, ice_size, pade_band), restated operation for
// operation: double, + - x / only, no contraction, so that the tables equal the host's to the last bit.
//
// Shape: one wavefront per sample, four samples per workgroup, lanes over the layers in chunks of 64.  The sequential
// "rank[i+1] = rank[i] where decide[i] <= overlap[i]" is resolved per chunk with one ballot: a lane whose layer does not
// copy is a head, every lane takes the rank of the nearest head at or below it (bit operations on the 64-bit mask, one
// shuffle), and the last lane's resolved rank is carried into the next chunk.  What does not depend on the layer is
// worked out once per wave: the liquid's three Pade quotients (one radius for the whole call) and the ice's for each of
// the eight temperature classes (lane k holds class k; a layer fetches its class with a shuffle).  The three rows of the
// beta tables a (5, 5) water PDF reads are staged in LDS per workgroup (tables of up to kBetaLdsPoints abscissae;
// larger ones are read from global memory), and the segment is found by bisection: the first x_i > at of the ascending
// x, the one the library's linear scan stops at.  Stores run along the layers: contiguous per property plane.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../grt_kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kWaves = 4;
constexpr int kBlock = 64*kWaves;
constexpr int kBetaLdsPoints = 1024;               // 3 rows x 8 bytes x 1024 = 24 KiB of LDS at the most

// incomplete_beta.c:32-64 / beta_lookup: the segment [x_{i-1}, x_i] with the first x_i > at, i in 1 .. nx - 2, else the
// last one; slope, then intercept, then the line
__device__ inline double beta_lookup(double const *x, double const *y, int nx, double at)
{
    int lo = 1, hi = nx - 1;
    while (lo < hi)
    {
        int const mid = (lo + hi) >> 1;
        if (x[mid] > at) hi = mid; else lo = mid + 1;
    }
    double const slope = (y[lo] - y[lo - 1])/(x[lo] - x[lo - 1]);
    double const intercept = y[lo] - slope*x[lo];
    return slope*at + intercept;
}

__device__ inline double horner(double const *c, int n, double x)
{
    double v = c[0];
    for (int i = 1; i < n; ++i)
    {
        v = c[i] + x*v;
    }
    return v;
}

// pade_band without the content: the three quotients of band b at this radius; false: no size regime holds the radius
__device__ inline bool pade_quotients(GrtCloudPhaseDev const &o, int b, double radius, double &ext, double &ssa, double &asy)
{
    int s = 0;
    while (s < o.nsize && !(o.size_lo[s] <= radius && o.size_hi[s] >= radius))
    {
        ++s;
    }
    ext = ssa = asy = 0.;
    if (s == o.nsize)
    {
        return false;
    }
    double const dr = radius - o.size_ref[s];
    size_t const at = (size_t)b*(size_t)o.nsize + (size_t)s;
    ext = horner(o.coef[0] + at*(size_t)o.np, o.np, dr)/horner(o.coef[1] + at*(size_t)o.nq, o.nq, dr);
    ssa = horner(o.coef[2] + at*(size_t)o.np, o.np, dr)/horner(o.coef[3] + at*(size_t)o.nq, o.nq, dr);
    asy = horner(o.coef[4] + at*(size_t)o.np, o.np, dr)/horner(o.coef[5] + at*(size_t)o.nq, o.nq, dr);
    return true;
}

// clouds_lib.c:47-82: the temperature class of a layer, and a class's crystal size [microns]
__device__ inline int ice_class(double t)
{
    double const below_freezing[7] = {25., 30., 35., 40., 45., 50., 55.};
    double const tfreeze = 273.16;
    int k = 0;
    while (k < 7 && !(t > tfreeze - below_freezing[k]))
    {
        ++k;
    }
    return k;
}

__device__ inline double ice_class_size(int k)
{
    double const size[8] = {100.6, 80.8, 93.5, 63.9, 42.5, 39.9, 21.6, 20.2};
    return size[k];
}

// Philox4x32-10 (Salmon et al., SC11): ten rounds, the key bumped between rounds
__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                     uint32_t r[4])
{
    for (int round = 0; round < 10; ++round)
    {
        if (round > 0)
        {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        uint64_t const p0 = (uint64_t)0xD2511F53u*c0, p1 = (uint64_t)0xCD9E8D57u*c2;
        uint32_t const n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
    }
    r[0] = c0; r[1] = c1; r[2] = c2; r[3] = c3;
}

// 53 bits of two words as a double in [0, 1)
__device__ inline double unit_interval(uint32_t hi, uint32_t lo)
{
    return ((double)(hi >> 5)*67108864. + (double)(lo >> 6))*(1./9007199254740992.);
}

__global__ __launch_bounds__(kBlock) void cloud_sample_kernel(GrtCloudSampleArgs a, int beta_in_lds)
{
    extern __shared__ double beta_rows[];          // [3][num_x]: x, inverse (5, 5), value (6, 5)
    int const lane = threadIdx.x & 63;
    int const wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int const nx = a.num_x;
    double const *bx = a.x, *binv = a.inverse_pq, *bval = a.value_p1q;
    if (beta_in_lds)
    {
        for (int j = threadIdx.x; j < nx; j += kBlock)
        {
            beta_rows[j] = a.x[j];
            beta_rows[nx + j] = a.inverse_pq[j];
            beta_rows[2*nx + j] = a.value_p1q[j];
        }
        __syncthreads();
        bx = beta_rows;
        binv = beta_rows + nx;
        bval = beta_rows + 2*nx;
    }
    int const L = a.num_layers, S = a.subcolumns, B = a.num_bands;
    uint64_t const total = (uint64_t)a.ncol*2*(uint64_t)S*(uint64_t)B;
    uint64_t const sample = (uint64_t)blockIdx.x*kWaves + (uint64_t)wave;
    if (sample >= total)
    {
        return;                                    // (a whole wave: nothing below waits for the workgroup)
    }
    // libc's order of a driver's draws: column, pass, subcolumn, band
    int const band = (int)(sample % (uint64_t)B);
    uint64_t rest = sample/(uint64_t)B;
    int const s = (int)(rest % (uint64_t)S);
    rest /= (uint64_t)S;
    int const pass = (int)(rest & 1);
    int const c = (int)(rest >> 1);

    // what the layers share: the liquid's quotients, and -- lane k, k < 8 -- the ice's of temperature class k
    double l_ext, l_ssa, l_asy, i_ext, i_ssa, i_asy;
    bool const l_held = pade_quotients(a.liquid, band, a.liquid_radius, l_ext, l_ssa, l_asy);
    int const i_held = pade_quotients(a.ice, band, ice_class_size(lane & 7)/2.0, i_ext, i_ssa, i_asy) ? 1 : 0;

    size_t const col = (size_t)c*(size_t)L;
    double const *cfp = a.cloud_fraction + col, *lwp = a.liquid_content + col, *iwp = a.ice_content + col;
    double const *tp = a.temperature + col;
    double const *ovp = a.overlap + (size_t)c*(size_t)(L - 1);
    double const *u = a.uniforms != nullptr ? a.uniforms + sample*(uint64_t)(2*L - 1) : nullptr;
    size_t const plane = (size_t)B*(size_t)L;
    // set 2 pass + phase, subcolumn-major: [4][S][ncol][3][B][L]
    double *liquid = a.tables + ((((size_t)(2*pass)*(size_t)S + (size_t)s)*(size_t)a.ncol + (size_t)c)*3*(size_t)B +
                                 (size_t)band)*(size_t)L;
    double *ice = liquid + (size_t)S*(size_t)a.ncol*3*plane;

    double carry_rank = 0.;
    int carry_copies = 0;                          // the chunk's first layer takes the rank of the layer before it
    for (int base = 0; base < L; base += 64)
    {
        int const i = base + lane;
        bool const in = i < L, has_next = i + 1 < L;
        double rank = 0., decide = 0.;
        if (u != nullptr)
        {
            if (in) rank = u[i];
            if (has_next) decide = u[L + i];
        }
        else
        {
            uint32_t r[4];
            philox4x32_10((uint32_t)i, (uint32_t)band, (uint32_t)(pass*GRT_SAMPLER_MAX_SUBCOLUMNS + s),
                          a.column0 + (uint32_t)c, a.key0, a.key1, r);
            rank = unit_interval(r[0], r[1]);
            decide = unit_interval(r[2], r[3]);
        }
        // layer i + 1 takes layer i's (resolved) rank where decide[i] <= overlap[i]: copies cascade down the column
        int const next_copies = has_next && decide <= ovp[i] ? 1 : 0;
        int const from_below = __shfl_up(next_copies, 1);
        int const copies = lane == 0 ? carry_copies : from_below;
        unsigned long long const heads = __ballot(!copies);
        unsigned long long const mine = heads & ((2ull << lane) - 1ull);       // heads at or below this lane
        double r = __shfl(rank, mine != 0 ? 63 - __builtin_clzll(mine) : 0);
        if (mine == 0)
        {
            r = carry_rank;
        }
        carry_rank = __shfl(r, 63);
        carry_copies = __shfl(next_copies, 63);

        double ql = 0., qi = 0., t = 0.;
        if (in)
        {
            double const cf = cfp[i], lwc = lwp[i], iwc = iwp[i];
            t = tp[i];
            if (r > (1. - cf))
            {
                // stochastic_clouds.c:94-120 with the (p, q) = (5, 5) PDF: p/(p + q) = 5/10
                double const qs = beta_lookup(bx, binv, nx, 1. - cf);
                double const width = (lwc + iwc)/((5./10.)*(1. - beta_lookup(bx, bval, nx, qs)) - qs*cf);
                double const total_water = width*(beta_lookup(bx, binv, nx, r) - qs);
                double const liquid_fraction = lwc/(lwc + iwc);
                ql = total_water*liquid_fraction;
                qi = total_water*(1. - liquid_fraction);
            }
        }
        int const k = ice_class(t);
        double const ke = __shfl(i_ext, k), ks = __shfl(i_ssa, k), ka = __shfl(i_asy, k);
        int const kheld = __shfl(i_held, k);
        if (in)
        {
            bool const wet = l_held && ql > 0., icy = kheld != 0 && qi > 0.;
            liquid[i] = wet ? ql*l_ext : 0.;
            liquid[plane + i] = wet ? l_ssa : 0.;
            liquid[2*plane + i] = wet ? l_asy : 0.;
            ice[i] = icy ? qi*ke : 0.;
            ice[plane + i] = icy ? ks : 0.;
            ice[2*plane + i] = icy ? ka : 0.;
        }
    }
}

}  // namespace

extern "C" int grt_launch_cloud_sample(void *stream, GrtCloudSampleArgs const *a)
{
    if (a == nullptr || a->ncol < 1 || a->num_layers < 1 || a->subcolumns < 1 ||
        a->subcolumns > GRT_SAMPLER_MAX_SUBCOLUMNS || a->num_bands < 1 || a->num_x < 2 || a->x == nullptr ||
        a->inverse_pq == nullptr || a->value_p1q == nullptr || a->liquid.nsize < 1 || a->ice.nsize < 1 ||
        a->liquid.np < 1 || a->liquid.nq < 1 || a->ice.np < 1 || a->ice.nq < 1 || a->cloud_fraction == nullptr ||
        a->liquid_content == nullptr || a->ice_content == nullptr || a->temperature == nullptr ||
        (a->num_layers > 1 && a->overlap == nullptr) || a->tables == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    uint64_t const samples = (uint64_t)a->ncol*2*(uint64_t)a->subcolumns*(uint64_t)a->num_bands;
    uint64_t const blocks = (samples + kWaves - 1)/kWaves;
    if (blocks > 0x7fffffffull)
    {
        return (int)hipErrorInvalidValue;
    }
    int const in_lds = a->num_x <= kBetaLdsPoints;
    size_t const lds = in_lds ? sizeof(double)*3*(size_t)a->num_x : 0;
    hipLaunchKernelGGL(cloud_sample_kernel, dim3((unsigned)blocks), dim3(kBlock), lds, (hipStream_t)stream, *a, in_lds);
    return (int)hipGetLastError();
}
