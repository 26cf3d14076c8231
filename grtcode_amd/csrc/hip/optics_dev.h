// optics_dev.h -- device helpers shared by the optics and solver kernels: Rayleigh optical depth, the two-object
// clear-sky combination, and the block-level trapezoid partial sums of the fused (integrated-output) solvers.
#ifndef GRT_OPTICS_DEV_H_
#define GRT_OPTICS_DEV_H_
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../grt_kernels.h"
#include "exp_pair.h"

#pragma clang fp contract(off)

// shortwave/src/rayleigh.c:38-39
__device__ __forceinline__ double rayleigh_tau(double w, double n)
{
    double const W = w*1.e-4;
    return (n*1.e-20*W*W*W*W)/(0.268675*1.e5*(9.38076E2 - 10.8426*W*W));
}

// Rayleigh + add_optics({gas, rayleigh}) for one (layer, wavenumber) (driver.c:247-270,381-383): with gas
// omega = g = 0 and Rayleigh omega = 1, g = 0 the sums of optics.c:138-145 are, term by term and in that order,
//   g_sum = 0*0*tg + 0*1*tr, o_sum = 0*tg + 1*tr, t_sum = tg + tr.
__device__ __forceinline__ void clear_sky_combine(double tg, double tr, double &tau, double &omega, double &g)
{
    double gs = 0., os = 0., ts = 0.;
    gs += 0.*0.*tg;  os += 0.*tg;  ts += tg;
    gs += 0.*1.*tr;  os += 1.*tr;  ts += tr;
    if (!(gs == 0. && os > 0. && os < 1.7976931348623157e308))
    {
        gs /= os;           // (+0 over a positive finite number is +0: every clear-sky layer skips the division)
    }
    os /= ts;
    g = gs;
    omega = os;
    tau = ts;
}

// add_optics({gas, rayleigh, liquid cloud, ice cloud}) for one (layer, wavenumber) (driver.c:518-530): the sums of
// optics.c:138-145 term by term in that order, gas omega = g = 0 and Rayleigh omega = 1, g = 0 written out as in
// clear_sky_combine.  Cloud terms of zero add exact zeros: a point with no cloud gets clear_sky_combine's doubles.
__device__ __forceinline__ void allsky_combine(double tg, double tr, double tl, double ol, double gl, double ti, double oi,
                                               double gi, double &tau, double &omega, double &g)
{
    double gs = 0., os = 0., ts = 0.;
    gs += 0.*0.*tg;  os += 0.*tg;  ts += tg;
    gs += 0.*1.*tr;  os += 1.*tr;  ts += tr;
    gs += gl*ol*tl;  os += ol*tl;  ts += tl;
    gs += gi*oi*ti;  os += oi*ti;  ts += ti;
    if (!(gs == 0. && os > 0. && os < 1.7976931348623157e308))
    {
        gs /= os;           // (as clear_sky_combine: +0 over a positive finite number is +0)
    }
    os /= ts;
    g = gs;
    omega = os;
    tau = ts;
}

// The solver kernels' cloud arguments: none in the clear-sky instances, one GrtCloudArgs in the all-sky ones (their
// template parameter pack: the clear-sky instances keep their parameter list)
__device__ __forceinline__ GrtCloudArgs cloud_args()
{
    return GrtCloudArgs{0, nullptr, nullptr, nullptr, nullptr, nullptr};
}

__device__ __forceinline__ GrtCloudArgs cloud_args(GrtCloudArgs const &c)
{
    return c;
}

// One cloud object's optics at (layer j, a point that takes band `band`) from a column's band table tab [3][B][L]
// (extinction, albedo, asymmetry; GrtCloudArgs): optical depth = extinction x layer thickness (driver.c:518-526); no band
// (band < 0): no cloud.
__device__ __forceinline__ void cloud_layer(double const *tab, int B, int L, int band, int j, double thickness, double &t,
                                            double &o, double &g)
{
    t = 0.; o = 0.; g = 0.;
    if (band >= 0)
    {
        uint64_t const at = (uint64_t)band*L + j, plane = (uint64_t)B*L;
        t = tab[at]*thickness;
        o = tab[plane + at];
        g = tab[2*plane + at];
    }
}

// ---- the spectral tables' part of the gas optical depth, added where tau is read (GrtContinua, grt_kernels.h) ----
// write_tile's expressions in write_tile's order (gas_optics_dev.h; kernels.c:484-487 and :585-630): the same doubles as
// a gas-optics launch that adds them itself.  A thread owns one grid point and walks the layers: its table entries are
// read ONCE -- the water-vapour four and the first kContinuaRegs linear tables that hold anything at this workgroup's
// points stay in registers; further ones (24 CFC tables that all overlap one workgroup: not a thing) are read per layer.
constexpr int kContinuaRegs = 6;
struct PointContinua
{
    bool h2o;
    double cf, cs, t0f, t0;
    int n, rest_from;                       // tables in registers; first table index not looked at yet
    int k[kContinuaRegs];
    double t[kContinuaRegs];
};

// lo .. hi: the grid points of the calling workgroup (which tables are skipped is decided for all of its threads alike)
__device__ __forceinline__ void continua_load(GrtContinua const &c, uint64_t nw, uint64_t i, long long lo, long long hi,
                                              PointContinua &pc)
{
    pc.h2o = c.has_h2o_ctm && c.spans.h2o_lo < hi && c.spans.h2o_hi > lo;
    pc.cf = pc.cs = pc.t0f = pc.t0 = 0.;
    if (pc.h2o)
    {
        pc.cf = c.h2o_tables[i];
        pc.cs = c.h2o_tables[nw + i];
        pc.t0f = c.h2o_tables[2*nw + i];
        pc.t0 = c.h2o_tables[3*nw + i];
    }
    pc.n = 0;
    int k = 0;
#pragma unroll
    for (int q = 0; q < kContinuaRegs; ++q)
    {
        pc.k[q] = 0;
        pc.t[q] = 0.;
        while (k < c.num_tables && !(c.spans.lo[k] < hi && c.spans.hi[k] > lo))
        {
            ++k;
        }
        if (k < c.num_tables)
        {
            pc.k[q] = k;
            pc.t[q] = c.tables[(uint64_t)k*nw + i];
            pc.n = q + 1;
            ++k;
        }
    }
    pc.rest_from = k;
}

// tau of (layer, point) + the tables' part; col_state: this column's block of GrtContinua.colstate
__device__ __forceinline__ double continua_add(GrtContinua const &c, PointContinua const &pc, double const *col_state,
                                               int layer, uint64_t nw, uint64_t i, long long lo, long long hi, double v)
{
    double const *cont = col_state + c.off_cont + (uint64_t)layer*GRT_MAX_TABLES;
    if (pc.h2o)
    {
        double const *h2o = col_state + c.off_h2o + (uint64_t)layer*4;
        v += h2o[0]*((pc.cs*h2o[1]*grt_exp(pc.t0*h2o[3])) + (pc.cf*h2o[2]*grt_exp(pc.t0f*h2o[3])));
    }
#pragma unroll
    for (int q = 0; q < kContinuaRegs; ++q)
    {
        if (q < pc.n)
        {
            v += cont[pc.k[q]]*pc.t[q];
        }
    }
    for (int k = pc.rest_from; k < c.num_tables; ++k)
    {
        if (c.spans.lo[k] < hi && c.spans.hi[k] > lo)
        {
            v += cont[k]*c.tables[(uint64_t)k*nw + i];
        }
    }
    return v;
}

// Spectral trapezoid of driver.c:302-326 inside a solver: every thread holds its own wavenumber's values of the NV
// rows that are integrated; sum_i 0.5 (f_i + f_{i+1}) dw = sum_i weight_i f_i with weight dw (dw/2 at both ends).
// Wavefront shuffle reduction, then LDS across the block's waves; thread 0 stores the block's NV partial sums at
// partials[(row_base + v)*nblocks + block].  A second tiny launch adds the blocks in a fixed order (deterministic).
template <int NV, int BLOCK>
__device__ __forceinline__ void block_partials(double (&val)[NV], double *partials, uint64_t row_base, unsigned nblocks,
                                               unsigned block)
{
    __shared__ double part[NV][BLOCK/64];
#pragma unroll
    for (int v = 0; v < NV; ++v)
    {
        double s = val[v];
        for (int off = 32; off > 0; off >>= 1)
        {
            s += __shfl_down(s, off, 64);
        }
        if ((threadIdx.x & 63) == 0)
        {
            part[v][threadIdx.x >> 6] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < NV)
    {
        double s = part[threadIdx.x][0];
        for (int k = 1; k < BLOCK/64; ++k)
        {
            s += part[threadIdx.x][k];
        }
        partials[(row_base + threadIdx.x)*nblocks + block] = s;
    }
}

// Profile form of the fused solvers: every level's flux is a row of its own, 2 V rows per column -- more accumulators than
// a thread has registers for, so each level's weighted value is summed across the wave as soon as it is produced, by
// block_partials' shuffle tree, and lane 0 parks the wave's sum at lds[row*(BLOCK/64) + wave].  lds: dynamic LDS of
// nrows*(BLOCK/64) doubles.
template <int BLOCK>
__device__ __forceinline__ void wave_row_sum(double s, double *lds, int row)
{
    for (int off = 32; off > 0; off >>= 1)
    {
        s += __shfl_down(s, off, 64);
    }
    if ((threadIdx.x & 63) == 0)
    {
        lds[row*(BLOCK/64) + (threadIdx.x >> 6)] = s;
    }
}

// ... and after the sweeps: the waves' sums of each row added in wave order (block_partials' association: a row that is
// also one of the six-row form's gets the same bits), stored at partials[(row_base + row)*nblocks + block].
template <int BLOCK>
__device__ __forceinline__ void block_row_partials(double const *lds, int nrows, double *partials, uint64_t row_base,
                                                   unsigned nblocks, unsigned block)
{
    __syncthreads();
    for (int r = threadIdx.x; r < nrows; r += BLOCK)
    {
        double s = lds[r*(BLOCK/64)];
        for (int k = 1; k < BLOCK/64; ++k)
        {
            s += lds[r*(BLOCK/64) + k];
        }
        partials[(row_base + r)*nblocks + block] = s;
    }
}

#endif
