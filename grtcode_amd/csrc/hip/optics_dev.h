// optics_dev.h -- device helpers shared by the optics and solver kernels: Rayleigh optical depth, the two-object
// clear-sky combination, the fused solvers' layer optics (LayerOptics), where a solver's level fluxes go (LevelSink),
// and the block-level trapezoid partial sums of the fused (integrated-output) solvers.
#ifndef GRT_OPTICS_DEV_H_
#define GRT_OPTICS_DEV_H_
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../grt_kernels.h"
#include "exp_pair.h"

#pragma clang fp contract(off)

// workgroup of the solvers' chain and fused forms (grt_solver_blocks: the partial sums of one launch)
constexpr int kSolverBlock = GRT_SOLVER_BLOCK;

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

// add_optics({gas, rayleigh, aerosol}) for one (layer, wavenumber) (driver.c:426-434): the sums of optics.c:138-145 term by
// term in that order, as clear_sky_combine and allsky_combine write them.  An aerosol of exact zeros adds exact zeros: a
// point with no aerosol gets clear_sky_combine's doubles.
__device__ __forceinline__ void aerosol_combine(double tg, double tr, double ta, double oa, double ga, double &tau,
                                                double &omega, double &g)
{
    double gs = 0., os = 0., ts = 0.;
    gs += 0.*0.*tg;  os += 0.*tg;  ts += tg;
    gs += 0.*1.*tr;  os += 1.*tr;  ts += tr;
    gs += ga*oa*ta;  os += oa*ta;  ts += ta;
    if (!(gs == 0. && os > 0. && os < 1.7976931348623157e308))
    {
        gs /= os;           // (as clear_sky_combine: +0 over a positive finite number is +0)
    }
    os /= ts;
    g = gs;
    omega = os;
    tau = ts;
}

// add_optics({gas, rayleigh, aerosol, liquid cloud, ice cloud}) for one (layer, wavenumber): the physically complete set,
// the sums of optics.c:138-145 term by term in that order -- the aerosol in slot 2, where driver.c:426-434 puts it, the
// clouds behind it as in driver.c:518-530.  An aerosol of exact zeros adds exact zeros before the clouds: allsky_combine's
// doubles; clouds of exact zeros add exact zeros after the aerosol: aerosol_combine's doubles.
__device__ __forceinline__ void sky_combine(double tg, double tr, double ta, double oa, double ga, double tl, double ol,
                                            double gl, double ti, double oi, double gi, double &tau, double &omega,
                                            double &g)
{
    double gs = 0., os = 0., ts = 0.;
    gs += 0.*0.*tg;  os += 0.*tg;  ts += tg;
    gs += 0.*1.*tr;  os += 1.*tr;  ts += tr;
    gs += ga*oa*ta;  os += oa*ta;  ts += ta;
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

// ---- fixed-order sums: the bit identities between the fused forms rest on every one of them adding in these orders ----
// WAVE_SUM(s);  the double variable s of the 64 lanes of a wave by a shuffle tree; lane 0's s holds the sum.  (A statement
// macro: as a function the tree comes out of the compiler in another instruction order in the level-sum instances.)
#define WAVE_SUM(s) do { for (int off_ = 32; off_ > 0; off_ >>= 1) { (s) += __shfl_down((s), off_, 64); } } while (0)

// a row of n block partial sums by one wave: lane-strided, then WAVE_SUM; lane 0 holds the sum
__device__ __forceinline__ double wave_strided_sum(double const *p, unsigned n)
{
    double s = 0.;
    for (unsigned b = threadIdx.x; b < n; b += 64)
    {
        s += p[b];
    }
    WAVE_SUM(s);
    return s;
}

// the sums the WAVES waves of a workgroup left at part[0 .. WAVES - 1], in wave order
template <int WAVES>
__device__ __forceinline__ double waves_sum(double const *part)
{
    double s = part[0];
    for (int k = 1; k < WAVES; ++k)
    {
        s += part[k];
    }
    return s;
}

// ---- what joins gas and Rayleigh in a solver kernel instance: its parameter pack ----
// lw_kernel / sw_kernel take their joined arguments as a pack after the band's own (GrtSolverInstance, grt_kernels.h:
// nothing, GrtCloudArgs, GrtAerosolArgs or GrtSubcolumnArgs, a GrtAerosolArgs behind a GrtCloudArgs or a GrtSubcolumnArgs
// where both join, and a GrtBandArgs last in the per-bin instances), so that an
// instance's kernel arguments hold what it reads and nothing else.  has<T, Pack...>: whether the pack holds a T;
// pick<T>(pack...): that element, or a T of zeros and null pointers.
template <typename T, typename... Pack> constexpr bool has = (std::is_same_v<T, Pack> || ... || false);

template <typename T>
__device__ __forceinline__ T pick()
{
    return T{};
}

template <typename T, typename First, typename... Rest>
__device__ __forceinline__ T pick(First const &first, Rest const &...rest)
{
    if constexpr (std::is_same_v<T, First>)
    {
        return first;
    }
    else
    {
        return pick<T>(rest...);
    }
}

// the cloud tables of an instance: its GrtCloudArgs, or its GrtSubcolumnArgs' (all-sky: the pack holds either)
template <typename... Pack> constexpr bool has_clouds = has<GrtCloudArgs, Pack...> || has<GrtSubcolumnArgs, Pack...>;

template <typename... Pack>
__device__ __forceinline__ GrtCloudArgs pick_clouds(Pack const &...pack)
{
    if constexpr (has<GrtSubcolumnArgs, Pack...>)
    {
        return pick<GrtSubcolumnArgs>(pack...).clouds;
    }
    else
    {
        return pick<GrtCloudArgs>(pack...);
    }
}

// What grid row blockIdx.y stands for: col, the column whose gas state (tau_gas, temperatures, sun) and aerosol table it
// reads; tab, its cloud tables' column; slot, its partial sums' column; park, its rows of the shortwave park block; sun,
// where its cosine of the zenith angle lies (the zenith instances: in the join's mu).  All are blockIdx.y but in the
// subcolumn instances (GrtSubcolumnArgs: row y is column y / count, subcolumn first + y % count), in the zenith instances
// (GrtZenithArgs: row y is column y / count, angle first + y % count; the slot is c zeniths + k, and so is sun) and in the
// instances that hold both (row y is column y / (draws x angles), draw s and angle k from the remainder, the angles of a
// draw next to each other; the slot is (c zeniths + k) subcolumns + s, sun stays c zeniths + k).
struct SolverRow { int col, tab, slot, park, sun; };

template <typename... Pack>
__device__ __forceinline__ SolverRow solver_row(int ncol, Pack const &...pack)
{
    int const y = blockIdx.y;
    if constexpr (has<GrtSubcolumnArgs, Pack...> && has<GrtZenithArgs, Pack...>)
    {
        GrtSubcolumnArgs const sc = pick<GrtSubcolumnArgs>(pack...);
        GrtZenithArgs const zn = pick<GrtZenithArgs>(pack...);
        int const per = sc.count*zn.count;
        int const c = y/per;
        int const rest = y - c*per;
        int const ds = rest/zn.count;
        int const s = sc.first + ds;
        int const k = zn.first + (rest - ds*zn.count);
        int const sun = c*zn.zeniths + k;
        return SolverRow{c, s*ncol + c, sun*sc.subcolumns + s, y, sun};
    }
    else if constexpr (has<GrtSubcolumnArgs, Pack...>)
    {
        GrtSubcolumnArgs const sc = pick<GrtSubcolumnArgs>(pack...);
        int const c = y/sc.count;
        int const s = sc.first + (y - c*sc.count);
        return SolverRow{c, s*ncol + c, c*sc.subcolumns + s, y, c};
    }
    else if constexpr (has<GrtZenithArgs, Pack...>)
    {
        GrtZenithArgs const zn = pick<GrtZenithArgs>(pack...);
        int const c = y/zn.count;
        int const k = zn.first + (y - c*zn.count);
        return SolverRow{c, c, c*zn.zeniths + k, y, c*zn.zeniths + k};
    }
    else
    {
        return SolverRow{y, y, y, y, y};
    }
}

// The chunk of a tile kernel's workgroup (sw_tile_kernel, lw_tile_kernel; GrtTileArgs): grid row y is the six-row
// instance's `row`, blockIdx.z a chunk of TN consecutive tiles from k0 on.  Tile k0 + u is live(u) when the column has it;
// it is tile c T + k0 + u of the launch, and its partial sums lie at slot (c T + k0 + u) S + draw (the kernels say both where
// they use them: a member per rule costs lw_tile_kernel instructions).
template <int TN>
struct TileChunk
{
    int T, k0, S, draw;

    template <typename... Pack>
    __device__ __forceinline__ TileChunk(GrtTileArgs const &tl, SolverRow const &row, Pack const &...pack)
    {
        T = tl.tiles;
        k0 = (tl.chunk_first + (int)blockIdx.z)*TN;
        S = 1;
        if constexpr (has<GrtSubcolumnArgs, Pack...>)
        {
            S = pick<GrtSubcolumnArgs>(pack...).subcolumns;
        }
        draw = row.slot - row.col*S;
    }
    __device__ __forceinline__ bool live(int u) const { return k0 + u < T; }
};

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

// The aerosol object at (layer j, wavenumber w) from one interval's block tab [3][NI][2][L] + interval*2 L of a column's
// table (GrtAerosolArgs: tau, omega, g; slope then intercept): linear_sample's m w + b (utilities.c:235-246); no interval
// (interval < 0): no aerosol.  plane = NI 2 L, the doubles from one property to the next.
__device__ __forceinline__ void aerosol_layer(double const *tab, uint64_t plane, int L, int interval, int j, double w,
                                              double &t, double &o, double &g)
{
    t = 0.; o = 0.; g = 0.;
    if (interval >= 0)
    {
        double const *q = tab + j;
        t = q[0]*w + q[L];
        o = q[plane]*w + q[plane + L];
        g = q[2*plane]*w + q[2*plane + L];
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
// WAVE_SUM, then waves_sum across the block's waves through LDS; thread v stores row v's sum at
// partials[(row_base + v)*nblocks + block].  A second tiny launch adds the blocks in a fixed order (deterministic).
// SPLIT < NV: the rows from SPLIT on go to a second array, row v at partials2[(row_base2 + v - SPLIT)*nblocks + block]
// (the direct-beam rows beside the six: summed as the six are, stored apart).
template <int NV, int BLOCK, int SPLIT = NV>
__device__ __forceinline__ void block_partials(double (&val)[NV], double *partials, uint64_t row_base, unsigned nblocks,
                                               unsigned block, double *partials2 = nullptr, uint64_t row_base2 = 0)
{
    __shared__ double part[NV][BLOCK/64];
#pragma unroll
    for (int v = 0; v < NV; ++v)
    {
        double s = val[v];
        WAVE_SUM(s);
        if ((threadIdx.x & 63) == 0)
        {
            part[v][threadIdx.x >> 6] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x < SPLIT)
    {
        partials[(row_base + threadIdx.x)*nblocks + block] = waves_sum<BLOCK/64>(part[threadIdx.x]);
    }
    else if (SPLIT < NV && threadIdx.x < NV)
    {
        partials2[(row_base2 + threadIdx.x - SPLIT)*nblocks + block] = waves_sum<BLOCK/64>(part[threadIdx.x]);
    }
}

// Profile form of the fused solvers: every level's flux is a row of its own, 2 V rows per column -- more accumulators than
// a thread has registers for, so each level's weighted value is summed across the wave as soon as it is produced, by
// WAVE_SUM, and lane 0 parks the wave's sum at lds[row*(BLOCK/64) + wave].  lds: dynamic LDS of
// nrows*(BLOCK/64) doubles.
template <int BLOCK>
__device__ __forceinline__ void wave_row_sum(double s, double *lds, int row)
{
    WAVE_SUM(s);
    if ((threadIdx.x & 63) == 0)
    {
        lds[row*(BLOCK/64) + (threadIdx.x >> 6)] = s;
    }
}

// ... and after the sweeps: the waves' sums of each row by waves_sum (as block_partials: a row that is also one of the
// six-row form's gets the same bits), stored at partials[(row_base + row)*nblocks + block].
template <int BLOCK>
__device__ __forceinline__ void block_row_partials(double const *lds, int nrows, double *partials, uint64_t row_base,
                                                   unsigned nblocks, unsigned block)
{
    __syncthreads();
    for (int r = threadIdx.x; r < nrows; r += BLOCK)
    {
        partials[(row_base + r)*nblocks + block] = waves_sum<BLOCK/64>(lds + r*(BLOCK/64));
    }
}

// driver.c:302-326: sum 0.5 (f_i + f_{i+1}) dw over the grid = sum weight_i f_i -- dw, dw/2 at both ends, and 0 for
// the idle lanes of the last block
__device__ __forceinline__ double trapezoid_weight(uint64_t i, uint64_t nw, double dw, bool live)
{
    return !live ? 0. : ((i == 0 || i + 1 == nw) ? 0.5*dw : dw);
}

// The fused forms' layer optics: tau, omega, g of (layer j, point ii) formed in registers from tau_gas -- the spectral
// tables' part added if the gas-optics launch left it to the solver (a table entry read once per point), Rayleigh, and
// clear_sky_combine (the expressions and order of clear_sky_kernel: identical values).  ALLSKY: the liquid and ice cloud
// objects join (GrtCloudArgs): the point reads its two band indices once, each layer forms the two objects from the
// column's band tables and allsky_combine adds the four.  Built once per thread from the fields both solvers' argument
// structs carry; FUSED false (the spectral forms, which read their optics): nothing is loaded.  tab: the column of the
// cloud tables (SolverRow; col but in the subcolumn instances).  AEROSOL (clear-sky forms): the aerosol object joins
// (GrtAerosolArgs): the point reads its interval once, each layer forms the object from the column's slope and intercept
// table (six loads, three multiply-adds) and aerosol_combine adds the three.  The aerosol table is the column's, whatever
// the subcolumn: it is indexed by col, never by tab.  ALLSKY and AEROSOL: both join, and sky_combine adds the five; the
// aerosol's slopes and intercepts are loaded per layer, as in the aerosol forms, so the thread holds the two band indices,
// one interval and one more pointer on top of the all-sky forms' state.
template <bool FUSED, bool ALLSKY, bool AEROSOL = false>
struct LayerOptics
{
    GrtContinua const *c;
    double const *tau, *nl, *cstate;
    double w;
    uint64_t nw, ii;
    long long blk_lo, blk_hi;
    bool add_continua;
    PointContinua pc;
    GrtCloudArgs cl;
    int L, col, band_l, band_i;
    uint64_t ctab;
    double const *atab;                     // AEROSOL: the column's table at this point's interval
    uint64_t aplane;
    int ainterval;

    template <typename Args>
    __device__ __forceinline__ LayerOptics(Args const &a, GrtCloudArgs const &cl_, int col_, int tab, uint64_t ii_,
                                           GrtAerosolArgs const &ae = GrtAerosolArgs{0, nullptr, nullptr})
    {
        L = a.num_levels - 1;
        col = col_;
        ii = ii_;
        nw = a.nw;
        w = a.w0 + ii*a.dw;
        tau = a.tau_gas + (uint64_t)col*a.optics_stride + ii;
        nl = a.n_layer + (uint64_t)col*L;
        c = &a.continua;
        blk_lo = (long long)blockIdx.x*kSolverBlock;
        blk_hi = blk_lo + kSolverBlock < (long long)nw ? blk_lo + kSolverBlock : (long long)nw;
        add_continua = FUSED && a.add_continua;
        cstate = c->colstate + (uint64_t)col*c->stride;
        if (add_continua)
        {
            continua_load(*c, nw, ii, blk_lo, blk_hi, pc);
        }
        cl = cl_;
        band_l = ALLSKY ? cl.band_liquid[ii] : -1;
        band_i = ALLSKY ? cl.band_ice[ii] : -1;
        ctab = ALLSKY ? (uint64_t)tab*3*(uint64_t)cl.num_bands*L : 0;
        ainterval = AEROSOL ? ae.interval[ii] : -1;
        aplane = AEROSOL ? 2*(uint64_t)ae.num_intervals*L : 0;
        atab = AEROSOL ? ae.tables + (uint64_t)col*3*aplane + (uint64_t)(ainterval < 0 ? 0 : ainterval)*2*L : nullptr;
    }

    __device__ __forceinline__ void at(int j, double &t, double &om, double &gg) const
    {
        double tg = tau[(uint64_t)j*nw];
        if (add_continua)
        {
            tg = continua_add(*c, pc, cstate, j, nw, ii, blk_lo, blk_hi, tg);
        }
        if constexpr (ALLSKY && AEROSOL)
        {
            double const th = cl.thickness[(uint64_t)col*L + j];
            double at_, ao, ag, lt, lo, lg, it, io, ig;
            aerosol_layer(atab, aplane, L, ainterval, j, w, at_, ao, ag);
            cloud_layer(cl.liquid + ctab, cl.num_bands, L, band_l, j, th, lt, lo, lg);
            cloud_layer(cl.ice + ctab, cl.num_bands, L, band_i, j, th, it, io, ig);
            sky_combine(tg, rayleigh_tau(w, nl[j]), at_, ao, ag, lt, lo, lg, it, io, ig, t, om, gg);
        }
        else if constexpr (ALLSKY)
        {
            double const th = cl.thickness[(uint64_t)col*L + j];
            double lt, lo, lg, it, io, ig;
            cloud_layer(cl.liquid + ctab, cl.num_bands, L, band_l, j, th, lt, lo, lg);
            cloud_layer(cl.ice + ctab, cl.num_bands, L, band_i, j, th, it, io, ig);
            allsky_combine(tg, rayleigh_tau(w, nl[j]), lt, lo, lg, it, io, ig, t, om, gg);
        }
        else if constexpr (AEROSOL)
        {
            double at_, ao, ag;
            aerosol_layer(atab, aplane, L, ainterval, j, w, at_, ao, ag);
            aerosol_combine(tg, rayleigh_tau(w, nl[j]), at_, ao, ag, t, om, gg);
        }
        else
        {
            clear_sky_combine(tg, rayleigh_tau(w, nl[j]), t, om, gg);
        }
    }
};

// One window of a window table (grt_kernels.h): its five ints by name, each read where a kernel asks for it.  Three
// rules on them are written out at the kernels' sites, each marked `(Window: <rule>)`, because a member function that holds
// one moves instructions in every kernel it was tried in; the canonical forms, which a site writes in its own integer width:
//   pair    the window's pair in solver block b, one it has a point in:   first_pair + b - first_block
//   span    grid point i is one of its points:                            0 <= i - first < count
//   weight  ... and its weight there:                                     weights[weight_at + (i - first)]
struct Window
{
    int const *e;
    __device__ __forceinline__ int first() const { return e[0]; }
    __device__ __forceinline__ int count() const { return e[1]; }
    __device__ __forceinline__ int weight_at() const { return e[2]; }
    __device__ __forceinline__ int first_block() const { return e[3]; }
    __device__ __forceinline__ int first_pair() const { return e[4]; }
    // the blocks it has a point in, which is how many pairs it has
    __device__ __forceinline__ int blocks() const { return (e[0] + e[1] - 1)/kSolverBlock - e[3] + 1; }
};
// window k of the entries (K: the index arithmetic of the site), and the q-th window of a block list
template <typename K>
__device__ __forceinline__ Window window_at(int const *entries, K k)
{
    return Window{entries + (K)GRT_WINDOW_INTS*k};
}
template <typename K = int>
__device__ __forceinline__ Window window_of(int const *entries, int const *block_list, int q)
{
    return window_at<K>(entries, block_list[q]);
}

// Where a solver's level fluxes go, level lev top first.  Spectral forms (FUSED false): the rows flux_up / flux_down
// [V][nw] at this thread's point.  Fused form: the six integrated output rows in registers (up TOA, up surface, up user,
// down TOA, down surface, down user) and, at finish(), their trapezoid partial sums (block_partials).  PROFILE (fused
// form only): every level's upward and downward flux leaves instead, 2 V rows per column: each level's weighted value is
// summed across the wave where the sweep produces it, the waves' sums wait in dynamic LDS (2 V x kSolverBlock/64
// doubles) and finish() stores the block's sums at partials[(c*2 V + r)*nblocks + block], r = level (up), V + level
// (down).  Same association as block_partials: the six-row form's rows come out the same to the bit.
// SPECTRAL (fused six-row form only): finish() also stores each live point's six values, unweighted, to the caller's
// rows -- up TOA, surface, user at flux_up + c flux_stride + k nw (k = 0, 1, 2), down at flux_down + ... -- before it
// weights them (grt_pipeline_run_spectral).
// BANDED (profile form only; grt_pipeline_run_band_profiles): a level's flux leaves once per wavenumber bin that has a
// point in this workgroup (GrtBandArgs: grt_bin_table's list for the block), weighted with that bin's trapezoid weights
// (bin_partials_kernel's rule).  A workgroup inside one bin keeps one weight per point and does the profile form's work;
// one that holds edges sums each level once per bin, the weight formed from the bin's two edges where it is used.  The
// waves' sums wait in dynamic LDS, [bins of the block][2 V][kSolverBlock/64], and finish() stores bin b's at
// partials[(c*2 V + r)*per_row + offset(b) + block - first_block(b)].
// DIRECT (shortwave, fused six-row and profile forms; GrtDirectArgs): the direct beam at a level leaves too, by
// put_direct() -- three more rows in registers (TOA, surface, user) that ride with the six through block_partials, or V
// more rows of wave sums behind the 2 V in dynamic LDS (3 V x kSolverBlock/64 doubles) --, to the join's own partial sums.
// The longwave's surface-temperature Jacobian (GrtJacobianArgs) is the same third row group: lw_kernel hands every level's
// dF_up/dT_surf to put_direct() and its partial sums' array in a GrtDirectArgs.
// RESPONSES (profile form only, with or without DIRECT; GrtResponseArgs, grt_pipeline_run_sky_weighted): the broadband
// group of G V rows (G = 2, 3 with DIRECT) is summed as without it -- x*pwt, the same wave_row_sum, the same rows --, and
// each response of the block's list (block_start / block_list: an explicit list, responses overlap) gets a group of G V
// wave sums of its own behind it, of x*(pwt*r).  The products pwt*r of the list wait in dynamic LDS behind the wave sums,
// [responses of the block][kSolverBlock], written once by the constructor -- each thread writes and reads its own entries
// only, so no barrier is needed --: a list indexed per thread in registers would live in scratch memory.  finish() stores
// response q's sums at its partials[(slot P + pair) G V + r], pair = first pair + block - first block of the response.  A
// workgroup with an empty list does exactly the profile form's work.
template <bool ON> struct DirectRows {};
template <> struct DirectRows<true> { double out[3]; double *partials; };
template <bool ON> struct ResponseRows {};
template <> struct ResponseRows<true> { GrtResponseArgs a; int lo, count; double const *wt; };

template <bool FUSED, bool PROFILE, bool SPECTRAL = false, bool BANDED = false, bool DIRECT = false, bool RESPONSES = false>
struct LevelSink
{
    static_assert(!DIRECT || (FUSED && !SPECTRAL && !BANDED), "the direct beam leaves the six-row and profile forms");
    static_assert(!RESPONSES || (PROFILE && !BANDED), "the response rows leave the profile form");
    static constexpr int GROUPS = DIRECT ? 3 : 2;   // RESPONSES: row groups of V rows per response (and of the broadband group)
    double *fu, *fd;            // spectral forms (and SPECTRAL): flux_up / flux_down at this thread's point
    uint64_t nw, i;
    int V, user, col;
    double pwt;                 // PROFILE: this point's trapezoid weight
    bool live;
    double out[6];
    GrtBandArgs bins;           // BANDED
    int bin_lo, bin_count;      // ... the first bin with a point in this workgroup, and how many there are
    double dw;
    DirectRows<DIRECT> direct;  // DIRECT
    ResponseRows<RESPONSES> resp;   // RESPONSES

    template <typename Args>
    __device__ __forceinline__ LevelSink(Args const &a, int col_, uint64_t i_, bool live_,
                                         GrtBandArgs const &bins_ = GrtBandArgs{0, 0, nullptr, 0},
                                         GrtDirectArgs const &direct_ = GrtDirectArgs{nullptr},
                                         GrtResponseArgs const &resp_ = GrtResponseArgs{0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr})
    {
        if constexpr (DIRECT)
        {
            direct.partials = direct_.partials;
            direct.out[0] = direct.out[1] = direct.out[2] = 0.;
        }
        col = col_;
        i = i_;
        live = live_;
        nw = a.nw;
        V = a.num_levels;
        user = a.user_level;
        fu = FUSED && !SPECTRAL ? nullptr : a.flux_up + (uint64_t)col*a.flux_stride + i;
        fd = FUSED && !SPECTRAL ? nullptr : a.flux_down + (uint64_t)col*a.flux_stride + i;
        pwt = PROFILE && !BANDED ? trapezoid_weight(i, nw, a.dw, live) : 0.;
        bins = bins_;
        bin_lo = bin_count = 0;
        dw = a.dw;
        if (BANDED)
        {
            int const *blk = bins.table + 4*bins.num_bins + 2*blockIdx.x;
            bin_lo = blk[0];
            bin_count = blk[1] - blk[0];
            pwt = bin_count == 1 ? bin_weight(bin_lo) : 0.;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k)
        {
            out[k] = 0.;
        }
        if constexpr (RESPONSES)
        {
            resp.a = resp_;
            resp.lo = resp_.block_start[blockIdx.x];
            resp.count = resp_.block_start[blockIdx.x + 1] - resp.lo;
            // this thread's pwt*r of the block's responses, behind the (1 + count) groups of wave sums
            double *wt = level_sums() + (size_t)(1 + resp.count)*GROUPS*V*(kSolverBlock/64) + threadIdx.x;
            resp.wt = wt;
            for (int q = 0; q < resp.count; ++q)
            {
                Window const w = window_of(resp_.entry, resp_.block_list, resp.lo + q);
                long long const at = (long long)i - w.first();                  // (Window: span, weight)
                wt[q*kSolverBlock] = live && at >= 0 && at < w.count() ? pwt*resp_.weights[w.weight_at() + at] : 0.;
            }
        }
    }

    static __device__ __forceinline__ double *level_sums()
    {
        // PROFILE: [2 V][kSolverBlock/64] (DIRECT: [3 V]); BANDED: that per bin of the block; RESPONSES: that once more per
        // response of the block, then the staged weights [responses of the block][kSolverBlock]
        extern __shared__ double level_sums_[];
        return level_sums_;
    }

    // RESPONSES: the value x of broadband row `row` once more per response of the block's list, weighted with its pwt*r
    __device__ __forceinline__ void put_responses(int row, double x)
    {
        if constexpr (RESPONSES)
        {
            for (int q = 0; q < resp.count; ++q)
            {
                wave_row_sum<kSolverBlock>(x*resp.wt[q*kSolverBlock], level_sums(), (1 + q)*GROUPS*V + row);
            }
        }
    }

    // BANDED: this point's trapezoid weight in bin b -- dw/2 at the bin's two edges, dw between them, 0 elsewhere (an idle
    // lane lies beyond every edge)
    __device__ __forceinline__ double bin_weight(int b) const
    {
        int const *e = bins.table + 4*b;
        long long const at = (long long)i;
        return (at == e[0] || at == e[1]) ? 0.5*dw : ((at > e[0] && at < e[1]) ? dw : 0.);
    }

    // whether a flux of level lev leaves the kernel
    __device__ __forceinline__ bool wanted(int lev) const
    {
        return !FUSED || PROFILE || lev == 0 || lev == V - 1 || lev == user;
    }

    // level lev's upward (down false) or downward flux at this point is x
    __device__ __forceinline__ void put(int lev, bool down, double x)
    {
        if (PROFILE && BANDED && bin_count != 1)
        {
            for (int q = 0; q < bin_count; ++q)
            {
                wave_row_sum<kSolverBlock>(x*bin_weight(bin_lo + q), level_sums(), q*2*V + (down ? V : 0) + lev);
            }
        }
        else if (PROFILE)
        {
            wave_row_sum<kSolverBlock>(x*pwt, level_sums(), (down ? V : 0) + lev);
            put_responses((down ? V : 0) + lev, x);
        }
        else if (FUSED)
        {
            int const k = down ? 3 : 0;
            out[k] = lev == 0 ? x : out[k];
            out[k + 1] = lev + 1 == V ? x : out[k + 1];
            out[k + 2] = lev == user ? x : out[k + 2];
        }
        else
        {
            (down ? fd : fu)[(uint64_t)lev*nw] = x;
        }
    }

    // DIRECT: level lev's direct beam at this point is x (for a level that is wanted())
    __device__ __forceinline__ void put_direct(int lev, double x)
    {
        if constexpr (DIRECT && PROFILE)
        {
            wave_row_sum<kSolverBlock>(x*pwt, level_sums(), 2*V + lev);
            put_responses(2*V + lev, x);
        }
        else if constexpr (DIRECT)
        {
            direct.out[0] = lev == 0 ? x : direct.out[0];
            direct.out[1] = lev + 1 == V ? x : direct.out[1];
            direct.out[2] = lev == user ? x : direct.out[2];
        }
    }

    // ... is 0 at every point (its sums are 0 whatever the weights)
    __device__ __forceinline__ void put_zero(int lev, bool down)
    {
        if (PROFILE)
        {
            if ((threadIdx.x & 63) == 0)
            {
                for (int q = 0; q < (BANDED ? bin_count : 1); ++q)
                {
                    level_sums()[(q*2*V + (down ? V : 0) + lev)*(kSolverBlock/64) + (threadIdx.x >> 6)] = 0.;
                }
                if constexpr (RESPONSES)
                {
                    for (int q = 1; q <= resp.count; ++q)
                    {
                        level_sums()[(q*GROUPS*V + (down ? V : 0) + lev)*(kSolverBlock/64) + (threadIdx.x >> 6)] = 0.;
                    }
                }
            }
        }
        else
        {
            put(lev, down, 0.);
        }
    }

    // (the fused forms' partials and weights are read here, where the kernel ends)
    template <typename Args>
    __device__ __forceinline__ void finish(Args const &a)
    {
        if (PROFILE && BANDED)
        {
            // (block_row_partials per bin of the block)
            __syncthreads();
            double const *lds = level_sums();
            for (int k = threadIdx.x; k < bin_count*2*V; k += kSolverBlock)
            {
                int const q = k/(2*V), r = k - q*2*V;
                int const *e = bins.table + 4*(bin_lo + q);
                a.partials[((uint64_t)col*2*V + r)*bins.per_row + e[2] + (int)blockIdx.x - e[3]] =
                    waves_sum<kSolverBlock/64>(lds + k*(kSolverBlock/64));
            }
        }
        else if (PROFILE)
        {
            block_row_partials<kSolverBlock>(level_sums(), 2*V, a.partials, (uint64_t)col*2*V, gridDim.x, blockIdx.x);
            if constexpr (DIRECT)
            {
                block_row_partials<kSolverBlock>(level_sums() + 2*V*(kSolverBlock/64), V, direct.partials, (uint64_t)col*V,
                                                 gridDim.x, blockIdx.x);
            }
            if constexpr (RESPONSES)
            {
                // (block_row_partials per response of the block's list, behind its barrier)
                int const rows = GROUPS*V;
                double const *lds = level_sums() + rows*(kSolverBlock/64);
                for (int k = threadIdx.x; k < resp.count*rows; k += kSolverBlock)
                {
                    int const q = k/rows, r = k - q*rows;
                    Window const w = window_of(resp.a.entry, resp.a.block_list, resp.lo + q);
                    uint64_t const pair = (uint64_t)(w.first_pair() + (int)blockIdx.x - w.first_block());   // (Window: pair)
                    resp.a.partials[((uint64_t)col*resp.a.per_row + pair)*rows + r] =
                        waves_sum<kSolverBlock/64>(lds + k*(kSolverBlock/64));
                }
            }
        }
        else if constexpr (DIRECT)
        {
            // (the six rows' weights and sums below, on nine)
            double const wt = trapezoid_weight(i, nw, a.dw, live);
            double nine[9];
#pragma unroll
            for (int k = 0; k < 9; ++k)
            {
                nine[k] = (k < 6 ? out[k] : direct.out[k - 6])*wt;
            }
            block_partials<9, kSolverBlock, 6>(nine, a.partials, (uint64_t)col*6, gridDim.x, blockIdx.x, direct.partials,
                                               (uint64_t)col*3);
        }
        else if (FUSED)
        {
            if (SPECTRAL && live)
            {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                {
                    fu[(uint64_t)k*nw] = out[k];
                    fd[(uint64_t)k*nw] = out[3 + k];
                }
            }
            double const wt = trapezoid_weight(i, nw, a.dw, live);
#pragma unroll
            for (int k = 0; k < 6; ++k)
            {
                out[k] *= wt;
            }
            block_partials<6, kSolverBlock>(out, a.partials, (uint64_t)col*6, gridDim.x, blockIdx.x);
        }
    }
};

#endif
