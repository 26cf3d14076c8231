// k_optics.hip -- streaming (HBM-bound) optics kernels for gfx950: Rayleigh, optics
// combination, sub-sampling, the fused clear-sky combine, the spectral trapezoid and its wavenumber bins.
// One thread per wavenumber (or per element), coalesced fp64 reads/writes, grid-stride
// so one launch covers any grid size with <= 2048 workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../grt_kernels.h"
#include "optics_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;

inline unsigned grid_for(uint64_t n)
{
    uint64_t const b = (n + kBlock - 1)/kBlock;
    return (unsigned)(b < 2048 ? (b ? b : 1) : 2048);
}

// the layers' number densities travel as a kernel argument (at most 200 doubles): the one-column call has nothing to
// upload and nothing to wait for
constexpr int kRayleighMaxLayers = 200;            // MAX_NUM_LAYERS of the public header
struct RayleighLayers { double n[kRayleighMaxLayers]; };

__global__ __launch_bounds__(kBlock) void rayleigh_kernel(int L, double w0, double dw, uint64_t nw,
                                                          RayleighLayers lay, double *tau,
                                                          double *omega, double *g)
{
    double const *n_layer = lay.n;
    uint64_t const total = (uint64_t)L*nw;
    for (uint64_t o = (uint64_t)blockIdx.x*kBlock + threadIdx.x; o < total; o += (uint64_t)gridDim.x*kBlock)
    {
        uint64_t const i = o/nw;
        uint64_t const j = o - i*nw;
        double const w = w0 + j*dw;                      // rayleigh.c:63
        omega[o] = 1.;
        g[o] = 0.;
        tau[o] = rayleigh_tau(w, n_layer[i]);
    }
}

// utilities/src/optics.c:128-148 (result object starts zero-filled: optics.c:194-199)
__global__ __launch_bounds__(kBlock) void add_optics_kernel(uint64_t n, int K, GrtOpticsPtrs in,
                                                            double *tau, double *omega, double *g)
{
    for (uint64_t i = (uint64_t)blockIdx.x*kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x*kBlock)
    {
        double gs = 0., os = 0., ts = 0.;
        for (int j = 0; j < K; ++j)
        {
            double const t = in.tau[j][i], o = in.omega[j][i], gg = in.g[j][i];
            gs += gg*o*t;
            os += o*t;
            ts += t;
        }
        gs /= os;
        os /= ts;
        g[i] = gs;
        omega[i] = os;
        tau[i] = ts;
    }
}

// The same for any number of objects (the reference has no limit, optics.c:84-124): the K x 3 array pointers come from a
// device table [3][K] (tau rows, omega rows, g rows) instead of the kernel arguments; same sums in the same order.
__global__ __launch_bounds__(kBlock) void add_optics_table_kernel(uint64_t n, int K, double const *const *tab,
                                                                  double *tau, double *omega, double *g)
{
    for (uint64_t i = (uint64_t)blockIdx.x*kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x*kBlock)
    {
        double gs = 0., os = 0., ts = 0.;
        for (int j = 0; j < K; ++j)
        {
            double const t = tab[j][i], o = tab[K + j][i], gg = tab[2*K + j][i];
            gs += gg*o*t;
            os += o*t;
            ts += t;
        }
        gs /= os;
        os /= ts;
        g[i] = gs;
        omega[i] = os;
        tau[i] = ts;
    }
}

// utilities/src/optics.c:306-321
__global__ __launch_bounds__(kBlock) void sample_optics_kernel(uint64_t n, uint64_t factor, double *tau,
                                                               double *omega, double *g,
                                                               double const *tau_in,
                                                               double const *omega_in,
                                                               double const *g_in)
{
    for (uint64_t i = (uint64_t)blockIdx.x*kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x*kBlock)
    {
        uint64_t const o = i*factor;
        tau[i] = tau_in[o];
        omega[i] = omega_in[o];
        g[i] = g_in[o];
    }
}

// Rayleigh + add_optics({gas, rayleigh}) in one pass (driver.c:247-270,381-383):
// with gas omega = g = 0 and Rayleigh omega = 1, g = 0 the sums of optics.c:138-145 are
//   g_sum = 0*0*tg + 0*1*tr, o_sum = 0*tg + 1*tr, t_sum = tg + tr.
__global__ __launch_bounds__(kBlock) void clear_sky_kernel(int L, int ncol, double w0, double dw,
                                                           uint64_t nw, double const *n_layer,
                                                           double const *tau_gas, double *tau,
                                                           double *omega, double *g)
{
    uint64_t const per_col = (uint64_t)L*nw;
    uint64_t const total = per_col*ncol;
    for (uint64_t o = (uint64_t)blockIdx.x*kBlock + threadIdx.x; o < total; o += (uint64_t)gridDim.x*kBlock)
    {
        uint64_t const c = o/per_col;
        uint64_t const r = o - c*per_col;
        uint64_t const i = r/nw;
        uint64_t const j = r - i*nw;
        double const tr = rayleigh_tau(w0 + j*dw, n_layer[c*L + i]);
        double t, om, gg;
        clear_sky_combine(tau_gas[o], tr, t, om, gg);
        g[o] = gg;
        omega[o] = om;
        tau[o] = t;
    }
}

// Materialised all-sky form: the liquid and ice cloud objects of grt_pipeline_run_allsky on the grid, [ncol][L][nw] each,
// from the band tables (GrtCloudArgs; cloud_layer: tau = extinction x thickness, nothing where a point has no band), for
// add_optics' kernel to add to gas and Rayleigh.
__global__ __launch_bounds__(kBlock) void spread_clouds_kernel(int L, int ncol, uint64_t nw, GrtCloudArgs c,
                                                               double *lt, double *lo, double *lg,
                                                               double *it, double *io, double *ig)
{
    uint64_t const per_col = (uint64_t)L*nw;
    uint64_t const total = per_col*ncol;
    for (uint64_t o = (uint64_t)blockIdx.x*kBlock + threadIdx.x; o < total; o += (uint64_t)gridDim.x*kBlock)
    {
        uint64_t const col = o/per_col;
        uint64_t const r = o - col*per_col;
        int const j = (int)(r/nw);
        uint64_t const i = r - (uint64_t)j*nw;
        uint64_t const tab = col*3*(uint64_t)c.num_bands*L;
        double const th = c.thickness[col*L + j];
        cloud_layer(c.liquid + tab, c.num_bands, L, c.band_liquid[i], j, th, lt[o], lo[o], lg[o]);
        cloud_layer(c.ice + tab, c.num_bands, L, c.band_ice[i], j, th, it[o], io[o], ig[o]);
    }
}

// Materialised form of grt_pipeline_run_aerosols: the aerosol object of every column on the grid, [ncol][L][nw] each, from
// the columns' slope and intercept tables (GrtAerosolArgs; aerosol_layer: the fused solvers' expressions).
__global__ __launch_bounds__(kBlock) void spread_aerosols_kernel(int L, int ncol, double w0, double dw, uint64_t nw,
                                                                 GrtAerosolArgs c, double *tau, double *omega, double *g)
{
    uint64_t const per_col = (uint64_t)L*nw;
    uint64_t const total = per_col*ncol;
    uint64_t const plane = 2*(uint64_t)c.num_intervals*L;
    for (uint64_t o = (uint64_t)blockIdx.x*kBlock + threadIdx.x; o < total; o += (uint64_t)gridDim.x*kBlock)
    {
        uint64_t const col = o/per_col;
        uint64_t const r = o - col*per_col;
        int const j = (int)(r/nw);
        uint64_t const i = r - (uint64_t)j*nw;
        int const interval = c.interval[i];
        double const *tab = c.tables + col*3*plane + (uint64_t)(interval < 0 ? 0 : interval)*2*L;
        aerosol_layer(tab, plane, L, interval, j, w0 + i*dw, tau[o], omega[o], g[o]);
    }
}

// grt_pipeline_set_surface: each column's surface emissivity or albedo on the band's grid, rows [ncol][nw], from the
// columns' slope and intercept entries (GrtSurfaceArgs): one thread per column and grid point reads the point's entry
// index and the column's (m, b) and stores m w + b -- linear_sample's expression (utilities.c:235-246); the entries of the
// two constant ranges have m = 0, and 0 w + b is b.  Consecutive lanes store consecutive doubles.
__global__ __launch_bounds__(kBlock) void spread_surface_kernel(int ncol, double w0, double dw, uint64_t nw, GrtSurfaceArgs c,
                                                                double *rows)
{
    uint64_t const total = nw*(uint64_t)ncol;
    for (uint64_t o = (uint64_t)blockIdx.x*kBlock + threadIdx.x; o < total; o += (uint64_t)gridDim.x*kBlock)
    {
        uint64_t const col = o/nw;
        uint64_t const i = o - col*nw;
        double const *mb = c.tables + (col*(uint64_t)c.num_entries + (uint64_t)c.entry[i])*2;
        double const w = w0 + i*dw;
        rows[o] = mb[0]*w + mb[1];
    }
}

// tau_gas += the spectral tables' part, for a tau the gas-optics launch wrote without it (GrtGasOpticsArgs.skip_tables):
// the pipeline's fused solvers add it themselves; this completes the array for a caller that wants to LOOK at tau_gas
// (grt_pipeline_views).  One thread per grid point and column, walking the layers: continua_add's doubles.
__global__ __launch_bounds__(kBlock) void add_continua_kernel(GrtContinua c, int L, uint64_t nw, double *tau_gas, uint64_t col_stride)
{
    uint64_t const i = (uint64_t)blockIdx.x*kBlock + threadIdx.x;
    int const col = blockIdx.y;
    long long const lo = (long long)blockIdx.x*kBlock, hi = lo + kBlock < (long long)nw ? lo + kBlock : (long long)nw;
    uint64_t const ii = i < nw ? i : nw - 1;
    PointContinua pc;
    continua_load(c, nw, ii, lo, hi, pc);
    double const *cstate = c.colstate + (uint64_t)col*c.stride;
    double *tau = tau_gas + (uint64_t)col*col_stride + ii;
    for (int j = 0; j < L && i < nw; ++j)
    {
        tau[(uint64_t)j*nw] = continua_add(c, pc, cstate, j, nw, ii, lo, hi, tau[(uint64_t)j*nw]);
    }
}

// framework/src/driver.c:302-326: one workgroup per row; wavefront shuffle reduction,
// then LDS across the 4 waves.  (Summation order differs from the serial loop.)
__global__ __launch_bounds__(kBlock) void integrate_rows_kernel(double const *const *rows, uint64_t nw,
                                                                double dw, double *out, int group,
                                                                int out_stride, int out_offset)
{
    __shared__ double part[kBlock/64];
    double const *row = rows[blockIdx.x];
    double s = 0.;
    for (uint64_t i = threadIdx.x; i + 1 < nw; i += kBlock)
    {
        s += 0.5*(row[i] + row[i + 1])*dw;
    }
    WAVE_SUM(s);
    if ((threadIdx.x & 63) == 0)
    {
        part[threadIdx.x >> 6] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        int const r = blockIdx.x;
        out[(r/group)*out_stride + out_offset + (r % group)] = ((part[0] + part[1]) + part[2]) + part[3];
    }
}

// Second stage of the fused solvers' trapezoid: one wavefront per output row adds the blocks' partial sums in a
// fixed order (wave_strided_sum): same bits every run.
__global__ __launch_bounds__(64) void reduce_partials_kernel(double const *partials, unsigned nblocks, double *out,
                                                             int group, int out_stride, int out_offset)
{
    int const r = blockIdx.x;
    double const s = wave_strided_sum(partials + (uint64_t)r*nblocks, nblocks);
    if (threadIdx.x == 0)
    {
        out[(r/group)*out_stride + out_offset + (r % group)] = s;
    }
}

// grt_pipeline_run_subcolumns: the mean over a column's S subcolumns of one output row.  One wavefront per (column, row):
// each subcolumn's block sums by wave_strided_sum as reduce_partials_kernel adds them, then the
// subcolumns in order, then one division by S (driver.c:585-589).  S = 1: reduce_partials_kernel's bits.
__global__ __launch_bounds__(64) void subcolumn_mean_kernel(double const *partials, int S, int rows, unsigned nblocks,
                                                            double *out, int out_stride, int out_offset)
{
    int const c = blockIdx.x/rows;
    int const r = blockIdx.x - c*rows;
    double m = 0.;
    for (int s = 0; s < S; ++s)
    {
        double const x = wave_strided_sum(partials + ((uint64_t)(c*S + s)*rows + r)*nblocks, nblocks);
        m = s == 0 ? x : m + x;
    }
    if (threadIdx.x == 0)
    {
        out[(uint64_t)c*out_stride + out_offset + r] = m/(double)S;
    }
}

// The mean over the draws of output row r, in subcolumn_mean_kernel's order: draw s of S lies at slot first + s of `rows`
// rows; each draw's blocks by wave_strided_sum, the draws in order, then one division by S.  S = 1: the slot's sum as it
// is, behind a branch of its own -- written as a select, the division is evaluated for every row and thrown away.
// (subcolumn_mean_kernel keeps its own loop: it divides whatever S is, and through this helper its code grew by seven
// instructions and changed registers.)
__device__ __forceinline__ double draws_mean(double const *partials, uint64_t first, int S, int rows, int r, unsigned nblocks)
{
    if (S == 1)
    {
        return wave_strided_sum(partials + (first*rows + r)*nblocks, nblocks);
    }
    double x = 0.;
    for (int s = 0; s < S; ++s)
    {
        double const xs = wave_strided_sum(partials + ((first + s)*rows + r)*nblocks, nblocks);
        x = s == 0 ? xs : x + xs;
    }
    return x/(double)S;
}

// The materialised form's subcolumn loop (driver.c:503-589): sum += x per subcolumn (first: the sum starts at 0), then
// x = sum/S
__global__ __launch_bounds__(kBlock) void flux_accumulate_kernel(uint64_t n, double const *x, double *sum, int first)
{
    for (uint64_t i = (uint64_t)blockIdx.x*kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x*kBlock)
    {
        sum[i] = (first ? 0. : sum[i]) + x[i];
    }
}

__global__ __launch_bounds__(kBlock) void flux_mean_kernel(uint64_t n, double const *sum, int S, double *x)
{
    for (uint64_t i = (uint64_t)blockIdx.x*kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x*kBlock)
    {
        x[i] = sum[i]/(double)S;
    }
}

// ---- wavenumber bins of spectral rows (grt_pipeline_run_spectral), in the fused solvers' association ----
// Bin table (grt_bin_table): per bin {first edge, last edge, offset of its partial sums in a row's, first block}, then
// per 128-point solver block {first bin, one past the last bin} that has a point in the block.  A bin over the whole
// grid takes the fused six-row form's weights, block trees and block order: the same bits as its integral.
constexpr int kBinChunk = 64;           // bins of one block summed before their block sums are stored
constexpr int kBinRowGroups = 32;       // gridDim.y of the two binning launches

inline unsigned bin_blocks(uint64_t nw)
{
    return (unsigned)((nw + kSolverBlock - 1)/kSolverBlock);
}

// one workgroup per (128-point block, row): per bin that has a point in the block, sum_i x_i w_i as block_partials
// sums a row (WAVE_SUM, then waves_sum), stored at partials[row P + offset(bin) + block - first_block(bin)].  Row r: in + (r/6) in_stride + (r%6) nw, or
// -- rows given (the level fluxes of grt_pipeline_run_band_profiles' materialised form) -- rows[r].
__global__ __launch_bounds__(kSolverBlock) void bin_partials_kernel(double const *in, uint64_t in_stride,
                                                                    double const *const *rows, int nrows, uint64_t nw,
                                                                    double dw, int nbins, int const *tab, uint64_t P,
                                                                    double *partials)
{
    __shared__ double part[kBinChunk][kSolverBlock/64];
    unsigned const block = blockIdx.x;
    int const b_lo = tab[4*nbins + 2*block], b_hi = tab[4*nbins + 2*block + 1];
    long long const i = (long long)block*kSolverBlock + threadIdx.x;
    bool const live = i < (long long)nw;
    for (int r = blockIdx.y; r < nrows; r += gridDim.y)
    {
        double const x = !live ? 0. : (rows != nullptr ? rows[r][i] : in[(uint64_t)(r/6)*in_stride + (uint64_t)(r % 6)*nw + i]);
        double *prow = partials + (uint64_t)r*P;
        for (int b0 = b_lo; b0 < b_hi; b0 += kBinChunk)
        {
            int const nb = b_hi - b0 < kBinChunk ? b_hi - b0 : kBinChunk;
            for (int q = 0; q < nb; ++q)
            {
                int const *e = tab + 4*(b0 + q);
                // (trapezoid_weight's doubles: dw/2 at the bin's two edges, dw between them)
                double const w = (i == e[0] || i == e[1]) ? 0.5*dw : ((i > e[0] && i < e[1]) ? dw : 0.);
                double s = x*w;
                WAVE_SUM(s);
                if ((threadIdx.x & 63) == 0)
                {
                    part[q][threadIdx.x >> 6] = s;
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < nb)
            {
                int const *e = tab + 4*(b0 + threadIdx.x);
                prow[e[2] + block - e[3]] = waves_sum<kSolverBlock/64>(part[threadIdx.x]);
            }
            __syncthreads();
        }
    }
}

// one wavefront per (bin, row): the bin's block sums in block order by wave_strided_sum, as reduce_partials_kernel's.  `group` rows
// per column; bin b of row r goes to out + (r/group) out_stride + (r%group) nbins + b, or -- levels > 0: the rows are a
// column's levels, up then down (group = 2 levels) -- + ((r%group/levels) nbins + b) levels + r%levels.
__global__ __launch_bounds__(64) void bin_reduce_kernel(int nrows, int group, int levels, int nbins, int const *tab,
                                                        uint64_t P, double const *partials, double *out,
                                                        uint64_t out_stride)
{
    int const b = blockIdx.x;
    int const *e = tab + 4*b;
    unsigned const nblk = (unsigned)(e[1]/kSolverBlock - e[3]) + 1;
    for (int r = blockIdx.y; r < nrows; r += gridDim.y)
    {
        // (wave_strided_sum, written out: as a call the loop over the rows is scheduled differently)
        double const *p = partials + (uint64_t)r*P + e[2];
        double s = 0.;
        for (unsigned k = threadIdx.x; k < nblk; k += 64)
        {
            s += p[k];
        }
        WAVE_SUM(s);
        if (threadIdx.x == 0)
        {
            int const k = r % group;
            uint64_t const at = levels > 0 ? ((uint64_t)(k/levels)*nbins + b)*levels + k % levels : (uint64_t)k*nbins + b;
            out[(uint64_t)(r/group)*out_stride + at] = s;
        }
    }
}

// the materialised form's spectral rows: out + (r/6) out_stride + (r%6) nw <- rows[r]
__global__ __launch_bounds__(kBlock) void copy_rows_kernel(double const *const *rows, int nrows, uint64_t nw, double *out,
                                                           uint64_t out_stride)
{
    uint64_t const i = (uint64_t)blockIdx.x*kBlock + threadIdx.x;
    if (i >= nw)
    {
        return;
    }
    for (int r = blockIdx.y; r < nrows; r += gridDim.y)
    {
        out[(uint64_t)(r/6)*out_stride + (uint64_t)(r % 6)*nw + i] = rows[r][i];
    }
}

// The heating rate of layer j, between levels j (upper) and j + 1, from a column's level pressures p [V] mb and level
// fluxes up, dn [V]:  H_j = (g/c_p) ((dn_j - up_j) - (dn_{j+1} - up_{j+1}))/(100 (p_{j+1} - p_j)) 86 400   [K day-1]
__device__ __forceinline__ double heating_rate(double gravity, double cp, double const *p, double const *up,
                                               double const *dn, int j)
{
    double const net_top = dn[j] - up[j], net_bottom = dn[j + 1] - up[j + 1];
    return (gravity/cp)*((net_top - net_bottom)/(100.*(p[j + 1] - p[j])))*86400.;
}

// Last step of grt_pipeline_run_profiles (sets = 1), grt_pipeline_run_allsky_profiles (sets = 2: clear sky, then
// all-sky) and grt_pipeline_run_sky (the sets it was asked for): one thread per (column, set, band, layer j) reads the band's level fluxes
// levels[c][set][2 band + {0: up, 1: down}][V] and forms the heating rate of layer j (heating_rate),
// and -- thread j = 0 -- the band's six rows of the six-row form (up top, up surface, up user, down top, down surface, down
// user: grt_pipeline_run's layout).  A band that is not computed (bit clear in `bands`) gets zeros everywhere.
__global__ __launch_bounds__(kBlock) void profile_finish_kernel(int ncol, int sets, int V, int bands, int user,
                                                                double gravity, double cp, double const *pressure,
                                                                double *levels, double *heating, double *fluxes)
{
    int const L = V - 1;
    uint64_t const t = (uint64_t)blockIdx.x*kBlock + threadIdx.x;
    if (t >= (uint64_t)ncol*sets*2*L)
    {
        return;
    }
    int const j = (int)(t % L);
    int const band = (int)((t/L) % 2);
    uint64_t const cs = t/(2*(uint64_t)L);         // c sets + set
    int const c = (int)(cs/sets);
    double *up = levels + (cs*4 + 2*band)*V;
    double *dn = up + V;
    double *six = fluxes ? fluxes + cs*12 + 6*band : nullptr;
    double *h = heating ? heating + (cs*2 + band)*L + j : nullptr;
    if (!((bands >> band) & 1))
    {
        up[j] = 0.;
        dn[j] = 0.;
        if (j + 1 == L)
        {
            up[L] = 0.;
            dn[L] = 0.;
        }
        if (h)
        {
            *h = 0.;
        }
        if (six && j == 0)
        {
            for (int k = 0; k < 6; ++k)
            {
                six[k] = 0.;
            }
        }
        return;
    }
    if (h)
    {
        *h = heating_rate(gravity, cp, pressure + (uint64_t)c*V, up, dn, j);
    }
    if (six && j == 0)
    {
        six[0] = up[0];
        six[1] = up[L];
        six[2] = user >= 0 ? up[user] : 0.;
        six[3] = dn[0];
        six[4] = dn[L];
        six[5] = user >= 0 ? dn[user] : 0.;
    }
}

// Last step of grt_pipeline_run_band_profiles: one thread per (column, set, bin q of the lw_bins + sw_bins, layer j) reads
// the bin's level fluxes in levels[c][set][2 lw_bins + 2 sw_bins][V] (per set the longwave's [2][lw_bins][V], up then
// down, then the shortwave's) and forms heating_rate of layer j from them, as profile_finish_kernel does.
__global__ __launch_bounds__(kBlock) void band_profile_finish_kernel(int ncol, int sets, int V, int lw_bins, int sw_bins,
                                                                     double gravity, double cp, double const *pressure,
                                                                     double const *levels, double *heating)
{
    int const L = V - 1, nb = lw_bins + sw_bins;
    uint64_t const t = (uint64_t)blockIdx.x*kBlock + threadIdx.x;
    if (t >= (uint64_t)ncol*sets*nb*L)
    {
        return;
    }
    int const j = (int)(t % L);
    int const q = (int)((t/L) % nb);
    uint64_t const cs = t/((uint64_t)nb*L);        // c sets + set
    int const c = (int)(cs/sets);
    double const *set = levels + cs*2*(uint64_t)nb*V;
    double const *up = q < lw_bins ? set + (uint64_t)q*V : set + (2*(uint64_t)lw_bins + (q - lw_bins))*V;
    double const *dn = up + (uint64_t)(q < lw_bins ? lw_bins : sw_bins)*V;
    heating[(cs*nb + q)*L + j] = heating_rate(gravity, cp, pressure + (uint64_t)c*V, up, dn, j);
}

// Level row r of the profile form's rows = 2 V (up then down levels) among the six rows at `six`: rows 0, V - 1 and user as
// profile_finish_kernel picks them, +0.0 without a user level
__device__ __forceinline__ void keep_six_rows(double *six, int rows, int r, int user, double x)
{
    int const V = rows/2, down = r/V, lev = r - down*V;
    double *q = six + 3*down;
    if (lev == 0)
    {
        q[0] = x;
        if (user < 0)
        {
            q[2] = 0.;
        }
    }
    if (lev == V - 1)
    {
        q[1] = x;
    }
    if (lev == user)
    {
        q[2] = x;
    }
}

// grt_pipeline_run_zeniths (S = 1, sets = 1, set = 0) and grt_pipeline_run_sky_zeniths, one set of a column's `sets`: every
// sun angle's own rows, and their weighted mean over a column's Z angles, over partial sums that hold S cloud draws per
// angle (slot (c Z + k) S + s).  One wavefront per (column, row): the angle's draws_mean (a night angle, mu <= 0: +0.0),
// stored where the set's per-angle rows lie; then the angles in order -- w_k x_k, the product rounded before it is added,
// or, without weights, the plain sum and one division by Z as subcolumn_mean_kernel's.  Z = 1 and S = 1 without weights:
// reduce_partials_kernel's bits.  six (profile form): every angle's six rows too (keep_six_rows).
__global__ __launch_bounds__(64) void sky_zenith_mean_kernel(double const *partials, int Z, int S, int rows, unsigned nblocks,
                                                             double const *mu, double const *weight, double *per_angle,
                                                             double *six, int sets, int set, int user, double *out,
                                                             int out_stride, int out_offset)
{
    int const c = blockIdx.x/rows;
    int const r = blockIdx.x - c*rows;
    double m = 0.;
    for (int k = 0; k < Z; ++k)
    {
        uint64_t const sun = (uint64_t)c*Z + k, angle = ((uint64_t)c*sets + set)*Z + k;
        double x = draws_mean(partials, sun*S, S, rows, r, nblocks);
        x = mu[sun] > 0. ? x : 0.;
        if (per_angle != nullptr && threadIdx.x == 0)
        {
            per_angle[angle*rows + r] = x;
        }
        if (six != nullptr && threadIdx.x == 0)
        {
            keep_six_rows(six + angle*6, rows, r, user, x);
        }
        double const term = weight != nullptr ? weight[sun]*x : x;
        m = k == 0 ? term : m + term;
    }
    if (out != nullptr && threadIdx.x == 0)
    {
        out[(uint64_t)c*out_stride + out_offset + r] = weight != nullptr ? m : m/(double)Z;
    }
}

// grt_pipeline_run_sky_tiles: one band of one set of a column's `sets`, over partial sums that hold S cloud draws per tile
// (slot (c T + t) S + s).  One wavefront per (column, row of the six): the tile's draws_mean, stored where the set's
// per-tile rows lie; then the tiles in order, each times its fraction, the product rounded before it is added -- no
// fractions: the plain sum and one division by T.
__global__ __launch_bounds__(64) void tile_mean_kernel(double const *partials, int T, int S, unsigned nblocks,
                                                       double const *fraction, double *per_tile, int sets, int set,
                                                       int band, double *out, int out_stride, int out_offset)
{
    int const c = blockIdx.x/6;
    int const r = blockIdx.x - c*6;
    double m = 0.;
    for (int t = 0; t < T; ++t)
    {
        uint64_t const tile = (uint64_t)c*T + t;
        double const x = draws_mean(partials, tile*S, S, 6, r, nblocks);
        if (per_tile != nullptr && threadIdx.x == 0)
        {
            per_tile[(((uint64_t)c*sets + set)*T + t)*12 + 6*band + r] = x;
        }
        double const term = fraction != nullptr ? fraction[tile]*x : x;
        m = t == 0 ? term : m + term;
    }
    if (out != nullptr && threadIdx.x == 0)
    {
        out[(uint64_t)c*out_stride + out_offset + r] = fraction != nullptr ? m : m/(double)T;
    }
}

} // namespace

extern "C" int grt_launch_tile_mean(void *stream, double const *partials, int ncol, int tiles, int subcolumns,
                                    unsigned nblocks, double const *fraction, double *per_tile, int sets, int set, int band,
                                    double *out, int out_stride, int out_offset)
{
    if (ncol < 1 || tiles < 1 || subcolumns < 1 || nblocks < 1 || sets < 1 || set < 0 || set >= sets || band < 0 || band > 1 ||
        partials == nullptr || (out == nullptr && per_tile == nullptr))
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(tile_mean_kernel, dim3((unsigned)(ncol*6)), dim3(64), 0, (hipStream_t)stream, partials, tiles,
                       subcolumns, nblocks, fraction, per_tile, sets, set, band, out, out_stride, out_offset);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_band_profile_finish(void *stream, int ncol, int sets, int num_levels, int lw_bins, int sw_bins,
                                              double gravity, double cp, double const *pressure, double const *levels,
                                              double *heating)
{
    if (ncol < 1 || sets < 1 || sets > 2 || num_levels < 2 || lw_bins < 0 || sw_bins < 0 || lw_bins + sw_bins < 1 ||
        levels == nullptr || heating == nullptr || pressure == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    uint64_t const threads = (uint64_t)ncol*sets*(uint64_t)(lw_bins + sw_bins)*(uint64_t)(num_levels - 1);
    hipLaunchKernelGGL(band_profile_finish_kernel, dim3((unsigned)((threads + kBlock - 1)/kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, ncol, sets, num_levels, lw_bins, sw_bins, gravity, cp, pressure, levels,
                       heating);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_profile_finish(void *stream, int ncol, int sets, int num_levels, int bands, int user_level,
                                         double gravity, double cp, double const *pressure, double *levels, double *heating,
                                         double *fluxes)
{
    if (ncol < 1 || sets < 1 || sets > GRT_PROFILE_MAX_SETS || num_levels < 2 || user_level >= num_levels ||
        levels == nullptr ||
        (heating && pressure == nullptr))
    {
        return (int)hipErrorInvalidValue;
    }
    uint64_t const threads = (uint64_t)ncol*sets*2*(uint64_t)(num_levels - 1);
    hipLaunchKernelGGL(profile_finish_kernel, dim3((unsigned)((threads + kBlock - 1)/kBlock)), dim3(kBlock), 0,
                       (hipStream_t)stream, ncol, sets, num_levels, bands, user_level, gravity, cp, pressure, levels,
                       heating, fluxes);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_reduce_partials(void *stream, double const *partials, int nrows, unsigned nblocks,
                                          double *out, int group, int out_stride, int out_offset)
{
    if (nrows < 1)
    {
        return 0;
    }
    hipLaunchKernelGGL(reduce_partials_kernel, dim3(nrows), dim3(64), 0, (hipStream_t)stream, partials, nblocks, out,
                       group, out_stride, out_offset);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_subcolumn_mean(void *stream, double const *partials, int ncol, int subcolumns, int rows,
                                          unsigned nblocks, double *out, int out_stride, int out_offset)
{
    if (ncol < 1 || subcolumns < 1 || rows < 1 || nblocks < 1 || (uint64_t)ncol*(uint64_t)rows > 0x7fffffffull ||
        partials == nullptr || out == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(subcolumn_mean_kernel, dim3((unsigned)(ncol*rows)), dim3(64), 0, (hipStream_t)stream, partials,
                       subcolumns, rows, nblocks, out, out_stride, out_offset);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_zenith_mean(void *stream, double const *partials, int ncol, int zeniths, int rows,
                                      unsigned nblocks, double const *mu, double const *weight, double *per_angle,
                                      double *six, int user_level, double *out, int out_stride, int out_offset)
{
    if (ncol < 1 || zeniths < 1 || rows < 1 || nblocks < 1 || (uint64_t)ncol*(uint64_t)rows > 0x7fffffffull ||
        partials == nullptr || mu == nullptr || (out == nullptr && per_angle == nullptr && six == nullptr) ||
        (six != nullptr && (rows % 2 != 0 || user_level >= rows/2)))
    {
        return (int)hipErrorInvalidValue;
    }
    // (no draws, one set: the sky kernel at S = 1, sets = 1, set = 0)
    hipLaunchKernelGGL(sky_zenith_mean_kernel, dim3((unsigned)(ncol*rows)), dim3(64), 0, (hipStream_t)stream, partials,
                       zeniths, 1, rows, nblocks, mu, weight, per_angle, six, 1, 0, user_level, out, out_stride, out_offset);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_sky_zenith_mean(void *stream, double const *partials, int ncol, int zeniths, int subcolumns,
                                          int rows, unsigned nblocks, double const *mu, double const *weight,
                                          double *per_angle, double *six, int sets, int set, int user_level, double *out,
                                          int out_stride, int out_offset)
{
    if (ncol < 1 || zeniths < 1 || subcolumns < 1 || rows < 1 || nblocks < 1 ||
        (uint64_t)ncol*(uint64_t)rows > 0x7fffffffull || sets < 1 || set < 0 || set >= sets || partials == nullptr ||
        mu == nullptr || (out == nullptr && per_angle == nullptr && six == nullptr) ||
        (six != nullptr && (rows % 2 != 0 || user_level >= rows/2)))
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(sky_zenith_mean_kernel, dim3((unsigned)(ncol*rows)), dim3(64), 0, (hipStream_t)stream, partials,
                       zeniths, subcolumns, rows, nblocks, mu, weight, per_angle, six, sets, set, user_level, out,
                       out_stride, out_offset);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_flux_accumulate(void *stream, uint64_t n, double const *x, double *sum, int first)
{
    hipLaunchKernelGGL(flux_accumulate_kernel, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, n, x, sum, first);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_flux_mean(void *stream, uint64_t n, double const *sum, int subcolumns, double *x)
{
    if (subcolumns < 1)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(flux_mean_kernel, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream, n, sum, subcolumns, x);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_rayleigh(void *stream, int num_layers, double w0, double dw, uint64_t nw,
                                   double const *n_layer_host, double *tau, double *omega, double *g)
{
    if (num_layers < 1 || num_layers > kRayleighMaxLayers)
    {
        return (int)hipErrorInvalidValue;
    }
    RayleighLayers lay;
    for (int i = 0; i < kRayleighMaxLayers; ++i)
    {
        lay.n[i] = i < num_layers ? n_layer_host[i] : 0.;
    }
    hipLaunchKernelGGL(rayleigh_kernel, dim3(grid_for((uint64_t)num_layers*nw)), dim3(kBlock), 0,
                       (hipStream_t)stream, num_layers, w0, dw, nw, lay, tau, omega, g);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_add_optics(void *stream, uint64_t n, int num_optics, GrtOpticsPtrs const *in,
                                     double *tau, double *omega, double *g)
{
    if (num_optics < 1 || num_optics > 8)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(add_optics_kernel, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream,
                       n, num_optics, *in, tau, omega, g);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_add_optics_table(void *stream, uint64_t n, int num_optics, double const *const *table_dev,
                                           double *tau, double *omega, double *g)
{
    if (num_optics < 1 || table_dev == NULL)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(add_optics_table_kernel, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream,
                       n, num_optics, table_dev, tau, omega, g);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_sample_optics(void *stream, uint64_t n, uint64_t factor, double *tau,
                                        double *omega, double *g, double const *tau_in,
                                        double const *omega_in, double const *g_in)
{
    hipLaunchKernelGGL(sample_optics_kernel, dim3(grid_for(n)), dim3(kBlock), 0, (hipStream_t)stream,
                       n, factor, tau, omega, g, tau_in, omega_in, g_in);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_clear_sky_optics(void *stream, int num_layers, int ncol, double w0, double dw,
                                           uint64_t nw, double const *n_layer, double const *tau_gas,
                                           double *tau, double *omega, double *g)
{
    hipLaunchKernelGGL(clear_sky_kernel, dim3(grid_for((uint64_t)num_layers*nw*ncol)), dim3(kBlock), 0,
                       (hipStream_t)stream, num_layers, ncol, w0, dw, nw, n_layer, tau_gas, tau, omega, g);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_spread_clouds(void *stream, int num_layers, int ncol, uint64_t nw, GrtCloudArgs const *c,
                                        double *liquid_tau, double *liquid_omega, double *liquid_g,
                                        double *ice_tau, double *ice_omega, double *ice_g)
{
    if (num_layers < 1 || ncol < 1 || c->num_bands < 1 || c->band_liquid == nullptr || c->band_ice == nullptr ||
        c->thickness == nullptr || c->liquid == nullptr || c->ice == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(spread_clouds_kernel, dim3(grid_for((uint64_t)num_layers*nw*ncol)), dim3(kBlock), 0,
                       (hipStream_t)stream, num_layers, ncol, nw, *c, liquid_tau, liquid_omega, liquid_g,
                       ice_tau, ice_omega, ice_g);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_spread_aerosols(void *stream, int num_layers, int ncol, double w0, double dw, uint64_t nw,
                                          GrtAerosolArgs const *c, double *tau, double *omega, double *g)
{
    if (num_layers < 1 || ncol < 1 || !grt_aerosol_args_ok(c) || tau == nullptr || omega == nullptr || g == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(spread_aerosols_kernel, dim3(grid_for((uint64_t)num_layers*nw*ncol)), dim3(kBlock), 0,
                       (hipStream_t)stream, num_layers, ncol, w0, dw, nw, *c, tau, omega, g);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_spread_surface(void *stream, int ncol, double w0, double dw, uint64_t nw, GrtSurfaceArgs const *c,
                                         double *rows)
{
    if (ncol < 1 || nw < 1 || !grt_surface_args_ok(c) || rows == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(spread_surface_kernel, dim3(grid_for(nw*(uint64_t)ncol)), dim3(kBlock), 0, (hipStream_t)stream, ncol,
                       w0, dw, nw, *c, rows);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_add_continua(void *stream, GrtContinua const *c, int num_layers, int ncol, uint64_t nw,
                                       double *tau_gas, uint64_t col_stride)
{
    hipLaunchKernelGGL(add_continua_kernel, dim3((unsigned)((nw + kBlock - 1)/kBlock), (unsigned)ncol), dim3(kBlock), 0,
                       (hipStream_t)stream, *c, num_layers, nw, tau_gas, col_stride);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_integrate_rows(void *stream, double const *const *rows_dev, int nrows,
                                         uint64_t nw, double dw, double *out, int group,
                                         int out_stride, int out_offset)
{
    if (nrows < 1)
    {
        return 0;
    }
    if (group < 1)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(integrate_rows_kernel, dim3(nrows), dim3(kBlock), 0, (hipStream_t)stream,
                       rows_dev, nw, dw, out, group, out_stride, out_offset);
    return (int)hipGetLastError();
}

extern "C" size_t grt_bin_table_ints(int nbins, uint64_t nw)
{
    return 4*(size_t)nbins + 2*(size_t)bin_blocks(nw);
}

extern "C" size_t grt_bin_table(int const *edges_h, int nbins, uint64_t nw, int *table_h)
{
    unsigned const nblocks = bin_blocks(nw);
    int *blk = table_h + 4*(size_t)nbins;
    for (unsigned k = 0; k < nblocks; ++k)
    {
        blk[2*k] = nbins;
        blk[2*k + 1] = 0;
    }
    size_t off = 0;
    for (int b = 0; b < nbins; ++b)
    {
        int const e0 = edges_h[b], e1 = edges_h[b + 1];
        int const first = e0/kSolverBlock, last = e1/kSolverBlock;
        int *t = table_h + 4*(size_t)b;
        t[0] = e0;
        t[1] = e1;
        t[2] = (int)off;
        t[3] = first;
        off += (size_t)(last - first + 1);
        for (int k = first; k <= last; ++k)
        {
            blk[2*k] = b < blk[2*k] ? b : blk[2*k];
            blk[2*k + 1] = b + 1 > blk[2*k + 1] ? b + 1 : blk[2*k + 1];
        }
    }
    for (unsigned k = 0; k < nblocks; ++k)
    {
        if (blk[2*k] >= blk[2*k + 1])
        {
            blk[2*k] = blk[2*k + 1] = 0;            // (no bin has a point in this block)
        }
    }
    return off;
}

extern "C" int grt_launch_bin_rows(void *stream, double const *in, uint64_t in_stride, int nrows, uint64_t nw, double dw,
                                   int nbins, int const *table_dev, size_t partials_per_row, double *partials,
                                   double *out, uint64_t out_stride)
{
    if (nrows < 1 || nbins < 1)
    {
        return 0;
    }
    if (in == nullptr || table_dev == nullptr || partials == nullptr || out == nullptr || nw < 2)
    {
        return (int)hipErrorInvalidValue;
    }
    // (each workgroup takes every kBinRowGroups-th row: a few thousand workgroups per launch, not one per row)
    unsigned const gy = (unsigned)(nrows < kBinRowGroups ? nrows : kBinRowGroups);
    hipStream_t const s = (hipStream_t)stream;
    hipLaunchKernelGGL(bin_partials_kernel, dim3(bin_blocks(nw), gy), dim3(kSolverBlock), 0, s, in, in_stride,
                       (double const *const *)nullptr, nrows, nw, dw, nbins, table_dev, (uint64_t)partials_per_row,
                       partials);
    hipLaunchKernelGGL(bin_reduce_kernel, dim3((unsigned)nbins, gy), dim3(64), 0, s, nrows, 6, 0, nbins, table_dev,
                       (uint64_t)partials_per_row, (double const *)partials, out, out_stride);
    return (int)hipGetLastError();
}

extern "C" int grt_bin_block_max(int const *edges_h, int nbins)
{
    // (the bins of a block are consecutive; the fullest block is the last block of the first of its bins)
    int most = 0;
    for (int b = 0; b < nbins; ++b)
    {
        int const last = edges_h[b + 1]/kSolverBlock;
        int j = b;
        while (j < nbins && edges_h[j]/kSolverBlock <= last)
        {
            ++j;
        }
        most = j - b > most ? j - b : most;
    }
    return most;
}

extern "C" int grt_launch_bin_reduce(void *stream, int nrows, int num_levels, int nbins, int const *table_dev,
                                     size_t partials_per_row, double const *partials, double *out, uint64_t out_stride)
{
    if (nrows < 1 || nbins < 1)
    {
        return 0;
    }
    if (num_levels < 1 || nrows % (2*num_levels) != 0 || table_dev == nullptr || partials == nullptr || out == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    unsigned const gy = (unsigned)(nrows < kBinRowGroups ? nrows : kBinRowGroups);
    hipLaunchKernelGGL(bin_reduce_kernel, dim3((unsigned)nbins, gy), dim3(64), 0, (hipStream_t)stream, nrows, 2*num_levels,
                       num_levels, nbins, table_dev, (uint64_t)partials_per_row, partials, out, out_stride);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_bin_level_rows(void *stream, double const *const *rows_dev, int nrows, int num_levels, uint64_t nw,
                                         double dw, int nbins, int const *table_dev, size_t partials_per_row,
                                         double *partials, double *out, uint64_t out_stride)
{
    if (nrows < 1 || nbins < 1)
    {
        return 0;
    }
    if (rows_dev == nullptr || table_dev == nullptr || partials == nullptr || nw < 2)
    {
        return (int)hipErrorInvalidValue;
    }
    unsigned const gy = (unsigned)(nrows < kBinRowGroups ? nrows : kBinRowGroups);
    hipLaunchKernelGGL(bin_partials_kernel, dim3(bin_blocks(nw), gy), dim3(kSolverBlock), 0, (hipStream_t)stream,
                       (double const *)nullptr, (uint64_t)0, rows_dev, nrows, nw, dw, nbins, table_dev,
                       (uint64_t)partials_per_row, partials);
    return grt_launch_bin_reduce(stream, nrows, num_levels, nbins, table_dev, partials_per_row, partials, out, out_stride);
}

extern "C" int grt_launch_copy_rows(void *stream, double const *const *rows_dev, int nrows, uint64_t nw, double *out,
                                    uint64_t out_stride)
{
    if (nrows < 1)
    {
        return 0;
    }
    unsigned const gy = (unsigned)(nrows < 65535 ? nrows : 65535);
    hipLaunchKernelGGL(copy_rows_kernel, dim3((unsigned)((nw + kBlock - 1)/kBlock), gy), dim3(kBlock), 0,
                       (hipStream_t)stream, rows_dev, nrows, nw, out, out_stride);
    return (int)hipGetLastError();
}

// ---- response-weighted level rows (grt_pipeline_run_sky_weighted; GrtResponseArgs, grt_kernels.h) ----
namespace {

constexpr int kResponseChunk = 64;      // responses of one block summed before their block sums are stored
constexpr int kResponseFinishBlock = 256;

// The materialised form's twin of LevelSink's response form: one workgroup per (128-point block, slot).  Row (g, level) of
// the slot is rows.p[g] + (slot V + level) nw; per response of the block's list, sum_i x_i (t_i r(i)) as the sink sums it
// (WAVE_SUM, then waves_sum), stored at partials[(slot P + pair) G V + g V + level].
struct ResponseRowGroups { double const *p[3]; };

__global__ __launch_bounds__(kSolverBlock) void response_rows_kernel(GrtResponseArgs r, ResponseRowGroups rows, int G, int V,
                                                                     uint64_t nw, double dw)
{
    __shared__ double part[kResponseChunk][kSolverBlock/64];
    unsigned const block = blockIdx.x, slot = blockIdx.y;
    int const lo = r.block_start[block], hi = r.block_start[block + 1];
    uint64_t const i = (uint64_t)block*kSolverBlock + threadIdx.x;
    bool const live = i < nw;
    double const pwt = trapezoid_weight(i, nw, dw, live);
    int const nrows = G*V;
    for (int row = 0; row < nrows; ++row)
    {
        int const g = row/V, lev = row - g*V;
        double const x = live ? rows.p[g][((uint64_t)slot*V + lev)*nw + i] : 0.;
        for (int q0 = lo; q0 < hi; q0 += kResponseChunk)
        {
            int const nq = hi - q0 < kResponseChunk ? hi - q0 : kResponseChunk;
            for (int q = 0; q < nq; ++q)
            {
                Window const win = window_of(r.entry, r.block_list, q0 + q);
                long long const at = (long long)i - win.first();                // (Window: span, weight)
                double const w = live && at >= 0 && at < win.count() ? pwt*r.weights[win.weight_at() + at] : 0.;
                double s = x*w;
                WAVE_SUM(s);
                if ((threadIdx.x & 63) == 0)
                {
                    part[q][threadIdx.x >> 6] = s;
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < nq)
            {
                Window const win = window_at(r.entry, r.block_list[q0 + threadIdx.x]);
                uint64_t const pair = (uint64_t)(win.first_pair() + (int)block - win.first_block());    // (Window: pair)
                r.partials[((uint64_t)slot*r.per_row + pair)*nrows + row] = waves_sum<kSolverBlock/64>(part[threadIdx.x]);
            }
            __syncthreads();
        }
    }
}

// n partial sums p[0], p[stride], ... added by ONE thread in wave_strided_sum's association: 64 lane sums, each from +0.0
// over every 64th term in order, then the shuffle tree of WAVE_SUM (lane l takes lane l + off, off = 32 .. 1) -- what
// reduce_partials_kernel gives for a row of n blocks, to the bit.
__device__ __forceinline__ double strided_tree_sum(double const *p, unsigned n, uint64_t stride)
{
    double lane[64];
#pragma unroll
    for (int l = 0; l < 64; ++l)
    {
        double s = 0.;
        for (unsigned b = l; b < n; b += 64)
        {
            s += p[(uint64_t)b*stride];
        }
        lane[l] = s;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
#pragma unroll
        for (int l = 0; l < off; ++l)
        {
            lane[l] += lane[l + off];
        }
    }
    return lane[0];
}

// one thread per output row (column, response, row group, level), the level fastest: per draw s = 0 .. S - 1 in order the
// response's blocks as reduce_partials_kernel adds that many, then one division by S as subcolumn_mean_kernel's
__global__ __launch_bounds__(kResponseFinishBlock) void response_finish_kernel(GrtResponseArgs r, int G, int ncol, int S,
                                                                               int V, double *out, uint64_t out_stride,
                                                                               uint64_t out_offset)
{
    uint64_t const t = (uint64_t)blockIdx.x*kResponseFinishBlock + threadIdx.x;
    uint64_t const rows = (uint64_t)G*V;
    if (t >= (uint64_t)ncol*r.responses*rows)
    {
        return;
    }
    uint64_t const row = t % rows, k = (t/rows) % (uint64_t)r.responses, c = t/(rows*(uint64_t)r.responses);
    Window const w = window_at(r.entry, k);
    unsigned const nblk = (unsigned)w.blocks();
    double m = 0.;
    for (int s = 0; s < S; ++s)
    {
        double const x = strided_tree_sum(r.partials + ((c*S + s)*r.per_row + (uint64_t)w.first_pair())*rows + row, nblk, rows);
        m = s == 0 ? x : m + x;
    }
    out[c*out_stride + out_offset + k*rows + row] = m/(double)S;
}

// the actinic flux of every (column, set, response, level) from the three finished shortwave rows, in this order
__global__ __launch_bounds__(kResponseFinishBlock) void actinic_rows_kernel(double const *weighted, uint64_t stride, int ncol,
                                                                            int sets, int R, int V, double const *mu0,
                                                                            double mu_dif, double *actinic)
{
    uint64_t const t = (uint64_t)blockIdx.x*kResponseFinishBlock + threadIdx.x;
    uint64_t const per = (uint64_t)R*V;
    if (t >= (uint64_t)ncol*sets*per)
    {
        return;
    }
    uint64_t const lev = t % V, k = (t/V) % (uint64_t)R, i = t/per, c = i/(uint64_t)sets;
    double const *three = weighted + i*stride + k*3*V + lev;
    double const up = three[0], down = three[V], beam = three[2*(uint64_t)V];
    double const m = mu0[c];
    actinic[t] = (beam/m + (down - beam)/mu_dif) + up/mu_dif;
}

} // namespace

extern "C" int grt_launch_response_rows(void *stream, GrtResponseArgs const *r, double const *const rows[3], int groups,
                                        int slots, int num_levels, uint64_t nw, double dw)
{
    if (!grt_response_args_ok(r) || rows == nullptr || groups < 2 || groups > 3 || slots < 1 || slots > 65535 ||
        num_levels < 1 || nw < 2)
    {
        return (int)hipErrorInvalidValue;
    }
    ResponseRowGroups g = {{rows[0], rows[1], groups == 3 ? rows[2] : nullptr}};
    for (int k = 0; k < groups; ++k)
    {
        if (g.p[k] == nullptr)
        {
            return (int)hipErrorInvalidValue;
        }
    }
    hipLaunchKernelGGL(response_rows_kernel, dim3(bin_blocks(nw), (unsigned)slots), dim3(kSolverBlock), 0, (hipStream_t)stream,
                       *r, g, groups, num_levels, nw, dw);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_response_finish(void *stream, GrtResponseArgs const *r, int groups, int ncol, int subcolumns,
                                          int num_levels, double *out, uint64_t out_stride, uint64_t out_offset)
{
    if (!grt_response_args_ok(r) || groups < 2 || groups > 3 || ncol < 1 || subcolumns < 1 || num_levels < 1 || out == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    uint64_t const threads = (uint64_t)ncol*(uint64_t)r->responses*(uint64_t)groups*(uint64_t)num_levels;
    hipLaunchKernelGGL(response_finish_kernel, dim3((unsigned)((threads + kResponseFinishBlock - 1)/kResponseFinishBlock)),
                       dim3(kResponseFinishBlock), 0, (hipStream_t)stream, *r, groups, ncol, subcolumns, num_levels, out,
                       out_stride, out_offset);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_actinic_rows(void *stream, double const *weighted, uint64_t stride, int ncol, int sets, int responses,
                                       int num_levels, double const *mu0, double mu_dif, double *actinic)
{
    if (weighted == nullptr || ncol < 1 || sets < 1 || responses < 1 || num_levels < 1 || mu0 == nullptr || actinic == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    uint64_t const threads = (uint64_t)ncol*(uint64_t)sets*(uint64_t)responses*(uint64_t)num_levels;
    hipLaunchKernelGGL(actinic_rows_kernel, dim3((unsigned)((threads + kResponseFinishBlock - 1)/kResponseFinishBlock)),
                       dim3(kResponseFinishBlock), 0, (hipStream_t)stream, weighted, stride, ncol, sets, responses, num_levels,
                       mu0, mu_dif, actinic);
    return (int)hipGetLastError();
}
