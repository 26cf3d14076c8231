// k_longwave.hip -- four-stream no-scattering longwave solver for gfx950.
//
// Reference: longwave/src/longwave.c:68-264 (planck_law, effective_planck, lw_flux,
// lw_fluxes_kernel).  One thread per (wavenumber, column); tau/omega are read and the
// fluxes written as (layer|level, wavenumber) rows, so every access is coalesced across
// the wavefront.  The reference walks stream -> layer and keeps three 200-element
// per-thread arrays; we walk layer -> stream with the four stream intensities in
// registers, which needs no per-thread array and produces each flux element by the
// same left-to-right sum (0 + c2[0] I0) + c2[1] I1 + c2[2] I2 + c2[3] I3 as the
// reference's `+=` over its stream loop (longwave.c:184,194-205), i.e. identical values.
// The Planck terms do not depend on the stream and are evaluated once per layer and
// direction instead of once per stream (same inputs, same results).
//
// SURVEY.md §8a19 prices it at 1 944 B per wavenumber at 60 layers; measured it is a latency
// chain -- 120 dependent layer steps with six fp64 exp each on 26 000 threads at 1 cm-1 -- which is why column
// batches share a launch.  lw_kernel has one instance per GrtSolverInstance that exists (grt_kernels.h; the list is in
// grt_launch_lw): what leaves it is its OUT -- spectral fluxes (GRT_OUT_CHAINS), or, fused, the partial sums of the six
// rows, of the six rows that are also stored at every point, of every level, or of every level per wavenumber bin -- and
// what joins gas and Rayleigh is the types of its pack: nothing, GrtCloudArgs, GrtAerosolArgs or GrtSubcolumnArgs, a
// GrtAerosolArgs behind either form of the clouds where both join, and a GrtBandArgs last where OUT is per bin; a
// GrtJacobianArgs last (six rows or every level, with any of the cloud and aerosol joins) makes the instance that also
// leaves dF_up/dT_surf of its upward sweep (LevelSink: DIRECT, the third row group).  The fused six-row clear-sky
// instance is the production pipeline's.  lw_radiance_kernel, further down, is the radiance at viewing angles beside a
// pass's solver (grt_launch_lw_radiances): the same recurrence with a stream's c1 replaced by minus the viewing secant;
// lw_weighting_kernel behind it, the channels' transmittances and contribution functions.
// lw_tile_kernel, behind the spectral form, is the six-row instance for several surface tiles per column
// (grt_launch_lw_tiles): one downward sweep and one set of layer terms for a chunk of tiles, the surface and the streams
// per tile.
//
// What these kernels must say alike, to the bit, is said once: LwPoint (a thread's row, point and layer optical depth),
// absorption_tau (tau (1 - omega) of a materialised pass), AngleChunk (blockIdx.z's viewing angles), stream_step and
// jacobian_step (a layer of the four streams and of their derivatives), channel_row_mean (a channel row from its pairs).
// A new longwave kernel takes its point, its angles and its layer optical depth from these.  LwPoint, absorption_tau and
// effective_planck live in longwave_dev.h: k_longwave_scatter.hip takes its point and its source terms from there too.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../grt_kernels.h"
#include "optics_dev.h"
#include "solver_dispatch.h"
#include "planck_dev.h"
#include "longwave_dev.h"

#pragma clang fp contract(off)

namespace {

// the four streams' constants (longwave.c:160-168)
constexpr double kC1[4] = {-14.402613260847248, -3.0302159969901132, -1.4925584280108841, -1.0746123148178333};
constexpr double kC2[4] = {0.07587638482015649, 0.676114979733751, 1.3726594476601073, 1.0169418413757783};
// (planck_law and its constants, longwave.c:68-94: planck_dev.h, shared with the correlated-k source sums)

// planck(T, w) and with it dB/dT = B (x/T) e/(e - 1), x = c2 w/T, e = exp(x), from planck()'s own exponential (the same
// expressions: the same B); 0 where planck() clamps x
__device__ __forceinline__ double planck_dT(double T, double w, double &dbdt)
{
    double const c1 = kPlanckC1;
    double const c2 = kPlanckC2;
    double x = c2*w/T;
    bool const clamped = x > kMaxExpArg;
    if (clamped)
    {
        x = kMaxExpArg;
    }
    double const e = exp(x);
    double const b = (c1*w*w*w)/(e - 1.);
    dbdt = clamped ? 0. : b*(x/T)*(e/(e - 1.));
    return b;
}

// extinction of a beam over optical depth tau (longwave.c:177-183): c1 is a stream's constant, or minus the secant of
// a viewing angle
__device__ __forceinline__ double beam_extinction(double c1, double tau)
{
    double e = c1*tau;
    if (e > kMaxExpArg)
    {
        e = kMaxExpArg;
    }
    return exp(e);
}

// ... of stream s
__device__ __forceinline__ double extinction(int s, double tau)
{
    return beam_extinction(kC1[s], tau);
}

// One beam through one layer (longwave.c:193-194): I <- (1 - e) val + I e, e its extinction over the layer
__device__ __forceinline__ double beam_step(double I, double val, double e)
{
    double const p = (1. - e)*val;                                       // longwave.c:193
    return p + I*e;
}

// One layer of the four streams (longwave.c:186-195, 204-211): I_s <- (1 - ext_s) val + I_s ext_s; returns the flux
// sum_s c2[s] I_s.  ext(s) gives stream s's extinction where the step needs it (worked out there, or read ahead); e takes
// the four it used.
template <typename Ext>
__device__ __forceinline__ double stream_step(double (&I)[4], double val, Ext ext, double (&e)[4])
{
    double f = 0.;
#pragma unroll
    for (int s = 0; s < 4; ++s)
    {
        e[s] = ext(s);
        I[s] = beam_step(I[s], val, e[s]);
        f += kC2[s]*I[s];                                                // longwave.c:195
    }
    return f;
}

template <typename Ext>
__device__ __forceinline__ double stream_step(double (&I)[4], double val, Ext ext)
{
    double e[4];
    return stream_step(I, val, ext, e);
}

// sum_s c2[s] D_s, in stream_step's order: dF_up/dT_surf from the four streams' derivatives
__device__ __forceinline__ double jacobian_flux(double const (&D)[4])
{
    double f = 0.;
#pragma unroll
    for (int s = 0; s < 4; ++s)
    {
        f += kC2[s]*D[s];
    }
    return f;
}

// One layer on the way up for the streams' derivatives with respect to the surface temperature: the layer emits nothing
// that depends on it, so D_s <- D_s ext_s with the extinctions of the layer's stream_step; returns sum_s c2[s] D_s
template <typename Ext>
__device__ __forceinline__ double jacobian_step(double (&D)[4], Ext ext)
{
#pragma unroll
    for (int s = 0; s < 4; ++s)
    {
        D[s] = D[s]*ext(s);
    }
    return jacobian_flux(D);
}

// The surface (longwave.c:202): emission bs at emissivity emis, the rest of each stream reflected; returns the flux
__device__ __forceinline__ double surface_step(double (&I)[4], double emis, double bs)
{
    double f = 0.;
#pragma unroll
    for (int s = 0; s < 4; ++s)
    {
        I[s] = emis*bs + (1 - emis)*I[s];
        f += kC2[s]*I[s];
    }
    return f;
}

// The four streams' derivatives with respect to the surface temperature beside lw_kernel's upward sweep: there with a
// GrtJacobianArgs in the pack, nothing without
template <bool ON> struct StreamDerivatives {};
template <> struct StreamDerivatives<true> { double D[4]; };

// OUT fused (GRT_OUT_ROWS and after): the clear-sky tail of the pipeline in one kernel -- Rayleigh and the two-object
// optics combination are formed per layer in registers from tau_gas (LayerOptics: identical values), nothing spectral is
// written, and the six integrated output rows leave as per-block trapezoid partial sums (LevelSink).
// GRT_OUT_LEVELS: every level's upward and downward flux leaves instead, 2 V rows per column; GRT_OUT_LEVEL_BINS: once per
// wavenumber bin (the pack's GrtBandArgs); GRT_OUT_ROWS_POINTS: the six rows also leave at every point, unweighted
// (LevelSink).
// Joins (fused forms): clouds (a GrtCloudArgs, or the draws of a GrtSubcolumnArgs), the aerosol object or both join per
// layer (LayerOptics).  Only LwPoint::layer_tau changes: what leaves the kernel is OUT's.
// A GrtJacobianArgs in the pack (GRT_OUT_ROWS and GRT_OUT_LEVELS): the upward sweep carries D[4] beside I[4], seeded at
// the surface with emis dB/dT(T_surf, w), and every level's sum_s c2[s] D_s leaves through the sink's third row group.
template <GrtSolverOutput OUT, typename... Joins>
__global__ __launch_bounds__(kSolverBlock) void lw_kernel(GrtLwArgs a, Joins... joins)
{
    uint64_t const i = (uint64_t)blockIdx.x*kSolverBlock + threadIdx.x;
    constexpr bool FUSED = grt_out_fused(OUT), PROFILE = grt_out_levels(OUT), SPECTRAL = OUT == GRT_OUT_ROWS_POINTS;
    static_assert(has<GrtBandArgs, Joins...> == (OUT == GRT_OUT_LEVEL_BINS), "bins go with GRT_OUT_LEVEL_BINS alone");
    constexpr bool JACOBIAN = has<GrtJacobianArgs, Joins...>;
    static_assert(!JACOBIAN || OUT == GRT_OUT_ROWS || OUT == GRT_OUT_LEVELS, "the Jacobian leaves the six-row and level forms");
    if (!FUSED && i >= a.nw)                      // (fused form: idle lanes of the last block follow along, weight 0)
    {
        return;
    }
    LwPoint<FUSED, Joins...> const p(a, i, joins...);
    int const L = p.L;
    double const w = p.w;
    constexpr bool RESPONSES = has<GrtResponseArgs, Joins...>;
    static_assert(!RESPONSES || (OUT == GRT_OUT_LEVELS && !JACOBIAN), "the response rows leave the level form, without the Jacobian");
    LevelSink<FUSED, PROFILE, SPECTRAL, has<GrtBandArgs, Joins...>, JACOBIAN, RESPONSES> sink(
        a, p.row.slot, i, p.live, pick<GrtBandArgs>(joins...), GrtDirectArgs{pick<GrtJacobianArgs>(joins...).partials},
        pick<GrtResponseArgs>(joins...));

    double I[4] = {0., 0., 0., 0.};
    sink.put_zero(0, true);                                              // longwave.c:171
    for (int j = 0; j < L; ++j)
    {
        double const t = p.layer_tau(j);
        double const val = effective_planck(planck(p.tl[j], w), planck(p.tv[j + 1], w), t);
        sink.put(j + 1, true, stream_step(I, val, [&](int s) { return extinction(s, t); }));
    }
    // the surface, and with the Jacobian the seed of the streams' derivatives, from planck()'s own exponential
    StreamDerivatives<JACOBIAN> d;
    double bs;
    if constexpr (JACOBIAN)
    {
        double dbdt;
        bs = planck_dT(a.t_surf[p.col], w, dbdt);
        d.D[0] = d.D[1] = d.D[2] = d.D[3] = p.emis*dbdt;
    }
    else
    {
        bs = planck(a.t_surf[p.col], w);
    }
    sink.put(L, false, surface_step(I, p.emis, bs));
    if constexpr (JACOBIAN)
    {
        sink.put_direct(L, jacobian_flux(d.D));
    }
    for (int j = L - 1; j >= 0; --j)
    {
        double const t = p.layer_tau(j);
        double const val = effective_planck(planck(p.tl[j], w), planck(p.tv[j], w), t);
        double e[4];
        sink.put(j, false, stream_step(I, val, [&](int s) { return extinction(s, t); }, e));
        if constexpr (JACOBIAN)
        {
            sink.put_direct(j, jacobian_step(d.D, [&](int s) { return e[s]; }));
        }
    }
    sink.finish(a);
}

// ---- the longwave of a correlated-k model on its g-points (grt_launch_ck_lw; GrtCkSolveArgs, grt_kernels.h) ----
// One thread per (column, bin, class), the class fastest: every read of a layer's class sums and every store of a level
// is coalesced.  The g-point's layer optical depths, Planck terms and emissivity are the class means sum/W; then
// lw_kernel's two sweeps on them, operation for operation, gas only (omega = 0).  The four streams stay in registers; no
// LDS, no cross-lane traffic.  The flux per cm-1 times W, the class's W m-2, leaves at every level.  An empty class
// (W = 0) leaves +0.0 and solves nothing.
__global__ __launch_bounds__(kSolverBlock) void ck_lw_kernel(GrtCkSolveArgs a)
{
    uint64_t const per_col = (uint64_t)a.num_bins*(uint64_t)a.num_classes;
    uint64_t const t = (uint64_t)blockIdx.x*kSolverBlock + threadIdx.x;
    if (t >= (uint64_t)a.ncol*per_col)
    {
        return;
    }
    uint64_t const col = t/per_col, at = t - col*per_col;
    int const V = a.num_levels, L = V - 1;
    double const W = a.weight_sum[col*per_col + at];
    double const *T = a.tau_sum + col*(uint64_t)L*per_col + at;              // layer j at T[j per_col]
    double const *S = a.source_sum + col*(uint64_t)(2*V + 1)*per_col + at;   // source row r at S[r per_col]
    double *up = a.flux_up + col*(uint64_t)V*per_col + at, *dn = a.flux_down + col*(uint64_t)V*per_col + at;
    if (!(W > 0.))
    {
        for (int lev = 0; lev < V; ++lev)
        {
            up[(uint64_t)lev*per_col] = 0.;
            dn[(uint64_t)lev*per_col] = 0.;
        }
        return;
    }
    double I[4] = {0., 0., 0., 0.};
    dn[0] = 0.;                                                          // longwave.c:171
    for (int j = 0; j < L; ++j)
    {
        double const tl = T[(uint64_t)j*per_col]/W;
        double const val = effective_planck(S[(uint64_t)(V + j)*per_col]/W, S[(uint64_t)(j + 1)*per_col]/W, tl);
        dn[(uint64_t)(j + 1)*per_col] = stream_step(I, val, [&](int s) { return extinction(s, tl); })*W;
    }
    up[(uint64_t)L*per_col] = surface_step(I, S[(uint64_t)(2*V)*per_col]/W, S[(uint64_t)(2*V - 1)*per_col]/W)*W;
    for (int j = L - 1; j >= 0; --j)
    {
        double const tl = T[(uint64_t)j*per_col]/W;
        double const val = effective_planck(S[(uint64_t)(V + j)*per_col]/W, S[(uint64_t)j*per_col]/W, tl);
        up[(uint64_t)j*per_col] = stream_step(I, val, [&](int s) { return extinction(s, tl); })*W;
    }
}

// ---- the surface-temperature Jacobian of the materialised form (grt_launch_lw_surface_jacobian) ----
// One thread per (wavenumber, column) walks the layers of the tau, omega a pass left on the grid upward from the surface:
// the seed emis dB/dT(T_surf, w) in each stream, then the solver's own extinctions of tau (1 - omega), layer by layer.
constexpr int kJacobianBlock = 128;

__global__ __launch_bounds__(kJacobianBlock) void lw_surface_jacobian_kernel(GrtLwArgs a, double *jacobian)
{
    uint64_t const i = (uint64_t)blockIdx.x*kJacobianBlock + threadIdx.x;
    int const col = blockIdx.y;
    if (i >= a.nw)
    {
        return;
    }
    int const V = a.num_levels;
    int const L = V - 1;
    uint64_t const nw = a.nw;
    double const w = a.w0 + i*a.dw;                                      // longwave.c:246
    double const *tau = a.tau + (uint64_t)col*a.optics_stride + i;
    double const *omega = a.omega ? a.omega + (uint64_t)col*a.optics_stride + i : nullptr;
    double const emis = a.emis[(uint64_t)col*a.emis_stride + i];
    double *out = jacobian + (uint64_t)col*(uint64_t)V*nw + i;
    double dbdt;
    planck_dT(a.t_surf[col], w, dbdt);
    double D[4] = {emis*dbdt, emis*dbdt, emis*dbdt, emis*dbdt};
    out[(uint64_t)L*nw] = jacobian_flux(D);
    for (int j = L - 1; j >= 0; --j)
    {
        uint64_t const o = (uint64_t)j*nw;
        double const t = absorption_tau(tau, omega, o);
        out[o] = jacobian_step(D, [&](int s) { return extinction(s, t); });
    }
}

// ---- radiances at viewing angles (grt_launch_lw_radiances; GrtRadianceArgs, grt_kernels.h) ----
// A stream of the solver is a radiance at the secant -c1[s]; lw_radiance_kernel carries a chunk of up to kRadianceChunk
// viewing angles' radiances through the same two sweeps, on the arguments the pass's solver gets: FUSED, the layer optics
// of the instance's joins formed in registers (LayerOptics, as lw_kernel's), else the tau, omega the pass left on the
// grid.  A layer's optics and its two Planck terms are formed once per layer and sweep and shared by the chunk's angles;
// the padding angles of a last chunk repeat its last real secant and write nothing.  What leaves: the upward radiance at
// the top and the downward one at the surface, as trapezoid partial sums [slot][angles][2][nblocks] (idle lanes of the
// last block follow along, weight 0) and, where asked for, at every point, with or as brightness temperatures.  The
// channel form (a GrtChannelArgs last in the joins; grt_launch_lw_channels) leaves the sums of an instrument's channels too.
constexpr int kRadianceChunk = GRT_RADIANCE_CHUNK;

// planck() solved for T: c2 w / log1p(c1 w^3 / I); +0.0 where there is no radiance
__device__ __forceinline__ double brightness_temperature(double I, double w)
{
    return I > 0. ? kPlanckC2*w/log1p((kPlanckC1*w*w*w)/I) : 0.;
}

// The chunk of viewing angles of blockIdx.z, for the radiance and the weighting kernel: n real angles from `first` on, c1
// of angle q minus its secant -- the padding angles of a last chunk repeat its last real one --, and angle_base, the chunk's
// first angle among the partial sums' [slot][angles]: the slot is the grid row's in the fused form and (column, draw of the
// launch) in the materialised one.
template <bool FUSED>
struct AngleChunk
{
    int first, n;
    double c1[kRadianceChunk];
    uint64_t angle_base;

    __device__ __forceinline__ AngleChunk(GrtRadianceArgs const &r, SolverRow const &row)
    {
        int const slot = FUSED ? row.slot : row.col*r.subcolumns + r.draw;
        first = (int)blockIdx.z*kRadianceChunk;
        n = r.angles - first < kRadianceChunk ? r.angles - first : kRadianceChunk;
#pragma unroll
        for (int q = 0; q < kRadianceChunk; ++q)
        {
            c1[q] = -r.secant[(uint64_t)row.col*r.angles + first + (q < n ? q : n - 1)];
        }
        angle_base = (uint64_t)slot*r.angles + first;
    }
};

// the partial sums of a chunk's N real angles: rows (up, down) of angle q at row_base + 2 q
template <int N>
__device__ __forceinline__ void radiance_partials(double const (&up)[kRadianceChunk], double const (&dn)[kRadianceChunk],
                                                  double wt, double *partials, uint64_t row_base)
{
    double val[2*N];
#pragma unroll
    for (int q = 0; q < N; ++q)
    {
        val[2*q] = up[q]*wt;
        val[2*q + 1] = dn[q]*wt;
    }
    block_partials<2*N, kSolverBlock>(val, partials, row_base, gridDim.x, blockIdx.x);
}

// The channel form's last step (GrtChannelArgs, grt_kernels.h): per channel of this block's list, real angle of the chunk
// and row, sum_i W_c(i) value(i) over the block's points -- W_c(i) = 0 outside the channel's span and in the idle lanes
// -- by WAVE_SUM, then waves_sum, as block_partials adds a row.  A wave none of whose 64 points lies in the span (the same
// in all its lanes: the span is the table's) leaves +0.0 without the tree.  kChannelChunk channels are summed before their
// sums are stored, one by each thread: row v of channel q at partials[(row_base + v) pairs + pair(q, block)].
constexpr int kChannelChunk = kSolverBlock/(2*kRadianceChunk);

__device__ __forceinline__ void channel_partials(GrtChannelArgs const &ch, double const (&up)[kRadianceChunk],
                                                 double const (&dn)[kRadianceChunk], int n, uint64_t row_base, uint64_t i,
                                                 bool live)
{
    static_assert(kChannelChunk*2*kRadianceChunk == kSolverBlock, "one thread stores one (channel, angle, row) of a chunk");
    __shared__ double part[kChannelChunk][2*kRadianceChunk][kSolverBlock/64];
    unsigned const block = blockIdx.x;
    int const lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long const at = (long long)i, wave_lo = at - lane, wave_hi = wave_lo + 63;
    int const k_lo = ch.block_start[block], k_hi = ch.block_start[block + 1];
    for (int k0 = k_lo; k0 < k_hi; k0 += kChannelChunk)
    {
        int const nb = k_hi - k0 < kChannelChunk ? k_hi - k0 : kChannelChunk;
        for (int q = 0; q < nb; ++q)
        {
            Window const w = window_of<uint64_t>(ch.entry, ch.block_list, k0 + q);
            long long const first = w.first(), last = first + w.count() - 1;    // (Window: span, weight, as first <= i <= last)
            if (first <= wave_hi && last >= wave_lo)
            {
                double const W = (live && at >= first && at <= last) ? ch.weights[(uint64_t)w.weight_at() + (uint64_t)(at - first)] : 0.;
#pragma unroll
                for (int k = 0; k < kRadianceChunk; ++k)
                {
                    if (k < n)
                    {
                        double su = W*up[k], sd = W*dn[k];
                        WAVE_SUM(su);
                        WAVE_SUM(sd);
                        if (lane == 0)
                        {
                            part[q][2*k][wave] = su;
                            part[q][2*k + 1][wave] = sd;
                        }
                    }
                }
            }
            else if (lane == 0)
            {
                for (int v = 0; v < 2*n; ++v)
                {
                    part[q][v][wave] = 0.;
                }
            }
        }
        __syncthreads();
        int const q = threadIdx.x/(2*kRadianceChunk), v = threadIdx.x % (2*kRadianceChunk);
        if (q < nb && v < 2*n)
        {
            Window const w = window_of<uint64_t>(ch.entry, ch.block_list, k0 + q);
            uint64_t const pair = (uint64_t)w.first_pair() + block - (unsigned)w.first_block();     // (Window: pair)
            ch.partials[(row_base + v)*ch.pairs + pair] = waves_sum<kSolverBlock/64>(part[q][v]);
        }
        __syncthreads();
    }
}

template <bool FUSED, typename... Joins>
__global__ __launch_bounds__(kSolverBlock) void lw_radiance_kernel(GrtLwArgs a, GrtRadianceArgs r, Joins... joins)
{
    static_assert(kRadianceChunk == 4, "the chunk's partial sums are listed for one to four angles");
    constexpr bool CHANNELS = has<GrtChannelArgs, Joins...>;     // (the channel form: a GrtChannelArgs last in the joins)
    uint64_t const i = (uint64_t)blockIdx.x*kSolverBlock + threadIdx.x;
    LwPoint<FUSED, Joins...> const p(a, i, joins...);         // (idle lanes of the last block follow along, weight 0)
    AngleChunk<FUSED> const ang(r, p.row);
    int const col = p.col, L = p.L, first = ang.first, n = ang.n;
    bool const live = p.live;
    double const w = p.w;

    double I[kRadianceChunk] = {0., 0., 0., 0.};
    for (int j = 0; j < L; ++j)
    {
        double const t = p.layer_tau(j);
        double const val = effective_planck(planck(p.tl[j], w), planck(p.tv[j + 1], w), t);
#pragma unroll
        for (int q = 0; q < kRadianceChunk; ++q)
        {
            I[q] = beam_step(I[q], val, beam_extinction(ang.c1[q], t));
        }
    }
    double const down[kRadianceChunk] = {I[0], I[1], I[2], I[3]};
    surface_step(I, p.emis, planck(a.t_surf[col], w));                   // (specular: the same angle, longwave.c:202)
    for (int j = L - 1; j >= 0; --j)
    {
        double const t = p.layer_tau(j);
        double const val = effective_planck(planck(p.tl[j], w), planck(p.tv[j], w), t);
#pragma unroll
        for (int q = 0; q < kRadianceChunk; ++q)
        {
            I[q] = beam_step(I[q], val, beam_extinction(ang.c1[q], t));
        }
    }

    if (live && (r.spectral != nullptr || r.brightness != nullptr))
    {
        uint64_t const base = (uint64_t)col*r.col_stride + (uint64_t)(2*first)*a.nw + i;
#pragma unroll
        for (int q = 0; q < kRadianceChunk; ++q)
        {
            if (q < n)
            {
                uint64_t const up_at = base + (uint64_t)(2*q)*a.nw, down_at = up_at + a.nw;
                if (r.spectral != nullptr)
                {
                    r.spectral[up_at] = I[q];
                    r.spectral[down_at] = down[q];
                }
                if (r.brightness != nullptr)
                {
                    r.brightness[up_at] = brightness_temperature(I[q], w);
                    r.brightness[down_at] = brightness_temperature(down[q], w);
                }
            }
        }
    }
    double const wt = trapezoid_weight(i, a.nw, a.dw, live);
    uint64_t const row_base = ang.angle_base*2;
    switch (n)                                                           // (the same in every thread of the workgroup)
    {
    case 1: radiance_partials<1>(I, down, wt, r.partials, row_base); break;
    case 2: radiance_partials<2>(I, down, wt, r.partials, row_base); break;
    case 3: radiance_partials<3>(I, down, wt, r.partials, row_base); break;
    default: radiance_partials<4>(I, down, wt, r.partials, row_base); break;
    }
    if constexpr (CHANNELS)
    {
        channel_partials(pick<GrtChannelArgs>(joins...), I, down, n, row_base, i, live);
    }
}

// The mean over the S draws of row `row` of channel c from its pairs, for both finishing kernels: a draw's pairs added in
// ascending order from the first, the draws' sums in order (draw s's row lies s `stride` rows behind draw 0's), divided by
// S where there is more than one, then by the sum of the channel's weights.
__device__ __forceinline__ double channel_row_mean(GrtChannelArgs const &ch, double const *partials, uint64_t c, uint64_t row,
                                                   uint64_t stride, int S)
{
    Window const w = window_at(ch.entry, c);
    int const npairs = (w.first() + w.count() - 1)/kSolverBlock - w.first_block() + 1;    // (Window::blocks, which moves the loop)
    double m = 0.;
    for (int s = 0; s < S; ++s)
    {
        double const *p = partials + (row + s*stride)*ch.pairs + w.first_pair();
        double x = p[0];
        for (int k = 1; k < npairs; ++k)
        {
            x += p[k];
        }
        m = s == 0 ? x : m + x;
    }
    if (S > 1)
    {
        m = m/(double)S;
    }
    return m/ch.sum_w[c];
}

// grt_launch_channel_finish (grt_kernels.h): the channels' pairs into channel radiances and brightness temperatures
constexpr int kChannelFinishBlock = 256;
__global__ __launch_bounds__(kChannelFinishBlock) void channel_finish_kernel(GrtChannelArgs ch, int ncol, int S, int rows, double *out,
                                                                double *brightness, uint64_t out_stride,
                                                                uint64_t out_offset)
{
    uint64_t const t = (uint64_t)blockIdx.x*kChannelFinishBlock + threadIdx.x;
    uint64_t const C = (uint64_t)ch.channels;
    if (t >= (uint64_t)ncol*rows*C)
    {
        return;
    }
    uint64_t const c = t % C, r = (t/C) % rows, col = t/(C*rows);
    double const R = channel_row_mean(ch, ch.partials, c, col*S*rows + r, rows, S);
    uint64_t const to = col*out_stride + out_offset + r*C + c;
    out[to] = R;
    if (brightness != nullptr)
    {
        brightness[to] = brightness_temperature(R, ch.center[c]);
    }
}

// ---- channel transmittances and contribution functions (grt_launch_lw_weighting; GrtWeightingArgs, grt_kernels.h) ----
// lw_weighting_kernel runs behind the channel form of lw_radiance_kernel on its arguments, instance and grid, and makes the
// downward sweep only: going down it knows a level's transmittance to space T_j, the layer's contribution K_j = ((1 - e_j)
// P_j) T_j to the upward radiance at the top and the downward radiance, and after the last layer the two surface rows.
// The rows of a layer leave at once, so no thread holds a profile: every thread writes its point's T_j and K_j of the
// chunk's real angles to an LDS tile [quantity][angle][point] -- consecutive threads, consecutive doubles --, and after a
// barrier the workgroup's threads take the channels of the block's list in turn -- consecutive threads, consecutive pairs --
// and each adds, per real angle and quantity, W_c(i) value(i) over the channel's points inside the block in ascending point
// index, one sequential sum from +0.0 each, a weight loaded once for all of them.  Two tiles in turn: a thread may still
// gather layer j while another writes layer j + 1, and the barrier of layer j + 1 lies between the gather of j and the
// writes of j + 2.  Idle lanes of the last block follow along to the barriers; what they write is never read, a channel's
// span lies on the grid.
__device__ __forceinline__ void weighting_gather(GrtChannelArgs const &ch, GrtWeightingArgs const &wa,
                                                 double const (&tile)[2][kRadianceChunk][kSolverBlock], int n, bool with_t,
                                                 uint64_t angle_base, uint64_t R, int k_row0, int row)
{
    unsigned const block = blockIdx.x;
    int const blk_lo = (int)block*kSolverBlock, blk_hi = blk_lo + kSolverBlock - 1;
    int const k_lo = ch.block_start[block], nch = ch.block_start[block + 1] - k_lo;
    bool const put_t = with_t && wa.transmittance, put_k = wa.contribution != 0;
    // one thread per channel of the block's list: a weight is loaded once for the chunk's angles and both quantities
    for (int k = threadIdx.x; k < nch; k += kSolverBlock)
    {
        Window const w = window_of<uint64_t>(ch.entry, ch.block_list, k_lo + k);
        int const first = w.first(), last = first + w.count() - 1;              // (Window: span, weight, cut to the block)
        int const lo = first > blk_lo ? first : blk_lo, hi = last < blk_hi ? last : blk_hi;
        double const *W = ch.weights + (uint64_t)w.weight_at() + (uint64_t)(lo - first);
        int const at = lo - blk_lo, count = hi - lo + 1;
        // (eight weight loads in flight ahead of the sums)
        double st[kRadianceChunk] = {0., 0., 0., 0.}, sk[kRadianceChunk] = {0., 0., 0., 0.};
#pragma unroll 8
        for (int p = 0; p < count; ++p)
        {
            double const wp = W[p];
#pragma unroll
            for (int q = 0; q < kRadianceChunk; ++q)
            {
                if (q < n)
                {
                    st[q] += wp*tile[0][q][at + p];
                    sk[q] += wp*tile[1][q][at + p];
                }
            }
        }
        uint64_t const pair = (uint64_t)w.first_pair() + block - (unsigned)w.first_block();     // (Window: pair)
#pragma unroll
        for (int q = 0; q < kRadianceChunk; ++q)
        {
            if (q < n)
            {
                double *to = wa.partials + ((angle_base + q)*R + (uint64_t)row)*ch.pairs + pair;
                if (put_t)
                {
                    to[0] = st[q];
                }
                if (put_k)
                {
                    to[(uint64_t)k_row0*ch.pairs] = sk[q];
                }
            }
        }
    }
}

template <bool FUSED, typename... Joins>
__global__ __launch_bounds__(kSolverBlock) void lw_weighting_kernel(GrtLwArgs a, GrtRadianceArgs r, GrtChannelArgs ch,
                                                                    GrtWeightingArgs wa, Joins... joins)
{
    __shared__ double tile[2][2][kRadianceChunk][kSolverBlock];      // [turn][T, K][angle][point]: 16 KiB
    uint64_t const i = (uint64_t)blockIdx.x*kSolverBlock + threadIdx.x;
    LwPoint<FUSED, Joins...> const p(a, i, joins...);         // (idle lanes of the last block follow along, never read)
    AngleChunk<FUSED> const ang(r, p.row);
    int const V = p.V, L = p.L, n = ang.n;
    double const w = p.w, emis = p.emis;
    uint64_t const angle_base = ang.angle_base;
    uint64_t const R = (uint64_t)((wa.transmittance ? V : 0) + (wa.contribution ? V + 1 : 0));
    int const k_row0 = wa.transmittance ? V : 0;                         // (the transmittance rows come first)

    double I[kRadianceChunk] = {0., 0., 0., 0.};
    double T[kRadianceChunk] = {1., 1., 1., 1.};
    for (int j = 0; j < L; ++j)
    {
        double const t = p.layer_tau(j);
        double const bc = planck(p.tl[j], w);
        double const val = effective_planck(bc, planck(p.tv[j + 1], w), t);      // the downward sweep's
        double const up = effective_planck(bc, planck(p.tv[j], w), t);           // the upward sweep's: P_j
        double (&tl_)[2][kRadianceChunk][kSolverBlock] = tile[j & 1];
#pragma unroll
        for (int q = 0; q < kRadianceChunk; ++q)
        {
            double const e = beam_extinction(ang.c1[q], t);
            if (q < n)
            {
                tl_[0][q][threadIdx.x] = T[q];
                tl_[1][q][threadIdx.x] = ((1. - e)*up)*T[q];
            }
            I[q] = beam_step(I[q], val, e);
            T[q] = T[q]*e;
        }
        __syncthreads();
        weighting_gather(ch, wa, tl_, n, true, angle_base, R, k_row0, j);
    }
    // level L and the surface's emission, then the reflected downwelling (specular, longwave.c:202)
    double const bs = planck(a.t_surf[p.col], w);
    for (int u = L; u <= L + 1; ++u)
    {
        double (&tl_)[2][kRadianceChunk][kSolverBlock] = tile[u & 1];
#pragma unroll
        for (int q = 0; q < kRadianceChunk; ++q)
        {
            if (q < n)
            {
                tl_[0][q][threadIdx.x] = T[q];
                tl_[1][q][threadIdx.x] = u == L ? (emis*bs)*T[q] : ((1 - emis)*I[q])*T[q];
            }
        }
        __syncthreads();
        weighting_gather(ch, wa, tl_, n, u == L, angle_base, R, k_row0, u);
    }
}

// grt_launch_weighting_finish (grt_kernels.h): the rows' pairs into transmittance profiles and contribution functions
__global__ __launch_bounds__(kChannelFinishBlock) void weighting_finish_kernel(GrtChannelArgs ch, GrtWeightingArgs wa, int ncol,
                                                                               int S, int A, int V, double *transmittance,
                                                                               uint64_t t_stride, uint64_t t_offset,
                                                                               double *contribution, uint64_t k_stride,
                                                                               uint64_t k_offset)
{
    uint64_t const t = (uint64_t)blockIdx.x*kChannelFinishBlock + threadIdx.x;
    uint64_t const C = (uint64_t)ch.channels, R = (uint64_t)((wa.transmittance ? V : 0) + (wa.contribution ? V + 1 : 0));
    if (t >= (uint64_t)ncol*A*R*C)
    {
        return;
    }
    uint64_t const c = t % C, r = (t/C) % R, angle = (t/(C*R)) % A, col = t/(C*R*A);
    double const out = channel_row_mean(ch, wa.partials, c, (col*S*A + angle)*R + r, A*R, S);
    uint64_t const nt = wa.transmittance ? (uint64_t)V : 0;
    if (r < nt)
    {
        transmittance[col*t_stride + t_offset + (angle*V + r)*C + c] = out;
    }
    else
    {
        contribution[col*k_stride + k_offset + (angle*(V + 1) + (r - nt))*C + c] = out;
    }
}

// ---- spectral form of few columns: the layers' terms first, by one thread per (layer, wavenumber) ----
// One column of the longwave band is 3 250 threads for lw_kernel<GRT_OUT_CHAINS> -- fifty waves on a thousand SIMDs, each with 120
// dependent layer steps of six exp.  What costs in a step does not depend on the step before: lw_terms_kernel fills
// terms[col][6 j + k][nw] with the four streams' extinctions exp(c1[s] t) and the effective Planck terms of the
// downward and of the upward sweep; lw_sweeps_kernel carries the four intensities through them, six layers' terms read
// ahead of the chain at a time.  Same expressions, same order, same doubles as lw_kernel<GRT_OUT_CHAINS>: identical fluxes.
constexpr int kTermsBlock = 256;
constexpr int kSweepBlock = 64;
constexpr int kSweepChunk = 6;

__global__ __launch_bounds__(kTermsBlock) void lw_terms_kernel(GrtLwArgs a)
{
    int const col = blockIdx.y;
    int const V = a.num_levels;
    int const L = V - 1;
    uint64_t const nw = a.nw;
    uint64_t const o = (uint64_t)blockIdx.x*kTermsBlock + threadIdx.x;       // j nw + i
    if (o >= (uint64_t)L*nw)
    {
        return;
    }
    uint64_t const j = o/nw;
    uint64_t const i = o - j*nw;
    double const w = a.w0 + i*a.dw;                                      // longwave.c:246
    uint64_t const at = (uint64_t)col*a.optics_stride + o;
    double const t = absorption_tau(a.tau, a.omega, at);
    double const *tl = a.t_layers + (uint64_t)col*L;
    double const *tv = a.t_levels + (uint64_t)col*V;
    double const bc = planck(tl[j], w);
    double *q = a.layer_terms + ((uint64_t)col*6*(uint64_t)L + 6*j)*nw + i;
#pragma unroll
    for (int s = 0; s < 4; ++s)
    {
        q[(uint64_t)s*nw] = extinction(s, t);
    }
    q[4*nw] = effective_planck(bc, planck(tv[j + 1], w), t);             // the downward sweep's (longwave.c:186-193)
    q[5*nw] = effective_planck(bc, planck(tv[j], w), t);                 // the upward sweep's (:204-211)
}

__global__ __launch_bounds__(kSweepBlock) void lw_sweeps_kernel(GrtLwArgs a)
{
    uint64_t const i = (uint64_t)blockIdx.x*kSweepBlock + threadIdx.x;
    int const col = blockIdx.y;
    if (i >= a.nw)
    {
        return;
    }
    int const V = a.num_levels;
    int const L = V - 1;
    uint64_t const nw = a.nw;
    double const w = a.w0 + i*a.dw;
    double const emis = a.emis[(uint64_t)col*a.emis_stride + i];
    double const *tt = a.layer_terms + (uint64_t)col*6*(uint64_t)L*nw + i;
    LevelSink<false, false> sink(a, col, i, true);
    double I[4] = {0., 0., 0., 0.};
    sink.put_zero(0, true);                                              // longwave.c:171
    for (int jb = 0; jb < L; jb += kSweepChunk)
    {
        double ex[kSweepChunk][4], vl[kSweepChunk];
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            double const *q = tt + (uint64_t)(6*(jb + u < L ? jb + u : L - 1))*nw;
#pragma unroll
            for (int s = 0; s < 4; ++s)
            {
                ex[u][s] = q[(uint64_t)s*nw];
            }
            vl[u] = q[4*nw];
        }
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            int const j = jb + u;
            if (j < L)
            {
                sink.put(j + 1, true, stream_step(I, vl[u], [&](int s) { return ex[u][s]; }));
            }
        }
    }
    sink.put(L, false, surface_step(I, emis, planck(a.t_surf[col], w)));
    for (int jb = L - 1; jb >= 0; jb -= kSweepChunk)
    {
        double ex[kSweepChunk][4], vl[kSweepChunk];
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            double const *q = tt + (uint64_t)(6*(jb - u >= 0 ? jb - u : 0))*nw;
#pragma unroll
            for (int s = 0; s < 4; ++s)
            {
                ex[u][s] = q[(uint64_t)s*nw];
            }
            vl[u] = q[5*nw];
        }
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            int const j = jb - u;
            if (j >= 0)
            {
                sink.put(j, false, stream_step(I, vl[u], [&](int s) { return ex[u][s]; }));
            }
        }
    }
}

// ---- several surface tiles per column on one walk through the layers (grt_launch_lw_tiles; GrtTileArgs, grt_kernels.h) ----
// Of lw_kernel<GRT_OUT_ROWS>, the downward sweep does not know the surface, and a layer of the upward sweep is I_s <-
// (1 - e_s) val + I_s e_s with val and the four e_s the atmosphere's alone.  Grid row y is the six-row instance's (a
// column, or a column and cloud draw: LwPoint as it is), blockIdx.z a chunk of TN consecutive tiles: the thread makes the
// downward sweep once, gives each tile of its chunk its own copy of the four streams at the surface -- the tile's
// emissivity row, planck() of the tile's temperature, surface_step --, and on the way up forms a layer's optical depth, its
// two Planck terms and its four extinctions once and runs beam_step and the c2 sum per tile, in stream_step's order.
// Every tile's six rows leave through a LevelSink at the tile's slot (c tiles + t) subcolumns + s: lw_kernel's doubles
// through lw_kernel's sums.  What the chunk is and which of its tiles the column has: TileChunk (optics_dev.h); tiles past
// the column's last are skipped by a flag that is uniform per workgroup.
// the three rows of one direction, as LevelSink::put keeps them (TOA, surface, user level)
__device__ __forceinline__ void keep_row(double (&three)[3], int lev, int V, int user, double x)
{
    three[0] = lev == 0 ? x : three[0];
    three[1] = lev + 1 == V ? x : three[1];
    three[2] = lev == user ? x : three[2];
}

template <int TN, typename... Joins>
__global__ __launch_bounds__(kSolverBlock) void lw_tile_kernel(GrtLwArgs a, GrtTileArgs tl, Joins... joins)
{
    uint64_t const i = (uint64_t)blockIdx.x*kSolverBlock + threadIdx.x;
    LwPoint<true, Joins...> const p(a, i, joins...);             // (idle lanes of the last block follow along, weight 0)
    int const L = p.L, V = p.V, user = a.user_level;
    TileChunk<TN> const chunk(tl, p.row, joins...);
    int const T = chunk.T, k0 = chunk.k0, S = chunk.S, draw = chunk.draw;
    double const w = p.w;

    // the downward sweep, shared by the tiles
    double down[3] = {0., 0., 0.};                                       // longwave.c:171
    double I0[4] = {0., 0., 0., 0.};
    for (int j = 0; j < L; ++j)
    {
        double const t = p.layer_tau(j);
        double const val = effective_planck(planck(p.tl[j], w), planck(p.tv[j + 1], w), t);
        keep_row(down, j + 1, V, user, stream_step(I0, val, [&](int s) { return extinction(s, t); }));
    }
    // the surface of each tile of the chunk, on its own copy of the streams
    double I[TN][4], up[TN][3];
#pragma unroll
    for (int u = 0; u < TN; ++u)
    {
        up[u][0] = up[u][1] = up[u][2] = 0.;
#pragma unroll
        for (int s = 0; s < 4; ++s)
        {
            I[u][s] = I0[s];
        }
        if (chunk.live(u))
        {
            uint64_t const tile = (uint64_t)p.col*T + k0 + u;
            double const emis = tl.rows != nullptr ? tl.rows[tile*p.nw + p.ii] : p.emis;
            keep_row(up[u], L, V, user, surface_step(I[u], emis, planck(tl.t_surf[tile], w)));
        }
    }
    for (int j = L - 1; j >= 0; --j)
    {
        double const t = p.layer_tau(j);
        double const val = effective_planck(planck(p.tl[j], w), planck(p.tv[j], w), t);
        double e[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
        {
            e[s] = extinction(s, t);
        }
#pragma unroll
        for (int u = 0; u < TN; ++u)
        {
            if (chunk.live(u))
            {
                keep_row(up[u], j, V, user, stream_step(I[u], val, [&](int s) { return e[s]; }));
            }
        }
    }
#pragma unroll
    for (int u = 0; u < TN; ++u)
    {
        if (!chunk.live(u))
        {
            continue;
        }
        LevelSink<true, false> sink(a, (p.col*T + k0 + u)*S + draw, i, p.live);       // (TileChunk's slot rule: a copy)
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            sink.out[k] = up[u][k];
            sink.out[3 + k] = down[k];
        }
        __syncthreads();                            // (block_partials' LDS is the tile before's: every wave has read it)
        sink.finish(a);
    }
}

// the one launch site of lw_kernel: the instance of OUT and of the joined arguments' types, on the instance's grid and LDS
template <GrtSolverOutput OUT, typename... Joins>
int launch(hipStream_t s, GrtSolverInstance const &in, GrtLwArgs const &a, Joins const &...joins)
{
    dim3 const grid(grt_solver_blocks(a.nw), (unsigned)grt_solver_grid_rows(&in, a.ncol), 1);
    hipLaunchKernelGGL((lw_kernel<OUT, Joins...>), grid, dim3(kSolverBlock), grt_solver_lds(&in, a.num_levels), s, a,
                       joins...);
    return (int)hipGetLastError();
}

// ... and of lw_radiance_kernel: the instance's grid rows, the chunks of angles along z
template <bool FUSED, typename... Joins>
int launch_radiances(hipStream_t s, GrtSolverInstance const &in, GrtLwArgs const &a, GrtRadianceArgs const &r,
                     Joins const &...joins)
{
    dim3 const grid(grt_solver_blocks(a.nw), (unsigned)grt_solver_grid_rows(&in, a.ncol),
                    (unsigned)((r.angles + kRadianceChunk - 1)/kRadianceChunk));
    hipLaunchKernelGGL((lw_radiance_kernel<FUSED, Joins...>), grid, dim3(kSolverBlock), 0, s, a, r, joins...);
    return (int)hipGetLastError();
}

// ... and of lw_weighting_kernel, on the same grid
template <bool FUSED, typename... Joins>
int launch_weighting(hipStream_t s, GrtSolverInstance const &in, GrtLwArgs const &a, GrtRadianceArgs const &r,
                     GrtChannelArgs const &c, GrtWeightingArgs const &w, Joins const &...joins)
{
    dim3 const grid(grt_solver_blocks(a.nw), (unsigned)grt_solver_grid_rows(&in, a.ncol),
                    (unsigned)((r.angles + kRadianceChunk - 1)/kRadianceChunk));
    hipLaunchKernelGGL((lw_weighting_kernel<FUSED, Joins...>), grid, dim3(kSolverBlock), 0, s, a, r, c, w, joins...);
    return (int)hipGetLastError();
}

// ... and of lw_tile_kernel: TN tiles per thread, the six-row instance's grid rows, the launch's chunks along z
template <int TN, typename... Joins>
int launch_tiles(hipStream_t s, GrtLwArgs const &a, GrtTileArgs const &t, int draws, Joins const &...joins)
{
    if (!grt_tile_args_ok(&t, TN) || t.t_surf == nullptr || (uint64_t)a.ncol*(uint64_t)draws > 65535u || t.chunk_count > 65535)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL((lw_tile_kernel<TN, Joins...>), dim3(grt_solver_blocks(a.nw), (unsigned)(a.ncol*draws), (unsigned)t.chunk_count),
                       dim3(kSolverBlock), 0, s, a, t, joins...);
    return (int)hipGetLastError();
}

} // namespace

extern "C" unsigned grt_solver_blocks(uint64_t nw)
{
    return (unsigned)((nw + kSolverBlock - 1)/kSolverBlock);
}

extern "C" int grt_launch_ck_lw(void *stream, GrtCkSolveArgs const *a)
{
    if (!grt_ck_solve_args_ok(a))
    {
        return (int)hipErrorInvalidValue;
    }
    uint64_t const threads = (uint64_t)a->ncol*(uint64_t)a->num_bins*(uint64_t)a->num_classes;
    hipLaunchKernelGGL(ck_lw_kernel, dim3((unsigned)((threads + kSolverBlock - 1)/kSolverBlock)), dim3(kSolverBlock), 0,
                       (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_lw(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a)
{
    uint64_t const cells = (uint64_t)(a->num_levels - 1)*a->nw;
    if (!grt_solver_instance_ok(*in, *a) || in->scatter != nullptr ||       // (grt_launch_lw_scatter's)
        (in->out == GRT_OUT_LAYERS && (a->layer_terms == nullptr || cells > 0xffffffffull*kTermsBlock)))
    {
        return (int)hipErrorInvalidValue;
    }
    hipStream_t const s = (hipStream_t)stream;
    if (in->out == GRT_OUT_LAYERS)
    {
        hipLaunchKernelGGL(lw_terms_kernel, dim3((unsigned)((cells + kTermsBlock - 1)/kTermsBlock), a->ncol, 1),
                           dim3(kTermsBlock), 0, s, *a);
        hipLaunchKernelGGL(lw_sweeps_kernel, dim3((unsigned)((a->nw + kSweepBlock - 1)/kSweepBlock), a->ncol, 1),
                           dim3(kSweepBlock), 0, s, *a);
        return (int)hipGetLastError();
    }
    // every instance of lw_kernel there is (grt_lw_instance_exists)
    auto const site = [&](auto, auto out, auto const &...joins) { return launch<decltype(out)::value>(s, *in, *a, joins...); };
    return grt_launch_output<grt_lw_instance_exists>(in->out, grt_solver_joins(*in), site);
}

extern "C" int grt_launch_lw_surface_jacobian(void *stream, GrtLwArgs const *a, double *jacobian)
{
    if (a == nullptr || jacobian == nullptr || a->ncol < 1 || a->ncol > 65535 || a->nw < 2 || a->num_levels < 2 ||
        a->tau == nullptr || a->t_surf == nullptr || a->emis == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(lw_surface_jacobian_kernel, dim3((unsigned)((a->nw + kJacobianBlock - 1)/kJacobianBlock), a->ncol, 1),
                       dim3(kJacobianBlock), 0, (hipStream_t)stream, *a, jacobian);
    return (int)hipGetLastError();
}

// grt_launch_lw_radiances, or -- c given -- grt_launch_lw_channels: the instance of the join, with c last in its joins; or
// -- w given too -- grt_launch_lw_weighting: lw_weighting_kernel's instance of the join
static int launch_lw_radiances(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a, GrtRadianceArgs const *r,
                               GrtChannelArgs const *c, GrtWeightingArgs const *w = nullptr)
{
    if (in == nullptr || a == nullptr || !grt_radiance_args_ok(r) || in->zeniths != nullptr || a->ncol < 1 || a->nw < 2 ||
        a->num_levels < 2 || grt_solver_grid_rows(in, a->ncol) > 65535 || a->t_layers == nullptr || a->t_levels == nullptr ||
        a->t_surf == nullptr || a->emis == nullptr || (in->clouds != nullptr && in->subcolumns != nullptr) ||
        (in->clouds != nullptr && !grt_cloud_args_ok(in->clouds)) ||
        (in->aerosols != nullptr && !grt_aerosol_args_ok(in->aerosols)) ||
        (in->subcolumns != nullptr && !grt_subcolumn_args_ok(in->subcolumns)))
    {
        return (int)hipErrorInvalidValue;
    }
    hipStream_t const s = (hipStream_t)stream;
    // (the materialised instance reads the pass's tau, omega on the grid; bins, zeniths, direct and jacobian are not read)
    GrtSolverInstance const front = {in->out, in->clouds, in->aerosols, in->subcolumns};
    if (grt_out_fused(in->out) ? a->tau_gas == nullptr || a->n_layer == nullptr : a->tau == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    // every instance of lw_radiance_kernel there is, c last in its joins where given, and of lw_weighting_kernel
    // (grt_lw_radiance_instance_exists)
    auto const launch_form = [&](auto fused) -> int
    {
        constexpr bool FUSED = decltype(fused)::value;
        if (w != nullptr)
        {
            auto const site = [&](auto, auto, auto const &...joins)
            { return launch_weighting<FUSED>(s, *in, *a, *r, *c, *w, joins...); };
            return grt_launch_joined<grt_lw_radiance_instance_exists, FUSED>(grt_solver_joins(front), site);
        }
        auto const site = [&](auto, auto, auto const &...joins) { return launch_radiances<FUSED>(s, *in, *a, *r, joins...); };
        return grt_launch_joined<grt_lw_radiance_instance_exists, FUSED>(std::tuple_cat(grt_solver_joins(front), std::make_tuple(c)),
                                                                         site);
    };
    return grt_out_fused(in->out) ? launch_form(std::true_type{}) : launch_form(std::false_type{});
}

extern "C" int grt_launch_lw_radiances(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a, GrtRadianceArgs const *r)
{
    return launch_lw_radiances(stream, in, a, r, nullptr);
}

extern "C" int grt_launch_lw_channels(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a, GrtRadianceArgs const *r,
                                      GrtChannelArgs const *c)
{
    return grt_channel_args_ok(c) ? launch_lw_radiances(stream, in, a, r, c) : (int)hipErrorInvalidValue;
}

extern "C" int grt_launch_channel_finish(void *stream, GrtChannelArgs const *c, int ncol, int subcolumns, int angles,
                                         double *out, double *brightness, uint64_t out_stride, uint64_t out_offset)
{
    if (!grt_channel_args_ok(c) || ncol < 1 || subcolumns < 1 || angles < 1 || out == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    int const rows = 2*angles;
    uint64_t const threads = (uint64_t)ncol*rows*(uint64_t)c->channels;
    hipLaunchKernelGGL(channel_finish_kernel, dim3((unsigned)((threads + kChannelFinishBlock - 1)/kChannelFinishBlock)),
                       dim3(kChannelFinishBlock), 0, (hipStream_t)stream, *c, ncol, subcolumns, rows, out, brightness,
                       out_stride, out_offset);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_lw_weighting(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a, GrtRadianceArgs const *r,
                                       GrtChannelArgs const *c, GrtWeightingArgs const *w)
{
    return grt_channel_args_ok(c) && grt_weighting_args_ok(w) ? launch_lw_radiances(stream, in, a, r, c, w) :
                                                                  (int)hipErrorInvalidValue;
}

extern "C" int grt_launch_weighting_finish(void *stream, GrtChannelArgs const *c, GrtWeightingArgs const *w, int ncol,
                                           int subcolumns, int angles, int num_levels, double *transmittance,
                                           uint64_t t_stride, uint64_t t_offset, double *contribution, uint64_t k_stride,
                                           uint64_t k_offset)
{
    if (!grt_channel_args_ok(c) || !grt_weighting_args_ok(w) || ncol < 1 || subcolumns < 1 || angles < 1 || num_levels < 2 ||
        (w->transmittance && transmittance == nullptr) || (w->contribution && contribution == nullptr))
    {
        return (int)hipErrorInvalidValue;
    }
    uint64_t const threads = (uint64_t)ncol*angles*(uint64_t)grt_weighting_rows(w, num_levels)*(uint64_t)c->channels;
    if ((threads + kChannelFinishBlock - 1)/kChannelFinishBlock > 0x7fffffffull)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(weighting_finish_kernel, dim3((unsigned)((threads + kChannelFinishBlock - 1)/kChannelFinishBlock)),
                       dim3(kChannelFinishBlock), 0, (hipStream_t)stream, *c, *w, ncol, subcolumns, angles, num_levels,
                       transmittance, t_stride, t_offset, contribution, k_stride, k_offset);
    return (int)hipGetLastError();
}

extern "C" int grt_tile_chunk(GrtSubcolumnArgs const *sc, GrtAerosolArgs const *ae)
{
    GrtSolverInstance const joined = {GRT_OUT_ROWS, nullptr, ae, sc};
    return grt_tile_chunk_of(grt_join_set(grt_solver_joins(joined)));
}

extern "C" int grt_launch_lw_tiles(void *stream, GrtLwArgs const *a, GrtTileArgs const *t, GrtSubcolumnArgs const *sc,
                                   GrtAerosolArgs const *ae)
{
    GrtSolverInstance const in = {GRT_OUT_ROWS}, joined = {GRT_OUT_ROWS, nullptr, ae, sc};
    if (a == nullptr || t == nullptr || !grt_solver_instance_ok(in, *a) || a->t_layers == nullptr || a->t_levels == nullptr ||
        a->emis == nullptr || (sc != nullptr && !grt_subcolumn_args_ok(sc)) || (ae != nullptr && !grt_aerosol_args_ok(ae)))
    {
        return (int)hipErrorInvalidValue;
    }
    hipStream_t const s = (hipStream_t)stream;
    int const draws = sc != nullptr ? sc->count : 1;
    auto const site = [&](auto set, auto const &...joins)
    { return launch_tiles<grt_tile_chunk_of(decltype(set)::value)>(s, *a, *t, draws, joins...); };
    return grt_launch_joined<grt_tile_instance_exists>(grt_solver_joins(joined), site);
}
