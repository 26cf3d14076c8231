// k_shortwave.hip -- two-stream delta-Eddington + adding shortwave solver for gfx950.
//
// Reference: shortwave/src/shortwave.c:68-453 (delta_eddington_scaling_jww1976,
// meador_weaver_1980, eddington_mw1980, sw_adding, sw_flux, sw_fluxes_kernel).
// One thread per (wavenumber, column), coalesced (layer|level, wavenumber) rows.
//
// The reference keeps five 200-element layer arrays plus three level arrays per thread
// (scratch spills on a GPU).  We run the adding method as two sweeps with O(1) state:
//   sweep 1 (surface -> TOA): layer R/T from the Eddington solution, the downward-beam
//     reflectances of shortwave.c:280-294 are parked in the output rows themselves
//     (flux_up[i] <- R_dir_downward[i], flux_down[i] <- R_dif_downward[i]);
//   sweep 2 (TOA -> surface): layer R/T are recomputed (same inputs, same values), the
//     upward-beam reflectance of :299-306 is carried in registers, and each parked
//     pair is consumed and overwritten by the final fluxes of :308-329,401-405,447-451.
// Every expression keeps the reference's evaluation order, so results are identical.  Measured: in that
// form the kernel is fp64-VALU-bound (two delta-Eddington solutions per layer and sweep: 70 000 instructions per wave),
// not HBM-bound.  The fused six-row clear-sky instance, the production pipeline's, therefore trades bytes for flops: its
// first sweep parks the five properties of every layer with the reflectances and its second sweep reads them back (the
// same doubles: identical fluxes) -- 0.69 instead of 1.04 ms for 8 columns, at 4.2 TB/s.  sw_kernel has one instance per
// GrtSolverInstance that exists: what leaves it is its OUT, and what joins gas and Rayleigh or rides with them is the types
// of its pack, in the order of the GRT_JOIN_ bits.  Which instances exist is grt_sw_instance_exists' rule (grt_kernels.h),
// and grt_launch_joined (solver_dispatch.h) takes a launch from the pointers that are set to the kernel's pack.
// sw_zenith_kernel is the six-row instance for several sun angles per column on shared layer properties
// (grt_launch_sw_zeniths), and sw_tile_kernel, behind it, the six-row instance for several surface tiles per column
// (grt_launch_sw_tiles): the layer properties once for a chunk of tiles, what reads the albedo per tile.
// Said once for the three: the one sweep's state and step (OneSweep), what leaves it at the surface (one_sweep_exit), its
// rule (GRT_SW_ONE_SWEEP, grt_kernels.h), a night row's zeros (night_fill), a grid row and a chunk of tiles (solver_row,
// TileChunk: optics_dev.h).  sw_zenith_kernel keeps its own grid row and split of the step, and the tile kernels their
// slot: each says at the copy which shared text it follows (as members they cost scalar spills or instructions).
// The in-kernel range checks of the reference are no-ops on device builds
// (debug.h:105-116) and are not restated.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../grt_kernels.h"
#include "optics_dev.h"
#include "solver_dispatch.h"
#include "exp_pair.h"

#pragma clang fp contract(off)

namespace {

constexpr double kMaxExpArg = 700.;   // grtcode_config.h:41

struct LayerRT { double R, T, Tpure; };

// exp(+-t k) of the last Eddington solution of this layer: the direct-beam and the diffuse solution share k and, unless
// one of them had its optical depth clamped (shortwave.c:137-145), t -- then the second call takes the first call's two
// exponentials (same arguments, same values) instead of evaluating them again
struct ExpKt { double t, tkp, tkm; bool valid; };

// The gammas of the Eddington approximation (shortwave.c:226-230) for a beam of cosine mu
struct Gammas { double g1, g2, g3; };

__device__ __forceinline__ Gammas eddington_gammas(double omega, double g, double mu)
{
    Gammas gm;
    gm.g1 = 0.25*(7. - omega*(4. + 3.*g));
    gm.g2 = -0.25*(1. - omega*(4. - 3.*g));
    gm.g3 = 0.25*(2. - 3.*g*mu);
    return gm;
}

// T_pure of a layer for a beam of cosine mu (shortwave.c:114-168): what passes through without being absorbed or
// scattered -- exp(-tau/mu) without scattering, else exp(-t/mu) of the optical depth t that the clamp of :137-145 leaves, and
// 1 for a layer that holds nothing (exp(t/mu) <= 1).  The one place T_pure is worked out: eddington() below and the direct
// beam of the materialised form (sw_direct_beam_kernel) both call it.  rest(k, t, tp, tm) runs on the way, in a scattering
// layer that holds something: what the rest of the Eddington solution there takes over -- k, t and exp(+-t/mu).
template <typename Rest>
__device__ __forceinline__ double pure_transmission(double omega, double tau, double mu, Gammas const &gm, Rest &&rest)
{
    if (omega <= 0.0)
    {
        return grt_exp(-tau/mu);         // (exp_pair.h: the constants this kernel holds anyway)
    }
    double const k = sqrt(gm.g1*gm.g1 - gm.g2*gm.g2);
    double t = tau;
    double const tau_over_mu = tau/mu;
    if (1./mu > k && tau_over_mu > kMaxExpArg)
    {
        t = kMaxExpArg*mu;
    }
    else if (tau*k > kMaxExpArg)
    {
        t = kMaxExpArg/k;
    }
    // (t is tau unless a clamp struck: the quotient above is then t/mu -- the same division of the same doubles)
    double t_over_mu = tau_over_mu;
    if (t != tau)
    {
        t_over_mu = t/mu;
    }
    // (the three exponential pairs of a layer -- exp(+-t/mu) here and in the other beam's call, exp(+-t k) -- each
    // through one shared reduction and polynomial: exp_pair.h)
    double tp, tm;
    grt_exp_pair(t_over_mu, &tp, &tm);
    if (tp <= 1.0)
    {
        return 1.;
    }
    rest(k, t, tp, tm);
    return tm;
}

// shortwave.c:97-207 (+ gamma definitions :226-230).  WITH_PURE mirrors T_pure != NULL.
template <bool WITH_PURE>
__device__ __forceinline__ LayerRT eddington(double omega, double tau, double mu, double g, ExpKt &shared)
{
    LayerRT r;
    Gammas const gm = eddington_gammas(omega, g, mu);
    double const gamma1 = gm.g1, gamma2 = gm.g2, gamma3 = gm.g3;
    bool solved = false;
    r.R = 0.;
    r.Tpure = pure_transmission(omega, tau, mu, gm, [&](double k, double t, double tp, double tm)
    {
        double const gamma4 = 1. - gamma3;
        double const alpha1 = gamma1*gamma4 + gamma2*gamma3;
        double const alpha2 = gamma1*gamma3 + gamma2*gamma4;
        double tkm, tkp;
        if (shared.valid && shared.t == t)
        {
            tkm = shared.tkm;
            tkp = shared.tkp;
        }
        else
        {
            grt_exp_pair(t*k, &tkp, &tkm);
            shared.t = t;
            shared.tkm = tkm;
            shared.tkp = tkp;
            shared.valid = true;
        }
        if (omega >= 1.)
        {
            r.R = (1./(1. + gamma1*t))*(gamma1*t + (gamma3 - gamma1*mu)*(1. - tm));
            r.T = 1. - r.R;
        }
        else
        {
            r.R = (omega/((1. - k*k*mu*mu)*((k + gamma1)*tkp + (k - gamma1)*tkm)))*
                  ((1. - k*mu)*(alpha2 + k*gamma3)*tkp - (1. + k*mu)*(alpha2 - k*gamma3)*tkm -
                  2.*k*(gamma3 - alpha2*mu)*tm);
            r.T = tm*(1. - (omega/((1. - k*k*mu*mu)*((k + gamma1)*tkp +
                  (k - gamma1)*tkm)))*((1. + k*mu)*(alpha1 + k*gamma4)*tkp -
                  (1. - k*mu)*(alpha1 - k*gamma4)*tkm - 2.*k*(gamma4 + alpha1*mu)*tp));
        }
        solved = true;
    });
    if (!solved)
    {
        r.T = r.Tpure;      // (no scattering, :117-122: R = 0, T = exp(-tau/mu); nothing in the layer, :152-157: R = 0, T = 1)
    }
    if (WITH_PURE)
    {
        if (r.Tpure > r.T)
        {
            r.T = r.Tpure;
        }
    }
    return r;
}

struct LayerProps { double Rdir, Tdir, Tpure, Rdif, Tdif; };

// shortwave.c:86-89.  With g = 0 exactly -- every clear-sky layer: Rayleigh scattering and absorbing gases -- the
// scaling is the identity in floating point too (g/(g + 1) = 0, f = 0, (1 - 0) omega/(1 - omega 0) = omega/1,
// tau (1 - 0) = tau: each step exact), so the two divisions are skipped and the same doubles go on
__device__ __forceinline__ void delta_scaling(double omega, double g, double tau, double &os, double &gs, double &ts)
{
    gs = g; os = omega; ts = tau;
    if (g != 0. || !(omega*0. == 0.))           // (an infinite or NaN omega takes the expressions as written)
    {
        gs = g/(g + 1.);
        double const f = g*g;
        os = (1. - f)*omega/(1. - omega*f);
        ts = tau*(1. - omega*f);
    }
}

__device__ __forceinline__ LayerProps layer_props(double omega, double g, double tau,
                                                  double mu_dir, double mu_dif)
{
    double gs, os, ts;
    delta_scaling(omega, g, tau, os, gs, ts);
    ExpKt shared = {0., 0., 0., false};
    LayerRT const d = eddington<true>(os, ts, mu_dir, gs, shared);
    LayerRT const s = eddington<false>(os, ts, mu_dif, gs, shared);
    LayerProps p;
    p.Rdir = d.R; p.Tdir = d.T; p.Tpure = d.Tpure; p.Rdif = s.R; p.Tdif = s.T;
    return p;
}

// The five properties of a layer as rows q, q + nw, .. q + 4 nw: Rdir, Tdir, Tpure, Rdif, Tdif (the fused form's park,
// the layers form's layer_props)
__device__ __forceinline__ void store_props(double *q, uint64_t nw, LayerProps const &p)
{
    q[0] = p.Rdir; q[nw] = p.Tdir; q[2*nw] = p.Tpure; q[3*nw] = p.Rdif; q[4*nw] = p.Tdif;
}

__device__ __forceinline__ LayerProps load_props(double const *q, uint64_t nw)
{
    LayerProps p;
    p.Rdir = q[0]; p.Tdir = q[nw]; p.Tpure = q[2*nw]; p.Rdif = q[3*nw]; p.Tdif = q[4*nw];
    return p;
}

// sweep 1 (shortwave.c:280-294), one layer up: the downward-beam reflectances at the layer's top from those at its bottom
__device__ __forceinline__ void sweep1_step(LayerProps const &p, double &Rdir_dn, double &Rdif_dn)
{
    double const A = p.Tpure;
    double const B = 1./(1. - p.Rdif*Rdif_dn);
    double const ndir = p.Rdir + (A*Rdir_dn + (p.Tdir - A)*Rdif_dn)*p.Tdif*B;
    double const ndif = p.Rdif + p.Tdif*p.Tdif*Rdif_dn*B;
    Rdir_dn = ndir;
    Rdif_dn = ndif;
}

// sweep 2 (shortwave.c:299-316) from the top: the direct and diffuse beams at level lev and R_dif_upward above it
struct Sweep2
{
    double dir = 1.;
    double dif = 0.;
    double Rup2 = 0.;     // R_dif_upward[lev-2]
    double Rup = 0.;      // R_dif_upward[lev-1]
};

// ... one layer down: layer lev - 1 takes the sweep to level lev
__device__ __forceinline__ void sweep2_step(Sweep2 &s, LayerProps const &p, int lev)
{
    // R_dif_upward[lev-1]  (:299-306)
    s.Rup2 = s.Rup;
    if (lev == 1)
    {
        s.Rup = p.Rdif;
    }
    else
    {
        double const Bu = 1./(1. - p.Rdif*s.Rup2);
        s.Rup = p.Rdif + p.Tdif*p.Tdif*s.Rup2*Bu;
    }
    if (lev > 1)
    {
        double const C = 1./(1. - p.Rdif*s.Rup2);
        s.dif = (s.dir*p.Rdir*s.Rup2 + s.dif)*p.Tdif*C + s.dir*(p.Tdir - p.Tpure);
    }
    else
    {
        s.dif = s.dir*(p.Tdir - p.Tpure);
    }
    s.dir *= p.Tpure;
}

// The fluxes at a level (shortwave.c:318-329) from the beams that reach it, the reflectance Rup of what lies above it to
// diffuse light from below, and the downward-beam reflectances rdir, rdif of what lies below it
__device__ __forceinline__ void level_flux(double dir, double dif, double Rup, double rdir, double rdif, double &up,
                                           double &dn)
{
    double const B = 1./(1. - rdif*Rup);
    up = (dir*rdir + dif*rdif)*B;
    dn = dir*(1. + rdir*Rup*B) + dif*B;
}

// ... scaled as shortwave.c:401-405 and :447-451 and handed to the sink
template <typename Sink>
__device__ __forceinline__ void put_level(Sink &sink, int lev, double up, double dn, double scale, double tsi)
{
    up *= scale;
    dn *= scale;
    sink.put(lev, false, tsi*up);
    sink.put(lev, true, tsi*dn);
}

// the direct beam that reaches a level (shortwave.c:306, :323), scaled as the downward flux beside it is
template <typename Sink>
__device__ __forceinline__ void put_direct(Sink &sink, int lev, double dir, double scale, double tsi)
{
    dir *= scale;
    sink.put_direct(lev, tsi*dir);
}

// The one sweep of the fused six-row forms when no flux is asked for between the top and the surface (GRT_SW_ONE_SWEEP's
// rule: user level -1, 0 or L -- the pipeline's usual call), top to surface, nothing parked.  The reference's downward
// sweep (shortwave.c:299-329) carries the direct beam, the diffuse beam over a black lower boundary and the reflectance
// Ru of the atmosphere above; two more numbers ride along -- Rd, the reflectance of the slab above to the direct beam, and
// Tu, its transmission of diffuse light from below to the top: adding layer p below the slab,
//     Rd' = Rd + Tu (dir Rdir_p + dif Rdif_p) C,   Tu' = Tu Tdif_p C,   C = 1/(1 - Rdif_p Ru)
// (the slab's own reflection plus what layer p sends back up through it; all orders of reflection between the two in
// C).  At the surface the reference's expressions give the fluxes there, and the top's upward flux is
// Rd + Tu x (the upward flux at the surface): the adding method's identity for what shortwave.c:280-294 builds from
// the bottom (R_dir_downward[0]) -- the same number to rounding (1e-15), not to the bit; the surface fluxes are the
// reference's own operations.  Two delta-Eddington solutions per layer, and no 80 bytes per layer and wavenumber parked.
struct OneSweep
{
    double dir = 1., dif = 0., Ru = 0., Rd = 0., Tu = 1.;
    // layer p below the slab (C, Tu and Ru depend on the optics alone; Rd and dif read the slab as it was above the layer)
    __device__ __forceinline__ void step(LayerProps const &p)
    {
        double const C = 1./(1. - p.Rdif*Ru);
        Rd = Rd + Tu*((dir*p.Rdir + dif*p.Rdif)*C);
        Tu = Tu*(p.Tdif*C);
        dif = (dir*p.Rdir*Ru + dif)*p.Tdif*C + dir*(p.Tdir - p.Tpure);          // shortwave.c:312-316
        Ru = p.Rdif + p.Tdif*p.Tdif*Ru*C;                                        // :299-306
        dir *= p.Tpure;
    }
};

// ... and what leaves it over a surface of these albedos: the fluxes there, the top's upward flux and, DIRECT, the beam at both
template <bool DIRECT, typename Sink>
__device__ __forceinline__ void one_sweep_exit(Sink &sink, int L, OneSweep const &s, double alb_dir, double alb_dif,
                                               double scale, double tsi)
{
    double up_s, dn_s;                                                          // :318-329 at the surface
    level_flux(s.dir, s.dif, s.Ru, alb_dir, alb_dif, up_s, dn_s);
    put_level(sink, 0, s.Rd + s.Tu*up_s, 1., scale, tsi);
    put_level(sink, L, up_s, dn_s, scale, tsi);
    if constexpr (DIRECT)
    {
        put_direct(sink, 0, 1., scale, tsi);
        put_direct(sink, L, s.dir, scale, tsi);
    }
}

// a night row or angle (uniform per workgroup): +0.0 in this workgroup's nrows partial sums of the slot and -- a
// GrtDirectArgs is joined -- in its drows of the direct beam's; nothing is solved
template <typename... Joins>
__device__ __forceinline__ void night_fill(GrtSwArgs const &a, int slot, int nrows, int drows, Joins const &...joins)
{
    for (int r = threadIdx.x; r < nrows; r += kSolverBlock)
    {
        a.partials[((uint64_t)slot*nrows + r)*gridDim.x + blockIdx.x] = 0.;
    }
    if constexpr (has<GrtDirectArgs, Joins...>)
    {
        double *dp = pick<GrtDirectArgs>(joins...).partials;
        for (int r = threadIdx.x; r < drows; r += kSolverBlock)
        {
            dp[((uint64_t)slot*drows + r)*gridDim.x + blockIdx.x] = 0.;
        }
    }
}

// the cosine of the zenith angle of a grid row: the column's, or -- zenith instances -- the row's angle's
template <typename... Joins>
__device__ __forceinline__ double row_mu(GrtSwArgs const &a, SolverRow const &row, Joins const &...joins)
{
    if constexpr (has<GrtZenithArgs, Joins...>)
    {
        return pick<GrtZenithArgs>(joins...).mu[row.sun];
    }
    else
    {
        return a.mu_dir[row.col];
    }
}

// the cosine the direct beam has in layer j of the row whose own cosine is mu_row: that cosine, or -- a GrtZenithSlantArgs
// is joined -- the layer's own of sun angle `sun` (c zeniths + k) of L layers.  The index is made of blockIdx, the layer
// counter and kernel arguments alone: a scalar load, no vector register
template <typename... Joins>
__device__ __forceinline__ double layer_mu(double mu_row, int sun, int L, int j, Joins const &...joins)
{
    if constexpr (has<GrtZenithSlantArgs, Joins...>)
    {
        return pick<GrtZenithSlantArgs>(joins...).mu_layer[(uint64_t)sun*(uint64_t)L + (uint64_t)j];
    }
    else
    {
        return mu_row;
    }
}

// the direct-beam albedo of column col at grid point ii: the column's row, or -- a GrtZenithSurfaceArgs is joined -- the
// pair of sun angle `sun` (c zeniths + k) at the point's entry, evaluated as spread_surface_kernel evaluates it (multiply,
// then add: the double that kernel would write into the angle's row)
template <typename... Joins>
__device__ __forceinline__ double row_alb_dir(GrtSwArgs const &a, int col, int sun, uint64_t ii, Joins const &...joins)
{
    if constexpr (has<GrtZenithSurfaceArgs, Joins...>)
    {
        GrtZenithSurfaceArgs const zs = pick<GrtZenithSurfaceArgs>(joins...);
        double const *mb = zs.tables + ((uint64_t)sun*(uint64_t)zs.num_entries + (uint64_t)zs.entry[ii])*2;
        double const w = a.w0 + ii*a.dw;
        return mb[0]*w + mb[1];
    }
    else
    {
        return a.alb_dir[(uint64_t)col*a.alb_stride + ii];
    }
}

// OUT fused (GRT_OUT_ROWS and after): the clear-sky tail in one kernel -- tau, omega, g of a layer are formed in registers
// from tau_gas and the Rayleigh optical depth (LayerOptics: identical values), the first sweep's reflectances are parked
// in a scratch block instead of the output rows, nothing spectral is written and the six integrated output rows leave as
// per-block trapezoid partial sums (LevelSink).
// GRT_OUT_LEVELS, GRT_OUT_LEVEL_BINS: the reference's two sweeps always (shortwave.c:280-329) -- the first parks the
// downward-beam reflectances of EVERY level in rows 0 .. 2 V - 1 of the park block, the second produces up and down at
// every level and the sink sums each across the wave at once (as lw_kernel's), per wavenumber bin with the pack's
// GrtBandArgs.  GRT_OUT_ROWS_POINTS: the six rows also leave at every point, unweighted (LevelSink).
// Joins (fused forms): clouds (a GrtCloudArgs, or the draws of a GrtSubcolumnArgs), the aerosol object or both join per
// layer (LayerOptics), as in lw_kernel; the one-sweep and two-sweep rule is OUT's own.  props_of is the only place that reads
// the joined tables, and the fused forms call it in their first (or only) sweep: the two-sweep forms' second sweep reads
// the parked properties.
template <GrtSolverOutput OUT, typename... Joins>
__global__ __launch_bounds__(kSolverBlock) void sw_kernel(GrtSwArgs a, Joins... joins)
{
    uint64_t const i = (uint64_t)blockIdx.x*kSolverBlock + threadIdx.x;
    constexpr bool FUSED = grt_out_fused(OUT), PROFILE = grt_out_levels(OUT), SPECTRAL = OUT == GRT_OUT_ROWS_POINTS;
    constexpr bool DIRECT = has<GrtDirectArgs, Joins...>;
    static_assert(has<GrtBandArgs, Joins...> == (OUT == GRT_OUT_LEVEL_BINS), "bins go with GRT_OUT_LEVEL_BINS alone");
    static_assert(!DIRECT || OUT == GRT_OUT_ROWS || OUT == GRT_OUT_LEVELS, "the direct beam leaves the six-row and level forms");
    static_assert(!has<GrtZenithSurfaceArgs, Joins...> || has<GrtZenithArgs, Joins...>,
                  "every angle's own direct albedo goes with the sun angles");
    static_assert(!has<GrtZenithSlantArgs, Joins...> || (has<GrtZenithArgs, Joins...> && DIRECT && FUSED),
                  "a sun cosine per layer goes with the sun angles and the direct beam, fused forms");
    constexpr bool RESPONSES = has<GrtResponseArgs, Joins...>;
    static_assert(!RESPONSES || (OUT == GRT_OUT_LEVELS && DIRECT), "the response rows leave the level form, the direct beam with them");
    SolverRow const row = solver_row(a.ncol, joins...);
    int const col = row.col;
    bool const live = i < a.nw;
    if (!FUSED && !live)
    {
        return;
    }
    uint64_t const ii = live ? i : a.nw - 1;      // (fused form: idle lanes of the last block follow along, weight 0)
    int const V = a.num_levels;
    int const L = V - 1;
    uint64_t const nw = a.nw;
    double const *tau = a.tau + (uint64_t)col*a.optics_stride + ii;
    double const *omega = FUSED ? nullptr : a.omega + (uint64_t)col*a.optics_stride + ii;
    double const *g = FUSED ? nullptr : a.g + (uint64_t)col*a.optics_stride + ii;
    double const mu_dir = row_mu(a, row, joins...);
    double const mu_dif = a.mu_dif;
    if constexpr (has<GrtZenithArgs, Joins...>)
    {
        if (!(mu_dir > 0.))
        {
            night_fill(a, row.slot, PROFILE ? 2*a.num_levels : 6, PROFILE ? a.num_levels : 3, joins...);
            return;
        }
    }
    // where the first sweep parks R_dir_downward / R_dif_downward of every level
    uint64_t const park_rows = 2*(uint64_t)V + 5*(uint64_t)L;
    double *fu = FUSED ? a.park + ((uint64_t)row.park*park_rows + 0)*nw + ii : a.flux_up + (uint64_t)col*a.flux_stride + ii;
    double *fd = FUSED ? a.park + ((uint64_t)row.park*park_rows + V)*nw + ii : a.flux_down + (uint64_t)col*a.flux_stride + ii;
    // fused form: the five properties of layer j, rows 2 V + 5 j .. + 4 of the column's block -- written by the first
    // sweep, read by the second (the same values as working them out again: two Eddington solutions, 6 exp and ~13
    // divisions a layer, which is what this kernel's time is made of)
    double *pp = FUSED ? a.park + ((uint64_t)row.park*park_rows + 2*(uint64_t)V)*nw + ii : nullptr;
    int const user = a.user_level;
    LevelSink<FUSED, PROFILE, SPECTRAL, has<GrtBandArgs, Joins...>, DIRECT, RESPONSES> sink(
        a, row.slot, i, live, pick<GrtBandArgs>(joins...), pick<GrtDirectArgs>(joins...), pick<GrtResponseArgs>(joins...));
    LayerOptics<FUSED, has_clouds<Joins...>, has<GrtAerosolArgs, Joins...>> const optics(
        a, pick_clouds(joins...), col, row.tab, ii, pick<GrtAerosolArgs>(joins...));                    // (fused forms)

    auto props_of = [&](int j) -> LayerProps
    {
        if (FUSED)
        {
            double t, om, gg;
            optics.at(j, t, om, gg);
            // (a sun cosine per layer: named in the slant instances alone, so that every other instance's closure, and with
            // it its code, stays what it was)
            if constexpr (has<GrtZenithSlantArgs, Joins...>)
            {
                return layer_props(om, gg, t, layer_mu(mu_dir, row.sun, L, j, joins...), mu_dif);
            }
            else
            {
                return layer_props(om, gg, t, mu_dir, mu_dif);
            }
        }
        uint64_t const o = (uint64_t)j*nw;
        return layer_props(omega[o], g[o], tau[o], mu_dir, mu_dif);
    };

    if (FUSED && !PROFILE && GRT_SW_ONE_SWEEP(user, L, a.one_sweep))
    {
        OneSweep sweep;
        for (int j = 0; j < L; ++j)
        {
            sweep.step(props_of(j));
        }
        double const scale = a.solar[ii]*mu_dir;
        double const tsi = a.tsi[col];
        one_sweep_exit<DIRECT>(sink, L, sweep, row_alb_dir(a, col, row.sun, ii, joins...),
                               a.alb_dif[(uint64_t)col*a.alb_stride + ii], scale, tsi);
        sink.finish(a);
        return;
    }

    // sweep 1: shortwave.c:280-294
    double Rdir_dn = row_alb_dir(a, col, row.sun, ii, joins...);
    double Rdif_dn = a.alb_dif[(uint64_t)col*a.alb_stride + ii];
    // Fused form: only three levels' fluxes leave the kernel (top, surface, the user's), so the downward-beam reflectances
    // of the other levels are never needed again -- the surface's are the albedos, the top's and the user level's stay in
    // registers, and nothing of this sweep but the layer properties is parked (round 4: 2 V fewer rows written and read
    // back per column; the same doubles reach the same expressions, so the fluxes are the same to the last bit).
    double const surf_rdir = Rdir_dn, surf_rdif = Rdif_dn;
    double user_rdir = Rdir_dn, user_rdif = Rdif_dn;        // (the user level is the surface, or set below)
    if (!FUSED || PROFILE)
    {
        fu[(uint64_t)L*nw] = Rdir_dn;
        fd[(uint64_t)L*nw] = Rdif_dn;
    }
    for (int j = L - 1; j >= 0; --j)
    {
        uint64_t const o = (uint64_t)j*nw;
        LayerProps const p = props_of(j);
        if (FUSED)
        {
            store_props(pp + (uint64_t)(5*j)*nw, nw, p);
        }
        sweep1_step(p, Rdir_dn, Rdif_dn);
        if (FUSED && !PROFILE)
        {
            user_rdir = j == user ? Rdir_dn : user_rdir;
            user_rdif = j == user ? Rdif_dn : user_rdif;
        }
        else
        {
            fu[o] = Rdir_dn;
            fd[o] = Rdif_dn;
        }
    }

    // sweep 2: shortwave.c:299-329 fused, then the scalings of :401-405 and :447-451
    double const scale = a.solar[ii]*mu_dir;
    double const tsi = a.tsi[col];
    Sweep2 s;
    put_level(sink, 0, s.dir*(FUSED ? Rdir_dn : fu[0]), s.dir, scale, tsi);   // R[0] = dir_beam*R_dir_downward[0], T[0]
    if constexpr (DIRECT)
    {
        put_direct(sink, 0, s.dir, scale, tsi);
    }
    for (int lev = 1; lev < V; ++lev)
    {
        sweep2_step(s, FUSED ? load_props(pp + (uint64_t)(5*(lev - 1))*nw, nw) : props_of(lev - 1), lev);
        if (!sink.wanted(lev))
        {
            continue;
        }
        uint64_t const ol = (uint64_t)lev*nw;
        double const rdir = FUSED && !PROFILE ? (lev == L ? surf_rdir : user_rdir) : fu[ol];   // R_dir_downward[lev] of sweep 1
        double const rdif = FUSED && !PROFILE ? (lev == L ? surf_rdif : user_rdif) : fd[ol];   // R_dif_downward[lev]
        double up, dn;
        level_flux(s.dir, s.dif, s.Rup, rdir, rdif, up, dn);
        put_level(sink, lev, up, dn, scale, tsi);
        if constexpr (DIRECT)
        {
            put_direct(sink, lev, s.dir, scale, tsi);
        }
    }
    sink.finish(a);
}

// ---- the shortwave of a correlated-k model on its g-points (grt_launch_ck_sw; GrtCkSolveArgs, grt_kernels.h) ----
// One thread per (column, bin, class), the class fastest: every read of a layer's class sums and every store of a level
// is coalesced.  The g-point's gas optical depth of a layer is the class mean sum/W, its Rayleigh optical depth the layer's
// air column times the class sum of the cross-section, over W; clear_sky_combine and layer_props on them, then the
// reference's two sweeps (sw_kernel's materialised form): the first parks the two downward-beam reflectances of every level
// in the output arrays, the second consumes each pair and overwrites it with the level's fluxes.  The scale is the class
// SUM of the solar curve times mu_dir, then tsi, by put_level into a PairSink: W m-2 per class.  An empty class (W = 0) and a
// night column (mu_dir <= 0) leave +0.0 and solve nothing.
struct PairSink        // (put_level's sink over two arrays: level lev's pair at fu[lev stride], fd[lev stride])
{
    double *fu, *fd;
    uint64_t stride;
    __device__ __forceinline__ void put(int lev, bool down, double x) { (down ? fd : fu)[(uint64_t)lev*stride] = x; }
};

__global__ __launch_bounds__(kSolverBlock) void ck_sw_kernel(GrtCkSolveArgs a)
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
    double const *S = a.source_sum + col*(uint64_t)4*per_col + at;           // source row r at S[r per_col]
    double const *nl = a.n_layer + col*(uint64_t)L;
    double *fu = a.flux_up + col*(uint64_t)V*per_col + at, *fd = a.flux_down + col*(uint64_t)V*per_col + at;
    double const mu_dir = a.mu_dir[col], mu_dif = a.mu_dif;
    if (!(W > 0.) || !(mu_dir > 0.))
    {
        for (int lev = 0; lev < V; ++lev)
        {
            fu[(uint64_t)lev*per_col] = 0.;
            fd[(uint64_t)lev*per_col] = 0.;
        }
        return;
    }
    double const ray = S[0];

    auto props_of = [&](int j) -> LayerProps
    {
        double const tg = T[(uint64_t)j*per_col]/W, tr = (nl[j]*ray)/W;
        double tt, om, gg;
        clear_sky_combine(tg, tr, tt, om, gg);
        return layer_props(om, gg, tt, mu_dir, mu_dif);
    };

    // sweep 1: shortwave.c:280-294
    double Rdir_dn = S[2*per_col]/W;
    double Rdif_dn = S[3*per_col]/W;
    fu[(uint64_t)L*per_col] = Rdir_dn;
    fd[(uint64_t)L*per_col] = Rdif_dn;
    for (int j = L - 1; j >= 0; --j)
    {
        sweep1_step(props_of(j), Rdir_dn, Rdif_dn);
        fu[(uint64_t)j*per_col] = Rdir_dn;
        fd[(uint64_t)j*per_col] = Rdif_dn;
    }

    // sweep 2: shortwave.c:299-329, then the scalings of :401-405 and :447-451
    double const scale = S[per_col]*mu_dir;
    double const tsi = a.tsi[col];
    PairSink sink = {fu, fd, per_col};
    Sweep2 s;
    put_level(sink, 0, s.dir*Rdir_dn, s.dir, scale, tsi);      // R[0] = dir_beam*R_dir_downward[0], T[0]
    for (int lev = 1; lev < V; ++lev)
    {
        sweep2_step(s, props_of(lev - 1), lev);
        double up, dn;
        level_flux(s.dir, s.dif, s.Rup, fu[(uint64_t)lev*per_col], fd[(uint64_t)lev*per_col], up, dn);
        put_level(sink, lev, up, dn, scale, tsi);
    }
}

// ---- several sun angles per column on one walk through the layers (grt_launch_sw_zeniths) ----
// Of sw_kernel<GRT_OUT_ROWS>'s one sweep, a layer's optics (tau_gas, continua, Rayleigh and what joins them: LayerOptics),
// its delta-scaling, its diffuse Eddington solution with k and exp(+-t k), and C, Ru, Tu of the sweep depend on the optics
// alone; the angle's own are the direct-beam solution, dir, dif, Rd and the scale at the surface: OneSweep::step's lines,
// split by hand into the two (a member per part costs this kernel scalar spills), then one_sweep_exit.  Grid row y is a column,
// a cloud draw of it (Joins holds a GrtSubcolumnArgs: draws first .. first + count - 1, the chunks of a draw next to each
// other) and a chunk of ZN consecutive angles: the thread does the shared part of a layer once and the angle's part ZN
// times, each in sw_kernel's expressions and order on the same doubles (exp(+-t k) is a function of its argument, whichever
// call evaluates it first), so every angle's partial sums are the zenith instance's of sw_kernel<GRT_OUT_ROWS> with the
// same joins, bit for bit, at its slot (c zeniths + k) subcolumns + s.  Angles past the column's last and night angles
// (mu <= 0) are skipped by flags that are uniform per workgroup; a night angle's slot gets +0.0.  Joins: nothing, a
// GrtAerosolArgs, a GrtSubcolumnArgs, or a GrtAerosolArgs behind a GrtSubcolumnArgs; behind any of the four a
// GrtZenithSurfaceArgs (the angle's own direct albedo at the surface, in place of the column's), a GrtDirectArgs (the angle's
// direct beam at the top and the surface -- 1 and dir[u], scaled as the rows beside them -- through the sink's three more
// rows) or both: sw_kernel's zenith instances with those joins, bit for bit.  With a GrtZenithSlantArgs ahead of the
// GrtDirectArgs the direct-beam solution of angle u in layer j takes layer_mu's cosine in place of mu[u]; the scale stays
// solar x mu[u].
template <int ZN, typename... Joins>
__global__ __launch_bounds__(kSolverBlock) void sw_zenith_kernel(GrtSwArgs a, GrtZenithArgs zn, Joins... joins)
{
    uint64_t const i = (uint64_t)blockIdx.x*kSolverBlock + threadIdx.x;
    bool const live = i < a.nw;
    uint64_t const ii = live ? i : a.nw - 1;      // (idle lanes of the last block follow along, weight 0)
    int const Z = zn.zeniths, chunks = (Z + ZN - 1)/ZN;
    // (solver_row's subcolumn rule on y / chunks, by hand: through solver_row the subcolumn instances gain instructions)
    int const y = blockIdx.y;
    int const cd = y/chunks;                      // (column, or -- subcolumns -- column and draw)
    int const k0 = (y - cd*chunks)*ZN;
    int col = cd, tab = cd, S = 1, draw = 0;
    if constexpr (has<GrtSubcolumnArgs, Joins...>)
    {
        GrtSubcolumnArgs const sc = pick<GrtSubcolumnArgs>(joins...);
        col = cd/sc.count;
        draw = sc.first + (cd - col*sc.count);
        tab = draw*a.ncol + col;
        S = sc.subcolumns;
    }
    int const L = a.num_levels - 1;
    double const mu_dif = a.mu_dif;
    double mu[ZN];
    bool day[ZN];
    bool any = false;
#pragma unroll
    for (int u = 0; u < ZN; ++u)
    {
        mu[u] = k0 + u < Z ? zn.mu[(uint64_t)col*Z + k0 + u] : 0.;
        day[u] = mu[u] > 0.;
        any = any || day[u];
    }
    double dir[ZN], dif[ZN], Rd[ZN];
#pragma unroll
    for (int u = 0; u < ZN; ++u)
    {
        dir[u] = 1.; dif[u] = 0.; Rd[u] = 0.;
    }
    double Ru = 0., Tu = 1.;
    if (any)
    {
        LayerOptics<true, has_clouds<Joins...>, has<GrtAerosolArgs, Joins...>> const optics(
            a, pick_clouds(joins...), col, tab, ii, pick<GrtAerosolArgs>(joins...));
        for (int j = 0; j < L; ++j)
        {
            double t, om, gg, os, gs, ts;
            optics.at(j, t, om, gg);
            delta_scaling(om, gg, t, os, gs, ts);
            ExpKt shared = {0., 0., 0., false};
            LayerRT const s = eddington<false>(os, ts, mu_dif, gs, shared);
            // (OneSweep::step's lines from here on, its C, Tu, Ru once and its Rd, dif, dir per angle: a copy, see above)
            double const C = 1./(1. - s.R*Ru);
#pragma unroll
            for (int u = 0; u < ZN; ++u)
            {
                if (day[u])
                {
                    ExpKt mine = shared;
                    // (the angle's cosine in this layer: asked for where it is used -- the kernel holds every scalar register
                    // there is, and a cosine asked for earlier in the layer displaces others for longer)
                    LayerRT const d = eddington<true>(os, ts, layer_mu(mu[u], col*Z + k0 + u, L, j, joins...), gs, mine);
                    Rd[u] = Rd[u] + Tu*((dir[u]*d.R + dif[u]*s.R)*C);
                    dif[u] = (dir[u]*d.R*Ru + dif[u])*s.T*C + dir[u]*(d.T - d.Tpure);      // shortwave.c:312-316
                    dir[u] *= d.Tpure;
                }
            }
            Tu = Tu*(s.T*C);
            Ru = s.R + s.T*s.T*Ru*C;                                                         // :299-306
        }
    }
    constexpr bool DIRECT = has<GrtDirectArgs, Joins...>, SURFACE = has<GrtZenithSurfaceArgs, Joins...>;
    static_assert(!has<GrtZenithSlantArgs, Joins...> || DIRECT, "a sun cosine per layer goes with the direct beam");
    // (the column's direct albedo, once; with a GrtZenithSurfaceArgs every angle reads its own below)
    double const alb_col = SURFACE ? 0. : a.alb_dir[(uint64_t)col*a.alb_stride + ii];
    double const alb_dif = a.alb_dif[(uint64_t)col*a.alb_stride + ii];
    double const solar = a.solar[ii], tsi = a.tsi[col];
#pragma unroll
    for (int u = 0; u < ZN; ++u)
    {
        if (k0 + u >= Z)
        {
            continue;
        }
        int const sun = col*Z + k0 + u, slot = sun*S + draw;
        if (!day[u])
        {
            night_fill(a, slot, 6, 3, joins...);
            continue;
        }
        // (six rows, and -- a GrtDirectArgs is joined -- the angle's direct beam at the top and the surface beside them)
        LevelSink<true, false, false, false, DIRECT> sink(a, slot, i, live, GrtBandArgs{0, 0, nullptr, 0},
                                                          pick<GrtDirectArgs>(joins...));
        one_sweep_exit<DIRECT>(sink, L, OneSweep{dir[u], dif[u], Ru, Rd[u], Tu},
                               SURFACE ? row_alb_dir(a, col, sun, ii, joins...) : alb_col, alb_dif, solar*mu[u], tsi);
        __syncthreads();                            // (block_partials' LDS is the angle before's: every wave has read it)
        sink.finish(a);
    }
}

// ---- several surface tiles per column on one walk through the layers (grt_launch_sw_tiles; GrtTileArgs, grt_kernels.h) ----
// Of sw_kernel<GRT_OUT_ROWS>, only level_flux at a level and Rd + Tu x (the upward flux at the surface) read the albedo in
// the one sweep; of its two sweeps, only sweep1_step, through the pair (R_dir_downward, R_dif_downward) it carries up from
// the albedos.  Grid row y is the six-row instance's (a column, or a column and cloud draw), blockIdx.z a chunk of TN
// consecutive tiles: a TileChunk (optics_dev.h).  One sweep (GRT_SW_ONE_SWEEP): OneSweep once, one_sweep_exit per tile.  Two
// sweeps: the layer properties are formed and parked once (sw_kernel's fused layout, at park row z gridDim.y + y),
// sweep1_step runs per tile on the tile's pair, the user level's pair kept per tile; the second sweep runs once, its
// beams and R_dif_upward kept where it passes the user level; then level_flux per tile at the top, the user level and
// the surface.  Every tile's six rows leave through a LevelSink at the tile's slot: sw_kernel's doubles through
// sw_kernel's sums.  Tiles past the column's last are skipped by a flag that is uniform per workgroup.
template <int TN, typename... Joins>
__global__ __launch_bounds__(kSolverBlock) void sw_tile_kernel(GrtSwArgs a, GrtTileArgs tl, Joins... joins)
{
    uint64_t const i = (uint64_t)blockIdx.x*kSolverBlock + threadIdx.x;
    SolverRow const row = solver_row(a.ncol, joins...);
    int const col = row.col;
    bool const live = i < a.nw;
    uint64_t const ii = live ? i : a.nw - 1;      // (idle lanes of the last block follow along, weight 0)
    int const V = a.num_levels, L = V - 1, user = a.user_level;
    TileChunk<TN> const chunk(tl, row, joins...);
    int const T = chunk.T, k0 = chunk.k0, S = chunk.S, draw = chunk.draw;
    uint64_t const nw = a.nw;
    double const mu_dir = a.mu_dir[col], mu_dif = a.mu_dif;
    LayerOptics<true, has_clouds<Joins...>, has<GrtAerosolArgs, Joins...>> const optics(
        a, pick_clouds(joins...), col, row.tab, ii, pick<GrtAerosolArgs>(joins...));
    auto props_of = [&](int j) -> LayerProps
    {
        double t, om, gg;
        optics.at(j, t, om, gg);
        return layer_props(om, gg, t, mu_dir, mu_dif);
    };
    // the tiles' albedos: their own rows, or -- no rows -- the instance's for every tile
    double alb_dir[TN], alb_dif[TN];
#pragma unroll
    for (int u = 0; u < TN; ++u)
    {
        alb_dir[u] = alb_dif[u] = 0.;
        if (chunk.live(u))
        {
            uint64_t const at = ((uint64_t)col*T + k0 + u)*nw + ii;
            alb_dir[u] = tl.rows != nullptr ? tl.rows[at] : a.alb_dir[(uint64_t)col*a.alb_stride + ii];
            alb_dif[u] = tl.rows != nullptr ? (tl.rows_dif != nullptr ? tl.rows_dif[at] : tl.rows[at]) :
                                              a.alb_dif[(uint64_t)col*a.alb_stride + ii];
        }
    }
    double const scale = a.solar[ii]*mu_dir;
    double const tsi = a.tsi[col];

    if (GRT_SW_ONE_SWEEP(user, L, a.one_sweep))
    {
        OneSweep sweep;
        for (int j = 0; j < L; ++j)
        {
            sweep.step(props_of(j));
        }
#pragma unroll
        for (int u = 0; u < TN; ++u)
        {
            if (!chunk.live(u))
            {
                continue;
            }
            LevelSink<true, false> sink(a, (col*T + k0 + u)*S + draw, i, live);       // (TileChunk's slot rule: a copy)
            one_sweep_exit<false>(sink, L, sweep, alb_dir[u], alb_dif[u], scale, tsi);
            __syncthreads();                        // (block_partials' LDS is the tile before's: every wave has read it)
            sink.finish(a);
        }
        return;
    }

    // sweep 1 (shortwave.c:280-294): the layer properties once, parked; the downward-beam reflectances per tile
    uint64_t const park_rows = 2*(uint64_t)V + 5*(uint64_t)L;
    uint64_t const park_row = (uint64_t)blockIdx.z*gridDim.y + (uint64_t)row.park;
    double *pp = a.park + (park_row*park_rows + 2*(uint64_t)V)*nw + ii;
    double Rdir_dn[TN], Rdif_dn[TN], user_rdir[TN], user_rdif[TN];
#pragma unroll
    for (int u = 0; u < TN; ++u)
    {
        Rdir_dn[u] = user_rdir[u] = alb_dir[u];             // (the user level is the surface, or set below)
        Rdif_dn[u] = user_rdif[u] = alb_dif[u];
    }
    for (int j = L - 1; j >= 0; --j)
    {
        LayerProps const p = props_of(j);
        store_props(pp + (uint64_t)(5*j)*nw, nw, p);
#pragma unroll
        for (int u = 0; u < TN; ++u)
        {
            if (chunk.live(u))
            {
                sweep1_step(p, Rdir_dn[u], Rdif_dn[u]);
                user_rdir[u] = j == user ? Rdir_dn[u] : user_rdir[u];
                user_rdif[u] = j == user ? Rdif_dn[u] : user_rdif[u];
            }
        }
    }
    // sweep 2 (shortwave.c:299-316), once: what reaches the user level, then what reaches the surface
    Sweep2 s, at_user;
    for (int lev = 1; lev < V; ++lev)
    {
        sweep2_step(s, load_props(pp + (uint64_t)(5*(lev - 1))*nw, nw), lev);
        if (lev == user)
        {
            at_user = s;
        }
    }
#pragma unroll
    for (int u = 0; u < TN; ++u)
    {
        if (!chunk.live(u))
        {
            continue;
        }
        LevelSink<true, false> sink(a, (col*T + k0 + u)*S + draw, i, live);           // (TileChunk's slot rule: a copy)
        put_level(sink, 0, 1.*Rdir_dn[u], 1., scale, tsi);     // R[0] = dir_beam*R_dir_downward[0], T[0]
        double up, dn;
        if (user > 0 && user < L)
        {
            level_flux(at_user.dir, at_user.dif, at_user.Rup, user_rdir[u], user_rdif[u], up, dn);
            put_level(sink, user, up, dn, scale, tsi);
        }
        level_flux(s.dir, s.dif, s.Rup, alb_dir[u], alb_dif[u], up, dn);             // :318-329 at the surface
        put_level(sink, L, up, dn, scale, tsi);
        __syncthreads();                            // (block_partials' LDS is the tile before's: every wave has read it)
        sink.finish(a);
    }
}

// ---- spectral form of few columns: the layer properties first, by one thread per (layer, wavenumber) ----
// One column of the 1 cm-1 shortwave band is 50 000 threads for sw_kernel<GRT_OUT_CHAINS>: not one wave per SIMD, each working
// through 120 layer steps of two delta-Eddington solutions (six exp and a dozen divisions) one after the other.  The
// solutions of different layers do not depend on each other; only the adding sweeps do, and they are a few operations
// per layer.  So: sw_props_kernel fills props[col][5 j + k][nw] (k: Rdir, Tdir, Tpure, Rdif, Tdif -- the park layout of
// the fused form) with layer_props() of every (layer, wavenumber), and sw_sweeps_kernel runs the two sweeps of
// sw_kernel<GRT_OUT_CHAINS> -- the same expressions in the same order on the same doubles, so the fluxes are the same to the last
// bit -- reading six layers' properties at a time ahead of the dependent chain.
constexpr int kPropsBlock = 256;
constexpr int kSweepBlock = 64;
constexpr int kSweepChunk = 6;

__global__ __launch_bounds__(kPropsBlock) void sw_props_kernel(GrtSwArgs a)
{
    int const col = blockIdx.y;
    int const L = a.num_levels - 1;
    uint64_t const nw = a.nw;
    uint64_t const o = (uint64_t)blockIdx.x*kPropsBlock + threadIdx.x;       // j nw + i: the optics arrays' own index
    if (o >= (uint64_t)L*nw)
    {
        return;
    }
    uint64_t const j = o/nw;
    uint64_t const i = o - j*nw;
    uint64_t const at = (uint64_t)col*a.optics_stride + o;
    store_props(a.layer_props + ((uint64_t)col*5*(uint64_t)L + 5*j)*nw + i, nw,
                layer_props(a.omega[at], a.g[at], a.tau[at], a.mu_dir[col], a.mu_dif));
}

__global__ __launch_bounds__(kSweepBlock) void sw_sweeps_kernel(GrtSwArgs a)
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
    double const mu_dir = a.mu_dir[col];
    double const *pp = a.layer_props + (uint64_t)col*5*(uint64_t)L*nw + i;
    double *fu = a.flux_up + (uint64_t)col*a.flux_stride + i;
    double *fd = a.flux_down + (uint64_t)col*a.flux_stride + i;
    LevelSink<false, false> sink(a, col, i, true);
    auto load = [&](int j) -> LayerProps
    {
        return load_props(pp + (uint64_t)(5*j)*nw, nw);
    };

    // sweep 1: shortwave.c:280-294 (as in sw_kernel<GRT_OUT_CHAINS>: the downward-beam reflectances are parked in the output rows)
    double Rdir_dn = a.alb_dir[(uint64_t)col*a.alb_stride + i];
    double Rdif_dn = a.alb_dif[(uint64_t)col*a.alb_stride + i];
    fu[(uint64_t)L*nw] = Rdir_dn;
    fd[(uint64_t)L*nw] = Rdif_dn;
    // (the next six layers' properties are asked for before the chain works through the six it has: the loads' latency
    // is as long as the six steps)
    LayerProps pr[kSweepChunk], nx[kSweepChunk];
#pragma unroll
    for (int u = 0; u < kSweepChunk; ++u)
    {
        pr[u] = load(L - 1 - u >= 0 ? L - 1 - u : 0);
    }
    for (int jb = L - 1; jb >= 0; jb -= kSweepChunk)
    {
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            int const j = jb - kSweepChunk - u;
            nx[u] = load(j >= 0 ? j : 0);
        }
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            int const j = jb - u;
            if (j >= 0)
            {
                uint64_t const o = (uint64_t)j*nw;
                sweep1_step(pr[u], Rdir_dn, Rdif_dn);
                fu[o] = Rdir_dn;
                fd[o] = Rdif_dn;
            }
        }
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            pr[u] = nx[u];
        }
    }

    // sweep 2: shortwave.c:299-329 fused, then the scalings of :401-405 and :447-451
    double const scale = a.solar[i]*mu_dir;
    double const tsi = a.tsi[col];
    Sweep2 s;
    put_level(sink, 0, s.dir*Rdir_dn, s.dir, scale, tsi);   // R[0] = dir_beam*R_dir_downward[0] (the value sweep 1 has
                                                             // just stored in fu[0]), T[0] = dir_beam
    double rd[kSweepChunk], rf[kSweepChunk], nrd[kSweepChunk], nrf[kSweepChunk];
#pragma unroll
    for (int u = 0; u < kSweepChunk; ++u)
    {
        int const lev = 1 + u < V ? 1 + u : V - 1;
        pr[u] = load(lev - 1);
        rd[u] = fu[(uint64_t)lev*nw];              // R_dir_downward[lev] of sweep 1
        rf[u] = fd[(uint64_t)lev*nw];              // R_dif_downward[lev]
    }
    for (int lb = 1; lb < V; lb += kSweepChunk)
    {
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            int const lev = lb + kSweepChunk + u < V ? lb + kSweepChunk + u : V - 1;
            nx[u] = load(lev - 1);
            nrd[u] = fu[(uint64_t)lev*nw];
            nrf[u] = fd[(uint64_t)lev*nw];
        }
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            int const lev = lb + u;
            if (lev < V)
            {
                sweep2_step(s, pr[u], lev);        // layer lev-1
                double up, dn;
                level_flux(s.dir, s.dif, s.Rup, rd[u], rf[u], up, dn);
                put_level(sink, lev, up, dn, scale, tsi);
            }
        }
#pragma unroll
        for (int u = 0; u < kSweepChunk; ++u)
        {
            pr[u] = nx[u];
            rd[u] = nrd[u];
            rf[u] = nrf[u];
        }
    }
}

// ---- the direct beam of the materialised form (grt_launch_sw_direct_beam) ----
// One thread per (wavenumber, column) walks the layers of the tau, omega, g a pass left on the grid: the delta-scaling and
// T_pure of layer_props()'s direct-beam solution (the same device functions on the same doubles: the solver's own dir),
// the running product from the top, scaled as put_direct scales it.
constexpr int kDirectBlock = 128;

__global__ __launch_bounds__(kDirectBlock) void sw_direct_beam_kernel(GrtSwArgs a, double *direct)
{
    uint64_t const i = (uint64_t)blockIdx.x*kDirectBlock + threadIdx.x;
    int const col = blockIdx.y;
    if (i >= a.nw)
    {
        return;
    }
    int const V = a.num_levels;
    uint64_t const nw = a.nw;
    double const *tau = a.tau + (uint64_t)col*a.optics_stride + i;
    double const *omega = a.omega + (uint64_t)col*a.optics_stride + i;
    double const *g = a.g + (uint64_t)col*a.optics_stride + i;
    double *out = direct + (uint64_t)col*(uint64_t)V*nw + i;
    double const mu = a.mu_dir[col];
    double const scale = a.solar[i]*mu;
    double const tsi = a.tsi[col];
    double dir = 1.;
    out[0] = tsi*(dir*scale);
    for (int lev = 1; lev < V; ++lev)
    {
        uint64_t const o = (uint64_t)(lev - 1)*nw;
        double gs, os, ts;
        delta_scaling(omega[o], g[o], tau[o], os, gs, ts);
        dir *= pure_transmission(os, ts, mu, eddington_gammas(os, gs, mu), [](double, double, double, double) {});
        out[(uint64_t)lev*nw] = tsi*(dir*scale);
    }
}

// rows [n][3] of levels [n][V]: TOA, surface, the user level (+0.0 without one)
__global__ __launch_bounds__(64) void direct_rows_kernel(int n, int V, int user, double const *levels, double *rows)
{
    int const k = blockIdx.x*64 + threadIdx.x;
    if (k < n)
    {
        double const *lv = levels + (uint64_t)k*V;
        rows[3*(uint64_t)k] = lv[0];
        rows[3*(uint64_t)k + 1] = lv[V - 1];
        rows[3*(uint64_t)k + 2] = user >= 0 ? lv[user] : 0.;
    }
}

// the one launch site of sw_kernel: the instance of OUT and of the joined arguments' types, on the instance's grid and LDS
template <GrtSolverOutput OUT, typename... Joins>
int launch(hipStream_t s, GrtSolverInstance const &in, GrtSwArgs const &a, Joins const &...joins)
{
    dim3 const grid(grt_solver_blocks(a.nw), (unsigned)grt_solver_grid_rows(&in, a.ncol), 1);
    hipLaunchKernelGGL((sw_kernel<OUT, Joins...>), grid, dim3(kSolverBlock), grt_solver_lds(&in, a.num_levels), s, a,
                       joins...);
    return (int)hipGetLastError();
}

// ... of sw_zenith_kernel: ZN angles per thread, grid row = (column, draw of the launch, chunk)
template <int ZN, typename... Joins>
int launch_zeniths(hipStream_t s, GrtSwArgs const &a, GrtZenithArgs const &z, int draws, Joins const &...joins)
{
    uint64_t const rows = (uint64_t)a.ncol*(uint64_t)draws*(uint64_t)((z.zeniths + ZN - 1)/ZN);
    if (rows > 65535u)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL((sw_zenith_kernel<ZN, Joins...>), dim3(grt_solver_blocks(a.nw), (unsigned)rows, 1),
                       dim3(kSolverBlock), 0, s, a, z, joins...);
    return (int)hipGetLastError();
}

// ... and of sw_tile_kernel: TN tiles per thread, the six-row instance's grid rows, the launch's chunks along z
template <int TN, typename... Joins>
int launch_tiles(hipStream_t s, GrtSwArgs const &a, GrtTileArgs const &t, int draws, Joins const &...joins)
{
    if (!grt_tile_args_ok(&t, TN) || (uint64_t)a.ncol*(uint64_t)draws > 65535u || t.chunk_count > 65535)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL((sw_tile_kernel<TN, Joins...>), dim3(grt_solver_blocks(a.nw), (unsigned)(a.ncol*draws), (unsigned)t.chunk_count),
                       dim3(kSolverBlock), 0, s, a, t, joins...);
    return (int)hipGetLastError();
}

} // namespace

extern "C" int grt_launch_ck_sw(void *stream, GrtCkSolveArgs const *a)
{
    if (!grt_ck_solve_args_ok(a) || a->n_layer == nullptr || a->mu_dir == nullptr || a->tsi == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    uint64_t const threads = (uint64_t)a->ncol*(uint64_t)a->num_bins*(uint64_t)a->num_classes;
    hipLaunchKernelGGL(ck_sw_kernel, dim3((unsigned)((threads + kSolverBlock - 1)/kSolverBlock)), dim3(kSolverBlock), 0,
                       (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_sw(void *stream, GrtSolverInstance const *in, GrtSwArgs const *a)
{
    uint64_t const cells = (uint64_t)(a->num_levels - 1)*a->nw;
    if (!grt_solver_instance_ok(*in, *a) || (grt_sw_parks(in, a) && a->park == nullptr) ||
        (in->out == GRT_OUT_LAYERS && (a->layer_props == nullptr || cells > 0xffffffffull*kPropsBlock ||
                                       a->omega == nullptr || a->g == nullptr)))
    {
        return (int)hipErrorInvalidValue;
    }
    hipStream_t const s = (hipStream_t)stream;
    if (in->out == GRT_OUT_LAYERS)
    {
        hipLaunchKernelGGL(sw_props_kernel, dim3((unsigned)((cells + kPropsBlock - 1)/kPropsBlock), a->ncol, 1),
                           dim3(kPropsBlock), 0, s, *a);
        hipLaunchKernelGGL(sw_sweeps_kernel, dim3((unsigned)((a->nw + kSweepBlock - 1)/kSweepBlock), a->ncol, 1),
                           dim3(kSweepBlock), 0, s, *a);
        return (int)hipGetLastError();
    }
    // every instance of sw_kernel there is (grt_sw_instance_exists)
    auto const site = [&](auto, auto out, auto const &...joins) { return launch<decltype(out)::value>(s, *in, *a, joins...); };
    return grt_launch_output<grt_sw_instance_exists>(in->out, grt_solver_joins(*in), site);
}

namespace {

// the joins of a shared-layer or a tile launch as an instance's (its GrtZenithArgs or GrtTileArgs is a parameter of its own)
GrtSolverInstance joined(GrtSubcolumnArgs const *sc, GrtAerosolArgs const *ae, GrtDirectArgs const *d = nullptr,
                         GrtZenithSurfaceArgs const *zs = nullptr, GrtZenithSlantArgs const *sl = nullptr)
{
    GrtSolverInstance in = {GRT_OUT_ROWS};
    in.subcolumns = sc;
    in.aerosols = ae;
    in.direct = d;
    in.zenith_surface = zs;
    in.zenith_slant = sl;
    return in;
}

} // namespace

extern "C" int grt_zenith_chunk(GrtSubcolumnArgs const *sc, GrtAerosolArgs const *ae, GrtDirectArgs const *d,
                                GrtZenithSurfaceArgs const *zs, GrtZenithSlantArgs const *sl)
{
    return grt_zenith_chunk_of(grt_join_set(grt_solver_joins(joined(sc, ae, d, zs, sl))));
}

extern "C" int grt_launch_sw_zeniths(void *stream, GrtSwArgs const *a, GrtZenithArgs const *z, GrtSubcolumnArgs const *sc,
                                     GrtAerosolArgs const *ae, GrtDirectArgs const *d, GrtZenithSurfaceArgs const *zs,
                                     GrtZenithSlantArgs const *sl)
{
    GrtSolverInstance const in = {GRT_OUT_ROWS};
    if (!grt_solver_instance_ok(in, *a) || z == nullptr || z->mu == nullptr || z->zeniths < 1 || !grt_sw_one_sweep(a) ||
        (sc != nullptr && !grt_subcolumn_args_ok(sc)) || (ae != nullptr && !grt_aerosol_args_ok(ae)) ||
        (d != nullptr && !grt_direct_args_ok(d)) || (zs != nullptr && !grt_zenith_surface_args_ok(zs)) ||
        (sl != nullptr && !grt_zenith_slant_args_ok(sl)))
    {
        return (int)hipErrorInvalidValue;
    }
    hipStream_t const s = (hipStream_t)stream;
    int const draws = sc != nullptr ? sc->count : 1;
    // every instance of sw_zenith_kernel there is (grt_sw_zenith_instance_exists: a cosine per layer needs the direct beam)
    auto const site = [&](auto set, auto const &...joins)
    { return launch_zeniths<grt_zenith_chunk_of(decltype(set)::value)>(s, *a, *z, draws, joins...); };
    return grt_launch_joined<grt_sw_zenith_instance_exists>(grt_solver_joins(joined(sc, ae, d, zs, sl)), site);
}

extern "C" int grt_launch_sw_tiles(void *stream, GrtSwArgs const *a, GrtTileArgs const *t, GrtSubcolumnArgs const *sc,
                                   GrtAerosolArgs const *ae)
{
    GrtSolverInstance const in = {GRT_OUT_ROWS};
    if (a == nullptr || t == nullptr || !grt_solver_instance_ok(in, *a) || (!grt_sw_one_sweep(a) && a->park == nullptr) ||
        (sc != nullptr && !grt_subcolumn_args_ok(sc)) || (ae != nullptr && !grt_aerosol_args_ok(ae)))
    {
        return (int)hipErrorInvalidValue;
    }
    hipStream_t const s = (hipStream_t)stream;
    int const draws = sc != nullptr ? sc->count : 1;
    auto const site = [&](auto set, auto const &...joins)
    { return launch_tiles<grt_tile_chunk_of(decltype(set)::value)>(s, *a, *t, draws, joins...); };
    return grt_launch_joined<grt_tile_instance_exists>(grt_solver_joins(joined(sc, ae)), site);
}

extern "C" int grt_launch_sw_direct_beam(void *stream, GrtSwArgs const *a, double *direct)
{
    if (a == nullptr || direct == nullptr || a->ncol < 1 || a->ncol > 65535 || a->nw < 2 || a->num_levels < 2 ||
        a->tau == nullptr || a->omega == nullptr || a->g == nullptr || a->mu_dir == nullptr || a->tsi == nullptr ||
        a->solar == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(sw_direct_beam_kernel, dim3((unsigned)((a->nw + kDirectBlock - 1)/kDirectBlock), a->ncol, 1),
                       dim3(kDirectBlock), 0, (hipStream_t)stream, *a, direct);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_direct_rows(void *stream, int n, int num_levels, int user_level, double const *levels, double *rows)
{
    if (n < 1 || num_levels < 2 || user_level >= num_levels || levels == nullptr || rows == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(direct_rows_kernel, dim3((unsigned)((n + 63)/64)), dim3(64), 0, (hipStream_t)stream, n, num_levels,
                       user_level, levels, rows);
    return (int)hipGetLastError();
}
