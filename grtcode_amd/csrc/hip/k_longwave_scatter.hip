// k_longwave_scatter.hip -- the longwave scattering correction for gfx950: two-stream adding, solved twice per grid point.
//
// There is no reference counterpart: longwave.c treats every particle as an absorber (tau (1 - omega), longwave.c:252),
// and so does lw_kernel.  What this file adds is the difference a two-stream solve sees between the layer optics as they
// are and their absorption twin, to be added to lw_kernel's four-stream fluxes:
//
//   delta_up_i = F_up_i[tau, omega, g] - F_up_i[tau (1 - omega), 0, 0]      (the same for down),  corrected = four-stream + delta.
//
// Both solves run through the same functions below, so a point none of whose layers scatters (omega = 0 everywhere) gives
// the two the same inputs and the difference is exactly +0.0; the four-stream quadrature stays what carries everything
// that does not scatter.  Per layer, with D = 1.66 (two_stream_layer):
//
//   gamma1 = D (1 - omega (1 + g)/2),  gamma2 = D omega (1 - g)/2,  k = sqrt(max((gamma1 - gamma2)(gamma1 + gamma2), 1e-12)),
//   x = min(k tau, 700),  e = exp(-x),  E = -expm1(-2 x),  m = -expm1(-x),  den = k (1 + e e) + gamma1 E,
//   R = gamma2 E/den,  T = 2 k e/den,  eps = (k m m + (gamma1 - gamma2) E)/den     (= 1 - R - T, no cancelling difference),
//   S_up = eps pi effective_planck(B(t_layer_j), B(t_level_j), tau (1 - omega)),
//   S_down = eps pi effective_planck(B(t_layer_j), B(t_level_j+1), tau (1 - omega)).
//
// planck and effective_planck are the device functions lw_kernel uses, on the arguments it gives them (longwave_dev.h,
// planck_dev.h): the source of the correction is the no-scattering solver's own.  Adding, level V - 1 the surface and
// layer j between levels j and j + 1 (adding_up, adding_down):
//
//   A_L = 1 - emis,  U_L = emis pi B(t_surf)
//   up:    beta_j = 1/(1 - A_{j+1} R_j);  A_j = R_j + T_j T_j A_{j+1} beta_j;  U_j = S_up_j + T_j (U_{j+1} + A_{j+1} S_down_j) beta_j
//   down:  F_down_0 = 0, F_up_0 = U_0;  F_down_{j+1} = (T_j F_down_j + R_j U_{j+1} + S_down_j) beta_j;
//          F_up_{j+1} = A_{j+1} F_down_{j+1} + U_{j+1}
//
// One thread per (grid point, grid row), kSolverBlock threads a workgroup, exactly as lw_kernel (LwPoint).  The first sweep
// runs from the surface to the top with (A, U) of both solves in registers -- no per-thread array -- and parks what the
// second needs in coalesced rows [grid row][layer][GRT_SCATTER_PARK_ROWS][pw], pw the launch's workgroups x kSolverBlock:
// R_j, T_j, S_down_j, A_{j+1}, U_{j+1} of the scattering solve, then of the twin.  The second sweep runs from the top down
// on those rows, with no exponential, square root or Planck term of its own, and hands both differences of every level to
// a LevelSink: the spectral rows (GRT_OUT_CHAINS), the six rows' or every level's partial sums (GRT_OUT_ROWS,
// GRT_OUT_LEVELS) -- lw_kernel's sums, association and layout.  Parking the layers' R, T, S_down beside A and U, as the
// shortwave parks its five layer properties, and not A and U alone with the layers worked out a second time, follows
// from a measurement.  Control flow is uniform across a wave wherever the sink sums a level: the idle
// lanes of a last block follow along at the last point with weight 0, and park in places of their own.
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

constexpr double kDiffusivity = 1.66;
constexpr double kPi = 3.14159265358979323846;
constexpr double kMinK2 = 1e-12;
constexpr int kParkRows = GRT_SCATTER_PARK_ROWS;

// reflectance, transmittance and the two thermal sources of one layer; pu, pd: the effective Planck terms of the upward and
// the downward source (of the layer's absorption optical depth, whatever the solve)
__device__ __forceinline__ void two_stream_layer(double tau, double omega, double g, double pu, double pd, double &R,
                                                 double &T, double &su, double &sd)
{
    double const g1 = kDiffusivity*(1. - omega*(1. + g)/2.);
    double const g2 = kDiffusivity*omega*(1. - g)/2.;
    double const k = sqrt(fmax((g1 - g2)*(g1 + g2), kMinK2));
    double const x = fmin(k*tau, kMaxExpArg);
    double const e = exp(-x);
    double const E = -expm1(-2.*x);
    double const m = -expm1(-x);
    double const den = k*(1. + e*e) + g1*E;
    R = g2*E/den;
    T = 2.*k*e/den;
    double const eps = (k*m*m + (g1 - g2)*E)/den;
    su = eps*kPi*pu;
    sd = eps*kPi*pd;
}

// the layer under the stack (A, U) below it: the stack seen from the layer's top
__device__ __forceinline__ void adding_up(double R, double T, double su, double sd, double &A, double &U)
{
    double const beta = 1./(1. - A*R);
    double const a = R + T*T*A*beta;
    U = su + T*(U + A*sd)*beta;
    A = a;
}

// the fluxes at the layer's bottom from the downward flux at its top and the stack (A, U) below it
__device__ __forceinline__ void adding_down(double R, double T, double sd, double A, double U, double &fd, double &fu)
{
    double const beta = 1./(1. - A*R);
    fd = (T*fd + R*U + sd)*beta;
    fu = A*fd + U;
}

// tau, omega, g of layer j of a thread's point: FUSED, formed in registers from the instance's joins (LayerOptics, as every
// fused solver's), else read from the tau, omega, g a pass left on the grid (omega, g NULL: 0)
template <bool FUSED, typename... Joins>
__device__ __forceinline__ void layer_optics(LwPoint<FUSED, Joins...> const &p, double const *g, int j, double &t, double &om,
                                             double &gg)
{
    if constexpr (FUSED)
    {
        p.optics.at(j, t, om, gg);
    }
    else
    {
        uint64_t const o = (uint64_t)j*p.nw;
        t = p.tau[o];
        om = p.omega ? p.omega[o] : 0.;
        gg = g ? g[o] : 0.;
    }
}

template <GrtSolverOutput OUT, typename... Joins>
__global__ __launch_bounds__(kSolverBlock) void lw_scatter_kernel(GrtLwArgs a, GrtScatterArgs sa, Joins... joins)
{
    uint64_t const i = (uint64_t)blockIdx.x*kSolverBlock + threadIdx.x;
    constexpr bool FUSED = grt_out_fused(OUT), PROFILE = grt_out_levels(OUT);
    static_assert(OUT == GRT_OUT_CHAINS || OUT == GRT_OUT_ROWS || OUT == GRT_OUT_LEVELS, "the chain, six-row and level forms");
    if (!FUSED && i >= a.nw)                      // (fused form: idle lanes of the last block follow along, weight 0)
    {
        return;
    }
    LwPoint<FUSED, Joins...> const p(a, i, joins...);
    int const L = p.L;
    double const w = p.w;
    LevelSink<FUSED, PROFILE> sink(a, p.row.slot, i, p.live);
    double const *g = !FUSED && sa.g ? sa.g + (uint64_t)p.col*a.optics_stride + p.ii : nullptr;
    uint64_t const pw = (uint64_t)gridDim.x*kSolverBlock;
    double *park = sa.park + (uint64_t)p.row.park*(uint64_t)L*kParkRows*pw + i;

    // sweep 1, from the surface to the top: (A, U) of the scattering solve and of its absorption twin
    double const bs = planck(a.t_surf[p.col], w);
    double As = 1. - p.emis, Us = p.emis*kPi*bs;
    double Aa = As, Ua = Us;
    for (int j = L - 1; j >= 0; --j)
    {
        double t, om, gg;
        layer_optics(p, g, j, t, om, gg);
        double const ta = t*(1. - om);                                   // longwave.c:252
        double const bc = planck(p.tl[j], w);
        double const pu = effective_planck(bc, planck(p.tv[j], w), ta);
        double const pd = effective_planck(bc, planck(p.tv[j + 1], w), ta);
        double *q = park + (uint64_t)j*kParkRows*pw;
        double R, T, su, sd;
        two_stream_layer(t, om, gg, pu, pd, R, T, su, sd);
        q[0] = R; q[pw] = T; q[2*pw] = sd; q[3*pw] = As; q[4*pw] = Us;
        adding_up(R, T, su, sd, As, Us);
        two_stream_layer(ta, 0., 0., pu, pd, R, T, su, sd);
        q[5*pw] = R; q[6*pw] = T; q[7*pw] = sd; q[8*pw] = Aa; q[9*pw] = Ua;
        adding_up(R, T, su, sd, Aa, Ua);
    }

    // sweep 2, from the top down: both solves' fluxes at every level, and their differences to the sink
    double *su_out = nullptr, *sd_out = nullptr;
    if constexpr (!FUSED)
    {
        if (sa.flux_up != nullptr)
        {
            su_out = sa.flux_up + (uint64_t)p.col*a.flux_stride + i;
            sd_out = sa.flux_down + (uint64_t)p.col*a.flux_stride + i;
        }
    }
    double fds = 0., fus = Us, fda = 0., fua = Ua;
    sink.put(0, false, fus - fua);
    sink.put_zero(0, true);
    if (su_out != nullptr)
    {
        su_out[0] = fus;
        sd_out[0] = fds;
    }
    for (int j = 0; j < L; ++j)
    {
        double const *q = park + (uint64_t)j*kParkRows*pw;
        adding_down(q[0], q[pw], q[2*pw], q[3*pw], q[4*pw], fds, fus);
        adding_down(q[5*pw], q[6*pw], q[7*pw], q[8*pw], q[9*pw], fda, fua);
        sink.put(j + 1, false, fus - fua);
        sink.put(j + 1, true, fds - fda);
        if (su_out != nullptr)
        {
            su_out[(uint64_t)(j + 1)*p.nw] = fus;
            sd_out[(uint64_t)(j + 1)*p.nw] = fds;
        }
    }
    sink.finish(a);
}

// the one launch site of lw_scatter_kernel: the instance of OUT and of the joined arguments' types, on lw_kernel's grid and LDS
template <GrtSolverOutput OUT, typename... Joins>
int launch(hipStream_t s, GrtSolverInstance const &in, GrtLwArgs const &a, Joins const &...joins)
{
    dim3 const grid(grt_solver_blocks(a.nw), (unsigned)grt_solver_grid_rows(&in, a.ncol), 1);
    hipLaunchKernelGGL((lw_scatter_kernel<OUT, Joins...>), grid, dim3(kSolverBlock), grt_solver_lds(&in, a.num_levels), s, a,
                       *in.scatter, joins...);
    return (int)hipGetLastError();
}

constexpr int kAddBlock = 256;
__global__ __launch_bounds__(kAddBlock) void scatter_add_kernel(int n, int rows, double *corrected, uint64_t out_stride,
                                                                uint64_t out_offset, double const *delta,
                                                                uint64_t delta_stride, uint64_t delta_offset)
{
    uint64_t const t = (uint64_t)blockIdx.x*kAddBlock + threadIdx.x;
    if (t >= (uint64_t)n*(uint64_t)rows)
    {
        return;
    }
    uint64_t const c = t/(uint64_t)rows, r = t - c*(uint64_t)rows;
    double *to = corrected + c*out_stride + out_offset + r;
    *to = *to + delta[c*delta_stride + delta_offset + r];
}

} // namespace

extern "C" int grt_launch_lw_scatter(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a)
{
    if (in == nullptr || a == nullptr || in->scatter == nullptr || !grt_solver_instance_ok(*in, *a) ||
        a->t_layers == nullptr || a->t_levels == nullptr || a->t_surf == nullptr || a->emis == nullptr ||
        (!grt_out_fused(in->out) && a->tau == nullptr))
    {
        return (int)hipErrorInvalidValue;
    }
    hipStream_t const s = (hipStream_t)stream;
    // every instance of lw_scatter_kernel there is (grt_lw_scatter_instance_exists)
    auto const site = [&](auto, auto out, auto const &...joins) { return launch<decltype(out)::value>(s, *in, *a, joins...); };
    return grt_launch_output<grt_lw_scatter_instance_exists>(in->out, grt_solver_joins(*in), site);
}

extern "C" int grt_launch_scatter_add(void *stream, int n, int rows, double *corrected, uint64_t out_stride,
                                      uint64_t out_offset, double const *delta, uint64_t delta_stride, uint64_t delta_offset)
{
    if (n < 1 || rows < 1 || corrected == nullptr || delta == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    uint64_t const threads = (uint64_t)n*(uint64_t)rows;
    hipLaunchKernelGGL(scatter_add_kernel, dim3((unsigned)((threads + kAddBlock - 1)/kAddBlock)), dim3(kAddBlock), 0,
                       (hipStream_t)stream, n, rows, corrected, out_stride, out_offset, delta, delta_stride, delta_offset);
    return (int)hipGetLastError();
}
