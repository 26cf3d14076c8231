// longwave_dev.h -- what the longwave kernels of more than one file must say alike, to the bit: the effective Planck term
// of a layer, the absorption optical depth of a materialised pass and a thread's point of a longwave pass (LwPoint).
// k_longwave.hip (the four-stream solver and the kernels beside it) and k_longwave_scatter.hip (the two-stream scattering
// correction) take their point, their layer optics and their source terms from here.
#ifndef GRT_LONGWAVE_DEV_H_
#define GRT_LONGWAVE_DEV_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../grt_kernels.h"
#include "optics_dev.h"
#include "planck_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr double kMaxExpArg = 700.;   // grtcode_config.h:41

// longwave.c:100-118 with the two Planck values supplied by the caller
__device__ __forceinline__ double effective_planck(double bc, double be, double tau)
{
    double const a = 0.193;
    double const b = 0.013;
    return (bc + (a*tau + b*tau*tau)*be)/(1. + a*tau + b*tau*tau);
}

// Absorption optical depth of a layer of a materialised pass: tau (1 - omega) at offset o of the pass's rows, omega 0
// where the pass left none  (longwave.c:252)
__device__ __forceinline__ double absorption_tau(double const *tau, double const *omega, uint64_t o)
{
    return omega ? tau[o]*(1. - omega[o]) : tau[o]*(1. - 0.);
}

// One thread's point of a longwave pass, for every kernel that walks a column's layers at a grid point on a solver
// instance's arguments (lw_kernel, lw_radiance_kernel, lw_weighting_kernel): the grid row, the point -- an idle lane of the
// last block follows along at the last one --, its wavenumber, the column's temperatures and emissivity, and the layers'
// absorption optical depth: FUSED, formed in registers from the instance's joins (LayerOptics), else read from the tau,
// omega the pass left on the grid.
template <bool FUSED, typename... Joins>
struct LwPoint
{
    SolverRow const row;
    int const col;
    bool const live;
    uint64_t const ii, nw;
    int const V, L;
    double const w;                                                      // longwave.c:246
    double const *const tau, *const omega, *const tl, *const tv;
    double const emis;
    LayerOptics<FUSED, has_clouds<Joins...>, has<GrtAerosolArgs, Joins...>> const optics;                  // (fused forms)

    __device__ __forceinline__ LwPoint(GrtLwArgs const &a, uint64_t i, Joins const &...joins)
        : row(solver_row(a.ncol, joins...)), col(row.col), live(i < a.nw), ii(live ? i : a.nw - 1), nw(a.nw),
          V(a.num_levels), L(V - 1), w(a.w0 + ii*a.dw), tau(a.tau + (uint64_t)col*a.optics_stride + ii),
          omega((!FUSED && a.omega) ? a.omega + (uint64_t)col*a.optics_stride + ii : nullptr),
          tl(a.t_layers + (uint64_t)col*L), tv(a.t_levels + (uint64_t)col*V),
          emis(a.emis[(uint64_t)col*a.emis_stride + ii]),
          optics(a, pick_clouds(joins...), col, row.tab, ii, pick<GrtAerosolArgs>(joins...))
    {
    }

    // absorption optical depth of layer j: tau (1 - omega)  (longwave.c:252)
    __device__ __forceinline__ double layer_tau(int j) const
    {
        if (FUSED)
        {
            double t, om, gg;
            optics.at(j, t, om, gg);
            return t*(1. - om);
        }
        return absorption_tau(tau, omega, (uint64_t)j*nw);
    }
};

} // namespace

#endif
