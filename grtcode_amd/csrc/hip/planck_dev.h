// planck_dev.h -- the Planck function and the wavenumber of a grid point as the longwave solver forms them, for every
// kernel that must form the same doubles: the solver kernels (k_longwave.hip) and the source sums of a correlated-k model
// (k_kdist.hip: kdist_sources_kernel).
#ifndef GRT_PLANCK_DEV_H_
#define GRT_PLANCK_DEV_H_
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)

// planck_law's constants (longwave.c:70-71)
constexpr double kPlanckC1 = 1.1910429526245744e-8;
constexpr double kPlanckC2 = 1.4387773538277202;
constexpr double kPlanckMaxExpArg = 700.;   // grtcode_config.h:41

// the wavenumber of grid point i (longwave.c:246)
__device__ __forceinline__ double grid_wavenumber(double w0, double dw, uint64_t i)
{
    return w0 + i*dw;
}

// longwave.c:68-94
__device__ __forceinline__ double planck(double T, double w)
{
    double const c1 = kPlanckC1;
    double const c2 = kPlanckC2;
    double e = c2*w/T;
    if (e > kPlanckMaxExpArg)
    {
        e = kPlanckMaxExpArg;
    }
    e = exp(e);
    return (c1*w*w*w)/(e - 1.);
}

#endif
