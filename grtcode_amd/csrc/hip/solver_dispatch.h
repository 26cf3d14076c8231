// solver_dispatch.h -- from the joins an instance has set at run time to the template arguments of its kernel.
//
// A solver kernel takes the joined structs that are set as a parameter pack, in the order of the GRT_JOIN_ bits
// (grt_kernels.h), and which sets exist is one constexpr rule per kernel family there.  grt_launch_joined walks a tuple of
// pointers in that order (entry k is bit k), appends each one that is set to the pack and hands the finished pack to the
// family's launch site.  A prefix that no existing instance extends is cut at compile time, so the kernels that get
// instantiated are exactly the rule's, and a set outside it is hipErrorInvalidValue.
#ifndef GRT_SOLVER_DISPATCH_H_
#define GRT_SOLVER_DISPATCH_H_
#include <hip/hip_runtime.h>
#include <tuple>
#include <type_traits>
#include "../grt_kernels.h"

namespace grt_dispatch {

// whether some instance has exactly the joins `Set` among the first K of N and any of the others
template <auto Exists, unsigned Set, int K, int N, auto... Head>
constexpr bool extends()
{
    for (unsigned rest = 0; rest < 1u << (N - K); ++rest)
    {
        if (Exists(Head..., Set | rest << K))
        {
            return true;
        }
    }
    return false;
}

template <auto Exists, unsigned Set, int K, auto... Head, typename Ptrs, typename Site, typename... Joins>
int walk(Ptrs const &ptrs, Site const &site, Joins const &...joins)
{
    constexpr int N = std::tuple_size_v<Ptrs>;
    if constexpr (!extends<Exists, Set, K, N, Head...>())
    {
        return (int)hipErrorInvalidValue;
    }
    else if constexpr (K == N)
    {
        return site(std::integral_constant<unsigned, Set>{}, std::integral_constant<decltype(Head), Head>{}..., joins...);
    }
    else
    {
        auto const *const p = std::get<K>(ptrs);
        return p != nullptr ? walk<Exists, Set | 1u << K, K + 1, Head...>(ptrs, site, joins..., *p) :
                              walk<Exists, Set, K + 1, Head...>(ptrs, site, joins...);
    }
}

} // namespace grt_dispatch

// site(set, head..., joins...) for the instance Exists(Head..., set) of the pointers that are set in `ptrs`: the set and the
// head (an output, a flag, or nothing: what the family's rule takes ahead of the set) as std::integral_constant
template <auto Exists, auto... Head, typename Ptrs, typename Site>
int grt_launch_joined(Ptrs const &ptrs, Site const &site)
{
    return grt_dispatch::walk<Exists, 0u, 0, Head...>(ptrs, site);
}

// ... with the output, too, known at run time only: site(set, out, joins...)
template <auto Exists, int O = 0, typename Ptrs, typename Site>
int grt_launch_output(GrtSolverOutput out, Ptrs const &ptrs, Site const &site)
{
    if constexpr (O > (int)GRT_OUT_LEVEL_BINS)
    {
        return (int)hipErrorInvalidValue;
    }
    else
    {
        return (int)out == O ? grt_launch_joined<Exists, (GrtSolverOutput)O>(ptrs, site) :
                               grt_launch_output<Exists, O + 1>(out, ptrs, site);
    }
}

#endif
