// k_kdist.hip -- k-distributions of optical-depth rows (grt_ext.h: grt_kdist_rows, grt_pipeline_run_kdist) and their
// correlated form under one class map per group of rows.
//
// One 256-thread workgroup per (row, bin).  A bin's points are classified against K - 1 class edges, and per class the
// points are counted and their trapezoid weights W_i and the products T_i = W_i tau_i are summed -- each sum the plain
// left-to-right sum in increasing grid index, from +0.0, every product rounded before it is added: the result is a pure
// function of the inputs, bit-identical run to run and to a sequential model on the host.
//
// The workgroup walks its bin in chunks of kChunkPoints points, two phases a chunk:
//   1. every thread takes the points tid, tid + 256, ... of the chunk (coalesced 8-byte loads), finds each one's class by
//      bisection over the class edges in LDS and parks the class (16 bits), W_i and T_i in LDS;
//   2. thread t owns the classes t, t + 256, ...: a wave walks the chunk's classes in index order -- every lane reads the
//      same LDS addresses, a broadcast -- and W_i, T_i and 1 are added in the owner's registers.  With K <= 64 wave 0 owns
//      every class and walks alone, in straight-line code; beyond, every wave that has classes walks, four points a
//      step, and passes a point of another wave's class by on a scalar branch.  A wave none of whose classes exists goes
//      straight to the barrier.
// The accumulators stay in registers across the chunks and are stored once.  No atomics, no tree, no contraction.
// LDS: 18 bytes a point and the class edges, 18 432 + 8 (K - 1) bytes, all in the dynamic region: the eight workgroups
// that a CU's 32 waves allow up to K = 257, six at K = 1024.  (Measured, 64 columns of the bench grids, 16 bins, K = 64:
// 7.9 ms with chunks of 2048 points, four workgroups a CU; 5.0 ms with 1024 -- phase 2 waits for LDS once every four
// points, and a second resident wave per SIMD fills the wait.)
//
// The correlated form (grt_kdist_class_map, grt_kdist_mapped_rows, grt_pipeline_run_kdist_correlated) fixes one class per
// (group, point) -- kdist_map_kernel: the class of a key row or of the sum of the group's rows, 16 bits a point -- and
// reduces every row of the group under it: kdist_mapped_kernel is kdist_kernel with phase 1's bisection replaced by a
// 2-byte load from the map; phase 2 (sum_chunk) is the same function for both.
//
// The flux solves on g-classes (grt_pipeline_run_ck_fluxes) take two more kernels from here: kdist_sources_kernel, the
// mapped kernel with the row's value at a point computed -- the solvers' own Planck function and Rayleigh cross-section --
// instead of loaded, and ck_bin_sum_kernel, the sequential sum of a bin's class fluxes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../grt_kernels.h"
#include "optics_dev.h"
#include "planck_dev.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kChunkPoints = 1024;      // points staged at a time (grt_kdist_chunk_points)
constexpr int kMaxClasses = GRT_KDIST_CLASS_LIMIT;
constexpr int kStep = 4;                // points of phase 2 per LDS read
constexpr unsigned kNoClass = 0xffffu;  // pads a chunk's last step: beyond every class (kMaxClasses <= 0xffff)

static_assert(kChunkPoints % kThreads == 0, "every thread stages the same number of points of a full chunk");
static_assert(kStep == 4 && kChunkPoints % kStep == 0, "load_step reads four points; a padded chunk fits its buffers");
static_assert(kMaxClasses <= 4*kThreads, "a thread owns at most four classes");
static_assert(kMaxClasses < (int)kNoClass, "the class of a point is parked in 16 bits, and the pad is none of them");

// the number of class edges e[0 .. ne - 1] (ascending) with e[k] <= tau, by plain double comparisons: a NaN gives 0
__device__ __forceinline__ int class_of(double const *e, int ne, double tau)
{
    int lo = 0, hi = ne;
    while (lo < hi)
    {
        int const mid = (lo + hi) >> 1;
        if (e[mid] <= tau) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One step of phase 2: the classes (16 bits each), W and T of the four points from j on, in four wide LDS reads.  The
// empty asm pins the values in registers here: without it the compiler moves each read behind the select that uses it,
// under that point's lane mask, and waits for every one of them in turn.
__device__ __forceinline__ void load_step(unsigned short const *c_s, double const *w_s, double const *t_s, int j,
                                          uint64_t &four, double (&w)[kStep], double (&t)[kStep])
{
    four = *reinterpret_cast<uint64_t const *>(c_s + j);
    double2 const w01 = *reinterpret_cast<double2 const *>(w_s + j), w23 = *reinterpret_cast<double2 const *>(w_s + j + 2);
    double2 const t01 = *reinterpret_cast<double2 const *>(t_s + j), t23 = *reinterpret_cast<double2 const *>(t_s + j + 2);
    w[0] = w01.x, w[1] = w01.y, w[2] = w23.x, w[3] = w23.y;
    t[0] = t01.x, t[1] = t01.y, t[2] = t23.x, t[3] = t23.y;
    asm volatile("" : "+v"(four), "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(t[0]), "+v"(t[1]), "+v"(t[2]),
                 "+v"(t[3]));
}

// Phase 2 of a chunk, for both kernels: the owners of the classes add the chunk's `padded` parked points (a multiple of
// kStep, the pad of class kNoClass) to their count, wsum and tsum, in index order.
template <int NC>
__device__ __forceinline__ void sum_chunk(unsigned short const *c_s, double const *w_s, double const *t_s, int padded,
                                          int K, int tid, int wave, bool wave_has_classes, int (&count)[NC],
                                          double (&wsum)[NC], double (&tsum)[NC])
{
    // A point of another thread's class adds +0.0, which changes no bit of a sum that started from +0.0: x + (+0.0)
    // is x for every x but -0.0, NaN and the infinities included, and such a sum is never -0.0 (only -0.0 + -0.0
    // gives that).  So the select sits on the term, off the accumulators' dependency chain.
    if (NC == 1 && K <= 64)
    {
        // one wave owns every class: straight-line code, no point passed by
        if (wave == 0)
        {
            for (int j = 0; j < padded; j += kStep)
            {
                uint64_t four;
                double w[kStep], t[kStep];
                load_step(c_s, w_s, t_s, j, four, w, t);
#pragma unroll
                for (int q = 0; q < kStep; ++q)
                {
                    bool const mine = ((unsigned)(four >> (16*q)) & 0xffffu) == (unsigned)tid;
                    count[0] += mine ? 1 : 0;
                    wsum[0] = __dadd_rn(wsum[0], mine ? w[q] : 0.);
                    tsum[0] = __dadd_rn(tsum[0], mine ? t[q] : 0.);
                }
            }
        }
    }
    else if (wave_has_classes)
    {
        for (int j = 0; j < padded; j += kStep)
        {
            uint64_t four;
            double w[kStep], t[kStep];
            load_step(c_s, w_s, t_s, j, four, w, t);
            unsigned const lo = __builtin_amdgcn_readfirstlane((unsigned)four);
            unsigned const hi = __builtin_amdgcn_readfirstlane((unsigned)(four >> 32));
#pragma unroll
            for (int q = 0; q < kStep; ++q)
            {
                // (the same for every lane, and in scalar registers: class = slot x 256 + wave x 64 + lane)
                unsigned const cls = ((q < 2 ? lo : hi) >> (16*(q & 1))) & 0xffffu;
                if (((cls >> 6) & 3u) != (unsigned)wave)
                {
                    continue;      // another wave's class
                }
                unsigned slot = cls >> 8;
#pragma unroll
                for (int c = 0; c < NC; ++c)
                {
                    if (NC > 1)
                    {
                        // (every test on a value of its own, in a scalar register: the NC tests stay a chain of scalar
                        // branches where the compiler would else fold them into one switch over divergent blocks --
                        // measured at K = 1024, 64 columns of the bench grids: 18.1 ms as a switch, 10.9 ms as the chain)
                        asm volatile("" : "+s"(slot));
                    }
                    if (NC == 1 || slot == (unsigned)c)
                    {
                        if (NC > 1)
                        {
                            asm volatile("");      // (keeps the scalar branch a branch: not NC selects a point)
                        }
                        bool const mine = cls == (unsigned)(tid + c*kThreads);
                        count[c] += mine ? 1 : 0;
                        wsum[c] = __dadd_rn(wsum[c], mine ? w[q] : 0.);
                        tsum[c] = __dadd_rn(tsum[c], mine ? t[q] : 0.);
                    }
                }
            }
        }
    }
}

// NC: the classes a thread owns (K <= NC x 256)
template <int NC>
__global__ __launch_bounds__(kThreads) void kdist_kernel(GrtKdistArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double *w_s = reinterpret_cast<double *>(lds);                          // [kChunkPoints]
    double *t_s = w_s + kChunkPoints;                                       // [kChunkPoints]
    unsigned short *c_s = reinterpret_cast<unsigned short *>(t_s + kChunkPoints);   // [kChunkPoints]
    double *e_s = reinterpret_cast<double *>(c_s + kChunkPoints);           // [K - 1]

    int const tid = threadIdx.x, K = a.num_classes, ne = K - 1;
    // (the wave's number in a scalar register: what it compares a point's class with is then a scalar branch)
    int const wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    for (int k = tid; k < ne; k += kThreads)
    {
        e_s[k] = a.class_edges[k];
    }
    // (wave-uniform: the lowest class of this thread's wave)
    bool const wave_has_classes = wave*64 < K;
    double const half_dw = 0.5*a.dw;

    long long const items = a.rows*(long long)a.num_bins;
    for (long long item = blockIdx.x; item < items; item += gridDim.x)
    {
        long long const row = item/a.num_bins;
        int const bin = (int)(item - row*a.num_bins);
        int const first = a.edges[bin], last = a.edges[bin + 1];
        double const *tau = a.tau + row*a.n;
        int count[NC];
        double wsum[NC], tsum[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
        {
            count[c] = 0;
            wsum[c] = 0.;
            tsum[c] = 0.;
        }
        // (start in 64 bits: the last chunk of a bin that ends near 2^31 must not wrap)
        for (long long start = first; start <= last; start += kChunkPoints)
        {
            int const m = (int)min((long long)kChunkPoints, last - start + 1);
            int const padded = (m + kStep - 1) & ~(kStep - 1);
            __syncthreads();               // the class edges are in place; the chunk before has been summed
            for (int j = tid; j < m; j += kThreads)
            {
                long long const i = start + j;
                double const x = tau[i];
                double w = (i == first || i == last) ? half_dw : a.dw;
                if (a.weight != nullptr)
                {
                    w = __dmul_rn(w, a.weight[i]);
                }
                w_s[j] = w;
                t_s[j] = __dmul_rn(w, x);
                c_s[j] = (unsigned short)class_of(e_s, ne, x);
            }
            for (int j = m + tid; j < padded; j += kThreads)
            {
                w_s[j] = 0.;
                t_s[j] = 0.;
                c_s[j] = (unsigned short)kNoClass;
            }
            __syncthreads();
            sum_chunk<NC>(c_s, w_s, t_s, padded, K, tid, wave, wave_has_classes, count, wsum, tsum);
        }
#pragma unroll
        for (int c = 0; c < NC; ++c)
        {
            int const cls = tid + c*kThreads;
            if (cls < K)
            {
                long long const at = item*K + cls;
                if (a.points != nullptr) a.points[at] = count[c];
                if (a.weight_sum != nullptr) a.weight_sum[at] = wsum[c];
                if (a.tau_sum != nullptr) a.tau_sum[at] = tsum[c];
            }
        }
    }
}

// The class map of grt_kdist_class_map: map[g][i] = class_of(key_i), the key row key_row of group g or (key_row < 0) the
// sum of the group's rows in order from +0.0, every add rounded.  A workgroup takes kChunkPoints points of a group at a
// time, thread t the points t, t + 256, ...: consecutive lanes read consecutive doubles of every row and store
// consecutive shorts.
__global__ __launch_bounds__(kThreads) void kdist_map_kernel(GrtKdistMapArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double *e_s = reinterpret_cast<double *>(lds);                          // [K - 1]
    int const tid = threadIdx.x, ne = a.num_classes - 1;
    for (int k = tid; k < ne; k += kThreads)
    {
        e_s[k] = a.class_edges[k];
    }
    __syncthreads();
    long long const tiles = (a.n + kChunkPoints - 1)/kChunkPoints, items = a.groups*tiles;
    for (long long item = blockIdx.x; item < items; item += gridDim.x)
    {
        long long const g = item/tiles, start = (item - g*tiles)*kChunkPoints;
        double const *x = a.x + g*a.rows_per_group*a.n;
        long long const end = min(a.n, start + kChunkPoints);
        for (long long i = start + tid; i < end; i += kThreads)
        {
            double key;
            if (a.key_row >= 0)
            {
                key = x[a.key_row*a.n + i];
            }
            else
            {
                key = 0.;
                for (long long r = 0; r < a.rows_per_group; ++r)
                {
                    key = __dadd_rn(key, x[r*a.n + i]);
                }
            }
            a.map[g*a.n + i] = (unsigned short)class_of(e_s, ne, key);
        }
    }
}

// grt_kdist_mapped_rows: kdist_kernel's walk, one workgroup per (group, row, bin), with the class of a point read from the
// group's map in place of the bisection -- an entry that names no class (>= K) becomes the pad, which no thread owns.  The
// counts and the weight sums are the same for every row of a group: the workgroup of row 0 stores them.
// LDS: 18 bytes a point, 18 432 bytes.
template <int NC>
__global__ __launch_bounds__(kThreads) void kdist_mapped_kernel(GrtKdistMappedArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double *w_s = reinterpret_cast<double *>(lds);                          // [kChunkPoints]
    double *t_s = w_s + kChunkPoints;                                       // [kChunkPoints]
    unsigned short *c_s = reinterpret_cast<unsigned short *>(t_s + kChunkPoints);   // [kChunkPoints]

    int const tid = threadIdx.x, K = a.num_classes;
    int const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    bool const wave_has_classes = wave*64 < K;
    double const half_dw = 0.5*a.dw;

    long long const per_group = a.rows_per_group*(long long)a.num_bins, items = a.groups*per_group;
    for (long long item = blockIdx.x; item < items; item += gridDim.x)
    {
        long long const g = item/per_group, row = (item - g*per_group)/a.num_bins;
        int const bin = (int)(item - g*per_group - row*a.num_bins);
        int const first = a.edges[bin], last = a.edges[bin + 1];
        double const *v = a.values + g*a.group_stride + row*a.n;
        unsigned short const *map = a.map + g*a.n;
        int count[NC];
        double wsum[NC], tsum[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c)
        {
            count[c] = 0;
            wsum[c] = 0.;
            tsum[c] = 0.;
        }
        for (long long start = first; start <= last; start += kChunkPoints)
        {
            int const m = (int)min((long long)kChunkPoints, last - start + 1);
            int const padded = (m + kStep - 1) & ~(kStep - 1);
            __syncthreads();               // the chunk before has been summed
            for (int j = tid; j < m; j += kThreads)
            {
                long long const i = start + j;
                double const x = v[i];
                unsigned const cls = map[i];
                double w = (i == first || i == last) ? half_dw : a.dw;
                if (a.weight != nullptr)
                {
                    w = __dmul_rn(w, a.weight[i]);
                }
                w_s[j] = w;
                t_s[j] = __dmul_rn(w, x);
                c_s[j] = (unsigned short)(cls < (unsigned)K ? cls : kNoClass);
            }
            for (int j = m + tid; j < padded; j += kThreads)
            {
                w_s[j] = 0.;
                t_s[j] = 0.;
                c_s[j] = (unsigned short)kNoClass;
            }
            __syncthreads();
            sum_chunk<NC>(c_s, w_s, t_s, padded, K, tid, wave, wave_has_classes, count, wsum, tsum);
        }
        bool const shared_out = row == 0;
#pragma unroll
        for (int c = 0; c < NC; ++c)
        {
            int const cls = tid + c*kThreads;
            if (cls < K)
            {
                long long const at = (g*a.num_bins + bin)*K + cls;
                if (shared_out && a.points != nullptr) a.points[at] = count[c];
                if (shared_out && a.weight_sum != nullptr) a.weight_sum[at] = wsum[c];
                if (a.tau_sum != nullptr) a.tau_sum[item*K + cls] = tsum[c];
            }
        }
    }
}

// The value of source row `row` of column g at grid point i (GrtCkSourceArgs, grt_kernels.h): the longwave's Planck rows
// by the solver's own planck() at the solver's own wavenumber (planck_dev.h), the shortwave's Rayleigh cross-section by
// the solver's rayleigh_tau with n = 1 (optics_dev.h); the data rows are loaded.
__device__ __forceinline__ double source_value(GrtCkSourceArgs const &a, long long g, int row, long long i)
{
    int const V = a.num_levels;
    if (a.longwave)
    {
        if (row == 2*V)
        {
            return a.data[0][(uint64_t)g*a.data_stride[0] + (uint64_t)i];
        }
        double const T = row < V ? a.t_levels[g*V + row] : (row < 2*V - 1 ? a.t_layers[g*(V - 1) + (row - V)] : a.t_surf[g]);
        return planck(T, grid_wavenumber(a.w0, a.dw, (uint64_t)i));
    }
    if (row == 0)
    {
        return rayleigh_tau(grid_wavenumber(a.w0, a.dw, (uint64_t)i), 1.0);
    }
    return a.data[row - 1][(uint64_t)g*a.data_stride[row - 1] + (uint64_t)i];
}

// The source sums of a correlated-k model: kdist_mapped_kernel's walk, one workgroup per (column, source row, bin), phase 1
// with the row's value at the point computed (source_value) instead of loaded; phase 2 is sum_chunk.  Only the sums of
// weight x value leave: the counts and the weight sums are the mapped reduction's.
// LDS: 18 bytes a point, 18 432 bytes.
// OWNED: the classes a thread owns, as the other kernels' NC
template <int OWNED>
__global__ __launch_bounds__(kThreads) void kdist_sources_kernel(GrtCkSourceArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double *w_s = reinterpret_cast<double *>(lds);                          // [kChunkPoints]
    double *t_s = w_s + kChunkPoints;                                       // [kChunkPoints]
    unsigned short *c_s = reinterpret_cast<unsigned short *>(t_s + kChunkPoints);   // [kChunkPoints]

    int const tid = threadIdx.x, K = a.num_classes;
    int const wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    bool const wave_has_classes = wave*64 < K;
    double const half_dw = 0.5*a.dw;
    int const R = a.longwave ? 2*a.num_levels + 1 : 4;

    long long const per_group = R*(long long)a.num_bins, items = a.ncol*per_group;
    for (long long item = blockIdx.x; item < items; item += gridDim.x)
    {
        long long const g = item/per_group;
        int const row = (int)((item - g*per_group)/a.num_bins);
        int const bin = (int)(item - g*per_group - (long long)row*a.num_bins);
        int const first = a.edges[bin], last = a.edges[bin + 1];
        unsigned short const *map = a.map + g*a.n;
        int count[OWNED];
        double wsum[OWNED], tsum[OWNED];
#pragma unroll
        for (int c = 0; c < OWNED; ++c)
        {
            count[c] = 0;
            wsum[c] = 0.;
            tsum[c] = 0.;
        }
        for (long long start = first; start <= last; start += kChunkPoints)
        {
            int const m = (int)min((long long)kChunkPoints, last - start + 1);
            int const padded = (m + kStep - 1) & ~(kStep - 1);
            __syncthreads();               // the chunk before has been summed
            for (int j = tid; j < m; j += kThreads)
            {
                long long const i = start + j;
                double const x = source_value(a, g, row, i);
                unsigned const cls = map[i];
                double const w = (i == first || i == last) ? half_dw : a.dw;
                w_s[j] = w;
                t_s[j] = __dmul_rn(w, x);
                c_s[j] = (unsigned short)(cls < (unsigned)K ? cls : kNoClass);
            }
            for (int j = m + tid; j < padded; j += kThreads)
            {
                w_s[j] = 0.;
                t_s[j] = 0.;
                c_s[j] = (unsigned short)kNoClass;
            }
            __syncthreads();
            sum_chunk<OWNED>(c_s, w_s, t_s, padded, K, tid, wave, wave_has_classes, count, wsum, tsum);
        }
#pragma unroll
        for (int c = 0; c < OWNED; ++c)
        {
            int const cls = tid + c*kThreads;
            if (cls < K)
            {
                a.source_sum[item*K + cls] = tsum[c];
            }
        }
    }
}

// The bin sums of a correlated-k model's class fluxes: one thread per row of K classes adds them in class order from +0.0.
__global__ __launch_bounds__(kThreads) void ck_bin_sum_kernel(double const *in, long long rows, int K, double *out)
{
    long long const r = (long long)blockIdx.x*kThreads + threadIdx.x;
    if (r >= rows)
    {
        return;
    }
    double const *x = in + r*K;
    double sum = 0.;
    for (int k = 0; k < K; ++k)
    {
        sum = __dadd_rn(sum, x[k]);
    }
    out[r] = sum;
}

}  // namespace

extern "C" int grt_launch_ck_sources(void *stream, GrtCkSourceArgs const *a)
{
    if (a == nullptr || a->map == nullptr || a->source_sum == nullptr || a->edges == nullptr || a->ncol < 1 || a->n < 2 ||
        a->num_levels < 2 || a->num_bins < 1 || a->num_classes < 2 || a->num_classes > kMaxClasses || a->data[0] == nullptr ||
        (a->longwave ? a->t_levels == nullptr || a->t_layers == nullptr || a->t_surf == nullptr
                     : a->data[1] == nullptr || a->data[2] == nullptr))
    {
        return (int)hipErrorInvalidValue;
    }
    long long const items = a->ncol*(a->longwave ? 2*a->num_levels + 1 : 4)*(long long)a->num_bins;
    unsigned const blocks = (unsigned)(items < (1ll << 20) ? items : (1ll << 20));
    size_t const lds = (size_t)kChunkPoints*(2*sizeof(double) + sizeof(unsigned short));
    hipStream_t const s = (hipStream_t)stream;
    if (a->num_classes <= kThreads)
    {
        hipLaunchKernelGGL(kdist_sources_kernel<1>, dim3(blocks), dim3(kThreads), lds, s, *a);
    }
    else if (a->num_classes <= 2*kThreads)
    {
        hipLaunchKernelGGL(kdist_sources_kernel<2>, dim3(blocks), dim3(kThreads), lds, s, *a);
    }
    else
    {
        hipLaunchKernelGGL(kdist_sources_kernel<4>, dim3(blocks), dim3(kThreads), lds, s, *a);
    }
    return (int)hipGetLastError();
}

extern "C" int grt_launch_ck_bin_sum(void *stream, double const *in, long long rows, int num_classes, double *out)
{
    if (in == nullptr || out == nullptr || rows < 1 || num_classes < 1 || (rows + kThreads - 1)/kThreads > 0x7fffffffll)
    {
        return (int)hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(ck_bin_sum_kernel, dim3((unsigned)((rows + kThreads - 1)/kThreads)), dim3(kThreads), 0,
                       (hipStream_t)stream, in, rows, num_classes, out);
    return (int)hipGetLastError();
}

extern "C" int grt_kdist_chunk(void)
{
    return kChunkPoints;
}

extern "C" int grt_launch_kdist(void *stream, GrtKdistArgs const *a)
{
    if (a == nullptr || a->tau == nullptr || a->rows < 1 || a->n < 2 || a->num_bins < 1 || a->edges == nullptr ||
        a->num_classes < 2 || a->num_classes > kMaxClasses || a->class_edges == nullptr ||
        (a->points == nullptr && a->weight_sum == nullptr && a->tau_sum == nullptr))
    {
        return (int)hipErrorInvalidValue;
    }
    long long const items = a->rows*(long long)a->num_bins;
    unsigned const blocks = (unsigned)(items < (1ll << 20) ? items : (1ll << 20));
    size_t const lds = (size_t)kChunkPoints*(2*sizeof(double) + sizeof(unsigned short)) +
                       sizeof(double)*(size_t)(a->num_classes - 1);
    hipStream_t const s = (hipStream_t)stream;
    if (a->num_classes <= kThreads)
    {
        hipLaunchKernelGGL(kdist_kernel<1>, dim3(blocks), dim3(kThreads), lds, s, *a);
    }
    else if (a->num_classes <= 2*kThreads)
    {
        hipLaunchKernelGGL(kdist_kernel<2>, dim3(blocks), dim3(kThreads), lds, s, *a);
    }
    else
    {
        hipLaunchKernelGGL(kdist_kernel<4>, dim3(blocks), dim3(kThreads), lds, s, *a);
    }
    return (int)hipGetLastError();
}

extern "C" int grt_launch_kdist_map(void *stream, GrtKdistMapArgs const *a)
{
    if (a == nullptr || a->x == nullptr || a->map == nullptr || a->groups < 1 || a->rows_per_group < 1 || a->n < 1 ||
        a->key_row >= a->rows_per_group || a->num_classes < 2 || a->num_classes > kMaxClasses ||
        a->class_edges == nullptr)
    {
        return (int)hipErrorInvalidValue;
    }
    long long const items = a->groups*((a->n + kChunkPoints - 1)/kChunkPoints);
    unsigned const blocks = (unsigned)(items < (1ll << 20) ? items : (1ll << 20));
    size_t const lds = sizeof(double)*(size_t)(a->num_classes - 1);
    hipLaunchKernelGGL(kdist_map_kernel, dim3(blocks), dim3(kThreads), lds, (hipStream_t)stream, *a);
    return (int)hipGetLastError();
}

extern "C" int grt_launch_kdist_mapped(void *stream, GrtKdistMappedArgs const *args)
{
    if (args == nullptr || args->values == nullptr || args->map == nullptr || args->groups < 1 ||
        args->rows_per_group < 1 || args->n < 2 || args->group_stride < args->rows_per_group*args->n ||
        args->num_bins < 1 || args->edges == nullptr || args->num_classes < 2 || args->num_classes > kMaxClasses ||
        (args->points == nullptr && args->weight_sum == nullptr && args->tau_sum == nullptr))
    {
        return (int)hipErrorInvalidValue;
    }
    GrtKdistMappedArgs a = *args;
    if (a.tau_sum == nullptr)
    {
        a.rows_per_group = 1;      // the counts and the weight sums are row 0's workgroups' alone
    }
    long long const items = a.groups*a.rows_per_group*(long long)a.num_bins;
    unsigned const blocks = (unsigned)(items < (1ll << 20) ? items : (1ll << 20));
    size_t const lds = (size_t)kChunkPoints*(2*sizeof(double) + sizeof(unsigned short));
    hipStream_t const s = (hipStream_t)stream;
    if (a.num_classes <= kThreads)
    {
        hipLaunchKernelGGL(kdist_mapped_kernel<1>, dim3(blocks), dim3(kThreads), lds, s, a);
    }
    else if (a.num_classes <= 2*kThreads)
    {
        hipLaunchKernelGGL(kdist_mapped_kernel<2>, dim3(blocks), dim3(kThreads), lds, s, a);
    }
    else
    {
        hipLaunchKernelGGL(kdist_mapped_kernel<4>, dim3(blocks), dim3(kThreads), lds, s, a);
    }
    return (int)hipGetLastError();
}
