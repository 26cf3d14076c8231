/* grt_kernels.h -- C-callable launch wrappers of the hand-written gfx950 kernels.
 *
 * Shared between the C99 host layer (csrc/host) and the HIP translation units
 * (csrc/hip).  Every wrapper enqueues on the given stream and returns a
 * hipError_t cast to int (0 == success); none of them allocates or synchronises.
 * All pointers are device pointers unless a name ends in _h.
 */
#ifndef GRT_KERNELS_H_
#define GRT_KERNELS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRT_MAX_ISO 18      /* largest isotopologue count in the molecule table (O3) */
#define GRT_MAX_SLOTS 53    /* NUM_MOLS */
#define GRT_MAX_TABLES 32   /* 4 H2O + 1 O3 + 21 CFC + 3 CIA + spare */

/* Merged line store: all active molecules, sorted by unshifted centre.  The five
   f32 arrays hold values the reference itself reads through a float
   (parse_HITRAN_file.c:197-212), so nothing is lost by the narrower storage. */
typedef struct GrtLineStore
{
    uint64_t n;
    double const *v0;       /* centre [cm-1] */
    double const *s0;       /* strength rescaled at load (parse_HITRAN_file.c:372-384) */
    float const *yair;
    float const *yself;
    float const *en;
    float const *nexp;
    float const *delta;
    uint8_t const *iso;     /* 1-based isotopologue id */
    uint8_t const *slot;    /* molecule slot (order of add_molecule) */
    double dmax;            /* max |delta| over the store: bound on the pressure shift */
    double nmax;            /* max |nexp| over the store and, per molecule slot, the largest yair / yself */
    float yair_max[GRT_MAX_SLOTS];   /* [cm-1 atm-1]: together a bound on the Lorentz half-width of any */
    float yself_max[GRT_MAX_SLOTS];  /* line in a layer (kernels.c:105-106), see k_gas_optics_mp.hip */
    /* Packed fp32 records of the same lines, in the same order, for the lean first pass of the two-pass moment kernel
       (k_gas_optics_mp.hip: lean_block) -- built for ONE grid (lean_w0, lean_wres); NULL: none.  The lean loop takes TWO
       lines per lane and does their arithmetic with gfx950's packed fp32 instructions (v_pk_fma_f32 ...: one instruction,
       two lines), so the records come PAIR-INTERLEAVED: pair q = lines 2q, 2q + 1 (an odd store's last pair repeats the
       last line with its strength zeroed), every field of the two lines side by side -- a 16-byte load puts each field
       in an aligned register pair, the operand form of the packed instructions.
         lean_a [2][npair][4]: plane 0: d0 of line 2q, of line 2q + 1, c0 of line 2q, of line 2q + 1 -- d0 = offset of the
                        UNSHIFTED centre from its nearest grid point, in grid steps, [-0.5, 0.5); c0 = that grid point's
                        index floor((v0 - w0)/wres + 0.5) (int32 bit pattern);
                        plane 1: v0 as f32 (twice), s0 * 2^GRT_LEAN_S0_SHIFT as f32 (twice)
         lean_b [2][npair][4]: plane 0: yair (twice), yself (twice); plane 1: en (twice), delta (twice)
         lean_c [npair][2]: per line: bits 0-7   index of the temperature exponent, nexp*100 (255: not a whole number of
                        hundredths below 128), bits 8-13  molecule slot,  bits 14-23  slot*GRT_MAX_ISO + iso - 1,
                        bit 31     the line always takes the general path (strength outside the scaled fp32 range, ...) */
    /*   lean_x [n][2] doubles: what the exact preparation of a core point needs of its line in ONE 16-byte load: the fp64
                        centre v0, and yair, yself (two f32 in the second double's place) */
    float const *lean_a;
    float const *lean_b;
    uint32_t const *lean_c;
    double const *lean_x;
    uint64_t lean_npair;
    double lean_w0, lean_wres;
} GrtLineStore;
#define GRT_LEAN_S0_SHIFT 96
#define GRT_LEAN_GENERAL 0x80000000u

/* Per-column layer state prepared on the host in the reference's arithmetic
   (curtis_godson.c:25-106, kernels.c:52-66,117-127) and uploaded once per column.
   Layout of one column block (doubles):
     lay  [L][4]            : pavg, tavg, 1/tavg, log(296/tavg)
     ms   [nslot][L][4]     : ps, pavg-ps, ns, doppler factor sqrt(2 kb T/(m c c))
     q    [nslot][L][GRT_MAX_ISO] : 1/Q(T, iso)
     cont [L][GRT_MAX_TABLES] : per-layer multiplier of each continuum-type table
     h2o  [L][4]            : N_s(296/T), Ps, P-Ps, 296-T  (kernels.c:484-487)
*/
typedef struct GrtColumnLayout
{
    int num_layers;
    int num_slots;
    int num_tables;      /* linear tables: tau += cont[layer][k]*table[k][f] */
    int has_h2o_ctm;     /* tables 0..3 of the h2o block are F296,S296,CKDF,CKDS */
    uint64_t stride;     /* doubles per column */
    uint64_t off_lay, off_ms, off_q, off_cont, off_h2o;
} GrtColumnLayout;

/* Where the spectral tables hold anything: [lo, hi) = from the first to one past the last grid point whose entry is not
   +-0 (a CFC's band, a CIA pair's; the water-vapour pair: either 296 K coefficient).  Outside it the reference adds
   cont*0 (kernels.c:585-630 run over the whole grid): a workgroup whose points lie outside skips the table's loads. */
typedef struct GrtTableSpans
{
    int lo[GRT_MAX_TABLES], hi[GRT_MAX_TABLES];
    int h2o_lo, h2o_hi;
} GrtTableSpans;

typedef struct GrtGasOpticsArgs
{
    GrtLineStore lines;
    GrtColumnLayout lay;
    double const *colstate;   /* [ncol][lay.stride] */
    double const *tables;     /* [num_tables][nw] linear tables (O3, CFC, CIA) */
    double const *h2o_tables; /* [4][nw] or NULL */
    double w0, wres;          /* bins.w0 / bins.wres (spectral_bin.c:39-40) */
    uint64_t nw;
    int ncol;
    double *tau;              /* [ncol][L][nw] */
    uint64_t tau_col_stride;  /* doubles between columns */
    int tile;                 /* wavenumbers per workgroup (multiple of 64) */
    int nslice;               /* line slices per tile (>=1); >1 uses global atomics */
    int fast;                 /* 0: reference operation order; 1: fused form, far wings by cell moments
                                 where the window is wide enough; 2: fused form, every point in the ring;
                                 3: as 1 in two passes (cell moments through gmom) */
    float *gmom;              /* two-pass form only: [ncol][L] blocks of gmom_stride floats; level 0 = [nw][mom_terms] cell
                                 moments, then (tree_levels > 0) levels 1..tree_levels: level l holds ceil(nw/2^l) cells and
                                 starts where nw_pad*(2 - 2^(1-l)) cells end, nw_pad = nw rounded up to a multiple of
                                 2^tree_levels (grt_gas_optics_moment_floats sizes a block) */
    uint64_t gmom_stride;
    int halo;                 /* two-pass form: grid points either side of a cell tile the first pass may add to
                                 (the window's half-width, or -- tree form -- a bound on the near-field radius) */
    int rcap;                 /* widest near field taken for the sake of Humlicek region 1 */
    int tree_levels;          /* > 0: far field by the cell hierarchy (fine grids), this many coarse levels */
    int mom_terms;            /* moments per cell: 8, or -- tree form on sparse lines -- 12 (near field 3.95 |z|max
                                 instead of 7.8 |z|max); 0 means 8 in the one-pass form */
    int profile_tag;          /* != 0: time the line kernel under this tag (the two-pass gather under tag +
                                 GRT_TAG_FAR_OFFSET) */
    int near_block;           /* set by the plan: 64 where the tree form's gather shares its walk per wave -- near
                                 fields are then whole 64-point blocks (the halo leaves room for that); else 0 */
    int deterministic;        /* != 0 (GRT_DETERMINISTIC=1 / grt_set_deterministic): every floating-point sum in one fixed
                                 order, so that two runs agree to the last bit -- one wave of a workgroup takes all of its
                                 lines in store order, one line slice, and the two-pass form's first pass runs in
                                 tile_nphase launches of non-overlapping cell tiles.  A verification mode: ~4x slower. */
    unsigned long long *probe;     /* != NULL (grt_gas_optics_probe; cell-moment kernels only): an instrumented instance of the
                                 kernel runs and leaves 24 words per workgroup at record ((col L + layer) tiles + tile) nslice +
                                 slice: clock at entry, clock at exit, candidate lines, R | corrected << 16 | moments << 17,
                                 then sums over its waves of: 64-line blocks worked on, ring steps, near-centre points queued,
                                 moment reductions, lane-by-lane moment adds, region-1 correction steps, near-centre walk steps;
                                 word 11: clock when the prologue is done, 12: when every wave has left the line loop (the
                                 epilogue starts), 13: when the last wave left it; 14-21: clocks the waves spent in preparation,
                                 moment reduction and adds, near-centre walk and queue pushes, region-1 corrections, near
                                 field, the rest of the line loop, evaluating queued points, moment terms.  Zeroed by the caller. */
    int direct_near;          /* set by the plan (cell-moment forms): seven-point near fields (R = 3) by direct evaluation +
                                 row reduction instead of the ring */
    int tile_phase, tile_nphase;   /* set by the launcher: this launch takes cell tiles t with t % tile_nphase == tile_phase
                                 (tile_nphase <= 1: all of them) */
    uint32_t const *tile_ranges;   /* two-pass form, or NULL: [tiles][2] first / one-past-last line of the store whose centre can
                                 fall in cell tile t under any pressure shift up to the bound the host built the table for
                                 (a superset: the kernel decides membership line by line) -- spares every workgroup the
                                 search of the sorted store, ten dependent loads before its waves can start */
    int lean;                 /* set by the plan (two-pass form, single-level gather, lines.lean_a built for this grid): the
                                 first pass takes the lean fp32 form of the line loop wherever a workgroup's near fields are
                                 seven points wide (GRT_LEAN=0 in the environment switches it off: comparison runs) */
    uint32_t const *tile_items;    /* two-pass form, or NULL: the launch's work list [n_items][4] = {cell tile, first line, one past
                                 the last line, ordinal of this piece within its tile} in place of tiles x nslice equal slices --
                                 a tile that holds many lines appears in several pieces, a sparse one once (the host cuts by
                                 line count: a lone column of a band whose lines crowd into a few tiles, as real line lists'
                                 do, would otherwise be a few hundred long workgroups and thousands of short ones).  nslice is
                                 then 1 when no tile is cut and 2 when any is (moments and tau are added with atomics) */
    uint32_t n_items;
    GrtTableSpans spans;
    int *radius_table;        /* two-pass form, single-level gather, or NULL: [ncol][L][cell tiles] near-field radii of the first
                                 pass's cell tiles (near_radius), filled by the launcher before the gather, whose workgroups
                                 each look at the ten or so tiles they touch */
    int skip_tables;          /* != 0: leave the spectral tables' part (continua, CFC, CIA) out of tau: the caller adds it where
                                 it reads tau (the pipeline's fused solvers, GrtContinua) -- a table entry is then read once
                                 per grid point and column instead of once per layer as well */
    int narrow;               /* set by the plan (two-pass form, single-level gather): the band ends below 4 000 cm-1 (the
                                 longwave: Doppler widths far below the grid step), and the first pass takes its narrow-Doppler
                                 instance, whose ring and lean loop have a short form for waves in which only a line's OWN grid
                                 point can be anything but Lorentzian.  (The last field: no kernel argument moved with it.) */
} GrtGasOpticsArgs;

/* What a kernel needs to add the spectral tables' part of the gas optical depth itself (write_tile's expressions in
   write_tile's order, gas_optics_dev.h: tau + water-vapour continuum + the linear tables in ascending order). */
typedef struct GrtContinua
{
    double const *colstate;   /* [ncol][stride]: GrtColumnLayout's cont [L][GRT_MAX_TABLES] and h2o [L][4] blocks */
    uint64_t stride, off_cont, off_h2o;
    double const *tables;     /* [num_tables][nw] */
    double const *h2o_tables; /* [4][nw] or NULL */
    int num_tables, has_h2o_ctm;
    GrtTableSpans spans;
} GrtContinua;
/* tau_gas [ncol][L][nw] (column stride col_stride) += the tables' part: completes a tau the gas-optics launch wrote with
   skip_tables set (same doubles as without it) */
int grt_launch_add_continua(void *stream, GrtContinua const *c, int num_layers, int ncol, uint64_t nw,
                            double *tau_gas, uint64_t col_stride);


int grt_launch_gas_optics(void *stream, GrtGasOpticsArgs const *a);
/* HIP-event brackets on the library stream (grt_device.c; grt_ext.h: grt_profile_* and the tags, GRT_TAG_...) */
enum { GRT_TAG_FAR_OFFSET = 5 };    /* from a line kernel's tag (GRT_TAG_GAS_LW / _SW) to its far-field gather's (GRT_TAG_FAR_LW / _SW) */
int grt_profile_begin(void *stream, int tag);
void grt_profile_end(void *stream, int slot);
/* fast == 1 / 3: the cell-moment kernels (k_gas_optics_mp.hip), launched with the arguments as given; whether they apply
   to a grid and shape (no buffer pointer read), and whether the two-pass form's first pass can take the lean line loop */
int grt_launch_gas_optics_mp(void *stream, GrtGasOpticsArgs const *a);
int grt_gas_optics_mp_shape(GrtGasOpticsArgs const *a);
int grt_gas_optics_lean_shape(GrtGasOpticsArgs const *a);
/* which (group, layer-and-column index) workgroup b of a line-kernel launch of nb = ngroups*per_group workgroups takes:
   the kernels' own mapping (grt_work_order.h), compiled for the host (grt_gas_launch.c) */
void grt_work_order(unsigned nb, unsigned per_group, unsigned ngroups, unsigned b, unsigned *group, unsigned *rem);
int grt_tree_gather_by_wave(long long fsteps);   /* k_gas_optics_far.hip: the tree gather's near fields in 64-point blocks */
uint64_t grt_gas_optics_moment_floats(uint64_t nw, int levels, int terms);   /* per (column, layer) block of gmom */
double grt_gas_optics_moment_separation(int terms);   /* near field / |z|max that keeps the series' remainder at 7e-8 */

/* The RFM sweep methods (k_gas_optics_sweep.hip; kernels.c:135-406,514-581).  Per molecule: `prep` holds
   vnn, snn, gamma, alpha as [4][L][n] (grt_launch_line_prep); grt_launch_sweep_sort writes them sorted by
   shifted centre per layer (sort_lines); grt_launch_sweep adds the molecule to tau / bins.tau by method 0
   (wavenumber_sweep, needs sorted input) or 1 (line_sweep); grt_launch_sweep_interpolate finishes. */
typedef struct GrtSweepBins
{
    double w0, wres;
    uint64_t num_wpoints, n;
    int ppb, do_interp, do_last_interp;
    double const *w;        /* device (n, 3) */
    double *tau;            /* device (layer, n, 3) */
    uint64_t const *l, *r;  /* device (n) */
} GrtSweepBins;
int grt_launch_sweep_sort(void *stream, uint64_t n, int num_layers, double const *v0, double shift_max,
                          double const *lay, double const *prep, double *sorted);
int grt_launch_sweep(void *stream, int method, uint64_t n, int num_layers, double const *lines,
                     double const *ns, GrtSweepBins const *bins, double *tau);
int grt_launch_sweep_interpolate(void *stream, int num_layers, GrtSweepBins const *bins, double *tau);

/* Debug/parity hook: per-(layer,line) preparation only (kernels.c:34-131) and the
   integer window [s,e] of kernels.c:431-437 (s=1,e=0 when the line is skipped). */
int grt_launch_line_prep(void *stream, GrtGasOpticsArgs const *a, int col,
                         double *vnn, double *snn, double *gamma, double *alpha,
                         int64_t *win_s, int64_t *win_e);

/* Debug/parity hook: rfm_voigt_line_shape (RFM_voigt.c:85-281) for one line on n points, from the device functions the
   line kernels use; fast = 0 reference operation order, 1 fused arithmetic. */
int grt_launch_voigt_debug(void *stream, int fast, double w_start, uint64_t n, double wres, double center,
                           double gamma, double alpha, double *K_dev);

/* Debug/parity hook: the near-centre line shape at n given fp32 (x, y), by the variant of voigt_class / voigt_near the
   line kernels instantiate (0-4: see voigt_points_kernel); K before the scaling of RFM_voigt.c:278, cls the class chosen
   (-1: none).  Unknown variant or n == 0: hipErrorInvalidValue. */
int grt_launch_voigt_points(void *stream, int variant, uint64_t n, double const *x_dev, double const *y_dev,
                            double *K_dev, int *cls_dev);

/* Debug/parity hook: one device math function at n arguments.  op 0: grt_exp_pair (out0 = e^a, out1 = e^-a), 1: grt_exp,
   2: exp_fast, 3: exp_fp64, 4: reference_repwid (widened); out1 is written by op 0 alone.  Unknown op or n == 0:
   hipErrorInvalidValue. */
int grt_launch_device_math(void *stream, int op, uint64_t n, double const *a_dev, double *out0_dev, double *out1_dev);

/* rayleigh.c:29-68: n_layer [L] on the HOST (it travels as a kernel argument). */
int grt_launch_rayleigh(void *stream, int num_layers, double w0, double dw, uint64_t nw,
                        double const *n_layer_host, double *tau, double *omega, double *g);

/* optics.c:128-148: K objects, each [n]; pointers passed by value (K <= 8). */
typedef struct GrtOpticsPtrs { double const *tau[8]; double const *omega[8]; double const *g[8]; } GrtOpticsPtrs;
int grt_launch_add_optics(void *stream, uint64_t n, int num_optics, GrtOpticsPtrs const *in,
                          double *tau, double *omega, double *g);

/* ... any K: table_dev is a DEVICE array [3][K] of array pointers (tau, omega, g of each object) */
int grt_launch_add_optics_table(void *stream, uint64_t n, int num_optics, double const *const *table_dev,
                                double *tau, double *omega, double *g);

/* optics.c:306-321 */
int grt_launch_sample_optics(void *stream, uint64_t n, uint64_t factor, double *tau,
                             double *omega, double *g, double const *tau_in,
                             double const *omega_in, double const *g_in);

/* longwave.c:226-264.  Batched: column c uses tau/omega + c*optics_stride, temps at
   t_layers + c*L, t_levels + c*V, t_surf[c]; emis shared unless emis_stride != 0. */
typedef struct GrtLwArgs
{
    int num_levels, ncol;
    double w0, dw;
    uint64_t nw;
    double const *tau, *omega;      /* [ncol][L][nw]; omega may be NULL (treated as 0) */
    uint64_t optics_stride;
    double const *t_layers, *t_levels, *t_surf;
    double const *emis; uint64_t emis_stride;
    double *flux_up, *flux_down;    /* [ncol][V][nw]; NULL in the fused form: nothing spectral is stored (spectral six-row
                                       form: the six rows' bases, GRT_OUT_ROWS_POINTS) */
    uint64_t flux_stride;
    int user_level;                 /* -1: none */
    /* Fused clear-sky form (driver.c:360-424 + 285-356 with -integrated in one kernel, GRT_OUT_ROWS): the
       kernel forms Rayleigh (rayleigh.c:38-39) and the two-object combination (optics.c:138-145) per layer in
       registers from tau_gas [ncol][L][nw] (column stride optics_stride) and the air columns n_layer [ncol][L],
       and leave only the trapezoid partial sums of the six output rows (up TOA, up surface, up user, down TOA,
       down surface, down user) at partials[(c*6 + k)*nblocks + block]; grt_launch_reduce_partials finishes. */
    double const *tau_gas, *n_layer;
    double *partials;
    int add_continua;               /* fused form: tau_gas was written without the tables' part -- add it (continua) */
    GrtContinua continua;
    /* spectral form, GRT_OUT_LAYERS: scratch [ncol][6 L][nw].  The four streams' extinctions and the two effective
       Planck terms of every layer are worked out first by one thread per (layer, wavenumber), and the two sweeps read
       them (the same doubles through the same expressions: identical fluxes) -- see GrtSwArgs.layer_props */
    double *layer_terms;
} GrtLwArgs;
unsigned grt_solver_blocks(uint64_t nw);     /* workgroups along the spectrum of one solver launch (size of `partials`) */
int grt_launch_reduce_partials(void *stream, double const *partials, int nrows, unsigned nblocks,
                               double *out, int group, int out_stride, int out_offset);

/* shortwave.c:410-453 */
typedef struct GrtSwArgs
{
    int num_levels, ncol;
    uint64_t nw;
    double dw;
    double const *tau, *omega, *g;  /* [ncol][L][nw] */
    uint64_t optics_stride;
    double const *mu_dir;           /* [ncol] */
    double mu_dif;
    double const *alb_dir, *alb_dif; uint64_t alb_stride;
    double const *tsi;              /* [ncol] */
    double const *solar;            /* [nw] */
    double *flux_up, *flux_down; uint64_t flux_stride;   /* NULL in the fused form (spectral six-row form: as GrtLwArgs) */
    int user_level;
    /* fused clear-sky form, as in GrtLwArgs; the first sweep parks, per column, its downward-beam reflectances
       (2 V rows of nw) and the five properties of every layer (5 L rows) in park [ncol][2 V + 5 L][nw]: the second
       sweep reads the properties back instead of working them out again */
    double const *tau_gas, *n_layer;
    double w0;
    double *partials, *park;
    int add_continua;               /* as in GrtLwArgs */
    GrtContinua continua;
    /* fused form, no flux asked for between top and surface (user_level -1, 0 or num_levels - 1): ONE sweep from the top,
       nothing parked (k_shortwave.hip); 0: the two sweeps of the reference's order (GRT_SW_TWO_SWEEPS=1 in the environment) */
    int one_sweep;
    /* spectral form, GRT_OUT_LAYERS: scratch [ncol][5 L][nw].  The five properties of every
       layer are worked out first by one thread per (layer, wavenumber) -- a column of 50 000 wavenumbers is then 3 million
       independent delta-Eddington pairs instead of 50 000 chains of 120 -- and the two sweeps read them (the same
       doubles through the same expressions: identical fluxes) */
    double *layer_props;
} GrtSwArgs;
/* whether the fused form takes its one sweep (the rule above): the one expression, for the kernels on their own copies of
   the user level, the last level's index and the flag, and for the host on the arguments */
#define GRT_SW_ONE_SWEEP(user, last, one_sweep) (((user) < 0 || (user) == 0 || (user) == (last)) && (one_sweep))
static inline int grt_sw_one_sweep(GrtSwArgs const *a)
{
    return GRT_SW_ONE_SWEEP(a->user_level, a->num_levels - 1, a->one_sweep);
}

/* Profile form of the fused solvers (GRT_OUT_LEVELS, grt_pipeline_run_profiles): the fused form's arguments, but every
   level's upward and downward flux leaves as trapezoid partial sums, 2 V rows per column at
   partials[(c*2 V + r)*nblocks + block], r = level (up) and V + level (down), levels top first; reduced with
   grt_launch_reduce_partials(nrows = ncol*2 V).  The shortwave form always takes the two sweeps and needs `park`
   (one_sweep and user_level are not read); each wave sums a level as the sweep produces it, in dynamic LDS of
   2 V x 2 doubles per workgroup.  Rows 0, L and user_level are, bit for bit, the six-row form's (the shortwave's: its
   two-sweep form's). */
/* levels [ncol][sets][4][V] (up, down of band 0, then of band 1) -> heating [ncol][sets][2][V-1] K day-1 (NULL: not
   formed) from the level pressures pressure [ncol][V] mb, and fluxes [ncol][sets][12] (NULL: not formed) in
   grt_pipeline_run's layout; the rows of a band whose bit in `bands` is clear are zeroed, level fluxes included, in every
   set.  sets = 1: grt_pipeline_run_profiles; 2: grt_pipeline_run_allsky_profiles (clear sky, then all-sky); up to
   GRT_PROFILE_MAX_SETS: grt_pipeline_run_sky. */
#define GRT_PROFILE_MAX_SETS 4          /* grt_ext.h: GRT_SKY_MAX_SETS */
int grt_launch_profile_finish(void *stream, int ncol, int sets, int num_levels, int bands, int user_level, double gravity,
                              double cp, double const *pressure, double *levels, double *heating, double *fluxes);

/* All-sky form of the fused solvers (clouds joined, grt_pipeline_run_allsky): the fused form's arguments (six-row
   partial sums), and per layer the liquid and ice cloud objects formed in registers from the band tables below and combined with
   gas and Rayleigh by allsky_combine (optics_dev.h).  band_liquid / band_ice: DEVICE [nw] band of each grid point, -1 for
   none; thickness [ncol][L] m; liquid / ice [ncol][3][num_bands][L] (extinction m-1, albedo, asymmetry).
   With GRT_OUT_LEVELS (grt_pipeline_run_allsky_profiles): the same cloud objects in the profile form -- its
   partial sums, dynamic LDS and, shortwave, its two sweeps and park block; the cloud tables are read in the first sweep
   only. */
typedef struct GrtCloudArgs
{
    int num_bands;
    int const *band_liquid, *band_ice;
    double const *thickness;
    double const *liquid, *ice;
} GrtCloudArgs;
static inline int grt_cloud_args_ok(GrtCloudArgs const *c)
{
    return c != NULL && c->num_bands >= 1 && c->band_liquid != NULL && c->band_ice != NULL && c->thickness != NULL &&
           c->liquid != NULL && c->ice != NULL;
}

/* Aerosol form of the fused solvers (aerosols joined, six rows or every level; grt_pipeline_run_aerosols): the
   fused or the profile form's arguments, and per layer the aerosol object formed in registers and combined with gas and
   Rayleigh by aerosol_combine (optics_dev.h).  The aerosol's tau, omega, g are given per layer on a coarse wavenumber grid
   of NA points and put on the spectral grid by the reference's linear_sample (utilities.c:235-246): the host turns each
   interval's two points into a slope and an intercept once, and a grid point evaluates slope w + intercept.
   interval: DEVICE [nw], the interval j of each grid point (x[j] < w <= x[j+1]), -1 for a point outside the aerosol grid
   (no aerosol there); tables: DEVICE [ncol][3][num_intervals][2][L] (tau, omega, g; slope then intercept): a thread's walk
   over the layers is contiguous, and the lanes of a wave that share an interval read the same addresses. */
typedef struct GrtAerosolArgs
{
    int num_intervals;              /* NA - 1 >= 1 */
    int const *interval;
    double const *tables;
} GrtAerosolArgs;
static inline int grt_aerosol_args_ok(GrtAerosolArgs const *c)
{
    return c != NULL && c->num_intervals >= 1 && c->interval != NULL && c->tables != NULL;
}

/* Materialised form: the aerosol object of the same tables spread onto the grid, [ncol][L][nw] each (zero where a point
   has no interval). */
int grt_launch_spread_aerosols(void *stream, int num_layers, int ncol, double w0, double dw, uint64_t nw,
                               GrtAerosolArgs const *c, double *tau, double *omega, double *g);

/* grt_pipeline_set_surface: a surface property (emissivity, direct or diffuse albedo) of every column on the band's grid,
   rows [ncol][nw], as interpolate_to_grid(..., linear_sample, constant_extrapolation) puts a column's NS knots there
   (utilities.c:149-246, :77-92).  The host turns a column's knots into num_entries = NS + 1 slope and intercept pairs --
   entry 0: (0, y[0]) for w <= x[0]; entry 1 + j: interval j, x[j] < w <= x[j+1]; entry NS: (0, y[NS-2]) for w > x[NS-1]
   (the reference's value there) --, so every point evaluates slope w + intercept.  entry: DEVICE [nw], each grid point's
   entry, every value in 0 .. num_entries - 1; tables: DEVICE [ncol][num_entries][2]. */
typedef struct GrtSurfaceArgs
{
    int num_entries;                /* NS + 1 >= 3 */
    int const *entry;
    double const *tables;
} GrtSurfaceArgs;
static inline int grt_surface_args_ok(GrtSurfaceArgs const *c)
{
    return c != NULL && c->num_entries >= 3 && c->entry != NULL && c->tables != NULL;
}
/* A sun cosine per layer for the direct beam of a zenith instance (grt_pipeline_run_sky_zeniths_slant: the pseudo-spherical
   approximation): joined behind a GrtZenithArgs, the row of column c under angle k uses, in layer j (top layer first),
   mu_layer[(c zeniths + k) L + j] wherever its direct-beam solution uses the row's cosine -- eddington<true>, its gamma3,
   the optical-depth clamp, T_pure and so the running direct beam.  The diffuse solution, the sweeps, the level expressions
   and the flux scale solar x mu[c zeniths + k] stay the row's.  A night row (mu <= 0) reads none of its entries.  The index
   is uniform per workgroup: scalar loads.  A slant instance always carries a GrtDirectArgs.
   mu_layer: DEVICE [ncol][zeniths][L], each day entry in (0, 1]. */
typedef struct GrtZenithSlantArgs
{
    double const *mu_layer;
} GrtZenithSlantArgs;
static inline int grt_zenith_slant_args_ok(GrtZenithSlantArgs const *c)
{
    return c != NULL && c->mu_layer != NULL;
}
int grt_launch_spread_surface(void *stream, int ncol, double w0, double dw, uint64_t nw, GrtSurfaceArgs const *c,
                              double *rows);

/* Subcolumn form of the two all-sky forms (subcolumns joined in place of clouds, six rows or every level;
   grt_pipeline_run_subcolumns): one launch solves subcolumns first .. first + count - 1 of every column, a->ncol columns of
   gas state (tau_gas, n_layer, temperatures, sun, continua) and `subcolumns` cloud draws per column.  Row y of the grid
   is column c = y / count, subcolumn s = first + y % count, so that the draws of one column run next to each other and
   share its tau_gas in the caches.  clouds.liquid / .ice hold the tables subcolumn-major, [subcolumns][ncol][3][B][L]
   (draw s of column c at (s ncol + c) 3 B L); thickness stays [ncol][L].  Partial sums go to the slot c subcolumns + s
   (six-row: partials[((c S + s) 6 + k) nblocks + block]; profile: [((c S + s) 2 V + r) nblocks + block]); the shortwave's
   park block is indexed by y: the two-sweep forms need it for ncol x count columns.  grt_launch_subcolumn_mean reduces. */
typedef struct GrtSubcolumnArgs
{
    GrtCloudArgs clouds;
    int subcolumns, first, count;
} GrtSubcolumnArgs;
static inline int grt_subcolumn_args_ok(GrtSubcolumnArgs const *sc)
{
    return sc != NULL && grt_cloud_args_ok(&sc->clouds) && sc->subcolumns >= 1 && sc->count >= 1 && sc->first >= 0 &&
           sc->first + sc->count <= sc->subcolumns;
}

/* Zenith form of the two clear-sky fused forms (zeniths joined, six rows or every level; grt_pipeline_run_zeniths): one
   launch solves sun angles first .. first + count - 1 of every column on the column's one tau_gas.  Row y of the grid is
   column c = y / count, angle k = first + y % count, as the subcolumn form maps its rows: the row reads mu[c zeniths + k]
   in place of GrtSwArgs.mu_dir, leaves its partial sums at the slot c zeniths + k and parks at y.  A row whose mu <= 0 is a
   night sample: +0.0 partial sums, nothing solved.  Shortwave only.  grt_launch_zenith_mean reduces.
   With aerosols, subcolumns or both joined as well (grt_pipeline_run_sky_zeniths: the sets of grt_pipeline_run_sky under
   the angles): the aerosol table stays the column's; with subcolumns one launch solves subcolumns->count draws times
   zeniths->count angles of every column, row y is column c = y / (draws x angles), draw s and angle k from the remainder
   (the angles of a draw next to each other), the row reads mu[c zeniths + k] and the draw's cloud tables, leaves its partial
   sums at the slot (c zeniths + k) subcolumns + s and parks at y.  grt_launch_sky_zenith_mean reduces. */
typedef struct GrtZenithArgs
{
    double const *mu;               /* DEVICE [ncol][zeniths] */
    int zeniths, first, count;
} GrtZenithArgs;
static inline int grt_zenith_args_ok(GrtZenithArgs const *z)
{
    return z != NULL && z->mu != NULL && z->zeniths >= 1 && z->count >= 1 && z->first >= 0 &&
           z->first + z->count <= z->zeniths;
}
/* The direct-beam albedo of every (column, angle) of a zenith instance (grt_pipeline_run_sky_zeniths_direct): joined behind
   a GrtZenithArgs, the row of column c under angle k reads, in place of a->alb_dir, slope w + intercept of entry
   entry[i] of tables[(c zeniths + k) num_entries ..] -- GrtSurfaceArgs' entries and pairs (grt_surface_entry_map,
   grt_surface_tables over ncol x zeniths knot rows), evaluated per thread as grt_launch_spread_surface evaluates them
   (multiply, then add: the same double), so no [ncol][zeniths][nw] rows exist.  The diffuse albedo stays a->alb_dif.
   entry: DEVICE [nw]; tables: DEVICE [ncol][zeniths][num_entries][2]. */
typedef struct GrtZenithSurfaceArgs
{
    int num_entries;                /* NS + 1 >= 3 */
    int const *entry;
    double const *tables;
} GrtZenithSurfaceArgs;
static inline int grt_zenith_surface_args_ok(GrtZenithSurfaceArgs const *c)
{
    return c != NULL && c->num_entries >= 3 && c->entry != NULL && c->tables != NULL;
}
/* The shared-layer kernel of the zenith form (k_shortwave.hip: sw_zenith_kernel), six rows in one sweep
   (grt_sw_one_sweep(a) must hold: hipErrorInvalidValue otherwise): grid row y is column y / chunks and the
   GRT_ZENITH_CHUNK consecutive angles from (y % chunks) GRT_ZENITH_CHUNK on, chunks = ceil(zeniths / GRT_ZENITH_CHUNK);
   a thread forms a layer's optics, delta-scaling and diffuse Eddington solution once and the direct-beam solution per
   angle.  Every angle's partial sums are, bit for bit, the zenith instance's of GRT_OUT_ROWS (z's first and count are not
   read: one launch takes every angle).  sc, ae (either may be NULL): the kernel's instance with the draws of sc, the
   aerosol object or both joined, as the zenith instances join them -- grid row y is then (column, draw first + .. of
   sc->count, chunk), the chunks of a draw next to each other, at most 65 535 rows, and the partial sums lie at the slot
   (c zeniths + k) subcolumns + s.  d, zs (either may be NULL; grt_pipeline_run_sky_zeniths_direct): the instances that
   also leave every angle's direct beam at the top and the surface (GrtDirectArgs: three rows at the angle's slot, riding
   with its six), that read every angle's own direct albedo (GrtZenithSurfaceArgs), or both, behind each of the four
   joins.  Each instance carries the most angles of {2, 4} that leave it three waves per SIMD and no scratch
   (DESIGN.md 3.3); grt_zenith_chunk names an instance's -- GRT_ZENITH_CHUNK_DIRECT, _SURFACE and _DIRECT_SURFACE are the
   chunks of the instances with d, zs and both, the same behind each of the four joins.  sl (or NULL;
   grt_pipeline_run_sky_zeniths_slant; d must be set with it): the instances whose direct beam reads a cosine per layer
   (GrtZenithSlantArgs), with zs or without, behind each of the four joins: GRT_ZENITH_CHUNK_SLANT_SURFACE and
   GRT_ZENITH_CHUNK_SLANT. */
#define GRT_ZENITH_CHUNK 4
#define GRT_ZENITH_CHUNK_AEROSOLS 4
#define GRT_ZENITH_CHUNK_SUBCOLUMNS 4
#define GRT_ZENITH_CHUNK_SUBCOLUMNS_AEROSOLS 4
#define GRT_ZENITH_CHUNK_DIRECT 4
#define GRT_ZENITH_CHUNK_SURFACE 4
#define GRT_ZENITH_CHUNK_DIRECT_SURFACE 4
#define GRT_ZENITH_CHUNK_SLANT 4
#define GRT_ZENITH_CHUNK_SLANT_SURFACE 4
struct GrtDirectArgs;
int grt_zenith_chunk(GrtSubcolumnArgs const *sc, GrtAerosolArgs const *ae, struct GrtDirectArgs const *d,
                     GrtZenithSurfaceArgs const *zs, GrtZenithSlantArgs const *sl);
int grt_launch_sw_zeniths(void *stream, GrtSwArgs const *a, GrtZenithArgs const *z, GrtSubcolumnArgs const *sc,
                          GrtAerosolArgs const *ae, struct GrtDirectArgs const *d, GrtZenithSurfaceArgs const *zs,
                          GrtZenithSlantArgs const *sl);
/* The weighted mean over a column's angles of one output row, in a fixed order, and every angle's own rows: for column c
   and row r (of `rows` per slot) each angle's blocks are added as grt_launch_reduce_partials adds them -- an angle whose
   mu [ncol][zeniths] is <= 0 counts as +0.0 whatever its partial sums hold -- and stored at per_angle[(c zeniths + k) rows
   + r] (per_angle NULL: not stored); then the angles k = 0 .. zeniths - 1 in order, each times weight[c zeniths + k], the
   product rounded before it is added -- weight NULL: the plain sum, then one division by zeniths --, to
   out[c out_stride + out_offset + r] (out NULL: not formed).  zeniths = 1 without weights gives
   grt_launch_reduce_partials' bits.  six (or NULL; rows = 2 V, a column's up then down levels): every angle's six rows of
   grt_pipeline_run's layout as well, [ncol][zeniths][6], from its level rows 0, V - 1 and user_level. */
int grt_launch_zenith_mean(void *stream, double const *partials, int ncol, int zeniths, int rows, unsigned nblocks,
                           double const *mu, double const *weight, double *per_angle, double *six, int user_level,
                           double *out, int out_stride, int out_offset);
/* grt_pipeline_run_sky_zeniths' mean of one set: grt_launch_zenith_mean over partial sums that hold `subcolumns` draws per
   angle, at the slot (c zeniths + k) subcolumns + s, and with the set dimension in the per-angle outputs.  For column c,
   row r and angle k: each draw's blocks are added as grt_launch_reduce_partials adds them, the draws s = 0 .. S - 1 in
   order, then -- S > 1 -- one division by S, as grt_launch_subcolumn_mean does; a night angle counts as +0.0; stored at
   per_angle[((c sets + set) zeniths + k) rows + r] (NULL: not stored) and, rows = 2 V, the angle's six rows at
   six[((c sets + set) zeniths + k) 6 ..] (NULL: not stored); then the angles fold as in grt_launch_zenith_mean, to
   out[c out_stride + out_offset + r] (NULL: not formed).  subcolumns = 1 and sets = 1: grt_launch_zenith_mean's bits. */
int grt_launch_sky_zenith_mean(void *stream, double const *partials, int ncol, int zeniths, int subcolumns, int rows,
                               unsigned nblocks, double const *mu, double const *weight, double *per_angle, double *six,
                               int sets, int set, int user_level, double *out, int out_stride, int out_offset);

/* Surface-tile form of the two fused six-row forms (grt_pipeline_run_sky_tiles): `tiles` surfaces per column on the column's
   one atmosphere.  lw_tile_kernel (k_longwave.hip) and sw_tile_kernel (k_shortwave.hip) take the six-row instance's
   arguments and, as joins, nothing, a GrtAerosolArgs, a GrtSubcolumnArgs or a GrtAerosolArgs behind a GrtSubcolumnArgs
   (one draw per column is a GrtSubcolumnArgs of one subcolumn: the same tables, the same doubles).  Grid rows (y) are the
   instance's -- a column, or (column, draw first + .. of count) --, and blockIdx.z is a chunk of TN consecutive tiles,
   chunk_first + z: a thread does everything that does not see the surface once -- the longwave's downward sweep and, on
   the way up, a layer's optical depth, Planck terms and four extinctions; the shortwave's layer properties and whichever
   of its sweeps carry no albedo -- and the surface's part per tile, each in lw_kernel's / sw_kernel's expressions and
   order on the same doubles, so every tile's partial sums are, bit for bit, the six-row instance's with that tile's rows
   and temperature, at the slot (c tiles + t) subcolumns + s.  Tiles past the column's last are skipped by a flag that is
   uniform per workgroup.  The shortwave takes sw_kernel's rule for one sweep or two; its two-sweep form parks the layer
   properties in sw_kernel's fused layout at park row z gridDim.y + y (no per-tile rows are parked), so a launch's
   rows x chunk_count must fit the park block.
   t_surf: DEVICE [ncol][tiles] (longwave).  rows: DEVICE [ncol][tiles][nw], the tiles' emissivity (longwave) or direct
   albedo (shortwave) on the band's grid, as grt_launch_spread_surface writes them; NULL: every tile takes the instance's
   own (a->emis / a->alb_dir, a->alb_dif).  rows_dif: the diffuse albedo, or NULL: the direct one.
   Each instance carries the most tiles of {2, 4, 8} that leave it three waves per SIMD and no scratch in both bands
   (DESIGN.md 3.3); grt_tile_chunk names an instance's. */
typedef struct GrtTileArgs
{
    int tiles;                      /* T >= 1 */
    int chunk_first, chunk_count;   /* the launch's chunks: gridDim.z = chunk_count */
    double const *t_surf;
    double const *rows, *rows_dif;
} GrtTileArgs;
#define GRT_TILE_CHUNK 4
#define GRT_TILE_CHUNK_AEROSOLS 4
#define GRT_TILE_CHUNK_SUBCOLUMNS 4
#define GRT_TILE_CHUNK_SUBCOLUMNS_AEROSOLS 4
static inline int grt_tile_args_ok(GrtTileArgs const *t, int chunk)
{
    return t != NULL && t->tiles >= 1 && t->chunk_first >= 0 && t->chunk_count >= 1 &&
           (t->chunk_first + t->chunk_count - 1)*chunk < t->tiles && (t->rows != NULL || t->rows_dif == NULL);
}
int grt_tile_chunk(GrtSubcolumnArgs const *sc, GrtAerosolArgs const *ae);
int grt_launch_lw_tiles(void *stream, GrtLwArgs const *a, GrtTileArgs const *t, GrtSubcolumnArgs const *sc,
                        GrtAerosolArgs const *ae);
int grt_launch_sw_tiles(void *stream, GrtSwArgs const *a, GrtTileArgs const *t, GrtSubcolumnArgs const *sc,
                        GrtAerosolArgs const *ae);
/* grt_pipeline_run_sky_tiles' mean of one band of one set, in a fixed order: for column c, row r (of 6) and tile t each
   draw's blocks are added as grt_launch_reduce_partials adds them, the draws s = 0 .. S - 1 in order, then -- S > 1 -- one
   division by S, as grt_launch_subcolumn_mean does; stored at per_tile[(((c sets + set) tiles + t) 12 + 6 band + r]
   (NULL: not stored); then the tiles t = 0 .. tiles - 1 in order, each times fraction[c tiles + t], the product rounded
   before it is added -- fraction NULL: the plain sum, then one division by tiles --, to out[c out_stride + out_offset + r]
   (NULL: not formed).  One wavefront per (column, row).  tiles = 1 without fractions: grt_launch_subcolumn_mean's bits. */
int grt_launch_tile_mean(void *stream, double const *partials, int ncol, int tiles, int subcolumns, unsigned nblocks,
                         double const *fraction, double *per_tile, int sets, int set, int band, double *out,
                         int out_stride, int out_offset);

/* Direct-beam form of the shortwave's fused six-row and profile forms (direct joined, with any of the cloud and aerosol
   joins or none; grt_pipeline_run_sky_direct): the instance's arguments, sweeps and partial sums, and beside them the
   direct beam of the sweep -- the running product of the layers' T_pure (shortwave.c:306, :323), scaled as the other rows
   are -- at the same levels, as trapezoid partial sums of its own: three rows per slot (TOA, surface, user level) at
   partials[(slot 3 + k) nblocks + block] in the six-row form, V rows per slot (levels top first) at
   partials[(slot V + level) nblocks + block] in the profile form, slot as the instance's own partial sums have it.  The
   three (V) rows ride with the six (2 V) through the same wave and workgroup sums: rows 0, L and user_level of the
   profile form are, bit for bit, the six-row form's three, in its one sweep and in its two.  The profile form's dynamic
   LDS is 3 V x 2 doubles per workgroup.  Shortwave only; reduced as the instance's own rows are.  Behind a GrtZenithArgs
   (grt_pipeline_run_sky_zeniths_direct: with a GrtZenithSurfaceArgs between them, or without) the slot is the zenith
   instance's, (c zeniths + k) subcolumns + s, a night sample's rows are +0.0, and grt_launch_sky_zenith_mean reduces. */
typedef struct GrtDirectArgs
{
    double *partials;
} GrtDirectArgs;
static inline int grt_direct_args_ok(GrtDirectArgs const *d)
{
    return d != NULL && d->partials != NULL;
}
/* Materialised form: the same direct beam from the tau, omega, g a pass has left on the grid (GrtSwArgs: tau, omega, g,
   optics_stride, mu_dir, tsi, solar), one thread per column and grid point walking the layers with the solver's own
   T_pure; direct [ncol][V][nw], levels top first, W m-2 per cm-1. */
int grt_launch_sw_direct_beam(void *stream, GrtSwArgs const *a, double *direct);
/* rows [n][3] (TOA, surface, user level; +0.0 with user_level < 0) from levels [n][V] */
int grt_launch_direct_rows(void *stream, int n, int num_levels, int user_level, double const *levels, double *rows);

/* Surface-temperature Jacobian form of the longwave's fused six-row and profile forms (jacobian joined, with any of the
   cloud and aerosol joins or none; grt_pipeline_run_sky_jacobian): the instance's arguments, sweeps and partial sums, and
   beside them dF_up/dT_surf of the upward sweep at the same levels.  The surface enters each stream once
   (longwave.c:202), D_s = emis dB/dT(T_surf, w) there, every layer above multiplies D_s by the stream's extinction, and
   a level's value is ((0 + c2[0] D_0) + c2[1] D_1) + c2[2] D_2) + c2[3] D_3; dB/dT = B (x/T) e/(e - 1), x = c2 w/T, e =
   exp(x), and 0 where planck() clamps x.  It leaves as the direct beam of the shortwave does (GrtDirectArgs): three rows
   per slot (TOA, surface, user level) at partials[(slot 3 + k) nblocks + block] in the six-row form, V rows per slot at
   partials[(slot V + level) nblocks + block] in the profile form, through the same wave and workgroup sums -- rows 0, L
   and user_level of the profile form are, bit for bit, the six-row form's three.  The profile form's dynamic LDS is 3 V x
   2 doubles per workgroup.  Longwave only; reduced as the instance's own rows are. */
typedef struct GrtJacobianArgs
{
    double *partials;
} GrtJacobianArgs;
static inline int grt_jacobian_args_ok(GrtJacobianArgs const *d)
{
    return d != NULL && d->partials != NULL;
}
/* Materialised form: the same Jacobian from the tau, omega a pass has left on the grid (GrtLwArgs: tau, omega,
   optics_stride, t_surf, emis), one thread per column and grid point walking the layers upward from the surface with
   the solver's own extinctions; jacobian [ncol][V][nw], levels top first, W m-2 K-1 per cm-1. */
int grt_launch_lw_surface_jacobian(void *stream, GrtLwArgs const *a, double *jacobian);

/* Longwave radiances at viewing angles (grt_pipeline_run_sky_radiances): a kernel of its own, lw_radiance_kernel, beside
   the solver of a pass, on the pass's GrtLwArgs exactly as that solver gets it (fused form: tau_gas, n_layer and the
   continua it may have to add; materialised form: the tau, omega the pass has left on the grid).  The four streams of the
   solver are radiances at the secants -c1[s]; a radiance at secant m is the same recurrence with c1[s] replaced by -m:
   per grid point t_j = tau_j (1 - omega_j), e_j = exp(min((-m) t_j, 700)), downward from I = 0 with I <- (1 - e_j) P_j +
   I e_j, the surface I <- emis B(T_surf) + (1 - emis) I, and upward the same step; what leaves is the upward radiance at
   the top and the downward one at the surface, W m-2 sr-1 per cm-1.  One thread per (grid point, grid row, chunk of up to
   GRT_RADIANCE_CHUNK angles): the block is GRT_SOLVER_BLOCK, grid row y is the solver instance's (a column, or a column
   and cloud draw: grt_solver_grid_rows), the chunk is blockIdx.z; a layer's optics and Planck terms are formed once and
   shared by the chunk's angles, whose intensities stay in registers.  The padding angles of a last chunk repeat the last
   real secant and write nothing.
   secant: DEVICE [ncol][angles].  partials: the trapezoid partial sums [slot][angles][2][nblocks] (up at the top, then
   down at the surface; idle lanes weigh 0), slot = the solver instance's (column, or column x subcolumns + draw; the
   materialised form: column x subcolumns + draw with this struct's two fields), finished by grt_launch_reduce_partials
   or grt_launch_subcolumn_mean on angles x 2 rows.  spectral, brightness (either may be NULL; one draw per column only):
   the radiances and their brightness temperatures T_b = c2 w / log1p(c1 w^3 / I) (planck()'s constants; +0.0 where I <=
   0) of column c at base + c col_stride + (k 2 + d) nw + i: a wave writes 64 consecutive points of one row. */
#define GRT_RADIANCE_CHUNK 4
typedef struct GrtRadianceArgs
{
    double const *secant;
    int angles;
    int subcolumns, draw;           /* materialised form: the slot is column x subcolumns + draw */
    double *partials;
    double *spectral, *brightness;
    uint64_t col_stride;
} GrtRadianceArgs;
static inline int grt_radiance_args_ok(GrtRadianceArgs const *r)
{
    return r != NULL && r->secant != NULL && r->angles >= 1 && r->partials != NULL && r->subcolumns >= 1 && r->draw >= 0 &&
           r->draw < r->subcolumns;
}

/* ---- The window table (grt_window_table, host; Window, optics_dev.h) ----
   A window is the grid points first .. first + count - 1 with a weight each, at weights + its weight offset.  Instrument
   channels (GrtChannelArgs) and spectral responses (GrtResponseArgs) are windows; they overlap freely, so a 128-point
   solver block has an explicit list of its windows, not a range.  A (window, block) pair is a window and a block it has a
   point in: pair = the window's first pair + block - its first block.  One device allocation holds the doubles first --
   every window's weights, then what the kind adds --, then the ints:
     entry [count][GRT_WINDOW_INTS]   per window: first point, count, weight offset, first block, first pair;
     block_start [nblocks + 1]        where block b's list starts in block_list;
     block_list [pairs]               the windows of block 0, of block 1, ...: each list in ascending order. */
#define GRT_WINDOW_INTS 5

/* Instrument channels of those radiances (grt_pipeline_run_sky_channels): the channel form of lw_radiance_kernel, the
   radiance form with a GrtChannelArgs last in its joins.  The channels are the windows of a window table, W_c the weights
   of channel c.  After the upward sweep a workgroup forms, per channel of its block's list, real angle and row, sum_i W_c(i) value(i) over its 128 points -- a lane
   outside the channel's span or past the grid weighs 0; WAVE_SUM, then the two waves in order, as block_partials adds a
   row; a wave that holds no point of the channel adds +0.0 without the tree -- and stores it at partials[((slot angles +
   angle) 2 + row) pairs + pair]: a channel's sums depend on its own weights and the grid alone.  Behind the weights
   the table's doubles hold sum_w [C] (summed in index order) and center [C] (the caller's, or the centroid sum W w / sum W).
   grt_launch_channel_finish (channel_finish_kernel): one thread per (column, angle, row, channel); per draw s = 0 .. S - 1
   in order the channel's pairs in block order, then -- S > 1 -- one division by S, one by sum_w, stored at out[c
   out_stride + out_offset + (angle 2 + row) C + channel]; brightness (or NULL): T = c2 v / log1p(c1 v^3 / R) at v =
   center, +0.0 where R <= 0, at the same place. */
typedef struct GrtChannelArgs
{
    int channels;                   /* C */
    uint64_t pairs;                 /* P */
    int const *entry;               /* DEVICE [C][GRT_WINDOW_INTS] */
    int const *block_start;         /* DEVICE [nblocks + 1] */
    int const *block_list;          /* DEVICE [P] */
    double const *weights;          /* DEVICE [the channels' points] */
    double const *sum_w, *center;   /* DEVICE [C] each */
    double *partials;               /* DEVICE [slot][angles][2][P] */
} GrtChannelArgs;
static inline int grt_channel_args_ok(GrtChannelArgs const *c)
{
    return c != NULL && c->channels >= 1 && c->pairs >= 1 && c->entry != NULL && c->block_start != NULL &&
           c->block_list != NULL && c->weights != NULL && c->sum_w != NULL && c->center != NULL && c->partials != NULL;
}

/* Channel transmittance profiles and contribution functions of the upward radiance at the top
   (grt_pipeline_run_sky_weighting): lw_weighting_kernel, behind the channel form of lw_radiance_kernel on that launch's
   arguments, instance and grid.  It makes the downward sweep only.  Per grid point and angle of the chunk, with e_j the
   layer's extinction at the viewing secant: T_0 = 1, T_{j+1} = T_j e_j (level to space); K_j = ((1 - e_j) P_j) T_j, P_j
   the upward sweep's effective Planck term; the downward radiance steps as lw_radiance_kernel's; after the last layer
   K_L = (emis B(T_surf)) T_L and K_{L+1} = ((1 - emis) I_dn) T_L.  The reduction is a gather through LDS: per layer every
   thread writes its point's T_j and K_j of each real angle to a tile [quantity][angle][point] (two tiles in turn, one
   barrier a layer); then the workgroup's threads take the channels of the block's list in turn and each adds, per real
   angle and quantity, W_c(i) value(i) over the channel's points inside the block in ascending point index, one sequential
   sum from +0.0 each, and stores it at partials[((slot angles + angle) R + row) pairs + pair], the pair of
   GrtChannelArgs' table.  Points outside a channel's span and idle lanes are never read.  Rows: R = (transmittance ? V :
   0) + (contribution ? V + 1 : 0), the V transmittance rows (level 0 .. V - 1) first where both are asked for.
   grt_launch_weighting_finish: one thread per (column, angle, row, channel), the channel fastest; per draw s = 0 .. S - 1
   in order the channel's pairs in block order, then -- S > 1 -- one division by S, one by sum_w; row r of the
   transmittances at transmittance[c t_stride + t_offset + (angle V + r) C + channel], of the contributions at
   contribution[c k_stride + k_offset + (angle (V + 1) + r) C + channel].  c->partials is not read by either launch. */
typedef struct GrtWeightingArgs
{
    int transmittance, contribution;    /* which of the two row groups leave (not both 0) */
    double *partials;                   /* DEVICE [slot][angles][R][P] */
} GrtWeightingArgs;
static inline int grt_weighting_rows(GrtWeightingArgs const *w, int num_levels)
{
    return (w->transmittance ? num_levels : 0) + (w->contribution ? num_levels + 1 : 0);
}
static inline int grt_weighting_args_ok(GrtWeightingArgs const *w)
{
    return w != NULL && (w->transmittance || w->contribution) && w->partials != NULL;
}

/* Banded profile form of the two profile forms (GRT_OUT_LEVEL_BINS, clear sky or clouds joined;
   grt_pipeline_run_band_profiles): the profile form's arguments, sweeps and park block, but every level's
   flux leaves once per wavenumber bin that has a point in the workgroup's 128 grid points.  A point weights a level's
   value with the trapezoid weight of the bin (grt_launch_bin_rows' rule: dw inside, dw/2 at the bin's two edges, 0
   elsewhere and for idle lanes); a workgroup inside one bin -- all but the few that hold an edge -- does exactly the
   profile form's work, one wave sum per level and direction; one that holds edges repeats the wave sum for each of its
   bins.  Partial sums go where grt_bin_table places them, partials[(c*2 V + r)*per_row + offset(b) + block -
   first_block(b)], r = level (up) and V + level (down); grt_launch_bin_reduce finishes.  Dynamic LDS: block_bins x 2 V x
   2 doubles, block_bins = grt_bin_block_max of the edges.  The single bin {0, nw - 1} gives the profile form's partial
   sums, bit for bit. */
typedef struct GrtBandArgs
{
    int num_bins;
    int block_bins;                 /* the most bins with a point in one workgroup: sizes the dynamic LDS */
    int const *table;               /* DEVICE: grt_bin_table's ints */
    uint64_t per_row;               /* partial sums per row (grt_bin_table's return value) */
} GrtBandArgs;
static inline int grt_band_args_ok(GrtBandArgs const *bn)
{
    return bn != NULL && bn->num_bins >= 1 && bn->block_bins >= 1 && bn->table != NULL && bn->per_row >= 1;
}

/* Response form of the two profile forms (GRT_OUT_LEVELS with any of the cloud and aerosol joins or none, the shortwave's
   always together with `direct`; grt_pipeline_run_sky_weighted): the profile form's arguments, sweeps, park block and
   partial sums -- the broadband rows are summed exactly as without it --, and beside them every level's rows under
   spectral response functions.  The responses are the windows of a window table (above GrtChannelArgs), r_k
   the weights of response k: not normalised, any finite sign, and the table's only doubles.  A workgroup stages t_i r_k(i) -- t_i the band's trapezoid weight, 0
   for idle lanes and outside the response's span -- for the responses of its block's list in dynamic LDS, [responses of
   the block][128], once at kernel start; every level's value x then leaves once more per response of the list as the
   wave sums of x (t r), in its own group of G V rows behind the broadband group (G = 2: up, down; 3 with the third row
   group), and finish() stores the list's sums at partials[(slot P + pair) G V + row], row = level (up), V + level (down),
   2 V + level (third group): without atomics, a fixed place per (slot, response, row, block).  A workgroup whose list is
   empty does exactly the profile form's work.  Dynamic LDS: (1 + block_max) G V x 2 doubles of wave sums and block_max x
   128 doubles of weights.
   grt_launch_response_rows: the materialised form's twin -- the same weights, wave and workgroup sums on rows [slots][G]
   [V][nw] the spectral solvers (and the direct-beam kernel) left on the grid, row group g of slot c at rows[g] + c V nw,
   to the same partial sums.
   grt_launch_response_finish: one thread per output row (column, response, row of the G V): per draw s = 0 .. S - 1 in
   order the response's blocks in the association grt_launch_reduce_partials has for that many blocks, then one division by
   S as grt_launch_subcolumn_mean's, to out[c out_stride + out_offset + (k G + g) V + level].
   grt_launch_actinic_rows: from finished shortwave rows [n][R][3][V] (row group stride `stride` doubles per n) the actinic
   flux (S/mu0 + (D - S)/mu_dif) + U/mu_dif, in that order, to actinic[i a_stride + (k V + level)]; mu0 [ncol], i = c sets +
   set. */
typedef struct GrtResponseArgs
{
    int responses;                  /* R */
    int block_max;                  /* the most responses with a point in one workgroup: sizes the dynamic LDS */
    uint64_t per_row;               /* P: the (response, block) pairs, partial sums per row and slot */
    int const *entry;               /* DEVICE [R][GRT_WINDOW_INTS] */
    int const *block_start;         /* DEVICE [nblocks + 1] */
    int const *block_list;          /* DEVICE [P] */
    double const *weights;          /* DEVICE [the responses' points] */
    double *partials;               /* DEVICE [slot][P][G V] */
} GrtResponseArgs;
static inline int grt_response_args_ok(GrtResponseArgs const *r)
{
    return r != NULL && r->responses >= 1 && r->block_max >= 1 && r->per_row >= 1 && r->entry != NULL &&
           r->block_start != NULL && r->block_list != NULL && r->weights != NULL && r->partials != NULL;
}
int grt_launch_response_rows(void *stream, GrtResponseArgs const *r, double const *const rows[3], int groups, int slots,
                             int num_levels, uint64_t nw, double dw);
int grt_launch_response_finish(void *stream, GrtResponseArgs const *r, int groups, int ncol, int subcolumns, int num_levels,
                               double *out, uint64_t out_stride, uint64_t out_offset);
int grt_launch_actinic_rows(void *stream, double const *weighted, uint64_t stride, int ncol, int sets, int responses,
                            int num_levels, double const *mu0, double mu_dif, double *actinic);

/* Longwave scattering correction (k_longwave_scatter.hip: lw_scatter_kernel; grt_pipeline_run_sky_scattering,
   grt_lw_scatter_levels).  lw_kernel takes every particle as an absorber, tau (1 - omega).  The correction is the
   difference of two two-stream adding solves of the same code at every grid point,
     delta_i = F_i[tau, omega, g] - F_i[tau (1 - omega), 0, 0]      (upward and downward, every level i),
   so a point none of whose layers scatters gets exactly +0.0.  Per layer, D = 1.66:
     gamma1 = D (1 - omega (1 + g)/2), gamma2 = D omega (1 - g)/2, k = sqrt(max((gamma1 - gamma2)(gamma1 + gamma2), 1e-12)),
     x = min(k tau, 700), e = exp(-x), E = -expm1(-2 x), m = -expm1(-x), den = k (1 + e e) + gamma1 E,
     R = gamma2 E/den, T = 2 k e/den, eps = (k m m + (gamma1 - gamma2) E)/den      (= 1 - R - T without the cancellation),
     S_up = eps pi effective_planck(B(t_layer), B(t_level j), tau (1 - omega)), S_down = ... B(t_level j + 1) ...:
   planck and effective_planck are lw_kernel's, on lw_kernel's arguments.  Adding, level V - 1 the surface:
     A_L = 1 - emis, U_L = emis pi B(t_surf);
     up:   beta_j = 1/(1 - A_{j+1} R_j), A_j = R_j + T_j T_j A_{j+1} beta_j, U_j = S_up_j + T_j (U_{j+1} + A_{j+1} S_down_j) beta_j;
     down: F_down_0 = 0, F_up_0 = U_0, F_down_{j+1} = (T_j F_down_j + R_j U_{j+1} + S_down_j) beta_j,
           F_up_{j+1} = A_{j+1} F_down_{j+1} + U_{j+1}.
   One thread per grid point and grid row, GRT_SOLVER_BLOCK threads a workgroup, as lw_kernel: the first sweep runs from the
   surface to the top with (A, U) of both solves in registers and parks, per layer j, GRT_SCATTER_PARK_ROWS rows -- R_j,
   T_j, S_down_j, A_{j+1}, U_{j+1} of the scattering solve, then of its absorption twin -- at
   park[((y L + j) GRT_SCATTER_PARK_ROWS + r) pw + i], y the grid row of the launch and pw = workgroups x GRT_SOLVER_BLOCK
   (every thread its own place: idle lanes of the last block park too); the second sweep runs from the top down, reads
   them back and hands both differences of every level to a LevelSink.  park_rows: the grid rows the block has room for --
   a launch of more is refused.  Instances: GRT_OUT_CHAINS -- the tau, omega of GrtLwArgs and g (NULL: 0) on the grid, the
   differences to GrtLwArgs' flux_up / flux_down [ncol][V][nw] and, where given, the scattering solve's own fluxes to
   flux_up / flux_down here --, and GRT_OUT_ROWS and GRT_OUT_LEVELS with every join of clouds and aerosols lw_kernel has,
   the differences' partial sums to GrtLwArgs' partials, laid out as lw_kernel's. */
#define GRT_SCATTER_PARK_ROWS 10
typedef struct GrtScatterArgs
{
    double *park;
    uint64_t park_rows;
    double const *g;                /* GRT_OUT_CHAINS: [ncol][L][nw] at GrtLwArgs' optics_stride, or NULL */
    double *flux_up, *flux_down;    /* GRT_OUT_CHAINS: [ncol][V][nw] at GrtLwArgs' flux_stride, or NULL */
} GrtScatterArgs;
static inline int grt_scatter_args_ok(GrtScatterArgs const *sa)
{
    return sa != NULL && sa->park != NULL && sa->park_rows >= 1 && (sa->flux_up != NULL) == (sa->flux_down != NULL);
}
/* corrected[c out_stride + out_offset + r] += delta[c delta_stride + delta_offset + r], r < rows, c < n: one fp64
   addition each (grt_pipeline_run_sky_scattering: a set's longwave rows and their differences) */
int grt_launch_scatter_add(void *stream, int n, int rows, double *corrected, uint64_t out_stride, uint64_t out_offset,
                           double const *delta, uint64_t delta_stride, uint64_t delta_offset);

/* One instance of lw_kernel / sw_kernel (k_longwave.hip, k_shortwave.hip), described once for the launchers, the kernels
   and the pipeline: what leaves the kernel ... */
typedef enum GrtSolverOutput
{
    GRT_OUT_CHAINS,         /* spectral fluxes [V][nw]: one thread per wavenumber and column through all the layers */
    GRT_OUT_LAYERS,         /* the same fluxes, the layers' terms first (layer_terms / layer_props), then the sweeps */
    /* fused (the kernel forms the layer optics from tau_gas and integrates over the band): partial sums of ... */
    GRT_OUT_ROWS,           /* the six output rows */
    GRT_OUT_ROWS_POINTS,    /* the six rows, and the six rows at every point: up TOA, surface, user at flux_up + c
                               flux_stride + k nw, k = 0, 1, 2, down at flux_down + ... (grt_pipeline_run_spectral) */
    GRT_OUT_LEVELS,         /* every level's up and down flux */
    GRT_OUT_LEVEL_BINS      /* every level's up and down flux per wavenumber bin of `bins` */
} GrtSolverOutput;
/* ... and what joins gas and Rayleigh in a fused instance, or rides with it: every pointer NULL is clear sky.  The kind of
   instance follows from which pointers are set, and a kernel takes the structs that are set as arguments after its band's
   own, in the order of the GRT_JOIN_ bits below.  Which sets exist is said once per kernel family, by the rules behind
   grt_sw_instance_exists and its kin at the end of this file; grt_launch_joined (hip/solver_dispatch.h) turns a set into the
   kernel's template arguments.  The next joined object is a pointer here, a bit in the order, a line in a rule and a
   `pick` where the kernel reads it. */
typedef struct GrtSolverInstance
{
    GrtSolverOutput out;
    GrtCloudArgs const *clouds;
    GrtAerosolArgs const *aerosols;
    GrtSubcolumnArgs const *subcolumns;
    GrtBandArgs const *bins;
    GrtZenithArgs const *zeniths;
    GrtDirectArgs const *direct;
    GrtJacobianArgs const *jacobian;
    GrtResponseArgs const *responses;
    GrtScatterArgs const *scatter;  /* grt_launch_lw_scatter's instances (GRT_OUT_CHAINS, _ROWS, _LEVELS): no other launcher's */
    GrtZenithSurfaceArgs const *zenith_surface;
    GrtZenithSlantArgs const *zenith_slant;
} GrtSolverInstance;
/* a join as a bit, in the order the kernels take the joins in their packs (grt_solver_joins lists the pointers in it);
   GRT_JOIN_CHANNELS is the GrtChannelArgs last in lw_radiance_kernel's pack, which no GrtSolverInstance carries, and
   `scatter` has no bit: lw_scatter_kernel takes its GrtScatterArgs as a parameter of its own, ahead of the pack */
enum
{
    GRT_JOIN_CLOUDS = 1 << 0, GRT_JOIN_SUBCOLUMNS = 1 << 1, GRT_JOIN_AEROSOLS = 1 << 2, GRT_JOIN_ZENITHS = 1 << 3,
    GRT_JOIN_ZENITH_SURFACE = 1 << 4, GRT_JOIN_ZENITH_SLANT = 1 << 5, GRT_JOIN_DIRECT = 1 << 6, GRT_JOIN_JACOBIAN = 1 << 7,
    GRT_JOIN_RESPONSES = 1 << 8, GRT_JOIN_BINS = 1 << 9, GRT_JOIN_CHANNELS = 1 << 10, GRT_JOIN_BITS = 11
};
#ifdef __cplusplus
#define GRT_FN constexpr
#else
#define GRT_FN static inline
#endif
GRT_FN int grt_out_fused(GrtSolverOutput out) { return out >= GRT_OUT_ROWS; }
GRT_FN int grt_out_levels(GrtSolverOutput out) { return out >= GRT_OUT_LEVELS; }
#undef GRT_FN
/* the rows of its grid: a column each, or (subcolumns, zeniths) `count` subcolumns or angles of every column -- with both,
   every angle of every subcolumn of the launch */
static inline uint64_t grt_solver_grid_rows(GrtSolverInstance const *in, int ncol)
{
    return (uint64_t)ncol*(uint64_t)(in->subcolumns != NULL ? in->subcolumns->count : 1)*
           (uint64_t)(in->zeniths != NULL ? in->zeniths->count : 1);
}
/* its dynamic LDS: 2 V doubles per wave of its workgroup where every level leaves (3 V with the direct beam or the
   surface-temperature Jacobian), that per bin of a block with bins; with responses, that once more per response of a
   block and the block's staged weights, 128 doubles per response */
#define GRT_SOLVER_BLOCK 128
static inline size_t grt_solver_lds(GrtSolverInstance const *in, int num_levels)
{
    size_t const levels = sizeof(double)*(in->direct != NULL || in->jacobian != NULL ? 3 : 2)*(size_t)num_levels*(GRT_SOLVER_BLOCK/64);
    if (grt_out_levels(in->out) && in->responses != NULL)
    {
        return levels*(1 + (size_t)in->responses->block_max) + sizeof(double)*GRT_SOLVER_BLOCK*(size_t)in->responses->block_max;
    }
    return !grt_out_levels(in->out) ? 0 : (in->bins != NULL ? levels*(size_t)in->bins->block_bins : levels);
}
/* the doubles of a scattering park block (GrtScatterArgs) for `rows` grid rows of a band of nw points and num_levels levels */
static inline uint64_t grt_scatter_park_doubles(uint64_t rows, int num_levels, uint64_t nw)
{
    uint64_t const pw = (nw + GRT_SOLVER_BLOCK - 1)/GRT_SOLVER_BLOCK*GRT_SOLVER_BLOCK;
    return rows*(uint64_t)(num_levels - 1)*GRT_SCATTER_PARK_ROWS*pw;
}
/* the most responses one block may hold at num_levels levels and `groups` row groups (2; 3 with the third row group):
   16 G V (1 + R_b) + 1024 R_b <= 65536 */
static inline int grt_response_block_limit(int num_levels, int groups)
{
    long long const levels = 16ll*groups*num_levels;
    long long const r = (65536 - levels)/(levels + 8*GRT_SOLVER_BLOCK);
    return r < 0 ? 0 : (int)r;
}
/* whether the shortwave instance takes the two sweeps and needs `park` */
static inline int grt_sw_parks(GrtSolverInstance const *in, GrtSwArgs const *a)
{
    return grt_out_fused(in->out) && (grt_out_levels(in->out) || !grt_sw_one_sweep(a));
}
/* The one launcher of each band: checks the instance (grt_solver_instance_ok below and the fields only its own arguments
   carry: the layers' scratch, the shortwave's park block) and launches it; hipErrorInvalidValue for an instance that
   cannot run or has no kernel behind it. */
int grt_launch_lw(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a);
int grt_launch_sw(void *stream, GrtSolverInstance const *in, GrtSwArgs const *a);
/* lw_scatter_kernel (GrtScatterArgs, in->scatter) in the instance of in's output and joins, on the longwave solver's
   arguments: GRT_OUT_CHAINS writes the differences where that solver writes its fluxes, the fused forms leave their partial
   sums where it leaves its own.  hipErrorInvalidValue for an instance without `scatter`, one that cannot run, or a grid of
   more rows than the park block holds. */
int grt_launch_lw_scatter(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a);
/* lw_radiance_kernel (GrtRadianceArgs) beside the longwave solver of instance `in`, on that solver's arguments: the
   instance's joins select the kernel (none, clouds, aerosols, subcolumns, clouds or subcolumns with aerosols) and its grid
   rows, a spectral output form (GRT_OUT_CHAINS, GRT_OUT_LAYERS) the materialised one; bins, zeniths, direct and jacobian
   are not read. */
int grt_launch_lw_radiances(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a, GrtRadianceArgs const *r);
/* ... its channel form (GrtChannelArgs): the same launch, and the channels' partial sums beside everything it leaves */
int grt_launch_lw_channels(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a, GrtRadianceArgs const *r,
                           GrtChannelArgs const *c);
int grt_launch_channel_finish(void *stream, GrtChannelArgs const *c, int ncol, int subcolumns, int angles, double *out,
                              double *brightness, uint64_t out_stride, uint64_t out_offset);
/* ... and the channels' transmittance profiles and contribution functions (GrtWeightingArgs): the same instance, grid and
   arguments, c->partials not read */
int grt_launch_lw_weighting(void *stream, GrtSolverInstance const *in, GrtLwArgs const *a, GrtRadianceArgs const *r,
                            GrtChannelArgs const *c, GrtWeightingArgs const *w);
int grt_launch_weighting_finish(void *stream, GrtChannelArgs const *c, GrtWeightingArgs const *w, int ncol, int subcolumns,
                                int angles, int num_levels, double *transmittance, uint64_t t_stride, uint64_t t_offset,
                                double *contribution, uint64_t k_stride, uint64_t k_offset);
/* The subcolumn mean of the partial sums above, in a fixed order: for column c and row r (of `rows` per slot) each
   subcolumn's blocks are added as grt_launch_reduce_partials adds them, then the subcolumns s = 0 .. S - 1 in order, then
   the sum is divided by S; out[c out_stride + out_offset + r].  S = 1 gives grt_launch_reduce_partials' bits. */
int grt_launch_subcolumn_mean(void *stream, double const *partials, int ncol, int subcolumns, int rows, unsigned nblocks,
                              double *out, int out_stride, int out_offset);
/* Materialised form of grt_pipeline_run_subcolumns (driver.c:503-584): sum[i] = (first ? 0 : sum[i]) + x[i], i < n; and
   at the end x[i] = sum[i]/S. */
int grt_launch_flux_accumulate(void *stream, uint64_t n, double const *x, double *sum, int first);
int grt_launch_flux_mean(void *stream, uint64_t n, double const *sum, int subcolumns, double *x);
/* Materialised form: the cloud objects of the same tables spread onto the grid, [ncol][L][nw] each (tau = extinction x
   thickness; zero where a point has no band). */
int grt_launch_spread_clouds(void *stream, int num_layers, int ncol, uint64_t nw, GrtCloudArgs const *c,
                             double *liquid_tau, double *liquid_omega, double *liquid_g,
                             double *ice_tau, double *ice_omega, double *ice_g);

/* The cloud sampler (k_cloud_sample.hip; grt_ext.h: grt_cloud_sampler_run): the band optics of `subcolumns` draws per
   column and pass from the columns' cloud fields.  One wavefront per sample (column, pass, subcolumn, band), lanes over
   layers in chunks of 64.  Everything is DEVICE memory.  Of the beta tables the kernel reads three rows only, the (5, 5)
   water PDF's: inverse[q = 5][p = 5] twice and value[q = 5][p = 6]; x must ascend (the segment is found by bisection).
   A phase's coef [band][size][coefficient] as PadeOptics holds them.  uniforms [ncol][2][S][B][2 L - 1] or NULL: then
   Philox4x32-10 with key (key0, key1) and counter (layer, band, pass GRT_SAMPLER_MAX_SUBCOLUMNS + s, column0 + c).
   tables [4][S][ncol][3][B][L]: lw_liquid, lw_ice, sw_liquid, sw_ice. */
#define GRT_SAMPLER_MAX_SUBCOLUMNS 64   /* grt_ext.h: GRT_MAX_SUBCOLUMNS */
typedef struct GrtCloudPhaseDev
{
    int nsize, np, nq;
    double const *size_lo, *size_hi, *size_ref;
    double const *coef[6];
} GrtCloudPhaseDev;
typedef struct GrtCloudSampleArgs
{
    int ncol, num_layers, subcolumns, num_bands;
    int num_x;
    double const *x, *inverse_pq, *value_p1q;       /* [num_x] each */
    GrtCloudPhaseDev liquid, ice;
    double const *cloud_fraction, *liquid_content, *ice_content, *temperature;   /* [ncol][L] */
    double const *overlap;                           /* [ncol][L-1] */
    double liquid_radius;
    double const *uniforms;
    uint32_t key0, key1, column0;
    double *tables;
} GrtCloudSampleArgs;
int grt_launch_cloud_sample(void *stream, GrtCloudSampleArgs const *a);

/* K-distributions of optical-depth rows (k_kdist.hip; grt_ext.h: grt_kdist_rows, which defines the reduction): per row of
   tau [rows][n], bin b of edges [num_bins + 1] (grid-point indices, strictly increasing in 0 .. n - 1) and class k of the
   num_classes that class_edges [num_classes - 1] (strictly increasing) cut -- the number of the bin's points in the class,
   the sum of their trapezoid weights (dw, dw/2 at the bin's two end points, times weight [n] where that is given) and the
   sum of weight x tau, each sum sequential in increasing grid index.  Everything is DEVICE memory; the outputs are
   [rows][num_bins][num_classes], any of them NULL, not all.  One workgroup per (row, bin);
   grt_kdist_chunk: the points it stages at a time. */
#define GRT_KDIST_CLASS_LIMIT 1024      /* grt_ext.h: GRT_KDIST_MAX_CLASSES */
typedef struct GrtKdistArgs
{
    double const *tau;
    long long rows, n;
    double dw;
    int num_classes, num_bins;
    double const *class_edges;
    int const *edges;
    double const *weight;           /* or NULL: 1 */
    int *points;
    double *weight_sum, *tau_sum;
} GrtKdistArgs;
int grt_kdist_chunk(void);
int grt_launch_kdist(void *stream, GrtKdistArgs const *a);

/* Correlated k-distributions (k_kdist.hip; grt_ext.h: grt_kdist_class_map and grt_kdist_mapped_rows, which define them).
   The map: per group g of x [groups][rows_per_group][n] and point i, the class (as above) of the key -- x[g][key_row][i],
   or with key_row < 0 the sum of the group's rows in order from +0.0 -- to map [groups][n].
   The mapped reduction: row r of group g starts at values + g group_stride + r n; a point's class is map[g][i], and an
   entry >= num_classes belongs to no class.  points and weight_sum are [groups][num_bins][num_classes] (the same for
   every row), tau_sum [groups][rows_per_group][num_bins][num_classes]; any of them NULL, not all.  One workgroup per
   (group, row, bin), per (group, bin) without tau_sum. */
typedef struct GrtKdistMapArgs
{
    double const *x;
    long long groups, rows_per_group, n;
    long long key_row;              /* or < 0: the sum of the rows */
    int num_classes;
    double const *class_edges;
    unsigned short *map;
} GrtKdistMapArgs;
typedef struct GrtKdistMappedArgs
{
    double const *values;
    long long group_stride;
    unsigned short const *map;
    long long groups, rows_per_group, n;
    double dw;
    int num_classes, num_bins;
    int const *edges;
    double const *weight;           /* or NULL: 1 */
    int *points;
    double *weight_sum, *tau_sum;
} GrtKdistMappedArgs;
int grt_launch_kdist_map(void *stream, GrtKdistMapArgs const *a);
int grt_launch_kdist_mapped(void *stream, GrtKdistMappedArgs const *a);

/* Flux solves of a correlated-k model on its g-classes (grt_ext.h: grt_pipeline_run_ck_fluxes, which defines them).
   The source sums (k_kdist.hip: kdist_sources_kernel): the mapped reduction's walk, one workgroup per (column, source row,
   bin), with the row's value at a point computed -- the Planck function at a level's, a layer's or the surface's
   temperature (longwave rows 0 .. V - 1, V .. 2 V - 2, 2 V - 1), the Rayleigh cross-section (shortwave row 0) -- or loaded
   from a data row -- data[0] (longwave row 2 V: the emissivity), data[0 .. 2] (shortwave rows 1 .. 3: the solar curve, the
   direct and the diffuse albedo), column c's at data[k] + c data_stride[k].  source_sum is [ncol][R][num_bins]
   [num_classes], R = 2 V + 1 or 4.  A map entry >= num_classes belongs to no class. */
typedef struct GrtCkSourceArgs
{
    int longwave;                   /* != 0: the longwave's rows */
    int num_levels;
    long long ncol, n;
    double w0, dw;
    int num_classes, num_bins;
    int const *edges;
    unsigned short const *map;      /* [ncol][n] */
    double const *t_levels, *t_layers, *t_surf;     /* longwave: [ncol][V], [ncol][V - 1], [ncol] */
    double const *data[3];
    uint64_t data_stride[3];
    double *source_sum;
} GrtCkSourceArgs;
int grt_launch_ck_sources(void *stream, GrtCkSourceArgs const *a);
/* The solve (k_longwave.hip: ck_lw_kernel, k_shortwave.hip: ck_sw_kernel): one thread per (column, bin, class) walks the
   column's layers on the class means -- weight_sum [ncol][num_bins][num_classes], tau_sum [ncol][V - 1][..][..],
   source_sum [ncol][R][..][..] -- and leaves every level's flux of the class in W m-2 at flux_up, flux_down
   [ncol][V][..][..]; +0.0 for a class of weight 0 and (shortwave) for a column with mu_dir <= 0.  The shortwave reads
   n_layer [ncol][V - 1], mu_dir and tsi [ncol] and mu_dif too. */
typedef struct GrtCkSolveArgs
{
    int num_levels, ncol, num_bins, num_classes;
    double const *weight_sum, *tau_sum, *source_sum;
    double *flux_up, *flux_down;
    double const *n_layer, *mu_dir, *tsi;
    double mu_dif;
} GrtCkSolveArgs;
static inline int grt_ck_solve_args_ok(GrtCkSolveArgs const *a)
{
    return a != NULL && a->num_levels >= 2 && a->ncol >= 1 && a->num_bins >= 1 && a->num_classes >= 2 &&
           a->num_classes <= GRT_KDIST_CLASS_LIMIT && a->weight_sum != NULL && a->tau_sum != NULL &&
           a->source_sum != NULL && a->flux_up != NULL && a->flux_down != NULL &&
           /* (a grid of workgroups of GRT_SOLVER_BLOCK threads) */
           ((uint64_t)a->ncol*(uint64_t)a->num_bins*(uint64_t)a->num_classes + GRT_SOLVER_BLOCK - 1)/GRT_SOLVER_BLOCK <= 0x7fffffffull;
}
int grt_launch_ck_lw(void *stream, GrtCkSolveArgs const *a);
int grt_launch_ck_sw(void *stream, GrtCkSolveArgs const *a);
/* The bin sums (k_kdist.hip: ck_bin_sum_kernel): out[r] = (((+0.0 + in[r K]) + in[r K + 1]) + ...) + in[r K + K - 1] for
   every row r < rows, one thread a row. */
int grt_launch_ck_bin_sum(void *stream, double const *in, long long rows, int num_classes, double *out);

/* Fused Rayleigh + combine for the clear-sky driver sequence (rayleigh.c:39 +
   optics.c:138-145 with K=2, gas omega=g=0, Rayleigh omega=1,g=0):
   tau_tot = tau_gas + tau_R, omega = tau_R/tau_tot, g = 0/ tau_R.  n_layer [ncol][L]. */
int grt_launch_clear_sky_optics(void *stream, int num_layers, int ncol, double w0, double dw,
                                uint64_t nw, double const *n_layer, double const *tau_gas,
                                double *tau, double *omega, double *g);

/* driver.c:302-326 on device rows: sum 0.5*(row[i]+row[i+1])*dw of row r goes to
   out[(r/group)*out_stride + out_offset + r%group]. */
int grt_launch_integrate_rows(void *stream, double const *const *rows_dev, int nrows,
                              uint64_t nw, double dw, double *out, int group, int out_stride,
                              int out_offset);
/* Wavenumber bins of spectral rows (grt_pipeline_run_spectral), deterministic and in the fused solvers' association: bin b
   of a row is sum_i x_i w_i over the row's points, w_i = dw inside edges[b] .. edges[b+1], dw/2 at those two points, 0
   elsewhere; summed per 128-point solver block as block_partials does (a 64-lane shuffle tree, then wave 0 + wave 1),
   then the bin's blocks in order from its first block as reduce_partials does.  A bin over the whole grid is the six-row
   form's integral to the bit.  Row r (of nrows) is in + (r/6) in_stride + (r%6) nw; its bins go to
   out + (r/6) out_stride + (r%6) nbins + b.  table_dev: grt_bin_table's ints; partials: nrows x the partial sums
   per row that grt_bin_table returns, doubles. */
size_t grt_bin_table_ints(int nbins, uint64_t nw);
/* the table of edges_h [nbins + 1] (host, strictly increasing in 0 .. nw - 1) into table_h [grt_bin_table_ints]; returns
   the partial sums per row */
size_t grt_bin_table(int const *edges_h, int nbins, uint64_t nw, int *table_h);
int grt_launch_bin_rows(void *stream, double const *in, uint64_t in_stride, int nrows, uint64_t nw, double dw,
                        int nbins, int const *table_dev, size_t partials_per_row, double *partials, double *out,
                        uint64_t out_stride);
/* Wavenumber bins of level fluxes (grt_pipeline_run_band_profiles).  Row r (of nrows = ncol x 2 V) is level r % V of
   column r / (2 V), upward when r % (2 V) < V; its bin b goes to out + (r / (2 V)) out_stride + ((r % (2 V) / V) nbins + b) V
   + r % V: per column [2][nbins][V], up then down.
   grt_bin_block_max: the most bins of edges_h [nbins + 1] that have a point in one 128-point solver block.
   grt_launch_bin_reduce: the second stage alone, on the partial sums a banded profile solver left (GrtBandArgs), each
   bin's blocks in order from its first as reduce_partials adds them: a bin over the whole grid is the profile form's
   level flux to the bit.
   grt_launch_bin_level_rows: both stages on the materialised form's spectra, row r at rows_dev[r] [nw] (DEVICE table),
   weighted and summed as grt_launch_bin_rows does. */
int grt_bin_block_max(int const *edges_h, int nbins);
int grt_launch_bin_reduce(void *stream, int nrows, int num_levels, int nbins, int const *table_dev, size_t partials_per_row,
                          double const *partials, double *out, uint64_t out_stride);
int grt_launch_bin_level_rows(void *stream, double const *const *rows_dev, int nrows, int num_levels, uint64_t nw, double dw,
                              int nbins, int const *table_dev, size_t partials_per_row, double *partials, double *out,
                              uint64_t out_stride);
/* Last step of grt_pipeline_run_band_profiles: levels [ncol][sets][2 lw_bins + 2 sw_bins][V] (per set the longwave's
   [2][lw_bins][V], up then down, then the shortwave's) -> heating [ncol][sets][lw_bins + sw_bins][V-1] K day-1, by
   grt_launch_profile_finish's formula and constants on each bin's level fluxes; pressure [ncol][V] mb. */
int grt_launch_band_profile_finish(void *stream, int ncol, int sets, int num_levels, int lw_bins, int sw_bins,
                                   double gravity, double cp, double const *pressure, double const *levels,
                                   double *heating);
/* out + (r/6) out_stride + (r%6) nw  <-  rows_dev[r] [nw], r < nrows (the materialised form's spectral rows) */
int grt_launch_copy_rows(void *stream, double const *const *rows_dev, int nrows, uint64_t nw, double *out,
                         uint64_t out_stride);

#ifdef __cplusplus
}
#include <tuple>

/* The pointers of an instance in the order of the GRT_JOIN_ bits -- the order of a kernel's pack -- and the bit-set of
   those that are set, of these or of any such tuple (entry k is bit k). */
inline auto grt_solver_joins(GrtSolverInstance const &in)
{
    return std::make_tuple(in.clouds, in.subcolumns, in.aerosols, in.zeniths, in.zenith_surface, in.zenith_slant, in.direct,
                           in.jacobian, in.responses, in.bins);
}
template <typename... P>
inline unsigned grt_join_set(std::tuple<P...> const &joins)
{
    return std::apply([](auto const *...p)
                      {
                          unsigned set = 0, bit = 1;
                          ((set |= p != nullptr ? bit : 0u, bit <<= 1), ...);
                          return set;
                      }, joins);
}

/* Which instances exist: one rule per kernel family, on the output and the bit-set `m` of the joins.  The launchers
   instantiate exactly these (grt_launch_joined, hip/solver_dispatch.h) and grt_solver_instance_ok refuses every other.
   GRT_OUT_LAYERS is the two-kernel form, no instance of these templates: its launchers take it with no join at all. */
constexpr unsigned GRT_JOIN_FRONT = GRT_JOIN_CLOUDS | GRT_JOIN_SUBCOLUMNS | GRT_JOIN_AEROSOLS;
/* the joins every fused output shares: the clouds in one form at most, the aerosol object with either or alone */
constexpr bool grt_front_exists(unsigned m) { return (m & GRT_JOIN_CLOUDS) == 0 || (m & GRT_JOIN_SUBCOLUMNS) == 0; }
/* ... and what the outputs other than the six rows and the levels take, in both bands: the chains nothing, the six rows at
   every point the clouds or nothing, the bins `bins` behind the clouds or behind nothing */
constexpr bool grt_plain_instance_exists(GrtSolverOutput out, unsigned m)
{
    return out == GRT_OUT_CHAINS ? m == 0 : out == GRT_OUT_ROWS_POINTS ? (m & ~GRT_JOIN_CLOUDS) == 0 :
           out == GRT_OUT_LEVEL_BINS && (m & ~GRT_JOIN_CLOUDS) == GRT_JOIN_BINS;
}
constexpr bool grt_sw_instance_exists(GrtSolverOutput out, unsigned m)
{
    if (out != GRT_OUT_ROWS && out != GRT_OUT_LEVELS)
    {
        return grt_plain_instance_exists(out, m);
    }
    bool const direct = (m & GRT_JOIN_DIRECT) != 0;
    if (!grt_front_exists(m) || (m & (GRT_JOIN_JACOBIAN | GRT_JOIN_BINS | GRT_JOIN_CHANNELS)) != 0)
    {
        return false;
    }
    if ((m & GRT_JOIN_ZENITHS) != 0)    // never with clouds or responses; a cosine per layer needs the direct beam
    {
        return (m & (GRT_JOIN_CLOUDS | GRT_JOIN_RESPONSES)) == 0 && ((m & GRT_JOIN_ZENITH_SLANT) == 0 || direct);
    }
    // what goes behind the zeniths goes with nothing else; the responses leave the levels beside the direct beam
    return (m & (GRT_JOIN_ZENITH_SURFACE | GRT_JOIN_ZENITH_SLANT)) == 0 &&
           ((m & GRT_JOIN_RESPONSES) == 0 || (direct && out == GRT_OUT_LEVELS));
}
constexpr bool grt_lw_instance_exists(GrtSolverOutput out, unsigned m)
{
    if (out != GRT_OUT_ROWS && out != GRT_OUT_LEVELS)
    {
        return grt_plain_instance_exists(out, m);
    }
    // the Jacobian or the responses (the levels') behind the front, not both
    unsigned const behind = m & ~GRT_JOIN_FRONT;
    return grt_front_exists(m) && (behind == 0 || behind == GRT_JOIN_JACOBIAN ||
                                   (behind == GRT_JOIN_RESPONSES && out == GRT_OUT_LEVELS));
}
/* lw_scatter_kernel (the GrtScatterArgs is a parameter of its own, ahead of the pack) */
constexpr bool grt_lw_scatter_instance_exists(GrtSolverOutput out, unsigned m)
{
    return out == GRT_OUT_CHAINS ? m == 0 : (out == GRT_OUT_ROWS || out == GRT_OUT_LEVELS) && grt_front_exists(m) &&
                                            (m & ~GRT_JOIN_FRONT) == 0;
}
/* lw_radiance_kernel, with the channels last or without, and -- never with GRT_JOIN_CHANNELS: the GrtChannelArgs is a
   parameter of its own there -- lw_weighting_kernel: the front behind the fused form, nothing behind the materialised one */
constexpr bool grt_lw_radiance_instance_exists(bool fused, unsigned m)
{
    return grt_front_exists(m) && (m & ~(GRT_JOIN_FRONT | GRT_JOIN_CHANNELS)) == 0 && (fused || (m & GRT_JOIN_FRONT) == 0);
}
/* sw_zenith_kernel (the GrtZenithArgs is a parameter of its own): what a zenith instance of the six rows takes behind it */
constexpr bool grt_sw_zenith_instance_exists(unsigned m)
{
    return (m & GRT_JOIN_ZENITHS) == 0 && grt_sw_instance_exists(GRT_OUT_ROWS, m | GRT_JOIN_ZENITHS);
}
/* lw_tile_kernel and sw_tile_kernel */
constexpr bool grt_tile_instance_exists(unsigned m)
{
    return (m & ~(GRT_JOIN_SUBCOLUMNS | GRT_JOIN_AEROSOLS)) == 0;
}
/* the angles per thread of a shared-layer instance and the tiles per thread of a tile instance (grt_zenith_chunk,
   grt_tile_chunk) */
constexpr int grt_zenith_chunk_of(unsigned m)
{
    bool const surface = (m & GRT_JOIN_ZENITH_SURFACE) != 0, aerosols = (m & GRT_JOIN_AEROSOLS) != 0;
    return (m & GRT_JOIN_ZENITH_SLANT) != 0 ? (surface ? GRT_ZENITH_CHUNK_SLANT_SURFACE : GRT_ZENITH_CHUNK_SLANT) :
           (m & GRT_JOIN_DIRECT) != 0 ? (surface ? GRT_ZENITH_CHUNK_DIRECT_SURFACE : GRT_ZENITH_CHUNK_DIRECT) :
           surface ? GRT_ZENITH_CHUNK_SURFACE :
           (m & GRT_JOIN_SUBCOLUMNS) != 0 ? (aerosols ? GRT_ZENITH_CHUNK_SUBCOLUMNS_AEROSOLS : GRT_ZENITH_CHUNK_SUBCOLUMNS) :
           aerosols ? GRT_ZENITH_CHUNK_AEROSOLS : GRT_ZENITH_CHUNK;
}
constexpr int grt_tile_chunk_of(unsigned m)
{
    bool const aerosols = (m & GRT_JOIN_AEROSOLS) != 0;
    return (m & GRT_JOIN_SUBCOLUMNS) != 0 ? (aerosols ? GRT_TILE_CHUNK_SUBCOLUMNS_AEROSOLS : GRT_TILE_CHUNK_SUBCOLUMNS) :
           aerosols ? GRT_TILE_CHUNK_AEROSOLS : GRT_TILE_CHUNK;
}
/* ... and the band's rule for an instance as the launchers get it: the longwave's with `scatter` is lw_scatter_kernel's */
inline bool grt_band_instance_exists(GrtSolverInstance const &in, GrtSwArgs const &)
{
    unsigned const m = grt_join_set(grt_solver_joins(in));
    return in.scatter == nullptr && (in.out == GRT_OUT_LAYERS ? m == 0 : grt_sw_instance_exists(in.out, m));
}
inline bool grt_band_instance_exists(GrtSolverInstance const &in, GrtLwArgs const &)
{
    unsigned const m = grt_join_set(grt_solver_joins(in));
    return in.scatter != nullptr ? grt_lw_scatter_instance_exists(in.out, m) :
           in.out == GRT_OUT_LAYERS ? m == 0 : grt_lw_instance_exists(in.out, m);
}

/* Whether the instance `in` can run on `a` (GrtLwArgs or GrtSwArgs: the fields both carry), for both launchers: that it
   exists in a's band, each set pointer's own fields, what the output reads and writes, a grid of at most 65 535 rows and the
   64 KiB of LDS. */
template <typename Args>
inline bool grt_solver_instance_ok(GrtSolverInstance const &in, Args const &a)
{
    bool const fused = grt_out_fused(in.out), flux_rows = a.flux_up != nullptr && a.flux_down != nullptr;
    // (two grid points for a trapezoid; the chain form of the scattering correction integrates nothing: one will do)
    uint64_t const least_points = in.scatter != nullptr && !fused ? 1 : 2;
    // (the scattering correction parks per grid row: no more of them than its block holds)
    bool const scatter_ok = in.scatter == nullptr || (grt_scatter_args_ok(in.scatter) &&
                                                      grt_solver_grid_rows(&in, a.ncol) <= in.scatter->park_rows);
    return grt_band_instance_exists(in, a) && scatter_ok && a.ncol >= 1 && a.nw >= least_points && a.num_levels >= 2 &&
           (in.clouds == nullptr || grt_cloud_args_ok(in.clouds)) &&
           (in.aerosols == nullptr || grt_aerosol_args_ok(in.aerosols)) &&
           (in.subcolumns == nullptr || grt_subcolumn_args_ok(in.subcolumns)) &&
           (in.bins == nullptr || grt_band_args_ok(in.bins)) &&
           (in.zeniths == nullptr || grt_zenith_args_ok(in.zeniths)) &&
           (in.zenith_surface == nullptr || grt_zenith_surface_args_ok(in.zenith_surface)) &&
           (in.zenith_slant == nullptr || grt_zenith_slant_args_ok(in.zenith_slant)) &&
           (in.direct == nullptr || grt_direct_args_ok(in.direct)) &&
           (in.jacobian == nullptr || grt_jacobian_args_ok(in.jacobian)) &&
           (in.responses == nullptr || grt_response_args_ok(in.responses)) &&
           (fused ? a.tau_gas != nullptr && a.n_layer != nullptr && a.partials != nullptr : flux_rows) &&
           (in.out != GRT_OUT_ROWS_POINTS || flux_rows) &&
           grt_solver_grid_rows(&in, a.ncol) <= 65535u && grt_solver_lds(&in, a.num_levels) <= 65536;
}
#endif
#endif
