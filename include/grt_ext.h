/* grt_ext.h -- entry points beyond the reference's ABI.
 *
 * The reference ABI (grtcode_hip_api.h) is one column per call, synchronous, with
 * host-pointer outputs.  That shape cannot fill 256 CUs at coarse grids (3 250 points
 * in the 1 cm-1 longwave band) and forces 2*V*n doubles over PCIe per call, so the
 * production path is the batched, device-resident form below; the reference-shaped
 * calls are its ncol == 1 wrappers plus the copies the old signatures demand.
 * Everything here is plain C: pointers, sizes, no torch types.
 */
#ifndef GRT_EXT_H_
#define GRT_EXT_H_

#include "grtcode_hip_api.h"

/* ---- partition sums (replaces gas-optics/src/tips2017.c, a missing blob) ----------
 * Q(mol,T,iso) is served from a user-supplied table when one is loaded, otherwise from
 * a closed-form model: classical rotor x harmonic oscillators,
 * Q296(mol,iso) * (T/296)^beta * Qvib(T)/Qvib(296) (beta = 1 for linear molecules, 1.5
 * otherwise; within 0.1 % of the five TIPS-2017 values of test_tips2017.c:34-65), with a
 * warning on stderr the first time a molecule is served that way.  Only ratios Q(296)/Q(T)
 * reach the optical depths (parse_HITRAN_file.c:382 x kernels.c:62,85).
 * Table file: CSV with header, rows "mol_id,iso,T,Q", T ascending per (mol,iso);
 * linear interpolation in T, clamped at the ends.  Loading or dropping a table re-scales the
 * line strengths of every gas-optics object at its next calculation (the 296 K strengths are
 * kept as tabulated; Q(296) is applied when the device line store is built).
 * grt_tips_source: 0 = table, 1 = rotor x oscillators, 2 = rotor alone (no fundamentals
 * tabulated for that molecule), -1 = ids out of range. */
EXTERN int grt_tips_load(char const *path);
EXTERN int grt_tips_reset(void);
EXTERN int grt_tips_is_table(void);
EXTERN int grt_tips_source(int mol_id, int iso);

/* ---- HITRAN line parameters: parse once ------------------------------------------
 * The first add_molecule on a .par file indexes every molecule's records in memory (later calls, any molecule,
 * any object of the process, filter from that; GRT_HITRAN_CACHE=0 restores the reference's scan per call).
 * With GRT_HITRAN_CACHE_DIR=<directory> in the environment the index is also kept as a binary file there,
 * keyed by the .par file's path, size and modification time, and later processes read that instead of parsing
 * text.  stats = {requests served from memory, index files read, .par files scanned}. */
EXTERN int grt_hitran_index_stats(long long stats[3]);

/* ---- struct sizes for FFI callers (ctypes; cf. fortran-bindings/malloc_structs.c:40-66) */
enum grt_struct_kind
{
    GRT_SPECTRAL_GRID = 0, GRT_OPTICS, GRT_GAS_OPTICS, GRT_SOLAR_FLUX, GRT_LONGWAVE, GRT_SHORTWAVE, GRT_CLOUDS,
    GRT_CLOUD_PHASE, GRT_CLOUD_MODEL, GRT_CLOUD_FIELDS, GRT_LW_SCATTER
};
/* ... and the kinds that came after it, in the same numbering: GrtZenithSurface_t, GrtZenithDirect_t */
enum grt_struct_kind_more
{
    GRT_ZENITH_SURFACE = GRT_LW_SCATTER + 1, GRT_ZENITH_DIRECT
};
/* ... GrtZenithSlant_t */
enum grt_struct_kind_slant
{
    GRT_ZENITH_SLANT = GRT_ZENITH_DIRECT + 1
};
EXTERN size_t grt_sizeof(int kind);

/* ---- line lists from memory ------------------------------------------------------
 * Same effect as add_molecule() reading these records from a HITRAN .par file:
 * s_raw is the tabulated 296 K strength and is rescaled here exactly as
 * parse_HITRAN_file.c:372-384 does; yair/yself/en/nexp/delta are narrowed to float as
 * the file reader does (:197-212).  Lines outside the grid's [w0,wn] are dropped (:340). */
EXTERN int grt_add_molecule_lines(GasOptics_t *gas_optics, int molecule_id, uint64_t num_lines,
                                  int const *iso, double const *v0, double const *s_raw,
                                  double const *yair, double const *yself, double const *en,
                                  double const *nexp, double const *delta);

/* ---- launch tuning for the line kernel (tile, nslice: 0 keeps the automatic value) --
 * fast: 3 = fused arithmetic, far wings summed by cell moments, two passes (every line prepared once; cell moments
 *          through a device buffer of 32 bytes per column, layer and wavenumber) -- the production form, what bench.py
 *          runs and THE DEFAULT OF A NEW OBJECT (tau within 2e-6 of each layer's maximum, fluxes ~1e-5 W m-2 from the
 *          reference's: two orders inside the 1e-3 W m-2 of the interface's contract);
 *       1 = the same in one pass; 2 = fused arithmetic, every window point evaluated;
 *       0 = the reference's operation order (tau within 1e-11 of the reference's; 3.3x slower through the one-column
 *          calls).  GRT_GAS_OPTICS_FAST=0|1|2|3 in the environment sets the default of new objects for callers that
 *          cannot call this function (an unchanged reference driver).  optical_depth_method = wavenumber_sweep /
 *          line_sweep always run in reference order. */
EXTERN int grt_gas_optics_tune(GasOptics_t *gas_optics, int tile, int nslice, int fast);

/* What the last line-by-line launch of this object actually ran (the fused forms fall back 3 -> 1 -> 2 where a
 * grid does not suit them): info = {fast, tile, nslice, coarse levels of the cell hierarchy (0: single-level
 * far field), near-field halo in grid points, moment-buffer bytes, moments per cell (8; 12 on sparse fine grids), columns per
 * launch -- a batch whose cell moments would not fit the device runs in column groups, one after the other through the same
 * scratch, with the launch parameters of the undivided batch (GRT_SCRATCH_CAP_MB in the environment: a cap for tests)}.  Windows of more than 200 points a side
 * (grids finer than ~0.12 cm-1) make fast = 3 sum the far field through a hierarchy of cells. */
EXTERN int grt_gas_optics_last_launch(GasOptics_t const *gas_optics, long long info[8]);

/* ---- deterministic mode ------------------------------------------------------------
 * The fused forms (fast 1-3) and line slices accumulate with floating-point atomics in LDS and in tau, in whatever
 * order the hardware schedules waves and workgroups: two runs of the same input agree to ~1e-11 of a layer's largest
 * tau (fp32 cell moments) / ~1e-16 (fp64 near fields), not to the last bit.  With GRT_DETERMINISTIC=1 in the
 * environment (read at every launch), or grt_set_deterministic(1), every sum is formed in one fixed order and repeated
 * runs are bit-identical: one wave of each workgroup takes all of its lines in store order, tiles are never cut into
 * line slices, and the first pass of the two-pass form runs as a sequence of launches over non-overlapping cell tiles.
 * The values are as good as the default mode's (same formulas, another order); throughput is about a third (G1: 123
 * instead of 360 columns/s).
 * grt_set_deterministic(-1) returns control to the environment variable. */
EXTERN int grt_set_deterministic(int on);
EXTERN int grt_deterministic(void);

/* ---- batched columns ------------------------------------------------------------- */
typedef struct GrtColumns
{
    int ncol;
    int num_levels;
    fp_t const *pressure;               /* [ncol][V] mb, TOA first (as calculate_optical_depth) */
    fp_t const *temperature;            /* [ncol][V] K */
    fp_t const *layer_temperature;      /* [ncol][V-1] K */
    fp_t const *surface_temperature;    /* [ncol] K */
    fp_t const *molecule_ppmv;          /* [ncol][num_molecules][V], add_molecule order */
    fp_t const *cfc_ppmv;               /* [ncol][num_cfcs][V], add_cfc order (may be NULL) */
    fp_t const *cia_ppmv;               /* [ncol][NUM_CIAS][V] by CiaId_t (may be NULL) */
    fp_t const *cos_zenith;             /* [ncol] */
    fp_t const *total_solar_irradiance; /* [ncol] W m-2 */
} GrtColumns_t;

/* launch.c:40-226 for ncol columns in one launch; tau_dev is DEVICE memory [ncol][L][n]. */
EXTERN int grt_optical_depth_batch(GasOptics_t *gas_optics, GrtColumns_t const *columns,
                                   fp_t *tau_dev);

/* ---- clear-sky flux pipeline (driver.c:360-424 + 285-356 with -integrated) -------- */
#define GRT_FLUXES_PER_BAND 6   /* up TOA, up surface, up user level, down TOA, down surface, down user level */
#define GRT_FLUXES_PER_COLUMN (2*GRT_FLUXES_PER_BAND)   /* longwave six, then shortwave six */

typedef struct GrtPipeline GrtPipeline_t;

/* lw_gas / sw_gas: gas-optics objects on the longwave / shortwave grids (either may be
   NULL to skip that band).  emissivity [n_lw], albedo [n_sw] (direct == diffuse, as
   driver.c:118-119) and solar [n_sw] are host arrays copied once. */
EXTERN int grt_pipeline_create(GrtPipeline_t **pipeline, GasOptics_t *lw_gas, GasOptics_t *sw_gas,
                               int max_columns, int user_level, fp_t const *emissivity,
                               fp_t const *albedo, fp_t const *solar_flux);
/* keep_spectra = 0 (what grt_pipeline_create does): production form -- the solvers form Rayleigh and the optics
   combination in registers from tau_gas, keep nothing spectral and integrate in-kernel; device memory per column is
   tau_gas and 6 x nblocks partial sums -- instead of four optics and two flux arrays.  The shortwave solver runs ONE
   sweep from the top when user_level is -1, 0 or the surface; with a user level in between (or GRT_SW_TWO_SWEEPS=1 in the
   environment) it takes the reference's two sweeps and parks, between them, [2 V + 5 L][n] rows per column (422 rows at
   60 layers: 1.35 GB for 8 columns of 50 000 points) in a block allocated at the first such launch.  (api.Pipeline in Python defaults to
   spectral=True, i.e. keep_spectra = 1, because the parity tests want spectra; this C entry point defaults to 0.)
   keep_spectra = 1: tau, omega, g and flux_up/down are materialised as the reference's calls would leave them
   (grt_pipeline_views; parity tests, spectral output). */
EXTERN int grt_pipeline_create_ex(GrtPipeline_t **pipeline, GasOptics_t *lw_gas, GasOptics_t *sw_gas,
                                  int max_columns, int user_level, fp_t const *emissivity,
                                  fp_t const *albedo, fp_t const *solar_flux, int keep_spectra);
EXTERN int grt_pipeline_destroy(GrtPipeline_t **pipeline);

/* Enqueue the whole hot path for columns->ncol (<= max_columns) columns and write the
   integrated fluxes [ncol][GRT_FLUXES_PER_COLUMN] to fluxes_dev (DEVICE memory).
   Asynchronous on the library stream; grt_pipeline_sync() waits for it. */
EXTERN int grt_pipeline_run(GrtPipeline_t *pipeline, GrtColumns_t const *columns, fp_t *fluxes_dev);
EXTERN int grt_pipeline_sync(GrtPipeline_t *pipeline);
/* The HIP stream every kernel of this device is enqueued on (for event timing). */
EXTERN void *grt_pipeline_stream(GrtPipeline_t *pipeline);
/* Device views of the last run's spectral arrays (for parity tests): band 0 = lw, 1 = sw.  tau_gas always; the rest
   only on a pipeline created with keep_spectra = 1 (GRTCODE_VALUE_ERR otherwise).  (keep_spectra = 0: the shortwave
   solver adds the spectral tables' part of tau -- continua, CFC, CIA -- itself, from tables it reads once per grid point;
   asking for tau_gas queues, once per run, the small kernel that adds that part to the array: the same doubles a
   gas-optics call delivers.  Asynchronous on the pipeline's stream like the run.) */
EXTERN int grt_pipeline_views(GrtPipeline_t *pipeline, int band, fp_t **tau_gas, fp_t **tau,
                              fp_t **omega, fp_t **g, fp_t **flux_up, fp_t **flux_down);

/* ---- broadband flux profiles and heating rates ------------------------------------------
 * The same batch as grt_pipeline_run, with the broadband flux at EVERY level and the heating rate of every layer:
 *   level_fluxes_dev [ncol][GRT_PROFILE_ROWS_PER_COLUMN][V]: longwave up, longwave down, shortwave up, shortwave down,
 *                    each over the levels top first, W m-2 (required);
 *   heating_dev      [ncol][GRT_HEATING_ROWS_PER_COLUMN][V-1]: longwave, shortwave, K day-1, positive for warming (may be
 *                    NULL): layer j, between levels j and j + 1,
 *                    H_j = (GRT_GRAVITY/GRT_SPECIFIC_HEAT_AIR) ((dn_j - up_j) - (dn_{j+1} - up_{j+1}))/(100 (p_{j+1} - p_j))
 *                          x 86 400 s day-1,  p the level pressures in mb (x 100: Pa);
 *   fluxes_dev       [ncol][GRT_FLUXES_PER_COLUMN], as grt_pipeline_run writes it, from rows 0, L and the user level (may
 *                    be NULL).
 * All DEVICE memory; asynchronous on the pipeline's lane like grt_pipeline_run.  A band whose gas-optics object is NULL
 * gives zero rows.  The production form (keep_spectra = 0) writes no spectra: each level is summed across the spectrum
 * inside the solvers, and per band [max_columns][2 V][nblocks] partial sums (24 MB for 64 columns of a 50 000-point
 * band at 61 levels) are allocated at the first call.  Its shortwave solver always takes the two sweeps of the
 * reference and so needs the park block of the two-sweep form ([2 V + 5 L][n] per column: allocated at the first call
 * too, 10.8 GB for 64 columns of the 1 cm-1 band): the upward flux at the top is then the two-sweep form's, within
 * 1e-13 relative of the one-sweep form grt_pipeline_run takes by default.  Rows 0, L and the user level are, bit for
 * bit, those of grt_pipeline_run (shortwave: with GRT_SW_TWO_SWEEPS=1) in the deterministic mode.  keep_spectra = 1:
 * the same outputs from the materialised spectra, integrated row by row.  GRTCODE_VALUE_ERR for ncol outside
 * 1 .. max_columns, a NULL level_fluxes_dev, fewer than 2 levels. */
#define GRT_PROFILE_ROWS_PER_COLUMN 4    /* LW up, LW down, SW up, SW down; each [V], levels TOA first, W m-2 */
#define GRT_HEATING_ROWS_PER_COLUMN 2    /* LW, SW; each [V-1], K day-1 */
#define GRT_GRAVITY 9.80665              /* m s-2 */
#define GRT_SPECIFIC_HEAT_AIR 1004.64    /* J kg-1 K-1, dry air at constant pressure */
EXTERN int grt_pipeline_run_profiles(GrtPipeline_t *pipeline, GrtColumns_t const *columns,
                                     fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev);

/* ---- all-sky (cloudy, aerosol-free) fluxes ------------------------------------------------------------------------
 * driver.c:474-597 with one subcolumn: the clear-sky pass of grt_pipeline_run, then the same solvers on
 * add_optics({gas, Rayleigh, liquid cloud, ice cloud}).  The cloud optics come per band, as the clouds library
 * computes them before it spreads them onto a grid (clouds_lib.h: grt_clouds_band_optics, grt_clouds_bands); the
 * pipeline never calls that library.  Separate longwave and shortwave sets: the driver draws the subcolumns once per pass.
 * A grid point j takes the bands of the value driver.c:476-488 passes for it -- max(w0 - dw, 0) for j = 0, the midpoint
 * of the centres j - 1 and j otherwise -- under optics_utils.c:118-169's rules: bands written in ascending order, later
 * ones overwriting earlier ones; the first point at or above a band's lower limit up to, not including, the last point
 * at or below its upper limit; band 0 extended down; a parametrisation's own last band extended up (the ice's only when
 * num_ice_bands == num_liquid_bands); ice band b mapped with the ice limits for b < num_liquid_bands only.  A point no
 * band covers has no cloud (the reference leaves whatever the arrays held there).  Layer optical depth =
 * extinction x thickness.  All arrays are HOST memory, read during the call. */
typedef struct GrtClouds
{
    int num_liquid_bands;               /* B >= 1 */
    int num_ice_bands;                  /* >= B */
    fp_t const *liquid_band_lo, *liquid_band_hi;   /* [B] cm-1 */
    fp_t const *ice_band_lo, *ice_band_hi;         /* [num_ice_bands] cm-1 */
    fp_t const *thickness;              /* [ncol][L] m */
    fp_t const *lw_liquid, *lw_ice;     /* [ncol][3][B][L]: extinction m-1, single-scattering albedo, asymmetry */
    fp_t const *sw_liquid, *sw_ice;     /* [ncol][3][B][L] */
} GrtClouds_t;

#define GRT_ALLSKY_FLUXES_PER_COLUMN (2*GRT_FLUXES_PER_COLUMN)   /* clear-sky twelve, then all-sky twelve */

/* fluxes_dev [ncol][GRT_ALLSKY_FLUXES_PER_COLUMN] (DEVICE memory): values 0-11 are exactly what grt_pipeline_run writes,
   values 12-23 the all-sky set in the same order.  Same solvers, surface inputs, user level and shortwave sweep rule as
   grt_pipeline_run.  The production form (keep_spectra = 0) forms the cloud terms in the solver kernels from the band
   tables (GRT_TAG_ALLSKY_LW and _SW); the materialised form spreads them into [ncol][L][n] arrays, adds the four objects with
   add_optics' kernel and runs the spectral solvers: afterwards grt_pipeline_views shows the all-sky pass's tau, omega, g
   and fluxes.  GRTCODE_VALUE_ERR, with nothing launched, for: clouds NULL, num_liquid_bands < 1, num_ice_bands <
   num_liquid_bands, a NULL array (the band limits, thickness and the two sets of each band the pipeline has), ncol outside
   1 .. max_columns.  Asynchronous on the pipeline's lane like grt_pipeline_run. */
EXTERN int grt_pipeline_run_allsky(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtClouds_t const *clouds,
                                   fp_t *fluxes_dev);

/* ---- all-sky level fluxes and heating rates ----------------------------------------------------------------------
 * grt_pipeline_run_profiles and grt_pipeline_run_allsky together: the same batch and cloud inputs as
 * grt_pipeline_run_allsky, with the broadband flux at every level and the heating rate of every layer of the clear-sky
 * pass and of the all-sky pass.  Each column's block of every output is the clear-sky set, laid out exactly as
 * grt_pipeline_run_profiles writes it, followed by the all-sky set in the same layout:
 *   level_fluxes_dev [ncol][GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN][V]: clear LW up, LW down, SW up, SW down, then the same
 *                    four rows all-sky (required);
 *   heating_dev      [ncol][GRT_ALLSKY_HEATING_ROWS_PER_COLUMN][V-1]: clear LW, clear SW, all-sky LW, all-sky SW, K day-1,
 *                    grt_pipeline_run_profiles' formula and constants (may be NULL);
 *   fluxes_dev       [ncol][GRT_ALLSKY_FLUXES_PER_COLUMN], grt_pipeline_run_allsky's layout, from rows 0, L and the user
 *                    level of each set (may be NULL).
 * All DEVICE memory; asynchronous on the pipeline's lane.  One gas-optics launch per band serves both passes; the cloud
 * band maps, tables and subcolumn rule are grt_pipeline_run_allsky's; the shortwave always takes the reference's two
 * sweeps, as grt_pipeline_run_profiles does; a band whose gas-optics object is NULL gives zero rows.  The production form
 * (keep_spectra = 0) solves the all-sky pass in the profile form of the solvers with the cloud objects formed inside
 * (GRT_TAG_ALLSKY_LW and _SW); its partial sums, park block and cloud buffers are those grt_pipeline_run_profiles and
 * grt_pipeline_run_allsky allocate, shared by the two passes in stream order.  keep_spectra = 1: the spectra of both
 * passes, integrated row by row; afterwards grt_pipeline_views shows the all-sky pass.  In the deterministic mode the
 * clear-sky set is, bit for bit, grt_pipeline_run_profiles', and rows 0, L and the user level of the all-sky set are
 * grt_pipeline_run_allsky's (shortwave: with GRT_SW_TWO_SWEEPS=1).  GRTCODE_VALUE_ERR, with nothing launched, for what
 * either of the two refuses: a NULL level_fluxes_dev, fewer than 2 levels, clouds NULL, num_liquid_bands < 1,
 * num_ice_bands < num_liquid_bands, a NULL array in the cloud inputs, ncol outside 1 .. max_columns. */
#define GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN (2*GRT_PROFILE_ROWS_PER_COLUMN)   /* 8: clear sky, then all-sky */
#define GRT_ALLSKY_HEATING_ROWS_PER_COLUMN (2*GRT_HEATING_ROWS_PER_COLUMN)   /* 4: clear sky, then all-sky */
EXTERN int grt_pipeline_run_allsky_profiles(GrtPipeline_t *pipeline, GrtColumns_t const *columns,
                                            GrtClouds_t const *clouds, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                            fp_t *fluxes_dev);

/* ---- all-sky fluxes averaged over several cloud subcolumns ----------------------------------------------------------
 * driver.c:474-597 with num_subcolumns = S: per column, S draws of the cloud objects, each added to gas and Rayleigh and
 * solved, the spectral fluxes of the S solves summed and divided by S before they are integrated.  The clouds come as
 * grt_pipeline_run_allsky takes them but for the four optics sets, which hold S draws per column:
 * lw_liquid, lw_ice, sw_liquid, sw_ice [ncol][S][3][B][L], subcolumn s of column c at (c S + s) 3 B L; thickness stays
 * [ncol][L].  Two forms:
 *   level_fluxes_dev == NULL (six rows): fluxes_dev [ncol][GRT_ALLSKY_FLUXES_PER_COLUMN] (required) in
 *                    grt_pipeline_run_allsky's layout -- values 0-11 its clear-sky set, values 12-23 the subcolumn mean of
 *                    the all-sky set; grt_pipeline_run's shortwave sweep rule;
 *   level_fluxes_dev != NULL (profiles): grt_pipeline_run_allsky_profiles' layouts -- level_fluxes_dev
 *                    [ncol][GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN][V], heating_dev [ncol][GRT_ALLSKY_HEATING_ROWS_PER_COLUMN][V-1]
 *                    and fluxes_dev [ncol][GRT_ALLSKY_FLUXES_PER_COLUMN] (both may be NULL) -- the all-sky rows the
 *                    subcolumn means, the heating rates and six rows formed from those mean level fluxes; the shortwave
 *                    always takes two sweeps.
 * All DEVICE memory; asynchronous on the pipeline's lane.  One gas-optics launch per band serves the clear-sky pass and
 * all S subcolumns; band maps, tables and cloud rules are grt_pipeline_run_allsky's.  The mean is taken in a fixed
 * order: per subcolumn the blocks as the other entry points add them, then the subcolumns s = 0 .. S - 1, then one
 * division by S; with S = 1 every value is, bit for bit, grt_pipeline_run_allsky's or grt_pipeline_run_allsky_profiles'.
 * The production form (keep_spectra = 0) solves all S subcolumns of a band in one launch of the subcolumn instance of the
 * all-sky solver (GRT_TAG_ALLSKY_LW / _SW; the shortwave's two-sweep forms in as many launches as the park block of
 * max_columns columns needs) and reduces with a deterministic kernel (GRT_TAG_SUBCOLUMN_MEAN); it allocates per band
 * [max_columns][S][6 or 2 V][blocks] partial sums at the first call that needs more than it holds, and no larger park
 * block.  keep_spectra = 1: driver.c's loop literally -- per subcolumn the all-sky optics, the spectral solver and the
 * sum of its fluxes; afterwards grt_pipeline_views shows the last subcolumn's tau, omega, g and the mean fluxes.
 * GRTCODE_VALUE_ERR, with nothing launched and the outputs untouched, for: num_subcolumns outside
 * 1 .. GRT_MAX_SUBCOLUMNS, level_fluxes_dev and fluxes_dev both NULL, fewer than 2 levels in the profile form, and what
 * grt_pipeline_run_allsky refuses in clouds and ncol. */
#define GRT_MAX_SUBCOLUMNS 64
EXTERN int grt_pipeline_run_subcolumns(GrtPipeline_t *pipeline, GrtColumns_t const *columns,
                                       GrtClouds_t const *clouds, int num_subcolumns,
                                       fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev);

/* ---- cloud subcolumns sampled on the device from cloud fields ------------------------------------------------------
 * What grt_pipeline_run_subcolumns takes ready-made, made on the device: the band optics of S cloud subcolumns per column
 * and pass from what a model holds -- cloud fraction, liquid and ice water content, overlap parameter, temperature.  One
 * sample (column, pass, subcolumn, band) is one sample_subcolumn of the clouds library followed by its pade_band of liquid
 * and ice for every layer (clouds/stochastic_clouds.c:11-28, 94-120, incomplete_beta.c:32-64, clouds_lib.c:47-82,
 * cloud_pade_optics.c:152-213), operation for operation in double with no contraction: L rank values and L - 1 decision
 * values are drawn; for ascending i, rank[i+1] = rank[i] where decide[i] <= overlap[i] (copies cascade); a layer is
 * cloudy where rank > 1 - cf, strictly; the three beta lookups take the segment with the first x_i > at (the last one
 * beyond the table), slope first, then intercept; the water PDF is (5, 5); the ice radius is the size of the layer's
 * temperature class / 2; a radius no size regime holds, or a content that is not > 0, gives three zeros.  A fresh
 * subcolumn is drawn for every band, as the reference does.  A cloudy layer with no water at all gives NaN contents and
 * therefore zero optics, as in the library.  The pipeline never links libclouds.a (a site may substitute the reference's
 * own), so the parametrisation arrives as data: */
typedef struct GrtCloudPhase
{
    int nband, nsize, np, nq;           /* bands, size regimes, numerator and denominator coefficients */
    fp_t const *band_lo, *band_hi;      /* [nband] cm-1 */
    fp_t const *size_lo, *size_hi, *size_ref;   /* [nsize] microns */
    fp_t const *coef[6];                /* ext_p, ext_q, ssa_p, ssa_q, asy_p, asy_q: [band][size][coefficient] */
} GrtCloudPhase_t;
/* The three tables as the clouds library holds them after loading, HOST arrays read by grt_cloud_sampler_create alone:
   the Pade numbers already rounded to single precision (pade_load), the beta tables with x ascending and shapes up to 6. */
typedef struct GrtCloudModel
{
    int num_shape, num_x;               /* beta tables: shape parameters 1 .. num_shape (>= 6), abscissae (>= 2) */
    fp_t const *x;                      /* [num_x] */
    fp_t const *value, *inverse;        /* [q - 1][p - 1][x] */
    GrtCloudPhase_t liquid, ice;        /* ice.nband >= liquid.nband = B, whose bands drive the loop */
} GrtCloudModel_t;
typedef struct GrtCloudSampler GrtCloudSampler_t;
/* uploads the tables once; GRTCODE_VALUE_ERR for a NULL argument or array, shapes outside the ranges above, x that
   descends */
EXTERN int grt_cloud_sampler_create(GrtCloudSampler_t **sampler, Device_t device, GrtCloudModel_t const *model);
EXTERN int grt_cloud_sampler_destroy(GrtCloudSampler_t **sampler);

/* Where the draws come from.
 *   uniforms != NULL: from the caller, HOST [ncol][2][S][B][2 L - 1], in libc's order for a driver with num_subcolumns =
 *     S -- per column the longwave pass, then the shortwave pass; per pass S subcolumns; per subcolumn B bands; per band L
 *     ranks, then L - 1 decisions.  The parity hook, and the way to reproduce a rand()-driven run (rand()/RAND_MAX).
 *   uniforms == NULL: from Philox4x32-10 on the device.  Key (seed's low 32 bits, seed's high 32 bits); counter (layer i,
 *     band, pass GRT_MAX_SUBCOLUMNS + s, column_offset + c -- its low 32 bits); the four words r0 .. r3 of that ONE call
 *     give layer i's rank, ((r0 >> 5) 2^26 + (r1 >> 6)) 2^-53, and the decision of the pair (i, i + 1) the same way from
 *     (r2, r3).  Both lie in [0, 1), where the reference's rand()/RAND_MAX lie in [0, 1].  A column's clouds then depend
 *     on the seed and its global index alone: not on the batch it is in, the rank that holds it or the order of calls. */
typedef struct GrtCloudFields
{
    int ncol, num_layers;
    int num_subcolumns;                 /* S, 1 .. GRT_MAX_SUBCOLUMNS */
    fp_t const *cloud_fraction;         /* [ncol][L], each in [0, 1] */
    fp_t const *liquid_content;         /* [ncol][L] g m-3, >= 0 */
    fp_t const *ice_content;            /* [ncol][L] g m-3, >= 0 */
    fp_t const *temperature;            /* [ncol][L] K; NULL (grt_pipeline_run_cloud_fields only): the columns' layer_temperature */
    fp_t const *thickness;              /* [ncol][L] m (grt_pipeline_run_cloud_fields only) */
    fp_t const *overlap;                /* [ncol][L-1] (calculate_overlap's alpha; not read when L == 1) */
    fp_t liquid_radius;                 /* microns (the driver passes 10.0) */
    uint64_t seed;
    int64_t column_offset;              /* global index of column 0 */
    fp_t const *uniforms;               /* [ncol][2][S][B][2 L - 1], or NULL: the generator */
} GrtCloudFields_t;

/* tables_dev (DEVICE memory) [4][S][ncol][3][B][L]: the sets lw_liquid, lw_ice, sw_liquid, sw_ice, each subcolumn-major
   with extinction m-1, single-scattering albedo and asymmetry per liquid band and layer -- what grt_pipeline_run_subcolumns
   leaves on the device after the thickness block.  One kernel (GRT_TAG_CLOUD_SAMPLER), one wavefront per sample; asynchronous on
   the device's current lane (the fields are copied out before the call returns).  GRTCODE_VALUE_ERR, with nothing
   launched and tables_dev untouched, for: a NULL sampler, fields, tables_dev or required array (temperature here); S
   outside 1 .. GRT_MAX_SUBCOLUMNS; ncol or num_layers < 1; a cloud fraction outside [0, 1] or not finite; a content that
   is negative or not finite. */
EXTERN int grt_cloud_sampler_run(GrtCloudSampler_t *sampler, GrtCloudFields_t const *fields, fp_t *tables_dev);

/* grt_pipeline_run_subcolumns with S = fields->num_subcolumns and the tables made by the sampler: its two output forms,
   layouts, sweep rules and subcolumn mean.  The band limits of the cloud maps are the sampler's model's; the kernel writes
   the tables straight into the pipeline's cloud buffer, and only the thickness crosses PCIe with the fields: no
   [S][ncol][3][B][L] set is formed on the host.  Everything after the tables is grt_pipeline_run_subcolumns' code: the
   result equals, bit for bit in the deterministic mode, grt_pipeline_run_subcolumns fed grt_cloud_sampler_run's tables.
   GRTCODE_VALUE_ERR, with nothing launched and the outputs untouched, for what grt_cloud_sampler_run refuses (temperature
   may be NULL here) and: a NULL thickness; fields->ncol != columns->ncol; ncol outside 1 .. max_columns; num_layers !=
   num_levels - 1; level_fluxes_dev and fluxes_dev both NULL; fewer than 2 levels in the profile form; a sampler of
   another device. */
EXTERN int grt_pipeline_run_cloud_fields(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtCloudSampler_t *sampler,
                                         GrtCloudFields_t const *fields, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                         fp_t *fluxes_dev);

/* ---- clear-sky fluxes with aerosols ------------------------------------------------------------------------------
 * driver.c:426-472: the clear-clean pass of grt_pipeline_run (gas and Rayleigh), then the same solvers on
 * add_optics({gas, Rayleigh, aerosol}), both on ONE gas-optics launch per band -- what aerosol direct forcing (the
 * difference of the two sets) needs.  The aerosol comes per band, layer and property (optical depth of the layer,
 * single-scattering albedo, asymmetry) on a coarse wavenumber grid of NA points shared by the columns, and is put on the
 * spectral grid as interpolate_to_grid(..., linear_sample, NULL) does (utilities.c:149-222, :235-246): a grid point w in
 * the interval x[j] < w <= x[j+1] takes m w + b, m = (y[j+1] - y[j])/(x[j+1] - x[j]), b = y[j] - m x[j].  A point with
 * w <= x[0] or w > x[NA-1] has NO aerosol here (tau = omega = g = 0; the reference leaves whatever its buffers held).
 * Then the sums of optics.c:138-145 over gas (omega = g = 0), Rayleigh (omega = 1, g = 0) and the aerosol, in that order,
 * and the solver with the clear-clean pass's surface inputs and user level.  num_points == 0: that band's aerosol set is
 * its clear-clean set, bit for bit, and its grid and optics are not read.  All arrays are HOST memory, read during the
 * call. */
typedef struct GrtAerosols
{
    int lw_num_points, sw_num_points;   /* NA of each band's aerosol grid; 0: no aerosol in that band */
    fp_t const *lw_grid, *sw_grid;      /* [NA] cm-1, strictly increasing, shared by the columns */
    fp_t const *lw_optics, *sw_optics;  /* [ncol][3][L][NA]: optical depth of the layer, albedo, asymmetry */
} GrtAerosols_t;

/* Two forms, in grt_pipeline_run_subcolumns' manner, the aerosol set where the all-sky set is there:
 *   level_fluxes_dev == NULL (six rows): fluxes_dev [ncol][GRT_ALLSKY_FLUXES_PER_COLUMN] (required) -- values 0-11 exactly
 *                    what grt_pipeline_run writes, values 12-23 the aerosol set in the same order; grt_pipeline_run's
 *                    shortwave sweep rule;
 *   level_fluxes_dev != NULL (profiles): grt_pipeline_run_allsky_profiles' layouts -- level_fluxes_dev
 *                    [ncol][GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN][V], heating_dev [ncol][GRT_ALLSKY_HEATING_ROWS_PER_COLUMN][V-1]
 *                    and fluxes_dev [ncol][GRT_ALLSKY_FLUXES_PER_COLUMN] (both may be NULL) -- the clear-clean set as
 *                    grt_pipeline_run_profiles writes it, then the aerosol set; the shortwave always takes two sweeps.
 * All DEVICE memory; asynchronous on the pipeline's lane.  The production form (keep_spectra = 0) forms the aerosol
 * object inside the aerosol instances of the fused solvers (GRT_TAG_AEROSOL_LW and _SW): the host turns each column's
 * [3][L][NA] into slope and intercept tables [3][NA-1][2][L] once (the divisions), a grid point reads its interval once
 * and each layer does six loads and three multiply-adds; nothing spectral is stored.  keep_spectra = 1: driver.c's
 * sequence literally -- the aerosol spread into [ncol][L][n] arrays, add_optics' kernel over the three objects, the
 * spectral solvers, the row-wise trapezoid; afterwards grt_pipeline_views shows the aerosol pass's tau, omega, g and
 * fluxes.  Allocated at the first call that needs them: the table staging (max_columns x 6 x L x (NA - 1) doubles per
 * band, host and device) and one int per grid point and band (rebuilt when a band's aerosol grid changes; the call then
 * waits for the lane); partial sums and the park block are those of the other entry points.  In the deterministic mode
 * the clear-clean set is, bit for bit, grt_pipeline_run's / grt_pipeline_run_profiles'; an aerosol of zeros gives the
 * clear-clean set in the aerosol rows, bit for bit, in every mode.  GRTCODE_VALUE_ERR, with nothing launched and the
 * outputs untouched, for: aerosols NULL; num_points of 1 or negative; a NULL grid or optics with num_points >= 2; a grid
 * that is not strictly increasing; level_fluxes_dev and fluxes_dev both NULL; fewer than 2 levels in the profile form;
 * ncol outside 1 .. max_columns.  A band whose gas-optics object is NULL ignores its aerosol fields and gives zero rows. */
EXTERN int grt_pipeline_run_aerosols(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtAerosols_t const *aerosols,
                                     fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev);

/* ---- clouds and aerosols in one call -----------------------------------------------------------------------------
 * What driver.c's column_calculation (driver.c:360-597) writes for a cloudy column with aerosols, and the set it lacks,
 * on ONE gas-optics launch per band: up to four sets per column, each solved once --
 *   GRT_SKY_CLEAN          gas + Rayleigh, grt_pipeline_run's set; always formed, whether or not the bit is given;
 *   GRT_SKY_AEROSOL        + aerosol: grt_pipeline_run_aerosols' second set (driver.c:426-472);
 *   GRT_SKY_CLOUD          + liquid and ice cloud, aerosol-free: grt_pipeline_run_subcolumns' second set
 *                          (driver.c:474-597), the mean over num_subcolumns draws;
 *   GRT_SKY_CLOUD_AEROSOL  + aerosol + liquid and ice cloud, the physically complete all-sky set: add_optics of
 *                          {gas, Rayleigh, aerosol, liquid, ice} -- the sums of optics.c:138-145 in that order, the aerosol
 *                          in slot 2 where driver.c:426-434 puts it, the clouds behind it --, the same solvers, the mean
 *                          over the same draws; every draw of a column takes that column's aerosol.
 * The sets that are asked for leave packed, in bit order, clean first.  With N = grt_pipeline_sky_set_count(sets) sets:
 *   level_fluxes_dev == NULL (six rows): fluxes_dev [ncol][N][GRT_FLUXES_PER_COLUMN] (required); grt_pipeline_run's
 *                    shortwave sweep rule;
 *   level_fluxes_dev != NULL (profiles): level_fluxes_dev [ncol][N][GRT_PROFILE_ROWS_PER_COLUMN][V], heating_dev
 *                    [ncol][N][GRT_HEATING_ROWS_PER_COLUMN][V-1] and fluxes_dev [ncol][N][GRT_FLUXES_PER_COLUMN] (both may
 *                    be NULL), each set as grt_pipeline_run_profiles writes its one; the shortwave always takes two sweeps.
 * All DEVICE memory; asynchronous on the pipeline's lane.  clouds: as grt_pipeline_run_subcolumns takes them, tables per
 * subcolumn; aerosols: as grt_pipeline_run_aerosols takes them; inputs that no requested set needs are not read.  A band
 * the pipeline lacks gives zeros in every set; a band that was given no aerosol (num_points == 0) runs its aerosol sets
 * without the object.  grt_pipeline_set_surface applies to every set.  The production form solves the complete set in
 * instances of the fused solvers that hold both joins (GRT_TAG_SKY_LW and _SW; the other sets count under their own
 * passes' tags); keep_spectra = 1 spreads the aerosol and the clouds and adds the five objects with add_optics' kernel,
 * and grt_pipeline_views afterwards shows the last set's (last subcolumn's) tau, omega, g.  In the deterministic mode
 * each set is, bit for bit, what the entry point named above writes for it; an aerosol of zeros makes the complete set
 * the cloud set and cloud-free tables make it the aerosol set, bit for bit, in every mode.  GRTCODE_VALUE_ERR, with
 * nothing launched and the outputs untouched, for: sky NULL; bits in `sets` outside the four; a cloud set without clouds;
 * an aerosol set without aerosols; num_subcolumns outside 1 .. GRT_MAX_SUBCOLUMNS with a cloud set; what
 * grt_pipeline_run_subcolumns refuses in the clouds and grt_pipeline_run_aerosols in the aerosols; both outputs NULL;
 * fewer than 2 levels in the profile form; ncol outside 1 .. max_columns.  A night column: GRTCODE_RANGE_ERR, as
 * everywhere. */
#define GRT_SKY_CLEAN          1u  /* gas + Rayleigh; always formed, whether or not the bit is given */
#define GRT_SKY_AEROSOL        2u  /* + aerosol                   (driver.c:426-472) */
#define GRT_SKY_CLOUD          4u  /* + liquid and ice cloud      (driver.c:474-597, aerosol-free) */
#define GRT_SKY_CLOUD_AEROSOL  8u  /* + aerosol + liquid and ice cloud */
#define GRT_SKY_MAX_SETS       4

typedef struct GrtSky
{
    GrtClouds_t const *clouds;       /* needed by the two cloud sets; tables per subcolumn as grt_pipeline_run_subcolumns takes them */
    GrtAerosols_t const *aerosols;   /* needed by the two aerosol sets */
    int num_subcolumns;              /* 1 .. GRT_MAX_SUBCOLUMNS: the cloud sets are the mean over that many draws */
    unsigned sets;
} GrtSky_t;

EXTERN int grt_pipeline_sky_set_count(unsigned sets);   /* 1 .. 4; 0 for bits outside the four */
EXTERN int grt_pipeline_run_sky(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev);

/* ---- the direct beam of every sky set -------------------------------------------------------------------------------
 * grt_pipeline_run_sky in every respect -- the sets and their packing order, both output forms, the shortwave sweep rule,
 * the surface in force, the input checks -- and with it the part of each set's downward shortwave flux that is still in
 * the direct solar beam.  With N = grt_pipeline_sky_set_count(sets):
 *   direct_fluxes_dev       [ncol][N][GRT_DIRECT_ROWS_PER_SET] (required): the direct beam at the top of the atmosphere, at
 *                           the surface and at the user level, W m-2; with user_level < 0 the user row is +0.0;
 *   direct_level_fluxes_dev [ncol][N][V] (profile form only; may be NULL): the direct beam at every level, top first.
 * The value is the reference's own dir_beam at that level (shortwave.c:306, :323): the running product, from the top, of
 * the layers' T_pure (meador_weaver_1980, shortwave.c:118-121 and :147-168, the optical-depth clamp of :137-145
 * included), times solar_flux[w] cos_zenith and the total solar irradiance as the other rows are (:401-405, :447-451),
 * integrated over the band with the same trapezoid.  Two things to know about it:
 *   - it is the DELTA-SCALED direct beam (Joseph, Wiscombe and Weinman 1976; shortwave.c:86-89): the optical depth of a
 *     layer is tau (1 - omega g^2), so the beam includes the forward-scattered peak, as in every delta-two-stream model; it
 *     is not what a pyrheliometer of narrow aperture sees under cloud;
 *   - the diffuse downward flux is down - direct, formed by the caller from the matching row of fluxes_dev or
 *     level_fluxes_dev.
 * A cloud set's value is the mean over its num_subcolumns draws, taken as the other rows take theirs: subcolumns 0 .. S - 1
 * in order, then one division by S.  sets == GRT_SKY_CLEAN with clouds and aerosols NULL is the clear-sky split on its own.
 * A pipeline without a shortwave band writes zeros to both direct outputs.  All DEVICE memory; asynchronous on the
 * pipeline's lane.  The production form takes the direct beam out of the solvers that compute the sets (instances of
 * their own, which also leave the beam of their sweep: three more rows, or V, beside the set's own partial sums; the
 * launches count under grt_pipeline_run_sky's tags); keep_spectra = 1 forms it from each set's tau, omega, g on the grid
 * with a kernel of its own (GRT_TAG_DIRECT_BEAM) and the row-wise trapezoid.  In the deterministic mode every output
 * grt_pipeline_run_sky also writes is grt_pipeline_run_sky's, bit for bit; the direct TOA row is the set's down TOA row;
 * rows 0, V - 1 and user_level of direct_level_fluxes_dev are the six-row form's three direct rows, whichever sweep rule
 * it ran under.  GRTCODE_VALUE_ERR, with nothing launched and every output untouched, for: direct NULL;
 * direct_fluxes_dev NULL; direct_level_fluxes_dev given in the six-row form (level_fluxes_dev NULL); everything
 * grt_pipeline_run_sky refuses.  A night column: GRTCODE_RANGE_ERR, as everywhere. */
#define GRT_DIRECT_ROWS_PER_SET 3   /* direct-beam downward shortwave flux at TOA, surface, user level; W m-2 */
typedef struct GrtDirectBeam
{
    fp_t *direct_fluxes_dev;        /* DEVICE [ncol][N][GRT_DIRECT_ROWS_PER_SET]; required */
    fp_t *direct_level_fluxes_dev;  /* DEVICE [ncol][N][V], levels top first; profile form only; may be NULL */
} GrtDirectBeam_t;

EXTERN int grt_pipeline_run_sky_direct(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                       GrtDirectBeam_t const *direct,
                                       fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev);

/* ---- the surface-temperature Jacobian of the longwave, of every sky set --------------------------------------------
 * grt_pipeline_run_sky in every respect -- the sets and their packing order, both output forms, the shortwave sweep rule,
 * the surface in force (the Jacobian takes that column's emissivity row), the input checks -- and with it the derivative
 * of each set's upward longwave flux with respect to the surface temperature, dF_up(level)/dT_surf, which a host model
 * that calls radiation less often than its surface changes uses to keep the longwave consistent with the surface
 * (Hogan and Bozzo 2015; RRTMG's idrv = 1; ecRad's lw_derivatives).  With N = grt_pipeline_sky_set_count(sets):
 *   jacobian_fluxes_dev       [ncol][N][GRT_JACOBIAN_ROWS_PER_SET] (required): the derivative at the top of the
 *                             atmosphere, at the surface and at the user level, W m-2 K-1; with user_level < 0 the user
 *                             row is +0.0;
 *   jacobian_level_fluxes_dev [ncol][N][V] (profile form only; may be NULL): the derivative at every level, top first.
 * The value is the exact derivative of the discrete four-stream solver, not a finite difference: the surface enters each
 * stream once (longwave.c:202, I_s = emis B(T_surf) + (1 - emis) I_s), every layer above multiplies the stream by its
 * extinction exp(c1[s] t), t = tau (1 - omega), and nothing else in the upward sweep depends on T_surf, so per grid point
 *   D_s(surface) = emis(w) dB/dT(T_surf, w),   D_s(level j) = D_s(level j + 1) exp(c1[s] t_j),
 *   J(level j, w) = (((0 + c2[0] D_0) + c2[1] D_1) + c2[2] D_2) + c2[3] D_3,
 * with dB/dT = B (x/T) e/(e - 1), x = c2 w/T, e = exp(x), and 0 where planck_law clamps x (x > 700); integrated over the
 * band with the same trapezoid as every other row.  The longwave has no scattering: the downward fluxes do not depend
 * on T_surf, their derivative is identically zero and is not returned.  A cloud set's value is the mean over its
 * num_subcolumns draws, taken as the other rows take theirs: subcolumns 0 .. S - 1 in order, then one division by S.
 * sets == GRT_SKY_CLEAN with clouds and aerosols NULL is the clear-sky Jacobian on its own.  A pipeline without a longwave
 * band writes zeros to both Jacobian outputs.  All DEVICE memory; asynchronous on the pipeline's lane.  The production
 * form takes the Jacobian out of the solvers that compute the sets (instances of their own, whose upward sweep carries
 * the four derivatives beside the four intensities: three more rows, or V, beside the set's own partial sums; the
 * launches count under grt_pipeline_run_sky's tags); keep_spectra = 1 forms it from each set's tau and omega on the grid
 * with a kernel of its own (GRT_TAG_SURFACE_JACOBIAN) and the row-wise trapezoid.  In the deterministic mode every output
 * grt_pipeline_run_sky also writes is grt_pipeline_run_sky's, bit for bit; rows 0, V - 1 and user_level of
 * jacobian_level_fluxes_dev are the six-row form's three rows; the surface row is the same double in every set of a
 * column.  GRTCODE_VALUE_ERR, with nothing launched and every output untouched, for: jacobian NULL; jacobian_fluxes_dev
 * NULL; jacobian_level_fluxes_dev given in the six-row form (level_fluxes_dev NULL); everything grt_pipeline_run_sky
 * refuses.
 * Not covered: the several-sun-angle entry points (the longwave does not depend on the sun: call this one beside them),
 * cloud fields sampled on the device, and spectral or per-bin Jacobians. */
#define GRT_JACOBIAN_ROWS_PER_SET 3   /* dF_up/dT_surf at TOA, surface, user level; W m-2 K-1 */
typedef struct GrtSurfaceJacobian
{
    fp_t *jacobian_fluxes_dev;        /* DEVICE [ncol][N][GRT_JACOBIAN_ROWS_PER_SET]; required */
    fp_t *jacobian_level_fluxes_dev;  /* DEVICE [ncol][N][V], levels top first; profile form only; may be NULL */
} GrtSurfaceJacobian_t;

EXTERN int grt_pipeline_run_sky_jacobian(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                         GrtSurfaceJacobian_t const *jacobian,
                                         fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev);

/* ---- longwave radiances at viewing angles, of every sky set ----------------------------------------------------------
 * grt_pipeline_run_sky's six-row form in every respect -- the sets and their packing order (N =
 * grt_pipeline_sky_set_count(sets)), the surface in force (a radiance takes that column's emissivity row), the input checks,
 * asynchronous on the pipeline's lane -- and with it the radiance an instrument sees along one line of sight: per column
 * A viewing angles, given as secants m = 1/cos(viewing zenith angle), and per angle two rows: the upward radiance at the
 * top of the atmosphere (a sounder's spectrum) and the downward radiance at the surface (an upward-looking
 * interferometer's).  The definition is the reference's own longwave recurrence: its four streams are radiances at the
 * Gauss-Legendre secants -c1[s] (longwave.c:160-168), and a radiance at secant m is the same recurrence with c1[s]
 * replaced by -m.  Per grid point w, with t_j = tau_j (1 - omega_j) (longwave.c:252) and e_j = exp(min((-m) t_j, 700)):
 *   downward from the top, I = 0, then for j = 0 .. L - 1: I <- (1 - e_j) P_j + I e_j, P_j = effective_planck(B(T_layer j),
 *   B(T_level j + 1), t_j): after the last layer I is the downward radiance at the surface;
 *   the surface, I <- emis B(T_surf) + (1 - emis) I (longwave.c:202: specular reflection of the same angle);
 *   upward for j = L - 1 .. 0 with P_j from T_level j: after layer 0 I is the upward radiance at the top.
 * Units: W m-2 sr-1 per cm-1, what planck_law returns; integrated over the band with the same trapezoid as every other
 * row: W m-2 sr-1.  Radiances at the four secants -c1[s], weighted ((0 + c2[0] R_0) + c2[1] R_1) + c2[2] R_2) + c2[3] R_3,
 * are the solver's flux at that point, bit for bit.  The brightness temperature of a point is T_b = c2 w / log1p(c1 w^3 /
 * I) with planck_law's constants, +0.0 where I <= 0.
 *   radiances_dev          [ncol][N][A][2] (required): band-integrated, up at the top then down at the surface;
 *   spectral_radiances_dev [ncol][N][A][2][n_lw] (may be NULL): the same at every grid point of the longwave band;
 *   brightness_dev         [ncol][N][A][2][n_lw] (may be NULL): their brightness temperatures, K.
 * fluxes_dev is grt_pipeline_run_sky's [ncol][N][12], or NULL: then no flux solver and no shortwave gas optics run at all,
 * only the longwave gas optics and the radiance kernel (a satellite simulation), columns->cos_zenith is not read and a
 * night column is not an error.  A cloud set's integrated radiance is the mean over its num_subcolumns draws, taken as
 * the other rows take theirs: draws 0 .. S - 1 in order, then one division by S.  A pipeline without a longwave band
 * writes zeros to every radiance output.  The radiances come from a kernel of their own (GRT_TAG_RADIANCE), queued behind
 * each set's longwave solver (with fluxes_dev NULL: in its place) on the solver's own arguments; in the deterministic mode
 * every output grt_pipeline_run_sky also writes is grt_pipeline_run_sky's, bit for bit, and an angle's values do not
 * depend on the other angles of the call.  GRTCODE_VALUE_ERR, with nothing launched and every output untouched, for:
 * radiances NULL; radiances_dev NULL; view_secant NULL; num_angles outside 1 .. GRT_MAX_VIEW_ANGLES; a secant that is
 * NaN, infinite or below 1; a spectral or brightness output together with a cloud set at num_subcolumns > 1; everything
 * grt_pipeline_run_sky refuses.
 * Not covered: the profile form and radiances at interior levels, per-bin radiances, shortwave (scattered solar)
 * radiances, and cloud fields sampled on the device (instrument channels, cloud sets of several draws among them:
 * grt_pipeline_run_sky_channels below). */
#define GRT_MAX_VIEW_ANGLES 16
#define GRT_RADIANCE_ROWS_PER_ANGLE 2      /* upward at the top of the atmosphere, downward at the surface */
typedef struct GrtRadiances
{
    int num_angles;                     /* A, 1 .. GRT_MAX_VIEW_ANGLES */
    fp_t const *view_secant;            /* HOST [ncol][A]: 1/cos(viewing zenith angle), finite and >= 1 */
    fp_t *radiances_dev;                /* DEVICE [ncol][N][A][2], band-integrated, W m-2 sr-1; required */
    fp_t *spectral_radiances_dev;       /* DEVICE [ncol][N][A][2][n_lw], per cm-1; may be NULL */
    fp_t *brightness_dev;               /* DEVICE [ncol][N][A][2][n_lw], K; may be NULL */
} GrtRadiances_t;
EXTERN int grt_pipeline_run_sky_radiances(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                          GrtRadiances_t const *radiances, fp_t *fluxes_dev);

/* ---- instrument-channel radiances and brightness temperatures, of every sky set -------------------------------------
 * grt_pipeline_run_sky_radiances in every respect -- the sets and their packing, the viewing angles, every output of
 * `radiances`, fluxes_dev NULL or not, the surface in force, the input checks, asynchronous on the pipeline's lane, both
 * forms of the pipeline -- and with it what an instrument channel measures: per column, set, viewing angle and row (the
 * upward radiance at the top of the atmosphere, then the downward one at the surface) the mean of the spectral radiance
 * weighted with the spectral response function (SRF) of each of C channels, reduced on the device so that no spectral
 * row has to leave it.  Channel c is the grid points i = first[c] + k, k = 0 .. count_c - 1 (count_c = offset[c + 1] -
 * offset[c]) of the longwave band with the weights W_k = weights[offset[c] + k], the SRF sampled on the grid:
 *   R_c = (sum_k W_k I(i)) / (sum_k W_k),      W m-2 sr-1 per cm-1,
 * I the radiance of grt_pipeline_run_sky_radiances at that point; sum_k W_k is summed on the host in index order.
 * Channels may overlap, repeat, come in any order and be one point wide; a weight may be negative (the side lobes of an
 * apodised line shape) as long as the channel's sum is > 0.  The brightness temperature of a channel is
 *   T_c = c2 v_c / log1p(c1 v_c^3 / R_c),      K,
 * with planck_law's constants, +0.0 where R_c <= 0, at v_c = center[c], or -- center NULL -- the centroid sum_k W_k w_i /
 * sum_k W_k of the grid's w_i = w0 + i dw: the monochromatic-equivalent temperature at the channel centre.  NO
 * band-correction coefficients are applied: an instrument team's (a, b) of T = a + b T_c is the caller's to apply.
 *   channel_radiances_dev  [ncol][N][A][2][C] (required);
 *   channel_brightness_dev [ncol][N][A][2][C] (may be NULL).
 * A cloud set's channel radiance is the mean over its num_subcolumns draws, taken as the integrated rows take theirs:
 * draws 0 .. S - 1 in order, then one division by S; its brightness temperature is that of the mean radiance.  Channel
 * outputs are therefore allowed with S > 1; radiances->spectral_radiances_dev and brightness_dev keep their S = 1 rule.
 * A pipeline without a longwave band writes zeros to both channel outputs (and does not look at first and offset's
 * range).  The sums are formed inside the radiance kernel (its channel form, GRT_TAG_RADIANCE) per channel and 128-point
 * solver block the channel has a point in, in a fixed order without atomics -- a channel's value does not depend on the
 * other channels, angles or columns of the call --, and finished by a kernel of one thread per output
 * (GRT_TAG_CHANNELS).  The call takes max_columns x S x A x 2 x P doubles of scratch at the first call that needs more, P
 * = grt_channel_pair_count(channels, n_lw); the device table of an instrument is kept and reused as long as first, offset,
 * weights and center hold the same values.  In the deterministic mode every output grt_pipeline_run_sky_radiances also
 * writes is grt_pipeline_run_sky_radiances', bit for bit.
 * grt_channel_pair_count: host code only.  P, the number of (channel, 128-point solver block) pairs in which a channel has
 * at least one point on a grid of num_points points; -1 for anything the entry point would refuse in `channels` (the
 * two output pointers are not looked at) and for num_points < 1.
 * GRTCODE_VALUE_ERR, with nothing launched and every output untouched, for: channels NULL; channel_radiances_dev NULL;
 * first, offset or weights NULL; num_channels outside 1 .. GRT_MAX_CHANNELS; offset[0] != 0 or offset not strictly
 * increasing; first[c] < 0 or first[c] + count_c > n_lw; a weight that is NaN or infinite; a channel's sum of weights not
 * finite or <= 0; a center that is NaN, infinite or <= 0; everything grt_pipeline_run_sky_radiances refuses.
 * Not covered: shortwave (scattered solar) radiances, radiances at interior levels, cloud fields sampled on the device,
 * the example drivers, band-correction coefficients. */
#define GRT_MAX_CHANNELS 16384
typedef struct GrtChannels
{
    int num_channels;              /* C, 1 .. GRT_MAX_CHANNELS */
    int const *first;              /* HOST [C]: grid index of the channel's first point in the longwave band */
    int const *offset;             /* HOST [C + 1]: offset[0] = 0, strictly increasing; channel c has offset[c+1]-offset[c] points */
    fp_t const *weights;           /* HOST [offset[C]]: the SRF sampled on the grid, channel after channel; any finite sign */
    fp_t const *center;            /* HOST [C] cm-1, finite and > 0, or NULL: the weighted centroid sum W w / sum W */
    fp_t *channel_radiances_dev;   /* DEVICE [ncol][N][A][2][C], W m-2 sr-1 per cm-1; required */
    fp_t *channel_brightness_dev;  /* DEVICE [ncol][N][A][2][C], K; may be NULL */
} GrtChannels_t;
EXTERN long long grt_channel_pair_count(GrtChannels_t const *channels, long long num_points);
EXTERN int grt_pipeline_run_sky_channels(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                         GrtRadiances_t const *radiances, GrtChannels_t const *channels, fp_t *fluxes_dev);

/* ---- channel transmittance profiles and contribution functions, of every sky set -----------------------------------
 * grt_pipeline_run_sky_channels in every respect -- the sets and their packing, the viewing secants, every output of
 * `radiances` and `channels`, fluxes_dev NULL or not, the surface in force, the input checks, asynchronous on the
 * pipeline's lane, both forms of the pipeline -- and with it, for the UPWARD RADIANCE AT THE TOP OF THE ATMOSPHERE only,
 * per column, set, viewing angle and channel the level-to-space transmittance profile (its differences are the weighting
 * function) and the contribution function: how much of that radiance comes from each layer, from the surface's emission
 * and from the reflected downwelling.  Per longwave grid point i, draw and viewing secant m, in the radiance kernel's own
 * expressions: t_j = tau_j (1 - omega_j); e_j = exp(min((-m) t_j, 700)); T_0 = 1, T_{j+1} = T_j e_j (level 0 the top,
 * level V - 1 the surface); P_j = effective_planck(B(T_layer j), B(T_level j), t_j), the upward sweep's; I_dn the downward
 * radiance at the surface as grt_pipeline_run_sky_radiances forms it; and V + 1 contribution rows
 *   K_j     = ((1 - e_j) P_j) T_j          layer j = 0 .. L - 1 (L = V - 1),
 *   K_L     = (emis B(T_surf)) T_L         the surface's emission,
 *   K_{L+1} = ((1 - emis) I_dn) T_L        the reflected downwelling (specular),
 * whose sum is the upward radiance of grt_pipeline_run_sky_radiances at that point up to rounding.  Both are linear in
 * the per-point values, so their SRF-weighted means are exact; with the W_k and sum of grt_pipeline_run_sky_channels
 *   transmittance[v][c] = sum_k W_k T_v(i) / sum_k W_k,      dimensionless,
 *   contribution[r][c]  = sum_k W_k K_r(i) / sum_k W_k,      W m-2 sr-1 per cm-1.
 *   transmittance_dev [ncol][N][A][V][C]     (may be NULL);
 *   contribution_dev  [ncol][N][A][V + 1][C] (may be NULL; not both).
 * A cloud set of S draws gives the mean over the draws 0 .. S - 1 in order, then one division by S; the profiles are
 * allowed with S > 1, as the channel outputs are.  A pipeline without a longwave band writes zeros to both.
 * A kernel of its own (GRT_TAG_WEIGHTING) runs behind the radiance kernel of grt_pipeline_run_sky_channels, whose launches
 * are queued unchanged: in the deterministic mode every output that call also writes is that call's, bit for bit.  It
 * makes the downward sweep only and sums each row per channel and 128-point solver block in ascending point index,
 * without atomics: a value does not depend on the other channels, angles or columns of the call, and repeated calls are
 * bit-identical in either mode.  A kernel of one thread per output finishes (GRT_TAG_WEIGHTING_FINISH).  Scratch, beside
 * grt_pipeline_run_sky_channels': max_columns x S x A x R x P doubles at the first call that needs more, P =
 * grt_channel_pair_count(channels, n_lw), S the draws of the call's cloud sets (1 without one), R the rows asked for: V
 * for the transmittances plus V + 1 for the contributions, 2 V + 1 for both.
 * GRTCODE_VALUE_ERR, with nothing launched and every output untouched, for: weighting NULL; both of its pointers NULL;
 * everything grt_pipeline_run_sky_channels refuses.
 * Not covered: the contributions to the downward radiance, observer levels inside the atmosphere, per-point (spectral)
 * profiles, shortwave, cloud fields sampled on the device, the example drivers. */
typedef struct GrtWeighting
{
    fp_t *transmittance_dev;   /* DEVICE [ncol][N][A][V][C], dimensionless; may be NULL */
    fp_t *contribution_dev;    /* DEVICE [ncol][N][A][V + 1][C], W m-2 sr-1 per cm-1; may be NULL */
} GrtWeighting_t;              /* not both NULL */
EXTERN int grt_pipeline_run_sky_weighting(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                          GrtRadiances_t const *radiances, GrtChannels_t const *channels,
                                          GrtWeighting_t const *weighting, fp_t *fluxes_dev);

/* ---- spectral and band-integrated fluxes ---------------------------------------------------------------------------
 * driver.c's output without -integrated (output_fluxes, driver.c:285-356): the six rows of grt_pipeline_run at EVERY grid
 * point, and -- where the caller gives bin edges -- the same rows integrated over wavenumber bins, for a batch of columns,
 * clear sky (clouds NULL) or clear sky and all-sky (clouds as grt_pipeline_run_allsky takes them).  sets = 1 without
 * clouds, 2 with them (the clear-sky set first, as grt_pipeline_run_allsky); n_lw, n_sw: the grid points of the
 * pipeline's two gas-optics objects, 0 for a band whose object is NULL (it takes no room).
 *   spectral_dev [ncol][sets][6 n_lw + 6 n_sw] (required): per set the longwave's six rows [6][n_lw], then the
 *                shortwave's [6][n_sw], in GRT_FLUXES_PER_BAND order (up TOA, up surface, up user level, down TOA, down
 *                surface, down user level), W m-2 per cm-1; with user_level < 0 the two user rows are zeros;
 *   binned_dev   [ncol][sets][6 lw_num_bins + 6 sw_num_bins], each band [6][num_bins] in the same row order, W m-2
 *                (required if either bin count is > 0, ignored otherwise): bin b of a band is the trapezoid over its
 *                grid points edges[b] .. edges[b + 1],  sum_{i = edges[b]}^{edges[b+1] - 1} 0.5 (f_i + f_{i+1}) dw;
 *                adjacent bins share their edge point, so contiguous bins add up to the bin over their union, and the
 *                single bin {0, n - 1} is the broadband value;
 *   fluxes_dev   [ncol][GRT_FLUXES_PER_COLUMN] without clouds, [ncol][GRT_ALLSKY_FLUXES_PER_COLUMN] with them (required):
 *                exactly what grt_pipeline_run / grt_pipeline_run_allsky write, from the same solver launches.
 * lw_edges, sw_edges: HOST arrays of num_bins + 1 strictly increasing grid-point indices in 0 .. n - 1 (NULL / 0: no bins
 * for that band).  All outputs are DEVICE memory; asynchronous on the pipeline's lane like grt_pipeline_run; the
 * shortwave sweep rule is grt_pipeline_run's.  The production form (keep_spectra = 0) runs the fused six-row solvers in a
 * form that also stores the six rows at every point; the bins are summed from those rows by a deterministic kernel
 * (GRT_TAG_BINS) in the fused solvers' association, so that a bin {0, n - 1} is, bit for bit, the matching fluxes_dev
 * value.  keep_spectra = 1: rows 0, L and the user level of the materialised fluxes, the same binning kernel, and
 * fluxes_dev from the row-wise trapezoid.  A new set of edges is uploaded (the call then waits for the lane); the bins'
 * partial sums, [max_columns][6][about num_bins + n/128] doubles per band, are allocated at the first call that needs
 * them.  GRTCODE_VALUE_ERR, with nothing launched, for: a NULL spectral_dev or fluxes_dev, num_bins < 0, bins with NULL
 * edges or a NULL binned_dev, edges not strictly increasing or outside 0 .. n - 1, bins for a band whose gas-optics
 * object is NULL, ncol outside 1 .. max_columns, and what grt_pipeline_run_allsky refuses in clouds. */
EXTERN int grt_pipeline_run_spectral(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtClouds_t const *clouds,
                                     int const *lw_edges, int lw_num_bins, int const *sw_edges, int sw_num_bins,
                                     fp_t *spectral_dev, fp_t *binned_dev, fp_t *fluxes_dev);

/* ---- level fluxes and heating rates per wavenumber bin ----------------------------------------------------------------
 * What a band model is compared against: every level's upward and downward flux, and every layer's heating rate,
 * integrated over wavenumber bins instead of over the whole grid, for a batch of columns, clear sky (clouds NULL) or clear
 * sky and all-sky (clouds as grt_pipeline_run_allsky takes them).  sets = 1 without clouds, 2 with them (the clear-sky set
 * first, as grt_pipeline_run_allsky_profiles).  lw_edges, sw_edges: as grt_pipeline_run_spectral takes them -- HOST arrays
 * of num_bins + 1 strictly increasing grid-point indices in 0 .. n - 1, adjacent bins sharing their edge point; NULL / 0:
 * no bins for that band, which is then not computed and takes no room; at least one band must have bins.
 *   band_levels_dev  [ncol][sets][2 lw_num_bins + 2 sw_num_bins][V] (required): per set the longwave's [2][lw_num_bins][V]
 *                    (upward, then downward), then the shortwave's [2][sw_num_bins][V]; W m-2, levels top first.  Bin b of
 *                    a level is the trapezoid sum_{i = edges[b]}^{edges[b+1] - 1} 0.5 (f_i + f_{i+1}) dw of that level's
 *                    spectral flux: contiguous bins add up to the bin over their union, and the single bin {0, n - 1} is
 *                    the broadband level flux;
 *   band_heating_dev [ncol][sets][lw_num_bins + sw_num_bins][V-1] (may be NULL), K day-1: grt_pipeline_run_profiles'
 *                    formula and constants on each bin's level fluxes.
 * Both are DEVICE memory; asynchronous on the pipeline's lane like grt_pipeline_run.  The shortwave always takes the
 * reference's two sweeps, as grt_pipeline_run_profiles does; one gas-optics launch per band serves both sets.  The
 * production form (keep_spectra = 0) runs the banded instances of the fused profile solvers: a point weights a level's
 * value with the trapezoid weight of each bin it belongs to, a workgroup that lies inside one bin does the profile form's
 * work, one that holds bin edges sums each level once per bin it holds; the partial sums, [max_columns][2 V][about
 * num_bins + n/128] doubles per band (allocated at the first call that needs them, shared with
 * grt_pipeline_run_spectral's), are added per bin in a fixed order (GRT_TAG_BAND_PROFILES, with the heating-rate kernel).  In the
 * deterministic mode the single bin {0, n - 1} per band gives grt_pipeline_run_profiles' level fluxes and heating rates
 * bit for bit, and with clouds grt_pipeline_run_allsky_profiles' two sets.  keep_spectra = 1: the spectral solvers, then
 * the same weights and sums on the [V][n] flux rows; afterwards grt_pipeline_views shows the last pass.  A new set of
 * edges is uploaded (the call then waits for the lane).
 * grt_pipeline_band_profile_bin_limit: the most bins that may have a point in one block of 128 consecutive grid points
 * (block k: points 128 k .. 128 k + 127), floor(65536 / (32 V)) -- a workgroup's wave sums, 2 V rows x 2 waves x 8 bytes
 * per bin, must fit the 64 KiB of LDS it gets; 33 at V = 61.  Bins of 128 or more points never come near it.
 * GRTCODE_VALUE_ERR, with nothing launched and the outputs untouched, for: a NULL band_levels_dev; what
 * grt_pipeline_run_spectral refuses in edges (bins for a band whose gas-optics object is NULL included); no bins in
 * either band; fewer than 2 levels; more bins in one block than the limit; ncol outside 1 .. max_columns; and what
 * grt_pipeline_run_allsky refuses in clouds. */
EXTERN int grt_pipeline_run_band_profiles(GrtPipeline_t *pipeline, GrtColumns_t const *columns,
                                          GrtClouds_t const *clouds, int const *lw_edges, int lw_num_bins,
                                          int const *sw_edges, int sw_num_bins, fp_t *band_levels_dev,
                                          fp_t *band_heating_dev);
EXTERN int grt_pipeline_band_profile_bin_limit(GrtPipeline_t const *pipeline);

/* ---- k-distributions of the layer optical depths ------------------------------------------------------------------------
 * What a band model is built from: inside each wavenumber bin and each layer, the distribution of the line-by-line
 * optical depth -- g(k) and the mean optical depth of each k-class, uniformly or source-weighted -- reduced on the device
 * next to the array, so that [ncol][L][n] doubles of tau (1.5 GB per 64 columns of the 1 cm-1 shortwave band) leave as
 * [ncol][L][bins][K] numbers.  The reduction, for one row tau[0 .. n - 1] on a grid of spacing dw:
 *   bins     num_bins + 1 strictly increasing grid-point indices, as grt_pipeline_run_spectral takes them; adjacent bins
 *            share their edge point;
 *   classes  K - 1 strictly increasing, finite class edges e[0 .. K - 2] in units of tau;
 *   weight   s[0 .. n - 1], each >= 0 and finite, or NULL: 1 (a Planck or solar curve, say).
 * For bin b and each of its points i = edges[b] .. edges[b + 1]:
 *   w_i = dw, 0.5 dw at the bin's two end points;  W_i = fl(w_i s_i) (w_i without a weight);  T_i = fl(W_i tau_i);
 *   class(i) = the number of class edges e_k <= tau_i, by plain double comparisons: a tau equal to an edge goes to the
 *   upper class; tau <= 0, tau below e[0] and NaN go to class 0; +inf goes to class K - 1.  No logarithm is taken.
 * Per (row, bin, class k): points, the number of the bin's points in class k; weight, the sum of their W_i; tau, the sum
 * of their T_i.  Each of the two sums is the plain left-to-right sum of its terms in increasing grid index, from +0.0,
 * every product rounded before it is added (no fused multiply-add), without floating-point atomics and without a tree; an
 * empty class gives 0, +0.0, +0.0.  The result is therefore a pure function of the inputs: bit-identical from run to run
 * in the default and in the deterministic mode, and what a sequential sum on the host (numpy's cumsum) gives, bit for bit.
 * From it: g at the upper edge of class k is cumsum(weight)/sum(weight); the class mean of tau is tau/weight; the sum of
 * tau over the classes is the bin's trapezoid integral of s tau.
 *
 * grt_kdist_rows: the primitive.  tau_dev [rows][n] is any DEVICE array (what grt_optical_depth_batch wrote, say);
 *   band's outputs are [rows][num_bins][K].  Asynchronous on the device's current lane.
 * grt_pipeline_run_kdist: stages the columns, runs, for each band that has bins, the gas optics once -- the whole of it,
 *   the spectral tables' part included: a following grt_pipeline_views(band, &tau_gas, ...) shows exactly the array that
 *   was reduced and queues nothing -- and reduces tau_gas with rows = ncol L: a band's outputs are [ncol][L][num_bins][K].
 *   No solver, no Rayleigh kernel and no clear-sky optics run; a band without bins is not computed at all (a call with
 *   longwave bins only never touches the shortwave line list); the surface in force, clouds, aerosols and the columns'
 *   sun angles play no part.  Asynchronous on the pipeline's lane like grt_pipeline_run.
 * grt_kdist_chunk_points: the points the kernel stages at a time (tests sit on its multiples).
 * One kernel (GRT_TAG_KDIST), one workgroup per (row, bin).  Bin edges, class edges and weights are uploaded when their
 * bytes differ from the last call's (the call then waits for the lane); the same inputs again cost nothing.  The
 * pipeline keeps them per band and frees them when it is destroyed; grt_kdist_rows keeps one set per device.
 * GRTCODE_VALUE_ERR, with nothing launched and the outputs untouched, for: a NULL kdist, band or class_edges; K outside
 * 2 .. GRT_KDIST_MAX_CLASSES; class edges that are not strictly increasing or not finite; everything
 * grt_pipeline_run_spectral refuses in edges (bins for a band whose gas-optics object is NULL included); no bins in
 * either band; a band with bins and all three outputs NULL; a weight that is negative or not finite; rows < 1, n < 2 or
 * a dw that is not positive and finite (grt_kdist_rows); ncol outside 1 .. max_columns; a lane other than the
 * pipeline's. */
#define GRT_KDIST_MAX_CLASSES 1024
typedef struct GrtKdistBand
{
    int const *edges;        /* HOST [num_bins + 1], as grt_pipeline_run_spectral's; NULL / 0: band not computed */
    int num_bins;
    fp_t const *weight;      /* HOST [n] spectral weight, >= 0 and finite, or NULL: 1 */
    int *points_dev;         /* DEVICE [rows][num_bins][K], or NULL */
    fp_t *weight_dev;        /* DEVICE [rows][num_bins][K], or NULL */
    fp_t *tau_dev;           /* DEVICE [rows][num_bins][K], or NULL */
} GrtKdistBand_t;
typedef struct GrtKdist
{
    int num_classes;         /* K: 2 .. GRT_KDIST_MAX_CLASSES */
    fp_t const *class_edges; /* HOST [K - 1], strictly increasing, finite */
    GrtKdistBand_t lw, sw;
} GrtKdist_t;

EXTERN int grt_kdist_rows(Device_t device, fp_t const *tau_dev, long long rows, long long n, fp_t dw,
                          int num_classes, fp_t const *class_edges, GrtKdistBand_t const *band);
EXTERN int grt_pipeline_run_kdist(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtKdist_t const *kdist);
EXTERN int grt_kdist_chunk_points(void);

/* ---- correlated k-distributions: every row of a group under one class map --------------------------------------------------
 * A correlated-k band model fixes one ordering of the spectral points per column and bin -- that of a reference layer, or
 * of the column's vertical optical depth -- and averages every layer's optical depth, the source weights and the fluxes
 * each g-point must carry over the same sets of points.  Here the ordering is the class of a key, kept on the device as a
 * map of 16-bit classes, and any rows are reduced under it.  The values are x[g][r][i]: group g of G (a column), row r of R
 * (a layer, the top one first, as in tau_gas [ncol][L][n]), grid point i of n.
 *   key   GRT_KDIST_KEY_ROW: key_i = x[g][key_row][i];  GRT_KDIST_KEY_SUM: key_i = (((+0.0 + x[g][0][i]) + x[g][1][i]) + ...)
 *         + x[g][R - 1][i], every add rounded, the rows in order, nothing contracted (a column's vertical optical depth);
 *   map   map[g][i] = class(key_i), an unsigned short, by grt_kdist_rows' rule and no other: the number of class edges
 *         e_k <= key_i; a NaN and anything below e[0] give 0, +inf gives K - 1.  It does not depend on bins.
 * The mapped reduction, with grt_kdist_rows' bins, w_i, W_i = fl(w_i s_i) and weight s: per group, bin b and class k,
 * points is the number of the bin's points with map[g][i] == k, weight the sum of their W_i and, per row r, tau the sum of
 * fl(W_i v[g][r][i]) over them -- each sum left to right in increasing grid index from +0.0, every product rounded before
 * it is added, no atomics, no tree: bit for bit a sequential sum on the host.  points and weight are the same for every
 * row and have no row axis.  A map entry >= K belongs to no class and is counted nowhere: the reduction never indexes by
 * it, so a bad map cannot write out of bounds.
 *
 * grt_kdist_class_map: map_dev [groups][n] from x_dev [groups][rows_per_group][n].  Asynchronous on the current lane.
 * grt_kdist_mapped_rows: row r of group g starts at values_dev + g group_stride + r n (group_stride in doubles, >=
 *   rows_per_group n); band's points_dev and weight_dev are [groups][num_bins][K], its tau_dev
 *   [groups][rows_per_group][num_bins][K].  The stride applies the call to grt_pipeline_run_spectral's spectral_dev
 *   [ncol][sets][6 n_lw + 6 n_sw]: the longwave rows with base spectral_dev, stride sets (6 n_lw + 6 n_sw) and 6 rows per
 *   group, the shortwave rows with base + 6 n_lw.  With weight NULL the class sums of a flux row are W m-2 per class: the
 *   line-by-line flux of each g-class.
 * grt_pipeline_run_kdist_correlated: grt_pipeline_run_kdist -- the staging, the whole gas optics of each band that has bins,
 *   no solver, grt_pipeline_views afterwards showing the array that was reduced, asynchronous on the pipeline's lane --
 *   with, per band, the map built from tau_gas with that band's key (kind; layer in 0 .. L - 1 with GRT_KDIST_KEY_ROW,
 *   ignored with GRT_KDIST_KEY_SUM) and every layer reduced under it: points_dev and weight_dev [ncol][num_bins][K],
 *   tau_dev [ncol][L][num_bins][K].  The class edges classify the key only.  With map_dev NULL the map lives in pipeline
 *   scratch (max_columns n shorts per band, allocated at the first call that needs it, freed with the pipeline); with
 *   map_dev given the caller keeps it for later grt_kdist_mapped_rows calls.
 * Two kernels (GRT_TAG_KDIST_MAP, GRT_TAG_KDIST_MAPPED), the latter one workgroup per (group, row, bin).
 * GRTCODE_VALUE_ERR, with nothing launched and the outputs untouched, for: everything grt_kdist_rows and
 * grt_pipeline_run_kdist refuse in classes, edges, bins, weights, dw, counts and lane; a NULL x_dev, values_dev, map_dev
 * (of the two rows calls) or keys; groups < 1, rows_per_group < 1 or n < 2; a key kind other than the two; key_row outside
 * 0 .. rows_per_group - 1 (layer outside 0 .. L - 1 for a band that has bins) with GRT_KDIST_KEY_ROW; group_stride <
 * rows_per_group n. */
enum { GRT_KDIST_KEY_ROW = 0, GRT_KDIST_KEY_SUM = 1 };

EXTERN int grt_kdist_class_map(Device_t device, fp_t const *x_dev, long long groups, long long rows_per_group,
                               long long n, int key_kind, long long key_row, int num_classes,
                               fp_t const *class_edges, unsigned short *map_dev);
EXTERN int grt_kdist_mapped_rows(Device_t device, fp_t const *values_dev, long long group_stride,
                                 unsigned short const *map_dev, long long groups, long long rows_per_group,
                                 long long n, fp_t dw, int num_classes, GrtKdistBand_t const *band);

typedef struct GrtKdistKey
{
    int kind;                /* GRT_KDIST_KEY_ROW or GRT_KDIST_KEY_SUM */
    int layer;               /* the key layer, 0 .. L - 1 (GRT_KDIST_KEY_ROW) */
    unsigned short *map_dev; /* DEVICE [ncol][n], or NULL: the map stays in pipeline scratch */
} GrtKdistKey_t;
typedef struct GrtKdistKeys
{
    GrtKdistKey_t lw, sw;
} GrtKdistKeys_t;
EXTERN int grt_pipeline_run_kdist_correlated(GrtPipeline_t *pipeline, GrtColumns_t const *columns,
                                             GrtKdist_t const *kdist, GrtKdistKeys_t const *keys);

/* ---- flux solves of a correlated-k model on its g-classes -------------------------------------------------------------------
 * The other half of the loop: the clear-clean fluxes of the band model that the class map defines, every level, per
 * (bin, class) and per bin, next to grt_pipeline_run_band_profiles' line-by-line bins of the same columns.  Per band,
 * column c, bin b with points i = edges[b] .. edges[b + 1], w_i = dw (0.5 dw at the bin's two ends), v_i = w0 + i dw as
 * the solvers form it, class k = the bin's points with map[c][i] == k.  Every sum below is the mapped reduction's: left to
 * right in grid order from +0.0, each product rounded before it is added, no atomics, no tree, nothing contracted.  No
 * spectral weight.
 *   map, W, T  exactly grt_pipeline_run_kdist_correlated's: the map of the band's key over tau_gas -- or map_given_dev,
 *              used as is, the key ignored --, W[c][b][k] = sum w_i, T[c][l][b][k] = sum fl(w_i tau_i), grt_kdist_mapped_rows'
 *              bits.
 *   sources    sum fl(w_i x_i) per class, [ncol][R][bins][K].  Longwave, R = 2 V + 1: rows 0 .. V - 1 x = B(t_levels[c][v],
 *              v_i), rows V .. 2 V - 2 x = B(t_layers[c][l], v_i), row 2 V - 1 x = B(t_surf[c], v_i), B the longwave
 *              solver's own Planck function; row 2 V x = the emissivity in force at the point.  Shortwave, R = 4: row 0 the
 *              Rayleigh optical depth of one molecule per cm2 (the solvers' expression with n = 1), row 1 the solar
 *              curve, rows 2 and 3 the direct and the diffuse albedo in force.  The data rows are grt_kdist_mapped_rows of
 *              those rows, bit for bit; the Rayleigh row has no transcendental and is reproduced by a host restatement bit
 *              for bit.
 *   the solve  one g-point per (c, b, k) with W > 0.  Longwave: t_l = T[l]/W (gas only, omega = 0), the Planck terms and
 *              the emissivity row/W, then the longwave solver's two sweeps, operation for operation; the result per cm-1
 *              is multiplied by W last.  Shortwave: t_gas = T[l]/W, t_ray = fl(n_layer[c][l] row0)/W, combined as the
 *              clear-sky optics combine them, the layer's delta-Eddington properties with the column's cos_zenith and
 *              the diffuse cosine 0.5, the reference's two sweeps with the albedos row2/W, row3/W; scaled by row1
 *              cos_zenith, then by the column's total solar irradiance: the flux is linear in the solar term, so the class
 *              SUM of the solar curve goes in.  flux_up_dev, flux_down_dev [ncol][V][bins][K]: W m-2 per class.  A class of
 *              no points gives +0.0 at every level and solves nothing; so does, in the shortwave, a column with cos_zenith
 *              <= 0 (night columns are allowed in this call: cos_zenith <= 1 is all that is asked).
 *   bin sums   bin_up_dev, bin_down_dev [ncol][V][bins]: (((+0.0 + f[0]) + f[1]) + ...) + f[K - 1] over the classes.
 * What runs, asynchronously on the pipeline's lane, per band that has bins: the whole gas optics as grt_pipeline_run_kdist
 * runs it; the map kernel (GRT_TAG_KDIST_MAP) unless a map is given; the mapped reduction (GRT_TAG_KDIST_MAPPED); the source
 * sums (GRT_TAG_CK_SOURCES), the mapped kernel with the row's value computed at the point; the solve, one thread per
 * (column, bin, class), and behind it the bin sums where asked for (GRT_TAG_CK_LW / GRT_TAG_CK_SW, one bracket).  No
 * line-by-line solver, Rayleigh or clear-sky optics kernel runs; a band without bins is not computed at all; a following
 * grt_pipeline_views shows the tau_gas that was reduced.  Whatever of weight_dev, tau_dev, source_dev and the map the caller
 * leaves NULL lives in pipeline scratch (max_columns bins K (1 + L + R) doubles and max_columns n shorts per band),
 * allocated at the first call that needs it, freed with the pipeline.  Class edges and bin edges share
 * grt_pipeline_run_kdist's per-band block: the same classes and bins again cost a comparison.  The class edges classify
 * the key only: with a map given in every band that has bins, class_edges may be NULL.  A given map's entry >= K belongs
 * to no class, is counted nowhere and indexes nothing.
 * GRTCODE_VALUE_ERR, with nothing launched and the outputs untouched, for: everything grt_pipeline_run_kdist_correlated
 * refuses in classes, edges, bins, key, counts and lane; a NULL ck; no bins in either band; bins for a band whose gas-optics
 * object is NULL; a band with bins and flux_up_dev or flux_down_dev NULL; one of bin_up_dev, bin_down_dev without the other;
 * class_edges NULL while a band with bins has no given map. */
typedef struct GrtCkBand
{
    int const *edges;                      /* HOST [num_bins + 1], as grt_pipeline_run_kdist's; NULL / 0: band not computed */
    int num_bins;
    GrtKdistKey_t key;                     /* kind, layer, map_dev (DEVICE out [ncol][n], or NULL: pipeline scratch) */
    unsigned short const *map_given_dev;   /* DEVICE [ncol][n] or NULL; given: used as is, key ignored, map_dev not written */
    int *points_dev;                       /* DEVICE [ncol][num_bins][K], or NULL */
    fp_t *weight_dev;                      /* DEVICE [ncol][num_bins][K], or NULL */
    fp_t *tau_dev;                         /* DEVICE [ncol][L][num_bins][K], or NULL */
    fp_t *source_dev;                      /* DEVICE [ncol][R][num_bins][K], or NULL (R = 2 V + 1 longwave, 4 shortwave) */
    fp_t *flux_up_dev, *flux_down_dev;     /* DEVICE [ncol][V][num_bins][K]; both required for a band with bins */
    fp_t *bin_up_dev, *bin_down_dev;       /* DEVICE [ncol][V][num_bins], or NULL (both or neither) */
} GrtCkBand_t;
typedef struct GrtCkFluxes
{
    int num_classes;                       /* K: 2 .. GRT_KDIST_MAX_CLASSES */
    fp_t const *class_edges;               /* HOST [K - 1], or NULL where every band with bins is given its map */
    GrtCkBand_t lw, sw;
} GrtCkFluxes_t;
EXTERN int grt_pipeline_run_ck_fluxes(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtCkFluxes_t const *ck);

/* ---- per-column surface emissivity and albedo ----------------------------------------------------------------------
 * driver.c:101-117: each column's own surface emissivity and albedo, given on coarse wavenumber grids of NS points shared
 * by the columns and put on the band's grid as interpolate_to_grid(grid, x, y, NS, out, linear_sample,
 * constant_extrapolation) does (utilities.c:149-246, :77-92).  A grid point w = w0 + i dw takes
 *   y[0]                                    for w <= x[0],
 *   m_j w + b_j                             for x[j] < w <= x[j+1],  m_j = (y[j+1] - y[j])/(x[j+1] - x[j]),
 *                                           b_j = y[j] - m_j x[j]  (multiply, then add: no contraction),
 *   y[NS-2]                                 for w > x[NS-1]  (the reference hands its extrapolation the LAST SEGMENT, so
 *                                           the value above the grid is the one before the last; kept).
 * Once set, the surface holds for every later grt_pipeline_run* call on this pipeline -- every entry point, both passes
 * or sets of each, keep_spectra = 0 and 1 -- until it is replaced or cleared with surface == NULL; after a clear the
 * arrays given to grt_pipeline_create apply again, bit for bit.  A run with a surface set needs columns->ncol ==
 * surface->ncol: GRTCODE_VALUE_ERR otherwise, with nothing launched and the outputs untouched.  A band with a point
 * count of 0 keeps its creation-time array; a band whose gas-optics object is NULL ignores its fields.
 * The arrays are HOST memory, read during the call.  The host does the divisions once -- each column's [NS] becomes NS + 1
 * slope and intercept pairs, the two constant ranges as (0, y[0]) and (0, y[NS-2]) --, and a kernel (GRT_TAG_SURFACE) writes
 * each column's row on the device, one thread per column and grid point: a few kB cross PCIe instead of
 * [ncol][n_lw] + 2 [ncol][n_sw] doubles.  Asynchronous on the pipeline's lane like a run.  Allocated at the first call
 * that needs them: [max_columns][n] doubles per band (twice that for the shortwave when diffuse_albedo is given: without
 * it both beams read the direct rows), the small staging buffer, and one int per grid point and band (rebuilt when that
 * band's surface grid changes; the call then waits for the lane).
 * GRTCODE_VALUE_ERR, with nothing launched and the previous surface (or none) still in force, for: ncol outside
 * 1 .. max_columns; a point count that is 1 or negative; a NULL grid or value array where the count is >= 2; a grid that
 * is not strictly increasing; a knot value outside [0, 1] (the range grt_pipeline_create enforces).
 * In the deterministic mode, column c of a batch with a surface equals, bit for bit, a pipeline created with column c's
 * interpolated rows as its shared arrays; so does a surface of constant knots equal to the creation-time constants and a
 * run without a surface. */
typedef struct GrtSurface
{
    int ncol;
    int emissivity_num_points, albedo_num_points;   /* NS >= 2 each; 0: that band keeps the creation-time array */
    fp_t const *emissivity_grid, *albedo_grid;      /* [NS] cm-1, strictly increasing, shared by the columns */
    fp_t const *emissivity;                         /* [ncol][NS] */
    fp_t const *direct_albedo;                      /* [ncol][NS] */
    fp_t const *diffuse_albedo;                     /* [ncol][NS], or NULL: the direct one (driver.c:116-117) */
} GrtSurface_t;
EXTERN int grt_pipeline_set_surface(GrtPipeline_t *pipeline, GrtSurface_t const *surface);

/* ---- several sun angles per column on one gas-optics pass -----------------------------------------------------------
 * The clear-clean set (gas and Rayleigh) of grt_pipeline_run or grt_pipeline_run_profiles under Z sun angles per column:
 * a diurnal mean, a zenith sweep, a training set.  The optical depths do not depend on the sun, so each band's gas optics
 * run once per column; the longwave is solved once, the shortwave once per angle, and the shortwave rows that leave are
 * the weighted mean over the angles.  columns->cos_zenith is not read (it may be NULL); total_solar_irradiance stays per
 * column.  A cos_zenith <= 0 is a night sample: its shortwave rows are +0.0 and nothing is solved for it.  Two forms, in
 * grt_pipeline_run_subcolumns' manner:
 *   level_fluxes_dev == NULL (six rows): fluxes_dev [ncol][GRT_FLUXES_PER_COLUMN] in grt_pipeline_run's layout (may be NULL
 *                    when zenith_fluxes_dev is given: then neither the longwave nor the mean is formed); its shortwave
 *                    sweep rule;
 *   level_fluxes_dev != NULL (profiles): grt_pipeline_run_profiles' three layouts, the heating rates and the six rows
 *                    formed from the mean level fluxes; the shortwave always takes two sweeps.
 * The mean is taken in a fixed order: each angle's blocks as the other entry points add them, then the angles k = 0 ..
 * Z - 1; without weights the sum and one division by Z (night samples included), with weights sum w_k F_k, each product
 * rounded before it is added.  With Z = 1 and no weights every value is, bit for bit in the deterministic mode,
 * grt_pipeline_run's or grt_pipeline_run_profiles' for that cos_zenith.  A surface set with grt_pipeline_set_surface
 * applies; a pipeline without a shortwave band runs the longwave and zeroes the shortwave outputs.
 * The production form (keep_spectra = 0) solves the angles in the zenith instances of the shortwave solver, grid row =
 * (column, angle) -- the two-sweep forms in as many launches as the park block of max_columns columns needs -- or, six
 * rows in one sweep, in the shared-layer kernel, which walks the layers once for GRT_ZENITH_CHUNK angles (k_shortwave.hip;
 * GRT_ZENITH_SHARED=0 in the environment, read per call: the zenith instance instead, the same bits), all under
 * GRT_TAG_ZENITH_SW, and reduces with a deterministic kernel (GRT_TAG_ZENITH_MEAN); it allocates per band
 * [max_columns][Z][6 or 2 V][blocks] partial sums at the first call that needs more than it holds.  keep_spectra = 1:
 * the literal loop -- per angle the spectral solver and the row-wise trapezoid (a column's night angle runs on its last
 * day angle before it, else its first one after it, and is zeroed where the mean is taken); afterwards
 * grt_pipeline_views shows each column's last day angle's fluxes.
 * GRTCODE_VALUE_ERR, with nothing launched and the outputs untouched, for: num_zeniths outside 1 .. GRT_MAX_ZENITHS; a
 * NULL cos_zenith, or an entry that is NaN or above 1; a weight that is negative or NaN; fluxes_dev, level_fluxes_dev and
 * both per-angle outputs all NULL; zenith_level_fluxes_dev in the six-row form; what grt_pipeline_run and
 * grt_pipeline_run_profiles refuse in ncol and the levels.  Asynchronous on the pipeline's lane. */
#define GRT_MAX_ZENITHS 64
typedef struct GrtZeniths
{
    int num_zeniths;                    /* Z, 1 .. GRT_MAX_ZENITHS */
    fp_t const *cos_zenith;             /* HOST [ncol][Z]; a value <= 0 is a night sample: its shortwave rows are +0.0 */
    fp_t const *weight;                 /* HOST [ncol][Z], or NULL: the plain mean over all Z samples, night ones included */
    fp_t *zenith_fluxes_dev;            /* DEVICE [ncol][Z][GRT_FLUXES_PER_BAND], the shortwave six rows of every angle; may be NULL */
    fp_t *zenith_level_fluxes_dev;      /* DEVICE [ncol][Z][2][V], shortwave up then down; profile form only; may be NULL */
} GrtZeniths_t;
EXTERN int grt_pipeline_run_zeniths(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtZeniths_t const *zeniths,
                                    fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev);

/* ---- every sky set under several sun angles per column, on one gas-optics pass --------------------------------------
 * grt_pipeline_run_sky's sets -- N = grt_pipeline_sky_set_count(sky->sets) of them, packed as it packs them -- with the
 * shortwave of every set solved under the Z = zeniths->num_zeniths sun angles of grt_pipeline_run_zeniths: a diurnal-mean
 * cloud radiative effect, an aerosol forcing averaged over a day, an all-sky zenith sweep.  Each band's gas optics run
 * once; the longwave of every set is solved once, as grt_pipeline_run_sky solves it; the cloud tables are staged once
 * and the S draws of a column are the same under every angle.  GrtSky_t and GrtZeniths_t are the two entry points' own;
 * columns->cos_zenith is not read; a cos_zenith <= 0 is a night sample: nothing is solved for it and its rows are +0.0
 * in every set.  Two forms:
 *   level_fluxes_dev == NULL (six rows): fluxes_dev [ncol][N][GRT_FLUXES_PER_COLUMN], the shortwave six of each set the
 *                    mean over the angles (may be NULL when zenith_fluxes_dev is given: then neither the longwave nor
 *                    the mean is formed);
 *   level_fluxes_dev != NULL (profiles): grt_pipeline_run_sky's three layouts, the shortwave rows the mean over the
 *                    angles, the heating rates and the six rows formed from the mean level fluxes.
 * The per-angle outputs of GrtZeniths_t stay optional and gain the set dimension: zenith_fluxes_dev
 * [ncol][N][Z][GRT_FLUXES_PER_BAND] in either form, zenith_level_fluxes_dev [ncol][N][Z][2][V] in the profile form.
 * The mean is taken in a fixed order, for (column, set, angle): the blocks as the other entry points add them; in a
 * cloud set the draws s = 0 .. S - 1 in order and one division by S; that is the angle's value, stored at the per-angle
 * output; then the angles k = 0 .. Z - 1 by grt_pipeline_run_zeniths' rule (with weights sum w_k F_k, each product
 * rounded before it is added; without, the sum and one division by Z, night samples included).  In the deterministic
 * mode every angle's rows of every set are, bit for bit, grt_pipeline_run_sky's for that cos_zenith, the clean set's are
 * grt_pipeline_run_zeniths', and the longwave rows are grt_pipeline_run_sky's.  A surface set with
 * grt_pipeline_set_surface applies to every set and angle; a pipeline without a shortwave band runs the longwave sets
 * and zeroes every shortwave output, the per-angle outputs included.
 * The production form (keep_spectra = 0) solves a set's angles and draws in the zenith instances of the shortwave solver
 * that hold the set's joins, grid row = (column, draw, angle), in as many launches as 65 535 grid rows and -- two-sweep
 * forms -- the park block of max_columns columns need; the clean set takes grt_pipeline_run_zeniths' path (the
 * shared-layer kernel for six rows in one sweep, GRT_TAG_ZENITH_SW), and GRT_ZENITH_SHARED=1 in the environment sends the
 * other sets' one-sweep six-row form to the shared-layer kernel's instances with their joins too (the same bits; not the
 * default until it is measured faster).  The joined sets' launches count under GRT_TAG_SKY_ZENITH_SW, the
 * mean kernel under GRT_TAG_SKY_ZENITH_MEAN; per band [max_columns][Z][S][6 or 2 V][blocks] partial sums are allocated at
 * the first call that needs more.  keep_spectra = 1: the literal loop -- per draw the set's optics, per angle the spectral
 * solver and the row-wise trapezoid (night samples as in grt_pipeline_run_zeniths), then the same mean kernel.
 * Not covered: cloud fields sampled on the device, spectral and per-bin outputs (the direct beam under several angles:
 * grt_pipeline_run_sky_zeniths_direct below).
 * GRTCODE_VALUE_ERR, with nothing launched and every output untouched, for everything grt_pipeline_run_sky refuses in
 * `sky`, everything grt_pipeline_run_zeniths refuses in `zeniths`, and fluxes_dev, level_fluxes_dev and both per-angle
 * outputs all NULL.  Asynchronous on the pipeline's lane. */
EXTERN int grt_pipeline_run_sky_zeniths(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                        GrtZeniths_t const *zeniths, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                        fp_t *fluxes_dev);

/* ---- ... with a direct-beam albedo per sun angle, and every angle's direct beam --------------------------------------
 * grt_pipeline_run_sky_zeniths in every respect -- sets and packing, both output forms, sweep rule, the per-angle outputs
 * of GrtZeniths_t, night samples, the fold over the angles, the longwave -- with two additions, either or both:
 *   surface != NULL: the direct-beam albedo of column c under angle k is that (column, angle)'s knots, put on the band's
 *     grid by grt_pipeline_set_surface's rule (the two constant ranges, the last segment's value above the grid, m w + b as
 *     multiply, then add): the double that entry point would leave in a column's row for those knots.  Open water, snow
 *     and most land reflect more of a low sun.  The diffuse albedo, the emissivity and the longwave stay those of the
 *     surface in force (grt_pipeline_set_surface, or the creation-time arrays), which this call does not touch.  A night
 *     angle's knots are checked but not read.
 *   direct != NULL: grt_pipeline_run_sky_direct's direct beam -- delta-scaled, the running product of T_pure, scaled and
 *     integrated as the other rows are -- per angle and folded over the angles in the order and arithmetic of the other
 *     rows (a cloud set's draws first, one division by S, then the angles: with weights the sum of w_k F_k, each product
 *     rounded; without, the sum and one division by Z).  A night angle's direct rows are +0.0.  The level outputs belong
 *     to the profile form; there the three rows are levels 0, V - 1 and the user level of the V.
 * In the deterministic mode every angle's rows of every set, the direct ones included, are, bit for bit,
 * grt_pipeline_run_sky_direct's under that cos_zenith with that angle's knots as the direct albedo of the surface in
 * force; with surface == NULL every output grt_pipeline_run_sky_zeniths also writes has its bits.  A pipeline without a
 * shortwave band runs the longwave and writes +0.0 to every shortwave and direct output.
 * The production form (keep_spectra = 0) evaluates the albedo per thread from the staged (column, angle) pairs -- no
 * [ncol][Z][points] rows exist -- in zenith instances of the shortwave solver and of the shared-layer kernel of their
 * own (k_shortwave.hip; routing and GRT_ZENITH_SHARED as in grt_pipeline_run_sky_zeniths), and allocates per band
 * [max_columns][Z][S][3 or V][blocks] partial sums of the direct beam at the first call that needs more.  keep_spectra =
 * 1: the literal loop -- per angle the angle's rows are written into a buffer of the call's own [max_columns][points],
 * then the spectral solver, the direct-beam kernel and the row-wise trapezoids run.
 * GRTCODE_VALUE_ERR, with nothing launched and every output and the surface in force untouched, for everything
 * grt_pipeline_run_sky_zeniths refuses; surface and direct both NULL; all four outputs of `direct` NULL; a level output
 * of `direct` in the six-row form; albedo_num_points < 2; a NULL albedo_grid or direct_albedo; a grid that is not
 * strictly increasing; a knot outside [0, 1] or not finite.  Asynchronous on the pipeline's lane. */
typedef struct GrtZenithSurface
{
    int albedo_num_points;              /* NS >= 2 */
    fp_t const *albedo_grid;            /* HOST [NS] cm-1, strictly increasing, shared by columns and angles */
    fp_t const *direct_albedo;          /* HOST [ncol][Z][NS], each in [0, 1] */
} GrtZenithSurface_t;
typedef struct GrtZenithDirect
{
    fp_t *direct_fluxes_dev;                /* DEVICE [ncol][N][GRT_DIRECT_ROWS_PER_SET]: mean over the angles; TOA, surface, user level */
    fp_t *direct_level_fluxes_dev;          /* DEVICE [ncol][N][V]: mean, every level; profile form only */
    fp_t *zenith_direct_fluxes_dev;         /* DEVICE [ncol][N][Z][GRT_DIRECT_ROWS_PER_SET] */
    fp_t *zenith_direct_level_fluxes_dev;   /* DEVICE [ncol][N][Z][V]; profile form only */
} GrtZenithDirect_t;                        /* any may be NULL, not all four */
EXTERN int grt_pipeline_run_sky_zeniths_direct(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                               GrtZeniths_t const *zeniths, GrtZenithSurface_t const *surface,
                                               GrtZenithDirect_t const *direct, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                               fp_t *fluxes_dev);
/* the host staging of `surface` (pure host code): values [ncol][zeniths][ns] on the grid x [ns] -> grt_pipeline_set_surface's
   slope and intercept entries of every (column, angle) knot row, tables [ncol][zeniths][ns + 1][2], and -- by_angle != NULL --
   the same pairs angle-major, [zeniths][ncol][ns + 1][2] (the materialised form's) */
EXTERN void grt_zenith_surface_tables(fp_t const *x, int ns, int ncol, int zeniths, fp_t const *values, fp_t *tables,
                                      fp_t *by_angle);

/* ---- ... with a sun cosine per layer for the direct beam: the pseudo-spherical approximation ---------------------------
 * grt_pipeline_run_sky_zeniths_direct in every respect -- sets and packing, both output forms, sweep rule, the per-angle
 * outputs, the fold over the angles, the optional surface and direct beam, the longwave -- but the geometry of the direct
 * beam.  A plane-parallel column attenuates the beam in every layer by exp(-tau/mu0): an air mass of 1/mu0, 1000 at
 * mu0 = 1e-3, where a spherical planet has about 38 at the horizon.  Here the direct beam sees, in each layer, the cosine
 * it has there; the diffuse field stays plane-parallel.
 *   - For column c, angle k and layer j (top layer first), the caller gives layer_cos_zenith[c][k][j] in (0, 1].
 *   - In layer j the direct-beam solution uses that value wherever it uses mu_dir today.  That covers eddington<true>, its
 *     gamma3, the optical-depth clamp, T_pure and so the running direct beam.
 *   - The diffuse solution (mu_dif), the adding sweeps and the level expressions are untouched.
 *   - The flux scale stays solar * cos_zenith[c][k].  That is the angle's own cosine, the one at the column's lowest level,
 *     as put_level and put_direct apply it today.
 *   - The surface albedo rules of grt_pipeline_set_surface and of `zenith_surface` are untouched.
 *   - cos_zenith <= 0 stays a night sample: +0.0, nothing solved, the angle's layer cosines not read.
 * slant == NULL: grt_pipeline_run_sky_zeniths_direct with the other arguments, refusals included.  With a slant,
 * zenith_surface and zenith_direct may both be NULL.  In the deterministic mode, with every layer's cosine equal to the
 * angle's cos_zenith, every output has grt_pipeline_run_sky_zeniths_direct's bits.  Outputs and their layouts are that
 * call's.  A pipeline without a shortwave band runs the longwave and writes +0.0 to every shortwave and direct output.
 * The cosines are copied once per call into a device block [max_columns][Z][L] of the pipeline's own and joined to zenith
 * instances of the shortwave solver and of the shared-layer kernel of their own (k_shortwave.hip: GrtZenithSlantArgs;
 * routing and GRT_ZENITH_SHARED as in grt_pipeline_run_sky_zeniths); every slant instance carries the direct beam, so
 * its partial sums are allocated whether or not zenith_direct asks for them.
 * Not covered: a sun below the horizon that still lights upper layers (cos_zenith <= 0 is night at every level); a
 * pipeline in the materialised form (keep_spectra = 1); refraction; what grt_pipeline_run_sky_zeniths does not cover.
 * GRTCODE_VALUE_ERR, with nothing launched and every output untouched, for everything
 * grt_pipeline_run_sky_zeniths_direct refuses (but surface and direct both NULL, which is allowed here); a NULL
 * layer_cos_zenith; a day sample (cos_zenith > 0) with a layer cosine that is not finite, is <= 0 or is > 1; a pipeline
 * in the materialised form.  Asynchronous on the pipeline's lane. */
typedef struct GrtZenithSlant
{
    fp_t const *layer_cos_zenith;       /* HOST [ncol][Z][L], top layer first */
} GrtZenithSlant_t;
EXTERN int grt_pipeline_run_sky_zeniths_slant(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                              GrtZeniths_t const *zeniths, GrtZenithSlant_t const *slant,
                                              GrtZenithSurface_t const *zenith_surface,
                                              GrtZenithDirect_t const *zenith_direct, fp_t *level_fluxes_dev,
                                              fp_t *heating_dev, fp_t *fluxes_dev);
/* The layer cosines of the straight ray that reaches the column's lowest level under cos_zenith, on a sphere of radius
   radius_m (pure host code).  height_m [ncol][V], top first, strictly descending; cos_zenith [ncol][Z];
   layer_cos_zenith [ncol][Z][L], L = V - 1.  With r0 = radius + height[V-1], rt = radius + height[j],
   rb = radius + height[j+1], s2 = r0 r0 (1 - mu0 mu0), a = sqrt(rt rt - s2), b = sqrt(rb rb - s2), layer j's cosine is
   (a + b)/(rt + rb): the layer's thickness over the ray's path length in it, written so that nothing cancels -- finite at
   mu0 = 0 and exactly 1 at mu0 = 1.  radius_m == 0 is a flat planet: every layer gets mu0 itself, bit for bit.  The
   entries of an angle below the horizon (cos_zenith < 0) are set to 0; cos_zenith = 0 gets the horizon ray's cosines;
   the pipeline, where cos_zenith <= 0 is a night sample, reads neither.  The ray to the surface is the exact
   geometry for the beam at the surface and an approximation for the levels above it, whose own rays cross the upper
   layers a little more steeply.  GRTCODE_VALUE_ERR, with nothing written, for a negative or non-finite radius,
   num_levels < 2, ncol or num_zeniths < 1, heights that are not finite or not strictly descending, |cos_zenith| > 1 or
   NaN; GRTCODE_NULL_ERR for a NULL pointer. */
EXTERN int grt_slant_cosines(double radius_m, int ncol, int num_levels, int num_zeniths, double const *height_m,
                             double const *cos_zenith, double *layer_cos_zenith);

/* ---- several surface tiles per column on one gas-optics pass -----------------------------------------------------------
 * grt_pipeline_run_sky (its six-row form) with T surfaces per column: land, open water, sea ice, snow -- each tile with its
 * own emissivity, albedo and skin temperature under the column's one atmosphere.  Each band's gas optics run once; the
 * solvers walk the layers once for a chunk of tiles and do only the surface's part per tile (k_longwave.hip:
 * lw_tile_kernel, k_shortwave.hip: sw_tile_kernel).  N = grt_pipeline_sky_set_count(sky->sets) sets, packed as
 * grt_pipeline_run_sky packs them; the S draws of a column's cloud sets are the same over every tile.
 * A tile's rows on the band grids are grt_pipeline_set_surface's for its knots, to the bit (the same host pairs, the same
 * kernel).  A band with a point count of 0 takes, for every tile, the surface in force: grt_pipeline_set_surface's rows,
 * else the creation-time arrays -- tiles that differ only in temperature are a valid call.  The surface in force is not
 * changed by this call and applies again afterwards.  columns->surface_temperature is not read and may be NULL.
 * tile_fluxes_dev [ncol][N][T][GRT_FLUXES_PER_COLUMN]: every tile's twelve rows in grt_pipeline_run's layout;
 * fluxes_dev [ncol][N][GRT_FLUXES_PER_COLUMN]: the mean over the tiles; at least one of the two is given.  The mean is
 * taken in a fixed order, for (column, set, tile): the blocks as the other entry points add them; in a cloud set the draws
 * s = 0 .. S - 1 in order and one division by S; that is the tile's value, stored at tile_fluxes_dev; then the tiles
 * t = 0 .. T - 1 -- with fractions sum f_t F_t, each product rounded before it is added (the fractions need not sum to
 * one); without, the sum and one division by T.  In the deterministic mode tile t's rows of every set are, bit for bit,
 * grt_pipeline_run_sky's after grt_pipeline_set_surface with tile t's knots and columns->surface_temperature set to tile
 * t's; with T = 1 and no fractions the whole fluxes_dev is.  A pipeline without a shortwave band zeroes the shortwave
 * rows of both outputs; without a longwave band, the longwave rows.
 * The production form (keep_spectra = 0) launches under GRT_TAG_TILE_LW and GRT_TAG_TILE_SW and reduces with a
 * deterministic kernel (GRT_TAG_TILE_MEAN); the tiles' rows are written by grt_pipeline_set_surface's kernel
 * (GRT_TAG_SURFACE) into [max_columns T][n] doubles of pipeline scratch per band and array, and per band
 * [max_columns][T][S][6][blocks] partial sums are allocated at the first call that needs more.  keep_spectra = 1: the
 * literal loop -- per draw the set's optics, per tile the spectral solver on the tile's rows and temperature and the
 * row-wise trapezoid, then the same mean kernel.
 * Not covered: the profile, spectral and per-bin forms; the direct beam, the surface-temperature Jacobian and radiances
 * per tile; several sun angles with tiles; cloud fields sampled on the device; multi-GPU gathers of tile_fluxes_dev; the
 * example drivers.
 * GRTCODE_VALUE_ERR, with nothing launched and every output untouched, for: everything grt_pipeline_run_sky refuses in
 * `sky`; everything grt_pipeline_set_surface refuses in grids, counts and values (NaN included); num_tiles outside
 * 1 .. GRT_MAX_TILES; a NULL tiles; a NULL surface_temperature with a longwave band; a tile temperature outside
 * MIN_TEMPERATURE .. MAX_TEMPERATURE, or NaN; a fraction that is negative or NaN; both outputs NULL; ncol outside
 * 1 .. max_columns.  Asynchronous on the pipeline's lane. */
#define GRT_MAX_TILES 16
typedef struct GrtSurfaceTiles
{
    int num_tiles;                         /* T, 1 .. GRT_MAX_TILES */
    fp_t const *fraction;                  /* HOST [ncol][T] or NULL */
    fp_t const *surface_temperature;       /* HOST [ncol][T] K; required with a longwave band */
    int num_emissivity_points, num_albedo_points;          /* NS_e, NS_a: 0 or >= 2, as in GrtSurface_t */
    fp_t const *emissivity_grid, *albedo_grid;             /* HOST [NS], strictly increasing, shared */
    fp_t const *emissivity;                /* HOST [ncol][T][NS_e] */
    fp_t const *direct_albedo;             /* HOST [ncol][T][NS_a] */
    fp_t const *diffuse_albedo;            /* HOST [ncol][T][NS_a] or NULL: the direct one */
    fp_t *tile_fluxes_dev;                 /* DEVICE [ncol][N][T][12] or NULL */
} GrtSurfaceTiles_t;
EXTERN int grt_pipeline_run_sky_tiles(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                      GrtSurfaceTiles_t const *tiles, fp_t *fluxes_dev /* [ncol][N][12] or NULL */);

/* ---- response-weighted level fluxes and actinic flux, of every sky set ----------------------------------------------
 * grt_pipeline_run_sky in its PROFILE FORM in every respect -- the sets and their packing, the surface in force, the input
 * checks, asynchronous on the pipeline's lane, the two-sweep shortwave, every output it writes (level_fluxes_dev is
 * required; heating_dev and fluxes_dev may be NULL) -- and beside them the same level rows under spectral weights that
 * are not a box: a photolysis cross-section times quantum yield, the erythemal action spectrum, photon-weighted PAR, the
 * response of a pyranometer, a pyrgeometer dome or a window channel -- reduced on the device, so that no [V][n] row has
 * to leave it.  Response k of a band is the grid points i = first[k] + j, j = 0 .. count_k - 1 (count_k = offset[k + 1] -
 * offset[k]) with r_k(i) = weights[offset[k] + j], and 0 elsewhere.  Responses may overlap, repeat, come in any order, be
 * one point wide and carry any finite sign; they are NOT normalised.  With t_i the whole band's trapezoid weight (dw, dw/2
 * at the points 0 and n - 1),
 *   X_k(level) = sum_i (t_i r_k(i)) F_i(level),      W m-2 x the unit of r,
 * each term formed as F (t r); F is the level's upward flux, its downward flux and, in the shortwave, its direct beam
 * (grt_pipeline_run_sky_direct's: the delta-scaled beam, per unit horizontal area).
 *   weighted_levels_dev [ncol][N][2 R_lw + 3 R_sw][V] (required): per set the longwave's [R_lw][2][V] (up, down), then the
 *                       shortwave's [R_sw][3][V] (up, down, direct); levels top first.  A band with no responses takes no
 *                       room; at least one band must have some.
 *   actinic_levels_dev  [ncol][N][R_sw][V] (may be NULL): the actinic flux of the shortwave responses,
 *                         A_k(level) = (S_k/mu0 + (D_k - S_k)/mu_dif) + U_k/mu_dif,
 *                       formed in that order from the three finished rows (S direct, D down, U up); mu0 the column's
 *                       cos_zenith, mu_dif the solver's 0.5 (driver.c:110).  The direct beam counts once per unit area
 *                       normal to it, each diffuse hemisphere is taken as isotropic, as every delta-two-stream actinic
 *                       flux is; the beam is the DELTA-SCALED one, so forward-scattered light counts as beam.
 * A cloud set's row is the mean over its num_subcolumns draws, 0 .. S - 1 in order, then one division by S; its actinic
 * flux is formed from the means.  A band the pipeline lacks can carry no responses and has no rows here (its rows of
 * level_fluxes_dev are zeros, as grt_pipeline_run_sky writes them).
 * Identities (deterministic mode, bit for bit): every output grt_pipeline_run_sky also writes is grt_pipeline_run_sky's;
 * the response r = 1 on the whole grid gives level_fluxes_dev's rows of the band and grt_pipeline_run_sky_direct's
 * direct_level_fluxes_dev; a response's rows do not depend on the other responses, columns or sets of the call; 2 r gives
 * twice the rows, -r their negatives; D_k = S_k at the top level.
 * How it runs (keep_spectra = 0): the profile solvers in their response form (the passes' own tags) -- the broadband rows
 * summed as ever, and per response that has a point in a workgroup's 128 grid points one more group of wave sums, the
 * products t r staged in LDS; a workgroup outside every response does the profile form's work --, their sums stored
 * without atomics per (response, solver block) pair; then a finishing kernel of one thread per output row and the actinic
 * kernel (both under GRT_TAG_BAND_PROFILES).  keep_spectra = 1: the spectral solvers and the direct-beam kernel
 * (GRT_TAG_DIRECT_BEAM), a kernel that applies the same weights and sums to the [V][n] rows, the same finishing kernels.
 * Scratch per band: max_columns x S x P x G V doubles at the first call that needs more, G = 2 (longwave) or 3
 * (shortwave), S the draws of the call's cloud sets (1 without one), P = grt_response_pair_count(responses, band, n) --
 * about n/128 for a response over the whole grid: broad responses are the expensive ones.  The device tables are kept and
 * reused while first, offset and weights hold the same values.
 * grt_response_pair_count: host code only.  P, the number of (response, 128-point solver block) pairs in which a response
 * of `band` (0 longwave, 1 shortwave) has a point on a grid of num_points points; 0 for a band without responses; -1 for
 * anything the entry point would refuse in that band's four fields, for another band and for num_points < 1.
 * grt_pipeline_response_block_limit: the most responses that may have a point in one block of 128 consecutive grid points
 * (block b: points 128 b .. 128 b + 127) at this pipeline's V: the workgroup's wave sums and staged weights must fit its
 * 64 KiB of LDS, 16 G V (1 + R_b) + 1024 R_b <= 65536 -- 15 in the shortwave and 21 in the longwave at V = 61.  -1 for
 * another band.
 * GRTCODE_VALUE_ERR, with nothing launched and every output untouched, for: responses NULL; weighted_levels_dev NULL;
 * both counts 0; a count outside 0 .. GRT_MAX_RESPONSES; a count > 0 with first, offset or weights NULL; responses for a
 * band the pipeline lacks; offset[0] != 0 or offset not strictly increasing; first[k] < 0 or first[k] + count_k > n; a
 * weight that is NaN or infinite; more responses in one block than the limit; actinic_levels_dev with sw_num_responses
 * == 0; level_fluxes_dev NULL; everything grt_pipeline_run_sky refuses.  A night column: GRTCODE_RANGE_ERR, as everywhere.
 * Not covered: the several-sun-angle and surface-tile entry points, cloud fields sampled on the device, weighted heating
 * rates, the Jacobian rows, the example drivers. */
#define GRT_MAX_RESPONSES 256                 /* per band */
typedef struct GrtResponses
{
    int lw_num_responses;          /* R_lw, 0 .. GRT_MAX_RESPONSES */
    int const *lw_first;           /* HOST [R_lw]: grid index of the response's first point in the longwave band */
    int const *lw_offset;          /* HOST [R_lw + 1]: offset[0] = 0, strictly increasing */
    fp_t const *lw_weights;        /* HOST [lw_offset[R_lw]]: r_k sampled on the grid, response after response */
    int sw_num_responses;          /* R_sw: the same of the shortwave band */
    int const *sw_first;
    int const *sw_offset;
    fp_t const *sw_weights;
    fp_t *weighted_levels_dev;     /* DEVICE [ncol][N][2 R_lw + 3 R_sw][V]; required */
    fp_t *actinic_levels_dev;      /* DEVICE [ncol][N][R_sw][V]; may be NULL */
} GrtResponses_t;
EXTERN int grt_pipeline_run_sky_weighted(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                         GrtResponses_t const *responses, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                         fp_t *fluxes_dev);
EXTERN long long grt_response_pair_count(GrtResponses_t const *responses, int band /* 0 lw, 1 sw */, long long num_points);
EXTERN int grt_pipeline_response_block_limit(GrtPipeline_t const *pipeline, int band);

/* ---- longwave scattering by clouds and aerosols ------------------------------------------
 * The longwave solver (calculate_lw_fluxes, and the longwave of every grt_pipeline_run_...) treats every particle as a
 * pure absorber: a layer's optical depth is tau (1 - omega), and g is never read (longwave.c:252).  That stays so.
 * grt_pipeline_run_sky_scattering is grt_pipeline_run_sky, and with it the scattering correction of every set's longwave:
 * the difference of two two-stream adding solves of the same code at every grid point,
 *   delta_up_i = F_up_i[tau, omega, g] - F_up_i[tau (1 - omega), 0, 0]     (the same for down; every level i),
 * integrated over the band as the fluxes are, and   corrected = four-stream + delta.   Per layer, with D = 1.66:
 *   gamma1 = D (1 - omega (1 + g)/2),  gamma2 = D omega (1 - g)/2,  k = sqrt(max((gamma1 - gamma2)(gamma1 + gamma2), 1e-12)),
 *   x = min(k tau, 700),  e = exp(-x),  E = -expm1(-2 x),  m = -expm1(-x),  den = k (1 + e e) + gamma1 E,
 *   R = gamma2 E/den,  T = 2 k e/den,  eps = (k m m + (gamma1 - gamma2) E)/den      (= 1 - R - T),
 *   S_up = eps pi effective_planck(B(t_layer_j), B(t_level_j), tau (1 - omega)),  S_down = ... B(t_level_j+1) ...
 * with the solver's own planck_law and effective_planck (longwave.c:68-118).  Adding, level V - 1 the surface:
 *   A_L = 1 - emis,  U_L = emis pi B(t_surf)
 *   up:    beta_j = 1/(1 - A_{j+1} R_j);  A_j = R_j + T_j T_j A_{j+1} beta_j;  U_j = S_up_j + T_j (U_{j+1} + A_{j+1} S_down_j) beta_j
 *   down:  F_down_0 = 0, F_up_0 = U_0;  F_down_{j+1} = (T_j F_down_j + R_j U_{j+1} + S_down_j) beta_j;
 *          F_up_{j+1} = A_{j+1} F_down_{j+1} + U_{j+1}
 * Where no layer of a point scatters both solves see the same numbers and the difference is exactly +0.0.
 *
 * Outputs.  level_fluxes_dev, heating_dev, fluxes_dev: grt_pipeline_run_sky's, in its layouts and forms
 * (level_fluxes_dev == NULL: the six-row form); every longwave value is grt_pipeline_run_sky's plus its difference, one
 * fp64 addition; the heating rates are formed from the corrected levels; the shortwave values are grt_pipeline_run_sky's
 * bit for bit.  scatter_dev [ncol][N][6] (N sets, as packed there): the differences of up TOA, up surface, up user level,
 * down TOA, down surface, down user level (+0.0 without a user level), W m-2.  scatter_levels_dev [ncol][N][2][V], profile
 * form only: up then down at every level, top first; its rows 0, V - 1 and the user level are scatter_dev's.  Either may
 * be NULL, not both.  Every set gets its differences, the clean one too (Rayleigh scattering: tiny, not zero); a cloud
 * set's are the mean over its draws, in grt_pipeline_run_subcolumns' order and arithmetic.  grt_pipeline_set_surface
 * applies.  With keep_spectra = 1 the correction runs on the tau, omega, g each pass leaves on the grid.
 * Memory: the first call allocates the longwave band's park block, max_columns x (V - 1) x 10 rows of the band's points
 * rounded up to 128; a cloud set of more draws than fit is solved in several launches.  Other calls allocate nothing more.
 * Counted under GRT_TAG_SCATTER_LW and GRT_TAG_SCATTER_FINISH.
 * GRTCODE_VALUE_ERR, with nothing launched and the outputs untouched, for: everything grt_pipeline_run_sky refuses; both
 * scatter outputs NULL; scatter_levels_dev in the six-row form; a pipeline without a longwave band.
 * Not covered: the radiance, channel, weighting, Jacobian, tile, zenith, weighted, band-profile and ck entry points, and
 * calculate_lw_fluxes, which keep the reference's semantics; more than two streams.
 *
 * grt_lw_scatter_levels: the same kernel on optics of the caller's, everything a DEVICE array: tau, omega, g
 * [ncol][V - 1][n] (omega, g may be NULL: 0), the temperatures [ncol][V - 1], [ncol][V], [ncol], the emissivity
 * [ncol][n], on the grid w0 + i dw.  delta_up_dev, delta_down_dev [ncol][V][n]: the spectral differences, W m-2 per
 * cm-1; flux_up_dev, flux_down_dev (both or neither): the scattering solve's own fluxes.  It allocates and frees its
 * park block and waits for the result.  GRTCODE_VALUE_ERR for a NULL struct, a required pointer that is NULL, ncol < 1 or
 * > 65535, num_levels < 2, n < 1, a dw that is not positive and finite, one of flux_up_dev and flux_down_dev alone. */
typedef struct GrtLwScatter
{
    int ncol;
    int num_levels;
    long long n;
    fp_t w0, dw;
    fp_t const *tau_dev, *omega_dev, *g_dev;
    fp_t const *layer_temperature_dev, *level_temperature_dev, *surface_temperature_dev;
    fp_t const *emissivity_dev;
    fp_t *delta_up_dev, *delta_down_dev;
    fp_t *flux_up_dev, *flux_down_dev;
} GrtLwScatter_t;
EXTERN int grt_lw_scatter_levels(Device_t device, GrtLwScatter_t const *scatter);
EXTERN int grt_pipeline_run_sky_scattering(GrtPipeline_t *pipeline, GrtColumns_t const *columns, GrtSky_t const *sky,
                                           fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev,
                                           fp_t *scatter_levels_dev, fp_t *scatter_dev);

/* ---- columns across the GPUs of one node ------------------------------------
 * One process per GPU; contiguous ceil-sized column blocks; one gather of the [columns][GRT_FLUXES_PER_COLUMN]
 * flux blocks to rank 0.  The reference fans out processes with -x/-X column ranges and merges per-shard files
 * afterwards (GRTworkflow/run-rfmip-irf.sh:103-148); this is that scheme inside one node.
 * transport GRT_MULTI_RCCL: ncclGather over xGMI on the library stream (device pointers, asynchronous; the
 * communicator id travels through `rendezvous_dir`, a directory all ranks see); GRT_MULTI_FILES: per-rank files in
 * `rendezvous_dir` assembled by rank 0 (host or device pointers, synchronous) -- the reference's own scheme, and the
 * way the multi-rank path runs where there is no GPU.  GRT_MULTI_TIMEOUT [s] bounds every wait (default 600).
 * File transport: exchange files are named <kind>_<job tag>_<call number>_rank<r>.bin, the tag being GRT_MULTI_JOB in the
 * environment (the same for all ranks of a job; letters, digits, '-'; default "0").  A gather needs no two ranks alive at
 * the same time (a rank writes its block and leaves; rank 0 may start last); grt_multi_max is a barrier and does.  Rank 0
 * removes everything its job wrote when it is destroyed, so a directory is reusable after a clean run; files under other
 * tags are never touched or read, so with a tag of its own a job is also safe from the leftovers of one that crashed
 * (without tags: empty the directory after a crash).  RCCL transport: rank 0 removes the communicator id on destroy. */
enum grt_multi_transport { GRT_MULTI_RCCL = 0, GRT_MULTI_FILES = 1 };
typedef struct GrtMulti GrtMulti_t;
/* rank's block of a num_columns-column set: [first, first + count), count <= ceil(num_columns/world), 0 for ranks beyond the end */
EXTERN int grt_multi_shard(int num_columns, int rank, int world, int *first, int *count);
EXTERN int grt_multi_create(GrtMulti_t **multi, int transport, Device_t device, int rank, int world,
                            char const *rendezvous_dir);
EXTERN int grt_multi_destroy(GrtMulti_t **multi);
/* local: this rank's [count][row_doubles] block; all (rank 0 only): room for world*ceil(num_columns/world) rows, the first
   num_columns of which are the columns in order (short blocks are padded, so no sizes are exchanged).  Any row width:
   e.g. 4 V + 2 (V - 1) for the level fluxes and heating rates of grt_pipeline_run_profiles, 8 V + 4 (V - 1) for those of
   grt_pipeline_run_allsky_profiles, sets (2 NB V + NB (V - 1)) for the level fluxes and heating rates of
   grt_pipeline_run_band_profiles with NB = lw_num_bins + sw_num_bins (two gathers: its two outputs are two buffers). */
EXTERN int grt_multi_gather_rows(GrtMulti_t *multi, fp_t const *local, int num_columns, int row_doubles, fp_t *all,
                                 int on_device);
/* grt_multi_gather_rows with rows of GRT_FLUXES_PER_COLUMN: the [count][12] blocks of grt_pipeline_run. */
EXTERN int grt_multi_gather_fluxes(GrtMulti_t *multi, fp_t const *local, int num_columns, fp_t *all, int on_device);
EXTERN int grt_multi_broadcast(GrtMulti_t *multi, void *buffer_dev, size_t bytes);   /* RCCL only: replicate from rank 0 */
EXTERN int grt_multi_max(GrtMulti_t *multi, double *value);    /* barrier + maximum over the ranks (timing brackets) */

/* ---- HIP-event timing of individual kernels on the library stream -------------------
 * Each tag names what one pair of events brackets; grt_profile_read(tag, ...) gives the time and the launches counted
 * under it.  Read after grt_pipeline_sync(). */
enum
{
    /* 1 = line-by-line kernel on a grid of <= 10 000 points (longwave band at 1 cm-1), and of a pipeline's longwave band */
    GRT_TAG_GAS_LW = 1,
    /* 2 = line-by-line kernel on a larger grid (shortwave band), and of a pipeline's shortwave band */
    GRT_TAG_GAS_SW = 2,
    /* 3 / 4 = LW / SW solver of the clear-sky (clear-clean) pass of every grt_pipeline_run_... */
    GRT_TAG_SOLVER_LW = 3,
    GRT_TAG_SOLVER_SW = 4,
    /* 5 = clear-sky optics combine (materialised form) */
    GRT_TAG_CLEAR_OPTICS = 5,
    /* 6 / 7 = far-field gather kernel of the two-pass line kernel (longwave / shortwave band; GRT_TAG_GAS_LW / _SW then
       cover its first pass) */
    GRT_TAG_FAR_LW = 6,
    GRT_TAG_FAR_SW = 7,
    /* 8 / 9 = LW / SW solver of the all-sky pass of grt_pipeline_run_allsky, _allsky_profiles, _subcolumns (each band's
       launches together), _cloud_fields, _spectral and _band_profiles */
    GRT_TAG_ALLSKY_LW = 8,
    GRT_TAG_ALLSKY_SW = 9,
    /* 10 = the wavenumber-bin kernel of grt_pipeline_run_spectral (both of its launches; its solvers count under
       GRT_TAG_SOLVER_... and GRT_TAG_ALLSKY_...) */
    GRT_TAG_BINS = 10,
    /* 11 = the subcolumn-mean kernel of grt_pipeline_run_subcolumns (with S > 1) */
    GRT_TAG_SUBCOLUMN_MEAN = 11,
    /* 12 / 13 = LW / SW solver of the aerosol pass of grt_pipeline_run_aerosols */
    GRT_TAG_AEROSOL_LW = 12,
    GRT_TAG_AEROSOL_SW = 13,
    /* 14 = the per-bin reduction and the heating-rate kernel of grt_pipeline_run_band_profiles (its solvers count under
       GRT_TAG_SOLVER_... and GRT_TAG_ALLSKY_...); and of grt_pipeline_run_sky_weighted the finishing kernel of the response
       rows (one launch per band and set; keep_spectra = 1: with the kernel that weights the [V][n] rows before it) and the
       actinic kernel (its solvers count under grt_pipeline_run_sky's tags) */
    GRT_TAG_BAND_PROFILES = 14,
    /* 15 = the surface-row kernel of grt_pipeline_set_surface (all its launches) */
    GRT_TAG_SURFACE = 15,
    /* 16 = the cloud-sampling kernel of grt_cloud_sampler_run and grt_pipeline_run_cloud_fields */
    GRT_TAG_CLOUD_SAMPLER = 16,
    /* 17 / 18 = LW / SW solver of the pass of grt_pipeline_run_sky that joins aerosol and clouds (GRT_SKY_CLOUD_AEROSOL; its
       other sets count under GRT_TAG_SOLVER_..., GRT_TAG_AEROSOL_... and GRT_TAG_ALLSKY_...) */
    GRT_TAG_SKY_LW = 17,
    GRT_TAG_SKY_SW = 18,
    /* 19 = the shortwave solver launches of grt_pipeline_run_zeniths, every angle's together (its longwave counts under
       GRT_TAG_SOLVER_LW); 20 = its mean kernel */
    GRT_TAG_ZENITH_SW = 19,
    GRT_TAG_ZENITH_MEAN = 20,
    /* 21 = the direct-beam kernel of grt_pipeline_run_sky_direct's materialised form (every set's, every subcolumn's) */
    GRT_TAG_DIRECT_BEAM = 21,
    /* 22 = the shortwave solver launches of grt_pipeline_run_sky_zeniths' sets with aerosol, clouds or both, every angle's
       and draw's together (its clean set counts under GRT_TAG_ZENITH_SW, its longwave under grt_pipeline_run_sky's tags);
       23 = its mean kernel, every set's */
    GRT_TAG_SKY_ZENITH_SW = 22,
    GRT_TAG_SKY_ZENITH_MEAN = 23,
    /* 24 = the Jacobian kernel of grt_pipeline_run_sky_jacobian's materialised form (every set's, every subcolumn's; the
       fused instances count under grt_pipeline_run_sky's tags) */
    GRT_TAG_SURFACE_JACOBIAN = 24,
    /* 25 = the radiance kernel of grt_pipeline_run_sky_radiances (every set's, every draw's, in both forms) */
    GRT_TAG_RADIANCE = 25,
    /* 26 = the finishing kernel of grt_pipeline_run_sky_channels (one launch per set; the channel form of the radiance
       kernel counts under 25) */
    GRT_TAG_CHANNELS = 26,
    /* 27 = the transmittance and contribution kernel of grt_pipeline_run_sky_weighting (every set's, every draw's, in both
       forms); 28 = its finishing kernel (one launch per set) */
    GRT_TAG_WEIGHTING = 27,
    GRT_TAG_WEIGHTING_FINISH = 28,
    /* 29 = the k-distribution kernel of grt_kdist_rows and grt_pipeline_run_kdist (the latter's gas optics counts under
       1 / 2 and 6 / 7) */
    GRT_TAG_KDIST = 29,
    /* 30 = the class-map kernel of grt_kdist_class_map and grt_pipeline_run_kdist_correlated; 31 = the mapped reduction of
       grt_kdist_mapped_rows and grt_pipeline_run_kdist_correlated (the latter's gas optics counts under 1 / 2 and 6 / 7) */
    GRT_TAG_KDIST_MAP = 30,
    GRT_TAG_KDIST_MAPPED = 31,
    /* 32 = the source sums of grt_pipeline_run_ck_fluxes (one launch per band that has bins); 33 / 34 = its LW / SW solve on
       the g-classes with the bin sums behind it (its gas optics counts under 1 / 2 and 6 / 7, its map and its mapped
       reduction under 30 and 31) */
    GRT_TAG_CK_SOURCES = 32,
    GRT_TAG_CK_LW = 33,
    GRT_TAG_CK_SW = 34,
    /* 35 / 36 = the LW / SW tile kernels of grt_pipeline_run_sky_tiles, every set's launches (keep_spectra = 1: its spectral
       solver launches; its gas optics counts under 1 / 2 and 6 / 7, the tiles' rows under 15); 37 = its mean kernel, one
       launch per band and set */
    GRT_TAG_TILE_LW = 35,
    GRT_TAG_TILE_SW = 36,
    GRT_TAG_TILE_MEAN = 37
};
/* ... continued behind the last of them: 38 = the scattering-correction kernel of grt_pipeline_run_sky_scattering, every
   set's launches (its solvers count under grt_pipeline_run_sky's tags), and of grt_lw_scatter_levels; 39 = what turns its
   partial sums or spectral rows into a set's differences and adds them to the set's longwave rows (the reductions, the
   subcolumn mean, the addition, the row pick) */
enum
{
    GRT_TAG_SCATTER_LW = GRT_TAG_TILE_MEAN + 1,
    GRT_TAG_SCATTER_FINISH
};
EXTERN int grt_profile_enable(int on);
EXTERN int grt_profile_read(int tag, double *total_ms, int *launches, int reset);

/* ---- parked Optics_t blocks -------------------------------------------------------------
 * destroy_optics parks a device block (at most six, none above 512 MB, oldest evicted first) so that the next
 * create_optics / add_optics of the same size -- a driver's column loop does both per band and column
 * (driver.c:382-383, 424) -- skips hipFree + hipMalloc.  grt_optics_cache_flush() gives the parked blocks back to the
 * device, e.g. before a large allocation.  One caller thread, as everywhere in this interface. */
EXTERN int grt_optics_cache_flush(void);

/* ---- several batches in flight ----------------------------------------------------------
 * Every call enqueues on one HIP stream per device, in call order.  grt_device_use_lane(device, k), k = 0..3, makes the
 * calls that follow use stream k of that device: a caller with two pipelines (each with gas-optics objects of its own)
 * alternates lanes batch by batch, and the end of one batch -- far-field gather, solvers -- can overlap the next batch's
 * line kernel (bench.py --lanes: +0.7 % with two lanes, +1.4 % with three on G1: those kernels keep the vector pipe busy
 * themselves, so there is little to hide; the mechanism is for callers whose batches leave the GPU idler).  Objects used
 * together must be used on the same lane; grt_device_synchronize(device) waits for all lanes. */
EXTERN int grt_device_use_lane(Device_t device, int lane);
EXTERN int grt_device_synchronize(Device_t device);

/* ---- plain device-memory helpers for FFI callers (tests, bench) -------------------- */
EXTERN int grt_device_malloc(Device_t device, void **ptr, size_t bytes);
EXTERN int grt_device_free(Device_t device, void *ptr);
EXTERN int grt_device_to_host(Device_t device, void *dst_host, void const *src_dev, size_t bytes);
EXTERN int grt_host_to_device(Device_t device, void *dst_dev, void const *src_host, size_t bytes);

/* ---- parity hook: per-(layer,line) preparation of kernels.c:34-131 and the integer
 * windows of kernels.c:431-437 for one column, in merged-store order.  Host outputs:
 * slot/iso [N]; v0 [N]; vnn, snn, gamma, alpha, win_s, win_e [L][N] (win_s > win_e when
 * the line is skipped).  *num_lines receives N; pass NULL arrays to query N only. */
EXTERN int grt_debug_line_prep(GasOptics_t *gas_optics, fp_t *pressure, fp_t *temperature,
                               uint64_t *num_lines, uint8_t *slot, double *v0, double *vnn,
                               double *snn, double *gamma, double *alpha, int64_t *win_s,
                               int64_t *win_e);

/* ---- cost-analysis hook: per-workgroup clocks and event counts of the two-pass line kernel (single-level grids, and
 * the cell hierarchy's twelve-moment form of sparse lines).
 * buffer_dev: DEVICE memory of `words` 64-bit words, zeroed by the caller before each launch; 24 words per workgroup at
 * record ((column L + layer) tiles + tile) nslice + slice: clock at entry, clock at exit, candidate lines,
 * R | corrected << 16 | moments << 17, then sums over the workgroup's waves of 64-line blocks worked on, ring steps,
 * near-centre points queued, moment reductions, lane-by-lane moment adds, region-1 correction steps, near-centre walk
 * steps; words 11-13: clock when the prologue is done, when every wave has left the line loop, when the last wave left
 * it; words 14-21: clocks the waves spent in preparation, moment reduction and adds, near-centre walk and queue
 * pushes, region-1 corrections, near field (ring), the rest of the line loop, evaluating queued points, moment terms
 * (each mark waits for the wave's outstanding LDS operations: phases that end in LDS adds look longer than they are);
 * words 22-23: ring steps taken without the range test / with the Lorentzian alone (cell hierarchy form).  An instrumented instance of the kernel runs while a buffer is set (tile/nslice: grt_gas_optics_last_launch);
 * NULL switches back to the production instance.  scripts/line_cost_by_wavenumber.py. */
EXTERN int grt_gas_optics_probe(GasOptics_t *gas_optics, void *buffer_dev, uint64_t words);

/* ---- parity hook: the strengths of the device line store (merged store order) as the kernels read them, i.e. after
 * the rescaling of parse_HITRAN_file.c:372-384 with the partition sums current at the last build.  Pass s0_out = NULL
 * to query the count. */
EXTERN int grt_debug_line_strengths(GasOptics_t *gas_optics, uint64_t *num_lines, double *s0_out);

/* ---- parity hook: the line shape itself.  Same inputs as rfm_voigt_line_shape(LineShapeInputs_t, K)
 * (gas-optics/src/RFM_voigt.c:85-281, line_shape.h:26-35): K[i], i < num_wpoints, at w + i*wres for a line at
 * line_center with Lorentz / Doppler half-widths gamma / alpha, evaluated on the DEVICE by the functions the
 * line kernels are built from.  fast = 0: reference operation order; 1: the fused forms' arithmetic. */
EXTERN int grt_debug_voigt(Device_t device, int fast, fp_t w, uint64_t num_wpoints, fp_t wres, fp_t line_center,
                           fp_t gamma, fp_t alpha, fp_t *K);

/* ---- parity hook: the near-centre line shape point by point.  x[i], y[i], i < n: doubles that hold fp32 values (X and Y
 * of RFM_voigt.c:165/95); K[i]: what the device's voigt_near returns there, BEFORE the scaling of RFM_voigt.c:278;
 * cls[i]: the class of formula voigt_class sorted the point into, -1 where no class is involved.  variant 0: reference
 * operation order; 1: fused arithmetic; 2: sorted into classes 0 / 1 / 2 and evaluated by that class's code alone;
 * 3: classes 0 / 1 / 2 / 3 (region 3 apart); 4: as 3, region 4 in packed registers -- the production instance's own
 * dispatch.  Variants 0 and 1 also take |x| >= XLIM0 (K as :170 leaves it, likewise before :278) and
 * y >= 70.55 (K of :103, which has no :278), with REPWID = 1. */
EXTERN int grt_debug_voigt_points(Device_t device, int variant, uint64_t n, fp_t const *x, fp_t const *y, fp_t *K, int *cls);

/* ---- parity hook: the device's own exponentials and REPWID at n arguments.  op 0: grt_exp_pair (out0 = e^a, out1 = e^-a);
 * 1: grt_exp; 2: exp_fast; 3: exp_fp64; 4: reference_repwid(a), widened to double.  out1 is written for op 0 only. */
EXTERN int grt_debug_device_math(Device_t device, int op, uint64_t n, fp_t const *a, fp_t *out0, fp_t *out1);

/* ---- parity hook: the 1/Q(T, iso) block of one column's state as the DEVICE holds it (the path of
 * calc_partition_functions, kernels.c:52-66: evaluated on the host per layer and isotopologue, shipped inside the
 * column state, read by the line kernels as q[slot][layer][iso-1]).  q_out: host [num_molecules][L][GRT_MAX_ISO = 18],
 * zero beyond a molecule's isotopologue count. */
EXTERN int grt_debug_partition_functions(GasOptics_t *gas_optics, fp_t *pressure, fp_t *temperature, double *q_out);

/* ---- test hook: the work list of the object's last two-pass launch table (GrtGasOpticsArgs.tile_items: a launch of few
 * workgroups cuts crowded tiles by line count) and the per-tile candidate ranges it was cut from, as the host built them.
 * *num_items / *num_tiles: counts (0 before the first launch of the two-pass form); items: host [num_items][4] = {tile,
 * first line, one past the last, ordinal}, ranges: host [num_tiles][2]; either may be NULL to ask for the counts only. */
EXTERN int grt_debug_tile_items(GasOptics_t *gas_optics, uint32_t *num_items, uint32_t *items, uint64_t *num_tiles,
                                uint32_t *ranges);

/* ---- test hook: what a pipeline object holds between calls, from its host bookkeeping alone (nothing is launched, nothing
 * waits).  counts [3]: the scratch slots per band (the GRT_SCRATCH_... enumerators of grt_pipeline_internal.h), the
 * pinned staging buffers of the object and the keyed tables per band, always written.  scratch_doubles: host [2][counts[0]],
 * the capacity in doubles of every slot of the longwave, then of the shortwave band, in the enumerators' order;
 * staging_doubles: host [counts[1]], the capacity of every GrtStaging member of the object in the order the struct
 * declares them; key_bytes: host [2][counts[2]], the length of the key every GrtKeyedTable of a band was built for and of its
 * kdist_table, in the order the struct declares them, 0 where none is stored.  Any of the three may be NULL: a caller asks
 * for the counts first (tests/test_gpu_pipeline_history.py). */
EXTERN int grt_debug_pipeline_holdings(GrtPipeline_t const *pipeline, int *counts, uint64_t *scratch_doubles,
                                       uint64_t *staging_doubles, uint64_t *key_bytes);

#endif
