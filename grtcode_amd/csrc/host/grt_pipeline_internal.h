/* grt_pipeline_internal.h -- what the three files of the batched pipeline share: the object (grt_pipeline.c), what turns a
 * caller's clouds, aerosols and bin edges into device arguments (grt_pipeline_inputs.c), and the solves of one band
 * (grt_pipeline_solve.c).  Nothing here is exported from the shared library. */
#ifndef GRT_PIPELINE_INTERNAL_H_
#define GRT_PIPELINE_INTERNAL_H_

#include "grt_internal.h"

/* A device table of ints that depends only on a few host inputs (its key): rebuilt when a call's key differs from the
   one it was built for (grt_keyed_table). */
typedef struct GrtKeyedTable
{
    int *table;            /* device */
    void *key;             /* host: the bytes the table was built from; NULL: the table holds nothing that can be relied on */
    size_t key_bytes;
} GrtKeyedTable;
/* writes the host table for the key at hand from the caller's ctx */
typedef int (*GrtTableFill)(void *ctx, int *table);

/* The host inputs of a k-distribution call on the device (grt_kdist.c): one block -- the class edges [K - 1], the weight
   [n] where one is given, then the bin edges [num_bins + 1] --, uploaded again when a call's bytes differ from the ones it
   holds. */
typedef struct GrtKdistTable
{
    void *block;           /* device */
    void *key;             /* host: the bytes the block was uploaded from, in its order; NULL: nothing that can be relied on */
    size_t key_bytes;
    size_t num_edges;      /* class edges the block was laid out for */
    size_t num_weights;    /* n, or 0: no weight */
} GrtKdistTable;

/* Per-batch inputs: a pinned host buffer, refilled every call, and its device copy. */
typedef struct GrtStaging
{
    double *h, *d;
    size_t doubles;        /* capacity of each */
    void *uploaded;        /* event: h has been copied out and may be refilled */
} GrtStaging;

/* A device buffer of doubles that a call allocates when it first needs it and replaces when it needs a larger one
   (grt_scratch_need); every band's are freed by walking them (grt_pipeline_release). */
typedef struct GrtScratch
{
    double *d;
    size_t doubles;        /* its capacity */
} GrtScratch;

enum
{
    /* fused form, shortwave: [max_cols][2 V + 5 L][n] first-sweep reflectances and layer properties of the two-sweep form
       (10.8 GB for 64 columns of the 1 cm-1 band), which the level forms share with the two-sweep six-row forms */
    GRT_SCRATCH_PARK,
    /* fused form, grt_pipeline_run_profiles (and _allsky_profiles: both passes in turn): [max_cols][2 V][nblocks] */
    GRT_SCRATCH_LEVEL_PARTIALS,
    /* materialised form of the all-sky and the aerosol pass and of grt_pipeline_run_sky's pass with both (the passes of
       a call take the block in turn, in stream order): Rayleigh [3][L][n], zeros [L][n], then the spread objects' tau,
       omega, g [3 objects][max_cols][L][n] (aerosol: 3 arrays, liquid and ice: 6, all three: 9, the aerosol first),
       replaced when a pass needs more arrays */
    GRT_SCRATCH_SPREAD,
    /* grt_pipeline_run_spectral's and grt_pipeline_run_band_profiles' partial sums: [max_cols][6 or 2 V][bin_per_row] */
    GRT_SCRATCH_BIN_PARTIALS,
    /* grt_pipeline_run_subcolumns, fused form: [max_cols][S][6 or 2 V][nblocks] partial sums of the all-sky pass */
    GRT_SCRATCH_SUB_PARTIALS,
    /* ... materialised form: [2][max_cols][V][n] sums of the subcolumns' up and down fluxes */
    GRT_SCRATCH_FLUX_SUM,
    /* grt_pipeline_set_surface: the columns' rows [max_cols][n] -- the emissivity (longwave) or the direct albedo
       (shortwave), and -- shortwave, when a diffuse albedo was given -- the diffuse albedo */
    GRT_SCRATCH_SURF_ROWS,
    GRT_SCRATCH_SURF_ROWS_DIF,
    /* grt_pipeline_run_zeniths and grt_pipeline_run_sky_zeniths (its sets take the block in turn, in stream order),
       shortwave: [max_cols][Z][S][6 or 2 V][nblocks] partial sums of every angle and cloud draw, S = 1 but in a cloud set
       (materialised form: [max_cols][Z][S][6 or 2 V] integrated rows) */
    GRT_SCRATCH_ZEN_PARTIALS,
    /* grt_pipeline_run_sky_direct, shortwave, fused form: [max_cols][S][3 or V][nblocks] partial sums of the direct beam;
       the longwave band's blocks of these four names hold the same of grt_pipeline_run_sky_jacobian's surface-temperature
       Jacobian (each band has one such third row group at most) */
    GRT_SCRATCH_DIRECT_PARTIALS,
    /* ... materialised form: [max_cols][V][n] the direct beam of the pass just solved (fixed size: direct_rows_d points
       into it), and -- with subcolumns -- [max_cols][V][n] its sum */
    GRT_SCRATCH_DIRECT_BEAM,
    GRT_SCRATCH_DIRECT_SUM,
    /* ... profile form without direct_level_fluxes_dev: [max_cols][GRT_SKY_MAX_SETS][V] the levels its three rows come from */
    GRT_SCRATCH_DIRECT_LEVELS,
    /* grt_pipeline_run_sky_radiances, longwave, both forms: [max_cols][S][A][2][nblocks] partial sums of the radiances of
       every angle and cloud draw, S = 1 but in a cloud set of several draws; sized at the first call that needs more */
    GRT_SCRATCH_RADIANCE_PARTIALS,
    /* grt_pipeline_run_sky_channels, longwave, both forms: [max_cols][S][A][2][P] the channels' partial sums per (channel,
       solver block) pair of every angle and cloud draw, S the draws of the call's cloud sets (1 without one) for every
       set of the call; sized at the first call that needs more */
    GRT_SCRATCH_CHANNEL_PARTIALS,
    /* grt_pipeline_run_sky_weighting, longwave, both forms: [max_cols][S][A][R][P] the partial sums of the channels'
       transmittance and contribution rows per (channel, solver block) pair, S as above, R the rows asked for (V
       transmittances, V + 1 contributions; 2 V + 1 for both); sized at the first call that needs more */
    GRT_SCRATCH_WEIGHTING_PARTIALS,
    /* grt_pipeline_run_kdist_correlated without a map_dev of the caller's: the band's class map, [max_cols][n] unsigned
       shorts (in doubles, rounded up) */
    GRT_SCRATCH_KDIST_MAP,
    /* grt_pipeline_run_ck_fluxes, what the caller takes no copy of: the class weights [max_cols][bins][K], the class sums of
       tau [max_cols][L][bins][K] and of the sources [max_cols][2 V + 1 or 4][bins][K]; each replaced when a call's bins x K
       need more (its map: GRT_SCRATCH_KDIST_MAP) */
    GRT_SCRATCH_CK_WEIGHT,
    GRT_SCRATCH_CK_TAU,
    GRT_SCRATCH_CK_SOURCE,
    /* grt_pipeline_run_sky_tiles: the tiles' rows [max_cols T][n] -- the emissivity (longwave) or the direct albedo
       (shortwave), and -- shortwave, when a diffuse albedo was given -- the diffuse albedo; replaced when a call's T needs
       more */
    GRT_SCRATCH_TILE_ROWS,
    GRT_SCRATCH_TILE_ROWS_DIF,
    /* ... [max_cols][T][S][6][nblocks] partial sums of every tile and cloud draw, S = 1 but in a cloud set, its sets in
       turn in stream order (materialised form: [max_cols][T][S][6] integrated rows); replaced when a call needs more */
    GRT_SCRATCH_TILE_PARTIALS,
    /* grt_pipeline_run_sky_weighted, both forms: [max_cols][S][P][G V] the responses' partial sums per (response, solver
       block) pair, S the draws of the call's cloud sets (1 without one) for every set of the call, G = 2 (longwave) or 3
       (shortwave); sized at the first call that needs more */
    GRT_SCRATCH_RESPONSE_PARTIALS,
    /* grt_pipeline_run_sky_scattering, longwave, both forms: the scattering kernel's park block (GrtScatterArgs), max_cols
       grid rows of (V - 1) x GRT_SCATTER_PARK_ROWS rows of the band's points rounded up to the solver block; allocated at
       the first such call */
    GRT_SCRATCH_SCATTER_PARK,
    /* ... [max_cols][S][6 or 2 V][nblocks] partial sums of the differences of every draw, S = 1 but in a cloud set of
       several draws, its sets in turn in stream order (materialised form: [max_cols][S][6 or 2 V] integrated rows) */
    GRT_SCRATCH_SCATTER_PARTIALS,
    /* ... profile form without scatter_levels_dev: [max_cols][GRT_SKY_MAX_SETS][2][V] the levels its six rows come from */
    GRT_SCRATCH_SCATTER_LEVELS,
    /* grt_pipeline_run_sky_zeniths_direct, shortwave, fused form: [max_cols][Z][S][3 or V][nblocks] partial sums of the
       direct beam of every angle and cloud draw, its sets in turn in stream order (materialised form: [max_cols][Z][S][3 or
       V] integrated rows); replaced when a call needs more */
    GRT_SCRATCH_ZEN_DIRECT_PARTIALS,
    /* ... profile form without zenith_direct_level_fluxes_dev: [max_cols][GRT_SKY_MAX_SETS][Z][V] the levels every angle's
       three rows come from (the mean's: GRT_SCRATCH_DIRECT_LEVELS) */
    GRT_SCRATCH_ZEN_DIRECT_LEVELS,
    /* ... materialised form with a GrtZenithSurface_t: [max_cols][n] the direct-albedo rows of the angle being solved (the
       rows of the surface in force, GRT_SCRATCH_SURF_ROWS, are not written) */
    GRT_SCRATCH_ZEN_SURF_ROWS,
    /* grt_pipeline_run_sky_zeniths_slant, shortwave: [max_cols][Z][L] the direct beam's cosine of every layer under every
       angle, copied from the caller's array once per call; replaced when a call needs more */
    GRT_SCRATCH_ZEN_SLANT,
    GRT_SCRATCH_COUNT
};

typedef struct GrtBand
{
    GasOptics_t *gas;
    uint64_t n;            /* grid points */
    double *tau_gas;       /* [cols][L][n] */
    int tau_gas_lacks_tables;      /* the last run left the spectral tables' part to the solver (grt_pipeline_views completes it) */
    int last_cols;
    double *tau, *omega, *g;
    double *flux_up, *flux_down;   /* [cols][V][n] */
    double **rows_d;       /* [cols][6] device row pointers for the trapezoid */
    double *zero_row;      /* [n] zeros: stands in for the user level when there is none */
    /* fused form (no spectra kept): */
    double *partials;      /* [cols][6][nblocks] trapezoid partial sums */
    unsigned nblocks;
    /* grt_pipeline_run_profiles (and _allsky_profiles), materialised form, allocated at the first call: [cols][2 V] device
       row pointers (up levels, then down levels) */
    double **level_rows_d;
    /* grt_pipeline_run_sky_direct (longwave band: grt_pipeline_run_sky_jacobian), materialised form, allocated at the first call of each form: device row pointers into
       GRT_SCRATCH_DIRECT_BEAM, [0]: [cols][3] (TOA, surface, user level or the zero row), [1]: [cols][V] */
    double **direct_rows_d[2];
    GrtScratch scratch[GRT_SCRATCH_COUNT];     /* what the calls allocate on demand (GRT_SCRATCH_...) */
    /* grt_pipeline_run_allsky (and _allsky_profiles): [2][n] cloud band of each grid point (liquid, ice), -1: none; its key:
       the band limits (B, num_ice_bands, liquid lo/hi, ice lo/hi) */
    GrtKeyedTable cloud_map;
    /* grt_pipeline_run_aerosols: [n] interval of the band's aerosol grid each grid point lies in, -1: none; its key: that
       grid */
    GrtKeyedTable aer_map;
    /* grt_pipeline_run_spectral's and grt_pipeline_run_band_profiles' bins (they run in stream order): grt_bin_table of
       the edges [bin_count + 1] (its key) */
    GrtKeyedTable bin_table;
    size_t bin_per_row;    /* partial sums per row */
    /* grt_pipeline_run_kdist: this band's class edges, weight and bin edges on the device */
    GrtKdistTable kdist_table;
    /* grt_pipeline_set_surface: [n] entry of the band's surface grid each grid point takes (grt_surface_entry_map); its key:
       that grid */
    GrtKeyedTable surf_map;
    /* grt_pipeline_run_sky_channels (longwave band): the instrument's table (GrtChannelArgs: weights, sums and centers,
       then the channels' and the blocks' ints); its key: the grid's points and the channels' first, offset, weights, center */
    GrtKeyedTable channel_table;
    /* grt_pipeline_run_sky_tiles: [n] entry of the band's tile grid each grid point takes, as surf_map; its key: that grid */
    GrtKeyedTable tile_map;
    /* grt_pipeline_run_sky_weighted: the band's response table (GrtResponseArgs: the weights, then the responses' and the
       blocks' ints); its key: the grid's points and the responses' first, offset, weights */
    GrtKeyedTable response_table;
    /* grt_pipeline_run_sky_zeniths_direct (shortwave band): [n] entry of the call's albedo grid each grid point takes, as
       surf_map; its key: that grid */
    GrtKeyedTable zen_surf_map;
    int surf_set, surf_dif_set;   /* the surface in force gives this band rows (, and diffuse rows of their own) */
} GrtBand;

struct GrtPipeline
{
    Device_t device;
    int lane;              /* the lane selected when the pipeline was created: grt_pipeline_stream names THAT stream */
    int max_cols, num_levels, user_level;
    int keep_spectra;      /* 0: fused solvers, integrated fluxes only (production); 1: tau/omega/g and fluxes materialised */
    GrtBand band[2];       /* 0: longwave, 1: shortwave */
    GrtStaging small;      /* the small per-column inputs, at the offsets below */
    size_t off_n, off_tl, off_tv, off_ts, off_mu, off_tsi, off_p, small_doubles;
    double *emis_d, *albedo_d, *solar_d;
    /* grt_pipeline_run_allsky's band tables: [cols][L] thickness, then [cols][3][B][L] of the longwave liquid, longwave ice,
       shortwave liquid, shortwave ice */
    GrtStaging cloud;
    /* grt_pipeline_run_aerosols' slope and intercept tables: the longwave's [cols][3][NA - 1][2][L], then the shortwave's */
    GrtStaging aer;
    /* grt_pipeline_set_surface's slope and intercept entries: the emissivity's [cols][NS + 1][2], then the direct albedo's,
       then the diffuse albedo's */
    GrtStaging surf;
    /* grt_pipeline_run_zeniths' angles: cos_zenith [cols][Z], the weights [cols][Z], then -- materialised form -- the
       cosines angle-major [Z][cols], night samples replaced by a day angle of their column */
    GrtStaging zen;
    /* grt_pipeline_run_sky_radiances' viewing secants [cols][A] */
    GrtStaging rad;
    /* grt_pipeline_run_sky_tiles' inputs: the temperatures [cols][T], the same tile-major [T][cols] (materialised form), the
       fractions [cols][T], then the slope and intercept entries of the tiles' emissivity [cols T][NS + 1][2], direct albedo
       and diffuse albedo */
    GrtStaging tile;
    /* grt_pipeline_run_sky_zeniths_direct's slope and intercept entries of the direct albedo: [cols][Z][NS + 1][2], or --
       materialised form -- angle-major [Z][cols][NS + 1][2] */
    GrtStaging zen_surf;
    int surface_ncol;     /* columns of the surface in force; 0: none (the creation-time arrays apply) */
};

/* The bins of a run, per band.  Of a six-row run (grt_pipeline_run_spectral): with the six rows at every point, to
   spectral, and their bins, to binned; of a profile run (grt_pipeline_run_band_profiles): every level's flux per bin, the
   run's output. */
typedef struct GrtBins
{
    double *spectral, *binned;     /* the six-row run's */
    int const *edges[2];
    int num_bins[2];
} GrtBins;

/* The viewing angles of a grt_pipeline_run_sky_radiances call, staged (grt_stage_radiances): A secants per column on the
   device, and where every set's radiances go. */
typedef struct GrtRadianceRun
{
    int angles;
    double const *secant;          /* DEVICE [ncol][A] */
    double *integrated;            /* DEVICE [ncol][sets][A][2] */
    double *spectral, *brightness; /* DEVICE [ncol][sets][A][2][n], or NULL */
} GrtRadianceRun;

/* The channels of a grt_pipeline_run_sky_channels call, staged (grt_stage_channels): the instrument's table on the device
   (args.partials: set by the pass's launch), and where every set's channel outputs go. */
typedef struct GrtChannelRun
{
    GrtChannelArgs args;
    double *radiances, *brightness; /* DEVICE [ncol][sets][A][2][C]; brightness may be NULL */
    int slots;                      /* slots per column of the scratch: the most draws any set of the call has, so that the
                                       call's first set sizes GRT_SCRATCH_CHANNEL_PARTIALS for all of them */
} GrtChannelRun;

/* The profiles of a grt_pipeline_run_sky_weighting call, staged (grt_stage_weighting): which row groups leave
   (args.partials: set by the pass's launch), and where every set's go. */
typedef struct GrtWeightingRun
{
    GrtWeightingArgs args;
    double *transmittance;          /* DEVICE [ncol][sets][A][V][C], or NULL */
    double *contribution;           /* DEVICE [ncol][sets][A][V + 1][C], or NULL */
} GrtWeightingRun;

/* The responses of a grt_pipeline_run_sky_weighted call on one band, staged (grt_stage_responses): the band's table on the
   device (args.partials: set by the pass's launch), and where every set's rows of the band go. */
typedef struct GrtResponseRun
{
    GrtResponseArgs args;
    int groups;                     /* G: 2 (longwave: up, down) or 3 (shortwave: up, down, direct) */
    double *out;                    /* DEVICE: the band's rows of column 0, set 0 in weighted_levels_dev */
    uint64_t set_doubles;           /* (2 R_lw + 3 R_sw) V: from one set to the next */
    int slots;                      /* slots per column of the scratch: the most draws any set of the call has */
} GrtResponseRun;

/* The scattering correction of a grt_pipeline_run_sky_scattering call: where every set's differences go, in the layout of
   the run's longwave rows -- [ncol][sets][6], or (profile) [ncol][sets][2][V], up then down. */
typedef struct GrtScatterRun
{
    double *out;
} GrtScatterRun;

/* One solve of a band on the run's tau_gas.  What joins gas and Rayleigh: nothing (clear sky), the cloud objects (all-sky
   pass), the aerosol object (aerosol pass; aer NULL there: a band that was given no aerosol, which runs the form without
   the object under the aerosol pass's profile tags) or both (grt_pipeline_run_sky's complete set).  Which rows leave: the six of driver.c:272-280 or (profile) every level's
   up then down flux, to set `set` of the `sets` in the column's out_stride doubles at out; with bins, the six rows at
   every point and their bins too (grt_pipeline_run_spectral) or (profile) every level's flux per bin of the edges
   instead, to out's [ncol][sets][2 lw bins + 2 sw bins][V] (grt_pipeline_run_band_profiles). */
typedef struct GrtPass
{
    GrtCloudArgs const *clouds;
    GrtAerosolArgs const *aer;
    int aer_pass;
    int profile;
    int defer;                     /* the solver adds the spectral tables' part of tau, from continua (band_gas_optics) */
    GrtContinua const *continua;
    double *out;
    int out_stride;
    int sets;
    int set;                       /* its place among the column's sets: 0 the clear-sky set, then the others as packed */
    GrtBins const *bins;
    /* grt_pipeline_run_sky_direct (NULL: not asked for): the shortwave's direct beam leaves too, the pass's three rows
       (TOA, surface, user level) or -- profile -- V levels to set `set` of direct [ncol][sets][3 or V] */
    double *direct;
    /* grt_pipeline_run_sky_jacobian (NULL: not asked for): the longwave's dF_up/dT_surf leaves too, laid out as direct is */
    double *jacobian;
    /* grt_pipeline_run_sky_radiances (NULL: not asked for): the longwave's radiance kernel is queued behind the pass's
       solver -- out NULL: in its place --, the pass's to set `set` of each output */
    GrtRadianceRun const *radiances;
    /* grt_pipeline_run_sky_channels (NULL: not asked for; with radiances only): that kernel in its channel form, and the
       channels' finishing kernel behind it */
    GrtChannelRun const *channels;
    /* grt_pipeline_run_sky_weighting (NULL: not asked for; with channels only): the weighting kernel behind that one, and
       its finishing kernel beside the channels' */
    GrtWeightingRun const *weighting;
    /* grt_pipeline_run_sky_tiles (NULL: not asked for; six rows only): every band's solve is grt_band_solve_tiles', the mean
       over the tiles to out (may be NULL) and every tile's rows to the pass's set of tiles->per_tile */
    struct GrtTileRun const *tiles;
    /* grt_pipeline_run_sky_weighted (NULL: not asked for, or the band has no responses; profile form only, the shortwave
       with `direct`): the band's level rows leave under its responses too, to the pass's set of responses->out */
    GrtResponseRun const *responses;
    /* grt_pipeline_run_sky_scattering (NULL: not asked for): the longwave's scattering kernel is queued behind the pass's
       solver, on its instance and arguments, and the pass's differences go to set `set` of scatter->out */
    GrtScatterRun const *scatter;
} GrtPass;

/* The surface tiles of a grt_pipeline_run_sky_tiles call, staged (grt_stage_tiles): T per column, their temperatures and
   fractions on the device, each band's rows in its GRT_SCRATCH_TILE_ROWS(_DIF) where the band was given knots, and where
   every tile's own rows go. */
typedef struct GrtTileRun
{
    int tiles;
    double const *t_surf;          /* DEVICE [ncol][T] */
    double const *t_surf_by_tile;  /* DEVICE [T][ncol] (materialised form) */
    double const *fraction;        /* DEVICE [ncol][T], or NULL */
    int np[2];                     /* the knots each band was given; 0: every tile takes the surface in force */
    int dif;                       /* the shortwave was given a diffuse albedo of its own */
    double *per_tile;              /* DEVICE [ncol][sets][T][12], or NULL */
} GrtTileRun;

/* The sun angles of a grt_pipeline_run_zeniths or grt_pipeline_run_sky_zeniths call, staged (grt_stage_zeniths): Z per column, their cosines and weights
   on the device, and where every angle's own rows go. */
typedef struct GrtZenithRun
{
    int zeniths;
    double const *mu;              /* DEVICE [ncol][Z] */
    double const *weight;          /* DEVICE [ncol][Z], or NULL */
    double const *mu_by_angle;     /* DEVICE [Z][ncol], a day angle everywhere (materialised form) */
    double *per_angle;             /* DEVICE [ncol][Z][6 or 2 V], or NULL */
    double *six;                   /* profile form: DEVICE [ncol][Z][6], every angle's six rows from its levels, or NULL */
    int sky;                       /* grt_pipeline_run_sky_zeniths: both carry the pass's sets, [ncol][sets][Z][...] */
    /* grt_pipeline_run_sky_zeniths_direct (all zero: not asked for).  The (column, angle) direct albedo, staged
       (grt_stage_zenith_surface): surface.tables [ncol][Z][E][2] -- materialised form: [Z][ncol][E][2], angle k's columns
       at k ncol E 2 --, surface.entry the band's map; surface.tables NULL: the surface in force under every angle */
    GrtZenithSurfaceArgs surface;
    /* ... the direct beam leaves too (direct != 0): every angle's rows to direct_per_angle, DEVICE [ncol][sets][Z][3 or V],
       and their mean to direct_out, DEVICE [ncol][sets][3 or V] (either may be NULL, not both) */
    int direct;
    double *direct_per_angle, *direct_out;
    /* grt_pipeline_run_sky_zeniths_slant (mu_layer NULL: not asked for): the direct beam's cosine per layer, DEVICE
       [ncol][Z][L]; the fused instances then carry the direct beam whether or not `direct` asks for its rows */
    GrtZenithSlantArgs slant;
} GrtZenithRun;

/* the doubles from one set of a column to the next */
static inline int grt_set_offset(GrtPipeline_t const *p, int profile)
{
    return profile ? GRT_PROFILE_ROWS_PER_COLUMN*p->num_levels : GRT_FLUXES_PER_COLUMN;
}

static inline int grt_aerosol_points(GrtAerosols_t const *ae, int bi)
{
    return bi == 0 ? ae->lw_num_points : ae->sw_num_points;
}

/* grt_pipeline.c */
GRT_PRIVATE int grt_scratch_need(GrtPipeline_t *p, GrtScratch *buf, size_t doubles, int *fresh);
/* the row-pointer table rows_h [n] (integrate_rows' rows) to the device at *rows_d; rows_h is freed */
GRT_PRIVATE int grt_upload_rows(GrtPipeline_t *p, double **rows_h, size_t n, double ***rows_d);

/* grt_pipeline_inputs.c */
GRT_PRIVATE int grt_staging_reserve(GrtPipeline_t *p, GrtStaging *st, size_t need, size_t want);
GRT_PRIVATE int grt_staging_upload(GrtPipeline_t *p, GrtStaging *st, size_t need);
GRT_PRIVATE void grt_staging_free(GrtPipeline_t *p, GrtStaging *st);
GRT_PRIVATE void grt_keyed_table_free(GrtPipeline_t *p, GrtKeyedTable *t);
GRT_PRIVATE int grt_stage_clouds(GrtPipeline_t *p, GrtClouds_t const *cl, int C, int S);
GRT_PRIVATE int grt_stage_cloud_fields(GrtPipeline_t *p, GrtClouds_t const *cl, GrtCloudSampler_t *sampler,
                                       GrtCloudFields_t const *fields, fp_t const *temperature, int C, int S);
GRT_PRIVATE int grt_band_clouds(GrtPipeline_t *p, GrtBand *b, int bi, GrtClouds_t const *cl, int C, int S, GrtCloudArgs *ca);
GRT_PRIVATE int grt_stage_aerosols(GrtPipeline_t *p, GrtAerosols_t const *ae, int C);
GRT_PRIVATE int grt_band_aerosols(GrtPipeline_t *p, GrtBand *b, int bi, GrtAerosols_t const *ae, int C, GrtAerosolArgs *aa);
GRT_PRIVATE int grt_check_grid(char const *name, char const *kind, char const *none, char const *what, int nx,
                               fp_t const *grid, fp_t const *values);
GRT_PRIVATE int grt_check_surface(GrtPipeline_t const *p, GrtSurface_t const *sf, int np[2]);
GRT_PRIVATE int grt_stage_surface(GrtPipeline_t *p, GrtSurface_t const *sf, int const np[2]);
GRT_PRIVATE int grt_check_tiles(GrtPipeline_t const *p, GrtSurfaceTiles_t const *tl, int C, int np[2]);
GRT_PRIVATE int grt_stage_tiles(GrtPipeline_t *p, GrtSurfaceTiles_t const *tl, int C, int const np[2], GrtTileRun *tr);
GRT_PRIVATE int grt_stage_zeniths(GrtPipeline_t *p, GrtZeniths_t const *zn, int C, GrtZenithRun *zr);
/* what grt_pipeline_run_sky_zeniths_direct refuses in its surface for C columns under Z angles (nothing is touched); the
   checked surface's pairs to the device and the shortwave band's entry map brought up to date, as zr->surface */
GRT_PRIVATE int grt_check_zenith_surface(GrtZenithSurface_t const *zs, int C, int Z);
GRT_PRIVATE int grt_stage_zenith_surface(GrtPipeline_t *p, GrtZenithSurface_t const *zs, int C, GrtZenithRun *zr);
/* what grt_pipeline_run_sky_zeniths_slant refuses in its layer cosines for C columns of L layers under the angles of zn
   (nothing is touched); the checked cosines to the shortwave band's device block, as zr->slant */
GRT_PRIVATE int grt_check_zenith_slant(GrtZenithSlant_t const *sl, GrtZeniths_t const *zn, int C, int L);
GRT_PRIVATE int grt_stage_zenith_slant(GrtPipeline_t *p, GrtZenithSlant_t const *sl, int C, GrtZenithRun *zr);
GRT_PRIVATE int grt_check_radiances(GrtRadiances_t const *rd, int C);
GRT_PRIVATE int grt_stage_radiances(GrtPipeline_t *p, GrtRadiances_t const *rd, int C, GrtRadianceRun *rr);
/* One band's windows as the caller gave them: window k is the points first[k] .. of the grid, offset[k + 1] - offset[k] of
   them, with the weights at weights + offset[k].  The messages call one `band` + `kind` ("shortwave " + "response", "" +
   "channel").  grt_check_windows: what both kinds are refused for on a grid of n points, and their (window, block) pairs. */
typedef struct GrtWindows
{
    int count;
    int const *first, *offset;
    fp_t const *weights;
    char const *kind, *band;
} GrtWindows;
GRT_PRIVATE int grt_check_windows(GrtWindows const *w, long long n, long long *pairs);
GRT_PRIVATE int grt_check_channels(GrtChannels_t const *ch, long long n, long long *pairs);
GRT_PRIVATE int grt_stage_channels(GrtPipeline_t *p, GrtBand *b, GrtChannels_t const *ch, long long pairs,
                                   GrtChannelRun *cr);
/* one band's responses (bi: 0 longwave, 1 shortwave) on a grid of n points and at most block_limit in one block (< 0: not
   checked); *pairs, *block_max: its (response, block) pairs and the most responses in one block */
GRT_PRIVATE int grt_check_responses(GrtResponses_t const *rs, int bi, long long n, int block_limit, long long *pairs,
                                    int *block_max);
GRT_PRIVATE int grt_stage_responses(GrtPipeline_t *p, GrtBand *b, int bi, GrtResponses_t const *rs, long long pairs,
                                    int block_max, GrtResponseRun *rr);
GRT_PRIVATE int grt_check_weighting(GrtWeighting_t const *wt);
GRT_PRIVATE void grt_stage_weighting(GrtWeighting_t const *wt, GrtWeightingRun *wr);
GRT_PRIVATE int grt_band_bins(GrtPipeline_t *p, GrtBand *b, int const *edges, int nbins, int rows);
/* the rules of a band's bin edges on a grid of n points (`name`: the band's, for the messages): none, or num_bins + 1
   strictly increasing grid-point indices in 0 .. n - 1, and an output to write them to */
GRT_PRIVATE int grt_check_bin_edges(char const *name, int const *edges, int num_bins, long long n, int has_output);

/* grt_kdist.c: the checks of the classes and of one band's inputs on a grid of n points (its edges apart); the band's
   inputs brought up to date in *t and the reduction of tau_dev [rows][n] queued on the device's current lane; *t freed */
GRT_PRIVATE int grt_kdist_check_classes(int num_classes, fp_t const *class_edges);
GRT_PRIVATE int grt_kdist_check_band(char const *name, GrtKdistBand_t const *band, long long n);
GRT_PRIVATE int grt_kdist_reduce(Device_t device, GrtKdistTable *t, fp_t const *tau_dev, long long rows, long long n,
                                 fp_t dw, int num_classes, fp_t const *class_edges, GrtKdistBand_t const *band);
GRT_PRIVATE void grt_kdist_table_free(Device_t device, GrtKdistTable *t);
/* ... the correlated form: a key's rules for groups of rows_per_group rows (*row: the key row, -1: the rows' sum); the map
   of tau_dev [groups][rows_per_group][n] under that key queued to map_dev, and every row's reduction under it behind it */
GRT_PRIVATE int grt_kdist_check_key(char const *name, int kind, long long key_row, long long rows_per_group, long long *row);
GRT_PRIVATE int grt_kdist_reduce_correlated(Device_t device, GrtKdistTable *t, fp_t const *tau_dev, long long groups,
                                            long long rows_per_group, long long n, fp_t dw, int num_classes,
                                            fp_t const *class_edges, long long key_row, unsigned short *map_dev,
                                            GrtKdistBand_t const *band);
/* ... grt_pipeline_run_ck_fluxes' form of it: the class edges may be NULL (none on the device), a given map takes the
   place of the key's (no map kernel, map_dev not written), no weight; *edges_dev: the bin edges on the device */
GRT_PRIVATE int grt_kdist_reduce_ck(Device_t device, GrtKdistTable *t, fp_t const *tau_dev, long long groups,
                                    long long rows_per_group, long long n, fp_t dw, int num_classes,
                                    fp_t const *class_edges, long long key_row, unsigned short const *map_given_dev,
                                    unsigned short *map_dev, GrtKdistBand_t const *band, int const **edges_dev);

/* grt_pipeline_solve.c */
/* the source sums, the solve and the bin sums of grt_pipeline_run_ck_fluxes for one band, on the class weights and class
   sums of tau the mapped reduction left at weight_sum, tau_sum */
GRT_PRIVATE int grt_band_solve_ck(GrtPipeline_t *p, GrtBand *b, int bi, int C, int num_classes, int const *edges_dev,
                                  unsigned short const *map_dev, double const *weight_sum, double const *tau_sum,
                                  double *source_sum, GrtCkBand_t const *out);
GRT_PRIVATE int grt_band_solve(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps);
GRT_PRIVATE int grt_band_solve_subcolumns(GrtPipeline_t *p, GrtBand *b, int bi, int C, int S, GrtPass const *ps);
GRT_PRIVATE int grt_band_solve_tiles(GrtPipeline_t *p, GrtBand *b, int bi, int C, int S, GrtPass const *ps);
GRT_PRIVATE int grt_band_solve_zeniths(GrtPipeline_t *p, GrtBand *b, int C, int S, GrtPass const *ps,
                                       GrtZenithRun const *zr);

#endif
