/* grt_pipeline.c -- batched, device-resident clear-sky flux pipeline (grt_ext.h).
 *
 * This is the production shape of the hot path: what framework/src/driver.c does per
 * column in column_calculation() (driver.c:360-424: set ppmv -> calculate_optical_depth
 * -> rayleigh_scattering -> add_optics -> calculate_{lw,sw}_fluxes -> output_fluxes with
 * -integrated, driver.c:285-356), done for a whole batch of columns with
 *   - one host prologue + one small upload per column (layer state, a few kB),
 *   - one line-by-line launch per band for the batch,
 *   - one solver launch per band that forms Rayleigh and the two-object optics combination per layer
 *     in registers from tau_gas (no tau/omega/g arrays, no per-column allocation as in optics.c:84-124),
 *     keeps no spectral flux and leaves the trapezoid of the six output rows as per-block partial sums
 *     (wavefront shuffles + LDS), and one tiny launch that adds the blocks in a fixed order: 6 numbers
 *     per band and column on the device (ready for an RCCL gather; nothing crosses PCIe),
 *   - or, for callers that want spectra (grt_pipeline_create_ex(..., keep_spectra = 1): parity tests, a
 *     driver without -integrated), the materialised form: one streaming Rayleigh + combine pass,
 *     solvers writing [level][wavenumber] fluxes, a row-wise trapezoid launch.
 * grt_pipeline_run_profiles runs the same prologue and gas optics, then the profile form of the solvers (every level's
 * flux summed per block in-kernel, or -- materialised form -- integrated row by row from the spectra) and one small
 * kernel that forms the level fluxes, the heating rates and the six-row output from them.
 * grt_pipeline_run_allsky runs grt_pipeline_run's clear-sky pass and then, on the same tau_gas, the all-sky pass of
 * driver.c:474-597: the cloud objects formed from band tables inside the solvers (or, materialised form, spread onto the
 * grid and added by the add_optics kernel).
 * grt_pipeline_run_allsky_profiles runs both: the profile form of the clear-sky pass, then of the all-sky pass, on one
 * tau_gas, and one finishing launch for the two sets.
 * grt_pipeline_run_subcolumns runs either of the two with the all-sky pass averaged over several cloud subcolumns, all of
 * them on the one tau_gas.
 * grt_pipeline_run_aerosols runs the clear-clean pass of grt_pipeline_run or grt_pipeline_run_profiles and then, on the
 * same tau_gas, the clear-sky pass with aerosols of driver.c:426-472: the aerosol object formed inside the solvers from
 * per-column slope and intercept tables (or, materialised form, spread onto the grid and added by the add_optics kernel).
 * All work is enqueued on the device's library stream; nothing synchronises.
 */
#include <stdlib.h>
#include <string.h>
#include "grt_internal.h"

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
    double *park;          /* shortwave: [cols][2 V + 5 L][n] first-sweep reflectances and layer properties */
    double *partials;      /* [cols][6][nblocks] trapezoid partial sums */
    unsigned nblocks;
    /* grt_pipeline_run_profiles (and _allsky_profiles: both passes in turn), allocated at the first call: */
    double *level_partials;        /* fused form: [cols][2 V][nblocks] */
    double **level_rows_d;         /* materialised form: [cols][2 V] device row pointers (up levels, then down levels) */
    /* grt_pipeline_run_allsky (and _allsky_profiles): */
    int *cloud_map;        /* [2][n] cloud band of each grid point (liquid, ice), -1: none */
    double *cloud_key;     /* host: the band limits cloud_map was built for (B, num_ice_bands, liquid lo/hi, ice lo/hi) */
    size_t cloud_key_n;
    double *cloud_block;   /* materialised form: liquid and ice tau, omega, g [6][cols][L][n], Rayleigh [3][L][n], zeros [L][n] */
    /* grt_pipeline_run_spectral's bins: */
    int *bin_edges;        /* host: the edges bin_table was built for [bin_count + 1] */
    int bin_count;
    int *bin_table;        /* device: grt_bin_table of those edges */
    size_t bin_per_row;    /* partial sums per row */
    double *bin_partials;  /* [max_cols][6][bin_cap] */
    size_t bin_cap;
    /* grt_pipeline_run_subcolumns, allocated at the first call that needs them (or more of them): */
    double *sub_partials;  /* fused form: [max_cols][S][6 or 2 V][nblocks] partial sums of the all-sky pass */
    size_t sub_cap;        /* its doubles */
    double *flux_sum;      /* materialised form: [2][max_cols][V][n] sums of the subcolumns' up and down fluxes */
    /* grt_pipeline_run_aerosols: */
    int *aer_map;          /* [n] interval of the band's aerosol grid each grid point lies in, -1: none */
    double *aer_key;       /* host: the aerosol grid aer_map was built for */
    int aer_key_n;
    double *aer_block;     /* materialised form: aerosol tau, omega, g [3][max_cols][L][n], Rayleigh [3][L][n], zeros [L][n] */
} GrtBand;

struct GrtPipeline
{
    Device_t device;
    int lane;              /* the lane selected when the pipeline was created: grt_pipeline_stream names THAT stream */
    int max_cols, num_levels, user_level;
    int keep_spectra;      /* 0: fused solvers, integrated fluxes only (production); 1: tau/omega/g and fluxes materialised */
    GrtBand band[2];       /* 0: longwave, 1: shortwave */
    /* per-batch small inputs: pinned host staging + device copies */
    double *small_h, *small_d;
    void *small_uploaded;  /* event: small_h has been copied out and may be refilled */
    size_t off_n, off_tl, off_tv, off_ts, off_mu, off_tsi, off_p, small_doubles;
    double *emis_d, *albedo_d, *solar_d;
    /* grt_pipeline_run_allsky's band tables: pinned host staging + device copy, [cols][L] thickness, then [cols][3][B][L]
       of the longwave liquid, longwave ice, shortwave liquid, shortwave ice */
    double *cloud_h, *cloud_d;
    size_t cloud_doubles;
    void *cloud_uploaded;
    /* grt_pipeline_run_aerosols' slope and intercept tables: pinned host staging + device copy, the longwave's
       [cols][3][NA - 1][2][L], then the shortwave's */
    double *aer_h, *aer_d;
    size_t aer_doubles;
    void *aer_uploaded;
};

static void grt_pipeline_release(GrtPipeline_t **pipeline);

/* the row-pointer table rows_h [n] (integrate_rows' rows) to the device at *rows_d; rows_h is freed (after the upload) */
static int upload_rows(GrtPipeline_t *p, double **rows_h, size_t n, double ***rows_d)
{
    void *s = grt_dev_stream(p->device);
    double **d = NULL;
    int rc = grt_dev_alloc(p->device, (void **)&d, sizeof(double *)*n);
    if (rc == GRTCODE_SUCCESS) rc = grt_dev_upload(p->device, d, rows_h, sizeof(double *)*n, s);
    if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(p->device, s);
    free(rows_h);
    if (rc != GRTCODE_SUCCESS)
    {
        grt_dev_free(p->device, d);
        GRT_TRY(rc);
    }
    *rows_d = d;
    return GRTCODE_SUCCESS;
}

static int band_alloc(GrtPipeline_t *p, GrtBand *b, GasOptics_t *gas)
{
    memset(b, 0, sizeof(*b));
    if (gas == NULL)
    {
        return GRTCODE_SUCCESS;
    }
    b->gas = gas;
    b->n = gas->grid.n;
    ((GrtGasOpticsImpl *)gas->impl)->profile_tag = (b == &p->band[0]) ? 1 : 2;
    size_t const L = (size_t)p->num_levels - 1, V = (size_t)p->num_levels, C = (size_t)p->max_cols;
    size_t const opt = sizeof(double)*C*L*b->n, flx = sizeof(double)*C*V*b->n;
    void *blk = NULL;
    if (!p->keep_spectra)
    {
        /* fused form: tau_gas and the partial sums (the shortwave solver's park block -- 2 V + 5 L rows per column, 10.8 GB
           for 64 columns of the 1 cm-1 band -- is allocated when a launch first needs it: its two-sweep form, see run) */
        b->nblocks = grt_solver_blocks(b->n);
        size_t const part = sizeof(double)*C*6*b->nblocks;
        GRT_TRY(grt_dev_alloc(p->device, &blk, opt + part));
        b->tau_gas = blk;
        b->park = NULL;
        b->partials = b->tau_gas + C*L*b->n;
        return GRTCODE_SUCCESS;
    }
    GRT_TRY(grt_dev_alloc(p->device, &blk, 4*opt + 2*flx + sizeof(double)*b->n));
    b->tau_gas = blk;
    b->tau = b->tau_gas + C*L*b->n;
    b->omega = b->tau + C*L*b->n;
    b->g = b->omega + C*L*b->n;
    b->flux_up = b->g + C*L*b->n;
    b->flux_down = b->flux_up + C*V*b->n;
    b->zero_row = b->flux_down + C*V*b->n;
    void *s = grt_dev_stream(p->device);
    GRT_TRY(grt_dev_zero(p->device, b->zero_row, sizeof(double)*b->n, s));
    /* row table: up TOA, up surface, up user, down TOA, down surface, down user (driver.c:272-280) */
    double **rows_h = malloc(sizeof(double *)*C*6);
    if (rows_h == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for the row table of %zu columns.", C);
    }
    for (size_t c = 0; c < C; ++c)
    {
        double *up = b->flux_up + c*V*b->n, *dn = b->flux_down + c*V*b->n;
        rows_h[c*6 + 0] = up;
        rows_h[c*6 + 1] = up + (V - 1)*b->n;
        rows_h[c*6 + 2] = p->user_level >= 0 ? up + (size_t)p->user_level*b->n : b->zero_row;
        rows_h[c*6 + 3] = dn;
        rows_h[c*6 + 4] = dn + (V - 1)*b->n;
        rows_h[c*6 + 5] = p->user_level >= 0 ? dn + (size_t)p->user_level*b->n : b->zero_row;
    }
    GRT_TRY(upload_rows(p, rows_h, C*6, &b->rows_d));
    return GRTCODE_SUCCESS;
}

static int pipeline_build(GrtPipeline_t *p, GasOptics_t *lw_gas, GasOptics_t *sw_gas, int max_columns,
                          fp_t const *emissivity, fp_t const *albedo, fp_t const *solar_flux)
{
    GRT_TRY(grt_dev_require(p->device));
    GRT_TRY(band_alloc(p, &p->band[0], lw_gas));
    GRT_TRY(band_alloc(p, &p->band[1], sw_gas));
    size_t const L = (size_t)p->num_levels - 1, V = (size_t)p->num_levels, C = (size_t)max_columns;
    p->off_n = 0;
    p->off_tl = p->off_n + C*L;
    p->off_tv = p->off_tl + C*L;
    p->off_ts = p->off_tv + C*V;
    p->off_mu = p->off_ts + C;
    p->off_tsi = p->off_mu + C;
    p->off_p = p->off_tsi + C;         /* level pressures [C][V] mb: the heating rates of grt_pipeline_run_profiles */
    p->small_doubles = p->off_p + C*V;
    GRT_TRY(grt_host_alloc_pinned((void **)&p->small_h, sizeof(double)*p->small_doubles));
    GRT_TRY(grt_dev_alloc(p->device, (void **)&p->small_d, sizeof(double)*p->small_doubles));
    void *s = grt_dev_stream(p->device);
    if (lw_gas != NULL)
    {
        GRT_REQUIRE_PTR(emissivity);
        for (uint64_t i = 0; i < lw_gas->grid.n; ++i)
        {
            GRT_REQUIRE_RANGE(emissivity[i], 0., 1.);
        }
        GRT_TRY(grt_dev_alloc(p->device, (void **)&p->emis_d, sizeof(double)*lw_gas->grid.n));
        GRT_TRY(grt_dev_upload(p->device, p->emis_d, emissivity, sizeof(double)*lw_gas->grid.n, s));
    }
    if (sw_gas != NULL)
    {
        GRT_REQUIRE_PTR(albedo);
        GRT_REQUIRE_PTR(solar_flux);
        for (uint64_t i = 0; i < sw_gas->grid.n; ++i)
        {
            GRT_REQUIRE_RANGE(albedo[i], 0., 1.);
        }
        GRT_TRY(grt_dev_alloc(p->device, (void **)&p->albedo_d, sizeof(double)*sw_gas->grid.n));
        GRT_TRY(grt_dev_alloc(p->device, (void **)&p->solar_d, sizeof(double)*sw_gas->grid.n));
        GRT_TRY(grt_dev_upload(p->device, p->albedo_d, albedo, sizeof(double)*sw_gas->grid.n, s));
        GRT_TRY(grt_dev_upload(p->device, p->solar_d, solar_flux, sizeof(double)*sw_gas->grid.n, s));
    }
    GRT_TRY(grt_dev_sync(p->device, s));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_create(GrtPipeline_t **pipeline, GasOptics_t *lw_gas, GasOptics_t *sw_gas,
                               int max_columns, int user_level, fp_t const *emissivity,
                               fp_t const *albedo, fp_t const *solar_flux)
{
    GRT_TRY(grt_pipeline_create_ex(pipeline, lw_gas, sw_gas, max_columns, user_level, emissivity, albedo, solar_flux, 0));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_create_ex(GrtPipeline_t **pipeline, GasOptics_t *lw_gas, GasOptics_t *sw_gas,
                                  int max_columns, int user_level, fp_t const *emissivity,
                                  fp_t const *albedo, fp_t const *solar_flux, int keep_spectra)
{
    GRT_REQUIRE_PTR(pipeline);
    GRT_REQUIRE_RANGE(max_columns, 1, 65535);
    GasOptics_t *any = lw_gas ? lw_gas : sw_gas;
    GRT_REQUIRE_PTR(any);
    if (lw_gas && sw_gas)
    {
        GRT_REQUIRE_EQ(lw_gas->device, sw_gas->device);
        GRT_REQUIRE_EQ(lw_gas->num_levels, sw_gas->num_levels);
    }
    GRT_REQUIRE_RANGE(user_level, -1, any->num_levels - 1);
    if (lw_gas != NULL)
    {
        GRT_REQUIRE_GRID_POINTS(&lw_gas->grid);
    }
    if (sw_gas != NULL)
    {
        GRT_REQUIRE_GRID_POINTS(&sw_gas->grid);
    }
    GrtPipeline_t *p = calloc(1, sizeof(*p));
    if (p == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for the pipeline object.%s", "");
    }
    p->device = any->device;
    p->lane = grt_dev_lane(any->device);
    p->max_cols = max_columns;
    p->num_levels = any->num_levels;
    p->user_level = user_level;
    p->keep_spectra = keep_spectra != 0;
    /* one way out: whatever a failing step leaves allocated (GBs of HBM per band) goes back through destroy */
    int const rc = pipeline_build(p, lw_gas, sw_gas, max_columns, emissivity, albedo, solar_flux);
    if (rc != GRTCODE_SUCCESS)
    {
        grt_err_frame(__FILE__, __LINE__);
        GrtPipeline_t *dead = p;
        grt_pipeline_release(&dead);
        return rc;
    }
    *pipeline = p;
    return GRTCODE_SUCCESS;
}

/* Frees everything a (possibly half-built) pipeline holds; never touches the error text of a failure in flight. */
static void grt_pipeline_release(GrtPipeline_t **pipeline)
{
    GrtPipeline_t *p = *pipeline;
    for (int b = 0; b < 2; ++b)
    {
        grt_dev_free(p->device, p->band[b].tau_gas);
        grt_dev_free(p->device, p->band[b].park);
        grt_dev_free(p->device, p->band[b].rows_d);
        grt_dev_free(p->device, p->band[b].level_partials);
        grt_dev_free(p->device, p->band[b].level_rows_d);
        grt_dev_free(p->device, p->band[b].cloud_map);
        grt_dev_free(p->device, p->band[b].cloud_block);
        free(p->band[b].cloud_key);
        grt_dev_free(p->device, p->band[b].bin_table);
        grt_dev_free(p->device, p->band[b].bin_partials);
        free(p->band[b].bin_edges);
        grt_dev_free(p->device, p->band[b].sub_partials);
        grt_dev_free(p->device, p->band[b].flux_sum);
        grt_dev_free(p->device, p->band[b].aer_map);
        grt_dev_free(p->device, p->band[b].aer_block);
        free(p->band[b].aer_key);
    }
    grt_dev_free(p->device, p->aer_d);
    grt_host_free_pinned(p->aer_h);
    grt_dev_event_destroy(p->device, &p->aer_uploaded);
    grt_dev_free(p->device, p->cloud_d);
    grt_host_free_pinned(p->cloud_h);
    grt_dev_event_destroy(p->device, &p->cloud_uploaded);
    grt_dev_free(p->device, p->small_d);
    grt_host_free_pinned(p->small_h);
    grt_dev_event_destroy(p->device, &p->small_uploaded);
    grt_dev_free(p->device, p->emis_d);
    grt_dev_free(p->device, p->albedo_d);
    grt_dev_free(p->device, p->solar_d);
    free(p);
    *pipeline = NULL;
}

EXTERN int grt_pipeline_destroy(GrtPipeline_t **pipeline)
{
    GRT_REQUIRE_PTR(pipeline);
    if (*pipeline == NULL)
    {
        return GRTCODE_SUCCESS;
    }
    GRT_TRY(grt_dev_sync((*pipeline)->device, grt_dev_stream((*pipeline)->device)));
    grt_pipeline_release(pipeline);
    return GRTCODE_SUCCESS;
}

EXTERN void *grt_pipeline_stream(GrtPipeline_t *pipeline)
{
    return pipeline ? grt_dev_stream_of_lane(pipeline->device, pipeline->lane) : NULL;
}

EXTERN int grt_pipeline_sync(GrtPipeline_t *pipeline)
{
    GRT_REQUIRE_PTR(pipeline);
    GRT_TRY(grt_dev_sync(pipeline->device, grt_dev_stream(pipeline->device)));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_views(GrtPipeline_t *pipeline, int band, fp_t **tau_gas, fp_t **tau,
                              fp_t **omega, fp_t **g, fp_t **flux_up, fp_t **flux_down)
{
    GRT_REQUIRE_PTR(pipeline);
    GRT_REQUIRE_RANGE(band, 0, 1);
    GrtBand *b = &pipeline->band[band];
    if (!pipeline->keep_spectra && (tau || omega || g || flux_up || flux_down))
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "this pipeline keeps no spectra (only tau_gas): create it with "
                 "grt_pipeline_create_ex(..., keep_spectra = 1).%s", "");
    }
    if (tau_gas != NULL && b->tau_gas_lacks_tables)
    {
        /* the last run's solver added the tables' part of tau itself: complete the array for the caller who looks at it */
        GrtContinua c;
        grt_gas_optics_continua(b->gas, &c);
        GRT_TRY(grt_dev_check(grt_launch_add_continua(grt_dev_stream_of_lane(pipeline->device, pipeline->lane), &c, b->gas->num_layers, b->last_cols,
                                                      b->n, b->tau_gas, (uint64_t)b->gas->num_layers*b->n), "continua kernel"));
        b->tau_gas_lacks_tables = 0;
    }
    if (tau_gas) *tau_gas = b->tau_gas;
    if (tau) *tau = b->tau;
    if (omega) *omega = b->omega;
    if (g) *g = b->g;
    if (flux_up) *flux_up = b->flux_up;
    if (flux_down) *flux_down = b->flux_down;
    return GRTCODE_SUCCESS;
}

/* What grt_pipeline_run and grt_pipeline_run_profiles check and stage alike: the arguments, the lane, and the small
   per-column inputs, uploaded to small_d on the library stream. */
static int stage_columns(GrtPipeline_t *p, GrtColumns_t const *cols)
{
    GRT_REQUIRE_RANGE(cols->ncol, 1, p->max_cols);
    GRT_REQUIRE_EQ(cols->num_levels, p->num_levels);
    GRT_REQUIRE_PTR(cols->pressure);
    GRT_REQUIRE_PTR(cols->temperature);
    int const V = p->num_levels, L = V - 1, C = cols->ncol;
    /* A pipeline belongs to the lane (HIP stream) that was selected when it was created: grt_pipeline_stream() hands THAT
       stream to the caller (who orders a gather behind it), while the kernels below go to the lane selected now.  The two
       must be the same: select the pipeline's lane before running it. */
    if (grt_dev_lane(p->device) != p->lane)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "this pipeline was created on lane %d, lane %d is selected: call grt_device_use_lane "
                 "before grt_pipeline_run.", p->lane, grt_dev_lane(p->device));
    }
    void *s = grt_dev_stream(p->device);
    /* the pinned staging buffer is reused every call: wait until the previous batch's copy of it has
       left -- not for its kernels, so that this batch is prepared on the host while that one runs */
    GRT_TRY(grt_dev_event_wait(p->device, p->small_uploaded));

    /* small per-column inputs: air column amounts for Rayleigh (rayleigh.c:104-128 via
       curtis_godson.c:25-40), temperatures, sun geometry */
    fp_t const mbtoatm = 0.000986923f;
    fp_t const c_air = 2.147822334314468e+25;
    for (int c = 0; c < C; ++c)
    {
        fp_t const *pm = cols->pressure + (size_t)c*V;
        for (int i = 0; i < L; ++i)
        {
            fp_t dp = pm[i]*mbtoatm - pm[i + 1]*mbtoatm;
            dp = dp >= 0.f ? dp : -1.f*dp;
            p->small_h[p->off_n + (size_t)c*L + i] = c_air*dp;
        }
    }
    memcpy(p->small_h + p->off_p, cols->pressure, sizeof(double)*(size_t)C*V);
    if (p->band[0].gas != NULL)
    {
        GRT_REQUIRE_PTR(cols->layer_temperature);
        GRT_REQUIRE_PTR(cols->surface_temperature);
        for (int c = 0; c < C; ++c)
        {
            GRT_REQUIRE_RANGE(cols->surface_temperature[c], MIN_TEMPERATURE, MAX_TEMPERATURE);
            for (int i = 0; i < L; ++i)
            {
                GRT_REQUIRE_RANGE(cols->layer_temperature[(size_t)c*L + i], MIN_TEMPERATURE, MAX_TEMPERATURE);
            }
        }
        memcpy(p->small_h + p->off_tl, cols->layer_temperature, sizeof(double)*(size_t)C*L);
        memcpy(p->small_h + p->off_tv, cols->temperature, sizeof(double)*(size_t)C*V);
        memcpy(p->small_h + p->off_ts, cols->surface_temperature, sizeof(double)*(size_t)C);
    }
    if (p->band[1].gas != NULL)
    {
        GRT_REQUIRE_PTR(cols->cos_zenith);
        GRT_REQUIRE_PTR(cols->total_solar_irradiance);
        for (int c = 0; c < C; ++c)
        {
            if (!(cols->cos_zenith[c] > 0. && cols->cos_zenith[c] <= 1.))
            {
                GRT_FAIL(GRTCODE_RANGE_ERR, "cosine of zenith angle (%e) of column %d outside (0, 1]"
                         " (night columns are skipped by the caller: driver.c:706).", cols->cos_zenith[c], c);
            }
        }
        memcpy(p->small_h + p->off_mu, cols->cos_zenith, sizeof(double)*(size_t)C);
        memcpy(p->small_h + p->off_tsi, cols->total_solar_irradiance, sizeof(double)*(size_t)C);
    }
    GRT_TRY(grt_dev_upload(p->device, p->small_d, p->small_h, sizeof(double)*p->small_doubles, s));
    GRT_TRY(grt_dev_event_record(p->device, &p->small_uploaded, s));
    return GRTCODE_SUCCESS;
}

/* gas optics of one band for the batch (launch.c:40-226).  Fused form: the spectral tables' part of tau (continua, CFC,
   CIA) is left to the solver kernel, which reads a table entry once per grid point and column instead of once per layer
   as well (the same expressions in the same order: the same doubles; GRT_DEFER_CONTINUA=0 in the environment: comparison
   runs).  *defer: the solver adds that part, from *continua. */
static int band_gas_optics(GrtPipeline_t *p, GrtBand *b, int bi, GrtColumns_t const *cols, GrtContinua *continua,
                           int *defer)
{
    *defer = 0;
    if (!p->keep_spectra && bi == 1)
    {
        /* (shortwave band only.  Measured per 64 columns of the 1 cm-1 grids: the shortwave gather 3.93 -> 3.01 ms, its
           solver 3.09 -> 3.60; the longwave band, whose solver is the lighter kernel, 0.26 + 0.36 -> 0.21 + 0.48) */
        char const *env = getenv("GRT_DEFER_CONTINUA");
        *defer = grt_gas_optics_defer_tables(b->gas, !(env != NULL && env[0] == '0'));
    }
    int const rc_gas = grt_optical_depth_batch(b->gas, cols, b->tau_gas);
    grt_gas_optics_defer_tables(b->gas, 0);                  /* (the object's own entry points deliver the whole tau) */
    GRT_TRY(rc_gas);
    grt_gas_optics_continua(b->gas, continua);               /* (the column state's place is known after the batch call) */
    b->tau_gas_lacks_tables = *defer;
    b->last_cols = cols->ncol;
    return GRTCODE_SUCCESS;
}

/* The solvers' arguments.  Fused forms: Rayleigh, add_optics({gas, rayleigh}) and the solver in one launch (driver.c:268,
   382-424) on tau_gas; spectral form: the materialised tau, omega (, g) in, [level][wavenumber] fluxes out.  The caller
   sets the partial sums and, shortwave, the park block. */
static void lw_args(GrtPipeline_t const *p, GrtBand const *b, int C, int fused, int defer, GrtContinua const *continua,
                    GrtLwArgs *a)
{
    SpectralGrid_t const *grid = &b->gas->grid;
    int const V = p->num_levels, L = V - 1;
    memset(a, 0, sizeof(*a));
    a->num_levels = V; a->ncol = C; a->w0 = grid->w0; a->dw = grid->dw; a->nw = b->n;
    a->optics_stride = (uint64_t)L*b->n;
    a->t_layers = p->small_d + p->off_tl; a->t_levels = p->small_d + p->off_tv;
    a->t_surf = p->small_d + p->off_ts;
    a->emis = p->emis_d; a->emis_stride = 0;
    a->user_level = p->user_level;
    if (fused)
    {
        a->tau_gas = b->tau_gas; a->n_layer = p->small_d + p->off_n;
        a->add_continua = defer;
        if (defer) a->continua = *continua;
    }
    else
    {
        a->tau = b->tau; a->omega = b->omega;
        a->flux_up = b->flux_up; a->flux_down = b->flux_down; a->flux_stride = (uint64_t)V*b->n;
    }
}

static void sw_args(GrtPipeline_t const *p, GrtBand const *b, int C, int fused, int defer, GrtContinua const *continua,
                    GrtSwArgs *a)
{
    SpectralGrid_t const *grid = &b->gas->grid;
    int const V = p->num_levels, L = V - 1;
    memset(a, 0, sizeof(*a));
    a->num_levels = V; a->ncol = C; a->nw = b->n; a->dw = grid->dw; a->w0 = grid->w0;
    a->optics_stride = (uint64_t)L*b->n;
    a->mu_dir = p->small_d + p->off_mu; a->mu_dif = 0.5;        /* driver.c:110 */
    a->alb_dir = p->albedo_d; a->alb_dif = p->albedo_d; a->alb_stride = 0;   /* driver.c:118-119 */
    a->tsi = p->small_d + p->off_tsi; a->solar = p->solar_d;
    a->user_level = p->user_level;
    if (fused)
    {
        a->tau_gas = b->tau_gas; a->n_layer = p->small_d + p->off_n;
        a->add_continua = defer;
        if (defer) a->continua = *continua;
        /* (read at every step, so that a test can compare the two forms in one process) */
        char const *env = getenv("GRT_SW_TWO_SWEEPS");
        a->one_sweep = !(env != NULL && env[0] == '1');
    }
    else
    {
        a->tau = b->tau; a->omega = b->omega; a->g = b->g;
        a->flux_up = b->flux_up; a->flux_down = b->flux_down; a->flux_stride = (uint64_t)V*b->n;
    }
}

/* the shortwave solver's two-sweep form: reflectances of 2 V levels and five properties of L layers per column and
   wavenumber, allocated at the first launch that needs them */
static int park_block(GrtPipeline_t *p, GrtBand *b)
{
    if (b->park == NULL)
    {
        size_t const V = (size_t)p->num_levels;
        void *pk = NULL;
        GRT_TRY(grt_dev_alloc(p->device, &pk, sizeof(double)*(size_t)p->max_cols*(2*V + 5*(V - 1))*b->n));
        b->park = pk;
    }
    return GRTCODE_SUCCESS;
}

/* grt_pipeline_run_spectral's outputs of one pass: the spectral rows and bins of set `set` of `sets` */
typedef struct SpectralOut
{
    double *spectral, *binned;
    int sets, set;
    int const *edges[2];
    int num_bins[2];
} SpectralOut;

/* where band bi's six spectral rows (or bins, per = bins) of column 0 start in a [ncol][sets][6 per_lw + 6 per_sw]
   block, and the doubles from one column to the next */
static size_t spectral_offset(SpectralOut const *so, int bi, size_t per_lw, size_t per_sw, size_t *col_stride)
{
    size_t const set_doubles = 6*(per_lw + per_sw);
    *col_stride = (size_t)so->sets*set_doubles;
    return (size_t)so->set*set_doubles + (bi == 1 ? 6*per_lw : 0);
}

static size_t band_points(GrtPipeline_t const *p, int bi)
{
    return p->band[bi].gas != NULL ? p->band[bi].n : 0;
}

/* the band's solver in `form` (GRT_SOLVER_CHAINS: the spectral form), timed under profile tag 3/4, or 8/9 with clouds, or
   12/13 in the aerosol pass (aer: the aerosol forms' tables; tagged: the materialised aerosol pass);
   the profile forms share the band's park block with the two-sweep six-row forms (the passes run in stream order); the
   spectral six-row forms store their rows where so places the band's */
static int band_solver(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtSolverForm form, int defer,
                       GrtContinua const *continua, GrtCloudArgs const *clouds, GrtAerosolArgs const *aer, int aer_pass,
                       double *partials, SpectralOut const *so)
{
    GrtFormKind const k = grt_form_kind(form);
    void *s = grt_dev_stream(p->device);
    int slot, krc;
    if (bi == 0)
    {
        GrtLwArgs a;
        lw_args(p, b, C, k.fused, defer, continua, &a);
        a.partials = partials;
        if (k.spectral)
        {
            size_t stride;
            a.flux_up = so->spectral + spectral_offset(so, bi, band_points(p, 0), band_points(p, 1), &stride);
            a.flux_down = a.flux_up + 3*b->n;
            a.flux_stride = stride;
        }
        slot = grt_profile_begin(s, aer_pass ? 12 : (clouds ? 8 : 3));
        krc = k.aerosol ? grt_launch_lw_aerosols(s, form, &a, aer) : grt_launch_lw(s, form, &a, clouds);
    }
    else
    {
        GrtSwArgs a;
        sw_args(p, b, C, k.fused, defer, continua, &a);
        a.partials = partials;
        if (k.spectral)
        {
            size_t stride;
            a.flux_up = so->spectral + spectral_offset(so, bi, band_points(p, 0), band_points(p, 1), &stride);
            a.flux_down = a.flux_up + 3*b->n;
            a.flux_stride = stride;
        }
        if (k.profile || (k.fused && !grt_sw_one_sweep(&a)))
        {
            GRT_TRY(park_block(p, b));
        }
        a.park = b->park;
        slot = grt_profile_begin(s, aer_pass ? 13 : (clouds ? 9 : 4));
        krc = k.aerosol ? grt_launch_sw_aerosols(s, form, &a, aer) : grt_launch_sw(s, form, &a, clouds);
    }
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, bi == 0 ? "longwave kernel" : "shortwave kernel"));
    return GRTCODE_SUCCESS;
}

/* Materialised form: Rayleigh + add_optics({gas, rayleigh}) (driver.c:268, 382-383) into the band's tau, omega, g */
static int band_clear_sky_optics(GrtPipeline_t *p, GrtBand *b, int C)
{
    SpectralGrid_t const *grid = &b->gas->grid;
    void *s = grt_dev_stream(p->device);
    int const slot = grt_profile_begin(s, 5);
    int const krc = grt_launch_clear_sky_optics(s, p->num_levels - 1, C, grid->w0, grid->dw, b->n, p->small_d + p->off_n,
                                                b->tau_gas, b->tau, b->omega, b->g);
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "clear-sky optics kernel"));
    return GRTCODE_SUCCESS;
}

/* materialised form: the row table of every level's up and down flux, [max_cols][2 V] */
static int level_rows(GrtPipeline_t *p, GrtBand *b)
{
    if (b->level_rows_d != NULL)
    {
        return GRTCODE_SUCCESS;
    }
    size_t const V = (size_t)p->num_levels, C = (size_t)p->max_cols;
    double **rows_h = malloc(sizeof(double *)*C*2*V);
    if (rows_h == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for the level row table of %zu columns.", C);
    }
    for (size_t c = 0; c < C; ++c)
    {
        for (size_t k = 0; k < V; ++k)
        {
            rows_h[(c*2 + 0)*V + k] = b->flux_up + (c*V + k)*b->n;
            rows_h[(c*2 + 1)*V + k] = b->flux_down + (c*V + k)*b->n;
        }
    }
    GRT_TRY(upload_rows(p, rows_h, C*2*V, &b->level_rows_d));
    return GRTCODE_SUCCESS;
}

/* ---- all-sky inputs (grt_pipeline_run_allsky) ---------------------------------------------------------------------- */

/* first index in [0, n) whose value is >= target (n if none), last index whose value is <= target (-1 if none) */
static int first_not_below(double const *w, int n, double target)
{
    int lo = 0, hi = n;
    while (lo < hi)
    {
        int const mid = (lo + hi)/2;
        if (w[mid] < target) lo = mid + 1; else hi = mid;
    }
    return lo;
}

static int last_not_above(double const *w, int n, double target)
{
    int lo = 0, hi = n;
    while (lo < hi)
    {
        int const mid = (lo + hi)/2;
        if (w[mid] <= target) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

/* The band each point of w [n] ends up with when bands 0 .. nb - 1 of a parametrisation of `own` bands are written in
   order, as optics_utils.c:118-169 writes them: [first >= lo, last <= hi), band 0 extended down, band own - 1 up. */
static void cloud_band_map(double const *lo, double const *hi, int own, int nb, double const *w, int n, int *idx)
{
    for (int j = 0; j < n; ++j)
    {
        idx[j] = -1;
    }
    for (int b = 0; b < nb; ++b)
    {
        int const from = first_not_below(w, n, lo[b]);
        int const upto = last_not_above(w, n, hi[b]);
        if (b == 0)
        {
            for (int j = 0; j < from; ++j) idx[j] = 0;
        }
        for (int j = from; j < upto; ++j) idx[j] = b;
        if (b == own - 1)
        {
            for (int j = upto < 0 ? 0 : upto; j < n; ++j) idx[j] = b;
        }
    }
}

/* the band's cloud arguments for a batch of C columns of S subcolumns staged by stage_clouds: its per-point cloud bands
   for these band limits are built on the host when the limits differ from the last call's */
static int band_clouds(GrtPipeline_t *p, GrtBand *b, int bi, GrtClouds_t const *cl, int C, int S, GrtCloudArgs *ca)
{
    int const B = cl->num_liquid_bands, NI = cl->num_ice_bands;
    size_t const L = (size_t)p->num_levels - 1, set = (size_t)S*(size_t)C*3*(size_t)B*L;
    ca->num_bands = B;
    ca->thickness = p->cloud_d;
    ca->liquid = p->cloud_d + (size_t)C*L + (size_t)(2*bi)*set;
    ca->ice = ca->liquid + set;
    size_t const nkey = 2 + 2*(size_t)B + 2*(size_t)NI;
    double *key = malloc(sizeof(double)*nkey);
    if (key == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for %zu band limits.", nkey);
    }
    key[0] = B; key[1] = NI;
    memcpy(key + 2, cl->liquid_band_lo, sizeof(double)*B);
    memcpy(key + 2 + B, cl->liquid_band_hi, sizeof(double)*B);
    memcpy(key + 2 + 2*B, cl->ice_band_lo, sizeof(double)*NI);
    memcpy(key + 2 + 2*B + NI, cl->ice_band_hi, sizeof(double)*NI);
    if (b->cloud_map != NULL && b->cloud_key_n == nkey && memcmp(b->cloud_key, key, sizeof(double)*nkey) == 0)
    {
        free(key);
        ca->band_liquid = b->cloud_map;
        ca->band_ice = b->cloud_map + b->n;
        return GRTCODE_SUCCESS;
    }
    int const n = (int)b->n;
    double *w = malloc(sizeof(double)*(size_t)n);
    int *idx = malloc(sizeof(int)*2*(size_t)n);
    int rc = (w == NULL || idx == NULL) ? GRTCODE_NULL_ERR : GRTCODE_SUCCESS;
    if (rc == GRTCODE_SUCCESS)
    {
        /* what driver.c:476-488 passes to cloud_optics as the grid's "wavenumbers": band limits, not centres */
        SpectralGrid_t const *grid = &b->gas->grid;
        for (uint64_t j = 1; j < b->n; ++j)
        {
            w[j] = 0.5*((grid->w0 + (j - 1)*grid->dw) + (grid->w0 + j*grid->dw));
        }
        w[0] = grid->w0 - grid->dw;
        if (w[0] < 0.)
        {
            w[0] = 0;
        }
        cloud_band_map(cl->liquid_band_lo, cl->liquid_band_hi, B, B, w, n, idx);
        cloud_band_map(cl->ice_band_lo, cl->ice_band_hi, NI, B, w, n, idx + n);
        void *s = grt_dev_stream(p->device);
        if (b->cloud_map == NULL)
        {
            void *m = NULL;
            rc = grt_dev_alloc(p->device, &m, sizeof(int)*2*(size_t)n);
            b->cloud_map = m;
        }
        /* (the last batch's kernels may still read the old map; then idx is freed: wait both times) */
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(p->device, s);
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_upload(p->device, b->cloud_map, idx, sizeof(int)*2*(size_t)n, s);
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(p->device, s);
    }
    free(w);
    free(idx);
    if (rc != GRTCODE_SUCCESS)
    {
        free(key);
        GRT_TRY(rc);
    }
    free(b->cloud_key);
    b->cloud_key = key;
    b->cloud_key_n = nkey;
    ca->band_liquid = b->cloud_map;
    ca->band_ice = b->cloud_map + b->n;
    return GRTCODE_SUCCESS;
}

/* the band tables of the batch to the device: [C][L] thickness, then the four sets, each [S][C][3][B][L] -- the caller's
   [C][S][3][B][L] subcolumn-major, so that subcolumn s of every column is one [C][3][B][L] block (S = 1: as given) */
static int stage_clouds(GrtPipeline_t *p, GrtClouds_t const *cl, int C, int S)
{
    size_t const L = (size_t)p->num_levels - 1, B = (size_t)cl->num_liquid_bands, tab = 3*B*L;
    size_t const set = (size_t)S*(size_t)C*tab, need = (size_t)C*L + 4*set;
    GRT_TRY(grt_dev_event_wait(p->device, p->cloud_uploaded));
    if (need > p->cloud_doubles)
    {
        /* (sized for max_columns at this band and subcolumn count: a later batch of the same shape reuses it) */
        size_t const want = (size_t)p->max_cols*L*(1 + 12*B*(size_t)S);
        void *s = grt_dev_stream(p->device);
        GRT_TRY(grt_dev_sync(p->device, s));
        grt_dev_free(p->device, p->cloud_d);
        grt_host_free_pinned(p->cloud_h);
        p->cloud_d = NULL;
        p->cloud_h = NULL;
        p->cloud_doubles = 0;
        GRT_TRY(grt_host_alloc_pinned((void **)&p->cloud_h, sizeof(double)*want));
        GRT_TRY(grt_dev_alloc(p->device, (void **)&p->cloud_d, sizeof(double)*want));
        p->cloud_doubles = want;
    }
    double *h = p->cloud_h;
    memcpy(h, cl->thickness, sizeof(double)*(size_t)C*L);
    h += (size_t)C*L;
    fp_t const *sets[4] = {cl->lw_liquid, cl->lw_ice, cl->sw_liquid, cl->sw_ice};
    for (int k = 0; k < 4; ++k)
    {
        if (sets[k] != NULL)
        {
            for (size_t s = 0; s < (size_t)S; ++s)
            {
                for (size_t c = 0; c < (size_t)C; ++c)
                {
                    memcpy(h + k*set + (s*(size_t)C + c)*tab, sets[k] + (c*(size_t)S + s)*tab, sizeof(double)*tab);
                }
            }
        }
        else
        {
            memset(h + k*set, 0, sizeof(double)*set);
        }
    }
    void *s = grt_dev_stream(p->device);
    GRT_TRY(grt_dev_upload(p->device, p->cloud_d, p->cloud_h, sizeof(double)*need, s));
    GRT_TRY(grt_dev_event_record(p->device, &p->cloud_uploaded, s));
    return GRTCODE_SUCCESS;
}

/* Materialised form: the cloud objects spread onto the grid, Rayleigh, add_optics of the four objects per column
   (driver.c:507-530) -- tau, omega, g of the band are the all-sky pass's */
static int band_allsky_optics(GrtPipeline_t *p, GrtBand *b, int C, GrtCloudArgs const *ca)
{
    SpectralGrid_t const *grid = &b->gas->grid;
    int const L = p->num_levels - 1;
    uint64_t const per = (uint64_t)L*b->n, all = per*(uint64_t)p->max_cols;
    void *s = grt_dev_stream(p->device);
    if (b->cloud_block == NULL)
    {
        void *blk = NULL;
        GRT_TRY(grt_dev_alloc(p->device, &blk, sizeof(double)*(6*all + 4*per)));
        b->cloud_block = blk;
        GRT_TRY(grt_dev_zero(p->device, b->cloud_block + 6*all + 3*per, sizeof(double)*per, s));
    }
    double *cloud[6];
    for (int k = 0; k < 6; ++k)
    {
        cloud[k] = b->cloud_block + k*all;
    }
    double *ray = b->cloud_block + 6*all, *zero = ray + 3*per;
    GRT_TRY(grt_dev_check(grt_launch_spread_clouds(s, L, C, b->n, ca, cloud[0], cloud[1], cloud[2], cloud[3], cloud[4],
                                                   cloud[5]), "cloud spreading kernel"));
    for (int c = 0; c < C; ++c)
    {
        /* Rayleigh of this column (rayleigh.c:29-68: its number densities travel as a kernel argument) */
        GRT_TRY(grt_dev_check(grt_launch_rayleigh(s, L, grid->w0, grid->dw, b->n, p->small_h + p->off_n + (size_t)c*L,
                                                  ray, ray + per, ray + 2*per), "Rayleigh kernel"));
        GrtOpticsPtrs in;
        memset(&in, 0, sizeof(in));
        uint64_t const o = (uint64_t)c*per;
        in.tau[0] = b->tau_gas + o; in.omega[0] = zero; in.g[0] = zero;
        in.tau[1] = ray; in.omega[1] = ray + per; in.g[1] = ray + 2*per;
        in.tau[2] = cloud[0] + o; in.omega[2] = cloud[1] + o; in.g[2] = cloud[2] + o;
        in.tau[3] = cloud[3] + o; in.omega[3] = cloud[4] + o; in.g[3] = cloud[5] + o;
        GRT_TRY(grt_dev_check(grt_launch_add_optics(s, per, 4, &in, b->tau + o, b->omega + o, b->g + o),
                              "add_optics kernel (all-sky)"));
    }
    return GRTCODE_SUCCESS;
}

/* ---- aerosol inputs (grt_pipeline_run_aerosols) ---------------------------------------------------------------------- */

static int aerosol_points(GrtAerosols_t const *ae, int bi)
{
    return bi == 0 ? ae->lw_num_points : ae->sw_num_points;
}

/* The interval of the aerosol grid x [na] (strictly increasing) each of the n points w0 + i dw lies in, as
   interpolate2 (utilities.c:149-222) assigns them: j with x[j] < w <= x[j+1]; -1 for w <= x[0] and for w > x[na-1],
   which the reference does not write. */
void grt_aerosol_interval_map(double w0, double dw, uint64_t n, double const *x, int na, int *interval)
{
    for (uint64_t i = 0; i < n; ++i)
    {
        double const w = w0 + i*dw;
        interval[i] = (w <= x[0] || w > x[na - 1]) ? -1 : first_not_below(x, na, w) - 1;
    }
}

/* linear_sample's (utilities.c:235-246) slope and intercept of every interval, layer and property of ncol columns:
   optics [ncol][3][L][na] -> tables [ncol][3][na - 1][2][L] (GrtAerosolArgs) */
void grt_aerosol_tables(double const *x, int na, int ncol, int num_layers, double const *optics, double *tables)
{
    size_t const L = (size_t)num_layers, NA = (size_t)na, NI = NA - 1;
    for (size_t cp = 0; cp < (size_t)ncol*3; ++cp)
    {
        for (size_t l = 0; l < L; ++l)
        {
            double const *y = optics + (cp*L + l)*NA;
            for (size_t j = 0; j < NI; ++j)
            {
                double const m = (y[j + 1] - y[j])/(x[j + 1] - x[j]);
                double const b = y[j] - m*x[j];
                tables[((cp*NI + j)*2 + 0)*L + l] = m;
                tables[((cp*NI + j)*2 + 1)*L + l] = b;
            }
        }
    }
}

/* the batch's slope and intercept tables to the device: the longwave's [C][3][NA - 1][2][L], then the shortwave's (a band
   the pipeline does not have, or one given no aerosol, takes no room) */
static int stage_aerosols(GrtPipeline_t *p, GrtAerosols_t const *ae, int C)
{
    size_t const L = (size_t)p->num_levels - 1;
    size_t per[2], need = 0, want = 0;
    for (int bi = 0; bi < 2; ++bi)
    {
        int const na = p->band[bi].gas != NULL ? aerosol_points(ae, bi) : 0;
        per[bi] = na > 0 ? 6*L*((size_t)na - 1) : 0;
        need += (size_t)C*per[bi];
        want += (size_t)p->max_cols*per[bi];
    }
    if (need == 0)
    {
        return GRTCODE_SUCCESS;
    }
    GRT_TRY(grt_dev_event_wait(p->device, p->aer_uploaded));
    void *s = grt_dev_stream(p->device);
    if (need > p->aer_doubles)
    {
        /* (sized for max_columns at these grids: a later batch of the same shape reuses it) */
        GRT_TRY(grt_dev_sync(p->device, s));
        grt_dev_free(p->device, p->aer_d);
        grt_host_free_pinned(p->aer_h);
        p->aer_d = NULL;
        p->aer_h = NULL;
        p->aer_doubles = 0;
        GRT_TRY(grt_host_alloc_pinned((void **)&p->aer_h, sizeof(double)*want));
        GRT_TRY(grt_dev_alloc(p->device, (void **)&p->aer_d, sizeof(double)*want));
        p->aer_doubles = want;
    }
    if (per[0] > 0)
    {
        grt_aerosol_tables(ae->lw_grid, ae->lw_num_points, C, (int)L, ae->lw_optics, p->aer_h);
    }
    if (per[1] > 0)
    {
        grt_aerosol_tables(ae->sw_grid, ae->sw_num_points, C, (int)L, ae->sw_optics, p->aer_h + (size_t)C*per[0]);
    }
    GRT_TRY(grt_dev_upload(p->device, p->aer_d, p->aer_h, sizeof(double)*need, s));
    GRT_TRY(grt_dev_event_record(p->device, &p->aer_uploaded, s));
    return GRTCODE_SUCCESS;
}

/* the band's aerosol arguments for a batch of C columns staged by stage_aerosols: its per-point intervals are built on the
   host when the band's aerosol grid differs from the last call's */
static int band_aerosols(GrtPipeline_t *p, GrtBand *b, int bi, GrtAerosols_t const *ae, int C, GrtAerosolArgs *aa)
{
    int const na = aerosol_points(ae, bi);
    double const *x = bi == 0 ? ae->lw_grid : ae->sw_grid;
    size_t const L = (size_t)p->num_levels - 1;
    int const na_lw = p->band[0].gas != NULL ? ae->lw_num_points : 0;
    aa->num_intervals = na - 1;
    aa->tables = p->aer_d + (bi == 1 && na_lw > 0 ? (size_t)C*6*L*((size_t)na_lw - 1) : 0);
    if (b->aer_map != NULL && b->aer_key_n == na && memcmp(b->aer_key, x, sizeof(double)*(size_t)na) == 0)
    {
        aa->interval = b->aer_map;
        return GRTCODE_SUCCESS;
    }
    double *key = malloc(sizeof(double)*(size_t)na);
    int *idx = malloc(sizeof(int)*b->n);
    int rc = (key == NULL || idx == NULL) ? GRTCODE_NULL_ERR : GRTCODE_SUCCESS;
    if (rc == GRTCODE_SUCCESS)
    {
        memcpy(key, x, sizeof(double)*(size_t)na);
        grt_aerosol_interval_map(b->gas->grid.w0, b->gas->grid.dw, b->n, x, na, idx);
        void *s = grt_dev_stream(p->device);
        if (b->aer_map == NULL)
        {
            void *m = NULL;
            rc = grt_dev_alloc(p->device, &m, sizeof(int)*b->n);
            b->aer_map = m;
        }
        /* (the last batch's kernels may still read the old map; then idx is freed: wait both times) */
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(p->device, s);
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_upload(p->device, b->aer_map, idx, sizeof(int)*b->n, s);
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(p->device, s);
    }
    free(idx);
    if (rc != GRTCODE_SUCCESS)
    {
        free(key);
        free(b->aer_key);               /* (the device map may be half written: it is rebuilt at the next call) */
        b->aer_key = NULL;
        b->aer_key_n = 0;
        GRT_TRY(rc);
    }
    free(b->aer_key);
    b->aer_key = key;
    b->aer_key_n = na;
    aa->interval = b->aer_map;
    return GRTCODE_SUCCESS;
}

/* Materialised form: the aerosol object spread onto the grid, Rayleigh, add_optics of the three objects per column
   (driver.c:426-434) -- tau, omega, g of the band are the aerosol pass's */
static int band_aerosol_optics(GrtPipeline_t *p, GrtBand *b, int C, GrtAerosolArgs const *aa)
{
    SpectralGrid_t const *grid = &b->gas->grid;
    int const L = p->num_levels - 1;
    uint64_t const per = (uint64_t)L*b->n, all = per*(uint64_t)p->max_cols;
    void *s = grt_dev_stream(p->device);
    if (b->aer_block == NULL)
    {
        void *blk = NULL;
        GRT_TRY(grt_dev_alloc(p->device, &blk, sizeof(double)*(3*all + 4*per)));
        b->aer_block = blk;
        GRT_TRY(grt_dev_zero(p->device, b->aer_block + 3*all + 3*per, sizeof(double)*per, s));
    }
    double *aer[3] = {b->aer_block, b->aer_block + all, b->aer_block + 2*all};
    double *ray = b->aer_block + 3*all, *zero = ray + 3*per;
    GRT_TRY(grt_dev_check(grt_launch_spread_aerosols(s, L, C, grid->w0, grid->dw, b->n, aa, aer[0], aer[1], aer[2]),
                          "aerosol spreading kernel"));
    for (int c = 0; c < C; ++c)
    {
        GRT_TRY(grt_dev_check(grt_launch_rayleigh(s, L, grid->w0, grid->dw, b->n, p->small_h + p->off_n + (size_t)c*L,
                                                  ray, ray + per, ray + 2*per), "Rayleigh kernel"));
        GrtOpticsPtrs in;
        memset(&in, 0, sizeof(in));
        uint64_t const o = (uint64_t)c*per;
        in.tau[0] = b->tau_gas + o; in.omega[0] = zero; in.g[0] = zero;
        in.tau[1] = ray; in.omega[1] = ray + per; in.g[1] = ray + 2*per;
        in.tau[2] = aer[0] + o; in.omega[2] = aer[1] + o; in.g[2] = aer[2] + o;
        GRT_TRY(grt_dev_check(grt_launch_add_optics(s, per, 3, &in, b->tau + o, b->omega + o, b->g + o),
                              "add_optics kernel (aerosols)"));
    }
    return GRTCODE_SUCCESS;
}

/* ---- spectral rows and bins (grt_pipeline_run_spectral) ------------------------------------------------------------ */

/* the band's bin table for these edges (built and uploaded when they differ from the last call's) and room for the partial
   sums of max_cols x 6 rows */
static int band_bins(GrtPipeline_t *p, GrtBand *b, int const *edges, int nbins)
{
    void *s = grt_dev_stream(p->device);
    if (b->bin_table == NULL || b->bin_count != nbins ||
        memcmp(b->bin_edges, edges, sizeof(int)*((size_t)nbins + 1)) != 0)
    {
        size_t const nt = grt_bin_table_ints(nbins, b->n);
        int *tab = malloc(sizeof(int)*nt);
        int *key = malloc(sizeof(int)*((size_t)nbins + 1));
        if (tab == NULL || key == NULL)
        {
            free(tab);
            free(key);
            GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for the table of %d bins.", nbins);
        }
        size_t const per_row = grt_bin_table(edges, nbins, b->n, tab);
        memcpy(key, edges, sizeof(int)*((size_t)nbins + 1));
        /* (the last batch's kernels may still read the old table; then tab is freed: wait both times) */
        int rc = grt_dev_sync(p->device, s);
        if (rc == GRTCODE_SUCCESS)
        {
            grt_dev_free(p->device, b->bin_table);
            b->bin_table = NULL;
            free(b->bin_edges);
            b->bin_edges = NULL;
            void *t = NULL;
            rc = grt_dev_alloc(p->device, &t, sizeof(int)*nt);
            b->bin_table = t;
        }
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_upload(p->device, b->bin_table, tab, sizeof(int)*nt, s);
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(p->device, s);
        free(tab);
        if (rc != GRTCODE_SUCCESS)
        {
            free(key);
            grt_dev_free(p->device, b->bin_table);
            b->bin_table = NULL;
            GRT_TRY(rc);
        }
        b->bin_edges = key;
        b->bin_count = nbins;
        b->bin_per_row = per_row;
    }
    if (b->bin_per_row > b->bin_cap)
    {
        GRT_TRY(grt_dev_sync(p->device, s));
        grt_dev_free(p->device, b->bin_partials);
        b->bin_partials = NULL;
        b->bin_cap = 0;
        void *pt = NULL;
        GRT_TRY(grt_dev_alloc(p->device, &pt, sizeof(double)*(size_t)p->max_cols*6*b->bin_per_row));
        b->bin_partials = pt;
        b->bin_cap = b->bin_per_row;
    }
    return GRTCODE_SUCCESS;
}

/* One solve of a band for grt_pipeline_run_spectral: the six rows at every point into the caller's spectral block, the
   -integrated six into out, and the bins.  Fused form: the spectral six-row solver (its rows stored where it weights
   them) and the fixed-order sum of its partial sums; materialised form: the spectral solver, its rows 0, L and the user
   level copied out, the row-wise trapezoid.  The bins are summed from the stored rows by the binning kernel (profile
   tag 10). */
static int band_solve_spectral(GrtPipeline_t *p, GrtBand *b, int bi, int C, int defer, GrtContinua const *continua,
                               GrtCloudArgs const *clouds, double *out, int out_stride, int out_offset,
                               SpectralOut const *so)
{
    void *s = grt_dev_stream(p->device);
    size_t stride;
    double *rows = so->spectral + spectral_offset(so, bi, band_points(p, 0), band_points(p, 1), &stride);
    if (!p->keep_spectra)
    {
        GRT_TRY(band_solver(p, b, bi, C, clouds ? GRT_SOLVER_ALLSKY_SPECTRAL : GRT_SOLVER_SPECTRAL, defer, continua,
                            clouds, NULL, 0, b->partials, so));
        GRT_TRY(grt_dev_check(grt_launch_reduce_partials(s, b->partials, C*GRT_FLUXES_PER_BAND, b->nblocks, out,
                                                         GRT_FLUXES_PER_BAND, out_stride, out_offset),
                              "flux reduction kernel"));
    }
    else
    {
        GRT_TRY(clouds ? band_allsky_optics(p, b, C, clouds) : band_clear_sky_optics(p, b, C));
        GRT_TRY(band_solver(p, b, bi, C, GRT_SOLVER_CHAINS, defer, continua, clouds, NULL, 0, NULL, NULL));
        GRT_TRY(grt_dev_check(grt_launch_copy_rows(s, (double const *const *)b->rows_d, C*GRT_FLUXES_PER_BAND, b->n,
                                                   rows, stride), "spectral row copy kernel"));
        GRT_TRY(grt_dev_check(grt_launch_integrate_rows(s, (double const *const *)b->rows_d, C*GRT_FLUXES_PER_BAND, b->n,
                                                        b->gas->grid.dw, out, GRT_FLUXES_PER_BAND, out_stride,
                                                        out_offset), "spectral integration kernel"));
    }
    int const nbins = so->num_bins[bi];
    if (nbins > 0)
    {
        GRT_TRY(band_bins(p, b, so->edges[bi], nbins));
        size_t bstride;
        double *binned = so->binned + spectral_offset(so, bi, (size_t)so->num_bins[0], (size_t)so->num_bins[1], &bstride);
        int const slot = grt_profile_begin(s, 10);
        int const krc = grt_launch_bin_rows(s, rows, stride, C*GRT_FLUXES_PER_BAND, b->n, b->gas->grid.dw, nbins,
                                            b->bin_table, b->bin_per_row, b->bin_partials, binned, bstride);
        grt_profile_end(s, slot);
        GRT_TRY(grt_dev_check(krc, "spectral binning kernel"));
    }
    return GRTCODE_SUCCESS;
}

/* ---- the run ------------------------------------------------------------------------------------------------------ */

/* One solve of a band on this run's tau_gas: Rayleigh, add_optics({gas, rayleigh}) -- or, with clouds, add_optics({gas,
   rayleigh, liquid, ice}) --, the solver and the -integrated output (driver.c:268, 382-424, 507-530, 302-326) of `rows`
   rows per column, the six of driver.c:272-280 or (profile) every level's up then down flux, to
   out[c*out_stride + out_offset + bi*rows + r].  Fused form: all of it in one solver launch, then the fixed-order sum of
   its per-block partial sums (profile: in level_partials, which the clear-sky and the all-sky pass of
   grt_pipeline_run_allsky_profiles take in turn); materialised form: tau, omega, g and the spectral fluxes in the band's
   arrays, then the row-wise trapezoid.  aer_pass: the aerosol pass of grt_pipeline_run_aerosols (profile tags 12 / 13) --
   add_optics({gas, rayleigh, aerosol}) from aer's tables, or, aer NULL (a band given no aerosol), the clear-sky solve
   again. */
static int band_solve(GrtPipeline_t *p, GrtBand *b, int bi, int C, int defer, GrtContinua const *continua,
                      GrtCloudArgs const *clouds, GrtAerosolArgs const *aer, int aer_pass, int profile, double *out,
                      int out_stride, int out_offset, SpectralOut const *so)
{
    int const V = p->num_levels, rows = profile ? 2*V : GRT_FLUXES_PER_BAND;
    out_offset += bi*rows;
    void *s = grt_dev_stream(p->device);
    if (so != NULL)
    {
        GRT_TRY(band_solve_spectral(p, b, bi, C, defer, continua, clouds, out, out_stride, out_offset, so));
        return GRTCODE_SUCCESS;
    }
    if (!p->keep_spectra)
    {
        if (profile && b->level_partials == NULL)
        {
            void *lp = NULL;
            GRT_TRY(grt_dev_alloc(p->device, &lp, sizeof(double)*(size_t)p->max_cols*2*(size_t)V*b->nblocks));
            b->level_partials = lp;
        }
        double *partials = profile ? b->level_partials : b->partials;
        GrtSolverForm const form = aer ? (profile ? GRT_SOLVER_AEROSOL_PROFILE : GRT_SOLVER_AEROSOL)
                                 : profile ? (clouds ? GRT_SOLVER_ALLSKY_PROFILE : GRT_SOLVER_PROFILE)
                                           : (clouds ? GRT_SOLVER_ALLSKY : GRT_SOLVER_FUSED);
        GRT_TRY(band_solver(p, b, bi, C, form, defer, continua, clouds, aer, aer_pass, partials, so));
        GRT_TRY(grt_dev_check(grt_launch_reduce_partials(s, partials, C*rows, b->nblocks, out, rows, out_stride, out_offset),
                              "flux reduction kernel"));
        return GRTCODE_SUCCESS;
    }
    GRT_TRY(aer ? band_aerosol_optics(p, b, C, aer) : clouds ? band_allsky_optics(p, b, C, clouds)
                                                             : band_clear_sky_optics(p, b, C));
    GRT_TRY(band_solver(p, b, bi, C, GRT_SOLVER_CHAINS, defer, continua, clouds, NULL, aer_pass, NULL, NULL));
    if (profile)
    {
        GRT_TRY(level_rows(p, b));
    }
    GRT_TRY(grt_dev_check(grt_launch_integrate_rows(s, (double const *const *)(profile ? b->level_rows_d : b->rows_d),
                                                    C*rows, b->n, b->gas->grid.dw, out, rows, out_stride, out_offset),
                          "spectral integration kernel"));
    return GRTCODE_SUCCESS;
}

/* The all-sky pass of grt_pipeline_run_subcolumns for one band, S subcolumns of every column on this run's tau_gas
   (driver.c:503-589), its mean rows to out as band_solve writes them.  ca: the band's tables staged subcolumn-major.
   Fused form: the subcolumn instance of the all-sky solver over C x S grid rows, each subcolumn's partial sums in
   sub_partials, then their fixed-order mean (profile tag 11; S = 1: the fixed-order sum of band_solve).  The shortwave's
   two-sweep forms park C x count columns at a time in the band's park block, count = what fits in its max_cols, in
   stream order.  Materialised form: per subcolumn the all-sky optics, the spectral solver and the sum of its fluxes;
   then the mean into the band's flux arrays, and the row-wise trapezoid. */
static int band_solve_subcolumns(GrtPipeline_t *p, GrtBand *b, int bi, int C, int S, int defer,
                                 GrtContinua const *continua, GrtCloudArgs const *ca, int profile, double *out,
                                 int out_stride, int out_offset)
{
    int const V = p->num_levels, rows = profile ? 2*V : GRT_FLUXES_PER_BAND;
    out_offset += bi*rows;
    void *s = grt_dev_stream(p->device);
    size_t const tab = (size_t)C*3*(size_t)ca->num_bands*(size_t)(V - 1);
    if (!p->keep_spectra)
    {
        size_t const need = (size_t)p->max_cols*(size_t)S*(size_t)rows*b->nblocks;
        if (need > b->sub_cap)
        {
            GRT_TRY(grt_dev_sync(p->device, s));
            grt_dev_free(p->device, b->sub_partials);
            b->sub_partials = NULL;
            b->sub_cap = 0;
            void *sp = NULL;
            GRT_TRY(grt_dev_alloc(p->device, &sp, sizeof(double)*need));
            b->sub_partials = sp;
            b->sub_cap = need;
        }
        GrtLwArgs lw;
        GrtSwArgs sw;
        int group = 65535/C;                   /* (grid rows) */
        if (bi == 0)
        {
            lw_args(p, b, C, 1, defer, continua, &lw);
            lw.partials = b->sub_partials;
        }
        else
        {
            sw_args(p, b, C, 1, defer, continua, &sw);
            sw.partials = b->sub_partials;
            if (profile || !grt_sw_one_sweep(&sw))
            {
                GRT_TRY(park_block(p, b));
                group = p->max_cols/C;
            }
            sw.park = b->park;
        }
        group = group < S ? group : S;
        int const slot = grt_profile_begin(s, bi == 0 ? 8 : 9);
        int krc = 0;
        for (int first = 0; first < S && krc == 0; first += group)
        {
            GrtSubcolumnArgs sc;
            sc.clouds = *ca;
            sc.subcolumns = S;
            sc.first = first;
            sc.count = S - first < group ? S - first : group;
            krc = bi == 0 ? grt_launch_lw_subcolumns(s, profile, &lw, &sc) : grt_launch_sw_subcolumns(s, profile, &sw, &sc);
        }
        grt_profile_end(s, slot);
        GRT_TRY(grt_dev_check(krc, bi == 0 ? "longwave subcolumn kernel" : "shortwave subcolumn kernel"));
        if (S == 1)
        {
            GRT_TRY(grt_dev_check(grt_launch_reduce_partials(s, b->sub_partials, C*rows, b->nblocks, out, rows, out_stride,
                                                             out_offset), "flux reduction kernel"));
            return GRTCODE_SUCCESS;
        }
        int const mslot = grt_profile_begin(s, 11);
        int const mrc = grt_launch_subcolumn_mean(s, b->sub_partials, C, S, rows, b->nblocks, out, out_stride, out_offset);
        grt_profile_end(s, mslot);
        GRT_TRY(grt_dev_check(mrc, "subcolumn mean kernel"));
        return GRTCODE_SUCCESS;
    }
    uint64_t const per = (uint64_t)C*(uint64_t)V*b->n, all = (uint64_t)p->max_cols*(uint64_t)V*b->n;
    if (b->flux_sum == NULL)
    {
        void *fs = NULL;
        GRT_TRY(grt_dev_alloc(p->device, &fs, sizeof(double)*2*all));
        b->flux_sum = fs;
    }
    for (int j = 0; j < S; ++j)
    {
        GrtCloudArgs cj = *ca;
        cj.liquid += (size_t)j*tab;
        cj.ice += (size_t)j*tab;
        GRT_TRY(band_allsky_optics(p, b, C, &cj));
        GRT_TRY(band_solver(p, b, bi, C, GRT_SOLVER_CHAINS, defer, continua, &cj, NULL, 0, NULL, NULL));
        GRT_TRY(grt_dev_check(grt_launch_flux_accumulate(s, per, b->flux_up, b->flux_sum, j == 0), "flux sum kernel"));
        GRT_TRY(grt_dev_check(grt_launch_flux_accumulate(s, per, b->flux_down, b->flux_sum + all, j == 0),
                              "flux sum kernel"));
    }
    GRT_TRY(grt_dev_check(grt_launch_flux_mean(s, per, b->flux_sum, S, b->flux_up), "flux mean kernel"));
    GRT_TRY(grt_dev_check(grt_launch_flux_mean(s, per, b->flux_sum + all, S, b->flux_down), "flux mean kernel"));
    if (profile)
    {
        GRT_TRY(level_rows(p, b));
    }
    GRT_TRY(grt_dev_check(grt_launch_integrate_rows(s, (double const *const *)(profile ? b->level_rows_d : b->rows_d),
                                                    C*rows, b->n, b->gas->grid.dw, out, rows, out_stride, out_offset),
                          "spectral integration kernel"));
    return GRTCODE_SUCCESS;
}

/* What the run entry points share after their argument checks: the batch (and its clouds) staged, then per band
   the gas optics and the solve into out (band_solve) -- with clouds, the clear-sky solve and then the all-sky one, whose
   rows follow the clear-sky set's GRT_FLUXES_PER_COLUMN or (profile) GRT_PROFILE_ROWS_PER_COLUMN V.  subcolumns > 0
   (grt_pipeline_run_subcolumns): the all-sky pass is the mean over that many subcolumns (band_solve_subcolumns). */
static int pipeline_run(GrtPipeline_t *p, GrtColumns_t const *cols, GrtClouds_t const *cl, GrtAerosols_t const *ae,
                        int subcolumns, int profile, double *out, int out_stride, SpectralOut *so)
{
    GRT_TRY(stage_columns(p, cols));
    int const C = cols->ncol, S = subcolumns > 0 ? subcolumns : 1;
    if (cl != NULL)
    {
        GRT_TRY(stage_clouds(p, cl, C, S));
    }
    if (ae != NULL)
    {
        GRT_TRY(stage_aerosols(p, ae, C));
    }
    for (int bi = 0; bi < 2; ++bi)
    {
        GrtBand *b = &p->band[bi];
        if (b->gas == NULL)
        {
            if (!profile)
            {
                /* a skipped band's six values (and its all-sky six) are zeros, as the profile forms' rows are: the
                   caller's buffer is not left holding whatever it held before */
                void *s = grt_dev_stream(p->device);
                for (int c = 0; c < C; ++c)
                {
                    double *six = out + (size_t)c*out_stride + GRT_FLUXES_PER_BAND*bi;
                    GRT_TRY(grt_dev_zero(p->device, six, sizeof(double)*GRT_FLUXES_PER_BAND, s));
                    if (cl != NULL || ae != NULL)
                    {
                        GRT_TRY(grt_dev_zero(p->device, six + GRT_FLUXES_PER_COLUMN, sizeof(double)*GRT_FLUXES_PER_BAND, s));
                    }
                }
            }
            continue;
        }
        GrtCloudArgs ca;
        if (cl != NULL)
        {
            GRT_TRY(band_clouds(p, b, bi, cl, C, S, &ca));
        }
        GrtContinua continua;
        int defer;
        GRT_TRY(band_gas_optics(p, b, bi, cols, &continua, &defer));
        if (so != NULL)
        {
            so->set = 0;
        }
        GRT_TRY(band_solve(p, b, bi, C, defer, &continua, NULL, NULL, 0, profile, out, out_stride, 0, so));
        if (ae != NULL)
        {
            /* the aerosol set follows the clear-clean one, as the all-sky set does */
            int const set = profile ? GRT_PROFILE_ROWS_PER_COLUMN*p->num_levels : GRT_FLUXES_PER_COLUMN;
            GrtAerosolArgs aa;
            int const has = aerosol_points(ae, bi) > 0;
            if (has)
            {
                GRT_TRY(band_aerosols(p, b, bi, ae, C, &aa));
            }
            GRT_TRY(band_solve(p, b, bi, C, defer, &continua, NULL, has ? &aa : NULL, 1, profile, out, out_stride, set,
                               NULL));
        }
        if (cl != NULL)
        {
            int const set = profile ? GRT_PROFILE_ROWS_PER_COLUMN*p->num_levels : GRT_FLUXES_PER_COLUMN;
            if (so != NULL)
            {
                so->set = 1;
            }
            if (subcolumns > 0)
            {
                GRT_TRY(band_solve_subcolumns(p, b, bi, C, S, defer, &continua, &ca, profile, out, out_stride, set));
                continue;
            }
            GRT_TRY(band_solve(p, b, bi, C, defer, &continua, &ca, NULL, 0, profile, out, out_stride, set, so));
        }
    }
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run(GrtPipeline_t *p, GrtColumns_t const *cols, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    GRT_REQUIRE_PTR(fluxes_dev);
    GRT_TRY(pipeline_run(p, cols, NULL, NULL, 0, 0, fluxes_dev, GRT_FLUXES_PER_COLUMN, NULL));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run_profiles(GrtPipeline_t *p, GrtColumns_t const *cols, fp_t *level_fluxes_dev,
                                     fp_t *heating_dev, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (level_fluxes_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "level_fluxes_dev is NULL: the level fluxes [ncol][%d][%d] are the output.",
                 GRT_PROFILE_ROWS_PER_COLUMN, p->num_levels);
    }
    if (cols->ncol < 1 || cols->ncol > p->max_cols)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d columns asked for, this pipeline was created for 1 to %d.", cols->ncol, p->max_cols);
    }
    if (p->num_levels < 2)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "heating rates need at least 2 levels (%d).", p->num_levels);
    }
    int const V = p->num_levels;
    /* [c][2 V] rows of band bi -> level_fluxes_dev[c][2 bi + {0, 1}][V], then the level fluxes' heating rates and six rows */
    GRT_TRY(pipeline_run(p, cols, NULL, NULL, 0, 1, level_fluxes_dev, GRT_PROFILE_ROWS_PER_COLUMN*V, NULL));
    int const bands = (p->band[0].gas != NULL) | (p->band[1].gas != NULL) << 1;
    GRT_TRY(grt_dev_check(grt_launch_profile_finish(grt_dev_stream(p->device), cols->ncol, 1, V, bands, p->user_level,
                                                    GRT_GRAVITY, GRT_SPECIFIC_HEAT_AIR, p->small_d + p->off_p,
                                                    level_fluxes_dev, heating_dev, fluxes_dev), "heating rate kernel"));
    return GRTCODE_SUCCESS;
}

/* grt_pipeline_run_allsky's and grt_pipeline_run_allsky_profiles' checks of the cloud inputs and the batch size */
static int check_clouds(GrtPipeline_t const *p, GrtColumns_t const *cols, GrtClouds_t const *cl)
{
    if (cl == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no cloud inputs (GrtClouds_t is NULL).%s", "");
    }
    if (cl->num_liquid_bands < 1 || cl->num_ice_bands < cl->num_liquid_bands)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d liquid and %d ice bands: at least one liquid band, and no fewer ice bands.",
                 cl->num_liquid_bands, cl->num_ice_bands);
    }
    if (cl->liquid_band_lo == NULL || cl->liquid_band_hi == NULL || cl->ice_band_lo == NULL || cl->ice_band_hi == NULL ||
        cl->thickness == NULL || (p->band[0].gas != NULL && (cl->lw_liquid == NULL || cl->lw_ice == NULL)) ||
        (p->band[1].gas != NULL && (cl->sw_liquid == NULL || cl->sw_ice == NULL)))
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "a NULL array in the cloud inputs.%s", "");
    }
    if (cols->ncol < 1 || cols->ncol > p->max_cols)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d columns asked for, this pipeline was created for 1 to %d.", cols->ncol, p->max_cols);
    }
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run_allsky(GrtPipeline_t *p, GrtColumns_t const *cols, GrtClouds_t const *cl, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    GRT_REQUIRE_PTR(fluxes_dev);
    GRT_TRY(check_clouds(p, cols, cl));
    GRT_TRY(pipeline_run(p, cols, cl, NULL, 0, 0, fluxes_dev, GRT_ALLSKY_FLUXES_PER_COLUMN, NULL));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run_allsky_profiles(GrtPipeline_t *p, GrtColumns_t const *cols, GrtClouds_t const *cl,
                                            fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (level_fluxes_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "level_fluxes_dev is NULL: the level fluxes [ncol][%d][%d] are the output.",
                 GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN, p->num_levels);
    }
    if (p->num_levels < 2)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "heating rates need at least 2 levels (%d).", p->num_levels);
    }
    GRT_TRY(check_clouds(p, cols, cl));
    int const V = p->num_levels;
    /* clear-sky [c][2 V] rows of band bi -> level_fluxes_dev[c][2 bi + {0, 1}][V], all-sky -> [c][4 + 2 bi + {0, 1}][V];
       then both sets' heating rates and six rows */
    GRT_TRY(pipeline_run(p, cols, cl, NULL, 0, 1, level_fluxes_dev, GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN*V, NULL));
    int const bands = (p->band[0].gas != NULL) | (p->band[1].gas != NULL) << 1;
    GRT_TRY(grt_dev_check(grt_launch_profile_finish(grt_dev_stream(p->device), cols->ncol, 2, V, bands, p->user_level,
                                                    GRT_GRAVITY, GRT_SPECIFIC_HEAT_AIR, p->small_d + p->off_p,
                                                    level_fluxes_dev, heating_dev, fluxes_dev), "heating rate kernel"));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run_subcolumns(GrtPipeline_t *p, GrtColumns_t const *cols, GrtClouds_t const *cl,
                                       int num_subcolumns, fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (num_subcolumns < 1 || num_subcolumns > GRT_MAX_SUBCOLUMNS)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d subcolumns asked for: 1 to %d.", num_subcolumns, GRT_MAX_SUBCOLUMNS);
    }
    if (level_fluxes_dev == NULL && fluxes_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "level_fluxes_dev and fluxes_dev are both NULL: nothing to write.%s", "");
    }
    if (level_fluxes_dev != NULL && p->num_levels < 2)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "heating rates need at least 2 levels (%d).", p->num_levels);
    }
    GRT_TRY(check_clouds(p, cols, cl));
    if (level_fluxes_dev == NULL)
    {
        /* grt_pipeline_run_allsky's layout and shortwave sweep rule */
        GRT_TRY(pipeline_run(p, cols, cl, NULL, num_subcolumns, 0, fluxes_dev, GRT_ALLSKY_FLUXES_PER_COLUMN, NULL));
        return GRTCODE_SUCCESS;
    }
    /* grt_pipeline_run_allsky_profiles' layouts; the heating rates and six rows of the mean level fluxes */
    int const V = p->num_levels;
    GRT_TRY(pipeline_run(p, cols, cl, NULL, num_subcolumns, 1, level_fluxes_dev, GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN*V, NULL));
    int const bands = (p->band[0].gas != NULL) | (p->band[1].gas != NULL) << 1;
    GRT_TRY(grt_dev_check(grt_launch_profile_finish(grt_dev_stream(p->device), cols->ncol, 2, V, bands, p->user_level,
                                                    GRT_GRAVITY, GRT_SPECIFIC_HEAT_AIR, p->small_d + p->off_p,
                                                    level_fluxes_dev, heating_dev, fluxes_dev), "heating rate kernel"));
    return GRTCODE_SUCCESS;
}

/* one band's aerosol inputs: none, or at least two strictly increasing grid points and the optics */
static int check_aerosol_band(char const *name, int na, fp_t const *grid, fp_t const *optics)
{
    if (na < 0 || na == 1)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s aerosol grid points: 0 (no aerosol) or at least 2.", na, name);
    }
    if (na == 0)
    {
        return GRTCODE_SUCCESS;
    }
    if (grid == NULL || optics == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s aerosol grid points with a NULL grid or NULL optics.", na, name);
    }
    for (int j = 0; j + 1 < na; ++j)
    {
        if (!(grid[j + 1] > grid[j]))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%s aerosol grid not strictly increasing (grid[%d] = %e, grid[%d] = %e).", name, j,
                     grid[j], j + 1, grid[j + 1]);
        }
    }
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run_aerosols(GrtPipeline_t *p, GrtColumns_t const *cols, GrtAerosols_t const *ae,
                                     fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (ae == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no aerosol inputs (GrtAerosols_t is NULL).%s", "");
    }
    if (level_fluxes_dev == NULL && fluxes_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "level_fluxes_dev and fluxes_dev are both NULL: nothing to write.%s", "");
    }
    if (level_fluxes_dev != NULL && p->num_levels < 2)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "heating rates need at least 2 levels (%d).", p->num_levels);
    }
    /* (a band the pipeline does not have ignores its aerosol fields) */
    GrtAerosols_t a = *ae;
    if (p->band[0].gas == NULL)
    {
        a.lw_num_points = 0;
    }
    if (p->band[1].gas == NULL)
    {
        a.sw_num_points = 0;
    }
    GRT_TRY(check_aerosol_band("longwave", a.lw_num_points, a.lw_grid, a.lw_optics));
    GRT_TRY(check_aerosol_band("shortwave", a.sw_num_points, a.sw_grid, a.sw_optics));
    if (cols->ncol < 1 || cols->ncol > p->max_cols)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d columns asked for, this pipeline was created for 1 to %d.", cols->ncol, p->max_cols);
    }
    if (level_fluxes_dev == NULL)
    {
        /* grt_pipeline_run_allsky's layout (the aerosol set where the all-sky set is) and shortwave sweep rule */
        GRT_TRY(pipeline_run(p, cols, NULL, &a, 0, 0, fluxes_dev, GRT_ALLSKY_FLUXES_PER_COLUMN, NULL));
        return GRTCODE_SUCCESS;
    }
    /* grt_pipeline_run_allsky_profiles' layouts; both sets' heating rates and six rows */
    int const V = p->num_levels;
    GRT_TRY(pipeline_run(p, cols, NULL, &a, 0, 1, level_fluxes_dev, GRT_ALLSKY_PROFILE_ROWS_PER_COLUMN*V, NULL));
    int const bands = (p->band[0].gas != NULL) | (p->band[1].gas != NULL) << 1;
    GRT_TRY(grt_dev_check(grt_launch_profile_finish(grt_dev_stream(p->device), cols->ncol, 2, V, bands, p->user_level,
                                                    GRT_GRAVITY, GRT_SPECIFIC_HEAT_AIR, p->small_d + p->off_p,
                                                    level_fluxes_dev, heating_dev, fluxes_dev), "heating rate kernel"));
    return GRTCODE_SUCCESS;
}

/* one band's bins: none, or num_bins + 1 strictly increasing grid-point indices in 0 .. n - 1 of a band that is computed */
static int check_bins(GrtPipeline_t const *p, int bi, int const *edges, int num_bins, fp_t const *binned_dev)
{
    char const *name = bi == 0 ? "longwave" : "shortwave";
    if (num_bins < 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s bins.", num_bins, name);
    }
    if (num_bins == 0)
    {
        return GRTCODE_SUCCESS;
    }
    if (p->band[bi].gas == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s bins asked for, and this pipeline has no %s band.", num_bins, name, name);
    }
    if (edges == NULL || binned_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s bins with NULL edges or a NULL binned_dev.", num_bins, name);
    }
    long long const n = (long long)p->band[bi].n;
    if (edges[0] < 0 || (long long)edges[num_bins] > n - 1)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s bin edges %d .. %d outside the grid's points 0 .. %lld.", name, edges[0],
                 edges[num_bins], n - 1);
    }
    for (int b = 0; b < num_bins; ++b)
    {
        if (edges[b + 1] <= edges[b])
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%s bin edges not strictly increasing (edges[%d] = %d, edges[%d] = %d).", name, b,
                     edges[b], b + 1, edges[b + 1]);
        }
    }
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run_spectral(GrtPipeline_t *p, GrtColumns_t const *cols, GrtClouds_t const *cl,
                                     int const *lw_edges, int lw_num_bins, int const *sw_edges, int sw_num_bins,
                                     fp_t *spectral_dev, fp_t *binned_dev, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (spectral_dev == NULL || fluxes_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "spectral_dev and fluxes_dev are required (%s is NULL).",
                 spectral_dev == NULL ? "spectral_dev" : "fluxes_dev");
    }
    GRT_TRY(check_bins(p, 0, lw_edges, lw_num_bins, binned_dev));
    GRT_TRY(check_bins(p, 1, sw_edges, sw_num_bins, binned_dev));
    if (cols->ncol < 1 || cols->ncol > p->max_cols)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d columns asked for, this pipeline was created for 1 to %d.", cols->ncol, p->max_cols);
    }
    if (cl != NULL)
    {
        GRT_TRY(check_clouds(p, cols, cl));
    }
    SpectralOut so;
    so.spectral = spectral_dev;
    so.binned = binned_dev;
    so.sets = cl != NULL ? 2 : 1;
    so.set = 0;
    so.edges[0] = lw_edges;
    so.edges[1] = sw_edges;
    so.num_bins[0] = lw_num_bins;
    so.num_bins[1] = sw_num_bins;
    GRT_TRY(pipeline_run(p, cols, cl, NULL, 0, 0, fluxes_dev, cl != NULL ? GRT_ALLSKY_FLUXES_PER_COLUMN : GRT_FLUXES_PER_COLUMN,
                         &so));
    return GRTCODE_SUCCESS;
}
