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
 * grt_pipeline_run_cloud_fields is grt_pipeline_run_subcolumns with the subcolumns' band tables written into the cloud
 * buffer by the device cloud sampler (grt_cloud_sampler.c, k_cloud_sample.hip) from the columns' cloud fields.
 * grt_pipeline_run_aerosols runs the clear-clean pass of grt_pipeline_run or grt_pipeline_run_profiles and then, on the
 * same tau_gas, the clear-sky pass with aerosols of driver.c:426-472: the aerosol object formed inside the solvers from
 * per-column slope and intercept tables (or, materialised form, spread onto the grid and added by the add_optics kernel).
 * grt_pipeline_run_sky runs up to four sets of one driver.c column -- clear-clean, with aerosol, with clouds, with both -- on
 * one gas-optics launch per band: the passes of the entry points above, and the pass that joins aerosol and clouds.
 * grt_pipeline_run_sky_direct is grt_pipeline_run_sky with the direct beam of every set's shortwave beside its rows: taken
 * out of the same solver launches (instances that leave it too), or -- materialised form -- formed from each set's optics.
 * grt_pipeline_run_sky_jacobian is its longwave counterpart, by the same route: the derivative of every set's upward
 * longwave flux with respect to the surface temperature beside the set's rows.
 * grt_pipeline_run_sky_radiances is its six-row form with the longwave radiances at viewing angles of every set, from a
 * kernel of their own queued behind each set's longwave solver -- or, without flux rows, in its place: then the shortwave
 * band is not touched at all.
 * grt_pipeline_run_sky_zeniths is grt_pipeline_run_sky with the shortwave of every set solved under several sun angles per
 * column, as grt_pipeline_run_zeniths solves the clean set's: one gas-optics launch per band, one set of cloud draws.
 * grt_pipeline_run_sky_tiles is grt_pipeline_run_sky's six-row form with several surfaces per column -- emissivity, albedo
 * and skin temperature per tile -- solved on the column's one atmosphere: one gas-optics launch per band, the solvers' walk
 * through the layers shared by a chunk of tiles, every tile's rows and their weighted mean.
 * grt_pipeline_run_band_profiles runs the profile form of the clear-sky pass and, with clouds, of the all-sky pass with
 * every level's flux integrated per wavenumber bin instead of over the whole grid, and one finishing launch for the bins'
 * heating rates.
 * grt_pipeline_run_kdist runs the prologue and the gas optics of the bands that have bins and no solver at all: tau_gas is
 * reduced to its k-distribution per layer and bin (grt_kdist.c, k_kdist.hip); grt_pipeline_run_kdist_correlated reduces
 * every layer under one class map per column, that of a key layer or of the column's vertical optical depth.
 * grt_pipeline_set_surface gives the columns of the runs that follow their own surface emissivity and albedo
 * (driver.c:101-117): rows written on the device from each column's few knots, read by the solvers in place of the shared
 * creation-time arrays.
 * All work is enqueued on the device's library stream; nothing synchronises.
 * Here: the object, the small per-column inputs, the gas optics, the run and the entry points with their checks;
 * grt_pipeline_inputs.c stages what a caller gives besides the columns, grt_pipeline_solve.c solves one band.
 */
#include <stdlib.h>
#include <string.h>
#include "grt_pipeline_internal.h"

static void grt_pipeline_release(GrtPipeline_t **pipeline);

/* the row-pointer table rows_h [n] (integrate_rows' rows) to the device at *rows_d; rows_h is freed (after the upload) */
int grt_upload_rows(GrtPipeline_t *p, double **rows_h, size_t n, double ***rows_d)
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

/* buf holds at least `doubles` doubles afterwards.  One that is large enough stays as it is, contents included.  One that
   is not is replaced, and a live buffer is replaced only after the lane's stream has drained: kernels of an earlier call
   on this lane may still read the old block.  (A buffer that appears for the first time has no reader to wait for.)
   *fresh (unless NULL): the buffer is new, its contents are not the last call's.  A failed allocation leaves it empty. */
int grt_scratch_need(GrtPipeline_t *p, GrtScratch *buf, size_t doubles, int *fresh)
{
    if (fresh != NULL)
    {
        *fresh = doubles > buf->doubles;
    }
    if (doubles <= buf->doubles)
    {
        return GRTCODE_SUCCESS;
    }
    if (buf->d != NULL)
    {
        GRT_TRY(grt_dev_sync(p->device, grt_dev_stream(p->device)));
        grt_dev_free(p->device, buf->d);
        buf->d = NULL;
        buf->doubles = 0;
    }
    void *blk = NULL;
    GRT_TRY(grt_dev_alloc(p->device, &blk, sizeof(double)*doubles));
    buf->d = blk;
    buf->doubles = doubles;
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
    ((GrtGasOpticsImpl *)gas->impl)->profile_tag = (b == &p->band[0]) ? GRT_TAG_GAS_LW : GRT_TAG_GAS_SW;
    size_t const L = (size_t)p->num_levels - 1, V = (size_t)p->num_levels, C = (size_t)p->max_cols;
    size_t const opt = sizeof(double)*C*L*b->n, flx = sizeof(double)*C*V*b->n;
    void *blk = NULL;
    if (!p->keep_spectra)
    {
        /* fused form: tau_gas and the partial sums (the shortwave solver's park block is allocated when a launch first
           needs it: its two-sweep form, GRT_SCRATCH_PARK) */
        b->nblocks = grt_solver_blocks(b->n);
        size_t const part = sizeof(double)*C*6*b->nblocks;
        GRT_TRY(grt_dev_alloc(p->device, &blk, opt + part));
        b->tau_gas = blk;
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
    GRT_TRY(grt_upload_rows(p, rows_h, C*6, &b->rows_d));
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
    GRT_TRY(grt_staging_reserve(p, &p->small, p->small_doubles, p->small_doubles));
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
        grt_dev_free(p->device, p->band[b].rows_d);
        grt_dev_free(p->device, p->band[b].level_rows_d);
        grt_dev_free(p->device, p->band[b].direct_rows_d[0]);
        grt_dev_free(p->device, p->band[b].direct_rows_d[1]);
        for (int k = 0; k < GRT_SCRATCH_COUNT; ++k)
        {
            grt_dev_free(p->device, p->band[b].scratch[k].d);
        }
        grt_keyed_table_free(p, &p->band[b].cloud_map);
        grt_keyed_table_free(p, &p->band[b].aer_map);
        grt_keyed_table_free(p, &p->band[b].bin_table);
        grt_keyed_table_free(p, &p->band[b].surf_map);
        grt_keyed_table_free(p, &p->band[b].channel_table);
        grt_keyed_table_free(p, &p->band[b].tile_map);
        grt_keyed_table_free(p, &p->band[b].response_table);
        grt_keyed_table_free(p, &p->band[b].zen_surf_map);
        grt_kdist_table_free(p->device, &p->band[b].kdist_table);
    }
    grt_staging_free(p, &p->zen_surf);
    grt_staging_free(p, &p->tile);
    grt_staging_free(p, &p->rad);
    grt_staging_free(p, &p->zen);
    grt_staging_free(p, &p->surf);
    grt_staging_free(p, &p->aer);
    grt_staging_free(p, &p->cloud);
    grt_staging_free(p, &p->small);
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

/* A pipeline belongs to the lane (HIP stream) that was selected when it was created: grt_pipeline_stream() hands THAT
   stream to the caller (who orders a gather behind it), while the kernels of a call go to the lane selected now.  The two
   must be the same: select the pipeline's lane before running it. */
static int check_lane(GrtPipeline_t const *p)
{
    if (grt_dev_lane(p->device) != p->lane)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "this pipeline was created on lane %d, lane %d is selected: call grt_device_use_lane "
                 "before grt_pipeline_run.", p->lane, grt_dev_lane(p->device));
    }
    return GRTCODE_SUCCESS;
}

/* A block of the pipeline's own for what a profile run's rows are picked from where the caller takes no copy of it: max_cols
   x GRT_SKY_MAX_SETS x per_set doubles in scratch block `slot` of band b, as *block */
static int own_levels(GrtPipeline_t *p, GrtBand *b, int slot, size_t per_set, double **block)
{
    GRT_TRY(check_lane(p));
    GrtScratch *own = &b->scratch[slot];
    GRT_TRY(grt_scratch_need(p, own, (size_t)p->max_cols*GRT_SKY_MAX_SETS*per_set, NULL));
    *block = own->d;
    return GRTCODE_SUCCESS;
}

/* A band that is not there leaves zeros, as its rows are, and not whatever the caller's buffer held before: n doubles of
   `out`, where that output is given */
static int zero_absent(GrtPipeline_t *p, fp_t *out, size_t n)
{
    if (out != NULL)
    {
        GRT_TRY(grt_dev_zero(p->device, out, sizeof(double)*n, grt_dev_stream(p->device)));
    }
    return GRTCODE_SUCCESS;
}

/* What grt_pipeline_run and grt_pipeline_run_profiles check and stage alike: the arguments, the lane, and the small
   per-column inputs, uploaded to small.d on the library stream.  own_sun 1: the run brings its sun angles itself
   (grt_pipeline_run_zeniths), and the columns' cos_zenith is not read; GRT_SUN_MAY_BE_DOWN: cos_zenith is read and a
   column may be a night column (grt_pipeline_run_ck_fluxes, whose solver leaves zeros there); with GRT_SURFACE_IS_TILES
   added, the run brings its surface temperatures itself (grt_pipeline_run_sky_tiles), and the columns' are not read. */
#define GRT_SUN_MAY_BE_DOWN 2
#define GRT_SURFACE_IS_TILES 4
static int stage_columns(GrtPipeline_t *p, GrtColumns_t const *cols, int own_sun)
{
    int const own_surface = (own_sun & GRT_SURFACE_IS_TILES) != 0;
    own_sun &= ~GRT_SURFACE_IS_TILES;
    GRT_REQUIRE_RANGE(cols->ncol, 1, p->max_cols);
    GRT_REQUIRE_EQ(cols->num_levels, p->num_levels);
    GRT_REQUIRE_PTR(cols->pressure);
    GRT_REQUIRE_PTR(cols->temperature);
    int const V = p->num_levels, L = V - 1, C = cols->ncol;
    GRT_TRY(check_lane(p));
    GRT_TRY(grt_staging_reserve(p, &p->small, p->small_doubles, p->small_doubles));

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
            p->small.h[p->off_n + (size_t)c*L + i] = c_air*dp;
        }
    }
    memcpy(p->small.h + p->off_p, cols->pressure, sizeof(double)*(size_t)C*V);
    if (p->band[0].gas != NULL)
    {
        GRT_REQUIRE_PTR(cols->layer_temperature);
        if (!own_surface)
        {
            GRT_REQUIRE_PTR(cols->surface_temperature);
        }
        for (int c = 0; c < C; ++c)
        {
            if (!own_surface)
            {
                GRT_REQUIRE_RANGE(cols->surface_temperature[c], MIN_TEMPERATURE, MAX_TEMPERATURE);
            }
            for (int i = 0; i < L; ++i)
            {
                GRT_REQUIRE_RANGE(cols->layer_temperature[(size_t)c*L + i], MIN_TEMPERATURE, MAX_TEMPERATURE);
            }
        }
        memcpy(p->small.h + p->off_tl, cols->layer_temperature, sizeof(double)*(size_t)C*L);
        memcpy(p->small.h + p->off_tv, cols->temperature, sizeof(double)*(size_t)C*V);
        if (!own_surface)
        {
            memcpy(p->small.h + p->off_ts, cols->surface_temperature, sizeof(double)*(size_t)C);
        }
    }
    if (p->band[1].gas != NULL)
    {
        GRT_REQUIRE_PTR(cols->total_solar_irradiance);
        if (own_sun != 1)
        {
            GRT_REQUIRE_PTR(cols->cos_zenith);
        }
        for (int c = 0; c < C && own_sun == GRT_SUN_MAY_BE_DOWN; ++c)
        {
            /* (a NaN fails the comparison) */
            if (!(cols->cos_zenith[c] <= 1.))
            {
                GRT_FAIL(GRTCODE_RANGE_ERR, "cosine of zenith angle (%e) of column %d above 1.", cols->cos_zenith[c], c);
            }
        }
        for (int c = 0; c < C && !own_sun; ++c)
        {
            if (!(cols->cos_zenith[c] > 0. && cols->cos_zenith[c] <= 1.))
            {
                GRT_FAIL(GRTCODE_RANGE_ERR, "cosine of zenith angle (%e) of column %d outside (0, 1]"
                         " (night columns are skipped by the caller: driver.c:706).", cols->cos_zenith[c], c);
            }
        }
        if (own_sun != 1)
        {
            memcpy(p->small.h + p->off_mu, cols->cos_zenith, sizeof(double)*(size_t)C);
        }
        memcpy(p->small.h + p->off_tsi, cols->total_solar_irradiance, sizeof(double)*(size_t)C);
    }
    GRT_TRY(grt_staging_upload(p, &p->small, p->small_doubles));
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

/* ---- the surface ------------------------------------------------------------------------------------------------------ */

/* grt_ext.h.  Everything is checked before anything is touched, so a refused call leaves the surface in force as it was;
   then the rows are written on the lane, behind the runs already queued there, which read the rows of the surface before. */
EXTERN int grt_pipeline_set_surface(GrtPipeline_t *p, GrtSurface_t const *surface)
{
    GRT_REQUIRE_PTR(p);
    if (surface == NULL)
    {
        p->surface_ncol = 0;
        for (int bi = 0; bi < 2; ++bi)
        {
            p->band[bi].surf_set = p->band[bi].surf_dif_set = 0;
        }
        return GRTCODE_SUCCESS;
    }
    int np[2];
    GRT_TRY(grt_check_surface(p, surface, np));
    GRT_TRY(check_lane(p));
    /* (a failure from here on is the device's: no surface is in force then, rather than rows half written) */
    p->surface_ncol = 0;
    GRT_TRY(grt_stage_surface(p, surface, np));
    p->surface_ncol = surface->ncol;
    for (int bi = 0; bi < 2; ++bi)
    {
        p->band[bi].surf_set = np[bi] > 0;
        p->band[bi].surf_dif_set = bi == 1 && np[1] > 0 && surface->diffuse_albedo != NULL;
    }
    return GRTCODE_SUCCESS;
}

/* ---- the run ------------------------------------------------------------------------------------------------------ */

/* What joins the gas in a run's sets after the first: nothing (all zero: the run has one set), clouds, aerosols, or both.
   subcolumns > 0 (grt_pipeline_run_subcolumns): a pass with clouds is the mean over that many subcolumns
   (grt_band_solve_subcolumns); with a sampler (grt_pipeline_run_cloud_fields), their tables are written on the device
   from `fields`, and clouds holds the band limits and the thickness only.  sets: the GRT_SKY_... sets that leave, packed
   in bit order (grt_pipeline_run_sky); 0: the clean set, then the set of whichever of clouds and aerosols is given. */
typedef struct GrtJoin
{
    GrtClouds_t const *clouds;
    GrtCloudSampler_t *sampler;
    GrtCloudFields_t const *fields;
    GrtAerosols_t const *aerosols;
    int subcolumns;
    unsigned sets;
    GrtZeniths_t const *zeniths;       /* grt_pipeline_run_zeniths, _run_sky_zeniths: every set's shortwave is the mean over
                                          these angles; with `sets`, the per-angle outputs hold every set's */
    GrtRadiances_t const *radiances;   /* grt_pipeline_run_sky_radiances: every set's longwave leaves its radiances at these
                                          viewing angles too; rows->out NULL: and nothing else runs */
    GrtChannels_t const *channels;     /* grt_pipeline_run_sky_channels (with radiances): and the channels of an instrument */
    long long channel_pairs;           /* ... their (channel, solver block) pairs on the longwave grid (grt_check_channels) */
    GrtWeighting_t const *weighting;   /* grt_pipeline_run_sky_weighting (with channels): and the channels' transmittance
                                          profiles and contribution functions */
    GrtSurfaceTiles_t const *tiles;    /* grt_pipeline_run_sky_tiles: every set of both bands is solved over these surfaces
                                          per column (six rows; rows->out NULL: the tiles' own rows alone) */
    int tile_points[2];                /* ... the knots each band takes of them (grt_check_tiles) */
    GrtResponses_t const *responses;   /* grt_pipeline_run_sky_weighted (profile form): every set's level rows of a band leave
                                          under the band's responses too */
    long long response_pairs[2];       /* ... each band's (response, solver block) pairs and the most responses in one */
    int response_block_max[2];         /* block (grt_check_responses) */
    GrtZenithSurface_t const *zenith_surface;  /* grt_pipeline_run_sky_zeniths_direct (with zeniths and sets): every angle's
                                                  shortwave reads its own direct albedo */
    int zenith_direct;                 /* ... every angle's direct beam leaves too, in the run's form (three rows, or V): */
    double *zenith_direct_out;         /* DEVICE [ncol][sets][3 or V], the mean over the angles, or NULL */
    double *zenith_direct_per_angle;   /* DEVICE [ncol][sets][Z][3 or V], or NULL */
    GrtZenithSlant_t const *zenith_slant;      /* grt_pipeline_run_sky_zeniths_slant (with zeniths and sets; the fused form):
                                                  every angle's direct beam reads a cosine per layer */
} GrtJoin;

#define GRT_SKY_ALL (GRT_SKY_CLEAN | GRT_SKY_AEROSOL | GRT_SKY_CLOUD | GRT_SKY_CLOUD_AEROSOL)
_Static_assert(GRT_SKY_MAX_SETS == GRT_PROFILE_MAX_SETS, "the finishing kernel takes every set of grt_pipeline_run_sky");

/* the sets of a run: the clean one always, whether or not its bit is given */
static unsigned join_sets(GrtJoin const *join)
{
    if (join->sets != 0)
    {
        return join->sets | GRT_SKY_CLEAN;
    }
    return GRT_SKY_CLEAN | (join->aerosols != NULL ? GRT_SKY_AEROSOL : 0u) | (join->clouds != NULL ? GRT_SKY_CLOUD : 0u);
}

EXTERN int grt_pipeline_sky_set_count(unsigned sets)
{
    if ((sets & ~GRT_SKY_ALL) != 0)
    {
        return 0;
    }
    int n = 0;
    for (unsigned bit = GRT_SKY_CLEAN; bit <= GRT_SKY_CLOUD_AEROSOL; bit <<= 1)
    {
        n += ((sets | GRT_SKY_CLEAN) & bit) != 0;
    }
    return n;
}

/* What the run entry points share after their argument checks: the batch (and its clouds and aerosols) staged, then per
   band the gas optics, once, and one solve per set of the run (join_sets) into rows->out, each a copy of `rows` (the
   run's form, output and bins) completed into one pass: the clear-sky solve, then in bit order the aerosol pass, the
   all-sky pass and the pass with both, each set's rows behind the one before (grt_set_offset). */
static int pipeline_run(GrtPipeline_t *p, GrtColumns_t const *cols, GrtJoin const *join, GrtPass const *rows)
{
    GrtClouds_t const *cl = join->clouds;
    GrtAerosols_t const *ae = join->aerosols;
    if (p->surface_ncol > 0 && cols->ncol != p->surface_ncol)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d columns asked for, the surface in force (grt_pipeline_set_surface) has %d.",
                 cols->ncol, p->surface_ncol);
    }
    int const radiances_only = join->radiances != NULL && rows->out == NULL;
    GRT_TRY(stage_columns(p, cols, (join->zeniths != NULL || radiances_only) | (join->tiles != NULL ? GRT_SURFACE_IS_TILES : 0)));
    int const C = cols->ncol, S = join->subcolumns > 0 ? join->subcolumns : 1;
    unsigned const sets = join_sets(join);
    GrtZenithRun zr;
    if (join->zeniths != NULL)
    {
        GRT_TRY(grt_stage_zeniths(p, join->zeniths, C, &zr));
        zr.sky = join->sets != 0;
        if (join->zenith_surface != NULL && p->band[1].gas != NULL)
        {
            GRT_TRY(grt_stage_zenith_surface(p, join->zenith_surface, C, &zr));
        }
        if (join->zenith_slant != NULL && p->band[1].gas != NULL)
        {
            GRT_TRY(grt_stage_zenith_slant(p, join->zenith_slant, C, &zr));
        }
        zr.direct = join->zenith_direct;
        zr.direct_out = join->zenith_direct_out;
        zr.direct_per_angle = join->zenith_direct_per_angle;
    }
    GrtRadianceRun rr;
    if (join->radiances != NULL && p->band[0].gas != NULL)
    {
        GRT_TRY(grt_stage_radiances(p, join->radiances, C, &rr));
    }
    GrtChannelRun cr;
    if (join->channels != NULL && p->band[0].gas != NULL)
    {
        GRT_TRY(grt_stage_channels(p, &p->band[0], join->channels, join->channel_pairs, &cr));
        cr.slots = (sets & (GRT_SKY_CLOUD | GRT_SKY_CLOUD_AEROSOL)) != 0 ? S : 1;
    }
    GrtWeightingRun wr;
    if (join->weighting != NULL)
    {
        grt_stage_weighting(join->weighting, &wr);
    }
    GrtTileRun tr;
    if (join->tiles != NULL)
    {
        GRT_TRY(grt_stage_tiles(p, join->tiles, C, join->tile_points, &tr));
        if (p->band[0].gas == NULL || p->band[1].gas == NULL)
        {
            /* a band that is not there: its rows are zeros in both outputs -- everything is zeroed here, in stream order
               ahead of the kernels that write the other band's rows */
            size_t const slots = (size_t)C*(size_t)rows->sets;
            GRT_TRY(zero_absent(p, rows->out, slots*GRT_FLUXES_PER_COLUMN));
            GRT_TRY(zero_absent(p, tr.per_tile, slots*(size_t)tr.tiles*GRT_FLUXES_PER_COLUMN));
        }
    }
    if (cl != NULL && join->sampler != NULL)
    {
        /* (the kernel writes the tables where grt_stage_clouds puts them) */
        fp_t const *t = join->fields->temperature != NULL ? join->fields->temperature : cols->layer_temperature;
        GRT_TRY(grt_stage_cloud_fields(p, cl, join->sampler, join->fields, t, C, S));
    }
    else if (cl != NULL)
    {
        GRT_TRY(grt_stage_clouds(p, cl, C, S));
    }
    if (ae != NULL)
    {
        GRT_TRY(grt_stage_aerosols(p, ae, C));
    }
    for (int bi = 0; bi < 2; ++bi)
    {
        GrtBand *b = &p->band[bi];
        if (radiances_only)
        {
            if (bi == 1 || b->gas == NULL)
            {
                continue;              /* (grt_pipeline_run_sky_radiances for the radiances alone: no shortwave at all) */
            }
        }
        else if (rows->out == NULL && join->tiles == NULL && (bi == 0 || b->gas == NULL))
        {
            continue;                  /* (grt_pipeline_run_zeniths for the angles' own rows alone: no longwave, no mean) */
        }
        if (b->gas == NULL)
        {
            if (!rows->profile && join->tiles == NULL)
            {
                /* a skipped band's six values are zeros in every set, as the profile forms' rows are: the caller's
                   buffer is not left holding whatever it held before */
                void *s = grt_dev_stream(p->device);
                for (int c = 0; c < C; ++c)
                {
                    double *six = rows->out + (size_t)c*rows->out_stride + GRT_FLUXES_PER_BAND*bi;
                    for (int k = 0; k < rows->sets; ++k)
                    {
                        GRT_TRY(grt_dev_zero(p->device, six + (size_t)k*grt_set_offset(p, 0),
                                             sizeof(double)*GRT_FLUXES_PER_BAND, s));
                    }
                }
            }
            continue;
        }
        if (rows->bins != NULL && rows->profile && rows->bins->num_bins[bi] == 0)
        {
            continue;                  /* (a band without bins has no rows: nothing of it is computed) */
        }
        GrtCloudArgs ca;
        if (cl != NULL)
        {
            GRT_TRY(grt_band_clouds(p, b, bi, cl, C, S, &ca));
        }
        GrtContinua continua;
        GrtPass ps = *rows;
        ps.radiances = bi == 0 && join->radiances != NULL ? &rr : NULL;
        ps.channels = bi == 0 && join->channels != NULL ? &cr : NULL;
        ps.weighting = ps.channels != NULL && join->weighting != NULL ? &wr : NULL;
        ps.tiles = join->tiles != NULL ? &tr : NULL;
        GrtResponseRun rsr;
        if (join->responses != NULL && (bi == 0 ? join->responses->lw_num_responses : join->responses->sw_num_responses) > 0)
        {
            GrtResponses_t const *rs = join->responses;
            GRT_TRY(grt_stage_responses(p, b, bi, rs, join->response_pairs[bi], join->response_block_max[bi], &rsr));
            size_t const V = (size_t)p->num_levels, lw_rows = 2*(size_t)rs->lw_num_responses*V;
            rsr.out = rs->weighted_levels_dev + (bi == 1 ? lw_rows : 0);
            rsr.set_doubles = (uint64_t)(lw_rows + 3*(size_t)rs->sw_num_responses*V);
            rsr.slots = (sets & (GRT_SKY_CLOUD | GRT_SKY_CLOUD_AEROSOL)) != 0 ? S : 1;
            ps.responses = &rsr;
        }
        GrtAerosolArgs aa;
        int const band_aer = ae != NULL && grt_aerosol_points(ae, bi) > 0;
        int aa_ready = 0;
        GRT_TRY(band_gas_optics(p, b, bi, cols, &continua, &ps.defer));
        ps.continua = &continua;
        for (unsigned bit = GRT_SKY_CLEAN; bit <= GRT_SKY_CLOUD_AEROSOL; bit <<= 1)
        {
            if (!(sets & bit))
            {
                continue;
            }
            /* (a band that was given no aerosol runs its aerosol sets without the object) */
            ps.aer_pass = (bit & (GRT_SKY_AEROSOL | GRT_SKY_CLOUD_AEROSOL)) != 0;
            if (ps.aer_pass && band_aer && !aa_ready)
            {
                GRT_TRY(grt_band_aerosols(p, b, bi, ae, C, &aa));
                aa_ready = 1;
            }
            ps.aer = ps.aer_pass && band_aer ? &aa : NULL;
            ps.clouds = (bit & (GRT_SKY_CLOUD | GRT_SKY_CLOUD_AEROSOL)) != 0 ? &ca : NULL;
            if (join->tiles != NULL)
            {
                GRT_TRY(grt_band_solve_tiles(p, b, bi, C, S, &ps));
            }
            else if (bi == 1 && join->zeniths != NULL)
            {
                zr.per_angle = rows->profile ? join->zeniths->zenith_level_fluxes_dev : join->zeniths->zenith_fluxes_dev;
                zr.six = rows->profile ? join->zeniths->zenith_fluxes_dev : NULL;
                GRT_TRY(grt_band_solve_zeniths(p, b, C, S, &ps, &zr));
            }
            else
            {
                GRT_TRY(ps.clouds != NULL && join->subcolumns > 0 ? grt_band_solve_subcolumns(p, b, bi, C, S, &ps) :
                        grt_band_solve(p, b, bi, C, &ps));
            }
            ++ps.set;
        }
    }
    return GRTCODE_SUCCESS;
}

/* ---- the entry points -------------------------------------------------------------------------------------------- */

/* the checks the entry points share (each in that entry point's own order) */
static int check_columns(GrtPipeline_t const *p, GrtColumns_t const *cols)
{
    if (cols->ncol < 1 || cols->ncol > p->max_cols)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d columns asked for, this pipeline was created for 1 to %d.", cols->ncol, p->max_cols);
    }
    return GRTCODE_SUCCESS;
}

static int check_two_levels(GrtPipeline_t const *p)
{
    if (p->num_levels < 2)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "heating rates need at least 2 levels (%d).", p->num_levels);
    }
    return GRTCODE_SUCCESS;
}

/* The rows of a run of `sets` sets per column in the form its two outputs ask for: the profile form, to
   level_fluxes_dev, when that is given, else the six-row form, to fluxes_dev.  rows_form: for the runs that have checked
   their outputs themselves and may leave without rows (the angles' own rows, the radiances or the tiles' rows alone);
   output_form: one of the two is needed, and the profile form needs two levels. */
static void rows_form(GrtPipeline_t const *p, int sets, fp_t *level_fluxes_dev, fp_t *fluxes_dev, GrtPass *rows)
{
    memset(rows, 0, sizeof(*rows));
    rows->profile = level_fluxes_dev != NULL;
    rows->out = rows->profile ? level_fluxes_dev : fluxes_dev;
    rows->sets = sets;
    rows->out_stride = sets*grt_set_offset(p, rows->profile);
}

static int output_form(GrtPipeline_t const *p, int sets, fp_t *level_fluxes_dev, fp_t *fluxes_dev, GrtPass *rows)
{
    if (level_fluxes_dev == NULL && fluxes_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "level_fluxes_dev and fluxes_dev are both NULL: nothing to write.%s", "");
    }
    if (level_fluxes_dev != NULL)
    {
        GRT_TRY(check_two_levels(p));
    }
    rows_form(p, sets, level_fluxes_dev, fluxes_dev, rows);
    return GRTCODE_SUCCESS;
}

/* what closes such a run: in the profile form, the level fluxes' heating rates and six rows, of every set */
static int finish_profiles(GrtPipeline_t *p, int ncol, GrtPass const *rows, fp_t *heating, fp_t *fluxes)
{
    if (!rows->profile)
    {
        return GRTCODE_SUCCESS;
    }
    int const bands = (p->band[0].gas != NULL) | (p->band[1].gas != NULL) << 1;
    GRT_TRY(grt_dev_check(grt_launch_profile_finish(grt_dev_stream(p->device), ncol, rows->sets, p->num_levels, bands,
                                                    p->user_level, GRT_GRAVITY, GRT_SPECIFIC_HEAT_AIR,
                                                    p->small.d + p->off_p, rows->out, heating, fluxes),
                          "heating rate kernel"));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run(GrtPipeline_t *p, GrtColumns_t const *cols, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    GRT_REQUIRE_PTR(fluxes_dev);
    GrtJoin const join = {0};
    GrtPass rows;
    GRT_TRY(output_form(p, 1, NULL, fluxes_dev, &rows));
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
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
    GRT_TRY(check_columns(p, cols));
    /* [c][2 V] rows of band bi -> level_fluxes_dev[c][2 bi + {0, 1}][V], then the level fluxes' heating rates and six rows */
    GrtJoin const join = {0};
    GrtPass rows;
    GRT_TRY(output_form(p, 1, level_fluxes_dev, fluxes_dev, &rows));
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    GRT_TRY(finish_profiles(p, cols->ncol, &rows, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_pipeline_run_zeniths' and grt_pipeline_run_sky_zeniths' checks of the sun angles, the outputs and the batch */
static int check_zeniths(GrtPipeline_t const *p, GrtColumns_t const *cols, GrtZeniths_t const *zn, fp_t const *level_fluxes_dev,
                         fp_t const *fluxes_dev)
{
    if (zn == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no sun angles (GrtZeniths_t is NULL).%s", "");
    }
    if (zn->num_zeniths < 1 || zn->num_zeniths > GRT_MAX_ZENITHS)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d sun angles per column asked for: 1 to %d.", zn->num_zeniths, GRT_MAX_ZENITHS);
    }
    if (zn->cos_zenith == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "cos_zenith is NULL: the sun angles [ncol][%d] are the input.", zn->num_zeniths);
    }
    int const profile = level_fluxes_dev != NULL;
    if (!profile && fluxes_dev == NULL && zn->zenith_fluxes_dev == NULL && zn->zenith_level_fluxes_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "fluxes_dev, level_fluxes_dev and both per-angle outputs are NULL: nothing to write.%s",
                 "");
    }
    if (!profile && zn->zenith_level_fluxes_dev != NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "zenith_level_fluxes_dev is given in the six-row form (level_fluxes_dev is NULL).%s", "");
    }
    GRT_TRY(check_columns(p, cols));
    if (cols->num_levels != p->num_levels)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "columns of %d levels: this pipeline has %d.", cols->num_levels, p->num_levels);
    }
    if (profile)
    {
        GRT_TRY(check_two_levels(p));
    }
    size_t const n = (size_t)cols->ncol*(size_t)zn->num_zeniths;
    for (size_t k = 0; k < n; ++k)
    {
        if (!(zn->cos_zenith[k] <= 1.))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "cosine of zenith angle %zu of column %zu (%e) is NaN or above 1.",
                     k % (size_t)zn->num_zeniths, k/(size_t)zn->num_zeniths, zn->cos_zenith[k]);
        }
        if (zn->weight != NULL && !(zn->weight[k] >= 0.))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "weight of zenith angle %zu of column %zu (%e) is negative or NaN.",
                     k % (size_t)zn->num_zeniths, k/(size_t)zn->num_zeniths, zn->weight[k]);
        }
    }
    return GRTCODE_SUCCESS;
}

/* What closes both: the run of `sets` sets per column under the angles of join->zeniths, in the form the outputs ask for
   (fluxes_dev may be NULL with a per-angle output: then neither the longwave nor the mean is formed) */
static int run_under_zeniths(GrtPipeline_t *p, GrtColumns_t const *cols, GrtJoin const *join, int sets,
                             fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev)
{
    GrtZeniths_t const *zn = join->zeniths;
    GrtPass rows;
    rows_form(p, sets, level_fluxes_dev, fluxes_dev, &rows);
    GRT_TRY(pipeline_run(p, cols, join, &rows));
    GRT_TRY(finish_profiles(p, cols->ncol, &rows, heating_dev, fluxes_dev));
    if (p->band[1].gas == NULL)
    {
        /* no shortwave band: every angle's rows are zeros, as the band's rows of the mean are */
        size_t const n = (size_t)cols->ncol*(size_t)sets*(size_t)zn->num_zeniths;
        GRT_TRY(zero_absent(p, zn->zenith_fluxes_dev, n*GRT_FLUXES_PER_BAND));
        GRT_TRY(zero_absent(p, zn->zenith_level_fluxes_dev, n*2*(size_t)p->num_levels));
    }
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: the clear-clean set under several sun angles per column, on one gas-optics pass per band */
EXTERN int grt_pipeline_run_zeniths(GrtPipeline_t *p, GrtColumns_t const *cols, GrtZeniths_t const *zn,
                                    fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    GRT_TRY(check_zeniths(p, cols, zn, level_fluxes_dev, fluxes_dev));
    /* grt_pipeline_run's layout, or grt_pipeline_run_profiles' three; the shortwave rows the mean over the angles */
    GrtJoin const join = {.zeniths = zn};
    GRT_TRY(run_under_zeniths(p, cols, &join, 1, level_fluxes_dev, heating_dev, fluxes_dev));
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
    GRT_TRY(check_columns(p, cols));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run_allsky(GrtPipeline_t *p, GrtColumns_t const *cols, GrtClouds_t const *cl, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    GRT_REQUIRE_PTR(fluxes_dev);
    GRT_TRY(check_clouds(p, cols, cl));
    GrtJoin const join = {.clouds = cl};
    GrtPass rows;
    GRT_TRY(output_form(p, 2, NULL, fluxes_dev, &rows));
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
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
    /* clear-sky [c][2 V] rows of band bi -> level_fluxes_dev[c][2 bi + {0, 1}][V], all-sky -> [c][4 + 2 bi + {0, 1}][V];
       then both sets' heating rates and six rows */
    GrtJoin const join = {.clouds = cl};
    GrtPass rows;
    GRT_TRY(output_form(p, 2, level_fluxes_dev, fluxes_dev, &rows));
    GRT_TRY(check_clouds(p, cols, cl));
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    GRT_TRY(finish_profiles(p, cols->ncol, &rows, heating_dev, fluxes_dev));
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
    /* grt_pipeline_run_allsky's layout and shortwave sweep rule; or grt_pipeline_run_allsky_profiles' layouts, the heating
       rates and six rows of the mean level fluxes */
    GrtJoin const join = {.clouds = cl, .subcolumns = num_subcolumns};
    GrtPass rows;
    GRT_TRY(output_form(p, 2, level_fluxes_dev, fluxes_dev, &rows));
    GRT_TRY(check_clouds(p, cols, cl));
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    GRT_TRY(finish_profiles(p, cols->ncol, &rows, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: grt_pipeline_run_subcolumns with the tables sampled on the device from the cloud fields */
EXTERN int grt_pipeline_run_cloud_fields(GrtPipeline_t *p, GrtColumns_t const *cols, GrtCloudSampler_t *sampler,
                                         GrtCloudFields_t const *fields, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                         fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    GRT_TRY(grt_cloud_sampler_check(sampler, fields, 0));
    if (fields->thickness == NULL || (fields->temperature == NULL && cols->layer_temperature == NULL))
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "a NULL array in the cloud fields (thickness; temperature with no layer temperatures "
                 "in the columns).%s", "");
    }
    if (grt_cloud_sampler_device(sampler) != p->device)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "the sampler was created on device %d, the pipeline on device %d.",
                 (int)grt_cloud_sampler_device(sampler), (int)p->device);
    }
    if (fields->ncol != cols->ncol)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "cloud fields of %d columns for a batch of %d.", fields->ncol, cols->ncol);
    }
    GRT_TRY(check_columns(p, cols));
    if (fields->num_layers != p->num_levels - 1 || cols->num_levels != p->num_levels)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "cloud fields of %d layers, columns of %d levels: this pipeline has %d levels.",
                 fields->num_layers, cols->num_levels, p->num_levels);
    }
    GrtPass rows;
    GRT_TRY(output_form(p, 2, level_fluxes_dev, fluxes_dev, &rows));
    GrtClouds_t cl;
    memset(&cl, 0, sizeof(cl));
    grt_cloud_sampler_bands(sampler, &cl);
    cl.thickness = fields->thickness;
    GrtJoin const join = {.clouds = &cl, .sampler = sampler, .fields = fields, .subcolumns = fields->num_subcolumns};
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    GRT_TRY(finish_profiles(p, cols->ncol, &rows, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* one band's aerosol inputs: none, or at least two strictly increasing grid points and the optics */
static int check_aerosol_band(char const *name, int na, fp_t const *grid, fp_t const *optics)
{
    GRT_TRY(grt_check_grid(name, " aerosol", "no aerosol", "optics", na, grid, optics));
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
    /* grt_pipeline_run_allsky's layout (the aerosol set where the all-sky set is) and shortwave sweep rule; or
       grt_pipeline_run_allsky_profiles' layouts, both sets' heating rates and six rows */
    GrtPass rows;
    GRT_TRY(output_form(p, 2, level_fluxes_dev, fluxes_dev, &rows));
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
    GRT_TRY(check_columns(p, cols));
    GrtJoin const join = {.aerosols = &a};
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    GRT_TRY(finish_profiles(p, cols->ncol, &rows, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_pipeline_run_sky's (, _sky_direct's and _sky_zeniths') checks of the request: the sets, and that what they need is
   there; *nsets: the sets per column */
static int check_sky_sets(GrtSky_t const *sky, int *nsets)
{
    if (sky == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no sky inputs (GrtSky_t is NULL).%s", "");
    }
    *nsets = grt_pipeline_sky_set_count(sky->sets);
    if (*nsets == 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "sets 0x%x: bits outside GRT_SKY_CLEAN | _AEROSOL | _CLOUD | _CLOUD_AEROSOL (0x%x).",
                 sky->sets, GRT_SKY_ALL);
    }
    int const with_clouds = (sky->sets & (GRT_SKY_CLOUD | GRT_SKY_CLOUD_AEROSOL)) != 0;
    int const with_aerosols = (sky->sets & (GRT_SKY_AEROSOL | GRT_SKY_CLOUD_AEROSOL)) != 0;
    if (with_clouds && sky->clouds == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "sets 0x%x ask for a cloud set, and clouds is NULL.", sky->sets);
    }
    if (with_aerosols && sky->aerosols == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "sets 0x%x ask for an aerosol set, and aerosols is NULL.", sky->sets);
    }
    if (with_clouds && (sky->num_subcolumns < 1 || sky->num_subcolumns > GRT_MAX_SUBCOLUMNS))
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d subcolumns asked for: 1 to %d.", sky->num_subcolumns, GRT_MAX_SUBCOLUMNS);
    }
    return GRTCODE_SUCCESS;
}

/* ... and of its inputs and the batch; *join: the run they describe, its aerosols in *a */
static int sky_join(GrtPipeline_t const *p, GrtColumns_t const *cols, GrtSky_t const *sky, GrtAerosols_t *a, GrtJoin *join)
{
    int const with_clouds = (sky->sets & (GRT_SKY_CLOUD | GRT_SKY_CLOUD_AEROSOL)) != 0;
    int const with_aerosols = (sky->sets & (GRT_SKY_AEROSOL | GRT_SKY_CLOUD_AEROSOL)) != 0;
    /* (inputs that no set asks for are not looked at; a band the pipeline does not have ignores its aerosol fields) */
    memset(a, 0, sizeof(*a));
    if (with_aerosols)
    {
        *a = *sky->aerosols;
        if (p->band[0].gas == NULL)
        {
            a->lw_num_points = 0;
        }
        if (p->band[1].gas == NULL)
        {
            a->sw_num_points = 0;
        }
        GRT_TRY(check_aerosol_band("longwave", a->lw_num_points, a->lw_grid, a->lw_optics));
        GRT_TRY(check_aerosol_band("shortwave", a->sw_num_points, a->sw_grid, a->sw_optics));
    }
    GRT_TRY(with_clouds ? check_clouds(p, cols, sky->clouds) : check_columns(p, cols));
    /* one draw per column: the all-sky instances of the solvers; more: their subcolumn instances and the mean */
    memset(join, 0, sizeof(*join));
    join->clouds = with_clouds ? sky->clouds : NULL;
    join->aerosols = with_aerosols ? a : NULL;
    join->subcolumns = with_clouds && sky->num_subcolumns > 1 ? sky->num_subcolumns : 0;
    join->sets = sky->sets | GRT_SKY_CLEAN;
    return GRTCODE_SUCCESS;
}

/* The third row group a sky run may carry beside its rows, the outputs attached: the shortwave's direct beam
   (grt_pipeline_run_sky_direct: band 1) or the longwave's surface-temperature Jacobian (grt_pipeline_run_sky_jacobian:
   band 0); three: [ncol][sets][3], required; levels: [ncol][sets][V], profile form only, may be NULL */
typedef struct SkyThird
{
    int band;
    char const *what, *arg, *three_name, *levels_name;
    fp_t *three, *levels;
    int missing;                   /* the caller's struct is NULL */
} SkyThird;

/* grt_pipeline_run_sky and, with a third row group, grt_pipeline_run_sky_direct and _jacobian: the same request */
static int run_sky(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky, SkyThird const *third,
                   fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (third != NULL)
    {
        if (third->missing || third->three == NULL)
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%s is NULL: the %s rows [ncol][sets][%d] are the output.",
                     third->missing ? third->arg : third->three_name, third->what, GRT_DIRECT_ROWS_PER_SET);
        }
        if (level_fluxes_dev == NULL && third->levels != NULL)
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%s is given in the six-row form (level_fluxes_dev is NULL).", third->levels_name);
        }
    }
    int nsets;
    GRT_TRY(check_sky_sets(sky, &nsets));
    GrtPass rows;
    GRT_TRY(output_form(p, nsets, level_fluxes_dev, fluxes_dev, &rows));
    GrtAerosols_t a;
    GrtJoin join;
    GRT_TRY(sky_join(p, cols, sky, &a, &join));
    GrtBand *tb = third != NULL ? &p->band[third->band] : NULL;
    int const V = p->num_levels;
    double *third_rows = NULL;
    if (third != NULL && tb->gas != NULL)
    {
        /* the passes' third rows: the caller's three per set, or -- profile form -- V levels per set, the caller's or the
           pipeline's own, and the three rows from them afterwards */
        third_rows = rows.profile ? third->levels : third->three;
        if (third_rows == NULL)
        {
            GRT_TRY(own_levels(p, tb, GRT_SCRATCH_DIRECT_LEVELS, (size_t)V, &third_rows));
        }
        if (third->band == 1)
        {
            rows.direct = third_rows;
        }
        else
        {
            rows.jacobian = third_rows;
        }
    }
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    GRT_TRY(finish_profiles(p, cols->ncol, &rows, heating_dev, fluxes_dev));
    if (third != NULL)
    {
        size_t const slots = (size_t)cols->ncol*(size_t)nsets;
        if (tb->gas == NULL)
        {
            GRT_TRY(zero_absent(p, third->three, slots*GRT_DIRECT_ROWS_PER_SET));
            GRT_TRY(zero_absent(p, third->levels, slots*(size_t)V));
        }
        else if (rows.profile)
        {
            GRT_TRY(grt_dev_check(grt_launch_direct_rows(grt_dev_stream(p->device), (int)slots, V, p->user_level, third_rows,
                                                         third->three), "row pick kernel"));
        }
    }
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: the sets of one driver.c column that are asked for, on one gas-optics pass per band */
EXTERN int grt_pipeline_run_sky(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky, fp_t *level_fluxes_dev,
                                fp_t *heating_dev, fp_t *fluxes_dev)
{
    GRT_TRY(run_sky(p, cols, sky, NULL, level_fluxes_dev, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: grt_pipeline_run_sky, and the scattering correction of every set's longwave, added to its rows */
EXTERN int grt_pipeline_run_sky_scattering(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                           fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev,
                                           fp_t *scatter_levels_dev, fp_t *scatter_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (scatter_levels_dev == NULL && scatter_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "scatter_levels_dev and scatter_dev are both NULL: the differences are the output.%s", "");
    }
    if (level_fluxes_dev == NULL && scatter_levels_dev != NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "scatter_levels_dev is given in the six-row form (level_fluxes_dev is NULL).%s", "");
    }
    if (p->band[0].gas == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "this pipeline has no longwave band: nothing to correct.%s", "");
    }
    int nsets;
    GRT_TRY(check_sky_sets(sky, &nsets));
    GrtPass rows;
    GRT_TRY(output_form(p, nsets, level_fluxes_dev, fluxes_dev, &rows));
    GrtAerosols_t a;
    GrtJoin join;
    GRT_TRY(sky_join(p, cols, sky, &a, &join));
    int const V = p->num_levels, C = cols->ncol, lw_rows = rows.profile ? 2*V : GRT_FLUXES_PER_BAND;
    /* the passes' differences: the caller's six per set, or -- profile form -- 2 V levels per set, the caller's or the
       pipeline's own, and the six rows from them afterwards */
    GrtScatterRun sr = {rows.profile ? scatter_levels_dev : scatter_dev};
    if (sr.out == NULL)
    {
        GRT_TRY(own_levels(p, &p->band[0], GRT_SCRATCH_SCATTER_LEVELS, 2*(size_t)V, &sr.out));
    }
    rows.scatter = &sr;
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    /* every longwave row of every set += its difference, then the heating rates and six rows of the corrected levels */
    void *s = grt_dev_stream(p->device);
    int const slot = grt_profile_begin(s, GRT_TAG_SCATTER_FINISH);
    int krc = grt_launch_scatter_add(s, C*nsets, lw_rows, rows.out, (uint64_t)grt_set_offset(p, rows.profile), 0, sr.out,
                                     (uint64_t)lw_rows, 0);
    if (krc == 0 && rows.profile && scatter_dev != NULL)
    {
        krc = grt_launch_direct_rows(s, C*nsets*2, V, p->user_level, sr.out, scatter_dev);
    }
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "scattering addition kernel"));
    GRT_TRY(finish_profiles(p, C, &rows, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: grt_pipeline_run_sky, and the direct beam of every set's shortwave */
EXTERN int grt_pipeline_run_sky_direct(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                       GrtDirectBeam_t const *direct, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                       fp_t *fluxes_dev)
{
    SkyThird const third = {1, "direct-beam", "direct (GrtDirectBeam_t)", "direct_fluxes_dev", "direct_level_fluxes_dev",
                            direct != NULL ? direct->direct_fluxes_dev : NULL,
                            direct != NULL ? direct->direct_level_fluxes_dev : NULL, direct == NULL};
    GRT_TRY(run_sky(p, cols, sky, &third, level_fluxes_dev, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: grt_pipeline_run_sky, and the surface-temperature Jacobian of every set's upward longwave */
EXTERN int grt_pipeline_run_sky_jacobian(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                         GrtSurfaceJacobian_t const *jacobian, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                         fp_t *fluxes_dev)
{
    SkyThird const third = {0, "surface Jacobian", "jacobian (GrtSurfaceJacobian_t)", "jacobian_fluxes_dev",
                            "jacobian_level_fluxes_dev", jacobian != NULL ? jacobian->jacobian_fluxes_dev : NULL,
                            jacobian != NULL ? jacobian->jacobian_level_fluxes_dev : NULL, jacobian == NULL};
    GRT_TRY(run_sky(p, cols, sky, &third, level_fluxes_dev, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: grt_pipeline_run_sky's profile form, and every set's level rows under the bands' spectral responses */
EXTERN int grt_pipeline_run_sky_weighted(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                         GrtResponses_t const *rs, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                         fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (rs == NULL || rs->weighted_levels_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s is NULL: the weighted level rows [ncol][sets][2 R_lw + 3 R_sw][V] are the output.",
                 rs == NULL ? "responses (GrtResponses_t)" : "weighted_levels_dev");
    }
    GrtJoin weighted;
    memset(&weighted, 0, sizeof(weighted));
    for (int bi = 0; bi < 2; ++bi)
    {
        GrtBand const *b = &p->band[bi];
        GRT_TRY(grt_check_responses(rs, bi, b->gas != NULL ? (long long)b->n : 0, grt_pipeline_response_block_limit(p, bi),
                                    &weighted.response_pairs[bi], &weighted.response_block_max[bi]));
    }
    if (rs->lw_num_responses == 0 && rs->sw_num_responses == 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no responses in either band: nothing to weight.%s", "");
    }
    if (rs->actinic_levels_dev != NULL && rs->sw_num_responses == 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "actinic_levels_dev is given without shortwave responses.%s", "");
    }
    if (level_fluxes_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "level_fluxes_dev is NULL: the call is grt_pipeline_run_sky's profile form.%s", "");
    }
    int nsets;
    GRT_TRY(check_sky_sets(sky, &nsets));
    GrtPass rows;
    GRT_TRY(output_form(p, nsets, level_fluxes_dev, fluxes_dev, &rows));
    GrtAerosols_t a;
    GrtJoin join;
    GRT_TRY(sky_join(p, cols, sky, &a, &join));
    join.responses = rs;
    memcpy(join.response_pairs, weighted.response_pairs, sizeof(join.response_pairs));
    memcpy(join.response_block_max, weighted.response_block_max, sizeof(join.response_block_max));
    int const V = p->num_levels;
    if (rs->sw_num_responses > 0)
    {
        /* the shortwave's response rows ride with the direct beam's: its levels go to the pipeline's own block */
        GRT_TRY(own_levels(p, &p->band[1], GRT_SCRATCH_DIRECT_LEVELS, (size_t)V, &rows.direct));
    }
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    GRT_TRY(finish_profiles(p, cols->ncol, &rows, heating_dev, fluxes_dev));
    if (rs->actinic_levels_dev != NULL)
    {
        void *s = grt_dev_stream(p->device);
        uint64_t const lw_rows = 2*(uint64_t)rs->lw_num_responses*(uint64_t)V;
        GRT_TIMED(s, GRT_TAG_BAND_PROFILES, "actinic flux kernel",
                  grt_launch_actinic_rows(s, rs->weighted_levels_dev + lw_rows,
                                          lw_rows + 3*(uint64_t)rs->sw_num_responses*(uint64_t)V, cols->ncol, nsets,
                                          rs->sw_num_responses, V, p->small.d + p->off_mu, 0.5, rs->actinic_levels_dev));
    }
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: the (response, solver block) pairs of a band's responses on a grid of num_points; -1: responses the call refuses */
EXTERN long long grt_response_pair_count(GrtResponses_t const *rs, int band, long long num_points)
{
    long long pairs;
    int block_max;
    if (rs == NULL || band < 0 || band > 1 || num_points < 1 ||
        grt_check_responses(rs, band, num_points, -1, &pairs, &block_max) != GRTCODE_SUCCESS)
    {
        return -1;
    }
    return pairs;
}

/* grt_ext.h: the most responses of a band with a point in one solver block at this pipeline's V */
EXTERN int grt_pipeline_response_block_limit(GrtPipeline_t const *p, int band)
{
    if (p == NULL || band < 0 || band > 1)
    {
        return -1;
    }
    return grt_response_block_limit(p->num_levels, band == 0 ? 2 : 3);
}

/* grt_pipeline_run_sky_radiances, and -- channels_asked -- grt_pipeline_run_sky_channels, which is the same call with the
   channels of an instrument (ch; checked here, NULL included) */
static int run_sky_radiances(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky, GrtRadiances_t const *rd,
                             int channels_asked, GrtChannels_t const *ch, int weighting_asked, GrtWeighting_t const *wt,
                             fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (rd == NULL || rd->radiances_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s is NULL: the radiances [ncol][sets][angles][%d] are the output.",
                 rd == NULL ? "radiances (GrtRadiances_t)" : "radiances_dev", GRT_RADIANCE_ROWS_PER_ANGLE);
    }
    int nsets;
    GRT_TRY(check_sky_sets(sky, &nsets));
    GrtAerosols_t a;
    GrtJoin join;
    GRT_TRY(sky_join(p, cols, sky, &a, &join));
    GRT_TRY(grt_check_radiances(rd, cols->ncol));
    long long pairs = 0;
    if (channels_asked)
    {
        GRT_TRY(grt_check_channels(ch, p->band[0].gas != NULL ? (long long)p->band[0].n : 0, &pairs));
        if (ch->channel_radiances_dev == NULL)
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "channel_radiances_dev is NULL: the channel radiances [ncol][sets][angles][%d][%d] are "
                     "the output.", GRT_RADIANCE_ROWS_PER_ANGLE, ch->num_channels);
        }
    }
    if (weighting_asked)
    {
        GRT_TRY(grt_check_weighting(wt));
    }
    int const spectral = rd->spectral_radiances_dev != NULL || rd->brightness_dev != NULL;
    if (spectral && join.subcolumns > 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s is given with a cloud set of %d draws: the radiances at every point are those of one "
                 "draw per column.", rd->spectral_radiances_dev != NULL ? "spectral_radiances_dev" : "brightness_dev",
                 join.subcolumns);
    }
    join.radiances = rd;
    join.channels = channels_asked ? ch : NULL;
    join.channel_pairs = pairs;
    join.weighting = weighting_asked ? wt : NULL;
    GrtPass rows;
    rows_form(p, nsets, NULL, fluxes_dev, &rows);
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    if (p->band[0].gas == NULL)
    {
        /* no longwave band (a spectral row of such a pipeline has no points) */
        size_t const per_level = (size_t)cols->ncol*(size_t)nsets*(size_t)rd->num_angles;
        size_t const rows_all = per_level*GRT_RADIANCE_ROWS_PER_ANGLE;
        GRT_TRY(zero_absent(p, rd->radiances_dev, rows_all));
        if (channels_asked)
        {
            size_t const channels = (size_t)ch->num_channels, V = (size_t)p->num_levels;
            GRT_TRY(zero_absent(p, ch->channel_radiances_dev, rows_all*channels));
            GRT_TRY(zero_absent(p, ch->channel_brightness_dev, rows_all*channels));
            if (weighting_asked)
            {
                GRT_TRY(zero_absent(p, wt->transmittance_dev, per_level*channels*V));
                GRT_TRY(zero_absent(p, wt->contribution_dev, per_level*channels*(V + 1)));
            }
        }
    }
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: grt_pipeline_run_sky's six-row form, and the longwave radiances of every set at the columns' viewing angles;
   fluxes_dev NULL: the radiances alone */
EXTERN int grt_pipeline_run_sky_radiances(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                          GrtRadiances_t const *rd, fp_t *fluxes_dev)
{
    return run_sky_radiances(p, cols, sky, rd, 0, NULL, 0, NULL, fluxes_dev);
}

/* grt_ext.h: ... and the radiances and brightness temperatures of an instrument's channels */
EXTERN int grt_pipeline_run_sky_channels(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                         GrtRadiances_t const *rd, GrtChannels_t const *ch, fp_t *fluxes_dev)
{
    return run_sky_radiances(p, cols, sky, rd, 1, ch, 0, NULL, fluxes_dev);
}

/* grt_ext.h: ... and the channels' level-to-space transmittance profiles and contribution functions */
EXTERN int grt_pipeline_run_sky_weighting(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                          GrtRadiances_t const *rd, GrtChannels_t const *ch, GrtWeighting_t const *wt,
                                          fp_t *fluxes_dev)
{
    return run_sky_radiances(p, cols, sky, rd, 1, ch, 1, wt, fluxes_dev);
}

/* grt_ext.h: the (channel, solver block) pairs of an instrument on a grid of num_points; -1: channels the call refuses */
EXTERN long long grt_channel_pair_count(GrtChannels_t const *ch, long long num_points)
{
    long long pairs;
    if (num_points < 1 || grt_check_channels(ch, num_points, &pairs) != GRTCODE_SUCCESS)
    {
        return -1;
    }
    return pairs;
}

/* grt_ext.h: the sets of grt_pipeline_run_sky, the shortwave of each under several sun angles per column */
EXTERN int grt_pipeline_run_sky_zeniths(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                        GrtZeniths_t const *zn, fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    int nsets;
    GRT_TRY(check_sky_sets(sky, &nsets));
    GrtAerosols_t a;
    GrtJoin join;
    GRT_TRY(sky_join(p, cols, sky, &a, &join));
    GRT_TRY(check_zeniths(p, cols, zn, level_fluxes_dev, fluxes_dev));
    join.zeniths = zn;
    GRT_TRY(run_under_zeniths(p, cols, &join, nsets, level_fluxes_dev, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_pipeline_run_sky_zeniths_direct and, with slant, grt_pipeline_run_sky_zeniths_slant: one body */
static int sky_zeniths_direct(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky, GrtZeniths_t const *zn,
                              GrtZenithSlant_t const *slant, GrtZenithSurface_t const *surface,
                              GrtZenithDirect_t const *direct, fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev)
{
    int nsets;
    GRT_TRY(check_sky_sets(sky, &nsets));
    GrtAerosols_t a;
    GrtJoin join;
    GRT_TRY(sky_join(p, cols, sky, &a, &join));
    GRT_TRY(check_zeniths(p, cols, zn, level_fluxes_dev, fluxes_dev));
    if (surface == NULL && direct == NULL && slant == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "surface and direct are both NULL: grt_pipeline_run_sky_zeniths is that call.%s", "");
    }
    int const profile = level_fluxes_dev != NULL, V = p->num_levels, Z = zn->num_zeniths;
    if (direct != NULL)
    {
        if (direct->direct_fluxes_dev == NULL && direct->direct_level_fluxes_dev == NULL &&
            direct->zenith_direct_fluxes_dev == NULL && direct->zenith_direct_level_fluxes_dev == NULL)
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "the four outputs of direct (GrtZenithDirect_t) are all NULL: nothing to write.%s", "");
        }
        if (!profile && (direct->direct_level_fluxes_dev != NULL || direct->zenith_direct_level_fluxes_dev != NULL))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%s is given in the six-row form (level_fluxes_dev is NULL).",
                     direct->direct_level_fluxes_dev != NULL ? "direct_level_fluxes_dev" : "zenith_direct_level_fluxes_dev");
        }
    }
    if (surface != NULL)
    {
        GRT_TRY(grt_check_zenith_surface(surface, cols->ncol, Z));
    }
    if (slant != NULL)
    {
        if (p->keep_spectra)
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "a pipeline in the materialised form (keep_spectra = 1): the layer cosines join the "
                     "fused solver alone.%s", "");
        }
        GRT_TRY(grt_check_zenith_slant(slant, zn, cols->ncol, V - 1));
    }
    join.zeniths = zn;
    join.zenith_surface = surface;
    join.zenith_slant = slant;
    GrtBand *sw = &p->band[1];
    if (direct != NULL && sw->gas != NULL)
    {
        /* the passes' direct rows: the caller's three per set (and angle), or -- profile form -- V levels, the caller's or
           the pipeline's own, and the three rows from them afterwards */
        join.zenith_direct = 1;
        join.zenith_direct_out = profile ? direct->direct_level_fluxes_dev : direct->direct_fluxes_dev;
        join.zenith_direct_per_angle = profile ? direct->zenith_direct_level_fluxes_dev : direct->zenith_direct_fluxes_dev;
        if (profile && join.zenith_direct_out == NULL && direct->direct_fluxes_dev != NULL)
        {
            GRT_TRY(own_levels(p, sw, GRT_SCRATCH_DIRECT_LEVELS, (size_t)V, &join.zenith_direct_out));
        }
        if (profile && join.zenith_direct_per_angle == NULL && direct->zenith_direct_fluxes_dev != NULL)
        {
            GRT_TRY(own_levels(p, sw, GRT_SCRATCH_ZEN_DIRECT_LEVELS, (size_t)Z*(size_t)V, &join.zenith_direct_per_angle));
        }
    }
    GRT_TRY(run_under_zeniths(p, cols, &join, nsets, level_fluxes_dev, heating_dev, fluxes_dev));
    if (direct == NULL)
    {
        return GRTCODE_SUCCESS;
    }
    void *s = grt_dev_stream(p->device);
    size_t const slots = (size_t)cols->ncol*(size_t)nsets;
    if (sw->gas == NULL)
    {
        /* no shortwave band: zeros, as the band's rows are */
        fp_t *const out[4] = {direct->direct_fluxes_dev, direct->zenith_direct_fluxes_dev, direct->direct_level_fluxes_dev,
                              direct->zenith_direct_level_fluxes_dev};
        for (int k = 0; k < 4; ++k)
        {
            GRT_TRY(zero_absent(p, out[k], slots*(size_t)(k & 1 ? Z : 1)*(size_t)(k < 2 ? GRT_DIRECT_ROWS_PER_SET : V)));
        }
    }
    else if (profile)
    {
        if (direct->direct_fluxes_dev != NULL)
        {
            GRT_TRY(grt_dev_check(grt_launch_direct_rows(s, (int)slots, V, p->user_level, join.zenith_direct_out,
                                                         direct->direct_fluxes_dev), "row pick kernel"));
        }
        if (direct->zenith_direct_fluxes_dev != NULL)
        {
            GRT_TRY(grt_dev_check(grt_launch_direct_rows(s, (int)(slots*(size_t)Z), V, p->user_level,
                                                         join.zenith_direct_per_angle, direct->zenith_direct_fluxes_dev),
                                  "row pick kernel"));
        }
    }
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: grt_pipeline_run_sky_zeniths with a direct-beam albedo per (column, angle), every angle's direct beam, or both */
EXTERN int grt_pipeline_run_sky_zeniths_direct(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                               GrtZeniths_t const *zn, GrtZenithSurface_t const *surface,
                                               GrtZenithDirect_t const *direct, fp_t *level_fluxes_dev, fp_t *heating_dev,
                                               fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    GRT_TRY(sky_zeniths_direct(p, cols, sky, zn, NULL, surface, direct, level_fluxes_dev, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: ... with a sun cosine per layer for the direct beam (slant NULL: the call above) */
EXTERN int grt_pipeline_run_sky_zeniths_slant(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                              GrtZeniths_t const *zn, GrtZenithSlant_t const *slant,
                                              GrtZenithSurface_t const *surface, GrtZenithDirect_t const *direct,
                                              fp_t *level_fluxes_dev, fp_t *heating_dev, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    GRT_TRY(sky_zeniths_direct(p, cols, sky, zn, slant, surface, direct, level_fluxes_dev, heating_dev, fluxes_dev));
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: the sets of grt_pipeline_run_sky's six-row form over several surface tiles per column */
EXTERN int grt_pipeline_run_sky_tiles(GrtPipeline_t *p, GrtColumns_t const *cols, GrtSky_t const *sky,
                                      GrtSurfaceTiles_t const *tiles, fp_t *fluxes_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    int nsets;
    GRT_TRY(check_sky_sets(sky, &nsets));
    if (tiles == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no surface tiles (GrtSurfaceTiles_t is NULL).%s", "");
    }
    if (fluxes_dev == NULL && tiles->tile_fluxes_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "fluxes_dev and tile_fluxes_dev are both NULL: nothing to write.%s", "");
    }
    GrtAerosols_t a;
    GrtJoin join;
    GRT_TRY(sky_join(p, cols, sky, &a, &join));
    if (cols->num_levels != p->num_levels)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "columns of %d levels: this pipeline has %d.", cols->num_levels, p->num_levels);
    }
    GRT_TRY(grt_check_tiles(p, tiles, cols->ncol, join.tile_points));
    join.tiles = tiles;
    /* (the draws of a cloud set go through the subcolumn form, one draw included: the cloud form's doubles) */
    join.subcolumns = join.clouds != NULL ? sky->num_subcolumns : 0;
    GrtPass rows;
    rows_form(p, nsets, NULL, fluxes_dev, &rows);
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    return GRTCODE_SUCCESS;
}

/* one band's bins: none, or num_bins + 1 strictly increasing grid-point indices in 0 .. n - 1 of a band that is computed */
static int check_bins(GrtPipeline_t const *p, int bi, int const *edges, int num_bins, fp_t const *binned_dev)
{
    char const *name = bi == 0 ? "longwave" : "shortwave";
    if (num_bins > 0 && p->band[bi].gas == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s bins asked for, and this pipeline has no %s band.", num_bins, name, name);
    }
    GRT_TRY(grt_check_bin_edges(name, edges, num_bins, (long long)p->band[bi].n, binned_dev != NULL));
    return GRTCODE_SUCCESS;
}

/* grt_ext.h: the k-distributions of the bands' tau_gas -- each layer's own (keys NULL) or, correlated, every layer's under
   the map of its band's key.  The entry points alone: the checks of the classes, of a band's inputs and of a key, the
   tables and the launches are grt_kdist.c's. */
static int run_kdist(GrtPipeline_t *p, GrtColumns_t const *cols, GrtKdist_t const *kd, GrtKdistKey_t const *const *keys)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (kd == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no k-distribution inputs (GrtKdist_t is NULL).%s", "");
    }
    GRT_TRY(grt_kdist_check_classes(kd->num_classes, kd->class_edges));
    GrtKdistBand_t const *kb[2] = {&kd->lw, &kd->sw};
    long long const L = p->num_levels - 1;
    long long key_row[2] = {0, 0};
    for (int bi = 0; bi < 2; ++bi)
    {
        /* (a band's output: any of its three) */
        void const *out = kb[bi]->points_dev != NULL ? (void const *)kb[bi]->points_dev :
                          kb[bi]->weight_dev != NULL ? (void const *)kb[bi]->weight_dev : (void const *)kb[bi]->tau_dev;
        GRT_TRY(check_bins(p, bi, kb[bi]->edges, kb[bi]->num_bins, out));
        if (kb[bi]->num_bins > 0)
        {
            GRT_TRY(grt_kdist_check_band(bi == 0 ? "longwave" : "shortwave", kb[bi], (long long)p->band[bi].n));
            if (keys != NULL)
            {
                GRT_TRY(grt_kdist_check_key(bi == 0 ? "longwave" : "shortwave", keys[bi]->kind, keys[bi]->layer, L,
                                            &key_row[bi]));
            }
        }
    }
    if (kd->lw.num_bins + kd->sw.num_bins == 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no bins in either band: nothing to write.%s", "");
    }
    GRT_TRY(check_columns(p, cols));
    GRT_TRY(check_lane(p));
    /* (no solver runs: the columns' sun angles are not read) */
    GRT_TRY(stage_columns(p, cols, 1));
    for (int bi = 0; bi < 2; ++bi)
    {
        GrtBand *b = &p->band[bi];
        if (kb[bi]->num_bins == 0)
        {
            continue;                  /* (a band without bins is not computed: its line list is not touched) */
        }
        unsigned short *map = keys != NULL ? keys[bi]->map_dev : NULL;
        if (keys != NULL && map == NULL)
        {
            GrtScratch *own = &b->scratch[GRT_SCRATCH_KDIST_MAP];
            GRT_TRY(grt_scratch_need(p, own, ((size_t)p->max_cols*b->n + 3)/4, NULL));
            map = (unsigned short *)own->d;
        }
        /* the whole of tau, the spectral tables' part included (band_gas_optics leaves that to a solver) */
        GRT_TRY(grt_optical_depth_batch(b->gas, cols, b->tau_gas));
        b->tau_gas_lacks_tables = 0;
        b->last_cols = cols->ncol;
        if (keys == NULL)
        {
            GRT_TRY(grt_kdist_reduce(p->device, &b->kdist_table, b->tau_gas, cols->ncol*L, (long long)b->n,
                                     b->gas->grid.dw, kd->num_classes, kd->class_edges, kb[bi]));
        }
        else
        {
            GRT_TRY(grt_kdist_reduce_correlated(p->device, &b->kdist_table, b->tau_gas, cols->ncol, L, (long long)b->n,
                                                b->gas->grid.dw, kd->num_classes, kd->class_edges, key_row[bi], map,
                                                kb[bi]));
        }
    }
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_run_kdist(GrtPipeline_t *p, GrtColumns_t const *cols, GrtKdist_t const *kd)
{
    return run_kdist(p, cols, kd, NULL);
}

EXTERN int grt_pipeline_run_kdist_correlated(GrtPipeline_t *p, GrtColumns_t const *cols, GrtKdist_t const *kd,
                                             GrtKdistKeys_t const *keys)
{
    if (keys == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no keys (GrtKdistKeys_t is NULL): grt_pipeline_run_kdist is the call without them.%s", "");
    }
    GrtKdistKey_t const *const by_band[2] = {&keys->lw, &keys->sw};
    return run_kdist(p, cols, kd, by_band);
}

/* grt_ext.h: the fluxes of the correlated-k model on its g-classes.  Per band that has bins: run_kdist's gas optics, map
   and mapped reduction (grt_kdist.c), with the caller's map in place of the key's where one is given and pipeline scratch
   in place of the outputs the caller does not take; then the source sums, the solve and the bin sums
   (grt_pipeline_solve.c). */
EXTERN int grt_pipeline_run_ck_fluxes(GrtPipeline_t *p, GrtColumns_t const *cols, GrtCkFluxes_t const *ck)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (ck == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no correlated-k inputs (GrtCkFluxes_t is NULL).%s", "");
    }
    GrtCkBand_t const *cb[2] = {&ck->lw, &ck->sw};
    if (ck->class_edges != NULL)
    {
        GRT_TRY(grt_kdist_check_classes(ck->num_classes, ck->class_edges));
    }
    else if (ck->num_classes < 2 || ck->num_classes > GRT_KDIST_MAX_CLASSES)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d classes asked for: 2 to %d.", ck->num_classes, GRT_KDIST_MAX_CLASSES);
    }
    long long const L = p->num_levels - 1;
    long long key_row[2] = {0, 0};
    for (int bi = 0; bi < 2; ++bi)
    {
        char const *name = bi == 0 ? "longwave" : "shortwave";
        GrtCkBand_t const *c = cb[bi];
        GRT_TRY(check_bins(p, bi, c->edges, c->num_bins, c->flux_up_dev != NULL && c->flux_down_dev != NULL ? c->flux_up_dev : NULL));
        if (c->num_bins == 0)
        {
            continue;
        }
        if ((c->bin_up_dev != NULL) != (c->bin_down_dev != NULL))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%s %s is NULL and the other is not: both bin sums or neither.", name,
                     c->bin_up_dev == NULL ? "bin_up_dev" : "bin_down_dev");
        }
        if (c->map_given_dev == NULL)
        {
            if (ck->class_edges == NULL)
            {
                GRT_FAIL(GRTCODE_VALUE_ERR, "class_edges is NULL and the %s band is given no map: the class edges classify "
                         "its key.", name);
            }
            GRT_TRY(grt_kdist_check_key(name, c->key.kind, c->key.layer, L, &key_row[bi]));
        }
    }
    if (ck->lw.num_bins + ck->sw.num_bins == 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no bins in either band: nothing to write.%s", "");
    }
    GRT_TRY(check_two_levels(p));
    GRT_TRY(check_columns(p, cols));
    GRT_TRY(check_lane(p));
    /* (the sun angles are read where the shortwave is solved, and a night column is solved to zeros) */
    GRT_TRY(stage_columns(p, cols, ck->sw.num_bins > 0 ? GRT_SUN_MAY_BE_DOWN : 1));
    for (int bi = 0; bi < 2; ++bi)
    {
        GrtBand *b = &p->band[bi];
        GrtCkBand_t const *c = cb[bi];
        if (c->num_bins == 0)
        {
            continue;                  /* (a band without bins is not computed: its line list is not touched) */
        }
        size_t const classes = (size_t)p->max_cols*(size_t)c->num_bins*(size_t)ck->num_classes;
        size_t const source_rows = bi == 0 ? 2*(size_t)p->num_levels + 1 : 4;
        unsigned short *map = c->key.map_dev;
        if (c->map_given_dev == NULL && map == NULL)
        {
            GrtScratch *own = &b->scratch[GRT_SCRATCH_KDIST_MAP];
            GRT_TRY(grt_scratch_need(p, own, ((size_t)p->max_cols*b->n + 3)/4, NULL));
            map = (unsigned short *)own->d;
        }
        double *weight = c->weight_dev, *tau = c->tau_dev, *source = c->source_dev;
        if (weight == NULL)
        {
            GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_CK_WEIGHT], classes, NULL));
            weight = b->scratch[GRT_SCRATCH_CK_WEIGHT].d;
        }
        if (tau == NULL)
        {
            GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_CK_TAU], classes*(size_t)L, NULL));
            tau = b->scratch[GRT_SCRATCH_CK_TAU].d;
        }
        if (source == NULL)
        {
            GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_CK_SOURCE], classes*source_rows, NULL));
            source = b->scratch[GRT_SCRATCH_CK_SOURCE].d;
        }
        /* the whole of tau, the spectral tables' part included (band_gas_optics leaves that to a solver) */
        GRT_TRY(grt_optical_depth_batch(b->gas, cols, b->tau_gas));
        b->tau_gas_lacks_tables = 0;
        b->last_cols = cols->ncol;
        GrtKdistBand_t const sums = {.edges = c->edges, .num_bins = c->num_bins, .points_dev = c->points_dev,
                                     .weight_dev = weight, .tau_dev = tau};
        int const *edges_dev;
        GRT_TRY(grt_kdist_reduce_ck(p->device, &b->kdist_table, b->tau_gas, cols->ncol, L, (long long)b->n, b->gas->grid.dw,
                                    ck->num_classes, ck->class_edges, key_row[bi], c->map_given_dev, map, &sums, &edges_dev));
        GRT_TRY(grt_band_solve_ck(p, b, bi, cols->ncol, ck->num_classes, edges_dev,
                                  c->map_given_dev != NULL ? c->map_given_dev : map, weight, tau, source, c));
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
    GRT_TRY(check_columns(p, cols));
    if (cl != NULL)
    {
        GRT_TRY(check_clouds(p, cols, cl));
    }
    GrtBins const bins = {.spectral = spectral_dev, .binned = binned_dev, .edges = {lw_edges, sw_edges},
                          .num_bins = {lw_num_bins, sw_num_bins}};
    GrtJoin const join = {.clouds = cl};
    GrtPass rows;
    GRT_TRY(output_form(p, cl != NULL ? 2 : 1, NULL, fluxes_dev, &rows));
    rows.bins = &bins;
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_pipeline_band_profile_bin_limit(GrtPipeline_t const *p)
{
    if (p == NULL || p->num_levels < 1)
    {
        return 0;
    }
    /* the fused solvers' wave sums of one workgroup, 2 V rows x 2 waves x 8 bytes per bin, in 64 KiB of LDS */
    return 65536/(32*p->num_levels);
}

EXTERN int grt_pipeline_run_band_profiles(GrtPipeline_t *p, GrtColumns_t const *cols, GrtClouds_t const *cl,
                                          int const *lw_edges, int lw_num_bins, int const *sw_edges, int sw_num_bins,
                                          fp_t *band_levels_dev, fp_t *band_heating_dev)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(cols);
    if (band_levels_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "band_levels_dev is NULL: the level fluxes per bin are the output.%s", "");
    }
    GRT_TRY(check_bins(p, 0, lw_edges, lw_num_bins, band_levels_dev));
    GRT_TRY(check_bins(p, 1, sw_edges, sw_num_bins, band_levels_dev));
    if (lw_num_bins + sw_num_bins == 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no bins in either band: nothing to write.%s", "");
    }
    GRT_TRY(check_two_levels(p));
    int const *edges[2] = {lw_edges, sw_edges};
    int const num_bins[2] = {lw_num_bins, sw_num_bins};
    int const limit = grt_pipeline_band_profile_bin_limit(p);
    for (int bi = 0; bi < 2; ++bi)
    {
        int const most = num_bins[bi] > 0 ? grt_bin_block_max(edges[bi], num_bins[bi]) : 0;
        if (most > limit)
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s bins have a point in one block of 128 grid points: at most %d with %d levels "
                     "(grt_pipeline_band_profile_bin_limit).", most, bi == 0 ? "longwave" : "shortwave", limit,
                     p->num_levels);
        }
    }
    GRT_TRY(cl != NULL ? check_clouds(p, cols, cl) : check_columns(p, cols));
    int const sets = cl != NULL ? 2 : 1, V = p->num_levels;
    GrtBins const bins = {.edges = {lw_edges, sw_edges}, .num_bins = {lw_num_bins, sw_num_bins}};
    GrtJoin const join = {.clouds = cl};
    GrtPass const rows = {.profile = 1, .out = band_levels_dev, .bins = &bins, .sets = sets,
                          .out_stride = sets*2*(lw_num_bins + sw_num_bins)*V};
    GRT_TRY(pipeline_run(p, cols, &join, &rows));
    if (band_heating_dev != NULL)
    {
        void *s = grt_dev_stream(p->device);
        GRT_TIMED(s, GRT_TAG_BAND_PROFILES, "band heating rate kernel",
                  grt_launch_band_profile_finish(s, cols->ncol, sets, V, lw_num_bins, sw_num_bins, GRT_GRAVITY,
                                                 GRT_SPECIFIC_HEAT_AIR, p->small.d + p->off_p, band_levels_dev,
                                                 band_heating_dev));
    }
    return GRTCODE_SUCCESS;
}

/* what the object holds on demand, read from its bookkeeping (grt_ext.h): the members in the order
   grt_pipeline_internal.h declares them */
EXTERN int grt_debug_pipeline_holdings(GrtPipeline_t const *p, int *counts, uint64_t *scratch_doubles,
                                       uint64_t *staging_doubles, uint64_t *key_bytes)
{
    GRT_REQUIRE_PTR(p);
    GRT_REQUIRE_PTR(counts);
    GrtStaging const *const staging[] = {&p->small, &p->cloud, &p->aer, &p->surf, &p->zen, &p->rad, &p->tile, &p->zen_surf};
    int const num_staging = (int)(sizeof(staging)/sizeof(staging[0]));
    int num_tables = 0;
    for (int bi = 0; bi < 2; ++bi)
    {
        GrtBand const *b = &p->band[bi];
        size_t const held[] = {b->cloud_map.key != NULL ? b->cloud_map.key_bytes : 0,
                               b->aer_map.key != NULL ? b->aer_map.key_bytes : 0,
                               b->bin_table.key != NULL ? b->bin_table.key_bytes : 0,
                               b->kdist_table.key != NULL ? b->kdist_table.key_bytes : 0,
                               b->surf_map.key != NULL ? b->surf_map.key_bytes : 0,
                               b->channel_table.key != NULL ? b->channel_table.key_bytes : 0,
                               b->tile_map.key != NULL ? b->tile_map.key_bytes : 0,
                               b->response_table.key != NULL ? b->response_table.key_bytes : 0,
                               b->zen_surf_map.key != NULL ? b->zen_surf_map.key_bytes : 0};
        num_tables = (int)(sizeof(held)/sizeof(held[0]));
        for (int k = 0; k < num_tables && key_bytes != NULL; ++k)
        {
            key_bytes[bi*num_tables + k] = held[k];
        }
        for (int k = 0; k < GRT_SCRATCH_COUNT && scratch_doubles != NULL; ++k)
        {
            scratch_doubles[bi*GRT_SCRATCH_COUNT + k] = b->scratch[k].doubles;
        }
    }
    for (int k = 0; k < num_staging && staging_doubles != NULL; ++k)
    {
        staging_doubles[k] = staging[k]->doubles;
    }
    counts[0] = GRT_SCRATCH_COUNT;
    counts[1] = num_staging;
    counts[2] = num_tables;
    return GRTCODE_SUCCESS;
}
