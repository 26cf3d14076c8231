/* grt_pipeline_inputs.c -- what turns a caller's clouds, aerosols, surface and bin edges into device arguments of the batched
 * pipeline: the per-batch tables staged through pinned memory, and the per-point maps that depend only on band limits,
 * an aerosol grid or bin edges and are rebuilt when those change. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "grt_pipeline_internal.h"

/* The pinned buffer is reused every call: wait until the previous batch's copy of it has left -- not for its kernels, so
   that this batch is prepared on the host while that one runs.  A buffer of fewer than `need` doubles is replaced by one
   of `want` (sized for max_columns at this call's shape: a later batch of the same shape reuses it). */
int grt_staging_reserve(GrtPipeline_t *p, GrtStaging *st, size_t need, size_t want)
{
    GRT_TRY(grt_dev_event_wait(p->device, st->uploaded));
    if (need > st->doubles)
    {
        GRT_TRY(grt_dev_sync(p->device, grt_dev_stream(p->device)));
        grt_dev_free(p->device, st->d);
        grt_host_free_pinned(st->h);
        st->d = NULL;
        st->h = NULL;
        st->doubles = 0;
        GRT_TRY(grt_host_alloc_pinned((void **)&st->h, sizeof(double)*want));
        GRT_TRY(grt_dev_alloc(p->device, (void **)&st->d, sizeof(double)*want));
        st->doubles = want;
    }
    return GRTCODE_SUCCESS;
}

/* the first `need` doubles to the device on the library stream */
int grt_staging_upload(GrtPipeline_t *p, GrtStaging *st, size_t need)
{
    void *s = grt_dev_stream(p->device);
    GRT_TRY(grt_dev_upload(p->device, st->d, st->h, sizeof(double)*need, s));
    GRT_TRY(grt_dev_event_record(p->device, &st->uploaded, s));
    return GRTCODE_SUCCESS;
}

void grt_staging_free(GrtPipeline_t *p, GrtStaging *st)
{
    grt_dev_free(p->device, st->d);
    grt_host_free_pinned(st->h);
    grt_dev_event_destroy(p->device, &st->uploaded);
}

/* The sun angles of a batch (grt_pipeline_run_zeniths) into p->zen and onto the device: the cosines [C][Z], the weights
   [C][Z] if given, and the cosines angle-major [Z][C] for the materialised form's loop over the angles, where a night
   sample stands as its column's last day angle before it, else its first one after it, else 1 (the solver then has a
   sun to solve for; the mean kernel zeroes the sample) */
int grt_stage_zeniths(GrtPipeline_t *p, GrtZeniths_t const *zn, int C, GrtZenithRun *zr)
{
    size_t const Z = (size_t)zn->num_zeniths, n = (size_t)C*Z;
    memset(zr, 0, sizeof(*zr));
    GRT_TRY(grt_staging_reserve(p, &p->zen, 3*n, 3*(size_t)p->max_cols*GRT_MAX_ZENITHS));
    double *h = p->zen.h;
    memcpy(h, zn->cos_zenith, sizeof(double)*n);
    if (zn->weight != NULL)
    {
        memcpy(h + n, zn->weight, sizeof(double)*n);
    }
    else
    {
        memset(h + n, 0, sizeof(double)*n);
    }
    for (size_t c = 0; c < (size_t)C; ++c)
    {
        double const *mu = zn->cos_zenith + c*Z;
        double stand_in = 1.;
        for (size_t k = Z; k-- > 0;)
        {
            stand_in = mu[k] > 0. ? mu[k] : stand_in;        /* (ends as the column's first day angle) */
        }
        for (size_t k = 0; k < Z; ++k)
        {
            stand_in = mu[k] > 0. ? mu[k] : stand_in;
            h[2*n + k*(size_t)C + c] = stand_in;
        }
    }
    GRT_TRY(grt_staging_upload(p, &p->zen, 3*n));
    zr->zeniths = zn->num_zeniths;
    zr->mu = p->zen.d;
    zr->weight = zn->weight != NULL ? p->zen.d + n : NULL;
    zr->mu_by_angle = p->zen.d + 2*n;
    return GRTCODE_SUCCESS;
}

/* grt_pipeline_run_sky_radiances' checks of the viewing angles of a batch of C columns: how many, and every secant finite
   and at least 1 (nothing is touched) */
int grt_check_radiances(GrtRadiances_t const *rd, int C)
{
    if (rd->num_angles < 1 || rd->num_angles > GRT_MAX_VIEW_ANGLES)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d viewing angles per column asked for: 1 to %d.", rd->num_angles, GRT_MAX_VIEW_ANGLES);
    }
    if (rd->view_secant == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "view_secant is NULL: the viewing secants [ncol][%d] are the input.", rd->num_angles);
    }
    size_t const n = (size_t)C*(size_t)rd->num_angles;
    for (size_t k = 0; k < n; ++k)
    {
        /* (a NaN fails the first comparison, an infinity the second) */
        if (!(rd->view_secant[k] >= 1.) || !(rd->view_secant[k] <= 1.79769313486231570815e+308))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "secant of viewing angle %zu of column %zu (%e) is NaN, infinite or below 1.",
                     k % (size_t)rd->num_angles, k/(size_t)rd->num_angles, rd->view_secant[k]);
        }
    }
    return GRTCODE_SUCCESS;
}

/* The viewing secants of a batch (grt_pipeline_run_sky_radiances) into p->rad and onto the device, [C][A] */
int grt_stage_radiances(GrtPipeline_t *p, GrtRadiances_t const *rd, int C, GrtRadianceRun *rr)
{
    size_t const n = (size_t)C*(size_t)rd->num_angles;
    GRT_TRY(grt_staging_reserve(p, &p->rad, n, (size_t)p->max_cols*GRT_MAX_VIEW_ANGLES));
    memcpy(p->rad.h, rd->view_secant, sizeof(double)*n);
    GRT_TRY(grt_staging_upload(p, &p->rad, n));
    rr->angles = rd->num_angles;
    rr->secant = p->rad.d;
    rr->integrated = rd->radiances_dev;
    rr->spectral = rd->spectral_radiances_dev;
    rr->brightness = rd->brightness_dev;
    return GRTCODE_SUCCESS;
}

/* a key given as parts that lie apart in the caller's memory: compared in place, copied only when the table is rebuilt */
typedef struct GrtKeyPart { void const *bytes; size_t n; } GrtKeyPart;

/* t->table for the key `parts`, taken one after the other: as it is when it was built for the same bytes, else `ints` ints
   written by fill(ctx, .) on the host and uploaded.  The stored key is dropped before the device table is touched and set
   again only when the whole call succeeded, so a failure half way leaves a table that the next call rebuilds, whatever its
   key. */
static int grt_keyed_table_parts(GrtPipeline_t *p, GrtKeyedTable *t, GrtKeyPart const *parts, int nparts, size_t ints,
                                 GrtTableFill fill, void *ctx)
{
    size_t key_bytes = 0;
    for (int k = 0; k < nparts; ++k)
    {
        key_bytes += parts[k].n;
    }
    if (t->key != NULL && t->key_bytes == key_bytes)
    {
        char const *at = t->key;
        int same = 1;
        for (int k = 0; k < nparts && same; at += parts[k].n, ++k)
        {
            same = parts[k].n == 0 || memcmp(at, parts[k].bytes, parts[k].n) == 0;
        }
        if (same)
        {
            return GRTCODE_SUCCESS;
        }
    }
    void *new_key = malloc(key_bytes);
    int *host = malloc(sizeof(int)*ints);
    if (new_key == NULL || host == NULL)
    {
        free(new_key);
        free(host);
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for a table of %zu ints.", ints);
    }
    int rc = fill(ctx, host);
    if (rc == GRTCODE_SUCCESS)
    {
        char *to = new_key;
        for (int k = 0; k < nparts; to += parts[k].n, ++k)
        {
            if (parts[k].n > 0)
            {
                memcpy(to, parts[k].bytes, parts[k].n);
            }
        }
        free(t->key);
        t->key = NULL;
        void *s = grt_dev_stream(p->device);
        /* (the last batch's kernels may still read the old table; then host is freed: wait both times) */
        rc = grt_dev_sync(p->device, s);
        if (rc == GRTCODE_SUCCESS)
        {
            /* (its size may depend on the key: grt_bin_table_ints) */
            grt_dev_free(p->device, t->table);
            t->table = NULL;
            rc = grt_dev_alloc(p->device, (void **)&t->table, sizeof(int)*ints);
        }
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_upload(p->device, t->table, host, sizeof(int)*ints, s);
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(p->device, s);
    }
    free(host);
    if (rc != GRTCODE_SUCCESS)
    {
        free(new_key);
        GRT_TRY(rc);
    }
    t->key = new_key;
    t->key_bytes = key_bytes;
    return GRTCODE_SUCCESS;
}

/* ... for a key in one piece */
static int grt_keyed_table(GrtPipeline_t *p, GrtKeyedTable *t, void const *key, size_t key_bytes, size_t ints,
                           GrtTableFill fill, void *ctx)
{
    GrtKeyPart const part = {key, key_bytes};
    return grt_keyed_table_parts(p, t, &part, 1, ints, fill, ctx);
}

void grt_keyed_table_free(GrtPipeline_t *p, GrtKeyedTable *t)
{
    grt_dev_free(p->device, t->table);
    free(t->key);
}

/* how many of the ascending w [n] are < target (or_equal: <= target): the first index whose value is >= target (n if
   none); or_equal, one more than the last index whose value is <= target */
static int count_below(double const *w, int n, double target, int or_equal)
{
    int lo = 0, hi = n;
    while (lo < hi)
    {
        int const mid = (lo + hi)/2;
        if (w[mid] < target || (or_equal && w[mid] == target)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

/* The band each point of w [n] ends up with when bands 0 .. nb - 1 of a parametrisation of `own` bands are written in
   order, as optics_utils.c:118-169 writes them: [first >= lo, last <= hi), band 0 extended down, band own - 1 up. */
void grt_cloud_band_map(double const *lo, double const *hi, int own, int nb, double const *w, int n, int *idx)
{
    for (int j = 0; j < n; ++j)
    {
        idx[j] = -1;
    }
    for (int b = 0; b < nb; ++b)
    {
        int const from = count_below(w, n, lo[b], 0);
        int const upto = count_below(w, n, hi[b], 1) - 1;
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

typedef struct CloudMapFill { GrtClouds_t const *cl; SpectralGrid_t const *grid; } CloudMapFill;

static int fill_cloud_map(void *ctx, int *idx)
{
    CloudMapFill const *f = ctx;
    SpectralGrid_t const *grid = f->grid;
    int const n = (int)grid->n, B = f->cl->num_liquid_bands;
    double *w = malloc(sizeof(double)*grid->n);
    if (w == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for the band limits of %d grid points.", n);
    }
    /* what driver.c:476-488 passes to cloud_optics as the grid's "wavenumbers": band limits, not centres */
    for (uint64_t j = 1; j < grid->n; ++j)
    {
        w[j] = 0.5*((grid->w0 + (j - 1)*grid->dw) + (grid->w0 + j*grid->dw));
    }
    w[0] = grid->w0 - grid->dw;
    if (w[0] < 0.)
    {
        w[0] = 0;
    }
    grt_cloud_band_map(f->cl->liquid_band_lo, f->cl->liquid_band_hi, B, B, w, n, idx);
    grt_cloud_band_map(f->cl->ice_band_lo, f->cl->ice_band_hi, f->cl->num_ice_bands, B, w, n, idx + n);
    free(w);
    return GRTCODE_SUCCESS;
}

/* the band's cloud arguments for a batch of C columns of S subcolumns staged by grt_stage_clouds: its per-point cloud
   bands for these band limits are built on the host when the limits differ from the last call's */
int grt_band_clouds(GrtPipeline_t *p, GrtBand *b, int bi, GrtClouds_t const *cl, int C, int S, GrtCloudArgs *ca)
{
    int const B = cl->num_liquid_bands, NI = cl->num_ice_bands;
    size_t const L = (size_t)p->num_levels - 1, set = (size_t)S*(size_t)C*3*(size_t)B*L;
    ca->num_bands = B;
    ca->thickness = p->cloud.d;
    ca->liquid = p->cloud.d + (size_t)C*L + (size_t)(2*bi)*set;
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
    CloudMapFill f = {cl, &b->gas->grid};
    int const rc = grt_keyed_table(p, &b->cloud_map, key, sizeof(double)*nkey, 2*(size_t)b->n, fill_cloud_map, &f);
    free(key);
    GRT_TRY(rc);
    ca->band_liquid = b->cloud_map.table;
    ca->band_ice = b->cloud_map.table + b->n;
    return GRTCODE_SUCCESS;
}

/* the band tables of the batch to the device: [C][L] thickness, then the four sets, each [S][C][3][B][L] -- the caller's
   [C][S][3][B][L] subcolumn-major, so that subcolumn s of every column is one [C][3][B][L] block (S = 1: as given) */
int grt_stage_clouds(GrtPipeline_t *p, GrtClouds_t const *cl, int C, int S)
{
    size_t const L = (size_t)p->num_levels - 1, B = (size_t)cl->num_liquid_bands, tab = 3*B*L;
    size_t const set = (size_t)S*(size_t)C*tab, need = (size_t)C*L + 4*set;
    GRT_TRY(grt_staging_reserve(p, &p->cloud, need, (size_t)p->max_cols*L*(1 + 12*B*(size_t)S)));
    double *h = p->cloud.h;
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
    GRT_TRY(grt_staging_upload(p, &p->cloud, need));
    return GRTCODE_SUCCESS;
}

/* grt_stage_clouds for tables that are made on the device: the same buffer and layout, but only the thickness [C][L] is
   uploaded; the sampler's kernel writes the four [S][C][3][B][L] sets behind it from the cloud fields (which it stages
   itself), on the pipeline's lane and so ahead of the solvers that read them */
int grt_stage_cloud_fields(GrtPipeline_t *p, GrtClouds_t const *cl, GrtCloudSampler_t *sampler, GrtCloudFields_t const *fields,
                           fp_t const *temperature, int C, int S)
{
    size_t const L = (size_t)p->num_levels - 1, B = (size_t)cl->num_liquid_bands, tab = 3*B*L;
    size_t const set = (size_t)S*(size_t)C*tab, need = (size_t)C*L + 4*set;
    GRT_TRY(grt_staging_reserve(p, &p->cloud, need, (size_t)p->max_cols*L*(1 + 12*B*(size_t)S)));
    memcpy(p->cloud.h, cl->thickness, sizeof(double)*(size_t)C*L);
    GRT_TRY(grt_staging_upload(p, &p->cloud, (size_t)C*L));
    GRT_TRY(grt_cloud_sampler_enqueue(sampler, fields, temperature, p->cloud.d + (size_t)C*L));
    return GRTCODE_SUCCESS;
}

/* ---- piecewise linear on a grid of the caller's own: the aerosol optics and the surface ------------------------------- */

/* One band's input: no points, or at least two strictly increasing ones with values on them.  The messages call it `name`
   + `kind`, and say what no points stand for (`none`) and what the values are (`what`). */
int grt_check_grid(char const *name, char const *kind, char const *none, char const *what, int nx, fp_t const *grid,
                   fp_t const *values)
{
    if (nx < 0 || nx == 1)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s%s grid points: 0 (%s) or at least 2.", nx, name, kind, none);
    }
    if (nx == 0)
    {
        return GRTCODE_SUCCESS;
    }
    if (grid == NULL || values == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s%s grid points with a NULL grid or NULL %s.", nx, name, kind, what);
    }
    for (int j = 0; j + 1 < nx; ++j)
    {
        if (!(grid[j + 1] > grid[j]))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%s%s grid not strictly increasing (grid[%d] = %e, grid[%d] = %e).", name, kind, j,
                     grid[j], j + 1, grid[j + 1]);
        }
    }
    return GRTCODE_SUCCESS;
}

/* Where each of the n points w0 + i dw lies in the grid x [nx] (strictly increasing), as interpolate2
   (utilities.c:149-222) assigns them: k = 1 + j with x[j] < w <= x[j+1], 0 for w <= x[0], nx for w > x[nx-1].  ends: the
   map is k, the two ranges outside the grid being entries of their own (constant_extrapolation, utilities.c:77-92);
   else it is the interval j, and -1 outside the grid, which the reference does not write there. */
static void grid_map(double w0, double dw, uint64_t n, double const *x, int nx, int ends, int *map)
{
    for (uint64_t i = 0; i < n; ++i)
    {
        int const k = count_below(x, nx, w0 + i*dw, 0);
        map[i] = ends ? k : (k == 0 || k == nx ? -1 : k - 1);
    }
}

/* linear_sample's (utilities.c:235-246) slope and intercept of the interval from point j to point j + 1 */
static inline void linear_pair(double const *x, double const *y, size_t j, double *slope, double *intercept)
{
    double const m = (y[j + 1] - y[j])/(x[j + 1] - x[j]);
    double const b = y[j] - m*x[j];
    *slope = m;
    *intercept = b;
}

/* a band's map for the grid x, as grt_keyed_table fills it */
typedef struct GridMapFill { SpectralGrid_t const *grid; double const *x; int nx, ends; } GridMapFill;

static int fill_grid_map(void *ctx, int *map)
{
    GridMapFill const *f = ctx;
    grid_map(f->grid->w0, f->grid->dw, f->grid->n, f->x, f->nx, f->ends, map);
    return GRTCODE_SUCCESS;
}

/* The interval of the aerosol grid x [na] each of the n points lies in: j with x[j] < w <= x[j+1]; -1 for w <= x[0] and
   for w > x[na-1]. */
void grt_aerosol_interval_map(double w0, double dw, uint64_t n, double const *x, int na, int *interval)
{
    grid_map(w0, dw, n, x, na, 0, interval);
}

/* the slope and intercept of every interval, layer and property of ncol columns:
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
                linear_pair(x, y, j, &tables[((cp*NI + j)*2 + 0)*L + l], &tables[((cp*NI + j)*2 + 1)*L + l]);
            }
        }
    }
}

/* the batch's slope and intercept tables to the device: the longwave's [C][3][NA - 1][2][L], then the shortwave's (a band
   the pipeline does not have, or one given no aerosol, takes no room) */
int grt_stage_aerosols(GrtPipeline_t *p, GrtAerosols_t const *ae, int C)
{
    size_t const L = (size_t)p->num_levels - 1;
    size_t per[2], need = 0, want = 0;
    for (int bi = 0; bi < 2; ++bi)
    {
        int const na = p->band[bi].gas != NULL ? grt_aerosol_points(ae, bi) : 0;
        per[bi] = na > 0 ? 6*L*((size_t)na - 1) : 0;
        need += (size_t)C*per[bi];
        want += (size_t)p->max_cols*per[bi];
    }
    if (need == 0)
    {
        return GRTCODE_SUCCESS;
    }
    GRT_TRY(grt_staging_reserve(p, &p->aer, need, want));
    if (per[0] > 0)
    {
        grt_aerosol_tables(ae->lw_grid, ae->lw_num_points, C, (int)L, ae->lw_optics, p->aer.h);
    }
    if (per[1] > 0)
    {
        grt_aerosol_tables(ae->sw_grid, ae->sw_num_points, C, (int)L, ae->sw_optics, p->aer.h + (size_t)C*per[0]);
    }
    GRT_TRY(grt_staging_upload(p, &p->aer, need));
    return GRTCODE_SUCCESS;
}

/* the band's aerosol arguments for a batch of C columns staged by grt_stage_aerosols: its per-point intervals are built on
   the host when the band's aerosol grid differs from the last call's */
int grt_band_aerosols(GrtPipeline_t *p, GrtBand *b, int bi, GrtAerosols_t const *ae, int C, GrtAerosolArgs *aa)
{
    int const na = grt_aerosol_points(ae, bi);
    size_t const L = (size_t)p->num_levels - 1;
    int const na_lw = p->band[0].gas != NULL ? ae->lw_num_points : 0;
    aa->num_intervals = na - 1;
    aa->tables = p->aer.d + (bi == 1 && na_lw > 0 ? (size_t)C*6*L*((size_t)na_lw - 1) : 0);
    GridMapFill f = {&b->gas->grid, bi == 0 ? ae->lw_grid : ae->sw_grid, na, 0};
    GRT_TRY(grt_keyed_table(p, &b->aer_map, f.x, sizeof(double)*(size_t)na, b->n, fill_grid_map, &f));
    aa->interval = b->aer_map.table;
    return GRTCODE_SUCCESS;
}

/* The entry of the surface grid x [ns] each of the n points takes: 0 for w <= x[0], 1 + j for x[j] < w <= x[j+1], ns for
   w > x[ns-1]. */
void grt_surface_entry_map(double w0, double dw, uint64_t n, double const *x, int ns, int *entry)
{
    grid_map(w0, dw, n, x, ns, 1, entry);
}

/* values [ncol][ns] -> tables [ncol][ns + 1][2], slope then intercept: entry 0 the constant y[0] below the grid, entry
   1 + j the pair of interval j, entry ns the constant above the grid -- y[ns-2], what
   the reference's extrapolation takes from the last SEGMENT it is handed (utilities.c:215-219).  A constant entry has
   slope 0: 0 w + b is b. */
void grt_surface_tables(double const *x, int ns, int ncol, double const *values, double *tables)
{
    size_t const NS = (size_t)ns, NE = NS + 1;
    for (size_t c = 0; c < (size_t)ncol; ++c)
    {
        double const *y = values + c*NS;
        double *t = tables + c*NE*2;
        t[0] = 0.;
        t[1] = y[0];
        for (size_t j = 0; j + 1 < NS; ++j)
        {
            linear_pair(x, y, j, &t[(1 + j)*2 + 0], &t[(1 + j)*2 + 1]);
        }
        t[NS*2 + 0] = 0.;
        t[NS*2 + 1] = y[NS - 2];
    }
}

/* one band's surface inputs: none, or at least two strictly increasing grid points and knot values in [0, 1] */
static int check_surface_band(char const *name, int ns, int ncol, fp_t const *grid, fp_t const *values, fp_t const *second)
{
    GRT_TRY(grt_check_grid(name, "", "the creation-time array", "values", ns, grid, values));
    fp_t const *arrays[2] = {values, second};
    for (int k = 0; k < 2 && ns > 0; ++k)
    {
        for (size_t i = 0; arrays[k] != NULL && i < (size_t)ncol*(size_t)ns; ++i)
        {
            if (!(arrays[k][i] >= 0. && arrays[k][i] <= 1.))
            {
                GRT_FAIL(GRTCODE_VALUE_ERR, "%s value %e of column %zu, point %zu outside [0, 1].", name, arrays[k][i],
                         i/(size_t)ns, i%(size_t)ns);
            }
        }
    }
    return GRTCODE_SUCCESS;
}

/* what grt_pipeline_set_surface refuses; np: the points each band takes (0: a band the pipeline does not have, or one that
   keeps its creation-time array) */
int grt_check_surface(GrtPipeline_t const *p, GrtSurface_t const *sf, int np[2])
{
    if (sf->ncol < 1 || sf->ncol > p->max_cols)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "a surface of %d columns, this pipeline was created for 1 to %d.", sf->ncol, p->max_cols);
    }
    np[0] = p->band[0].gas != NULL ? sf->emissivity_num_points : 0;
    np[1] = p->band[1].gas != NULL ? sf->albedo_num_points : 0;
    GRT_TRY(check_surface_band("surface emissivity", np[0], sf->ncol, sf->emissivity_grid, sf->emissivity, NULL));
    GRT_TRY(check_surface_band("surface albedo", np[1], sf->ncol, sf->albedo_grid, sf->direct_albedo, sf->diffuse_albedo));
    return GRTCODE_SUCCESS;
}

/* The three arrays of a surface, by band: values[k] is emissivity, direct albedo, diffuse albedo where band k > 0 takes
   points (np) and the array is given, else NULL.  Returns the doubles their slope and intercept entries take per row. */
static size_t surface_arrays(int const np[2], fp_t const *emissivity, fp_t const *direct, fp_t const *diffuse,
                             fp_t const *values[3])
{
    values[0] = np[0] > 0 ? emissivity : NULL;
    values[1] = np[1] > 0 ? direct : NULL;
    values[2] = np[1] > 0 ? diffuse : NULL;
    size_t per = 0;
    for (int k = 0; k < 3; ++k)
    {
        per += values[k] != NULL ? 2*((size_t)np[k > 0] + 1) : 0;
    }
    return per;
}

/* `rows` rows of a surface (surface_arrays' values on grid[band]) to the device through st, which the caller reserved for
   `front` doubles of its own, written already, and the rows' entries behind them: the entries (grt_surface_tables), array
   after array, the upload, and per array the band's per-point entry map -- its tile_map (tiles) or surf_map, built
   when the grid differs from the last call's --, `cap` rows of scratch (id[1]: the diffuse albedo's, id[0]: the others') and
   the launch that writes the rows there (GRT_TAG_SURFACE). */
static int stage_surface_rows(GrtPipeline_t *p, GrtStaging *st, int tiles, int const id[2], size_t rows, size_t cap,
                              fp_t const *const grid[2], int const np[2], fp_t const *const values[3], size_t front)
{
    size_t off[3], need = front;
    for (int k = 0; k < 3; ++k)
    {
        off[k] = need;
        if (values[k] != NULL)
        {
            grt_surface_tables(grid[k > 0], np[k > 0], (int)rows, values[k], st->h + off[k]);
            need += rows*2*((size_t)np[k > 0] + 1);
        }
    }
    GRT_TRY(grt_staging_upload(p, st, need));
    void *s = grt_dev_stream(p->device);
    for (int k = 0; k < 3; ++k)
    {
        if (values[k] == NULL)
        {
            continue;
        }
        GrtBand *b = &p->band[k > 0];
        GrtKeyedTable *map = tiles ? &b->tile_map : &b->surf_map;
        SpectralGrid_t const *g = &b->gas->grid;
        GridMapFill f = {g, grid[k > 0], np[k > 0], 1};
        GRT_TRY(grt_keyed_table(p, map, f.x, sizeof(double)*(size_t)f.nx, b->n, fill_grid_map, &f));
        GrtScratch *out = &b->scratch[id[k == 2]];
        GRT_TRY(grt_scratch_need(p, out, cap*b->n, NULL));
        GrtSurfaceArgs const sa = {f.nx + 1, map->table, st->d + off[k]};
        int const slot = grt_profile_begin(s, GRT_TAG_SURFACE);
        int const krc = grt_launch_spread_surface(s, (int)rows, g->w0, g->dw, b->n, &sa, out->d);
        grt_profile_end(s, slot);
        GRT_TRY(grt_dev_check(krc, "surface row kernel"));
    }
    return GRTCODE_SUCCESS;
}

/* A checked surface (grt_check_surface's np) to the device: the columns' rows, stage_surface_rows into the bands'
   GRT_SCRATCH_SURF_ROWS(_DIF) through their surf_map.  The bands' surf_set / surf_dif_set say what is in force afterwards;
   the caller sets them when this has succeeded. */
int grt_stage_surface(GrtPipeline_t *p, GrtSurface_t const *sf, int const np[2])
{
    size_t const C = (size_t)sf->ncol, M = (size_t)p->max_cols;
    fp_t const *values[3], *const grid[2] = {sf->emissivity_grid, sf->albedo_grid};
    size_t const per = surface_arrays(np, sf->emissivity, sf->direct_albedo, sf->diffuse_albedo, values);
    int const id[2] = {GRT_SCRATCH_SURF_ROWS, GRT_SCRATCH_SURF_ROWS_DIF};
    if (per == 0)
    {
        return GRTCODE_SUCCESS;
    }
    GRT_TRY(grt_staging_reserve(p, &p->surf, C*per, M*per));
    return stage_surface_rows(p, &p->surf, 0, id, C, M, grid, np, values, 0);
}

/* ---- surface tiles (grt_pipeline_run_sky_tiles) ---- */

/* What grt_pipeline_run_sky_tiles refuses in its tiles for a batch of C columns, the output pointers apart (nothing is
   touched): the tile count, the surface's rules for grids, counts and knot values on C x T rows, the temperatures of a
   pipeline with a longwave band, the fractions.  np: the knots each band takes (0: a band the pipeline does not have, or
   one whose tiles all take the surface in force). */
int grt_check_tiles(GrtPipeline_t const *p, GrtSurfaceTiles_t const *tl, int C, int np[2])
{
    if (tl->num_tiles < 1 || tl->num_tiles > GRT_MAX_TILES)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d surface tiles per column asked for: 1 to %d.", tl->num_tiles, GRT_MAX_TILES);
    }
    int const rows = C*tl->num_tiles;
    np[0] = p->band[0].gas != NULL ? tl->num_emissivity_points : 0;
    np[1] = p->band[1].gas != NULL ? tl->num_albedo_points : 0;
    GRT_TRY(check_surface_band("tile emissivity", np[0], rows, tl->emissivity_grid, tl->emissivity, NULL));
    GRT_TRY(check_surface_band("tile albedo", np[1], rows, tl->albedo_grid, tl->direct_albedo, tl->diffuse_albedo));
    if (p->band[0].gas != NULL)
    {
        if (tl->surface_temperature == NULL)
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "surface_temperature is NULL: the tiles' temperatures [ncol][%d] are the input of "
                     "the longwave band.", tl->num_tiles);
        }
        for (int k = 0; k < rows; ++k)
        {
            /* (a NaN fails the comparison) */
            if (!(tl->surface_temperature[k] >= MIN_TEMPERATURE && tl->surface_temperature[k] <= MAX_TEMPERATURE))
            {
                GRT_FAIL(GRTCODE_VALUE_ERR, "temperature of tile %d of column %d (%e) is NaN or outside %g .. %g.",
                         k % tl->num_tiles, k/tl->num_tiles, tl->surface_temperature[k], (double)MIN_TEMPERATURE,
                         (double)MAX_TEMPERATURE);
            }
        }
    }
    for (int k = 0; k < rows && tl->fraction != NULL; ++k)
    {
        if (!(tl->fraction[k] >= 0.))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "fraction of tile %d of column %d (%e) is negative or NaN.", k % tl->num_tiles,
                     k/tl->num_tiles, tl->fraction[k]);
        }
    }
    return GRTCODE_SUCCESS;
}

/* Checked tiles (grt_check_tiles' np) to the device, as grt_stage_surface brings a surface there: the temperatures [C T]
   and [T][C] and the fractions in front, then the C x T rows, stage_surface_rows into the bands' GRT_SCRATCH_TILE_ROWS(_DIF)
   through a map of the tiles' own (tile_map).  The surface in force and its rows are not touched. */
int grt_stage_tiles(GrtPipeline_t *p, GrtSurfaceTiles_t const *tl, int C, int const np[2], GrtTileRun *tr)
{
    size_t const T = (size_t)tl->num_tiles, R = (size_t)C*T, M = (size_t)p->max_cols*T;
    fp_t const *values[3], *const grid[2] = {tl->emissivity_grid, tl->albedo_grid};
    size_t const per = surface_arrays(np, tl->emissivity, tl->direct_albedo, tl->diffuse_albedo, values);
    int const id[2] = {GRT_SCRATCH_TILE_ROWS, GRT_SCRATCH_TILE_ROWS_DIF};
    GRT_TRY(grt_staging_reserve(p, &p->tile, R*(3 + per), M*(3 + per)));
    double *h = p->tile.h;
    for (size_t k = 0; k < R; ++k)
    {
        double const ts = tl->surface_temperature != NULL && p->band[0].gas != NULL ? tl->surface_temperature[k] : 0.;
        h[k] = ts;
        h[R + (k % T)*(size_t)C + k/T] = ts;
        h[2*R + k] = tl->fraction != NULL ? tl->fraction[k] : 0.;
    }
    GRT_TRY(stage_surface_rows(p, &p->tile, 1, id, R, M, grid, np, values, 3*R));
    tr->tiles = tl->num_tiles;
    tr->t_surf = p->tile.d;
    tr->t_surf_by_tile = p->tile.d + R;
    tr->fraction = tl->fraction != NULL ? p->tile.d + 2*R : NULL;
    tr->np[0] = np[0];
    tr->np[1] = np[1];
    tr->dif = values[2] != NULL;
    tr->per_tile = tl->tile_fluxes_dev;
    return GRTCODE_SUCCESS;
}

/* ---- a direct-beam albedo per sun angle (grt_pipeline_run_sky_zeniths_direct) ---- */

/* grt_ext.h: grt_surface_tables over the ncol x zeniths knot rows, and the same pairs angle-major where asked for */
EXTERN void grt_zenith_surface_tables(fp_t const *x, int ns, int ncol, int zeniths, fp_t const *values, fp_t *tables,
                                      fp_t *by_angle)
{
    size_t const Z = (size_t)zeniths, C = (size_t)ncol, per = 2*((size_t)ns + 1);
    grt_surface_tables(x, ns, ncol*zeniths, values, tables);
    for (size_t r = 0; by_angle != NULL && r < C*Z; ++r)
    {
        memcpy(by_angle + ((r % Z)*C + r/Z)*per, tables + r*per, sizeof(double)*per);
    }
}

/* What grt_pipeline_run_sky_zeniths_direct refuses in its surface for a batch of C columns under Z angles (nothing is
   touched): fewer than two knots, a NULL grid or albedo array, a grid that is not strictly increasing, a knot of any
   (column, angle) -- a night angle's too -- outside [0, 1] or not finite. */
int grt_check_zenith_surface(GrtZenithSurface_t const *zs, int C, int Z)
{
    if (zs->albedo_num_points < 2)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d knots of the per-angle direct albedo: at least 2.", zs->albedo_num_points);
    }
    GRT_TRY(check_surface_band("per-angle direct albedo", zs->albedo_num_points, C*Z, zs->albedo_grid, zs->direct_albedo,
                               NULL));
    return GRTCODE_SUCCESS;
}

/* A checked surface to the device, as grt_stage_surface brings a column's there: the C x Z knot rows' slope and intercept
   entries (grt_surface_tables) -- column-major for the fused form's join, angle-major for the materialised form's loop --
   and the shortwave band's per-point entries (grt_surface_entry_map; built when the grid differs from the last call's).
   No rows are written here, and the surface in force is not touched. */
int grt_stage_zenith_surface(GrtPipeline_t *p, GrtZenithSurface_t const *zs, int C, GrtZenithRun *zr)
{
    GrtBand *b = &p->band[1];
    int const ns = zs->albedo_num_points;
    size_t const per = 2*((size_t)ns + 1), rows = (size_t)C*(size_t)zr->zeniths;
    /* (both layouts are staged; the form in use is uploaded) */
    GRT_TRY(grt_staging_reserve(p, &p->zen_surf, 2*rows*per, 2*(size_t)p->max_cols*GRT_MAX_ZENITHS*per));
    grt_zenith_surface_tables(zs->albedo_grid, ns, C, zr->zeniths, zs->direct_albedo, p->zen_surf.h, p->zen_surf.h + rows*per);
    if (p->keep_spectra)
    {
        memcpy(p->zen_surf.h, p->zen_surf.h + rows*per, sizeof(double)*rows*per);
    }
    GRT_TRY(grt_staging_upload(p, &p->zen_surf, rows*per));
    GridMapFill f = {&b->gas->grid, zs->albedo_grid, ns, 1};
    GRT_TRY(grt_keyed_table(p, &b->zen_surf_map, f.x, sizeof(double)*(size_t)ns, b->n, fill_grid_map, &f));
    zr->surface.num_entries = ns + 1;
    zr->surface.entry = b->zen_surf_map.table;
    zr->surface.tables = p->zen_surf.d;
    return GRTCODE_SUCCESS;
}

/* ---- a sun cosine per layer for the direct beam (grt_pipeline_run_sky_zeniths_slant) ---- */

/* grt_ext.h: the layer cosines of the straight ray that reaches the column's lowest level */
EXTERN int grt_slant_cosines(double radius_m, int ncol, int num_levels, int num_zeniths, double const *height_m,
                             double const *cos_zenith, double *layer_cos_zenith)
{
    GRT_REQUIRE_PTR(height_m);
    GRT_REQUIRE_PTR(cos_zenith);
    GRT_REQUIRE_PTR(layer_cos_zenith);
    if (!(radius_m >= 0.) || !isfinite(radius_m))
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "planet radius %e m: finite and at least 0 (0: a flat planet).", radius_m);
    }
    if (ncol < 1 || num_levels < 2 || num_zeniths < 1)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d columns of %d levels under %d angles: at least 1, 2 and 1.", ncol, num_levels,
                 num_zeniths);
    }
    size_t const C = (size_t)ncol, V = (size_t)num_levels, L = V - 1, Z = (size_t)num_zeniths;
    for (size_t c = 0; c < C; ++c)
    {
        double const *h = height_m + c*V;
        for (size_t j = 0; j < V; ++j)
        {
            if (!isfinite(h[j]) || (j > 0 && !(h[j] < h[j - 1])))
            {
                GRT_FAIL(GRTCODE_VALUE_ERR, "height of level %zu of column %zu (%e m) is not finite or not below the level "
                         "above it: top first, strictly descending.", j, c, h[j]);
            }
        }
        for (size_t k = 0; k < Z; ++k)
        {
            if (!(fabs(cos_zenith[c*Z + k]) <= 1.))
            {
                GRT_FAIL(GRTCODE_VALUE_ERR, "cosine of zenith angle %zu of column %zu (%e) is NaN or beyond 1 in size.", k, c,
                         cos_zenith[c*Z + k]);
            }
        }
    }
    for (size_t c = 0; c < C; ++c)
    {
        double const *h = height_m + c*V;
        double const r0 = radius_m + h[V - 1];
        for (size_t k = 0; k < Z; ++k)
        {
            double const mu0 = cos_zenith[c*Z + k];
            double *out = layer_cos_zenith + (c*Z + k)*L;
            double const s2 = r0*r0*(1. - mu0*mu0);
            for (size_t j = 0; j < L; ++j)
            {
                if (mu0 < 0.)
                {
                    out[j] = 0.;            /* (night; mu0 = 0 is the horizon's ray: finite, though no entry point reads it) */
                }
                else if (radius_m == 0.)
                {
                    out[j] = mu0;
                }
                else
                {
                    double const rt = radius_m + h[j], rb = radius_m + h[j + 1];
                    double const a = sqrt(rt*rt - s2), b = sqrt(rb*rb - s2);
                    out[j] = (a + b)/(rt + rb);
                }
            }
        }
    }
    return GRTCODE_SUCCESS;
}

/* What grt_pipeline_run_sky_zeniths_slant refuses in its layer cosines (nothing is touched): a NULL array, and under a day
   sample (cos_zenith > 0) a layer cosine that is not finite, is <= 0 or is > 1.  A night sample's entries are not read. */
int grt_check_zenith_slant(GrtZenithSlant_t const *sl, GrtZeniths_t const *zn, int C, int L)
{
    if (sl->layer_cos_zenith == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "layer_cos_zenith is NULL: the layer cosines [ncol][%d][%d] are the input.",
                 zn->num_zeniths, L);
    }
    size_t const n = (size_t)C*(size_t)zn->num_zeniths;
    for (size_t r = 0; r < n; ++r)
    {
        if (!(zn->cos_zenith[r] > 0.))
        {
            continue;
        }
        double const *mu = sl->layer_cos_zenith + r*(size_t)L;
        for (int j = 0; j < L; ++j)
        {
            if (!(mu[j] > 0.) || !(mu[j] <= 1.))
            {
                GRT_FAIL(GRTCODE_VALUE_ERR, "cosine of layer %d under zenith angle %zu of column %zu (%e) is not in (0, 1].", j,
                         r % (size_t)zn->num_zeniths, r/(size_t)zn->num_zeniths, mu[j]);
            }
        }
    }
    return GRTCODE_SUCCESS;
}

/* The checked cosines to the device, once per call: a block of the shortwave band's, [max_cols][Z][L] at this call's Z.
   (The copy reads the caller's pageable array before it returns, as every copy from such memory does.) */
int grt_stage_zenith_slant(GrtPipeline_t *p, GrtZenithSlant_t const *sl, int C, GrtZenithRun *zr)
{
    GrtScratch *block = &p->band[1].scratch[GRT_SCRATCH_ZEN_SLANT];
    size_t const per = (size_t)zr->zeniths*(size_t)(p->num_levels - 1);
    GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*per, NULL));
    GRT_TRY(grt_dev_upload(p->device, block->d, sl->layer_cos_zenith, sizeof(double)*(size_t)C*per, grt_dev_stream(p->device)));
    zr->slant.mu_layer = block->d;
    return GRTCODE_SUCCESS;
}

/* ---- windows: instrument channels (grt_pipeline_run_sky_channels) and spectral responses (_run_sky_weighted) ---- */

static GrtWindows channel_windows(GrtChannels_t const *ch)
{
    GrtWindows const w = {ch->num_channels, ch->first, ch->offset, ch->weights, "channel", ""};
    return w;
}

static GrtWindows response_windows(GrtResponses_t const *rs, int bi)
{
    GrtWindows const lw = {rs->lw_num_responses, rs->lw_first, rs->lw_offset, rs->lw_weights, "response", "longwave "};
    GrtWindows const sw = {rs->sw_num_responses, rs->sw_first, rs->sw_offset, rs->sw_weights, "response", "shortwave "};
    return bi == 0 ? lw : sw;
}

/* What every window set is refused for on a grid of n points (n < 1: no grid, so no range check and no pairs), its count
   apart, which the caller has checked: a NULL field, weights that do not start at 0, a window without a point or off the
   grid, a weight that is not finite.  *pairs: the (window, solver block) pairs in which a window has a point.  Nothing is
   touched. */
int grt_check_windows(GrtWindows const *w, long long n, long long *pairs)
{
    if (w->first == NULL || w->offset == NULL || w->weights == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s of the %s%ss is NULL.",
                 w->first == NULL ? "first" : (w->offset == NULL ? "offset" : "weights"), w->band, w->kind);
    }
    if (w->offset[0] != 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "offset[0] of the %s%ss is %d: the first %s's weights start at 0.", w->band, w->kind,
                 w->offset[0], w->kind);
    }
    long long P = 0;
    for (int k = 0; k < w->count; ++k)
    {
        if (w->offset[k + 1] <= w->offset[k])
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%soffset[%d] = %d is not above offset[%d] = %d: a %s has at least one point.", w->band,
                     k + 1, w->offset[k + 1], k, w->offset[k], w->kind);
        }
        long long const count = (long long)w->offset[k + 1] - w->offset[k];
        if (n >= 1 && (w->first[k] < 0 || w->first[k] + count > n))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%s%s %d takes the points %d .. %lld of a band of %lld.", w->band, w->kind, k,
                     w->first[k], w->first[k] + count - 1, n);
        }
        for (int j = w->offset[k]; j < w->offset[k + 1]; ++j)
        {
            if (!isfinite(w->weights[j]))
            {
                GRT_FAIL(GRTCODE_VALUE_ERR, "weight %d of %s%s %d (%e) is NaN or infinite.", j - w->offset[k], w->band, w->kind,
                         k, w->weights[j]);
            }
        }
        if (n >= 1)
        {
            P += (w->first[k] + count - 1)/GRT_SOLVER_BLOCK - w->first[k]/GRT_SOLVER_BLOCK + 1;
        }
    }
    *pairs = P;
    return GRTCODE_SUCCESS;
}

/* the ints of the window table (grt_kernels.h) of `count` windows with `pairs` pairs on a grid of nblocks solver blocks */
size_t grt_window_table_ints(int count, size_t nblocks, long long pairs)
{
    return (size_t)GRT_WINDOW_INTS*(size_t)count + nblocks + 1 + (size_t)pairs;
}

/* ... written to ints for the checked windows first, offset [count]: the entries, block_start, the block lists */
void grt_window_table(int const *first, int const *offset, int count, size_t nblocks, int *ints)
{
    int *block_start = ints + (size_t)GRT_WINDOW_INTS*(size_t)count, *block_list = block_start + nblocks + 1;
    memset(block_start, 0, sizeof(int)*(nblocks + 1));
    int pair = 0;
    for (int k = 0; k < count; ++k)
    {
        int const points = offset[k + 1] - offset[k];
        int const b_lo = first[k]/GRT_SOLVER_BLOCK, b_hi = (first[k] + points - 1)/GRT_SOLVER_BLOCK;
        int *e = ints + (size_t)GRT_WINDOW_INTS*(size_t)k;
        e[0] = first[k]; e[1] = points; e[2] = offset[k]; e[3] = b_lo; e[4] = pair;
        pair += b_hi - b_lo + 1;
        for (int b = b_lo; b <= b_hi; ++b)
        {
            ++block_start[b + 1];               /* (counts first, then their running sum) */
        }
    }
    for (size_t b = 0; b < nblocks; ++b)
    {
        block_start[b + 1] += block_start[b];
    }
    /* the windows of a block in ascending order: block_start[b] walks block b's list and ends where the next one starts,
       then every start moves back up by one block */
    for (int k = 0; k < count; ++k)
    {
        int const *e = ints + (size_t)GRT_WINDOW_INTS*(size_t)k;
        for (int b = e[3]; b <= (e[0] + e[1] - 1)/GRT_SOLVER_BLOCK; ++b)
        {
            block_list[block_start[b]++] = k;
        }
    }
    memmove(block_start + 1, block_start, sizeof(int)*nblocks);
    block_start[0] = 0;
}

/* The device table of windows on band b's grid, as grt_keyed_table keeps it: the doubles first (the table is a device
   allocation: aligned for them) -- the weights and, of channels, sum_w and center [count] each --, then the window table. */
typedef struct WindowTableFill
{
    GrtWindows w;
    GrtChannels_t const *ch;          /* the channels the windows are, or NULL */
    SpectralGrid_t const *grid;
    size_t nblocks, doubles;
} WindowTableFill;

static int fill_window_table(void *ctx, int *table)
{
    WindowTableFill const *f = ctx;
    GrtWindows const *w = &f->w;
    size_t const W = (size_t)w->offset[w->count];
    double *weights = (double *)table, *sum_w = weights + W, *center = sum_w + w->count;
    memcpy(weights, w->weights, sizeof(double)*W);
    for (int c = 0; f->ch != NULL && c < w->count; ++c)
    {
        double sum = 0., wsum = 0.;       /* (both in index order) */
        for (int k = w->offset[c]; k < w->offset[c + 1]; ++k)
        {
            sum += w->weights[k];
            wsum += w->weights[k]*(f->grid->w0 + (double)(w->first[c] + k - w->offset[c])*f->grid->dw);
        }
        sum_w[c] = sum;
        center[c] = f->ch->center != NULL ? f->ch->center[c] : wsum/sum;
    }
    grt_window_table(w->first, w->offset, w->count, f->nblocks, table + 2*f->doubles);
    return GRTCODE_SUCCESS;
}

/* The checked windows w (`pairs`: grt_check_windows' on b's grid) as b's device table t -- built and uploaded when the
   grid's points, the count, first, offset, weights or, of channels ch, the centers differ from the last call's -- and
   where its parts lie. */
typedef struct WindowTable { double const *weights; int const *entry, *block_start, *block_list; } WindowTable;

static int stage_windows(GrtPipeline_t *p, GrtBand *b, GrtKeyedTable *t, GrtWindows const *w, GrtChannels_t const *ch,
                         long long pairs, WindowTable *wt)
{
    size_t const N = (size_t)w->count, W = (size_t)w->offset[N];
    WindowTableFill f = {*w, ch, &b->gas->grid, grt_solver_blocks(b->n), W + (ch != NULL ? 2*N : 0)};
    /* the key: the grid's points, the count and -- channels -- whether centers are given, then first, offset, weights and
       the centers, where they are */
    long long const h[3] = {(long long)b->n, w->count, ch != NULL && ch->center != NULL};
    GrtKeyPart const key[5] = {{h, sizeof(long long)*(ch != NULL ? 3 : 2)}, {w->first, sizeof(int)*N},
                               {w->offset, sizeof(int)*(N + 1)}, {w->weights, sizeof(double)*W},
                               {ch != NULL ? ch->center : NULL, h[2] ? sizeof(double)*N : 0}};
    size_t const ints = 2*f.doubles + grt_window_table_ints(w->count, f.nblocks, pairs);
    GRT_TRY(grt_keyed_table_parts(p, t, key, ch != NULL ? 5 : 4, ints, fill_window_table, &f));
    wt->weights = (double const *)t->table;
    wt->entry = t->table + 2*f.doubles;
    wt->block_start = wt->entry + (size_t)GRT_WINDOW_INTS*N;
    wt->block_list = wt->block_start + f.nblocks + 1;
    return GRTCODE_SUCCESS;
}

/* What grt_pipeline_run_sky_channels and grt_channel_pair_count check of an instrument's channels on a grid of n points
   (n < 1: a pipeline without a longwave band, no range check), the output pointers apart; *pairs: the (channel, solver
   block) pairs in which a channel has a point (0 without a grid).  Nothing is touched. */
int grt_check_channels(GrtChannels_t const *ch, long long n, long long *pairs)
{
    if (ch == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "channels (GrtChannels_t) is NULL: %s", "the instrument's channels are the input.");
    }
    if (ch->num_channels < 1 || ch->num_channels > GRT_MAX_CHANNELS)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d channels asked for: 1 to %d.", ch->num_channels, GRT_MAX_CHANNELS);
    }
    GrtWindows const w = channel_windows(ch);
    long long P;
    GRT_TRY(grt_check_windows(&w, n, &P));
    for (int c = 0; c < ch->num_channels; ++c)
    {
        double sum = 0.;                  /* (in index order: what the table divides by) */
        for (int k = ch->offset[c]; k < ch->offset[c + 1]; ++k)
        {
            sum += ch->weights[k];
        }
        if (!(sum > 0.) || !isfinite(sum))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "the weights of channel %d add up to %e: a sum that is finite and above 0 is needed.",
                     c, sum);
        }
        if (ch->center != NULL && (!(ch->center[c] > 0.) || !isfinite(ch->center[c])))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "center of channel %d (%e) is NaN, infinite or not above 0.", c, ch->center[c]);
        }
    }
    *pairs = P;
    return GRTCODE_SUCCESS;
}

/* The channels of a grt_pipeline_run_sky_channels call (checked by grt_check_channels on b's grid, which gave `pairs`) as
   the longwave band's device table, and where their outputs go */
int grt_stage_channels(GrtPipeline_t *p, GrtBand *b, GrtChannels_t const *ch, long long pairs, GrtChannelRun *cr)
{
    GrtWindows const w = channel_windows(ch);
    WindowTable wt;
    GRT_TRY(stage_windows(p, b, &b->channel_table, &w, ch, pairs, &wt));
    memset(cr, 0, sizeof(*cr));
    GrtChannelArgs *a = &cr->args;
    a->channels = w.count;
    a->pairs = (uint64_t)pairs;
    a->entry = wt.entry;
    a->block_start = wt.block_start;
    a->block_list = wt.block_list;
    a->weights = wt.weights;
    a->sum_w = a->weights + w.offset[w.count];
    a->center = a->sum_w + w.count;
    cr->radiances = ch->channel_radiances_dev;
    cr->brightness = ch->channel_brightness_dev;
    return GRTCODE_SUCCESS;
}

/* What grt_pipeline_run_sky_weighted and grt_response_pair_count check of one band's responses on a grid of n points (a
   band without responses: nothing) and at most block_limit of them in one block (< 0: not checked).  Nothing is touched. */
int grt_check_responses(GrtResponses_t const *rs, int bi, long long n, int block_limit, long long *pairs, int *block_max)
{
    GrtWindows const r = response_windows(rs, bi);
    *pairs = 0;
    *block_max = 0;
    if (r.count < 0 || r.count > GRT_MAX_RESPONSES)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %sresponses asked for: 0 to %d.", r.count, r.band, GRT_MAX_RESPONSES);
    }
    if (r.count == 0)
    {
        return GRTCODE_SUCCESS;
    }
    if (n < 1)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %sresponses, and this pipeline has no %sband.", r.count, r.band, r.band);
    }
    long long P;
    GRT_TRY(grt_check_windows(&r, n, &P));
    /* the most responses with a point in one block: a count per block */
    size_t const nblocks = (size_t)((n + GRT_SOLVER_BLOCK - 1)/GRT_SOLVER_BLOCK);
    int *held = calloc(nblocks, sizeof(int));
    if (held == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for the response counts of %zu blocks.", nblocks);
    }
    int most = 0, most_at = 0;
    for (int k = 0; k < r.count; ++k)
    {
        long long const last = r.first[k] + ((long long)r.offset[k + 1] - r.offset[k]) - 1;
        for (long long blk = r.first[k]/GRT_SOLVER_BLOCK; blk <= last/GRT_SOLVER_BLOCK; ++blk)
        {
            if (++held[blk] > most)
            {
                most = held[blk];
                most_at = (int)blk;
            }
        }
    }
    free(held);
    if (block_limit >= 0 && most > block_limit)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %sresponses have a point in block %d (points %d .. %d): at most %d "
                 "(grt_pipeline_response_block_limit).", most, r.band, most_at, most_at*GRT_SOLVER_BLOCK,
                 most_at*GRT_SOLVER_BLOCK + GRT_SOLVER_BLOCK - 1, block_limit);
    }
    *pairs = P;
    *block_max = most;
    return GRTCODE_SUCCESS;
}

/* Band bi's responses of a grt_pipeline_run_sky_weighted call (checked by grt_check_responses on b's grid, which gave
   `pairs` and `block_max`) as the band's device table */
int grt_stage_responses(GrtPipeline_t *p, GrtBand *b, int bi, GrtResponses_t const *rs, long long pairs, int block_max,
                        GrtResponseRun *rr)
{
    GrtWindows const w = response_windows(rs, bi);
    WindowTable wt;
    GRT_TRY(stage_windows(p, b, &b->response_table, &w, NULL, pairs, &wt));
    memset(rr, 0, sizeof(*rr));
    GrtResponseArgs *a = &rr->args;
    a->responses = w.count;
    a->block_max = block_max;
    a->per_row = (uint64_t)pairs;
    a->entry = wt.entry;
    a->block_start = wt.block_start;
    a->block_list = wt.block_list;
    a->weights = wt.weights;
    rr->groups = bi == 0 ? 2 : 3;
    return GRTCODE_SUCCESS;
}

/* ---- channel transmittances and contribution functions (grt_pipeline_run_sky_weighting) ---- */

/* What grt_pipeline_run_sky_weighting checks of its own argument.  Nothing is touched. */
int grt_check_weighting(GrtWeighting_t const *wt)
{
    if (wt == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "weighting (GrtWeighting_t) is NULL: %s", "it names the outputs.");
    }
    if (wt->transmittance_dev == NULL && wt->contribution_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "transmittance_dev and contribution_dev are both NULL: %s", "one of them is the output.");
    }
    return GRTCODE_SUCCESS;
}

/* ... staged: nothing of it lies on the host */
void grt_stage_weighting(GrtWeighting_t const *wt, GrtWeightingRun *wr)
{
    memset(wr, 0, sizeof(*wr));
    wr->args.transmittance = wt->transmittance_dev != NULL;
    wr->args.contribution = wt->contribution_dev != NULL;
    wr->transmittance = wt->transmittance_dev;
    wr->contribution = wt->contribution_dev;
}

/* one band's bins on a grid of n points: none, or num_bins + 1 strictly increasing grid-point indices in 0 .. n - 1 and
   somewhere to write them (grt_pipeline_run_spectral, _run_band_profiles, _run_kdist, grt_kdist_rows) */
int grt_check_bin_edges(char const *name, int const *edges, int num_bins, long long n, int has_output)
{
    if (num_bins < 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s bins.", num_bins, name);
    }
    if (num_bins == 0)
    {
        return GRTCODE_SUCCESS;
    }
    if (edges == NULL || !has_output)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s bins with NULL edges or a NULL binned_dev.", num_bins, name);
    }
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

typedef struct BinTableFill { int const *edges; int nbins; uint64_t n; size_t per_row; } BinTableFill;

static int fill_bin_table(void *ctx, int *table)
{
    BinTableFill *f = ctx;
    f->per_row = grt_bin_table(f->edges, f->nbins, f->n, table);
    return GRTCODE_SUCCESS;
}

/* the band's bin table for these edges (built and uploaded when they differ from the last call's) and room for the partial
   sums of max_cols x `rows` rows */
int grt_band_bins(GrtPipeline_t *p, GrtBand *b, int const *edges, int nbins, int rows)
{
    BinTableFill f = {edges, nbins, b->n, b->bin_per_row};
    GRT_TRY(grt_keyed_table(p, &b->bin_table, edges, sizeof(int)*((size_t)nbins + 1), grt_bin_table_ints(nbins, b->n),
                            fill_bin_table, &f));
    b->bin_per_row = f.per_row;
    GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_BIN_PARTIALS], (size_t)p->max_cols*(size_t)rows*b->bin_per_row, NULL));
    return GRTCODE_SUCCESS;
}
