/* grt_cloud_sampler.c -- the host side of the device cloud sampler (grt_ext.h: grt_cloud_sampler_*): the parametrisation
 * tables uploaded once, a batch's cloud fields staged through pinned memory, the argument checks, the launch
 * (k_cloud_sample.hip).  The model arrives as data: nothing here reads a parameter file or links libclouds.a. */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "grt_internal.h"

#define PDF_P 5        /* the clouds library's water PDF (clouds_lib.c:18-45): shape (5, 5) */
#define PDF_Q 5

struct GrtCloudSampler
{
    Device_t device;
    int num_bands[2];                  /* liquid (B), ice */
    double *band_lo[2], *band_hi[2];   /* host copies of the band limits: the pipeline's cloud maps */
    double *model_d;                   /* device: every table the kernel reads, one block */
    GrtCloudSampleArgs args;           /* the model's part, filled once */
    /* a batch's fields: pinned host buffer, refilled every call, and its device copy */
    double *h, *d;
    size_t doubles;
    void *uploaded;                    /* event: h has been copied out and may be refilled */
};

static int check_phase(char const *name, GrtCloudPhase_t const *o)
{
    if (o->nband < 1 || o->nsize < 1 || o->np < 1 || o->nq < 1)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s parametrisation: %d bands, %d size regimes, %d and %d coefficients: at least one of "
                 "each.", name, o->nband, o->nsize, o->np, o->nq);
    }
    if (o->band_lo == NULL || o->band_hi == NULL || o->size_lo == NULL || o->size_hi == NULL || o->size_ref == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "a NULL array in the %s parametrisation.", name);
    }
    for (int k = 0; k < 6; ++k)
    {
        if (o->coef[k] == NULL)
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "coefficient array %d of the %s parametrisation is NULL.", k, name);
        }
    }
    return GRTCODE_SUCCESS;
}

static size_t phase_doubles(GrtCloudPhase_t const *o)
{
    size_t const cells = (size_t)o->nband*(size_t)o->nsize;
    return 3*(size_t)o->nsize + 3*cells*((size_t)o->np + (size_t)o->nq);
}

/* a phase's tables into the host image at *at (advanced), their device addresses into dev */
static void pack_phase(GrtCloudPhase_t const *o, double *image, size_t *at, double const *base_d, GrtCloudPhaseDev *dev)
{
    size_t const ns = (size_t)o->nsize, cells = (size_t)o->nband*ns;
    fp_t const *sizes[3] = {o->size_lo, o->size_hi, o->size_ref};
    double const **dst[3] = {&dev->size_lo, &dev->size_hi, &dev->size_ref};
    dev->nsize = o->nsize;
    dev->np = o->np;
    dev->nq = o->nq;
    for (int k = 0; k < 3; ++k)
    {
        memcpy(image + *at, sizes[k], sizeof(double)*ns);
        *dst[k] = base_d + *at;
        *at += ns;
    }
    for (int k = 0; k < 6; ++k)
    {
        size_t const n = cells*(size_t)(k % 2 == 0 ? o->np : o->nq);
        memcpy(image + *at, o->coef[k], sizeof(double)*n);
        dev->coef[k] = base_d + *at;
        *at += n;
    }
}

EXTERN int grt_cloud_sampler_create(GrtCloudSampler_t **sampler, Device_t device, GrtCloudModel_t const *m)
{
    if (sampler == NULL || m == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "grt_cloud_sampler_create: a NULL %s.", sampler == NULL ? "sampler" : "model");
    }
    *sampler = NULL;
    if (m->num_shape < PDF_P + 1 || m->num_x < 2)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "beta tables of %d shape parameters and %d abscissae: the water PDF reads shapes (5, 5) "
                 "and (6, 5), and a segment needs 2 points.", m->num_shape, m->num_x);
    }
    if (m->x == NULL || m->value == NULL || m->inverse == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "a NULL array in the beta tables.%s", "");
    }
    for (int i = 0; i + 1 < m->num_x; ++i)
    {
        /* (the kernel finds its segment by bisection: the first x_i > at of an ascending x is the linear scan's) */
        if (!(m->x[i + 1] >= m->x[i]))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "the beta tables' x descends (x[%d] = %e, x[%d] = %e).", i, m->x[i], i + 1, m->x[i + 1]);
        }
    }
    GRT_TRY(check_phase("liquid", &m->liquid));
    GRT_TRY(check_phase("ice", &m->ice));
    if (m->ice.nband < m->liquid.nband)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d ice bands, %d liquid bands, whose bands drive the loop: no fewer ice bands.",
                 m->ice.nband, m->liquid.nband);
    }
    GRT_TRY(grt_dev_require(device));
    GrtCloudSampler_t *sp = calloc(1, sizeof(*sp));
    size_t const nx = (size_t)m->num_x, total = 3*nx + phase_doubles(&m->liquid) + phase_doubles(&m->ice);
    double *image = malloc(sizeof(double)*total);
    if (sp == NULL || image == NULL)
    {
        free(sp);
        free(image);
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for the cloud model (%zu doubles).", total);
    }
    sp->device = device;
    GrtCloudPhase_t const *phase[2] = {&m->liquid, &m->ice};
    int rc = GRTCODE_SUCCESS;
    for (int k = 0; k < 2 && rc == GRTCODE_SUCCESS; ++k)
    {
        size_t const nb = (size_t)phase[k]->nband;
        sp->num_bands[k] = phase[k]->nband;
        sp->band_lo[k] = malloc(sizeof(double)*nb);
        sp->band_hi[k] = malloc(sizeof(double)*nb);
        if (sp->band_lo[k] == NULL || sp->band_hi[k] == NULL)
        {
            rc = GRTCODE_NULL_ERR;
            break;
        }
        memcpy(sp->band_lo[k], phase[k]->band_lo, sizeof(double)*nb);
        memcpy(sp->band_hi[k], phase[k]->band_hi, sizeof(double)*nb);
    }
    if (rc == GRTCODE_SUCCESS) rc = grt_dev_alloc(device, (void **)&sp->model_d, sizeof(double)*total);
    if (rc == GRTCODE_SUCCESS)
    {
        /* value / inverse are [q - 1][p - 1][x]: the rows of inverse (p, q) and of value (p + 1, q) */
        size_t const ns = (size_t)m->num_shape;
        GrtCloudSampleArgs *a = &sp->args;
        a->num_x = m->num_x;
        a->num_bands = m->liquid.nband;
        memcpy(image, m->x, sizeof(double)*nx);
        memcpy(image + nx, m->inverse + ((size_t)(PDF_Q - 1)*ns + (size_t)(PDF_P - 1))*nx, sizeof(double)*nx);
        memcpy(image + 2*nx, m->value + ((size_t)(PDF_Q - 1)*ns + (size_t)PDF_P)*nx, sizeof(double)*nx);
        a->x = sp->model_d;
        a->inverse_pq = sp->model_d + nx;
        a->value_p1q = sp->model_d + 2*nx;
        size_t at = 3*nx;
        pack_phase(&m->liquid, image, &at, sp->model_d, &a->liquid);
        pack_phase(&m->ice, image, &at, sp->model_d, &a->ice);
        void *s = grt_dev_stream(device);
        rc = grt_dev_upload(device, sp->model_d, image, sizeof(double)*total, s);
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(device, s);
    }
    free(image);
    if (rc != GRTCODE_SUCCESS)
    {
        grt_cloud_sampler_destroy(&sp);
        GRT_TRY(rc);
    }
    *sampler = sp;
    return GRTCODE_SUCCESS;
}

EXTERN int grt_cloud_sampler_destroy(GrtCloudSampler_t **sampler)
{
    if (sampler == NULL || *sampler == NULL)
    {
        return GRTCODE_SUCCESS;
    }
    GrtCloudSampler_t *sp = *sampler;
    if (sp->model_d != NULL || sp->d != NULL)
    {
        grt_dev_sync(sp->device, grt_dev_stream(sp->device));
    }
    grt_dev_free(sp->device, sp->model_d);
    grt_dev_free(sp->device, sp->d);
    grt_host_free_pinned(sp->h);
    grt_dev_event_destroy(sp->device, &sp->uploaded);
    for (int k = 0; k < 2; ++k)
    {
        free(sp->band_lo[k]);
        free(sp->band_hi[k]);
    }
    free(sp);
    *sampler = NULL;
    return GRTCODE_SUCCESS;
}

Device_t grt_cloud_sampler_device(GrtCloudSampler_t const *sp)
{
    return sp->device;
}

/* the model's band limits as the all-sky entry points take them; thickness and the optics sets are left alone */
void grt_cloud_sampler_bands(GrtCloudSampler_t const *sp, GrtClouds_t *cl)
{
    cl->num_liquid_bands = sp->num_bands[0];
    cl->num_ice_bands = sp->num_bands[1];
    cl->liquid_band_lo = sp->band_lo[0];
    cl->liquid_band_hi = sp->band_hi[0];
    cl->ice_band_lo = sp->band_lo[1];
    cl->ice_band_hi = sp->band_hi[1];
}

/* what grt_cloud_sampler_run and grt_pipeline_run_cloud_fields refuse alike; need_temperature: fields->temperature must
   be given (the pipeline falls back on the columns' layer temperatures) */
int grt_cloud_sampler_check(GrtCloudSampler_t const *sp, GrtCloudFields_t const *f, int need_temperature)
{
    if (sp == NULL || f == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no cloud %s (NULL).", sp == NULL ? "sampler" : "fields");
    }
    if (f->num_subcolumns < 1 || f->num_subcolumns > GRT_MAX_SUBCOLUMNS)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d subcolumns asked for: 1 to %d.", f->num_subcolumns, GRT_MAX_SUBCOLUMNS);
    }
    if (f->ncol < 1 || f->num_layers < 1)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "cloud fields of %d columns and %d layers: at least one of each.", f->ncol, f->num_layers);
    }
    if (f->cloud_fraction == NULL || f->liquid_content == NULL || f->ice_content == NULL ||
        (need_temperature && f->temperature == NULL) || (f->num_layers > 1 && f->overlap == NULL))
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "a NULL array in the cloud fields.%s", "");
    }
    size_t const n = (size_t)f->ncol*(size_t)f->num_layers;
    for (size_t i = 0; i < n; ++i)
    {
        double const cf = f->cloud_fraction[i], lwc = f->liquid_content[i], iwc = f->ice_content[i];
        if (!(cf >= 0. && cf <= 1.))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "cloud fraction %e (column %zu, layer %zu): 0 to 1.", cf, i/(size_t)f->num_layers,
                     i % (size_t)f->num_layers);
        }
        if (!(lwc >= 0. && isfinite(lwc)) || !(iwc >= 0. && isfinite(iwc)))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "water contents %e (liquid), %e (ice) (column %zu, layer %zu): finite and not "
                     "negative.", lwc, iwc, i/(size_t)f->num_layers, i % (size_t)f->num_layers);
        }
    }
    return GRTCODE_SUCCESS;
}

/* The fields of a batch grt_cloud_sampler_check has passed to the device, and the kernel into tables_dev
   [4][S][ncol][3][B][L], on the device's current lane.  temperature [ncol][L]: fields->temperature or its stand-in.
   The pinned buffer is reused every call: wait until the previous batch's copy of it has left, not for its kernel. */
int grt_cloud_sampler_enqueue(GrtCloudSampler_t *sp, GrtCloudFields_t const *f, fp_t const *temperature, double *tables_dev)
{
    size_t const C = (size_t)f->ncol, L = (size_t)f->num_layers, S = (size_t)f->num_subcolumns, B = (size_t)sp->num_bands[0];
    size_t const layers = C*L, pairs = C*(L - 1);
    size_t const draws = f->uniforms != NULL ? C*2*S*B*(2*L - 1) : 0, need = 4*layers + pairs + draws;
    void *s = grt_dev_stream(sp->device);
    GRT_TRY(grt_dev_event_wait(sp->device, sp->uploaded));
    if (need > sp->doubles)
    {
        GRT_TRY(grt_dev_sync(sp->device, s));
        grt_dev_free(sp->device, sp->d);
        grt_host_free_pinned(sp->h);
        sp->d = NULL;
        sp->h = NULL;
        sp->doubles = 0;
        GRT_TRY(grt_host_alloc_pinned((void **)&sp->h, sizeof(double)*need));
        GRT_TRY(grt_dev_alloc(sp->device, (void **)&sp->d, sizeof(double)*need));
        sp->doubles = need;
    }
    fp_t const *src[4] = {f->cloud_fraction, f->liquid_content, f->ice_content, temperature};
    for (int k = 0; k < 4; ++k)
    {
        memcpy(sp->h + (size_t)k*layers, src[k], sizeof(double)*layers);
    }
    if (pairs > 0)
    {
        memcpy(sp->h + 4*layers, f->overlap, sizeof(double)*pairs);
    }
    if (draws > 0)
    {
        memcpy(sp->h + 4*layers + pairs, f->uniforms, sizeof(double)*draws);
    }
    GRT_TRY(grt_dev_upload(sp->device, sp->d, sp->h, sizeof(double)*need, s));
    GRT_TRY(grt_dev_event_record(sp->device, &sp->uploaded, s));

    GrtCloudSampleArgs a = sp->args;
    a.ncol = f->ncol;
    a.num_layers = f->num_layers;
    a.subcolumns = f->num_subcolumns;
    a.cloud_fraction = sp->d;
    a.liquid_content = sp->d + layers;
    a.ice_content = sp->d + 2*layers;
    a.temperature = sp->d + 3*layers;
    a.overlap = sp->d + 4*layers;
    a.uniforms = draws > 0 ? sp->d + 4*layers + pairs : NULL;
    a.liquid_radius = f->liquid_radius;
    a.key0 = (uint32_t)(f->seed & 0xffffffffu);
    a.key1 = (uint32_t)(f->seed >> 32);
    a.column0 = (uint32_t)((uint64_t)f->column_offset & 0xffffffffu);
    a.tables = tables_dev;
    int const slot = grt_profile_begin(s, GRT_TAG_CLOUD_SAMPLER);
    int const krc = grt_launch_cloud_sample(s, &a);
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "cloud sampling kernel"));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_cloud_sampler_run(GrtCloudSampler_t *sampler, GrtCloudFields_t const *fields, fp_t *tables_dev)
{
    GRT_TRY(grt_cloud_sampler_check(sampler, fields, 1));
    if (tables_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "tables_dev is NULL: the tables [4][%d][%d][3][%d][%d] are the output.",
                 fields->num_subcolumns, fields->ncol, sampler->num_bands[0], fields->num_layers);
    }
    GRT_TRY(grt_cloud_sampler_enqueue(sampler, fields, fields->temperature, tables_dev));
    return GRTCODE_SUCCESS;
}
