/* grt_kdist.c -- the host side of the k-distributions of optical-depth rows (grt_ext.h: grt_kdist_rows,
 * grt_pipeline_run_kdist, grt_kdist_chunk_points) and of the correlated ones under one class map per group
 * (grt_kdist_class_map, grt_kdist_mapped_rows, grt_pipeline_run_kdist_correlated): the argument checks, the class edges,
 * weight and bin edges of a call kept on the device until a call brings other ones, the launches (k_kdist.hip).  The
 * pipeline entry points themselves, which run the gas optics in front of the reduction, are grt_pipeline.c's;
 * grt_pipeline_run_ck_fluxes takes its map and its mapped reduction from here too (grt_kdist_reduce_ck). */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "grt_pipeline_internal.h"

_Static_assert(GRT_KDIST_MAX_CLASSES == GRT_KDIST_CLASS_LIMIT, "the kernel's class limit is the interface's");

/* grt_kdist_rows', grt_kdist_class_map's and grt_kdist_mapped_rows' inputs on the device, one set each per device: they
   live as long as the process */
#define GRT_KDIST_DEVICES 64
static GrtKdistTable g_rows_table[GRT_KDIST_DEVICES], g_map_table[GRT_KDIST_DEVICES], g_mapped_table[GRT_KDIST_DEVICES];

int grt_kdist_check_classes(int num_classes, fp_t const *class_edges)
{
    if (num_classes < 2 || num_classes > GRT_KDIST_MAX_CLASSES)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d classes asked for: 2 to %d.", num_classes, GRT_KDIST_MAX_CLASSES);
    }
    if (class_edges == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "class_edges is NULL: the %d class edges are the input.", num_classes - 1);
    }
    for (int k = 0; k < num_classes - 1; ++k)
    {
        if (!isfinite(class_edges[k]))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "class edge %d (%e) is not finite.", k, class_edges[k]);
        }
        if (k > 0 && !(class_edges[k] > class_edges[k - 1]))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "class edges not strictly increasing (edge %d = %e, edge %d = %e).", k - 1,
                     class_edges[k - 1], k, class_edges[k]);
        }
    }
    return GRTCODE_SUCCESS;
}

/* a band that has bins: an output to write, and a weight, where one is given, that is >= 0 and finite at all n points */
int grt_kdist_check_band(char const *name, GrtKdistBand_t const *band, long long n)
{
    if (band->points_dev == NULL && band->weight_dev == NULL && band->tau_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d %s bins and points_dev, weight_dev and tau_dev all NULL: nothing to write.",
                 band->num_bins, name);
    }
    for (long long i = 0; band->weight != NULL && i < n; ++i)
    {
        /* (a NaN fails the first comparison) */
        if (!(band->weight[i] >= 0.) || !isfinite(band->weight[i]))
        {
            GRT_FAIL(GRTCODE_VALUE_ERR, "%s weight %lld (%e) is negative or not finite.", name, i, band->weight[i]);
        }
    }
    return GRTCODE_SUCCESS;
}

void grt_kdist_table_free(Device_t device, GrtKdistTable *t)
{
    grt_dev_free(device, t->block);
    free(t->key);
    memset(t, 0, sizeof(*t));
}

/* *t for these class edges [ne], weight [nw] (nw == 0: none) and bin edges [nb + 1] (NULL: none): as it is when it holds the same bytes,
   else uploaded behind everything queued on the lane, which may still read the block it replaces.  The key is dropped
   before the block is touched and set again only when all of it succeeded (as grt_keyed_table's). */
static int kdist_table(Device_t device, GrtKdistTable *t, fp_t const *class_edges, size_t ne, fp_t const *weight, size_t nw,
                       int const *edges, size_t nb)
{
    size_t const part[3] = {sizeof(double)*ne, sizeof(double)*nw, edges != NULL ? sizeof(int)*(nb + 1) : 0};
    void const *from[3] = {class_edges, weight, edges};
    size_t const bytes = part[0] + part[1] + part[2];
    if (t->key != NULL && t->key_bytes == bytes && t->num_edges == ne && t->num_weights == nw)
    {
        char const *at = t->key;
        int same = 1;
        for (int k = 0; k < 3 && same; at += part[k], ++k)
        {
            same = part[k] == 0 || memcmp(at, from[k], part[k]) == 0;
        }
        if (same)
        {
            return GRTCODE_SUCCESS;
        }
    }
    char *image = malloc(bytes);
    if (image == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for %zu bytes of k-distribution inputs.", bytes);
    }
    char *to = image;
    for (int k = 0; k < 3; to += part[k], ++k)
    {
        if (part[k] > 0)
        {
            memcpy(to, from[k], part[k]);
        }
    }
    free(t->key);
    t->key = NULL;
    void *s = grt_dev_stream(device);
    int rc = grt_dev_sync(device, s);
    if (rc == GRTCODE_SUCCESS)
    {
        grt_dev_free(device, t->block);
        t->block = NULL;
        rc = grt_dev_alloc(device, &t->block, bytes);
    }
    if (rc == GRTCODE_SUCCESS) rc = grt_dev_upload(device, t->block, image, bytes, s);
    if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(device, s);
    if (rc != GRTCODE_SUCCESS)
    {
        free(image);
        GRT_TRY(rc);
    }
    t->key = image;
    t->key_bytes = bytes;
    t->num_edges = ne;
    t->num_weights = nw;
    return GRTCODE_SUCCESS;
}

/* the reduction of tau_dev [rows][n] into band's outputs, every argument checked already */
int grt_kdist_reduce(Device_t device, GrtKdistTable *t, fp_t const *tau_dev, long long rows, long long n, fp_t dw,
                     int num_classes, fp_t const *class_edges, GrtKdistBand_t const *band)
{
    size_t const ne = (size_t)num_classes - 1, nw = band->weight != NULL ? (size_t)n : 0;
    GRT_TRY(kdist_table(device, t, class_edges, ne, band->weight, nw, band->edges, (size_t)band->num_bins));
    double const *doubles = t->block;
    GrtKdistArgs const a = {.tau = tau_dev, .rows = rows, .n = n, .dw = dw, .num_classes = num_classes,
                            .num_bins = band->num_bins, .class_edges = doubles,
                            .edges = (int const *)(doubles + ne + nw), .weight = nw > 0 ? doubles + ne : NULL,
                            .points = band->points_dev, .weight_sum = band->weight_dev, .tau_sum = band->tau_dev};
    void *s = grt_dev_stream(device);
    int const slot = grt_profile_begin(s, GRT_TAG_KDIST);
    int const krc = grt_launch_kdist(s, &a);
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "k-distribution kernel"));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_kdist_rows(Device_t device, fp_t const *tau_dev, long long rows, long long n, fp_t dw, int num_classes,
                          fp_t const *class_edges, GrtKdistBand_t const *band)
{
    if (tau_dev == NULL || band == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s is NULL.", tau_dev == NULL ? "tau_dev" : "band");
    }
    GRT_TRY(grt_kdist_check_classes(num_classes, class_edges));
    if (rows < 1 || n < 2)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%lld rows of %lld points: at least 1 row of at least 2 points.", rows, n);
    }
    if (!(dw > 0.) || !isfinite(dw))
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "grid spacing (%e) is not positive and finite.", dw);
    }
    GRT_TRY(grt_check_bin_edges("row", band->edges, band->num_bins, n, 1));
    if (band->num_bins == 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no bins: nothing to write.%s", "");
    }
    GRT_TRY(grt_kdist_check_band("row", band, n));
    GRT_TRY(grt_dev_require(device));
    GRT_TRY(grt_kdist_reduce(device, &g_rows_table[device], tau_dev, rows, n, dw, num_classes, class_edges, band));
    return GRTCODE_SUCCESS;
}

/* the class map of x_dev [groups][rows_per_group][n] under the class edges on the device; key_row < 0: the rows' sum */
static int launch_map(Device_t device, double const *class_edges_dev, fp_t const *x_dev, long long groups,
                      long long rows_per_group, long long n, long long key_row, int num_classes, unsigned short *map_dev)
{
    GrtKdistMapArgs const a = {.x = x_dev, .groups = groups, .rows_per_group = rows_per_group, .n = n, .key_row = key_row,
                               .num_classes = num_classes, .class_edges = class_edges_dev, .map = map_dev};
    void *s = grt_dev_stream(device);
    int const slot = grt_profile_begin(s, GRT_TAG_KDIST_MAP);
    int const krc = grt_launch_kdist_map(s, &a);
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "class-map kernel"));
    return GRTCODE_SUCCESS;
}

/* the reduction of the groups' rows under map_dev into band's outputs; the weight (or NULL) and the bin edges on the device */
static int launch_mapped(Device_t device, fp_t const *values_dev, long long group_stride, unsigned short const *map_dev,
                         long long groups, long long rows_per_group, long long n, fp_t dw, int num_classes,
                         double const *weight_dev, int const *edges_dev, GrtKdistBand_t const *band)
{
    GrtKdistMappedArgs const a = {.values = values_dev, .group_stride = group_stride, .map = map_dev, .groups = groups,
                                  .rows_per_group = rows_per_group, .n = n, .dw = dw, .num_classes = num_classes,
                                  .num_bins = band->num_bins, .edges = edges_dev, .weight = weight_dev,
                                  .points = band->points_dev, .weight_sum = band->weight_dev, .tau_sum = band->tau_dev};
    void *s = grt_dev_stream(device);
    int const slot = grt_profile_begin(s, GRT_TAG_KDIST_MAPPED);
    int const krc = grt_launch_kdist_mapped(s, &a);
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "mapped k-distribution kernel"));
    return GRTCODE_SUCCESS;
}

/* what a key may be for groups of rows_per_group rows (`name`: whose key, for the messages); *row: the key row, -1: the sum */
int grt_kdist_check_key(char const *name, int kind, long long key_row, long long rows_per_group, long long *row)
{
    if (kind != GRT_KDIST_KEY_ROW && kind != GRT_KDIST_KEY_SUM)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s key kind %d: GRT_KDIST_KEY_ROW (%d) or GRT_KDIST_KEY_SUM (%d).", name, kind,
                 GRT_KDIST_KEY_ROW, GRT_KDIST_KEY_SUM);
    }
    if (kind == GRT_KDIST_KEY_ROW && (key_row < 0 || key_row >= rows_per_group))
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s key row %lld: 0 to %lld.", name, key_row, rows_per_group - 1);
    }
    *row = kind == GRT_KDIST_KEY_ROW ? key_row : -1;
    return GRTCODE_SUCCESS;
}

/* the correlated reduction of tau_dev [groups][rows_per_group][n], every argument checked already: the map of the key
   (key_row, < 0: the sum) to map_dev, then every row under it into band's outputs */
int grt_kdist_reduce_correlated(Device_t device, GrtKdistTable *t, fp_t const *tau_dev, long long groups,
                                long long rows_per_group, long long n, fp_t dw, int num_classes, fp_t const *class_edges,
                                long long key_row, unsigned short *map_dev, GrtKdistBand_t const *band)
{
    size_t const ne = (size_t)num_classes - 1, nw = band->weight != NULL ? (size_t)n : 0;
    GRT_TRY(kdist_table(device, t, class_edges, ne, band->weight, nw, band->edges, (size_t)band->num_bins));
    double const *doubles = t->block;
    GRT_TRY(launch_map(device, doubles, tau_dev, groups, rows_per_group, n, key_row, num_classes, map_dev));
    GRT_TRY(launch_mapped(device, tau_dev, rows_per_group*n, map_dev, groups, rows_per_group, n, dw, num_classes,
                          nw > 0 ? doubles + ne : NULL, (int const *)(doubles + ne + nw), band));
    return GRTCODE_SUCCESS;
}

int grt_kdist_reduce_ck(Device_t device, GrtKdistTable *t, fp_t const *tau_dev, long long groups, long long rows_per_group,
                        long long n, fp_t dw, int num_classes, fp_t const *class_edges, long long key_row,
                        unsigned short const *map_given_dev, unsigned short *map_dev, GrtKdistBand_t const *band,
                        int const **edges_dev)
{
    size_t const ne = class_edges != NULL ? (size_t)num_classes - 1 : 0;
    GRT_TRY(kdist_table(device, t, class_edges, ne, NULL, 0, band->edges, (size_t)band->num_bins));
    double const *doubles = t->block;
    *edges_dev = (int const *)(doubles + ne);
    if (map_given_dev == NULL)
    {
        GRT_TRY(launch_map(device, doubles, tau_dev, groups, rows_per_group, n, key_row, num_classes, map_dev));
    }
    GRT_TRY(launch_mapped(device, tau_dev, rows_per_group*n, map_given_dev != NULL ? map_given_dev : map_dev, groups,
                          rows_per_group, n, dw, num_classes, NULL, *edges_dev, band));
    return GRTCODE_SUCCESS;
}

static int check_groups(long long groups, long long rows_per_group, long long n)
{
    if (groups < 1 || rows_per_group < 1 || n < 2)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%lld groups of %lld rows of %lld points: at least 1 group of at least 1 row of at "
                 "least 2 points.", groups, rows_per_group, n);
    }
    return GRTCODE_SUCCESS;
}

EXTERN int grt_kdist_class_map(Device_t device, fp_t const *x_dev, long long groups, long long rows_per_group, long long n,
                               int key_kind, long long key_row, int num_classes, fp_t const *class_edges,
                               unsigned short *map_dev)
{
    if (x_dev == NULL || map_dev == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s is NULL.", x_dev == NULL ? "x_dev" : "map_dev");
    }
    GRT_TRY(grt_kdist_check_classes(num_classes, class_edges));
    GRT_TRY(check_groups(groups, rows_per_group, n));
    long long row;
    GRT_TRY(grt_kdist_check_key("the", key_kind, key_row, rows_per_group, &row));
    GRT_TRY(grt_dev_require(device));
    GrtKdistTable *t = &g_map_table[device];
    GRT_TRY(kdist_table(device, t, class_edges, (size_t)num_classes - 1, NULL, 0, NULL, 0));
    GRT_TRY(launch_map(device, t->block, x_dev, groups, rows_per_group, n, row, num_classes, map_dev));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_kdist_mapped_rows(Device_t device, fp_t const *values_dev, long long group_stride,
                                 unsigned short const *map_dev, long long groups, long long rows_per_group, long long n,
                                 fp_t dw, int num_classes, GrtKdistBand_t const *band)
{
    if (values_dev == NULL || map_dev == NULL || band == NULL)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%s is NULL.", values_dev == NULL ? "values_dev" : map_dev == NULL ? "map_dev" : "band");
    }
    if (num_classes < 2 || num_classes > GRT_KDIST_MAX_CLASSES)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "%d classes asked for: 2 to %d.", num_classes, GRT_KDIST_MAX_CLASSES);
    }
    GRT_TRY(check_groups(groups, rows_per_group, n));
    /* (in this order: rows_per_group n cannot overflow where the stride holds it) */
    if (group_stride/rows_per_group < n || group_stride < rows_per_group*n)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "a group stride of %lld doubles for %lld rows of %lld points: at least their product.",
                 group_stride, rows_per_group, n);
    }
    if (!(dw > 0.) || !isfinite(dw))
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "grid spacing (%e) is not positive and finite.", dw);
    }
    GRT_TRY(grt_check_bin_edges("row", band->edges, band->num_bins, n, 1));
    if (band->num_bins == 0)
    {
        GRT_FAIL(GRTCODE_VALUE_ERR, "no bins: nothing to write.%s", "");
    }
    GRT_TRY(grt_kdist_check_band("row", band, n));
    GRT_TRY(grt_dev_require(device));
    GrtKdistTable *t = &g_mapped_table[device];
    size_t const nw = band->weight != NULL ? (size_t)n : 0;
    GRT_TRY(kdist_table(device, t, NULL, 0, band->weight, nw, band->edges, (size_t)band->num_bins));
    double const *doubles = t->block;
    GRT_TRY(launch_mapped(device, values_dev, group_stride, map_dev, groups, rows_per_group, n, dw, num_classes,
                          nw > 0 ? doubles : NULL, (int const *)(doubles + nw), band));
    return GRTCODE_SUCCESS;
}

EXTERN int grt_kdist_chunk_points(void)
{
    return grt_kdist_chunk();
}
