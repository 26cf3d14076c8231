/* rfmip_batch_driver.c -- a netCDF-free, batched counterpart of rfmip-irf/src/rfmip-irf.c + framework/src/driver.c
 * for clear-sky columns, using the device-resident pipeline of include/grt_ext.h instead of the per-column loop of
 * driver.c:691-743.
 *
 * What it keeps of the reference's data preparation (rfmip-irf.c):
 *   - pressures arrive in Pa and are used in mb (:175-200, x 0.01);
 *   - water vapour and ozone arrive as LAYER mole fractions and are interpolated to levels in pressure, end levels
 *     copied (:290-308); the well-mixed gases are one global-mean value per experiment (:310-325);
 *   - cos(zenith) from degrees, columns with the sun below the horizon get no shortwave (driver.c:706);
 *   - a spectrally constant surface albedo / emissivity (the two-point "constant" grids of :221-256 with
 *     constant_extrapolation, driver.c:102-115): one value for the whole run, the last column's, or -- with
 *     -surface-per-column -- each column's own, as the reference application takes them;
 *   - N2 for the collision-induced absorption at 0.781 (driver.c: set_cia_ppmv with a constant profile).
 *
 * Input file (little-endian, our own flat dump standing in for multiple_input4MIPs_radiation_RFMIP_*.nc):
 *   int32 magic 0x47525443 ("GRTC"), int32 ncol, int32 nlev,
 *   float64 global-mean mole fractions [5]: CO2, CH4, N2O, CO, O2,
 *   then per column: level_pressure_Pa[nlev], layer_pressure_Pa[nlev-1], level_temperature[nlev],
 *   layer_temperature[nlev-1], surface_temperature, surface_emissivity, surface_albedo, solar_zenith_angle_deg,
 *   total_solar_irradiance, h2o_layer[nlev-1], o3_layer[nlev-1]   (all float64).
 *
 * Usage:  rfmip_batch_driver HITRAN.par SOLAR.csv COLUMNS.bin [-h2o-ctm DIR] [-o3-ctm FILE] [-CFC-11 FILE ppmv]
 *             [-CFC-12 FILE ppmv] [-N2-N2 FILE] [-O2-N2 FILE] [-O2-O2 FILE] [-w-lw W0 -W-lw WN -r-lw DW]
 *             [-w-sw W0 -W-sw WN -r-sw DW] [-chunk N] [-fast 0|1|2|3] [-d DEVICE]
 *             [-ranks N -rank K -rendezvous DIR [-transport rccl|files]] [-profiles] [-bin-width DW] [-surface-per-column]
 * Output: one line per column "col <i>: rlut rlus rldt rlds rsut rsus rsdt rsds" [W m-2] (zeros for the shortwave
 * of night columns).  With -profiles each column's line is followed by its broadband fluxes at every level, top first,
 * "lev <k>: rlu rld rsu rsd" [W m-2], and the heating rate of every layer, "lay <j>: hr_lw hr_sw" [K day-1]
 * (grt_pipeline_run_profiles; its shortwave is the two-sweep form, so lev 0's rsu may differ from the col line's rsut
 * in the last digits).
 * With -bin-width DW each column's line is followed by its fluxes integrated over wavenumber bins of round(DW/dw) grid
 * points from each band's first point (the last bin shorter; adjacent bins share their edge point),
 * "lwbin <b>: w_lo w_hi rlut rlus rldt rlds" and "swbin <b>: w_lo w_hi rsut rsus rsdt rsds" [cm-1, W m-2]
 * (grt_pipeline_run_spectral; night columns get zeros in their shortwave bins).
 * With -surface-per-column every column is solved over its own surface_emissivity and surface_albedo: per chunk the
 * two-point grids of rfmip-irf.c:221-256 go to the chunk's pipeline with grt_pipeline_set_surface.  Without it the last
 * column's two values serve all columns.
 *
 * Several GPUs of one node: start one process per GPU with the same arguments plus -ranks N -rank K (K = 0..N-1,
 * normally with -d K) and a directory all of them see.  Every rank computes its contiguous block of the columns
 * (grt_multi_shard -- the in-node form of run-rfmip-irf.sh's -x/-X fan-out, GRTworkflow/run-rfmip-irf.sh:103-132) and
 * one gather brings the flux blocks to rank 0, which prints all columns: ncclGather over xGMI (-transport rccl, the
 * default) or per-rank files in the rendezvous directory (-transport files: the reference's per-shard outputs +
 * combiner in one step; also how several ranks share one GPU in tests).
 *
 * Each kind of result (the 12 fluxes, -profiles rows, -bin-width rows) is one Kind entry below: its row length, its
 * buffers and the function that runs a chunk.  Allocation, the per-chunk scatter, the gather and the frees loop over
 * the entries, so a further kind is one more entry and its run function.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "grt_ext.h"
#ifdef GRT_BACKTRACE    /* -DGRT_BACKTRACE -rdynamic: a fatal signal prints where it happened (tests build it that way) */
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>
static void fatal_signal(int sig)
{
    void *frames[64];
    int const n = backtrace(frames, 64);
    char const msg[] = "rfmip_batch_driver: fatal signal, backtrace:\n";
    if (write(2, msg, sizeof(msg) - 1) < 0) _exit(128 + sig);
    backtrace_symbols_fd(frames, n, 2);
    signal(sig, SIG_DFL);
    raise(sig);
}
#endif

#include "example_support.h"

enum { FLUXES, PROFILES, BINS, NUM_KINDS };

/* what a run function needs besides its own kind */
typedef struct Run
{
    Device_t device;
    int V, L, chunk;
    SpectralGrid_t const *grids[2];             /* longwave, shortwave */
    int *edges[2], nb[2];                       /* -bin-width: grid-point edges and bin counts of the two bands */
    GrtPipeline_t *pipe[2];                     /* day, night */
    int surface_per_column;                     /* -surface-per-column */
} Run;

/* One kind of result: `row` doubles per column.  run() sends a chunk of m columns through the pipeline and leaves m rows
 * in `host`, *stride doubles apart, of which the first *keep are this class's (day or night) to take. */
typedef struct Kind
{
    char const *name;
    int row, enabled;
    size_t dev_doubles[3];                      /* per column, of the device buffers this kind needs (0: none) */
    fp_t *dev[3], *host, *all;                  /* device buffers and host staging of a chunk; [columns][row] of the run */
    int (*run)(struct Kind *kind, Run const *r, GrtColumns_t const *cols, int night, size_t *stride, size_t *keep);
} Kind;

/* the host arrays of GrtColumns_t, for all the columns of the file or for one chunk */
typedef struct Columns
{
    double *p, *t, *tl, *ts, *mu, *tsi, *mol, *cfc, *cia;
    double *emis, *alb;                         /* [n][2]: each column's value at the two points of the constant grid */
} Columns;

/* -bin-width: grid-point edges every round(width/dw) points from 0, the last at n - 1; returns the bin count */
static int bin_edges(SpectralGrid_t const *grid, double width, int **edges)
{
    long long k = llround(width/grid->dw);
    k = k < 1 ? 1 : k;
    long long const n = (long long)grid->n;
    int const nb = (int)((n - 1 + k - 1)/k);
    *edges = malloc(sizeof(int)*((size_t)nb + 1));
    for (int b = 0; b < nb; ++b)
    {
        (*edges)[b] = (int)(b*k);
    }
    (*edges)[nb] = (int)(n - 1);
    return nb;
}

/* ---- the three kinds ---------------------------------------------------------------------------------------------- */
static int run_fluxes(Kind *k, Run const *r, GrtColumns_t const *cols, int night, size_t *stride, size_t *keep)
{
    check(grt_pipeline_run(r->pipe[night], cols, k->dev[0]));
    check(grt_pipeline_sync(r->pipe[night]));
    check(grt_device_to_host(r->device, k->host, k->dev[0], sizeof(fp_t)*cols->ncol*GRT_FLUXES_PER_COLUMN));
    *stride = GRT_FLUXES_PER_COLUMN;
    *keep = night ? GRT_FLUXES_PER_BAND : GRT_FLUXES_PER_COLUMN;
    return EXIT_SUCCESS;
}

/* per column the level fluxes [4][V] and then the heating rates [2][L]; the two come back in device buffers of their own
 * (the night pipeline has no shortwave band: its shortwave rows come back zero) */
static int run_profiles(Kind *k, Run const *r, GrtColumns_t const *cols, int night, size_t *stride, size_t *keep)
{
    int const m = cols->ncol;
    size_t const nl = (size_t)GRT_PROFILE_ROWS_PER_COLUMN*r->V, nh = (size_t)GRT_HEATING_ROWS_PER_COLUMN*r->L;
    fp_t *levels = k->host + (size_t)r->chunk*k->row, *heating = levels + (size_t)r->chunk*nl;
    check(grt_pipeline_run_profiles(r->pipe[night], cols, k->dev[0], k->dev[1], NULL));
    check(grt_pipeline_sync(r->pipe[night]));
    check(grt_device_to_host(r->device, levels, k->dev[0], sizeof(fp_t)*m*nl));
    check(grt_device_to_host(r->device, heating, k->dev[1], sizeof(fp_t)*m*nh));
    for (int j = 0; j < m; ++j)
    {
        memcpy(k->host + (size_t)j*k->row, levels + j*nl, sizeof(fp_t)*nl);
        memcpy(k->host + (size_t)j*k->row + nl, heating + j*nh, sizeof(fp_t)*nh);
    }
    *stride = *keep = (size_t)k->row;
    return EXIT_SUCCESS;
}

/* per column the longwave bins [6][nb_lw] and then the shortwave bins [6][nb_sw]
 * (the night pipeline has no shortwave band: it takes no shortwave bins, its rows are shorter, and the rest stays zero) */
static int run_bins(Kind *k, Run const *r, GrtColumns_t const *cols, int night, size_t *stride, size_t *keep)
{
    int const row = night ? 6*r->nb[0] : k->row;
    check(grt_pipeline_run_spectral(r->pipe[night], cols, NULL, r->edges[0], r->nb[0], night ? NULL : r->edges[1],
                                    night ? 0 : r->nb[1], k->dev[0], k->dev[1], k->dev[2]));
    check(grt_pipeline_sync(r->pipe[night]));
    check(grt_device_to_host(r->device, k->host, k->dev[1], sizeof(fp_t)*cols->ncol*row));
    *stride = *keep = (size_t)row;
    return EXIT_SUCCESS;
}

/* ---- the steps of main -------------------------------------------------------------------------------------------- */
static double *read_dump(char const *path, int *ncol, int *V, double gm[5], size_t *per_col)
{
    FILE *f = fopen(path, "rb");
    if (f == NULL)
    {
        fprintf(stderr, "cannot open %s\n", path);
        return NULL;
    }
    int header[3];
    if (fread(header, sizeof(int), 3, f) != 3 || header[0] != 0x47525443 || fread(gm, sizeof(double), 5, f) != 5)
    {
        fprintf(stderr, "%s is not a GRTC column dump\n", path);
        return NULL;
    }
    *ncol = header[1];
    *V = header[2];
    int const L = *V - 1;
    *per_col = (size_t)*V + L + *V + L + 5 + 2*(size_t)L;
    double *raw = malloc(sizeof(double)**per_col**ncol);
    if (fread(raw, sizeof(double), *per_col**ncol, f) != *per_col*(size_t)*ncol)
    {
        fprintf(stderr, "%s is truncated\n", path);
        return NULL;
    }
    fclose(f);
    return raw;
}

/* the longwave and the shortwave gas optics (driver.c:617-625, 193-211); the CFCs asked for and their ppmv */
static int build_gas_optics(int argc, char **argv, GasOptics_t lbl[2], int V, SpectralGrid_t const *const grids[2],
                            Device_t const *device, int *ncfc, double cfc_ppmv[2])
{
    int const method = line_sample, fast = (int)number(argc, argv, "-fast", 3.);
    for (int b = 0; b < 2; ++b)
    {
        check(create_gas_optics(&lbl[b], V, grids[b], device, argv[1], option(argc, argv, "-h2o-ctm", 1),
                                option(argc, argv, "-o3-ctm", 1), NULL, &method));
        for (int k = 0; k < 7; ++k)
        {
            check(add_molecule(&lbl[b], hitran_id[k], NULL, NULL));
        }
        *ncfc = 0;
        for (int k = 0; k < 2; ++k)
        {
            if (option(argc, argv, cfc_flags[k].flag, 1))
            {
                check(add_cfc(&lbl[b], cfc_flags[k].id, option(argc, argv, cfc_flags[k].flag, 1)));
                cfc_ppmv[(*ncfc)++] = atof(option(argc, argv, cfc_flags[k].flag, 2));
            }
        }
        for (int k = 0; k < 3; ++k)
        {
            if (option(argc, argv, cia_flags[k].flag, 1))
            {
                check(add_cia(&lbl[b], cia_flags[k].s1, cia_flags[k].s2, option(argc, argv, cia_flags[k].flag, 1)));
            }
        }
        check(grt_gas_optics_tune(&lbl[b], 0, 0, fast));
    }
    return EXIT_SUCCESS;
}

static Columns alloc_columns(int n, int V)
{
    int const L = V - 1;
    Columns c = {malloc(sizeof(double)*n*V), malloc(sizeof(double)*n*V), malloc(sizeof(double)*n*L),
                 malloc(sizeof(double)*n), malloc(sizeof(double)*n), malloc(sizeof(double)*n),
                 malloc(sizeof(double)*n*7*V), malloc(sizeof(double)*(n*2*V + 1)), malloc(sizeof(double)*n*NUM_CIAS*V),
                 malloc(sizeof(double)*n*2), malloc(sizeof(double)*n*2)};
    return c;
}

static void free_columns(Columns *c)
{
    free(c->p); free(c->t); free(c->tl); free(c->ts); free(c->mu); free(c->tsi); free(c->mol); free(c->cfc); free(c->cia);
    free(c->emis); free(c->alb);
}

/* the buffers of the enabled kinds: for a chunk on the device and on the host, for `rows` columns (all ranks' blocks) */
static int allocate_kinds(Run const *r, Kind *kinds, size_t rows)
{
    for (Kind *k = kinds; k < kinds + NUM_KINDS; ++k)
    {
        if (!k->enabled) continue;
        for (int d = 0; d < 3; ++d)
        {
            if (k->dev_doubles[d]) check(grt_device_malloc(r->device, (void **)&k->dev[d], sizeof(fp_t)*r->chunk*k->dev_doubles[d]));
        }
        /* (the profiles stage their two device buffers behind the chunk's rows: twice the rows) */
        k->host = malloc(sizeof(fp_t)*r->chunk*k->row*2);
        k->all = calloc(rows*k->row, sizeof(fp_t));
    }
    return EXIT_SUCCESS;
}

static int free_kinds(Run const *r, Kind *kinds)
{
    for (Kind *k = kinds; k < kinds + NUM_KINDS; ++k)
    {
        for (int d = 0; d < 3 && k->enabled; ++d)
        {
            if (k->dev_doubles[d]) check(grt_device_free(r->device, k->dev[d]));
        }
        free(k->host);
        free(k->all);
    }
    return EXIT_SUCCESS;
}

/* raw columns -> the batched layout of GrtColumns_t.  Every column's own surface emissivity and albedo are kept, at both
 * points of the two-point constant grid (rfmip-irf.c:221-256), for -surface-per-column; *emis_value and *albedo_value are
 * the LAST column's: without that flag one value serves the whole run, like the app's -e / -a, whatever the other columns
 * of the file say. */
static Columns prepare_columns(double const *raw, size_t per_col, int ncol, int V, double const gm[5], int ncfc,
                               double const cfc_ppmv[2], double *emis_value, double *albedo_value)
{
    int const L = V - 1;
    Columns a = alloc_columns(ncol, V);
    double *pl = malloc(sizeof(double)*L);
    for (int c = 0; c < ncol; ++c)
    {
        double const *r = raw + per_col*c;
        double const *plev = r, *play = r + V, *tlev = play + L, *tlay = tlev + V, *scal = tlay + L;
        double const *h2o = scal + 5, *o3 = h2o + L;
        for (int k = 0; k < V; ++k)
        {
            a.p[c*V + k] = plev[k]*0.01;                            /* Pa -> mb (rfmip-irf.c:186) */
            a.t[c*V + k] = tlev[k];
        }
        for (int k = 0; k < L; ++k)
        {
            pl[k] = play[k]*0.01;
            a.tl[c*L + k] = tlay[k];
        }
        a.ts[c] = scal[0];
        *emis_value = a.emis[2*c] = a.emis[2*c + 1] = scal[1];
        *albedo_value = a.alb[2*c] = a.alb[2*c + 1] = scal[2];
        a.mu[c] = cos(2.*M_PI*scal[3]/360.);
        a.tsi[c] = scal[4];
        double *m = a.mol + (size_t)c*7*V;
        layers_to_levels(m + 0*V, h2o, L, pl, a.p + c*V);            /* rfmip-irf.c:295-308 */
        layers_to_levels(m + 2*V, o3, L, pl, a.p + c*V);
        int const gm_slot[5] = {1, 5, 3, 4, 6};                      /* CO2, CH4, N2O, CO, O2 in hitran_id order */
        for (int g = 0; g < 5; ++g)
        {
            for (int k = 0; k < V; ++k)
            {
                m[gm_slot[g]*V + k] = gm[g]*1.e6;
            }
        }
        for (int k = 0; k < V; ++k)
        {
            for (int j = 0; j < ncfc; ++j)
            {
                a.cfc[((size_t)c*ncfc + j)*V + k] = cfc_ppmv[j];
            }
            a.cia[((size_t)c*NUM_CIAS + CIA_N2)*V + k] = 0.781e6;
            a.cia[((size_t)c*NUM_CIAS + CIA_O2)*V + k] = gm[4]*1.e6;
        }
    }
    free(pl);
    return a;
}

/* One class of this rank's columns (day or night; they go through different pipelines), in chunks that are contiguous
 * in the class: gather the chunk's columns (they need not be adjacent in the file), run every kind, scatter its rows. */
static int run_class(Run const *r, Kind *kinds, Columns const *a, Columns *c, int ncfc, int const *ids, int n, int night)
{
    int const V = r->V, L = r->L;
    for (int first = 0; first < n; first += r->chunk)
    {
        int const m = n - first < r->chunk ? n - first : r->chunk;
        for (int j = 0; j < m; ++j)
        {
            int const i = ids[first + j];
            memcpy(c->p + j*V, a->p + i*V, sizeof(double)*V);
            memcpy(c->t + j*V, a->t + i*V, sizeof(double)*V);
            memcpy(c->tl + j*L, a->tl + i*L, sizeof(double)*L);
            c->ts[j] = a->ts[i]; c->mu[j] = a->mu[i]; c->tsi[j] = a->tsi[i];
            memcpy(c->emis + 2*j, a->emis + 2*i, sizeof(double)*2);
            memcpy(c->alb + 2*j, a->alb + 2*i, sizeof(double)*2);
            memcpy(c->mol + (size_t)j*7*V, a->mol + (size_t)i*7*V, sizeof(double)*7*V);
            memcpy(c->cfc + (size_t)j*ncfc*V, a->cfc + (size_t)i*ncfc*V, sizeof(double)*ncfc*V);
            memcpy(c->cia + (size_t)j*NUM_CIAS*V, a->cia + (size_t)i*NUM_CIAS*V, sizeof(double)*NUM_CIAS*V);
        }
        GrtColumns_t cols = {m, V, c->p, c->t, c->tl, c->ts, c->mol, ncfc ? c->cfc : NULL, c->cia, c->mu, c->tsi};
        if (r->surface_per_column)
        {
            /* the chunk's own surface, on the constant grids of rfmip-irf.c:221-256: every grid point lies above them and
               takes the value constant_extrapolation finds there (the night pipeline has no shortwave: no albedo) */
            static fp_t const constant_grid[2] = {-1., 0.};
            GrtSurface_t const surface = {.ncol = m, .emissivity_num_points = 2, .albedo_num_points = 2,
                                          .emissivity_grid = constant_grid, .albedo_grid = constant_grid,
                                          .emissivity = c->emis, .direct_albedo = c->alb, .diffuse_albedo = NULL};
            check(grt_pipeline_set_surface(r->pipe[night], &surface));
        }
        for (Kind *k = kinds; k < kinds + NUM_KINDS; ++k)
        {
            if (!k->enabled) continue;
            size_t stride = 0, keep = 0;
            if (k->run(k, r, &cols, night, &stride, &keep)) return EXIT_FAILURE;
            for (int j = 0; j < m; ++j)
            {
                memcpy(k->all + (size_t)ids[first + j]*k->row, k->host + j*stride, sizeof(fp_t)*keep);
            }
        }
    }
    return EXIT_SUCCESS;
}

/* one gather per kind of this rank's block of rows to rank 0: between host buffers with the file transport,
 * between device buffers, on the library stream, with RCCL */
static int gather(Run const *r, Kind *kinds, GrtMulti_t *multi, int files, int ncol, int rank, int world, int shard_first,
                  int shard_count)
{
    size_t const per_rank = (size_t)((ncol + world - 1)/world);
    for (Kind *k = kinds; k < kinds + NUM_KINDS; ++k)
    {
        if (!k->enabled) continue;
        size_t const block = sizeof(fp_t)*per_rank*k->row, mine = sizeof(fp_t)*(size_t)shard_count*k->row;
        fp_t *local = k->all + (size_t)shard_first*k->row, *all = NULL;
        if (files)
        {
            all = rank == 0 ? calloc(per_rank*world*k->row, sizeof(fp_t)) : NULL;
        }
        else
        {
            fp_t *host = local;
            local = NULL;
            check(grt_device_malloc(r->device, (void **)&local, block));
            if (rank == 0) check(grt_device_malloc(r->device, (void **)&all, block*world));
            if (shard_count > 0) check(grt_host_to_device(r->device, local, host, mine));
        }
        check(grt_multi_gather_rows(multi, local, ncol, k->row, all, !files));
        if (files)
        {
            if (rank == 0) memcpy(k->all, all, sizeof(fp_t)*(size_t)ncol*k->row);
            free(all);
        }
        else
        {
            check(grt_pipeline_sync(r->pipe[0]));          /* the gather runs on the library stream */
            if (rank == 0) check(grt_device_to_host(r->device, k->all, all, sizeof(fp_t)*(size_t)ncol*k->row));
            check(grt_device_free(r->device, local));
            check(grt_device_free(r->device, all));
        }
    }
    return EXIT_SUCCESS;
}

static void print_columns(Run const *r, Kind const *kinds, int ncol)
{
    int const V = r->V, L = r->L;
    for (int c = 0; c < ncol; ++c)
    {
        fp_t const *x = kinds[FLUXES].all + (size_t)c*GRT_FLUXES_PER_COLUMN;
        printf("col %d: %.15e %.15e %.15e %.15e %.15e %.15e %.15e %.15e\n", c, x[0], x[1], x[3], x[4], x[6], x[7], x[9], x[10]);
        for (int band = 0; band < 2 && kinds[BINS].enabled; ++band)
        {
            /* the band's six rows [6][nb] of this column: up TOA, up surface, up user, down TOA, down surface, down user */
            int const nb = r->nb[band];
            fp_t const *row = kinds[BINS].all + (size_t)c*kinds[BINS].row + (band ? 6*r->nb[0] : 0);
            SpectralGrid_t const *g = r->grids[band];
            for (int b = 0; b < nb; ++b)
            {
                printf("%s %d: %.15e %.15e %.15e %.15e %.15e %.15e\n", band ? "swbin" : "lwbin", b,
                       g->w0 + r->edges[band][b]*g->dw, g->w0 + r->edges[band][b + 1]*g->dw, row[b], row[nb + b],
                       row[3*nb + b], row[4*nb + b]);
            }
        }
        if (kinds[PROFILES].enabled)
        {
            fp_t const *row = kinds[PROFILES].all + (size_t)c*kinds[PROFILES].row, *h = row + GRT_PROFILE_ROWS_PER_COLUMN*V;
            for (int k = 0; k < V; ++k)
            {
                printf("lev %d: %.15e %.15e %.15e %.15e\n", k, row[k], row[V + k], row[2*V + k], row[3*V + k]);
            }
            for (int j = 0; j < L; ++j)
            {
                printf("lay %d: %.15e %.15e\n", j, h[j], h[L + j]);
            }
        }
    }
}

int main(int argc, char **argv)
{
#ifdef GRT_BACKTRACE
    signal(SIGSEGV, fatal_signal);
    signal(SIGBUS, fatal_signal);
    signal(SIGFPE, fatal_signal);
    signal(SIGABRT, fatal_signal);
#endif
    if (argc < 4)
    {
        fprintf(stderr, "usage: %s HITRAN.par SOLAR.csv COLUMNS.bin [options]\n", argv[0]);
        return EXIT_FAILURE;
    }
    int ncol, V;
    double gm[5];
    size_t per_col;
    double *raw = read_dump(argv[3], &ncol, &V, gm, &per_col);
    if (raw == NULL)
    {
        return EXIT_FAILURE;
    }
    int const L = V - 1;

    /* grids, device, gas optics (driver.c:912-931) */
    SpectralGrid_t lw_grid, sw_grid;
    check(create_spectral_grid(&lw_grid, number(argc, argv, "-w-lw", 1.), number(argc, argv, "-W-lw", 3250.),
                               number(argc, argv, "-r-lw", 1.)));
    check(create_spectral_grid(&sw_grid, number(argc, argv, "-w-sw", 1.), number(argc, argv, "-W-sw", 50000.),
                               number(argc, argv, "-r-sw", 1.)));
    Device_t device;
    int dev_id = (int)number(argc, argv, "-d", 0.);
    check(create_device(&device, option(argc, argv, "-d", 1) ? &dev_id : NULL));
    Run r = {.device = device, .V = V, .L = L, .chunk = (int)number(argc, argv, "-chunk", 16.), .grids = {&lw_grid, &sw_grid},
             .surface_per_column = option(argc, argv, "-surface-per-column", 0) != NULL};
    GasOptics_t lbl[2];
    int ncfc = 0;
    double cfc_ppmv[2] = {0., 0.};
    if (build_gas_optics(argc, argv, lbl, V, r.grids, &device, &ncfc, cfc_ppmv))
    {
        return EXIT_FAILURE;
    }
    SolarFlux_t solar;
    check(create_solar_flux(&solar, &sw_grid, argv[2]));

    double emis_value = 0., albedo_value = 0.;
    Columns all = prepare_columns(raw, per_col, ncol, V, gm, ncfc, cfc_ppmv, &emis_value, &albedo_value);
    free(raw);
    Columns part = alloc_columns(r.chunk, V);
    fp_t *emissivity = malloc(sizeof(fp_t)*lw_grid.n), *albedo = malloc(sizeof(fp_t)*sw_grid.n);
    for (uint64_t i = 0; i < lw_grid.n; ++i) emissivity[i] = emis_value;
    for (uint64_t i = 0; i < sw_grid.n; ++i) albedo[i] = albedo_value;
    check(grt_pipeline_create(&r.pipe[0], &lbl[0], &lbl[1], r.chunk, -1, emissivity, albedo, solar.incident_flux));
    check(grt_pipeline_create(&r.pipe[1], &lbl[0], NULL, r.chunk, -1, emissivity, NULL, NULL));

    /* the kinds of result: the 12 fluxes always, -profiles and -bin-width on request */
    double const bin_width = number(argc, argv, "-bin-width", 0.);
    for (int b = 0; b < 2 && bin_width > 0.; ++b)
    {
        r.nb[b] = bin_edges(r.grids[b], bin_width, &r.edges[b]);
    }
    size_t const nl = (size_t)GRT_PROFILE_ROWS_PER_COLUMN*V, nh = (size_t)GRT_HEATING_ROWS_PER_COLUMN*L;
    Kind kinds[NUM_KINDS] = {
        [FLUXES] = {"fluxes", GRT_FLUXES_PER_COLUMN, 1, {GRT_FLUXES_PER_COLUMN}, .run = run_fluxes},
        [PROFILES] = {"profiles", (int)(nl + nh), option(argc, argv, "-profiles", 0) != NULL, {nl, nh}, .run = run_profiles},
        [BINS] = {"bins", 6*(r.nb[0] + r.nb[1]), bin_width > 0.,
                  {6*(lw_grid.n + sw_grid.n), 6*(size_t)(r.nb[0] + r.nb[1]), GRT_FLUXES_PER_COLUMN}, .run = run_bins}};

    /* this rank's block of the columns */
    int const world = (int)number(argc, argv, "-ranks", 1.), rank = (int)number(argc, argv, "-rank", 0.);
    char const *tr = option(argc, argv, "-transport", 1);
    int const files = tr != NULL && strcmp(tr, "files") == 0;
    int shard_first = 0, shard_count = ncol;
    GrtMulti_t *multi = NULL;
    if (world > 1)
    {
        char const *dir = option(argc, argv, "-rendezvous", 1);
        if (dir == NULL)
        {
            fprintf(stderr, "-ranks needs -rendezvous DIR\n");
            return EXIT_FAILURE;
        }
        check(grt_multi_create(&multi, files ? GRT_MULTI_FILES : GRT_MULTI_RCCL, device, rank, world, dir));
        check(grt_multi_shard(ncol, rank, world, &shard_first, &shard_count));
    }
    if (allocate_kinds(&r, kinds, (size_t)((ncol + world - 1)/world)*world))
    {
        return EXIT_FAILURE;
    }

    int *ids = malloc(sizeof(int)*ncol);
    for (int night = 0; night < 2; ++night)
    {
        int n = 0;
        for (int c = shard_first; c < shard_first + shard_count; ++c)
        {
            if ((all.mu[c] <= 0.) == (night == 1)) ids[n++] = c;
        }
        if (run_class(&r, kinds, &all, &part, ncfc, ids, n, night))
        {
            return EXIT_FAILURE;
        }
    }
    free(ids);
    free_columns(&part);
    free_columns(&all);
    if (multi != NULL)
    {
        if (gather(&r, kinds, multi, files, ncol, rank, world, shard_first, shard_count))
        {
            return EXIT_FAILURE;
        }
        double seconds = 0.;
        check(grt_multi_max(multi, &seconds));             /* everybody is done before anybody tears down */
        check(grt_multi_destroy(&multi));
    }
    if (rank == 0)
    {
        print_columns(&r, kinds, ncol);
    }
    check(grt_pipeline_destroy(&r.pipe[0]));
    check(grt_pipeline_destroy(&r.pipe[1]));
    if (free_kinds(&r, kinds))
    {
        return EXIT_FAILURE;
    }
    free(r.edges[0]);
    free(r.edges[1]);
    check(destroy_solar_flux(&solar));
    check(destroy_gas_optics(&lbl[0]));
    check(destroy_gas_optics(&lbl[1]));
    return EXIT_SUCCESS;
}
