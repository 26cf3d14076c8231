/* grt_pipeline_solve.c -- the solves of one band of the batched pipeline on the run's tau_gas, each described by a GrtPass:
 * the solver launch, the materialised optics that precede it when spectra are kept, and what turns its partial sums or
 * spectral fluxes into the rows the caller asked for. */
#include <stdlib.h>
#include <string.h>
#include "grt_pipeline_internal.h"

/* the profile tag its solver is timed under */
static int pass_tag(GrtPass const *ps, int bi)
{
    static int const tag[4][2] = {{GRT_TAG_SOLVER_LW, GRT_TAG_SOLVER_SW}, {GRT_TAG_ALLSKY_LW, GRT_TAG_ALLSKY_SW},
                                  {GRT_TAG_AEROSOL_LW, GRT_TAG_AEROSOL_SW}, {GRT_TAG_SKY_LW, GRT_TAG_SKY_SW}};
    return tag[(ps->aer_pass ? 2 : 0) + (ps->clouds != NULL)][bi];
}

/* the six rows at every point leave too (grt_pipeline_run_spectral) */
static int pass_spectral(GrtPass const *ps)
{
    return ps->bins != NULL && !ps->profile;
}

/* The third row group of a pass beside its up and down rows: the shortwave's direct beam (grt_pipeline_run_sky_direct) or
   the longwave's surface-temperature Jacobian (grt_pipeline_run_sky_jacobian) -- each band has at most one, so both go
   one way through this file and share the band's scratch blocks.  The fused form's partial sums of it, as the join of
   whichever band it is (partials NULL: the pass leaves none) */
typedef struct ThirdRows
{
    double *partials;
    GrtDirectArgs direct;
    GrtJacobianArgs jacobian;
    /* grt_pipeline_run_sky_weighted: the band's response rows leave too (response_partials; with_responses 0: they do not) */
    int with_responses;
    GrtResponseArgs responses;
} ThirdRows;

/* its solver instance (materialised: the spectral form, after pass_optics); bn: its per-bin instance; sc: the pass's
   clouds as the subcolumns of sc; tr: band bi's instance that leaves the third row group too */
static GrtSolverInstance pass_instance(GrtPipeline_t const *p, GrtPass const *ps, GrtBandArgs const *bn,
                                       GrtSubcolumnArgs const *sc, ThirdRows const *tr, int bi)
{
    GrtSolverInstance in = {GRT_OUT_CHAINS, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL};
    if (!p->keep_spectra)
    {
        in.out = pass_spectral(ps) ? GRT_OUT_ROWS_POINTS : (bn != NULL ? GRT_OUT_LEVEL_BINS :
                 (ps->profile ? GRT_OUT_LEVELS : GRT_OUT_ROWS));
        in.clouds = sc != NULL ? NULL : ps->clouds;
        in.aerosols = ps->aer;
        in.subcolumns = sc;
        in.bins = bn;
        if (tr != NULL && tr->partials != NULL)
        {
            in.direct = bi == 1 ? &tr->direct : NULL;
            in.jacobian = bi == 0 ? &tr->jacobian : NULL;
        }
        in.responses = tr != NULL && tr->with_responses ? &tr->responses : NULL;
    }
    return in;
}

/* where band bi's solve of the pass leaves its third row group (NULL: it has none): the shortwave's direct beam or the
   longwave's Jacobian, where it is asked for; its rows per set and column, and where the pass's start in a column's
   direct_stride doubles of it */
static double *third_out(GrtPass const *ps, int bi)
{
    return bi == 1 ? ps->direct : ps->jacobian;
}

static int pass_direct(GrtPass const *ps, int bi)
{
    return third_out(ps, bi) != NULL;
}

static int direct_rows(GrtPipeline_t const *p, GrtPass const *ps)
{
    return ps->profile ? p->num_levels : GRT_DIRECT_ROWS_PER_SET;
}

static int direct_stride(GrtPipeline_t const *p, GrtPass const *ps)
{
    return ps->sets*direct_rows(p, ps);
}

static int direct_offset(GrtPipeline_t const *p, GrtPass const *ps)
{
    return ps->set*direct_rows(p, ps);
}

/* fused form: the partial sums of the third row group of `slots` slots per column, as *tr, where the pass leaves one (else
   *tr stays empty and the instance has no such join) */
static int direct_partials(GrtPipeline_t *p, GrtBand *b, int bi, GrtPass const *ps, int slots, ThirdRows *tr)
{
    memset(tr, 0, sizeof(*tr));
    if (pass_direct(ps, bi))
    {
        GrtScratch *block = &b->scratch[GRT_SCRATCH_DIRECT_PARTIALS];
        GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*(size_t)slots*(size_t)direct_rows(p, ps)*b->nblocks, NULL));
        tr->partials = tr->direct.partials = tr->jacobian.partials = block->d;
    }
    return GRTCODE_SUCCESS;
}

/* grt_pipeline_run_sky_weighted: the pass's response table with the band's partial sums of `slots` slots per column
   (GRT_SCRATCH_RESPONSE_PARTIALS, [max_cols][slots][P][G V], sized for the call's largest set at once), as *ra */
static int response_partials(GrtPipeline_t *p, GrtBand *b, GrtPass const *ps, int slots, GrtResponseArgs *ra)
{
    GrtResponseRun const *rr = ps->responses;
    GrtScratch *block = &b->scratch[GRT_SCRATCH_RESPONSE_PARTIALS];
    size_t const most = (size_t)(rr->slots > slots ? rr->slots : slots);
    GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*most*(size_t)rr->args.per_row*(size_t)rr->groups*
                                       (size_t)p->num_levels, NULL));
    *ra = rr->args;
    ra->partials = block->d;
    return GRTCODE_SUCCESS;
}

/* ... fused form: as the join of the pass's instance in *tr, behind direct_partials (a pass without responses: nothing) */
static int response_join(GrtPipeline_t *p, GrtBand *b, GrtPass const *ps, int slots, ThirdRows *tr)
{
    if (ps->responses != NULL)
    {
        GRT_TRY(response_partials(p, b, ps, slots, &tr->responses));
        tr->with_responses = 1;
    }
    return GRTCODE_SUCCESS;
}

/* ... and what turns the partial sums of its S draws into the pass's set of the band's response rows: the finishing kernel
   (GRT_TAG_BAND_PROFILES), each response's blocks in the fixed-order sum's association, the draws in order, one division */
static int finish_responses(GrtPipeline_t *p, int C, int S, GrtPass const *ps, GrtResponseArgs const *ra)
{
    GrtResponseRun const *rr = ps->responses;
    void *s = grt_dev_stream(p->device);
    GRT_TIMED(s, GRT_TAG_BAND_PROFILES, "response finishing kernel",
              grt_launch_response_finish(s, ra, rr->groups, C, S, p->num_levels, rr->out, (uint64_t)ps->sets*rr->set_doubles,
                                         (uint64_t)ps->set*rr->set_doubles));
    return GRTCODE_SUCCESS;
}

/* Materialised form of the response rows: from the [C][V][n] fluxes the pass (the mean over its subcolumns) has left in the
   band's arrays -- and, shortwave, its direct beam in GRT_SCRATCH_DIRECT_BEAM --, the same weights and sums into the same
   partial sums, one slot per column, then the same finishing kernel (both under GRT_TAG_BAND_PROFILES) */
static int response_rows(GrtPipeline_t *p, GrtBand *b, int C, GrtPass const *ps)
{
    if (ps->responses == NULL)
    {
        return GRTCODE_SUCCESS;
    }
    GrtResponseRun const *rr = ps->responses;
    void *s = grt_dev_stream(p->device);
    GrtResponseArgs ra;
    GRT_TRY(response_partials(p, b, ps, 1, &ra));
    double const *const rows[3] = {b->flux_up, b->flux_down, rr->groups == 3 ? b->scratch[GRT_SCRATCH_DIRECT_BEAM].d : NULL};
    GRT_TIMED(s, GRT_TAG_BAND_PROFILES, "response row kernel",
              grt_launch_response_rows(s, &ra, rows, rr->groups, C, p->num_levels, b->n, b->gas->grid.dw));
    GRT_TRY(finish_responses(p, C, 1, ps, &ra));
    return GRTCODE_SUCCESS;
}

/* its rows per band and column, and where band bi's start in a column's out_stride doubles */
static int pass_rows(GrtPipeline_t const *p, GrtPass const *ps)
{
    return ps->profile ? 2*p->num_levels : GRT_FLUXES_PER_BAND;
}

static int pass_offset(GrtPipeline_t const *p, GrtPass const *ps, int bi)
{
    return ps->set*grt_set_offset(p, ps->profile) + bi*pass_rows(p, ps);
}

static size_t band_points(GrtPipeline_t const *p, int bi)
{
    return p->band[bi].gas != NULL ? p->band[bi].n : 0;
}

/* where band bi's rows of the pass's set and column 0 start in a [ncol][sets][rows (per_lw + per_sw)] block -- rows: 6 or
   2 V; per: the bands' grid points, or their bins --, and the doubles from one column to the next */
static size_t bins_offset(GrtPass const *ps, int bi, size_t rows, size_t per_lw, size_t per_sw, size_t *col_stride)
{
    size_t const set_doubles = rows*(per_lw + per_sw);
    *col_stride = (size_t)ps->sets*set_doubles;
    return (size_t)ps->set*set_doubles + (bi == 1 ? rows*per_lw : 0);
}

/* ... of the six rows at every point (pass_spectral) */
static double *spectral_rows(GrtPipeline_t const *p, GrtPass const *ps, int bi, size_t *col_stride)
{
    return ps->bins->spectral + bins_offset(ps, bi, GRT_FLUXES_PER_BAND, band_points(p, 0), band_points(p, 1), col_stride);
}

/* The solvers' arguments.  Fused forms: Rayleigh, add_optics({gas, rayleigh}) and the solver in one launch (driver.c:268,
   382-424) on tau_gas; spectral form: the materialised tau, omega (, g) in, [level][wavenumber] fluxes out.  The caller
   sets the partial sums and, shortwave, the park block. */
static void lw_args(GrtPipeline_t const *p, GrtBand const *b, int C, int fused, GrtPass const *ps, GrtLwArgs *a)
{
    SpectralGrid_t const *grid = &b->gas->grid;
    int const V = p->num_levels, L = V - 1;
    memset(a, 0, sizeof(*a));
    a->num_levels = V; a->ncol = C; a->w0 = grid->w0; a->dw = grid->dw; a->nw = b->n;
    a->optics_stride = (uint64_t)L*b->n;
    a->t_layers = p->small.d + p->off_tl; a->t_levels = p->small.d + p->off_tv;
    a->t_surf = p->small.d + p->off_ts;
    a->emis = p->emis_d; a->emis_stride = 0;
    if (b->surf_set)
    {
        a->emis = b->scratch[GRT_SCRATCH_SURF_ROWS].d; a->emis_stride = b->n;          /* grt_pipeline_set_surface: driver.c:101-107 */
    }
    a->user_level = p->user_level;
    if (fused)
    {
        a->tau_gas = b->tau_gas; a->n_layer = p->small.d + p->off_n;
        a->add_continua = ps->defer;
        if (ps->defer) a->continua = *ps->continua;
    }
    else
    {
        a->tau = b->tau; a->omega = b->omega;
        a->flux_up = b->flux_up; a->flux_down = b->flux_down; a->flux_stride = (uint64_t)V*b->n;
    }
}

static void sw_args(GrtPipeline_t const *p, GrtBand const *b, int C, int fused, GrtPass const *ps, GrtSwArgs *a)
{
    SpectralGrid_t const *grid = &b->gas->grid;
    int const V = p->num_levels, L = V - 1;
    memset(a, 0, sizeof(*a));
    a->num_levels = V; a->ncol = C; a->nw = b->n; a->dw = grid->dw; a->w0 = grid->w0;
    a->optics_stride = (uint64_t)L*b->n;
    a->mu_dir = p->small.d + p->off_mu; a->mu_dif = 0.5;        /* driver.c:110 */
    a->alb_dir = p->albedo_d; a->alb_dif = p->albedo_d; a->alb_stride = 0;   /* driver.c:118-119 */
    if (b->surf_set)
    {
        /* grt_pipeline_set_surface: driver.c:111-117 */
        a->alb_dir = b->scratch[GRT_SCRATCH_SURF_ROWS].d;
        a->alb_dif = b->scratch[b->surf_dif_set ? GRT_SCRATCH_SURF_ROWS_DIF : GRT_SCRATCH_SURF_ROWS].d;
        a->alb_stride = b->n;
    }
    a->tsi = p->small.d + p->off_tsi; a->solar = p->solar_d;
    a->user_level = p->user_level;
    if (fused)
    {
        a->tau_gas = b->tau_gas; a->n_layer = p->small.d + p->off_n;
        a->add_continua = ps->defer;
        if (ps->defer) a->continua = *ps->continua;
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

/* The arguments of the band's solver in the instance in, in whichever of the two structs is the band's: the partial sums,
   where the six rows at every point go, and the shortwave's park block (the two-sweep form: reflectances of 2 V levels
   and five properties of L layers per column and wavenumber), which the level forms share with the two-sweep six-row
   forms (the passes run in stream order) */
typedef struct SolverArgs { GrtLwArgs lw; GrtSwArgs sw; } SolverArgs;

static int solver_args(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps, GrtSolverInstance const *in,
                       double *partials, SolverArgs *a)
{
    size_t stride = 0;
    double *rows = in->out == GRT_OUT_ROWS_POINTS ? spectral_rows(p, ps, bi, &stride) : NULL;
    if (bi == 0)
    {
        lw_args(p, b, C, grt_out_fused(in->out), ps, &a->lw);
        a->lw.partials = partials;
        if (rows != NULL)
        {
            a->lw.flux_up = rows;
            a->lw.flux_down = rows + 3*b->n;
            a->lw.flux_stride = stride;
        }
        return GRTCODE_SUCCESS;
    }
    sw_args(p, b, C, grt_out_fused(in->out), ps, &a->sw);
    a->sw.partials = partials;
    if (rows != NULL)
    {
        a->sw.flux_up = rows;
        a->sw.flux_down = rows + 3*b->n;
        a->sw.flux_stride = stride;
    }
    if (grt_sw_parks(in, &a->sw))
    {
        size_t const V = (size_t)p->num_levels;
        GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_PARK], (size_t)p->max_cols*(2*V + 5*(V - 1))*b->n, NULL));
    }
    a->sw.park = b->scratch[GRT_SCRATCH_PARK].d;
    return GRTCODE_SUCCESS;
}

static int solver_launch(void *s, int bi, GrtSolverInstance const *in, SolverArgs const *a)
{
    return bi == 0 ? grt_launch_lw(s, in, &a->lw) : grt_launch_sw(s, in, &a->sw);
}

/* the band's solver in the pass's instance (bn: its per-bin one; tr: the one that leaves the third row group too), timed
   under the pass's profile tag */
static int band_solver(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps, double *partials,
                       GrtBandArgs const *bn, ThirdRows const *tr)
{
    GrtSolverInstance const in = pass_instance(p, ps, bn, NULL, tr, bi);
    void *s = grt_dev_stream(p->device);
    SolverArgs a;
    GRT_TRY(solver_args(p, b, bi, C, ps, &in, partials, &a));
    GRT_TIMED(s, pass_tag(ps, bi), bi == 0 ? "longwave kernel" : "shortwave kernel", solver_launch(s, bi, &in, &a));
    return GRTCODE_SUCCESS;
}

/* A walk over `total` items -- a pass's draws, its sun angles, its tile chunks -- in launches of at most `step`, on the
   first/count pair the launcher reads: for (first = count = 0; krc == 0 && walk(total, step, &first, &count); ) krc = the
   launch.  The first launch error stops it, and what is not queued then stays not queued.  One span covers a whole walk,
   so those spans are opened and closed by hand.
   The step is what one launch may hold.  row_limit: the grid rows of C columns each, 65 535 along the grid's y or --
   parks: the launch parks every row, as the shortwave's two-sweep forms and the longwave's scattering kernel do -- the
   max_cols of the band's park block.  A walk with another nested in it (angles, tile chunks) takes row_limit/(the inner
   walk's items per launch) of it.
   walk needs first = count = 0 before its first call, as the for above sets them, and step >= 1: a step of 0 never ends.
   row_limit is 1 or more because a run has C <= max_cols columns and a pipeline max_cols <= 65 535
   (grt_pipeline_create_ex), and every nested divisor is itself cut to the limit it divides. */
static int walk(int total, int step, int *first, int *count)
{
    *first += *count;
    *count = total - *first < step ? total - *first : step;
    return *first < total;
}

static int row_limit(GrtPipeline_t const *p, int C, int parks)
{
    return (parks ? p->max_cols : 65535)/C;
}

/* the pass's clouds as the S subcolumns of *sc, for the instances and launchers that take them so (they point at *sc and
   read the first and count a walk leaves there); NULL for a pass without clouds, whose one draw is walked on *sc all the
   same */
static GrtSubcolumnArgs *pass_subcolumns(GrtPass const *ps, int S, GrtSubcolumnArgs *sc)
{
    memset(sc, 0, sizeof(*sc));
    if (ps->clouds == NULL)
    {
        return NULL;
    }
    sc->clouds = *ps->clouds;
    sc->subcolumns = S;
    return sc;
}

/* Draw j of a pass whose clouds hold their draws subcolumn-major, for the materialised loops: the pass on draw j's tables,
   which *cj holds (a pass without clouds: the pass itself) */
static GrtPass pass_draw(GrtPipeline_t const *p, GrtPass const *ps, int C, int j, GrtCloudArgs *cj)
{
    GrtPass pj = *ps;
    if (ps->clouds != NULL)
    {
        size_t const tab = (size_t)C*3*(size_t)ps->clouds->num_bands*(size_t)(p->num_levels - 1);
        *cj = *ps->clouds;
        cj->liquid += (size_t)j*tab;
        cj->ice += (size_t)j*tab;
        pj.clouds = cj;
    }
    return pj;
}

/* What turns a block's [C][S][rows] rows of nblocks partial sums each into column c's rows at out[c stride + offset ..]:
   the fixed-order sum of the blocks or -- S > 1 -- the subcolumn mean kernel, draws 0 .. S - 1 in order, then one division
   by S.  The launch alone: whether it is timed, and as what it is checked, is its caller's. */
static int partial_rows(void *s, double const *partials, int C, int S, int rows, unsigned nblocks, double *out, int stride,
                        int offset)
{
    return S == 1 ? grt_launch_reduce_partials(s, partials, C*rows, nblocks, out, rows, stride, offset) :
                    grt_launch_subcolumn_mean(s, partials, C, S, rows, nblocks, out, stride, offset);
}

/* whether band bi's solve of the pass leaves radiances too (grt_pipeline_run_sky_radiances: the longwave's) */
static int pass_radiances(GrtPass const *ps, int bi)
{
    return bi == 0 && ps->radiances != NULL;
}

/* The pass's radiance launch (GRT_TAG_RADIANCE), queued behind its longwave solver -- or, a pass without flux rows, in its
   place -- on that solver's instance and arguments (pass_instance, solver_args: the continua it may have to add
   included).  Its partial sums go to GRT_SCRATCH_RADIANCE_PARTIALS, [max_cols][S][A][2][nblocks]; the spectral outputs,
   where given, to the pass's set of [ncol][sets][A][2][n].  Fused form: sc, the pass's clouds as its subcolumns (NULL:
   S = 1), walked in groups of grid rows as the solver's launches are; materialised form: the tau, omega left on the
   grid, draw `draw` of S. */
static int band_radiances(GrtPipeline_t *p, GrtBand *b, int C, int S, int draw, GrtPass const *ps, GrtSubcolumnArgs *sc)
{
    GrtRadianceRun const *rr = ps->radiances;
    void *s = grt_dev_stream(p->device);
    size_t const per_slot = (size_t)rr->angles*GRT_RADIANCE_ROWS_PER_ANGLE;
    GrtScratch *block = &b->scratch[GRT_SCRATCH_RADIANCE_PARTIALS];
    /* (the kernel's own blocks along the spectrum: the materialised form keeps no b->nblocks) */
    GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*(size_t)S*per_slot*grt_solver_blocks(b->n), NULL));
    GrtSolverInstance const in = pass_instance(p, ps, NULL, sc, NULL, 0);
    SolverArgs a;
    GRT_TRY(solver_args(p, b, 0, C, ps, &in, NULL, &a));
    size_t const set_doubles = per_slot*b->n;
    GrtRadianceArgs r;
    memset(&r, 0, sizeof(r));
    r.secant = rr->secant; r.angles = rr->angles; r.subcolumns = S; r.draw = draw; r.partials = block->d;
    r.spectral = rr->spectral != NULL ? rr->spectral + (size_t)ps->set*set_doubles : NULL;
    r.brightness = rr->brightness != NULL ? rr->brightness + (size_t)ps->set*set_doubles : NULL;
    r.col_stride = (uint64_t)ps->sets*set_doubles;
    /* (grt_pipeline_run_sky_channels: the kernel's channel form, its pairs' sums to GRT_SCRATCH_CHANNEL_PARTIALS,
       [max_cols][S][A][2][P]) */
    GrtChannelArgs ch;
    if (ps->channels != NULL)
    {
        ch = ps->channels->args;
        GrtScratch *pairs = &b->scratch[GRT_SCRATCH_CHANNEL_PARTIALS];
        int const slots = ps->channels->slots > S ? ps->channels->slots : S;   /* (the call's cloud sets': sized once) */
        GRT_TRY(grt_scratch_need(p, pairs, (size_t)p->max_cols*(size_t)slots*per_slot*(size_t)ch.pairs, NULL));
        ch.partials = pairs->d;
    }
    /* (grt_pipeline_run_sky_weighting: the weighting kernel's pairs' sums to GRT_SCRATCH_WEIGHTING_PARTIALS,
       [max_cols][S][A][R][P]; the largest block of the call, asked for before either kernel of the pass is queued) */
    GrtWeightingArgs wa;
    memset(&wa, 0, sizeof(wa));
    if (ps->weighting != NULL)
    {
        wa = ps->weighting->args;
        GrtScratch *wpairs = &b->scratch[GRT_SCRATCH_WEIGHTING_PARTIALS];
        int const wslots = ps->channels->slots > S ? ps->channels->slots : S;
        GRT_TRY(grt_scratch_need(p, wpairs, (size_t)p->max_cols*(size_t)wslots*(size_t)rr->angles*
                                                (size_t)grt_weighting_rows(&wa, p->num_levels)*(size_t)ch.pairs, NULL));
        wa.partials = wpairs->d;
    }
    /* (a launch without subcolumns is a walk of one step, on a pair that no launcher reads) */
    GrtSubcolumnArgs one, *w = sc != NULL ? sc : &one;
    int const draws = sc != NULL ? S : 1, group = row_limit(p, C, 0);
    int const slot = grt_profile_begin(s, GRT_TAG_RADIANCE);
    int krc = 0;
    for (w->first = w->count = 0; krc == 0 && walk(draws, group, &w->first, &w->count); )
    {
        krc = ps->channels != NULL ? grt_launch_lw_channels(s, &in, &a.lw, &r, &ch) : grt_launch_lw_radiances(s, &in, &a.lw, &r);
    }
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "longwave radiance kernel"));
    if (ps->weighting == NULL)
    {
        return GRTCODE_SUCCESS;
    }
    /* (the weighting kernel behind it on the same instance and arguments, GRT_TAG_WEIGHTING) */
    int const wslot = grt_profile_begin(s, GRT_TAG_WEIGHTING);
    for (w->first = w->count = 0; krc == 0 && walk(draws, group, &w->first, &w->count); )
    {
        krc = grt_launch_lw_weighting(s, &in, &a.lw, &r, &ch, &wa);
    }
    grt_profile_end(s, wslot);
    GRT_TRY(grt_dev_check(krc, "longwave weighting kernel"));
    return GRTCODE_SUCCESS;
}

/* ... and what turns the partial sums of its S draws into the pass's set of the integrated radiances [ncol][sets][A][2]
   (partial_rows; the mean of several draws counts under GRT_TAG_SUBCOLUMN_MEAN, the sum of one is not timed) */
static int finish_radiances(GrtPipeline_t *p, GrtBand *b, int C, int S, GrtPass const *ps)
{
    GrtRadianceRun const *rr = ps->radiances;
    void *s = grt_dev_stream(p->device);
    int const rows = rr->angles*GRT_RADIANCE_ROWS_PER_ANGLE;
    GRT_TIMED(s, S == 1 ? GRT_UNTIMED : GRT_TAG_SUBCOLUMN_MEAN, S == 1 ? "radiance reduction kernel" : "subcolumn mean kernel",
              partial_rows(s, b->scratch[GRT_SCRATCH_RADIANCE_PARTIALS].d, C, S, rows, grt_solver_blocks(b->n), rr->integrated,
                           ps->sets*rows, ps->set*rows));
    return GRTCODE_SUCCESS;
}

/* ... and -- grt_pipeline_run_sky_channels -- the pairs' sums of the S draws into the pass's set of the channel radiances
   and brightness temperatures [ncol][sets][A][2][C] (GRT_TAG_CHANNELS); a pass without channels: nothing */
static int finish_channels(GrtPipeline_t *p, GrtBand *b, int C, int S, GrtPass const *ps)
{
    if (ps->channels == NULL)
    {
        return GRTCODE_SUCCESS;
    }
    GrtChannelRun const *cr = ps->channels;
    void *s = grt_dev_stream(p->device);
    GrtChannelArgs ch = cr->args;
    ch.partials = b->scratch[GRT_SCRATCH_CHANNEL_PARTIALS].d;
    uint64_t const set_doubles = (uint64_t)ps->radiances->angles*GRT_RADIANCE_ROWS_PER_ANGLE*(uint64_t)ch.channels;
    GRT_TIMED(s, GRT_TAG_CHANNELS, "channel finishing kernel",
              grt_launch_channel_finish(s, &ch, C, S, ps->radiances->angles, cr->radiances, cr->brightness,
                                        (uint64_t)ps->sets*set_doubles, (uint64_t)ps->set*set_doubles));
    return GRTCODE_SUCCESS;
}

/* ... and -- grt_pipeline_run_sky_weighting -- the rows' sums of the S draws into the pass's set of the transmittances
   [ncol][sets][A][V][C] and contributions [ncol][sets][A][V + 1][C] (GRT_TAG_WEIGHTING_FINISH); a pass without: nothing */
static int finish_weighting(GrtPipeline_t *p, GrtBand *b, int C, int S, GrtPass const *ps)
{
    if (ps->weighting == NULL)
    {
        return GRTCODE_SUCCESS;
    }
    GrtWeightingRun const *wr = ps->weighting;
    void *s = grt_dev_stream(p->device);
    GrtChannelArgs ch = ps->channels->args;
    ch.partials = b->scratch[GRT_SCRATCH_CHANNEL_PARTIALS].d;
    GrtWeightingArgs wa = wr->args;
    wa.partials = b->scratch[GRT_SCRATCH_WEIGHTING_PARTIALS].d;
    int const A = ps->radiances->angles, V = p->num_levels;
    uint64_t const t_set = (uint64_t)A*(uint64_t)V*(uint64_t)ch.channels;
    uint64_t const k_set = (uint64_t)A*(uint64_t)(V + 1)*(uint64_t)ch.channels;
    GRT_TIMED(s, GRT_TAG_WEIGHTING_FINISH, "weighting finishing kernel",
              grt_launch_weighting_finish(s, &ch, &wa, C, S, A, V, wr->transmittance, (uint64_t)ps->sets*t_set,
                                          (uint64_t)ps->set*t_set, wr->contribution, (uint64_t)ps->sets*k_set,
                                          (uint64_t)ps->set*k_set));
    return GRTCODE_SUCCESS;
}

/* The radiances of a pass in two halves: band_radiances queues the launches, radiance_outputs the three finishing steps
   behind them (a materialised pass of several draws: a launch per draw, then the finish).  pass_radiance_tail is both in
   a row, for the pass whose draws one launch walk covers (a pass without radiances: nothing). */
static int radiance_outputs(GrtPipeline_t *p, GrtBand *b, int C, int S, GrtPass const *ps)
{
    GRT_TRY(finish_radiances(p, b, C, S, ps));
    GRT_TRY(finish_channels(p, b, C, S, ps));
    GRT_TRY(finish_weighting(p, b, C, S, ps));
    return GRTCODE_SUCCESS;
}

static int pass_radiance_tail(GrtPipeline_t *p, GrtBand *b, int bi, int C, int S, GrtPass const *ps, GrtSubcolumnArgs *sc)
{
    if (pass_radiances(ps, bi))
    {
        GRT_TRY(band_radiances(p, b, C, S, 0, ps, sc));
        GRT_TRY(radiance_outputs(p, b, C, S, ps));
    }
    return GRTCODE_SUCCESS;
}

/* Rayleigh + add_optics({gas, rayleigh}) (driver.c:268, 382-383) into the band's tau, omega, g */
static int clear_sky_optics(GrtPipeline_t *p, GrtBand *b, int C)
{
    SpectralGrid_t const *grid = &b->gas->grid;
    void *s = grt_dev_stream(p->device);
    GRT_TIMED(s, GRT_TAG_CLEAR_OPTICS, "clear-sky optics kernel",
              grt_launch_clear_sky_optics(s, p->num_levels - 1, C, grid->w0, grid->dw, b->n, p->small.d + p->off_n, b->tau_gas,
                                          b->tau, b->omega, b->g));
    return GRTCODE_SUCCESS;
}

/* The aerosol object (driver.c:426-434), the cloud objects (driver.c:507-530: liquid, ice) or all three spread onto the
   grid, then per column Rayleigh and add_optics({gas, rayleigh, the spread objects: the aerosol first, as in the fused
   solvers' sky_combine}) -- tau, omega, g of the band are the pass's */
static int spread_optics(GrtPipeline_t *p, GrtBand *b, int C, GrtPass const *ps)
{
    SpectralGrid_t const *grid = &b->gas->grid;
    int const L = p->num_levels - 1, first_cloud = ps->aer != NULL ? 1 : 0;
    int const objects = first_cloud + (ps->clouds != NULL ? 2 : 0);
    uint64_t const per = (uint64_t)L*b->n, all = per*(uint64_t)p->max_cols;
    void *s = grt_dev_stream(p->device);
    GrtScratch *block = &b->scratch[GRT_SCRATCH_SPREAD];
    int fresh;
    GRT_TRY(grt_scratch_need(p, block, 4*per + 3*objects*all, &fresh));
    if (fresh)
    {
        GRT_TRY(grt_dev_zero(p->device, block->d + 3*per, sizeof(double)*per, s));
    }
    double *ray = block->d, *zero = ray + 3*per, *x[9];
    for (int k = 0; k < 3*objects; ++k)
    {
        x[k] = zero + per + k*all;
    }
    if (ps->aer != NULL)
    {
        GRT_TRY(grt_dev_check(grt_launch_spread_aerosols(s, L, C, grid->w0, grid->dw, b->n, ps->aer, x[0], x[1], x[2]),
                              "aerosol spreading kernel"));
    }
    if (ps->clouds != NULL)
    {
        double **y = x + 3*first_cloud;
        GRT_TRY(grt_dev_check(grt_launch_spread_clouds(s, L, C, b->n, ps->clouds, y[0], y[1], y[2], y[3], y[4], y[5]),
                              "cloud spreading kernel"));
    }
    for (int c = 0; c < C; ++c)
    {
        /* Rayleigh of this column (rayleigh.c:29-68: its number densities travel as a kernel argument) */
        GRT_TRY(grt_dev_check(grt_launch_rayleigh(s, L, grid->w0, grid->dw, b->n, p->small.h + p->off_n + (size_t)c*L,
                                                  ray, ray + per, ray + 2*per), "Rayleigh kernel"));
        GrtOpticsPtrs in;
        memset(&in, 0, sizeof(in));
        uint64_t const o = (uint64_t)c*per;
        in.tau[0] = b->tau_gas + o; in.omega[0] = zero; in.g[0] = zero;
        in.tau[1] = ray; in.omega[1] = ray + per; in.g[1] = ray + 2*per;
        for (int k = 0; k < objects; ++k)
        {
            in.tau[2 + k] = x[3*k] + o; in.omega[2 + k] = x[3*k + 1] + o; in.g[2 + k] = x[3*k + 2] + o;
        }
        GRT_TRY(grt_dev_check(grt_launch_add_optics(s, per, 2 + objects, &in, b->tau + o, b->omega + o, b->g + o),
                              objects == 3 ? "add_optics kernel (aerosols and clouds)" :
                              (ps->aer != NULL ? "add_optics kernel (aerosols)" : "add_optics kernel (all-sky)")));
    }
    return GRTCODE_SUCCESS;
}

/* the materialised optics a pass runs before its spectral solver */
static int pass_optics(GrtPipeline_t *p, GrtBand *b, int C, GrtPass const *ps)
{
    GRT_TRY(ps->aer != NULL || ps->clouds != NULL ? spread_optics(p, b, C, ps) : clear_sky_optics(p, b, C));
    return GRTCODE_SUCCESS;
}

/* the row table of every level's up and down flux, [max_cols][2 V] */
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
    GRT_TRY(grt_upload_rows(p, rows_h, C*2*V, &b->level_rows_d));
    return GRTCODE_SUCCESS;
}

/* the row-wise trapezoid of the band's spectral fluxes, the pass's six rows or 2 V of every column: column c's to
   out[c out_stride + out_offset ..], under the profile tag `tag` (GRT_UNTIMED: not timed) */
static int integrate_rows_to(GrtPipeline_t *p, GrtBand *b, int C, GrtPass const *ps, int tag, double *out, int out_stride,
                             int out_offset)
{
    void *s = grt_dev_stream(p->device);
    int const rows = pass_rows(p, ps);
    if (ps->profile)
    {
        GRT_TRY(level_rows(p, b));
    }
    GRT_TIMED(s, tag, "spectral integration kernel",
              grt_launch_integrate_rows(s, (double const *const *)(ps->profile ? b->level_rows_d : b->rows_d), C*rows, b->n,
                                        b->gas->grid.dw, out, rows, out_stride, out_offset));
    return GRTCODE_SUCCESS;
}

/* ... into the pass's own rows */
static int integrate_rows(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps)
{
    GRT_TRY(integrate_rows_to(p, b, C, ps, GRT_UNTIMED, ps->out, ps->out_stride, pass_offset(p, ps, bi)));
    return GRTCODE_SUCCESS;
}

/* Materialised form of the third row group: from the tau, omega, g the pass (its last subcolumn) has left in the band's
   arrays, every level's direct beam (shortwave, GRT_TAG_DIRECT_BEAM) or surface-temperature Jacobian (longwave,
   GRT_TAG_SURFACE_JACOBIAN) on the grid, [C][V][n] in GRT_SCRATCH_DIRECT_BEAM */
static int direct_beam(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps)
{
    void *s = grt_dev_stream(p->device);
    GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_DIRECT_BEAM], (size_t)p->max_cols*(size_t)p->num_levels*b->n, NULL));
    if (bi == 0)
    {
        GrtLwArgs a;
        lw_args(p, b, C, 0, ps, &a);
        GRT_TIMED(s, GRT_TAG_SURFACE_JACOBIAN, "surface Jacobian kernel",
                  grt_launch_lw_surface_jacobian(s, &a, b->scratch[GRT_SCRATCH_DIRECT_BEAM].d));
        return GRTCODE_SUCCESS;
    }
    GrtSwArgs a;
    sw_args(p, b, C, 0, ps, &a);
    GRT_TIMED(s, GRT_TAG_DIRECT_BEAM, "direct-beam kernel",
              grt_launch_sw_direct_beam(s, &a, b->scratch[GRT_SCRATCH_DIRECT_BEAM].d));
    return GRTCODE_SUCCESS;
}

/* ... and the row-wise trapezoid of it into three rows -- TOA, surface and the user level (the zero row without one) -- or,
   profile, every level: column c's at out[c out_stride + out_offset ..] */
static int direct_integrate_to(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps, double *out, int out_stride,
                               int out_offset)
{
    size_t const V = (size_t)p->num_levels, cols = (size_t)p->max_cols, rows = (size_t)direct_rows(p, ps);
    double *beam = b->scratch[GRT_SCRATCH_DIRECT_BEAM].d;
    double ***table = &b->direct_rows_d[ps->profile != 0];
    if (*table == NULL)
    {
        double **rows_h = malloc(sizeof(double *)*cols*rows);
        if (rows_h == NULL)
        {
            GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for the %s row table of %zu columns.",
                     bi == 1 ? "direct-beam" : "surface Jacobian", cols);
        }
        for (size_t c = 0; c < cols; ++c)
        {
            double *lev = beam + c*V*b->n;
            for (size_t k = 0; k < rows && ps->profile; ++k)
            {
                rows_h[c*rows + k] = lev + k*b->n;
            }
            if (!ps->profile)
            {
                rows_h[c*rows + 0] = lev;
                rows_h[c*rows + 1] = lev + (V - 1)*b->n;
                rows_h[c*rows + 2] = p->user_level >= 0 ? lev + (size_t)p->user_level*b->n : b->zero_row;
            }
        }
        GRT_TRY(grt_upload_rows(p, rows_h, cols*rows, table));
    }
    GRT_TRY(grt_dev_check(grt_launch_integrate_rows(grt_dev_stream(p->device), (double const *const *)*table, C*(int)rows,
                                                    b->n, b->gas->grid.dw, out, (int)rows, out_stride, out_offset),
                          "spectral integration kernel"));
    return GRTCODE_SUCCESS;
}

/* ... into the pass's own third rows */
static int direct_integrate(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps)
{
    GRT_TRY(direct_integrate_to(p, b, bi, C, ps, third_out(ps, bi), direct_stride(p, ps), direct_offset(p, ps)));
    return GRTCODE_SUCCESS;
}

/* ---- grt_pipeline_run_sky_scattering: the longwave's scattering correction behind a pass's solver ---- */
static int pass_scatter(GrtPass const *ps, int bi)
{
    return bi == 0 && ps->scatter != NULL;
}

/* the park block of the longwave band, max_cols grid rows: allocated at the first call that scatters, as *sa */
static int scatter_park(GrtPipeline_t *p, GrtBand *b, GrtScatterArgs *sa)
{
    GrtScratch *park = &b->scratch[GRT_SCRATCH_SCATTER_PARK];
    GRT_TRY(grt_scratch_need(p, park, (size_t)grt_scatter_park_doubles((uint64_t)p->max_cols, p->num_levels, b->n), NULL));
    memset(sa, 0, sizeof(*sa));
    sa->park = park->d;
    sa->park_rows = (uint64_t)p->max_cols;
    return GRTCODE_SUCCESS;
}

/* what turns the block's [C][S][rows] rows of nblocks partial sums each into the pass's set of the differences
   (partial_rows; one draw or several, under GRT_TAG_SCATTER_FINISH) */
static int scatter_finish(GrtPipeline_t *p, GrtBand *b, int C, int S, unsigned nblocks, GrtPass const *ps)
{
    void *s = grt_dev_stream(p->device);
    int const rows = pass_rows(p, ps);
    GRT_TIMED(s, GRT_TAG_SCATTER_FINISH, "scattering reduction kernel",
              partial_rows(s, b->scratch[GRT_SCRATCH_SCATTER_PARTIALS].d, C, S, rows, nblocks, ps->scatter->out, ps->sets*rows,
                           ps->set*rows));
    return GRTCODE_SUCCESS;
}

/* Fused form: the scattering kernel in the pass's instance (sc: its clouds as the subcolumns of sc, S of them; NULL:
   S = 1), its partial sums to GRT_SCRATCH_SCATTER_PARTIALS at the solver's slots, as many draws a launch as its park block
   holds (row_limit), in stream order; then scatter_finish */
static int scatter_fused(GrtPipeline_t *p, GrtBand *b, int C, int S, GrtPass const *ps, GrtSubcolumnArgs *sc)
{
    void *s = grt_dev_stream(p->device);
    int const rows = pass_rows(p, ps);
    GrtScratch *block = &b->scratch[GRT_SCRATCH_SCATTER_PARTIALS];
    GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*(size_t)S*(size_t)rows*b->nblocks, NULL));
    GrtScatterArgs sa;
    GRT_TRY(scatter_park(p, b, &sa));
    GrtSolverInstance in = pass_instance(p, ps, NULL, sc, NULL, 0);
    in.scatter = &sa;
    SolverArgs a;
    GRT_TRY(solver_args(p, b, 0, C, ps, &in, block->d, &a));
    GrtSubcolumnArgs one, *w = sc != NULL ? sc : &one;                /* (as band_radiances walks) */
    int const slot = grt_profile_begin(s, GRT_TAG_SCATTER_LW);
    int krc = 0;
    for (w->first = w->count = 0; krc == 0 && walk(sc != NULL ? S : 1, row_limit(p, C, 1), &w->first, &w->count); )
    {
        krc = grt_launch_lw_scatter(s, &in, &a.lw);
    }
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "longwave scattering kernel"));
    GRT_TRY(scatter_finish(p, b, C, S, b->nblocks, ps));
    return GRTCODE_SUCCESS;
}

/* Materialised form, draw j of S: the chain instance on the tau, omega, g the pass has left in the band's arrays.  The
   differences take the place of the fluxes in the band's flux arrays -- the pass's solver has run, and its fluxes are
   integrated or summed --, and their row-wise trapezoid goes to row (c S + j) of GRT_SCRATCH_SCATTER_PARTIALS, one
   value a row; scatter_finish after the last draw */
static int scatter_spectral(GrtPipeline_t *p, GrtBand *b, int C, int S, int j, GrtPass const *ps)
{
    void *s = grt_dev_stream(p->device);
    int const rows = pass_rows(p, ps);
    GrtScratch *block = &b->scratch[GRT_SCRATCH_SCATTER_PARTIALS];
    GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*(size_t)S*(size_t)rows, NULL));
    GrtScatterArgs sa;
    GRT_TRY(scatter_park(p, b, &sa));
    sa.g = b->g;
    GrtSolverInstance in = pass_instance(p, ps, NULL, NULL, NULL, 0);
    in.scatter = &sa;
    GrtLwArgs a;
    lw_args(p, b, C, 0, ps, &a);
    GRT_TIMED(s, GRT_TAG_SCATTER_LW, "longwave scattering kernel", grt_launch_lw_scatter(s, &in, &a));
    GRT_TRY(integrate_rows_to(p, b, C, ps, GRT_TAG_SCATTER_FINISH, block->d, S*rows, j*rows));
    if (j == S - 1)
    {
        GRT_TRY(scatter_finish(p, b, C, S, 1, ps));
    }
    return GRTCODE_SUCCESS;
}

/* One solve of a band for grt_pipeline_run_spectral: the six rows at every point into the caller's spectral block, the
   -integrated six into out, and the bins.  Fused form: the spectral six-row solver (its rows stored where it weights
   them) and the fixed-order sum of its partial sums; materialised form: the spectral solver, its rows 0, L and the user
   level copied out, the row-wise trapezoid.  The bins are summed from the stored rows by the binning kernel
   (GRT_TAG_BINS). */
static int band_solve_spectral(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps)
{
    void *s = grt_dev_stream(p->device);
    GrtBins const *so = ps->bins;
    size_t stride;
    double *rows = spectral_rows(p, ps, bi, &stride);
    if (!p->keep_spectra)
    {
        GRT_TRY(band_solver(p, b, bi, C, ps, b->partials, NULL, NULL));
        GRT_TRY(grt_dev_check(partial_rows(s, b->partials, C, 1, GRT_FLUXES_PER_BAND, b->nblocks, ps->out, ps->out_stride,
                                           pass_offset(p, ps, bi)), "flux reduction kernel"));
    }
    else
    {
        GRT_TRY(pass_optics(p, b, C, ps));
        GRT_TRY(band_solver(p, b, bi, C, ps, NULL, NULL, NULL));
        GRT_TRY(grt_dev_check(grt_launch_copy_rows(s, (double const *const *)b->rows_d, C*GRT_FLUXES_PER_BAND, b->n,
                                                   rows, stride), "spectral row copy kernel"));
        GRT_TRY(integrate_rows(p, b, bi, C, ps));
    }
    int const nbins = so->num_bins[bi];
    if (nbins > 0)
    {
        GRT_TRY(grt_band_bins(p, b, so->edges[bi], nbins, GRT_FLUXES_PER_BAND));
        size_t bstride;
        double *binned = so->binned + bins_offset(ps, bi, GRT_FLUXES_PER_BAND, (size_t)so->num_bins[0],
                                                  (size_t)so->num_bins[1], &bstride);
        GRT_TIMED(s, GRT_TAG_BINS, "spectral binning kernel",
                  grt_launch_bin_rows(s, rows, stride, C*GRT_FLUXES_PER_BAND, b->n, b->gas->grid.dw, nbins, b->bin_table.table,
                                      b->bin_per_row, b->scratch[GRT_SCRATCH_BIN_PARTIALS].d, binned, bstride));
    }
    return GRTCODE_SUCCESS;
}

/* One solve of a band for grt_pipeline_run_band_profiles: every level's up and down flux per bin of the band's edges,
   into the band's [2][bins][V] of the pass's set.  Fused form: the banded instance of the profile solver, whose partial
   sums lie where the bin table places them, and each bin's blocks added in a fixed order; materialised form: the
   spectral solver, then the binning kernel on its 2 V flux rows per column.  The reduction counts under
   GRT_TAG_BAND_PROFILES. */
static int band_solve_band_profiles(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps)
{
    GrtBins const *bp = ps->bins;
    void *s = grt_dev_stream(p->device);
    int const V = p->num_levels, rows = 2*V, nbins = bp->num_bins[bi];
    size_t out_stride;
    double *out = ps->out + bins_offset(ps, bi, (size_t)rows, (size_t)bp->num_bins[0], (size_t)bp->num_bins[1], &out_stride);
    GRT_TRY(grt_band_bins(p, b, bp->edges[bi], nbins, rows));
    double *bin_partials = b->scratch[GRT_SCRATCH_BIN_PARTIALS].d;
    if (!p->keep_spectra)
    {
        GrtBandArgs const bn = {nbins, grt_bin_block_max(bp->edges[bi], nbins), b->bin_table.table, b->bin_per_row};
        GRT_TRY(band_solver(p, b, bi, C, ps, bin_partials, &bn, NULL));
        GRT_TIMED(s, GRT_TAG_BAND_PROFILES, "level binning kernel",
                  grt_launch_bin_reduce(s, C*rows, V, nbins, b->bin_table.table, b->bin_per_row, bin_partials, out, out_stride));
        return GRTCODE_SUCCESS;
    }
    GRT_TRY(pass_optics(p, b, C, ps));
    GRT_TRY(band_solver(p, b, bi, C, ps, NULL, NULL, NULL));
    GRT_TRY(level_rows(p, b));
    GRT_TIMED(s, GRT_TAG_BAND_PROFILES, "level binning kernel",
              grt_launch_bin_level_rows(s, (double const *const *)b->level_rows_d, C*rows, V, b->n, b->gas->grid.dw, nbins,
                                        b->bin_table.table, b->bin_per_row, bin_partials, out, out_stride));
    return GRTCODE_SUCCESS;
}

/* The steps the fused forms of grt_band_solve and grt_band_solve_subcolumns share, each in its own order.  pass_rows_out:
   what turns the partial sums of the pass's S draws -- its rows' in `partials`, its third row group's in tr->partials
   where it leaves one -- into its rows and third rows (partial_rows).  One draw: two fixed-order sums, not timed; several:
   the two means under one span of GRT_TAG_SUBCOLUMN_MEAN. */
static int pass_rows_out(GrtPipeline_t *p, GrtBand *b, int bi, int C, int S, GrtPass const *ps, double const *partials,
                         ThirdRows const *tr)
{
    void *s = grt_dev_stream(p->device);
    int const rows = pass_rows(p, ps), drows = direct_rows(p, ps), offset = pass_offset(p, ps, bi);
    if (S == 1)
    {
        GRT_TRY(grt_dev_check(partial_rows(s, partials, C, 1, rows, b->nblocks, ps->out, ps->out_stride, offset),
                              "flux reduction kernel"));
        if (tr->partials != NULL)
        {
            GRT_TRY(grt_dev_check(partial_rows(s, tr->partials, C, 1, drows, b->nblocks, third_out(ps, bi), direct_stride(p, ps),
                                               direct_offset(p, ps)),
                                  bi == 1 ? "direct-beam reduction kernel" : "surface Jacobian reduction kernel"));
        }
        return GRTCODE_SUCCESS;
    }
    int const slot = grt_profile_begin(s, GRT_TAG_SUBCOLUMN_MEAN);
    int krc = partial_rows(s, partials, C, S, rows, b->nblocks, ps->out, ps->out_stride, offset);
    if (krc == 0 && tr->partials != NULL)
    {
        krc = partial_rows(s, tr->partials, C, S, drows, b->nblocks, third_out(ps, bi), direct_stride(p, ps),
                           direct_offset(p, ps));
    }
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "subcolumn mean kernel"));
    return GRTCODE_SUCCESS;
}

/* ... the longwave's scattering correction and radiances behind the pass's solver (sc: its clouds as the subcolumns of sc;
   NULL: S = 1) */
static int pass_scatter_radiances(GrtPipeline_t *p, GrtBand *b, int bi, int C, int S, GrtPass const *ps, GrtSubcolumnArgs *sc)
{
    if (pass_scatter(ps, bi))
    {
        GRT_TRY(scatter_fused(p, b, C, S, ps, sc));
    }
    GRT_TRY(pass_radiance_tail(p, b, bi, C, S, ps, sc));
    return GRTCODE_SUCCESS;
}

/* One solve of a band: Rayleigh, add_optics({gas, rayleigh} and what the pass joins to them), the solver and the
   -integrated output (driver.c:268, 382-424, 426-434, 507-530, 302-326) of the pass's rows, to
   out[c*out_stride + its offset + r].  Fused form: all of it in one solver launch, then the fixed-order sum of its
   per-block partial sums (profile: in level_partials, which the passes of one call take in turn); materialised form: tau,
   omega, g and the spectral fluxes in the band's arrays, then the row-wise trapezoid. */
int grt_band_solve(GrtPipeline_t *p, GrtBand *b, int bi, int C, GrtPass const *ps)
{
    if (ps->bins != NULL)
    {
        GRT_TRY(ps->profile ? band_solve_band_profiles(p, b, bi, C, ps) : band_solve_spectral(p, b, bi, C, ps));
        return GRTCODE_SUCCESS;
    }
    if (p->keep_spectra)
    {
        GRT_TRY(pass_optics(p, b, C, ps));
        if (ps->out != NULL)
        {
            GRT_TRY(band_solver(p, b, bi, C, ps, NULL, NULL, NULL));
            GRT_TRY(integrate_rows(p, b, bi, C, ps));
        }
        if (pass_direct(ps, bi))
        {
            GRT_TRY(direct_beam(p, b, bi, C, ps));
            GRT_TRY(direct_integrate(p, b, bi, C, ps));
        }
        GRT_TRY(response_rows(p, b, C, ps));
        if (pass_scatter(ps, bi))
        {
            GRT_TRY(scatter_spectral(p, b, C, 1, 0, ps));
        }
        GRT_TRY(pass_radiance_tail(p, b, bi, C, 1, ps, NULL));
        return GRTCODE_SUCCESS;
    }
    if (ps->out != NULL)
    {
        ThirdRows da;
        GRT_TRY(direct_partials(p, b, bi, ps, 1, &da));
        GRT_TRY(response_join(p, b, ps, 1, &da));
        if (ps->profile)
        {
            GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_LEVEL_PARTIALS],
                                     (size_t)p->max_cols*(size_t)pass_rows(p, ps)*b->nblocks, NULL));
        }
        double *partials = ps->profile ? b->scratch[GRT_SCRATCH_LEVEL_PARTIALS].d : b->partials;
        GRT_TRY(band_solver(p, b, bi, C, ps, partials, NULL, &da));
        GRT_TRY(pass_rows_out(p, b, bi, C, 1, ps, partials, &da));
        if (da.with_responses)
        {
            GRT_TRY(finish_responses(p, C, 1, ps, &da.responses));
        }
    }
    GRT_TRY(pass_scatter_radiances(p, b, bi, C, 1, ps, NULL));
    return GRTCODE_SUCCESS;
}

/* The all-sky pass of grt_pipeline_run_subcolumns for one band, S subcolumns of every column on this run's tau_gas
   (driver.c:503-589), its mean rows to out as grt_band_solve writes them.  ps->clouds: the band's tables staged
   subcolumn-major; ps->aer (grt_pipeline_run_sky): the aerosol object joins every subcolumn, from its column's table.  Fused form: the subcolumn instance of the all-sky solver over C x S grid rows, each subcolumn's
   partial sums in sub_partials, then their fixed-order mean (GRT_TAG_SUBCOLUMN_MEAN; S = 1: the fixed-order sum of
   grt_band_solve).  The shortwave's two-sweep forms park C x count columns at a time in the band's park block, count =
   what fits in its max_cols, in stream order.  Materialised form: per subcolumn the all-sky optics, the spectral solver
   and the sum of its fluxes; then the mean into the band's flux arrays, and the row-wise trapezoid. */
int grt_band_solve_subcolumns(GrtPipeline_t *p, GrtBand *b, int bi, int C, int S, GrtPass const *ps)
{
    int const V = p->num_levels;
    void *s = grt_dev_stream(p->device);
    if (!p->keep_spectra)
    {
        /* (in points at sc: the walks go over sc.first and sc.count, which the launchers alone read) */
        GrtSubcolumnArgs sc = {*ps->clouds, S, 0, 0};
        if (ps->out == NULL)
        {
            /* (grt_pipeline_run_sky_radiances without flux rows: the radiance kernel in the solver's place) */
            GRT_TRY(pass_radiance_tail(p, b, bi, C, S, ps, &sc));
            return GRTCODE_SUCCESS;
        }
        GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_SUB_PARTIALS],
                                 (size_t)p->max_cols*(size_t)S*(size_t)pass_rows(p, ps)*b->nblocks, NULL));
        double *sub_partials = b->scratch[GRT_SCRATCH_SUB_PARTIALS].d;
        ThirdRows da;
        GRT_TRY(direct_partials(p, b, bi, ps, S, &da));
        GRT_TRY(response_join(p, b, ps, S, &da));
        GrtSolverInstance const in = pass_instance(p, ps, NULL, &sc, &da, bi);
        SolverArgs a;
        GRT_TRY(solver_args(p, b, bi, C, ps, &in, sub_partials, &a));
        int const group = row_limit(p, C, bi == 1 && grt_sw_parks(&in, &a.sw));
        int const slot = grt_profile_begin(s, pass_tag(ps, bi));
        int krc = 0;
        for (sc.first = sc.count = 0; krc == 0 && walk(S, group, &sc.first, &sc.count); )
        {
            krc = solver_launch(s, bi, &in, &a);
        }
        grt_profile_end(s, slot);
        GRT_TRY(grt_dev_check(krc, bi == 0 ? "longwave subcolumn kernel" : "shortwave subcolumn kernel"));
        GRT_TRY(pass_scatter_radiances(p, b, bi, C, S, ps, &sc));
        if (da.with_responses)
        {
            GRT_TRY(finish_responses(p, C, S, ps, &da.responses));
        }
        GRT_TRY(pass_rows_out(p, b, bi, C, S, ps, sub_partials, &da));
        return GRTCODE_SUCCESS;
    }
    uint64_t const per = (uint64_t)C*(uint64_t)V*b->n, all = (uint64_t)p->max_cols*(uint64_t)V*b->n;
    GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_FLUX_SUM], 2*all, NULL));
    double *flux_sum = b->scratch[GRT_SCRATCH_FLUX_SUM].d;
    if (pass_direct(ps, bi))
    {
        GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_DIRECT_SUM], all, NULL));
    }
    double *direct_sum = b->scratch[GRT_SCRATCH_DIRECT_SUM].d;
    for (int j = 0; j < S; ++j)
    {
        GrtCloudArgs cj;
        GrtPass const pj = pass_draw(p, ps, C, j, &cj);
        GRT_TRY(pass_optics(p, b, C, &pj));
        if (pass_radiances(ps, bi))
        {
            GRT_TRY(band_radiances(p, b, C, S, j, &pj, NULL));
        }
        if (ps->out == NULL)
        {
            continue;
        }
        GRT_TRY(band_solver(p, b, bi, C, &pj, NULL, NULL, NULL));
        GRT_TRY(grt_dev_check(grt_launch_flux_accumulate(s, per, b->flux_up, flux_sum, j == 0), "flux sum kernel"));
        GRT_TRY(grt_dev_check(grt_launch_flux_accumulate(s, per, b->flux_down, flux_sum + all, j == 0),
                              "flux sum kernel"));
        if (pass_scatter(ps, bi))
        {
            GRT_TRY(scatter_spectral(p, b, C, S, j, &pj));
        }
        if (pass_direct(ps, bi))
        {
            GRT_TRY(direct_beam(p, b, bi, C, &pj));
            GRT_TRY(grt_dev_check(grt_launch_flux_accumulate(s, per, b->scratch[GRT_SCRATCH_DIRECT_BEAM].d, direct_sum,
                                                             j == 0), "flux sum kernel"));
        }
    }
    if (pass_radiances(ps, bi))
    {
        GRT_TRY(radiance_outputs(p, b, C, S, ps));
    }
    if (ps->out == NULL)
    {
        return GRTCODE_SUCCESS;
    }
    GRT_TRY(grt_dev_check(grt_launch_flux_mean(s, per, flux_sum, S, b->flux_up), "flux mean kernel"));
    GRT_TRY(grt_dev_check(grt_launch_flux_mean(s, per, flux_sum + all, S, b->flux_down), "flux mean kernel"));
    GRT_TRY(integrate_rows(p, b, bi, C, ps));
    if (pass_direct(ps, bi))
    {
        GRT_TRY(grt_dev_check(grt_launch_flux_mean(s, per, direct_sum, S, b->scratch[GRT_SCRATCH_DIRECT_BEAM].d),
                              "flux mean kernel"));
        GRT_TRY(direct_integrate(p, b, bi, C, ps));
    }
    GRT_TRY(response_rows(p, b, C, ps));
    return GRTCODE_SUCCESS;
}

/* The shortwave of grt_pipeline_run_zeniths and of a set of grt_pipeline_run_sky_zeniths: the pass under zr->zeniths sun
   angles per column on this run's tau_gas -- with clouds, as the mean over the S draws ps->clouds holds subcolumn-major,
   the same draws under every angle --, every angle's rows to zr->per_angle and their weighted mean to out as
   grt_band_solve writes its rows (either may be NULL).  Fused form: the partial sums of every (angle, draw) in
   zen_partials, slot (c Z + k) S + s.  Here, and nowhere else, is decided which kernel leaves them: six rows in one sweep
   may take the shared-layer kernel -- the clean pass unless GRT_ZENITH_SHARED=0 in the environment (read per call), a
   pass with clouds or aerosols only with GRT_ZENITH_SHARED=1 --, in as many launches as 65 535 grid rows
   of (column, draw, chunk) need; everything else takes the zenith instances of the solver over C x draws x angles grid
   rows, the two-sweep forms as many (draw, angle) pairs at a time as fit the band's park block of max_cols columns, in
   stream order.  The clean pass counts under GRT_TAG_ZENITH_SW, the others under GRT_TAG_SKY_ZENITH_SW.  Then the
   fixed-order mean (GRT_TAG_ZENITH_MEAN; zr->sky: GRT_TAG_SKY_ZENITH_MEAN).  Materialised form: per draw the pass's
   optics, per angle the spectral solver and the row-wise trapezoid into the (angle, draw) rows of zen_partials; then the
   same mean kernel (one block per row).
   grt_pipeline_run_sky_zeniths_direct (zr->surface, zr->direct): with a staged surface the fused instances take the
   GrtZenithSurfaceArgs join, and the materialised loop writes each angle's direct-albedo rows into a buffer of its own
   ahead of the angle's solve; with the direct beam the fused instances take the GrtDirectArgs join too (partial sums in
   GRT_SCRATCH_ZEN_DIRECT_PARTIALS at the same slots), the materialised loop runs the direct-beam kernel and its trapezoid
   per (angle, draw), and the same mean kernel folds the three rows or V into zr->direct_per_angle and zr->direct_out.
   grt_pipeline_run_sky_zeniths_slant (zr->slant; fused form alone): the instances take the GrtZenithSlantArgs join as well. */
int grt_band_solve_zeniths(GrtPipeline_t *p, GrtBand *b, int C, int S, GrtPass const *ps, GrtZenithRun const *zr)
{
    int const Z = zr->zeniths, rows = pass_rows(p, ps), out_offset = pass_offset(p, ps, 1);
    int const joined = ps->clouds != NULL || ps->aer != NULL;
    int const sw_tag = ps->clouds != NULL || ps->aer_pass ? GRT_TAG_SKY_ZENITH_SW : GRT_TAG_ZENITH_SW;
    void *s = grt_dev_stream(p->device);
    GrtScratch *block = &b->scratch[GRT_SCRATCH_ZEN_PARTIALS];
    /* grt_pipeline_run_sky_zeniths_direct: every angle's direct beam beside its rows, three rows or V at the same slots */
    GrtScratch *dblock = &b->scratch[GRT_SCRATCH_ZEN_DIRECT_PARTIALS];
    int const drows = direct_rows(p, ps);
    GrtZenithSurfaceArgs const *zs = zr->surface.tables != NULL ? &zr->surface : NULL;
    /* grt_pipeline_run_sky_zeniths_slant (fused form): the direct beam's cosine per layer; its instances always carry the
       direct beam, whose rows are folded below only where zr->direct asks for them */
    GrtZenithSlantArgs const *sl = zr->slant.mu_layer != NULL ? &zr->slant : NULL;
    unsigned nblocks = 1;
    S = ps->clouds != NULL ? S : 1;
    if (!p->keep_spectra)
    {
        nblocks = b->nblocks;
        GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*(size_t)Z*(size_t)S*(size_t)rows*nblocks, NULL));
        if (zr->direct || sl != NULL)
        {
            GRT_TRY(grt_scratch_need(p, dblock, (size_t)p->max_cols*(size_t)Z*(size_t)S*(size_t)drows*nblocks, NULL));
        }
        GrtDirectArgs const da = {dblock->d};
        /* (in points at za and sc: the loops below walk their first and count, which the launchers alone read) */
        GrtZenithArgs za = {zr->mu, Z, 0, 0};
        GrtSubcolumnArgs sc, *draws = pass_subcolumns(ps, S, &sc);
        GrtSolverInstance in = pass_instance(p, ps, NULL, draws, NULL, 1);
        in.zeniths = &za;
        in.direct = zr->direct || sl != NULL ? &da : NULL;
        in.zenith_surface = zs;
        in.zenith_slant = sl;
        SolverArgs a;
        GRT_TRY(solver_args(p, b, 1, C, ps, &in, block->d, &a));
        char const *env = getenv("GRT_ZENITH_SHARED");
        int const parks = grt_sw_parks(&in, &a.sw), limit = row_limit(p, C, parks);
        int const chunk = grt_zenith_chunk(draws, ps->aer, in.direct, zs, sl), chunks = (Z + chunk - 1)/chunk;
        int const shared = !ps->profile && !parks && chunks <= limit &&
                           (joined ? env != NULL && env[0] == '1' : !(env != NULL && env[0] == '0'));
        /* the grid rows a draw of a column takes in one launch: every chunk of the shared-layer kernel, which walks no
           angles (za stays as it is), or the angles of a launch of the zenith instances */
        int const per_draw = shared ? chunks : (limit < Z ? limit : Z);
        int const slot = grt_profile_begin(s, sw_tag);
        int krc = 0;
        for (sc.first = sc.count = 0; krc == 0 && walk(S, limit/per_draw, &sc.first, &sc.count); )
        {
            if (shared)
            {
                krc = grt_launch_sw_zeniths(s, &a.sw, &za, draws, ps->aer, in.direct, zs, sl);
                continue;
            }
            for (za.first = za.count = 0; krc == 0 && walk(Z, per_draw, &za.first, &za.count); )
            {
                krc = grt_launch_sw(s, &in, &a.sw);
            }
        }
        grt_profile_end(s, slot);
        GRT_TRY(grt_dev_check(krc, "shortwave zenith kernel"));
    }
    else
    {
        GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*(size_t)Z*(size_t)S*(size_t)rows, NULL));
        if (ps->profile)
        {
            GRT_TRY(level_rows(p, b));         /* (the table ahead of the call's other blocks, not at the first trapezoid) */
        }
        if (zr->direct)
        {
            GRT_TRY(grt_scratch_need(p, dblock, (size_t)p->max_cols*(size_t)Z*(size_t)S*(size_t)drows, NULL));
            GRT_TRY(grt_scratch_need(p, &b->scratch[GRT_SCRATCH_DIRECT_BEAM], (size_t)p->max_cols*(size_t)p->num_levels*b->n,
                                     NULL));
        }
        /* every angle's own direct albedo: the angle's rows [C][n] in a buffer of the call's own -- the rows of the surface
           in force are not written -- and, where the diffuse albedo is the creation-time array, a copy of it per column
           behind them: the solver reads both albedos at one stride */
        double *angle_rows = NULL, *dif_rows = NULL;
        if (zs != NULL)
        {
            GrtScratch *own = &b->scratch[GRT_SCRATCH_ZEN_SURF_ROWS];
            GRT_TRY(grt_scratch_need(p, own, 2*(size_t)p->max_cols*b->n, NULL));
            angle_rows = own->d;
            if (!b->surf_set)
            {
                dif_rows = own->d + (size_t)p->max_cols*b->n;
                for (int c = 0; c < C; ++c)
                {
                    GRT_TRY(grt_dev_copy(p->device, dif_rows + (size_t)c*b->n, p->albedo_d, sizeof(double)*b->n, s));
                }
            }
        }
        for (int j = 0; j < S; ++j)
        {
            GrtCloudArgs cj;
            GrtPass const pj = pass_draw(p, ps, C, j, &cj);
            GRT_TRY(pass_optics(p, b, C, &pj));
            GrtSolverInstance const in = pass_instance(p, &pj, NULL, NULL, NULL, 1);
            SolverArgs a;
            GRT_TRY(solver_args(p, b, 1, C, &pj, &in, NULL, &a));
            for (int k = 0; k < Z; ++k)
            {
                a.sw.mu_dir = zr->mu_by_angle + (size_t)k*C;
                if (zs != NULL)
                {
                    GrtSurfaceArgs const sa = {zs->num_entries, zs->entry,
                                               zs->tables + (size_t)k*(size_t)C*(size_t)zs->num_entries*2};
                    GRT_TIMED(s, GRT_TAG_SURFACE, "surface row kernel",
                              grt_launch_spread_surface(s, C, b->gas->grid.w0, b->gas->grid.dw, b->n, &sa, angle_rows));
                    a.sw.alb_dir = angle_rows;
                    a.sw.alb_dif = dif_rows != NULL ? dif_rows : a.sw.alb_dif;
                    a.sw.alb_stride = b->n;
                }
                GRT_TIMED(s, sw_tag, "shortwave kernel", grt_launch_sw(s, &in, &a.sw));
                GRT_TRY(integrate_rows_to(p, b, C, ps, GRT_UNTIMED, block->d, Z*S*rows, (k*S + j)*rows));
                if (zr->direct)
                {
                    /* the angle's direct beam on the grid from the draw's optics, and its row-wise trapezoid */
                    GRT_TIMED(s, GRT_TAG_DIRECT_BEAM, "direct-beam kernel",
                              grt_launch_sw_direct_beam(s, &a.sw, b->scratch[GRT_SCRATCH_DIRECT_BEAM].d));
                    GRT_TRY(direct_integrate_to(p, b, 1, C, ps, dblock->d, Z*S*drows, (k*S + j)*drows));
                }
            }
        }
    }
    GRT_TIMED(s, zr->sky ? GRT_TAG_SKY_ZENITH_MEAN : GRT_TAG_ZENITH_MEAN, "zenith mean kernel", zr->sky ?
              grt_launch_sky_zenith_mean(s, block->d, C, Z, S, rows, nblocks, zr->mu, zr->weight, zr->per_angle, zr->six,
                                         ps->sets, ps->set, p->user_level, ps->out, ps->out_stride, out_offset) :
              grt_launch_zenith_mean(s, block->d, C, Z, rows, nblocks, zr->mu, zr->weight, zr->per_angle, zr->six,
                                     p->user_level, ps->out, ps->out_stride, out_offset));
    if (zr->direct)
    {
        /* (the same kernel on the direct beam's three rows or V: the draws, one division, then the angles) */
        GRT_TIMED(s, GRT_TAG_SKY_ZENITH_MEAN, "zenith mean kernel",
                  grt_launch_sky_zenith_mean(s, dblock->d, C, Z, S, drows, nblocks, zr->mu, zr->weight, zr->direct_per_angle,
                                             NULL, ps->sets, ps->set, p->user_level, zr->direct_out, direct_stride(p, ps),
                                             direct_offset(p, ps)));
    }
    return GRTCODE_SUCCESS;
}

/* One set of grt_pipeline_run_sky_tiles for one band: the pass over ps->tiles->tiles surfaces per column on this run's
   tau_gas -- with clouds, as the mean over the S draws ps->clouds holds subcolumn-major, the same draws over every tile --,
   every tile's six rows to the pass's set of tiles->per_tile and their mean to out as grt_band_solve writes its rows
   (either may be NULL).  A band that was given knots reads the tiles' rows in GRT_SCRATCH_TILE_ROWS(_DIF); one that was
   not, the surface in force for every tile.  Fused form: the tile kernel of the pass's joins (GRT_TAG_TILE_LW / _SW), grid
   row = (column, draw of the launch), its chunks of grt_tile_chunk tiles along z, in as many launches as 65 535 grid rows
   and -- the shortwave's two sweeps -- the park block of max_cols rows need; the partial sums of every (tile, draw) in
   tile_partials, slot (c T + t) S + s.  Materialised form: per draw the pass's optics, per tile the spectral solver on the
   tile's rows and temperature and the row-wise trapezoid into the (tile, draw) rows of tile_partials.  Then the
   fixed-order mean (GRT_TAG_TILE_MEAN; materialised form: one block per row). */
int grt_band_solve_tiles(GrtPipeline_t *p, GrtBand *b, int bi, int C, int S, GrtPass const *ps)
{
    GrtTileRun const *tr = ps->tiles;
    int const T = tr->tiles, rows = GRT_FLUXES_PER_BAND, tag = bi == 0 ? GRT_TAG_TILE_LW : GRT_TAG_TILE_SW;
    void *s = grt_dev_stream(p->device);
    GrtScratch *block = &b->scratch[GRT_SCRATCH_TILE_PARTIALS];
    double const *tile_rows = tr->np[bi] > 0 ? b->scratch[GRT_SCRATCH_TILE_ROWS].d : NULL;
    double const *tile_rows_dif = tile_rows != NULL && bi == 1 && tr->dif ? b->scratch[GRT_SCRATCH_TILE_ROWS_DIF].d : NULL;
    unsigned nblocks = 1;
    S = ps->clouds != NULL ? S : 1;
    if (!p->keep_spectra)
    {
        nblocks = b->nblocks;
        GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*(size_t)T*(size_t)S*(size_t)rows*nblocks, NULL));
        /* (the loops below walk sc's and ta's first and count, which the launchers alone read) */
        GrtSubcolumnArgs sc, *draws = pass_subcolumns(ps, S, &sc);
        GrtSolverInstance const in = pass_instance(p, ps, NULL, draws, NULL, bi);
        SolverArgs a;
        GRT_TRY(solver_args(p, b, bi, C, ps, &in, block->d, &a));
        GrtTileArgs ta = {T, 0, 0, tr->t_surf, tile_rows, tile_rows_dif};
        int const chunk = grt_tile_chunk(draws, ps->aer), chunks = (T + chunk - 1)/chunk;
        /* (the chunks lie along the grid's z, so they count against the park block alone: the two sweeps park (draw, chunk)
           pairs of C rows each) */
        int const parks = bi == 1 && grt_sw_parks(&in, &a.sw), limit = row_limit(p, C, parks);
        int const per_launch = parks && limit < chunks ? limit : chunks;
        int const slot = grt_profile_begin(s, tag);
        int krc = 0;
        for (sc.first = sc.count = 0; krc == 0 && walk(S, parks ? limit/per_launch : limit, &sc.first, &sc.count); )
        {
            for (ta.chunk_first = ta.chunk_count = 0; krc == 0 && walk(chunks, per_launch, &ta.chunk_first, &ta.chunk_count); )
            {
                krc = bi == 0 ? grt_launch_lw_tiles(s, &a.lw, &ta, draws, ps->aer) :
                                grt_launch_sw_tiles(s, &a.sw, &ta, draws, ps->aer);
            }
        }
        grt_profile_end(s, slot);
        GRT_TRY(grt_dev_check(krc, bi == 0 ? "longwave tile kernel" : "shortwave tile kernel"));
    }
    else
    {
        GRT_TRY(grt_scratch_need(p, block, (size_t)p->max_cols*(size_t)T*(size_t)S*(size_t)rows, NULL));
        for (int j = 0; j < S; ++j)
        {
            GrtCloudArgs cj;
            GrtPass const pj = pass_draw(p, ps, C, j, &cj);
            GRT_TRY(pass_optics(p, b, C, &pj));
            GrtSolverInstance const in = pass_instance(p, &pj, NULL, NULL, NULL, bi);
            SolverArgs a;
            GRT_TRY(solver_args(p, b, bi, C, &pj, &in, NULL, &a));
            for (int t = 0; t < T; ++t)
            {
                /* the tile's rows and temperature in the columns' place */
                if (bi == 0)
                {
                    a.lw.t_surf = tr->t_surf_by_tile + (size_t)t*C;
                    if (tile_rows != NULL)
                    {
                        a.lw.emis = tile_rows + (size_t)t*b->n;
                        a.lw.emis_stride = (uint64_t)T*b->n;
                    }
                }
                else if (tile_rows != NULL)
                {
                    a.sw.alb_dir = tile_rows + (size_t)t*b->n;
                    a.sw.alb_dif = (tile_rows_dif != NULL ? tile_rows_dif : tile_rows) + (size_t)t*b->n;
                    a.sw.alb_stride = (uint64_t)T*b->n;
                }
                GRT_TIMED(s, tag, bi == 0 ? "longwave kernel" : "shortwave kernel", solver_launch(s, bi, &in, &a));
                GRT_TRY(integrate_rows_to(p, b, C, ps, GRT_UNTIMED, block->d, T*S*rows, (t*S + j)*rows));
            }
        }
    }
    GRT_TIMED(s, GRT_TAG_TILE_MEAN, "tile mean kernel",
              grt_launch_tile_mean(s, block->d, C, T, S, nblocks, tr->fraction, tr->per_tile, ps->sets, ps->set, bi, ps->out,
                                   ps->out_stride, pass_offset(p, ps, bi)));
    return GRTCODE_SUCCESS;
}

/* grt_pipeline_run_ck_fluxes, one band: the class sums of the sources under the map (k_kdist.hip), the solve of every
   g-point on the class means (k_longwave.hip / k_shortwave.hip: the solvers' own layer steps) and the classes' sum per bin.
   The temperatures, the surface in force, the sun and the solar curve are the ones the band's line-by-line solver reads. */
int grt_band_solve_ck(GrtPipeline_t *p, GrtBand *b, int bi, int C, int num_classes, int const *edges_dev,
                      unsigned short const *map_dev, double const *weight_sum, double const *tau_sum, double *source_sum,
                      GrtCkBand_t const *out)
{
    void *s = grt_dev_stream(p->device);
    int const V = p->num_levels;
    GrtPass ps;
    memset(&ps, 0, sizeof(ps));
    GrtCkSourceArgs src;
    memset(&src, 0, sizeof(src));
    src.longwave = bi == 0; src.num_levels = V; src.ncol = C; src.n = (long long)b->n;
    src.w0 = b->gas->grid.w0; src.dw = b->gas->grid.dw;
    src.num_classes = num_classes; src.num_bins = out->num_bins; src.edges = edges_dev; src.map = map_dev;
    src.source_sum = source_sum;
    GrtCkSolveArgs a;
    memset(&a, 0, sizeof(a));
    a.num_levels = V; a.ncol = C; a.num_bins = out->num_bins; a.num_classes = num_classes;
    a.weight_sum = weight_sum; a.tau_sum = tau_sum; a.source_sum = source_sum;
    a.flux_up = out->flux_up_dev; a.flux_down = out->flux_down_dev;
    if (bi == 0)
    {
        GrtLwArgs lw;
        lw_args(p, b, C, 1, &ps, &lw);
        src.t_levels = lw.t_levels; src.t_layers = lw.t_layers; src.t_surf = lw.t_surf;
        src.data[0] = lw.emis; src.data_stride[0] = lw.emis_stride;
    }
    else
    {
        GrtSwArgs sw;
        sw_args(p, b, C, 1, &ps, &sw);
        src.data[0] = sw.solar; src.data_stride[0] = 0;
        src.data[1] = sw.alb_dir; src.data_stride[1] = sw.alb_stride;
        src.data[2] = sw.alb_dif; src.data_stride[2] = sw.alb_stride;
        a.n_layer = sw.n_layer; a.mu_dir = sw.mu_dir; a.tsi = sw.tsi; a.mu_dif = sw.mu_dif;
    }
    int slot = grt_profile_begin(s, GRT_TAG_CK_SOURCES);
    int krc = grt_launch_ck_sources(s, &src);
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, "correlated-k source kernel"));
    slot = grt_profile_begin(s, bi == 0 ? GRT_TAG_CK_LW : GRT_TAG_CK_SW);
    krc = bi == 0 ? grt_launch_ck_lw(s, &a) : grt_launch_ck_sw(s, &a);
    if (krc == 0 && out->bin_up_dev != NULL)
    {
        long long const rows = (long long)C*V*out->num_bins;
        krc = grt_launch_ck_bin_sum(s, out->flux_up_dev, rows, num_classes, out->bin_up_dev);
        if (krc == 0)
        {
            krc = grt_launch_ck_bin_sum(s, out->flux_down_dev, rows, num_classes, out->bin_down_dev);
        }
    }
    grt_profile_end(s, slot);
    GRT_TRY(grt_dev_check(krc, bi == 0 ? "correlated-k longwave kernel" : "correlated-k shortwave kernel"));
    return GRTCODE_SUCCESS;
}
