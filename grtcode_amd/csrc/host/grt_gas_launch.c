/* grt_gas_launch.c -- the launch of a batch of columns on the line-by-line kernels: plan() decides the form and shape once
 * per batch without side effects, bind() binds one column group's buffers to it (the only step that may sync the stream). */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "grt_internal.h"
#include "../grt_work_order.h"

/* the kernels' work order as a host function (tests/test_work_order.py walks it) */
void grt_work_order(unsigned nb, unsigned per_group, unsigned ngroups, unsigned b, unsigned *group, unsigned *rem)
{
    grt_work_order_map(nb, per_group, ngroups, b, group, rem);
}

/* two-pass form: windows of more than this many points a side take the far field through the cell hierarchy */
#define TREE_MIN_FSTEPS 200
/* work list: crowded tiles go in pieces of ~ITEM_LINES lines, tiles of more than 1.6 ITEM_LINES lines are cut */
#define ITEM_LINES 10000u

/* What plan() decided for a batch: the launch's final form and shape, and what bind() has to provide for it. */
typedef struct LaunchPlan
{
    GrtGasOpticsArgs a;       /* the common fields and the form: fast, tile, nslice, tree_levels, mom_terms, rcap, halo, lean,
                                 narrow, direct_near, near_block, deterministic, gmom_stride; no column group, no scratch */
    int tables;               /* the tile tables are built for this launch (two-pass form, < 2^32 lines in the store) */
    int items;                /* ... and their work list taken in place of tiles x nslice equal slices (unless a probe is) */
    double pmax;              /* the batch's largest layer pressure: what the tile tables must cover */
    size_t moment_bytes;      /* cell moments one column needs (0: no two-pass form) */
    size_t radius_bytes;      /* near-field radius table one column needs (0: none) */
    uint64_t probe_words;     /* probe words one column needs (0: the form has no instrumented instance) */
} LaunchPlan;

static void auto_tune(GasOptics_t const *go, int ncol, int moments, int *tile, int *nslice)
{
    GrtGasOpticsImpl const *im = impl_of(go);
    uint64_t const nw = go->grid.n;
    /* lines a workgroup of `cells` cells has to prepare, on average */
    double const per_cell = nw > 0 ? (double)im->store.n/(double)nw : 0.;
    int t = im->tile;
    if (t == 0)
    {
        /* the one-pass moment kernel keeps tile + 2*fsteps cells of 8 moments in LDS next to the tile; the
           two-pass one only the tile's own cells, and its tiles are powers of two (256 measured best at
           1 cm-1: four workgroups per CU) */
        int want = moments == 2 ? 256 : (moments ? 512 : 1024);
        /* two-pass form on a short grid: narrower tiles before line slices (the G1 longwave band, 3 250 points x 60
           layers x 8 columns: 64-cell tiles in one slice 5.75 ms, 256-cell tiles in four slices 5.92 ms) -- as long as
           a tile keeps a few thousand lines: a workgroup's fixed costs (column state, the table of temperature powers,
           clearing and flushing its accumulators) are paid per tile.  One column of the G1 shortwave band (30 lines per
           cell): 256-cell tiles 1.91 ms, 128-cell tiles 1.98-2.14 ms. */
        /* Round 4: the same with MANY columns too while a tile holds more than ~24 000 lines -- all the (layer, column)
           workgroups of a tile read one slice of the line store, which should stay in an XCD's 4 MB L2 next to everything
           else: G1 longwave, 64 columns per launch, 256-cell tiles (79 000 lines, 2.8 MB of packed records) 40.2 ms,
           128-cell 36.5, 64-cell 34.9 (a tile-size sweep of bench.py; the script is at commit 625d7b3). */
        /* ONE column of that band with the round-4 lean first pass: 128-cell tiles in four slices 0.559 ms, 64-cell tiles
           in two 0.594, 256-cell in eight 0.581 (scripts/sweep_one_column.py) -- a lone column stops at 128 */
        /* Round 5 (all layers on the lean loop, region 2 inside it): with many columns the wide tile is ahead again -- G1
           longwave, 64 columns per launch: 256-cell tiles 22.35 ms, 128-cell 22.6, 64-cell 22.9-23.2 (a workgroup's fixed
           costs weigh more against a faster loop) -- so tiles are narrowed only to make workgroups, not for the L2's sake */
        while (moments == 2 && want > (ncol == 1 ? 128 : 64) && per_cell*(double)(want/2) >= 6000.
               && ((nw + want - 1)/want)*(uint64_t)go->num_layers*(uint64_t)ncol < 16384)
        {
            want >>= 1;
        }
        t = nw >= (uint64_t)want ? want : (int)(((nw + 63)/64)*64);
        if (moments == 2)
        {
            while (t & (t - 1))
            {
                t += 64;                /* next power of two */
            }
        }
    }
    int ns = im->nslice;
    if (ns == 0)
    {
        /* enough workgroups to cover 256 CUs (1 024 resident workgroups) several times over, but no slice of fewer than
           ~8 000 lines.  Measured, G1 longwave band (308 lines per cell), 8 columns x 256-cell tiles (6 240 workgroups
           unsliced): one slice 6.34 ms, two or four 6.14, eight 6.28; ONE column x 64-cell tiles (3 060 workgroups,
           19 700 lines each): one slice 0.85 ms, two 0.81, four 0.81, eight 0.90-0.99. */
        uint64_t const blocks = ((nw + t - 1)/t)*(uint64_t)go->num_layers*(uint64_t)ncol;
        double const per_tile = per_cell*(double)t;
        ns = 1;
        while (blocks*ns < 16384 && ns < 16 && per_tile/(double)(2*ns) >= 8000.)
        {
            ns *= 2;
        }
    }
    *tile = t;
    *nslice = ns;
}

/* Tree form of the two-pass kernel: a bound, over the batch's columns and layers, on how far from a line's
   centre index the first pass may add to tau -- near_radius() of k_gas_optics_mp.hip with the region-1 reach
   uncapped (the moment bound sep |z|max from the largest Lorentz width any line can have in a layer; Humlicek
   region 1, XLIM0 <= 123.4 Doppler units, at the top of the grid for the lightest molecule), plus a margin
   for the device's exp(). */
static int near_halo_bound(GasOptics_t const *go, int ncol, double w_top, double wres, double sep)
{
    GrtGasOpticsImpl const *im = impl_of(go);
    GrtColumnLayout const *lo = &im->layout;
    int const L = go->num_layers;
    double worst = 3.;
    for (int c = 0; c < ncol; ++c)
    {
        double const *cs = im->colstate_h + (size_t)c*lo->stride;
        for (int i = 0; i < L; ++i)
        {
            double gmax = 0., dop = 0.;
            for (int sl = 0; sl < go->num_molecules; ++sl)
            {
                double const *ms = cs + lo->off_ms + ((size_t)sl*L + i)*4;
                double const g = (double)im->store.yair_max[sl]*fabs(ms[1]) + (double)im->store.yself_max[sl]*fabs(ms[0]);
                gmax = g > gmax ? g : gmax;
                dop = ms[3] > dop ? ms[3] : dop;
            }
            double const eta = gmax*exp(im->store.nmax*fabs(cs[lo->off_lay + (size_t)i*4 + 3]))/wres;
            double const r_mp = ceil(sep*sqrt(0.25 + eta*eta));
            double const reach = 123.4*(0.83255461115*w_top*dop)/(0.832554611*wres) + 2.;
            worst = r_mp > worst ? r_mp : worst;
            worst = reach > worst ? reach : worst;
        }
    }
    worst = worst*1.001 + 2.;
    return worst < 1e9 ? (int)worst : 1000000000;
}

/* Two-pass form: which lines of the sorted store can have their centre in cell tile t -- searched here, once per (tile size,
   pressure bound), instead of by every workgroup (k_gas_optics_mp.hip: candidate_range_wave, ten dependent loads of v0 before
   a workgroup's waves can start).  A line's shifted centre is v0 + delta p (kernels.c:44), |delta| <= store.dmax, so with
   p up to the bound the candidates of the tile [F0, F1) lie in [w0 + (F0 - 1.5) wres - dmax p, w0 + (F1 + 0.5) wres + dmax p]
   -- the kernel's own margins; membership is decided line by line there, this is a superset.  The bound covers the batch
   (pmax, its largest layer pressure) with room to spare, so the tables are built once. */
static int tile_tables(GasOptics_t *go, GrtGasOpticsArgs const *a, double pmax)
{
    GrtGasOpticsImpl *im = impl_of(go);
    uint64_t const tiles = (a->nw + (uint64_t)a->tile - 1)/(uint64_t)a->tile;
    if (im->tile_ranges_d != NULL && im->tr_tile == a->tile && im->tr_tiles == tiles && pmax <= im->tr_pbound)
    {
        return GRTCODE_SUCCESS;
    }
    double const pbound = pmax*1.25 > 2. ? pmax*1.25 : 2.;
    uint32_t *host = malloc(sizeof(uint32_t)*2*(size_t)tiles);
    if (host == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for %zu tile ranges.", (size_t)tiles);
    }
    double const *v = im->sorted_v0_h;
    uint64_t const n = im->store.n;
    double const shift = im->store.dmax*pbound;
    for (uint64_t t = 0; t < tiles; ++t)
    {
        double const F0 = (double)(t*(uint64_t)a->tile);
        double const F1 = (double)((t + 1)*(uint64_t)a->tile < a->nw ? (t + 1)*(uint64_t)a->tile : a->nw);
        double const wlo = a->w0 + (F0 - 1.5)*a->wres - shift, whi = a->w0 + (F1 + 0.5)*a->wres + shift;
        uint64_t l = 0, h = n;
        while (l < h)
        {
            uint64_t const m = (l + h) >> 1;
            if (v[m] < wlo) l = m + 1; else h = m;
        }
        host[2*t] = (uint32_t)l;
        h = n;
        while (l < h)
        {
            uint64_t const m = (l + h) >> 1;
            if (v[m] <= whi) l = m + 1; else h = m;
        }
        host[2*t + 1] = (uint32_t)l;
    }
    /* The same ranges as a work list cut by line count (GrtGasOpticsArgs.tile_items): a tile that holds more than
       ~16 000 candidate lines goes in pieces of ~10 000 (at most 16) -- what the measured one-column optimum of a dense
       band comes to (G1 longwave, 308 lines per cell: 128-cell tiles in four slices) -- and a sparse tile in one. */
    uint32_t *items = malloc(sizeof(uint32_t)*4*16*(size_t)tiles);
    uint32_t n_items = 0;
    int cut = 1;                    /* the largest number of pieces a tile goes in */
    uint32_t const cut_from = ITEM_LINES + ITEM_LINES*3u/5u;
    for (uint64_t t = 0; t < tiles && items != NULL; ++t)
    {
        uint32_t const lo_j = host[2*t], hi_j = host[2*t + 1], cnt = hi_j - lo_j;
        uint32_t pieces = cnt > cut_from ? (cnt + ITEM_LINES/2u)/ITEM_LINES : 1u;
        pieces = pieces > 16u ? 16u : pieces;
        cut = (int)pieces > cut ? (int)pieces : cut;
        uint32_t const per = (cnt + pieces - 1u)/pieces;
        for (uint32_t k = 0; k < pieces; ++k)
        {
            uint32_t const b = lo_j + per*k < hi_j ? lo_j + per*k : hi_j;
            uint32_t const e = b + per < hi_j ? b + per : hi_j;
            items[4*(size_t)n_items] = (uint32_t)t;
            items[4*(size_t)n_items + 1] = b;
            items[4*(size_t)n_items + 2] = e;
            items[4*(size_t)n_items + 3] = k;
            ++n_items;
        }
    }
    GRT_TRY(grt_dev_sync(go->device, grt_dev_stream(go->device)));      /* (a launch may still read the old tables) */
    GRT_TRY(grt_dev_free(go->device, im->tile_ranges_d));
    im->tile_ranges_d = NULL;
    GRT_TRY(grt_dev_free(go->device, im->tile_items_d));
    im->tile_items_d = NULL;
    im->n_items = 0;
    int rc = grt_dev_alloc(go->device, (void **)&im->tile_ranges_d, sizeof(uint32_t)*2*(size_t)tiles);
    void *s = grt_dev_stream(go->device);
    if (rc == GRTCODE_SUCCESS) rc = grt_dev_upload(go->device, im->tile_ranges_d, host, sizeof(uint32_t)*2*(size_t)tiles, s);
    if (rc == GRTCODE_SUCCESS && items != NULL)
    {
        rc = grt_dev_alloc(go->device, (void **)&im->tile_items_d, sizeof(uint32_t)*4*(size_t)n_items);
        if (rc == GRTCODE_SUCCESS) rc = grt_dev_upload(go->device, im->tile_items_d, items, sizeof(uint32_t)*4*(size_t)n_items, s);
    }
    if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(go->device, s);
    free(im->tile_ranges_h);
    free(im->tile_items_h);
    im->tile_ranges_h = host;           /* (kept: grt_debug_tile_items) */
    im->tile_items_h = items;
    GRT_TRY(rc);
    im->n_items = im->tile_items_d != NULL ? n_items : 0;
    im->items_cut = cut;
    im->tr_tile = a->tile;
    im->tr_tiles = tiles;
    im->tr_pbound = pbound;
    return GRTCODE_SUCCESS;
}

/* Deterministic mode (grt_ext.h): -1 = follow GRT_DETERMINISTIC in the environment (read at every launch, so that a
   test can switch it inside one process), 0 / 1 = forced off / on. */
static int g_deterministic = -1;

EXTERN int grt_set_deterministic(int on)
{
    GRT_REQUIRE_RANGE(on, -1, 1);
    g_deterministic = on;
    return GRTCODE_SUCCESS;
}

EXTERN int grt_deterministic(void)
{
    if (g_deterministic >= 0)
    {
        return g_deterministic;
    }
    char const *env = getenv("GRT_DETERMINISTIC");
    return env != NULL && env[0] != '\0' && !(env[0] == '0' && env[1] == '\0');
}

int grt_gas_optics_defer_tables(GasOptics_t *go, int on)
{
    GrtGasOpticsImpl *im = impl_of(go);
    im->defer_tables = on != 0 && go->optical_depth_method == line_sample;
    return im->defer_tables;
}

void grt_gas_optics_continua(GasOptics_t *go, GrtContinua *c)
{
    GrtGasOpticsImpl *im = impl_of(go);
    memset(c, 0, sizeof(*c));
    c->colstate = im->colstate_d;
    c->stride = im->layout.stride;
    c->off_cont = im->layout.off_cont;
    c->off_h2o = im->layout.off_h2o;
    c->tables = im->lin_tables;
    c->h2o_tables = im->h2o_tables;
    c->num_tables = im->num_lin;
    c->has_h2o_ctm = im->h2o_tables != NULL;
    c->spans = im->spans;
}

void grt_gas_common_args(GasOptics_t const *go, int ncol, double *tau, uint64_t tau_col_stride, GrtGasOpticsArgs *a)
{
    GrtGasOpticsImpl const *im = impl_of(go);
    memset(a, 0, sizeof(*a));
    a->lines = im->store;
    a->lay = im->layout;
    a->colstate = im->colstate_d;
    a->tables = im->lin_tables;
    a->h2o_tables = im->h2o_tables;
    a->spans = im->spans;
    a->skip_tables = im->defer_tables && go->optical_depth_method == line_sample;
    a->w0 = go->bins.w0;
    a->wres = go->bins.wres;
    a->nw = go->bins.num_wpoints;
    a->ncol = ncol;
    a->tau = tau;
    a->tau_col_stride = tau_col_stride;
    a->fast = im->fast;
}

/* The launch of a batch of ncol columns (their states in colstate_h): tiles, slices and bounds are chosen for the BATCH,
   also where it runs in column groups (grt_gas_launch_columns). */
static void plan(GasOptics_t const *go, int ncol, LaunchPlan *p)
{
    GrtGasOpticsImpl const *im = impl_of(go);
    GrtGasOpticsArgs *a = &p->a;
    memset(p, 0, sizeof(*p));
    grt_gas_common_args(go, ncol, NULL, 0, a);
    long long const fsteps = (long long)ceil((double)25.f/a->wres);
    if (im->fast == 1 || im->fast == 3)
    {
        /* fused form: far wings by cell moments where the grid's windows are wide enough for that */
        auto_tune(go, ncol, im->fast == 3 ? 2 : 1, &a->tile, &a->nslice);
        a->rcap = 12;
        if (im->fast == 3)
        {
            /* two passes: the cells' moments travel through global memory.  Windows of more than 200 points a
               side (grids finer than ~0.12 cm-1; measured equal at 0.2, 8 % ahead at 0.1, 1.5x at 0.05 cm-1):
               far field through the cell hierarchy */
            a->halo = (int)(fsteps < 0x3fffffff ? fsteps : 0x3fffffff);
            a->mom_terms = 8;
            if (fsteps > TREE_MIN_FSTEPS)
            {
                int levels = 0;
                while ((4ll << (levels + 1)) <= fsteps && levels < 20)     /* cells of up to fsteps/4 points */
                {
                    ++levels;
                }
                a->tree_levels = levels;
                a->nslice = 1;
                double const w_top = a->w0 + ((double)a->nw + (double)fsteps)*a->wres;
                /* Cell tiles and moments per cell, in order of preference (measured on 0.001-0.01 cm-1, 10^6 lines):
                   two cells per line and more -- tiles of 1 024 cells (3 workgroups per CU), moments added straight to
                   global memory lane by lane, twelve of them (half the near field in the pressure-broadened layers);
                   denser lines -- tiles of 512 cells (256 below half a cell per line), eight moments reduced in
                   registers and kept in LDS.  Each falls back to the other, then to narrower tiles, where the
                   first pass's tile + 2*halo accumulators do not fit LDS. */
                uint64_t const per_line = a->lines.n > 0 ? a->nw/a->lines.n : a->nw;
                int sparse_tile = 1024;
                while ((uint64_t)sparse_tile < 128*per_line && sparse_tile < 2048) sparse_tile <<= 1;
                int const dense_tile = 2*a->nw >= a->lines.n ? 512 : 256;
                int cand[8], ncand = 0;
                if (im->tile != 0)
                {
                    cand[ncand++] = im->tile;
                }
                else if (per_line >= 2)
                {
                    cand[ncand++] = sparse_tile; cand[ncand++] = 1024; cand[ncand++] = dense_tile;
                    cand[ncand++] = 256; cand[ncand++] = 128; cand[ncand++] = 64;
                }
                else
                {
                    cand[ncand++] = dense_tile; cand[ncand++] = 1024; cand[ncand++] = 256;
                    cand[ncand++] = 128; cand[ncand++] = 64;
                }
                for (int k = 0; k < ncand; ++k)
                {
                    a->tile = cand[k];
                    while ((uint64_t)a->tile > a->nw && a->tile > 64) a->tile >>= 1;
                    a->mom_terms = a->tile > 512 ? 12 : 8;
                    a->rcap = near_halo_bound(go, ncol, w_top, a->wres, grt_gas_optics_moment_separation(a->mom_terms));
                    /* (near fields may be rounded out to 64-point blocks, GrtGasOpticsArgs.near_block; never beyond the window) */
                    a->halo = (long long)a->rcap + 64 < fsteps ? a->rcap + 64 : (int)fsteps;
                    if (grt_gas_optics_mp_shape(a))
                    {
                        break;
                    }
                }
            }
            a->gmom_stride = grt_gas_optics_moment_floats(a->nw, a->tree_levels, a->mom_terms);
        }
        if (!grt_gas_optics_mp_shape(a))
        {
            a->fast = im->fast == 3 ? 1 : 2;
            a->tree_levels = 0;
            a->mom_terms = 0;
            a->rcap = 12;
            if (a->fast == 1)
            {
                auto_tune(go, ncol, 1, &a->tile, &a->nslice);
                if (!grt_gas_optics_mp_shape(a))
                {
                    a->fast = 2;
                }
            }
        }
    }
    if (a->fast != 1 && a->fast != 3)
    {
        auto_tune(go, ncol, 0, &a->tile, &a->nslice);
    }
    a->direct_near = a->fast == 1 || a->fast == 3;
    uint64_t const tiles = (a->nw + (uint64_t)a->tile - 1)/(uint64_t)a->tile;
    if (a->fast == 3)
    {
        char const *lean = getenv("GRT_LEAN");                 /* GRT_LEAN=0: the general line loop everywhere */
        a->lean = !(lean != NULL && lean[0] == '0') && grt_gas_optics_lean_shape(a);
        /* a single-level band that ends below 4 000 cm-1 -- the longwave -- takes the narrow-Doppler instance: 6.05 -> 5.9 ms
           at 1 cm-1; on the shortwave band the extra code cost more than the few waves it serves gained */
        a->narrow = a->tree_levels == 0 && a->w0 + (double)a->nw*a->wres <= 4000.;
        a->near_block = a->tree_levels > 0 && grt_tree_gather_by_wave(fsteps) ? 64 : 0;
        p->moment_bytes = sizeof(float)*(size_t)a->gmom_stride*(size_t)go->num_layers;
        /* (the cell tiles' near-field radii, worked out once per launch for the single-level gather's workgroups) */
        p->radius_bytes = a->tree_levels == 0 ? sizeof(int)*(size_t)tiles*(size_t)go->num_layers : 0;
        if (a->tree_levels == 0 || a->mom_terms == 12)
        {
            /* the instrumented instance of the two-pass first pass (cost analysis): 24 words per workgroup */
            p->probe_words = 24*tiles*(uint64_t)a->nslice*(uint64_t)go->num_layers;
        }
        p->tables = im->sorted_v0_h != NULL && im->store.n > 0 && im->store.n < 0xffffffffull;
        for (int c = 0; c < ncol && p->tables && im->colstate_h != NULL; ++c)
        {
            double const *lay = im->colstate_h + (size_t)c*im->layout.stride + im->layout.off_lay;
            for (int i = 0; i < go->num_layers; ++i)
            {
                p->pmax = fabs(lay[(size_t)i*4]) > p->pmax ? fabs(lay[(size_t)i*4]) : p->pmax;
            }
        }
        /* the work list instead of tiles x nslice equal slices: few workgroups (a lone column, a small batch), the flat
           two-pass form, slices left to the library (tune(nslice = 0)); GRT_TILE_ITEMS=0 keeps the equal slices */
        char const *env = getenv("GRT_TILE_ITEMS");
        p->items = p->tables && im->nslice == 0 && a->tree_levels == 0 && !grt_deterministic()
                   && !(env != NULL && env[0] == '0') && tiles*(uint64_t)go->num_layers*(uint64_t)ncol < 16384;
    }
    if (grt_deterministic())
    {
        /* one line slice per tile (slices add to tau in the scheduler's order), one wave per workgroup on the lines, the
           two-pass form's first pass in launches of non-overlapping tiles: k_gas_optics_mp.hip */
        a->deterministic = 1;
        a->nslice = 1;
    }
}

/* a scratch buffer of the object at least `need` bytes long */
static int grow(GasOptics_t *go, void **buf, size_t *have, size_t need)
{
    if (need > *have)
    {
        GRT_TRY(grt_dev_free(go->device, *buf));
        *buf = NULL;
        *have = 0;
        GRT_TRY(grt_dev_alloc(go->device, buf, need));
        *have = need;
    }
    return GRTCODE_SUCCESS;
}

/* The plan's launch for columns c0 .. c0 + ncol - 1 of the batch, with the object's buffers bound. */
static int bind(GasOptics_t *go, LaunchPlan const *p, int c0, int ncol, double *tau, uint64_t tau_col_stride,
                GrtGasOpticsArgs *a)
{
    GrtGasOpticsImpl *im = impl_of(go);
    *a = p->a;
    a->ncol = ncol;
    a->colstate = im->colstate_d + (size_t)c0*im->layout.stride;
    a->tau = tau + (size_t)c0*tau_col_stride;
    a->tau_col_stride = tau_col_stride;
    if (p->moment_bytes > 0)
    {
        GRT_TRY(grow(go, (void **)&im->gmom, &im->gmom_bytes, p->moment_bytes*(size_t)ncol));
        a->gmom = im->gmom;
    }
    if (p->radius_bytes > 0)
    {
        GRT_TRY(grow(go, (void **)&im->radius_table, &im->radius_bytes, p->radius_bytes*(size_t)ncol));
        a->radius_table = im->radius_table;
    }
    if (im->probe != NULL && p->probe_words > 0 && p->probe_words*(uint64_t)ncol <= im->probe_words)
    {
        a->probe = im->probe;
        a->lean = 0;                    /* (the instrumented instance is one of the general line loop) */
    }
    if (p->tables)
    {
        GRT_TRY(tile_tables(go, a, p->pmax));
        a->tile_ranges = im->tile_ranges_d;
        if (p->items && a->probe == NULL && im->n_items > 0)
        {
            a->tile_items = im->tile_items_d;
            a->n_items = im->n_items;
            a->nslice = im->items_cut > 1 ? 2 : 1;
        }
    }
    return GRTCODE_SUCCESS;
}

/* launch.c:40-226 with optical_depth_method wavenumber_sweep / line_sweep, one column at a time: continua,
   CFCs and CIA first (the line kernel with an empty line list writes exactly those), then molecule by
   molecule the per-(layer, line) preparation, the per-layer sort (wavenumber_sweep) and the sweep, then the
   interpolation of the bins' line-wing values onto the grid. */
static int launch_sweep_columns(GasOptics_t *go, int ncol, double *tau_dev, uint64_t tau_col_stride)
{
    GrtGasOpticsImpl *im = impl_of(go);
    void *s = grt_dev_stream(go->device);
    int const L = go->num_layers;
    uint64_t nmax = 0;
    for (int sl = 0; sl < go->num_molecules; ++sl)
    {
        if (im->mstore[sl].n > nmax) nmax = im->mstore[sl].n;
    }
    if (nmax > 0 && im->sweep_scratch == NULL)
    {
        GRT_TRY(grt_dev_alloc(go->device, (void **)&im->sweep_scratch, sizeof(double)*8*(size_t)L*nmax));
    }
    GRT_TRY(grt_gas_optics_upload_states(go, ncol));
    GrtSweepBins bins = {go->bins.w0, go->bins.wres, go->bins.num_wpoints, go->bins.n, go->bins.ppb,
                         go->bins.do_interp, go->bins.do_last_interp, go->bins.w, go->bins.tau, go->bins.l, go->bins.r};
    int const method = go->optical_depth_method == wavenumber_sweep ? 0 : 1;
    for (int c = 0; c < ncol; ++c)
    {
        double const *cs = im->colstate_d + (size_t)c*im->layout.stride;
        double *tau = tau_dev + (size_t)c*tau_col_stride;
        GrtGasOpticsArgs args;
        grt_gas_common_args(go, 1, tau, tau_col_stride, &args);
        args.colstate = cs;
        args.fast = 0;
        auto_tune(go, 1, 0, &args.tile, &args.nslice);
        args.nslice = 1;
        GrtLineStore const all = args.lines;
        args.lines.n = 0;
        GRT_TRY(grt_dev_check(grt_launch_gas_optics(s, &args), "continuum pass"));
        GRT_TRY(grt_dev_zero(go->device, go->bins.tau, sizeof(fp_t)*go->bins.isize*(size_t)L, s));
        for (int sl = 0; sl < go->num_molecules; ++sl)
        {
            uint64_t const n = im->mstore[sl].n;
            if (n == 0)
            {
                continue;
            }
            double *prep = im->sweep_scratch, *sorted = im->sweep_scratch + 4*(size_t)L*nmax;
            args.lines = im->mstore[sl];
            GRT_TRY(grt_dev_check(grt_launch_line_prep(s, &args, 0, prep, prep + (size_t)L*n, prep + 2*(size_t)L*n,
                                                       prep + 3*(size_t)L*n, NULL, NULL), "line prep kernel"));
            double const *lines = prep;
            /* wavenumber_sweep needs the reference's per-layer sort_lines; line_sweep runs bin-parallel here,
               which needs the same order */
            {
                GRT_TRY(grt_dev_check(grt_launch_sweep_sort(s, n, L, im->mstore[sl].v0, im->mstore[sl].dmax,
                                                            cs + im->layout.off_lay, prep, sorted), "sweep sort kernel"));
                lines = sorted;
            }
            double const *ns = cs + im->layout.off_ms + ((size_t)sl*L)*4 + 2;
            GRT_TRY(grt_dev_check(grt_launch_sweep(s, method, n, L, lines, ns, &bins, tau), "sweep kernel"));
        }
        args.lines = all;
        GRT_TRY(grt_dev_check(grt_launch_sweep_interpolate(s, L, &bins, tau), "sweep interpolation kernel"));
    }
    return GRTCODE_SUCCESS;
}

/* Scratch the library may hold for one launch's cell moments [bytes]: GRT_SCRATCH_CAP_MB in the environment (read at every
   launch: tests), else 60 % of what the device had free, plus what this object already held, when a batch of this object
   first did not fit. */
static size_t scratch_cap(GasOptics_t *go)
{
    GrtGasOpticsImpl *im = impl_of(go);
    char const *env = getenv("GRT_SCRATCH_CAP_MB");
    if (env != NULL && atof(env) > 0.)
    {
        return (size_t)(atof(env)*1048576.);
    }
    if (im->scratch_cap_bytes == 0)
    {
        /* asked ONCE per object: a cap that followed the free memory would grow with every batch (what the object holds is
           no longer free), and every growth is a hipFree + hipMalloc of tens of GB -- seconds on this runtime */
        size_t free_b = 0, total_b = 0;
        if (grt_dev_mem_info(go->device, &free_b, &total_b) != GRTCODE_SUCCESS)
        {
            return (size_t)-1;
        }
        im->scratch_cap_bytes = (size_t)(0.6*(double)free_b) + im->gmom_bytes;
    }
    return im->scratch_cap_bytes;
}

static int launch_column_group(GasOptics_t *go, LaunchPlan const *p, int c0, int ncol, double *tau_dev,
                               uint64_t tau_col_stride)
{
    GrtGasOpticsImpl *im = impl_of(go);
    void *s = grt_dev_stream(go->device);
    GrtGasOpticsArgs args;
    GRT_TRY(bind(go, p, c0, ncol, tau_dev, tau_col_stride, &args));
    if (args.nslice > 1)
    {
        /* slices accumulate with atomics (launch.c:61 zeroes tau in every case) */
        GRT_TRY(grt_dev_zero(go->device, args.tau, sizeof(double)*tau_col_stride*ncol, s));
    }
    _Static_assert(GRT_TAG_FAR_LW == GRT_TAG_GAS_LW + GRT_TAG_FAR_OFFSET && GRT_TAG_FAR_SW == GRT_TAG_GAS_SW + GRT_TAG_FAR_OFFSET,
                   "the far-field gather's tags follow the line kernel's");
    int const tag = im->profile_tag ? im->profile_tag : (args.nw <= 10000 ? GRT_TAG_GAS_LW : GRT_TAG_GAS_SW);
    /* (with a work list, "nslice" reports the largest number of pieces a tile was cut into) */
    long long const info[8] = {args.fast, args.tile, args.tile_items != NULL ? im->items_cut : args.nslice, args.tree_levels, args.fast == 3 ? args.halo : 0,
                               args.fast == 3 ? (long long)im->gmom_bytes : 0,
                               (args.fast == 1 || args.fast == 3) ? (args.mom_terms ? args.mom_terms : 8) : 0, ncol};
    memcpy(im->last_launch, info, sizeof(info));
    int rc;
    if (args.fast == 3)
    {
        args.profile_tag = tag;         /* the launcher times its two kernels separately */
        rc = grt_launch_gas_optics(s, &args);
    }
    else
    {
        int const slot = grt_profile_begin(s, tag);
        rc = grt_launch_gas_optics(s, &args);
        grt_profile_end(s, slot);
    }
    GRT_TRY(grt_dev_check(rc, "gas optics kernel"));
    return GRTCODE_SUCCESS;
}

/* The batch's columns, all in one launch -- or, where the cell moments of all of them would not fit the device (18.7 GB
   per column on the 0.001 cm-1 grid), in the largest column groups that do, one after the other on the stream through
   the same scratch.  Every group is launched with the one plan of the undivided batch (its bounds are the batch's:
   near_halo_bound, the tile tables' pressure bound), so a column's optical depths do not depend on how the batch was
   divided -- bit for bit in the deterministic mode.  The reference has no such limit either: one column per call, whatever
   the grid (gas_optics.c:433-454). */
int grt_gas_launch_columns(GasOptics_t *go, int ncol, double *tau_dev, uint64_t tau_col_stride)
{
    GrtGasOpticsImpl *im = impl_of(go);
    if (go->optical_depth_method != line_sample)
    {
        return launch_sweep_columns(go, ncol, tau_dev, tau_col_stride);
    }
    GRT_TRY(grt_gas_optics_upload_states(go, ncol));
    LaunchPlan p;
    plan(go, ncol, &p);
    int group = ncol;
    size_t const per = p.moment_bytes;
    if (ncol > 1 && per > 0 && per*(size_t)ncol > im->gmom_bytes)
    {
        size_t const cap = scratch_cap(go);
        if (per*(size_t)ncol > cap)
        {
            group = (int)(cap/per);
            group = group < 1 ? 1 : group;
        }
    }
    int rc = GRTCODE_SUCCESS;
    for (int c0 = 0; c0 < ncol && rc == GRTCODE_SUCCESS; c0 += group)
    {
        rc = launch_column_group(go, &p, c0, ncol - c0 < group ? ncol - c0 : group, tau_dev, tau_col_stride);
    }
    im->last_launch[7] = group;         /* columns per launch (grt_gas_optics_last_launch) */
    GRT_TRY(rc);
    return GRTCODE_SUCCESS;
}
