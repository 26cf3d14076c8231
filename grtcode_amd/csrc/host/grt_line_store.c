/* grt_line_store.c -- the device line store: every molecule's host lines merged by centre into one structure of arrays
 * in HBM (GrtLineStore, grt_kernels.h), with the strengths rescaled on the way; for the line-sample method also the lean
 * first pass's packed records, for the sweep methods one store per molecule.
 *
 * Contract: the strength rescaling of parse_HITRAN_file.c:372-384; the molecule-by-molecule line lists of the sweep
 * methods, launch.c:78-159.
 *
 * Layout decisions (ours): one device allocation per store, its arrays each on a 256-byte boundary (v0, S as f64; the
 * five parameters the reference itself reads through a float as f32; iso and molecule slot as u8): 37 B/line instead of
 * the reference's 60 B.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "grt_internal.h"

/* parse_HITRAN_file.c:372-384: S <- S * Q(296)/(e^{c2 E/296} (1 - e^{c2 nu/296})).  The host keeps the
   tabulated 296 K strengths; this factor is applied when the device store is built (upload_lines), with
   the partition sums of the provider current at that moment (grt_tips.c), so that a table loaded after
   add_molecule() is never mixed with strengths scaled by another provider. */
/* one line; q296 [GRT_MAX_ISO + 1]: this molecule's Q(296 K, iso), filled on first use (negative = not yet) */
static inline void rescale_one(int mol_id, fp_t *q296, int iso, double v0, float en, double *s0)
{
    fp_t const tref = 296.f;
    fp_t const c2 = -1.4387686f;
    if (q296[iso] < 0.)
    {
        q296[iso] = Q(mol_id, tref, iso);
    }
    fp_t const e = en;
    *s0 *= q296[iso]/(exp(c2*e/tref)*(1.f - exp(c2*v0/tref)));
}

void grt_rescale_strengths(int mol_id, uint64_t n, uint8_t const *iso, double const *v0, float const *en,
                           double *s0)
{
    fp_t q296[GRT_MAX_ISO + 1];
    for (int k = 0; k <= GRT_MAX_ISO; ++k)
    {
        q296[k] = -1.;
    }
    for (uint64_t i = 0; i < n; ++i)
    {
        rescale_one(mol_id, q296, iso[i], v0[i], en[i], &s0[i]);
    }
}

typedef struct SortKey { double v0; uint32_t idx; uint8_t slot; } SortKey;

static int sort_key_cmp(void const *a, void const *b)
{
    SortKey const *x = a, *y = b;
    if (x->v0 < y->v0) return -1;
    if (x->v0 > y->v0) return 1;
    if (x->slot != y->slot) return x->slot < y->slot ? -1 : 1;
    return x->idx < y->idx ? -1 : (x->idx > y->idx ? 1 : 0);
}

/* The arrays of one store's device block, in block order (GrtLineStore).  The lean records exist in the merged store of
   the line-sample method only, and are kept per PAIR of lines: an odd store has one line of padding. */
enum { B_V0, B_S0, B_YAIR, B_YSELF, B_EN, B_NEXP, B_DELTA, B_ISO, B_SLOT, B_LEAN_A, B_LEAN_B, B_LEAN_C, B_LEAN_X, B_COUNT };

/* offsets of the arrays, each on a 256-byte boundary; returns the block's size */
static size_t block_layout(uint64_t total, int with_lean, size_t off[B_COUNT])
{
    static size_t const line_bytes[B_COUNT] = {
        [B_V0] = sizeof(double), [B_S0] = sizeof(double), [B_YAIR] = sizeof(float), [B_YSELF] = sizeof(float),
        [B_EN] = sizeof(float), [B_NEXP] = sizeof(float), [B_DELTA] = sizeof(float), [B_ISO] = 1, [B_SLOT] = 1,
        [B_LEAN_A] = 4*sizeof(float), [B_LEAN_B] = 4*sizeof(float), [B_LEAN_C] = sizeof(uint32_t), [B_LEAN_X] = 2*sizeof(double)};
    uint64_t const padded = 2*((total + 1)/2);
    size_t bytes = 0;
    for (int a = 0; a < (with_lean ? B_COUNT : B_LEAN_A); ++a)
    {
        off[a] = bytes;
        bytes = grt_align256(bytes + line_bytes[a]*(a >= B_LEAN_A ? padded : total));
    }
    return bytes;
}

/* The lean first pass (k_gas_optics_mp.hip: lean_block) works in fp32 from quantities that depend on the line and the
   grid only: the grid point nearest the unshifted centre and the centre's offset from it -- the pressure shift
   (kernels.c:44) is added to the offset per layer, and whenever that sum comes within 1e-5 of the halfway mark the line
   takes the general path, which forms kernels.c:431-432 in fp64 -- the strength scaled into fp32's range, and the
   temperature exponent as an index into the per-layer table of (296/T)^(k/100) (kernels.c:105).  The records of the
   lines l (rescaled strengths) on the grid w0 + i wres, in the layout GrtLineStore describes. */
static void pack_lean(GrtHostLines const *l, uint8_t const *slot, double w0, double wres, float *la, float *lb,
                      uint32_t *lc, double *lx)
{
    uint64_t const total = l->n, npair = (total + 1)/2;
    for (uint64_t k = 0; k < total; ++k)
    {
        double const uu = (l->v0[k] - w0)/wres;
        double const c0 = floor(uu + 0.5);
        uint32_t flags = 0;
        int32_t ci = 0;
        if (!(fabs(c0) < 1e9))
        {
            flags |= GRT_LEAN_GENERAL;
        }
        else
        {
            ci = (int32_t)c0;
        }
        double const ss = ldexp(l->s0[k], GRT_LEAN_S0_SHIFT);
        if (!(ss >= 0x1p-100 && ss <= 0x1p100))
        {
            flags |= GRT_LEAN_GENERAL;      /* (zero, negative or NaN strengths included) */
        }
        float const n100 = l->nexp[k]*100.f, nk = rintf(n100);
        uint32_t ik = 255;
        if (fabsf(n100 - nk) <= 2e-5f && nk >= 0.f && nk < 128.f)       /* (the kernel's own test, kPowTable entries) */
        {
            ik = (uint32_t)nk;
        }
        else
        {
            flags |= GRT_LEAN_GENERAL;
        }
        if (l->iso[k] < 1 || l->iso[k] > GRT_MAX_ISO)
        {
            flags |= GRT_LEAN_GENERAL;
        }
        /* pair q = k/2, half h = k%2: every field of the two lines side by side (GrtLineStore) */
        uint64_t const q = k >> 1, h = k & 1;
        float const sv = (flags & GRT_LEAN_GENERAL) ? 0.f : (float)ss;
        float const v0f = (float)l->v0[k];
        la[4*q + h] = (float)(uu - c0);
        memcpy(&la[4*q + 2 + h], &ci, sizeof(ci));
        la[4*(npair + q) + h] = v0f;
        la[4*(npair + q) + 2 + h] = sv;
        lb[4*q + h] = l->yair[k]; lb[4*q + 2 + h] = l->yself[k];
        lb[4*(npair + q) + h] = l->en[k]; lb[4*(npair + q) + 2 + h] = l->delta[k];
        uint32_t const ti = (uint32_t)slot[k]*GRT_MAX_ISO + (uint32_t)(l->iso[k] >= 1 ? l->iso[k] - 1 : 0);
        lc[k] = ik | ((uint32_t)slot[k] << 8) | ((ti & 1023u) << 14) | flags;
        lx[2*k] = l->v0[k];
        memcpy((char *)&lx[2*k + 1], &l->yair[k], 4);
        memcpy((char *)&lx[2*k + 1] + 4, &l->yself[k], 4);
        if (k + 1 == total && h == 0)
        {
            /* padding: the last line again, strength zero (never a line of any workgroup's range; finite numbers for
               the lanes that prepare it) */
            la[4*q + 1] = la[4*q]; la[4*q + 3] = la[4*q + 2];
            la[4*(npair + q) + 1] = v0f; la[4*(npair + q) + 3] = 0.f;
            lb[4*q + 1] = l->yair[k]; lb[4*q + 3] = l->yself[k];
            lb[4*(npair + q) + 1] = l->en[k]; lb[4*(npair + q) + 3] = l->delta[k];
            lc[k + 1] = lc[k] | GRT_LEAN_GENERAL;
        }
    }
}

/* Upload the lines named by `keys` (already in the wanted order) as one structure of arrays. */
/* with_lean: also the packed fp32 records of the lean first pass (GrtLineStore.lean_*), for the object's own grid. */
static int upload_lines(GasOptics_t *go, SortKey const *keys, uint64_t total, GrtLineStore *st, void **block,
                        size_t *bytes_out, int with_lean)
{
    GrtGasOpticsImpl *im = impl_of(go);
    size_t off[B_COUNT];
    size_t const bytes = block_layout(total, with_lean, off);
    unsigned char *host = malloc(bytes);
    if (host == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory staging %zu lines for the device.", (size_t)total);
    }
    /* the block's first eight arrays are those of GrtHostLines, in the same order */
    GrtHostLines staged = {total, (double *)(host + off[B_V0]), (double *)(host + off[B_S0]),
                           (float *)(host + off[B_YAIR]), (float *)(host + off[B_YSELF]), (float *)(host + off[B_EN]),
                           (float *)(host + off[B_NEXP]), (float *)(host + off[B_DELTA]), host + off[B_ISO]};
    uint8_t *slot = host + off[B_SLOT];
    st->n = total;
    st->dmax = 0.;
    st->nmax = 0.;
    memset(st->yair_max, 0, sizeof(st->yair_max));
    memset(st->yself_max, 0, sizeof(st->yself_max));
    for (uint64_t k = 0; k < total; ++k)
    {
        int const sl = keys[k].slot;
        grt_copy_host_line(&staged, k, &im->host[sl], keys[k].idx);
        slot[k] = keys[k].slot;
        double const ad = fabs((double)staged.delta[k]);
        if (ad > st->dmax) st->dmax = ad;
        if (staged.yair[k] > st->yair_max[sl]) st->yair_max[sl] = staged.yair[k];
        if (staged.yself[k] > st->yself_max[sl]) st->yself_max[sl] = staged.yself[k];
        if (fabs((double)staged.nexp[k]) > st->nmax) st->nmax = fabs((double)staged.nexp[k]);
    }
    /* strengths: tabulated -> the reference's pre-scaled form.  In a store merged by centre the molecules interleave
       line by line, so Q(296 K) is kept per (slot, isotopologue) for the whole build -- a few dozen evaluations of the
       provider instead of one per line */
    {
        static fp_t q296[GRT_MAX_SLOTS][GRT_MAX_ISO + 1];
        for (int sl = 0; sl < GRT_MAX_SLOTS; ++sl)
        {
            for (int k = 0; k <= GRT_MAX_ISO; ++k)
            {
                q296[sl][k] = -1.;
            }
        }
        for (uint64_t k = 0; k < total; ++k)
        {
            rescale_one(go->mols[slot[k]].id, q296[slot[k]], staged.iso[k], staged.v0[k], staged.en[k], &staged.s0[k]);
        }
    }
    if (with_lean)
    {
        pack_lean(&staged, slot, go->bins.w0, go->bins.wres, (float *)(host + off[B_LEAN_A]),
                  (float *)(host + off[B_LEAN_B]), (uint32_t *)(host + off[B_LEAN_C]), (double *)(host + off[B_LEAN_X]));
    }
    int rc = grt_dev_alloc(go->device, block, bytes);
    void *s = grt_dev_stream(go->device);
    if (rc == GRTCODE_SUCCESS) rc = grt_dev_upload(go->device, *block, host, bytes, s);
    if (rc == GRTCODE_SUCCESS) rc = grt_dev_sync(go->device, s);
    free(host);
    GRT_TRY(rc);
    unsigned char *d = *block;
    st->v0 = (double const *)(d + off[B_V0]);
    st->s0 = (double const *)(d + off[B_S0]);
    st->yair = (float const *)(d + off[B_YAIR]);
    st->yself = (float const *)(d + off[B_YSELF]);
    st->en = (float const *)(d + off[B_EN]);
    st->nexp = (float const *)(d + off[B_NEXP]);
    st->delta = (float const *)(d + off[B_DELTA]);
    st->iso = d + off[B_ISO];
    st->slot = d + off[B_SLOT];
    st->lean_a = with_lean ? (float const *)(d + off[B_LEAN_A]) : NULL;
    st->lean_b = with_lean ? (float const *)(d + off[B_LEAN_B]) : NULL;
    st->lean_c = with_lean ? (uint32_t const *)(d + off[B_LEAN_C]) : NULL;
    st->lean_x = with_lean ? (double const *)(d + off[B_LEAN_X]) : NULL;
    st->lean_npair = with_lean ? (total + 1)/2 : 0;
    st->lean_w0 = with_lean ? go->bins.w0 : 0.;
    st->lean_wres = with_lean ? go->bins.wres : 0.;
    if (bytes_out != NULL) *bytes_out = bytes;
    return GRTCODE_SUCCESS;
}

/* The sweep methods work molecule by molecule (launch.c:78-159): one store each, sorted by centre. */
static int upload_molecule_stores(GasOptics_t *go, SortKey const *keys, uint64_t total)
{
    GrtGasOpticsImpl *im = impl_of(go);
    SortKey *mk = malloc(sizeof(SortKey)*total);
    if (mk == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory for the per-molecule stores.%s", "");
    }
    int rc = GRTCODE_SUCCESS;
    for (int sl = 0; sl < go->num_molecules && rc == GRTCODE_SUCCESS; ++sl)
    {
        uint64_t n = 0;
        for (uint64_t k = 0; k < total; ++k)
        {
            if (keys[k].slot == sl) mk[n++] = keys[k];
        }
        if (n > 0)
        {
            rc = upload_lines(go, mk, n, &im->mstore[sl], &im->mstore_block[sl], NULL, 0);
        }
    }
    free(mk);
    GRT_TRY(rc);
    return GRTCODE_SUCCESS;
}

int grt_build_line_store(GasOptics_t *go)
{
    GrtGasOpticsImpl *im = impl_of(go);
    GRT_TRY(grt_free_line_store(go));
    uint64_t total = 0;
    for (int s = 0; s < go->num_molecules; ++s)
    {
        total += im->host[s].n;
    }
    im->store.n = total;
    if (total == 0)
    {
        im->store_dirty = 0;
        im->store_tips_generation = grt_tips_generation();
        return GRTCODE_SUCCESS;
    }
    SortKey *keys = malloc(sizeof(SortKey)*total);
    if (keys == NULL)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory sorting %zu lines.", (size_t)total);
    }
    uint64_t k = 0;
    for (int s = 0; s < go->num_molecules; ++s)
    {
        for (uint64_t j = 0; j < im->host[s].n; ++j, ++k)
        {
            keys[k].v0 = im->host[s].v0[j];
            keys[k].idx = (uint32_t)j;
            keys[k].slot = (uint8_t)s;
        }
    }
    qsort(keys, total, sizeof(SortKey), sort_key_cmp);
    size_t bytes = 0;
    int rc = upload_lines(go, keys, total, &im->store, &im->store_block, &bytes, go->optical_depth_method == line_sample);
    if (rc == GRTCODE_SUCCESS && go->optical_depth_method == line_sample)
    {
        /* the sorted centres stay on the host as well, for the launch's tile tables (grt_gas_launch.c) */
        im->sorted_v0_h = malloc(sizeof(double)*(size_t)total);
        for (uint64_t k = 0; k < total && im->sorted_v0_h != NULL; ++k) im->sorted_v0_h[k] = keys[k].v0;
    }
    else if (rc == GRTCODE_SUCCESS)
    {
        rc = upload_molecule_stores(go, keys, total);
    }
    free(keys);
    GRT_TRY(rc);
    im->store_dirty = 0;
    im->store_tips_generation = grt_tips_generation();
    GRT_INFO("Line store: %zu lines, %zu bytes on device %d.", (size_t)total, bytes, go->device);
    return GRTCODE_SUCCESS;
}

/* The stores and everything derived from them: the sweep scratch, the sorted centres and the launch's tile tables. */
int grt_free_line_store(GasOptics_t *go)
{
    GrtGasOpticsImpl *im = impl_of(go);
    GRT_TRY(grt_dev_free(go->device, im->store_block));
    im->store_block = NULL;
    memset(&im->store, 0, sizeof(im->store));
    for (int sl = 0; sl < NUM_MOLS; ++sl)
    {
        GRT_TRY(grt_dev_free(go->device, im->mstore_block[sl]));
        im->mstore_block[sl] = NULL;
        memset(&im->mstore[sl], 0, sizeof(im->mstore[sl]));
    }
    GRT_TRY(grt_dev_free(go->device, im->sweep_scratch));
    im->sweep_scratch = NULL;
    free(im->sorted_v0_h);
    im->sorted_v0_h = NULL;
    GRT_TRY(grt_dev_free(go->device, im->tile_ranges_d));
    im->tile_ranges_d = NULL;
    GRT_TRY(grt_dev_free(go->device, im->tile_items_d));
    im->tile_items_d = NULL;
    free(im->tile_items_h);
    free(im->tile_ranges_h);
    im->tile_items_h = im->tile_ranges_h = NULL;
    im->n_items = 0;
    im->tr_tile = 0;
    return GRTCODE_SUCCESS;
}
