/* grt_hitran.c -- the HITRAN line-list reader: one molecule's lines from a .par file into host staging (GrtHostLines),
 * through an index of every molecule parsed once per file, kept in memory and optionally on disk.
 *
 * Contract: parse_HITRAN_file.c:224-413 (records :77-100, isotopologue codes :177-194, the float fields :197-212, the
 * range filter :340).  The strengths stay as tabulated (296 K): the rescaling of :372-384 is applied when the device
 * store is built (grt_line_store.c).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include "grt_internal.h"

/* The arrays of GrtHostLines, described once: where each pointer sits in the struct and the bytes of one element.  This
   order is the on-disk index's (file order = checksum order); reserve, free and copy walk the same list. */
static struct { size_t at, width; } const g_arrays[] = {
    {offsetof(GrtHostLines, v0), sizeof(double)}, {offsetof(GrtHostLines, s0), sizeof(double)},
    {offsetof(GrtHostLines, yair), sizeof(float)}, {offsetof(GrtHostLines, yself), sizeof(float)},
    {offsetof(GrtHostLines, en), sizeof(float)}, {offsetof(GrtHostLines, nexp), sizeof(float)},
    {offsetof(GrtHostLines, delta), sizeof(float)}, {offsetof(GrtHostLines, iso), sizeof(uint8_t)}};
enum { NUM_ARRAYS = sizeof(g_arrays)/sizeof(g_arrays[0]) };

/* (the pointers are of different types: read and written as bytes) */
static unsigned char *array_of(GrtHostLines const *l, int a)
{
    unsigned char *p;
    memcpy(&p, (char const *)l + g_arrays[a].at, sizeof(p));
    return p;
}

void grt_free_host_lines(GrtHostLines *l)
{
    for (int a = 0; a < NUM_ARRAYS; ++a) free(array_of(l, a));
    memset(l, 0, sizeof(*l));
}

int grt_reserve_host_lines(GrtHostLines *l, uint64_t cap)
{
    int ok = 1;
    for (int a = 0; a < NUM_ARRAYS; ++a)
    {
        void *p = realloc(array_of(l, a), g_arrays[a].width*cap);
        if (p != NULL) memcpy((char *)l + g_arrays[a].at, &p, sizeof(p)); else ok = 0;
    }
    if (!ok)
    {
        GRT_FAIL(GRTCODE_NULL_ERR, "out of host memory reserving %llu lines.", (unsigned long long)cap);
    }
    return GRTCODE_SUCCESS;
}

void grt_copy_host_line(GrtHostLines *dst, uint64_t j, GrtHostLines const *src, uint64_t k)
{
    for (int a = 0; a < NUM_ARRAYS; ++a)
    {
        size_t const w = g_arrays[a].width;
        memcpy(array_of(dst, a) + w*j, array_of(src, a) + w*k, w);
    }
}

static int fixed_field(char const *rec, int off, int len, char *buf)
{
    memcpy(buf, rec + off, (size_t)len);
    buf[len] = '\0';
    return off + len;
}

/* HITRAN-2012 160-character records (parse_HITRAN_file.c:77-100): mol(2) iso(1) nu(12)
   S(10) A(10) g_air(5) g_self(5) E"(10) n(4) delta(8) + 93 unused.  A record is kept
   when the molecule matches and w0 <= nu <= wn (:340).  Isotopologue codes: '0' -> 10,
   'A'.. -> 11.. (:177-194). */
/* One pass over the file.  mol_id != 0: the reference's behaviour -- keep this molecule's records with
   w0 <= nu <= wn in `out` (one bucket).  mol_id == 0: every molecule's records, unfiltered, into
   out[molecule - 1] (NUM_MOLS buckets; records of unknown molecule numbers are skipped) -- the parse-once
   index below.  Strengths are left as tabulated (296 K). */
static int scan_hitran(char const *path, int mol_id, double w0, double wn, GrtHostLines *out, uint64_t *bad_line)
{
    FILE *fp = NULL;
    GRT_TRY(open_file(&fp, path, "r"));
    uint64_t cap[NUM_MOLS];
    memset(cap, 0, sizeof(cap));
    char *line = NULL;
    size_t linecap = 0;
    ssize_t len;
    size_t lineno = 0;
    int rc = GRTCODE_SUCCESS;
    while ((len = getline(&line, &linecap, fp)) != -1)
    {
        ++lineno;
        if (len > 162 || len < 160)
        {
            grt_err_begin(GRTCODE_VALUE_ERR, __FILE__, __LINE__, "Found bad record at line %zu"
                          " (%zd characters, expected 160-162) in file %s.", lineno, len, path);
            rc = GRTCODE_VALUE_ERR;
            break;
        }
        char buf[16];
        int off = fixed_field(line, 0, 2, buf);
        int mol = 0;
        if ((rc = to_int(buf, &mol)) != GRTCODE_SUCCESS) break;
        if (mol_id != 0 ? mol != mol_id : (mol < 1 || mol > NUM_MOLS))
        {
            continue;
        }
        int const bucket = mol_id != 0 ? 0 : mol - 1;
        GrtHostLines *o = &out[bucket];
        if (o->n == cap[bucket])
        {
            cap[bucket] = cap[bucket] ? 2*cap[bucket] : 65536;
            if ((rc = grt_reserve_host_lines(o, cap[bucket])) != GRTCODE_SUCCESS) break;
        }
        uint64_t const k = o->n;
        /* the record's own fields.  One molecule at a time (the reference's behaviour) a field that does not
           parse is an error; in index mode it is an error only for whoever asks for THAT molecule later
           (parse_HITRAN_file.c:300-313 never looks at the fields of another molecule's records), so the
           record is skipped and its line number remembered */
        int frc = GRTCODE_SUCCESS;
        off = fixed_field(line, off, 1, buf);
        int iso = 0;
        if (buf[0] == '0') iso = 10;
        else if (buf[0] >= 'A' && buf[0] <= 'Z') iso = buf[0] - 'A' + 11;
        else frc = to_int(buf, &iso);
        if (frc == GRTCODE_SUCCESS && (iso < 1 || iso > GRT_MAX_ISO))
        {
            grt_err_begin(GRTCODE_VALUE_ERR, __FILE__, __LINE__, "isotopologue %d on line %zu of %s"
                          " is outside 1-%d.", iso, lineno, path, GRT_MAX_ISO);
            frc = GRTCODE_VALUE_ERR;
        }
        /* nu(12) S(10) A(10, unused) g_air(5) g_self(5) E"(10) n(4) delta(8); the last five are kept as floats
           (parse_HITRAN_file.c:197-212) */
        static int const width[8] = {12, 10, 10, 5, 5, 10, 4, 8};
        double f[8] = {0.};
        for (int c = 0; c < 8 && frc == GRTCODE_SUCCESS; ++c)
        {
            off = fixed_field(line, off, width[c], buf);
            frc = c == 2 ? GRTCODE_SUCCESS : to_double(buf, &f[c]);
        }
        if (frc == GRTCODE_SUCCESS)
        {
            o->iso[k] = (uint8_t)iso; o->v0[k] = f[0]; o->s0[k] = f[1];
            o->yair[k] = (float)f[3]; o->yself[k] = (float)f[4]; o->en[k] = (float)f[5]; o->nexp[k] = (float)f[6];
            o->delta[k] = (float)f[7];
        }
        if (frc == GRTCODE_SUCCESS && !(isfinite(o->v0[k]) && isfinite(o->s0[k])))
        {
            grt_err_begin(GRTCODE_VALUE_ERR, __FILE__, __LINE__, "non-finite line centre or strength on line %zu"
                          " of %s.", lineno, path);
            frc = GRTCODE_VALUE_ERR;
        }
        if (frc != GRTCODE_SUCCESS)
        {
            if (mol_id == 0 && bad_line != NULL)
            {
                if (bad_line[bucket] == 0)
                {
                    bad_line[bucket] = lineno;
                    GRT_WARN("record %zu of %s (molecule %d) does not parse; requests for that molecule will fail.",
                             lineno, path, mol);
                }
                continue;
            }
            rc = frc;
            break;
        }
        if (mol_id == 0 || (w0 < 0 && wn < 0) || (o->v0[k] >= w0 && o->v0[k] <= wn))
        {
            o->n++;
        }
    }
    free(line);
    if (fclose(fp) != 0 && rc == GRTCODE_SUCCESS)
    {
        grt_err_begin(GRTCODE_IO_ERR, __FILE__, __LINE__, "error closing file %s.", path);
        rc = GRTCODE_IO_ERR;
    }
    if (rc != GRTCODE_SUCCESS)
    {
        for (int m = 0; m < (mol_id != 0 ? 1 : NUM_MOLS); ++m)
        {
            grt_free_host_lines(&out[m]);
        }
        grt_err_frame(__FILE__, __LINE__);
    }
    return rc;
}

/* Parse-once index (§8(f)-3).  The reference scans the whole .par file once per add_molecule -- seven
   passes over a few hundred MB for one band, again for the second band.  Here the first request for a
   file parses every molecule's records into memory once; later requests (any molecule, any gas-optics
   object of this process) filter from memory.  Keyed by path, size and modification time; the two most
   recent files are kept.  GRT_HITRAN_CACHE=0 in the environment restores one scan per call;
   GRT_HITRAN_CACHE_DIR=<directory> keeps a binary copy of the index on disk for later processes. */
typedef struct HitranIndex
{
    char path[DIR_PATH_LEN];
    long long size, mtime;
    unsigned long stamp;
    GrtHostLines mol[NUM_MOLS];
    uint64_t bad_line[NUM_MOLS];   /* first record of a molecule the parser refused (0: none): a request for THAT
                                      molecule re-scans the file and fails like the reference; others are served */
} HitranIndex;
static HitranIndex g_hitran_index[2];
static unsigned long g_hitran_stamp = 0;
static long long g_hitran_stats[3];     /* requests served from memory, index files read, .par files scanned */

/* On-disk copy of the index (GRT_HITRAN_CACHE_DIR=<directory> in the environment): one binary file per
   (.par path, size, modification time), the arrays of every molecule as they sit in memory.  A later
   process reads that instead of parsing text: a few hundred MB of %12lf fields become a few reads. */
#define GRT_IDX_MAGIC "GRTIDX02"
typedef struct IndexHeader
{
    char magic[8];
    long long size, mtime;
    uint64_t num_mols, path_hash;
    uint64_t max_iso, record_bytes;    /* GRT_MAX_ISO and the bytes per line of the arrays below: a build with other limits re-parses */
    uint64_t checksum;                 /* FNV-1a over every array, in file order */
    uint64_t n[NUM_MOLS];
    uint64_t bad_line[NUM_MOLS];       /* first record of that molecule the text parser refused (0: none) */
} IndexHeader;

static uint64_t fnv1a(uint64_t h, void const *data, size_t bytes)
{
    unsigned char const *p = data;
    for (size_t i = 0; i < bytes; ++i)
    {
        h = (h ^ p[i])*1099511628211ull;
    }
    return h;
}
#define FNV_BASIS 1469598103934665603ull

static uint64_t path_hash(char const *par)
{
    return fnv1a(FNV_BASIS, par, strlen(par));
}

static int index_file_name(char const *par, long long size, long long mtime, char *out, size_t len)
{
    char const *dir = getenv("GRT_HITRAN_CACHE_DIR");
    if (dir == NULL || dir[0] == '\0')
    {
        return 0;
    }
    int const w = snprintf(out, len, "%s/%016llx_%lld_%lld.grtidx", dir, (unsigned long long)path_hash(par), size, mtime);
    return w > 0 && (size_t)w < len;
}

static uint64_t record_bytes(void)      /* bytes per line, all arrays */
{
    uint64_t b = 0;
    for (int a = 0; a < NUM_ARRAYS; ++a) b += g_arrays[a].width;
    return b;
}

static uint64_t index_checksum(GrtHostLines *mol)
{
    uint64_t h = FNV_BASIS;
    for (int m = 0; m < NUM_MOLS; ++m)
    {
        for (int a = 0; a < NUM_ARRAYS && mol[m].n > 0; ++a)
        {
            h = fnv1a(h, array_of(&mol[m], a), g_arrays[a].width*mol[m].n);
        }
    }
    return h;
}

/* 1 when the index was read from its file; 0 when there is none (or it does not match: the caller scans). */
static int index_read(char const *file, char const *par, long long size, long long mtime, GrtHostLines *mol,
                      uint64_t *bad_line)
{
    FILE *fp = fopen(file, "rb");
    if (fp == NULL)
    {
        return 0;
    }
    IndexHeader h;
    int ok = fread(&h, sizeof(h), 1, fp) == 1 && memcmp(h.magic, GRT_IDX_MAGIC, 8) == 0 && h.size == size
             && h.mtime == mtime && h.num_mols == NUM_MOLS && h.path_hash == path_hash(par)
             && h.max_iso == GRT_MAX_ISO && h.record_bytes == record_bytes();
    for (int m = 0; m < NUM_MOLS && ok; ++m)
    {
        if (h.n[m] == 0)
        {
            continue;
        }
        ok = h.n[m] < ((uint64_t)1 << 40) && grt_reserve_host_lines(&mol[m], h.n[m]) == GRTCODE_SUCCESS;
        for (int a = 0; a < NUM_ARRAYS && ok; ++a)
        {
            ok = fread(array_of(&mol[m], a), g_arrays[a].width, h.n[m], fp) == h.n[m];
        }
        mol[m].n = ok ? h.n[m] : 0;
    }
    ok = ok && fgetc(fp) == EOF;        /* nothing may follow the last array */
    fclose(fp);
    /* the file is trusted no further than the text would be: same bytes as written (checksum), isotopologue codes
       inside the range the kernels index 1/Q with, finite centres and strengths */
    ok = ok && index_checksum(mol) == h.checksum;
    for (int m = 0; m < NUM_MOLS && ok; ++m)
    {
        for (uint64_t k = 0; k < mol[m].n && ok; ++k)
        {
            ok = mol[m].iso[k] >= 1 && mol[m].iso[k] <= GRT_MAX_ISO && isfinite(mol[m].v0[k]) && isfinite(mol[m].s0[k]);
        }
    }
    if (ok) memcpy(bad_line, h.bad_line, sizeof(h.bad_line));
    for (int m = 0; m < NUM_MOLS && !ok; ++m)
    {
        grt_free_host_lines(&mol[m]);
    }
    return ok;
}

/* Best effort: a cache that cannot be written is not an error.  Written under a temporary name and renamed,
   so that a reader never sees half a file. */
static void index_write(char const *file, char const *par, long long size, long long mtime, GrtHostLines *mol,
                        uint64_t const *bad_line)
{
    char tmp[DIR_PATH_LEN + 64];
    if (snprintf(tmp, sizeof(tmp), "%s.%ld.tmp", file, (long)getpid()) >= (int)sizeof(tmp))
    {
        return;
    }
    FILE *fp = fopen(tmp, "wb");
    if (fp == NULL)
    {
        return;
    }
    IndexHeader h;
    memset(&h, 0, sizeof(h));
    memcpy(h.magic, GRT_IDX_MAGIC, 8);
    h.size = size; h.mtime = mtime; h.num_mols = NUM_MOLS; h.path_hash = path_hash(par);
    h.max_iso = GRT_MAX_ISO; h.record_bytes = record_bytes();
    h.checksum = index_checksum(mol);
    for (int m = 0; m < NUM_MOLS; ++m)
    {
        h.n[m] = mol[m].n;
        h.bad_line[m] = bad_line[m];
    }
    int ok = fwrite(&h, sizeof(h), 1, fp) == 1;
    for (int m = 0; m < NUM_MOLS && ok; ++m)
    {
        for (int a = 0; a < NUM_ARRAYS && ok && mol[m].n > 0; ++a)
        {
            ok = fwrite(array_of(&mol[m], a), g_arrays[a].width, mol[m].n, fp) == mol[m].n;
        }
    }
    ok = (fclose(fp) == 0) && ok;
    if (!ok || rename(tmp, file) != 0)
    {
        remove(tmp);
    }
}

static int hitran_index(char const *path, HitranIndex **out)
{
    struct stat st;
    if (stat(path, &st) != 0)
    {
        GRT_FAIL(GRTCODE_IO_ERR, "failed to open file %s.", path);
    }
    long long const mtime = (long long)st.st_mtim.tv_sec*1000000000ll + st.st_mtim.tv_nsec;
    HitranIndex *victim = &g_hitran_index[0];
    for (int i = 0; i < 2; ++i)
    {
        HitranIndex *h = &g_hitran_index[i];
        if (h->stamp != 0 && strcmp(h->path, path) == 0 && h->size == (long long)st.st_size && h->mtime == mtime)
        {
            h->stamp = ++g_hitran_stamp;
            g_hitran_stats[0]++;
            *out = h;
            return GRTCODE_SUCCESS;
        }
        if (h->stamp < victim->stamp)
        {
            victim = h;
        }
    }
    for (int m = 0; m < NUM_MOLS; ++m)
    {
        grt_free_host_lines(&victim->mol[m]);
    }
    victim->stamp = 0;
    char file[DIR_PATH_LEN + 64];
    int const on_disk = index_file_name(path, (long long)st.st_size, mtime, file, sizeof(file));
    memset(victim->bad_line, 0, sizeof(victim->bad_line));
    if (on_disk && index_read(file, path, (long long)st.st_size, mtime, victim->mol, victim->bad_line))
    {
        GRT_INFO("Read the index of %s from %s.", path, file);
        g_hitran_stats[1]++;
    }
    else
    {
        GRT_INFO("Indexing HITRAN line parameters of every molecule in %s.", path);
        GRT_TRY(scan_hitran(path, 0, 0., 0., victim->mol, victim->bad_line));
        g_hitran_stats[2]++;
        if (on_disk)
        {
            index_write(file, path, (long long)st.st_size, mtime, victim->mol, victim->bad_line);
        }
    }
    GRT_TRY(copy_str(victim->path, path, DIR_PATH_LEN));
    victim->size = (long long)st.st_size;
    victim->mtime = mtime;
    victim->stamp = ++g_hitran_stamp;
    *out = victim;
    return GRTCODE_SUCCESS;
}

/* {requests served from the in-memory index, index files read, .par files scanned for the index} since the
   library was loaded (grt_ext.h) */
EXTERN int grt_hitran_index_stats(long long stats[3])
{
    GRT_REQUIRE_PTR(stats);
    memcpy(stats, g_hitran_stats, sizeof(g_hitran_stats));
    return GRTCODE_SUCCESS;
}

int grt_parse_hitran(char const *path, int mol_id, double w0, double wn, GrtHostLines *out)
{
    GRT_REQUIRE_PTR(path);
    GRT_REQUIRE_PTR(out);
    memset(out, 0, sizeof(*out));
    char const *env = getenv("GRT_HITRAN_CACHE");
    if (mol_id < 1 || mol_id > NUM_MOLS || (env != NULL && env[0] == '0'))
    {
        GRT_INFO("Reading HITRAN line parameters for molecule %d from %s.", mol_id, path);
        GRT_TRY(scan_hitran(path, mol_id, w0, wn, out, NULL));
    }
    else
    {
        HitranIndex *idx = NULL;
        GRT_TRY(hitran_index(path, &idx));
        if (idx->bad_line[mol_id - 1] != 0)
        {
            /* this molecule has a record the parser refused: scan for it alone, which fails there as the reference does */
            GRT_TRY(scan_hitran(path, mol_id, w0, wn, out, NULL));
            return GRTCODE_SUCCESS;
        }
        GrtHostLines const *src = &idx->mol[mol_id - 1];
        if (src->n > 0)
        {
            GRT_TRY(grt_reserve_host_lines(out, src->n));
        }
        for (uint64_t k = 0; k < src->n; ++k)
        {
            if ((w0 < 0 && wn < 0) || (src->v0[k] >= w0 && src->v0[k] <= wn))      /* parse_HITRAN_file.c:340 */
            {
                grt_copy_host_line(out, out->n++, src, k);
            }
        }
    }
    return GRTCODE_SUCCESS;      /* strengths as tabulated: see grt_rescale_strengths */
}
