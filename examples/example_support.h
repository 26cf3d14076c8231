/* example_support.h -- what the example callers share and that needs only this repository's include/: error checking,
 * command-line look-up, the flag tables, the column text format and the layer-to-level interpolation.  Static inline
 * functions and constant tables only, so every example still compiles from its one .c file.
 */
#ifndef GRT_EXAMPLE_SUPPORT_H
#define GRT_EXAMPLE_SUPPORT_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gas_optics.h"
#include "grtcode_utilities.h"

#define MAXV 201
#define NSPEC 9

#define check(call) { int rc_ = (call); if (rc_ != GRTCODE_SUCCESS) { char b_[4096]; \
    grtcode_errstr(rc_, b_, 4096); fprintf(stderr, "[%s:%d] %s\n", __FILE__, __LINE__, b_); return EXIT_FAILURE; } }

/* The argument `skip` places after the first `name` on the command line (0: the flag itself, 1: its value,
 * 2: the second value of "-CFC-11 FILE ppmv"); NULL if the flag is absent or the line ends before that place. */
static inline char const *option(int argc, char **argv, char const *name, int skip)
{
    for (int i = 1; i + skip < argc; ++i)
    {
        if (strcmp(argv[i], name) == 0)
        {
            return argv[i + skip];
        }
    }
    return NULL;
}

static inline fp_t number(int argc, char **argv, char const *name, fp_t fallback)
{
    char const *v = option(argc, argv, name, 1);
    return v != NULL ? atof(v) : fallback;
}

/* layer abundances of the column text format, in this order; the first seven are line-by-line molecules */
static char const *const species[NSPEC] = {"H2O", "CO2", "O3", "N2O", "CO", "CH4", "O2", "CFC11", "CFC12"};
static int const hitran_id[7] = {H2O, CO2, O3, N2O, CO, CH4, O2};

typedef struct CfcFlag { int id; char *flag; int spec; } CfcFlag;      /* spec: its place in species[] */
static CfcFlag const cfc_flags[2] = {{CFC11, "-CFC-11", 7}, {CFC12, "-CFC-12", 8}};

typedef struct CiaFlag { int s1, s2; char *flag; } CiaFlag;
static CiaFlag const cia_flags[3] = {{CIA_N2, CIA_N2, "-N2-N2"}, {CIA_O2, CIA_N2, "-O2-N2"}, {CIA_O2, CIA_O2, "-O2-O2"}};

/* ---- the column text format: lines "name: v0 v1 ...", a line "column:" opens the next column ---------------------- */
typedef struct Column
{
    int num_levels;
    fp_t level_pressure[MAXV], level_temperature[MAXV], layer_pressure[MAXV], layer_temperature[MAXV];
    fp_t surface_temperature, solar_zenith_angle, toa_solar_irradiance;
    fp_t abundance[NSPEC][MAXV];                                            /* layer mole fractions, by species[] */
    fp_t cloud_fraction[MAXV], liquid_water_content[MAXV], ice_water_content[MAXV];     /* optional, zero when absent */
} Column_t;

static inline int read_values(char *text, fp_t *dst, int max)
{
    int n = 0;
    for (char *tok = strtok(text, " \t\r\n"); tok != NULL && n < max; tok = strtok(NULL, " \t\r\n"))
    {
        dst[n++] = atof(tok);
    }
    return n;
}

/* Reads the file's columns into *cols (malloc'd) and returns how many, or -1 if the file cannot be opened.  With
 * `fold`, "column:" lines are ignored and all blocks fall into ONE column in file order, a later block's field
 * overwriting an earlier one's -- what a single-column caller makes of a file with several blocks. */
static inline int read_columns(char const *path, int fold, Column_t **cols)
{
    *cols = NULL;
    FILE *f = fopen(path, "r");
    if (f == NULL)
    {
        return -1;
    }
    int n = 0;
    static char line[1 << 16];
    while (fgets(line, sizeof(line), f) != NULL)
    {
        char *colon = strchr(line, ':');
        if (colon == NULL)
        {
            continue;
        }
        *colon = '\0';
        char *vals = colon + 1;
        int const opens = !fold && strcmp(line, "column") == 0;
        if (opens || n == 0)
        {
            *cols = realloc(*cols, sizeof(**cols)*(size_t)(n + 1));
            memset(&(*cols)[n], 0, sizeof(**cols));
            ++n;
            if (opens)
            {
                continue;
            }
        }
        Column_t *c = &(*cols)[n - 1];
        if (strcmp(line, "level_pressure") == 0) c->num_levels = read_values(vals, c->level_pressure, MAXV);
        else if (strcmp(line, "level_temperature") == 0) read_values(vals, c->level_temperature, MAXV);
        else if (strcmp(line, "layer_pressure") == 0) read_values(vals, c->layer_pressure, MAXV);
        else if (strcmp(line, "layer_temperature") == 0) read_values(vals, c->layer_temperature, MAXV);
        else if (strcmp(line, "surface_temperature") == 0) read_values(vals, &c->surface_temperature, 1);
        else if (strcmp(line, "solar_zenith_angle") == 0) read_values(vals, &c->solar_zenith_angle, 1);
        else if (strcmp(line, "toa_solar_irradiance") == 0) read_values(vals, &c->toa_solar_irradiance, 1);
        else if (strcmp(line, "cloud_fraction") == 0) read_values(vals, c->cloud_fraction, MAXV);
        else if (strcmp(line, "liquid_water_content") == 0) read_values(vals, c->liquid_water_content, MAXV);
        else if (strcmp(line, "ice_water_content") == 0) read_values(vals, c->ice_water_content, MAXV);
        else
        {
            for (int k = 0; k < NSPEC; ++k)
            {
                if (strcmp(line, species[k]) == 0) read_values(vals, c->abundance[k], MAXV);
            }
        }
    }
    fclose(f);
    return n;
}

/* Layer mole fractions -> ppmv on the levels by interpolation in pressure, end levels copied.  The reference has it
 * twice, as (sum)*1e6 in a statement of its own (circ/src/basic-circ-test.c:51-66) and as 1e6*(sum) in one expression
 * (rfmip-irf/src/rfmip-irf.c:295-308).  The sum ends in a division, so nothing can be contracted into it, and it is
 * rounded to a double either way where double expressions are evaluated in double (FLT_EVAL_METHOD 0, as on x86-64);
 * an IEEE product does not depend on the order of its factors.  So the two give the same bits, and this is both. */
static inline void layers_to_levels(fp_t *ppmv, fp_t const *abundance, int num_layers, fp_t const *layer_pressure,
                                    fp_t const *level_pressure)
{
    fp_t const to_ppmv = 1.e6;
    ppmv[0] = abundance[0]*to_ppmv;
    ppmv[num_layers] = abundance[num_layers - 1]*to_ppmv;
    for (int k = 1; k < num_layers; ++k)
    {
        ppmv[k] = to_ppmv*(abundance[k - 1] + (abundance[k] - abundance[k - 1])*
                  (level_pressure[k] - layer_pressure[k - 1])/(layer_pressure[k] - layer_pressure[k - 1]));
    }
}

#endif
