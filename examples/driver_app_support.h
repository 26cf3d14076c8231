/* driver_app_support.h -- what the two applications of the reference's framework/src/driver.h share (driver_app.c,
 * driver_app_dump.c): the text flux file behind create_flux_file / write_output / close_flux_file, destroy_atmosphere,
 * the CIA pairs and the continuum arguments.  For the ONE .c file of an application, which defines APP_NAME (the prefix
 * of its error messages) before including it: write_output, close_flux_file and destroy_atmosphere below ARE the
 * callbacks driver.h declares, so they have external linkage; everything else is static inline.
 */
#ifndef GRT_DRIVER_APP_SUPPORT_H
#define GRT_DRIVER_APP_SUPPORT_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "driver.h"
#include "gas_optics.h"
#include "grtcode_utilities.h"
#include "example_support.h"

static inline void die(char const *what, char const *arg)
{
    fprintf(stderr, APP_NAME ": %s%s\n", what, arg ? arg : "");
    exit(EXIT_FAILURE);
}

/* ---- the text flux file: one line per write_output call, "<time> <column> <variable name> <count> v0 v1 ..." ------ */
struct Output
{
    FILE *file;
    int integrated, num_levels, column_offset;      /* column_offset: global index of the first column of this run */
    uint64_t n_lw, n_sw;
};

/* create_flux_file for an application whose columns start at column_offset; suffix ends the header line's bracket */
static inline void open_flux_file(Output_t **output, char const *path, Atmosphere_t const *atm, SpectralGrid_t const *lw_grid,
                                  SpectralGrid_t const *sw_grid, int integrated, int column_offset, char const *suffix)
{
    Output_t *o = malloc(sizeof(*o));
    o->file = fopen(path, "w");
    if (o->file == NULL)
    {
        die("cannot create output file ", path);
    }
    o->integrated = integrated;
    o->num_levels = atm->num_levels;
    o->column_offset = column_offset;
    o->n_lw = lw_grid->n;
    o->n_sw = sw_grid->n;
    fprintf(o->file, "# time column variable count values  (lw grid %g-%g @%g, sw grid %g-%g @%g, %s%s)\n",
            lw_grid->w0, lw_grid->wn, lw_grid->dw, sw_grid->w0, sw_grid->wn, sw_grid->dw,
            integrated ? "integrated [W m-2]" : "spectral [W m-2 cm]", suffix);
    *output = o;
}

static inline char const *variable_name(Variables_t id)
{
    switch (id)
    {
        case RLUTCSAF: return "rlutcsaf";
        case RLUSCSAF: return "rluscsaf";
        case RLDSCSAF: return "rldscsaf";
        case RLUCSAF_USER_LEVEL: return "rlucsaf_user_level";
        case RLDCSAF_USER_LEVEL: return "rldcsaf_user_level";
        case RSUTCSAF: return "rsutcsaf";
        case RSUSCSAF: return "rsuscsaf";
        case RSDTCSAF: return "rsdtcsaf";
        case RSDSCSAF: return "rsdscsaf";
        case RSUCSAF_USER_LEVEL: return "rsucsaf_user_level";
        case RSDCSAF_USER_LEVEL: return "rsdcsaf_user_level";
        /* the all-sky and aerosol passes: the driver writes these only for an atmosphere that is not clear / not clean */
        case RLUTAF: return "rlutaf";
        case RLUSAF: return "rlusaf";
        case RLDSAF: return "rldsaf";
        case RLUAF_USER_LEVEL: return "rluaf_user_level";
        case RLDAF_USER_LEVEL: return "rldaf_user_level";
        case RSUTAF: return "rsutaf";
        case RSUSAF: return "rsusaf";
        case RSDTAF: return "rsdtaf";
        case RSDSAF: return "rsdsaf";
        case RSUAF_USER_LEVEL: return "rsuaf_user_level";
        case RSDAF_USER_LEVEL: return "rsdaf_user_level";
        case RLUTCS: return "rlutcs";
        case RLUSCS: return "rluscs";
        case RLDSCS: return "rldscs";
        case RLUCS_USER_LEVEL: return "rlucs_user_level";
        case RLDCS_USER_LEVEL: return "rldcs_user_level";
        case RSUTCS: return "rsutcs";
        case RSUSCS: return "rsuscs";
        case RSDTCS: return "rsdtcs";
        case RSDSCS: return "rsdscs";
        case RSUCS_USER_LEVEL: return "rsucs_user_level";
        case RSDCS_USER_LEVEL: return "rsdcs_user_level";
        case LEVEL_PRESSURE: return "level_pressure";
        case LEVEL_TEMPERATURE: return "level_temperature";
        case LAYER_TEMPERATURE: return "layer_temperature";
        case SURFACE_TEMPERATURE: return "surface_temperature";
        case H2O_VMR: return "h2o_vmr";
        default: return NULL;      /* variables these applications do not keep */
    }
}

void write_output(Output_t *output, Variables_t id, fp_t const *data, int time, int column)
{
    char const *name = variable_name(id);
    if (name == NULL || data == NULL)
    {
        return;
    }
    size_t count = 1;
    if (is_longwave_flux(id))
    {
        count = output->integrated ? 1 : output->n_lw;
    }
    else if (is_shortwave_flux(id))
    {
        count = output->integrated ? 1 : output->n_sw;
    }
    else if (id == LEVEL_PRESSURE || id == LEVEL_TEMPERATURE || id == H2O_VMR)
    {
        count = (size_t)output->num_levels;
    }
    else if (id == LAYER_TEMPERATURE)
    {
        count = (size_t)output->num_levels - 1;
    }
    fprintf(output->file, "%d %d %s %zu", time, output->column_offset + column, name, count);
    for (size_t i = 0; i < count; ++i)
    {
        fprintf(output->file, " %.17g", data[i]);
    }
    fprintf(output->file, "\n");
}

void close_flux_file(Output_t * const output)
{
    fclose(output->file);
    free(output);
}

void destroy_atmosphere(Atmosphere_t *atm)
{
    free(atm->level_pressure); free(atm->level_temperature); free(atm->layer_pressure);
    free(atm->layer_temperature); free(atm->surface_temperature); free(atm->solar_zenith_angle);
    free(atm->total_solar_irradiance); free(atm->albedo_grid); free(atm->surface_albedo);
    free(atm->emissivity_grid); free(atm->surface_emissivity);
    free(atm->cloud_fraction); free(atm->liquid_water_content); free(atm->ice_water_content); free(atm->layer_thickness);
    for (int i = 0; i < atm->num_molecules; ++i) free(atm->ppmv[i]);
    for (int i = 0; i < atm->num_cfcs; ++i) free(atm->cfc_ppmv[i]);
    for (int i = 0; i < atm->num_cia_species; ++i) free(atm->cia_ppmv[i]);
    free(atm->molecules); free(atm->ppmv); free(atm->cfc); free(atm->cfc_ppmv);
    free(atm->cia); free(atm->cia_species); free(atm->cia_ppmv);
    memset(atm, 0, sizeof(*atm));
}

/* ---- command-line pieces ------------------------------------------------------------------------------------------ */
/* the CIA pairs asked for and the abundance of each species they involve: ppmv_of(species) is that species' malloc'd
 * ppmv array over every (time, column, level) of the atmosphere */
static inline void add_cias(Parser_t *parser, Atmosphere_t *atm, fp_t *(*ppmv_of)(int species, void *ctx), void *ctx)
{
    atm->cia = malloc(sizeof(Cia_t)*3);
    atm->cia_species = malloc(sizeof(int)*2);
    atm->cia_ppmv = malloc(sizeof(fp_t *)*2);
    atm->num_cias = atm->num_cia_species = 0;
    for (int i = 0; i < 3; ++i)
    {
        Cia_t *c = &atm->cia[atm->num_cias];
        if (!get_argument(*parser, cia_flags[i].flag, c->path))
        {
            continue;
        }
        c->id[0] = cia_flags[i].s1;
        c->id[1] = cia_flags[i].s2;
        for (int j = 0; j < 2; ++j)
        {
            int k = 0;
            while (k < atm->num_cia_species && atm->cia_species[k] != c->id[j]) ++k;
            if (k == atm->num_cia_species)
            {
                atm->cia_species[k] = c->id[j];
                atm->cia_ppmv[k] = ppmv_of(c->id[j], ctx);
                atm->num_cia_species++;
            }
        }
        atm->num_cias++;
    }
}

static inline void continua(Parser_t *parser, Atmosphere_t *atm)
{
    if (!get_argument(*parser, "-h2o-ctm", atm->h2o_ctm))
    {
        snprintf(atm->h2o_ctm, valuelen, "%s", "none");
    }
    if (!get_argument(*parser, "-o3-ctm", atm->o3_ctm))
    {
        snprintf(atm->o3_ctm, valuelen, "%s", "none");
    }
}

#endif
