/* driver_app.c -- a netCDF-free application object for the reference's framework/src/driver.c.
 *
 * framework/src/driver.c holds main(), the command line, the column loop and the flux output of every
 * GRTCODE application; an application supplies five callbacks (framework/src/driver.h:165-203):
 * create_atmosphere, destroy_atmosphere, create_flux_file, write_output, close_flux_file.  The reference's
 * own applications (rfmip-irf.c, era5.c, circ.c) implement them on netCDF, which this image does not have.
 * This file implements them on flat text, so that the UNCHANGED driver.c -- compiled where it lies, linked
 * with the reference's own argparse.c and this library -- runs clear-sky columns end to end:
 *
 *   grtcode_driver HITRAN.par SOLAR.csv COLUMNS.txt [-H2O -CO2 -O3 -N2O -CO -CH4 -O2]
 *       [-h2o-ctm DIR] [-o3-ctm FILE] [-CFC-11 FILE] [-CFC-12 FILE] [-N2-N2 FILE] [-O2-N2 FILE] [-O2-O2 FILE]
 *       [-a ALBEDO] [-e EMISSIVITY] [-x FIRST] [-X LAST] [-aerosols] [-clouds]
 *       + driver.c's own options (-d, -r-lw, -r-sw, -w-lw, -W-lw, -w-sw, -W-sw, -integrated, -flux-at-level, -o, -v)
 *
 * COLUMNS.txt: one or more columns, each a block of lines "name: v0 v1 ..." opened by a line "column:" --
 *   level_pressure [mb], level_temperature [K], layer_pressure [mb], layer_temperature [K],
 *   surface_temperature [K], solar_zenith_angle [deg], toa_solar_irradiance [W m-2 on a horizontal surface],
 *   layer abundances (mole fraction) H2O CO2 O3 N2O CO CH4 O2 CFC11 CFC12.
 * Column semantics are those of circ/src/basic-circ-test.c: level abundances pressure-interpolated from the
 * layer values (:51-66), cos(zenith) (:118-120), irradiance divided by it (:122-124), two-point constant
 * albedo / emissivity grids (:127-137, :147-153; emissivity 1 unless -e), N2 at 0.781 for the CIA pairs (:270-277).
 * -clouds makes the driver run its cloud pass too (driver.c:474-597: clear = 0) with the optional per-layer fields
 *   cloud_fraction, liquid_water_content [g m-3], ice_water_content [g m-3] of the column file (zero when absent) and
 *   layer thicknesses from the hydrostatic relation of basic-circ-test.c:155-166.  That pass calls a clouds library
 *   (clouds/clouds_lib.h) -- libclouds.a of THIS repository only stops the run; link the reference's, or any object with
 *   those four functions -- and fills Optics_t arrays in place on the host: run with GRT_OPTICS_HOST_VISIBLE=1.
 * -aerosols makes the driver also run its aerosol pass (driver.c:426-472: clean = 0), whose optics the reference itself
 * leaves at zero -- the body of calculate_aerosol_optics is commented out (driver.c:223-238) -- so the "clear-sky" fluxes
 * it writes (rlutcs, ...) equal the "clear-clean-sky" ones (rlutcsaf, ...): the pass is plumbing, exercised as such.
 *
 * Output (-o PATH, default output.nc as driver.c names it -- but text): one line per write_output call,
 *   "<time> <column> <variable name> <count> v0 v1 ...", fluxes in W m-2 (or W m-2 cm with spectral output).
 *
 * create_atmosphere and create_flux_file are here; write_output, close_flux_file, destroy_atmosphere and the text flux
 * file are examples/driver_app_support.h, the column reader and the interpolation examples/example_support.h.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#define APP_NAME "driver_app"
#include "driver_app_support.h"

static Column_t *read_usable_columns(char const *path, int *count)
{
    Column_t *cols;
    int const n = read_columns(path, 0, &cols);
    if (n < 0)
    {
        die("cannot open column file ", path);
    }
    if (n == 0 || cols[0].num_levels < 2)
    {
        die("no usable column in ", path);
    }
    for (int i = 1; i < n; ++i)
    {
        if (cols[i].num_levels != cols[0].num_levels)
        {
            die("columns with different numbers of levels in ", path);
        }
    }
    *count = n;
    return cols;
}

/* the abundance of a CIA species on the levels of the selected columns: N2 constant, O2 from the column file */
typedef struct CiaCtx { Column_t const *cols; Atmosphere_t const *atm; } CiaCtx;

static fp_t *cia_ppmv_of(int species, void *ctx)
{
    CiaCtx const *x = ctx;
    Atmosphere_t const *atm = x->atm;
    size_t const C = (size_t)atm->num_columns, V = (size_t)atm->num_levels, L = (size_t)atm->num_layers;
    fp_t *ppmv = malloc(sizeof(fp_t)*C*V);
    for (size_t c = 0; c < C; ++c)
    {
        if (species == CIA_N2)
        {
            for (size_t l = 0; l < V; ++l) ppmv[c*V + l] = 0.781*1.e6;       /* basic-circ-test.c:272-275 */
        }
        else
        {
            layers_to_levels(ppmv + c*V, x->cols[atm->x + (int)c].abundance[6], atm->num_layers,
                             atm->layer_pressure + c*L, atm->level_pressure + c*V);
        }
    }
    return ppmv;
}

Atmosphere_t create_atmosphere(Parser_t * const parser)
{
    snprintf(parser->description, desclen, "Clear-sky line-by-line fluxes for columns read from a flat text file.");
    add_argument(parser, "column_file", NULL, "Text file with one or more columns.", NULL);
    int one = 1;
    add_argument(parser, "-a", "--surface-albedo", "Spectrally constant surface albedo.", &one);
    add_argument(parser, "-e", "--surface-emissivity", "Spectrally constant surface emissivity.", &one);
    add_argument(parser, "-CFC-11", NULL, "CSV file with CFC-11 cross sections.", &one);
    add_argument(parser, "-CFC-12", NULL, "CSV file with CFC-12 cross sections.", &one);
    add_argument(parser, "-CH4", NULL, "Include CH4.", NULL);
    add_argument(parser, "-CO", NULL, "Include CO.", NULL);
    add_argument(parser, "-CO2", NULL, "Include CO2.", NULL);
    add_argument(parser, "-H2O", NULL, "Include H2O.", NULL);
    add_argument(parser, "-h2o-ctm", NULL, "Directory containing H2O continuum files", &one);
    add_argument(parser, "-N2-N2", NULL, "CSV file with N2-N2 collison cross sections", &one);
    add_argument(parser, "-N2O", NULL, "Include N2O.", NULL);
    add_argument(parser, "-O2", NULL, "Include O2.", NULL);
    add_argument(parser, "-O2-N2", NULL, "CSV file with O2-N2 collison cross sections", &one);
    add_argument(parser, "-O2-O2", NULL, "CSV file with O2-O2 collison cross sections", &one);
    add_argument(parser, "-O3", NULL, "Include O3.", NULL);
    add_argument(parser, "-o3-ctm", NULL, "Ozone continuum file", &one);
    add_argument(parser, "-x", "--column-lower-bound", "Starting column index.", &one);
    add_argument(parser, "-X", "--column-upper-bound", "Ending column index.", &one);
    add_argument(parser, "-aerosols", NULL, "Also run the driver's aerosol pass (with the reference's zero aerosol optics).", NULL);
    add_argument(parser, "-clouds", NULL, "Also run the driver's cloud pass (needs a clouds library and GRT_OPTICS_HOST_VISIBLE=1).", NULL);
    parse_args(*parser);

    char buffer[valuelen];
    get_argument(*parser, "column_file", buffer);
    int total = 0;
    Column_t *cols = read_usable_columns(buffer, &total);
    int const x = get_argument(*parser, "-x", buffer) ? atoi(buffer) : 0;
    int const X = get_argument(*parser, "-X", buffer) ? atoi(buffer) : total - 1;
    if (x < 0 || X >= total || X < x)
    {
        die("column range -x/-X outside the file", NULL);
    }

    Atmosphere_t atm;
    memset(&atm, 0, sizeof(atm));
    atm.x = x;
    atm.X = X;
    atm.num_columns = X - x + 1;
    atm.num_times = 1;
    atm.num_levels = cols[0].num_levels;
    atm.num_layers = atm.num_levels - 1;
    atm.clean = get_argument(*parser, "-aerosols", NULL) ? 0 : 1;
    atm.clear = get_argument(*parser, "-clouds", NULL) ? 0 : 1;
    size_t const C = (size_t)atm.num_columns, V = (size_t)atm.num_levels, L = (size_t)atm.num_layers;
    atm.level_pressure = malloc(sizeof(fp_t)*C*V);
    atm.level_temperature = malloc(sizeof(fp_t)*C*V);
    atm.layer_pressure = malloc(sizeof(fp_t)*C*L);
    atm.layer_temperature = malloc(sizeof(fp_t)*C*L);
    atm.surface_temperature = malloc(sizeof(fp_t)*C);
    atm.solar_zenith_angle = malloc(sizeof(fp_t)*C);
    atm.total_solar_irradiance = malloc(sizeof(fp_t)*C);
    fp_t const albedo = get_argument(*parser, "-a", buffer) ? atof(buffer) : 0.2;
    fp_t const emissivity = get_argument(*parser, "-e", buffer) ? atof(buffer) : 1.;
    atm.albedo_grid_size = 2;
    atm.albedo_grid = malloc(sizeof(fp_t)*2);
    atm.albedo_grid[0] = -1.;
    atm.albedo_grid[1] = 0.;
    atm.surface_albedo = malloc(sizeof(fp_t)*2*C);
    atm.emissivity_grid_size = 2;
    atm.emissivity_grid = malloc(sizeof(fp_t)*2);
    atm.emissivity_grid[0] = -1.;
    atm.emissivity_grid[1] = 0.;
    atm.surface_emissivity = malloc(sizeof(fp_t)*2*C);
    if (!atm.clear)
    {
        atm.cloud_fraction = malloc(sizeof(fp_t)*C*L);
        atm.liquid_water_content = malloc(sizeof(fp_t)*C*L);
        atm.ice_water_content = malloc(sizeof(fp_t)*C*L);
        atm.layer_thickness = malloc(sizeof(fp_t)*C*L);
        for (size_t c = 0; c < C; ++c)
        {
            Column_t const *col = &cols[x + (int)c];
            memcpy(atm.cloud_fraction + c*L, col->cloud_fraction, sizeof(fp_t)*L);
            memcpy(atm.liquid_water_content + c*L, col->liquid_water_content, sizeof(fp_t)*L);
            memcpy(atm.ice_water_content + c*L, col->ice_water_content, sizeof(fp_t)*L);
            for (size_t i = 0; i < L; ++i)
            {
                /* basic-circ-test.c:155-166 */
                fp_t const gas_constant = 8.314462, gravity = 9.81, kg_per_g = .001, molar_mass = 28.9647;
                atm.layer_thickness[c*L + i] = (fabs(log(col->level_pressure[i]) - log(col->level_pressure[i + 1]))*
                                               col->layer_temperature[i]*gas_constant)/(molar_mass*kg_per_g*gravity);
            }
        }
    }
    for (size_t c = 0; c < C; ++c)
    {
        Column_t const *col = &cols[x + (int)c];
        memcpy(atm.level_pressure + c*V, col->level_pressure, sizeof(fp_t)*V);
        memcpy(atm.level_temperature + c*V, col->level_temperature, sizeof(fp_t)*V);
        memcpy(atm.layer_pressure + c*L, col->layer_pressure, sizeof(fp_t)*L);
        memcpy(atm.layer_temperature + c*L, col->layer_temperature, sizeof(fp_t)*L);
        atm.surface_temperature[c] = col->surface_temperature;
        atm.solar_zenith_angle[c] = (fp_t)cos(2.*M_PI*col->solar_zenith_angle/360.);
        atm.total_solar_irradiance[c] = col->toa_solar_irradiance/atm.solar_zenith_angle[c];
        atm.surface_albedo[2*c] = atm.surface_albedo[2*c + 1] = albedo;
        atm.surface_emissivity[2*c] = atm.surface_emissivity[2*c + 1] = emissivity;
    }

    /* molecules, in the order of basic-circ-test.c:177-185 */
    static struct { int id; char const *flag; int spec; } const mols[7] = {
        {CH4, "-CH4", 5}, {CO, "-CO", 4}, {CO2, "-CO2", 1}, {H2O, "-H2O", 0}, {N2O, "-N2O", 3}, {O2, "-O2", 6}, {O3, "-O3", 2}};
    atm.molecules = malloc(sizeof(int)*7);
    atm.ppmv = malloc(sizeof(fp_t *)*7);
    for (int i = 0; i < 7; ++i)
    {
        if (get_argument(*parser, (char *)mols[i].flag, NULL))
        {
            atm.molecules[atm.num_molecules] = mols[i].id;
            fp_t *ppmv = atm.ppmv[atm.num_molecules] = malloc(sizeof(fp_t)*C*V);
            for (size_t c = 0; c < C; ++c)
            {
                layers_to_levels(ppmv + c*V, cols[x + (int)c].abundance[mols[i].spec], atm.num_layers,
                                 atm.layer_pressure + c*L, atm.level_pressure + c*V);
            }
            atm.num_molecules++;
        }
    }
    continua(parser, &atm);
    atm.cfc = malloc(sizeof(Cfc_t)*2);
    atm.cfc_ppmv = malloc(sizeof(fp_t *)*2);
    for (int i = 0; i < 2; ++i)
    {
        if (get_argument(*parser, cfc_flags[i].flag, atm.cfc[atm.num_cfcs].path))
        {
            atm.cfc[atm.num_cfcs].id = cfc_flags[i].id;
            fp_t *ppmv = atm.cfc_ppmv[atm.num_cfcs] = malloc(sizeof(fp_t)*C*V);
            for (size_t c = 0; c < C; ++c)
            {
                layers_to_levels(ppmv + c*V, cols[x + (int)c].abundance[cfc_flags[i].spec], atm.num_layers,
                                 atm.layer_pressure + c*L, atm.level_pressure + c*V);
            }
            atm.num_cfcs++;
        }
    }
    CiaCtx ctx = {cols, &atm};
    add_cias(parser, &atm, cia_ppmv_of, &ctx);
    free(cols);
    return atm;
}

void create_flux_file(Output_t **output, char const * const path, Atmosphere_t const * const atm,
                      SpectralGrid_t const * const lw_grid, SpectralGrid_t const * const sw_grid,
                      int const user_level, int const integrated)
{
    (void)user_level;
    open_flux_file(output, path, atm, lw_grid, sw_grid, integrated, 0, "");
}
