/* clouds_lib.h -- entry points of the cloud-optics library as framework/src/driver.c calls them
 * (clouds/clouds_lib.h; driver.c:181, 507, 667, 759), implemented in libclouds.a of this repository
 * (grtcode_amd/csrc/host/grt_clouds.c: host C99, like the reference's clouds/): Pade cloud optics per band, stochastic
 * sampling of the condensate from a beta-distributed total water with maximum-random overlap (libc rand(), the same
 * draws in the same order), band-to-grid mapping.
 *
 * Parameter files: the reference's three netCDF files (-beta-path, -ice-path, -liquid-path) as GRTDUMP1 flat files with
 * the same variable names (scripts/netcdf_to_dump.py converts them on a box that has netCDF4).  The driver's cloud pass
 * fills Optics_t arrays in place on the host (driver.c:507-525): run it with GRT_OPTICS_HOST_VISIBLE=1 so that
 * create_optics hands out host-visible memory.  GRT_CLOUDS_SEED=<n> makes initialize_clouds_lib call
 * srand(n) (the reference never seeds).
 */
#ifndef CLOUDS_LIB_H
#define CLOUDS_LIB_H

int initialize_clouds_lib(char const *beta_path, char const *ice_path, char const *liquid_path);
int finalize_clouds_lib();
int cloud_optics(const double *wavenum, int num_wavenum, int num_layers, const double *mean_cloud_fraction,
                 const double *mean_liquid_content, const double *mean_ice_content, const double *overlap,
                 const double liquid_radius, const double *temperature, double *beta_liquid, double *omega_liquid,
                 double *g_liquid, double *beta_ice, double *omega_ice, double *g_ice);
int calculate_overlap(int const num_layers, double const *altitude, double const scale_length, double *alpha);

/* Test hooks (not part of the reference's interface): one subcolumn's condensate exactly as cloud_optics draws it per band
   (clouds/stochastic_clouds.c:94-120), and a look-up in the loaded incomplete-beta tables.  tests/test_clouds_library.py
   compares the first with the reference's own stochastic_clouds.c (oracle/_ref/libstochastic_ref.so), which gets its
   beta_inverse / beta_value from the second (tests/support/beta_bridge.c) -- the reference's incomplete_beta.c needs netCDF. */
int grt_clouds_sample_subcolumn(int num_layers, const double *cloud_fraction, const double *lwc, const double *iwc,
                                const double *overlap, double *ql, double *qi);
double grt_clouds_beta(int inverse, int p, int q, double x);

/* Band-level optics for the batched pipeline's all-sky pass (grt_pipeline_run_allsky, grt_ext.h), which takes the optics
   per band and maps them onto its grids itself.  grt_clouds_band_optics: what cloud_optics computes before it spreads
   the bands onto a grid -- the same rand() calls in the same order -- as liquid[3][B][L] and ice[3][B][L] (extinction m-1,
   single-scattering albedo, asymmetry; band b of the ice is the ice parametrisation's band b), B the liquid
   parametrisation's band count.  grt_clouds_bands: the loaded band limits in cm-1 (ice != 0: the ice's), as the library
   uses them (rounded to single precision); lo / hi may be NULL to ask for the count. */
int grt_clouds_band_optics(int num_layers, const double *cf, const double *lwc, const double *iwc, const double *overlap,
                           const double liquid_radius, const double *layer_temperature, double *liquid, double *ice);
int grt_clouds_bands(int ice, int *num_bands, double *lo, double *hi);

#endif
