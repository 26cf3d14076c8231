/* sweep_bounds_main.c -- the oracle's sweep methods on grids of a few bins, as a program of its own so that it can be
 * built with -fsanitize=address,undefined (tests/test_oracle_sweep_shapes.py compiles it together with
 * oracle/grt_oracle.c and runs it as a child process).
 *
 * Grids: m = 1, 2, 3, 25, 26, 27 bins at dw = 2, 1, 0.3, 0.25 (1, 2, 4, 5 points a bin), m ppb points and, where a bin
 * has more than one point, m ppb + 1; from 500 cm-1; a grid of one point is left out (no grid constructor makes one).
 * 37 prepared lines in 3 layers, centres 0.1 cm-1 inside the grid's ends, shifted by up to 0.02 cm-1 per layer, so
 * that the per-layer sort has work to do.  Both methods.  Prints one checksum per method; exit status 0 unless a
 * result is not finite or is negative. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "grt_oracle.h"

enum { LAYERS = 3, LINES = 37 };

static uint64_t state = 20261020u;

static double uniform(void)         /* [0, 1) */
{
    state = state*6364136223846793005ull + 1442695040888963407ull;
    return (double)(state >> 11)/9007199254740992.;
}

static int compare(void const *a, void const *b)
{
    double const x = *(double const *)a, y = *(double const *)b;
    return (x > y) - (x < y);
}

int main(void)
{
    int const bins_of[] = {1, 2, 3, 25, 26, 27};
    double const dws[] = {2., 1., 0.3, 0.25};
    double const w0 = 500.;
    double sum[2] = {0., 0.};
    int grids = 0, bad = 0;
    for (int a = 0; a < 6; ++a)
    {
        for (int b = 0; b < 4; ++b)
        {
            int const ppb = (int)(floor(1./dws[b]) + 1);
            for (int extra = 0; extra <= (ppb > 1 ? 1 : 0); ++extra)
            {
                uint64_t const nw = (uint64_t)bins_of[a]*ppb + extra;
                if (nw < 2)
                {
                    continue;
                }
                double const lo = w0 + 0.1, hi = w0 + (nw - 1)*dws[b] - 0.1;
                double v0[LINES], ns[LAYERS];
                for (int k = 0; k < LINES; ++k)
                {
                    v0[k] = lo + (hi - lo)*uniform();
                }
                qsort(v0, LINES, sizeof(*v0), compare);
                for (int method = 0; method < 2; ++method)
                {
                    double *buf = malloc(sizeof(*buf)*4*LAYERS*LINES);
                    double *vnn = buf, *snn = buf + LAYERS*LINES, *gamma = buf + 2*LAYERS*LINES, *alpha = buf + 3*LAYERS*LINES;
                    for (int i = 0; i < LAYERS; ++i)
                    {
                        ns[i] = 1e18*pow(30., i);
                        for (int k = 0; k < LINES; ++k)
                        {
                            int const o = i*LINES + k;
                            vnn[o] = v0[k] + 0.02*(2.*uniform() - 1.)*(i + 1)/LAYERS;
                            snn[o] = 1e-22*(0.1 + uniform());
                            gamma[o] = 0.07*pow(30., i - 2)*(0.5 + uniform());
                            alpha[o] = 5e-4*(0.8 + 0.4*uniform());
                        }
                    }
                    double *tau = calloc((size_t)LAYERS*nw, sizeof(*tau));
                    OrcBins bins;
                    orc_bins_create(&bins, LAYERS, w0, nw, dws[b], 1.);
                    if (method == 0)
                    {
                        orc_sort_lines(LINES, LAYERS, vnn, snn, gamma, alpha);
                        orc_bin_sweep(LINES, LAYERS, vnn, snn, gamma, alpha, ns, &bins, tau);
                    }
                    else
                    {
                        orc_line_sweep(LINES, LAYERS, vnn, snn, gamma, alpha, ns, &bins, tau);
                    }
                    orc_interpolate(&bins, tau);
                    orc_bins_destroy(&bins);
                    for (uint64_t f = 0; f < LAYERS*nw; ++f)
                    {
                        if (!(tau[f] >= 0.) || !isfinite(tau[f]))
                        {
                            ++bad;
                        }
                        sum[method] += tau[f];
                    }
                    free(tau);
                    free(buf);
                }
                ++grids;
            }
        }
    }
    printf("%d grids, %d bad values, checksums %.17g %.17g\n", grids, bad, sum[0], sum[1]);
    return bad == 0 ? 0 : 1;
}
