"""Surface albedo parametrisations that depend on the sun's elevation, for the knots of api.make_zenith_surface."""
import numpy as np


def ocean_direct_albedo(mu):
    """Direct-beam albedo of open water under a sun of zenith cosine mu (Taylor et al. 1996, Q. J. R. Meteorol. Soc. 122,
    839-861): 0.037/(1.1 mu**1.4 + 0.15) -- 0.0296 under an overhead sun, 0.037/0.15 = 0.2467 at the horizon.  mu: a
    scalar or an array; values below 0 (night samples) take the horizon's value, so that the knots stay in [0, 1]."""
    m = np.clip(np.asarray(mu, dtype=np.float64), 0.0, 1.0)
    return 0.037 / (1.1 * m ** 1.4 + 0.15)
