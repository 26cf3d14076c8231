"""What the device cloud sampler's tests (test_cloud_sampler_host.py, test_gpu_cloud_sampler.py,
test_gpu_pipeline_cloud_fields.py) share: Philox4x32-10 in numpy, written from the published algorithm (Salmon, Moraes,
Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC11), the draws the sampler takes from it, cloud fields that
hold the sampler's edge cases, and the expected tables from cloud_bands.band_optics fed given draws in the driver's order.
A plain module: pytest does not rewrite its asserts."""
import numpy as np

from cloud_bands import band_optics

M0, M1 = 0xD2511F53, 0xCD9E8D57           # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85           # the key increments (golden ratio, sqrt(3) - 1)
MAX_SUBCOLUMNS = 64                       # grt_ext.h: GRT_MAX_SUBCOLUMNS
SETS = ("lw_liquid", "lw_ice", "sw_liquid", "sw_ice")
TFREEZE = np.float64(273.16)


def philox4x32_10(counter, key):
    """counter [..., 4] and key (k0, k1) of 32-bit words -> [..., 4] uint32: ten rounds, the key bumped between rounds."""
    counter = np.asarray(counter, dtype=np.uint64)
    c = [counter[..., j] for j in range(4)]
    k0, k1 = int(key[0]) & 0xffffffff, int(key[1]) & 0xffffffff
    low = np.uint64(0xffffffff)
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & low, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & low]
    return np.stack(c, axis=-1).astype(np.uint32)


def unit_interval(hi, lo):
    """53 bits of two 32-bit words as a double in [0, 1): ((hi >> 5) 2^26 + (lo >> 6)) 2^-53."""
    hi, lo = np.asarray(hi, dtype=np.uint32), np.asarray(lo, dtype=np.uint32)
    return ((hi >> np.uint32(5)).astype(np.float64) * 2.0 ** 26 + (lo >> np.uint32(6)).astype(np.float64)) * 2.0 ** -53


def philox_uniforms(seed, column_offset, ncol, S, B, L):
    """[ncol][2][S][B][2 L - 1]: the draws of the sampler's generator mode in its uniforms layout.  Key (seed's low word,
    its high word); counter (layer, band, pass 64 + s, column_offset + c); words 0, 1 give layer i's rank, words 2, 3 the
    decision of the pair (i, i + 1)."""
    c, p, s, b, i = np.meshgrid(np.arange(ncol), np.arange(2), np.arange(S), np.arange(B), np.arange(L), indexing="ij")
    counter = np.stack([i, b, p * MAX_SUBCOLUMNS + s, (column_offset + c) & 0xffffffff], axis=-1)
    r = philox4x32_10(counter, (seed & 0xffffffff, (seed >> 32) & 0xffffffff))
    rank, decide = unit_interval(r[..., 0], r[..., 1]), unit_interval(r[..., 2], r[..., 3])
    return np.concatenate([rank, decide[..., :L - 1]], axis=-1)


def libc_uniforms(rand, ncol, S, B, L):
    """[ncol][2][S][B][2 L - 1] from successive rand() calls: libc's order for a driver with num_subcolumns = S."""
    n = ncol * 2 * S * B * (2 * L - 1)
    return np.array([rand() for _ in range(n)]).reshape(ncol, 2, S, B, 2 * L - 1)


def boundary(degrees):
    """The temperature exactly on an ice class boundary, as the library forms it: tfreeze - degrees in double."""
    return TFREEZE - np.float64(degrees)


def edge_fields(ncol, L, seed):
    """Cloud fields [ncol][L] whose layers cycle, from (layer + column), through: partial cover with liquid and ice,
    overcast, liquid only, clear, ice only, cloudy with no water at all; temperatures through the eight ice classes and
    exactly on two class boundaries; overlap parameters through 0.5, 0, 1 and 0.9."""
    rng = np.random.default_rng(seed)
    temps = [260.0, 245.0, boundary(25.0), 240.0, 235.0, 230.0, boundary(40.0), 225.0, 220.0, 210.0]
    cf, lwc, iwc, t = (np.zeros((ncol, L)) for _ in range(4))
    ov = np.zeros((ncol, max(L - 1, 0)))
    for c in range(ncol):
        for j in range(L):
            kind = (j + c) % 6
            cf[c, j] = (0.75, 1.0, 0.6, 0.0, 0.5, 0.7)[kind]
            wet, icy = kind in (0, 1, 2), kind in (0, 1, 4)
            lwc[c, j] = 0.05 + 0.2 * rng.random() if wet else 0.0
            iwc[c, j] = 0.005 + 0.03 * rng.random() if icy else 0.0
            t[c, j] = temps[(j + 3 * c) % len(temps)]
            if j < L - 1:
                ov[c, j] = (0.5, 0.0, 1.0, 0.9)[(j + c) % 4]
    return dict(cf=cf, lwc=lwc, iwc=iwc, t=t, ov=ov)


def plant_edges(u, f):
    """Into the draws u [ncol][2][S][B][2 L - 1] of edge_fields' column 0, first pass and subcolumn, what a generator
    hardly ever gives: a decision exactly equal to its overlap (band 0, pair 0: the copy is taken), a rank exactly
    1 - cf on a layer that keeps its own rank (band 0, layer 2: not cloudy, the comparison is strict), and -- bands 1 and
    2, where there are that many -- a first rank beyond the last table abscissa and one exactly on it."""
    L = f["cf"].shape[1]
    B = u.shape[3]
    if L >= 2:
        u[0, 0, 0, 0, L + 0] = f["ov"][0, 0]                       # decide[0] == overlap[0] = 0.5
    if L >= 3:
        u[0, 0, 0, 0, L + 1] = 0.25                                 # > overlap[1] = 0: layer 2 keeps its own rank
        u[0, 0, 0, 0, 2] = 1.0 - f["cf"][0, 2]
    else:
        u[0, 1, 0, 0, 0] = 1.0 - f["cf"][0, 0]                      # (second pass: layer 0 always keeps its rank)
    if B >= 2:
        u[0, 0, 0, 1, 0] = 1.25
    if B >= 3:
        u[0, 0, 0, 2, 0] = 1.0
    return u


def expected_tables(tables, f, u, liquid_radius=10.0):
    """[4][S][ncol][3][B][L], the sampler's output layout, from cloud_bands.band_optics fed the draws u
    [ncol][2][S][B][2 L - 1] in their order."""
    ncol, _, S, B, _ = u.shape
    L = f["cf"].shape[1]
    out = np.zeros((4, S, ncol, 3, B, L))
    with np.errstate(invalid="ignore", divide="ignore"):            # (a cloudy layer with no water: 0/0, as in the library)
        for c in range(ncol):
            for p in range(2):
                for s in range(S):
                    draw = iter(u[c, p, s].ravel()).__next__
                    liquid, ice = band_optics(tables, draw, f["cf"][c], f["lwc"][c], f["iwc"][c], f["ov"][c], liquid_radius,
                                              f["t"][c])
                    out[2 * p, s, c], out[2 * p + 1, s, c] = liquid, ice
    return out


def pipeline_fields(cols, seed, clear=False):
    """Cloud fields of each column as pipeline_support.subcolumn_clouds makes them -- overcast, partial and clear layers,
    ice only aloft, liquid only at the bottom --, the overlap parameter and the layer thickness."""
    L = cols[0]["p"].size - 1
    rng = np.random.default_rng(seed)
    out = {k: [] for k in ("cf", "lwc", "iwc", "ov", "th", "t")}
    for c, col in enumerate(cols):
        cf = np.where(rng.random(L) < 0.5, rng.random(L), 0.0)
        cf[L - 3 - c % 4] = 1.0
        cf[2] = 0.0
        lwc = np.where(cf > 0, 0.2 * rng.random(L), 0.0)
        iwc = np.where(cf > 0, 0.03 * rng.random(L), 0.0)
        lwc[np.arange(L) < L // 3] = 0.0
        iwc[L - 2:] = 0.0
        cf[(lwc + iwc) == 0.0] = 0.0
        if clear:
            cf[:], lwc[:], iwc[:] = 0.0, 0.0, 0.0
        out["cf"].append(cf)
        out["lwc"].append(lwc)
        out["iwc"].append(iwc)
        out["ov"].append(np.exp(-np.abs(np.diff(np.log(col["p"][1:] + col["p"][:-1]))) / 0.5))
        out["th"].append(29.3 * col["t_layer"] * np.log(col["p"][1:] / col["p"][:-1]))
        out["t"].append(col["t_layer"])
    return {k: np.array(v) for k, v in out.items()}
