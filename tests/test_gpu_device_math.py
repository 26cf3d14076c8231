"""The device math the line kernels and the solvers rest on (grt_debug_device_math), each function against
numpy.longdouble (x87 extended: 64-bit significand, exponents far beyond a double's, so that subnormal doubles need no
other reference) at 2^18 arguments, and each held to the bound its own comment states:

  grt_exp_pair / grt_exp (exp_pair.h; on the device every Horner step is an inline v_fma_f64, rint and ldexp come from the
      device library): <= 1.06 units in the last place, the bound tests/test_exp_pair.py asserts for the same text
      compiled by gcc, over that test's four argument classes and 700 < |x| <= 745, the rest of the header's domain;
      where the result is a subnormal double, <= 1 unit of 2^-1074 (the error of the scaled significand vanishes next to
      that spacing: one rounding is left); where e^x exceeds the largest double, inf; grt_exp's bits are the pair's; the
      special values as the host test requires them.  How many device results differ from the host's bits is printed.
  exp_fast: relative error <= 1.5e-7 on [-700, 2] -- one fp32 step of v_exp_f32 on a result in [0.707, 1.414], 2^-23,
      plus the narrowing of the reduced argument, 2^-26 ln 2, plus 1e-13 from the fp64 reduction.
  exp_fp64: relative error <= 1e-10, the code's claim, on (-2, 0], [-1, 1] (its two uses) and [-700, 700]; the series
      truncates at about 7e-12 and the measured worst should sit near that.
  reference_repwid: the correctly rounded float of 0.832554611f / alpha for alpha log-uniform over 1e-8 ... 1 (line
      centres from 1 cm-1 in cold layers to 50 000 cm-1 in warm ones), wherever the exact quotient is not within 1e-12
      (a hundred times the function's 1e-14) of a rounding tie."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from grtcode_amd import api

pytestmark = pytest.mark.gpu

LD = np.longdouble
N = 2 ** 18
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "grtcode_amd", "csrc", "hip", "exp_pair.h")
DBL_MAX, DBL_MIN = np.finfo(np.float64).max, np.finfo(np.float64).tiny
UNIT = LD(2.0) ** -1074

HOST = r"""
#include "%s"
void host_pair(long n, double const *x, double *p, double *m, double *one)
{
    for (long i = 0; i < n; ++i)
    {
        grt_exp_pair(x[i], &p[i], &m[i]);
        one[i] = grt_exp(x[i]);
    }
}
"""


def test_longdouble_is_wide_enough():
    assert np.finfo(LD).nmant >= 63 and np.finfo(LD).minexp <= -16000 and np.finfo(LD).maxexp >= 16000


def exp_arguments():
    """The four classes of tests/test_exp_pair.py -- the solver's domain, near zero, nearer, next to the reduction's
    breakpoints (n + 1/2) ln 2 -- and the rest of the header's domain, 700 < |x| <= 745."""
    rng = np.random.default_rng(7)
    k = N // 5
    u = lambda n: rng.uniform(-1.0, 1.0, n)
    brk = (np.floor(u(k) * 1000) + 0.5) * 0.6931471805599453 + (rng.uniform(0.0, 1.0, k) - 0.5) * 1e-9
    edge = rng.uniform(700.0, 745.0, N - 4 * k)
    edge[0], edge[1] = np.nextafter(700.0, 800.0), 745.0
    edge *= np.where(rng.uniform(size=edge.size) < 0.5, -1.0, 1.0)
    x = np.concatenate([u(k) * 700.0, u(k) * 2.0, u(k) * 1e-3, brk, edge])
    assert x.size == N and np.abs(x).max() == 745.0 and np.abs(x[: 4 * k]).max() <= 700.0
    return x


def exp_errors(got, x):
    """Error of got against e^x: in units of the last place where the result is a normal double, in units of 2^-1074
    where it is subnormal; where e^x is beyond the doubles got must be inf (error 0, else inf)."""
    want = np.exp(x.astype(LD))
    over, sub = want > LD(DBL_MAX), want < LD(DBL_MIN)
    # (within half a step above the largest double the correctly rounded result still is that double: none is drawn there)
    assert not np.any(over & (want < LD(DBL_MAX) * (1 + LD(2.0) ** -52)))
    _, e = np.frexp(want)
    with np.errstate(invalid="ignore", over="ignore"):
        err = np.abs(got.astype(LD) - want) / np.where(sub, UNIT, np.ldexp(LD(1.0), e - 53))
    err = np.where(over, np.where(np.isposinf(got), 0.0, np.inf), err)
    return err.astype(np.float64), over, sub


@pytest.fixture(scope="module")
def exps(device):
    x = exp_arguments()
    p, m = api.debug_device_math(device, "exp_pair", x)
    one, none = api.debug_device_math(device, "exp", x)
    assert none is None
    return x, p, m, one


def test_exp_pair_and_exp_are_within_about_one_unit_in_the_last_place(exps):
    x, p, m, one = exps
    worst = {}
    for name, got, arg in (("e^x", p, x), ("e^-x", m, -x), ("grt_exp", one, x)):
        err, over, sub = exp_errors(got, arg)
        normal = ~over & ~sub
        j, js = np.argmax(np.where(normal, err, 0)), np.argmax(np.where(sub, err, 0))
        print(f"{name}: worst {err[j]:.4f} units in the last place at x = {x[j]!r}; {int(sub.sum())} subnormal results, worst "
              f"{err[js]:.4f} units of 2^-1074 at x = {x[js]!r}; {int(over.sum())} beyond the doubles, all inf: {bool(np.all(err[over] == 0))}")
        worst[name] = (err[normal].max(), err[sub].max() if sub.any() else 0.0, err[over].max() if over.any() else 0.0)
        assert sub.sum() > 1000 and over.sum() > 1000 and np.all(np.isfinite(got[~over]))
    for name, (normal, sub, over) in worst.items():
        assert normal <= 1.06, name
        assert sub <= 1.0, name
        assert over == 0.0, name
    assert np.array_equal(one.view(np.uint64), p.view(np.uint64))          # grt_exp: the pair's e^x, bit for bit


def test_exp_special_values(device):
    p, m = api.debug_device_math(device, "exp_pair", np.array([0.0, np.nan]))
    assert p[0] == 1.0 and m[0] == 1.0 and np.isnan(p[1]) and np.isnan(m[1])
    one, _ = api.debug_device_math(device, "exp", np.array([0.0, np.nan, 800.0, -800.0, np.inf, -np.inf]))
    assert one[0] == 1.0 and np.isnan(one[1])
    assert one[2] == np.inf and one[3] == 0.0 and one[4] == np.inf and one[5] == 0.0      # beyond the clamp: as exp gives


def test_hooks_refuse_what_they_do_not_know(lib, device):
    a = np.zeros(4)
    o0, o1 = np.zeros(4), np.zeros(4)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    lib.grt_debug_device_math.argtypes = [C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    for op, n in ((5, 4), (-1, 4), (0, 0)):
        assert lib.grt_debug_device_math(device, op, n, dp(a), dp(o0), dp(o1)) != 0
    cls = np.zeros(4, dtype=np.int32)
    lib.grt_debug_voigt_points.argtypes = [C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]
    for variant, n in ((5, 4), (-1, 4), (0, 0)):
        assert lib.grt_debug_voigt_points(device, variant, n, dp(a), dp(a), dp(o0), cls.ctypes.data_as(C.POINTER(C.c_int))) != 0


def test_device_bits_against_the_host_compilation(exps, tmp_path):
    """The same header through gcc, as tests/test_exp_pair.py builds it: how many of the device's results have other
    bits.  Reported, not asserted: fma, rint and ldexp are exact operations on either side, so none is expected."""
    x, p, m, one = exps
    src = tmp_path / "host.c"
    src.write_text(HOST % HEADER)
    so = tmp_path / "libhost.so"
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src), "-lm"], check=True)
    host = C.CDLL(str(so))
    hp, hm, ho = np.zeros(N), np.zeros(N), np.zeros(N)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    host.host_pair(C.c_long(N), dp(x), dp(hp), dp(hm), dp(ho))
    for name, dev, hst in (("e^x", p, hp), ("e^-x", m, hm), ("grt_exp", one, ho)):
        differ = np.nonzero(dev.view(np.uint64) != hst.view(np.uint64))[0]
        first = f"; first at x = {x[differ[0]]!r}: device {dev[differ[0]]!r}, host {hst[differ[0]]!r}" if differ.size else ""
        print(f"{name}: {differ.size} of {N} device results differ from the host's bits{first}")
    assert np.all(np.isfinite(hp) | (hp == np.inf))


def test_exp_fast_is_within_its_fp32_step(device):
    x = np.random.default_rng(11).uniform(-700.0, 2.0, N)
    x[0], x[1] = -700.0, 2.0
    got, _ = api.debug_device_math(device, "exp_fast", x)
    want = np.exp(x.astype(LD))
    rel = (np.abs(got.astype(LD) - want) / want).astype(np.float64)
    j = np.argmax(rel)
    print(f"exp_fast: worst relative error {rel[j]:.3e} at x = {x[j]!r}")
    assert rel.max() <= 1.5e-7


def test_exp_fp64_keeps_its_claim(device):
    rng = np.random.default_rng(13)
    k = N // 3
    x = np.concatenate([-rng.uniform(0.0, 2.0, k), rng.uniform(-1.0, 1.0, k), rng.uniform(-700.0, 700.0, N - 2 * k)])
    x[0], x[k], x[2 * k], x[2 * k + 1] = 0.0, 1.0, -700.0, 700.0
    got, _ = api.debug_device_math(device, "exp_fp64", x)
    want = np.exp(x.astype(LD))
    rel = (np.abs(got.astype(LD) - want) / want).astype(np.float64)
    for name, s in (("(-2, 0]", slice(0, k)), ("[-1, 1]", slice(k, 2 * k)), ("[-700, 700]", slice(2 * k, N))):
        j = s.start + np.argmax(rel[s])
        print(f"exp_fp64 on {name}: worst relative error {rel[j]:.3e} at x = {x[j]!r}")
    assert rel.max() <= 1e-10


def repwid_cases():
    """alpha, the expected float, and which alpha are kept: the exact quotient (in long double: 5e-20) not within 1e-12
    relative of the midpoint of two neighbouring floats."""
    rng = np.random.default_rng(17)
    alpha = 10.0 ** rng.uniform(-8.0, 0.0, N)
    alpha[0], alpha[1] = 1e-8, 1.0
    q = LD(np.float32(0.832554611)) / alpha.astype(LD)
    f = q.astype(np.float32)
    lo, hi = np.nextafter(f, np.float32(0)), np.nextafter(f, np.float32(np.inf))
    mids = np.stack([(f.astype(LD) + lo.astype(LD)) / 2, (f.astype(LD) + hi.astype(LD)) / 2])
    keep = (np.abs(mids - q) / q).min(axis=0) >= LD(1e-12)
    want = np.float32(np.float64(np.float32(0.832554611)) / alpha)
    return alpha, want, keep


def test_repwid_ties_are_rare():
    alpha, want, keep = repwid_cases()
    print(f"reference_repwid: {int((~keep).sum())} of {N} alpha within 1e-12 of a rounding tie")
    assert (~keep).sum() < 1e-4 * N
    assert want.dtype == np.float32 and want.min() > 0.8 and want.max() < 1e8


def test_repwid_is_the_correctly_rounded_float(device):
    alpha, want, keep = repwid_cases()
    got, _ = api.debug_device_math(device, "repwid", alpha)
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)      # a float, widened
    wrong = keep & (got != want.astype(np.float64))
    print(f"reference_repwid: {int(wrong.sum())} of {int(keep.sum())} differ from the correctly rounded float"
          f"; at the {int((~keep).sum())} near-ties {int((got != want)[~keep].sum())} differ")
    assert not wrong.any(), (int(wrong.sum()), alpha[wrong][:5], got[wrong][:5], want[wrong][:5])
