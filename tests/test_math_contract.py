"""The numeric contract (include/chroma_math.h) against double-precision NumPy, and the
Philox4x32-10 generator against the published Random123 known-answer vectors."""
import numpy as np
import pytest

import contract_inputs as ci


def ulp_err(got, ref64):
    ref32 = ref64.astype(np.float32)
    ulp = np.spacing(np.abs(ref32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref64) / np.maximum(ulp, 1e-45)


@pytest.fixture(scope='module')
def rng():
    return np.random.default_rng(1234)


def test_log_exp(oracle_mod, rng):
    x = rng.uniform(0, 1, 200000).astype(np.float32)
    x[x == 0] = 1e-10
    assert ulp_err(oracle_mod.math_fn('log', x), np.log(x.astype(np.float64))).max() < 1.5
    x = (10 ** rng.uniform(-37, 38, 100000)).astype(np.float32)
    assert ulp_err(oracle_mod.math_fn('log', x), np.log(x.astype(np.float64))).max() < 1.5
    x = rng.uniform(-87, 88, 200000).astype(np.float32)
    assert ulp_err(oracle_mod.math_fn('exp', x), np.exp(x.astype(np.float64))).max() < 1.5
    special = np.array([0.0, -1.0, np.inf, 1.0], dtype=np.float32)
    out = oracle_mod.math_fn('log', special)
    assert out[0] == -np.inf and np.isnan(out[1]) and out[2] == np.inf and out[3] == 0.0
    assert oracle_mod.math_fn('exp', np.array([-200.0, 200.0, 0.0], np.float32)).tolist() == [0.0, np.inf, 1.0]


def test_trig(oracle_mod, rng):
    x = rng.uniform(-20, 20, 200000).astype(np.float32)
    x64 = x.astype(np.float64)
    assert np.abs(oracle_mod.math_fn('sin', x) - np.sin(x64)).max() < 1.5e-7
    assert np.abs(oracle_mod.math_fn('cos', x) - np.cos(x64)).max() < 1.5e-7
    t = oracle_mod.math_fn('tan', x)
    assert np.max(np.abs(t - np.tan(x64)) / np.abs(np.tan(x64))) < 5e-7


def test_inverse_trig(oracle_mod, rng):
    x = rng.uniform(-1, 1, 200000).astype(np.float32)
    x64 = x.astype(np.float64)
    assert ulp_err(oracle_mod.math_fn('asin', x), np.arcsin(x64)).max() < 3.0
    assert ulp_err(oracle_mod.math_fn('acos', x), np.arccos(x64)).max() < 2.0
    # out of range -> NaN: this is how total internal reflection is detected (photon.h:314,335)
    out = oracle_mod.math_fn('asin', np.array([1.0000001, -1.5, 1.0, -1.0], np.float32))
    assert np.isnan(out[0]) and np.isnan(out[1]) and out[2] == np.float32(np.pi / 2) and out[3] == -np.float32(np.pi / 2)
    y = rng.normal(size=100000).astype(np.float32)
    x2 = rng.normal(size=100000).astype(np.float32)
    assert np.abs(oracle_mod.math_fn('atan2', y, x2) - np.arctan2(y.astype(np.float64), x2.astype(np.float64))).max() < 4e-7


def test_contract_vs_libm_variant(oracle_mod, rng):
    x = rng.uniform(1e-6, 1, 10000).astype(np.float32)
    a = oracle_mod.math_fn('log', x)
    b = oracle_mod.math_fn('log', x, variant='libm')
    assert np.max(np.abs(a - b) / np.abs(b)) < 3e-7


def test_philox_known_answers(oracle_mod):
    # Random123 kat_vectors, philox4x32 with 10 rounds
    kat = [
        ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
        ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
        ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
         [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
    ]
    for ctr, key, expect in kat:
        assert oracle_mod.philox(ctr, key).tolist() == expect


def test_uniform_stream(oracle_mod):
    u = oracle_mod.uniform_stream(12345, 77, 4096)
    assert u.min() > 0.0 and u.max() <= 1.0            # curand_uniform's (0, 1]
    assert abs(u.mean() - 0.5) < 0.02
    # resuming mid-stream gives the same numbers: the per-photon counter is all the state
    assert np.array_equal(oracle_mod.uniform_stream(12345, 77, 96, start=1000), u[1000:1096])
    # word -> float mapping of curand_uniform: x * 2^-32 + 2^-33
    words = np.array([0, 1, 0x7fffffff, 0xffffffff], dtype=np.uint32)
    got = oracle_mod.math_fn('uniform', words.view(np.float32))
    expect = (words.astype(np.float32) * np.float32(2.0 ** -32) + np.float32(2.0 ** -33)).astype(np.float32)
    assert np.array_equal(got, expect) and got[-1] == 1.0 and got[0] > 0
    # different photons and seeds decorrelate
    v = oracle_mod.uniform_stream(12345, 78, 4096)
    assert abs(np.corrcoef(u, v)[0, 1]) < 0.05


# ---- the WHOLE declared domain of each function against float64: deterministic strided sweeps over the bit patterns (every
# binade is visited, about 4 million points per function), the +-8 ulp neighbours of the header's branch constants, the
# special values and the zero signs.  The bounds are the ones above; tan's bound as an angle is the sin/cos figure (the same
# reduction, the same class of polynomial). ------------------------------------------------------------------------------
def sweep(lo_bits, hi_bits, stride, both_signs=False):
    """The floats with bit patterns lo, lo + stride, ... up to and including hi (non-negative ones; optionally mirrored)."""
    b = np.concatenate([np.arange(lo_bits, hi_bits, stride, dtype=np.int64), [hi_bits]]).astype(np.uint32)
    if both_signs:
        b = np.concatenate([b, b | np.uint32(0x80000000)])
    return ci.f32(b)


def test_log_whole_domain(oracle_mod):
    x = np.concatenate([sweep(1, ci.FLT_MAX_BITS, 509), ci.f32(ci.branch_points('log'))])         # every positive float class, subnormals included
    assert len(x) > 4000000 and x.min() == ci.f32([1])[0] and (x < ci.f32([ci.FLT_MIN_BITS])[0]).sum() > 16000
    assert ulp_err(oracle_mod.math_fn('log', x), np.log(x.astype(np.float64))).max() < 1.5
    out = oracle_mod.math_fn('log', ci.f32([0, 0x80000000, 0x7f800000, 0x80000001, 0xbf800000, 0xff800000, 0x7fc00000, 0x7f800001]))
    assert out[0] == -np.inf and out[1] == -np.inf and out[2] == np.inf and np.isnan(out[3:]).all()


def test_exp_whole_domain(oracle_mod):
    hi, lo = np.float32(ci.EXP_HI), np.float32(ci.EXP_LO)
    x = np.concatenate([sweep(0, ci.word(hi), 521), -sweep(0, ci.word(-lo), 521), ci.f32(ci.branch_points('exp'))])
    x = np.unique(x[(x >= lo) & (x <= hi)])
    assert len(x) > 4000000 and x.max() == hi and x.min() == lo
    got, ref = oracle_mod.math_fn('exp', x), np.exp(x.astype(np.float64))
    # (the largest argument, 0x42b17218, lies 3e-7 above log(FLT_MAX): there the correctly rounded single is +inf itself)
    over = ref >= 2.0 ** 128 * (1 - 2.0 ** -25)
    assert over.sum() == 1 and x[over][0] == hi and got[over][0] == np.inf
    ok = (ref >= np.finfo(np.float32).tiny) & ~over
    assert ok.sum() > len(x) - 4 and np.isfinite(got[ok]).all()
    assert ulp_err(got[ok], ref[ok]).max() < 1.5
    # outside: exactly 0 below the lower limit, exactly +inf above the upper one, NaN for NaN
    below = -sweep(ci.word(-lo) + 1, 0x7f800000, 8191)
    above = sweep(ci.word(hi) + 1, 0x7f800000, 8191)
    assert below[0] == np.nextafter(lo, np.float32(-np.inf)) and below[-1] == -np.inf and above[0] == np.nextafter(hi, np.float32(np.inf))
    assert np.array_equal(ci.bits(oracle_mod.math_fn('exp', below)), np.zeros(len(below), np.uint32))            # +0, bit for bit
    assert (oracle_mod.math_fn('exp', above) == np.inf).all()
    assert np.isnan(oracle_mod.math_fn('exp', ci.f32([0x7fc00000, 0xffc00000, 0x7f800001]))).all()


def trig_sweep():
    x = np.concatenate([sweep(0, ci.word(ci.TRIG_MAX), 587, both_signs=True), ci.f32(ci.trig_borders())])
    x = x[np.abs(x) <= ci.TRIG_MAX]
    assert len(x) > 4000000 and x.max() == ci.TRIG_MAX and x.min() == -ci.TRIG_MAX
    return x


def outside_trig():
    x = sweep(ci.word(ci.TRIG_MAX) + 1, 0x7f800000, 4093, both_signs=True)           # 8192 + 1 ulp ... inf
    return np.concatenate([x, ci.f32([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001])])


def test_sin_cos_whole_domain(oracle_mod):
    x = trig_sweep()
    x64 = x.astype(np.float64)
    assert np.abs(oracle_mod.math_fn('sin', x) - np.sin(x64)).max() < 1.5e-7
    assert np.abs(oracle_mod.math_fn('cos', x) - np.cos(x64)).max() < 1.5e-7
    out = outside_trig()
    assert np.isnan(oracle_mod.math_fn('sin', out)).all() and np.isnan(oracle_mod.math_fn('cos', out)).all()


def test_tan_whole_domain_as_an_angle(oracle_mod):
    """Over [-8192, 8192] tan is held as an ANGLE: |t - ref| / (1 + ref^2) is the error of atan(t).  Its relative error is
    bounded on [-20, 20] only (test_trig above; 1.65e-7 measured): near its zeros and poles the absolute error of the
    three-part reduction, which grows with the argument, is divided by a value near 0 -- 1.2e-5 at 2668.78296."""
    x = np.concatenate([trig_sweep(), ci.f32(ci.neighbours([1e-4], both_signs=True))])
    t = oracle_mod.math_fn('tan', x).astype(np.float64)
    ref = np.tan(x.astype(np.float64))
    assert np.isfinite(t).all()
    assert (np.abs(t - ref) / (1.0 + ref * ref)).max() < 1.5e-7
    near = np.abs(x) <= 20
    assert near.sum() > 3000000 and np.max(np.abs(t[near] - ref[near])[ref[near] != 0] / np.abs(ref[near][ref[near] != 0])) < 5e-7
    assert np.isnan(oracle_mod.math_fn('tan', outside_trig())).all()


def test_asin_acos_whole_domain(oracle_mod):
    x = np.concatenate([sweep(0, 0x3f800000, 541, both_signs=True), ci.f32(ci.branch_points('asin')), ci.f32(ci.branch_points('acos'))])
    out = x[np.abs(x) > 1]
    assert len(out) == 4 * 8                    # the 8 neighbours beyond +-1, from both functions' lists
    assert np.isnan(oracle_mod.math_fn('asin', out)).all() and np.isnan(oracle_mod.math_fn('acos', out)).all()
    x = x[np.abs(x) <= 1]
    x64 = x.astype(np.float64)
    assert len(x) > 3900000 and x.max() == 1 and x.min() == -1
    assert ulp_err(oracle_mod.math_fn('asin', x), np.arcsin(x64)).max() < 3.0
    assert ulp_err(oracle_mod.math_fn('acos', x), np.arccos(x64)).max() < 2.0
    assert np.isnan(oracle_mod.math_fn('asin', ci.f32([0x7fc00000, 0x7f800000, 0xff800000]))).all()
    assert np.isnan(oracle_mod.math_fn('acos', ci.f32([0x7fc00000, 0x7f800000, 0xff800000]))).all()


def test_atan2_exponent_and_sign_grid(oracle_mod):
    # every pair of finite exponent fields (0: zero and the subnormals) x 4 mantissas each x all four sign pairs
    v = ((np.arange(255, dtype=np.uint32) << 23)[:, None] | np.array([0, 0x7fffff, 0x400000, 0x2aaaaa], np.uint32)[None, :]).ravel()
    v = np.concatenate([v, v | np.uint32(0x80000000)])
    yb, xb = np.meshgrid(v, v, indexing='ij')
    y, x = ci.f32(yb.ravel()), ci.f32(xb.ravel())
    assert len(y) == 2040 * 2040
    got = oracle_mod.math_fn('atan2', y, x)
    assert np.abs(got - np.arctan2(y.astype(np.float64), x.astype(np.float64))).max() < 4e-7
    # atan alone (atan2(v, 1)) with the neighbours of its two branch constants: within the 3 ulp the header's class allows
    a = np.concatenate([sweep(0, ci.FLT_MAX_BITS, 1021, both_signs=True), ci.f32(ci.branch_points('atan'))])
    assert ulp_err(oracle_mod.math_fn('atan2', a, np.ones_like(a)), np.arctan(a.astype(np.float64))).max() < 3.0
    assert np.array_equal(oracle_mod.math_fn('atan', a), oracle_mod.math_fn('atan2', a, np.ones_like(a)))        # (as values: -0 == +0)


def test_atan2_special_values(oracle_mod):
    """C's atan2 in every zero / infinity / NaN combination, the finite operands +-denorm, +-1, +-FLT_MAX beside them.  The
    value is C's everywhere.  The SIGN OF A ZERO result is C's for x = -0 and x = +0, and pinned AS IT IS where the header
    departs from C: for x > 0 the result is formed as 0.0f + atan(y / x), so atan2(-0, x > 0) and atan2(y < 0, +inf) give +0
    where C gives -0.  (The bits are shared with the reference-physics libraries built from the same header: recorded, not
    changed.)"""
    s = ci.f32(ci.SPECIALS)
    y, x = [a.ravel() for a in np.meshgrid(s, s, indexing='ij')]
    special = ~(np.isfinite(y) & (y != 0) & np.isfinite(x) & (x != 0))             # at least one zero, infinity or NaN
    y, x = y[special], x[special]
    got = oracle_mod.math_fn('atan2', y, x)
    with np.errstate(all='ignore'):
        want = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(np.float32)
    nan = np.isnan(y) | np.isnan(x)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan], want[~nan])                                   # the values (here -0 == +0) ...
    zero = ~nan & (want == 0)
    # ... and the zeros' signs: the 9 pairs with x > 0 and y = -0 (5), or y < 0 finite beside x = +inf (4), are C's -0 and the header's +0
    departs = zero & (x > 0) & np.signbit(y)
    assert departs.sum() == 9 and np.signbit(want[departs]).all()
    assert (ci.bits(got[departs]) == 0).all()
    assert np.array_equal(ci.bits(got[~nan & ~departs]), ci.bits(want[~nan & ~departs]))      # every other result, zeros included, bit for bit C's
    pi = np.float32(np.pi)
    z = oracle_mod.math_fn('atan2', ci.f32([0, 0x80000000, 0, 0x80000000]), ci.f32([0x80000000, 0x80000000, 0, 0]))
    assert ci.bits(z).tolist() == ci.bits(np.array([pi, -pi, 0.0, -0.0], np.float32)).tolist()      # atan2(+-0, -0) = +-pi, atan2(+-0, +0) = +-0


def test_zero_signs_are_pinned(oracle_mod):
    """sin(-0) and tan(-0) give +0 (`sneg` is x < 0), asin(-0) gives -0 (returned as it came): different from libm, and kept,
    because the engine, the oracle and the reference-physics libraries all produce these bits from the one header."""
    mz = ci.f32([0x80000000])
    for fn, want in (('sin', 0), ('tan', 0), ('asin', 0x80000000), ('cos', 0x3f800000), ('acos', int(ci.bits(np.float32(np.pi / 2))[0])),
                     ('exp', 0x3f800000), ('sqrt', 0x80000000), ('atan', 0x00000000), ('floor', 0x80000000), ('round', 0x80000000)):
        assert int(ci.bits(oracle_mod.math_fn(fn, mz))[0]) == want, fn
    pz = ci.f32([0])
    for fn in ('sin', 'tan', 'asin', 'atan', 'sqrt', 'floor', 'round'):
        assert int(ci.bits(oracle_mod.math_fn(fn, pz))[0]) == 0, fn


def test_exact_primitives_against_numpy(oracle_mod):
    """The ops that are ONE correctly rounded IEEE operation, or exact, on the host build: sqrt and the quotient (float64's
    53 bits make the double rounding harmless for both), floor, round (half away from zero), fmin / fmax as CUDA's (a NaN
    operand yields the other), the saturating conversions, the word -> (0, 1] mapping, and a fused fma."""
    rng = np.random.default_rng(7)
    with np.errstate(all='ignore'):
        x = ci.f32(np.concatenate([ci.unary_grid(rng, 509), ci.integer_borders()]))
        x64 = x.astype(np.float64)
        same = lambda got, want: np.array_equal(ci.bits(got)[~np.isnan(want)], ci.bits(want)[~np.isnan(want)]) and np.array_equal(np.isnan(got), np.isnan(want))
        assert same(oracle_mod.math_fn('sqrt', x), np.sqrt(x64).astype(np.float32))
        assert same(oracle_mod.math_fn('floor', x), np.floor(x64).astype(np.float32))
        assert same(oracle_mod.math_fn('round', x), np.copysign(np.floor(np.abs(x64) + 0.5), x64).astype(np.float32))
        i = ci.bits(oracle_mod.math_fn('f2i', x)).view(np.int32)
        assert np.array_equal(i, np.where(np.isnan(x64), 0, np.clip(np.trunc(x64), -2.0 ** 31, 2.0 ** 31 - 1)).astype(np.int64).astype(np.int32))
        u = ci.bits(oracle_mod.math_fn('f2u32', x))
        assert np.array_equal(u, np.where(np.isnan(x64), 0, np.clip(np.trunc(x64), 0, 2.0 ** 32 - 1)).astype(np.uint64).astype(np.uint32))
        a, b = [ci.f32(w) for w in ci.binary_inputs(rng, 1 << 16)]
        assert same(oracle_mod.math_fn('div', a, b), (a.astype(np.float64) / b.astype(np.float64)).astype(np.float32))
        an, bn = np.isnan(a), np.isnan(b)
        assert same(oracle_mod.math_fn('fmin', a, b), np.where(an, b, np.where(bn, a, np.where(b < a, b, a))))
        assert same(oracle_mod.math_fn('fmax', a, b), np.where(an, b, np.where(bn, a, np.where(b > a, b, a))))
    w = ci.uniform_inputs(rng, 1 << 16)
    got = oracle_mod.math_fn('uniform', ci.f32(w))
    # x * 2^-32 + 2^-33 with (float)x rounded to nearest even first: float64 holds every intermediate exactly
    assert np.array_equal(got, (w.astype(np.float32).astype(np.float64) * 2.0 ** -32 + 2.0 ** -33).astype(np.float32))
    assert got.min() > 0.0 and got.max() == 1.0
    assert got[ci.UNIFORM_WORDS.index(0xffffff80)] == 1.0 and got[ci.UNIFORM_WORDS.index(0xffffff7f)] == np.float32(1 - 2.0 ** -24)
    # fused: (1 + 2^-12)(1 - 2^-12) - 1 = -2^-24 exactly; an unfused multiply rounds the product to 1 and gives 0
    one = np.ones(1, np.float32)
    assert oracle_mod.math_fn('fma', one + np.float32(2.0 ** -12), one - np.float32(2.0 ** -12), -one)[0] == np.float32(-2.0 ** -24)


def test_rng_probe_streams(oracle_mod):
    """The probe with a stream word: stream 0 is oracle_uniform_stream; the stream word and the high id word change the
    draws; the draws continue across a block border and across the wrap of the 32-bit draw counter; a normal deviate is
    Box-Muller's cosine branch of two consecutive uniforms."""
    row = lambda seed, pid, stream, start: [seed & 0xffffffff, seed >> 32, pid & 0xffffffff, pid >> 32, stream, start]
    u = oracle_mod.rng_probe('rng_uniform', [row(12345, 77, 0, 0), row(12345, 77, 0, 3), row(12345, 77, 1, 0), row(12345, 77 + (1 << 32), 0, 0),
                                             row(12345, 77, 0, 0xfffffffc), row(12345, 77, 0, 0xffffffff)])
    s = oracle_mod.uniform_stream(12345, 77, 16)
    assert np.array_equal(u[0], s[:8]) and np.array_equal(u[1], s[3:11])
    assert not np.array_equal(u[2], u[0]) and not np.array_equal(u[3], u[0])
    assert np.array_equal(u[4][4:], s[:4]) and np.array_equal(u[5][1:], s[:7]) and np.array_equal(u[4][3:], u[5][:5])     # the counter wraps to 0
    for start in ci.STREAM_STARTS:
        un = oracle_mod.rng_probe('rng_uniform', [row(9, 1 << 40, 0xffffffff, start)])[0].astype(np.float64)
        g = oracle_mod.rng_probe('rng_normal', [row(9, 1 << 40, 0xffffffff, start)])[0]
        want = np.sqrt(-2.0 * np.log(un[0::2])) * np.cos(2 * np.pi * un[1::2])
        # radius <= sqrt(-2 log 2^-33) = 6.8; the angle 6.2831855f * u2 is rounded to single (<= 3.8e-7) and cm_cosf adds
        # 1.5e-7 at most: 6.8 * 5.3e-7 = 3.6e-6, and a few ulp of the radius and of the product (<= 1e-6) on top
        assert np.abs(g - want).max() < 5e-6
    for ctr, key, expect in ci.PHILOX_KAT:
        assert oracle_mod.rng_probe('philox', [ctr + key])[0].tolist() == expect
