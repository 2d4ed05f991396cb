"""Input arrays for the pins on the numeric contract (include/chroma_math.h), built BY CONSTRUCTION so that every edge is
certain to be present: tests/test_math_contract.py (the host build against float64) and tests/test_gpu_math_contract.py
(the device build against the host build, bit for bit) share them.  Everything is made of bit patterns; nothing here runs
the code under test."""
import numpy as np

FLT_MAX_BITS = 0x7f7fffff
FLT_MIN_BITS = 0x00800000
EXP_HI = 88.72283905206835          # cm_expf: +inf above
EXP_LO = -87.33654475055310         # cm_expf: 0 below
LOG2E = 1.44269504088896341
TRIG_MAX = 8192.0
TRIG_OCTANTS = 10431                # j * pi/4 <= 8192 for j <= 10430; 10431 is the first border beyond


def f32(b):
    return np.ascontiguousarray(np.asarray(b).astype(np.uint32)).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def word(v):
    """The bit pattern of one float32 value, as an int."""
    return int(bits(np.float32(v))[0])


def neighbours(values, k=8, both_signs=False):
    """The floats within k ulp of each value (sign-magnitude steps on the bit pattern: values are nonzero, finite)."""
    b = bits(np.asarray(values, np.float64).astype(np.float32).ravel()).astype(np.int64)
    mag, sign = b & 0x7fffffff, b & 0x80000000
    assert (mag > k).all() and (mag + k < 0x7f800000).all()
    out = ((mag[:, None] + np.arange(-k, k + 1)[None, :]) | sign[:, None]).ravel()
    if both_signs:
        out = np.concatenate([out, out ^ 0x80000000])
    return out.astype(np.uint32)


def unary_grid(rng, nrand=4093):
    """Every exponent field 0..255 x (mantissa all-zeros, all-ones, 0x400000, nrand random ones) x both signs: +-0, the
    smallest and the largest subnormal, +-FLT_MIN, +-FLT_MAX, +-inf, quiet and signalling NaNs with payloads.
    2 * 256 * (3 + nrand) words: 2 097 152 with the default."""
    mant = np.concatenate([np.tile(np.array([0, 0x7fffff, 0x400000], np.uint32), (256, 1)),
                           rng.integers(0, 1 << 23, (256, nrand), dtype=np.uint32)], axis=1)
    mant[0, 3] = 1                                       # the smallest subnormal
    mant[255, 3] = 1                                     # a signalling NaN with the smallest payload
    pos = ((np.arange(256, dtype=np.uint32) << 23)[:, None] | mant).ravel()
    return np.concatenate([pos, pos | np.uint32(0x80000000)])


def trig_borders():
    """+-8192 and every octant border j * pi/4 (where cm_trig_reduce's j changes), each with its +-8 ulp neighbours."""
    j = np.arange(1, TRIG_OCTANTS + 1, dtype=np.float64)
    return neighbours(np.concatenate([[TRIG_MAX], j * (np.pi / 4)]), both_signs=True)


def integer_borders():
    """Where floor, round and the two integer conversions can go wrong: +-2^31 and 2^32 with their neighbours, halves and
    integers up to where floats have no fraction bits left, -0.5, 0.99999994, NaN, +-inf."""
    small = np.arange(1, 65, dtype=np.float64)
    v = np.concatenate([[2.0 ** 31, 2.0 ** 32, 2.0 ** 23, 2.0 ** 24, 2.0 ** 22, 2.0 ** 30, 2.0 ** 63, 2.0 ** 64, 0.5, 0.99999994, 1e-4],
                        small, small + 0.5, 2.0 ** 23 - small, 2.0 ** 22 + small + 0.5])
    extra = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7f800000, 0xff800000, 0, 0x80000000, 1, 0x80000001], np.uint32)
    return np.concatenate([neighbours(v, both_signs=True), bits(np.array([-0.5, 0.99999994, 0.5, -0.99999994], np.float32)), extra])


def branch_points(op):
    """The +-8 ulp neighbours of every branch constant of `op` in the header (words; empty where it has none)."""
    if op == 'log':
        # m < 0.70710678 is tested on the mantissa: in every binade, subnormal ones (scaled by 2^23 first) included
        k = np.arange(-140, 128)
        return np.concatenate([neighbours(np.ldexp(np.float64(np.float32(0.70710678118654752440)), k)), neighbours([1.0]),
                               np.arange(FLT_MIN_BITS - 8, FLT_MIN_BITS + 9, dtype=np.uint32)])
    if op == 'exp':
        k = np.arange(-126, 129, dtype=np.float64)
        ties = np.concatenate([(k - 0.5) / LOG2E, (k + 0.5) / LOG2E])       # x * log2e = k +- 0.5: where n = round(...) steps
        return neighbours(np.concatenate([[EXP_HI, EXP_LO], ties]))
    if op in ('sin', 'cos'):
        return trig_borders()
    if op == 'tan':
        return np.concatenate([trig_borders(), neighbours([1e-4], both_signs=True)])
    if op == 'asin':
        return neighbours([1e-4, 0.5, 1.0], both_signs=True)
    if op == 'acos':
        return neighbours([0.5, 1.0], both_signs=True)
    if op == 'atan':
        return neighbours([0.4142135623730950, 2.414213562373095], both_signs=True)
    if op in ('floor', 'round', 'f2i', 'f2u32'):
        return integer_borders()
    return np.zeros(0, np.uint32)


def unary_inputs(op, rng):
    return np.concatenate([unary_grid(rng), branch_points(op)]).astype(np.uint32)


UNIFORM_WORDS = [0, 1, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, 0x7fffffff, 0x80000000, 0xffffff7f, 0xffffff80, 0xffffff81, 0xffffffff]


def uniform_inputs(rng, nrand=1 << 21):
    return np.concatenate([np.array(UNIFORM_WORDS, np.uint32), rng.integers(0, 1 << 32, nrand, dtype=np.uint32)])


# +-0, +-denorm (the smallest and the largest), +-1, +-FLT_MAX, +-inf, a quiet and a signalling NaN
SPECIALS = np.array([0, 0x80000000, 1, 0x80000001, 0x007fffff, 0x807fffff, 0x3f800000, 0xbf800000, FLT_MAX_BITS, 0xff7fffff,
                     0x7f800000, 0xff800000, 0x7fc00000, 0x7f800001], np.uint32)


def binary_inputs(rng, nrand=1 << 19):
    """(x words, y words): the full cross product of SPECIALS with itself, a grid over ALL exponent pairs (0..255 each) in
    all four sign pairs with six mantissa pairs, random bit patterns, and normal deviates (ordinary magnitudes)."""
    sx, sy = [a.ravel() for a in np.meshgrid(SPECIALS, SPECIALS, indexing='ij')]
    ex, ey = [a.ravel() for a in np.meshgrid(np.arange(256, dtype=np.uint32) << 23, np.arange(256, dtype=np.uint32) << 23, indexing='ij')]
    gx, gy = [], []
    for signs in ((0, 0), (0x80000000, 0), (0, 0x80000000), (0x80000000, 0x80000000)):
        for mants in ((0, 0), (0x7fffff, 0), (0, 0x7fffff), (0x400000, 0x2aaaaa), None, None):
            mx, my = rng.integers(0, 1 << 23, (2, len(ex)), dtype=np.uint32) if mants is None else np.array(mants, np.uint32)
            gx.append(ex | np.uint32(signs[0]) | mx)
            gy.append(ey | np.uint32(signs[1]) | my)
    rx, ry = rng.integers(0, 1 << 32, (2, nrand), dtype=np.uint32)
    nx, ny = bits(rng.normal(size=(2, nrand // 2)).astype(np.float32))
    x = np.concatenate([sx] + gx + [rx, nx, nx])          # (the last pair: equal operands, for fmin / fmax / a quotient of 1)
    y = np.concatenate([sy] + gy + [ry, ny, nx])
    return x.astype(np.uint32), y.astype(np.uint32)


def ternary_inputs(rng, nrand=1 << 20):
    """(x, y, z words) for fma: the cube of SPECIALS, random bit patterns, and products that cancel against z to within a
    few ulp (where a fused and an unfused multiply-add differ most)."""
    sx, sy, sz = [a.ravel() for a in np.meshgrid(SPECIALS, SPECIALS, SPECIALS, indexing='ij')]
    rx, ry, rz = rng.integers(0, 1 << 32, (3, nrand), dtype=np.uint32)
    a, b = rng.normal(size=(2, nrand)).astype(np.float32)
    c = bits(-(a * b)) + rng.integers(-4, 5, nrand).astype(np.uint32)
    return (np.concatenate([sx, rx, bits(a)]).astype(np.uint32), np.concatenate([sy, ry, bits(b)]).astype(np.uint32),
            np.concatenate([sz, rz, c]).astype(np.uint32))


def ulp_err(got, ref64):
    """|got - ref| in units of the spacing of floats at ref (the measure tests/test_math_contract.py has always used)."""
    ref32 = ref64.astype(np.float32)
    ulp = np.spacing(np.abs(ref32)).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref64) / np.maximum(ulp, 1e-45)


def float64_error(op, xw, got, yw=None):
    """The worst error of `got` (float32 results for the input words `xw`) against float64 libm over the inputs that lie
    in op's declared domain, in the measure the contract states for op: (measure, worst, x at the worst, points measured);
    None for an op without an approximation error."""
    with np.errstate(all='ignore'):
        x = f32(xw).astype(np.float64)
        g = np.asarray(got, np.float32)
        if op == 'log':
            sel, ref, kind = (x > 0) & np.isfinite(x), np.log(x), 'ulp'
        elif op == 'exp':
            ref = np.exp(x)
            sel, kind = (x >= np.float32(EXP_LO)) & (x <= np.float32(EXP_HI)) & (ref >= 2.0 ** -126) & (ref < 2.0 ** 128 * (1 - 2.0 ** -25)), 'ulp'
        elif op in ('sin', 'cos'):
            sel, ref, kind = np.abs(x) <= TRIG_MAX, (np.sin if op == 'sin' else np.cos)(x), 'abs'
        elif op == 'tan':
            sel, ref, kind = np.abs(x) <= TRIG_MAX, np.tan(x), 'angle'
        elif op in ('asin', 'acos'):
            sel, ref, kind = np.abs(x) <= 1.0, (np.arcsin if op == 'asin' else np.arccos)(x), 'ulp'
        elif op == 'atan':
            sel, ref, kind = np.isfinite(x), np.arctan(x), 'ulp'
        elif op == 'atan2':
            y = f32(yw).astype(np.float64)
            sel, ref, kind = ~(np.isnan(x) | np.isnan(y)), np.arctan2(x, y), 'abs'
        else:
            return None
        sel = np.flatnonzero(sel)
        g, ref = g[sel], ref[sel]
        if kind == 'ulp':
            e = ulp_err(g, ref)
        elif kind == 'abs':
            e = np.abs(g.astype(np.float64) - ref)
        else:
            e = np.abs(g.astype(np.float64) - ref) / (1.0 + ref * ref)
        k = int(np.argmax(e))
        return kind, float(e[k]), float(x[sel[k]]), len(sel)


PHILOX_KAT = [     # Random123 kat_vectors, philox4x32 with 10 rounds: (counter, key, expected)
    ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def philox_inputs(rng, nrand=1 << 18):
    """[n][6] words: the three known-answer inputs first, then random counters and keys."""
    kat = np.array([c + k for c, k, _ in PHILOX_KAT], np.uint32)
    return np.concatenate([kat, rng.integers(0, 1 << 32, (nrand, 6), dtype=np.uint32)])


STREAM_STARTS = [0, 1, 2, 3, 4, 0xfffffffc, 0xfffffffd, 0xfffffffe, 0xffffffff]


def stream_inputs(rng, nseeds=64):
    """[n][6] words (seed lo, seed hi, id lo, id hi, stream, start): photon ids below and above 2^32, streams 0, 1 and
    0xffffffff, and the start counters at which the 8 uniforms (or a normal's pair of them) cross a Philox block border
    and the wrap of the 32-bit counter; random seeds, and a block of wholly random words."""
    ids = [0, 1, 77, 0xffffffff, 1 << 32, (1 << 32) + 1, 0xB0B0000000000000 + 5, (1 << 64) - 1]
    rows = []
    for seed in [0, 12345, (1 << 64) - 1] + [int(s) for s in rng.integers(0, 1 << 63, nseeds, dtype=np.uint64)]:
        for pid in ids:
            for stream in (0, 1, 0xffffffff):
                for start in STREAM_STARTS:
                    rows.append([seed & 0xffffffff, seed >> 32, pid & 0xffffffff, pid >> 32, stream, start])
    return np.concatenate([np.array(rows, np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, (1 << 15, 6), dtype=np.uint32)])
