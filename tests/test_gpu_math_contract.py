"""The numeric contract ON THE DEVICE, primitive by primitive: include/chroma_math.h as hipcc compiles it for gfx950
(chroma_probe_math, csrc/kernels_probe_math.h: one call per element, the op a kernel argument) against the same header as
the host compiler compiles it for the CPU oracle (oracle_math3 / oracle_rng_probe, the `contract` build).

For each op: ONE input array, one device call, one oracle call, and bits(device) == bits(oracle) for EVERY element.  Two
NaNs count as equal (the project's rule elsewhere: a NaN's payload is not part of the contract); there is no other
tolerance and no element is left out.  The inputs are built by construction (tests/contract_inputs.py): every exponent
field 0..255 with the all-zeros, all-ones, 0x400000 and 4093 random mantissas in both signs (+-0, the smallest and the
largest subnormal, +-FLT_MIN, +-FLT_MAX, +-inf, quiet and signalling NaNs), the +-8 ulp neighbours of every branch constant
of the header, and for the two- and three-operand ops the cross product of the special values, all exponent pairs and
random words.

Why the whole-history tests (test_gpu_parity.py, test_gpu_ref_physics.py, the DAQ and step-light tests) are not made
redundant by this, nor this by them: they see the contract only at the arguments the demo geometries visit, and report a
difference as "3 of 20000 photons differ"; this file names the primitive and the input.  And what it shows carries over:
the probe shows the header as compiled into the probe kernel, but with contraction off and no fast math every statement
of the header is a single IEEE operation, so the copy inlined into k_physics cannot differ from the one probed here.

Elements per op (the counts the assertions cover) and the device's worst errors against float64 libm over exactly these
inputs, within each function's declared domain -- measured on an MI355X, printed by the tests (pytest -s), and, the
device agreeing with the host bit for bit, equal to the host's on the same inputs:

    op            elements    worst error of the device against float64 (where; inputs in the domain)
    log           2 101 742   0.748 ulp            (at 1.41421294;   1 049 069)
    exp           2 105 856   0.996 ulp            (at -38.4696465;  1 101 264, results >= FLT_MIN)
    sin           2 451 840   7.65e-8 absolute     (at 6536.86523;   1 501 520 in [-8192, 8192])
    cos           2 451 840   7.82e-8 absolute     (at 1698.81677;   1 501 520)
    tan           2 451 874   9.10e-8 as an angle, |t - ref| / (1 + ref^2)   (at 834.877808; 1 501 554)
    asin          2 097 254   2.10 ulp             (at 0.524892807;  1 040 472 in [-1, 1])
    acos          2 097 220   1.21 ulp             (at -0.5159747;   1 040 438)
    atan          2 097 220   2.61 ulp             (at 0.453195065;  2 089 028 finite)
    atan2         2 621 636   2.68e-7 absolute     (at y = 2.13585615; 2 609 211 without a NaN operand)
    sqrt          2 097 152   exact (one IEEE operation), as are floor and round (2 106 243 each), f2i and f2u32
    div, fmin, fmax   2 621 636 each     fma   2 099 896     u32_to_uniform   2 097 163 words
    philox        262 147 counters (1 048 588 words)     rng_uniform  47 240 streams x 8 draws     rng_normal  47 240 x 4

The whole file takes 1.5 s on the device machine.
"""
import numpy as np
import pytest

import contract_inputs as ci

pytestmark = pytest.mark.gpu

UNARY = ['log', 'exp', 'sin', 'cos', 'tan', 'asin', 'acos', 'atan', 'sqrt', 'floor', 'round', 'f2i', 'f2u32']
BINARY = ['atan2', 'div', 'fmin', 'fmax']
INTEGER_RESULT = ('f2i', 'f2u32', 'philox')            # their words are integers: no two of them are "both NaN"


def device_math(op, x, y=None, z=None):
    """chroma_probe_math on word arrays; the output is pre-filled so that an element the kernel skipped cannot pass."""
    from chroma_amd import gpu, _lib
    from chroma_amd.gpu.tools import to_gpu, GPUArray
    import oracle
    ctx = gpu.get_context()
    x = np.ascontiguousarray(x, np.uint32)
    width_in = 6 if op in oracle.RNG_PROBE_WIDTH else 1
    n = x.size // width_in
    dev = [None if a is None else to_gpu(np.ascontiguousarray(a, np.uint32).reshape(-1), ctx) for a in (x, y, z)]
    out = GPUArray(n * oracle.RNG_PROBE_WIDTH.get(op, 1), np.uint32, ctx).fill(0xA5A5A5A5)
    _lib.check(ctx._lib.chroma_probe_math(ctx.handle, oracle.MATH_OPS[op], n, *[None if d is None else d.ptr for d in dev], out.ptr))
    return out.get()


def oracle_math(oracle_mod, op, x, y=None, z=None):
    if op in oracle_mod.RNG_PROBE_WIDTH:
        return oracle_mod.rng_probe(op, x).view(np.uint32).reshape(-1)
    return ci.bits(oracle_mod.math_fn(op, ci.f32(x), None if y is None else ci.f32(y), None if z is None else ci.f32(z)))


def assert_same_bits(op, dev, orc, *inputs):
    """bits(device) == bits(oracle) everywhere, two NaNs equal; on failure: the op, how many differ, the first input in hex
    with both outputs."""
    assert dev.shape == orc.shape and dev.dtype == orc.dtype == np.uint32
    same = dev == orc
    if op not in INTEGER_RESULT:
        isnan = lambda w: (w & 0x7fffffff) > 0x7f800000
        same |= isnan(dev) & isnan(orc)
    if same.all():
        return
    bad = np.flatnonzero(~same)
    k = int(bad[0])
    width = dev.size // (inputs[0].size // (6 if inputs[0].ndim == 2 else 1))
    row = k // width
    shown = ' '.join('%08x' % w for a in inputs for w in np.atleast_1d(a[row]))
    pytest.fail('%s: %d of %d elements differ between device and oracle; first at element %d (output word %d): input %s -> device %08x, oracle %08x'
                % (op, len(bad), dev.size, row, k % width, shown, dev[k], orc[k]))


def report(op, x, dev, y=None):
    err = ci.float64_error(op, x, ci.f32(dev), y)
    if err is None:
        print('%-12s %9d elements' % (op, dev.size))
    else:
        print('%-12s %9d elements   %.3g %s at %.9g (%d in the domain)' % (op, dev.size, err[1], err[0], err[2], err[3]))


@pytest.mark.parametrize('op', UNARY)
def test_unary_op_device_equals_host(oracle_mod, op):
    x = ci.unary_inputs(op, np.random.default_rng(100 + UNARY.index(op)))
    assert x.size >= 2 * 256 * 4096
    dev = device_math(op, x)
    assert_same_bits(op, dev, oracle_math(oracle_mod, op, x), x)
    report(op, x, dev)


def test_u32_to_uniform_device_equals_host(oracle_mod):
    x = ci.uniform_inputs(np.random.default_rng(120))
    dev = device_math('uniform', x)
    assert_same_bits('uniform', dev, oracle_math(oracle_mod, 'uniform', x), x)
    u = ci.f32(dev)
    assert (u > 0.0).all() and (u <= 1.0).all()                   # curand_uniform's (0, 1]
    assert u[ci.UNIFORM_WORDS.index(0xffffffff)] == 1.0 and u[ci.UNIFORM_WORDS.index(0xffffff80)] == 1.0     # (ties to even, up)
    assert u[ci.UNIFORM_WORDS.index(0xffffff7f)] < 1.0
    report('uniform', x, dev)


@pytest.mark.parametrize('op', BINARY)
def test_binary_op_device_equals_host(oracle_mod, op):
    x, y = ci.binary_inputs(np.random.default_rng(130 + BINARY.index(op)))
    assert x.size >= 14 * 14 + 4 * 6 * 65536
    dev = device_math(op, x, y)
    assert_same_bits(op, dev, oracle_math(oracle_mod, op, x, y), x, y)
    report(op, x, dev, y)


def test_fma_device_equals_host(oracle_mod):
    x, y, z = ci.ternary_inputs(np.random.default_rng(140))
    dev = device_math('fma', x, y, z)
    assert_same_bits('fma', dev, oracle_math(oracle_mod, 'fma', x, y, z), x, y, z)
    report('fma', x, dev)


def test_philox_device_equals_host_and_the_known_answers(oracle_mod):
    w = ci.philox_inputs(np.random.default_rng(150))
    dev = device_math('philox', w)
    for k, (_, _, expect) in enumerate(ci.PHILOX_KAT):             # Random123's kat_vectors, on the device
        assert dev[4 * k:4 * k + 4].tolist() == expect
    assert_same_bits('philox', dev, oracle_math(oracle_mod, 'philox', w), w)
    report('philox', w, dev)


@pytest.mark.parametrize('op', ['rng_uniform', 'rng_normal'])
def test_rng_stream_device_equals_host(oracle_mod, op):
    """Ids below and above 2^32, streams 0, 1 and 0xffffffff, starts at which a draw (or the pair of draws of a normal)
    crosses a Philox block border and the wrap of the draw counter."""
    w = ci.stream_inputs(np.random.default_rng(160))
    dev = device_math(op, w)
    orc = oracle_math(oracle_mod, op, w)
    assert_same_bits(op, dev, orc, w)
    if op == 'rng_uniform':
        # the stream word and the high id word are in the key of the draws: the probe is not the stream-0 probe in disguise
        row = lambda seed, pid, stream, start: np.array([[seed & 0xffffffff, seed >> 32, pid & 0xffffffff, pid >> 32, stream, start]], np.uint32)
        base = device_math(op, row(12345, 77, 0, 0))
        assert np.array_equal(ci.f32(base), oracle_mod.uniform_stream(12345, 77, 8))
        assert not np.array_equal(base, device_math(op, row(12345, 77, 1, 0)))
        assert not np.array_equal(base, device_math(op, row(12345, 77 + (1 << 32), 0, 0)))
        assert np.array_equal(base[4:], device_math(op, row(12345, 77, 0, 4))[:4])
    report(op, w, dev)


def test_probe_kernels_compile_the_header_alike_and_repeat(oracle_mod):
    """cm_sinf / cm_cosf through chroma_probe_math equal columns 4 and 3 of the `rotate` probe (chroma_probe fn 3, k_probe:
    another kernel, the same header) for the same angles; and a second run of a probe gives the same bits."""
    from chroma_amd import gpu, _lib
    from chroma_amd.gpu.tools import to_gpu, GPUArray
    ctx = gpu.get_context()

    def engine_probe_rotate(x):
        d_x, out = to_gpu(x.reshape(-1), ctx), GPUArray(5 * len(x), np.float32, ctx)
        _lib.check(ctx._lib.chroma_probe(ctx.handle, 3, len(x), d_x.ptr, None, None, 0, 0.0, 1.0, out.ptr))
        return out.get().reshape(len(x), 5)

    rng = np.random.default_rng(170)
    phi = np.concatenate([rng.uniform(-np.pi, np.pi, 100000), rng.uniform(-8192, 8192, 100000),
                          ci.f32(ci.trig_borders()[::7]), [0.0, -0.0, 1e-4, -1e-4, 8192.0, -8192.0, 8193.0, np.inf, np.nan]]).astype(np.float32)
    n = len(phi)
    a = np.tile(np.array([0.6, 0.0, 0.8], np.float32), (n, 1))
    axis = np.tile(np.array([0.0, 1.0, 0.0], np.float32), (n, 1))
    rot = engine_probe_rotate(np.ascontiguousarray(np.column_stack([a, phi, axis]), np.float32))
    sin, cos = device_math('sin', ci.bits(phi)), device_math('cos', ci.bits(phi))
    assert_same_bits('cos (rotate probe)', cos, ci.bits(rot[:, 3]), ci.bits(phi))
    assert_same_bits('sin (rotate probe)', sin, ci.bits(rot[:, 4]), ci.bits(phi))
    # the same bits on a second run, NaN payloads included
    assert np.array_equal(sin, device_math('sin', ci.bits(phi)))
    x = ci.unary_inputs('tan', np.random.default_rng(171))
    assert np.array_equal(device_math('tan', x), device_math('tan', x))
    w = ci.stream_inputs(np.random.default_rng(172))
    assert np.array_equal(device_math('rng_normal', w), device_math('rng_normal', w))


def test_bad_arguments_are_refused():
    from chroma_amd import gpu, _lib
    from chroma_amd.gpu.tools import to_gpu
    ctx = gpu.get_context()
    d = to_gpu(np.zeros(8, np.uint32), ctx)
    call = lambda op, x, y, z, out: ctx._lib.chroma_probe_math(ctx.handle, op, 8, x, y, z, out)
    assert call(-1, d.ptr, None, None, d.ptr) != 0 and call(22, d.ptr, None, None, d.ptr) != 0
    assert call(0, None, None, None, d.ptr) != 0 and call(0, d.ptr, None, None, None) != 0
    assert call(7, d.ptr, None, None, d.ptr) != 0 and call(18, d.ptr, d.ptr, None, d.ptr) != 0
    assert ctx._lib.chroma_probe_math(ctx.handle, 0, 1 << 31, d.ptr, None, None, d.ptr) != 0
    assert ctx._lib.chroma_probe_math(ctx.handle, 0, 0, d.ptr, None, None, d.ptr) == 0
