"""Python access to the CPU oracle (oracle/chroma_oracle.c) -- TEST INFRASTRUCTURE.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this
package.  It is the checker, never the thing measured or shipped: nothing under
chroma_amd/ imports it.

``variant='contract'`` loads the build whose transcendental functions come from
include/chroma_math.h (bit-exact comparand of the HIP engine); ``variant='libm'`` the
build against the host libm (independent check that the physics does not hinge on the
contract's polynomials).
"""
import ctypes
import os
import subprocess
from ctypes import POINTER, c_float, c_int32, c_uint32, c_uint64, c_void_p

import numpy as np

from chroma_amd import _lib as _abi        # only for the ctypes Structure definitions of the C ABI
from chroma_amd import event

_HERE = os.path.dirname(os.path.abspath(__file__))
_libs = {}


REF_PHYSICS_LIBS = {'contract': 'libchroma_ref_physics_contract.so', 'libm': 'libchroma_ref_physics_libm.so'}


def ref_physics_path(variant='contract'):
    return os.path.join(_HERE, '_ref', REF_PHYSICS_LIBS[variant])


def have_ref_physics():
    return all(os.path.exists(ref_physics_path(v)) for v in REF_PHYSICS_LIBS)


def ref_pdf_path():
    return os.path.join(_HERE, '_ref', 'libchroma_ref_pdf.so')


def have_ref_pdf():
    return os.path.exists(ref_pdf_path())


def build(force=False):
    """Compile liboracle.so / liboracle_libm.so (and oracle/_ref when the reference is present).  The host builds of
    the reference's physics (oracle/_ref/libchroma_ref_physics_*.so) and of its PDF kernels (libchroma_ref_pdf.so) are
    made on their own when only they are missing: the Makefile's `ref-physics` and `ref-pdf` targets compile them if
    the reference tree is there and say so if it is not."""
    have = all(os.path.exists(os.path.join(_HERE, n)) for n in ('liboracle.so', 'liboracle_libm.so'))
    if have and not force:
        if not have_ref_physics():
            subprocess.check_call(['make', '-C', _HERE, 'ref-physics'], stdout=subprocess.DEVNULL)
        if not have_ref_pdf():
            subprocess.check_call(['make', '-C', _HERE, 'ref-pdf'], stdout=subprocess.DEVNULL)
        return
    subprocess.check_call(['make', '-C', _HERE, 'all'], stdout=subprocess.DEVNULL)


_SINGLE_ARGTYPES = [POINTER(_abi.GeometryDesc), POINTER(_abi.PhotonArrays), _abi.Rng, c_int32,
                    POINTER(c_float), c_float, c_float, c_float, c_float, c_int32, c_int32, c_float,
                    c_int32, c_int32]
_RUN_DAQ_ARGTYPES = [POINTER(_abi.GeometryDesc), POINTER(_abi.DaqTables), c_int32, c_int32, c_uint32,
                     POINTER(_abi.PhotonArrays), _abi.Rng, c_uint32, c_float, c_void_p, c_void_p, c_void_p]
_RUN_DAQ_MANY_ARGTYPES = [POINTER(_abi.GeometryDesc), POINTER(_abi.DaqTables), c_int32, c_int32, c_uint32,
                          POINTER(_abi.PhotonArrays), _abi.Rng, c_uint32, c_float, c_int32, c_int32,
                          c_void_p, c_void_p, c_void_p]


def load(variant='contract'):
    if variant in _libs:
        return _libs[variant]
    name = {'contract': 'liboracle.so', 'libm': 'liboracle_libm.so'}[variant]
    path = os.path.join(_HERE, name)
    if variant == 'contract' and os.environ.get('CHROMA_ORACLE_LIBRARY'):       # (a sanitizer build: tools/asan_host.sh)
        path = os.environ['CHROMA_ORACLE_LIBRARY']
    if not os.path.exists(path):
        build()
    lib = ctypes.CDLL(path)
    lib.oracle_variant.restype = ctypes.c_char_p
    assert lib.oracle_variant().decode() == variant
    lib.oracle_propagate.restype = c_int32
    lib.oracle_propagate.argtypes = [POINTER(_abi.GeometryDesc), POINTER(_abi.PhotonArrays), c_uint64, _abi.Rng,
                                     c_int32, c_int32, c_int32, c_int32, POINTER(_abi.PropagateStats)]
    lib.oracle_to_diffuse.restype = c_int32
    lib.oracle_to_diffuse.argtypes = [POINTER(_abi.GeometryDesc), POINTER(_abi.PhotonArrays), c_uint64, _abi.Rng, c_int32, c_void_p,
                                      c_void_p, POINTER(_abi.PropagateStats)]
    lib.oracle_distance_to_mesh.restype = c_int32
    lib.oracle_distance_to_mesh.argtypes = [POINTER(_abi.GeometryDesc), c_uint64, c_void_p, c_void_p, c_void_p, c_void_p,
                                            POINTER(_abi.PropagateStats)]
    lib.oracle_generate_bomb.restype = c_int32
    lib.oracle_generate_bomb.argtypes = [POINTER(_abi.PhotonArrays), c_uint64, c_uint64, c_uint64, POINTER(c_float),
                                         c_float, c_float]
    lib.oracle_run_daq.restype = c_int32
    lib.oracle_run_daq.argtypes = _RUN_DAQ_ARGTYPES
    lib.oracle_run_daq_many.restype = c_int32
    lib.oracle_run_daq_many.argtypes = _RUN_DAQ_MANY_ARGTYPES
    lib.oracle_math.restype = c_int32
    lib.oracle_math.argtypes = [c_int32, c_uint64, c_void_p, c_void_p, c_void_p]
    lib.oracle_philox.restype = None
    lib.oracle_philox.argtypes = [c_void_p, c_void_p, c_void_p]
    lib.oracle_uniform_stream.restype = None
    lib.oracle_uniform_stream.argtypes = [c_uint64, c_uint64, c_uint32, c_uint32, c_void_p]
    lib.oracle_single.restype = c_int32
    lib.oracle_single.argtypes = _SINGLE_ARGTYPES
    _libs[variant] = lib
    return lib


_ref_libs = {}


def load_ref_physics(variant='contract'):
    """The reference's OWN physics and DAQ sources compiled for the host (oracle/ref_physics_driver.cc) -- only what
    oracle/_ref holds is loaded, the reference tree itself is never read here.  None when the library is not there."""
    if variant in _ref_libs:
        return _ref_libs[variant]
    path = ref_physics_path(variant)
    if not os.path.exists(path):
        return None
    lib = ctypes.CDLL(path)
    lib.ref_phys_variant.restype = ctypes.c_char_p
    assert lib.ref_phys_variant().decode() == variant
    lib.ref_phys_propagate.restype = c_int32
    lib.ref_phys_propagate.argtypes = [POINTER(_abi.GeometryDesc), POINTER(_abi.PhotonArrays), c_uint64, _abi.Rng,
                                       c_int32, c_int32, c_int32, POINTER(c_uint64)]
    lib.ref_phys_single.restype = c_int32
    lib.ref_phys_single.argtypes = _SINGLE_ARGTYPES
    lib.ref_phys_run_daq.restype = c_int32
    lib.ref_phys_run_daq.argtypes = _RUN_DAQ_ARGTYPES
    lib.ref_phys_run_daq_many.restype = c_int32
    lib.ref_phys_run_daq_many.argtypes = _RUN_DAQ_MANY_ARGTYPES
    if hasattr(lib, 'ref_hybrid_lookup'):                    # (a library built before the hybrid render was added has none)
        lib.ref_hybrid_lookup.restype = c_int32
        lib.ref_hybrid_lookup.argtypes = [POINTER(_abi.GeometryDesc), c_int32, c_int32, c_int32, POINTER(c_float), _abi.Rng, c_void_p,
                                          c_float, POINTER(c_float), c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]
        lib.ref_hybrid_image.restype = c_int32
        lib.ref_hybrid_image.argtypes = [POINTER(_abi.GeometryDesc), c_int32, _abi.Rng, c_void_p, c_void_p, c_void_p, c_float,
                                         POINTER(c_float), c_void_p, c_void_p, c_void_p, c_int32, c_int32]
        lib.ref_hybrid_pixels.restype = c_int32
        lib.ref_hybrid_pixels.argtypes = [c_int32, c_void_p, c_void_p, c_int32]
    _ref_libs[variant] = lib
    return lib


REF_HYBRID_ENTRIES = ('ref_hybrid_lookup', 'ref_hybrid_image', 'ref_hybrid_pixels')


def have_ref_hybrid():
    """True when both physics libraries of oracle/_ref hold the reference's hybrid render (chroma/cuda/hybrid_render.cu
    behind the three entries of oracle/ref_physics_driver.cc); libraries built before it was added do not."""
    if not have_ref_physics():
        return False
    libs = [load_ref_physics(v) for v in REF_PHYSICS_LIBS]
    return all(lib is not None and all(hasattr(lib, name) for name in REF_HYBRID_ENTRIES) for lib in libs)


def _f3(v):
    return (c_float * 3)(*[float(x) for x in v])


def ref_hybrid_lookup(packed, seed, id_base, counters, nthreads, total_threads, offset, source, wavelength, xyz, lookup1, lookup2,
                      max_steps=10, variant='contract'):
    """ONE update_xyz_lookup launch of the reference (hybrid_render.cu:63-131) over ``nthreads`` threads, thread k on the stream
    ``id_base + k`` at ``counters[k]``, added onto copies of ``lookup1`` / ``lookup2`` ([ntriangles][3] float32).  Returns
    (lookup1, lookup2, counters, (triangle, side, value)): the tables and the counters after the launch, and thread k's own
    addition -- the row, the table (side 1: lookup1, side 0: lookup2) and the three values it handed to fAtomicAdd, triangle -1
    and zeros where it added nothing."""
    lib = load_ref_physics(variant)
    ntri = int(packed.desc.ntriangles)
    l1, l2 = [np.array(a, dtype=np.float32, order='C', copy=True).reshape(ntri, 3) for a in (lookup1, lookup2)]
    n = max(int(nthreads), 0)
    ctr = np.array(counters, dtype=np.uint32, order='C', copy=True)
    assert len(ctr) >= n
    tri = np.full(n, -1, np.int32)
    side = np.zeros(n, np.uint32)
    value = np.zeros((n, 3), np.float32)
    rc = lib.ref_hybrid_lookup(ctypes.byref(packed.desc), int(nthreads), int(total_threads), int(offset), _f3(source),
                               _abi.Rng(int(seed), int(id_base)), ctr.ctypes.data, float(wavelength), _f3(xyz), l1.ctypes.data,
                               l2.ctypes.data, int(max_steps), tri.ctypes.data, side.ctypes.data, value.ctypes.data)
    if rc != 0:
        raise RuntimeError('ref_hybrid_lookup failed (%d)' % rc)
    return l1, l2, ctr, (tri, side, value)


def ref_hybrid_image(packed, seed, id_base, counters, origins, directions, wavelength, xyz, lookup1, lookup2, image, nlookup_calls,
                     max_steps=10, variant='contract'):
    """ONE update_xyz_image launch of the reference (hybrid_render.cu:133-168) over the rays given, added onto a copy of
    ``image`` ([nrays][3] float32).  Returns (image, counters) after the launch."""
    lib = load_ref_physics(variant)
    ntri = int(packed.desc.ntriangles)
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    n = len(o)
    l1, l2 = [np.ascontiguousarray(a, dtype=np.float32).reshape(ntri, 3) for a in (lookup1, lookup2)]
    img = np.array(image, dtype=np.float32, order='C', copy=True).reshape(-1, 3)
    ctr = np.array(counters, dtype=np.uint32, order='C', copy=True)
    assert len(d) == n and len(img) >= n and len(ctr) >= n
    rc = lib.ref_hybrid_image(ctypes.byref(packed.desc), n, _abi.Rng(int(seed), int(id_base)), ctr.ctypes.data, o.ctypes.data,
                              d.ctypes.data, float(wavelength), _f3(xyz), l1.ctypes.data, l2.ctypes.data, img.ctypes.data,
                              int(nlookup_calls), int(max_steps))
    if rc != 0:
        raise RuntimeError('ref_hybrid_image failed (%d)' % rc)
    return img, ctr


def ref_hybrid_pixels(image, nimages, variant='contract'):
    """process_image of the reference (hybrid_render.cu:170-200) on ``image`` ([n][3] float32).  Returns (pixels, left_out):
    ``left_out`` [n][3] marks the channels that are NaN after the division by ``nimages``.  The reference converts
    floorf(NaN) to unsigned, which a host build leaves undefined (the device gives 0), so those channels -- and only those --
    are handed to it as 0.0 and their eight bits of ``pixels`` mean nothing."""
    lib = load_ref_physics(variant)
    img = np.array(image, dtype=np.float32, order='C', copy=True).reshape(-1, 3)
    with np.errstate(invalid='ignore', over='ignore'):
        left_out = np.isnan(img / np.float32(nimages))
    img[left_out] = 0.0
    pixels = np.zeros(len(img), np.uint32)
    rc = lib.ref_hybrid_pixels(len(img), img.ctypes.data, pixels.ctypes.data, int(nimages))
    if rc != 0:
        raise RuntimeError('ref_hybrid_pixels failed (%d)' % rc)
    return pixels, left_out


def load_ref_pdf():
    """The reference's OWN PDF kernels compiled for the host (oracle/ref_pdf_driver.cc over chroma/cuda/pdf.cu), against
    the host libm.  Only what oracle/_ref holds is loaded; None when the library is not there."""
    if 'pdf' in _ref_libs:
        return _ref_libs['pdf']
    if not have_ref_pdf():
        return None
    lib = ctypes.CDLL(ref_pdf_path())
    lib.ref_pdf_variant.restype = ctypes.c_char_p
    assert lib.ref_pdf_variant().decode() == 'libm'
    lib.ref_pdf_table_size.restype = c_int32
    lib.ref_pdf_table_size.argtypes = []
    lib.ref_pdf_bin_hits.restype = c_int32
    lib.ref_pdf_bin_hits.argtypes = [c_int32, c_int32, c_uint32, c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float,
                                     c_int32, c_float, c_float, c_void_p]
    lib.ref_pdf_eval_accumulate.restype = c_int32
    lib.ref_pdf_eval_accumulate.argtypes = [c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_float,
                                            c_float, c_float, c_int32, c_int32, c_void_p, c_void_p, c_void_p]
    lib.ref_pdf_moments.restype = c_int32
    lib.ref_pdf_moments.argtypes = [c_int32, c_int32, c_int32, c_uint32] + [c_void_p] * 2 + [c_float] * 4 + [c_void_p] * 5
    lib.ref_pdf_kernel_eval.restype = c_int32
    lib.ref_pdf_kernel_eval.argtypes = [c_int32, c_int32, c_int32, c_uint32] + [c_void_p] * 5 + [c_float] * 4 + [c_void_p] * 5
    _ref_libs['pdf'] = lib
    return lib


REF_PDF_TABLE_SIZE = 1000           # distance_table[1000] of accumulate_nearest_neighbor (pdf.cu:118)
REF_PDF_GUARD = 0xA5A5A5A5


def _channel_copies(a, ndaq, stride, nchannels, dtype=np.float32):
    """A C-contiguous float32 copy of a GPUChannels-layout array, long enough for ndaq copies of nchannels at stride."""
    a = np.array(a, dtype=dtype, order='C', copy=True)
    assert a.ndim == 1 and stride >= nchannels and len(a) >= (ndaq - 1) * stride + nchannels
    return a


def ref_bin_hits(t, q, nchannels, ndaq, stride, tbins, trange, qbins, qrange, hitcount=None, pdf=None):
    """bin_hits (pdf.cu:9-32), once per copy in copy order, with the argument list of tests/test_pdf_host.bin_hits_*.
    The histogram carries one guard row behind the last channel, which has to stay as it was: the reference writes the
    bin a time just below tmax rounds up to, row `tbins`, into the next channel's row.  Returns (hitcount, pdf)."""
    lib = load_ref_pdf()
    t, q = _channel_copies(t, ndaq, stride, nchannels), _channel_copies(q, ndaq, stride, nchannels)
    hitcount = np.zeros(nchannels, np.uint32) if hitcount is None else np.array(hitcount, np.uint32, copy=True)
    hist = np.full((nchannels + 1, tbins, qbins), REF_PDF_GUARD, np.uint32)
    hist[:nchannels] = 0 if pdf is None else np.asarray(pdf, np.uint32).reshape(nchannels, tbins, qbins)
    rc = lib.ref_pdf_bin_hits(nchannels, ndaq, stride, q.ctypes.data, t.ctypes.data, hitcount.ctypes.data, tbins,
                              float(trange[0]), float(trange[1]), qbins, float(qrange[0]), float(qrange[1]), hist.ctypes.data)
    if rc != 0:
        raise RuntimeError('ref_pdf_bin_hits refused its arguments (%d)' % rc)
    assert (hist[nchannels] == REF_PDF_GUARD).all(), 'the reference binned a hit behind its histogram'
    return hitcount, np.ascontiguousarray(hist[:nchannels])


def ref_eval_accumulate(event_hit, event_time, mc_time, nchannels, ndaq, stride, min_twidth, trange, k, state=None):
    """accumulate_bincount + accumulate_nearest_neighbor (pdf.cu:34-150) as chroma/gpu/pdf.py launches them, with the
    argument list of tests/test_pdf_host.eval_accumulate_*: state = (hitcount, bincount, nearest[nchannels, k]).  The
    copies are packed to stride nchannels for the call (the reference's own indexing).  ValueError, without a call,
    when k + ndaq exceeds the reference's distance table."""
    lib = load_ref_pdf()
    if k + ndaq > REF_PDF_TABLE_SIZE:
        raise ValueError('k + ndaq = %d exceeds the reference distance table of %d entries' % (k + ndaq, REF_PDF_TABLE_SIZE))
    assert lib.ref_pdf_table_size() == REF_PDF_TABLE_SIZE
    hit = np.ascontiguousarray(np.asarray(event_hit).astype(bool))
    mc = _channel_copies(mc_time, ndaq, stride, nchannels)
    packed = np.ascontiguousarray(np.stack([mc[i * stride:i * stride + nchannels] for i in range(ndaq)])).reshape(-1)
    if state is None:
        state = (np.zeros(nchannels, np.uint32), np.zeros(nchannels, np.uint32), np.full((nchannels, k), 1e9, np.float32))
    hitcount, bincount, nearest = (np.array(a, copy=True) for a in state)
    hit_to_channel = np.flatnonzero(hit).astype(np.uint32)
    channel_to_hit = np.maximum(0, hit.cumsum() - 1).astype(np.uint32)           # chroma/gpu/pdf.py:267
    nhit = len(hit_to_channel)
    by_hit = np.ascontiguousarray(nearest[hit_to_channel], dtype=np.float32).reshape(nhit, k)
    ev_hit = hit.astype(np.uint32)
    ev_time = np.ascontiguousarray(event_time, dtype=np.float32)
    rc = lib.ref_pdf_eval_accumulate(nchannels, ndaq, ev_hit.ctypes.data, ev_time.ctypes.data, packed.ctypes.data,
                                     hitcount.ctypes.data, bincount.ctypes.data, float(min_twidth), float(trange[0]),
                                     float(trange[1]), k, nhit, channel_to_hit.ctypes.data, hit_to_channel.ctypes.data,
                                     by_hit.ctypes.data)
    if rc != 0:
        raise RuntimeError('ref_pdf_eval_accumulate refused its arguments (%d)' % rc)
    nearest[hit_to_channel] = by_hit
    return hitcount, bincount, nearest


def ref_moments(t, q, nchannels, ndaq, stride, trange, qrange, time_only=True, state=None):
    """accumulate_moments (pdf.cu:223-265), once per copy in copy order; arguments of tests/test_pdf_host.moments_*."""
    lib = load_ref_pdf()
    t, q = _channel_copies(t, ndaq, stride, nchannels), _channel_copies(q, ndaq, stride, nchannels)
    if state is None:
        state = (np.zeros(nchannels, np.uint32),) + tuple(np.zeros(nchannels, np.float32) for _ in range(4))
    m0, t1, t2, q1, q2 = (np.array(a, copy=True) for a in state)
    rc = lib.ref_pdf_moments(int(bool(time_only)), nchannels, ndaq, stride, t.ctypes.data, q.ctypes.data, float(trange[0]),
                             float(trange[1]), float(qrange[0]), float(qrange[1]), m0.ctypes.data, t1.ctypes.data,
                             t2.ctypes.data, q1.ctypes.data, q2.ctypes.data)
    if rc != 0:
        raise RuntimeError('ref_pdf_moments refused its arguments (%d)' % rc)
    return m0, t1, t2, q1, q2


def ref_kernel_eval(event_hit, event_time, event_charge, t, q, nchannels, ndaq, stride, trange, qrange, inv_tbw, inv_qbw,
                    time_only=True, state=None):
    """accumulate_kernel_eval (pdf.cu:271-368), once per copy in copy order; arguments of
    tests/test_pdf_host.kernel_eval_*, but the state and the result are the reference's float32 sums:
    (hitcount, time_pdf_values, charge_pdf_values)."""
    lib = load_ref_pdf()
    t, q = _channel_copies(t, ndaq, stride, nchannels), _channel_copies(q, ndaq, stride, nchannels)
    if state is None:
        state = (np.zeros(nchannels, np.uint32), np.zeros(nchannels, np.float32), np.zeros(nchannels, np.float32))
    count, tv, qv = (np.array(a, dtype=d, copy=True) for a, d in zip(state, (np.uint32, np.float32, np.float32)))
    ev_hit = np.ascontiguousarray(np.asarray(event_hit).astype(bool).astype(np.uint32))
    ev_t, ev_q, itb, iqb = (np.ascontiguousarray(a, dtype=np.float32) for a in (event_time, event_charge, inv_tbw, inv_qbw))
    rc = lib.ref_pdf_kernel_eval(int(bool(time_only)), nchannels, ndaq, stride, ev_hit.ctypes.data, ev_t.ctypes.data,
                                 ev_q.ctypes.data, t.ctypes.data, q.ctypes.data, float(trange[0]), float(trange[1]),
                                 float(qrange[0]), float(qrange[1]), itb.ctypes.data, iqb.ctypes.data, count.ctypes.data,
                                 tv.ctypes.data, qv.ctypes.data)
    if rc != 0:
        raise RuntimeError('ref_pdf_kernel_eval refused its arguments (%d)' % rc)
    return count, tv, qv


class HostPhotons(object):
    """Writable host copies of the ten photon arrays + the ctypes struct pointing at them."""
    FIELDS = (('pos', np.float32), ('dir', np.float32), ('pol', np.float32), ('wavelengths', np.float32),
              ('t', np.float32), ('flags', np.uint32), ('last_hit_triangles', np.int32), ('weights', np.float32),
              ('evidx', np.uint32))

    def __init__(self, photons=None, n=None, rng_counters=None):
        if photons is not None:
            n = len(photons)
            for name, dtype in self.FIELDS:
                setattr(self, name, np.array(getattr(photons, name), dtype=dtype, order='C', copy=True))
        else:
            for name, dtype in self.FIELDS:
                shape = (n, 3) if name in ('pos', 'dir', 'pol') else (n,)
                setattr(self, name, np.zeros(shape, dtype=dtype))
        self.rng_counters = np.zeros(n, dtype=np.uint32) if rng_counters is None \
            else np.array(rng_counters, dtype=np.uint32, copy=True)
        self.n = n
        self.struct = _abi.PhotonArrays()
        for name, _ in self.FIELDS:
            setattr(self.struct, name, getattr(self, name).ctypes.data)
        self.struct.rng_counters = self.rng_counters.ctypes.data

    def photons(self):
        return event.Photons(self.pos, self.dir, self.pol, self.wavelengths, self.t, self.last_hit_triangles,
                             self.flags, self.weights, self.evidx)


def propagate(packed, photons, seed, photon_id_base=0, max_steps=10, use_weights=False, scatter_first=0,
              rng_counters=None, nthreads=1, variant='contract'):
    """Run the oracle on ``photons`` (event.Photons).  Returns (Photons, rng_counters, stats dict)."""
    lib = load(variant)
    hp = HostPhotons(photons, rng_counters=rng_counters)
    stats = _abi.PropagateStats()
    rc = lib.oracle_propagate(ctypes.byref(packed.desc), ctypes.byref(hp.struct), hp.n, _abi.Rng(int(seed), int(photon_id_base)),
                              int(max_steps), int(bool(use_weights)), int(scatter_first), int(nthreads), ctypes.byref(stats))
    if rc != 0:
        raise RuntimeError('oracle_propagate failed (%d)' % rc)
    return hp.photons(), hp.rng_counters, stats.as_dict()


def to_diffuse(packed, photons, seed, photon_id_base=0, max_steps=10, rng_counters=None, active=None, variant='contract'):
    """to_diffuse of the hybrid render (hybrid_render.cu:20-58) on ``photons``: the step loop without propagate's division of
    direction and polarisation by their norms on load, left after the first step that sets REFLECT_DIFFUSE.  ``active``:
    boolean mask of the photons to run (the others come back as they are).  Returns (Photons, rng_counters, side), ``side``
    the inside_to_outside of the last triangle each photon hit (0 where it hit none)."""
    lib = load(variant)
    hp = HostPhotons(photons, rng_counters=rng_counters)
    mask = None if active is None else np.ascontiguousarray(active, dtype=np.uint8)
    side = np.zeros(hp.n, dtype=np.uint32)
    rc = lib.oracle_to_diffuse(ctypes.byref(packed.desc), ctypes.byref(hp.struct), hp.n, _abi.Rng(int(seed), int(photon_id_base)),
                               int(max_steps), None if mask is None else mask.ctypes.data, side.ctypes.data, None)
    if rc != 0:
        raise RuntimeError('oracle_to_diffuse failed (%d)' % rc)
    return hp.photons(), hp.rng_counters, side


def ref_propagate(packed, photons, seed, photon_id_base=0, max_steps=10, use_weights=False, scatter_first=0,
                  rng_counters=None, variant='contract'):
    """``propagate`` through the reference's own kernel and its host loop (ref_phys_propagate).  Returns
    (Photons, rng_counters, {'launches': n})."""
    lib = load_ref_physics(variant)
    hp = HostPhotons(photons, rng_counters=rng_counters)
    launches = c_uint64(0)
    rc = lib.ref_phys_propagate(ctypes.byref(packed.desc), ctypes.byref(hp.struct), hp.n, _abi.Rng(int(seed), int(photon_id_base)),
                                int(max_steps), int(bool(use_weights)), int(scatter_first), ctypes.byref(launches))
    if rc != 0:
        raise RuntimeError('ref_phys_propagate failed (%d)' % rc)
    return hp.photons(), hp.rng_counters, {'launches': launches.value}


SINGLE = {'rayleigh_scatter': 0, 'propagate_at_boundary': 1, 'specular_reflector': 2, 'diffuse_reflector': 3,
          'propagate_at_surface': 4, 'propagate_to_boundary': 5}


def _single(fn, packed, which, photon, seed, photon_id, counter, normal, n1, n2, absorption_length, scattering_length,
            material1, surface_index, distance_to_boundary, use_weights, scatter_first):
    hp = HostPhotons(photon, rng_counters=[counter])
    assert hp.n == 1
    nrm = (c_float * 3)(*[float(x) for x in normal])
    command = fn(ctypes.byref(packed.desc), ctypes.byref(hp.struct), _abi.Rng(int(seed), int(photon_id)), SINGLE[which], nrm,
                 float(n1), float(n2), float(absorption_length), float(scattering_length), int(material1), int(surface_index),
                 float(distance_to_boundary), int(bool(use_weights)), int(scatter_first))
    if command <= -100:
        raise RuntimeError('single routine %s refused its arguments (%d)' % (which, command))
    return hp.photons(), int(hp.rng_counters[0]), command


def single(packed, which, photon, seed=0, photon_id=0, counter=0, normal=(0.0, 0.0, 1.0), n1=1.0, n2=1.0,
           absorption_length=1.0, scattering_length=1.0, material1=0, surface_index=-1, distance_to_boundary=0.0,
           use_weights=False, scatter_first=0, variant='contract'):
    """ONE call of one physics routine (a name of ``SINGLE``) of the oracle on a one-photon ``photon`` with an explicit
    State; the stream is (seed, photon_id) at ``counter``.  Returns (Photons, counter afterwards, command), command
    being BREAK 0 / CONTINUE 1 / PASS 2, or -1 for the two routines that return nothing."""
    return _single(load(variant).oracle_single, packed, which, photon, seed, photon_id, counter, normal, n1, n2, absorption_length,
                   scattering_length, material1, surface_index, distance_to_boundary, use_weights, scatter_first)


def ref_single(packed, which, photon, seed=0, photon_id=0, counter=0, normal=(0.0, 0.0, 1.0), n1=1.0, n2=1.0,
               absorption_length=1.0, scattering_length=1.0, material1=0, surface_index=-1, distance_to_boundary=0.0,
               use_weights=False, scatter_first=0, variant='contract'):
    """``single`` through the reference's own routine (ref_phys_single)."""
    return _single(load_ref_physics(variant).ref_phys_single, packed, which, photon, seed, photon_id, counter, normal, n1, n2,
                   absorption_length, scattering_length, material1, surface_index, distance_to_boundary, use_weights, scatter_first)


def distance_to_mesh(packed, origins, directions, variant='contract', last_hits=None, normalize=True):
    """(distance, triangle) for a ray bundle; misses give distance nan-filled here and triangle -1.
    ``last_hits``: per-ray triangle the ray must not hit (intersect_mesh's last_hit_triangle).
    ``normalize=False``: intersect_mesh on the directions as they are, not distance_to_mesh's direction / norm(direction)."""
    lib = load(variant)
    o = np.ascontiguousarray(origins, dtype=np.float32)
    d = np.ascontiguousarray(directions, dtype=np.float32)
    n = len(o)
    dist = np.full(n, np.nan, dtype=np.float32)
    tri = np.empty(n, dtype=np.int32)
    stats = _abi.PropagateStats()
    lh = None if last_hits is None else np.ascontiguousarray(last_hits, dtype=np.int32)
    cast = lib.oracle_intersect_mesh if normalize else lib.oracle_intersect_mesh_as_given
    cast.restype = c_int32
    cast.argtypes = [POINTER(_abi.GeometryDesc), c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, POINTER(_abi.PropagateStats)]
    cast(ctypes.byref(packed.desc), n, o.ctypes.data, d.ctypes.data, None if lh is None else lh.ctypes.data, dist.ctypes.data,
         tri.ctypes.data, ctypes.byref(stats))
    return dist, tri, stats.as_dict()


def reference_test_order(nodes, variant='contract'):
    """Triangles in the order the reference walk tests them when every box is entered (see
    oracle_reference_test_order).  ``nodes``: packed uint4 record array or [n][4] uint32."""
    lib = load(variant)
    raw = np.ascontiguousarray(nodes).view(np.uint32).reshape(-1, 4)
    nleaf = int(((raw[:, 3] >> 28) == 0).sum())
    out = np.empty(max(nleaf, 1), dtype=np.uint32)
    lib.oracle_reference_test_order.restype = ctypes.c_int64
    lib.oracle_reference_test_order.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
    n = lib.oracle_reference_test_order(raw.ctypes.data, len(raw), out.ctypes.data, len(out))
    if n < 0:
        raise RuntimeError('reference stack overflow')
    return out[:min(n, len(out))]


def generate_bomb(n, seed, id_base=0, pos=(0, 0, 0), wavelength_lo=400.0, wavelength_hi=0.0, variant='contract'):
    lib = load(variant)
    hp = HostPhotons(n=n)
    p = (c_float * 3)(*[float(x) for x in pos])
    lib.oracle_generate_bomb(ctypes.byref(hp.struct), n, int(seed), int(id_base), p, float(wavelength_lo), float(wavelength_hi))
    return hp.photons()


def daq_state(nwords):
    """The three channel arrays of a DAQ as begin_acquire leaves them: (earliest time bits = 1e9, charge counts 0, histories 0)."""
    return (np.full(nwords, np.float32(1e9).view(np.uint32), dtype=np.uint32), np.zeros(nwords, dtype=np.uint32),
            np.zeros(nwords, dtype=np.uint32))


def run_daq(packed, photons, tables_host, charge_unit, seed, photon_id_base=0, acquisition=0, weight=1.0,
            start_photon=0, nphotons=None, variant='contract', state=None, reference=False):
    """run_daq on HOST arrays (``reference``: through the reference's own kernel, ref_phys_run_daq).  ``tables_host`` = (time_cdf_x, time_cdf_y, charge_cdf_x, charge_cdf_y) float32
    arrays of equal pairwise length.  Returns (earliest_time float32, charge float32, histories uint32, hit mask).
    ``state``: the three arrays of ``daq_state`` to acquire ONTO, in place (a second acquire without a reset);
    None: fresh ones."""
    fn = load_ref_physics(variant).ref_phys_run_daq if reference else load(variant).oracle_run_daq
    hp = HostPhotons(photons)
    tx, ty, qx, qy = [np.ascontiguousarray(a, dtype=np.float32) for a in tables_host]
    tab = _abi.DaqTables(tx.ctypes.data, ty.ctypes.data, len(tx), qx.ctypes.data, qy.ctypes.data, len(qx), float(charge_unit))
    nch = packed.desc.nchannels
    t_int, q_int, hist = daq_state(nch) if state is None else state
    assert all(a.dtype == np.uint32 and a.flags['C_CONTIGUOUS'] and len(a) >= nch for a in (t_int, q_int, hist))
    if nphotons is None:
        nphotons = hp.n - start_photon
    fn(ctypes.byref(packed.desc), ctypes.byref(tab), int(start_photon), int(nphotons), event.SURFACE_DETECT,
       ctypes.byref(hp.struct), _abi.Rng(int(seed), int(photon_id_base)), int(acquisition), float(weight),
       t_int.ctypes.data, q_int.ctypes.data, hist.ctypes.data)
    t = t_int.view(np.float32)
    return t, (q_int.astype(np.float32) * np.float32(charge_unit)).astype(np.float32), hist, t < 1e8


def run_daq_many(packed, photons, tables_host, charge_unit, seed, ndaq, photon_id_base=0, acquisition=0, weight=1.0,
                 start_photon=0, nphotons=None, variant='contract', state=None, channel_stride=None, reference=False):
    """run_daq_many on HOST arrays (``reference``: through the reference's own kernel, ref_phys_run_daq_many): ``ndaq`` acquisitions side by side (copy i = entries [i*stride, (i+1)*stride),
    ``channel_stride`` = nchannels unless given).  Returns (earliest_time float32, charge float32, histories uint32,
    hit mask), each of ndaq * stride entries.  ``state``: as in ``run_daq``, arrays of at least ndaq * stride words."""
    fn = load_ref_physics(variant).ref_phys_run_daq_many if reference else load(variant).oracle_run_daq_many
    hp = HostPhotons(photons)
    tx, ty, qx, qy = [np.ascontiguousarray(a, dtype=np.float32) for a in tables_host]
    tab = _abi.DaqTables(tx.ctypes.data, ty.ctypes.data, len(tx), qx.ctypes.data, qy.ctypes.data, len(qx), float(charge_unit))
    nch = packed.desc.nchannels if channel_stride is None else int(channel_stride)
    assert nch >= packed.desc.nchannels
    t_int, q_int, hist = daq_state(nch * ndaq) if state is None else state
    assert all(a.dtype == np.uint32 and a.flags['C_CONTIGUOUS'] and len(a) >= nch * ndaq for a in (t_int, q_int, hist))
    if nphotons is None:
        nphotons = hp.n - start_photon
    fn(ctypes.byref(packed.desc), ctypes.byref(tab), int(start_photon), int(nphotons), event.SURFACE_DETECT,
       ctypes.byref(hp.struct), _abi.Rng(int(seed), int(photon_id_base)), int(acquisition), float(weight),
       int(ndaq), int(nch), t_int.ctypes.data, q_int.ctypes.data, hist.ctypes.data)
    t = t_int.view(np.float32)
    return t, (q_int.astype(np.float32) * np.float32(charge_unit)).astype(np.float32), hist, t < 1e8


# one primitive of include/chroma_math.h per element: the op numbers of oracle_math3, oracle_rng_probe and the engine's
# chroma_probe_math ('uniform' takes its words, 'f2i' and 'f2u32' give their integers, as the bits of float32 arrays)
MATH_OPS = {'log': 0, 'exp': 1, 'sin': 2, 'cos': 3, 'tan': 4, 'asin': 5, 'acos': 6, 'atan2': 7, 'sqrt': 8, 'uniform': 9,
            'atan': 10, 'floor': 11, 'round': 12, 'f2i': 13, 'f2u32': 14, 'div': 15, 'fmin': 16, 'fmax': 17, 'fma': 18,
            'philox': 19, 'rng_uniform': 20, 'rng_normal': 21}
RNG_PROBE_WIDTH = {'philox': 4, 'rng_uniform': 8, 'rng_normal': 4}


def math_fn(fn, x, y=None, z=None, variant='contract'):
    lib = load(variant)
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = x if y is None else np.ascontiguousarray(y, dtype=np.float32)
    z = x if z is None else np.ascontiguousarray(z, dtype=np.float32)
    assert x.size == y.size == z.size and MATH_OPS[fn] <= 18
    out = np.empty_like(x)
    lib.oracle_math3.restype = c_int32
    lib.oracle_math3.argtypes = [c_int32, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p]
    rc = lib.oracle_math3(MATH_OPS[fn], x.size, x.ctypes.data, y.ctypes.data, z.ctypes.data, out.ctypes.data)
    assert rc == 0
    return out


def rng_probe(fn, words, variant='contract'):
    """'philox': words [n][6] = counter 0..3, key 0..1 -> [n][4] uint32.  'rng_uniform' / 'rng_normal': words [n][6] =
    seed lo, seed hi, photon id lo, id hi, stream word, start counter -> the 8 uniforms / 4 normal deviates that follow,
    [n][8] / [n][4] float32."""
    lib = load(variant)
    lib.oracle_rng_probe.restype = c_int32
    lib.oracle_rng_probe.argtypes = [c_int32, c_uint64, c_void_p, c_void_p]
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 6)
    out = np.empty((len(w), RNG_PROBE_WIDTH[fn]), dtype=np.uint32)
    rc = lib.oracle_rng_probe(MATH_OPS[fn], len(w), w.ctypes.data, out.ctypes.data)
    assert rc == 0
    return out if fn == 'philox' else out.view(np.float32)


def render(packed, origins, directions, alpha_depth=10, bg_color=0, state=None, variant='contract'):
    """render.cu on host arrays.  ``state`` = (dx, dxlen, color) of a previous call (keep_last_render), else fresh.
    Returns (pixels uint32, (dx [n][alpha_depth], dxlen [n], color [n][alpha_depth][4]))."""
    lib = load(variant)
    lib.oracle_render.restype = c_int32
    lib.oracle_render.argtypes = [POINTER(_abi.GeometryDesc), c_uint64, c_void_p, c_void_p, c_uint32, c_uint32, c_void_p, c_void_p,
                                  c_void_p, c_void_p]
    o = np.ascontiguousarray(origins, dtype=np.float32)
    d = np.ascontiguousarray(directions, dtype=np.float32)
    n = len(o)
    if state is None:
        dx = np.zeros((n, alpha_depth), dtype=np.float32)
        dxlen = np.zeros(n, dtype=np.uint32)
        color = np.zeros((n, alpha_depth, 4), dtype=np.float32)
    else:
        dx, dxlen, color = [np.array(a, copy=True) for a in state]
    pixels = np.zeros(n, dtype=np.uint32)
    rc = lib.oracle_render(ctypes.byref(packed.desc), n, o.ctypes.data, d.ctypes.data, int(alpha_depth), int(bg_color) & 0xFFFFFFFF,
                           pixels.ctypes.data, dx.ctypes.data, dxlen.ctypes.data, color.ctypes.data)
    if rc != 0:
        raise RuntimeError('oracle_render failed (%d)' % rc)
    return pixels, (dx, dxlen, color)


PROBES = {'interp_property': 0, 'interp_idx': 1, 'interp': 2, 'rotate': 3}


def probe(fn, x, tab_x=None, tab_f=None, start=0.0, step=1.0, variant='contract'):
    """One call per element of a single function of the path (oracle_probe).  'rotate': x is [n][7]
    (a, phi, axis) and the result [n][5] (rotated vector, cos phi, sin phi)."""
    lib = load(variant)
    lib.oracle_probe.restype = c_int32
    lib.oracle_probe.argtypes = [c_int32, c_uint64, c_void_p, c_void_p, c_void_p, c_uint32, c_float, c_float, c_void_p]
    x = np.ascontiguousarray(x, dtype=np.float32)
    n = len(x)
    out = np.empty((n, 5) if fn == 'rotate' else n, dtype=np.float32)
    tx = None if tab_x is None else np.ascontiguousarray(tab_x, dtype=np.float32)
    tf = None if tab_f is None else np.ascontiguousarray(tab_f, dtype=np.float32)
    ntab = len(tx) if tx is not None else (len(tf) if tf is not None else 0)
    rc = lib.oracle_probe(PROBES[fn], n, x.ctypes.data, None if tx is None else tx.ctypes.data,
                          None if tf is None else tf.ctypes.data, ntab, float(start), float(step), out.ctypes.data)
    assert rc == 0
    return out


def philox(counter, key):
    lib = load()
    c = np.array(counter, dtype=np.uint32)
    k = np.array(key, dtype=np.uint32)
    out = np.zeros(4, dtype=np.uint32)
    lib.oracle_philox(c.ctypes.data, k.ctypes.data, out.ctypes.data)
    return out


def uniform_stream(seed, photon_id, n, start=0):
    lib = load()
    out = np.empty(n, dtype=np.float32)
    lib.oracle_uniform_stream(int(seed), int(photon_id), int(start), int(n), out.ctypes.data)
    return out
