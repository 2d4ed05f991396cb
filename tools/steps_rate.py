"""What generating photons from particle steps costs on the device, next to uploading them and to propagating them:
1e7 and 1e8 scintillation photons from a muon-like track of 1e4 segments (ONE segment shape, not a spread of event types).
Per size: the counting call (count kernel + scan + the total read back), the generating call (k_steps_generate, 64 bytes of
stores per photon) with its store bandwidth against the HBM figures of the MI355X, the time the measured 53 GB/s upload
 would need for the same photons, and chroma_propagate_hits on them.  Times are host clocks around work
that ends in a device synchronise, best of the repetitions.  usage: steps_rate.py [c3|detector|lite|tiny] [sizes ...]  (GPU box)"""
import ctypes, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from chroma_amd import _lib, demo, gpu
from chroma_amd.demo.optics import water
from chroma_amd.geometry import Material, standard_wavelengths
from chroma_amd.loader import create_geometry_from_obj

HBM_ACHIEVABLE, HBM_PEAK, UPLOAD = 6.3e12, 8.0e12, 53e9          # bytes/s: float4 copy measured, spec, pageable NumPy -> HBM
config = sys.argv[1] if len(sys.argv) > 1 else 'c3'
sizes = [int(float(x)) for x in sys.argv[2:]] or [10_000_000, 100_000_000]
NSEG, REPS = 10_000, 3

ctx = gpu.create_cuda_context(0)
t0 = time.perf_counter()
geo = create_geometry_from_obj({'tiny': demo.tiny, 'lite': demo.detector_lite, 'detector': demo.detector, 'c3': demo.detector29k}[config]())
detector = gpu.GPUDetector(geo)
print('%s on %s: geometry in %.1f s' % (config, ctx.device_name(), time.perf_counter() - t0), flush=True)

wl = standard_wavelengths.astype(float)
scint = Material('scintillating_water')
scint.refractive_index = water.refractive_index
scint.set('scintillation_spectrum', np.where(np.abs(wl - 430) < 50, 1.0 + np.cos((wl - 430) * np.pi / 50), 0.0))
scint.scintillation_light_yield = 1.0e4
t = np.arange(0, 1000, 0.05)
scint.scintillation_waveform = np.column_stack([t, np.exp(-t / 5.0)])
source = gpu.steps.LightSource(scint)
radius = 0.4 * float(np.abs(geo.mesh.vertices).max())
x = np.linspace(-radius, radius, NSEG + 1)
zero = np.zeros(NSEG)


def timed(f):
    ctx.synchronize()
    t0 = time.perf_counter()
    out = f()
    ctx.synchronize()
    return time.perf_counter() - t0, out


for n in sizes:
    seg = gpu.steps.Segments(np.column_stack([x[:-1], zero, zero]), np.column_stack([x[1:], zero, zero]), x[:-1] / 299.79, x[1:] / 299.79,
                             1.0, 0.0, n / NSEG / scint.scintillation_light_yield, 0)
    device = {name: gpu.to_gpu(getattr(seg, name).reshape(-1), ctx) for name in ('a', 'b', 't_a', 't_b', 'beta', 'z', 'qedep', 'evidx')}
    s = seg.struct({name: a.ptr for name, a in device.items()})
    d_offsets = gpu.empty(2 * NSEG + 1, np.uint32, ctx)
    total = ctypes.c_uint64()
    count = lambda: _lib.check(ctx._lib.chroma_steps_count(ctx.handle, ctypes.byref(source.struct), ctypes.byref(s), 11, d_offsets.ptr,
                                                           ctypes.byref(total)))
    count()
    photons = gpu.GPUPhotonsSlice(rng_counters=gpu.empty(total.value, np.uint32, ctx), **gpu.photon._alloc_fields(total.value, ctx))
    arrays = gpu.photon._structure(photons)
    generate = lambda: _lib.check(ctx._lib.chroma_steps_generate(ctx.handle, ctypes.byref(source.struct), ctypes.byref(s), 11, d_offsets.ptr,
                                                                 ctypes.byref(arrays), total.value))
    generate()                                                   # warm-up: code objects, the scratch block
    t_count = min(timed(count)[0] for _ in range(REPS))
    t_gen = min(timed(generate)[0] for _ in range(REPS))
    nbytes = 64 * total.value
    rng = _lib.Rng(7, 0)
    t_prop, hits = [], 0
    for rep in range(2):                                         # (the second call: working buffers sized; it regenerates its input)
        generate()
        dt, found = timed(lambda: photons.propagate_hits(detector, rng, max_steps=100, device=True))
        t_prop.append(dt); hits = len(found[0])
    out = {'config': config, 'segments': NSEG, 'photons': total.value, 'count_s': t_count, 'generate_s': t_gen,
           'store_bytes': nbytes, 'store_bytes_per_s': nbytes / t_gen, 'share_of_hbm_achievable': nbytes / t_gen / HBM_ACHIEVABLE,
           'share_of_hbm_peak': nbytes / t_gen / HBM_PEAK, 'upload_at_53GBps_s': nbytes / UPLOAD,
           'generate_over_upload': (t_count + t_gen) / (nbytes / UPLOAD), 'propagate_hits_s': min(t_prop), 'hits': hits,
           'generate_over_propagate': (t_count + t_gen) / min(t_prop)}
    print(json.dumps(out), flush=True)
    del photons, arrays
