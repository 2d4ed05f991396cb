"""What digitising the gates of one chunk of the time-binned DAQ costs, beside the trigger call it follows:

    python tools/daq_digitize_probe.py [--repeats 7] [--label NAME] [--events 500] [--channels 29007] [--bins 1000] [--pe 2000]
                                       [--dark 0.05] [--trigger 40,8,64,16,48] [--taps 147] [--sigma 1.5]

Both calls are functions of the pulse arrays alone, so the probe needs no geometry: it makes the pulses of one chunk on the host
from a seed -- per event ``--pe`` photoelectrons on uniformly drawn channels in a Gaussian burst of 4 bins' sigma around a drawn
bin, and ``--dark`` noise pulses per channel anywhere in the window, reduced per (event, channel, bin) as
chroma_daq_acquire_pulses writes them -- and uploads them once.  The defaults are a chunk of the 29 007-channel detector: 500
events, 1 000 bins.  Then, ``--repeats`` times after one warm-up each and interleaved, by the host clock around calls that return
with their work done: chroma_daq_trigger_pulses, chroma_daq_digitize_gates on ALL its hits in one call, and the copy of the
samples and flag words back to the host.  Prints the medians (min .. max), the samples per second of the digitise call and the
bytes read back, and checks a few traces against the host twin."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np

from chroma_amd import _lib, gpu
from chroma_amd.gpu.tools import to_gpu, empty


def make_pulses(rng, nevents, nchannels, nbins, pe, dark):
    """(offsets, channel, bin, npe, q_int, t_first, flags) of one chunk, in (event, channel, bin) order."""
    keys = []
    for r in range(nevents):
        centre = rng.integers(nbins // 4, 3 * nbins // 4)
        b = np.clip(np.rint(rng.normal(centre, 4.0, pe)), 0, nbins - 1).astype(np.int64)
        c = rng.integers(0, nchannels, pe)
        ndark = rng.poisson(dark * nchannels)
        b = np.concatenate([b, rng.integers(0, nbins, ndark)])
        c = np.concatenate([c, rng.integers(0, nchannels, ndark)])
        keys.append((r * nchannels + c) * nbins + b)
    keys, npe = np.unique(np.concatenate(keys), return_counts=True)
    row, rest = keys // (nchannels * nbins), keys % (nchannels * nbins)
    n = len(keys)
    q_int = (npe * rng.integers(40000, 90000, n)).astype(np.uint32)          # (a charge unit of 2^-16 of a few photoelectrons)
    return (np.searchsorted(row, np.arange(nevents + 1)).astype(np.uint32), (rest // nbins).astype(np.int32), (rest % nbins).astype(np.uint32),
            npe.astype(np.uint32), q_int, ((rest % nbins) * 0.25).astype(np.float32), np.ones(n, dtype=np.uint32))


def clocked(fn, *args):
    t0 = time.perf_counter()
    rc = fn(*args)
    ms = 1e3 * (time.perf_counter() - t0)
    _lib.check(rc)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--label', default='')
    ap.add_argument('--events', type=int, default=500)
    ap.add_argument('--channels', type=int, default=29007)
    ap.add_argument('--bins', type=int, default=1000)
    ap.add_argument('--pe', type=int, default=2000, help='photoelectrons of the burst of every event')
    ap.add_argument('--dark', type=float, default=0.05, help='noise pulses per channel and event')
    ap.add_argument('--trigger', default='40,8,64,16,48', help='THRESHOLD,WIDTH,HOLDOFF,PRE,POST in bins (nhit)')
    ap.add_argument('--taps', type=int, default=147, help='the bins of the biexponential pulse shape')
    ap.add_argument('--sigma', type=float, default=1.5, help='electronics noise in ADC counts (0: none)')
    args = ap.parse_args()
    ctx = gpu.create_cuda_context(0)
    lib, handle = ctx._lib, ctx.handle
    rng = np.random.default_rng(7)
    host = make_pulses(rng, args.events, args.channels, args.bins, args.pe, args.dark)
    npulses = len(host[1])
    d_offsets, d_channel, d_bin, d_npe, d_q_int, d_t_first, d_flags = [to_gpu(a) for a in host]
    trigger = gpu.DaqTrigger(*[int(x) for x in args.trigger.split(',')])
    digitizer = gpu.DaqDigitizer.biexponential(20.0, 2.0, 10.0, 0.5, length=args.taps, bits=14, pedestal=200, noise_sigma=args.sigma)
    charge_unit = 2.0 ** -16
    struct, keep = digitizer.struct(charge_unit)
    win, trig = _lib.DaqWindow(0.0, 0.25, args.bins), trigger.struct()
    G = trigger.pre + trigger.post
    capacity = args.events * -(-args.bins // trigger.holdoff)
    d_trig_offsets, d_trig_bin, d_trig_sum, d_hit_offsets = (empty(args.events + 1, np.uint32), empty(capacity, np.uint32), empty(capacity, np.uint32),
                                                             empty(capacity + 1, np.uint32))
    d_hits = [empty(npulses, np.uint32) for _ in range(5)]
    ntriggers, nhits = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def trigger_call():
        return clocked(lib.chroma_daq_trigger_pulses, handle, args.events, args.channels, ctypes.byref(win), ctypes.byref(trig), d_offsets.ptr, d_channel.ptr,
                       d_bin.ptr, d_npe.ptr, d_q_int.ptr, d_t_first.ptr, d_flags.ptr, npulses, capacity, d_trig_offsets.ptr, d_trig_bin.ptr, d_trig_sum.ptr,
                       d_hit_offsets.ptr, npulses, *([a.ptr for a in d_hits] + [None, ctypes.byref(ntriggers), ctypes.byref(nhits)]))
    trigger_call()
    nt, nh = int(ntriggers.value), int(nhits.value)
    d_adc, d_trace_flags = empty(nh * G, np.uint16), empty(nh, np.uint32)

    def digitize_call():
        return clocked(lib.chroma_daq_digitize_gates, handle, args.events, args.channels, ctypes.byref(win), ctypes.byref(trig), ctypes.byref(struct), 5, 0,
                       d_offsets.ptr, d_channel.ptr, d_bin.ptr, d_q_int.ptr, npulses, d_trig_offsets.ptr, d_trig_bin.ptr, nt, d_hit_offsets.ptr,
                       d_hits[0].ptr, nh, 0, nh, nh * G, d_adc.ptr, d_trace_flags.ptr)
    times = {'trigger': [], 'digitize': [], 'back': []}
    for repeat in range(args.repeats + 1):
        a = trigger_call()
        b = digitize_call()
        t0 = time.perf_counter()
        adc, trace_flags = d_adc.get(), d_trace_flags.get()
        c = 1e3 * (time.perf_counter() - t0)
        if repeat:
            times['trigger'].append(a)
            times['digitize'].append(b)
            times['back'].append(c)
    # a few traces against the host twin
    offsets = host[0].astype(np.int64)
    pulses = gpu.EventPulses(gpu.DaqWindow(0.0, 0.25, args.bins), args.channels, charge_unit, offsets[:3] - offsets[0], *[a[:offsets[2]] for a in host[1:]],
                             outside=np.zeros((2, 2), dtype=np.uint32))
    twin = pulses.trigger(trigger).digitize(digitizer, seed=5, acquisition=0)
    assert len(twin.adc) and np.array_equal(twin.adc, adc.reshape(nh, G)[:len(twin.adc)]) and np.array_equal(twin.trace_flags, trace_flags[:len(twin.adc)])
    cell = lambda ts: '%8.2f (%7.2f .. %7.2f)' % (statistics.median(ts), min(ts), max(ts))
    out_trigger = 4 * (args.events + 1 + 3 * nt + 1 + 5 * nh)
    out_digitize = adc.nbytes + trace_flags.nbytes
    print('# %s  %d events x %d channels x %d bins, %d pulses, %r, %d taps, sigma %g; %d repeats after one warm-up; ms, median (min .. max)'
          % (args.label, args.events, args.channels, args.bins, npulses, trigger, args.taps, args.sigma, args.repeats))
    print('# triggers | gated hits | samples | chroma_daq_trigger_pulses | chroma_daq_digitize_gates | samples/s | read-back of the traces | '
          'bytes of the traces | bytes of the trigger\'s outputs | ratio of the times | ratio of the bytes | clipped traces')
    print('%d | %d | %d | %s | %s | %.3g | %s | %d | %d | %.2f | %.2f | %d'
          % (nt, nh, nh * G, cell(times['trigger']), cell(times['digitize']), nh * G / (1e-3 * statistics.median(times['digitize'])), cell(times['back']),
             out_digitize, out_trigger, statistics.median(times['digitize']) / statistics.median(times['trigger']), out_digitize / out_trigger,
             int((trace_flags != 0).sum())), flush=True)
    del keep


if __name__ == '__main__':
    main()
