"""What reducing the traces of one chunk of the time-binned DAQ on the device costs, beside the digitise call it follows and the
copy of the traces it can replace:

    python tools/daq_reduce_probe.py [--repeats 7] [--label NAME] [--events 500] [--channels 29007] [--bins 1000] [--pe 2000]
                                     [--dark 0.05] [--trigger 40,8,64,16,48] [--taps 147] [--sigma 1.5]
                                     [--reduce 6,2,30,0.5,0,2]

The synthetic chunk of tools/daq_digitize_probe.py (its pulses, its trigger, its digitiser), digitised once; then, ``--repeats``
times after one warm-up each and interleaved, by the host clock around calls that return with their work done:
chroma_daq_digitize_gates on all hits, chroma_daq_reduce_traces on all traces (count, scan and fill together), the copy of the
found arrays (per trace the offsets, base, flag word and the digitiser's trace flags; per found pulse the seven arrays) and the copy
of the traces with their flags, both into host arrays made once.  Prints the medians (min .. max), the bytes of each copy and the
two paths side by side -- digitise + copy of the traces against digitise + reduce + copy of the found arrays -- then what the
reduction makes of the truth: the distribution of q_reco / q_true (the trace's found charge over the gated hit's charge) and of
t_reco - t_first (ns) over the traces with a found pulse.  The first 2000 traces are checked against the host twin."""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

import numpy as np

from chroma_amd import _lib, gpu
from chroma_amd.gpu.daq import FOUND_COLUMNS, reduce_traces_host
from chroma_amd.gpu.tools import to_gpu, empty
from daq_digitize_probe import make_pulses, clocked


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
    ap.add_argument('--reduce', default='6,2,30,0.5,0,2', help='THRESHOLD,LEAD,LAG,CFD,NBASELINE,MIN_WIDTH of the reducer')
    args = ap.parse_args()
    ctx = gpu.create_cuda_context(0)
    lib, handle = ctx._lib, ctx.handle
    rng = np.random.default_rng(7)
    host = make_pulses(rng, args.events, args.channels, args.bins, args.pe, args.dark)
    npulses = len(host[1])
    d_offsets, d_channel, d_bin, d_npe, d_q_int, d_t_first, d_flags = [to_gpu(a) for a in host]
    trigger = gpu.DaqTrigger(*[int(x) for x in args.trigger.split(',')])
    digitizer = gpu.DaqDigitizer.biexponential(20.0, 2.0, 10.0, 0.5, length=args.taps, bits=14, pedestal=200, noise_sigma=args.sigma)
    parts = args.reduce.split(',')
    reducer = gpu.DaqReducer.for_digitizer(digitizer, int(parts[0]), lead=int(parts[1]), lag=int(parts[2]), cfd=float(parts[3]), nbaseline=int(parts[4]),
                                           min_width=int(parts[5]))
    charge_unit = 2.0 ** -16
    struct, keep = digitizer.struct(charge_unit)
    reducer_struct = reducer.struct()
    window = gpu.DaqWindow(0.0, 0.25, args.bins)
    win, trig = _lib.DaqWindow(0.0, 0.25, args.bins), trigger.struct()
    G = trigger.pre + trigger.post
    reducer.check(G)
    capacity = args.events * -(-args.bins // trigger.holdoff)
    d_trig_offsets, d_trig_bin, d_trig_sum, d_hit_offsets = (empty(args.events + 1, np.uint32), empty(capacity, np.uint32), empty(capacity, np.uint32),
                                                             empty(capacity + 1, np.uint32))
    d_hits = [empty(npulses, np.uint32) for _ in range(5)]
    ntriggers, nhits = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(lib.chroma_daq_trigger_pulses(handle, args.events, args.channels, ctypes.byref(win), ctypes.byref(trig), d_offsets.ptr, d_channel.ptr, d_bin.ptr,
                                             d_npe.ptr, d_q_int.ptr, d_t_first.ptr, d_flags.ptr, npulses, capacity, d_trig_offsets.ptr, d_trig_bin.ptr,
                                             d_trig_sum.ptr, d_hit_offsets.ptr, npulses, *([a.ptr for a in d_hits] + [None, ctypes.byref(ntriggers), ctypes.byref(nhits)])))
    nt, nh = int(ntriggers.value), int(nhits.value)
    d_adc, d_trace_flags = empty(nh * G, np.uint16), empty(nh, np.uint32)

    def digitize_call():
        return clocked(lib.chroma_daq_digitize_gates, handle, args.events, args.channels, ctypes.byref(win), ctypes.byref(trig), ctypes.byref(struct), 5, 0,
                       d_offsets.ptr, d_channel.ptr, d_bin.ptr, d_q_int.ptr, npulses, d_trig_offsets.ptr, d_trig_bin.ptr, nt, d_hit_offsets.ptr,
                       d_hits[0].ptr, nh, 0, nh, nh * G, d_adc.ptr, d_trace_flags.ptr)
    digitize_call()
    # the room for the found pulses: what a first call reports (the capacity protocol), as GPUEventDaq grows its buffers
    d_per_trace = [empty(nh + 1, np.uint32), empty(nh, np.int32), empty(nh, np.uint32)]
    nfound = ctypes.c_uint64(0)
    rc = lib.chroma_daq_reduce_traces(handle, ctypes.byref(reducer_struct), G, nh, d_adc.ptr, 0, *([a.ptr for a in d_per_trace] + [None] * 7 + [ctypes.byref(nfound)]))
    assert rc == 0 or nfound.value > 0
    room = int(nfound.value)
    d_found = [empty(max(room, 1), kind) for _, kind in FOUND_COLUMNS]

    def reduce_call():
        return clocked(lib.chroma_daq_reduce_traces, handle, ctypes.byref(reducer_struct), G, nh, d_adc.ptr, room,
                       *([a.ptr for a in d_per_trace] + [a.ptr for a in d_found] + [ctypes.byref(nfound)]))
    # both copies go into host arrays made (and touched) once, so that the clock sees the copies and not the host's allocator
    def back(dst, src):
        if dst.nbytes:
            _lib.check(lib.chroma_memcpy_dtoh(handle, _lib.ptr(dst), ctypes.c_void_p(src.ptr), dst.nbytes))
    per_trace = [np.zeros(len(x), dtype=x.dtype) for x in d_per_trace]
    found = [np.zeros(room, dtype=kind) for _, kind in FOUND_COLUMNS]
    flags_back, adc, trace_flags = np.zeros(nh, dtype=np.uint32), np.zeros(nh * G, dtype=np.uint16), np.zeros(nh, dtype=np.uint32)
    times = {'digitize': [], 'reduce': [], 'found': [], 'traces': []}
    for repeat in range(args.repeats + 1):
        a = digitize_call()
        b = reduce_call()
        t0 = time.perf_counter()
        for dst, src in zip(per_trace + found + [flags_back], d_per_trace + d_found + [d_trace_flags]):
            back(dst, src)
        c = 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        back(adc, d_adc)
        back(trace_flags, d_trace_flags)
        d = 1e3 * (time.perf_counter() - t0)
        if repeat:
            for name, ms in zip(('digitize', 'reduce', 'found', 'traces'), (a, b, c, d)):
                times[name].append(ms)
    assert int(nfound.value) == room
    # a few traces against the host twin
    adc = adc.reshape(nh, G)
    twin = reduce_traces_host(adc[:2000], reducer)
    n = int(twin[0][-1])
    assert np.array_equal(twin[0], per_trace[0][:2001]) and np.array_equal(twin[1], per_trace[1][:2000]) and np.array_equal(twin[2], per_trace[2][:2000])
    assert n > 0 and all(np.array_equal(a, b[:n]) for a, b in zip(twin[3:], found))
    med = lambda name: statistics.median(times[name])
    cell = lambda name: '%8.2f (%7.2f .. %7.2f)' % (med(name), min(times[name]), max(times[name]))
    bytes_found = sum(a.nbytes for a in per_trace) + sum(a.nbytes for a in found) + flags_back.nbytes
    bytes_traces = adc.nbytes + trace_flags.nbytes
    print('# %s  %d events x %d channels x %d bins, %d pulses, %r, %d taps, sigma %g, %r; %d repeats after one warm-up; ms, median (min .. max)'
          % (args.label, args.events, args.channels, args.bins, npulses, trigger, args.taps, args.sigma, reducer, args.repeats))
    print('# traces | samples | found pulses | chroma_daq_digitize_gates | chroma_daq_reduce_traces | copy of the found arrays | copy of the traces | '
          'bytes of the found arrays | bytes of the traces | digitise + copy of the traces | digitise + reduce + copy of the found arrays')
    print('%d | %d | %d | %s | %s | %s | %s | %d | %d | %.2f | %.2f'
          % (nh, nh * G, room, cell('digitize'), cell('reduce'), cell('found'), cell('traces'), bytes_found, bytes_traces, med('digitize') + med('traces'),
             med('digitize') + med('reduce') + med('found')), flush=True)
    # what the reduction makes of the truth
    offsets = per_trace[0].astype(np.int64)
    has = np.diff(offsets) > 0
    first = offsets[:-1][has]
    hit_offsets = d_hit_offsets[:nt + 1].get().astype(np.int64)
    trig_bin = d_trig_bin[:nt].get().astype(np.int64)
    of = np.repeat(np.arange(nt), np.diff(hit_offsets))
    q_true = d_hits[2][:nh].get().astype(np.float64) * charge_unit
    t_true = d_hits[3][:nh].get().view(np.float32).astype(np.float64)
    q_reco = np.add.reduceat(found[4].astype(np.float64), first) / (reducer.N * reducer.polarity * reducer.gain) if len(first) else np.zeros(0)
    t_reco = window.t0 + window.dt * (trig_bin[of[has]] - trigger.pre + found[5][first].astype(np.float64) / 256.0)
    ratio, delta = q_reco / q_true[has], t_reco - t_true[has]
    spread = lambda x: 'mean %.4g, 5 %% %.4g, 50 %% %.4g, 95 %% %.4g' % ((x.mean(),) + tuple(np.percentile(x, (5, 50, 95)))) if len(x) else 'none'
    print('# traces with a found pulse: %d of %d (%.4f); busy baselines %d; pulses with TIME_AT_EDGE %d, OPEN_AT_START %d, OPEN_AT_END %d'
          % (has.sum(), nh, has.mean(), int((per_trace[2] != 0).sum()), int((found[6] & 1 != 0).sum()), int((found[6] & 2 != 0).sum()), int((found[6] & 4 != 0).sum())))
    print('# q_reco / q_true: %s' % spread(ratio))
    print('# t_reco - t_first, ns: %s' % spread(delta), flush=True)
    del keep


if __name__ == '__main__':
    main()
