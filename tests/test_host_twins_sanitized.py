"""The seven host twins under sanitizers, as a stand-alone program (no GPU; nothing is loaded into Python, nothing preloaded).

The twins (steps_host, particles_host, daq_noise_host, daq_digitize_host, daq_reduce_host, seed_host, dirseed_host .cpp) share
their arithmetic with the device through the *_common.h headers.  GPU code cannot be sanitised, so those headers compiled for
the host are the sanitizer coverage the device arithmetic gets.  tests/host_twin_check.cpp and the seven units are built twice
with the host compiler, once per module:

    -O2
    -O1 -g -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all

both with -std=c++17 -ffp-contract=off.  float-cast-overflow is named because GCC's -fsanitize=undefined does not include it,
and a float -> integer cast out of range is the undefined arithmetic these headers are most likely to hold.

The cases are the host tests' own.  For the length of this module every call of a twin through the library (``_lib.load()``) is
also a case of the program: ``Recorder`` writes the call's arguments -- scalars, arrays, structs and the arrays their members
point to, as they stand before the call -- into a case file (the format is in host_twin_check.cpp), lets the library's twin run,
runs both programs on the file and asserts of each: exit status 0, an empty stderr (no sanitizer report), the twin's status
and every array and struct byte for byte what the library's twin left.  The host tests hold the library's twin to their
restatements; they run here again, unchanged, with that check under every call.  Arrays are found by the addresses
``_lib.ptr`` handed out, so a blob has exactly its array's size and a read or write behind its end is the sanitizer's.

Then one set per family at the extremes its header admits (the ``test_extremes_*``), where undefined arithmetic would sit.
"""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from chroma_amd import _lib
from conftest import ROOT

import test_seed_host as SEED
import test_dirseed_host as DIR
import test_daq_noise_host as NOISE
import test_daq_digitize_host as DIGITIZE
import test_daq_reduce_host as REDUCE
import test_steps_host as STEPS
import test_steps_media_host as MEDIA
import test_particles_host as PARTICLES
from test_gpu_photon_arrays import host_geos, daq_tables          # noqa: F401
from test_daq_noise_host import noise_cases          # noqa: F401
from test_steps_host import cherenkov, scintillation          # noqa: F401
from test_steps_media_host import media, case          # noqa: F401
from signed_charge import signed_geos, WINDOW          # noqa: F401

UNITS = ('steps_host', 'particles_host', 'daq_noise_host', 'daq_digitize_host', 'daq_reduce_host', 'seed_host', 'dirseed_host')
TWINS = ('chroma_vertex_seed_host', 'chroma_direction_seed_host', 'chroma_daq_noise_host', 'chroma_daq_digitize_host', 'chroma_daq_reduce_host',
         'chroma_steps_count_host', 'chroma_steps_generate_host', 'chroma_steps_count_media_host', 'chroma_steps_generate_media_host',
         'chroma_particles_advance_host', 'chroma_particles_track_host', 'chroma_particles_points_host', 'chroma_particles_segments_host')
FLAGS = {'plain': ['-O2'],
         'sanitized': ['-O1', '-g', '-fsanitize=address,undefined,float-cast-overflow', '-fno-sanitize-recover=all']}


def build_programs(directory):
    """{'plain': path, 'sanitized': path} of host_twin_check built over the seven units."""
    compiler = shutil.which('c++') or shutil.which('g++')
    command = [compiler] if compiler else ['/opt/rocm/bin/hipcc', '-x', 'c++']          # (what builds the library's host units)
    csrc = os.path.join(ROOT, 'chroma_amd', 'csrc')
    sources = [os.path.join(csrc, unit + '.cpp') for unit in UNITS]
    programs = {}
    for which, flags in FLAGS.items():
        programs[which] = os.path.join(str(directory), 'host_twin_check_' + which)
        subprocess.run(command + ['-std=c++17', '-ffp-contract=off'] + flags + ['-pthread', os.path.join(ROOT, 'tests', 'host_twin_check.cpp')] + sources +
                       ['-o', programs[which], '-lm'], check=True, timeout=600)
    return programs


class Recorder(object):
    """Every call of a twin through the library, made again by the stand-alone programs and compared."""

    def __init__(self, lib, programs, directory):
        self.lib, self.programs, self.directory = lib, programs, str(directory)
        self.real = {name: getattr(lib, name) for name in TWINS}
        self.real_ptr = _lib.ptr
        self.arrays = {}          # address -> the array _lib.ptr was asked for (kept alive: no address is used twice)
        self.calls = dict.fromkeys(TWINS, 0)
        self.refused = dict.fromkeys(TWINS, 0)

    # ---- what the tests hand the library
    def ptr(self, arr):
        if arr is not None:
            assert arr.flags['C_CONTIGUOUS']
            known = self.arrays.get(arr.ctypes.data)
            if known is None or known.nbytes < arr.nbytes:
                self.arrays[arr.ctypes.data] = arr
        return self.real_ptr(arr)

    def owner(self, address):
        """(array, offset) of an address ``_lib.ptr`` handed out, or of one inside such an array"""
        arr = self.arrays.get(address)
        if arr is not None:
            return arr, 0
        for base, arr in self.arrays.items():
            if base < address < base + arr.nbytes:
                return arr, address - base
        raise AssertionError('a pointer to memory that _lib.ptr did not hand out: 0x%x' % address)

    # ---- a call as a case file
    class Case(object):
        def __init__(self):
            self.blobs, self.index, self.relocs, self.slots = [], {}, [], []          # blobs: (object, its bytes before the call, pointer offsets)

    def blob_of_array(self, case, arr):
        key = ('a', arr.ctypes.data, arr.nbytes)
        if key not in case.index:
            case.index[key] = len(case.blobs)
            case.blobs.append((arr, arr.tobytes(), ()))
        return case.index[key]

    def pointer_fields(self, kind, base=0):
        """the offsets of the pointer members of a ctypes type"""
        if isinstance(kind, type) and issubclass(kind, ctypes.Structure):
            out = []
            for field in kind._fields_:
                out += self.pointer_fields(field[1], base + getattr(kind, field[0]).offset)
            return out
        if kind is ctypes.c_void_p:
            return [base]
        assert not (isinstance(kind, type) and issubclass(kind, ctypes._Pointer)), 'a typed pointer member'
        return []

    def raw(self, obj, pointers):
        data = bytearray(ctypes.string_at(ctypes.addressof(obj), ctypes.sizeof(obj)))
        for offset in pointers:
            data[offset:offset + 8] = bytes(8)
        return bytes(data)

    def blob_of_object(self, case, obj):
        key = ('o', ctypes.addressof(obj))
        if key not in case.index:
            pointers = self.pointer_fields(type(obj))
            case.index[key] = b = len(case.blobs)
            case.blobs.append((obj, self.raw(obj, pointers), tuple(pointers)))
            for offset in pointers:
                address = ctypes.c_uint64.from_address(ctypes.addressof(obj) + offset).value
                if address:
                    arr, inside = self.owner(address)
                    case.relocs.append((b, offset, self.blob_of_array(case, arr), inside))
        return case.index[key]

    def record(self, name, args):
        fn = self.real[name]
        assert len(args) == len(fn.argtypes), name
        case = self.Case()
        for kind, arg in zip(fn.argtypes, args):
            if issubclass(kind, ctypes._Pointer):
                if arg is None:
                    case.slots.append(None)
                    continue
                obj = arg._obj if hasattr(arg, '_obj') else (arg.contents if isinstance(arg, ctypes._Pointer) else arg)
                assert isinstance(obj, kind._type_), (name, kind, arg)
                case.slots.append((self.blob_of_object(case, obj), 0))
            elif kind is ctypes.c_void_p:
                address = arg.value if isinstance(arg, ctypes.c_void_p) else arg
                if not address:
                    case.slots.append(None)
                else:
                    arr, inside = self.owner(int(address))
                    case.slots.append((self.blob_of_array(case, arr), inside))
            elif kind is ctypes.c_float:
                case.slots.append(struct.unpack('<I', struct.pack('<f', float(arg)))[0])
            elif kind is ctypes.c_double:
                case.slots.append(struct.unpack('<Q', struct.pack('<d', float(arg)))[0])
            else:
                value = kind(int(arg.value if hasattr(arg, 'value') else arg)).value          # (as ctypes converts it)
                case.slots.append(value & 0xffffffffffffffff)
        return case

    def write(self, name, case, path):
        out = [b'TWINCALL', struct.pack('<I', len(name)), name.encode(), struct.pack('<I', len(case.blobs))]
        for _, data, _ in case.blobs:
            out += [struct.pack('<Q', len(data)), data]
        out.append(struct.pack('<I', len(case.relocs)))
        out += [struct.pack('<IQIQ', *r) for r in case.relocs]
        out.append(struct.pack('<I', len(case.slots)))
        for slot in case.slots:
            out.append(b'\x02' if slot is None else struct.pack('<BQ', 0, slot) if isinstance(slot, int) else struct.pack('<BIQ', 1, *slot))
        with open(path, 'wb') as f:
            f.write(b''.join(out))

    def after(self, case):
        """the blobs as the library's twin left them"""
        return [obj.tobytes() if isinstance(obj, np.ndarray) else self.raw(obj, pointers) for obj, _, pointers in case.blobs]

    def proxy(self, name):
        def call(*args):
            case = self.record(name, args)
            path = os.path.join(self.directory, 'case.bin')
            self.write(name, case, path)
            status = self.real[name](*args)
            want = self.after(case)
            self.calls[name] += 1
            self.refused[name] += status != 0
            what = '%s, call %d' % (name, self.calls[name])
            for which, program in self.programs.items():
                out = os.path.join(self.directory, 'out_%s.bin' % which)
                run = subprocess.run([program, path, out], capture_output=True, text=True, timeout=600)
                assert run.returncode == 0 and run.stderr == '', '%s, %s: exit status %d\n%s' % (what, which, run.returncode, run.stderr[-4000:])
                with open(out, 'rb') as f:
                    data = f.read()
                assert len(data) == 4 + sum(len(w) for w in want), '%s, %s: %d bytes written' % (what, which, len(data))
                assert struct.unpack('<i', data[:4])[0] == status, '%s, %s: status %d, the library twin\'s %d' % (what, which, struct.unpack('<i', data[:4])[0], status)
                at = 4
                for b, w in enumerate(want):
                    assert data[at:at + len(w)] == w, '%s, %s: blob %d (%d bytes) is not what the library twin left' % (what, which, b, len(w))
                    at += len(w)
            return status
        call.argtypes, call.restype = self.real[name].argtypes, self.real[name].restype
        return call


@pytest.fixture(scope='module')
def programs(tmp_path_factory):
    return build_programs(tmp_path_factory.mktemp('host_twin_check'))


@pytest.fixture(scope='module', autouse=True)
def recorder(programs, tmp_path_factory):
    """Installed before any other fixture of this module runs: the twins the fixtures call are cases too."""
    lib = _lib.load()
    r = Recorder(lib, programs, tmp_path_factory.mktemp('host_twin_cases'))
    with pytest.MonkeyPatch.context() as patch:
        patch.setattr(_lib, 'ptr', r.ptr)
        for name in TWINS:
            patch.setattr(lib, name, r.proxy(name))
        yield r


def made(recorder, names, calls, refused=0):
    """the calls a test made through the programs, by twin: at least ``calls`` of each, ``refused`` refusals in all"""
    def check(before):
        for name in names:
            assert recorder.calls[name] - before[0][name] >= calls, '%s: %d calls' % (name, recorder.calls[name] - before[0][name])
        assert sum(recorder.refused[name] - before[1][name] for name in names) >= refused
    return (dict(recorder.calls), dict(recorder.refused)), check


# ---- the existing case tables, family by family ------------------------------------------------------------------------------------
def test_vertex_seed_cases_and_refusals(recorder):
    before, check = made(recorder, ['chroma_vertex_seed_host'], len(SEED.CASES) + len(SEED.refusals()), len(SEED.refusals()))
    for c in SEED.CASES:
        SEED.test_host_twin_is_the_restatement(c)
    SEED.test_host_twin_without_scores()
    for name, change in SEED.refusals():
        SEED.test_host_refusals_write_nothing(name, change)
    SEED.test_host_refuses_a_null_seeder_and_too_many_scores()
    SEED.test_no_fits_is_ok_and_writes_nothing()
    check(before)


def test_direction_seed_cases_and_refusals(recorder):
    before, check = made(recorder, ['chroma_direction_seed_host'], len(DIR.CASES) + len(DIR.refusals()), len(DIR.refusals()))
    for c in DIR.CASES:
        DIR.test_host_twin_is_the_restatement(c)
    DIR.test_host_twin_without_cos_hist()
    for name, change in DIR.refusals():
        DIR.test_host_refusals_write_nothing(name, change)
    DIR.test_the_small_call_is_valid_and_no_fits_write_nothing()
    check(before)


@pytest.mark.parametrize('which', ['tiny', 'stress'])
def test_noise_cases(recorder, host_geos, noise_cases, which):
    before, check = made(recorder, ['chroma_daq_noise_host'], len([c for c in NOISE.ALL_CASES if c[0] == which]))
    NOISE.test_the_host_twin_is_the_restatement(host_geos, noise_cases, which)
    check(before)


def test_noise_refusals(recorder, host_geos):
    before, check = made(recorder, ['chroma_daq_noise_host'], 10, 10)
    NOISE.test_the_host_twin_refuses_what_the_header_says(host_geos)
    check(before)


def test_digitiser_cases_and_refusals(recorder):
    before, check = made(recorder, ['chroma_daq_digitize_host'], 20, len(DIGITIZE.refusals()))
    for which in range(5):
        DIGITIZE.test_the_host_twin_and_digitize_are_the_restatement_on_the_trigger_sets(which)
    DIGITIZE.test_the_host_twin_and_digitize_are_the_restatement_on_the_handmade_sets()
    DIGITIZE.test_saturation_sets_exactly_the_flags_expected()
    DIGITIZE.test_the_sum_wraps_in_64_bits()
    DIGITIZE.test_unit_taps_give_the_clipped_charge_counts_of_the_waveform()
    DIGITIZE.test_row_r_of_a_call_is_row_0_of_a_call_with_acquisition_plus_r()
    DIGITIZE.test_a_slice_is_that_part_of_the_whole()
    DIGITIZE.test_a_channel_outside_the_detector_and_a_trigger_in_no_row_have_no_signal()
    DIGITIZE.test_the_host_twin_refuses_what_the_header_says_and_writes_nothing()
    check(before)


def test_reducer_cases_and_refusals(recorder):
    before, check = made(recorder, ['chroma_daq_reduce_host'], 20, len(REDUCE.refusals()))
    REDUCE.test_the_host_twin_is_the_restatement_on_the_digitised_trigger_sets()
    for index in range(len(REDUCE.handmade())):
        REDUCE.test_the_host_twin_and_the_package_are_the_restatement_on_the_handmade_traces(index)
    for index in range(3):
        REDUCE.test_the_integral_of_a_full_scale_trace_of_65536_samples_needs_its_64_bits(index)
    REDUCE.test_the_twin_and_the_package_are_the_restatement_on_300_random_traces()
    REDUCE.test_the_host_twin_refuses_what_the_header_says_and_writes_nothing()
    REDUCE.test_too_little_room_writes_the_count_and_the_per_trace_arrays_and_leaves_the_pulse_arrays()
    REDUCE.test_no_traces_is_ok_and_writes_nothing_but_the_count()
    check(before)


def test_step_light_cases(recorder, cherenkov, scintillation):
    before, check = made(recorder, ['chroma_steps_count_host', 'chroma_steps_generate_host'], 3, 1)
    STEPS.test_counts_are_those_of_the_restatement_bit_for_bit()
    STEPS.test_cherenkov_count_sum_follows_frank_tamm()
    STEPS.test_no_cherenkov_light_below_threshold_without_charge_or_length()
    STEPS.test_cherenkov_photons_are_those_of_the_restatement(cherenkov)
    STEPS.test_scintillation_count_sums(scintillation)
    STEPS.test_batching_does_not_change_the_photons()
    STEPS.test_capacity_and_bad_sources_are_refused()
    check(before)


def test_step_light_media_cases(recorder, media, case):
    before, check = made(recorder, ['chroma_steps_count_media_host', 'chroma_steps_generate_media_host'], 3, 4)
    MEDIA.test_each_segment_emits_what_its_mediums_source_emits(media, case)
    MEDIA.test_two_calls_with_consecutive_bases_give_the_same_photons(media, case)
    MEDIA.test_no_segments(media)
    MEDIA.test_a_bad_table_is_refused_with_a_message(case)
    check(before)


def test_particle_cases(recorder):
    from chroma_amd.demo.optics import water
    from chroma_amd.geometry import Material
    # (chroma_particles_segments_host has no caller among the host tests: test_extremes_particles calls it)
    before, check = made(recorder, ['chroma_particles_advance_host', 'chroma_particles_track_host', 'chroma_particles_points_host'], 1)
    stopping, two =PARTICLES.P.StoppingMedia([water]), PARTICLES.P.StoppingMedia([water, Material('vacuum')])
    for scatter in (False, True):
        PARTICLES.test_tracks_keep_the_step_rules(stopping, scatter)
    PARTICLES.test_tracks_do_not_depend_on_the_split_into_calls(stopping)
    PARTICLES.test_edge_boundary_at_zero_and_at_the_physics_step(two)
    PARTICLES.test_edge_leaving(two)
    PARTICLES.test_edge_the_energy_cut(two)
    PARTICLES.test_edge_untracked_truncated_and_nan(two)
    PARTICLES.test_segments_feed_the_light_source(stopping)
    check(before)


# ---- one set per family at the extremes its header admits ----------------------------------------------------------------------------
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
TOP = 2 ** 23


def ends_of_int32(channels):
    return [(c, t, 255) for c in range(channels) for t in (INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX)]


def test_extremes_vertex_seed(recorder):
    """Coordinates at +-2^23 under the greatest step (2^21) and 8 levels, slowness 2^24 (a flight of 2^33 ticks), bins of 2^20
    ticks times 1024, times and tau0 at the ends of int32, and 65535 hits of weight 255 in one bin under sixteen 255s."""
    corners = [(x, y, z) for x in (-TOP, TOP) for y in (-TOP, TOP) for z in (-TOP, TOP)]
    widest = SEED.seeder_of(slowness=2 ** 24, bin_ticks=2 ** 20, nbins=1024, shape=[255] * 16, step=2 ** 21, nlevels=8)
    cand = [(TOP, TOP, TOP), (-TOP, -TOP, -TOP), (0, 0, 0), (TOP, -TOP, 0)]
    fits = [(tau0, ends_of_int32(8)) for tau0 in (INT32_MIN, INT32_MAX, 0, -1)]
    before, check = made(recorder, ['chroma_vertex_seed_host'], 4)
    rc, out, sizes = SEED.call_host(SEED.case_of('extremes', widest, corners, cand, fits))
    assert rc == 0
    assert out[1][:4].max() > 0, 'no fit scores: the extremes put every hit outside'
    # the slowest clock against the fastest: one tick a bin, and slowness 1
    for slowness, bin_ticks in ((1, 1), (2 ** 24, 1), (1, 2 ** 20)):
        p = SEED.seeder_of(slowness=slowness, bin_ticks=bin_ticks, nbins=1024, shape=[255] * 16, step=2 ** 21, nlevels=8)
        assert SEED.call_host(SEED.case_of('extremes', p, corners, cand, fits))[0] == 0
    # the fullest bin: 65535 hits of weight 255 under a shape of sixteen 255s (255 * 255 * 65535 < 2^32), one level
    full = SEED.seeder_of(slowness=2 ** 24, bin_ticks=2 ** 20, nbins=1024, shape=[255] * 16, step=2 ** 21, nlevels=1)
    rc, out, sizes = SEED.call_host(SEED.case_of('full', full, corners[:1], [corners[0]], [(INT32_MIN, [(0, INT32_MIN, 2 ** 32 - 1)] * 65535)]))
    assert rc == 0 and out[1][0] == 255 * 255 * 65535 and out[4][0] == 0
    # beyond the header: refused, nothing written
    for field, value in (('step', 2 ** 21 + 1), ('nlevels', 9), ('slowness', 2 ** 24 + 1), ('bin_ticks', 2 ** 20 + 1), ('nbins', 1025)):
        case = SEED.case_of('beyond', dict(widest, **{field: value}), corners, cand, fits)
        rc, out, sizes = SEED.call_host(case)
        assert rc == SEED.CHROMA_ERR_INVALID and all(np.all(a == SEED.SENTINEL) for a in out), field
    check(before)


def test_extremes_direction_seed(recorder):
    """The vertex seed's extremes through the direction seed: vertices and channels at +-2^23, candidates at +-2^15, the greatest
    step (2^13) under 8 levels, 256 cosine bins of 255, the timing cut with slowness 2^24 and bins of 2^20 ticks, times, tau0 and
    the bin word at their ends, and 65535 hits of weight 255."""
    corners = [(x, y, z) for x in (-TOP, TOP) for y in (-TOP, TOP) for z in (-TOP, TOP)]
    big = [(2 ** 15, -2 ** 15, 2 ** 15), (-2 ** 15, 2 ** 15, -2 ** 15), (2 ** 15, 0, 0), (0, 0, -2 ** 15), (1, 0, 0)]
    timing = DIR.timing_of(slowness=2 ** 24, bin_ticks=2 ** 20, nbins=1024)
    before, check = made(recorder, ['chroma_direction_seed_host'], 4)
    for first, width in ((0, 1), (0, 2048), (1023, 2048)):
        seeder = DIR.seeder_of(log2_ncos=8, step=2 ** 13, nlevels=8, first=first, width=width, profile=[255] * 256)
        fits = [(v, tau0, b, ends_of_int32(8)) for v in (corners[0], corners[7], (0, 0, 0)) for tau0, b in ((INT32_MIN, 0), (INT32_MAX, 2 ** 32 - 1), (0, 1023))]
        rc, out, sizes = DIR.call_host(DIR.case_of('extremes', seeder, corners, big, fits, timing))
        assert rc == 0
        rc, out, sizes = DIR.call_host(DIR.case_of('extremes_untimed', seeder, corners, big, fits))
        assert rc == 0 and DIR.body(out[1], len(fits)).max() > 0
    full = DIR.seeder_of(log2_ncos=8, step=2 ** 13, nlevels=1, profile=[255] * 256)
    rc, out, sizes = DIR.call_host(DIR.case_of('full', full, corners[:2], big[:1], [(corners[0], 0, 0, [(1, 0, 2 ** 32 - 1)] * 65535)]))
    assert rc == 0 and DIR.body(out[1], 1)[0] == 255 * 255 * 65535
    for field, value in (('step', 2 ** 13 + 1), ('nlevels', 9), ('log2_ncos', 9)):
        seeder = dict(DIR.seeder_of(log2_ncos=8, step=2 ** 13, nlevels=8, profile=[255] * 256), **{field: value})
        rc, out, sizes = DIR.call_host(DIR.case_of('beyond', seeder, corners, big, [(corners[0], 0, 0, ends_of_int32(8))]))
        assert rc == DIR.CHROMA_ERR_INVALID and all(a is None or np.all(a == DIR.SENTINEL) for a in out), field
    check(before)


def test_extremes_reducer(recorder):
    """The largest baseline (64 samples) and threshold (65535) the header takes on samples of 65535 and of 0, both polarities: the
    products N * v, N * threshold and the baseline's sum at their largest; lead, lag, min_width and cfd at their ends."""
    G = 200
    high, low = np.full(G, 65535, dtype=np.uint16), np.zeros(G, dtype=np.uint16)
    step_up, step_down, comb = low.copy(), high.copy(), low.copy()
    step_up[64:], step_down[64:], comb[64::2] = 65535, 0, 65535
    adc = np.array([high, low, step_up, step_down, comb, comb[::-1]])
    before, check = made(recorder, ['chroma_daq_reduce_host'], 16, 3)
    found = 0
    for polarity in (1, -1):
        for nbaseline, pedestal in ((64, 0), (0, 65535), (0, 0), (1, 65535)):
            for threshold in (65535, 1):
                for lead, lag, min_width, cfd in ((65535, 65535, 1, 256), (0, 0, 65536, 1), (0, 0, 1, 1)):
                    r = REDUCE.Reducer('extreme', threshold, polarity=polarity, nbaseline=nbaseline, pedestal=pedestal, baseline_spread=0, min_width=min_width,
                                       lead=lead, lag=lag, cfd=cfd)
                    rc, v = REDUCE.host_reduce(adc, r, len(adc) * G)
                    assert rc == 0, r.__dict__
                    found += v['nfound'].value
    assert found > 50
    for change in ({'r.nbaseline': 65}, {'r.threshold': 65536}, {'r.threshold': 0}):
        rc, v = REDUCE.host_reduce(adc, REDUCE.Reducer('beyond', 1), len(adc) * G, change=change)
        assert rc == REDUCE.ERR_INVALID and REDUCE.untouched(v, [name for name, _ in REDUCE.PER_TRACE + REDUCE.PER_PULSE])
    check(before)


def test_extremes_digitiser(recorder):
    """Charge counts of 0xffffffff and of 0 against 1024 taps at the ends of int32, every shift and pedestal end, 1 and 16 bits."""
    rng = np.random.default_rng(5)
    ps = DIGITIZE.from_rows(1, 2, 4096, [{(0, b) for b in range(10, 1300)} | {(1, 10), (1, 1200)}], rng)
    ps.q_int[:] = np.where(np.arange(len(ps)) % 3 == 1, 0, 0xffffffff).astype(np.uint32)
    trig = (1, 1, 1400, 2, 1398)
    want = DIGITIZE.brute_of(ps, 'nhit', *trig)
    assert len(want['hit_channel']) >= 2
    taps = [np.full(1024, INT32_MIN), np.full(1024, INT32_MAX), np.where(np.arange(1024) % 2, INT32_MIN, INT32_MAX)]
    before, check = made(recorder, ['chroma_daq_digitize_host'], 12)
    seen = set()
    for t in taps:
        for shift, pedestal, bits, sigma in ((0, INT32_MAX, 16, 0.0), (31, INT32_MIN, 1, 8.0), (0, INT32_MIN, 16, 8.0), (31, 0, 16, 0.0), (16, INT32_MAX, 1, 0.0)):
            dig = DIGITIZE.Digitiser('extreme', t, shift, pedestal, bits, sigma)
            rc, adc, flags = DIGITIZE.host_rc(ps, trig, want, dig)
            assert rc == 0
            seen.update(np.unique(adc[:-8]).tolist())
    assert {0, 1, 65535} <= seen
    check(before)


def noise_rc(lib, tables, window, count_cdf, accept, nrows, nchannels, capacity, seed=NOISE.SEED, acquisition=NOISE.BASE):
    (tx, ty, qx, qy), unit = tables
    qx, qy = np.ascontiguousarray(qx), np.ascontiguousarray(qy)
    t = _lib.DaqTables(None, None, 0, _lib.ptr(qx), _lib.ptr(qy), len(qx), unit)
    win = _lib.DaqWindow(*window)
    noise = _lib.DaqNoise(_lib.ptr(count_cdf), len(count_cdf), _lib.ptr(accept), NOISE.NOISE)
    columns = [np.full(capacity + 8, 0xA5A5A5A5, dtype=np.uint32) for _ in range(5)]
    n = ctypes.c_uint64(0)
    rc = lib.chroma_daq_noise_host(ctypes.byref(t), ctypes.byref(win), ctypes.byref(noise), nrows, nchannels, seed, acquisition, capacity,
                                   *([_lib.ptr(a) for a in columns] + [ctypes.byref(n)]))
    return rc, int(n.value), columns


@pytest.mark.parametrize('kind', ['table', 'gaussian'])
def test_extremes_noise(recorder, signed_geos, kind):
    """The signed charge tables (a negative charge counts 0: the conversion that a raw cast leaves undefined), a count table of
    64 entries that word 0 climbs to its end, accept words of 0, 1, 2^31 - 1 and 2^31, one bin and 65536 bins."""
    geo = signed_geos[kind]
    lib = _lib.load()
    count_cdf = np.linspace(0, 2 ** 32 - 1, 64).astype(np.uint64).astype(np.uint32)
    accept = np.resize(np.array([0, 2 ** 31, 1, 2 ** 31 - 1, 2 ** 30, 2 ** 31], dtype=np.uint32), geo.nchannels)
    before, check = made(recorder, ['chroma_daq_noise_host'], 6, 3)
    for window in ((-1e30, 1e30, 1), (1e30, 1e-30, 65536), WINDOW):
        rc, n, columns = noise_rc(lib, daq_tables(geo), window, count_cdf, accept, 5, geo.nchannels, 0)
        assert rc == -1 and n > 500, 'no room: refused with the count'
        rc, n, columns = noise_rc(lib, daq_tables(geo), window, count_cdf, accept, 5, geo.nchannels, n)
        assert rc == 0
        channel, charge_int = columns[1][:n], columns[4][:n]
        assert not np.isin(channel, np.flatnonzero(accept == 0)).any() and np.isin(np.flatnonzero(accept == 2 ** 31), channel).all()
        assert (charge_int == 0).sum() >= 0.2 * n and (charge_int > 0).sum() >= 0.2 * n and charge_int.max() <= 65536
        assert all((a[n:] == 0xA5A5A5A5).all() for a in columns)
        words = np.bincount(columns[0][:n].astype(np.int64) * geo.nchannels + channel, minlength=5 * geo.nchannels)
        assert words.max() >= 40, 'no word climbs the count table'
    check(before)


def count_rc(source, seg, seed, medium=None):
    """chroma_steps_count_host / _media_host called directly: (rc, offsets, total).  More than 2^32 - 1 photons are refused, with
    the offsets and the total written."""
    lib = _lib.load()
    offsets = np.full(2 * len(seg) + 1, 0xA5A5A5A5, dtype=np.uint32)
    total = ctypes.c_uint64(0xA5A5A5A5)
    s = seg.struct()
    if medium is None:
        rc = lib.chroma_steps_count_host(ctypes.byref(source.struct), ctypes.byref(s), seed, _lib.ptr(offsets), ctypes.byref(total))
    else:
        medium = np.ascontiguousarray(medium, dtype=np.int32)
        rc = lib.chroma_steps_count_media_host(ctypes.byref(source.desc), ctypes.byref(s), _lib.ptr(medium), seed, _lib.ptr(offsets), ctypes.byref(total))
    assert rc == (-1 if total.value > 0xffffffff else 0)
    return rc, offsets, total.value


def test_extremes_step_light(recorder):
    """Means either side of 16 (the switch from Knuth's product to the rounded normal), means of 2^31 and beyond (the count
    saturates at 2^31 - 1; a call of more than 2^32 - 1 photons is refused), NaN and infinite beta, zero-length segments, NaN,
    negative and infinite deposits."""
    steps = STEPS.steps
    src = steps.LightSource(STEPS.medium(STEPS.SLOPED_N, spectrum=True, light_yield=1000.0, waveform=True), STEPS.WL)
    f32 = np.float32
    before, check = made(recorder, ['chroma_steps_count_host', 'chroma_steps_generate_host'], 1, 1)
    # scintillation: mean = yield * qedep
    sixteen = f32(16.0) / f32(1000.0)
    near = [np.nextafter(sixteen, f32(0)), sixteen, np.nextafter(sixteen, f32(1)), 0.0159, 0.0161, np.nan, -1.0, 0.0, -np.inf]
    beyond = [2.0 ** 31 / 1000.0, 2.2e6, 4.3e6, 1e30, 3e38, np.inf]
    segments = lambda qedep: steps.Segments(np.zeros((len(qedep), 3)), np.zeros((len(qedep), 3)) + [0.0, 0.0, 1e-3], 0.0, 1.0, 0.5, 1.0, qedep, 0)
    rc, offsets, total = count_rc(src, segments(near), STEPS.SEED)
    counts = np.diff(offsets.astype(np.int64))[1::2]
    assert rc == 0 and counts[:5].min() >= 1 and counts[:5].max() < 60 and not counts[5:].any(), counts
    for q in beyond:
        rc, offsets, total = count_rc(src, segments([q]), STEPS.SEED)
        assert rc == 0 and 2 ** 31 - 2 ** 24 <= total <= 2 ** 31 - 1, (q, total)
    rc, offsets, total = count_rc(src, segments(beyond), STEPS.SEED)
    assert rc == -1 and total > 2 ** 32
    # Cherenkov: the mean grows with the length; beta at, below and beyond every sense
    lengths = [0.0, 1e-30, 0.05, 0.08, 0.1, 1e7, 1e9, 1e30, 3e38, np.inf, np.nan]
    betas = [0.9, 1.0, np.nextafter(f32(1), f32(2)), 0.0, -0.9, np.inf, -np.inf, np.nan, 1e30, 1e-30]
    seen = set()
    for length in lengths:
        a = np.zeros((len(betas), 3))
        with np.errstate(invalid='ignore', over='ignore'):
            seg = steps.Segments(a, a + length * np.array([0.6, 0.0, 0.8]), 0.0, 1.0, betas, 1.0, 0.0, 0)
        rc, offsets, total = count_rc(src, seg, STEPS.SEED)
        counts = np.diff(offsets.astype(np.int64))[0::2]
        assert counts[3] == 0 and (length != 0.0 or total == 0), (length, counts)
        seen.update(counts.tolist())
    assert 2 ** 31 - 1 in seen and any(0 < c <= 16 for c in seen) and any(16 < c < 1000 for c in seen), sorted(seen)[:20]
    # small enough to make: photons of zero-length and of ordinary segments, a NaN beta among them
    few = steps.Segments(np.zeros((4, 3)), [[0, 0, 0], [0, 0, 0.05], [0, 0, 0.1], [0, 0, 0]], 0.0, [0.0, 1.0, 1.0, 0.0], [0.9, 0.9, 1.0, np.nan], 1.0, [0.02, 0.0, 0.017, 0.03], 0)
    assert len(steps.generate_photons(few, src, STEPS.SEED)) > 20
    check(before)


def test_extremes_step_light_media(recorder, media):
    """The same through the media table: rows inside, outside and at the ends of int32."""
    steps = MEDIA.steps
    before, check = made(recorder, ['chroma_steps_count_media_host', 'chroma_steps_generate_media_host'], 1, 1)
    qedep = [0.0, 16.0 / 120.0, 0.134, 2.0 ** 31 / 120.0, 1e30, np.inf, np.nan, 0.4]
    beta = [0.9, np.nan, np.inf, 0.99, 0.0, 1.0, -np.inf, 0.99]
    n = len(qedep)
    seg = steps.Segments(np.zeros((n, 3)), np.array([[0.0, 0.0, 0.0]] * 2 + [[0.0, 0.0, 0.08]] * (n - 2)), 0.0, 1.0, beta, 1.0, qedep, 0)
    refused = 0
    for medium in ([1] * n, [2] * n, [0, 1, 2, 3, -1, 2 ** 31 - 1, -2 ** 31, 1], [0, 0, 0, 1, 0, 0, 0, 0]):
        rc, offsets, total = count_rc(media, seg, MEDIA.SEED, medium=medium)
        refused += rc != 0
    assert 1 <= refused <= 3
    quiet = steps.Segments(np.zeros((3, 3)), [[0, 0, 0], [0, 0, 0.08], [0, 0, 0.1]], 0.0, 1.0, [0.9, 0.99, np.nan], 1.0, [0.1, 0.0, 0.134], 0)
    assert len(steps.generate_photons(quiet, media, MEDIA.SEED, medium=[1, 0, 2])) > 10
    check(before)


def test_extremes_particles(recorder):
    """Kinetic energies below the table's first node (1 keV), above its last (100 GeV), NaN and infinite; max_steps = 0 (refused);
    the tracks' segments through chroma_particles_segments_host."""
    from chroma_amd.demo.optics import water
    from chroma_amd.geometry import Material
    P = PARTICLES.P
    lib = _lib.load()
    two = P.StoppingMedia([water, Material('vacuum')], birks={'water': 0.1})
    energies = [1e-30, 1e-4, np.nextafter(np.float32(1e-3), np.float32(0)), 1e-3, 1e5, np.nextafter(np.float32(1e5), np.float32(1e6)), 1e9, 3e38, np.inf, np.nan, 0.0,
                -1.0, 100.0]
    vertices = [PARTICLES.vertex(name, ke, direction=(1, 2, 2)) for ke in energies for name in ('mu-', 'e-', 'alpha')]
    before, check = made(recorder, ['chroma_particles_advance_host', 'chroma_particles_track_host', 'chroma_particles_points_host',
                                    'chroma_particles_segments_host'], 1, 2)
    for scatter in (False, True):
        stepper = P.Stepper(two, max_steps=12, max_step=1e30, max_loss=1.0, ke_cut=0.0, scatter=scatter)
        state = P.ParticleState(vertices, evidx=7)
        options = stepper.options(outside=0)
        matrix, matrix_struct = P.point_arrays(state.n * (stepper.max_steps + 1), fill=-7)
        particles = state.struct()
        total = ctypes.c_uint64()
        assert lib.chroma_particles_track_host(ctypes.byref(two.desc), ctypes.byref(particles), ctypes.byref(options), 3, ctypes.byref(matrix_struct),
                                               ctypes.byref(total)) == 0
        assert state.n <= total.value <= state.n * 13 and len(set(state.status.tolist())) >= 3, state.status
        flat, flat_struct = P.point_arrays(total.value)
        offsets = np.zeros(state.n + 1, dtype=np.uint32)
        assert lib.chroma_particles_points_host(ctypes.byref(particles), 12, ctypes.byref(matrix_struct), ctypes.byref(flat_struct), _lib.ptr(offsets), total.value) == 0
        nseg = total.value - state.n
        twin = {name: np.zeros((nseg, 3) if name in 'ab' else nseg, np.uint32 if name == 'evidx' else np.float32) for name in ('a', 'b', 't_a', 't_b', 'beta', 'z', 'qedep', 'evidx')}
        medium = np.zeros(nseg, np.int32)
        seg = _lib.StepSegments()
        for name, a in twin.items():
            setattr(seg, name, _lib.ptr(a))
        assert lib.chroma_particles_segments_host(ctypes.byref(particles), 12, ctypes.byref(matrix_struct), ctypes.byref(seg), _lib.ptr(medium), nseg) == 0
        # one iteration more, each particle with a triangle at 0, at infinity and at NaN ahead
        for distance in (0.0, np.inf, np.nan, 1e-30):
            again = P.ParticleState(vertices)
            P.advance(again, stepper, 5, P.point_arrays(again.n * 13, fill=-7)[1], [distance] * again.n, [4] * again.n, [0, 1, -1] * len(energies))
        # max_steps = 0: refused, nothing written
        for max_steps in (0, -1):
            refused = P.ParticleState(vertices)
            options = stepper.options(outside=0)
            options.max_steps = max_steps
            points, points_struct = P.point_arrays(refused.n, fill=-7)
            particles = refused.struct()
            total = ctypes.c_uint64(99)
            assert lib.chroma_particles_track_host(ctypes.byref(two.desc), ctypes.byref(particles), ctypes.byref(options), 3, ctypes.byref(points_struct),
                                                   ctypes.byref(total)) == -1
            assert all((a == -7).all() for a in points.values()) and not refused.nsteps.any() and not refused.status.any()
    check(before)
