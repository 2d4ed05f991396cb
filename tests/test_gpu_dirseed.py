"""The direction seed on the device: chroma_direction_seed == chroma_direction_seed_host == the restatement of
tests/test_dirseed_host.py on its case table, every output and cos_hist, between sentinel words; a batch cut into several launches of
every kernel; scratch reuse across calls of different sizes; two threads on one handle; what the header refuses; GPUDirectionSeeder
against DirectionSeeder on the host, with the rows uploaded and handed over from the vertex seed on the device; and
Simulation(daq_direction=...) and chroma-sim --daq-direction against EventTriggers.direction on the host.  No physical accuracy is
asserted on simulated light."""
import ctypes
import threading

import numpy as np
import pytest

from chroma_amd import _lib, event
from test_dirseed_host import (CASES, CASES_BY_NAME, CHROMA_ERR_INVALID, GUARD, SENTINEL, case_arrays, check_outputs, output_sizes, python_layer_fixture,
                               refusals, refused_call, small_case, struct_of, timing_struct)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


def device_call(gpu, seeder, timing, args, out_sizes):
    """chroma_direction_seed on the host arrays ``args`` (case_arrays order; None stays NULL): (rc, the guarded output arrays read back)"""
    from chroma_amd.gpu.tools import to_gpu
    ctx = gpu.get_context()
    up = lambda a: None if a is None else to_gpu(a if len(a) else np.zeros(1, dtype=a.dtype), ctx=ctx)
    p = lambda d: None if d is None else ctypes.c_void_p(d.ptr)
    nchannels, channel_pos, ncand, cand, nfits, offsets, tau0, vertex, bin, hit_channel, hit_time, hit_weight = args
    d_in = [up(a) for a in (channel_pos, cand, vertex, bin, hit_channel, hit_time, hit_weight)]
    d_out = [None if n is None else to_gpu(np.full(n + 2 * GUARD, SENTINEL, dtype=np.uint32), ctx=ctx) for n in out_sizes]
    behind_guard = lambda d: None if d is None else ctypes.c_void_p(d.ptr + 4 * GUARD)
    s = None if seeder is None else ctypes.byref(struct_of(seeder))
    t = None if timing is None else ctypes.byref(timing_struct(timing))
    rc = ctx._lib.chroma_direction_seed(ctx.handle, s, t, nchannels, p(d_in[0]), ncand, p(d_in[1]), nfits, _lib.ptr(offsets), _lib.ptr(tau0), p(d_in[2]), p(d_in[3]),
                                        p(d_in[4]), p(d_in[5]), p(d_in[6]), *[behind_guard(d) for d in d_out])
    return rc, [None if d is None else d.get() for d in d_out]


def run_case(gpu, case, cos_hist=True):
    sizes = output_sizes(case, cos_hist)
    rc, out = device_call(gpu, case['seeder'], case['timing'], case_arrays(case), sizes)
    assert rc == 0, gpu.get_context()._lib.chroma_last_error()
    check_outputs(case, out, sizes, 'device')


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_the_call_is_the_restatement(gpu, case):
    run_case(gpu, case)


def test_consecutive_calls_of_different_sizes_reuse_the_scratch(gpu):
    for name in ('random_65fits', 'weights', 'random_sizes', 'no_hits', 'random_65fits'):
        run_case(gpu, CASES_BY_NAME[name], cos_hist=name != 'weights')


@pytest.mark.parametrize('blocks', [7, 2])
def test_a_batch_cut_into_several_launches_is_the_restatement(gpu, monkeypatch, blocks):
    """65 fits of 3 blocks each at level 0 (17 candidates) and 2509 hits (10 blocks of records): with 7 blocks to a launch two fits a
    launch at level 0 (33 launches), 10 launches of the refinement and 2 of the records; with 2 -- fewer than a fit's -- a fit a
    launch, 33 of the refinement and 5 of the records; the nine fits of up to 1025 hits likewise"""
    monkeypatch.setenv('CHROMA_SEED_LAUNCH_BLOCKS', str(blocks))
    run_case(gpu, CASES_BY_NAME['random_65fits'])
    run_case(gpu, CASES_BY_NAME['random_sizes'])


def test_two_threads_on_one_handle(gpu):
    ctx = gpu.get_context()
    errors = []

    def work(names):
        try:
            with ctx.bound():
                for _ in range(4):
                    for name in names:
                        run_case(gpu, CASES_BY_NAME[name])
        except BaseException as e:          # (an assertion of the thread is the test's)
            errors.append(e)

    threads = [threading.Thread(target=work, args=(names,)) for names in (('random_7cand', 'window'), ('random_64cand', 'levels_8'))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize('name,change', refusals(), ids=[r[0] for r in refusals()])
def test_refusals_write_nothing(gpu, name, change):
    case, d = refused_call(change)
    d['out'] = [None if a is None else len(a) - 2 * GUARD for a in d['out']]
    rc, out = device_call(gpu, d['seeder'], d['timing'], d['args'], d['out'])
    assert rc == CHROMA_ERR_INVALID, name
    assert all(a is None or np.all(a == SENTINEL) for a in out), name


def test_no_fits_and_a_call_without_times(gpu):
    case = small_case()
    sizes = output_sizes(case)
    args = list(case_arrays(case))
    args[4] = 0
    rc, out = device_call(gpu, case['seeder'], case['timing'], args, sizes)
    assert rc == 0 and all(np.all(a == SENTINEL) for a in out)
    args = list(case_arrays(case))
    args[6] = args[8] = args[10] = None          # (without times neither the timing nor tau0 nor the bins are needed)
    rc, out = device_call(gpu, case['seeder'], None, args, sizes)
    assert rc == 0
    check_outputs(dict(case, name='small_untimed', hit_time=None), out, sizes, 'device')


def same_fits(a, b, cos_hist=True):
    for name in ('dir', 'dir_int', 'score', 'cand', 'level_score', 'inside', 'outside', 'nhits') + (('cos_hist',) if cos_hist else ()):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize('prompt_ns', [(1.0, 2.5), None])
def test_gpu_direction_seeder_is_fit_many_on_the_host_uploaded_and_handed_over(gpu, prompt_ns):
    from chroma_amd.gpu.seed import GPUDirectionSeeder, GPUVertexSeeder
    seeder, offsets, channel, t, w = python_layer_fixture(prompt_ns)
    seeds = seeder.vertex_seeder.fit_many(offsets, channel, t, w)
    host = seeder.fit_many(seeds, offsets, channel, t, w, cos_hist=True)
    assert host.inside.sum() > 0
    vertex_runner = GPUVertexSeeder(gpu.get_context(), seeder.vertex_seeder)
    runner = GPUDirectionSeeder(gpu.get_context(), seeder, vertex=vertex_runner)
    assert runner.channel_pos is vertex_runner.channel_pos
    for dev in (runner.fit_many(seeds, offsets, channel, t, w, cos_hist=True), seeder.fit_many(seeds, offsets, channel, t, w, gpu=runner, cos_hist=True),
                seeder.fit_many(seeds, offsets, channel, t, w, gpu=gpu.get_context(), cos_hist=True)):
        same_fits(dev, host)
    # the vertex seed, then the direction seed about it on what the first left on the device
    dev_seeds, handed = runner.fit_both(vertex_runner, offsets, channel, t, w, cos_hist=True)
    for name in ('pos', 't0', 'score', 'bin', 'cand', 'level_score', 'outside', 'nhits', 'pos_int'):
        assert np.array_equal(getattr(dev_seeds, name), getattr(seeds, name)), name
    same_fits(handed, host)
    # its default stays what it was
    assert isinstance(vertex_runner.run(seeder.vertex_seeder.prepare(offsets, channel, t, w)), list)
    none, nothing = runner.fit_both(vertex_runner, [0], [], [], [])
    assert len(none) == 0 and len(nothing) == 0 and len(seeder.fit_many(none, [0], [], [], gpu=runner)) == 0


def test_simulation_seeds_every_firing_s_direction_as_the_host_does(gpu, tiny_geometry, tmp_path):
    from conftest import bomb
    from chroma_amd.gpu import tools
    from chroma_amd.seed import DirectionSeeder, DirFits, VertexSeeder
    from chroma_amd.sim import Simulation
    previous = tools._current
    window = (-8.0, 0.5, 512)
    trigger = gpu.DaqTrigger(2, 16, 64, 8, 40)
    digitizer = gpu.DaqDigitizer.biexponential(30.0, 1.0, 6.0, 0.5, bits=12, pedestal=150, noise_sigma=2.0)
    reducer = gpu.DaqReducer.for_digitizer(digitizer, 8, lead=2, lag=6, nbaseline=4, min_width=2, time_offset_ns=0.75)
    seeder = VertexSeeder.for_detector(tiny_geometry, 200.0, levels=3, weights='npe')
    direction = DirectionSeeder(seeder, profile=DirectionSeeder.cherenkov_profile(0.75, 0.2, fill=0.1), grid=4, levels=3, prompt_ns=(2.0, 6.0))
    try:
        with pytest.raises(ValueError):
            Simulation(tiny_geometry, seed=21, daq_direction=direction)
        firings = 0
        for reduced in (True, False):
            batch = [bomb(n, seed=300 + k) for k, n in enumerate([400, 1, 3000, 64])]
            batch.insert(2, event.Photons())
            sim = Simulation(tiny_geometry, seed=21, daq_seeder=seeder if reduced else None, daq_direction=direction if reduced else None)
            kw = dict(daq_digitizer=digitizer, daq_reducer=reducer) if reduced else dict(daq_seeder=seeder, daq_direction=direction)
            source = 'reco' if reduced else 'gate'
            events = list(sim.simulate(batch, run_daq=True, max_steps=100, daq_window=window, daq_trigger=trigger, **kw))
            with pytest.raises(ValueError):
                list(Simulation(tiny_geometry, seed=21).simulate([bomb(10, seed=1)], run_daq=True, daq_window=window, daq_trigger=trigger, daq_direction=direction))
            del sim
            for ev in events:
                t = ev.triggers
                assert isinstance(t.directions, DirFits) and len(t.directions) == len(t) == len(t.vertices)
                for k in range(len(t)):
                    vertex = t.seed(k, seeder, source=source)
                    assert np.array_equal(t.vertices.pos_int[k:k + 1], vertex.pos_int) and np.array_equal(t.vertices.bin[k:k + 1], vertex.bin)
                    same_fits(t.directions[k:k + 1], t.direction(k, direction, vertex, source=source), cos_hist=False)
                firings += len(t)
        assert firings >= 2
        # a (cos_c, sigma, fill, levels) in place of a DirectionSeeder, without a reducer: the batch's directions in one host call
        sim = Simulation(tiny_geometry, seed=21)
        batch = [bomb(n, seed=300 + k) for k, n in enumerate([400, 3000])]
        events = list(sim.simulate(batch, run_daq=True, max_steps=100, daq_window=window, daq_trigger=trigger, daq_seeder=seeder, daq_direction=(0.75, 0.2, 0.1, 2)))
        made = sim._direction_of[1]
        del sim
        assert made.levels == 2 and made.vertex_seeder is seeder and made.profile.tolist() == DirectionSeeder.cherenkov_profile(0.75, 0.2, 0.1)
        assert sum(len(ev.triggers) for ev in events) >= 1
        for ev in events:
            for k in range(len(ev.triggers)):
                same_fits(ev.triggers.directions[k:k + 1], ev.triggers.direction(k, made, ev.triggers.vertices[k:k + 1], source='gate'), cos_hist=False)
        # chroma-sim --daq-direction: a direction per firing beside the seeds
        from chroma_amd import cli
        path = str(tmp_path / 'direction.npz')
        assert cli.main(['@chroma_amd.demo.tiny', '-n', '2', '--nphotons', '900', '-s', '4', '--max-steps', '100', '--daq-window=-8,0.5,512', '--daq-trigger',
                         '2,16,64,8,40', '--daq-seed', '200,500,2', '--daq-direction', '0.75,0.2,0.1,2', '-o', path]) == 0
        saved = np.load(path)
        cli_seeder = VertexSeeder.of((200.0, 500.0, 2), tiny_geometry)
        cli_direction = DirectionSeeder.of((0.75, 0.2, 0.1, 2), cli_seeder)
        nseeds = 0
        for k in range(2):
            rows = [saved['ev%d/trigger_hit_%s' % (k, name)] for name in ('offsets', 'channel', 't', 'npe')]
            seeds = cli_seeder.fit_many(*rows)
            want = cli_direction.fit_many(seeds, *rows)
            assert np.array_equal(saved['ev%d/seed_pos' % k], seeds.pos) and len(seeds) == len(saved['ev%d/trigger_bin' % k])
            for name, column in (('dir_dir', want.dir), ('dir_score', want.score), ('dir_inside', want.inside), ('dir_outside', want.outside),
                                 ('dir_level_score', want.level_score)):
                assert np.array_equal(saved['ev%d/%s' % (k, name)], column), (k, name)
            nseeds += len(seeds)
        assert nseeds >= 1
    finally:
        tools._current = previous
