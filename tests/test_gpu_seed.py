"""The vertex seed on the device: chroma_vertex_seed == chroma_vertex_seed_host == the restatement of tests/test_seed_host.py on
its case sets, every output and the scores, behind sentinels; scratch reuse across calls of different sizes; two threads on one
handle; what the header refuses; and Simulation(daq_seeder=...) and chroma-sim --daq-seed against Triggers.seed on the host.  No physical accuracy is
asserted on simulated light."""
import ctypes
import threading

import numpy as np
import pytest

from chroma_amd import _lib, event
from test_seed_host import (CASES, CASES_BY_NAME, CHROMA_ERR_INVALID, GUARD, OUTPUTS, SENTINEL, case_arrays, check_outputs, output_sizes, refusals,
                            refused_call, small_case, struct_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def gpu():
    from chroma_amd import gpu as g
    ctx = g.create_cuda_context(0)
    yield g
    ctx.pop()


def device_call(gpu, seeder, args, out_sizes):
    """chroma_vertex_seed on the host arrays ``args`` (case_arrays order; None stays NULL): (rc, the guarded output arrays read back)"""
    from chroma_amd.gpu.tools import to_gpu
    ctx = gpu.get_context()
    up = lambda a: None if a is None else to_gpu(a if len(a) else np.zeros(1, dtype=a.dtype), ctx=ctx)
    p = lambda d: None if d is None else ctypes.c_void_p(d.ptr)
    nchannels, channel_pos, ncand, cand, nfits, offsets, tau0, hit_channel, hit_time, hit_weight = args
    d_in = [up(channel_pos), up(cand), up(hit_channel), up(hit_time), up(hit_weight)]
    d_out = [None if n is None else to_gpu(np.full(n + GUARD, SENTINEL, dtype=np.uint32), ctx=ctx) for n in out_sizes]
    s = struct_of(seeder)
    rc = ctx._lib.chroma_vertex_seed(ctx.handle, ctypes.byref(s), nchannels, p(d_in[0]), ncand, p(d_in[1]), nfits, _lib.ptr(offsets), _lib.ptr(tau0),
                                     p(d_in[2]), p(d_in[3]), p(d_in[4]), *[p(d) for d in d_out])
    return rc, [None if d is None else d.get() for d in d_out]


def run_case(gpu, case, scores=True):
    sizes = output_sizes(case, scores)
    rc, out = device_call(gpu, case['seeder'], case_arrays(case), sizes)
    assert rc == 0, gpu.get_context()._lib.chroma_last_error()
    check_outputs(case, out, sizes, 'device')


@pytest.mark.parametrize('case', CASES, ids=[c['name'] for c in CASES])
def test_the_call_is_the_restatement(gpu, case):
    run_case(gpu, case)


def test_consecutive_calls_of_different_sizes_reuse_the_scratch(gpu):
    for name in ('random_65x65', 'k1', 'random_2x257', 'no_hits', 'random_65x65'):
        run_case(gpu, CASES_BY_NAME[name], scores=name != 'k1')


@pytest.mark.parametrize('blocks', [20, 5])
def test_a_batch_cut_into_several_launches_is_the_restatement(gpu, monkeypatch, blocks):
    """65 fits of 9 blocks each at level 0 with 20 blocks to a launch (two fits a launch: 33 launches, and 4 of the refinement) and
    with 5 (fewer than a fit's: a fit a launch, 13 launches of the refinement); 2 fits of 33 blocks likewise"""
    monkeypatch.setenv('CHROMA_SEED_LAUNCH_BLOCKS', str(blocks))
    run_case(gpu, CASES_BY_NAME['random_65x65'])
    run_case(gpu, CASES_BY_NAME['random_2x257'])


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

    threads = [threading.Thread(target=work, args=(names,)) for names in (('random_2x64', 'tau_edges'), ('random_2x257', 'step_1'))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors


@pytest.mark.parametrize('name,change', refusals(), ids=[r[0] for r in refusals()])
def test_refusals_write_nothing(gpu, name, change):
    case, d = refused_call(change)
    d['out'] = [None if a is None else len(a) - GUARD for a in d['out']]
    rc, out = device_call(gpu, d['seeder'], d['args'], d['out'])
    assert rc == CHROMA_ERR_INVALID, name
    assert all(a is None or np.all(a == SENTINEL) for a in out), name


def test_a_null_seeder_too_many_scores_and_no_fits(gpu):
    from chroma_amd.gpu.tools import to_gpu
    ctx = gpu.get_context()
    case = small_case()
    sizes = output_sizes(case)
    args = list(case_arrays(case))
    args[4] = 0
    rc, out = device_call(gpu, case['seeder'], args, sizes)
    assert rc == 0 and all(np.all(a == SENTINEL) for a in out)
    # nfits * ncand = 2^32 with the scores asked for
    ncand, nfits = 2 ** 20, 2 ** 12
    big = (0, None, ncand, np.zeros(3 * ncand, dtype=np.int32), nfits, np.zeros(nfits + 1, dtype=np.uint32), np.zeros(nfits, dtype=np.int32), None, None, None)
    rc, out = device_call(gpu, case['seeder'], big, [3 * nfits, nfits, nfits, nfits, nfits, 3 * nfits, 8])
    assert rc == CHROMA_ERR_INVALID and all(np.all(a == SENTINEL) for a in out)
    d = [to_gpu(a, ctx=ctx) for a in case_arrays(case) if not isinstance(a, int)]
    assert ctx._lib.chroma_vertex_seed(ctx.handle, None, 2, ctypes.c_void_p(d[0].ptr), 2, ctypes.c_void_p(d[1].ptr), 0, None, None, None, None, None,
                                       None, None, None, None, None, None, None) == CHROMA_ERR_INVALID


def test_gpu_vertex_seeder_is_fit_many_on_the_host(gpu):
    from chroma_amd.gpu.seed import GPUVertexSeeder
    from test_seed_host import python_layer_fixture
    seeder, offsets, channel, t, w = python_layer_fixture()
    host = seeder.fit_many(offsets, channel, t, w, scores=True)
    runner = GPUVertexSeeder(gpu.get_context(), seeder)
    for dev in (runner.fit_many(offsets, channel, t, w, scores=True), seeder.fit_many(offsets, channel, t, w, gpu=runner, scores=True)):
        for name in ('pos', 't0', 'score', 'bin', 'cand', 'level_score', 'outside', 'nhits', 'pos_int', 'scores'):
            assert np.array_equal(getattr(dev, name), getattr(host, name)), name
    assert len(seeder.fit_many([0], [], [], gpu=runner)) == 0


def test_simulation_seeds_every_firing_as_the_host_does(gpu, tiny_geometry, tmp_path):
    from conftest import bomb
    from chroma_amd.gpu import tools
    from chroma_amd.seed import SeedFits, VertexSeeder
    from chroma_amd.sim import Simulation
    previous = tools._current
    window = (-8.0, 0.5, 512)
    trigger = gpu.DaqTrigger(2, 16, 64, 8, 40)
    digitizer = gpu.DaqDigitizer.biexponential(30.0, 1.0, 6.0, 0.5, bits=12, pedestal=150, noise_sigma=2.0)
    reducer = gpu.DaqReducer.for_digitizer(digitizer, 8, lead=2, lag=6, nbaseline=4, min_width=2, time_offset_ns=0.75)
    seeder = VertexSeeder.for_detector(tiny_geometry, 200.0, levels=3, weights='npe')
    try:
        firings = 0
        for reduced in (True, False):
            batch = [bomb(n, seed=300 + k) for k, n in enumerate([400, 1, 3000, 64])]
            batch.insert(2, event.Photons())
            sim = Simulation(tiny_geometry, seed=21, daq_seeder=seeder if reduced else None)
            kw = dict(daq_digitizer=digitizer, daq_reducer=reducer) if reduced else dict(daq_seeder=seeder)
            events = list(sim.simulate(batch, run_daq=True, max_steps=100, daq_window=window, daq_trigger=trigger, **kw))
            with pytest.raises(ValueError):
                list(sim.simulate([bomb(10, seed=1)], run_daq=True, daq_window=window, daq_seeder=seeder))
            del sim
            for ev in events:
                t = ev.triggers
                assert isinstance(t.vertices, SeedFits) and len(t.vertices) == len(t)
                for k in range(len(t)):
                    want = t.seed(k, seeder, source='reco' if reduced else 'gate')
                    for name in ('pos', 't0', 'score', 'bin', 'cand', 'level_score', 'outside', 'nhits'):
                        assert np.array_equal(getattr(t.vertices, name)[k:k + 1], getattr(want, name)), (ev.id, k, name)
                firings += len(t)
        assert firings >= 2
        # chroma-sim --daq-seed: a seed per firing beside the triggers
        from chroma_amd import cli
        path = str(tmp_path / 'seed.npz')
        assert cli.main(['@chroma_amd.demo.tiny', '-n', '2', '--nphotons', '900', '-s', '4', '--max-steps', '100', '--daq-window=-8,0.5,512', '--daq-trigger',
                         '2,16,64,8,40', '--daq-seed', '200,500,2', '-o', path]) == 0
        saved = np.load(path)
        nseeds = 0
        for k in range(2):
            n = len(saved['ev%d/trigger_bin' % k])
            assert saved['ev%d/seed_pos' % k].shape == (n, 3) and saved['ev%d/seed_t0' % k].shape == (n,)
            assert saved['ev%d/seed_score' % k].shape == (n,) and saved['ev%d/seed_outside' % k].shape == (n,)
            nseeds += n
        assert nseeds >= 1
    finally:
        tools._current = previous
