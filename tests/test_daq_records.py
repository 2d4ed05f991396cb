"""The idioms every stage of the DAQ's Python driver shares (chroma_amd.gpu.daq.records, .results.dense_channels): stitching the
chunks of a ragged table, rebasing pulse_trigger, the call that counts and is made again, and the dense Channels of sparse
columns.  Pure NumPy: no GPU, no library.
"""
import numpy as np
import pytest

from chroma_amd._lib import ChromaError
from chroma_amd.gpu.daq.records import Columns, Ragged, rebase_triggers, count_then_fill, NO_TRIGGER, PULSE_COLUMNS
from chroma_amd.gpu.daq.results import dense_channels

TABLE = (('a', np.int32), ('b', np.uint32), ('c', np.float32), ('d', np.int64))


def ragged_table(nrows=300, seed=5):
    """(offsets int64 (nrows + 1), columns in TABLE's order): rows of 0 .. 4 entries, empty ones at the start, in the middle and at
    the end; every bit pattern of a word may occur, NaNs among the floats included."""
    rng = np.random.default_rng(seed)
    counts = rng.integers(0, 5, nrows)
    counts[[0, 1, nrows // 2, nrows // 2 + 1, nrows - 2, nrows - 1]] = 0
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    n = int(offsets[-1])
    words = rng.integers(0, 2 ** 32, (3, n), dtype=np.uint64).astype(np.uint32)
    return offsets, [words[0].view(np.int32), words[1], words[2].view(np.float32), rng.integers(-2 ** 62, 2 ** 62, n, dtype=np.int64)]


def assert_bits(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize('rows_per_chunk', [1, 7, 300])
def test_chunks_of_a_ragged_table_stitch_back_to_it_bit_for_bit(rows_per_chunk):
    offsets, columns = ragged_table()
    assert offsets[-1] > 400 and len(offsets) == 301
    ragged = Ragged(TABLE)
    for first in range(0, 300, rows_per_chunk):
        last = min(300, first + rows_per_chunk)
        w = slice(int(offsets[first]), int(offsets[last]))
        # a chunk as a call returns it: offsets from 0, uint32
        ragged.append((offsets[first:last + 1] - offsets[first]).astype(np.uint32), [a[w] for a in columns])
        assert ragged.total == offsets[last]
    got_offsets, got = ragged.finish()
    assert_bits(got_offsets, offsets, 'offsets')
    assert list(got) == [name for name, _ in TABLE]
    for (name, _), want in zip(TABLE, columns):
        assert_bits(got[name], want, name)


def test_no_chunk_and_empty_chunks_give_typed_empties():
    offsets, got = Ragged(TABLE).finish()
    assert_bits(offsets, np.zeros(1, dtype=np.int64), 'offsets of no chunk')
    for name, kind in TABLE:
        assert_bits(got[name], np.zeros(0, dtype=kind), name)
    ragged = Ragged(TABLE)
    for nrows in (3, 0, 2):
        ragged.append(np.zeros(nrows + 1, dtype=np.uint32), [np.zeros(0, dtype=kind) for _, kind in TABLE])
    offsets, got = ragged.finish()
    assert_bits(offsets, np.zeros(6, dtype=np.int64), 'offsets of empty chunks')
    for name, kind in TABLE:
        assert_bits(got[name], np.zeros(0, dtype=kind), name)
    # the columns without offsets, one with a shape per entry (the traces: hits x samples)
    table = (('adc', (np.uint16, (8,))), ('trace_flags', np.uint32))
    got = Columns(table).finish()
    assert_bits(got['adc'], np.zeros((0, 8), dtype=np.uint16), 'adc of no chunk')
    assert_bits(got['trace_flags'], np.zeros(0, dtype=np.uint32), 'trace_flags of no chunk')
    both = Columns(table)
    both.append([np.arange(16, dtype=np.uint16).reshape(2, 8), np.array([1, 2], dtype=np.uint32)])
    both.append([np.arange(16, 24, dtype=np.uint16).reshape(1, 8), np.array([3], dtype=np.uint32)])
    got = both.finish()
    assert both.total == 3
    assert_bits(got['adc'], np.arange(24, dtype=np.uint16).reshape(3, 8), 'adc')
    assert_bits(got['trace_flags'], np.array([1, 2, 3], dtype=np.uint32), 'trace_flags')
    assert [name for name, _ in PULSE_COLUMNS] == ['channel', 'bin', 'npe', 'q_int', 't_first', 'flags']


def test_pulse_trigger_is_rebased_by_the_firings_before_and_no_trigger_survives():
    of = np.array([0, NO_TRIGGER, 2, 2, NO_TRIGGER, 0xfffffffe], dtype=np.uint32)
    assert_bits(rebase_triggers(of, 0), of, 'by nothing')
    assert_bits(rebase_triggers(of[:5], 1500), np.array([1500, NO_TRIGGER, 1502, 1502, NO_TRIGGER], dtype=np.uint32), 'by 1500')
    # and back, as an event's own numbering takes the firings before it off
    assert_bits(rebase_triggers(rebase_triggers(of[:5], 1500), -1500), of[:5], 'there and back')
    assert_bits(rebase_triggers(np.zeros(0, dtype=np.uint32), 7), np.zeros(0, dtype=np.uint32), 'of no pulse')


class FakeCall(object):
    """A library call that counts: fails with rc 7 while it has room for less than ``there_are`` (as told per call)."""

    def __init__(self, *there_are):
        self.there_are = list(there_are)
        self.capacities = []

    def __call__(self, capacity):
        self.capacities.append(capacity)
        n = self.there_are[len(self.capacities) - 1]
        return (0 if n <= capacity else 7), n


def test_a_call_that_fits_is_made_once():
    call = FakeCall(1024)
    assert count_then_fill(call, 1024, spare=True) == (1024, 1024) and call.capacities == [1024]
    call = FakeCall(0)
    assert count_then_fill(call, 0) == (0, 0) and call.capacities == [0]


def test_a_call_that_reports_more_is_made_again_with_room_for_it():
    call = FakeCall(1030, 1030)
    assert count_then_fill(call, 0) == (1030, 1030) and call.capacities == [0, 1030]                    # host arrays: exactly
    call = FakeCall(1030, 1030)
    assert count_then_fill(call, 1024, spare=True) == (1030, 1287) and call.capacities == [1024, 1287]          # device buffers: n + n // 4


def test_a_call_that_fails_for_another_reason_is_not_made_again():
    calls = []

    def call(capacity):
        calls.append(capacity)
        return 3, 5
    with pytest.raises(ChromaError):
        count_then_fill(call, 8)
    assert calls == [8]


def test_a_second_call_that_still_reports_more_is_the_last():
    call = FakeCall(10, 20, 20)
    with pytest.raises(ChromaError):
        count_then_fill(call, 4)
    assert call.capacities == [4, 10]


def test_dense_channels_of_sparse_columns():
    none = dense_channels(5, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.float32), np.zeros(0, dtype=np.uint32))
    assert_bits(none.t, np.full(5, 1e9, dtype=np.float32), 't of nothing')
    assert not none.hit.any() and not none.q.any() and not none.flags.any()
    assert none.q.dtype == np.float32 and none.flags.dtype == np.uint32 and none.hit.dtype == bool
    # a word whose accepted times were all negative comes with t = 1e9: touched, not hit
    some = dense_channels(5, np.array([1, 3, 4], dtype=np.int32), np.array([2.5, 1e9, -0.5], dtype=np.float32),
                          np.array([1.0, 0.5, 0.25], dtype=np.float32), np.array([4, 8, 12], dtype=np.uint32))
    assert some.hit.tolist() == [False, True, False, False, True]
    assert_bits(some.t, np.array([1e9, 2.5, 1e9, 1e9, -0.5], dtype=np.float32), 't')
    assert_bits(some.q, np.array([0, 1.0, 0, 0.5, 0.25], dtype=np.float32), 'q')
    assert_bits(some.flags, np.array([0, 4, 0, 8, 12], dtype=np.uint32), 'flags')
