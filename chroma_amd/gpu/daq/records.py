"""The record families of the time-binned DAQ -- per family one table of (name, dtype) in the order of the C calls' arguments, from
which every buffer list, dtype tuple and typed empty is derived -- and the two idioms every stage shares: stitching the chunks of a
batch (``Columns``, ``Ragged``) and calling twice where the first call counts (``count_then_fill``).  Pure NumPy."""
import numpy as np

from chroma_amd import _lib

PULSE_COLUMNS = (('channel', np.int32), ('bin', np.uint32), ('npe', np.uint32), ('q_int', np.uint32), ('t_first', np.float32), ('flags', np.uint32))
FIRING_COLUMNS = (('bin', np.uint32), ('sum', np.uint32))
HIT_COLUMNS = (('hit_channel', np.int32), ('hit_npe', np.uint32), ('hit_q_int', np.uint32), ('hit_t_first', np.float32), ('hit_flags', np.uint32))
# the per-pulse arrays of a trace reduction, in the order of chroma_daq_reduce_traces' arguments, and its per-trace ones
FOUND_COLUMNS = (('found_start', np.uint32), ('found_width', np.uint32), ('found_peak', np.uint32), ('found_peak_sample', np.uint32),
                 ('found_integral', np.int64), ('found_time', np.uint32), ('found_flags', np.uint32))
REDUCED_COLUMNS = (('trace_base', np.int32), ('reduced_flags', np.uint32))

NO_TRIGGER = 0xffffffff          # pulse_trigger of a pulse that lies in no gate


def names(table):
    return tuple(name for name, _ in table)


def kinds(table):
    return [kind for _, kind in table]


def named(table, columns):
    """{name: column} of ``columns`` in the order of ``table``"""
    return dict(zip(names(table), columns))


def columns_of(table, record):
    """The columns of ``table`` out of ``record`` ({name: column}), in its order."""
    return [record[name] for name in names(table)]


def zeros_of(table, n=0):
    """A zeroed host array of ``n`` entries per column of ``table``."""
    return [np.zeros(n, dtype=kind) for kind in kinds(table)]


class Columns(object):
    """The chunks of a table joined: ``append(columns)`` takes a chunk's columns in the order of ``table`` ((name, dtype) each; a
    dtype may carry a shape per entry, as (np.uint16, (G,))), ``finish()`` gives {name: the concatenated column}, typed empties
    where there was no chunk.  ``total`` counts the entries so far."""

    def __init__(self, table):
        self.table = tuple(table)
        self.parts = [[] for _ in self.table]
        self.total = 0

    def append(self, columns):
        for part, a in zip(self.parts, columns):
            part.append(a)
        self.total += len(columns[0])

    def finish(self):
        return named(self.table, [np.concatenate(part) if part else np.zeros(0, dtype=kind) for part, kind in zip(self.parts, kinds(self.table))])


class Ragged(Columns):
    """The chunks of a ragged table joined: rows of entries, ``append(offsets, columns)`` with a chunk's ``offsets`` (rows + 1, from
    0) into its columns; ``finish()`` gives (offsets (every row + 1, int64, from 0), {name: column})."""

    def __init__(self, table):
        Columns.__init__(self, table)
        self.offsets = [np.zeros(1, dtype=np.int64)]

    def append(self, offsets, columns):
        self.offsets.append(np.asarray(offsets)[1:].astype(np.int64) + self.total)
        Columns.append(self, columns)

    def finish(self):
        return np.concatenate(self.offsets), Columns.finish(self)


def rebase_triggers(pulse_trigger, by):
    """``pulse_trigger`` (uint32) with ``by`` added to every firing number (modulo 2^32); ``NO_TRIGGER`` stays."""
    return np.where(pulse_trigger == NO_TRIGGER, pulse_trigger, pulse_trigger + np.uint32(by & 0xffffffff)).astype(np.uint32)


def count_then_fill(call, capacity, spare=False):
    """``call(capacity)`` -> (rc, reported): a library call that fills room for ``capacity`` entries and reports how many there
    are.  If it fails and reports more than the room, it is made again, once, with room for what it reported -- exactly (host
    arrays), or with ``spare`` a quarter more (device buffers, which are kept).  Raises what ``rc`` says; returns (reported,
    the capacity of the last call)."""
    for attempt in range(2):
        rc, reported = call(capacity)
        reported = int(reported)
        if rc == 0 or attempt or reported <= capacity:
            break
        capacity = reported + reported // 4 if spare else reported
    _lib.check(rc)
    return reported, capacity


def index_of(i, n, what):
    """``i`` as an index into ``n`` things (negative: from the end), or IndexError('<what> i of n')."""
    i = int(i)
    if i < 0:
        i += n
    if not 0 <= i < n:
        raise IndexError('%s %d of %d' % (what, i, n))
    return i


def whole(value, lo, hi, no_number, no_fit):
    """``value`` as an int if it is a whole number in lo .. hi, else ValueError(no_number) or ValueError(no_fit)."""
    try:
        n = int(value)
    except (TypeError, ValueError):
        raise ValueError(no_number)
    if n != value or not lo <= n <= hi:
        raise ValueError(no_fit)
    return n
