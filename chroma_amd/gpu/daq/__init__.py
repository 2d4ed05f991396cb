"""GPUDaq / GPUChannels: per-channel earliest hit time, charge and history
(reference: chroma/gpu/daq.py:8-100 over chroma/cuda/daq.cu).

``ndaq == 1`` runs ``run_daq``; ``ndaq > 1`` runs ``run_daq_many`` (daq.cu:88-150): that many
independent acquisitions of the same photons side by side, each with a unit normal jitter on the hit
time (``GPUChannels.iterate_copies`` walks them).  The random numbers a detected photon consumes
(weight gate, jitter, time smear, charge) come from Philox stream ``1 + acquisition`` of that photon
(copy i from word 8 i on), so propagation draws are not disturbed and two acquisitions of the same
photons differ.

``GPUEventDaq`` runs the per-event acquisitions of a whole batch -- what ``Simulation.simulate(run_daq=True)`` asks for -- as one
acquisition over a row of channels per event and reads the touched words back sparse (``EventChannels``).  Its
``acquire_pulses`` is the time-binned view of the same photoelectrons (chroma_daq_count_pulses / chroma_daq_acquire_pulses): per
(event, channel, time bin of a ``DaqWindow``) the number of photoelectrons, their charge, the earliest of their times and the OR
of their histories, only the bins that hold something (``EventPulses``, per event ``Pulses``).  With a ``DaqTrigger`` the pulses are
triggered where they lie on the device (chroma_daq_trigger_pulses): the firings of a multiplicity or photoelectron sum over a
coincidence window, and per firing the channels of its readout gate (``EventTriggers``, per event ``Triggers``);
``EventPulses.trigger`` is the same computed in NumPy on the host arrays.  With a ``DaqNoise`` the PMTs' dark counts are drawn on
the device as further photoelectrons of the pulses (chroma_daq_acquire_pulses_noise), flagged ``event.DARK_NOISE``, and reach
the trigger like any other; ``DaqNoise.sample`` draws the same ones on the host.  With a ``DaqDigitizer`` the gated hits are read out
as ADC traces (chroma_daq_digitize_gates) and with a ``DaqReducer`` the pulses in those are found (chroma_daq_reduce_traces);
``EventTriggers.digitize`` and ``.reduce`` are the same on the host.

The modules, each importing only those before it: ``records`` (the column tables, the chunk stitching, the count-then-fill call),
``settings`` (the five settings classes and the ``DaqChain`` of them), ``results`` (the containers and the host twins that build them), ``device`` (the drivers).
"""
from chroma_amd.gpu.daq.records import (PULSE_COLUMNS, FIRING_COLUMNS, HIT_COLUMNS, FOUND_COLUMNS, REDUCED_COLUMNS, NO_TRIGGER, Columns,
                                        Ragged, rebase_triggers, count_then_fill)
from chroma_amd.gpu.daq.settings import (DaqWindow, DaqNoise, DaqTrigger, DaqDigitizer, DaqReducer, DaqChain, DAQ_NEEDS, daq_needs, CLIPPED_HIGH,
                                         CLIPPED_LOW, TIME_AT_EDGE, OPEN_AT_START, OPEN_AT_END, BASELINE_BUSY, _padded_cdf)
from chroma_amd.gpu.daq.results import (EventChannels, Pulses, EventPulses, FoundPulses, Triggers, EventTriggers, dense_channels,
                                        trigger_pulses_host, reduce_traces_host, _set_found, _time_image, _time_bits, _follow)
from chroma_amd.gpu.daq.device import GPUChannels, GPUDaq, GPUEventDaq, _make_tables
