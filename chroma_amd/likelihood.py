"""Likelihood of a detector event given a photon source (reference: chroma/likelihood.py).

The reference returns ``uncertainties.ufloat`` values; that package is not a dependency here, so the results are
``Measurement`` objects with the same ``nominal_value`` and ``std_dev`` attributes.  The vertex generators of the
reference become iterables of Photons (or Events that carry ``photons_beg``): there is no GEANT4 here.
"""
from itertools import islice
from math import sqrt

import numpy as np


class Measurement(object):
    """A value with a standard deviation: the part of ``uncertainties.ufloat`` the likelihood uses (uncorrelated
    errors add in quadrature)."""

    def __init__(self, nominal_value, std_dev=0.0):
        self.nominal_value = float(nominal_value)
        self.std_dev = float(std_dev)

    def __neg__(self):
        return Measurement(-self.nominal_value, self.std_dev)

    def __add__(self, other):
        if isinstance(other, Measurement):
            return Measurement(self.nominal_value + other.nominal_value, sqrt(self.std_dev ** 2 + other.std_dev ** 2))
        return Measurement(self.nominal_value + float(other), self.std_dev)

    __radd__ = __add__

    def __sub__(self, other):
        return self + (-other if isinstance(other, Measurement) else -float(other))

    def __float__(self):
        return self.nominal_value

    def __lt__(self, other):
        return self.nominal_value < float(other)

    def __gt__(self, other):
        return self.nominal_value > float(other)

    def __repr__(self):
        return '%r+/-%r' % (self.nominal_value, self.std_dev)


def _pdf_floor(trange, qrange, time_only):
    if time_only:
        return 1.0 / (trange[1] - trange[0])
    return 1.0 / (trange[1] - trange[0]) / (qrange[1] - qrange[0])


class Likelihood(object):
    "Class to evaluate likelihoods for detector events."

    def __init__(self, sim, event=None, tbins=100, trange=(-0.5, 999.5), qbins=10, qrange=(-0.5, 49.5), time_only=True):
        """``sim``: the Simulation that builds the PDFs; ``event``: the detector event being reconstructed (or call
        set_event() before eval()); ``tbins``/``trange``, ``qbins``/``qrange``: PDF binning; ``time_only``: use the
        time observable alone."""
        self.sim = sim
        self.tbins = tbins
        self.trange = trange
        self.qbins = qbins
        self.qrange = qrange
        self.time_only = time_only
        if event is not None:
            self.set_event(event)

    def set_event(self, event):
        "Set the detector event being reconstructed."
        self.event = event

    def eval_channel_vbin(self, vertex_generator, nevals, nreps=16, ndaq=50):
        """Hit probability and time PDF density per channel by the variable-bin method.
        Returns (hit probabilities, PDF values, PDF uncertainties)."""
        ntotal = nevals * nreps * ndaq
        hitcount, pdf_prob, pdf_prob_uncert = self.sim.eval_pdf(self.event.channels, islice(vertex_generator, nevals),
                                                                0.2, self.trange, 1, self.qrange, nreps=nreps, ndaq=ndaq,
                                                                time_only=self.time_only, min_bin_content=320)
        hit_prob = hitcount.astype(np.float32) / ntotal
        # zero or NaN densities take the flat PDF's value
        bad_value = (pdf_prob <= 0.0) | np.isnan(pdf_prob)
        pdf_floor = _pdf_floor(self.trange, self.qrange, self.time_only)
        pdf_prob[bad_value] = pdf_floor
        pdf_prob_uncert[bad_value] = pdf_floor
        return hit_prob, pdf_prob, pdf_prob_uncert

    def eval(self, vertex_generator, nevals, nreps=16, ndaq=50):
        """Negative log likelihood that the event came from ``vertex_generator``: log of the probability of each
        channel being hit or not, plus log of the PDF density at each hit channel's time."""
        ntotal = nevals * nreps * ndaq
        hit_prob, pdf_prob, pdf_prob_uncert = self.eval_channel_vbin(vertex_generator, nevals, nreps, ndaq)
        hit = np.asarray(self.event.channels.hit).astype(bool)
        hit_prob = np.array(hit_prob, dtype=np.float32)
        hit_prob[~hit] = 1.0 - hit_prob[~hit]                   # channels the event did not hit: probability of that
        hit_prob = np.maximum(hit_prob, 0.5 / ntotal)           # floor: keep the log finite
        log_likelihood = Measurement(np.log(hit_prob).sum(), 0.0)
        log_likelihood += Measurement(np.log(pdf_prob[hit]).sum(), 0.0)
        return -log_likelihood

    def setup_kernel(self, vertex_generator, nevals, nreps, ndaq, oversample_factor):
        self.sim.setup_kernel(self.event.channels, islice(vertex_generator, nevals * oversample_factor), self.trange,
                              self.qrange, nreps=nreps, ndaq=ndaq, time_only=self.time_only, scale_factor=oversample_factor)

    def eval_kernel(self, vertex_generator, nevals, nreps=16, ndaq=50, navg=10):
        """Negative log likelihood from the kernel estimate, averaged over ``navg`` evaluations: (mean, error of the
        mean).  As in the reference, only the PDF densities of the hit channels enter (the hit / not-hit term is
        skipped)."""
        ntotal = nevals * nreps * ndaq
        hit = np.asarray(self.event.channels.hit).astype(bool)
        mom0, mom1, mom2 = 0, 0.0, 0.0
        for _ in range(navg):
            hitcount, pdf_prob, pdf_prob_uncert = self.sim.eval_kernel(self.event.channels, islice(vertex_generator, nevals),
                                                                       self.trange, self.qrange, nreps=nreps, ndaq=ndaq,
                                                                       time_only=self.time_only)
            bad_value = (pdf_prob <= 0.0) | np.isnan(pdf_prob)
            pdf_floor = _pdf_floor(self.trange, self.qrange, self.time_only)
            pdf_prob[bad_value] = pdf_floor
            pdf_prob_uncert[bad_value] = pdf_floor
            log_likelihood = np.log(pdf_prob[hit]).sum()
            if np.isfinite(log_likelihood):
                mom0 += 1
                mom1 += log_likelihood
                mom2 += log_likelihood ** 2
        avg_like = mom1 / mom0
        rms_like = max(mom2 / mom0 - avg_like ** 2, 0.0) ** 0.5
        return Measurement(-avg_like, rms_like / sqrt(mom0))
