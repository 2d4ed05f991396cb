"""GPUPDF / GPUKernelPDF: per-channel PDFs of hit time and charge built from DAQ output, and their evaluation at one
detector event (reference: chroma/gpu/pdf.py over chroma/cuda/pdf.cu; kernels: chroma_amd/csrc/kernels_pdf.h).

Every accumulate call takes a GPUChannels and uses ALL its copies (``ndaq`` of them at ``stride``) in one launch.  The
host-side arithmetic that turns the device counters into PDF values and kernel bandwidths is in the module-level
functions ``pdf_eval_values`` and ``kernel_bandwidths`` (pure NumPy).
"""
import numpy as np

from chroma_amd import _lib
from chroma_amd.gpu.tools import GPUArray, get_context, to_gpu, zeros

MAX_MIN_BIN_CONTENT = 1024


def _channel_layout(gpuchannels, nchannels):
    """(ndaq, stride) of a GPUChannels covering ``nchannels`` channels, checked against the size of its arrays."""
    ndaq = int(getattr(gpuchannels, 'ndaq', 1))
    stride = int(getattr(gpuchannels, 'stride', len(gpuchannels.t)))
    n = len(gpuchannels.t)
    if ndaq < 1 or stride < nchannels or len(gpuchannels.q) != n or (ndaq - 1) * stride + nchannels > n:
        raise ValueError('channel arrays of %d entries do not hold %d copies of %d channels at stride %d'
                         % (n, ndaq, nchannels, stride))
    if gpuchannels.t.dtype != np.float32 or gpuchannels.q.dtype != np.float32:
        raise TypeError('channel times and charges must be float32 device arrays')
    return ndaq, stride


def pdf_eval_values(event_hit, hitcount, bincount, nearest, min_twidth, min_bin_content):
    """PDF value and its uncertainty per channel from the counters of accumulate_pdf_eval (chroma/gpu/pdf.py:330-372).

    ``nearest``: (nchannels, min_bin_content) table of the smallest distances, 1e9 where there is none.  High-stats
    channels (bincount >= min_bin_content) take bincount / hitcount / min_twidth; low-stats channels the event hit,
    with some MC, take n / hitcount / (2 d) where d is the n-th nearest distance (n the number of distances found, or
    the first entry when none was).  Others are zero.  Returns (pdf_value, pdf_value * fractional uncertainty)."""
    evhit = np.asarray(event_hit).astype(bool)
    hitcount = np.asarray(hitcount)
    bincount = np.asarray(bincount)
    nearest = np.asarray(nearest, dtype=np.float32).reshape(len(hitcount), min_bin_content)
    pdf_value = np.zeros(len(hitcount), dtype=float)
    pdf_frac_uncert = np.zeros_like(pdf_value)

    high_stats = bincount >= min_bin_content
    if high_stats.any():
        pdf_value[high_stats] = bincount[high_stats].astype(float) / hitcount[high_stats] / min_twidth
        pdf_frac_uncert[high_stats] = 1.0 / np.sqrt(bincount[high_stats])

    low_stats = ~high_stats & (hitcount > 0) & evhit
    last_valid_entry = np.maximum(0, (nearest < 1e9).astype(int).sum(axis=1) - 1)
    distance = nearest[np.arange(len(last_valid_entry)), last_valid_entry]
    if low_stats.any():
        pdf_value[low_stats] = (last_valid_entry[low_stats] + 1).astype(float) / hitcount[low_stats] / distance[low_stats] / 2.0
        pdf_frac_uncert[low_stats] = 1.0 / np.sqrt(last_valid_entry[low_stats] + 1)
    return pdf_value, pdf_value * pdf_frac_uncert


def kernel_bandwidths(hitcount, tmom1, tmom2, event_time, time_only=True, qmom1=None, qmom2=None, event_charge=None,
                      scale_factor=1.0):
    """Inverse kernel bandwidths per channel from the moments of accumulate_moments (chroma/gpu/pdf.py:61-112), as
    float32 arrays (time, charge); zero where the bandwidth is not positive, and the charge one is all zeros when
    ``time_only``.  The formula is the reference's: Silverman's rule, d = 1 or 2 dimensions, with the density
    factor min(1 / rms, exp(-0.5 (x - mean) / rms) / (sqrt(2 pi) rms)) (its exponent is not squared there either)."""
    rho = 1.0
    mom0 = np.maximum(np.asarray(hitcount), 1)
    tmom1 = np.asarray(tmom1)
    tmom2 = np.asarray(tmom2)
    d = 1 if time_only else 2
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        tmean = tmom1 / mom0
        tvar = np.maximum(tmom2 / mom0 - tmean ** 2, 0.0)      # round-off can make it negative
        trms = tvar ** 0.5
        dimensionality_factor = ((4.0 / (d + 2)) / (mom0 / scale_factor)) ** (-1.0 / (d + 4))
        gaussian_density = np.minimum(1.0 / trms, (1.0 / np.sqrt(2.0 * np.pi)) * np.exp(-0.5 * ((event_time - tmean) / trms)) / trms)
        time_bandwidths = dimensionality_factor / gaussian_density * rho
        inv_time = np.zeros_like(time_bandwidths)
        positive = time_bandwidths > 0
        inv_time[positive] = time_bandwidths[positive] ** -1
        if time_only:
            inv_charge = np.zeros_like(inv_time)
        else:
            qmean = np.asarray(qmom1) / mom0
            qrms = (np.asarray(qmom2) / mom0 - qmean ** 2) ** 0.5
            gaussian_density = np.minimum(1.0 / qrms, (1.0 / np.sqrt(2.0 * np.pi)) * np.exp(-0.5 * ((event_charge - qmean) / qrms)) / qrms)
            inv_charge = (dimensionality_factor / gaussian_density * rho) ** -1
    return inv_time.astype(np.float32), np.asarray(inv_charge).astype(np.float32)


class GPUKernelPDF(object):
    """Kernel density estimate of each hit channel's time (and charge) PDF at the event's value."""

    def __init__(self, ctx=None):
        self.ctx = ctx if ctx is not None else get_context()

    def setup_moments(self, nchannels, trange, qrange, time_only=True):
        """Device counters for the moments that set the bandwidths; ``trange`` / ``qrange``: (min, max) of the PDF."""
        self.hitcount_gpu = zeros(nchannels, np.uint32, self.ctx)
        self.tmom1_gpu = zeros(nchannels, np.float32, self.ctx)
        self.tmom2_gpu = zeros(nchannels, np.float32, self.ctx)
        self.qmom1_gpu = zeros(nchannels, np.float32, self.ctx)
        self.qmom2_gpu = zeros(nchannels, np.float32, self.ctx)
        self.trange = trange
        self.qrange = qrange
        self.time_only = time_only

    def clear_moments(self):
        "Reset the moments to start accumulating new Monte Carlo."
        for a in (self.hitcount_gpu, self.tmom1_gpu, self.tmom2_gpu, self.qmom1_gpu, self.qmom2_gpu):
            a.fill(0)

    def accumulate_moments(self, gpuchannels, nthreads_per_block=64):
        """Add every copy of a DAQ result to the moments."""
        nchannels = self.hitcount_gpu.size
        ndaq, stride = _channel_layout(gpuchannels, nchannels)
        _lib.check(self.ctx._lib.chroma_pdf_moments(
            self.ctx.handle, int(bool(self.time_only)), nchannels, ndaq, stride, gpuchannels.t.ptr, gpuchannels.q.ptr,
            float(self.trange[0]), float(self.trange[1]), float(self.qrange[0]), float(self.qrange[1]),
            self.hitcount_gpu.ptr, self.tmom1_gpu.ptr, self.tmom2_gpu.ptr, self.qmom1_gpu.ptr, self.qmom2_gpu.ptr))

    def compute_bandwidth(self, event_hit, event_time, event_charge, scale_factor=1.0):
        """Bandwidths for the kernel estimate from the accumulated moments (see ``kernel_bandwidths``)."""
        inv_time, inv_charge = kernel_bandwidths(
            self.hitcount_gpu.get(), self.tmom1_gpu.get(), self.tmom2_gpu.get(), np.asarray(event_time), self.time_only,
            None if self.time_only else self.qmom1_gpu.get(), None if self.time_only else self.qmom2_gpu.get(),
            None if self.time_only else np.asarray(event_charge), scale_factor=scale_factor)
        self.inv_time_bandwidths_gpu = to_gpu(inv_time, self.ctx)
        self.inv_charge_bandwidths_gpu = to_gpu(inv_charge, self.ctx)

    def setup_kernel(self, event_hit, event_time, event_charge):
        """The event to evaluate at: hit flag, time and charge per channel (time and charge ignored where not hit)."""
        self.event_hit_gpu = to_gpu(np.asarray(event_hit).astype(np.uint32), self.ctx)
        self.event_time_gpu = to_gpu(np.asarray(event_time).astype(np.float32), self.ctx)
        self.event_charge_gpu = to_gpu(np.asarray(event_charge).astype(np.float32), self.ctx)
        self.hitcount_gpu.fill(0)
        self.time_pdf_values_gpu = zeros(len(event_hit), np.float32, self.ctx)
        self.charge_pdf_values_gpu = zeros(len(event_hit), np.float32, self.ctx)

    def clear_kernel(self):
        self.hitcount_gpu.fill(0)
        self.time_pdf_values_gpu.fill(0)
        self.charge_pdf_values_gpu.fill(0)

    def accumulate_kernel(self, gpuchannels, nthreads_per_block=64):
        "Add every copy of a DAQ result to the kernel estimate."
        nchannels = self.event_hit_gpu.size
        ndaq, stride = _channel_layout(gpuchannels, nchannels)
        _lib.check(self.ctx._lib.chroma_pdf_kernel_eval(
            self.ctx.handle, int(bool(self.time_only)), nchannels, ndaq, stride, self.event_hit_gpu.ptr,
            self.event_time_gpu.ptr, self.event_charge_gpu.ptr, gpuchannels.t.ptr, gpuchannels.q.ptr,
            float(self.trange[0]), float(self.trange[1]), float(self.qrange[0]), float(self.qrange[1]),
            self.inv_time_bandwidths_gpu.ptr, self.inv_charge_bandwidths_gpu.ptr, self.hitcount_gpu.ptr,
            self.time_pdf_values_gpu.ptr, self.charge_pdf_values_gpu.ptr))

    def get_kernel_eval(self):
        """(hitcount, PDF value per channel, zeros): the kernel sums divided by the MC hits that entered them."""
        hitcount = self.hitcount_gpu.get()
        time_pdf_values = self.time_pdf_values_gpu.get()
        time_pdf_values /= np.maximum(1, hitcount)          # (float32 in place, as the reference)
        charge_pdf_values = self.charge_pdf_values_gpu.get()
        charge_pdf_values /= np.maximum(1, hitcount)
        pdf_values = time_pdf_values if self.time_only else time_pdf_values * charge_pdf_values
        return hitcount, pdf_values, np.zeros_like(pdf_values)


class GPUPDF(object):
    """Binned (channel, time, charge) PDFs, and the variable-bin evaluation of each channel's time PDF at one event."""

    def __init__(self, ctx=None):
        self.ctx = ctx if ctx is not None else get_context()

    def setup_pdf(self, nchannels, tbins, trange, qbins, qrange):
        """Histograms of ``tbins`` x ``qbins`` bins over ``trange`` x ``qrange`` for each of ``nchannels`` channels."""
        self.events_in_histogram = 0
        self.hitcount_gpu = zeros(nchannels, np.uint32, self.ctx)
        self.pdf_gpu = zeros(nchannels * tbins * qbins, np.uint32, self.ctx)
        self.nchannels = nchannels
        self.tbins = tbins
        self.trange = trange
        self.qbins = qbins
        self.qrange = qrange

    def clear_pdf(self):
        """Rezero the PDF counters."""
        self.events_in_histogram = 0
        self.hitcount_gpu.fill(0)
        self.pdf_gpu.fill(0)

    def add_hits_to_pdf(self, gpuchannels, nthreads_per_block=64):
        """Bin every copy of a DAQ result."""
        ndaq, stride = _channel_layout(gpuchannels, self.nchannels)
        _lib.check(self.ctx._lib.chroma_pdf_bin_hits(
            self.ctx.handle, self.nchannels, ndaq, stride, gpuchannels.q.ptr, gpuchannels.t.ptr, int(self.tbins),
            float(self.trange[0]), float(self.trange[1]), int(self.qbins), float(self.qrange[0]), float(self.qrange[1]),
            self.hitcount_gpu.ptr, self.pdf_gpu.ptr))
        self.events_in_histogram += ndaq

    def get_pdfs(self):
        """The 1-D hitcount array and the 3-D [channel, time, charge] histogram."""
        return self.hitcount_gpu.get(), self.pdf_gpu.get().reshape(self.nchannels, self.tbins, self.qbins)

    def setup_pdf_eval(self, event_hit, event_time, event_charge, min_twidth, trange, min_qwidth, qrange,
                       min_bin_content=10, time_only=True):
        """Evaluate each channel's PDF at the event's value as the Monte Carlo runs: a bin at least ``min_twidth`` wide
        around the event's time, widened until it holds ``min_bin_content`` MC hits (chroma/gpu/pdf.py:218-276).
        Only the time observable is supported, as in the reference."""
        if not time_only:
            raise NotImplementedError('pdf_eval supports the time observable only (time_only=True)')
        min_bin_content = int(min_bin_content)
        if not 1 <= min_bin_content <= MAX_MIN_BIN_CONTENT:
            raise ValueError('min_bin_content must be in 1 .. %d' % MAX_MIN_BIN_CONTENT)
        event_hit = np.asarray(event_hit).astype(bool)
        self.map_hit_offset_to_channel_id = np.flatnonzero(event_hit).astype(np.uint32)
        self.event_nhit = len(self.map_hit_offset_to_channel_id)
        self.map_hit_offset_to_channel_id_gpu = to_gpu(self.map_hit_offset_to_channel_id, self.ctx)
        self.event_hit_gpu = to_gpu(event_hit.astype(np.uint32), self.ctx)
        self.event_time_gpu = to_gpu(np.asarray(event_time).astype(np.float32), self.ctx)
        self.event_charge_gpu = to_gpu(np.asarray(event_charge).astype(np.float32), self.ctx)
        self.eval_hitcount_gpu = zeros(len(event_hit), np.uint32, self.ctx)
        self.eval_bincount_gpu = zeros(len(event_hit), np.uint32, self.ctx)
        self.nearest_mc_gpu = GPUArray(self.event_nhit * min_bin_content, np.float32, self.ctx).fill(1e9)
        self.min_twidth = min_twidth
        self.trange = trange
        self.min_qwidth = min_qwidth
        self.qrange = qrange
        self.min_bin_content = min_bin_content
        self.time_only = time_only

    def clear_pdf_eval(self):
        "Reset PDF evaluation counters to start accumulating new Monte Carlo."
        self.eval_hitcount_gpu.fill(0)
        self.eval_bincount_gpu.fill(0)
        self.nearest_mc_gpu.fill(1e9)

    def accumulate_pdf_eval(self, gpuchannels, nthreads_per_block=64, max_blocks=10000):
        "Add every copy of a DAQ result to the PDF evaluation."
        nchannels = self.event_hit_gpu.size
        ndaq, stride = _channel_layout(gpuchannels, nchannels)
        _lib.check(self.ctx._lib.chroma_pdf_eval_accumulate(
            self.ctx.handle, nchannels, ndaq, stride, self.event_hit_gpu.ptr, self.event_time_gpu.ptr, gpuchannels.t.ptr,
            self.event_nhit, self.map_hit_offset_to_channel_id_gpu.ptr, float(self.min_twidth), float(self.trange[0]),
            float(self.trange[1]), self.min_bin_content, self.eval_hitcount_gpu.ptr, self.eval_bincount_gpu.ptr,
            self.nearest_mc_gpu.ptr))

    def get_nearest_mc(self):
        """(nchannels, min_bin_content) table of the nearest MC distances, 1e9 where there is none."""
        nearest = np.full((self.event_hit_gpu.size, self.min_bin_content), 1e9, dtype=np.float32)
        if self.event_nhit:
            nearest[self.map_hit_offset_to_channel_id] = self.nearest_mc_gpu.get().reshape(self.event_nhit, self.min_bin_content)
        return nearest

    def get_pdf_eval(self):
        """(hitcount, PDF value, PDF uncertainty) per channel (see ``pdf_eval_values``)."""
        evhit = self.event_hit_gpu.get().astype(bool)
        hitcount = self.eval_hitcount_gpu.get()
        bincount = self.eval_bincount_gpu.get()
        pdf_value, pdf_uncert = pdf_eval_values(evhit, hitcount, bincount, self.get_nearest_mc(), self.min_twidth,
                                                self.min_bin_content)
        return hitcount, pdf_value, pdf_uncert
