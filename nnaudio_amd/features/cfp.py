"""Combined frequency and periodicity features (drop-in for ``nnAudio.features.Combined_Frequency_Periodicity`` and
``nnAudio.features.CFP``, reference: Installation/nnAudio/features/cfp.py).

L. Su and Y.-H. Yang, "Combining Spectral and Temporal Representations for Multipitch Estimation of Polyphonic Music",
IEEE/ACM TASLP 23(10), 2015: a magnitude spectrum, its generalised cepstrum and the generalised cepstrum of that, each
through a power-law rectifier, mapped to a common log-frequency axis by two triangular filterbanks and multiplied.

On a CUDA tensor with ``N = int(fs / fr)`` an even product of 2s and 5s up to 16000 (8 / 16 / 32 kHz material at integer
``fr``) and no log layer (``g[i] == 0``), the whole chain of a pair of frames runs inside one workgroup
(``csrc/cfp.hip``: the length-N FFTs in LDS, nothing but the waveform read and the filterbank outputs written;
``engine.cfp_served`` asks the library).  Everything else -- CPU tensors, 44.1 kHz's N = 22050, a log layer -- runs the
same steps as torch operators (``engine.cfp_composition``); ``engine.set_cfp_kernel(False)`` / ``MISPEC_CFP_KERNEL=0``
forces that route.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import engine


def _log_frequency_filterbanks(f, q, fr, fc, tc, NumPerOct, fs):
    """The two triangular filterbanks, float64: rows are log-spaced centre frequencies ``fc 2^(i / NumPerOct)`` below
    ``1 / tc``; row i rises from centre i - 1 to centre i and falls to centre i + 1, evaluated on the frequency axis
    ``f`` (first matrix) and on ``1 / q`` (second matrix).  Row 0 and the last centre have no filter of their own."""
    stop = 1 / tc
    n_est = int(np.ceil(np.log2(stop / fc)) * NumPerOct)
    centres = []
    for i in range(n_est):
        c = fc * pow(2, float(i) / NumPerOct)
        if not c < stop:
            break
        centres.append(c)
    n = len(centres)

    def triangle(axis, lo, mid, hi):
        up = (axis - lo) / (mid - lo)
        down = (hi - axis) / (hi - mid)
        return np.where((axis > lo) & (axis < mid), up, np.where((axis > mid) & (axis < hi), down, 0.0))

    fmat = np.zeros((n - 1, len(f)), dtype=np.float64)
    qmat = np.zeros((n - 1, len(q)), dtype=np.float64)
    with np.errstate(divide="ignore"):
        fq = 1 / q  # (inf at quefrency 0: outside every triangle)
    for i in range(1, n - 1):
        lo, mid, hi = centres[i - 1], centres[i], centres[i + 1]
        a = int(round(lo / fr))
        b = int(round(hi / fr) + 1)
        if a >= b - 1:
            fmat[i, a] = 1
        else:
            if b > len(f):
                raise IndexError("CFP: filter %d reaches bin %d of a %d-bin frequency axis" % (i, b - 1, len(f)))
            fmat[i, a:b] = triangle(f[a:b], lo, mid, hi)
        a = int(round(fs / hi))
        b = int(round(fs / lo) + 1)
        if b > len(q):
            raise IndexError("CFP: filter %d reaches quefrency bin %d of %d" % (i, b - 1, len(q)))
        qmat[i, a:b] = triangle(fq[a:b], lo, mid, hi)
    return fmat, qmat


class _CFPBase(nn.Module):
    """What the two classes share: constructor, buffers and the forward; they differ in the frames they keep and in
    what they return."""

    _drop_edge_frames = False

    def __init__(self, fr=2, fs=16000, hop_length=320, window_size=2049, fc=80, tc=1 / 1000, g=[0.24, 0.6, 1],
                 NumPerOct=48):
        super().__init__()
        self.window_size = window_size
        self.hop_length = hop_length
        self.N = int(fs / float(fr))
        if np.size(g) < 2:
            raise ValueError("CFP: g needs at least two exponents (the spectrum's and the cepstrum's), got %r" % (g,))
        if window_size > self.N:
            raise ValueError("CFP: window_size (%d) must be <= N = int(fs / fr) (%d)" % (window_size, self.N))
        f = fs * np.linspace(0, 0.5, np.round(self.N // 2), endpoint=True)
        self.pad_value = self.N - window_size
        from scipy.signal.windows import blackmanharris

        self.register_buffer("h", torch.tensor(blackmanharris(window_size)).float())
        self.NumofLayer = np.size(g)
        self.g = g
        self.tc_idx = round(fs * tc)
        self.fc_idx = round(fc / fr)
        self.HighFreqIdx = int(round((1 / tc) / fr) + 1)
        self.HighQuefIdx = int(round(fs / fc) + 1)
        self.f = f[: self.HighFreqIdx]
        self.q = np.arange(self.HighQuefIdx) / float(fs)
        if self.HighQuefIdx > int(round(self.N / 2)):
            raise ValueError("CFP: the quefrency axis (%d bins, fs / fc) does not fit half a frame (N = %d)"
                             % (self.HighQuefIdx, self.N))
        fmat, qmat = _log_frequency_filterbanks(self.f, self.q, fr, fc, tc, NumPerOct, fs)
        self.register_buffer("freq2logfreq_matrix", torch.tensor(fmat).float())
        self.register_buffer("quef2logfreq_matrix", torch.tensor(qmat).float())
        # per (buffers' identity and version): the kernel's operands (supports, twiddles, window norm) -- not buffers
        self._derived = {}

    def _operands(self):
        bufs = (self.h, self.freq2logfreq_matrix, self.quef2logfreq_matrix)
        key = tuple((b.data_ptr(), b._version, b.device, tuple(b.shape)) for b in bufs)
        hit = self._derived.get(key)
        if hit is None:
            hit = engine.cfp_operands(*bufs, self.N)
            self._derived = {key: hit}  # (one entry: a module serves one device at a time)
        return hit

    def _forward(self, x):
        if x.dim() != 2:
            raise ValueError("CFP expects a (batch, samples) tensor, got shape %s" % (tuple(x.shape),))
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("CFP is not differentiable: call it under torch.no_grad() or on x.detach()")
        x = x.detach().to(torch.float32)
        # frames of the signal padded by N // 2 on both sides, as torch.stft counts them (1 + samples // hop for even N)
        T = 1 + (x.shape[1] + 2 * (self.N // 2) - self.N) // int(self.hop_length)
        first, n_frames = (1, max(T - 2, 0)) if self._drop_edge_frames else (0, T)
        out = engine.cfp(x, self.h, self.freq2logfreq_matrix, self.quef2logfreq_matrix, N=self.N,
                         hop=int(self.hop_length), g=[float(v) for v in np.ravel(self.g)], tc_idx=int(self.tc_idx),
                         fc_idx=int(self.fc_idx), first_frame=first, n_frames=n_frames,
                         outputs=4 if self._drop_edge_frames else 1, operands=self._operands)
        self.t = np.arange(self.hop_length, np.ceil(len(x) / float(self.hop_length)) * self.hop_length,
                           self.hop_length)
        return out

    def extra_repr(self) -> str:
        return "N={}, hop_length={}, window_size={}, g={}".format(self.N, self.hop_length, self.window_size, self.g)


_COMMON_DOC = """
    Same constructor arguments and defaults as the reference: ``fr`` (frequency resolution in Hz; ``N = int(fs / fr)``
    points per transform), ``fs``, ``hop_length``, ``window_size`` (Blackman-Harris window, centred in the N-point
    frame), ``fc`` (lowest frequency), ``tc`` (1 / highest frequency), ``g`` (one exponent per non-linear layer; 0
    means log) and ``NumPerOct``.  Same attributes (``window_size``, ``hop_length``, ``N``, ``pad_value``,
    ``NumofLayer``, ``g``, ``tc_idx``, ``fc_idx``, ``HighFreqIdx``, ``HighQuefIdx``, ``f``, ``q``) and buffers (``h``,
    ``freq2logfreq_matrix``, ``quef2logfreq_matrix``: equal to the reference's element for element).  ``t`` is set by
    every forward and is what the reference computes: ``arange(hop, ceil(len(x) / hop) hop, hop)`` with ``len(x)`` the
    BATCH size (the reference's expression; kept, it is documented as "not used").

    Input ``(batch, samples)``, zero-padded by ``N // 2`` on both sides, ``T = 1 + samples // hop_length`` frames:

        s0   = |DFT_N(h frame)| / ||h||                     spec = relu(s0) ** g[0]
        odd i:  ceps = nl(Re DFT_N(spec) / sqrt(N), g[i], tc_idx)
        even i: spec = nl(Re DFT_N(ceps) / sqrt(N), g[i], fc_idx)
        nl(X, g, c) = relu(X) with the first c and the last c bins zeroed, ** g   (g == 0: log(relu(X) + 1e-8))
        tfrL0 = F s0,  tfrLF = F spec,  tfrLQ = Q ceps,  Z = tfrLF tfrLQ          each (batch, rows of F, frames)

    Input of another floating type is converted to float32; the output is float32.

    Deliberate deviations from the reference:
      1. ``len(g) == 1`` raises ``ValueError`` at construction (the reference fails in forward on an unbound name);
      2. ``window_size > N`` raises ``ValueError`` at construction (the reference fails inside ``torch.stft``), and so
         does a quefrency axis longer than half a frame (the reference fails in its last matmul);
      3. input that is not 2-D raises ``ValueError`` (the reference fails inside ``torch.stft`` or later);
      4. it is not differentiable: with grad mode on and ``x.requires_grad`` it raises instead of returning a
         detached tensor;
      5. the window is ``scipy.signal.windows.blackmanharris`` (the name the reference uses left scipy in 1.13).
    Kept as the reference has it: a cutoff (``tc_idx`` / ``fc_idx``) of 0 zeroes the WHOLE layer (its ``X[-0:] = 0``).
"""


class Combined_Frequency_Periodicity(_CFPBase):
    _drop_edge_frames = True

    def forward(self, x):
        """``(batch, samples)`` -> ``(Z, tfrL0, tfrLF, tfrLQ)``, each ``(batch, n_out, T - 2)``."""
        return self._forward(x)


class CFP(_CFPBase):
    def forward(self, x):
        """``(batch, samples)`` -> ``Z`` ``(batch, n_out, T)``."""
        return self._forward(x)[0]


Combined_Frequency_Periodicity.__doc__ = (
    "Waveform -> ``(Z, tfrL0, tfrLF, tfrLQ)`` without the first and the last frame (``T - 2`` frames), as the\n"
    "    reference's class of this name." + _COMMON_DOC)
CFP.__doc__ = ("Waveform -> ``Z`` alone, all ``T`` frames (the frame count of the other spectrogram classes), as the\n"
               "    reference's class of this name." + _COMMON_DOC)
