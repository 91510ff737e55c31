"""Per-channel energy normalisation (PCEN): the trainable dynamic-range compression of Y. Wang, P. Getreuer, T. Hughes,
R. F. Lyon and R. A. Saurous, "Trainable Frontend For Robust and Far-Field Keyword Spotting", ICASSP 2017; the semantics
are ``librosa.pcen``'s with ``max_size=1`` and time on the last axis.  The reference has no counterpart.

The smoother is a first-order recurrence along time.  On CUDA tensors one wave per (clip, channel) row solves it by a
scan over chunks of 64 frames (``csrc/pcen.hip``), forward and backward in one launch each; CPU tensors without grad run
the library's host loop, and ``torch.compile``, CPU tensors with grad and ``engine.set_pcen_kernel(False)`` /
``MISPEC_PCEN_KERNEL=0`` run the same steps as torch operators (``engine.pcen_composition``).
"""
import numpy as np
import torch
import torch.nn as nn

from .. import engine


class PCEN(nn.Module):
    """``out = (S * (eps + M)**(-gain) + bias)**power - bias**power`` with the smoothed energy

        M[-1] = S[..., 0]   (or ``state``);      M[t] = (1 - b) * M[t-1] + b * S[..., t]

    for a non-negative spectrogram ``S`` of shape ``(batch, channels, frames)`` or ``(channels, frames)`` -- the output
    of ``MelSpectrogram`` or ``STFT(output_format="Magnitude")``.  ``b`` is given directly or derived from
    ``time_constant`` (seconds) as librosa does: ``Tf = time_constant * sr / hop_length``,
    ``b = (sqrt(1 + 4 Tf**2) - 1) / (2 Tf**2)``.

    ``gain``, ``bias``, ``power`` and ``b`` are tensors of shape ``(1,)``, or ``(n_bins,)`` when ``n_bins`` is given (one
    value per channel, initialised from the scalars): buffers, or ``nn.Parameter`` s with ``trainable=True``.  Training
    does not constrain them: keep ``b`` in (0, 1] and ``power`` positive (e.g. by clamping after the optimizer step).

    ``forward(S, state=None, return_state=False)``: ``state`` ``(batch, channels)`` is the smoother's last value of the
    previous chunk (chunked or streaming use: the chunks' outputs concatenate to the output of the whole);
    ``return_state=True`` returns ``(out, state)`` with the state detached.

    Deviations from ``librosa.pcen``:

    * time is the last axis and there is no ``axis`` argument; ``max_size`` is 1 (no max-filter over frequency, no
      ``max_axis``);
    * ``power`` must be > 0: the ``power == 0`` form ``log1p(S * smooth / bias)`` is not offered, and ``bias == 0`` goes
      through the general formula instead of librosa's special case (the same value);
    * the input is used as it is: librosa's default scaling of its examples (``S * 2**31``) is the caller's, and no
      warning is raised for unscaled input;
    * the initial state is librosa's default (``lfilter_zi`` scaled by the first frame, which for this filter is the
      first frame itself); a given ``state`` is ``M[-1]`` directly, librosa's ``zi`` is ``(1 - b)`` times it; the
      returned state likewise is ``M[..., -1]``, not ``zf``;
    * the smoothed energy enters as ``(eps + M)**(-gain)``, librosa evaluates ``exp(-gain * (log(eps) + log1p(M / eps)))``:
      equal up to rounding;
    * the parameters may differ per channel and be trained; the input and the output are float32 (other floating types
      are converted), every step in between is evaluated in float64 and the result rounded once.
    """

    def __init__(self, sr=22050, hop_length=512, gain=0.98, bias=2.0, power=0.5, time_constant=0.4, eps=1e-6, b=None,
                 n_bins=None, trainable=False):
        super().__init__()
        if not eps > 0:
            raise ValueError("PCEN: eps must be > 0, got %r" % (eps,))
        if not power > 0:
            raise ValueError("PCEN: power must be > 0 (the power == 0 log form is not offered), got %r" % (power,))
        if gain < 0:
            raise ValueError("PCEN: gain must be >= 0, got %r" % (gain,))
        if bias < 0:
            raise ValueError("PCEN: bias must be >= 0, got %r" % (bias,))
        if b is None:
            if not (time_constant > 0 and sr > 0 and hop_length > 0):
                raise ValueError("PCEN: time_constant, sr and hop_length must be > 0")
            t_frames = time_constant * sr / float(hop_length)
            b = (np.sqrt(1.0 + 4.0 * t_frames ** 2) - 1.0) / (2.0 * t_frames ** 2)
        if not 0 < b <= 1:
            raise ValueError("PCEN: b must be in (0, 1], got %r" % (b,))
        if n_bins is not None and int(n_bins) < 1:
            raise ValueError("PCEN: n_bins must be >= 1, got %r" % (n_bins,))
        self.sr, self.hop_length, self.time_constant = sr, hop_length, time_constant
        self.eps = float(eps)
        self.n_bins = None if n_bins is None else int(n_bins)
        self.trainable = trainable
        n = 1 if n_bins is None else int(n_bins)
        for name, value in (("gain", gain), ("bias", bias), ("power", power), ("b", b)):
            t = torch.full((n,), float(value), dtype=torch.float32)
            if trainable:
                self.register_parameter(name, nn.Parameter(t, requires_grad=True))
            else:
                self.register_buffer(name, t)

    def forward(self, S, state=None, return_state=False):
        squeeze = S.dim() == 2
        if squeeze:
            S = S[None]
        if S.dim() != 3:
            raise ValueError("PCEN expects (batch, channels, frames) or (channels, frames), got shape %s" % (tuple(S.shape),))
        if self.n_bins is not None and S.shape[1] != self.n_bins:
            raise ValueError("PCEN: this module has %d channels, the input has %d" % (self.n_bins, S.shape[1]))
        if state is not None and state.dim() == 1 and squeeze:
            state = state[None]
        out, last = engine.pcen(S.to(torch.float32), self.b, self.gain, self.bias, self.power, self.eps,
                                None if state is None else state.to(torch.float32))
        if squeeze:
            out, last = out[0], last[0]
        return (out, last) if return_state else out

    def extra_repr(self) -> str:
        def show(t):
            t = t.detach()
            return "%g" % float(t[0]) if t.numel() == 1 or bool((t == t[0]).all()) else "per-channel"

        return "gain={}, bias={}, power={}, b={}, eps={:g}, n_bins={}, trainable={}".format(
            show(self.gain), show(self.bias), show(self.power), show(self.b), self.eps, self.n_bins, self.trainable)
