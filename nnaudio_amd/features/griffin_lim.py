"""Griffin-Lim phase reconstruction (drop-in for ``nnAudio.features.Griffin_Lim``,
reference: Installation/nnAudio/features/griffin_lim.py:8-147).

Every iteration is one inverse STFT and one forward STFT of the same window x DFT basis: both run on the
library's transforms (the fp32 FFT kernels where the shape allows), and the phase update is fused into the forward
transform's tile flush (``engine.griffin_lim``).
"""
import numpy as np
import torch
import torch.nn as nn

from .. import engine


class Griffin_Lim(nn.Module):
    """Magnitude spectrogram ``(batch, n_fft // 2 + 1, frames)`` -> waveform ``(batch, samples)`` by the "fast
    Griffin-Lim" algorithm (Perraudin, Balazs & Soendergaard, WASPAA 2013), as librosa.griffinlim:

        beta = momentum / (1 + momentum),  tprev = 0,  A = (cos 2 pi r, sin 2 pi r),  r = torch.randn(S.shape)
        n_iter times:  y = iSTFT(S A);  R = STFT(y);  a = R - beta tprev;  A = a / (|a| + 1e-16);  tprev = R
        return iSTFT(S A)

    Same constructor arguments, defaults and attributes (``n_fft``, ``n_iter``, ``hop_length``, ``win_length``,
    ``center``, ``pad_mode``, ``momentum``, ``device``, ``w``) as the reference, and the same (empty) ``state_dict``.
    The initial phase is ONE draw ``torch.randn(S.shape, device=S.device)`` from the default generator, before any
    other random call.  Both transforms use ``w`` centre-padded to ``n_fft`` (as ``torch.stft`` / ``torch.istft``
    do); the inverse divides by the window-sum-square.  Output: float32, ``hop (T - 1)`` samples when centred,
    ``n_fft + hop (T - 1)`` when not (``torch.istft`` without ``length``).

    ``precision`` (not a constructor argument; None = the STFT family's default) names the arithmetic of the
    contraction route, as on ``STFT``; the FFT route is fp32 whatever it says.

    Deliberate deviations from the reference:
      1. it runs on torch >= 2 (the reference hands a real ``(..., 2)`` tensor to ``torch.istft``, which raises);
      2. the phase is drawn on ``S.device``, not on the constructor's ``device`` (the reference fails when they differ);
      3. ``center`` applies to both transforms, as in librosa (the reference always centres its ``torch.stft``, so
         ``center=False`` ends in a shape mismatch there);
      4. it is not differentiable: with grad mode on and ``S.requires_grad`` it raises instead of returning a
         detached tensor.
    """

    def __init__(self, n_fft, n_iter=32, hop_length=None, win_length=None, window="hann", center=True,
                 pad_mode="reflect", momentum=0.99, device="cpu"):
        super().__init__()
        self.n_fft = n_fft
        self.n_iter = n_iter
        self.center = center
        self.pad_mode = pad_mode
        self.momentum = momentum
        self.device = device
        self.win_length = n_fft if win_length is None else win_length
        self.hop_length = n_fft // 4 if hop_length is None else hop_length
        from scipy.signal import get_window

        # a plain attribute, as in the reference (its state_dict is empty)
        self.w = torch.tensor(get_window(window, int(self.win_length), fftbins=True), device=device).float()
        self.precision = None
        # per (device, precision, window version): window, bases and their derived operands -- not buffers
        self._derived = {}

    # ------------------------------------------------------------------ #
    def _operands(self, dev, precision):
        w = self.w
        key = (dev, precision, w.data_ptr(), w._version, tuple(w.shape))
        hit = self._derived.get(key)
        if hit is not None:
            return hit
        N = int(self.n_fft)
        wl = w.numel()
        if wl > N:
            raise RuntimeError("Griffin_Lim: win_length (%d) must be <= n_fft (%d)" % (wl, N))
        left = (N - wl) // 2  # centre-padded as torch.stft / torch.istft pad a shorter window
        window = torch.zeros(N, dtype=torch.float32, device=dev)
        window[left:left + wl] = w.detach().to(device=dev, dtype=torch.float32)
        F = N // 2 + 1
        n = np.arange(N)[:, None]
        k = np.arange(F)[None, :]
        ang = 2.0 * np.pi * ((n * k) % N) / N  # (N, F)
        # forward: window x DFT rows (the STFT module's basis with freq_scale='no'); inverse: [c cos | -c sin] with the
        # mirrored bins of the one-sided spectrum folded in (c = 1 at DC and Nyquist, 2 between: engine.istft_basis)
        cos_t = torch.from_numpy(np.cos(ang).T.astype(np.float32)).to(dev)
        sin_t = torch.from_numpy(np.sin(ang).T.astype(np.float32)).to(dev)
        basis_re = (cos_t * window).contiguous()
        basis_im = (sin_t * window).contiguous()
        c = np.full((1, F), 2.0)
        c[0, 0] = c[0, -1] = 1.0
        inv = np.concatenate((c * np.cos(ang), -c * np.sin(ang)), 1).astype(np.float32)
        inv_basis = torch.from_numpy(inv).to(dev)
        prep = engine.prepare_basis(basis_re, basis_im, precision, hop=self.hop_length) if dev.type == "cuda" else {}
        dft = dev.type == "cuda" and engine.istft_basis_is_dft(inv_basis, F)
        val = (window, basis_re, basis_im, inv_basis, dft, prep)
        self._derived = {key: val}  # (one entry: a module serves one device at a time)
        return val

    def _padding(self, out_len):
        """(pad, PAD_* id) of the forward transform, with STFT._framing's rule for reflect padding."""
        if not self.center:
            return 0, engine.PAD_NONE
        pad = int(self.n_fft) // 2
        if self.pad_mode == "constant":
            return pad, engine.PAD_ZERO
        if self.pad_mode == "reflect":
            if out_len < pad:
                raise AssertionError("Signal length shorter than reflect padding length (n_fft // 2).")
            return pad, engine.PAD_REFLECT
        raise ValueError("Griffin_Lim: pad_mode must be 'reflect' or 'constant', got %r" % (self.pad_mode,))

    def forward(self, S):
        """Convert a batch of magnitude spectrograms ``(batch, n_fft // 2 + 1, timesteps)`` to waveforms."""
        assert S.dim() == 3, "Please make sure your input is in the shape of (batch, freq_bins, timesteps)"
        if torch.is_grad_enabled() and S.requires_grad:
            raise RuntimeError("Griffin_Lim is not differentiable: call it under torch.no_grad() or on S.detach()")
        N, hop = int(self.n_fft), int(self.hop_length)
        F = N // 2 + 1
        if S.shape[1] != F:
            raise RuntimeError("Griffin_Lim(n_fft=%d) expects %d frequency bins, got %d" % (N, F, S.shape[1]))
        if hop <= 0:
            raise RuntimeError("Griffin_Lim: hop_length must be positive")
        dev = S.device
        mag = S.detach().to(torch.float32).contiguous()
        T = mag.shape[2]
        out_len = N + hop * (T - 1) - (2 * (N // 2) if self.center else 0)
        pad, pad_mode = self._padding(out_len)
        # the initial phase: ONE draw from the default generator (pinned: tests reproduce it); the angle and
        # S x (cos, sin) in float64, once per call (setup, not part of the iteration)
        r = torch.randn(mag.shape, device=dev, dtype=torch.float32)
        ph = (2.0 * np.pi) * r.double()
        m64 = mag.double()
        spec = torch.stack((m64 * torch.cos(ph), m64 * torch.sin(ph)), -1).to(torch.float32).contiguous()
        del r, ph, m64
        precision = engine.resolve_precision(self.precision, "f16x3")
        window, basis_re, basis_im, inv_basis, dft, prep = self._operands(dev, precision)
        beta = self.momentum / (1.0 + self.momentum)
        return engine.griffin_lim(mag, spec, n_iter=int(self.n_iter), beta=beta, inv_basis=inv_basis, dft=dft,
                                  window=window, hop=hop, pad=pad, pad_mode=pad_mode, basis_re=basis_re,
                                  basis_im=basis_im, precision=precision, prep=prep)

    def extra_repr(self) -> str:
        return "n_fft={}, n_iter={}, hop_length={}, win_length={}, momentum={}".format(
            self.n_fft, self.n_iter, self.hop_length, self.win_length, self.momentum)
