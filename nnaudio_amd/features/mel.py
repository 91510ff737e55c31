"""Mel spectrogram module (drop-in for ``nnAudio.features.MelSpectrogram``,
reference: Installation/nnAudio/features/mel.py:9-194).

The pipeline itself (STFT power spectrum -> filterbank) is shared with Gammatonegram:
``features/_filterbank.py``.

``MelSpectrogram.to_stft`` / ``MelSpectrogram.inverse`` go the other way (as in later releases of nnAudio, librosa's
``mel_to_stft`` / ``mel_to_audio`` and torchaudio's ``InverseMelScale``): a non-negative least squares problem per frame
column, on CUDA tensors solved by one launch that keeps the sparse bank and a tile of frames on chip
(``csrc/mel_nnls.hip``), then ``Griffin_Lim``."""

import torch
import torch.nn as nn

from .. import engine
from ..basis import dct_ortho_matrix, mel_filterbank
from ..utils import ParameterError
from ._filterbank import FilterbankSpectrogram


class MelSpectrogram(FilterbankSpectrogram):
    """``(batch, n_mels, frames)`` mel spectrogram; constructor, attributes and
    ``state_dict`` keys (``mel_basis``, ``stft.wsin`` ...) as the reference."""

    _basis_name, _label = "mel_basis", "Mel"

    def __init__(
        self,
        sr=22050,
        n_fft=2048,
        win_length=None,
        n_mels=128,
        hop_length=512,
        window="hann",
        center=True,
        pad_mode="reflect",
        power=2.0,
        htk=False,
        fmin=0.0,
        fmax=None,
        norm=1,
        trainable_mel=False,
        trainable_STFT=False,
        verbose=True,
        **kwargs
    ):
        super().__init__()
        self.trainable_mel = trainable_mel
        self._build(
            lambda: torch.from_numpy(mel_filterbank(sr, n_fft, n_mels, fmin, fmax, htk=htk, norm=norm)),
            sr=sr, n_fft=n_fft, win_length=win_length, hop_length=hop_length, window=window,
            center=center, pad_mode=pad_mode, power=power, trainable_basis=trainable_mel,
            trainable_STFT=trainable_STFT, verbose=verbose, stft_kwargs=kwargs)

    def extra_repr(self) -> str:
        return "Mel filter banks size = {}, trainable_mel={}".format(
            (*self.mel_basis.shape,), self.trainable_mel, self.trainable_STFT
        )

    # ------------------------------------------------------------------ #
    def _nnls_operands(self):
        """The inversion's derived operands (L, sparse tables, momentum tables) per (bank identity, version, device,
        power): a plain attribute, never a buffer -- ``state_dict`` does not change."""
        b = self.mel_basis
        key = (b.data_ptr(), b._version, b.device, tuple(b.shape), float(self.power))
        cache = self.__dict__.setdefault("_nnls_derived", {})
        hit = cache.get(key)
        if hit is None:
            hit = engine.mel_nnls_operands(b, self.power)
            self.__dict__["_nnls_derived"] = {key: hit}  # (one entry: a module serves one device at a time)
        return hit

    def to_stft(self, melspec, n_iter=256, momentum=True):
        """Mel spectrogram ``(batch, n_mels, frames)`` (or ``(n_mels, frames)``: a batch of one) -> magnitude
        spectrogram ``(batch, n_fft // 2 + 1, frames)``, float32: per frame column ``m`` the non-negative least squares
        problem ``min_{p >= 0} || M p - m ||^2`` (``M = mel_basis``) by a FIXED number of projected gradient steps with
        Nesterov momentum (FISTA) -- no early stopping, no host synchronisation, nothing random:

            L = largest eigenvalue of M M^T (float64, once per bank version);  eta = 1 / L
            beta_k = (t_k - 1) / t_{k+1},  t_0 = 1,  t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2     (momentum=False: 0)
            p = y = 0
            n_iter times:  r = M y - m;  p+ = max(y - eta M^T r, 0);  y = p+ + beta_k (p+ - p);  p = p+
            return p ** (1 / power)

        An all-zero bank (L == 0) and ``n_iter=0`` return zeros; bins no filter covers (below ``fmin`` / above
        ``fmax``) come back exactly 0.  The result is *a* non-negative spectrum whose mel projection matches ``melspec``,
        not *the* spectrum it was computed from: the problem is underdetermined (``n_mels`` equations for
        ``n_fft // 2 + 1`` unknowns), and for random non-negative spectra the recovered one differs from the true one by
        0.4 - 0.8 in relative L2 while its projection agrees to 1e-6 of the input's norm.

        CUDA tensors with a bank the library serves (``engine.mel_nnls_served``: sparse, contiguous rows -- every bank
        ``basis.mel_filterbank`` builds) run all steps in one launch, with the iterate in float64 and one rounding at
        the end; CPU tensors and other banks (a trained ``mel_basis``) run the same steps as float32 torch operators
        (``engine.mel_nnls_composition``).  Not differentiable:
        with grad mode on and ``melspec.requires_grad`` it raises."""
        if melspec.dim() == 2:
            melspec = melspec[None]
        if melspec.dim() != 3:
            raise ValueError("to_stft expects (batch, n_mels, frames) or (n_mels, frames), got shape %s"
                             % (tuple(melspec.shape),))
        n_mels = self.mel_basis.shape[0]
        if melspec.shape[1] != n_mels:
            raise ValueError("to_stft: this module has %d mel bands, the input has %d" % (n_mels, melspec.shape[1]))
        if torch.is_grad_enabled() and melspec.requires_grad:
            raise RuntimeError("to_stft is not differentiable: call it under torch.no_grad() or on melspec.detach()")
        mel = melspec.detach().to(torch.float32)
        return engine.mel_nnls(mel, self.mel_basis, power=self.power, n_iter=n_iter, momentum=momentum,
                               operands=self._nnls_operands)

    def inverse(self, melspec, n_iter=256, momentum=True, griffin_lim_iter=32, griffin_lim_momentum=0.99):
        """Mel spectrogram -> waveform ``(batch, samples)``: ``to_stft(melspec, n_iter, momentum)``, then
        ``Griffin_Lim`` with this module's ``n_fft``, ``stride`` (hop length), ``win_length``, ``window``, ``center`` and
        ``pad_mode``, built once per ``(griffin_lim_iter, griffin_lim_momentum)`` and kept as a plain attribute.  The
        initial phase is Griffin_Lim's one draw from the default generator: ``torch.manual_seed`` pins the result."""
        from .griffin_lim import Griffin_Lim

        S = self.to_stft(melspec, n_iter=n_iter, momentum=momentum)
        key = (int(griffin_lim_iter), float(griffin_lim_momentum))
        cache = self.__dict__.setdefault("_griffin_lim", {})
        gl = cache.get(key)
        if gl is None:
            gl = Griffin_Lim(int(self.n_fft), n_iter=key[0], hop_length=int(self.stride), win_length=self.stft.win_length,
                             window=self.stft.window, center=self.center, pad_mode=self.pad_mode, momentum=key[1])
            self.__dict__["_griffin_lim"] = {key: gl}
        return gl(S)


class MFCC(nn.Module):
    """Mel-frequency cepstral coefficients: ``MelSpectrogram`` -> ``power_to_db`` (per-clip
    ``top_db`` floor) -> orthonormal DCT-II over the mel axis -> first ``n_mfcc`` rows.
    Same constructor, buffers (``amin``, ``ref``, ``melspec_layer.*``) and output
    ``(batch, n_mfcc, frames)`` as the reference (mel.py:197-329).  The DCT runs as the same planar
    contraction kernel as the mel filterbank, with the (n_mfcc, n_mels) cosine matrix the
    reference evaluates through an FFT."""

    def __init__(self, sr=22050, n_mfcc=20, norm="ortho", verbose=True, ref=1.0, amin=1e-10,
                 top_db=80.0, **kwargs):
        super().__init__()
        self.melspec_layer = MelSpectrogram(sr=sr, verbose=verbose, **kwargs)
        self.m_mfcc = n_mfcc
        if amin <= 0:
            raise ParameterError("amin must be strictly positive")
        self.register_buffer("amin", torch.tensor([amin]))
        self.register_buffer("ref", torch.abs(torch.tensor([ref])))
        # host copies of the two scalars: forward must not read device buffers back (a
        # device-to-host sync per call, and it would break stream capture); refreshed by
        # load_state_dict
        self._amin_f, self._ref_f = float(amin), abs(float(ref))
        self.top_db = top_db
        self.n_mfcc = n_mfcc
        n_mels = self.melspec_layer.mel_basis.shape[0]
        # derived constant, not part of the reference's state_dict
        self.register_buffer("_dct_basis", torch.from_numpy(dct_ortho_matrix(min(n_mfcc, n_mels), n_mels)),
                             persistent=False)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
        self._amin_f = float(self.amin.detach().cpu())
        self._ref_f = float(self.ref.detach().cpu())

    def forward(self, x):
        spec = self.melspec_layer(x)
        if self.top_db is not None and self.top_db < 0:
            raise ParameterError("top_db must be non-negative")
        if spec.is_cuda and not engine.compiling() and not (torch.is_grad_enabled() and spec.requires_grad):
            # nothing to differentiate: decibels + DCT in one launch (mispec_mfcc_tail_f32)
            y = engine.mfcc_tail(spec, self._amin_f, self._ref_f, self.top_db, self._dct_basis)
            if y is not None:
                return y
        db = engine.power_to_db_autograd(spec, self._amin_f, self._ref_f, self.top_db)
        return engine.filterbank_autograd(self._dct_basis, db)

    def extra_repr(self) -> str:
        return "n_mfcc = {}".format((self.n_mfcc))
