"""Float64 statement of Griffin-Lim as ``nnaudio_amd.features.Griffin_Lim`` defines it (its docstring; the reference's
fast Griffin-Lim, whose own module does not run on torch >= 2, so it has no outputs to compare with): NumPy FFTs,
the window centre-padded to n_fft, reflect / zero padding and window-sum-square normalisation as torch.stft /
torch.istft do them.  Shared by tests/test_griffin_lim_cpu.py and tests/test_gpu_griffin_lim.py."""
import numpy as np
from scipy.signal import get_window


def window(n_fft, win_length=None, name="hann"):
    """The module's ``w`` (float32, as the reference builds it), centre-padded to n_fft, in float64."""
    wl = n_fft if win_length is None else win_length
    w = get_window(name, wl, fftbins=True).astype(np.float32).astype(np.float64)
    out = np.zeros(n_fft)
    left = (n_fft - wl) // 2
    out[left:left + wl] = w
    return out


def stft(y, n_fft, hop, w, center=True, pad_mode="reflect"):
    """(B, L) -> complex (B, n_fft // 2 + 1, T)"""
    y = np.asarray(y, dtype=np.float64)
    if center:
        p = n_fft // 2
        y = np.pad(y, ((0, 0), (p, p)), mode="reflect" if pad_mode == "reflect" else "constant")
    T = 1 + (y.shape[1] - n_fft) // hop
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    frames = y[:, idx] * w  # (B, T, N)
    return np.fft.rfft(frames, axis=-1).transpose(0, 2, 1)


def istft(X, n_fft, hop, w, center=True):
    """complex (B, F, T) -> (B, n_fft + hop (T - 1) [- 2 (n_fft // 2) when centred]); where the window-sum-square is
    <= 1e-10 the overlap-add is left undivided (the library's rule; torch.istft refuses such input instead)."""
    B, F, T = X.shape
    frames = np.fft.irfft(X.transpose(0, 2, 1), n=n_fft, axis=-1) * w  # (B, T, N)
    full = n_fft + hop * (T - 1)
    y = np.zeros((B, full))
    wss = np.zeros(full)
    for t in range(T):
        y[:, t * hop:t * hop + n_fft] += frames[:, t]
        wss[t * hop:t * hop + n_fft] += w * w
    y = np.where(wss > 1e-10, y / np.where(wss > 1e-10, wss, 1.0), y)
    if center:
        y = y[:, n_fft // 2:full - n_fft // 2]
    return y


def griffin_lim(S, r, n_iter, n_fft, hop=None, win_length=None, center=True, pad_mode="reflect", momentum=0.99,
                return_phase=False):
    """S (B, F, T) magnitude, r the module's initial draw (torch.randn(S.shape)) as an array -> float64 waveform."""
    hop = n_fft // 4 if hop is None else hop
    w = window(n_fft, win_length)
    S = np.asarray(S, dtype=np.float64)
    A = np.exp(2j * np.pi * np.asarray(r, dtype=np.float64))
    beta = momentum / (1.0 + momentum)
    tprev = np.zeros_like(A)
    for _ in range(n_iter):
        y = istft(S * A, n_fft, hop, w, center)
        R = stft(y, n_fft, hop, w, center, pad_mode)
        a = R - beta * tprev
        A = a / (np.abs(a) + 1e-16)
        tprev = R
    y = istft(S * A, n_fft, hop, w, center)
    return (y, A) if return_phase else y


def chirp(B, L, sr=16000.0, seed=0):
    """B seeded test clips: a linear chirp with a little noise, float32."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / sr
    out = []
    for b in range(B):
        f0, f1 = 200.0 + 150.0 * b, 3000.0 + 500.0 * b
        ph = 2 * np.pi * (f0 * t + 0.5 * (f1 - f0) * t * t / t[-1])
        out.append(0.5 * np.sin(ph) + 0.05 * rng.standard_normal(L))
    return np.stack(out).astype(np.float32)


def spectral_convergence(y, S, n_fft, hop, win_length=None, center=True, pad_mode="reflect"):
    """|| |STFT(y)| - S || / || S ||  (float64)"""
    w = window(n_fft, win_length)
    M = np.abs(stft(y, n_fft, hop, w, center, pad_mode))
    S = np.asarray(S, dtype=np.float64)
    return float(np.linalg.norm(M - S) / np.linalg.norm(S))


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))
