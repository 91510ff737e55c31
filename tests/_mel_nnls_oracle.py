"""NumPy statement of the mel inversion as ``MelSpectrogram.to_stft`` defines it (its docstring), dense, with the
arithmetic type a parameter: float64 is the truth, float32 the YARDSTICK -- an independent fp32 run, not the code under
test.  The rule both suites apply is tests/_cfp_cases.py's:

    err(ours vs oracle-float64)  <=  4 x err(oracle-float32 vs oracle-float64)        for max and for RMS,

over ALL elements; where the right-hand side is 0 (an all-zero input) ours must be exactly 0.  The rule is relative to
the yardstick because the fp32 drift itself depends on the settings: momentum accumulates rounding in the null space of
M (1e-4 of the peak after 256 steps, against 1e-6 without momentum)."""
import numpy as np

FACTOR = 4.0

# the banks of both suites: (sr, n_fft, n_mels, fmin, fmax, htk, norm)
BANKS = {
    "16/256": dict(sr=22050, n_fft=256, n_mels=16),
    "80/512": dict(sr=22050, n_fft=512, n_mels=80),
    "128/2048": dict(sr=22050, n_fft=2048, n_mels=128),
    "128/2048-htk": dict(sr=22050, n_fft=2048, n_mels=128, htk=True, norm=None),
    "40/1024-band": dict(sr=22050, n_fft=1024, n_mels=40, fmin=300.0, fmax=6000.0),
    "empty-rows": dict(sr=22050, n_fft=256, n_mels=128),
}


def betas(n_iter, momentum):
    """beta_k = (t_k - 1) / t_{k+1} in float64, rounded to the float32 table every route reads."""
    out = np.zeros(n_iter, dtype=np.float32)
    t = 1.0
    for k in range(n_iter):
        t_next = (1.0 + np.sqrt(1.0 + 4.0 * t * t)) / 2.0
        if momentum:
            out[k] = (t - 1.0) / t_next
        t = t_next
    return out


def lipschitz(M):
    M = np.asarray(M, dtype=np.float64)
    return float(np.linalg.eigvalsh(M @ M.T)[-1])


def nnls(mel, M, *, power, n_iter, momentum, dtype=np.float64):
    """mel (B, n_mels, T), M (n_mels, F) -> (B, F, T) in ``dtype``; every product, sum and constant in ``dtype``."""
    L = lipschitz(M)
    mel = np.asarray(mel).astype(dtype)
    Md = np.asarray(M).astype(dtype)
    B, _, T = mel.shape
    p = np.zeros((B, Md.shape[1], T), dtype=dtype)
    if L <= 0.0 or n_iter <= 0:
        return p
    eta = dtype(1.0 / L)
    beta = betas(n_iter, momentum).astype(dtype)
    y = p
    for k in range(n_iter):
        r = (Md @ y - mel).astype(dtype)
        pn = np.maximum(y - eta * (Md.T @ r), dtype(0)).astype(dtype)
        y = (pn + beta[k] * (pn - p)).astype(dtype)
        p = pn
    if power == 1:
        return p
    return np.sqrt(p) if power == 2 else p ** dtype(1.0 / power)


def errors(got, want):
    """(max, RMS) of got - want over ALL elements, in float64."""
    d = np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)
    if d.size == 0:
        return 0.0, 0.0
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


_cache = {}


def reference(key, mel, M, **kw):
    """(float64 result, (max, rms) of the float32 yardstick against it), computed once per ``key`` and shared."""
    hit = _cache.get(key)
    if hit is None:
        want = nnls(mel, M, dtype=np.float64, **kw)
        hit = (want, errors(nnls(mel, M, dtype=np.float32, **kw), want))
        want.setflags(write=False)
        _cache[key] = hit
    return hit


def check_rule(label, got, want, yard, extra=""):
    """Print the figures, then assert the rule.  Returns (max ratio, rms ratio)."""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert got.dtype == np.float32, (label, got.dtype)
    e_max, e_rms = errors(got, want)
    peak = float(np.abs(want).max()) if want.size else 0.0
    print("%s: max %.3e (oracle f32 %.3e) rms %.3e (oracle f32 %.3e) peak %.3e%s"
          % (label, e_max, yard[0], e_rms, yard[1], peak, extra))
    if yard[0] == 0.0:
        assert not got.any(), label
        return 0.0, 0.0
    assert e_max <= FACTOR * yard[0] and e_rms <= FACTOR * yard[1], (label, e_max, yard[0], e_rms, yard[1])
    return e_max / yard[0], e_rms / yard[1]
