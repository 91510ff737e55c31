"""NumPy statement of PCEN as ``features.PCEN`` defines it (its docstring): the smoother as a SEQUENTIAL recurrence over
the frames, the pointwise part as written, with the arithmetic type a parameter -- float64 is the truth, float32 the
YARDSTICK, an independent float32 run and not the code under test -- and the closed-form gradients in float64.  The
rule every PCEN suite applies is tests/_cfp_cases.py's and tests/_mel_nnls_oracle.py's:

    err(ours vs oracle-float64)  <=  4 x err(yardstick-float32 vs oracle-float64)        for max and for RMS,

over ALL elements of a case; where the right-hand side is 0 ours must be exactly 0.  For the forward the yardstick is
this file's float32 run, for the gradients the float32 autograd of ``engine.pcen_composition`` on the CPU.

The parameters and eps are float32 numbers (what the module holds and the library receives): both runs start from the
same float32 values, converted to the run's type."""
import numpy as np

FACTOR = 4.0

# (b, gain, bias, power, eps)
PARAMS = [
    (0.025, 0.98, 2.0, 0.5, 1e-6),
    (0.04, 0.8, 10.0, 0.25, 1e-6),
    (0.5, 1.0, 1.0, 1.0, 1e-6),
    (0.015, 0.6, 0.5, 0.7, 1e-12),
]
INPUTS = ("randn2", "randn2-2^31", "bursts", "ramp", "randn2-1e-9", "zeros")
# the chunk edges of a 64-frame scan: one frame, two, 63 / 64 / 65, two chunks and one more, several chunks with a tail,
# more rows than one workgroup, more channels than any block
SHAPES = [(1, 1, 1), (1, 1, 2), (2, 3, 63), (2, 3, 64), (2, 3, 65), (1, 5, 128), (1, 5, 129), (3, 17, 203), (2, 128, 130),
          (1, 1025, 70)]
GRAD_SHAPES = [(1, 5, 1), (2, 3, 65), (3, 17, 203)]


def make_input(name, shape, seed=0):
    """A non-negative float32 spectrogram (B, F, T)."""
    B, F, T = shape
    rng = np.random.default_rng(seed)
    if name == "randn2":
        x = rng.standard_normal(shape) ** 2
    elif name == "randn2-2^31":
        x = rng.standard_normal(shape) ** 2 * 2.0 ** 31
    elif name == "randn2-1e-9":
        x = rng.standard_normal(shape) ** 2 * 1e-9
    elif name == "bursts":  # a quiet background, +50 over ten frames, +1e3 on one frame (where the row is long enough)
        x = np.full(shape, 1e-4)
        for r in range(B * F):
            bi, f = divmod(r, F)
            t0 = int(rng.integers(0, max(T - 10, 1)))
            x[bi, f, t0:t0 + 10] += 50.0
            x[bi, f, int(rng.integers(0, T))] += 1e3
    elif name == "ramp":
        x = np.broadcast_to(np.linspace(0.0, 5.0, T), shape) * (1.0 + np.arange(F)[None, :, None] / F)
    elif name == "zeros":
        x = np.zeros(shape)
    else:
        raise KeyError(name)
    return np.ascontiguousarray(x, dtype=np.float32)


def params_f32(pset, n=None):
    """(b, gain, bias, power) as float32 arrays of shape (1,), or (n,) with a distinct value per channel, and eps."""
    b, gain, bias, power, eps = pset
    if n is None:
        return tuple(np.full(1, v, dtype=np.float32) for v in (b, gain, bias, power)) + (np.float32(eps),)
    ch = np.arange(n) / float(n)
    return ((b * (1.0 + 0.5 * ch)).astype(np.float32), (gain * (1.0 - 0.3 * ch)).astype(np.float32),
            (bias * (1.0 + 0.7 * ch)).astype(np.float32), (power * (1.0 + 0.4 * ch)).astype(np.float32), np.float32(eps))


def _col(p, dtype):
    return np.asarray(p, dtype=np.float32).astype(dtype).reshape(1, -1)


def smooth(S, b, state=None, dtype=np.float64):
    """M (B, F, T) of the sequential recurrence, every product and sum in ``dtype``."""
    S = np.asarray(S).astype(dtype)
    b = _col(b, dtype)
    a = (dtype(1) - b).astype(dtype)
    m = S[..., 0] if state is None else np.asarray(state).astype(dtype)
    M = np.empty(S.shape, dtype=dtype)
    for t in range(S.shape[-1]):
        m = (a * m + b * S[..., t]).astype(dtype)
        M[..., t] = m
    return M


def pcen(S, b, gain, bias, power, eps, state=None, dtype=np.float64):
    """(out, M) in ``dtype``."""
    M = smooth(S, b, state, dtype)
    S = np.asarray(S).astype(dtype)
    gain, bias, power = (_col(p, dtype)[..., None] for p in (gain, bias, power))
    eps = dtype(np.float32(eps))
    with np.errstate(over="ignore"):
        out = ((S * (eps + M) ** (-gain) + bias) ** power - bias ** power).astype(dtype)
    return out, M


def gradients(S, G, b, gain, bias, power, eps, state=None):
    """The closed-form gradients of sum(G * out) in float64: dict with dS (B, F, T), dstate (B, F) or None, and db,
    dgain, dbias, dpower of the parameters' shape ((1,): summed over everything, (F,): over clips and frames)."""
    f8 = np.float64
    _, M = pcen(S, b, gain, bias, power, eps, state, f8)
    S, G = np.asarray(S).astype(f8), np.asarray(G).astype(f8)
    n = np.asarray(b).size
    bc = _col(b, f8)
    b3 = bc[..., None]
    gain, bias, power = (_col(p, f8)[..., None] for p in (gain, bias, power))
    eps = f8(np.float32(eps))
    u = eps + M
    q = u ** (-gain)
    P = S * q
    z = P + bias
    c = power * z ** (power - 1.0)
    gc = G * c
    gM = -gain * gc * P / u
    lam = np.empty_like(gM)
    nxt = np.zeros(S.shape[:2])
    for t in range(S.shape[-1] - 1, -1, -1):
        nxt = gM[..., t] + (1.0 - bc) * nxt
        lam[..., t] = nxt
    dS = gc * q + b3 * lam
    tail = (1.0 - bc) * lam[..., 0]
    first = S[..., 0] if state is None else np.asarray(state).astype(f8)
    if state is None:
        dS[..., 0] += tail
    Mprev = np.concatenate([first[..., None], M[..., :-1]], axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        zlog = np.where(z > 0, z ** power * np.log(np.where(z > 0, z, 1.0)), 0.0)
        blog = np.where(bias > 0, bias ** power * np.log(np.where(bias > 0, bias, 1.0)), 0.0)
    per = {"db": lam * (S - Mprev), "dgain": -gc * P * np.log(u), "dbias": G * (c - power * bias ** (power - 1.0)),
           "dpower": G * (zlog - blog)}
    out = {"dS": dS, "dstate": None if state is None else tail}
    for k, v in per.items():
        out[k] = v.sum(axis=(0, 2)) if n > 1 else v.sum().reshape(1)
    return out


def errors(got, want):
    """(max, RMS) of got - want over ALL elements, in float64."""
    d = np.asarray(got, dtype=np.float64) - np.asarray(want, dtype=np.float64)
    if d.size == 0:
        return 0.0, 0.0
    return float(np.abs(d).max()), float(np.sqrt(np.mean(d * d)))


_cache = {}


def reference(key, S, b, gain, bias, power, eps, state=None):
    """(float64 out, float64 M, (max, rms) of the float32 yardstick's out against it), once per ``key``, shared."""
    hit = _cache.get(key)
    if hit is None:
        want, M = pcen(S, b, gain, bias, power, eps, state, np.float64)
        hit = (want, M, errors(pcen(S, b, gain, bias, power, eps, state, np.float32)[0], want))
        want.setflags(write=False)
        M.setflags(write=False)
        _cache[key] = hit
    return hit


def check_rule(label, got, want, yard, report=None):
    """Print the figures, then assert the rule.  Returns (max ratio, rms ratio)."""
    got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    assert got.dtype == np.float32, (label, got.dtype)
    e_max, e_rms = errors(got, want)
    peak = float(np.abs(want).max()) if want.size else 0.0
    print("%s: max %.3e (yardstick %.3e) rms %.3e (yardstick %.3e) peak %.3e" % (label, e_max, yard[0], e_rms, yard[1], peak))
    if yard[0] == 0.0:
        assert not (got - want.astype(np.float32)).any(), label
        ratios = (0.0, 0.0)
    else:
        assert e_max <= FACTOR * yard[0] and e_rms <= FACTOR * yard[1], (label, e_max, yard[0], e_rms, yard[1])
        ratios = (e_max / yard[0], e_rms / yard[1])
    if report is not None:
        report.append((label,) + ratios)
    return ratios


GRAD_NAMES = ("dS", "dstate", "db", "dgain", "dbias", "dpower")


def grad_reference(key, S, G, b, gain, bias, power, eps, state=None):
    """({name: float64 closed form}, {name: (max, rms) of the float32 yardstick}): the yardstick is the autograd of
    ``engine.pcen_composition`` in float32 on the CPU.  Once per ``key``, shared."""
    hit = _cache.get(("grad",) + tuple(key))
    if hit is None:
        import torch

        from nnaudio_amd import engine

        want = gradients(S, G, b, gain, bias, power, eps, state)
        leaves = [torch.from_numpy(np.array(v, dtype=np.float32)).requires_grad_(True) for v in (S, b, gain, bias, power)]
        st = None if state is None else torch.from_numpy(np.array(state, dtype=np.float32)).requires_grad_(True)
        out, _ = engine.pcen_composition(leaves[0], *leaves[1:], float(np.float32(eps)), st, dtype=torch.float32)
        out.backward(torch.from_numpy(np.asarray(G, dtype=np.float32)))
        got = dict(zip(("dS", "db", "dgain", "dbias", "dpower"), (v.grad.numpy() for v in leaves)))
        got["dstate"] = None if st is None else st.grad.numpy()
        yard = {k: errors(got[k], want[k]) for k in GRAD_NAMES if want[k] is not None}
        hit = (want, yard)
        _cache[("grad",) + tuple(key)] = hit
    return hit
