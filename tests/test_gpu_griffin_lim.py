"""Griffin_Lim on the MI355X: both routes of the forward transform against the float64 statement of the algorithm
(tests/_griffin_lim_oracle.py), the fused launch bit for bit against "Complex STFT + update kernel", the shapes that
fall back, convergence, and a bench-sized run."""
import ctypes

import numpy as np
import pytest
import torch

from tests import _griffin_lim_oracle as gl

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture
def fft_route():
    """tests/conftest.py switches the FFT route off for this module: the fused kernel lives there"""
    from nnaudio_amd import engine

    old = engine.set_fft(True)
    old_gl = engine.set_griffin_lim_fused(True)
    yield
    engine.set_fft(old)
    engine.set_griffin_lim_fused(old_gl)


def _magnitude(n_fft, hop, B, L, seed, win_length=None, center=True, pad_mode="reflect"):
    x = gl.chirp(B, L, seed=seed)
    return np.abs(gl.stft(x, n_fft, hop, gl.window(n_fft, win_length), center, pad_mode)).astype(np.float32)


def _run(S, seed, **kw):
    from nnaudio_amd import features

    m = features.Griffin_Lim(**kw)
    torch.manual_seed(seed)
    with torch.no_grad():
        return m(torch.from_numpy(S).to(DEV))


def _oracle(S, seed, **kw):
    torch.manual_seed(seed)
    r = torch.randn(S.shape, device=DEV).cpu().numpy()  # (the module's draw: same generator, same device)
    n_fft = kw["n_fft"]
    return gl.griffin_lim(S, r, kw.get("n_iter", 32), n_fft, kw.get("hop_length"), kw.get("win_length"),
                          kw.get("center", True), kw.get("pad_mode", "reflect"), kw.get("momentum", 0.99))


def _check(y, want, n_fft, center=True, tol=1e-5):
    y = y.cpu().numpy()
    assert y.dtype == np.float32 and y.shape == want.shape
    if not center:  # (untrimmed ends: the division by a vanishing window sum amplifies either side's rounding)
        y, want = y[:, n_fft // 2:-(n_fft // 2)], want[:, n_fft // 2:-(n_fft // 2)]
    err = gl.rel_l2(y, want)
    assert err <= tol, err


CASES = {
    "512": dict(n_fft=512),
    "1024": dict(n_fft=1024),
    "2048": dict(n_fft=2048),
    "1024-half-hop": dict(n_fft=1024, hop_length=512),
    "512-constant": dict(n_fft=512, pad_mode="constant"),
    "1024-short-window": dict(n_fft=1024, win_length=800),
    "512-no-momentum": dict(n_fft=512, momentum=0.0),
    "1024-uncentred": dict(n_fft=1024, center=False),
}


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("n_iter", [0, 1, 2])
@pytest.mark.parametrize("case", list(CASES))
def test_fft_route_matches_float64(fft_route, case, n_iter, fused):
    from nnaudio_amd import engine

    kw = dict(CASES[case], n_iter=n_iter)
    n_fft = kw["n_fft"]
    hop = kw.get("hop_length", n_fft // 4)
    B = 3 if n_iter == 1 else 1
    S = _magnitude(n_fft, hop, B, 12000, seed=n_fft + n_iter, win_length=kw.get("win_length"),
                   center=kw.get("center", True), pad_mode=kw.get("pad_mode", "reflect"))
    engine.set_griffin_lim_fused(fused)
    y = _run(S, 7, **kw)
    assert engine.griffin_lim_route() == (None if n_iter == 0 else "fft-fused" if fused else "separate")
    _check(y, _oracle(S, 7, **kw), n_fft, kw.get("center", True))


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "separate"])
@pytest.mark.parametrize("n_frames", [3, 5])
def test_short_clips(fft_route, fused, n_frames):
    """3 - 5 frames: the reflect-padded edge frames are most of the clip, and the fp32 / fp64 difference observed on the
    MI355X was 3.9e-5 (5 frames, either route: they are bit-identical) -- the update divides by |R - beta tprev|, which
    the momentum makes small for some bins; hence 1e-4 here instead of 1e-5"""
    from nnaudio_amd import engine

    kw = dict(n_fft=512, hop_length=256, n_iter=2)  # (3 frames of hop 128 rebuild 256 samples: too few to reflect-pad by 256)
    S = _magnitude(512, 256, 2, 256 * (n_frames - 1), seed=n_frames)
    assert S.shape[2] == n_frames
    engine.set_griffin_lim_fused(fused)
    y = _run(S, 3, **kw)
    assert engine.griffin_lim_route() == ("fft-fused" if fused else "separate")
    _check(y, _oracle(S, 3, **kw), 512, tol=1e-4)


@pytest.mark.parametrize("kw", [dict(n_fft=256), dict(n_fft=4096), dict(n_fft=1024, hop_length=300)],
                         ids=["n_fft-256", "n_fft-4096", "hop-300"])
def test_fallback_shapes_match_float64(fft_route, kw):
    """n_fft 256 / 4096: the fused launch refuses them (separate route); hop 300: fused forward transform, the
    inverse in two launches (the fused inverse wants a hop that is a multiple of 64 dividing n_fft)"""
    from nnaudio_amd import engine

    kw = dict(kw, n_iter=2)
    n_fft = kw["n_fft"]
    hop = kw.get("hop_length", n_fft // 4)
    S = _magnitude(n_fft, hop, 2, 16000, seed=n_fft)
    y = _run(S, 1, **kw)
    assert engine.griffin_lim_route() == ("fft-fused" if n_fft == 1024 else "separate")
    _check(y, _oracle(S, 1, **kw), n_fft)


@pytest.mark.parametrize("n_iter", [1, 2])
def test_contraction_route_matches_float64(both_stft_routes, n_iter):
    """the STFT family's two routes (tests/conftest.py): on the contraction kernels the forward transform runs in the
    module's default arithmetic (f16x3) and the update in its own kernel"""
    from nnaudio_amd import engine

    kw = dict(n_fft=1024, n_iter=n_iter)
    S = _magnitude(1024, 256, 2, 16000, seed=n_iter)
    y = _run(S, 2, **kw)
    assert engine.griffin_lim_route() == ("fft-fused" if both_stft_routes else "separate")
    _check(y, _oracle(S, 2, **kw), 1024)


def _operands(n_fft, hop):
    from nnaudio_amd import engine, features

    m = features.Griffin_Lim(n_fft, hop_length=hop)
    precision = engine.resolve_precision(None, "f16x3")
    return m._operands(torch.device(DEV), precision) + (precision,)


@pytest.mark.parametrize("n_fft,T", [(512, 37), (1024, 40), (2048, 21)])
def test_fused_launch_is_bit_identical_to_stft_plus_update(fft_route, n_fft, T):
    from nnaudio_amd import _abi, engine

    hop = n_fft // 4
    window, basis_re, basis_im, _, _, prep, precision = _operands(n_fft, hop)
    assert prep.get("basis_fold2") is not None
    g = torch.Generator(device=DEV).manual_seed(n_fft)
    B, F, L = 3, n_fft // 2 + 1, hop * (T - 1)
    y = torch.randn(B, L, device=DEV, generator=g)
    mag = torch.rand(B, F, T, device=DEV, generator=g)
    tprev0 = torch.randn(B, F, T, 2, device=DEV, generator=g)
    kw = dict(hop=hop, pad=n_fft // 2, pad_mode=engine.PAD_REFLECT, epilogue=engine.EPI_COMPLEX, im_sign=-1.0,
              precision=precision, **prep)
    R = engine.framed_gemm(y, basis_re, basis_im, **kw)  # the Complex-epilogue FFT launch
    assert R.shape == (B, F, T, 2)
    tprev = tprev0.clone()
    nxt = torch.full_like(tprev, float("nan"))
    a, _, _, keep = engine._framed_args(y, basis_re, basis_im, out=tprev, **kw)
    lib = _abi.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _abi.check(lib.mispec_griffin_lim_fft_f32(ctypes.byref(a), mag.data_ptr(), nxt.data_ptr(), 0.4, stream))
    torch.cuda.synchronize()
    assert torch.equal(tprev, R)
    tp2, nxt2 = tprev0.clone(), torch.empty_like(tprev0)
    engine.griffin_lim_update(R, tp2, mag, nxt2, 0.4)
    assert torch.equal(tp2, R)
    assert torch.equal(nxt, nxt2)
    # ... and the update rule itself, in float64
    a64 = torch.view_as_complex(R.double()) - 0.4 * torch.view_as_complex(tprev0.double())
    want = torch.view_as_real(mag.double() * a64 / (a64.abs() + 1e-16))
    assert float((nxt.double() - want).abs().max()) <= 1e-6 * float(mag.max())
    del keep


@pytest.mark.parametrize("n_fft", [512, 2048])
def test_module_output_same_bits_on_both_routes(fft_route, n_fft):
    from nnaudio_amd import engine

    S = _magnitude(n_fft, n_fft // 4, 2, 30000, seed=5)
    outs = []
    for fused in (True, False):
        engine.set_griffin_lim_fused(fused)
        outs.append(_run(S, 9, n_fft=n_fft, n_iter=4))
        assert engine.griffin_lim_route() == ("fft-fused" if fused else "separate")
    assert torch.equal(outs[0], outs[1])


def test_fused_launch_refusals(fft_route):
    from nnaudio_amd import _abi, engine

    lib = _abi.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n_fft, drop in ((4096, 0), (1024, 1)):
        hop = n_fft // 4
        _, basis_re, basis_im, _, _, _, precision = _operands(n_fft, hop)
        F = n_fft // 2 + 1 - drop
        br, bi = basis_re[:F].contiguous(), basis_im[:F].contiguous()
        prep = engine.prepare_basis(br, bi, precision, hop=hop)
        assert prep.get("basis_fold2") is not None
        y = torch.zeros(1, hop * 9, device=DEV)
        tprev = torch.zeros(1, F, 10, 2, device=DEV)
        a, _, _, keep = engine._framed_args(y, br, bi, out=tprev, hop=hop, pad=n_fft // 2, pad_mode=engine.PAD_REFLECT,
                                            epilogue=engine.EPI_COMPLEX, im_sign=-1.0, precision=precision, **prep)
        mag = torch.zeros(1, F, 10, device=DEV)
        nxt = torch.zeros_like(tprev)
        assert lib.mispec_griffin_lim_fft_f32(ctypes.byref(a), mag.data_ptr(), nxt.data_ptr(), 0.5, stream) == _abi.E_UNSUPPORTED
        assert lib.mispec_griffin_lim_fft_f32(ctypes.byref(a), None, nxt.data_ptr(), 0.5, stream) == _abi.E_INVALID
        del keep
    torch.cuda.synchronize()


def test_convergence_32_iterations(fft_route):
    """S of a real signal: 32 iterations reconstruct a spectrogram much closer to S than one does, and the spectral
    convergence matches the float64 run from the same initial phase"""
    from nnaudio_amd import engine

    n_fft, hop = 1024, 256
    S = _magnitude(n_fft, hop, 2, 48000, seed=21)
    sc = {}
    for n_iter in (1, 32):
        y = _run(S, 4, n_fft=n_fft, n_iter=n_iter)
        assert engine.griffin_lim_route() == "fft-fused"
        sc[n_iter] = gl.spectral_convergence(y.cpu().numpy(), S, n_fft, hop)
    want = gl.spectral_convergence(_oracle(S, 4, n_fft=n_fft, n_iter=32), S, n_fft, hop)
    assert sc[32] < sc[1]
    assert abs(sc[32] - want) <= 0.01 * want, (sc, want)


def test_bench_sized_run_is_finite_and_repeatable(fft_route):
    from nnaudio_amd import engine, features

    g = torch.Generator(device=DEV).manual_seed(0)
    S = torch.rand(64, 1025, 862, device=DEV, generator=g)
    m = features.Griffin_Lim(2048, n_iter=32, hop_length=512)
    outs = []
    with torch.no_grad():
        for _ in range(2):
            torch.manual_seed(1)
            outs.append(m(S))
            assert engine.griffin_lim_route() == "fft-fused"
    y = outs[0]
    assert y.dtype == torch.float32 and y.shape == (64, 440832)
    assert bool(torch.isfinite(y).all())
    assert torch.equal(outs[0], outs[1])
