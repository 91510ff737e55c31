"""Griffin_Lim without a GPU: the public surface, and the host path (libmispec's host loops for both transforms and
the update) against the float64 statement of the algorithm in tests/_griffin_lim_oracle.py."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

from tests import _griffin_lim_oracle as gl


@pytest.fixture(scope="module", autouse=True)
def _built():
    from nnaudio_amd import build

    build.build(verbose=False)


def test_signature_defaults_and_attributes():
    from nnaudio_amd import features

    sig = inspect.signature(features.Griffin_Lim.__init__)
    want = [("n_fft", inspect.Parameter.empty), ("n_iter", 32), ("hop_length", None), ("win_length", None),
            ("window", "hann"), ("center", True), ("pad_mode", "reflect"), ("momentum", 0.99), ("device", "cpu")]
    got = [(n, p.default) for n, p in sig.parameters.items() if n != "self"]
    assert got == want
    assert "Griffin_Lim" in features.__all__
    m = features.Griffin_Lim(512)
    assert (m.n_fft, m.n_iter, m.hop_length, m.win_length, m.center, m.pad_mode, m.momentum, m.device) == (
        512, 32, 128, 512, True, "reflect", 0.99, "cpu")
    assert m.w.dtype == torch.float32 and m.w.shape == (512,)
    from scipy.signal import get_window

    assert torch.equal(m.w, torch.tensor(get_window("hann", 512, fftbins=True)).float())
    m = features.Griffin_Lim(1024, n_iter=4, hop_length=300, win_length=800, window="hamming", center=False,
                             pad_mode="constant", momentum=0.5)
    assert (m.n_fft, m.n_iter, m.hop_length, m.win_length, m.center, m.pad_mode, m.momentum) == (
        1024, 4, 300, 800, False, "constant", 0.5)
    assert m.w.shape == (800,)
    assert m.precision is None


def test_state_dict_is_empty_before_and_after_a_call():
    from nnaudio_amd import features

    m = features.Griffin_Lim(256, n_iter=1)
    assert len(m.state_dict()) == 0
    m(torch.rand(1, 129, 6))
    assert len(m.state_dict()) == 0 and list(m.buffers()) == [] and list(m.children()) == []


def test_input_checks():
    from nnaudio_amd import features

    m = features.Griffin_Lim(256, n_iter=1)
    with pytest.raises(AssertionError, match="batch, freq_bins, timesteps"):
        m(torch.rand(129, 6))
    with pytest.raises(RuntimeError, match="129 frequency bins"):
        m(torch.rand(1, 128, 6))
    S = torch.rand(1, 129, 6, requires_grad=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        m(S)
    with torch.no_grad():
        assert m(S).shape == (1, 64 * 5)
    with pytest.raises(AssertionError, match="reflect padding"):  # (2 frames centred: 64 samples < n_fft // 2)
        m(torch.rand(1, 129, 2))
    with pytest.raises(ValueError, match="pad_mode"):
        features.Griffin_Lim(256, n_iter=1, pad_mode="circular")(torch.rand(1, 129, 6))


@pytest.mark.parametrize("center", [True, False])
def test_output_shape_and_dtype(center):
    from nnaudio_amd import features

    m = features.Griffin_Lim(256, n_iter=2, hop_length=64, center=center)
    y = m(torch.rand(2, 129, 9, dtype=torch.float64))
    assert y.dtype == torch.float32 and y.device.type == "cpu"
    assert y.shape == ((2, 64 * 8) if center else (2, 256 + 64 * 8))


def test_host_update_entry():
    """mispec_griffin_lim_update_host_f32 = the update rule in float32, and its argument checks"""
    from nnaudio_amd import _abi, engine

    g = torch.Generator().manual_seed(1)
    R, tp = torch.randn(3, 5, 2, generator=g), torch.randn(3, 5, 2, generator=g)
    mag = torch.rand(3, 5, generator=g)
    nxt = torch.empty(3, 5, 2)
    tp0 = tp.clone()
    engine.griffin_lim_update(R, tp, mag, nxt, 0.4)
    a = torch.view_as_complex(R.double()) - 0.4 * torch.view_as_complex(tp0.double())
    want = torch.view_as_real(mag.double() * a / (a.abs() + 1e-16))
    assert torch.equal(tp, R)
    assert float((nxt.double() - want).abs().max()) <= 1e-6
    lib = _abi.load()
    assert lib.mispec_griffin_lim_update_host_f32(None, None, None, None, 4, 0.5) == _abi.E_INVALID
    assert lib.mispec_griffin_lim_update_host_f32(R.data_ptr(), tp.data_ptr(), mag.data_ptr(), nxt.data_ptr(), 0,
                                                  0.5) == _abi.E_INVALID


def test_device_entries_refuse_bad_arguments_before_any_device_work():
    from nnaudio_amd import _abi

    lib = _abi.load()
    assert lib.mispec_griffin_lim_update_f32(None, None, None, None, 8, 0.5, None) == _abi.E_INVALID
    assert lib.mispec_griffin_lim_update_f32(4096, 8192, 12288, 16384, 0, 0.5, None) == _abi.E_INVALID
    assert lib.mispec_griffin_lim_update_f32(4096, 8192, 12288, 16384, -3, 0.5, None) == _abi.E_INVALID
    assert lib.mispec_griffin_lim_fft_f32(None, 4096, 8192, 0.5, None) == _abi.E_INVALID
    a = _abi.FramedGemmArgs()
    a.struct_size = ctypes.sizeof(_abi.FramedGemmArgs)
    assert lib.mispec_griffin_lim_fft_f32(ctypes.byref(a), None, 8192, 0.5, None) == _abi.E_INVALID
    assert lib.mispec_griffin_lim_fft_f32(ctypes.byref(a), 4096, 8192, 0.5, None) == _abi.E_INVALID  # (NULL x / basis / out)
    a.x = a.basis_re = a.basis_im = a.out = 4096
    a.n_clips, a.n_samples, a.n_frames, a.n_bins, a.kernel, a.hop = 1, 0, 5, 257, 512, 128
    assert lib.mispec_griffin_lim_fft_f32(ctypes.byref(a), 4096, 8192, 0.5, None) == _abi.E_INVALID
    assert b"non-positive" in lib.mispec_last_error()
    # well-formed but without the FFT route's operands (basis_fold2): refused, the caller falls back
    a.n_samples, a.pad, a.pad_mode, a.epilogue, a.im_sign = 1024, 256, 2, 0, -1.0
    a.n_frames = 9
    assert lib.mispec_griffin_lim_fft_f32(ctypes.byref(a), 4096, 8192, 0.5, None) == _abi.E_UNSUPPORTED


def _case(n_fft, hop, B, L, seed):
    x = gl.chirp(B, L, seed=seed)
    w = gl.window(n_fft)
    return np.abs(gl.stft(x, n_fft, hop, w)).astype(np.float32)


@pytest.mark.parametrize("n_iter", [0, 1, 2])
@pytest.mark.parametrize("kw", [
    dict(n_fft=256),
    dict(n_fft=512, hop_length=256),
    dict(n_fft=256, pad_mode="constant"),
    dict(n_fft=256, win_length=200),
    dict(n_fft=256, momentum=0.0),
    dict(n_fft=256, center=False),
], ids=["default", "half-hop", "constant", "short-window", "no-momentum", "uncentred"])
def test_host_path_matches_float64(kw, n_iter):
    from nnaudio_amd import engine, features

    n_fft = kw["n_fft"]
    hop = kw.get("hop_length", n_fft // 4)
    B = 3 if n_iter == 1 else 1
    S = _case(n_fft, hop, B, 4000, seed=n_fft + n_iter)
    m = features.Griffin_Lim(n_iter=n_iter, **kw)
    torch.manual_seed(11)
    r = torch.randn(S.shape)
    want = gl.griffin_lim(S, r.numpy(), n_iter, n_fft, hop, kw.get("win_length"), kw.get("center", True),
                          kw.get("pad_mode", "reflect"), kw.get("momentum", 0.99))
    torch.manual_seed(11)
    y = m(torch.from_numpy(S))
    assert engine.griffin_lim_route() == ("host" if n_iter else None)
    assert y.shape == want.shape
    y = y.numpy()
    if not kw.get("center", True):  # (untrimmed ends: the division by a vanishing window sum amplifies rounding)
        y, want = y[:, n_fft // 2:-(n_fft // 2)], want[:, n_fft // 2:-(n_fft // 2)]
    assert gl.rel_l2(y, want) <= 1e-5


def test_host_path_short_clip():
    """a clip of 4 frames"""
    from nnaudio_amd import features

    S = np.abs(gl.stft(gl.chirp(1, 384, seed=3), 256, 128, gl.window(256))).astype(np.float32)
    assert S.shape[2] == 4
    torch.manual_seed(5)
    want = gl.griffin_lim(S, torch.randn(S.shape).numpy(), 2, 256, 128)
    torch.manual_seed(5)
    y = features.Griffin_Lim(256, n_iter=2, hop_length=128)(torch.from_numpy(S)).numpy()
    assert gl.rel_l2(y, want) <= 1e-5
