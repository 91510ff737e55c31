"""MelSpectrogram.to_stft / inverse on the MI355X: the LDS-resident kernel (csrc/mel_nnls.hip) against the float64 NumPy
oracle under the rule of tests/_mel_nnls_oracle.py (4 x the oracle's own float32 error, max and RMS), with the
composition route on the same device printed beside it.  The shapes are the smallest at which the kernel can go wrong:
frame counts around the tile (TF = 16 frames up to n_fft 1024, 8 up to 2048, 4 above), banks with every register-slot count, uncovered bins,
empty rows.

The kernel keeps the iterate in float64 (csrc/mel_nnls.h says why: with a float32 iterate the first case here,
128/2048 T=1, measured 1.327e-06 max against the float32 oracle's 3.199e-07 on the MI355X -- 4.15 x, over the rule).  The
host model of the float64 kernel (tests/native/mel_nnls_harness.cpp, bit-identical to the kernel) gives at most 0.89 x
(max) and 0.79 x (RMS) over all inputs of this file."""
import numpy as np
import pytest
import torch

from tests import _mel_nnls_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

BANKS = dict(O.BANKS)
BANKS["128/4096"] = dict(sr=22050, n_fft=4096, n_mels=128)  # F = 2049: the 4-frame tiles
_modules = {}


def _module(name, power=2.0):
    """One module per (bank, power), shared by the tests (the n_fft = 2048 / 4096 STFT bases take a while to build)."""
    from nnaudio_amd import features

    key = (name, power)
    if key not in _modules:
        cfg = BANKS[name]
        _modules[key] = features.MelSpectrogram(hop_length=cfg["n_fft"] // 4, power=power, verbose=False, **cfg).to(DEV)
    return _modules[key]


def _tf(m):
    from nnaudio_amd import _abi

    return _abi.load().mispec_mel_nnls_tile_frames(m.mel_basis.shape[1])


def _mel(M, B, T, seed):
    rng = np.random.default_rng(seed)
    S = rng.random((B, M.shape[1], T)) ** 4
    return (M.astype(np.float64) @ S).astype(np.float32)


def _both(m, mel, **kw):
    """(kernel route, composition route) of one call, the kernel route asserted."""
    from nnaudio_amd import engine

    with torch.no_grad():
        got = m.to_stft(mel, **kw)
        assert engine.mel_nnls_route() == "kernel"
        old = engine.set_mel_nnls_kernel(False)
        try:
            comp = m.to_stft(mel, **kw)
            assert engine.mel_nnls_route() == "composition"
        finally:
            engine.set_mel_nnls_kernel(old)
    return got, comp


def _check(label, m, mel_np, mel_dev=None, **kw):
    M = m.mel_basis.cpu().numpy()
    mel_dev = torch.from_numpy(mel_np).to(DEV) if mel_dev is None else mel_dev
    got, comp = _both(m, mel_dev, **kw)
    want, yard = O.reference((label,), mel_np, M, power=float(m.power), **kw)
    c_max, c_rms = O.errors(comp.cpu().numpy(), want)
    O.check_rule(label, got, want, yard, extra="; composition max %.3e rms %.3e" % (c_max, c_rms))
    # the two routes agree under the same rule (the composition is held to it as well)
    O.check_rule(label + " (composition)", comp, want, yard)
    return got, want


@pytest.mark.parametrize("frames", ["1", "2", "TF-1", "TF", "TF+1", "2TF+3"])
@pytest.mark.parametrize("name", sorted(BANKS))
def test_banks_and_frame_counts(name, frames):
    m = _module(name)
    TF = _tf(m)
    assert TF == {4096: 4, 2048: 8}.get(BANKS[name]["n_fft"], 16)
    T = {"1": 1, "2": 2, "TF-1": TF - 1, "TF": TF, "TF+1": TF + 1, "2TF+3": 2 * TF + 3}[frames]
    M = m.mel_basis.cpu().numpy()
    got, _ = _check("%s T=%d" % (name, T), m, _mel(M, 3, T, seed=T), n_iter=8, momentum=True)
    assert tuple(got.shape) == (3, M.shape[1], T)
    uncovered = ~(M != 0).any(0)
    assert not got[:, torch.from_numpy(uncovered).to(DEV)].any()  # bins no filter covers: exactly 0
    if name == "40/1024-band":
        assert uncovered.sum() > 100


@pytest.mark.parametrize("power", [1.0, 2.0])
@pytest.mark.parametrize("momentum", [True, False])
@pytest.mark.parametrize("n_iter", [1, 64])
@pytest.mark.parametrize("name", sorted(BANKS))
def test_iterations_momentum_and_power(name, n_iter, momentum, power):
    m = _module(name, power)
    M = m.mel_basis.cpu().numpy()
    T = _tf(m) + 1
    _check("%s n_iter=%d momentum=%s power=%g" % (name, n_iter, momentum, power), m, _mel(M, 1, T, seed=n_iter),
           n_iter=n_iter, momentum=momentum)


def test_256_steps_and_zero_steps_on_the_smallest_bank():
    from nnaudio_amd import engine

    m = _module("16/256", 1.0)
    M = m.mel_basis.cpu().numpy()
    mel = _mel(M, 2, 19, seed=256)
    got, want = _check("16/256 n_iter=256", m, mel, n_iter=256, momentum=True)
    M64 = M.astype(np.float64)
    res = np.linalg.norm(M64 @ got.cpu().numpy().astype(np.float64) - mel) / np.linalg.norm(mel)
    res32 = np.linalg.norm(M64 @ O.nnls(mel, M, power=1.0, n_iter=256, momentum=True, dtype=np.float32) - mel) / np.linalg.norm(mel)
    print("16/256, 256 steps: || M p - m || / || m || kernel %.3e, float32 oracle %.3e" % (res, res32))
    assert res <= 4.0 * res32
    with torch.no_grad():
        zero = m.to_stft(torch.from_numpy(mel).to(DEV), n_iter=0)
    assert engine.mel_nnls_route() == "kernel" and tuple(zero.shape) == (2, 129, 19) and not zero.any()


def test_silent_clip_beside_a_loud_one_and_silent_columns():
    m = _module("128/2048")
    M = m.mel_basis.cpu().numpy()
    mel = _mel(M, 3, 21, seed=9) * 1e4
    mel[1] = 0.0               # a silent clip between two loud ones
    mel[0, :, 3] = 0.0         # silent columns inside a tile, and the tail tile's last column
    mel[2, :, 20] = 0.0
    got, _ = _check("silent beside loud", m, mel, n_iter=64, momentum=True)
    assert not got[1].any() and not got[0, :, 3].any() and not got[2, :, 20].any()
    assert float(got[0, :, 2].max()) > 0 and float(got[2, :, 19].max()) > 0
    all_zero = np.zeros((2, 128, 17), dtype=np.float32)
    got, _ = _check("all zero", m, all_zero, n_iter=8, momentum=True)
    assert not got.any()


def test_negative_mel_values_are_defined():
    """A column with negative mel values (no spectrogram has them; a model's output can): the iteration simply runs."""
    m = _module("80/512")
    M = m.mel_basis.cpu().numpy()
    mel = _mel(M, 2, 17, seed=10)
    mel[0, :, 5] = -mel[0, :, 5]
    mel[1, ::3, 16] *= -2.0
    got, _ = _check("negative columns", m, mel, n_iter=64, momentum=True)
    assert bool(torch.isfinite(got).all()) and float(got.min()) >= 0.0
    assert not got[0, :, 5].any()  # (all targets negative: the projection keeps p at 0)


def test_input_layouts():
    from nnaudio_amd import engine

    m = _module("80/512")
    M = m.mel_basis.cpu().numpy()
    mel_np = _mel(M, 3, 19, seed=11)
    mel = torch.from_numpy(mel_np).to(DEV)
    with torch.no_grad():
        want = m.to_stft(mel, n_iter=8)
        assert engine.mel_nnls_route() == "kernel"
        tr = mel.transpose(1, 2).contiguous().transpose(1, 2)   # a transposed view: frames are not of unit stride
        assert not tr.is_contiguous() and tr.stride(2) != 1
        assert torch.equal(m.to_stft(tr, n_iter=8), want) and engine.mel_nnls_route() == "kernel"
        wide = torch.full((3, 80 + 5, 19 + 7), 7.0, device=DEV)  # clip and row strides wider than the rows
        wide[:, :80, :19] = mel
        view = wide[:, :80, :19]
        assert view.stride() == (85 * 26, 26, 1)
        assert torch.equal(m.to_stft(view, n_iter=8), want) and engine.mel_nnls_route() == "kernel"
        assert torch.equal(m.to_stft(mel[1], n_iter=8)[0], want[1])          # 2-D input: a batch of one
        assert torch.equal(m.to_stft(mel.double(), n_iter=8), want)
        for b in range(3):                                                   # clips are computed on their own
            assert torch.equal(m.to_stft(mel[b:b + 1], n_iter=8)[0], want[b])


def test_guard_cells_around_the_output_stay_untouched():
    from nnaudio_amd import engine

    for name in ("16/256", "128/4096"):
        m = _module(name)
        TF = _tf(m)
        M = m.mel_basis.cpu().numpy()
        F, T = M.shape[1], TF + 3
        mel = torch.from_numpy(_mel(M, 2, T, seed=12)).to(DEV)
        with torch.no_grad():
            want = m.to_stft(mel, n_iter=8)
        big = torch.full((2, F + 2, T + 2 * TF), -7.0, device=DEV)
        out = big[:, 1:F + 1, 3:3 + T]
        with torch.no_grad():
            res = engine.mel_nnls(mel, m.mel_basis, power=m.power, n_iter=8, momentum=True, operands=m._nnls_operands, out=out)
        assert engine.mel_nnls_route() == "kernel" and res is out
        assert torch.equal(out, want)
        guard = torch.ones_like(big, dtype=torch.bool)
        guard[:, 1:F + 1, 3:3 + T] = False
        assert bool((big[guard] == -7.0).all())


def test_routes():
    from nnaudio_amd import engine, features

    for name in sorted(BANKS):
        m = _module(name)
        assert engine.mel_nnls_served(m.mel_basis, m.power), name
        with torch.no_grad():
            m.to_stft(torch.rand(1, m.mel_basis.shape[0], 3, device=DEV), n_iter=1)
        assert engine.mel_nnls_route() == "kernel", name
    # a dense random bank: the composition
    m = features.MelSpectrogram(sr=22050, n_fft=256, n_mels=16, hop_length=64, verbose=False).to(DEV)
    mel_np = _mel(m.mel_basis.cpu().numpy(), 2, 17, seed=13)
    mel = torch.from_numpy(mel_np).to(DEV)
    with torch.no_grad():
        kernel = m.to_stft(mel, n_iter=8)
        assert engine.mel_nnls_route() == "kernel"
        old = engine.set_mel_nnls_kernel(False)
        try:
            comp = m.to_stft(mel, n_iter=8)
            assert engine.mel_nnls_route() == "composition"
        finally:
            engine.set_mel_nnls_kernel(old)
        want, yard = O.reference(("routes",), mel_np, m.mel_basis.cpu().numpy(), power=2.0, n_iter=8, momentum=True)
        O.check_rule("routes: kernel", kernel, want, yard)
        O.check_rule("routes: composition", comp, want, yard)
        torch.manual_seed(0)
        m.mel_basis.copy_(torch.rand(16, 129, device=DEV))
        assert not engine.mel_nnls_served(m.mel_basis, 2.0)
        dense = m.to_stft(mel, n_iter=8)
        assert engine.mel_nnls_route() == "composition"
        Md = m.mel_basis.cpu().numpy()
        want, yard = O.reference(("routes dense",), mel_np, Md, power=2.0, n_iter=8, momentum=True)
        O.check_rule("routes: dense bank", dense, want, yard)
    # a trained bank: after one optimizer step every weight has moved, the bank is dense
    t = features.MelSpectrogram(sr=22050, n_fft=256, n_mels=16, hop_length=64, trainable_mel=True, verbose=False).to(DEV)
    with torch.no_grad():
        t.to_stft(mel, n_iter=2)
    assert engine.mel_nnls_route() == "kernel"
    opt = torch.optim.SGD([t.mel_basis], lr=1e-3)
    t(torch.randn(2, 4000, device=DEV)).sum().backward()
    opt.step()
    with torch.no_grad():
        out = t.to_stft(mel, n_iter=2)
    assert engine.mel_nnls_route() == "composition" and bool(torch.isfinite(out).all())
    assert sorted(t.state_dict()) == sorted(m.state_dict())


@pytest.mark.parametrize("shape,cfg", [((2, 128, 40), dict(sr=22050, n_fft=2048, n_mels=128, hop_length=512)),
                                       ((1, 16, 9), dict(sr=22050, n_fft=256, n_mels=16, hop_length=64))])
def test_inverse(both_stft_routes, shape, cfg):
    from nnaudio_amd import engine, features

    name = "128/2048" if cfg["n_fft"] == 2048 else "16/256"
    m = _module(name)
    assert m.stride == cfg["hop_length"]
    mel = torch.from_numpy(_mel(m.mel_basis.cpu().numpy(), shape[0], shape[2], seed=14)).to(DEV)
    with torch.no_grad():
        torch.manual_seed(21)
        y = m.inverse(mel, n_iter=16, griffin_lim_iter=4)
        route = engine.griffin_lim_route()
        assert engine.mel_nnls_route() == "kernel"
        gl = features.Griffin_Lim(cfg["n_fft"], n_iter=4, hop_length=cfg["hop_length"], win_length=cfg["n_fft"])
        S = m.to_stft(mel, n_iter=16)
        torch.manual_seed(21)
        two_step = gl(S)
        assert engine.griffin_lim_route() == route and route is not None
    assert tuple(y.shape) == (shape[0], cfg["hop_length"] * (shape[2] - 1)) and y.dtype == torch.float32
    assert y.is_cuda and bool(torch.isfinite(y).all()) and float(y.abs().max()) > 0
    assert torch.equal(y, two_step)
