"""features.PCEN on the MI355X: the scan kernels (csrc/pcen.hip) and the composition route on the same device against the
float64 NumPy oracle under the rule of tests/_pcen_oracle.py (4 x the float32 yardstick's error, max and RMS; exact
where the yardstick is exact).  The shapes sit at the edges of the 64-frame chunk: one and two frames, 63 / 64 / 65,
128 / 129, several chunks with a ragged tail, more rows than a workgroup holds, 1025 channels.

The kernels scan and evaluate the two powers in float64 and round once at the store (csrc/pcen.h says why: the
float32 form of the same kernel met the rule on every many-element case and missed it at (1, 1, 2), where a yardstick of
two elements is now and then exact to a tenth of an ulp).  Largest ratios measured on the MI355X (ours / yardstick, max
and RMS): forward, kernel and composition, 1.00 / 1.00 at the one- and two-element shapes and 0.52 / 0.40 elsewhere;
gradients 1.00 / 1.00.  The host model of the kernels (tests/native/pcen_harness.cpp) gives 1.00 / 1.00 over the same
inputs."""
import numpy as np
import pytest
import torch

from tests import _pcen_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _both(S, params, eps, state=None):
    """(kernel route, composition route) of one call on the device, the routes asserted."""
    from nnaudio_amd import engine

    with torch.no_grad():
        got, last = engine.pcen(S, *params, float(eps), state)
        assert engine.pcen_route() == "kernel"
        old = engine.set_pcen_kernel(False)
        try:
            comp, _ = engine.pcen(S, *params, float(eps), state)
            assert engine.pcen_route() == "composition"
        finally:
            engine.set_pcen_kernel(old)
    return got, last, comp


@pytest.mark.parametrize("shape", O.SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pi", range(len(O.PARAMS)))
def test_forward_meets_the_rule(shape, pi):
    report = []
    for name in O.INPUTS:
        S = O.make_input(name, shape)
        b, gain, bias, power, eps = O.params_f32(O.PARAMS[pi])
        want, M, yard = O.reference(("fwd", shape, pi, name, None), S, b, gain, bias, power, eps)
        (Sd,) = _t(S)
        got, last, comp = _both(Sd, _t(b, gain, bias, power), eps)
        assert tuple(got.shape) == shape and got.dtype == torch.float32 and got.is_contiguous()
        O.check_rule("kernel %s params %d %s" % (shape, pi, name), got, want, yard, report)
        O.check_rule("composition %s params %d %s" % (shape, pi, name), comp, want, yard, report)
        assert np.abs(last.cpu().numpy() - M[..., -1]).max() <= 1.2e-7 * np.abs(M[..., -1]).max()
        if name == "zeros":
            assert not got.any() and not comp.any()
    print("largest ratios: max %.2f rms %.2f" % (max(r[1] for r in report), max(r[2] for r in report)))


@pytest.mark.parametrize("shape", [(2, 3, 65), (2, 128, 130)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("pi", range(len(O.PARAMS)))
def test_per_channel_parameters(shape, pi):
    """A distinct value per channel: a row that read another channel's parameters is far outside the rule."""
    from nnaudio_amd import features

    for name in O.INPUTS:
        S = O.make_input(name, shape)
        b, gain, bias, power, eps = O.params_f32(O.PARAMS[pi], shape[1])
        want, _, yard = O.reference(("fwd", shape, pi, name, shape[1]), S, b, gain, bias, power, eps)
        got, _, comp = _both(_t(S)[0], _t(b, gain, bias, power), eps)
        O.check_rule("kernel per-channel %s params %d %s" % (shape, pi, name), got, want, yard)
        O.check_rule("composition per-channel %s params %d %s" % (shape, pi, name), comp, want, yard)
    m = features.PCEN(n_bins=shape[1], eps=float(eps)).to(DEV)
    with torch.no_grad():
        for p, v in zip((m.b, m.gain, m.bias, m.power), (b, gain, bias, power)):
            p.copy_(torch.from_numpy(v))
        assert torch.equal(m(_t(S)[0]), got)  # (the module is the same call)


def test_two_dimensional_and_strided_inputs():
    from nnaudio_amd import engine, features

    pi, shape = 0, (2, 3, 65)
    b, gain, bias, power, eps = O.params_f32(O.PARAMS[pi])
    m = features.PCEN(b=float(b[0]), gain=float(gain[0]), bias=float(bias[0]), power=float(power[0]), eps=float(eps)).to(DEV)
    S = O.make_input("randn2", shape)
    want, _, yard = O.reference(("fwd", shape, pi, "randn2", None), S, b, gain, bias, power, eps)
    (Sd,) = _t(S)
    with torch.no_grad():
        whole = m(Sd)
        one = m(Sd[1])  # (F, T)
        assert engine.pcen_route() == "kernel" and tuple(one.shape) == shape[1:] and torch.equal(one, whole[1])
        # a row-sliced view: clip and row strides pass through
        big = torch.full((2, 7, 65), 7.0, device=DEV)
        big[:, 2:5, :] = Sd
        view = big[:, 2:5, :]
        assert not view.is_contiguous()
        O.check_rule("row-sliced view", m(view), want, yard)
        assert torch.equal(m(view), whole) and float(big[:, :2].min()) == 7.0 and float(big[:, 5:].max()) == 7.0
        # a frame-strided view is made contiguous
        wide = torch.zeros((2, 3, 130), device=DEV)
        wide[..., ::2] = Sd
        assert torch.equal(m(wide[..., ::2]), whole)
        assert torch.equal(m(Sd.transpose(1, 2).contiguous().transpose(1, 2)), whole)


@pytest.mark.parametrize("splits", [(1,), (64,), (100,), (1, 64, 100)])
def test_chunked_use_through_state(splits):
    from nnaudio_amd import features

    shape, pi = (3, 17, 203), 0
    S = O.make_input("randn2", shape)
    b, gain, bias, power, eps = O.params_f32(O.PARAMS[pi])
    m = features.PCEN(b=float(b[0]), gain=float(gain[0]), bias=float(bias[0]), power=float(power[0]), eps=float(eps)).to(DEV)
    want, M, yard = O.reference(("fwd", shape, pi, "randn2", None), S, b, gain, bias, power, eps)
    (Sd,) = _t(S)
    edges = (0,) + tuple(splits) + (shape[2],)
    state, parts = None, []
    with torch.no_grad():
        for lo, hi in zip(edges[:-1], edges[1:]):
            out, state = m(Sd[..., lo:hi], state=state, return_state=True)
            assert tuple(state.shape) == shape[:2] and not state.requires_grad
            parts.append(out)
    O.check_rule("chunks %s" % (splits,), torch.cat(parts, dim=-1), want, yard)
    assert np.abs(state.cpu().numpy() - M[..., -1]).max() <= 2e-7 * np.abs(M[..., -1]).max()


def test_given_state():
    shape, pi = (3, 17, 203), 3
    S = O.make_input("bursts", shape)
    b, gain, bias, power, eps = O.params_f32(O.PARAMS[pi], shape[1])
    st = (np.random.default_rng(2).random(shape[:2]) * 3).astype(np.float32)
    want, _, yard = O.reference(("fwd-state", shape, pi, "bursts"), S, b, gain, bias, power, eps, st)
    got, _, comp = _both(_t(S)[0], _t(b, gain, bias, power), eps, _t(st)[0])
    O.check_rule("kernel, given state", got, want, yard)
    O.check_rule("composition, given state", comp, want, yard)


@pytest.mark.parametrize("shape", O.GRAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("per_channel", [False, True], ids=["scalar", "per-channel"])
@pytest.mark.parametrize("with_state", [False, True], ids=["first-frame", "state"])
def test_gradients_meet_the_rule(shape, per_channel, with_state):
    """dS, dstate and the four parameter gradients of sum(G * out) against the float64 closed form; the yardstick is the
    float32 composition's autograd on the CPU."""
    from nnaudio_amd import engine

    rng = np.random.default_rng(3)
    G = rng.standard_normal(shape).astype(np.float32)
    st = (rng.random(shape[:2]) * 2).astype(np.float32) if with_state else None
    report = []
    for pi, pset in enumerate(O.PARAMS):
        for name in O.INPUTS:
            S = O.make_input(name, shape)
            n = shape[1] if per_channel else None
            b, gain, bias, power, eps = O.params_f32(pset, n)
            want, yard = O.grad_reference(("gpu", shape, pi, name, n, with_state), S, G, b, gain, bias, power, eps, st)
            leaves = [t.requires_grad_(True) for t in _t(S, b, gain, bias, power)]
            state = None if st is None else _t(st)[0].requires_grad_(True)
            out, last = engine.pcen(leaves[0], *leaves[1:], float(eps), state)
            assert engine.pcen_route() == "kernel" and out.requires_grad and not last.requires_grad
            out.backward(_t(G)[0])
            got = dict(zip(("dS", "db", "dgain", "dbias", "dpower"), (v.grad for v in leaves)))
            got["dstate"] = None if state is None else state.grad
            for k in O.GRAD_NAMES:
                if want[k] is None:
                    assert got[k] is None
                    continue
                O.check_rule("%s params %d %s %s" % (shape, pi, name, k), got[k], want[k], yard[k], report)
    print("largest ratios: max %.2f rms %.2f" % (max(r[1] for r in report), max(r[2] for r in report)))


def test_partial_gradients_and_determinism():
    """Only what requires grad gets one; two backward runs give the same bits (no atomics)."""
    from nnaudio_amd import features

    m = features.PCEN(n_bins=17, trainable=True).to(DEV)
    (S,) = _t(O.make_input("randn2", (3, 17, 203)))
    (G,) = _t(np.random.default_rng(4).standard_normal((3, 17, 203)).astype(np.float32))
    runs = []
    for _ in range(2):
        m.zero_grad()
        m(S).backward(G)
        runs.append([p.grad.clone() for p in m.parameters()])
    assert S.grad is None and all(torch.equal(a, b) for a, b in zip(*runs))
    frozen = features.PCEN(n_bins=17).to(DEV)
    x = S.clone().requires_grad_(True)
    frozen(x).backward(G)
    assert x.grad is not None and bool(torch.isfinite(x.grad).all())


def test_one_optimizer_step_changes_all_parameters():
    from nnaudio_amd import engine, features

    m = features.PCEN(n_bins=16, trainable=True).to(DEV)
    before = {k: v.detach().clone() for k, v in m.named_parameters()}
    opt = torch.optim.SGD(m.parameters(), lr=1e-2)
    (S,) = _t(O.make_input("randn2", (2, 16, 130)))
    loss = (m(S) ** 2).mean()
    assert engine.pcen_route() == "kernel"
    loss.backward()
    opt.step()
    assert sorted(before) == ["b", "bias", "gain", "power"]
    for k, v in m.named_parameters():
        assert bool(torch.isfinite(v).all()) and bool((v != before[k]).any()), k


def test_route_follows_the_switch():
    from nnaudio_amd import engine, features

    m = features.PCEN().to(DEV)
    (S,) = _t(O.make_input("randn2", (2, 3, 65)))
    with torch.no_grad():
        m(S)
        assert engine.pcen_route() == "kernel"
        old = engine.set_pcen_kernel(False)
        try:
            m(S)
            assert engine.pcen_route() == "composition"
        finally:
            engine.set_pcen_kernel(old)
        m(S)
        assert engine.pcen_route() == "kernel"


def test_side_stream():
    from nnaudio_amd import features

    m = features.PCEN().to(DEV)
    (S,) = _t(O.make_input("randn2", (3, 17, 203)))
    with torch.no_grad():
        want = m(S)
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(side):
            got = m(S)
        side.synchronize()
    assert torch.equal(got, want)


def test_mel_spectrogram_into_pcen():
    from nnaudio_amd import features

    mel = features.MelSpectrogram(sr=22050, n_fft=256, n_mels=16, hop_length=64, verbose=False).to(DEV)
    m = features.PCEN(n_bins=16).to(DEV)
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 4000)).astype(np.float32)).to(DEV)
    with torch.no_grad():
        spec = mel(x)
        got = m(spec)
    S = spec.cpu().numpy()
    params = [p.cpu().numpy() for p in (m.b, m.gain, m.bias, m.power)]
    want, _, yard = O.reference(("mel",), S, *params, m.eps)
    assert tuple(got.shape) == tuple(spec.shape) and spec.shape[1] == 16
    O.check_rule("MelSpectrogram -> PCEN", got, want, yard)
