"""features.PCEN without a GPU: the oracle (tests/_pcen_oracle.py) against scipy's lfilter (librosa's definition) and its
closed-form gradients against float64 autograd, the module's surface, the host route and the composition under the
suite's rule, chunked use through ``state``, the host harness of csrc/pcen.h (the 64-lane model of both kernels; once
more under AddressSanitizer / UBSan as a stand-alone program) and the library's argument checks.

Largest ratios measured (ours / yardstick, max / RMS; the rule allows 4): host route and composition 1.00 / 1.00,
harness forward 1.00 / 1.00, harness gradients 1.00 / 1.00."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import _pcen_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_SHAPES = [(1, 1, 1), (1, 1, 2), (2, 3, 65), (3, 17, 203)]


def _t(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)) for a in arrays]


def _clang():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("amdclang++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_oracle_smoother_is_librosas_lfilter():
    """M = scipy.signal.lfilter([b], [1, b - 1], S, zi = lfilter_zi([b], [1, b - 1]) * S[..., :1]) to float64 rounding."""
    from scipy.signal import lfilter, lfilter_zi

    for pset in O.PARAMS:
        b = np.float64(np.float32(pset[0]))
        for name in O.INPUTS:
            S = O.make_input(name, (2, 3, 203)).astype(np.float64)
            zi = lfilter_zi([b], [1, b - 1])
            want, _ = lfilter([b], [1, b - 1], S, zi=zi * S[..., :1], axis=-1)
            got = O.smooth(S, np.float32(pset[0]))
            scale = np.abs(want).max()
            assert np.abs(got - want).max() <= 1e-13 * scale, (pset, name)


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("with_state", [False, True])
def test_closed_form_gradients_equal_float64_autograd(per_channel, with_state):
    from nnaudio_amd import engine

    shape = (2, 3, 65)
    rng = np.random.default_rng(1)
    for pset in O.PARAMS:
        for name in ("randn2", "bursts", "ramp"):
            S = O.make_input(name, shape).astype(np.float64) + 1e-3  # (away from S = 0, where d/dS of P is huge)
            G = rng.standard_normal(shape)
            state = rng.random(shape[:2]) + 0.1 if with_state else None
            b, gain, bias, power, eps = O.params_f32(pset, shape[1] if per_channel else None)
            want = O.gradients(S, G, b, gain, bias, power, eps, state)
            leaves = [torch.from_numpy(np.array(v, dtype=np.float64)).requires_grad_(True) for v in (S, b, gain, bias, power)]
            st = None if state is None else torch.from_numpy(state).requires_grad_(True)
            out, _ = engine.pcen_composition(leaves[0], *leaves[1:], float(eps), st)
            assert out.dtype == torch.float64
            out.backward(torch.from_numpy(G))
            got = dict(zip(("dS", "db", "dgain", "dbias", "dpower"), (v.grad.numpy() for v in leaves)))
            got["dstate"] = None if st is None else st.grad.numpy()
            for k in O.GRAD_NAMES:
                if want[k] is None:
                    assert got[k] is None
                    continue
                scale = np.abs(want[k]).max()
                assert np.abs(got[k] - want[k]).max() <= 1e-10 * scale, (pset, name, k, np.abs(got[k] - want[k]).max(), scale)


def test_module_surface():
    from nnaudio_amd import features

    assert "PCEN" in features.__all__
    m = features.PCEN()
    sd = m.state_dict()
    assert sorted(sd) == ["b", "bias", "gain", "power"] and all(tuple(v.shape) == (1,) for v in sd.values())
    assert not list(m.parameters()) and len(list(m.buffers())) == 4
    t_frames = 0.4 * 22050 / 512.0
    assert abs(float(m.b) - (np.sqrt(1 + 4 * t_frames ** 2) - 1) / (2 * t_frames ** 2)) < 1e-8
    assert float(m.gain) == np.float32(0.98) and float(m.bias) == 2.0 and float(m.power) == 0.5
    m = features.PCEN(n_bins=40, b=0.1, gain=0.5, bias=3.0, power=0.25, trainable=True)
    sd = m.state_dict()
    assert sorted(sd) == ["b", "bias", "gain", "power"] and all(tuple(v.shape) == (40,) for v in sd.values())
    assert len(list(m.parameters())) == 4 and not list(m.buffers()) and all(p.requires_grad for p in m.parameters())
    assert bool((m.b == np.float32(0.1)).all()) and bool((m.power == 0.25).all())
    assert "gain=0.5" in repr(m) and "n_bins=40" in repr(m) and "trainable=True" in repr(m)
    assert features.PCEN(sr=16000, hop_length=160, time_constant=0.06).b.item() == pytest.approx((np.sqrt(145.0) - 1.0) / 72.0, abs=1e-7)  # Tf = 6 frames
    features.PCEN(b=1.0, bias=0.0, gain=0.0)  # (the closed ends of the ranges)
    for kw in (dict(eps=0.0), dict(eps=-1e-6), dict(b=0.0), dict(b=1.5), dict(b=-0.1), dict(power=0.0), dict(power=-1.0),
               dict(gain=-0.1), dict(bias=-1.0), dict(n_bins=0)):
        with pytest.raises(ValueError):
            features.PCEN(**kw)
    with pytest.raises(ValueError, match="channels"):
        features.PCEN(n_bins=4)(torch.zeros(1, 5, 3))
    with pytest.raises(ValueError, match="frames"):
        features.PCEN()(torch.zeros(7))
    with pytest.raises(ValueError, match="state"):
        features.PCEN()(torch.zeros(2, 5, 3), state=torch.zeros(2, 4))


@pytest.mark.parametrize("shape", CPU_SHAPES)
@pytest.mark.parametrize("pi", range(len(O.PARAMS)))
def test_host_route_and_composition_meet_the_rule(shape, pi):
    from nnaudio_amd import engine

    report = []
    for name in O.INPUTS:
        S = O.make_input(name, shape)
        for n in (None, shape[1]):
            b, gain, bias, power, eps = O.params_f32(O.PARAMS[pi], n)
            want, _, yard = O.reference(("fwd", shape, pi, name, n), S, b, gain, bias, power, eps)
            with torch.no_grad():
                got, last = engine.pcen(*_t(S, b, gain, bias, power), float(eps))
                assert engine.pcen_route() == "host"
                comp, _ = engine.pcen_composition(*_t(S, b, gain, bias, power), float(eps))
            label = "%s params %d %s %s" % (shape, pi, name, "per-channel" if n else "scalar")
            O.check_rule("host " + label, got, want, yard, report)
            O.check_rule("composition " + label, comp, want, yard, report)
            if name == "zeros":
                assert not got.numpy().any() and not comp.numpy().any()
    print("largest ratios: max %.2f rms %.2f" % (max(r[1] for r in report), max(r[2] for r in report)))


def test_routes():
    from nnaudio_amd import engine, features

    S = torch.from_numpy(O.make_input("randn2", (2, 3, 20)))
    m = features.PCEN()
    with torch.no_grad():
        a = m(S)
    assert engine.pcen_route() == "host" and a.dtype == torch.float32 and tuple(a.shape) == (2, 3, 20)
    old = engine.set_pcen_kernel(False)
    try:
        with torch.no_grad():
            c = m(S)
        assert engine.pcen_route() == "composition"
    finally:
        assert engine.set_pcen_kernel(old) is False
    assert float((a - c).abs().max()) <= 1e-6
    mt = features.PCEN(trainable=True)
    y = mt(S)  # CPU tensors with grad: the composition, differentiable
    assert engine.pcen_route() == "composition" and y.requires_grad
    y.sum().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in mt.parameters())
    with torch.no_grad():  # (F, T) input, other floating types
        assert torch.equal(m(S[0]), a[0]) and torch.equal(m(S.double()), a)


@pytest.mark.parametrize("splits", [(1,), (64,), (100,), (1, 64, 100)])
def test_state_in_and_out(splits):
    """A row run in chunks with ``return_state`` / ``state`` against the oracle of the whole; a given state against the
    oracle with M[-1] = state."""
    from nnaudio_amd import features

    shape, pi = (2, 3, 203), 0
    S = O.make_input("randn2", shape)
    b, gain, bias, power, eps = O.params_f32(O.PARAMS[pi])
    m = features.PCEN(b=float(b[0]), gain=float(gain[0]), bias=float(bias[0]), power=float(power[0]), eps=float(eps))
    want, M, yard = O.reference(("fwd", shape, pi, "randn2", None), S, b, gain, bias, power, eps)
    edges = (0,) + tuple(splits) + (shape[2],)
    state, parts = None, []
    with torch.no_grad():
        for lo, hi in zip(edges[:-1], edges[1:]):
            out, state = m(torch.from_numpy(S[..., lo:hi]), state=state, return_state=True)
            assert tuple(state.shape) == shape[:2] and not state.requires_grad
            parts.append(out)
    O.check_rule("chunks %s" % (splits,), torch.cat(parts, dim=-1), want, yard)
    assert np.abs(state.numpy() - M[..., -1]).max() <= 2e-7 * np.abs(M[..., -1]).max()
    st = np.random.default_rng(2).random(shape[:2]).astype(np.float32) * 3
    want, _, yard = O.reference(("fwd-state", shape, pi), S, b, gain, bias, power, eps, st)
    with torch.no_grad():
        O.check_rule("given state", m(torch.from_numpy(S), state=torch.from_numpy(st)), want, yard)


def _write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for S, params, eps, state, G in cases:
            B, F, T = S.shape
            f.write(struct.pack("<4if", B * F, T, state is not None, G is not None, float(eps)))
            for p in params:  # per row: the row's channel's value
                f.write(np.tile(np.broadcast_to(p, (F,)), B).astype(np.float32).tobytes())
            f.write(S.tobytes())
            if state is not None:
                f.write(state.astype(np.float32).tobytes())
            if G is not None:
                f.write(G.astype(np.float32).tobytes())


def _read_results(path, cases):
    raw = open(path, "rb").read()
    pos, res = 0, []

    def take(n, dtype):
        nonlocal pos
        a = np.frombuffer(raw, dtype=dtype, count=n, offset=pos)
        pos += a.nbytes
        return a

    for S, params, eps, state, G in cases:
        B, F, T = S.shape
        r = {"out": take(B * F * T, np.float32).reshape(S.shape), "M": take(B * F * T, np.float64).reshape(S.shape),
             "last": take(B * F, np.float32).reshape(B, F)}
        if G is not None:
            r["dS"] = take(B * F * T, np.float32).reshape(S.shape)
            r["dstate"] = take(B * F, np.float32).reshape(B, F) if state is not None else None
            sums = take(B * F * 4, np.float64).reshape(B, F, 4).sum(0)  # over the clips, as the engine does
            if params[0].size == 1:
                sums = sums.sum(0, keepdims=True)
            for j, k in enumerate(("db", "dgain", "dbias", "dpower")):
                r[k] = sums[:, j].astype(np.float32)
        res.append(r)
    assert pos == len(raw)
    return res


def harness_cases():
    """Every input of the GPU suite: the forward shapes x parameter sets x inputs (scalar parameters, and per-channel
    ones where the GPU suite uses them), and the gradient shapes with random grad_output, scalar and per-channel,
    without and with a state."""
    cases, keys = [], []
    for shape in O.SHAPES:
        for pi, pset in enumerate(O.PARAMS):
            for name in O.INPUTS:
                for n in (None, shape[1]) if shape in ((2, 3, 65), (2, 128, 130)) else (None,):
                    p = O.params_f32(pset, n)
                    cases.append((O.make_input(name, shape), p[:4], p[4], None, None))
                    keys.append(("fwd", shape, pi, name, n))
    rng = np.random.default_rng(3)
    for shape in O.GRAD_SHAPES:
        G = rng.standard_normal(shape).astype(np.float32)
        st = (rng.random(shape[:2]) * 2).astype(np.float32)
        for pi, pset in enumerate(O.PARAMS):
            for name in O.INPUTS:
                for n in (None, shape[1]):
                    for state in (None, st):
                        p = O.params_f32(pset, n)
                        cases.append((O.make_input(name, shape), p[:4], p[4], state, G))
                        keys.append(("grad", shape, pi, name, n, state is not None))
    return cases, keys


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_harness_meets_the_rule(tmp_path, sanitize):
    """csrc/pcen.h compiled for the host (tests/native/pcen_harness.cpp): forward and backward of the 64-lane model on
    every input of the GPU suite, under the rule; built once more with -fsanitize=address,undefined (a stand-alone
    program: nothing is loaded into python), where the run must also end clean."""
    cxx = _clang()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "pcen_harness")
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run([cxx, *flags, "-std=c++17", "-I", os.path.join(ROOT, "nnaudio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "pcen_harness.cpp"), "-o", exe, "-lm"], check=True)
    cases, keys = harness_cases()
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "results.bin")
    _write_cases(src, cases)
    res = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(res.stdout)
    assert res.returncode == 0 and res.stdout.rstrip().endswith("%d cases ok" % len(cases)), res.stdout
    results = _read_results(dst, cases)
    if sanitize:  # (the figures are the first run's; here the run itself is the check, and that the results are finite)
        assert all(np.isfinite(v).all() for r in results for v in r.values() if v is not None)
        return
    fwd, grad = [], []
    for (S, params, eps, state, G), key, r in zip(cases, keys, results):
        if key[0] == "fwd":
            want, M, yard = O.reference(key, S, *params, eps)
            O.check_rule("harness %s" % (key,), r["out"], want, yard, fwd)
            assert np.abs(r["M"] - M).max() <= 1e-13 * max(np.abs(M).max(), 1e-30)
            assert np.array_equal(r["last"], r["M"][..., -1].astype(np.float32))
        else:
            want, yard = O.grad_reference(key, S, G, *params, eps, state)
            for k in O.GRAD_NAMES:
                if want[k] is not None:
                    O.check_rule("harness %s %s" % (key, k), r[k], want[k], yard[k], grad)
    print("largest ratios, forward: max %.2f rms %.2f; gradients: max %.2f rms %.2f"
          % (max(r[1] for r in fwd), max(r[2] for r in fwd), max(r[1] for r in grad), max(r[2] for r in grad)))


def test_argument_checks():
    from nnaudio_amd import _abi

    lib = _abi.load()
    for fn in (lib.mispec_pcen_f32, lib.mispec_pcen_bwd_f32):
        assert fn(None, None) == _abi.E_INVALID and b"NULL argument block" in lib.mispec_last_error()
    assert lib.mispec_pcen_host_f32(None) == _abi.E_INVALID
    a = _abi.PcenArgs()
    a.struct_size = 8
    assert lib.mispec_pcen_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"struct_size" in lib.mispec_last_error()
    a.struct_size = ctypes.sizeof(_abi.PcenArgs)
    assert lib.mispec_pcen_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"NULL pointer" in lib.mispec_last_error()
    a.s = a.b = a.gain = a.bias = a.power = a.out = 4096  # (nothing is dereferenced before the checks pass)
    assert lib.mispec_pcen_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"non-positive" in lib.mispec_last_error()
    a.n_clips, a.n_rows, a.n_frames, a.n_params, a.eps = 2, 3, 5, 2, 1e-6
    assert lib.mispec_pcen_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"n_params" in lib.mispec_last_error()
    a.n_params, a.eps = 3, 0.0
    assert lib.mispec_pcen_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"eps" in lib.mispec_last_error()
    a.eps, a.s_row_stride, a.s_clip_stride = 1e-6, 4, 15
    assert lib.mispec_pcen_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"stride of s" in lib.mispec_last_error()
    a.s_row_stride, a.out_row_stride, a.out_clip_stride = 5, 5, 14
    assert lib.mispec_pcen_host_f32(ctypes.byref(a)) == _abi.E_INVALID and b"stride of out" in lib.mispec_last_error()
    a.out_clip_stride, a.reserved = 15, 1
    assert lib.mispec_pcen_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"reserved" in lib.mispec_last_error()
    a.reserved = 0
    assert lib.mispec_pcen_bwd_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"grad_s or sums" in lib.mispec_last_error()
    a.m = a.grad_out = a.grad_s = a.sums = a.state_in = 4096
    assert lib.mispec_pcen_bwd_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"grad_state" in lib.mispec_last_error()
    a.grad_state = 4096
    assert lib.mispec_pcen_bwd_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"grad_out or grad_s" in lib.mispec_last_error()


def test_args_struct_layout_matches_the_header(tmp_path):
    from nnaudio_amd import _abi

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in _abi.PcenArgs._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mispec.h"', 'int main(void){',
            'printf("%zu\\n", sizeof(mispec_pcen_args));']
    prog += ['printf("%%zu\\n", offsetof(mispec_pcen_args, %s));' % f for f in fields]
    prog.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals[0] == ctypes.sizeof(_abi.PcenArgs)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_abi.PcenArgs, f).offset == off, f


def test_the_unit_is_part_of_the_gfx950_build():
    from nnaudio_amd import build

    assert any(os.path.basename(src) == "pcen.hip" for src, _ in build.UNITS)
    assert "pcen_fwd_kernelENS_10PcenParamsE" in build.refused_scratch({"pcen_fwd_kernelENS_10PcenParamsE": 8, "clean": 0},
                                                                       ablate=False)
    build.build(verbose=False)  # (compiles the unit for gfx950 when it is not up to date)
    assert os.path.exists(os.path.join(ROOT, "nnaudio_amd", "csrc", "libmispec.so"))
