"""CFP / Combined_Frequency_Periodicity without a GPU: buffers and attributes against the fixtures written from the
reference (scripts/gen_cfp_golden.py), the composition route under the tolerance rule of tests/_cfp_cases.py, the
documented deviations, the float64 oracle of the GPU suite, the host harness of csrc/cfp_fft.h and the library's query."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import _cfp_cases as C
from tests import _cfp_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_buffers_and_attributes_equal_the_reference(name):
    m, _ = C.build(name)
    rec, data = C.CASES[name], C.load(name)
    sd = m.state_dict()
    assert sorted(sd) == ["freq2logfreq_matrix", "h", "quef2logfreq_matrix"]
    for k, v in sd.items():
        want = data["buf_" + k]
        assert v.dtype == torch.float32 and tuple(v.shape) == want.shape, k
        assert np.array_equal(v.numpy(), want), k
    for a, want in rec["attrs"].items():
        if a == "t":
            continue
        assert getattr(m, a) == want, a
    assert np.array_equal(m.f, data["attr_f"]) and np.array_equal(m.q, data["attr_q"])
    assert m.g == rec["kwargs"].get("g", [0.24, 0.6, 1])


def test_default_shapes_and_supports():
    from nnaudio_amd import engine, features

    m = features.CFP()
    assert m.N == 8000 and m.HighFreqIdx == 501 and m.HighQuefIdx == 201 and m.tc_idx == 16 and m.fc_idx == 40
    assert tuple(m.freq2logfreq_matrix.shape) == (174, 501) and tuple(m.quef2logfreq_matrix.shape) == (174, 201)
    assert tuple(m.h.shape) == (2049,)
    for mat, widest in ((m.freq2logfreq_matrix, 14), (m.quef2logfreq_matrix, 6)):
        sup = engine.filterbank_support(mat)[0].numpy()
        assert (sup[:, 1] - sup[:, 0]).max() <= widest
        inside = np.zeros(mat.shape, dtype=bool)
        for r, (a, b) in enumerate(sup):
            inside[r, a:b] = True
        assert not (mat.numpy() != 0)[~inside].any()


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_composition_route_meets_the_rule(name):
    from nnaudio_amd import engine

    m, x = C.build(name)
    with torch.no_grad():
        y = m(x)
    assert engine.cfp_route() == "composition"
    assert torch.is_tensor(y) == (C.CASES[name]["class"] == "CFP")
    C.check_rule(name, y)
    assert np.array_equal(m.t, np.asarray(C.CASES[name]["attrs"]["t"]))


@pytest.mark.parametrize("name", C.CASE_NAMES)
def test_float64_oracle_agrees_with_the_reference(name):
    rec, data = C.CASES[name], C.load(name)
    m, _ = C.build(name)
    out = _cfp_oracle.cfp(data["x"], data["buf_h"], data["buf_freq2logfreq_matrix"], data["buf_quef2logfreq_matrix"],
                          N=m.N, hop=m.hop_length, g=m.g, tc_idx=m.tc_idx, fc_idx=m.fc_idx,
                          drop_edge_frames=rec["class"] != "CFP")
    for n, got in zip(C.NAMES, out[:len(rec["ref_f32_error"])]):
        want = data["out_" + n]
        assert got.shape == want.shape
        peak = np.abs(want).max()
        err = np.abs(got - want).max()
        print(name, n, "oracle vs reference float64: %.3e of peak %.3e" % (err / peak if peak else err, peak))
        assert err <= 1e-10 * peak, (name, n, err, peak)


def test_output_shapes_of_both_classes():
    from nnaudio_amd import features

    x = torch.randn(2, 4000)
    with torch.no_grad():
        z = features.CFP()(x)
        four = features.Combined_Frequency_Periodicity()(x)
    T = 1 + 4000 // 320
    assert tuple(z.shape) == (2, 174, T) and z.dtype == torch.float32
    assert len(four) == 4 and all(tuple(o.shape) == (2, 174, T - 2) for o in four)
    assert torch.equal(four[0], four[2] * four[3])
    # a clip shorter than one hop: one frame, none left after dropping the edges
    with torch.no_grad():
        assert tuple(features.CFP()(torch.randn(1, 100)).shape) == (1, 174, 1)
        assert tuple(features.Combined_Frequency_Periodicity()(torch.randn(1, 100))[0].shape) == (1, 174, 0)
    # other floating types are converted
    with torch.no_grad():
        assert torch.equal(features.CFP()(x.double()), z)


def test_state_dict_round_trip():
    from nnaudio_amd import features

    a = features.CFP(fr=4)
    b = features.CFP(fr=4)
    with torch.no_grad():
        b.h.zero_()
    b.load_state_dict(a.state_dict())
    x = torch.randn(1, 3000)
    with torch.no_grad():
        assert torch.equal(a(x), b(x))


def test_documented_deviations():
    from nnaudio_amd import features

    with pytest.raises(ValueError, match="at least two"):
        features.CFP(g=[0.24])
    with pytest.raises(ValueError, match="window_size"):
        features.Combined_Frequency_Periodicity(window_size=8001)
    m = features.CFP()
    with pytest.raises(ValueError, match=r"\(batch, samples\)"):
        m(torch.randn(16000))
    with pytest.raises(ValueError, match=r"\(batch, samples\)"):
        m(torch.randn(1, 1, 16000))
    x = torch.randn(1, 4000, requires_grad=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        m(x)
    with torch.no_grad():
        assert tuple(m(x).shape) == (1, 174, 13)
    assert not m(x.detach()).requires_grad


def test_cutoff_of_zero_zeroes_the_whole_layer():
    """The reference's ``X[:, :, -0:] = 0`` is the whole axis: a cutoff of 0 empties its layer.  (No constructor argument
    that the filterbanks accept rounds to a cutoff of 0; the attribute can be set, as on the reference's module.)"""
    from nnaudio_amd import features

    z = features.Combined_Frequency_Periodicity(fr=4)
    z.fc_idx = 0
    x = torch.randn(1, 4000)
    with torch.no_grad():
        Z, L0, LF, LQ = z(x)
    assert float(L0.abs().max()) > 0 and float(LQ.abs().max()) > 0
    assert float(LF.abs().max()) == 0 and float(Z.abs().max()) == 0
    want = _cfp_oracle.cfp(x.numpy(), z.h.numpy(), z.freq2logfreq_matrix.numpy(), z.quef2logfreq_matrix.numpy(), N=z.N,
                           hop=z.hop_length, g=z.g, tc_idx=z.tc_idx, fc_idx=z.fc_idx, drop_edge_frames=True)
    assert np.abs(want[2]).max() == 0
    assert np.abs(LQ.numpy() - want[3]).max() <= 1e-4 * np.abs(want[3]).max()


def test_legacy_import_location():
    with pytest.warns(Warning):
        import importlib

        import nnaudio_amd.Spectrogram as S

        importlib.reload(S)
    from nnaudio_amd import features

    assert S.CFP is features.CFP and S.Combined_Frequency_Periodicity is features.Combined_Frequency_Periodicity
    assert {"CFP", "Combined_Frequency_Periodicity"} <= set(features.__all__)


def test_switch_and_query():
    from nnaudio_amd import _abi, engine

    old = engine.set_cfp_kernel(False)
    assert engine.set_cfp_kernel(old) is False
    lib = _abi.load()
    assert lib.mispec_cfp_served(8000, 2049, 174, 3, 0) == 1
    assert lib.mispec_cfp_served(4000, 2049, 174, 2, 0) == 1 and lib.mispec_cfp_served(16000, 2049, 174, 4, 0) == 1
    assert lib.mispec_cfp_served(22050, 2049, 174, 3, 0) == 0  # 2 . 3^2 . 5^2 . 7^2
    assert lib.mispec_cfp_served(32000, 2049, 174, 3, 0) == 0  # 256 KB: beyond LDS
    assert lib.mispec_cfp_served(8000, 8001, 174, 3, 0) == 0 and lib.mispec_cfp_served(8000, 2049, 257, 3, 0) == 0
    assert lib.mispec_cfp_served(8000, 2049, 174, 1, 0) == 0 and lib.mispec_cfp_served(8000, 2049, 174, 9, 0) == 0
    assert lib.mispec_cfp_served(8000, 2049, 174, 3, 1) == 0  # a log layer (g == 0): the composition keeps it
    assert engine.cfp_served(8000, 2049, 174, [0.24, 0.6, 1]) and not engine.cfp_served(22050, 2049, 174, [0.24, 0.6, 1])
    assert not engine.cfp_served(8000, 2049, 174, [0.24, 0, 1])
    # the twiddle table: float64 values rounded once
    tw = np.empty((8000, 2), dtype=np.float32)
    assert lib.mispec_cfp_twiddles_host(8000, tw.ctypes.data) == 0
    k = np.arange(8000)
    assert np.array_equal(tw[:, 0], np.cos(-2 * np.pi * k / 8000).astype(np.float32)[:]) or \
        np.abs(tw[:, 0] - np.cos(2 * np.pi * k / 8000)).max() <= 6e-8
    assert np.abs(tw[:, 1] + np.sin(2 * np.pi * k / 8000)).max() <= 6e-8
    assert lib.mispec_cfp_twiddles_host(22050, tw.ctypes.data) == _abi.E_UNSUPPORTED
    # argument validation happens before any device work
    assert lib.mispec_cfp_f32(None, None) == _abi.E_INVALID
    a = _abi.CfpArgs()
    a.struct_size = 8
    assert lib.mispec_cfp_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"struct_size" in lib.mispec_last_error()
    a.struct_size = ctypes.sizeof(_abi.CfpArgs)
    assert lib.mispec_cfp_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"NULL" in lib.mispec_last_error()
    a.x = a.window = a.twiddle = a.fmat = a.qmat = a.f_support = a.q_support = a.z = 4096  # (nothing is dereferenced on the host)
    a.n_clips, a.n_samples, a.x_clip_stride, a.hop, a.n_frames, a.n_fft, a.window_size = 1, 16000, 16000, 320, 51, 22050, 2049
    a.n_out, a.f_cols, a.q_cols, a.n_layers, a.out_row_stride, a.out_clip_stride = 174, 501, 201, 3, 51, 174 * 51
    a.g[0], a.g[1], a.g[2] = 0.24, 0.6, 1.0
    assert lib.mispec_cfp_f32(ctypes.byref(a), None) == _abi.E_UNSUPPORTED
    a.n_fft, a.n_frames, a.out_row_stride, a.out_clip_stride = 8000, 52, 52, 174 * 52
    a.g[1] = 0.0
    assert lib.mispec_cfp_f32(ctypes.byref(a), None) == _abi.E_UNSUPPORTED and b"g == 0" in lib.mispec_last_error()
    a.g[1] = 0.6
    assert lib.mispec_cfp_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"more frames" in lib.mispec_last_error()


def test_args_struct_layout_matches_the_header(tmp_path):
    from nnaudio_amd import _abi

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in _abi.CfpArgs._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mispec.h"', 'int main(void){',
            'printf("%zu\\n", sizeof(mispec_cfp_args));']
    prog += ['printf("%%zu\\n", offsetof(mispec_cfp_args, %s));' % f for f in fields]
    prog.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals[0] == ctypes.sizeof(_abi.CfpArgs)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_abi.CfpArgs, f).offset == off, f


def _clang():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("amdclang++")):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_cfp_fft_header_against_float64_dft(tmp_path):
    """csrc/cfp_fft.h on the host: every served plan for N in {4000, 8000, 16000} and a set of small 2^a 5^b sizes, the
    magnitudes of a real frame and the two-frame packing behind the even part of the rectifier's output (tests/native/cfp_fft_harness.cpp)."""
    cxx = _clang()
    if cxx is None:
        pytest.skip("no clang++ (fft_core.h uses ext_vector_type)")
    exe = str(tmp_path / "cfp_fft_harness")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "nnaudio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "cfp_fft_harness.cpp"), "-o", exe, "-lm"], check=True)
    res = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout


def test_the_unit_is_part_of_the_gfx950_build():
    from nnaudio_amd import build

    assert any(os.path.basename(src) == "cfp.hip" for src, _ in build.UNITS)
    build.build(verbose=False)  # (compiles the unit for gfx950 when it is not up to date)
    assert os.path.exists(os.path.join(ROOT, "nnaudio_amd", "csrc", "libmispec.so"))
