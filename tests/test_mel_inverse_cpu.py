"""MelSpectrogram.to_stft / inverse without a GPU: the host harness of csrc/mel_nnls.h (sparse tables of real banks, the
kernel's iteration with the threads of a tile run one after the other, the served() rule), the composition route against
the NumPy oracle under the rule of tests/_mel_nnls_oracle.py, convergence as a property, the error paths and the
library's query and argument checks."""
import ctypes
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import _mel_nnls_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bank(name):
    from nnaudio_amd.basis import mel_filterbank

    return np.asarray(mel_filterbank(**O.BANKS[name]), dtype=np.float32)


def _module(name, power=2.0, **kw):
    from nnaudio_amd import features

    cfg = O.BANKS[name]
    return features.MelSpectrogram(hop_length=cfg["n_fft"] // 4, power=power, verbose=False, **cfg, **kw)


def _mel_of_random_spectrum(M, B, T, seed):
    """m = M S of a non-negative random spectrum (what a mel spectrogram is), float32."""
    rng = np.random.default_rng(seed)
    S = rng.random((B, M.shape[1], T)) ** 4
    return (M.astype(np.float64) @ S).astype(np.float32)


def _clang():
    for cand in ("/opt/rocm/lib/llvm/bin/clang++", shutil.which("clang++"), shutil.which("amdclang++"), shutil.which("g++")):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_banks_are_sparse_as_the_kernel_assumes():
    """Every row's non-zeros contiguous, at most 2 rows over a bin, the whole bank a few KB; the empty-rows bank has
    rows without a non-zero."""
    for name in O.BANKS:
        M = _bank(name)
        nz = M != 0
        for row in nz:
            idx = np.flatnonzero(row)
            assert idx.size == 0 or idx[-1] - idx[0] + 1 == idx.size, name
        assert nz.sum(0).max() <= 2, name
        assert nz.sum() <= 2100, name
    assert (~(_bank("empty-rows") != 0).any(1)).sum() > 0
    assert ((_bank("40/1024-band") != 0).sum(0) == 0).sum() > 100  # bins below fmin / above fmax


def test_header_tables_and_tile_iteration_on_the_host(tmp_path):
    """csrc/mel_nnls.h compiled for the host (tests/native/mel_nnls_harness.cpp): the tables of the five banks, the
    empty-rows bank and an n_fft = 4096 bank (16-, 8- and 4-frame tiles), two or more tiles with a ragged tail each, against the float64
    oracle under the rule; and the banks served() must refuse."""
    cxx = _clang()
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "mel_nnls_harness")
    subprocess.run([cxx, "-O2", "-std=c++17", "-I", os.path.join(ROOT, "nnaudio_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "mel_nnls_harness.cpp"), "-o", exe, "-lm"], check=True)
    from nnaudio_amd.basis import mel_filterbank

    banks = {n: _bank(n) for n in O.BANKS}
    banks["128/4096"] = np.asarray(mel_filterbank(22050, 4096, 128), dtype=np.float32)
    files = []
    for i, (name, M) in enumerate(banks.items()):
        F = M.shape[1]
        T = 16 + 3
        for power, n_iter, momentum in ((2.0, 64, True), (1.0, 8, False)):
            mel = _mel_of_random_spectrum(M, 1, T, seed=i)
            if n_iter == 8:
                mel[0, :, 1] = 0.0  # a silent column inside the tile
            want, yard = O.reference(("harness", name, power, n_iter, momentum), mel, M, power=power, n_iter=n_iter,
                                     momentum=momentum)
            path = str(tmp_path / ("case_%d_%d.bin" % (i, n_iter)))
            with open(path, "wb") as f:
                f.write(struct.pack("<4if3d", M.shape[0], F, T, n_iter, power, 1.0 / O.lipschitz(M), *yard))
                f.write(M.tobytes())
                f.write(mel[0].tobytes())
                f.write(O.betas(n_iter, momentum).tobytes())
                f.write(np.ascontiguousarray(want[0]).tobytes())
            files.append(path)
    res = subprocess.run([exe] + files, stdout=subprocess.PIPE, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout
    assert res.stdout.count("n_iter") == len(files) and res.stdout.rstrip().endswith("ok")


@pytest.mark.parametrize("name", ["16/256", "80/512"])
@pytest.mark.parametrize("power", [1.0, 2.0])
@pytest.mark.parametrize("momentum", [True, False])
@pytest.mark.parametrize("n_iter", [0, 1, 64])
def test_to_stft_on_cpu_tensors_meets_the_rule(name, power, momentum, n_iter):
    from nnaudio_amd import engine

    m = _module(name, power=power)
    M = m.mel_basis.numpy()
    mel = _mel_of_random_spectrum(M, 2, 7, seed=3)
    keys = sorted(m.state_dict())
    with torch.no_grad():
        got = m.to_stft(torch.from_numpy(mel), n_iter=n_iter, momentum=momentum)
    assert engine.mel_nnls_route() == "composition"
    assert sorted(m.state_dict()) == keys and not any(k.startswith("_") for k in keys)
    assert tuple(got.shape) == (2, M.shape[1], 7) and got.dtype == torch.float32
    want, yard = O.reference(("cpu", name, power, n_iter, momentum), mel, M, power=power, n_iter=n_iter, momentum=momentum)
    if n_iter == 0:
        assert not got.numpy().any() and not want.any()
        return
    O.check_rule("%s power %g momentum %s n_iter %d" % (name, power, momentum, n_iter), got, want, yard)


def test_two_dimensional_input_is_a_batch_of_one():
    m = _module("16/256")
    mel = torch.from_numpy(_mel_of_random_spectrum(m.mel_basis.numpy(), 1, 5, seed=4))
    with torch.no_grad():
        a = m.to_stft(mel[0], n_iter=16)
        b = m.to_stft(mel, n_iter=16)
    assert tuple(a.shape) == (1, 129, 5) and torch.equal(a, b)
    with torch.no_grad():  # other floating types are converted
        assert torch.equal(m.to_stft(mel.double(), n_iter=16), b)


def test_error_paths():
    m = _module("16/256")
    with pytest.raises(ValueError, match="16 mel bands"):
        m.to_stft(torch.zeros(1, 17, 4))
    with pytest.raises(ValueError, match="n_mels, frames"):
        m.to_stft(torch.zeros(16))
    with pytest.raises(ValueError, match="n_mels, frames"):
        m.to_stft(torch.zeros(1, 1, 16, 4))
    x = torch.rand(1, 16, 4, requires_grad=True)
    with pytest.raises(RuntimeError, match="not differentiable"):
        m.to_stft(x)
    with pytest.raises(RuntimeError, match="not differentiable"):
        m.inverse(x)
    with torch.no_grad():
        assert not m.to_stft(x, n_iter=2).requires_grad
    assert not m.to_stft(x.detach(), n_iter=2).requires_grad
    with pytest.raises(ValueError, match="n_iter"):
        m.to_stft(torch.zeros(1, 16, 4), n_iter=-1)
    assert tuple(m.to_stft(torch.zeros(0, 16, 4)).shape) == (0, 129, 4)
    assert tuple(m.to_stft(torch.zeros(2, 16, 0)).shape) == (2, 129, 0)


def test_all_zero_bank_and_all_zero_input_give_zeros():
    m = _module("16/256")
    mel = torch.from_numpy(_mel_of_random_spectrum(m.mel_basis.numpy(), 1, 3, seed=5))
    with torch.no_grad():
        assert not m.to_stft(torch.zeros(2, 16, 3), n_iter=8).any()
        m.mel_basis.zero_()  # (in place: the version counter invalidates the derived operands)
        out = m.to_stft(mel, n_iter=8)
    assert tuple(out.shape) == (1, 129, 3) and not out.any()


def test_derived_operands_follow_the_bank():
    from nnaudio_amd import engine

    m = _module("16/256")
    mel = torch.from_numpy(_mel_of_random_spectrum(m.mel_basis.numpy(), 1, 3, seed=6))
    with torch.no_grad():
        a = m.to_stft(mel, n_iter=8)
        ops = m._nnls_operands()
        assert m._nnls_operands() is ops and ops["served"]
        m.mel_basis.mul_(2.0)
        b = m.to_stft(mel, n_iter=8)
        assert m._nnls_operands() is not ops
    assert abs(m._nnls_operands()["L"] / ops["L"] - 4.0) < 1e-6
    # M -> 2 M: eta -> eta / 4 and the iterates halve (power 2: the square root of half)
    assert float((b * np.sqrt(2.0) - a).abs().max()) <= 1e-5 * float(a.abs().max())
    assert engine.mel_nnls_served(m.mel_basis, 2.0) and not engine.mel_nnls_served(torch.rand(16, 129), 2.0)
    assert "_nnls_derived" not in m.state_dict() and "_griffin_lim" not in dict(m.named_modules())


@pytest.mark.parametrize("name", ["16/256", "80/512"])
def test_convergence_of_the_projection(name):
    """|| M p - m || / || m || after 256 steps with momentum, for m = M S of a non-negative (uniform) random spectrum.
    The fp32 floor is measured here with the oracle's float32 run, and the module must stay within 4 x of it.
    Measured (float64 oracle / float32 oracle / module on CPU tensors): 7.3e-8 / 1.3e-7 / 1.3e-7 at 16 mels / n_fft 256,
    8.2e-7 / 9.4e-7 / 9.4e-7 at 80 / 512; the recovered spectrum is 0.52 and 0.44 (relative L2) away from the true one.
    The float64 run must also meet FISTA's guarantee f(p_k) - f* <= 2 L ||p_0 - p*||^2 / (k + 1)^2 with f = || M p - m ||^2 / 2,
    f* = 0 and p* = S (one of the minimisers), i.e. || M p_k - m || <= 2 sqrt(L) || S || / (k + 1) per frame column."""
    m = _module(name, power=1.0)
    M = m.mel_basis.numpy()
    M64 = M.astype(np.float64)
    S = np.random.default_rng(7).random((2, M.shape[1], 9))
    mel = (M64 @ S).astype(np.float32)

    def residual(p):
        p = np.asarray(p, dtype=np.float64)
        return float(np.linalg.norm(M64 @ p - mel) / np.linalg.norm(mel))

    p64 = O.nnls(mel, M, power=1.0, n_iter=256, momentum=True, dtype=np.float64)
    r64 = residual(p64)
    r32 = residual(O.nnls(mel, M, power=1.0, n_iter=256, momentum=True, dtype=np.float32))
    with torch.no_grad():
        got = m.to_stft(torch.from_numpy(mel), n_iter=256, momentum=True)
    ours = residual(got.numpy())
    print("%s: residual float64 oracle %.3e, float32 oracle %.3e, module %.3e" % (name, r64, r32, ours))
    bound = 2.0 * np.sqrt(O.lipschitz(M)) * np.linalg.norm(S, axis=1) / 257.0           # (2, 9): per frame column
    assert (np.linalg.norm(M64 @ p64 - mel, axis=1) <= bound + 1e-6 * np.linalg.norm(mel, axis=1)).all()
    assert ours <= 4.0 * r32
    assert float(got.min()) >= 0.0
    # ... and it is *a* solution, not the spectrum the mel values came from (the problem is underdetermined)
    rel = np.linalg.norm(got.numpy() - S) / np.linalg.norm(S)
    print("%s: recovered against true spectrum, relative L2 %.3f" % (name, rel))
    assert rel > 0.1


def test_inverse_is_to_stft_then_griffin_lim():
    from nnaudio_amd import features

    m = _module("16/256")
    mel = torch.from_numpy(_mel_of_random_spectrum(m.mel_basis.numpy(), 2, 9, seed=8))
    with torch.no_grad():
        torch.manual_seed(11)
        y = m.inverse(mel, n_iter=32, griffin_lim_iter=4)
        gl = features.Griffin_Lim(256, n_iter=4, hop_length=64, win_length=256, window="hann", center=True,
                                  pad_mode="reflect", momentum=0.99)
        torch.manual_seed(11)
        two_step = gl(m.to_stft(mel, n_iter=32))
    assert tuple(y.shape) == (2, 64 * (9 - 1)) and y.dtype == torch.float32 and bool(torch.isfinite(y).all())
    assert torch.equal(y, two_step)
    # the Griffin_Lim is built once per settings, a plain attribute: no sub-module, no state
    g0 = m._griffin_lim[(4, 0.99)]
    with torch.no_grad():
        m.inverse(mel, n_iter=2, griffin_lim_iter=4)
    assert m._griffin_lim[(4, 0.99)] is g0
    assert [n for n, _ in m.named_modules()] == ["", "stft"]
    assert sorted(m.state_dict()) == ["mel_basis", "stft.wcos", "stft.window_mask", "stft.wsin"]
    with torch.no_grad():
        m.inverse(mel, n_iter=2, griffin_lim_iter=2, griffin_lim_momentum=0.5)
    assert list(m._griffin_lim) == [(2, 0.5)] and m._griffin_lim[(2, 0.5)].momentum == 0.5


def test_betas_and_switch_and_query():
    from nnaudio_amd import _abi, engine

    assert np.array_equal(engine.mel_nnls_betas(64, True), O.betas(64, True))
    assert not engine.mel_nnls_betas(5, False).any() and engine.mel_nnls_betas(3, True)[0] == 0.0
    old = engine.set_mel_nnls_kernel(False)
    assert engine.set_mel_nnls_kernel(old) is False
    lib = _abi.load()
    for name in O.BANKS:
        M = np.ascontiguousarray(_bank(name))
        assert lib.mispec_mel_nnls_served(M.ctypes.data, M.shape[1], M.shape[0], M.shape[1], 2.0) == 1, name
        assert lib.mispec_mel_nnls_served(M.ctypes.data, M.shape[1], M.shape[0], M.shape[1], 0.0) == 0, name
        sizes = np.zeros(3, dtype=np.int32)
        assert lib.mispec_mel_nnls_tables_host(M.ctypes.data, M.shape[1], M.shape[0], M.shape[1], None, 0, sizes.ctypes.data) == 0
        assert sizes[1] == (M != 0).any(1).sum() and sizes[2] == (M != 0).sum()
        assert sizes[0] == 4 + 4 * sizes[1] + M.shape[1] + 2 * sizes[2]
        blob = np.zeros(int(sizes[0]) - 1, dtype=np.int32)
        assert lib.mispec_mel_nnls_tables_host(M.ctypes.data, M.shape[1], M.shape[0], M.shape[1], blob.ctypes.data, blob.size,
                                               sizes.ctypes.data) == _abi.E_INVALID and b"shorter" in lib.mispec_last_error()
    dense = np.random.default_rng(0).random((16, 129)).astype(np.float32)
    assert lib.mispec_mel_nnls_served(dense.ctypes.data, 129, 16, 129, 2.0) == 0
    assert lib.mispec_mel_nnls_served(None, 129, 16, 129, 2.0) == 0
    sizes = np.zeros(3, dtype=np.int32)
    assert lib.mispec_mel_nnls_tables_host(dense.ctypes.data, 129, 16, 129, None, 0, sizes.ctypes.data) == _abi.E_UNSUPPORTED
    assert [lib.mispec_mel_nnls_tile_frames(f) for f in (129, 513, 514, 1025, 1026, 2049)] == [16, 16, 8, 8, 4, 4]
    # argument validation happens before any device work
    assert lib.mispec_mel_nnls_f32(None, None) == _abi.E_INVALID
    a = _abi.MelNnlsArgs()
    a.struct_size = 8
    assert lib.mispec_mel_nnls_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"struct_size" in lib.mispec_last_error()
    a.struct_size = ctypes.sizeof(_abi.MelNnlsArgs)
    assert lib.mispec_mel_nnls_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"NULL" in lib.mispec_last_error()
    a.mel = a.tables = a.out = a.beta = 4096  # (nothing is dereferenced on the host)
    a.n_mels, a.n_bins, a.n_clips, a.n_frames, a.n_iter = 16, 129, 1, 5, 4
    a.mel_row_stride, a.mel_clip_stride, a.out_row_stride, a.out_clip_stride = 5, 80, 5, 129 * 5
    a.n_act, a.nnz, a.table_words, a.eta, a.power = 16, 231, 4 + 64 + 129 + 462, 0.5, 2.0
    a.mel_row_stride = 4
    assert lib.mispec_mel_nnls_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"stride" in lib.mispec_last_error()
    a.mel_row_stride, a.power = 5, 0.0
    assert lib.mispec_mel_nnls_f32(ctypes.byref(a), None) == _abi.E_UNSUPPORTED and b"power > 0" in lib.mispec_last_error()
    a.power, a.n_mels, a.mel_clip_stride = 2.0, 257, 257 * 5
    assert lib.mispec_mel_nnls_f32(ctypes.byref(a), None) == _abi.E_UNSUPPORTED
    a.n_mels, a.n_bins, a.out_clip_stride = 16, 4097, 4097 * 5
    assert lib.mispec_mel_nnls_f32(ctypes.byref(a), None) == _abi.E_UNSUPPORTED
    a.n_bins, a.out_clip_stride, a.table_words = 129, 129 * 5, 100
    assert lib.mispec_mel_nnls_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"table_words" in lib.mispec_last_error()
    a.table_words, a.reserved = 4 + 64 + 129 + 462, 1
    assert lib.mispec_mel_nnls_f32(ctypes.byref(a), None) == _abi.E_INVALID and b"reserved" in lib.mispec_last_error()


def test_args_struct_layout_matches_the_header(tmp_path):
    from nnaudio_amd import _abi

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no C compiler")
    fields = [f[0] for f in _abi.MelNnlsArgs._fields_]
    prog = ['#include <stdio.h>', '#include <stddef.h>', '#include "mispec.h"', 'int main(void){',
            'printf("%zu\\n", sizeof(mispec_mel_nnls_args));']
    prog += ['printf("%%zu\\n", offsetof(mispec_mel_nnls_args, %s));' % f for f in fields]
    prog.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(prog))
    exe = tmp_path / "layout"
    subprocess.check_call([gcc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    vals = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert vals[0] == ctypes.sizeof(_abi.MelNnlsArgs)
    for f, off in zip(fields, vals[1:]):
        assert getattr(_abi.MelNnlsArgs, f).offset == off, f


def test_the_unit_is_part_of_the_gfx950_build():
    from nnaudio_amd import build

    assert any(os.path.basename(src) == "mel_nnls.hip" for src, _ in build.UNITS)
    assert "mel_nnls_kernelILi8ELi17EE" in build.refused_scratch({"mel_nnls_kernelILi8ELi17EE": 8, "clean": 0}, ablate=False)
    build.build(verbose=False)  # (compiles the unit for gfx950 when it is not up to date)
    assert os.path.exists(os.path.join(ROOT, "nnaudio_amd", "csrc", "libmispec.so"))
