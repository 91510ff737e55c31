#!/usr/bin/env python3
"""Benchmark of the spectrogram hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full]

A plain run does what the headline needs and no more: it sets up, pre-warms, runs the W warm-up and the K timed
steps, writes --dump-outputs if given and prints the line (metric, value, unit, ms_per_step, dtype, config, "paths"
with the timed arithmetic alone, and "roofline" priced on the timed steps' own device time, traffic null).  The rest
of what is described below -- the other arithmetics, "extra", "gather", "roofline_cqt84", live traffic, the dominant
kernel timed alone, the reference's operator sequences on this GPU and the CPU baseline -- takes minutes of runs of
its own and is measured with ``--full`` only (``--extras``, ``--traffic`` and ``--cpu-baseline`` switch parts of it).

One "step" = one forward of the hot path over one batch of synthetic waveforms already
resident in HBM.  Workload at every N (weak scaling, per-GPU work fixed) is BASELINE.json's
configs[1]: STFT n_fft=2048 hop=512 hann, batch 64 x 10 s @ 44.1 kHz, Magnitude output.
The batch shards across ranks as independent clips (nnaudio_amd.dist); computing needs no
collective, so the timed region has none; the RCCL all-gather that reassembles the output
tensor is timed separately and reported under "gather" (never in `value`).

The step is the STFT module as it ships: its kernels are window x DFT (freq_scale='no'), so the
library evaluates every frame's DFT as an fp32 FFT (csrc/stft_fft.inl; one streaming pass: clips in,
spectrogram out) -- "roofline" prices it against the HBM roofline on the contract's algorithmic bytes.
The contraction kernels the same module uses when the FFT does not apply (trainable / non-linear
bases, n_fft > 2048) are timed in a --full run with the FFT switched off and reported under "paths":
"f16x3" (fp32 operands scaled by powers of two and split into (hi, lo) fp16 pairs, three f16 MFMAs per
product, fp32 accumulate; include/mispec.h MISPEC_PREC_F16X3; ~1e-7 of the spectrum peak), "bf16x3"
(split bf16, ~5e-6 of the peak) and "fp32" (fp32 MFMA), each with the dynamic range measured on this
device and its matrix-pipe roofline.

``--dump-outputs DIR`` writes what the last timed step returned (rank 0) to DIR/<workload>.npy after the timed
steps, at most 64 MB (a fixed seeded sample of a larger output, with its positions in DIR/<workload>_index.npy).  The
inputs are seeded, so two builds run with the same arguments can be compared output for output.

``python bench.py --gpus N`` without a torch.distributed environment starts its own N ranks
(``python -m torch.distributed.run``, one per GPU, RCCL) and relays rank 0's line.

Rank 0 prints ONE JSON line: metric = spectrogram frames/s (whole job), plus
  "roofline":        the STFT step as shipped = one launch of the FFT kernel: {"bound": "hbm", "achieved" =
                     algorithmic bytes (clips in + spectrogram out + the reference's two bases)
                     / the step's device time (HIP events on the launch stream), "peak" = 8000 GB/s, "frac",
                     "traffic" = fabric-side bytes per step from rocprofv3 PMC passes (FETCH_SIZE doubled as
                     MI355X_MICROARCH.md prescribes, + WRITE_SIZE) run live on this binary by this script
                     (``--traffic live``), or null}.  With ``--precision <p>`` the step is the contraction
                     kernels instead and the block is the matrix-pipe one: "achieved" = the flops the kernels
                     EXECUTE (MFMA instructions x 2 M N K; counted by the SQ_INSTS_VALU_MFMA_MOPS_* PMCs when
                     available, else from the tiling) / time; "peak" = the raw dense MFMA peak of the instruction
                     used (2500 TFLOP/s bf16 / f16, 157.3 fp32); "frac" <= 1; "algorithmic_frac" = 2 flop per
                     tap of the DENSE contraction the reference performs / time / (peak / MFMAs per product) --
                     it exceeds 1 once symmetric folds skip work, which is why it is not "frac".  The same
                     matrix-pipe figures of the contraction kernels are under "paths" in every --full run;
  "roofline_cqt84":  the same block for the other half of BASELINE.json's metric (CQT1992v2,
                     84 bins, B = 64), support-aware useful flops; as the module ships (fp32, default_module: true), with
                     same_bits_as_torch_conv1d = fraction of its complex output on this batch with the same bits as the
                     reference's own operator sequence on this GPU (reflect pad + F.conv1d, cqt.py:740-772) and
                     torch_conv1d_ms = what that sequence takes there; roofline_cqt84_f16x3 = the opt-in arithmetic;
  "extra":           Mel cfg3, Gammatonegram (as shipped: the FFT route, priced on bytes; "mel_f16x3" /
                     "gammatone_f16x3": the contraction route), and one rank's shard of cfg5 (CQT2010v2 and VQT,
                     64 x 30 s), each in its module's default arithmetic unless --precision is
                     given, timed with the same pre-warm and step count as the headline and priced
                     against both rooflines (with live traffic); at N > 1 also cfg4's real shard
                     (CQT1992v2, 16 clips per rank);
  "reference_ops_on_this_gpu": the reference forward's operator sequence for the headline workload (reflect pad + 2 x F.conv1d +
                     sqrt, stft.py:278-316) on THIS device through PyTorch-ROCm / MIOpen, inputs resident, configs[1]'s batch,
                     with the maximum difference from the product's spectrogram (of the peak) -- N = 1 only;
  "cpu_baseline":    the reference forward's operator sequence (pad + 2 x F.conv1d + sqrt, stft.py:278-316) on torch's CPU
                     kernels with the module's own buffers -- what nnAudio itself executes on a CPU; a restatement (kind
                     "port": the reference package is not on the GPU box) -- timed on this host on a bounded sample of the
                     same workload (rank 0, N=1 only); beside it the numpy port the parity tests check against
                     ("numpy_port"), torch.stft ("librosa_equivalent") and the same restatement for CQT84 ("cqt84").
"""
import argparse
import csv
import glob
import hashlib
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12  # FLOP/s, MI355X_MICROARCH.md (v_mfma_f32_32x32x2_f32)
PEAK_BF16_MFMA = 2.5e15   # FLOP/s dense, MI355X_MICROARCH.md (v_mfma_f32_32x32x16_bf16)
PEAK_HBM = 8.0e12         # B/s spec
MFMAS_PER_PRODUCT = {"fp32": 1, "bf16x3": 3, "f16x3": 3, "fft": 1}
# ("fft": the STFT's FFT path runs on the vector ALUs; the fp32 MFMA peak only prices its "algorithmic" flops)
RAW_PEAK = {"fp32": PEAK_F32_MFMA, "bf16x3": PEAK_BF16_MFMA, "f16x3": PEAK_BF16_MFMA, "fft": PEAK_F32_MFMA}  # f16 = bf16 rate
# peak for the precision used, in ALGORITHMIC flops ("bf16x3" = the dense bf16 MFMA
# peak / 3 MFMAs per product = 833 TFLOP/s, cfg2 floor 0.56 ms; fp32 MFMA 157.3, floor 2.95 ms)
PEAK = {k: RAW_PEAK[k] / MFMAS_PER_PRODUCT[k] for k in RAW_PEAK}
PRECISIONS = ("f16x3", "bf16x3", "fp32")
MOPS_COUNTERS = ("SQ_INSTS_VALU_MFMA_MOPS_F16", "SQ_INSTS_VALU_MFMA_MOPS_BF16", "SQ_INSTS_VALU_MFMA_MOPS_F32")


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def kernel_source_sha():
    """Fingerprint of the kernel sources the loaded library was built from."""
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(ROOT, "nnaudio_amd", "csrc", "*"))):
        if f.endswith((".hip", ".inl", ".h")):
            h.update(open(f, "rb").read())
    h.update(open(os.path.join(ROOT, "include", "mispec.h"), "rb").read())
    return h.hexdigest()[:16]


def fold_geometry(n_bins, K, fused_fb=False):
    """(bins inside whole MFMA tiles, folded taps per component) of the folded STFT contraction for
    an n_fft/2+1-bin Fourier basis -- mirror of plan_fold2 / plan_fold in csrc/mispec.hip: the second
    fold (K/4 taps, even and odd bins in 128-bin tiles, the Nyquist bin in the pre-pass) unless the
    filterbank is fused (then the single fold, K/2 taps)."""
    up = lambda v, m: (v + m - 1) // m * m
    if not fused_fb and K % 64 == 0 and n_bins >= 128:
        ne, no = (n_bins + 1) // 2, n_bins // 2
        if ne > 128 and ne % 128 == 1:
            ne -= 1
        return up(ne, 128) + up(no, 128), up(K // 4, 16)
    nb = n_bins - 1 if (n_bins > 128 and n_bins % 128 == 1) else n_bins
    return up(nb, 128), up(K // 2, 16)


def workload(name, device, B=None):
    """-> (module, make_input(seed), meta) ; meta: algorithmic flops / bytes per launch."""
    from nnaudio_amd import features

    B0 = B
    up = lambda v, m: (v + m - 1) // m * m
    if name == "stft":
        B, L, K, hop = B0 or 64, 441000, 2048, 512
        F, T = K // 2 + 1, L // hop + 1
        m = features.STFT(n_fft=K, hop_length=hop, window="hann", output_format="Magnitude",
                          verbose=False).to(device)
        flops = 2.0 * (2 * F) * K * B * T
        byts = 4.0 * (B * L + B * F * T + 2 * F * K)
        tag = "STFT n_fft=2048 hop=512 hann, B=64 x 10 s @ 44.1 kHz, Magnitude (configs[1])"
        bound = "mfma"
        bins, taps = fold_geometry(F, K, False)
        executed = 2.0 * (2 * bins) * taps * up(B * T, 128)  # products; x 3 MFMAs for the split arithmetics
    elif name == "stft4096":
        # n_fft = 4096 (a common music setting): the composite instance of the FFT route (two 2048-point halves + a butterfly)
        B, L, K, hop = B0 or 64, 441000, 4096, 1024
        F, T = K // 2 + 1, L // hop + 1
        m = features.STFT(n_fft=K, hop_length=hop, window="hann", output_format="Magnitude", verbose=False).to(device)
        flops = 2.0 * (2 * F) * K * B * T
        byts = 4.0 * (B * L + B * F * T + 2 * F * K)
        tag = "STFT n_fft=4096 hop=1024 hann, B=%d x 10 s @ 44.1 kHz, Magnitude" % B
        bound, executed = "hbm", None
    elif name in ("mel", "gammatone"):
        B, L, K, hop, M = (B0 or 256, 110250, 1024, 512, 128) if name == "mel" else (B0 or 64, 441000, 2048, 512, 64)
        F, T = K // 2 + 1, L // hop + 1
        if name == "mel":
            m = features.MelSpectrogram(sr=22050, n_fft=K, n_mels=M, hop_length=hop,
                                        verbose=False).to(device)
            tag = "MelSpectrogram n_fft=1024 hop=512 n_mels=128, B=%d x 5 s @ 22.05 kHz (configs[2])" % B
        else:
            m = features.Gammatonegram(sr=44100, n_fft=K, n_bins=M, hop_length=hop, verbose=False).to(device)
            tag = "Gammatonegram n_fft=2048 hop=512 64 bins, B=%d x 10 s @ 44.1 kHz (configs[1]'s batch)" % B
        flops = 2.0 * (2 * F) * K * B * T + 2.0 * M * F * B * T
        byts = 4.0 * (B * L + B * M * T + 2 * F * K + M * F)
        bound = "mfma"
        # the folded STFT (the banded mel reduction runs on the VALU inside its epilogue; the dense
        # gammatone reduction is a second, fp32-MFMA launch: not counted here)
        bins, taps = fold_geometry(F, K, name == "mel")
        executed = 2.0 * (2 * bins) * taps * up(B * T, 128)
    elif name == "cqt":
        B, L, hop = B0 or 64, 441000, 512
        m = features.CQT1992v2(sr=44100, hop_length=hop, fmin=32.70, n_bins=84, bins_per_octave=12,
                               verbose=False).to(device)
        T = L // hop + 1
        useful = float(m.lenghts.sum().item())
        flops = 2.0 * 2 * useful * B * T  # support-aware ("useful") flops
        byts = 4.0 * (B * L + B * 84 * T + 2 * useful)
        tag = "CQT1992v2 84 bins / 12 bpo hop=512, B=%d x 10 s @ 44.1 kHz, Magnitude" % B
        bound = "mfma"
        # executed: 8-bin (16-row MFMA) tiles over the tap range of their longest bin, zero padding included
        # (round 5: framed_gemm_kernel<..., T16>, round 6: cqt_chain_kernel; 16-bin tiles before: 1.49 x the useful products, now 1.22 x)
        lens = m.lenghts.detach().cpu().numpy()
        executed = {"fp32": 2.0 * sum(16 * float(lens[i:i + 8].max()) for i in range(0, 84, 8)) * B * T,
                    # the split arithmetics' strip kernel: 16-bin tiles
                    "split": 2.0 * sum(32 * float(lens[i:i + 16].max()) for i in range(0, 84, 16)) * B * T}
    elif name in ("cqt2010", "vqt"):
        B, L, hop = B0 or 64, 1323000, 512
        if name == "cqt2010":
            m = features.CQT2010v2(sr=44100, hop_length=hop, n_bins=96, verbose=False).to(device)
        else:
            m = features.VQT(sr=44100, hop_length=hop, n_bins=96, gamma=0, verbose=False).to(device)
        T = L // hop + 1
        nt = 256 * 2 * 12 * 8 * B * T * 2.0
        dec = sum(2.0 * 256 * B * (L // (2 ** o)) for o in range(1, 8))
        flops = nt + dec
        byts = 4.0 * (B * L + B * 96 * T)
        tag = ("%s 96 bins hop=512, B=64 x 30 s @ 44.1 kHz (one rank's shard of configs[4])"
               % ("CQT2010v2" if name == "cqt2010" else "VQT gamma=0"))
        bound = "hbm"
        executed = None
    elif name == "mfcc":
        B, L, K, hop, M = B0 or 256, 110250, 1024, 512, 128
        F, T = K // 2 + 1, L // hop + 1
        m = features.MFCC(sr=22050, n_mfcc=20, n_fft=K, n_mels=M, hop_length=hop, verbose=False).to(device)
        tag = "MFCC 20 coefficients over MelSpectrogram n_fft=1024 hop=512 n_mels=128, B=%d x 5 s @ 22.05 kHz" % B
        flops = 2.0 * (2 * F) * K * B * T + 2.0 * M * F * B * T + 2.0 * 20 * M * B * T
        byts = 4.0 * (B * L + B * 20 * T + 2 * F * K + M * F)
        bound, executed = "hbm", None
    elif name == "istft":
        # the step on the other side of the STFT (stft.py:15-63): cfg2's Complex spectrogram back to 64 x 10 s
        B, L, K, hop = B0 or 64, 441000, 2048, 512
        F, T = K // 2 + 1, L // hop + 1
        fwd = features.STFT(n_fft=K, hop_length=hop, window="hann", iSTFT=True, output_format="Complex",
                            verbose=False).to(device)

        class _Inverse(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.stft = fwd
                self.precision = None

            def forward(self, X):
                return self.stft.inverse(X, length=L)

        m = _Inverse()
        tag = "inverse STFT n_fft=2048 hop=512 hann of a (64, 1025, 862, 2) spectrogram -> 64 x 10 s @ 44.1 kHz"
        flops = 2.0 * (2 * F) * K * B * T
        byts = 4.0 * (B * F * T * 2 + B * L)
        bound, executed = "hbm", None

        def make_spec(seed):
            g = torch.Generator(device="cpu").manual_seed(seed)
            with torch.no_grad():
                return fwd(torch.randn(B, L, generator=g, dtype=torch.float32).to(device))

        return m, make_spec, dict(B=B, L=L, T=T, frames=B * T, flops=flops, bytes=byts, tag=tag,
                                  bound=bound, executed=executed, name=name)
    else:
        raise SystemExit("unknown workload %r" % name)

    def make_input(seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return torch.randn(B, L, generator=g, dtype=torch.float32).to(device)

    return m, make_input, dict(B=B, L=L, T=T, frames=B * T, flops=flops, bytes=byts, tag=tag,
                               bound=bound, executed=executed, name=name)


def prewarm(module, x, ms):
    """Untimed start-up work: the first launches after an idle period run 15-20 % slower (clock
    ramp, ~30 ms and more), which a short --steps/--warmup run would otherwise average in."""
    t0 = time.perf_counter()
    if ms > 0:
        with torch.no_grad():
            while (time.perf_counter() - t0) * 1e3 < ms:
                for _ in range(10):
                    module(x)
                torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def timed_steps(module, x, steps, warmup, sync, keep_last=False):
    """W untimed steps, then exactly K timed steps bracketed by sync() on both sides.
    Returns (wall seconds, device seconds from events on the launch stream), and with keep_last
    also what the last timed step returned (None when K = 0)."""
    y = None
    with torch.no_grad():
        for _ in range(warmup):
            y = module(x)
        sync()
        e0 = torch.cuda.Event(enable_timing=True)
        e1 = torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(steps):
            y = module(x)
        e1.record()
        sync()
        t1 = time.perf_counter()
    if keep_last:
        return t1 - t0, e0.elapsed_time(e1) * 1e-3, (y if steps > 0 else None)
    del y
    return t1 - t0, e0.elapsed_time(e1) * 1e-3


DUMP_BUDGET = 60 << 20  # bytes, all arrays of one --dump-outputs together (under 64 MB, headers included)
DUMP_SAMPLE_SEED = 20240601


def dump_outputs(y, out_dir, name, budget=DUMP_BUDGET):
    """Write what a step returned as ``out_dir/<name>.npy`` (float32; float64 stays float64), for comparing two
    builds output for output.  A tuple / list of tensors becomes ``<name>_<i>``; complex tensors are stored as
    (..., 2) real pairs.  An array larger than its share of `budget` is replaced by a fixed sample: the elements at
    sorted flat (C-order) positions drawn with a fixed seed from its shape alone, values in ``<name>.npy`` and
    the positions (exact in float64) in ``<name>_index.npy``.  Returns {file name: shape written}."""
    ys = list(y) if isinstance(y, (tuple, list)) else [y]
    names = [name] if len(ys) == 1 else ["%s_%d" % (name, i) for i in range(len(ys))]
    share = budget // len(ys) - 4096  # (room for the .npy headers)
    os.makedirs(out_dir, exist_ok=True)
    written = {}
    for nm, t in zip(names, ys):
        t = t.detach()
        if t.is_complex():
            t = torch.view_as_real(t)
        t = t.to(torch.float64 if t.dtype == torch.float64 else torch.float32)
        item = t.element_size()
        n = t.numel()
        if n * item <= share:
            arrays = {nm: t.cpu().numpy()}
        else:
            # values + float64 positions in the share; drawn with replacement, duplicates dropped
            k = share // (item + 8)
            idx = np.unique(np.random.default_rng(DUMP_SAMPLE_SEED).integers(0, n, size=k))
            vals = t.reshape(-1)[torch.from_numpy(idx).to(t.device)].cpu().numpy()
            arrays = {nm: vals, nm + "_index": idx.astype(np.float64)}
        for fn, a in arrays.items():
            np.save(os.path.join(out_dir, fn + ".npy"), np.ascontiguousarray(a))
            written[fn + ".npy"] = list(a.shape)
    return written


def module_precision(name, precision):
    """The arithmetic a workload's module runs in: --precision when given, else the module's own
    default: "fft" for the STFT family (window x DFT kernels: the fp32 FFT path, whatever the precision
    setting), f16x3 for CQT2010v2 / VQT, fp32 for CQT1992v2 (nnaudio_amd.engine)."""
    if precision:
        return precision
    if name in ("stft", "stft4096", "mel", "gammatone", "mfcc", "istft"):
        from nnaudio_amd import engine

        return "fft" if engine.fft_enabled() else "f16x3"
    return "fp32" if name == "cqt" else "f16x3"


def reference_ops_on_gpu(x):
    """What the REFERENCE'S OWN operator sequence for the headline workload costs on this GPU: nnAudio's STFT.forward is
    ReflectionPad1d + two F.conv1d with the windowed Fourier kernels + sqrt (stft.py:278-316); with PyTorch-ROCm that is
    MIOpen on the MI355X.  Restated here on a product module's buffers (the same values the reference registers), timed with
    inputs resident, next to the product's Magnitude of the same clips (maximum difference, of the peak)."""
    import torch.nn.functional as F

    from nnaudio_amd import features

    m = features.STFT(n_fft=2048, hop_length=512, window="hann", output_format="Magnitude", verbose=False).to(x.device)
    kc, ks = (k if k.dim() == 3 else k[:, None, :] for k in (m.wcos, m.wsin))  # (registered (freq_bins, 1, n_fft), as the reference's)
    with torch.no_grad():
        def reference():
            xp = F.pad(x[:, None, :], (m.pad_amount, m.pad_amount), mode="reflect")
            re, im = F.conv1d(xp, kc, stride=m.stride), F.conv1d(xp, ks, stride=m.stride)
            return torch.sqrt(re.pow(2) + im.pow(2))

        ref = reference()
        y = m(x)
        err = float((y - ref).abs().max() / ref.abs().max())
        sync = torch.cuda.synchronize if x.is_cuda else (lambda: None)
        sync()
        t0 = time.perf_counter()
        for _ in range(3):
            reference()
        sync()
        ms = (time.perf_counter() - t0) / 3 * 1e3
    return {"what": "reflect pad + 2 x F.conv1d + sqrt (stft.py:278-316) on this GPU, configs[1]'s batch", "ms_per_step": round(ms, 3),
            "value": round(x.shape[0] * ref.shape[2] / ms * 1e3, -3), "unit": "frames/s", "max_diff_of_peak": float("%.2e" % err)}


def reference_ops_mel_on_gpu(device):
    """The reference's operator sequence for configs[2] (mel.py:184-189: stft(x, 'Magnitude') ** power, then
    torch.matmul(mel_basis, spec); the STFT being pad + 2 x F.conv1d + sqrt) on this GPU, on a product module's buffers, beside
    the product's own forward of the same clips."""
    import torch.nn.functional as F

    from nnaudio_amd import features

    m = features.MelSpectrogram(sr=22050, n_fft=1024, n_mels=128, hop_length=512, verbose=False).to(device)
    x = torch.randn(256, 110250, generator=torch.Generator().manual_seed(301)).to(device)
    st = m.stft
    kc, ks = (k if k.dim() == 3 else k[:, None, :] for k in (st.wcos, st.wsin))
    with torch.no_grad():
        def reference():
            xp = F.pad(x[:, None, :], (st.pad_amount, st.pad_amount), mode="reflect")
            re, im = F.conv1d(xp, kc, stride=st.stride), F.conv1d(xp, ks, stride=st.stride)
            return torch.matmul(m.mel_basis, torch.sqrt(re.pow(2) + im.pow(2)) ** m.power)

        ref = reference()
        err = float((m(x) - ref).abs().max() / ref.abs().max())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            reference()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 3 * 1e3
    return {"what": "reflect pad + 2 x F.conv1d + sqrt, ** power, matmul(mel_basis, .) (mel.py:184-189) on this GPU, configs[2]'s batch",
            "ms_per_step": round(ms, 3), "value": round(x.shape[0] * ref.shape[2] / ms * 1e3, -3), "unit": "frames/s",
            "max_diff_of_peak": float("%.2e" % err)}


def reference_ops_cqt2010_on_gpu(device):
    """The reference's operator sequence for one rank's shard of configs[4] (CQT2010v2.forward, cqt.py:1085-1130, with
    get_cqt_complex and downsampling_by_2 of utils.py:498-521, 102-124: per octave pad + 2 x F.conv1d, between octaves the
    anti-alias F.conv1d with stride 2, the growing torch.cat) on this GPU, on a product module's buffers, beside the product's
    own forward (f16x3 streaming kernel) of the same clips."""
    import torch.nn.functional as F

    from nnaudio_amd import features

    m = features.CQT2010v2(sr=44100, hop_length=512, n_bins=96, verbose=False).to(device)
    x = torch.randn(64, 1323000, generator=torch.Generator().manual_seed(302)).to(device)
    kr, ki = m.cqt_kernels_real, m.cqt_kernels_imag
    pad = m.n_fft // 2
    with torch.no_grad():
        def octave(sig, hop):
            xp = F.pad(sig, (pad, pad), mode=m.pad_mode) if m.pad_mode == "reflect" else F.pad(sig, (pad, pad))
            return torch.stack((F.conv1d(xp, kr, stride=hop), -F.conv1d(xp, ki, stride=hop)), -1)

        def reference():
            sig = x[:, None, :]
            if m.earlydownsample:
                f = m.early_downsample_filter
                sig = F.conv1d(sig, f, stride=int(m.downsample_factor), padding=(f.shape[-1] - 1) // 2)
            hop = m.hop_length
            out = octave(sig, hop)
            for _ in range(m.n_octaves - 1):
                hop //= 2
                sig = F.conv1d(sig, m.lowpass_filter, stride=2, padding=(m.lowpass_filter.shape[-1] - 1) // 2)
                out = torch.cat((octave(sig, hop), out), 1)
            out = out[:, -m.n_bins:, :] * m.downsample_factor * torch.sqrt(m.lenghts.view(-1, 1, 1))
            return torch.sqrt(out.pow(2).sum(-1))

        ref = reference()
        err = float((m(x) - ref).abs().max() / ref.abs().max())
        del ref
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(2):
            reference()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / 2 * 1e3
    T = x.shape[1] // 512 + 1
    return {"what": "CQT2010v2.forward's operator sequence (cqt.py:1085-1130, utils.py:498-521, 102-124) on this GPU, one rank's shard of configs[4]",
            "ms_per_step": round(ms, 3), "value": round(x.shape[0] * T / ms * 1e3, -3), "unit": "frames/s",
            "max_diff_of_peak": float("%.2e" % err)}


def same_bits_as_conv1d(mod, x, timed=False):
    """CQT1992v2 module (Magnitude) on `x` against torch's conv1d with the module's own buffers (reference cqt.py:740-772):
    fraction of the (re, im) elements with identical bits; timed: also the milliseconds of that operator sequence on x's device."""
    import torch.nn.functional as F

    with torch.no_grad():
        y = mod(x, output_format="Complex")
        s = torch.sqrt(mod.lenghts.view(-1, 1))

        def reference():
            xp = F.pad(x[:, None, :], (mod.kernel_width // 2,) * 2, mode="reflect")
            return (F.conv1d(xp, mod.cqt_kernels_real, stride=mod.hop_length) * s,
                    -F.conv1d(xp, mod.cqt_kernels_imag, stride=mod.hop_length) * s)

        re, im = reference()
        same = round(float(((y[..., 0] == re) & (y[..., 1] == im)).float().mean()), 6)
        if not timed:
            return same
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            reference()
        torch.cuda.synchronize()
        return same, round((time.perf_counter() - t0) / 3 * 1e3, 3)


def executed_flops(meta, precision):
    """MFMA flops the kernels execute per step, from the tiling (None: no model for this workload)."""
    ex = meta.get("executed")
    if isinstance(ex, dict):  # per arithmetic (CQT1992v2: the fp32 tile kernel and the strip kernel tile the bank differently)
        ex = ex["fp32" if precision == "fp32" else "split"]
    if not ex:
        return None
    return ex * MFMAS_PER_PRODUCT[precision]


def roofline_block(meta, dev_step_s, precision, traffic=None, kernel="", executed=None, executed_source="tiling"):
    """The line's roofline object for one workload (per launch = per step).  MFMA-bound workloads:
    achieved = EXECUTED flops / time against the raw MFMA peak (frac <= 1); the contract's
    algorithmic figure (2 flop per tap of the dense contraction) sits beside it."""
    fl = meta["flops"] / dev_step_s
    by = meta["bytes"] / dev_step_s
    blk = {"bound": meta["bound"], "unit": "TFLOP/s" if meta["bound"] == "mfma" else "GB/s",
           "traffic": traffic, "kernel": kernel, "step_device_ms": dev_step_s * 1e3,
           "algorithmic_flops_per_launch": meta["flops"],
           "algorithmic_bytes_per_launch": meta["bytes"],
           "algorithmic_tflops": fl / 1e12,
           "algorithmic_frac": None if precision == "fft" else fl / PEAK[precision],
           "algorithmic_frac_what": "2 flop per tap of the dense contraction / time / (raw MFMA peak / MFMAs per "
                                    "product): the SURVEY 8d figure; > 1 is possible because the symmetric folds skip work",
           "hbm_frac_on_algorithmic_bytes": by / PEAK_HBM}
    if executed is None and precision != "fft":
        executed = executed_flops(meta, precision)
        executed_source = "tiling"
    if executed:
        ex = executed / dev_step_s
        blk.update(executed_flops_per_launch=executed, executed_source=executed_source,
                   executed_mfma_tflops=ex / 1e12, executed_frac_of_raw_mfma_peak=ex / RAW_PEAK[precision])
    if meta["bound"] == "mfma" and executed:
        blk.update(achieved=executed / dev_step_s / 1e12, peak=RAW_PEAK[precision] / 1e12,
                   frac=executed / dev_step_s / RAW_PEAK[precision])
    elif meta["bound"] == "mfma":
        blk.update(achieved=fl / 1e12, peak=PEAK[precision] / 1e12, frac=min(1.0, fl / PEAK[precision]))
    else:
        blk.update(achieved=by / 1e9, peak=PEAK_HBM / 1e9, frac=by / PEAK_HBM)
    return blk


# ---------------------------------------------------------------------------------------
# HBM-side traffic of one step, measured live: rocprofv3 PMC passes (counters only, one counter
# per pass) over a child process that runs a few steps of one workload
# ---------------------------------------------------------------------------------------
def pmc_child(name, precision, steps):
    import nnaudio_amd

    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    nnaudio_amd.set_precision(precision or None)
    if precision and name == "stft":  # a forced arithmetic benchmarks the contraction kernels
        from nnaudio_amd import engine

        engine.set_fft(False)
    module, make_input, _ = workload(name, device)
    x = make_input(0)
    with torch.no_grad():
        for _ in range(steps):
            module(x)
    torch.cuda.synchronize()


def _ours(kernel_name):
    return not (kernel_name.startswith("void at::") or kernel_name.startswith("__amd_rocclr")
                or "at::native" in kernel_name)


def measure_traffic(name, precision, steps=4, timeout=150):
    """-> dict(bytes_per_step, fetch_bytes, write_bytes, mfma_flops, per_kernel, method) or raises.
    Three rocprofv3 passes (counters only) over a child process running `steps` forwards:
    FETCH_SIZE, WRITE_SIZE, and the MFMA op counters (SQ_INSTS_VALU_MFMA_MOPS_*: 512 flops each)."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        raise RuntimeError("rocprofv3 not found")
    res = {}
    per_kernel = {}
    env = dict(os.environ, TMPDIR="/tmp")
    for env_key in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(env_key, None)
    passes = [("FETCH_SIZE",), ("WRITE_SIZE",), MOPS_COUNTERS]
    for counters in passes:
        d = tempfile.mkdtemp(prefix="mispec_pmc_", dir="/tmp")
        try:
            cmd = [prof, "--pmc", *counters, "--output-format", "csv", "-d", d, "-o", "pmc", "--",
                   sys.executable, os.path.abspath(__file__), "--pmc-child", name,
                   "--precision", precision or "auto", "--steps", str(steps)]
            try:
                subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=timeout, check=True)
            except Exception:
                if counters is MOPS_COUNTERS:  # the op counters are a bonus: the byte passes decide
                    continue
                raise
            files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            if not files:
                if counters is MOPS_COUNTERS:
                    continue
                raise RuntimeError("no counter_collection.csv from the %s pass" % (counters,))
            for f in files:
                for r in csv.DictReader(open(f)):
                    counter = r.get("Counter_Name")
                    if counter not in counters or not _ours(r.get("Kernel_Name", "")):
                        continue
                    v = float(r.get("Counter_Value") or 0.0)
                    v *= 512.0 if counter in MOPS_COUNTERS else 1024.0  # MFMA ops -> flops; KB -> bytes
                    res[counter] = res.get(counter, 0.0) + v / steps
                    k = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "")
                    k = k.split("(")[0].split("<")[0][-60:]
                    per_kernel.setdefault(k, {}).setdefault(counter, 0.0)
                    per_kernel[k][counter] += v / steps
        finally:
            shutil.rmtree(d, ignore_errors=True)
    # gfx950: FETCH_SIZE tallies 64 B per 128-B request of a 16 B/lane stream (MI355X_MICROARCH.md,
    # HBM section): doubled.  Infinity-Cache hits are included: an upper bound on HBM bytes.
    fetch = 2.0 * res["FETCH_SIZE"]
    for k in per_kernel:
        if "FETCH_SIZE" in per_kernel[k]:
            per_kernel[k]["FETCH_SIZE"] *= 2.0
    mfma = {c: res[c] for c in MOPS_COUNTERS if c in res}
    return {"bytes_per_step": fetch + res["WRITE_SIZE"], "fetch_bytes": fetch,
            "write_bytes": res["WRITE_SIZE"], "mfma_flops": sum(mfma.values()) if mfma else None,
            "mfma_flops_by_type": mfma, "per_kernel": per_kernel,
            "method": "rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE / SQ_INSTS_VALU_MFMA_MOPS_{F16,BF16,F32} (x 512 flops), "
                      "separate passes over %d steps of this binary, run by bench.py; FETCH_SIZE x2 (gfx950 "
                      "16 B/lane streams); fabric-side bytes (Infinity-Cache hits included)" % steps}


def dynamic_range_db(device, precision):
    """What the arithmetic leaves in the silent bins of a pure tone, relative to the peak (dB): STFT
    n_fft=2048 of a sine exactly on bin 400, bins more than 20 away from it, interior frames."""
    from nnaudio_amd import features

    m = features.STFT(n_fft=2048, hop_length=512, output_format="Complex", verbose=False).to(device)
    if precision is not None:
        m.precision = precision
    n = torch.arange(40 * 512, dtype=torch.float64)
    x = torch.cos(2 * np.pi * 400 * n / 2048 + 0.3).to(torch.float32)[None, :].to(device)
    with torch.no_grad():
        y = m(x)[0, :, 4:-4].double()
    mag = torch.sqrt(y[..., 0] ** 2 + y[..., 1] ** 2)
    silent = torch.cat((mag[:380], mag[420:]))
    return float(20 * torch.log10(silent.max() / mag.max() + 1e-300))


def cpu_baseline(budget_s=15.0):
    """CPU baselines on this host, each on a bounded sample of its workload (frames/s):
      value               the reference forward's OPERATOR SEQUENCE for configs[1] (stft.py:278-316: ReflectionPad1d, two F.conv1d
                          with wcos / wsin, sqrt of the squares) on torch's CPU kernels with the module's own buffers -- what nnAudio
                          itself executes on a CPU; the reference package is not on the GPU box, so this is a restatement
                          (kind "port"), not an import (VERDICT r4 "missing" 7)
      numpy_port          oracle/spectral_oracle.py (numpy float32 BLAS), the checker the parity tests use
      librosa_equivalent  torch.stft(...).abs(): the FFT algorithm librosa.stft runs (librosa cannot be installed)
      cqt84               the same operator-sequence restatement for CQT1992v2 84 bins (cqt.py:740-772)"""
    import torch.nn.functional as Fnn

    from nnaudio_amd import features
    from oracle import spectral_oracle as O

    m = features.STFT(n_fft=2048, hop_length=512, window="hann", output_format="Magnitude",
                      verbose=False)
    rng = np.random.default_rng(0)
    n = 8
    x = rng.standard_normal((n, 441000)).astype(np.float32)
    xt = torch.from_numpy(x)
    wc_t, ws_t = m.wcos.detach(), m.wsin.detach()

    def ref_ops():
        xp = Fnn.pad(xt[:, None, :], (1024, 1024), mode="reflect")
        re, im = Fnn.conv1d(xp, wc_t, stride=512), Fnn.conv1d(xp, ws_t, stride=512)
        return torch.sqrt(re.pow(2) + im.pow(2))

    with torch.no_grad():
        ref_ops()
        t0 = time.perf_counter()
        reps, dt = 0, 0.0
        while dt < budget_s and reps < 200:  # repeat the sample until ~budget_s of CPU work
            ref_ops()
            reps += 1
            dt = time.perf_counter() - t0
    cores = int(torch.get_num_threads())
    out = dict(value=reps * n * 862 / dt, unit="frames/s", cores=cores, kind="port",
               sample="%d x %d of 64 clips (10 s @ 44.1 kHz) of configs[1]: the reference forward's operator sequence (pad + 2 x "
                      "F.conv1d + sqrt, stft.py:278-316) on torch's CPU kernels with the module's buffers; the reference package "
                      "itself is not on the GPU box, %.1f s" % (reps, n, dt))
    try:
        wsin, wcos = m.wsin.numpy(), m.wcos.numpy()
        xs = x[:2]
        t0 = time.perf_counter()
        reps1 = 0
        while time.perf_counter() - t0 < 5.0 and reps1 < 20:
            O.stft(xs, wsin, wcos, 512, output_format="Magnitude", acc=np.float32)
            reps1 += 1
        dt1 = time.perf_counter() - t0
        out["numpy_port"] = dict(value=reps1 * xs.shape[0] * 862 / dt1, unit="frames/s",
                                 what="oracle/spectral_oracle.py (numpy float32 BLAS restatement, the parity checker), "
                                      "%d clips x %d, %.1f s" % (xs.shape[0], reps1, dt1))
    except Exception as e:
        out["numpy_port"] = {"error": repr(e)}
    try:
        win = torch.hann_window(2048, periodic=True)
        t0 = time.perf_counter()
        reps2 = 0
        while time.perf_counter() - t0 < 4.0:
            torch.stft(xt, 2048, hop_length=512, window=win, center=True, pad_mode="reflect",
                       return_complex=True).abs()
            reps2 += 1
        dt2 = time.perf_counter() - t0
        out["librosa_equivalent"] = dict(
            value=reps2 * xt.shape[0] * 862 / dt2, unit="frames/s", cores=cores,
            what="torch.stft(n_fft=2048, hop=512, hann, reflect).abs() on CPU: the FFT algorithm of "
                 "librosa.stft (librosa is not installed), %d clips x %d, %.1f s" % (xt.shape[0], reps2, dt2))
    except Exception as e:
        out["librosa_equivalent"] = {"error": repr(e)}
    try:
        c = features.CQT1992v2(sr=44100, hop_length=512, fmin=32.70, n_bins=84, bins_per_octave=12,
                               verbose=False)
        kr, ki, ln = c.cqt_kernels_real.detach(), c.cqt_kernels_imag.detach(), c.lenghts.detach()
        xc = xt[:2]

        def cqt_ops():
            xp = Fnn.pad(xc[:, None, :], (c.kernel_width // 2, c.kernel_width // 2), mode="reflect")
            re = Fnn.conv1d(xp, kr, stride=512) * torch.sqrt(ln.view(-1, 1))
            im = -Fnn.conv1d(xp, ki, stride=512) * torch.sqrt(ln.view(-1, 1))
            return torch.sqrt(re.pow(2) + im.pow(2))

        with torch.no_grad():
            cqt_ops()
            t0 = time.perf_counter()
            reps3 = 0
            while time.perf_counter() - t0 < 6.0 and reps3 < 50:
                cqt_ops()
                reps3 += 1
            dt3 = time.perf_counter() - t0
        out["cqt84"] = dict(value=reps3 * xc.shape[0] * 862 / dt3, unit="frames/s", cores=cores, kind="port",
                            sample="%d x %d clips (10 s @ 44.1 kHz): the reference CQT1992v2 forward's operator sequence (pad + 2 x "
                                   "F.conv1d with the 32768-tap kernels + sqrt, cqt.py:740-772) on torch's CPU kernels, %.1f s"
                                   % (reps3, xc.shape[0], dt3))
    except Exception as e:
        out["cqt84"] = {"error": repr(e)}
    return out


# ---------------------------------------------------------------------------------------
# the printed line: the contract's fields only, <= LINE_BUDGET characters; everything else goes
# to the side file bench_detail.json (the driver keeps 8 KB of stdout: a longer line is unparsed)
# ---------------------------------------------------------------------------------------
LINE_BUDGET = 4096
DETAIL_FILE = "bench_detail.json"


def _r(v, sig=5):
    """Numbers to `sig` significant digits (the line is a report, the side file keeps full precision)."""
    if isinstance(v, bool) or v is None or isinstance(v, (int, str)):
        return v
    if isinstance(v, float):
        if v != v or v in (float("inf"), float("-inf")):
            return None
        if v == 0.0:
            return 0.0
        return float("%.*g" % (sig, v))
    return v


def _pick(d, keys):
    return {k: _r(d[k]) for k in keys if isinstance(d, dict) and k in d and d[k] is not None}


def _short_kernel(name, n=60):
    return (name or "").split(" (")[0][:n]


def compact_line(out):
    """The one-line JSON record from the full result dict: contract fields, the roofline /
    cpu_baseline objects, one short record per path / extra.  No prose longer than 80 characters,
    no per-kernel dictionaries (those are in the side file)."""
    line = _pick(out, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                       "higher_is_better", "scaling", "dtype", "data"))
    line["vs_baseline"] = out.get("vs_baseline")
    cfg = out.get("config", {})
    line["config"] = {"workload": cfg.get("workload", "")[:90], "global_batch": cfg.get("global_batch"),
                      "precision": (cfg.get("precision_short") or cfg.get("precision") or "")[:80],
                      "parallelism": (cfg.get("parallelism") or "")[:48]}
    rk = ("bound", "achieved", "peak", "unit", "frac", "traffic", "step_device_ms",
          "algorithmic_bytes_per_launch")

    def roof(blk):
        r = _pick(blk, rk)
        r.setdefault("traffic", None)
        if blk.get("bound") == "mfma":
            r.update(_pick(blk, ("algorithmic_frac", "hbm_frac_on_algorithmic_bytes")))
        dk = blk.get("dominant_kernel")
        if dk:
            r["dominant_kernel"] = {"name": _short_kernel(dk.get("name")), "avg_ms": _r(dk.get("avg_ms"))}
        return r

    if "roofline" in out:
        line["roofline"] = roof(out["roofline"])
    if "paths" in out:
        line["paths"] = {}
        for k, v in out["paths"].items():
            if isinstance(v, dict):
                line["paths"][k] = _pick(v, ("ms_per_step", "mfma_frac", "hbm_frac_on_algorithmic_bytes"))
    # CQT84, the other half of the metric: ONE headline block, the module as it ships (default_module: true).  The opt-in f16x3
    # arithmetic (strip kernel: untouched since round 2, 0.27 useful of its pipe) is no headline any more: its
    # time stays under extra.cqt_f16x3, its full block in bench_detail.json (roofline_cqt84_f16x3)
    if "roofline_cqt84" in out:
        line["roofline_cqt84"] = _pick(out["roofline_cqt84"], ("precision", "default_module", "ms_per_step", "frames_per_s", "bound", "achieved", "peak",
                                                               "unit", "frac", "algorithmic_frac", "traffic", "same_bits_as_torch_conv1d", "torch_conv1d_ms"))
    if "extra" in out:
        line["extra"] = {}
        for k, v in out["extra"].items():
            if not isinstance(v, dict):
                continue
            if "error" in v:
                line["extra"][k] = {"error": str(v["error"])[:60]}
                continue
            e = _pick(v, ("ms_per_step",))
            blk = v.get("roofline") or {}
            e.update(_pick(blk, ("frac", "traffic")))
            if blk.get("bound"):
                e["bound"] = blk["bound"]
            if not blk:  # (records priced in place: the training step)
                e.update(_pick(v, ("frac", "bound", "forward_only_ms", "precision")))
            line["extra"][k] = e
    if "gather" in out:
        g = out["gather"]
        line["gather"] = ({"error": str(g["error"])[:60]} if "error" in g else
                          {k: _pick(v, ("with_gather_ms_per_step", "without_gather_ms_per_step", "bytes_per_rank"))
                           if isinstance(v, dict) else _r(v) for k, v in g.items() if k != "what"})
    if isinstance(out.get("reference_ops_on_this_gpu"), dict):
        line["reference_ops_on_this_gpu"] = _pick(out["reference_ops_on_this_gpu"], ("ms_per_step", "value", "unit", "max_diff_of_peak", "error"))
        for key in ("mel_cfg3", "cqt2010_cfg5_shard"):
            if isinstance(out["reference_ops_on_this_gpu"].get(key), dict):
                line["reference_ops_on_this_gpu"][key] = _pick(out["reference_ops_on_this_gpu"][key], ("ms_per_step", "max_diff_of_peak", "error"))
    cb = out.get("cpu_baseline")
    if cb:
        c = _pick(cb, ("value", "unit", "cores", "kind"))
        c.setdefault("value", None)
        c.setdefault("cores", None)
        c["sample"] = (cb.get("sample") or "")[:100]
        for sub in ("numpy_port", "librosa_equivalent", "cqt84"):
            if isinstance(cb.get(sub), dict) and "value" in cb[sub]:
                c[sub] = {"value": _r(cb[sub]["value"])}
        line["cpu_baseline"] = c
    for k in ("kernel_source_sha", "detail", "detail_sha16"):
        if k in out:
            line[k] = out[k]
    # last resort, in order: drop what is least part of the contract until the line fits
    for victim in ("gather", "extra", "paths"):
        if len(json.dumps(line)) <= LINE_BUDGET:
            break
        if victim in line:
            line[victim] = {"see": DETAIL_FILE}
    return line


def emit(out, detail_dir=None):
    """Write the full record to the side file, print the compact line LAST on stdout."""
    detail_dir = detail_dir or os.environ.get("MISPEC_BENCH_DETAIL_DIR") or ROOT
    blob = json.dumps(out, indent=1, sort_keys=True)
    path = os.path.join(detail_dir, DETAIL_FILE if out.get("n_gpus", 1) == 1
                        else "bench_detail_n%d.json" % out["n_gpus"])
    try:
        with open(path, "w") as f:
            f.write(blob)
        out = dict(out, detail=os.path.relpath(path, ROOT), detail_sha16=hashlib.sha256(blob.encode()).hexdigest()[:16])
    except OSError as e:
        log("bench detail file not written: %r" % (e,))
    line = json.dumps(compact_line(out), separators=(",", ":"))
    sys.stderr.flush()
    print(line, flush=True)
    return line


def self_launch(args):
    """``python bench.py --gpus N`` outside torch.distributed.run: start N ranks (one per GPU, RCCL)
    of this script with the same arguments and relay rank 0's JSON line."""
    import socket

    n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if n_dev < args.gpus:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible" % (args.gpus, n_dev))
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    raise SystemExit(subprocess.run(cmd, env=env).returncode)


def parse_args(argv=None):
    """The command line.  --extras, --cpu-baseline and --traffic default to what --full says: all on with it,
    all off without it; given explicitly, they hold either way."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--workload", default="stft", choices=["stft", "stft4096", "mel", "gammatone", "cqt", "cqt2010", "vqt", "mfcc", "istft"])
    ap.add_argument("--full", action="store_true",
                    help="measure more than the headline (minutes): the dominant kernel timed alone, the reference's "
                         "operator sequence on this GPU, and by default the extras, live traffic and the CPU baseline; "
                         "without it the run sets up, warms up, times the steps and prints the line")
    ap.add_argument("--extras", type=int, default=None,
                    help="also time the other arithmetics, CQT84, Mel cfg3, Gammatonegram, the cfg5 shard and the gather "
                         "(default: 1 with --full, else 0)")
    ap.add_argument("--cpu-baseline", type=int, default=None, help="(default: 1 with --full, else 0)")
    ap.add_argument("--prewarm-ms", type=float, default=300.0,
                    help="untimed start-up work before the warm-up steps (GPU out of its idle clocks)")
    ap.add_argument("--precision", default="auto", choices=["auto"] + list(PRECISIONS),
                    help="arithmetic of every timed module; auto = each module's own default (STFT family "
                         "f16x3, the CQT modules fp32; CQT84 is additionally reported in f16x3 and bf16x3)")
    ap.add_argument("--traffic", default=None, choices=["live", "off"],
                    help="live: rocprofv3 PMC passes over a child process (N=1 only); off: null "
                         "(default: live with --full, else off)")
    ap.add_argument("--pmc-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one returned (rank 0) as DIR/<workload>.npy: "
                         "float32, at most 64 MB, a fixed seeded sample of a larger output (see dump_outputs)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.extras is None:
        args.extras = int(args.full)
    if args.cpu_baseline is None:
        args.cpu_baseline = int(args.full)
    if args.traffic is None:
        args.traffic = "live" if args.full else "off"
    return args


def main():
    args = parse_args()
    forced = None if args.precision == "auto" else args.precision

    if args.pmc_child:
        pmc_child(args.pmc_child, forced, args.steps)
        return

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        self_launch(args)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d inside a torch.distributed job of %d ranks" % (args.gpus, world))
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (no CPU fallback)")
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    import nnaudio_amd
    from nnaudio_amd import engine

    module, make_input, meta = workload(args.workload, device)
    x = make_input(rank)

    def max_over_ranks(*vals):
        t = torch.tensor(vals, dtype=torch.float64, device=device)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return [float(v) for v in t]

    def run_path(mod, xin, me, precision, steps, warmup, fft=True, keep_last=None):
        """Time `steps` forwards in one arithmetic; whole-job numbers (max over ranks).  precision "fft": the
        module as it ships (STFT: the FFT path); otherwise the contraction kernels in that arithmetic.
        keep_last: a list that receives what the last timed step returned."""
        nnaudio_amd.set_precision(None if precision == "fft" else precision)
        old_fft = engine.set_fft(fft)
        try:
            wall, dev_s, last = timed_steps(mod, xin, steps, warmup, sync, keep_last=True)
            if keep_last is not None:
                keep_last.append(last)
            del last
        finally:
            engine.set_fft(old_fft)
        nnaudio_amd.set_precision(forced)
        wall, dev_s = max_over_ranks(wall, dev_s)
        per = dev_s / steps
        res = {"frames_per_s": me["frames"] * world * steps / wall, "ms_per_step": wall / steps * 1e3,
               "step_device_ms": per * 1e3,
               "algorithmic_tflops": me["flops"] / per / 1e12,
               "algorithmic_frac": None if precision == "fft" else me["flops"] / per / PEAK[precision],
               "hbm_frac_on_algorithmic_bytes": me["bytes"] / per / PEAK_HBM}
        ex = None if precision == "fft" else executed_flops(me, precision)
        if ex:
            res["executed_mfma_tflops"] = ex / per / 1e12
            res["mfma_frac"] = ex / per / RAW_PEAK[precision]  # executed flops / raw MFMA peak: <= 1
        return wall, dev_s, res

    def dominant_kernel(precision):
        """STFT: the main contraction alone (1024 of the 1025 bins: whole row blocks; the Nyquist
        bin rides in the pre-pass or in tail tiles), with its pre-pass, events on the launch stream."""
        if precision == "fft":  # the whole step is ONE kernel: stft_fft_kernel
            prep = engine.prepare_basis(module.wcos, module.wsin, "fp32", hop=512)

            class _F:
                def __call__(self, _):
                    return engine.framed_gemm(x, module.wcos, module.wsin, hop=512, pad=1024, pad_mode=engine.PAD_REFLECT,
                                              epilogue=engine.EPI_MAGNITUDE, precision="fp32", fft=True, **prep)

            _, d = timed_steps(_F(), x, args.steps, 2, sync)
            per = d / args.steps
            return {"name": "stft_fft_kernel<1024, 1, false> (M = n_fft / 2, MISPEC_EPI_MAGNITUDE, no filterbank: fp32 radix-16/16/4 FFT of every frame on the "
                            "vector ALUs, one wave per frame, tile transposed through LDS)",
                    "avg_ms": per * 1e3, "algorithmic_bytes": meta["bytes"],
                    "achieved_GBps": meta["bytes"] / per / 1e9, "frac_of_hbm_peak": meta["bytes"] / per / PEAK_HBM}
        wc, ws = module.wcos[:1024], module.wsin[:1024]
        prep = engine.prepare_basis(wc, ws, precision, hop=512)

        class _M:
            def __call__(self, _):
                return engine.framed_gemm(x, wc, ws, hop=512, pad=1024, pad_mode=engine.PAD_REFLECT,
                                          epilogue=engine.EPI_MAGNITUDE, precision=precision, fft=False, **prep)

        _, d = timed_steps(_M(), x, args.steps, 2, sync)
        fl = 2.0 * 2048 * 2048 * meta["frames"]
        per = d / args.steps
        bins, taps = fold_geometry(1024, 2048, False)
        ex = 2.0 * (2 * bins) * taps * ((meta["frames"] + 127) // 128 * 128) * MFMAS_PER_PRODUCT[precision]
        return {"name": engine.describe_framed_kernel(precision, prep), "avg_ms": per * 1e3,
                "algorithmic_flops": fl, "algorithmic_tflops": fl / per / 1e12,
                "algorithmic_frac": fl / per / PEAK[precision],
                "executed_flops": ex, "executed_tflops": ex / per / 1e12, "frac_of_raw_mfma_peak": ex / per / RAW_PEAK[precision]}

    prec = module_precision(args.workload, forced)
    # the STFT as it ships runs the FFT path whatever the precision setting (fp32 arithmetic); a forced
    # --precision or MISPEC_FFT=0 benchmarks the contraction kernels instead
    use_fft = prec == "fft"
    if use_fft:
        meta["bound"] = "hbm"
    nnaudio_amd.set_precision(forced)
    prewarm_ms = prewarm(module, x, args.prewarm_ms)
    last = [] if args.dump_outputs else None
    wall, dev_s, primary = run_path(module, x, meta, prec, args.steps, args.warmup, fft=use_fft, keep_last=last)
    dumped = None
    if last is not None:
        if rank == 0:  # (rank 0's clips are make_input(0): the same as at N = 1)
            dumped = dump_outputs(last[0], args.dump_outputs, args.workload)
            log("dump-outputs: %s -> %s" % (dumped, args.dump_outputs))
        del last
    paths = {prec: primary}
    dominant = None
    if args.full and args.workload == "stft":
        dominant = dominant_kernel(prec)
    if args.extras and args.workload == "stft":
        for other in PRECISIONS:
            if other == prec:
                continue
            _, _, paths[other] = run_path(module, x, meta, other, max(3, args.steps // 2), 2, fft=False)
            paths[other]["dominant_kernel"] = dominant_kernel(other)
            paths[other]["what"] = "contraction kernels (FFT path switched off), " + other
        for pr in paths:  # what each arithmetic leaves in silent bins, relative to the peak
            try:
                old_fft = engine.set_fft(pr == "fft")
                try:
                    paths[pr]["dynamic_range_db"] = dynamic_range_db(device, None if pr == "fft" else pr)
                finally:
                    engine.set_fft(old_fft)
            except Exception as e:
                paths[pr]["dynamic_range_db"] = None
                log("dynamic range (%s): %r" % (pr, e))

    frames_total = meta["frames"] * world * args.steps
    kern_s = dev_s / args.steps
    src_sha = kernel_source_sha()
    what = {"f16x3": "f16x3: fp32 operands scaled by powers of two and split into fp16 hi+lo, 3 f16 MFMAs per "
                     "product, fp32 accumulate (err ~1e-7 of peak: fp32 class); the STFT module's default",
            "bf16x3": "bf16x3: fp32 operands split into bf16 hi+lo, 3 bf16 MFMAs per product, fp32 accumulate "
                      "(err ~5e-6 of peak, 1e-4 parity bar)",
            "fp32": "fp32 MFMA, fp32 accumulate",
            "fft": "fp32 FFT of every windowed frame (radix 16 x 16 x 4 complex FFT of 1024 points + real-input "
                   "post-processing on the vector ALUs; err ~2e-7 of peak); what STFT runs when its kernels are "
                   "window x DFT (freq_scale='no', not trainable, n_fft 256 ... 2048)"}[prec]
    out = {
        "metric": "spectrogram frames/sec",
        "value": frames_total / wall,
        "unit": "frames/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": wall / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32" if prec in ("fp32", "fft") else prec,
        "data": "synthetic",
        "prewarm_ms": prewarm_ms,
        "kernel_source_sha": src_sha,
        "dynamic_range_db": paths[prec].get("dynamic_range_db"),
        "config": {"workload": meta["tag"], "global_batch": meta["B"] * world,
                   "clip_samples": meta["L"], "frames_per_clip": meta["T"],
                   "precision": what,
                   "precision_short": {"fft": "fp32 FFT per frame (VALU), err ~2e-7 of peak",
                                       "f16x3": "split fp16 hi+lo, 3 f16 MFMAs per product, fp32 accumulate",
                                       "bf16x3": "split bf16 hi+lo, 3 bf16 MFMAs per product, fp32 accumulate",
                                       "fp32": "fp32 MFMA, fp32 accumulate"}[prec],
                   "parallelism": "batch-sharded x%d, no data-path collective" % world},
        "roofline": roofline_block(
            meta, kern_s, prec,
            kernel=("one step = ONE launch of stft_fft_kernel (fp32 FFT per frame, no pre-pass, no workspace); achieved = "
                    "algorithmic bytes (clips in + spectrogram out + the reference's two bases, SURVEY 8d; the 16.8 MB of "
                    "bases are counted but never read by this kernel: on the 339 MB it moves the fraction is 0.95 x this) / step "
                    "device time against the 8 TB/s HBM peak; the matrix-pipe rooflines of the contraction kernels are under paths")
            if prec == "fft" else
                   "one step = pre-pass + main contraction; achieved = EXECUTED MFMA flops (the folded kernels run "
                   "a quarter of the dense taps, x 3 MFMAs per product for the split arithmetics) / step device "
                   "time; peak = raw dense MFMA peak of the instruction"),
        "paths": paths,
    }
    if dumped is not None:
        out["dump_outputs"] = {"dir": args.dump_outputs, "arrays": dumped,
                               "what": "the last timed step's output, rank 0; *_index: sampled flat positions"}
    out["roofline"]["dominant_kernel"] = dominant

    extra = {}
    traffic_jobs = [(args.workload, forced, out, "roofline")]
    if args.extras:
        del x
        torch.cuda.empty_cache()
        n2 = max(20, args.steps)  # every extra under the headline's rules: pre-warm + >= 20 steps
        jobs = [("cqt", None, None), ("cqt", "f16x3", None), ("cqt", "bf16x3", None),
                ("mel", None, None), ("gammatone", None, None), ("cqt2010", None, None), ("vqt", None, None),
                ("cqt2010", "bf16x3", None), ("cqt2010", "fp32", None),
                ("mel", "f16x3", None), ("gammatone", "f16x3", None),  # (the contraction kernels, FFT off)
                ("mfcc", None, None), ("istft", None, None), ("stft4096", None, None)]
        if world > 1:
            # N > 1: the per-GPU numbers above are the N = 1 line's business (every rank would repeat them, each with
            # its barriers and reductions: minutes of wall time and thirteen more places for one rank to fall out of
            # step with the others); what N ranks add is cfg4's real shard (128 clips over 8 ranks) and the gathers below
            jobs = [("cqt", "f16x3", 16)]
        for name, pr2, b2 in jobs:
            if name == args.workload:
                continue
            key = name if pr2 is None else ("%s_%s" % (name, pr2) + ("_cfg4_shard" if b2 else ""))
            try:
                pr = pr2 or module_precision(name, forced)
                m2, mk2, me2 = workload(name, device, B=b2)
                m2.precision = pr2  # (None: the module's default / the process-wide override)
                if pr == "fft":  # one streaming kernel (filterbank reduced in its tile): priced on bytes
                    me2["bound"] = "hbm"
                x2 = mk2(100 + rank)
                prewarm(m2, x2, args.prewarm_ms)
                w2, d2, r2 = run_path(m2, x2, me2, pr, n2, max(5, args.warmup // 2), fft=pr == "fft")
                blk = roofline_block(me2, d2 / n2, pr)
                if name == "gammatone" and pr == "fft":
                    # ("hbm" describes the first of the step's two launches only)
                    blk["bound_note"] = ("two launches: the FFT kernel writes the power spectrogram frame-major (priced on bytes: "
                                         "this block), then the dense 64 x 1025 filterbank is an fp32 MFMA contraction over a frame's "
                                         "bins -- 2*64*1025 flop per frame, MFMA-bound (~0.082 ms = 0.56 of the fp32 matrix peak; "
                                         "profiles/r06/rocprofv3_gammatone_frame_major_kernel_stats.csv)")
                    blk["second_launch_mfma_flops"] = 2.0 * 64 * 1025 * me2["frames"]
                r2.update(workload=me2["tag"], precision=pr, steps=n2, roofline=blk)
                extra[key] = r2
                if name == "cqt" and not b2 and (pr2 is None or pr2 == "f16x3"):
                    # CQT84 is the other half of BASELINE.json's metric.  roofline_cqt84 is the module AS IT SHIPS
                    # (default precision: fp32 = one float32 FMA chain over the taps per output, bit-identical to torch's
                    # conv1d on this MI355X; the reference's six CQT1992v2 fixture assertions pass verbatim, f16x3 misses
                    # 2.7 % of the log-magnitude one: tests/test_reference_order.py); roofline_cqt84_f16x3 is the opt-in
                    # `module.precision = "f16x3"` (4.7e-7 of the peak against float64: inside north_star's 1e-4).
                    default = pr2 is None
                    blk["kernel"] = (("one step = ONE launch of cqt_chain_kernel (round 6: fp32 16x16x4 MFMA tiles, supports per 8 bins, taps ascending = the reference's "
                                      "FMA chain; the frames' samples in LDS delay lines refilled by LDS-DMA, the bank streamed through LDS as MFMA "
                                      "fragments; 4 multiplying + 4 loading waves per workgroup; no pre-pass, no workspace); "
                                      if pr == "fp32" else
                                      "one step = clip absmax + split pre-passes + framed_%s_strip_kernel; " % pr) +
                                     "achieved = executed MFMA flops (row tiles over the tap range of their longest bin) / "
                                     "step device time; algorithmic = useful (support-aware) flops 2*2*sum(lenghts) per frame")
                    key84 = "roofline_cqt84" if default else "roofline_cqt84_f16x3"
                    out[key84] = dict(blk, workload=me2["tag"], precision=pr, default_module=default,
                                      frames_per_s=r2["frames_per_s"], ms_per_step=r2["ms_per_step"], steps=n2)
                    if default:
                        # measured here, on this run's module: the fraction of its complex output (one clip) that has the
                        # SAME BITS as the reference's own operator sequence on this GPU -- reflect pad + F.conv1d with the
                        # module's kernels (cqt.py:740-772; MIOpen's fp32 FMA chain over the taps)
                        try:
                            # (the WHOLE bench batch: also what the reference's own GPU path costs on this device)
                            same, ref_ms = same_bits_as_conv1d(m2, x2, timed=True)
                            out[key84]["same_bits_as_torch_conv1d"], out[key84]["torch_conv1d_ms"] = same, ref_ms
                        except Exception as e:
                            out[key84]["same_bits_as_torch_conv1d"] = repr(e)[:80]
                    traffic_jobs.append(("cqt", pr2, out, key84))
                elif pr2 is None and name != "istft":  # (its input is made by a forward STFT inside the profiled process)
                    traffic_jobs.append((name, forced, extra[key], "roofline"))
                del m2, x2
                torch.cuda.empty_cache()
            except Exception as e:  # extras must never take the primary number down
                extra[key] = {"error": repr(e)}
        if world == 1 and args.workload == "stft":
            # A TRAINING step: nnAudio's selling point is trainable bases (stft.py:238-242).  STFT(trainable=True) on cfg2's
            # batch, Magnitude, loss.backward(): forward on the dense contraction kernels (trained kernels are not window x
            # DFT: no FFT route, no folds) + the epilogue adjoint + the d-basis contraction (frames x output); x needs no grad.
            for tkey, tprec in (("stft_trainable_fwd_bwd", None), ("stft_trainable_fwd_bwd_fp32", "fp32")):
                try:
                    from nnaudio_amd import features

                    mt = features.STFT(n_fft=2048, hop_length=512, window="hann", output_format="Magnitude", trainable=True,
                                       verbose=False).to(device)
                    mt.precision = tprec
                    xt = make_input(200 + rank)
                    nt = max(5, min(20, args.steps // 10))

                    def train_step():
                        mt.zero_grad(set_to_none=True)
                        mt(xt).mean().backward()

                    for _ in range(3):
                        train_step()
                    sync()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0 = time.perf_counter()
                    e0.record()
                    for _ in range(nt):
                        train_step()
                    e1.record()
                    sync()
                    wt, dt = time.perf_counter() - t0, e0.elapsed_time(e1) * 1e-3
                    with torch.no_grad():
                        t_fwd = timed_steps(mt, xt, nt, 2, sync)[1] / nt
                    fl = 2.0 * meta["flops"]  # forward + d basis, each the dense contraction (2 flop per tap)
                    pr_t = tprec or "f16x3"  # (the STFT module's default arithmetic on the contraction route)
                    extra[tkey] = {"ms_per_step": wt / nt * 1e3, "step_device_ms": dt / nt * 1e3, "forward_only_ms": t_fwd * 1e3,
                                   "steps": nt, "frames_per_s": meta["frames"] * nt / wt, "precision": pr_t,
                                   "algorithmic_flops": fl, "algorithmic_tflops": fl / (dt / nt) / 1e12,
                                   "frac": fl / (dt / nt) / PEAK[pr_t], "bound": "mfma",
                                   "what": "STFT(trainable=True) cfg2 batch, Magnitude: zero_grad + forward + mean().backward() "
                                           "(d wsin, d wcos); algorithmic flops = forward + d-basis contraction, dense, against the "
                                           "fp32-equivalent MFMA peak of the arithmetic"}
                    del mt, xt
                    torch.cuda.empty_cache()
                except Exception as e:
                    extra[tkey] = {"error": repr(e)}
        out["extra"] = extra

    # output reassembly over xGMI (RCCL all-gather), outside the reported value: the step with the
    # in-place gather (kernels write into this rank's slice of a persistent gather buffer) vs without
    if world > 1 and args.extras:
        try:
            from nnaudio_amd import dist as D

            x = make_input(rank)
            sm = D.ShardedModule(module)
            B = meta["B"]
            # ShardedModule slices [lo, hi) out of a (B * world, L) batch: only this rank's block
            # of that tensor is ever filled
            full_in = torch.empty((B * world, meta["L"]), dtype=torch.float32, device=device)
            lo, hi = D.shard_bounds(B * world, world, rank)
            full_in[lo:hi].copy_(x)
            n3 = max(5, args.steps // 4)
            wg, dg = timed_steps(sm, full_in, n3, 3, sync)
            wg, dg = max_over_ranks(wg, dg)
            with torch.no_grad():
                y_bytes = sm(full_in)[lo:hi].numel() * 4.0
            out["gather"] = {"with_gather_ms_per_step": wg / n3 * 1e3,
                             "without_gather_ms_per_step": wall / args.steps * 1e3,
                             "frames_per_s_with_gather": meta["frames"] * world * n3 / wg,
                             "bytes_per_rank": y_bytes,
                             "what": "in-place all_gather_into_tensor of the full output tensor; every "
                                     "rank's block is written by the kernels into its slice of a "
                                     "persistent gather buffer (nnaudio_amd.dist.ShardedModule)"}
            del full_in
            # the same for the shards the reference's multi-GPU configs name: cfg4 (CQT1992v2, 128 clips over 8
            # ranks = 16 per rank) and cfg5 (CQT2010v2, 512 clips over 8 ranks = 64 per rank; per-rank work
            # fixed as N grows, like the headline)
            def all_ranks_ok(ok):
                """One rank failing while the others enter a collective is a hang, not an error record: agree first."""
                t = torch.tensor([1.0 if ok else 0.0], dtype=torch.float64, device=device)
                dist.all_reduce(t, op=dist.ReduceOp.MIN)
                return bool(t.item() > 0.5)

            for key, name, pr2, b2 in (("cqt_cfg4_shard", "cqt", "f16x3", 16), ("cqt2010_cfg5_shard", "cqt2010", None, None)):
                # rank-local part (construction, allocation, the un-gathered timing's kernels) under try; every collective
                # (max_over_ranks, the sharded module's all-gather) only after all ranks have said they got this far
                err, st = None, {}
                try:
                    m2, mk2, me2 = workload(name, device, B=b2)
                    m2.precision = pr2
                    x2 = mk2(100 + rank)
                    B2 = x2.shape[0]
                    full2 = torch.empty((B2 * world, x2.shape[1]), dtype=torch.float32, device=device)
                    lo2, hi2 = D.shard_bounds(B2 * world, world, rank)
                    full2[lo2:hi2].copy_(x2)
                    sm2 = D.ShardedModule(m2)
                    with torch.no_grad():
                        m2(x2)  # (builds the cached operands; any unsupported-shape error shows here, on this rank alone)
                    torch.cuda.synchronize()
                    st = dict(m2=m2, x2=x2, full2=full2, sm2=sm2, me2=me2, lo2=lo2, hi2=hi2)
                except Exception as e:
                    err = repr(e)[:200]
                if not all_ranks_ok(err is None):
                    out["gather"][key] = {"error": err or "another rank failed before the collectives"}
                    st.clear()
                    torch.cuda.empty_cache()
                    continue
                m2, x2, full2, sm2, me2, lo2, hi2 = (st[k] for k in ("m2", "x2", "full2", "sm2", "me2", "lo2", "hi2"))
                w0, d0 = timed_steps(m2, x2, n3, 3, sync)
                w0, d0 = max_over_ranks(w0, d0)
                w1, d1 = timed_steps(sm2, full2, n3, 3, sync)
                w1, d1 = max_over_ranks(w1, d1)
                with torch.no_grad():
                    yb = sm2(full2)[lo2:hi2].numel() * 4.0
                out["gather"][key] = {"with_gather_ms_per_step": w1 / n3 * 1e3, "without_gather_ms_per_step": w0 / n3 * 1e3,
                                      "frames_per_s_with_gather": me2["frames"] * world * n3 / w1, "bytes_per_rank": yb,
                                      "workload": me2["tag"]}
                del m2, sm2, x2, full2
                st.clear()
                torch.cuda.empty_cache()
        except Exception as e:
            out["gather"] = {"error": repr(e)}

    if rank == 0 and world == 1 and args.traffic == "live":
        torch.cuda.empty_cache()
        for name, pr, holder, key in traffic_jobs:
            if key not in holder:
                continue
            blk = holder[key]
            try:
                t = measure_traffic(name, pr)
                blk["traffic"] = t["bytes_per_step"]
                blk["traffic_detail"] = {k: t[k] for k in ("fetch_bytes", "write_bytes", "per_kernel", "method")}
                if t.get("mfma_flops") and blk.get("bound") == "mfma":
                    # the counted MFMA flops replace the tiling model behind achieved / frac
                    per = blk["step_device_ms"] * 1e-3
                    raw = RAW_PEAK[module_precision(name, pr)]
                    blk.update(executed_flops_per_launch=t["mfma_flops"], executed_source="pmc",
                               executed_mfma_tflops=t["mfma_flops"] / per / 1e12,
                               executed_frac_of_raw_mfma_peak=t["mfma_flops"] / per / raw,
                               executed_by_instruction=t["mfma_flops_by_type"],
                               achieved=t["mfma_flops"] / per / 1e12, peak=raw / 1e12,
                               frac=min(1.0, t["mfma_flops"] / per / raw))
            except Exception as e:
                blk["traffic"] = None
                blk["traffic_detail"] = {"error": repr(e)[:300]}

    if args.full and rank == 0 and world == 1 and args.workload == "stft":
        try:  # the reference's operator sequence on THIS device (torch / MIOpen), beside the CPU one below
            out["reference_ops_on_this_gpu"] = reference_ops_on_gpu(make_input(300))
            torch.cuda.empty_cache()
        except Exception as e:
            out["reference_ops_on_this_gpu"] = {"error": repr(e)[:80]}
        if args.extras:  # ... and for configs[2] and one rank's shard of configs[4] (VERDICT r5 "missing" 5)
            for key, fn in (("mel_cfg3", reference_ops_mel_on_gpu), ("cqt2010_cfg5_shard", reference_ops_cqt2010_on_gpu)):
                try:
                    out["reference_ops_on_this_gpu"][key] = fn(device)
                except Exception as e:
                    out["reference_ops_on_this_gpu"][key] = {"error": repr(e)[:80]}
                torch.cuda.empty_cache()
    if rank == 0 and world == 1 and args.cpu_baseline:
        try:
            out["cpu_baseline"] = cpu_baseline()
        except Exception as e:
            out["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": os.cpu_count(),
                                   "kind": "port", "sample": "failed: %r" % (e,)}
    elif rank == 0 and args.cpu_baseline:
        out["cpu_baseline"] = {"value": None, "unit": "frames/s", "cores": None, "kind": "port",
                               "sample": "measured at N=1 only"}

    if rank == 0:
        emit(out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
