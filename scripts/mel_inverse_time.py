"""MelSpectrogram.to_stft at 64 mel spectrograms of 862 frames (20 s at 22.05 kHz, hop 512), 256 steps with momentum:
128 mels / n_fft 2048 (the README's shape: a (64, 1025, 862) spectrum) and 80 mels / n_fft 512 -- the kernel route
(csrc/mel_nnls.hip: all steps of a tile of frames in LDS) against the composition route (two matmuls and the elementwise
steps per iteration on the same device; as it ships, float64, and in float32), alternated and warmed up; ms per call (torch events; medians of the rounds).
``--batch B`` / ``--iters N`` time another batch size / step count, ``--kernel-only`` runs the kernel route alone (for
a profiler)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnaudio_amd import engine, features  # noqa: E402

FRAMES = 862
ROUNDS, REPS = 5, 2


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    batch, n_iter = arg("--batch", 64), arg("--iters", 256)
    kernel_only = "--kernel-only" in sys.argv
    dev = torch.device("cuda")
    torch.manual_seed(0)
    for n_fft, n_mels in ((2048, 128), (512, 80)):
        m = features.MelSpectrogram(sr=22050, n_fft=n_fft, n_mels=n_mels, hop_length=512, verbose=False).to(dev)
        spec = torch.rand(batch, n_fft // 2 + 1, FRAMES, device=dev) ** 4
        mel = torch.matmul(m.mel_basis, spec)
        del spec

        def kernel():
            engine.set_mel_nnls_kernel(True)
            return m.to_stft(mel, n_iter=n_iter)

        def composition():
            engine.set_mel_nnls_kernel(False)
            return m.to_stft(mel, n_iter=n_iter)

        def composition_f32():  # the float32 operator sequence: the yardstick for speed
            engine.set_mel_nnls_kernel(False)
            ops = m._nnls_operands()
            return engine.mel_nnls_composition(mel, m.mel_basis, power=m.power, n_iter=n_iter, momentum=True, L=ops["L"],
                                               dtype=torch.float32)

        runs = {"kernel": kernel} if kernel_only else {"kernel": kernel, "composition": composition,
                                                       "composition-f32": composition_f32}
        routes, outs = {}, {}
        with torch.no_grad():
            for name, fn in runs.items():  # warm-up (and the route each one takes)
                for _ in range(2):
                    outs[name] = fn()
                routes[name] = engine.mel_nnls_route()
            torch.cuda.synchronize()
            times = {k: [] for k in runs}
            for _ in range(ROUNDS):
                for name, fn in runs.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(REPS):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / REPS)
        engine.set_mel_nnls_kernel(True)
        for name in runs:
            ms = statistics.median(times[name])
            print("n_fft=%-4d n_mels=%-3d (%d, %d, %d) n_iter=%d %-15s route %-11s %9.3f ms per call  %7.4f ms per step  (rounds: %s)"
                  % (n_fft, n_mels, batch, n_mels, FRAMES, n_iter, name, routes[name], ms, ms / max(n_iter, 1),
                     " ".join("%.2f" % t for t in times[name])), flush=True)
        if not kernel_only:
            d = (outs["kernel"] - outs["composition"]).abs().max().item()
            res = (torch.matmul(m.mel_basis, outs["kernel"] ** 2) - mel).norm().item() / mel.norm().item()
            print("n_fft=%-4d max |kernel - composition| = %.3e (peak %.3e); || M p - m || / || m || = %.3e"
                  % (n_fft, d, outs["composition"].abs().max().item(), res), flush=True)
        del outs, mel
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
