"""Griffin_Lim at the bench batch (64 x 10 s @ 44.1 kHz, n_fft 2048, hop 512: S is (64, 1025, 862)), n_iter = 32:
the fused route (STFT + phase update in one launch), the separate route (Complex STFT, then the update kernel) and the
torch-native equivalent (torch.stft / torch.istft with return_complex=True + elementwise ops: the reference's algorithm
made to run), alternated and warmed up; ms per call and per iteration (torch events; medians of the rounds)."""
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnaudio_amd import engine, features  # noqa: E402

B, F, T, N, HOP, N_ITER = 64, 1025, 862, 2048, 512, 32
ROUNDS, REPS = 5, 3


def torch_native(S, w, n_iter, momentum=0.99):
    """fast Griffin-Lim on torch's own transforms (same initial draw as the module)"""
    r = torch.randn(S.shape, device=S.device)
    angles = torch.polar(torch.ones_like(r), 2 * math.pi * r)
    beta = momentum / (1 + momentum)
    tprev = torch.zeros_like(angles)
    for _ in range(n_iter):
        y = torch.istft(S * angles, N, HOP, window=w)
        rebuilt = torch.stft(y, N, HOP, window=w, pad_mode="reflect", return_complex=True)
        a = rebuilt - beta * tprev
        angles = a / (a.abs() + 1e-16)
        tprev = rebuilt
    return torch.istft(S * angles, N, HOP, window=w)


def main():
    engine.set_fft(True)
    dev = torch.device("cuda")
    S = torch.rand(B, F, T, device=dev)
    m = features.Griffin_Lim(N, n_iter=N_ITER, hop_length=HOP, device=dev)
    w = m.w.to(dev)

    def fused():
        engine.set_griffin_lim_fused(True)
        return m(S)

    def separate():
        engine.set_griffin_lim_fused(False)
        return m(S)

    def native():
        return torch_native(S, w, N_ITER)

    runs = {"fused": fused, "separate": separate, "torch": native}
    routes = {}
    with torch.no_grad():
        for name, fn in runs.items():  # warm-up (and the route each one takes)
            for _ in range(2):
                fn()
            routes[name] = engine.griffin_lim_route() if name != "torch" else "torch.stft / torch.istft"
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
    engine.set_griffin_lim_fused(True)
    for name in runs:
        ms = statistics.median(times[name])
        print("%-9s %-26s %8.3f ms per call  %6.3f ms per iteration  (rounds: %s)"
              % (name, routes[name], ms, ms / N_ITER, " ".join("%.2f" % t for t in times[name])))


if __name__ == "__main__":
    main()
