"""features.PCEN at 64 spectrograms of 862 frames (20 s at 22.05 kHz, hop 512): mel-sized (64, 128, 862) and STFT-sized
(64, 1025, 862) -- the kernel route (csrc/pcen.hip: one wave per row scans the recurrence) against the composition route
(a loop of torch operators over the frames on the same device; as it ships, float64 steps, and in float32), the forward
alone and forward plus backward (input and the four parameters require grad), alternated and warmed up; ms per call
(torch events; medians of the rounds), the bytes the kernels must move and their share of the HBM rate.
``--kernel-only`` runs the kernel route alone (for a profiler)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnaudio_amd import engine, features  # noqa: E402

SHAPES = ((64, 128, 862), (64, 1025, 862))
ROUNDS, REPS = 5, 3
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12  # bytes / s: a float4 copy on the MI355X; the data sheet


def main():
    kernel_only = "--kernel-only" in sys.argv
    dev = torch.device("cuda")
    torch.manual_seed(0)
    for shape in SHAPES:
        S = torch.randn(shape, device=dev) ** 2
        G = torch.randn(shape, device=dev)
        m = features.PCEN(n_bins=shape[1], trainable=True).to(dev)
        params = (m.b, m.gain, m.bias, m.power)
        n = S.numel()
        # the bytes the kernels must move: forward S in, out; grad-mode forward also M (float64); backward S, M, G in, dS out
        nbytes = {"forward": 8 * n, "forward+backward": (4 + 4 + 8) * n + (4 + 8 + 4 + 4) * n}

        def forward(route, dtype=None):
            def run():
                engine.set_pcen_kernel(route == "kernel")
                with torch.no_grad():
                    if dtype is not None:
                        return engine.pcen_composition(S, *params, m.eps, dtype=dtype)[0]
                    return m(S)
            return run

        def both(route, dtype=None):
            x = S.clone().requires_grad_(True)

            def run():
                engine.set_pcen_kernel(route == "kernel")
                x.grad = None
                m.zero_grad(set_to_none=True)
                out = engine.pcen_composition(x, *params, m.eps, dtype=dtype)[0] if dtype is not None else m(x)
                out.backward(G)
                return x.grad
            return run

        runs = {("forward", "kernel"): forward("kernel"), ("forward+backward", "kernel"): both("kernel")}
        if not kernel_only:
            runs.update({("forward", "composition"): forward("composition"),
                         ("forward", "composition-f32"): forward("composition", torch.float32),
                         ("forward+backward", "composition"): both("composition"),
                         ("forward+backward", "composition-f32"): both("composition", torch.float32)})
        routes, outs = {}, {}
        for key, fn in runs.items():  # warm-up (and the route each one takes)
            for _ in range(2):
                outs[key] = fn()
            routes[key] = engine.pcen_route() if not key[1].endswith("f32") else "composition"
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for key, fn in runs.items():
                reps = REPS * (10 if key[1] == "kernel" else 1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[key].append(e0.elapsed_time(e1) / reps)
        engine.set_pcen_kernel(True)
        for key in runs:
            ms = statistics.median(times[key])
            line = "%s %-16s %-15s route %-11s %9.4f ms per call (rounds: %s)" % (
                shape, key[0], key[1], routes[key], ms, " ".join("%.3f" % t for t in times[key]))
            if key[1] == "kernel":
                rate = nbytes[key[0]] / (ms * 1e-3)
                line += "  %.1f MB -> %.2f TB/s = %.0f %% of the measured copy rate, %.0f %% of the data sheet's" % (
                    nbytes[key[0]] / 1e6, rate / 1e12, 100 * rate / HBM_MEASURED, 100 * rate / HBM_SPEC)
            print(line, flush=True)
        if not kernel_only:
            for what in ("forward", "forward+backward"):
                d = (outs[(what, "kernel")] - outs[(what, "composition")]).abs().max().item()
                print("%s %s: max |kernel - composition| = %.3e (peak %.3e)"
                      % (shape, what, d, outs[(what, "composition")].abs().max().item()), flush=True)
        del outs, S, G
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
