"""CFP at 64 clips of 10 s at 16 kHz (hop 320: 501 frames per clip, 32 064 frames), at the default fr = 2 (N = 8000) and at
fr = 1 (N = 16000) and fr = 4 (N = 4000): the kernel route (csrc/cfp.hip: the whole chain of a pair of frames in LDS)
against the composition route (torch.stft / torch.fft / matmul on the same device: the reference's operator sequence),
alternated and warmed up; ms per call (torch events; medians of the rounds).  ``--batch B`` times another batch size,
``--kernel-only`` runs the kernel route alone (for a profiler)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nnaudio_amd import engine, features  # noqa: E402

SAMPLES = 160000
ROUNDS, REPS = 5, 3


def main():
    batch = int(sys.argv[sys.argv.index("--batch") + 1]) if "--batch" in sys.argv else 64
    kernel_only = "--kernel-only" in sys.argv
    dev = torch.device("cuda")
    torch.manual_seed(0)
    x = torch.randn(batch, SAMPLES, device=dev)
    for fr in (2, 1, 4):
        m = features.CFP(fr=fr).to(dev)

        def kernel():
            engine.set_cfp_kernel(True)
            return m(x)

        def composition():
            engine.set_cfp_kernel(False)
            return m(x)

        runs = {"kernel": kernel} if kernel_only else {"kernel": kernel, "composition": composition}
        routes, outs = {}, {}
        with torch.no_grad():
            for name, fn in runs.items():  # warm-up (and the route each one takes)
                for _ in range(2):
                    outs[name] = fn()
                routes[name] = engine.cfp_route()
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
        engine.set_cfp_kernel(True)
        frames = outs["kernel"].shape[0] * outs["kernel"].shape[2]
        for name in runs:
            ms = statistics.median(times[name])
            print("fr=%d N=%-5d %-11s route %-11s %9.3f ms per call  %7.3f us per frame  (rounds: %s)"
                  % (fr, m.N, name, routes[name], ms, 1e3 * ms / frames, " ".join("%.2f" % t for t in times[name])))
        if not kernel_only:
            d = (outs["kernel"] - outs["composition"]).abs().max().item()
            print("fr=%d N=%-5d max |kernel - composition| = %.3e (peak %.3e), %d frames" %
                  (fr, m.N, d, outs["composition"].abs().max().item(), frames))
        del outs
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
