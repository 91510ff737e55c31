"""Write the CFP fixtures, tests/golden/cfp_<case>.npz + tests/golden/cfp_cases.json, by RUNNING the reference:

    python scripts/gen_cfp_golden.py /path/to/nnAudio/Installation

Nothing of the reference is copied: its package is imported from the path given, ``scipy.signal.blackmanharris`` (which
left scipy in 1.13) is pointed at ``scipy.signal.windows.blackmanharris`` for the run, and per case the script stores
the input, the module's three buffers, the outputs of the reference run in float64 (``module.double()``, ``x.double()``)
and, per output tensor, the max and RMS error of the reference's own float32 run against that float64 run -- the
right-hand side of the tests' tolerance rule (tests/test_cfp_cpu.py).  One file per case keeps every file small.
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden")
NAMES = ("Z", "tfrL0", "tfrLF", "tfrLQ")


def signals(kind, batch, samples, fs, rng):
    t = np.arange(samples) / fs
    if kind == "noise":
        return rng.standard_normal((batch, samples))
    tone = sum(np.sin(2 * np.pi * 220.0 * k * t + k) / k for k in range(1, 9)) / 2
    if kind == "tone":
        return np.stack([tone * (1 - 0.3 * b) for b in range(batch)])
    if kind == "tone+noise":
        return np.stack([tone * (1 - 0.3 * b) for b in range(batch)]) + 1e-3 * rng.standard_normal((batch, samples))
    if kind == "burst":
        x = np.zeros((batch, samples))
        a, b = samples // 3, samples // 3 + samples // 8
        x[:, a:b] = rng.standard_normal((batch, b - a)) * np.hanning(b - a)
        return x
    if kind == "zeros":
        return np.zeros((batch, samples))
    raise ValueError(kind)


# name, class, constructor arguments, signal, batch, samples
CASES = [
    ("cfp_default_noise", "CFP", {}, "noise", 2, 16000),
    ("combined_default_noise", "Combined_Frequency_Periodicity", {}, "noise", 1, 16000),
    ("combined_default_tone", "Combined_Frequency_Periodicity", {}, "tone", 1, 16000),
    ("cfp_tone_noise", "CFP", {}, "tone+noise", 2, 16320),          # T = 52: even
    ("cfp_burst_ragged", "CFP", {}, "burst", 1, 16123),             # samples not a multiple of hop; T = 51: odd
    ("cfp_zeros", "CFP", {}, "zeros", 1, 8000),
    ("combined_g2", "Combined_Frequency_Periodicity", {"g": [0.24, 0.6]}, "noise", 1, 12000),
    ("cfp_g4", "CFP", {"g": [0.24, 0.6, 1, 0.8]}, "tone+noise", 1, 16000),
    ("cfp_g_log", "CFP", {"g": [0.24, 0, 1]}, "noise", 1, 16000),
    ("cfp_fr4", "CFP", {"fr": 4}, "tone+noise", 2, 16000),          # N = 4000
    ("combined_fr1", "Combined_Frequency_Periodicity", {"fr": 1}, "noise", 1, 16000),  # N = 16000
    ("cfp_fr1_tone", "CFP", {"fr": 1}, "tone", 1, 16000),
    ("cfp_fs44100", "CFP", {"fs": 44100, "fc": 20, "tc": 1 / 20000}, "tone+noise", 1, 22050),  # N = 22050: composition
]


def main(ref_path):
    sys.path.insert(0, ref_path)
    import scipy.signal
    import scipy.signal.windows
    import torch

    if not hasattr(scipy.signal, "blackmanharris"):
        scipy.signal.blackmanharris = scipy.signal.windows.blackmanharris
    from nnAudio import features as ref_features

    index = {}
    for i, (name, cls, kw, kind, batch, samples) in enumerate(CASES):
        rng = np.random.default_rng(1000 + i)
        fs = kw.get("fs", 16000)
        x = signals(kind, batch, samples, fs, rng).astype(np.float32)
        with torch.no_grad():
            m = getattr(ref_features, cls)(**kw)
            y32 = m(torch.from_numpy(x))
            y64 = m.double()(torch.from_numpy(x).double())
        if cls == "CFP":
            y32, y64 = (y32,), (y64,)
        m32 = getattr(ref_features, cls)(**kw)
        arrays = {"x": x}
        for k, v in m32.state_dict().items():
            arrays["buf_" + k] = v.numpy()
        rec = {"class": cls, "kwargs": kw, "signal": kind, "file": "cfp_%s.npz" % name, "ref_f32_error": {},
               "attrs": {a: (getattr(m32, a) if not isinstance(getattr(m32, a), (np.integer, np.floating)) else getattr(m32, a).item())
                         for a in ("N", "pad_value", "tc_idx", "fc_idx", "HighFreqIdx", "HighQuefIdx", "window_size", "hop_length")}}
        rec["attrs"]["NumofLayer"] = int(m32.NumofLayer)
        rec["attrs"]["t"] = np.asarray(m.t).tolist()
        arrays["attr_f"] = np.asarray(m32.f)
        arrays["attr_q"] = np.asarray(m32.q)
        for n, a32, a64 in zip(NAMES, y32, y64):
            a64 = a64.numpy()
            assert np.isfinite(a64).all() and a64.dtype == np.float64, name
            d = a32.double().numpy() - a64
            rec["ref_f32_error"][n] = {"max": float(np.abs(d).max()), "rms": float(np.sqrt(np.mean(d * d))),
                                       "peak": float(np.abs(a64).max())}
            arrays["out_" + n] = a64
        path = os.path.join(OUT, rec["file"])
        np.savez_compressed(path, **arrays)
        rec["bytes"] = os.path.getsize(path)
        index[name] = rec
        print(name, {n: "%.2e/%.2e (peak %.2e)" % (e["max"], e["rms"], e["peak"]) for n, e in rec["ref_f32_error"].items()},
              rec["bytes"], flush=True)
    with open(os.path.join(OUT, "cfp_cases.json"), "w") as f:
        json.dump(index, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1])
