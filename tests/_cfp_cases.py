"""Access to the CFP fixtures (tests/golden/cfp_cases.json + one cfp_<case>.npz per case, written by
scripts/gen_cfp_golden.py from runs of the reference) and the tolerance rule both CFP suites apply:

    err(ours vs reference-float64)  <=  4 x err(reference-float32 vs reference-float64)      for max and for RMS,

per case and output tensor, over ALL elements, the right-hand side read from the fixture; where it is 0 (the all-zeros
input) ours must be exactly equal.  The factor 4 is the room for another correct fp32 FFT (a different factorisation and
summation order draws an independent error of the same size; the max over 1e4 - 1e5 elements is a tail statistic)."""
import json
import os

import numpy as np

from tests import _cfp_oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ("Z", "tfrL0", "tfrLF", "tfrLQ")
FACTOR = 4.0

with open(os.path.join(GOLDEN, "cfp_cases.json")) as _f:
    CASES = json.load(_f)
CASE_NAMES = sorted(CASES)


def load(name):
    return np.load(os.path.join(GOLDEN, CASES[name]["file"]))


def build(name, device="cpu"):
    """The module of a case (this library's) and its input as a float32 torch tensor."""
    import torch

    from nnaudio_amd import features

    rec = CASES[name]
    m = getattr(features, rec["class"])(**rec["kwargs"]).to(device)
    return m, torch.from_numpy(load(name)["x"]).to(device)


def as_tuple(y):
    return tuple(y) if isinstance(y, (tuple, list)) else (y,)


def check_rule(name, outputs, report=None):
    """Assert the rule for every output tensor of a case; prints each figure before asserting.  Returns the ratios."""
    rec, data = CASES[name], load(name)
    outputs = as_tuple(outputs)
    assert len(outputs) == len(rec["ref_f32_error"])
    ratios, failed = {}, []
    for n, got in zip(NAMES, outputs):
        want = data["out_" + n]
        got = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
        assert got.shape == want.shape, (name, n, got.shape, want.shape)
        assert got.dtype == np.float32, (name, n, got.dtype)
        e_max, e_rms = _cfp_oracle.errors(got, want)
        ref = rec["ref_f32_error"][n]
        line = "%s %s: max %.3e (reference f32 %.3e) rms %.3e (reference f32 %.3e) peak %.3e" % (
            name, n, e_max, ref["max"], e_rms, ref["rms"], ref["peak"])
        print(line)
        if report is not None:
            report.append(line)
        if ref["max"] == 0.0:
            if not np.array_equal(got, want.astype(np.float32)):
                failed.append(line)
            ratios[n] = (0.0, 0.0)
            continue
        ratios[n] = (e_max / ref["max"], e_rms / ref["rms"])
        if not (e_max <= FACTOR * ref["max"] and e_rms <= FACTOR * ref["rms"]):
            failed.append(line)
    assert not failed, "\n".join(failed)
    return ratios
