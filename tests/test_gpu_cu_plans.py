"""The launch plans that are sized from the number of compute units, run at other counts than the card's own.

Every site that sizes a launch from the CU count reads it through ``device_cus()`` / ``mispec_device_cus()``
(csrc/mispec.hip), and ``mispec_set_plan_cus`` (``engine.plan_cus``) overrides it.  A small cap makes a
float64-checkable problem run many tiles per persistent workgroup, cross clip boundaries inside a workgroup's run
and take every branch of the fold kernels' rounds rule -- code the card's own count (256) only reaches at bench
sizes.  Each site gets (a) bit identity with the uncapped run where the plan does not reorder any output's sum,
(b) a float64 reference at the tolerance of the existing sweep of that path, (c) evidence that the capped run took
the regime it claims."""
import ctypes

import numpy as np
import pytest
import torch

from tests._golden import assert_parity, assert_phase_parity
from tests.test_gpu_fold2 import BUDGET, _dft_basis
from tests.test_gpu_parity import DEV, _cfg5_sampled_check, _fourier_like_basis, _np_framed

pytestmark = pytest.mark.gpu

# every function of nnaudio_amd/csrc that calls device_cus() / mispec_device_cus(), and the tests below that run
# its plans at other counts (tests/test_abi.py::test_cu_plan_site_table_is_complete keeps this table true)
SITES = {
    "launch_fft_cfg": "test_fft_instances_at_capped_counts, test_fused_mel_at_capped_counts, "
                      "test_frame_major_at_capped_counts",
    "launch_framed_bf16x3": "test_strip_kernels_at_capped_counts (bf16x3)",
    "launch_fold": "test_fold_rounds_rule_at_capped_counts (fold)",
    "launch_fold2": "test_fold_rounds_rule_at_capped_counts (fold2)",
    "route_framed": "test_strip_kernels_at_capped_counts (f16x3, fp32), test_strip_workspace_sized_under_another_count",
    "mispec_istft_frames_fft_f32": "test_inverse_fft_at_capped_counts",
    "mispec_istft_fft_f32": "test_inverse_fft_at_capped_counts",
    "mispec_mfcc_tail_f32": "test_mfcc_tail_at_capped_counts",
    "mispec_octave_pyramid_f32": "test_fused_octave_kernel_at_capped_counts",
    "mispec_octave_stream_f32": "test_octave_stream_default_segments_at_capped_counts, "
                                "test_octave_stream_modules_at_capped_counts",
}

# caps: 1 and 5 give several tiles per workgroup; 37 is not a multiple of 8 (the FFT grids are rounded up to 8);
# 32 is one XCD of a partitioned MI355X; 0 = the device's own count (the run the others are compared with)
CAPS = (1, 5, 32, 37)


def _roundup8(v):
    return (v + 7) // 8 * 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(request):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; torch.cuda.is_available() is False")
    from nnaudio_amd import _abi

    _abi.load()
    n = torch.cuda.get_device_properties(0).multi_processor_count
    tr = request.config.pluginmanager.get_plugin("terminalreporter")
    cm = request.config.pluginmanager.get_plugin("capturemanager")
    if tr is not None and cm is not None:
        with cm.global_and_fixture_disabled():  # (the log shows the count every capped run was compared with)
            tr.write_line("test_gpu_cu_plans: capped plans compared against the device's own count, %d CUs" % n)


@pytest.fixture(autouse=True)
def _plan_cus_reset():
    """no override leaks into or out of a test of this module"""
    from nnaudio_amd import _abi, engine

    assert engine.plan_cus_override() == 0
    yield
    _abi.load().mispec_set_plan_cus(0)


@pytest.fixture
def fft_on():
    """(tests/conftest.py switches the FFT route off for every module but test_gpu_fft)"""
    from nnaudio_amd import engine

    old = engine.set_fft(True)
    yield
    engine.set_fft(old)


def _at_caps(run, caps=CAPS):
    """run() uncapped, then under every cap -> {0: y, cap: y}"""
    from nnaudio_amd import engine

    out = {0: run()}
    for c in caps:
        with engine.plan_cus(c):
            out[c] = run()
    torch.cuda.synchronize()
    return out


def _assert_bit_identical(ys, what):
    for c, y in ys.items():
        assert y.shape == ys[0].shape and torch.equal(y, ys[0]), "%s: cap %d differs from the device's plan, max |d| %.3e" % (
            what, c, float((y.double() - ys[0].double()).abs().max()))


# ---------------------------------------------------------------------------------------------------------------
# FFT path (launch_fft_cfg): persistent grid min(tiles, per_cu x CUs) rounded up to 8; at most 32 frames per tile
# (fft_tile_row, csrc/stft_fft.inl), so B ceil(T / 32) tiles against a grid of at most roundup8(2 cap) workgroups
# ---------------------------------------------------------------------------------------------------------------
B_FFT, T_FFT = 3, 517  # 517 = 16 x 32 + 5: a ragged last tile in every instance; 17 / 33 / 65 tiles per clip do not
                       # divide the per-XCD ranges, so workgroup runs cross clip boundaries


def _fft_problem(K, rng):
    hop = K // 4
    pad = K // 2
    L = (T_FFT - 1) * hop + int(rng.integers(0, hop))  # center=True: L // hop + 1 = T frames, reflect at both ends
    assert L // hop + 1 == T_FFT
    x = rng.standard_normal((B_FFT, L)).astype(np.float32)
    return x, hop, pad


def _rfft_ref(x, w, K, hop, pad, F):
    """float64 windowed frames through np.fft.rfft: for a window x DFT basis the same operation as the
    contraction -- re = sum x w cos, im = -sum x w sin (the _np_framed convention)"""
    from oracle import spectral_oracle as O

    xp = O.pad_signal(x, pad, "reflect").astype(np.float64)
    fr = O.frames(xp, K, hop)  # (B, T, K)
    X = np.fft.rfft(fr * np.asarray(w, np.float64)[None, None, :], axis=-1)[..., :F]
    return np.ascontiguousarray(X.real.transpose(0, 2, 1)), np.ascontiguousarray(X.imag.transpose(0, 2, 1))


def test_fft_problem_has_three_tiles_per_workgroup_at_the_small_caps():
    for c in (1, 5):
        assert B_FFT * -(-T_FFT // 32) >= 3 * _roundup8(2 * c), c


_EPIS = ["complex", "magnitude", "power2", "power1", "phase", "cossin"]


@pytest.mark.parametrize("K,epi", [(K, e) for K in (256, 512, 1024, 2048) for e in _EPIS] +
                         [(4096, e) for e in ("complex", "magnitude", "power2", "phase")])
def test_fft_instances_at_capped_counts(K, epi):
    from nnaudio_amd import engine

    rng = np.random.default_rng(K + len(epi))
    x, hop, pad = _fft_problem(K, rng)
    F = K // 2 + 1
    wr, wi = _dft_basis(F, K, "random", rng)  # (an asymmetric window)
    xd, wrd, wid = (torch.as_tensor(a).to(DEV) for a in (x, wr, wi))
    prep = engine.prepare_basis(wrd, wid, "fp32", hop=hop)
    assert "basis_fold2" in prep
    e, extra = {"complex": (engine.EPI_COMPLEX, {}), "magnitude": (engine.EPI_MAGNITUDE, {}),
                "power2": (engine.EPI_POWER, dict(power=2.0)), "power1": (engine.EPI_POWER, dict(power=1.0, eps=1e-8)),
                "phase": (engine.EPI_PHASE_ATAN2, {}), "cossin": (engine.EPI_PHASE_COSSIN, {})}[epi]
    kw = dict(hop=hop, pad=pad, pad_mode=2, precision="fp32", epilogue=e, **extra)
    ys = _at_caps(lambda: engine.framed_gemm(xd, wrd, wid, fft=True, **kw, **prep))
    y_gemm = engine.framed_gemm(xd, wrd, wid, fft=False, **kw, **prep)
    assert not torch.equal(ys[1], y_gemm), "the contraction kernels ran"
    _assert_bit_identical(ys, "fft K %d %s" % (K, epi))  # (a tile's arithmetic does not depend on who runs it)
    y = ys[1].cpu().numpy()
    re, im = _rfft_ref(x, wr[0], K, hop, pad, F)
    what = "fft K %d %s, cap 1" % (K, epi)
    mag = np.sqrt(re * re + im * im)
    # (the tolerances of tests/test_gpu_fft.py::test_fft_path_against_float64)
    if epi == "complex":
        ref = np.stack((re, im), -1)
        assert_parity(y, ref, rel=1e-4, what=what)
        assert np.abs(y - ref).max() <= 2e-6 * np.abs(ref).max(), what
    elif epi == "magnitude":
        assert_parity(y, mag, rel=1e-4, what=what)
        assert np.abs(y - mag).max() <= 2e-6 * mag.max(), what
    elif epi == "power2":
        assert_parity(y, mag * mag, rel=1e-4, what=what)
    elif epi == "power1":
        assert_parity(y, np.sqrt(mag * mag + 1e-8), rel=1e-4, what=what)
    elif epi == "phase":
        assert_phase_parity(y, np.arctan2(im, re), mag, what=what)
    else:
        ang = np.arctan2(im, re)
        assert_phase_parity(y, np.stack((np.cos(ang), np.sin(ang)), -1), mag, what=what)


@pytest.mark.parametrize("kw", [dict(sr=16000, n_fft=512, n_mels=40, hop_length=128),
                                dict(sr=44100, n_fft=2048, n_mels=229, hop_length=512)])
def test_fused_mel_at_capped_counts(kw, fft_on):
    """the filterbank reduced in the FFT kernel's tile flush (deferred to the next tile of the workgroup)"""
    from nnaudio_amd import engine, features
    from oracle import spectral_oracle as O

    m = features.MelSpectrogram(verbose=False, **kw).to(DEV)
    hop = kw["hop_length"]
    L = (T_FFT - 1) * hop + 7
    x = np.random.default_rng(kw["n_fft"]).standard_normal((B_FFT, L)).astype(np.float32)
    xd = torch.as_tensor(x).to(DEV)
    with torch.no_grad():
        ys = _at_caps(lambda: m(xd))
        engine.set_fft(False)
        g = m(xd)
        engine.set_fft(True)
    assert ys[0].shape == (B_FFT, kw["n_mels"], T_FFT) and not torch.equal(g, ys[1]), "the contraction ran"
    _assert_bit_identical(ys, "fused mel %s" % kw)
    ref = O.filterbank_spectrogram(x, m.stft.wsin.cpu().numpy(), m.stft.wcos.cpu().numpy(), hop,
                                   m.mel_basis.cpu().numpy())
    assert_parity(ys[1].cpu().numpy(), ref, rel=1e-4, what="fused mel cap 1")


@pytest.mark.parametrize("K", [1024, 2048])
def test_frame_major_at_capped_counts(K):
    """out_frame_major (Gammatonegram's power spectrogram as (B, T, Fp) rows)"""
    from nnaudio_amd import engine

    rng = np.random.default_rng(K + 1)
    x, hop, pad = _fft_problem(K, rng)
    F = K // 2 + 1
    Fp = (F + 31) // 32 * 32
    wr, wi = _dft_basis(F, K, "hann", rng)
    xd, wrd, wid = (torch.as_tensor(a).to(DEV) for a in (x, wr, wi))
    prep = engine.prepare_basis(wrd, wid, "fp32", hop=hop)
    kw = dict(hop=hop, pad=pad, pad_mode=2, precision="fp32", epilogue=engine.EPI_POWER, power=2.0)
    ys = _at_caps(lambda: engine.framed_gemm(xd, wrd, wid, out_frame_major=Fp, fft=True, **kw, **prep))
    _assert_bit_identical(ys, "frame-major K %d" % K)
    y = ys[1].cpu().numpy()
    assert y.shape == (B_FFT, T_FFT, Fp) and not y[:, :, F:].any()
    re, im = _rfft_ref(x, wr[0], K, hop, pad, F)
    assert_parity(y[:, :, :F].transpose(0, 2, 1), re * re + im * im, rel=1e-4, what="frame-major K %d cap 1" % K)


# ---------------------------------------------------------------------------------------------------------------
# inverse STFT: istft_fft_kernel (grid min(tiles of 8 frames, CUs) rounded up to 8) and the fused inverse
# (runs per clip = ceil(CUs / clips), at most a quarter of its tiles re-walked)
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_fft,hop,B,T", [(2048, 512, 3, 201), (1024, 256, 2, 133), (512, 128, 5, 77)])
def test_inverse_fft_at_capped_counts(n_fft, hop, B, T):
    from nnaudio_amd import engine, features
    from oracle import spectral_oracle as O

    m = features.STFT(n_fft=n_fft, hop_length=hop, iSTFT=True, output_format="Complex", verbose=False).to(DEV)
    g = torch.Generator().manual_seed(n_fft + T)
    spec = torch.randn(B, n_fft // 2 + 1, T, 2, generator=g)
    length = (T - 1) * hop - 5
    specd = spec.to(DEV)
    assert B * -(-T // 8) >= 3 * 8  # cap 1 / 5: grid of 8 workgroups, >= 3 tiles each
    old_fft = engine.set_fft(True)
    try:
        fused = _at_caps(lambda: m.inverse(specd, length=length), caps=(1, 5, 32, 37))
        old = engine.set_istft_fused(False)
        try:
            two = _at_caps(lambda: m.inverse(specd, length=length))
        finally:
            engine.set_istft_fused(old)
        engine.set_fft(False)
        r = m.inverse(specd, length=length)
    finally:
        engine.set_fft(old_fft)
    assert not torch.equal(r, fused[0]), "the contraction ran"
    _assert_bit_identical(two, "istft_fft_kernel n_fft %d" % n_fft)
    _assert_bit_identical(fused, "fused inverse n_fft %d" % n_fft)
    assert torch.equal(fused[1], two[1]) and torch.equal(fused[0], two[0])  # the fused inverse == the two launches
    sd = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
    ref = O.istft(spec.numpy(), sd["kernel_cos_inv"], sd["kernel_sin_inv"], sd["window_mask"], n_fft, hop,
                  center=True, onesided=True, length=length)
    for c in (1, 0):
        y = fused[c].cpu().numpy()
        assert np.abs(y - ref).max() <= 3e-6 * np.abs(ref).max(), c  # (test_inverse_fft_matches_the_contraction_and_inverts)


def test_fused_inverse_runs_per_clip_follow_the_cap():
    """mirror of the run plan (mispec.hip mispec_istft_fft_f32): one run per clip at cap 1, many on the device"""
    def runs(cus, n_clips, n_fft, hop, start, out_len):
        span = 8 * hop
        n_tiles = -(-(start + out_len) // span)
        n_warm = -(-(n_fft - hop) // span)
        r = -(-cus // n_clips)
        most = max(n_tiles // (4 * max(n_warm, 1)), 1)
        r = max(min(r, most), 1)
        per = -(-n_tiles // r)
        return -(-n_tiles // per)

    n = torch.cuda.get_device_properties(0).multi_processor_count
    # the first shape of test_inverse_fft_at_capped_counts
    args = (3, 2048, 512, 1024, 200 * 512 - 5)
    assert runs(1, *args) == 1 and runs(n, *args) > 1


# ---------------------------------------------------------------------------------------------------------------
# MFCC tail: shares per clip = ceil(4 CUs / clips) -> 64-frame tiles per workgroup
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,n_mels,n_mfcc,T", [(2, 128, 20, 461), (3, 40, 13, 300), (1, 229, 40, 1000)])
def test_mfcc_tail_at_capped_counts(B, n_mels, n_mfcc, T):
    from nnaudio_amd import engine
    from nnaudio_amd.features.mel import dct_ortho_matrix
    from oracle import spectral_oracle as O

    rng = np.random.default_rng(T)
    mel = (rng.random((B, n_mels, T)) ** 6 * 10.0).astype(np.float32)
    mel[0, :, : T // 3] *= 1e-9  # (a quiet stretch: the top_db floor is active)
    dct = dct_ortho_matrix(n_mfcc, n_mels)
    meld, dctd = torch.as_tensor(mel).to(DEV), torch.as_tensor(np.asarray(dct, np.float32)).to(DEV)
    n_tiles = -(-T // 64)
    shares = max(1, min(-(-4 * 1 // B), n_tiles))
    assert -(-n_tiles // shares) >= 3  # cap 1: a workgroup owns >= 3 tiles (mispec.hip mispec_mfcc_tail_f32)
    ys = _at_caps(lambda: engine.mfcc_tail(meld, 1e-10, 1.0, 80.0, dctd))
    assert ys[0] is not None and ys[0].shape == (B, n_mfcc, T)
    _assert_bit_identical(ys, "mfcc tail")
    ref = np.einsum("kn,bnt->bkt", np.asarray(dct, np.float64), O.power_to_db(mel, 1e-10, 1.0, 80.0))
    for c in (1, 0):
        y = ys[c].cpu().numpy()
        assert np.abs(y - ref).max() <= 2e-6 * np.abs(ref).max(), c  # (test_mfcc_tail_in_one_launch)


# ---------------------------------------------------------------------------------------------------------------
# fold kernels: the rounds rule of launch_fold (mispec.hip:2698-2716) and launch_fold2 (:2829-2846)
# ---------------------------------------------------------------------------------------------------------------
def _fold_branch(n_cols, n_tiles_m, n_cu):
    """mirror of the rule: '128' = 128-frame tiles only, '256' = 256-frame tiles only, 'mixed' = whole rounds on
    256-frame tiles + a tail on 128-frame ones"""
    tn = -(-n_cols // 256)
    grid = tn * n_tiles_m
    rounds = grid / n_cu
    if rounds <= 0.5:
        return "128"
    if rounds > 1.0:
        whole = int(rounds) * n_cu // n_tiles_m
        if whole < tn:
            half = -(-(n_cols - whole * 256) // 128) * n_tiles_m
            tail = 0.8 * half / n_cu
            mixed = whole * n_tiles_m / n_cu + max(tail, 0.8)
            if mixed < int(rounds + 0.999) - 0.05:
                return "mixed"
    return "256"


# (kind, B, L, bins, K, hop, pad, mode, window): fold2 = window x DFT basis with the FFT route off (bench.fold_geometry:
# 8 row tiles for 1025 bins); fold = a basis with the Fourier symmetry only (2 row tiles for 200 bins)
FOLD_SHAPES = {
    "fold2": (3, 100000, 1025, 2048, 256, 1024, 2, "hann"),
    "fold": (2, 192000, 200, 512, 77, 256, 2, None),
}


def _fold_geometry(kind, B, L, F, K, hop, pad):
    import bench

    bins, _taps = bench.fold_geometry(F, K, fused_fb=(kind == "fold"))
    T = (L + 2 * pad - K) // hop + 1
    return B * T, bins // 128


def _fold_cases():
    cases = []
    for kind, s in FOLD_SHAPES.items():
        B, L, F, K, hop, pad = s[:6]
        n_cols, n_tm = _fold_geometry(kind, B, L, F, K, hop, pad)
        for cap in (1, 32, 37, 64):
            br = _fold_branch(n_cols, n_tm, cap)
            for prec in ("fp32", "bf16x3", "f16x3"):
                cases.append(pytest.param(kind, cap, prec, id="%s-cap%d-%s-%s" % (kind, cap, br, prec)))
    return cases


def test_fold_cases_hit_every_branch_of_the_rounds_rule():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    for kind, s in FOLD_SHAPES.items():
        B, L, F, K, hop, pad = s[:6]
        n_cols, n_tm = _fold_geometry(kind, B, L, F, K, hop, pad)
        seen = {_fold_branch(n_cols, n_tm, c) for c in (1, 32, 37, 64, n)}
        assert seen == {"128", "256", "mixed"}, (kind, seen)


@pytest.mark.parametrize("kind,cap,precision", _fold_cases())
def test_fold_rounds_rule_at_capped_counts(kind, cap, precision):
    from nnaudio_amd import engine

    B, L, F, K, hop, pad, mode, window = FOLD_SHAPES[kind]
    rng = np.random.default_rng(F + K + hop)
    x = rng.standard_normal((B, L)).astype(np.float32)
    if kind == "fold2":
        wr, wi = _dft_basis(F, K, window, rng)
        scale = None
    else:
        wr, wi = _fourier_like_basis(rng, F, K, False)
        scale = rng.uniform(0.5, 2.0, F).astype(np.float32)
    if precision == "f16x3":  # (as test_symmetric_fold_kernel: the fp16 pairs hold coefficient x 2^14)
        wr, wi = 0.3 * wr, 0.3 * wi
    xd, wrd, wid = (torch.as_tensor(a).to(DEV) for a in (x, wr, wi))
    prep = engine.prepare_basis(wrd, wid, precision, hop=hop)
    assert ("basis_fold2" if kind == "fold2" else "basis_fold") in prep
    kw = dict(hop=hop, pad=pad, pad_mode=mode, precision=precision, epilogue=engine.EPI_COMPLEX)
    if scale is not None:
        kw["row_scale"] = torch.as_tensor(scale).to(DEV)
    ys = _at_caps(lambda: engine.framed_gemm(xd, wrd, wid, fft=False, **kw, **prep), caps=(cap,))
    # the tile height changes which workgroup computes a frame, not the order of its sum over the taps
    _assert_bit_identical(ys, "%s %s cap %d" % (kind, precision, cap))
    dense = engine.framed_gemm(xd, wrd, wid, fft=False, **kw, **{k: v for k, v in prep.items() if k == "basis_split"})
    assert not torch.equal(dense, ys[cap]), "the fold kernel did not run"
    re, im = _np_framed(x, wr, wi, hop, pad, mode, scale)
    ref = np.stack((re, im), -1)
    y = ys[cap].cpu().numpy()
    what = "%s %s cap %d" % (kind, precision, cap)
    assert_parity(y, ref, rel=1e-4, what=what)
    err = np.abs(y - ref).max() / np.abs(ref).max()
    budget = BUDGET[precision] if kind == "fold2" else (2e-5 if precision == "bf16x3" else 3e-6)
    assert err <= budget, "%s: %.2e of the peak" % (what, err)


# ---------------------------------------------------------------------------------------------------------------
# strip kernels (bf16x3 / f16x3 / fp32): the plan's jobs and grid (2 per CU), 64- or 128-frame jobs by the count
# ---------------------------------------------------------------------------------------------------------------
STRIP_SHAPES = [  # (B, L, bins, K, hop, pad, mode) of test_strip_kernel_epilogues
    (3, 50000, 84, 4096, 256, 2048, 2),
    (7, 17000, 100, 1024, 96, 0, 0),
]


def _strip_bank(shape):
    B, L, F, K, hop, pad, mode = shape
    rng = np.random.default_rng(L)
    x = rng.standard_normal((B, L)).astype(np.float32)
    half = np.geomspace(K // 2 - 3, 24, F).astype(np.int64)
    lo, hi = K // 2 - half, K // 2 + half + (np.arange(F) % 2)
    keep = (np.arange(K)[None, :] >= lo[:, None]) & (np.arange(K)[None, :] < hi[:, None])
    wr = (rng.standard_normal((F, K)) * keep).astype(np.float32)
    wi = (rng.standard_normal((F, K)) * keep).astype(np.float32)
    sup = np.ascontiguousarray(np.stack([lo, hi], 1).astype(np.int32))
    sc = rng.uniform(0.5, 2.0, F).astype(np.float32)
    return x, wr, wi, sup, sc


def _strip_operands(shape, precision):
    from nnaudio_amd import engine

    x, wr, wi, sup, sc = _strip_bank(shape)
    xd, wrd, wid, scd = (torch.as_tensor(a).to(DEV) for a in (x, wr, wi, sc))
    supd = torch.as_tensor(sup).to(DEV)
    supd.host_copy = sup
    B, L, F, K, hop, pad, mode = shape
    extra = {}
    if precision == "f16x3":
        extra["basis_split"] = engine.frag_basis_f16(wrd, wid)
    elif precision == "fp32":
        extra["basis_split"] = engine.frag_basis_f32(wrd, wid)
    kw = dict(hop=hop, pad=pad, pad_mode=mode, precision=precision, row_support=supd, row_scale=scd,
              epilogue=engine.EPI_COMPLEX, **extra)
    return (x, wr, wi, sc), (xd, wrd, wid), kw


def _strip_plan(xd, wrd, wid, kw, n_cu):
    from nnaudio_amd import _abi, engine

    a, _o, _d, _keep = engine._framed_args(xd, wrd, wid, **kw)
    buf = (ctypes.c_int32 * (1 + 8 * 36))()
    n = _abi.load().mispec_strip_plan(ctypes.byref(a), n_cu, buf, len(buf))
    assert n > 0, "the strip kernel is not planned: %s" % _abi.load().mispec_last_error()
    return list(buf[:1 + 36 * n])


def _tap_split(plan):
    """the per-pass grouping of a mispec_strip_plan: super-stage range + per wave (tile, taps, super-stages,
    reduction group) -- what decides the order of a row tile's sum"""
    n = (len(plan) - 1) // 36
    return [[plan[2 + 36 * i:4 + 36 * i]] + [plan[5 + 36 * i + 8 * w:12 + 36 * i + 8 * w] for w in range(4)]
            for i in range(n)]


@pytest.mark.parametrize("shape", STRIP_SHAPES)
@pytest.mark.parametrize("precision", ["bf16x3", "f16x3", "fp32"])
def test_strip_kernels_at_capped_counts(shape, precision):
    from nnaudio_amd import engine

    (x, wr, wi, sc), (xd, wrd, wid), kw = _strip_operands(shape, precision)
    n = torch.cuda.get_device_properties(0).multi_processor_count
    plans = {c: _strip_plan(xd, wrd, wid, kw, c) for c in (1, 5, 32, 37, n)}
    assert any(plans[c] != plans[n] for c in CAPS), "no cap changes the strip plan of %s" % (shape,)
    ys = _at_caps(lambda: engine.framed_gemm(xd, wrd, wid, **kw))
    # bit identity only where the cap keeps the device's tap split: plan_strip (mispec.hip) groups the row tiles
    # into passes and gives each wave a run of a tile's super-stages (StripWave kb / ke / ja / jb), whose partial
    # sums the group then reduces (framed_bf16x3_strip.inl) -- another grouping adds the same products in another
    # order.  64- or 128-frame jobs alone (nf, slab rows, frame tiles) keep the order.
    kept = [c for c in CAPS if _tap_split(plans[c]) == _tap_split(plans[n])]
    assert kept, "no cap keeps the device's tap split of %s: bit identity is not checked" % (shape,)
    _assert_bit_identical({c: ys[c] for c in [0] + kept}, "strip %s %s" % (precision, shape))
    B, L, F, K, hop, pad, mode = shape
    re, im = _np_framed(x, wr, wi, hop, pad, mode, sc)
    ref = np.stack((re, im), -1)
    tol = 1e-4 if precision == "bf16x3" else 1e-5  # (test_strip_kernel_epilogues)
    for c in [0] + list(CAPS):
        y = ys[c].cpu().numpy()
        assert np.abs(y - ref).max() <= tol * np.abs(ref).max(), (precision, c)


def test_strip_workspace_sized_under_another_count():
    """A workspace sized by mispec_framed_gemm_workspace_bytes under one count and launched under another: the
    strip paths' workspace (strip16_ws_bytes; the strip32 branch of the query) holds the split / padded signal,
    the job counter and the per-clip maxima -- no term depends on the plan, and whether plan_strip succeeds does
    not depend on its slot count (n_slots only ranks the feasible groupings).  So no strip shape's workspace grows
    with the count: the size is the same under every cap, a launch under another cap with it computes what the
    device's plan computes, and one byte less is refused with MISPEC_E_INVALID before any kernel runs."""
    from nnaudio_amd import _abi, engine

    lib = _abi.load()
    for precision in ("f16x3", "fp32"):
        shape = STRIP_SHAPES[0]
        _h, (xd, wrd, wid), kw = _strip_operands(shape, precision)
        ref = engine.framed_gemm(xd, wrd, wid, **kw)
        sizes = {}
        for c in (1, 5, 37, 0):
            with engine.plan_cus(c):
                a, out, _d, keep = engine._framed_args(xd, wrd, wid, **kw)
                sizes[c] = lib.mispec_framed_gemm_workspace_bytes(ctypes.byref(a))
        assert sizes[0] > 0 and len(set(sizes.values())) == 1, sizes
        need = sizes[0]
        for size_cap, run_cap in ((1, 0), (0, 1), (5, 37)):
            with engine.plan_cus(run_cap):
                a, out, _d, keep = engine._framed_args(xd, wrd, wid, **kw)
                ws = torch.empty(need, dtype=torch.uint8, device=DEV)
                a.workspace, a.workspace_bytes = ws.data_ptr(), sizes[size_cap]
                stream = torch.cuda.current_stream().cuda_stream
                assert lib.mispec_framed_gemm_f32(ctypes.byref(a), ctypes.c_void_p(stream)) == 0, lib.mispec_last_error()
                torch.cuda.synchronize()
                assert torch.equal(out, ref), (precision, size_cap, run_cap)
                a.workspace_bytes = need - 1
                assert lib.mispec_framed_gemm_f32(ctypes.byref(a), ctypes.c_void_p(stream)) == _abi.E_INVALID
                assert b"workspace too small" in lib.mispec_last_error()


# ---------------------------------------------------------------------------------------------------------------
# octave kernels: default segments per clip of the streaming kernel (ceil(CUs / clips)), frames per work item of
# the fused pyramid kernel (nf: 8192 level-0 samples, but >= ~4 items per CU, within 80 KB of LDS)
# ---------------------------------------------------------------------------------------------------------------
def test_octave_stream_default_segments_at_capped_counts():
    """the kernel with n_segments = 0 (its own plan) against the float64 recursion.  No bit identity: each
    segment starts its fp16 operand scale from its own first chunk (octave_stream.hip, the F16 operand scale of
    the streaming loop), so another segment plan splits the samples of a segment's later chunks differently."""
    from tests.test_gpu_stream import _run_kernel
    from tests.test_octave_stream_cpu import library_plan

    n = torch.cuda.get_device_properties(0).multi_processor_count
    B, L0, hop0, K = 2, 70000, 512, (192, 192, 192, 192)
    x = np.random.default_rng(3).standard_normal((B, L0)).astype(np.float32)
    segs = {}
    for c in (1, 5, 32, 37, n):
        rc, p = library_plan(L0, hop0, K, L0 // hop0 + 1, 0, n_cus=c, n_clips=B)
        assert rc == 0
        segs[c] = p.n_segments
    assert segs[1] == 1 and segs[n] > 1, segs
    from nnaudio_amd import engine

    for c in (1, 5, 37):
        with engine.plan_cus(c):
            err = _run_kernel(x, K, hop0, 0, "f16x3", True)  # (asserts the kernel took the shape)
        assert err < 2e-6, (c, err)  # (test_stream_kernel_matches_the_float64_recursion)


@pytest.mark.parametrize("cls", ["CQT2010v2", "VQT"])
def test_octave_stream_modules_at_capped_counts(cls):
    from nnaudio_amd import engine, features

    kw = dict(sr=44100, hop_length=512, n_bins=96, output_format="Complex", verbose=False)
    m = getattr(features, cls)(**(dict(kw, gamma=10) if cls == "VQT" else kw)).to(DEV)
    m.precision = "f16x3"
    x = torch.randn(3, 132300, generator=torch.Generator().manual_seed(8))
    xd = x.to(DEV)
    assert engine.octave_stream_enabled()
    with torch.no_grad():
        for c in (1, 5, 37):
            with engine.plan_cus(c):
                y = m(xd)
            _cfg5_sampled_check(m, x, y, np.random.default_rng(c), "%s f16x3 cap %d" % (cls, c), tol=5e-6)


def _pyramid_nf(hop0, n_frames, n_clips, n_cu):
    """mirror of the first two steps of the nf rule (mispec.hip mispec_octave_pyramid_f32; the LDS fit may lower it)"""
    nf = (8192 // hop0 + 15) // 16 * 16
    cap = (n_frames * n_clips // (4 * n_cu) + 15) // 16 * 16
    return max(16, min(nf, cap))


@pytest.mark.parametrize("precision", ["bf16x3", "f16x3"])
def test_fused_octave_kernel_at_capped_counts(precision):
    """the pyramid kernel (octave stream off) with nf moved from 16 (the device's count) to its maximum (cap 1).
    No bit identity: nf sets which frames share a work item, and with it the fp16 operand scale of the item
    (f16x3: p.item_scale) and the halo each item decimates again."""
    from nnaudio_amd import engine, features

    B, L, hop = 3, 66150, 128  # (_cfg5_sampled_check samples clips 0 .. 2)
    T = L // hop + 1
    n = torch.cuda.get_device_properties(0).multi_processor_count
    nfs = {c: _pyramid_nf(hop, T, B, c) for c in (1, 5, 32, 37, n)}
    assert nfs[n] == 16 and nfs[1] == 64 and nfs[37] == 16, nfs
    m = features.CQT2010v2(sr=44100, hop_length=hop, n_bins=96, output_format="Complex", verbose=False).to(DEV)
    m.precision = precision
    x = torch.randn(B, L, generator=torch.Generator().manual_seed(12))
    xd = x.to(DEV)
    tol = 1e-4 if precision == "bf16x3" else 5e-6  # (test_cfg5_fused_octave_kernel)
    old = engine.set_octave_stream(False)
    try:
        with torch.no_grad():
            ys = _at_caps(lambda: m(xd), caps=(1, 5, 37))
            m.precision = "fp32"
            y32 = m(xd)
            m.precision = precision
    finally:
        engine.set_octave_stream(old)
    for c, y in ys.items():
        assert not torch.equal(y, y32), "the fused kernel did not run"
        _cfg5_sampled_check(m, x, y, np.random.default_rng(20 + c), "pyramid %s cap %d" % (precision, c), tol=tol)
