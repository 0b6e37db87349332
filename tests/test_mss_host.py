"""flamo_amd.optimize.loss.mss_loss without a GPU: the class's torch lines against a second statement of the definition written
here (``statement``: the basis entry by entry from beta_k, the frames from F.pad + unfold, the three forms, the mask, the
norms), its gradient for every option, the magnitudes against a direct per-bin sum, the noise-energy rule, the conditions on
the test signals that keep a mask entry or a sign from flipping between precisions, the inputs that take the torch lines, the
sizes the kernels take, and the ninth header's place in the C ABI.

The phases.  beta_k j / n_fft reaches 2048 cycles, where a float64 product is rounded to 4.5e-13 cycles (3e-12 rad): two
float64 statements that round it differently are 1e-12 apart in the gradient, the limit of the comparison below.  So the
statement reduces the phase to its fraction in extended precision (numpy's longdouble) before the float64 cosine, and the
class reduces it in integers (``ops.mss_cycles``): two routes to the same float64 basis."""
import ctypes
import inspect
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import check_close
from test_edr_host import _header_symbols
from test_mrstft_host import signals

NFFT = (128, 256, 512, 1024, 2048, 4096)
_basis = {}


def grid(sample_rate, nfft):
    """(a, s) of beta_k = a + k s as exact fractions"""
    K = nfft // 2 + 1
    return Fraction(20 * nfft, sample_rate), Fraction((sample_rate // 2 - 20) * nfft, sample_rate * K)


def basis(sample_rate, nfft):
    """(cos, sin)(2 pi beta_k j / n_fft), two float64 (K, n_fft) matrices, every entry from its own beta_k and j"""
    if (sample_rate, nfft) not in _basis:
        assert np.finfo(np.longdouble).eps < 1e-18
        ld = np.longdouble
        K = nfft // 2 + 1
        a = ld(20) * ld(nfft) / ld(sample_rate)
        s = ld(sample_rate // 2 - 20) * (ld(nfft) / ld(sample_rate)) / ld(K)
        beta = a + np.arange(K, dtype=ld) * s
        cycles = beta[:, None] * np.arange(nfft, dtype=ld)[None, :] / ld(nfft)
        ang = torch.from_numpy((cycles - np.floor(cycles)).astype(np.float64)) * (2 * math.pi)
        _basis[sample_rate, nfft] = (torch.cos(ang), torch.sin(ang))
    return _basis[sample_rate, nfft]


def frames_of(y, nfft, hop):
    """(rows, F, n_fft): every (batch, channel) column reflect-padded by n_fft // 2 and cut into frames"""
    B, T, N = y.shape
    rows = y.permute(0, 2, 1).reshape(B * N, 1, T)
    fr = F.pad(rows, (nfft // 2, nfft // 2), mode="reflect")[:, 0].unfold(-1, nfft, hop)
    assert fr.shape[1] == 1 + T // hop
    return fr


def spectrograms(y, nfft, overlap=0.75, sample_rate=48000):
    """M (rows, K, F) in y's dtype; the square root's derivative at an exact zero is taken as 0"""
    hop = int(nfft * (1 - overlap))
    cos, sin = (m.to(y.dtype) for m in basis(sample_rate, nfft))
    fr = frames_of(y, nfft, hop) * torch.hann_window(nfft, periodic=True, dtype=torch.float64).to(y.dtype)
    re, im = torch.einsum("rfj,kj->rkf", fr, cos), -torch.einsum("rfj,kj->rkf", fr, sin)
    power = re.square() + im.square()
    zero = power == 0
    return torch.where(zero, torch.zeros_like(power), torch.where(zero, torch.ones_like(power), power).sqrt())


def noise_energy_rule(M_t, sample_rate, hop):
    """mean(M_t[:, :, -int(0.01 sample_rate / hop)]^2): frame 0 when that integer is 0"""
    return M_t[:, :, -int(0.01 * sample_rate / hop)].square().mean()


def snr_of(M_t, ne):
    ne = torch.as_tensor(ne, dtype=M_t.dtype)
    return 10 * torch.log10(torch.maximum(M_t.square(), ne * 1.01) - ne) - 10 * torch.log10(ne)


def statement(y_pred, y_true, nfft=NFFT, overlap=0.75, sample_rate=48000, energy_norm=False, apply_mask=False, threshold=5.0,
              p="fro", log_term=False, alpha=1.0, form=None, noise_energy=None, parts=None):
    """The criterion of (B, T, N) signals as the issue states it, summed over the resolutions.  ``noise_energy`` None is derived
    at the first resolution and kept for the others.  ``parts``, a list, receives (M_p, M_t, mask) per resolution."""
    if energy_norm:
        y_pred, y_true = y_pred / y_pred.square().sum().sqrt(), y_true / y_true.square().sum().sqrt()
    loss = 0
    ne = noise_energy
    two, one = (lambda d: d.square().sum().sqrt()), (lambda d: d.abs().sum())
    for n in nfft:
        hop = int(n * (1 - overlap))
        M_p, M_t = (spectrograms(y, n, overlap, sample_rate) for y in (y_pred, y_true))
        mask = torch.ones_like(M_t)
        count = numel = M_t.numel()
        if apply_mask:
            if ne is None:
                ne = noise_energy_rule(M_t.detach(), sample_rate, hop)
            mask = torch.where(snr_of(M_t.detach(), ne) < threshold, torch.zeros_like(M_t), mask)
            count = mask.sum()
        d = (M_t - M_p) * mask
        dl = (M_t.log() - M_p.log()) * mask if (log_term or form is not None) else None
        if form is None:
            norm = two if p in ("fro", 2) else one
            loss = loss + norm(d) / count + (alpha * norm(dl) / count if log_term else 0)
        elif form == "yamamoto":
            loss = loss + two(d) / two(M_t) + alpha * one(dl) / numel
        else:
            assert form == "magenta"
            loss = loss + (one(d) + alpha * one(dl)) / numel
        if parts is not None:
            parts.append((M_p.detach(), M_t.detach(), mask))
    return loss


def statement_grad(yp, yt, cotangent=1.0, **kw):
    y = yp.clone().requires_grad_(True)
    loss = statement(y, yt, **kw)
    (g,) = torch.autograd.grad(cotangent * loss, [y])
    return loss.detach(), g


# name -> (shape, seed, class options): the cases of tests/test_mss_gpu.py
CASES = {
    "shortest": ((1, 2049, 1), 4, {}),                      # 3 frames at 4096, both margins nearly the whole signal; 65 at 128
    "rows": ((2, 2603, 2), 2, {}),                          # rows and channels, T divisible by no hop
    "only128": ((1, 2049, 1), 4, dict(nfft=[128])),
    "only4096": ((1, 2049, 1), 4, dict(nfft=[4096])),
    "odd_size": ((2, 2603, 2), 2, dict(nfft=[300])),        # K = 151, hop 75, no power of two, every tile tail
    "log": ((1, 2603, 1), 1, dict(log_term=True)),
    "one_log": ((1, 2603, 1), 1, dict(p=1, log_term=True, alpha=0.5)),
    "yamamoto": ((1, 2603, 1), 1, dict(form="yamamoto")),
    "magenta": ((1, 2603, 1), 1, dict(form="magenta", alpha=0.5)),
    "rate8000": ((1, 2603, 1), 1, dict(sample_rate=8000)),
    "half": ((1, 2603, 1), 1, dict(overlap=0.5)),
    "norm": ((2, 2603, 2), 2, dict(energy_norm=True)),
    "mask": ((1, 2049, 1), 4, dict(nfft=[2048, 4096], apply_mask=True, noise_energy=1.0)),
    "mask_rows": ((2, 2603, 2), 2, dict(apply_mask=True, noise_energy=1.0)),
    "mask_one": ((1, 2603, 1), 1, dict(apply_mask=True, noise_energy=1.0, p=1)),
    "mask_yamamoto": ((1, 2603, 1), 1, dict(apply_mask=True, noise_energy=1.0, form="yamamoto")),
    "mask_derived": ((1, 2603, 1), 1, dict(apply_mask=True)),
}


def crit_kw(opts, device="cpu"):
    """(the class's instance, the statement's keywords)"""
    from flamo_amd.optimize.loss import mss_loss
    crit = mss_loss(device=device, **opts)
    return crit, dict(nfft=tuple(crit.nfft), overlap=crit.overlap, sample_rate=crit.sample_rate, energy_norm=crit.energy_norm,
                      apply_mask=crit.apply_mask, threshold=crit.threshold, p=crit.p, log_term=crit.log_term, alpha=crit.alpha,
                      form=crit.form, noise_energy=crit.noise_energy)


def conditions(name, yp, yt, kw):
    """The conditions on a case's signals, asserted with the statement; returns (kept share per resolution, smallest SNR
    margin in dB, smallest |M_t - M_p| / max M_t, smallest M)."""
    parts = []
    statement(yp, yt, parts=parts, **kw)
    ne = kw["noise_energy"]
    shares, margin, gap, least = [], math.inf, math.inf, math.inf
    for n, (M_p, M_t, mask) in zip(kw["nfft"], parts):
        gap = min(gap, ((M_t - M_p).abs().min() / M_t.max()).item())
        least = min(least, M_p.min().item(), M_t.min().item())
        if kw["apply_mask"]:
            if ne is None:
                ne = noise_energy_rule(M_t, kw["sample_rate"], int(n * (1 - kw["overlap"])))
            shares.append(mask.mean().item())
            margin = min(margin, (snr_of(M_t, ne) - kw["threshold"]).abs().min().item())
    print(f"[cond] {name}: kept {['%.3f' % s for s in shares]}  SNR margin {margin:.2e} dB  min |M_t - M_p| / max M_t {gap:.2e}"
          f"  min M {least:.2e}")
    if kw["apply_mask"]:
        assert all(s > 0 for s in shares), "every masked case keeps at least one entry at every resolution"
        assert any(0.05 < s < 0.95 for s in shares), "one resolution's kept share lies strictly between 0.05 and 0.95"
        assert margin >= 1e-6
    if kw["p"] == 1 or kw["log_term"] or kw["form"] is not None:
        assert gap >= 1e-12 and least > 0
    return shares, margin, gap, least


@pytest.mark.parametrize("name", list(CASES))
def test_torch_lines_agree_with_the_statement(name):
    shape, seed, opts = CASES[name]
    crit, kw = crit_kw(opts)
    yp, yt = signals(shape, seed)
    want, gwant = statement_grad(yp, yt, 3.0, **kw)
    y = yp.clone().requires_grad_(True)
    got = crit(y, yt)
    assert got.dim() == 0 and got.dtype == torch.float64 and type(got.grad_fn).__name__ != "_MSSBackward"
    (g,) = torch.autograd.grad(3.0 * got, [y])
    assert torch.isfinite(got) and torch.isfinite(g).all() and want.item() > 0
    check_close(f"mss_host/{name}/loss", got.detach().reshape(1), want.reshape(1), 1e-12)
    check_close(f"mss_host/{name}/grad", g, gwant, 1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_signals_keep_masks_and_signs_apart(name):
    shape, seed, opts = CASES[name]
    conditions(name, *signals(shape, seed), crit_kw(opts)[1])


@pytest.mark.parametrize("sample_rate,nfft,overlap", [(48000, 128, 0.75), (48000, 4096, 0.75), (8000, 300, 0.5)])
def test_magnitudes_are_a_direct_sum_per_bin(sample_rate, nfft, overlap):
    """sum_j w_j x_j cos / sin(2 pi beta_k j / n) with the phase an exact fraction, at a handful of (k, f); bin 0 sits at 20 Hz
    and the last bin under Nyquist"""
    from flamo_amd.optimize.loss import mss_loss
    K, hop = nfft // 2 + 1, int(nfft * (1 - overlap))
    a, s = grid(sample_rate, nfft)
    assert a * sample_rate / nfft == 20 and 20 < (a + (K - 1) * s) * sample_rate / nfft < sample_rate // 2
    assert (a + K * s) * sample_rate / nfft == sample_rate // 2 and s < 1
    if (sample_rate, nfft) == (48000, 128):
        assert abs(float(s) - 0.98379) < 5e-6
    if (sample_rate, nfft) == (48000, 4096):
        assert abs(float(s) - 0.99868) < 5e-6 and round(float((a + (K - 1) * s) * sample_rate / nfft)) == 23988
    yt = signals((1, 2603, 1), 1)[1]
    crit = mss_loss(nfft=[nfft], overlap=overlap, sample_rate=sample_rate)
    M = crit.lin_stft(yt[:, :, 0], nfft)
    assert M.shape == (1, K, 1 + 2603 // hop) and M.dtype == torch.float64
    assert crit.lin_stft(yt[:, :, 0].float(), nfft).dtype == torch.float32
    fr = frames_of(yt, nfft, hop)[0] * torch.hann_window(nfft, periodic=True, dtype=torch.float64)
    for k, f in ((0, 0), (1, 2), (K // 2, 1), (K - 2, M.shape[2] - 1), (K - 1, 0), (K - 1, M.shape[2] - 1)):
        beta = a + k * s
        ang = [2 * math.pi * float((beta * j / nfft) % 1) for j in range(nfft)]
        x = fr[f].tolist()
        re = math.fsum(v * math.cos(t) for v, t in zip(x, ang))
        im = -math.fsum(v * math.sin(t) for v, t in zip(x, ang))
        assert abs(M[0, k, f].item() - math.hypot(re, im)) <= 1e-12 * M.max().item(), (k, f)


def test_one_dimensional_inputs_and_the_shape_assertion():
    from flamo_amd.optimize.loss import mss_loss
    crit = mss_loss(nfft=[128, 512])
    yp, yt = signals((1, 1100, 1), 3)
    a = yp[0, :, 0].clone().requires_grad_(True)
    b = yp.clone().requires_grad_(True)
    la, lb = crit(a, yt[0, :, 0]), crit(b, yt)
    assert la.dim() == 0 and torch.equal(la, lb)
    assert torch.equal(torch.autograd.grad(la, [a])[0], torch.autograd.grad(lb, [b])[0][0, :, 0])
    with pytest.raises(AssertionError, match="same shape"):
        crit(torch.randn(1, 1100, 1), torch.randn(1, 1101, 1))
    with pytest.raises(AssertionError, match="same shape"):
        crit(torch.randn(1100, 2), torch.randn(1100, 2))


def test_constructor_attributes_and_defaults():
    from flamo_amd import optimize
    from flamo_amd.optimize import loss
    from flamo_amd.optimize.loss import mss_loss
    assert loss.mss_loss is mss_loss and not hasattr(optimize, "mss_loss")
    sig = inspect.signature(mss_loss.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("nfft", [128, 256, 512, 1024, 2048, 4096]), ("overlap", 0.75), ("sample_rate", 48000), ("energy_norm", False),
        ("device", "cpu"), ("name", "MSS"), ("apply_mask", False), ("threshold", 5), ("p", "fro"), ("log_term", False),
        ("alpha", 1.0), ("form", None), ("noise_energy", None)]
    crit = mss_loss()
    assert (crit.nfft, crit.overlap, crit.sample_rate, crit.energy_norm, crit.device, crit.name, crit.apply_mask, crit.threshold,
            crit.p, crit.log_term, crit.alpha, crit.form, crit.noise_energy) == \
        ([128, 256, 512, 1024, 2048, 4096], 0.75, 48000, False, "cpu", "MSS", False, 5, "fro", False, 1.0, None, None)
    assert isinstance(crit, torch.nn.Module) and callable(crit._torch_forward) and callable(crit._on_kernels)
    assert callable(crit._rows) and callable(crit.lin_stft)
    with pytest.raises(ValueError, match="form"):
        mss_loss(form="x")
    assert mss_loss(form="yamamoto").form == "yamamoto" and mss_loss(form="magenta").form == "magenta"
    assert "mixes channels" in mss_loss.__doc__ and "graph" in mss_loss.__doc__ and "not re-exported" in mss_loss.__doc__


def test_noise_energy_is_derived_once_and_kept():
    """frame -int(0.01 sample_rate / hop) of the FIRST resolution of the FIRST call, then the same number for every later
    resolution and call"""
    from flamo_amd.optimize.loss import mss_loss
    yp, yt = signals((1, 2603, 1), 1)
    crit = mss_loss(nfft=[256, 1024], apply_mask=True)
    assert int(0.01 * 48000 / 64) == 7
    want = spectrograms(yt, 256)[:, :, -7].square().mean()
    assert torch.equal(want, noise_energy_rule(spectrograms(yt, 256), 48000, 64))
    first = crit(yp, yt)
    assert isinstance(crit.noise_energy, float) and abs(crit.noise_energy - want.item()) <= 1e-12 * want.item()
    kept = crit.noise_energy
    check_close("mss_host/noise/first", first.reshape(1), statement(yp, yt, nfft=(256, 1024), apply_mask=True).reshape(1), 1e-12)
    # another target, another order of resolutions: the number stays
    yp2, yt2 = signals((1, 2603, 1), 9)
    crit.nfft = [1024, 256]
    second = crit(yp2, yt2)
    assert crit.noise_energy == kept
    check_close("mss_host/noise/second", second.reshape(1),
                statement(yp2, yt2, nfft=(1024, 256), apply_mask=True, noise_energy=kept).reshape(1), 1e-12)
    # hop 2048 at 8 kHz: int(0.01 * 8000 / 2048) = 0, so frame -0 = frame 0, not the last one
    yp3, yt3 = signals((1, 4500, 1), 5)
    low = mss_loss(nfft=[4096], overlap=0.5, sample_rate=8000, apply_mask=True)
    low(yp3, yt3)
    M = spectrograms(yt3, 4096, 0.5, 8000)
    assert M.shape[-1] == 3 and abs(low.noise_energy - M[:, :, 0].square().mean().item()) <= 1e-12 * low.noise_energy
    assert abs(low.noise_energy - M[:, :, -1].square().mean().item()) > 1e-3 * low.noise_energy
    # a number that was passed is never replaced
    given = mss_loss(nfft=[256], apply_mask=True, noise_energy=1e-3)
    given(yp, yt)
    assert given.noise_energy == 1e-3


def test_float32_host_tensors_take_the_torch_lines():
    crit, kw = crit_kw(dict(log_term=True))
    yp, yt = signals((2, 2603, 1), 5)
    got = crit(yp.float(), yt.float())
    assert got.dtype == torch.float32
    check_close("mss_host/f32/loss", got.double().reshape(1), statement(yp, yt, **kw).reshape(1), 2e-6)


def test_inputs_that_take_the_torch_lines():
    from flamo_amd import ops
    from flamo_amd.optimize.loss import mss_loss
    yp, yt = signals((1, 1100, 2), 4)
    crit = mss_loss(nfft=[128, 256])
    assert not crit._on_kernels(yp, yt)                                        # host tensors
    yt.requires_grad_(True)
    crit(yp, yt).backward()                                                    # a target that takes a gradient gets one
    assert yt.grad is not None and torch.isfinite(yt.grad).all() and torch.count_nonzero(yt.grad) > 0
    three = mss_loss(nfft=[128, 256], p=3)                                     # another p: torch's vector norm
    yt = yt.detach()
    parts = []
    statement(yp, yt, nfft=(128, 256), parts=parts)
    want = sum((M_t - M_p).abs().pow(3).sum().pow(1 / 3) / M_t.numel() for M_p, M_t, _ in parts)
    check_close("mss_host/p3", three(yp, yt).reshape(1), want.reshape(1), 1e-12)
    # a sample rate that is no integer: the float64 product of the phases, on the torch lines
    odd = mss_loss(nfft=[128], sample_rate=44100.5)
    assert torch.isfinite(odd(yp, yt)) and not ops.mss_supported((1, 1100, 2), [128], 0.75, 44100.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mss_loss(yp, yt)


def test_a_silent_stretch_has_a_zero_derivative():
    """the first 700 samples of the prediction exactly zero: M_p = 0 exactly on the frames inside; the torch lines give a
    finite loss and an exactly zero gradient there without the log term, and a non-finite loss with it"""
    yp, yt = signals((1, 2603, 1), 1, silent=700)
    for lines in (statement, crit_kw(dict(nfft=[128, 512]))[0]._torch_forward):
        y = yp.clone().requires_grad_(True)
        loss = lines(y, yt, nfft=(128, 512)) if lines is statement else lines(y, yt)
        (g,) = torch.autograd.grad(loss, [y])
        assert torch.isfinite(loss) and torch.isfinite(g).all() and torch.count_nonzero(g[:, :256]) == 0
        assert torch.count_nonzero(g[:, 700:]) > 0
    assert not torch.isfinite(statement(yp, yt, nfft=(128, 512), log_term=True))
    assert not torch.isfinite(crit_kw(dict(nfft=[128, 512], log_term=True))[0](yp, yt))


def _built():
    from flamo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_sizes_the_kernels_take():
    from flamo_amd import ops
    _built()
    ok = ops.mss_supported
    assert ok((1, 2049, 1)) and ok((2, 2603, 2)) and ok((4, 96000, 2), NFFT, 0.75, 48000, "fro", None)
    assert not ok((1, 2048, 1)) and ok((1, 2048, 1), [128, 2048])                      # n_fft / 2 < T
    assert ok((1, 65, 1), [128]) and not ok((1, 64, 1), [128])
    for good in ([16], [300], [20, 4092], [768], [128] * 8, (4096, 128)):                 # no power of two is asked for
        assert ok((1, 9000, 1), good), good
    for bad in ([12], [8192], [4100], [18], [130], [], [128] * 9, [128.5], None, 128):
        assert not ok((1, 9000, 1), bad), bad
    assert ok((1, 9000, 1), [128], 0.99) and not ok((1, 9000, 1), [128], 0.999)            # hop = int(1.28) = 1; int(0.128) = 0
    assert not ok((1, 9000, 1), [128], 1.5) and not ok((1, 9000, 1), [128], "x")
    assert ok((1, 1 << 30, 1), [4096]) and not ok((1, (1 << 30) + 1, 1), [4096])
    assert not ok((1, 1 << 30, 3), [128], 0.99)                                            # 2^31 frames and more
    assert not ok((1, 1 << 30, 1), [16]) and ok((1, 1 << 27, 1), [16])                     # 2^24 workgroups and more in a launch
    assert not ok((4, 1 << 30, 1), [4096]) and ok((3, 1 << 30, 1), [4096])                 # 2^32 samples: a thread per sample
    for p in ("fro", 2, 1):
        assert ok((1, 9000, 1), NFFT, 0.75, 48000, p)
    for p in (3, "nuc", None, 0.5, float("inf")):
        assert not ok((1, 9000, 1), NFFT, 0.75, 48000, p), p
    for form in (None, "yamamoto", "magenta"):
        assert ok((1, 9000, 1), NFFT, 0.75, 48000, "fro", form)
    for form in ("x", 0, [], "Yamamoto"):
        assert not ok((1, 9000, 1), NFFT, 0.75, 48000, "fro", form), form
    for sr in (48000, 44100, 8000, 80, 48000.0):
        assert ok((1, 9000, 1), NFFT, 0.75, sr), sr
    for sr in (79, 1, 0, -48000, "48000", None, float("nan"), float("inf"), True):
        assert not ok((1, 9000, 1), NFFT, 0.75, sr), sr
    assert not ok((9000,)) and not ok((0, 9000, 1)) and not ok((1, 9000.5, 1))


def test_host_tables_hold_the_basis():
    """the seed and step tables of ops._mss_host against the statement's basis: a run of rotations from a seed walks the
    basis's own entries"""
    from flamo_amd import ops
    for sr, n in ((48000, 128), (8000, 300), (48000, 4096)):
        K, NJ, NK = n // 2 + 1, -(-n // 64), -(-(n // 2 + 1) // 64)
        tab = ops._mss_host(sr, n)
        assert tab.dtype == torch.float64 and tab.numel() == n + 2 * (K * NJ + 5 * K + n * NK + 5 * n)
        assert ops._mss_host(sr, n) is tab
        cos, sin = basis(sr, n)
        w, rest = tab[:n], tab[n:].reshape(-1, 2)
        fseed, fstep = rest[:K * NJ].reshape(K, NJ, 2), rest[K * NJ:K * NJ + 5 * K].reshape(K, 5, 2)
        bseed = rest[K * NJ + 5 * K:K * NJ + 5 * K + n * NK].reshape(n, NK, 2)
        bstep = rest[K * NJ + 5 * K + n * NK:].reshape(n, 5, 2)
        assert torch.equal(w, torch.hann_window(n, periodic=True, dtype=torch.float64))
        # the two routes to the fraction of a cycle end one rounding of a number under 1 apart, 1.1e-16, which is 7e-16 rad;
        # the product by 2 pi and the cosine add a rounding each
        tol = 4e-15
        assert (fseed[..., 0] - cos[:, ::64]).abs().max() <= tol and (fseed[..., 1] + sin[:, ::64]).abs().max() <= tol
        assert (fstep[..., 0] - cos[:, :5]).abs().max() <= tol and (fstep[..., 1] + sin[:, :5]).abs().max() <= tol
        assert (bseed[..., 0] - cos[::64].T).abs().max() <= tol and (bseed[..., 1] - sin[::64].T).abs().max() <= tol
        # exp(+i (theta_c - theta_0) j) = E[c, j] conj(E[0, j])
        for c in range(5):
            re = cos[c] * cos[0] + sin[c] * sin[0]
            im = sin[c] * cos[0] - cos[c] * sin[0]
            assert (bstep[:, c, 0] - re).abs().max() <= 2 * tol and (bstep[:, c, 1] - im).abs().max() <= 2 * tol


def test_a_run_of_rotations_stays_on_the_basis():
    """what the kernels' lanes do, in float64 here: start at seed x step[offset], multiply by step[4] fifteen times, and land
    on the basis's own entries.  The bound: a table entry is within 1.2e-15 of its exact value (the fraction of a cycle is
    rounded once, 7e-16 rad; the product by 2 pi and the cosine add a rounding each), a complex product adds 3.2e-16, the step
    enters 15 times, and the statement's basis is a table entry itself: 3 x 1.2e-15 + 15 x (1.2e-15 + 3.2e-16) + 3.2e-16 =
    2.7e-14.  Measured: 1.7e-14 at 4096.  That is the re-seed distance of 16 steps (64 samples or bins)."""
    from flamo_amd import ops

    def cmul(a, b):
        return torch.stack((a[..., 0] * b[..., 0] - a[..., 1] * b[..., 1], a[..., 0] * b[..., 1] + a[..., 1] * b[..., 0]), -1)

    for sr, n in ((48000, 128), (8000, 300), (48000, 4096)):
        K, NJ, NK = n // 2 + 1, -(-n // 64), -(-(n // 2 + 1) // 64)
        rest = ops._mss_host(sr, n)[n:].reshape(-1, 2)
        fseed, fstep = rest[:K * NJ].reshape(K, NJ, 2), rest[K * NJ:K * NJ + 5 * K].reshape(K, 5, 2)
        bseed = rest[K * NJ + 5 * K:K * NJ + 5 * K + n * NK].reshape(n, NK, 2)
        bstep = rest[K * NJ + 5 * K + n * NK:].reshape(n, 5, 2)
        cos, sin = basis(sr, n)
        worst = 0.0
        for seed, step, c, si, count, size in ((fseed, fstep, cos, -sin, NJ, n), (bseed, bstep, cos.T, sin.T, NK, K)):
            for offset in range(4):
                ph = cmul(seed, step[:, offset][:, None, :])
                for s in range(16):
                    at = 64 * torch.arange(count) + 4 * s + offset
                    ok, at = at < size, at.clamp(max=size - 1)
                    err = torch.maximum((ph[..., 0] - c[:, at]).abs(), (ph[..., 1] - si[:, at]).abs())[:, ok]
                    worst = max(worst, err.max().item())
                    ph = cmul(ph, step[:, 4][:, None, :])
        print(f"[rotation] sample_rate {sr} n_fft {n}: {worst:.2e} from the basis after a run of 16")
        assert worst <= 2.7e-14


ENTRIES = ["fl_mss_bwd_f32", "fl_mss_bwd_f64", "fl_mss_frames", "fl_mss_fwd_f32", "fl_mss_fwd_f64", "fl_mss_gframe_elems",
           "fl_mss_keep_doubles", "fl_mss_launches", "fl_mss_partial_doubles", "fl_mss_table_doubles"]


def test_ninth_header_is_bound_and_exported():
    from flamo_amd import _lib
    syms = _header_symbols("flamo_hip_mss.h")
    assert syms == ENTRIES and sorted(_lib._SIGNATURES_MSS) == ENTRIES
    assert not set(ENTRIES) & set(_lib.EXPORTS)
    others = (_lib._SIGNATURES_EDC, _lib._SIGNATURES_AVGPOW, _lib._SIGNATURES_FDNATT, _lib._SIGNATURES_MRSTFT,
              _lib._SIGNATURES_EDR, _lib._SIGNATURES_MELMSS, _lib._SIGNATURES_FILTERBANK)
    for other in others:
        assert not set(ENTRIES) & set(other)
    assert len({id(t) for t in others}) == 7                   # with the main header and this one: nine
    for name in ("fl_mss_fwd", "fl_mss_bwd"):
        assert _lib._SIGNATURES_MSS[name + "_f32"] == _lib._SIGNATURES_MSS[name + "_f64"]
    _built()
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in ENTRIES:
        assert hasattr(handle, s), f"{s} declared in include/flamo_hip_mss.h but not exported"
    L = _lib.lib()
    for name, (res, args) in _lib._SIGNATURES_MSS.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name


def _res(*pairs):
    flat = [v for t in pairs for v in t]
    return len(pairs), (ctypes.c_int * len(flat))(*flat)


def test_query_entries_and_launch_counts():
    """the launches depend on the list of n_fft alone -- here on nothing at all: three forward, two backward"""
    L = _built()
    six = _res(*[(n, n // 4) for n in NFFT])
    F1 = (65, 33, 17, 9, 5, 3)                                         # frames of T = 2049
    F2 = (82, 41, 21, 11, 6, 3)                                        # ... of T = 2603
    K = [n // 2 + 1 for n in NFFT]
    assert L.fl_mss_frames(1, 2049, 1, *six) == sum(F1) and L.fl_mss_frames(2, 2603, 2, *six) == 4 * sum(F2)
    assert L.fl_mss_gframe_elems(1, 2049, 1, *six) == sum(f * n for f, n in zip(F1, NFFT))
    assert L.fl_mss_keep_doubles(1, 2049, 1, *six, 0) == 65
    assert L.fl_mss_keep_doubles(1, 2049, 1, *six, 1) == 65 + 3 * sum(f * k for f, k in zip(F1, K))
    assert L.fl_mss_keep_doubles(2, 2603, 2, *six, 1) == 65 + 3 * 4 * sum(f * k for f, k in zip(F2, K))
    # six sums per workgroup of 16 frames x 256 bins
    assert L.fl_mss_partial_doubles(2, 2603, 2, *six) == 6 * 4 * sum(-(-f // 16) * -(-k // 256) for f, k in zip(F2, K))
    assert L.fl_mss_table_doubles(*six) == sum(n + 2 * (k * -(-n // 64) + 5 * k + n * -(-k // 64) + 5 * n) for n, k in zip(NFFT, K))
    # about 28 MB per row of two seconds at 48 kHz
    assert 27e6 < 8 * (L.fl_mss_keep_doubles(1, 96000, 1, *six, 1) - 65) < 29e6
    lists = [six, _res((128, 32)), _res((4096, 1024)), _res((300, 75)), _res((16, 4), (4096, 1)), _res(*[(128, 32)] * 8)]
    for some in lists:
        assert L.fl_mss_launches(*some, 0) == 3 and L.fl_mss_launches(*some, 1) == 2
        assert L.fl_mss_launches(*some, 0) <= 4 and L.fl_mss_launches(*some, 1) <= 3
    for bad in (_res((12, 3)), _res((8192, 2048)), _res((130, 32)), _res((128, 0)), _res(*[(128, 32)] * 9)):
        assert L.fl_mss_frames(1, 9000, 1, *bad) == -1 and L.fl_mss_launches(*bad, 0) == -1 and L.fl_mss_launches(*bad, 1) == -1
        assert L.fl_mss_table_doubles(*bad) == -1 and L.fl_mss_keep_doubles(1, 9000, 1, *bad, 1) == -1
        assert L.fl_mss_partial_doubles(1, 9000, 1, *bad) == -1 and L.fl_mss_gframe_elems(1, 9000, 1, *bad) == -1
    assert L.fl_mss_frames(1, 2048, 1, *six) == -1 and L.fl_mss_gframe_elems(1, 2048, 1, *six) == -1
    assert L.fl_mss_frames(0, 9000, 1, *six) == -1 and L.fl_mss_keep_doubles(1, 2048, 1, *six, 0) == -1


def test_entries_check_their_arguments():
    L = _built()
    one = ctypes.c_void_p(16)          # never dereferenced: the checks come first
    R, res = _res((128, 32), (4096, 1024))
    sizes = (("B", 1), ("T", 9000), ("N", 1), ("R", R), ("res", res), ("tab", one), ("norm", 2), ("form", 0), ("log_term", 0))
    fwd_args = ((("yp", one), ("spb", 9000), ("spt", 1), ("spc", 1), ("yt", one), ("stb", 9000), ("stt", 1), ("stc", 1)) + sizes
                + (("alpha", 1.0), ("apply_mask", 0), ("threshold", 5.0), ("noise_energy", 1.0), ("planes", 1), ("partial", one),
                   ("keep", one), ("loss", one), ("stream", None)))
    bwd_args = sizes + (("apply_mask", 0), ("threshold", 5.0), ("noise_energy", 1.0), ("keep", one), ("gloss", one),
                        ("gframes", one), ("gy", one), ("stream", None))
    call = lambda fn, args, **kw: fn(*[kw.get(n, v) for n, v in args])
    fwd_ptrs = ("yp", "yt", "res", "tab", "partial", "keep", "loss")
    bwd_ptrs = ("res", "tab", "keep", "gloss", "gframes", "gy")
    for fn, args, ptrs in ((L.fl_mss_fwd_f32, fwd_args, fwd_ptrs), (L.fl_mss_fwd_f64, fwd_args, fwd_ptrs),
                           (L.fl_mss_bwd_f32, bwd_args, bwd_ptrs), (L.fl_mss_bwd_f64, bwd_args, bwd_ptrs)):
        for name in ptrs:
            assert call(fn, args, **{name: None}) == -1 and b"null" in L.fl_last_error(), name
        assert call(fn, args, T=2048) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, B=0) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, R=0) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, res=_res((130, 32), (4096, 1024))[1]) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, norm=3) == -1 and b"norm" in L.fl_last_error()
        assert call(fn, args, form=3) == -1 and b"form" in L.fl_last_error()
        assert call(fn, args, form=-1) == -1 and b"form" in L.fl_last_error()
        for ne in (0.0, -1.0, float("nan"), float("inf")):
            assert call(fn, args, apply_mask=1, noise_energy=ne) == -1 and b"noise_energy" in L.fl_last_error(), ne
        assert call(fn, args, tab=ctypes.c_void_p(24)) == -1 and b"aligned" in L.fl_last_error()
