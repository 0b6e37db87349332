"""flamo_amd.optimize.mel_mss_loss without a GPU: the class's torch lines against a second statement of the definition written
here (``statement``: torch.stft row by row, the mel matrix of tests/test_edr_host.py built entry by entry, the mask, the norms),
its gradient for every option, ``ops.mel_basis`` at n_fft // 8 bands from 0 Hz, the noise-energy rule, the conditions on the
test signals that keep a mask entry or a sign from flipping between precisions, the inputs that take the torch lines, the
sizes the kernels take, and the seventh header's place in the C ABI."""
import ctypes
import inspect
import math
import os

import pytest
import torch

from conftest import check_close
from test_edr_host import _header_symbols, statement_mel
from test_mrstft_host import signals

NFFT = (128, 256, 512, 1024, 2048, 4096)
_mel = {}


def mel_matrix(sample_rate, nfft):
    if (sample_rate, nfft) not in _mel:
        _mel[sample_rate, nfft] = statement_mel(sample_rate, nfft, n_mels=nfft // 8, fmin=0.0, fmax=sample_rate // 2)
    return _mel[sample_rate, nfft]


def mel_spectrograms(y, nfft, overlap=0.75, sample_rate=48000):
    """(rows, nfft // 8, F) in y's dtype: one torch.stft per (batch, channel) column, |X|^2, the mel projection"""
    B, T, N = y.shape
    hop = int(nfft * (1 - overlap))
    W = mel_matrix(sample_rate, nfft).to(y.dtype)
    window = torch.hann_window(nfft, periodic=True, dtype=y.dtype)
    rows = []
    for b in range(B):
        for c in range(N):
            X = torch.stft(y[b, :, c], n_fft=nfft, hop_length=hop, win_length=nfft, window=window, center=True,
                           pad_mode="reflect", return_complex=True)
            assert tuple(X.shape) == (nfft // 2 + 1, 1 + T // hop)
            rows.append(W @ (X.real.square() + X.imag.square()))
    return torch.stack(rows)


def noise_energy_rule(m_t, sample_rate, hop):
    """mean(m_t[:, :, -int(0.01 sample_rate / hop)]^2): frame 0 when that integer is 0"""
    return m_t[:, :, -int(0.01 * sample_rate / hop)].square().mean()


def snr_of(m_t, ne):
    ne = torch.as_tensor(ne, dtype=m_t.dtype)
    return 10 * torch.log10(torch.maximum(m_t.square(), ne * 1.01) - ne) - 10 * torch.log10(ne)


def statement(y_pred, y_true, nfft=NFFT, overlap=0.75, sample_rate=48000, energy_norm=False, apply_mask=False, threshold=5.0,
              p="fro", log_term=False, alpha=1.0, noise_energy=None, parts=None):
    """The criterion of (B, T, N) signals as the issue states it, summed over the resolutions.  ``noise_energy`` None is derived
    at the first resolution and kept for the others.  ``parts``, a list, receives (m_p, m_t, mask) per resolution."""
    if energy_norm:
        y_pred, y_true = y_pred / y_pred.square().sum().sqrt(), y_true / y_true.square().sum().sqrt()
    loss = 0
    ne = noise_energy
    for n in nfft:
        hop = int(n * (1 - overlap))
        m_p, m_t = (mel_spectrograms(y, n, overlap, sample_rate) for y in (y_pred, y_true))
        mask = torch.ones_like(m_t)
        if apply_mask:
            if ne is None:
                ne = noise_energy_rule(m_t.detach(), sample_rate, hop)
            mask = torch.where(snr_of(m_t.detach(), ne) < threshold, torch.zeros_like(m_t), mask)
            count = mask.sum()
        else:
            count = m_t.numel()
        terms = [((m_t - m_p) * mask, 1.0)] + ([((m_t.log() - m_p.log()) * mask, alpha)] if log_term else [])
        for d, weight in terms:
            norm = d.square().sum().sqrt() if p in ("fro", 2) else d.abs().sum()
            loss = loss + weight * norm / count
        if parts is not None:
            parts.append((m_p.detach(), m_t.detach(), mask))
    return loss


def statement_grad(yp, yt, cotangent=1.0, **kw):
    y = yp.clone().requires_grad_(True)
    loss = statement(y, yt, **kw)
    (g,) = torch.autograd.grad(cotangent * loss, [y])
    return loss.detach(), g


# name -> (shape, seed, class options): the cases of tests/test_mel_mss_gpu.py
CASES = {
    "shortest": ((1, 2049, 1), 4, {}),                      # 3 frames at 4096, both margins nearly the whole signal; 65 at 128
    "rows": ((2, 2603, 2), 2, {}),                          # rows and channels, T divisible by no hop
    "only128": ((1, 2049, 1), 4, dict(nfft=[128])),
    "only4096": ((1, 2049, 1), 4, dict(nfft=[4096])),
    "log": ((1, 2603, 1), 1, dict(log_term=True)),
    "one_log": ((1, 2603, 1), 1, dict(p=1, log_term=True, alpha=0.5)),
    "rate8000": ((1, 2603, 1), 1, dict(sample_rate=8000)),
    "half": ((1, 2603, 1), 1, dict(overlap=0.5)),
    "norm": ((2, 2603, 2), 2, dict(energy_norm=True)),
    "mask": ((1, 2049, 1), 4, dict(apply_mask=True, noise_energy=1e-3)),
    "mask_rows": ((2, 2603, 2), 2, dict(apply_mask=True, noise_energy=1e-3)),
    "mask_one": ((1, 2603, 1), 1, dict(apply_mask=True, noise_energy=1e-3, p=1)),
    "mask_derived": ((1, 2603, 1), 1, dict(apply_mask=True, log_term=True)),
}


def crit_kw(opts, device="cpu"):
    """(the class's instance, the statement's keywords)"""
    from flamo_amd.optimize import mel_mss_loss
    crit = mel_mss_loss(device=device, **opts)
    return crit, dict(nfft=tuple(crit.nfft), overlap=crit.overlap, sample_rate=crit.sample_rate, energy_norm=crit.energy_norm,
                      apply_mask=crit.apply_mask, threshold=crit.threshold, p=crit.p, log_term=crit.log_term, alpha=crit.alpha,
                      noise_energy=crit.noise_energy)


def conditions(name, yp, yt, kw):
    """The conditions on a case's signals, asserted with the statement; returns (kept share per resolution, smallest SNR
    margin in dB, smallest |m_t - m_p| / max m_t)."""
    parts = []
    statement(yp, yt, parts=parts, **kw)
    ne = kw["noise_energy"]
    shares, margin, gap = [], math.inf, math.inf
    for n, (m_p, m_t, mask) in zip(kw["nfft"], parts):
        gap = min(gap, ((m_t - m_p).abs().min() / m_t.max()).item())
        if kw["apply_mask"]:
            if ne is None:
                ne = noise_energy_rule(m_t, kw["sample_rate"], int(n * (1 - kw["overlap"])))
            shares.append(mask.mean().item())
            margin = min(margin, (snr_of(m_t, ne) - kw["threshold"]).abs().min().item())
    print(f"[cond] {name}: kept {['%.3f' % s for s in shares]}  SNR margin {margin:.2e} dB  min |m_t - m_p| / max m_t {gap:.2e}")
    if kw["apply_mask"]:
        assert all(s > 0 for s in shares), "every masked case keeps at least one entry at every resolution"
        assert any(0.05 < s < 0.95 for s in shares), "one resolution's kept share lies strictly between 0.05 and 0.95"
        assert margin >= 1e-6
    if kw["p"] == 1:
        assert gap >= 1e-12
    return shares, margin, gap


@pytest.mark.parametrize("name", list(CASES))
def test_torch_lines_agree_with_the_statement(name):
    shape, seed, opts = CASES[name]
    crit, kw = crit_kw(opts)
    yp, yt = signals(shape, seed)
    want, gwant = statement_grad(yp, yt, 3.0, **kw)
    y = yp.clone().requires_grad_(True)
    got = crit(y, yt)
    assert got.dim() == 0 and got.dtype == torch.float64 and type(got.grad_fn).__name__ != "_MelMSSBackward"
    (g,) = torch.autograd.grad(3.0 * got, [y])
    assert torch.isfinite(got) and torch.isfinite(g).all() and want.item() > 0
    check_close(f"mel_mss_host/{name}/loss", got.detach().reshape(1), want.reshape(1), 1e-12)
    check_close(f"mel_mss_host/{name}/grad", g, gwant, 1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_signals_keep_masks_and_signs_apart(name):
    shape, seed, opts = CASES[name]
    conditions(name, *signals(shape, seed), crit_kw(opts)[1])


def test_one_dimensional_inputs_and_the_shape_assertion():
    from flamo_amd.optimize import mel_mss_loss
    crit = mel_mss_loss(nfft=[128, 512])
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
    from flamo_amd.optimize import mel_mss_loss
    assert optimize.mel_mss_loss is mel_mss_loss and not hasattr(optimize, "mss_loss")
    sig = inspect.signature(mel_mss_loss.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("nfft", [128, 256, 512, 1024, 2048, 4096]), ("overlap", 0.75), ("sample_rate", 48000), ("energy_norm", False),
        ("device", "cpu"), ("name", "MelMSS"), ("apply_mask", False), ("threshold", 5), ("p", "fro"), ("log_term", False),
        ("alpha", 1.0), ("noise_energy", None)]
    crit = mel_mss_loss()
    assert (crit.nfft, crit.overlap, crit.sample_rate, crit.energy_norm, crit.device, crit.name, crit.apply_mask, crit.threshold,
            crit.p, crit.log_term, crit.alpha, crit.noise_energy) == \
        ([128, 256, 512, 1024, 2048, 4096], 0.75, 48000, False, "cpu", "MelMSS", False, 5, "fro", False, 1.0, None)
    assert isinstance(crit, torch.nn.Module) and callable(crit._torch_forward) and callable(crit._on_kernels)
    m = crit.mel_stft(torch.randn(3, 2603, dtype=torch.float64), 512)
    assert m.shape == (3, 64, 21) and m.dtype == torch.float64 and (m > 0).all()
    assert "mixes channels" in mel_mss_loss.__doc__ and "graph" in mel_mss_loss.__doc__


@pytest.mark.parametrize("sample_rate", [48000, 44100, 8000])
@pytest.mark.parametrize("nfft", NFFT)
def test_mel_basis_at_an_eighth_of_the_frame(sample_rate, nfft):
    from flamo_amd import ops
    W = ops.mel_basis(sample_rate, nfft, n_mels=nfft // 8, fmin=0, fmax=sample_rate // 2)
    assert W.shape == (nfft // 8, nfft // 2 + 1) and W.dtype == torch.float64
    ref = mel_matrix(sample_rate, nfft)
    assert ((W - ref).abs().max() / ref.abs().max()).item() <= 1e-13
    taps = (W > 0).sum(1)
    assert taps.min() >= 1 and taps.max() <= 34                # no empty band; the longest spans 34 bins
    band = torch.nonzero(W.T)                                  # (bin, band) pairs, sorted by bin
    for k in range(W.shape[1]):                                # at most two bands per bin, and those consecutive
        js = band[band[:, 0] == k][:, 1].tolist()
        assert len(js) <= 2 and (len(js) < 2 or js[1] == js[0] + 1), (k, js)
    idx, w, nnz = ops._edr_mel_tables(W.numpy())
    nm, nb = nfft // 8, nfft // 2 + 1
    assert idx.size == 3 * nm + nb and w.size == nnz + 2 * nb and nnz == int(taps.sum())
    back = torch.zeros_like(W)
    for j in range(nm):
        back[j, idx[j]:idx[j] + idx[nm + j]] = torch.from_numpy(w[idx[2 * nm + j]:idx[2 * nm + j] + idx[nm + j]])
    assert torch.equal(back, W)


def test_noise_energy_is_derived_once_and_kept():
    """frame -int(0.01 sample_rate / hop) of the FIRST resolution of the FIRST call, then the same number for every later
    resolution and call"""
    from flamo_amd.optimize import mel_mss_loss
    yp, yt = signals((1, 2603, 1), 1)
    crit = mel_mss_loss(nfft=[256, 1024], apply_mask=True)
    assert int(0.01 * 48000 / 64) == 7
    want = noise_energy_rule(mel_spectrograms(yt, 256), 48000, 64)
    assert torch.equal(want, mel_spectrograms(yt, 256)[:, :, -7].square().mean())
    first = crit(yp, yt)
    assert isinstance(crit.noise_energy, float) and abs(crit.noise_energy - want.item()) <= 1e-12 * want.item()
    kept = crit.noise_energy
    check_close("mel_mss_host/noise/first", first.reshape(1),
                statement(yp, yt, nfft=(256, 1024), apply_mask=True).reshape(1), 1e-12)
    # another target, another order of resolutions: the number stays
    yp2, yt2 = signals((1, 2603, 1), 9)
    crit.nfft = [1024, 256]
    second = crit(yp2, yt2)
    assert crit.noise_energy == kept
    check_close("mel_mss_host/noise/second", second.reshape(1),
                statement(yp2, yt2, nfft=(1024, 256), apply_mask=True, noise_energy=kept).reshape(1), 1e-12)
    # hop 2048 at 8 kHz: int(0.01 * 8000 / 2048) = 0, so frame -0 = frame 0, not the last one
    yp3, yt3 = signals((1, 4500, 1), 5)
    low = mel_mss_loss(nfft=[4096], overlap=0.5, sample_rate=8000, apply_mask=True)
    low(yp3, yt3)
    m = mel_spectrograms(yt3, 4096, 0.5, 8000)
    assert m.shape[-1] == 3 and abs(low.noise_energy - m[:, :, 0].square().mean().item()) <= 1e-12 * low.noise_energy
    assert abs(low.noise_energy - m[:, :, -1].square().mean().item()) > 1e-3 * low.noise_energy
    # a number that was passed is never replaced
    given = mel_mss_loss(nfft=[256], apply_mask=True, noise_energy=1e-3)
    given(yp, yt)
    assert given.noise_energy == 1e-3


def test_float32_host_tensors_take_the_torch_lines():
    crit, kw = crit_kw(dict(log_term=True))
    yp, yt = signals((2, 2603, 1), 5)
    got = crit(yp.float(), yt.float())
    assert got.dtype == torch.float32
    check_close("mel_mss_host/f32/loss", got.double().reshape(1), statement(yp, yt, **kw).reshape(1), 2e-6)


def test_inputs_that_take_the_torch_lines():
    from flamo_amd import ops
    from flamo_amd.optimize import mel_mss_loss
    yp, yt = signals((1, 1100, 2), 4)
    crit = mel_mss_loss(nfft=[128, 256])
    assert not crit._on_kernels(yp, yt)                                        # host tensors
    yt.requires_grad_(True)
    crit(yp, yt).backward()                                                    # a target that takes a gradient gets one
    assert yt.grad is not None and torch.isfinite(yt.grad).all() and torch.count_nonzero(yt.grad) > 0
    three = mel_mss_loss(nfft=[128, 256], p=3)                                 # another p: torch's vector norm
    yt = yt.detach()
    parts = []
    statement(yp, yt, nfft=(128, 256), parts=parts)
    want = sum((m_t - m_p).abs().pow(3).sum().pow(1 / 3) / m_t.numel() for m_p, m_t, _ in parts)
    check_close("mel_mss_host/p3", three(yp, yt).reshape(1), want.reshape(1), 1e-12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mel_mss_loss(yp, yt)


def _built():
    from flamo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_sizes_the_kernels_take():
    from flamo_amd import ops
    _built()
    ok = ops.mel_mss_supported
    assert ok((1, 2049, 1)) and ok((2, 2603, 2)) and ok((4, 96000, 2), NFFT, 0.75, 48000, "fro")
    assert not ok((1, 2048, 1)) and ok((1, 2048, 1), [128, 2048])                      # n_fft / 2 < T
    assert ok((1, 65, 1), [128]) and not ok((1, 64, 1), [128])
    for bad in ([64], [8192], [768], [], [128] * 9, [128.5], None, 128):
        assert not ok((1, 9000, 1), bad), bad
    assert ok((1, 9000, 1), [128] * 8) and ok((1, 9000, 1), (4096, 128))
    assert ok((1, 9000, 1), [128], 0.99) and not ok((1, 9000, 1), [128], 0.999)            # hop = int(1.28) = 1; int(0.128) = 0
    assert not ok((1, 9000, 1), [128], 1.5) and not ok((1, 9000, 1), [128], "x")
    assert ok((1, 1 << 30, 1), [4096]) and not ok((1, (1 << 30) + 1, 1), [4096])
    assert not ok((1, 1 << 30, 3), [128], 0.99)                                            # 2^31 frames and more
    for p in ("fro", 2, 1):
        assert ok((1, 9000, 1), NFFT, 0.75, 48000, p)
    for p in (3, "nuc", None, 0.5, float("inf")):
        assert not ok((1, 9000, 1), NFFT, 0.75, 48000, p), p
    for sr in (48000, 44100, 8000):
        assert ok((1, 9000, 1), NFFT, 0.75, sr)
    assert not ok((1, 9000, 1), NFFT, 0.75, 1) and not ok((1, 9000, 1), NFFT, 0.75, "48000")
    assert not ok((9000,)) and not ok((0, 9000, 1)) and not ok((1, 9000.5, 1))


ENTRIES = ["fl_melmss_bwd_f32", "fl_melmss_bwd_f64", "fl_melmss_frames", "fl_melmss_fwd_f32", "fl_melmss_fwd_f64",
           "fl_melmss_gframe_elems", "fl_melmss_keep_doubles", "fl_melmss_launches", "fl_melmss_mel_doubles", "fl_melmss_mel_ints"]


def test_seventh_header_is_bound_and_exported():
    from flamo_amd import _lib
    syms = _header_symbols("flamo_hip_melmss.h")
    assert syms == ENTRIES and sorted(_lib._SIGNATURES_MELMSS) == ENTRIES
    assert not set(ENTRIES) & set(_lib.EXPORTS)
    for other in (_lib._SIGNATURES_EDC, _lib._SIGNATURES_AVGPOW, _lib._SIGNATURES_FDNATT, _lib._SIGNATURES_MRSTFT,
                  _lib._SIGNATURES_EDR):
        assert not set(ENTRIES) & set(other)
    for name in ("fl_melmss_fwd", "fl_melmss_bwd"):
        assert _lib._SIGNATURES_MELMSS[name + "_f32"] == _lib._SIGNATURES_MELMSS[name + "_f64"]
    handle = ctypes.CDLL(_lib.LIB_PATH) if os.path.exists(_lib.LIB_PATH) else None
    if handle is not None:
        for s in ENTRIES:
            assert hasattr(handle, s), f"{s} declared in include/flamo_hip_melmss.h but not exported"
        L = _lib.lib()
        for name, (res, args) in _lib._SIGNATURES_MELMSS.items():
            fn = getattr(L, name)
            assert fn.restype is res and list(fn.argtypes) == args, name


def _res(*triples):
    flat = [v for t in triples for v in t]
    return len(triples), (ctypes.c_int * len(flat))(*flat)


def test_query_entries_and_launch_counts():
    """the launches depend on the list of n_fft alone: two frame launches when both size classes have a resolution, one
    otherwise, plus combine and final forward and the overlap-add backward -- at most four and three"""
    L = _built()
    assert L.fl_melmss_keep_doubles() == 65
    six = _res(*[(n, n // 4, 7) for n in NFFT])
    assert L.fl_melmss_frames(1, 2049, 1, *six) == 65 + 33 + 17 + 9 + 5 + 3
    assert L.fl_melmss_frames(2, 2603, 2, *six) == 4 * (82 + 41 + 21 + 11 + 6 + 3)
    assert L.fl_melmss_gframe_elems(1, 2049, 1, *six) == 65 * 128 + 33 * 256 + 17 * 512 + 9 * 1024 + 5 * 2048 + 3 * 4096
    assert L.fl_melmss_mel_ints(*six) == sum(3 * (n // 8) + n // 2 + 1 for n in NFFT)
    assert L.fl_melmss_mel_doubles(*six) == sum(7 + 2 * (n // 2 + 1) for n in NFFT)
    assert L.fl_melmss_launches(*six, 0) == 4 and L.fl_melmss_launches(*six, 1) == 3
    for only in (128, 1024, 2048, 4096):
        one = _res((only, only // 4, 0))
        assert L.fl_melmss_launches(*one, 0) == 3 and L.fl_melmss_launches(*one, 1) == 2
    assert L.fl_melmss_launches(*_res((128, 32, 0), (256, 64, 0), (1024, 256, 0)), 0) == 3
    assert L.fl_melmss_launches(*_res((1024, 256, 0), (2048, 512, 0)), 0) == 4
    for bad in (_res((64, 16, 0)), _res((8192, 2048, 0)), _res((768, 192, 0)), _res((128, 0, 0)), _res((128, 32, -1)),
                _res((128, 32, 16 * 65 + 1)), _res(*[(128, 32, 0)] * 9)):
        assert L.fl_melmss_frames(1, 9000, 1, *bad) == -1 and L.fl_melmss_launches(*bad, 0) == -1
        assert L.fl_melmss_mel_ints(*bad) == -1 and L.fl_melmss_mel_doubles(*bad) == -1
    assert L.fl_melmss_frames(1, 2048, 1, *six) == -1 and L.fl_melmss_gframe_elems(1, 2048, 1, *six) == -1
    assert L.fl_melmss_frames(0, 9000, 1, *six) == -1


def test_entries_check_their_arguments():
    L = _built()
    one = ctypes.c_void_p(16)          # never dereferenced: the checks come first
    R, res = _res((128, 32, 40), (4096, 1024, 5000))
    head = (("yp", one), ("spb", 9000), ("spt", 1), ("spc", 1), ("yt", one), ("stb", 9000), ("stt", 1), ("stc", 1), ("B", 1),
            ("T", 9000), ("N", 1), ("R", R), ("res", res), ("wtab", one), ("tw", one), ("melidx", one), ("melw", one), ("norm", 2),
            ("log_term", 0))
    fwd_args = head + (("alpha", 1.0), ("apply_mask", 0), ("threshold", 5.0), ("noise_energy", 1.0), ("partial", one),
                       ("keep", one), ("loss", one), ("stream", None))
    bwd_args = head + (("apply_mask", 0), ("threshold", 5.0), ("noise_energy", 1.0), ("keep", one), ("gloss", one),
                       ("gframes", one), ("gy", one), ("stream", None))
    call = lambda fn, args, **kw: fn(*[kw.get(n, v) for n, v in args])
    fwd_ptrs = ("yp", "yt", "res", "wtab", "tw", "melidx", "melw", "partial", "keep", "loss")
    bwd_ptrs = ("yp", "yt", "res", "wtab", "tw", "melidx", "melw", "keep", "gloss", "gframes", "gy")
    for fn, args, ptrs in ((L.fl_melmss_fwd_f32, fwd_args, fwd_ptrs), (L.fl_melmss_fwd_f64, fwd_args, fwd_ptrs),
                           (L.fl_melmss_bwd_f32, bwd_args, bwd_ptrs), (L.fl_melmss_bwd_f64, bwd_args, bwd_ptrs)):
        for name in ptrs:
            assert call(fn, args, **{name: None}) == -1 and b"null" in L.fl_last_error(), name
        assert call(fn, args, T=2048) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, B=0) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, R=0) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, res=_res((768, 192, 0), (4096, 1024, 0))[1]) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, norm=3) == -1 and b"norm" in L.fl_last_error()
        assert call(fn, args, apply_mask=1, noise_energy=0.0) == -1 and b"noise_energy" in L.fl_last_error()
        assert call(fn, args, apply_mask=1, noise_energy=float("nan")) == -1 and b"noise_energy" in L.fl_last_error()
        assert call(fn, args, tw=ctypes.c_void_p(24)) == -1 and b"aligned" in L.fl_last_error()
