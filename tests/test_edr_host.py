"""flamo_amd.optimize.edr_loss without a GPU: the class's torch lines against a second statement of the definition written here
(``statement``: torch.stft row by row, a mel matrix built entry by entry, flip / cumsum / flip, the masked assignment), its
gradient, the conditions on the test signals that keep a sign or a clip from flipping between precisions, ``ops.mel_basis``,
the inputs that take the torch lines, the sizes the kernels take, and the sixth header's place in the C ABI."""
import ctypes
import inspect
import math
import os
import re

import pytest
import torch

from conftest import check_close
from test_mrstft_host import signals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def statement_mel(sample_rate, nfft, n_mels=64, fmin=20.0, fmax=None):
    """the Slaney mel basis (htk=False, norm=1) entry by entry, float64"""
    fmax = sample_rate // 2 if fmax is None else fmax
    step = math.log(6.4) / 27.0

    def mel(f):
        return f / (200.0 / 3.0) if f < 1000.0 else 15.0 + math.log(f / 1000.0) / step

    def hz(m):
        return m * (200.0 / 3.0) if m < 15.0 else 1000.0 * math.exp(step * (m - 15.0))

    lo, hi = mel(fmin), mel(fmax)
    pts = [hz(lo + (hi - lo) * i / (n_mels + 1)) for i in range(n_mels + 2)]
    nb = nfft // 2 + 1
    W = torch.zeros(n_mels, nb, dtype=torch.float64)
    for j in range(n_mels):
        for k in range(nb):
            f = (sample_rate / 2) * k / (nb - 1)
            v = min((f - pts[j]) / (pts[j + 1] - pts[j]), (pts[j + 2] - f) / (pts[j + 2] - pts[j + 1]))
            W[j, k] = max(0.0, v) * 2.0 / (pts[j + 2] - pts[j])
    return W


_mel = {}


def _statement_mel(sample_rate, nfft):
    if (sample_rate, nfft) not in _mel:
        _mel[sample_rate, nfft] = statement_mel(sample_rate, nfft)
    return _mel[sample_rate, nfft]


def relief(y_pred, y_true, nfft=1024, hop=480, win=960, sample_rate=48000, energy_norm=False):
    """(edr_p, edr_t, clip), each (rows, 64, F), the first two in the dtype of the inputs: per row one torch.stft with the
    periodic Hann window of ``win`` samples, |X|^2, the mel projection, the backward integral over frames of its square, dB.
    ``clip`` is where the target's E is exactly 0 (its relief -inf); there the logarithm is given 1, so both entries hold 0 dB
    and no 0 * inf reaches a gradient.  Under ``energy_norm`` a band with E[0] = 0 is divided by 1: it stays 0 and is clipped."""
    B, T, N = y_pred.shape
    W = _statement_mel(sample_rate, nfft).to(y_pred.dtype)
    window = torch.hann_window(win, periodic=True, dtype=y_pred.dtype)
    out = []
    for y in (y_pred, y_true):
        rows = []
        for b in range(B):
            for c in range(N):
                X = torch.stft(y[b, :, c], n_fft=nfft, hop_length=hop, win_length=win, window=window, center=True,
                               pad_mode="reflect", return_complex=True)
                assert tuple(X.shape) == (nfft // 2 + 1, 1 + T // hop)
                m = W @ (X.real.square() + X.imag.square())
                E = m.square().flip(-1).cumsum(-1).flip(-1)
                if energy_norm:
                    E = E / torch.where(E[:, :1] == 0, torch.ones_like(E[:, :1]), E[:, :1])
                rows.append(E)
        out.append(torch.stack(rows))
    clip = out[1] == 0
    return [10 * torch.log10(torch.where(clip, torch.ones_like(E), E)) for E in out] + [clip]


def statement(y_pred, y_true, **kw):
    """The criterion of (B, T, N) signals as the issue states it: where the target's relief is -inf both entries become
    finfo(dtype).eps; sum |edr_t - edr_p| / sum |edr_t| over everything at once."""
    ep, et, clip = relief(y_pred, y_true, **kw)
    eps = torch.full_like(et, torch.finfo(et.dtype).eps)
    ep, et = torch.where(clip, eps, ep), torch.where(clip, eps, et)
    return (et - ep).abs().sum() / et.abs().sum()


def edr_signals(shape, seed, tail=0):
    """``signals`` of tests/test_mrstft_host.py (noise under -60 / -50 dB envelopes, float64 with float32 values) with the
    last ``tail`` samples of the TARGET exactly zero"""
    yp, yt = signals(shape, seed)
    if tail:
        yt[:, shape[1] - tail:] = 0.0
    return yp, yt


def statement_grad(yp, yt, cotangent=1.0, **kw):
    y = yp.clone().requires_grad_(True)
    loss = statement(y, yt, **kw)
    (g,) = torch.autograd.grad(cotangent * loss, [y])
    return loss.detach(), g


# name -> (shape, seed, zeroed tail of the target, class options)
CASES = {
    "shortest": ((1, 513, 1), 1, 0, {}),                 # T = nfft / 2 + 1: both frames reach both reflected ends
    "rows": ((2, 4800, 3), 2, 0, {}),
    "odd": ((1, 2603, 2), 3, 0, {}),
    "tail": ((1, 4800, 2), 4, 1500, {}),                 # 3 of 11 frames of the target are silent: clipped
    "small": ((1, 700, 2), 6, 0, dict(sample_rate=8000, nfft=256)),                          # 2 complex values per lane
    "big": ((1, 2603, 1), 7, 0, dict(sample_rate=96000, nfft=2048, overlap=0.75)),           # 16
    "mid": ((1, 1400, 1), 5, 0, dict(sample_rate=16000, nfft=512)),                          # 4
    "rows_norm": ((2, 4800, 3), 2, 0, dict(energy_norm=True)),
    "tail_norm": ((1, 4800, 2), 4, 1500, dict(energy_norm=True)),
}
FRAMES = {"shortest": 2, "rows": 11, "odd": 6, "tail": 11, "small": 9, "big": 6, "mid": 9, "rows_norm": 11, "tail_norm": 11}


def crit_kw(opts, device="cpu"):
    """(the class's instance, the statement's keywords)"""
    from flamo_amd.optimize import edr_loss
    crit = edr_loss(device=device, **opts)
    hop = int(crit.win_length * (1 - crit.overlap))
    return crit, dict(nfft=crit.nfft, hop=hop, win=crit.win_length, sample_rate=crit.sample_rate, energy_norm=crit.energy_norm)


@pytest.mark.parametrize("name", list(CASES))
def test_torch_lines_agree_with_the_statement(name):
    shape, seed, tail, opts = CASES[name]
    crit, kw = crit_kw(opts)
    yp, yt = edr_signals(shape, seed, tail)
    want, gwant = statement_grad(yp, yt, 3.0, **kw)
    y = yp.clone().requires_grad_(True)
    got = crit(y, yt)
    assert got.dim() == 0 and got.dtype == torch.float64 and type(got.grad_fn).__name__ != "_EDRBackward"
    (g,) = torch.autograd.grad(3.0 * got, [y])
    assert torch.isfinite(got) and torch.isfinite(g).all() and 0.22 < want.item() < 0.36
    check_close(f"edr_host/{name}/loss", got.detach().reshape(1), want.reshape(1), 1e-12)
    check_close(f"edr_host/{name}/grad", g, gwant, 1e-12)


@pytest.mark.parametrize("name", list(CASES))
def test_signals_keep_signs_and_clips_apart(name):
    """every unclipped |edr_t - edr_p| is at least 1e-4 dB (frame 0 excepted under energy_norm, where it is an exact 0 on both
    sides), so no sign flips between the precisions; the clipped share of the tail cases is 3 frames of 11"""
    shape, seed, tail, opts = CASES[name]
    kw = crit_kw(opts)[1]
    ep, et, clip = relief(*edr_signals(shape, seed, tail), **kw)
    assert ep.shape == (shape[0] * shape[2], 64, FRAMES[name])
    diff = (et - ep).abs()
    if kw["energy_norm"]:
        assert torch.count_nonzero(ep[..., 0]) == 0 and torch.count_nonzero(et[..., 0]) == 0
        diff, keep = diff[..., 1:], ~clip[..., 1:]
    else:
        keep = ~clip
    assert torch.isfinite(ep).all() and torch.isfinite(diff[keep]).all()
    print(f"[cond] {name}: min |edr_t - edr_p| {diff[keep].min().item():.2e} dB, clipped {clip.double().mean().item():.3f}")
    assert diff[keep].min() >= 1e-4
    share = clip.double().mean().item()
    if tail:
        assert 0 < share <= 0.3 and clip[..., -3:].all() and not clip[..., :-3].any()
    else:
        assert share == 0


def silent_channel(shape, seed):
    """``edr_signals`` with the last channel exactly zero in BOTH signals: every band of that row is clipped in every frame"""
    yp, yt = edr_signals(shape, seed)
    yp[..., -1] = 0.0
    yt[..., -1] = 0.0
    return yp, yt


@pytest.mark.parametrize("energy_norm", [False, True])
def test_band_silent_in_both_signals_is_clipped_and_takes_no_gradient(energy_norm):
    """a row that is silent in prediction and target adds eps per entry to the denominator and nothing else: the loss and the
    gradient are finite (no 0 / 0 from E / E[0], no 0 * inf from the logarithm) and the silent row's gradient is 0"""
    crit, kw = crit_kw(dict(energy_norm=energy_norm))
    yp, yt = silent_channel((1, 2603, 2), 3)
    want, gwant = statement_grad(yp, yt, 3.0, **kw)
    assert relief(yp, yt, **kw)[2].double().mean() == 0.5
    y = yp.clone().requires_grad_(True)
    got = crit(y, yt)
    (g,) = torch.autograd.grad(3.0 * got, [y])
    assert torch.isfinite(want) and torch.isfinite(gwant).all() and torch.isfinite(got) and torch.isfinite(g).all()
    assert torch.count_nonzero(gwant[..., 1]) == 0 and torch.count_nonzero(g[..., 1]) == 0
    check_close(f"edr_host/silent{int(energy_norm)}/loss", got.detach().reshape(1), want.reshape(1), 1e-12)
    check_close(f"edr_host/silent{int(energy_norm)}/grad", g, gwant, 1e-12)


def test_float32_host_tensors_take_the_torch_lines():
    crit, kw = crit_kw({})
    yp, yt = edr_signals((2, 2603, 1), 5)
    got = crit(yp.float(), yt.float())
    assert got.dtype == torch.float32
    check_close("edr_host/f32/loss", got.double().reshape(1), statement(yp, yt, **kw).reshape(1), 2e-6)


def test_constructor_attributes_and_defaults():
    from flamo_amd import optimize
    from flamo_amd.optimize import edr_loss
    assert optimize.edr_loss is edr_loss
    sig = inspect.signature(edr_loss.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("nfft", 1024), ("overlap", 0.5), ("sample_rate", 48000), ("energy_norm", False), ("device", "cpu"), ("name", "EDR")]
    crit = edr_loss()
    assert (crit.nfft, crit.overlap, crit.sample_rate, crit.energy_norm, crit.device, crit.name, crit.win_length) == \
        (1024, 0.5, 48000, False, "cpu", "EDR", 960)
    assert edr_loss(sample_rate=8000).win_length == 160
    assert isinstance(crit, torch.nn.Module) and callable(crit._torch_forward) and not hasattr(crit, "get_edr")
    x = torch.randn(2, 1000, 3)
    assert crit.discard_last_n_percent(x, 0.5).shape == (2, 995, 3)
    # (..., F, N): the integral runs over the axis before the last
    z = torch.rand(2, 5, 7, 3, dtype=torch.float64)
    E, Z = crit.schroeder_backward_int(z)
    assert torch.equal(Z, torch.ones_like(z)) and torch.allclose(E[:, :, 0], z.square().sum(-2)) and torch.equal(E[:, :, -1], z[:, :, -1] ** 2)
    En, Zn = edr_loss(energy_norm=True).schroeder_backward_int(z)
    assert Zn.shape == (2, 5, 1, 3) and torch.equal(En[:, :, 0], torch.ones(2, 5, 3, dtype=torch.float64))
    m = crit.mel_stft(torch.randn(3, 2603, dtype=torch.float64))
    assert m.shape == (3, 64, 6) and m.dtype == torch.float64 and (m > 0).all()


def test_one_dimensional_inputs_and_the_shape_assertion():
    from flamo_amd.optimize import edr_loss
    crit = edr_loss()
    yp, yt = edr_signals((1, 1100, 1), 3)
    a = yp[0, :, 0].clone().requires_grad_(True)
    b = yp.clone().requires_grad_(True)
    la, lb = crit(a, yt[0, :, 0]), crit(b, yt)
    assert la.dim() == 0 and torch.equal(la, lb)
    assert torch.equal(torch.autograd.grad(la, [a])[0], torch.autograd.grad(lb, [b])[0][0, :, 0])
    with pytest.raises(AssertionError, match="same shape"):
        crit(torch.randn(1, 1100, 1), torch.randn(1, 1101, 1))
    with pytest.raises(AssertionError, match="same shape"):
        crit(torch.randn(1100, 2), torch.randn(1100, 2))


def test_target_that_takes_a_gradient_gets_one_on_the_host():
    from flamo_amd.optimize import edr_loss
    yp, yt = edr_signals((1, 1100, 2), 4)
    yt.requires_grad_(True)
    edr_loss()(yp, yt).backward()
    assert yt.grad is not None and torch.isfinite(yt.grad).all() and torch.count_nonzero(yt.grad) > 0


def test_op_refuses_host_tensors():
    from flamo_amd import ops
    y = torch.randn(1, 1100, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edr_loss(y, y.clone())


@pytest.mark.parametrize("sample_rate,nfft", [(48000, 1024), (8000, 256), (16000, 512), (96000, 2048)])
def test_mel_basis(sample_rate, nfft):
    from flamo_amd import ops
    W = ops.mel_basis(sample_rate, nfft)
    assert W.shape == (64, nfft // 2 + 1) and W.dtype == torch.float64 and not W.is_cuda
    assert torch.equal(W, ops.mel_basis(sample_rate, nfft, n_mels=64, fmin=20.0, fmax=sample_rate // 2))
    ref = _statement_mel(sample_rate, nfft)
    assert ((W - ref).abs().max() / ref.abs().max()).item() <= 1e-14
    assert (W >= 0).all() and torch.count_nonzero(W[:, 0]) == 0
    taps = (W > 0).sum(1)
    assert taps.min() >= 1                                      # no empty band
    for k in range(W.shape[1]):                                 # at most two bands per bin, and those consecutive
        js = torch.nonzero(W[:, k])[:, 0].tolist()
        assert len(js) <= 2 and (len(js) < 2 or js[1] == js[0] + 1), (k, js)
    area = W.sum(1) * sample_rate / nfft
    wide = taps >= 8
    assert wide.any() and ((area[wide] - 1).abs() <= 0.02).all()
    if (sample_rate, nfft) == (48000, 1024):
        assert int(taps.sum()) == 991 and int(taps.max()) == 62
    if (sample_rate, nfft) == (96000, 2048):
        assert int(taps.sum()) == 1972 and int(taps.max()) == 143


def test_mel_tables_hold_the_matrix():
    """the two tables the kernels read, expanded again, are the host matrix to the bit"""
    from flamo_amd import ops
    for sample_rate, nfft in ((48000, 1024), (8000, 256)):
        W = ops.mel_basis(sample_rate, nfft).numpy()
        idx, w, nnz = ops._edr_mel_tables(W)
        nb = nfft // 2 + 1
        assert idx.dtype.name == "int32" and idx.size == 192 + nb and w.dtype.name == "float64" and w.size == nnz + 2 * nb
        start, count, off, band = idx[:64], idx[64:128], idx[128:192], idx[192:]
        assert nnz == (W > 0).sum() and (band >= 0).all() and (band <= 62).all()
        fwd, bwd = 0 * W, 0 * W
        for j in range(64):
            assert 0 <= start[j] and start[j] + count[j] <= nb and 0 <= off[j] and off[j] + count[j] <= nnz
            fwd[j, start[j]:start[j] + count[j]] = w[off[j]:off[j] + count[j]]
        for k in range(nb):
            bwd[band[k], k], bwd[band[k] + 1, k] = w[nnz + 2 * k], w[nnz + 2 * k + 1]
        assert (fwd == W).all() and (bwd == W).all()


def test_sizes_the_kernels_take():
    from flamo_amd import ops
    ok = ops.edr_supported
    assert ok((1, 513, 1), 1024, 480, 960) and ok((4, 96000, 2), 1024, 480, 960) and ok((1, 129, 1), 256, 1, 1)
    assert not ok((1, 512, 1), 1024, 480, 960)                                  # T <= nfft / 2
    assert ok((1, 1 << 30, 1), 2048, 512, 2048) and not ok((1, (1 << 30) + 1, 1), 2048, 512, 2048)
    assert not ok((1, 1 << 30, 3), 256, 1, 256)                                 # 2^31 frames and more
    assert not ok((1, 4800, 1), 128, 32, 128) and not ok((1, 4800, 1), 4096, 32, 128)
    assert not ok((1, 4800, 1), 768, 32, 128) and not ok((1, 4800, 1), 512, 32, 513)
    assert not ok((1, 4800, 1), 512, 0, 512) and not ok((1, 4800, 1), 512, 32, 0) and not ok((1, 4800, 1), 512, 32.5, 512)
    assert not ok((4800,), 1024, 480, 960) and not ok((0, 4800, 1), 1024, 480, 960)


def _header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fl_[a-z0-9_]+)\s*\(", src)))


ENTRIES = ["fl_edr_band_doubles", "fl_edr_bwd_f32", "fl_edr_bwd_f64", "fl_edr_frames", "fl_edr_fwd_f32", "fl_edr_fwd_f64",
           "fl_edr_gframe_elems", "fl_edr_keep_doubles", "fl_edr_mel_doubles", "fl_edr_mel_ints"]


def test_sixth_header_is_bound_and_exported():
    from flamo_amd import _lib
    syms = _header_symbols("flamo_hip_edr.h")
    assert syms == ENTRIES and sorted(_lib._SIGNATURES_EDR) == ENTRIES
    assert not set(ENTRIES) & set(_lib.EXPORTS)
    for other in (_lib._SIGNATURES_EDC, _lib._SIGNATURES_AVGPOW, _lib._SIGNATURES_FDNATT, _lib._SIGNATURES_MRSTFT):
        assert not set(ENTRIES) & set(other)
    for name in ("fl_edr_fwd", "fl_edr_bwd"):
        assert _lib._SIGNATURES_EDR[name + "_f32"] == _lib._SIGNATURES_EDR[name + "_f64"]
    if os.path.exists(_lib.LIB_PATH):
        handle = ctypes.CDLL(_lib.LIB_PATH)
        for s in ENTRIES:
            assert hasattr(handle, s), f"{s} declared in include/flamo_hip_edr.h but not exported"
        L = _lib.lib()
        for name, (res, args) in _lib._SIGNATURES_EDR.items():
            fn = getattr(L, name)
            assert fn.restype is res and list(fn.argtypes) == args, name


def _built():
    from flamo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_query_entries_agree_with_the_python_side():
    from flamo_amd import ops
    L = _built()
    assert L.fl_edr_keep_doubles() == 1 and L.fl_edr_mel_ints(1024) == 192 + 513 and L.fl_edr_mel_doubles(1024, 991) == 991 + 1026
    assert L.fl_edr_frames(1, 513, 1, 1024, 480, 960) == 2 and L.fl_edr_frames(2, 4800, 3, 1024, 480, 960) == 11
    assert L.fl_edr_band_doubles(2, 4800, 3, 1024, 480, 960) == 6 * 11 * 64
    assert L.fl_edr_gframe_elems(2, 4800, 3, 1024, 480, 960) == 6 * 11 * 960
    for q in (L.fl_edr_frames, L.fl_edr_band_doubles, L.fl_edr_gframe_elems):
        assert q(1, 512, 1, 1024, 480, 960) == -1
    for shape, res in (((1, 1 << 30, 3), (256, 1, 256)), ((1, 4800, 1), (768, 32, 128)), ((1, 4800, 1), (512, 32, 513)),
                       ((1, 4800, 1), (512, 0, 512)), ((1, 4800, 1), (128, 32, 128)), ((0, 4800, 1), (1024, 480, 960)),
                       ((1, (1 << 30) + 1, 1), (2048, 512, 2048)), ((2, 2603, 2), (1024, 480, 960)),
                       ((1, 1 << 30, 1), (2048, 512, 2048)), ((1, 4800, 1), (4096, 32, 128))):
        assert (L.fl_edr_frames(*shape, *res) >= 0) == ops.edr_supported(shape, *res), (shape, res)


def test_entries_check_their_arguments():
    L = _built()
    one = ctypes.c_void_p(16)          # never dereferenced: the checks come first
    fwd_args = (("yp", one), ("spb", 513), ("spt", 1), ("spc", 1), ("yt", one), ("stb", 513), ("stt", 1), ("stc", 1), ("B", 1),
                ("T", 513), ("N", 1), ("nfft", 1024), ("hop", 480), ("win", 960), ("wtab", one), ("tw", one), ("melidx", one),
                ("melw", one), ("nnz", 991), ("energy_norm", 0), ("eps", 1e-7), ("mel", one), ("kept", one), ("rowsum", one),
                ("keep", one), ("loss", one), ("stream", None))
    bwd_args = (("yp", one), ("spb", 513), ("spt", 1), ("spc", 1), ("B", 1), ("T", 513), ("N", 1), ("nfft", 1024), ("hop", 480),
                ("win", 960), ("wtab", one), ("tw", one), ("melidx", one), ("melw", one), ("nnz", 991), ("mel", one), ("kept", one),
                ("keep", one), ("gloss", one), ("gmel", one), ("gframes", one), ("gy", one), ("stream", None))
    call = lambda fn, args, **kw: fn(*[kw.get(n, v) for n, v in args])
    fwd_ptrs = ("yp", "yt", "wtab", "tw", "melidx", "melw", "mel", "rowsum", "keep", "loss")          # (kept may be null)
    bwd_ptrs = ("yp", "wtab", "tw", "melidx", "melw", "mel", "kept", "keep", "gloss", "gmel", "gframes", "gy")
    for fn, args, ptrs in ((L.fl_edr_fwd_f32, fwd_args, fwd_ptrs), (L.fl_edr_fwd_f64, fwd_args, fwd_ptrs),
                           (L.fl_edr_bwd_f32, bwd_args, bwd_ptrs), (L.fl_edr_bwd_f64, bwd_args, bwd_ptrs)):
        for name in ptrs:
            assert call(fn, args, **{name: None}) == -1 and b"null" in L.fl_last_error(), name
        assert call(fn, args, T=512) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, nfft=768) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, B=0) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, nnz=-1) == -1 and b"mel table" in L.fl_last_error()
        assert call(fn, args, nnz=64 * 513 + 1) == -1 and b"mel table" in L.fl_last_error()
        assert call(fn, args, tw=ctypes.c_void_p(20)) == -1 and b"aligned" in L.fl_last_error()
    assert call(L.fl_edr_fwd_f32, fwd_args, eps=-1.0) == -1 and b"eps" in L.fl_last_error()
