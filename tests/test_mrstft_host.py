"""flamo_amd.optimize.MultiResoSTFT without a GPU: the class's torch lines against a second statement of the definition written
here (``statement``: torch.stft row by row, the norms and means written out), its gradient, the inputs that take the torch lines,
the sizes the kernels take, and the fifth header's place in the C ABI."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import check_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


def statement(y_pred, y_true, resolutions=DEFAULT, weights=(1.0, 1.0, 0.0), eps=1e-8):
    """The criterion of (B, T, N) signals as the issue states it: per resolution one torch.stft per row with the periodic Hann
    window of ``win`` samples, M = sqrt(clamp(re^2 + im^2, min=eps)), sc = |M_t - M_p|_F / |M_t|_F over everything at once,
    log = mean |log M_p - log M_t|, lin = mean |M_p - M_t|; the mean over the resolutions of the weighted three."""
    B, T, N = y_pred.shape
    w_sc, w_log, w_lin = weights
    total = 0.0
    for n_fft, hop, win in resolutions:
        window = torch.hann_window(win, periodic=True, dtype=y_pred.dtype, device=y_pred.device)
        diff2 = true2 = log1 = lin1 = 0.0
        count = 0
        for b in range(B):
            for c in range(N):
                M = []
                for y in (y_pred, y_true):
                    X = torch.stft(y[b, :, c], n_fft=n_fft, hop_length=hop, win_length=win, window=window, center=True,
                                   pad_mode="reflect", return_complex=True)
                    assert tuple(X.shape) == (n_fft // 2 + 1, 1 + T // hop)
                    M.append((X.real.square() + X.imag.square()).clamp(min=eps).sqrt())
                Mp, Mt = M
                diff2 = diff2 + (Mt - Mp).square().sum()
                true2 = true2 + Mt.square().sum()
                log1 = log1 + (Mp.log() - Mt.log()).abs().sum()
                lin1 = lin1 + (Mp - Mt).abs().sum()
                count += Mp.numel()
        total = total + w_sc * diff2.sqrt() / true2.sqrt() + w_log * log1 / count + w_lin * lin1 / count
    return total / len(resolutions)


def signals(shape, seed, silent=0):
    """(prediction, target), (B, T, N) float64 with float32 values: noise under exponential envelopes, -60 / -50 dB at the end
    (the signals of tests/test_average_power_gpu.py, one column per batch item and channel); the first `silent` samples of
    the prediction are exactly zero"""
    B, T, N = shape
    gen = torch.Generator().manual_seed(seed)
    ramp = (torch.arange(T, dtype=torch.float64) / (T - 1))[None, :, None]
    yp, yt = ((torch.randn(shape, dtype=torch.float64, generator=gen) * 10 ** (end_db * ramp / 20)).float().double()
              for end_db in (-60.0, -50.0))
    yp[:, :silent] = 0.0
    return yp, yt


def statement_grad(yp, yt, cotangent=1.0, **kw):
    y = yp.clone().requires_grad_(True)
    loss = statement(y, yt, **kw)
    (g,) = torch.autograd.grad(cotangent * loss, [y])
    return loss.detach(), g


CASES = [
    ((1, 1025, 1), {}, 0),
    ((2, 1500, 3), {}, 0),
    ((1, 2603, 2), dict(w_sc=0.5, w_log_mag=2.0, w_lin_mag=0.25), 0),
    ((1, 1400, 1), dict(fft_sizes=(512,), hop_sizes=(128,), win_lengths=(512,), w_sc=0.0, w_lin_mag=0.5), 600),
    ((1, 300, 2), dict(fft_sizes=(256, 100), hop_sizes=(64, 7), win_lengths=(100, 33), eps=1e-5), 0),
]


def _kw(opts):
    from flamo_amd.optimize import MultiResoSTFT
    crit = MultiResoSTFT(**opts)
    return crit, dict(resolutions=crit.resolutions(), weights=(crit.w_sc, crit.w_log_mag, crit.w_lin_mag), eps=crit.eps)


@pytest.mark.parametrize("i", range(len(CASES)))
def test_torch_lines_agree_with_the_statement(i):
    shape, opts, silent = CASES[i]
    crit, kw = _kw(opts)
    yp, yt = signals(shape, 10 + i, silent)
    want, gwant = statement_grad(yp, yt, 3.0, **kw)
    y = yp.clone().requires_grad_(True)
    got = crit(y, yt)
    assert got.dim() == 0 and got.dtype == torch.float64
    (g,) = torch.autograd.grad(3.0 * got, [y])
    assert torch.isfinite(got) and torch.isfinite(g).all()
    check_close(f"mrstft_host/{i}/loss", got.detach().reshape(1), want.reshape(1), 1e-12)
    check_close(f"mrstft_host/{i}/grad", g, gwant, 1e-12)
    if silent:      # the samples that only the frames 0 .. 2 (all under the clamp) hold: an exact zero there
        assert (shape, silent) == ((1, 1400, 1), 600) and torch.count_nonzero(g[:, :128]) == 0 and torch.count_nonzero(g[:, 128:]) > 0


def test_constructor_attributes_and_defaults():
    from flamo_amd import optimize
    from flamo_amd.optimize import MultiResoSTFT
    assert optimize.MultiResoSTFT is MultiResoSTFT
    sig = inspect.signature(MultiResoSTFT.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("fft_sizes", (1024, 2048, 512)), ("hop_sizes", (120, 240, 50)), ("win_lengths", (600, 1200, 240)), ("w_sc", 1.0),
        ("w_log_mag", 1.0), ("w_lin_mag", 0.0), ("eps", 1e-8), ("name", "MultiResoSTFT"), ("device", "cpu")]
    crit = MultiResoSTFT()
    assert crit.resolutions() == DEFAULT and crit.name == "MultiResoSTFT" and crit.device == "cpu"
    assert isinstance(crit, torch.nn.Module) and callable(crit._torch_forward)
    with pytest.raises(AssertionError, match="same"):
        MultiResoSTFT(fft_sizes=(512, 256), hop_sizes=(64,), win_lengths=(512, 256))


def test_one_dimensional_inputs_and_the_shape_assertion():
    from flamo_amd.optimize import MultiResoSTFT
    crit = MultiResoSTFT()
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
    with pytest.raises(RuntimeError):          # T <= n_fft / 2: what torch.stft raises for the reflect padding
        crit(torch.randn(1, 1024, 1), torch.randn(1, 1024, 1))


def test_target_that_takes_a_gradient_gets_one_on_the_host():
    from flamo_amd.optimize import MultiResoSTFT
    yp, yt = signals((1, 1100, 2), 4)
    yt.requires_grad_(True)
    MultiResoSTFT()(yp, yt).backward()
    assert yt.grad is not None and torch.count_nonzero(yt.grad) == yt.numel()


def test_float32_host_tensors_take_the_torch_lines():
    from flamo_amd.optimize import MultiResoSTFT
    yp, yt = signals((2, 1100, 1), 5)
    got = MultiResoSTFT()(yp.float(), yt.float())
    assert got.dtype == torch.float32
    check_close("mrstft_host/f32/loss", got.double().reshape(1), statement(yp, yt).reshape(1), 2e-6)


def test_op_refuses_host_tensors():
    from flamo_amd import ops
    y = torch.randn(1, 1100, 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mrstft_loss(y, y.clone())


def test_sizes_the_kernels_take():
    from flamo_amd import ops
    ok = ops.mrstft_supported
    assert ok((1, 1025, 1), DEFAULT) and ok((4, 96000, 2), DEFAULT) and ok((1, 129, 1), ((256, 1, 1),))
    assert not ok((1, 1024, 1), DEFAULT)                                  # T <= n_fft / 2
    assert ok((1, 1 << 30, 1), ((2048, 512, 2048),)) and not ok((1, (1 << 30) + 1, 1), ((2048, 512, 2048),))
    assert not ok((1, 1 << 30, 3), ((256, 1, 256),))                      # 2^31 frames and more
    assert not ok((1, 4800, 1), ((128, 32, 128),)) and not ok((1, 4800, 1), ((4096, 32, 128),))
    assert not ok((1, 4800, 1), ((768, 32, 128),)) and not ok((1, 4800, 1), ((512, 32, 513),))
    assert not ok((1, 4800, 1), ((512, 0, 512),)) and not ok((1, 4800, 1), ((512, 32, 0),))
    assert not ok((1, 4800, 1), ((512, 32.5, 512),)) and not ok((1, 4800, 1), ((512, 32),))
    assert not ok((1, 4800, 1), ()) and not ok((1, 4800, 1), ((256, 64, 256),) * 9) and ok((1, 4800, 1), ((256, 64, 256),) * 8)
    assert not ok((4800,), DEFAULT) and not ok((0, 4800, 1), DEFAULT) and not ok((1, 4800, 1), DEFAULT, eps=-1.0)


def _header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fl_[a-z0-9_]+)\s*\(", src)))


ENTRIES = ["fl_mrstft_blocks", "fl_mrstft_bwd_f32", "fl_mrstft_bwd_f64", "fl_mrstft_fwd_f32", "fl_mrstft_fwd_f64",
           "fl_mrstft_gframe_elems", "fl_mrstft_keep_doubles"]


def test_fifth_header_is_bound_and_exported():
    from flamo_amd import _lib
    syms = _header_symbols("flamo_hip_mrstft.h")
    assert syms == ENTRIES and sorted(_lib._SIGNATURES_MRSTFT) == ENTRIES
    assert not set(ENTRIES) & set(_lib.EXPORTS) and len(_lib.EXPORTS) == 183
    for other in (_lib._SIGNATURES_EDC, _lib._SIGNATURES_AVGPOW, _lib._SIGNATURES_FDNATT):
        assert not set(ENTRIES) & set(other)
    for name in ("fl_mrstft_fwd", "fl_mrstft_bwd"):
        assert _lib._SIGNATURES_MRSTFT[name + "_f32"] == _lib._SIGNATURES_MRSTFT[name + "_f64"]
    if os.path.exists(_lib.LIB_PATH):
        handle = ctypes.CDLL(_lib.LIB_PATH)
        for s in ENTRIES:
            assert hasattr(handle, s), f"{s} declared in include/flamo_hip_mrstft.h but not exported"
        L = _lib.lib()
        for name, (res, args) in _lib._SIGNATURES_MRSTFT.items():
            fn = getattr(L, name)
            assert fn.restype is res and list(fn.argtypes) == args, name


def _built():
    from flamo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def _cres(res):
    flat = [v for r in res for v in r]
    return (ctypes.c_int * len(flat))(*flat)


def test_query_entries_agree_with_the_python_side():
    from flamo_amd import ops
    L = _built()
    assert L.fl_mrstft_keep_doubles() == 65
    d = _cres(DEFAULT)
    # one workgroup per (resolution, row, frame); win samples of gradient per frame
    assert L.fl_mrstft_blocks(1, 1025, 1, 3, d) == 9 + 5 + 21
    assert L.fl_mrstft_gframe_elems(1, 1025, 1, 3, d) == 9 * 600 + 5 * 1200 + 21 * 240
    assert L.fl_mrstft_blocks(4, 96000, 2, 3, d) == 8 * (801 + 401 + 1921)
    assert L.fl_mrstft_blocks(1, 1024, 1, 3, d) == -1 and L.fl_mrstft_gframe_elems(1, 1024, 1, 3, d) == -1
    assert L.fl_mrstft_blocks(1, 1025, 1, 0, d) == -1 and L.fl_mrstft_blocks(1, 1025, 1, 3, None) == -1
    for shape, res in (((1, 1 << 30, 3), ((256, 1, 256),)), ((1, 4800, 1), ((768, 32, 128),)), ((1, 4800, 1), ((512, 32, 513),)),
                       ((1, 4800, 1), ((512, 0, 512),)), ((1, 4800, 1), ((128, 32, 128),)), ((0, 4800, 1), DEFAULT),
                       ((1, (1 << 30) + 1, 1), ((2048, 512, 2048),)), ((1, 4800, 1), ((256, 64, 256),) * 9),
                       ((2, 2603, 2), DEFAULT), ((1, 1 << 30, 1), ((2048, 512, 2048),))):
        want = ops.mrstft_supported(shape, res)
        assert (L.fl_mrstft_blocks(*shape, len(res), _cres(res)) >= 0) == want, (shape, res)


def test_entries_check_their_arguments():
    L = _built()
    one = ctypes.c_void_p(16)          # never dereferenced: the checks come first
    d = _cres(DEFAULT)
    fwd_args = (("yp", one), ("spb", 1025), ("spt", 1), ("spc", 1), ("yt", one), ("stb", 1025), ("stt", 1), ("stc", 1), ("B", 1),
                ("T", 1025), ("N", 1), ("R", 3), ("res", d), ("wtab", one), ("tw", one), ("w_sc", 1.0), ("w_log", 1.0),
                ("w_lin", 0.0), ("eps", 1e-8), ("partial", one), ("keep", one), ("loss", one), ("stream", None))
    bwd_args = fwd_args[:15] + (("eps", 1e-8), ("keep", one), ("gloss", one), ("gframes", one), ("gy", one), ("stream", None))
    call = lambda fn, args, **kw: fn(*[kw.get(n, v) for n, v in args])
    for fn, args, ptrs in ((L.fl_mrstft_fwd_f32, fwd_args, ("yp", "yt", "res", "wtab", "tw", "partial", "keep", "loss")),
                           (L.fl_mrstft_fwd_f64, fwd_args, ("yp", "yt", "res", "wtab", "tw", "partial", "keep", "loss")),
                           (L.fl_mrstft_bwd_f32, bwd_args, ("yp", "yt", "res", "wtab", "tw", "keep", "gloss", "gframes", "gy")),
                           (L.fl_mrstft_bwd_f64, bwd_args, ("yp", "yt", "res", "wtab", "tw", "keep", "gloss", "gframes", "gy"))):
        for name in ptrs:
            assert call(fn, args, **{name: None}) == -1 and b"null" in L.fl_last_error(), name
        assert call(fn, args, T=1024) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, R=9) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, B=0) == -1 and b"bad sizes" in L.fl_last_error()
        assert call(fn, args, eps=-1.0) == -1 and b"eps" in L.fl_last_error()
        assert call(fn, args, tw=ctypes.c_void_p(20)) == -1 and b"aligned" in L.fl_last_error()
