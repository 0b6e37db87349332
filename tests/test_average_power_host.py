"""flamo_amd.optimize.AveragePower without a GPU: the class on host float64 tensors against the values recorded from the
reference's AveragePower (tests/golden/average_power.npz, tools/gen_golden.py::gen_average_power), its constructor, the shapes
it refuses, and the third header's place in the C ABI."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import check_close, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def average_power_cases():
    """[(index, T, options, y_pred, y_true, loss, gradient, the reference's float32 loss)] of the fixture, float64"""
    meta, arrays = load_golden("average_power")
    assert meta["cotangent"] == 3.0
    out = []
    for k, case in enumerate(meta["cases"]):
        si = case["signals"]
        opts = {n: (tuple(v) if isinstance(v, list) else v) for n, v in case["options"].items()}
        out.append((k, case["T"], opts, arrays[f"s{si}_y_pred"].double(), arrays[f"s{si}_y_true"].double(),
                    arrays[f"c{k}_loss"].double(), arrays[f"c{k}_grad"].double(), arrays[f"c{k}_loss_f32"].double()))
    return out


def last_used_sample(T, sj):
    """one past the last sample that a frame read by the smoothing covers: frames f <= sj (J - 1) + 63, frame f holds the
    samples 256 f - 512 .. 256 f + 511"""
    F = 1 + T // 256
    J = (F - 64) // sj + 1
    return min(T, 256 * (sj * (J - 1) + 63) + 512)


def test_fixture_holds_the_cases_the_criterion_is_specified_on():
    cases = average_power_cases()
    assert [(c[1], c[2]) for c in cases] == [(16128, {}), (17152, {}), (17152, dict(energy_norm=True, stride=(2, 3)))]
    for _, T, _, yp, yt, loss, grad, loss32 in cases:
        assert tuple(yp.shape) == tuple(yt.shape) == tuple(grad.shape) == (T,) and loss.numel() == 1 and loss32.numel() == 1
        for y in (yp, yt):
            assert torch.equal(y.float().double(), y) and torch.equal(y.bfloat16().double(), y) and (y != 0).all()
    assert torch.equal(cases[1][3], cases[2][3]) and torch.equal(cases[1][4], cases[2][4])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "average_power.npz")) < 600 * 1024


def test_class_on_host_float64_reproduces_the_reference():
    from flamo_amd.optimize import AveragePower
    for k, T, opts, yp, yt, loss, grad, _ in average_power_cases():
        y = yp.clone().requires_grad_(True)
        got = AveragePower(**opts)(y, yt)
        (g,) = torch.autograd.grad(3.0 * got, [y])
        tag = f"average_power_host/{k}"
        check_close(tag + "/loss", got.detach().reshape(1), loss.reshape(1), 1e-13)
        check_close(tag + "/grad", g, grad, 1e-12)


def test_gradient_is_zero_beyond_the_last_used_frame():
    """T = 20000: F = 79 frames, J = 4 columns, frames 76 .. 78 unread -- every sample from 256 * 75 + 512 on gets an exact zero
    (the right-hand reflection belongs to unread frames too), every one before it a gradient"""
    from flamo_amd.optimize import AveragePower
    torch.manual_seed(3)
    T = 20000
    env = 10 ** (-3 * torch.arange(T, dtype=torch.float64) / T)
    y = (torch.randn(T, dtype=torch.float64) * env).requires_grad_(True)
    t = torch.randn(T, dtype=torch.float64) * env
    (g,) = torch.autograd.grad(AveragePower()(y, t), [y])
    end = last_used_sample(T, 4)
    assert end == 256 * 75 + 512 < T
    assert torch.count_nonzero(g[end:]) == 0 and torch.count_nonzero(g[:end]) == end
    assert last_used_sample(16128, 4) == 16128 and last_used_sample(17152, 4) == 17152 and last_used_sample(17152, 3) == 17152


def test_constructor_attributes_and_defaults():
    from flamo_amd.optimize import AveragePower
    sig = inspect.signature(AveragePower.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("energy_norm", False), ("name", "Average Power"), ("stride", (4, 4)), ("device", "cpu")]
    crit = AveragePower()
    assert (crit.energy_norm, crit.name, crit.stride, crit.device) == (False, "Average Power", (4, 4), "cpu")
    crit = AveragePower(True, "ap", (2, 3), "cuda")
    assert (crit.energy_norm, crit.name, crit.stride, crit.device) == (True, "ap", (2, 3), "cuda")
    h = torch.hann_window(64, dtype=torch.float64)
    assert torch.equal(crit.window2d(h), h[:, None] * h[None, :])
    for name in ("forward", "average_power", "window2d", "_torch_forward"):
        assert callable(getattr(crit, name))


def test_one_dimensional_and_three_dimensional_inputs_agree():
    from flamo_amd.optimize import AveragePower
    torch.manual_seed(5)
    T = 17200          # 68 frames: two columns (with one, the reference's squeeze() drops the axis)
    yp, yt = torch.randn(T, dtype=torch.float64), torch.randn(T, dtype=torch.float64)
    for opts in ({}, dict(energy_norm=True, stride=(2, 3))):
        crit = AveragePower(**opts)
        a = yp.clone().requires_grad_(True)
        b = yp.clone().requires_grad_(True)
        la, lb = crit(a, yt), crit(b[None, :, None], yt[None, :, None])
        assert la.dim() == 0 and torch.equal(la, lb)
        assert torch.equal(torch.autograd.grad(la, [a])[0], torch.autograd.grad(lb, [b])[0])
    loss, S1, S2 = AveragePower().average_power(yp[None, :, None], yt[None, :, None])
    assert tuple(S1.shape) == tuple(S2.shape) == (113, 1 + (1 + T // 256 - 64) // 4) and loss.dim() == 0


def test_shapes_the_reference_rejects_raise():
    from flamo_amd.optimize import AveragePower
    crit = AveragePower()
    with pytest.raises(RuntimeError):
        crit(torch.randn(2, 16128, 1), torch.randn(2, 16128, 1))
    with pytest.raises(RuntimeError):
        crit(torch.randn(1, 16128, 2), torch.randn(1, 16128, 2))
    with pytest.raises(RuntimeError):
        crit(torch.randn(16127), torch.randn(16127))
    with pytest.raises(AssertionError, match="same shape"):
        crit(torch.randn(1, 16128, 1), torch.randn(1, 16129, 1))


def test_target_that_takes_a_gradient_gets_one_on_the_host():
    from flamo_amd.optimize import AveragePower
    torch.manual_seed(6)
    yp, yt = torch.randn(16128, dtype=torch.float64), torch.randn(16128, dtype=torch.float64, requires_grad=True)
    AveragePower()(yp, yt).backward()
    assert yt.grad is not None and torch.count_nonzero(yt.grad) == yt.numel()


def test_op_refuses_host_tensors():
    from flamo_amd import ops
    y = torch.randn(16128)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.average_power(y, y.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.average_power(y[None, :, None], y.clone()[None, :, None], stride=(2, 3))


def _header_symbols(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fl_[a-z0-9_]+)\s*\(", src)))


def test_third_header_is_exported_and_bound():
    from flamo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    syms = _header_symbols("flamo_hip_avgpow.h")
    assert len(syms) == 7 and sorted(_lib._SIGNATURES_AVGPOW) == syms
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(handle, s), f"{s} declared in include/flamo_hip_avgpow.h but not exported"
    L = _lib.lib()
    for name, (res, args) in _lib._SIGNATURES_AVGPOW.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
        if name.endswith("_f32"):
            assert _lib._SIGNATURES_AVGPOW[name[:-4] + "_f64"] == (res, args), name
    assert sum(n.endswith("_f32") for n in syms) == 2 and sum(n.endswith("_f64") for n in syms) == 2
    # the main table is still the main header's, and no name is declared in two headers
    main, edc = _header_symbols("flamo_hip.h"), _header_symbols("flamo_hip_edc.h")
    assert sorted(_lib.EXPORTS) == main and _lib.EXPORTS == tuple(_lib._SIGNATURES) and len(main) == 183
    assert sorted(_lib._SIGNATURES_EDC) == edc and len(edc) == 9
    assert not set(main) & set(syms) and not set(edc) & set(syms) and not set(main) & set(edc)


def test_query_entries():
    from flamo_amd import _lib
    L = _lib.lib()
    assert L.fl_avgpow_frames(16128) == 64 and L.fl_avgpow_frames(96000) == 376 and L.fl_avgpow_frames(16127) == -1
    assert L.fl_avgpow_frames((1 << 30) + 1) == -1 and L.fl_avgpow_frames(-5) == -1
    # Q[2][F][I] and three partial sums per workgroup of 256 entries of P; 4 scalars and P1, P2
    assert L.fl_avgpow_work_doubles(16128, 4, 4) == 2 * 64 * 113 + 3 and L.fl_avgpow_keep_doubles(16128, 4, 4) == 4 + 2 * 113
    assert L.fl_avgpow_work_doubles(24000, 2, 3) == 2 * 94 * 225 + 3 * ((225 * 11 + 255) // 256)
    assert L.fl_avgpow_keep_doubles(24000, 2, 3) == 4 + 2 * 225 * 11
    for bad in ((16000, 4, 4), (16128, 0, 4), (16128, 4, -1)):
        assert L.fl_avgpow_work_doubles(*bad) == -1 and L.fl_avgpow_keep_doubles(*bad) == -1


def test_entries_check_their_arguments():
    from flamo_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: the checks come first
    odd = ctypes.c_void_p(24)
    fwd = lambda fn, **kw: fn(*[kw.get(n, d) for n, d in (("yp", one), ("sp", 1), ("yt", one), ("st", 1), ("T", 16128), ("si", 4), ("sj", 4),
                                                          ("w", one), ("h", one), ("tw", one), ("work", one), ("keep", one), ("P1", one),
                                                          ("P2", one), ("loss", one), ("stream", None))])
    bwd = lambda fn, **kw: fn(*[kw.get(n, d) for n, d in (("yp", one), ("sp", 1), ("T", 16128), ("si", 4), ("sj", 4), ("w", one), ("h", one),
                                                          ("tw", one), ("keep", one), ("gloss", one), ("gframes", one), ("gy", one),
                                                          ("stream", None))])
    for fn in (L.fl_avgpow_fwd_f32, L.fl_avgpow_fwd_f64):
        for name in ("yp", "yt", "w", "h", "tw", "work", "keep", "P1", "P2", "loss"):
            assert fwd(fn, **{name: None}) == -1 and b"null" in L.fl_last_error(), name
        assert fwd(fn, T=16127) == -1 and b"bad sizes" in L.fl_last_error()
        assert fwd(fn, T=(1 << 30) + 1) == -1 and b"bad sizes" in L.fl_last_error()
        assert fwd(fn, si=0) == -1 and b"bad sizes" in L.fl_last_error()
        assert fwd(fn, sj=-2) == -1 and b"bad sizes" in L.fl_last_error()
        assert fwd(fn, sp=0) == -1 and b"strides" in L.fl_last_error()
        assert fwd(fn, st=-1) == -1 and b"strides" in L.fl_last_error()
    assert fwd(L.fl_avgpow_fwd_f32, w=ctypes.c_void_p(20)) == -1 and b"aligned" in L.fl_last_error()
    assert fwd(L.fl_avgpow_fwd_f64, w=odd) == -1 and b"aligned" in L.fl_last_error()
    for fn in (L.fl_avgpow_bwd_f32, L.fl_avgpow_bwd_f64):
        for name in ("yp", "w", "h", "tw", "keep", "gloss", "gframes", "gy"):
            assert bwd(fn, **{name: None}) == -1 and b"null" in L.fl_last_error(), name
        assert bwd(fn, T=100) == -1 and b"bad sizes" in L.fl_last_error()
        assert bwd(fn, si=0) == -1 and bwd(fn, sj=0) == -1
        assert bwd(fn, sp=0) == -1 and b"stride" in L.fl_last_error()
    assert bwd(L.fl_avgpow_bwd_f64, gframes=odd) == -1 and b"aligned" in L.fl_last_error()
