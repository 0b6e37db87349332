"""flamo_amd.optimize.edc_loss without a GPU: the class on host float64 tensors against the values recorded from the reference's
broadband edc_loss (tests/golden/edc_loss.npz, tools/gen_golden.py::gen_edc_loss), its constructor, the guards that keep the
-60 dB clip boundary from deciding a float32 comparison, and the second header's place in the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import check_close, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def edc_cases():
    """[(index, shape, options, y_pred, y_true, loss, gradient)] of the fixture, float64"""
    meta, arrays = load_golden("edc_loss")
    assert meta["cotangent"] == 3.0
    out = []
    for k, case in enumerate(meta["cases"]):
        si = case["signals"]
        out.append((k, tuple(case["shape"]), case["options"], arrays[f"s{si}_y_pred"].double(), arrays[f"s{si}_y_true"].double(),
                    arrays[f"c{k}_loss"].double(), arrays[f"c{k}_grad"].double()))
    return out


def test_fixture_holds_the_cases_the_criterion_is_specified_on():
    sets = [{}, {"energy_norm": True}, {"clip": True}, {"convergence": True}, {"energy_norm": True, "clip": True, "convergence": True}]
    cases = edc_cases()
    assert [(c[1], c[2]) for c in cases] == [((2, 1500, 3), o) for o in sets] + [((3, 777, 5), sets[0]), ((3, 777, 5), sets[-1])]
    for _, shape, _, yp, yt, loss, grad in cases:
        assert tuple(yp.shape) == tuple(yt.shape) == tuple(grad.shape) == shape and loss.numel() == 1
        for y in (yp, yt):
            assert torch.equal(y.float().double(), y) and (y != 0).all()          # float32 values, no exact zero
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "edc_loss.npz")) < 600 * 1024


def test_class_on_host_float64_reproduces_the_reference():
    from flamo_amd.optimize import edc_loss
    for k, shape, opts, yp, yt, loss, grad in edc_cases():
        y = yp.clone().requires_grad_(True)
        got = edc_loss(is_broadband=True, **opts)(y, yt)
        (g,) = torch.autograd.grad(3.0 * got, [y])
        tag = f"edc_host/{k}"
        check_close(tag + "/loss", got.detach().reshape(1), loss.reshape(1), 1e-13)
        check_close(tag + "/grad", g, grad, 1e-12)
        keep = int(np.round(0.995 * shape[1]))
        assert torch.count_nonzero(g[:, keep:]) == 0 and torch.count_nonzero(g[:, :keep]) == g[:, :keep].numel()


def test_clip_boundary_is_far_from_every_entry_of_the_clip_cases():
    """a float32 curve is about 1e-5 dB from the float64 one: no entry of the target's curve may sit within 1e-4 dB of the
    -60 dB boundary, and the clipped part of each column is neither nothing nor nearly all of it"""
    from flamo_amd.optimize import edc_loss
    n = 0
    for k, shape, opts, yp, yt, loss, grad in edc_cases():
        if not opts.get("clip"):
            continue
        n += 1
        e = edc_loss(is_broadband=True, energy_norm=opts.get("energy_norm", False)).get_edc(yt)
        bound = e[:, :1] - 60
        assert torch.equal(e.amax(dim=1, keepdim=True), e[:, :1])
        assert ((e - bound).abs().amin(dim=1) > 1e-4).all(), k
        frac = (e < bound).double().mean(dim=1)
        assert ((frac > 0.05) & (frac < 0.95)).all(), (k, frac)
    assert n == 3


def test_constructor_attributes_and_defaults():
    from flamo_amd.optimize import edc_loss
    import inspect
    sig = inspect.signature(edc_loss.__init__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("sample_rate", 48000), ("is_broadband", False), ("n_fractions", 1), ("energy_norm", False), ("convergence", False),
        ("clip", False), ("name", "EDC"), ("device", "cpu")]
    crit = edc_loss(is_broadband=True)
    assert (crit.sample_rate, crit.is_broadband, crit.n_fractions, crit.energy_norm, crit.convergence, crit.clip, crit.name,
            crit.device, crit.discard_n) == (48000, True, 1, False, False, False, "EDC", "cpu", 0.5)
    assert isinstance(crit.mse, torch.nn.MSELoss) and crit.mse.reduction == "mean"
    crit = edc_loss(44100, True, 3, True, True, True, "edc", "cuda")
    assert (crit.sample_rate, crit.n_fractions, crit.energy_norm, crit.convergence, crit.clip, crit.name, crit.device) == (
        44100, 3, True, True, True, "edc", "cuda")
    x = torch.arange(1.0, 401.0, dtype=torch.float64).reshape(1, 200, 2)
    assert crit.discard_last_n_percent(x, 0.5).shape == (1, 199, 2) and crit.discard_last_n_percent(x, 10).shape == (1, 180, 2)
    E, Z = crit.schroeder_backward_int(x)
    assert torch.equal(Z, (x ** 2).sum(1, keepdim=True)) and torch.equal(E[:, 0], torch.ones(1, 2, dtype=torch.float64))
    plain = edc_loss(is_broadband=True)
    E, Z = plain.schroeder_backward_int(x)
    assert torch.equal(Z, torch.ones_like(x)) and torch.equal(E[:, -1], x[:, -1] ** 2) and torch.equal(E[:, 0], (x ** 2).sum(1))
    assert torch.equal(plain.get_edc(x), 10 * torch.log10(plain.schroeder_backward_int(x[:, :199])[0]))


def test_subband_form_is_refused_at_construction():
    from flamo_amd.optimize import edc_loss
    with pytest.raises(NotImplementedError, match="pyfar"):
        edc_loss()
    with pytest.raises(NotImplementedError, match="fractional-octave"):
        edc_loss(is_broadband=False, n_fractions=3)


def test_one_dimensional_inputs_are_one_column():
    from flamo_amd.optimize import edc_loss
    torch.manual_seed(5)
    decay = torch.exp(-torch.arange(600, dtype=torch.float64) / 80)
    yp, yt = torch.randn(600, dtype=torch.float64) * decay, torch.randn(600, dtype=torch.float64) * decay
    for opts in ({}, dict(energy_norm=True, clip=True, convergence=True)):
        crit = edc_loss(is_broadband=True, **opts)
        a = yp.clone().requires_grad_(True)
        b = yp.clone().requires_grad_(True)
        la, lb = crit(a, yt), crit(b[None, :, None], yt[None, :, None])
        assert la.dim() == 0 and torch.equal(la, lb)
        assert torch.equal(torch.autograd.grad(la, [a])[0], torch.autograd.grad(lb, [b])[0])
    with pytest.raises(AssertionError, match="same shape"):
        edc_loss(is_broadband=True)(torch.randn(2, 50, 3), torch.randn(2, 50, 1))


def test_target_that_takes_a_gradient_gets_one_on_the_host():
    from flamo_amd.optimize import edc_loss
    torch.manual_seed(6)
    yp, yt = torch.randn(2, 300, 2, dtype=torch.float64), torch.randn(2, 300, 2, dtype=torch.float64, requires_grad=True)
    edc_loss(is_broadband=True, convergence=True)(yp, yt).backward()
    assert yt.grad is not None and torch.count_nonzero(yt.grad[:, :298]) == yt.grad[:, :298].numel()


def test_ops_refuse_host_tensors():
    from flamo_amd import ops
    y = torch.randn(1, 100, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edc_loss(y, y.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.edc_db(y)


def _edc_header_symbols():
    src = open(os.path.join(ROOT, "include", "flamo_hip_edc.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(fl_[a-z0-9_]+)\s*\(", src)))


def test_second_header_is_exported_and_bound():
    from flamo_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    syms = _edc_header_symbols()
    assert len(syms) == 9 and sorted(_lib._SIGNATURES_EDC) == syms
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(handle, s), f"{s} declared in include/flamo_hip_edc.h but not exported"
    L = _lib.lib()
    for name, (res, args) in _lib._SIGNATURES_EDC.items():
        fn = getattr(L, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    for name, sig in _lib._SIGNATURES_EDC.items():
        if name.endswith("_f32"):
            assert _lib._SIGNATURES_EDC[name[:-4] + "_f64"] == sig, name
    assert sum(n.endswith("_f32") for n in syms) == 4
    # the main table is still the main header's, and no name is declared twice
    main = open(os.path.join(ROOT, "include", "flamo_hip.h")).read()
    main = sorted(set(re.findall(r"\b(fl_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S))))
    assert sorted(_lib.EXPORTS) == main and _lib.EXPORTS == tuple(_lib._SIGNATURES) and not set(main) & set(syms)
    tile = L.fl_edc_tile()
    assert tile > 0 and tile % 64 == 0


def test_entries_check_their_arguments():
    from flamo_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)          # never dereferenced: the size checks come first
    assert L.fl_edc_tile_sums_f32(None, 0, 1, 100, 99, 1, 100, None, None) == -1 and b"null" in L.fl_last_error()
    assert L.fl_edc_tile_sums_f32(one, 0, 1, 100, 101, 1, 100, one, None) == -1 and b"bad sizes" in L.fl_last_error()
    assert L.fl_edc_tile_sums_f64(one, 1, 1, 100, 99, 1, 96, one, None) == -1 and b"pitch" in L.fl_last_error()
    assert L.fl_edc_bwd_f64(one, 0, 0, 100, 99, 1, 100, one, one, one, one, one, None, 0, one, None) == -1
