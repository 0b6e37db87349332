"""ops.edc_loss / ops.edc_db / flamo_amd.optimize.edc_loss on the GPU (csrc/edc.hip): the recorded values of the reference's
broadband edc_loss, larger shapes against the class's host float64 lines, both memory layouts, padding, determinism, and the
criterion on the fused Shell pipeline.  Tolerances are those of the streaming criteria (tests/test_objectives.py): 2e-6 in
float32, 1e-13 in float64, on loss and gradient."""
import numpy as np
import pytest
import torch

from conftest import check_close
from test_edc_host import edc_cases

COTANGENT = 3.0


def _tol(dtype):
    return 2e-6 if dtype == torch.float32 else 1e-13


def _planar(y, pad_value=float("nan")):
    """the same (B, T, N) values as a signal-planar view: memory (B, N, pitch), pitch > T, the padding holds `pad_value`"""
    B, T, N = y.shape
    pitch = (T + 32) // 32 * 32 + 32
    mem = torch.full((B, N, pitch), pad_value, dtype=y.dtype, device=y.device)
    mem[..., :T] = y.movedim(1, -1)
    view = mem[..., :T].movedim(-1, 1)
    assert tuple(view.shape) == (B, T, N) and (not view.is_contiguous() or N == 1)
    return view


def _laid_out(y, planar):
    return _planar(y) if planar else y.contiguous()


def _signals(shape, seed):
    """(prediction, target) in float64 with float32 values: noise under per-channel exponential envelopes, -80 / -70 dB at the end"""
    B, T, N = shape
    gen = torch.Generator().manual_seed(seed)
    ramp = torch.arange(T, dtype=torch.float64)[None, :, None] / (T - 1)
    out = []
    for end_db in (-80.0, -70.0):
        ends = end_db - 1.5 * torch.arange(N, dtype=torch.float64)[None, None, :]
        out.append((torch.randn(B, T, N, dtype=torch.float64, generator=gen) * 10 ** (ends * ramp / 20)).float().double())
    return out


def _host(yp, yt, opts):
    """loss and gradient (cotangent 3) of the class's host lines in float64"""
    from flamo_amd.optimize import edc_loss
    y = yp.clone().requires_grad_(True)
    loss = edc_loss(is_broadband=True, **opts)(y, yt)
    (g,) = torch.autograd.grad(COTANGENT * loss, [y])
    return loss.detach(), g


def _device(gpu, yp, yt, opts, dtype, pred_planar, true_planar):
    from flamo_amd.optimize import edc_loss
    y = _laid_out(yp.to(device=gpu, dtype=dtype), pred_planar).requires_grad_(True)
    t = _laid_out(yt.to(device=gpu, dtype=dtype), true_planar)
    loss = edc_loss(is_broadband=True, device="cuda", **opts)(y, t)
    assert loss.dim() == 0 and loss.dtype == dtype and type(loss.grad_fn).__name__ == "_EDCLossBackward"
    (g,) = torch.autograd.grad(COTANGENT * loss, [y])
    assert tuple(g.shape) == tuple(yp.shape)
    return loss.detach().cpu().double(), g.cpu().double()


@pytest.fixture(scope="module")
def golden():
    return edc_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("planar", [False, True])
def test_golden_cases(gpu, golden, dtype, planar):
    for k, shape, opts, yp, yt, loss, grad in golden:
        got, g = _device(gpu, yp, yt, opts, dtype, planar, planar)
        tag = f"edc_gpu/golden{k}_{str(dtype)[-2:]}_{int(planar)}"
        check_close(tag + "/loss", got.reshape(1), loss.reshape(1), _tol(dtype))
        check_close(tag + "/grad", g, grad, _tol(dtype))
        keep = int(np.round(0.995 * shape[1]))
        assert torch.count_nonzero(g[:, keep:]) == 0


# (shape, seed, options, prediction planar, target planar); clip only at T <= 5000, where the target's curve moves by more per
# sample than float32 resolves at the -60 dB boundary (the guard below keeps every entry 1e-4 dB away from it)
LARGER = [
    ((2, 5000, 3), 1, dict(energy_norm=True, clip=True, convergence=True), False, True),
    ((1, 20011, 1), 2, dict(energy_norm=True, convergence=True), False, False),
    ((3, 2400, 8), 3, dict(clip=True), True, False),
    ((1, 3001, 16), 4, dict(energy_norm=True, clip=True, convergence=True), True, True),
    ((1, 192000, 1), 5, dict(energy_norm=True, convergence=True), False, False),
    ((2, 96000, 8), 6, dict(convergence=True), True, False),
]
_larger_ref = {}


def _larger(i):
    """signals and the host float64 result of LARGER[i], computed once"""
    if i not in _larger_ref:
        shape, seed, opts, _, _ = LARGER[i]
        yp, yt = _signals(shape, seed)
        _larger_ref[i] = (yp, yt) + _host(yp, yt, opts)
    return _larger_ref[i]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("i", range(len(LARGER)))
def test_larger_shapes_against_the_host_lines(gpu, i, dtype):
    from flamo_amd import _lib
    from flamo_amd.optimize import edc_loss
    shape, seed, opts, pred_planar, true_planar = LARGER[i]
    keep = int(np.round(0.995 * shape[1]))
    assert -(-keep // _lib.lib().fl_edc_tile()) >= 3          # at least three tiles per column: carries from both sides
    yp, yt, loss, grad = _larger(i)
    if opts.get("clip"):
        assert shape[1] <= 5000
        e = edc_loss(is_broadband=True, energy_norm=opts.get("energy_norm", False)).get_edc(yt)
        assert ((e - (e[:, :1] - 60)).abs().amin(dim=1) > 1e-4).all()
        frac = (e < e[:, :1] - 60).double().mean(dim=1)
        assert ((frac > 0.05) & (frac < 0.95)).all()
    got, g = _device(gpu, yp, yt, opts, dtype, pred_planar, true_planar)
    tag = f"edc_gpu/{'x'.join(map(str, shape))}_{str(dtype)[-2:]}"
    check_close(tag + "/loss", got.reshape(1), loss.reshape(1), _tol(dtype))
    check_close(tag + "/grad", g, grad, _tol(dtype))
    assert torch.count_nonzero(g[:, keep:]) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_curve_in_db(gpu, dtype):
    """ops.edc_db and the class's get_edc on the device against the host lines, both layouts; the curve is (B, T', N) contiguous"""
    from flamo_amd import ops
    from flamo_amd.optimize import edc_loss
    yp, _ = _signals((2, 2400, 5), 7)
    for energy_norm in (False, True):
        crit = edc_loss(is_broadband=True, energy_norm=energy_norm)
        ref = crit.get_edc(yp)
        for planar in (False, True):
            y = _laid_out(yp.to(device=gpu, dtype=dtype), planar)
            e = crit.get_edc(y)
            assert tuple(e.shape) == (2, 2388, 5) and e.is_contiguous() and e.dtype == dtype and not e.requires_grad
            assert torch.equal(e, ops.edc_db(y, energy_norm=energy_norm))
            check_close(f"edc_gpu/db_{str(dtype)[-2:]}_{int(energy_norm)}_{int(planar)}", e.cpu().double(), ref, _tol(dtype))
            if energy_norm:      # E[0] / Z is one to a few roundings (Z adds the tile sums, E[0] a carry and a scan)
                assert e[:, 0].abs().max() < 50 * torch.finfo(dtype).eps


@pytest.mark.gpu
def test_padding_is_neither_read_nor_written(gpu):
    """the planar prediction's padding holds NaN (a read would spoil the loss); the backward entry is handed a gradient buffer
    full of a sentinel and leaves the padded columns alone, writes exact zeros from T' to T"""
    from flamo_amd import _lib, ops
    shape, opts = (2, 1500, 3), dict(energy_norm=True, clip=True, convergence=True)
    yp, yt = _signals(shape, 8)
    y = _planar(yp.to(gpu).float()).requires_grad_(True)
    t = _planar(yt.to(gpu).float())
    loss = ops.edc_loss(y, t, **opts)
    assert torch.isfinite(loss)
    (g,) = torch.autograd.grad(loss, [y], retain_graph=True)          # (the node's saved tensors are read below)
    ref_loss, ref_g = _host(yp, yt, opts)
    check_close("edc_gpu/pad/loss", loss.detach().cpu().double().reshape(1), ref_loss.reshape(1), 2e-6)
    check_close("edc_gpu/pad/grad", g.cpu().double() * COTANGENT, ref_g, 2e-6)
    # the same backward launch into a buffer of this test's own
    ym, w, sums, den = loss.grad_fn.saved_tensors
    planar, pitch, B, T, Tk, N, energy_norm = loss.grad_fn.cfg
    assert planar == 1 and pitch > T and (B, T, N) == shape and Tk == 1492
    buf = torch.full((B, N, pitch), -7.0, device=gpu)
    one = torch.ones((), device=gpu)
    _lib.check(_lib.lib().fl_edc_bwd_f32(ym.data_ptr(), planar, B, T, Tk, N, pitch, sums[0].data_ptr(), w.data_ptr(), sums[1].data_ptr(),
                                         sums[2].data_ptr(), one.data_ptr(), den.data_ptr(), int(energy_norm), buf.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream), "edc_bwd")
    assert torch.equal(buf[..., :T].movedim(-1, 1), g)
    assert (buf[..., T:] == -7.0).all() and torch.count_nonzero(buf[..., Tk:T]) == 0


@pytest.mark.gpu
def test_two_runs_are_bit_identical(gpu):
    yp, yt = _signals((2, 5000, 3), 9)
    for dtype in (torch.float32, torch.float64):
        for opts in ({}, dict(energy_norm=True, clip=True, convergence=True)):
            runs = []
            for _ in range(2):
                from flamo_amd import ops
                y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
                loss = ops.edc_loss(y, yt.to(device=gpu, dtype=dtype), **opts)
                (g,) = torch.autograd.grad(loss, [y])
                runs.append((loss.detach().clone(), g.clone()))
            assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.gpu
def test_arguments_the_op_refuses(gpu):
    from flamo_amd import ops
    y = torch.randn(2, 300, 2, device=gpu)
    with pytest.raises(ValueError, match="differ"):
        ops.edc_loss(y, torch.randn(2, 300, 1, device=gpu))
    with pytest.raises(ValueError, match="differ"):
        ops.edc_loss(y, y.double())
    with pytest.raises(ValueError, match=r"\(B, T, N\)"):
        ops.edc_db(y[0])
    assert not ops.edc_loss(y, y.clone() * 0.5).requires_grad          # nothing to differentiate: no w is kept


@pytest.mark.gpu
def test_edc_on_the_fused_shell_against_oracle(gpu):
    """config-2 miniature (nfft 24000, 4 channels, batch 5, float32) on random input, trained under the criterion against a
    random target: loss and the gradients of the Matrix and GEQ parameters against the float64 oracle graph under the class's
    host lines -- the bars of test_mse_on_the_fused_shell_against_oracle -- and the same step replayed by GraphedStep"""
    from collections import OrderedDict
    from flamo_amd.graph import GraphedStep
    from flamo_amd.optimize import edc_loss
    from flamo_amd.processor import dsp, system
    from oracle import hotpath as O
    torch.manual_seed(11)
    nfft, N, B = 24000, 4, 5
    kw = dict(nfft=nfft, alias_decay_db=0.0, device=gpu, dtype=torch.float32)
    mat = dsp.Matrix(size=(N, N), requires_grad=True, **kw)
    geq = dsp.GEQ(size=(N, N), requires_grad=True, **kw)
    model = system.Shell(system.Series(OrderedDict(mix=mat, eq=geq)), dsp.FFT(nfft), dsp.iFFT(nfft))
    x = torch.randn(B, nfft, N, device=gpu)
    t = torch.randn(B, nfft, N, device=gpu)
    crit = edc_loss(is_broadband=True, device="cuda")
    loss = crit(model(x), t)
    assert type(loss.grad_fn).__name__ == "_EDCLossBackward"
    loss.backward()
    W, G = (p.detach().cpu().double().requires_grad_(True) for p in (mat.param, geq.param))
    yo = O.config2_forward(x.cpu().double(), W, G, nfft)
    ref = edc_loss(is_broadband=True)(yo, t.cpu().double())
    gW, gG = torch.autograd.grad(ref, [W, G])
    check_close("edc_shell/loss", loss.detach().cpu().double().reshape(1), ref.detach().reshape(1), 1e-5)
    check_close("edc_shell/g_W", mat.param.grad.cpu().double(), gW, 1e-5)
    check_close("edc_shell/g_geq", geq.param.grad.cpu().double(), gG, 1e-4)
    params = [mat.param, geq.param]
    gs = GraphedStep(lambda xx: crit(model(xx), t), (x,), params, warmup=2)
    for _ in range(2):
        lg = gs.replay()
    torch.cuda.synchronize()
    assert abs(lg.item() - loss.item()) <= 1e-6 * abs(loss.item())
    check_close("edc_shell/replay_g_W", mat.param.grad.cpu().double(), gW, 1e-5)
