"""ops.edr_loss / flamo_amd.optimize.edr_loss on the GPU (csrc/edr.hip).  The yardstick is always the float64 statement of the
definition evaluated on the CPU (tests/test_edr_host.py::statement), never the code under test.

Limits, the project's own (tests/test_mrstft_gpu.py, tests/test_objectives.py).  float64: loss and gradient to 1e-10 -- the
1 / E of the dB value is the only amplifier, and the float32 torch statement's own gradient error against float64 is 2e-7 .. 7e-7
on these signals, so float64 sits near 1e-15; 1e-10 is far below an indexing, window, mel-table or adjoint mistake (1e-3 and
above).  float32 loss: the streaming criteria's 2e-6.  float32 gradient: no constant -- the torch float32 statement is evaluated
on the same inputs on the CPU, and the kernels' l2 and max-norm errors against float64 must be at most twice its errors.  The
signals keep every unclipped |edr_t - edr_p| above 1e-4 dB (asserted on the CPU with the reference), so no sign flips between
the precisions.

Measured on an MI355X: float64 losses at 0 .. 8e-16 and gradients at 1.3e-15 .. 1.7e-14 l2; float32 losses at 2e-9 .. 5e-8 and
gradients at 3.1e-8 .. 3.7e-8 l2 (8e-8 max-norm) where the float32 statement is at 1.4e-7 .. 6.0e-7."""
import pytest
import torch

from conftest import check_close, maxerr, relerr
from test_edr_host import CASES as HOST_CASES, crit_kw, edr_signals, relief, silent_channel, statement_grad

COTANGENT = 3.0
NODE = "_EDRBackward"

# name -> (shape, seed, zeroed tail of the target, class options, planar memory)
CASES = {name: case + (False,) for name, case in HOST_CASES.items()}
CASES["planar"] = HOST_CASES["rows"] + (True,)                  # the same values behind a transposed (B, N, T) view
# F = 84 frames, T divisible by no hop: the relief and prefix kernels cut a row into 16 segments of 6 frames, so 14 segments
# are full and two wavefronts have none
CASES["long"] = ((1, 40013, 1), 8, 0, {}, False)
_ref = {}


def _reference(name):
    """signals, the float64 statement's loss and gradient (cotangent 3) and the float32 statement's gradient errors against
    them, all on the CPU, computed once; the conditions on the signals are asserted here"""
    shape, seed, tail, opts, _ = CASES[name]
    key = (shape, seed, tail, tuple(sorted(opts.items())))          # ("planar" shares the values of "rows")
    if key not in _ref:
        yp, yt = edr_signals(shape, seed, tail)
        kw = crit_kw(opts)[1]
        ep, et, clip = relief(yp, yt, **kw)
        keep = ~clip
        if kw["energy_norm"]:
            keep[..., 0] = False
        assert ((et - ep).abs()[keep] >= 1e-4).all() and (tail > 0) == bool(clip.any())
        loss, grad = statement_grad(yp, yt, COTANGENT, **kw)
        _, g32 = statement_grad(yp.float(), yt.float(), COTANGENT, **kw)
        _ref[key] = (yp, yt, loss, grad, relerr(g32.double(), grad), maxerr(g32.double(), grad))
    return _ref[key]


def _device(gpu, name, dtype, use_class=True):
    from flamo_amd import ops
    shape, seed, tail, opts, planar = CASES[name]
    yp, yt = _reference(name)[:2]
    crit, kw = crit_kw(opts, "cuda")
    if planar:
        B, T, N = shape
        leaf = yp.transpose(1, 2).contiguous().to(device=gpu, dtype=dtype).requires_grad_(True)
        y, t = leaf.transpose(1, 2), yt.transpose(1, 2).contiguous().to(device=gpu, dtype=dtype).transpose(1, 2)
        assert tuple(y.shape) == shape and y.stride() == (N * T, 1, T) and t.stride() == (N * T, 1, T)
    else:
        leaf = y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
        t = yt.to(device=gpu, dtype=dtype)
    loss = crit(y, t) if use_class else ops.edr_loss(y, t, **kw)
    assert loss.dim() == 0 and loss.dtype == dtype and type(loss.grad_fn).__name__ == NODE
    (g,) = torch.autograd.grad(COTANGENT * loss, [leaf])
    if planar:
        g = g.transpose(1, 2)
    assert tuple(g.shape) == shape and g.dtype == dtype
    return loss.detach().cpu().double(), g.cpu().double()


def _check(tag, name, dtype, got, g):
    yp, yt, loss, grad, l2_32, mx_32 = _reference(name)
    assert torch.isfinite(loss) and torch.isfinite(grad).all() and torch.isfinite(got) and torch.isfinite(g).all()
    if dtype == torch.float64:
        check_close(tag + "/loss", got.reshape(1), loss.reshape(1), 1e-10)
        check_close(tag + "/grad", g, grad, 1e-10)
        return
    check_close(tag + "/loss", got.reshape(1), loss.reshape(1), 2e-6)
    l2, mx = relerr(g, grad), maxerr(g, grad)
    print(f"[parity] {tag}/grad: l2 {l2:.3e}  max {mx:.3e}  (limit 2 x the float32 torch statement's: l2 {l2_32:.3e}  max {mx_32:.3e})")
    assert l2 <= 2 * l2_32, (tag, "l2", l2, l2_32)
    assert mx <= 2 * mx_32, (tag, "max-norm", mx, mx_32)


@pytest.mark.gpu
@pytest.mark.parametrize("via", ["class", "op"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(CASES))
def test_shapes_against_the_float64_statement(gpu, name, dtype, via):
    got, g = _device(gpu, name, dtype, use_class=via == "class")
    _check(f"edr_gpu/{name}_{str(dtype)[-2:]}_{via}", name, dtype, got, g)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_prediction_equal_to_a_clipped_target_gives_exact_zeros(gpu, dtype):
    """a prediction equal to the target, whose last three frames are clipped: every unclipped difference is an exact 0 and the
    clipped entries add nothing to the numerator, so the loss is an exact 0 and so is the gradient (sign(0) = 0)"""
    from flamo_amd import ops
    yt = _reference("tail")[1].to(device=gpu, dtype=dtype)
    y = yt.clone().requires_grad_(True)
    for norm in (False, True):
        loss = ops.edr_loss(y, yt, energy_norm=norm)
        (g,) = torch.autograd.grad(loss, [y])
        assert loss.item() == 0.0 and torch.count_nonzero(g) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("energy_norm", [False, True], ids=["plain", "norm"])
def test_band_silent_in_both_signals_takes_no_gradient(gpu, energy_norm, dtype):
    """one channel exactly zero in prediction and target: its bands are clipped in every frame (E[0] = 0 under energy_norm),
    the loss and the live channel's gradient are the statement's and the silent channel's gradient is an exact 0"""
    from flamo_amd import ops
    kw = crit_kw(dict(energy_norm=energy_norm))[1]
    yp, yt = silent_channel((1, 2603, 2), 3)
    loss, grad = statement_grad(yp, yt, COTANGENT, **kw)
    y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
    got = ops.edr_loss(y, yt.to(device=gpu, dtype=dtype), **kw)
    (g,) = torch.autograd.grad(COTANGENT * got, [y])
    got, g = got.detach().cpu().double(), g.cpu().double()
    assert torch.isfinite(got) and torch.isfinite(g).all() and torch.count_nonzero(g[..., 1]) == 0
    tol = 1e-10 if dtype == torch.float64 else 2e-6
    check_close(f"edr_gpu/silent_{'norm' if energy_norm else 'plain'}_{str(dtype)[-2:]}/loss", got.reshape(1), loss.reshape(1), tol)
    if dtype == torch.float64:
        check_close(f"edr_gpu/silent_{'norm' if energy_norm else 'plain'}_64/grad", g, grad, 1e-10)


@pytest.mark.gpu
def test_two_runs_are_bit_identical(gpu):
    from flamo_amd import ops
    for name in ("odd", "tail_norm"):
        yp, yt = _reference(name)[:2]
        kw = crit_kw(CASES[name][3])[1]
        for dtype in (torch.float32, torch.float64):
            runs = []
            for _ in range(2):
                y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
                loss = ops.edr_loss(y, yt.to(device=gpu, dtype=dtype), **kw)
                (g,) = torch.autograd.grad(loss, [y])
                runs.append((loss.detach().clone(), g.clone()))
            assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.gpu
def test_arguments_the_op_refuses_and_the_class_routes(gpu):
    from flamo_amd import ops
    from flamo_amd.optimize import edr_loss
    y = torch.randn(1, 1100, 2, device=gpu)
    with pytest.raises(ValueError, match="differ"):
        ops.edr_loss(y, torch.randn(1, 1101, 2, device=gpu))
    with pytest.raises(ValueError, match="differ"):
        ops.edr_loss(y, y.double())
    with pytest.raises(ValueError, match="float32 / float64"):
        ops.edr_loss(y.half(), y.half())
    with pytest.raises(ValueError, match="float32 / float64"):
        ops.edr_loss(y[0], y[0].clone())
    with pytest.raises(ValueError, match="no gradient"):
        ops.edr_loss(y, y.clone().requires_grad_(True))
    for frames in ((768, 64, 300), (512, 64, 513), (4096, 64, 300), (512, 0, 512), (512, 64.5, 512), (128, 32, 128)):
        with pytest.raises(ValueError, match="frames"):
            ops.edr_loss(y, y.clone(), *frames)
    with pytest.raises(ValueError, match="frames"):
        ops.edr_loss(y[:, :512], y[:, :512].clone())          # T <= nfft / 2
    with pytest.raises(ValueError, match="sample_rate"):
        ops.edr_loss(y, y.clone(), sample_rate=40)
    assert not ops.edr_supported((1, 512, 2), 1024, 480, 960) and ops.edr_supported((1, 1100, 2), 1024, 480, 960)
    loss = ops.edr_loss(y, y.clone() * 0.5)
    assert not loss.requires_grad and loss.grad_fn is None          # nothing to differentiate: nothing is kept
    # the class sends the same cases to its torch lines (float64 there, nfft 256: one small FFT plan made by the runtime)
    y = y.double()
    yg = y.clone().requires_grad_(True)
    t = (y * 0.5).requires_grad_(True)
    small = edr_loss(nfft=256, sample_rate=8000, device="cuda")
    assert small._on_kernels(yg, t.detach()) and not small._on_kernels(yg, t)
    loss = small(yg, t)
    assert type(loss.grad_fn).__name__ != NODE
    loss.backward()
    assert t.grad is not None and yg.grad is not None and torch.isfinite(t.grad).all() and torch.count_nonzero(t.grad) > 0
    assert type(small(yg, t.detach()).grad_fn).__name__ == NODE
    assert not small._on_kernels(yg, y.float()) and not small._on_kernels(yg.half(), y.half())
    assert not small._on_kernels(yg.cpu(), y.cpu())
    other = edr_loss(nfft=200, sample_rate=8000, device="cuda")          # a frame length the kernels do not take
    assert not other._on_kernels(yg, y * 0.5) and type(other(yg, y * 0.5).grad_fn).__name__ != NODE
    assert type(edr_loss(device="cuda")(yg, y * 0.5).grad_fn).__name__ == NODE


@pytest.mark.gpu
def test_criterion_on_a_shell(gpu):
    """parallelFilter(24 taps, 2 channels) -> Matrix(2, 2) at nfft 2048, one batch item, float64: loss and parameter gradients
    through the kernels against those through the class's torch lines on the same device"""
    from collections import OrderedDict
    from flamo_amd.optimize import edr_loss
    from flamo_amd.processor import dsp, system
    from test_mrstft_host import signals
    torch.manual_seed(21)
    nfft, N = 2048, 2
    dt = torch.float64
    kw = dict(nfft=nfft, alias_decay_db=0.0, device=gpu, dtype=dt)
    fir = dsp.parallelFilter(size=(24, N), requires_grad=True, **kw)
    mix = dsp.Matrix(size=(N, N), requires_grad=True, **kw)
    model = system.Shell(system.Series(OrderedDict(fir=fir, mix=mix)), dsp.FFT(nfft, dtype=dt), dsp.iFFT(nfft, dtype=dt))
    xs, ts = signals((1, nfft, N), 7)
    x, t = xs.to(gpu), ts.to(gpu)
    crit = edr_loss(nfft=256, sample_rate=8000, device="cuda")          # (the FFT plan of the routing test)
    params = [fir.param, mix.param]
    loss = crit(model(x), t)
    assert type(loss.grad_fn).__name__ == NODE
    got = torch.autograd.grad(COTANGENT * loss, params)
    ref = crit._torch_forward(model(x), t)
    want = torch.autograd.grad(COTANGENT * ref, params)
    check_close("edr_gpu/shell/loss", loss.detach().cpu().reshape(1), ref.detach().cpu().reshape(1), 1e-10)
    check_close("edr_gpu/shell/g_fir", got[0].cpu(), want[0].cpu(), 1e-10)
    check_close("edr_gpu/shell/g_mix", got[1].cpu(), want[1].cpu(), 1e-10)


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_graph(gpu):
    """one forward + backward captured with torch.cuda.graph and replayed twice on new input values returns the eager run's
    bits: nothing is read back and no allocation depends on the data"""
    from flamo_amd import ops
    shape = (2, 2603, 2)
    inputs = [edr_signals(shape, 30 + k, 700 * (k == 2)) for k in range(3)]          # (the last with clipped frames)
    eager = []
    for yp, yt in inputs:
        y = yp.to(device=gpu, dtype=torch.float32).requires_grad_(True)
        loss = ops.edr_loss(y, yt.to(device=gpu, dtype=torch.float32), energy_norm=True)
        (g,) = torch.autograd.grad(COTANGENT * loss, [y])
        eager.append((loss.detach().clone(), g.clone()))
    ys = inputs[0][0].to(device=gpu, dtype=torch.float32).requires_grad_(True)
    ts = inputs[0][1].to(device=gpu, dtype=torch.float32)

    def step():
        loss = ops.edr_loss(ys, ts, energy_norm=True)
        (g,) = torch.autograd.grad(COTANGENT * loss, [ys])
        return loss.detach(), g

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        loss_s, g_s = step()
    for k in (1, 2):
        with torch.no_grad():
            ys.copy_(inputs[k][0])
            ts.copy_(inputs[k][1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.isfinite(loss_s) and torch.equal(loss_s, eager[k][0]) and torch.equal(g_s, eager[k][1])
