"""ops.average_power / flamo_amd.optimize.AveragePower on the GPU (csrc/avgpow.hip): the recorded values of the reference's
class, further shapes and strides against the class's host float64 lines, a prediction with a silent onset, the smoothed
spectrograms, determinism, the op's refusals, strided views, and the criterion on a Shell.  Tolerances: 1e-12 in float64 and
the streaming criteria's 2e-6 in float32 (tests/test_objectives.py), on loss and gradient."""
import pytest
import torch

from conftest import check_close, check_closer
from test_average_power_host import average_power_cases, last_used_sample

COTANGENT = 3.0


def _tol(dtype):
    return 2e-6 if dtype == torch.float32 else 1e-12


def _signals(T, seed, silent=0):
    """(prediction, target), (T,) float64 with float32 values: noise under exponential envelopes, -60 / -50 dB at the end; the
    prediction's first `silent` samples are exactly zero"""
    gen = torch.Generator().manual_seed(seed)
    ramp = torch.arange(T, dtype=torch.float64) / (T - 1)
    yp, yt = ((torch.randn(T, dtype=torch.float64, generator=gen) * 10 ** (end_db * ramp / 20)).float().double()
              for end_db in (-60.0, -50.0))
    yp[:silent] = 0.0
    return yp, yt


def _host(yp, yt, opts):
    """loss, gradient (cotangent 3) and the smoothed spectrograms of the class's host lines in float64"""
    from flamo_amd.optimize import AveragePower
    y = yp.clone().requires_grad_(True)
    crit = AveragePower(**opts)
    loss = crit(y, yt)
    (g,) = torch.autograd.grad(COTANGENT * loss, [y])
    with torch.no_grad():
        _, P1, P2 = crit.average_power(yp[None, :, None], yt[None, :, None])      # (without energy_norm's division)
    return loss.detach(), g, P1, P2


def _device(gpu, yp, yt, opts, dtype):
    from flamo_amd.optimize import AveragePower
    y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
    loss = AveragePower(device="cuda", **opts)(y, yt.to(device=gpu, dtype=dtype))
    assert loss.dim() == 0 and loss.dtype == dtype
    (g,) = torch.autograd.grad(COTANGENT * loss, [y])
    assert tuple(g.shape) == tuple(yp.shape) and g.dtype == dtype
    return loss.detach().cpu().double(), g.cpu().double()


@pytest.fixture(scope="module")
def golden():
    return average_power_cases()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_golden_cases(gpu, golden, dtype):
    for k, T, opts, yp, yt, loss, grad, loss32 in golden:
        got, g = _device(gpu, yp, yt, opts, dtype)
        tag = f"average_power_gpu/golden{k}_{str(dtype)[-2:]}"
        if dtype == torch.float32:      # ... and no farther from the float64 value than the reference's own float32 run
            check_closer(tag + "/loss", got.reshape(1), loss32.reshape(1), loss.reshape(1), _tol(dtype))
        else:
            check_close(tag + "/loss", got.reshape(1), loss.reshape(1), _tol(dtype))
        check_close(tag + "/grad", g, grad, _tol(dtype))


# (T, seed, options, samples of silence at the prediction's start, precisions)
BOTH = (torch.float64, torch.float32)
SHAPES = [
    (20000, 1, {}, 0, BOTH),                          # F = 79, J = 4, frames 76 .. 78 unread: the tail's gradient is zero
    (24000, 2, dict(stride=(2, 3)), 0, BOTH),
    (33000, 3, dict(stride=(8, 1)), 0, BOTH),
    (96000, 4, {}, 0, (torch.float32,)),
    (20000, 5, {}, 3000, BOTH),                       # whole frames with |X| = 0: the onset delay of a measured response
]
_ref = {}


def _reference(i):
    """signals and the host float64 result of SHAPES[i], computed once"""
    if i not in _ref:
        T, seed, opts, silent, _ = SHAPES[i]
        yp, yt = _signals(T, seed, silent)
        _ref[i] = (yp, yt) + _host(yp, yt, opts)
    return _ref[i]


@pytest.mark.gpu
@pytest.mark.parametrize("i,dtype", [(i, d) for i, s in enumerate(SHAPES) for d in s[4]])
def test_shapes_against_the_host_lines(gpu, i, dtype):
    T, seed, opts, silent, _ = SHAPES[i]
    yp, yt, loss, grad, _, _ = _reference(i)
    assert torch.isfinite(loss) and torch.isfinite(grad).all()
    got, g = _device(gpu, yp, yt, opts, dtype)
    assert torch.isfinite(got) and torch.isfinite(g).all()
    tag = f"average_power_gpu/{T}_{i}_{str(dtype)[-2:]}"
    check_close(tag + "/loss", got.reshape(1), loss.reshape(1), _tol(dtype))
    check_close(tag + "/grad", g, grad, _tol(dtype))
    end = last_used_sample(T, opts.get("stride", (4, 4))[1])
    assert torch.count_nonzero(g[end:]) == 0 and torch.count_nonzero(grad[end:]) == 0
    if i == 0:
        assert end == 19712 and torch.count_nonzero(g[:end]) == end


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_smoothed_spectrograms(gpu, dtype):
    """average_power() returns the loss and P1, P2 of the host lines; they take no gradient"""
    from flamo_amd import ops
    from flamo_amd.optimize import AveragePower
    for i in (1, 4):
        T, seed, opts, silent, _ = SHAPES[i]
        yp, yt, loss, _, P1, P2 = _reference(i)
        y = yp.to(device=gpu, dtype=dtype)[None, :, None].requires_grad_(True)
        t = yt.to(device=gpu, dtype=dtype)[None, :, None]
        got, S1, S2 = AveragePower(device="cuda", **opts).average_power(y, t)
        assert type(got.grad_fn).__name__ == "_AveragePowerBackward" and not S1.requires_grad and not S2.requires_grad
        assert tuple(S1.shape) == tuple(P1.shape) and S1.dtype == dtype
        tag = f"average_power_gpu/P_{T}_{i}_{str(dtype)[-2:]}"
        check_close(tag + "/loss", got.detach().cpu().double().reshape(1), loss.reshape(1), _tol(dtype))
        check_close(tag + "/P1", S1.cpu().double(), P1, _tol(dtype))
        check_close(tag + "/P2", S2.cpu().double(), P2, _tol(dtype))
        l2, Q1, Q2 = ops.average_power(y.detach(), t, stride=opts.get("stride", (4, 4)))
        assert torch.equal(l2, got.detach()) and torch.equal(Q1, S1) and torch.equal(Q2, S2)


@pytest.mark.gpu
def test_two_runs_are_bit_identical(gpu):
    from flamo_amd import ops
    yp, yt = _signals(24000, 9)
    for dtype in (torch.float32, torch.float64):
        for stride in ((4, 4), (2, 3)):
            runs = []
            for _ in range(2):
                y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
                loss, P1, P2 = ops.average_power(y, yt.to(device=gpu, dtype=dtype), stride=stride)
                (g,) = torch.autograd.grad(loss, [y])
                runs.append((loss.detach().clone(), g.clone(), P1.clone(), P2.clone()))
            assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.gpu
def test_arguments_the_op_refuses(gpu):
    from flamo_amd import ops
    y = torch.randn(16128, device=gpu)
    with pytest.raises(ValueError, match="differ"):
        ops.average_power(y, torch.randn(16129, device=gpu))
    with pytest.raises(ValueError, match="differ"):
        ops.average_power(y, y.double())
    with pytest.raises(ValueError, match="one real"):
        ops.average_power(torch.randn(2, 16128, 1, device=gpu), torch.randn(2, 16128, 1, device=gpu))
    with pytest.raises(ValueError, match="one real"):
        ops.average_power(torch.randn(1, 16128, 2, device=gpu), torch.randn(1, 16128, 2, device=gpu))
    with pytest.raises(ValueError, match="one real"):
        ops.average_power(y.half(), y.half())
    with pytest.raises(ValueError, match="fewer than 64 frames"):
        ops.average_power(y[:16127], y[:16127].clone())
    for stride in ((0, 4), (4, -1), (4,), 4, (2.5, 4)):
        with pytest.raises(ValueError, match="stride"):
            ops.average_power(y, y.clone(), stride=stride)
    loss, P1, P2 = ops.average_power(y, y.clone() * 0.5)
    assert not loss.requires_grad and loss.grad_fn is None          # nothing to differentiate: nothing is kept
    yg = y.clone().requires_grad_(True)
    loss, _, _ = ops.average_power(yg, y * 0.5)
    assert [tuple(s.shape) for s in loss.grad_fn.saved_tensors] == [(16128,), (4 + 2 * 113,)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_strided_views(gpu, dtype):
    """a (1, T, 1) view with a time stride of 3 (the op reads it in place; the class takes its torch lines for it) and one of
    a signal-planar row with padding behind it"""
    from flamo_amd import ops
    from flamo_amd.optimize import AveragePower
    T, seed, opts, _, _ = SHAPES[0]
    yp, yt, loss, grad, _, _ = _reference(0)
    wide = torch.full((1, T, 3), float("nan"), dtype=dtype, device=gpu)
    wide[:, :, 1] = yp.to(device=gpu, dtype=dtype)
    wide.requires_grad_(True)
    view = wide[:, :, 1:2]
    assert tuple(view.shape) == (1, T, 1) and view.stride(1) == 3
    tw = torch.full((1, T, 2), float("nan"), dtype=dtype, device=gpu)
    tw[:, :, 0] = yt.to(device=gpu, dtype=dtype)
    tag = f"average_power_gpu/strided_{str(dtype)[-2:]}"
    for n, fn in enumerate((lambda a, b: ops.average_power(a, b)[0], AveragePower(device="cuda"))):
        if n == 1 and dtype == torch.float32:
            continue      # the class's torch lines in float32 are the reference's float32 arithmetic: not held to this bar
        got = fn(view, tw[:, :, 0:1])
        assert (type(got.grad_fn).__name__ == "_AveragePowerBackward") == (n == 0)
        (g,) = torch.autograd.grad(COTANGENT * got, [wide])
        check_close(f"{tag}/{n}/loss", got.detach().cpu().double().reshape(1), loss.reshape(1), _tol(dtype))
        check_close(f"{tag}/{n}/grad", g[0, :, 1].cpu().double(), grad, _tol(dtype))
        assert torch.count_nonzero(g[0, :, 0]) == 0 and torch.count_nonzero(g[0, :, 2]) == 0
    mem = torch.full((1, 1, T + 96), float("nan"), dtype=dtype, device=gpu)
    mem[0, 0, :T] = yp.to(device=gpu, dtype=dtype)
    planar = mem[..., :T].movedim(-1, 1).requires_grad_(True)
    assert tuple(planar.shape) == (1, T, 1) and planar.stride(1) == 1
    got = AveragePower(device="cuda")(planar, yt.to(device=gpu, dtype=dtype)[None, :, None])
    assert type(got.grad_fn).__name__ == "_AveragePowerBackward"
    (g,) = torch.autograd.grad(COTANGENT * got, [planar])
    check_close(tag + "/planar/loss", got.detach().cpu().double().reshape(1), loss.reshape(1), _tol(dtype))
    check_close(tag + "/planar/grad", g[0, :, 0].cpu().double(), grad, _tol(dtype))


@pytest.mark.gpu
def test_average_power_on_a_shell_against_oracle(gpu):
    """Matrix(1, 1) -> GEQ(1, 1), nfft 24000, batch 1, float32, on random input under the criterion against a random target:
    loss and the gradients of the Matrix and GEQ parameters against the float64 oracle graph under the class's host lines --
    the bars of test_edc_on_the_fused_shell_against_oracle -- and the same step replayed by GraphedStep"""
    from collections import OrderedDict
    from flamo_amd.graph import GraphedStep
    from flamo_amd.optimize import AveragePower
    from flamo_amd.processor import dsp, system
    from oracle import hotpath as O
    torch.manual_seed(12)
    nfft, N, B = 24000, 1, 1
    kw = dict(nfft=nfft, alias_decay_db=0.0, device=gpu, dtype=torch.float32)
    mat = dsp.Matrix(size=(N, N), requires_grad=True, **kw)
    geq = dsp.GEQ(size=(N, N), requires_grad=True, **kw)
    model = system.Shell(system.Series(OrderedDict(mix=mat, eq=geq)), dsp.FFT(nfft), dsp.iFFT(nfft))
    x = torch.randn(B, nfft, N, device=gpu)
    t = torch.randn(B, nfft, N, device=gpu)
    crit = AveragePower(device="cuda")

    def eager_step():
        # The step's autograd graph must be gone before the capture below.  At batch 1 the Shell folds nothing and builds its
        # responses on the current stream, here the default one, and that is the stream the parameters' gradient accumulators
        # remember for as long as a graph holds them: autograd would pull the default stream into the capture.
        loss = crit(model(x), t)
        assert type(loss.grad_fn).__name__ == "_AveragePowerBackward"
        loss.backward()
        return loss.detach()

    loss = eager_step()
    W, G = (p.detach().cpu().double().requires_grad_(True) for p in (mat.param, geq.param))
    yo = O.config2_forward(x.cpu().double(), W, G, nfft)
    ref = AveragePower()(yo, t.cpu().double())
    gW, gG = torch.autograd.grad(ref, [W, G])
    check_close("average_power_shell/loss", loss.cpu().double().reshape(1), ref.detach().reshape(1), 1e-5)
    check_close("average_power_shell/g_W", mat.param.grad.cpu().double(), gW, 1e-5)
    check_close("average_power_shell/g_geq", geq.param.grad.cpu().double(), gG, 1e-4)
    params = [mat.param, geq.param]
    gs = GraphedStep(lambda xx: crit(model(xx), t), (x,), params, warmup=2)
    for _ in range(2):
        lg = gs.replay()
    torch.cuda.synchronize()
    assert abs(lg.item() - loss.item()) <= 1e-6 * abs(loss.item())
    check_close("average_power_shell/replay_g_W", mat.param.grad.cpu().double(), gW, 1e-5)
