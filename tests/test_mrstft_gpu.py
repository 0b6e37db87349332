"""ops.mrstft_loss / flamo_amd.optimize.MultiResoSTFT on the GPU (csrc/mrstft.hip).  The yardstick is always the float64
statement of the definition evaluated on the CPU (tests/test_mrstft_host.py::statement).

Limits.  float64: loss and gradient to 1e-10 -- the 1 / M of the log term amplifies rounding by up to ~5e3 on these signals
(the float32 torch statement's own gradient error against float64 is 2e-5 .. 3e-4), which in float64 is ~6e-13; 1e-10 leaves two
orders and is far below an indexing, window or adjoint mistake (1e-3 and above).  float32 loss: the streaming criteria's 2e-6
(tests/test_objectives.py).  float32 gradient: no constant -- the torch float32 statement is evaluated on the same inputs on
the CPU, and the kernels' l2 and max-norm errors against float64 must be at most twice its errors (radix-8 register passes round
differently from pocketfft; the conditioning is the same).  The kernels transform in double under either precision (DESIGN
4.6) and come out at 3e-8 .. 4e-8 where the float32 statement is at 2e-6 .. 1e-4."""
import pytest
import torch

from conftest import check_close, maxerr, relerr
from test_mrstft_host import DEFAULT, signals, statement, statement_grad

COTANGENT = 3.0
NODE = "_MRSTFTBackward"

# (shape, seed, silent samples at the prediction's start, class options, planar memory)
CASES = {
    "shortest": ((1, 1025, 1), 1, 0, {}, False),            # the shortest legal T: every 2048-frame reaches both reflected ends
    "rows": ((2, 4800, 3), 2, 0, {}, False),                # rows from batch and channel strides, channel-innermost
    "odd": ((1, 2603, 2), 3, 0, {}, False),                 # T divisible by no hop
    "silent": ((1, 4800, 1), 4, 700, {}, False),            # whole frames under the clamp
    "planar": ((2, 4800, 3), 2, 0, {}, True),               # the same values behind a transposed (B, N, T) view
    "full_window": ((2, 1400, 1), 5, 0, dict(fft_sizes=(512,), hop_sizes=(128,), win_lengths=(512,), w_sc=0.0, w_lin_mag=0.5), False),
    "smallest": ((1, 700, 2), 6, 0, dict(fft_sizes=(256,), hop_sizes=(64,), win_lengths=(100,)), False),
}
_ref = {}


def _crit(opts, device="cuda"):
    from flamo_amd.optimize import MultiResoSTFT
    crit = MultiResoSTFT(device=device, **opts)
    return crit, dict(resolutions=crit.resolutions(), weights=(crit.w_sc, crit.w_log_mag, crit.w_lin_mag), eps=crit.eps)


def _reference(name):
    """signals, the float64 statement's loss and gradient (cotangent 3) and the float32 statement's gradient errors against
    them, all on the CPU, computed once"""
    shape, seed, silent, opts, _ = CASES[name]
    key = (shape, seed, silent, tuple(sorted(opts.items())))          # ("planar" shares the values of "rows")
    if key not in _ref:
        yp, yt = signals(shape, seed, silent)
        kw = _crit(opts, "cpu")[1]
        loss, grad = statement_grad(yp, yt, COTANGENT, **kw)
        _, g32 = statement_grad(yp.float(), yt.float(), COTANGENT, **kw)
        _ref[key] = (yp, yt, loss, grad, relerr(g32.double(), grad), maxerr(g32.double(), grad))
    return _ref[key]


def _device(gpu, name, dtype, use_class=True):
    from flamo_amd import ops
    shape, seed, silent, opts, planar = CASES[name]
    yp, yt = _reference(name)[:2]
    crit, kw = _crit(opts)
    if planar:
        B, T, N = shape
        leaf = yp.transpose(1, 2).contiguous().to(device=gpu, dtype=dtype).requires_grad_(True)
        y, t = leaf.transpose(1, 2), yt.transpose(1, 2).contiguous().to(device=gpu, dtype=dtype).transpose(1, 2)
        assert tuple(y.shape) == shape and y.stride() == (N * T, 1, T) and t.stride() == (N * T, 1, T)
    else:
        leaf = y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
        t = yt.to(device=gpu, dtype=dtype)
    loss = crit(y, t) if use_class else ops.mrstft_loss(y, t, **kw)
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
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(CASES))
def test_shapes_against_the_float64_statement(gpu, name, dtype):
    got, g = _device(gpu, name, dtype)
    _check(f"mrstft_gpu/{name}_{str(dtype)[-2:]}", name, dtype, got, g)


def _zero_end(n_fft, hop, win, silent):
    """samples 0 .. zero_end - 1 lie under the windows of all-silent frames only: frame f's window holds the samples
    f hop - a .. f hop - a + win - 1, a = n_fft / 2 - (n_fft - win) / 2"""
    a = n_fft // 2 - (n_fft - win) // 2
    fs = (silent + a - win) // hop          # the last frame whose window ends within the silence
    return max(0, (fs + 1) * hop - a)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_silent_onset_gives_exact_zeros(gpu, dtype):
    """700 silent samples: 5-12 % of the prediction's bins are under the clamp and next to none of the target's; with one resolution
    alone, the samples that only all-silent frames hold get an exact zero, in the statement and on the kernels alike (under
    the three resolutions together the 2048-frames leave no such sample: 600 - 240 > 0)"""
    from flamo_amd import ops
    shape, seed, silent, _, _ = CASES["silent"]
    yp, yt = _reference("silent")[:2]
    assert [_zero_end(*r, silent) for r in DEFAULT] == [180, 0, 480]
    clamped = clamped_t = bins = 0
    for n_fft, hop, win in DEFAULT:
        w = torch.hann_window(win, dtype=torch.float64)
        P = [torch.stft(y[0, :, 0], n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True).abs().square()
             for y in (yp, yt)]
        clamped, clamped_t, bins = clamped + int((P[0] < 1e-8).sum()), clamped_t + int((P[1] < 1e-8).sum()), bins + P[0].numel()
        for p in P:      # nothing within 1e-3 of eps: the clamp cannot flip between the precisions
            assert not ((p > 0.999e-8) & (p < 1.001e-8)).any()
    # (the quiet tail leaves a handful of bins of either signal under eps as well: 3 of the target's 67487 here)
    assert 0.05 <= clamped / bins <= 0.12 and clamped_t <= 5
    for res in (DEFAULT[0], DEFAULT[2]):
        end = _zero_end(*res, silent)
        _, gref = statement_grad(yp, yt, resolutions=(res,))
        y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
        (g,) = torch.autograd.grad(ops.mrstft_loss(y, yt.to(device=gpu, dtype=dtype), (res,)), [y])
        g = g.cpu()
        assert torch.isfinite(g).all()
        assert torch.count_nonzero(gref[0, :end]) == 0 and torch.count_nonzero(g[0, :end]) == 0
        # (sample `end` itself sits under the first live frame's w[0] = 0)
        rest = shape[1] - end - 1
        assert torch.count_nonzero(gref[0, end + 1:]) == rest and torch.count_nonzero(g[0, end + 1:]) == rest


@pytest.mark.gpu
def test_two_runs_are_bit_identical(gpu):
    from flamo_amd import ops
    yp, yt = _reference("odd")[:2]
    for dtype in (torch.float32, torch.float64):
        runs = []
        for _ in range(2):
            y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
            loss = ops.mrstft_loss(y, yt.to(device=gpu, dtype=dtype), weights=(1.0, 1.0, 0.5))
            (g,) = torch.autograd.grad(loss, [y])
            runs.append((loss.detach().clone(), g.clone()))
        assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.gpu
def test_arguments_the_op_refuses_and_the_class_routes(gpu):
    from flamo_amd import ops
    from flamo_amd.optimize import MultiResoSTFT
    y = torch.randn(1, 1100, 2, device=gpu)
    with pytest.raises(ValueError, match="differ"):
        ops.mrstft_loss(y, torch.randn(1, 1101, 2, device=gpu))
    with pytest.raises(ValueError, match="differ"):
        ops.mrstft_loss(y, y.double())
    with pytest.raises(ValueError, match="float32 / float64"):
        ops.mrstft_loss(y.half(), y.half())
    with pytest.raises(ValueError, match="float32 / float64"):
        ops.mrstft_loss(y[0], y[0].clone())
    with pytest.raises(ValueError, match="no gradient"):
        ops.mrstft_loss(y, y.clone().requires_grad_(True))
    for res in (((768, 64, 300),), ((512, 64, 513),), ((2048, 64, 2048), (4096, 64, 300)), ((512, 0, 512),), ((512, 64),), ()):
        with pytest.raises(ValueError, match="resolutions"):
            ops.mrstft_loss(y, y.clone(), res)
    with pytest.raises(ValueError, match="resolutions"):
        ops.mrstft_loss(y[:, :1024], y[:, :1024].clone())          # T <= n_fft / 2 of the 2048-frames
    with pytest.raises(ValueError, match="weights"):
        ops.mrstft_loss(y, y.clone(), weights=(1.0, 1.0))
    loss = ops.mrstft_loss(y, y.clone() * 0.5)
    assert not loss.requires_grad and loss.grad_fn is None          # nothing to differentiate: nothing is kept
    # the class sends the same cases to its torch lines, which raise what torch.stft raises
    # (one frame length on the torch lines here: every further length is another FFT plan made by the runtime;
    # and float64 there, as in test_criterion_on_a_shell, which then finds this plan made)
    y = y.double()
    yg = y.clone().requires_grad_(True)
    t = (y * 0.5).requires_grad_(True)
    small = MultiResoSTFT(fft_sizes=(256,), hop_sizes=(64,), win_lengths=(256,), device="cuda")
    assert small._on_kernels(yg, t.detach()) and not small._on_kernels(yg, t)
    loss = small(yg, t)
    assert type(loss.grad_fn).__name__ != NODE
    loss.backward()
    assert t.grad is not None and yg.grad is not None
    assert type(small(yg, t.detach()).grad_fn).__name__ == NODE
    assert not MultiResoSTFT(fft_sizes=(768,), hop_sizes=(64,), win_lengths=(300,), device="cuda")._on_kernels(yg, y * 0.5)
    assert not small._on_kernels(yg, y.float()) and not small._on_kernels(yg.half(), y.half())
    with pytest.raises(RuntimeError):
        MultiResoSTFT(fft_sizes=(512,), hop_sizes=(64,), win_lengths=(513,), device="cuda")(yg, y * 0.5)
    with pytest.raises(RuntimeError):
        MultiResoSTFT(fft_sizes=(2048,), hop_sizes=(240,), win_lengths=(1200,), device="cuda")(yg[:, :1024], y[:, :1024] * 0.5)
    assert type(MultiResoSTFT(device="cuda")(yg, y * 0.5).grad_fn).__name__ == NODE


@pytest.mark.gpu
def test_criterion_on_a_shell(gpu):
    """parallelFilter(24 taps, 2 channels) -> Matrix(2, 2) at nfft 2048, one batch item, float64, two resolutions: loss and
    parameter gradients through the kernels against those through the class's torch lines on the same device"""
    from collections import OrderedDict
    from flamo_amd.optimize import MultiResoSTFT
    from flamo_amd.processor import dsp, system
    torch.manual_seed(21)
    nfft, N = 2048, 2
    dt = torch.float64
    kw = dict(nfft=nfft, alias_decay_db=0.0, device=gpu, dtype=dt)
    fir = dsp.parallelFilter(size=(24, N), requires_grad=True, **kw)
    mix = dsp.Matrix(size=(N, N), requires_grad=True, **kw)
    model = system.Shell(system.Series(OrderedDict(fir=fir, mix=mix)), dsp.FFT(nfft, dtype=dt), dsp.iFFT(nfft, dtype=dt))
    xs, ts = signals((1, nfft, N), 7)
    x, t = xs.to(gpu), ts.to(gpu)
    crit = MultiResoSTFT(fft_sizes=(1024, 256), hop_sizes=(120, 64), win_lengths=(600, 256), device="cuda")      # (two FFT plans)
    params = [fir.param, mix.param]
    loss = crit(model(x), t)
    assert type(loss.grad_fn).__name__ == NODE
    got = torch.autograd.grad(COTANGENT * loss, params)
    ref = crit._torch_forward(model(x), t)
    want = torch.autograd.grad(COTANGENT * ref, params)
    check_close("mrstft_gpu/shell/loss", loss.detach().cpu().reshape(1), ref.detach().cpu().reshape(1), 1e-10)
    check_close("mrstft_gpu/shell/g_fir", got[0].cpu(), want[0].cpu(), 1e-10)
    check_close("mrstft_gpu/shell/g_mix", got[1].cpu(), want[1].cpu(), 1e-10)


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_graph(gpu):
    """one forward + backward captured with torch.cuda.graph and replayed twice on new input values returns the eager run's
    bits: nothing is read back and no allocation depends on the data"""
    from flamo_amd import ops
    shape = (2, 2603, 2)
    inputs = [signals(shape, 30 + k) for k in range(3)]
    eager = []
    for yp, yt in inputs:
        y = yp.to(device=gpu, dtype=torch.float32).requires_grad_(True)
        loss = ops.mrstft_loss(y, yt.to(device=gpu, dtype=torch.float32), weights=(1.0, 1.0, 0.5))
        (g,) = torch.autograd.grad(COTANGENT * loss, [y])
        eager.append((loss.detach().clone(), g.clone()))
    ys = inputs[0][0].to(device=gpu, dtype=torch.float32).requires_grad_(True)
    ts = inputs[0][1].to(device=gpu, dtype=torch.float32)

    def step():
        loss = ops.mrstft_loss(ys, ts, weights=(1.0, 1.0, 0.5))
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
        assert torch.equal(loss_s, eager[k][0]) and torch.equal(g_s, eager[k][1])
