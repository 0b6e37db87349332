"""ops.mss_loss / flamo_amd.optimize.loss.mss_loss on the GPU (csrc/mss.hip).  The yardstick is always the float64 statement of
the definition evaluated on the CPU (tests/test_mss_host.py::statement), never the code under test.

Limits, the project's own (tests/test_mel_mss_gpu.py).  float64: loss and gradient to 1e-10.  float32 loss: the streaming
criteria's 2e-6.  float32 gradient: no constant -- the torch float32 statement is evaluated on the same inputs on the CPU, and
the kernels' l2 and max-norm errors against float64 must be at most twice its errors.  The signals keep every |SNR - threshold|
above 1e-6 dB and, for the 1-norm and the log terms, every |M_t - M_p| above 1e-12 of the largest M_t and every M above 0
(asserted on the CPU with the statement), so no mask entry and no sign flips between the precisions.

The achieved errors are quoted in DESIGN.md 4.6."""
import pytest
import torch

from conftest import check_close, maxerr, relerr
from test_mss_host import CASES as HOST_CASES, conditions, crit_kw, noise_energy_rule, spectrograms, statement, statement_grad
from test_mrstft_host import signals

COTANGENT = 3.0
NODE = "_MSSBackward"

# name -> (shape, seed, class options, planar memory)
CASES = {name: case + (False,) for name, case in HOST_CASES.items()}
CASES["planar"] = HOST_CASES["rows"] + (True,)                  # the same values behind a transposed (B, N, T) view
_ref = {}


def _reference(name):
    """signals, the float64 statement's loss and gradient (cotangent 3) and the float32 statement's gradient errors against
    them, all on the CPU, computed once; the conditions on the signals are asserted here"""
    shape, seed, opts, _ = CASES[name]
    key = (shape, seed, tuple(sorted((k, str(v)) for k, v in opts.items())))          # ("planar" shares the values of "rows")
    if key not in _ref:
        yp, yt = signals(shape, seed)
        kw = crit_kw(opts)[1]
        conditions(name, yp, yt, kw)
        loss, grad = statement_grad(yp, yt, COTANGENT, **kw)
        kw32 = dict(kw)
        if kw["apply_mask"] and kw["noise_energy"] is None:
            # (the float32 statement with the float64 statement's noise energy: one mask, two precisions of the arithmetic)
            n0 = kw["nfft"][0]
            kw32["noise_energy"] = noise_energy_rule(spectrograms(yt, n0, kw["overlap"], kw["sample_rate"]), kw["sample_rate"],
                                                     int(n0 * (1 - kw["overlap"]))).item()
        _, g32 = statement_grad(yp.float(), yt.float(), COTANGENT, **kw32)
        _ref[key] = (yp, yt, loss, grad, relerr(g32.double(), grad), maxerr(g32.double(), grad))
    return _ref[key]


def _device(gpu, name, dtype, use_class=True):
    from flamo_amd import ops
    shape, seed, opts, planar = CASES[name]
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
    if use_class:
        assert crit._on_kernels(y, t)
        loss = crit(y, t)
    else:
        yy, tt = y, t
        if kw.pop("energy_norm"):          # (the class's step before the op)
            yy, tt = y / torch.norm(y, p=2), t / torch.norm(t, p=2)
        loss = ops.mss_loss(yy, tt, **kw)
    assert loss.dim() == 0 and loss.dtype == dtype
    (g,) = torch.autograd.grad(COTANGENT * loss, [leaf])
    if planar:
        g = g.transpose(1, 2)
    assert tuple(g.shape) == shape and g.dtype == dtype
    return loss, g.cpu().double()


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


# (the op takes a number for the noise energy: the case that derives it runs through the class alone)
RUNS = [(name, "class" if name == "mask_derived" or n % 2 == 0 else "op") for n, name in enumerate(CASES)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name,via", RUNS, ids=[f"{n}-{v}" for n, v in RUNS])
def test_cases_against_the_float64_statement(gpu, name, via, dtype):
    loss, g = _device(gpu, name, dtype, use_class=via == "class")
    # energy_norm divides in torch before the op: the node of the loss is the op's either way
    assert type(loss.grad_fn).__name__ == NODE
    _check(f"mss_gpu/{name}_{str(dtype)[-2:]}_{via}", name, dtype, loss.detach().cpu().double(), g)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_both_layouts_give_the_same_result(gpu, dtype):
    """channel-innermost and planar memory of the same (2, 2603, 2) values: the same frames reach the same instructions"""
    (la, ga), (lb, gb) = _device(gpu, "rows", dtype, use_class=False), _device(gpu, "planar", dtype, use_class=False)
    assert torch.equal(la, lb) and torch.equal(ga, gb)


@pytest.mark.gpu
def test_derived_noise_energy_is_the_statement_s_and_is_kept(gpu):
    """through the class with noise_energy None: the number derived on the device from the first resolution of the first call
    is the rule's (frame -7 of the 128-point resolution), and it stays on the module"""
    shape, seed, opts, _ = CASES["mask_derived"]
    yp, yt = _reference("mask_derived")[:2]
    crit = crit_kw(opts, "cuda")[0]
    want = noise_energy_rule(spectrograms(yt, 128), 48000, 32).item()
    crit(yp.to(gpu), yt.to(gpu))
    assert isinstance(crit.noise_energy, float) and abs(crit.noise_energy - want) <= 1e-12 * want
    kept = crit.noise_energy
    crit(yt.to(gpu) * 0.5, yp.to(gpu))
    assert crit.noise_energy == kept


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("form", ["fro", 1, "magenta"])
def test_prediction_equal_to_the_target_gives_exact_zeros(gpu, form, dtype):
    """every difference is an exact 0: the loss is 0 and so is the gradient -- the norm's subgradient at 0 for "fro", sign(0) =
    0 for the 1-norms -- with the log term and the mask too"""
    from flamo_amd import ops
    yt = _reference("rows")[1].to(device=gpu, dtype=dtype)
    y = yt.clone().requires_grad_(True)
    base = dict(form="magenta") if form == "magenta" else dict(p=form)
    for kw in ({}, dict(log_term=True), dict(log_term=True, apply_mask=True, noise_energy=1.0)):
        loss = ops.mss_loss(y, yt, **base, **kw)
        (g,) = torch.autograd.grad(loss, [y])
        assert loss.item() == 0.0 and torch.count_nonzero(g) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_prediction_with_a_silent_start(gpu, dtype):
    """the first 700 samples of the prediction exactly zero, nfft = [128, 512]: M_p = 0 exactly on the frames inside.  Without
    the log term the result is finite and the statement's, and the gradient is exactly 0 on the samples that only such frames
    cover (t < 256: the 512-point frame 4 starts there); with it the statement is non-finite, and so are the kernels"""
    from flamo_amd import ops
    yp, yt = signals((1, 2603, 1), 1, silent=700)
    nfft = (128, 512)
    loss, grad = statement_grad(yp, yt, COTANGENT, nfft=nfft)
    assert torch.isfinite(loss) and torch.isfinite(grad).all() and torch.count_nonzero(grad[:, :256]) == 0
    y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
    t = yt.to(device=gpu, dtype=dtype)
    got = ops.mss_loss(y, t, nfft)
    (g,) = torch.autograd.grad(COTANGENT * got, [y])
    tag = f"mss_gpu/silent_{str(dtype)[-2:]}"
    check_close(tag + "/loss", got.detach().cpu().double().reshape(1), loss.reshape(1), 1e-10 if dtype == torch.float64 else 2e-6)
    if dtype == torch.float64:
        check_close(tag + "/grad", g.cpu(), grad, 1e-10)
    assert torch.isfinite(g).all() and torch.count_nonzero(g[:, :256]) == 0 and torch.count_nonzero(g[:, 700:]) > 0
    assert not torch.isfinite(statement(yp, yt, nfft=nfft, log_term=True))
    assert not torch.isfinite(ops.mss_loss(y, t, nfft, log_term=True))


@pytest.mark.gpu
def test_two_runs_are_bit_identical(gpu):
    from flamo_amd import ops
    for name in ("rows", "mask_one"):
        yp, yt = _reference(name)[:2]
        kw = crit_kw(CASES[name][2])[1]
        kw.pop("energy_norm")
        for dtype in (torch.float32, torch.float64):
            runs = []
            for _ in range(2):
                y = yp.to(device=gpu, dtype=dtype).requires_grad_(True)
                loss = ops.mss_loss(y, yt.to(device=gpu, dtype=dtype), **kw)
                (g,) = torch.autograd.grad(loss, [y])
                runs.append((loss.detach().clone(), g.clone()))
            assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.gpu
def test_arguments_the_op_refuses_and_the_class_routes(gpu):
    from flamo_amd import ops
    from flamo_amd.optimize.loss import mss_loss
    y = torch.randn(1, 2100, 2, device=gpu)
    few = [128, 256]
    with pytest.raises(ValueError, match="differ"):
        ops.mss_loss(y, torch.randn(1, 2101, 2, device=gpu), few)
    with pytest.raises(ValueError, match="differ"):
        ops.mss_loss(y, y.double(), few)
    with pytest.raises(ValueError, match="float32 / float64"):
        ops.mss_loss(y.half(), y.half(), few)
    with pytest.raises(ValueError, match="float32 / float64"):
        ops.mss_loss(y[0], y[0].clone(), few)
    with pytest.raises(ValueError, match="no gradient"):
        ops.mss_loss(y, y.clone().requires_grad_(True), few)
    for nfft in ([12], [128, 8192], [18], [], [128] * 9, [128.5]):
        with pytest.raises(ValueError, match="resolutions"):
            ops.mss_loss(y, y.clone(), nfft)
    assert ops.mss_loss(y, y.clone() * 0.5, [128, 4096]).isfinite()      # T = 2100 > 4096 / 2
    assert ops.mss_loss(y, y.clone() * 0.5, [16, 300]).isfinite()        # no power of two is asked for
    with pytest.raises(ValueError, match="resolutions"):
        ops.mss_loss(y[:, :2048], y[:, :2048].clone())                  # T <= n_fft / 2 at 4096
    with pytest.raises(ValueError, match="resolutions"):
        ops.mss_loss(y, y.clone(), few, overlap=0.999)                  # hop 0
    with pytest.raises(ValueError, match="p must be"):
        ops.mss_loss(y, y.clone(), few, p=3)
    with pytest.raises(ValueError, match="form must be"):
        ops.mss_loss(y, y.clone(), few, form="x")
    with pytest.raises(ValueError, match="sample_rate"):
        ops.mss_loss(y, y.clone(), few, sample_rate=79)
    for ne in (None, 0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="noise_energy"):
            ops.mss_loss(y, y.clone(), few, apply_mask=True, noise_energy=ne)
    loss = ops.mss_loss(y, y.clone() * 0.5, few)
    assert not loss.requires_grad and loss.grad_fn is None          # nothing to differentiate: nothing is kept
    # the class sends the same cases to its torch lines (float64 there, two short resolutions)
    y = y.double()
    yg = y.clone().requires_grad_(True)
    t = (y * 0.5).requires_grad_(True)
    small = mss_loss(nfft=few, device="cuda")
    assert small._on_kernels(yg, t.detach()) and not small._on_kernels(yg, t)
    loss = small(yg, t)
    assert type(loss.grad_fn).__name__ != NODE
    loss.backward()
    assert t.grad is not None and yg.grad is not None and torch.isfinite(t.grad).all() and torch.count_nonzero(t.grad) > 0
    assert type(small(yg, t.detach()).grad_fn).__name__ == NODE
    assert not small._on_kernels(yg, y.float()) and not small._on_kernels(yg.half(), y.half())
    assert not small._on_kernels(yg.cpu(), y.cpu())
    for other in (mss_loss(nfft=few, p=3, device="cuda"), mss_loss(nfft=[256, 8192], device="cuda"),
                  mss_loss(nfft=[18, 256], device="cuda")):
        long = other.nfft[-1] == 8192
        a, b = (torch.cat([yg, yg], 1), torch.cat([y, y], 1) * 0.5) if long else (yg, y * 0.5)
        assert not other._on_kernels(a, b) and type(other(a, b).grad_fn).__name__ != NODE
    assert not mss_loss(device="cuda")._on_kernels(yg[:, :2048], y[:, :2048])          # T <= n_fft / 2 at 4096
    assert type(mss_loss(device="cuda")(yg, y * 0.5).grad_fn).__name__ == NODE


@pytest.mark.gpu
def test_criterion_on_a_shell(gpu):
    """parallelFilter(24 taps, 2 channels) -> Matrix(2, 2) at nfft 4096, one batch item, float64, form "yamamoto": loss and
    parameter gradients through the kernels (all six resolutions) against those through the class's torch lines on the same
    device"""
    from collections import OrderedDict
    from flamo_amd.optimize.loss import mss_loss
    from flamo_amd.processor import dsp, system
    torch.manual_seed(21)
    nfft, N = 4096, 2
    dt = torch.float64
    kw = dict(nfft=nfft, alias_decay_db=0.0, device=gpu, dtype=dt)
    fir = dsp.parallelFilter(size=(24, N), requires_grad=True, **kw)
    mix = dsp.Matrix(size=(N, N), requires_grad=True, **kw)
    model = system.Shell(system.Series(OrderedDict(fir=fir, mix=mix)), dsp.FFT(nfft, dtype=dt), dsp.iFFT(nfft, dtype=dt))
    xs, ts = signals((1, nfft, N), 7)
    x, t = xs.to(gpu), ts.to(gpu)
    crit = mss_loss(form="yamamoto", device="cuda")
    params = [fir.param, mix.param]
    loss = crit(model(x), t)
    assert type(loss.grad_fn).__name__ == NODE
    got = torch.autograd.grad(COTANGENT * loss, params)
    ref = crit._torch_forward(model(x), t)
    want = torch.autograd.grad(COTANGENT * ref, params)
    check_close("mss_gpu/shell/loss", loss.detach().cpu().reshape(1), ref.detach().cpu().reshape(1), 1e-10)
    check_close("mss_gpu/shell/g_fir", got[0].cpu(), want[0].cpu(), 1e-10)
    check_close("mss_gpu/shell/g_mix", got[1].cpu(), want[1].cpu(), 1e-10)


@pytest.mark.gpu
def test_forward_and_backward_replay_from_a_graph(gpu):
    """one forward + backward captured with torch.cuda.graph and replayed twice on new input values returns the eager run's
    bits: nothing is read back and no allocation depends on the data (the noise energy is passed: deriving it reads back)"""
    from flamo_amd import ops
    shape = (2, 2603, 2)
    kw = dict(log_term=True, apply_mask=True, noise_energy=1.0)
    inputs = [signals(shape, 30 + k) for k in range(3)]
    eager = []
    for yp, yt in inputs:
        y = yp.to(device=gpu, dtype=torch.float32).requires_grad_(True)
        loss = ops.mss_loss(y, yt.to(device=gpu, dtype=torch.float32), **kw)
        (g,) = torch.autograd.grad(COTANGENT * loss, [y])
        eager.append((loss.detach().clone(), g.clone()))
    ys = inputs[0][0].to(device=gpu, dtype=torch.float32).requires_grad_(True)
    ts = inputs[0][1].to(device=gpu, dtype=torch.float32)

    def step():
        loss = ops.mss_loss(ys, ts, **kw)
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
