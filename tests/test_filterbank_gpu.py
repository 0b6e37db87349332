"""ops.filterbank / auxiliary.filterbank.FilterBank on the GPU (csrc/filterbank.hip between the library's real transforms)
against the float64 statement of test_filterbank_host.py: output and gradient under a cotangent of scale 3, the accuracy of the
responses the kernel evaluates for the low bands, layouts, determinism and the refusals.

Limits: float64 1e-10 (l2; the max-norm 1e-9), the project's float64 limit.  In float32 the l2 and the max-norm error may each
be at most twice that of the class's torch float32 lines on the same inputs, computed on the CPU here (the rule of
tests/test_mel_mss_gpu.py): the yardstick is what float32 transforms around exact responses lose."""
import numpy as np
import pytest
import torch

from conftest import check_close, maxerr, relerr
from test_filterbank_host import decaying_noise, make_bank, statement_bank, statement_responses

# (shape, fraction, order, centres handed to set_center_frequencies, input behind a transposed (B, N, T) view)
CASES = [
    ((2, 960, 3), 1, 5, None, False),                      # 11 bands
    ((2, 960, 3), 3, 2, None, False),                      # 30 bands
    ((1, 961, 2), 3, 8, None, False),                      # odd: T' = T - 1, the forward transform has no plan; 16 poles per band
    ((1, 4800, 1), 3, 5, None, False),
    ((1, 961, 2), 1, 5, [0, 1000, 24000], False),          # the low- and the high-pass branch
    ((2, 960, 3), 1, 8, None, True),
]
_refs = {}


def _case(i):
    """(bank, x, cotangent, statement output, statement gradient, float32 lines' output and gradient), computed once"""
    if i not in _refs:
        shape, fraction, order, centers, _ = CASES[i]
        bank = make_bank(fraction, order, centers)
        H = statement_responses(bank.get_center_frequencies(), order, 48000, shape[1] // 2 + 1)
        x = decaying_noise(shape, 10 + i, 1.0).float().double()
        xr = x.clone().requires_grad_(True)
        y = statement_bank(xr, H)
        C = 3.0 * torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(20 + i)).float().double()
        (g,) = torch.autograd.grad(y, [xr], C)
        x32 = x.float().requires_grad_(True)
        y32 = bank._torch_forward(x32)
        (g32,) = torch.autograd.grad(y32, [x32], C.float())
        _refs[i] = (bank, x, C, y.detach(), g, y32.detach().double(), g32.double())
    return _refs[i]


def _on_device(gpu, x, dtype, transposed):
    xd = x.to(device=gpu, dtype=dtype)
    if transposed:
        xd = xd.transpose(1, 2).contiguous().transpose(1, 2)
        assert not xd.is_contiguous() or xd.shape[2] == 1
    return xd.requires_grad_(True)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("i", range(len(CASES)))
def test_against_the_statement(gpu, i, dtype):
    """Achieved on an MI355X: float64 output <= 4.2e-15, gradient <= 4.4e-15; float32 1.8e-7 ... 2.3e-7 (l2) where the torch
    float32 lines stand at 1.7e-7 ... 2.0e-7: at most 1.3 of them in l2 and 1.4 in the max-norm."""
    from flamo_amd import ops
    shape, fraction, order, centers, transposed = CASES[i]
    bank, x, C, yref, gref, y32, g32 = _case(i)
    xd = _on_device(gpu, x, dtype, transposed)
    y = ops.filterbank(xd, bank)
    K = len(bank.get_center_frequencies())
    assert tuple(y.shape) == (shape[0], 2 * (shape[1] // 2), shape[2], K) and y.dtype == dtype
    assert type(y.grad_fn).__name__ == "_FilterBankBackward"
    (g,) = torch.autograd.grad(y, [xd], C.to(device=gpu, dtype=dtype))
    assert tuple(g.shape) == shape
    y, g = y.detach().cpu().double(), g.cpu().double()
    tag = f"filterbank_gpu/{i}_{str(dtype)[-2:]}"
    if dtype == torch.float64:
        check_close(tag + "/y", y, yref, 1e-10)
        check_close(tag + "/grad", g, gref, 1e-10)
        return
    for what, got, ref, lines in (("y", y, yref, y32), ("grad", g, gref, g32)):
        l2, mx, l2_lines, mx_lines = relerr(got, ref), maxerr(got, ref), relerr(lines, ref), maxerr(lines, ref)
        print(f"[parity] {tag}/{what}: l2 {l2:.3e} max {mx:.3e}; the torch float32 lines: l2 {l2_lines:.3e} max {mx_lines:.3e}")
        assert l2 <= 2 * l2_lines and mx <= 2 * mx_lines, (tag, what, l2, l2_lines, mx, mx_lines)


@pytest.mark.gpu
def test_the_class_routes_device_tensors_to_the_op(gpu):
    from flamo_amd import ops
    bank, x, _, yref, _, _, _ = _case(0)
    xd = x.to(gpu)
    y = bank(xd)
    assert type(bank(xd.requires_grad_(True)).grad_fn).__name__ == "_FilterBankBackward"
    assert torch.equal(y, ops.filterbank(xd.detach(), bank))
    check_close("filterbank_gpu/class", y.cpu(), yref, 1e-10)
    check_close("filterbank_gpu/torch_lines_on_device", bank._torch_forward(xd.detach()).cpu(), yref, 1e-10)
    # band signals are the columns edc_loss takes as they are: a view of planar memory, and so is its flatten(2)
    flat = y.flatten(2)
    assert flat.data_ptr() == y.data_ptr() and ops._edc_mem(flat)[1] == 1
    # a setter drops the constants on the device
    fresh = make_bank(1)
    fresh(xd.detach())
    held = fresh._device_consts[gpu.index][1]
    fresh(xd.detach())
    assert fresh._device_consts[gpu.index][1] is held          # placed once per (device, state)
    fresh.set_order(4)
    assert not fresh._device_consts
    H4 = statement_responses(fresh.get_center_frequencies(), 4, 48000, x.shape[1] // 2 + 1)
    check_close("filterbank_gpu/after_setter", fresh(xd.detach()).cpu(), statement_bank(x, H4), 1e-10)


@pytest.mark.gpu
def test_response_accuracy_of_the_low_bands(gpu):
    """a unit impulse through the float32 op at T = 4800, 30 bands: rfft(output) / rfft(impulse) against the statement's H, at
    most 2e-5 absolute in every band (4 times the 5e-6 of a float32 evaluation about z = 1; a float32 polynomial evaluation
    misses by three orders of magnitude).  The kernel evaluates in double: achieved 1e-7, float32 transforms' rounding."""
    from flamo_amd import ops
    T = 4800
    bank = make_bank(3, 5)
    H = statement_responses(bank.get_center_frequencies(), 5, 48000, T // 2 + 1)
    imp = torch.zeros(1, T, 1, device=gpu)
    imp[0, 0, 0] = 1
    y = ops.filterbank(imp, bank).cpu().double()
    got = torch.fft.rfft(y[0, :, 0, :], dim=0).transpose(0, 1).numpy()          # (K, M); the impulse's transform is 1
    err = np.abs(got - H).max(axis=1)
    print("[parity] filterbank_gpu/impulse: worst band errors", np.sort(err)[-3:], "bands", np.argsort(err)[-3:])
    assert np.abs(H).max(axis=1).min() > 0.99 and err.max() < 2e-5


@pytest.mark.gpu
def test_two_runs_are_bit_identical(gpu):
    from flamo_amd import ops
    bank, x, C, *_ = _case(1)
    for dtype in (torch.float32, torch.float64):
        runs = []
        for _ in range(2):
            xd = x.to(device=gpu, dtype=dtype).requires_grad_(True)
            y = ops.filterbank(xd, bank)
            (g,) = torch.autograd.grad(y, [xd], C.to(device=gpu, dtype=dtype))
            runs.append((y.detach().clone(), g.clone()))
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.gpu
def test_arguments_the_op_refuses(gpu):
    from flamo_amd import ops
    bank = make_bank(1)
    x = torch.randn(1, 480, 2, device=gpu)
    with pytest.raises(ValueError, match="ROCm device"):
        ops.filterbank(x.cpu(), bank)
    with pytest.raises(ValueError, match=r"\(B, T, N\)"):
        ops.filterbank(torch.complex(x, x), bank)
    with pytest.raises(ValueError, match=r"\(B, T, N\)"):
        ops.filterbank(x[0], bank)
    with pytest.raises(ValueError, match="up to 18"):
        ops.filterbank(x, make_bank(1, 9))
    wide = make_bank(1, 2, sample_rate=96000)
    wide.set_center_frequencies(np.geomspace(20.0, 20000.0, 35).tolist())
    with pytest.raises(ValueError, match="got 35 bands"):
        ops.filterbank(x, wide)
    assert not ops.filterbank_supported(wide) and ops.filterbank_supported(bank)
    # the class sends what the kernels do not take through its torch lines
    assert make_bank(1, 9)(x).shape == (1, 480, 2, 11)
    # all 34 nominal third-octave bands, order 8: the largest bank the kernels take
    full = make_bank(3, 8, fmin=10.0, fmax=40000.0, sample_rate=96000)
    assert len(full.get_center_frequencies()) == 34
    assert ops.filterbank(x, full).shape == (1, 480, 2, 34)
