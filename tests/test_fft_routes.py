"""Every kernel route of the layered FFT (csrc/fft.hip: make_plan + launch_fft behind ops.rfft / ops.irfft) against
torch.fft in float64 on the CPU.

launch_fft picks its kernels from (nfft, precision, number of signals, input length, layout).  Each test below names the
route it is written for; test_plans_the_gpu_tests_rely_on (host only) pins the (L1, L2) plans, so that a change of the
planner cannot move the GPU tests off those routes without this file noticing.

Reference: torch.fft.rfft / irfft in float64 on the CPU; for float32 runs the inputs are drawn in float32 and widened.
The rising anti-alias envelope is 10^(|dB| t / (20 nfft)) (dsp.py:158-162, 201-205), as in tests/test_spectral.py::_ref.
Limits (conftest.cc: relative l2 error below the limit, max-norm error below ten times it): float64 1e-10, float32 1e-5,
the project's own (tests/test_hip_parity.py)."""
import ctypes

import pytest
import torch

from conftest import cc

TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
CD = {torch.float64: torch.complex128, torch.float32: torch.complex64}
DTYPES = [torch.float64, torch.float32]
DB = 30.0
FL_ERR_UNSUPPORTED = -2

# nfft -> (L1, L2): both sub-lengths on the two-register-stage kernels (kFastSplits), in both precisions.  Together the ten
# lengths launch every split 200 / 240 / 300 / 320 / 400 / 480 as a column pass (L1) AND as a row pass (L2).
FAST_PLANS = {80000: (200, 200), 96000: (200, 240), 115200: (240, 240), 180000: (300, 300), 192000: (300, 320),
              204800: (320, 320), 256000: (320, 400), 320000: (400, 400), 384000: (400, 480), 460800: (480, 480)}
# "long columns, short rows" (L1 > L2, generic Stockham kernels with one or two columns per tile)
LONG_F64 = (156250, (625, 125))      # 2 5^7
LONG_F32 = (322102, (1331, 121))     # 2 11^5


def _plan(nfft, f64):
    from flamo_amd import _lib
    l1, l2 = ctypes.c_int(0), ctypes.c_int(0)
    rc = _lib.lib().fl_fft_plan(nfft, int(f64), ctypes.byref(l1), ctypes.byref(l2))
    return rc, (l1.value, l2.value)


# ----------------------------------------------------------------------------- 1. host: the plans
def test_plans_the_gpu_tests_rely_on():
    """fl_fft_plan for the lengths of this file (no GPU): the fast lengths plan the same in both precisions."""
    for nfft, want in FAST_PLANS.items():
        for f64 in (False, True):
            assert _plan(nfft, f64) == (0, want), (nfft, f64)
    assert _plan(LONG_F64[0], True) == (0, LONG_F64[1])
    assert _plan(LONG_F32[0], False) == (0, LONG_F32[1])
    assert _plan(LONG_F32[0], True)[0] == FL_ERR_UNSUPPORTED         # rows of 1331 exceed twice the float64 row limit
    # few-signal mode (launch_fft): cdiv(L2, 16) * nsig < 64 -- one signal is inside it at every split, six are outside
    for _, l2 in FAST_PLANS.values():
        assert -(-l2 // 16) * 1 < 64 <= -(-l2 // 16) * 6
    assert -(-240 // 16) * 4 < 64 <= -(-240 // 16) * 5                # the boundary case of test_few_signal_boundary


# ----------------------------------------------------------------------------- reference and comparison
def _envelope(nfft, db, ndim):
    t = torch.arange(nfft, dtype=torch.float64)
    return (10.0 ** (abs(db) / (20.0 * nfft) * t)).view((1, -1) + (1,) * (ndim - 2))


def _draw(seed, dt, shape, nfft):
    """CPU inputs in precision dt: x of `shape` (B, T, rest...), cotangent C of its spectrum, half spectrum Z (non-zero
    imaginary parts at DC and Nyquist: C2R ignores them) and cotangent c of its inverse transform."""
    g = torch.Generator().manual_seed(seed)
    B, rest, M = shape[0], tuple(shape[2:]), nfft // 2 + 1
    x = torch.randn(shape, dtype=dt, generator=g)
    C = torch.randn((B, M, *rest), dtype=CD[dt], generator=g)
    Z = torch.randn((B, M, *rest), dtype=CD[dt], generator=g)
    c = torch.randn((B, nfft, *rest), dtype=dt, generator=g)
    assert Z[:, 0].imag.abs().min() > 0 and Z[:, -1].imag.abs().min() > 0
    return x, C, Z, c


def _ref_forward(x, C, nfft, norm, db):
    """float64: X = rfft(x[:nfft] e, nfft) and d/dx sum Re(X conj C)"""
    xr = x.double().requires_grad_(True)
    xx = xr[:, :nfft]
    if db:
        xx = xx * _envelope(nfft, db, x.dim())[:, : xx.shape[1]]
    X = torch.fft.rfft(xx, n=nfft, dim=1, norm=norm)
    if C is None:
        return X.detach(), None
    (g,) = torch.autograd.grad(torch.sum(torch.real(X * torch.conj(C.to(torch.complex128)))), [xr])
    return X.detach(), g


def _ref_inverse(Z, c, nfft, norm, db):
    """float64: y = irfft(Z, nfft) e and d/dZ sum(y c)"""
    Zr = Z.to(torch.complex128).requires_grad_(True)
    y = torch.fft.irfft(Zr, n=nfft, dim=1, norm=norm)
    if db:
        y = y * _envelope(nfft, db, y.dim())
    (g,) = torch.autograd.grad(torch.sum(y * c.double()), [Zr])
    return y.detach(), g


def _check_forward(xg, x, C, nfft, dt, tag="", norm="backward", db=DB, grad=True):
    """ops.rfft of the device tensor xg (the values of the CPU tensor x, in whatever layout) and its gradient"""
    from flamo_amd import ops
    Xr, gr = _ref_forward(x, C if grad else None, nfft, norm, db)
    if grad:
        xg = xg.requires_grad_(True)
    X = ops.rfft(xg, nfft, norm, db)
    assert X.shape == Xr.shape and X.dtype == CD[dt]
    cc(tag + "X", X.detach().cpu(), Xr, TOL[dt])
    if not grad:
        return None
    (g,) = torch.autograd.grad(torch.sum(torch.real(X * torch.conj(C.to(xg.device)))), [xg])
    assert g.shape == x.shape and g.dtype == dt
    cc(tag + "gx", g.cpu(), gr, TOL[dt])
    return g


def _check_inverse(Z, c, nfft, dt, dev, tag="", norm="ortho", db=DB, grad=True):
    from flamo_amd import ops
    yr, gr = _ref_inverse(Z, c, nfft, norm, db)
    Zg = Z.to(dev).requires_grad_(grad)
    y = ops.irfft(Zg, nfft, norm, db)
    assert y.shape == yr.shape and y.dtype == dt
    cc(tag + "y", y.detach().cpu(), yr, TOL[dt])
    if grad:
        (g,) = torch.autograd.grad(torch.sum(y * c.to(dev)), [Zg])
        assert g.shape == Z.shape
        cc(tag + "gZ", g.cpu(), gr, TOL[dt])


def _check_both(dev, dt, nfft, shape, seed):
    x, C, Z, c = _draw(seed, dt, shape, nfft)
    _check_forward(x.to(dev), x, C, nfft, dt)
    _check_inverse(Z, c, nfft, dt, dev)


def _shape(nsig, T):
    return {1: (1, T, 1), 3: (1, T, 3), 4: (1, T, 4), 5: (5, T, 1), 6: (2, T, 3)}[nsig]


# ----------------------------------------------------------------------------- 2. fast splits x few-signal mode
@pytest.mark.gpu
@pytest.mark.parametrize("nsig", [1, 6], ids=["few", "regular"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nfft", sorted(FAST_PLANS))
def test_fast_split_matrix(gpu, nfft, dt, nsig):
    """fft_cols_fast / fft_cols_ipair / fft_rows_fast at every split, as columns and as rows, forward and inverse with both
    gradients.  One signal: few-signal mode (four columns per workgroup, the paired inverse with CD = 4 in float32, row tiles
    of two rows with a partial last tile wherever the row count is odd: 101 rows at L1 = 200).  Six: the regular tiles."""
    _check_both(gpu, dt, nfft, _shape(nsig, nfft), seed=nfft + nsig)


@pytest.mark.gpu
@pytest.mark.parametrize("nsig", [4, 5])
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
def test_few_signal_boundary(gpu, dt, nsig):
    """L2 = 240: cdiv(240, 16) nsig < 64 holds for four signals (few-signal tiles) and fails for five (regular tiles)"""
    _check_both(gpu, dt, 115200, _shape(nsig, 115200), seed=nsig)


# ----------------------------------------------------------------------------- 3. ragged lengths on the fast kernels
@pytest.mark.gpu
@pytest.mark.parametrize("nsig", [1, 6], ids=["few", "regular"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nfft", [96000, 460800])
def test_fast_ragged_input_lengths(gpu, nfft, dt, nsig):
    """T < nfft: the guarded loader (LOAD_PACK) of fft_cols_fast zero-pads, also at odd T and T = 1, and the gradient is the
    cropped store of fft_rows_fast<EPI_IRFFT_STORE> (odd T: odd signal stride, no paired stores on every other signal).
    T > nfft: the input is cut, the gradient beyond sample nfft is exactly zero."""
    for T in (1, 7, nfft // 2 + 1, nfft - 1, nfft + 3):
        x, C, _, _ = _draw(nfft + T, dt, _shape(nsig, T), nfft)
        g = _check_forward(x.to(gpu), x, C, nfft, dt, tag=f"T{T}_")
        if T > nfft:
            assert torch.count_nonzero(g[:, nfft:]).item() == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nfft", [96000, 460800])
def test_fast_planar_odd_stride(gpu, nfft, dt):
    """A planar input whose signals are an odd number of elements apart: pair loads would be misaligned on every other signal,
    so the host must choose the guarded loader at full length"""
    from flamo_amd import ops
    B, N = 2, 3
    x, C, _, _ = _draw(nfft + 1, dt, (B, nfft, N), nfft)
    buf = torch.zeros(B, N, nfft + 1, dtype=dt, device=gpu)
    buf[..., :nfft] = x.to(gpu).movedim(1, -1)
    xg = buf[..., :nfft].movedim(-1, 1).detach()
    assert ops._is_planar(xg) and ops._lead_pitch(xg.movedim(1, -1)) == nfft + 1
    _check_forward(xg, x, C, nfft, dt)


# ----------------------------------------------------------------------------- 4. long columns, short rows
@pytest.mark.gpu
@pytest.mark.parametrize("nsig", [1, 3])
@pytest.mark.parametrize("nfft,dt", [(LONG_F64[0], torch.float64), (LONG_F32[0], torch.float32)], ids=["156250-f64", "322102-f32"])
def test_long_column_plans(gpu, nfft, dt, nsig):
    """L1 > L2 (625 x 125, 1331 x 121): fft_cols with two columns per tile and a partial last tile, radix 5 / 11 stages"""
    _check_both(gpu, dt, nfft, _shape(nsig, nfft), seed=nfft + nsig)


# ----------------------------------------------------------------------------- 5. radices 7, 11, 13
@pytest.mark.gpu
@pytest.mark.parametrize("max_single", [0, 8], ids=["plan-default", "plan-two-pass"])
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nfft", [2 * 7 * 7 * 4, 2 * 11 * 11 * 4, 2 * 13 * 13 * 4, 2 * 7 * 11 * 13])
def test_radix_7_11_13(gpu, nfft, dt, max_single):
    """Radix 7 / 11 / 13 stages single-pass (default plan) and in both passes of the forced two-pass plan (14 x 14, 22 x 22,
    26 x 26, 13 x 77), with a ragged input T = nfft - 3"""
    from flamo_amd import _lib
    L = _lib.lib()
    assert L.fl_debug_set_fft_max_single(max_single) == 0
    try:
        rc, (l1, l2) = _plan(nfft, dt == torch.float64)
        assert rc == 0 and 2 * l1 * l2 == nfft and (l1 == 1) == (max_single == 0)
        _check_both(gpu, dt, nfft, (2, nfft - 3, 3), seed=nfft)
    finally:
        L.fl_debug_set_fft_max_single(0)


# ----------------------------------------------------------------------------- 6. channel-innermost source
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nfft", [96000, 256000])
def test_channel_innermost_fast(gpu, nfft, dt):
    """fl_rfft_ci_* at fast lengths: the layout conversion fused into the guarded loader of fft_cols_fast, blocks of a batch
    item grouped per XCD; full length and T < nfft"""
    from flamo_amd import ops
    assert ops.CI_MAX_CHANNELS == 0
    ops.CI_MAX_CHANNELS = 16
    try:
        for shape in ((2, nfft, 2), (1, nfft, 3, 2), (2, nfft - 5, 8)):
            x, _, _, _ = _draw(nfft + shape[-1], dt, shape, nfft)
            xg = x.to(gpu)
            assert xg.is_contiguous() and not ops._is_planar(xg)         # the condition of _rfft_any for the fused read
            _check_forward(xg, x, None, nfft, dt, tag="x".join(map(str, shape)) + "_", grad=False)
    finally:
        ops.CI_MAX_CHANNELS = 0


# ----------------------------------------------------------------------------- 7. tuning hooks
@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTYPES, ids=["f64", "f32"])
@pytest.mark.parametrize("nfft", [96000, 460800])
def test_fast_tuning_hooks(gpu, nfft, dt):
    """fl_debug_set_fft_fast(code + 1000 rows): 16 / 32 force the column tile of pass 1 (32: float32 only; both switch the
    paired inverse and the few-signal mode off), rows > 0 caps the rows per workgroup of pass 2"""
    from flamo_amd import _lib, ops
    L = _lib.lib()
    x, _, Z, c = _draw(nfft, dt, (2, nfft, 3), nfft)
    Xr, _ = _ref_forward(x, None, nfft, "backward", DB)
    yr, _ = _ref_inverse(Z, c, nfft, "ortho", DB)
    xg, Zg = x.to(gpu), Z.to(gpu)
    try:
        for code in (16, 32, 1 + 1000 * 1, 1 + 1000 * 3):
            assert L.fl_debug_set_fft_fast(code) == 0
            cc(f"hook{code}_X", ops.rfft(xg, nfft, "backward", DB).cpu(), Xr, TOL[dt])
            cc(f"hook{code}_y", ops.irfft(Zg, nfft, "ortho", DB).cpu(), yr, TOL[dt])
    finally:
        L.fl_debug_set_fft_fast(1)
