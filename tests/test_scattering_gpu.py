"""ScatteringMatrix / VelvetNoiseMatrix on the GPU: the per-bin kernels (ops.scatter_response) and the FIR route against the
reference's recorded responses and gradients (tests/golden/scat_*.npz, velvet_*.npz).  The recorded rows (`bins`) pin the
response to the reference directly; the float64 restatement of the factored form (tests/test_scattering_host.py, which pins it
to the same rows at 1e-12) is the truth at every bin."""
import math
from collections import OrderedDict

import pytest
import torch

from conftest import cc, load_golden
from test_scattering_host import CASES, build, cotangent, factored_response, gamma_of, stage_matrices

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
LEARNABLE = [n for n in CASES if n.startswith("scat")]
# (forward vs the float64-envelope truth, gradient vs the golden): the oracle pin in float64, the parity bar in float32
TOL = {F64: (1e-10, 1e-9), F32: (1e-5, 1e-5)}
_truth = {}


def truth(name):
    """(meta, arrays, H at every bin, cotangent at every bin), float64 on the host, once per case"""
    if name not in _truth:
        meta, z = load_golden(name)
        H = factored_response(stage_matrices(meta, z["param"]), z["shifts"], z["m_L"], z["m_R"], meta["gain_per_sample"],
                              gamma_of(meta), meta["nfft"])
        _truth[name] = (meta, z, H, cotangent(meta))
    return _truth[name]


def cdtype(dtype):
    return torch.complex128 if dtype == F64 else torch.complex64


def response_and_grad(mod, C):
    mod.param.grad = None
    H = mod.freq_response(mod.param)
    if mod.param.requires_grad:
        H.backward(C.to(device=H.device, dtype=H.dtype))
    return H.detach(), (None if mod.param.grad is None else mod.param.grad.clone())


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_forward(gpu, name, dtype):
    from flamo_amd.processor import dsp
    meta, z, Ht, _ = truth(name)
    mod = build(dsp, meta, z, dtype, gpu)
    assert mod._per_bin_now(mod.param)
    with torch.no_grad():
        H = mod.freq_response(mod.param)
    assert H.shape == Ht.shape and H.dtype == cdtype(dtype)
    cc("rows_vs_H_f64env", H[z["bins"].to(gpu)], z["H_f64env"], TOL[dtype][0])
    cc("all_bins_vs_factored_f64", H, Ht, TOL[dtype][0])
    cc("rows_vs_H_ref", H[z["bins"].to(gpu)], z["H_ref"], 1e-5)


@pytest.mark.parametrize("dtype,tol", [(F64, 1e-12), (F32, 1e-5)], ids=["f64", "f32"])
def test_unitary_without_gain_and_envelope(gpu, dtype, tol):
    from flamo_amd.processor import dsp
    meta, z, _, _ = truth("scat_n2")
    assert meta["alias_decay_db"] == 0 and meta["gain_per_sample"] == 1
    mod = build(dsp, meta, z, dtype, gpu)
    with torch.no_grad():
        H = mod.freq_response(mod.param).to(torch.complex128)
    err = (H @ H.mH - torch.eye(meta["N"], dtype=torch.complex128, device=gpu)).abs().max().item()
    print(f"[scattering] |H H^H - I| = {err:.2e}")
    assert err < tol


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", LEARNABLE)
def test_gradient_and_determinism(gpu, name, dtype):
    from flamo_amd.processor import dsp
    meta, z, _, C = truth(name)
    mod = build(dsp, meta, z, dtype, gpu)
    _, g1 = response_and_grad(mod, C)
    _, g2 = response_and_grad(mod, C)
    cc("grad_param", g1, z["grad"], TOL[dtype][1])
    assert torch.equal(g1, g2)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_fir_route_agrees(gpu, name, dtype, monkeypatch):
    from flamo_amd.processor import dsp
    meta, z, Ht, C = truth(name)
    mod = build(dsp, meta, z, dtype, gpu)
    monkeypatch.setattr(dsp, "SCATTERING_PER_BIN", False)
    assert not mod._per_bin_now(mod.param)
    H, g = response_and_grad(mod, C)
    cc("fir_route_H", H, Ht, TOL[dtype][0])
    if g is not None:
        cc("fir_route_grad", g, z["grad"], TOL[dtype][1])


def test_more_taps_than_nfft_takes_the_fir_route(gpu):
    """L = 81 taps at nfft = 64: the reference's response is that of the FIR matrix cut at nfft taps"""
    from flamo_amd.auxiliary.scattering import ScatteringMapping
    from flamo_amd.processor import dsp
    nfft, db = 64, 30.0
    mL, mR = torch.tensor([5.0, 1, 7, 20], dtype=F64), torch.tensor([9.0, 3, 2, 15], dtype=F64)
    shifts = torch.tensor([[0.0, 3, 7, 9], [0, 12, 24, 36]], dtype=F64)
    torch.manual_seed(5)
    mod = dsp.ScatteringMatrix(size=(3, 4, 4), nfft=nfft, m_L=mL.to(gpu), m_R=mR.to(gpu), requires_grad=True, alias_decay_db=db,
                               device=gpu, dtype=F64)
    mod.map_filter.shifts = shifts.to(gpu)
    assert mod.map_filter.fir_length() == 81 and not mod._per_bin_now(mod.param)
    H = mod.freq_response(mod.param).detach()
    host = ScatteringMapping(4, n_stages=2, gain_per_sample=0.9999, m_L=mL, m_R=mR, dtype=F64)
    host.shifts = shifts
    up = torch.triu(mod.param.detach().cpu(), diagonal=1)
    fir = host(torch.linalg.matrix_exp(up - up.mT))[:nfft]
    env = torch.tensor(10.0 ** (-db / nfft / 20.0), dtype=F64) ** torch.arange(nfft, dtype=F64)
    cc("truncated_fir", H, torch.fft.rfft(fir * env.view(-1, 1, 1), n=nfft, dim=0), 1e-10)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_bin_shard(gpu, dtype):
    from flamo_amd import ops
    from flamo_amd.processor import dsp
    meta, z, _, C = truth("scat_n4")
    mod = build(dsp, meta, z, dtype, gpu)
    lo, n = 100, 77
    with torch.no_grad():
        full = mod.freq_response(mod.param)
    # the gradient of the shard's own bins, in float64 on the host
    p = z["param"].clone().requires_grad_(True)
    Hs = factored_response(stage_matrices(meta, p), z["shifts"], z["m_L"], z["m_R"], meta["gain_per_sample"], gamma_of(meta),
                           meta["nfft"], torch.arange(lo, lo + n))
    (want,) = torch.autograd.grad(torch.sum(torch.real(Hs * C[lo:lo + n].conj())), [p])
    try:
        ops.set_bin_shard(lo, n)
        part, g = response_and_grad(mod, C[lo:lo + n])
    finally:
        ops.set_bin_shard(0, None)
    assert part.shape == (n, meta["N"], meta["N"])
    assert torch.equal(part, full[lo:lo + n])
    cc("shard_grad", g, want, TOL[dtype][1])


def test_end_to_end_fdn(gpu):
    """Shell(FFT, Gain(4,1) -> Recursion(parallelDelay, ScatteringMatrix(4,4,4)) -> Gain(1,4), |.|), float64, dB = 30: output and
    every gradient against the golden's float64 evaluation; sparsity_loss on the model is the mean over the 4 stages"""
    from flamo_amd import optimize
    from flamo_amd.processor import dsp, system
    meta, z, _, _ = truth("scat_n4")
    nfft = meta["nfft"]
    kw = dict(nfft=nfft, alias_decay_db=meta["alias_decay_db"], device=gpu, dtype=F64)
    ig, og = dsp.Gain(size=(4, 1), requires_grad=True, **kw), dsp.Gain(size=(1, 4), requires_grad=True, **kw)
    ig.assign_value(z["fdn_b"].to(gpu))
    og.assign_value(z["fdn_c"].to(gpu))
    dl = dsp.parallelDelay(size=(4,), max_len=200, isint=True, **kw)
    dl.assign_value(dl.sample2s(z["fdn_delays"].to(gpu)))
    sc = build(dsp, meta, z, F64, gpu)
    core = system.Series(OrderedDict(input_gain=ig, feedback_loop=system.Recursion(fF=dl, fB=sc), output_gain=og))
    model = system.Shell(core, dsp.FFT(nfft, dtype=F64), dsp.Transform(lambda x: torch.abs(x), dtype=F64))
    x = torch.zeros(1, nfft, 1, device=gpu, dtype=F64)
    x[:, 0] = 1
    out = model(x)
    assert out.shape == (1, nfft // 2 + 1, 1)
    (out.reshape(-1) * z["fdn_w"].to(gpu)).sum().backward()
    cc("fdn_out", out.detach().reshape(-1), z["fdn_out"], 1e-8)
    cc("fdn_grad_b", ig.param.grad, z["fdn_grad_b"], 1e-8)
    cc("fdn_grad_c", og.param.grad, z["fdn_grad_c"], 1e-8)
    cc("fdn_grad_param", sc.param.grad, z["fdn_grad_param"], 1e-8)
    U = stage_matrices(meta, z["param"])
    want = torch.mean((U.abs().sum(dim=(-2, -1)) - 4 * 2.0) / (4 * (1 - 2.0)))
    got = optimize.sparsity_loss()(None, None, model)
    assert abs(got.item() - want.item()) < 1e-12


@pytest.mark.parametrize("name", ["scat_n4", "velvet_n4"])
def test_probe(gpu, name):
    from flamo_amd.processor import dsp
    meta, z, Ht, _ = truth(name)
    mod = build(dsp, meta, z, F64, gpu)
    with torch.no_grad():
        H = mod.freq_response(mod.param)
        for b in (0, 1, 77, meta["nfft"] // 2):
            zz = torch.exp(torch.tensor(2j * math.pi * b / meta["nfft"], dtype=torch.complex128, device=gpu))
            P = mod.probe(zz)
            assert (P - H[b]).abs().max().item() < 1e-11 and (P.cpu() - Ht[b]).abs().max().item() < 1e-11


def test_row_major_bin_order_and_long_spectrum(gpu):
    """inside ops.row_major_bins the response comes out in natural order and DSP._response_in_order permutes it; nfft = 96000:
    188 forward workgroups per column, the last one partial"""
    from flamo_amd import ops
    from flamo_amd.processor import dsp
    nfft, N = 96000, 4
    torch.manual_seed(3)
    mL, mR = torch.tensor([3.0, 1, 7, 2]), torch.tensor([5.0, 11, 2, 9])
    mod = dsp.ScatteringMatrix(size=(3, N, N), nfft=nfft, m_L=mL, m_R=mR, alias_decay_db=30.0, device=gpu, dtype=F32)
    assert mod._per_bin_now(mod.param)
    with torch.no_grad():
        H = mod._response_in_order(mod.param)
        with ops.row_major_bins(nfft):
            Hrm = mod._response_in_order(mod.param)
        assert torch.equal(Hrm, ops.permute_bins(H, nfft))
    bins = torch.tensor([0, 1, 255, 256, 24000, 47871, 47872, 47999, 48000])
    up = torch.triu(mod.param.detach().cpu().to(F64), diagonal=1)
    want = factored_response(torch.linalg.matrix_exp(up - up.mT), mod.map_filter.shifts.cpu(), mL, mR, 0.9999,
                             10.0 ** (-30.0 / nfft / 20.0), nfft, bins)
    cc("long_spectrum_rows", H[bins.to(gpu)], want, 1e-5)
