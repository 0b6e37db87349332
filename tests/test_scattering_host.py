"""ScatteringMatrix / VelvetNoiseMatrix, host side (no GPU): constructor contract, the delays drawn under a seed, the factored
form and the time-domain mapping against the reference's recorded responses (tests/golden/scat_*.npz, velvet_*.npz, written
by tools/gen_golden_scattering.py), and masked_mse_loss."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

F64 = torch.float64
CASES = ["scat_n2", "scat_n4", "scat_n6", "scat_n16", "velvet_n4"]


# ----------------------------------------------------------------------------- shared with tests/test_scattering_gpu.py
def gamma_of(meta):
    return 10.0 ** (-abs(meta["alias_decay_db"]) / meta["nfft"] / 20.0)


def cotangent(meta):
    """the cotangent of the fixtures at every bin (the golden's C holds its rows at `bins`): numpy's legacy stream"""
    M, N = meta["nfft"] // 2 + 1, meta["N"]
    ab = np.random.RandomState(meta["seed"]).standard_normal((2, M, N, N))
    return torch.from_numpy(ab[0] + 1j * ab[1])


def stage_matrices(meta, param):
    """U = map(param) in float64: exp of the skew part per stage (ScatteringMatrix), the parameter itself (Velvet)"""
    if meta["module"] == "VelvetNoiseMatrix":
        return param.to(F64)
    up = torch.triu(param.to(F64), diagonal=1)
    return torch.linalg.matrix_exp(up - up.mT)


def factored_response(U, shifts, m_L, m_R, g, gamma, nfft, bins=None):
    """H[f] = D(m_L) U_K G_K D(m_K) ... U_1 G_1 D(m_1) U_0 D(m_R) in float64 with integer phases:
    D(m) = diag(gamma^m exp(-2 pi i ((f m) mod nfft) / nfft)), G_s = diag(g^m_s)."""
    k = torch.arange(nfft // 2 + 1, dtype=torch.int64) if bins is None else torch.as_tensor(bins, dtype=torch.int64)

    def D(m, base):
        m = m.to(torch.int64)
        ang = -2 * math.pi * ((k[:, None] * m[None, :]) % nfft).to(F64) / nfft
        return torch.polar((base ** m.to(F64))[None, :].expand(len(k), -1).contiguous(), ang)

    H = U[0].to(torch.complex128)[None] * D(m_R, gamma)[:, None, :]
    for s in range(1, U.shape[0]):
        H = U[s].to(torch.complex128)[None] @ (D(shifts[s - 1], gamma * g)[:, :, None] * H)
    return D(m_L, gamma)[:, :, None] * H


def build(dsp, meta, z, dtype=F64, device=None, **over):
    """the drop-in module of a golden case, with the golden's parameter and delays"""
    N, st = meta["N"], meta["stages"]
    kw = dict(size=(st, N, N), nfft=meta["nfft"], gain_per_sample=meta["gain_per_sample"], m_L=z["m_L"].to(dtype), m_R=z["m_R"].to(dtype),
              alias_decay_db=meta["alias_decay_db"], device=device, dtype=dtype)
    if meta["module"] == "ScatteringMatrix":
        kw.update(sparsity=meta["sparsity"], pulse_size=meta["pulse_size"], requires_grad=True)
    else:
        kw.update(density=meta["density"])
    kw.update(over)
    torch.manual_seed(meta["seed"])
    mod = getattr(dsp, meta["module"])(**kw)
    mod.assign_value(z["param"].to(device=device, dtype=dtype))
    mod.map_filter.shifts = z["shifts"].to(device=device, dtype=dtype)
    return mod


# ----------------------------------------------------------------------------- tests
def test_constructor_contract():
    from flamo_amd.processor import dsp
    from flamo_amd.auxiliary.scattering import ScatteringMapping
    mL, mR = torch.tensor([1.0, 2, 3, 4]), torch.tensor([4.0, 3, 2, 1])
    m = dsp.ScatteringMatrix(size=(3, 4, 4), nfft=512, sparsity=2, gain_per_sample=0.999, pulse_size=2, m_L=mL, m_R=mR,
                             requires_grad=True, alias_decay_db=30.0)
    assert (m.sparsity, m.gain_per_sample, m.pulse_size, m.nfft, m.size) == (2, 0.999, 2, 512, (3, 4, 4))
    assert (m.input_channels, m.output_channels) == (4, 4)
    assert m.param.shape == (3, 4, 4) and m.param.requires_grad
    assert list(m.state_dict()) == ["param"]
    assert isinstance(m.map_filter, ScatteringMapping)
    mf = m.map_filter
    assert mf.shifts.shape == (2, 4) and mf.n_stages == 2 and mf.gain_per_sample == 0.999
    assert mf.sparsity_vect.tolist() == [2.0, 1.0] and torch.equal(mf.m_L, mL) and torch.equal(mf.m_R, mR)
    U = m.map(m.param.detach())
    assert torch.allclose(U @ U.mT, torch.eye(4).expand(3, 4, 4), atol=1e-5)
    assert m._fusable() and m._own_convolve is m.freq_convolve and dsp.SCATTERING_PER_BIN is True
    # no outer delays given: zeros
    m0 = dsp.ScatteringMatrix(size=(2, 2, 2), nfft=64)
    assert m0.map_filter.m_L.tolist() == [0.0, 0.0] and m0.map_filter.m_R.tolist() == [0.0, 0.0] and not m0.param.requires_grad

    v = dsp.VelvetNoiseMatrix(size=(3, 4, 4), nfft=512, density=0.2, m_L=mL, m_R=mR)
    assert (v.input_channels, v.output_channels) == (4, 4) and list(v.state_dict()) == ["param"]
    assert not v.param.requires_grad and v.pulse_size == 1 and v.sparsity == 1 / 0.2
    assert v.map_filter.sparsity == 5 and v.map_filter.sparsity_vect.tolist() == [5.0, 1.0]
    h = torch.tensor([[1.0, 1, 1, 1], [1, -1, 1, -1], [1, 1, -1, -1], [1, -1, -1, 1]]) / 2
    assert torch.allclose(v.param.detach(), h.expand(3, 4, 4), atol=1e-7)
    assert v.new_value == 1


def test_assertions_fire():
    from flamo_amd.processor import dsp
    with pytest.raises(AssertionError, match="Matrix must be square"):
        dsp.ScatteringMatrix(size=(3, 4, 3))
    with pytest.raises(AssertionError, match="Matrix must be square"):
        dsp.VelvetNoiseMatrix(size=(3, 4, 2))
    with pytest.raises(AssertionError, match="powers of 2"):
        dsp.VelvetNoiseMatrix(size=(3, 6, 6), m_L=torch.zeros(6), m_R=torch.zeros(6))


def test_hadamard_matrix():
    from flamo_amd.auxiliary.scattering import hadamard_matrix
    for N in (1, 2, 8, 16):
        H = hadamard_matrix(N)
        assert H.shape == (N, N) and torch.allclose(H @ H.T, torch.eye(N, dtype=F64), atol=1e-14)
        assert torch.allclose(H.abs(), torch.full((N, N), N ** -0.5, dtype=F64), atol=1e-15)


@pytest.mark.parametrize("name", CASES)
def test_shifts_under_the_stored_seed(name):
    """param first, then one torch.rand(N) per stage: the constructor draws what the reference drew"""
    from flamo_amd.processor import dsp
    meta, z = load_golden(name)
    N, st = meta["N"], meta["stages"]
    kw = dict(size=(st, N, N), nfft=meta["nfft"], m_L=z["m_L"], m_R=z["m_R"], dtype=F64)
    if meta["module"] == "ScatteringMatrix":
        kw.update(sparsity=meta["sparsity"], pulse_size=meta["pulse_size"])
    else:
        kw.update(density=meta["density"])
    torch.manual_seed(meta["seed"])
    mod = getattr(dsp, meta["module"])(**kw)
    assert torch.equal(mod.map_filter.shifts, z["shifts"])
    assert (z["shifts"] == 0).any() and (z["m_L"] > 0).all() and (z["m_R"] > 0).all()
    if meta["module"] == "ScatteringMatrix":
        assert torch.equal(mod.param.detach(), z["param"])


@pytest.mark.parametrize("name", CASES)
def test_factored_form_equals_the_recorded_response(name):
    meta, z = load_golden(name)
    assert torch.equal(cotangent(meta)[z["bins"]], z["C"])          # the full cotangent is the one the gradients were taken under
    U = stage_matrices(meta, z["param"])
    H = factored_response(U, z["shifts"], z["m_L"], z["m_R"], meta["gain_per_sample"], gamma_of(meta), meta["nfft"], z["bins"])
    err = (H - z["H_f64env"]).abs().max().item()
    quirk = (z["H_ref"] - z["H_f64env"]).abs().max().item()
    print(f"[scattering] {name}: factored form vs H_f64env {err:.2e}; the reference's float32 envelope costs it {quirk:.2e}")
    assert err < 1e-12
    assert quirk < (1e-5 if meta["alias_decay_db"] else 1e-12)


@pytest.mark.parametrize("name", CASES)
def test_mapping_fir_equals_the_recorded_response(name):
    """ScatteringMapping.forward on the CPU: L taps, and rfft(FIR gamma^n) is the recorded response; differentiable"""
    from flamo_amd.processor import dsp
    meta, z = load_golden(name)
    mod = build(dsp, meta, z)
    U = stage_matrices(meta, z["param"]).requires_grad_(True)
    fir = mod.map_filter(U)
    assert fir.shape == (meta["L"], meta["N"], meta["N"]) and mod.map_filter.fir_length() == meta["L"]
    env = torch.tensor(gamma_of(meta), dtype=F64) ** torch.arange(fir.shape[0], dtype=F64)
    H = torch.fft.rfft(fir * env.view(-1, 1, 1), n=meta["nfft"], dim=0)
    assert (H[z["bins"]].detach() - z["H_f64env"]).abs().max().item() < 1e-12
    # its gradient is that of the factored form
    C = cotangent(meta)
    (g1,) = torch.autograd.grad(torch.sum(torch.real(H * C.conj())), [U])
    U2 = U.detach().clone().requires_grad_(True)
    H2 = factored_response(U2, z["shifts"], z["m_L"], z["m_R"], meta["gain_per_sample"], gamma_of(meta), meta["nfft"])
    (g2,) = torch.autograd.grad(torch.sum(torch.real(H2 * C.conj())), [U2])
    assert (g1 - g2).abs().max().item() < 1e-10 * max(1.0, g2.abs().max().item())


def test_golden_gradient_is_that_of_the_factored_form():
    meta, z = load_golden("scat_n4")
    p = z["param"].clone().requires_grad_(True)
    H = factored_response(stage_matrices(meta, p), z["shifts"], z["m_L"], z["m_R"], meta["gain_per_sample"], gamma_of(meta), meta["nfft"])
    (g,) = torch.autograd.grad(torch.sum(torch.real(H * cotangent(meta).conj())), [p])
    assert (g - z["grad"]).abs().max().item() < 1e-10 * z["grad"].abs().max().item()


def test_probe_is_the_factored_form_at_z():
    from flamo_amd.processor import dsp
    meta, z = load_golden("scat_n4")
    mod = build(dsp, meta, z)
    for row in (0, 5, 77, len(z["bins"]) - 1):
        zz = torch.exp(torch.tensor(2j * math.pi * int(z["bins"][row]) / meta["nfft"], dtype=torch.complex128))
        assert (mod.probe(zz).detach() - z["H_f64env"][row]).abs().max().item() < 1e-11


def test_ops_scatter_response_has_no_cpu_fallback():
    from flamo_amd import ops
    U = torch.eye(2).expand(2, 2, 2).contiguous()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scatter_response(U, torch.zeros(1, 2), torch.zeros(2), torch.zeros(2), 1.0, 1.0, 64)
    with pytest.raises(ValueError):
        ops.scatter_response(torch.zeros(2, 2, 3), torch.zeros(1, 2), torch.zeros(2), torch.zeros(2), 1.0, 1.0, 64)
    assert ops.scatter_supported(32, 8) and not ops.scatter_supported(33, 2) and not ops.scatter_supported(4, 9)
    assert not ops.scatter_supported(1, 2) and not ops.scatter_supported(4, 1)


def test_kernel_range_matches_the_library():
    from flamo_amd import _lib, ops
    L = _lib.lib()
    for N in (1, 2, 6, 32, 33):
        for st in (1, 2, 8, 9):
            assert bool(L.fl_scatter_supported(N, st)) == ops.scatter_supported(N, st)
    assert L.fl_scatter_bwd_blocks(4, 0, 0) == 1 and L.fl_scatter_bwd_blocks(4, 481, 0) == 2 * 4       # two 256-bin tiles x 4 columns
    assert L.fl_scatter_response_c64(None, None, None, None, None, None, None, 4, 3, None, 64, 0, 33, None, 64, None) == -1


def test_masked_mse_loss_formula():
    from flamo_amd.optimize import generate_partitions, masked_mse_loss
    torch.manual_seed(0)
    crit = masked_mse_loss(nfft=62, n_samples=8, n_sets=2, regenerate_mask=False)
    assert (crit.nfft, crit.n_samples, crit.n_sets, crit.i) == (62, 8, 2, -1)
    assert crit.mask_indices.shape == (2 * (32 // 8), 8)
    for row in range(0, 8, 4):          # every set is a shuffle of the bins cut into rows: no bin twice
        assert sorted(crit.mask_indices[row:row + 4].reshape(-1).tolist()) == list(range(32))
    y, t = torch.randn(3, 32, 2, dtype=F64, requires_grad=True), torch.randn(3, 32, 2, dtype=F64)
    mask = torch.tensor([5, 0, 31, 7, 8, 9, 2, 30])
    crit.mask_indices = mask.view(1, 8)
    loss = crit(y, t)
    want = ((y[:, mask] - t[:, mask]) ** 2).mean()
    assert torch.equal(loss, want)
    (g,) = torch.autograd.grad(loss, [y])
    keep = torch.zeros(32, dtype=torch.bool)
    keep[mask] = True
    assert (g[:, ~keep] == 0).all() and (g[:, keep] != 0).all()
    p = generate_partitions(torch.arange(10), 3, 2, seed=4)
    assert p.shape == (6, 3) and torch.equal(p, generate_partitions(torch.arange(10), 3, 2, seed=4))


def test_masked_mse_loss_cycles_and_regenerates():
    from flamo_amd.optimize import masked_mse_loss
    torch.manual_seed(1)
    y, t = torch.randn(1, 32, 1), torch.zeros(1, 32, 1)
    fixed = masked_mse_loss(nfft=62, n_samples=16, n_sets=1, regenerate_mask=False)
    first = fixed.mask_indices.clone()
    seen = []
    for _ in range(5):
        fixed(y, t)
        seen.append(fixed.i)
    assert seen == [0, 1, 0, 1, 0] and torch.equal(fixed.mask_indices, first)
    assert torch.equal(fixed(y, t), (y[:, first[1]] ** 2).mean())
    fresh = masked_mse_loss(nfft=62, n_samples=16, n_sets=1, regenerate_mask=True)
    first = fresh.mask_indices.clone()
    fresh(y, t), fresh(y, t)
    assert torch.equal(fresh.mask_indices, first)          # both rows used, not yet regenerated
    fresh(y, t)
    assert fresh.i == 0 and fresh.mask_indices.shape == first.shape and not torch.equal(fresh.mask_indices, first)
