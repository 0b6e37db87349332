"""flamo_amd.auxiliary.reverb on the GPU: the three attenuation classes against the reference's recorded responses and
gradients (tests/golden/reverb.npz), the design kernels of csrc/fdnatt.hip alone against the package's host float64 lines,
determinism, the recorded FDN and HomogeneousFDN, which route a module takes, and a captured training step.

Bars.  Recorded responses of the trainable classes and the FDN's output: 2e-6 (float32 section values in the reference).  The
fitted equaliser: 3e-3 against the recording (test_modules_golden), 1e-10 / 1e-5 against the oracle on the sections this run
fitted (test_accurate_geq_kernels_tight).  Sections: two float32 ulps of a section's largest tap.  Gradients: 1e-3 against the
reference's (float32 buffers behind it), 5 TOL[dtype] against the float64 autograd of the host lines."""
from collections import OrderedDict
from types import SimpleNamespace

import pytest
import torch

from conftest import check_close
from test_hip_parity import CD, TOL
from test_reverb_host import F64, build_fdn, build_module, reverb_cases, reverb_golden

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32]
TRAINABLE = ("parallelFDNGEQ", "parallelFirstOrderShelving")
FS = 48000


def _tag(dtype):
    return str(dtype)[-2:]


def _device_module(case, delays, param, gpu, dtype, **kw):
    mod = build_module(case, delays, device=gpu, dtype=dtype, **kw)
    mod.assign_value(param.to(device=gpu, dtype=dtype))
    return mod


def _cascade_node(H):
    """the autograd node of the cascade behind a response (M, N)"""
    node = H.grad_fn
    while node is not None and type(node).__name__ != "_CascadeBackward":
        node = node.next_functions[0][0] if node.next_functions else None
    return node


_host = {}


def _host_gradient(k):
    """gradient of Re sum conj(W) H of recorded case k by float64 autograd of the host lines, computed once"""
    if k not in _host:
        _, c, param, delays, _, W, _ = reverb_cases()[k]
        mod = build_module(c, delays)
        mod.assign_value(param)
        (g,) = torch.autograd.grad(torch.sum(torch.real(mod.freq_response(mod.param) * torch.conj(W))), [mod.param])
        _host[k] = g
    return _host[k]


@pytest.mark.parametrize("dtype", DTYPES)
def test_recorded_responses_and_gradients(gpu, dtype):
    from flamo_amd import ops
    for k, c, param, delays, H, W, grad in reverb_cases(TRAINABLE):
        mod = _device_module(c, delays, param, gpu, dtype)
        got = mod.freq_response(mod.param)
        assert got.shape == H.shape and got.dtype == CD[dtype]
        assert isinstance(_cascade_node(got).design, ops.FdnAttenuation)
        tag = f"reverb_gpu/case{k}_{_tag(dtype)}"
        check_close(tag + "/H", got.detach().cpu(), H, 2e-6)
        (g,) = torch.autograd.grad(torch.sum(torch.real(got * torch.conj(W.to(device=gpu, dtype=CD[dtype])))), [mod.param])
        assert g.dtype == dtype and g.shape == param.shape
        check_close(tag + "/grad_vs_reference", g.cpu(), grad, 1e-3)
        check_close(tag + "/grad_vs_host_float64", g.cpu(), _host_gradient(k), 5 * TOL[dtype])
        (g2,) = torch.autograd.grad(torch.sum(torch.real(mod.freq_response(mod.param) * torch.conj(W.to(device=gpu, dtype=CD[dtype])))),
                                    [mod.param])
        assert torch.equal(g, g2)                 # two runs: the same bits


@pytest.mark.parametrize("dtype", DTYPES)
def test_fitted_equaliser(gpu, dtype):
    from oracle import hotpath as O
    for k, c, param, delays, H, _, _ in reverb_cases(("parallelFDNAccurateGEQ",)):
        mod = _device_module(c, delays, param, gpu, dtype)
        got = mod.freq_response(mod.param)
        assert got.shape == H.shape and got.dtype == CD[dtype] and not got.requires_grad
        tag = f"reverb_gpu/case{k}_{_tag(dtype)}"
        check_close(tag + "/H", got.cpu(), H, 3e-3)
        b, a = mod._sos_coeffs(mod.map(mod.param.double()))
        assert b.shape == (3, mod.n_gains + 1, len(delays))
        Href = O.sos_response(b.cpu().double(), a.cpu().double(), c["nfft"], O.gamma_of(c["alias_decay_db"], c["nfft"], F64))
        check_close(tag + "/H_vs_oracle_on_these_sections", got.cpu(), Href, 1e-10 if dtype == F64 else 1e-5)
        key = mod._design_cache[0]
        mod.freq_response(mod.param)
        assert mod._design_cache[0] is key        # the design is cached per parameter value: a second call does not refit


# ---- the design kernels alone
def _design_inputs(N, interval):
    from flamo_amd.functional import GEQDesign, eq_freqs
    gen = torch.Generator().manual_seed(7 * N + interval)
    delays = torch.randint(101, 2401, (N,), generator=gen).double()
    delays[0], delays[-1] = (101.0, 2400.0) if N > 1 else (2400.0, 2400.0)
    design = GEQDesign(*eq_freqs(interval=interval), fs=FS, R=2.7)
    rt = (torch.rand(design.n_bands, dtype=F64, generator=gen) * 2.9 + 0.1).float().double()
    rt[0], rt[-1] = torch.tensor(0.1).float().double(), 3.0
    return gen, delays, design, rt


def _check_sections(tag, got, ref):
    """|difference| of every tap within two float32 ulps (2.4e-7) of its section's largest tap"""
    largest = ref.abs().amax(dim=0, keepdim=True)
    worst = ((got - ref).abs() / largest).max().item()
    print(f"[parity] {tag}: worst tap difference {worst:.3e} of the section's largest tap (limit 2.4e-07)")
    assert worst <= 2.4e-7, (tag, worst)


@pytest.mark.parametrize("N", [1, 4, 6, 33, 65])
@pytest.mark.parametrize("interval", [1, 3])
def test_design_kernels_against_the_host_lines(gpu, N, interval):
    from flamo_amd import ops
    from flamo_amd.auxiliary import reverb
    gen, delays, design, rt = _design_inputs(N, interval)
    assert design.n_bands == (12 if interval == 1 else 30)
    slope = reverb.nyquist_slope(0.2, FS)
    d_dev = delays.to(gpu)
    packed = torch.cat([d_dev, design.device_consts(gpu)]).contiguous()
    jobs = [("geq", rt, lambda p: reverb.fdn_geq_sections_host(p, delays, FS, design),
             lambda p: ops.FdnAttenuation("fdn_geq", p, packed, N, float(FS), 0.0))]
    for wc in (0.7, 2.6, 3.5):           # 3.5: above the clamp, no gradient for w_c
        p0 = torch.tensor([1.3, wc]).double()
        jobs.append((f"shelf{wc}", p0, lambda p: reverb.fdn_shelf1_sections_host(p, delays, FS, slope),
                     lambda p: ops.FdnAttenuation("fdn_shelf1", p, d_dev, N, float(FS), slope)))
    for name, p0, host_fn, design_of in jobs:
        ph = p0.clone().requires_grad_(True)
        bh, ah = host_fn(ph)
        gb, ga = torch.randn(bh.shape, dtype=F64, generator=gen), torch.randn(ah.shape, dtype=F64, generator=gen)
        (gh,) = torch.autograd.grad((bh * gb).sum() + (ah * ga).sum(), [ph])
        for dtype in DTYPES:
            pd = p0.to(device=gpu, dtype=dtype).requires_grad_(True)
            b, a = ops.fdn_sections(design_of(pd))
            assert type(b.grad_fn).__name__ == "_FdnSectionsBackward" and b.dtype == F64 and b.shape == bh.shape
            tag = f"reverb_gpu/design_{name}_{N}_{interval}_{_tag(dtype)}"
            _check_sections(tag + "/b", b.detach().cpu(), bh.detach())
            _check_sections(tag + "/a", a.detach().cpu(), ah.detach())
            (g,) = torch.autograd.grad((b * gb.to(gpu)).sum() + (a * ga.to(gpu)).sum(), [pd])
            assert g.dtype == dtype
            check_close(tag + "/grad", g.cpu(), gh, 5 * TOL[dtype])
            if name == "shelf3.5":
                assert g[1].item() == 0.0 and gh[1].item() == 0.0


def test_design_backward_sums_block_partials_in_order(gpu):
    """the backward entry on several blocks of partials equals the one on their sum, and two runs give the same bits"""
    from flamo_amd import ops
    gen, delays, design, rt = _design_inputs(33, 1)
    packed = torch.cat([delays.to(gpu), design.device_consts(gpu)]).contiguous()
    d = ops.FdnAttenuation("fdn_geq", rt.to(gpu), packed, 33, float(FS), 0.0)
    part = torch.randn(5, 2, 3, 12, 33, dtype=F64, generator=gen).to(gpu)
    sec = (rt.to(gpu), packed)
    g5, _ = d.param_grads(sec, part)
    g5b, _ = d.param_grads(sec, part)
    g1, _ = d.param_grads(sec, part.sum(dim=0, keepdim=True).contiguous())
    assert torch.equal(g5, g5b)
    check_close("reverb_gpu/block_partials", g5.cpu(), g1.cpu(), 1e-13)


def test_arguments_the_design_refuses(gpu):
    from flamo_amd import ops
    d = torch.tensor([101.0, 157.0], dtype=F64, device=gpu)
    with pytest.raises(ValueError, match="packed"):
        ops.fdn_sections(ops.FdnAttenuation("fdn_geq", torch.ones(12, device=gpu), d, 2, 48000.0, 0.0))
    with pytest.raises(ValueError, match="parameters"):
        ops.fdn_sections(ops.FdnAttenuation("fdn_shelf1", torch.ones(3, device=gpu), d, 2, 48000.0, -0.00625))
    with pytest.raises(ValueError, match="unknown kind"):
        ops.fdn_sections(ops.FdnAttenuation("fdn_peq", torch.ones(2, device=gpu), d, 2, 48000.0, 0.0))


# ---- routes
@pytest.mark.parametrize("dtype", DTYPES)
def test_route_selection(gpu, dtype):
    """default map: the design kernel; a user-assigned map or fold_map=False: the torch lines, and the same response and
    gradient within the float32 bar"""
    from flamo_amd import ops
    for k, c, param, delays, H, W, _ in reverb_cases(TRAINABLE):
        if (c["nfft"], c["alias_decay_db"]) != (960, 30.0):
            continue
        Wd = W.to(device=gpu, dtype=CD[dtype])
        kernel = _device_module(c, delays, param, gpu, dtype)
        assert isinstance(kernel._cascade_spec(kernel.param), ops.FdnAttenuation)
        Hk = kernel.freq_response(kernel.param)
        (gk,) = torch.autograd.grad(torch.sum(torch.real(Hk * torch.conj(Wd))), [kernel.param])
        unfolded = _device_module(c, delays, param, gpu, dtype, fold_map=False)
        mapped = _device_module(c, delays, param, gpu, dtype)
        own = mapped.map
        mapped.map = lambda x: own(x)
        for name, mod in (("fold_map_false", unfolded), ("user_map", mapped)):
            assert isinstance(mod._cascade_spec(mod.param), ops.RawSections)
            Ht = mod.freq_response(mod.param)
            assert isinstance(_cascade_node(Ht).design, ops.RawSections)
            tag = f"reverb_gpu/route_{name}_{k}_{_tag(dtype)}"
            check_close(tag + "/H", Ht.detach().cpu(), Hk.detach().cpu(), 2e-6)
            check_close(tag + "/H_vs_reference", Ht.detach().cpu(), H, 2e-6)
            (gt,) = torch.autograd.grad(torch.sum(torch.real(Ht * torch.conj(Wd))), [mod.param])
            check_close(tag + "/grad", gt.cpu(), gk.cpu(), 5 * TOL[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
def test_standing_alone_and_inside_series(gpu, dtype):
    """module(X) = H X per line; Series(Matrix, module)(X) = H (W X)"""
    from flamo_amd.processor import dsp, system
    gen = torch.Generator().manual_seed(5)
    for k, c, param, delays, H, _, _ in reverb_cases():
        if (c["nfft"], c["alias_decay_db"]) != (960, 30.0) or c["octave_interval"] != 1:
            continue
        N, M = len(delays), c["nfft"] // 2 + 1
        mod = _device_module(c, delays, param, gpu, dtype)
        X = torch.randn(2, M, N, dtype=torch.complex128, generator=gen).to(torch.complex64).to(torch.complex128)
        tol = 3e-3 if "Accurate" in c["cls"] else 2e-6
        tag = f"reverb_gpu/apply{k}_{_tag(dtype)}"
        Y = mod(X.to(device=gpu, dtype=CD[dtype]))
        check_close(tag + "/alone", Y.detach().cpu(), H.unsqueeze(0) * X, tol)
        Hp, B, A = mod.get_poly_coeff(mod.map(mod.param.double()))      # (H, B, A) as the reference returns them
        S = {"parallelFDNGEQ": 12, "parallelFDNAccurateGEQ": 12, "parallelFirstOrderShelving": 1}[c["cls"]]
        assert B.shape == A.shape == (M, S, N) and B.dtype == CD[dtype]
        check_close(tag + "/poly_H", Hp.detach().cpu(), mod.freq_response(mod.param).detach().cpu(), 2e-6)
        if dtype == F64:      # section spectra cancel to 1e-5 of their taps near DC: 12 sections x 1e-16 x 1e5, rounded up
            check_close(tag + "/poly_BA", (B.prod(dim=1) / A.prod(dim=1)).detach().cpu(), Hp.detach().cpu(), 1e-9)
        mat = dsp.Matrix(size=(N, N), nfft=c["nfft"], alias_decay_db=c["alias_decay_db"], device=gpu, dtype=dtype)
        Wm = torch.randn(N, N, dtype=F64, generator=gen).float().double()
        mat.assign_value(Wm.to(device=gpu, dtype=dtype))
        Ys = system.Series(OrderedDict(mix=mat, att=mod))(X.to(device=gpu, dtype=CD[dtype]))
        ref = H.unsqueeze(0) * torch.einsum("nm,bfm->bfn", Wm.to(torch.complex128), X)
        check_close(tag + "/series", Ys.detach().cpu(), ref, tol)
        with pytest.raises(ValueError):
            mod(torch.zeros(1, M, N + 1, dtype=CD[dtype], device=gpu))


# ---- the recorded FDN
def _fdn(gpu, dtype, **att_kw):
    from flamo_amd.auxiliary import reverb
    from flamo_amd.processor import dsp, system
    meta, a = reverb_golden()
    model, p = build_fdn(dsp, system, reverb, meta["fdn"], gpu, dtype, a, **att_kw)
    return meta["fdn"], a, model, p


@pytest.mark.parametrize("dtype", DTYPES)
def test_recorded_fdn(gpu, dtype):
    """Shell(FFT, Series(Gain, Recursion(parallelDelay, Series(Matrix, parallelFDNGEQ)), Gain), iFFTAntiAlias): output at
    2e-6, parameter gradients at the bars of test_fdn_golden (5 x max(TOL, 2e-6); the attenuation's 1e-3 against the
    reference's float32-buffer gradient), state keys"""
    f, a, model, p = _fdn(gpu, dtype)
    assert list(model.state_dict().keys()) == f["state_keys"]
    x = a["fdn_x"].to(device=gpu, dtype=dtype).requires_grad_(True)
    y = model(x)
    tag = f"reverb_gpu/fdn_{_tag(dtype)}"
    check_close(tag + "/y", y.detach().cpu(), a["fdn_y"], 2e-6)
    plist = [p["ig"].param, p["og"].param, p["mix"].param, p["att"].param]
    g = torch.autograd.grad(torch.sum(y * a["fdn_c"].to(device=gpu, dtype=dtype)), [x] + plist)
    tol = max(TOL[dtype], 2e-6)
    for got, key in zip(g, ["fdn_gx", "fdn_g_in_gain", "fdn_g_out_gain", "fdn_g_U_param", "fdn_g_attn_param"]):
        check_close(f"{tag}/{key}", got.cpu(), a[key], 1e-3 if key == "fdn_g_attn_param" else 5 * tol)
    # the same system on the torch lines: the attenuation's gradient by another route, at the float64-backward bar
    _, _, model_t, pt = _fdn(gpu, dtype, fold_map=False)
    yt = model_t(a["fdn_x"].to(device=gpu, dtype=dtype))
    (gt,) = torch.autograd.grad(torch.sum(yt * a["fdn_c"].to(device=gpu, dtype=dtype)), [pt["att"].param])
    check_close(tag + "/y_vs_torch_lines", y.detach().cpu(), yt.detach().cpu(), 2e-6)
    check_close(tag + "/g_attn_vs_torch_lines", g[4].cpu(), gt.cpu(), 5 * TOL[dtype])


def test_captured_training_step(gpu):
    """one training step of the recorded FDN under mse_loss, replayed by GraphedStep: the eager loss"""
    from flamo_amd.graph import GraphedStep
    from flamo_amd.optimize import mse_loss
    f, a, model, p = _fdn(gpu, torch.float32)
    x = a["fdn_x"].to(device=gpu, dtype=torch.float32)
    target = (a["fdn_y"] * 0.5).to(device=gpu, dtype=torch.float32)
    crit = mse_loss()
    params = [p["ig"].param, p["og"].param, p["mix"].param, p["att"].param]

    def eager_step():
        # (the step's autograd graph must be gone before the capture: its gradient accumulators remember the default stream)
        loss = crit(model(x), target)
        grads = torch.autograd.grad(loss, params)
        return loss.detach().clone(), [g.clone() for g in grads]

    loss, grads = eager_step()
    assert torch.isfinite(loss) and loss.item() > 0
    gs = GraphedStep(lambda xx: crit(model(xx), target), (x,), params, warmup=2)
    for _ in range(2):
        lg = gs.replay()
    torch.cuda.synchronize()
    assert abs(lg.item() - loss.item()) <= 1e-6 * abs(loss.item())
    check_close("reverb_gpu/replay_g_attn", p["att"].param.grad.cpu(), grads[3].cpu(), 1e-5)
    check_close("reverb_gpu/replay_g_U", p["mix"].param.grad.cpu(), grads[2].cpu(), 1e-5)


# ---- HomogeneousFDN
@pytest.mark.parametrize("dtype", DTYPES)
def test_homogeneous_fdn(gpu, dtype):
    from flamo_amd.auxiliary import HomogeneousFDN
    meta, a = reverb_golden()
    h = meta["homogeneous"]
    hom = HomogeneousFDN(SimpleNamespace(device=gpu, dtype=dtype, **h["config"]))
    assert list(hom.model.state_dict().keys()) == h["state_keys"]
    raw = {key: a[f"hom_{key}"].numpy() for key in h["raw_keys"]}
    hom.set_raw_parameters(raw)
    back = hom.get_raw_parameters()
    assert list(back.keys()) == h["raw_keys"]
    for key in raw:               # set / get round trip, to the module's precision
        assert back[key].shape == raw[key].shape
        assert torch.equal(torch.from_numpy(back[key]).to(dtype), torch.from_numpy(raw[key]).to(dtype)), key
    with torch.no_grad():
        y = hom.model(a["hom_x"].to(device=gpu, dtype=dtype))
    check_close(f"reverb_gpu/homogeneous_{_tag(dtype)}/y", y.cpu(), a["hom_y"], max(TOL[dtype], 1e-8))
    hom.normalize_energy(target_energy=1)         # carries its own assertion
    H = hom.model.get_freq_response(identity=False)
    assert abs(torch.mean(torch.abs(H) ** 2).item() - 1.0) < 1e-4
    gains = hom.rt2gain(torch.tensor([1.0, 2.5], dtype=F64))
    check_close(f"reverb_gpu/homogeneous_{_tag(dtype)}/rt2gain", gains, a["hom_rt2gain"], 1e-14)
