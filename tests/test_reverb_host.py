"""flamo_amd.auxiliary.reverb without a GPU: the float64 torch lines of the delay-scaled attenuation designs against the
reference's recorded responses (tests/golden/reverb.npz), their analytic adjoint -- the arithmetic of csrc/fdnatt.hip's
backward kernels, written out here -- against autograd, the helpers, shapes and state keys, and the new C header."""
import ctypes
import math
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import GOLDEN, check_close, load_golden

F64 = torch.float64
LN10_20 = math.log(10.0) / 20.0


def reverb_golden():
    return load_golden("reverb")


def reverb_cases(classes=None):
    """[(k, case meta, param, delays, H, W, grad or None)] of the recorded module cases"""
    meta, a = reverb_golden()
    delays = torch.tensor(meta["delays"], dtype=F64)
    return [(k, c, a[f"c{k}_param"], delays, a[f"c{k}_H"], a[f"c{k}_W"].to(torch.complex128), a.get(f"c{k}_grad"))
            for k, c in enumerate(meta["cases"]) if classes is None or c["cls"] in classes]


def build_module(case, delays, device=None, dtype=F64, **kw):
    from flamo_amd.auxiliary import reverb
    common = dict(nfft=case["nfft"], delays=delays, alias_decay_db=case["alias_decay_db"], device=device, dtype=dtype)
    if case["cls"] == "parallelFirstOrderShelving":
        return reverb.parallelFirstOrderShelving(rt_nyquist=case["rt_nyquist"], requires_grad=True, **common, **kw)
    if case["cls"] == "parallelFDNGEQ":
        return reverb.parallelFDNGEQ(octave_interval=case["octave_interval"], requires_grad=True, **common, **kw)
    return reverb.parallelFDNAccurateGEQ(octave_interval=case["octave_interval"], **common)


def host_sections(case, param, delays, fs=48000):
    """(b, a) float64 (3, S, N) of a trainable case by the package's host lines"""
    from flamo_amd.auxiliary import reverb
    from flamo_amd.functional import GEQDesign, eq_freqs
    if case["cls"] == "parallelFDNGEQ":
        return reverb.fdn_geq_sections_host(param, delays, fs, GEQDesign(*eq_freqs(interval=case["octave_interval"]), fs=fs, R=2.7))
    return reverb.fdn_shelf1_sections_host(param, delays, fs, reverb.nyquist_slope(case["rt_nyquist"], fs))


# ---- the adjoint of the designs as csrc/fdnatt.hip computes it: dL/d(param) from dL/d(b, a), each (3, S, N)
def geq_adjoint(rt, delays, fs, design, gb, ga):
    """response_common.h geq_design_bwd per (band, line), chained through dg/drt = g (ln 10 / 20) 60 d / (rt^2 fs), summed over lines"""
    nb = design.n_bands
    g = 10 ** ((-60 / (rt * fs)).unsqueeze(-1) * delays.unsqueeze(0) / 20)
    dg = torch.zeros_like(g)
    dg[0] = gb[0, 0]
    for band, i in ((1, 0), (nb - 1, 1)):
        t2, stq = design.sh_t2[i], design.sh_st[i]
        gg = g[band]
        u = torch.sqrt(gg)
        q = torch.sqrt(u)
        du, dq = 0.5 / u, 0.25 * q / gg
        p = [u * t2 + stq * q + 1, 2 * u * t2 - 2, u * t2 - stq * q + 1]
        d = [u + stq * q + t2, 2 * t2 - 2 * u, u - stq * q + t2]
        dp = [t2 * du + stq * dq, 2 * t2 * du, t2 * du - stq * dq]
        dd = [du + stq * dq, -2 * du, du - stq * dq]
        ds = [du * p[j] + u * dp[j] for j in range(3)]
        if band == 1:
            dg[band] = sum(gb[j, band] * ds[j] + ga[j, band] * dd[j] for j in range(3))
        else:
            dg[band] = sum(gb[j, band] * (d[j] + gg * dd[j]) + ga[j, band] * ds[j] for j in range(3))
    t, c = design.pk_t.unsqueeze(-1), design.pk_c.unsqueeze(-1)
    dsg = 0.5 / torch.sqrt(g[2:nb - 1])
    B, A = gb[:, 2:nb - 1], ga[:, 2:nb - 1]
    dg[2:nb - 1] = B[0] * (dsg + t) + B[1] * (-2 * c * dsg) + B[2] * (dsg - t) + A[0] * dsg + A[1] * (-2 * c * dsg) + A[2] * dsg
    return (dg * g * LN10_20 * 60.0 * delays.unsqueeze(0) / (rt * rt * fs).unsqueeze(-1)).sum(dim=1)


def shelf1_adjoint(p, delays, fs, slope_nyq, gb, ga):
    r, wc = p[0], p[1]
    g_nyq = 10 ** (slope_nyq * delays / 20)
    t = torch.tan(wc.clamp(0, math.pi) / 2)
    sk = torch.sqrt(10 ** ((-60 / (r * fs)) * delays / 20) / g_nyq)
    Bs, As = (gb[0, 0] + gb[1, 0]) * g_nyq, ga[0, 0] + ga[1, 0]
    d_sk = Bs * t - As * t / (sk * sk)
    g_rt = (d_sk * sk * (0.5 * LN10_20) * 60.0 * delays / (r * r * fs)).sum()
    g_t = (Bs * sk + As / sk).sum()
    inside = bool(0.0 <= float(wc) <= math.pi)
    return torch.stack([g_rt, g_t * 0.5 * (1 + t * t) if inside else torch.zeros_like(g_t)])


def section_bar(dtype=F64):
    """Bar of the recorded responses of the trainable classes: the float64 GEQ parity bar of tests/test_hip_parity.py
    (test_modules_golden: max(TOL, 2e-6) -- the sections are float32 values behind the host libm's pow / tan, where an ulp
    moves a float32 rounding)"""
    from test_hip_parity import TOL
    return max(TOL[dtype], 2e-6)


def test_host_sections_reproduce_the_recorded_responses():
    from oracle import hotpath as O
    for k, c, param, delays, H, _, _ in reverb_cases(("parallelFDNGEQ", "parallelFirstOrderShelving")):
        b, a = host_sections(c, param, delays)
        S = 1 if c["cls"] == "parallelFirstOrderShelving" else param.shape[0]
        assert b.shape == a.shape == (3, S, len(delays)) and b.dtype == F64
        got = O.sos_response(b, a, c["nfft"], O.gamma_of(c["alias_decay_db"], c["nfft"], F64))
        check_close(f"reverb_host/sections{k}", got, H, section_bar())


def test_host_modules_reproduce_the_recorded_responses():
    """freq_response of the three classes on host float64 parameters; the fitted equaliser at the bar of the existing
    AccurateGEQ golden test (3e-3: its command gains come out of 100 float32 L-BFGS steps)"""
    for k, c, param, delays, H, _, _ in reverb_cases():
        if c["cls"] == "parallelFDNAccurateGEQ" and (c["nfft"], c["alias_decay_db"]) != (960, 30.0):
            continue        # one fit on the host is enough here; the GPU tests run them all
        mod = build_module(c, delays)
        mod.assign_value(param)
        got = mod.freq_response(mod.param)
        assert got.shape == H.shape and got.dtype == torch.complex128
        check_close(f"reverb_host/module{k}", got.detach(), H, 3e-3 if "Accurate" in c["cls"] else section_bar())
        Hp, B, A = mod.get_poly_coeff(mod.map(mod.param.double()))
        assert torch.equal(Hp.detach(), got.detach()) and B.shape[0] == A.shape[0] == c["nfft"] // 2 + 1


def test_host_gradients_against_the_recorded_ones():
    """autograd of the host lines against the reference's gradient, which passes through float32 buffers: 1e-3, the bar of the
    existing g_attn_param checks"""
    for k, c, param, delays, H, W, grad in reverb_cases(("parallelFDNGEQ", "parallelFirstOrderShelving")):
        mod = build_module(c, delays)
        mod.assign_value(param)
        Hm = mod.freq_response(mod.param)
        (g,) = torch.autograd.grad(torch.sum(torch.real(Hm * torch.conj(W))), [mod.param])
        check_close(f"reverb_host/grad{k}", g, grad, 1e-3)


@pytest.mark.parametrize("N,interval", [(1, 1), (4, 1), (6, 3), (33, 1), (65, 3)])
def test_analytic_adjoint_equals_autograd(N, interval):
    """the backward kernels' arithmetic against autograd of the host lines, both float64: 1e-12"""
    from flamo_amd.auxiliary import reverb
    from flamo_amd.functional import GEQDesign, eq_freqs
    gen = torch.Generator().manual_seed(100 + N)
    delays = torch.randint(101, 2401, (N,), generator=gen).double()
    fs = 48000
    design = GEQDesign(*eq_freqs(interval=interval), fs=fs, R=2.7)
    rt = (torch.rand(design.n_bands, dtype=F64, generator=gen) * 2.9 + 0.1).requires_grad_(True)
    b, a = reverb.fdn_geq_sections_host(rt, delays, fs, design)
    gb, ga = torch.randn(b.shape, dtype=F64, generator=gen), torch.randn(a.shape, dtype=F64, generator=gen)
    (g,) = torch.autograd.grad((b * gb).sum() + (a * ga).sum(), [rt])
    check_close(f"reverb_host/geq_adjoint_{N}_{interval}", geq_adjoint(rt.detach(), delays, fs, design, gb, ga), g, 1e-12)
    slope = reverb.nyquist_slope(0.2, fs)
    for wc in (0.4, 2.9, -0.1, 3.5):        # the last two outside the clamp: no gradient for w_c
        p = torch.tensor([1.3, wc], dtype=F64, requires_grad=True)
        b, a = reverb.fdn_shelf1_sections_host(p, delays, fs, slope)
        gb, ga = torch.randn(b.shape, dtype=F64, generator=gen), torch.randn(a.shape, dtype=F64, generator=gen)
        (g,) = torch.autograd.grad((b * gb).sum() + (a * ga).sum(), [p])
        got = shelf1_adjoint(p.detach(), delays, fs, slope, gb, ga)
        check_close(f"reverb_host/shelf_adjoint_{N}_{wc}", got, g, 1e-12)
        assert (got[1] == 0) == (wc < 0 or wc > math.pi)


def test_host_sections_are_float32_values():
    for k, c, param, delays, _, _, _ in reverb_cases(("parallelFDNGEQ",)):
        b, a = host_sections(c, param, delays)
        assert torch.equal(b.float().double(), b) and torch.equal(a.float().double(), a)
    c = dict(cls="parallelFirstOrderShelving", rt_nyquist=0.2)
    b, a = host_sections(c, torch.tensor([1.5, 0.7], dtype=F64), torch.tensor([101.0, 2400.0], dtype=F64))
    assert torch.equal(a.float().double(), a) and torch.count_nonzero(b[2]) == 0 and torch.count_nonzero(a[2]) == 0


def test_helpers():
    from flamo_amd.auxiliary import inverse_map_gamma, map_gamma, map_gfdn_gamma, rt2absorption, rt2slope
    delays = torch.tensor([101, 157, 211, 263], dtype=F64)      # (integer delays make 1 / delays a float32 exponent, as in the reference)
    x = torch.tensor([1.7, 0.0, 0.0, 0.0], dtype=F64)
    y = map_gamma(delays)(x)
    assert y.shape == (4,) and bool((y < 1).all()) and bool((y > 0.99 ** 263).all())
    assert torch.allclose(inverse_map_gamma(delays)(y), x[0].expand(4), rtol=0, atol=1e-9)
    z = map_gamma(delays, is_compressed=False)(torch.tensor([0.999], dtype=F64))
    assert torch.allclose(inverse_map_gamma(delays, is_compressed=False)(z), torch.full((4,), 0.999, dtype=F64), rtol=0, atol=1e-14)
    s = torch.tensor([0.995], dtype=F64)
    assert torch.allclose(torch.sigmoid(inverse_map_gamma()(s)) * 0.01 + 0.99, s, rtol=0, atol=1e-14)
    assert torch.equal(inverse_map_gamma(is_compressed=False)(s), s)
    rt = torch.tensor([0.5, 2.0], dtype=F64)
    assert torch.equal(rt2slope(rt, 48000), -60 / (rt * 48000))
    ab = rt2absorption(rt, 48000, delays)
    assert ab.shape == (2, 4) and torch.allclose(ab[1, 3], torch.tensor(-60 * 263 / (2.0 * 48000), dtype=F64))
    assert torch.equal(map_gfdn_gamma(delays, 2, 48000)(rt), ab)


def test_shapes_and_state_keys():
    from flamo_amd.auxiliary import reverb
    from flamo_amd.processor import dsp, system
    meta, a = reverb_golden()
    delays = torch.tensor(meta["delays"], dtype=F64)
    shapes = {"parallelFDNGEQ": (12,), "parallelFDNAccurateGEQ": (11,), "parallelFirstOrderShelving": (2,)}
    for c in meta["cases"]:
        mod = build_module(c, delays, dtype=torch.float32)
        if c["octave_interval"] == 1:
            assert tuple(mod.param.shape) == shapes[c["cls"]]
        assert list(mod.param.shape) == c["param_shape"] and mod.param.dtype == torch.float32
        assert list(mod.state_dict().keys()) == c["state_keys"]
        assert mod.input_channels == mod.output_channels == len(delays) and mod._diag
        assert mod.param.requires_grad == (c["cls"] != "parallelFDNAccurateGEQ")
    geq = reverb.parallelFDNGEQ(delays=delays)
    assert 1.0 <= float(geq.param.min()) and float(geq.param.max()) <= 3.0 and not geq.param.requires_grad
    with pytest.raises(AssertionError, match="Delays must be provided"):
        reverb.parallelFDNGEQ()
    f = meta["fdn"]
    model, _ = build_fdn(dsp, system, reverb, f, None, F64)
    assert list(model.state_dict().keys()) == f["state_keys"]
    h = meta["homogeneous"]
    hom = reverb.HomogeneousFDN(SimpleNamespace(device=None, dtype=F64, **h["config"]))
    assert list(hom.model.state_dict().keys()) == h["state_keys"] and list(hom.get_raw_parameters().keys()) == h["raw_keys"]
    check_close("reverb_host/rt2gain", hom.rt2gain(torch.tensor([1.0, 2.5], dtype=F64)), a["hom_rt2gain"], 1e-14)
    lines = hom.get_delay_lines()
    lo, hi = (round(ms * 48) for ms in h["config"]["delay_range_ms"])
    assert len(lines) == 4 and len(set(lines)) == 4 and all(lo <= d for d in lines) and max(lines) == lines[-1] > hi


def build_fdn(dsp, system, reverb, f, dev, dtype, a=None, **att_kw):
    """the recorded FDN: Gain -> Recursion(parallelDelay, Series(Matrix, parallelFDNGEQ)) -> Gain in an anti-aliased Shell"""
    from collections import OrderedDict
    N, nfft, db = f["N"], f["nfft"], f["alias_decay_db"]
    kw = dict(nfft=nfft, alias_decay_db=db, device=dev, dtype=dtype)
    fd = torch.tensor(f["delays"], dtype=F64)
    ig = dsp.Gain(size=(N, 1), requires_grad=True, **kw)
    og = dsp.Gain(size=(1, N), requires_grad=True, **kw)
    dl = dsp.parallelDelay(size=(N,), max_len=max(f["delays"]), isint=True, **kw)
    mix = dsp.Matrix(size=(N, N), matrix_type="orthogonal", requires_grad=True, **kw)
    att = reverb.parallelFDNGEQ(octave_interval=1, delays=fd, requires_grad=True, **kw, **att_kw)
    if a is not None:
        for mod, key in ((ig, "fdn_in_gain"), (og, "fdn_out_gain"), (dl, "fdn_delays_s"), (mix, "fdn_U_param"), (att, "fdn_attn_param")):
            mod.assign_value(a[key].to(device=dev, dtype=dtype))
    rec = system.Recursion(fF=dl, fB=system.Series(OrderedDict({"mixing_matrix": mix, "attenuation": att})))
    core = system.Series(OrderedDict({"input_gain": ig, "feedback_loop": rec, "output_gain": og}))
    model = system.Shell(core, dsp.FFT(nfft, dtype=dtype), dsp.iFFTAntiAlias(nfft, alias_decay_db=db, device=dev, dtype=dtype))
    return model, dict(ig=ig, og=og, mix=mix, att=att)


def test_fixture_size():
    assert os.path.getsize(os.path.join(GOLDEN, "reverb.npz")) < 600 * 1024
    meta, a = reverb_golden()
    assert not any(v.dim() == 3 and v.is_complex() for v in a.values())       # no (M, S, N) section spectra


def test_header_declares_what_the_library_exports():
    from flamo_amd import _lib
    syms = sorted(_lib._SIGNATURES_FDNATT)
    assert syms == ["fl_fdn_geq_sections", "fl_fdn_geq_sections_bwd", "fl_fdn_shelf1_sections", "fl_fdn_shelf1_sections_bwd"]
    if os.path.exists(_lib.LIB_PATH):
        handle = ctypes.CDLL(_lib.LIB_PATH)
        for s in syms:
            assert hasattr(handle, s), f"{s} declared in include/flamo_hip_fdnatt.h but not exported"
    for name, (res, args) in _lib._SIGNATURES_FDNATT.items():
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p, name
    assert not set(syms) & set(_lib.EXPORTS) and len(_lib.EXPORTS) == 183
