"""GPU parity tests: the HIP path (through the C ABI) against
  * the golden vectors produced by the reference itself (float64), and
  * the CPU oracle on seeded inputs, plus size-independent properties at BASELINE sizes.

Tolerances (relative l2 error against the float64 reference):
  float64 kernels 1e-10, float32 kernels 1e-5 (BASELINE.json north_star: <= 1e-5).
"""
import ctypes
from collections import OrderedDict

import pytest
import torch

from conftest import cc, check_close, check_closer, golden_names, load_golden

pytestmark = pytest.mark.gpu

TOL = {torch.float64: 1e-10, torch.float32: 1e-5}
CD = {torch.float64: torch.complex128, torch.float32: torch.complex64}


def _dev(t, dev, dt):
    if t.is_complex():
        return t.to(device=dev, dtype=CD[dt])
    return t.to(device=dev, dtype=dt)


@pytest.fixture(params=[torch.float64, torch.float32], ids=["f64", "f32"])
def dt(request):
    return request.param


@pytest.fixture(params=[0, 8], ids=["plan-default", "plan-two-pass"])
def plan(request):
    """Force the two-pass (four-step) FFT on small goldens so that path is covered too."""
    from flamo_amd import _lib
    _lib.lib().fl_debug_set_fft_max_single(request.param)
    yield request.param
    _lib.lib().fl_debug_set_fft_max_single(0)


# ----------------------------------------------------------------------------- transforms
@pytest.mark.parametrize("name", golden_names("fft_"))
def test_transforms_golden(gpu, dt, plan, name):
    from flamo_amd import ops
    meta, a = load_golden(name)
    nfft, norm, db = meta["nfft"], meta["norm"], meta["alias_decay_db"]
    x = _dev(a["x"], gpu, dt).requires_grad_(True)
    X = ops.rfft(x, nfft, norm, db)
    assert X.shape == a["X"].shape
    cc("X", X.cpu(), a['X'], TOL[dt])
    (gx,) = torch.autograd.grad(torch.sum(torch.real(X * torch.conj(_dev(a["C"], gpu, dt)))), [x])
    cc("gx", gx.cpu(), a['gx'], TOL[dt])
    Z = _dev(a["Z"], gpu, dt).requires_grad_(True)
    y = ops.irfft(Z, nfft, norm, db)
    assert y.shape == a["y"].shape
    cc("y", y.cpu(), a['y'], TOL[dt])
    (gZ,) = torch.autograd.grad(torch.sum(y * _dev(a["c"], gpu, dt)), [Z])
    cc("gZ", gZ.cpu(), a['gZ'], TOL[dt])


@pytest.mark.parametrize("nfft", [96000, 192000, 384000, 2 * 7 * 11 * 13 * 4])
def test_fft_full_size_properties(gpu, nfft):
    """BASELINE sizes: oracle comparison, round trip, linearity and Parseval."""
    from flamo_amd import ops
    from oracle import hotpath as O
    torch.manual_seed(nfft)
    for dt_, tol in ((torch.float32, 1e-5), (torch.float64, 1e-10)):
        x = torch.randn(2, nfft, 3, dtype=dt_, device=gpu)
        X = ops.rfft(x, nfft)
        cc("X", X.cpu(), O.rfft(x.cpu().double(), nfft), tol)
        y = ops.irfft(X, nfft)
        cc("y", y, x, tol)  # round trip
        x2 = torch.randn_like(x)
        lin = ops.rfft(2.5 * x - x2, nfft) - (2.5 * X - ops.rfft(x2, nfft))
        assert (lin.abs().max() / X.abs().max()).item() < (1e-5 if dt_ == torch.float32 else 1e-12)
        # Parseval with Hermitian weights
        w = torch.full((nfft // 2 + 1,), 2.0, device=gpu, dtype=dt_)
        w[0] = 1
        w[-1] = 1
        e_f = (X.abs() ** 2 * w.view(1, -1, 1)).sum() / nfft
        assert abs((e_f / (x ** 2).sum()).item() - 1) < (1e-4 if dt_ == torch.float32 else 1e-11)
        # anti-alias pair undoes itself up to gamma^-2t: irfft_aa(rfft_aa(x)) = x * gamma^-2t
        ya = ops.irfft(ops.rfft(x, nfft, "backward", 30.0), nfft, "backward", 30.0)
        env2 = O.alias_envelope(30.0, nfft).to(gpu) ** 2
        cc("ya", ya.double(), x.double() * env2.view(1, -1, 1), tol)


def test_fft_fast_kernels_match_generic(gpu):
    """The two-register-stage kernels (production lengths) against the generic Stockham kernels."""
    from flamo_amd import _lib, ops
    L = _lib.lib()
    for nfft in (96000, 192000, 384000):
        for dt_, tol in ((torch.float32, 2e-6), (torch.float64, 1e-13)):
            x = torch.randn(3, nfft, 2, dtype=dt_, device=gpu)
            Z = torch.randn(3, nfft // 2 + 1, 2, dtype=CD[dt_], device=gpu)
            Xf, yf = ops.rfft(x, nfft, "backward", 30.0), ops.irfft(Z, nfft, "ortho", 30.0)
            L.fl_debug_set_fft_fast(0)
            try:
                Xg, yg = ops.rfft(x, nfft, "backward", 30.0), ops.irfft(Z, nfft, "ortho", 30.0)
            finally:
                L.fl_debug_set_fft_fast(1)
            cc("Xf", Xf, Xg, tol)
            cc("yf", yf, yg, tol)
            L.fl_debug_set_fft_fast(2)          # fast kernels, inverse column pass without mirror-column pairing
            try:
                yu = ops.irfft(Z, nfft, "ortho", 30.0)
            finally:
                L.fl_debug_set_fft_fast(1)
            cc("yf", yf, yu, tol)


def test_fft_ragged_and_layouts(gpu):
    from flamo_amd import ops
    from oracle import hotpath as O
    nfft = 1500
    for T in (1, 7, 751, 1500, 1777):
        x = torch.randn(3, T, 2, dtype=torch.float64, device=gpu, requires_grad=True)
        X = ops.rfft(x, nfft, "ortho")
        xr = x.detach().cpu().requires_grad_(True)
        Xr = O.rfft(xr, nfft, "ortho")
        cc("X", X.cpu(), Xr, 1e-10)
        C = torch.randn_like(Xr)
        (g,) = torch.autograd.grad(torch.sum(torch.real(X * torch.conj(C.to(gpu)))), [x])
        (gr,) = torch.autograd.grad(torch.sum(torch.real(Xr * torch.conj(C))), [xr])
        assert g.shape == x.shape
        cc("g", g.cpu(), gr, 1e-10)
    # channel-innermost source read directly by the first FFT pass (fl_rfft_ci_*), both plans
    from flamo_amd import _lib
    ops.CI_MAX_CHANNELS = 16
    try:
        for max_single in (0, 8):
            _lib.lib().fl_debug_set_fft_max_single(max_single)
            for T in (751, 1500, 1777):
                x = torch.randn(3, T, 2, 2, dtype=torch.float64, device=gpu)
                cc("ops_rfft_x_nfft_backward", ops.rfft(x, nfft, 'backward').cpu(), O.rfft(x.cpu(), nfft), 1e-10)
        xb = torch.randn(2, 96000, 8, dtype=torch.float32, device=gpu)       # fast kernels, XCD-grouped blocks
        cc("ops_rfft_xb_96000", ops.rfft(xb, 96000).cpu(), O.rfft(xb.cpu().double(), 96000), 1e-05)
    finally:
        ops.CI_MAX_CHANNELS = 0
        _lib.lib().fl_debug_set_fft_max_single(0)
    # planar input (time axis contiguous) and empty batch
    xp = torch.randn(2, 3, nfft, dtype=torch.float64, device=gpu).movedim(-1, 1)
    cc("ops_rfft_xp_nfft", ops.rfft(xp, nfft).cpu(), O.rfft(xp.cpu(), nfft), 1e-10)
    assert ops.rfft(torch.zeros(0, nfft, 2, dtype=torch.float32, device=gpu), nfft).shape == (0, nfft // 2 + 1, 2)
    # half-length 17: no Stockham plan (the C ABI says so) -- the operator takes the chirp-z route (tests/test_round4.py)
    import ctypes
    l1, l2 = ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().fl_fft_plan(34, 0, ctypes.byref(l1), ctypes.byref(l2)) != 0 and not ops.fft_plan_ok(34, torch.float32)
    x34 = torch.randn(1, 34, 1, device=gpu)
    cc("ops_rfft_x34_34", ops.rfft(x34, 34).cpu(), O.rfft(x34.cpu().double(), 34), 1e-05)


# ----------------------------------------------------------------------------- modules
_MODULE_CASES = [n for n in golden_names() if load_golden(n)[0].get("cls")]


def _build_module(meta, a, dev, dt):
    from flamo_amd.processor import dsp
    kw = dict(meta["kwargs"])
    kw["size"] = tuple(kw["size"])
    mod = getattr(dsp, meta["cls"])(nfft=meta["nfft"], alias_decay_db=meta["alias_decay_db"], device=dev, dtype=dt,
                                    **kw)
    mod.assign_value(_dev(a["param"], dev, dt))
    return mod


def _f32_exact(t):
    """Round to float32 and back: values both the float32 GPU run and the float64 oracle can hold."""
    if t.is_complex():
        return t.to(torch.complex64).to(torch.complex128)
    return t.to(torch.float32).to(torch.float64)


def _module_reference(meta, a, dt):
    """Expected values for a module case.  float64: the golden vectors (the reference's own
    output).  float32: the pinned float64 oracle evaluated on the float32-rounded parameters and
    inputs -- the GEQ/Biquad cascades are ill-conditioned in their parameters at low frequency,
    so the comparison must start from the very same parameter values."""
    from test_oracle_golden import ORACLE_CLASSES, _module_response
    if dt == torch.float64 or meta["cls"] not in ORACLE_CLASSES:
        return a        # (float32 runs of the classes without an oracle restatement use the goldens, looser tolerance)
    from oracle import hotpath as O
    diag = meta["cls"].startswith("parallel")
    param = _f32_exact(a["param"]).requires_grad_(True)
    H, kind = _module_response(meta, a, param)
    fn = {("const", False): O.mimo_const, ("const", True): O.mimo_const_diag,
          ("bin", False): O.mimo_full, ("bin", True): O.mimo_diag}[(kind, diag)]
    X = _f32_exact(a["X"]).requires_grad_(True)
    C = _f32_exact(a["C"])
    Y = fn(H, X)
    g = torch.autograd.grad(torch.sum(torch.real(Y * torch.conj(C))), [X, param], allow_unused=True)
    X4 = _f32_exact(a["X4"])
    ref = dict(param=param.detach(), X=X.detach(), C=C, Y=Y.detach(), gX=g[0], X4=X4, Y4=fn(H.detach(), X4))
    if kind == "bin":
        ref["freq_response"] = H.detach()
    if "gparam" in a:
        ref["gparam"] = g[1]
    return ref


@pytest.mark.parametrize("name", _MODULE_CASES)
def test_modules_golden(gpu, dt, name):
    meta, a = load_golden(name)
    a = _module_reference(meta, a, dt)
    mod = _build_module(meta, a, gpu, dt)
    # GEQ sections are float32 inside the reference and their tan()/cos() constants come from the
    # host's float32 libm, which differs by an ulp between hosts: float32-class agreement there
    tol = max(TOL[dt], 2e-6) if "GEQ" in meta["cls"] else TOL[dt]
    from test_oracle_golden import ORACLE_CLASSES
    if meta["cls"] not in ORACLE_CLASSES:
        # SVF / PEQ sections are float32 in the reference (host libm ulps, as for GEQ); in float32 mode the
        # parameters themselves are rounded before the (steep) parameter maps
        tol = 2e-6 if dt == torch.float64 else 2e-4
    if "AccurateGEQ" in meta["cls"]:
        # the command gains come out of 100 float32 L-BFGS steps on the host: the reference's own result moves
        # by ~5e-4 from one host CPU to another (BLAS / libm ulps amplified by the iteration); the kernels
        # behind it are held to the usual tolerance in test_accurate_geq_kernels_tight below
        tol = 3e-3
    if "freq_response" in a:
        H = mod.freq_response(mod.param)
        assert H.shape == a["freq_response"].shape
        cc("H", H.detach().cpu(), a['freq_response'], tol)
    X = _dev(a["X"], gpu, dt).requires_grad_(True)
    Y = mod(X)
    assert Y.shape == a["Y"].shape
    cc("Y", Y.detach().cpu(), a['Y'], tol)
    wrt = [X] + ([mod.param] if "gparam" in a else [])
    g = torch.autograd.grad(torch.sum(torch.real(Y * torch.conj(_dev(a["C"], gpu, dt)))), wrt)
    cc("g_0", g[0].cpu(), a['gX'], tol)
    if "gparam" in a:
        # the reference's GEQ gradient itself passes through float32 buffers (dsp.py:2573-2585): 1e-4 class
        gtol = 1e-3 if ("GEQ" in meta["cls"] or meta["cls"] not in ORACLE_CLASSES) else max(tol, 1e-9)
        cc("g_1", g[1].cpu(), a['gparam'], gtol)
    # matrix-valued signal (B, M, N, N): the identity-probe path
    Y4 = mod(_dev(a["X4"], gpu, dt))
    cc("Y4", Y4.detach().cpu(), a['Y4'], tol)
    # channel-innermost (reference-contiguous) input gives the same result as planar input
    Yc = mod(_dev(a["X"], gpu, dt).contiguous())
    cc("Yc", Yc.detach().cpu(), a['Y'], tol)
    with pytest.raises(ValueError):
        mod(torch.zeros(1, meta["nfft"] // 2 + 1, a["X"].shape[2] + 1, dtype=CD[dt], device=gpu))


def test_integer_delay_phase_is_exact(gpu):
    """bit-exact integer delay indexing: the f32 response equals the correctly rounded f64 one."""
    from flamo_amd.processor import dsp
    from oracle import hotpath as O
    nfft = 192000
    m = torch.tensor([503.0, 997.0, 1499.0, 2713.0])
    d32 = dsp.parallelDelay(size=(4,), max_len=3000, isint=True, nfft=nfft, alias_decay_db=30.0, device=gpu)
    d32.assign_value(d32.sample2s(m.to(gpu)))
    H32 = d32.freq_response(d32.param).cpu()
    He = O.delay_response_exact(m.to(torch.int64), nfft, O.gamma_of(30.0, nfft))
    cc("H32", H32, He, 2e-07)  # float32 rounding only; the reference's own f32 run is 1e-3 off
    cc("H32", H32, O.delay_response(m.double(), nfft, O.gamma_of(30.0, nfft)), 2e-07)


# ----------------------------------------------------------------------------- composed systems
def _config2_model(dsp, system, meta, a, dev, dt):
    from collections import OrderedDict
    nfft, db, N = meta["nfft"], meta["alias_decay_db"], meta["N"]
    kw = dict(nfft=nfft, alias_decay_db=db, device=dev, dtype=dt)
    mat = dsp.Matrix(size=(N, N), matrix_type="random", requires_grad=True, **kw)
    geq = dsp.GEQ(size=(N, N), requires_grad=True, **kw)
    mat.assign_value(_dev(a["W"], dev, dt))
    geq.assign_value(_dev(a["geq_param"], dev, dt))
    core = system.Series(OrderedDict({"mix": mat, "eq": geq}))
    return system.Shell(core, dsp.FFT(nfft, dtype=dt), dsp.iFFT(nfft, dtype=dt)), mat, geq


@pytest.mark.parametrize("name", golden_names("config2"))
def test_config2_golden(gpu, dt, plan, name):
    from flamo_amd.processor import dsp, system
    from oracle import hotpath as O
    meta, a = load_golden(name)
    if dt == torch.float32:   # expected values: float64 oracle on the float32-rounded parameters / input
        leaves = [_f32_exact(a[k]).requires_grad_(True) for k in ("x", "W", "geq_param")]
        yo = O.config2_forward(leaves[0], leaves[1], leaves[2], meta["nfft"], meta["alias_decay_db"])
        go = torch.autograd.grad((yo ** 2).mean(), leaves)
        a = dict(x=leaves[0].detach(), W=leaves[1].detach(), geq_param=leaves[2].detach(), y=yo.detach(),
                 gx=go[0], gW=go[1], gG=go[2])
    model, mat, geq = _config2_model(dsp, system, meta, a, gpu, dt)
    assert list(model.state_dict().keys()) == meta["state_keys"]
    x = _dev(a["x"], gpu, dt).requires_grad_(True)
    y = model(x)
    tol = max(TOL[dt], 2e-6)          # float32 GEQ sections inside the reference (host libm ulp)
    tag = f"config2_golden/{name}/{str(dt)[6:]}/{plan}"
    check_close(tag + "/y", y.detach().cpu(), a["y"], tol)
    gx, gW, gG = torch.autograd.grad((y ** 2).mean(), [x, mat.param, geq.param])
    check_close(tag + "/gx", gx.cpu(), a["gx"], tol)
    check_close(tag + "/gW", gW.cpu(), a["gW"], tol)
    check_close(tag + "/gG", gG.cpu(), a["gG"], 1e-3)   # reference gradient passes through float32 buffers; recorded bound on top


def _fdn_model(dsp, system, meta, a, dev, dt):
    from collections import OrderedDict
    N, nfft, db = meta["N"], meta["nfft"], meta["alias_decay_db"]
    kw = dict(nfft=nfft, alias_decay_db=db, device=dev, dtype=dt)
    ig = dsp.Gain(size=(N, 1), requires_grad=True, **kw)
    og = dsp.Gain(size=(1, N), requires_grad=True, **kw)
    dl = dsp.parallelDelay(size=(N,), max_len=max(meta["delays"]), isint=True, **kw)
    mix = dsp.Matrix(size=(N, N), matrix_type="orthogonal", requires_grad=True, **kw)
    ig.assign_value(_dev(a["in_gain"], dev, dt))
    og.assign_value(_dev(a["out_gain"], dev, dt))
    dl.assign_value(_dev(a["delays_s"], dev, dt))
    mix.assign_value(_dev(a["U_param"], dev, dt))
    att = None
    if meta["attn"]:
        att = dsp.parallelGEQ(size=(N,), requires_grad=True, **kw)
        att.map = lambda x: 20 * torch.log10(torch.sigmoid(x))
        att.assign_value(_dev(a["attn_param"], dev, dt))
        fb = system.Series(OrderedDict({"mixing_matrix": mix, "attenuation": att}))
    else:
        fb = mix
    rec = system.Recursion(fF=dl, fB=fb)
    core = system.Series(OrderedDict({"input_gain": ig, "feedback_loop": rec, "output_gain": og}))
    model = system.Shell(core, dsp.FFT(nfft, dtype=dt), dsp.iFFTAntiAlias(nfft, alias_decay_db=db, device=dev, dtype=dt))
    return model, dict(ig=ig, og=og, mix=mix, att=att, rec=rec)


@pytest.mark.parametrize("name", ["fdn4", "fdn6", "fdn6_db0", "fdn16"])
def test_fdn_golden(gpu, dt, name):
    from flamo_amd.processor import dsp, system
    from oracle import hotpath as O
    meta, a = load_golden(name)
    # (the undamped loop, alias_decay_db = 0, runs in float32 too: measured 3e-7 against float64 where the reference's own
    # float32 run is 1.5e-4 off -- tests/test_round2_parity.py prints both)
    amap = lambda p_: 20 * torch.log10(torch.sigmoid(p_))  # noqa: E731
    full = dt == torch.float64
    if not full:   # expected values: float64 oracle on the float32-rounded parameters / input
        keys = ["x", "in_gain", "out_gain", "U_param"] + (["attn_param"] if meta["attn"] else [])
        lv = {k: _f32_exact(a[k]).requires_grad_(True) for k in keys}
        c = _f32_exact(a["c"])
        yo = O.fdn_forward(lv["x"], lv["in_gain"], lv["out_gain"], lv["U_param"], a["delays_s"], meta["nfft"],
                           meta["alias_decay_db"], attn_param=lv.get("attn_param"), attn_map=amap)
        go = torch.autograd.grad(torch.sum(yo * c), [lv[k] for k in keys])
        ref = {k: lv[k].detach() for k in keys}
        ref.update(y=yo.detach(), c=c, delays_s=a["delays_s"], gx=go[0], g_in_gain=go[1], g_out_gain=go[2],
                   g_U_param=go[3])
        if meta["attn"]:
            ref["g_attn_param"] = go[4]
        a = ref
    truth = None
    if meta["attn"]:
        # the float64 backward of the function the reference evaluates (same float32 section VALUES, no float32 graph behind
        # them): the reference's own gain gradient is 1e-5 .. 2e-4 from it, the yardstick of "g_attn_param" below
        lv = {k: a[k].detach().clone().requires_grad_(True) for k in ("x", "in_gain", "out_gain", "U_param", "attn_param")}
        yt = O.fdn_forward(lv["x"], lv["in_gain"], lv["out_gain"], lv["U_param"], a["delays_s"], meta["nfft"],
                           meta["alias_decay_db"], attn_param=lv["attn_param"], attn_map=amap, geq_exact=True)
        (truth,) = torch.autograd.grad(torch.sum(yt * a["c"]), [lv["attn_param"]])
    model, p = _fdn_model(dsp, system, meta, a, gpu, dt)
    assert list(model.state_dict().keys()) == meta["state_keys"]
    tol = max(TOL[dt], 2e-6 if meta["attn"] else 1e-8)   # float32 GEQ sections when attenuation is present
    x = _dev(a["x"], gpu, dt).requires_grad_(True)
    y = model(x)
    cc("y", y.detach().cpu(), a['y'], tol)
    plist = [p["ig"].param, p["og"].param, p["mix"].param] + ([p["att"].param] if meta["attn"] else [])
    g = torch.autograd.grad(torch.sum(y * _dev(a["c"], gpu, dt)), [x] + plist)
    keys = ["gx", "g_in_gain", "g_out_gain", "g_U_param"] + (["g_attn_param"] if meta["attn"] else [])
    for got, key in zip(g, keys):
        check_close(f"fdn_golden/{name}/{str(dt)[6:]}/{key}", got.cpu(), a[key], 1e-3 if key == "g_attn_param" else 5 * tol)
        if key == "g_attn_param":
            # (recorded on MI355X: 8e-14 .. 3e-12 in float64, 3e-7 .. 2e-6 in float32 -- the 1e-4 above is the reference's own noise)
            check_closer(f"fdn_golden/{name}/{str(dt)[6:]}/g_attn_param_vs_float64_backward", got.cpu(), a[key], truth,
                         1e-10 if full else 1e-5)
    if not full:
        return
    core = model.get_core()
    with torch.no_grad():
        cc("core__dev_a_Xf_gpu_dt", core(_dev(a['Xf'], gpu, dt)).cpu(), a['Yf'], tol)
        if "Xm" in a:
            cc("p_rec__dev_a_Xm_gpu_dt", p['rec'](_dev(a['Xm'], gpu, dt)).cpu(), a['Ym'], tol)
        ir = model.get_time_response(identity=False)
        fr = model.get_freq_response(identity=False)
        assert ir.shape == a["ir"].shape and fr.shape == a["fr"].shape
        cc("ir", ir.cpu(), a['ir'], tol)
        cc("fr", fr.cpu(), a['fr'], tol)
        if not meta["attn"]:   # analytic probe identity of examples/e10_probe.py (assert max diff < 5e-3 there)
            ones = torch.ones(1, meta["nfft"] // 2 + 1, 1, dtype=CD[dt], device=gpu)
            Hc = core(ones).reshape(-1).cpu()
            cc("Hc_a_probe_bins_long", Hc[a['probe_bins'].long()], a['probe'].reshape(-1), tol)


def test_identity_responses_golden(gpu, dt):
    from collections import OrderedDict
    from flamo_amd.processor import dsp, system
    meta, a = load_golden("rec3_identity")
    N, nfft, db = meta["N"], meta["nfft"], meta["alias_decay_db"]
    kw = dict(nfft=nfft, alias_decay_db=db, device=gpu, dtype=dt)
    dl = dsp.parallelDelay(size=(N,), max_len=60, isint=True, **kw)
    dl.assign_value(dl.sample2s(torch.tensor(meta["delays"], dtype=dt, device=gpu)))
    mix = dsp.Matrix(size=(N, N), matrix_type="orthogonal", **kw)
    mix.assign_value(_dev(a["U_param"], gpu, dt))
    att = dsp.parallelGain(size=(N,), **kw)
    att.assign_value(_dev(a["att"], gpu, dt))
    model = system.Shell(core=system.Recursion(fF=dl, fB=system.Series(OrderedDict({"mix": mix, "att": att}))))
    tol = max(TOL[dt], 1e-9)
    cc("model_get_time_response_identity_True", model.get_time_response(identity=True).cpu(), a['ir'], tol)
    cc("model_get_freq_response_identity_True", model.get_freq_response(identity=True).cpu(), a['fr'], tol)
    cc("model_get_time_response_identity_False", model.get_time_response(identity=False).cpu(), a['ir_vec'], tol)


def test_fdn16_full_size_against_oracle(gpu):
    """BASELINE config 3: 16-channel FDN at nfft=192000, float64 and float32 vs the float64 oracle."""
    from flamo_amd.processor import dsp, system
    from oracle import hotpath as O
    torch.manual_seed(130709)
    N, nfft, db = 16, 192000, 30.0
    delays = [503, 593, 701, 811, 919, 1031, 1151, 1259, 1381, 1493, 1613, 1741, 1873, 2003, 2381, 2713]
    meta = dict(N=N, nfft=nfft, alias_decay_db=db, delays=delays, attn=True)
    a = dict(in_gain=torch.randn(N, 1), out_gain=torch.randn(1, N), U_param=torch.randn(N, N),
             attn_param=torch.randn(12, N) * 0.3 + 2)
    a = {k: v.double() for k, v in a.items()}          # float32-representable values, held in float64
    a["delays_s"] = torch.tensor(delays, dtype=torch.float64) / 48000 * 100
    x = torch.zeros(1, nfft, 1, dtype=torch.float64)
    x[:, 0] = 1
    amap = lambda p: 20 * torch.log10(torch.sigmoid(p))
    yref = O.fdn_forward(x, a["in_gain"], a["out_gain"], a["U_param"], a["delays_s"], nfft, db,
                         attn_param=a["attn_param"], attn_map=amap)
    for dt_, tol in ((torch.float64, 2e-6), (torch.float32, 1e-5)):
        model, _ = _fdn_model(dsp, system, meta, a, gpu, dt_)
        with torch.no_grad():
            y = model(x.to(gpu, dt_))
        cc("y", y.cpu(), yref, tol)


def test_solve_properties(gpu):
    """A x = b residual and adjoint consistency for every supported N (padding paths included)."""
    from flamo_amd import ops
    torch.manual_seed(0)
    M = 301
    for N in (1, 2, 3, 4, 6, 8, 13, 16, 24, 32):
        P = (torch.randn(M, N, N, dtype=torch.complex128, device=gpu) * (0.4 / N ** 0.5))
        R = torch.randn(3, M, N, 2, dtype=torch.complex128, device=gpu)
        X = ops.solve(P, R, one_minus=True)
        A = torch.eye(N, dtype=torch.complex128, device=gpu) - P
        res = torch.einsum("fmn,bfnk->bfmk", A, X) - R
        assert (res.abs().max() / R.abs().max()).item() < 1e-12, N
        Xd = ops.solve(A, R, one_minus=False)
        cc("Xd", Xd, X, 1e-12)
        X32 = ops.solve(P.to(torch.complex64), R.to(torch.complex64), one_minus=True)
        cc("X32_to_torch_complex128", X32.to(torch.complex128), X, 1e-05)
    # a matrix that needs row exchanges (zero leading pivot)
    Pm = torch.tensor([[0.0, 1.0], [1.0, 0.0]], dtype=torch.complex128, device=gpu).expand(5, 2, 2).contiguous()
    R = torch.randn(1, 5, 2, dtype=torch.complex128, device=gpu)
    X = ops.solve(Pm, R, one_minus=False)
    cc("X_0", X[..., 0], R[..., 1], 1e-14)
    cc("X_1", X[..., 1], R[..., 0], 1e-14)
    # above 64 channels the matrix is factored per bin in LDS (round 3), up to what 160 KB holds: 138 in float32
    R65 = torch.randn(1, 4, 65, dtype=torch.complex64, device=gpu)
    cc("ops_solve_torch_zeros_4_65_65_dtype_torc", ops.solve(torch.zeros(4, 65, 65, dtype=torch.complex64, device=gpu), R65), R65, 1e-06)
    # ... and above that in a global-memory workspace (fl_solve_ws_*, round 5), to 1024 channels
    R139 = torch.randn(1, 4, 139, dtype=torch.complex64, device=gpu)
    cc("ops_solve_torch_zeros_4_139_139_workspace", ops.solve(torch.zeros(4, 139, 139, dtype=torch.complex64, device=gpu), R139), R139, 1e-06)
    with pytest.raises(RuntimeError):
        ops.solve(torch.zeros(2, 1025, 1025, dtype=torch.complex64, device=gpu),
                  torch.zeros(1, 2, 1025, dtype=torch.complex64, device=gpu))


def test_config2_full_size(gpu):
    """BASELINE config 2 (the metric's configuration): Series(Matrix 8x8, GEQ 8x8), nfft=96000, B=32,
    float32 on the GPU against the float64 oracle; forward and all gradients."""
    from flamo_amd.processor import dsp, system
    from oracle import hotpath as O
    torch.manual_seed(130709)
    N, nfft, B = 8, 96000, 8          # B=8 keeps the CPU oracle to a few seconds
    a = dict(W=torch.randn(N, N).double(),     # float32-representable values, held in float64
             geq_param=torch.empty(12, N, N).uniform_(10 ** (-6 / 20), 10 ** (6 / 20)).double())
    x = torch.randn(B, nfft, N).double()
    leaves = [t.clone().requires_grad_(True) for t in (x, a["W"], a["geq_param"])]
    yref = O.config2_forward(leaves[0], leaves[1], leaves[2], nfft)
    gref = torch.autograd.grad((yref ** 2).mean(), leaves)
    meta = dict(nfft=nfft, alias_decay_db=0.0, N=N)
    model, mat, geq = _config2_model(dsp, system, meta, a, gpu, torch.float32)
    xg = x.to(gpu, torch.float32).requires_grad_(True)
    y = model(xg)
    check_close("config2_full/y", y.detach().cpu(), yref.detach(), 1e-5)
    g = torch.autograd.grad((y ** 2).mean(), [xg, mat.param, geq.param])
    check_close("config2_full/gx", g[0].cpu(), gref[0], 1e-5)
    check_close("config2_full/gW", g[1].cpu(), gref[1], 1e-5)
    check_close("config2_full/gG", g[2].cpu(), gref[2], 1e-4)


def _config5_model(dsp, system, N, nfft, db, a, dev, dt, max_len=2000):
    """BASELINE config 5 (active-acoustics structure): anti-aliased transforms around
    Series(GEQ((N,N)), Recursion(fF = Series(Delay((N,N), isint), parallelGain(N)), fB = Matrix orthogonal))."""
    kw = dict(nfft=nfft, alias_decay_db=db, device=dev, dtype=dt)
    geq = dsp.GEQ(size=(N, N), **kw)
    dly = dsp.Delay(size=(N, N), max_len=max_len, isint=True, **kw)
    gain = dsp.parallelGain(size=(N,), **kw)
    mix = dsp.Matrix(size=(N, N), matrix_type="orthogonal", **kw)
    geq.assign_value(a["geq"].to(dev, dt))
    dly.assign_value(a["delay_s"].to(dev, dt))
    gain.assign_value(a["gain"].to(dev, dt))
    mix.assign_value(a["U"].to(dev, dt))
    core = system.Series(OrderedDict(eq=geq, loop=system.Recursion(fF=system.Series(OrderedDict(d=dly, g=gain)), fB=mix)))
    return system.Shell(core, dsp.FFTAntiAlias(nfft, alias_decay_db=db, dtype=dt), dsp.iFFTAntiAlias(nfft, alias_decay_db=db, dtype=dt))


def _config5_params(N, max_len=2000):
    g = torch.Generator().manual_seed(130709)
    m = torch.randint(1, max_len, (N, N), generator=g).double()
    return dict(geq=(torch.rand(12, N, N, generator=g) * (10 ** (6 / 20) - 10 ** (-6 / 20)) + 10 ** (-6 / 20)).float().double(),
                delay_s=(m / 48000 * 100).float().double(),            # seconds * unit, as Delay stores them
                gain=(torch.rand(N, generator=g) * 0.5 / N ** 0.5 + 0.01).float().double(),
                U=torch.randn(N, N, generator=g).float().double())


def test_config5_chain_against_oracle(gpu):
    """Config 5's structure (32x32 GEQ -> Recursion(Delay * parallelGain, orthogonal Matrix), anti-aliasing
    on) against the float64 oracle at a length the oracle finishes in seconds."""
    from flamo_amd.processor import dsp, system
    from oracle import hotpath as O
    N, nfft, db = 32, 9600, 30.0
    a = _config5_params(N)
    torch.manual_seed(5)
    x = torch.randn(1, nfft, N, dtype=torch.float64) * 0.1
    x[:, 0] += 1
    gamma = O.gamma_of(db, nfft, torch.float64)
    X = O.rfft(x, nfft, alias_decay_db=db)
    X = O.mimo_full(O.geq_response(a["geq"], nfft, gamma), X)
    m = O.delay_samples(a["delay_s"], 48000, 100, True)
    F = O.to_complex(a["gain"]).view(1, N, 1) * O.delay_response(m, nfft, gamma)
    Bk = O.to_complex(O.orthogonal(a["U"])).unsqueeze(0).expand(F.shape[0], N, N)
    yref = O.irfft(O.recursion(F, Bk, X), nfft, alias_decay_db=db)
    for dt_, tol in ((torch.float64, 1e-9), (torch.float32, 1e-5)):
        model = _config5_model(dsp, system, N, nfft, db, a, gpu, dt_)
        with torch.no_grad():
            y = model(x.to(gpu, dt_))
        cc("y", y.cpu(), yref, tol)


def test_config5_full_size_runs_and_is_linear(gpu):
    """Config 5 at its BASELINE size (32x32, nfft=384000, anti-aliasing 30 dB), float32: finite output,
    linearity in the input and agreement with the float64 run of the same kernels."""
    from flamo_amd.processor import dsp, system
    N, nfft, db = 32, 384000, 30.0
    a = _config5_params(N)
    torch.manual_seed(6)
    x1 = torch.zeros(1, nfft, N, dtype=torch.float64)
    x1[:, 0] = 1
    x2 = torch.randn(1, nfft, N, dtype=torch.float64) * 0.01
    m32 = _config5_model(dsp, system, N, nfft, db, a, gpu, torch.float32)
    with torch.no_grad():
        y1 = m32(x1.to(gpu, torch.float32))
        y2 = m32(x2.to(gpu, torch.float32))
        y12 = m32((x1 + 2 * x2).to(gpu, torch.float32))
        assert torch.isfinite(y1).all() and y1.shape == (1, nfft, N)
        cc("y12", y12, y1 + 2 * y2, 2e-05)
        m64 = _config5_model(dsp, system, N, nfft, db, a, gpu, torch.float64)
        y64 = m64(x1.to(gpu))
    cc("y1", y1.double(), y64, 1e-05)


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("name", golden_names("parallel_"))
def test_parallel_golden(gpu, dt, name):
    """system.Parallel (two branches summed / concatenated) against the reference's outputs and gradients."""
    from flamo_amd.processor import dsp, system
    meta, a = load_golden(name)
    rd = torch.float64 if dt == "f64" else torch.float32
    cd = torch.complex128 if dt == "f64" else torch.complex64
    tol = 1e-10 if dt == "f64" else 1e-5
    kw = dict(nfft=meta["nfft"], alias_decay_db=meta["alias_decay_db"], device=gpu, dtype=rd, requires_grad=True)
    g = dsp.Gain(size=(3, 2), **kw)
    pg = dsp.parallelGain(size=(3,), **kw)
    fir = dsp.Filter(size=(5, 3, 2), **kw)
    g.assign_value(a["g"].to(gpu, rd))
    pg.assign_value(a["pg"].to(gpu, rd))
    fir.assign_value(a["fir"].to(gpu, rd))
    par = system.Parallel(brA=OrderedDict(g=g, pg=pg), brB=fir, sum_output=meta["sum_output"])
    assert (par.input_channels, par.output_channels) == (meta["input_channels"], meta["output_channels"])
    X = a["X"].to(gpu, cd).requires_grad_(True)
    Y = par(X)
    cc("Y", Y.detach().cpu(), a['Y'], tol)
    L = torch.sum(torch.real(Y * torch.conj(a["C"].to(gpu, cd))))
    gX, gg, gpg, gfir = torch.autograd.grad(L, [X, g.param, pg.param, fir.param])
    for got, key in ((gX, "gX"), (gg, "gg"), (gpg, "gpg"), (gfir, "gfir")):
        cc("got", got.cpu(), a[key], tol * 10)


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_accurate_geq_kernels_tight(gpu, dt):
    """AccurateGEQ behind its host-side design: the cascade evaluated by the HIP kernel against the oracle's
    tail on the very sections this run designed (no L-BFGS noise in the comparison)."""
    from flamo_amd.processor import dsp
    from oracle import hotpath as O
    rd = torch.float64 if dt == "f64" else torch.float32
    meta, a = load_golden("accgeq_db30")
    mod = dsp.AccurateGEQ(size=(2, 2), nfft=meta["nfft"], alias_decay_db=meta["alias_decay_db"], device=gpu, dtype=rd)
    mod.assign_value(a["param"].to(gpu, rd))
    b, a_ = mod._sos_coeffs(mod.map(mod.param.double()))
    assert b.shape == (3, mod.n_gains + 1, 2, 2)
    gamma = O.gamma_of(meta["alias_decay_db"], meta["nfft"], torch.float64)
    Href = O.sos_response(b.cpu().double(), a_.cpu().double(), meta["nfft"], gamma)
    H = mod.freq_response(mod.param)
    cc("H", H.cpu(), Href, 1e-10 if dt == 'f64' else 1e-05)
    # the design is cached per parameter value: a second call does not refit
    key = mod._design_cache[0]
    mod.freq_response(mod.param)
    assert mod._design_cache[0] is key


# ----------------------------------------------------------------------------- config 4: colorless FDN training
@pytest.mark.parametrize("name", ["colorless6", "colorless16"])
def test_colorless_training_golden(gpu, dt, name):
    """BASELINE configs[3] in miniature: the Adam trajectory of examples/e8_colorless_fdn.py (|H| output layer,
    mse + 0.2 sparsity) recorded from the reference -- first estimate, first gradients, every step's losses, final
    parameters."""
    from tools import train_colorless_fdn as T
    meta, a = load_golden(name)
    model = T.build(gpu, dt, meta["N"], meta["nfft"], meta["alias_decay_db"], meta["delays"])
    assert list(model.state_dict().keys()) == meta["state_keys"]
    core = model.get_core()
    ig, og, mix = core.input_gain, core.output_gain, core.feedback_loop.feedback
    ig.assign_value(_dev(a["in_gain0"], gpu, dt))
    og.assign_value(_dev(a["out_gain0"], gpu, dt))
    mix.assign_value(_dev(a["U_param0"], gpu, dt))
    x, tgt = _dev(a["x"], gpu, dt), _dev(a["target"], gpu, dt)
    tol = 1e-9 if dt == torch.float64 else 2e-5
    est = model(x)
    assert est.shape == a['est0'].shape
    cc("est", est.detach().cpu(), a['est0'], tol)
    (T.mse_criterion(est, tgt) + 0.2 * T.sparsity_criterion(model)).backward()
    for p_, key in ((ig.param, "g_in_gain0"), (og.param, "g_out_gain0"), (mix.param, "g_U_param0")):
        cc("p__grad", p_.grad.cpu(), a[key], 10 * tol)
    log = T.train(model, x, tgt, meta["steps"], meta["lr"], log=[])
    log = torch.stack(log).double().cpu()
    cc("log", log, a['losses'], 10 * tol)
    # Adam's first steps are lr * sign(g): parameters whose gradient is ~0 amplify rounding, so the float32 run is
    # compared on the trajectory and on the parameters at a looser bound
    ptol = 1e-8 if dt == torch.float64 else 2e-3
    for p_, key in ((ig.param, "in_gain"), (og.param, "out_gain"), (mix.param, "U_param")):
        cc("p", p_.detach().cpu(), a[key], ptol)


def test_colorless_training_bin_sharded_two_ranks(gpu, tmp_path):
    """Two ranks sharing the GPU (gloo transport, staged through the host; RCCL refuses two ranks on one device):
    bin-sharded training must retrace the unsharded trajectory -- losses and final parameters."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "train_colorless_fdn.py")
    common = ["--N", "6", "--nfft", "4800", "--batch", "2", "--steps", "4", "--warmup", "0", "--lr", "1e-2",
              "--dtype", "float64"]
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    subprocess.run([sys.executable, tool, *common, "--dump", one], check=True, timeout=600, cwd=root)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), tool, *common, "--gpus", "2",
                    "--backend", "gloo", "--share-gpu", "--dump", two], check=True, timeout=900, cwd=root)
    r1, r2 = torch.load(one), torch.load(two)
    cc("torch_tensor_r2_losses_dtype_torch_float", torch.tensor(r2['losses'], dtype=torch.float64), torch.tensor(r1['losses'], dtype=torch.float64), 1e-10)
    assert r1["losses"][0][2] > r1["losses"][-1][2]            # it trains
    for k, v in r1["state"].items():
        cc("r2_state_k", r2['state'][k], v, 1e-09)


# ----------------------------------------------------------------------------- config 1: e7_biquad training
def test_e7_biquad_training_golden(gpu, dt):
    """BASELINE configs[0] at its own size: Shell(FFT(96000) -> Biquad((2,1), 2 sections, highpass, alias 30 dB) -> |.|),
    impulse input, nn.MSELoss, Adam -- first estimate and gradient, every step's loss, final parameters against the
    trajectory recorded from the reference (examples/e7_biquad.py)."""
    from flamo_amd.processor import dsp, system
    meta, a = load_golden("e7_biquad")
    nfft, dec = meta["nfft"], meta["decimation"]
    target = _dev(a["target"], gpu, dt)     # stored whole (the reference builds it through a float32 FFT of `a`)
    filt = dsp.Biquad(size=(2, 1), n_sections=meta["n_sections"], filter_type="highpass", nfft=nfft, fs=meta["fs"],
                      requires_grad=True, alias_decay_db=meta["alias_decay_db"], device=gpu, dtype=dt)
    model = system.Shell(core=filt, input_layer=dsp.FFT(nfft, dtype=dt),
                         output_layer=dsp.Transform(lambda z: torch.abs(z), device=gpu, dtype=dt))
    assert list(model.state_dict().keys()) == meta["state_keys"]
    filt.assign_value(_dev(a["param0"], gpu, dt))
    x = torch.zeros(1, nfft, 1, device=gpu, dtype=dt)
    x[:, 0, :] = 1
    tol = 1e-9 if dt == torch.float64 else 2e-5
    with torch.no_grad():
        cc("model_get_freq_response_dec", model.get_freq_response()[:, ::dec].cpu(), a['fr0_dec'], tol)
    crit = torch.nn.MSELoss()
    opt = torch.optim.Adam(model.parameters(), lr=meta["lr"])
    losses = []
    for it in range(meta["steps"]):
        opt.zero_grad()
        est = model(x)
        loss = crit(est, target)
        loss.backward()
        if it == 0:
            cc("est_dec", est.detach()[:, ::dec].cpu(), a['est0_dec'], tol)
            cc("filt_param_grad", filt.param.grad.cpu(), a['g_param0'], 1e-07 if dt == torch.float64 else 0.002)
        opt.step()
        losses.append(loss.detach())
    cc("torch_stack_losses", torch.stack(losses).double().cpu(), a['losses'], 10 * tol)
    cc("filt_param", filt.param.detach().cpu(), a['param'], 1e-08 if dt == torch.float64 else 0.001)


def test_config5_chain_bin_sharded_two_ranks(gpu, tmp_path):
    """BASELINE configs[4]'s structure (32 x 32: MFMA products, composed loop matrix, N = 32 solve) with the bins
    sharded over two ranks sharing the GPU (gloo transport staged through the host): output of the inverse transform
    behind the all-gather and every parameter gradient equal the unsharded run."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "run_sharded_chain.py")
    common = ["--N", "32", "--nfft", "3840", "--steps", "1", "--warmup", "0", "--dtype", "float64"]
    one, two = str(tmp_path / "one.pt"), str(tmp_path / "two.pt")
    subprocess.run([sys.executable, tool, *common, "--dump", one], check=True, timeout=600, cwd=root)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                    "--master-addr", "127.0.0.1", "--master-port", str(port), tool, *common, "--gpus", "2",
                    "--backend", "gloo", "--share-gpu", "--dump", two], check=True, timeout=900, cwd=root)
    r1, r2 = torch.load(one), torch.load(two)
    cc("r2_y", r2['y'], r1['y'], 1e-11)
    for g2, g1 in zip(r2["grads"], r1["grads"]):
        cc("g2", g2, g1, 1e-09)


def test_bench_contract_line(gpu):
    """bench.py prints exactly one JSON line on stdout with the fields the driver reads, a roofline object for the
    per-bin product and (without --no-cpu-baseline) a cpu_baseline object."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--full", "--no-cpu-baseline"], check=True, timeout=600, cwd=root, capture_output=True, text=True).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "products/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"]
    su = d["setup_before_warmup"]       # the sustained-state set-up is part of the line: how many repeats, first and last block
    assert 100 <= su["steps"] <= 400 and su["steps"] % 20 == 0 and su["ms_first_block"] > 0 and su["ms_last_block"] > 0
    M = 96000 // 2 + 1
    assert abs(d["value"] - 2 * 32 * M * 8 * 8 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and 0.2 < r["frac"] < 1.0
    assert abs(r["achieved"] - r["algorithmic_bytes"] / (r["launch_ms"] * 1e-3) / 1e9) / r["achieved"] < 1e-9
    assert r["algorithmic_bytes"] == 3 * 8 * 32 * M * 8 + 8 * M * 64      # scratch in, spectrum + scratch out, H
    assert r["traffic"] is None or r["traffic"] >= 0.9 * r["algorithmic_bytes"]
    sr = d["step_roofline"]
    assert abs(sr["unfused_bytes_per_step"] - 1.057e9) < 2e6 and 0 < sr["frac_of_unfused_floor"] < 1
    assert sr["pipeline_bytes_per_step"] > sr["unfused_bytes_per_step"]
    # (the step's streaming launches: the column pass with the response's workgroups, the row kernel, the inverse column pass
    # that also leaves the gradient's column pass, the gradient's row kernel)
    for k in ("spec_cols_fwd+response", "spec_cols_inv+grad_cols", "spec_mid_walk[8->8,spec]", "spec_gradh_walk"):
        assert 0.1 < d["kernels"][k]["frac_hbm_peak"] < 1.0, k
    assert "spec_mid_walk" in r["kernel"] and d["params"].startswith("tests/golden/bench_params.npz")
    assert d["input_grad"]["ms_per_step"] > d["ms_per_step"]
    for k in ("impulse", "alias30_wgn", "alias30_impulse"):
        assert d["variants"][k]["ms_per_step"] > 0, k
    sec = d["secondary"]
    for k in ("config3_fdn16_batch1", "config3_fdn16_batch8", "config4_colorless_training", "config5_chain_32x32"):
        assert sec[k]["ms_per_step"] > 0 and sec[k]["bin_solves_per_s"] > 0, k
    assert 0 < sec["config3_fdn16_batch1"]["solve"]["frac_fp32_vector_peak"] < 1
    assert d["device"]["hbm_copy_probe_GBs"] > 1000


def test_bench_plain_line_and_dumped_outputs(gpu, tmp_path):
    """bench.py without --full: the headline line alone (no side legs), and --dump-outputs writes the last timed step's loss
    and parameter gradients -- the same values an eager step of the same workload on the same inputs computes."""
    import json
    import os
    import subprocess
    import sys

    import numpy as np
    from conftest import relerr
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2",
                          "--dump-outputs", str(tmp_path)], check=True, timeout=600, cwd=root, capture_output=True, text=True).stdout
    lines = [ln for ln in out.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 4 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "products/s" and d["dtype"] == "f32"
    M = 96000 // 2 + 1
    assert abs(d["value"] - 2 * 32 * M * 8 * 8 / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-9
    for k in ("roofline", "kernels", "step_roofline", "ms_per_step_steady", "input_grad", "secondary", "device", "cpu_baseline"):
        assert k not in d, k
    dumped = {f[:-4]: np.load(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)}
    assert sorted(dumped) == ["grad_eq", "grad_mix", "loss"]
    assert all(a.dtype == np.float32 for a in dumped.values())
    sys.path.insert(0, root)
    import bench
    from flamo_amd import ops
    torch.manual_seed(130709)
    model, params = bench.build_model(gpu, torch.float32)
    torch.manual_seed(130709 + 1)
    x = torch.randn(bench.BATCH, bench.NFFT, bench.NCH, device=gpu)
    loss = ops.mean_square(model(x))
    loss.backward()
    assert relerr(torch.from_numpy(dumped["loss"]), loss.detach().cpu()) < 1e-5
    for name, p in zip(("grad_mix", "grad_eq"), params):
        assert dumped[name].shape == tuple(p.shape)
        assert relerr(torch.from_numpy(dumped[name]), p.grad.cpu()) < 1e-5, name
