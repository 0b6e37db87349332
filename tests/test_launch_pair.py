"""The deferred Matrix-then-cascade response launch (ops.paired_launch, csrc/fusedfwd.hip) against float64.

Between fl_launch_pair_begin and fl_launch_pair_flush the response kernel (fl_geq_response_rc_c64 / fl_sos_response_rc_c64) is
only RECORDED; the input's float32 forward column pass issues it later, in the same grid, or any other library call flushes it
first.  What can go wrong there is invisible to a paired-against-unpaired comparison: a module behind the pair reading the
response before it is written, buffers of the record freed (no_grad / inference_mode) and handed to the next allocation before
the kernel runs, a record silently dropped.  So every result here is compared with a float64 oracle built from oracle/hotpath.py
(the reference's own operations) on the float32-rounded parameters and input.
Tolerance: relative l2 error 1e-5 for float32 kernels (BASELINE.json north_star); 1e-4 for the equaliser-gain gradients (against
the float64 backward of the same function, geq_sos(exact=True)) and for an orthogonal matrix's parameter gradient (the
skew-symmetric part of dL/dW, a small projection of it: the float32 error of dL/dW is relatively larger there, 2e-6 to 1e-5
measured) -- the recorded achieved errors (tests/golden/achieved_errors.json) hold every check to 5x what the kernels reach."""
from collections import OrderedDict

import pytest
import torch

from conftest import cc

TOL = 1e-5
TOL_GAIN = 1e-4
NFFT, BATCH = 96000, 3
FS = 48000
NAN64 = complex(float("nan"), float("nan"))


# ----------------------------------------------------------------------------- float64 oracle
def _cascade(b, a, gamma):
    """prod over sections of O.sos_response, one section at a time (the (M, sections, N, N) spectra of a whole cascade are
    gigabytes at 16 channels): (M, No, Nmid) complex128"""
    from oracle import hotpath as O
    H = None
    for s in range(b.shape[1]):
        h = O.sos_response(b[:, s:s + 1], a[:, s:s + 1], NFFT, gamma)
        H = h if H is None else H * h
    return H


def _geq_sections(p, exact=True):
    from oracle import hotpath as O
    cf, sc = O.eq_freqs(1)
    return O.geq_sos(20 * torch.log10(torch.abs(p)), cf, sc, FS, exact=exact)


def _biquad_sections(p):
    """dsp.Biquad(filter_type="bandpass") on (n_sections, 3, ...) parameters: (b, a), each (3, n_sections, ...)"""
    from oracle import hotpath as O
    m = O.biquad_map(p, "bandpass")
    hz = lambda r: r * FS / 2  # noqa: E731  (fc in units of pi rad, functional.rad2hertz)
    return O.rbj_biquad("bandpass", hz(m[:, 0]), m[:, 2], FS, fc2_hz=hz(m[:, 1]))


def _poison_rows(N, dev):
    """free two NaN-filled blocks of the size of a response's pitched rows on the current stream: the G and H the next cascade
    operator allocates are handed these, so a launch that never runs leaves NaN rather than an earlier run's correct values"""
    from flamo_amd import ops
    blocks = [torch.full((N, N, ops._pitch(NFFT // 2 + 1)), NAN64, dtype=torch.complex64, device=dev) for _ in range(2)]
    del blocks


# ----------------------------------------------------------------------------- A1: Shell(fin -> Series(Matrix, cascade[, tail]) -> fout)
# (id: channels, anti-aliasing transforms at 30 dB, matrix type, cascade, module behind the pair)
CASES = [
    (8, False, "random", "geq", None),
    (8, False, "random", "geq", "pgain32"),
    (8, False, "random", "geq", "pgain64"),
    (8, True, "orthogonal", "geq", "gain64"),
    (8, True, "random", "biquad", None),
    (8, False, "orthogonal", "geq", None),
    (8, True, "orthogonal", "biquad", "pgain64"),
    (8, False, "random", "geq", "pdelay"),
    (4, True, "orthogonal", "geq", None),
    (4, False, "random", "biquad", "pgain64"),
    (16, False, "random", "geq", None),
    (16, True, "orthogonal", "biquad", "gain64"),
]


def _case_id(c):
    N, aa, mt, casc, tail = c
    return f"{N}-{'aa30' if aa else 'fft'}-{mt[:4]}-{casc}-{tail or 'none'}"


def _model(dev, N, aa, mt, casc, tail):
    from flamo_amd.processor import dsp, system
    db = 30.0 if aa else 0.0
    kw = dict(nfft=NFFT, alias_decay_db=db, device=dev)
    mods = OrderedDict(mix=dsp.Matrix(size=(N, N), matrix_type=mt, requires_grad=True, dtype=torch.float32, **kw))
    if casc == "geq":
        mods["flt"] = dsp.GEQ(size=(N, N), requires_grad=True, dtype=torch.float32, **kw)
    else:      # raw sections WITHOUT a gradient: the float kernel, the one that records (with one: double, no pair)
        mods["flt"] = dsp.Biquad(size=(N, N), n_sections=3, filter_type="bandpass", requires_grad=False, dtype=torch.float32, **kw)
    if tail in ("pgain32", "pgain64"):
        mods["tail"] = dsp.parallelGain(size=(N,), requires_grad=True, dtype=torch.float32, **kw)
    elif tail == "gain64":
        mods["tail"] = dsp.Gain(size=(N, N), requires_grad=True, dtype=torch.float32, **kw)
    elif tail == "pdelay":
        mods["tail"] = dsp.parallelDelay(size=(N,), max_len=2000, isint=True, dtype=torch.float32, **kw)
        delays = torch.randint(1, 1999, (N,), device=dev).to(torch.float32)
        mods["tail"].assign_value(mods["tail"].sample2s(delays))
    fin = dsp.FFTAntiAlias(NFFT, alias_decay_db=db, device=dev) if aa else dsp.FFT(NFFT)
    fout = dsp.iFFTAntiAlias(NFFT, alias_decay_db=db, device=dev) if aa else dsp.iFFT(NFFT)
    shell = system.Shell(system.Series(mods), fin, fout)
    if tail in ("pgain32", "pgain64", "gain64"):
        t = mods["tail"]
        if tail.endswith("64"):      # a float64 module behind the float32 pair (Series refuses mixed dtypes at construction)
            t.double()
        with torch.no_grad():
            if tail == "gain64":
                t.param.copy_(torch.randn(N, N, dtype=torch.float64, device=dev) / N ** 0.5)
            else:
                t.param.copy_(0.5 + torch.rand(N, dtype=torch.float64, device=dev))
    return shell, mods


def _oracle(x, mods, aa, mt, casc, tail):
    """float64 y and the gradients of mean(y^2) with respect to x and every parameter that has one"""
    from oracle import hotpath as O
    db = 30.0 if aa else None
    gamma = O.gamma_of(db or 0.0, NFFT)
    xo = x.detach().cpu().double().requires_grad_(True)
    leaves = {k: m.param.detach().cpu().double().requires_grad_(True) for k, m in mods.items() if m.param.requires_grad}
    W = O.orthogonal(leaves["mix"]) if mt == "orthogonal" else leaves["mix"]
    if casc == "geq":
        H = _cascade(*_geq_sections(leaves["flt"]), gamma)
    else:
        H = _cascade(*_biquad_sections(mods["flt"].param.detach().cpu().double()), gamma)
    X = O.rfft(xo, NFFT, alias_decay_db=db)
    X = O.mimo_full(H, O.mimo_const(O.to_complex(W), X))
    if tail in ("pgain32", "pgain64"):
        X = O.mimo_const_diag(O.to_complex(leaves["tail"]), X)
    elif tail == "gain64":
        X = O.mimo_const(O.to_complex(leaves["tail"]), X)
    elif tail == "pdelay":
        m = mods["tail"].get_delays()(mods["tail"].param.detach()).cpu().double().round()
        X = O.mimo_diag(O.delay_response_exact(m, NFFT, gamma), X)
    y = O.irfft(X, NFFT, alias_decay_db=db)
    grads = torch.autograd.grad((y ** 2).mean(), [xo] + list(leaves.values()))
    return y.detach(), dict(zip(["x"] + list(leaves), grads))


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_paired_shell_matches_float64(gpu, case):
    """Output (and in grad mode the gradients of x and of every parameter) of the fused Shell against the float64 oracle in
    grad, no_grad and inference_mode, with the responses built on the side stream and on the main stream.  Every case runs
    twice: the second run must issue the grid with both roles exactly where it has the shape (no module behind the pair, 4 / 8
    channels), leave nothing recorded, and equal the two-launch form bit for bit."""
    from flamo_amd import _lib, ops
    from flamo_amd.processor import system
    N, aa, mt, casc, tail = case
    torch.manual_seed(1000 + CASES.index(case))
    shell, mods = _model(gpu, N, aa, mt, casc, tail)
    x = torch.randn(BATCH, NFFT, N, device=gpu)
    yo, go = _oracle(x, mods, aa, mt, casc, tail)
    keys = [k for k, m in mods.items() if m.param.requires_grad]
    params = [mods[k].param for k in keys]
    L = _lib.lib()
    takes = tail is None and N in (4, 8)

    def run(mode):
        if mode == "grad":
            xg = x.clone().requires_grad_(True)
            y = shell(xg)
            g = torch.autograd.grad(ops.mean_square(y), [xg] + params)
            return [y.detach()] + [t.detach() for t in g]
        with (torch.no_grad() if mode == "no_grad" else torch.inference_mode()):
            return [shell(x)]

    overlap = system.OVERLAP_RESPONSES
    try:
        for side in (True, False):
            system.OVERLAP_RESPONSES = side
            for mode in ("grad", "no_grad", "inference"):
                tag = f"{mode}/{'side' if side else 'main'}"
                run(mode)          # (the first evaluation fills the twiddle tables between the two launches)
                n0 = L.fl_debug_launch_pair_count()
                paired = run(mode)
                n1 = L.fl_debug_launch_pair_count()
                assert not L.fl_launch_pair_pending(), tag
                assert n1 - n0 == (1 if takes else 0), (tag, n1 - n0)
                ops.LAUNCH_PAIRS = False
                try:
                    plain = run(mode)
                finally:
                    ops.LAUNCH_PAIRS = True
                assert L.fl_debug_launch_pair_count() == n1, tag
                for i, (p, q) in enumerate(zip(paired, plain)):
                    assert torch.equal(p, q), (tag, i)
                cc(f"{tag}/y", paired[0].cpu(), yo, TOL)
                if mode == "grad":
                    cc(f"{tag}/gx", paired[1].cpu(), go["x"], TOL)
                    for k, g in zip(keys, paired[2:]):
                        tol = TOL_GAIN if (k == "flt" and casc == "geq") or (k == "mix" and mt == "orthogonal") else TOL
                        cc(f"{tag}/g_{k}", g.cpu(), go[k], tol)
    finally:
        system.OVERLAP_RESPONSES = overlap
        ops.LAUNCH_PAIRS = True


# ----------------------------------------------------------------------------- A2: the record's buffers under no_grad
def _geq_and_oracle(dev, N, Wr):
    from flamo_amd.processor import dsp
    torch.manual_seed(7)
    geq = dsp.GEQ(size=(N, N), nfft=NFFT, device=dev, dtype=torch.float32)
    p = geq.param.detach()
    b, a = _geq_sections(p.cpu().double(), exact=False)
    Ho = _cascade(b.double(), a.double(), torch.tensor(1.0, dtype=torch.float64)) @ Wr.cpu().to(torch.complex128)
    return geq, p, Ho


def _biquad_and_oracle(dev, N, Wr):
    """float32 sections of a bandpass cascade and the float64 response of exactly those sections times Wr"""
    from flamo_amd.processor import dsp
    torch.manual_seed(8)
    bq = dsp.Biquad(size=(N, N), n_sections=3, filter_type="bandpass", nfft=NFFT, device=dev, dtype=torch.float32)
    b, a = bq._sos_coeffs(bq.map(bq.param.detach().double()))
    b32, a32 = b.float(), a.float()
    Ho = _cascade(b32.cpu().double(), a32.cpu().double(), torch.tensor(1.0, dtype=torch.float64)) @ Wr.cpu().to(torch.complex128)
    return b32, a32, Ho


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["geq", "sos"])
def test_recorded_launch_keeps_its_buffers_under_no_grad(gpu, kind):
    """Without an autograd graph nothing but the pending record holds the response operator's temporaries (the float32 copy
    of a float64 Wr, the float64 copies of float32 sections) and outputs (G; for the equaliser the designed sections b, a).
    Blocks of exactly their sizes are allocated and filled with NaN between the record and its flush -- the caching
    allocator hands back just-freed blocks of the same size on the same stream.  The deferred kernel must still read its own
    operands (H equals the float64 oracle) and write its own outputs (every filler is still all NaN)."""
    from flamo_amd import _lib, ops
    N = 8
    M = NFFT // 2 + 1
    Wr = torch.randn(N, N, dtype=torch.float64, device=gpu)       # Wr.to(float32) is a temporary of the operator
    L = _lib.lib()
    ops.twiddles(NFFT, torch.float64, gpu)
    if kind == "geq":
        geq, p, Ho = _geq_and_oracle(gpu, N, Wr)
        spec = geq._cascade_spec(p)
        S = p.shape[0]
    else:
        b32, a32, Ho = _biquad_and_oracle(gpu, N, Wr)
        S = b32.shape[1]
    with torch.no_grad(), ops.paired_launch(True) as pair:
        _poison_rows(N, gpu)
        if kind == "geq":
            H = ops.geq_cascade_rc(spec[1], spec[2], Wr, geq._gamma_f, NFFT)
        else:
            H = ops.sos_response_rc(b32, a32, Wr, 1.0, NFFT)
        assert L.fl_launch_pair_pending() == 1
        fillers = [torch.full((3, S, N, N), float("nan"), dtype=torch.float64, device=gpu),        # b (or its float64 copy)
                   torch.full((3, S, N, N), float("nan"), dtype=torch.float64, device=gpu),        # a
                   torch.full((N, N, ops._pitch(M)), NAN64, dtype=torch.complex64, device=gpu),  # G, pitched rows
                   torch.full((N, N), float("nan"), dtype=torch.float32, device=gpu)]            # Wc = Wr.to(float32)
        pair.flush()
        assert not L.fl_launch_pair_pending()
    torch.cuda.synchronize()
    cc("H", H.cpu(), Ho, TOL)
    for i, f in enumerate(fillers):
        assert bool(torch.isnan(f).all()), f"filler {i} was written: the deferred launch used a freed buffer"


# ----------------------------------------------------------------------------- A3: protocol
def _record_direct(L, dev, N, *, geq=None, sections=None, Wr32):
    """one fl_*_response_rc_c64 call through the C ABI on live buffers only (kept in the returned tuple), natural bin order.
    -> (H view (M, N, N), buffers)"""
    from flamo_amd import ops
    M = NFFT // 2 + 1
    P = ops._pitch(M)
    Wd = ops.twiddles(NFFT, torch.float64, dev)
    G = torch.full((N, N, P), NAN64, dtype=torch.complex64, device=dev)
    H = torch.full((N, N, P), NAN64, dtype=torch.complex64, device=dev)
    if geq is not None:
        x = geq.param.detach().contiguous()
        S = x.shape[0]
        b = torch.empty((3, S, N, N), dtype=torch.float64, device=dev)
        a = torch.empty_like(b)
        consts = geq._design.device_consts(dev)
        rc = L.fl_geq_response_rc_c64(x.data_ptr(), ops._geq_in_kind(x, True, False), S, consts.data_ptr(), b.data_ptr(), a.data_ptr(),
                                       N, N, N, Wr32.data_ptr(), 1.0, Wd.data_ptr(), NFFT, 0, M, G.data_ptr(), P, H.data_ptr(), P, 1,
                                       ops._stream())
        keep = (x, consts, b, a)
    else:
        b, a = (t.double().contiguous() for t in sections)
        S = b.shape[1]
        rc = L.fl_sos_response_rc_c64(b.data_ptr(), a.data_ptr(), S, N, N, N, Wr32.data_ptr(), 1.0, Wd.data_ptr(), NFFT, 0, M,
                                       G.data_ptr(), P, H.data_ptr(), P, 1, ops._stream())
        keep = (b, a)
    assert rc == 0, L.fl_last_error()
    return H[..., :M].movedim(-1, 0), keep + (Wd, G, H, Wr32)


@pytest.mark.gpu
def test_begin_with_a_launch_recorded_keeps_it(gpu):
    """fl_launch_pair_begin while a launch is recorded refuses (FL_ERR_BAD_ARG, with a message) and the record survives: the
    flush still issues it"""
    from flamo_amd import _lib, ops
    N = 8
    Wr = torch.randn(N, N, dtype=torch.float64, device=gpu)
    geq, _, Ho = _geq_and_oracle(gpu, N, Wr)
    L = _lib.lib()
    Wr32 = Wr.float().contiguous()
    with torch.no_grad(), ops.paired_launch(True) as pair:
        H, keep = _record_direct(L, gpu, N, geq=geq, Wr32=Wr32)
        assert L.fl_launch_pair_pending() == 1
        rc = L.fl_launch_pair_begin()
        assert rc == -1, rc
        assert b"pending" in L.fl_last_error()
        assert L.fl_launch_pair_pending() == 1
        pair.flush()
        assert not L.fl_launch_pair_pending()
    torch.cuda.synchronize()
    cc("H", H.cpu(), Ho, TOL)
    del keep


@pytest.mark.gpu
def test_two_recorded_launches_in_one_region(gpu):
    """Two response launches recorded in one region: the second issues the first (one slot), the flush the second -- both
    responses equal their float64 oracles.  Once through the C ABI directly (the library's slot), once through the operators
    (the Python side flushes before the second call)."""
    from flamo_amd import _lib, ops
    N = 8
    Wr = torch.randn(N, N, dtype=torch.float64, device=gpu)
    geq, p, Ho1 = _geq_and_oracle(gpu, N, Wr)
    b32, a32, Ho2 = _biquad_and_oracle(gpu, N, Wr)
    L = _lib.lib()
    Wr32 = Wr.float().contiguous()
    with torch.no_grad(), ops.paired_launch(True) as pair:
        H1, k1 = _record_direct(L, gpu, N, geq=geq, Wr32=Wr32)
        H2, k2 = _record_direct(L, gpu, N, sections=(b32, a32), Wr32=Wr32)
        assert L.fl_launch_pair_pending() == 1
        pair.flush()
    torch.cuda.synchronize()
    cc("direct/H1", H1.cpu(), Ho1, TOL)
    cc("direct/H2", H2.cpu(), Ho2, TOL)
    del k1, k2
    spec = geq._cascade_spec(p)
    with torch.no_grad(), ops.paired_launch(True) as pair:
        _poison_rows(N, gpu)
        H1 = ops.geq_cascade_rc(spec[1], spec[2], Wr, geq._gamma_f, NFFT)
        _poison_rows(N, gpu)
        H2 = ops.sos_response_rc(b32, a32, Wr, 1.0, NFFT)
        assert L.fl_launch_pair_pending() == 1
    assert not L.fl_launch_pair_pending()
    torch.cuda.synchronize()
    cc("ops/H1", H1.cpu(), Ho1, TOL)
    cc("ops/H2", H2.cpu(), Ho2, TOL)


class _FailingFlush:
    """stand-in for the library handle: begin succeeds, a launch is recorded, the flush fails"""

    def __init__(self):
        self.flushes = 0

    def fl_launch_pair_begin(self):
        return 0

    def fl_launch_pair_pending(self):
        return 1

    def fl_launch_pair_flush(self, stream):
        self.flushes += 1
        return -3

    def fl_last_error(self):
        return b"device lost"


def test_paired_launch_exit_keeps_the_body_exception(monkeypatch):
    """An exception raised in the region is the one that leaves it, with a failing flush's error chained as its cause; without
    one, the flush's error is raised."""
    from flamo_amd import _lib, ops
    stub = _FailingFlush()
    monkeypatch.setattr(_lib, "lib", lambda pair_ok=False: stub)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "LAUNCH_PAIRS", True)
    with pytest.raises(KeyError) as ei:
        with ops.paired_launch(True):
            raise KeyError("body")
    assert ei.value.args == ("body",)
    assert isinstance(ei.value.__cause__, RuntimeError) and "device lost" in str(ei.value.__cause__)
    assert stub.flushes == 1
    assert getattr(_lib._pair, "stream_of", None) is None
    with pytest.raises(RuntimeError, match="device lost"):
        with ops.paired_launch(True):
            pass
    assert stub.flushes == 2
    assert getattr(_lib._pair, "stream_of", None) is None
