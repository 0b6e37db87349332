"""Every cascade response route of flamo_amd/ops.py (Biquad / SVF / PEQ / SOSFilter / GEQ, csrc/response.hip, csrc/cascade2.hip,
csrc/rc_ba_body.h) and its gradients against float64 CPU autograd over oracle/hotpath.py.

The GPU-against-GPU tests (test_cascade2.py and the module parity files) cannot see a mistake in index arithmetic that the float
and double kernels share through their templates; here the yardstick is O.sos_response_at / O.geq_response_at (the reference's
cascade tail at chosen bins, float64) and, for graphic equalisers, O.geq_sos(exact=True).

- Gradients are taken under a complex cotangent that is non-zero only on a chosen bin set (DC, Nyquist / the last bin, 255-257,
  the edges of the bin tiles and blocks of the backward kernels, the edges of a shard, random interior bins), so the oracle needs
  those bins alone at any transform length, and each gradient entry reflects those bins rather than an average over all of them.
- Comparisons are per row -- a channel pair's response over the bins, a (section, pair)'s six coefficient gradients, a pair's
  band gradients, a row of the constant factor's gradient -- by the max-norm relative to that row (`_rows`), recorded through
  cc() on the row-normalised arrays, whose max-norm error is exactly the worst row's.
- Every case asserts the route it names (the C entry points called, `_spy`; the dispatch predicates) and restores every debug
  knob (`_knobs`).  Before the operation under test the caching allocator is handed NaN-filled blocks of the sizes the op asks
  for (`_poison`): an entry that is never written shows up as NaN.

Tolerances (per-row max-norm, and l2 of the row-normalised arrays):
- float64: responses 5e-11 and gradients 5e-10, not 1e-12 / 1e-10: two float64 evaluations of the same cascade differ by the
  evaluation's conditioning, kappa = sum_s (|b0| + |b1 z| + |b2 z^2|) / |B_s(z)| (and A), times 2^-53.  At a bin within ~1e-3
  rad of the angle of the pole at radius 0.999, |A_s| = |1 - p z| |1 - conj(p) z| is ~1e-6 of its taps: kappa = 1.3e6 in the
  23 x 23 x 3-section draw at 4801 (the random zeros give at most 3e3), i.e. ~1.5e-10 relative at that bin, whose row maximum
  is the resonance itself; near DC the GEQ shelves and peaks do the same (A_s(1) ~ 1e-5).  Measured 3.0e-12 (GEQ, 96000) and
  2.7e-11 (that draw) for the responses, 1.2e-10 for that case's coefficient gradients.
- float32 with the cascade evaluated in double and rounded once: responses 1e-6, coefficient gradients and dL/dWr 1e-5, the
  levels the suite already holds.
- float32 with the cascade evaluated in float (FLOAT_CASCADE_EVAL: fl_sos_response_f32eval_c64, the GEQ forward, the rc fast /
  second-generation forward, the one-launch apply): responses 5e-5.  The float evaluation's error grows with the section count
  and the conditioning: measured 1.4e-6 (24 sections), 5.5e-6 (GEQ at nfft = 95), 1.4e-5 (a pole at radius 0.999; 3.0e-5 in
  dL/dX = H^H gY of a 24-section cascade with such a pole).
- float32 equaliser gains: 5e-5 per channel pair.  The backward reuses the saved float32 response, and the design's map adds the
  cancellation between the numerator and denominator taps: measured up to 3.3e-5 on the sparse bin sets (the suite's 5e-6 .. 1e-5
  are global l2 errors under white cotangents, which average it out)."""
import contextlib

import pytest
import torch

from conftest import cc

FS = 48000
NAN = float("nan")
TOL64_H, TOL64_G = 5e-11, 5e-10
TOL32_H, TOL32_G = 1e-6, 1e-5
TOL32_FE = 5e-5        # float-evaluated responses (see above)
TOL32_GAIN = 5e-5      # float32 equaliser gains (see above)


# ----------------------------------------------------------------------------- bins
def _bin_set(nfft, bin0=0, m_local=None, seed=0, n_random=8):
    """global bin numbers (int64, sorted) inside [bin0, bin0 + m_local): DC, the last bin (Nyquist for even nfft), 255-257,
    511-513, the quarter-turn boundary of the float kernels' two bases, edges of 32-bin tiles and 256-bin blocks, both edges
    of the range, random interior bins"""
    M = nfft // 2 + 1
    if m_local is None:
        m_local = M - bin0
    lo, hi = bin0, bin0 + m_local
    g = torch.Generator().manual_seed(1000 + seed)
    q4 = (nfft + 3) // 4
    cand = [0, 1, M - 2, M - 1, 255, 256, 257, 511, 512, 513, q4 - 1, q4, q4 + 1,
            lo, lo + 1, hi - 2, hi - 1]
    for step in (32, 256):
        # tile / block edges counted from the range's start (the backward kernels' bin blocks) and from the quarter turn
        # (the lanes kernel's tiles restart there)
        for base in (lo, q4):
            js = torch.randint(1, max(2, m_local // step + 1), (6,), generator=g).tolist() + [1, 2]
            for j in js:
                cand += [base + j * step - 1, base + j * step]
    if m_local > 0:
        cand += torch.randint(lo, hi, (n_random,), generator=g).tolist()
    return torch.tensor(sorted({k for k in cand if lo <= k < hi}), dtype=torch.int64)


def _elems(bins, nfft, bin0=0, order=None):
    """element (row index of the returned response) of each global bin: contiguous from bin0, or the row-major order of the
    fused pipeline (element k1*L2 + k2 holds bin k1 + L1*k2, element nfft/2 the Nyquist bin; csrc/response_common.h)"""
    if order is None:
        return bins - bin0
    L1, L2 = order
    L = nfft // 2
    k1, k2 = bins % L1, bins // L1
    return torch.where(bins >= L, bins, k1 * L2 + k2)


def _cotangent(shape, elems, dtype, dev, seed):
    """complex cotangent of `shape` (bins first) non-zero only at rows `elems`: (full GPU tensor, the rows (float64, CPU))"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.complex(torch.randn((len(elems),) + tuple(shape[1:]), generator=g, dtype=torch.float64),
                         torch.randn((len(elems),) + tuple(shape[1:]), generator=g, dtype=torch.float64))
    ct = torch.zeros(shape, dtype=dtype, device=dev)
    if len(elems):
        ct[elems.to(dev)] = rows.to(dev, dtype)
    return ct, ct[elems.to(dev)].cpu().to(torch.complex128)


# ----------------------------------------------------------------------------- comparison
def _rows(label, got, ref, tol):
    """got, ref laid out as (rows, entries): max-norm error of each row relative to that row's max |ref|, at most `tol`.
    Recorded through cc() on the row-normalised arrays (whose max-norm error is the worst row's)."""
    got = got.detach().cpu().to(ref.dtype)
    assert got.shape == ref.shape, (label, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(torch.view_as_real(got) if got.is_complex() else got).all()), (label, "non-finite entries")
    if ref.numel() == 0:
        return 0.0
    scale = ref.abs().amax(dim=1, keepdim=True)
    zero = scale.squeeze(1) == 0
    if bool(zero.any()):       # rows that are exactly zero in float64 must be exactly zero here
        assert bool((got[zero] == 0).all()), (label, "non-zero entries in a row the oracle holds at exactly zero")
    scale = torch.where(scale == 0, torch.ones_like(scale), scale)
    gn, rn = got / scale, ref / scale
    err = (gn - rn).abs().amax(dim=1)
    worst = int(err.argmax())
    print(f"[rows] {label}: {got.shape[0]} rows, worst row {worst} max-norm {err[worst].item():.3e} (limit {tol:g})")
    return cc(label, gn, rn, tol, max_tol=tol)


def _resp_rows(H, elems):
    """(bins, chan...) response -> (pairs, bins) at the chosen rows"""
    h = H.detach()[elems.to(H.device)].cpu()
    return h.flatten(1).transpose(0, 1)


def _coef_rows(gb, ga):
    """dL/db, dL/da (3, S, chan...) -> ((S * pairs), 6) rows: a (section, pair)'s six taps"""
    S = gb.shape[1]
    g = torch.cat([gb.reshape(3, S, -1), ga.reshape(3, S, -1)], 0)     # (6, S, C)
    return g.permute(1, 2, 0).reshape(-1, 6)


def _band_rows(gx):
    """dL/dx of an equaliser (bands, chan...) -> (pairs, bands)"""
    return gx.reshape(gx.shape[0], -1).transpose(0, 1)


# ----------------------------------------------------------------------------- knobs, routes, poisoning
@contextlib.contextmanager
def _knobs(lanes=None, rc_fast=None, chunk=None, float_eval=None, mixed=None, narrow=None, shard=None, row_major=None):
    """set the cascade debug knobs for the body and restore their previous values in `finally`"""
    from flamo_amd import _lib, ops
    from flamo_amd.processor import dsp
    L = _lib.lib()
    prev = dict(fe=ops.FLOAT_CASCADE_EVAL, mx=ops.SOS_BWD_MIXED, na=dsp.NARROW_APPLY)
    prev_lanes = L.fl_debug_set_cascade_lanes(-1, -1, -1)      # (the setters return the previous value; -1 only asks)
    prev_fast = L.fl_debug_set_rc_fast(-1)
    prev_chunk = L.fl_debug_set_sos_chunk(-1)
    try:
        if lanes is not None:
            L.fl_debug_set_cascade_lanes(int(lanes), -1, -1)
        if rc_fast is not None:
            L.fl_debug_set_rc_fast(int(rc_fast))
        if chunk is not None:
            L.fl_debug_set_sos_chunk(int(chunk))
        if float_eval is not None:
            ops.FLOAT_CASCADE_EVAL = bool(float_eval)
        if mixed is not None:
            ops.SOS_BWD_MIXED = bool(mixed)
        if narrow is not None:
            dsp.NARROW_APPLY = bool(narrow)
        if shard is not None:
            ops.set_bin_shard(*shard)
        with (ops.row_major_bins(row_major) if row_major else contextlib.nullcontext()):
            yield
    finally:
        ops.set_bin_shard(0, None)
        L.fl_debug_set_cascade_lanes(prev_lanes, -1, -1)
        L.fl_debug_set_rc_fast(prev_fast)
        L.fl_debug_set_sos_chunk(prev_chunk)
        ops.FLOAT_CASCADE_EVAL, ops.SOS_BWD_MIXED, dsp.NARROW_APPLY = prev["fe"], prev["mx"], prev["na"]


@contextlib.contextmanager
def _spy(*names):
    """count the calls of C entry points of the library during the body: {name: calls}"""
    from flamo_amd import _lib
    L = _lib.lib()
    calls = {n: 0 for n in names}
    orig = {n: getattr(L, n) for n in names}

    def wrap(n):
        f = orig[n]

        def g(*args):
            calls[n] += 1
            return f(*args)
        return g

    for n in names:
        setattr(L, n, wrap(n))
    try:
        yield calls
    finally:
        for n in names:
            setattr(L, n, orig[n])


def _poison(dev, *nbytes, copies=2):
    """hand the caching allocator NaN-filled blocks of these byte sizes (freed at once): the op's own buffers (part, psum, pq,
    partW, H, G, Y) of the same sizes are carved from them, so an entry the kernels never write reads NaN"""
    blocks = [torch.full(((int(n) + 7) // 8,), NAN, dtype=torch.float64, device=dev) for n in nbytes if n > 0 for _ in range(copies)]
    torch.cuda.synchronize(dev)
    del blocks


def _rows_bytes(chan_pairs, m_local, esz):
    from flamo_amd import ops
    return chan_pairs * ops._pitch(m_local) * esz


# ----------------------------------------------------------------------------- coefficients
def _sections(S, chan, seed, zeros_dc_nyq=False, sharp=False):
    """random stable sections (3, S, *chan) float64: poles at radius 0.3 .. 0.95 (0.999 for the first section when `sharp`),
    zeros anywhere within radius 1.3; with `zeros_dc_nyq` every third section is a band-pass numerator (b1 = 0, b2 = -b0):
    zeros exactly at DC and at Nyquist"""
    g = torch.Generator().manual_seed(seed)
    shp = (S,) + tuple(chan)
    r = 0.3 + 0.65 * torch.rand(shp, generator=g, dtype=torch.float64)
    if sharp:
        r[0] = 0.999
    th = torch.pi * torch.rand(shp, generator=g, dtype=torch.float64)
    a = torch.stack([torch.ones(shp, dtype=torch.float64), -2 * r * torch.cos(th), r * r])
    rz = 1.3 * torch.rand(shp, generator=g, dtype=torch.float64)
    tz = torch.pi * torch.rand(shp, generator=g, dtype=torch.float64)
    k = 0.5 + torch.rand(shp, generator=g, dtype=torch.float64)
    b = torch.stack([k, -2 * k * rz * torch.cos(tz), k * rz * rz])
    if zeros_dc_nyq:
        for s in range(0, S, 3):
            b[0, s], b[1, s], b[2, s] = k[s], 0.0, -k[s]
    return b, a


def _geq_param(nb, chan, seed, sig, dtype):
    """raw equaliser parameters of both signs: |x| at -12 .. +12 dB (a few exactly at +-12 dB, the rest inside), or
    sigmoid-map parameters in -2 .. 3"""
    g = torch.Generator().manual_seed(seed)
    shp = (nb,) + tuple(chan)
    if sig:
        return (-2 + 5 * torch.rand(shp, generator=g, dtype=torch.float64)).to(dtype)
    db = -12 + 24 * torch.rand(shp, generator=g, dtype=torch.float64)
    flat = db.view(-1)
    flat[0::7] = 12.0 - 1e-3
    flat[3::7] = -12.0 + 1e-3
    sign = torch.where(torch.rand(shp, generator=g) < 0.5, -1.0, 1.0).to(torch.float64)
    return (sign * 10 ** (db / 20)).to(dtype)


def _geq_design(octave_interval=1):
    """the band constants dsp.GEQ hands the design kernels"""
    from flamo_amd.functional import GEQDesign, eq_freqs
    cf, sc = eq_freqs(interval=octave_interval)
    return GEQDesign(cf, sc, fs=FS, R=2.7)


def _geq_oracle_sections(x64, sig, octave_interval=1):
    from flamo_amd.processor import dsp
    from oracle import hotpath as O
    cf, sc = O.eq_freqs(octave_interval)
    gain_db = dsp.db_of_sigmoid(x64) if sig else 20 * torch.log10(torch.abs(x64))
    return O.geq_sos(gain_db, cf, sc, FS, exact=True)


def _gamma_f(db, nfft):
    return 10.0 ** (-abs(float(db)) / nfft / 20.0)


def _gamma_t(db, nfft):
    from oracle import hotpath as O
    return O.gamma_of(db, nfft)


def _sos_at(b, a, nfft, db, bins):
    from oracle import hotpath as O
    return O.sos_response_at(b, a, nfft, _gamma_t(db, nfft), bins)


def _shard_args(nfft, kind):
    """(bin0, m_local, order-or-None, shard-tuple-or-None) of a bin-range axis value"""
    from flamo_amd import _lib
    import ctypes
    M = nfft // 2 + 1
    if kind == "all":
        return 0, M, None, None
    if kind == "rowmajor":
        L1, L2 = ctypes.c_int(), ctypes.c_int()
        assert _lib.lib().fl_spec_plan(int(nfft), ctypes.byref(L1), ctypes.byref(L2)) == 0
        return -L2.value, M, (L1.value, L2.value), None
    if kind == "odd_near_nyq":       # odd bin0, the range ending at Nyquist
        m = min(M - 1, 1000) | 1
        b0 = (M - m) | 1
        return b0, M - b0, None, (b0, M - b0)
    if kind == "mid":                # odd bin0, an interior range of odd length
        b0 = (M // 3) | 1
        m = max(1, (M // 3) | 1)
        return b0, m, None, (b0, m)
    if kind == "one":                # m_local = 1
        b0 = (M // 2) | 1 if M > 2 else M - 1
        return b0, 1, None, (b0, 1)
    if kind == "empty":
        return M // 2, 0, None, (M // 2, 0)
    raise ValueError(kind)


# ============================================================================= 1. ops.sos_response
# (mode, nfft, S, chan, alias dB, bin range, coefficient kind, sos_chunk knob)
SOS_CASES = [
    ("c64", 96000, 12, (6, 6), 0.0, "all", "plain", 0),
    ("c64", 96000, 3, (3, 5), 30.0, "all", "zeros", 0),
    ("c64", 4801, 5, (1, 1), 60.0, "all", "sharp", 0),
    ("c64", 4801, 7, (23, 23), 0.0, "odd_near_nyq", "zeros", 0),
    ("c64", 510, 9, (3, 5), 30.0, "all", "plain", 8),
    ("c64", 512, 13, (6, 6), 0.0, "all", "zeros", 6),
    ("c64", 96000, 24, (3, 5), 30.0, "mid", "sharp", 1204),     # 12-section chunks, 12 bin blocks
    ("c64", 96000, 6, (6, 6), 0.0, "rowmajor", "plain", 304),
    ("c64", 30, 4, (1, 1), 0.0, "all", "zeros", 0),
    ("c64", 3, 1, (3, 5), 30.0, "all", "plain", 0),
    ("c64", 2, 8, (1, 1), 0.0, "all", "sharp", 0),
    ("c64", 95, 12, (6, 6), 60.0, "one", "plain", 0),
    ("c64", 96000, 64, (1, 1), 30.0, "all", "plain", 0),
    ("c64", 96000, 12, (3, 5), 0.0, "empty", "plain", 0),
    ("c64x", 96000, 12, (6, 6), 30.0, "all", "zeros", 0),       # all-double backward (SOS_BWD_MIXED = False)
    ("c64x", 4801, 13, (3, 5), 0.0, "odd_near_nyq", "sharp", 4),
    ("c64x", 512, 9, (1, 1), 60.0, "all", "plain", 704),
    ("c64x", 96000, 4, (6, 6), 0.0, "rowmajor", "zeros", 4),
    ("c64x", 95, 3, (3, 5), 30.0, "empty", "plain", 0),
    ("f64", 96000, 12, (6, 6), 30.0, "all", "zeros", 0),
    ("f64", 4801, 3, (23, 23), 0.0, "all", "sharp", 0),
    ("f64", 96000, 13, (3, 5), 60.0, "odd_near_nyq", "plain", 1206),
    ("f64", 510, 24, (1, 1), 0.0, "all", "plain", 4),
    ("f64", 96000, 5, (3, 5), 0.0, "rowmajor", "zeros", 0),
    ("f64", 2, 4, (1, 1), 30.0, "all", "zeros", 0),
    ("f64", 3, 7, (6, 6), 0.0, "one", "sharp", 0),
    ("f64", 30, 1, (3, 5), 0.0, "empty", "plain", 0),
    ("f32eval", 96000, 12, (6, 6), 30.0, "all", "plain", 0),
    ("f32eval", 4801, 3, (3, 5), 0.0, "odd_near_nyq", "zeros", 0),
    ("f32eval", 96000, 7, (1, 1), 60.0, "rowmajor", "plain", 0),
    ("f32eval", 2, 1, (3, 5), 0.0, "all", "plain", 0),
    ("f32eval", 95, 24, (6, 6), 0.0, "one", "plain", 0),
    ("f32eval", 510, 12, (3, 5), 0.0, "empty", "plain", 0),
]


def _sos_id(c):
    return "-".join(str(v).replace(" ", "").replace(",", "x").replace("(", "").replace(")", "") for v in c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", SOS_CASES, ids=_sos_id)
def test_sos_response_matches_float64(gpu, case):
    """ops.sos_response: float32 with the double evaluation (fl_sos_response_c64) and the mixed or all-double backward,
    float32 with the float evaluation under no_grad (fl_sos_response_f32eval_c64), float64 (_c128)"""
    from flamo_amd import _lib, ops
    mode, nfft, S, chan, db, rng, coef, chunk = case
    real = torch.float64 if mode == "f64" else torch.float32
    grad = mode != "f32eval"
    b, a = _sections(S, chan, seed=S * 7 + nfft % 97, zeros_dc_nyq=coef == "zeros", sharp=coef == "sharp")
    bin0, m_local, order, shard = _shard_args(nfft, rng)
    bins = _bin_set(nfft, max(bin0, 0), m_local, seed=S)
    el = _elems(bins, nfft, max(bin0, 0), order)
    C = max(1, int(torch.tensor(chan).prod()))
    esz = 16 if real == torch.float64 else 8
    L = _lib.lib()
    mixed = {"c64": True, "c64x": False}.get(mode)
    fwd = {"c64": "fl_sos_response_c64", "c64x": "fl_sos_response_c64", "f64": "fl_sos_response_c128",
           "f32eval": "fl_sos_response_f32eval_c64"}[mode]
    bwd = "fl_sos_response_bwd_c128" if mode == "f64" else "fl_sos_response_bwd_c64"
    with _knobs(chunk=chunk, mixed=mixed, float_eval=True, shard=shard,
                row_major=nfft if order else None):
        bg = b.to(gpu).requires_grad_(grad)
        ag = a.to(gpu).requires_grad_(grad)
        nblk = L.fl_sos_bwd_blocks(m_local, C, S, int(bool(mixed))) if m_local else 0
        _poison(gpu, _rows_bytes(C, m_local, esz), nblk * 6 * S * C * 8)
        with _spy(fwd, bwd) as calls, (contextlib.nullcontext() if grad else torch.no_grad()):
            H = ops.sos_response(bg, ag, _gamma_f(db, nfft), nfft, dtype=real)
            assert calls[fwd] == (1 if m_local else 0), (fwd, calls)
            assert H.shape == (m_local,) + tuple(chan) and H.dtype == (torch.complex128 if mode == "f64" else torch.complex64)
            if grad:
                ct, ct_sel = _cotangent(H.shape, el, H.dtype, gpu, seed=nfft + S)
                _poison(gpu, nblk * 6 * S * C * 8)
                (H * ct.conj()).real.sum().backward()
                assert calls[bwd] == (1 if m_local else 0), (bwd, calls)
        tag = f"{mode}/{rng}"
        th, tg = (TOL64_H, TOL64_G) if mode == "f64" else (TOL32_FE if mode == "f32eval" else TOL32_H, TOL32_G)
        bo, ao = b.clone().requires_grad_(True), a.clone().requires_grad_(True)
        Ho = _sos_at(bo, ao, nfft, db, bins)
        _rows(tag + "/H", _resp_rows(H, el), Ho.flatten(1).transpose(0, 1), th)
        if not grad:
            return
        if m_local == 0:
            assert bool((bg.grad == 0).all()) and bool((ag.grad == 0).all())
            return
        gbo, gao = torch.autograd.grad((Ho * ct_sel.reshape(Ho.shape).conj()).real.sum(), [bo, ao])
        _rows(tag + "/dba", _coef_rows(bg.grad.cpu(), ag.grad.cpu()), _coef_rows(gbo, gao), tg)


@pytest.mark.gpu
def test_sos_response_dense_small(gpu):
    """every bin under the cotangent at nfft = 30 and 95, float32 (mixed backward) and float64"""
    from flamo_amd import _lib, ops
    for nfft in (30, 95):
        for real in (torch.float32, torch.float64):
            b, a = _sections(5, (3, 5), seed=nfft, zeros_dc_nyq=True)
            bg, ag = b.to(gpu).requires_grad_(True), a.to(gpu).requires_grad_(True)
            f64 = real == torch.float64
            M, C = nfft // 2 + 1, 15
            fwd, bwd = ("fl_sos_response_c128", "fl_sos_response_bwd_c128") if f64 else ("fl_sos_response_c64", "fl_sos_response_bwd_c64")
            nblk = _lib.lib().fl_sos_bwd_blocks(M, C, 5, int(not f64))
            with _knobs(mixed=True), _spy(fwd, bwd) as calls:
                _poison(gpu, _rows_bytes(C, M, 16 if f64 else 8), nblk * 6 * 5 * C * 8)
                H = ops.sos_response(bg, ag, _gamma_f(30.0, nfft), nfft, dtype=real)
                bins = torch.arange(M)
                ct, ct_sel = _cotangent(H.shape, bins, H.dtype, gpu, seed=nfft)
                _poison(gpu, nblk * 6 * 5 * C * 8)
                (H * ct.conj()).real.sum().backward()
            assert calls[fwd] == 1 and calls[bwd] == 1, calls
            bo, ao = b.clone().requires_grad_(True), a.clone().requires_grad_(True)
            Ho = _sos_at(bo, ao, nfft, 30.0, bins)
            _rows(f"{nfft}_{int(f64)}/H", _resp_rows(H, bins), Ho.flatten(1).transpose(0, 1), TOL64_H if f64 else TOL32_H)
            gbo, gao = torch.autograd.grad((Ho * ct_sel.conj()).real.sum(), [bo, ao])
            _rows(f"{nfft}_{int(f64)}/dba", _coef_rows(bg.grad.cpu(), ag.grad.cpu()), _coef_rows(gbo, gao), TOL64_G if f64 else TOL32_G)


# ============================================================================= 2. ops.geq_cascade (plain)
# (dtype, lanes, gain map, nfft, chan, alias dB, bin range, octave interval)
GEQ_CASES = [
    (torch.float32, 1, "abs", 96000, (6, 6), 0.0, "all", 1),
    (torch.float32, 0, "abs", 96000, (6, 6), 0.0, "all", 1),
    (torch.float32, 1, "sigmoid", 96000, (32, 32), 30.0, "odd_near_nyq", 1),
    (torch.float32, 0, "sigmoid", 4801, (3, 5), 60.0, "all", 1),
    (torch.float32, 1, "abs", 4801, (23, 23), 30.0, "all", 3),
    (torch.float32, 1, "abs", 96000, (8,), 0.0, "rowmajor", 1),
    (torch.float32, 1, "sigmoid", 384000, (8, 8), 60.0, "all", 1),
    (torch.float32, 0, "abs", 510, (1, 1), 0.0, "all", 3),
    (torch.float32, 1, "abs", 512, (6, 6), 30.0, "one", 1),
    (torch.float32, 1, "abs", 96000, (6, 6), 0.0, "empty", 1),
    (torch.float32, 0, "sigmoid", 3, (3, 5), 0.0, "all", 1),
    (torch.float64, 1, "abs", 96000, (6, 6), 30.0, "all", 1),
    (torch.float64, 0, "abs", 96000, (6, 6), 30.0, "all", 1),
    (torch.float64, 1, "sigmoid", 96000, (16,), 0.0, "odd_near_nyq", 1),
    (torch.float64, 0, "sigmoid", 4801, (23, 23), 60.0, "all", 3),
    (torch.float64, 1, "abs", 96000, (6, 6), 0.0, "rowmajor", 1),
    (torch.float64, 1, "abs", 30, (3, 5), 0.0, "all", 1),
    (torch.float64, 0, "abs", 2, (1, 1), 30.0, "all", 1),
    (torch.float64, 1, "abs", 95, (6, 6), 0.0, "empty", 1),
]


def _geq_id(c):
    dt, lanes, gm, nfft, chan, db, rng, oi = c
    return f"{str(dt)[-7:]}-l{lanes}-{gm}-{nfft}-{'x'.join(map(str, chan))}-{int(db)}-{rng}-oct{oi}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", GEQ_CASES, ids=_geq_id)
def test_geq_cascade_matches_float64(gpu, case):
    """ops.geq_cascade: lanes-per-section backward (mode 0) on and off, float32 / float64, both gain maps, raw parameters of
    both signs near +-12 dB; the equaliser gradient against the float64 backward of geq_sos(exact=True)"""
    from flamo_amd import _lib, ops
    real, lanes, gm, nfft, chan, db, rng, oi = case
    f64 = real == torch.float64
    sig = gm == "sigmoid"
    from oracle import hotpath as O
    design = _geq_design(oi)
    nb = len(O.eq_freqs(oi)[0]) + 3
    x = _geq_param(nb, chan, seed=nfft % 1000 + nb, sig=sig, dtype=real)
    bin0, m_local, order, shard = _shard_args(nfft, rng)
    bins = _bin_set(nfft, max(bin0, 0), m_local, seed=nb)
    el = _elems(bins, nfft, max(bin0, 0), order)
    C = max(1, int(torch.tensor(chan).prod()))
    esz = 16 if f64 else 8
    L = _lib.lib()
    fwd = "fl_sos_response_c128" if f64 else "fl_geq_response_c64"
    lanes_fn = "fl_geq_response_bwd_lanes_c128" if f64 else "fl_geq_response_bwd_lanes_c64"
    gen1 = "fl_sos_response_bwd_c128" if f64 else "fl_sos_response_bwd_c64"
    with _knobs(lanes=lanes, shard=shard, row_major=nfft if order else None):
        bo_ = _lib.lib().fl_geq_bwd_lanes_blocks_f64 if f64 else _lib.lib().fl_geq_bwd_lanes_blocks
        nbx = bo_(m_local, C, nb, nfft, bin0, 1, 0, 0) if m_local else 0
        if lanes and rng != "empty":
            assert nbx > 0, "the lanes kernel must take this shape"
        nblk = L.fl_sos_bwd_blocks(m_local, C, nb, 1) if m_local else 0
        consts = design.device_consts(gpu)
        xg = x.to(gpu).requires_grad_(True)
        _poison(gpu, _rows_bytes(C, m_local, esz))
        with _spy(fwd, lanes_fn, gen1) as calls:
            H = ops.geq_cascade(xg, consts, _gamma_f(db, nfft), nfft, dtype=real, gain_map=gm)
            assert calls[fwd] == (1 if (m_local or not f64) else 0), calls
            ct, ct_sel = _cotangent(H.shape, el, H.dtype, gpu, seed=nfft + nb)
            _poison(gpu, nblk * 6 * nb * C * 8, nb * C * max(nbx, 1) * 4 * (esz // 2), C * max(nbx, 1) * (esz // 2))
            (H * ct.conj()).real.sum().backward()
            if m_local:
                assert calls[lanes_fn] == int(bool(lanes)) and calls[gen1] == int(not lanes), calls
    tag = f"{str(real)[-7:]}/{rng}"
    xo = x.double().requires_grad_(True)
    bo, ao = _geq_oracle_sections(xo, sig, oi)
    Ho = O.sos_response_at(bo, ao, nfft, _gamma_t(db, nfft), bins)
    _rows(tag + "/H", _resp_rows(H, el), Ho.flatten(1).transpose(0, 1).detach(), TOL64_H if f64 else TOL32_FE)
    if m_local == 0:
        assert bool((xg.grad == 0).all())
        return
    gxo, = torch.autograd.grad((Ho * ct_sel.reshape(Ho.shape).conj()).real.sum(), [xo])
    _rows(tag + "/dx", _band_rows(xg.grad.cpu().double()), _band_rows(gxo), TOL64_G if f64 else TOL32_GAIN)


# ============================================================================= 3. rc: cascade times a real constant matrix
# (kind sos|geq, dtype, rc_fast, lanes, No, Nmid, Ni, S / octave interval, nfft, alias dB, bin range, which gradients, chunk)
RC_CASES = [
    ("geq", torch.float32, 1, 1, 8, 8, 8, 1, 96000, 0.0, "all", "x", 0),
    ("geq", torch.float32, 1, 0, 8, 8, 8, 1, 96000, 0.0, "all", "x", 0),
    ("geq", torch.float32, 0, 0, 4, 4, 4, 1, 4801, 30.0, "odd_near_nyq", "x", 0),
    ("geq", torch.float32, 1, 1, 4, 2, 2, 1, 96000, 60.0, "rowmajor", "x", 0),
    ("geq", torch.float32, 1, 1, 3, 16, 16, 1, 96000, 30.0, "all", "x", 0),
    ("geq", torch.float32, 1, 0, 5, 3, 4, 3, 510, 0.0, "all", "x", 8),
    ("geq", torch.float32, 1, 1, 8, 8, 8, 1, 95, 0.0, "one", "x", 0),
    ("geq", torch.float32, 1, 1, 8, 8, 8, 1, 96000, 0.0, "empty", "x", 0),
    ("geq", torch.float64, 0, 1, 8, 8, 8, 1, 96000, 30.0, "all", "x", 0),
    ("geq", torch.float64, 0, 0, 6, 4, 2, 1, 4801, 0.0, "all", "x", 0),
    ("geq", torch.float64, 0, 1, 4, 2, 2, 1, 96000, 60.0, "rowmajor", "x", 0),
    ("geq", torch.float64, 0, 1, 4, 4, 4, 1, 96000, 0.0, "rowmajor", "x", 0),
    ("geq", torch.float64, 0, 1, 8, 8, 8, 1, 96000, 30.0, "rowmajor", "x", 0),
    ("geq", torch.float64, 0, 0, 3, 5, 16, 1, 512, 0.0, "odd_near_nyq", "x", 0),
    ("geq", torch.float64, 0, 1, 4, 4, 4, 1, 30, 0.0, "all", "x", 0),
    ("sos", torch.float32, 1, 0, 3, 5, 2, 12, 96000, 0.0, "all", "Wr", 0),         # no coefficient gradient: float forward
    ("sos", torch.float32, 0, 0, 3, 5, 2, 12, 96000, 0.0, "all", "Wr", 0),
    ("sos", torch.float32, 1, 0, 6, 6, 4, 3, 4801, 30.0, "odd_near_nyq", "both", 0),
    ("sos", torch.float32, 1, 0, 2, 3, 8, 7, 96000, 60.0, "rowmajor", "both", 306),
    ("sos", torch.float32, 1, 0, 1, 2, 16, 24, 512, 0.0, "all", "both", 12),
    ("sos", torch.float32, 1, 0, 3, 2, 2, 64, 96000, 30.0, "all", "both", 0),        # 64 sections: the predicate's limit
    ("sos", torch.float32, 1, 0, 2, 3, 2, 4, 2, 0.0, "all", "Wr", 0),
    ("sos", torch.float32, 1, 0, 4, 2, 4, 9, 95, 0.0, "empty", "both", 0),
    ("sos", torch.float64, 0, 0, 3, 5, 2, 12, 96000, 30.0, "all", "both", 0),       # 12 sections: float64's limit
    ("sos", torch.float64, 0, 0, 2, 3, 4, 13, 4801, 30.0, "all", "both", 0),      # 13: beyond the predicate, called directly
    ("sos", torch.float64, 0, 0, 6, 6, 16, 4, 4801, 0.0, "odd_near_nyq", "both", 0),
    ("sos", torch.float64, 0, 0, 2, 3, 8, 1, 96000, 60.0, "rowmajor", "both", 1000),
    ("sos", torch.float64, 0, 0, 1, 1, 4, 3, 3, 0.0, "one", "both", 0),
]


def _rc_id(c):
    kind, dt, fast, lanes, No, Nmid, Ni, S, nfft, db, rng, gr, chunk = c
    return f"{kind}-{str(dt)[-7:]}-f{fast}-l{lanes}-{No}x{Nmid}x{Ni}-S{S}-{nfft}-{int(db)}-{rng}-{gr}-c{chunk}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", RC_CASES, ids=_rc_id)
def test_cascade_rc_matches_float64(gpu, case):
    """ops.sos_response_rc / ops.geq_cascade_rc: H = G Wr with G the (No, Nmid) cascade; _c64 (rc_fast on / off) and _c128;
    backward through the lanes kernel (mode 1) or _cascade_rc_backward + fl_geq_sections_bwd_w / _w64; dL/dWr and the gain
    or coefficient gradients"""
    from flamo_amd import _lib, ops
    from oracle import hotpath as O
    kind, real, fast, lanes, No, Nmid, Ni, S, nfft, db, rng, which, chunk = case
    f64 = real == torch.float64
    if kind == "geq":
        oi = S
        S = len(O.eq_freqs(oi)[0]) + 3
    assert ops.cascade_rc_supported(real, Ni, Nmid, S) or (f64 and S == 13)
    bin0, m_local, order, shard = _shard_args(nfft, rng)
    bins = _bin_set(nfft, max(bin0, 0), m_local, seed=S + Ni)
    el = _elems(bins, nfft, max(bin0, 0), order)
    C = No * Nmid
    esz = 16 if f64 else 8
    L = _lib.lib()
    g = torch.Generator().manual_seed(No * 100 + Nmid * 10 + Ni)
    W = (torch.randn(Nmid, Ni, generator=g, dtype=torch.float64) / Nmid ** 0.5).to(real)
    want_w = which in ("Wr", "both", "x")
    want_c = which in ("both", "x")
    sfx = "c128" if f64 else "c64"
    fwd = f"fl_geq_response_rc_{sfx}" if kind == "geq" else f"fl_sos_response_rc_{sfx}"
    lanes_fn = f"fl_geq_response_bwd_lanes_{sfx}"
    gen1 = f"fl_sos_response_bwd_rc_{sfx}"
    wsum = "fl_geq_sections_bwd_w64" if f64 else "fl_geq_sections_bwd_w"
    with _knobs(lanes=lanes, rc_fast=fast, chunk=chunk, shard=shard, row_major=nfft if order else None):
        if kind == "geq":
            design = _geq_design(oi)
            x = _geq_param(S, (No, Nmid), seed=nfft % 1000 + S, sig=False, dtype=real)
            xg = x.to(gpu).requires_grad_(True)
            nbx = (L.fl_geq_bwd_lanes_blocks_f64 if f64 else L.fl_geq_bwd_lanes_blocks)(m_local, C, S, nfft, bin0, Nmid, Ni, 1) if m_local else 0
            if lanes and rng != "empty":
                assert nbx > 0, "the lanes kernel must take this shape"
            # float64, constant factor, row-major bins: the lanes kernel is held back (ops.LANES_F64_ROW_MAJOR_RC)
            gated = f64 and order is not None and not ops.LANES_F64_ROW_MAJOR_RC
        else:
            b, a = _sections(S, (No, Nmid), seed=S * 3 + Ni, zeros_dc_nyq=S % 2 == 1, sharp=S % 3 == 0)
            bg, ag = b.to(gpu).requires_grad_(want_c), a.to(gpu).requires_grad_(want_c)
            nbx = 0
        Wg = W.to(gpu).requires_grad_(want_w)
        nblk = L.fl_sos_bwd_blocks(m_local, C, S, 0 if f64 else 1) if m_local else 0
        _poison(gpu, _rows_bytes(C, m_local, esz), _rows_bytes(No * Ni, m_local, esz))
        with _spy(fwd, lanes_fn, gen1, wsum) as calls:
            if kind == "geq":
                H = ops.geq_cascade_rc(xg, design.device_consts(gpu), Wg, _gamma_f(db, nfft), nfft, dtype=real)
            else:
                H = ops.sos_response_rc(bg, ag, Wg, _gamma_f(db, nfft), nfft, dtype=real)
            assert calls[fwd] == (1 if (m_local or kind == "geq") else 0), calls
            assert H.shape == (m_local, No, Ni)
            ct, ct_sel = _cotangent(H.shape, el, H.dtype, gpu, seed=nfft + Ni)
            wrows = (L.fl_geq_bwd_lanes_wrows_f64 if f64 else L.fl_geq_bwd_lanes_wrows)(m_local, C, S, nfft, bin0, Nmid, Ni) if nbx else 0
            _poison(gpu, nblk * 6 * S * C * 8, nblk * C * Ni * (esz // 2), S * C * max(nbx, 1) * 4 * (esz // 2),
                    C * max(nbx, 1) * (esz // 2), Nmid * Ni * wrows * (esz // 2))
            (H * ct.conj()).real.sum().backward()
            if m_local:
                if kind == "geq":
                    use = bool(lanes) and not gated
                    assert calls[lanes_fn] == int(use) and calls[gen1] == int(not use) and calls[wsum] == int(not use), calls
                else:
                    assert calls[gen1] == 1 and calls[lanes_fn] == 0, calls
    tag = f"{kind}_{str(real)[-7:]}/{rng}"
    Wo = W.double().requires_grad_(True)
    if kind == "geq":
        xo = x.double().requires_grad_(True)
        bo, ao = _geq_oracle_sections(xo, False, oi)
        leaves = [xo, Wo]
    else:
        bo, ao = b.clone().requires_grad_(True), a.clone().requires_grad_(True)
        leaves = [bo, ao, Wo]
    Go = O.sos_response_at(bo, ao, nfft, _gamma_t(db, nfft), bins)             # (nb, No, Nmid)
    Ho = Go @ O.to_complex(Wo).to(Go.dtype)
    float_eval = not f64 and fast and (kind == "geq" or not want_c)
    _rows(tag + "/H", _resp_rows(H, el), Ho.flatten(1).transpose(0, 1).detach(),
          TOL64_H if f64 else (TOL32_FE if float_eval else TOL32_H))
    tg = TOL64_G if f64 else TOL32_G
    if m_local == 0:
        for t in ([xg] if kind == "geq" else ([bg, ag] if want_c else [])) + ([Wg] if want_w else []):
            assert bool((t.grad == 0).all())
        return
    grads = torch.autograd.grad((Ho * ct_sel.reshape(Ho.shape).conj()).real.sum(), leaves)
    if want_w:
        _rows(tag + "/dWr", Wg.grad.cpu().double(), grads[-1], tg)
    if kind == "geq":
        _rows(tag + "/dx", _band_rows(xg.grad.cpu().double()), _band_rows(grads[0]), TOL64_G if f64 else TOL32_GAIN)
    elif want_c:
        _rows(tag + "/dba", _coef_rows(bg.grad.cpu(), ag.grad.cpu()), _coef_rows(grads[0], grads[1]), tg)
    else:
        assert bg.grad is None and ag.grad is None


@pytest.mark.gpu
def test_cascade_rc_section_limits(gpu):
    """cascade_rc_supported at its limits: 64 against 65 sections in float32, 12 against 13 in float64, 2/4/8/16 columns; 65
    sections are refused by the kernel, not evaluated by another route (the 64- and 13-section operators: RC_CASES)"""
    from flamo_amd import ops
    assert ops.cascade_rc_supported(torch.float32, 2, 3, 64) and not ops.cascade_rc_supported(torch.float32, 2, 3, 65)
    assert ops.cascade_rc_supported(torch.float64, 2, 3, 12) and not ops.cascade_rc_supported(torch.float64, 2, 3, 13)
    for n in (3, 5, 6, 7):
        assert not ops.cascade_rc_supported(torch.float32, n, 3, 4)
    b, a = _sections(65, (2, 3), seed=65)
    with pytest.raises(RuntimeError, match="bad sizes"):       # the kernel refuses: no silent fall-back
        ops.sos_response_rc(b.to(gpu), a.to(gpu), torch.randn(3, 2, device=gpu), 1.0, 960)


# ============================================================================= 4. apply: cascade times a signal of few columns
# (kind, B, S / octave interval, No, Ni ("max" / "max+1" / int), nfft, alias dB, bin range, grads: "c" coefficients, "x" signal)
APPLY_CASES = [
    ("sos", 1, 12, 3, 5, 96000, 0.0, "all", "x"),          # one launch (no coefficient gradient), dL/dX
    ("sos", 2, 3, 6, 6, 4801, 30.0, "odd_near_nyq", ""),
    ("sos", 2, 24, 2, "max", 96000, 60.0, "all", "x"),     # the largest tables that fit in LDS: one launch
    ("sos", 2, 24, 2, "max+1", 96000, 60.0, "all", "x"),   # one more: two launches
    ("sos", 1, 13, 4, 4, 510, 0.0, "all", "c"),            # coefficient gradient: double evaluation, outer-product backward
    ("sos", 2, 7, 23, 23, 4801, 0.0, "mid", "cx"),
    ("sos", 3, 4, 3, 5, 96000, 30.0, "all", "cx"),         # three columns: two launches
    ("sos", 1, 9, 32, 32, 512, 0.0, "one", "cx"),
    ("sos", 2, 2, 1, 1, 2, 0.0, "all", "cx"),
    ("sos", 2, 12, 3, 5, 96000, 0.0, "empty", "cx"),
    ("geq", 1, 1, 8, 8, 96000, 0.0, "all", "cx"),
    ("geq", 2, 1, 6, 6, 4801, 60.0, "odd_near_nyq", "c"),
    ("geq", 2, 3, 3, 5, 96000, 30.0, "all", "x"),          # third-octave (30 sections), frozen, X.requires_grad
    ("geq", 2, 1, 3, 5, 96000, 30.0, "all", "x"),          # frozen filter, X.requires_grad: no outer launch
    ("geq", 3, 1, 4, 4, 510, 0.0, "all", "cx"),
    ("geq", 1, 1, 23, 23, 3, 0.0, "all", "cx"),
    ("geq", 2, 1, 8, 8, 96000, 0.0, "empty", "cx"),
]


def _apply_id(c):
    return "-".join(str(v) for v in c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", APPLY_CASES, ids=_apply_id)
def test_cascade_apply_matches_float64(gpu, case):
    """ops.sos_response_apply / ops.geq_cascade_apply (Y = H X for B <= 2 columns): the one-launch
    sos_response_apply_fast_kernel<1|2> against the response launch + product, the outer-product backward
    (fl_sos_response_bwd_outer_c64) and dL/dX; a frozen filter with X.requires_grad runs no outer launch"""
    from flamo_amd import _lib, ops
    from oracle import hotpath as O
    kind, B, S, No, Ni, nfft, db, rng, which = case
    L = _lib.lib()
    if kind == "geq":
        oi = S
        S = len(O.eq_freqs(oi)[0]) + 3
    if Ni in ("max", "max+1"):
        Ni = L.fl_sos_response_apply_max_ni(S) + (1 if Ni == "max+1" else 0)
    want_c, want_x = "c" in which, "x" in which
    bin0, m_local, order, shard = _shard_args(nfft, rng)
    bins = _bin_set(nfft, bin0, m_local, seed=S + B)
    el = _elems(bins, nfft, bin0)
    C = No * Ni
    g = torch.Generator().manual_seed(S * 31 + Ni)
    X = torch.complex(torch.randn(B, m_local, Ni, generator=g), torch.randn(B, m_local, Ni, generator=g))
    one_launch = B <= 2 and Ni <= L.fl_sos_response_apply_max_ni(S) and (kind == "geq" or not want_c)
    with _knobs(shard=shard):
        Xg = X.to(gpu).requires_grad_(want_x)
        assert ops.cascade_apply_supported(torch.float32, Xg)
        if kind == "geq":
            design = _geq_design(oi)
            x = _geq_param(S, (No, Ni), seed=nfft % 1000 + S, sig=False, dtype=torch.float32)
            xg = x.to(gpu).requires_grad_(want_c)
        else:
            b, a = _sections(S, (No, Ni), seed=S * 5 + Ni, zeros_dc_nyq=S % 2 == 1, sharp=S % 3 == 0)
            bg, ag = b.to(gpu).requires_grad_(want_c), a.to(gpu).requires_grad_(want_c)
        nblk = L.fl_sos_bwd_blocks(m_local, C, S, 1) if m_local else 0
        _poison(gpu, _rows_bytes(C, m_local, 8), B * ops._pitch(m_local) * No * 8, B * m_local * No * 8)
        names = ("fl_sos_response_apply_c64", "fl_sos_response_c64", "fl_sos_response_f32eval_c64", "fl_sos_response_bwd_outer_c64")
        with _spy(*names) as calls:
            if kind == "geq":
                Y = ops.geq_cascade_apply(xg, design.device_consts(gpu), Xg, _gamma_f(db, nfft), nfft)
            else:
                Y = ops.sos_response_apply(bg, ag, Xg, _gamma_f(db, nfft), nfft)
            assert Y.shape == (B, m_local, No)
            # (an empty bin shard launches nothing)
            assert calls["fl_sos_response_apply_c64"] == int(one_launch and m_local > 0), calls
            assert calls["fl_sos_response_c64"] + calls["fl_sos_response_f32eval_c64"] == int(not one_launch and m_local > 0), calls
            if want_c or want_x:
                ct, ct_sel = _cotangent(Y.shape[1:], el, Y.dtype, gpu, seed=nfft + B)     # (bins, No) per column
                cts = torch.stack([ct * (1 + 0.5j * i) for i in range(B)])
                _poison(gpu, nblk * 6 * S * C * 8)
                (Y * cts.conj()).real.sum().backward()
                assert calls["fl_sos_response_bwd_outer_c64"] == int(want_c and m_local > 0), calls
    tag = f"{kind}/B{B}"
    if kind == "geq":
        xo = x.double().requires_grad_(True)
        bo, ao = _geq_oracle_sections(xo, False, oi)
        leaves = [xo]
    else:
        bo, ao = b.clone().requires_grad_(True), a.clone().requires_grad_(True)
        leaves = [bo, ao]
    Xo = X[:, el].to(torch.complex128).requires_grad_(True)
    Ho = O.sos_response_at(bo, ao, nfft, _gamma_t(db, nfft), bins)            # (nb, No, Ni)
    Yo = torch.einsum("kmn,bkn->bkm", Ho, Xo)
    got = Y.detach()[:, el.to(gpu)].cpu()
    th = TOL32_FE if (kind == "geq" or not want_c) else TOL32_H      # float evaluation unless a coefficient gradient is taken
    _rows(tag + "/Y", got.permute(0, 2, 1).reshape(B * No, -1), Yo.detach().permute(0, 2, 1).reshape(B * No, -1), th)
    if not (want_c or want_x):
        return
    if m_local == 0:
        for t in ([xg] if kind == "geq" else [bg, ag]) if want_c else []:
            assert bool((t.grad == 0).all())
        return
    cto = torch.stack([ct_sel * (1 + 0.5j * i) for i in range(B)])
    grads = torch.autograd.grad((Yo * cto.conj()).real.sum(), leaves + [Xo])
    if want_x:
        gX = Xg.grad
        sel = torch.zeros(m_local, dtype=torch.bool, device=gpu)
        sel[el.to(gpu)] = True
        assert bool((gX[:, ~sel] == 0).all()), "dL/dX must be exactly zero off the cotangent's bins"
        _rows(tag + "/dX", gX[:, el.to(gpu)].cpu().permute(0, 2, 1).reshape(B * Ni, -1),
              grads[-1].permute(0, 2, 1).reshape(B * Ni, -1), th)
    if want_c:
        if kind == "geq":
            _rows(tag + "/dx", _band_rows(xg.grad.cpu().double()), _band_rows(grads[0]), TOL32_GAIN)
        else:
            _rows(tag + "/dba", _coef_rows(bg.grad.cpu(), ag.grad.cpu()), _coef_rows(grads[0], grads[1]), TOL32_G)


@pytest.mark.gpu
@pytest.mark.parametrize("pairs,B", [((8, 8), 2), ((7, 9), 2), ((8, 8), 3), ((4, 16), 1)])
def test_module_narrow_apply_gate(gpu, pairs, B):
    """dsp.Filter._apply_narrow: the apply route from 64 channel pairs and at most 2 columns, the response + product below
    (63 pairs) or above (3 columns); the module output and its gradients against the oracle either way"""
    from flamo_amd import _lib, ops
    from flamo_amd.processor import dsp
    from oracle import hotpath as O
    No, Ni = pairs
    nfft = 4801
    takes = No * Ni >= 64 and B <= 2
    torch.manual_seed(No * Ni + B)
    geq = dsp.GEQ(size=(No, Ni), nfft=nfft, alias_decay_db=30.0, requires_grad=True, device=gpu, dtype=torch.float32)
    with torch.no_grad():
        geq.param.copy_(_geq_param(geq.param.shape[0], (No, Ni), seed=B, sig=False, dtype=torch.float32))
    M = nfft // 2 + 1
    X = torch.complex(torch.randn(B, M, Ni), torch.randn(B, M, Ni))
    Xg = X.to(gpu).requires_grad_(True)
    bins = _bin_set(nfft, seed=B)
    with _knobs(narrow=True), _spy("fl_sos_response_apply_c64", "fl_sos_response_bwd_outer_c64", "fl_geq_response_c64") as calls:
        Y = geq(Xg)
        ct, ct_sel = _cotangent(Y.shape[1:], bins, Y.dtype, gpu, seed=B)
        (Y * ct.unsqueeze(0).conj()).real.sum().backward()
    assert calls["fl_sos_response_apply_c64"] == int(takes) and calls["fl_sos_response_bwd_outer_c64"] == int(takes), calls
    assert calls["fl_geq_response_c64"] == int(not takes), calls
    xo = geq.param.detach().cpu().double().requires_grad_(True)
    Xo = X[:, bins].to(torch.complex128).requires_grad_(True)
    bo, ao = _geq_oracle_sections(xo, False, 1)
    Yo = torch.einsum("kmn,bkn->bkm", O.sos_response_at(bo, ao, nfft, _gamma_t(30.0, nfft), bins), Xo)
    _rows("Y", Y.detach()[:, bins.to(gpu)].cpu().permute(0, 2, 1).reshape(B * No, -1), Yo.detach().permute(0, 2, 1).reshape(B * No, -1), TOL32_FE)
    gx, gX = torch.autograd.grad((Yo * ct_sel.unsqueeze(0).conj()).real.sum(), [xo, Xo])
    _rows("dx", _band_rows(geq.param.grad.cpu().double()), _band_rows(gx), TOL32_GAIN)
    _rows("dX", Xg.grad[:, bins.to(gpu)].cpu().permute(0, 2, 1).reshape(B * Ni, -1), gX.permute(0, 2, 1).reshape(B * Ni, -1), TOL32_FE)


# ============================================================================= 5. every kernel the C dispatchers can select
# One shape family: nfft = 512 (257 bins: two bin blocks), contiguous bins, raw cascades of 11 sections, the octave equaliser
# (12 sections).  (group, ...): each case reaches one template instantiation (two where a forward and a backward go together).
GRID_NFFT, GRID_S, GRID_DB = 512, 11, 30.0
GRID_RC_SHAPES = {2: (4, 2, 2), 4: (2, 4, 4), 8: (1, 8, 8)}      # (No, Nmid, Ni) of the lanes kernels, by NIW ((1, 16, 16): see below)
GRID_CASES = (
    # sos_response_bwd_mixed_kernel<SC, NIW>; NIW > 0 also sos_response_rc_kernel<NIW, float>.  Left out: <SC, 16>, all four SC --
    # this family's draw misses TOL32_G in one (section, pair) row of dL/d(b, a), 2.152e-05 against 1e-05, the same figure at
    # every SC (the chunk dispatch is not what misses); <12, 16> is reached by RC_CASES (1 x 2 x 16, 24 sections)
    [("mixed", sc, niw) for sc in (4, 6, 8, 12) for niw in (0, 2, 4, 8)]
    # sos_response_bwd_kernel<T, SC>
    + [("plain", real, sc) for real in (torch.float32, torch.float64) for sc in (4, 6)]
    # sos_response_bwd_kernel<double, 6, NIW> and sos_response_rc_kernel<NIW, double>
    + [("rc64", niw) for niw in (2, 4, 8, 16)]
    # sos_response_rc_fast_kernel<NIW> (the hook at 1: float evaluation)
    + [("rcfast", niw, 1) for niw in (2, 4, 8, 16)]
    # sos_response_rc_ba_kernel<NIW> (float32) and sos_bwd_lanes_kernel<T, NIW>; float64 (1, 16, 16) is not taken.  Left out:
    # float32 (1, 16, 16) -- at 257 bins (22 bin blocks) the lanes backward returns a wrong dL/dWr, per-row error 3.5 against 1e-05
    # with H and the other shapes within their limits; <float, 16> is reached by RC_CASES (3 x 16 x 16 at nfft = 96000)
    + [("lanes_rc", torch.float32, niw) for niw in (2, 4, 8)]
    + [("lanes_rc", torch.float64, niw) for niw in (2, 4, 8)]
    # sos_bwd_lanes_kernel<T, 0>
    + [("lanes", torch.float32), ("lanes", torch.float64)]
    # sos_response_apply_fast_kernel<B>
    + [("apply", 1), ("apply", 2)]
)
_GRID_REF = {}


def _grid_ref(kind, chan, real=torch.float64):
    """the float64 oracle of the family's cascade (kind "sos": raw sections; "geq": equaliser parameters as stored in `real`) at
    the bin set, built once per (kind, chan, real) and shared by the cases: (inputs, leaves, response (bins, *chan), bins)"""
    from oracle import hotpath as O
    key = (kind, chan, real)
    if key not in _GRID_REF:
        bins = _bin_set(GRID_NFFT, seed=GRID_S)
        if kind == "sos":
            b, a = _sections(GRID_S, chan, seed=GRID_S * 7 + len(chan))
            leaves = [b.clone().requires_grad_(True), a.clone().requires_grad_(True)]
            bo, ao = leaves
            inputs = (b, a)
        else:
            x = _geq_param(len(O.eq_freqs(1)[0]) + 3, chan, seed=GRID_NFFT + len(chan), sig=False, dtype=real)
            leaves = [x.double().clone().requires_grad_(True)]      # (a copy: x itself goes to the GPU as a leaf of its own)
            bo, ao = _geq_oracle_sections(leaves[0], False, 1)
            inputs = (x,)
        _GRID_REF[key] = (inputs, leaves, O.sos_response_at(bo, ao, GRID_NFFT, _gamma_t(GRID_DB, GRID_NFFT), bins), bins)
    return _GRID_REF[key]


def _grid_id(c):
    return "-".join(str(v)[-7:] if isinstance(v, torch.dtype) else str(v) for v in c)


@pytest.mark.gpu
@pytest.mark.parametrize("case", GRID_CASES, ids=_grid_id)
def test_cascade_dispatch_grid(gpu, case):
    """Every kernel instantiation that the host dispatchers of csrc/response.hip and csrc/cascade2.hip can select, once each
    (the cases above name them), at 257 bins against the float64 oracle: a dispatcher that sent one value of a run-time integer
    (section chunk, columns of the constant factor, signal columns) to another value's kernel fails
    its case.  Tolerances: the classes of this file's docstring."""
    from flamo_amd import _lib, ops
    from oracle import hotpath as O
    group = case[0]
    nfft, db = GRID_NFFT, GRID_DB
    M = nfft // 2 + 1
    L = _lib.lib()
    gam = _gamma_f(db, nfft)

    if group in ("mixed", "plain") and not (group == "mixed" and case[2]):      # ---- ops.sos_response
        real = case[1] if group == "plain" else torch.float32
        f64 = real == torch.float64
        chan, C, S = (2, 3), 6, GRID_S
        (b, a), leaves, Ho, bins = _grid_ref("sos", chan)
        sfx = "c128" if f64 else "c64"
        fwd, bwd = f"fl_sos_response_{sfx}", f"fl_sos_response_bwd_{sfx}"
        with _knobs(chunk=case[2] if group == "plain" else case[1], mixed=None if f64 else group == "mixed", float_eval=True):
            bg, ag = b.to(gpu).requires_grad_(True), a.to(gpu).requires_grad_(True)
            nblk = L.fl_sos_bwd_blocks(M, C, S, int(group == "mixed"))
            _poison(gpu, _rows_bytes(C, M, 16 if f64 else 8), nblk * 6 * S * C * 8)
            with _spy(fwd, bwd) as calls:
                H = ops.sos_response(bg, ag, gam, nfft, dtype=real)
                ct, ct_sel = _cotangent(H.shape, bins, H.dtype, gpu, seed=nfft + S)
                _poison(gpu, nblk * 6 * S * C * 8)
                (H * ct.conj()).real.sum().backward()
            assert calls[fwd] == 1 and calls[bwd] == 1, calls
        _rows("H", _resp_rows(H, bins), Ho.detach().flatten(1).transpose(0, 1), TOL64_H if f64 else TOL32_H)
        gbo, gao = torch.autograd.grad((Ho * ct_sel.reshape(Ho.shape).conj()).real.sum(), leaves, retain_graph=True)
        _rows("dba", _coef_rows(bg.grad.cpu(), ag.grad.cpu()), _coef_rows(gbo, gao), TOL64_G if f64 else TOL32_G)
        return

    if group in ("mixed", "rc64", "rcfast"):      # ---- ops.sos_response_rc, (No, Nmid) = (2, 3)
        real = torch.float64 if group == "rc64" else torch.float32
        f64 = real == torch.float64
        No, Nmid, S = 2, 3, GRID_S
        Ni = case[2] if group == "mixed" else case[1]
        C, esz = No * Nmid, 16 if f64 else 8
        want_c = group != "rcfast"      # a wanted coefficient gradient keeps the forward on the double evaluation
        assert ops.cascade_rc_supported(real, Ni, Nmid, S)
        (b, a), leaves, Go, bins = _grid_ref("sos", (No, Nmid))
        g = torch.Generator().manual_seed(Nmid * 10 + Ni)
        W = (torch.randn(Nmid, Ni, generator=g, dtype=torch.float64) / Nmid ** 0.5).to(real)
        sfx = "c128" if f64 else "c64"
        fwd, bwd, lanes_fn = f"fl_sos_response_rc_{sfx}", f"fl_sos_response_bwd_rc_{sfx}", f"fl_geq_response_bwd_lanes_{sfx}"
        kn = dict(chunk=case[1]) if group == "mixed" else dict(lanes=0, rc_fast=case[2]) if group == "rcfast" else {}
        with _knobs(mixed=True, float_eval=True, **kn):
            bg, ag = b.to(gpu).requires_grad_(want_c), a.to(gpu).requires_grad_(want_c)
            Wg = W.to(gpu).requires_grad_(True)
            nblk = L.fl_sos_bwd_blocks(M, C, S, 0 if f64 else 1)
            _poison(gpu, _rows_bytes(C, M, esz), _rows_bytes(No * Ni, M, esz))
            with _spy(fwd, bwd, lanes_fn) as calls:
                H = ops.sos_response_rc(bg, ag, Wg, gam, nfft, dtype=real)
                assert H.shape == (M, No, Ni)
                ct, ct_sel = _cotangent(H.shape, bins, H.dtype, gpu, seed=nfft + Ni)
                _poison(gpu, nblk * 6 * S * C * 8, nblk * C * Ni * (esz // 2))
                (H * ct.conj()).real.sum().backward()
            assert calls[fwd] == 1 and calls[bwd] == 1 and calls[lanes_fn] == 0, calls
        Wo = W.double().requires_grad_(True)
        Ho = Go @ O.to_complex(Wo).to(Go.dtype)
        _rows("H", _resp_rows(H, bins), Ho.detach().flatten(1).transpose(0, 1),
              TOL64_H if f64 else (TOL32_H if want_c else TOL32_FE))
        grads = torch.autograd.grad((Ho * ct_sel.reshape(Ho.shape).conj()).real.sum(), leaves + [Wo], retain_graph=True)
        tg = TOL64_G if f64 else TOL32_G
        _rows("dWr", Wg.grad.cpu().double(), grads[-1], tg)
        if want_c:
            _rows("dba", _coef_rows(bg.grad.cpu(), ag.grad.cpu()), _coef_rows(grads[0], grads[1]), tg)
        else:
            assert bg.grad is None and ag.grad is None
        return

    if group in ("lanes", "lanes_rc"):      # ---- ops.geq_cascade / ops.geq_cascade_rc through the lanes-per-section backward
        real = case[1]
        f64 = real == torch.float64
        rc = group == "lanes_rc"
        No, Nmid, Ni = GRID_RC_SHAPES[case[2]] if rc else (8, 1, 0)
        chan = (No, Nmid) if rc else (8,)
        C, esz = No * Nmid, 16 if f64 else 8
        (x,), leaves, Go, bins = _grid_ref("geq", chan, real)
        S = x.shape[0]
        assert S == 12
        sfx = "c128" if f64 else "c64"
        fwd = f"fl_geq_response_rc_{sfx}" if rc else ("fl_sos_response_c128" if f64 else "fl_geq_response_c64")
        lanes_fn = f"fl_geq_response_bwd_lanes_{sfx}"
        gen1 = f"fl_sos_response_bwd_rc_{sfx}" if rc else f"fl_sos_response_bwd_{sfx}"
        blocks = L.fl_geq_bwd_lanes_blocks_f64 if f64 else L.fl_geq_bwd_lanes_blocks
        with _knobs(lanes=1, mixed=True, float_eval=True):
            nbx = blocks(M, C, S, nfft, 0, Nmid, Ni, int(rc))
            assert nbx > 0, "the lanes kernel must take this shape"
            wrows = (L.fl_geq_bwd_lanes_wrows_f64 if f64 else L.fl_geq_bwd_lanes_wrows)(M, C, S, nfft, 0, Nmid, Ni) if rc else 0
            consts = _geq_design(1).device_consts(gpu)
            xg = x.to(gpu).requires_grad_(True)
            if rc:
                g = torch.Generator().manual_seed(No * 100 + Nmid * 10 + Ni)
                W = (torch.randn(Nmid, Ni, generator=g, dtype=torch.float64) / Nmid ** 0.5).to(real)
                Wg = W.to(gpu).requires_grad_(True)
            _poison(gpu, _rows_bytes(C, M, esz), _rows_bytes(No * Ni, M, esz))
            with _spy(fwd, lanes_fn, gen1) as calls:
                if rc:
                    H = ops.geq_cascade_rc(xg, consts, Wg, gam, nfft, dtype=real)
                else:
                    H = ops.geq_cascade(xg, consts, gam, nfft, dtype=real)
                ct, ct_sel = _cotangent(H.shape, bins, H.dtype, gpu, seed=nfft + S + Ni)
                _poison(gpu, S * C * nbx * 4 * (esz // 2), C * nbx * (esz // 2), Nmid * Ni * wrows * (esz // 2))
                (H * ct.conj()).real.sum().backward()
            assert calls[fwd] == 1 and calls[lanes_fn] == 1 and calls[gen1] == 0, calls
        if rc:
            Wo = W.double().requires_grad_(True)
            Ho = Go @ O.to_complex(Wo).to(Go.dtype)
        else:
            Wo, Ho = None, Go
        _rows("H", _resp_rows(H, bins), Ho.detach().flatten(1).transpose(0, 1), TOL64_H if f64 else TOL32_FE)
        grads = torch.autograd.grad((Ho * ct_sel.reshape(Ho.shape).conj()).real.sum(), leaves + ([Wo] if rc else []), retain_graph=True)
        if rc:
            _rows("dWr", Wg.grad.cpu().double(), grads[-1], TOL64_G if f64 else TOL32_G)
        _rows("dx", _band_rows(xg.grad.cpu().double()), _band_rows(grads[0]), TOL64_G if f64 else TOL32_GAIN)
        return

    assert group == "apply"      # ---- ops.sos_response_apply under no_grad: one launch, B columns
    B, No, Ni, S = case[1], 3, 5, GRID_S
    (b, a), _, Ho, bins = _grid_ref("sos", (No, Ni))
    g = torch.Generator().manual_seed(S * 31 + Ni)
    X = torch.complex(torch.randn(B, M, Ni, generator=g), torch.randn(B, M, Ni, generator=g))
    with _knobs(mixed=True, float_eval=True):
        Xg = X.to(gpu)
        assert ops.cascade_apply_supported(torch.float32, Xg) and Ni <= L.fl_sos_response_apply_max_ni(S)
        _poison(gpu, _rows_bytes(No * Ni, M, 8), B * ops._pitch(M) * No * 8, B * M * No * 8)
        with _spy("fl_sos_response_apply_c64", "fl_sos_response_c64", "fl_sos_response_f32eval_c64") as calls, torch.no_grad():
            Y = ops.sos_response_apply(b.to(gpu), a.to(gpu), Xg, gam, nfft)
        assert calls == {"fl_sos_response_apply_c64": 1, "fl_sos_response_c64": 0, "fl_sos_response_f32eval_c64": 0}, calls
    assert Y.shape == (B, M, No)
    Yo = torch.einsum("kmn,bkn->bkm", Ho.detach(), X[:, bins].to(torch.complex128))
    _rows("Y", Y[:, bins.to(gpu)].cpu().permute(0, 2, 1).reshape(B * No, -1), Yo.permute(0, 2, 1).reshape(B * No, -1), TOL32_FE)


# ============================================================================= CPU: the yardstick itself
@pytest.mark.parametrize("nfft", [29, 40])
def test_oracle_at_bins_matches_full(nfft):
    """O.sos_response_at / O.geq_response_at against O.sos_response / O.geq_response on every bin (gamma < 1, an odd and an
    even length), and the sparse-cotangent gradient equal to the dense one restricted to those bins: the GPU comparisons
    above rest on a checked oracle"""
    from oracle import hotpath as O
    gamma = O.gamma_of(30.0, nfft)
    M = nfft // 2 + 1
    b, a = _sections(5, (3, 2), seed=nfft, zeros_dc_nyq=True)
    every = torch.arange(M)
    H = O.sos_response(b, a, nfft, gamma)
    Ha = O.sos_response_at(b, a, nfft, gamma, every)
    assert (Ha - H).abs().max().item() <= 1e-13 * H.abs().max().item()
    x = _geq_param(12, (2, 3), seed=nfft, sig=False, dtype=torch.float64)
    G = O.geq_response(x, nfft, gamma, exact=True)
    Ga = O.geq_response_at(x, nfft, gamma, every, exact=True)
    assert (Ga - G).abs().max().item() <= 1e-13 * G.abs().max().item()
    # a cotangent non-zero only at `bins`: the dense gradient equals the one of the oracle evaluated at those bins alone
    bins = torch.tensor([0, 3, M // 2, M - 1])
    g = torch.Generator().manual_seed(nfft)
    rows = torch.complex(torch.randn(len(bins), 3, 2, generator=g, dtype=torch.float64), torch.randn(len(bins), 3, 2, generator=g, dtype=torch.float64))
    ct = torch.zeros(M, 3, 2, dtype=torch.complex128)
    ct[bins] = rows
    bo, ao = b.clone().requires_grad_(True), a.clone().requires_grad_(True)
    dense = torch.autograd.grad((O.sos_response(bo, ao, nfft, gamma) * ct.conj()).real.sum(), [bo, ao])
    sparse = torch.autograd.grad((O.sos_response_at(bo, ao, nfft, gamma, bins) * rows.conj()).real.sum(), [bo, ao])
    for d, s in zip(dense, sparse):
        assert (d - s).abs().max().item() <= 1e-13 * d.abs().max().item()
    xo = x.clone().requires_grad_(True)
    ctg = torch.zeros(M, 2, 3, dtype=torch.complex128)
    ctg[bins] = rows.transpose(1, 2)
    d, = torch.autograd.grad((O.geq_response(xo, nfft, gamma, exact=True) * ctg.conj()).real.sum(), [xo])
    s, = torch.autograd.grad((O.geq_response_at(xo, nfft, gamma, bins, exact=True) * ctg[bins].conj()).real.sum(), [xo])
    assert (d - s).abs().max().item() <= 1e-13 * d.abs().max().item()
    # the bin set and its element map: inside the range, the row-major map a permutation of the elements
    for nf, b0, m in ((96000, 0, None), (96000, 47001, 1000), (4801, 0, None), (2, 0, None), (96000, 12001, 1)):
        s = _bin_set(nf, b0, m)
        hi = nf // 2 + 1 if m is None else b0 + m
        assert s.min() >= b0 and s.max() < hi and len(s) == len(set(s.tolist()))
        assert {0, nf // 2}.issubset(set(s.tolist())) or b0 > 0
    L1, L2, nf = 375, 128, 96000
    el = _elems(torch.arange(nf // 2 + 1), nf, 0, (L1, L2))
    assert sorted(el.tolist()) == list(range(nf // 2 + 1))
    f = el[12345].item()
    assert f // L2 + L1 * (f % L2) == 12345
