"""auxiliary.filterbank.FilterBank on the host: its surface against the reference's, its torch lines against the reference's
recorded responses and outputs (tests/golden/filterbank_*.npz, tools/gen_golden_filterbank.py) and against a statement of the
definition written here -- a Butterworth design of this file's own (extended precision, the gain from the pass band's centre
instead of the transforms' gain rules) and the plain zero-pole form on the grid w_k = pi k / M.  The GPU tests share the
statement (test_filterbank_gpu.py, test_subband_edc_*.py)."""
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, check_close

LD, CLD = np.longdouble, np.clongdouble
REFERENCE_SIGNATURE = [("fraction", 3), ("order", 5), ("fmin", 20.0), ("fmax", 18000.0), ("sample_rate", 48000), ("nfft", None),
                       ("backend", "scipy")]
OCTAVE = [16, 31.5, 63, 125, 250, 500, 1000, 2000, 4000, 8000, 16000]
THIRD = [20, 25, 31.5, 40, 50, 63, 80, 100, 125, 160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000,
         5000, 6300, 8000, 10000, 12500, 16000]


# ----------------------------------------------------------------------------- the statement
def statement_zpk(order, edges, btype, fs):
    """(zeros, poles, gain) of the digital Butterworth filter, extended precision: prototype poles exp(i pi (2 m + n + 1) / 2n),
    edges pre-warped to 2 tan(pi f / fs), s = 2 (z - 1) / (z + 1); the gain makes |H| = 1 at DC (low-pass), at Nyquist
    (high-pass) or at the image of the analogue centre sqrt(w1 w2) (band-pass), where a Butterworth filter is exactly 1."""
    n = int(order)
    pi = LD(np.pi) + LD(1.2246467991473532e-16)          # pi to extended precision
    w = [2 * np.tan(pi * LD(f) / LD(fs)) for f in edges]
    proto = np.exp(1j * (pi * (2 * np.arange(n, dtype=LD) + n + 1) / (2 * n))).astype(CLD)
    if btype == "lowpass":
        s_z, s_p, at = np.zeros(0, CLD), w[0] * proto, CLD(1)
    elif btype == "highpass":
        s_z, s_p, at = np.zeros(n, CLD), w[0] / proto, CLD(-1)
    else:
        bw, w0 = w[1] - w[0], np.sqrt(w[0] * w[1])
        half = proto * bw / 2
        root = np.sqrt(half * half - w0 * w0)
        s_z, s_p = np.zeros(n, CLD), np.concatenate([half + root, half - root])
        at = (2 + 1j * w0) / (2 - 1j * w0)
    z = np.concatenate([(2 + s_z) / (2 - s_z), -np.ones(len(s_p) - len(s_z), CLD)])
    p = (2 + s_p) / (2 - s_p)
    gain = 1 / np.abs(np.prod(at - z) / np.prod(at - p))
    return z, p, gain


def statement_bands(centers, order, fs):
    """the reference's rule: a band-pass over fc / sqrt 2 ... fc sqrt 2; fc = 0 a low-pass at next / sqrt 2; fc = fs / 2 a
    high-pass at sqrt 2 previous"""
    r2 = np.sqrt(LD(2))
    out = []
    for i, fc in enumerate(centers):
        if fc == 0:
            out.append(statement_zpk(order, [LD(centers[i + 1]) / r2], "lowpass", fs))
        elif fc == fs / 2:
            out.append(statement_zpk(order, [LD(centers[i - 1]) * r2], "highpass", fs))
        else:
            out.append(statement_zpk(order, [LD(fc) / r2, LD(fc) * r2], "bandpass", fs))
    return out


def statement_responses(centers, order, fs, M):
    """(K, M) complex128: H_j = g prod (z - z_i) / prod (z - p_i) at z = exp(i pi k / M), k < M, in extended precision"""
    pi = LD(np.pi) + LD(1.2246467991473532e-16)
    zz = np.exp(1j * (pi * np.arange(M, dtype=LD) / M)).astype(CLD)
    H = np.empty((len(centers), M), dtype=np.complex128)
    for j, (z, p, g) in enumerate(statement_bands(centers, order, fs)):
        num, den = np.full(M, g, dtype=CLD), np.ones(M, dtype=CLD)
        for zi in z:
            num = num * (zz - zi)
        for pi_ in p:
            den = den * (zz - pi_)
        H[j] = (num / den).astype(np.complex128)
    return H


def statement_bank(x, H):
    """the band signals (B, 2 (T // 2), N, K) of x (B, T, N) in x's precision: bin k of rfft(x) times H[j, k], irfft per band"""
    Ht = torch.from_numpy(H).to(torch.complex64 if x.dtype == torch.float32 else torch.complex128)
    X = torch.fft.rfft(x, dim=1)
    return torch.stack([torch.fft.irfft(X * Ht[j][None, :, None], n=2 * (x.shape[1] // 2), dim=1) for j in range(H.shape[0])], dim=-1)


def decaying_noise(shape, seed, c):
    """randn exp(-6.9 c t / T), float64"""
    B, T, N = shape
    gen = torch.Generator().manual_seed(seed)
    t = torch.arange(T, dtype=torch.float64)[None, :, None]
    return torch.randn(B, T, N, dtype=torch.float64, generator=gen) * torch.exp(-6.9 * c * t / T)


def make_bank(fraction=1, order=5, centers=None, **kw):
    from flamo_amd.auxiliary import FilterBank
    bank = FilterBank(fraction=fraction, order=order, backend="torch", **kw)
    if centers is not None:
        bank.set_center_frequencies(centers)
    return bank


# ----------------------------------------------------------------------------- surface
def test_constructor_signature_is_the_references():
    from flamo_amd.auxiliary import FilterBank
    params = list(inspect.signature(FilterBank.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == REFERENCE_SIGNATURE


def test_lazy_table_of_the_package():
    from flamo_amd import auxiliary
    assert auxiliary.FilterBank is auxiliary.filterbank.FilterBank
    assert "FilterBank" in dir(auxiliary) and "filterbank" in dir(auxiliary) and "reverb" in dir(auxiliary)
    with pytest.raises(AttributeError):
        auxiliary.no_such_name


def test_no_scipy_in_the_module():
    from flamo_amd.auxiliary import filterbank
    with open(filterbank.__file__) as f:
        assert re.search(r"^\s*(import|from)\s+scipy", f.read(), re.M) is None


@pytest.mark.parametrize("kw, expect", [
    (dict(fraction=1), OCTAVE),
    (dict(fraction=3), THIRD),
    (dict(), THIRD),
    (dict(fraction=1, fmin=60.0), OCTAVE),          # the first loop stops at 16 Hz, the first nominal frequency under fmin
    (dict(fraction=3, fmin=60.0), THIRD),
    (dict(fraction=1, fmax=1000.0), OCTAVE[:7]),
    (dict(fraction=3, fmin=10.0, fmax=100.0), [16] + THIRD[:8]),
])
def test_centres(kw, expect):
    from flamo_amd.auxiliary import FilterBank
    bank = FilterBank(**kw)
    assert bank.get_center_frequencies() == expect and bank._center_frequencies == expect
    assert (bank._order, bank._sample_rate, bank._nfft, bank._backend) == (5, 48000, None, "scipy")


def test_other_fractions_are_refused():
    from flamo_amd.auxiliary import FilterBank
    with pytest.raises(AssertionError, match="fractions 1 and 3"):
        FilterBank(fraction=2)


def test_setters():
    bank = make_bank(1)
    H0 = bank.freq_response(241).copy()
    bank.set_order(3)
    assert bank._order == 3 and len(bank._zpk[0][1]) == 6
    assert np.abs(bank.freq_response(241) - H0).max() > 1e-3
    np.testing.assert_allclose(bank.freq_response(241), statement_responses(OCTAVE, 3, 48000, 241), rtol=0, atol=1e-11)
    bank.set_sample_rate(96000)
    assert bank._sample_rate == 96000
    np.testing.assert_allclose(bank.freq_response(100), statement_responses(OCTAVE, 3, 96000, 100), rtol=0, atol=1e-11)
    bank.set_center_frequencies([4000, 250, 1000])
    assert bank.get_center_frequencies() == [250.0, 1000.0, 4000.0]
    np.testing.assert_allclose(bank.freq_response(100), statement_responses([250, 1000, 4000], 3, 96000, 100), rtol=0, atol=1e-11)
    with pytest.raises(AssertionError, match="Center Frequencies"):
        bank.set_center_frequencies([100, 50000])
    with pytest.raises(AssertionError, match="Center Frequencies"):
        bank.set_center_frequencies([-1, 100])
    state, K, most, rec = bank.band_constants()
    assert K == 3 and most == 6 and rec.shape == (3, 68) and rec.dtype == np.float64
    bank.set_order(9)
    assert bank.band_constants()[0] != state and bank.band_constants()[2] == 18 and bank.band_constants()[3] is None


def test_refusals():
    from flamo_amd.auxiliary import FilterBank
    x = torch.randn(1, 480, 2, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="pytorch backend"):
        FilterBank()(x)                                             # backend="scipy", the default
    with pytest.raises(ValueError, match="nfft = 100"):
        FilterBank(fraction=1, backend="torch", nfft=100)(x)
    assert FilterBank(fraction=1, backend="torch", nfft=241)(x).shape == (1, 480, 2, 11)
    with pytest.raises(ValueError, match=r"band 10 \(16000 Hz"):
        FilterBank(fraction=1, sample_rate=40000)                   # 16000 sqrt 2 is beyond 20000 = fs / 2
    with pytest.raises(ValueError, match="band 1"):
        make_bank(1).set_center_frequencies([1000, 20000])          # 20000 sqrt 2 > 24000
    with pytest.raises(ValueError, match=r"\(B, T, N\)"):
        make_bank(1)(torch.randn(480))


# ----------------------------------------------------------------------------- the reference's fixtures
FIXTURES = ("filterbank_octave", "filterbank_third", "filterbank_lowhigh")


def load_fixture(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    assert meta["module"] == "FilterBank"
    return meta, {k: z[k] for k in z.files if k != "meta"}


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_of_the_reference(name):
    """responses and outputs of the class's float64 torch lines against the reference's own, limit 1e-9 of the largest |y| (of
    the largest |H| for the responses): 8 times what scipy's zero-pole form and its sosfreqz differ by.  Achieved: responses
    4.4e-12 (octave, third), 5.0e-14 (low / high); outputs 2.4e-13, 1.2e-13, 3.5e-15."""
    meta, a = load_fixture(name)
    assert a["freqz"].nbytes + a["y"].nbytes + a["x"].nbytes < 680_000
    bank = make_bank(meta["fraction"], meta["order"], meta["set_centers"], sample_rate=meta["sample_rate"])
    assert bank.get_center_frequencies() == a["centers"].tolist()
    x = torch.from_numpy(a["x"])
    H = bank.freq_response(x.shape[1] // 2 + 1)
    eH = np.abs(H - a["freqz"]).max() / np.abs(a["freqz"]).max()
    y = bank(x)
    assert tuple(y.shape) == a["y"].shape and y.dtype == torch.float64
    ey = np.abs(y.numpy() - a["y"]).max() / np.abs(a["y"]).max()
    print(f"[parity] {name}: responses {eH:.3e}  outputs {ey:.3e}  (limit 1e-9)")
    assert eH < 1e-9 and ey < 1e-9
    # ... and the statement itself stands as close to them
    Hs = statement_responses(a["centers"].tolist(), meta["order"], meta["sample_rate"], x.shape[1] // 2 + 1)
    assert np.abs(Hs - a["freqz"]).max() / np.abs(a["freqz"]).max() < 1e-9


# ----------------------------------------------------------------------------- the statement
def test_statement_design_against_scipy():
    signal = pytest.importorskip("scipy.signal")
    for order in (1, 2, 5, 8):
        for btype, edges in (("lowpass", [707.1]), ("highpass", [1414.2]), ("bandpass", [16 / np.sqrt(2), 16 * np.sqrt(2)]),
                             ("bandpass", [16000 / np.sqrt(2), 16000 * np.sqrt(2)])):
            z, p, k = signal.butter(order, edges if len(edges) > 1 else edges[0], btype=btype, fs=48000, output="zpk")
            zs, ps, gs = statement_zpk(order, edges, btype, 48000)
            assert len(zs) == len(z) and len(ps) == len(p)
            assert np.abs(np.sort(zs.real.astype(float)) - np.sort(z.real)).max() < 1e-12 and np.abs(zs.imag).max() == 0
            # every pole of one has a pole of the other within 2e-14 (scipy's float64 rounding), and the gains agree
            d = np.abs(ps.astype(complex)[:, None] - p[None, :])
            assert d.min(axis=1).max() < 2e-14 and d.min(axis=0).max() < 2e-14
            assert abs(float(gs) - k) < 1e-12 * abs(k)


# (shape, fraction, order, centres handed to set_center_frequencies)
STATEMENT_CASES = [
    ((2, 960, 3), 1, 5, None),
    ((2, 960, 3), 3, 2, None),
    ((1, 961, 2), 3, 8, None),
    ((1, 4800, 1), 3, 5, None),
    ((1, 961, 2), 1, 5, [0, 1000, 24000]),
]


@pytest.mark.parametrize("shape, fraction, order, centers", STATEMENT_CASES)
def test_torch_lines_against_the_statement(shape, fraction, order, centers):
    """the class's float64 lines against the statement, output and gradient, at the project's float64 limit 1e-10.
    Achieved: 5.4e-16 ... 3.4e-15 (l2), max-norm <= 4.2e-15."""
    bank = make_bank(fraction, order, centers)
    M = shape[1] // 2 + 1
    Hs = statement_responses(bank.get_center_frequencies(), order, 48000, M)
    assert np.abs(bank.freq_response(M) - Hs).max() < 1e-10
    x = decaying_noise(shape, 3, 1.0).requires_grad_(True)
    y = bank(x)
    ref = statement_bank(x, Hs)
    assert tuple(y.shape) == (shape[0], 2 * (shape[1] // 2), shape[2], len(Hs)) and y.dtype == torch.float64
    tag = f"filterbank_host/{'x'.join(map(str, shape))}_{len(Hs)}_{order}"
    check_close(tag + "/y", y.detach(), ref.detach(), 1e-10)
    C = 3.0 * torch.randn(y.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    (g,) = torch.autograd.grad(y, [x], C)
    (gr,) = torch.autograd.grad(ref, [x], C)
    check_close(tag + "/grad", g, gr, 1e-10)


def test_output_dtype_and_a_grid_per_call():
    """the two deliberate differences: a float32 input gives a float32 output, and a bank without nfft takes a second length"""
    bank = make_bank(1)
    x = decaying_noise((1, 480, 2), 5, 1.0)
    y32 = bank(x.float())
    assert y32.dtype == torch.float32 and bank._nfft is None
    assert (y32.double() - bank(x)).abs().max() < 1e-5
    assert bank(decaying_noise((1, 300, 1), 6, 1.0)).shape == (1, 300, 1, 11)


def test_impulse_response_of_the_bank():
    bank = make_bank(1, fmax=500.0, sample_rate=2000)
    ir = bank.get_filterbank_impulse_response()
    assert tuple(ir.shape) == (1, 40000, 1, 6) and ir.dtype == torch.float32
    impulse = torch.zeros(1, 40000, 1, dtype=torch.float64)
    impulse[0, 2000, 0] = 1
    Hs = statement_responses(bank.get_center_frequencies(), 5, 2000, 20001)
    assert (ir.double() - statement_bank(impulse, Hs)).abs().max() < 1e-5 * ir.abs().max()      # float32 against float64
    from flamo_amd.auxiliary import FilterBank
    with pytest.raises(NotImplementedError):
        FilterBank(fraction=1, fmax=500.0, sample_rate=2000).get_filterbank_impulse_response()
