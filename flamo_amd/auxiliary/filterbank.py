"""``FilterBank`` of the reference (flamo/auxiliary/filterbank.py:12-325): a Butterworth octave / third-octave bank applied in
the frequency domain -- one real transform, a product per band, one inverse real transform per band -- "useful, e.g., to get
the decay curves of RIRs".  The band filters are designed here (analogue prototype, band transform, bilinear transform with
pre-warping, float64 numpy): the package needs no scipy."""
import numpy as np
import torch
from torch import nn

from .. import ops

NOM_FREQ_F1 = (16, 31.5, 63, 125, 250, 500, 1000, 2000, 4000, 8000, 16000, 32000)
NOM_FREQ_F3 = (16, 20, 25, 31.5, 40, 50, 63, 80, 100, 125, 160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500,
               3150, 4000, 5000, 6300, 8000, 10000, 12500, 16000, 20000, 25000, 32000)


def butter_zpk(order, edges, btype, fs):
    """Digital Butterworth filter of ``order`` as (1 - z_i, 1 - p_i, gain), H(z) = gain prod (z - z_i) / prod (z - p_i), float64.
    ``btype`` "lowpass" / "highpass" with one edge frequency, "bandpass" with two, in the unit of ``fs``.  The analogue
    prototype (poles -exp(i pi m / 2n), m = -n+1, -n+3, ..., n-1) is moved to the pre-warped edges 4 tan(pi f / fs) and through
    the bilinear transform z = (4 + s) / (4 - s).  The roots are returned about z = 1, where the low bands' poles crowd:
    1 - (4 + s) / (4 - s) = -2 s / (4 - s) is formed without the cancellation of 1 - p."""
    n = int(order)
    if n < 1:
        raise ValueError(f"the filter order must be at least 1, got {order!r}")
    w = 4.0 * np.tan(np.pi * np.asarray(edges, dtype=np.float64) / fs)
    m = np.arange(-n + 1, n, 2)
    p = -np.exp(1j * np.pi * m / (2 * n))
    if btype == "lowpass":
        z, p, k = np.zeros(0, dtype=complex), w[0] * p, w[0] ** n
    elif btype == "highpass":
        z, p, k = np.zeros(n, dtype=complex), w[0] / p, 1.0
    else:
        bw, wo = w[1] - w[0], np.sqrt(w[0] * w[1])
        lp = p * bw / 2
        root = np.sqrt(lp * lp - wo * wo)
        z, p, k = np.zeros(n, dtype=complex), np.concatenate([lp + root, lp - root]), bw ** n
    gain = k * np.real(np.prod(4.0 - z) / np.prod(4.0 - p))
    one_minus_z = np.concatenate([-2.0 * z / (4.0 - z), np.full(len(p) - len(z), 2.0, dtype=complex)])      # the rest at z = -1
    one_minus_p = -2.0 * p / (4.0 - p)
    return one_minus_z, one_minus_p, float(gain)


class FilterBank(nn.Module):
    r"""Octave (``fraction=1``) or third-octave (``fraction=3``) Butterworth filter bank applied in the frequency domain, after
    the reference's class of the same name: same constructor, methods and attributes.

    **Centres.**  The nominal frequencies between ``fmin`` and ``fmax``, selected by the reference's rule as written: the list
    ends before the first nominal frequency above ``fmax``, and it starts at the first nominal frequency that ``fmin`` EXCEEDS
    (octaves) or at the one after it (third octaves).  The lists begin at 16 Hz, so ``fmin=20, fmax=18000`` gives 16 ... 16000
    Hz (11 bands) and 20 ... 16000 Hz (30 bands) -- and so does ``fmin=60``: the search stops at its first hit, 16 Hz.  Other
    fractions are refused as in the reference.  ``set_center_frequencies`` takes any frequencies in [0, fs / 2]; they are
    sorted, and the sorted list is the one the filters are designed from.

    **Design.**  Per centre fc a Butterworth band-pass of ``order`` over fc / sqrt 2 ... fc sqrt 2; a centre of exactly 0 a
    low-pass at the next centre / sqrt 2, a centre of exactly fs / 2 a high-pass at sqrt 2 times the previous one
    (``butter_zpk``, float64, no scipy).  A band edge at or above fs / 2 is a ValueError that names the band.

    **Grid.**  ``x`` (B, T, N) is transformed along time at its own length, and bin k of the M = T // 2 + 1 bins is multiplied
    by the band's response at w_k = pi k / M, k = 0 ... M - 1 -- M samples of [0, pi), what ``sosfreqz(sos, worN=M)`` returns in
    the reference -- NOT at the bin's own frequency 2 pi k / T.  The inverse transform has length T' = 2 (T // 2): the result is
    (B, T', N, K), bands last, a circular convolution.

    **Backend.**  ``backend="torch"`` runs; the default ``"scipy"`` ends in NotImplementedError, as the reference's ``forward``
    does (its ``if ... if ... else: raise`` falls through after the scipy branch).

    Two deliberate differences: the output has the INPUT's dtype (the reference returns float64 for a float32 input, promoted
    by its complex128 responses), and with ``nfft=None`` the grid is sized on every call (the reference fixes ``_nfft`` at its
    first call and fails on a second signal length); a given ``nfft`` other than T // 2 + 1 is a ValueError.

    Device float32 / float64 (B, T, N) tensors run on ``ops.filterbank`` (the library's real transforms around one band-split
    launch; the responses are evaluated inside the kernel and never stored); host tensors and everything else take the torch
    lines of ``_torch_forward``."""

    def __init__(self, fraction: int = 3, order: int = 5, fmin: float = 20.0, fmax: float = 18000.0, sample_rate: int = 48000,
                 nfft: int = None, backend: str = "scipy"):
        super().__init__()
        assert (fraction == 1) | (fraction == 3), "At the moment only fractions 1 and 3 are supported"
        nominal = NOM_FREQ_F1 if fraction == 1 else NOM_FREQ_F3
        index = [0, len(nominal)]
        for i, f in enumerate(nominal):
            if fmin > f:
                index[0] = i if fraction == 1 else i + 1
                break
        for i, f in enumerate(nominal):
            if f > fmax:
                index[1] = i
                break
        self._center_frequencies = list(nominal[index[0]:index[1]])
        self._order = order
        self._sample_rate = sample_rate
        self._backend = backend
        self._nfft = nfft
        self._design()

    # ------------------------------------------------------------------ design
    def _design(self):
        """the bands' (1 - z_i, 1 - p_i, gain) from the centres, the order and the sample rate; every cache is dropped"""
        self._zpk = self._get_octave_filters(self._center_frequencies, self._sample_rate, self._order)
        self._state = getattr(self, "_state", 0) + 1
        self._packed = None
        self._device_consts = {}
        self._responses = {}
        self._response_tensors = {}

    @staticmethod
    def _get_octave_filters(center_freqs, fs, order):
        """one ``butter_zpk`` design per centre frequency"""
        bands = []
        for i, fc in enumerate(center_freqs):
            if abs(fc) < 1e-6:
                if i + 1 >= len(center_freqs):
                    raise ValueError("a centre of 0 Hz (low-pass band) needs a centre above it")
                edges, btype = [(1 / np.sqrt(2)) * center_freqs[i + 1]], "lowpass"
            elif abs(fc - fs / 2) < 1e-6:
                if i == 0:
                    raise ValueError("a centre of fs / 2 (high-pass band) needs a centre below it")
                edges, btype = [np.sqrt(2) * center_freqs[i - 1]], "highpass"
            else:
                edges, btype = [fc / np.sqrt(2), fc * np.sqrt(2)], "bandpass"
            if not (0 < min(edges) and max(edges) < fs / 2):
                raise ValueError(f"band {i} ({fc:g} Hz, {btype}): its edges {', '.join(f'{e:g}' for e in edges)} Hz must lie "
                                 f"inside (0, fs / 2 = {fs / 2:g} Hz)")
            bands.append(butter_zpk(order, edges, btype, fs))
        return bands

    def set_sample_rate(self, sample_rate):
        """Sets the sample rate and updates the filters."""
        self._sample_rate = sample_rate
        self._design()

    def set_order(self, order):
        """Sets the filter order and updates the filters."""
        self._order = order
        self._design()

    def set_center_frequencies(self, center_freqs):
        """Sets the center frequencies (sorted) and updates the filters."""
        center_freqs_np = np.asarray(center_freqs, dtype=np.float64)
        assert not np.any(center_freqs_np < 0) and not np.any(center_freqs_np > self._sample_rate / 2), (
            "Center Frequencies must be greater than 0 and smaller than fs/2. Exceptions: exactly 0 or fs/2 "
            "will give lowpass or highpass bands")
        self._center_frequencies = np.sort(center_freqs_np).tolist()
        self._design()

    def get_center_frequencies(self):
        """Gets the center frequencies."""
        return self._center_frequencies

    # ------------------------------------------------------------------ what ops.filterbank reads
    def band_constants(self):
        """(state, K, most zeros or poles of a band, records): the bands as the float64 records of
        include/flamo_hip_filterbank.h -- per band the two counts, the gain, one unused entry, then 16 pairs (re, im) of
        1 - z_i and 16 pairs of 1 - p_i -- or records None when a band has more than 16 of either"""
        if self._packed is None:
            K, P = len(self._zpk), ops.FILTERBANK_MAX_ROOTS
            most = max([max(len(z), len(p)) for z, p, _ in self._zpk], default=0)
            rec = None
            if most <= P:
                rec = np.zeros((K, 4 + 4 * P), dtype=np.float64)
                for j, (z, p, g) in enumerate(self._zpk):
                    rec[j, :3] = len(z), len(p), g
                    rec[j, 4:4 + 2 * len(z)] = np.stack([z.real, z.imag], axis=-1).ravel()
                    rec[j, 4 + 2 * P:4 + 2 * P + 2 * len(p)] = np.stack([p.real, p.imag], axis=-1).ravel()
            self._packed = (self._state, K, most, rec)
        return self._packed

    # ------------------------------------------------------------------ responses and the torch lines
    def freq_response(self, M):
        """(K, M) complex128 numpy: the bands' responses at w_k = pi k / M, k < M, from the zeros and poles about z = 1:
        u = z - 1 = -2 sin^2(w / 2) + i sin w, H = g prod (u + (1 - z_i)) / prod (u + (1 - p_i))"""
        M = int(M)
        H = self._responses.get(M)
        if H is None:
            w = np.pi * np.arange(M, dtype=np.float64) / M
            u = -2.0 * np.sin(w / 2) ** 2 + 1j * np.sin(w)
            H = np.empty((len(self._zpk), M), dtype=np.complex128)
            for j, (z, p, g) in enumerate(self._zpk):
                num, den = np.full(M, g, dtype=np.complex128), np.ones(M, dtype=np.complex128)
                for c in z:
                    num = num * (u + c)
                for d in p:
                    den = den * (u + d)
                H[j] = num / den
            self._responses = {M: H}          # (one grid is kept: the signal length of a fit does not change)
        return H

    def _torch_forward(self, x):
        """the bank in plain torch on whatever device ``x`` lives: rfft, the product with the responses, irfft"""
        M = x.shape[1] // 2 + 1
        cplx = torch.complex64 if x.dtype == torch.float32 else torch.complex128
        key = (M, x.device, cplx)
        H = self._response_tensors.get(key)
        if H is None:          # (kept for the last grid, as the host array is: a fit calls with one length)
            H = torch.from_numpy(self.freq_response(M)).to(device=x.device, dtype=cplx)
            self._response_tensors = {key: H}
        X = torch.fft.rfft(x, dim=1)
        return torch.fft.irfft(X.unsqueeze(-1) * H.transpose(0, 1)[None, :, None, :], dim=1)

    def forward(self, x):
        """(B, T, N) -> (B, 2 (T // 2), N, K): the band signals, bands last"""
        if self._backend != "torch":
            raise NotImplementedError("No good implementation relying solely on the pytorch backend has been found yet"
                                      if self._backend == "scipy" else f"FilterBank: unknown backend {self._backend!r}")
        if x.dim() != 3:
            raise ValueError(f"FilterBank: a (B, T, N) signal, got {tuple(x.shape)}")
        M = x.shape[1] // 2 + 1
        if self._nfft is not None and self._nfft != M:
            raise ValueError(f"FilterBank: nfft = {self._nfft} but a signal of {x.shape[1]} samples has {M} bins "
                             f"(nfft is T // 2 + 1, or None to size the grid on every call)")
        if x.is_cuda and x.dtype in (torch.float32, torch.float64) and x.numel() > 0 and ops.filterbank_supported(self):
            return ops.filterbank(x, self)
        return self._torch_forward(x)

    def get_filterbank_impulse_response(self):
        """the band signals (1, 20 fs, 1, K) of a unit impulse at one second in 20 seconds of silence"""
        impulse = torch.zeros(1, self._sample_rate * 20, 1)
        impulse[0, self._sample_rate, 0] = 1
        return self.forward(impulse)
