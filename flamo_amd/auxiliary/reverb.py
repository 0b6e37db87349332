"""Feedback-delay-network builder and delay-scaled attenuation filters (flamo/auxiliary/reverb.py).

The attenuation filters in the feedback path of an FDN take reverberation times in seconds: line n, d[n] samples long, is
attenuated by -60 d[n] / (rt fs) dB per pass, so that every line decays by 60 dB in rt seconds.  Three classes, one cascade
per delay line each (``_diag``):

* ``parallelFDNGEQ``              a graphic equaliser per line, trainable (reverb.py:459-552)
* ``parallelFirstOrderShelving``  a first-order shelving filter per line, trainable (reverb.py:808-887)
* ``parallelFDNAccurateGEQ``      the fitted equaliser per line, not learnable (reverb.py:303-391)

On a device parameter under the class's own map the two trainable ones design their sections in one launch
(``ops.FdnAttenuation``, csrc/fdnatt.hip) and evaluate them by the cascade kernels every second-order-section class uses;
the gradient is the cascade backward and one design-backward launch.  The reference loops over the lines in Python.  A
user-assigned ``map`` (or ``fold_map=False``) takes the same mathematics as torch ops in front of the cascade kernels.  Host tensors
take the float64 torch lines below, which are also what the tests measure the kernels against.

``HomogeneousFDN`` (reverb.py:83-300) assembles the canonical FDN from any object with the attributes of the reference's
``HomogeneousFDNConfig``.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Optional

import numpy as np
import torch

from .. import ops
from ..functional import GEQDesign
from ..processor import dsp, system


# ----------------------------------------------------------------------------- helpers (reverb.py:17-81)
def rt2slope(rt60: torch.Tensor, fs: int):
    """Time in seconds of a 60 dB decay -> decay slope in dB per sample (reverb.py:17-21)."""
    return -60 / (rt60 * fs)


def rt2absorption(rt60: torch.Tensor, fs: int, delays_len: torch.Tensor):
    """... -> attenuation in dB of every delay line, (len(rt60), len(delays_len)) (reverb.py:24-29)."""
    slope = rt2slope(rt60, fs)
    return torch.einsum("i,j->ij", slope, delays_len)


class map_gamma(torch.nn.Module):
    """Gain per sample -> gain per delay line: sigmoid(x[0]) compressed into [0.99, 1], to the power of the line's length
    (reverb.py:31-46)."""

    def __init__(self, delays, is_compressed=True):
        super().__init__()
        self.delays = delays
        self.is_compressed = is_compressed
        self.g_min = 0.99
        self.g_max = 1.0

    def forward(self, x):
        # (the power is formed in float64 whatever the module's dtype: a float32 base under an exponent of a few hundred
        # samples would cost 1e-5 of the line's gain)
        delays = self.delays.to(x.device) if torch.is_tensor(self.delays) else self.delays
        x0 = x[0].double()
        if self.is_compressed:
            x0 = torch.sigmoid(x0) * (self.g_max - self.g_min) + self.g_min
        return (x0 ** delays).to(x.dtype)


class inverse_map_gamma(torch.nn.Module):
    """The inverse of ``map_gamma`` (of its compression alone when no delays are given) (reverb.py:48-69)."""

    def __init__(self, delays=None, is_compressed=True):
        super().__init__()
        self.delays = delays
        self.is_compressed = is_compressed
        self.g_min = 0.99
        self.g_max = 1.0

    def forward(self, y):
        delays = self.delays.to(y.device) if torch.is_tensor(self.delays) else self.delays
        if delays is not None:
            y = y ** (1 / delays)
        if not self.is_compressed:
            return y
        sig = (y - self.g_min) / (self.g_max - self.g_min)
        return torch.log(sig / (1 - sig))


class map_gfdn_gamma(torch.nn.Module):
    """Grouped reverberation times -> attenuation in dB per line (reverb.py:71-81)."""

    def __init__(self, delays: torch.Tensor, n_groups: int, fs: int):
        super().__init__()
        self.delays = delays
        self.n_groups = n_groups
        self.fs = fs

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return torch.mul(rt2slope(x, self.fs).unsqueeze(-1), self.delays.to(x.device).unsqueeze(0))


# ----------------------------------------------------------------------------- the designs as float64 torch lines
# What csrc/fdnatt.hip computes, written once: host tensors run these, and the tests hold the kernels to them.  VALUES carry the
# float32 roundings of the reference's float32 section buffers; the autograd graph behind them is the unrounded formulas
# (value = exact + (rounded - exact).detach()), which is the gradient the design kernels' backward computes.
def _f32(x):
    return x.to(torch.float32).to(torch.float64)


def _exact(x):
    return x


def _straight_through(fn, *args):
    exact = fn(_exact, *args)
    with torch.no_grad():
        rounded = fn(_f32, *(a.detach() if torch.is_tensor(a) else a for a in args))
    return tuple(e + (r - e).detach() for e, r in zip(exact, rounded))


def fdn_gain_db(rt: torch.Tensor, delays: torch.Tensor, fs) -> torch.Tensor:
    """rt (n_bands,) seconds, delays (N,) samples -> command gains in dB (n_bands, N): (-60 / (rt fs)) d"""
    return rt2slope(rt, fs).unsqueeze(-1) * delays.unsqueeze(0)


def _geq_taps(r, g, design: GEQDesign):
    """Sections of the graphic equaliser per line from linear gains g (n_bands, N), rounded by r where the reference stores
    into float32 buffers.  reverb.py:523-524 hands eq.geq one-element gain VECTORS (dsp.GEQ hands it scalars), and type promotion
    then keeps the shelves' whole-vector scalings g^(1/2) b and a g (functional.py:615-619) in float64: their products are
    rounded once, where GEQDesign.sections multiplies float32 values.  A float32 ulp in a shelf's tap is 2e-3 of the response
    near DC (b0 + b1 + b2 cancels), so the rounding points are those of THIS class."""
    nb = design.n_bands
    one, zero = torch.ones_like(g[0]), torch.zeros_like(g[0])
    b = [torch.stack([r(g[0]), zero, zero])]
    a = [torch.stack([one, zero, zero])]

    _, sh_t2, sh_st, pk_t, pk_c = design._consts(g.device)

    def shelf(gs, i):
        t2, st = sh_t2[i], sh_st[i]
        u, q = gs ** 0.5, gs ** 0.25
        p = r(torch.stack([u * t2 + st * q + 1, 2 * u * t2 - 2, u * t2 - st * q + 1]))
        d = r(torch.stack([u + st * q + t2, 2 * t2 - 2 * u, u - st * q + t2]))
        return r(u * p), d

    b_lo, a_lo = shelf(g[1], 0)
    s_hi, d_hi = shelf(g[nb - 1], 1)
    gp = g[2:nb - 1]
    t, c = pk_t.unsqueeze(-1), pk_c.unsqueeze(-1)
    sg = torch.sqrt(gp)
    bp = r(torch.stack([sg + gp * t, -2 * sg * c, sg - gp * t]))
    ap = r(torch.stack([sg + t, -2 * sg * c, sg - t]))
    b += [b_lo] + list(bp.unbind(1)) + [r(d_hi * g[nb - 1])]
    a += [a_lo] + list(ap.unbind(1)) + [s_hi]
    return torch.stack(b, dim=1), torch.stack(a, dim=1)


def fdn_geq_sections_host(rt: torch.Tensor, delays: torch.Tensor, fs, design: GEQDesign):
    """rt (n_bands,), delays (N,) -> (b, a), each (3, n_bands, N) float64: the graphic equaliser of every line
    (flamo/auxiliary/eq.py:57-111 on the gains of reverb.py:523-524)"""
    return fdn_geq_sections_from_db(fdn_gain_db(rt.double(), delays.double(), fs), design)


def fdn_geq_sections_from_db(gain_db: torch.Tensor, design: GEQDesign):
    """command gains in dB (n_bands, N) -> (b, a), each (3, n_bands, N) float64, on the device of the gains"""
    return _straight_through(_geq_taps, 10 ** (gain_db.double() / 20), design)


def nyquist_slope(rt_nyquist: float, fs) -> float:
    """dB per sample at the Nyquist frequency, formed in float32 as the reference forms it (reverb.py:824, 868)"""
    return float(rt2slope(torch.tensor(rt_nyquist, dtype=torch.float32), fs))


def _shelf1_taps(r, p, delays, fs, slope_nyq):
    g_nyq = 10 ** (slope_nyq * delays / 20)
    t = torch.tan(torch.clamp(p[1], min=0, max=torch.pi) / 2)
    sk = torch.sqrt(10 ** (rt2slope(p[0], fs) * delays / 20) / g_nyq)
    zero = torch.zeros_like(g_nyq)
    b = torch.stack([r(t * sk + 1) * g_nyq, r(t * sk - 1) * g_nyq, zero])
    a = torch.stack([r(t / sk + 1), r(t / sk - 1), zero])
    return b.unsqueeze(1), a.unsqueeze(1)


def fdn_shelf1_sections_host(p: torch.Tensor, delays: torch.Tensor, fs, slope_nyq: float):
    """p = (rt at DC, crossover w_c), delays (N,) -> (b, a), each (3, 1, N) float64: one first-order shelving section per
    line with a zero third tap (reverb.py:865-880)"""
    return _straight_through(_shelf1_taps, p.double(), delays.double(), fs, slope_nyq)


def sos_response_host(b: torch.Tensor, a: torch.Tensor, gamma: float, nfft: int) -> torch.Tensor:
    """prod B / prod A per bin of sections (3, S, ...) whose taps are weighted by gamma^[0, 1, 2] (reverb.py:531-537)"""
    env = (float(gamma) ** torch.arange(3, dtype=torch.float64, device=b.device)).view(3, *([1] * (b.dim() - 1)))
    B = torch.fft.rfft(b.double() * env, nfft, dim=0).prod(dim=1)
    A = torch.fft.rfft(a.double() * env, nfft, dim=0).prod(dim=1)
    H = B / A
    return torch.where(torch.abs(A) != 0, H, torch.finfo(H.dtype).eps * torch.ones_like(H))


def _rt_identity(x):
    """parallelFDNGEQ's parameter map (reverb.py:502); a named function so that the module can tell it from a user map"""
    return x


class _DelayScaled:
    """What the three attenuation classes share: the delays, uploaded once per device, the channel count, and a response for
    host tensors."""

    def _delays_on(self, device) -> torch.Tensor:
        """the delays as float64 on `device`, copied there once"""
        cache = self.__dict__.setdefault("_delays_dev", {})
        key = str(device)
        if key not in cache:
            cache[key] = torch.as_tensor(self.delays).detach().to(device=device, dtype=torch.float64).contiguous()
        return cache[key]

    def check_param_shape(self):
        assert len(self.size) == 1, "The parameter should contain only the command gains"

    def get_io(self):
        self.input_channels = len(self.delays)
        self.output_channels = len(self.delays)

    def _sos_to_response(self, b, a):
        if not b.is_cuda:
            return sos_response_host(b, a, self._gamma_f, self.nfft).to(torch.complex128 if self.dtype == torch.float64 else torch.complex64)
        return super()._sos_to_response(b, a)

    def _spectra(self, b, a):
        """B, A as the reference returns them from get_poly_coeff: rfft of the weighted taps"""
        env = (self._gamma_f ** torch.arange(3, dtype=torch.float64, device=b.device)).view(3, *([1] * (b.dim() - 1)))
        if b.is_cuda:
            return tuple(self.fft((t.double() * env).to(self.dtype)) for t in (b, a))
        return tuple(torch.fft.rfft(t.double() * env, self.nfft, dim=0) for t in (b, a))


class parallelFDNGEQ(_DelayScaled, dsp.parallelGEQ):
    """A graphic equaliser per delay line whose command gains follow from reverberation times: param (n_bands + 3,) in
    seconds, identity map, band k of line n commands -60 delays[n] / (param[k] fs) dB (reverb.py:459-552).  Meant for the
    feedback path of an FDN.  ``fold_map=False``: the gains always run as torch ops in front of the design kernel."""

    def __init__(self, octave_interval: int = 1, nfft: int = 2 ** 11, fs: int = 48000, delays: torch.Tensor = None,
                 requires_grad: bool = False, alias_decay_db: float = 0.0, device: Optional[str] = None,
                 dtype: torch.dtype = torch.float32, *, fold_map: bool = True):
        assert delays is not None, "Delays must be provided"
        self.delays = delays
        super().__init__(size=(), octave_interval=octave_interval, nfft=nfft, fs=fs, map=_rt_identity,
                         requires_grad=requires_grad, alias_decay_db=alias_decay_db, device=device, dtype=dtype,
                         fold_map=fold_map)

    def init_param(self):
        return torch.nn.init.uniform_(self.param, a=1.0, b=3.0)

    def _packed_on(self, device) -> torch.Tensor:
        """[delays, band constants] as the design kernels read them, uploaded once per device"""
        cache = self.__dict__.setdefault("_packed_dev", {})
        key = str(device)
        if key not in cache:
            cache[key] = torch.cat([self._delays_on(device), self._design.device_consts(device)]).contiguous()
        return cache[key]

    def _on_design_kernel(self, param) -> bool:
        return (self.map is _rt_identity and self.fold_map and torch.is_tensor(param) and param.is_cuda
                and param.dtype in (torch.float32, torch.float64))

    def _cascade_spec(self, param):
        if self._on_design_kernel(param):
            return ops.FdnAttenuation("fdn_geq", param, self._packed_on(param.device), len(self.delays), float(self.fs), 0.0)
        gain_db = fdn_gain_db(self.map(param.double()), self._delays_on(param.device), self.fs)
        return ops.RawSections("sos", *self._sos_coeffs(gain_db))

    def _sos_coeffs(self, gain_db):
        """command gains in dB (n_bands, N) -> this class's sections as torch ops (see _geq_taps: not the roundings of
        ops.geq_sections), on the device of the gains"""
        return fdn_geq_sections_from_db(gain_db, self._design)

    def get_freq_response(self):
        def response(param):
            if not param.is_cuda:
                return self.get_poly_coeff(self.map(param))[0]
            return self._cascade_spec(param).response(self._gamma_f, self.nfft, dtype=self.dtype)
        self.freq_response = response
        self._own_response = response

    def get_poly_coeff(self, param):
        """(H, B, A) for mapped parameters -- reverberation times -- as in the reference (reverb.py:515-537)"""
        rt = param.double()
        b, a = self._sos_coeffs(fdn_gain_db(rt, self._delays_on(rt.device), self.fs))
        return (self._sos_to_response(b, a), *self._spectra(b, a))


class parallelFDNAccurateGEQ(_DelayScaled, dsp.parallelAccurateGEQ):
    """The fitted graphic equaliser per delay line: param (n_bands + 2,) reverberation times in seconds, mapped to the target
    gains rt2slope(rt)[:, None] * delays[None, :] in dB; not learnable (reverb.py:303-391).  The fit runs on the host once
    per parameter value (AccurateGEQ._sos_coeffs); the reference repeats it per line on every forward call."""

    def __init__(self, octave_interval: int = 1, nfft: int = 2 ** 11, fs: int = 48000, delays: torch.Tensor = None,
                 alias_decay_db: float = 0.0, start_freq: float = 31.25, end_freq: float = 16000.0,
                 device: Optional[str] = None, dtype: torch.dtype = torch.float32):
        assert delays is not None, "Delays must be provided"
        self.delays = delays
        super().__init__(size=(), octave_interval=octave_interval, nfft=nfft, fs=fs,
                         map=lambda x: fdn_gain_db(x, self._delays_on(x.device).to(x.dtype), fs),
                         alias_decay_db=alias_decay_db, start_freq=start_freq, end_freq=end_freq, device=device, dtype=dtype)

    def get_poly_coeff(self, param):
        """(H, B, A) for mapped parameters -- target gains in dB (n_gains, N) (reverb.py:357-379)"""
        b, a = self._sos_coeffs(param)
        return (self._sos_to_response(b, a), *self._spectra(b, a))


class parallelFirstOrderShelving(_DelayScaled, dsp._SOSMixin, dsp.parallelFilter):
    """A first-order shelving filter per delay line: param = (rt at DC in seconds, crossover w_c in radians); the line's gain
    at the Nyquist frequency follows from ``rt_nyquist`` (reverb.py:808-887).  ``map`` turns the parameters into the two-tap
    pairs (b, a), each (2, N); the response is B / A of the taps weighted by gamma^[0, 1], evaluated by the cascade kernels as
    one section with a zero third tap."""

    def __init__(self, nfft: int = 2 ** 11, fs: int = 48000, rt_nyquist: float = 0.2, delays: torch.Tensor = None,
                 alias_decay_db: float = 0.0, device: str = None, requires_grad: bool = False,
                 dtype: torch.dtype = torch.float32, *, fold_map: bool = True):
        assert delays is not None, "Delays must be provided"
        self.delays = delays
        self.fs = fs
        self.fold_map = fold_map
        self.rt_nyquist = torch.tensor(rt_nyquist, device=device)
        self._slope_nyq = nyquist_slope(rt_nyquist, fs)
        own_map = lambda x: self.map_param(x, fs)  # noqa: E731
        super().__init__(size=(2,), nfft=nfft, map=own_map, alias_decay_db=alias_decay_db, device=device,
                         requires_grad=requires_grad, dtype=dtype)
        self._own_map = own_map
        self.alias_envelope_dcy = dsp._gamma(alias_decay_db, nfft, device, dtype) ** torch.arange(0, 2, 1, device=device, dtype=dtype)

    def check_param_shape(self):
        assert len(self.size) == 1, "Filter must be 1D, for 2D filters use Filter module."

    def map_param(self, param, fs):
        """(rt at DC, w_c) -> two-tap pairs (b, a), each (2, N) float64 (reverb.py:865-880)"""
        b, a = fdn_shelf1_sections_host(param, self._delays_on(param.device), fs, self._slope_nyq)
        return b[:2, 0], a[:2, 0]

    @staticmethod
    def _as_sections(taps):
        """two-tap pairs (2, N) -> sections (3, 1, N) with a zero third tap"""
        return tuple(torch.cat([t.double(), torch.zeros_like(t[:1], dtype=torch.float64)]).unsqueeze(1) for t in taps)

    def _on_design_kernel(self, param) -> bool:
        return (self.map is self._own_map and self.fold_map and torch.is_tensor(param) and param.is_cuda
                and param.dtype in (torch.float32, torch.float64))

    def _cascade_spec(self, param):
        if self._on_design_kernel(param):
            return ops.FdnAttenuation("fdn_shelf1", param, self._delays_on(param.device), len(self.delays), float(self.fs),
                                      self._slope_nyq)
        return ops.RawSections("sos", *self._as_sections(self.map(param.double())))

    def get_freq_response(self):
        def response(param):
            if not param.is_cuda:
                return self._sos_to_response(*self._as_sections(self.map(param.double())))
            return self._cascade_spec(param).response(self._gamma_f, self.nfft, dtype=self.dtype)
        self.freq_response = response
        self._own_response = response

    def get_poly_coeff(self, param):
        """(H, B, A) for mapped parameters -- the pairs (b, a) -- as in the reference (reverb.py:847-855)"""
        b, a = self._as_sections(param)
        B, A = self._spectra(b, a)
        return self._sos_to_response(b, a), B, A

    def probe(self, z: torch.Tensor):
        raise NotImplementedError("probe() not implemented for parallelFirstOrderShelving")


# ----------------------------------------------------------------------------- the canonical FDN (reverb.py:83-300)
class HomogeneousFDN:
    """Feedback delay network with homogeneous attenuation: Gain (N, 1) -> Recursion(fF = Series(parallelDelay,
    parallelGain under map_gamma), fB = orthogonal Matrix) -> Gain (1, N) between an FFT and an anti-aliased inverse
    (reverb.py:83-300).  ``config_dict`` is any object with the attributes of the reference's HomogeneousFDNConfig: N, delays,
    nfft, alias_decay_db, device, dtype, is_delay_int, the five ``*_grad`` flags, and sample_rate / delay_range_ms for
    ``rt2gain`` / ``get_delay_lines``."""

    def __init__(self, config_dict):
        self.config_dict = config_dict
        self.N = self.config_dict.N
        self.delays = self.config_dict.delays
        self.fdn = self.get_fdn_instance()
        self.set_model()

    def set_model(self, input_layer=None, output_layer=None):
        """(reverb.py:104-115)"""
        c = self.config_dict
        if input_layer is None:
            input_layer = dsp.FFT(c.nfft, dtype=c.dtype)
        if output_layer is None:
            output_layer = dsp.iFFTAntiAlias(nfft=c.nfft, alias_decay_db=c.alias_decay_db, device=c.device, dtype=c.dtype)
        self.model = self.get_shell(input_layer, output_layer)

    def get_fdn_instance(self):
        """(reverb.py:117-199)"""
        c = self.config_dict
        delay_lines = torch.tensor(self.delays)
        kw = dict(nfft=c.nfft, alias_decay_db=c.alias_decay_db, device=c.device, dtype=c.dtype)
        input_gain = dsp.Gain(size=(self.N, 1), requires_grad=c.input_gain_grad, **kw)
        output_gain = dsp.Gain(size=(1, self.N), requires_grad=c.output_gain_grad, **kw)
        delays = dsp.parallelDelay(size=(self.N,), max_len=int(delay_lines.max()), isint=c.is_delay_int,
                                   requires_grad=c.delays_grad, **kw)
        delays.assign_value(delays.sample2s(delay_lines.to(delays.param.device)))
        mixing_matrix = dsp.Matrix(size=(self.N, self.N), matrix_type="orthogonal", requires_grad=c.mixing_matrix_grad, **kw)
        attenuation = dsp.parallelGain(size=(self.N,), requires_grad=c.attenuation_grad, **kw)
        attenuation.map = map_gamma(delay_lines.to(attenuation.param.device))
        attenuation.assign_value(6 * torch.ones((self.N,), device=attenuation.param.device))
        feedforward = system.Series(OrderedDict({"delays": delays, "attenuation": attenuation}))
        feedback_loop = system.Recursion(fF=feedforward, fB=mixing_matrix)
        return system.Series(OrderedDict({"input_gain": input_gain, "feedback_loop": feedback_loop, "output_gain": output_gain}))

    def get_shell(self, input_layer, output_layer):
        return system.Shell(core=self.fdn, input_layer=input_layer, output_layer=output_layer)

    def get_delay_lines(self):
        """Co-prime delay line lengths in config.delay_range_ms (reverb.py:206-223)"""
        import sympy as sp
        c = self.config_dict
        delay_range_samps = np.round(np.asarray(c.delay_range_ms) * c.sample_rate / 1000).astype(int)
        prime_nums = np.array(list(sp.primerange(delay_range_samps[0], delay_range_samps[1])), dtype=np.int32)
        rand_primes = prime_nums[np.random.permutation(len(prime_nums))]
        return np.array(np.r_[rand_primes[: self.N - 1], sp.nextprime(delay_range_samps[1])], dtype=np.int32).tolist()

    def get_raw_parameters(self):
        """(reverb.py:225-237)"""
        with torch.no_grad():
            core = self.model.get_core()
            loop = core.feedback_loop
            return {"A": loop.feedback.param.cpu().numpy(),
                    "attenuation": loop.feedforward.attenuation.param.cpu().numpy(),
                    "B": core.input_gain.param.cpu().numpy(),
                    "C": core.output_gain.param.cpu().numpy(),
                    "m": loop.feedforward.delays.param.cpu().numpy()}

    def set_raw_parameters(self, param: dict):
        """(reverb.py:239-259)"""
        with torch.no_grad():
            core = self.model.get_core()
            loop = core.feedback_loop
            targets = {"A": (loop.feedback, False), "attenuation": (loop.feedforward.attenuation, True),
                       "B": (core.input_gain, False), "C": (core.output_gain, False), "m": (loop.feedforward.delays, True)}
            for key, value in param.items():
                if key in targets:
                    module, squeeze = targets[key]
                    value = torch.tensor(value)
                    module.assign_value((value.squeeze() if squeeze else value).to(module.param.device))
            self.model.set_core(core)

    def normalize_energy(self, target_energy=1):
        """Scales the input and output gains so that mean |H|^2 over the bins is target_energy (reverb.py:261-293)."""
        H = self.model.get_freq_response(identity=False)
        energy_H = torch.mean(torch.pow(torch.abs(H), 2))
        with torch.no_grad():
            core = self.model.get_core()
            scale = torch.pow(energy_H / target_energy, 1 / 4)
            core.input_gain.assign_value(torch.div(core.input_gain.param, scale))
            core.output_gain.assign_value(torch.div(core.output_gain.param, scale))
            self.model.set_core(core)
        H = self.model.get_freq_response(identity=False)
        energy_H = torch.mean(torch.pow(torch.abs(H), 2))
        assert abs(energy_H - target_energy) / target_energy < 0.0001, "Energy normalization failed"

    def rt2gain(self, rt60):
        """Reverberation time -> linear gain per delay line (reverb.py:295-300)"""
        gdB = rt2absorption(rt60, self.config_dict.sample_rate, torch.tensor(self.delays)).squeeze()
        return 10 ** (gdB / 20)
