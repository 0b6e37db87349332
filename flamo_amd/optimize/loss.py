"""``mse_loss`` and ``sparsity_loss`` of the reference (flamo/optimize/loss.py:12-103) on the library's kernels -- the two
criteria of the colorless-FDN training (examples/e8_colorless_fdn.py:137-138) -- and its broadband ``edc_loss``
(loss.py:674-809), ``AveragePower`` (loss.py:462-549) and mel-band ``edr_loss`` (loss.py:553-670), the criteria of a fit to a
measured room impulse response, and ``mel_mss_loss`` (loss.py:169-296), the criterion of its loss profiles, with its
linear-scale sibling ``mss_loss`` (loss.py:298-459).  ``subband_edc_loss`` is
the package's own: ``edc_loss``'s criterion on the band signals of ``auxiliary.filterbank.FilterBank``.

The reference's training loop calls ``criterion(estimations, targets)`` (flamo/optimize/trainer.py:179-189); with
``flamo_amd.optimize.mse_loss`` in that list the loop runs unedited and the criterion costs one streaming pass over the
prediction each way (``ops.mse``) instead of torch's sum / sub / pow / mean kernels and their backward."""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import ops
from .utils import generate_partitions


def _device_pair(y_pred, y_true):
    """whether (prediction, target) are what the framed criteria's kernels read: device tensors of one real precision, the
    target without a gradient (the sizes are the ops' ``*_supported`` queries)"""
    return (torch.is_tensor(y_pred) and torch.is_tensor(y_true) and y_pred.is_cuda and y_true.is_cuda
            and y_pred.dtype in (torch.float32, torch.float64) and y_true.dtype == y_pred.dtype and not y_true.requires_grad)


class mse_loss(nn.Module):
    """Wrapper for the mean squared error loss: nn.MSELoss()(y_pred.sum(-1), y_true.squeeze(-1)), as
    flamo/optimize/loss.py:101-102.  Same constructor and attributes (nfft, device, mse_loss, name)."""

    def __init__(self, nfft: int = None, device: str = "cpu"):
        super().__init__()
        self.nfft = nfft
        self.device = device
        self.mse_loss = nn.MSELoss()
        self.name = "MSE"

    def forward(self, y_pred, y_true):
        if (torch.is_tensor(y_pred) and y_pred.is_cuda and y_pred.dtype in (torch.float32, torch.float64) and y_pred.dim() >= 1
                and y_true.is_cuda and tuple(y_true.squeeze(-1).shape) == tuple(y_pred.shape[:-1]) and y_pred.numel() > 0
                and not y_true.requires_grad and y_true.dtype == y_pred.dtype and y_pred.shape[-1] <= ops.MSE_MAX_COLS):
            return ops.mse(y_pred, y_true, sum_last=True)
        # anything else (host tensors, complex predictions, a target that takes a gradient or has another dtype, more
        # summed columns than the kernel takes): the reference's own lines
        y_pred_sum = torch.sum(y_pred, dim=-1)
        return self.mse_loss(y_pred_sum, y_true.squeeze(-1))


class edc_loss(nn.Module):
    """Energy decay curve criterion, flamo/optimize/loss.py:674-809 in its broadband form: the mean squared difference, in dB,
    of the Schroeder backward integrals of prediction and target (B, T, N), after the last ``discard_n`` = 0.5 % of the samples
    are dropped.  ``energy_norm`` refers every curve to its own start, ``clip`` sets both curves to -180 dB where the TARGET's
    is more than 60 dB under its maximum, ``convergence`` divides by the mean square of the target's curve.  Same constructor,
    defaults, attributes and methods as the reference's class; the subband form (``is_broadband=False``, the reference's
    default) needs pyfar's fractional-octave filter bank and is refused at construction.

    Device float32 / float64 predictions against a gradient-free target of the same shape and dtype run on ``ops.edc_loss``
    (a tiled scan each way); host tensors, a target that takes a gradient and other dtypes take the torch lines below."""

    def __init__(self, sample_rate: int = 48000, is_broadband: bool = False, n_fractions: int = 1, energy_norm: bool = False,
                 convergence: bool = False, clip: bool = False, name: str = "EDC", device: str = "cpu"):
        super().__init__()
        if not is_broadband:
            raise NotImplementedError("edc_loss(is_broadband=False): the subband form needs pyfar's fractional-octave filter bank "
                                      "(pyfar.dsp.filter.fractional_octave_bands), which this package does not carry; "
                                      "construct it with is_broadband=True")
        self.sample_rate = sample_rate
        self.is_broadband = is_broadband
        self.n_fractions = n_fractions
        self.energy_norm = energy_norm
        self.convergence = convergence
        self.clip = clip
        self.name = name
        self.device = device
        self.discard_n = 0.5
        self.mse = nn.MSELoss(reduction="mean")

    @staticmethod
    def _on_kernels(x):
        return torch.is_tensor(x) and x.is_cuda and x.dim() == 3 and x.dtype in (torch.float32, torch.float64) and x.numel() > 0

    def discard_last_n_percent(self, x, n_percent):
        """x (B, T, N) without its last n_percent of samples"""
        keep = int(np.round((1 - n_percent / 100) * x.shape[1]))
        return x[:, :keep, :]

    def schroeder_backward_int(self, x):
        """(E, Z): E[b, s, c] = sum_{t >= s} x[b, t, c]^2 divided by Z, Z = its per-column maximum (``energy_norm``) or ones"""
        energy = x.square().flip(1).cumsum(1).flip(1)
        if self.energy_norm:
            norm_vals = energy.amax(dim=1, keepdim=True)
        else:
            norm_vals = torch.ones_like(energy)
        return energy / norm_vals, norm_vals

    def get_edc(self, x):
        """the curve in dB, (B, T', N)"""
        if self._on_kernels(x) and self.discard_n == ops.EDC_DISCARD_PERCENT:
            return ops.edc_db(x, energy_norm=self.energy_norm)
        return self._torch_edc(x)

    def _torch_edc(self, x):
        return 10 * torch.log10(self.schroeder_backward_int(self.discard_last_n_percent(x, self.discard_n))[0])

    def _torch_forward(self, y_pred, y_true):
        """the criterion in plain torch, on whatever device the tensors live"""
        e_pred, e_true = self._torch_edc(y_pred), self._torch_edc(y_true)
        if self.clip:
            below = e_true < e_true.amax(dim=1, keepdim=True) - 60
            floor = torch.full_like(e_true, -180.0)
            e_pred, e_true = torch.where(below, floor, e_pred), torch.where(below, floor, e_true)
        num = self.mse(e_pred, e_true)
        if self.convergence:
            return num / torch.mean(e_true ** 2)
        return num

    def forward(self, y_pred, y_true):
        if y_pred.dim() == 1:
            y_pred, y_true = y_pred[None, :, None], y_true[None, :, None]
        assert y_pred.shape == y_true.shape and y_true.dim() == 3, \
            "y_pred and y_true must have the same shape (n_batch, n_samples, n_channels)"
        if (self._on_kernels(y_pred) and y_true.is_cuda and y_true.dtype == y_pred.dtype and not y_true.requires_grad
                and self.discard_n == ops.EDC_DISCARD_PERCENT):
            return ops.edc_loss(y_pred, y_true, energy_norm=self.energy_norm, convergence=self.convergence, clip=self.clip)
        return self._torch_forward(y_pred, y_true)


class subband_edc_loss(nn.Module):
    """Subband energy-decay-curve criterion: ``edc_loss``'s broadband criterion applied to the band signals of prediction and
    target (B, T, N) under ``auxiliary.filterbank.FilterBank`` (Butterworth bands of ``order`` around ``center_frequencies``,
    by default the octave centres 63 ... 16000 Hz, the range the reference's subband form asks of pyfar, loss.py:723) --
    ``edc_loss(bank(y_pred).flatten(2), bank(y_true).flatten(2))``, every (channel, band) pair a column: the mean over batch,
    time, channels and bands of the squared difference of the curves in dB.  ``energy_norm``, ``convergence`` and ``clip`` as in
    ``edc_loss``.  The package's own name for what the reference's ``edc_loss(is_broadband=False)`` computes with pyfar's bank
    (``edc_loss`` itself keeps refusing that form).

    One deliberate difference from the reference's order: it drops the last 0.5 % of the samples first and filters second;
    here the FULL signals are filtered and the criterion's own discard then removes the end of the band signals.  The
    transforms so run at the signal's own length (96000 has a plan; round(0.995 96000) = 95520 = 2^5 3 5 199 would take the
    chirp-z route), and the broadband kernels serve unchanged.  The bank's convolution is circular either way.

    Device float32 / float64 predictions against a gradient-free target of the same shape and dtype run on
    ``ops.subband_edc_loss`` (``ops.filterbank``, then the kernels of ``ops.edc_loss``, one autograd node; float32 signals are
    carried in float64 between the transform and the loss, see there); host tensors, a target that takes a gradient and other
    dtypes take the torch lines below.  The target's curves are computed on every call."""

    DEFAULT_CENTERS = (63, 125, 250, 500, 1000, 2000, 4000, 8000, 16000)

    def __init__(self, center_frequencies=None, order: int = 5, sample_rate: int = 48000, energy_norm: bool = False,
                 convergence: bool = False, clip: bool = False, name: str = "SubbandEDC", device: str = "cpu"):
        super().__init__()
        from ..auxiliary.filterbank import FilterBank
        self.sample_rate = sample_rate
        self.order = order
        self.energy_norm = energy_norm
        self.convergence = convergence
        self.clip = clip
        self.name = name
        self.device = device
        self.bank = FilterBank(fraction=1, order=order, sample_rate=sample_rate, backend="torch")
        self.bank.set_center_frequencies(list(self.DEFAULT_CENTERS if center_frequencies is None else center_frequencies))
        self.center_frequencies = self.bank.get_center_frequencies()
        self.broadband = edc_loss(sample_rate=sample_rate, is_broadband=True, energy_norm=energy_norm, convergence=convergence,
                                  clip=clip, device=device)

    def _torch_forward(self, y_pred, y_true):
        """the criterion in plain torch, on whatever device the tensors live"""
        return self.broadband._torch_forward(self.bank._torch_forward(y_pred).flatten(2), self.bank._torch_forward(y_true).flatten(2))

    def forward(self, y_pred, y_true):
        if y_pred.dim() == 1:
            y_pred, y_true = y_pred[None, :, None], y_true[None, :, None]
        assert y_pred.shape == y_true.shape and y_true.dim() == 3, \
            "y_pred and y_true must have the same shape (n_batch, n_samples, n_channels)"
        if (edc_loss._on_kernels(y_pred) and y_true.is_cuda and y_true.dtype == y_pred.dtype and not y_true.requires_grad
                and ops.filterbank_supported(self.bank)):
            return ops.subband_edc_loss(y_pred, y_true, self.bank, energy_norm=self.energy_norm, convergence=self.convergence,
                                        clip=self.clip)
        return self._torch_forward(y_pred, y_true)


class AveragePower(nn.Module):
    """Average-power criterion, flamo/optimize/loss.py:462-549: the magnitude spectrograms of prediction and target (frames of
    1024 samples, hop 256, Hann window) are each smoothed by a 64 x 64 Hann window with ``stride``, and the criterion is the
    Frobenius norm of the difference of the two divided by the norm of each.  ``energy_norm`` divides both signals by their
    2-norm first.  One signal, (T,) or (1, T, 1), with T >= 16128 (64 frames).  Same constructor, defaults, attributes and
    methods as the reference's class.

    A device float32 / float64 prediction of one signal with unit time stride, against a gradient-free target of the same
    shape and dtype, runs on ``ops.average_power`` (a framed transform each way, the spectrograms never stored); host tensors,
    a target that takes a gradient, other dtypes and the shapes the reference itself rejects take the reference's torch lines
    (``_torch_forward``) and raise what they raise."""

    def __init__(self, energy_norm: bool = False, name: str = "Average Power", stride: tuple = (4, 4), device="cpu"):
        super().__init__()
        self.name = name
        self.energy_norm = energy_norm
        self.stride = stride
        self.device = device

    def forward(self, y_pred, y_true):
        if len(y_pred.shape) == 1:
            y_pred = y_pred.unsqueeze(0).unsqueeze(-1)
            y_true = y_true.unsqueeze(0).unsqueeze(-1)
        assert (y_pred.shape == y_true.shape) & (len(y_true.shape) == 3), \
            "y_pred and y_true must have the same shape (n_batch, n_samples, n_channels)"
        if self.energy_norm:
            y_pred = y_pred / torch.norm(y_pred, p=2)
            y_true = y_true / torch.norm(y_true, p=2)
        return self.average_power(y_pred, y_true)[0]

    def _on_kernels(self, y_pred, y_true):
        try:
            si, sj = self.stride
            strides_ok = int(si) == si and int(sj) == sj and si >= 1 and sj >= 1
        except (TypeError, ValueError):
            return False
        return (strides_ok and torch.is_tensor(y_pred) and torch.is_tensor(y_true) and y_pred.is_cuda and y_true.is_cuda
                and y_pred.dtype in (torch.float32, torch.float64) and y_true.dtype == y_pred.dtype
                and y_pred.dim() == 3 and y_pred.shape[0] == 1 and y_pred.shape[2] == 1 and y_pred.stride(1) == 1
                and y_true.shape == y_pred.shape and not y_true.requires_grad and y_pred.shape[1] >= ops.AVGPOW_MIN_T)

    def average_power(self, y_pred, y_true):
        """(loss, S1_win, S2_win): the criterion and the two smoothed spectrograms"""
        if self._on_kernels(y_pred, y_true):
            loss, P1, P2 = ops.average_power(y_pred, y_true, stride=tuple(int(s) for s in self.stride))
            return loss, P1.squeeze(), P2.squeeze()
        return self._torch_forward(y_pred, y_true)

    def _torch_forward(self, y_pred, y_true):
        """the reference's own lines, on whatever device the tensors live"""
        dev = y_pred.device
        S1 = torch.abs(torch.stft(y_pred.squeeze(), n_fft=1024, hop_length=256, window=torch.hann_window(1024).to(dev),
                                  return_complex=True))
        S2 = torch.abs(torch.stft(y_true.squeeze(), n_fft=1024, hop_length=256, window=torch.hann_window(1024).to(dev),
                                  return_complex=True))
        win = self.window2d(torch.hann_window(64, dtype=S1.dtype, device=dev))
        S1_win = F.conv2d(S1.unsqueeze(0).unsqueeze(0), win.unsqueeze(0).unsqueeze(0), stride=self.stride).squeeze()
        S2_win = F.conv2d(S2.unsqueeze(0).unsqueeze(0), win.unsqueeze(0).unsqueeze(0), stride=self.stride).squeeze()
        return (torch.norm(S2_win - S1_win, p="fro") / torch.norm(S1_win, p="fro") / torch.norm(S2_win, p="fro"),
                S1_win, S2_win)

    def window2d(self, window):
        """create a 2D window from a given 1D window"""
        return window[:, None] * window[None, :]


class MultiResoSTFT(nn.Module):
    """Multi-resolution STFT criterion of (B, T, N) signals, the one examples/e8_fdn.py of the reference registers beside
    ``sparsity_loss`` (there wrapped from the auraloss package, whose ``MultiResolutionSTFTLoss()`` defaults these are).
    Every (batch, channel) column is one row.  For each resolution (n_fft, hop, win), with the periodic Hann window of ``win``
    samples centred in the frame, reflect padding and M = sqrt(clamp(|X|^2, min=eps)) of the prediction (p) and the target (t):

        sc  = |M_t - M_p|_F / |M_t|_F        (both norms over all rows, bins and frames at once)
        log = mean |log M_p - log M_t|
        lin = mean |M_p - M_t|

    and the criterion is the mean over the resolutions of ``w_sc sc + w_log_mag log + w_lin_mag lin``.

    Device float32 / float64 predictions against a gradient-free target of the same shape and dtype run on
    ``ops.mrstft_loss`` (three launches forward, two backward for all resolutions, rows and both signals; the spectrograms
    are never stored); host tensors, other dtypes, a target that takes a gradient and the parameter sets the kernels do not
    take run the torch lines of ``_torch_forward`` and raise what ``torch.stft`` raises."""

    def __init__(self, fft_sizes=(1024, 2048, 512), hop_sizes=(120, 240, 50), win_lengths=(600, 1200, 240), w_sc: float = 1.0,
                 w_log_mag: float = 1.0, w_lin_mag: float = 0.0, eps: float = 1e-8, name: str = "MultiResoSTFT", device="cpu"):
        super().__init__()
        assert len(fft_sizes) == len(hop_sizes) == len(win_lengths) and len(fft_sizes) >= 1, \
            "fft_sizes, hop_sizes and win_lengths must have the same, non-zero length"
        self.fft_sizes = tuple(fft_sizes)
        self.hop_sizes = tuple(hop_sizes)
        self.win_lengths = tuple(win_lengths)
        self.w_sc = w_sc
        self.w_log_mag = w_log_mag
        self.w_lin_mag = w_lin_mag
        self.eps = eps
        self.name = name
        self.device = device

    def resolutions(self):
        return tuple(zip(self.fft_sizes, self.hop_sizes, self.win_lengths))

    def _on_kernels(self, y_pred, y_true):
        return (_device_pair(y_pred, y_true)
                and ops.mrstft_supported(tuple(y_pred.shape), self.resolutions(), self.eps))

    def forward(self, y_pred, y_true):
        if y_pred.dim() == 1:
            y_pred, y_true = y_pred[None, :, None], y_true[None, :, None]
        assert y_pred.shape == y_true.shape and y_true.dim() == 3, \
            "y_pred and y_true must have the same shape (n_batch, n_samples, n_channels)"
        if self._on_kernels(y_pred, y_true):
            return ops.mrstft_loss(y_pred, y_true, self.resolutions(), (self.w_sc, self.w_log_mag, self.w_lin_mag), self.eps)
        return self._torch_forward(y_pred, y_true)

    def _torch_forward(self, y_pred, y_true):
        """the definition in plain torch, on whatever device the tensors live"""
        B, T, N = y_pred.shape
        rows = [y.permute(0, 2, 1).reshape(B * N, T) for y in (y_pred, y_true)]
        total = 0.0
        for n_fft, hop, win in self.resolutions():
            w = torch.hann_window(win, dtype=y_pred.dtype, device=y_pred.device)
            Mp, Mt = (torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=self.eps))
                      for X in (torch.stft(r, n_fft, hop, win, w, center=True, pad_mode="reflect", return_complex=True)
                                for r in rows))
            sc = torch.linalg.vector_norm(Mt - Mp) / torch.linalg.vector_norm(Mt)
            log = torch.mean(torch.abs(torch.log(Mp) - torch.log(Mt)))
            lin = torch.mean(torch.abs(Mp - Mt))
            total = total + self.w_sc * sc + self.w_log_mag * log + self.w_lin_mag * lin
        return total / len(self.fft_sizes)


class edr_loss(nn.Module):
    """Energy decay relief criterion, flamo/optimize/loss.py:553-670 (Mezza et al., DAFx24): the frequency-dependent decay of
    (B, T, N) signals on 64 mel bands.  Every (batch, channel) column is one row -- for N = 1 the reference's layout exactly;
    for N > 1 the reference reshapes (B, T, N) to (B N, T) without a permute and mixes channels into time, which is not
    reproduced here.  With ``win_length`` = int(0.020 sample_rate), hop = int(win_length (1 - overlap)), the periodic Hann
    window centred in frames of ``nfft`` samples and reflect padding:

        P   = |X|^2                                   the power spectrogram, (rows, nfft / 2 + 1, F), F = 1 + T // hop
        m   = W P                                     W = ops.mel_basis(sample_rate, nfft): 64 bands from 20 Hz to sample_rate // 2
        E   = sum_{f' >= f} m[f']^2                   the backward integral over frames
        edr = 10 log10 E   (``energy_norm``: 10 log10 (E / E[0]))
        loss = sum |edr_t - edr_p| / sum |edr_t|      over all rows, bands and frames at once

    and where the TARGET's E is exactly 0 (its edr is -inf) both entries are replaced by finfo(dtype).eps: 0 to the numerator,
    eps to the denominator, no gradient.  The reference forms P as sqrt(re^2 + im^2) ** 2 (nnAudio), the same value wherever
    |X| > 0; |X|^2 taken directly has the gradient 0 at an exact zero.

    Same constructor, defaults and attributes as the reference's class (plus ``win_length``, which it sets too), and its
    methods but ``get_edr``, which there calls a ``filterbank`` method the class does not have.

    Device float32 / float64 predictions against a gradient-free target of the same shape and dtype run on ``ops.edr_loss``
    (three launches forward, three backward; the spectrograms are never stored); host tensors, other dtypes, a target that
    takes a gradient and the frame lengths the kernels do not take run the torch lines of ``_torch_forward``."""

    def __init__(self, nfft: int = 1024, overlap: float = 0.5, sample_rate: int = 48000, energy_norm: bool = False,
                 device: str = "cpu", name: str = "EDR"):
        super().__init__()
        self.nfft = nfft
        self.overlap = overlap
        self.sample_rate = sample_rate
        self.energy_norm = energy_norm
        self.win_length = int(0.020 * self.sample_rate)
        self.name = name
        self.device = device

    def hop_length(self):
        return int(self.win_length * (1 - self.overlap))

    def discard_last_n_percent(self, x, n_percent):
        """x (B, T, N) without its last n_percent of samples"""
        last_id = int(np.round((1 - n_percent / 100) * x.shape[1]))
        return x[:, 0:last_id, :]

    def schroeder_backward_int(self, x):
        """(E, Z) of x (..., F, N): E[..., f, c] = sum_{f' >= f} x[..., f', c]^2 divided by Z, Z = its maximum over f
        (``energy_norm``) or ones"""
        out = torch.flip(torch.cumsum(torch.flip(x, dims=[-2]) ** 2, dim=-2), dims=[-2])
        if self.energy_norm:
            norm_vals = torch.max(out, dim=-2, keepdim=True)[0]
        else:
            norm_vals = torch.ones(out.shape, device=out.device, dtype=out.dtype)
        return out / norm_vals, norm_vals

    def mel_stft(self, x):
        """the mel power spectrogram (rows, 64, F) of x (rows, T), in x's dtype"""
        window = torch.hann_window(self.win_length, periodic=True, dtype=x.dtype, device=x.device)
        X = torch.stft(x, self.nfft, self.hop_length(), self.win_length, window, center=True, pad_mode="reflect",
                       return_complex=True)
        W = ops.mel_basis(self.sample_rate, self.nfft, 64, 20.0, self.sample_rate // 2).to(device=x.device, dtype=x.dtype)
        return torch.matmul(W, X.real ** 2 + X.imag ** 2)

    def _on_kernels(self, y_pred, y_true):
        return (_device_pair(y_pred, y_true) and self.sample_rate // 2 > ops.EDR_FMIN
                and ops.edr_supported(tuple(y_pred.shape), self.nfft, self.hop_length(), self.win_length))

    def forward(self, y_pred, y_true):
        if len(y_pred.shape) == 1:
            y_pred = y_pred.unsqueeze(0).unsqueeze(-1)
            y_true = y_true.unsqueeze(0).unsqueeze(-1)
        assert (y_pred.shape == y_true.shape) & (len(y_true.shape) == 3), \
            "y_pred and y_true must have the same shape (n_batch, n_samples, n_channels)"
        if self._on_kernels(y_pred, y_true):
            return ops.edr_loss(y_pred, y_true, self.nfft, self.hop_length(), self.win_length, self.sample_rate, self.energy_norm)
        return self._torch_forward(y_pred, y_true)

    def _torch_forward(self, y_pred, y_true):
        """the definition in plain torch, on whatever device the tensors live"""
        B, T, N = y_pred.shape
        edr = []
        for y in (y_pred, y_true):
            m = self.mel_stft(y.permute(0, 2, 1).reshape(B * N, T))                      # (rows, 64, F)
            E = torch.flip(torch.cumsum(torch.flip(m, dims=[-1]) ** 2, dim=-1), dims=[-1])
            # (a silent band has E[0] = 0: it is divided by 1, stays 0 and is clipped below, not 0 / 0)
            E0 = torch.where(E[..., :1] == 0, torch.ones_like(E[..., :1]), E[..., :1])
            edr.append((E, E / E0 if self.energy_norm else E))
        (Ep, xp), (Et, xt) = edr
        clip = Et == 0
        one = torch.ones_like(xt)
        eps = torch.full_like(xt, torch.finfo(xt.dtype).eps)
        # (the logarithm only ever sees the clipped entries as 1: no 0 * inf reaches the gradient)
        edr_p = torch.where(clip, eps, 10 * torch.log10(torch.where(clip, one, xp)))
        edr_t = torch.where(clip, eps, 10 * torch.log10(torch.where(clip, one, xt)))
        return torch.sum(torch.abs(edr_t - edr_p)) / torch.sum(torch.abs(edr_t))


class mel_mss_loss(nn.Module):
    """Multi-scale spectral criterion on the mel scale, flamo/optimize/loss.py:169-296: the criterion of the reference's loss
    profiles (examples/e9_loss_profile.py).  Every (batch, channel) column of the (B, T, N) signals is one row -- for N = 1 the
    reference's layout exactly; for N > 1 the reference reshapes (B, T, N) to (B N, T) without a permute and mixes channels
    into time, which is not reproduced here (as in ``edr_loss``).  For every n_fft of ``nfft``, with hop = int(n_fft (1 -
    overlap)), the periodic Hann window of n_fft samples and reflect padding (nnAudio's MelSpectrogram at its defaults):

        P    = |X|^2                                  the power spectrogram, (rows, n_fft / 2 + 1, F), F = 1 + T // hop
        m    = W P                                    W = ops.mel_basis(sample_rate, n_fft, n_fft // 8, 0, sample_rate // 2)
        mask = 1, Nn = numel(m_t)                     or, with ``apply_mask``, with ne = ``noise_energy``:
               SNR = 10 log10(max(m_t^2, 1.01 ne) - ne) - 10 log10(ne),  mask = 0 where SNR < threshold,  Nn = sum mask
        loss += |(m_t - m_p) mask|_p / Nn
        loss += alpha |(log m_t - log m_p) mask|_p / Nn                                                   (``log_term``)

    summed (not averaged) over the resolutions; p = "fro" is the square root of the sum of squares over everything at once.
    Nothing is clamped: a band that is exactly 0 in either signal makes the log term non-finite, as in the reference.
    ``energy_norm`` divides both signals by their 2-norm over the whole tensor first.

    ``noise_energy`` None (or 0) is replaced at the first resolution of the first masked call by
    mean(m_t[:, :, -int(0.01 sample_rate / hop)]^2) -- frame 0 when that integer is 0 -- and then KEPT on the module, as a
    number, for every later resolution and call: the reference's statefulness.  Deriving it reads one number back from the
    device, once; pass ``noise_energy`` when the step is captured in a graph.

    Same constructor, defaults and attributes as the reference's class.  Device float32 / float64 predictions against a
    gradient-free target of the same shape and dtype run on ``ops.mel_mss_loss`` (at most four launches forward and three
    backward for all resolutions; the mel spectrograms are never stored); host tensors, other dtypes, a target that takes a
    gradient, other ``p`` and the resolutions the kernels do not take run the torch lines of ``_torch_forward``."""

    def __init__(self, nfft=[128, 256, 512, 1024, 2048, 4096], overlap: float = 0.75, sample_rate: int = 48000,
                 energy_norm: bool = False, device="cpu", name: str = "MelMSS", apply_mask: bool = False, threshold: float = 5,
                 p="fro", log_term: bool = False, alpha: float = 1.0, noise_energy=None):
        super().__init__()
        self.nfft = nfft
        self.overlap = overlap
        self.sample_rate = sample_rate
        self.energy_norm = energy_norm
        self.name = name
        self.device = device
        self.apply_mask = apply_mask
        self.threshold = threshold
        self.p = p
        self.log_term = log_term
        self.alpha = alpha
        self.noise_energy = noise_energy

    def hop_length(self, nfft):
        return int(nfft * (1 - self.overlap))

    def mel_stft(self, x, nfft):
        """the mel power spectrogram (rows, nfft // 8, F) of x (rows, T), in x's dtype"""
        window = torch.hann_window(nfft, periodic=True, dtype=x.dtype, device=x.device)
        X = torch.stft(x, nfft, self.hop_length(nfft), nfft, window, center=True, pad_mode="reflect", return_complex=True)
        W = ops.mel_basis(self.sample_rate, nfft, nfft // 8, 0.0, self.sample_rate // 2).to(device=x.device, dtype=x.dtype)
        return torch.matmul(W, X.real ** 2 + X.imag ** 2)

    def _noise(self, m_true, nfft):
        """``noise_energy``, derived from the target's mel spectrogram at this resolution when there is none yet, and kept"""
        if not self.noise_energy:
            frame = -int(0.01 * self.sample_rate / self.hop_length(nfft))
            self.noise_energy = float(torch.mean(m_true.detach()[:, :, frame] ** 2))
        return float(self.noise_energy)

    @staticmethod
    def _rows(y):
        B, T, N = y.shape
        return y.permute(0, 2, 1).reshape(B * N, T)

    def _on_kernels(self, y_pred, y_true):
        return (_device_pair(y_pred, y_true)
                and ops.mel_mss_supported(tuple(y_pred.shape), self.nfft, self.overlap, self.sample_rate, self.p))

    def forward(self, y_pred, y_true):
        if len(y_pred.shape) == 1:
            y_pred = y_pred.unsqueeze(0).unsqueeze(-1)
            y_true = y_true.unsqueeze(0).unsqueeze(-1)
        assert (y_pred.shape == y_true.shape) & (len(y_true.shape) == 3), \
            "y_pred and y_true must have the same shape (n_batch, n_samples, n_channels)"
        if not self._on_kernels(y_pred, y_true):
            return self._torch_forward(y_pred, y_true)
        if self.energy_norm:
            y_pred = y_pred / torch.norm(y_pred, p=2)
            y_true = y_true / torch.norm(y_true, p=2)
        ne = None
        if self.apply_mask:
            first = self.nfft[0]
            ne = self._noise(self.mel_stft(self._rows(y_true), first), first) if not self.noise_energy else float(self.noise_energy)
        return ops.mel_mss_loss(y_pred, y_true, self.nfft, self.overlap, self.sample_rate, self.p, self.log_term, self.alpha,
                                self.apply_mask, self.threshold, ne)

    def _torch_forward(self, y_pred, y_true):
        """the definition in plain torch, on whatever device the tensors live"""
        if self.energy_norm:
            y_pred = y_pred / torch.norm(y_pred, p=2)
            y_true = y_true / torch.norm(y_true, p=2)
        rows_p, rows_t = self._rows(y_pred), self._rows(y_true)
        loss = 0
        for nfft in self.nfft:
            m_p, m_t = self.mel_stft(rows_p, nfft), self.mel_stft(rows_t, nfft)
            mask = torch.ones_like(m_t)
            if self.apply_mask:
                ne = self._noise(m_t, nfft)
                snr = 10 * torch.log10(torch.clamp(m_t ** 2, min=ne * 1.01) - ne) - 10 * math.log10(ne)
                mask[snr < self.threshold] = 0
                n = torch.sum(mask)
            else:
                n = torch.numel(m_t)
            loss = loss + torch.norm((m_t - m_p) * mask, p=self.p) / n
            if self.log_term:
                loss = loss + self.alpha * torch.norm((torch.log(m_t) - torch.log(m_p)) * mask, p=self.p) / n
        return loss


class mss_loss(nn.Module):
    """Multi-scale spectral criterion on the LINEAR frequency scale, flamo/optimize/loss.py:298-459, in its plain, its
    "yamamoto" (Parallel WaveGAN) and its "magenta" (DDSP) form.  It lives here, ``from flamo_amd.optimize.loss import
    mss_loss`` -- the reference's own import path -- and is not re-exported from ``flamo_amd.optimize``, whose list of names
    is pinned by the tests of the criteria before it.

    Every (batch, channel) column of the (B, T, N) signals is one row -- for N = 1 the reference's layout exactly; for N > 1
    the reference reshapes (B, T, N) to (B N, T) without a permute and mixes channels into time, which is not reproduced here
    (as in ``edr_loss`` and ``mel_mss_loss``).  For every n = n_fft of ``nfft``, with hop = int(n (1 - overlap)), K = n // 2 +
    1, the periodic Hann window w of n samples and reflect padding by n // 2 (nnAudio's STFT with freq_scale="linear", fmin =
    20, fmax = sample_rate // 2, output_format="Magnitude"; nnAudio is no dependency):

        beta_k = a + k s,  a = 20 n / sample_rate,  s = (sample_rate // 2 - 20) (n / sample_rate) / K     fractional DFT bins
        X[k,f] = sum_j w_j x[f hop + j] exp(-2 pi i beta_k j / n)                  (rows, K, F), F = 1 + T // hop
        M      = sqrt(re^2 + im^2)                                                 nothing added, nothing clamped
        mask   = 1, Nn = numel(M_t)                or, with ``apply_mask``, with ne = ``noise_energy``:
                 SNR = 10 log10(max(M_t^2, 1.01 ne) - ne) - 10 log10(ne),  mask = 0 where SNR < threshold,
                 Nn = sum mask when ``form`` is None, else numel(M_t)
        d, dl  = (M_t - M_p) mask,  (log M_t - log M_p) mask
        form None:        |d|_p / Nn  +  alpha |dl|_p / Nn  (the second with ``log_term``)
        form "yamamoto":  |d|_fro / |M_t|_fro + alpha |dl|_1 / numel               (the denominator unmasked; p, log_term ignored)
        form "magenta":   (|d|_1 + alpha |dl|_1) / numel

    summed (not averaged) over the resolutions.  The derivative of the square root at an exact zero is taken as 0: a silent
    stretch of the prediction gives a finite loss and an exact-zero gradient without a log term; with one the loss is
    non-finite, as in the reference.  ``energy_norm`` divides both signals by their 2-norm over the whole tensor first.

    ``noise_energy`` None (or 0) is replaced at the first resolution of the first masked call by
    mean(M_t[:, :, -int(0.01 sample_rate / hop)]^2) -- frame 0 when that integer is 0 -- and then KEPT on the module, as a
    number, for every later resolution and call: the reference's statefulness.  Deriving it reads one number back from the
    device, once; pass ``noise_energy`` when the step is captured in a graph.

    Same constructor, order, defaults and attributes as the reference's class, with one difference: a ``form`` other than
    None, "yamamoto" or "magenta" raises ValueError here (the reference returns 0 for it).  Device float32 / float64
    predictions against a gradient-free target of the same shape and dtype run on ``ops.mss_loss`` (three launches forward and
    two backward for all resolutions: the transform is a dense float64 product on the matrix cores); host tensors, other
    dtypes, a target that takes a gradient, other ``p`` and the sizes the kernels do not take run the torch lines of
    ``_torch_forward``."""

    def __init__(self, nfft=[128, 256, 512, 1024, 2048, 4096], overlap: float = 0.75, sample_rate: int = 48000,
                 energy_norm: bool = False, device="cpu", name: str = "MSS", apply_mask: bool = False, threshold: float = 5,
                 p="fro", log_term: bool = False, alpha: float = 1.0, form: str = None, noise_energy=None):
        super().__init__()
        if form not in (None, "yamamoto", "magenta"):
            raise ValueError(f"mss_loss: form must be None, 'yamamoto' or 'magenta', got {form!r}")
        self.nfft = nfft
        self.overlap = overlap
        self.sample_rate = sample_rate
        self.energy_norm = energy_norm
        self.name = name
        self.device = device
        self.apply_mask = apply_mask
        self.threshold = threshold
        self.p = p
        self.log_term = log_term
        self.alpha = alpha
        self.form = form
        self.noise_energy = noise_energy
        self._bases = {}

    def hop_length(self, nfft):
        return int(nfft * (1 - self.overlap))

    def _basis(self, nfft, dtype, device):
        """the windowed basis (n_fft, 2 K), cos then -sin, built in float64 and cast; kept per (n_fft, dtype, device)"""
        key = (nfft, self.sample_rate, dtype, str(device))
        if key not in self._bases:
            cos, sin = ops.mss_basis(self.sample_rate, nfft, device)
            w = torch.hann_window(nfft, periodic=True, dtype=torch.float64, device=device)
            self._bases[key] = (torch.cat((cos, -sin)) * w).T.contiguous().to(dtype)
        return self._bases[key]

    def lin_stft(self, x, nfft):
        """the magnitude spectrogram (rows, nfft // 2 + 1, F) of x (rows, T) on the linear scale, in x's dtype"""
        K = nfft // 2 + 1
        padded = F.pad(x[:, None, :], (nfft // 2, nfft // 2), mode="reflect")[:, 0]
        X = padded.unfold(-1, nfft, self.hop_length(nfft)) @ self._basis(nfft, x.dtype, x.device)          # (rows, F, 2 K)
        power = (X[..., :K] ** 2 + X[..., K:] ** 2).transpose(1, 2)
        zero = power == 0
        # (the square root only ever sees the exact zeros as 1: its derivative there is taken as 0, no 0 * inf)
        return torch.where(zero, torch.zeros_like(power), torch.sqrt(torch.where(zero, torch.ones_like(power), power)))

    def _noise(self, M_true, nfft):
        """``noise_energy``, derived from the target's spectrogram at this resolution when there is none yet, and kept"""
        if not self.noise_energy:
            frame = -int(0.01 * self.sample_rate / self.hop_length(nfft))
            self.noise_energy = float(torch.mean(M_true.detach()[:, :, frame] ** 2))
        return float(self.noise_energy)

    @staticmethod
    def _rows(y):
        B, T, N = y.shape
        return y.permute(0, 2, 1).reshape(B * N, T)

    def _on_kernels(self, y_pred, y_true):
        return (_device_pair(y_pred, y_true)
                and ops.mss_supported(tuple(y_pred.shape), self.nfft, self.overlap, self.sample_rate, self.p, self.form))

    def forward(self, y_pred, y_true):
        if len(y_pred.shape) == 1:
            y_pred = y_pred.unsqueeze(0).unsqueeze(-1)
            y_true = y_true.unsqueeze(0).unsqueeze(-1)
        assert (y_pred.shape == y_true.shape) & (len(y_true.shape) == 3), \
            "y_pred and y_true must have the same shape (n_batch, n_samples, n_channels)"
        if not self._on_kernels(y_pred, y_true):
            return self._torch_forward(y_pred, y_true)
        if self.energy_norm:
            y_pred = y_pred / torch.norm(y_pred, p=2)
            y_true = y_true / torch.norm(y_true, p=2)
        ne = None
        if self.apply_mask:
            first = self.nfft[0]
            ne = self._noise(self.lin_stft(self._rows(y_true), first), first) if not self.noise_energy else float(self.noise_energy)
        return ops.mss_loss(y_pred, y_true, self.nfft, self.overlap, self.sample_rate, self.p, self.log_term, self.alpha,
                            self.apply_mask, self.threshold, ne, self.form)

    def _torch_forward(self, y_pred, y_true):
        """the definition in plain torch, on whatever device the tensors live"""
        if self.energy_norm:
            y_pred = y_pred / torch.norm(y_pred, p=2)
            y_true = y_true / torch.norm(y_true, p=2)
        rows_p, rows_t = self._rows(y_pred), self._rows(y_true)
        loss = 0
        for nfft in self.nfft:
            M_p, M_t = self.lin_stft(rows_p, nfft), self.lin_stft(rows_t, nfft)
            mask = torch.ones_like(M_t)
            n = numel = torch.numel(M_t)
            if self.apply_mask:
                ne = self._noise(M_t, nfft)
                snr = 10 * torch.log10(torch.clamp(M_t ** 2, min=ne * 1.01) - ne) - 10 * math.log10(ne)
                mask[snr < self.threshold] = 0
                n = torch.sum(mask)
            d = (M_t - M_p) * mask
            if self.form is None:
                loss = loss + torch.norm(d, p=self.p) / n
                if self.log_term:
                    loss = loss + self.alpha * torch.norm((torch.log(M_t) - torch.log(M_p)) * mask, p=self.p) / n
                continue
            dl = (torch.log(M_t) - torch.log(M_p)) * mask
            if self.form == "yamamoto":
                loss = loss + torch.norm(d, p="fro") / torch.norm(M_t, p="fro") + self.alpha * torch.norm(dl, p=1) / numel
            else:
                loss = loss + (torch.norm(d, p=1) + self.alpha * torch.norm(dl, p=1)) / numel
        return loss


class masked_mse_loss(nn.Module):
    """Mean squared error over a random subset of the frequency bins, flamo/optimize/loss.py:106-167: the bins are shuffled and
    cut into sets of ``n_samples`` (``generate_partitions``), every call takes the next set, and when all are used the walk
    starts over -- with freshly drawn sets when ``regenerate_mask``.  A few thousand samples per step: plain torch on
    whatever device the prediction lives."""

    def __init__(self, nfft: int, n_samples: int, n_sets: int = 1, regenerate_mask: bool = True, device: str = "cpu"):
        super().__init__()
        self.device = device
        self.n_samples = n_samples
        self.n_sets = n_sets
        self.nfft = nfft
        self.regenerate_mask = regenerate_mask
        self.mask_indices = self._draw()
        self.i = -1

    def _draw(self):
        return generate_partitions(torch.arange(self.nfft // 2 + 1), self.n_samples, self.n_sets)

    def forward(self, y_pred, y_true):
        self.i += 1
        if self.i >= self.mask_indices.shape[0]:
            self.i = 0
            if self.regenerate_mask:
                self.mask_indices = self._draw()
        mask = self.mask_indices[self.i].to(y_pred.device)
        return torch.mean(torch.pow(y_pred[:, mask] - y_true[:, mask], 2))


# where the reference looks for the mixing matrix of an FDN core, in its order (optimize/loss.py:41-49)
_MIXING_MATRIX_PATHS = (
    ("feedback_loop", "feedback"),
    ("feedback_loop", "feedback", "mixing_matrix"),
    ("branchA", "feedback_loop", "feedback", "mixing_matrix"),
)


def _mapped_mixing_matrix(core):
    """(module, map(param)) of the first place of ``_MIXING_MATRIX_PATHS`` that has a mapped parameter; the last place's
    own exception propagates when none has (the reference's nested try / except ends the same way)."""
    for n, path in enumerate(_MIXING_MATRIX_PATHS):
        try:
            module = core
            for name in path:
                module = getattr(module, name)
            return module, module.map(module.param)
        except Exception:
            if n == len(_MIXING_MATRIX_PATHS) - 1:
                raise


class sparsity_loss(nn.Module):
    """Sparsity of the feedback matrix of an FDN model's core, (sum|A| - N sqrt N) / (N (1 - sqrt N)) -- flamo/optimize/loss.py:12-63.
    Same signature (``y_pred`` and ``y_target`` are accepted and ignored, as flamo.optimize.trainer.Trainer passes them) and the same
    places the mixing matrix is looked for; a ``HouseholderMatrix`` holds the unit vector u and the criterion is that of
    ``I - 2 u u^T`` (loss.py:51-53); a (C, N, N) stack gives the mean over C.  On real square device matrices the criterion is one
    launch each way (``ops.sparsity``) instead of torch's abs / sum / sub / div / neg launches and their backward; complex
    matrices (the Householder form: its map returns a complex vector), host tensors and anything else take the torch lines."""

    def forward(self, y_pred, y_target, model):
        from ..processor.dsp import HouseholderMatrix

        mixing_matrix, A = _mapped_mixing_matrix(model.get_core())
        if isinstance(mixing_matrix, HouseholderMatrix):
            u = A
            A = torch.eye(u.shape[0], device=u.device, dtype=u.dtype) - 2 * u @ u.T
        N = A.shape[-1]
        root = N ** 0.5
        if (A.is_cuda and A.dtype in (torch.float32, torch.float64) and A.dim() in (2, 3) and A.shape[-2] == N and N >= 2
                and A.numel() > 0):
            return ops.sparsity(A)
        if A.dim() == 3:
            return torch.mean((torch.sum(torch.abs(A), dim=(-2, -1)) - N * root) / (N * (1 - root)))
        return -(torch.sum(torch.abs(A)) - N * root) / (N * (root - 1))
