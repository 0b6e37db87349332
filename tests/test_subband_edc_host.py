"""flamo_amd.optimize.subband_edc_loss on the host: its surface, and its torch lines against a float64 statement of the
definition written here -- the statement of the filter bank (test_filterbank_host.py) under Schroeder's backward integral in dB
and a mean squared error.  The GPU tests share the statement and the signals (test_subband_edc_gpu.py)."""
import inspect

import numpy as np
import pytest
import torch

from conftest import check_close
from test_filterbank_host import decaying_noise, statement_bank, statement_responses

OCTAVE_63_16K = [63, 125, 250, 500, 1000, 2000, 4000, 8000, 16000]
OPTIONS = [dict(), dict(energy_norm=True, convergence=True), dict(clip=True)]
COTANGENT = 3.0


def statement_curves(bands):
    """the energy decay curves in dB, and their energies, of band signals (B, T', N, K): the last 0.5 % of the samples dropped,
    E[s] = sum_{t >= s} y[t]^2"""
    keep = int(np.round(0.995 * bands.shape[1]))
    sq = bands[:, :keep].flatten(2) ** 2
    return torch.flip(torch.cumsum(torch.flip(sq, [1]), 1), [1])


def statement_loss(yp, yt, H, energy_norm=False, convergence=False, clip=False):
    """mean((e_p - e_t)^2) [/ mean(e_t^2)] over the curves e = 10 log10(E [/ E[0]]) of every (channel, band); with ``clip`` both
    are -180 dB where the target's curve is more than 60 dB under its start.  In the signals' precision."""
    Ep, Et = statement_curves(statement_bank(yp, H)), statement_curves(statement_bank(yt, H))
    if energy_norm:
        Ep, Et = Ep / Ep[:, :1], Et / Et[:, :1]
    ep, et = 10 * torch.log10(Ep), 10 * torch.log10(Et)
    if clip:
        below = et < et[:, :1] - 60
        ep, et = torch.where(below, torch.full_like(ep, -180.0), ep), torch.where(below, torch.full_like(et, -180.0), et)
    loss = ((ep - et) ** 2).mean()
    return loss / (et ** 2).mean() if convergence else loss


def statement_loss_and_grad(yp, yt, H, opts):
    """loss and gradient (cotangent 3) of the statement in yp's precision, as float64"""
    y = yp.clone().requires_grad_(True)
    loss = statement_loss(y, yt, H, **opts)
    (g,) = torch.autograd.grad(COTANGENT * loss, [y])
    return loss.detach().double(), g.double()


def clip_margin(yt, H):
    """the smallest |e_true - (max - 60)| in dB over the target's curves: how far every mask entry is from flipping"""
    et = 10 * torch.log10(statement_curves(statement_bank(yt, H)))
    return (et - (et[:, :1] - 60)).abs().min().item()


def signals(shape, seed):
    """(prediction, target): decaying noise, randn exp(-6.9 c t / T) with c = 1.3 and c = 1"""
    return decaying_noise(shape, seed, 1.3), decaying_noise(shape, seed + 100, 1.0)


def test_surface():
    from flamo_amd import optimize
    from flamo_amd.optimize import subband_edc_loss
    params = list(inspect.signature(subband_edc_loss.__init__).parameters.values())[1:]
    assert [(p.name, p.default) for p in params] == [
        ("center_frequencies", None), ("order", 5), ("sample_rate", 48000), ("energy_norm", False), ("convergence", False),
        ("clip", False), ("name", "SubbandEDC"), ("device", "cpu")]
    crit = subband_edc_loss()
    assert crit.center_frequencies == OCTAVE_63_16K and crit.bank.get_center_frequencies() == OCTAVE_63_16K
    assert crit.name == "SubbandEDC" and crit.bank._order == 5 and crit.bank._backend == "torch"
    assert subband_edc_loss(center_frequencies=[1000, 250], order=3).bank.get_center_frequencies() == [250, 1000]
    assert not hasattr(optimize, "mss_loss")
    assert not hasattr(crit, "_target_cache") and not any(torch.is_tensor(v) for v in vars(crit).values())      # nothing of a target is kept


@pytest.mark.parametrize("opts", OPTIONS, ids=["plain", "norm_conv", "clip"])
@pytest.mark.parametrize("shape", [(2, 960, 3), (1, 961, 2)])
def test_torch_lines_against_the_statement(shape, opts):
    """loss and gradient of the class's host lines in float64 against the statement, at the project's float64 limit 1e-10.
    Achieved: loss <= 2.6e-14, gradient <= 7.3e-12 (l2; max-norm <= 1.7e-11)."""
    from flamo_amd.optimize import subband_edc_loss
    yp, yt = signals(shape, 7)
    H = statement_responses(OCTAVE_63_16K, 5, 48000, shape[1] // 2 + 1)
    if opts.get("clip"):
        assert clip_margin(yt, H) > 1e-6
    ref, gref = statement_loss_and_grad(yp, yt, H, opts)
    y = yp.clone().requires_grad_(True)
    loss = subband_edc_loss(**opts)(y, yt)
    (g,) = torch.autograd.grad(COTANGENT * loss, [y])
    tag = f"subband_edc_host/{'x'.join(map(str, shape))}_{'_'.join(opts) or 'plain'}"
    check_close(tag + "/loss", loss.detach().reshape(1), ref.reshape(1), 1e-10)
    check_close(tag + "/grad", g, gref, 1e-10)


def test_one_signal_and_other_centres():
    """a 1-D pair is one (1, T, 1) signal; centres and order reach the bank"""
    from flamo_amd.optimize import subband_edc_loss
    yp, yt = signals((1, 960, 1), 8)
    H = statement_responses([250, 1000, 4000], 3, 48000, 481)
    loss = subband_edc_loss(center_frequencies=[4000, 250, 1000], order=3, energy_norm=True)(yp[0, :, 0], yt[0, :, 0])
    ref = statement_loss(yp, yt, H, energy_norm=True)
    check_close("subband_edc_host/1d", loss.reshape(1), ref.reshape(1), 1e-10)
