"""Sparse scattering: a stack of orthogonal matrices with integer delays between them as one filter matrix
(flamo/auxiliary/scattering.py; Schlecht & Habets, "Scattering in feedback delay networks", IEEE/ACM TASLP 28, 2020).

    U(z) = D_{m_L}(z) U_K D_{m_K}(z) ... U_1 D_{m_1}(z) U_0 D_{m_R}(z)

``ScatteringMapping.forward`` returns the time-domain form, an (L, N, N) FIR matrix, built with whole-tensor ops (a delay is
one ``scatter_add`` along the tap axis, a stage one ``einsum``), differentiable in the stage matrices, on whatever device they
live.  The frequency-domain modules (``dsp.ScatteringMatrix`` / ``dsp.VelvetNoiseMatrix``) evaluate the same factors per bin
on the GPU (``ops.scatter_response``) and use this form where that route does not apply.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn


def get_random_shifts(N, sparsity_vect, pulse_size, dtype=torch.float32):
    """(n_stages, N) stage delays: channel i of stage k waits floor(sparsity_k (i + 0.99 u)) pulses, u uniform in [0, 1), and
    a pulse of stage k+1 is as long as the whole spread of stage k (N sparsity_k pulses of stage k).  One ``torch.rand(N)`` per
    stage, first stage first: under one ``torch.manual_seed`` the delays are those of the reference's function of this name."""
    dev = sparsity_vect.device
    channel = torch.arange(0, N, device=dev, dtype=dtype)
    shifts = torch.zeros(sparsity_vect.shape[0], N, device=dev, dtype=dtype)
    for k, sparsity in enumerate(sparsity_vect):
        slot = torch.floor(sparsity * (channel + 0.99 * torch.rand(N, device=dev, dtype=dtype)))
        shifts[k] = (slot * pulse_size).int()
        pulse_size = pulse_size * N * sparsity
    return shifts


def hadamard_matrix(N):
    """Orthonormal Hadamard matrix (Sylvester's construction) of the first power of two that is >= N, float64"""
    H = torch.ones(1, 1, dtype=torch.float64)
    step = torch.tensor([[1.0, 1.0], [1.0, -1.0]], dtype=torch.float64) / 2.0 ** 0.5
    while H.shape[0] < N:
        H = torch.kron(H, step)
    return H


def _delay_taps(V, delays, dim):
    """V: (N, N, T) taps; row (dim 0) or column (dim 1) i moves ``delays[i]`` taps later -> (N, N, T + max delay)"""
    N, _, T = V.shape
    d = delays.to(device=V.device, dtype=torch.int64)
    out = torch.zeros(N, N, T + int(d.max()), device=V.device, dtype=V.dtype)
    where = torch.arange(T, device=V.device) + d.view(N, 1)                      # (N, T)
    where = where.view(N, 1, T) if dim == 0 else where.view(1, N, T)
    return out.scatter_add(2, where.expand(N, N, T), V)


class ScatteringMapping(nn.Module):
    """Maps the (n_stages + 1, N, N) stack U to the FIR matrix of U(z) above.

    Attributes (as the reference's class): ``shifts`` (n_stages, N) stage delays drawn by ``get_random_shifts``, ``m_L`` /
    ``m_R`` (N,) outer delays (zeros when not given), ``sparsity_vect``, ``n_stages``, ``sparsity``, ``gain_per_sample`` (row i
    of stage k is scaled by gain_per_sample ** shifts[k, i]).  The delay tensors hold integers in ``dtype`` and may be replaced;
    they are read when ``forward`` runs."""

    def __init__(self, N: int, n_stages: int = 3, sparsity: int = 3, gain_per_sample: float = 0.9999, pulse_size: int = 1,
                 m_L: Optional[torch.Tensor] = None, m_R: Optional[torch.Tensor] = None, device: Optional[str] = "cpu",
                 dtype: torch.dtype = torch.float32):
        super().__init__()
        self.n_stages = n_stages
        self.sparsity = sparsity
        self.gain_per_sample = gain_per_sample
        self.device = device
        self.dtype = dtype
        self.m_L = torch.zeros(N, device=device, dtype=dtype) if m_L is None else m_L
        self.m_R = torch.zeros(N, device=device, dtype=dtype) if m_R is None else m_R
        self.sparsity_vect = torch.ones(n_stages, device=device, dtype=dtype)
        self.sparsity_vect[0] = sparsity
        self.shifts = get_random_shifts(N, self.sparsity_vect, pulse_size, dtype=dtype)

    def fir_length(self) -> int:
        """taps of the FIR matrix: 1 + the longest way through the stage delays + the longest outer delays"""
        return 1 + int(self.shifts.max(dim=1).values.sum()) + int(self.m_L.max()) + int(self.m_R.max())

    def forward(self, U):
        assert U.shape[0] == self.n_stages + 1, "The input matrix must have n_stages+1 stages"
        assert U.shape[1] == U.shape[2], "The input matrix must be square"
        V = U[0].unsqueeze(-1)                                                   # (N, N, 1)
        for k in range(1, self.n_stages + 1):
            shift = self.shifts[k - 1]
            gain = (self.gain_per_sample ** shift.to(torch.float64)).to(device=U.device, dtype=U.dtype)
            V = torch.einsum("ik,kjt->ijt", U[k] * gain, _delay_taps(V, shift, 0))
        V = _delay_taps(_delay_taps(V, self.m_L, 0), self.m_R, 1)
        return V.permute(2, 0, 1)
