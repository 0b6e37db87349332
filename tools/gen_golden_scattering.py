"""Golden vectors of ScatteringMatrix / VelvetNoiseMatrix from the REFERENCE (float64, CPU), where it is checked out.

    python tools/gen_golden_scattering.py        # writes tests/golden/scat_*.npz and velvet_*.npz

Each file holds one module: the seed it was built under, ``param``, the delays the reference drew (``shifts``, ``m_L``,
``m_R``), the tap count of its FIR matrix (``L``) and, at the bins listed in ``bins`` (all of them where the file stays small,
otherwise the spectrum's ends, the bins around the wavefront boundaries of the kernels and random ones),

  * ``H_ref``     the reference's own ``freq_response(param)`` -- its envelope gamma ** arange(L) is float32 even in a
                  float64 module (L is a Python float), which costs 1e-6 where alias_decay_db != 0;
  * ``H_f64env``  the reference's own ``map_filter(map(param))`` FIR matrix times the float64 envelope, through rfft: the truth;
  * ``C``         the rows of the cotangent.

The cotangent covers EVERY bin: C = (a + i b) with a, b = RandomState(seed).standard_normal((2, M, N, N)) (the legacy stream,
frozen by numpy's compatibility policy); ``grad`` is the gradient of ``param`` under Re<C, H_f64env> over all bins, float64.
scat_n4 also holds a small feedback delay network around the module (see ``gen_fdn``).  Arrays and settings only.
The class name is stored under ``module`` in ``meta``: the key ``cls`` marks the fixtures of tools/gen_golden.py, which the
module-parity tests collect by it and rebuild from a ``kwargs`` entry these files do not have.
"""
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refimport  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
F64 = torch.float64
ROW_BUDGET = 150_000       # bytes of the three per-bin arrays of one file

# name, class, N, stages, nfft, alias_decay_db, gain_per_sample, constructor extras, seed
CASES = [
    ("scat_n2", "ScatteringMatrix", 2, 2, 960, 0.0, 1.0, dict(sparsity=3, pulse_size=2), 13),
    ("scat_n4", "ScatteringMatrix", 4, 4, 960, 30.0, 0.9999, dict(sparsity=3, pulse_size=1), 12),
    ("scat_n6", "ScatteringMatrix", 6, 3, 1500, 30.0, 0.999, dict(sparsity=2, pulse_size=1), 11),
    ("scat_n16", "ScatteringMatrix", 16, 3, 4096, 60.0, 0.9999, dict(sparsity=3, pulse_size=1), 14),
    ("velvet_n4", "VelvetNoiseMatrix", 4, 3, 2048, 30.0, 0.9999, dict(density=0.2), 15),
]


def cotangent(seed, M, N):
    ab = np.random.RandomState(seed).standard_normal((2, M, N, N))
    return ab[0] + 1j * ab[1]


def pick_bins(seed, M, N):
    rows = min(M, ROW_BUDGET // (3 * 16 * N * N))
    if rows >= M:
        return np.arange(M)
    fixed = [b for b in (0, 1, 63, 64, 65, 127, 128, 255, 256, 257, M - 2, M - 1) if 0 <= b < M][:rows]
    rest = np.random.RandomState(seed + 1000).permutation(M)
    chosen = list(dict.fromkeys(fixed + [int(b) for b in rest]))[:rows]
    return np.sort(np.asarray(chosen))


def f64env_response(mod, param, nfft, db):
    """the reference's FIR matrix, the envelope in float64"""
    fir = mod.map_filter(mod.map(param))
    gamma = 10.0 ** (-abs(db) / nfft / 20.0)
    env = torch.tensor(gamma, dtype=F64) ** torch.arange(fir.shape[0], dtype=F64)
    return torch.fft.rfft(fir * env.view(-1, 1, 1), n=nfft, dim=0), fir.shape[0]


def build(dsp, cls, N, stages, nfft, db, g, extra, seed):
    torch.manual_seed(seed)
    m_L = torch.randint(1, 12, (N,)).to(F64)
    m_R = torch.randint(1, 12, (N,)).to(F64)
    kw = dict(size=(stages, N, N), nfft=nfft, gain_per_sample=g, m_L=m_L, m_R=m_R, alias_decay_db=db, dtype=F64, **extra)
    if cls == "ScatteringMatrix":
        kw["requires_grad"] = True
    torch.manual_seed(seed)          # the constructor's draws (param, then the stage delays) start from the stored seed
    return getattr(dsp, cls)(**kw)


def gen_fdn(mod, nfft, db, seed):
    """|c (I - D S)^-1 D b| per bin: input gains b (4, 1), integer delay lines D, the scattering matrix S in the feedback path,
    output gains c (1, 4), driven by a unit impulse -- Shell(FFT, Series(Gain, Recursion(parallelDelay, ScatteringMatrix), Gain),
    magnitude) -- with the float64 envelope; gradients under sum(w * out) for a stored weight w."""
    N, M = 4, nfft // 2 + 1
    rs = np.random.RandomState(seed + 2000)
    b = torch.tensor(rs.standard_normal((N, 1)), dtype=F64, requires_grad=True)
    c = torch.tensor(rs.standard_normal((1, N)), dtype=F64, requires_grad=True)
    w = torch.tensor(rs.standard_normal(M), dtype=F64)
    delays = torch.tensor([59.0, 97.0, 131.0, 151.0], dtype=F64)
    gamma = 10.0 ** (-abs(db) / nfft / 20.0)
    k = torch.arange(M, dtype=torch.int64).view(-1, 1)
    phase = -2 * math.pi * ((k * delays.to(torch.int64).view(1, -1)) % nfft).to(F64) / nfft
    D = torch.diag_embed(torch.polar((gamma ** delays).view(1, -1).expand(M, -1).contiguous(), phase))
    S, _ = f64env_response(mod, mod.param, nfft, db)
    eye = torch.eye(N, dtype=torch.complex128)
    loop = torch.linalg.solve(eye - D @ S, D)
    out = torch.abs(c.to(torch.complex128) @ loop @ b.to(torch.complex128)).reshape(M)
    gb, gc, gp = torch.autograd.grad((out * w).sum(), [b, c, mod.param])
    return dict(fdn_b=b, fdn_c=c, fdn_w=w, fdn_delays=delays, fdn_out=out, fdn_grad_b=gb, fdn_grad_c=gc, fdn_grad_param=gp)


def main():
    dsp, _ = refimport.load()
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, cls, N, stages, nfft, db, g, extra, seed in CASES:
        mod = build(dsp, cls, N, stages, nfft, db, g, extra, seed)
        M = nfft // 2 + 1
        H_ref = mod.freq_response(mod.param).detach()
        H, L = f64env_response(mod, mod.param, nfft, db)
        C = torch.from_numpy(cotangent(seed, M, N))
        arrays = {}
        if mod.param.requires_grad:
            (arrays["grad"],) = torch.autograd.grad(torch.sum(torch.real(H * torch.conj(C))), [mod.param], retain_graph=True)
        bins = pick_bins(seed, M, N)
        arrays.update(param=mod.param, shifts=mod.map_filter.shifts, m_L=mod.map_filter.m_L, m_R=mod.map_filter.m_R,
                      bins=bins, H_ref=H_ref[bins], H_f64env=H.detach()[bins], C=C[bins])
        if name == "scat_n4":
            arrays.update(gen_fdn(mod, nfft, db, seed))
        meta = dict(module=cls, N=N, stages=stages, nfft=nfft, alias_decay_db=db, gain_per_sample=g, seed=seed, L=int(L), **extra)
        arrays = {k: (v.detach().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in arrays.items()}
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), **arrays)
        size = os.path.getsize(path)
        total += size
        print(f"{name:12s} {size / 1024:7.1f} KiB  L = {int(L):5d}  rows = {len(bins):4d} of {M}  shifts = {mod.map_filter.shifts.tolist()}")
        assert size < 200_000, name
    print(f"total {total / 1024:.1f} KiB")
    assert total < 1_000_000


if __name__ == "__main__":
    main()
