"""Time flamo_amd.optimize.loss.mss_loss, forward plus backward, eager, on two seconds at 48 kHz -- one response, (1, 96000, 1),
and a batch of four with two channels, (4, 96000, 2) -- with the default six resolutions 128 .. 4096, in float32 and float64,
in the plain and the "yamamoto" form, beside the same criterion in plain torch (the class's own `_torch_forward`, the
reference's dense-basis formulation, run on the same GPU).

    python tools/bench_mss.py [--min-seconds 0.5] [--limit 60] [--nfft 128 4096]

The two are alternated in one process after a warm-up; every measurement is a pair of device events around at least
``--min-seconds`` of back-to-back steps, and the best of three rounds is kept.  Every timed step runs under a time limit of its
own: a measurement that has not ended after ``--limit`` seconds of wall time raises instead of going on.  One JSON line per
case, with the two losses, their relative difference, the l2-relative difference of the two gradients and the library's
launch counts."""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import flamo_amd  # noqa: E402,F401  (before the first torch.cuda call)
import torch  # noqa: E402

from flamo_amd import _lib  # noqa: E402
from flamo_amd.optimize.loss import mss_loss  # noqa: E402
from bench_mrstft import measure  # noqa: E402

SHAPES = ((1, 96000, 1), (4, 96000, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--limit", type=float, default=60.0)
    ap.add_argument("--nfft", type=int, nargs="+", default=[128, 256, 512, 1024, 2048, 4096])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    flat = [v for n in args.nfft for v in (n, n // 4)]
    res = (ctypes.c_int * len(flat))(*flat)
    launches = [_lib.lib().fl_mss_launches(len(args.nfft), res, b) for b in (0, 1)]
    for shape in SHAPES:
        T = shape[1]
        for dtype in (torch.float32, torch.float64):
            for form in (None, "yamamoto"):
                torch.manual_seed(0)
                env = 10 ** (-3.0 * torch.arange(T, device=dev, dtype=torch.float64)[None, :, None] / T)
                y = (torch.randn(shape, device=dev, dtype=torch.float64) * env).to(dtype).requires_grad_(True)
                t = (torch.randn(shape, device=dev, dtype=torch.float64) * env ** 0.875).to(dtype)
                crit = mss_loss(nfft=args.nfft, form=form, device="cuda")
                assert crit._on_kernels(y, t)

                def hip_step():
                    y.grad = None
                    crit(y, t).backward()

                def torch_step():
                    y.grad = None
                    crit._torch_forward(y, t).backward()

                hip_step()
                l_hip, g_hip = crit(y, t).item(), y.grad.clone()
                torch_step()
                l_torch, g_torch = crit._torch_forward(y, t).item(), y.grad.clone()
                for _ in range(3):
                    hip_step()
                    torch_step()
                best = {"hip": float("inf"), "torch": float("inf")}
                for _ in range(args.rounds):
                    best["hip"] = min(best["hip"], measure(hip_step, args.min_seconds, args.limit))
                    best["torch"] = min(best["torch"], measure(torch_step, args.min_seconds, args.limit))
                print(json.dumps(dict(shape=list(shape), nfft=args.nfft, dtype=str(dtype)[6:], form=form,
                                      launches_fwd=launches[0], launches_bwd=launches[1],
                                      hip_ms=round(best["hip"] * 1e3, 4), torch_ms=round(best["torch"] * 1e3, 4),
                                      speedup=round(best["torch"] / best["hip"], 2), loss_hip=l_hip, loss_torch=l_torch,
                                      loss_rel_diff=abs(l_hip - l_torch) / abs(l_torch),
                                      grad_rel_diff=float((g_hip - g_torch).norm() / g_torch.norm()))), flush=True)
                del y, t, g_hip, g_torch, crit
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
