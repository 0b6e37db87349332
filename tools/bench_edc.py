"""Time flamo_amd.optimize.edc_loss, forward plus backward, on the two users' shapes -- a batch of multichannel responses
(32, 96000, 8) and one long response (1, 192000, 1) -- in float32 and float64, beside the same criterion in plain torch
(the class's own host lines, run on the same GPU).

    python tools/bench_edc.py [--min-seconds 0.5]

The two are alternated in one process after a warm-up; every measurement is a pair of device events around at least
``--min-seconds`` of back-to-back steps, and the best of three rounds is kept.  The algorithmic traffic is counted from the
shapes (`algorithmic_bytes`: the signal-sized passes of the HIP path); the figure printed is those bytes over the measured
time, not a measured bandwidth.  One JSON line per (shape, precision)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import flamo_amd  # noqa: E402,F401  (before the first torch.cuda call)
import torch  # noqa: E402

from flamo_amd.optimize import edc_loss  # noqa: E402

SHAPES = ((32, 96000, 8), (1, 192000, 1))


def algorithmic_bytes(shape, itemsize):
    """signal-sized passes of the HIP path, in bytes: the target is read twice (tile sums, curve) and its curve written once
    and read once; the prediction is read twice forward (tile sums, loss pass) and once backward; w is written once and read
    once; the gradient is written once -- ten passes over B*T*N elements (the per-tile sums are a 512th of one)"""
    B, T, N = shape
    return 10 * B * T * N * itemsize


def measure(step, min_seconds):
    """seconds per step: device events around enough back-to-back steps to last min_seconds"""
    n = 1
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            step()
        b.record()
        b.synchronize()
        s = a.elapsed_time(b) * 1e-3
        if s >= min_seconds:
            return s / n
        n = max(n + 1, int(n * min(10.0, 1.3 * min_seconds / max(s, 1e-6))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for shape in SHAPES:
        for dtype in (torch.float32, torch.float64):
            torch.manual_seed(0)
            B, T, N = shape
            env = 10 ** (-4.0 * torch.arange(T, device=dev, dtype=torch.float64)[None, :, None] / T)
            y = (torch.randn(shape, device=dev, dtype=torch.float64) * env).to(dtype).requires_grad_(True)
            t = (torch.randn(shape, device=dev, dtype=torch.float64) * env ** 0.875).to(dtype)
            crit = edc_loss(is_broadband=True, energy_norm=True, convergence=True, clip=True, device="cuda")

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
                best["hip"] = min(best["hip"], measure(hip_step, args.min_seconds))
                best["torch"] = min(best["torch"], measure(torch_step, args.min_seconds))
            nbytes = algorithmic_bytes(shape, y.element_size())
            print(json.dumps(dict(shape=list(shape), dtype=str(dtype)[6:], hip_ms=round(best["hip"] * 1e3, 4),
                                  torch_ms=round(best["torch"] * 1e3, 4), speedup=round(best["torch"] / best["hip"], 2),
                                  algorithmic_mb=round(nbytes / 1e6, 2), algorithmic_gb_per_s=round(nbytes / best["hip"] / 1e9, 1),
                                  loss_hip=l_hip, loss_torch=l_torch,
                                  grad_rel_diff=float((g_hip - g_torch).norm() / g_torch.norm()))), flush=True)


if __name__ == "__main__":
    main()
