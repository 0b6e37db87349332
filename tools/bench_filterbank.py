"""Time auxiliary.filterbank.FilterBank and flamo_amd.optimize.subband_edc_loss, forward plus backward, on one room impulse
response (1, 96000, 1) -- the octave bank (fraction=1, 11 bands; the criterion's own 9 bands) and the third-octave bank
(fraction=3, 30 bands) -- in float32 and float64, beside the same torch lines (the classes' own ``_torch_forward``) run on the
same GPU.

    python tools/bench_filterbank.py [--min-seconds 0.5]

The two are alternated in one process after a warm-up; every measurement is a pair of device events around at least
``--min-seconds`` of back-to-back steps, and the best of three rounds is kept.  ``launches`` is the number of device kernels of
one step (forward plus backward), counted by torch.profiler on one extra step of each (null where the profiler is not
available).  One JSON line per (what, bank, precision)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import flamo_amd  # noqa: E402,F401  (before the first torch.cuda call)
import torch  # noqa: E402

from flamo_amd.auxiliary import FilterBank  # noqa: E402
from flamo_amd.optimize import subband_edc_loss  # noqa: E402

SHAPE = (1, 96000, 1)
THIRD_OCTAVE_63_16K = [63, 80, 100, 125, 160, 200, 250, 315, 400, 500, 630, 800, 1000, 1250, 1600, 2000, 2500, 3150, 4000, 5000, 6300,
                       8000, 10000, 12500, 16000]


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


def count_launches(step):
    """device kernels of one step, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower()
                and "memset" not in e.name.lower())
        return n or None
    except Exception:      # noqa: BLE001  (a build without the profiler: the times stand without the count)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for what in ("FilterBank", "subband_edc_loss"):
        for fraction in (1, 3):
            for dtype in (torch.float32, torch.float64):
                torch.manual_seed(0)
                T = SHAPE[1]
                t_ax = torch.arange(T, device=dev, dtype=torch.float64)[None, :, None] / T
                y = (torch.randn(SHAPE, device=dev, dtype=torch.float64) * torch.exp(-6.9 * 1.3 * t_ax)).to(dtype).requires_grad_(True)
                t = (torch.randn(SHAPE, device=dev, dtype=torch.float64) * torch.exp(-6.9 * t_ax)).to(dtype)
                if what == "FilterBank":
                    mod = FilterBank(fraction=fraction, backend="torch")
                    K = len(mod.get_center_frequencies())
                    cot = torch.randn((SHAPE[0], T, SHAPE[2], K), device=dev, dtype=dtype)
                    hip = lambda: (mod(y) * cot).sum()                      # noqa: E731
                    ref = lambda: (mod._torch_forward(y) * cot).sum()        # noqa: E731
                else:
                    mod = subband_edc_loss(center_frequencies=None if fraction == 1 else THIRD_OCTAVE_63_16K, energy_norm=True,
                                           convergence=True, device="cuda")
                    K = len(mod.center_frequencies)
                    hip = lambda: mod(y, t)                                  # noqa: E731
                    ref = lambda: mod._torch_forward(y, t)                   # noqa: E731

                def hip_step():
                    y.grad = None
                    hip().backward()

                def torch_step():
                    y.grad = None
                    ref().backward()

                hip_step()
                v_hip, g_hip = hip().item(), y.grad.clone()
                torch_step()
                v_torch, g_torch = ref().item(), y.grad.clone()
                for _ in range(3):
                    hip_step()
                    torch_step()
                best = {"hip": float("inf"), "torch": float("inf")}
                for _ in range(args.rounds):
                    best["hip"] = min(best["hip"], measure(hip_step, args.min_seconds))
                    best["torch"] = min(best["torch"], measure(torch_step, args.min_seconds))
                launches = (None, None) if args.no_launch_count else (count_launches(hip_step), count_launches(torch_step))
                print(json.dumps(dict(what=what, shape=list(SHAPE), bands=K, dtype=str(dtype)[6:], hip_ms=round(best["hip"] * 1e3, 4),
                                      torch_ms=round(best["torch"] * 1e3, 4), speedup=round(best["torch"] / best["hip"], 2),
                                      launches_hip=launches[0], launches_torch=launches[1], value_hip=v_hip, value_torch=v_torch,
                                      grad_rel_diff=float((g_hip - g_torch).norm() / g_torch.norm()))), flush=True)


if __name__ == "__main__":
    main()
