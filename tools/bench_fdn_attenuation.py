"""Time the trainable delay-scaled attenuation filters of flamo_amd.auxiliary.reverb, response forward plus backward, at
N = 16 delay lines and nfft = 192000 in float32: parallelFDNGEQ at octave_interval 1 and 3 and parallelFirstOrderShelving,
on the design kernels (csrc/fdnatt.hip) beside the same classes on their torch lines (``fold_map=False``: the sections as
torch ops in front of the same cascade kernels), on the same GPU.

    python tools/bench_fdn_attenuation.py [--min-seconds 0.5]

The two are alternated in one process after a warm-up; every measurement is a pair of device events around at least
``--min-seconds`` of back-to-back steps, and the best of three rounds is kept.  One JSON line per class, with the
l2-relative difference of the two responses and of the two gradients."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import flamo_amd  # noqa: E402,F401  (before the first torch.cuda call)
import torch  # noqa: E402

from flamo_amd.auxiliary import reverb  # noqa: E402

N, NFFT = 16, 192000
DELAYS = [887, 911, 941, 1699, 1951, 2053, 977, 1129, 1237, 1361, 1523, 1013, 1787, 1871, 2203, 2399]


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
    delays = torch.tensor(DELAYS, dtype=torch.float64)
    kw = dict(nfft=NFFT, delays=delays, alias_decay_db=30.0, requires_grad=True, device=dev, dtype=torch.float32)
    builders = [("parallelFDNGEQ/octave_interval=1", lambda **k: reverb.parallelFDNGEQ(octave_interval=1, **kw, **k)),
                ("parallelFDNGEQ/octave_interval=3", lambda **k: reverb.parallelFDNGEQ(octave_interval=3, **kw, **k)),
                ("parallelFirstOrderShelving", lambda **k: reverb.parallelFirstOrderShelving(**kw, **k))]
    for name, build in builders:
        torch.manual_seed(0)
        hip, lines = build(), build(fold_map=False)
        value = torch.tensor([1.5, 0.6]) if hip.param.shape == (2,) else torch.rand(hip.param.shape) * 2.0 + 0.5
        hip.assign_value(value.to(dev))
        lines.assign_value(value.to(dev))
        W = torch.randn(NFFT // 2 + 1, N, dtype=torch.complex64, device=dev)

        def step_of(mod):
            def step():
                mod.param.grad = None
                torch.sum(torch.real(mod.freq_response(mod.param) * W)).backward()
            return step

        hip_step, torch_step = step_of(hip), step_of(lines)
        for _ in range(3):
            hip_step()
            torch_step()
        with torch.no_grad():
            H_hip, H_lines = hip.freq_response(hip.param), lines.freq_response(lines.param)
        best = {"hip": float("inf"), "torch": float("inf")}
        for _ in range(args.rounds):
            best["hip"] = min(best["hip"], measure(hip_step, args.min_seconds))
            best["torch"] = min(best["torch"], measure(torch_step, args.min_seconds))
        print(json.dumps(dict(module=name, N=N, nfft=NFFT, dtype="float32", hip_ms=round(best["hip"] * 1e3, 4),
                              torch_lines_ms=round(best["torch"] * 1e3, 4), speedup=round(best["torch"] / best["hip"], 2),
                              response_rel_diff=float((H_hip - H_lines).norm() / H_lines.norm()),
                              grad_rel_diff=float((hip.param.grad - lines.param.grad).norm() / lines.param.grad.norm()))),
              flush=True)


if __name__ == "__main__":
    main()
