"""Response of a scattering feedback matrix, forward + backward, on its two routes (MI355X).

    python tools/bench_scattering.py [--sizes 8 16] [--rounds 5] [--iters 20]

For N in --sizes, K+1 = 4 stages, sparsity 3, nfft = 96000, float32:

  * per_bin    ops.scatter_response(U) and its backward for a full cotangent (csrc/scattering.hip);
  * fir        dsp.Filter holding the IDENTICAL taps (the module's own map_filter(U), L x N x N): rfft of the FIR matrix and its
               backward -- what the library offered before the per-bin kernels, and without the cost of building the taps;
  * fir_module the module's own FIR route (SCATTERING_PER_BIN off): the taps built from U by ScatteringMapping, then the same.

Device events around `iters` calls, `rounds` windows per route, the routes alternating; the median window is reported.
`fwd_us` is the per-bin forward alone (back-to-back launches under no_grad) and `hbm_write_fraction` its M N^2 complex64
output over that time against 8 TB/s.  Needs a GPU: there is no host path to time.  One JSON line per size.
"""
import argparse
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BYTES_PER_S = 8e12


def window(fn, iters):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters       # us per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--nfft", type=int, default=96000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scattering: no GPU (timings are taken on the device only)")
    from flamo_amd import ops
    from flamo_amd.processor import dsp
    dev, nfft, M = torch.device("cuda:0"), args.nfft, args.nfft // 2 + 1
    for N in args.sizes:
        torch.manual_seed(N)
        mL, mR = torch.randint(1, 12, (N,)).float(), torch.randint(1, 12, (N,)).float()
        mod = dsp.ScatteringMatrix(size=(4, N, N), nfft=nfft, sparsity=3, m_L=mL, m_R=mR, requires_grad=True, alias_decay_db=30.0,
                                   device=dev, dtype=torch.float32)
        mf = mod.map_filter
        assert mod._per_bin_now(mod.param)
        U = mod.map(mod.param).detach().requires_grad_(True)
        consts = ops.scatter_consts(mf.shifts, mf.m_L, mf.m_R, mf.gain_per_sample, mod._gamma_f, nfft, torch.float32, dev)
        C = torch.randn(M, N, N, dtype=torch.complex64, device=dev)
        with torch.no_grad():
            taps = mf(U)
        flt = dsp.Filter(size=tuple(taps.shape), nfft=nfft, requires_grad=True, alias_decay_db=30.0, device=dev, dtype=torch.float32)
        flt.assign_value(taps)

        def per_bin():
            U.grad = None
            ops.scatter_response(U, mf.shifts, mf.m_L, mf.m_R, mf.gain_per_sample, mod._gamma_f, nfft, consts=consts).backward(C)

        def fir():
            flt.param.grad = None
            flt.freq_response(flt.param).backward(C)

        def fir_module():
            mod.param.grad = None
            dsp.SCATTERING_PER_BIN = False
            try:
                mod.freq_response(mod.param).backward(C)
            finally:
                dsp.SCATTERING_PER_BIN = True

        def fwd():
            with torch.no_grad():
                ops.scatter_response(U, mf.shifts, mf.m_L, mf.m_R, mf.gain_per_sample, mod._gamma_f, nfft, consts=consts)

        routes = dict(per_bin=per_bin, fir=fir, fir_module=fir_module, fwd=fwd)
        with torch.no_grad():       # the routes compute the same thing
            Ha = ops.scatter_response(U, mf.shifts, mf.m_L, mf.m_R, mf.gain_per_sample, mod._gamma_f, nfft, consts=consts)
            Hb = flt.freq_response(flt.param)
            diff = (Ha - Hb).abs().max().item()
        del Ha, Hb
        for fn in routes.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                times[k].append(window(fn, args.iters))
        med = {k: statistics.median(v) for k, v in times.items()}
        out_bytes = M * N * N * 8
        print(json.dumps(dict(N=N, stages=4, nfft=nfft, taps=int(taps.shape[0]), dtype="float32",
                              per_bin_us=round(med["per_bin"], 1), fir_us=round(med["fir"], 1), fir_module_us=round(med["fir_module"], 1),
                              fwd_us=round(med["fwd"], 1), out_bytes=out_bytes,
                              hbm_write_fraction=round(out_bytes / (med["fwd"] * 1e-6) / HBM_BYTES_PER_S, 3),
                              spread_us={k: [round(min(v), 1), round(max(v), 1)] for k, v in times.items()},
                              routes_max_abs_diff=diff)), flush=True)


if __name__ == "__main__":
    main()
