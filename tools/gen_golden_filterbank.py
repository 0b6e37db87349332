"""Golden vectors of auxiliary.filterbank.FilterBank from the REFERENCE (float64, CPU), where it is checked out.

    python tools/gen_golden_filterbank.py        # writes tests/golden/filterbank_*.npz

Each file holds one bank under ``backend="torch"``: a seeded float64 input ``x`` (B, T, N), the reference's centre frequencies
(``centers``), its band responses ``freqz`` (K, T // 2 + 1) -- scipy's ``sosfreqz`` of its second-order sections, sampled at
pi k / M -- and its output ``y`` (B, 2 (T // 2), N, K).  ``meta`` has the constructor arguments and, for the bank with the
low- and high-pass branches, the frequencies handed to ``set_center_frequencies``.  Arrays and settings only.  The class name is
stored under ``module``: the key ``cls`` marks the fixtures of tools/gen_golden.py.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refimport  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")

# name, input shape, constructor arguments, frequencies for set_center_frequencies (or None), seed
CASES = [
    ("filterbank_octave", (1, 480, 2), dict(fraction=1), None, 21),
    ("filterbank_third", (1, 481, 1), dict(fraction=3), None, 22),
    ("filterbank_lowhigh", (1, 480, 2), dict(fraction=1), [0, 1000, 24000], 23),
]


def main():
    refimport.load()
    from flamo.auxiliary.filterbank import FilterBank
    os.makedirs(OUT, exist_ok=True)
    for name, shape, kwargs, centers, seed in CASES:
        bank = FilterBank(backend="torch", **kwargs)
        if centers is not None:
            bank.set_center_frequencies(centers)
        x = torch.from_numpy(np.random.RandomState(seed).standard_normal(shape))
        y = bank(x)
        assert y.dtype == torch.float64 and bank.freqz.shape == (len(bank.get_center_frequencies()), shape[1] // 2 + 1)
        meta = dict(module="FilterBank", order=bank._order, sample_rate=bank._sample_rate, seed=seed, set_centers=centers, **kwargs)
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, meta=json.dumps(meta), x=x.numpy(), centers=np.asarray(bank.get_center_frequencies(), dtype=np.float64),
                            freqz=bank.freqz, y=y.numpy())
        size = os.path.getsize(path)
        print(f"{name:20s} {size / 1024:7.1f} KiB  K = {y.shape[-1]:2d}  y {tuple(y.shape)}")
        assert size < 680_000, name


if __name__ == "__main__":
    main()
