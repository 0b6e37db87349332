"""Host-side helpers of the criteria (flamo/optimize/utils.py)."""
from typing import Optional

import torch


def generate_partitions(tensor: torch.Tensor, n_samples: int, n_sets: int, seed: Optional[int] = None) -> torch.Tensor:
    """``n_sets`` random shuffles of ``tensor``, each cut into ``len(tensor) // n_samples`` rows of ``n_samples`` items (the rest
    of a shuffle is left out), stacked: (n_sets * (len // n_samples), n_samples).  One ``torch.randperm`` per set."""
    if seed is not None:
        torch.manual_seed(seed)
    length = len(tensor)
    rows = length // n_samples
    if length % n_samples != 0:
        print("Warning: Tensor length is not divisible by n_samples so there will be some samples left out.")
    sets = [tensor[torch.randperm(length)][: rows * n_samples].reshape(rows, n_samples) for _ in range(n_sets)]
    return torch.cat(sets, dim=0)
