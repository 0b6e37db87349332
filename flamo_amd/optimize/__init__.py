"""The criteria of flamo.optimize.loss that sit directly on the hot path's output, evaluated by the library's kernels."""
from .loss import (AveragePower, MultiResoSTFT, edc_loss, edr_loss, masked_mse_loss, mel_mss_loss, mse_loss, sparsity_loss,  # noqa: F401
                   subband_edc_loss)
from .utils import generate_partitions  # noqa: F401
