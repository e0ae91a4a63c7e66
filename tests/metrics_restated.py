"""The contract of include/eonerf_metrics.h in numpy fp64, written from the reference's metrics.py:17-22 (uncertainty_aware_loss) and
:60-69 (mse, psnr).  Imports nothing from the product path: the tests hold the library to THIS, and this to golden G6 (the
reference's own outputs)."""
import numpy as np

NAMES = ("loss", "coarse_color", "coarse_logbeta", "mse", "psnr", "n")


def image_metrics(pred, gt, beta=None):
    """pred, gt [n, 3], beta [n, 1] or [n] or None (any float dtype; widened to fp64 first) -> float64[6] =
    loss, coarse_color, coarse_logbeta, mse, psnr, n.  IEEE edge cases as torch's: 0 / 0, log(0), log10(0) are not errors."""
    pred = np.asarray(pred, dtype=np.float64).reshape(-1, 3)
    gt = np.asarray(gt, dtype=np.float64).reshape(-1, 3)
    assert pred.shape == gt.shape and pred.shape[0] > 0
    n = pred.shape[0]
    out = np.full(6, np.nan)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        sq = (pred - gt) ** 2
        if beta is not None:
            beta = np.asarray(beta, dtype=np.float64).reshape(n, 1)
            out[1] = (sq / (2 * beta ** 2)).mean()              # metrics.py:18
            out[2] = (3 + np.log(beta).mean()) / 2              # :19
            out[0] = out[1] + out[2]                            # :20
        out[3] = sq.mean()                                      # :61-65
        out[4] = -10 * np.log10(out[3])                         # :69
    out[5] = n
    return out
