"""Generates tests/golden/srbench_skimage.npz with scikit-image 0.18.3: one RGB u8 pair of 96 x 120 and, at crop borders 0 and
4, scikit-image's PSNR and Gaussian SSIM of the cropped pair
  * on the float64 BT.601 luma plane Y = (65481 R + 128553 G + 24966 B + 4080000) / 255000     (psnr_y, ssim_y),
  * on MATLAB's rounded u8 luma floor((2 X + 255000) / 510000), as float64                      (psnr_y_round, ssim_y_round),
  * on the RGB channels: PSNR over all elements, SSIM as the mean of the three channels' means  (psnr_rgb, ssim_rgb).
These are the three modes of include/sr_hip.h's sr_bench_u8.  Each array holds one value per crop border, in the order of
`crop_borders`.

Run with an interpreter that has scikit-image 0.18.3:
    python tests/golden/make_srbench_golden.py
Inputs are stored next to the expected values, so nothing depends on RNG stream stability.
"""
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings("ignore")
from skimage import __version__ as skv
from skimage.metrics import peak_signal_noise_ratio as psnr
from skimage.metrics import structural_similarity as ssim

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _srbench_ref as R


def gauss(x, y):
    return float(ssim(x, y, gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=255, multichannel=False))


a, b = R.img_pair(np.random.default_rng(20260519), 96, 120, 3)
CROPS = (0, 4)
out = {k: [] for k in ("psnr_y", "ssim_y", "psnr_y_round", "ssim_y_round", "psnr_rgb", "ssim_rgb")}
for cb in CROPS:
    ac, bc = R.crop(a, cb), R.crop(b, cb)
    ya, yb = R.x_int(ac) / 255000.0, R.x_int(bc) / 255000.0
    out["psnr_y"].append(float(psnr(ya, yb, data_range=255)))
    out["ssim_y"].append(gauss(ya, yb))
    ra, rb = R.y_round(ac).astype(np.float64), R.y_round(bc).astype(np.float64)
    out["psnr_y_round"].append(float(psnr(ra, rb, data_range=255)))
    out["ssim_y_round"].append(gauss(ra, rb))
    fa, fb = ac.astype(np.float64), bc.astype(np.float64)
    out["psnr_rgb"].append(float(psnr(fa, fb, data_range=255)))
    out["ssim_rgb"].append(float(np.mean([gauss(fa[..., c], fb[..., c]) for c in range(3)])))
dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "srbench_skimage.npz")
np.savez_compressed(dst, a=a, b=b, crop_borders=np.array(CROPS), skimage_version=np.array(skv),
                    **{k: np.array(v, dtype=np.float64) for k, v in out.items()})
print("wrote", dst, out)
