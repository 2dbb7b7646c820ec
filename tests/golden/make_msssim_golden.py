"""Generates tests/golden/msssim_skimage.npz with scikit-image 0.18.3: one gray u8 pair of 177 x 191 and the Gaussian SSIM mean
scikit-image gives at each of the five MS-SSIM levels, on the exactly pooled float64 planes (2 x 2 means, a last odd row or
column dropped; sums of 4^j u8 values divided by 4^j are exact in float64).  These are the S_j of include/sr_hip.h's MS-SSIM;
scikit-image does not expose cs, so CS_j is not in here.

Run with the interpreter that has scikit-image:
    /opt/conda/bin/python3.9 tests/golden/make_msssim_golden.py
Inputs are stored next to the expected values, so nothing depends on RNG stream stability.
"""
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings("ignore")
from skimage import __version__ as skv
from skimage.metrics import structural_similarity as ssim

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _msssim_ref as R

a, b = R.img_pair(np.random.default_rng(20260313), 177, 191)
pa, pb = R.planes(a, 5), R.planes(b, 5)
s = [ssim(x, y, gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=255, multichannel=False)
     for x, y in zip(pa, pb)]
dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "msssim_skimage.npz")
np.savez_compressed(dst, a=a, b=b, s=np.array(s, dtype=np.float64), skimage_version=np.array(skv))
print("wrote", dst, s, [p.shape for p in pa])
