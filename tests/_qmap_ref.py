"""NumPy restatement of the per-cell quality map (sr_quality_map_u8): the full SSIM maps S(y, x) of the three variants --
the algebra of oracle_np.ssim before its .mean(), built from the oracle's own filters and kernels -- the per-pixel squared
error, and the binning of a map by two edge lists.  Valid regions: uniform-7 cropped by 3, gauss-11 by 5, simple the whole
map."""
import numpy as np

from oracle import oracle_np as onp

PAD = {"uniform": 3, "gauss": 5, "simple": 0}


def img_pair(rng, h, w, cn=3):
    """tests/test_gpu_float_inputs.py::_img twice: one smooth field, two independent draws of +-12 noise."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = (128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0))[..., None]
    a = np.clip(base + rng.integers(-12, 13, (h, w, cn)), 0, 255).astype(np.uint8)
    b = np.clip(base + rng.integers(-12, 13, (h, w, cn)), 0, 255).astype(np.uint8)
    return (a, b) if cn == 3 else (a[..., 0], b[..., 0])


def gray(img, shift=15):
    return onp.rgb2gray_u8(img, shift) if img.ndim == 3 else img


def ssim_map(g1, g2, mode, data_range=255.0):
    """The SSIM map of two gray images over the whole frame (samples outside the valid region included)."""
    x, y = g1.astype(np.float64), g2.astype(np.float64)
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    if mode == "simple":
        c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        k = onp.cv_gaussian_kernel(11, 1.5)
        f = lambda a: onp._filter_sep(a, k, "reflect101")
        mu1, mu2 = f(x), f(y)
        mu1_sq, mu2_sq, mu12 = mu1 ** 2, mu2 ** 2, mu1 * mu2
        s1, s2, s12 = f(x ** 2) - mu1_sq, f(y ** 2) - mu2_sq, f(x * y) - mu12
        return ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu1_sq + mu2_sq + c1) * (s1 + s2 + c2))
    if mode == "uniform":
        k, cov_norm = np.full(7, 1.0 / 7.0), 49.0 / 48.0
    else:
        k, cov_norm = onp.gaussian_kernel1d(1.5, 3.5), 1.0
    f = lambda a: onp._filter_sep(a, k, "reflect")
    ux, uy = f(x), f(y)
    uxx, uyy, uxy = f(x * x), f(y * y), f(x * y)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))


def valid_mask(h, w, mode):
    p = PAD[mode]
    m = np.zeros((h, w), dtype=bool)
    if h > 2 * p and w > 2 * p:
        m[p:h - p, p:w - p] = True
    return m


def sq_err(a, b):
    """Per-pixel squared error, summed over the channels (exact integers)."""
    d = a.astype(np.int64) - b.astype(np.int64)
    d = d * d
    return d.sum(axis=2) if d.ndim == 3 else d


def uniform_edges(n, cell):
    return list(range(0, n, cell)) + [n]


def bin_map(m, x_edges, y_edges):
    """Sum of the 2-D map over every cell -> (gh, gw), in the map's dtype class (int64 or float64)."""
    out = np.zeros((len(y_edges) - 1, len(x_edges) - 1), dtype=np.int64 if m.dtype.kind in "iub" else np.float64)
    for gy in range(out.shape[0]):
        for gx in range(out.shape[1]):
            out[gy, gx] = m[y_edges[gy]:y_edges[gy + 1], x_edges[gx]:x_edges[gx + 1]].sum()
    return out


class Reference:
    """Everything one image pair needs, computed once: the squared-error map and the three masked SSIM maps."""

    def __init__(self, a, b, shift=15, data_range=255.0):
        self.h, self.w = a.shape[:2]
        self.sq = sq_err(a, b)
        g1, g2 = gray(a, shift), gray(b, shift)
        self.maps = {}
        for mode in PAD:
            if min(self.h, self.w) > 2 * PAD[mode]:
                self.maps[mode] = np.where(valid_mask(self.h, self.w, mode), ssim_map(g1, g2, mode, data_range), 0.0)
            else:
                self.maps[mode] = np.zeros((self.h, self.w))

    def cells(self, x_edges, y_edges):
        out = {"sse": bin_map(self.sq, x_edges, y_edges).astype(np.uint64)}
        for mode in PAD:
            out[f"ssim_{mode}"] = bin_map(self.maps[mode], x_edges, y_edges)
            out[f"count_{mode}"] = bin_map(valid_mask(self.h, self.w, mode), x_edges, y_edges)
        return out
