"""NumPy float64 restatement of the SR-benchmark PSNR / SSIM defined in include/sr_hip.h (sr_bench_u8), the kernel's block
geometry as the tests need it, and the inputs the tests use.

Crop both images by crop_border on every side.  Planes: the channels as they are ('channels'), the BT.601 luma
Y = X / 255000 with X = 65481 R + 128553 G + 24966 B + 4080000 in float64 ('y'), or the u8 plane floor((2 X + 255000) /
510000) ('y_round').  sse: Python integers (in 'y': the integer sum of (X - X')^2 over 255000^2).  SSIM: explicit 11 taps
(sigma 1.5), valid convolution (axis 0, then axis 1, in scipy.ndimage's order), population covariance, the mean over the
maps of all planes."""
import math

import numpy as np

import _msssim_ref as M

CHANNELS, Y, Y_ROUND = 0, 1, 2          # enum sr_bench_mode
YSCALE = 255000
WIN = 11
# csrc/sr_srbench.hip: a block produces OUT map columns from TX input columns; a small image is cut into chunks of ROWS_MIN map
# rows (more only from 1024 blocks up)
TX, OUT, ROWS_MIN = 256, 246, 16


def x_int(img):
    """The exact integer X = 255000 Y of an RGB u8 image (int64)."""
    i = img.astype(np.int64)
    return 65481 * i[..., 0] + 128553 * i[..., 1] + 24966 * i[..., 2] + 16 * YSCALE


def y_round(img):
    """MATLAB's uint8 rgb2ycbcr luma: X / 255000 rounded half up."""
    return ((2 * x_int(img) + YSCALE) // (2 * YSCALE)).astype(np.uint8)


def gray_as_y_round(v):
    """y_round of the RGB image with R = G = B = v, in closed form: X = 219000 v + 4080000."""
    return ((2 * (219000 * v.astype(np.int64) + 4080000) + 255000) // 510000).astype(np.uint8)


def crop(img, cb):
    return img[cb:img.shape[0] - cb, cb:img.shape[1] - cb]


def plan(h, w, cn, cb, mode):
    """-> (ch, cw, n_elems, n_map); ValueError like sr_bench_plan."""
    if cn not in (1, 3) or mode not in (CHANNELS, Y, Y_ROUND) or (mode != CHANNELS and cn != 3) or cb < 0 or h < 1 or w < 1:
        raise ValueError("invalid argument")
    ch, cw = h - 2 * cb, w - 2 * cb
    if min(ch, cw) < WIN:
        raise ValueError(f"both sides must be at least {WIN} after the crop")
    planes = cn if mode == CHANNELS else 1
    return ch, cw, ch * cw * planes, (ch - 10) * (cw - 10) * planes


def blocks(ch, cw, planes=1):
    """(row chunks, column blocks) the kernel cuts a small cropped image into."""
    mh, mw = ch - 10, cw - 10
    gy = -(-mw // OUT)
    assert -(-mh // ROWS_MIN) * gy * planes < 1024, "the tests' images take the shortest chunks"
    n = -(-mh // ROWS_MIN)
    step = -(-mh // n)
    return -(-mh // step), gy


def ssim_map_sum(x, y, data_range=255.0):
    """Sum of the SSIM map of two float64 planes."""
    k = M.taps()
    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    ux, uy = M._valid(x, k), M._valid(y, k)
    uxx, uyy, uxy = M._valid(x * x, k), M._valid(y * y, k), M._valid(x * y, k)
    vx, vy, vxy = uxx - ux * ux, uyy - uy * uy, uxy - ux * uy
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    return float(s.sum())


def planes_of(img, mode):
    """-> list of (float64 plane, exact integer plane, integer scale): plane = integer / scale."""
    if mode == Y:
        x = x_int(img)
        return [(x / float(YSCALE), x, YSCALE)]
    if mode == Y_ROUND:
        p = y_round(img).astype(np.int64)
        return [(p.astype(np.float64), p, 1)]
    chans = [img] if img.ndim == 2 else [img[..., c] for c in range(img.shape[2])]
    return [(c.astype(np.float64), c.astype(np.int64), 1) for c in chans]


def bench(a, b, cb=0, mode=Y, data_range=255.0):
    """-> {'sse' (int, or a float in mode Y), 'sse_int' (the integer numerator), 'ssim_sum', 'n_elems', 'n_map', 'psnr',
    'ssim'} of two u8 images of equal shape."""
    assert a.shape == b.shape and a.dtype == b.dtype == np.uint8
    cn = a.shape[2] if a.ndim == 3 else 1
    ch, cw, n_elems, n_map = plan(a.shape[0], a.shape[1], cn, cb, mode)
    pa, pb = planes_of(crop(a, cb), mode), planes_of(crop(b, cb), mode)
    sse_int, ssim_sum = 0, 0.0
    for (fa, ia, scale), (fb, ib, _) in zip(pa, pb):
        d = (ia - ib).astype(object)
        sse_int += int((d * d).sum())
        ssim_sum += ssim_map_sum(fa, fb, data_range)
    sse = sse_int / float(YSCALE) ** 2 if mode == Y else sse_int
    psnr = math.inf if sse_int == 0 else 10.0 * math.log10(data_range * data_range / (sse / n_elems))
    return {"sse": sse, "sse_int": sse_int, "ssim_sum": ssim_sum, "n_elems": n_elems, "n_map": n_map, "psnr": psnr,
            "ssim": ssim_sum / n_map}


def img_pair(rng, h, w, cn=3):
    """A textured image and a visibly distorted partner (block offsets, gain, noise): SSIM stays clear of 1, the channels
    differ from each other, and the squared differences are large enough that a pixel counted twice or not at all shows."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([128 + 60 * np.sin(xx / 11.0 + c) + 40 * np.cos(yy / 7.0 + 2 * c) for c in range(cn)], -1)
    a = np.clip(0.5 * rng.integers(0, 256, (h, w, cn)) + 0.5 * base, 0, 255).astype(np.uint8)
    d = (M._blocks(rng, h, w, 16, 40.0) + M._blocks(rng, h, w, 4, 30.0))[..., None]
    b = np.clip(0.8 * a + d + 6.0 * rng.standard_normal(a.shape) + 20.0, 0, 255).astype(np.uint8)
    return (a, b) if cn == 3 else (a[..., 0], b[..., 0])
