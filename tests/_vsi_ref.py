"""NumPy / SciPy float64 restatement of VSI with SDSP saliency, written from the definition in include/sr_hip.h in the
scripts' literal order (the authors' VSI.m and SDSP.m; parity with MATLAB is unpinned): numpy.fft for the transform, dense
per-axis matrices for imresize 'bilinear', the full-resolution saliency map really formed, mat2gray on it, then the F x F
mean, scipy's convolve2d for the Scharr gradient and the complex power for the chroma term.

`mut` names one deliberate mistake (the mutants of tests/test_vsi_host.py): 'sigma_c' (sigma_C = 0.25), 'no_mask' (the
frequency grid not zeroed beyond radius 0.5), 'centre' (SD centred at 128.5), 'no_mat2gray' (the resized map used as it is),
'abs_pow' (|S_c|^0.02 without the cosine), 'py_pool' (the pooling window centred as scipy's 'same' centres an even kernel),
'no_antialias' (no antialiasing: the triangle of support 2 even when the axis shrinks)."""
import numpy as np
from scipy.signal import convolve2d

N = 256
OMEGA0, SIGMA_F, SIGMA_D, SIGMA_C = 0.021, 1.34, 145.0, 0.001
C1, C2, C3, ALPHA, BETA = 1.27, 386.0, 130.0, 0.40, 0.02


def auto_f(h, w):
    return max(1, int(np.floor(min(h, w) / 256 + 0.5)))


def axis_taps(n_in, n_out, mut=None):
    """(w [n_out, P], idx [n_out, P]) of imresize's contribution rule with the triangle, before any trimming."""
    scale = n_out / n_in
    shrink = scale < 1 and mut != "no_antialias"
    kw = 2.0 / scale if shrink else 2.0
    P = int(np.ceil(kw)) + 2
    u = (np.arange(n_out) + 1) / scale + 0.5 * (1 - 1 / scale)
    left = np.floor(u - kw / 2)
    pos = left[:, None] + np.arange(P)[None, :]                 # 1-based, unreflected
    d = u[:, None] - pos
    tri = lambda x: np.maximum(0.0, 1.0 - np.abs(x))
    w = scale * tri(scale * d) if shrink else tri(d)
    w = w / w.sum(axis=1, keepdims=True)
    j = np.mod(pos.astype(np.int64) - 1, 2 * n_in)
    idx = np.where(j >= n_in, 2 * n_in - 1 - j, j)
    return w, idx


def axis_weights(n_in, n_out):
    """(w, idx) as sr_vsi_resize_weights returns them: all P = ceil(kw) + 2 taps, none trimmed."""
    w, idx = axis_taps(n_in, n_out)
    return w, idx.astype(np.int32)


def axis_matrix(n_in, n_out, mut=None):
    w, idx = axis_taps(n_in, n_out, mut)
    m = np.zeros((n_out, n_in))
    np.add.at(m, (np.repeat(np.arange(n_out), w.shape[1]), idx.ravel()), w.ravel())
    return m


def imresize(plane, oh, ow, mut=None):
    """imresize(plane, [oh ow], 'bilinear'): the axis with the smaller scale first, a tie vertical first."""
    h, w = plane.shape
    my, mx = axis_matrix(h, oh, mut), axis_matrix(w, ow, mut)
    if oh / h <= ow / w:
        return (my @ plane) @ mx.T
    return my @ (plane @ mx.T)


def rgb2lab(rgb):
    v = rgb / 255.0
    lin = np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    r, g, b = lin[0], lin[1], lin[2]
    x = (0.4124564 * r + 0.3575761 * g + 0.1804375 * b) / 0.950456
    y = 0.2126729 * r + 0.7151522 * g + 0.0721750 * b
    z = (0.0193339 * r + 0.1191920 * g + 0.9503041 * b) / 1.088754
    f = lambda t: np.where(t > 0.008856, np.cbrt(t), 7.787 * t + 16.0 / 116.0)
    fx, fy, fz = f(x), f(y), f(z)
    return np.stack([116.0 * fy - 16.0, 500.0 * (fx - fy), 200.0 * (fy - fz)])


def log_gabor(mut=None):
    u1, u2 = np.meshgrid((np.arange(N) - N // 2) / N, (np.arange(N) - N // 2) / N)
    if mut != "no_mask":
        mask = u1 ** 2 + u2 ** 2 > 0.25
        u1, u2 = np.where(mask, 0.0, u1), np.where(mask, 0.0, u2)
    u1, u2 = np.fft.ifftshift(u1), np.fft.ifftshift(u2)
    radius = np.sqrt(u1 ** 2 + u2 ** 2)
    radius[0, 0] = 1.0
    with np.errstate(divide="ignore"):
        lg = np.exp(-np.log(radius / OMEGA0) ** 2 / (2.0 * SIGMA_F ** 2))
    lg[0, 0] = 0.0
    return lg


def centre_prior(mut=None):
    c = 128.5 if mut == "centre" else 128.0
    r, col = np.meshgrid(np.arange(N) + 1.0, np.arange(N) + 1.0, indexing="ij")
    return np.exp(-((r - c) ** 2 + (col - c) ** 2) / SIGMA_D ** 2)


def sdsp(img, mut=None):
    """{'lab': [3, 256, 256], 'range': [min a, max a, min b, max b], 'vs256'} of one u8 RGB(A) image."""
    rgb = np.stack([imresize(img[..., k].astype(np.float64), N, N, mut) for k in range(3)])
    lab = rgb2lab(rgb)
    lg = log_gabor(mut)
    sf = np.sqrt(sum(np.real(np.fft.ifft2(np.fft.fft2(p) * lg)) ** 2 for p in lab))
    a, b = lab[1], lab[2]
    rng = np.array([a.min(), a.max(), b.min(), b.max()])
    with np.errstate(invalid="ignore", divide="ignore"):
        an, bn = (a - rng[0]) / (rng[1] - rng[0]), (b - rng[2]) / (rng[3] - rng[2])
        sigma_c = 0.25 if mut == "sigma_c" else SIGMA_C
        sc = 1.0 - np.exp(-(an ** 2 + bn ** 2) / sigma_c ** 2)
    return {"lab": lab, "range": rng, "vs256": sf * centre_prior(mut) * sc}


def saliency_full(img, mut=None):
    """(the h x w map after mat2gray, [min, max] before it, the sdsp record)."""
    s = sdsp(img, mut)
    vs = imresize(s["vs256"], img.shape[0], img.shape[1], mut)
    rng = np.array([vs.min(), vs.max()]) if not np.isnan(vs).any() else np.array([np.nan, np.nan])
    if mut != "no_mat2gray":
        with np.errstate(invalid="ignore", divide="ignore"):
            vs = (vs - rng[0]) / (rng[1] - rng[0])
    return vs, rng, s


def planes_int(img):
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    return np.stack([6 * r + 63 * g + 27 * b, 30 * r + 4 * g - 35 * b, 34 * r - 60 * g + 17 * b])


def pool_sum(plane, F, mut=None):
    """Window sums: window i of an axis covers i F + floor(F / 2) - F + 1 .. i F + floor(F / 2), zero outside."""
    h, w = plane.shape
    rows, cols = -(-h // F), -(-w // F)
    first = -(F // 2) if mut == "py_pool" else F // 2 - F + 1
    pad = np.zeros((h + 2 * F, w + 2 * F), plane.dtype)
    pad[F:F + h, F:F + w] = plane
    out = np.zeros((rows, cols), plane.dtype)
    for dy in range(F):
        for dx in range(F):
            ys, xs = F + first + dy, F + first + dx
            out = out + pad[ys:ys + rows * F:F, xs:xs + cols * F:F][:rows, :cols]
    return out


def pooled_int(img, F):
    return np.stack([pool_sum(p, F) for p in planes_int(img)])


def scharr(plane):
    dx = np.array([[3.0, 0.0, -3.0], [10.0, 0.0, -10.0], [3.0, 0.0, -3.0]]) / 16.0
    ix, iy = convolve2d(plane, dx, mode="same"), convolve2d(plane, dx.T, mode="same")
    return np.sqrt(ix ** 2 + iy ** 2)


def sim(u, v, k):
    return (2.0 * u * v + k) / (u ** 2 + v ** 2 + k)


def vsi(a, b, mut=None):
    """The record: 'sum_s', 'sum_w', 'value', 'F', 'size', 'a_range', 'b_range', 'vs_range' ([2, 2]), 'min_sc', 'neg' (the
    fraction of pooled samples with a negative S_c), 'sdsp' (both images' sdsp records)."""
    a, b = np.asarray(a), np.asarray(b)
    h, w = a.shape[:2]
    F = auto_f(h, w)
    side = []
    for img in (a, b):
        vs, rng, s = saliency_full(img, mut)
        lmn = np.stack([pool_sum(p, F, mut) for p in planes_int(img)]) / (100.0 * F * F)
        side.append({"vs": pool_sum(vs, F, mut) / (F * F), "lmn": lmn, "g": scharr(lmn[0]), "rng": rng, "s": s})
    p, q = side
    s_vs = sim(p["vs"], q["vs"], C1)
    s_g = sim(p["g"], q["g"], C2)
    s_c = sim(p["lmn"][1], q["lmn"][1], C3) * sim(p["lmn"][2], q["lmn"][2], C3)
    vsm = np.maximum(p["vs"], q["vs"])                          # keeps a NaN
    cw = np.abs(s_c) ** BETA if mut == "abs_pow" else np.real((s_c + 0j) ** BETA)
    sum_s, sum_w = float(np.sum(s_g ** ALPHA * s_vs * cw * vsm)), float(np.sum(vsm))
    with np.errstate(invalid="ignore", divide="ignore"):
        value = float(np.float64(sum_s) / np.float64(sum_w))
    return {"sum_s": sum_s, "sum_w": sum_w, "value": value, "F": F, "size": s_c.shape,
            "a_range": np.array([x["s"]["range"][:2] for x in side]), "b_range": np.array([x["s"]["range"][2:] for x in side]),
            "vs_range": np.array([x["rng"] for x in side]), "min_sc": float(s_c.min()), "neg": float((s_c < 0).mean()),
            "sdsp": [x["s"] for x in side]}


def case(h, w, cn=3, seed=0):
    """A coloured, textured u8 image and a distorted copy: blocks of random colour under noise, the copy with its own noise, a
    colour cast and a contrast change (a few pooled samples take the negative S_c branch)."""
    rnd = np.random.default_rng(1000 * h + w + 7 * seed)
    bh, bw = -(-h // 8), -(-w // 8)
    base = np.kron(rnd.integers(0, 256, (bh, bw, 3)), np.ones((8, 8, 1)))[:h, :w].astype(np.float64)
    a = np.clip(base + rnd.normal(0, 12, (h, w, 3)), 0, 255).round().astype(np.uint8)
    b = np.clip(0.8 * base + rnd.normal(0, 20, (h, w, 3)) + np.array([18.0, -6.0, 9.0]), 0, 255).round().astype(np.uint8)
    if cn == 4:
        alpha = rnd.integers(0, 256, (h, w, 1), dtype=np.uint8)
        a, b = np.concatenate([a, alpha], axis=2), np.concatenate([b, 255 - alpha], axis=2)
    return a, b


def complementary(h, w):
    """A pair whose chroma opposes over a large part: reddish against bluish, so sim(M1, M2) is negative there."""
    rnd = np.random.default_rng(h * 31 + w)
    y, x = np.mgrid[0:h, 0:w]
    a = np.stack([200 + 0 * x, 60 + (x * 40) // w, 40 + (y * 30) // h], axis=2) + rnd.integers(-20, 21, (h, w, 3))
    b = np.stack([40 + (y * 30) // h, 60 + (x * 40) // w, 210 + 0 * x], axis=2) + rnd.integers(-20, 21, (h, w, 3))
    half = w // 2
    b[:, :half] = a[:, :half] + rnd.integers(-9, 10, (h, half, 3))
    return np.clip(a, 0, 255).astype(np.uint8), np.clip(b, 0, 255).astype(np.uint8)
