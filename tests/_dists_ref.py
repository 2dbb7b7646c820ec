"""Restatement of DISTS as include/sr_hip.h defines it: the forward in torch-CPU at a chosen dtype (the L2 pooling is a grouped
conv2d there), the L2 pooling alone in NumPy fp32 with the header's operation order, and the sums and score in NumPy float64.
Shared by tests/test_dists_host.py and tests/test_gpu_dists.py."""
import numpy as np

CHANNELS = (3, 64, 128, 256, 512, 512)
TOTAL = sum(CHANNELS)
CONV_KEYS = ["stage1.0", "stage1.2", "stage2.5", "stage2.7", "stage3.10", "stage3.12", "stage3.14", "stage4.17", "stage4.19",
             "stage4.21", "stage5.24", "stage5.26", "stage5.28"]
STAGE_CONVS = (2, 2, 3, 3, 3)
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def layer_sizes(h, w):
    out = [(h, w), (h, w)]
    for _ in range(4):
        h, w = -(-h // 2), -(-w // 2)
        out.append((h, w))
    return out


def l2pool_np(x):
    """[C][H][W] fp32 -> [C][ceil(H/2)][ceil(W/2)] fp32 in the header's order: x * x rounded once, the nine terms added in
    row-major tap order onto 0, + 1e-12f, sqrt (IEEE, correctly rounded)."""
    x = np.asarray(x, dtype=np.float32)
    c, h, w = x.shape
    ho, wo = -(-h // 2), -(-w // 2)
    sq = np.zeros((c, 2 * ho + 1, 2 * wo + 1), np.float32)          # zero padding 1 in front, enough behind
    sq[:, 1:h + 1, 1:w + 1] = x * x
    g = (np.float32(0.25), np.float32(0.5), np.float32(0.25))
    s = np.zeros((c, ho, wo), np.float32)
    for j in range(3):
        for i in range(3):
            s = s + (g[j] * g[i]) * sq[:, j:j + 2 * ho:2, i:i + 2 * wo:2]
    return np.sqrt(s + np.float32(1e-12))


def to_rgb(img):
    """u8 HxW, HxWx1, HxWx3 or HxWx4 -> HxWx3 (gray repeated, alpha dropped)."""
    img = np.asarray(img)
    if img.ndim == 2:
        img = img[..., None]
    if img.shape[2] == 1:
        img = np.repeat(img, 3, axis=2)
    return img[:, :, :3]


def features(img, weights, dtype):
    """The five stage outputs (torch tensors [C][H][W] of `dtype`) of one u8 image."""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.ascontiguousarray(to_rgb(img))).permute(2, 0, 1).to(dtype) / 255
    mean = torch.tensor(np.asarray(weights.get("mean", MEAN), dtype=np.float32).reshape(3)).to(dtype).view(3, 1, 1)
    std = torch.tensor(np.asarray(weights.get("std", STD), dtype=np.float32).reshape(3)).to(dtype).view(3, 1, 1)
    x = ((x - mean) / std)[None]
    hann = torch.tensor([0.25, 0.5, 0.25], dtype=dtype)
    filt = torch.outer(hann, hann)
    outs, ki = [], 0
    for si, n in enumerate(STAGE_CONVS):
        if si > 0:
            ch = x.shape[1]
            x = torch.sqrt(F.conv2d(x * x, filt[None, None].repeat(ch, 1, 1, 1), stride=2, padding=1, groups=ch) + 1e-12)
        for _ in range(n):
            key = CONV_KEYS[ki]
            ki += 1
            x = F.relu(F.conv2d(x, torch.from_numpy(np.asarray(weights[key + ".weight"], np.float32)).to(dtype),
                                torch.from_numpy(np.asarray(weights[key + ".bias"], np.float32)).to(dtype), padding=1))
        outs.append(x[0])
    return outs


def sums(a, b, weights, dtype):
    """1475 x 5 float64 sums (a, b, a^2, b^2, a b) of the restated forward at `dtype`; stage 0 from the u8 values."""
    import torch
    with torch.no_grad():
        fa, fb = features(a, weights, dtype), features(b, weights, dtype)
    rows = []
    ua, ub = to_rgb(a).astype(np.int64), to_rgb(b).astype(np.int64)
    for c in range(3):
        p, q = ua[:, :, c], ub[:, :, c]
        rows.append([p.sum(), q.sum(), (p * p).sum(), (q * q).sum(), (p * q).sum()])
    out = [np.asarray(rows, dtype=np.float64)]
    for p, q in zip(fa, fb):
        p = p.double().numpy().reshape(p.shape[0], -1)
        q = q.double().numpy().reshape(q.shape[0], -1)
        out.append(np.stack([p.sum(1), q.sum(1), (p * p).sum(1), (q * q).sum(1), (p * q).sum(1)], axis=1))
    return np.concatenate(out, axis=0)


def score(s, hw, alpha, beta):
    """(DISTS, S1[1475], S2[1475]) from the sums in float64."""
    s = np.asarray(s, dtype=np.float64)
    n = np.concatenate([np.full(c, float(h) * float(w)) for c, (h, w) in zip(CHANNELS, hw)])
    d1 = np.concatenate([np.full(3, 255.0), np.ones(TOTAL - 3)])
    d2 = d1 * d1
    ma, mb = s[:, 0] / d1 / n, s[:, 1] / d1 / n
    va, vb, cab = s[:, 2] / d2 / n - ma * ma, s[:, 3] / d2 / n - mb * mb, s[:, 4] / d2 / n - ma * mb
    s1 = (2 * ma * mb + 1e-6) / (ma * ma + mb * mb + 1e-6)
    s2 = (2 * cab + 1e-6) / (va + vb + 1e-6)
    al = np.asarray(alpha, dtype=np.float32).reshape(-1).astype(np.float64)
    be = np.asarray(beta, dtype=np.float32).reshape(-1).astype(np.float64)
    tot = al.sum() + be.sum()
    return float(1.0 - np.sum(al / tot * s1 + be / tot * s2)), s1, s2


def dists(a, b, weights, dtype):
    s = sums(a, b, weights, dtype)
    return score(s, layer_sizes(*np.asarray(a).shape[:2]), weights["alpha"], weights["beta"])


def pair(rng, h, w, cn=3, sigma=9.0):
    """The sinusoid + noise pair of tests/test_gpu_lpips.py (cn = 0: a 2-D gray array)."""
    yy, xx = np.mgrid[0:h, 0:w]
    base = (128 + 64 * np.sin(xx / 37.0) + 48 * np.cos(yy / 23.0))
    shape = (h, w) if cn == 0 else (h, w, cn)
    base = base if cn == 0 else base[..., None]
    a = np.clip(base + rng.integers(-20, 21, shape), 0, 255).astype(np.uint8)
    b = np.clip(a.astype(np.float32) + rng.normal(0, sigma, shape), 0, 255).astype(np.uint8)
    return a, b
