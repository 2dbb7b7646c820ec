"""Torch-CPU restatement of the compact SR network's contract (include/sr_hip.h, "local SR backend") -- the yardstick of
tests/test_gpu_srnet.py -- plus the seeded synthetic weights and the test image.

PARITY UNPINNED: the Real-ESRGAN package (SRVGGNetCompact) and its checkpoints do not exist offline; this file restates the
published architecture with torch's own operators:

    x = u8 / 255;  y = conv2d(x, pad 1) -> prelu -> (conv2d -> prelu) x D -> conv2d;  o = pixel_shuffle(y, s) + nearest(x, s)

in float32 (what a torch user would run) and float64 (the truth the bounds are taken against).  It reads the state dict on
its own (it does not use the product's parser)."""
from __future__ import annotations

import functools

import numpy as np


# (F, D, s, h, w) of the float / u8 accuracy check: every case clamps.  F = 192 and 256 run the third and fourth 64-cout tile,
# the scale-4 cases the two-half tail (48 couts padded to 64) behind a body layer, on real weights.
CASES = [(64, 2, 2, 45, 77), (64, 16, 2, 40, 70), (128, 3, 3, 33, 41), (64, 0, 4, 9, 11), (64, 1, 1, 20, 35),
         (192, 1, 2, 17, 40), (256, 2, 4, 12, 35), (128, 2, 4, 19, 37)]
# degenerate images and exact / one-past multiples of the convolution's 8 x 32 block (too small to clamp on both sides)
EDGE_CASES = [(64, 3, 3, 1, 1), (64, 2, 2, 1, 50), (64, 2, 2, 50, 1), (64, 1, 2, 8, 32), (64, 1, 2, 9, 33), (64, 1, 4, 8, 33)]


def synthetic_state(n_feat: int, n_body: int, scale: int, seed: int = 20260313) -> dict:
    """Seeded weights in SRVGGNetCompact's naming: body.{2k} convolutions, body.{2k + 1} PReLU slopes.
    Convolutions N(0, sqrt(2 / (9 cin))), the tail's x 0.1, biases N(0, 0.01), slopes U(0.05, 0.3)."""
    rng = np.random.default_rng(seed)
    st = {}
    chans = [3] + [n_feat] * (n_body + 1) + [3 * scale * scale]
    for k in range(n_body + 2):
        cin, cout = chans[k], chans[k + 1]
        w = rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))
        if k == n_body + 1:
            w = w * 0.1
        st[f"body.{2 * k}.weight"] = w.astype(np.float32)
        st[f"body.{2 * k}.bias"] = (rng.standard_normal(cout) * 0.01).astype(np.float32)
        if k <= n_body:
            st[f"body.{2 * k + 1}.weight"] = rng.uniform(0.05, 0.3, cout).astype(np.float32)
    return st


def make_image(h: int, w: int, seed: int = 7) -> np.ndarray:
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (128 + 64 * np.sin(xx / 7.0) + 48 * np.cos(yy / 5.0))[..., None]
    return np.clip(base + rng.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8)


def _layers(state: dict):
    idx = sorted({int(k.split(".")[1]) for k in state})
    convs = [i for i in idx if np.asarray(state[f"body.{i}.weight"]).ndim == 4]
    out = []
    for i in convs:
        slope = state.get(f"body.{i + 1}.weight")
        if slope is not None and np.asarray(slope).ndim != 1:
            slope = None
        out.append((state[f"body.{i}.weight"], state[f"body.{i}.bias"], slope))
    return out


def forward(state: dict, img: np.ndarray, dtype: str = "float64", default_slope: float = 0.0) -> np.ndarray:
    """-> (h s, w s, 3) array of `dtype`, unclamped."""
    import torch
    import torch.nn.functional as Fn
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    layers = _layers(state)
    x = torch.from_numpy(np.array(img)).permute(2, 0, 1)[None]       # a copy: cached images are read-only
    x = x.to(torch.float32) / 255.0                      # the contract's fp32 division, exact in float64 afterwards
    x = x.to(dt)
    y = x
    with torch.no_grad():
        for n, (w, b, slope) in enumerate(layers):
            w, b = torch.from_numpy(np.asarray(w)).to(dt), torch.from_numpy(np.asarray(b)).to(dt)
            y = Fn.conv2d(y, w, b, stride=1, padding=1)
            if n < len(layers) - 1:
                y = Fn.prelu(y, torch.from_numpy(_slopes(slope, w.shape[0], default_slope)).to(dt))
        tail_c = layers[-1][0].shape[0]
        s = int(round((tail_c / 3) ** 0.5))
        o = Fn.pixel_shuffle(y, s) + Fn.interpolate(x, scale_factor=s, mode="nearest")
    return np.ascontiguousarray(o[0].permute(1, 2, 0).numpy())


def _slopes(slope, n: int, default_slope: float) -> np.ndarray:
    return np.full(n, default_slope, np.float32) if slope is None else np.array(np.broadcast_to(np.asarray(slope, np.float32), (n,)))


def _chain_conv(x: np.ndarray, w: np.ndarray, b: np.ndarray, fused: bool) -> np.ndarray:
    """3 x 3, zero padding 1, fp32, one output = one sequential chain: (cin, h, w) -> (cout, h, w).
    fused (the head): bias, then channels ascending, then taps ascending, each term one fmaf -- the product of two fp32
    values is exact in float64, so the chain runs in float64 and is rounded to fp32 after every term.
    not fused (body and tail): bias, then channel pairs (2p, 2p + 1) ascending, then taps ascending, then the even and the
    odd channel of the pair; each term is one rounded fp32 multiply and one rounded fp32 add."""
    cout, cin = w.shape[:2]
    h, wd = x.shape[1:]
    xp = np.zeros((cin, h + 2, wd + 2), np.float32)
    xp[:, 1:-1, 1:-1] = x
    w = np.asarray(w, np.float32).reshape(cout, cin, 9)
    acc = np.broadcast_to(np.asarray(b, np.float32)[:, None, None], (cout, h, wd)).copy()
    if fused:
        order = [(c, t) for c in range(cin) for t in range(9)]
    else:
        assert cin % 2 == 0
        order = [(2 * p + k, t) for p in range(cin // 2) for t in range(9) for k in (0, 1)]
    for c, t in order:
        v = xp[c, t // 3:t // 3 + h, t % 3:t % 3 + wd][None]
        wc = w[:, c, t][:, None, None]
        if fused:
            acc = (wc.astype(np.float64) * v.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
        else:
            acc = acc + wc * v                            # fp32 product, fp32 sum: two roundings
    return acc


def chain_forward(state: dict, img: np.ndarray, default_slope: float = 0.0) -> np.ndarray:
    """The forward in plain numpy fp32, summed in the order csrc/sr_srnet.hip documents (see _chain_conv), with the slope
    activation, the pixel shuffle written out as o[Y, X, c] = t[c s^2 + (Y % s) s + (X % s), Y / s, X / s] and the nearest base
    as one fp32 add.  No torch: a second statement of the contract beside forward().  -> float32 (h s, w s, 3), unclamped."""
    layers = _layers(state)
    x = (np.ascontiguousarray(img).astype(np.float32) / np.float32(255.0)).transpose(2, 0, 1)
    y = x
    for n, (w, b, slope) in enumerate(layers):
        y = _chain_conv(y, np.asarray(w), np.asarray(b), fused=n == 0)
        assert y.dtype == np.float32
        if n < len(layers) - 1:
            a = _slopes(slope, y.shape[0], default_slope)[:, None, None]
            y = np.where(y >= 0, y, a * y)
    s = int(round((y.shape[0] / 3) ** 0.5))
    Y, X, c = np.meshgrid(np.arange(img.shape[0] * s), np.arange(img.shape[1] * s), np.arange(3), indexing="ij")
    o = y[c * s * s + (Y % s) * s + (X % s), Y // s, X // s] + x[c, Y // s, X // s]
    assert o.dtype == np.float32
    return np.ascontiguousarray(o)


def quantize(o: np.ndarray) -> np.ndarray:
    """The u8 entry point's rounding on a float64 truth: rint(clip(o, 0, 1) * 255), half to even."""
    return np.rint(np.clip(o, 0.0, 1.0) * 255.0).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def case(n_feat: int, n_body: int, scale: int, h: int, w: int):
    """One shared reference per case, computed once: (state, image, float64 forward, e32 = max|float32 - float64|)."""
    state = synthetic_state(n_feat, n_body, scale)
    img = make_image(h, w)
    f64 = forward(state, img, "float64")
    f32 = forward(state, img, "float32")
    e32 = float(np.max(np.abs(f32.astype(np.float64) - f64)))
    for a in (img, f64):
        a.setflags(write=False)
    return state, img, f64, e32


@functools.lru_cache(maxsize=None)
def chain_case(n_feat: int, n_body: int, scale: int, h: int, w: int):
    """The second yardstick of a case, computed once: (chain_forward's output, e_chain = max|chain - float64|)."""
    state, img, f64, _ = case(n_feat, n_body, scale, h, w)
    chain = chain_forward(state, img)
    chain.setflags(write=False)
    return chain, float(np.max(np.abs(chain.astype(np.float64) - f64)))


def check_u8(got: np.ndarray, f64: np.ndarray, e32: float, max_exempt: float = 0.01) -> float:
    """Check 2 of the issue: every byte equals rint(clip(f64) * 255) except where the float64 value lies within
    255 * 8 * e32 levels of a half-integer, where either neighbour is accepted; the exempt share must stay <= 1 %.
    -> the exempt share."""
    lv = np.clip(f64, 0.0, 1.0) * 255.0
    want = np.rint(lv).astype(np.int64)
    frac = lv - np.floor(lv)
    near = np.abs(frac - 0.5) <= 255.0 * 8.0 * e32
    g = got.astype(np.int64)
    assert got.shape == f64.shape
    strict_bad = (~near) & (g != want)
    assert not strict_bad.any(), f"{int(strict_bad.sum())} bytes differ away from a rounding boundary (first at {np.argwhere(strict_bad)[0]})"
    loose_bad = near & (g != np.floor(lv)) & (g != np.floor(lv) + 1)
    assert not loose_bad.any(), f"{int(loose_bad.sum())} bytes near a boundary are neither neighbour"
    share = float(near.mean())
    assert share <= max_exempt, f"exempt share {share:.4%} above {max_exempt:.0%}"
    return share
