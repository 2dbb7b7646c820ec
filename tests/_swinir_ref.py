"""Torch-CPU restatement of the SwinIR backend's contract (include/sr_hip.h, "SwinIR") -- the yardstick of
tests/test_gpu_swinir.py and tests/test_swinir_host.py -- plus seeded synthetic weights under BasicSR's key names.

PARITY UNPINNED: neither the BasicSR package, the official SwinIR repository nor a checkpoint exists offline; this file restates
the published forward (resi_connection '1conv', ape False, patch_norm True, qkv_bias True, patch_size 1, window 8) with torch's
own operators (layer_norm, softmax, gelu, conv2d, linear) in float32 (what a torch user would run) and float64 (the truth the
bounds are taken against), and a second time in plain numpy in the documented order (chain_forward: fp32 chains for the
convolutions and the linear layers, np_layernorm, np_attention).  It reads the state dict on its own (it does not use the
product's parser).  img_range and rgb_mean ride in the state as extra entries, the way sr_network.load_network reads them from
a .npz; their fp32 values are the contract's parameters.  Also here: the mutants that show what the cases can see and the plan
rule restated."""
from __future__ import annotations

import functools
import math

import numpy as np

from _resnet_ref import RGB_MEAN
from _srnet_ref import _chain_conv, check_u8, make_image, quantize  # noqa: F401  (re-exported for the tests)

WIN, SHIFT, TOK, MID = 8, 4, 64, 64
IMG_RANGE = 2.0                     # not SwinIR's 1: a loader that drops the .npz entry must show
UPSAMPLERS = ("pixelshuffle", "pixelshuffledirect", "nearest+conv")
MUTANTS = ("no-shift", "no-mask", "bias-T", "no-qscale", "sample-var", "tanh-gelu", "zero-pad")

# (C, heads, hidden, L, D, scale, upsampler, h, w): the smallest that still reach every path -- a corner, an edge and an interior
# window (13 x 21 -> 16 x 24); one window whose shift wraps onto itself; C = 180 with x3; an odd depth on more than one 8 x 32
# block with nearest+conv; x1
CASES = [(60, 6, 120, 2, 2, 2, "pixelshuffledirect", 13, 21), (64, 2, 128, 1, 2, 4, "pixelshuffle", 8, 8),
         (180, 6, 360, 1, 2, 3, "pixelshuffle", 16, 24), (64, 4, 256, 2, 3, 4, "nearest+conv", 40, 70),
         (60, 6, 120, 1, 2, 1, "pixelshuffledirect", 9, 33)]
# the pad is larger than the side
EDGE_CASES = [(60, 6, 120, 1, 2, 2, "pixelshuffledirect", h, w) for h, w in [(1, 1), (1, 50), (50, 1)]]


def case_id(c) -> str:
    return f"C{c[0]}-h{c[1]}-m{c[2]}-L{c[3]}-D{c[4]}-x{c[5]}-{c[6]}-{c[7]}x{c[8]}"


def _stages(scale: int):
    return {1: [], 2: [2], 3: [3], 4: [2, 2]}[scale]


def table_names(L: int, D: int, scale: int, upsampler: str):
    """BasicSR's names of every table in sr_swinir_create's order."""
    names = ["conv_first", "patch_embed.norm"]
    for i in range(L):
        for j in range(D):
            b = f"layers.{i}.residual_group.blocks.{j}"
            names += [f"{b}.norm1", f"{b}.attn.qkv", f"{b}.attn.relative_position_bias_table", f"{b}.attn.proj", f"{b}.norm2", f"{b}.mlp.fc1",
                      f"{b}.mlp.fc2"]
        names.append(f"layers.{i}.conv")
    names += ["norm", "conv_after_body"]
    if upsampler == "pixelshuffle":
        return names + ["conv_before_upsample.0"] + [f"upsample.{2 * k}" for k in range(len(_stages(scale)))] + ["conv_last"]
    if upsampler == "pixelshuffledirect":
        return names + ["upsample.0"]
    return names + ["conv_before_upsample.0", "conv_up1", "conv_up2", "conv_hr", "conv_last"]


def table_shapes(C: int, heads: int, hidden: int, L: int, D: int, scale: int, upsampler: str):
    """(weight shape, bias shape or None) of every table, in the same order."""
    ln = ((C,), (C,))
    layer = [ln, ((3 * C, C), (3 * C,)), (((2 * WIN - 1) ** 2, heads), None), ((C, C), (C,)), ln, ((hidden, C), (hidden,)), ((C, hidden), (C,))]

    def conv(co, ci):
        return ((co, ci, 3, 3), (co,))

    shapes = [conv(C, 3), ln] + (layer * D + [conv(C, C)]) * L + [ln, conv(C, C)]
    if upsampler == "pixelshuffle":
        return shapes + [conv(MID, C)] + [conv(MID * r * r, MID) for r in _stages(scale)] + [conv(3, MID)]
    if upsampler == "pixelshuffledirect":
        return shapes + [conv(3 * scale * scale, C)]
    return shapes + [conv(MID, C)] + [conv(MID, MID)] * 3 + [conv(3, MID)]


def rel_index() -> np.ndarray:
    """(64, 64): the bias-table row of (query token i, key token j), as BasicSR builds relative_position_index."""
    coords = np.stack(np.meshgrid(np.arange(WIN), np.arange(WIN), indexing="ij")).reshape(2, -1)
    rel = (coords[:, :, None] - coords[:, None, :]).transpose(1, 2, 0) + (WIN - 1)
    return rel[:, :, 0] * (2 * WIN - 1) + rel[:, :, 1]


def region_map(hp: int, wp: int) -> np.ndarray:
    """calculate_mask's img_mask: the region number of every pixel of the rolled image."""
    m = np.zeros((hp, wp), np.int64)
    cnt = 0
    for hs in (slice(0, -WIN), slice(-WIN, -SHIFT), slice(-SHIFT, None)):
        for ws in (slice(0, -WIN), slice(-WIN, -SHIFT), slice(-SHIFT, None)):
            m[hs, ws] = cnt
            cnt += 1
    return m


def _windows(a: np.ndarray) -> np.ndarray:
    """(..., hp, wp) -> (..., windows, 64), windows row-major, tokens row-major."""
    hp, wp = a.shape[-2:]
    lead = a.shape[:-2]
    a = a.reshape(lead + (hp // WIN, WIN, wp // WIN, WIN))
    n = len(lead)
    return a.transpose(tuple(range(n)) + (n, n + 2, n + 1, n + 3)).reshape(lead + (-1, TOK))


def _unwindows(a: np.ndarray, hp: int, wp: int) -> np.ndarray:
    lead = a.shape[:-2]
    n = len(lead)
    a = a.reshape(lead + (hp // WIN, wp // WIN, WIN, WIN))
    return a.transpose(tuple(range(n)) + (n, n + 2, n + 1, n + 3)).reshape(lead + (hp, wp))


def attn_mask(hp: int, wp: int) -> np.ndarray:
    """(windows, 64, 64): -100 where two tokens of a window lie in different regions, else 0."""
    mw = _windows(region_map(hp, wp))
    return np.where(mw[:, None, :] != mw[:, :, None], -100.0, 0.0)


def synthetic_state(C: int, heads: int, hidden: int, L: int, D: int, scale: int, upsampler: str, seed: int = 20261019) -> dict:
    """Seeded weights under BasicSR's key names.  3 x 3 convolutions N(0, sqrt(2 / (9 cin))) / 2, conv_last (and the direct
    upsample.0) x 0.1, linear layers N(0, 1 / sqrt(cin)) / 2 (fc1: x 2, so that the GELU sees arguments of several units), biases N(0, 0.02); LayerNorm gamma in [0.5, 1.5], beta N(0, 0.1);
    bias tables N(0, 0.5) -- all non-trivial, so a dropped one shows.  Also the two buffers a loader must ignore, filled with
    what would break the forward if used (a zero relative_position_index, an attn_mask of 7s), and img_range / rgb_mean."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, (ws, bs) in zip(table_names(L, D, scale, upsampler), table_shapes(C, heads, hidden, L, D, scale, upsampler)):
        if name.endswith("relative_position_bias_table"):
            st[name] = (rng.standard_normal(ws) * 0.5).astype(np.float32)
            base = name[:-len("relative_position_bias_table")]
            st[base + "relative_position_index"] = np.zeros((TOK, TOK), np.int64)
            if int(name.split(".")[4]) % 2:
                st[base[:-len("attn.")] + "attn_mask"] = np.full((1, TOK, TOK), 7.0, np.float32)
        elif len(ws) == 1:
            st[f"{name}.weight"] = rng.uniform(0.5, 1.5, ws).astype(np.float32)
            st[f"{name}.bias"] = (rng.standard_normal(bs) * 0.1).astype(np.float32)
        elif len(ws) == 2:
            gain = 2.0 if name.endswith("mlp.fc1") else 0.5
            st[f"{name}.weight"] = (rng.standard_normal(ws) * gain / np.sqrt(ws[1])).astype(np.float32)
            st[f"{name}.bias"] = (rng.standard_normal(bs) * 0.02).astype(np.float32)
        else:
            gain = 0.1 if name == "conv_last" or (name == "upsample.0" and upsampler == "pixelshuffledirect") else 0.5
            st[f"{name}.weight"] = (rng.standard_normal(ws) * np.sqrt(2.0 / (9 * ws[1])) * gain).astype(np.float32)
            st[f"{name}.bias"] = (rng.standard_normal(bs) * 0.02).astype(np.float32)
    st["img_range"] = np.array(IMG_RANGE, np.float32)
    st["rgb_mean"] = np.array(RGB_MEAN, np.float32)
    return st


def _dims(state: dict):
    """-> (C, heads, hidden, L, D, scale, upsampler) read off the keys."""
    C = np.asarray(state["conv_first.weight"]).shape[0]
    L = len({k.split(".")[1] for k in state if k.startswith("layers.")})
    D = len({k.split(".")[4] for k in state if k.startswith("layers.0.residual_group.blocks.")})
    heads = np.asarray(state["layers.0.residual_group.blocks.0.attn.relative_position_bias_table"]).shape[1]
    hidden = np.asarray(state["layers.0.residual_group.blocks.0.mlp.fc1.weight"]).shape[0]
    if "conv_up1.weight" in state:
        return C, heads, hidden, L, D, 4, "nearest+conv"
    if "conv_before_upsample.0.weight" in state:
        ups = [k for k in state if k.startswith("upsample.") and k.endswith(".weight")]
        return C, heads, hidden, L, D, int(np.prod([int(round((np.asarray(state[k]).shape[0] / MID) ** 0.5)) for k in ups])), "pixelshuffle"
    return C, heads, hidden, L, D, int(round((np.asarray(state["upsample.0.weight"]).shape[0] / 3) ** 0.5)), "pixelshuffledirect"


def _consts(state: dict):
    return np.float32(state.get("img_range", 1.0)), np.asarray(state.get("rgb_mean", RGB_MEAN), np.float32)


def arrays(state: dict):
    """(weights, biases) in sr_swinir_create's order; a bias table's bias is None."""
    C, heads, hidden, L, D, s, up = _dims(state)
    ws, bs = [], []
    for n in table_names(L, D, s, up):
        if n.endswith("relative_position_bias_table"):
            ws.append(np.asarray(state[n]))
            bs.append(None)
        else:
            ws.append(np.asarray(state[f"{n}.weight"]))
            bs.append(np.asarray(state[f"{n}.bias"]))
    return ws, bs


def pad_image(img: np.ndarray, mode: str = "symmetric") -> np.ndarray:
    h, w = img.shape[:2]
    pads = ((0, -h % WIN), (0, -w % WIN), (0, 0))
    return np.pad(img, pads, mode="symmetric") if mode == "symmetric" else np.pad(img, pads, mode="constant")


def forward(state: dict, img: np.ndarray, dtype: str = "float64", mutant: str = "") -> np.ndarray:
    """-> (h s, w s, 3) array of `dtype`, unclamped.  mutant: what a wrong kernel would compute (MUTANTS), for the CPU check that
    the cases can see it."""
    import torch
    import torch.nn.functional as Fn
    assert mutant in ("",) + MUTANTS
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    C, heads, hidden, L, D, scale, up = _dims(state)
    d = C // heads
    rng_, mean = _consts(state)
    rg = float(rng_)
    hh, ww = img.shape[:2]
    padded = pad_image(img, "constant" if mutant == "zero-pad" else "symmetric")
    hp, wp = padded.shape[:2]
    rel = torch.from_numpy(rel_index().reshape(-1))
    mask = torch.from_numpy(attn_mask(hp, wp)).to(dt)

    def tensor(key):
        return torch.from_numpy(np.array(state[key])).to(dt)

    def conv(name, y):
        return Fn.conv2d(y, tensor(f"{name}.weight"), tensor(f"{name}.bias"), stride=1, padding=1)

    def lin(name, y):
        return Fn.linear(y, tensor(f"{name}.weight"), tensor(f"{name}.bias"))

    def norm(name, y):                                                  # y: (..., C)
        if mutant == "sample-var":
            mu = y.mean(-1, keepdim=True)
            return (y - mu) / torch.sqrt(y.var(-1, unbiased=True, keepdim=True) + 1e-5) * tensor(f"{name}.weight") + tensor(f"{name}.bias")
        return Fn.layer_norm(y, (C,), tensor(f"{name}.weight"), tensor(f"{name}.bias"), 1e-5)

    def tokens(y):                                                      # (1, C, hp, wp) -> (1, hp, wp, C)
        return y.permute(0, 2, 3, 1)

    def image(t):
        return t.permute(0, 3, 1, 2)

    def swin(name, x, shift):                                           # x: (1, hp, wp, C)
        y = norm(f"{name}.norm1", x)
        if shift:
            y = torch.roll(y, (-shift, -shift), (1, 2))
        win = y.view(1, hp // WIN, WIN, wp // WIN, WIN, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, TOK, C)
        qkv = lin(f"{name}.attn.qkv", win).reshape(-1, TOK, 3, heads, d).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        if mutant != "no-qscale":
            q = q * (d ** -0.5)
        a = q @ k.transpose(-2, -1)
        bias = tensor(f"{name}.attn.relative_position_bias_table")[rel].view(TOK, TOK, heads).permute(2, 0, 1)
        a = a + (bias.transpose(1, 2) if mutant == "bias-T" else bias)[None]
        if shift and mutant != "no-mask":
            a = a + mask[:, None]
        a = Fn.softmax(a, -1)
        o = lin(f"{name}.attn.proj", (a @ v).transpose(1, 2).reshape(-1, TOK, C))
        o = o.view(1, hp // WIN, wp // WIN, WIN, WIN, C).permute(0, 1, 3, 2, 4, 5).reshape(1, hp, wp, C)
        if shift:
            o = torch.roll(o, (shift, shift), (1, 2))
        x = x + o
        z = lin(f"{name}.mlp.fc1", norm(f"{name}.norm2", x))
        z = Fn.gelu(z, approximate="tanh") if mutant == "tanh-gelu" else Fn.gelu(z)
        return x + lin(f"{name}.mlp.fc2", z)

    p = torch.from_numpy(np.array(padded)).permute(2, 0, 1)[None]
    p = (p.to(torch.float32) / 255.0).to(dt)                          # the contract's fp32 division, exact in float64 afterwards
    meant = torch.from_numpy(np.array(mean)).to(dt).view(1, 3, 1, 1)
    lrelu = Fn.leaky_relu
    with torch.no_grad():
        h0 = conv("conv_first", (p - meant) * rg)
        t = norm("patch_embed.norm", tokens(h0))
        for i in range(L):
            r = t
            for j in range(D):
                t = swin(f"layers.{i}.residual_group.blocks.{j}", t, 0 if j % 2 == 0 or mutant == "no-shift" else SHIFT)
            t = tokens(conv(f"layers.{i}.conv", image(t))) + r
        f = conv("conv_after_body", image(norm("norm", t))) + h0
        if up == "pixelshuffle":
            y = lrelu(conv("conv_before_upsample.0", f), 0.01)
            for k, r in enumerate(_stages(scale)):
                y = Fn.pixel_shuffle(conv(f"upsample.{2 * k}", y), r)
            y = conv("conv_last", y)
        elif up == "pixelshuffledirect":
            y = Fn.pixel_shuffle(conv("upsample.0", f), scale)
        else:
            y = lrelu(conv("conv_before_upsample.0", f), 0.01)
            y = lrelu(conv("conv_up1", Fn.interpolate(y, scale_factor=2, mode="nearest")), 0.2)
            y = lrelu(conv("conv_up2", Fn.interpolate(y, scale_factor=2, mode="nearest")), 0.2)
            y = conv("conv_last", lrelu(conv("conv_hr", y), 0.2))
        o = (y / rg + meant)[:, :, :hh * scale, :ww * scale]
    return np.ascontiguousarray(o[0].permute(1, 2, 0).numpy())


# ---------------------------------------------------------------------------------------------------------------------------
# The documented order in plain numpy.
# ---------------------------------------------------------------------------------------------------------------------------
def np_layernorm(x: np.ndarray, gamma, beta, divisor_offset: int = 0) -> np.ndarray:
    """The header's LayerNorm on planes x (C, h, w) fp32 -> fp32: float64, channels ascending, two passes, the square rounded and
    then added, y = (float)((x - mean) * (1 / sqrt(var + 1e-5)) * gamma + beta).  divisor_offset -1: the sample-variance mutant."""
    C = x.shape[0]
    x8 = x.astype(np.float64)
    s = np.zeros(x.shape[1:], np.float64)
    for c in range(C):
        s = s + x8[c]
    mean = s / float(C)
    v = np.zeros_like(s)
    for c in range(C):
        dd = x8[c] - mean
        v = v + dd * dd
    rstd = 1.0 / np.sqrt(v / float(C + divisor_offset) + 1e-5)
    g8, b8 = np.asarray(gamma, np.float32).astype(np.float64), np.asarray(beta, np.float32).astype(np.float64)
    return ((x8 - mean) * rstd * g8[:, None, None] + b8[:, None, None]).astype(np.float32)


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in float64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def np_attention(qkv: np.ndarray, table: np.ndarray, heads: int, shift: int, dtype=np.float32) -> np.ndarray:
    """The header's window attention on planes qkv (3 C, hp, wp) whose q planes are already scaled -> (C, hp, wp), before proj.
    dtype float32: the documented order (fmaf chain over dd, + bias, + mask, exact maximum, exp, the sum over keys ascending,
    the division, then the fmaf chain over keys).  dtype float64: the same formula in float64, the truth of the random probe."""
    f = dtype
    C3, hp, wp = qkv.shape
    C = C3 // 3
    d = C // heads
    x = np.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    win = _windows(x.astype(f)).reshape(3, heads, d, -1, TOK)           # (3, head, dd, window, token)
    q, k, v = (win[i].transpose(2, 0, 3, 1) for i in range(3))          # (window, head, token, dd)
    a = np.zeros(q.shape[:3] + (TOK,), f)
    for dd in range(d):
        qq, kk = q[..., :, None, dd], k[..., None, :, dd]
        a = _fma32(qq, kk, a) if f == np.float32 else a + qq * kk
    bias = np.asarray(table, np.float32)[rel_index().reshape(-1)].reshape(TOK, TOK, heads).transpose(2, 0, 1).astype(f)
    a = a + bias[None]
    if shift:
        a = a + attn_mask(hp, wp).astype(f)[:, None]
    e = np.exp(a - a.max(-1, keepdims=True))
    assert e.dtype == f
    s = np.zeros(e.shape[:-1], f)
    for j in range(TOK):
        s = s + e[..., j]
    p = e / s[..., None]
    o = np.zeros(q.shape, f)
    for j in range(TOK):
        pj, vj = p[..., :, j, None], v[..., j, None, :]
        o = _fma32(pj, np.broadcast_to(vj, o.shape), o) if f == np.float32 else o + pj * vj
    o = o.transpose(1, 3, 0, 2).reshape(C, -1, TOK)                     # (head, dd, window, token) -> (C, window, token)
    o = _unwindows(o, hp, wp)
    return np.roll(o, (shift, shift), (1, 2)) if shift else o


def _chain_linear(x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """A linear layer over planes (cin, h, w) -> (cout, h, w) in the mainloop's order: bias, then channels ascending (pairs, even
    then odd), each term one rounded fp32 multiply and one rounded fp32 add."""
    w = np.asarray(w, np.float32)
    acc = np.broadcast_to(np.asarray(b, np.float32)[:, None, None], (w.shape[0],) + x.shape[1:]).copy()
    for c in range(w.shape[1]):
        acc = acc + w[:, c, None, None] * x[c][None]
    return acc


_erf = np.vectorize(math.erf, otypes=[np.float64])


def _gelu32(x: np.ndarray) -> np.ndarray:
    f = np.float32
    return f(0.5) * x * (f(1.0) + _erf((x * f(0.70710678118654752440)).astype(np.float64)).astype(f))


def _leaky(y, slope):
    return np.where(y >= 0, y, np.float32(slope) * y)


def _shuffle(y: np.ndarray, r: int) -> np.ndarray:
    c, h, w = y.shape
    return y.reshape(c // (r * r), r, r, h, w).transpose(0, 3, 1, 4, 2).reshape(c // (r * r), h * r, w * r)


def chain_forward(state: dict, img: np.ndarray) -> np.ndarray:
    """The header's six steps in plain numpy in the documented order.  No torch.  -> float32 (h s, w s, 3), unclamped."""
    f = np.float32
    C, heads, hidden, L, D, scale, up = _dims(state)
    d = C // heads
    rng_, mean = _consts(state)
    hh, ww = img.shape[:2]

    def conv(name, y, fused=False):
        return _chain_conv(y, np.asarray(state[f"{name}.weight"]), np.asarray(state[f"{name}.bias"]), fused=fused)

    def lin(name, y):
        return _chain_linear(y, state[f"{name}.weight"], state[f"{name}.bias"])

    def norm(name, y):
        return np_layernorm(y, state[f"{name}.weight"], state[f"{name}.bias"])

    p = (pad_image(np.ascontiguousarray(img)).astype(f) / f(255.0)).transpose(2, 0, 1)
    x = ((p - mean[:, None, None]) * rng_).astype(f)
    h0 = conv("conv_first", x, fused=True)
    r = norm("patch_embed.norm", h0)
    for i in range(L):
        t = r
        for j in range(D):
            b = f"layers.{i}.residual_group.blocks.{j}"
            qkv = lin(f"{b}.attn.qkv", norm(f"{b}.norm1", t))
            qkv[:C] = qkv[:C] * (f(1.0) / np.sqrt(f(d)))
            o = np_attention(qkv, state[f"{b}.attn.relative_position_bias_table"], heads, SHIFT if j % 2 else 0)
            t = lin(f"{b}.attn.proj", o) + t
            t = lin(f"{b}.mlp.fc2", _gelu32(lin(f"{b}.mlp.fc1", norm(f"{b}.norm2", t)))) + t
            assert t.dtype == f
        r = conv(f"layers.{i}.conv", t) + r
    y = conv("conv_after_body", norm("norm", r)) + h0
    if up == "pixelshuffle":
        y = _leaky(conv("conv_before_upsample.0", y), 0.01)
        for k, rr in enumerate(_stages(scale)):
            y = _shuffle(conv(f"upsample.{2 * k}", y), rr)
        y = conv("conv_last", y)
    elif up == "pixelshuffledirect":
        y = _shuffle(conv("upsample.0", y), scale)
    else:
        y = _leaky(conv("conv_before_upsample.0", y), 0.01)
        y = _leaky(conv("conv_up1", y.repeat(2, 1).repeat(2, 2)), 0.2)
        y = _leaky(conv("conv_up2", y.repeat(2, 1).repeat(2, 2)), 0.2)
        y = conv("conv_last", _leaky(conv("conv_hr", y), 0.2))
    o = (y / rng_ + mean[:, None, None])[:, :hh * scale, :ww * scale]
    assert o.dtype == f
    return np.ascontiguousarray(o.transpose(1, 2, 0))


@functools.lru_cache(maxsize=None)
def case(C: int, heads: int, hidden: int, L: int, D: int, s: int, up: str, h: int, w: int):
    """One shared reference per case, computed once: (state, image, float64 forward, e32 = max|float32 - float64|)."""
    state = synthetic_state(C, heads, hidden, L, D, s, up)
    img = make_image(h, w)
    f64 = forward(state, img, "float64")
    f32 = forward(state, img, "float32")
    e32 = float(np.max(np.abs(f32.astype(np.float64) - f64)))
    for a in (img, f64):
        a.setflags(write=False)
    return state, img, f64, e32


# ---------------------------------------------------------------------------------------------------------------------------
# The plan rule of include/sr_hip.h (sr_swinir_plan), restated.
# ---------------------------------------------------------------------------------------------------------------------------
TRUNK_CAP = 32 << 30
DEFAULT_TAIL = 256


def _pad(v: int, m: int) -> int:
    return -(-v // m) * m


def _tail_steps(scale: int, up: str):
    """(factor behind the convolution's store, resolution multiplier of the convolution) of the tail phase."""
    if up == "pixelshuffledirect":
        return [(scale, 1)]
    if up == "nearest+conv":
        return [(2, 1), (2, 2), (1, 4), (1, 4), (1, 4)]
    out, m = [(1, 1)], 1
    for r in _stages(scale):
        out.append((r, m))
        m *= r
    return out + [(1, scale)]


def tail_extents(steps, scale: int, lo: int, hi: int, length: int):
    out = [None] * len(steps)
    na, nb = lo * scale, hi * scale
    for i in range(len(steps) - 1, -1, -1):
        r, m = steps[i]
        na, nb = na // r, -(-nb // r)
        out[i] = (na, nb)
        na, nb = max(na - 1, 0), min(nb + 1, length * m)
    return out


def plan(C: int, hidden: int, scale: int, up: str, h: int, w: int, tail: int = 0):
    """-> (padded rows, padded columns, the tail's halo, tail sub-pieces, workspace bytes) as the header states them."""
    steps = _tail_steps(scale, up)
    g = 0
    for r, _ in reversed(steps):
        g = -(-g // r) + 1
    tail = tail or DEFAULT_TAIL
    hp, wp = _pad(h, WIN), _pad(w, WIN)
    side = []
    for length, plen in ((h, hp), (w, wp)):
        big = 0
        for lo in range(0, length, tail):
            e = tail_extents(steps, scale, lo, min(lo + tail, length), plen)
            big = max([big] + [(e[i][1] - e[i][0]) * steps[i][0] for i in range(len(steps) - 1)])
        side.append(big)
    p0, p4 = hp * wp, side[0] * _pad(side[1], 4)
    cp, qp = _pad(C, 64), max(_pad(3 * C, 64), _pad(hidden, 64))
    return hp, wp, g, -(-h // tail) * -(-w // tail), 4 * (4 * cp + qp) * p0 + 4 * 2 * MID * p4 + 3 * p0
