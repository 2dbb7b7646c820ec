"""Restatement of the Swin2SR backend's contract (include/sr_hip.h, "Swin2SR") -- the yardstick of tests/test_gpu_swin2sr.py and
tests/test_swin2sr_host.py -- plus seeded synthetic weights under the `transformers` package's key names and the conversion of
such a state to the official repository's layout.

What pins it: tests/golden/swin2sr_*.npz hold random-weight models of `transformers` 5.15.0's Swin2SRForImageSuperResolution run
in float64 (tests/golden/make_swin2sr_golden.py); forward(..., "float64") must reproduce their outputs to 1e-9.  The
convolutions, the linear layers, the LayerNorm and gelu are torch's own operators; the cosine attention and the continuous
position bias are plain numpy.  It reads the state dict on its own (it does not use the product's parser).  In float64 the input
is u8 / 255 in float64 (what the package is given); in float32 it is the contract's fp32 division.  The official layout, the -100
mask and sides that are no multiple of 8 (where the package's own model fails) rest on this file alone."""
from __future__ import annotations

import functools
import math

import numpy as np

from _resnet_ref import RGB_MEAN
from _srnet_ref import check_u8, make_image, quantize  # noqa: F401  (re-exported for the tests)
from _swinir_ref import MID, SHIFT, TOK, WIN, _fma32, _stages, _unwindows, _windows, attn_mask, pad_image, plan, rel_index  # noqa: F401

CPB = 512
MASK_PACKAGE, MASK_OFFICIAL = -200.0, -100.0
UPSAMPLERS = ("pixelshuffle", "pixelshuffledirect", "nearest+conv")
MUTANTS = ("mask-100", "no-clamp", "pre-norm", "q-scale", "no-sigmoid", "no-proj", "k-bias", "skip-e")
P = "swin2sr."

# (C, heads, hidden, L, D, scale, upsampler, h, w): d in {8, 10, 30}, C in {24, 60}, the three upsamplers, one window whose shift
# wraps onto itself, a corner / edge / interior window with padding (13 x 21 -> 16 x 24), no padding (16 x 24), a long strip with
# padding on one axis only (9 x 40 -> 16 x 40)
CASES = [(24, 3, 48, 2, 2, 2, "pixelshuffledirect", 8, 8), (60, 6, 120, 1, 2, 2, "pixelshuffle", 13, 21),
         (60, 2, 96, 1, 3, 4, "nearest+conv", 16, 24), (24, 3, 48, 1, 2, 3, "pixelshuffle", 9, 40),
         (60, 6, 120, 2, 1, 4, "pixelshuffledirect", 13, 21)]


def case_id(c) -> str:
    return f"C{c[0]}-h{c[1]}-m{c[2]}-L{c[3]}-D{c[4]}-x{c[5]}-{c[6]}-{c[7]}x{c[8]}"


def tail_names(scale: int, upsampler: str):
    if upsampler == "pixelshuffle":
        ups = ["upsample.upsample.convolution"] if scale == 3 else [f"upsample.upsample.convolution_{k}" for k in range(len(_stages(scale)))]
        return ["upsample.conv_before_upsample"] + ups + ["upsample.final_convolution"]
    if upsampler == "pixelshuffledirect":
        return ["upsample.conv"]
    return ["upsample.conv_before_upsample", "upsample.conv_up1", "upsample.conv_up2", "upsample.conv_hr", "upsample.final_convolution"]


def layer_prefix(i: int, j: int) -> str:
    return f"{P}encoder.stages.{i}.layers.{j}"


def state_shapes(C: int, heads: int, hidden: int, L: int, D: int, scale: int, upsampler: str) -> dict:
    """key -> shape of every parameter of the package's state dict."""
    sh = {}

    def wb(name, w, bias=True):
        sh[f"{name}.weight"] = w
        if bias:
            sh[f"{name}.bias"] = (w[0],)

    wb(f"{P}first_convolution", (C, 3, 3, 3))
    wb(f"{P}embeddings.patch_embeddings.projection", (C, C, 1, 1))
    wb(f"{P}embeddings.patch_embeddings.layernorm", (C,))
    for i in range(L):
        for j in range(D):
            b = layer_prefix(i, j)
            a = f"{b}.attention.self"
            sh[f"{a}.logit_scale"] = (heads, 1, 1)
            wb(f"{a}.continuous_position_bias_mlp.0", (CPB, 2))
            wb(f"{a}.continuous_position_bias_mlp.2", (heads, CPB), bias=False)
            wb(f"{a}.query", (C, C))
            wb(f"{a}.key", (C, C), bias=False)
            wb(f"{a}.value", (C, C))
            wb(f"{b}.attention.output.dense", (C, C))
            wb(f"{b}.layernorm_before", (C,))
            wb(f"{b}.intermediate.dense", (hidden, C))
            wb(f"{b}.output.dense", (C, hidden))
            wb(f"{b}.layernorm_after", (C,))
        wb(f"{P}encoder.stages.{i}.conv", (C, C, 3, 3))
        wb(f"{P}encoder.stages.{i}.patch_embed.projection", (C, C, 1, 1))
    wb(f"{P}layernorm", (C,))
    wb(f"{P}conv_after_body", (C, C, 3, 3))
    names = tail_names(scale, upsampler)
    if upsampler == "pixelshuffle":
        couts = [MID] + [MID * r * r for r in _stages(scale)] + [3]
        cins = [C] + [MID] * (len(couts) - 1)
    elif upsampler == "pixelshuffledirect":
        couts, cins = [3 * scale * scale], [C]
    else:
        couts, cins = [MID, MID, MID, MID, 3], [C, MID, MID, MID, MID]
    for n, co, ci in zip(names, couts, cins):
        wb(n, (co, ci, 3, 3))
    return sh


def draw(key: str, shape, rng) -> np.ndarray:
    """One parameter re-drawn: weights ~ 1.5 / sqrt(fan_in), LayerNorm gains 1 +- 0.2, logit_scale uniform in [ln 3, ln 200]
    (ln 100 is the clamp), biases N(0, 0.05)."""
    if key.endswith("logit_scale"):
        return rng.uniform(math.log(3.0), math.log(200.0), shape).astype(np.float32)
    if "layernorm" in key:
        return (rng.uniform(0.8, 1.2, shape) if key.endswith("weight") else rng.standard_normal(shape) * 0.1).astype(np.float32)
    if key.endswith("bias"):
        return (rng.standard_normal(shape) * 0.05).astype(np.float32)
    fan_in = int(np.prod(shape[1:]))
    return (rng.standard_normal(shape) * 1.5 / math.sqrt(fan_in)).astype(np.float32)


def synthetic_state(C: int, heads: int, hidden: int, L: int, D: int, scale: int, upsampler: str, seed: int = 20261020) -> dict:
    """Seeded weights under the package's key names, drawn as the goldens' are; the first head of every layer is clamped
    (logit_scale ln 200) and the second is not (ln 5) where there are two."""
    rng = np.random.default_rng(seed)
    st = {k: draw(k, s, rng) for k, s in state_shapes(C, heads, hidden, L, D, scale, upsampler).items()}
    for k in st:
        if k.endswith("logit_scale"):
            st[k][0] = np.float32(math.log(200.0))
            if heads > 1:
                st[k][1] = np.float32(math.log(5.0))
    return st


def dims(state: dict):
    """-> (C, heads, hidden, L, D, scale, upsampler) read off the package's keys."""
    C = np.asarray(state[f"{P}first_convolution.weight"]).shape[0]
    L = len({k.split(".")[3] for k in state if k.startswith(f"{P}encoder.stages.")})
    D = len({k.split(".")[5] for k in state if k.startswith(f"{P}encoder.stages.0.layers.")})
    heads = np.asarray(state[f"{layer_prefix(0, 0)}.attention.self.logit_scale"]).shape[0]
    hidden = np.asarray(state[f"{layer_prefix(0, 0)}.intermediate.dense.weight"]).shape[0]
    if "upsample.conv_up1.weight" in state:
        return C, heads, hidden, L, D, 4, "nearest+conv"
    if "upsample.conv_before_upsample.weight" in state:
        ups = [k for k in state if k.startswith("upsample.upsample.") and k.endswith(".weight")]
        return C, heads, hidden, L, D, int(np.prod([int(round((np.asarray(state[k]).shape[0] / MID) ** 0.5)) for k in ups])), "pixelshuffle"
    return C, heads, hidden, L, D, int(round((np.asarray(state["upsample.conv.weight"]).shape[0] / 3) ** 0.5)), "pixelshuffledirect"


def to_official(state: dict) -> dict:
    """The same state under the official repository's key names (qkv stacked, q_bias / v_bias, cpb_mlp, patch_embed.proj, ...)."""
    C, heads, hidden, L, D, scale, up = dims(state)
    out = {}

    def mv(src, dst, bias=True):
        out[f"{dst}.weight"] = np.asarray(state[f"{src}.weight"])
        if bias:
            out[f"{dst}.bias"] = np.asarray(state[f"{src}.bias"])

    mv(f"{P}first_convolution", "conv_first")
    mv(f"{P}embeddings.patch_embeddings.projection", "patch_embed.proj")
    mv(f"{P}embeddings.patch_embeddings.layernorm", "patch_embed.norm")
    for i in range(L):
        for j in range(D):
            b, o = layer_prefix(i, j), f"layers.{i}.residual_group.blocks.{j}"
            a = f"{b}.attention.self"
            out[f"{o}.attn.qkv.weight"] = np.concatenate([np.asarray(state[f"{a}.{n}.weight"]) for n in ("query", "key", "value")])
            out[f"{o}.attn.q_bias"] = np.asarray(state[f"{a}.query.bias"])
            out[f"{o}.attn.v_bias"] = np.asarray(state[f"{a}.value.bias"])
            out[f"{o}.attn.logit_scale"] = np.asarray(state[f"{a}.logit_scale"])
            mv(f"{a}.continuous_position_bias_mlp.0", f"{o}.attn.cpb_mlp.0")
            mv(f"{a}.continuous_position_bias_mlp.2", f"{o}.attn.cpb_mlp.2", bias=False)
            mv(f"{b}.attention.output.dense", f"{o}.attn.proj")
            mv(f"{b}.layernorm_before", f"{o}.norm1")
            mv(f"{b}.intermediate.dense", f"{o}.mlp.fc1")
            mv(f"{b}.output.dense", f"{o}.mlp.fc2")
            mv(f"{b}.layernorm_after", f"{o}.norm2")
            # the buffers a loader must recompute, filled with what would break the forward if trusted
            out[f"{o}.attn.relative_position_index"] = np.zeros((TOK, TOK), np.int64)
            out[f"{o}.attn.relative_coords_table"] = np.full((1, 2 * WIN - 1, 2 * WIN - 1, 2), 7.0, np.float32)
            if j % 2:
                out[f"{o}.attn_mask"] = np.full((1, TOK, TOK), 7.0, np.float32)
        mv(f"{P}encoder.stages.{i}.conv", f"layers.{i}.conv")
        mv(f"{P}encoder.stages.{i}.patch_embed.projection", f"layers.{i}.patch_embed.proj")
    mv(f"{P}layernorm", "norm")
    mv(f"{P}conv_after_body", "conv_after_body")
    if up == "pixelshuffle":
        official = ["conv_before_upsample.0"] + [f"upsample.{2 * k}" for k in range(len(_stages(scale)))] + ["conv_last"]
    elif up == "pixelshuffledirect":
        official = ["upsample.0"]
    else:
        official = ["conv_before_upsample.0", "conv_up1", "conv_up2", "conv_hr", "conv_last"]
    for src, dst in zip(tail_names(scale, up), official):
        mv(src, dst)
    for k in ("img_range", "rgb_mean", "mask_value"):
        if k in state:
            out[k] = state[k]
    return out


def coords_table(dtype=np.float64) -> np.ndarray:
    """(225, 2): the log-spaced relative coordinates of a window of 8, row (dy + 7) * 15 + dx + 7.  The package builds this
    buffer once with float32 torch operators, whatever the model's dtype is afterwards (a float64 model holds the float32 values
    widened), so this does the same; the library's own table starts from float64 coordinates (a rounding-level distance)."""
    import torch
    r = torch.arange(-(WIN - 1), WIN, dtype=torch.int64).float()
    t = torch.stack(torch.meshgrid([r, r], indexing="ij")).permute(1, 2, 0).contiguous()
    t = t / (WIN - 1)
    t = t * 8
    t = torch.sign(t) * torch.log2(torch.abs(t) + 1.0) / math.log2(8)
    return t.reshape(-1, 2).numpy().astype(dtype)


def coords_table64() -> np.ndarray:
    """The same table from float64 coordinates throughout: what the library's host unit starts from (include/sr_hip.h)."""
    r = np.arange(-(WIN - 1), WIN).astype(np.float64)
    t = np.stack(np.meshgrid(r, r, indexing="ij"), -1).reshape(-1, 2) * 8.0 / (WIN - 1)
    return np.sign(t) * np.log2(np.abs(t) + 1.0) / 3.0


def cpb_table(w1, b1, w2, dtype=np.float64, sigmoid: bool = True, coords=None) -> np.ndarray:
    """(225, heads): 16 sigmoid(W2 relu(W1 c + b1)) in `dtype`; coords: the coordinate table (default: the package's)."""
    f = dtype
    c = coords_table(f) if coords is None else np.asarray(coords).astype(f)
    u = np.maximum(c @ np.asarray(w1).astype(f).T + np.asarray(b1).astype(f), f(0))
    z = u @ np.asarray(w2).astype(f).T
    return (f(16) / (f(1) + np.exp(-z))).astype(f) if sigmoid else z


def logit_scale(ls, dtype=np.float64, clamp: bool = True) -> np.ndarray:
    f = dtype
    ls = np.asarray(ls).astype(f).reshape(-1)
    return np.exp(np.minimum(ls, f(math.log(1.0 / 0.01))) if clamp else ls).astype(f)


def np_attention(qkv: np.ndarray, table: np.ndarray, scale: np.ndarray, heads: int, shift: int, mask_value: float, dtype=np.float64,
                 chain: bool = False) -> np.ndarray:
    """The header's cosine window attention on planes qkv (3 C, hp, wp) -> (C, hp, wp), before proj.  table (225, heads): the
    position bias; scale (heads,).  chain (float32 only): the documented order (fmaf chains, the division by fmaxf(n, 1e-12f), one
    multiply by the scale, + bias, + mask, the sum over keys ascending, the division, the fmaf chain over keys)."""
    f = dtype
    C3, hp, wp = qkv.shape
    C = C3 // 3
    d = C // heads
    x = np.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    win = _windows(x.astype(f)).reshape(3, heads, d, -1, TOK)           # (3, head, dd, window, token)
    q, k, v = (win[i].transpose(2, 0, 3, 1) for i in range(3))          # (window, head, token, dd)

    def unit(t):
        if chain:
            ss = np.zeros(t.shape[:-1], f)
            for dd in range(d):
                ss = _fma32(t[..., dd], t[..., dd], ss)
            n = np.sqrt(ss)
        else:
            n = np.sqrt((t * t).sum(-1))
        return (t / np.maximum(n, f(1e-12))[..., None]).astype(f)

    q, k = unit(q), unit(k)
    if chain:
        a = np.zeros(q.shape[:3] + (TOK,), f)
        for dd in range(d):
            a = _fma32(q[..., :, None, dd], k[..., None, :, dd], a)
    else:
        a = q @ k.transpose(0, 1, 3, 2)
    a = a * np.asarray(scale).astype(f)[None, :, None, None]
    bias = np.asarray(table)[rel_index().reshape(-1)].reshape(TOK, TOK, heads).transpose(2, 0, 1).astype(f)
    a = a + bias[None]
    if shift:
        a = a + (attn_mask(hp, wp) * (mask_value / -100.0)).astype(f)[:, None]
    e = np.exp(a - a.max(-1, keepdims=True))
    assert e.dtype == f
    if chain:
        s = np.zeros(e.shape[:-1], f)
        for j in range(TOK):
            s = s + e[..., j]
        p = e / s[..., None]
        o = np.zeros(q.shape, f)
        for j in range(TOK):
            o = _fma32(p[..., :, j, None], np.broadcast_to(v[..., j, None, :], o.shape), o)
    else:
        p = e / e.sum(-1, keepdims=True)
        o = p @ v
    o = o.transpose(1, 3, 0, 2).reshape(C, -1, TOK)                     # (head, dd, window, token) -> (C, window, token)
    o = _unwindows(o, hp, wp)
    return np.roll(o, (shift, shift), (1, 2)) if shift else o


def np_layernorm_add(x: np.ndarray, gamma, beta, skip: np.ndarray) -> np.ndarray:
    """skip + (float)LN(x) on planes (C, h, w) fp32 -> the float64 value of the sum of the two fp32 terms (the kernel's one fp32
    add rounds it: half an ulp)."""
    from _swinir_ref import np_layernorm
    return skip.astype(np.float64) + np_layernorm(x, gamma, beta).astype(np.float64)


def forward(state: dict, img: np.ndarray, dtype: str = "float64", mutant: str = "", mask_value: float = MASK_PACKAGE) -> np.ndarray:
    """-> (h s, w s, 3) array of `dtype`, unclamped, from a package-layout state.  mutant: what a wrong kernel or a wrong reading of
    the model would compute (MUTANTS)."""
    import torch
    import torch.nn.functional as Fn
    assert mutant in ("",) + MUTANTS
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    f = {"float32": np.float32, "float64": np.float64}[dtype]
    C, heads, hidden, L, D, scale, up = dims(state)
    d = C // heads
    rg = float(np.float32(state.get("img_range", 1.0)))
    mean = np.asarray(state.get("rgb_mean", RGB_MEAN), np.float32)
    if mutant == "mask-100":
        mask_value = -100.0
    hh, ww = img.shape[:2]
    padded = pad_image(img)
    hp, wp = padded.shape[:2]

    def tensor(key):
        return torch.from_numpy(np.array(state[key])).to(dt)

    def conv(name, y, pad=1):
        return Fn.conv2d(y, tensor(f"{name}.weight"), tensor(f"{name}.bias"), stride=1, padding=pad)

    def lin(name, y, bias=True):
        return Fn.linear(y, tensor(f"{name}.weight"), tensor(f"{name}.bias") if bias else None)

    def norm(name, y):                                                  # y: (..., C)
        return Fn.layer_norm(y, (C,), tensor(f"{name}.weight"), tensor(f"{name}.bias"), 1e-5)

    def tokens(y):                                                      # (1, C, hp, wp) -> (1, hp, wp, C)
        return y.permute(0, 2, 3, 1)

    def image(t):
        return t.permute(0, 3, 1, 2)

    def attention(b, y, shift):                                         # y: (1, hp, wp, C) -> proj(attention(y))
        a = f"{b}.attention.self"
        q, v = lin(f"{a}.query", y), lin(f"{a}.value", y)
        k = lin(f"{a}.key", y, bias=False)
        if mutant == "k-bias":
            k = k + tensor(f"{a}.query.bias")
        qkv = torch.cat([q, k, v], -1)[0].permute(2, 0, 1).numpy()
        table = cpb_table(state[f"{a}.continuous_position_bias_mlp.0.weight"], state[f"{a}.continuous_position_bias_mlp.0.bias"],
                          state[f"{a}.continuous_position_bias_mlp.2.weight"], f, sigmoid=mutant != "no-sigmoid")
        sc = logit_scale(state[f"{a}.logit_scale"], f, clamp=mutant != "no-clamp")
        if mutant == "q-scale":                                         # SwinIR's d^-1/2 on the NORMALISED q: on q itself it is no mutant,
            sc = sc * f(d ** -0.5)                                      # the normalisation removes any positive factor (measured: 0)
        o = np_attention(qkv, table, sc, heads, shift, mask_value, f)
        o = torch.from_numpy(np.ascontiguousarray(o)).permute(1, 2, 0)[None]
        return lin(f"{b}.attention.output.dense", o)

    def layer(b, x, shift):
        if mutant == "pre-norm":
            x = x + attention(b, norm(f"{b}.layernorm_before", x), shift)
            return x + lin(f"{b}.output.dense", Fn.gelu(lin(f"{b}.intermediate.dense", norm(f"{b}.layernorm_after", x))))
        x = x + norm(f"{b}.layernorm_before", attention(b, x, shift))
        return x + norm(f"{b}.layernorm_after", lin(f"{b}.output.dense", Fn.gelu(lin(f"{b}.intermediate.dense", x))))

    p = torch.from_numpy(np.array(padded)).permute(2, 0, 1)[None]
    p = p.to(torch.float64) / 255.0 if dtype == "float64" else p.to(torch.float32) / 255.0
    meant = torch.from_numpy(np.array(mean)).to(dt).view(1, 3, 1, 1)
    lrelu = Fn.leaky_relu
    with torch.no_grad():
        h0 = conv(f"{P}first_convolution", (p - meant) * rg)
        e = h0 if mutant == "no-proj" else conv(f"{P}embeddings.patch_embeddings.projection", h0, pad=0)
        t = norm(f"{P}embeddings.patch_embeddings.layernorm", tokens(e))
        for i in range(L):
            r = t
            for j in range(D):
                t = layer(layer_prefix(i, j), t, SHIFT if j % 2 else 0)
            c = conv(f"{P}encoder.stages.{i}.conv", image(t))
            if mutant != "no-proj":
                c = conv(f"{P}encoder.stages.{i}.patch_embed.projection", c, pad=0)
            t = tokens(c) + r
        y = conv(f"{P}conv_after_body", image(norm(f"{P}layernorm", t))) + (e if mutant == "skip-e" else h0)
        tn = tail_names(scale, up)
        if up == "pixelshuffle":
            y = lrelu(conv(tn[0], y), 0.01)
            for name, r in zip(tn[1:-1], _stages(scale)):
                y = Fn.pixel_shuffle(conv(name, y), r)
            y = conv(tn[-1], y)
        elif up == "pixelshuffledirect":
            y = Fn.pixel_shuffle(conv(tn[0], y), scale)
        else:
            y = lrelu(conv(tn[0], y), 0.01)
            y = lrelu(conv(tn[1], Fn.interpolate(y, scale_factor=2, mode="nearest")), 0.2)
            y = lrelu(conv(tn[2], Fn.interpolate(y, scale_factor=2, mode="nearest")), 0.2)
            y = conv(tn[4], lrelu(conv(tn[3], y), 0.2))
        o = (y / rg + meant)[:, :, :hh * scale, :ww * scale]
    return np.ascontiguousarray(o[0].permute(1, 2, 0).numpy())


def e32_of(state: dict, img: np.ndarray, f64: np.ndarray, mask_value: float = MASK_PACKAGE) -> float:
    """max |float32 forward - float64 forward|: what a correct float32 implementation is away from the truth."""
    return float(np.max(np.abs(forward(state, img, "float32", mask_value=mask_value).astype(np.float64) - f64)))


@functools.lru_cache(maxsize=None)
def case(C: int, heads: int, hidden: int, L: int, D: int, s: int, up: str, h: int, w: int, mask_value: float = MASK_PACKAGE):
    """One shared reference per case, computed once: (state, image, float64 forward, e32)."""
    state = synthetic_state(C, heads, hidden, L, D, s, up)
    img = make_image(h, w)
    f64 = forward(state, img, "float64", mask_value=mask_value)
    e32 = e32_of(state, img, f64, mask_value)
    for a in (img, f64):
        a.setflags(write=False)
    return state, img, f64, e32


def load_golden(path: str):
    """A fixture of make_swin2sr_golden.py -> (state as fp32 arrays, [(u8 image, float64 reconstruction (h s, w s, 3)), ...]).  The
    int8 tables of fixture B are value = q * 2^-shift (exact in fp32)."""
    with np.load(path, allow_pickle=False) as z:
        files = list(z.files)
        state, cases = {}, []
        for k in files:
            if k.startswith(("input.", "reconstruction.", "q8.", "q8shift.")):
                continue
            state[k] = np.asarray(z[k])
        for k in files:
            if k.startswith("q8."):
                name = k[len("q8."):]
                state[name] = (np.asarray(z[k]).astype(np.float32) * np.float32(2.0 ** -int(z["q8shift." + name]))).astype(np.float32)
        n = 0
        while f"input.{n}" in files:
            cases.append((np.asarray(z[f"input.{n}"]), np.asarray(z[f"reconstruction.{n}"])))
            n += 1
    return state, cases
