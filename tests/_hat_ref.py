"""Torch-CPU restatement of the HAT backend's contract (include/sr_hip.h, "HAT") -- the yardstick of tests/test_gpu_hat.py and
tests/test_hat_host.py -- plus seeded synthetic weights under HAT's key names.

PARITY UNPINNED: neither the HAT package nor a checkpoint exists offline; this file restates the published forward
(resi_connection '1conv', ape False, patch_norm True, qkv_bias True, patch_size 1, window 16, overlap ratio 0.5, upsampler
pixelshuffle) with torch's own operators (layer_norm, softmax, gelu, conv2d, linear, unfold) in float32 (what a torch user would
run) and float64 (the truth the bounds are taken against), and the two attention kernels a second time in plain numpy in the
documented order (np_window_attention, np_oca).  It reads the state dict on its own (it does not use the product's parser).
img_range, rgb_mean and conv_scale ride in the state as extra entries, the way sr_network.load_network reads them from a .npz.
Also here: the two indices, the mutants that show what the cases can see and the plan rule restated."""
from __future__ import annotations

import functools

import numpy as np

from _resnet_ref import RGB_MEAN
from _srnet_ref import check_u8, make_image, quantize  # noqa: F401  (re-exported for the tests)
from _swinir_ref import _fma32, _pad, _stages, _tail_steps, tail_extents

WIN, SHIFT, TOK, EXT, KEYS, OFF, MID = 16, 8, 256, 24, 576, 4, 64
REL_ROWS, OCA_ROWS = (2 * WIN - 1) ** 2, (WIN + EXT - 1) ** 2
IMG_RANGE = 2.0                     # not HAT's 1: a loader that drops the .npz entry must show
CONV_SCALE = 0.1                    # not HAT's 0.01, for the same reason
SA_KEY, OCA_KEY = "relative_position_index_SA", "relative_position_index_OCA"      # registered once, on the top-level module
MUTANTS = ("symmetric-pad", "masked-oca-pad", "cab-on-x", "unpadded-mean", "conv-scale-1", "shift-4")

# (C, heads, hidden, n_mid, n_squeeze, L, D, scale, h, w): the smallest that still reach every path -- 19 x 37 pads to 32 x 48
# (a corner, an edge and an interior-column window, reflection on both axes) at every scale; HAT's widths (C 180, d = 30, three
# cout tiles, n_mid 60) on 33 x 17 -> 48 x 32; HAT-S's widths (C 144, d = 24, n_mid 6) on one window whose shift wraps onto
# itself and whose enlarged window touches all four borders
CASES = [(60, 6, 120, 20, 2, 2, 2, 2, 19, 37), (60, 6, 120, 20, 2, 2, 2, 3, 19, 37), (60, 6, 120, 20, 2, 2, 2, 4, 19, 37),
         (180, 6, 360, 60, 6, 1, 2, 2, 33, 17), (144, 6, 288, 6, 6, 1, 2, 2, 16, 16)]
# the n = 1 reflection: the single row / column is repeated
EDGE_CASES = [(60, 6, 120, 20, 2, 1, 2, 2, h, w) for h, w in [(1, 21), (18, 1)]]


def case_id(c) -> str:
    return f"C{c[0]}-h{c[1]}-m{c[2]}-mid{c[3]}-sq{c[4]}-L{c[5]}-D{c[6]}-x{c[7]}-{c[8]}x{c[9]}"


def table_names(L: int, D: int, scale: int):
    """HAT's names of every table in sr_hat_create's order."""
    names = ["conv_first", "patch_embed.norm"]
    for i in range(L):
        for j in range(D):
            b = f"layers.{i}.residual_group.blocks.{j}"
            names += [f"{b}.norm1", f"{b}.attn.qkv", f"{b}.attn.relative_position_bias_table", f"{b}.attn.proj", f"{b}.conv_block.cab.0",
                      f"{b}.conv_block.cab.2", f"{b}.conv_block.cab.3.attention.1", f"{b}.conv_block.cab.3.attention.3", f"{b}.norm2",
                      f"{b}.mlp.fc1", f"{b}.mlp.fc2"]
        o = f"layers.{i}.residual_group.overlap_attn"
        names += [f"{o}.norm1", f"{o}.qkv", f"{o}.relative_position_bias_table", f"{o}.proj", f"{o}.norm2", f"{o}.mlp.fc1", f"{o}.mlp.fc2",
                  f"layers.{i}.conv"]
    names += ["norm", "conv_after_body", "conv_before_upsample.0"]
    return names + [f"upsample.{2 * k}" for k in range(len(_stages(scale)))] + ["conv_last"]


def table_shapes(C: int, heads: int, hidden: int, mid: int, sq: int, L: int, D: int, scale: int):
    """(weight shape, bias shape or None) of every table, in the same order (the 1 x 1 layers as the state holds them: 4-d)."""
    ln = ((C,), (C,))

    def conv(co, ci, k=3):
        return ((co, ci, k, k), (co,))

    mlp = [ln, ((hidden, C), (hidden,)), ((C, hidden), (C,))]
    hab = [ln, ((3 * C, C), (3 * C,)), ((REL_ROWS, heads), None), ((C, C), (C,)), conv(mid, C), conv(C, mid), conv(sq, C, 1), conv(C, sq, 1)] + mlp
    ocab = [ln, ((3 * C, C), (3 * C,)), ((OCA_ROWS, heads), None), ((C, C), (C,))] + mlp
    shapes = [conv(C, 3), ln] + (hab * D + ocab + [conv(C, C)]) * L + [ln, conv(C, C)]
    return shapes + [conv(MID, C)] + [conv(MID * r * r, MID) for r in _stages(scale)] + [conv(3, MID)]


def rel_index() -> np.ndarray:
    """(256, 256): the bias-table row of (query token i, key token j) of a 16 x 16 window, as relative_position_index_SA."""
    coords = np.stack(np.meshgrid(np.arange(WIN), np.arange(WIN), indexing="ij")).reshape(2, -1)
    rel = (coords[:, :, None] - coords[:, None, :]).transpose(1, 2, 0) + (WIN - 1)
    return rel[:, :, 0] * (2 * WIN - 1) + rel[:, :, 1]


def oca_index_raw() -> np.ndarray:
    """(256, 576): calculate_rpi_oca as recalled -- (ky - qy + 16 - 24 + 1) * 39 + (kx - qx + 16 - 24 + 1); goes negative."""
    co = np.stack(np.meshgrid(np.arange(WIN), np.arange(WIN), indexing="ij")).reshape(2, -1)
    ce = np.stack(np.meshgrid(np.arange(EXT), np.arange(EXT), indexing="ij")).reshape(2, -1)
    rel = (ce[:, None, :] - co[:, :, None]).transpose(1, 2, 0) + (WIN - EXT + 1)
    return rel[:, :, 0] * (WIN + EXT - 1) + rel[:, :, 1]


def oca_index() -> np.ndarray:
    """The default index as the library hands it out: negatives wrapped once by + 1521 (torch's indexing)."""
    raw = oca_index_raw()
    return np.where(raw < 0, raw + OCA_ROWS, raw)


def region_map(hp: int, wp: int) -> np.ndarray:
    """calculate_mask's img_mask: the region number of every pixel of the rolled image."""
    m = np.zeros((hp, wp), np.int64)
    cnt = 0
    for hs in (slice(0, -WIN), slice(-WIN, -SHIFT), slice(-SHIFT, None)):
        for ws in (slice(0, -WIN), slice(-WIN, -SHIFT), slice(-SHIFT, None)):
            m[hs, ws] = cnt
            cnt += 1
    return m


def _windows(a: np.ndarray, win: int = WIN) -> np.ndarray:
    """(..., hp, wp) -> (..., windows, win^2), windows row-major, tokens row-major."""
    hp, wp = a.shape[-2:]
    lead = a.shape[:-2]
    a = a.reshape(lead + (hp // win, win, wp // win, win))
    n = len(lead)
    return a.transpose(tuple(range(n)) + (n, n + 2, n + 1, n + 3)).reshape(lead + (-1, win * win))


def _unwindows(a: np.ndarray, hp: int, wp: int, win: int = WIN) -> np.ndarray:
    lead = a.shape[:-2]
    n = len(lead)
    a = a.reshape(lead + (hp // win, wp // win, win, win))
    return a.transpose(tuple(range(n)) + (n, n + 2, n + 1, n + 3)).reshape(lead + (hp, wp))


def attn_mask(hp: int, wp: int) -> np.ndarray:
    """(windows, 256, 256): -100 where two tokens of a window lie in different regions, else 0."""
    mw = _windows(region_map(hp, wp))
    return np.where(mw[:, None, :] != mw[:, :, None], -100.0, 0.0)


def _ext_windows(a: np.ndarray) -> np.ndarray:
    """(..., hp, wp) -> (..., windows, 576): the 24 x 24 neighbourhood of every 16 x 16 window, zeros outside the image (nn.Unfold
    with kernel 24, stride 16, padding 4)."""
    hp, wp = a.shape[-2:]
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(OFF, OFF), (OFF, OFF)])
    out = [p[..., by * WIN:by * WIN + EXT, bx * WIN:bx * WIN + EXT].reshape(a.shape[:-2] + (KEYS,))
           for by in range(hp // WIN) for bx in range(wp // WIN)]
    return np.stack(out, axis=-2)


def synthetic_state(C: int, heads: int, hidden: int, mid: int, sq: int, L: int, D: int, scale: int, seed: int = 20261020,
                    file_index: bool = False) -> dict:
    """Seeded weights under HAT's key names, scaled as tests/_swinir_ref.py scales SwinIR's (all non-trivial, so a dropped table
    shows); the CAB's 1 x 1 layers N(0, 1 / sqrt(cin)) so that the sigmoid leaves 1/2.  Also the buffers a loader must handle,
    under the bare top-level keys HAT registers them with: a correct relative_position_index_SA and -- with file_index -- the
    raw relative_position_index_OCA with its negative values; attn_mask entries of 7s (to be ignored); and img_range / rgb_mean
    / conv_scale."""
    rng = np.random.default_rng(seed)
    st = {}
    for name, (ws, bs) in zip(table_names(L, D, scale), table_shapes(C, heads, hidden, mid, sq, L, D, scale)):
        if name.endswith("relative_position_bias_table"):
            st[name] = (rng.standard_normal(ws) * 0.5).astype(np.float32)
            base = name[:-len("relative_position_bias_table")]
            if not base.endswith("overlap_attn.") and int(name.split(".")[4]) % 2:
                st[base[:-len("attn.")] + "attn_mask"] = np.full((1, TOK, TOK), 7.0, np.float32)
        elif len(ws) == 1:
            st[f"{name}.weight"] = rng.uniform(0.5, 1.5, ws).astype(np.float32)
            st[f"{name}.bias"] = (rng.standard_normal(bs) * 0.1).astype(np.float32)
        elif len(ws) == 2:
            gain = 2.0 if name.endswith("mlp.fc1") else 0.5
            st[f"{name}.weight"] = (rng.standard_normal(ws) * gain / np.sqrt(ws[1])).astype(np.float32)
            st[f"{name}.bias"] = (rng.standard_normal(bs) * 0.02).astype(np.float32)
        elif ws[2] == 1:
            st[f"{name}.weight"] = (rng.standard_normal(ws) / np.sqrt(ws[1])).astype(np.float32)
            st[f"{name}.bias"] = (rng.standard_normal(bs) * 0.1).astype(np.float32)
        else:
            gain = 0.1 if name == "conv_last" else 0.5
            st[f"{name}.weight"] = (rng.standard_normal(ws) * np.sqrt(2.0 / (9 * ws[1])) * gain).astype(np.float32)
            st[f"{name}.bias"] = (rng.standard_normal(bs) * 0.02).astype(np.float32)
    st[SA_KEY] = rel_index().astype(np.int64)
    if file_index:
        st[OCA_KEY] = oca_index_raw().astype(np.int64)
    st["img_range"] = np.array(IMG_RANGE, np.float32)
    st["rgb_mean"] = np.array(RGB_MEAN, np.float32)
    st["conv_scale"] = np.array(CONV_SCALE, np.float32)
    return st


def _dims(state: dict):
    """-> (C, heads, hidden, mid, sq, L, D, scale) read off the keys."""
    C = np.asarray(state["conv_first.weight"]).shape[0]
    L = len({k.split(".")[1] for k in state if k.startswith("layers.")})
    D = len({k.split(".")[4] for k in state if k.startswith("layers.0.residual_group.blocks.")})
    b = "layers.0.residual_group.blocks.0."
    heads = np.asarray(state[b + "attn.relative_position_bias_table"]).shape[1]
    hidden = np.asarray(state[b + "mlp.fc1.weight"]).shape[0]
    mid = np.asarray(state[b + "conv_block.cab.0.weight"]).shape[0]
    sq = np.asarray(state[b + "conv_block.cab.3.attention.1.weight"]).shape[0]
    ups = [k for k in state if k.startswith("upsample.") and k.endswith(".weight")]
    scale = int(np.prod([int(round((np.asarray(state[k]).shape[0] / MID) ** 0.5)) for k in ups]))
    return C, heads, hidden, mid, sq, L, D, scale


def _consts(state: dict):
    return (np.float32(state.get("img_range", 1.0)), np.asarray(state.get("rgb_mean", RGB_MEAN), np.float32),
            np.float32(state.get("conv_scale", 0.01)))


def reflect_index(n: int, total: int, symmetric: bool = False) -> np.ndarray:
    """Source index of every padded index: reflection without the edge pixel, m = i mod (2 n - 2), m < n ? m : 2 n - 2 - m
    (n = 1: the pixel repeated); symmetric: SwinIR's form with the edge pixel, period 2 n."""
    i = np.arange(total)
    if symmetric:
        m = i % (2 * n)
        return np.where(m < n, m, 2 * n - 1 - m)
    if n == 1:
        return np.zeros(total, np.int64)
    m = i % (2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def pad_image(img: np.ndarray, symmetric: bool = False) -> np.ndarray:
    h, w = img.shape[:2]
    return img[reflect_index(h, _pad(h, WIN), symmetric)][:, reflect_index(w, _pad(w, WIN), symmetric)]


def forward(state: dict, img: np.ndarray, dtype: str = "float64", mutant: str = "") -> np.ndarray:
    """-> (h s, w s, 3) array of `dtype`, unclamped.  mutant: what a wrong kernel would compute (MUTANTS)."""
    import torch
    import torch.nn.functional as Fn
    assert mutant in ("",) + MUTANTS
    dt = {"float32": torch.float32, "float64": torch.float64}[dtype]
    C, heads, hidden, mid, sq, L, D, scale = _dims(state)
    d = C // heads
    rng_, mean, cs = _consts(state)
    rg = float(rng_)
    cscale = 1.0 if mutant == "conv-scale-1" else float(cs)
    shift_by = 4 if mutant == "shift-4" else SHIFT
    hh, ww = img.shape[:2]
    padded = pad_image(img, symmetric=mutant == "symmetric-pad")
    hp, wp = padded.shape[:2]
    nw = (hp // WIN) * (wp // WIN)
    rel = torch.from_numpy(rel_index().reshape(-1))
    okeys = sorted(k for k in state if k.endswith(OCA_KEY))
    oca = torch.from_numpy(np.asarray(state[okeys[0]]).astype(np.int64) if okeys else oca_index()).reshape(-1)
    mask = torch.from_numpy(attn_mask(hp, wp)).to(dt)
    inside = torch.from_numpy(_ext_windows(np.ones((hp, wp)))).to(dt)             # (windows, 576): 1 inside the image

    def tensor(key):
        return torch.from_numpy(np.array(state[key])).to(dt)

    def conv(name, y, pad=1):
        return Fn.conv2d(y, tensor(f"{name}.weight"), tensor(f"{name}.bias"), stride=1, padding=pad)

    def lin(name, y):
        return Fn.linear(y, tensor(f"{name}.weight"), tensor(f"{name}.bias"))

    def norm(name, y):                                                  # y: (..., C)
        return Fn.layer_norm(y, (C,), tensor(f"{name}.weight"), tensor(f"{name}.bias"), 1e-5)

    def tokens(y):                                                      # (1, C, hp, wp) -> (1, hp, wp, C)
        return y.permute(0, 2, 3, 1)

    def image(t):
        return t.permute(0, 3, 1, 2)

    def mlp(name, x):
        return x + lin(f"{name}.mlp.fc2", Fn.gelu(lin(f"{name}.mlp.fc1", norm(f"{name}.norm2", x))))

    def window_attention(name, y, shift):                               # y: (1, hp, wp, C) -> proj(o) rolled back
        if shift:
            y = torch.roll(y, (-shift, -shift), (1, 2))
        win = y.view(1, hp // WIN, WIN, wp // WIN, WIN, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, TOK, C)
        qkv = lin(f"{name}.attn.qkv", win).reshape(-1, TOK, 3, heads, d).permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0] * (d ** -0.5), qkv[1], qkv[2]
        a = q @ k.transpose(-2, -1)
        bias = tensor(f"{name}.attn.relative_position_bias_table")[rel].view(TOK, TOK, heads).permute(2, 0, 1)
        a = a + bias[None]
        if shift:
            a = a + mask[:, None]
        a = Fn.softmax(a, -1)
        o = lin(f"{name}.attn.proj", (a @ v).transpose(1, 2).reshape(-1, TOK, C))
        o = o.view(1, hp // WIN, wp // WIN, WIN, WIN, C).permute(0, 1, 3, 2, 4, 5).reshape(1, hp, wp, C)
        return torch.roll(o, (shift, shift), (1, 2)) if shift else o

    def cab(name, y):                                                   # y: (1, hp, wp, C) -> u * s as tokens
        u = conv(f"{name}.conv_block.cab.2", Fn.gelu(conv(f"{name}.conv_block.cab.0", image(y))))
        m = (u[:, :, :hh, :ww] if mutant == "unpadded-mean" else u).mean((2, 3), keepdim=True)
        z = torch.relu(conv(f"{name}.conv_block.cab.3.attention.1", m, 0))
        return tokens(u * torch.sigmoid(conv(f"{name}.conv_block.cab.3.attention.3", z, 0)))

    def hab(name, x, shift):
        y = norm(f"{name}.norm1", x)
        x = (x + window_attention(name, y, shift)) + cab(name, x if mutant == "cab-on-x" else y) * cscale
        return mlp(name, x)

    def ocab(name, x):
        y = norm(f"{name}.norm1", x)
        qkv = lin(f"{name}.qkv", y)                                     # (1, hp, wp, 3 C)
        q = qkv[..., :C].view(1, hp // WIN, WIN, wp // WIN, WIN, C).permute(0, 1, 3, 2, 4, 5).reshape(nw, TOK, heads, d).permute(0, 2, 1, 3)
        kv = Fn.unfold(image(qkv[..., C:]), kernel_size=EXT, stride=WIN, padding=OFF)      # zero-padded AFTER the projection
        kv = kv.view(2, heads, d, KEYS, nw).permute(0, 4, 1, 3, 2)      # (2, window, head, key, dd)
        a = (q * (d ** -0.5)) @ kv[0].transpose(-2, -1)
        bias = tensor(f"{name}.relative_position_bias_table")[oca].view(TOK, KEYS, heads).permute(2, 0, 1)
        a = a + bias[None]
        if mutant == "masked-oca-pad":
            a = a + (inside[:, None, None, :] - 1.0) * 100.0
        o = (Fn.softmax(a, -1) @ kv[1]).transpose(1, 2).reshape(nw, TOK, C)
        o = lin(f"{name}.proj", o).view(1, hp // WIN, wp // WIN, WIN, WIN, C).permute(0, 1, 3, 2, 4, 5).reshape(1, hp, wp, C)
        return mlp(name, x + o)

    p = torch.from_numpy(np.array(padded)).permute(2, 0, 1)[None]
    p = (p.to(torch.float32) / 255.0).to(dt)                          # the contract's fp32 division, exact in float64 afterwards
    meant = torch.from_numpy(np.array(mean)).to(dt).view(1, 3, 1, 1)
    with torch.no_grad():
        h0 = conv("conv_first", (p - meant) * rg)
        t = norm("patch_embed.norm", tokens(h0))
        for i in range(L):
            r = t
            for j in range(D):
                t = hab(f"layers.{i}.residual_group.blocks.{j}", t, shift_by if j % 2 else 0)
            t = ocab(f"layers.{i}.residual_group.overlap_attn", t)
            t = tokens(conv(f"layers.{i}.conv", image(t))) + r
        f = conv("conv_after_body", image(norm("norm", t))) + h0
        y = Fn.leaky_relu(conv("conv_before_upsample.0", f), 0.01)
        for k, r in enumerate(_stages(scale)):
            y = Fn.pixel_shuffle(conv(f"upsample.{2 * k}", y), r)
        y = conv("conv_last", y)
        o = (y / rg + meant)[:, :, :hh * scale, :ww * scale]
    return np.ascontiguousarray(o[0].permute(1, 2, 0).numpy())


# ---------------------------------------------------------------------------------------------------------------------------
# The two attention kernels in plain numpy, in the documented order (float32) and as the same formula in float64.
# ---------------------------------------------------------------------------------------------------------------------------
def _softmax_av(q, k, v, bias, mask, f):
    """q (..., nq, dd), k / v (..., nk, dd), bias broadcastable to (..., nq, nk), mask likewise or None -> (..., nq, dd)."""
    nk, d = k.shape[-2], k.shape[-1]
    a = np.zeros(q.shape[:-1] + (nk,), f)
    for dd in range(d):
        qq, kk = q[..., :, None, dd], k[..., None, :, dd]
        a = _fma32(qq, kk, a) if f == np.float32 else a + qq * kk
    a = a + bias.astype(f)
    if mask is not None:
        a = a + mask.astype(f)
    e = np.exp(a - a.max(-1, keepdims=True))
    assert e.dtype == f
    s = np.zeros(e.shape[:-1], f)
    for j in range(nk):
        s = s + e[..., j]
    p = e / s[..., None]
    o = np.zeros(q.shape, f)
    for j in range(nk):
        pj, vj = p[..., :, j, None], v[..., j, None, :]
        o = _fma32(pj, np.broadcast_to(vj, o.shape), o) if f == np.float32 else o + pj * vj
    return o


def np_window_attention(qkv: np.ndarray, table: np.ndarray, heads: int, shift: int, dtype=np.float32) -> np.ndarray:
    """The header's 16 x 16 window attention on planes qkv (3 C, hp, wp) whose q planes are already scaled -> (C, hp, wp)."""
    f = dtype
    C3, hp, wp = qkv.shape
    C = C3 // 3
    d = C // heads
    x = np.roll(qkv, (-shift, -shift), (1, 2)) if shift else qkv
    win = _windows(x.astype(f)).reshape(3, heads, d, -1, TOK)           # (3, head, dd, window, token)
    q, k, v = (win[i].transpose(2, 0, 3, 1) for i in range(3))          # (window, head, token, dd)
    bias = np.asarray(table, np.float32)[rel_index().reshape(-1)].reshape(TOK, TOK, heads).transpose(2, 0, 1)[None]
    o = _softmax_av(q, k, v, bias, attn_mask(hp, wp)[:, None] if shift else None, f)
    o = _unwindows(o.transpose(1, 3, 0, 2).reshape(C, -1, TOK), hp, wp)
    return np.roll(o, (shift, shift), (1, 2)) if shift else o


def np_oca(qkv: np.ndarray, table: np.ndarray, index, heads: int, dtype=np.float32, masked: bool = False) -> np.ndarray:
    """The header's overlapping cross-attention on planes qkv (3 C, hp, wp) -> (C, hp, wp).  index: (256, 576) with values in
    [-1521, 1520] (negatives wrap) or None for the default.  masked: the wrong form that masks the keys outside the image."""
    f = dtype
    C3, hp, wp = qkv.shape
    C = C3 // 3
    d = C // heads
    x = qkv.astype(f)
    q = _windows(x[:C]).reshape(heads, d, -1, TOK).transpose(2, 0, 3, 1)            # (window, head, query, dd)
    k = _ext_windows(x[C:2 * C]).reshape(heads, d, -1, KEYS).transpose(2, 0, 3, 1)   # (window, head, key, dd)
    v = _ext_windows(x[2 * C:]).reshape(heads, d, -1, KEYS).transpose(2, 0, 3, 1)
    idx = oca_index() if index is None else np.asarray(index)
    idx = np.where(idx < 0, idx + OCA_ROWS, idx)
    bias = np.asarray(table, np.float32)[idx.reshape(-1)].reshape(TOK, KEYS, heads).transpose(2, 0, 1)[None]
    mask = (_ext_windows(np.ones((hp, wp))) - 1.0)[:, None, None, :] * 100.0 if masked else None
    o = _softmax_av(q, k, v, bias, mask, f)
    return _unwindows(o.transpose(1, 3, 0, 2).reshape(C, -1, TOK), hp, wp)


@functools.lru_cache(maxsize=None)
def case(C: int, heads: int, hidden: int, mid: int, sq: int, L: int, D: int, s: int, h: int, w: int):
    """One shared reference per case, computed once: (state, image, float64 forward, e32 = max|float32 - float64|)."""
    state = synthetic_state(C, heads, hidden, mid, sq, L, D, s)
    img = make_image(h, w)
    f64 = forward(state, img, "float64")
    f32 = forward(state, img, "float32")
    e32 = float(np.max(np.abs(f32.astype(np.float64) - f64)))
    for a in (img, f64):
        a.setflags(write=False)
    return state, img, f64, e32


# ---------------------------------------------------------------------------------------------------------------------------
# The plan rule of include/sr_hip.h (sr_hat_plan), restated.
# ---------------------------------------------------------------------------------------------------------------------------
TRUNK_CAP = 32 << 30
DEFAULT_TAIL = 256


def bytes_per_pixel(C: int, hidden: int, mid: int) -> int:
    return 4 * (5 * _pad(C, 64) + _pad(mid, 64) + max(_pad(3 * C, 64), _pad(hidden, 64)))


def plan(C: int, hidden: int, mid: int, scale: int, h: int, w: int, tail: int = 0):
    """-> (padded rows, padded columns, the tail's halo, tail sub-pieces, workspace bytes) as the header states them."""
    steps = _tail_steps(scale, "pixelshuffle")
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
    ws = bytes_per_pixel(C, hidden, mid) * p0 + 4 * 2 * MID * p4 + 3 * p0 + 8 * C * -(-hp // 32) + 4 * C
    return hp, wp, g, -(-h // tail) * -(-w // tail), ws
