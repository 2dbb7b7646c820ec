#!/usr/bin/env python3
"""Writes tests/golden/swin2sr_direct_x2.npz (fixture A) and tests/golden/swin2sr_shuffle_x2.npz (fixture B): random-weight
Swin2SRForImageSuperResolution models of the `transformers` package run on the CPU in float64.

Run it where `transformers` imports (5.15.0 wrote the committed files); no test imports this script and nothing is fetched: the
models are built from a Swin2SRConfig.  Every parameter is re-drawn (tests/_swin2sr_ref.draw: weights ~ 1.5 / sqrt(fan_in),
LayerNorm gains 1 +- 0.2, logit_scale uniform in [ln 3, ln 200], so that heads on both sides of the clamp at ln 100 occur --
asserted), rounded to fp32, loaded into a float64 model, and the model's `reconstruction` is stored as float64 beside the fp32
weights under the package's key names and the u8 inputs.

  A  pixelshuffledirect x2, C 24, 2 heads (d 12), two stages of two layers, hidden 48; inputs 8 x 8 (one window: the shift wraps
     onto itself) and 16 x 24.
  B  pixelshuffle x2, the same trunk; input 16 x 24.  The three 64-feature tables of the reconstruction are drawn as small
     integers times 2^-k and stored as int8 ("q8.<key>" with "q8shift.<key>" = k), so that the file stays below the largest
     fixture already committed.

Sides are multiples of 8: the package's own model fails on any other (its patch_unembed is given the unpadded size).

Before a fixture is written the restatement (tests/_swin2sr_ref.py) must reproduce the package's output to 1e-9 in float64, and
every mutant of the restatement must land outside 8 e32 of it (e32: the float32 restatement's distance from the float64 one) --
the -100 mask on at least one input of the fixture, see make(); the weights are re-drawn with the next seed until both hold.
The "q scaled by d^-1/2" mutant scales the NORMALISED q: scaling q itself changes nothing, the normalisation removes it."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _swin2sr_ref as R  # noqa: E402

C, HEADS, HIDDEN, L, D, SCALE = 24, 2, 48, 2, 2, 2
SIZE_CAP = 416 * 1024
Q8 = {"upsample.conv_before_upsample.weight": 7, "upsample.upsample.convolution_0.weight": 8, "upsample.final_convolution.weight": 8}


def package_model(upsampler: str):
    from transformers import Swin2SRConfig, Swin2SRForImageSuperResolution
    cfg = Swin2SRConfig(image_size=64, patch_size=1, num_channels=3, num_channels_out=3, embed_dim=C, depths=[D] * L, num_heads=[HEADS] * L,
                        window_size=8, mlp_ratio=HIDDEN / C, qkv_bias=True, upscale=SCALE, img_range=1.0, resi_connection="1conv",
                        upsampler=upsampler, use_absolute_embeddings=False)
    return Swin2SRForImageSuperResolution(cfg).double().eval()


def draw_state(model, seed: int) -> dict:
    import torch
    rng = np.random.default_rng(seed)
    st = {}
    for key, p in model.state_dict().items():
        if key in Q8:                                       # small integers times 2^-k: exact in int8 and in fp32
            fan_in = int(np.prod(p.shape[1:]))
            q = np.clip(np.rint(rng.standard_normal(tuple(p.shape)) * 1.5 / math.sqrt(fan_in) * 2.0 ** Q8[key]), -127, 127)
            st[key] = (q * 2.0 ** -Q8[key]).astype(np.float32)
        else:
            st[key] = R.draw(key, tuple(p.shape), rng)
    clamp = math.log(100.0)
    for key, a in st.items():
        if key.endswith("logit_scale"):
            a.reshape(-1)[0], a.reshape(-1)[1] = np.float32(math.log(200.0)), np.float32(rng.uniform(math.log(3.0), math.log(50.0)))
            assert (a > clamp).any() and (a < clamp).any()
    model.load_state_dict({k: torch.from_numpy(v).double() for k, v in st.items()})
    return st


def run_package(model, img: np.ndarray) -> np.ndarray:
    import torch
    x = torch.from_numpy(img).permute(2, 0, 1)[None].double() / 255.0
    with torch.no_grad():
        y = model(pixel_values=x).reconstruction
    return np.ascontiguousarray(y[0].permute(1, 2, 0).numpy())


def make(upsampler: str, sizes, path: str, first_seed: int):
    model = package_model(upsampler)
    for seed in range(first_seed, first_seed + 50):
        st = draw_state(model, seed)
        imgs = [R.make_image(h, w) for h, w in sizes]
        outs = [run_package(model, im) for im in imgs]
        ratios = []
        for im, out in zip(imgs, outs):
            f64 = R.forward(st, im, "float64")
            err = float(np.max(np.abs(f64 - out)))
            assert err <= 1e-9, f"the restatement is {err:.3e} from the package"
            e32 = R.e32_of(st, im, out)
            seen = {}
            for m in R.MUTANTS:
                seen[m] = float(np.max(np.abs(R.forward(st, im, "float64", mutant=m) - out))) / e32
            print(f"{os.path.basename(path)} seed {seed} {im.shape[0]}x{im.shape[1]}: range [{out.min():.2f}, {out.max():.2f}]  e32 {e32:.2e}  "
                  f"restatement {err:.1e}  mutants / e32: " + "  ".join(f"{k} {v:.0f}" for k, v in seen.items()))
            ratios.append(seen)
        # every mutant outside 8 e32 of every stored output -- except the -100 mask, which must show on at least one of them: for
        # it to show at all, a masked key's score must come within about 10 of the row's maximum after only -100, that is, lie
        # some 90 above every unmasked key's of the at most 200 + 16 the scale and the bias span; in the single wrapped window of
        # the 8 x 8 input no draw of 50 produced that (ratio 0 every time), in the 16 x 24 input about one draw in five does
        if all(v > 8.0 for seen in ratios for m, v in seen.items() if m != "mask-100") and max(seen["mask-100"] for seen in ratios) > 8.0:
            break
    else:
        raise SystemExit("no seed separates every mutant")
    arrays = {}
    for k, v in st.items():
        if k in Q8:
            arrays["q8." + k] = np.rint(v.astype(np.float64) * 2.0 ** Q8[k]).astype(np.int8)
            arrays["q8shift." + k] = np.array(Q8[k], np.int32)
        else:
            arrays[k] = v
    for n, (im, out) in enumerate(zip(imgs, outs)):
        arrays[f"input.{n}"] = im
        arrays[f"reconstruction.{n}"] = out
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size <= SIZE_CAP, f"{path}: {size} bytes is above the cap of {SIZE_CAP}"
    st2, cases = R.load_golden(path)                        # what the tests will read is what was run
    assert all(np.array_equal(st2[k], st[k]) for k in st) and len(cases) == len(imgs)
    print(f"wrote {path}: {size} bytes")


if __name__ == "__main__":
    import transformers
    print("transformers", transformers.__version__)
    make("pixelshuffledirect", [(8, 8), (16, 24)], os.path.join(HERE, "swin2sr_direct_x2.npz"), 37)
    make("pixelshuffle", [(16, 24)], os.path.join(HERE, "swin2sr_shuffle_x2.npz"), 101)
