"""Generates tests/golden/deltae_skimage.npz with scikit-image 0.18.3: u8 image pairs and, for each, scikit-image's rgb2lab of
image 1 and its deltaE_ciede2000 / deltaE_cie76 maps of the pair, all float64 -- the definition of include/sr_hip.h's colour
difference.  Cases (`cases` lists the names; arrays are <name>_a, <name>_b, <name>_lab1, <name>_de00, <name>_de76):
  noisy      60 x 90 RGB: a smooth colourful image and a noisy, tinted partner (some pixels byte-equal)
  rows       24 x 90 RGB: 6 rows of equal pixels, 12 rows of unrelated colours (both hue wraps and both h_sum branches occur at
             least 10 times each: asserted), 6 rows with a black partner on either side (the C1' C2' == 0 branch)
  primaries  8 x 8 RGB: black, white, the saturated primaries and their complements, each against each
  gray       9 x 13, one channel, used as R = G = B
  rgba       7 x 11 x 4, alpha random and ignored
and constructed Lab pairs that no u8 pixel reaches (lab_pairs [n, 2, 3], lab_de00, lab_de76): hue differences of exactly pi with
unequal chromas (the strict comparisons decide), a zero chroma on one side (Hbar is the sum of the hues), equal triples.

The generator asserts on the reference alone, and reseeds until both hold (no test excludes a pixel):
  (a) no image pixel with C1' C2' != 0 has | |h_diff| - pi | < 1e-6: dE00 is discontinuous there;
  (b) no non-zero reference dE has 16 dE within 1e-6 of an integer, for either formula: a rounding could move a histogram count.

Regenerating does not reproduce the committed bits.  scikit-image's rgb2xyz is a matrix product handed to BLAS, whose order
of additions (and use of fused multiply-add) follows the CPU and the thread count: a second run with the same seed gives the
same inputs, wrap counts and closest approaches, but Lab and dE values that differ from the committed ones by up to about
2e-13 (only `primaries`, whose linear values are 0 or 1, is bit-equal).  "Each row summed left to right" in include/sr_hip.h
is therefore this project's choice within scikit-image's own spread, and the distances the tests print against the fixture
(about 4e-13 on the host, 3e-13 on the device) move by up to half of that with a regenerated fixture: that is no regression
while they stay below the bars (1e-12 host, 1e-9 device).

Run with an interpreter that has scikit-image 0.18.3:
    python tests/golden/make_deltae_golden.py
Inputs are stored next to the expected values, so nothing depends on RNG stream stability.
"""
import os
import sys
import warnings

import numpy as np

warnings.filterwarnings("ignore")
from skimage import __version__ as skv
from skimage.color import deltaE_cie76, deltaE_ciede2000, rgb2lab

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _deltae_ref as R


def make(seed):
    rng = np.random.default_rng(seed)
    cases = {}
    cases["noisy"] = R.img_pair(rng, 60, 90, 3)
    a = rng.integers(0, 256, (24, 90, 3), dtype=np.uint8)
    b = rng.integers(0, 256, (24, 90, 3), dtype=np.uint8)
    b[:6] = a[:6]
    b[18:21] = 0
    a[21:24] = 0
    a[23, ::2] = 0; b[23, ::2] = 0                      # black against black
    cases["rows"] = (a, b)
    cols = np.array([[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [0, 255, 255], [255, 0, 255],
                     [255, 255, 0]], np.uint8)
    cases["primaries"] = (np.ascontiguousarray(np.repeat(cols[:, None, :], 8, 1)), np.ascontiguousarray(np.repeat(cols[None], 8, 0)))
    cases["gray"] = R.img_pair(rng, 9, 13, 1)
    cases["rgba"] = R.img_pair(rng, 7, 11, 4)
    return cases


def reference(cases):
    out = {}
    for name, (a, b) in cases.items():
        l1, l2 = rgb2lab(R.to_rgb(a)), rgb2lab(R.to_rgb(b))
        out[name] = (l1, l2, deltaE_ciede2000(l1, l2), deltaE_cie76(l1, l2))
    return out


def conditions(ref):
    """(closest approach to (a), closest approach to (b), wrap counts) over every image case, from the reference alone."""
    near_pi, near_edge = np.inf, np.inf
    counts = {"over": 0, "under": 0, "sum_low": 0, "sum_high": 0, "zero_chroma": 0}
    for l1, l2, de00, de76 in ref.values():
        _, p = R.ciede2000(l1, l2, parts=True)
        live = p["CC"] != 0.0
        if live.any():
            near_pi = min(near_pi, float(np.abs(np.abs(p["h_diff"][live]) - np.pi).min()))
        wrapped = live & (np.abs(p["h_diff"]) > np.pi)
        counts["over"] += int((live & (p["h_diff"] > np.pi)).sum())
        counts["under"] += int((live & (p["h_diff"] < -np.pi)).sum())
        counts["sum_low"] += int((wrapped & (p["h_sum"] < 2 * np.pi)).sum())
        counts["sum_high"] += int((wrapped & (p["h_sum"] >= 2 * np.pi)).sum())
        counts["zero_chroma"] += int((~live).sum())
        for d in (de00, de76):
            nz = d[d != 0.0]
            if nz.size:
                near_edge = min(near_edge, float(np.abs(16.0 * nz - np.round(16.0 * nz)).min()))
    return near_pi, near_edge, counts


seed = 20261020
while True:
    cases = make(seed)
    ref = reference(cases)
    near_pi, near_edge, counts = conditions(ref)
    if near_pi >= 1e-6 and near_edge >= 1e-6:
        break
    seed += 1
assert near_pi >= 1e-6 and near_edge >= 1e-6
assert min(counts.values()) >= 10, counts
for name, (a, b) in cases.items():                       # equal pixels give exactly 0 in scikit-image, for both formulas
    same = np.all(R.to_rgb(a) == R.to_rgb(b), axis=-1)
    assert (ref[name][2][same] == 0.0).all() and (ref[name][3][same] == 0.0).all(), name
assert cases["noisy"][0].shape == (60, 90, 3) and np.all(R.to_rgb(cases["noisy"][0]) == R.to_rgb(cases["noisy"][1]), axis=-1).sum() > 100

lab_pairs = np.array([
    [[50.0, 10.0, 0.0], [50.0, -10.0, 0.0]],             # h_diff == pi exactly, equal chromas
    [[50.0, 10.0, 0.0], [50.0, -20.0, 0.0]],             # ... unequal chromas: the rotation term sees the sign of dH and Hbar
    [[50.0, -20.0, 0.0], [50.0, 10.0, 0.0]],             # h_diff == -pi exactly
    [[60.0, 30.0, 0.0], [40.0, -5.0, 0.0]],
    [[50.0, 0.0, 0.0], [50.0, -10.0, -10.0]],            # a zero chroma: Hbar is the sum of the hues
    [[30.0, 5.0, -40.0], [70.0, 0.0, 0.0]],
    [[50.0, 0.0, 0.0], [60.0, 0.0, 0.0]],                # both chromas zero
    [[50.0, 2.5, -7.0], [50.0, 2.5, -7.0]],              # equal triples
    [[50.0, 2.6772, -79.7751], [50.0, 0.0, -82.7485]],   # Sharma, Wu, Dalal: pair 1 of their table (2.0425)
    [[50.0, -1.0, 2.0], [50.0, 0.0, 0.0]],               # ... pair 8 (2.3669)
], np.float64)
lab_de00 = np.array([deltaE_ciede2000(p[0], p[1]) for p in lab_pairs], np.float64)
lab_de76 = np.array([deltaE_cie76(p[0], p[1]) for p in lab_pairs], np.float64)
assert abs(lab_de00[8] - 2.0425) < 5e-5 and abs(lab_de00[9] - 2.3669) < 5e-5 and lab_de00[7] == 0.0

arrays = {"cases": np.array(list(cases)), "skimage_version": np.array(skv), "seed": np.array(seed),
          "closest_to_pi": np.array(near_pi), "closest_to_bin_edge": np.array(near_edge),
          "wrap_counts": np.array([counts[k] for k in ("over", "under", "sum_low", "sum_high", "zero_chroma")]),
          "lab_pairs": lab_pairs, "lab_de00": lab_de00, "lab_de76": lab_de76}
for name, (a, b) in cases.items():
    l1, _, de00, de76 = ref[name]
    arrays.update({f"{name}_a": a, f"{name}_b": b, f"{name}_lab1": l1.astype(np.float64), f"{name}_de00": de00.astype(np.float64),
                   f"{name}_de76": de76.astype(np.float64)})
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "deltae_skimage.npz")
np.savez_compressed(path, **arrays)
print(f"scikit-image {skv}, seed {seed}: closest to pi {near_pi:.3g}, closest to a bin edge {near_edge:.3g}, {counts}; "
      f"{os.path.getsize(path)} bytes -> {path}")
