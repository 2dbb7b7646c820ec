"""NumPy / SciPy restatement of VIF in the pixel domain over four scales (MATLAB's vifp_mscale.m), written from the definition
in include/sr_hip.h.  The filter is the 2-D window (scipy.signal.correlate2d, 'valid'), so the separable kernel is held against
the unseparated form.  `mutant` switches one line of the definition to a plausible wrong one; tests/test_vif_host.py checks that
each moves the answer."""
import numpy as np
from scipy.signal import correlate2d

CHANNELS, Y, Y_ROUND = 0, 1, 2
SCALES = 4
MIN_SIDE = 41
MUTANTS = ("decimate_from_1", "same", "previous_window")


def taps(scale):
    """Side of the window of scale 1 .. 4."""
    return 2 ** (5 - scale) + 1


def fspecial(n, sd):
    """MATLAB's fspecial('gaussian', n, sd)."""
    r = np.arange(n) - (n - 1) / 2.0
    g = np.exp(-(r[:, None] ** 2 + r[None, :] ** 2) / (2.0 * sd * sd))
    g[g < np.finfo(np.float64).eps * g.max()] = 0.0
    return g / g.sum()


def window(scale):
    n = taps(scale)
    return fspecial(n, n / 5.0)


def x_int(img):
    i = img.astype(np.int64)
    return 65481 * i[..., 0] + 128553 * i[..., 1] + 24966 * i[..., 2] + 4080000


def plane(img, mode):
    """The float64 plane of a u8 image in gray-level units."""
    if img.ndim == 2 or img.shape[2] == 1:
        if mode != CHANNELS:
            raise ValueError("the Y modes need 3 channels")
        return img.reshape(img.shape[0], img.shape[1]).astype(np.float64)
    if img.shape[2] != 3 or mode == CHANNELS:
        raise ValueError("a colour image is compared on its luma")
    x = x_int(img)
    if mode == Y:
        return x.astype(np.float64) / 255000.0
    if mode == Y_ROUND:
        return ((2 * x + 255000) // 510000).astype(np.float64)
    raise ValueError("unknown mode")


def crop(img, cb):
    return img[cb:img.shape[0] - cb, cb:img.shape[1] - cb] if cb else img


def vifp(ref, dist, crop_border=0, mode=Y, mutant=None):
    """-> {'num': [4], 'den': [4], 'count': [4], 'sizes': [(h_s, w_s)], 'maps': [(mh_s, mw_s)], 'value'}; ref is the reference."""
    assert mutant is None or mutant in MUTANTS
    if ref.shape != dist.shape:
        raise ValueError("shapes differ")
    if crop_border < 0:
        raise ValueError("crop_border")
    x, y = plane(crop(ref, crop_border), mode), plane(crop(dist, crop_border), mode)
    if min(x.shape) < MIN_SIDE:
        raise ValueError(f"both sides must be at least {MIN_SIDE}")
    how = "same" if mutant == "same" else "valid"
    first = 1 if mutant == "decimate_from_1" else 0
    nums, dens, counts, sizes, maps, num_rows, den_rows = [], [], [], [], [], [], []
    for scale in range(1, SCALES + 1):
        w = window(scale)
        if scale > 1:
            wd = window(scale - 1) if mutant == "previous_window" else w
            x = correlate2d(x, wd, mode=how)[first::2, first::2]
            y = correlate2d(y, wd, mode=how)[first::2, first::2]
        mu1, mu2 = correlate2d(x, w, mode=how), correlate2d(y, w, mode=how)
        s1 = correlate2d(x * x, w, mode=how) - mu1 * mu1
        s2 = correlate2d(y * y, w, mode=how) - mu2 * mu2
        s12 = correlate2d(x * y, w, mode=how) - mu1 * mu2
        s1[s1 < 0] = 0.0
        s2[s2 < 0] = 0.0
        g = s12 / (s1 + 1e-10)
        sv = s2 - g * s12
        m = s1 < 1e-10
        g[m] = 0.0; sv[m] = s2[m]; s1[m] = 0.0
        m = s2 < 1e-10
        g[m] = 0.0; sv[m] = 0.0
        m = g < 0
        sv[m] = s2[m]; g[m] = 0.0
        sv[sv <= 1e-10] = 1e-10
        tn, td = np.log10(1.0 + g * g * s1 / (sv + 2.0)), np.log10(1.0 + s1 / 2.0)
        nums.append(float(tn.sum()))
        dens.append(float(td.sum()))
        num_rows.append(tn.sum(axis=1))
        den_rows.append(td.sum(axis=1))
        counts.append(int(mu1.size))
        sizes.append(x.shape)
        maps.append(mu1.shape)
    den = sum(dens)
    return {"num": nums, "den": dens, "count": counts, "sizes": sizes, "maps": maps, "num_rows": num_rows, "den_rows": den_rows,
            "value": sum(nums) / den if den != 0 else float("nan")}


def tile_rows(block, h):
    """The rows of `block` repeated down to h rows."""
    reps = -(-h // block.shape[0])
    return np.ascontiguousarray(np.tile(block, (reps,) + (1,) * (block.ndim - 1))[:h])


def vifp_tall(ref_block, dist_block, h, mode=Y):
    """vifp(tile_rows(ref_block, h), tile_rows(dist_block, h), 0, mode) without filtering h rows: the blocks have P rows, P a
    multiple of 8, so the planes of scale s (1-based) repeat every P / 2^(s - 1) rows (the decimation starts at row 0 and every
    period is even) and so does every row of the scale's map.  The 2-D restatement runs on three periods; the sums of the tall
    image are whole periods of its per-row sums plus a remainder, added with math.fsum.  tests/test_vif_host.py holds this
    against the direct evaluation."""
    import math
    P = ref_block.shape[0]
    assert P % 8 == 0 and h >= 3 * P and ref_block.shape == dist_block.shape
    r = vifp(tile_rows(ref_block, 3 * P), tile_rows(dist_block, 3 * P), 0, mode)
    sizes, counts = plan_sizes(h, ref_block.shape[1])
    nums, dens = [], []
    for s in range(SCALES):
        p, mh = P >> s, sizes[s][0] - taps(s + 1) + 1
        assert len(r["num_rows"][s]) >= p
        for rows, out in ((r["num_rows"][s], nums), (r["den_rows"][s], dens)):
            per = [float(v) for v in rows[:p]]
            out.append((mh // p) * math.fsum(per) + math.fsum(per[:mh % p]))
    den = sum(dens)
    return {"num": nums, "den": dens, "count": counts, "sizes": sizes, "value": sum(nums) / den if den != 0 else float("nan")}


def plan_sizes(h, w, crop_border=0):
    """The closed forms of the header: plane sizes and map sample counts of the four scales."""
    hs, ws = h - 2 * crop_border, w - 2 * crop_border
    if min(hs, ws) < MIN_SIDE:
        raise ValueError(f"both sides must be at least {MIN_SIDE}")
    sizes, counts = [], []
    for scale in range(1, SCALES + 1):
        n = taps(scale)
        if scale > 1:
            hs, ws = -(-(hs - (n - 1)) // 2), -(-(ws - (n - 1)) // 2)
        sizes.append((hs, ws))
        counts.append((hs - n + 1) * (ws - n + 1))
    return sizes, counts


def img_pair(rng, h, w, cn=3, noise=8.0, flat=None):
    """A block-structured image plus noise (no scale's den vanishes) and a noisier copy of it; flat = (y0, y1, x0, x1): a
    saturated flat patch in both."""
    shape = (h, w) if cn == 1 else (h, w, cn)
    base = rng.integers(0, 256, (h // 4 + 2, w // 4 + 2) + shape[2:]).astype(np.float64)
    up = np.repeat(np.repeat(base, 4, axis=0), 4, axis=1)[:h, :w]
    a = np.clip(np.rint(up + rng.normal(0.0, 6.0, shape)), 0, 255)
    b = np.clip(np.rint(a + rng.normal(0.0, noise, shape)), 0, 255)
    a, b = a.astype(np.uint8), b.astype(np.uint8)
    if flat is not None:
        y0, y1, x0, x1 = flat
        a[y0:y1, x0:x1] = 255
        b[y0:y1, x0:x1] = 255
    return a, b
