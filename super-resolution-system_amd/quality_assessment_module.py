"""quality_assessment_module -- MI355X-native mirror of the reference's full-reference metrics.

Call surface of quality_assessment_module.py:35-133,169-195,226-417,467-609: same class / method
names, arguments, return types and crop / preprocess rules.  PSNR (exact integer sum of squared
differences), RGB->gray, the three SSIM variants and the bicubic resize run as HIP kernels behind the
C ABI; only the final scalar formulas run on the host.  No CPU compute fallback.

SSIM branches: the reference calls skimage with ``multichannel=False``; a skimage that
accepts / ignores the keyword gives branch A (uniform 7x7 for ``multiscale=False``, Gaussian sigma 1.5
for ``multiscale=True``, cropped mean); one that rejects it gives branch B (``_calculate_ssim_simple``
for both).  ``ssim_branch`` selects it ('A' default).  ``gray_shift`` selects OpenCV's 15-bit (>= 4.x,
default) or 14-bit RGB2GRAY constants.

LPIPS (quality_assessment_module.py:135-146,197-224,419-465): the AlexNet / VGG16 forward of the ``lpips`` package
runs as hand-written fp32 MFMA convolutions (csrc/sr_lpips.hip), streamed in tiles so a 200 MP pair fits.  The
reference's constructor downloads pretrained weights by model name; this one never fetches anything: weights come
from ``lpips_weights={'vgg': <.npz path or dict>, 'alex': ...}`` (or SR_LPIPS_WEIGHTS_VGG / SR_LPIPS_WEIGHTS_ALEX),
a flat .npz of ``lpips.LPIPS(net).state_dict()`` arrays read with allow_pickle=False.  Without weights
``lpips_model_vgg`` stays None exactly like the reference when its import fails: ``evaluate_full_reference`` omits
the LPIPS keys and ``calculate_lpips`` raises RuntimeError.

No-reference and commercial metrics (quality_assessment_module.py:611-1193): ``evaluate_commercial`` (and
``evaluate_commercial_device`` for a canvas already in HBM) and ``evaluate_no_reference`` run every metric -- Laplacian
sharpness, contrast, 8-bit Lab colour statistics, YCrCb skin ratio, 5x5 texture, 3x3 noise residual, 8x8 block artifacts,
brightness regions, Canny edge density, the DFT high-frequency ratio and the MSCN / Sobel NIQE and BRISQUE stand-ins -- in
one sr_commercial_u8 call (csrc/sr_commercial.hip), all ROIs included; the host only finishes the scalar formulas and
keeps the reference's key order.  The pyiqa NIQE / BRISQUE models stay unavailable (``_niqe_available`` is False).

NIQE proper (no reference counterpart in code: the reference asks pyiqa for it): ``calculate_niqe_model`` /
``niqe_features`` / ``fit_niqe_model`` run the model of Mittal et al. as include/sr_hip.h defines it (csrc/sr_niqe.hip), with
pristine parameters the caller supplies or fits.  ``calculate_niqe`` and the 'niqe' report key stay the reference's MSCN
stand-in: another number under a similar name.

BRISQUE proper, likewise: ``calculate_brisque_model`` / ``brisque_features`` run the model of Mittal, Moorthy and Bovik as
include/sr_hip.h defines it (csrc/sr_brisque.hip) under an RBF epsilon-SVR the caller supplies (``load_brisque_model``,
``brisque_model_from_libsvm``; none ships).  ``calculate_brisque`` and the 'brisque' report key stay the reference's stand-in.
u8 HxW, HxWx3 and HxWx4 (alpha ignored) images only; an image side above the FFT's longest line (32768) raises
NotImplementedError before any device work.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, field
from enum import Enum
from typing import Any, Dict, List, Optional, Tuple, Union

import numpy as np

import _native


class AssessmentLevel(Enum):
    EXCELLENT = "excellent"
    GOOD = "good"
    FAIR = "fair"
    POOR = "poor"
    BAD = "bad"


@dataclass
class QualityThresholds:
    """quality_assessment_module.py:44-75."""
    PSNR_EXCELLENT: float = 40.0
    PSNR_GOOD: float = 35.0
    PSNR_FAIR: float = 30.0
    SSIM_EXCELLENT: float = 0.98
    SSIM_GOOD: float = 0.95
    SSIM_FAIR: float = 0.90
    LPIPS_EXCELLENT: float = 0.02
    LPIPS_GOOD: float = 0.05
    LPIPS_FAIR: float = 0.10
    NIQE_EXCELLENT: float = 3.0
    NIQE_GOOD: float = 5.0
    NIQE_FAIR: float = 8.0
    BRISQUE_EXCELLENT: float = 20.0
    BRISQUE_GOOD: float = 35.0
    BRISQUE_FAIR: float = 50.0
    DELTA_E_EXCELLENT: float = 1.0
    DELTA_E_GOOD: float = 3.0
    DELTA_E_FAIR: float = 5.0


@dataclass
class ScaleConfig:
    """quality_assessment_module.py:78-86."""
    scale_factors: List[float] = field(default_factory=lambda: [0.1, 0.2, 0.4])
    scale_names: Dict[float, str] = field(default_factory=lambda: {
        0.1: "structure_color", 0.2: "mid_frequency", 0.4: "high_frequency"})


class _DevImage:
    """A u8 image resident in HBM (dense HWC or HW): uploaded from an array, freshly allocated, or a view of memory
    somebody else owns (``ptr=``: the device-resident pipeline hands its source and canvas over this way)."""

    def __init__(self, ctx, arr: Optional[np.ndarray] = None, shape=None, ptr: Optional[int] = None):
        self.ctx = ctx
        self._ptr = None
        if ptr is not None:
            self.shape = tuple(shape)
            self.buf = None
            self._ptr = int(ptr)
        elif arr is not None:
            arr = np.ascontiguousarray(arr, dtype=np.uint8)
            self.shape = arr.shape
            self.buf = ctx.upload(arr)
        else:
            self.shape = tuple(shape)
            self.buf = ctx.alloc(int(np.prod(self.shape)))

    @property
    def h(self): return self.shape[0]

    @property
    def w(self): return self.shape[1]

    @property
    def cn(self): return self.shape[2] if len(self.shape) == 3 else 1

    @property
    def stride(self): return self.w * self.cn

    @property
    def ptr(self): return self._ptr if self.buf is None else self.buf.ptr

    def free(self):
        if self.buf is not None:
            self.buf.free()


class QualityAssessmentModule:
    def __init__(self, device: str = 'cpu', thresholds: Optional[QualityThresholds] = None,
                 scale_config: Optional[ScaleConfig] = None, gpu_index: int = 0, ssim_branch: str = 'A',
                 gray_shift: int = 15, lpips_weights: Optional[Dict[str, Any]] = None, lpips_tile: int = 4096,
                 dists_weights: Any = None, dists_tile: int = 4096):
        # the reference's `device` only places the LPIPS networks; the metrics here always run on the GPU
        self.device = device
        self.thresholds = thresholds or QualityThresholds()
        self.scale_config = scale_config or ScaleConfig()
        self.gpu_index = gpu_index
        if ssim_branch not in ('A', 'B'):
            raise ValueError("ssim_branch must be 'A' or 'B'")
        self.ssim_branch = ssim_branch
        self.gray_shift = gray_shift
        self.lpips_tile = int(lpips_tile)
        self.lpips_model_vgg = None      # stay None without caller-supplied weights (nothing is fetched)
        self.lpips_model_alex = None
        self._init_lpips_models(lpips_weights)
        self.dists_tile = int(dists_tile)
        self.dists_model = None          # stays None without caller-supplied weights (nothing is fetched)
        self._init_dists_model(dists_weights)
        self._niqe_available = False
        self._brisque_available = False

    def _ctx(self) -> "_native.Context":
        return _native.default_context(self.gpu_index)

    def _init_lpips_models(self, lpips_weights: Optional[Dict[str, Any]] = None) -> None:
        """quality_assessment_module.py:135-146 without the download: build the GPU models from caller-supplied
        state-dict arrays ({'vgg': path | dict, 'alex': path | dict}; env SR_LPIPS_WEIGHTS_<NET> as a default)."""
        src = dict(lpips_weights or {})
        for net in ("vgg", "alex"):
            if net not in src and os.environ.get(f"SR_LPIPS_WEIGHTS_{net.upper()}"):
                src[net] = os.environ[f"SR_LPIPS_WEIGHTS_{net.upper()}"]
        for net, w in src.items():
            if net not in ("vgg", "alex"):
                raise ValueError(f"lpips_weights: unknown net {net!r}")
            if isinstance(w, (str, os.PathLike)):
                w = _native.load_lpips_weights(os.fspath(w))
            setattr(self, f"lpips_model_{net}", _native.LpipsModel(self._ctx(), net, w))

    def _init_dists_model(self, dists_weights: Any = None) -> None:
        """DISTS from caller-supplied arrays: a flat .npz path or a dict (env SR_DISTS_WEIGHTS as a default) holding the VGG16
        convolutions and alpha / beta under the names _native.dists_pack_weights documents."""
        w = dists_weights if dists_weights is not None else (os.environ.get("SR_DISTS_WEIGHTS") or None)
        if w is None:
            return
        if isinstance(w, (str, os.PathLike)):
            w = _native.load_dists_weights(os.fspath(w))
        self.dists_model = _native.DistsModel(self._ctx(), w)

    # -- preprocessing (quality_assessment_module.py:169-195, 304-308) --------------------------------
    def _preprocess_image(self, image: Any, to_tensor: bool = False) -> np.ndarray:
        if hasattr(image, "detach") and hasattr(image, "dim"):        # torch tensor, CHW or 1xCHW
            if image.dim() == 4:
                image = image.squeeze(0)
            if image.dim() == 3:
                image = image.permute(1, 2, 0)
            image = image.detach().cpu().numpy()
        elif not isinstance(image, np.ndarray):                        # PIL image (main.py hands these in)
            image = np.asarray(image)
        if image.max() <= 1.0:
            image = (image * 255).astype(np.uint8)
        return image

    @staticmethod
    def _crop_pair(a: np.ndarray, b: np.ndarray):
        if a.shape != b.shape:
            mh, mw = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
            a, b = a[:mh, :mw], b[:mh, :mw]
        return a, b

    @staticmethod
    def _require_u8(img: np.ndarray, what: str) -> np.ndarray:
        if img.dtype != np.uint8:
            raise NotImplementedError(f"{what}: only uint8 images (after the reference's preprocess rule) are on "
                                      f"the HIP path; got {img.dtype}")
        return np.ascontiguousarray(img)

    # -- resize -------------------------------------------------------------------------------------------
    def _resize_dev(self, src: _DevImage, new_h: int, new_w: int) -> _DevImage:
        out_shape = (new_h, new_w, src.cn) if len(src.shape) == 3 else (new_h, new_w)
        dst = _DevImage(src.ctx, shape=out_shape)
        src.ctx.resize_cubic_u8(src.ptr, src.stride, src.h, src.w, src.cn, dst.ptr, dst.stride, new_h, new_w)
        return dst

    def downsample_bicubic(self, image: np.ndarray, scale_factor: float) -> np.ndarray:
        if scale_factor >= 1.0 or scale_factor <= 0:
            raise ValueError(f"scale_factor必须在(0, 1)范围内，当前值: {scale_factor}")
        h, w = image.shape[:2]
        return self.upsample_bicubic(image, (int(h * scale_factor), int(w * scale_factor)))

    def upsample_bicubic(self, image: np.ndarray, target_size: Tuple[int, int]) -> np.ndarray:
        img = self._require_u8(np.asarray(image), "bicubic resize")
        ctx = self._ctx()
        src = _DevImage(ctx, img)
        dst = self._resize_dev(src, int(target_size[0]), int(target_size[1]))
        out = ctx.download(dst.ptr, dst.shape, np.uint8)
        src.free(); dst.free()
        return out

    # -- MATLAB's bicubic imresize (no reference counterpart: the degradation of the classical SR benchmarks) ------------------
    _IMRESIZE_OUT = {np.dtype(np.uint8): _native.IMRESIZE_U8, np.dtype(np.float32): _native.IMRESIZE_F32,
                     np.dtype(np.float64): _native.IMRESIZE_F64}

    @classmethod
    def _imresize_args(cls, shape, scale, output_shape, antialiasing, dtype):
        """Every refusal of the imresize methods, on the host: ValueError, or SrNativeError naming the range for a scale
        outside [1/16, 16].  -> (h, w, cn, scale_y, scale_x, dh, dw, out_type, element size, output shape)."""
        shape = tuple(int(v) for v in shape)
        if len(shape) not in (2, 3):
            raise ValueError(f"imresize: need an H x W or H x W x C image, got shape {shape}")
        cn = shape[2] if len(shape) == 3 else 1
        try:
            out_type = cls._IMRESIZE_OUT[np.dtype(dtype)]
        except (KeyError, TypeError) as exc:
            raise ValueError(f"imresize: dtype must be uint8, float32 or float64, got {dtype!r}") from exc
        sy, sx, dh, dw = _native.imresize_geometry(shape[0], shape[1], scale, output_shape)
        _native.imresize_plan(shape[0], shape[1], cn, sy, sx, dh, dw, bool(antialiasing))      # cn, the scale range
        out_shape = (dh, dw, cn) if len(shape) == 3 else (dh, dw)
        return shape[0], shape[1], cn, sy, sx, dh, dw, out_type, np.dtype(dtype).itemsize, out_shape

    def imresize(self, image: np.ndarray, scale: Optional[float] = None, output_shape: Optional[Tuple[int, int]] = None,
                 antialiasing: bool = True, dtype=np.uint8) -> np.ndarray:
        """MATLAB's imresize(image, scale) / imresize(image, [dh dw]) with the bicubic kernel (a = -0.5, antialiased below 1,
        symmetric border), as include/sr_hip.h defines it and BasicSR's matlab_functions.imresize restates it: the resize
        the SR benchmarks make their low-resolution inputs with.  NOT downsample_bicubic / upsample_bicubic, which stay
        OpenCV's INTER_CUBIC.  Give exactly one of `scale` (both axes use it, sides ceil(n * scale)) and `output_shape`.
        u8 image H x W or H x W x C (C 1, 3 or 4), each axis scale in [1/16, 16].  dtype uint8: rounded half up and
        saturated; float32 / float64: the unclamped value in gray levels."""
        img = self._require_u8(np.asarray(image), "imresize")
        args = self._imresize_args(img.shape, scale, output_shape, antialiasing, dtype)
        h, w, cn, sy, sx, dh, dw, out_type, item, out_shape = args
        ctx = self._ctx()
        src, dst = _DevImage(ctx, img), None
        try:
            dst = ctx.alloc(dh * dw * cn * item)
            ctx.imresize(src.ptr, w * cn, h, w, cn, sy, sx, dst.ptr, dw * cn * item, dh, dw, antialias=bool(antialiasing),
                         out_type=out_type)
            return ctx.download(dst.ptr, out_shape, np.dtype(dtype).type)
        finally:
            src.free()
            if dst is not None:
                dst.free()

    def imresize_device(self, d_src: int, shape, d_dst: int, scale: Optional[float] = None,
                        output_shape: Optional[Tuple[int, int]] = None, antialiasing: bool = True, dtype=np.uint8,
                        src_stride: Optional[int] = None, dst_stride: Optional[int] = None) -> Tuple[int, ...]:
        """imresize on a u8 image that already lives in HBM, into d_dst (device addresses; dense unless the strides, in
        bytes, are given).  -> the output's shape.  Synchronous."""
        args = self._imresize_args(shape, scale, output_shape, antialiasing, dtype)
        h, w, cn, sy, sx, dh, dw, out_type, item, out_shape = args
        if not d_src or not d_dst:
            raise ValueError("imresize: null device pointer")
        ss = w * cn if src_stride is None else int(src_stride)
        ds = dw * cn * item if dst_stride is None else int(dst_stride)
        if ss < w * cn or ds < dw * cn * item:
            raise ValueError("imresize: a stride is shorter than a row")
        self._ctx().imresize(int(d_src), ss, h, w, cn, sy, sx, int(d_dst), ds, dh, dw, antialias=bool(antialiasing),
                             out_type=out_type)
        return out_shape

    def evaluate_sr_network(self, net, hr: np.ndarray, crop_border: Optional[int] = None, ensemble: int = 1, y_round: bool = False,
                            return_sr: bool = False) -> Dict[str, Any]:
        """The ground-truth benchmark of an SR network (sr_network.py) on one image, the protocol of the SR papers: the u8 RGB
        image `hr` is mod-cropped to net.scale, brought down by imresize(1 / net.scale) (MATLAB's bicubic), run through the
        network and compared with the cropped HR by the SR-benchmark PSNR / SSIM on Y (y_round: MATLAB's rounded u8 luma) and
        on RGB, a border of crop_border (default net.scale) pixels cropped.  Everything stays in HBM; only the numbers come
        down, and with return_sr the SR image ('sr').  -> {'psnr_y', 'ssim_y', 'psnr_rgb', 'ssim_rgb', 'crop_border',
        'scale', 'hr_shape', 'lr_shape'}."""
        from sr_network import ensemble_mask
        ensemble_mask(ensemble)
        img = self._require_u8(np.asarray(hr), "evaluate_sr_network")
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"evaluate_sr_network: need an H x W x 3 RGB image, got shape {img.shape}")
        s = int(net.scale)
        cb = s if crop_border is None else _native._whole(crop_border, "crop_border")
        H, W = img.shape[0] - img.shape[0] % s, img.shape[1] - img.shape[1] % s
        if H < s or W < s:
            raise ValueError(f"evaluate_sr_network: the image {img.shape[:2]} is smaller than the scale {s}")
        lr_args = self._imresize_args((H, W, 3), 1.0 / s, None, True, np.uint8)
        lh, lw = lr_args[5], lr_args[6]
        if (lh * s, lw * s) != (H, W):
            raise ValueError(f"evaluate_sr_network: ceil({H, W} / {s}) gave {lh, lw}")
        y_args = self._sr_benchmark_args((H, W, 3), (H, W, 3), cb, True, bool(y_round), 255.0)
        rgb_args = self._sr_benchmark_args((H, W, 3), (H, W, 3), cb, False, False, 255.0)
        ctx = self._ctx()
        full_stride = img.shape[1] * 3                                  # the mod-crop is a view: the same address, the full stride
        d_hr, d_lr, d_sr = _DevImage(ctx, img), None, None
        try:
            d_lr, d_sr = ctx.alloc(lh * lw * 3), ctx.alloc(H * W * 3)
            ctx.imresize(d_hr.ptr, full_stride, H, W, 3, 1.0 / s, 1.0 / s, d_lr.ptr, lw * 3, lh, lw)
            net.upscale_device(d_lr.ptr, (lh, lw, 3), d_sr.ptr, W * 3, ctx=ctx, ensemble=ensemble)
            out = {}
            for key, a in (("y", y_args), ("rgb", rgb_args)):
                sums = ctx.bench_u8(d_sr.ptr, W * 3, d_hr.ptr, full_stride, H, W, 3, crop_border=cb, mode=a[4], data_range=255.0)
                out["psnr_" + key], out["ssim_" + key] = _native.bench_values(sums, 255.0)
            out.update(crop_border=cb, scale=s, hr_shape=(H, W, 3), lr_shape=(lh, lw, 3))
            if return_sr:
                out["sr"] = ctx.download(d_sr.ptr, (H, W, 3), np.uint8)
            return out
        finally:
            ctx.sync()
            for b in (d_hr, d_lr, d_sr):
                if b is not None:
                    b.free()

    # -- device-level metrics ---------------------------------------------------------------------------
    def _psnr_dev(self, a: _DevImage, b: _DevImage, data_range: float) -> float:
        h, w = min(a.h, b.h), min(a.w, b.w)
        rowlen = w * a.cn
        sse = a.ctx.sse_u8(a.ptr, a.stride, b.ptr, b.stride, h, rowlen)
        return _native.psnr_from_sse(sse, h * rowlen, data_range)

    def _ssim_dev(self, a: _DevImage, b: _DevImage, multiscale: bool, data_range: float) -> float:
        h, w = min(a.h, b.h), min(a.w, b.w)
        mode = "simple" if self.ssim_branch == 'B' else ("gauss" if multiscale else "uniform")
        s, n = a.ctx.ssim_u8(a.ptr, a.stride, b.ptr, b.stride, h, w, a.cn, mode, self.gray_shift, data_range)
        return s / n

    # -- public metrics (quality_assessment_module.py:277-417) -----------------------------------------------
    def _pair(self, img1, img2, what: str, preprocessed: bool = False):
        # preprocessed: the caller has run _preprocess_image already (a second pass would scan both images for their
        # maximum again -- hundreds of milliseconds of host time at 200 MP)
        a = self._require_u8(img1 if preprocessed else self._preprocess_image(img1), what)
        b = self._require_u8(img2 if preprocessed else self._preprocess_image(img2), what)
        if a.ndim != b.ndim or (a.ndim == 3 and a.shape[2] != b.shape[2]):
            raise ValueError(f"{what}: images have different channel layouts {a.shape} vs {b.shape}")
        return a, b

    def calculate_psnr(self, img1: np.ndarray, img2: np.ndarray, data_range: float = 255.0) -> float:
        p1, p2 = self._preprocess_image(img1), self._preprocess_image(img2)
        if p1.dtype != np.uint8 or p2.dtype != np.uint8:
            # float images with max > 1 stay float in the reference: skimage promotes to >= fp32 and averages in fp64
            a32, b32 = self._crop_pair(np.asarray(p1), np.asarray(p2))
            a32 = np.ascontiguousarray(a32, dtype=np.float32)
            b32 = np.ascontiguousarray(b32, dtype=np.float32)
            ctx = self._ctx()
            da, db = ctx.upload(a32), ctx.upload(b32)
            try:
                rowlen = a32.size // a32.shape[0]
                sse = ctx.sse_f32(da.ptr, rowlen * 4, db.ptr, rowlen * 4, a32.shape[0], rowlen)
            finally:
                da.free(); db.free()
            mse = sse / a32.size
            return float("inf") if mse == 0 else float(10 * np.log10((data_range ** 2) / mse))
        a, b = self._pair(p1, p2, "calculate_psnr", preprocessed=True)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return float(self._psnr_dev(da, db, data_range))
        finally:
            da.free(); db.free()

    def _ssim_float(self, p1: np.ndarray, p2: np.ndarray, multiscale: bool, data_range: float) -> float:
        """Images that stay non-u8 after _preprocess_image (float arrays with max > 1, wider integers): the reference hands
        them on as they are -- a float32 RGB pair through cv2's float RGB2GRAY, a 2-D pair straight to skimage, which
        computes in float64 (quality_assessment_module.py:351-417).  Runs on sr_ssim_float; float64 RGB raises like
        cv2.cvtColor does."""
        a, b = self._crop_pair(np.asarray(p1), np.asarray(p2))
        if a.ndim != b.ndim or (a.ndim == 3 and a.shape[2] != b.shape[2]):
            raise ValueError(f"calculate_ssim: images have different channel layouts {a.shape} vs {b.shape}")
        if a.ndim == 3:
            if a.shape[2] != 3:
                raise ValueError("calculate_ssim: colour images must have 3 channels (cv2.COLOR_RGB2GRAY)")
            if a.dtype not in (np.uint8, np.float32) or b.dtype not in (np.uint8, np.float32):
                raise ValueError("calculate_ssim: cv2.cvtColor(RGB2GRAY) supports 8-bit, 16-bit and float32 images only "
                                 f"(got {a.dtype} / {b.dtype}); 16-bit RGB is not on the HIP path")
            if a.dtype != b.dtype:
                # cv2.cvtColor grays each image in its OWN dtype (quality_assessment_module.py:359-360): the uint8 partner gets
                # the rounded fixed-point gray, the float32 one the float formula -- two gray planes up to 0.5 level apart.
                # sr_ssim_float grays both with the float formula, so the mixed pair is refused rather than answered differently.
                raise NotImplementedError("calculate_ssim: one RGB image is uint8 and the other float32 after preprocessing; "
                                          "the HIP path takes RGB pairs of one dtype (convert one of them)")
            dt, code = np.float32, _native.SR_F32
        else:
            dt, code = (np.float32, _native.SR_F32) if (a.dtype == np.float32 and b.dtype == np.float32) else (np.float64, _native.SR_F64)
        a = np.ascontiguousarray(a, dtype=dt)
        b = np.ascontiguousarray(b, dtype=dt)
        h, w = a.shape[:2]
        cn = 3 if a.ndim == 3 else 1
        mode = "simple" if self.ssim_branch == 'B' else ("gauss" if multiscale else "uniform")
        ctx = self._ctx()
        da, db = ctx.upload(a), ctx.upload(b)
        try:
            es = a.dtype.itemsize
            s, n = ctx.ssim_float(da.ptr, w * cn * es, db.ptr, w * cn * es, h, w, cn, code, mode, data_range)
            return float(s / n)
        finally:
            da.free(); db.free()

    def calculate_ssim(self, img1: np.ndarray, img2: np.ndarray, multiscale: bool = True,
                       data_range: float = 255.0) -> float:
        p1, p2 = self._preprocess_image(img1), self._preprocess_image(img2)
        if np.asarray(p1).dtype != np.uint8 or np.asarray(p2).dtype != np.uint8:
            return self._ssim_float(p1, p2, multiscale, data_range)
        a, b = self._pair(p1, p2, "calculate_ssim", preprocessed=True)
        if a.ndim == 3 and a.shape[2] != 3:
            raise ValueError("calculate_ssim: colour images must have 3 channels (cv2.COLOR_RGB2GRAY)")
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return float(self._ssim_dev(da, db, multiscale, data_range))
        finally:
            da.free(); db.free()

    # -- multi-scale SSIM (no reference counterpart: the reference's 'ms_ssim' key is its single-scale Gaussian SSIM) ----------
    @staticmethod
    def _ms_ssim_args(h: int, w: int, cn: int, data_range: float, levels: int, weights):
        """Every refusal of the MS-SSIM methods, on the host: ValueError (SrShapeError for an image too small for `levels`)."""
        if cn not in (1, 3):
            raise ValueError("calculate_ms_ssim: colour images must have 3 channels (cv2.COLOR_RGB2GRAY)")
        if not (np.isfinite(data_range) and data_range > 0):
            raise ValueError(f"calculate_ms_ssim: data_range must be finite and positive, got {data_range!r}")
        plan = _native.ms_ssim_plan(h, w, levels)                       # levels outside 1..5, sides below 11 * 2^(levels-1)
        wt = _native.MS_SSIM_WEIGHTS[:int(levels)] if weights is None else tuple(float(v) for v in weights)
        if len(wt) != int(levels):
            raise ValueError(f"calculate_ms_ssim: {int(levels)} levels need {int(levels)} weights, got {len(wt)}")
        if not all(np.isfinite(wt)):
            raise ValueError("calculate_ms_ssim: weights must be finite")
        return plan, wt

    def _ms_ssim_dev(self, a: _DevImage, b: _DevImage, data_range: float, levels: int, wt, return_levels: bool):
        h, w = min(a.h, b.h), min(a.w, b.w)
        recs = a.ctx.ms_ssim_u8(a.ptr, a.stride, b.ptr, b.stride, h, w, a.cn, levels=int(levels), gray_shift=self.gray_shift,
                                data_range=float(data_range))
        v = _native.ms_ssim_value(recs, wt)
        if not return_levels:
            return v
        return v, {"s": [r[0] / r[2] for r in recs], "cs": [r[1] / r[2] for r in recs], "weights": list(wt)}

    def calculate_ms_ssim(self, img1: np.ndarray, img2: np.ndarray, data_range: float = 255.0, levels: int = 5, weights=None,
                          return_levels: bool = False):
        """Wang / Simoncelli / Bovik multi-scale SSIM of the common top-left rectangle of two u8 images (the preprocessing,
        u8 requirement and channel-layout check of calculate_ssim), as include/sr_hip.h defines it: exact 2 x 2 mean pooling
        (a last odd row or column dropped), Gaussian-11 SSIM over the valid region per level, the weighted product of the
        first levels' cs means and the last level's SSIM mean (weights: `levels` numbers, default Wang's).  Both sides must
        be at least 11 * 2^(levels - 1) (176 for 5 levels): a smaller image is a ValueError, the level count is never
        reduced.  return_levels: also {'s': [S_j], 'cs': [CS_j], 'weights': [...]}.  This is NOT the 'ms_ssim' key of
        evaluate_full_reference, which keeps the reference's single-scale value."""
        a, b = self._pair(img1, img2, "calculate_ms_ssim")
        cn = a.shape[2] if a.ndim == 3 else 1
        _, wt = self._ms_ssim_args(min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1]), cn, data_range, levels, weights)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._ms_ssim_dev(da, db, data_range, levels, wt, return_levels)
        finally:
            da.free(); db.free()

    def calculate_ms_ssim_device(self, d_img1: int, shape1, d_img2: int, shape2, data_range: float = 255.0, levels: int = 5,
                                 weights=None, return_levels: bool = False):
        """calculate_ms_ssim on two dense u8 images that already live in HBM (device addresses + shapes)."""
        shape1, shape2 = tuple(int(v) for v in shape1), tuple(int(v) for v in shape2)
        if len(shape1) not in (2, 3) or len(shape1) != len(shape2) or (len(shape1) == 3 and shape1[2] != shape2[2]):
            raise ValueError(f"calculate_ms_ssim: images have different channel layouts {shape1} vs {shape2}")
        if not d_img1 or not d_img2:
            raise ValueError("calculate_ms_ssim: null device pointer")
        cn = shape1[2] if len(shape1) == 3 else 1
        _, wt = self._ms_ssim_args(min(shape1[0], shape2[0]), min(shape1[1], shape2[1]), cn, data_range, levels, weights)
        ctx = self._ctx()
        return self._ms_ssim_dev(_DevImage(ctx, shape=shape1, ptr=d_img1), _DevImage(ctx, shape=shape2, ptr=d_img2), data_range,
                                 levels, wt, return_levels)

    # -- SR-benchmark PSNR / SSIM (no reference counterpart: BasicSR's calculate_psnr / calculate_ssim convention) -----------
    @staticmethod
    def _sr_benchmark_args(shape1, shape2, crop_border, test_y_channel: bool, y_round: bool, data_range: float):
        """Every refusal of the SR-benchmark methods, on the host: ValueError (SrShapeError for a crop that leaves a side
        below 11).  -> (h, w, cn, crop_border, mode, channel)."""
        shape1, shape2 = tuple(int(v) for v in shape1), tuple(int(v) for v in shape2)
        if shape1 != shape2:
            raise ValueError(f"evaluate_sr_benchmark: images must have the same shape, got {shape1} vs {shape2} "
                             "(nothing is cropped to a common rectangle)")
        if len(shape1) not in (2, 3):
            raise ValueError(f"evaluate_sr_benchmark: need an H x W or H x W x C image, got shape {shape1}")
        cn = shape1[2] if len(shape1) == 3 else 1
        if cn not in (1, 3):
            raise ValueError("evaluate_sr_benchmark: colour images must have 3 channels (RGB)")
        if test_y_channel and cn != 3:
            raise ValueError("evaluate_sr_benchmark: test_y_channel needs a 3-channel RGB image")
        if y_round and not test_y_channel:
            raise ValueError("evaluate_sr_benchmark: y_round applies to the Y channel only (test_y_channel=True)")
        if not (np.isfinite(data_range) and data_range > 0):
            raise ValueError(f"evaluate_sr_benchmark: data_range must be finite and positive, got {data_range!r}")
        mode = (_native.BENCH_Y_ROUND if y_round else _native.BENCH_Y) if test_y_channel else _native.BENCH_CHANNELS
        channel = ("y_round" if y_round else "y") if test_y_channel else ("rgb" if cn == 3 else "gray")
        _native.bench_plan(shape1[0], shape1[1], cn, crop_border, mode)          # crop_border < 0, a too-small crop
        return shape1[0], shape1[1], cn, int(crop_border), mode, channel

    @staticmethod
    def _sr_benchmark_dev(ctx, d1: int, d2: int, args, data_range: float) -> Dict[str, Any]:
        h, w, cn, cb, mode, channel = args
        sums = ctx.bench_u8(d1, w * cn, d2, w * cn, h, w, cn, crop_border=cb, mode=mode, data_range=float(data_range))
        psnr, ssim = _native.bench_values(sums, data_range)
        return {"psnr": psnr, "ssim": ssim, "crop_border": cb, "channel": channel}

    def evaluate_sr_benchmark(self, img1: np.ndarray, img2: np.ndarray, crop_border: int = 0, test_y_channel: bool = True,
                              y_round: bool = False, data_range: float = 255.0) -> Dict[str, Any]:
        """The PSNR and SSIM the SR papers and model cards quote (BasicSR's calculate_psnr / calculate_ssim with crop_border
        and test_y_channel), as include/sr_hip.h defines them: both u8 images cropped by crop_border on every side, then on
        the BT.601 luma Y carried exactly (test_y_channel; y_round: MATLAB's rounded u8 luma instead) or on the channels as
        they are; Gaussian-11 SSIM over the valid region, the mean over all planes.  -> {'psnr', 'ssim', 'crop_border',
        'channel'} with channel in 'y', 'y_round', 'rgb', 'gray'.  u8 images of equal shape only: another shape is a
        ValueError (nothing is cropped to a common rectangle), as is a crop that leaves a side below 11."""
        a = self._require_u8(np.asarray(img1), "evaluate_sr_benchmark")
        b = self._require_u8(np.asarray(img2), "evaluate_sr_benchmark")
        args = self._sr_benchmark_args(a.shape, b.shape, crop_border, test_y_channel, y_round, data_range)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._sr_benchmark_dev(ctx, da.ptr, db.ptr, args, data_range)
        finally:
            da.free(); db.free()

    def evaluate_sr_benchmark_device(self, d_img1: int, shape1, d_img2: int, shape2, crop_border: int = 0,
                                     test_y_channel: bool = True, y_round: bool = False, data_range: float = 255.0) -> Dict[str, Any]:
        """evaluate_sr_benchmark on two dense u8 images that already live in HBM (device addresses + shapes)."""
        args = self._sr_benchmark_args(shape1, shape2, crop_border, test_y_channel, y_round, data_range)
        if not d_img1 or not d_img2:
            raise ValueError("evaluate_sr_benchmark: null device pointer")
        return self._sr_benchmark_dev(self._ctx(), int(d_img1), int(d_img2), args, data_range)

    # -- VIF and GMSD (no reference counterpart: MATLAB's vifp_mscale.m and the authors' GMSD.m) ------------------------------
    @staticmethod
    def _plane_metric_args(what: str, plan, shape1, shape2, crop_border, test_y_channel: bool, y_round: bool, stride1, stride2):
        """Every refusal of the VIF / GMSD methods, on the host: ValueError (SrShapeError for a crop that leaves a side too
        small or a short stride).  Gray input uses the plane as it is.  -> (h, w, cn, crop_border, mode, stride1, stride2)."""
        shape1, shape2 = tuple(int(v) for v in shape1), tuple(int(v) for v in shape2)
        if shape1 != shape2:
            raise ValueError(f"{what}: images must have the same shape, got {shape1} vs {shape2} "
                             "(nothing is cropped to a common rectangle)")
        if len(shape1) not in (2, 3):
            raise ValueError(f"{what}: need an H x W or H x W x C image, got shape {shape1}")
        cn = shape1[2] if len(shape1) == 3 else 1
        if cn not in (1, 3):
            raise ValueError(f"{what}: colour images must have 3 channels (RGB)")
        if cn == 3 and not test_y_channel:
            raise ValueError(f"{what}: a colour image is compared on its luma only (test_y_channel=True)")
        if y_round and cn != 3:
            raise ValueError(f"{what}: y_round applies to the luma of an RGB image only")
        mode = _native.BENCH_CHANNELS if cn == 1 else (_native.BENCH_Y_ROUND if y_round else _native.BENCH_Y)
        plan(shape1[0], shape1[1], cn, crop_border, mode)                        # crop_border < 0, a too-small crop
        row = shape1[1] * cn
        s1, s2 = (row if s is None else int(s) for s in (stride1, stride2))
        if s1 < row or s2 < row:
            raise _native.SrShapeError(f"{what}: stride smaller than a row")
        return shape1[0], shape1[1], cn, int(crop_border), mode, s1, s2

    @staticmethod
    def _vif_dev(ctx, d_ref: int, d_dist: int, args, return_scales: bool):
        h, w, cn, cb, mode, s1, s2 = args
        scales = ctx.vif_u8(d_ref, s1, d_dist, s2, h, w, cn, crop_border=cb, mode=mode)
        v = _native.vif_value(scales)
        return (v, scales) if return_scales else v

    def calculate_vif(self, reference: np.ndarray, distorted: np.ndarray, crop_border: int = 0, test_y_channel: bool = True,
                      y_round: bool = False, return_scales: bool = False):
        """VIF in the pixel domain over four scales (MATLAB's vifp_mscale, "VIFp"), as include/sr_hip.h defines it: both u8
        images cropped by crop_border on every side, then on the BT.601 luma carried exactly (y_round: MATLAB's rounded u8
        luma instead); a gray image is used as it is.  NOT symmetric: `reference` is the reference.  1 for identical images up
        to 1e-11, NaN for a flat reference.  return_scales: (value, [(num_s, den_s, count)] of the four scales).  u8 images of
        equal shape only: another shape is a ValueError (nothing is cropped to a common rectangle), as is a crop that leaves
        a side below 41."""
        a = self._require_u8(np.asarray(reference), "calculate_vif")
        b = self._require_u8(np.asarray(distorted), "calculate_vif")
        args = self._plane_metric_args("calculate_vif", _native.vif_plan, a.shape, b.shape, crop_border, test_y_channel, y_round,
                                       None, None)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._vif_dev(ctx, da.ptr, db.ptr, args, return_scales)
        finally:
            da.free(); db.free()

    def calculate_vif_device(self, d_reference: int, shape1, d_distorted: int, shape2, crop_border: int = 0,
                             test_y_channel: bool = True, y_round: bool = False, return_scales: bool = False,
                             stride1: Optional[int] = None, stride2: Optional[int] = None):
        """calculate_vif on two u8 images that already live in HBM (device addresses + shapes; strides in bytes, dense when
        None)."""
        args = self._plane_metric_args("calculate_vif", _native.vif_plan, shape1, shape2, crop_border, test_y_channel, y_round,
                                       stride1, stride2)
        if not d_reference or not d_distorted:
            raise ValueError("calculate_vif: null device pointer")
        return self._vif_dev(self._ctx(), int(d_reference), int(d_distorted), args, return_scales)

    @staticmethod
    def _gmsd_dev(ctx, d1: int, d2: int, args) -> float:
        h, w, cn, cb, mode, s1, s2 = args
        return _native.gmsd_value(ctx.gmsd_u8(d1, s1, d2, s2, h, w, cn, crop_border=cb, mode=mode))

    def calculate_gmsd(self, img1: np.ndarray, img2: np.ndarray, crop_border: int = 0, test_y_channel: bool = True,
                       y_round: bool = False) -> float:
        """The gradient magnitude similarity deviation (the authors' GMSD.m), as include/sr_hip.h defines it: planes as
        calculate_vif, the 2 x 2 mean and every second sample, Prewitt gradient magnitudes, and the standard deviation (N - 1
        divisor) of the similarity map.  0 for identical images, larger is worse.  u8 images of equal shape only; a crop that
        leaves a side below 4 is a ValueError."""
        a = self._require_u8(np.asarray(img1), "calculate_gmsd")
        b = self._require_u8(np.asarray(img2), "calculate_gmsd")
        args = self._plane_metric_args("calculate_gmsd", _native.gmsd_plan, a.shape, b.shape, crop_border, test_y_channel, y_round,
                                       None, None)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._gmsd_dev(ctx, da.ptr, db.ptr, args)
        finally:
            da.free(); db.free()

    def calculate_gmsd_device(self, d_img1: int, shape1, d_img2: int, shape2, crop_border: int = 0, test_y_channel: bool = True,
                              y_round: bool = False, stride1: Optional[int] = None, stride2: Optional[int] = None) -> float:
        """calculate_gmsd on two u8 images that already live in HBM (device addresses + shapes; strides in bytes, dense when
        None)."""
        args = self._plane_metric_args("calculate_gmsd", _native.gmsd_plan, shape1, shape2, crop_border, test_y_channel, y_round,
                                       stride1, stride2)
        if not d_img1 or not d_img2:
            raise ValueError("calculate_gmsd: null device pointer")
        return self._gmsd_dev(self._ctx(), int(d_img1), int(d_img2), args)

    # -- FSIM / FSIMc (no reference counterpart: the authors' FeatureSIM.m) ---------------------------------------------------
    @staticmethod
    def _fsim_args(shape1, shape2, stride1, stride2) -> Tuple[int, int, int, int, int]:
        """Every refusal of the FSIM methods, on the host: ValueError (SrShapeError for a side below 16 or a short stride),
        SrNativeError for a pooled side above 2048.  -> (h, w, cn, stride1, stride2)."""
        shape1, shape2 = tuple(int(v) for v in shape1), tuple(int(v) for v in shape2)
        if shape1 != shape2:
            raise ValueError(f"calculate_fsim: images must have the same shape, got {shape1} vs {shape2} "
                             "(nothing is cropped to a common rectangle)")
        if len(shape1) not in (2, 3):
            raise ValueError(f"calculate_fsim: need an H x W or H x W x C image, got shape {shape1}")
        cn = shape1[2] if len(shape1) == 3 else 1
        _native.fsim_plan(shape1[0], shape1[1], cn)
        row = shape1[1] * cn
        s1, s2 = (row if s is None else int(s) for s in (stride1, stride2))
        if s1 < row or s2 < row:
            raise _native.SrShapeError("calculate_fsim: stride smaller than a row")
        return shape1[0], shape1[1], cn, s1, s2

    @staticmethod
    def _fsim_dev(ctx, d1: int, d2: int, args, return_parts: bool) -> Dict[str, Any]:
        h, w, cn, s1, s2 = args
        parts = ctx.fsim_u8(d1, s1, d2, s2, h, w, cn)
        v, vc = _native.fsim_value(parts)
        out = {'fsim': v, 'fsimc': vc}
        if return_parts:
            out['parts'] = parts
        return out

    def calculate_fsim(self, img1: np.ndarray, img2: np.ndarray, return_parts: bool = False) -> Dict[str, Any]:
        """FSIM and FSIMc (Zhang et al. 2011, the authors' FeatureSIM.m), as include/sr_hip.h defines them -> {'fsim',
        'fsimc'}: u8 images of equal shape with 1, 3 (RGB) or 4 channels (alpha ignored), both sides at least 16; a gray
        pair has fsimc == fsim.  Symmetric; 1 for identical images, NaN for a flat pair.  return_parts adds 'parts', the
        record of the three sums with F and the pooled size."""
        a = self._require_u8(np.asarray(img1), "calculate_fsim")
        b = self._require_u8(np.asarray(img2), "calculate_fsim")
        args = self._fsim_args(a.shape, b.shape, None, None)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._fsim_dev(ctx, da.ptr, db.ptr, args, return_parts)
        finally:
            da.free(); db.free()

    def calculate_fsim_device(self, d_img1: int, shape1, d_img2: int, shape2, return_parts: bool = False,
                              stride1: Optional[int] = None, stride2: Optional[int] = None) -> Dict[str, Any]:
        """calculate_fsim on two u8 images that already live in HBM (device addresses + shapes; strides in bytes, dense when
        None)."""
        args = self._fsim_args(shape1, shape2, stride1, stride2)
        if not d_img1 or not d_img2:
            raise ValueError("calculate_fsim: null device pointer")
        return self._fsim_dev(self._ctx(), int(d_img1), int(d_img2), args, return_parts)

    # -- VSI (no reference counterpart: the authors' VSI.m with SDSP.m) ---------------------------------------------------------
    @staticmethod
    def _vsi_args(shape1, shape2, stride1, stride2) -> Tuple[int, int, int, int, int]:
        """Every refusal of the VSI methods, on the host: ValueError (SrShapeError for a side below 16 or a short stride),
        SrNativeError for a gray image or F above 256.  -> (h, w, cn, stride1, stride2)."""
        shape1, shape2 = tuple(int(v) for v in shape1), tuple(int(v) for v in shape2)
        if shape1 != shape2:
            raise ValueError(f"calculate_vsi: images must have the same shape, got {shape1} vs {shape2} "
                             "(nothing is cropped to a common rectangle)")
        if len(shape1) not in (2, 3):
            raise ValueError(f"calculate_vsi: need an H x W x C image, got shape {shape1}")
        cn = shape1[2] if len(shape1) == 3 else 1
        _native.vsi_plan(shape1[0], shape1[1], cn)
        row = shape1[1] * cn
        s1, s2 = (row if s is None else int(s) for s in (stride1, stride2))
        if s1 < row or s2 < row:
            raise _native.SrShapeError("calculate_vsi: stride smaller than a row")
        return shape1[0], shape1[1], cn, s1, s2

    @staticmethod
    def _vsi_dev(ctx, d1: int, d2: int, args, return_parts: bool) -> Dict[str, Any]:
        h, w, cn, s1, s2 = args
        parts = ctx.vsi(d1, s1, d2, s2, h, w, cn)
        out = {'vsi': _native.vsi_value(parts)}
        if return_parts:
            out['parts'] = parts
        return out

    def calculate_vsi(self, img1: np.ndarray, img2: np.ndarray, return_parts: bool = False) -> Dict[str, Any]:
        """VSI (Zhang, Shen and Li 2014, the authors' VSI.m with SDSP saliency), as include/sr_hip.h defines it -> {'vsi'}: u8
        images of equal shape with 3 (RGB) or 4 channels (alpha ignored), both sides at least 16.  Symmetric; 1 for
        identical images, NaN for a pair with a flat a or b plane.  return_parts adds 'parts', the record of the two sums
        with F, the pooled size and the ranges of a, b and the saliency map."""
        a = self._require_u8(np.asarray(img1), "calculate_vsi")
        b = self._require_u8(np.asarray(img2), "calculate_vsi")
        args = self._vsi_args(a.shape, b.shape, None, None)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._vsi_dev(ctx, da.ptr, db.ptr, args, return_parts)
        finally:
            da.free(); db.free()

    def calculate_vsi_device(self, d_img1: int, shape1, d_img2: int, shape2, return_parts: bool = False,
                             stride1: Optional[int] = None, stride2: Optional[int] = None) -> Dict[str, Any]:
        """calculate_vsi on two u8 images that already live in HBM (device addresses + shapes; strides in bytes, dense when
        None)."""
        args = self._vsi_args(shape1, shape2, stride1, stride2)
        if not d_img1 or not d_img2:
            raise ValueError("calculate_vsi: null device pointer")
        return self._vsi_dev(self._ctx(), int(d_img1), int(d_img2), args, return_parts)

    # -- colour difference (no reference counterpart: scikit-image's rgb2lab and deltaE_ciede2000 / deltaE_cie76) ------------
    @staticmethod
    def _delta_e_args(what: str, shape1, shape2, crop_border, formula, stride1, stride2):
        """Every refusal of the colour-difference methods, on the host: ValueError (SrShapeError for a crop that leaves
        nothing or a short stride).  -> (h, w, cn, crop_border, formula, stride1, stride2, plan)."""
        shape1, shape2 = tuple(int(v) for v in shape1), tuple(int(v) for v in shape2)
        if shape1 != shape2:
            raise ValueError(f"{what}: images must have the same shape, got {shape1} vs {shape2} "
                             "(nothing is cropped to a common rectangle)")
        if len(shape1) not in (2, 3):
            raise ValueError(f"{what}: need an H x W or H x W x C image, got shape {shape1}")
        cn = shape1[2] if len(shape1) == 3 else 1
        if cn not in (1, 3, 4):
            raise ValueError(f"{what}: need a gray, RGB or RGBA image (1, 3 or 4 channels), got {cn}")
        f = _native.delta_e_formula(formula)
        if f not in (_native.DELTA_E_2000, _native.DELTA_E_76):
            raise ValueError(f"{what}: unknown formula {formula!r}")
        plan = _native.delta_e_plan(shape1[0], shape1[1], cn, crop_border, f)    # crop_border < 0, a crop that leaves nothing
        row = shape1[1] * cn
        s1, s2 = (row if s is None else int(s) for s in (stride1, stride2))
        if s1 < row or s2 < row:
            raise _native.SrShapeError(f"{what}: stride smaller than a row")
        return shape1[0], shape1[1], cn, int(crop_border), f, s1, s2, plan

    @staticmethod
    def _delta_e_percentiles(what: str, percentiles) -> Tuple[float, ...]:
        ps = tuple(float(p) for p in percentiles)
        for p in ps:
            if not (0.0 < p <= 100.0):
                raise ValueError(f"{what}: percentiles must lie in (0, 100], got {p!r}")
        return ps

    def _delta_e_dev(self, ctx, d1: int, d2: int, args, percentiles, return_map: bool) -> Dict[str, Any]:
        h, w, cn, cb, f, s1, s2, plan = args
        ch, cw = plan["size"]
        dmap = ctx.alloc(ch * cw * 8) if return_map else None
        try:
            rec = ctx.delta_e_u8(d1, s1, d2, s2, h, w, cn, crop_border=cb, formula=f, d_map=dmap.ptr if dmap else 0,
                                 map_stride=cw * 8 if dmap else 0)
            mean, rms = _native.delta_e_mean_rms(rec)
            out = {'mean': mean, 'rms': rms, 'max': float(rec['max'])}
            for p in percentiles:
                out[f'p{p:g}'] = _native.delta_e_percentile(rec, p)
            for t in (1, 3, 5):
                out[f'frac_above_{t}'] = _native.delta_e_fraction(rec, float(t))
            out.update(level=self._assess_delta_e(mean), formula='ciede2000' if f == _native.DELTA_E_2000 else 'cie76',
                       count=int(rec['count']))
            if dmap:
                out['map'] = ctx.download(dmap.ptr, (ch, cw), np.float64)
            return out
        finally:
            if dmap:
                dmap.free()

    def calculate_delta_e(self, img1: np.ndarray, img2: np.ndarray, formula: str = 'ciede2000', crop_border: int = 0,
                          percentiles=(50, 95, 99), return_map: bool = False) -> Dict[str, Any]:
        """The full-reference, per-pixel colour difference of two u8 images of equal shape (gray, RGB or RGBA with alpha
        ignored), as include/sr_hip.h defines it: scikit-image's rgb2lab (sRGB, D65 / 2 degrees) and deltaE_ciede2000
        ('ciede2000', kL = kC = kH = 1) or deltaE_cie76 ('cie76'), in float64, over the image cropped by crop_border.
        Returns mean, rms, max, p<p> for every p of `percentiles` (the lower edge of the 1/16-wide histogram bin that holds
        it), frac_above_1 / _3 / _5 (the exact fractions of pixels with dE >= 1, 3, 5), level (the thresholds of
        QualityThresholds.DELTA_E_* on the mean), formula and count; with return_map also 'map', the float64 dE of every
        cropped pixel.  0 everywhere for identical images.  NOT the private _calculate_delta_e / brand_color_delta_e_i of the
        commercial metrics: those compare a region MEAN in OpenCV's 8-bit integer Lab with one brand colour, by CIE76.  A shape
        mismatch is a ValueError (nothing is cropped to a common rectangle)."""
        a = self._require_u8(np.asarray(img1), "calculate_delta_e")
        b = self._require_u8(np.asarray(img2), "calculate_delta_e")
        ps = self._delta_e_percentiles("calculate_delta_e", percentiles)
        args = self._delta_e_args("calculate_delta_e", a.shape, b.shape, crop_border, formula, None, None)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._delta_e_dev(ctx, da.ptr, db.ptr, args, ps, return_map)
        finally:
            da.free(); db.free()

    def calculate_delta_e_device(self, d_img1: int, shape1, d_img2: int, shape2, formula: str = 'ciede2000', crop_border: int = 0,
                                 percentiles=(50, 95, 99), return_map: bool = False, stride1: Optional[int] = None,
                                 stride2: Optional[int] = None) -> Dict[str, Any]:
        """calculate_delta_e on two u8 images that already live in HBM (device addresses + shapes; strides in bytes, dense when
        None)."""
        ps = self._delta_e_percentiles("calculate_delta_e", percentiles)
        args = self._delta_e_args("calculate_delta_e", shape1, shape2, crop_border, formula, stride1, stride2)
        if not d_img1 or not d_img2:
            raise ValueError("calculate_delta_e: null device pointer")
        return self._delta_e_dev(self._ctx(), int(d_img1), int(d_img2), args, ps, return_map)

    def _delta_e_map_dev(self, ctx, d1: int, d2: int, args, xe: List[int], ye: List[int]) -> Dict[str, Any]:
        h, w, cn, cb, f, s1, s2, _ = args
        r = ctx.delta_e_cells_u8(d1, s1, d2, s2, h, w, cn, xe, ye, crop_border=cb, formula=f)
        area = np.outer(np.diff(ye), np.diff(xe)).astype(np.float64)
        return {"mean": r["sum"] / area, "max": r["max"], "x_edges": list(xe), "y_edges": list(ye)}

    def evaluate_delta_e_map(self, img1: np.ndarray, img2: np.ndarray, cell: Optional[int] = None, x_edges=None, y_edges=None,
                             formula: str = 'ciede2000') -> Dict[str, Any]:
        """Where the colour drifted: the mean and the largest colour difference (calculate_delta_e's, no crop) per cell of a
        separable grid, with the argument rules of evaluate_quality_map: uniform cells of `cell` pixels (default 256) or the
        edge lists x_edges (0 .. W) / y_edges (0 .. H).  Returns (gh, gw) arrays 'mean' and 'max' and the two edge lists.
        The difference is pointwise, so the cell means weighted by their areas give the global mean and the largest cell max
        is the global max.  Images of different shapes are a ValueError."""
        a = self._require_u8(np.asarray(img1), "evaluate_delta_e_map")
        b = self._require_u8(np.asarray(img2), "evaluate_delta_e_map")
        args = self._delta_e_args("evaluate_delta_e_map", a.shape, b.shape, 0, formula, None, None)
        xe, ye = self._map_edges(args[0], args[1], cell, x_edges, y_edges)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._delta_e_map_dev(ctx, da.ptr, db.ptr, args, xe, ye)
        finally:
            da.free(); db.free()

    def evaluate_delta_e_map_device(self, d_img1: int, shape1, d_img2: int, shape2, cell: Optional[int] = None, x_edges=None,
                                    y_edges=None, formula: str = 'ciede2000', stride1: Optional[int] = None,
                                    stride2: Optional[int] = None) -> Dict[str, Any]:
        """evaluate_delta_e_map on two u8 images that already live in HBM (device addresses + shapes; strides in bytes, dense
        when None)."""
        args = self._delta_e_args("evaluate_delta_e_map", shape1, shape2, 0, formula, stride1, stride2)
        xe, ye = self._map_edges(args[0], args[1], cell, x_edges, y_edges)
        if not d_img1 or not d_img2:
            raise ValueError("evaluate_delta_e_map: null device pointer")
        return self._delta_e_map_dev(self._ctx(), int(d_img1), int(d_img2), args, xe, ye)

    # -- HaarPSI (no reference counterpart: Reisenhofer, Bosse, Kutyniok, Wiegand 2018) ---------------------------------------
    @staticmethod
    def _haarpsi_args(what: str, shape1, shape2, crop_border, subsample, convention, stride1, stride2):
        """Every refusal of the HaarPSI methods, on the host: ValueError (SrShapeError for a crop that leaves a side below 2 or
        a short stride).  -> (h, w, cn, crop_border, subsample, convention, stride1, stride2, plan)."""
        shape1, shape2 = tuple(int(v) for v in shape1), tuple(int(v) for v in shape2)
        if shape1 != shape2:
            raise ValueError(f"{what}: images must have the same shape, got {shape1} vs {shape2} "
                             "(nothing is cropped to a common rectangle)")
        if len(shape1) not in (2, 3):
            raise ValueError(f"{what}: need an H x W or H x W x C image, got shape {shape1}")
        cn = shape1[2] if len(shape1) == 3 else 1
        if cn not in (1, 3, 4):
            raise ValueError(f"{what}: need a gray, RGB or RGBA image (1, 3 or 4 channels), got {cn}")
        conv = _native.haarpsi_convention(convention)
        if conv not in (_native.HAARPSI_MATLAB, _native.HAARPSI_PYTHON):
            raise ValueError(f"{what}: unknown convention {convention!r}")
        if not isinstance(subsample, (bool, np.bool_)):
            raise ValueError(f"{what}: subsample must be True or False, got {subsample!r}")
        plan = _native.haarpsi_plan(shape1[0], shape1[1], cn, crop_border, bool(subsample), conv)
        row = shape1[1] * cn
        s1, s2 = (row if s is None else int(s) for s in (stride1, stride2))
        if s1 < row or s2 < row:
            raise _native.SrShapeError(f"{what}: stride smaller than a row")
        return shape1[0], shape1[1], cn, int(crop_border), bool(subsample), conv, s1, s2, plan

    @staticmethod
    def _haarpsi_dev(ctx, d1: int, d2: int, args, return_parts: bool):
        h, w, cn, cb, sub, conv, s1, s2, _ = args
        rec = ctx.haarpsi(d1, s1, d2, s2, h, w, cn, crop_border=cb, subsample=sub, convention=conv)
        v = _native.haarpsi_value(rec)
        if not return_parts:
            return v
        return {"haarpsi": v, "num": rec["num"], "den": rec["den"], "channels": rec["channels"], "count": rec["count"],
                "subsample": sub, "convention": "python" if conv == _native.HAARPSI_PYTHON else "matlab"}

    def calculate_haarpsi(self, reference: np.ndarray, distorted: np.ndarray, crop_border: int = 0, subsample: bool = True,
                          convention: str = 'matlab', return_parts: bool = False):
        """HaarPSI, the Haar wavelet perceptual similarity index of two u8 images of equal shape (gray, RGB or RGBA with alpha
        ignored), as include/sr_hip.h defines it: C = 30, alpha = 4.2, three scales, over the image cropped by crop_border
        (both sides at least 2 afterwards).  Larger is better; 1 (within 1e-12) for identical images; symmetric; NaN for a
        black pair (every weight 0).  convention: 'matlab' (conv2 'same', the default) or 'python' (scipy convolve2d
        'same', whose window sits one sample earlier) -- the two official scripts differ by 1e-3 .. 1e-2 on small images.
        subsample = False skips the 2 x 2 pooling.  Returns the value, or with return_parts a dict with the value
        ('haarpsi'), the per-channel sums 'num' and 'den', 'channels', 'count', 'subsample' and 'convention'.  A shape
        mismatch is a ValueError (nothing is cropped to a common rectangle); float and 16-bit inputs are not built."""
        a = self._require_u8(np.asarray(reference), "calculate_haarpsi")
        b = self._require_u8(np.asarray(distorted), "calculate_haarpsi")
        args = self._haarpsi_args("calculate_haarpsi", a.shape, b.shape, crop_border, subsample, convention, None, None)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._haarpsi_dev(ctx, da.ptr, db.ptr, args, return_parts)
        finally:
            da.free(); db.free()

    def calculate_haarpsi_device(self, d_reference: int, shape1, d_distorted: int, shape2, crop_border: int = 0,
                                 subsample: bool = True, convention: str = 'matlab', return_parts: bool = False,
                                 stride1: Optional[int] = None, stride2: Optional[int] = None):
        """calculate_haarpsi on two u8 images that already live in HBM (device addresses + shapes; strides in bytes, dense when
        None)."""
        args = self._haarpsi_args("calculate_haarpsi", shape1, shape2, crop_border, subsample, convention, stride1, stride2)
        if not d_reference or not d_distorted:
            raise ValueError("calculate_haarpsi: null device pointer")
        return self._haarpsi_dev(self._ctx(), int(d_reference), int(d_distorted), args, return_parts)

    @staticmethod
    def _haarpsi_map_dev(ctx, d1: int, d2: int, args, xe: List[int], ye: List[int]) -> Dict[str, Any]:
        h, w, cn, cb, sub, conv, s1, s2, _ = args
        r = ctx.haarpsi_cells(d1, s1, d2, s2, h, w, cn, xe, ye, crop_border=cb, subsample=sub, convention=conv)
        val = np.array([[_native.haarpsi_cell_value(n, d) for n, d in zip(rn, rd)] for rn, rd in zip(r["num"], r["den"])],
                       np.float64).reshape(r["num"].shape)
        return {"haarpsi": val, "num": r["num"], "den": r["den"], "x_edges": list(xe), "y_edges": list(ye)}

    def evaluate_haarpsi_map(self, img1: np.ndarray, img2: np.ndarray, cell: Optional[int] = None, x_edges=None, y_edges=None,
                             subsample: bool = True, convention: str = 'matlab') -> Dict[str, Any]:
        """Where the similarity drops: HaarPSI (calculate_haarpsi's, no crop) per cell of a separable grid, with the argument
        rules of evaluate_quality_map: uniform cells of `cell` pixels (default 256) or the edge lists x_edges (0 .. W) /
        y_edges (0 .. H).  Returns (gh, gw) arrays 'haarpsi' (the value of the cell's own sums; NaN for a cell without weight),
        'num' and 'den' (summed over the channels) and the two edge lists.  A sample belongs to the cell that holds pixel
        (2 i, 2 j) (or (i, j) without subsampling): the cells' sums add up to the global ones.  Images of different shapes are
        a ValueError."""
        a = self._require_u8(np.asarray(img1), "evaluate_haarpsi_map")
        b = self._require_u8(np.asarray(img2), "evaluate_haarpsi_map")
        args = self._haarpsi_args("evaluate_haarpsi_map", a.shape, b.shape, 0, subsample, convention, None, None)
        xe, ye = self._map_edges(args[0], args[1], cell, x_edges, y_edges)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._haarpsi_map_dev(ctx, da.ptr, db.ptr, args, xe, ye)
        finally:
            da.free(); db.free()

    def evaluate_haarpsi_map_device(self, d_img1: int, shape1, d_img2: int, shape2, cell: Optional[int] = None, x_edges=None,
                                    y_edges=None, subsample: bool = True, convention: str = 'matlab',
                                    stride1: Optional[int] = None, stride2: Optional[int] = None) -> Dict[str, Any]:
        """evaluate_haarpsi_map on two u8 images that already live in HBM (device addresses + shapes; strides in bytes, dense
        when None)."""
        args = self._haarpsi_args("evaluate_haarpsi_map", shape1, shape2, 0, subsample, convention, stride1, stride2)
        xe, ye = self._map_edges(args[0], args[1], cell, x_edges, y_edges)
        if not d_img1 or not d_img2:
            raise ValueError("evaluate_haarpsi_map: null device pointer")
        return self._haarpsi_map_dev(self._ctx(), int(d_img1), int(d_img2), args, xe, ye)

    # -- NIQE, the model (no reference counterpart in code: the reference delegates to pyiqa.create_metric('niqe')) ----------
    @staticmethod
    def _niqe_args(shape, crop_border) -> Tuple[int, int, int, int]:
        """Every refusal of the NIQE methods, on the host: ValueError (SrShapeError for a side below 96 after the crop).
        -> (h, w, cn, crop_border)."""
        shape = tuple(int(v) for v in shape)
        if len(shape) not in (2, 3):
            raise ValueError(f"niqe: need an H x W or H x W x C image, got shape {shape}")
        cn = shape[2] if len(shape) == 3 else 1
        if cn not in (1, 3):
            raise ValueError("niqe: colour images must have 3 channels (RGB)")
        _native.niqe_plan(shape[0], shape[1], cn, crop_border)                    # crop_border < 0, a too-small crop
        return shape[0], shape[1], cn, int(crop_border)

    @staticmethod
    def _niqe_features_dev(ctx, d_img: int, args) -> Tuple[np.ndarray, np.ndarray]:
        h, w, cn, cb = args
        rec = ctx.niqe_u8(d_img, w * cn, h, w, cn, crop_border=cb)
        return _native.niqe_features(rec), _native.niqe_sharpness(rec)

    def niqe_features(self, image: np.ndarray, crop_border: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """The 36 NIQE features of every 96 x 96 block of a u8 image (RGB: on MATLAB's rounded u8 luma), as include/sr_hip.h
        defines them, and every block's sharpness (its mean sigma at scale 1), which fit_niqe_model selects by.
        -> (feat[nblocks, 36], sharpness[nblocks]), blocks row-major."""
        a = self._require_u8(np.asarray(image), "niqe_features")
        args = self._niqe_args(a.shape, crop_border)
        ctx = self._ctx()
        d = _DevImage(ctx, a)
        try:
            return self._niqe_features_dev(ctx, d.ptr, args)
        finally:
            d.free()

    @staticmethod
    def _niqe_value(feat: np.ndarray, params) -> float:
        v = _native.niqe_score(feat, params["mu_pris_param"], params["cov_pris_param"])
        if v != v:
            raise _native.SrShapeError(_native.last_error())
        return v

    def calculate_niqe_model(self, image: np.ndarray, params, crop_border: int = 0) -> float:
        """NIQE (Mittal, Soundararajan, Bovik 2013; the arithmetic of MATLAB's computequality and BasicSR's calculate_niqe) of
        a u8 image under the pristine model params = {'mu_pris_param': (36,) or (1, 36), 'cov_pris_param': (36, 36)} -- from
        load_niqe_params or fit_niqe_model; nothing is fetched.  Lower is better.  NOT calculate_niqe, which is the
        reference's MSCN stand-in.  A side below 96 after the crop, or fewer than two blocks without a NaN feature, is a
        ValueError (SrShapeError)."""
        params = check_niqe_params(params)
        feat, _ = self.niqe_features(image, crop_border)
        return self._niqe_value(feat, params)

    def calculate_niqe_model_device(self, d_image: int, shape, params, crop_border: int = 0) -> float:
        """calculate_niqe_model on a dense u8 image that already lives in HBM (device address + shape)."""
        params = check_niqe_params(params)
        args = self._niqe_args(shape, crop_border)
        if not d_image:
            raise ValueError("calculate_niqe_model: null device pointer")
        feat, _ = self._niqe_features_dev(self._ctx(), int(d_image), args)
        return self._niqe_value(feat, params)

    # -- BRISQUE, the model (no reference counterpart in code: the reference delegates to pyiqa.create_metric('brisque')) ----
    @staticmethod
    def _brisque_args(shape, crop_border) -> Tuple[int, int, int, int]:
        """Every refusal of the BRISQUE methods, on the host: ValueError (SrShapeError for a side below 16 after the crop).
        -> (h, w, cn, crop_border)."""
        shape = tuple(int(v) for v in shape)
        if len(shape) not in (2, 3):
            raise ValueError(f"brisque: need an H x W or H x W x C image, got shape {shape}")
        cn = shape[2] if len(shape) == 3 else 1
        if cn not in (1, 3):
            raise ValueError("brisque: colour images must have 3 channels (RGB)")
        _native.brisque_plan(shape[0], shape[1], cn, crop_border)                 # crop_border < 0, a too-small crop
        return shape[0], shape[1], cn, int(crop_border)

    @staticmethod
    def _brisque_features_dev(ctx, d_img: int, args) -> np.ndarray:
        h, w, cn, cb = args
        return _native.brisque_features(ctx.brisque_u8(d_img, w * cn, h, w, cn, crop_border=cb))

    def brisque_features(self, image: np.ndarray, crop_border: int = 0) -> np.ndarray:
        """The 36 BRISQUE features of a u8 image (RGB: on MATLAB's rounded u8 luma), as include/sr_hip.h defines them: 18 per
        scale over the whole cropped plane.  -> feat[36]; a fit without samples on one side is NaN."""
        a = self._require_u8(np.asarray(image), "brisque_features")
        args = self._brisque_args(a.shape, crop_border)
        ctx = self._ctx()
        d = _DevImage(ctx, a)
        try:
            return self._brisque_features_dev(ctx, d.ptr, args)
        finally:
            d.free()

    @staticmethod
    def _brisque_value(feat: np.ndarray, model) -> float:
        if np.isnan(feat).any():
            raise _native.SrShapeError("brisque: a feature is NaN (a fit without samples on one side of 0): the image has no score")
        return _native.brisque_score(feat, model)

    def calculate_brisque_model(self, image: np.ndarray, model, crop_border: int = 0) -> float:
        """BRISQUE (Mittal, Moorthy, Bovik 2012; the arithmetic of MATLAB's brisquescore and pyiqa's brisque) of a u8 image
        under the caller's RBF epsilon-SVR (load_brisque_model / brisque_model_from_libsvm; nothing is fetched, none ships).
        Lower is better.  NOT calculate_brisque, which is the reference's stand-in.  A side below 16 after the crop, or a
        NaN feature, is a ValueError (SrShapeError)."""
        model = _native.check_brisque_model(model)
        return self._brisque_value(self.brisque_features(image, crop_border), model)

    def calculate_brisque_model_device(self, d_image: int, shape, model, crop_border: int = 0) -> float:
        """calculate_brisque_model on a dense u8 image that already lives in HBM (device address + shape)."""
        model = _native.check_brisque_model(model)
        args = self._brisque_args(shape, crop_border)
        if not d_image:
            raise ValueError("calculate_brisque_model: null device pointer")
        return self._brisque_value(self._brisque_features_dev(self._ctx(), int(d_image), args), model)

    def _calculate_ssim_simple(self, img1: np.ndarray, img2: np.ndarray) -> float:
        """quality_assessment_module.py:391-417 on already-gray u8 images."""
        a = self._require_u8(np.asarray(img1), "_calculate_ssim_simple")
        b = self._require_u8(np.asarray(img2), "_calculate_ssim_simple")
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            s, n = ctx.ssim_u8(da.ptr, da.stride, db.ptr, db.stride, min(da.h, db.h), min(da.w, db.w), da.cn,
                               "simple", self.gray_shift)
            return float(s / n)
        finally:
            da.free(); db.free()

    def _to_lpips_tensor(self, image: np.ndarray) -> np.ndarray:
        """quality_assessment_module.py:197-224 as an ndarray (1, 3, H, W) in [-1, 1]; for inspection -- the GPU path
        applies the same arithmetic inside the stem convolution and never materialises this tensor."""
        img = np.asarray(image).astype(np.float32) / 255.0
        if img.ndim == 2:
            img = np.stack([img, img, img], axis=-1)
        elif img.shape[2] == 1:
            img = np.repeat(img, 3, axis=-1)
        elif img.shape[2] == 4:
            img = img[:, :, :3]
        return np.ascontiguousarray(img.transpose(2, 0, 1))[None] * np.float32(2.0) - np.float32(1.0)

    def _lpips_dev(self, a: _DevImage, b: _DevImage, net: str) -> float:
        model = self.lpips_model_vgg if net == 'vgg' else self.lpips_model_alex
        if model is None:
            raise RuntimeError("LPIPS模型未成功加载")
        h, w = min(a.h, b.h), min(a.w, b.w)                    # common top-left rectangle (:449-453)
        return model.value(a.ptr, a.stride, b.ptr, b.stride, h, w, a.cn, tile=self.lpips_tile)

    def calculate_lpips(self, img1: np.ndarray, img2: np.ndarray, net: str = 'vgg') -> float:
        if self.lpips_model_vgg is None:
            raise RuntimeError("LPIPS模型未成功加载")   # same error the reference raises without its models
        a = self._require_u8(self._preprocess_image(img1), "calculate_lpips")
        b = self._require_u8(self._preprocess_image(img2), "calculate_lpips")
        cn_a = a.shape[2] if a.ndim == 3 else 1
        cn_b = b.shape[2] if b.ndim == 3 else 1
        if cn_a != cn_b or cn_a not in (1, 3, 4):
            raise ValueError(f"calculate_lpips: channel layouts {a.shape} vs {b.shape}")
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return float(self._lpips_dev(da, db, net))
        finally:
            da.free(); db.free()

    # -- DISTS (no reference counterpart; include/sr_hip.h holds the definition, parity with DISTS_pytorch unpinned) -----------
    def _dists_dev(self, a: _DevImage, b: _DevImage) -> float:
        if self.dists_model is None:
            raise RuntimeError("DISTS needs caller-supplied weights (dists_weights= or SR_DISTS_WEIGHTS); none were given")
        if tuple(a.shape) != tuple(b.shape):
            raise ValueError(f"calculate_dists: images differ in shape: {tuple(a.shape)} vs {tuple(b.shape)}")
        if a.cn not in (1, 3, 4):
            raise ValueError(f"calculate_dists: 1, 3 or 4 channels, got {tuple(a.shape)}")
        return float(self.dists_model.value(a.ptr, a.stride, b.ptr, b.stride, a.h, a.w, a.cn, tile=self.dists_tile))

    def calculate_dists(self, img1: np.ndarray, img2: np.ndarray) -> float:
        """DISTS (Ding et al. 2020) of two u8 images of equal shape, lower is better, 0 for equal images (up to 1e-12)."""
        if self.dists_model is None:
            raise RuntimeError("DISTS needs caller-supplied weights (dists_weights= or SR_DISTS_WEIGHTS); none were given")
        a = self._require_u8(np.asarray(img1), "calculate_dists")
        b = self._require_u8(np.asarray(img2), "calculate_dists")
        if a.shape != b.shape:
            raise ValueError(f"calculate_dists: images differ in shape: {a.shape} vs {b.shape}")
        if a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (1, 3, 4)):
            raise ValueError(f"calculate_dists: 1, 3 or 4 channels, got {a.shape}")
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._dists_dev(da, db)
        finally:
            da.free(); db.free()

    def calculate_dists_device(self, d_img1: int, shape1, d_img2: int, shape2) -> float:
        """calculate_dists on two dense u8 images that already live in HBM (device addresses + shapes)."""
        if self.dists_model is None:
            raise RuntimeError("DISTS needs caller-supplied weights (dists_weights= or SR_DISTS_WEIGHTS); none were given")
        if not d_img1 or not d_img2:
            raise ValueError("calculate_dists: null device pointer")
        ctx = self._ctx()
        return self._dists_dev(_DevImage(ctx, shape=tuple(shape1), ptr=d_img1), _DevImage(ctx, shape=tuple(shape2), ptr=d_img2))

    # -- full-reference evaluation (quality_assessment_module.py:467-609) ------------------------------------
    def evaluate_full_reference(self, original: np.ndarray, upscaled: np.ndarray, scale_factor: int = 4) -> Dict[str, float]:
        o, u = self._pair(original, upscaled, "evaluate_full_reference")
        ctx = self._ctx()
        d_o, d_u = _DevImage(ctx, o), _DevImage(ctx, u)      # uploaded once, every metric reads HBM
        return self._evaluate_full_reference_dev(d_o, d_u)

    def evaluate_full_reference_device(self, d_original: int, original_shape, d_upscaled: int, upscaled_shape,
                                       scale_factor: int = 4) -> Dict[str, float]:
        """evaluate_full_reference on two dense u8 images that already live in HBM (device addresses + shapes): what
        the device-resident pipeline calls -- nothing is uploaded, only the scalar sums come back."""
        ctx = self._ctx()
        if len(original_shape) != len(upscaled_shape) or (len(original_shape) == 3 and original_shape[2] != upscaled_shape[2]):
            raise ValueError(f"evaluate_full_reference: images have different channel layouts {original_shape} vs {upscaled_shape}")
        return self._evaluate_full_reference_dev(_DevImage(ctx, shape=original_shape, ptr=d_original),
                                                 _DevImage(ctx, shape=upscaled_shape, ptr=d_upscaled))

    def _evaluate_full_reference_dev(self, d_o: _DevImage, d_u: _DevImage) -> Dict[str, float]:
        ctx = d_o.ctx
        try:
            metrics: Dict[str, Any] = {}
            metrics.update(self._downsample_comparison_dev(d_o, d_u))
            if d_o.shape == d_u.shape:
                # PSNR, SSIM and MS-SSIM of the full-size pair from ONE pass over both images (sr_assess_u8)
                h, w, cn = d_o.h, d_o.w, d_o.cn
                if self.ssim_branch == 'B':
                    flags, m1, m2 = _native.ASSESS_SSE | _native.ASSESS_SIMPLE, "simple", "simple"
                else:
                    flags, m1, m2 = _native.ASSESS_SSE | _native.ASSESS_UNIFORM7 | _native.ASSESS_GAUSS11, "uniform", "gauss"
                r = ctx.assess_u8(d_o.ptr, d_o.stride, d_u.ptr, d_u.stride, h, w, cn, flags=flags,
                                  gray_shift=self.gray_shift)
                metrics['psnr'] = float(_native.psnr_from_sse(int(round(r["sse"])), h * w * cn, 255.0))
                metrics['ssim'] = float(r[f"ssim_{m1}"] / _native.ssim_count(h, w, m1))
                metrics['ms_ssim'] = float(r[f"ssim_{m2}"] / _native.ssim_count(h, w, m2))
            else:
                metrics['psnr'] = float(self._psnr_dev(d_o, d_u, 255.0))
                metrics['ssim'] = float(self._ssim_dev(d_o, d_u, False, 255.0))
                metrics['ms_ssim'] = float(self._ssim_dev(d_o, d_u, True, 255.0))
            metrics['psnr_level'] = self._assess_psnr(metrics['psnr'])
            metrics['ssim_level'] = self._assess_ssim(metrics['ms_ssim'])
            if self.lpips_model_vgg is not None:               # only when weights were given (:508-511)
                metrics['lpips_vgg'] = float(self._lpips_dev(d_o, d_u, 'vgg'))
                if self.lpips_model_alex is not None:
                    metrics['lpips_alex'] = float(self._lpips_dev(d_o, d_u, 'alex'))
                metrics['lpips_level'] = self._assess_lpips(metrics['lpips_vgg'])
            metrics['overall_score'] = self._calculate_overall_score(metrics)
            if self.dists_model is not None and d_o.shape == d_u.shape:   # only with weights; takes no part in the overall score
                metrics['dists'] = self._dists_dev(d_o, d_u)
            return metrics
        finally:
            d_o.free(); d_u.free()

    # -- per-cell quality map (no reference counterpart: the reference's UI shows a heat-map it never computes) ----------
    @staticmethod
    def _map_edges(h: int, w: int, cell: Optional[int], x_edges, y_edges) -> Tuple[List[int], List[int]]:
        """The grid of a quality map: uniform cells of `cell` pixels (None: 256; the last row / column is smaller when
        `cell` does not divide the side) or the two edge lists.  Host only; ValueError for anything else."""
        if (x_edges is None) != (y_edges is None):
            raise ValueError("quality map: give both x_edges and y_edges, or neither")
        if x_edges is not None:
            if cell is not None:
                raise ValueError("quality map: give either cell or the edge lists, not both")
            xe, ye = [int(v) for v in x_edges], [int(v) for v in y_edges]
            if any(int(v) != v for v in list(x_edges) + list(y_edges)):
                raise ValueError("quality map: edges must be whole numbers")
        else:
            cell = 256 if cell is None else cell
            if int(cell) != cell or cell < 1:
                raise ValueError(f"quality map: cell must be a whole number >= 1, got {cell!r}")
            cell = int(cell)
            xe = list(range(0, w, cell)) + [w]
            ye = list(range(0, h, cell)) + [h]
        _native.quality_map_counts(h, w, "simple", xe, ye)              # the library's own edge check (host only)
        return xe, ye

    def evaluate_quality_map(self, img1: np.ndarray, img2: np.ndarray, cell: Optional[int] = None, x_edges=None,
                             y_edges=None) -> Dict[str, Any]:
        """Where the quality is bad: PSNR and SSIM per cell of a separable grid over the common top-left rectangle of the
        two images (preprocessing, u8 requirement and channel-layout check of calculate_psnr / calculate_ssim).  The grid
        is uniform cells of `cell` pixels (default 256) or the edge lists x_edges (0 .. W) / y_edges (0 .. H).  Returns
        x_edges, y_edges and (gh, gw) arrays: sse, mse, psnr (inf where mse == 0), ssim / ms_ssim (per-cell means with the
        branch rule of evaluate_full_reference: uniform / gauss for ssim_branch 'A', simple / simple for 'B'; nan for a cell
        without a valid sample) and ssim_count / ms_ssim_count.  Cells are bins for results: the filters read across their
        boundaries, so sums over the cells give the global metrics."""
        a, b = self._pair(img1, img2, "evaluate_quality_map")
        if a.ndim == 3 and a.shape[2] not in (1, 3):
            raise ValueError("evaluate_quality_map: colour images must have 3 channels (cv2.COLOR_RGB2GRAY)")
        h, w = min(a.shape[0], b.shape[0]), min(a.shape[1], b.shape[1])
        xe, ye = self._map_edges(h, w, cell, x_edges, y_edges)
        ctx = self._ctx()
        da, db = _DevImage(ctx, a), _DevImage(ctx, b)
        try:
            return self._quality_map_dev(da, db, xe, ye)
        finally:
            da.free(); db.free()

    def evaluate_quality_map_device(self, d_img1: int, shape1, d_img2: int, shape2, cell: Optional[int] = None, x_edges=None,
                                    y_edges=None) -> Dict[str, Any]:
        """evaluate_quality_map on two dense u8 images that already live in HBM (device addresses + shapes)."""
        shape1, shape2 = tuple(int(v) for v in shape1), tuple(int(v) for v in shape2)
        if len(shape1) not in (2, 3) or len(shape1) != len(shape2) or (len(shape1) == 3 and shape1[2] != shape2[2]):
            raise ValueError(f"evaluate_quality_map: images have different channel layouts {shape1} vs {shape2}")
        if len(shape1) == 3 and shape1[2] not in (1, 3):
            raise ValueError("evaluate_quality_map: colour images must have 3 channels (cv2.COLOR_RGB2GRAY)")
        h, w = min(shape1[0], shape2[0]), min(shape1[1], shape2[1])
        xe, ye = self._map_edges(h, w, cell, x_edges, y_edges)
        ctx = self._ctx()
        return self._quality_map_dev(_DevImage(ctx, shape=shape1, ptr=d_img1), _DevImage(ctx, shape=shape2, ptr=d_img2), xe, ye)

    def _quality_map_dev(self, a: _DevImage, b: _DevImage, xe: List[int], ye: List[int]) -> Dict[str, Any]:
        h, w, cn = min(a.h, b.h), min(a.w, b.w), a.cn
        if self.ssim_branch == 'B':
            flags, m1, m2 = _native.ASSESS_SSE | _native.ASSESS_SIMPLE, "simple", "simple"
        else:
            flags, m1, m2 = _native.ASSESS_SSE | _native.ASSESS_UNIFORM7 | _native.ASSESS_GAUSS11, "uniform", "gauss"
        r = a.ctx.quality_map_u8(a.ptr, a.stride, b.ptr, b.stride, h, w, cn, xe, ye, flags=flags, gray_shift=self.gray_shift)
        n1, n2 = _native.quality_map_counts(h, w, m1, xe, ye), _native.quality_map_counts(h, w, m2, xe, ye)
        elems = np.outer(np.diff(ye), np.diff(xe)).astype(np.float64) * cn
        mse = r["sse"].astype(np.float64) / elems
        with np.errstate(divide="ignore", invalid="ignore"):
            psnr = np.where(mse == 0, np.inf, 10.0 * np.log10(255.0 ** 2 / mse))
            ssim = np.where(n1 > 0, r[f"ssim_{m1}"] / n1, np.nan)
            ms_ssim = np.where(n2 > 0, r[f"ssim_{m2}"] / n2, np.nan)
        return {"x_edges": list(xe), "y_edges": list(ye), "sse": r["sse"], "mse": mse, "psnr": psnr, "ssim": ssim,
                "ms_ssim": ms_ssim, "ssim_count": n1, "ms_ssim_count": n2}

    def _downsample_comparison_dev(self, d_o: _DevImage, d_u: _DevImage) -> Dict[str, float]:
        out = {}
        for scale in self.scale_config.scale_factors:
            if scale >= 1.0 or scale <= 0:
                raise ValueError(f"scale_factor必须在(0, 1)范围内，当前值: {scale}")
            name = self.scale_config.scale_names.get(scale, f"scale_{scale}")
            if d_o.shape == d_u.shape and int(d_o.h * scale) >= 1 and int(d_o.w * scale) >= 1:
                # both bicubic resizes, PSNR and SSIM of the resized pair in one kernel: the resized images are
                # sampled on the fly and never written (sr_assess_resized_u8)
                dh, dw, cn = int(d_o.h * scale), int(d_o.w * scale), d_o.cn
                mode = "simple" if self.ssim_branch == 'B' else "uniform"
                bit = _native.ASSESS_SIMPLE if mode == "simple" else _native.ASSESS_UNIFORM7
                r = d_o.ctx.assess_resized_u8(d_o.ptr, d_o.stride, d_u.ptr, d_u.stride, d_o.h, d_o.w, cn, dh, dw,
                                              flags=_native.ASSESS_SSE | bit, gray_shift=self.gray_shift)
                out[f'psnr_{name}'] = float(_native.psnr_from_sse(int(round(r["sse"])), dh * dw * cn, 255.0))
                out[f'ssim_{name}'] = float(r[f"ssim_{mode}"] / _native.ssim_count(dh, dw, mode))
                continue
            sr = self._resize_dev(d_u, int(d_u.h * scale), int(d_u.w * scale))
            hr = self._resize_dev(d_o, int(d_o.h * scale), int(d_o.w * scale))
            out[f'psnr_{name}'] = float(self._psnr_dev(hr, sr, 255.0))
            out[f'ssim_{name}'] = float(self._ssim_dev(hr, sr, False, 255.0))
            sr.free(); hr.free()
        return out

    def _evaluate_downsample_comparison(self, original: np.ndarray, upscaled: np.ndarray, scale_factor: int) -> Dict[str, float]:
        o, u = self._pair(original, upscaled, "_evaluate_downsample_comparison")
        ctx = self._ctx()
        d_o, d_u = _DevImage(ctx, o), _DevImage(ctx, u)
        try:
            return self._downsample_comparison_dev(d_o, d_u)
        finally:
            d_o.free(); d_u.free()

    def _assess_psnr(self, v: float) -> str:
        t = self.thresholds
        if v >= t.PSNR_EXCELLENT:
            return AssessmentLevel.EXCELLENT.value
        if v >= t.PSNR_GOOD:
            return AssessmentLevel.GOOD.value
        if v >= t.PSNR_FAIR:
            return AssessmentLevel.FAIR.value
        return AssessmentLevel.POOR.value

    def _assess_ssim(self, v: float) -> str:
        t = self.thresholds
        if v >= t.SSIM_EXCELLENT:
            return AssessmentLevel.EXCELLENT.value
        if v >= t.SSIM_GOOD:
            return AssessmentLevel.GOOD.value
        if v >= t.SSIM_FAIR:
            return AssessmentLevel.FAIR.value
        return AssessmentLevel.POOR.value

    def _assess_lpips(self, v: float) -> str:
        t = self.thresholds
        if v <= t.LPIPS_EXCELLENT:
            return AssessmentLevel.EXCELLENT.value
        if v <= t.LPIPS_GOOD:
            return AssessmentLevel.GOOD.value
        if v <= t.LPIPS_FAIR:
            return AssessmentLevel.FAIR.value
        return AssessmentLevel.POOR.value

    def _calculate_overall_score(self, metrics: Dict[str, float]) -> float:
        scores = []
        if 'psnr' in metrics:
            scores.append(min(100, max(0, metrics['psnr'])))
        if 'ms_ssim' in metrics:
            scores.append(metrics['ms_ssim'] * 100)
        if 'lpips_vgg' in metrics:
            scores.append(max(0, (1 - metrics['lpips_vgg']) * 100))
        return float(np.mean(scores)) if scores else 0.0

    # -- no-reference and commercial metrics (quality_assessment_module.py:611-1193) -----------------------------------
    # Every metric runs in ONE sr_commercial_u8 call (csrc/sr_commercial.hip) that returns exact integer sums and fixed-order
    # fp64 sums; the scalar formulas below finish them.  The private helpers keep the reference's names and each take one
    # (host) image, like the reference's.

    def _commercial_image(self, image: Any, what: str) -> np.ndarray:
        img = self._require_u8(np.asarray(self._preprocess_image(image)), what)
        if img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] not in (3, 4)) or img.shape[0] < 1 or img.shape[1] < 1:
            raise ValueError(f"{what}: expected a u8 HxW, HxWx3 or HxWx4 image, got shape {img.shape}")
        return img

    @staticmethod
    def _check_dev_shape(shape, what: str) -> Tuple[int, ...]:
        shape = tuple(int(v) for v in shape)
        if len(shape) not in (2, 3) or (len(shape) == 3 and shape[2] not in (3, 4)) or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"{what}: expected a u8 HxW, HxWx3 or HxWx4 image, got shape {shape}")
        return shape

    def _cm_sums(self, d: _DevImage, flags: int, rois=(), roi_flags=()):
        if flags & _native.CM_HF and max(d.h, d.w) > _FFT_MAX_LEN:
            raise NotImplementedError(f"high-frequency ratio: image side {max(d.h, d.w)} is above the longest DFT line "
                                      f"the HIP FFT supports ({_FFT_MAX_LEN})")
        return d.ctx.commercial_u8(d.ptr, d.stride, d.h, d.w, d.cn, flags, rois, roi_flags, gray_shift=self.gray_shift)

    def _cm_host(self, image: Any, flags: int, what: str):
        img = self._commercial_image(image, what)
        ctx = self._ctx()
        if flags & _native.CM_HF and max(img.shape[:2]) > _FFT_MAX_LEN:
            raise NotImplementedError(f"{what}: image side {max(img.shape[:2])} is above the longest DFT line the HIP FFT "
                                      f"supports ({_FFT_MAX_LEN})")
        d = _DevImage(ctx, img)
        try:
            ints, flts = self._cm_sums(d, flags)
        finally:
            d.free()
        return img, ints[0], flts[0]

    # scalar finishing ----------------------------------------------------------------------------------------------
    @staticmethod
    def _var(s1: int, s2: int, n: int) -> float:
        """Population variance from exact integer sums, correctly rounded."""
        s1, s2, n = int(s1), int(s2), int(n)
        return (n * s2 - s1 * s1) / (n * n)

    @staticmethod
    def _color_variance_of(r, n: int) -> float:
        return float(QualityAssessmentModule._var(r[7], r[8], n))

    @staticmethod
    def _colorfulness_of(r, n: int) -> float:
        v = QualityAssessmentModule._var
        return float(np.sqrt(np.sqrt(v(r[9], r[10], n)) ** 2 + np.sqrt(v(r[11], r[12], n)) ** 2))

    @staticmethod
    def _noise_of(r, n: int) -> float:
        return float(np.sqrt(max(QualityAssessmentModule._var(r[4], r[5], n), 0.0)) / 16.0)

    @staticmethod
    def _artifact_of(r) -> float:
        nb = int(r[38])
        if nb <= 1:
            return 100.0
        s, q = int(r[17]), int(r[18]) + (int(r[19]) << 32)
        vv = (nb * q - s * s) / (nb * nb * 4096 * 4096)              # np.var of the block variances
        return float(max(0, 100 - vv / 100))

    @staticmethod
    def _uniformity_of(r, h: int, w: int) -> float:
        rh, rw = h // 4, w // 4
        if rh == 0 or rw == 0:
            return 0.0                                                # empty regions: NaN, and max(0, nan) is 0
        means = np.array([int(v) / (rh * rw) for v in r[20:36]], dtype=np.float64)
        return float(max(0, 100 - np.std(means)))

    @staticmethod
    def _oversharpen_of(r, n: int) -> float:
        return float(max(0, 100 - (int(r[36]) / n) * 500))

    @staticmethod
    def _hf_of(f) -> float:
        return float(f[5] / (f[6] + 1e-10))

    @staticmethod
    def _mscn_stats(f, n: int):
        mean = f[0] / n
        std = float(np.sqrt(max(f[1] / n - mean * mean, 0.0)))
        return float(mean), std, float(f[2] / n)

    def _niqe_of(self, f, n: int) -> float:
        mean, std, _ = self._mscn_stats(f, n)
        return float(np.clip((std + abs(mean)) * 2.0 + 3.0, 1.0, 15.0))

    def _brisque_of(self, r, f, n: int) -> float:
        mean, std, mabs = self._mscn_stats(f, n)
        gmean = f[3] / n
        gstd = float(np.sqrt(max(int(r[6]) / n - gmean * gmean, 0.0)))
        return float(np.clip(np.mean([mean, std, mabs, gmean, gstd]) * 10 + 20, 0, 100))

    @staticmethod
    def _face_of(r, n: int) -> float:
        ratio = int(r[13]) / n
        return float(np.clip(100 - abs(ratio - 0.3) * 100, 0, 100))

    @staticmethod
    def _skin_tone_of(r, n: int) -> float:
        lm, am, bm = int(r[7]) / n, int(r[9]) / n, int(r[11]) / n
        d = np.sqrt((lm - 70) ** 2 + (am - 15) ** 2 + (bm - 20) ** 2)
        return float(max(0, 100 - d))

    @staticmethod
    def _delta_e_of(r, n: int, reference_color) -> float:
        mean_color = np.array([int(r[14]) / n, int(r[15]) / n, int(r[16]) / n])
        ref_lab = _lab8(np.uint8([[reference_color]])[0, 0])
        img_lab = _lab8(mean_color.astype(np.uint8))
        return float(np.sqrt(np.sum((ref_lab.astype(np.float32) - img_lab.astype(np.float32)) ** 2)))

    # reference-named helpers (each one device call on a host image) --------------------------------------------------
    def _calculate_sharpness(self, image: np.ndarray) -> float:
        img, r, _ = self._cm_host(image, _native.CM_LAPG, "_calculate_sharpness")
        return float(self._var(r[0], r[1], img.shape[0] * img.shape[1]))

    def _calculate_contrast(self, image: np.ndarray) -> float:
        img, r, _ = self._cm_host(image, _native.CM_LAPG, "_calculate_contrast")
        return float(np.sqrt(self._var(r[2], r[3], img.shape[0] * img.shape[1])))

    def _calculate_colorfulness(self, image: np.ndarray) -> float:
        img = self._commercial_image(image, "_calculate_colorfulness")
        if img.ndim != 3:
            return 0.0
        _, r, _ = self._cm_host(img, _native.CM_LAB, "_calculate_colorfulness")
        return self._colorfulness_of(r, img.shape[0] * img.shape[1])

    def _calculate_color_variance(self, image: np.ndarray) -> float:
        img = self._commercial_image(image, "_calculate_color_variance")
        if img.ndim != 3:
            return 0.0
        _, r, _ = self._cm_host(img, _native.CM_LAB, "_calculate_color_variance")
        return self._color_variance_of(r, img.shape[0] * img.shape[1])

    def _calculate_hf_ratio(self, image: np.ndarray) -> float:
        _, _, f = self._cm_host(image, _native.CM_HF, "_calculate_hf_ratio")
        return self._hf_of(f)

    def _detect_oversharpen(self, image: np.ndarray) -> float:
        img, r, _ = self._cm_host(image, _native.CM_CANNY, "_detect_oversharpen")
        return self._oversharpen_of(r, img.shape[0] * img.shape[1])

    def _detect_artifacts(self, image: np.ndarray) -> float:
        _, r, _ = self._cm_host(image, _native.CM_BLOCKS, "_detect_artifacts")
        return self._artifact_of(r)

    def _estimate_noise(self, image: np.ndarray) -> float:
        img, r, _ = self._cm_host(image, _native.CM_NOISE, "_estimate_noise")
        return self._noise_of(r, img.shape[0] * img.shape[1])

    def _calculate_brightness_uniformity(self, image: np.ndarray) -> float:
        img, r, _ = self._cm_host(image, _native.CM_REGIONS, "_calculate_brightness_uniformity")
        return self._uniformity_of(r, img.shape[0], img.shape[1])

    def _calculate_texture_score(self, image: np.ndarray) -> float:
        img, _, f = self._cm_host(image, _native.CM_TEX, "_calculate_texture_score")
        return float(f[4] / (img.shape[0] * img.shape[1]))

    def _calculate_face_naturalness(self, image: np.ndarray) -> float:
        img = self._commercial_image(image, "_calculate_face_naturalness")
        if img.ndim != 3:
            return 50.0
        _, r, _ = self._cm_host(img, _native.CM_SKIN, "_calculate_face_naturalness")
        return self._face_of(r, img.shape[0] * img.shape[1])

    def _calculate_skin_tone_naturalness(self, image: np.ndarray) -> float:
        img = self._commercial_image(image, "_calculate_skin_tone_naturalness")
        if img.ndim != 3:
            return 50.0
        _, r, _ = self._cm_host(img, _native.CM_LAB, "_calculate_skin_tone_naturalness")
        return self._skin_tone_of(r, img.shape[0] * img.shape[1])

    def _calculate_delta_e(self, image: np.ndarray, reference_color: Tuple[int, int, int]) -> float:
        img = self._commercial_image(image, "_calculate_delta_e")
        if img.ndim != 3:
            return 100.0
        _, r, _ = self._cm_host(img, _native.CM_RGB, "_calculate_delta_e")
        return self._delta_e_of(r, img.shape[0] * img.shape[1], reference_color)

    def _calculate_niqe_simple(self, image: np.ndarray) -> float:
        img, _, f = self._cm_host(image, _native.CM_MSCN, "_calculate_niqe_simple")
        return self._niqe_of(f, img.shape[0] * img.shape[1])

    def _calculate_brisque_simple(self, image: np.ndarray) -> float:
        img, r, f = self._cm_host(image, _native.CM_MSCN | _native.CM_SOBEL, "_calculate_brisque_simple")
        return self._brisque_of(r, f, img.shape[0] * img.shape[1])

    def calculate_niqe(self, image: np.ndarray) -> float:
        # the pyiqa model branch stays unavailable (_niqe_available is False): the simplified stand-in runs
        return self._calculate_niqe_simple(self._preprocess_image(image))

    def calculate_brisque(self, image: np.ndarray) -> float:
        return self._calculate_brisque_simple(self._preprocess_image(image))

    # levels and the composite score ------------------------------------------------------------------------------------
    def _assess_niqe(self, v: float) -> str:
        t = self.thresholds
        if v <= t.NIQE_EXCELLENT:
            return AssessmentLevel.EXCELLENT.value
        if v <= t.NIQE_GOOD:
            return AssessmentLevel.GOOD.value
        if v <= t.NIQE_FAIR:
            return AssessmentLevel.FAIR.value
        return AssessmentLevel.POOR.value

    def _assess_brisque(self, v: float) -> str:
        t = self.thresholds
        if v <= t.BRISQUE_EXCELLENT:
            return AssessmentLevel.EXCELLENT.value
        if v <= t.BRISQUE_GOOD:
            return AssessmentLevel.GOOD.value
        if v <= t.BRISQUE_FAIR:
            return AssessmentLevel.FAIR.value
        return AssessmentLevel.POOR.value

    def _assess_delta_e(self, v: float) -> str:
        t = self.thresholds
        if v <= t.DELTA_E_EXCELLENT:
            return AssessmentLevel.EXCELLENT.value
        if v <= t.DELTA_E_GOOD:
            return AssessmentLevel.GOOD.value
        if v <= t.DELTA_E_FAIR:
            return AssessmentLevel.FAIR.value
        return AssessmentLevel.POOR.value

    def _calculate_commercial_score(self, metrics: Dict[str, float]) -> float:
        scores = []
        if 'global_sharpness' in metrics:
            scores.append(min(100, metrics['global_sharpness'] / 10))
        if 'high_frequency_ratio' in metrics:
            scores.append(min(100, metrics['high_frequency_ratio'] * 500))
        if 'oversharpen_score' in metrics:
            scores.append(metrics['oversharpen_score'])
        if 'artifact_score' in metrics:
            scores.append(metrics['artifact_score'])
        return float(np.mean(scores)) if scores else 50.0

    # public evaluations ----------------------------------------------------------------------------------------------
    def evaluate_no_reference(self, image: Any) -> Dict[str, Any]:
        """quality_assessment_module.py:749-780: NIQE / BRISQUE stand-ins, sharpness, contrast, colorfulness from one
        device pass."""
        img = self._commercial_image(image, "evaluate_no_reference")
        flags = _native.CM_LAPG | _native.CM_MSCN | _native.CM_SOBEL | (_native.CM_LAB if img.ndim == 3 else 0)
        _, r, f = self._cm_host(img, flags, "evaluate_no_reference")
        n = img.shape[0] * img.shape[1]
        m: Dict[str, Any] = {}
        m['niqe'] = self._niqe_of(f, n)
        m['niqe_level'] = self._assess_niqe(m['niqe'])
        m['brisque'] = self._brisque_of(r, f, n)
        m['brisque_level'] = self._assess_brisque(m['brisque'])
        m['sharpness'] = float(self._var(r[0], r[1], n))
        m['contrast'] = float(np.sqrt(self._var(r[2], r[3], n)))
        m['colorfulness'] = self._colorfulness_of(r, n) if img.ndim == 3 else 0.0
        return m

    def evaluate_commercial(self, image: Any, roi_regions: Optional[List[Dict]] = None) -> Dict[str, Any]:
        """quality_assessment_module.py:873-1193 with the reference's key order; one upload, one device pass."""
        img = self._commercial_image(image, "evaluate_commercial")
        plan = self._roi_plan(img.shape, roi_regions)
        if max(img.shape[:2]) > _FFT_MAX_LEN:
            raise NotImplementedError(f"evaluate_commercial: image side {max(img.shape[:2])} is above the longest DFT line "
                                      f"the HIP FFT supports ({_FFT_MAX_LEN})")
        ctx = self._ctx()
        d = _DevImage(ctx, img)
        try:
            return self._evaluate_commercial_dev(d, plan)
        finally:
            d.free()

    def evaluate_commercial_device(self, d_image: int, shape, roi_regions: Optional[List[Dict]] = None) -> Dict[str, Any]:
        """evaluate_commercial on a dense u8 image already in HBM (device address + shape): nothing is uploaded, a few
        hundred bytes of sums come back."""
        shape = self._check_dev_shape(shape, "evaluate_commercial")
        plan = self._roi_plan(shape, roi_regions)
        if max(shape[:2]) > _FFT_MAX_LEN:
            raise NotImplementedError(f"evaluate_commercial: image side {max(shape[:2])} is above the longest DFT line the "
                                      f"HIP FFT supports ({_FFT_MAX_LEN})")
        return self._evaluate_commercial_dev(_DevImage(self._ctx(), shape=shape, ptr=d_image), plan)

    @staticmethod
    def _roi_plan(shape, roi_regions) -> List[Tuple[int, str, Tuple[int, int, int, int], Any]]:
        """The reference's ROI rules (:905-925, :1010-1030): (index, type, clipped bbox, reference_color) of every ROI that
        keeps a non-empty area.  Raises like the reference would (before any device work) on a malformed bbox."""
        H, W = int(shape[0]), int(shape[1])
        plan = []
        if not roi_regions:
            return plan
        for i, roi in enumerate(roi_regions):
            rtype = roi.get('type', f'roi_{i}')
            bbox = roi.get('bbox', [0, 0, W, H])
            x, y, w, h = bbox
            for v in (x, y, w, h):
                if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                    raise TypeError(f"roi {i}: bbox values must be integers, got {bbox!r}")
            x, y = max(0, int(x)), max(0, int(y))
            w, h = min(int(w), W - x), min(int(h), H - y)
            if w > 0 and h > 0:
                plan.append((i, rtype, (x, y, w, h), roi.get('reference_color', None)))
        return plan

    def _evaluate_commercial_dev(self, d: _DevImage, plan) -> Dict[str, Any]:
        colour = d.cn >= 3
        rois, rflags, slot = [], [], {}
        for i, rtype, box, ref in plan:
            f = 0
            if rtype == 'text':
                f = _native.CM_LAPG
            elif rtype == 'product':
                f = _native.CM_TEX
            elif rtype == 'face' and colour:
                f = _native.CM_SKIN
            elif rtype == 'brand' and ref is not None and colour:
                np.uint8([[ref]])                                     # a bad reference colour raises before the device call
                f = _native.CM_RGB
            if f:
                slot[i] = 1 + len(rois)
                rois.append(box)
                rflags.append(f)
        flags = (_native.CM_LAPG | _native.CM_NOISE | _native.CM_BLOCKS | _native.CM_REGIONS | _native.CM_CANNY |
                 _native.CM_HF | (_native.CM_LAB if colour else 0))
        ints, flts = self._cm_sums(d, flags, rois, rflags)
        g, gf = ints[0], flts[0]
        h, w = d.h, d.w
        n = h * w
        m: Dict[str, Any] = {}
        # 1. detail fidelity
        m['global_sharpness'] = float(self._var(g[0], g[1], n))
        m['high_frequency_ratio'] = self._hf_of(gf)
        for i, rtype, (x, y, rw, rh), _ in plan:
            nr = rw * rh
            if rtype == 'text':
                r = ints[slot[i]]
                m[f'text_sharpness_{i}'] = float(self._var(r[0], r[1], nr))
                m[f'text_contrast_{i}'] = float(np.sqrt(self._var(r[2], r[3], nr)))
            elif rtype == 'product':
                m[f'product_texture_{i}'] = float(flts[slot[i]][4] / nr)
            elif rtype == 'face':
                m[f'face_naturalness_{i}'] = self._face_of(ints[slot[i]], nr) if colour else 50.0
        # 2. colour accuracy
        m['color_variance'] = self._color_variance_of(g, n) if colour else 0.0
        for i, rtype, (x, y, rw, rh), ref in plan:
            nr = rw * rh
            if rtype == 'brand' and ref is not None:
                de = self._delta_e_of(ints[slot[i]], nr, ref) if colour else 100.0
                m[f'brand_color_delta_e_{i}'] = de
                m[f'brand_color_accuracy_{i}'] = self._assess_delta_e(de)
            elif rtype == 'face':
                m[f'skin_tone_naturalness_{i}'] = self._skin_tone_of(ints[slot[i]], nr) if colour else 50.0
        # 3. visual comfort
        m['oversharpen_score'] = self._oversharpen_of(g, n)
        m['artifact_score'] = self._artifact_of(g)
        m['noise_level'] = self._noise_of(g, n)
        m['brightness_uniformity'] = self._uniformity_of(g, h, w)
        # 4. composite
        m['commercial_score'] = self._calculate_commercial_score(m)
        return m


_FFT_MAX_LEN = 32768          # sr_fft_max_len(): longest DFT line of the hand-written FFT (checked against the library)


# -- the pristine model of NIQE: check, fit, save, load ---------------------------------------------------------------------
def mod_crop(image: np.ndarray, scale: int) -> np.ndarray:
    """The top-left (h - h % scale) x (w - w % scale) of an image, as a view: what the SR benchmarks do to a ground-truth
    image before they degrade it, so that the upscaled result has its size."""
    s = _native._whole(scale, "scale")
    if s < 1:
        raise ValueError(f"mod_crop: scale must be >= 1, got {s}")
    image = np.asarray(image)
    h, w = image.shape[:2]
    return image[:h - h % s, :w - w % s]


def check_niqe_params(params) -> Dict[str, np.ndarray]:
    """-> {'mu_pris_param': float64 (36,), 'cov_pris_param': float64 (36, 36)}; ValueError for missing keys or other shapes
    (mu may come as (36,) or (1, 36))."""
    try:
        mu, cov = np.asarray(params["mu_pris_param"], dtype=np.float64), np.asarray(params["cov_pris_param"], dtype=np.float64)
    except (KeyError, TypeError, IndexError) as exc:
        raise ValueError("NIQE parameters need the keys 'mu_pris_param' and 'cov_pris_param'") from exc
    if mu.shape not in ((36,), (1, 36)):
        raise ValueError(f"NIQE parameters: mu_pris_param must have shape (36,) or (1, 36), got {mu.shape}")
    if cov.shape != (36, 36):
        raise ValueError(f"NIQE parameters: cov_pris_param must have shape (36, 36), got {cov.shape}")
    return {"mu_pris_param": np.ascontiguousarray(mu.reshape(36)), "cov_pris_param": np.ascontiguousarray(cov)}


def fit_niqe_model(images, threshold: float = 0.75, module: Optional[QualityAssessmentModule] = None) -> Dict[str, np.ndarray]:
    """The pristine model of NIQE fitted from the caller's own sharp u8 images by the published training rule (MATLAB's
    estimatemodelparam): per image the blocks whose sharpness exceeds threshold x the image's sharpest block, pooled; their
    mean and sample covariance.  -> {'mu_pris_param', 'cov_pris_param'}.  Fewer than 37 usable blocks is a ValueError that
    gives the count."""
    q = module or QualityAssessmentModule()
    feats, sharps = [], []
    for img in images:
        f, s = q.niqe_features(img)
        feats.append(f)
        sharps.append(s)
    mu, cov, _ = _native.niqe_fit(feats, sharps, threshold)
    return {"mu_pris_param": mu, "cov_pris_param": cov}


def save_niqe_params(path: str, params) -> None:
    """.npz with BasicSR's key names (mu_pris_param (1, 36), cov_pris_param (36, 36)), or .mat with MATLAB's (mu_prisparam,
    cov_prisparam) through scipy.io."""
    p = check_niqe_params(params)
    mu, cov = p["mu_pris_param"].reshape(1, 36), p["cov_pris_param"]
    if str(path).lower().endswith(".mat"):
        try:
            from scipy import io as sio
        except ImportError as exc:
            raise RuntimeError("writing a .mat parameter file needs scipy") from exc
        sio.savemat(str(path), {"mu_prisparam": mu, "cov_prisparam": cov})
    elif str(path).lower().endswith(".npz"):
        with open(str(path), "wb") as f:
            np.savez(f, mu_pris_param=mu, cov_pris_param=cov)
    else:
        raise ValueError(f"NIQE parameter files are .npz or .mat, got {path!r}")


def load_niqe_params(path: str) -> Dict[str, np.ndarray]:
    """Reads what save_niqe_params writes: BasicSR's niqe_pris_params.npz layout, or MATLAB's modelparameters.mat layout."""
    if str(path).lower().endswith(".mat"):
        try:
            from scipy import io as sio
        except ImportError as exc:
            raise RuntimeError("reading a .mat parameter file needs scipy") from exc
        z = sio.loadmat(str(path))
        if "mu_prisparam" not in z or "cov_prisparam" not in z:
            raise ValueError(f"{path}: no mu_prisparam / cov_prisparam")
        return check_niqe_params({"mu_pris_param": z["mu_prisparam"], "cov_pris_param": z["cov_prisparam"]})
    if str(path).lower().endswith(".npz"):
        with np.load(str(path), allow_pickle=False) as z:
            if "mu_pris_param" not in z.files or "cov_pris_param" not in z.files:
                raise ValueError(f"{path}: no mu_pris_param / cov_pris_param")
            return check_niqe_params({"mu_pris_param": z["mu_pris_param"], "cov_pris_param": z["cov_pris_param"]})
    raise ValueError(f"NIQE parameter files are .npz or .mat, got {path!r}")


# -- the regressor of BRISQUE: check, save, load, read libsvm's files (the code is _native's) -------------------------------------
check_brisque_model = _native.check_brisque_model
save_brisque_model = _native.save_brisque_model
load_brisque_model = _native.load_brisque_model
brisque_model_from_libsvm = _native.brisque_model_from_libsvm


def _lab_tables_b() -> Tuple[np.ndarray, np.ndarray]:
    """cv2's 8-bit RGB2Lab tables (OpenCV 4.x color_lab.cpp initLabTabs), the rule k_lab_tables builds on the device:
    sRGB gamma x 255 x 2^3 and the cube-root table x 2^15 over 3072 steps of 1 / (255 x 2^3), computed in fp64 and
    rounded half to even."""
    x = np.arange(256, dtype=np.float64) / 255.0
    gamma = np.rint(255.0 * 8.0 * np.where(x <= 0.04045, x / 12.92, ((x + 0.055) / 1.055) ** 2.4)).astype(np.int64)
    t = np.arange(3072, dtype=np.float64) / (255.0 * 8.0)
    cb = np.rint(32768.0 * np.where(t < 216.0 / 24389.0, t * (841.0 / 108.0) + 16.0 / 116.0, np.cbrt(t))).astype(np.int64)
    return gamma, cb


_LAB_COEFFS = np.array([[int(np.rint(4096.0 * c / wp)) for c in row] for row, wp in zip(
    ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227)),
    (0.950456, 1.0, 1.088754))], dtype=np.int64)


def _lab8(rgb) -> np.ndarray:
    """cv2.cvtColor(np.uint8([[rgb]]), COLOR_RGB2LAB)[0, 0] for one colour (alpha ignored) -> uint8[3]."""
    gamma, cb = _LAB_TABLES
    v = np.asarray(rgb, dtype=np.int64).reshape(-1)[:3]
    lin = gamma[v]
    f = cb[(_LAB_COEFFS @ lin + (1 << 11)) >> 12]
    L = (296 * f[1] - ((16 * 255 * (1 << 15) + 50) // 100) + (1 << 14)) >> 15
    a = (500 * (f[0] - f[1]) + 128 * (1 << 15) + (1 << 14)) >> 15
    b = (200 * (f[1] - f[2]) + 128 * (1 << 15) + (1 << 14)) >> 15
    return np.clip(np.array([L, a, b]), 0, 255).astype(np.uint8)


_LAB_TABLES = _lab_tables_b()
