#!/usr/bin/env python3
"""main -- SuperResolutionPipeline / PipelineConfig entry points over the MI355X-native stages.

Keeps the reference's names, config fields and defaults, result record and five-stage order
(main.py:47-89,92-134,157-192,269-441).  Stages 1, 3 and 4 (tile -> blend -> assess) run on the GPU
through tiling_module / blending_module / quality_assessment_module.  Stage 2 of the reference is a
remote vendor API (out of scope): here it is a pluggable ``sr_backend`` whose default
is the bicubic stub of BASELINE.json's configs, executed on the GPU with the resize kernel; with
``PipelineConfig.sr_weights`` set it is a local SR network of sr_network.py (compact, MSRResNet / EDSR, RRDBNet x4, RCAN
or SwinIR; caller-supplied weights).  RCAN pools every channel over the image it is given, so each tile pools over itself -- as
every tiled inference of RCAN does -- and ``block_size`` then affects the SR values.  SwinIR likewise: each tile is reflected,
padded to a multiple of 8 and cut into shifted windows on its own, as in every tiled SwinIR inference.

What is wired differently from the reference, because the reference's own wiring cannot run
(SURVEY.md 0.3): tiles are read from ``tile.data``; ``TileInfo(image, x, y, row, col)`` is built with
positional fields; the fused ndarray is saved through Pillow; QA receives ndarrays.  The fixed x2 tile
scale of main.py:217,322 is kept as the default ``sr_scale`` (an added field; every original field
keeps its name and default).  Importing this module does not create ``super_resolution.log``.

Several GPUs (one process per GPU, RANK / WORLD_SIZE / LOCAL_RANK in the environment -- ``python main.py in out
--gpus N`` starts its own ranks, a launcher such as torchrun works too): ``process()`` runs the sharded form of the same
stages.  The SR stage's tiles are owned one set per rank (the reference's fan-out is ``ParallelBlender``'s thread pool,
blending_module.py:1665-1705; here it is processes over RCCL), the canvas is blended in horizontal strips whose
owners receive the tile rows (+ pyramid halo) they need from the tile owners, the strips are gathered on rank 0, which
assesses and writes exactly what the one-GPU run writes: same file bytes, same scores.
"""
from __future__ import annotations

import asyncio
import json
import logging
import os
import sys
import time
from dataclasses import dataclass
from datetime import datetime
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional

import numpy as np

from blending_module import BlendingModule, TileInfo
from quality_assessment_module import QualityAssessmentModule
from tiling_module import Tile, TileMetadata, TilingModule

logger = logging.getLogger(__name__)


@dataclass
class PipelineConfig:
    """main.py:47-75 (same fields and defaults) + sr_scale."""
    block_size: int = 2048
    overlap_ratio: float = 0.2
    padding_mode: str = 'mirror'
    target_resolution: str = "100MP"
    seedream_strength: float = 0.5
    seedream_steps: int = 50
    blend_method: str = 'laplacian'
    num_pyramid_levels: int = 6
    max_agents: int = 60
    max_concurrent: int = 30
    enable_qa: bool = True
    qa_device: str = 'cpu'
    volc_ak: str = ""
    volc_sk: str = ""
    volc_region: str = "cn-beijing"
    sr_scale: int = 2          # the reference hard-codes 2 (main.py:217,322)
    qa_map_cell: int = 0       # > 0 (with enable_qa): stage 4 also writes a per-cell quality map of this cell size
    qa_ms_ssim: bool = False   # (with enable_qa): stage 4 also reports the 5-scale MS-SSIM of the canvas against the INTER_CUBIC
                               # resize of the source ('ms_ssim_5scale'; the 'ms_ssim' key keeps the reference's single-scale value)
    qa_benchmark: bool = False # (with enable_qa): stage 4 also reports the SR-benchmark PSNR / SSIM (Y channel and RGB, a border of
                               # sr_scale pixels cropped) of the canvas against the INTER_CUBIC resize of the source ('sr_benchmark')
    qa_dists_weights: str = "" # (with enable_qa): path of DISTS weights (.npz: the VGG16 convolutions and alpha / beta): stage 4 also reports
                               # the DISTS of the canvas against the INTER_CUBIC resize of the source ('dists')
    qa_vif: bool = False       # (with enable_qa): stage 4 also reports the 4-scale pixel-domain VIF of the canvas against the INTER_CUBIC
                               # resize of the source (the reference), on the exact luma ('vifp', 'vifp_scales')
    qa_gmsd: bool = False      # (with enable_qa): ... and the gradient magnitude similarity deviation of the same pair ('gmsd')
    qa_fsim: bool = False      # (with enable_qa): ... and the phase-congruency feature similarity of the same pair ('fsim', 'fsimc')
    qa_vsi: bool = False       # (with enable_qa): ... and the visual saliency-induced index (SDSP saliency) of the same pair ('vsi')
    qa_delta_e: bool = False   # (with enable_qa): stage 4 also reports the per-pixel CIEDE2000 colour difference of the canvas against the
                               # INTER_CUBIC resize of the source ('delta_e'; with qa_map_cell > 0 also 'delta_e_map' over the same cells)
    qa_haarpsi: bool = False   # (with enable_qa): stage 4 also reports HaarPSI of the canvas against the INTER_CUBIC resize of the source
                               # ('haarpsi'; with qa_map_cell > 0 also 'haarpsi_map' over the same cells)
    qa_niqe_params: str = ""   # (with enable_qa): path of NIQE's pristine parameters (.npz with BasicSR's keys, or .mat): stage 4 also
                               # reports the NIQE of the canvas ('niqe_model'; the 'niqe' key keeps the reference's stand-in heuristic)
    qa_brisque_model: str = "" # (with enable_qa): path of a BRISQUE regressor (.npz: sv, sv_coef, gamma, rho, feature_min, feature_max): stage 4
                               # also reports the BRISQUE of the canvas ('brisque_model'; the 'brisque' key keeps the reference's stand-in)
    device_resident: bool = True   # with the built-in SR stub: source uploaded once, every stage on device pointers,
                                   # only the canvas comes back for the writer (a custom sr_backend gets host arrays)
    sr_weights: str = ""       # path of an SR network's weights (.npz, or .pth / .pt where torch imports): stage 2 runs the
                               # network (sr_network.load_network: compact, MSRResNet / EDSR, RRDBNet x4, RCAN, SwinIR, HAT or Swin2SR) instead of the
                               # bicubic stub, device-resident too (RCAN: each tile pools its channel means over itself; SwinIR: each
                               # tile is padded and windowed on its own)
    sr_act: str = "prelu"      # activation of a compact network whose weights hold no PReLU slopes: 'relu' or 'leakyrelu'
                               # (ignored for the residual family)
    sr_ensemble: int = 1       # (with sr_weights) geometric self-ensemble of the network: 1 off, 2 identity + horizontal flip, 4 the
                               # four flips, 8 all eight flips / rotations, averaged on the device (the "+" results of SR papers)
    benchmark_degrade: bool = False  # the input file is the GROUND TRUTH: it is mod-cropped to sr_scale and brought down by MATLAB's
                               # bicubic imresize(1 / sr_scale) on the GPU, that low-resolution image is the source of stages 1 - 3
                               # exactly as if it had been the input file, and stage 4 adds 'benchmark_hr': the SR-benchmark PSNR / SSIM
                               # of the canvas against the ground truth.  Device-resident path, built-in backends, one GPU only


@dataclass
class PipelineResult:
    """main.py:78-89."""
    success: bool
    output_path: Optional[str]
    processing_time: float
    total_blocks: int
    successful_blocks: int
    failed_blocks: int
    quality_score: Optional[float]
    quality_report: Optional[Dict[str, Any]]
    error_message: Optional[str]


def bicubic_stub_backend(pipeline: "SuperResolutionPipeline", tile: Tile, prompt: str) -> Optional[np.ndarray]:
    """SR stand-in: cv2.INTER_CUBIC-style upscale of the padded tile by sr_scale, on the GPU."""
    s = pipeline.config.sr_scale
    data = tile.data
    return pipeline.quality_module.upsample_bicubic(data, (data.shape[0] * s, data.shape[1] * s))


def compact_net_backend(pipeline: "SuperResolutionPipeline", tile: Tile, prompt: str) -> Optional[np.ndarray]:
    """Local SR: the compact network of PipelineConfig.sr_weights on the padded tile (host array in, host array out)."""
    return pipeline.sr_net.upscale(np.ascontiguousarray(tile.data), ensemble=pipeline.config.sr_ensemble)


class SuperResolutionPipeline:
    """tiling -> super-resolution -> blending -> quality assessment -> output."""

    def __init__(self, config: PipelineConfig, sr_backend: Optional[Callable] = None):
        self.config = config
        self.logger = logging.getLogger(self.__class__.__name__)
        self.tiling_module = TilingModule(block_size=config.block_size, overlap_ratio=config.overlap_ratio,
                                          padding_mode=config.padding_mode, output_scale=float(config.sr_scale))
        self.blending_module = BlendingModule(method=config.blend_method, num_levels=config.num_pyramid_levels)
        self.quality_module = QualityAssessmentModule(device=config.qa_device)
        self._niqe_params = None       # qa_niqe_params, read at the first use
        self._brisque_model = None     # qa_brisque_model, read at the first use
        self._dists_model = None       # qa_dists_weights, loaded at the first use
        self.sr_net = None
        if config.benchmark_degrade:
            import _launch
            if sr_backend is not None:
                raise ValueError("benchmark_degrade needs a built-in backend (the stub or sr_weights): a custom sr_backend gets host "
                                 "arrays, and the ground truth stays in HBM")
            if not config.device_resident:
                raise ValueError("benchmark_degrade runs on the device-resident path only (device_resident=False was asked for)")
            if _launch.dist_env()[1] > 1:
                raise ValueError("benchmark_degrade runs on one GPU: the sharded pipeline (WORLD_SIZE > 1) is out of its scope")
        if config.sr_ensemble != 1:
            from sr_network import ensemble_mask
            ensemble_mask(config.sr_ensemble)                                                # ValueError outside {1, 2, 4, 8}
            if not config.sr_weights:
                raise ValueError("sr_ensemble needs sr_weights: the bicubic stub has nothing to ensemble")
        if config.sr_weights and sr_backend is None:
            from sr_network import load_network
            self.sr_net = load_network(config.sr_weights, act=config.sr_act)                 # host work: no device call yet
            if self.sr_net.scale != config.sr_scale:
                raise ValueError(f"the network of {config.sr_weights} upscales by {self.sr_net.scale} but sr_scale is {config.sr_scale}")
            sr_backend = compact_net_backend
        self.sr_backend = sr_backend or bicubic_stub_backend
        self.sr_module = None
        self.scheduler = None

    async def __aenter__(self):
        return self

    async def __aexit__(self, exc_type, exc_val, exc_tb):
        return None

    def _calculate_target_size(self, original_size: tuple, target_resolution: str) -> tuple:
        """main.py:157-192 (the reference defines it but process() never applies it; kept for callers)."""
        width, height = original_size
        presets = {"100MP": 100, "150MP": 150, "200MP": 200}
        if target_resolution in presets:
            import _native
            return _native.target_size(int(width), int(height), presets[target_resolution])
        try:
            w, h = map(int, target_resolution.split('x'))
            return (w, h)
        except Exception:  # noqa: BLE001
            self.logger.warning("无法解析目标分辨率: %s，使用默认100MP", target_resolution)
            return (12245, 8163)

    def _builtin_backend(self) -> bool:
        """The SR stage is one of the pipeline's own GPU backends (stub or network): the device-resident paths apply."""
        return self.sr_backend is bicubic_stub_backend or (self.sr_net is not None and self.sr_backend is compact_net_backend)

    def _sr_tile_device(self, ctx, d_src: int, block: int, d_dst: int, dst_stride: int):
        """Stage 2 for one block x block x 3 tile, HBM -> HBM, on ctx's stream: the network, or the bicubic stand-in."""
        out_block = block * self.config.sr_scale
        if self.sr_net is not None:
            self.sr_net.upscale_device(d_src, (block, block, 3), d_dst, dst_stride, ctx=ctx, ensemble=self.config.sr_ensemble)
        else:
            ctx.resize_cubic_u8(d_src, block * 3, block, block, 3, d_dst, dst_stride, out_block, out_block)

    async def _process_single_tile(self, tile: Tile, prompt: str) -> Optional[np.ndarray]:
        try:
            return self.sr_backend(self, tile, prompt)
        except Exception as exc:  # noqa: BLE001 - a failed tile is dropped from the blend (main.py:221-223,310-325)
            self.logger.error("分块 %s 处理失败: %s", tile.metadata.block_id, exc)
            return None

    async def _parallel_upscale(self, tiles: List[Tile], prompt: str) -> List[Optional[np.ndarray]]:
        sem = asyncio.Semaphore(self.config.max_concurrent)

        async def limited(t: Tile):
            async with sem:
                return await self._process_single_tile(t, prompt)

        return list(await asyncio.gather(*[limited(t) for t in tiles]))

    def _write_outputs(self, fused: np.ndarray, output_path: str, report: Optional[Dict[str, Any]]):
        """Stage 5 (main.py:399-410): TIFF-LZW / PNG (compress_level 3) / JPEG-95 by extension + the QA report JSON.
        The reference calls Pillow's single-threaded writers; here the three formats are written by the native
        multi-threaded encoders behind the C ABI (sr_encode_*): same pixels back from any decoder."""
        import _native
        Path(output_path).parent.mkdir(parents=True, exist_ok=True)
        _native.write_image(fused, output_path, png_level=3, jpeg_quality=95)
        if report:
            with open(output_path.rsplit('.', 1)[0] + '_qa_report.json', 'w', encoding='utf-8') as f:
                json.dump(report, f, indent=2, ensure_ascii=False, default=str)

    def _ms_ssim(self, ctx, report: Dict[str, Any], d_src: int, src_shape, d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'ms_ssim_5scale' / 'ms_ssim_5scale_levels' entries (qa_ms_ssim): Wang's 5-scale MS-SSIM of the
        canvas against the INTER_CUBIC resize of the source to the canvas size, both in HBM.  A canvas below 176 pixels on a
        side has no fifth level: both entries are None and 'ms_ssim_5scale_note' says why (the run does not fail).  One helper
        for the device-resident, the host-array and the sharded path."""
        import _native
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        ih, iw = int(src_shape[0]), int(src_shape[1])
        try:
            _native.ms_ssim_plan(H, W, 5)
        except ValueError as exc:
            report['ms_ssim_5scale'], report['ms_ssim_5scale_levels'], report['ms_ssim_5scale_note'] = None, None, str(exc)
            return
        ref = ctx.alloc(H * W * cn)
        try:
            ctx.resize_cubic_u8(d_src, iw * cn, ih, iw, cn, ref.ptr, W * cn, H, W)
            v, lv = self.quality_module.calculate_ms_ssim_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn), levels=5,
                                                                 return_levels=True)
        finally:
            ctx.sync()
            ref.free()
        report['ms_ssim_5scale'], report['ms_ssim_5scale_levels'] = float(v), lv

    def _sr_benchmark(self, ctx, report: Dict[str, Any], d_src: int, src_shape, d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'sr_benchmark' entry (qa_benchmark): the PSNR / SSIM convention of the SR literature -- a border
        of sr_scale pixels cropped, on the BT.601 luma ('psnr_y', 'ssim_y') and on the RGB channels ('psnr_rgb', 'ssim_rgb') --
        of the canvas against the INTER_CUBIC resize of the source to the canvas size, both in HBM.  A canvas with a side
        below 11 after the crop has no SSIM window: the four values are None and 'sr_benchmark_note' says why (the run does
        not fail).  One helper for the device-resident, the host-array and the sharded path."""
        import _native
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        ih, iw = int(src_shape[0]), int(src_shape[1])
        cb = int(self.config.sr_scale)
        out = {'psnr_y': None, 'ssim_y': None, 'psnr_rgb': None, 'ssim_rgb': None, 'crop_border': cb}
        report['sr_benchmark'] = out
        try:
            _native.bench_plan(H, W, cn, cb, _native.BENCH_Y)
        except ValueError as exc:
            report['sr_benchmark_note'] = str(exc)
            return
        ref = ctx.alloc(H * W * cn)
        try:
            ctx.resize_cubic_u8(d_src, iw * cn, ih, iw, cn, ref.ptr, W * cn, H, W)
            q = self.quality_module
            y = q.evaluate_sr_benchmark_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn), crop_border=cb, test_y_channel=True)
            rgb = q.evaluate_sr_benchmark_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn), crop_border=cb, test_y_channel=False)
        finally:
            ctx.sync()
            ref.free()
        out.update(psnr_y=y['psnr'], ssim_y=y['ssim'], psnr_rgb=rgb['psnr'], ssim_rgb=rgb['ssim'])

    def _vif_gmsd(self, ctx, report: Dict[str, Any], d_src: int, src_shape, d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'vifp' / 'vifp_scales' (qa_vif) and 'gmsd' (qa_gmsd) entries: the 4-scale pixel-domain VIF and
        the gradient magnitude similarity deviation of the canvas against the INTER_CUBIC resize of the source to the canvas
        size (the reference), both in HBM, on the exact BT.601 luma, no crop.  A canvas too small (a side below 41 for VIF,
        below 4 for GMSD) or a NaN value (VIF of a flat reference; GMSD has none) gives None and 'vifp_note' / 'gmsd_note' says why (the run
        does not fail).  One helper for the device-resident, the host-array and the sharded path."""
        import _native
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        ih, iw = int(src_shape[0]), int(src_shape[1])
        todo = []
        if self.config.qa_vif:
            report['vifp'], report['vifp_scales'] = None, None
            try:
                _native.vif_plan(H, W, cn, 0, _native.BENCH_Y)
                todo.append('vif')
            except ValueError as exc:
                report['vifp_note'] = str(exc)
        if self.config.qa_gmsd:
            report['gmsd'] = None
            try:
                _native.gmsd_plan(H, W, cn, 0, _native.BENCH_Y)
                todo.append('gmsd')
            except ValueError as exc:
                report['gmsd_note'] = str(exc)
        if not todo:
            return
        ref = ctx.alloc(H * W * cn)
        try:
            ctx.resize_cubic_u8(d_src, iw * cn, ih, iw, cn, ref.ptr, W * cn, H, W)
            q = self.quality_module
            if 'vif' in todo:
                v, scales = q.calculate_vif_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn), return_scales=True)
                report['vifp_scales'] = [{'num': n, 'den': d, 'count': c} for n, d, c in scales]
                if v == v:
                    report['vifp'] = float(v)
                else:
                    report['vifp_note'] = "the reference is flat at every scale: VIF is 0 / 0"
            if 'gmsd' in todo:
                report['gmsd'] = float(q.calculate_gmsd_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn)))
        finally:
            ctx.sync()
            ref.free()

    def _fsim(self, ctx, report: Dict[str, Any], d_src: int, src_shape, d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'fsim' / 'fsimc' entries (qa_fsim): FSIM and FSIMc of the canvas against the INTER_CUBIC resize of
        the source to the canvas size, both in HBM.  A refusal of the plan (a side below 16, a pooled long side above 2048) or a
        NaN value (a flat pair) gives None for both and 'fsim_note' says why (the run does not fail).  Neither value enters
        overall_score.  One helper for the device-resident, the host-array and the sharded path."""
        import _native
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        ih, iw = int(src_shape[0]), int(src_shape[1])
        report['fsim'], report['fsimc'] = None, None
        try:
            _native.fsim_plan(H, W, cn)
        except (ValueError, _native.SrNativeError) as exc:
            report['fsim_note'] = str(exc)
            return
        ref = ctx.alloc(H * W * cn)
        try:
            ctx.resize_cubic_u8(d_src, iw * cn, ih, iw, cn, ref.ptr, W * cn, H, W)
            v = self.quality_module.calculate_fsim_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn))
            if v['fsim'] == v['fsim'] and v['fsimc'] == v['fsimc']:
                report['fsim'], report['fsimc'] = float(v['fsim']), float(v['fsimc'])
            else:
                report['fsim_note'] = "the pair is flat: FSIM is 0 / 0"
        finally:
            ctx.sync()
            ref.free()

    def _vsi(self, ctx, report: Dict[str, Any], d_src: int, src_shape, d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'vsi' entry (qa_vsi): VSI of the canvas against the INTER_CUBIC resize of the source to the canvas
        size, both in HBM.  A refusal of the plan (a side below 16, a gray image, F above 256) or a NaN value (a flat a or b
        plane, a constant saliency map) gives None and 'vsi_note' says why (the run does not fail).  The value does not enter
        overall_score.  One helper for the device-resident, the host-array and the sharded path."""
        import _native
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        ih, iw = int(src_shape[0]), int(src_shape[1])
        report['vsi'] = None
        try:
            _native.vsi_plan(H, W, cn)
        except (ValueError, _native.SrNativeError) as exc:
            report['vsi_note'] = str(exc)
            return
        ref = ctx.alloc(H * W * cn)
        try:
            ctx.resize_cubic_u8(d_src, iw * cn, ih, iw, cn, ref.ptr, W * cn, H, W)
            v = self.quality_module.calculate_vsi_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn))['vsi']
            if v == v:
                report['vsi'] = float(v)
            else:
                report['vsi_note'] = "the pair is flat in a, b or saliency: VSI is 0 / 0"
        finally:
            ctx.sync()
            ref.free()

    def _haarpsi(self, ctx, report: Dict[str, Any], d_src: int, src_shape, d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'haarpsi' entry (qa_haarpsi): HaarPSI (calculate_haarpsi's defaults, no crop) of the canvas
        against the INTER_CUBIC resize of the source to the canvas size, the reference, both in HBM -- and, with
        qa_map_cell > 0, 'haarpsi_map': its value over the uniform cells of report['quality_map'] (None for a cell without
        weight).  A refusal or a NaN (a black pair) gives None and 'haarpsi_note' says why (the run does not fail).  Takes no
        part in overall_score.  One helper for the device-resident, the host-array and the sharded path."""
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        ih, iw = int(src_shape[0]), int(src_shape[1])
        cell = int(self.config.qa_map_cell)
        report['haarpsi'] = None
        if cell > 0:
            report['haarpsi_map'] = None
        q = self.quality_module
        ref = None
        try:
            q._haarpsi_args("calculate_haarpsi", (H, W, cn), (H, W, cn), 0, True, 'matlab', None, None)
            ref = ctx.alloc(H * W * cn)
            ctx.resize_cubic_u8(d_src, iw * cn, ih, iw, cn, ref.ptr, W * cn, H, W)
            v = q.calculate_haarpsi_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn))
            if v != v:
                report['haarpsi_note'] = "HaarPSI is undefined for this pair: every weight is 0 (both images are black)"
            else:
                report['haarpsi'] = float(v)
            if cell > 0:
                m = q.evaluate_haarpsi_map_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn), cell=cell)
                report['haarpsi_map'] = {"cell": cell, "grid": [int(n) for n in m["haarpsi"].shape], "x_edges": m["x_edges"],
                                         "y_edges": m["y_edges"],
                                         "haarpsi": [[None if x != x else float(x) for x in r] for r in m["haarpsi"]]}
        except ValueError as exc:
            report['haarpsi_note'] = str(exc)
        finally:
            if ref is not None:
                ctx.sync()
                ref.free()

    def _delta_e(self, ctx, report: Dict[str, Any], d_src: int, src_shape, d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'delta_e' entry (qa_delta_e): the per-pixel CIEDE2000 colour difference of the canvas against
        the INTER_CUBIC resize of the source to the canvas size, both in HBM, no crop -- calculate_delta_e's dict -- and, with
        qa_map_cell > 0, 'delta_e_map': its mean and maximum over the uniform cells of report['quality_map'].  A refusal gives
        None and 'delta_e_note' says why (the run does not fail).  Takes no part in overall_score.  One helper for the
        device-resident, the host-array and the sharded path."""
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        ih, iw = int(src_shape[0]), int(src_shape[1])
        cell = int(self.config.qa_map_cell)
        report['delta_e'] = None
        if cell > 0:
            report['delta_e_map'] = None
        q = self.quality_module
        ref = None
        try:
            q._delta_e_args("calculate_delta_e", (H, W, cn), (H, W, cn), 0, 'ciede2000', None, None)
            ref = ctx.alloc(H * W * cn)
            ctx.resize_cubic_u8(d_src, iw * cn, ih, iw, cn, ref.ptr, W * cn, H, W)
            report['delta_e'] = q.calculate_delta_e_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn))
            if cell > 0:
                m = q.evaluate_delta_e_map_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn), cell=cell)
                report['delta_e_map'] = {"cell": cell, "grid": [int(v) for v in m["mean"].shape], "x_edges": m["x_edges"],
                                         "y_edges": m["y_edges"], "mean": [[float(v) for v in r] for r in m["mean"]],
                                         "max": [[float(v) for v in r] for r in m["max"]]}
        except ValueError as exc:
            report['delta_e_note'] = str(exc)
        finally:
            if ref is not None:
                ctx.sync()
                ref.free()

    def _degrade(self, ctx, hr: np.ndarray):
        """benchmark_degrade's stage 0: the ground truth goes up once and stays in HBM; its mod-crop to sr_scale (a view: the
        same address, the full stride) is brought down by MATLAB's bicubic imresize(1 / sr_scale) on the GPU, and the
        low-resolution image -- 1 / sr_scale^2 of the ground truth -- comes down once to feed split_array.
        -> (the device buffer of the ground truth, its row stride in bytes, the cropped shape, the low-resolution array)."""
        s = int(self.config.sr_scale)
        H, W = hr.shape[0] - hr.shape[0] % s, hr.shape[1] - hr.shape[1] % s
        if H < s or W < s:
            raise ValueError(f"benchmark_degrade: the image {hr.shape[:2]} is smaller than sr_scale {s}")
        d_hr, d_lr = ctx.upload(hr), None
        try:
            lh, lw = H // s, W // s
            d_lr = ctx.alloc(lh * lw * 3)
            shape = self.quality_module.imresize_device(d_hr.ptr, (H, W, 3), d_lr.ptr, scale=1.0 / s, src_stride=hr.shape[1] * 3)
            if shape != (lh, lw, 3):
                raise ValueError(f"benchmark_degrade: imresize gave {shape}, not {(lh, lw, 3)}")
            lr = ctx.download(d_lr.ptr, (lh, lw, 3), np.uint8)
        except Exception:
            d_hr.free()
            raise
        finally:
            if d_lr is not None:
                d_lr.free()
        return d_hr, hr.shape[1] * 3, (H, W, 3), lr

    def _benchmark_hr(self, ctx, report: Dict[str, Any], d_hr: int, hr_stride: int, d_canvas: int, canvas_shape, lr_shape) -> None:
        """Stage 4's 'benchmark_hr' entry (benchmark_degrade): the SR-benchmark PSNR / SSIM -- a border of sr_scale pixels
        cropped, on the BT.601 luma and on the RGB channels -- of the canvas against the mod-cropped ground truth, both in
        HBM: the keys of QualityAssessmentModule.evaluate_sr_network.  A side below 11 after the crop has no SSIM window:
        the entry is None and 'benchmark_hr_note' says why (the run does not fail)."""
        import _native
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        cb = int(self.config.sr_scale)
        try:
            _native.bench_plan(H, W, cn, cb, _native.BENCH_Y)
        except ValueError as exc:
            report['benchmark_hr'], report['benchmark_hr_note'] = None, str(exc)
            return
        out = {}
        try:
            for key, mode in (("y", _native.BENCH_Y), ("rgb", _native.BENCH_CHANNELS)):
                sums = ctx.bench_u8(d_canvas, W * cn, d_hr, hr_stride, H, W, cn, crop_border=cb, mode=mode, data_range=255.0)
                out["psnr_" + key], out["ssim_" + key] = _native.bench_values(sums, 255.0)
        finally:
            ctx.sync()
        out.update(crop_border=cb, scale=cb, hr_shape=[H, W, cn], lr_shape=[int(v) for v in lr_shape])
        report['benchmark_hr'] = out

    def _dists(self, ctx, report: Dict[str, Any], d_src: int, src_shape, d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'dists' entry (qa_dists_weights): DISTS of the canvas against the INTER_CUBIC resize of the
        source to the canvas size (the pair of 'sr_benchmark'), both in HBM, under the weights of the configured file.  One
        helper for the device-resident, the host-array and the sharded path."""
        import _native
        if self._dists_model is None:
            self._dists_model = _native.DistsModel(ctx, _native.load_dists_weights(self.config.qa_dists_weights))
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        ih, iw = int(src_shape[0]), int(src_shape[1])
        ref = ctx.alloc(H * W * cn)
        try:
            ctx.resize_cubic_u8(d_src, iw * cn, ih, iw, cn, ref.ptr, W * cn, H, W)
            report['dists'] = float(self._dists_model.value(ref.ptr, W * cn, d_canvas, W * cn, H, W, cn,
                                                            tile=self.quality_module.dists_tile))
        finally:
            ctx.sync()
            ref.free()

    def _niqe_model(self, ctx, report: Dict[str, Any], d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'niqe_model' entry (qa_niqe_params): the NIQE of the canvas in HBM (no crop) under the pristine
        parameters of the configured file.  Not the 'niqe' key of the commercial section, which is the reference's MSCN
        stand-in.  A canvas with a side below 96, or with fewer than two blocks free of NaN features, has no score: the entry
        is None and 'niqe_model_note' says why (the run does not fail).  One helper for the device-resident, the host-array
        and the sharded path."""
        import quality_assessment_module as qam
        if self._niqe_params is None:
            self._niqe_params = qam.load_niqe_params(self.config.qa_niqe_params)
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        try:
            report['niqe_model'] = float(self.quality_module.calculate_niqe_model_device(d_canvas, (H, W, cn), self._niqe_params))
        except ValueError as exc:
            report['niqe_model'], report['niqe_model_note'] = None, str(exc)
        finally:
            ctx.sync()

    def _brisque_model_entry(self, ctx, report: Dict[str, Any], d_canvas: int, canvas_shape) -> None:
        """Stage 4's optional 'brisque_model' entry (qa_brisque_model): the BRISQUE of the canvas in HBM (no crop) under the
        regressor of the configured file.  Not the 'brisque' key of the commercial section, which is the reference's
        stand-in.  A canvas with a side below 16, or with a NaN feature, has no score: the entry is None and
        'brisque_model_note' says why (the run does not fail).  One helper for the device-resident, the host-array and the
        sharded path."""
        import quality_assessment_module as qam
        if self._brisque_model is None:
            self._brisque_model = qam.load_brisque_model(self.config.qa_brisque_model)
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        try:
            report['brisque_model'] = float(self.quality_module.calculate_brisque_model_device(d_canvas, (H, W, cn), self._brisque_model))
        except ValueError as exc:
            report['brisque_model'], report['brisque_model_note'] = None, str(exc)
        finally:
            ctx.sync()

    def _quality_map(self, ctx, d_src: int, src_shape, d_canvas: int, canvas_shape, tiles: List[Tile],
                     output_path: str) -> Dict[str, Any]:
        """Stage 4's optional 'quality_map' section (qa_map_cell > 0): where the canvas differs from the INTER_CUBIC resize
        of the source to the canvas size -- per uniform cell of qa_map_cell pixels and per tile (its ownership region,
        tile_cell_edges).  Both images are in HBM; the resize goes into a temporary.  Also writes <name>_qa_map.png, a
        gh x gw gray image of floor(255 * clip(ms_ssim, 0, 1)) (0 for a cell without a valid sample).  One helper for the
        device-resident, the host-array and the sharded path."""
        import _native
        from tiling_module import tile_cell_edges
        qm = self.quality_module
        H, W, cn = int(canvas_shape[0]), int(canvas_shape[1]), int(canvas_shape[2])
        ih, iw = int(src_shape[0]), int(src_shape[1])
        ref = ctx.alloc(H * W * cn)
        try:
            ctx.resize_cubic_u8(d_src, iw * cn, ih, iw, cn, ref.ptr, W * cn, H, W)
            m = qm.evaluate_quality_map_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn), cell=int(self.config.qa_map_cell))
            try:
                pos = [(t.metadata.global_x, t.metadata.global_y, 0, 0) for t in tiles]
                xe, ye = tile_cell_edges(pos, self.tiling_module.overlap_pixels, self.config.sr_scale, W, H)
                t = qm.evaluate_quality_map_device(ref.ptr, (H, W, cn), d_canvas, (H, W, cn), x_edges=xe, y_edges=ye)
            except ValueError as exc:
                t, tiles_section = None, {"available": False, "note": str(exc)}
        finally:
            ctx.sync()
            ref.free()

        def num(v):
            v = float(v)
            return None if v != v else v

        def rows(a):
            return [[num(v) for v in r] for r in a]

        def rect(mm, gy, gx):
            x0, y0 = mm["x_edges"][gx], mm["y_edges"][gy]
            return [x0, y0, mm["x_edges"][gx + 1] - x0, mm["y_edges"][gy + 1] - y0]

        gh, gw = m["ms_ssim"].shape
        ms = m["ms_ssim"]
        order = [i for i in np.argsort(np.where(np.isnan(ms), np.inf, ms), axis=None, kind="stable") if not np.isnan(ms.flat[i])]
        worst = [{"gy": int(i // gw), "gx": int(i % gw), "rect": rect(m, int(i // gw), int(i % gw)),
                  "ms_ssim": num(ms.flat[i]), "ssim": num(m["ssim"].flat[i]), "psnr": num(m["psnr"].flat[i])} for i in order[:5]]
        if t is not None:
            ncol = len(t["x_edges"]) - 1
            col = {x: c for c, x in enumerate(sorted({p[0] for p in pos}))}
            row = {y: r for r, y in enumerate(sorted({p[1] for p in pos}))}
            tiles_section = []
            for i, p in enumerate(pos):                                # list order = the order of split_image's tiles
                gy, gx = row[p[1]], col[p[0]]
                tiles_section.append({"index": i, "row": gy, "col": gx, "rect": rect(t, gy, gx),
                                      "psnr": num(t["psnr"][gy, gx]), "ssim": num(t["ssim"][gy, gx]),
                                      "ms_ssim": num(t["ms_ssim"][gy, gx])})
            assert len(tiles_section) == ncol * (len(t["y_edges"]) - 1)
        png = output_path.rsplit('.', 1)[0] + '_qa_map.png'
        Path(png).parent.mkdir(parents=True, exist_ok=True)
        gray = np.floor(255.0 * np.clip(np.nan_to_num(ms, nan=0.0), 0.0, 1.0)).astype(np.uint8)
        _native.write_image(gray, png, png_level=3)
        return {"cell": int(self.config.qa_map_cell), "grid": [int(gh), int(gw)], "x_edges": m["x_edges"], "y_edges": m["y_edges"],
                "sse": [[int(v) for v in r] for r in m["sse"]], "psnr": rows(m["psnr"]), "ssim": rows(m["ssim"]),
                "ms_ssim": rows(ms), "worst_cells": worst, "image": os.path.basename(png), "tiles": tiles_section}

    @staticmethod
    def _commercial(evaluate) -> Dict[str, Any]:
        """Stage 4's commercial section (main.py:369-386 of the reference); a canvas with a side beyond the hand-written
        DFT (sr_fft_max_len) gets a labelled stub instead of failing the image."""
        try:
            return evaluate()
        except NotImplementedError as exc:
            return {"available": False, "note": str(exc)}

    async def _process_device(self, input_path: str, output_path: str, roi_regions, start: float) -> PipelineResult:
        """The five stages with the data resident in HBM (main.py:293-410 order): the decoded source goes up once
        (the only large H2D), tiles are cut and padded, the bicubic SR stand-in runs per tile, the tiles are fused and
        the canvas assessed against the source -- all on device addresses -- and only the finished canvas comes down
        (the only large D2H) for the writer.  Same arithmetic as the host-array path, so the same results."""
        from tiling_module import _load_rgb
        tm, s = self.tiling_module, self.config.sr_scale
        self.transfers = None
        st = self.stage_times = {}
        t_mark = time.perf_counter()

        def lap(name):
            nonlocal t_mark
            ctx.sync()
            now = time.perf_counter()
            st[name] = now - t_mark
            t_mark = now

        original = _load_rgb(input_path)
        ctx = self.quality_module._ctx()
        h2d0, d2h0 = ctx.h2d_bytes, ctx.d2h_bytes
        lap("decode")
        d_hr = None
        if self.config.benchmark_degrade:
            # the file is the ground truth: from here on `original` is its imresize(1 / s), as if that had been the input file
            d_hr, hr_stride, hr_shape, original = self._degrade(ctx, original)
            lap("degrade")
        ih, iw = original.shape[:2]
        sr_bufs, canvas = [], None
        try:
            # Stage 1: tiling (metadata on the host, pixels stay on the GPU)
            tiles = tm.split_array(original, image_hash=tm._compute_image_hash(input_path), image_path=input_path,
                                   device_resident=True)
            ts = tm.device_tiles
            block, out_block = tm.block_size, tm.block_size * s
            lap("upload+tile")
            # Stage 2: SR (the network, or the bicubic stand-in), tile by tile, HBM -> HBM
            for i in range(len(tiles)):
                buf = ctx.alloc(out_block * out_block * 3)
                sr_bufs.append(buf)
                self._sr_tile_device(ctx, ts.tile_ptr(i), block, buf.ptr, out_block * 3)
            lap("sr_net" if self.sr_net is not None else "sr_stub")
            # Stage 3: blending (the canvas is cropped to the un-padded image, scaled)
            rects = [(t.metadata.global_x * s, t.metadata.global_y * s, out_block, out_block) for t in tiles]
            H, W = ih * s, iw * s
            canvas = self.blending_module.fuse_device([b.ptr for b in sr_bufs], [out_block * 3] * len(tiles), rects, (H, W), 3,
                                                      laplacian=self.config.blend_method != 'weighted')
            lap("blend")
            # Stage 4: quality assessment, source (still resident from stage 1) vs canvas
            report, score = None, None
            if self.config.enable_qa:
                qa = self.quality_module.evaluate_full_reference_device(ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3),
                                                                        scale_factor=W / iw)
                report = {'full_reference': qa,
                          'commercial': self._commercial(lambda: self.quality_module.evaluate_commercial_device(
                              canvas.ptr, (H, W, 3), roi_regions or [])),
                          'timestamp': datetime.now().isoformat()}
                if self.config.qa_map_cell > 0:
                    report['quality_map'] = self._quality_map(ctx, ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3), tiles, output_path)
                if self.config.qa_ms_ssim:
                    self._ms_ssim(ctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3))
                if self.config.qa_benchmark:
                    self._sr_benchmark(ctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3))
                if self.config.qa_vif or self.config.qa_gmsd:
                    self._vif_gmsd(ctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3))
                if self.config.qa_delta_e:
                    self._delta_e(ctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3))
                if self.config.qa_haarpsi:
                    self._haarpsi(ctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3))
                if self.config.qa_fsim:
                    self._fsim(ctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3))
                if self.config.qa_vsi:
                    self._vsi(ctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3))
                if self.config.qa_niqe_params:
                    self._niqe_model(ctx, report, canvas.ptr, (H, W, 3))
                if self.config.qa_brisque_model:
                    self._brisque_model_entry(ctx, report, canvas.ptr, (H, W, 3))
                if self.config.qa_dists_weights:
                    self._dists(ctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.ptr, (H, W, 3))
                if d_hr is not None:
                    assert hr_shape == (H, W, 3)
                    self._benchmark_hr(ctx, report, d_hr.ptr, hr_stride, canvas.ptr, (H, W, 3), (ih, iw, 3))
                score = qa.get('overall_score', 0)
            lap("assess")
            # Stage 5: the one download, then the writer
            fused = ctx.download(canvas.ptr, (H, W, 3), np.uint8)
            lap("download")
        finally:
            ctx.sync()
            for b in sr_bufs + ([canvas] if canvas is not None else []) + ([d_hr] if d_hr is not None else []):
                b.free()
            tm.release_device_tiles()
        self.transfers = {"h2d_bytes": ctx.h2d_bytes - h2d0, "d2h_bytes": ctx.d2h_bytes - d2h0,
                          "source_bytes": int(original.nbytes), "canvas_bytes": int(fused.nbytes)}
        self._write_outputs(fused, output_path, report)
        st["write"] = time.perf_counter() - t_mark
        return PipelineResult(True, output_path, time.time() - start, len(tiles), len(tiles), 0, score, report, None)

    async def _process_sharded(self, input_path: str, output_path: str, roi_regions, start: float, rank: int, world: int,
                               local_rank: int) -> PipelineResult:
        """process() on ``world`` GPUs, this process being rank ``rank`` (main.py:269-441 stage order; the fan-out the
        reference does with ParallelBlender's threads, blending_module.py:1665-1705, is one process per GPU here).
          stage 1  every rank decodes the source and cuts the (input-space) tiles -- the source is the small image;
          stage 2  the SR stand-in runs for the tiles this rank OWNS (owners chosen by the exchange planner), straight
                   into the buffers the exchange sends from;
          stage 3  the canvas is split into horizontal strips; every strip owner receives the tile rows (+ pyramid halo)
                   it needs -- one grouped batch of point-to-point transfers (RCCL over xGMI; gloo in the rehearsal) --
                   and blends its rows with the kernels of the one-GPU path: bit-identical rows;
          stage 4/5  the strips are gathered on rank 0, which assesses (same calls as the one-GPU path) and writes.
        Every rank returns the same result record (rank 0's, broadcast)."""
        import torch
        import torch.distributed as dist
        import _launch
        import device_pipeline as dp
        from tiling_module import _load_rgb
        backend = os.environ.get("SR_DIST_BACKEND", "nccl")
        ndev = max(torch.cuda.device_count(), 1)
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible -- the HIP path has no CPU fallback")
        dev_index = local_rank if backend == "nccl" else local_rank % ndev    # gloo: the one-GPU rehearsal shares a card
        torch.cuda.set_device(dev_index)
        _launch.stage("GPU visible")
        created = False
        if not dist.is_initialized():
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if backend == "nccl":
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", dev_index))
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)
            created = True
        _launch.stage(f"process group ({backend}, world {world}) initialised")
        pipe = None
        tm, s = self.tiling_module, self.config.sr_scale
        try:
            tm.device = self.blending_module.device = dev_index
            self.quality_module.gpu_index = dev_index
            original = _load_rgb(input_path)
            ih, iw = original.shape[:2]
            # stage 1: tiling (every rank; metadata on the host, pixels on this rank's GPU)
            tiles = tm.split_array(original, image_hash=tm._compute_image_hash(input_path), image_path=input_path,
                                   device_resident=True)
            ts = tm.device_tiles
            block, out_block = tm.block_size, tm.block_size * s
            rects = [(t.metadata.global_x * s, t.metadata.global_y * s, out_block, out_block) for t in tiles]
            H, W = ih * s, iw * s
            geo = dp.Geometry(W, H, rects, 3, self.config.num_pyramid_levels, "cosine")
            pipe = dp.DevicePipeline(geo, rank, world, dev_index)
            self.shard_info = {"rank": rank, "world": world, "owned_tiles": list(pipe.owned), "strip": list(pipe.strip),
                               "bytes_received": pipe.xplan.bytes_received(rank, geo)}
            tm._ctx().sync()                                  # the tiles were cut on the module's stream
            _launch.stage("tiles cut")
            # stage 2: the SR stand-in for the tiles this rank owns, into the buffers the exchange sends from
            for t in pipe.owned:
                buf = pipe.local_tiles[t]
                self._sr_tile_device(pipe.ctx, ts.tile_ptr(t), block, buf.data_ptr(), buf.stride(0))
            # stage 3: rows to the strip owners, strip blend
            pending = pipe.stage_exchange(0)
            pipe.stage_blend(pending)
            _launch.stage("strip blended")
            canvas = pipe.gather_canvas(dst=0)
            _launch.stage("canvas gathered")
            result = None
            if rank == 0:
                report, score = None, None
                qctx = self.quality_module._ctx()
                if self.config.enable_qa:
                    qa = self.quality_module.evaluate_full_reference_device(ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3),
                                                                            scale_factor=W / iw)
                    report = {'full_reference': qa,
                              'commercial': self._commercial(lambda: self.quality_module.evaluate_commercial_device(
                                  canvas.data_ptr(), (H, W, 3), roi_regions or [])),
                              'timestamp': datetime.now().isoformat()}
                    if self.config.qa_map_cell > 0:
                        report['quality_map'] = self._quality_map(qctx, ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3),
                                                                  tiles, output_path)
                    if self.config.qa_ms_ssim:
                        self._ms_ssim(qctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3))
                    if self.config.qa_benchmark:
                        self._sr_benchmark(qctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3))
                    if self.config.qa_vif or self.config.qa_gmsd:
                        self._vif_gmsd(qctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3))
                    if self.config.qa_delta_e:
                        self._delta_e(qctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3))
                    if self.config.qa_haarpsi:
                        self._haarpsi(qctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3))
                    if self.config.qa_fsim:
                        self._fsim(qctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3))
                    if self.config.qa_vsi:
                        self._vsi(qctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3))
                    if self.config.qa_niqe_params:
                        self._niqe_model(qctx, report, canvas.data_ptr(), (H, W, 3))
                    if self.config.qa_brisque_model:
                        self._brisque_model_entry(qctx, report, canvas.data_ptr(), (H, W, 3))
                    if self.config.qa_dists_weights:
                        self._dists(qctx, report, ts.d_img.ptr, (ih, iw, 3), canvas.data_ptr(), (H, W, 3))
                    score = qa.get('overall_score', 0)
                fused = qctx.download(canvas.data_ptr(), (H, W, 3), np.uint8)
                self._write_outputs(fused, output_path, report)
                result = PipelineResult(True, output_path, time.time() - start, len(tiles), len(tiles), 0, score, report, None)
            box = [result]
            dist.broadcast_object_list(box, src=0)
            _launch.stage("result broadcast")
            return box[0]
        finally:
            torch.cuda.synchronize()
            if pipe is not None:
                pipe.close()
            tm.release_device_tiles()
            if created:
                dist.destroy_process_group()

    async def process(self, input_path: str, output_path: str, prompt: str = "",
                      roi_regions: Optional[List[Dict]] = None) -> PipelineResult:
        start = time.time()
        import _launch
        rank, world, local_rank = _launch.dist_env()
        if (world > 1 and self.config.device_resident and self._builtin_backend()
                and self.config.blend_method != 'weighted'):
            try:
                return await self._process_sharded(input_path, output_path, roi_regions, start, rank, world, local_rank)
            except Exception as exc:  # noqa: BLE001 - the reference reports every failure in the result record
                self.logger.error("Pipeline执行失败: %s", exc, exc_info=True)
                return PipelineResult(False, None, time.time() - start, 0, 0, 0, None, None, str(exc))
        if world > 1 and rank != 0:
            # what does not shard (a custom SR backend hands host arrays around; the weighted blend has no strip form): rank 0
            # runs the one-GPU path, the others have nothing to do
            return PipelineResult(True, None, time.time() - start, 0, 0, 0, None, None, None)
        if self.config.device_resident and self._builtin_backend():
            try:
                return await self._process_device(input_path, output_path, roi_regions, start)
            except Exception as exc:  # noqa: BLE001 - the reference reports every failure in the result record
                self.logger.error("Pipeline执行失败: %s", exc, exc_info=True)
                return PipelineResult(False, None, time.time() - start, 0, 0, 0, None, None, str(exc))
        try:
            # Stage 1: tiling
            tiles = self.tiling_module.split_image(input_path)
            # Stage 2: super-resolution of every tile
            results = await self._parallel_upscale(tiles, prompt)
            ok = [r for r in results if r is not None]
            failed = len(results) - len(ok)
            if not ok:
                raise RuntimeError("所有分块处理失败")
            s = self.config.sr_scale
            step = self.tiling_module.block_size - self.tiling_module.overlap_pixels
            infos = []
            for tile, res in zip(tiles, results):
                if res is not None:
                    m = tile.metadata
                    infos.append(TileInfo(res, m.global_x * s, m.global_y * s, m.global_y // step, m.global_x // step))
            # Stage 3: blending (the canvas is cropped to the un-padded image, scaled)
            from PIL import Image
            with Image.open(input_path) as im:
                iw, ih = im.size
                original = np.asarray(im.convert("RGB"), dtype=np.uint8)
            out_shape = (ih * s, iw * s)
            if self.config.blend_method == 'weighted':
                fused = self.blending_module.weighted_average_fusion(infos, output_shape=out_shape)
            else:
                fused = self.blending_module.laplacian_fusion(infos, None, output_shape=out_shape)
            # Stage 4: quality assessment
            report, score = None, None
            if self.config.enable_qa:
                qa = self.quality_module.evaluate_full_reference(original=original, upscaled=fused,
                                                                 scale_factor=fused.shape[1] / original.shape[1])
                report = {'full_reference': qa,
                          'commercial': self._commercial(lambda: self.quality_module.evaluate_commercial(fused, roi_regions or [])),
                          'timestamp': datetime.now().isoformat()}
                if self.config.qa_map_cell > 0:
                    qctx = self.quality_module._ctx()
                    d_src, d_fused = qctx.upload(original), qctx.upload(fused)
                    try:
                        report['quality_map'] = self._quality_map(qctx, d_src.ptr, original.shape, d_fused.ptr, fused.shape,
                                                                  tiles, output_path)
                    finally:
                        d_src.free(); d_fused.free()
                if self.config.qa_ms_ssim:
                    qctx = self.quality_module._ctx()
                    d_src, d_fused = qctx.upload(original), qctx.upload(fused)
                    try:
                        self._ms_ssim(qctx, report, d_src.ptr, original.shape, d_fused.ptr, fused.shape)
                    finally:
                        d_src.free(); d_fused.free()
                if self.config.qa_benchmark:
                    qctx = self.quality_module._ctx()
                    d_src, d_fused = qctx.upload(original), qctx.upload(fused)
                    try:
                        self._sr_benchmark(qctx, report, d_src.ptr, original.shape, d_fused.ptr, fused.shape)
                    finally:
                        d_src.free(); d_fused.free()
                if self.config.qa_vif or self.config.qa_gmsd:
                    qctx = self.quality_module._ctx()
                    d_src, d_fused = qctx.upload(original), qctx.upload(fused)
                    try:
                        self._vif_gmsd(qctx, report, d_src.ptr, original.shape, d_fused.ptr, fused.shape)
                    finally:
                        d_src.free(); d_fused.free()
                if self.config.qa_delta_e:
                    qctx = self.quality_module._ctx()
                    d_src, d_fused = qctx.upload(original), qctx.upload(fused)
                    try:
                        self._delta_e(qctx, report, d_src.ptr, original.shape, d_fused.ptr, fused.shape)
                    finally:
                        d_src.free(); d_fused.free()
                if self.config.qa_haarpsi:
                    qctx = self.quality_module._ctx()
                    d_src, d_fused = qctx.upload(original), qctx.upload(fused)
                    try:
                        self._haarpsi(qctx, report, d_src.ptr, original.shape, d_fused.ptr, fused.shape)
                    finally:
                        d_src.free(); d_fused.free()
                if self.config.qa_fsim:
                    qctx = self.quality_module._ctx()
                    d_src, d_fused = qctx.upload(original), qctx.upload(fused)
                    try:
                        self._fsim(qctx, report, d_src.ptr, original.shape, d_fused.ptr, fused.shape)
                    finally:
                        d_src.free(); d_fused.free()
                if self.config.qa_vsi:
                    qctx = self.quality_module._ctx()
                    d_src, d_fused = qctx.upload(original), qctx.upload(fused)
                    try:
                        self._vsi(qctx, report, d_src.ptr, original.shape, d_fused.ptr, fused.shape)
                    finally:
                        d_src.free(); d_fused.free()
                if self.config.qa_niqe_params:
                    qctx = self.quality_module._ctx()
                    d_fused = qctx.upload(fused)
                    try:
                        self._niqe_model(qctx, report, d_fused.ptr, fused.shape)
                    finally:
                        d_fused.free()
                if self.config.qa_brisque_model:
                    qctx = self.quality_module._ctx()
                    d_fused = qctx.upload(fused)
                    try:
                        self._brisque_model_entry(qctx, report, d_fused.ptr, fused.shape)
                    finally:
                        d_fused.free()
                if self.config.qa_dists_weights:
                    qctx = self.quality_module._ctx()
                    d_src, d_fused = qctx.upload(original), qctx.upload(fused)
                    try:
                        self._dists(qctx, report, d_src.ptr, original.shape, d_fused.ptr, fused.shape)
                    finally:
                        d_src.free(); d_fused.free()
                score = qa.get('overall_score', 0)
            # Stage 5: output
            self._write_outputs(fused, output_path, report)
            return PipelineResult(True, output_path, time.time() - start, len(tiles), len(ok), failed, score, report, None)
        except Exception as exc:  # noqa: BLE001 - the reference reports every failure in the result record
            self.logger.error("Pipeline执行失败: %s", exc, exc_info=True)
            return PipelineResult(False, None, time.time() - start, 0, 0, 0, None, None, str(exc))


def shard_plan(image_size, config: PipelineConfig, world: int) -> Dict[str, Any]:
    """Host only: what process() on ``world`` ranks will do with an image of ``image_size`` (w, h) -- the output-space tile
    rectangles, the strip of every rank, the owner of every tile and the bytes every rank receives.  (The planner is host
    code of the C ABI, so this runs without a GPU.)"""
    import device_pipeline as dp
    tm = TilingModule(block_size=config.block_size, overlap_ratio=config.overlap_ratio, padding_mode=config.padding_mode,
                      output_scale=float(config.sr_scale))
    iw, ih = image_size
    s, out_block = config.sr_scale, config.block_size * config.sr_scale
    rects = [(x * s, y * s, out_block, out_block) for (x, y, _, _) in tm._calculate_tile_positions(iw, ih)]
    geo = dp.Geometry(iw * s, ih * s, rects, 3, config.num_pyramid_levels, "cosine")
    xp = dp.make_exchange_plan(geo, world)
    return {"canvas": [iw * s, ih * s], "rects": rects, "bounds": list(xp.bounds), "owners": list(xp.owners),
            "rows": [list(r) for r in xp.rows], "bytes_received": [xp.bytes_received(r, geo) for r in range(world)]}


async def main() -> int:
    import argparse
    ap = argparse.ArgumentParser(description="tile -> bicubic-stub SR -> Laplacian blend -> QA on MI355X GPUs")
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--block-size", type=int, default=2048)
    ap.add_argument("--sr-scale", type=int, default=2)
    ap.add_argument("--sr-weights", default="", metavar="PATH",
                    help="weights of an SR network (.npz / .pth: compact, MSRResNet / EDSR, RCAN, SwinIR, or RRDBNet x4 with --sr-scale 4): stage 2 runs it "
                         "instead of the bicubic stub")
    ap.add_argument("--sr-act", default="prelu", metavar="NAME", help="prelu (slopes in the weights), relu or leakyrelu")
    ap.add_argument("--sr-ensemble", type=int, choices=(1, 2, 4, 8), default=1,
                    help="with --sr-weights: geometric self-ensemble of the network over 2 (identity + horizontal flip), 4 (the four "
                         "flips) or 8 (all flips and rotations) members, averaged on the GPU; 1 = off")
    ap.add_argument("--qa-ms-ssim", action="store_true",
                    help="stage 4 also reports Wang's 5-scale MS-SSIM of the result against the bicubic resize of the input "
                         "(report key ms_ssim_5scale)")
    ap.add_argument("--qa-benchmark", action="store_true",
                    help="stage 4 also reports the SR-benchmark PSNR / SSIM (Y channel and RGB, a border of --sr-scale pixels "
                         "cropped) of the result against the bicubic resize of the input (report key sr_benchmark)")
    ap.add_argument("--qa-vif", action="store_true",
                    help="stage 4 also reports the 4-scale pixel-domain VIF (vifp_mscale) of the result against the bicubic resize "
                         "of the input, which is the reference (report keys vifp, vifp_scales)")
    ap.add_argument("--qa-fsim", action="store_true",
                    help="stage 4 also reports FSIM and FSIMc (phase-congruency feature similarity) of the result against the "
                         "bicubic resize of the input (report keys fsim, fsimc)")
    ap.add_argument("--qa-gmsd", action="store_true",
                    help="stage 4 also reports the gradient magnitude similarity deviation of the result against the bicubic "
                         "resize of the input (report key gmsd)")
    ap.add_argument("--qa-vsi", action="store_true",
                    help="stage 4 also reports VSI (visual saliency-induced index, SDSP saliency) of the result against the "
                         "bicubic resize of the input (report key vsi)")
    ap.add_argument("--qa-delta-e", action="store_true",
                    help="stage 4 also reports the per-pixel CIEDE2000 colour difference of the result against the bicubic resize "
                         "of the input (report key delta_e; with --qa-map-cell also delta_e_map over the same cells)")
    ap.add_argument("--qa-haarpsi", action="store_true",
                    help="stage 4 also reports HaarPSI (Haar wavelet perceptual similarity) of the result against the bicubic resize "
                         "of the input (report key haarpsi; with --qa-map-cell also haarpsi_map over the same cells)")
    ap.add_argument("--qa-map-cell", type=int, default=0, metavar="N",
                    help="N > 0: stage 4 also writes the per-cell PSNR / SSIM map over uniform cells of N pixels (report key "
                         "quality_map, PipelineConfig.qa_map_cell); 0 = off")
    ap.add_argument("--qa-niqe-params", default="", metavar="PATH",
                    help="NIQE's pristine parameters (.npz with the keys mu_pris_param / cov_pris_param, or .mat): stage 4 also "
                         "reports the NIQE of the result (report key niqe_model; the key niqe stays the stand-in heuristic)")
    ap.add_argument("--qa-brisque-model", default="", metavar="PATH",
                    help="a BRISQUE regressor (.npz with the keys sv, sv_coef, gamma, rho, feature_min, feature_max): stage 4 also "
                         "reports the BRISQUE of the result (report key brisque_model; the key brisque stays the stand-in heuristic)")
    ap.add_argument("--qa-dists-weights", default="", metavar="PATH",
                    help="DISTS weights (.npz with the VGG16 convolutions stageN.K.weight / .bias, or features.K.*, and alpha / "
                         "beta): stage 4 also reports the DISTS of the result against the bicubic resize of the input (report "
                         "key dists)")
    ap.add_argument("--benchmark-degrade", action="store_true",
                    help="the input is the ground truth: it is mod-cropped to --sr-scale, brought down by MATLAB's bicubic "
                         "imresize(1 / scale) on the GPU, upscaled, and stage 4 also reports the SR-benchmark PSNR / SSIM of the "
                         "result against the input (report key benchmark_hr); one GPU only")
    ap.add_argument("--gpus", type=int, default=1, help="GPUs of this node to use: N > 1 starts one process per GPU (RCCL)")
    ap.add_argument("--deadline-s", type=float, default=1800.0,
                    help="--gpus N: ranks still running after this many seconds are terminated (status 124)")
    ap.add_argument("--plan-only", action="store_true",
                    help="no GPU work: every rank computes the shard plan of the input, the ranks compare them over the "
                         "process group and rank 0 prints it as one JSON line")
    args = ap.parse_args()
    import _launch
    if args.gpus < 1:
        print("main.py: --gpus must be >= 1", file=sys.stderr)
        return 2
    if args.benchmark_degrade and args.gpus > 1:
        print("main.py: --benchmark-degrade runs on one GPU (--gpus 1)", file=sys.stderr)
        return 2
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # children only: this process never touches torch or the GPU (and nothing that has is ever exec'ed)
        return _launch.launch_ranks(args.gpus, os.path.abspath(__file__), sys.argv[1:], args.deadline_s, who="main.py")
    rank, world, _ = _launch.dist_env()
    if world != args.gpus:
        print(f"main.py: launched with WORLD_SIZE={world} but --gpus {args.gpus}", file=sys.stderr)
        return 2
    logging.basicConfig(level=logging.INFO, stream=sys.stdout)
    cfg = PipelineConfig(block_size=args.block_size, sr_scale=args.sr_scale, sr_weights=args.sr_weights, sr_act=args.sr_act, sr_ensemble=args.sr_ensemble,
                         qa_ms_ssim=args.qa_ms_ssim, qa_benchmark=args.qa_benchmark, qa_vif=args.qa_vif, qa_gmsd=args.qa_gmsd, qa_delta_e=args.qa_delta_e, qa_haarpsi=args.qa_haarpsi, qa_map_cell=args.qa_map_cell, qa_fsim=args.qa_fsim, qa_vsi=args.qa_vsi,
                         qa_niqe_params=args.qa_niqe_params, qa_brisque_model=args.qa_brisque_model, qa_dists_weights=args.qa_dists_weights,
                         benchmark_degrade=args.benchmark_degrade)
    if args.plan_only:
        from PIL import Image
        with Image.open(args.input) as im:
            plan = shard_plan(im.size, cfg, world)
        if world > 1:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            dist.init_process_group("gloo", rank=rank, world_size=world)
            plans = [None] * world
            dist.all_gather_object(plans, plan)
            same = all(p == plans[0] for p in plans)
            dist.destroy_process_group()
            if not same:
                print("main.py: the ranks disagree on the shard plan", file=sys.stderr)
                return 3
        if rank == 0:
            print(json.dumps({"world": world, **plan}), flush=True)
        return 0
    async with SuperResolutionPipeline(cfg) as pipe:
        res = await pipe.process(args.input, args.output, prompt="")
    if rank == 0:
        print(res)
    return 0 if res.success else 1


if __name__ == "__main__":
    sys.exit(asyncio.run(main()))
