#!/usr/bin/env python3
"""bench.py -- megapixels/sec of tile + blend + QA on a synthetic 720p -> 200 MP job (BASELINE.json).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--workload 200MP|150MP|100MP|4MP|200MP-kd ...]
                    [--mode strips|batch] [--dump-outputs DIR] [--full [--no-pcie] [--no-cpu-baseline] [--no-prof] [--sweep ...]]

One process per GPU (N > 1: launched by torch.distributed.run, RCCL over xGMI).  A "step" is one
pass of the hot path over one synthetic image: overlap-tile extract of the 5x5 tile grid from the
device-resident SR output, [exchange of tile rows between tile owners and strip owners],
Laplacian-pyramid blend of the canvas strips, PSNR + SSIM (uniform-7, Gaussian-11 cropped,
Gaussian-11 full-frame) of the canvas against the reference upscale, one all-reduce of the metric
partial sums.  N > 1 splits the SAME image over the ranks (strong scaling; --mode strips, the default and the
BASELINE metric).  --mode batch is BASELINE config 4: every rank runs the whole pipeline on its own image, no
communication on the data path (weak scaling).  "-kd" workloads use the non-uniform k-d tiling of config 5.

Prints ONE JSON line (rank 0).  ``value`` = canvas megapixels / max-over-ranks wall time per step,
inputs already resident in HBM; ``ms_per_step`` = milliseconds of one timed step (--steps of them).
A plain run only sets up, warms up, times the steps and prints the line.  ``--full`` adds everything
else: ``roofline`` describes the dominant kernel (HIP-event time measured here, on the stream the
kernels run on), the per-kernel table, the PCIe and single-image figures, the ``sweep`` of further
workloads, ``cpu_baseline`` -- the CPU oracle
(oracle/sr_oracle.c, OpenMP) timed on this node's host cores on a bounded sample of the same workload
-- and ``parity``, that sample through the HIP pipeline compared with the oracle.

``--dump-outputs DIR`` writes what the timed path computed in its last step (the canvas, sampled, and
the scores) as DIR/<name>.npy; the inputs are seeded, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(ROOT, "super-resolution-system_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

WORKLOAD_CHOICES = ["4MP", "100MP", "150MP", "200MP", "100MP-kd", "150MP-kd", "200MP-kd"]
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling


def synthetic_source(w: int = 1080, h: int = 720, seed: int = 20260313, noise_seed_offset: int = 0) -> np.ndarray:
    """smooth field + integer noise, 3:2 so the 200 MP preset is reached."""
    rng = np.random.default_rng(seed + noise_seed_offset)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for c in range(3):
        chans.append(128 + 64 * np.sin(xx / 37.0 + 0.7 * c) + 48 * np.cos(yy / 23.0 + 1.3 * c))
    img = np.stack(chans, axis=-1) + rng.integers(-12, 13, (h, w, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def fused_gather_enabled() -> bool:
    """The library's default: the final gather builds R_1 itself (k_final_fused); SR_FUSED_FINAL=0 selects the unfused pair."""
    return os.environ.get("SR_FUSED_FINAL", "1")[:1] != "0"


def down2_enabled() -> bool:
    """The library's default for u8 RGB tiles: levels 1 and 2 of the Gaussian pyramid out of one march (k_down2_march);
    SR_DOWN2=0 selects the two launches of round 3."""
    return os.environ.get("SR_DOWN2", "1")[:1] != "0"


def algorithmic_bytes(geo, fused: bool = None) -> dict:
    """Bytes each kernel family must move per step (DESIGN.md 'kernels and their rooflines').  With the fused gather
    (round 3) R_1 is never written or read: the collapse chain stops at level 2 and the gather reads G_1, W_1, G_2, R_2."""
    n, m = geo.tile_pixels, geo.canvas_pixels
    fused = fused_gather_enabled() if fused is None else fused
    s14 = sum(4.0 ** -i for i in range(1, 5))
    s24 = sum(4.0 ** -i for i in range(2, 5))
    s25 = sum(4.0 ** -i for i in range(2, 6))
    s35 = sum(4.0 ** -i for i in range(3, 6))
    d2 = down2_enabled()
    up_all = (34.0 * s14 + 28.0 * 4.0 ** -5) * n                      # G_i, G_i+1/4, R_i+1/4, W_i in; R_i out, levels 5..1
    out = {
        "tile_extract": 6.0 * n,                                   # 3 B read + 3 B write per tile px
        # u8 in (3) + G1 out (12/4); round 4's march also writes G2 (12/16) and G1 is never read back for it
        "down_l0": (6.75 if d2 else 6.0) * n,
        "down_l1p": (12.0 * s24 + 12.0 * s35) * n if d2 else (12.0 * s14 + 12.0 * s25) * n,     # G2..G4 (G1..G4) in, G3..G5 (G2..G5) out
        "up_level": (34.0 * s24 + 28.0 * 4.0 ** -5) * n if fused else up_all,       # fused: levels 5..2 only
        # fused: u8 tile 3 + G_1 12/4 + W_1 4/4 + (G_2 + R_2) 24/16 per tile px in; u8 canvas out
        "final_gather": (3.0 + 3.0 + 1.0 + 1.5) * n + 3.0 * m if fused else 9.0 * n + 3.0 * m,
        "assess_all": 6.0 * m,                                     # both u8 images once: SSE + 3 SSIM variants (one pass)
        # the reference-shaped model of SURVEY 8(d) (scatter into fp32 accumulators), for comparison
        "_survey_blend_model": 63.30 * n + 19.0 * m,
    }
    return out


# bench kernel family -> prefix of the rocprofv3 kernel name(s) (template arguments change between builds: matched by prefix)
ROCPROF_PREFIXES = {"tile_extract": ["k_tile_extract"], "down_l0": ["k_down_march<0,", "k_down2_march<"],
                    "down_l1p": ["k_down_march<2,", "k_down2_cols"],
                    "up_level": ["k_up_level_blk<"],
                    "final_gather": ["k_final_fast<", "k_final_fused<", "k_final_march1<", "k_final_marchn<", "k_final_marchp<", "k_final_rect<"],
                    "assess_all": ["k_assess_march<"]}
BLEND_FAMILIES = ("down_l0", "down_l1p", "up_level", "final_gather")
# VALU model of the fused assessment: per pixel (= per thread and row) the march issues ~223 VALU instructions
# (118 of them fp64) and the loader ~14 more (SQ_INSTS_VALU of a launch: 742 M wave-instructions for 200 MP = 237 per
# 64-pixel row).  On gfx950 a wave's VALU instruction occupies its SIMD for 4 cycles whatever the type (fp64, fp32 and
# integer alike; only packed fp32 does two lanes' worth): measured on this path, profiles/r03_*.
ASSESS_VALU_INSTR_PER_PX = 237
VALU_CYCLES_PER_WAVE_INSTR = 4
GPU_SIMDS, GPU_CLOCK_HZ = 256 * 4, 2.4e9


def family_of(kernel_name: str):
    k = kernel_name.replace("void ", "")
    for fam, prefixes in ROCPROF_PREFIXES.items():
        if any(k.startswith(p) for p in prefixes):
            return fam
    return None


def measured_traffic() -> dict:
    """HBM bytes per LAUNCH SET (all launches of the family in one step) from the newest committed PMC summary
    (tools/summarize_profiles.py: FETCH_SIZE / WRITE_SIZE in their own rocprofv3 passes; `total_2x` = reads doubled as
    MI355X_MICROARCH.md prescribes for gfx950, `total` = reads scaled by the factor calibrated on the pure-copy kernel)."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json")))      # rNN_<letter>_traffic.json: name order
    data = None
    while files and data is None:
        cand = json.load(open(files[-1]))
        if cand.get("format") == 2:                       # per-launch records (round 3 on); older summaries are not read
            data = cand
        else:
            files.pop()
    if data is None:
        return {}
    out = {"_source": os.path.basename(files[-1]), "_note": data.get("note"), "_build_digest": data.get("build_digest")}
    for name, rec in data.get("kernels", {}).items():
        fam = family_of(name)
        if fam is None:
            continue
        acc = out.setdefault(fam, {"total": 0.0, "total_2x": 0.0, "launches_per_step": 0.0})
        acc["total"] += rec["per_step"]["total"]
        acc["total_2x"] += rec["per_step"]["total_2x"]
        acc["launches_per_step"] += rec["launches_per_step"]
    return out


def traffic_stale(traffic: dict):
    """True when the PMC summary the `traffic` figures come from was collected on another build of the library than the one
    loaded now (source digest compiled into libsrhip.so), None when either side is unknown."""
    try:
        import _native
        now = _native.load().sr_source_digest().decode()
    except Exception:  # noqa: BLE001
        return None
    then = traffic.get("_build_digest")
    return None if not then or not now else (then != now)


def cpu_baseline(seed_img: np.ndarray, geo_full, budget_tiles=(3, 3), repeats: int = 3) -> dict:
    """The CPU oracle on a bounded sample: a rows x cols corner of the same tile grid (same tile size / overlap /
    levels), tile extract + Laplacian blend + PSNR + 3 x SSIM.  One warm-up on a 2 x 2 corner (library load, OpenMP
    team start-up), then `repeats` timed runs of the sample: the median run is reported."""
    from oracle import oracle_c as oc
    x0, y0, tw, th = geo_full.rects[0]
    step_x = geo_full.rects[1][0] - x0 if len(geo_full.rects) > 1 else tw
    ncols_full = sum(1 for r in geo_full.rects if r[1] == y0)
    step_y = geo_full.rects[ncols_full][1] - y0 if len(geo_full.rects) > ncols_full else th
    scale = geo_full.canvas_w / seed_img.shape[1]

    def one(rows, cols):
        W, H = (cols - 1) * step_x + tw, (rows - 1) * step_y + th
        sw, sh = int(np.ceil(W / scale)) + 4, int(np.ceil(H / scale)) + 4
        src = np.ascontiguousarray(seed_img[:sh, :sw])
        ref = oc.resize_cubic_u8(src, int(sw * scale), int(sh * scale))[:H, :W]
        img = np.ascontiguousarray(ref)
        ref = np.ascontiguousarray(np.clip(ref.astype(np.int16) + 2, 0, 255).astype(np.uint8))
        rects = [(c * step_x, r * step_y, tw, th) for r in range(rows) for c in range(cols)]
        t0 = time.perf_counter()
        tiles = [np.ascontiguousarray(img[y:y + h, x:x + w]) for (x, y, w, h) in rects]          # tile
        t1 = time.perf_counter()
        canvas = oc.laplacian_fusion(tiles, [(y, x) for (x, y, _, _) in rects], (H, W), geo_full.levels,
                                     geo_full.weight_type)                                          # blend
        t2 = time.perf_counter()
        scores = {"psnr": oc.psnr(ref, canvas)}                                                     # QA
        g1, g2 = oc.rgb2gray_u8(ref), oc.rgb2gray_u8(canvas)
        for mode in ("uniform", "gauss", "simple"):
            scores[f"ssim_{mode}"] = oc.ssim(g1, g2, mode)
        t3 = time.perf_counter()
        keep.update(img=img, ref=ref, canvas=canvas, scores=scores, rows=rows, cols=cols,
                    grid=dict(tile_w=tw, tile_h=th, rows=rows, cols=cols, ov_x=tw - step_x, ov_y=th - step_y))
        return W, H, (t1 - t0, t2 - t1, t3 - t2)

    keep = {}
    rows, cols = min(budget_tiles[0], len(geo_full.rects) // max(ncols_full, 1)), min(budget_tiles[1], ncols_full)
    one(min(2, rows), min(2, cols))                                      # warm-up, not reported
    runs = [one(rows, cols) for _ in range(max(1, repeats))]
    W, H = runs[0][0], runs[0][1]
    totals = sorted(sum(r[2]) for r in runs)
    med = min(runs, key=lambda r: abs(sum(r[2]) - totals[len(totals) // 2]))[2]
    mp = W * H / 1e6
    return keep, {"value": mp / sum(med), "unit": "MP/s", "cores": oc.num_threads(), "kind": "port",
            "omp_num_threads_env": os.environ.get("OMP_NUM_THREADS"), "host_cpus": os.cpu_count(),
            "runs_s": [round(t, 3) for t in totals], "statistic": f"median of {len(runs)} runs after 1 warm-up",
            "sample": f"{rows}x{cols} corner of the tile grid ({W}x{H} = {mp:.1f} MP canvas, tiles {tw}x{th}): "
                      f"extract {med[0]:.2f}s + laplacian blend {med[1]:.2f}s + PSNR/3xSSIM {med[2]:.2f}s; "
                      f"oracle/sr_oracle.c with OpenMP (restated reference CPU path, cv2/skimage absent)"}


def parity_vs_oracle(sample: dict, geo_full, device_index: int) -> dict:
    """The CHECK that goes with cpu_baseline (outside every timed region): the oracle's sample -- the same corner of the
    tile grid, same inputs -- through the HIP pipeline object, canvas compared byte for byte, PSNR for equality, the three
    SSIM variants by relative error.  (Full-size comparisons of every BASELINE config: tests/test_gpu_fullsize.py.)"""
    import torch
    import device_pipeline as dp
    geo = dp.grid_geometry(levels=geo_full.levels, weight_type=geo_full.weight_type, **sample["grid"])
    H, W = geo.canvas_h, geo.canvas_w
    assert sample["canvas"].shape == (H, W, 3)
    # the sample's canvas is below the size from which the library takes the marched gather by itself: the check must run the
    # kernels the timed workload ran (SR_MARCH is read when the plan is made)
    prev = os.environ.get("SR_MARCH")
    if prev is None:
        os.environ["SR_MARCH"] = "2"
    try:
        pipe = dp.DevicePipeline(geo, 0, 1, device_index)
    finally:
        if prev is None:
            os.environ.pop("SR_MARCH", None)
    d_img = torch.from_numpy(sample["img"].reshape(H, W * 3)).to(pipe.dev)
    d_ref = torch.from_numpy(sample["ref"].reshape(H, W * 3)).to(pipe.dev)
    pipe.step(d_img, d_ref)
    torch.cuda.synchronize()
    got = pipe.canvas.cpu().numpy().reshape(H, W, 3)
    m = pipe.metrics()
    pipe.close()
    want = sample["scores"]
    ndiff = int(np.count_nonzero(got != sample["canvas"]))
    rel = {k: abs(m[k] - want[k]) / max(abs(want[k]), 1e-300) for k in ("ssim_uniform", "ssim_gauss", "ssim_simple")}
    return {"canvas_equal": ndiff == 0, "canvas_bytes_differing": ndiff, "canvas_bytes": int(got.size),
            "psnr_equal": m["psnr"] == want["psnr"], "psnr_gpu": m["psnr"], "psnr_oracle": want["psnr"],
            "ssim_rel_err": max(rel.values()), "ssim_rel_err_by_mode": rel, "ssim_tolerance": 1e-9,
            "sample": f"{sample['rows']}x{sample['cols']} corner of the tile grid, {W}x{H} canvas "
                      f"({W * H / 1e6:.1f} MP): HIP pipeline vs oracle/sr_oracle.c on the same inputs, outside the timed region",
            "oracle": "restated reference CPU path; its OpenCV-defined semantics are parity-unpinned (DESIGN.md 2)"}


DUMP_SAMPLE = 1 << 21        # canvas bytes kept by --dump-outputs: 8 MB of values + 16 MB of their indices
DUMP_SEED = 20261016


def dump_outputs(out_dir: str, canvas: np.ndarray, quality: dict) -> None:
    """--dump-outputs: what a caller of the timed path receives from its last step -- the blended u8 canvas [H, W*cn] and
    the scores -- as out_dir/<name>.npy in float32 / float64.  A 200 MP canvas is 600 MB of bytes, so it is kept as a fixed,
    seeded sample of its bytes (with their flat indices) plus its exact row and column sums (~25 MB in all)."""
    os.makedirs(out_dir, exist_ok=True)
    flat = canvas.reshape(-1)
    k = min(flat.size, DUMP_SAMPLE)
    idx = np.arange(flat.size) if k == flat.size else \
        np.sort(np.random.default_rng(DUMP_SEED).choice(flat.size, k, replace=False))
    arrays = {"canvas_sample": flat[idx].astype(np.float32),
              "canvas_sample_index": idx.astype(np.float64),
              "canvas_row_sums": canvas.sum(axis=1, dtype=np.int64).astype(np.float64),
              "canvas_col_sums": canvas.sum(axis=0, dtype=np.int64).astype(np.float64)}
    for name, v in quality.items():
        arrays[name] = np.array([v], dtype=np.float64)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


_STAGE_FILE = os.environ.get("SR_BENCH_STAGE_FILE")


def _stage(name: str) -> None:
    """Progress marker of one rank (N > 1 only): the launcher prints each rank's last completed stage when its deadline
    passes, so a rank stuck in a collective is named instead of the run dying silently at the driver's limit."""
    if _STAGE_FILE:
        try:
            with open(_STAGE_FILE, "a") as f:
                f.write(f"{time.time():.3f} {name}\n")
        except OSError:
            pass


def _launch_ranks(n: int, argv, deadline_s: float) -> int:
    """``python bench.py --gpus N`` without a launcher around it: the N ranks as fresh child processes
    (super-resolution-system_amd/_launch.py: env:// rendezvous on 127.0.0.1, per-rank stage markers, deadline -> 124, never exec)."""
    import _launch
    return _launch.launch_ranks(n, os.path.abspath(__file__), argv, deadline_s, who="bench.py")


def run_workload(args, workload: str, steps: int, warmup: int, detailed: bool, dist_state, dump_dir=None) -> dict:
    """One measurement of `workload` on the ranks of `dist_state`; returns the result record on rank 0 (None elsewhere).
    `detailed` (--full) adds the per-kernel, PCIe, single-image and CPU-baseline figures; `dump_dir` receives the outputs
    of the last timed step (dump_outputs)."""
    import torch
    import torch.distributed as dist
    import device_pipeline as dp

    world, rank, local_rank, backend, dev = dist_state
    geo = dp.workload_geometry(workload)
    H, W, cn = geo.canvas_h, geo.canvas_w, geo.cn
    _stage(f"{workload}: start")

    # ---- inputs, resident in HBM before the timed region ----------------------------------------
    # reference = whole-image bicubic upscale of the synthetic 720p source; image (the "SR output" the
    # tiles are cut from) = the same upscale of a slightly different noise draw, so PSNR is finite.
    batch = args.mode == "batch"
    src_ref = synthetic_source(noise_seed_offset=rank if batch else 0)
    src_img = np.clip(src_ref.astype(np.int16) + np.random.default_rng(7).integers(-3, 4, src_ref.shape), 0, 255).astype(np.uint8)
    pipe = dp.DevicePipeline(geo, 0, 1, local_rank) if batch else dp.DevicePipeline(geo, rank, world, local_rank)
    ctx = pipe.ctx

    class _Prof:
        """sr_prof_* on both contexts of the pipeline (blend on the main stream, assessment on the second one)."""
        ctxs = (pipe.ctx, pipe.qa_ctx)

        def enable(self, on):
            for c in self.ctxs:
                c.prof_enable(on)

        def select(self, name):
            for c in self.ctxs:
                c.prof_select(name)

        def reset(self):
            for c in self.ctxs:
                c.prof_reset()

        def get(self):
            out = {}
            for c in self.ctxs:
                for k, (ms, n) in c.prof_get().items():
                    a = out.get(k, (0.0, 0))
                    out[k] = (a[0] + ms, a[1] + n)
            return out

    prof_ctl = _Prof()
    no_prof = args.no_prof or not detailed
    t_src = torch.from_numpy(np.stack([src_ref, src_img])).to(dev)
    reference = torch.empty((H, W * cn), dtype=torch.uint8, device=dev)
    image = torch.empty((H, W * cn), dtype=torch.uint8, device=dev)
    sh, sw = src_ref.shape[:2]
    ctx.resize_cubic_u8(t_src[0].data_ptr(), sw * cn, sh, sw, cn, reference.data_ptr(), W * cn, H, W)
    torch.cuda.synchronize()
    t_stub = time.perf_counter()                 # the SR stand-in (bicubic upscale to the output size), timed once:
    ctx.resize_cubic_u8(t_src[1].data_ptr(), sw * cn, sh, sw, cn, image.data_ptr(), W * cn, H, W)
    torch.cuda.synchronize()                     # the "end-to-end" column of SURVEY 8(d), never part of `value`
    sr_stub_ms = 1e3 * (time.perf_counter() - t_stub)
    _stage(f"{workload}: inputs resident, pipeline built")

    def barrier():
        if world > 1:
            dist.barrier()

    # A stream of K images (DevicePipeline.pipeline_step): the assessment of image i runs on a second HIP stream beside
    # the tile stage and pyramids of image i+1 (fp64-VALU-bound next to bandwidth-bound work), and for N > 1 the tile
    # stage + exchange of image i+1 are posted as soon as image i's rows have arrived, so the xGMI transfer runs under
    # the blend of image i.  Every image goes through every stage inside the timed region.
    lp_model, lp_value = None, None
    if args.lpips != "none":
        if world > 1 and not batch:
            raise SystemExit("--lpips needs one GPU or --mode batch (a strip owner holds only its rows of the canvas)")
        import _native
        lp_model = _native.LpipsModel(ctx, args.lpips, _native.lpips_synthetic_weights(args.lpips))

    def run_steps(k):
        nonlocal lp_value
        if k <= 0:
            return
        pipe.pipeline_begin(image)
        for i in range(k):
            pipe.pipeline_step(reference, image if i + 1 < k else None)
            if lp_model is not None:                     # synchronous (returns the layer sums): ends the overlap for this image
                torch.cuda.current_stream(dev).synchronize()
                lp_value = lp_model.value(reference.data_ptr(), reference.stride(0), pipe.canvas.data_ptr(), pipe.canvas.stride(0),
                                          H, W, cn)
            if evs is not None:
                evs[i + 1].record()
        pipe.pipeline_finish()

    # Per-kernel HIP-event timing costs two event records per kernel family per step and those serialise neighbouring
    # kernels (~2 % of a step on one GPU, far more of a 1/8 step).  So: all families are timed during the warm-up (to
    # find the dominant kernel) and in a short pass after the timed region (the `kernels` table); inside the timed
    # region only the dominant kernel is timed -- that measurement is what `roofline` reports.
    evs = None
    dominant = "assess_all"
    if not no_prof and warmup > 0:
        prof_ctl.enable(True)
        prof_ctl.reset()
    run_steps(warmup)
    torch.cuda.synchronize()
    _stage(f"{workload}: warm-up ({warmup} steps) done")
    if not no_prof and warmup > 0:
        warm = prof_ctl.get()
        if warm:
            dominant = max(warm.items(), key=lambda kv: kv[1][0])[0]

    if not no_prof:
        prof_ctl.enable(True)
        prof_ctl.select(dominant)
        prof_ctl.reset()
    # per-step device time (events on the stream the kernels run on): median / min beside the mean of the contract
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    barrier()
    torch.cuda.synchronize()
    _stage(f"{workload}: barrier before the timed region passed")
    t0 = time.perf_counter()
    evs[0].record()
    run_steps(steps)
    torch.cuda.synchronize()
    _stage(f"{workload}: timed steps enqueued and synchronised")
    barrier()
    elapsed = time.perf_counter() - t0
    _stage(f"{workload}: timed region ({steps} steps) done")
    step_ms = sorted(evs[i].elapsed_time(evs[i + 1]) for i in range(steps))
    prof_timed = {} if no_prof else prof_ctl.get()               # the dominant kernel, inside the timed region
    if dump_dir:
        # before anything else runs on the pipeline: the strips of N > 1 are gathered on rank 0 (batch: rank 0's own image)
        canvas = pipe.gather_canvas(0) if (world > 1 and not batch) else pipe.canvas
        quality = pipe.metrics()
        if rank == 0:
            if lp_model is not None:
                quality[f"lpips_{args.lpips}_synthetic_weights"] = lp_value
            dump_outputs(dump_dir, canvas.cpu().numpy(), quality)
        del canvas
        _stage(f"{workload}: outputs written")
    prof, prof_steps = {}, max(1, min(steps, 5))
    # one image at a time, nothing overlapped, no per-kernel events: what an isolated image costs (the image stream above
    # hides the assessment of image i under the pyramids of image i+1)
    latency_single = None
    if detailed:
        pipe.step(image, reference)
        torch.cuda.synchronize()
        tl = time.perf_counter()
        for _ in range(prof_steps):
            pipe.step(image, reference)
        torch.cuda.synchronize()
        latency_single = round(1e3 * (time.perf_counter() - tl) / prof_steps, 4)
    if not no_prof:
        # every family, in its own pass after the timed region, one image at a time on one stream (step()): standalone
        # kernel durations -- in the timed region the assessment shares the GPU with the next image's pyramids
        prof_ctl.select(None)
        prof_ctl.reset()
        for _ in range(prof_steps):
            pipe.step(image, reference)
        torch.cuda.synchronize()
        prof = prof_ctl.get()
    prof_ctl.enable(False)

    _stage(f"{workload}: per-kernel pass done")
    t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    metrics = pipe.metrics()
    # N > 1: what every rank exchanged and how long its grouped batch took, gathered on rank 0 so a scaling curve can be
    # explained (strip bounds, bytes in / out per rank, tiles owned)
    ranks_info = None
    if world > 1 and not batch:
        xp = pipe.xplan
        mine = {"rank": rank, "strip_rows": list(pipe.strip), "blend_rows": [pipe.row_begin, pipe.row_end],
                "tiles_owned": len(pipe.owned), "tiles_received": len(xp.recvs(rank)),
                "exchange_bytes_in": xp.bytes_received(rank, geo),
                "exchange_bytes_out": sum((b - a) * geo.rects[tt][2] * geo.cn for (_, tt, a, b) in xp.sends(rank)),
                "exchange_wait_ms_per_step": round(1e3 * pipe.exchange_wait_s / max(pipe.exchange_waits, 1), 4),
                "kernel_ms_per_step": {kk: round(ms / prof_steps, 4) for kk, (ms, _) in prof.items()}}
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        ranks_info = gathered
    elif world > 1 and batch:
        # config 4: one image per rank, nothing on the data path between them -- every rank's own line, gathered
        mine = {"rank": rank, "image_noise_seed_offset": rank, "tiles_owned": len(geo.rects), "tiles_received": 0,
                "exchange_bytes_in": 0, "exchange_bytes_out": 0, "collectives_on_data_path": 0,
                "step_ms_median": round(step_ms[len(step_ms) // 2], 4),
                "quality": {k: (v if np.isfinite(v) else str(v)) for k, v in metrics.items()}}
        gathered = [None] * world
        dist.all_gather_object(gathered, mine)
        ranks_info = gathered
    _stage(f"{workload}: results gathered")

    pcie = None
    if world == 1 and detailed and not args.no_pcie:
        # the boundary's host-buffer variant: inputs uploaded, canvas downloaded (pinned host memory); never `value`
        h_in = torch.empty((2, H, W * cn), dtype=torch.uint8).pin_memory()
        h_out = torch.empty((H, W * cn), dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()
        ta = time.perf_counter()
        image.copy_(h_in[0], non_blocking=True)
        reference.copy_(h_in[1], non_blocking=True)
        torch.cuda.synchronize()
        tb = time.perf_counter()
        h_out.copy_(pipe.canvas, non_blocking=True)
        torch.cuda.synchronize()
        tc = time.perf_counter()
        pcie = {"h2d_ms": round(1e3 * (tb - ta), 3), "h2d_GB": round(2 * H * W * cn / 1e9, 3),
                "d2h_ms": round(1e3 * (tc - tb), 3), "d2h_GB": round(H * W * cn / 1e9, 3),
                "note": "pinned host buffers, one copy engine; add to ms_per_step for the host-buffer boundary"}
        del h_in, h_out

    out = None
    if rank == 0:
        ms_per_step = 1e3 * elapsed / steps
        mp = geo.canvas_pixels / 1e6
        alg = algorithmic_bytes(geo)
        images = world if batch else 1
        div = world if (world > 1 and not batch) else 1          # strips: each rank moves ~1/N of the bytes
        blend_alg = sum(alg[kk] for kk in ("down_l0", "down_l1p", "up_level", "final_gather")) / div
        out = {
            "metric": "megapixels/sec tile+blend+QA at 200MP, 1/2/4/8 GPU",
            "value": round(images * mp / (elapsed / steps), 1),
            "unit": "MP/s",
            "n_gpus": world, "steps": steps, "warmup": warmup,
            "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True,
            "scaling": "weak" if batch else "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic" if backend == "nccl" else f"synthetic (REHEARSAL backend {backend}: not a measurement)",
            "config": {"workload": f"720p->{workload} {geo.canvas_w}x{geo.canvas_h} canvas, "
                                   f"{len(geo.rects)} tiles {geo.rects[0][2]}x{geo.rects[0][3]}, {geo.levels}-level "
                                   f"Laplacian blend (cosine weights) + PSNR + SSIM(uniform7,gauss11,simple)",
                       "tile_pixels": geo.tile_pixels, "canvas_pixels": geo.canvas_pixels,
                       "parallelism": (f"batch{world}" if batch else f"strips{world}") if world > 1 else "single",
                       "stream": "assessment of image i on a second HIP stream beside tile+pyramids of image i+1"
                                 + ("; exchange of image i+1 under the blend of image i" if (world > 1 and not batch) else "")},
            "step_ms": {"median": round(step_ms[len(step_ms) // 2], 4), "min": round(step_ms[0], 4),
                        "max": round(step_ms[-1], 4), "clock": "HIP events on the main stream between consecutive images, rank 0"},
            "quality": {k: (v if np.isfinite(v) else str(v)) for k, v in metrics.items()},
        }
        try:
            import _native
            out["build_digest"] = _native.load().sr_source_digest().decode()      # the library this line was measured on
        except Exception:  # noqa: BLE001
            out["build_digest"] = None
        if ranks_info is not None:
            out["ranks"] = ranks_info
            if not batch:
                out["config"]["strip_bounds"] = list(pipe.xplan.bounds)
        if lp_model is not None:
            out["config"]["workload"] += f" + LPIPS-{args.lpips} (synthetic weights, parity unpinned)"
            out["quality"][f"lpips_{args.lpips}_synthetic_weights"] = lp_value
        if detailed:
            kernels = {}
            share = 1.0 / world if (world > 1 and not batch) else 1.0         # each rank moves ~1/N of the bytes (+ halo)
            parts = {}
            for name, (ms, launches) in prof.items():
                nsteps = prof_steps
                per_step_ms = ms / nsteps
                if name.startswith("gather_"):                       # the launches inside final_gather (marched zones / block kernel)
                    parts[name[len("gather_"):]] = round(per_step_ms, 4)
                    continue
                b = alg.get(name)
                kernels[name] = {"ms_per_step": round(per_step_ms, 4), "launches_per_step": launches / nsteps,
                                 "timed_in": "separate sequential pass (standalone)",
                                 "alg_GB": None if b is None else round(b * share / 1e9, 4),
                                 "GBps": None if b is None or per_step_ms <= 0 else round(b * share / 1e9 / (per_step_ms / 1e3), 1)}
            if parts and "final_gather" in kernels:
                kernels["final_gather"]["parts_ms"] = parts
                kernels["final_gather"]["parts_note"] = ("march<N>: column-marching kernels over the zones covered by N tiles; rest: what "
                                                         "no march item takes (bands along the tile edges), as rectangles of cells "
                                                         "(k_final_rect; the block kernel where nothing is marched)")
            roofline = None
            traffic = measured_traffic() if (world == 1 and workload == "200MP") else {}
            cands = [(v["ms_per_step"], k) for k, v in kernels.items() if v["alg_GB"] is not None]
            if cands:
                _, dom = max(cands)
                k = kernels[dom]
                lps = max(k["launches_per_step"], 1)
                alg_launch = k["alg_GB"] * 1e9 / lps
                per_launch_ms = k["ms_per_step"] / lps
                achieved = alg_launch / 1e9 / (per_launch_ms / 1e3) if per_launch_ms > 0 else 0.0
                standalone = {"avg_launch_ms": round(per_launch_ms, 4), "achieved": round(achieved, 1),
                              "frac": round(achieved / HBM_PEAK_GBS, 4)}
                if dom in prof_timed and prof_timed[dom][1] > 0:      # the same kernel as it ran inside the timed region
                    t_ms, t_n = prof_timed[dom]
                    per_launch_ms = t_ms / t_n
                    achieved = alg_launch / 1e9 / (per_launch_ms / 1e3) if per_launch_ms > 0 else 0.0
                tr = traffic.get(dom)
                roofline = {"bound": "valu_fp64" if dom == "assess_all" else "hbm", "kernel": dom,
                            "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS,
                            "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                            # HBM bytes per launch from the PMC counters, reads doubled as the microarchitecture guide
                            # prescribes for gfx950 (traffic_calibrated: reads scaled by the factor measured on the pure copy)
                            "traffic": (tr["total_2x"] / max(tr["launches_per_step"], 1)) if tr else None,
                            "traffic_calibrated": (tr["total"] / max(tr["launches_per_step"], 1)) if tr else None,
                            "traffic_source": traffic.get("_source"),
                            "traffic_build_digest": traffic.get("_build_digest"),
                            "traffic_stale": traffic_stale(traffic),      # counters collected on another build of the library
                            "avg_launch_ms": round(per_launch_ms, 4),
                            "alg_bytes_per_launch": alg_launch,
                            "measured_in": "timed region (this kernel shares the GPU with the next image's tile stage and "
                                           "pyramids there)" if dom in prof_timed else "separate sequential pass",
                            "standalone": standalone}
                if dom == "assess_all":
                    # the kernel that dominates is not HBM-bound: its own roof is fp64 VALU issue (the reference's SSIM is
                    # float64).  floor = pixels x (fp64-rate instr x 4 + fp32-rate instr x 2 cycles per wave of 64) / SIMDs / clock
                    px = geo.canvas_pixels * share
                    cyc = ASSESS_VALU_INSTR_PER_PX * VALU_CYCLES_PER_WAVE_INSTR
                    floor_ms = 1e3 * (px / 64.0) * cyc / GPU_SIMDS / GPU_CLOCK_HZ
                    roofline["valu"] = {"floor_ms": round(floor_ms, 4), "frac": round(floor_ms / per_launch_ms, 4) if per_launch_ms > 0 else None,
                                        "frac_standalone": round(floor_ms / standalone["avg_launch_ms"], 4) if standalone["avg_launch_ms"] > 0 else None,
                                        "model": f"{ASSESS_VALU_INSTR_PER_PX} VALU instructions per pixel (SQ_INSTS_VALU / pixels x 64) x "
                                                 f"{VALU_CYCLES_PER_WAVE_INSTR} cycles per wave-instruction, {GPU_SIMDS} SIMDs at "
                                                 f"{GPU_CLOCK_HZ / 1e9:.1f} GHz: the time the kernel's own instruction stream needs at 100 % VALU "
                                                 "busy"}
                    roofline["note"] = ("fp64-VALU-bound: `frac` is the HBM fraction the contract asks for, `valu.frac` the fraction "
                                        "of the kernel's own (instruction-issue) roof")
            blend_ms = sum(v["ms_per_step"] for kk, v in kernels.items() if kk in ("weight_down",) + BLEND_FAMILIES)
            roofline_blend = None
            if blend_ms > 0:
                bt = [traffic.get(kk) for kk in BLEND_FAMILIES]
                roofline_blend = {"bound": "hbm", "kernels": [kk for kk in BLEND_FAMILIES if kk in kernels],
                                  "achieved": round(blend_alg / 1e9 / (blend_ms / 1e3), 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": round(blend_alg / 1e9 / (blend_ms / 1e3) / HBM_PEAK_GBS, 4),
                                  "alg_bytes": blend_alg, "ms": round(blend_ms, 4),
                                  "fused_gather": fused_gather_enabled(),
                                  # what rocprof counted (separate --pmc passes, newest committed summary) over the same time:
                                  # the "rocprof achieved-HBM-GB/s" of the north star
                                  "traffic": sum(t["total_2x"] for t in bt) if all(bt) else None,
                                  "traffic_calibrated": sum(t["total"] for t in bt) if all(bt) else None,
                                  "achieved_counter_GBps": round(sum(t["total"] for t in bt) / 1e9 / (blend_ms / 1e3), 1) if all(bt) else None,
                                  "frac_counter": round(sum(t["total"] for t in bt) / 1e9 / (blend_ms / 1e3) / HBM_PEAK_GBS, 4) if all(bt) else None,
                                  "traffic_source": traffic.get("_source"),
                                  "traffic_stale": traffic_stale(traffic),
                                  # SURVEY 8(d)'s contract model (scatter into fp32 accumulators: 63.30 B per tile px + 19 B per
                                  # canvas px) priced on the same time: above 1 BY DESIGN -- this gather never materialises the fp32
                                  # canvas, so it moves a third of those bytes; not evidence of skipped work (see `parity`)
                                  "frac_survey_model": round(alg["_survey_blend_model"] / div / 1e9 / (blend_ms / 1e3) / HBM_PEAK_GBS, 4),
                                  "timed_in": "separate sequential pass (standalone kernels, one image at a time)",
                                  "note": "the Laplacian blend of one image (pyramid down chain, collapse, canvas gather); "
                                          "alg_bytes is THIS design's byte model (R_1 is never written: the gather forms it on the "
                                          "fly); frac = alg_bytes / time / 8 TB/s, frac_counter the same with the bytes rocprof counted"}
            gpu_ms = sum(v["ms_per_step"] for v in kernels.values())
            total_alg = sum(alg[kk] for kk in kernels if kk in alg)
            out.update({
                "pcie": pcie,
                "end_to_end": {"sr_stub_ms": round(sr_stub_ms, 3), "ms_per_image_with_stub": round(ms_per_step + sr_stub_ms, 3),
                               "note": "SR stand-in = cv2.INTER_CUBIC upscale of the 720p source on the GPU (sr_resize_cubic_u8), "
                                       "outside the timed region and outside the roofline"},
                "roofline": roofline,
                "roofline_blend": roofline_blend,
                "latency_ms_single_image": latency_single,
                "kernels": kernels,
                "blend": {"ms_per_step": round(blend_ms, 4),
                          "alg_GB": round(blend_alg / 1e9, 3),
                          "GBps": None if blend_ms <= 0 else round(blend_alg / 1e9 / (blend_ms / 1e3), 1),
                          "frac_of_peak": None if blend_ms <= 0 else round(blend_alg / 1e9 / (blend_ms / 1e3) / HBM_PEAK_GBS, 4),
                          "survey_model_GBps": None if blend_ms <= 0 else round(alg["_survey_blend_model"] / div / 1e9 / (blend_ms / 1e3), 1)},
                "summary": {"gpu_kernel_ms_per_step": round(gpu_ms, 4), "blend_ms_per_step": round(blend_ms, 4),
                            "alg_GB_per_step": round(total_alg / 1e9, 3),
                            "blend_GBps_vs_survey_model": None if blend_ms <= 0 else
                            round(alg["_survey_blend_model"] / 1e9 / (blend_ms / 1e3), 1),
                            "whole_step_alg_GBps": None if ms_per_step <= 0 else round(total_alg / 1e9 / (ms_per_step / 1e3), 1)},
            })
    pipe.close()
    del pipe, reference, image, t_src
    torch.cuda.empty_cache()
    if out is not None and detailed:
        out["cpu_baseline"] = out["parity"] = None
        if world == 1 and not args.no_cpu_baseline:
            # the k-d workloads time the grid geometry of the same canvas (same pixels, same kernels on the CPU side)
            geo_grid = dp.workload_geometry(workload.replace("-kd", ""))
            sample, out["cpu_baseline"] = cpu_baseline(src_ref, geo_grid)
            out["parity"] = parity_vs_oracle(sample, geo_grid, local_rank)   # the oracle as checker, never in a timed region
            del sample
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--workload", default="200MP", choices=WORKLOAD_CHOICES)
    ap.add_argument("--mode", default="strips", choices=["strips", "batch"],
                    help="strips: one image over all ranks (strong scaling, the BASELINE metric); "
                         "batch: one image per rank, no data-path communication (config 4, weak scaling)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the timed path computed in its last step as DIR/<name>.npy (float32 / float64, ~25 MB): "
                         "a fixed, seeded sample of the canvas bytes with their indices, the canvas's row and column sums, "
                         "and the scores")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline figure: per-kernel table and roofline (kernel timing in the warm-up "
                         "and around the dominant kernel in the timed region), PCIe copies, single-image latency, the "
                         "--sweep workloads, the CPU baseline and the parity check against the oracle")
    ap.add_argument("--sweep", default="100MP,150MP",
                    help="with --full: comma list of further workloads measured briefly after the main one and reported in the "
                         "`sweep` object of the same JSON line (north_star: 100 / 150 / 200 MP); '' or 'none' to skip")
    ap.add_argument("--sweep-steps", type=int, default=8)
    ap.add_argument("--no-pcie", action="store_true",
                    help="with --full: skip the host->device (inputs) / device->host (canvas) timing that N=1 runs report "
                         "beside the resident rate")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the parity check")
    ap.add_argument("--lpips", default="none", choices=["none", "alex", "vgg"],
                    help="BASELINE config 5 whole: add LPIPS(canvas, reference) of this backbone to every timed image (seeded "
                         "synthetic weights -- the pretrained ones are not available offline; timing does not depend on their "
                         "values); one GPU or batch mode only.  Not part of the default line.")
    ap.add_argument("--no-prof", action="store_true", help="with --full: skip the per-kernel HIP-event timing")
    ap.add_argument("--deadline-s", type=float, default=900.0,
                    help="self-launched N > 1 runs: after this many seconds the launcher terminates the ranks still running, "
                         "prints every rank's last completed stage and exits 124")
    args = ap.parse_args()

    if args.gpus < 1:
        print("bench.py: --gpus must be >= 1", file=sys.stderr)
        return 2
    if args.steps < 1 or args.warmup < 0:
        print("bench.py: --steps must be >= 1 and --warmup >= 0", file=sys.stderr)
        return 2
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        return _launch_ranks(args.gpus, sys.argv[1:], args.deadline_s)   # children only; this process never touches the GPU
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: launched with WORLD_SIZE={world} but --gpus {args.gpus}", file=sys.stderr)
        return 2

    _stage("process started")
    if str(rank) in os.environ.get("SR_BENCH_TEST_HANG_RANKS", "").split(","):   # tests: the launcher's deadline path
        time.sleep(600)
    import torch
    import torch.distributed as dist

    if not torch.cuda.is_available():
        print("bench.py: no GPU visible -- the HIP path has no CPU fallback", file=sys.stderr)
        return 2
    # SR_DIST_BACKEND=gloo is the single-GPU rehearsal of the multi-rank path (ranks share one card, rows staged
    # through the host); the measured configuration is always RCCL ("nccl"), one rank per GPU.
    backend = os.environ.get("SR_DIST_BACKEND", "nccl")
    if backend != "nccl":
        local_rank = local_rank % max(torch.cuda.device_count(), 1)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    _stage("torch imported, GPU visible")
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
    _stage(f"process group ({backend}, world {world}) initialised")
    state = (world, rank, local_rank, backend, dev)

    out = run_workload(args, args.workload, args.steps, args.warmup, args.full, state, args.dump_outputs)
    sweep = [w for w in args.sweep.split(",") if w and w != "none" and w != args.workload] if args.full else []
    sweep_out = {}
    for wl in sweep:
        if wl not in WORKLOAD_CHOICES:
            print(f"bench.py: unknown sweep workload {wl!r}", file=sys.stderr)
            return 2
        r = run_workload(args, wl, max(1, args.sweep_steps), min(args.warmup, 2), False, state)
        if r is not None:
            sweep_out[wl] = {k: r[k] for k in ("value", "unit", "ms_per_step", "steps", "warmup", "step_ms", "quality")}
            sweep_out[wl]["workload"] = r["config"]["workload"]
    if rank == 0:
        if args.full:
            out["sweep"] = sweep_out
        print(json.dumps(out), flush=True)
    _stage("JSON line printed")
    if world > 1:
        dist.destroy_process_group()
    _stage("done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
