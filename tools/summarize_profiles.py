#!/usr/bin/env python3
"""Turns ONE collection made by tools/collect_profiles.sh (gpurun_out/profiles_<tag>/) into the committed summaries:
    profiles/<prefix>_kernel_stats.csv   rocprofv3 --kernel-trace --stats summary (same command as the bench line)
    profiles/<prefix>_traffic.json       per-kernel HBM bytes PER LAUNCH and per step from FETCH_SIZE / WRITE_SIZE
    profiles/<prefix>_bench.json         the bench line of the same build (its roofline pointed at these counters)
    profiles/<prefix>_bench_<wl>.json    the other workloads

Rules (round-2 verdict, weak #3):
  * only the run directory named in <collection>/run_id.txt is read -- gpurun MERGES gpurun_out/, so an older collection
    under the same tag may still sit beside the new one; every counter CSV must come from one build (the bench line's
    source digest is recorded);
  * every kernel is divided by ITS OWN launch count (per launch); per step = that x its launches per step, where the steps
    of the run are the launches of k_tile_extract in the SAME run (one per step by construction, cross-checked);
  * reads are reported twice: `2x` = FETCH_SIZE x 2 as MI355X_MICROARCH.md prescribes for gfx950, `calibrated` = FETCH_SIZE x
    the factor measured on k_tile_extract (a pure copy whose byte count is known);
  * the script FAILS when a bench kernel family's corrected traffic is below 0.9 x its algorithmic bytes (that can only be
    a bookkeeping error).
  * bench.py's byte model counts G_1 as fp32 (down_l0 6.75 B, final_gather 8.5 B per tile pixel).  A build that keeps G_1 of
    u8 tiles in 16 bits (sr_blend_plan_g1_format) writes and reads 1.5 B per tile pixel less in each of the two families: a
    third argument `g1u16` takes them off the model the refusal above compares with (the bench line's own GBps fields keep
    bench.py's model and so understate such a build).
usage: tools/summarize_profiles.py <tag> <prefix> [g1u16]      e.g.  r03a  r03_a
"""
import collections
import csv
import glob
import json
import os
import shutil
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as bench_mod  # noqa: E402

tag, prefix = sys.argv[1], sys.argv[2]
src = f"gpurun_out/profiles_{tag}"
run_id = open(f"{src}/run_id.txt").read().strip()
meta = json.load(open(f"{src}/{run_id}/meta.json"))
run = f"{src}/{run_id}"
os.makedirs("profiles", exist_ok=True)
shutil.copy(f"{run}/kernel_stats.csv", f"profiles/{prefix}_kernel_stats.csv")
bench = json.load(open(f"{run}/bench.json"))


def counter(name):
    """-> kernel -> list of per-launch counter values (this run only)."""
    agg = collections.defaultdict(list)
    files = glob.glob(f"{run}/pmc_{name}/**/*_counter_collection.csv", recursive=True)
    if not files:
        sys.exit(f"no counter CSV for {name} under {run}")
    for f in files:
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] == name:
                agg[r["Kernel_Name"].split("(")[0].replace("void ", "")].append(float(r["Counter_Value"]))
    return agg


fetch, write = counter("FETCH_SIZE"), counter("WRITE_SIZE")
tile_px, canvas_px = bench["config"]["tile_pixels"], bench["config"]["canvas_pixels"]
ext = fetch.get("k_tile_extract")
if not ext:
    sys.exit("k_tile_extract missing from the FETCH_SIZE pass")
known_read = 3.0 * tile_px                      # k_tile_extract reads exactly the tile pixels once per launch
# Steps the PMC command ran = launches of k_tile_extract in THIS run (exactly one per step by construction: warm-up, timed
# steps and the single-image latency pass all go through the tile stage once); cross-checked against the command line.
pmc_steps = len(ext)
if pmc_steps < meta["pmc_steps"] + meta["pmc_warmup"] or len(write.get("k_tile_extract", [])) != pmc_steps:
    sys.exit(f"k_tile_extract ran {pmc_steps} times in the FETCH pass, {len(write.get('k_tile_extract', []))} in the WRITE pass; the "
             f"command asked for at least {meta['pmc_steps'] + meta['pmc_warmup']} steps")
cal = known_read / (sum(ext) / len(ext) * 1024.0)
out = {"format": 2, "run_id": run_id, "build_digest": meta.get("build_digest"),
       "pmc_command_steps": pmc_steps, "fetch_calibration_factor": cal,
       "note": "per_launch = counter sum over the kernel's launches / its own launch count; per_step = sum / steps of the PMC "
               "command; read_2x = FETCH_SIZE*1024*2 (MI355X_MICROARCH.md: gfx950 reports half the bytes of wide streaming "
               "reads), read = FETCH_SIZE*1024*factor calibrated on k_tile_extract; write = WRITE_SIZE*1024",
       "kernels": {}}
for k in sorted(set(fetch) | set(write)):
    if not k.startswith("k_"):
        continue
    nf, nw = len(fetch.get(k, [])), len(write.get(k, []))
    if nf and nw and nf != nw:
        sys.exit(f"{k}: {nf} launches in the FETCH pass, {nw} in the WRITE pass -- not one build / one command")
    n = max(nf, nw)
    raw, wr = sum(fetch.get(k, [])) * 1024.0, sum(write.get(k, [])) * 1024.0
    rec = {}
    for label, div in (("per_launch", n), ("per_step", pmc_steps)):
        rec[label] = {"read": raw * cal / div, "read_2x": raw * 2.0 / div, "write": wr / div,
                      "total": (raw * cal + wr) / div, "total_2x": (raw * 2.0 + wr) / div}
    rec["launches"] = n
    rec["launches_per_step"] = n / pmc_steps
    out["kernels"][k] = rec

# consistency: corrected traffic of a bench family can not be below its algorithmic bytes
geo = type("G", (), {"tile_pixels": tile_px, "canvas_pixels": canvas_px})
alg = dict(bench_mod.algorithmic_bytes(geo))
if len(sys.argv) > 3 and sys.argv[3] == "g1u16":
    for fam in ("down_l0", "final_gather"):
        alg[fam] -= 1.5 * tile_px
fam_tot = collections.defaultdict(float)
for k, rec in out["kernels"].items():
    fam = bench_mod.family_of(k)
    if fam:
        fam_tot[fam] += rec["per_step"]["total_2x"]
out["families"] = {}
bad = []
for fam, tot in sorted(fam_tot.items()):
    ratio = tot / alg[fam]
    out["families"][fam] = {"traffic_2x_per_step": tot, "alg_bytes_per_step": alg[fam], "ratio": ratio}
    if ratio < 0.9:
        bad.append(f"{fam}: {tot / 1e9:.3f} GB counted (2x-corrected) < 0.9 x {alg[fam] / 1e9:.3f} GB algorithmic")
json.dump(out, open(f"profiles/{prefix}_traffic.json", "w"), indent=1)
if bad:
    sys.exit("traffic below algorithmic bytes -- bookkeeping error:\n  " + "\n  ".join(bad))

# the bench line of this collection was printed before this summary existed: point its rooflines at these counters
roof = bench.get("roofline") or {}
fam = roof.get("kernel")
if fam in fam_tot:
    lps = sum(rec["launches_per_step"] for k, rec in out["kernels"].items() if bench_mod.family_of(k) == fam)
    roof["traffic"] = fam_tot[fam] / max(lps, 1)
    roof["traffic_calibrated"] = sum(rec["per_step"]["total"] for k, rec in out["kernels"].items()
                                     if bench_mod.family_of(k) == fam) / max(lps, 1)
    roof["traffic_source"], roof["traffic_build_digest"] = f"{prefix}_traffic.json", out["build_digest"]
    roof["traffic_stale"] = (bench.get("build_digest") != out["build_digest"]) if bench.get("build_digest") else None
rb = bench.get("roofline_blend") or {}
if rb and all(f in fam_tot for f in bench_mod.BLEND_FAMILIES):
    rb["traffic"] = sum(fam_tot[f] for f in bench_mod.BLEND_FAMILIES)
    rb["traffic_calibrated"] = sum(rec["per_step"]["total"] for k, rec in out["kernels"].items()
                                   if bench_mod.family_of(k) in bench_mod.BLEND_FAMILIES)
    if rb.get("ms"):
        rb["achieved_counter_GBps"] = round(rb["traffic_calibrated"] / 1e9 / (rb["ms"] / 1e3), 1)
        rb["frac_counter"] = round(rb["achieved_counter_GBps"] / bench_mod.HBM_PEAK_GBS, 4)
    rb["traffic_source"] = f"{prefix}_traffic.json"
    rb["traffic_stale"] = (bench.get("build_digest") != out["build_digest"]) if bench.get("build_digest") else None
json.dump(bench, open(f"profiles/{prefix}_bench.json", "w"), indent=1)
for f in glob.glob(f"{run}/bench_*.json"):
    name = os.path.basename(f)
    if name == "bench_under_trace.json" or os.path.getsize(f) == 0:
        continue
    shutil.copy(f, f"profiles/{prefix}_{name}")
# cross-check: the trace's average duration of the dominant kernel vs the bench line's own HIP-event time
for r in csv.DictReader(open(f"profiles/{prefix}_kernel_stats.csv")):
    if bench_mod.family_of(r["Name"]) == fam:
        print(f"[check] {fam}: rocprofv3 average {float(r['AverageNs']) / 1e6:.4f} ms over {r['Calls']} calls; bench line: "
              f"{roof.get('avg_launch_ms')} ms in region, {roof.get('standalone', {}).get('avg_launch_ms')} ms standalone")
print(json.dumps(out["families"], indent=1))
