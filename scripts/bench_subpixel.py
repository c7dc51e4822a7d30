#!/usr/bin/env python3
"""What the sub-level disparity pass costs: an interleaved A/B in one process.

Leg "c2": the C2 step (5 views, 1920x1080, D = 128, K = 5, S = 32) through
Pipeline(fused=True), subpixel=False and subpixel=True in alternating blocks
of steps.  Leg "c5_sweep": C5's per-pixel sweep stage alone (5 views,
4096x3072, D = 256, K = 7: window planes + fused sweep, with and without the
post-pass).  Each leg also times the post-pass call by itself (HIP events).
Every block is device-synchronised before and after; a leg's time is the mean
over its blocks, the spread their min..max.

Writes profiles/subpixel/ab.json with both step times, their difference, the
spread, and the parent commit's C2 step (profiles/r06/bench_default.json) for
comparison with the subpixel=False leg.

    python scripts/bench_subpixel.py [--blocks 5] [--steps 5] [--warmup 3] [--legs c2,c5_sweep]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cl_multiview_stereo_amd import params, synth  # noqa: E402
from cl_multiview_stereo_amd.engine import Engine  # noqa: E402
from cl_multiview_stereo_amd.pipeline import Pipeline, PixelSweep  # noqa: E402

LEGS = {
    "c2": dict(aw=5, W=1920, H=1080, S=32, dmax=127, K=5, nh=4, whole_step=True),
    "c5_sweep": dict(aw=5, W=4096, H=3072, S=40, dmax=255, K=7, nh=4, whole_step=False),
}


def block_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def summary(xs):
    return {"ms": round(sum(xs) / len(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "blocks": len(xs)}


def run_leg(e, name, cfg, blocks, steps, warmup):
    W, H, aw = cfg["W"], cfg["H"], cfg["aw"]
    st = params.Settings(spixl_size=cfg["S"], array_width=aw, array_height=1, min_disp=0, max_disp=cfg["dmax"], inc=1,
                         neib_hor=cfg["nh"], neib_ver=0, bl_ratio=1.0, window=cfg["K"], cost="ncc")
    stack, _ = synth.make_stack(W, H, aw, 1, 0, cfg["dmax"], 1.0, 0x5EED + 2)  # bench.py's stack
    rgbx = torch.from_numpy(stack).to(e.device)
    fns = {}
    if cfg["whole_step"]:
        for sub in (False, True):
            p = Pipeline(e, st, W, H, pixel_cost="ncc", fused=True, subpixel=sub)
            fns[sub] = (lambda p=p: p.exe_pipeline(rgbx))
        cam = p.cam
        lab, l8 = e.cvt(rgbx)
    else:
        cam = Pipeline(e, st, W, H, pixel_cost=None).cam
        lab, l8 = e.cvt(rgbx)
        for sub in (False, True):
            ps = PixelSweep(e, cam, W, H, "ncc", cfg["K"], fused=True, subpixel=sub)
            fns[sub] = (lambda ps=ps: ps.run(lab, l8, 0, aw))
    for sub in (False, True):
        block_ms(fns[sub], warmup)
    t = {False: [], True: []}
    for _ in range(blocks):  # off, on, off, on, ...
        for sub in (False, True):
            t[sub].append(block_ms(fns[sub], steps))
    # the post-pass call by itself
    box = e.box_stats(l8, cfg["K"])
    disp, _ = e.ncc_wta_range(l8, box, cam, 0, aw, cfg["K"], want_conf=False)
    out = torch.empty_like(disp)
    e.ncc_sub_range(l8, box, cam, 0, aw, cfg["K"], disp=disp, out=out)
    evs = []
    for _ in range(blocks * steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        e.ncc_sub_range(l8, box, cam, 0, aw, cfg["K"], disp=disp, out=out)
        b.record()
        evs.append((a, b))
    torch.cuda.synchronize()
    call = [a.elapsed_time(b) for a, b in evs]
    moved = float((out != disp).float().mean())
    off, on = summary(t[False]), summary(t[True])
    return {
        "what": ("whole Pipeline(fused=True) step" if cfg["whole_step"] else "PixelSweep(fused=True).run: window planes + "
                 "fused sweep") + f", {aw} views {W}x{H}, D = {cfg['dmax'] + 1}, K = {cfg['K']}",
        "steps_per_leg": blocks * steps,
        "subpixel_off": off,
        "subpixel_on": on,
        "difference_ms": round(on["ms"] - off["ms"], 4),
        "difference_share_of_step": round((on["ms"] - off["ms"]) / off["ms"], 4),
        "post_pass_call_ms": summary(call),
        "pixels_moved_share": round(moved, 4),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default="c2,c5_sweep")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subpixel", "ab.json"))
    a = ap.parse_args()
    if a.blocks * a.steps < 20:
        ap.error("at least 20 timed steps per leg (blocks x steps)")
    e = Engine(0)
    res = {"device": torch.cuda.get_device_name(0), "library": e.L.mvs_version().decode(),
           "method": f"{a.blocks} alternating blocks of {a.steps} steps per setting after {a.warmup} warm-up steps "
                     "each, host clock around device-synchronised blocks; ms = mean over blocks, min / max = spread"}
    for name in a.legs.split(","):
        res[name] = run_leg(e, name, LEGS[name], a.blocks, a.steps, a.warmup)
        print(name, json.dumps(res[name]), flush=True)
        torch.cuda.empty_cache()
    parent = os.path.join(ROOT, "profiles", "r06", "bench_default.json")
    if "c2" in res and os.path.exists(parent):
        ms = json.load(open(parent)).get("ms_per_step")
        res["parent_c2_ms_per_step"] = {"ms": ms, "source": "profiles/r06/bench_default.json (bench.py, 20 steps)"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(a.out, ROOT))


if __name__ == "__main__":
    main()
