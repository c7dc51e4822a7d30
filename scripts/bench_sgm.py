#!/usr/bin/env python3
"""What the semi-global aggregation costs at the C2 shape (5 views, 1920x1080,
D = 128, K = 5, S = 32): an interleaved A/B in one process.

Leg "step": the two-pass step, Pipeline(fused=False), with sgm=False and
sgm=True in alternating blocks of steps, each block device-synchronised before
and after; a setting's time is the mean over its blocks, the spread their
min..max.  The sgm=False leg runs no code of the aggregation: it is the step
`bench.py --two-pass` times, for comparison with the parent commit.

Leg "call": mvs_sgm_d alone on one view's volume (HIP events around each call),
for each single path and for paths=15, against its compulsory traffic: a path
reads vol once and writes agg once, and every path after the first reads agg
as well, so a single path moves 2 and paths=15 moves 4 + 4 + 3 = 11 passes of
4 D H W bytes.  The achieved bytes per second is that over the call's time.

Writes profiles/sgm/ab.json.

    python scripts/bench_sgm.py [--blocks 5] [--steps 4] [--warmup 2] [--calls 20]
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
from cl_multiview_stereo_amd.pipeline import Pipeline  # noqa: E402

C2 = dict(aw=5, W=1920, H=1080, S=32, dmax=127, K=5, nh=4)
PASSES = {1: 2, 2: 2, 4: 2, 8: 2, 15: 11}  # of 4 D H W bytes: vol reads + agg writes + agg reads


def block_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def summary(xs):
    return {"ms": round(sum(xs) / len(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm", "ab.json"))
    a = ap.parse_args()
    cfg = C2
    W, H, aw, D = cfg["W"], cfg["H"], cfg["aw"], cfg["dmax"] + 1
    e = Engine(0)
    st = params.Settings(spixl_size=cfg["S"], array_width=aw, array_height=1, min_disp=0, max_disp=cfg["dmax"], inc=1,
                         neib_hor=cfg["nh"], neib_ver=0, bl_ratio=1.0, window=cfg["K"], cost="ncc")
    stack, _ = synth.make_stack(W, H, aw, 1, 0, cfg["dmax"], 1.0, 0x5EED + 2)  # bench.py's stack
    rgbx = torch.from_numpy(stack).to(e.device)
    res = {"device": torch.cuda.get_device_name(0), "library": e.L.mvs_version().decode(),
           "shape": f"{aw} views {W}x{H}, D = {D}, K = {cfg['K']}",
           "method": f"step: {a.blocks} alternating blocks of {a.steps} steps per setting after {a.warmup} warm-up "
                     f"steps each, host clock around device-synchronised blocks; call: {a.calls} calls per mask, HIP "
                     "events around each; ms = mean, min / max = spread"}
    # ---- the two-pass step, sgm off and on
    fns = {}
    for on in (False, True):
        p = Pipeline(e, st, W, H, pixel_cost="ncc", fused=False, sgm=on)
        fns[on] = (lambda p=p: p.exe_pipeline(rgbx))
    for on in (False, True):
        block_ms(fns[on], a.warmup)
    t = {False: [], True: []}
    for _ in range(a.blocks):  # off, on, off, on, ...
        for on in (False, True):
            t[on].append(block_ms(fns[on], a.steps))
    off, on = summary(t[False]), summary(t[True])
    res["step"] = {"what": "whole Pipeline(fused=False) step", "sgm_off": off, "sgm_on": on,
                   "difference_ms": round(on["ms"] - off["ms"], 4),
                   "difference_ms_per_view": round((on["ms"] - off["ms"]) / aw, 4)}
    print("step", json.dumps(res["step"]), flush=True)
    # ---- the call alone, the centre view's volume
    cam = p.cam
    _, l8 = e.cvt(rgbx)
    box = e.box_stats(l8, cfg["K"])
    vol = e.ncc_volume(l8, box, cam, aw // 2, cfg["K"])
    agg = torch.empty_like(vol)
    unit = 4.0 * D * H * W
    res["call"] = {"what": "mvs_sgm_d on one view's volume", "bytes_per_pass": unit}
    for paths in (1, 2, 4, 8, 15):
        for _ in range(2):
            e.sgm(vol, 0.1, 0.8, paths, out=agg)
        evs = []
        for _ in range(a.calls):
            x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            x.record()
            e.sgm(vol, 0.1, 0.8, paths, out=agg)
            y.record()
            evs.append((x, y))
        torch.cuda.synchronize()
        s = summary([x.elapsed_time(y) for x, y in evs])
        s["compulsory_gb"] = round(PASSES[paths] * unit / 1e9, 3)
        s["achieved_tb_per_s"] = round(PASSES[paths] * unit / (s["ms"] * 1e-3) / 1e12, 3)
        res["call"][f"paths_{paths}"] = s
        print("call", paths, json.dumps(s), flush=True)
    lev = e.levels_dev(cam)
    raw, _ = e.wta(vol, lev)
    win, _ = e.wta(agg, lev)
    res["call"]["winner_moved_share"] = round(float((raw != win).float().mean()), 4)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(a.out, ROOT))


if __name__ == "__main__":
    main()
