#!/usr/bin/env python3
"""What the diagonal paths of the semi-global aggregation cost at the C2 shape
(1920x1080, D = 128, K = 5): mvs_sgm8_d alone on the centre view's volume, HIP
events around each call, for each diagonal path (masks 16, 32, 64, 128), the
four together (240) and all eight (255), and in the same run for comparison
the vertical path (4) and the four axis-aligned ones (15) through mvs_sgm_d.

Compulsory traffic: a path reads vol once and writes agg once, and every path
after the first reads agg as well: 2 passes of 4 D H W bytes for one path,
4 + 4 + 3 = 11 for four, 8 + 8 + 7 = 23 for eight.  A diagonal path moves the
same compulsory bytes as a vertical one; `ratio_to_vertical` is its time over
mask 4's of this run.

Writes profiles/sgm8/ab.json.

    python scripts/bench_sgm8.py [--calls 20] [--out FILE] [--masks 1,4,16,15,255]

--masks: other masks than the default set (an A/B of two builds of the library
through MVS_LIB on a few of them); the ratios and the winners' share are
written for the masks they need.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cl_multiview_stereo_amd import params, synth  # noqa: E402
from cl_multiview_stereo_amd.engine import Engine  # noqa: E402
from cl_multiview_stereo_amd.pipeline import Pipeline  # noqa: E402

C2 = dict(aw=5, W=1920, H=1080, S=32, dmax=127, K=5, nh=4)
MASKS = (4, 15, 16, 32, 64, 128, 240, 255)


def passes(mask):
    n = bin(mask).count("1")
    return 3 * n - 1  # n reads of vol, n writes of agg, n - 1 reads of agg


def summary(xs):
    return {"ms": round(sum(xs) / len(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm8", "ab.json"))
    ap.add_argument("--masks", default=",".join(map(str, MASKS)))
    a = ap.parse_args()
    masks = tuple(int(m) for m in a.masks.split(","))
    cfg = C2
    W, H, aw, D = cfg["W"], cfg["H"], cfg["aw"], cfg["dmax"] + 1
    e = Engine(0)
    st = params.Settings(spixl_size=cfg["S"], array_width=aw, array_height=1, min_disp=0, max_disp=cfg["dmax"], inc=1,
                         neib_hor=cfg["nh"], neib_ver=0, bl_ratio=1.0, window=cfg["K"], cost="ncc")
    stack, _ = synth.make_stack(W, H, aw, 1, 0, cfg["dmax"], 1.0, 0x5EED + 2)  # bench.py's stack
    rgbx = torch.from_numpy(stack).to(e.device)
    cam = Pipeline(e, st, W, H, pixel_cost="ncc").cam
    _, l8 = e.cvt(rgbx)
    box = e.box_stats(l8, cfg["K"])
    vol = e.ncc_volume(l8, box, cam, aw // 2, cfg["K"])
    agg = torch.empty_like(vol)
    unit = 4.0 * D * H * W
    res = {"device": torch.cuda.get_device_name(0), "library": e.L.mvs_version().decode(),
           "shape": f"one view's volume, {W}x{H}, D = {D}, K = {cfg['K']}",
           "method": f"{a.calls} calls per mask after 2 warm-up calls, HIP events around each; ms = mean, min / max = "
                     "spread; masks up to 15 go through mvs_sgm_d, larger ones through mvs_sgm8_d",
           "bytes_per_pass": unit, "call": {}}
    lev = e.levels_dev(cam)
    for paths in masks:
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
        s["compulsory_gb"] = round(passes(paths) * unit / 1e9, 3)
        s["achieved_tb_per_s"] = round(passes(paths) * unit / (s["ms"] * 1e-3) / 1e12, 3)
        if paths in (15, 255):  # the winners, for the share of pixels the diagonal paths move
            s["_win"] = e.wta(agg, lev)[0].clone()
        res["call"][f"paths_{paths}"] = s
        print("call", paths, json.dumps({k: v for k, v in s.items() if k != "_win"}), flush=True)
    if 4 in masks:
        vert = res["call"]["paths_4"]["ms"]
        for paths in (16, 32, 64, 128):
            if paths in masks:
                res["call"][f"paths_{paths}"]["ratio_to_vertical"] = round(res["call"][f"paths_{paths}"]["ms"] / vert, 3)
    wins = [res["call"][f"paths_{m}"].pop("_win") for m in (15, 255) if m in masks]
    if len(wins) == 2:
        res["winner_8_paths_differs_from_4_paths_share"] = round(float((wins[0] != wins[1]).float().mean()), 4)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(a.out, ROOT))


if __name__ == "__main__":
    main()
