#!/usr/bin/env python3
"""What aggregating several volumes per call buys at the C2 shape (5 views,
1920x1080, D = 128, K = 5, S = 32): interleaved A/Bs in one process.

Leg "call": the five views' NCC volumes in one [5, D, H, W] buffer.  Per mask
(1 horizontal, 4 vertical, 16 diagonal, 15, 255), alternately in the same loop,
(a) N mvs_sgm8_d calls back to back and (b) one mvs_sgm8_batch_d over the same N
volumes, HIP events around each; N = 5 for every mask, N = 2 and 3 as well for
masks 15 and 255.  Compulsory traffic: a path reads vol once and writes agg
once, and every path after the first reads agg as well: (3 n - 1) N passes of
4 D H W bytes for n paths.  The achieved bytes per second is that over the
time; a streamed copy reaches 6.3 TB/s on this chip.  Before timing a mask the
two forms' aggregates are compared bit for bit.

Leg "step": the whole step, Pipeline(sgm=True) two-pass and fused, sgm_paths 15
and 255, with sgm_batch 1 and 5 in alternating blocks of steps, each block
device-synchronised before and after; a setting's time is the mean over its
blocks, the spread their min..max.

Writes profiles/sgm_batch/ab.json.

    python scripts/bench_sgm_batch.py [--calls 20] [--blocks 3] [--steps 4] [--warmup 2] [--legs call,step]
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

from cl_multiview_stereo_amd import _lib, params, synth  # noqa: E402
from cl_multiview_stereo_amd.engine import Engine  # noqa: E402
from cl_multiview_stereo_amd.pipeline import Pipeline  # noqa: E402

C2 = dict(aw=5, W=1920, H=1080, S=32, dmax=127, K=5, nh=4)
CASES = [(1, 5), (4, 5), (16, 5), (15, 5), (255, 5), (15, 2), (15, 3), (255, 2), (255, 3)]  # (mask, N)
COPY_TB_PER_S = 6.3


def passes(mask):
    n = bin(mask).count("1")
    return 3 * n - 1  # n reads of vol, n writes of agg, n - 1 reads of agg


def summary(xs):
    return {"ms": round(sum(xs) / len(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def timed(fn):
    x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    x.record()
    fn()
    y.record()
    return x, y


def block_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def leg_call(e, a, cfg, st, rgbx, res):
    W, H, aw, D = cfg["W"], cfg["H"], cfg["aw"], cfg["dmax"] + 1
    cam = Pipeline(e, st, W, H, pixel_cost="ncc").cam
    _, l8 = e.cvt(rgbx)
    box = e.box_stats(l8, cfg["K"])
    vols = e.empty((aw, D, H, W), torch.float32)
    for z in range(aw):
        e.ncc_volume(l8, box, cam, z, cfg["K"], out=vols[z])
    one, bat = torch.empty_like(vols), torch.empty_like(vols)
    unit = 4.0 * D * H * W
    res["call"] = {"what": "N mvs_sgm8_d calls back to back (calls) against one mvs_sgm8_batch_d (batch) over the "
                           "same N volumes", "bytes_per_pass": unit, "streamed_copy_tb_per_s": COPY_TB_PER_S}
    for paths, N in CASES:
        def calls():
            for z in range(N):
                _lib.check(e.L.mvs_sgm8_d(e.ctx, W, H, D, vols[z].data_ptr(), 0.1, 0.8, paths, one[z].data_ptr()),
                           "mvs_sgm8_d")

        def batch():
            e.sgm_batch(vols[:N], 0.1, 0.8, paths, out=bat[:N])

        for _ in range(2):
            calls()
            batch()
        equal = bool(torch.equal(one[:N].view(torch.int32), bat[:N].view(torch.int32)))
        if not equal:
            raise SystemExit(f"paths {paths} N {N}: the batched aggregate differs from the single calls'")
        ev = {"calls": [], "batch": []}
        for _ in range(a.calls):  # calls, batch, calls, batch, ...
            ev["calls"].append(timed(calls))
            ev["batch"].append(timed(batch))
        torch.cuda.synchronize()
        r = {"bit_identical": equal, "compulsory_gb": round(passes(paths) * N * unit / 1e9, 3)}
        for k in ("calls", "batch"):
            s = summary([x.elapsed_time(y) for x, y in ev[k]])
            s["achieved_tb_per_s"] = round(passes(paths) * N * unit / (s["ms"] * 1e-3) / 1e12, 3)
            s["share_of_streamed_copy"] = round(s["achieved_tb_per_s"] / COPY_TB_PER_S, 3)
            r[k] = s
        r["batch_over_calls"] = round(r["batch"]["ms"] / r["calls"]["ms"], 4)
        # beyond the spread: the two forms' min..max ranges do not meet
        r["ranges_disjoint"] = bool(r["batch"]["max"] < r["calls"]["min"] or r["calls"]["max"] < r["batch"]["min"])
        res["call"][f"paths_{paths}_N{N}"] = r
        print("call", paths, N, json.dumps(r), flush=True)


def leg_step(e, a, cfg, st, rgbx, res):
    W, H, aw = cfg["W"], cfg["H"], cfg["aw"]
    res["step"] = {"what": "whole Pipeline(sgm=True) step, sgm_batch 1 against 5"}
    for fused in (False, True):
        for paths in (15, 255):
            fns = {}
            for B in (1, aw):
                p = Pipeline(e, st, W, H, pixel_cost="ncc", fused=fused, sgm=True, sgm_paths=paths, sgm_batch=B)
                fns[B] = (lambda p=p: p.exe_pipeline(rgbx))
            for B in fns:
                block_ms(fns[B], a.warmup)
            t = {B: [] for B in fns}
            for _ in range(a.blocks):  # 1, 5, 1, 5, ...
                for B in fns:
                    t[B].append(block_ms(fns[B], a.steps))
            s1, s5 = summary(t[1]), summary(t[aw])
            r = {"sgm_batch_1": s1, f"sgm_batch_{aw}": s5, "difference_ms": round(s5["ms"] - s1["ms"], 4),
                 "ranges_disjoint": bool(s5["max"] < s1["min"] or s1["max"] < s5["min"])}
            res["step"][f"{'fused' if fused else 'two_pass'}_paths_{paths}"] = r
            print("step", fused, paths, json.dumps(r), flush=True)
            del fns, p
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="call,step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm_batch", "ab.json"))
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
           "method": f"call: {a.calls} alternating repeats per case after 2 warm-up repeats, HIP events around each; "
                     f"step: {a.blocks} alternating blocks of {a.steps} steps per setting after {a.warmup} warm-up "
                     "steps each, host clock around device-synchronised blocks; ms = mean, min / max = spread"}
    legs = a.legs.split(",")
    if "call" in legs:
        leg_call(e, a, cfg, st, rgbx, res)
        torch.cuda.empty_cache()
    if "step" in legs:
        leg_step(e, a, cfg, st, rgbx, res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", os.path.relpath(a.out, ROOT))


if __name__ == "__main__":
    main()
