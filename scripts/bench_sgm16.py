#!/usr/bin/env python3
"""What the 16-bit aggregation costs and saves at the C2 shape (5 views,
1920x1080, D = 128, K = 5, S = 32): interleaved A/Bs in one process, float32
(mvs_sgm8_batch_d, the parent's call) against uint16 (mvs_sgm8_u16_batch_d).

Leg "call": the five views' NCC volumes in one float32 [5, D, H, W] buffer and,
quantised, in one uint16 buffer.  Per mask (1 horizontal, 4 vertical, 16
diagonal, 15, 255), alternately in the same loop, one float32 call and one
uint16 call over the same N = 5 volumes, HIP events around each; median and
min..max over the repeats.  Compulsory traffic as in bench_sgm_batch.py:
(3 n - 1) N passes of D H W elements for n paths, 4 or 2 bytes each.  Before a
mask is timed, element 0 of the uint16 batch is compared bit for bit with a
call of N = 1 on it.

Leg "pass": mvs_quant_u16_d (reads 4, writes 2 bytes per cell) and
mvs_wta_u16_d (reads 2 bytes per cell) alone on one volume, beside mvs_wta_d
(4 bytes per cell), with their bytes per second against the streamed-copy
figure.

Leg "step": the whole step, Pipeline(sgm=True, sgm_batch=5) two-pass and fused,
sgm_paths 15 and 255, with sgm_dtype f32 and u16 in alternating blocks of
steps, each block device-synchronised before and after; a setting's time is
the mean over its blocks, the spread their min..max.  The share of pixels whose
disp_agg differs between the two dtypes is reported per setting.

Writes profiles/sgm16/ab.json.

    python scripts/bench_sgm16.py [--calls 20] [--blocks 3] [--steps 4] [--warmup 2] [--legs call,pass,step]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cl_multiview_stereo_amd import params, synth  # noqa: E402
from cl_multiview_stereo_amd.engine import Engine  # noqa: E402
from cl_multiview_stereo_amd.pipeline import Pipeline  # noqa: E402

C2 = dict(aw=5, W=1920, H=1080, S=32, dmax=127, K=5, nh=4)
MASKS = [1, 4, 16, 15, 255]
COPY_TB_PER_S = 6.3
P1F, P2F, P1U, P2U = 0.1, 0.8, 205, 1638


def passes(mask):
    n = bin(mask).count("1")
    return 3 * n - 1  # n reads of vol, n writes of agg, n - 1 reads of agg


def summary(xs):
    return {"median_ms": round(statistics.median(xs), 4), "mean_ms": round(sum(xs) / len(xs), 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def timed(fn):
    x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    x.record()
    fn()
    y.record()
    return x, y


def rate(s, nbytes):
    s["achieved_tb_per_s"] = round(nbytes / (s["median_ms"] * 1e-3) / 1e12, 3)
    s["share_of_streamed_copy"] = round(s["achieved_tb_per_s"] / COPY_TB_PER_S, 3)
    return s


def block_ms(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def alternate(fns, repeats):
    """fns: name -> callable; name -> per-repeat milliseconds, the callables taking turns."""
    for _ in range(2):
        for fn in fns.values():
            fn()
    ev = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ev[k].append(timed(fn))
    torch.cuda.synchronize()
    return {k: [x.elapsed_time(y) for x, y in v] for k, v in ev.items()}


def volumes(e, cfg, st, rgbx):
    W, H, aw, D = cfg["W"], cfg["H"], cfg["aw"], cfg["dmax"] + 1
    cam = Pipeline(e, st, W, H, pixel_cost="ncc").cam
    _, l8 = e.cvt(rgbx)
    box = e.box_stats(l8, cfg["K"])
    vols = e.empty((aw, D, H, W), torch.float32)
    for z in range(aw):
        e.ncc_volume(l8, box, cam, z, cfg["K"], out=vols[z])
    return cam, vols


def leg_call(e, a, cfg, vols, res):
    aw, D, H, W = vols.shape
    q = e.quant_u16(vols)
    af, au, a1 = torch.empty_like(vols), torch.empty_like(q), torch.empty_like(q[:1])
    cells = float(D * H * W)
    res["call"] = {"what": "one mvs_sgm8_batch_d (f32) against one mvs_sgm8_u16_batch_d (u16) over the same N = 5 volumes",
                   "cells_per_pass": cells, "streamed_copy_tb_per_s": COPY_TB_PER_S,
                   "largest_quantised_cost": int(q.view(torch.int16).max())}
    for paths in MASKS:
        fns = {"f32": lambda: e.sgm_batch(vols, P1F, P2F, paths, out=af),
               "u16": lambda: e.sgm_u16_batch(q, P1U, P2U, paths, out=au)}
        fns["u16"]()
        e.sgm_u16_batch(q[:1], P1U, P2U, paths, out=a1)
        equal = bool(torch.equal(a1.view(torch.int16), au[:1].view(torch.int16)))
        if not equal:
            raise SystemExit(f"paths {paths}: element 0 of the batch differs from N = 1")
        ms = alternate(fns, a.calls)
        r = {"element_0_is_N1": equal}
        for k, size in (("f32", 4), ("u16", 2)):
            r[k] = rate(summary(ms[k]), passes(paths) * aw * cells * size)
            r[k]["compulsory_gb"] = round(passes(paths) * aw * cells * size / 1e9, 3)
        r["u16_over_f32"] = round(r["u16"]["median_ms"] / r["f32"]["median_ms"], 4)
        r["ranges_disjoint"] = bool(r["u16"]["max"] < r["f32"]["min"] or r["f32"]["max"] < r["u16"]["min"])
        res["call"][f"paths_{paths}_N{aw}"] = r
        print("call", paths, json.dumps(r), flush=True)


def leg_pass(e, a, cam, vols, res):
    _, D, H, W = vols.shape
    cells = float(D * H * W)
    lev = e.levels_dev(cam)
    v = vols[0]
    q = e.quant_u16(v)
    agg = e.sgm_u16_batch(q[None], P1U, P2U, 255)[0]
    aggf = e.sgm_batch(v[None], P1F, P2F, 255)[0]
    disp, conf = e.empty((H, W), torch.float32), e.empty((H, W), torch.float32)
    ms = alternate({"quant_u16": lambda: e.quant_u16(v, out=q),
                    "wta_u16": lambda: e.wta_u16(agg, lev, disp=disp, conf=conf),
                    "wta_f32": lambda: e.wta(aggf, lev, disp=disp, conf=conf)}, a.calls)
    res["pass"] = {"what": "the streaming passes alone on one volume [D, H, W]", "streamed_copy_tb_per_s": COPY_TB_PER_S,
                   "quant_u16": rate(summary(ms["quant_u16"]), 6 * cells),
                   "wta_u16": rate(summary(ms["wta_u16"]), 2 * cells + 8.0 * H * W),
                   "wta_f32": rate(summary(ms["wta_f32"]), 4 * cells + 8.0 * H * W)}
    print("pass", json.dumps(res["pass"]), flush=True)


def leg_step(e, a, cfg, st, rgbx, res):
    W, H, aw = cfg["W"], cfg["H"], cfg["aw"]
    res["step"] = {"what": "whole Pipeline(sgm=True, sgm_batch=5) step, sgm_dtype f32 against u16"}
    for fused in (False, True):
        for paths in (15, 255):
            fns, last = {}, {}
            for dt in ("f32", "u16"):
                p = Pipeline(e, st, W, H, pixel_cost="ncc", fused=fused, sgm=True, sgm_paths=paths, sgm_batch=aw,
                             sgm_dtype=dt)

                def run(p=p, dt=dt):
                    last[dt] = p.exe_pipeline(rgbx)

                fns[dt] = run
            for dt in fns:
                block_ms(fns[dt], a.warmup)
            t = {dt: [] for dt in fns}
            for _ in range(a.blocks):  # f32, u16, f32, u16, ...
                for dt in fns:
                    t[dt].append(block_ms(fns[dt], a.steps))
            sf, su = summary(t["f32"]), summary(t["u16"])
            moved = float((last["f32"].disp_agg != last["u16"].disp_agg).float().mean())
            raw_same = bool(torch.equal(last["f32"].disp, last["u16"].disp) and torch.equal(last["f32"].conf, last["u16"].conf))
            r = {"f32": sf, "u16": su, "difference_ms": round(su["mean_ms"] - sf["mean_ms"], 4),
                 "ranges_disjoint": bool(su["max"] < sf["min"] or sf["max"] < su["min"]),
                 "disp_agg_differs_on": round(moved, 6), "disp_and_conf_identical": raw_same}
            res["step"][f"{'fused' if fused else 'two_pass'}_paths_{paths}"] = r
            print("step", fused, paths, json.dumps(r), flush=True)
            del fns, last, p
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="call,pass,step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm16", "ab.json"))
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
           "method": f"call, pass: {a.calls} alternating repeats per case after 2 warm-up repeats, HIP events around each, "
                     f"median and min / max; step: {a.blocks} alternating blocks of {a.steps} steps per setting after "
                     f"{a.warmup} warm-up steps each, host clock around device-synchronised blocks, mean and min / max"}
    legs = a.legs.split(",")
    if "call" in legs or "pass" in legs:
        cam, vols = volumes(e, cfg, st, rgbx)
        if "call" in legs:
            leg_call(e, a, cfg, vols, res)
        if "pass" in legs:
            leg_pass(e, a, cam, vols, res)
        del vols
        torch.cuda.empty_cache()
    if "step" in legs:
        leg_step(e, a, cfg, st, rgbx, res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
