#!/usr/bin/env python3
"""What the sub-level disparity of the aggregate costs at the C2 shape (5 views,
1920x1080, D = 128, K = 5, S = 32): interleaved A/Bs in one process.

Leg "pass": one view's NCC volume [128, 1080, 1920], quantised, and its real
aggregates (paths = 255, uint16 and float32).  Alternately in one loop
mvs_wta_u16_d(agg) and mvs_wta_u16_sub_d(agg, raw), then likewise mvs_wta_d and
mvs_wta_agg_sub_d; HIP events around each call, median and min..max over the
repeats.  Bytes: D H W cells of agg; the new calls also three raw cells and
three output words per pixel (the plain ones two output words).  Before the
timing disp and conf of the two calls are compared bit for bit.  The one
condition: the new call's median stays below twice the plain winner call's on
the same agg (what a winner pass plus a separate sub-level pass over agg
would cost at least); the script exits with status 1 otherwise.

Leg "step": the whole step, Pipeline(sgm=True, sgm_batch=5, sgm_paths=255)
two-pass and fused, sgm_dtype f32 and u16, with sgm_subpixel off and on in
alternating blocks of steps, each block device-synchronised before and after;
a setting's time is the mean over its blocks, the spread their min..max.

Writes profiles/sgm_sub/ab.json.

    python scripts/bench_sgm_sub.py [--calls 20] [--blocks 3] [--steps 4] [--warmup 2] [--legs pass,step]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_sgm16 import C2, COPY_TB_PER_S, P1F, P1U, P2F, P2U, alternate, block_ms, rate, summary  # noqa: E402
from cl_multiview_stereo_amd import params, synth  # noqa: E402
from cl_multiview_stereo_amd.engine import Engine  # noqa: E402
from cl_multiview_stereo_amd.pipeline import Pipeline  # noqa: E402

PATHS = 255


def leg_pass(e, a, cfg, st, rgbx, res):
    W, H, D = cfg["W"], cfg["H"], cfg["dmax"] + 1
    cam = Pipeline(e, st, W, H, pixel_cost="ncc").cam
    _, l8 = e.cvt(rgbx)
    box = e.box_stats(l8, cfg["K"])
    z = cfg["aw"] // 2
    vol = e.ncc_volume(l8, box, cam, z, cfg["K"])
    q = e.quant_u16(vol)
    aggu = e.sgm_u16_batch(q[None], P1U, P2U, PATHS)[0]
    aggf = e.sgm_batch(vol[None], P1F, P2F, PATHS)[0]
    lev = e.levels_dev(cam)
    new = lambda: e.empty((H, W), torch.float32)
    d0, c0, d1, c1, s1 = new(), new(), new(), new(), new()
    cells, px = float(D * H * W), float(H * W)
    res["pass"] = {"what": f"the winner pass of one aggregate [D, H, W] (view {z}, paths {PATHS}) without and with the "
                           "sub-level fit through the raw volume", "streamed_copy_tb_per_s": COPY_TB_PER_S}
    ok = True
    for dt, size, plain, sub in (("u16", 2, lambda: e.wta_u16(aggu, lev, disp=d0, conf=c0),
                                  lambda: e.wta_u16_sub(aggu, q, lev, disp=d1, conf=c1, out=s1)),
                                 ("f32", 4, lambda: e.wta(aggf, lev, disp=d0, conf=c0),
                                  lambda: e.wta_agg_sub(aggf, vol, lev, disp=d1, conf=c1, out=s1))):
        plain()
        sub()
        if not (torch.equal(d0, d1) and torch.equal(c0, c1)):
            raise SystemExit(f"{dt}: disp / conf of the two calls differ")
        moved = float((s1 != d1).float().mean())
        ms = alternate({"wta": plain, "wta_sub": sub}, a.calls)
        r = {"wta": rate(summary(ms["wta"]), size * cells + 8 * px),
             "wta_sub": rate(summary(ms["wta_sub"]), size * cells + (3 * size + 12) * px),
             "disp_and_conf_identical": True, "share_of_pixels_the_fit_moves": round(moved, 4)}
        r["sub_over_wta"] = round(r["wta_sub"]["median_ms"] / r["wta"]["median_ms"], 4)
        r["added_ms"] = round(r["wta_sub"]["median_ms"] - r["wta"]["median_ms"], 4)
        r["below_twice_the_winner_pass"] = bool(r["wta_sub"]["median_ms"] < 2 * r["wta"]["median_ms"])
        ok = ok and r["below_twice_the_winner_pass"]
        res["pass"][dt] = r
        print("pass", dt, json.dumps(r), flush=True)
    return ok


def leg_step(e, a, cfg, st, rgbx, res):
    W, H, aw = cfg["W"], cfg["H"], cfg["aw"]
    res["step"] = {"what": f"whole Pipeline(sgm=True, sgm_batch=5, sgm_paths={PATHS}) step, sgm_subpixel off against on"}
    for fused in (False, True):
        for dt in ("f32", "u16"):
            fns, last = {}, {}
            # a third pipeline with the option off, built last: each pipeline has buffers of its own, and what two
            # equal settings differ by is the part of a difference that the option does not explain
            for k in a.order.split(",") + ["off_again"]:
                p = Pipeline(e, st, W, H, pixel_cost="ncc", fused=fused, sgm=True, sgm_paths=PATHS, sgm_batch=aw,
                             sgm_dtype=dt, sgm_subpixel=(k == "on"))

                def run(p=p, k=k):
                    last[k] = p.exe_pipeline(rgbx)

                fns[k] = run
            for k in fns:
                block_ms(fns[k], a.warmup)
            t = {k: [] for k in fns}
            for _ in range(a.blocks):  # the settings take turns
                for k in fns:
                    t[k].append(block_ms(fns[k], a.steps))
            s0, s1, s2 = summary(t["off"]), summary(t["on"]), summary(t["off_again"])
            same = all(torch.equal(getattr(last["off"], n), getattr(last["on"], n))
                       for n in ("disp", "conf", "disp_agg", "conf_agg"))
            r = {"built_in_order": list(fns), "off": s0, "on": s1, "off_again": s2,
                 "difference_ms": round(s1["mean_ms"] - s0["mean_ms"], 4),
                 "off_again_minus_off_ms": round(s2["mean_ms"] - s0["mean_ms"], 4),
                 "ranges_disjoint": bool(s1["max"] < s0["min"] or s0["max"] < s1["min"]),
                 "other_outputs_identical": bool(same)}
            res["step"][f"{'fused' if fused else 'two_pass'}_{dt}"] = r
            print("step", fused, dt, json.dumps(r), flush=True)
            del fns, last, p
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--legs", default="pass,step")
    ap.add_argument("--order", default="off,on", choices=["off,on", "on,off"],
                    help="step: the order in which the two settings' pipelines (and their buffers) are built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sgm_sub", "ab.json"))
    a = ap.parse_args()
    cfg = C2
    W, H, aw, D = cfg["W"], cfg["H"], cfg["aw"], cfg["dmax"] + 1
    e = Engine(0)
    st = params.Settings(spixl_size=cfg["S"], array_width=aw, array_height=1, min_disp=0, max_disp=cfg["dmax"], inc=1,
                         neib_hor=cfg["nh"], neib_ver=0, bl_ratio=1.0, window=cfg["K"], cost="ncc")
    stack, _ = synth.make_stack(W, H, aw, 1, 0, cfg["dmax"], 1.0, 0x5EED + 2)  # bench.py's stack
    rgbx = torch.from_numpy(stack).to(e.device)
    res = {"device": torch.cuda.get_device_name(0), "library": e.L.mvs_version().decode(),
           "shape": f"{aw} views {W}x{H}, D = {D}, K = {cfg['K']}"}
    legs = a.legs.split(",")
    methods = {"pass": f"{a.calls} alternating repeats per case after 2 warm-up repeats, HIP events around each, median "
                       "and min / max",
               "step": f"{a.blocks} alternating blocks of {a.steps} steps per setting after {a.warmup} warm-up steps "
                       "each, host clock around device-synchronised blocks, mean and min / max"}
    res["method"] = {k: v for k, v in methods.items() if k in legs}  # of the legs this file holds
    ok = True
    if "pass" in legs:
        ok = leg_pass(e, a, cfg, st, rgbx, res)
        torch.cuda.empty_cache()
    if "step" in legs:
        leg_step(e, a, cfg, st, rgbx, res)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    if not ok:
        raise SystemExit("the new call's median is not below twice the winner pass's")


if __name__ == "__main__":
    main()
