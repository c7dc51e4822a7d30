#!/usr/bin/env python3
"""One timed call per kernel of sgm_kernels.h and of the winner passes whose instruction stream is not the
parent's (profiles/sgm_unify/isa_compare.txt), for an A/B of two builds of libmvs.so: run it once per build
(MVS_LIB names the library), the builds taking turns, and compare the medians.

  f32 lanes, 16-byte pieces    mvs_sgm_d, mask 1, at D = 64, 128, 256 (1920 x 1080) and 512, 1024 (960 x 540): 1, 2,
                               4, 8, 16 levels per lane
  f32 lanes, several waves     mvs_sgm_d mask 1 and mvs_sgm8_d mask 16 (the strided form) at D = 1025, 256 x 256:
                               256 and 511 lines, one workgroup each, the smallest shape that gives each of the 256
                               CUs one
  winner passes                mvs_wta_d, mvs_wta_agg_sub_d, mvs_wta_u16_d and mvs_wta_u16_sub_d at D = 128,
                               1920 x 1080 (four pixels per lane for uint16) and 1919 x 1079 (one pixel per lane)

Costs are seeded uniform noise: the kernels' work does not depend on the values, only the winner passes' gathers
do, and both builds get the same.  Per case: 3 warm-up calls, then --calls calls with HIP events around each;
median, min and max in milliseconds.  Prints one JSON line per case and writes them all to --out.

    MVS_LIB=/path/to/libmvs.so python scripts/bench_sgm_unify.py --out run.json [--calls 20] [--only REGEX]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from cl_multiview_stereo_amd import _lib  # noqa: E402
from cl_multiview_stereo_amd.engine import Engine  # noqa: E402


def noise(shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(shape, generator=g, device="cuda", dtype=torch.float32) * 2.0


def time_call(fn, calls):
    for _ in range(3):
        fn()
    ev = []
    for _ in range(calls):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record()
        fn()
        y.record()
        ev.append((x, y))
    torch.cuda.synchronize()
    ms = [x.elapsed_time(y) for x, y in ev]
    return {"median_ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4),
            "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default="", help="a regular expression: time the cases whose name it finds")
    a = ap.parse_args()
    e = Engine(0)
    res = {"lib": os.path.realpath(_lib.LIB_PATH), "calls": a.calls, "cases": {}}

    def case(name, fn):
        if not re.search(a.only, name):
            return
        res["cases"][name] = r = time_call(fn, a.calls)
        print(name, json.dumps(r), flush=True)

    for D, W, H in ((64, 1920, 1080), (128, 1920, 1080), (256, 1920, 1080), (512, 960, 540), (1024, 960, 540)):
        vol = noise((D, H, W), D)  # k_sgm_lanes<SgmF32, 1 | 2 | 4 | 8 | 16, VEC>
        out = torch.empty_like(vol)
        case(f"sgm_f32_mask1_D{D}_{W}x{H}", lambda: e.sgm(vol, 0.1, 0.8, 1, out=out))
        del vol, out
    vol = noise((1025, 256, 256), 7)  # k_sgm_lanes<SgmF32, 16, scalar, MW> and <..., MW, DIAG>
    out = torch.empty_like(vol)
    for mask in (1, 16):
        case(f"sgm_f32_mask{mask}_D1025_256x256", lambda: e.sgm(vol, 0.1, 0.8, mask, out=out))
    del vol, out
    for W, H in ((1920, 1080), (1919, 1079)):
        lv = torch.arange(128, device="cuda", dtype=torch.float32)
        raw = noise((128, H, W), 11)
        agg = noise((128, H, W), 12)
        if W == 1920:  # k_wta<1, 16> and k_wta_agg_sub<16> have one form
            case(f"wta_f32_{W}x{H}", lambda: e.wta(agg, lv))
            case(f"wta_agg_sub_{W}x{H}", lambda: e.wta_agg_sub(agg, raw, lv))
        rq, aq = e.quant_u16(raw), e.quant_u16(agg)
        del raw, agg
        case(f"wta_u16_{W}x{H}", lambda: e.wta_u16(aq, lv))  # k_wta_u16<4, 8> | <1, 16>
        case(f"wta_u16_sub_{W}x{H}", lambda: e.wta_u16_sub(aq, rq, lv))
        del rq, aq
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
