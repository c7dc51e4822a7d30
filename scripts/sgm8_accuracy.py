#!/usr/bin/env python3
"""The two accuracy tables of DESIGN.md 4c, on the CPU (the oracle and
tests/sgm8_ref.py): the share of centre-view pixels more than one level off the
scene's disparity with four and with eight paths, on the rectangle scenes of
synth.make_stack (seeds 0..5) and on the disc-and-diamond scenes of
tests/test_sgm8_cpu.py (seeds 900..905), 256 x 128.

    python scripts/sgm8_accuracy.py
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cl_multiview_stereo_amd import synth  # noqa: E402
from tests.test_sgm8_cpu import bad_shares, scene  # noqa: E402

W, H = 256, 128


def main():
    print("rectangles (synth.make_stack)\n| seed | raw | paths = 15 | paths = 255 |\n|---|---|---|---|")
    for seed in range(6):
        stack, gt = synth.make_stack(W, H, 5, 1, 0, 31, 1.0, 0x5EED + seed)
        raw, b15, b255 = bad_shares(stack, gt)
        print(f"| {seed} | {raw:.3f} | {b15:.3f} | {b255:.3f} |", flush=True)
    print("discs and diamonds\n| seed | raw | paths = 15 | paths = 240 | paths = 255 | 255 / 15 |\n|---|---|---|---|---|---|")
    for seed in range(900, 906):
        stack, gt = scene(W, H, seed)
        raw, b15, b240, b255 = bad_shares(stack, gt, (15, 240, 255))
        print(f"| {seed} | {raw:.3f} | {b15:.3f} | {b240:.3f} | {b255:.3f} | {b255 / b15:.2f} |", flush=True)


if __name__ == "__main__":
    main()
