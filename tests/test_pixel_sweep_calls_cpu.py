"""PixelSweep.run's engine calls, pinned: every option set the constructor takes (fused x subpixel x sgm, sgm_batch in
1, 2, 7, both sgm_dtype, sgm_subpixel) over the view ranges [0, 5) and [1, 4), driven against a stub engine that
allocates on the CPU and records every other call by name and arguments.  A tensor that aliases one of the sweep's
buffers is written as name+storage_offset(shape), a Python scalar by value, anything else by shape (or type) only.
The log of each run must equal tests/golden/pixel_sweep_calls.txt, which

    python tests/test_pixel_sweep_calls_cpu.py > tests/golden/pixel_sweep_calls.txt

wrote from the sweep as it stood before its drivers became one loop: same calls, same order, same buffers."""
from __future__ import annotations

import itertools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from cl_multiview_stereo_amd import params  # noqa: E402
from cl_multiview_stereo_amd.engine import CameraArray  # noqa: E402
from cl_multiview_stereo_amd.pipeline import PixelSweep  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "pixel_sweep_calls.txt")
V, W, H, D, K, PATHS = 5, 12, 6, 8, 5, 255
BUFFERS = ("vol", "agg", "q", "levels", "disp_sub", "disp_agg", "conf_agg", "disp_agg_sub")


class StubEngine:
    """empty allocates on the CPU, levels_dev gives the levels; every other method records (name, args, kwargs)."""

    def __init__(self):
        self.calls = []

    def empty(self, shape, dtype):
        return torch.zeros(tuple(shape), dtype=dtype)

    def levels_dev(self, cam):
        return torch.from_numpy(cam.levels.copy())

    def __getattr__(self, name):
        def record(*args, **kwargs):
            self.calls.append((name, args, kwargs))
        return record


def _cases():
    for fused, subpixel, sgm, batch, dtype, sgm_sub, zr in itertools.product(
            (False, True), (False, True), (False, True), (1, 2, 7), ("f32", "u16"), (False, True), ((0, 5), (1, 4))):
        if not sgm and (dtype == "u16" or sgm_sub):
            continue  # the constructor refuses these
        yield (f"fused={int(fused)} subpixel={int(subpixel)} sgm={int(sgm)} sgm_batch={batch} sgm_dtype={dtype} "
               f"sgm_subpixel={int(sgm_sub)} z={zr[0]}..{zr[1]}",
               dict(fused=fused, subpixel=subpixel, sgm=sgm, sgm_batch=batch, sgm_dtype=dtype, sgm_subpixel=sgm_sub), zr)


CASES = {name: (kw, zr) for name, kw, zr in _cases()}


def _shape(t):
    return "(" + ",".join(str(n) for n in t.shape) + ")"


def run_log(kw, zr):
    """The lines of one run: one per recorded call."""
    vs, sn = params.flatten_subsets(params.neighbour_lists(V, 1, 1, 0))
    cam = CameraArray(V, 1.0, params.disparity_levels(0, D - 1, 1), vs, sn)
    assert cam.D == D and cam.view_count == V
    e = StubEngine()
    sweep = PixelSweep(e, cam, W, H, "ncc", K, sgm_p1=0.1, sgm_p2=0.8, sgm_paths=PATHS, **kw)
    n = zr[1] - zr[0]
    named = {"disp": torch.zeros((n, H, W)), "conf": torch.zeros((n, H, W))}
    sweep.run(None, torch.zeros((V, H, W), dtype=torch.uint8), zr[0], zr[1], disp_out=named["disp"],
              conf_out=named["conf"])
    named.update({b: getattr(sweep, b) for b in BUFFERS if getattr(sweep, b) is not None})
    owner = {t.untyped_storage().data_ptr(): b for b, t in named.items()}
    assert len(owner) == len(named)

    def fmt(a):
        if isinstance(a, torch.Tensor):
            b = owner.get(a.untyped_storage().data_ptr())
            return _shape(a) if b is None else f"{b}+{a.storage_offset()}{_shape(a)}"
        if a is None or isinstance(a, (bool, int, float, str)):
            return repr(a)
        return type(a).__name__

    return [name + "(" + ", ".join([fmt(a) for a in args] + [f"{k}={fmt(a)}" for k, a in kwargs.items()]) + ")"
            for name, args, kwargs in e.calls]


def _golden():
    runs, cur = {}, None
    with open(GOLDEN) as f:
        for line in f.read().splitlines():
            if line.startswith("# "):
                cur = runs.setdefault(line[2:], [])
            elif line:
                cur.append(line)
    return runs


_WANT = _golden() if os.path.exists(GOLDEN) else {}


def test_the_golden_holds_every_run():
    assert len(CASES) == 120 and set(_WANT) == set(CASES)
    assert all(len(log) >= 2 for log in _WANT.values())  # the shortest: box_stats, ncc_wta_range


@pytest.mark.parametrize("case", list(CASES))
def test_calls(case):
    got, want = run_log(*CASES[case]), _WANT[case]
    assert "\n".join(got) == "\n".join(want)


if __name__ == "__main__":
    for name, (kw, zr) in CASES.items():
        print("# " + name)
        print("\n".join(run_log(kw, zr)))
        print()
