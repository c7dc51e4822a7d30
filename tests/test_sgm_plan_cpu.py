"""plan_sgm (csrc/launch_plan.cpp), the launch planner of the semi-global
aggregation, on the CPU: tests/host/sgm_plan_check.cpp links only the planner
(plain C++, g++, address and undefined-behaviour sanitizers), walks W, H in
{1, 2, 3, 63, 64, 65, 300, 1920, 4096} and D in {1, 2, 63, 64, 65, 128, 256,
257, 1100} over the four paths, asserts each plan's invariants (every row or
column covered exactly once, levels covered >= D, block <= 1024, LDS <= 160 KB,
the grid positive and inside HIP's limits) and prints one line per case."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgm_plan_invariants(tmp_path):
    exe = str(tmp_path / "sgm_plan_check")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cl_multiview_stereo_amd", "csrc"), exe,
                    "SPLANCHK=" + exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    # a sanitizer report ends the process with a non-zero status and its text on stderr
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == 9 * 9 * 9 * 4 + 2 and not any("FAILED" in ln or "error" in ln for ln in lines)
    # both forms, every level count per lane, both wave layouts and the 16-byte pieces occur
    assert {ln.split("form=")[1].split()[0] for ln in lines} == {"lanes", "columns"}
    assert {ln.split("lpl=")[1].split()[0] for ln in lines if "form=lanes" in ln} == {"1", "2", "4", "8", "16"}
    assert any("form=lanes" in ln and " waves=2 " in ln for ln in lines)
    assert any(" vec=1 " in ln for ln in lines) and any("form=lanes" in ln and " vec=0 " in ln for ln in lines)
