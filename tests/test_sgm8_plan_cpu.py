"""plan_sgm_diag (csrc/launch_plan.cpp), the launch planner of the diagonal
paths of the semi-global aggregation, on the CPU: tests/host/
sgm_diag_plan_check.cpp links only the planner (plain C++, g++, address and
undefined-behaviour sanitizers), walks W, H in {1, 2, 3, 63, 64, 65, 300, 1920}
and D in {1, 16, 17, 128, 256, 257, 1100} over paths 4..7, asserts each plan's
invariants (block <= 1024, LDS the kernel's static amount, the grid positive,
levels covered >= D; for W, H <= 65 the plan's own (workgroup, lane, row) ->
(x, y) map visits every pixel exactly once, each visit's predecessor being the
same lane's previous pixel) and prints one line per case."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgm_diag_plan_invariants(tmp_path):
    exe = str(tmp_path / "sgm_diag_plan_check")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cl_multiview_stereo_amd", "csrc"), exe,
                    "SDPLANCHK=" + exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    # a sanitizer report ends the process with a non-zero status and its text on stderr
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert len(lines) == 8 * 8 * 7 * 4 + 2 and not any("FAILED" in ln or "error" in ln for ln in lines)
    # both forms, both thread-limit instantiations of the sheared form, both level counts per lane and the
    # multi-wave layout of the lanes form, both shears and both walking orders occur
    assert {ln.split("form=")[1].split()[0] for ln in lines} == {"sheared", "lanes"}
    assert {ln.split("block=")[1].split()[0] for ln in lines if "form=sheared" in ln} == {"64", "128", "512", "1024"}
    assert {ln.split("lpl=")[1].split()[0] for ln in lines if "form=lanes" in ln} == {"8", "16"}
    assert any("form=lanes" in ln and " waves=2 " in ln for ln in lines)
    assert {(ln.split("sx=")[1].split()[0], ln.split("rev=")[1].split()[0]) for ln in lines} == {
        ("1", "0"), ("1", "1"), ("-1", "0"), ("-1", "1")}
