"""plan_sgm_batch (csrc/launch_plan.cpp), the argument rules and the kernel-form
choice of mvs_sgm8_batch_d, on the CPU: tests/host/sgm_batch_plan_check.cpp
links only the planner (plain C++, g++, address and undefined-behaviour
sanitizers), walks N in {1, 2, 3, 5, 65535, 65536, 0, -1}, strides
D H W + {-1 .. 4} and base offsets of 0..3 floats for each buffer, and asserts
per case that the error equals the stated rules, that vec_ok equals the
element-by-element congruence of vol and agg mod 16 bytes, and that the overlap
rule equals an interval test; overlapping, nested, interleaved and abutting
span pairs and the largest shape (65535 volumes of 2^41 floats) follow.  It
prints one line per case."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgm_batch_plan_rules(tmp_path):
    exe = str(tmp_path / "sgm_batch_plan_check")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cl_multiview_stereo_amd", "csrc"), exe,
                    "SBPLANCHK=" + exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    # a sanitizer report ends the process with a non-zero status and its text on stderr
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    # 8 batch sizes x 6 x 6 strides x 4 x 4 offsets, 11 span pairs, 5 cases at the largest shape
    assert len(lines) == 8 * 6 * 6 * 4 * 4 + 11 + 5 and not any("FAILED" in ln for ln in lines)
    ok = [ln for ln in lines if "-> ok" in ln]
    # every rule refuses something, and both kernel forms are chosen, with one element and with several
    for why in ("N must be in 1..65535", "a stride below D*H*W", "the vol and agg spans overlap"):
        assert any("-> " + why in ln for ln in lines), why
    assert {(ln.split(" N=")[1].split()[0] == "1", ln.split("vec_ok=")[1]) for ln in ok} == {
        (True, "0"), (True, "1"), (False, "0"), (False, "1")}
    assert all(ln.split("grid_y=")[1].split()[0] == ln.split(" N=")[1].split()[0] for ln in ok)
    assert any(" N=65535 " in ln for ln in ok) and not any(" N=65536 " in ln or " N=0 " in ln or " N=-1 " in ln for ln in ok)
