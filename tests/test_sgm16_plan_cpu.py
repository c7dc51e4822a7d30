"""plan_sgm_batch at kSgmU16, sgm_piece_vec_ok and the piece phase (csrc/launch_plan.cpp,
launch_plan.h), the argument rules and the kernel-form choice of
mvs_sgm8_u16_batch_d, on the CPU: tests/host/sgm16_plan_check.cpp links only
the planner (plain C++, g++, address and undefined-behaviour sanitizers) and
checks, against brute force, the span and stride rules in 2-byte elements
(element strides near 2^41 included), vec_ok as the element-by-element
congruence of vol and agg mod 16 bytes, the level limit of 256, and the phase
of the eight-pixel pieces for every line address mod 16 bytes and every line
length up to 40.  It prints one line per case."""
from __future__ import annotations

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sgm16_plan_rules(tmp_path):
    exe = str(tmp_path / "sgm16_plan_check")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cl_multiview_stereo_amd", "csrc"), exe,
                    "S16PLANCHK=" + exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    # a sanitizer report ends the process with a non-zero status and its text on stderr
    assert r.returncode == 0 and r.stderr == "", (r.stdout[-2000:], r.stderr[-2000:])
    lines = r.stdout.splitlines()
    assert not any("FAILED" in ln for ln in lines)
    plans = [ln for ln in lines if ln.startswith("W=")]
    phases = [ln for ln in lines if ln.startswith("phase ")]
    # 8 batch sizes x 6 x 6 strides x 4 x 4 offsets, 14 single cases, 4 x 5 + 2 at strides near 2^41; 8 addresses x 40
    assert len(plans) == 8 * 6 * 6 * 4 * 4 + 14 + 22 and len(phases) == 8 * 40 and len(lines) == len(plans) + len(phases)
    assert {ln.split("ph=")[1] for ln in phases} == set("01234567")
    ok = [ln for ln in plans if "-> ok" in ln]
    # every rule refuses something, and both kernel forms are chosen, with one element and with several
    for why in ("N must be in 1..65535", "a stride below D*H*W", "the vol and agg spans overlap",
                "a pointer that is not 2-byte aligned", "more than 256 levels"):
        assert any("-> " + why in ln for ln in plans), why
    assert {(ln.split(" N=")[1].split()[0] == "1", ln.split("vec_ok=")[1]) for ln in ok} == {
        (True, "0"), (True, "1"), (False, "0"), (False, "1")}
    assert all(ln.split("grid_y=")[1].split()[0] == ln.split(" N=")[1].split()[0] for ln in ok)
    assert any(" N=65535 " in ln for ln in ok) and not any(" N=65536 " in ln or " N=0 " in ln or " N=-1 " in ln for ln in ok)
    assert any("+2199023255553 " in ln for ln in ok)  # a stride of 2^41 + 1 elements
