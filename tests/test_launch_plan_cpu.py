"""The launch planners of the superpixel sweep, the per-pixel SAD sweep and the
view-consistency filter (csrc/launch_plan.cpp) against the golden of the
launchers' decisions, on the CPU.

tests/host/launch_plan_check.cpp links only the planner (plain C++, g++,
address and undefined-behaviour sanitizers) and prints, per case, one line per
planned launch: the kernel and its template coordinates, the launch arguments
as ints, the grid, the LDS bytes, the table's length and FNV-1a hash, the
re-layout launches in order and the reported sweep_last slots; for an error,
its message.  tests/golden/launch_plans.txt holds the same lines printed by
launch_sweep_spixl, launch_sad_band_t / launch_sweep_pixel_sad and
launch_remove_incons as they were before the planners were split out of them:
a host-only build of those functions' text, their kernel launches, scratch
allocation and table upload replaced by the print.  So every decision -- form,
waves per superpixel, slot offsets, SadRec shifts, bw, brows, LDS bytes, the
filter ladder's branch and q's 16 coordinates -- is pinned.

One exception, stated so that nobody takes it for the old launcher's output:
as written, the old launch_sweep_spixl never reached its row-major fallback
when the re-layout scratch could not be had (the MVS_E_NOMEM status it had
just handled was returned by the next status check).  The lines of the calls
with allow_relayout = false that had slots to build (their case comments say
"without the scratch") were printed by the same text with that status cleared,
which is the fallback its comments describe and the launcher now performs.

Each case runs in a process of its own with its knobs set in that process."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.txt")
KNOBS = ("MVS_SWEEP_", "MVS_SAD_", "MVS_FILTER_")


def _golden():
    cases, name = {}, None
    with open(GOLDEN) as f:
        for line in f:
            if line.startswith("== "):
                name = line[3:].strip()
                cases[name] = []
            else:
                cases[name].append(line.rstrip("\n"))
    return cases


_CASES = _golden()


@pytest.fixture(scope="session")
def checker(tmp_path_factory):
    d = tmp_path_factory.mktemp("launch_plan")
    exe = str(d / "launch_plan_check")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cl_multiview_stereo_amd", "csrc"), exe,
                    "LPLANCHK=" + exe], check=True)
    return exe


def _run(checker, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith(KNOBS)}
    return subprocess.run([checker, *args], env=env, capture_output=True, text=True)


def test_case_list(checker):
    r = _run(checker, "--list")
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == list(_CASES)


@pytest.mark.parametrize("case", list(_CASES))
def test_launch_plan(checker, case):
    r = _run(checker, case)
    # a sanitizer report ends the process with a non-zero status and its text on stderr
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    got, want = r.stdout.splitlines(), _CASES[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: line {i} differs\n got  {g}\n want {w}"
    assert len(got) == len(want), f"{case}: {len(got)} lines, golden has {len(want)}"


def test_every_form_kernel_branch_and_error_is_covered():
    """The golden holds every form of the sweep (at both wave layouts where the
    form has them), every SAD kernel choice, every branch of the filter's
    ladder, all 16 coordinates of the q kernel and each error message once."""
    lines = [ln for c in _CASES.values() for ln in c]
    forms = {m.group(0) for ln in lines for m in [re.search(r"sweep form=\d lps=\d+", ln)] if m}
    assert forms == {f"sweep form={f} lps={l}" for f in (0, 1, 3) for l in (32, 64)} | {"sweep form=2 lps=64"}
    assert {m.group(1) for ln in lines for m in [re.search(r"form=2 lps=64 wps=(\d)", ln)] if m} == {"1", "2", "4"}
    assert any(re.search(r"relayouts=\d+:1:\d+", ln) for ln in lines)
    assert any(re.search(r"relayouts=\S*\d+:2:\d+", ln) and re.search(r"relayouts=\S*\d+:3:\d+", ln) for ln in lines)
    sad = {m.group(1) for ln in lines for m in [re.search(r"sad kern=(band TH=8 PPW=\d AFF=\d BWT=\d+|gather)", ln)] if m}
    assert sad == {f"band TH=8 PPW={p} {ab}" for p in (1, 2) for ab in ("AFF=0 BWT=0", "AFF=1 BWT=64", "AFF=1 BWT=128")} | {"gather"}
    filt = {m.group(1) for ln in lines for m in [re.search(r"filter kern=(\w+)", ln)] if m}
    assert filt == {"sel8", "px16_8", "q", "px32", "sel64", "plain"}
    assert {m.group(1) for ln in lines for m in [re.search(r"kern=px32 FB=(\d)", ln)] if m} == {"2", "4", "8"}
    q = {m.group(0) for ln in lines for m in [re.search(r"kern=q FB=\d NS=\d ROWB=\d RM=\d", ln)] if m}
    assert q == {f"kern=q FB={fb} NS={ns} ROWB={rb} RM={rm}" for fb in (2, 4) for ns in (1, 2) for rb in (0, 1) for rm in (0, 1)}
    assert {m.group(1) for ln in lines for m in [re.search(r"kern=q .* inb=(\d)", ln)] if m} == {"0", "1"}
    assert any(ln.endswith(" none") for ln in lines)
    errors = sorted(ln.split("error: ", 1)[1] for ln in lines if " error: " in ln)
    unfit = "k_sad_band variant %s cannot stage this geometry (MVS_SAD_KERNEL set explicitly)"
    assert errors == sorted([
        "superpixel sweep: image too large for 32-bit offsets",
        unfit % "sys8x2",
        unfit % "sys8",
        unfit % "auto",
        unfit % "sys16",
    ])
