"""The NCC sweep's launch planner (csrc/ncc_plan.cpp) against the golden of
the launcher's decisions, on the CPU.

tests/host/ncc_plan_check.cpp links only the planner (plain C++, g++, address
and undefined-behaviour sanitizers) and prints, per case, one line per launch:
the kernel family and template coordinates, the complete launch arguments, the
plan table's length and FNV-1a hash, the LDS bytes and the reported variant
slots; for an argument error, its message.  tests/golden/ncc_launch_plans.txt
holds the same lines printed by the launcher as it was before the planner was
split out of it (a host-only build of that launch_ncc_refs, its launches
replaced by the print), so every decision -- kernel form per view, run
grouping, LDS sizes, shift tables -- is pinned, not only the last launch's
variant.  Each case runs in a process of its own: MVS_NCC_DPW and MVS_NCC_NW
are read once per process, and a case's knobs are set in that process."""
from __future__ import annotations

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ncc_launch_plans.txt")


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
    exe = str(tmp_path_factory.mktemp("ncc_plan") / "ncc_plan_check")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "cl_multiview_stereo_amd", "csrc"), "plancheck",
                    "PLANCHK=" + exe], check=True)
    return exe


def _run(checker, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MVS_NCC_")}
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


def test_every_error_and_kernel_family_is_covered():
    """The golden holds each argument error of the planner once and both kernel families."""
    lines = [ln for c in _CASES.values() for ln in c]
    errors = sorted(ln.split("error: ", 1)[1] for ln in lines if " error: " in ln)
    assert errors == sorted([
        "fused NCC sweep: at most 65535 levels",
        "NCC sweep supports at most 16 neighbours per reference view",
        "view_subset entry out of range",
        "NCC sweep needs W >= 2",
        "NCC window must be 5 or 7",
        "NCC sweep: neighbour shifts too large for the LDS band",
        "the NCC cost volume holds one reference view",
    ])
    assert any(" fam=mfma " in ln for ln in lines) and any(" fam=scalar " in ln for ln in lines)
