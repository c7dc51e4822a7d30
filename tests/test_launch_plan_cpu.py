"""The launch planners of the SLIC stage, the superpixel sweep, the per-pixel
SAD sweep and the view-consistency filter (csrc/launch_plan.cpp) against the
golden of the launchers' decisions, on the CPU.

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

The SLIC cases (`slic_*`) came later, by the same method: their lines were
printed by a host-only build of mvs_slic_d and its seven launchers
(launch_init_centers, launch_edge_step, launch_assign, launch_assign_tiles,
launch_update_finalize, launch_update, launch_suppress) as they were before
plan_slic, verbatim, every kernel launch replaced by a print of the kernel, its
template arguments, grid, block, pointer arguments by role (lab, spixl,
labels, scratch, null) and scalar arguments (xy and col as bit patterns), and
mvs::scratch by a print of the size (`scratch=`, 0 where it was not called).
That build is not kept.  So the launch sequence, which of labels / 16-bit
copies / tile partials each assignment writes, each kernel form and the
scratch size are pinned.  The stand-alone tile-partial update kernel that text
still launched in one branch was stubbed the same way, and no case reached it.

Each case runs in a process of its own with its knobs set in that process."""
from __future__ import annotations

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.txt")
KNOBS = ("MVS_SWEEP_", "MVS_SAD_", "MVS_FILTER_", "MVS_SLIC_")


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
    ladder, all 16 coordinates of the q kernel and each error message once;
    every SLIC kernel form, spixl_size class, iteration count, knob and scratch
    user."""
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
    # -- SLIC: every case's calls as lists of lines
    calls = {}
    for name, c in _CASES.items():
        for ln in c:
            if " slic " in ln:
                calls.setdefault((name, ln.split()[0]), []).append(ln)
    assert calls and all(c[-1].split()[2].startswith("scratch=") for c in calls.values())

    def num(ln, key):
        return int(re.search(r"[=,]%s:(\d+)" % key, ln).group(1))

    def kerns(c):
        return [ln.split()[2] for ln in c[:-1]]

    def knobs(name, **kv):
        # the case's knobs are exactly kv (its name says so: the case list is C++)
        want = {"slic_tiles9": {"TILES9": "1"}, "slic_tiles9_other": {"TILES9": "2"}, "slic_update0": {"UPDATE": "0"},
                "slic_update1": {"UPDATE": "1"}, "slic_update_nan": {"UPDATE": "walk"},
                "slic_both_knobs": {"UPDATE": "0", "TILES9": "1"}}
        return want.get(name, {}) == kv
    every = [(n, c) for (n, _), c in calls.items()]
    forms = {k for _, c in every for k in kerns(c)}
    assert forms == ({"k_init_centers", "k_edge", "k_edge_store", "k_apply_edge", "k_suppress"}
                     | {f"k_assign<S3={s}>" for s in (0, 1)} | {f"k_assign_tiles<S3={s}>" for s in (0, 1)}
                     | {f"k_assign_tiles4<S16={s}>" for s in (2, 4)} | {f"k_update_finalize<CPL={c}>" for c in (6, 0)}
                     | {f"{k}<UT={u},LT={l}>" for k in ("k_update_walk", "k_update") for u in (4, 1) for l in (16, 32)})
    # each S at an image size that is a multiple of neither 16 nor S
    odd = {num(c[0], "S") for _, c in every
           if all(num(c[0], d) % 16 and num(c[0], d) % num(c[0], "S") for d in "WH")}
    assert odd >= {6, 8, 12, 16, 32, 40, 48, 64, 96}
    # no_iter = 0, 1, 2, 5 (the updates of a call) on the walk, the 4-cell and the 9-cell path
    for upd, asg in (("k_update_walk", "k_assign<"), ("k_update_finalize", "k_assign_tiles4<"),
                     ("k_update_finalize", "k_assign_tiles<")):
        its = {sum(k.startswith(upd) for k in kerns(c)) for _, c in every if any(k.startswith(asg) for k in kerns(c))}
        assert its >= {0, 1, 2, 5}, (asg, its)
    # search = 1 on both paths; at S = 32 it gives the 9-cell kernel
    assert any("k_assign<S3=1>" in kerns(c) for _, c in every)
    assert any("k_assign_tiles<S3=1>" in kerns(c) and num(c[0], "S") == 32 for n, c in every if knobs(n))
    assert any("k_assign_tiles4<S16=2>" in kerns(c) and num(c[0], "S") == 32 for n, c in every if knobs(n))
    # MVS_SLIC_TILES9=1 at S = 32 and 64: the 9-cell kernel of the 2x2 loop
    t9 = {num(c[0], "S") for n, c in every if knobs(n, TILES9="1") and "k_assign_tiles<S3=0>" in kerns(c)}
    assert t9 >= {32, 64}
    # MVS_SLIC_UPDATE=0: k_update with both UT and both label types, where the walk ran without it
    u0 = {k for n, c in every if knobs(n, UPDATE="0") for k in kerns(c) if k.startswith("k_update")}
    assert u0 >= {f"k_update<UT={u},LT={l}>" for u in (4, 1) for l in (16, 32)}
    assert not any(k.startswith("k_update_walk") for k in u0)
    # the edge step's three settings and the connectivity pass, off and on
    edge = {tuple(k for k in kerns(c) if "edge" in k) for _, c in every}
    assert edge == {(), ("k_edge", "k_edge_store"), ("k_edge", "k_apply_edge")}
    assert {kerns(c).count("k_suppress") for _, c in every} == {0, 2}
    sup = [ln for _, c in every for ln in c if " k_suppress " in ln]
    assert {re.search(r"bufs=(\S+)", ln).group(1) for ln in sup} == {"in:labels,out:scratch", "in:scratch,out:labels"}
    # more than 65536 superpixels: no 16-bit copies, and with nothing else to hold no scratch at all
    big = [c for _, c in every if num(c[0], "mw") * num(c[0], "mh") > 65536 and num(c[0], "S") % 16]
    assert big and not any("lb16:scratch" in ln or "LT=16" in ln for c in big for ln in c)
    assert any(c[-1].endswith("scratch=0") and len(c) > 3 for c in big)
    assert any(len(c) > 3 and num(c[0], "mw") * num(c[0], "mh") == 65536 and "LT=16" in c[2] for _, c in every)
    # W H = 2^27, S % 16 != 0, no knob: k_update by size
    assert any(num(c[0], "W") * num(c[0], "H") == 1 << 27 and num(c[0], "S") % 16 and knobs(n)
               and any(k.startswith("k_update<") for k in kerns(c)) for n, c in every)
    # several views
    assert any(re.search(r"k_init_centers grid=\d+,\d+,([2-9]|\d\d)", c[0]) for _, c in every)
