"""Every kernel form of the superpixel plane sweep against the oracle, on built
inputs (tests/sweep_content.py; their states are pinned on the CPU by
tests/test_sweep_content_cpu.py).

launch_sweep_spixl picks one of k_sweep_spixl_ring<1|2|4> (HZ form on
LDS-staged rows), k_sweep_spixl<32|64, false, true> (HZ gathers),
k_sweep_spixl<32|64, false> (general gathers) and k_sweep_spixl<32|64, true>
(gathers from the copies k_relayout_lab<1|2|3> builds) from the level count,
the neighbour geometry, integer or fractional level products, the kSwU window
bound and MVS_SWEEP_{WPS,TRANSPOSE,HZ,RING} (read per call).  Each run here

  * hands lab, spixl (slot 7 NaN, the other slots random) and rep to the
    device as they are -- no SLIC, no k_boundary;
  * compares the WHOLE returned spixl tensor with orc.sweep's bit for bit:
    slot 7 written for every superpixel of the swept views, slots 0..6 and
    the other views untouched;
  * asserts through Engine.sweep_last_variant() the form it means to run."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd.engine import CameraArray
from oracle import oracle as orc
from tests import sweep_content as sc

pytestmark = pytest.mark.gpu

GENERAL, HZ_GATHER, HZ_RING, RELAID = 0, 1, 2, 3
SWITCHES = ("MVS_SWEEP_WPS", "MVS_SWEEP_TRANSPOSE", "MVS_SWEEP_HZ", "MVS_SWEEP_RING")


@functools.lru_cache(maxsize=None)
def _want(name, z0, z1):
    m = sc.make(name)
    return orc.sweep(m["lab"], m["spixl"], m["rep"], m["levels"], m["vs"], m["sn"], m["aw"], m["bl"], m["S"], z0, z1)


class Case:
    """The inputs of one sweep_content case on the device."""

    def __init__(self, engine, monkeypatch, name):
        self.eng, self.mp, self.name = engine, monkeypatch, name
        m = self.m = sc.make(name)
        self.cam = CameraArray(m["aw"], m["bl"], m["levels"], m["vs"], m["sn"])
        self.lab = torch.from_numpy(m["lab"]).cuda()
        self.spixl = torch.from_numpy(m["spixl"]).cuda()
        self.rep = torch.from_numpy(m["rep"]).cuda()

    def run(self, z0=0, z1=None, **env):
        """One sweep of views [z0, z1) under the MVS_SWEEP_* switches given
        (the others unset), checked against the oracle; returns the form report."""
        m = self.m
        z1 = m["V"] if z1 is None else z1
        for k in SWITCHES:
            self.mp.delenv(k, raising=False)
        for k, v in env.items():
            self.mp.setenv("MVS_SWEEP_" + k, str(v))
        sp = self.spixl.clone()
        assert torch.isnan(sp[..., 7]).all()
        self.eng.sweep_spixl(self.lab, sp, self.rep, self.cam, m["S"], z0, z1)
        got, want = sp.cpu().numpy(), _want(self.name, z0, z1)
        v = self.eng.sweep_last_variant()
        bad = got.view(np.uint32) != want.view(np.uint32)
        if bad.any():
            idx = np.argwhere(bad)
            pytest.fail(f"{self.name} views [{z0}, {z1}) {env} {v}: {len(idx)}/{got.size} words differ from the "
                        f"oracle; first (view, row, col, slot) {idx[:4].tolist()}: "
                        f"{[float(got[tuple(i)]) for i in idx[:4]]} vs {[float(want[tuple(i)]) for i in idx[:4]]}")
        assert not np.isnan(got[z0:z1, ..., 7]).any()
        return v

    def expect(self, form, lps=None, wps=None, z0=0, z1=None, **env):
        v = self.run(z0, z1, **env)
        assert v["FORM"] == form, (self.name, env, v)
        if lps is not None:
            assert v["LPS"] == lps, (self.name, env, v)
        if wps is not None:
            assert v["WPS"] == wps, (self.name, env, v)
        assert v["TMODE"] == int(env.get("TRANSPOSE", 2)), (self.name, env, v)
        if form != RELAID:
            assert v["RELAID"] == 0, (self.name, env, v)
        return v


def _own_wps(D):
    """The launcher's waves per superpixel: ceil(D / 64), three rounded up to four."""
    w = (D + 63) // 64
    return 4 if w >= 3 else w


# ---- every form on the same horizontal input ---------------------------------------
@pytest.mark.parametrize("D", [33, 64, 65, 130, 200])
@pytest.mark.parametrize("content", ["per64", "per16"])
def test_every_form_on_one_horizontal_input(engine, monkeypatch, content, D):
    """5 x 1 array, every other view a neighbour, S = 16, ties in 53-83 % of
    the superpixels at D >= 64 (30-50 % >= 64 levels apart at D >= 130): the ring
    kernel at 1, 2 and 4 waves per superpixel, the HZ gathers and the general
    gathers at 1, 2 and 4, all equal to the oracle (so to one another).  D =
    65: the second pass (or wave) has one live lane; D = 130: two waves of
    four idle."""
    c = Case(engine, monkeypatch, f"h5_{content}_d{D}")
    c.expect(HZ_RING, 64, 1)
    c.expect(HZ_GATHER, 64, _own_wps(D), RING=0)
    c.expect(GENERAL, 64, _own_wps(D), HZ=0)
    for w in (1, 2, 4):
        c.expect(HZ_RING, 64, w, WPS=w)
        c.expect(HZ_GATHER, 64, w, RING=0, WPS=w)
        c.expect(GENERAL, 64, w, HZ=0, WPS=w)
    c.expect(GENERAL, 64, _own_wps(D), HZ=0, TRANSPOSE=0)
    # a view sub-range: the other views' slot 7 stays NaN
    c.expect(HZ_RING, 64, 1, z0=1, z1=3)
    c.expect(HZ_GATHER, 64, _own_wps(D), z0=4, z1=5, RING=0)


@pytest.mark.parametrize("name", ["h3_s8_per16_d33", "h5_w48_per16_d70"])
def test_short_and_clipped_staging_windows(engine, monkeypatch, name):
    """S = 8 with |dx| = 1 and 33 levels: every staging window is under 64
    columns (one short LDS-DMA piece).  A 48-column image: every window is
    clipped by the image on one side or both."""
    c = Case(engine, monkeypatch, name)
    c.expect(HZ_RING, 64, 1)
    for w in (2, 4):
        c.expect(HZ_RING, 64, w, WPS=w)
    c.expect(HZ_GATHER, 64, RING=0)
    c.expect(GENERAL, 64, HZ=0)


# ---- the ring kernel's window bound, both sides --------------------------------------
@pytest.mark.parametrize("content", ["per16", "cheap"])
def test_window_bound_last_fit_and_first_miss(engine, monkeypatch, content):
    """4 x 1 array, 70 unit levels, every extent S - 1: S = 73 needs exactly
    kSwU = 336 columns by the launcher's bound and must run the ring kernel
    (unclipped 334-column windows are staged); S = 74 needs 338 and must fall
    to the HZ gathers."""
    c = Case(engine, monkeypatch, f"bound_s73_{content}")
    c.expect(HZ_RING, 64, 1)
    for w in (2, 4):
        c.expect(HZ_RING, 64, w, WPS=w)
    c.expect(HZ_GATHER, 64, 2, RING=0)
    c = Case(engine, monkeypatch, f"bound_s74_{content}")
    c.expect(HZ_GATHER, 64, 2)
    c.expect(HZ_GATHER, 64, 4, WPS=4)
    c.expect(GENERAL, 64, 2, HZ=0)


@pytest.mark.parametrize("content", ["per16", "per64"])
def test_production_fallback_to_hz_gathers(engine, monkeypatch, content):
    """S = 48 on the 5 x 1 array: 94 + 2 + 252 + 1 = 349 columns, past the ring
    kernel's slot, so k_sweep_spixl<64, false, true> runs -- here with 130
    levels (four waves per superpixel, two idle) and ties >= 64 levels apart
    in 70-80 % of the superpixels."""
    c = Case(engine, monkeypatch, f"bound_s48_{content}")
    c.expect(HZ_GATHER, 64, 4)
    for w in (1, 2, 4):
        c.expect(HZ_GATHER, 64, w, WPS=w)  # the window bound does not depend on the wave count
    c.expect(GENERAL, 64, 4, HZ=0)


# ---- the merge of the waves' winners ------------------------------------------------------
@pytest.mark.parametrize("form", ["ring", "hz", "general", "relaid"])
def test_merge_of_wave_winners_compares_level_indices(engine, monkeypatch, form):
    """300 levels, so a wave takes several 64-level passes and wave 0 also
    holds levels past those of the other waves; on these inputs 20-70 % of the
    superpixels have the first of their tied levels in another wave while wave
    0 ties with a later one (test_sweep_content_cpu).  The (cost, index)
    comparison of the LDS merge decides those -- in k_sweep_spixl at the
    launcher's own four waves, in k_sweep_spixl_ring under MVS_SWEEP_WPS."""
    if form == "relaid":
        c = Case(engine, monkeypatch, "merge_t")
        assert c.expect(RELAID, 64, 4)["RELAID"] > 0
        c.expect(GENERAL, 64, 4, TRANSPOSE=0)
        for w in (1, 2):
            c.expect(RELAID, 64, w, WPS=w)
            c.expect(GENERAL, 64, w, WPS=w, TRANSPOSE=0)
        return
    c = Case(engine, monkeypatch, "merge_h")
    want, env = {"ring": (HZ_RING, {}), "hz": (HZ_GATHER, dict(RING=0)), "general": (GENERAL, dict(HZ=0))}[form]
    c.expect(want, 64, 1 if form == "ring" else 4, **env)
    for w in (1, 2, 4):
        c.expect(want, 64, w, WPS=w, **env)


# ---- D <= 32: two superpixels per wave ------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 31, 32])
def test_two_superpixels_per_wave(engine, monkeypatch, D):
    """27 superpixels per view (odd: the last half-wave has no superpixel), HZ
    and general gathers on the 5 x 1 array, re-laid and general on the 3 x 3."""
    c = Case(engine, monkeypatch, f"half_h_d{D}")
    assert c.m["spixl"][0, ..., 0].size == 27
    c.expect(HZ_GATHER, 32, 1)
    c.expect(HZ_GATHER, 32, 1, WPS=4)  # ignored at D <= 32
    c.expect(GENERAL, 32, 1, HZ=0)
    c = Case(engine, monkeypatch, f"half_t_d{D}")
    for mode in (1, 2):
        assert c.expect(RELAID, 32, 1, TRANSPOSE=mode)["RELAID"] > 0
    c.expect(GENERAL, 32, 1, TRANSPOSE=0)
    assert c.expect(RELAID, 32, 1, z0=4, z1=7)["RELAID"] > 0


# ---- level lists ----------------------------------------------------------------------
@pytest.mark.parametrize("content", ["cheap", "per16"])
def test_level_lists(engine, monkeypatch, content):
    """3 x 1 array, both other views neighbours, S = 8.  Signed, descending and
    shuffled integer lists take the ring kernel (the staging window comes from
    the pass's lowest and highest level, wherever they sit); half steps are
    fractional for |dx| = 1 and must take the general form; half steps with
    only the |dx| = 2 neighbours are integer shifts again and must take an HZ
    form (view 1 then has no neighbour)."""
    for kind, D in (("signed", 41), ("desc", 70), ("shuffled", 70)):
        c = Case(engine, monkeypatch, f"lv_{kind}_{content}")
        assert c.m["D"] == D
        c.expect(HZ_RING, 64, 1)
        c.expect(HZ_RING, 64, 2, WPS=2)
        c.expect(HZ_GATHER, 64, _own_wps(D), RING=0)
        c.expect(GENERAL, 64, _own_wps(D), HZ=0)
    c = Case(engine, monkeypatch, f"lv_half_{content}")
    c.expect(GENERAL, 64, 2)
    c.expect(GENERAL, 64, 1, WPS=1)
    c.expect(GENERAL, 64, 2, RING=0)
    c = Case(engine, monkeypatch, f"lv_half_dx2_{content}")
    assert c.m["sn"].tolist() == [1, 0, 1]
    c.expect(HZ_RING, 64, 1)
    c.expect(HZ_GATHER, 64, 2, RING=0)
    c.expect(GENERAL, 64, 2, HZ=0)


# ---- 2-D arrays and the re-laid copies ---------------------------------------------------
@pytest.mark.parametrize("size", list(sc.SIZES_2D))
@pytest.mark.parametrize("D", [32, 130, 200])
@pytest.mark.parametrize("bl", [1.0, 1.0359])
@pytest.mark.parametrize("content", ["p2d16", "cheap"])
@pytest.mark.parametrize("array", ["a3x3", "a8x4"])
def test_2d_arrays_row_major_and_relaid(engine, monkeypatch, array, content, bl, D, size):
    """3 x 3 with the 8 surrounding views and 8 x 4 with 5 nearest neighbours;
    images of 150 x 45, 70 x 27 (H < 32) and 45 x 100 (H > W), neither
    dimension a multiple of k_relayout_lab's 32 x 32 tile.  Row-major gathers
    (MVS_SWEEP_TRANSPOSE=0), transposed vertical neighbours (1) and sheared
    diagonal ones too (2): all equal to the oracle.  200 levels: four waves
    per superpixel; 130: two of four idle; 32: two superpixels per wave."""
    c = Case(engine, monkeypatch, f"{array}_{content}_bl{bl}_d{D}_{size}")
    lps, wps = (32, 1) if D <= 32 else (64, 4)
    v0 = c.expect(GENERAL, lps, wps, TRANSPOSE=0)
    assert v0["RELAID"] == 0
    v1 = c.expect(RELAID, lps, wps, TRANSPOSE=1)
    v2 = c.expect(RELAID, lps, wps, TRANSPOSE=2)
    assert 0 < v1["RELAID"] < v2["RELAID"], (v1, v2)  # mode 2 adds the sheared copies
    assert c.expect(RELAID, lps, wps) == v2  # the default is mode 2
    if D > 32 and size == "70x27":
        for w in (1, 2):
            c.expect(RELAID, 64, w, WPS=w)
            c.expect(GENERAL, 64, w, WPS=w, TRANSPOSE=0)


def test_camera_rows_with_and_without_vertical_neighbours(engine, monkeypatch):
    """3 x 2 array: views 0-2 list their horizontal neighbours only, views 3-5
    also the camera above.  The range (0, 3) runs an HZ form, (3, 6) and
    (0, 6) the re-laid one; each equals the oracle on its views and leaves the
    others alone."""
    c = Case(engine, monkeypatch, "a3x2_rows")
    assert c.m["sn"].tolist() == [2, 2, 2, 3, 3, 3]
    c.expect(HZ_RING, 64, 1, z0=0, z1=3)
    c.expect(HZ_GATHER, 64, 2, z0=0, z1=3, RING=0)
    assert c.expect(RELAID, 64, 2, z0=3, z1=6)["RELAID"] == 3  # views 0-2 transposed
    assert c.expect(RELAID, 64, 2, z0=0, z1=6)["RELAID"] == 3
    c.expect(GENERAL, 64, 2, z0=3, z1=6, TRANSPOSE=0)
    c.expect(HZ_RING, 64, 1, z0=1, z1=2)


# ---- degenerate content ----------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "noise", "empty"])
def test_degenerate_content_through_every_form(engine, monkeypatch, kind):
    """flat: every level pair ties and level index 0 (value 5) must win.
    noise: the all-outside cost 750 wins at the first level that reaches it.
    empty: reference view 1 has no neighbour and gets +0.0.  Ring, HZ gathers
    and general on the 5 x 1 array; re-laid and general on the 3 x 3."""
    c = Case(engine, monkeypatch, f"{kind}_h")
    D = c.m["D"]
    c.expect(HZ_RING, 64, 1)
    for w in (2, 4):
        c.expect(HZ_RING, 64, w, WPS=w)
    c.expect(HZ_GATHER, 64, _own_wps(D), RING=0)
    c.expect(GENERAL, 64, _own_wps(D), HZ=0)
    c.expect(HZ_RING, 64, 1, z0=1, z1=2)
    c = Case(engine, monkeypatch, f"{kind}_t")
    assert c.expect(RELAID, 64, _own_wps(D))["RELAID"] > 0
    assert c.expect(RELAID, 64, _own_wps(D), TRANSPOSE=1)["RELAID"] > 0
    c.expect(GENERAL, 64, _own_wps(D), TRANSPOSE=0)
    # view 1 alone: with no neighbour nothing is re-laid and nothing leaves its camera row
    c.expect(HZ_RING if kind == "empty" else RELAID, 64, 1 if kind == "empty" else _own_wps(D), z0=1, z1=2)
