"""k_sweep_spixl_ring's two row-step paths against the oracle, on built inputs.

Per (64-level pass, neighbour) the ring kernel takes its whole-window path --
all 25 reference taps inside the image and no lane's tap column outside it, so
the tap addresses are set once and the 25-tap chain runs without the outside
marker -- or else the general row-steps.  MVS_SWEEP_RING_FAST=0 (read per
call, a kernel argument, no part of the plan) forces the general row-steps
everywhere.  Every case here runs under both settings; slot 7 of the returned
spixl (and everything else in it) must equal orc.sweep's bit for bit, and
mvs_sweep_last_variant_n must report the ring form.

Inputs are made by hand as in tests/sweep_content.py: Lab contents, centres
and extents as plain arrays, no SLIC and no k_boundary.

  interior   5 x 1 array, 640 x 128, S = 32, levels 0 .. 127 (two passes), the
             centres on the plain grid: both signs of dx, |dx| up to 4, the
             whole-window path on most (pass, neighbour) pairs of the inner
             superpixels, the general one at the image's sides.
  narrow     200 x 96, S = 16, levels 0 .. 69: D no multiple of 64 (the last
             pass has 58 idle lanes), windows clamped at both borders, lanes of
             one pass projecting outside while others do not.
  single     D = 33, one neighbour per view: one pass, nothing staged ahead
             for a next neighbour.
  edges      centres on the image's first and last column and row with extents
             up to S - 1, so reference taps leave the image in rows and in
             columns; cells of extent 0 whose staged window is under 64 columns
             (one short LDS-DMA piece)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd.engine import CameraArray
from oracle import oracle as orc
from tests import sweep_content as sc

pytestmark = pytest.mark.gpu

HZ_RING = 2
K_SW_U = 336  # kSwU (launch_plan.h): the columns of a ring slot
SWITCHES = ("MVS_SWEEP_WPS", "MVS_SWEEP_TRANSPOSE", "MVS_SWEEP_HZ", "MVS_SWEEP_RING", "MVS_SWEEP_RING_FAST")

# name: content, aw, W, H, S, D, the neighbour lists, grid centres (True) or sc.geometry's border centres,
# the reference views swept (each in a launch of its own)
CASES = {
    "interior": dict(content="cheap", aw=5, W=640, H=128, S=32, D=128, cam=dict(nh=4), grid=True, refs=(0, 2, 4)),
    "narrow": dict(content="per16", aw=5, W=200, H=96, S=16, D=70, cam=dict(nh=4), grid=False, refs=(0, 2, 4)),
    "single": dict(content="per16", aw=2, W=160, H=48, S=16, D=33, cam=dict(nh=1), grid=False, refs=(0, 1)),
    "edges": dict(content="cheap", aw=3, W=120, H=40, S=16, D=33, cam=dict(nh=2), grid=False, refs=(0, 1, 2)),
}


@functools.lru_cache(maxsize=None)
def _inputs(name):
    c = CASES[name]
    V = c["aw"]
    sp, rep = sc.geometry(V, c["W"], c["H"], c["S"])
    if c["grid"]:  # the plain grid's centres (quarter-pixel fractions kept): none on the image border
        mh, mw = sp.shape[1:3]
        frac = sp[..., 1:3] - np.floor(sp[..., 1:3])
        sp[..., 1] = (np.arange(mw) * c["S"] + c["S"] // 2).astype(np.float32)[None, None, :] + frac[..., 0]
        sp[..., 2] = (np.arange(mh) * c["S"] + c["S"] // 2).astype(np.float32)[None, :, None] + frac[..., 1]
        assert (sp[..., 1] < c["W"]).all() and (sp[..., 2] < c["H"]).all()
    vs, sn = sc.camera(c["aw"], 1, **c["cam"])
    m = dict(c, V=V, lab=sc.lab(c["content"], c["aw"], 1, c["W"], c["H"]), spixl=sp, rep=rep,
             levels=sc.level_list("unit", c["D"]), vs=vs, sn=sn, bl=1.0)
    return m  # (shared: nothing below writes to these arrays)


@functools.lru_cache(maxsize=None)
def _want(name, z):
    m = _inputs(name)
    return orc.sweep(m["lab"], m["spixl"], m["rep"], m["levels"], m["vs"], m["sn"], m["aw"], m["bl"], m["S"], z, z + 1)


def _max_dx(m):
    vs = np.asarray(m["vs"]).reshape(m["V"], m["V"])
    return max(abs(int(vs[z, k]) % m["aw"] - z % m["aw"]) for z in range(m["V"]) for k in range(int(m["sn"][z])))


def _tap_steps(m, z):
    """(stx, sty) per superpixel of view z, the kernel's float arithmetic."""
    dr = m["rep"][z].reshape(-1, 8).astype(np.int64)
    lr = np.maximum(dr[:, 0], np.maximum(dr[:, 1], dr[:, 2])) + np.maximum(dr[:, 5], np.maximum(dr[:, 6], dr[:, 7]))
    tb = np.maximum(dr[:, 0], np.maximum(dr[:, 3], dr[:, 5])) + np.maximum(dr[:, 2], np.maximum(dr[:, 4], dr[:, 7]))
    f = lambda s: np.maximum(1.0, 0.25 * s.astype(np.float32).astype(np.float64)).astype(np.float32)
    return f(lr), f(tb)


def _ref_taps(m, z):
    """Reference tap columns [M, 5] and rows [M, 5] of view z (possibly outside the image)."""
    sp = m["spixl"][z].reshape(-1, 8)
    stx, sty = _tap_steps(m, z)
    i = np.arange(-2, 3).astype(np.float32)[None, :]
    return (np.trunc(sp[:, 1:2] + i * stx[:, None]).astype(np.int64),
            np.trunc(sp[:, 2:3] + i * sty[:, None]).astype(np.int64))


def _run(engine, monkeypatch, name, **env):
    m = _inputs(name)
    # the launcher's window bound for the ring form, on the CPU
    assert 2 * (m["S"] - 1) + 2 + 63 * _max_dx(m) <= K_SW_U, name
    cam = CameraArray(m["aw"], m["bl"], m["levels"], m["vs"], m["sn"])
    lab = torch.from_numpy(m["lab"]).cuda()
    spixl = torch.from_numpy(m["spixl"]).cuda()
    rep = torch.from_numpy(m["rep"]).cuda()
    for fast in (None, 0):
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv("MVS_SWEEP_" + k, str(v))
        if fast is not None:
            monkeypatch.setenv("MVS_SWEEP_RING_FAST", str(fast))
        for z in m["refs"]:
            sp = spixl.clone()
            engine.sweep_spixl(lab, sp, rep, cam, m["S"], z, z + 1)
            v = engine.sweep_last_variant()
            assert v["FORM"] == HZ_RING, (name, z, fast, env, v)
            assert v["WPS"] == int(env.get("WPS", 1)), (name, z, fast, env, v)
            got, want = sp.cpu().numpy(), _want(name, z)
            bad = got.view(np.uint32) != want.view(np.uint32)
            if bad.any():
                idx = np.argwhere(bad)
                pytest.fail(f"{name} view {z} MVS_SWEEP_RING_FAST={fast} {env}: {len(idx)}/{got.size} words differ "
                            f"from the oracle; first (view, row, col, slot) {idx[:4].tolist()}: "
                            f"{[float(got[tuple(i)]) for i in idx[:4]]} vs {[float(want[tuple(i)]) for i in idx[:4]]}")
            assert not np.isnan(got[z, ..., 7]).any()


def test_interior_whole_windows(engine, monkeypatch):
    """Two 64-level passes, dx from -4 to 4; most superpixels have all 25
    reference taps inside, and of those most (pass, neighbour) pairs keep
    every lane's columns inside (the whole-window path), the rest do not."""
    m = _inputs("interior")
    W, H = m["W"], m["H"]
    for z in m["refs"]:
        xr, yr = _ref_taps(m, z)
        full = ((xr >= 0) & (xr < W)).all(1) & ((yr >= 0) & (yr < H)).all(1)
        assert full.mean() > 0.5, (z, full.mean())
        # whole windows: for some superpixels at every dx of the view, for others at none or some
        whole = np.zeros(len(xr), np.int64)
        for v in range(m["V"]):
            if v != z:
                for lo in (0, 64):
                    sh = np.array([lo, lo + 63]) * (v - z)
                    whole += full & (xr.min(1) - sh.max() >= 0) & (xr.max(1) - sh.min() < W)
        assert (whole == 8).any() and (whole[full] < 8).any(), (z, np.bincount(whole))
    _run(engine, monkeypatch, "interior")


def test_narrow_image_clamped_windows_and_idle_lanes(engine, monkeypatch):
    """200 columns against shifts up to 4 x 69: every window of the outer
    neighbours is clamped on a side, and the second pass has 6 live lanes."""
    m = _inputs("narrow")
    assert m["D"] % 64 == 6
    _run(engine, monkeypatch, "narrow")


def test_narrow_image_two_waves_per_superpixel(engine, monkeypatch):
    """The <2> instantiation (MVS_SWEEP_WPS=2): each wave one pass, the winners merged through LDS."""
    _run(engine, monkeypatch, "narrow", WPS=2)


def test_single_pass_single_neighbour(engine, monkeypatch):
    m = _inputs("single")
    assert m["D"] == 33 and m["sn"].tolist() == [1, 1]
    _run(engine, monkeypatch, "single")


def test_edges_outside_taps_and_short_windows(engine, monkeypatch):
    """Reference taps outside the image in rows (first and last map row) and in
    columns (first and last map column), and superpixels of extent 0 whose
    window towards a |dx| = 1 neighbour is 5 + 32 columns."""
    m = _inputs("edges")
    W, H = m["W"], m["H"]
    for z in m["refs"]:
        xr, yr = _ref_taps(m, z)
        assert (xr < 0).any() and (xr >= W).any() and (yr < 0).any() and (yr >= H).any()
        inside = (xr >= 0) & (xr < W)
        span = np.where(inside, xr, -1).max(1) - np.where(inside, xr, 1 << 30).min(1) + 1 + (m["D"] - 1)
        assert (span < 64).any(), (z, span.min())
    _run(engine, monkeypatch, "edges")
