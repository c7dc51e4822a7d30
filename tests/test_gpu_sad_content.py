"""Every kernel of the per-pixel SAD sweep against the oracle, on built inputs
(tests/sad_content.py; their states are pinned on the CPU by
tests/test_sad_content_cpu.py).

plan_sad picks, per reference view, one of six k_sad_band instantiations
(16- or 8-level chunks; rows addressed affinely on a 64- or 128-column band, or
through the row table) or the gather kernel k_sweep_pixel_sad, from the level
list, the neighbour geometry, bl_ratio and MVS_SAD_{KERNEL,AFF} (read per
call).  Each run here

  * hands Lab to the device as a float tensor as it is -- no cvt: magnitudes
    up to 100 per channel, a NaN fourth channel;
  * sweeps every view in one call and compares with orc.sweep_pixel_sad bit
    for bit;
  * names each band form in turn and expects the oracle's bits where the case
    table says the form can stage every view, the "cannot stage" error where
    it says it cannot -- so the table is checked against the planner;
  * runs the cases whose row shifts are all integral through the row table
    too (MVS_SAD_AFF set)."""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd.engine import CameraArray
from oracle import oracle as orc
from tests import sad_content as sd

pytestmark = pytest.mark.gpu

SWITCHES = ("MVS_SAD_KERNEL", "MVS_SAD_AFF")
SENTINEL = 0x7FC5A5A5  # a NaN no sweep produces


@functools.lru_cache(maxsize=None)
def _want(name):
    m = sd.make(name)
    return orc.sweep_pixel_sad(m["lab"], m["levels"], m["vs"], m["sn"], m["aw"], m["bl"])


class Case:
    """The inputs of one sad_content case on the device."""

    def __init__(self, engine, monkeypatch, name):
        self.eng, self.mp, self.name = engine, monkeypatch, name
        m = self.m = sd.make(name)
        self.cam = CameraArray(m["aw"], m["bl"], m["levels"], m["vs"], m["sn"])
        self.lab = torch.from_numpy(m["lab"]).cuda()

    def env(self, kernel=None, table=False):
        for k in SWITCHES:
            self.mp.delenv(k, raising=False)
        if kernel:
            self.mp.setenv("MVS_SAD_KERNEL", kernel)
        if table:
            self.mp.setenv("MVS_SAD_AFF", "0")
        return f"{self.name} kernel={kernel or 'unset'}{' row table' if table else ''}"

    def check(self, got, z0, tag):
        """got [z1 - z0, H, W] against the oracle's views z0 .., bit for bit."""
        want = _want(self.name)[z0:z0 + got.shape[0]]
        assert got.shape == want.shape and got.dtype == np.float32, (tag, got.shape, want.shape)
        bad = got.view(np.uint32) != want.view(np.uint32)
        for z in range(got.shape[0]):
            if bad[z].any():
                idx = np.argwhere(bad[z])
                pytest.fail(f"{tag} view {z0 + z}: {len(idx)}/{bad[z].size} disparities differ from the oracle; first "
                            f"(y, x) {idx[:3].tolist()}: {[float(got[z][tuple(i)]) for i in idx[:3]]} vs "
                            f"{[float(want[z][tuple(i)]) for i in idx[:3]]}")

    def run(self, kernel=None, table=False):
        """One sweep of every view under the switches given (the others unset), checked against the oracle."""
        tag = self.env(kernel, table)
        self.check(self.eng.sweep_pixel_sad(self.lab, self.cam).cpu().numpy(), 0, tag)

    def refuses(self, kernel):
        """The named band form cannot stage some view: the call fails loudly, it does not fall back."""
        tag = self.env(kernel)
        with pytest.raises(Exception, match="cannot stage"):
            self.eng.sweep_pixel_sad(self.lab, self.cam)
            pytest.fail(f"{tag}: ran, but the case table says the form cannot stage every view")


@pytest.mark.parametrize("name", list(sd.CASES))
def test_every_kernel_on_built_inputs(engine, monkeypatch, name):
    """The planner's own choice, each band form named, the gather kernel, and
    the row-table path of the affine cases: all equal to the oracle, or the
    "cannot stage" error where the table says a band form does not fit."""
    c = Case(engine, monkeypatch, name)
    c.run()
    for form in sd.FORMS:
        fits = all(form in f for f in c.m["forms"])
        if fits:
            c.run(form)
            if c.m["affine"]:
                c.run(form, table=True)
        else:
            c.refuses(form)
    c.run("gather")
    if c.m["affine"]:
        c.run(table=True)


@pytest.mark.parametrize("kernel", [None, "sys8x2", "sys8", "gather"])
@pytest.mark.parametrize("name", ["signed_t_bl1", "half_h", "noise_h", "tiny_3x2"])
def test_only_the_views_asked_for_are_written(engine, monkeypatch, name, kernel):
    """Views [1, V - 1) into the middle of a buffer filled with a NaN bit
    pattern, one guard plane before and one after: every pixel of the swept
    views is written (and equals the oracle), the guards keep their bits."""
    c = Case(engine, monkeypatch, name)
    if kernel in sd.FORMS and not all(kernel in f for f in c.m["forms"]):
        c.refuses(kernel)
        return
    tag = c.env(kernel)
    V, H, W = c.m["V"], c.m["H"], c.m["W"]
    z0, z1 = 1, V - 1
    buf = torch.full((z1 - z0 + 2, H, W), SENTINEL, dtype=torch.int32, device=c.lab.device).view(torch.float32)
    out = c.eng.sweep_pixel_sad(c.lab, c.cam, z0, z1, out=buf[1:-1])
    assert out.data_ptr() == buf[1:-1].data_ptr()
    got = buf.cpu().numpy()
    for g, where in ((0, "before"), (-1, "after")):
        hit = np.argwhere(got[g].view(np.uint32) != SENTINEL)
        assert len(hit) == 0, (f"{tag}: {len(hit)} words of the guard plane {where} the output written, "
                               f"first (y, x) {hit[:3].tolist()}")
    left = np.argwhere(got[1:-1].view(np.uint32) == SENTINEL)
    assert len(left) == 0, f"{tag}: {len(left)} output pixels not written, first (view, y, x) {left[:3].tolist()}"
    c.check(got[1:-1], z0, tag)
