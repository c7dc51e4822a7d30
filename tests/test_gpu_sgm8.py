"""The diagonal paths of the semi-global aggregation (csrc/sgm.hip, mvs_sgm8_d)
against the definition in tests/sgm8_ref.py, bit for bit.

Random volumes walk the level counts on and around every boundary of the two
kernel forms (a wave's chunk of 16 levels, the two thread-limit instantiations
of the sheared form at 8 and 9 waves, its last level count 256, the first of the
lanes form 257, several waves per line at 1100) over image sizes that give one
full workgroup of 64 diagonals, one more, several, H >> W (clipped row ranges),
W >> H and one-pixel lines; every mask and every penalty pair meets every level
count.  Before the GPU is compared, the reference's eight single-path volumes
are shown to differ pairwise on at least 0.15 of the cells (every shape with D,
H, W >= 3, every pair with P2 > 0), so a kernel that walks the wrong diagonal
cannot pass.

Unaligned bases, mvs_sgm8_d with masks 1..15 against mvs_sgm_d, natural volumes
(orc.ncc_volume on a synthetic stack), `out=` reuse, the pipeline's
`sgm_paths` and the argument errors follow."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd import _lib, params, synth
from cl_multiview_stereo_amd.pipeline import Pipeline, PixelSweep
from oracle import oracle as orc
from tests import sgm8_ref as s8
from tests import sgm_ref as sg

pytestmark = pytest.mark.gpu

MASKS = [16, 32, 64, 128, 48, 192, 240, 255, 0x55, 17]
PEN = [(0.1, 0.8), (0.0, 0.0), (0.25, 0.25), (0.5, 4.0)]
DS = [1, 2, 16, 17, 64, 65, 128, 130, 256, 257]
# (H, W): 75 and 71 diagonals (two workgroups); 64 (one full workgroup); 65; H >> W, 132 diagonals (three workgroups
# with clipped row ranges); 75; one-pixel lines
SIZES = [(6, 70), (5, 67), (2, 63), (2, 64), (130, 3), (70, 6), (4, 1), (1, 7), (1, 1)]
SHAPES = [(D, H, W) for D in DS for H, W in SIZES] + [(1100, 3, 5)]  # 1100: two waves per line of the lanes form


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.count_nonzero(a != b)
    assert bad == 0, f"{what}: {bad}/{a.size} differ, first at {np.argwhere(a != b)[:3].tolist()}"


def pen_of(i, k, H, W):
    """The penalty pair of mask i on shape k: it rotates with both, as in test_gpu_sgm.py."""
    return PEN[(i + k) % 4] if H * W > 1 else PEN[i % 4]


class Singles:
    """The reference's eight single-path volumes of one volume, per penalty pair, computed once."""

    def __init__(self, vol):
        self.vol, self.L = vol, {}

    def get(self, P1, P2):
        if (P1, P2) not in self.L:
            self.L[(P1, P2)] = [s8.single(self.vol, b, P1, P2) for b in range(8)]
        return self.L[(P1, P2)]

    def agg(self, P1, P2, mask):
        out = None
        for b, L in enumerate(self.get(P1, P2)):
            if mask >> b & 1:
                out = L if out is None else out + L
        return out


def not_vacuous(ref, P1, P2, what, least=0.15):
    """The reference's eight single-path volumes differ pairwise (see the module's text)."""
    L = ref.get(P1, P2)
    share = min(float((L[i] != L[j]).mean()) for i in range(8) for j in range(i))
    if P2 > 0:
        assert share >= least, (what, share)
    return share


# ---- 1. random volumes -------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_volumes(engine, shape):
    D, H, W = shape
    k = SHAPES.index(shape)
    vol = sg.random_volume(D, H, W, seed=300 + k)
    ref = Singles(vol)
    if D >= 3 and H >= 3 and W >= 3:
        for P1, P2 in PEN:
            not_vacuous(ref, P1, P2, (shape, P1, P2))
    gv = torch.from_numpy(vol).cuda()
    out = engine.empty(shape, torch.float32)
    for i, mask in enumerate(MASKS):
        P1, P2 = pen_of(i, k, H, W)
        want = ref.agg(P1, P2, mask)
        out.fill_(float("nan"))  # stale contents must not show
        got = engine.sgm(gv, P1, P2, mask, out=out)
        assert got.data_ptr() == out.data_ptr()
        same(got, want, f"D{D} H{H} W{W} paths={mask} P1={P1} P2={P2}")
    same(gv, vol, "the volume is left as it was")


def test_reference_sums_as_sgm8():
    """Singles.agg above is sgm8_ref.sgm8: the same sum in the same order."""
    vol = sg.random_volume(17, 5, 9, seed=9)
    ref = Singles(vol)
    for mask in MASKS:
        same(ref.agg(0.1, 0.8, mask), s8.sgm8(vol, 0.1, 0.8, mask), f"paths={mask}")


def test_every_mask_and_penalty_meets_every_level_count():
    seen = {}
    for k, (D, H, W) in enumerate(SHAPES):
        for i, mask in enumerate(MASKS):
            seen.setdefault(D, set()).add((mask, pen_of(i, k, H, W)))
    for D in DS:
        assert {m for m, _ in seen[D]} == set(MASKS) and {p for _, p in seen[D]} == set(PEN), D
    assert {m for m, _ in seen[1100]} == set(MASKS)


@pytest.mark.parametrize("paths", [240, 255])
def test_unaligned_bases(engine, paths):
    """vol and agg one and three floats past a 16-byte boundary, and the two on different boundaries."""
    D, H, W = 66, 5, 67
    vol = sg.random_volume(D, H, W, seed=7)
    want = s8.sgm8(vol, 0.1, 0.8, paths)
    n = D * H * W
    for ov, oa in ((1, 1), (3, 3), (1, 0), (0, 2)):
        bv = engine.empty((n + 4,), torch.float32)
        ba = engine.empty((n + 4,), torch.float32).fill_(float("nan"))
        gv = bv[ov:ov + n].view(D, H, W)
        gv.copy_(torch.from_numpy(vol))
        ga = ba[oa:oa + n].view(D, H, W)
        assert gv.data_ptr() % 16 == 4 * ov and ga.data_ptr() % 16 == 4 * oa
        same(engine.sgm(gv, 0.1, 0.8, paths, out=ga), want, f"offsets {ov}, {oa} floats")
        pad = np.concatenate([bits(ba[:oa]), bits(ba[oa + n:])])
        assert (pad == bits(np.float32("nan"))).all(), "a store outside agg"


def test_masks_up_to_15_are_mvs_sgm_d(engine):
    D, H, W = 66, 5, 67
    vol = torch.from_numpy(sg.random_volume(D, H, W, seed=8)).cuda()
    a4, a8 = engine.empty((D, H, W), torch.float32), engine.empty((D, H, W), torch.float32)
    for paths in range(1, 16):
        a8.fill_(float("nan"))
        engine.sgm(vol, 0.1, 0.8, paths, out=a4)  # mvs_sgm_d
        _lib.check(engine.L.mvs_sgm8_d(engine.ctx, W, H, D, vol.data_ptr(), 0.1, 0.8, paths, a8.data_ptr()), "mvs_sgm8_d")
        same(a8, a4, f"paths={paths}")


# ---- 2. natural volumes --------------------------------------------------------------
AW, NW_, NH_ = 5, 300, 40


def _settings(dmax=31):
    return params.Settings(spixl_size=8, array_width=AW, array_height=1, neib_hor=1, neib_ver=0, min_disp=0,
                           max_disp=dmax, inc=1, bl_ratio=1.0, window=5)


@pytest.fixture(scope="module")
def natural():
    """test_gpu_sgm.py's stack, its oracle volumes over levels 0..31 and their winners raw, with four and with eight
    paths, all five views."""
    stack, _ = synth.make_stack(NW_, NH_, AW, 1, 4, 27, 1.0, 0x5EED + 13)
    l8 = orc.l8(orc.cvt(stack))
    vs, sn = params.flatten_subsets(params.neighbour_lists(AW, 1, 1, 0))
    levels = params.disparity_levels(0, 31, 1)
    vols = [orc.ncc_volume(l8, levels, vs, sn, AW, 1.0, 5, z) for z in range(AW)]
    agg8 = [s8.sgm8(v, 0.1, 0.8, 255) for v in vols]
    raw = [orc.wta(v, levels) for v in vols]
    win4 = [orc.wta(sg.sgm(v, 0.1, 0.8, 15), levels) for v in vols]
    win8 = [orc.wta(a, levels) for a in agg8]
    return stack, l8, vols, agg8, raw, win4, win8


def _moved(win4, win8, what):
    """Asserted first: the eight-path winner differs from the four-path winner on some pixels of every view."""
    share = [float((a[0] != b[0]).mean()) for a, b in zip(win4, win8)]
    print(f"{what}: the 8-path winner differs from the 4-path one on {['%.3f' % s for s in share]} of the pixels")
    assert min(share) > 0, (what, share)


@pytest.mark.parametrize("dmax", [31, 127])
def test_natural_volumes(engine, natural, dmax):
    stack, l8h, vols, agg8, raw, win4, win8 = natural
    cam = Pipeline(engine, _settings(dmax), NW_, NH_, pixel_cost="ncc").cam
    levels = cam.levels
    if dmax != 31:
        vols = [orc.ncc_volume(l8h, levels, cam.view_subset, cam.subset_num, AW, 1.0, 5, z) for z in range(AW)]
        agg8 = [s8.sgm8(v, 0.1, 0.8, 255) for v in vols]
        win4 = [orc.wta(sg.sgm(v, 0.1, 0.8, 15), levels) for v in vols]
        win8 = [orc.wta(a, levels) for a in agg8]
    _moved(win4, win8, f"levels 0..{dmax}")
    _, l8 = engine.cvt(torch.from_numpy(stack).cuda())
    box = engine.box_stats(l8, 5)
    lev = engine.levels_dev(cam)
    for z in range(AW):
        gv = engine.ncc_volume(l8, box, cam, z, 5)
        same(gv, vols[z], f"volume z{z}")
        ga = engine.sgm(gv, paths=255)
        same(ga, agg8[z], f"aggregate z{z} levels 0..{dmax}")
        d, c = engine.wta(ga, lev)
        same(d, win8[z][0], f"aggregated disp z{z} levels 0..{dmax}")
        same(c, win8[z][1], f"aggregated conf z{z} levels 0..{dmax}")


# ---- 3. out= reuse ---------------------------------------------------------------------
def test_out_reuse_across_two_volumes(engine):
    """The first path stores, it does not add: nothing of the first aggregate shows in the second."""
    D, H, W = 33, 7, 45
    a, b = sg.random_volume(D, H, W, seed=11), sg.random_volume(D, H, W, seed=12)
    out = engine.empty((D, H, W), torch.float32)
    for paths in (255, 128, 96):
        same(engine.sgm(torch.from_numpy(a).cuda(), paths=paths, out=out), s8.sgm8(a, paths=paths), f"first, paths={paths}")
        same(engine.sgm(torch.from_numpy(b).cuda(), paths=paths, out=out), s8.sgm8(b, paths=paths), f"second, paths={paths}")


# ---- 4. pipeline -----------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_pipeline(engine, natural, fused):
    stack, _, vols, agg8, raw, win4, win8 = natural
    _moved(win4, win8, "pipeline")
    rgbx = torch.from_numpy(stack).cuda()
    on = Pipeline(engine, _settings(), NW_, NH_, pixel_cost="ncc", fused=fused, sgm=True, sgm_paths=255).exe_pipeline(rgbx)
    off = Pipeline(engine, _settings(), NW_, NH_, pixel_cost="ncc", fused=fused).exe_pipeline(rgbx)
    dflt = Pipeline(engine, _settings(), NW_, NH_, pixel_cost="ncc", fused=fused, sgm=True).exe_pipeline(rgbx)
    assert tuple(on.disp_agg.shape) == tuple(on.conf_agg.shape) == tuple(on.disp.shape) == (AW, NH_, NW_)
    same(on.disp, off.disp, f"disp with and without sgm, fused {fused}")
    same(on.conf, off.conf, f"conf with and without sgm, fused {fused}")
    for z in range(AW):
        same(on.disp[z], raw[z][0], f"pipeline disp z{z} fused {fused}")
        same(on.conf[z], raw[z][1], f"pipeline conf z{z} fused {fused}")
        same(on.disp_agg[z], win8[z][0], f"pipeline disp_agg z{z} fused {fused}")
        same(on.conf_agg[z], win8[z][1], f"pipeline conf_agg z{z} fused {fused}")
        # sgm_paths left at its default: the four paths, as before
        same(dflt.disp_agg[z], win4[z][0], f"default disp_agg z{z} fused {fused}")
        same(dflt.conf_agg[z], win4[z][1], f"default conf_agg z{z} fused {fused}")


@pytest.mark.parametrize("fused", [True, False])
def test_pixel_sweep_view_shard(engine, natural, fused):
    """Reference views [1, 4), the four diagonal paths alone."""
    stack, _, vols, agg8, raw, win4, win8 = natural
    lab, l8 = engine.cvt(torch.from_numpy(stack).cuda())
    cam = Pipeline(engine, _settings(), NW_, NH_, pixel_cost="ncc").cam
    ps = PixelSweep(engine, cam, NW_, NH_, "ncc", 5, fused=fused, sgm=True, sgm_paths=240)
    disp, conf = ps.run(lab, l8, 1, 4, views=cam.views_needed(1, 4))
    assert tuple(ps.disp_agg.shape) == tuple(ps.conf_agg.shape) == (3, NH_, NW_)
    for i, z in enumerate(range(1, 4)):
        wd, wc = orc.wta(s8.sgm8(vols[z], 0.1, 0.8, 240), cam.levels)
        assert (wd != win8[z][0]).any()  # the mask reaches the kernel
        same(disp[i], raw[z][0], f"shard disp z{z}")
        same(conf[i], raw[z][1], f"shard conf z{z}")
        same(ps.disp_agg[i], wd, f"shard disp_agg z{z}")
        same(ps.conf_agg[i], wc, f"shard conf_agg z{z}")


# ---- 5. errors -------------------------------------------------------------------------
def test_errors(engine):
    D, H, W = 4, 3, 5
    vol = torch.from_numpy(sg.random_volume(D, H, W, seed=1)).cuda()
    agg = engine.empty((D, H, W), torch.float32)
    L, ctx = engine.L, engine.ctx
    v, a = vol.data_ptr(), agg.data_ptr()

    def rc(ctx=ctx, W=W, H=H, D=D, v=v, P1=0.1, P2=0.8, paths=255, a=a):
        r = L.mvs_sgm8_d(ctx, W, H, D, v, P1, P2, paths, a)
        if r != 0:
            assert b"mvs_sgm8_d" in L.mvs_last_error() or b"sgm" in L.mvs_last_error()
        return r

    assert rc() == 0
    assert rc(ctx=None) == -1 and rc(v=None) == -1 and rc(a=None) == -1
    assert b"mvs_sgm8_d" in L.mvs_last_error()
    assert rc(W=0) == -1 and rc(H=0) == -1 and rc(W=-3) == -1 and rc(W=1 << 20, H=1 << 20) == -1
    assert rc(D=0) == -1 and rc(D=-1) == -1 and rc(D=16385) == -1
    for paths in (0, 256, -1):
        assert rc(paths=paths) == -1, paths
        assert b"mvs_sgm8_d: paths must be a mask in 1..255" in L.mvs_last_error()
    inf, nan = float("inf"), float("nan")
    for P1, P2 in ((-0.1, 0.8), (0.1, -0.8), (0.9, 0.8), (nan, 0.8), (0.1, nan), (0.1, inf), (inf, inf), (-inf, 0.8)):
        assert rc(P1=P1, P2=P2) == -1, (P1, P2)
    assert rc(a=v) == -1
    assert rc(P1=0.0, P2=0.0) == 0 and rc(P1=0.5, P2=0.5) == 0 and rc(paths=16) == 0 and rc(paths=1) == 0
    with pytest.raises(_lib.MvsError, match="agg must not be vol"):
        engine.sgm(vol, paths=255, out=vol)
    with pytest.raises(_lib.MvsError, match="mvs_sgm8_d: paths must be a mask in 1..255"):
        engine.sgm(vol, paths=256)
    cam = Pipeline(engine, _settings(), W, H, pixel_cost="ncc").cam
    for bad in (0, 256):
        with pytest.raises(ValueError):
            PixelSweep(engine, cam, W, H, "ncc", 5, sgm=True, sgm_paths=bad)
        with pytest.raises(ValueError):
            Pipeline(engine, _settings(), W, H, pixel_cost="ncc", sgm=True, sgm_paths=bad)
    engine.synchronize()
