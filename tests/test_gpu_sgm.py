"""The semi-global aggregation kernels (csrc/sgm.hip, mvs_sgm_d) against the
definition in tests/sgm_ref.py, bit for bit.

Random volumes walk the level counts on and around every boundary of the two
kernel forms (a lane's and a wave's level chunk, one and several levels per
lane, the columns form's 256-level limit, several waves per line) at two image
sizes, one of them with a 16-byte tail and a plane pitch that is no multiple of
four floats; every path mask and every penalty pair meets every level count.
Before the GPU is compared, the reference's four single-path volumes are shown
to differ pairwise on at least a quarter of the cells, so a kernel that walks
the wrong way or the wrong axis cannot pass.  That holds for every penalty pair
with P2 > 0 and is asserted for those; with P1 = P2 = 0 every path is
(vol + m) - m, the cost itself up to one rounding, on any path (the reference
gives 0.00 .. 0.24 there), so nothing can be asserted for that pair; every level
count meets it on masks that the other pairs cover on the same shape.

Natural volumes (orc.ncc_volume on a synthetic stack), `out=` reuse, the
pipeline's `sgm=True` and the argument errors follow."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd import _lib, params, synth
from cl_multiview_stereo_amd.pipeline import Pipeline, PixelSweep
from oracle import oracle as orc
from tests import sgm_ref as sg

pytestmark = pytest.mark.gpu

MASKS = [1, 2, 4, 8, 3, 12, 15]
PEN = [(0.1, 0.8), (0.0, 0.0), (0.25, 0.25), (0.5, 4.0)]
DS = [1, 2, 3, 63, 64, 65, 128, 130, 257]
SHAPES = ([(D, 6, 70) for D in DS] + [(D, 5, 67) for D in DS]
          # the smallest shapes with a level-chunk edge, a wave edge, a one-pixel path or a tail in play
          + [(3, 4, 1), (2, 1, 7), (65, 1, 1), (40, 130, 3)]
          # sixteen levels per lane; two waves per line (the LDS exchange of the lanes form)
          + [(600, 3, 9), (1100, 3, 5)])


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.count_nonzero(a != b)
    assert bad == 0, f"{what}: {bad}/{a.size} differ, first at {np.argwhere(a != b)[:3].tolist()}"


def not_vacuous(vol, P1, P2, what, least=0.25):
    """The reference's four single-path volumes differ pairwise (see the module's text)."""
    L = [sg.single(vol, b, P1, P2) for b in range(4)]
    share = min(float((L[i] != L[j]).mean()) for i in range(4) for j in range(i))
    if P2 > 0:
        assert share >= least, (what, share)
    return share


# ---- 1. random volumes -------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_volumes(engine, shape):
    """Every mask on every shape; the penalty pair rotates with the mask and the
    shape, so that the two (or more) shapes of a level count meet all four."""
    D, H, W = shape
    k = SHAPES.index(shape)
    vol = sg.random_volume(D, H, W, seed=100 + k)
    assert (vol == 2).any() or vol.size < 32
    if D >= 3 and H >= 3 and W >= 3:
        for P1, P2 in PEN:
            not_vacuous(vol, P1, P2, (shape, P1, P2))
    gv = torch.from_numpy(vol).cuda()
    out = engine.empty(shape, torch.float32)
    for i, mask in enumerate(MASKS):
        P1, P2 = PEN[(i + k) % 4] if H * W > 1 else PEN[i % 4]
        want = sg.sgm(vol, P1, P2, mask)
        out.fill_(float("nan"))  # stale contents must not show
        got = engine.sgm(gv, P1, P2, mask, out=out)
        assert got.data_ptr() == out.data_ptr()
        same(got, want, f"D{D} H{H} W{W} paths={mask} P1={P1} P2={P2}")
    same(gv, vol, "the volume is left as it was")


def test_every_mask_and_penalty_meets_every_level_count():
    """The pruning of the product above, checked: per level count the runs cover all masks and all pairs."""
    seen = {}
    for k, (D, H, W) in enumerate(SHAPES):
        for i, mask in enumerate(MASKS):
            seen.setdefault(D, set()).add((mask, PEN[(i + k) % 4] if H * W > 1 else PEN[i % 4]))
    for D in DS:
        assert {m for m, _ in seen[D]} == set(MASKS) and {p for _, p in seen[D]} == set(PEN), D


@pytest.mark.parametrize("paths", [3, 15])
def test_unaligned_bases(engine, paths):
    """vol and agg one float past a 16-byte boundary (every piece's phase moves),
    and the two on different boundaries (no 16-byte pieces at all)."""
    D, H, W = 66, 5, 67
    vol = sg.random_volume(D, H, W, seed=7)
    want = sg.sgm(vol, 0.1, 0.8, paths)
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


# ---- 2. natural volumes --------------------------------------------------------------
AW, NW_, NH_ = 5, 300, 40


@pytest.fixture(scope="module")
def natural():
    """The stack, its oracle volumes and reference aggregates over levels 0..31, all five views."""
    stack, _ = synth.make_stack(NW_, NH_, AW, 1, 4, 27, 1.0, 0x5EED + 13)
    l8 = orc.l8(orc.cvt(stack))
    vs, sn = params.flatten_subsets(params.neighbour_lists(AW, 1, 1, 0))
    levels = params.disparity_levels(0, 31, 1)
    vols = [orc.ncc_volume(l8, levels, vs, sn, AW, 1.0, 5, z) for z in range(AW)]
    aggs = [sg.sgm(v, 0.1, 0.8, 15) for v in vols]
    raw = [orc.wta(v, levels) for v in vols]
    win = [orc.wta(a, levels) for a in aggs]
    return stack, l8, vols, aggs, raw, win


def _moved(raw, win, what):
    """Asserted first: the aggregation changes the winner on at least 0.15 of the pixels of every view."""
    share = [float((r[0] != w[0]).mean()) for r, w in zip(raw, win)]
    print(f"{what}: the aggregated winner differs from the raw one on {['%.3f' % s for s in share]} of the pixels")
    assert min(share) >= 0.15, (what, share)


@pytest.mark.parametrize("dmax", [31, 127])
def test_natural_volumes(engine, natural, dmax):
    stack, l8h, vols, aggs, raw, win = natural
    st = params.Settings(spixl_size=8, array_width=AW, array_height=1, neib_hor=1, neib_ver=0, min_disp=0,
                         max_disp=dmax, inc=1, bl_ratio=1.0, window=5)
    cam = Pipeline(engine, st, NW_, NH_, pixel_cost="ncc").cam
    levels = cam.levels
    if dmax != 31:
        vols = [orc.ncc_volume(l8h, levels, cam.view_subset, cam.subset_num, AW, 1.0, 5, z) for z in range(AW)]
        aggs = [sg.sgm(v, 0.1, 0.8, 15) for v in vols]
        raw = [orc.wta(v, levels) for v in vols]
        win = [orc.wta(a, levels) for a in aggs]
    _moved(raw, win, f"levels 0..{dmax}")
    for z in (0, 2):
        share = not_vacuous(vols[z], 0.1, 0.8, ("natural", dmax, z), least=0.34)
        print(f"levels 0..{dmax} view {z}: the four paths differ pairwise on at least {share:.3f} of the cells")
    _, l8 = engine.cvt(torch.from_numpy(stack).cuda())
    same(l8, l8h, "l8")
    box = engine.box_stats(l8, 5)
    lev = engine.levels_dev(cam)
    for z in range(AW):
        gv = engine.ncc_volume(l8, box, cam, z, 5)
        same(gv, vols[z], f"volume z{z}")
        ga = engine.sgm(gv)
        same(ga, aggs[z], f"aggregate z{z} levels 0..{dmax}")
        d, c = engine.wta(ga, lev)
        same(d, win[z][0], f"aggregated disp z{z} levels 0..{dmax}")
        same(c, win[z][1], f"aggregated conf z{z} levels 0..{dmax}")


# ---- 3. out= reuse ---------------------------------------------------------------------
def test_out_reuse_across_two_volumes(engine):
    """The first path stores, it does not add: nothing of the first aggregate shows in the second."""
    D, H, W = 33, 7, 45
    a, b = sg.random_volume(D, H, W, seed=11), sg.random_volume(D, H, W, seed=12)
    out = engine.empty((D, H, W), torch.float32)
    for paths in (15, 8, 6):
        same(engine.sgm(torch.from_numpy(a).cuda(), paths=paths, out=out), sg.sgm(a, paths=paths), f"first, paths={paths}")
        same(engine.sgm(torch.from_numpy(b).cuda(), paths=paths, out=out), sg.sgm(b, paths=paths), f"second, paths={paths}")


# ---- 4. pipeline -----------------------------------------------------------------------
def _settings():
    return params.Settings(spixl_size=8, array_width=AW, array_height=1, neib_hor=1, neib_ver=0, min_disp=0,
                           max_disp=31, inc=1, bl_ratio=1.0, window=5)


@pytest.mark.parametrize("fused", [True, False])
def test_pipeline(engine, natural, fused):
    stack, _, vols, aggs, raw, win = natural
    _moved(raw, win, "pipeline")
    rgbx = torch.from_numpy(stack).cuda()
    on = Pipeline(engine, _settings(), NW_, NH_, pixel_cost="ncc", fused=fused, sgm=True).exe_pipeline(rgbx)
    off = Pipeline(engine, _settings(), NW_, NH_, pixel_cost="ncc", fused=fused).exe_pipeline(rgbx)
    assert off.disp_agg is None and off.conf_agg is None
    assert tuple(on.disp_agg.shape) == tuple(on.conf_agg.shape) == tuple(on.disp.shape) == (AW, NH_, NW_)
    same(on.disp, off.disp, f"disp with and without sgm, fused {fused}")
    same(on.conf, off.conf, f"conf with and without sgm, fused {fused}")
    for z in range(AW):
        same(on.disp[z], raw[z][0], f"pipeline disp z{z} fused {fused}")
        same(on.conf[z], raw[z][1], f"pipeline conf z{z} fused {fused}")
        same(on.disp_agg[z], win[z][0], f"pipeline disp_agg z{z} fused {fused}")
        same(on.conf_agg[z], win[z][1], f"pipeline conf_agg z{z} fused {fused}")
    # with the sub-level fit: it stays on the raw volume
    both = Pipeline(engine, _settings(), NW_, NH_, pixel_cost="ncc", fused=fused, sgm=True, subpixel=True).exe_pipeline(rgbx)
    sub = Pipeline(engine, _settings(), NW_, NH_, pixel_cost="ncc", fused=fused, subpixel=True).exe_pipeline(rgbx)
    same(both.disp_sub, sub.disp_sub, f"disp_sub with and without sgm, fused {fused}")
    same(both.disp_agg, on.disp_agg, f"disp_agg with and without subpixel, fused {fused}")


@pytest.mark.parametrize("fused", [True, False])
def test_pixel_sweep_view_shard(engine, natural, fused):
    """Reference views [1, 4), planes built for the block and its neighbours only; other penalties."""
    stack, _, vols, aggs, raw, win = natural
    lab, l8 = engine.cvt(torch.from_numpy(stack).cuda())
    cam = Pipeline(engine, _settings(), NW_, NH_, pixel_cost="ncc").cam
    ps = PixelSweep(engine, cam, NW_, NH_, "ncc", 5, fused=fused, sgm=True, sgm_p1=0.25, sgm_p2=1.5)
    disp, conf = ps.run(lab, l8, 1, 4, views=cam.views_needed(1, 4))
    assert tuple(ps.disp_agg.shape) == tuple(ps.conf_agg.shape) == (3, NH_, NW_)
    for i, z in enumerate(range(1, 4)):
        wd, wc = orc.wta(sg.sgm(vols[z], 0.25, 1.5, 15), cam.levels)
        assert (wd != win[z][0]).any()  # the penalties reach the kernel
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
    v, a = C.c_void_p(vol.data_ptr()), C.c_void_p(agg.data_ptr())

    def rc(ctx=ctx, W=W, H=H, D=D, v=v, P1=0.1, P2=0.8, paths=15, a=a):
        r = L.mvs_sgm_d(ctx, W, H, D, v, C.c_float(P1), C.c_float(P2), paths, a)
        if r != 0:
            assert b"mvs_sgm_d" in L.mvs_last_error() or b"sgm" in L.mvs_last_error()
        return r

    assert rc() == 0
    assert rc(ctx=None) == -1 and rc(v=None) == -1 and rc(a=None) == -1
    assert rc(W=0) == -1 and rc(H=0) == -1 and rc(W=-3) == -1 and rc(W=1 << 20, H=1 << 20) == -1
    assert rc(D=0) == -1 and rc(D=-1) == -1 and rc(D=16385) == -1
    for paths in (0, 16, -1, 31):
        assert rc(paths=paths) == -1, paths
    inf, nan = float("inf"), float("nan")
    for P1, P2 in ((-0.1, 0.8), (0.1, -0.8), (0.9, 0.8), (nan, 0.8), (0.1, nan), (0.1, inf), (inf, inf), (-inf, 0.8)):
        assert rc(P1=P1, P2=P2) == -1, (P1, P2)
    assert rc(a=v) == -1
    assert rc(P1=0.0, P2=0.0) == 0 and rc(P1=0.5, P2=0.5) == 0 and rc(paths=1) == 0
    with pytest.raises(_lib.MvsError, match="agg must not be vol"):
        engine.sgm(vol, out=vol)
    with pytest.raises(ValueError):
        engine.sgm(vol, out=engine.empty((D, H, W + 1), torch.float32))
    with pytest.raises(ValueError):
        engine.sgm(vol.transpose(1, 2))
    with pytest.raises(ValueError):
        engine.sgm(vol.double())
    cam = Pipeline(engine, _settings(), W, H, pixel_cost="ncc").cam
    with pytest.raises(ValueError):
        PixelSweep(engine, cam, W, H, "sad", 5, sgm=True)
    with pytest.raises(ValueError):
        Pipeline(engine, _settings(), W, H, pixel_cost="sad", sgm=True)
    engine.synchronize()
