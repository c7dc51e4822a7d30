"""Several volumes per call (csrc/sgm.hip through mvs_sgm8_batch_d): element i of
the batch holds, bit for bit, what tests/sgm8_ref.sgm8 gives for volume i.

1. Random volumes on the smallest shapes that reach every kernel form and
   boundary (the table at SHAPES), batches of 1, 2, 3 and 5, the masks of M13
   and the penalty pairs of test_gpu_sgm8.py, both rotating so that every level
   count meets horizontal, vertical and diagonal masks with every batch size.
   Before the GPU is compared, the elements' reference aggregates are shown to
   differ pairwise on at least 0.9 of their cells (shapes with D, H, W >= 3), so
   a kernel that reads or writes the wrong element cannot pass.
2. Strides above D H W (multiples of 4 floats and not, equal for vol and agg and
   not: the last two pairs force the 4-byte form) with bases 0, 1 and 3 floats
   past a 16-byte boundary: the gaps and the tail of agg keep their NaN pattern,
   the vol buffer is unchanged.
3. N = 1 is mvs_sgm8_d.  4. N = 65535 on one-cell volumes, and 65536 refused.
5. Natural volumes (orc.ncc_volume on a synthetic stack), five views in one
   call.  6. The pipeline's `sgm_batch`.  7. The argument errors."""
from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd import _lib, params, synth
from cl_multiview_stereo_amd.pipeline import Pipeline, PixelSweep
from oracle import oracle as orc
from tests import sgm8_ref as s8
from tests import sgm_ref as sg
from tests import test_gpu_sgm8 as t8

pytestmark = pytest.mark.gpu

same, bits, Singles, PEN = t8.same, t8.bits, t8.Singles, t8.PEN
M13 = [255, 15, 240, 5, 0x50, 1, 2, 4, 8, 16, 32, 64, 128]
NS = [1, 2, 3, 5]
# (D, H, W), the smallest that reach each form and boundary:
SHAPES = [
    (17, 6, 70),    # two waves, two workgroups in the columns and sheared forms
    (64, 5, 67), (65, 5, 67),    # levels per lane 1 -> 2
    (130, 6, 70),   # nine waves: the 1,024-thread instantiations; 4 levels per lane
    (256, 2, 64), (257, 2, 64),  # last of the columns / sheared forms, first of the lanes form with 8 levels per lane
    (1100, 3, 5),   # several waves per line of the lanes form
    (16, 130, 3),   # H >> W, clipped row ranges
    (5, 1, 7), (3, 4, 1),        # one-pixel lines
]
NAN = np.float32("nan")


def n_of(i, k):
    """The batch size of mask i on shape k: it rotates with both (the i // 4 so that the vertical masks, which sit
    at i = 0, 1, 3, 7, 8, meet all four)."""
    return NS[(i + i // 4 + k) % 4]


def kinds(mask):
    return {k for k, m in (("horizontal", 3), ("vertical", 12), ("diagonal", 240)) if mask & m}


# ---- 1. random volumes -------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_volumes(engine, shape):
    D, H, W = shape
    k = SHAPES.index(shape)
    vols = [sg.random_volume(D, H, W, seed=500 + 17 * k + i) for i in range(max(NS))]
    refs = [Singles(v) for v in vols]
    gv = torch.from_numpy(np.stack(vols)).cuda()
    out = engine.empty((max(NS),) + shape, torch.float32)
    for i, mask in enumerate(M13):
        P1, P2 = t8.pen_of(i, k, H, W)
        N = n_of(i, k)
        want = [r.agg(P1, P2, mask) for r in refs[:N]]
        if D >= 3 and H >= 3 and W >= 3:  # on the reference alone: no two elements could be mistaken for each other
            share = min([float((want[a] != want[b]).mean()) for a in range(N) for b in range(a)], default=1.0)
            assert share >= 0.9, (shape, mask, P1, P2, share)
        out.fill_(float("nan"))  # stale contents must not show
        got = engine.sgm_batch(gv[:N], P1, P2, mask, out=out[:N])
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (N,) + shape
        for j in range(N):
            same(got[j], want[j], f"D{D} H{H} W{W} N={N} element {j} paths={mask} P1={P1} P2={P2}")
        assert (bits(out[N:]) == bits(NAN)).all(), "a store behind the last element"
    same(gv, np.stack(vols), "the volumes are left as they were")


def test_every_level_count_meets_every_mask_class_and_batch_size():
    for k, (D, H, W) in enumerate(SHAPES):
        seen, pens = set(), set()
        for i, mask in enumerate(M13):
            seen |= {(kind, n_of(i, k)) for kind in kinds(mask)}
            pens.add(t8.pen_of(i, k, H, W))
        assert seen == set(itertools.product(("horizontal", "vertical", "diagonal"), NS)), (D, seen)
        assert pens == set(PEN), D
    assert len({D for D, _, _ in SHAPES}) == len(SHAPES)  # one shape per level count: the above is per D


# ---- 2. strides and phases -----------------------------------------------------------
SD, SH, SW = 66, 5, 67
SN = SD * SH * SW


@pytest.fixture(scope="module")
def three():
    """Three volumes of (66, 5, 67) and their aggregates for paths 15 and 255."""
    vols = [sg.random_volume(SD, SH, SW, seed=700 + i) for i in range(3)]
    return vols, {p: [s8.sgm8(v, 0.1, 0.8, p) for v in vols] for p in (15, 255)}


@pytest.mark.parametrize("paths", [15, 255])
def test_strides_and_phases(engine, three, paths):
    vols, aggs = three
    N = 3
    hv = torch.from_numpy(np.stack(vols)).cuda()
    for (dv, da), ov, oa in itertools.product(((0, 0), (1, 1), (3, 3), (4, 0), (1, 2), (0, 3)), (0, 1, 3), (0, 1, 3)):
        sv, sa = SN + dv, SN + da
        bv = engine.empty((ov + (N - 1) * sv + SN + 4,), torch.float32).fill_(7.0)
        ba = engine.empty((oa + (N - 1) * sa + SN + 4,), torch.float32).fill_(float("nan"))
        gv = bv.as_strided((N, SD, SH, SW), (sv, SH * SW, SW, 1), ov)
        ga = ba.as_strided((N, SD, SH, SW), (sa, SH * SW, SW, 1), oa)
        gv.copy_(hv)
        before = bv.clone()
        assert gv.data_ptr() % 16 == 4 * ov and ga.data_ptr() % 16 == 4 * oa
        what = f"strides D H W + {dv}, {da}, offsets {ov}, {oa} floats, paths={paths}"
        got = engine.sgm_batch(gv, 0.1, 0.8, paths, out=ga)
        assert got.data_ptr() == ga.data_ptr()
        flat = bits(ba)
        inside = np.zeros(flat.shape, bool)
        for j in range(N):
            lo = oa + j * sa
            same(flat[lo:lo + SN].reshape(SD, SH, SW), aggs[paths][j], f"element {j}, {what}")
            inside[lo:lo + SN] = True
        assert (flat[~inside] == bits(NAN)).all(), f"a store outside agg: {what}"
        same(bv, before, f"the vol buffer, {what}")


# ---- 3. one element is mvs_sgm8_d ----------------------------------------------------
def test_one_element_is_mvs_sgm8_d(engine):
    D, H, W = SD, SH, SW
    vol = torch.from_numpy(sg.random_volume(D, H, W, seed=8)).cuda()
    a1, ab = engine.empty((D, H, W), torch.float32), engine.empty((1, D, H, W), torch.float32)
    for paths in list(range(1, 16)) + t8.MASKS:
        a1.fill_(float("nan"))
        ab.fill_(float("nan"))
        _lib.check(engine.L.mvs_sgm8_d(engine.ctx, W, H, D, vol.data_ptr(), 0.1, 0.8, paths, a1.data_ptr()), "mvs_sgm8_d")
        engine.sgm_batch(vol[None], 0.1, 0.8, paths, out=ab)
        same(ab[0], a1, f"paths={paths}")


# ---- 4. the grid axis ------------------------------------------------------------------
def test_grid_axis_limit(engine):
    """65535 one-cell volumes: every path's L is the cost, the aggregate the sum of the copies in order."""
    N = 65535
    h = (np.arange(N + 1, dtype=np.float32) / np.float32(65536)).astype(np.float32)
    vol = torch.from_numpy(h).cuda()
    agg = engine.empty((N + 1,), torch.float32)
    want8 = h.copy()
    for _ in range(7):
        want8 = want8 + h
    for paths, want in ((255, want8), (1, h)):
        agg.fill_(float("nan"))
        engine.sgm_batch(vol[:N].view(N, 1, 1, 1), 0.1, 0.8, paths, out=agg[:N].view(N, 1, 1, 1))
        same(agg[:N], want[:N], f"paths={paths}")
        assert bits(agg[N:]) == bits(NAN)
    L = engine.L
    assert L.mvs_sgm8_batch_d(engine.ctx, 1, 1, 1, N + 1, vol.data_ptr(), 1, 0.1, 0.8, 255, agg.data_ptr(), 1) == -1
    assert b"mvs_sgm8_batch_d: N must be in 1..65535" in L.mvs_last_error()
    engine.synchronize()


# ---- 5. natural volumes ----------------------------------------------------------------
AW, NW_, NH_ = t8.AW, t8.NW_, t8.NH_


@pytest.fixture(scope="module")
def natural():
    """test_gpu_sgm8.py's stack; per level set (0..31, 0..127) the oracle volumes of the five views, their eight-path
    aggregates and winners, the raw winners and the four-path winners."""
    stack, _ = synth.make_stack(NW_, NH_, AW, 1, 4, 27, 1.0, 0x5EED + 13)
    l8 = orc.l8(orc.cvt(stack))
    vs, sn = params.flatten_subsets(params.neighbour_lists(AW, 1, 1, 0))
    out = {}
    for dmax in (31, 127):
        levels = params.disparity_levels(0, dmax, 1)
        vols = [orc.ncc_volume(l8, levels, vs, sn, AW, 1.0, 5, z) for z in range(AW)]
        agg8 = [s8.sgm8(v, 0.1, 0.8, 255) for v in vols]
        out[dmax] = dict(vols=vols, agg8=agg8, raw=[orc.wta(v, levels) for v in vols],
                         win4=[orc.wta(sg.sgm(v, 0.1, 0.8, 15), levels) for v in vols],
                         win8=[orc.wta(a, levels) for a in agg8])
    return stack, out


@pytest.mark.parametrize("dmax", [31, 127])
def test_natural_volumes(engine, natural, dmax):
    stack, refs = natural
    r = refs[dmax]
    t8._moved(r["win4"], r["win8"], f"levels 0..{dmax}")
    cam = Pipeline(engine, t8._settings(dmax), NW_, NH_, pixel_cost="ncc").cam
    _, l8 = engine.cvt(torch.from_numpy(stack).cuda())
    box = engine.box_stats(l8, 5)
    lev = engine.levels_dev(cam)
    gv = engine.empty((AW, dmax + 1, NH_, NW_), torch.float32)
    for z in range(AW):
        engine.ncc_volume(l8, box, cam, z, 5, out=gv[z])
        same(gv[z], r["vols"][z], f"volume z{z}")
    ga = engine.sgm_batch(gv, paths=255)
    for z in range(AW):
        same(ga[z], r["agg8"][z], f"aggregate z{z} levels 0..{dmax}")
        d, c = engine.wta(ga[z], lev)
        same(d, r["win8"][z][0], f"aggregated disp z{z} levels 0..{dmax}")
        same(c, r["win8"][z][1], f"aggregated conf z{z} levels 0..{dmax}")


# ---- 6. pipeline -----------------------------------------------------------------------
@pytest.mark.parametrize("fused", [True, False])
def test_pipeline(engine, natural, fused):
    stack, refs = natural
    r = refs[31]
    t8._moved(r["win4"], r["win8"], "pipeline")
    rgbx = torch.from_numpy(stack).cuda()

    def run(B):
        return Pipeline(engine, t8._settings(), NW_, NH_, pixel_cost="ncc", fused=fused, subpixel=True, sgm=True,
                        sgm_paths=255, sgm_batch=B).exe_pipeline(rgbx)

    one = run(1)
    for B in (2, 5, 7):  # 7: more than the five views
        on = run(B)
        assert tuple(on.disp_agg.shape) == tuple(on.conf_agg.shape) == tuple(on.disp.shape) == (AW, NH_, NW_)
        for z in range(AW):
            what = f"z{z} fused {fused} sgm_batch {B}"
            same(on.disp[z], r["raw"][z][0], f"pipeline disp {what}")
            same(on.conf[z], r["raw"][z][1], f"pipeline conf {what}")
            same(on.disp_agg[z], r["win8"][z][0], f"pipeline disp_agg {what}")
            same(on.conf_agg[z], r["win8"][z][1], f"pipeline conf_agg {what}")
        for name in ("disp", "conf", "disp_sub", "disp_agg", "conf_agg"):
            same(getattr(on, name), getattr(one, name), f"{name}, sgm_batch {B} against 1, fused {fused}")


def test_pipeline_buffers(engine):
    """[min(B, V), D, H, W] with B > 1; with 1 (and without sgm) the buffers of before."""
    def ps(**kw):
        return Pipeline(engine, t8._settings(), NW_, NH_, pixel_cost="ncc", **kw).pixel

    D = 32
    for B, n in ((2, 2), (5, 5), (7, 5)):
        p = ps(sgm=True, sgm_batch=B, fused=True)
        assert tuple(p.vol.shape) == tuple(p.agg.shape) == (n, D, NH_, NW_)
    p = ps(sgm=True, fused=True)
    assert tuple(p.vol.shape) == tuple(p.agg.shape) == (D, NH_, NW_)
    p = ps(sgm_batch=5)  # no aggregation: the option allocates nothing
    assert tuple(p.vol.shape) == (D, NH_, NW_) and p.agg is None
    assert ps(sgm_batch=5, fused=True).vol is None


@pytest.mark.parametrize("fused", [True, False])
def test_pixel_sweep_view_shard(engine, natural, fused):
    """Reference views [1, 4) in groups of 2 + 1, the four diagonal paths alone."""
    stack, refs = natural
    r = refs[31]
    lab, l8 = engine.cvt(torch.from_numpy(stack).cuda())
    cam = Pipeline(engine, t8._settings(), NW_, NH_, pixel_cost="ncc").cam
    ps = PixelSweep(engine, cam, NW_, NH_, "ncc", 5, fused=fused, sgm=True, sgm_paths=240, sgm_batch=2)
    disp, conf = ps.run(lab, l8, 1, 4, views=cam.views_needed(1, 4))
    assert tuple(ps.disp_agg.shape) == tuple(ps.conf_agg.shape) == (3, NH_, NW_)
    for i, z in enumerate(range(1, 4)):
        wd, wc = orc.wta(s8.sgm8(r["vols"][z], 0.1, 0.8, 240), cam.levels)
        assert (wd != r["win8"][z][0]).any()  # the mask reaches the kernel
        same(disp[i], r["raw"][z][0], f"shard disp z{z}")
        same(conf[i], r["raw"][z][1], f"shard conf z{z}")
        same(ps.disp_agg[i], wd, f"shard disp_agg z{z}")
        same(ps.conf_agg[i], wc, f"shard conf_agg z{z}")


# ---- 7. errors -------------------------------------------------------------------------
def test_errors(engine):
    D, H, W = 4, 3, 5
    n = D * H * W
    buf = engine.empty((8 * n,), torch.float32).fill_(0.5)
    L, ctx = engine.L, engine.ctx
    v, a = buf.data_ptr(), buf.data_ptr() + 4 * 4 * n  # two spans of up to four tight elements

    def rc(ctx=ctx, W=W, H=H, D=D, N=2, v=v, vs=n, P1=0.1, P2=0.8, paths=255, a=a, as_=n):
        r = L.mvs_sgm8_batch_d(ctx, W, H, D, N, v, vs, P1, P2, paths, a, as_)
        if r != 0:
            assert b"mvs_sgm8_batch_d" in L.mvs_last_error()
        return r

    assert rc() == 0
    assert rc(ctx=None) == -1 and rc(v=None) == -1 and rc(a=None) == -1
    for N in (0, -1, 65536):
        assert rc(N=N) == -1, N
        assert b"mvs_sgm8_batch_d: N must be in 1..65535" in L.mvs_last_error()
    assert rc(vs=n - 1) == -1 and rc(as_=n - 1) == -1
    assert b"stride" in L.mvs_last_error()
    # overlapping spans: agg inside vol's span (and its gap), agg = vol + D H W with two tight elements, agg = vol
    assert rc(N=2, vs=3 * n, a=v + 4 * n) == -1 and b"overlap" in L.mvs_last_error()
    assert rc(N=2, a=v + 4 * n) == -1 and b"overlap" in L.mvs_last_error()
    assert rc(a=v) == -1 and rc(N=1, a=v) == -1 and rc(N=2, a=v + 4 * (2 * n - 1)) == -1
    # abutting spans are accepted, either way round
    assert rc(N=2, a=v + 4 * 2 * n) == 0 and rc(N=2, v=v + 4 * 2 * n, a=v) == 0 and rc(N=4) == 0
    assert rc(N=1, a=v + 4 * n) == 0
    # everything mvs_sgm8_d refuses
    assert rc(W=0) == -1 and rc(H=0) == -1 and rc(W=-3) == -1 and rc(W=1 << 20, H=1 << 20) == -1
    assert rc(D=0) == -1 and rc(D=-1) == -1 and rc(D=16385) == -1
    for paths in (0, 256, -1):
        assert rc(paths=paths) == -1, paths
        assert b"mvs_sgm8_batch_d: paths must be a mask in 1..255" in L.mvs_last_error()
    inf, nan = float("inf"), float("nan")
    for P1, P2 in ((-0.1, 0.8), (0.1, -0.8), (0.9, 0.8), (nan, 0.8), (0.1, nan), (0.1, inf), (inf, inf), (-inf, 0.8)):
        assert rc(P1=P1, P2=P2) == -1, (P1, P2)
    assert rc(P1=0.0, P2=0.0) == 0 and rc(P1=0.5, P2=0.5) == 0 and rc(paths=16) == 0 and rc(paths=1) == 0
    # the Python layer
    vols = buf[:2 * n].view(2, D, H, W)
    with pytest.raises(ValueError):
        engine.sgm_batch(vols[0])  # three dimensions
    with pytest.raises(ValueError):
        engine.sgm_batch(vols.double())
    with pytest.raises(ValueError):
        engine.sgm_batch(vols, out=engine.empty((2, D, H, W), torch.float64))
    with pytest.raises(ValueError):
        engine.sgm_batch(vols, out=engine.empty((3, D, H, W), torch.float32))
    with pytest.raises(ValueError):
        engine.sgm_batch(buf[:2 * 2 * n].view(2, D, H, 2 * W)[..., :W])  # elements that are not contiguous
    with pytest.raises(_lib.MvsError, match="mvs_sgm8_batch_d: the vol and agg spans overlap"):
        engine.sgm_batch(vols, out=vols)
    with pytest.raises(_lib.MvsError, match="mvs_sgm8_batch_d: paths must be a mask in 1..255"):
        engine.sgm_batch(vols, paths=256)
    cam = Pipeline(engine, t8._settings(), W, H, pixel_cost="ncc").cam
    for bad in (0, -2):
        with pytest.raises(ValueError):
            PixelSweep(engine, cam, W, H, "ncc", 5, sgm=True, sgm_batch=bad)
        with pytest.raises(ValueError):
            Pipeline(engine, t8._settings(), W, H, pixel_cost="ncc", sgm=True, sgm_batch=bad)
    engine.synchronize()
