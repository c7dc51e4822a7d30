"""Semi-global aggregation on 16-bit integer costs (csrc/sgm16.hip through
mvs_quant_u16_d, mvs_sgm8_u16_batch_d and mvs_wta_u16_d) against the definition
in tests/sgm16_ref.py, bit for bit.

1. Random volumes (integer costs 0..4094, one cell in sixteen exactly 4094) on
   the smallest shapes that reach every kernel form and boundary (the table at
   SHAPES), the thirteen masks of test_gpu_sgm_batch.M13, batches of 1, 2, 3
   and 5 and four penalty pairs, all rotating so that every level count meets
   horizontal, vertical and diagonal masks with every batch size.  Before the
   GPU is compared, the elements' reference aggregates are shown to differ
   pairwise on at least 0.9 of their cells (shapes with D, H, W >= 3).  agg is
   pre-filled with 0xA5A5: nothing behind the last element changes, and vol is
   unchanged.
2. The extreme case: every cost 4094 (and a volume that alternates 0 and 4094),
   P1 = P2 = 4095, all eight paths: nothing wraps.
3. Strides and phases on (66, 5, 67), N = 3: bases 0, 1, 3 and 7 elements past a
   16-byte boundary, stride surpluses (0,0), (1,1), (8,8), (8,0) and (1,2), the
   last forcing the 2-byte form; gaps and tail keep the sentinel.
4. quant_u16.  5. wta_u16.  6. The pipeline's `sgm_dtype="u16"`.  7. The
   argument errors.

The tensors are torch.uint16; sentinels are written and results read through
int16 views of the same bits."""
from __future__ import annotations

import itertools

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd import _lib, params, synth
from cl_multiview_stereo_amd.pipeline import Pipeline, PixelSweep
from oracle import oracle as orc
from tests import sgm16_ref as s16
from tests.test_gpu_sgm_batch import M13, NS, kinds, n_of

pytestmark = pytest.mark.gpu

PEN = [(205, 1638), (0, 0), (512, 512), (1024, 4095)]
# (D, H, W), the smallest that reach each form and boundary:
SHAPES = [
    (17, 6, 70),    # two waves, two workgroups in the columns and sheared forms
    (64, 5, 67), (65, 5, 67),    # levels per lane 1 -> 2
    (130, 6, 70),   # nine waves: the 1,024-thread instantiations; 4 levels per lane
    (256, 2, 64),   # the last level count
    (16, 130, 3),   # H >> W, clipped row ranges
    (5, 1, 7), (3, 4, 1),        # one-pixel lines
    (33, 3, 23),    # a plane pitch of 69 elements: eight consecutive levels take all eight piece phases
]
SENT = 0xA5A5
SENT_I16 = SENT - 65536


def dev(a):
    """A uint16 numpy array on the GPU, as torch.uint16."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.uint16
    return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)


def host(t):
    """A uint16 (or int16-viewed) tensor as a uint16 numpy array."""
    t = t.view(torch.int16) if t.dtype == torch.uint16 else t
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint16)


def fill(t, value=SENT_I16):
    t.view(torch.int16).fill_(value)
    return t


def same(got, want, what):
    got = host(got) if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.count_nonzero(got != want)
    assert bad == 0, f"{what}: {bad}/{got.size} differ, first at {np.argwhere(got != want)[:3].tolist()}"


def same_f(got, want, what):
    got, want = got.cpu().numpy().view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.count_nonzero(got != want)
    assert bad == 0, f"{what}: {bad}/{got.size} differ, first at {np.argwhere(got != want)[:3].tolist()}"


def pen_of(i, k, H, W):
    """The penalty pair of mask i on shape k: it rotates with both."""
    return PEN[(i + k) % 4] if H * W > 1 else PEN[i % 4]


class Singles:
    """The reference's eight single-path volumes of one volume, per penalty pair, computed once."""

    def __init__(self, vol):
        self.vol, self.L = vol, {}

    def agg(self, p1, p2, mask):
        if (p1, p2) not in self.L:
            self.L[(p1, p2)] = [s16.single(self.vol, b, p1, p2) for b in range(8)]
        return s16.sum_paths([L for b, L in enumerate(self.L[(p1, p2)]) if mask >> b & 1])


# ---- 1. random volumes -------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_random_volumes(engine, shape):
    D, H, W = shape
    k = SHAPES.index(shape)
    vols = [s16.random_volume(D, H, W, seed=1600 + 17 * k + i) for i in range(max(NS))]
    refs = [Singles(v) for v in vols]
    gv = dev(np.stack(vols))
    out = engine.empty((max(NS),) + shape, torch.uint16)
    for i, mask in enumerate(M13):
        p1, p2 = pen_of(i, k, H, W)
        N = n_of(i, k)
        want = [r.agg(p1, p2, mask) for r in refs[:N]]
        if D >= 3 and H >= 3 and W >= 3:  # on the reference alone: no two elements could be mistaken for each other
            share = min([float((want[a] != want[b]).mean()) for a in range(N) for b in range(a)], default=1.0)
            assert share >= 0.9, (shape, mask, p1, p2, share)
        fill(out)  # stale contents must not show
        got = engine.sgm_u16_batch(gv[:N], p1, p2, mask, out=out[:N])
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (N,) + shape
        for j in range(N):
            same(got[j], want[j], f"D{D} H{H} W{W} N={N} element {j} paths={mask} P1={p1} P2={p2}")
        assert (host(out[N:]) == SENT).all(), "a store behind the last element"
    same(gv, np.stack(vols), "the volumes are left as they were")
    # without out=: a uint16 tensor of the batch's shape
    got = engine.sgm_u16_batch(gv[:2], 205, 1638, 255)
    assert got.dtype == torch.uint16 and tuple(got.shape) == (2,) + shape
    same(got[1], refs[1].agg(205, 1638, 255), "out=None")


def test_every_level_count_meets_every_mask_class_and_batch_size():
    for k, (D, H, W) in enumerate(SHAPES):
        seen, pens = set(), set()
        for i, mask in enumerate(M13):
            seen |= {(kind, n_of(i, k)) for kind in kinds(mask)}
            pens.add(pen_of(i, k, H, W))
        assert seen == set(itertools.product(("horizontal", "vertical", "diagonal"), NS)), (D, seen)
        assert pens == set(PEN), D
    assert len({D for D, _, _ in SHAPES}) == len(SHAPES)  # one shape per level count: the above is per D
    # (33, 3, 23): the lines of eight consecutive levels start at all eight phases
    assert {(d * 3 * 23) % 8 for d in range(8)} == set(range(8))


# ---- 2. the extreme case -------------------------------------------------------------
def test_extreme_case_does_not_wrap(engine):
    D, H, W = 256, 2, 64
    full = np.full((D, H, W), s16.MAX_COST, np.uint16)
    alt = np.zeros((D, H, W), np.uint16)
    alt[0::3] = s16.MAX_COST
    alt[1::3, ::2, 1::2] = alt[1::3, 1::2, ::2] = s16.MAX_COST
    alt[2::3, ::2, ::2] = alt[2::3, 1::2, 1::2] = s16.MAX_COST
    want = [s16.sgm16(v, 4095, 4095, 255) for v in (full, alt)]
    assert max(int(w.max()) for w in want) <= 65512
    assert int(want[0].max()) == 8 * s16.MAX_COST and int(want[1].max()) > 32767  # (above 15 bits: a signed slip shows)
    out = fill(engine.empty((3, D, H, W), torch.uint16))
    got = engine.sgm_u16_batch(dev(np.stack([full, alt])), 4095, 4095, 255, out=out[:2])
    for j in range(2):
        same(got[j], want[j], f"the extreme case, element {j}")
    assert (host(out[2:]) == SENT).all()


# ---- 3. strides and phases -----------------------------------------------------------
SD, SH, SW = 66, 5, 67
SN = SD * SH * SW


@pytest.fixture(scope="module")
def three():
    """Three volumes of (66, 5, 67) and their aggregates for paths 15 and 255."""
    vols = [s16.random_volume(SD, SH, SW, seed=1700 + i) for i in range(3)]
    return vols, {p: [s16.sgm16(v, 205, 1638, p) for v in vols] for p in (15, 255)}


@pytest.mark.parametrize("paths", [15, 255])
def test_strides_and_phases(engine, three, paths):
    vols, aggs = three
    N = 3
    hv = dev(np.stack(vols)).view(torch.int16)
    surplus = ((0, 0), (1, 1), (8, 8), (8, 0), (1, 2))
    for (dv, da), ov, oa in itertools.product(surplus, (0, 1, 3, 7), (0, 1, 3, 7)):
        sv, sa = SN + dv, SN + da
        bv = engine.empty((ov + (N - 1) * sv + SN + 8,), torch.int16).fill_(7)
        ba = engine.empty((oa + (N - 1) * sa + SN + 8,), torch.int16).fill_(SENT_I16)
        gv = bv.as_strided((N, SD, SH, SW), (sv, SH * SW, SW, 1), ov)
        ga = ba.as_strided((N, SD, SH, SW), (sa, SH * SW, SW, 1), oa)
        gv.copy_(hv)
        before = bv.clone()
        assert gv.data_ptr() % 16 == 2 * ov and ga.data_ptr() % 16 == 2 * oa
        what = f"strides D H W + {dv}, {da}, offsets {ov}, {oa} elements, paths={paths}"
        got = engine.sgm_u16_batch(gv.view(torch.uint16), 205, 1638, paths, out=ga.view(torch.uint16))
        assert got.data_ptr() == ga.data_ptr()
        flat = host(ba)
        inside = np.zeros(flat.shape, bool)
        for j in range(N):
            lo = oa + j * sa
            same(flat[lo:lo + SN].reshape(SD, SH, SW), aggs[paths][j], f"element {j}, {what}")
            inside[lo:lo + SN] = True
        assert (flat[~inside] == SENT).all(), f"a store outside agg: {what}"
        assert torch.equal(bv, before), f"the vol buffer, {what}"
    # int16-viewed tensors are taken as they are
    ga = fill(engine.empty((N, SD, SH, SW), torch.uint16))
    engine.sgm_u16_batch(hv, 205, 1638, paths, out=ga.view(torch.int16))
    same(ga, np.stack(aggs[paths]), "int16-viewed tensors")


# ---- 4. quant_u16 ---------------------------------------------------------------------------
def quant_pool(n):
    """The exact values 0, 2 and -0.005, values whose product with 2047 lies within one ulp of a half-integer, then
    random floats in [-0.01, 2.01]."""
    F = np.float32
    rng = np.random.default_rng(44)
    half = []
    for k in (0, 1, 2, 3, 204, 1023, 2046, 2047, 3000, 4092, 4093):
        up = dn = F(k + 0.5) / F(2047)
        near = [up]
        for _ in range(3):
            up, dn = np.nextafter(up, F(3)), np.nextafter(dn, F(-1))
            near += [up, dn]
        mine = [x for x in near if abs(x * F(2047) - F(k + 0.5)) <= np.spacing(F(k + 0.5))]
        assert len(mine) >= 1, k
        half += mine
    pool = np.concatenate([np.array([0.0, 2.0, -0.005], F), np.array(half, F),
                           (F(2.02) * rng.random(4200, dtype=np.float32) - F(0.01)).astype(F)])
    prod = pool[3:3 + len(half)] * F(2047)
    assert (prod == np.floor(prod) + F(0.5)).any() and (prod != np.floor(prod) + F(0.5)).any()  # on and beside k + 1/2
    return np.ascontiguousarray(pool[:n])


@pytest.mark.parametrize("n", [1, 7, 4099])
def test_quant_u16(engine, n):
    src = quant_pool(n)
    want = s16.quant(src)
    assert len(src) == n and (n < 7 or {0, 4094} <= set(want.tolist()))
    for os_, od in itertools.product((0, 1), (0, 1, 5)):
        bs = engine.empty((n + 8,), torch.float32).fill_(1.0)
        bd = engine.empty((n + 16,), torch.int16).fill_(SENT_I16)
        bs[os_:os_ + n].copy_(torch.from_numpy(src))
        assert bs.data_ptr() % 16 == 0 and bd.data_ptr() % 16 == 0
        got = engine.quant_u16(bs[os_:os_ + n], out=bd[od:od + n])
        assert got.data_ptr() == bd.data_ptr() + 2 * od
        flat = host(bd)
        same(flat[od:od + n], want, f"n={n}, source offset {os_}, destination offset {od}")
        assert (flat[:od] == SENT).all() and (flat[od + n:] == SENT).all(), (n, os_, od)
        assert torch.equal(bs[os_:os_ + n].cpu(), torch.from_numpy(src))
    vol = torch.from_numpy(quant_pool(4095).reshape(5, 9, 91)).cuda()  # a volume, out=None
    q = engine.quant_u16(vol)
    assert q.dtype == torch.uint16 and tuple(q.shape) == (5, 9, 91)
    same(q, s16.quant(vol.cpu().numpy()), "a volume")


def test_quant_u16_errors(engine):
    L, ctx = engine.L, engine.ctx
    s = engine.empty((64,), torch.float32).fill_(0.5)
    d = engine.empty((64,), torch.int16).fill_(SENT_I16)
    sp, dp = s.data_ptr(), d.data_ptr()
    assert L.mvs_quant_u16_d(ctx, 16, sp, dp) == 0 and L.mvs_quant_u16_d(ctx, 0, sp, dp) == 0
    fill(d)
    for args in ((None, 16, sp, dp), (ctx, 16, None, dp), (ctx, 16, sp, None), (ctx, 16, sp, dp + 1), (ctx, 16, sp + 2, dp),
                 (ctx, 16, sp, sp), (ctx, 16, sp, sp + 62), (ctx, 16, sp + 4, sp)):
        assert L.mvs_quant_u16_d(*args) == -1, args
        assert b"mvs_quant_u16_d" in L.mvs_last_error()
    engine.synchronize()
    assert (host(d) == SENT).all() and bool((s == 0.5).all())
    with pytest.raises(ValueError):
        engine.quant_u16(s.double())
    with pytest.raises(ValueError):
        engine.quant_u16(s, out=engine.empty((64,), torch.float32))
    with pytest.raises(ValueError):
        engine.quant_u16(s, out=engine.empty((63,), torch.uint16))


# ---- 5. wta_u16 -----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 4, 130])
def test_wta_u16(engine, D):
    rng = np.random.default_rng(50 + D)
    levels = (np.arange(D, dtype=np.float32) * np.float32(0.5) + np.float32(1.25)).astype(np.float32)
    lev = torch.from_numpy(levels).cuda()
    # (H, W): 63 and 35 pixels are a multiple of no vector width, 60 takes the 8-byte form
    for (H, W), off in (((7, 9), 0), ((5, 7), 0), ((6, 10), 0), ((6, 10), 1), ((6, 10), 2)):
        agg = rng.choice(np.array([5, 9, 40000, 65512], np.uint16), size=(D, H, W))
        wd, wc = s16.wta(agg, levels)
        if D >= 4:
            assert (np.sort(agg, axis=0)[0] == np.sort(agg, axis=0)[1]).mean() > 0.2  # the minimum is tied often
        buf = engine.empty((D * H * W + 8,), torch.uint16)
        ga = buf[off:off + D * H * W].view(D, H, W)
        ga.view(torch.int16).copy_(torch.from_numpy(agg.view(np.int16)))
        assert ga.data_ptr() % 16 == 2 * off
        what = f"D={D} H={H} W={W} offset {off}"
        d, c = engine.wta_u16(ga, lev)
        same_f(d, wd, f"disp, {what}")
        same_f(c, wc, f"conf, {what}")
        disp = engine.empty((H, W), torch.float32).fill_(-1.0)
        d2, c2 = engine.wta_u16(ga, lev, disp=disp, want_conf=False)  # conf = NULL
        assert c2 is None and d2.data_ptr() == disp.data_ptr()
        same_f(d2, wd, f"disp without conf, {what}")
        same(ga, agg, "the aggregate is left as it was")
    L = engine.L
    assert L.mvs_wta_u16_d(engine.ctx, 9, 7, 0, ga.data_ptr(), lev.data_ptr(), d.data_ptr(), None) == -1
    assert L.mvs_wta_u16_d(engine.ctx, 10, 6, D, buf.data_ptr() + 1, lev.data_ptr(), d.data_ptr(), None) == -1
    assert b"mvs_wta_u16_d" in L.mvs_last_error()
    engine.synchronize()


# ---- 6. pipeline -----------------------------------------------------------------------------
PW, PH, PV, PD = 96, 40, 5, 16


def _settings():
    return params.Settings(spixl_size=8, array_width=PV, array_height=1, neib_hor=1, neib_ver=0, min_disp=0,
                           max_disp=PD - 1, inc=1, bl_ratio=1.0, window=5)


@pytest.fixture(scope="module")
def chain():
    """A small synthetic stack and, per view, the reference chain: orc.ncc_volume, the reference quantiser, sgm16_ref
    for masks 15 and 255, the reference winner."""
    stack, _ = synth.make_stack(PW, PH, PV, 1, 0, PD - 1, 1.0, 0x5EED + 16)
    l8 = orc.l8(orc.cvt(stack))
    levels = params.disparity_levels(0, PD - 1, 1)
    vs, sn = params.flatten_subsets(params.neighbour_lists(PV, 1, 1, 0))
    qs = [s16.quant(orc.ncc_volume(l8, levels, vs, sn, PV, 1.0, 5, z)) for z in range(PV)]
    win = {m: [s16.wta(s16.sgm16(q, s16.P1, s16.P2, m), levels) for q in qs] for m in (15, 255)}
    assert any((a[0] != b[0]).any() for a, b in zip(win[15], win[255]))  # the mask reaches the result
    return stack, win


@pytest.mark.parametrize("fused", [True, False])
def test_pipeline(engine, chain, fused):
    stack, win = chain
    rgbx = torch.from_numpy(stack).cuda()

    def run(**kw):
        return Pipeline(engine, _settings(), PW, PH, pixel_cost="ncc", fused=fused, subpixel=True, sgm=True,
                        **kw).exe_pipeline(rgbx)

    for paths in (15, 255):
        plain = run(sgm_paths=paths)
        for B in (1, 2, 5):
            on = run(sgm_paths=paths, sgm_batch=B, sgm_dtype="u16")
            what = f"fused {fused} sgm_paths {paths} sgm_batch {B}"
            assert tuple(on.disp_agg.shape) == tuple(on.conf_agg.shape) == (PV, PH, PW)
            for z in range(PV):
                same_f(on.disp_agg[z], win[paths][z][0], f"disp_agg z{z} {what}")
                same_f(on.conf_agg[z], win[paths][z][1], f"conf_agg z{z} {what}")
            for name in ("disp", "conf", "disp_sub"):
                same_f(getattr(on, name), getattr(plain, name).cpu().numpy(), f"{name} with and without the option, {what}")


def test_pipeline_buffers_and_errors(engine):
    """4 D H W + 2 B 2 D H W bytes with the option; with the default nothing new."""
    def ps(**kw):
        return Pipeline(engine, _settings(), PW, PH, pixel_cost="ncc", **kw).pixel

    for B, n in ((1, 1), (2, 2), (5, 5), (7, 5)):
        for fused in (True, False):
            p = ps(sgm=True, sgm_batch=B, fused=fused, sgm_dtype="u16")
            assert tuple(p.vol.shape) == (PD, PH, PW) and p.vol.dtype == torch.float32
            assert tuple(p.q.shape) == tuple(p.agg.shape) == (n, PD, PH, PW)
            assert p.q.dtype == p.agg.dtype == torch.uint16
            assert (p.p1_u16, p.p2_u16) == (205, 1638)
    p = ps(sgm=True, sgm_batch=2, fused=True)
    assert p.q is None and p.sgm_dtype == "f32" and p.agg.dtype == torch.float32
    cam = Pipeline(engine, _settings(), PW, PH, pixel_cost="ncc").cam
    for kw in (dict(sgm_dtype="u16"), dict(sgm=True, sgm_dtype="u8"), dict(sgm=True, sgm_dtype="u16", sgm_p2=2.5),
               dict(sgm=True, sgm_dtype="u16", sgm_p1=0.9, sgm_p2=0.8), dict(sgm=True, sgm_dtype="u16", sgm_p1=-0.1)):
        with pytest.raises(ValueError):
            Pipeline(engine, _settings(), PW, PH, pixel_cost="ncc", **kw)
        with pytest.raises(ValueError):
            PixelSweep(engine, cam, PW, PH, "ncc", 5, **kw)
    with pytest.raises(ValueError):
        Pipeline(engine, _settings(), PW, PH, pixel_cost="sad", sgm_dtype="u16")


# ---- 7. errors -------------------------------------------------------------------------
def test_errors(engine):
    D, H, W = 4, 3, 5
    n = D * H * W
    buf = fill(engine.empty((8 * n + 2 * 257 * 4,), torch.uint16), 100)
    agg_half = buf[4 * n:]
    L, ctx = engine.L, engine.ctx
    v, a = buf.data_ptr(), buf.data_ptr() + 2 * 4 * n  # two spans of up to four tight elements
    E_ARG, E_UNSUPPORTED = -1, -4

    def rc(ctx=ctx, W=W, H=H, D=D, N=2, v=v, vs=n, P1=205, P2=1638, paths=255, a=a, as_=n):
        r = L.mvs_sgm8_u16_batch_d(ctx, W, H, D, N, v, vs, P1, P2, paths, a, as_)
        if r != 0:
            assert b"mvs_sgm8_u16_batch_d" in L.mvs_last_error()
        return r

    def untouched():
        engine.synchronize()
        assert (host(agg_half) == 100).all()

    assert rc(D=257, N=1, H=1, W=4, vs=257 * 4, as_=257 * 4, a=v + 2 * 257 * 4) == E_UNSUPPORTED
    assert b"256 levels" in L.mvs_last_error()
    assert rc(P2=4096) == E_ARG and rc(P1=1639) == E_ARG and rc(P1=-1) == E_ARG and rc(P1=4096, P2=4096) == E_ARG
    assert b"penalties" in L.mvs_last_error()
    for paths in (0, 256, -1):
        assert rc(paths=paths) == E_ARG, paths
        assert b"mvs_sgm8_u16_batch_d: paths must be a mask in 1..255" in L.mvs_last_error()
    assert rc(v=v + 1) == E_ARG and rc(a=a + 1) == E_ARG
    assert b"2-byte aligned" in L.mvs_last_error()
    assert rc(N=2, vs=3 * n, a=v + 2 * n) == E_ARG and b"overlap" in L.mvs_last_error()
    assert rc(N=2, a=v + 2 * n) == E_ARG and rc(a=v) == E_ARG and rc(N=2, a=v + 2 * (2 * n - 1)) == E_ARG
    assert rc(vs=n - 1) == E_ARG and rc(as_=n - 1) == E_ARG
    assert b"stride" in L.mvs_last_error()
    for N in (0, -1, 65536):
        assert rc(N=N) == E_ARG, N
        assert b"mvs_sgm8_u16_batch_d: N must be in 1..65535" in L.mvs_last_error()
    assert rc(ctx=None) == E_ARG and rc(v=None) == E_ARG and rc(a=None) == E_ARG
    assert rc(W=0) == E_ARG and rc(H=0) == E_ARG and rc(D=0) == E_ARG and rc(W=1 << 20, H=1 << 20) == E_ARG
    untouched()
    # accepted: abutting spans, the limits of the penalties, one path
    assert rc() == 0 and rc(N=4) == 0 and rc(N=2, v=a, a=v) == 0
    assert rc(P1=0, P2=0) == 0 and rc(P1=4095, P2=4095) == 0 and rc(paths=16) == 0 and rc(paths=1) == 0
    # the Python layer
    vols = buf[:2 * n].view(2, D, H, W)
    with pytest.raises(ValueError):
        engine.sgm_u16_batch(vols[0])  # three dimensions
    with pytest.raises(ValueError):
        engine.sgm_u16_batch(vols.float())
    with pytest.raises(ValueError):
        engine.sgm_u16_batch(vols, out=engine.empty((2, D, H, W), torch.float32))
    with pytest.raises(ValueError):
        engine.sgm_u16_batch(vols, out=engine.empty((3, D, H, W), torch.uint16))
    with pytest.raises(ValueError):
        engine.sgm_u16_batch(vols, 0.1, 0.8)  # the float32 call's penalties
    with pytest.raises(_lib.MvsError, match="mvs_sgm8_u16_batch_d: the vol and agg spans overlap"):
        engine.sgm_u16_batch(vols, out=vols)
    with pytest.raises(_lib.MvsError, match="mvs_sgm8_u16_batch_d: paths must be a mask in 1..255"):
        engine.sgm_u16_batch(vols, paths=256)
    engine.synchronize()
