"""The sub-level disparity of a semi-global aggregate on the GPU (csrc/wta.hip
and csrc/sgm16.hip through mvs_wta_agg_sub_d and mvs_wta_u16_sub_d) against the
definition in tests/sgm_sub_ref.py, bit for bit.

1. Independent random agg and raw, so that all four classes occur (b at an
   end, a side without a window, raw without a minimum at b, fitted), on the
   smallest shapes that reach every kernel form (the table at CASES).  Before
   the GPU is compared the reference alone must show every class often enough.
   disp and conf equal the plain winner pass on the same agg; the same disp_sub
   comes out with disp and / or conf NULL; the outputs are slices of larger
   buffers that keep their sentinel outside; the inputs are left as they were.
2. agg is vol: wta_sub(vol)'s bits.
3. The pipeline's sgm_subpixel in its three aggregation paths, fused and
   two-pass.
4. The argument errors."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd import params, synth
from cl_multiview_stereo_amd.pipeline import Pipeline
from oracle import oracle as orc
from tests import sgm16_ref as s16
from tests import sgm8_ref as s8
from tests import sgm_sub_ref as ss
from tests import subpixel_ref as sr

pytestmark = pytest.mark.gpu

F = np.float32
SENT = -777.0
# ((D, H, W), elements agg starts past an 8-byte boundary, elements raw does)
CASES = [
    ((1, 5, 70), 0, 0), ((2, 5, 70), 0, 0), ((3, 5, 70), 0, 0), ((4, 5, 70), 0, 0),
    ((17, 5, 70), 0, 0),    # H W = 350: the one-pixel form, a partial last block, a level tail behind the unrolled loop
    ((33, 6, 72), 0, 0), ((256, 6, 72), 0, 0),  # H W = 432: the four-pixel form of the uint16 pass; 33: its level tail
    ((17, 6, 72), 1, 0),    # agg one element past the boundary: the one-pixel form although H W % 4 == 0
    ((17, 6, 72), 0, 1),    # raw one element past it while agg is aligned: the four-pixel form, raw on its own
]
IDS = ["x".join(map(str, s)) + (f"+agg{a}" if a else "") + (f"+raw{r}" if r else "") for s, a, r in CASES]


def levels_of(D):
    """Steps of 0.5, 0.7, 1 or 3 from 0.05, wrapped into [0, 4): not ordered (the definition does not ask for it),
    steps of either sign.  0.7 and 3 are no powers of two, so off * step is rounded, and a level stays as small as
    the product, so that rounding reaches the sum: a fused multiply-add in levels[b] + off * step would show
    (test_every_class_and_edge_occurs counts the pixels on which it would)."""
    rng = np.random.default_rng(7000 + D)
    up = 0.05 + np.concatenate([[0], np.cumsum(rng.choice([0.5, 0.7, 1.0, 3.0], D - 1))])
    return np.mod(up, 4.0).astype(np.float32)


def fused_would_give(levels, off, b):
    """levels[b] + off * step with the product kept exact (float64 holds it) and one rounding at the end: what a fused
    multiply-add computes."""
    D = levels.shape[0]
    lm, lb, lp = levels[np.clip(b - 1, 0, D - 1)], levels[b], levels[np.clip(b + 1, 0, D - 1)]
    step = np.where(off < 0, lb - lm, lp - lb).astype(np.float32)
    return (lb.astype(np.float64) + off.astype(np.float64) * step.astype(np.float64)).astype(np.float32)


def inputs(dtype, k):
    """[(name, agg, raw)] of case k: two aggregates (ties at the minimum common / rare) times two raw volumes (the
    reference's random volume; few distinct values, so that rp == r0 occurs), drawn independently of each other."""
    D, H, W = CASES[k][0]
    rng = np.random.default_rng([81, k, dtype == "u16"])
    if dtype == "u16":
        aggs = [("agg 0..63", rng.integers(0, 64, (D, H, W)).astype(np.uint16)),
                ("agg 0..59999", rng.integers(0, 60000, (D, H, W)).astype(np.uint16))]
        raws = [("raw random_volume", s16.random_volume(D, H, W, seed=8100 + k)),
                ("raw 0..7", rng.integers(0, 8, (D, H, W)).astype(np.uint16))]
    else:
        aggs = [("agg k/4", (rng.integers(0, 64, (D, H, W)) * 0.25).astype(np.float32)),
                ("agg random", (rng.random((D, H, W)) * 50).astype(np.float32))]
        few = (rng.integers(0, 8, (D, H, W)) * 0.125).astype(np.float32)
        few[rng.random((D, H, W)) < 1 / 16] = F(2.0)
        raws = [("raw random_volume", sr.random_volume(D, H, W, seed=8100 + k)), ("raw k/8 and 2", few)]
    return [(f"{an}, {rn}", a, r) for an, a in aggs for rn, r in raws]


_REF = {}


def ref(dtype, k):
    """[(name, agg, raw, levels, (disp_sub, cls, off, b))] of case k, computed once."""
    if (dtype, k) not in _REF:
        lev = levels_of(CASES[k][0][0])
        fit = ss.fit_u16 if dtype == "u16" else ss.fit_f32
        _REF[(dtype, k)] = [(n, a, r, lev, fit(a, r, lev)) for n, a, r in inputs(dtype, k)]
    return _REF[(dtype, k)]


def put(engine, a, off):
    """a on the GPU, its first element `off` elements past a 16-byte boundary."""
    tdt = torch.uint16 if a.dtype == np.uint16 else torch.float32
    buf = engine.empty((a.size + 8,), tdt)
    t = buf[off:off + a.size].view(a.shape)
    src = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    (t.view(torch.int16) if a.dtype == np.uint16 else t).copy_(src)
    assert t.data_ptr() % 16 == a.itemsize * off
    return t


def host(t):
    t = t.view(torch.int16) if t.dtype == torch.uint16 else t
    a = np.ascontiguousarray(t.cpu().numpy())
    return a.view(np.uint16) if a.dtype == np.int16 else a


def same_f(got, want, what):
    got, want = (x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in (got, want))
    got, want = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.count_nonzero(got != want)
    assert bad == 0, f"{what}: {bad}/{got.size} differ, first at {np.argwhere(got != want)[:3].tolist()}"


class Guarded:
    """Three [H, W] outputs as slices of one larger buffer filled with a sentinel."""
    PAD = 24

    def __init__(self, engine, H, W):
        self.n = H * W
        self.buf = engine.empty((3, self.n + 2 * self.PAD), torch.float32).fill_(SENT)
        self.out = [self.buf[i, self.PAD:self.PAD + self.n].view(H, W) for i in range(3)]

    def check(self, written, what):
        """Rows in `written` may have changed inside their slice; everything else holds the sentinel."""
        b = self.buf.cpu().numpy()
        for i in range(3):
            assert (b[i, :self.PAD] == F(SENT)).all() and (b[i, self.PAD + self.n:] == F(SENT)).all(), (what, i)
            if i not in written:
                assert (b[i] == F(SENT)).all(), (what, i)


def call(engine, dtype, *a, **kw):
    return (engine.wta_u16_sub if dtype == "u16" else engine.wta_agg_sub)(*a, **kw)


# ---- 1. random, independent agg and raw -------------------------------------------------------
@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_random(engine, dtype, k):
    (D, H, W), oa, orw = CASES[k]
    for name, agg, raw, levels, (wsub, cls, off, b) in ref(dtype, k):
        what = f"{dtype} D{D} H{H} W{W} agg+{oa} raw+{orw}: {name}"
        if D >= 4:  # on the reference alone: the fit and its refusal both carry weight
            assert (cls == ss.FITTED).mean() >= 0.1 and (cls == ss.NO_MINIMUM).mean() >= 0.2, what
        ga, gr = put(engine, agg, oa), put(engine, raw, orw)
        lev = torch.from_numpy(levels).cuda()
        wd, wc = (engine.wta_u16 if dtype == "u16" else engine.wta)(ga, lev)  # the plain winner pass on the same agg
        g = Guarded(engine, H, W)
        d, c, s = call(engine, dtype, ga, gr, lev, disp=g.out[0], conf=g.out[1], out=g.out[2])
        assert (d.data_ptr(), c.data_ptr(), s.data_ptr()) == tuple(o.data_ptr() for o in g.out)
        same_f(s, wsub, f"disp_sub, {what}")
        same_f(d, wd, f"disp, {what}")
        same_f(c, wc, f"conf, {what}")
        same_f(d, levels[b], f"disp against the reference's winner, {what}")
        g.check({0, 1, 2}, what)
        for with_disp, with_conf in ((True, False), (False, True), (False, False)):
            g = Guarded(engine, H, W)
            d, c, s = call(engine, dtype, ga, gr, lev, disp=g.out[0] if with_disp else None,
                           conf=g.out[1] if with_conf else None, out=g.out[2], want_conf=with_conf)
            assert (d is None) == (not with_disp) and (c is None) == (not with_conf)
            same_f(s, wsub, f"disp_sub with disp {with_disp} conf {with_conf}, {what}")
            if with_disp:
                same_f(d, wd, f"disp without conf, {what}")
            if with_conf:
                same_f(c, wc, f"conf without disp, {what}")
            g.check({2} | ({0} if with_disp else set()) | ({1} if with_conf else set()), what)
        s = call(engine, dtype, ga, gr, lev)[2]  # out=None: a new [H, W] tensor
        same_f(s, wsub, f"disp_sub, out=None, {what}")
        assert np.array_equal(host(ga), agg) and np.array_equal(host(gr), raw), what
        assert np.array_equal(lev.cpu().numpy(), levels), what


@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_every_class_and_edge_occurs(dtype):
    """Over all shapes together, on the reference alone: b = 0, b = D - 1, a side without a window, rp == r0."""
    first = last = no_window = tie = fused = 0
    for k, ((D, H, W), _, _) in enumerate(CASES):
        for name, agg, raw, levels, (wsub, cls, off, b) in ref(dtype, k):
            fused += int(((cls == ss.FITTED) & (fused_would_give(levels, off, b) != wsub)).sum())
            if D >= 2:
                first += int((b == 0).sum())
                last += int((b == D - 1).sum())
            no_window += int((cls == ss.NO_WINDOW).sum())
            tie += int(((cls == ss.FITTED) & (off == F(0.5))).sum())
            assert (wsub[cls != ss.FITTED] == levels[b][cls != ss.FITTED]).all()
            assert (wsub[(cls == ss.FITTED) & (off != 0)] != levels[b][(cls == ss.FITTED) & (off != 0)]).all()
    assert min(first, last, no_window, tie) >= 20, (first, last, no_window, tie)
    assert fused >= 100, fused  # pixels whose bits a fused multiply-add would change


# ---- 2. agg is vol ----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [3, 17, 33])
def test_agg_is_vol(engine, D):
    H, W = 6, 70
    levels = levels_of(D)
    lev = torch.from_numpy(levels).cuda()
    vol = sr.random_volume(D, H, W, seed=5)
    gv = torch.from_numpy(vol).cuda()
    d, c, s = engine.wta_agg_sub(gv, gv, lev, disp=engine.empty((H, W), torch.float32))
    same_f(s, engine.wta_sub(gv, lev), f"agg is vol, D={D}: wta_sub's bits")
    same_f(s, sr.fit(vol, levels)[0], f"agg is vol, D={D}: subpixel_ref.fit")
    wd, wc = engine.wta(gv, lev)
    same_f(d, wd, "disp")
    same_f(c, wc, "conf")
    s = engine.wta_agg_sub(gv, gv.clone(), lev)[2]  # the same values in another buffer
    same_f(s, sr.fit(vol, levels)[0], f"agg equals vol, D={D}")
    raw = s16.random_volume(D, H, W, seed=6)
    gr = put(engine, raw, 0)
    wsub, cls, _, _ = ss.fit_u16(raw, raw, levels)
    assert not (cls == ss.NO_MINIMUM).any()
    same_f(engine.wta_u16_sub(gr, gr, lev)[2], wsub, f"uint16, agg is raw, D={D}")


# ---- 3. pipeline ------------------------------------------------------------------------------
PW, PH, PV, PD, PATHS = 96, 40, 5, 16, 255


def _settings():
    return params.Settings(spixl_size=8, array_width=PV, array_height=1, neib_hor=1, neib_ver=0, min_disp=0,
                           max_disp=PD - 1, inc=1, bl_ratio=1.0, window=5)


@pytest.fixture(scope="module")
def chain():
    """The small synthetic stack of test_gpu_sgm16.py's pipeline test and, per view, the reference chain: the cost
    volume, float32: sgm8_ref, uint16: the reference quantiser and sgm16_ref; then sgm_sub_ref on (aggregate, raw)."""
    stack, _ = synth.make_stack(PW, PH, PV, 1, 0, PD - 1, 1.0, 0x5EED + 16)
    l8 = orc.l8(orc.cvt(stack))
    levels = params.disparity_levels(0, PD - 1, 1)
    vs, sn = params.flatten_subsets(params.neighbour_lists(PV, 1, 1, 0))
    vols = [orc.ncc_volume(l8, levels, vs, sn, PV, 1.0, 5, z) for z in range(PV)]
    qs = [s16.quant(v) for v in vols]
    want = {"f32": [ss.fit_f32(s8.sgm8(v, 0.1, 0.8, PATHS), v, levels) for v in vols],
            "u16": [ss.fit_u16(s16.sgm16(q, s16.P1, s16.P2, PATHS), q, levels) for q in qs]}
    for dtype in want:  # the option reaches the result, and not only through the raw volume's own winner
        assert min((w[1] == ss.FITTED).mean() for w in want[dtype]) >= 0.1  # (the bound of the random shapes)
        assert any((w[3] != np.argmin(v, 0)).any() for w, v in zip(want[dtype], vols))
    return stack, levels, vols, want


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("kw", [dict(sgm_batch=1), dict(sgm_batch=2), dict(sgm_batch=1, sgm_dtype="u16"),
                                dict(sgm_batch=2, sgm_dtype="u16")], ids=lambda kw: "-".join(map(str, kw.values())))
def test_pipeline(engine, chain, fused, kw):
    """sgm_batch = 2 over five views: groups of 2, 2 and 1."""
    stack, levels, vols, want = chain
    rgbx = torch.from_numpy(stack).cuda()

    def run(**more):
        return Pipeline(engine, _settings(), PW, PH, pixel_cost="ncc", fused=fused, subpixel=True, sgm=True,
                        sgm_paths=PATHS, **kw, **more).exe_pipeline(rgbx)

    off, on = run(), run(sgm_subpixel=True)
    what = f"fused {fused} {kw}"
    assert off.disp_agg_sub is None and tuple(on.disp_agg_sub.shape) == (PV, PH, PW)
    w = want[kw.get("sgm_dtype", "f32")]
    for z in range(PV):
        same_f(on.disp_agg_sub[z], w[z][0], f"disp_agg_sub z{z} {what}")
        same_f(on.disp_agg[z], levels[w[z][3]], f"disp_agg z{z} against the reference's winner, {what}")
        same_f(on.disp_sub[z], sr.fit(vols[z], levels)[0], f"disp_sub z{z} {what}")
    for name in ("disp", "conf", "disp_sub", "disp_agg", "conf_agg"):
        same_f(getattr(on, name), getattr(off, name).cpu().numpy(), f"{name} with and without the option, {what}")
    # without subpixel: the option stands on its own
    alone = Pipeline(engine, _settings(), PW, PH, pixel_cost="ncc", fused=fused, sgm=True, sgm_paths=PATHS,
                     sgm_subpixel=True, **kw).exe_pipeline(rgbx)
    assert alone.disp_sub is None
    same_f(alone.disp_agg_sub, on.disp_agg_sub.cpu().numpy(), f"disp_agg_sub without subpixel, {what}")


# ---- 4. errors --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["u16", "f32"])
def test_errors(engine, dtype):
    D, H, W = 4, 3, 6
    n, P = D * H * W, H * W
    es = 2 if dtype == "u16" else 4
    L, ctx = engine.L, engine.ctx
    fn = L.mvs_wta_u16_sub_d if dtype == "u16" else L.mvs_wta_agg_sub_d
    name = b"mvs_wta_u16_sub_d" if dtype == "u16" else b"mvs_wta_agg_sub_d"
    vol = engine.empty((2, D, H, W), torch.uint16 if dtype == "u16" else torch.float32)
    vol.view(torch.int16).fill_(3) if dtype == "u16" else vol.fill_(0.5)
    lev = torch.from_numpy(levels_of(D)).cuda()
    outs = engine.empty((4, P), torch.float32).fill_(SENT)
    a, r, l = vol[0].data_ptr(), vol[1].data_ptr(), lev.data_ptr()
    d, c, s = (outs[i].data_ptr() for i in range(3))

    def rc(ctx=ctx, W=W, H=H, D=D, a=a, r=r, l=l, d=d, c=c, s=s):
        got = fn(ctx, W, H, D, a, r, l, d, c, s)
        if got != 0:
            assert name in L.mvs_last_error()
        return got

    assert rc(ctx=None) == -1 and rc(a=None) == -1 and rc(r=None) == -1 and rc(l=None) == -1 and rc(s=None) == -1
    assert rc(W=0) == -1 and rc(H=0) == -1 and rc(D=0) == -1 and rc(D=-1) == -1 and rc(W=1 << 20, H=1 << 20) == -1
    if dtype == "u16":
        assert rc(a=a + 1) == -1 and rc(r=r + 1) == -1
        assert b"2-byte aligned" in L.mvs_last_error()
    # outputs that overlap each other
    assert rc(d=s) == -1 and rc(c=s) == -1 and rc(d=c) == -1 and rc(s=d + 4) == -1 and rc(c=d + 4 * (P - 1)) == -1
    assert b"overlap" in L.mvs_last_error()
    # outputs that overlap an input
    assert rc(s=a) == -1 and rc(s=a + es * (n - 1)) == -1 and rc(d=r) == -1 and rc(c=r + es * P) == -1
    assert rc(s=l) == -1 and rc(c=l) == -1
    assert b"overlaps an input" in L.mvs_last_error()
    engine.synchronize()
    assert bool((outs == SENT).all())  # nothing was launched
    # accepted: disp and conf NULL, agg and raw one buffer, outputs that abut
    assert rc(d=None) == 0 and rc(c=None) == 0 and rc(d=None, c=None) == 0 and rc(r=a) == 0 and rc() == 0
    engine.synchronize()
    assert bool((outs[3] == SENT).all()) and not bool((outs[:3] == SENT).any())
    # the Python layer
    meth = engine.wta_u16_sub if dtype == "u16" else engine.wta_agg_sub
    other = engine.empty((D, H, W), torch.float32 if dtype == "u16" else torch.uint16)
    for args, kw in (((vol[0], vol[1][:3], lev), {}), ((vol[0], other, lev), {}), ((other, vol[1], lev), {}),
                     ((vol[0], vol[1], lev[:3]), {}), ((vol[0], vol[1], lev), dict(out=outs[0])),
                     ((vol[0], vol[1], lev), dict(disp=outs[0].view(H, W).double()))):
        with pytest.raises(ValueError):
            meth(*args, **kw)
    engine.synchronize()
