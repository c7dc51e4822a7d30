"""Built inputs for the per-pixel SAD sweep (helper, no tests; numpy only).

Every other SAD test feeds mvs_sweep_pixel_sad_d synth.make_stack images
converted by cvt, with ascending non-negative integer levels.
engine.sweep_pixel_sad and orc.sweep_pixel_sad take Lab, the level list and
the neighbour lists as plain arrays, so here they are made by hand, on top of
tests/sweep_content.py (whose contents, level lists, camera() and costs() are
reused as they are):

  lab()          sweep_content's contents plus per12 / per10 / p2d12, whose
                 period is no multiple of a chunk of 8 or 16 levels, swap5,
                 whose winners turn on the order of the colour sum, and a
                 fourth channel of NaN on request
  level_list()   sweep_content's lists plus even (0, 2, 4, ...) and far500
                 (500, 501, ...: every projection leaves the image)
  s1_geometry()  the centres and extents with which sweep_content.costs()
                 restates the per-pixel sweep (S = 1: pixel (x, y) is its own
                 superpixel, unit tap steps)
  costs()        the per-level cost on that grid, restated in numpy float32
  band_fit()     the rule by which a k_sad_band form can stage a view

CASES names every input the GPU tests run (tests/test_gpu_sad_content.py) and
records, per reference view, which band forms can take it;
tests/test_sad_content_cpu.py pins the state each case is there for on the
oracle alone.  Everything is deterministic in its arguments."""
from __future__ import annotations

import numpy as np

from tests import sweep_content as sc

f32 = np.float32
SEED = sc.SEED
FORMS = ("sys8x2", "sys8")       # the band forms plan_sad tries, in its order; "gather" takes everything
LEVELS_PER_CHUNK = {"sys8x2": 16, "sys8": 8}
PAIRS_PER_WAVE = {"sys8x2": 2, "sys8": 1}


# ---- Lab contents ------------------------------------------------------------
def lab(content, aw, ah, W, H, seed=SEED, wnan=False):
    """float32 [V, H, W, 4]; .w = 0, or NaN with wnan.

    per12 / per10  as sweep_content's per16: columns of period p, constant
                   down the rows, view v shifted by vx * d0(y), d0 = 3 + 7
                   (y // 12), odd views with L += 0.75 (tied minima above
                   zero).  Levels p apart tie, and p is no multiple of a chunk
                   (8 or 16 levels): the tied levels fall into different
                   waves, the first of them not always into the lowest.
    p2d12          a 12 x 12 tile shifted by (vx * d0, vy * d0): 2-D arrays.
    swap5          view 0 all zero; every other view zero but for one pixel
                   in five, (2 + 5 k, 2 + 5 l), so that a 5 x 5 window holds
                   exactly one of them and a level's cost is that pixel's
                   colour sum, formed once.  Along a row the pixels come in
                   pairs (p, q, r), (p, r, q) with p, q, r near 11, their sum
                   in [32, 34) -- where adding and taking off the 30 of a tap
                   is exact -- and (p + q) + r != (p + r) + q in float32: the
                   two sums of the cheapest pair are an ulp apart, and which
                   is lower depends on the order |dL| + |da| + |db| is added in.
    everything else: sweep_content.lab."""
    V = aw * ah
    if content == "swap5":
        rng = np.random.default_rng([seed, sum(map(ord, content)), W, H])
        ys, xs = np.arange(2, H, 5), np.arange(2, W, 5)
        t = rng.uniform(10.7, 11.3, (len(ys), (len(xs) + 1) // 2, 3)).astype(f32)
        while True:
            same = (t[..., 0] + t[..., 1]) + t[..., 2] == (t[..., 0] + t[..., 2]) + t[..., 1]
            if not same.any():
                break
            t[same] = rng.uniform(10.7, 11.3, (int(same.sum()), 3)).astype(f32)
        lx = np.arange(len(xs))
        col = np.where((lx % 2 == 1)[None, :, None], t[:, lx // 2][..., [0, 2, 1]], t[:, lx // 2])
        out = np.zeros((V, H, W, 4), f32)
        out[1:, ys[:, None], xs[None, :], :3] = col
        return out
    if content in ("per12", "per10", "p2d12"):
        rng = np.random.default_rng([seed, sum(map(ord, content)), W, H])
        vx = (np.arange(V) % aw)[:, None, None]
        vy = (np.arange(V) // aw)[:, None, None]
        y = np.arange(H)[None, :, None]
        x = np.arange(W)[None, None, :]
        d0 = sc._d0(H)[None, :, None]
        if content == "p2d12":
            out = sc._colours(rng, (12, 12))[(y + vy * d0) % 12, (x + vx * d0) % 12]
        else:
            p = int(content[3:])
            out = sc._colours(rng, (p,))[(x + vx * d0) % p]
            out[1::2, :, :, 0] += f32(0.75)
        out = np.ascontiguousarray(out, f32)
    else:
        out = sc.lab(content, aw, ah, W, H, seed)
    assert out.shape == (V, H, W, 4) and np.isfinite(out).all() and not out[..., 3].any()
    if wnan:
        out[..., 3] = np.nan
    return out


# ---- level lists -------------------------------------------------------------
def level_list(kind, D, seed=SEED):
    """float32 [D]: "even" 0, 2, 4, ...; "far500" 500, 501, ...; else sweep_content.level_list."""
    if kind == "even":
        return np.ascontiguousarray(2 * np.arange(D), f32)
    if kind == "far500":
        return np.ascontiguousarray(500 + np.arange(D), f32)
    return sc.level_list(kind, D, seed)


# ---- the S = 1 geometry --------------------------------------------------------
def s1_geometry(V, W, H):
    """(spixl [V, H, W, 8] float32, rep [V, H, W, 8] uint8) of the S = 1 grid as
    orc.sweep_pixel_sad builds it: the centre of pixel (x, y) is (x, y), every
    extent 0 (unit tap steps).  Only slots 1 and 2 matter to costs()."""
    sp = np.zeros((V, H, W, 8), f32)
    sp[..., 1] = np.arange(W, dtype=f32)[None, None, :]
    sp[..., 2] = np.arange(H, dtype=f32)[None, :, None]
    return sp, np.zeros((V, H, W, 8), np.uint8)


def costs_general(m, z):
    """sweep_content.costs of reference view z of the inputs m = make(name)
    under s1_geometry: (cost [H W, D], ntap, frac), the pixels in row-major
    order.  It gathers both colours of every (pixel, level, tap) anew: exact,
    and slow -- costs() below is the same arithmetic on the S = 1 grid."""
    sp, rep = s1_geometry(m["V"], m["W"], m["H"])
    return sc.costs(m["lab"], sp, rep, m["levels"], m["vs"], m["sn"], m["aw"], m["bl"], z)


def costs(m, z, frac=True):
    """costs_general() restated for the S = 1 grid, where the tap (i, j) of
    pixel (x, y) is pixel (x + i, y + j): per neighbour the absolute
    differences of every (level, pixel) of the image plus its 2-pixel halo are
    formed once, and the 25 taps are shifted views of that plane, summed in
    the reference's order (x offset outer, y offset inner; val += 30, and for
    a tap inside the image val -= 30, val += ad).  Returns (cost [H W, D]
    float32 -- the minimum over neighbours, 1e6 with an empty list --, ntap
    [H W, D] -- the in-image taps of the first neighbour that attains it --,
    fracx, fracy [H W, D] bool -- some in-image tap of any neighbour has
    xr - d dx, or yr - bl d dy, in (-1, 0): truncated to column or row 0; None
    without frac, which saves a third of the time)."""
    lab3 = m["lab"][..., :3]
    W, H, aw, D = m["W"], m["H"], m["aw"], m["D"]
    lv, bl = m["levels"], f32(m["bl"])
    k30 = f32(30.0)
    xr, yr = np.arange(-2, W + 2), np.arange(-2, H + 2)
    a = lab3[z][np.clip(yr, 0, H - 1)][:, np.clip(xr, 0, W - 1)]  # [H + 4, W + 4, 3]
    cost = np.full((D, H, W), f32(1000000.0), f32)
    ntap = np.zeros((D, H, W), np.int16)
    fracx = np.zeros((D, H, W), bool) if frac else None
    fracy = np.zeros((D, H, W), bool) if frac else None
    for view in m["vs"][z, :m["sn"][z]]:
        view = int(view)
        fx = xr.astype(f32)[None, :] - (lv * f32(view % aw - z % aw))[:, None]     # [D, W + 4]
        fy = yr.astype(f32)[None, :] - ((bl * lv) * f32(view // aw - z // aw))[:, None]  # [D, H + 4]
        assert fx.dtype == f32 and fy.dtype == f32
        xp, yp = np.trunc(fx).astype(np.int64), np.trunc(fy).astype(np.int64)
        okx = (xr >= 0) & (xr < W) & (xp >= 0) & (xp < W)
        oky = (yr >= 0) & (yr < H) & (yp >= 0) & (yp < H)
        ok = oky[:, :, None] & okx[:, None, :]                                          # [D, H + 4, W + 4]
        b = lab3[view][np.clip(yp, 0, H - 1)[:, :, None], np.clip(xp, 0, W - 1)[:, None, :]]
        ad = np.abs(a[..., 0] - b[..., 0]) + np.abs(a[..., 1] - b[..., 1])
        ad = ad + np.abs(a[..., 2] - b[..., 2])
        negx = ok & (fx < 0)[:, None, :]
        negy = ok & (fy < 0)[:, :, None]
        val = np.zeros((D, H, W), f32)
        cnt = np.zeros((D, H, W), np.int16)
        for i in range(5):
            for j in range(5):
                o = ok[:, j:j + H, i:i + W]
                v30 = val + k30
                val = np.where(o, (v30 - k30) + ad[:, j:j + H, i:i + W], v30)
                cnt += o
                if frac:
                    fracx |= negx[:, j:j + H, i:i + W]
                    fracy |= negy[:, j:j + H, i:i + W]
        take = val < cost  # the oracle's strict-< scan over the neighbours
        cost = np.where(take, val, cost)
        ntap = np.where(take, cnt, ntap)
    assert cost.dtype == f32
    return tuple(None if t is None else np.ascontiguousarray(t.reshape(D, H * W).T) for t in (cost, ntap, fracx, fracy))


# ---- which band form can stage a view ---------------------------------------------
def band_fit(m, z, form):
    """The band pitch (64 or 128 columns) with which k_sad_band form `form` can
    stage reference view z, or None.  The rule (sad_band_geometry), restated:
    every column shift d dx is integral; within every chunk of 16 (sys8x2) or
    8 (sys8) list-consecutive levels the column shifts of a neighbour span at
    most 64; two buffers of (12 + ceil(row-shift span) [+ 1 unless every row
    shift is integral]) rows of that pitch, 16 bytes a pixel, plus the row
    table fit 160 KiB."""
    DC = LEVELS_PER_CHUNK[form]
    aw, lv, bl = m["aw"], m["levels"], f32(m["bl"])
    span_x, span_y, aff = 0, f32(0), True
    for view in m["vs"][z, :m["sn"][z]]:
        dx, dy = int(view) % aw - z % aw, int(view) // aw - z // aw
        fdx, fdy = lv * f32(dx), (bl * lv) * f32(dy)
        if (fdx != np.trunc(fdx)).any():
            return None
        aff = aff and bool((fdy == np.trunc(fdy)).all())
        for c in range(0, len(lv), DC):
            span_x = max(span_x, int(fdx[c:c + DC].max() - fdx[c:c + DC].min()))
            span_y = max(span_y, fdy[c:c + DC].max() - fdy[c:c + DC].min())
    bw = (64 + span_x + 63) // 64 * 64
    brows = 12 + int(np.ceil(span_y)) + (0 if aff else 1)
    lds = 16 * 2 * brows * bw + (0 if aff else 4 * 2 * DC * 12)
    return bw if bw <= 128 and lds <= 160 * 1024 else None


# ---- the cases the GPU tests run ------------------------------------------------
BOTH = frozenset(FORMS)
NEITHER = frozenset()


def _case(content, aw, ah, W, H, D, levels="unit", bl=1.0, affine=True, forms=BOTH, bw64=(), wnan=False, seed=SEED,
          **cam):
    """forms: the band forms that can stage a view -- one set for every view,
    or a tuple of one set per view.  bw64: the views whose band is 64 columns
    wide (the BWT = 64 instantiations in the affine form); the others' is 128.
    affine: every row shift (bl d dy) is integral, so the band forms address
    rows affinely unless MVS_SAD_AFF is set.  All three written by hand from
    sad_band_geometry; band_fit() and the GPU tests check them."""
    V = aw * ah
    forms = tuple(forms) if isinstance(forms, tuple) else (forms,) * V
    assert len(forms) == V
    return dict(content=content, aw=aw, ah=ah, W=W, H=H, D=D, levels=levels, bl=bl, affine=affine, forms=forms,
                bw64=tuple(bw64), wnan=wnan, seed=seed, cam=cam)


T33 = dict(aw=3, ah=3, W=70, H=27, nh=1, nv=1)  # the 3 x 3 array on a 70 x 27 image, the 8 surrounding views
H31 = dict(aw=3, ah=1, W=120, H=40, nh=2)       # the 3 x 1 array on 120 x 40, both other views neighbours
CASES = {}
# ties whose first level sits in a higher wave than a later one, |dx| up to 4
CASES["per12_h5"] = _case("per12", 5, 1, 130, 30, 70, nh=4)
CASES["per10_h3"] = _case("per10", 3, 1, 130, 30, 70, nh=2)
# the same in two dimensions: the affine and the row-table form
CASES["p2d12_bl1"] = _case("p2d12", D=40, **T33)
CASES["p2d12_bl1.0359"] = _case("p2d12", D=40, bl=1.0359, affine=False, **T33)
# cost 750 from some level on, tied with every later level.  (A pixel near an image corner can have a level with
# one or two taps inside that happen to cost under 30 each, so under 750 in all: about every second seed of noise_t
# has one to four such pixels among its 17010 -- 23 has four --, this one none.)
CASES["noise_h"] = _case("noise", 3, 1, 160, 24, 200, nh=1)
CASES["noise_t"] = _case("noise", D=130, bl=1.0359, affine=False, seed=25, **T33)
# level lists
CASES["signed_h"] = _case("per12", D=41, levels="signed", **H31)
CASES["desc_h"] = _case("per12", D=70, levels="desc", **H31)
CASES["pairs5_h"] = _case("per12", D=70, levels="pairs5", **H31)
# 70 shuffled levels: with this seed the fifth chunk of 8 holds levels 66 apart (of 16: the second and third, 65 and
# 66), so even the |dx| = 1 neighbours of view 1 need more than 64 columns of shift; 20 shuffled levels: at most 38
CASES["shuf70_h"] = _case("cheap", D=70, levels="shuffled", forms=NEITHER, **H31)
CASES["shuf20_h"] = _case("cheap", D=20, levels="shuffled", **H31)
# half steps: fractional column shifts at |dx| = 1 (gather only), integral at |dx| = 2 (view 1 then has no
# neighbour: no shift at all, a 64-column band that is never staged)
CASES["half_h"] = _case("cheap", D=70, levels="half", forms=NEITHER, **H31)
CASES["half_dx2"] = _case("per12", 3, 1, 120, 40, 70, levels="half", bw64=(1,), lists=sc.dx2_only(3))
# negative levels: every band extent reversed, negative row offsets
CASES["signed_t_bl1"] = _case("p2d12", D=41, levels="signed", **T33)
CASES["signed_t_bl1.0359"] = _case("p2d12", D=41, levels="signed", bl=1.0359, affine=False, **T33)
# bl_ratio 0.5: even levels shift whole rows (affine), unit levels half rows (rows in (-1, 0) truncate to row 0)
CASES["even_bl0.5"] = _case("p2d12", D=20, levels="even", bl=0.5, **T33)
CASES["unit_bl0.5"] = _case("cheap", D=20, bl=0.5, affine=False, **T33)
# vertical neighbours only: no column shift, 64-column bands
CASES["v1x3_bl1"] = _case("p2d12", 1, 3, 70, 40, 40, bw64=(0, 1, 2), nv=2)
CASES["v1x3_signed_bl1"] = _case("p2d12", 1, 3, 70, 40, 40, levels="signed", bw64=(0, 1, 2), nv=2)
CASES["v1x3_bl1.0359"] = _case("p2d12", 1, 3, 70, 40, 40, levels="signed", bl=1.0359, affine=False, bw64=(0, 1, 2),
                               nv=2)
# the order of the colour sum: a level's cost is one pixel's |dL| + |da| + |db|, and the two cheapest are an ulp apart
CASES["assoc_h"] = _case("swap5", 2, 1, 130, 30, 40, nh=1)
# one level; every projection outside the image
CASES["d1"] = _case("cheap", 3, 1, 70, 20, 1, levels="far500", bw64=(0, 1, 2), nh=2)
CASES["far500"] = _case("cheap", 3, 1, 120, 20, 16, levels="far500", nh=2)
# neighbour counts that differ per view; a view without neighbours (its band: 64 columns, never staged)
CASES["rows_a3x2"] = _case("p2d12", 3, 2, 70, 27, 40, lists=sc.rows_then_columns(3, 2))
CASES["empty_t"] = _case("p2d12", D=40, bl=1.0359, affine=False, bw64=(4,), empty=(4,), **T33)
# images below a window (5 x 5) or a tile (60 x 8)
CASES["tiny_1x1"] = _case("cheap", 3, 1, 1, 1, 9, nh=2)
CASES["tiny_3x2"] = _case("cheap", 3, 1, 3, 2, 9, nh=2)
CASES["tiny_5x70"] = _case("cheap", 3, 3, 5, 70, 9, levels="signed", nh=1, nv=1)
CASES["tiny_64x4"] = _case("cheap", 3, 1, 64, 4, 9, nh=2)
# the fourth channel is loaded and must be ignored
CASES["wnan_aff"] = dict(CASES["p2d12_bl1"], wnan=True)
CASES["wnan_tab"] = dict(CASES["p2d12_bl1.0359"], wnan=True)
WNAN_OF = {"wnan_aff": "p2d12_bl1", "wnan_tab": "p2d12_bl1.0359"}


def make(name):
    """The inputs of CASES[name]: dict(lab, levels, vs, sn, V, and the case's own keys)."""
    c = CASES[name]
    V = c["aw"] * c["ah"]
    vs, sn = sc.camera(c["aw"], c["ah"], **c["cam"])
    return dict(c, V=V, lab=lab(c["content"], c["aw"], c["ah"], c["W"], c["H"], c["seed"], c["wnan"]),
                levels=level_list(c["levels"], c["D"]), vs=vs, sn=sn)
