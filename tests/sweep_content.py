"""Built inputs for the superpixel plane sweep (helper, no tests; numpy only).

Every other sweep test feeds the kernels SLIC's own centres and k_boundary's
extents on synth.make_stack images: centres never on the image border, extents
never 0 or S - 1, ascending non-negative integer levels, costs that almost
never tie.  engine.sweep_spixl and orc.sweep take Lab, centres and extents as
plain arrays, so here all three are made by hand:

  geometry()  centres [V, mh, mw, 8] and extents [V, mh, mw, 8] (uint8)
  lab()       Lab contents whose costs tie exactly across far levels, leave
              the image, are flat, or are ordinary
  level_list()  unit, signed, descending, shuffled and half-step level lists
  camera()    neighbour lists of an array
  costs()     orc_sweep's per-level cost restated in numpy float32

CASES names every (content, geometry, level list) the GPU tests run
(tests/test_gpu_sweep_forms.py); tests/test_sweep_content_cpu.py pins the
state each is there for on the oracle alone.  Everything is deterministic in
its arguments."""
from __future__ import annotations

import numpy as np

from cl_multiview_stereo_amd import params

f32 = np.float32
SEED = 23


# ---- centres and extents ---------------------------------------------------
def geometry(V, W, H, S, seed=SEED, rep_all=None):
    """(spixl [V, mh, mw, 8] float32, rep [V, mh, mw, 8] uint8).

    Centres (slots 1, 2): the grid's, with fractional parts from {0, .25, .5,
    .75}; the first and last map column sit on image column 0 and W - 1, the
    first and last map row on image row 0 and H - 1.  Slot 7 is NaN (the
    sweep's output), the other slots random (the sweep must leave them).
    Extents: random in [0, S - 1] with a lattice of all-0 cells (unit tap
    steps) and all-(S - 1) cells (the widest window); rep_all: every extent
    that value instead.  Nothing outside the contract: centres inside the
    image, extents <= S - 1."""
    mw, mh = params.map_size(W, H, S)
    rng = np.random.default_rng([seed, V, W, H, S])
    sp = rng.uniform(-50.0, 50.0, (V, mh, mw, 8)).astype(f32)
    frac = rng.integers(0, 4, (2, V, mh, mw)).astype(f32) * f32(0.25)
    cx = np.minimum((np.arange(mw) * S + S // 2).astype(f32)[None, None, :] + frac[0], f32(W - 1))
    cy = np.minimum((np.arange(mh) * S + S // 2).astype(f32)[None, :, None] + frac[1], f32(H - 1))
    cx[:, :, 0] = 0.0
    cx[:, :, -1] = W - 1
    cy[:, 0, :] = 0.0
    cy[:, -1, :] = H - 1
    sp[..., 1] = cx
    sp[..., 2] = cy
    sp[..., 7] = np.nan
    rep = rng.integers(0, S, (V, mh, mw, 8)).astype(np.uint8)
    cell = np.arange(mh)[:, None] * mw + np.arange(mw)[None, :] + np.arange(V)[:, None, None]
    rep[cell % 5 == 1] = 0
    rep[cell % 5 == 3] = S - 1
    if rep_all is not None:
        rep[:] = rep_all
    return np.ascontiguousarray(sp), np.ascontiguousarray(rep)


# ---- Lab contents ------------------------------------------------------------
def _d0(H):
    """The matching disparity of image row y: one per band of 12 rows."""
    return 3 + 7 * (np.arange(H) // 12)


def _colours(rng, shape):
    """Random Lab colours (L in [0, 100], a and b in [-60, 60]), .w = 0."""
    c = np.zeros(shape + (4,), f32)
    c[..., 0] = rng.uniform(0.0, 100.0, shape)
    c[..., 1] = rng.uniform(-60.0, 60.0, shape)
    c[..., 2] = rng.uniform(-60.0, 60.0, shape)
    return c


def lab(content, aw, ah, W, H, seed=SEED):
    """float32 [V, H, W, 4] with .w = 0, all finite.

    per16 / per64  columns of period p, constant down the rows; view v shifted
                   by vx * d0(y), d0 = 3 + 7 (y // 12): a horizontal neighbour
                   matches the reference at every level congruent to d0 mod p
                   (winners differ per row band), and odd views carry
                   L += 0.75, so tied minima sit above zero.
    p2d16          a 16 x 16 tile shifted by (vx * d0, vy * d0): 2-D arrays.
    flat           one colour everywhere.
    noise          uniform in [-100, 100] per view: an in-image tap costs far
                   more than the 30 of an outside one, so the winner is the
                   first level at which some neighbour's whole window has left
                   the image, cost exactly 25 * 30 = 750.
    cheap          uniform in [0, 20] per view: ordinary distinct minima."""
    V = aw * ah
    rng = np.random.default_rng([seed, sum(map(ord, content)), W, H])
    vx = (np.arange(V) % aw)[:, None, None]
    vy = (np.arange(V) // aw)[:, None, None]
    y = np.arange(H)[None, :, None]
    x = np.arange(W)[None, None, :]
    d0 = _d0(H)[None, :, None]
    if content in ("per16", "per64"):
        p = int(content[3:])
        out = _colours(rng, (p,))[(x + vx * d0) % p]
        out[1::2, :, :, 0] += f32(0.75)
    elif content == "p2d16":
        out = _colours(rng, (16, 16))[(y + vy * d0) % 16, (x + vx * d0) % 16]
    elif content == "flat":
        out = np.zeros((V, H, W, 4), f32)
        out[..., :3] = (f32(41.5), f32(-7.25), f32(12.0))
    elif content == "noise":
        out = np.zeros((V, H, W, 4), f32)
        out[..., :3] = rng.uniform(-100.0, 100.0, (V, H, W, 3))
    elif content == "cheap":
        out = np.zeros((V, H, W, 4), f32)
        out[..., :3] = rng.uniform(0.0, 20.0, (V, H, W, 3))
    else:
        raise ValueError(content)
    out = np.ascontiguousarray(out, f32)
    assert out.shape == (V, H, W, 4) and np.isfinite(out).all() and not out[..., 3].any()
    return out


# ---- level lists -------------------------------------------------------------
def level_list(kind, D, seed=SEED):
    """float32 [D]: "unit" 0 .. D - 1, "pairs5" 5, 5, 6, 6, ... (every level
    twice, none 0: whatever the content, levels 2 k and 2 k + 1 cost the same),
    "signed" centred on zero (dmin < 0), "desc" D - 1 .. 0, "shuffled" a seeded
    permutation of the unit list, "half" 0.5 k."""
    k = np.arange(D)
    if kind == "unit":
        lv = k
    elif kind == "pairs5":
        lv = k // 2 + 5
    elif kind == "signed":
        lv = k - D // 2
    elif kind == "desc":
        lv = k[::-1]
    elif kind == "shuffled":
        lv = np.random.default_rng([seed, D, 7]).permutation(D)
    elif kind == "half":
        lv = 0.5 * k
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(lv, f32)


def camera(aw, ah, nh=0, nv=0, knn=None, lists=None, empty=()):
    """(view_subset [V, V], subset_num [V]): the reference's neighbour lists
    (nh, nv), the knn nearest neighbours, or hand-made `lists`; the views in
    `empty` get no neighbour at all."""
    if lists is None:
        lists = params.nearest_neighbours(aw, ah, knn) if knn else params.neighbour_lists(aw, ah, nh, nv)
    lists = [[] if z in empty else list(l) for z, l in enumerate(lists)]
    return params.flatten_subsets(lists)


def dx2_only(aw):
    """Hand-made lists of a aw x 1 array: only the neighbours two cameras away."""
    return [[v for v in (z - 2, z + 2) if 0 <= v < aw] for z in range(aw)]


def rows_then_columns(aw=3, ah=2):
    """Hand-made lists of a aw x 2 array: the first camera row lists its
    horizontal neighbours only, the second also the camera above."""
    out = []
    for z in range(aw * ah):
        zx, zy = z % aw, z // aw
        l = [zy * aw + v for v in range(aw) if v != zx]
        out.append(l + [zx] if zy == 1 else l)
    return out


# ---- the per-level cost, restated ---------------------------------------------
def costs(lab, spixl, rep, levels, vs, sn, aw, bl, z):
    """orc_sweep's cost (oracle/mvs_oracle.c, initial_depth_estimation_v2) of
    reference view z, op for op in float32, vectorised over superpixels and
    levels: (cost [M, D] float32 -- the minimum over neighbours, 1e6 with an
    empty list --, ntap [M, D] -- the in-image taps of the first neighbour
    that attains it, 0 with an empty list --, frac [M, D] bool -- some
    in-image tap of any neighbour has xr - d dx in (-1, 0), truncated to
    column 0).  levels[first argmin of cost] is the oracle's winner (0.0 where
    no cost is below 1e6)."""
    lab = np.asarray(lab, f32)
    V, H, W = lab.shape[:3]
    levels = np.asarray(levels, f32)
    D = len(levels)
    vs = np.asarray(vs).reshape(V, V)
    sp = np.asarray(spixl, f32)[z].reshape(-1, 8)
    dr = np.asarray(rep)[z].reshape(-1, 8).astype(np.int64)
    M = sp.shape[0]
    bl_ = np.maximum(dr[:, 0], np.maximum(dr[:, 1], dr[:, 2]))
    br_ = np.maximum(dr[:, 5], np.maximum(dr[:, 6], dr[:, 7]))
    bt_ = np.maximum(dr[:, 0], np.maximum(dr[:, 3], dr[:, 5]))
    bb_ = np.maximum(dr[:, 2], np.maximum(dr[:, 4], dr[:, 7]))
    # (float)fmax(1.0, 0.25 * (double)(float)(bl_ + br_))
    stx = np.maximum(1.0, 0.25 * (bl_ + br_).astype(f32).astype(np.float64)).astype(f32)
    sty = np.maximum(1.0, 0.25 * (bt_ + bb_).astype(f32).astype(np.float64)).astype(f32)
    cx, cy = sp[:, 1], sp[:, 2]
    rx, ry = z % aw, z // aw
    d = levels[None, :]
    bld = f32(bl) * d
    cost = np.full((M, D), f32(1000000.0), f32)
    ntap = np.zeros((M, D), np.int64)
    frac = np.zeros((M, D), bool)
    k30 = f32(30.0)
    nn = int(sn[z])
    if nn == 0:
        return cost, ntap, frac
    view = vs[z, :nn].astype(np.int64)[:, None, None]  # every neighbour at once: [nn, M, D]
    fdx = d[None] * (view % aw - rx).astype(f32)
    fdy = bld[None] * (view // aw - ry).astype(f32)
    val = np.zeros((nn, M, D), f32)
    cnt = np.zeros((nn, M, D), np.int64)
    for i in range(-2, 3):
        for j in range(-2, 3):
            xr = np.trunc(cx + f32(i) * stx).astype(np.int64)[None, :, None]
            yr = np.trunc(cy + f32(j) * sty).astype(np.int64)[None, :, None]
            fx = xr.astype(f32) - fdx
            xp = np.trunc(fx).astype(np.int64)
            yp = np.trunc(yr.astype(f32) - fdy).astype(np.int64)
            val = val + k30
            ok = (xr >= 0) & (yr >= 0) & (xp >= 0) & (yp >= 0) & (xr < W) & (yr < H) & (xp < W) & (yp < H)
            a = lab[z, np.clip(yr, 0, H - 1), np.clip(xr, 0, W - 1)]
            b = lab[view, np.clip(yp, 0, H - 1), np.clip(xp, 0, W - 1)]
            ad = np.abs(a[..., 0] - b[..., 0]) + np.abs(a[..., 1] - b[..., 1])
            ad = ad + np.abs(a[..., 2] - b[..., 2])
            val = np.where(ok, (val - k30) + ad, val)
            cnt += ok
            frac |= (ok & (fx < 0)).any(0)
    for n in range(nn):  # the oracle's strict-< scan over the neighbours
        take = val[n] < cost
        cost = np.where(take, val[n], cost)
        ntap = np.where(take, cnt[n], ntap)
    assert cost.dtype == f32
    return cost, ntap, frac


def winners(cost, levels):
    """The oracle's scan: the first level of strictly lowest cost, 0.0 if none is below 1e6."""
    levels = np.asarray(levels, f32)
    best = cost.min(1)
    return np.where(best < f32(1000000.0), levels[cost.argmin(1)], f32(0.0)).astype(f32)


# ---- the cases the GPU tests run ------------------------------------------------
def _case(content, aw, ah, W, H, S, D, levels="unit", bl=1.0, rep_all=None, **cam):
    return dict(content=content, aw=aw, ah=ah, W=W, H=H, S=S, D=D, levels=levels, bl=bl, rep_all=rep_all, cam=cam)


CASES = {}
# every form on one horizontal input: the 5 x 1 array, every other view a neighbour
for _c in ("per64", "per16"):
    for _D in (33, 64, 65, 130, 200):
        CASES[f"h5_{_c}_d{_D}"] = _case(_c, 5, 1, 160, 48, 16, _D, nh=4)
# staging windows under 64 columns (14 + 2 + 32 + 1), and windows clipped by a 48-column image
CASES["h3_s8_per16_d33"] = _case("per16", 3, 1, 160, 48, 8, 33, nh=1)
CASES["h5_w48_per16_d70"] = _case("per16", 5, 1, 48, 48, 16, 70, nh=4)
# the ring's window bound: 2 (S - 1) + 2 + 63 * 3 + 1 = 336 at S = 73 (its last fit), 338 at S = 74;
# S = 48 on the 5 x 1 array: 94 + 2 + 252 + 1 = 349
for _c in ("per16", "cheap"):
    CASES[f"bound_s73_{_c}"] = _case(_c, 4, 1, 420, 80, 73, 70, rep_all=72, nh=3)
    CASES[f"bound_s74_{_c}"] = _case(_c, 4, 1, 420, 80, 74, 70, rep_all=73, nh=3)
CASES["bound_s48_per16"] = _case("per16", 5, 1, 200, 60, 48, 130, nh=4)
CASES["bound_s48_per64"] = _case("per64", 5, 1, 200, 60, 48, 130, nh=4)
# D <= 32: two superpixels per wave, 9 x 3 = 27 superpixels (the last half-wave idle)
for _D in (1, 2, 31, 32):
    CASES[f"half_h_d{_D}"] = _case("per16", 5, 1, 144, 48, 16, _D, nh=4)
    CASES[f"half_t_d{_D}"] = _case("p2d16", 3, 3, 144, 48, 16, _D, nh=1, nv=1)
# level lists: the 3 x 1 array, both other views neighbours
for _c in ("cheap", "per16"):
    CASES[f"lv_signed_{_c}"] = _case(_c, 3, 1, 120, 40, 8, 41, levels="signed", nh=2)
    CASES[f"lv_desc_{_c}"] = _case(_c, 3, 1, 120, 40, 8, 70, levels="desc", nh=2)
    CASES[f"lv_shuffled_{_c}"] = _case(_c, 3, 1, 120, 40, 8, 70, levels="shuffled", nh=2)
    CASES[f"lv_half_{_c}"] = _case(_c, 3, 1, 120, 40, 8, 70, levels="half", nh=2)
    CASES[f"lv_half_dx2_{_c}"] = _case(_c, 3, 1, 120, 40, 8, 70, levels="half", lists=dx2_only(3))
# 2-D arrays: vertical and diagonal neighbours, image sizes off the 32 x 32 relayout tiles
SIZES_2D = {"150x45": (150, 45, 16), "70x27": (70, 27, 8), "45x100": (45, 100, 16)}
for _a, _kw in (("a3x3", dict(aw=3, ah=3, nh=1, nv=1)), ("a8x4", dict(aw=8, ah=4, knn=5))):
    for _c in ("p2d16", "cheap"):
        for _bl in (1.0, 1.0359):
            for _D in (32, 130, 200):
                for _sz, (_W, _H, _S) in SIZES_2D.items():
                    _kw2 = dict(_kw)
                    CASES[f"{_a}_{_c}_bl{_bl}_d{_D}_{_sz}"] = _case(_c, _kw2.pop("aw"), _kw2.pop("ah"), _W, _H, _S, _D,
                                                                   bl=_bl, **_kw2)
# a 3 x 2 array whose first camera row lists horizontal neighbours only
CASES["a3x2_rows"] = _case("p2d16", 3, 2, 150, 45, 16, 70, lists=rows_then_columns(3, 2))
# degenerate content, and a reference view without neighbours (view 1)
CASES["flat_h"] = _case("flat", 5, 1, 160, 48, 16, 70, levels="pairs5", nh=4)
CASES["flat_t"] = _case("flat", 3, 3, 70, 27, 8, 70, levels="pairs5", nh=1, nv=1)
CASES["noise_h"] = _case("noise", 5, 1, 160, 48, 16, 130, nh=4)
CASES["noise_t"] = _case("noise", 3, 3, 70, 27, 8, 130, nh=1, nv=1)
# 300 levels: a wave holds levels 64 apart in turn (wave h of w: 64 (h + w p) ..), so a later wave can hold the
# FIRST of tied levels while wave 0 holds a later one.  Only |dx| = 1 (and |dy| = 1) neighbours: a window has left
# the image from a level between 64 and 128 on for the superpixels in the middle, and ties with every level after
CASES["merge_h"] = _case("noise", 3, 1, 160, 48, 16, 300, nh=1)
CASES["merge_t"] = _case("noise", 3, 3, 150, 150, 16, 300, nh=1, nv=1)
CASES["empty_h"] =_case("per16", 5, 1, 160, 48, 16, 70, nh=4, empty=(1,))
CASES["empty_t"] = _case("p2d16", 3, 3, 70, 27, 8, 70, nh=1, nv=1, empty=(1,))


def make(name):
    """The inputs of CASES[name]: dict(lab, spixl, rep, levels, vs, sn, V, and the case's own keys)."""
    c = CASES[name]
    V = c["aw"] * c["ah"]
    sp, rep = geometry(V, c["W"], c["H"], c["S"], rep_all=c["rep_all"])
    vs, sn = camera(c["aw"], c["ah"], **c["cam"])
    return dict(c, V=V, lab=lab(c["content"], c["aw"], c["ah"], c["W"], c["H"]), spixl=sp, rep=rep,
                levels=level_list(c["levels"], c["D"]), vs=vs, sn=sn)
