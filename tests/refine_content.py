"""Built inputs for the superpixel-plane refinement (helper, no tests; numpy only).

Every other refinement test feeds k_init_state, k_propagate and
k_spixl_to_image{,4} SLIC's centres, k_boundary's extents, the integer-level
sweep's disparities and the reference's kernel-size schedule on
synth.make_stack scenes.  The stage entry points take spixl, labels, rep and
the schedule as plain values, so here they are made by hand:

  colour()     slots 3..5 over the superpixel map: smooth, flat, far, graded,
               tile3
  disparity()  slot 7: half (k + 0.5), signed, wide, plane, huge
  label_map()  the S-grid, or a mixed map (a random cell of the pixel's 3 x 3
               block of cells; 2 % any cell of the view)
  cameras()    3 x 1, 3 x 3, and a 4 x 3 array with hand-made lists of 0, 3, 8,
               9 and 11 neighbours
  schedule()   the reference's (params.refine_params / prop_schedule) or a
               dense one: nks far steps of kss cells, iterations 0 and 4

centres and extents are tests.sweep_content.geometry()'s (fractional centres,
border centres on column / row 0 and W - 1 / H - 1, extents 0 .. S - 1),
neighbour lists tests.sweep_content.camera()'s.  Two restatements, written from
the reference's formulas (oracle/mvs_oracle.c cites the lines), not from the
kernel: term_counts() -- per cell the valid smoothness terms and the valid
plane candidates -- and init_pixels() -- per (cell, neighbour, sample) the
pixel init_consistency reads, under round-half-away and round-half-even.

Contract: every input finite, labels < mw * mh, |d * dx| < 2^24.

CASES names every (colour, disparity, labels, camera, map, schedule) the GPU
tests run (tests/test_gpu_refine_content.py); tests/test_refine_content_cpu.py
pins the state each is there for on the oracle alone.  oracle_stages() runs
the oracle over a case's schedule once per process, for both.  Everything is
deterministic in its arguments."""
from __future__ import annotations

import functools

import numpy as np

from cl_multiview_stereo_amd import params
from tests import sweep_content as sc

f32 = np.float32
SEED = 29
HUGE = 100000.0  # |HUGE * dx| <= 3e5 < 2^24, and no image here is 1e5 pixels wide
PLANE = (0.05, -0.03, 6.0)  # d = a cx + b cy + c


def _rng(*key):
    return np.random.default_rng([SEED] + [sum(map(ord, k)) if isinstance(k, str) else int(k) for k in key])


# ---- slots 3..5 ---------------------------------------------------------------
def colour(kind, V, mh, mw):
    """float32 [V, mh, mw, 3].
    smooth  uniform in [0, 3]: every similarity well above zero.
    flat    one colour: every similarity 1, flatness exp(-1/8).
    far     uniform in [-100, 100]: every similarity 0, so wn == 0.
    graded  (25.3 x, 25.3 y, 0) + uniform [-0.5, 0.5]: horizontal and vertical
            neighbours about 25 Lab units apart (simi about mvs_expf(-80), a
            tiny normal number; some below 1e-37), diagonal ones 36 (simi 0).
    tile3   nine colours 60 or more apart, chosen by (x mod 3, y mod 3): the
            cells 3 apart along a row or column share a colour exactly, every
            cell nearer than that is far.  With one far step of kss = 2.5 the
            far plane candidates sit 3 cells away (simi == 1) while the far
            smoothness terms sit 2 away (flatness 0, step 1): wn == 0, every
            sm is 0.000001f, and such a candidate's sm * simi EQUALS the
            current sm -- the strict > of the accept test decides."""
    rng = _rng("colour", kind, V, mh, mw)
    if kind == "smooth":
        out = rng.uniform(0.0, 3.0, (V, mh, mw, 3))
    elif kind == "flat":
        out = np.broadcast_to(np.array([41.5, -7.25, 12.0]), (V, mh, mw, 3))
    elif kind == "far":
        out = rng.uniform(-100.0, 100.0, (V, mh, mw, 3))
    elif kind == "graded":
        out = rng.uniform(-0.5, 0.5, (V, mh, mw, 3))
        out[..., 0] += 25.3 * np.arange(mw)[None, None, :]
        out[..., 1] += 25.3 * np.arange(mh)[None, :, None]
    elif kind == "tile3":
        nine = np.array([[60.0 * (k % 3), 60.0 * (k // 3) - 60.0, 25.0 * k - 100.0] for k in range(9)])
        out = np.broadcast_to(nine[(np.arange(mh)[:, None] % 3) * 3 + np.arange(mw)[None, :] % 3], (V, mh, mw, 3))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(out, f32)


# ---- slot 7 --------------------------------------------------------------------
def disparity(kind, spixl):
    """float32 [V, mh, mw] for the centres of `spixl`.
    half    k + 0.5, k in 0..7, per cell and view: with |dx| = 1, d * dx is a
            half-way shift.
    signed  integers in [-6, 6].
    wide    integers in [-20, 20]: neighbours up to 40 levels apart, so that
            exp(-diff^2 alpha) falls to 1e-10 and a product with a tiny simi
            is subnormal.
    plane   a cx + b cy + c, the same in all views.
    huge    one constant that takes every sample of every neighbour off the image."""
    shape = spixl.shape[:3]
    rng = _rng("disparity", kind, *shape)
    if kind == "half":
        out = rng.integers(0, 8, shape) + 0.5
    elif kind == "signed":
        out = rng.integers(-6, 7, shape)
    elif kind == "wide":
        out = rng.integers(-20, 21, shape)
    elif kind == "plane":
        a, b, c = (f32(v) for v in PLANE)
        out = a * spixl[..., 1] + b * spixl[..., 2] + c
    elif kind == "huge":
        out = np.full(shape, HUGE)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(out, f32)


# ---- labels ----------------------------------------------------------------------
def grid_labels(V, W, H, S):
    """init_label_per_pixl (orc.grid's labels): mw (y / S) + x / S."""
    mw, _ = params.map_size(W, H, S)
    lb = mw * (np.arange(H) // S)[:, None] + (np.arange(W) // S)[None, :]
    return np.ascontiguousarray(np.broadcast_to(lb, (V, H, W)), np.uint32)


def label_map(kind, V, W, H, S):
    """uint32 [V, H, W], every label < mw * mh.  "grid": the S-grid.  "mixed":
    each pixel takes a random cell of its own 3 x 3 block of cells (clipped to
    the map), and about 2 % of the pixels any cell of the view."""
    if kind == "grid":
        return grid_labels(V, W, H, S)
    if kind != "mixed":
        raise ValueError(kind)
    mw, mh = params.map_size(W, H, S)
    rng = _rng("labels", V, W, H, S)
    gx = np.clip((np.arange(W) // S)[None, None, :] + rng.integers(-1, 2, (V, H, W)), 0, mw - 1)
    gy = np.clip((np.arange(H) // S)[None, :, None] + rng.integers(-1, 2, (V, H, W)), 0, mh - 1)
    lb = gy * mw + gx
    anyc = rng.random((V, H, W)) < 0.02
    lb[anyc] = rng.integers(0, mw * mh, int(anyc.sum()))
    return np.ascontiguousarray(lb, np.uint32)


# ---- cameras ----------------------------------------------------------------------
L43_COUNTS = (3, 8, 0, 8, 3, 8, 9, 11, 9, 3, 11, 8)  # views 0..5: at most 8 neighbours; the array's maximum 11
L43_LOW = (0, 6)


def lists_4x3():
    """Hand-made lists of a 4 x 3 array: view z lists its L43_COUNTS[z] nearest views."""
    return [params.nearest_neighbours(4, 3, n)[z] if n else [] for z, n in enumerate(L43_COUNTS)]


CAMERAS = {
    "c3x1": dict(aw=3, ah=1, bl=1.0, cam=dict(nh=2)),
    "c3x1_empty1": dict(aw=3, ah=1, bl=1.0, cam=dict(nh=2, empty=(1,))),
    "c3x3": dict(aw=3, ah=3, bl=1.0359, cam=dict(nh=1, nv=1)),  # the middle view: exactly 8 neighbours
    "l4x3": dict(aw=4, ah=3, bl=1.0359, cam=dict(lists=lists_4x3())),
}

MAPS = {  # W, H, S
    "m32": (256, 256, 8),    # 32 x 32: every far term of nks = 13 valid for the central cells
    "m13x9": (100, 70, 8),   # V * M no multiple of 4, W % 4 == 0
    "m9x3": (131, 37, 16),   # W % 4 != 0: the one-pixel fusion kernel
    "m1x1": (8, 8, 8), "m5x1": (40, 8, 8), "m1x5": (8, 40, 8), "m2x2": (16, 16, 8),
}


# ---- schedules ----------------------------------------------------------------------
def schedule(kind, S):
    """dict(rp: params.refine_params' scalars, init: (nks, kss) of init_state,
    props: [(iter, nks, kss)] of the propagate calls, each on the one before's
    output).  "ref": the reference's five iterations.  ("dense", nks, kss):
    iteration 0, then iteration 4 (which switches off the `iter < 4` half of
    the accept tests) on its output, both with nks far steps of kss cells."""
    rp = params.refine_params(params.Settings(spixl_size=S))
    if kind == "ref":
        props = [(it,) + params.prop_schedule(it, rp["kernel_steps"], rp["kss"]) for it in range(5)]
        return dict(rp=rp, init=(rp["kernel_steps"], rp["kss"]), props=props)
    _, nks, kss = kind
    return dict(rp=rp, init=(nks, float(kss)), props=[(0, nks, float(kss)), (4, nks, float(kss))])


# ---- the restatements -----------------------------------------------------------------
def step_size_of(flx, kss):
    """(int)((double)(flx * kss) + 0.5), at least 1 (clcode.cl compute_smoothness)."""
    s = ((np.asarray(flx, f32) * f32(kss)).astype(np.float64) + 0.5).astype(np.int64)
    return np.maximum(s, 1)


def _far(pos, n, step, nks):
    """How many of the far steps i = 1..nks reach a cell at pos - (i step + 1) and at pos + (i step + 1)."""
    st = np.arange(1, nks + 1).reshape((nks,) + (1,) * np.ndim(pos)) * step
    return ((pos > st).astype(np.int64) + (pos < n - st - 1)).sum(0)


def term_counts(flat0, nks, kss):
    """(nvt, nvalid), int [.., mh, mw]: per cell the valid smoothness terms of
    compute_smoothness (the in-map 8-neighbours, then left / right / up / down
    at i * step_size_of(flat0, kss) + 1 cells, i = 1..nks) and the valid plane
    candidates of propagate (the same with the step (int)kss)."""
    flat0 = np.asarray(flat0, f32)
    mh, mw = flat0.shape[-2:]
    x = np.broadcast_to(np.arange(mw)[None, :], flat0.shape)
    y = np.broadcast_to(np.arange(mh)[:, None], flat0.shape)
    nx = (x > 0).astype(np.int64) + (x < mw - 1) + 1
    ny = (y > 0).astype(np.int64) + (y < mh - 1) + 1
    n8 = nx * ny - 1
    ss = step_size_of(flat0, kss)
    ssz = int(kss)
    nvt = n8 + _far(x, mw, ss, nks) + _far(y, mh, ss, nks)
    nvalid = n8 + _far(x, mw, ssz, nks) + _far(y, mh, ssz, nks)
    return nvt, nvalid


def round_half_away(v):
    v = np.asarray(v, f32).astype(np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(f32)


def round_half_even(v):
    return np.rint(np.asarray(v, f32))


def init_pixels(m, z):
    """initialize_consistency's sample geometry for reference view z:
    dict(views [nn], xr, yr int [M, 9] (the sample in the reference view; sample
    t = 3 (i + 1) + (j + 1), i the x direction), and for each tie rule r in
    ("ha", "he") xp_r, yp_r int [nn, M, 9] (the pixel read in neighbour n) and
    in_r bool (it lies in the image))."""
    W, H, aw = m["W"], m["H"], m["aw"]
    sp = m["spixl"][z].reshape(-1, 8)
    rep = m["rep"][z].reshape(-1, 8).astype(np.int64)
    smp = np.concatenate([rep[:, :4], np.zeros((len(rep), 1), np.int64), rep[:, 4:]], 1)
    t = np.arange(9)
    xr = np.trunc(sp[:, 1]).astype(np.int64)[:, None] + smp * (t // 3 - 1)[None, :]
    yr = np.trunc(sp[:, 2]).astype(np.int64)[:, None] + smp * (t % 3 - 1)[None, :]
    nn = int(m["sn"][z])
    views = np.asarray(m["vs"]).reshape(m["V"], m["V"])[z, :nn].astype(np.int64)
    d = sp[:, 7][None, :, None]
    fdx = d * (views % aw - z % aw).astype(f32)[:, None, None]
    fdy = (f32(m["bl"]) * d) * (views // aw - z // aw).astype(f32)[:, None, None]
    out = dict(views=views, xr=xr, yr=yr)
    for r, rnd in (("ha", round_half_away), ("he", round_half_even)):
        xp = np.trunc(xr.astype(f32)[None] - rnd(fdx)).astype(np.int64)
        yp = np.trunc(yr.astype(f32)[None] - rnd(fdy)).astype(np.int64)
        out["xp_" + r], out["yp_" + r] = xp, yp
        out["in_" + r] = (xp >= 0) & (yp >= 0) & (xp < W) & (yp < H)
    return out


# ---- the cases the GPU tests run --------------------------------------------------------
def _case(colour, disp, labels, camera, map_, sched):
    return dict(colour=colour, disp=disp, labels=labels, camera=camera, map=map_, sched=sched)


def _dense(nks, kss):
    return ("dense", nks, kss)


CASES = {
    # dense far terms on the 32 x 32 map: all 8 + 4 nks terms and candidates valid for the central cells (kss 1.0),
    # every lane layout of the last candidate group; nks 13 (the last FAST, 61 terms) against 14 (65 terms: one
    # lane per candidate) and 16; kss 2.5: candidates every 2 cells, terms every 1 (smooth) or 2 (flat) cells
    "dense_n0_k1": _case("smooth", "plane", "mixed", "c3x1", "m32", _dense(0, 1.0)),
    "dense_n1_k25": _case("smooth", "plane", "mixed", "c3x1", "m32", _dense(1, 2.5)),
    "dense_n13_k1": _case("smooth", "plane", "mixed", "c3x3", "m32", _dense(13, 1.0)),
    "dense_n13_k25": _case("flat", "half", "grid", "c3x1", "m32", _dense(13, 2.5)),
    "dense_n14_k1": _case("smooth", "plane", "mixed", "c3x1", "m32", _dense(14, 1.0)),
    "dense_n14_k25": _case("smooth", "plane", "mixed", "c3x1", "m32", _dense(14, 2.5)),
    "dense_n16_k1": _case("smooth", "signed", "mixed", "c3x1", "m32", _dense(16, 1.0)),
    "dense_n16_k25": _case("flat", "plane", "grid", "c3x1", "m32", _dense(16, 2.5)),
    # rounding ties: |dx| = 1 and d = k + 0.5 (the 3 x 3 array: the lane-parallel path, 8 neighbours)
    "half_3x3": _case("smooth", "half", "mixed", "c3x3", "m13x9", "ref"),
    "half_w131": _case("smooth", "half", "mixed", "c3x1", "m9x3", "ref"),
    # the 4 x 3 lists (0, 3, 8, 9, 11 neighbours): FAST for views [0, 6) alone, the per-wave choice for the rest;
    # with half-way shifts in the one-lane-per-candidate consistency too
    "l4x3_plane": _case("smooth", "plane", "mixed", "l4x3", "m13x9", "ref"),
    "l4x3_half": _case("smooth", "half", "mixed", "l4x3", "m13x9", "ref"),
    "l4x3_dense": _case("smooth", "signed", "mixed", "l4x3", "m13x9", _dense(13, 1.0)),
    # empty consistency: a view without neighbours; every sample off the image
    "empty_view": _case("smooth", "plane", "mixed", "c3x1_empty1", "m13x9", "ref"),
    "huge": _case("smooth", "huge", "mixed", "c3x1", "m13x9", "ref"),
    # underflow: every simi 0 (wn == 0); simi about 1e-35 (wn tiny, subnormal products)
    "far": _case("far", "signed", "grid", "c3x1", "m13x9", "ref"),
    # equality in the plane accept tests: sm 0.000001f on both sides and cs the margin on both sides (far colours,
    # view 1 without neighbours); sm * simi == the current sm (tile3)
    "far_empty": _case("far", "signed", "mixed", "c3x1_empty1", "m13x9", "ref"),
    "tile3": _case("tile3", "signed", "mixed", "c3x1", "m13x9", _dense(1, 2.5)),
    "graded": _case("graded", "wide", "grid", "c3x1", "m13x9", "ref"),
    "graded_n0": _case("graded", "wide", "mixed", "c3x1", "m13x9", _dense(0, 1.0)),
    "graded_dense": _case("graded", "signed", "mixed", "c3x1", "m13x9", _dense(13, 1.0)),
    # signed disparities at border centres; W % 4 != 0
    "signed": _case("smooth", "signed", "mixed", "c3x1", "m13x9", "ref"),
    "signed_w131": _case("smooth", "signed", "mixed", "c3x3", "m9x3", "ref"),
    "plane_w131": _case("smooth", "plane", "mixed", "c3x1", "m9x3", "ref"),
    # tiny maps: no 8-neighbour (1 x 1), no valid triangle (5 x 1, 1 x 5), the smallest map with one (2 x 2)
    "tiny_1x1": _case("smooth", "signed", "grid", "c3x1", "m1x1", "ref"),
    "tiny_5x1": _case("smooth", "plane", "mixed", "c3x1", "m5x1", "ref"),
    "tiny_1x5": _case("smooth", "half", "mixed", "c3x1", "m1x5", "ref"),
    "tiny_2x2": _case("smooth", "signed", "mixed", "c3x1", "m2x2", "ref"),
    "tiny_5x1_dense": _case("smooth", "signed", "grid", "c3x1", "m5x1", _dense(13, 1.0)),
}
DENSE_M32 = [n for n, c in CASES.items() if c["map"] == "m32"]


@functools.lru_cache(maxsize=None)
def make(name):
    """The inputs of CASES[name]: dict(spixl, labels, rep, vs, sn, V, W, H, S, mw, mh, aw, ah, bl, rp, init,
    props, and the case's own keys).  Cached: treat the arrays as read-only."""
    c = CASES[name]
    cam = CAMERAS[c["camera"]]
    W, H, S = MAPS[c["map"]]
    V = cam["aw"] * cam["ah"]
    mw, mh = params.map_size(W, H, S)
    sp, rep = sc.geometry(V, W, H, S)
    sp[..., 3:6] = colour(c["colour"], V, mh, mw)
    sp[..., 7] = disparity(c["disp"], sp)
    labels = label_map(c["labels"], V, W, H, S)
    vs, sn = sc.camera(cam["aw"], cam["ah"], **cam["cam"])
    assert np.isfinite(sp).all() and labels.max() < mw * mh and rep.max() <= S - 1
    assert np.abs(sp[..., 7]).max() * max(cam["aw"], cam["ah"]) * 1.04 < 2 ** 24
    out = dict(c, V=V, W=W, H=H, S=S, mw=mw, mh=mh, aw=cam["aw"], ah=cam["ah"], bl=cam["bl"], spixl=sp, labels=labels,
               rep=rep, vs=vs, sn=sn, **schedule(c["sched"], S))
    for a in (sp, labels, rep, vs, sn):
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_stages(name):
    """The oracle's stages of a case, computed once per process: dict(flat, state0, states: one per entry of
    props, disp: spixl_to_image of the last state)."""
    from oracle import oracle as orc
    m = make(name)
    rp, S = m["rp"], m["S"]
    geo = (m["vs"], m["sn"], m["aw"], m["bl"], S)
    flat = orc.flatness(m["spixl"], rp["flat_gamma"])
    st0 = orc.init_state(m["spixl"], m["labels"], m["rep"], flat, *geo, rp["init_gamma"], rp["init_alpha"],
                         m["init"][0], m["init"][1], rp["fuse"])
    states, cur = [], st0
    for it, nks, kss in m["props"]:
        cur = orc.propagate(m["spixl"], m["labels"], m["rep"], flat, *geo, it, rp["prop_alpha"], rp["prop_gamma"],
                            rp["fuse"], nks, kss, cur)
        states.append(cur)
    disp = orc.spixl_to_image(m["spixl"], m["labels"], cur, S)
    return dict(flat=flat, state0=st0, states=states, disp=disp)
