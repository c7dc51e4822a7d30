"""The built refinement inputs (tests/refine_content.py) reach the states they
are there for -- on the oracle alone, so that the GPU tests built on them
(tests/test_gpu_refine_content.py) cannot go vacuous.

For every case orc.flatness, orc.init_state, every orc.propagate output and
orc.spixl_to_image are finite (the bit comparison is never about NaN
payloads).  Then the state of each family: half-way shifts that change what is
summed, all 8 + 4 nks smoothness terms and plane candidates valid and every
lane layout of the last candidate group, accepted planes and triangles,
wn == 0 and wn tiny with subnormal products, empty consistency, tiny maps,
samples brought back into the image by a signed shift, the 4 x 3 lists' counts.
The shares asserted are conditions fixed beforehand; the values observed on
these seeds are in the docstrings."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from cl_multiview_stereo_amd import params
from oracle import oracle as orc
from tests import refine_content as rc

f32 = np.float32
SM_NONE = f32(0.000001)  # compute_smoothness with wn == 0
CS_NONE = f32(0.01)      # compute_consistency's margin: no view counted


def _expf(x):
    fn = orc.lib().orc_dm_expf
    fn.restype, fn.argtypes = C.c_float, [C.c_float]
    return f32(fn(C.c_float(float(x))))


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- every case -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rc.CASES))
def test_inputs_are_inside_the_contract_and_the_oracle_stays_finite(name):
    m, o = rc.make(name), rc.oracle_stages(name)
    mw, mh, W, H, S = m["mw"], m["mh"], m["W"], m["H"], m["S"]
    assert (mw, mh) == orc.map_size(W, H, S)
    assert m["spixl"].dtype == f32 and np.isfinite(m["spixl"]).all()
    assert m["labels"].dtype == np.uint32 and m["labels"].shape == (m["V"], H, W) and m["labels"].max() < mw * mh
    assert m["rep"].dtype == np.uint8 and m["rep"].max() <= S - 1
    cx, cy = m["spixl"][..., 1], m["spixl"][..., 2]
    assert (cx >= 0).all() and (cx <= W - 1).all() and (cy >= 0).all() and (cy <= H - 1).all()
    assert (cx[:, :, -1] == W - 1).all() and (cy[:, -1, :] == H - 1).all()
    mdx = max(m["aw"], m["ah"]) - 1
    assert float(np.abs(m["spixl"][..., 7]).max()) * max(mdx, 1) * 1.0359 < 2 ** 24
    assert len(o["states"]) == len(m["props"])
    for k, a in [("flat", o["flat"]), ("state0", o["state0"]), ("disp", o["disp"])] + list(enumerate(o["states"])):
        assert np.isfinite(a).all(), (name, k)
    assert o["disp"].shape == (m["V"], H, W)


def test_inputs_are_deterministic():
    for name in ("dense_n13_k1", "l4x3_half", "graded"):
        a = rc.make(name)
        rc.make.cache_clear()
        b = rc.make(name)
        assert a is not b
        for k in ("spixl", "labels", "rep", "vs", "sn"):
            assert np.array_equal(a[k], b[k]), (name, k)


def test_grid_labels_are_the_oracles_and_mixed_labels_mix():
    """The restated S-grid equals orc.grid's labels.  In a mixed map a pixel's
    label is its own grid cell for about one pixel in nine (observed 0.146 on
    the 13 x 9 map, borders clip) and lies outside its 3 x 3 block of cells for
    about 2 % (observed 0.018)."""
    for W, H, S in (rc.MAPS["m13x9"], rc.MAPS["m9x3"], rc.MAPS["m2x2"]):
        _, _, lb = orc.grid(np.zeros((H, W, 4), np.uint8), S)
        assert np.array_equal(rc.grid_labels(2, W, H, S), np.stack([lb, lb]))
    W, H, S = rc.MAPS["m13x9"]
    mw, _ = params.map_size(W, H, S)
    g, mix = rc.grid_labels(3, W, H, S).astype(np.int64), rc.label_map("mixed", 3, W, H, S).astype(np.int64)
    own = float((g == mix).mean())
    out = float(((np.abs(g % mw - mix % mw) > 1) | (np.abs(g // mw - mix // mw) > 1)).mean())
    assert 0.08 <= own <= 0.20 and 0.005 <= out <= 0.03, (own, out)


def test_colour_fields_give_the_similarities_they_are_named_for():
    """mvs_expf returns 0 from -87 down, so a similarity is never subnormal
    itself, and mvs_expf(-80) = 1.8e-35 is a normal number; graded neighbours
    sit 24.45 .. 26.23 units apart horizontally and vertically (simi 4e-38 ..
    4e-33 at gamma = 1/8, or 0) and >= 34.7 diagonally (simi 0)."""
    assert _expf(-80.0) > f32(1e-35) and _expf(-80.0) < f32(3e-35)
    assert _expf(-85.0) > np.finfo(f32).tiny and _expf(-87.0) == 0 and _expf(-200.0) == 0
    g = rc.colour("graded", 1, 9, 13)[0].astype(np.float64)
    dh = np.sqrt(((g[:, 1:] - g[:, :-1]) ** 2).sum(-1))
    dv = np.sqrt(((g[1:] - g[:-1]) ** 2).sum(-1))
    dd = np.sqrt(((g[1:, 1:] - g[:-1, :-1]) ** 2).sum(-1))
    assert 24.0 < min(dh.min(), dv.min()) and max(dh.max(), dv.max()) < 26.7 and dd.min() > 34.0
    assert len(np.unique(rc.colour("flat", 2, 3, 4).reshape(-1, 3), axis=0)) == 1
    far = rc.colour("far", 1, 9, 13)
    assert far.min() < -90 and far.max() > 90
    sm = rc.colour("smooth", 1, 9, 13)
    assert sm.min() >= 0 and sm.max() <= 3


# ---- rounding ties ------------------------------------------------------------------------
def _tie_share(name):
    """Share of cells with a sample whose half-away and half-even pixels both
    lie in the image and carry labels whose superpixels hold different slot-7
    values; and the share of (cell, neighbour, sample) whose two pixels differ."""
    m = rc.make(name)
    hit, moved = [], []
    for z in range(m["V"]):
        if m["sn"][z] == 0:
            hit.append(np.zeros(m["mw"] * m["mh"], bool))
            continue
        p = rc.init_pixels(m, z)
        both = p["in_ha"] & p["in_he"]
        v = p["views"][:, None, None]
        W, H = m["W"], m["H"]
        la = m["labels"][v, np.clip(p["yp_ha"], 0, H - 1), np.clip(p["xp_ha"], 0, W - 1)]
        le = m["labels"][v, np.clip(p["yp_he"], 0, H - 1), np.clip(p["xp_he"], 0, W - 1)]
        d7 = m["spixl"][..., 7].reshape(m["V"], -1)
        differ = both & (d7[v, la] != d7[v, le])
        hit.append(differ.any((0, 2)))
        moved.append((p["xp_ha"] != p["xp_he"]) | (p["yp_ha"] != p["yp_he"]))
    return float(np.concatenate(hit).mean()), float(np.concatenate([a.ravel() for a in moved]).mean())


@pytest.mark.parametrize("name", ["half_3x3", "half_w131", "l4x3_half", "dense_n13_k25", "tiny_1x5"])
def test_half_way_shifts_change_what_is_summed(name):
    """In at least a tenth of the cells some sample's round-half-away pixel and
    round-half-even pixel carry labels whose superpixels hold different slot-7
    values: a wrong tie rule changes the sums, not merely an address.
    Observed: half_3x3 0.49, half_w131 0.43, l4x3_half 0.53,
    dense_n13_k25 0.25, tiny_1x5 0.33; 27-36 % of the (cell, neighbour, sample)
    pixels move.  With integer disparities no pixel moves at all."""
    share, moved = _tie_share(name)
    assert share >= 0.10 and moved >= 0.10, (name, share, moved)
    for other in ("signed", "dense_n16_k1"):
        assert _tie_share(other) == (0.0, 0.0), other


# ---- dense far terms ------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.DENSE_M32)
def test_dense_schedules_fill_the_term_and_candidate_lists(name):
    """On the 32 x 32 map with kss = 1.0 and nks <= 14 some cell has all
    8 + 4 nks smoothness terms valid and some cell all 8 + 4 nks plane
    candidates (observed: 16 cells at nks = 13, 4 at nks = 14, per view); with
    nks >= 13 and kss = 1.0 the valid candidates modulo 8 take a value in each
    of {1}, {2}, {3, 4}, {5, 6, 7} and {0} -- the five lane layouts of the last
    candidate group (observed: every residue 0..7; with kss = 2.5 the
    candidates step by 2 cells and dense_n13_k25 reaches {0, 2, 3, 4, 5, 7},
    four of the five).  The restated counts never exceed 8 + 4 nks."""
    m, o = rc.make(name), rc.oracle_stages(name)
    nks, kss = m["init"]
    nvt, nvalid = rc.term_counts(o["flat"][..., 0], nks, kss)
    full = 8 + 4 * nks
    assert nvt.max() <= full and nvalid.max() <= full and nvt.min() >= 3 and nvalid.min() >= 3
    assert nvt.shape == nvalid.shape == (m["V"], 32, 32)
    if kss == 1.0 and nks <= 14:
        assert (nvt == full).any() and (nvalid == full).any(), (name, int(nvt.max()), int(nvalid.max()))
    if nks >= 13 and kss == 1.0:
        res = set(np.unique(nvalid % 8).tolist())
        for layout in ({1}, {2}, {3, 4}, {5, 6, 7}, {0}):
            assert res & layout, (name, sorted(res))
    if nks == 0:
        assert (nvt == nvalid).all() and set(np.unique(nvt).tolist()) == {3, 5, 8}


def test_term_counts_follow_the_flatness_step():
    """step_size_of(flat0, kss): with one colour flat0 = exp(-1/8) = 0.88, so
    kss = 2.5 gives term steps of 2 cells, as the candidates' (int)kss; with
    smooth colours flat0 is 0.001 .. 0.72 and the terms step by 1 or 2 cells
    while the candidates step by 2: the two lists differ (observed: in 98 % of
    the cells of dense_n14_k25, none of dense_n13_k25)."""
    for name, same in (("dense_n13_k25", True), ("dense_n14_k25", False)):
        m, o = rc.make(name), rc.oracle_stages(name)
        nvt, nvalid = rc.term_counts(o["flat"][..., 0], *m["init"])
        ss = rc.step_size_of(o["flat"][..., 0], m["init"][1])
        assert set(np.unique(ss).tolist()) == ({2} if same else {1, 2}), name
        assert (nvt == nvalid).all() if same else (nvt != nvalid).mean() > 0.5, name
    # the reference schedule at S = 8: every far candidate and almost every far term off a 13 x 9 map (a far
    # term survives only where flat0 is below 0.01 and the step falls to a few cells)
    m, o = rc.make("signed"), rc.oracle_stages("signed")
    nvt, nvalid = rc.term_counts(o["flat"][..., 0], *m["init"])
    assert m["init"] == (13, 328.0) and nvalid.max() <= 8 and (nvt <= 8).mean() >= 0.8
    print("reference schedule, 13 x 9: cells with a valid far term", float((nvt > 8).mean()))


@pytest.mark.parametrize("name", rc.DENSE_M32)
def test_dense_propagate_accepts_planes_and_triangles(name):
    """Iteration 0's output differs from its input in at least half the cells
    and at least one cell in twenty has nz != 1 (a triangle was accepted).
    Observed (changed / nz != 1): n0_k1 1.00 / 0.93, n1_k25 1.00 / 0.85,
    n13_k1 1.00 / 0.85, n13_k25 0.89 / 0.20, n14_k1 1.00 / 0.72, n14_k25
    1.00 / 0.75, n16_k1 0.93 / 0.10, n16_k25 1.00 / 0.52.  Iteration 4 runs on
    that output, so its input normals have left (0, 0, 1), and it changes some
    cell too (observed 0.73 .. 0.97 of the cells)."""
    o = rc.oracle_stages(name)
    s0, s1, s2 = o["state0"], o["states"][0], o["states"][1]
    assert (s0[..., 3:] == f32([0, 0, 1])).all()
    changed = float((_bits(s1) != _bits(s0)).any(-1).mean())
    tilted = float((s1[..., 5] != 1).mean())
    assert changed >= 0.5 and tilted >= 0.05, (name, changed, tilted)
    assert (_bits(s2) != _bits(s1)).any(), name


# ---- underflow ---------------------------------------------------------------------------------
def test_far_colours_leave_no_weight():
    """sm == 0.000001f (wn == 0) in at least half the cells of the init state
    (observed 0.90; the rest have a neighbour within a few units by chance)."""
    o = rc.oracle_stages("far")
    share = float((o["state0"][..., 1] == SM_NONE).mean())
    assert share >= 0.5, share
    assert (o["states"][-1][..., 1] == SM_NONE).mean() >= 0.5


def _init_smoothness(m, z, x, y, nks, kss, flat0):
    """init_smoothness (clcode.cl:1136-1254) of one cell in float32 numpy
    scalars with the oracle's expf: (sm, wn, the products, the far terms valid)."""
    sp, mw, mh = m["spixl"][z], m["mw"], m["mh"]
    gamma, alpha = f32(m["rp"]["init_gamma"]), f32(m["rp"]["init_alpha"])
    c, disp = sp[y, x, 3:6], sp[y, x, 7]

    def dist(a, b):
        d = a - b
        s = d[0] * d[0]
        s = s + d[1] * d[1]
        s = s + d[2] * d[2]
        return np.sqrt(s)

    def ens(diff, k):
        return _expf(((-diff) * diff) * k)

    sm, wn, prods = f32(0), f32(0), []

    def term(q, g, a, b):
        nonlocal sm, wn
        simi = ens(dist(a, b), g)
        prods.append(simi * ens(disp - q[7], alpha))
        sm = sm + prods[-1]
        wn = wn + simi

    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            px, py = x + i, y + j
            if 0 <= px < mw and 0 <= py < mh and (i or j):
                term(sp[py, px], gamma, sp[py, px, 3:6], c)
    ss = int(rc.step_size_of(flat0, kss))
    nfar = 0
    for i in range(1, nks + 1):
        gi, step = gamma * f32(1 + i), i * ss
        cand = [(x - (step + 1), y), (x + (step + 1), y), (x, y - step - 1), (x, y + step + 1)]
        ok = [x > step, x < mw - step - 1, y > step, y < mh - step - 1]
        for (qx, qy), k in zip(cand, ok):
            if k:
                nfar += 1
                term(sp[qy, qx], gi, c, sp[qy, qx, 3:6])
    assert sm.dtype == wn.dtype == f32
    return (sm / wn if wn > 0 else SM_NONE), wn, prods, nfar


@pytest.mark.parametrize("name", ["graded_n0", "graded", "graded_dense"])
def test_graded_colours_give_tiny_weights_and_subnormal_products(name):
    """The smoothness of every cell, restated in float32 numpy with
    orc_dm_expf, equals the oracle's state0[..., 1] bit for bit: in graded_n0
    (nks = 0) no cell has a far term and the 8-neighbour products stand alone;
    in the other two the flatness is 0, the far step 1 cell, and every cell
    has valid far terms (all with simi == 0), restated too.  Some cell has
    0 < wn < 1e-30, a subnormal product and a finite sm.  Observed: all 351
    cells have 0 < wn < 1e-30; 189 of them hold a subnormal product in graded
    and graded_n0 (the wide disparities), 4 in graded_dense (signed ones)."""
    m, o = rc.make(name), rc.oracle_stages(name)
    nks, kss = m["init"]
    tiny_wn = subn = near = zero = 0
    tiny = np.finfo(f32).tiny
    for z in range(m["V"]):
        for y in range(m["mh"]):
            for x in range(m["mw"]):
                with np.errstate(under="ignore"):
                    sm, wn, prods, nfar = _init_smoothness(m, z, x, y, nks, kss, o["flat"][z, y, x, 0])
                assert _bits(sm) == _bits(o["state0"][z, y, x, 1]), (name, z, y, x, nfar, sm, o["state0"][z, y, x, 1])
                near += nfar == 0
                zero += wn == 0
                if 0 < wn < f32(1e-30) and np.isfinite(sm):
                    tiny_wn += 1
                    subn += any(0 < p < tiny for p in prods)
    cells = m["V"] * m["mh"] * m["mw"]
    print(name, "cells", cells, "no far term", near, "tiny wn", tiny_wn, "with a subnormal product", subn, "wn == 0", zero)
    assert near == (cells if nks == 0 else 0), (name, near)
    assert tiny_wn >= 1 and subn >= 1, (name, tiny_wn, subn, cells)
    assert float(o["state0"][..., 1].max()) <= 1.0


# ---- empty consistency ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,views", [("huge", (0, 1, 2)), ("empty_view", (1,)), ("far_empty", (1,)), ("l4x3_plane", (2,)),
                                        ("l4x3_half", (2,)), ("l4x3_dense", (2,))])
def test_empty_consistency_is_the_margin(name, views):
    """cs == 0.01f in every cell of a view without neighbours and of every view
    whose samples all leave the image, after init and after every iteration;
    the other views of the same case have cs above the margin somewhere."""
    m, o = rc.make(name), rc.oracle_stages(name)
    for st in [o["state0"]] + o["states"]:
        for z in range(m["V"]):
            if z in views:
                assert (st[z, ..., 2] == CS_NONE).all(), (name, z)
            else:
                assert (st[z, ..., 2] > CS_NONE).any(), (name, z)
    if name == "huge":
        for z in range(m["V"]):  # restated: no sample of any neighbour lies in the image, under either tie rule
            p = rc.init_pixels(m, z)
            assert m["sn"][z] == 2 and not p["in_ha"].any() and not p["in_he"].any()
    else:
        assert all(m["sn"][z] == 0 for z in views) and (np.delete(m["sn"], views) > 0).all()


# ---- equality in the plane accept tests ---------------------------------------------------------------
def test_far_colours_in_a_view_without_neighbours_tie_the_product_test():
    """far_empty, view 1: cs is the margin for every plane, and wherever
    wn == 0 every plane's sm is 0.000001f, so a candidate's cs * sm EQUALS the
    current sm * cs while its disparity differs; its simi is 0, so the first
    accept test is off.  The strict > keeps such a cell as it is through all
    five iterations.  Condition: at least half of view 1's cells.  Observed:
    0.95 (111 of 117 cells), each with 2 to 8 neighbours of another disparity."""
    m, o = rc.make("far_empty"), rc.oracle_stages("far_empty")
    s0 = o["state0"][1]
    d = m["spixl"][1, ..., 7]
    other = np.zeros(d.shape, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ys, xs = np.mgrid[0:m["mh"], 0:m["mw"]]
                qy, qx = ys + dy, xs + dx
                ok = (qy >= 0) & (qy < m["mh"]) & (qx >= 0) & (qx < m["mw"])
                other |= ok & (d[np.clip(qy, 0, m["mh"] - 1), np.clip(qx, 0, m["mw"] - 1)] != d)
    tied = (s0[..., 1] == SM_NONE) & (s0[..., 2] == CS_NONE) & other
    assert tied.mean() >= 0.5, float(tied.mean())
    for st in o["states"]:
        assert np.array_equal(_bits(st[1][tied]), _bits(s0[tied]))
    assert (_bits(o["states"][0][0]) != _bits(o["state0"][0])).any()  # views with neighbours do move


def test_tile3_ties_the_similarity_test():
    """tile3 with one far step of kss = 2.5: every sm is 0.000001f (wn == 0:
    the 8 neighbours and the far terms 2 cells away are 60 or more Lab units
    off), the far plane candidates sit 3 cells away and share the cell's colour
    exactly, so simi == 1 and sm * simi == the current sm.  Condition: every
    cell has such a candidate, and at least half have one whose disparity
    differs.  Observed: 1.00 and 1.00; iteration 0 leaves 0.23 of the cells
    unchanged, which `>=` would move."""
    m, o = rc.make("tile3"), rc.oracle_stages("tile3")
    assert m["init"] == (1, 2.5) and m["props"][0] == (0, 1, 2.5)
    assert (o["flat"][..., 0] == 0).all() and (rc.step_size_of(o["flat"][..., 0], 2.5) == 1).all()
    for st in [o["state0"]] + o["states"]:
        assert (st[..., 1] == SM_NONE).all()
    col, d = m["spixl"][..., 3:6], m["spixl"][..., 7]
    assert np.array_equal(col[:, :, 3:], col[:, :, :-3]) and np.array_equal(col[:, 3:], col[:, :-3])
    g = col[0].astype(np.float64)
    for dy, dx in ((0, 1), (1, 0), (1, 1), (0, 2), (2, 0)):
        assert np.sqrt(((g[dy:, dx:] - g[:g.shape[0] - dy, :g.shape[1] - dx]) ** 2).sum(-1)).min() >= 59.0
    has = np.ones(d.shape, bool)  # 13 x 9: x - 3 or x + 3 is always in the map
    differs = np.zeros(d.shape, bool)
    differs[:, :, 3:] |= d[:, :, 3:] != d[:, :, :-3]
    differs[:, :, :-3] |= d[:, :, :-3] != d[:, :, 3:]
    differs[:, 3:] |= d[:, 3:] != d[:, :-3]
    differs[:, :-3] |= d[:, :-3] != d[:, 3:]
    assert has.all() and differs.mean() >= 0.5, float(differs.mean())
    assert SM_NONE * _expf(0.0) == SM_NONE
    same = (_bits(o["states"][0]) == _bits(o["state0"])).all(-1).mean()
    assert 0.05 <= same, float(same)


# ---- the reference schedule ---------------------------------------------------------------------------
def test_the_reference_schedule_is_orc_refines():
    """schedule("ref") drives the stage entry points through the iterations
    orc.refine runs: same flatness, init state, five states and fused map."""
    m, o = rc.make("half_3x3"), rc.oracle_stages("half_3x3")
    r = orc.refine(m["spixl"], m["labels"], m["rep"], m["vs"], m["sn"], m["aw"], m["bl"], m["S"], 2.0, 6.0, 1.0, 13,
                   1080, 5, False)
    assert np.array_equal(_bits(r["flat"]), _bits(o["flat"])) and np.array_equal(_bits(r["state0"]), _bits(o["state0"]))
    for it in range(5):
        assert np.array_equal(_bits(r["states"][it]), _bits(o["states"][it])), it
    assert np.array_equal(_bits(r["disp"]), _bits(o["disp"]))


# ---- tiny maps --------------------------------------------------------------------------------------
def test_tiny_maps():
    """1 x 1: no neighbour and no candidate, so sm == 0.000001f and the normal
    (0, 0, 1) throughout, the state never moves.  5 x 1 and 1 x 5: plane
    candidates but no valid triangle: nz stays 1 (all of it exactly (0, 0, 1)),
    yet some cell takes a neighbour's plane (observed: 0.53-0.80 of the cells
    change in iteration 0).  2 x 2: the smallest map with a valid triangle
    (observed: nz != 1 in 0.58 of the cells after iteration 0)."""
    o = rc.oracle_stages("tiny_1x1")
    for st in [o["state0"]] + o["states"]:
        assert (st[..., 1] == SM_NONE).all() and (st[..., 3:] == f32([0, 0, 1])).all()
        assert np.array_equal(_bits(st), _bits(o["state0"]))
    for name in ("tiny_5x1", "tiny_1x5", "tiny_5x1_dense"):
        m, o = rc.make(name), rc.oracle_stages(name)
        assert min(m["mw"], m["mh"]) == 1 and max(m["mw"], m["mh"]) == 5
        for st in o["states"]:
            assert (st[..., 3:] == f32([0, 0, 1])).all(), name
        assert (_bits(o["states"][0]) != _bits(o["state0"])).any(), name
    m, o = rc.make("tiny_2x2"), rc.oracle_stages("tiny_2x2")
    assert (m["mw"], m["mh"]) == (2, 2) and (o["states"][0][..., 5] != 1).any()
    assert [rc.make(n)["mw"] * rc.make(n)["mh"] for n in ("tiny_1x1", "tiny_5x1", "tiny_1x5", "tiny_2x2")] == [1, 5, 5, 4]


# ---- signed disparities at border centres ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["signed", "signed_w131", "dense_n16_k1"])
def test_signed_shifts_bring_outside_samples_back(name):
    """The in-image test is on (xp, yp) alone: a sample whose xr < 0 (a centre
    on column 0) or xr >= W lies in the image after a shift of the right sign.
    Observed: signed 49 such (cell, neighbour, sample) triples, signed_w131
    34, dense_n16_k1 180; and 151 with yr < 0 or yr >= H on the 3 x 3 array."""
    m = rc.make(name)
    nx = ny = 0
    for z in range(m["V"]):
        p = rc.init_pixels(m, z)
        outx = ((p["xr"] < 0) | (p["xr"] >= m["W"]))[None]
        outy = ((p["yr"] < 0) | (p["yr"] >= m["H"]))[None]
        nx += int((p["in_ha"] & outx).sum())
        ny += int((p["in_ha"] & outy).sum())
    assert nx >= 1, (name, nx)
    if m["ah"] > 1:
        assert ny >= 1, (name, ny)
    assert (m["spixl"][..., 7] < 0).any() and (m["spixl"][..., 1] == 0).any()


# ---- the 4 x 3 lists ---------------------------------------------------------------------------------------
def test_the_4x3_lists():
    """Counts exactly {0, 3, 8, 9, 11}; views [0, 6) hold counts <= 8 only
    while the array's maximum is 11, and the rest holds the 9s and 11s; every
    list names distinct other views."""
    m = rc.make("l4x3_plane")
    sn = m["sn"].tolist()
    assert sn == list(rc.L43_COUNTS) and set(sn) == {0, 3, 8, 9, 11} and m["V"] == 12 and m["aw"] == 4
    z0, z1 = rc.L43_LOW
    assert max(sn[z0:z1]) == 8 and max(sn) == 11 and min(sn[z1:]) >= 3 and {9, 11} <= set(sn[z1:])
    for z in range(12):
        l = m["vs"][z, :sn[z]].tolist()
        assert len(set(l)) == len(l) and z not in l and all(0 <= v < 12 for v in l)
    # the 3 x 3 array's middle view has exactly 8 neighbours, the 3 x 1 array's views 2
    assert rc.make("half_3x3")["sn"].tolist() == [3, 5, 3, 5, 8, 5, 3, 5, 3]
    assert rc.make("signed")["sn"].tolist() == [2, 2, 2]
