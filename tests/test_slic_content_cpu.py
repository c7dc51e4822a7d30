"""tests/slic_content.py on the oracle alone: every built input reaches the
state it was built for, so that tests/test_gpu_slic_content.py compares the
kernels with the oracle where they can go wrong.  Each floor is a condition
the builder was made to meet (counts seen when written are in the docstrings),
not a measurement of the code under test."""
from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as orc
from tests import slic_content as sc

f32 = np.float32


def _kind(*kinds):
    return [n for n, c in sc.CASES.items() if c["kind"] in kinds]


def test_case_table():
    """Lab within [-128, 128] and float32; two differing views wherever the
    image is small; every pixel of every oracle run is assigned to a cell of
    the map (the undefined (uint32_t)(-1.0f) is not under test)."""
    for name, c in sc.CASES.items():
        if c["kind"] in ("wide", "labels32", "legal"):
            continue
        L = sc.lab(name)
        assert L.dtype == f32 and L.shape[0] == 2 and np.abs(L[..., :3]).max() <= 128, name
        assert not np.array_equal(L[0], L[1]), name
        mw, mh = orc.map_size(L.shape[2], L.shape[1], c["S"])
        for out in sc.oracle(name):
            assert out[1].max() < mw * mh, name
    for name in _kind("wide", "labels32", "legal"):  # one view; the same bounds at the iteration counts compared
        c, L = sc.CASES[name], sc.lab(name)
        assert L.dtype == f32 and L.shape[0] == 1 and np.abs(L[..., :3]).max() <= 128, name
        mw, mh = orc.map_size(L.shape[2], L.shape[1], c["S"])
        for p in (0,) if c["kind"] == "wide" else sc.passes(name):
            assert sc.oracle(name, p)[0][1].max() < mw * mh, (name, p)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_slic_from_lab_follows_orc_edge_step(mode):
    """orc.slic_from_lab's edge_enable against orc_slic_ex's own edge step
    (oracle/mvs_oracle.c orc_edge_step) on an 8-bit image."""
    rgbx = np.random.default_rng(5).integers(0, 256, (40, 52, 4), dtype=np.uint8)
    lab, sp, lb = orc.slic(rgbx, 8, 0.6, 2, False, mode)
    out = orc.slic_from_lab(orc.cvt(rgbx), 8, 0.6, 2, False, 0, mode)
    assert len(out) == (3 if mode == 1 else 2)
    assert np.array_equal(out[1], lb) and np.array_equal(out[0].view(np.uint32), sp.view(np.uint32))
    if mode == 1:
        assert np.array_equal(out[2].view(np.uint32), lab.view(np.uint32))
        assert not np.array_equal(lab, orc.cvt(rgbx))


def _first_assignment(name, v):
    c = sc.CASES[name]
    L = sc.lab(name)[v]
    sp = orc.init_centers(L, c["S"])
    lb = orc.assign(L, sp, c["S"], c["weight"], c["search"])
    assert np.array_equal(lb, sc.oracle(name, 0)[v][1])
    return sc.tie_stats(L, sp, c["S"], c["weight"], c["search"]), lb


@pytest.mark.parametrize("name", _kind("near"))
def test_near_ties(name):
    """Per view, in the first assignment: at least 8 pixels with a candidate
    whose d2 lies above the least with d2 * 0.99999905 <= least, and at least
    one whose oracle label is NOT the first candidate of least d2 (two d2 an
    ulp apart whose square roots round together: the earlier candidate keeps
    the pixel).  A fast path without its ambiguity test gets exactly those
    wrong.  Seen (near, discriminating) per view: near_s8 (74, 1), (72, 1);
    near_s40 (82, 1), (38, 1); near_s8_search1 (126, 1), (100, 1); near_s32
    (59, 1), (67, 1); near_s64 (102, 2), (83, 1); near_s16 (67, 1), (47, 1);
    near_s48 (73, 1), (96, 3); near_s16_search1 (111, 2), (91, 1);
    near_s48_search1 (127, 2), (176, 5)."""
    for v in range(2):
        st, lb = _first_assignment(name, v)
        # the numpy restatement of slic_dist's d2 is the oracle's: away from the near ties the first least d2
        # is the label, and the reference's loop over sqrtf(d2) is the label everywhere
        assert np.array_equal(st["first"][~st["near"]], lb[~st["near"]])
        assert np.array_equal(st["ref"], lb)
        assert st["near"].sum() >= 8, (name, v, int(st["near"].sum()))
        assert (st["first"] != lb).sum() >= 1, (name, v)
        assert (st["lo"] < 9.0e11).all()


@pytest.mark.parametrize("name", _kind("flat"))
def test_exact_ties(name):
    """A flat colour on W, H multiples of S: pixels with candidates 0 and 1, 0
    and 2, and 2 and 3 at exactly the least d2 (the first keeps the pixel), in
    the first assignment.  (The first update moves the centres off the
    lattice -- every tie went one way -- and the later assignments have none.)"""
    for v in range(2):
        st, lb = _first_assignment(name, v)
        assert np.array_equal(st["ref"], lb)
        d2, lo = st["d2"], st["lo"]
        for i, j in ((0, 1), (0, 2), (2, 3)):
            tie = (d2[i] == lo) & (d2[j] == lo)
            if i == 2:
                tie &= ~(d2[0] == lo) & ~(d2[1] == lo)
            assert tie.sum() >= 1, (name, v, i, j)
            assert (lb[tie] == st["ids"][i][tie]).all()


@pytest.mark.parametrize("name", _kind("empty"))
def test_empty_superpixel(name):
    """The bottom right superpixel has n == 0 after the first update, its
    centre is zeroed, an assignment follows, and it is still empty after the
    case's last update (seen: exactly that one in every case and view after
    update 1; empty_s8 view 1 has a second from update 2 on)."""
    c = sc.CASES[name]
    assert c["no_iter"] >= 2
    for v in range(2):
        for no_iter in (1, c["no_iter"]):
            sp = sc.oracle(name, no_iter)[v][0]
            assert sp[-1, -1, 6] == 0 and not sp[-1, -1, 1:6].any(), (name, v, no_iter)
            assert sp[-1, -1, 0] == sp.shape[0] * sp.shape[1] - 1
        lb = sc.oracle(name, c["no_iter"])[v][1]
        assert not (lb == sp.shape[0] * sp.shape[1] - 1).any()


@pytest.mark.parametrize("name", _kind("blocks"))
def test_tile_membership(name):
    """(superpixel, window tile) pairs with all 256 pixels members (the packed
    count wraps to 0) and with exactly one member, in the labels every update
    of the case reads.  Seen (full, single) in the first assignment:
    blocks_s16 (20, 26), (18, 33); blocks_s32 (69, 47), (57, 59); blocks_s40
    (45, 83), (47, 82)."""
    c = sc.CASES[name]
    for v in range(2):
        for no_iter in range(c["no_iter"]):
            full, single = sc.tile_counts(sc.oracle(name, no_iter)[v][1], c["S"])
            assert full >= 1 and single >= 1, (name, v, no_iter, full, single)


def test_ragged_sizes():
    """The ragged table holds what it is there for."""
    r = sc.RAGGED
    assert (8, 5, 4) in r and (6, 6, 6) in r  # one cell: an image smaller than S, and S x S
    assert orc.map_size(5, 4, 8) == (1, 1) and orc.map_size(6, 6, 6) == (1, 1)
    assert orc.map_size(7, 50, 8)[0] == 1 and orc.map_size(50, 7, 8)[1] == 1  # 1 x n and n x 1 cells
    assert (16, 10, 40) in r and (16, 40, 10) in r  # W < 16 and H < 16 on the tile path
    for S in (8, 16, 32):
        want = {1, S // 2, S // 2 + 1, S - 1}
        assert {W % S for s, W, H in r if s == S} >= want and {H % S for s, W, H in r if s == S} >= want
    assert any(s == 32 and W % 16 for s, W, H in r)
    for S, W, H in r:
        assert f"ragged_s{S}_{W}x{H}" in sc.CASES


@pytest.mark.parametrize("name", _kind("labels32"))
def test_label_range(name):
    """l32_*: labels of 65,536 and above (the uint32_t update kernels);
    l16_s6: exactly 65,536 cells, the largest label 65,535."""
    c = sc.CASES[name]
    _, H, W, _ = sc.lab(name).shape
    mw, mh = orc.map_size(W, H, c["S"])
    top = max(int(sc.oracle(name, p)[0][1].max()) for p in sc.passes(name))
    if name.startswith("l32"):
        assert mw * mh > 65536 and top >= 65536
    else:
        assert mw * mh == 65536 and top == 65535


@pytest.mark.parametrize("name", _kind("suppress"))
def test_suppression(name):
    """Each pass changes at least 1 % of the labels; in each, pixels sit exactly
    at the threshold (cnt == 16) and pixels are relabelled while their window
    holds several other labels (dl: the last differing neighbour).  Seen: 76 %
    and 57 % changed at S = 8, 49 % and 21 % at S = 32; 361 to 2117 pixels at
    cnt == 16."""
    c = sc.CASES[name]
    for v in range(2):
        _, lb = orc.slic_from_lab(sc.lab(name)[v], c["S"], c["weight"], c["no_iter"], False, c["search"])
        l1 = orc.suppress(lb)
        l2 = orc.suppress(l1)
        assert np.array_equal(l2, sc.oracle(name)[v][1])
        for a, b in ((lb, l1), (l1, l2)):
            cnt, kinds = sc.suppress_counts(a)
            assert np.array_equal(cnt >= 16, a != b)  # the restatement counts what the oracle counts
            assert (a != b).mean() >= 0.01
            assert (cnt == 16).sum() >= 1 and ((cnt >= 16) & (kinds >= 2)).sum() >= 1


_DXY = ((-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1))


def _edge_moves(L, S):
    """Per centre inside the image: (moved, tied) -- tied: its least edge value
    lies below its own and at two neighbours or more -- with the move checked
    to be the first such neighbour in the reference's order."""
    H, W = L.shape[:2]
    e = orc.edge(L)
    sp0 = orc.init_centers(L, S)
    sp1 = orc.apply_edge(L, e, S, sp0)
    moved = tied = 0
    for a, b in zip(sp0.reshape(-1, 8), sp1.reshape(-1, 8)):
        cx, cy = int(a[1]), int(a[2])
        if cx >= W or cy >= H:
            assert np.array_equal(a, b)
            continue
        nb = [(cx + dx, cy + dy) for dx, dy in _DXY if 0 <= cx + dx < W and 0 <= cy + dy < H]
        vals = [e[y, x] for x, y in nb]
        if min(vals) < e[cy, cx]:
            moved += 1
            tied += vals.count(min(vals)) >= 2
            x, y = nb[vals.index(min(vals))]
            assert (b[1], b[2]) == (x, y) and np.array_equal(b[3:6], L[y, x, :3])
        else:
            assert np.array_equal(a, b)
    return moved, tied, sp0


@pytest.mark.parametrize("name", _kind("edge_flat", "edge_step", "edge_border", "edge_noise"))
def test_edge_cases(name):
    """flat: every edge value 0, no centre moves.  step: centres move, some
    with their least edge value at several neighbours (seen: 6 and 8 of 48 at
    S = 8, all tied).  border: every centre on the last row, the last
    column's on the last column, and centres move."""
    c = sc.CASES[name]
    for v in range(2):
        L = sc.lab(name)[v]
        H, W = L.shape[:2]
        moved, tied, sp0 = _edge_moves(L, c["S"])
        if c["kind"] == "edge_flat":
            assert not orc.edge(L).any() and moved == 0
        else:
            assert moved >= 1
        if c["kind"] == "edge_step":
            assert tied >= 1
        if c["kind"] == "edge_border":
            assert (sp0[..., 2] == H - 1).all() and sp0[0, -1, 1] == W - 1


def _far_cells(W, H, S, n=512):
    """The superpixels of the n cell columns (rows, for a tall image) farthest from the origin."""
    mw, mh = orc.map_size(W, H, S)
    sp = np.arange(mw * mh).reshape(mh, mw)
    return (sp[:, -n:] if W >= H else sp[-n:]).ravel()


@pytest.mark.parametrize("name", _kind("wide"))
def test_wide_strips_leave_the_float_tree(name):
    """Beyond W = 65,536 the update kernels' integer tile sums of member x
    (rounded to float once) differ from the reference's float tree: at least
    one (superpixel, tile) pair of the strip's far end does, so the case tells
    the two apart.  Seen, of the pairs of the last 512 cell columns: wide_walk
    (W = 2^20 + 16) 32 of 1024, wide_tiles9 8 of 5091, wide_tiles4 129 of 9200;
    at W = 262,160 the walk has none (some 50 members a tile: sums below 2^24)."""
    c = sc.CASES[name]
    assert not c["legal"]
    L = sc.lab(name)[0]
    H, W = L.shape[:2]
    assert W > sc.MAX_DIM and W * H <= 2 ** 27
    lb = sc.oracle(name, 0)[0][1]
    bad, pairs = sc.inexact_tile_sums(lb, c["S"], 0, _far_cells(W, H, c["S"]))
    assert bad >= 1, (name, bad, pairs)


@pytest.mark.parametrize("name", _kind("legal"))
def test_largest_legal_sizes_keep_the_float_tree(name):
    """At W = 65,536 (H = 65,536) every tile sum of member x and of member y
    is exact: 256 members of at most 65,535 stay below 2^24, and the far end
    of each case shows no differing pair."""
    assert 256 * (sc.MAX_DIM - 1) < 2 ** 24 < 256 * (sc.MAX_DIM + 255)
    c = sc.CASES[name]
    L = sc.lab(name)[0]
    H, W = L.shape[:2]
    assert max(W, H) == sc.MAX_DIM
    lb = sc.oracle(name, 0)[0][1]
    for axis in (0, 1):
        bad, pairs = sc.inexact_tile_sums(lb, c["S"], axis, _far_cells(W, H, c["S"]))
        assert bad == 0 and pairs > 0, (name, axis, bad, pairs)
