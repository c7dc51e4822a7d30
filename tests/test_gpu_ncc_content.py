"""Every NCC / WTA kernel family against the oracle on adversarial image
content (tests/ncc_content.py), bit for bit.

The other parity tests draw natural images (synth.make_stack): no two levels
of a pixel tie, no correlation reaches +-1, only cells without a valid window
cost 2.  The contents here tie the minimum exactly at levels 16, 32 and 5
apart (a matrix-core lane's own pair, its next chunk, across level classes),
put costs below 0, at 0, 1 and 2 and on the clamp (tests/test_ncc_content_cpu.py
pins those states on the oracle alone), so the folds and merges have to
reproduce orc_wta's rule: strict < first minimum in level order, c2 the
minimum outside best +- 1, confidence 0 without such a level.

Families: (a) matrix-core K = 5 horizontal (pair fold), (b) matrix-core K = 7
(med3 fold), (c) matrix-core VERT forms, (d) scalar fused kernels, (e) the
two-pass path and k_wta on hand-made volumes, (f) ncc_wta_range; and the
K = 7 range sweep over a whole 5 x 1 array on natural images.  Each asserts
through ncc_last_variant that its family ran."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd import synth
from cl_multiview_stereo_amd.engine import CameraArray
from oracle import oracle as orc
from tests import ncc_content as nc

pytestmark = pytest.mark.gpu

ZH = [(2, 24), (0, 27), (0, 24), (2, 27)]  # (reference view, height): tests/test_ncc_content_cpu.py's
H_CASES = ["per16", "per32", "per5", "per16_inv", "per16_part", "per16_block", "rows", "rows_inv", "sat_inv", "full",
           "impulses"]
DMAX = 63


def bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.count_nonzero(a != b)
    assert bad == 0, f"{what}: {bad}/{a.size} differ, first at {np.argwhere(a != b)[:3].tolist()}"


@pytest.fixture
def eng(engine):
    engine.set_ncc_variant()
    yield engine
    engine.set_ncc_variant()  # back to automatic for the other tests


def _cam(g, dmax):
    levels, vs, sn = nc.camera(g["aw"], g["ah"], dmax, nh=g.get("nh", 0), knn=g.get("knn"), bl=g["bl"])
    return CameraArray(g["aw"], g["bl"], levels, vs, sn)


_ORACLE = {}  # (content, K, geometry, reference, height) -> (stack, volume at the geometry's most levels)


def _oracle_h(case, K, z, H):
    """Horizontal geometry, levels 0..63 (a volume's first D levels are the
    volume of levels 0..D-1: one volume serves every D)."""
    key = (case, K, "h", z, H)
    if key not in _ORACLE:
        g = nc.HORIZONTAL
        cam = _cam(g, DMAX)
        l8 = nc.make(case, g["aw"], H, g["W"], ref=z)
        _ORACLE[key] = (l8, orc.ncc_volume(l8, cam.levels, cam.view_subset, cam.subset_num, g["aw"], g["bl"], K, z))
    return _ORACLE[key]


_WTA = {}


def _want_h(case, K, z, H, D):
    key = (case, K, z, H, D)
    if key not in _WTA:
        l8, vol = _oracle_h(case, K, z, H)
        _WTA[key] = orc.wta(vol[:D], np.arange(D, dtype=np.float32))
    return _WTA[key]


def _dev(eng, l8, K):
    t = torch.from_numpy(l8).cuda()
    return t, eng.box_stats(t, K)


@pytest.mark.parametrize("case", H_CASES)
def test_mfma_k5_horizontal(eng, case):
    """(a) k_ncc_mfma<5, ..., NDB = 2>: the pair fold without the clamp and
    the 16-class merge.  D = 64 (whole 32-level chunks), 41 (TAIL), 33 (one
    real level in the last chunk); with and without the confidence."""
    for z, H in ZH:
        l8, _ = _oracle_h(case, 5, z, H)
        t, box = _dev(eng, l8, 5)
        for D in (64, 41, 33):
            cam = _cam(nc.HORIZONTAL, D - 1)
            od, oc = _want_h(case, 5, z, H, D)
            fd, fc = eng.ncc_wta(t, box, cam, z, 5)
            v = eng.ncc_last_variant()
            assert (v["K"], v["DPW"], v["FUSE"]) == (5, 32, 1), v  # DPW 32: matrix-core, 32-level chunks
            tag = f"{case} z{z} H{H} D{D}"
            same(fd, od, f"k5 mfma disp {tag}")
            same(fc, oc, f"k5 mfma conf {tag}")
            nd, none = eng.ncc_wta(t, box, cam, z, 5, want_conf=False)
            assert none is None and eng.ncc_last_variant()["DPW"] == 32
            same(nd, od, f"k5 mfma disp, no confidence {tag}")


@pytest.mark.parametrize("case", H_CASES)
def test_mfma_k7_horizontal(eng, case):
    """(b) k_ncc_mfma<7, ..., NDB = 1>: the clamped med3 fold, 16-level
    chunks, D = 64 and 41, double-buffered bands (NB = 2: the only horizontal
    form); the 128-column pitch with whole chunks (C5's kernel) must be among
    the cases that ran."""
    whole128 = 0
    for z, H in ZH:
        l8, _ = _oracle_h(case, 7, z, H)
        t, box = _dev(eng, l8, 7)
        for D in (64, 41):
            cam = _cam(nc.HORIZONTAL, D - 1)
            od, oc = _want_h(case, 7, z, H, D)
            fd, fc = eng.ncc_wta(t, box, cam, z, 7)
            v = eng.ncc_last_variant()
            assert (v["K"], v["DPW"], v["FUSE"]) == (7, 16, 1), v
            tag = f"{case} z{z} H{H} D{D}"
            same(fd, od, f"k7 mfma disp {tag}")
            same(fc, oc, f"k7 mfma conf {tag}")
            assert v["NB"] == 2, v
            if D % 16 == 0 and v["BW"] == 128:
                whole128 += 1
    assert whole128 >= 2, "the 128-column pitch with whole chunks never ran"


@pytest.mark.parametrize("form", ["auto", "22", "21", "12", "11"])
@pytest.mark.parametrize("case", ["per2d16", "rows", "full"])
def test_mfma_vertical_forms(eng, case, form, monkeypatch):
    """(c) k_ncc_mfma<5, ..., VERT>: the 8 x 4 array's 5 nearest neighbours
    at bl = 1.0, 128 levels; a corner, an edge and an interior reference view;
    every (level blocks per chunk, band buffers) form and the launcher's
    choice.  The corner view's list holds a neighbour two rows away: its bands
    may miss the LDS cap and take the scalar kernel, the other two must run
    the matrix-core form."""
    monkeypatch.setenv("MVS_NCC_MFMA_V", "1" if form == "auto" else form)
    g = nc.VERTICAL
    cam = _cam(g, g["dmax"])
    forms = {}
    for z in (0, 3, 11):
        key = (case, 5, "v", z, g["H"])
        if key not in _ORACLE:
            l8 = nc.make(case, g["aw"] * g["ah"], g["H"], g["W"], ref=z)
            _ORACLE[key] = (l8, orc.ncc_volume(l8, cam.levels, cam.view_subset, cam.subset_num, g["aw"], g["bl"], 5,
                                               z))
            _WTA[key] = orc.wta(_ORACLE[key][1], cam.levels)
        od, oc = _WTA[key]
        t, box = _dev(eng, _ORACLE[key][0], 5)
        fd, fc = eng.ncc_wta(t, box, cam, z, 5)
        v = eng.ncc_last_variant()
        same(fd, od, f"vert disp {case} z{z} form {form}")
        same(fc, oc, f"vert conf {case} z{z} form {form}")
        if v["DPW"] >= 16:
            assert v["PAR"] == 0 and v["FUSE"] == 1, v
            forms[z] = f"{v['DPW'] // 16}{v['NB']}"
    assert {3, 11} <= set(forms), forms
    if form != "auto":
        assert set(forms.values()) == {form}, forms


_SCALAR = [None, (8, 4), (4, 2), (4, 1)]  # automatic, then forced (waves, levels per wave)


@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("case", H_CASES)
def test_scalar_fused(eng, case, K, monkeypatch):
    """(d) the scalar fused kernels (k_ncc_volume's FUSE fold across levels
    per wave, waves and chunks): the automatic variant with the matrix-core
    forms off, and chunks of 32, 8 and 4 levels forced, so that ties 16 apart
    fall inside a chunk and across chunks."""
    monkeypatch.setenv("MVS_NCC_MFMA", "0")
    for z, H in ZH:
        l8, _ = _oracle_h(case, K, z, H)
        t, box = _dev(eng, l8, K)
        for D in (64, 41):
            cam = _cam(nc.HORIZONTAL, D - 1)
            od, oc = _want_h(case, K, z, H, D)
            for var in _SCALAR:
                eng.set_ncc_variant(*(var or ()))
                fd, fc = eng.ncc_wta(t, box, cam, z, K)
                v = eng.ncc_last_variant()
                assert v["K"] == K and v["DPW"] < 16 and v["FUSE"] == 1, v
                if var:
                    assert (v["NW"], v["DPW"]) == var, v
                tag = f"{case} K{K} z{z} H{H} D{D} variant {var}"
                same(fd, od, f"scalar fused disp {tag}")
                same(fc, oc, f"scalar fused conf {tag}")
                nd, _ = eng.ncc_wta(t, box, cam, z, K, want_conf=False)
                same(nd, od, f"scalar fused disp, no confidence {tag}")


@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("case", H_CASES)
def test_two_pass(eng, case, K):
    """(e) ncc_volume then wta: the volume's bits (negative costs, exact 0, 1
    and 2) as well as k_wta's choice on them."""
    for z, H in ZH:
        l8, vol = _oracle_h(case, K, z, H)
        t, box = _dev(eng, l8, K)
        for D in (64, 41):
            cam = _cam(nc.HORIZONTAL, D - 1)
            od, oc = _want_h(case, K, z, H, D)
            gv = eng.ncc_volume(t, box, cam, z, K)
            v = eng.ncc_last_variant()
            assert v["K"] == K and v["DPW"] < 16 and v["FUSE"] == 0, v
            tag = f"{case} K{K} z{z} H{H} D{D}"
            same(gv, vol[:D], f"volume {tag}")
            d, c = eng.wta(gv, eng.levels_dev(cam))
            same(d, od, f"wta disp {tag}")
            same(c, oc, f"wta conf {tag}")
            nd, _ = eng.wta(gv, eng.levels_dev(cam), want_conf=False)
            same(nd, od, f"wta disp, no confidence {tag}")


def _hand_volume(kind, D, H=6, W=70):
    """Hand-made costs [D, H, W] (float32): a random background in [0.5, 1.5)
    with the named structure of exact ties laid over it."""
    rng = np.random.default_rng([D, len(kind)])
    vol = (0.5 + rng.random((D, H, W))).astype(np.float32)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    low = np.float32(0.25)
    if kind == "all_equal":
        vol[:] = np.float32(0.75)
    elif kind == "all_two":
        vol[:] = np.float32(2.0)
    elif kind in ("pair_adjacent", "pair_skip_one"):  # the minimum at d and d + 1 only / at d and d + 2
        gap = 1 if kind == "pair_adjacent" else 2
        d = rng.integers(0, D - gap, (H, W))
        vol[d, yy, xx] = low
        vol[d + gap, yy, xx] = low
    elif kind == "first_last":
        vol[0] = low
        vol[D - 1] = low
    elif kind == "runner_up_tied":  # a unique minimum, the second smallest tied next to it and far from it
        d = rng.integers(1, D - 3, (H, W))
        vol[d, yy, xx] = np.float32(0.125)
        vol[d - 1, yy, xx] = low
        vol[d + 3, yy, xx] = low
    else:
        assert kind == "random"
    return vol


@pytest.mark.parametrize("kind,D", [("all_equal", 40), ("all_two", 40), ("pair_adjacent", 40), ("pair_skip_one", 40),
                                    ("first_last", 40), ("runner_up_tied", 40), ("all_equal", 1), ("random", 1),
                                    ("all_equal", 2), ("random", 2), ("pair_adjacent", 2), ("all_equal", 3),
                                    ("random", 3), ("pair_skip_one", 3), ("first_last", 3), ("pair_adjacent", 17),
                                    ("pair_skip_one", 17), ("first_last", 16)])
def test_wta_hand_made_volumes(engine, kind, D):
    """(e) k_wta on volumes no image produces on demand: every cost equal,
    the minimum repeated at d and d + 1 only (no level outside best +- 1 ties:
    the confidence is the gap to the rest), at d and d + 2 (confidence 0), at
    the first and last level, D = 1, 2, 3 (no level outside best +- 1 at all:
    confidence 0), costs of exactly 2 everywhere; D on and off the kernel's
    16-level unroll.  Levels that are not their own index."""
    vol = _hand_volume(kind, D)
    levels = (np.arange(D, dtype=np.float32) * np.float32(0.5) + np.float32(3)).astype(np.float32)
    od, oc = orc.wta(vol, levels)
    if kind in ("all_equal", "all_two", "first_last"):
        assert (od == levels[0]).all()
    if kind in ("all_equal", "all_two", "pair_skip_one", "first_last") or D <= 2:
        assert (oc == 0).all()
    if kind == "pair_adjacent" and D > 3:
        assert (oc >= 0.25).all()
    d, c = engine.wta(torch.from_numpy(vol).cuda(), torch.from_numpy(levels).cuda())
    same(d, od, f"wta disp {kind} D{D}")
    same(c, oc, f"wta conf {kind} D{D}")
    nd, _ = engine.wta(torch.from_numpy(vol).cuda(), torch.from_numpy(levels).cuda(), want_conf=False)
    same(nd, od, f"wta disp, no confidence {kind} D{D}")


@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("case", ["per16", "per16_alt"])
def test_range_every_view(eng, case, K):
    """(f) mvs_ncc_wta_range_d over the whole 5 x 1 array in one call on
    periodic(16), views identical and alternate views inverted (one stack for
    every reference: a reference then sees both +1 and -1 neighbours); every
    view against the oracle."""
    g = nc.HORIZONTAL
    H, V = 24, g["aw"]
    cam = _cam(g, DMAX)
    l8 = nc.make(case, V, H, g["W"])
    t, box = _dev(eng, l8, K)
    rd, rc = eng.ncc_wta_range(t, box, cam, 0, V, K)
    v = eng.ncc_last_variant()
    assert (v["K"], v["DPW"], v["FUSE"]) == (K, 32 if K == 5 else 16, 1), v
    nd, _ = eng.ncc_wta_range(t, box, cam, 0, V, K, want_conf=False)
    for z in range(V):
        key = (case, K, "h", z, H)
        if key not in _ORACLE:  # (the stack does not depend on the reference: per16's entries are _oracle_h's)
            _ORACLE[key] = (l8, orc.ncc_volume(l8, cam.levels, cam.view_subset, cam.subset_num, V, g["bl"], K, z))
        od, oc = _want_h(case, K, z, H, DMAX + 1)
        same(rd[z], od, f"range disp {case} K{K} z{z}")
        same(rc[z], oc, f"range conf {case} K{K} z{z}")
        same(nd[z], od, f"range disp, no confidence {case} K{K} z{z}")


@pytest.mark.parametrize("nh", [4, 2])
def test_range_k7_whole_array_natural(eng, monkeypatch, nh):
    """The K = 7 matrix-core sweep over a range of reference views on natural
    images (ADVICE: compared with the oracle only on views 1..3 at D = 101 and
    an even height): the 5 x 1 array, levels 0..255 (16 whole 16-level
    chunks), 300 x 31 (odd height), views 0..4 in one call, every view against
    the oracle; then the range split into launches of two views
    (MVS_NCC_RUN=2): the same bits.  nh = 4: every other view a neighbour
    (shifts up to 4 columns per level); nh = 2: neighbour counts 2, 3, 4, 3, 2,
    so each reference's records start at its own plan index."""
    aw, W, H, dmax, K = 5, 300, 31, 255, 7
    stack, _ = synth.make_stack(W, H, aw, 1, 0, dmax, 1.0, 0x5EED + 13)
    cam = _cam(dict(aw=aw, ah=1, nh=nh, bl=1.0), dmax)
    assert [int(n) for n in cam.subset_num] == ([4] * 5 if nh == 4 else [2, 3, 4, 3, 2])
    lab, l8 = eng.cvt(torch.from_numpy(stack).cuda())
    box = eng.box_stats(l8, K)
    rd, rc = eng.ncc_wta_range(l8, box, cam, 0, 5, K)
    v = eng.ncc_last_variant()
    assert (v["K"], v["DPW"], v["FUSE"]) == (7, 16, 1), v
    l8h = l8.cpu().numpy()
    for z in range(aw):
        want = orc.ncc_volume(l8h, cam.levels, cam.view_subset, cam.subset_num, aw, 1.0, K, z)
        od, oc = orc.wta(want, cam.levels)
        same(rd[z], od, f"range vs oracle disp z{z}")
        same(rc[z], oc, f"range vs oracle conf z{z}")
    monkeypatch.setenv("MVS_NCC_RUN", "2")
    sd, sc = eng.ncc_wta_range(l8, box, cam, 0, 5, K)
    v = eng.ncc_last_variant()
    assert (v["K"], v["DPW"], v["FUSE"]) == (7, 16, 1), v
    same(sd, rd, "range in launches of two views, disp")
    same(sc, rc, "range in launches of two views, conf")
