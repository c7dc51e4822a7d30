"""The adversarial NCC contents (tests/ncc_content.py) reach the states they
are meant to reach -- on the oracle alone (orc.ncc_volume + orc.wta), so that
the GPU tests built on them (tests/test_gpu_ncc_content.py) cannot go vacuous:
exact cost ties at levels far apart, negative costs, costs of exactly 0, 1 and
2 with valid windows, costs on the clamp's boundary.  Validity comes from the
geometry (ncc_content.valid_windows: the oracle's header rule), not from the
costs.  Every content x (K, reference view, height) the GPU tests use.

Not visible here: the cells whose cost exceeds 2 before the clamp (the fused
K = 5 matrix-core fold lets them stand for the clamped 2).  The oracle clamps;
on a scratch copy of it with the clamp removed, periodic(16) with inverted
neighbours (reference 2, levels 0..63, 200 x 24) showed 96 (K = 5) / 144
(K = 7) cells at 2.0000002."""
from __future__ import annotations

import functools

import numpy as np
import pytest

from oracle import oracle as orc
from tests import ncc_content as nc

# (reference view, height): the 5 x 1 array's middle and end view, even and odd height
ZH = [(2, 24), (0, 27), (0, 24), (2, 27)]
DMAX = 63


@functools.lru_cache(maxsize=None)
def _state(case, K, z, H):
    g = nc.HORIZONTAL
    levels, vs, sn = nc.camera(g["aw"], g["ah"], DMAX, nh=g["nh"])
    l8 = nc.make(case, g["aw"] * g["ah"], H, g["W"], ref=z)
    vol = orc.ncc_volume(l8, levels, vs, sn, g["aw"], g["bl"], K, z)
    disp, conf = orc.wta(vol, levels)
    rin, nvalid = nc.valid_windows(levels, vs, sn, g["aw"], g["bl"], K, z, H, g["W"])
    return l8, vol, disp, conf, rin, nvalid


def _far_ties(vol):
    """Pixels whose minimum is attained at two levels more than one apart."""
    D = vol.shape[0]
    idx = np.arange(D)[:, None, None]
    at = vol == vol.min(0)
    return np.where(at, idx, -1).max(0) - np.where(at, idx, D).min(0) > 1


def _window_var(img, K):
    """n * Sqq - Sq^2 of every K x K window inside the image (int64)."""
    H, W = img.shape
    q = img.astype(np.int64) - 128
    s = np.zeros((H - K + 1, W - K + 1), np.int64)
    ss = np.zeros_like(s)
    for j in range(K):
        for i in range(K):
            v = q[j:j + H - K + 1, i:i + W - K + 1]
            s += v
            ss += v * v
    return K * K * ss - s * s


def test_generators_are_deterministic_l8_stacks():
    for case in nc.CASES:
        a = nc.make(case, 5, 24, 200, ref=2)
        b = nc.make(case, 5, 24, 200, ref=2)
        assert a.dtype == np.uint8 and a.shape == (5, 24, 200) and a.flags.c_contiguous, case
        assert np.array_equal(a, b), case
    a = nc.periodic(5, 24, 200, 16, seed=3)
    assert np.array_equal(a[:, :, :-16], a[:, :, 16:]) and not np.array_equal(a[:, :, :-8], a[:, :, 8:])
    t = nc.periodic2d(4, 72, 200, 16, seed=3)
    assert np.array_equal(t[:, :-16], t[:, 16:]) and np.array_equal(t[:, :, :-16], t[:, :, 16:])
    inv = nc.periodic(5, 24, 200, 16, seed=3, invert="neighbours", ref=2)
    assert np.array_equal(inv[2], a[2]) and all(np.array_equal(inv[v], 255 - a[v]) for v in (0, 1, 3, 4))
    some = nc.periodic(5, 24, 200, 16, seed=3, invert=(1, 4))
    assert np.array_equal(some[[0, 2, 3]], a[[0, 2, 3]]) and np.array_equal(some[[1, 4]], 255 - a[[1, 4]])
    blk = nc.periodic(5, 24, 200, 16, seed=3, block=(2, 6, 20, 60, 140, 77))
    assert (blk[2, 6:20, 60:140] == 77).all() and np.array_equal(blk[[0, 1, 3, 4]], a[[0, 1, 3, 4]])
    r = nc.rows_only(3, 24, 200)
    assert (r == r[:, :, :1]).all() and len(np.unique(r[0])) > 12
    assert set(np.unique(nc.saturated(3, 24, 200))) == {0, 255}
    f = nc.full_range(5, 24, 200)
    assert f.min() == 0 and f.max() == 255 and not np.array_equal(f[0], f[1])
    im = nc.impulses(3, 24, 200)
    assert set(np.unique(im)) == {128, 129} and 0.01 < (im == 129).mean() < 0.1


def test_valid_windows_is_the_oracles_rule():
    """The geometric validity agrees with the oracle where the oracle shows
    it: on full-range noise no valid cell costs 2, so cost == 2 exactly where
    no neighbour window is valid."""
    for K, (z, H) in ((5, ZH[1]), (7, ZH[0])):
        l8, vol, disp, conf, rin, nvalid = _state("full", K, z, H)
        assert np.array_equal(vol == 2.0, nvalid == 0)
        assert (nvalid[:, ~rin] == 0).all() and (nvalid[0][rin] == 4).all()


@pytest.mark.parametrize("z,H", ZH)
@pytest.mark.parametrize("K", [5, 7])
@pytest.mark.parametrize("case", ["per16", "per32", "per5", "per16_part", "per16_alt"])
def test_periodic_same_views(case, K, z, H):
    """Periodic columns with at least one neighbour equal to the reference:
    >= 50 % of the pixels have a minimum below 1 at two levels more than one
    apart, >= 1 % of the cells are negative, >= 1 % exactly 0, and the
    confidence is 0 wherever the minimum ties at non-adjacent levels."""
    l8, vol, disp, conf, rin, nvalid = _state(case, K, z, H)
    far = _far_ties(vol) & (vol.min(0) < 1.0)
    assert far.mean() >= 0.5, far.mean()
    assert (vol < 0).mean() >= 0.01, (vol < 0).mean()
    assert (vol == 0).mean() >= 0.01, (vol == 0).mean()
    assert (conf[_far_ties(vol)] == 0).all()
    if case in ("per16_part", "per16_alt") and z == 0:
        # the end view's last valid neighbour (view 1) is inverted: cost 2 with valid windows
        assert np.count_nonzero((vol == 2.0) & (nvalid > 0)) >= 100


@pytest.mark.parametrize("z,H", ZH)
@pytest.mark.parametrize("K", [5, 7])
def test_periodic_inverted(K, z, H):
    """Every neighbour 255 - reference: >= 1 % of the cells cost exactly 2
    while the reference window and at least one shifted window lie inside the
    image (correlation -1: on the clamp), and the minimum still ties far."""
    l8, vol, disp, conf, rin, nvalid = _state("per16_inv", K, z, H)
    share = ((vol == 2.0) & (nvalid > 0)).mean()
    assert share >= 0.01, share
    far = _far_ties(vol) & (vol.min(0) < 2.0)
    assert far.mean() >= 0.5, far.mean()
    assert (conf[_far_ties(vol)] == 0).all()


@pytest.mark.parametrize("z,H", ZH)
@pytest.mark.parametrize("K", [5, 7])
def test_rows_only_same(K, z, H):
    """Row-constant image, identical views: every pixel whose windows are
    valid at all levels has one cost at all levels, some of them negative."""
    l8, vol, disp, conf, rin, nvalid = _state("rows", K, z, H)
    allv = nvalid.min(0) > 0
    assert allv.sum() >= 1000
    cols = vol[:, allv]
    assert (cols == cols[0]).all()
    assert (cols[0] < 0).sum() >= 100 and cols[0].max() < 1e-6
    assert (disp[allv] == 0).all() and (conf[allv] == 0).all()


@pytest.mark.parametrize("z,H", ZH)
@pytest.mark.parametrize("K", [5, 7])
def test_rows_only_inverted(K, z, H):
    """Row-constant, neighbours inverted: among the cells with valid windows
    both 2.0 and a value in (1.999, 2.0) occur (the fused merge's
    all2 = !(best < 2) boundary), and nothing else."""
    l8, vol, disp, conf, rin, nvalid = _state("rows_inv", K, z, H)
    v = vol[nvalid > 0]
    assert (v == 2.0).sum() >= 1000
    assert ((v > 1.999) & (v < 2.0)).sum() >= 1000
    assert v.min() > 1.999


@pytest.mark.parametrize("z,H", ZH)
@pytest.mark.parametrize("K", [5, 7])
def test_saturated_inverted(K, z, H):
    """0 / 255 noise, neighbours inverted: far ties (here also above 1) in
    >= 5 % of the pixels, costs of exactly 2 with valid windows; at K = 7
    window variances above 2^24 (K = 5 cannot reach it: at most 25 * 12 * 255^2
    - (12 * 255)^2 < 2^24)."""
    l8, vol, disp, conf, rin, nvalid = _state("sat_inv", K, z, H)
    far = _far_ties(vol)
    assert far.mean() >= 0.05, far.mean()
    assert (conf[far] == 0).all()
    assert ((vol == 2.0) & (nvalid > 0)).mean() >= 0.002
    if K == 7:
        assert (_window_var(l8[z], K) > 2 ** 24).mean() >= 0.5


@pytest.mark.parametrize("z,H", ZH)
@pytest.mark.parametrize("K", [5, 7])
def test_full_range(K, z, H):
    """Independent noise per view: large sums, no ties (the plain path on
    extreme operands); at K = 7 some window variances pass 2^24."""
    l8, vol, disp, conf, rin, nvalid = _state("full", K, z, H)
    var = np.stack([_window_var(l8[v], K) for v in range(l8.shape[0])])
    assert var.max() < 2 ** 31
    assert var.max() > (2 ** 24 if K == 7 else 2 ** 22)
    assert 0.1 < vol.min() and vol[nvalid > 0].max() < 2.0


@pytest.mark.parametrize("z,H", ZH)
@pytest.mark.parametrize("K", [5, 7])
def test_impulses(K, z, H):
    """128 with isolated 129s: window variances down to n - 1, cost exactly 1
    with a valid neighbour window in >= 1 % of the cells (textureless
    reference windows, and textured ones whose best neighbour is textureless),
    exact ties of the minimum at far levels, costs of exactly 0."""
    l8, vol, disp, conf, rin, nvalid = _state("impulses", K, z, H)
    var = _window_var(l8[z], K)
    assert var[var > 0].min() == K * K - 1 and (var == 0).any()
    assert ((vol == 1.0) & (nvalid > 0)).mean() >= 0.01
    assert _far_ties(vol).mean() >= 0.3
    assert (conf[_far_ties(vol)] == 0).all()
    assert (vol == 0).sum() >= 100


@pytest.mark.parametrize("z,H", ZH)
@pytest.mark.parametrize("K", [5, 7])
def test_constant_block(K, z, H):
    """A constant block in view 2.  Reference 2: its textureless windows cost
    exactly 1 at every level with a valid neighbour (>= 1 % of the cells, all
    levels tied).  Reference 0: textured windows meet the textureless
    neighbour -- cost exactly 1 where it is the best one (>= 100 cells)."""
    l8, vol, disp, conf, rin, nvalid = _state("per16_block", K, z, H)
    one = (vol == 1.0) & (nvalid > 0)
    if z == 2:
        assert one.mean() >= 0.01, one.mean()
        allv = nvalid.min(0) > 0
        flat = allv & (vol == 1.0).all(0)
        assert flat.sum() >= 100 and (conf[flat] == 0).all() and (disp[flat] == 0).all()
    else:
        assert one.sum() >= 100, one.sum()
    assert (_far_ties(vol) & (vol.min(0) < 1.0)).mean() >= 0.5


@pytest.mark.parametrize("z", [0, 3, 11])
@pytest.mark.parametrize("case", ["per2d16", "rows", "full"])
def test_vertical_geometry(case, z):
    """The 8 x 4 array's 5 nearest neighbours (corner, edge and interior
    reference view): the 16 x 16 tile ties far levels through horizontal,
    vertical and diagonal neighbours alike; row-constant images tie through
    the horizontal neighbours; full-range noise has no ties."""
    g = nc.VERTICAL
    levels, vs, sn = nc.camera(g["aw"], g["ah"], g["dmax"], knn=g["knn"], bl=g["bl"])
    l8 = nc.make(case, g["aw"] * g["ah"], g["H"], g["W"], ref=z)
    vol = orc.ncc_volume(l8, levels, vs, sn, g["aw"], g["bl"], 5, z)
    disp, conf = orc.wta(vol, levels)
    far = _far_ties(vol)
    if case == "full":
        assert not (far & (vol.min(0) < 2.0)).any()
    else:
        assert (far & (vol.min(0) < 1.0)).mean() >= 0.5, far.mean()
        assert (vol < 0).mean() >= 0.01 and (vol == 0).mean() >= 0.01
        assert (conf[far] == 0).all()
