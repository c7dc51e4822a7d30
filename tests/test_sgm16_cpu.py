"""The 16-bit semi-global aggregation's definition (tests/sgm16_ref.py) on the
CPU: the bound that keeps every value inside 16 bits, the order-free sum, a
pixel-by-pixel restatement, accuracy against the float32 definition
(tests/sgm8_ref.py) on the scenes of DESIGN.md 4b / 4c, and the three entry
points at the library boundary."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

from cl_multiview_stereo_amd import _lib, params, synth
from oracle import oracle as orc
from tests import sgm16_ref as s16
from tests import sgm8_ref as s8
from tests.test_sgm8_cpu import scene

PEN = [(205, 1638), (0, 0), (512, 512), (1024, 4095)]


def test_constants():
    assert (s16.SCALE, s16.MAX_COST, s16.MAX_P) == (2047, 4094, 4095)
    assert (s16.P1, s16.P2) == (int(round(0.1 * 2047)), int(round(0.8 * 2047))) == (205, 1638)
    assert s16.MAX_COST == 2 * s16.SCALE and 8 * (s16.MAX_COST + s16.MAX_P) == 65512 < 65536


@pytest.mark.parametrize("p1,p2", PEN)
def test_path_bound(p1, p2):
    """vol <= L <= vol + P2 on random volumes, every path."""
    vol = s16.random_volume(19, 7, 33, seed=11)
    for b in range(8):
        L = s16.single(vol, b, p1, p2)
        assert (L >= vol).all() and (L <= vol.astype(np.int64) + p2).all(), b


def test_extreme_case_stays_inside_16_bits():
    """Every cost 4094, P1 = P2 = 4095, all eight paths: at most 65512."""
    vol = np.full((9, 6, 11), s16.MAX_COST, np.uint16)
    Ls = [s16.single(vol, b, 4095, 4095) for b in range(8)]
    assert max(int(L.max()) for L in Ls) <= 8189
    agg = s16.sgm16(vol, 4095, 4095, 255)
    assert agg.dtype == np.uint16 and int(agg.max()) <= 65512
    # and the bound is nearly met by a volume that alternates 0 and 4094 between neighbouring pixels
    vol = np.zeros((3, 6, 11), np.uint16)
    vol[0] = s16.MAX_COST
    vol[1, ::2, 1::2] = vol[1, 1::2, ::2] = s16.MAX_COST
    vol[2, ::2, ::2] = vol[2, 1::2, 1::2] = s16.MAX_COST
    agg = s16.sgm16(vol, 4095, 4095, 255)
    assert int(agg.max()) <= 65512
    print("largest aggregate of the alternating volume:", int(agg.max()))


def test_sum_is_order_free():
    vol = s16.random_volume(17, 9, 21, seed=2)
    Ls = [s16.single(vol, b) for b in range(8)]
    want = s16.sgm16(vol, paths=255)
    for perm in itertools.islice(itertools.permutations(range(8)), 0, 40320, 4999):
        assert np.array_equal(s16.sum_paths([Ls[b] for b in perm]), want), perm
    assert np.array_equal(s16.sgm16(vol, paths=0xA0), (Ls[5] + Ls[7]).astype(np.uint16))
    for b in range(8):
        assert np.array_equal(s16.sgm16(vol, paths=1 << b), Ls[b].astype(np.uint16)), b
    # the eight paths are eight different volumes
    for i in range(8):
        for j in range(i):
            assert (Ls[i] != Ls[j]).mean() >= 0.15, (i, j)


def scalar_path(vol, dx, dy, p1, p2):
    """One path pixel by pixel and level by level from the definition, plain Python integers."""
    D, H, W = vol.shape
    L = np.zeros((D, H, W), np.int64)
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    for y in ys:
        for x in xs:
            qx, qy = x - dx, y - dy
            if not (0 <= qx < W and 0 <= qy < H):
                L[:, y, x] = vol[:, y, x]
                continue
            q = [int(v) for v in L[:, qy, qx]]
            m = min(q)
            for d in range(D):
                t = min(q[d], m + p2)
                if d > 0:
                    t = min(t, q[d - 1] + p1)
                if d < D - 1:
                    t = min(t, q[d + 1] + p1)
                L[d, y, x] = int(vol[d, y, x]) + t - m
    return L


@pytest.mark.parametrize("p1,p2", PEN)
def test_paths_by_hand(p1, p2):
    vol = s16.random_volume(5, 4, 6, seed=8)
    steps = {0: (1, 0), 1: (-1, 0), 2: (0, 1), 3: (0, -1), **s16.DIAG}
    for b, (dx, dy) in steps.items():
        assert np.array_equal(s16.single(vol, b, p1, p2), scalar_path(vol, dx, dy, p1, p2)), b
    one = s16.random_volume(1, 4, 6, seed=9)  # one level: L is vol on every path
    for b in range(8):
        assert np.array_equal(s16.single(one, b, p1, p2), one), b


def test_quantiser():
    F = np.float32
    c = np.array([-0.005, 0.0, 2.0, 2.5, 1.0, 0.1, 0.8, 0.5 / 2047, 1.5 / 2047, 2.5 / 2047], F)
    q = s16.quant(c)
    assert q.dtype == np.uint16 and q[:7].tolist() == [0, 0, 4094, 4094, 2047, 205, 1638]
    # round-to-nearest-even of the ROUNDED float32 product: state the product and round it here
    prod = (np.clip(c, F(0), F(2)) * F(2047)).astype(F)
    assert q.tolist() == [int(np.rint(float(p))) for p in prod]


def test_winner_rule():
    lev = np.arange(5, dtype=np.float32) * 2
    a = np.array([7, 3, 3, 9, 3], np.uint16).reshape(5, 1, 1)
    d, c = s16.wta(a, lev)
    assert d[0, 0] == 2.0 and c[0, 0] == np.float32(0) / np.float32(2047)  # first of the ties; c2 = agg[4] = 3
    a = np.array([1, 5, 9, 4, 6], np.uint16).reshape(5, 1, 1)
    d, c = s16.wta(a, lev)
    assert d[0, 0] == 0.0 and c[0, 0] == np.float32(3) / np.float32(2047)
    for D in (1, 2, 3):
        a = np.arange(D, 0, -1, dtype=np.uint16).reshape(D, 1, 1)
        d, c = s16.wta(a, lev[:D])
        assert d[0, 0] == lev[D - 1] and c[0, 0] == (np.float32(2) / np.float32(2047) if D == 3 else 0)


# ---- accuracy against the float32 definition ------------------------------------------------
def _scenes():
    for seed in (0, 1, 3):
        yield f"make_stack {seed}", synth.make_stack(256, 128, 5, 1, 0, 31, 1.0, 0x5EED + seed)
    for seed in (900, 901, 903):
        yield f"discs and diamonds {seed}", scene(256, 128, seed)


@pytest.mark.parametrize("k", range(6))
def test_accuracy_against_float32(k):
    """The six 256 x 128 scenes of DESIGN.md 4b / 4c, masks 15 and 255, P1 = 205, P2 = 1638 against 0.1, 0.8: the share
    of pixels more than one level off the ground truth may differ by at most 0.005 and the winners on at most 0.01 of
    the pixels.  The two references alone gave at most 0.0009 and 0.0022: the caps are 5x and 4.5x that."""
    name, (stack, gt) = list(_scenes())[k]
    aw = 5
    l8 = orc.l8(orc.cvt(stack))
    levels = params.disparity_levels(0, 31, 1)
    vs, sn = params.flatten_subsets(params.neighbour_lists(aw, 1, 1, 0))
    vol = orc.ncc_volume(l8, levels, vs, sn, aw, 1.0, 5, aw // 2)
    q = s16.quant(vol)
    assert int(q.max()) <= s16.MAX_COST
    for mask in (15, 255):
        Ls = [s16.single(q, b) for b in range(8) if mask >> b & 1]
        wf = orc.wta(s8.sgm8(vol, 0.1, 0.8, mask), levels)[0]
        wi = s16.wta(s16.sum_paths(Ls), levels)[0]
        bf, bi = float((np.abs(wf - gt) > 1).mean()), float((np.abs(wi - gt) > 1).mean())
        moved = float((wf != wi).mean())
        print(f"{name} mask {mask}: bad>1 float32 {bf:.4f}, uint16 {bi:.4f} (|diff| {abs(bf - bi):.4f}), winners "
              f"differ on {moved:.4f}; largest path value {max(int(L.max()) for L in Ls)}, largest sum "
              f"{int(sum(Ls).max())}")
        assert abs(bf - bi) <= 0.005
        assert moved <= 0.01


# ---- the boundary ---------------------------------------------------------------------------
def test_boundary_exports_the_entry_points():
    L = _lib.load()
    v = L.mvs_version()
    for old in (b"0.9.1", b"0.9.1.1", b"0.9.1.1.1", b"0.9.1.1.1.1"):
        assert old in v
    for name, nargs in (("mvs_quant_u16_d", 4), ("mvs_sgm8_u16_batch_d", 12), ("mvs_wta_u16_d", 8)):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == nargs
    assert L.mvs_quant_u16_d(None, 4, None, None) == -1 and b"mvs_quant_u16_d" in L.mvs_last_error()
    assert L.mvs_sgm8_u16_batch_d(None, 4, 4, 3, 1, None, 48, 205, 1638, 255, None, 48) == -1
    assert b"mvs_sgm8_u16_batch_d" in L.mvs_last_error()
    assert L.mvs_wta_u16_d(None, 4, 4, 3, None, None, None, None) == -1 and b"mvs_wta_u16_d" in L.mvs_last_error()
