"""The eight-path semi-global aggregation's definition (tests/sgm8_ref.py) on
the CPU: symmetries of the four diagonal paths, the sum order, accuracy on
scenes whose depth boundaries are round or diagonal, and the
entry point mvs_sgm8_d at the library boundary."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from cl_multiview_stereo_amd import _lib, params, synth
from oracle import oracle as orc
from tests import sgm8_ref as s8
from tests import sgm_ref as sg

F = np.float32
PEN = [(0.1, 0.8), (0.0, 0.0), (0.25, 0.25), (0.5, 4.0)]  # test_sgm_cpu.py's


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.count_nonzero(a != b)
    assert bad == 0, f"{what}: {bad}/{a.size} differ, first at {np.argwhere(a != b)[:3].tolist()}"


def T(v):
    return np.ascontiguousarray(v.transpose(0, 2, 1))


def test_step_is_the_loop_body_of_the_four_path_reference():
    """A row of two pixels: the second pixel of bit 0 is one step from the first."""
    vol = sg.random_volume(9, 5, 2, seed=6)
    for P1, P2 in PEN:
        L = sg.single(vol, 0, P1, P2)
        same(s8.step(vol[:, :, 0], vol[:, :, 1], F(P1), F(P2)), L[:, :, 1], f"step, P1={P1} P2={P2}")


@pytest.mark.parametrize("P1,P2", PEN)
def test_diagonal_symmetries(P1, P2):
    vol = sg.random_volume(40, 6, 70, seed=1)
    same(s8.single(vol, 4, P1, P2), T(s8.single(T(vol), 4, P1, P2)), "bit 4 against bit 4 of the transpose")
    same(s8.single(vol, 6, P1, P2), T(s8.single(T(vol), 7, P1, P2)), "bit 6 against bit 7 of the transpose")
    same(s8.single(vol, 5, P1, P2), s8.single(vol[:, ::-1, ::-1].copy(), 4, P1, P2)[:, ::-1, ::-1],
         "bit 5 against bit 4 on the volume flipped in x and y")
    same(s8.single(vol, 6, P1, P2), s8.single(vol[:, :, ::-1].copy(), 4, P1, P2)[:, :, ::-1],
         "bit 6 against bit 4 on the x-mirrored volume")


def test_a_diagonal_path_by_hand():
    """Bit 4 on a 3 x 4 image, pixel by pixel from the definition: the first row and the first column start a path."""
    vol = sg.random_volume(5, 3, 4, seed=8)
    P1, P2 = F(0.1), F(0.8)
    for bit, (dx, dy) in s8.DIAG.items():
        L = s8.single(vol, bit, P1, P2)
        want = np.empty_like(vol)
        ys = range(3) if dy > 0 else range(2, -1, -1)
        for y in ys:
            for x in range(4):
                qx, qy = x - dx, y - dy
                if 0 <= qx < 4 and 0 <= qy < 3:
                    want[:, y, x] = s8.step(want[:, qy, qx][:, None], vol[:, y, x][:, None], P1, P2)[:, 0]
                else:
                    want[:, y, x] = vol[:, y, x]
        same(L, want, f"bit {bit}")


@pytest.mark.parametrize("P1,P2", PEN)
def test_sum_order_and_single_paths(P1, P2):
    vol = sg.random_volume(17, 9, 33, seed=2)
    for paths in (1, 6, 10, 15):
        same(s8.sgm8(vol, P1, P2, paths), sg.sgm(vol, P1, P2, paths), f"paths={paths} is the four-path reference")
    L = [s8.single(vol, b, P1, P2) for b in range(8)]
    want = L[0]
    for b in range(1, 8):
        want = want + L[b]
    same(s8.sgm8(vol, P1, P2, 255), want, "paths=255")
    same(s8.sgm8(vol, P1, P2, 0xA0), L[5] + L[7], "paths=0xA0")
    for b in range(8):
        same(s8.sgm8(vol, P1, P2, 1 << b), L[b], f"paths={1 << b}")
    # the order is part of the definition: another one differs in some last bits
    other = ((L[7] + L[6]) + (L[5] + L[4])) + ((L[3] + L[2]) + (L[1] + L[0]))
    share = float((bits(s8.sgm8(vol, P1, P2, 255)) != bits(other)).mean())
    print(f"P1={P1} P2={P2}: another summation order differs on {share:.2f} of the cells")
    assert share > 0
    # the eight paths are eight different volumes (with P2 = 0 every path is (vol + m) - m: vol up to a rounding)
    for i in range(8):
        for j in range(i):
            assert (L[i] != L[j]).mean() >= 0.15 if P2 > 0 else (L[i] != L[j]).any(), (i, j)


def test_one_pixel_lines():
    """With W = 1, with H = 1 and at 1 x 1 every diagonal line is one pixel: L is vol."""
    for shape, seed in (((5, 4, 1), 3), ((5, 1, 7), 4), ((5, 1, 1), 5)):
        vol = sg.random_volume(*shape, seed=seed)
        for bit in range(4, 8):
            same(s8.single(vol, bit), vol, f"bit {bit} on {shape}")
        same(s8.sgm8(vol, paths=240), ((vol + vol) + vol) + vol, f"paths=240 on {shape}")


# ---- accuracy on round and diagonal boundaries ---------------------------------------------
def scene(W, H, seed):
    """Discs and diamonds of flat colour on a blurred noise texture; disparity 3 with four discs or diamonds of
    integer disparities in 4..27."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]

    def shape(lo, hi):
        cx, cy, r = rng.integers(0, W), rng.integers(0, H), rng.integers(lo, hi)
        return ((xs - cx) ** 2 + (ys - cy) ** 2 <= r * r) if rng.random() < 0.5 else (abs(xs - cx) + abs(ys - cy) <= r)

    tex = synth._box3(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8))
    for _ in range(4):
        m = shape(H // 8, H // 3)
        tex[m] = rng.integers(0, 256, size=3, dtype=np.uint8)
    disp = np.full((H, W), 3.0)
    for _ in range(4):
        m = shape(H // 6, H // 2)
        disp[m] = float(rng.integers(4, 28))
    return synth.render_stack(tex, disp, 5, 1, 1.0, rng), disp


def bad_shares(stack, gt, masks=(15, 255)):
    """The share of centre-view pixels more than one level off gt: the raw winner's, then one per mask.
    orc.ncc_volume, K = 5, a 5 x 1 array, nearest neighbours, levels 0..31, P1 = 0.1, P2 = 0.8."""
    aw = 5
    l8 = orc.l8(orc.cvt(stack))
    levels = params.disparity_levels(0, 31, 1)
    vs, sn = params.flatten_subsets(params.neighbour_lists(aw, 1, 1, 0))
    vol = orc.ncc_volume(l8, levels, vs, sn, aw, 1.0, 5, aw // 2)
    out = [float((np.abs(orc.wta(vol, levels)[0] - gt) > 1).mean())]
    for m in masks:
        out.append(float((np.abs(orc.wta(s8.sgm8(vol, 0.1, 0.8, m), levels)[0] - gt) > 1).mean()))
    return out


@pytest.mark.parametrize("seed", [900, 901, 902, 903])
def test_accuracy_on_round_and_diagonal_boundaries(seed):
    """DESIGN.md 4c's second table, the 256 x 128 scenes of discs and diamonds: eight
    paths leave fewer pixels more than one level off than four.  The reference
    alone gives, raw / paths = 15 / paths = 255 (ratio 255 / 15):
        seed 900: 0.243 / 0.074 / 0.050 (0.67)    seed 901: 0.192 / 0.053 / 0.032 (0.61)
        seed 902: 0.206 / 0.029 / 0.020 (0.69)    seed 903: 0.165 / 0.041 / 0.028 (0.69)
    The 0.85 is margin over those for reruns elsewhere, not a tuned threshold."""
    stack, gt = scene(256, 128, seed)
    raw, b15, b255 = bad_shares(stack, gt)
    print(f"seed {seed}: bad>1 raw {raw:.3f}, paths=15 {b15:.3f}, paths=255 {b255:.3f} (ratio {b255 / b15:.3f})")
    assert raw > 0.05  # not vacuous
    assert b255 < 0.85 * b15


# ---- the boundary ---------------------------------------------------------------------------
def test_boundary_exports_the_entry_point():
    L = _lib.load()
    assert "mvs_sgm8_d" in _lib.EXPORTS and hasattr(L, "mvs_sgm8_d")
    assert L.mvs_sgm8_d.argtypes is not None and len(L.mvs_sgm8_d.argtypes) == 9
    assert b"0.9.1.1" in L.mvs_version()
    assert L.mvs_sgm8_d(None, 4, 4, 3, None, 0.1, 0.8, 255, None) == -1
    assert b"mvs_sgm8_d" in L.mvs_last_error()
    # and mvs_sgm_d's own message still names mvs_sgm_d
    assert L.mvs_sgm_d(None, 4, 4, 3, None, C.c_float(0.1), C.c_float(0.8), 15, None) == -1
    assert b"mvs_sgm_d" in L.mvs_last_error() and b"mvs_sgm8_d" not in L.mvs_last_error()
