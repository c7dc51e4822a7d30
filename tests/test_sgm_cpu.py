"""The semi-global aggregation's definition (tests/sgm_ref.py) on the CPU:
properties of the reference on random volumes, the accuracy table of DESIGN.md
4b on scenes of known disparity, and the entry point at the library boundary."""
from __future__ import annotations

import numpy as np
import pytest

from cl_multiview_stereo_amd import _lib, params, synth
from oracle import oracle as orc
from tests import sgm_ref as sg

F = np.float32
PEN = [(0.1, 0.8), (0.0, 0.0), (0.25, 0.25), (0.5, 4.0)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b, what):
    a, b = bits(a), bits(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.count_nonzero(a != b)
    assert bad == 0, f"{what}: {bad}/{a.size} differ, first at {np.argwhere(a != b)[:3].tolist()}"


@pytest.mark.parametrize("P1,P2", PEN)
def test_rows_and_columns_are_one_definition(P1, P2):
    """Left->right on vol is top->bottom on the spatial transpose, bit for bit;
    likewise the two reversed paths."""
    vol = sg.random_volume(40, 6, 70, seed=1)
    volT = np.ascontiguousarray(vol.transpose(0, 2, 1))
    for h, v in ((0, 2), (1, 3)):
        a = sg.single(vol, h, P1, P2)
        b = sg.single(volT, v, P1, P2)
        same(a, b.transpose(0, 2, 1), f"bit {h} against bit {v} of the transpose")
    # and a reversed path is the forward one on the mirrored volume
    same(sg.single(vol, 1, P1, P2), sg.single(vol[:, :, ::-1].copy(), 0, P1, P2)[:, :, ::-1], "right->left")
    same(sg.single(vol, 3, P1, P2), sg.single(vol[:, ::-1].copy(), 2, P1, P2)[:, ::-1], "bottom->top")


@pytest.mark.parametrize("P1,P2", PEN)
def test_all_paths_is_the_sum_in_bit_order(P1, P2):
    vol = sg.random_volume(17, 9, 33, seed=2)
    L = [sg.single(vol, b, P1, P2) for b in range(4)]
    same(sg.sgm(vol, P1, P2, 15), ((L[0] + L[1]) + L[2]) + L[3], "paths=15")
    same(sg.sgm(vol, P1, P2, 10), L[1] + L[3], "paths=10")
    for b in range(4):
        same(sg.sgm(vol, P1, P2, 1 << b), L[b], f"paths={1 << b}")
    # the order is part of the definition: another one differs in some last bits
    assert (bits(sg.sgm(vol, P1, P2, 15)) != bits((L[3] + L[2]) + (L[1] + L[0]))).any()
    # the four paths are four different volumes (with P2 = 0 every path is (vol + m) - m: vol up to a rounding)
    for i in range(4):
        for j in range(i):
            assert (L[i] != L[j]).mean() >= 0.25 if P2 > 0 else (L[i] != L[j]).any(), (i, j)


def test_zero_penalties_are_no_copy():
    """With P1 = P2 = 0, t = m and L = (vol + m) - m, which rounds: nobody may
    turn that case into a copy of vol."""
    vol = sg.random_volume(40, 6, 70, seed=3)
    L = sg.single(vol, 0, 0.0, 0.0)
    share = float((L != vol).mean())
    print(f"P1 = P2 = 0: L differs from vol on {share:.3f} of the cells")
    assert share > 0
    assert (L[:, :, 0] == vol[:, :, 0]).all()  # the first pixel of a path is the cost itself
    assert np.abs(L - vol).max() < 1e-6


def test_one_level_and_one_pixel():
    """D = 1: no neighbour levels; L = (vol + min(L, L + P2)) - L.  A path of one pixel is the cost."""
    vol = sg.random_volume(1, 3, 5, seed=4)
    L = sg.single(vol, 0)
    want = vol.copy()
    for x in range(1, 5):
        want[:, :, x] = (vol[:, :, x] + want[:, :, x - 1]) - want[:, :, x - 1]
    same(L, want, "D = 1")
    one = sg.random_volume(5, 1, 1, seed=5)
    same(sg.sgm(one, paths=1), one, "one pixel")
    same(sg.sgm(one), ((one + one) + one) + one, "one pixel, four paths")


@pytest.mark.parametrize("seed", [0, 1, 3, 5])
def test_accuracy_on_known_disparity(seed):
    """DESIGN.md 4b's table, the 256 x 128 scenes: the share of centre-view
    pixels more than one level off falls to under half of the raw winner's (the
    reference alone gives ratios 0.074, 0.067, 0.175 and 0.097 for these four
    seeds: the factor is margin for reruns elsewhere, not a tuned threshold)."""
    W, H, aw = 256, 128, 5
    stack, gt = synth.make_stack(W, H, aw, 1, 0, 31, 1.0, 0x5EED + seed)
    l8 = orc.l8(orc.cvt(stack))
    levels = params.disparity_levels(0, 31, 1)
    vs, sn = params.flatten_subsets(params.neighbour_lists(aw, 1, 1, 0))
    vol = orc.ncc_volume(l8, levels, vs, sn, aw, 1.0, 5, aw // 2)
    raw, _ = orc.wta(vol, levels)
    agg, _ = orc.wta(sg.sgm(vol, 0.1, 0.8, 15), levels)
    bad_raw, bad_agg = float((np.abs(raw - gt) > 1).mean()), float((np.abs(agg - gt) > 1).mean())
    mae_raw, mae_agg = float(np.abs(raw - gt).mean()), float(np.abs(agg - gt).mean())
    print(f"seed {seed}: bad>1 raw {bad_raw:.3f} -> aggregated {bad_agg:.3f} (ratio {bad_agg / bad_raw:.3f}), "
          f"MAE {mae_raw:.2f} -> {mae_agg:.2f}")
    assert bad_raw > 0.05  # not vacuous
    assert bad_agg < 0.5 * bad_raw


def test_boundary_exports_the_entry_point():
    L = _lib.load()
    assert "mvs_sgm_d" in _lib.EXPORTS and hasattr(L, "mvs_sgm_d")
    assert b"0.9.1" in L.mvs_version()
    import ctypes as C
    assert L.mvs_sgm_d(None, 4, 4, 3, None, C.c_float(0.1), C.c_float(0.8), 15, None) == -1
    assert b"mvs_sgm_d" in L.mvs_last_error()
