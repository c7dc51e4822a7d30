"""The sub-level disparity's definition (tests/subpixel_ref.py) on the CPU:
hand-made volumes with known answers, the invariants den > 0 and |off| <= 0.5
on oracle volumes, the accuracy table of DESIGN.md on scenes of known
fractional disparity, and the two entry points at the library boundary."""
from __future__ import annotations

import numpy as np
import pytest

from cl_multiview_stereo_amd import _lib, params
from oracle import oracle as orc
from tests import subpixel_ref as sr

F = np.float32
CASES = sr.hand_cases()


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_hand_made(name):
    _, vol, levels, want = next(c for c in CASES if c[0] == name)
    sub, ok, off, b = sr.fit(vol, levels)
    assert sub.dtype == np.float32 and sub.shape == vol.shape[1:]
    assert (sub == want).all(), (name, sub.flat[0], want)
    od, _ = orc.wta(vol, levels)
    assert (levels[b] == od).all()  # the same winner as orc.wta's


def test_hand_made_states():
    """What each named case is there for."""
    got = {n: sr.fit(v, l) for n, v, l, _ in CASES}
    sub, ok, off, b = got["parabola_10.25"]
    assert ok.all() and (off == F(0.25)).all() and (b == 10).all() and (sub == F(10.25)).all()
    for n in ("tie_right", "tie_three"):
        assert got[n][1].all() and (got[n][2] == F(0.5)).all()
    for n in ("winner_first", "winner_last", "left_side_two", "right_side_two", "all_two", "D1", "D2_first",
              "D2_last", "D3_first", "D3_last"):
        assert not got[n][1].any() and (got[n][2] == 0).all(), n
    assert got["D3_mid"][1].all() and (got["D3_mid"][2] == F(0.25)).all()
    # the side-dependent step: the same |off| moves by a quarter of the gap on its side
    assert (got["half_levels_right"][0] == F(4.125)).all() and (got["half_levels_left"][0] == F(3.875)).all()
    assert (got["uneven_right"][0] == F(8.25)).all() and (got["uneven_left"][0] == F(7.0)).all()


def test_unit_levels_reduce_to_disp_plus_off():
    vol = sr.random_volume(17, seed=3)
    levels = np.arange(17, dtype=np.float32)
    sub, ok, off, b = sr.fit(vol, levels)
    assert ok.any() and (off != 0).any()
    assert (sub == (levels[b] + off)).all()
    assert (off[(vol.min(0) == np.take_along_axis(vol, np.clip(b + 1, 0, 16)[None], 0)[0]) & ok] == F(0.5)).all()


def _scene(d, K, seed=0x5EED):
    """(integer-level error, fitted error, share of fitted pixels, share with off != 0)."""
    V, W, H, dmax = 5, 200, 24, 31
    l8 = sr.sinusoid_scene(d, V, W, H, seed)
    levels = params.disparity_levels(0, dmax, 1)
    vs, sn = params.flatten_subsets(params.neighbour_lists(V, 1, 1, 0))
    vol = orc.ncc_volume(l8, levels, vs, sn, V, 1.0, K, V // 2)
    sub, ok, off, b = sr.fit(vol, levels)  # asserts den > 0, |off| <= 0.5
    od, _ = orc.wta(vol, levels)
    assert (od == levels[b]).all()
    e_int = float(np.abs(od[ok].astype(np.float64) - d).mean())
    e_sub = float(np.abs(sub[ok].astype(np.float64) - d).mean())
    return e_int, e_sub, float(ok.mean()), float((off != 0).mean())


@pytest.mark.parametrize("d,K", [(10.25, 5), (13.7, 5), (7.9, 5), (10.25, 7)])
def test_accuracy_on_known_fractional_disparity(d, K):
    """DESIGN.md's table: over fitted pixels the mean absolute error of
    disp_sub is under half that of the integer-level disp (the reference
    alone gives ratios near 0.2: the factor two is margin for another seed)."""
    e_int, e_sub, share, moved = _scene(d, K)
    print(f"d={d} K={K}: integer-level MAE {e_int:.3f}, parabola fit {e_sub:.3f}, ratio {e_sub / e_int:.2f}, "
          f"fitted share {share:.2f}")
    assert share > 0.5 and moved > 0.3  # not vacuous
    assert e_sub < 0.5 * e_int


def test_boundary_exports_the_new_entry_points():
    L = _lib.load()
    for name in ("mvs_wta_sub_d", "mvs_ncc_sub_range_d"):
        assert name in _lib.EXPORTS
        assert hasattr(L, name), name
    assert b"0.9" in L.mvs_version()
    assert L.mvs_wta_sub_d(None, 4, 4, 3, None, None, None) == -1
    assert L.mvs_ncc_sub_range_d(None, 4, 4, None, None, None, 5, 0, 1, None, None) == -1
