"""The sub-level disparity of a semi-global aggregate (tests/sgm_sub_ref.py) on
the CPU: hand-made columns with known answers in both dtypes, the reduction to
subpixel_ref.fit when the aggregate is the volume, the accuracy table of
DESIGN.md 4f on scenes of known fractional disparity (references alone), the
two entry points at the library boundary and the option's ValueError."""
from __future__ import annotations

import numpy as np
import pytest

from cl_multiview_stereo_amd import _lib, params
from cl_multiview_stereo_amd.engine import CameraArray
from cl_multiview_stereo_amd.pipeline import Pipeline, PixelSweep
from oracle import oracle as orc
from tests import sgm16_ref as s16
from tests import sgm8_ref as s8
from tests import sgm_sub_ref as ss
from tests import subpixel_ref as sr

F = np.float32
ar = lambda D: np.arange(D, dtype=np.float32)
HALF = (ar(6) * F(0.5) + F(3)).astype(np.float32)      # 3 + 0.5 i
UNEVEN = np.array([1, 2, 4, 8, 9, 12], np.float32)    # gaps 1, 2, 4, 1, 3
PARABOLA = [(4 * d - 41) ** 2 for d in range(20)]       # 16 (d - 10.25)^2: 25, 1, 9 around d = 10

# (name, agg column, raw column (integers, 4094 = no valid window), levels, disp_sub, class)
HAND = [
    ("parabola_10.25", [abs(d - 10) * 100 + 7 for d in range(20)], PARABOLA, ar(20), 10.25, ss.FITTED),
    ("tie_right", [9, 9, 3, 3, 9], [1000, 500, 250, 250, 1000], ar(5), 2.5, ss.FITTED),   # rp == r0: +0.5
    ("tie_three", [9, 3, 3, 3, 9], [1000, 250, 250, 250, 1000], ar(5), 1.5, ss.FITTED),   # the first minimum of agg
    ("winner_first", [1, 5, 6, 7], [500, 250, 1000, 1500], ar(4), 0.0, ss.END),
    ("winner_last", [7, 6, 5, 1], [1500, 1000, 250, 500], ar(4), 3.0, ss.END),
    ("D1", [5], [500], ar(1) + F(7), 7.0, ss.END),
    ("D2_first", [1, 2], [250, 500], ar(2), 0.0, ss.END),
    ("D2_last", [2, 1], [500, 250], ar(2), 1.0, ss.END),
    ("D3_mid", [5, 1, 5], [1000, 250, 500], ar(3), 1.25, ss.FITTED),
    ("D3_first", [1, 5, 5], [1000, 250, 500], ar(3), 0.0, ss.END),
    ("D3_last", [5, 5, 1], [1000, 250, 500], ar(3), 2.0, ss.END),
    ("left_side_no_window", [5, 1, 5, 5], [4094, 500, 1000, 1500], ar(4), 1.0, ss.NO_WINDOW),
    ("right_side_no_window", [5, 5, 1, 5], [1500, 1000, 500, 4094], ar(4), 2.0, ss.NO_WINDOW),
    ("raw_rises_to_the_right", [9, 9, 1, 9, 9], [100, 200, 300, 400, 500], ar(5) + F(2), 4.0, ss.NO_MINIMUM),
    ("raw_rises_to_the_left", [9, 9, 1, 9, 9], [500, 400, 300, 200, 100], ar(5) + F(2), 4.0, ss.NO_MINIMUM),
    ("raw_tied_on_the_left", [9, 9, 1, 9, 9], [500, 300, 300, 400, 500], ar(5), 2.0, ss.NO_MINIMUM),  # rm == r0
    ("raw_maximum", [9, 9, 1, 9, 9], [100, 200, 900, 200, 100], ar(5), 2.0, ss.NO_MINIMUM),
    ("agg_moved_the_winner", [9, 9, 9, 1, 9, 9], [1500, 200, 1000, 250, 500, 1500], ar(6), 3.25, ss.FITTED),
    ("half_levels_right", [9, 9, 1, 9, 9, 9], [1500, 1000, 250, 500, 1000, 1500], HALF, 4.125, ss.FITTED),
    ("half_levels_left", [9, 9, 1, 9, 9, 9], [1500, 500, 250, 1000, 1000, 1500], HALF, 3.875, ss.FITTED),
    ("uneven_right", [9, 9, 9, 1, 9, 9], [1500, 1250, 1000, 250, 500, 1500], UNEVEN, 8.25, ss.FITTED),
    ("uneven_left", [9, 9, 9, 1, 9, 9], [1500, 1250, 500, 250, 1000, 1500], UNEVEN, 7.0, ss.FITTED),
]
NAMES = [c[0] for c in HAND]


def as_f32(raw):
    """The integer column as float32 costs: k / 2048 (exact, so every quotient of the fit is the integer form's), and
    2.0, "no valid window", for 4094."""
    raw = np.asarray(raw, np.int64)
    return np.where(raw == ss.MAX_COST, F(2.0), raw.astype(np.float32) / F(2048)).astype(np.float32)


def hand(name, dtype):
    """(agg, raw, levels, want disp_sub, want class) of a hand-made column, tiled as subpixel_ref._tile does."""
    _, agg, raw, levels, want, cls = next(c for c in HAND if c[0] == name)
    if dtype == "u16":
        return ss.tile(agg, dtype=np.uint16), ss.tile(raw, dtype=np.uint16), levels, F(want), cls
    return ss.tile(np.asarray(agg, np.float32)), ss.tile(as_f32(raw)), levels, F(want), cls


def fit(dtype, agg, raw, levels):
    return (ss.fit_u16 if dtype == "u16" else ss.fit_f32)(agg, raw, levels)


@pytest.mark.parametrize("dtype", ["u16", "f32"])
@pytest.mark.parametrize("name", NAMES)
def test_hand_made(name, dtype):
    agg, raw, levels, want, wcls = hand(name, dtype)
    assert agg.shape == raw.shape == (len(levels), 5, 70)
    sub, cls, off, b = fit(dtype, agg, raw, levels)
    assert sub.dtype == np.float32 and sub.shape == agg.shape[1:]
    assert (cls == wcls).all(), (name, int(cls.flat[0]), wcls)
    assert (sub == want).all(), (name, sub.flat[0], want)
    wd = (s16.wta(agg, levels) if dtype == "u16" else orc.wta(agg, levels))[0]
    assert (levels[b] == wd).all()  # the winner pass's winner
    if wcls != ss.FITTED:
        assert (sub == levels[b]).all() and (off == 0).all()


def test_hand_made_states():
    """What the named cases are there for."""
    for dtype in ("u16", "f32"):
        got = {n: fit(dtype, *hand(n, dtype)[:3]) for n in NAMES}
        assert (got["parabola_10.25"][2] == F(0.25)).all() and (got["parabola_10.25"][3] == 10).all()
        for n in ("tie_right", "tie_three"):
            assert (got[n][2] == F(0.5)).all(), n
        assert (got["tie_three"][3] == 1).all()
        # the aggregate's winner (3), not the raw volume's (1), and raw has a local minimum there
        agg, raw, levels, _, _ = hand("agg_moved_the_winner", dtype)
        assert (np.argmin(raw, 0) == 1).all() and (got["agg_moved_the_winner"][3] == 3).all()
        assert {int(got[n][1].flat[0]) for n in NAMES} == {ss.END, ss.NO_WINDOW, ss.NO_MINIMUM, ss.FITTED}
        assert {len(hand(n, dtype)[2]) for n in NAMES} >= {1, 2, 3}


def test_the_two_dtypes_agree_on_the_hand_made_columns():
    """k / 2048 is exact in float32, so the float32 form's quotient is the integer form's."""
    for n in NAMES:
        u, f = fit("u16", *hand(n, "u16")[:3]), fit("f32", *hand(n, "f32")[:3])
        for a, b in zip(u, f):
            assert np.array_equal(a, b), n


@pytest.mark.parametrize("D", [1, 2, 3, 4, 17, 33])
def test_reduces_to_the_raw_fit_when_the_aggregate_is_the_volume(D):
    vol = sr.random_volume(D, seed=3)
    levels = (ar(D) * F(0.5) + F(1.25)).astype(np.float32)
    sub, cls, off, b = ss.fit_f32(vol, vol, levels)
    wsub, wok, woff, wb = sr.fit(vol, levels)
    assert np.array_equal(sub.view(np.uint32), wsub.view(np.uint32))
    assert np.array_equal(cls == ss.FITTED, wok) and np.array_equal(off, woff) and np.array_equal(b, wb)
    assert not (cls == ss.NO_MINIMUM).any()
    if D >= 4:
        assert wok.any() and (cls == ss.NO_WINDOW).any()
    raw = s16.random_volume(D, 6, 70, seed=40 + D)
    raw[:, 0] = raw[:, 0] >> 9  # costs 0..7: the minimum is tied often
    sub, cls, off, b = ss.fit_u16(raw, raw, levels)
    assert not (cls == ss.NO_MINIMUM).any()
    if D >= 4:
        assert (cls == ss.FITTED).any() and (off == F(0.5)).any()


def test_no_winner_in_float32():
    """No aggregated cost below the winner pass's initial 1e6: disp is 0 (orc.wta), and so is disp_sub."""
    agg = ss.tile([2e6, 1e6, 3e6, 2e6])
    raw = ss.tile([1.0, 0.25, 0.5, 1.0])
    sub, cls, off, b = ss.fit_f32(agg, raw, ar(4) + F(3))
    assert (orc.wta(agg, ar(4) + F(3))[0] == 0).all()
    assert (sub == 0).all() and (cls == ss.END).all()


# ---- accuracy on scenes of known fractional disparity -------------------------------------------
def _mae(x, d, m=None):
    e = np.abs(np.asarray(x, np.float64) - d)
    return float(e.mean() if m is None else e[m].mean())


@pytest.mark.parametrize("d,K", [(10.25, 5), (13.7, 5), (7.9, 5), (10.25, 7)])
def test_accuracy_on_known_fractional_disparity(d, K):
    """DESIGN.md 4f's table (mean absolute error in levels; subpixel_ref.sinusoid_scene, 5 x 200 x 24, levels 0..31,
    the centre view, penalties 205 / 1638 and 0.1 / 0.8), the references alone.  Over the fitted pixels the error of
    disp_agg_sub is under half that of disp_agg (ratios of 0.10 to 0.25 were measured: the factor two is the margin
    test_subpixel_cpu.py takes for another seed), more than half of the pixels are fitted, and over all pixels
    disp_agg_sub is below the raw volume's disp_sub."""
    V, W, H, dmax = 5, 200, 24, 31
    l8 = sr.sinusoid_scene(d, V, W, H, 0x5EED)
    levels = params.disparity_levels(0, dmax, 1)
    vs, sn = params.flatten_subsets(params.neighbour_lists(V, 1, 1, 0))
    vol = orc.ncc_volume(l8, levels, vs, sn, V, 1.0, K, V // 2)
    disp = orc.wta(vol, levels)[0]
    disp_sub = sr.fit(vol, levels)[0]
    q = s16.quant(vol)
    print(f"d={d} K={K}: disp {_mae(disp, d):.3f}, disp_sub {_mae(disp_sub, d):.3f} (all pixels)")
    for mask in (15, 255):
        for dtype in ("u16", "f32"):
            if dtype == "u16":
                agg, raw = s16.sgm16(q, s16.P1, s16.P2, mask), q
                form_a = ss.fit_through_agg_u16(agg, raw, levels)
            else:
                agg, raw = s8.sgm8(vol, 0.1, 0.8, mask), vol
                form_a = ss.fit_through_agg_f32(agg, raw, levels)
            sub, cls, off, b = fit(dtype, agg, raw, levels)  # asserts den > 0, |off| <= 0.5, the tie rule
            ok = cls == ss.FITTED
            disp_agg = levels[b]
            e_agg, e_sub, e_a = _mae(disp_agg, d, ok), _mae(sub, d, ok), _mae(form_a, d, ok)
            print(f"  mask {mask} {dtype}: disp_agg all {_mae(disp_agg, d):.3f} | fitted pixels: disp_agg {e_agg:.3f}, "
                  f"(a) through the aggregate {e_a:.3f}, (b) through raw at the aggregate's winner {e_sub:.3f} "
                  f"(ratio {e_sub / e_agg:.2f}) | (b) all {_mae(sub, d):.3f} | fitted share {ok.mean():.3f}, classes "
                  f"0/1/2 {(cls == 0).mean():.3f}/{(cls == 1).mean():.3f}/{(cls == 2).mean():.3f}")
            assert ok.mean() > 0.5
            assert e_sub < 0.5 * e_agg
            assert _mae(sub, d) < _mae(disp_sub, d)


# ---- the boundary ---------------------------------------------------------------------------
def test_boundary_exports_the_entry_points():
    L = _lib.load()
    assert b"0.9.1.1.1.1.1" in L.mvs_version()
    for name in ("mvs_wta_agg_sub_d", "mvs_wta_u16_sub_d"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert len(getattr(L, name).argtypes) == 10
        assert getattr(L, name)(None, 4, 4, 3, None, None, None, None, None, None) == -1
        assert name.encode() in L.mvs_last_error()


def test_option_needs_sgm():
    """The constructors refuse sgm_subpixel without sgm before they touch the engine (None here)."""
    st = params.Settings(spixl_size=8, array_width=5, array_height=1, neib_hor=1, neib_ver=0, min_disp=0, max_disp=15,
                         inc=1, bl_ratio=1.0, window=5)
    vs, sn = params.flatten_subsets(params.neighbour_lists(5, 1, 1, 0))
    cam = CameraArray(5, 1.0, params.disparity_levels(0, 15, 1), vs, sn)
    for kw in (dict(), dict(subpixel=True), dict(fused=True), dict(subpixel=True, sgm=False)):
        with pytest.raises(ValueError, match="sgm_subpixel"):
            Pipeline(None, st, 96, 40, pixel_cost="ncc", sgm_subpixel=True, **kw)
        with pytest.raises(ValueError, match="sgm_subpixel"):
            PixelSweep(None, cam, 96, 40, "ncc", 5, sgm_subpixel=True, **kw)
