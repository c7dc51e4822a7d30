"""The sub-level disparity of a semi-global aggregate, in numpy (helper, no
tests; include/mvs.h at mvs_wta_agg_sub_d and mvs_wta_u16_sub_d).

The winner is the aggregate's; the parabola goes through the RAW costs of the
same view at that winner and its two index neighbours, and only where the raw
costs have a minimum there.  Per pixel, with an aggregate agg[0..D-1], raw
costs raw[0..D-1] and levels[0..D-1] (which need not be ordered):

uint16 form (fit_u16):
    b    = first index of the minimum of agg                    (sgm16_ref.wta's rule)
    rm, r0, rp = raw[b-1], raw[b], raw[b+1]                      (integers)
    ok   = 0 < b < D-1  and  rm < 4094  and  rp < 4094           (4094: no valid window)
           and  rm > r0  and  rp >= r0                           (raw has a minimum at b, orc.wta's tie rule)
    den  = (rm - r0) + (rp - r0)                                 (integer, 1 .. 8186 when ok)
    off  = float32(rm - rp) / float32(2 * den)                   (one float32 divide)
    step = off < 0 ? levels[b] - levels[b-1] : levels[b+1] - levels[b]
    disp_sub = ok ? levels[b] + off * step : levels[b]           (product rounded, then the sum)

float32 form (fit_f32): b by orc.wta's rule on agg (the first index of the
minimum; where no cost is below 1e6, the winner pass's initial cost, there is
no winner and disp_sub is 0, as disp is); cm, c0, cp from the raw vol;
ok = 0 < b < D-1 and cm < 2 and cp < 2 and cm > c0 and cp >= c0; from there
subpixel_ref.fit's arithmetic.  With agg and vol holding the same values the
result is subpixel_ref.fit(vol)'s, bit for bit.

Both assert den > 0, |off| <= 0.5 and the tie rule (rp == r0 gives +0.5) on
every input, and return (disp_sub, cls, off, b) with the class map
    0: b at an end (or no winner)   1: a side without a window
    2: raw has no minimum at b       3: fitted.
fit_through_agg_* is form (a) of DESIGN.md 4f, the fit through the aggregated
costs themselves: kept for the comparison only, no entry point computes it."""
from __future__ import annotations

import numpy as np

F = np.float32
MAX_COST = 4094
WTA_INIT = F(1000000.0)
END, NO_WINDOW, NO_MINIMUM, FITTED = 0, 1, 2, 3


def _take(a, i):
    return np.take_along_axis(a, np.clip(i, 0, a.shape[0] - 1)[None], axis=0)[0]


def _classes(b, D, window, minimum):
    inner = (b > 0) & (b < D - 1)
    return np.where(~inner, END, np.where(~window, NO_WINDOW, np.where(~minimum, NO_MINIMUM, FITTED))).astype(np.int8)


def _finish(b, cls, off, levels):
    """off (float32, valid where fitted) -> disp_sub, with the asserts on off."""
    D = levels.shape[0]
    ok = cls == FITTED
    assert off.dtype == np.float32
    assert (np.abs(off[ok]) <= F(0.5)).all(), "|off| > 0.5"
    off = np.where(ok, off, F(0.0)).astype(np.float32)
    lm, lb, lp = levels[np.clip(b - 1, 0, D - 1)], levels[b], levels[np.clip(b + 1, 0, D - 1)]
    step = np.where(off < 0, lb - lm, lp - lb).astype(np.float32)
    t = (off * step).astype(np.float32)
    sub = np.where(ok, lb + t, lb).astype(np.float32)
    return sub, off


def fit_u16(agg, raw, levels):
    """agg, raw uint16 [D, ...], levels [D] -> (disp_sub float32, cls int8, off float32, b), each [...]."""
    agg, raw = np.asarray(agg), np.asarray(raw)
    levels = np.ascontiguousarray(levels, np.float32)
    D = agg.shape[0]
    assert agg.dtype == np.uint16 and raw.dtype == np.uint16 and agg.shape == raw.shape and levels.shape == (D,)
    b = agg.astype(np.int64).argmin(axis=0)  # the first index of the minimum
    r = raw.astype(np.int64)
    rm, r0, rp = _take(r, b - 1), _take(r, b), _take(r, b + 1)
    cls = _classes(b, D, (rm < MAX_COST) & (rp < MAX_COST), (rm > r0) & (rp >= r0))
    ok = cls == FITTED
    den = (rm - r0) + (rp - r0)
    assert (den[ok] > 0).all() and (den[ok] <= 2 * MAX_COST - 2).all(), "den outside 1..8186 on a fitted pixel"
    den = np.where(ok, den, 1)
    off = ((rm - rp).astype(np.float32) / (2 * den).astype(np.float32)).astype(np.float32)  # (integers below 2^24: exact)
    assert (off[ok & (rp == r0)] == F(0.5)).all() and (off[ok & (rp != r0)] < F(0.5)).all(), "+0.5 iff rp == r0"
    sub, off = _finish(b, cls, off, levels)
    return sub, cls, off, b


def fit_f32(agg, vol, levels):
    """agg, vol float32 [D, ...], levels [D] -> (disp_sub, cls, off, b)."""
    agg = np.ascontiguousarray(agg, np.float32)
    vol = np.ascontiguousarray(vol, np.float32)
    levels = np.ascontiguousarray(levels, np.float32)
    D = agg.shape[0]
    assert agg.shape == vol.shape and levels.shape == (D,) and not np.isnan(agg).any() and not np.isnan(vol).any()
    b = np.argmin(agg, axis=0)  # the first occurrence of the minimum: strict < in level order
    none = _take(agg, b) >= WTA_INIT  # orc.wta: no cost below the initial one, disp = 0
    cm, c0, cp = _take(vol, b - 1), _take(vol, b), _take(vol, b + 1)
    cls = _classes(b, D, (cm < F(2.0)) & (cp < F(2.0)), (cm > c0) & (cp >= c0))
    cls[none] = END
    ok = cls == FITTED
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        den = (cm - c0) + (cp - c0)
        off = (F(0.5) * (cm - cp)) / den
    assert den.dtype == np.float32 and (den[ok] > 0).all(), "den <= 0 on a fitted pixel"
    assert (off[ok & (cp == c0)] == F(0.5)).all(), "a tie cp == c0 must give +0.5"
    sub, off = _finish(b, cls, off, levels)
    sub[none] = F(0.0)
    return sub, cls, off, b


# ---- form (a): the fit through the aggregated costs, for DESIGN.md 4f's comparison only -------------
def fit_through_agg_u16(agg, raw, levels):
    """Parabola through agg[b-1], agg[b], agg[b+1] on the pixels fit_u16 fits (so the two forms are compared on
    one set of pixels) -> disp float32."""
    sub, cls, _, b = fit_u16(agg, raw, levels)
    a = np.asarray(agg).astype(np.int64)
    am, a0, ap = _take(a, b - 1), _take(a, b), _take(a, b + 1)
    den = np.maximum((am - a0) + (ap - a0), 1)
    off = np.where(cls == FITTED, (am - ap) / (2.0 * den), 0.0)
    return (np.asarray(levels, np.float64)[b] + off).astype(np.float32)  # unit level steps


def fit_through_agg_f32(agg, vol, levels):
    sub, cls, _, b = fit_f32(agg, vol, levels)
    a = np.asarray(agg).astype(np.float64)
    am, a0, ap = _take(a, b - 1), _take(a, b), _take(a, b + 1)
    den = (am - a0) + (ap - a0)
    den = np.where(den > 0, den, 1.0)
    off = np.where(cls == FITTED, 0.5 * (am - ap) / den, 0.0)
    return (np.asarray(levels, np.float64)[b] + off).astype(np.float32)


def tile(col, H=5, W=70, dtype=np.float32):
    """One pixel's column [D] as a volume [D, H, W] (subpixel_ref._tile, any dtype)."""
    col = np.asarray(col, dtype)
    return np.ascontiguousarray(np.broadcast_to(col[:, None, None], (col.shape[0], H, W)))
