"""The sub-level disparity's definition, in numpy (helper, no tests).

A three-point parabola fit through the costs of the winning level and its two
neighbours in level order.  All arithmetic is float32, each operation rounded,
no fused multiply-add (numpy float32 arrays do exactly that).  For a pixel
with costs vol[0..D-1] (orc.ncc_volume's definition) and levels[0..D-1]:

    b    = first index of the minimum, in level order, strict <   (orc.wta's rule)
    cm, c0, cp = vol[b-1], vol[b], vol[b+1]
    ok   = 0 < b < D-1  and  cm < 2.0f  and  cp < 2.0f
    den  = (cm - c0) + (cp - c0)
    off  = (0.5f * (cm - cp)) / den
    step = off < 0 ? levels[b] - levels[b-1] : levels[b+1] - levels[b]
    disp_sub = ok ? levels[b] + off * step : levels[b]

ok:   a cost of 2 means no valid window (or the clamp): a side level at cost 2
      is not a measurement.
den:  > 0 whenever ok holds: the first minimum makes cm > c0 strictly, cp >= c0.
off:  rounded subtraction is monotone, so cm - cp <= cm - c0 <= den and
      cp - cm <= cp - c0 <= den: |off| <= 0.5 exactly; cp == c0 gives +0.5.
off * step: the product is rounded first, then the sum.

fit() asserts den > 0, |off| <= 0.5 and the tie rule on every volume it is
given.  hand_cases() are the hand-made volumes the CPU and the GPU tests
share; sinusoid_scene() renders the known-fractional-disparity scenes of the
accuracy table."""
from __future__ import annotations

import numpy as np

F = np.float32


def fit(vol, levels):
    """vol [D, ...] float32, levels [D] -> (disp_sub, ok, off, b), each [...]
    (off is 0 where ok is false)."""
    vol = np.ascontiguousarray(vol, np.float32)
    levels = np.ascontiguousarray(levels, np.float32)
    D = vol.shape[0]
    assert levels.shape == (D,) and not np.isnan(vol).any()
    b = np.argmin(vol, axis=0)  # the first occurrence of the minimum: strict < in level order
    take = lambda i: np.take_along_axis(vol, np.clip(i, 0, D - 1)[None], axis=0)[0]
    cm, c0, cp = take(b - 1), take(b), take(b + 1)
    ok = (b > 0) & (b < D - 1) & (cm < F(2.0)) & (cp < F(2.0))
    lm, lb, lp = levels[np.clip(b - 1, 0, D - 1)], levels[b], levels[np.clip(b + 1, 0, D - 1)]
    with np.errstate(divide="ignore", invalid="ignore"):
        den = (cm - c0) + (cp - c0)
        off = (F(0.5) * (cm - cp)) / den
    assert den.dtype == np.float32 and off.dtype == np.float32
    assert (den[ok] > 0).all(), "den <= 0 on a fitted pixel"
    assert (np.abs(off[ok]) <= F(0.5)).all(), "|off| > 0.5"
    assert (off[ok & (cp == c0)] == F(0.5)).all(), "a tie cp == c0 must give +0.5"
    off = np.where(ok, off, F(0.0)).astype(np.float32)
    step = np.where(off < 0, lb - lm, lp - lb).astype(np.float32)
    t = (off * step).astype(np.float32)
    sub = np.where(ok, lb + t, lb).astype(np.float32)
    return sub, ok, off, b


def _tile(col, H=5, W=70):
    """One pixel's costs [D] as a volume [D, H, W] (more than one wave per row)."""
    col = np.asarray(col, np.float32)
    return np.ascontiguousarray(np.broadcast_to(col[:, None, None], (col.shape[0], H, W)))


def hand_cases():
    """[(name, vol [D, H, W], levels [D], expected disp_sub scalar or None)]."""
    ar = lambda D: np.arange(D, dtype=np.float32)
    cases = []
    d = ar(20)
    cases.append(("parabola_10.25", _tile((d - F(10.25)) ** 2 / F(64)), ar(20), 10.25))
    cases.append(("tie_right", _tile([1, 0.5, 0.25, 0.25, 1]), ar(5), 2.5))
    cases.append(("tie_three", _tile([1, 0.25, 0.25, 0.25, 1]), ar(5), 1.5))  # first minimum, cp == c0
    cases.append(("winner_first", _tile([0.25, 0.5, 1, 1.5]), ar(4), 0.0))
    cases.append(("winner_last", _tile([1.5, 1, 0.5, 0.25]), ar(4), 3.0))
    cases.append(("left_side_two", _tile([2, 0.5, 1, 1.5]), ar(4), 1.0))
    cases.append(("right_side_two", _tile([1.5, 1, 0.5, 2]), ar(4), 2.0))
    cases.append(("all_two", _tile([2, 2, 2, 2]), ar(4), 0.0))
    cases.append(("negative_costs", _tile([0.5, -0.25, -0.5, 0.25]), ar(4), 1.75))
    cases.append(("D1", _tile([0.5]), ar(1) + F(7), 7.0))
    cases.append(("D2_first", _tile([0.25, 0.5]), ar(2), 0.0))
    cases.append(("D2_last", _tile([0.5, 0.25]), ar(2), 1.0))
    cases.append(("D3_mid", _tile([1.0, 0.25, 0.5]), ar(3), 1.0 + 0.5 * 0.5 / 1.0))
    cases.append(("D3_first", _tile([0.25, 0.5, 1.0]), ar(3), 0.0))
    cases.append(("D3_last", _tile([1.0, 0.5, 0.25]), ar(3), 2.0))
    half = (ar(6) * F(0.5) + F(3)).astype(np.float32)  # 3 + 0.5 i
    cases.append(("half_levels_right", _tile([1.5, 1.0, 0.25, 0.5, 1, 1.5]), half, 4.0 + 0.25 * 0.5))
    cases.append(("half_levels_left", _tile([1.5, 0.5, 0.25, 1.0, 1, 1.5]), half, 4.0 - 0.25 * 0.5))
    uneven = np.array([1, 2, 4, 8, 9, 12], np.float32)  # gaps 1, 2, 4, 1, 3
    cases.append(("uneven_right", _tile([1.5, 1.25, 1.0, 0.25, 0.5, 1.5]), uneven, 8.0 + 0.25 * 1.0))
    cases.append(("uneven_left", _tile([1.5, 1.25, 0.5, 0.25, 1.0, 1.5]), uneven, 8.0 - 0.25 * 4.0))
    return [(n, v, l, None if e is None else F(e)) for n, v, l, e in cases]


def random_volume(D, H=6, W=70, seed=0):
    """Costs in [0.5, 1.5) with, per pixel, one of: nothing laid over; the
    minimum tied at d and d + 1; at d and d + 2; a side level at exactly 2."""
    rng = np.random.default_rng([seed, D])
    vol = (0.5 + rng.random((D, H, W))).astype(np.float32)
    if D >= 4:
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        kind = rng.integers(0, 4, (H, W))
        d = rng.integers(1, D - 2, (H, W))
        for k, (gap, val) in {1: (1, 0.25), 2: (2, 0.25), 3: (1, 2.0)}.items():
            m = kind == k
            vol[d[m], yy[m], xx[m]] = F(0.25)
            vol[d[m] + gap, yy[m], xx[m]] = F(val)
    return vol


def sinusoid_scene(d, V=5, W=200, H=24, seed=0, terms=16):
    """uint8 [V, H, W]: a sum of sinusoids T rendered analytically as
    I_v(x, y) = T(x + d * v, y), a V x 1 array of one fronto-parallel plane at
    disparity d (the neighbour at column offset dx sees the reference's pixel
    x at x - d * dx: the sweep's convention)."""
    rng = np.random.default_rng([seed, 0x5B])
    # wavelengths of 4..12 pixels in directions up to 1.2 rad off the x axis: structure at the
    # scale of a 5 x 5 window in both axes (longer waves alone look like ramps inside a window and
    # match at many levels: the winner is then wrong by whole levels, which no fit repairs), no
    # aliasing, and sixteen incommensurate terms so that no shift within the 32 levels repeats
    wl = rng.uniform(4.0, 12.0, terms)
    th = rng.uniform(-1.2, 1.2, terms)
    ph = rng.uniform(0, 2 * np.pi, terms)
    am = rng.uniform(0.5, 1.0, terms)
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    out = np.zeros((V, H, W), np.uint8)
    for v in range(V):
        xs = x + d * v
        t = sum(a * np.sin(2 * np.pi * (np.cos(q) * xs + np.sin(q) * y) / w + p) for a, q, w, p in zip(am, th, wl, ph))
        out[v] = np.clip(np.rint(127.5 + 110.0 * t / am.sum()), 0, 255).astype(np.uint8)
    return out
