"""The definition of the semi-global aggregation on 16-bit integer costs
(include/mvs.h at mvs_quant_u16_d, mvs_sgm8_u16_batch_d and mvs_wta_u16_d) in
numpy.  The aggregation is int64 arithmetic throughout; float32 appears only
in the quantiser's one multiply and the confidence's one divide.

    quant:  q = rint_to_even(min(max(c, 0), 2) * 2047)           (float32 multiply)
    path:   first pixel:  L(p, d) = vol[d][p]
            else:  m = min_k L(q, k)
                   t = min(L(q, d), L(q, d-1) + P1 (d > 0), L(q, d+1) + P1 (d < D-1), m + P2)
                   L(p, d) = vol[d][p] + t - m
    agg = the sum of L over the set bits of `paths` (bits and directions: tests/sgm8_ref.py)
    wta:    b = the first index of the minimum, disp = levels[b],
            c2 = min of agg[k] over |k - b| > 1, conf = float32(c2 - agg[b]) / float32(2047), 0 without such a k

With vol <= MAX_COST and 0 <= P1 <= P2 <= MAX_P: L <= vol + P2 <= 8189, eight
paths sum to at most 65512, so the uint16 result is exact."""
from __future__ import annotations

import numpy as np

SCALE, MAX_COST, MAX_P = 2047, 4094, 4095
P1, P2 = 205, 1638  # 0.1 and 0.8
DIAG = {4: (1, 1), 5: (-1, -1), 6: (-1, 1), 7: (1, -1)}  # (dx, dy) per pixel
AXIS = ((2, False), (2, True), (1, False), (1, True))    # (axis of vol [D, H, W], reversed) of bits 0..3
BIG = np.int64(1) << 40  # a level that does not exist


def quant(c):
    c = np.asarray(c)
    assert c.dtype == np.float32 and not np.isnan(c).any()
    t = np.minimum(np.maximum(c, np.float32(0)), np.float32(2)) * np.float32(SCALE)
    assert t.dtype == np.float32
    return np.rint(t).astype(np.uint16)


def check_volume(vol, strict=True):
    vol = np.asarray(vol)
    assert vol.dtype == np.uint16 and vol.ndim == 3 and vol.shape[0] >= 1
    if strict:
        assert int(vol.max()) <= MAX_COST
    return vol.astype(np.int64)


def check_penalties(p1, p2):
    assert int(p1) == p1 and int(p2) == p2 and 0 <= p1 <= p2 <= MAX_P, (p1, p2)
    return np.int64(p1), np.int64(p2)


def step(p, v, p1, p2):
    """One step: p = L of the pixels before [D, n], v = the costs [D, n], int64."""
    m = p.min(axis=0)
    up = np.full_like(p, BIG)
    up[1:] = p[:-1] + p1
    dn = np.full_like(p, BIG)
    dn[:-1] = p[1:] + p1
    t = np.minimum(np.minimum(p, up), np.minimum(dn, (m + p2)[None]))
    return v + t - m[None]


def axis_path(v64, axis, rev, p1, p2):
    v = np.moveaxis(v64, axis, 1)
    v = v[:, ::-1] if rev else v
    L = np.empty_like(v)
    L[:, 0] = v[:, 0]
    for i in range(1, v.shape[1]):
        L[:, i] = step(L[:, i - 1], v[:, i], p1, p2)
    L = L[:, ::-1] if rev else L
    return np.ascontiguousarray(np.moveaxis(L, 1, axis))


def diag_path(v64, dx, dy, p1, p2):
    """Flipped so that the path runs down-right, where the pixel before (y, x) is (y-1, x-1)."""
    v = v64[:, ::-1] if dy < 0 else v64
    v = v[:, :, ::-1] if dx < 0 else v
    L = np.empty_like(v)
    L[:, 0] = v[:, 0]
    for y in range(1, v.shape[1]):
        L[:, y, 0] = v[:, y, 0]
        if v.shape[2] > 1:
            L[:, y, 1:] = step(L[:, y - 1, :-1], v[:, y, 1:], p1, p2)
    L = L[:, :, ::-1] if dx < 0 else L
    L = L[:, ::-1] if dy < 0 else L
    return np.ascontiguousarray(L)


def single(vol, bit, p1=P1, p2=P2, strict=True):
    """L of one path, int64 [D, H, W]."""
    v = check_volume(vol, strict)
    p1, p2 = check_penalties(p1, p2)
    L = axis_path(v, *AXIS[bit], p1, p2) if bit < 4 else diag_path(v, *DIAG[bit], p1, p2)
    assert L.dtype == np.int64
    return L


def sum_paths(Ls):
    """The aggregate of single-path volumes: their sum, which must fit 16 bits."""
    agg = np.zeros_like(Ls[0])
    for L in Ls:
        agg = agg + L
    assert int(agg.min()) >= 0 and int(agg.max()) <= 65535, "a 16-bit value would wrap"
    return agg.astype(np.uint16)


def sgm16(vol, p1=P1, p2=P2, paths=255):
    assert 1 <= paths <= 255
    return sum_paths([single(vol, b, p1, p2) for b in range(8) if paths >> b & 1])


def wta(agg, levels):
    """(disp, conf) float32 [H, W] of a uint16 aggregate [D, H, W]."""
    agg = np.asarray(agg)
    assert agg.dtype == np.uint16 and agg.ndim == 3
    levels = np.asarray(levels, np.float32)
    D = agg.shape[0]
    assert levels.shape == (D,)
    a = agg.astype(np.int64)
    b = a.argmin(axis=0)  # the first index of the minimum
    best = np.take_along_axis(a, b[None], 0)[0]
    k = np.arange(D)[:, None, None]
    far = np.abs(k - b[None]) > 1
    c2 = np.where(far, a, BIG).min(axis=0)
    diff = np.where(c2 < BIG, c2 - best, 0).astype(np.float32)  # (below 2^24: exact)
    conf = (diff / np.float32(SCALE)).astype(np.float32)
    return levels[b].astype(np.float32), conf


def random_volume(D, H, W, seed):
    """Integer costs in 0..4094, about one cell in sixteen exactly 4094 (no valid window)."""
    rng = np.random.default_rng(seed)
    vol = rng.integers(0, MAX_COST + 1, size=(D, H, W), dtype=np.uint16)
    vol[rng.random((D, H, W)) < 1 / 16] = MAX_COST
    return vol
