"""The definition of the semi-global aggregation (include/mvs.h at mvs_sgm_d)
in numpy, float32 throughout, every operation rounded.

A path visits the pixels of one image row or column in order; q is the pixel
before p on it:

    first pixel:  L(p, d) = vol[d][p]
    else:  m = min_k L(q, k)
           t = min(L(q, d), L(q, d-1) + P1 (d > 0), L(q, d+1) + P1 (d < D-1), m + P2)
           L(p, d) = (vol[d][p] + t) - m

agg = ((L_b0 + L_b1) + L_b2) + L_b3 over the set bits of `paths` in bit order:
bit 0 left->right, 1 right->left, 2 top->bottom, 3 bottom->top."""
from __future__ import annotations

import numpy as np

F = np.float32
PATHS = ((2, False), (2, True), (1, False), (1, True))  # (axis of vol [D, H, W], reversed) of bits 0..3


def check_volume(vol):
    vol = np.asarray(vol)
    assert vol.dtype == np.float32 and vol.ndim == 3 and vol.shape[0] >= 1
    assert not np.isnan(vol).any(), "the volume holds a NaN"
    assert not (np.signbit(vol) & (vol == 0)).any(), "the volume holds a -0.0"
    return vol


def path(vol, axis, rev, P1, P2):
    """L of one path: axis 2 = along x, 1 = along y."""
    P1, P2 = F(P1), F(P2)
    v = np.moveaxis(vol, axis, 1)
    v = v[:, ::-1] if rev else v
    L = np.empty_like(v)
    L[:, 0] = v[:, 0]
    for i in range(1, v.shape[1]):
        p = L[:, i - 1]
        m = p.min(axis=0)
        up = np.full_like(p, np.inf)
        up[1:] = p[:-1] + P1
        dn = np.full_like(p, np.inf)
        dn[:-1] = p[1:] + P1
        t = np.minimum(np.minimum(p, up), np.minimum(dn, (m + P2)[None]))
        L[:, i] = (v[:, i] + t) - m[None]
    L = L[:, ::-1] if rev else L
    assert L.dtype == np.float32
    return np.ascontiguousarray(np.moveaxis(L, 1, axis))


def single(vol, bit, P1=0.1, P2=0.8):
    axis, rev = PATHS[bit]
    return path(check_volume(vol), axis, rev, P1, P2)


def sgm(vol, P1=0.1, P2=0.8, paths=15):
    """The aggregate of the paths in the mask, summed in bit order."""
    vol = check_volume(vol)
    assert 1 <= paths <= 15 and np.isfinite(P1) and np.isfinite(P2) and 0 <= F(P1) <= F(P2)
    agg = None
    for bit, (axis, rev) in enumerate(PATHS):
        if paths >> bit & 1:
            L = path(vol, axis, rev, P1, P2)
            agg = L if agg is None else agg + L
    assert agg.dtype == np.float32
    return agg


def random_volume(D, H, W, seed):
    """Costs 2 * random in [0, 2), about one cell in sixteen exactly 2 (no valid window)."""
    rng = np.random.default_rng(seed)
    vol = (F(2) * rng.random((D, H, W), dtype=np.float32)).astype(np.float32)
    vol[rng.random((D, H, W)) < 1 / 16] = F(2)
    return vol
