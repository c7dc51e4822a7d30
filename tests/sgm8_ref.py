"""The definition of the eight-path semi-global aggregation (include/mvs.h at
mvs_sgm8_d) in numpy, float32 throughout, every operation rounded.

The recurrence and bits 0..3 are tests/sgm_ref.py's.  Bits 4..7 are the
diagonal paths; a path visits (x0 + i dx, y0 + i dy), its first pixel is a
pixel whose predecessor (x - dx, y - dy) lies outside the image (L = vol there):

    bit 4: (dx, dy) = (+1, +1) down-right     bit 5: (-1, -1) up-left
    bit 6: (-1, +1) down-left                 bit 7: (+1, -1) up-right

agg = ((((((L_b0 + L_b1) + L_b2) + L_b3) + L_b4) + L_b5) + L_b6) + L_b7 over
the set bits of `paths`, in bit order."""
from __future__ import annotations

import numpy as np

from tests import sgm_ref as sg
from tests.sgm_ref import check_volume, random_volume  # noqa: F401  (one import for the users of this module)

F = np.float32
DIAG = {4: (1, 1), 5: (-1, -1), 6: (-1, 1), 7: (1, -1)}  # (dx, dy) per pixel


def step(p, v, P1, P2):
    """One step of the recurrence: p = L of the pixels before [D, n], v = the costs [D, n].
    The loop body of sgm_ref.path, word for word."""
    m = p.min(axis=0)
    up = np.full_like(p, np.inf)
    up[1:] = p[:-1] + P1
    dn = np.full_like(p, np.inf)
    dn[:-1] = p[1:] + P1
    t = np.minimum(np.minimum(p, up), np.minimum(dn, (m + P2)[None]))
    return (v + t) - m[None]


def diag(vol, dx, dy, P1, P2):
    """L of one diagonal path: flipped so that it runs down-right, where the pixel before (y, x) is (y-1, x-1)."""
    P1, P2 = F(P1), F(P2)
    v = vol[:, ::-1] if dy < 0 else vol
    v = v[:, :, ::-1] if dx < 0 else v
    L = np.empty_like(v)
    L[:, 0] = v[:, 0]
    for y in range(1, v.shape[1]):
        L[:, y, 0] = v[:, y, 0]
        if v.shape[2] > 1:
            L[:, y, 1:] = step(L[:, y - 1, :-1], v[:, y, 1:], P1, P2)
    L = L[:, :, ::-1] if dx < 0 else L
    L = L[:, ::-1] if dy < 0 else L
    assert L.dtype == np.float32
    return np.ascontiguousarray(L)


def single(vol, bit, P1=0.1, P2=0.8):
    if bit < 4:
        return sg.single(vol, bit, P1, P2)
    return diag(check_volume(vol), *DIAG[bit], P1, P2)


def sgm8(vol, P1=0.1, P2=0.8, paths=255):
    """The aggregate of the paths in the mask, summed in bit order."""
    vol = check_volume(vol)
    assert 1 <= paths <= 255 and np.isfinite(P1) and np.isfinite(P2) and 0 <= F(P1) <= F(P2)
    agg = None
    for bit in range(8):
        if paths >> bit & 1:
            L = single(vol, bit, P1, P2)
            agg = L if agg is None else agg + L
    assert agg.dtype == np.float32
    return agg
