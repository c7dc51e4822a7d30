"""Adversarial image content for the NCC / WTA kernels (helper, no tests).

synth.make_stack draws natural, noisy images: no two levels of a pixel cost
the same, no correlation reaches +-1, and only cells without a valid window
cost 2.  The generators here return a uint8 [V, H, W] L8 stack (it goes
straight into engine.box_stats / engine.ncc_* and orc.ncc_volume, no cvt)
whose costs tie exactly across far levels, go negative, equal 0, 1 and 2, and
sit on the clamp -- the states the folds and merges of the fused kernels
branch on.  Everything is deterministic in its arguments.

invert: views replaced by 255 - image -- an iterable of view indices, or
        "neighbours" (every view except `ref`).
block:  (view, y0, y1, x0, x1, value): that block of one view set constant
        (a textureless window meets textured ones), applied after `invert`.

CASES / HORIZONTAL / VERTICAL name the contents and geometries the GPU tests
run (tests/test_gpu_ncc_content.py) and whose states the CPU tests pin on the
oracle alone (tests/test_ncc_content_cpu.py)."""
from __future__ import annotations

import numpy as np

from cl_multiview_stereo_amd import params


def _finish(base, V, invert, ref, block):
    """base: [H, W] (one image for every view) or [V, H, W]."""
    st = np.broadcast_to(base, (V,) + base.shape[-2:]).copy() if base.ndim == 2 else base.copy()
    st = np.ascontiguousarray(st, np.uint8)
    if invert is not None:
        if isinstance(invert, str):
            if invert != "neighbours" or ref is None:
                raise ValueError("invert: a set of views, or 'neighbours' with ref")
            views = [v for v in range(V) if v != ref]
        else:
            views = sorted(int(v) for v in invert)
        for v in views:
            st[v] = 255 - st[v]
    if block is not None:
        v, y0, y1, x0, x1, val = block
        st[v, y0:y1, x0:x1] = val
    return st


def periodic(V, H, W, p, seed=0, invert=None, ref=None, block=None):
    """Columns periodic with period p, full-range random values, the same
    image in every view: levels p apart see the same windows."""
    rng = np.random.default_rng([seed, p, 1])
    tile = rng.integers(0, 256, (H, p), dtype=np.uint8)
    return _finish(tile[:, np.arange(W) % p], V, invert, ref, block)


def periodic2d(V, H, W, p, seed=0, invert=None, ref=None, block=None):
    """A p x p tile repeated: shifts by multiples of p along either axis tie
    (lists with vertical neighbours at bl = 1.0)."""
    rng = np.random.default_rng([seed, p, 2])
    tile = rng.integers(0, 256, (p, p), dtype=np.uint8)
    return _finish(tile[np.arange(H)[:, None] % p, np.arange(W)[None, :] % p], V, invert, ref, block)


def rows_only(V, H, W, seed=0, invert=None, ref=None, block=None):
    """Each row one constant value: a horizontal shift changes nothing."""
    rng = np.random.default_rng([seed, 3])
    col = rng.integers(0, 256, (H, 1), dtype=np.uint8)
    return _finish(np.repeat(col, W, axis=1), V, invert, ref, block)


def saturated(V, H, W, seed=0, invert=None, ref=None, block=None):
    """Random 0 / 255, the same image in every view."""
    rng = np.random.default_rng([seed, 4])
    return _finish((rng.integers(0, 2, (H, W), dtype=np.uint8) * 255).astype(np.uint8), V, invert, ref, block)


def full_range(V, H, W, seed=0, invert=None, ref=None, block=None):
    """Independent random 0..255 per view: variances above 2^24, large Srp."""
    rng = np.random.default_rng([seed, 5])
    return _finish(rng.integers(0, 256, (V, H, W), dtype=np.uint8), V, invert, ref, block)


def impulses(V, H, W, seed=0, invert=None, ref=None, block=None, every=23):
    """128 everywhere with isolated 129s (about one pixel in `every`), the same
    image in every view: var as low as n - 1, many textureless windows."""
    rng = np.random.default_rng([seed, 6])
    img = np.full((H, W), 128, np.uint8)
    img[rng.integers(0, every, (H, W)) == 0] = 129
    return _finish(img, V, invert, ref, block)


_GEN = {"periodic": periodic, "periodic2d": periodic2d, "rows_only": rows_only, "saturated": saturated,
        "full_range": full_range, "impulses": impulses}

# name -> (generator, its keyword arguments); "neighbours" inverts every view but the reference
CASES = {
    "per16": ("periodic", dict(p=16)),
    "per32": ("periodic", dict(p=32)),
    "per5": ("periodic", dict(p=5)),
    "per16_inv": ("periodic", dict(p=16, invert="neighbours")),
    # only views 1 and 4 inverted: a level's best is +1 from one neighbour while others hold -1
    "per16_part": ("periodic", dict(p=16, invert=(1, 4))),
    # alternate views inverted whatever the reference: one stack for a range of reference views
    "per16_alt": ("periodic", dict(p=16, invert=(1, 3))),
    # a constant block in view 2: a textureless reference window against textured
    # neighbours (reference 2), textured against textureless (reference 0)
    "per16_block": ("periodic", dict(p=16, block=(2, 6, 20, 60, 140, 77))),
    "rows": ("rows_only", dict()),
    "rows_inv": ("rows_only", dict(invert="neighbours")),
    "sat_inv": ("saturated", dict(invert="neighbours")),
    "full": ("full_range", dict()),
    "impulses": ("impulses", dict()),
    "per2d16": ("periodic2d", dict(p=16)),
}
SEED = 11


def make(case, V, H, W, ref=None, seed=SEED):
    gen, kw = CASES[case]
    return _GEN[gen](V, H, W, seed=seed, ref=ref, **kw)


def camera(aw, ah, dmax, nh=0, nv=0, knn=None, bl=1.0):
    """(levels 0..dmax, view_subset, subset_num) of an aw x ah array."""
    levels = params.disparity_levels(0, dmax, 1)
    lists = params.nearest_neighbours(aw, ah, knn) if knn else params.neighbour_lists(aw, ah, nh, nv)
    vs, sn = params.flatten_subsets(lists)
    return levels, vs, sn


# the 5 x 1 array, every other view a neighbour (reference 2: +-1 and +-2), 200 columns
HORIZONTAL = dict(aw=5, ah=1, nh=4, W=200, bl=1.0)
# test_mfma_vertical_forms' geometry: 8 x 4, 5 nearest neighbours, 128 levels
VERTICAL = dict(aw=8, ah=4, knn=5, W=200, H=72, dmax=127, bl=1.0)


def valid_windows(levels, vs, sn, aw, bl, K, z, H, W):
    """The oracle's validity rule from the geometry alone (oracle/mvs_oracle.c,
    the NCC volume's header comment): (rin [H, W], nvalid [D, H, W]) -- whether
    the reference window lies in the image, and how many neighbours' shifted
    windows do (0 wherever the reference window does not)."""
    r = K // 2
    V = vs.shape[0]
    y = np.arange(H)[:, None]
    x = np.arange(W)[None, :]
    rin = (x - r >= 0) & (x + r < W) & (y - r >= 0) & (y + r < H)
    nvalid = np.zeros((len(levels), H, W), np.int32)
    rx, ry = z % aw, z // aw
    f = np.float32
    for dl, d in enumerate(np.asarray(levels, np.float32)):
        for n in range(int(sn[z])):
            view = int(vs[z, n]) if vs.ndim == 2 else int(vs[V * z + n])
            dx, dy = view % aw - rx, view // aw - ry
            # roundf: half away from zero
            tx = int(np.copysign(np.floor(np.abs(f(d * f(dx))) + f(0.5)), f(d * f(dx))))
            t = f(f(f(bl) * d) * f(dy))
            ty = int(np.copysign(np.floor(np.abs(t) + f(0.5)), t))
            px, py = x - tx, y - ty
            nvalid[dl] += rin & (px - r >= 0) & (px + r < W) & (py - r >= 0) & (py + r < H)
    return rin, nvalid
