"""Built Lab inputs for the SLIC stage (helper, no tests; numpy and the oracle only).

Every other SLIC test feeds mvs_slic_d what k_cvt makes of a synth.make_stack
scene, so its Lab stays on the 8-bit gamut lattice and reaches the kernels'
rare branches by luck.  mvs_slic_d takes Lab as plain floats, so here the Lab
image is made by hand, one builder per state of cl_multiview_stereo_amd/csrc/
slic.hip that a test should reach:

  near_tie()   flat L = 50 with per-pixel L steps of 2^-9 and a = (x mod 3) 2^-8:
               at the pixels halfway between two centres the candidates' d2
               differ by an ulp or two, so their square roots may round together
               (k_assign<false> / k_assign_tiles4's ambiguity test)
  flat()       one colour per view: exact ties between candidates 0/1, 0/2, 2/3
  empty()      W mod S = S/2 puts the last column's centres at x = W, where they
               take the colour of the NEXT row's first pixel; that column is far
               from everything else, so those superpixels lose every pixel and
               the update zeroes their centres (the n == 0 branches)
  blocks()     cell-aligned colours, far apart, with a few pixels of a neighbour
               cell's colour: 16 x 16 tiles wholly inside one superpixel (the
               packed count wraps to 0) and tiles with exactly one member
  noise()      uniform Lab: ragged maps, the 65,536-wide strips
  pattern()    cheap integer arithmetic: the maps of more than 65,536 cells
  stripes()    2-pixel stripes plus noise: labels the suppression passes change
  step()       one vertical or horizontal step: the edge modes

Contract: L, a, b within [-128, 128] (so every d2 is far below the reference's
999999.9999 first-candidate bound and every pixel is assigned), the 4th float
arbitrary (nothing may read it).

CASES names every input the GPU tests run (tests/test_gpu_slic_content.py);
tests/test_slic_content_cpu.py pins, on the oracle alone, the state each is
there for.  The restatements below (cand_d2, window_tiles, tree256,
suppress_counts) are written from oracle/mvs_oracle.c's loops in numpy float32,
in its operation order.  Everything is deterministic in its arguments."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle as orc

f32 = np.float32
SEED = 53
NEAR = f32(0.99999905)  # the kernels' near-tie factor (slic.hip k_assign)
MAX_DIM = 65536         # mvs_slic_d's bound on W and on H (include/mvs.h)


def _rng(*key):
    return np.random.default_rng([SEED] + [sum(map(ord, k)) if isinstance(k, str) else int(k) for k in key])


def _stack(L, a, b, key):
    """[V, H, W, 4] from three [V, H, W] planes; the 4th float is noise."""
    out = np.empty(L.shape + (4,), f32)
    out[..., 0], out[..., 1], out[..., 2] = L, a, b
    out[..., 3] = _rng("w", *key).uniform(-9, 9, L.shape)
    assert np.abs(out[..., :3]).max() <= 128
    return out


# ---- builders -----------------------------------------------------------------------------------
def near_tie(V, H, W, seed, steps=16):
    rng = _rng("near", V, H, W, seed)
    x = np.broadcast_to(np.arange(W), (V, H, W))
    L = 50 + rng.integers(0, steps, (V, H, W)) * 2.0 ** -9
    a = (x % 3) * 2.0 ** -8
    b = np.arange(V)[:, None, None] * 2.0 ** -7 + np.zeros((V, H, W))
    return _stack(L, a, b, ("near", seed))


def flat(V, H, W):
    o = np.ones((V, H, W))
    v = np.arange(V)[:, None, None]
    return _stack((50 + 10 * v) * o, 5.5 * o, -7.25 * v * o, ("flat",))


def empty(V, H, W, S):
    assert W % S == S // 2
    rng = _rng("empty", V, H, W, S)
    L, a, b = 50 + rng.uniform(-2, 2, (V, H, W)), rng.uniform(-2, 2, (V, H, W)), rng.uniform(-2, 2, (V, H, W))
    L[:, :, 0], a[:, :, 0], b[:, :, 0] = -100, 100, -100
    return _stack(L, a, b, ("empty", S))


def blocks(V, H, W, S, salt=256):
    rng = _rng("blocks", V, H, W, S)
    y, x = np.mgrid[0:H, 0:W]
    cx, cy = np.broadcast_to(x // S, (V, H, W)), np.broadcast_to(y // S, (V, H, W))
    s = rng.integers(0, salt, (V, H, W)) == 0  # such a pixel takes the colour of a cell next to its own
    cx = cx + np.where(s, rng.integers(-1, 2, (V, H, W)), 0)
    cy = cy + np.where(s, rng.integers(-1, 2, (V, H, W)), 0)
    v = np.arange(V)[:, None, None]
    L = (cx % 3 - 1) * 80.0 + v  # nine colours 80 apart: the 3 x 3 cells around a pixel all differ
    a = (cy % 3 - 1) * 80.0 - v
    return _stack(L, a, 3.0 + 0 * L, ("blocks", S))


def noise(V, H, W, key=0, amp=30.0):
    rng = _rng("noise", V, H, W, key)
    return _stack(50 + rng.uniform(-amp, amp, (V, H, W)), rng.uniform(-amp, amp, (V, H, W)),
                  rng.uniform(-amp, amp, (V, H, W)), ("noise", key))


def pattern(V, H, W):
    y, x = np.mgrid[0:H, 0:W]
    L = ((x * 7 + y * 13) % 64 + 20).astype(f32)
    a = ((x * 3 + y * 5) % 32 - 16).astype(f32)
    b = ((x ^ y) % 16).astype(f32)
    out = np.empty((V, H, W, 4), f32)
    out[..., 0], out[..., 1], out[..., 2], out[..., 3] = L, a, b, 1.5
    return out


def stripes(V, H, W, amp):
    rng = _rng("stripes", V, H, W)
    y, x = np.mgrid[0:H, 0:W]
    v = np.arange(V)[:, None, None]
    s = np.where(v % 2 == 0, x, y) // 2 % 2  # view 0: vertical stripes, view 1: horizontal
    L = 30 + 40.0 * s + rng.uniform(-amp, amp, (V, H, W))
    return _stack(L, rng.uniform(-amp, amp, (V, H, W)), rng.uniform(-amp, amp, (V, H, W)), ("stripes",))


def step(V, H, W, at):
    """view 0: L jumps at column `at`; view 1: at row `at`; no noise, so the
    edge magnitude repeats exactly along the step."""
    y, x = np.mgrid[0:H, 0:W]
    v = np.arange(V)[:, None, None]
    L = np.where(np.where(v % 2 == 0, x, y) < at, 20.0, 80.0)
    return _stack(L, 4.0 + 0 * L, -3.0 * v + 0 * L, ("step",))


# ---- the case table -----------------------------------------------------------------------------
TILES9 = {"MVS_SLIC_TILES9": "1"}
UPDATE0 = {"MVS_SLIC_UPDATE": "0"}


def _c(kind, build, S, no_iter=3, search=0, conn=False, edge=0, weight=0.6, passes=None, legal=True):
    """env: the knob settings every case runs under besides the default -- the 9-cell k_assign_tiles where
    k_assign_tiles4 would run (the 2x2 loop at S = 32, 64), k_update where k_update_walk would (off the tile path)."""
    env = (TILES9,) if S in (32, 64) and not search else (UPDATE0,) if S % 16 else ()
    return dict(kind=kind, build=build, S=S, weight=weight, no_iter=no_iter, search=search, conn=conn, edge=edge,
                env=env, passes=passes, legal=legal)

CASES = {}
# near ties: k_assign<false> (S = 8, 40), k_assign<true> (S = 8, search 1), k_assign_tiles4<2>, <4> (32, 64; with
# MVS_SLIC_TILES9 k_assign_tiles<false>), k_assign_tiles<false> (16, 48), k_assign_tiles<true> (16, 48 with
# search 1: the nine candidates on the tile path).  The seeds are the first whose first assignment meets
# test_slic_content_cpu's floors (searched on the oracle).  name: (S, W, H, seed, search)
NEAR_TIE = {"near_s8": (8, 100, 70, 16, 0), "near_s40": (40, 250, 170, 1, 0), "near_s8_search1": (8, 100, 70, 9, 1),
            "near_s32": (32, 200, 150, 8, 0), "near_s64": (64, 330, 250, 0, 0), "near_s16": (16, 130, 90, 0, 0),
            "near_s48": (48, 250, 200, 1, 0), "near_s16_search1": (16, 130, 90, 0, 1),
            "near_s48_search1": (48, 250, 200, 1, 1)}
for _n, (_S, _W, _H, _seed, _search) in NEAR_TIE.items():
    CASES[_n] = _c("near", functools.partial(near_tie, 2, _H, _W, _seed), _S, search=_search)
# exact ties: W and H multiples of S, so the pixels on a cell's first column / row are equidistant
for _S, _W, _H in ((8, 64, 48), (16, 96, 64), (32, 128, 96), (64, 192, 128)):
    CASES[f"flat_s{_S}"] = _c("flat", functools.partial(flat, 2, _H, _W), _S)
# empty superpixels: walk / k_update (8), k_update_finalize<6> (32), k_update_finalize<0> (16, 48, 64)
# (0 < H mod S <= S/2 as well: no pixel then has the bottom right cell among its candidates but its own,
# which join the cell to their left)
for _S, _W, _H in ((8, 100, 66), (32, 208, 136), (16, 136, 84), (48, 264, 200), (64, 352, 208)):
    CASES[f"empty_s{_S}"] = _c("empty", functools.partial(empty, 2, _H, _W, _S), _S)
# tile membership: full tiles and one-member tiles on the tile route (16, 32) and the window walk (40)
for _S, _W, _H in ((16, 130, 90), (32, 200, 150), (40, 250, 170)):
    CASES[f"blocks_s{_S}"] = _c("blocks", functools.partial(blocks, 2, _H, _W, _S), _S)
# small and ragged maps: (S, W, H)
RAGGED = [(8, 5, 4), (6, 6, 6), (8, 7, 50), (8, 50, 7), (16, 10, 40), (16, 40, 10), (32, 20, 90), (32, 75, 50),
          (8, 41, 44), (8, 44, 45), (8, 45, 47), (8, 47, 41),
          (16, 65, 72), (16, 72, 73), (16, 73, 79), (16, 79, 65),
          (32, 97, 80), (32, 80, 113), (32, 113, 127), (32, 127, 97), (12, 90, 61), (48, 100, 130), (64, 70, 200)]
for _S, _W, _H in RAGGED:
    CASES[f"ragged_s{_S}_{_W}x{_H}"] = _c("ragged", functools.partial(noise, 2, _H, _W, _S), _S, no_iter=2)
# more than 65,536 cells: the uint32_t forms of k_update / k_update_walk (UT = 1 at S = 6, 4 at S = 12);
# 1536 x 1536 at S = 6 has exactly 65,536: the last map that takes the 16-bit copies
for _n, _S, _W, _H in (("l32_s6", 6, 1542, 1536), ("l32_s12", 12, 3084, 3072), ("l16_s6", 6, 1536, 1536)):
    CASES[_n] = _c("labels32", functools.partial(pattern, 1, _H, _W), _S, no_iter=2, passes=(1, 2))
# suppression
for _S, _W, _H, _amp in ((8, 100, 70, 12.0), (32, 200, 150, 12.0)):
    CASES[f"suppress_s{_S}"] = _c("suppress", functools.partial(stripes, 2, _H, _W, _amp), _S, no_iter=2, conn=True)
# edge modes on built Lab
for _m in (1, 2):
    CASES[f"edge{_m}_flat"] = _c("edge_flat", functools.partial(flat, 2, 48, 64), 8, no_iter=1, edge=_m)
    CASES[f"edge{_m}_step_s8"] = _c("edge_step", functools.partial(step, 2, 48, 64, 12), 8, no_iter=2, edge=_m)
    CASES[f"edge{_m}_step_s16"] = _c("edge_step", functools.partial(step, 2, 64, 96, 24), 16, no_iter=2, edge=_m)
    # H < S and W = 8 k + 1: every centre on the last row, the last column's on the last column
    CASES[f"edge{_m}_border"] = _c("edge_border", functools.partial(noise, 2, 2, 41, "border"), 8, no_iter=2, edge=_m)
    CASES[f"edge{_m}_noise_s32"] = _c("edge_noise", functools.partial(noise, 2, 70, 100, "edge"), 32, no_iter=2,
                                      edge=_m)
# the widest and tallest images mvs_slic_d takes: the walk, the 9-cell tiles, tiles4
for _n, _S, _W, _H in (("legal_w_s7", 7, MAX_DIM, 8), ("legal_w_s16", 16, MAX_DIM, 20),
                       ("legal_w_s32", 32, MAX_DIM, 40), ("legal_h_s32", 32, 40, MAX_DIM)):
    CASES[_n] = _c("legal", functools.partial(noise, 1, _H, _W, _n), _S, no_iter=2)
# beyond the bound: strips wide enough that a tile's sum of member x is no longer exact in float.  (At S = 7
# a window tile holds some 50 members, so the walk's strip is 2^20 wide where 2^18 serves the tile routes.)
WIDE = {"wide_walk": (7, 1048592, 8), "wide_tiles9": (16, 262160, 20), "wide_tiles4": (32, 262160, 40)}  # S, W, H
for _n, (_S, _W, _H) in WIDE.items():
    CASES[_n] = _c("wide", functools.partial(noise, 1, _H, _W, _n), _S, no_iter=1, legal=False)


@functools.lru_cache(maxsize=6)
def lab(name):
    """The case's Lab stack, float32 [V, H, W, 4] (read only)."""
    a = CASES[name]["build"]()
    a.setflags(write=False)
    return a


def passes(name):
    """The iteration counts the GPU tests compare a case at."""
    c = CASES[name]
    return tuple(sorted({0, 1, 2, c["no_iter"]})) if c["passes"] is None else c["passes"]


_ORACLE = {}


def oracle(name, no_iter=None):
    """orc.slic_from_lab of every view, once per (case, no_iter): a list of
    (spixl, labels) or, with edge mode 1, (spixl, labels, lab)."""
    c = CASES[name]
    no_iter = c["no_iter"] if no_iter is None else no_iter
    if (name, no_iter) not in _ORACLE:
        L = lab(name)
        _ORACLE[name, no_iter] = [orc.slic_from_lab(L[v], c["S"], c["weight"], no_iter, c["conn"], c["search"],
                                                    c["edge"]) for v in range(L.shape[0])]
    return _ORACLE[name, no_iter]


# ---- restatements -------------------------------------------------------------------------------
def cand_d2(lab1, sp, S, weight=0.6, search=0):
    """find_center_association's candidates for every pixel of one view, in
    loop order: (d2 [K, H, W] float32 -- slic_dist's argument of sqrtf, NaN for
    a cell outside the map --, ids [K, H, W])."""
    H, W = lab1.shape[:2]
    mh, mw = sp.shape[:2]
    y, x = np.mgrid[0:H, 0:W]
    cxg, cyg = x // S, y // S
    dX, dY = (x + S // 2) // S - cxg, (y + S // 2) // S - cyg
    xy = f32(1.0) / (f32(1.4242) * f32(S))
    col = f32(15.0) / (f32(1.7321) * f32(128.0))
    sn, cn, w = xy * xy, col * col, f32(weight)
    xf, yf = x.astype(f32), y.astype(f32)
    flat_sp = np.ascontiguousarray(sp, f32).reshape(-1, 8)
    nc = 3 if search else 2
    d2s, ids = [], []
    for ii in range(nc):
        for jj in range(nc):
            ox, oy = (jj - 1, ii - 1) if search else (jj - 1 + dY, ii - 1 + dX)  # (the reference swaps the deltas)
            cx, cy = cxg + ox, cyg + oy
            ok = (cx >= 0) & (cy >= 0) & (cx < mw) & (cy < mh)
            ci = np.where(ok, cy * mw + cx, 0)
            c = flat_sp[ci]
            a = (lab1[..., 0] - c[..., 3]) * (lab1[..., 0] - c[..., 3])
            a = a + (lab1[..., 1] - c[..., 4]) * (lab1[..., 1] - c[..., 4])
            a = a + (lab1[..., 2] - c[..., 5]) * (lab1[..., 2] - c[..., 5])
            b = (xf - c[..., 1]) * (xf - c[..., 1])
            b = b + (yf - c[..., 2]) * (yf - c[..., 2])
            d = (a * cn) + w * (b * sn)
            assert d.dtype == f32
            d2s.append(np.where(ok, d, f32(np.nan)))
            ids.append(np.where(ok, cy * mw + cx, -1))
    return np.stack(d2s), np.stack(ids)


def tie_stats(lab1, sp, S, weight=0.6, search=0):
    """Per pixel of one assignment: near (some candidate's d2 lies above the
    least, within the kernels' factor of it), first (the label of the first
    candidate of least d2), ref (the reference's loop: strict < on sqrtf(d2),
    starting from 999999.9999f) and the candidates' d2 / ids."""
    d2, ids = cand_d2(lab1, sp, S, weight, search)
    with np.errstate(invalid="ignore"):
        lo = np.nanmin(d2, 0)
        near = ((d2 > lo) & (d2 * NEAR <= lo)).any(0)
        k = np.argmax(d2 == lo, 0)
        first = np.take_along_axis(ids, k[None], 0)[0]
        best = np.full(lo.shape, f32(999999.9999), f32)
        ref = np.full(lo.shape, -1, np.int64)
        for q in range(len(d2)):
            d = np.sqrt(d2[q])
            take = d < best  # (NaN: False)
            best, ref = np.where(take, d, best), np.where(take, ids[q], ref)
    return dict(near=near, first=first, ref=ref, d2=d2, ids=ids, lo=lo)


def window_tiles(labels, S, sps=None):
    """update_cluster_center's 16 x 16 window tiles for one view's labels:
    yields (t, mem [N, 256] bool, px [N, 256], py [N, 256]) per tile index t,
    over the N superpixels `sps` (default: all mw * mh), local index k = 16 ly + lx."""
    H, W = labels.shape
    mw, mh = orc.map_size(W, H, S)
    G = int(np.ceil(f32(S * S * 9) / f32(256)))
    cpl = S * 3 // 16
    sp = np.arange(mw * mh) if sps is None else np.asarray(sps)
    gx, gy = sp % mw, sp // mw
    l16 = np.arange(16)
    flat_lb = labels.ravel()
    for t in range(G):
        nbx, nby = t % cpl, t // cpl
        pxo, pyo = nbx * 16 + l16, nby * 16 + l16
        px = (gx * S - S)[:, None] + pxo[None]
        py = (gy * S - S)[:, None] + pyo[None]
        vx = (pxo < 3 * S)[None] & (px >= 0) & (px < W)
        vy = (pyo < 3 * S)[None] & (py >= 0) & (py < H)
        idx = np.clip(py, 0, H - 1)[:, :, None] * W + np.clip(px, 0, W - 1)[:, None, :]
        mem = vy[:, :, None] & vx[:, None, :] & (flat_lb[idx] == sp[:, None, None])
        n = len(sp)
        yield (t, mem.reshape(n, 256), np.broadcast_to(px[:, None, :], (n, 16, 16)).reshape(n, 256),
               np.broadcast_to(py[:, :, None], (n, 16, 16)).reshape(n, 256))


def tree256(v):
    """The reference's LDS tree over the last axis (256): v[k] += v[k + i], i = 128 .. 1, in float32."""
    v = np.array(v, f32)
    i = 128
    while i:
        v[..., :i] = v[..., :i] + v[..., i:2 * i]
        i //= 2
    return v[..., 0]


def tile_counts(labels, S):
    """-> (full, single): the (superpixel, tile) pairs with 256 members and with exactly one."""
    full = single = 0
    for _, mem, _, _ in window_tiles(labels, S):
        n = mem.sum(1)
        full += int((n == 256).sum())
        single += int((n == 1).sum())
    return full, single


def inexact_tile_sums(labels, S, axis=0, sps=None):
    """The (superpixel, tile) pairs whose sum of member x (axis 0) or y (axis 1)
    as ONE integer rounded to float differs from the reference's float tree --
    the pairs at which the kernels' integer tile sums leave the reference."""
    bad = pairs = 0
    for _, mem, px, py in window_tiles(labels, S, sps):
        p = px if axis == 0 else py
        exact = np.where(mem, p, 0).sum(1)
        tree = tree256(np.where(mem, p, 0))
        bad += int((exact.astype(f32) != tree).sum())
        pairs += int(mem.any(1).sum())
    return bad, pairs


def suppress_counts(labels):
    """Per interior pixel of supress_local_lable's 5 x 5 window: (cnt -- the
    neighbours whose label differs --, kinds -- how many distinct labels they
    carry, up to 3 counted), both 0 on the 2-pixel border."""
    H, W = labels.shape
    lb = labels.astype(np.int64)
    cnt = np.zeros((H, W), np.int64)
    kinds = np.zeros((H, W), np.int64)
    if H < 5 or W < 5:
        return cnt, kinds
    c = lb[2:-2, 2:-2]
    a = np.full(c.shape, -1, np.int64)
    b = np.full(c.shape, -1, np.int64)
    k3 = np.zeros(c.shape, bool)
    for j in range(5):
        for i in range(5):
            n = lb[j:H - 4 + j, i:W - 4 + i]
            d = n != c
            cnt[2:-2, 2:-2] += d
            new_a = d & (a < 0)
            a = np.where(new_a, n, a)
            new_b = d & (n != a) & (b < 0)
            b = np.where(new_b, n, b)
            k3 |= d & (n != a) & (n != b)
    kinds[2:-2, 2:-2] = (a >= 0).astype(np.int64) + (b >= 0) + k3
    return cnt, kinds
