"""Device-side stage API on torch tensors, backed by libmvs.so (HIP, gfx950).

torch supplies device memory, the HIP stream and ``torch.distributed``; every
compute step is a hand-written HIP kernel reached through the C-ABI in
include/mvs.h.  Tensors are in the reference layouts:

    rgbx   uint8   [V, H, W, 4]     lab    float32 [V, H, W, 4]
    spixl  float32 [V, mh, mw, 8]   labels int32   [V, H, W] (uint32 bits; the refinement
                                    and fusion also take 16-bit maps)
    rep    uint8   [V, mh, mw, 8]   state  float32 [V, mh, mw, 6]
    disp   float32 [V, H, W]
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .params import map_size


def _ptr(t: torch.Tensor | None):
    if t is None:
        return None
    if not t.is_cuda:
        raise ValueError("libmvs device API needs CUDA (HIP) tensors")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return C.c_void_p(t.data_ptr())


def _label_fn(L, name: str, labels: torch.Tensor):
    """The uint32 entry point `name`_d, or its 16-bit twin `name`_l16_d for
    int16/uint16 label maps (the narrowed all-gather's; bits read unsigned)."""
    if labels.dtype == torch.int32:
        return getattr(L, name + "_d")
    if labels.dtype in (torch.int16, torch.uint16):
        return getattr(L, name + "_l16_d")
    raise ValueError(f"labels must be int32 or 16-bit, not {labels.dtype}")


def _runs(views):
    """Sorted view ids -> contiguous [v0, v1) runs."""
    vs = sorted(set(int(v) for v in views))
    runs = []
    for v in vs:
        if runs and runs[-1][1] == v:
            runs[-1][1] = v + 1
        else:
            runs.append([v, v + 1])
    return [tuple(r) for r in runs]


@dataclass
class CameraArray:
    """Host-side camera-array metadata (pipeline::perform_depth_est)."""
    array_width: int
    bl_ratio: float
    levels: np.ndarray        # float32 [D]
    view_subset: np.ndarray   # int32 [V, V]
    subset_num: np.ndarray    # int32 [V]

    def __post_init__(self):
        self.levels = np.ascontiguousarray(self.levels, np.float32)
        self.view_subset = np.ascontiguousarray(self.view_subset, np.int32)
        self.subset_num = np.ascontiguousarray(self.subset_num, np.int32)
        self._desc = _lib.ArrayDesc(
            int(self.subset_num.shape[0]), int(self.array_width), float(self.bl_ratio),
            self.levels.ctypes.data_as(C.POINTER(C.c_float)), int(self.levels.shape[0]),
            self.view_subset.ctypes.data_as(C.POINTER(C.c_int32)),
            self.subset_num.ctypes.data_as(C.POINTER(C.c_int32)))

    @property
    def view_count(self) -> int:
        return int(self.subset_num.shape[0])

    @property
    def D(self) -> int:
        return int(self.levels.shape[0])

    def views_needed(self, z0: int, z1: int) -> list[int]:
        """Reference views [z0, z1) and every view their neighbour lists name:
        the views whose images a shard owning [z0, z1) reads."""
        need = set(range(z0, z1))
        for z in range(z0, z1):
            need.update(int(v) for v in self.view_subset[z, :int(self.subset_num[z])])
        return sorted(need)

    def desc(self):
        return C.byref(self._desc)


class Engine:
    """One libmvs context on one GPU (one process per GPU)."""

    def __init__(self, device: int = 0):
        self.L = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.MvsError("no GPU visible: the MI355X engine has no CPU fallback")
        self.device = torch.device("cuda", device)
        ctx = C.c_void_p()
        _lib.check(self.L.mvs_create(device, C.byref(ctx)), "mvs_create")
        self.ctx = ctx
        self._levels_dev = {}

    def close(self):
        if self.ctx:
            self.L.mvs_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _stream(self):
        s = torch.cuda.current_stream(self.device).cuda_stream
        self.L.mvs_set_stream(self.ctx, C.c_void_p(s))

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.device)

    # ---- SLIC -------------------------------------------------------------
    def cvt(self, rgbx: torch.Tensor, want_l8: bool = True):
        V, H, W, _ = rgbx.shape
        lab = self.empty((V, H, W, 4), torch.float32)
        l8 = self.empty((V, H, W), torch.uint8) if want_l8 else None
        self._stream()
        _lib.check(self.L.mvs_cvt_d(self.ctx, _ptr(rgbx), V, W, H, _ptr(lab), _ptr(l8)), "mvs_cvt_d")
        return lab, l8

    def cvt_views(self, rgbx: torch.Tensor, views, lab: torch.Tensor, l8: torch.Tensor | None = None):
        """cvt of the listed views only, into full-size [V, ...] lab / l8 (a view
        shard converts its block and the block's neighbours)."""
        V, H, W, _ = rgbx.shape
        self._stream()
        for v0, v1 in _runs(views):
            _lib.check(self.L.mvs_cvt_d(self.ctx, _ptr(rgbx[v0:v1]), v1 - v0, W, H, _ptr(lab[v0:v1]),
                                        None if l8 is None else _ptr(l8[v0:v1])), "mvs_cvt_d")
        return lab, l8

    def slic(self, lab: torch.Tensor, S: int, weight: float = 0.6, no_iter: int = 5, enforce_connectivity=False,
             spixl=None, labels=None, edge_enable: int = 0, search: int = 0):
        """mvs_slic_d.  edge_enable (include/mvs.h): 0 off, 1 the reference's
        apply_edge_values as it behaves (overwrites `lab` in place), 2 the
        intended centre perturbation.  search: 0 the reference's active 2x2
        candidate loop, 1 the 3x3 loop behind its comment switch."""
        V, H, W, _ = lab.shape
        mw, mh = map_size(W, H, S)
        # s7 (disparity) is never written by the reference's SLIC (clcode.cl:285-293);
        # k_init_centers zeroes it, so every word of spixl is written
        spixl = self.empty((V, mh, mw, 8), torch.float32) if spixl is None else spixl
        labels = self.empty((V, H, W), torch.int32) if labels is None else labels
        if spixl.shape != (V, mh, mw, 8) or labels.shape != (V, H, W):
            raise ValueError("slic: output shapes do not match")
        p = _lib.SlicParams(int(S), float(weight), int(no_iter), int(bool(enforce_connectivity)), int(edge_enable),
                            int(search))
        self._stream()
        _lib.check(self.L.mvs_slic_d(self.ctx, _ptr(lab), V, W, H, C.byref(p), _ptr(spixl), _ptr(labels)),
                   "mvs_slic_d")
        return spixl, labels

    def grid(self, lab: torch.Tensor, S: int):
        V, H, W, _ = lab.shape
        mw, mh = map_size(W, H, S)
        spixl = self.empty((V, mh, mw, 8), torch.float32)  # every word written (s7 = 0)
        labels = self.empty((V, H, W), torch.int32)
        self._stream()
        _lib.check(self.L.mvs_grid_d(self.ctx, _ptr(lab), V, W, H, S, _ptr(spixl), _ptr(labels)), "mvs_grid_d")
        return spixl, labels

    # ---- photo-consistency ----------------------------------------------
    def boundary(self, spixl: torch.Tensor, labels: torch.Tensor, S: int):
        V, H, W = labels.shape
        mw, mh = map_size(W, H, S)
        rep = self.empty((V, mh, mw, 8), torch.uint8)
        self._stream()
        _lib.check(self.L.mvs_boundary_d(self.ctx, V, W, H, S, _ptr(spixl), _ptr(labels), _ptr(rep)),
                   "mvs_boundary_d")
        return rep

    def sweep_spixl(self, lab, spixl, rep, cam: CameraArray, S: int, z0: int = 0, z1: int | None = None):
        """initial_depth_estimation_v2 in place on spixl[..., 7]."""
        V, H, W, _ = lab.shape
        z1 = V if z1 is None else z1
        self._stream()
        _lib.check(self.L.mvs_sweep_spixl_d(self.ctx, W, H, S, _ptr(lab), _ptr(spixl), _ptr(rep), cam.desc(), z0, z1),
                   "mvs_sweep_spixl_d")
        return spixl

    def sweep_last_variant(self) -> dict:
        """The last sweep_spixl launch: FORM (0 general gathers, 1 HZ gathers, 2 HZ
        ring, 3 re-laid copies), LPS (lanes per superpixel, 32 | 64), WPS (waves per
        superpixel), TMODE (MVS_SWEEP_TRANSPOSE in effect), RELAID ((view, kind)
        copies built; 0: none needed, or the scratch fell back)."""
        v = (C.c_int32 * 5)()
        if self.L.mvs_sweep_last_variant_n(self.ctx, v, 5) != 5:
            raise _lib.MvsError("mvs_sweep_last_variant_n: unexpected slot count")
        return dict(zip(("FORM", "LPS", "WPS", "TMODE", "RELAID"), list(v)))

    def sweep_pixel_sad(self, lab, cam: CameraArray, z0: int = 0, z1: int | None = None, out=None):
        V, H, W, _ = lab.shape
        z1 = V if z1 is None else z1
        out = self.empty((z1 - z0, H, W), torch.float32) if out is None else out
        self._stream()
        _lib.check(self.L.mvs_sweep_pixel_sad_d(self.ctx, W, H, _ptr(lab), cam.desc(), z0, z1, _ptr(out)),
                   "mvs_sweep_pixel_sad_d")
        return out

    def box_stats(self, l8, K: int = 5, out=None):
        V, H, W = l8.shape
        # [0] window stats {S, bits(1/var | NaN)}, [1] packed intensities {lo, hi};
        # rows pairwise interleaved over Hp = H rounded up to even (include/mvs.h)
        out = self.empty((2, V, H + (H & 1), W, 2), torch.int32) if out is None else out
        self._stream()
        _lib.check(self.L.mvs_box_stats_d(self.ctx, _ptr(l8), V, W, H, K, _ptr(out)), "mvs_box_stats_d")
        return out

    def box_stats_views(self, l8, K: int, views, out):
        """Window planes of the listed views only, into a full V-view buffer."""
        V, H, W = l8.shape
        self._stream()
        for v0, v1 in _runs(views):
            _lib.check(self.L.mvs_box_stats_range_d(self.ctx, _ptr(l8), V, W, H, K, v0, v1, _ptr(out)),
                       "mvs_box_stats_range_d")
        return out

    def set_ncc_variant(self, waves: int = 0, levels_per_wave: int = 0, band_w: int = 0, general_rows: bool = False):
        """Force the NCC sweep variant tried first (0 = automatic; test / tuning hook)."""
        _lib.check(self.L.mvs_set_ncc_variant(self.ctx, int(waves), int(levels_per_wave), int(band_w),
                                              int(bool(general_rows))), "mvs_set_ncc_variant")

    def set_kernel_timing(self, on: bool) -> None:
        """Record start / stop events of every fused NCC sweep launch's own dispatch (bench aid)."""
        _lib.check(self.L.mvs_set_kernel_timing(self.ctx, int(bool(on))), "mvs_set_kernel_timing")

    def kernel_times(self, cap: int = 8192) -> list:
        """The recorded fused-sweep launches' kernel times in ms (waits for them; starts a new record)."""
        buf = (C.c_float * cap)()
        n = C.c_int(0)
        rc = self.L.mvs_kernel_times(self.ctx, buf, cap, C.byref(n))
        if rc != 0 and n.value > cap:
            return self.kernel_times(n.value)  # the record is kept: read it whole
        _lib.check(rc, "mvs_kernel_times")
        return list(buf[:n.value])

    def ncc_last_variant(self) -> dict:
        """The last NCC launch: K, tile rows, levels per wave, waves, band width,
        PAR (row parity: 0 mixed, 1 every band row pair-aligned, 2 odd pk / even
        stats rows), FUSE, NB (band buffers: 1 single, 2 double)."""
        v = (C.c_int32 * 8)()
        if self.L.mvs_ncc_last_variant_n(self.ctx, v, 8) != 8:
            raise _lib.MvsError("mvs_ncc_last_variant_n: unexpected slot count")
        return dict(zip(("K", "TH", "DPW", "NW", "BW", "PAR", "FUSE", "NB"), list(v)))

    def ncc_volume(self, l8, box, cam: CameraArray, z: int, K: int = 5, out=None):
        V, H, W = l8.shape
        out = self.empty((cam.D, H, W), torch.float32) if out is None else out
        self._stream()
        _lib.check(self.L.mvs_ncc_volume_d(self.ctx, W, H, _ptr(l8), _ptr(box), cam.desc(), K, z, _ptr(out)),
                   "mvs_ncc_volume_d")
        return out

    def ncc_wta(self, l8, box, cam: CameraArray, z: int, K: int = 5, disp=None, conf=None, want_conf: bool = True):
        """ncc_volume + wta in one kernel: the volume never reaches HBM (bit-identical)."""
        V, H, W = l8.shape
        disp = self.empty((H, W), torch.float32) if disp is None else disp
        if want_conf and conf is None:
            conf = self.empty((H, W), torch.float32)
        self._stream()
        _lib.check(self.L.mvs_ncc_wta_d(self.ctx, W, H, _ptr(l8), _ptr(box), cam.desc(), K, z, _ptr(disp),
                                        _ptr(conf) if want_conf else None), "mvs_ncc_wta_d")
        return disp, conf

    def ncc_wta_range(self, l8, box, cam: CameraArray, z0: int, z1: int, K: int = 5, disp=None, conf=None,
                      want_conf: bool = True):
        """ncc_wta for reference views [z0, z1) into disp/conf [z1 - z0, H, W]; views sharing a
        sweep variant go in one launch (bit-identical to one ncc_wta per view)."""
        V, H, W = l8.shape
        n = z1 - z0
        disp = self.empty((n, H, W), torch.float32) if disp is None else disp
        if want_conf and conf is None:
            conf = self.empty((n, H, W), torch.float32)
        for t in (disp, conf) if want_conf else (disp,):
            if tuple(t.shape) != (n, H, W) or not t.is_contiguous():
                raise ValueError("disp / conf must be contiguous [z1 - z0, H, W]")
        self._stream()
        _lib.check(self.L.mvs_ncc_wta_range_d(self.ctx, W, H, _ptr(l8), _ptr(box), cam.desc(), K, z0, z1,
                                              _ptr(disp), _ptr(conf) if want_conf else None),
                   "mvs_ncc_wta_range_d")
        return disp, conf

    def levels_dev(self, cam: CameraArray) -> torch.Tensor:
        key = cam.levels.tobytes()
        t = self._levels_dev.get(key)
        if t is None:
            t = torch.from_numpy(cam.levels.copy()).to(self.device)
            self._levels_dev[key] = t
        return t

    def _wta_call(self, name, vol, levels, disp, conf, want_conf):
        """wta and wta_u16: the winner pass `name` over vol [D, H, W]."""
        D, H, W = vol.shape
        disp = self.empty((H, W), torch.float32) if disp is None else disp
        if want_conf and conf is None:
            conf = self.empty((H, W), torch.float32)
        self._stream()
        _lib.check(getattr(self.L, name)(self.ctx, W, H, D, _ptr(vol), _ptr(levels), _ptr(disp),
                                         _ptr(conf) if want_conf else None), name)
        return disp, conf

    def wta(self, vol, levels: torch.Tensor, disp=None, conf=None, want_conf: bool = True):
        return self._wta_call("mvs_wta_d", vol, levels, disp, conf, want_conf)

    def wta_sub(self, vol, levels: torch.Tensor, out=None):
        """Sub-level disparity over a materialised volume [D, H, W]: the parabola fit through
        the winner's cost and its two neighbours' in level order (include/mvs.h)."""
        D, H, W = vol.shape
        out = self.empty((H, W), torch.float32) if out is None else out
        if tuple(out.shape) != (H, W) or tuple(levels.shape) != (D,):
            raise ValueError("wta_sub: out must be [H, W], levels [D]")
        self._stream()
        _lib.check(self.L.mvs_wta_sub_d(self.ctx, W, H, D, _ptr(vol), _ptr(levels), _ptr(out)), "mvs_wta_sub_d")
        return out

    def sgm(self, vol, P1: float = 0.1, P2: float = 0.8, paths: int = 15, out=None):
        """Semi-global aggregation of a volume [D, H, W] (include/mvs.h at mvs_sgm_d): the path
        costs of the paths in the mask (1 left->right, 2 right->left, 4 top->bottom, 8 bottom->top;
        16 down-right, 32 up-left, 64 down-left, 128 up-right: mvs_sgm8_d, called for masks above
        15 only) summed in bit order into out [D, H, W], which must not be vol.  wta on the result
        gives the aggregated disparity and confidence."""
        D, H, W = vol.shape
        out = self.empty((D, H, W), torch.float32) if out is None else out
        if tuple(out.shape) != (D, H, W) or vol.dtype != torch.float32 or out.dtype != torch.float32:
            raise ValueError("sgm: vol and out must be float32 [D, H, W]")
        self._stream()
        name = "mvs_sgm_d" if int(paths) <= 15 else "mvs_sgm8_d"
        _lib.check(getattr(self.L, name)(self.ctx, W, H, D, _ptr(vol), C.c_float(P1), C.c_float(P2), int(paths),
                                         _ptr(out)), name)
        return out

    def _sgm_batch_call(self, name, what, dtypes, tname, vols, P1, P2, paths, out):
        """sgm_batch and sgm_u16_batch: the entry point `name` on vols and out of a dtype in dtypes (tname in the
        messages; an out made here has dtypes[0]), with the penalties as the entry point takes them."""
        if vols.dim() != 4 or vols.dtype not in dtypes:
            raise ValueError(f"{what}: vols must be {tname} [N, D, H, W]")
        N, D, H, W = vols.shape
        if N < 1:
            raise ValueError(f"{what}: vols holds no volume")
        out = self.empty((N, D, H, W), dtypes[0]) if out is None else out
        if tuple(out.shape) != (N, D, H, W) or out.dtype not in dtypes:
            raise ValueError(f"{what}: out must be {tname} [N, D, H, W]")
        for t in (vols, out):
            if not t[0].is_contiguous() or (N > 1 and t.stride(0) < D * H * W):
                raise ValueError(f"{what}: every element must be contiguous, with stride(0) >= D * H * W")
        self._stream()
        # (at N = 1 a tensor's stride(0) is arbitrary and is not read)
        vs, os_ = (D * H * W, D * H * W) if N == 1 else (vols.stride(0), out.stride(0))
        _lib.check(getattr(self.L, name)(self.ctx, W, H, D, N, _ptr(vols[0]), vs, P1, P2, int(paths), _ptr(out[0]),
                                         os_), name)
        return out

    def sgm_batch(self, vols, P1: float = 0.1, P2: float = 0.8, paths: int = 15, out=None):
        """sgm of N volumes of one shape in one call (include/mvs.h at mvs_sgm8_batch_d): vols
        float32 [N, D, H, W], one launch per path over all N; out[i] holds the bits sgm(vols[i])
        gives.  Each vols[i] is contiguous and stride(0) >= D * H * W (a view into a padded buffer
        is allowed); out obeys the same rule and must not overlap vols, gaps included.  vols and
        out together are 2 * N * 4 * D * H * W bytes."""
        return self._sgm_batch_call("mvs_sgm8_batch_d", "sgm_batch", (torch.float32,), "float32", vols, P1, P2, paths,
                                    out)

    # ---- semi-global aggregation on 16-bit integer costs (include/mvs.h at mvs_sgm8_u16_batch_d) ----
    # The tensors are torch.uint16 (this torch build allocates it and gives its data_ptr; empty() here makes
    # uint16); torch.int16 tensors, the same bits viewed, are accepted as well.
    U16 = (torch.uint16, torch.int16)

    def quant_u16(self, vol, out=None):
        """float32 costs -> uint16: rint_to_even(min(max(c, 0), 2) * 2047) (mvs_quant_u16_d).  vol is
        contiguous float32 of any shape; out has the same shape, uint16 (or int16-viewed)."""
        if vol.dtype != torch.float32 or not vol.is_contiguous():
            raise ValueError("quant_u16: vol must be contiguous float32")
        out = self.empty(tuple(vol.shape), torch.uint16) if out is None else out
        if tuple(out.shape) != tuple(vol.shape) or out.dtype not in self.U16 or not out.is_contiguous():
            raise ValueError("quant_u16: out must be contiguous uint16 of vol's shape")
        self._stream()
        _lib.check(self.L.mvs_quant_u16_d(self.ctx, vol.numel(), _ptr(vol), _ptr(out)), "mvs_quant_u16_d")
        return out

    def sgm_u16_batch(self, vols, P1: int = 205, P2: int = 1638, paths: int = 15, out=None):
        """The aggregate of N uint16 volumes of one shape in one call (mvs_sgm8_u16_batch_d): vols
        [N, D, H, W] with costs <= 4094, integer penalties 0 <= P1 <= P2 <= 4095 (in units of 1 / 2047
        of NCC cost), D <= 256; out[i] is the exact sum of the paths of the mask over vols[i].  The
        layout rules are sgm_batch's, in 2-byte elements; vols and out together are
        2 * N * 2 * D * H * W bytes."""
        if int(P1) != P1 or int(P2) != P2:
            raise ValueError("sgm_u16_batch: the penalties are integers")
        return self._sgm_batch_call("mvs_sgm8_u16_batch_d", "sgm_u16_batch", self.U16, "uint16", vols, int(P1), int(P2),
                                    paths, out)

    def wta_u16(self, agg, levels: torch.Tensor, disp=None, conf=None, want_conf: bool = True):
        """Winner (the first index of the minimum) and confidence ((c2 - best) / 2047) of a uint16
        aggregate [D, H, W] (mvs_wta_u16_d)."""
        if agg.dim() != 3 or agg.dtype not in self.U16:
            raise ValueError("wta_u16: agg must be uint16 [D, H, W]")
        D, H, W = agg.shape
        if tuple(levels.shape) != (D,) or levels.dtype != torch.float32:
            raise ValueError("wta_u16: levels must be float32 [D]")
        for t in (disp, conf) if want_conf else (disp,):  # (one left out is made below, as asked for here)
            if t is not None and (tuple(t.shape) != (H, W) or t.dtype != torch.float32):
                raise ValueError("wta_u16: disp / conf must be float32 [H, W]")
        return self._wta_call("mvs_wta_u16_d", agg, levels, disp, conf, want_conf)

    def _wta_sub_call(self, name, what, agg, raw, levels, disp, conf, out, want_conf):
        D, H, W = agg.shape
        if tuple(raw.shape) != (D, H, W) or raw.dtype != agg.dtype:
            raise ValueError(f"{what}: the raw volume must have agg's shape and dtype")
        if tuple(levels.shape) != (D,) or levels.dtype != torch.float32:
            raise ValueError(f"{what}: levels must be float32 [D]")
        out = self.empty((H, W), torch.float32) if out is None else out
        if want_conf and conf is None:
            conf = self.empty((H, W), torch.float32)
        if not want_conf:
            conf = None
        for t in (disp, conf, out):
            if t is not None and (tuple(t.shape) != (H, W) or t.dtype != torch.float32):
                raise ValueError(f"{what}: disp / conf / out must be float32 [H, W]")
        self._stream()
        _lib.check(getattr(self.L, name)(self.ctx, W, H, D, _ptr(agg), _ptr(raw), _ptr(levels), _ptr(disp), _ptr(conf),
                                         _ptr(out)), name)
        return disp, conf, out

    def wta_agg_sub(self, agg, vol, levels: torch.Tensor, disp=None, conf=None, out=None, want_conf: bool = True):
        """Winner of a float32 aggregate [D, H, W] with the sub-level disparity of that winner: the parabola
        through the costs of the raw volume vol [D, H, W] at the aggregate's winner and its two neighbours, where
        vol has a minimum there (mvs_wta_agg_sub_d).  agg is read once.  Returns (disp, conf, out): out [H, W] is
        the sub-level disparity; disp is written only where a tensor is given (else None), conf unless
        want_conf is False; both hold wta(agg)'s bits."""
        if agg.dim() != 3 or agg.dtype != torch.float32:
            raise ValueError("wta_agg_sub: agg must be float32 [D, H, W]")
        return self._wta_sub_call("mvs_wta_agg_sub_d", "wta_agg_sub", agg, vol, levels, disp, conf, out, want_conf)

    def wta_u16_sub(self, agg, raw, levels: torch.Tensor, disp=None, conf=None, out=None, want_conf: bool = True):
        """wta_agg_sub for a uint16 aggregate and the quantised volume raw it was aggregated from
        (mvs_wta_u16_sub_d): disp and conf hold wta_u16(agg)'s bits."""
        if agg.dim() != 3 or agg.dtype not in self.U16 or raw.dtype not in self.U16:
            raise ValueError("wta_u16_sub: agg and raw must be uint16 [D, H, W]")
        if raw.dtype != agg.dtype:
            raw = raw.view(agg.dtype)
        return self._wta_sub_call("mvs_wta_u16_sub_d", "wta_u16_sub", agg, raw, levels, disp, conf, out, want_conf)

    def ncc_sub_range(self, l8, box, cam: CameraArray, z0: int, z1: int, K: int = 5, disp=None, out=None):
        """The same for reference views [z0, z1) without a volume: disp [z1 - z0, H, W] is what
        ncc_wta_range wrote; the three costs are recomputed from the window planes (bit-identical
        to ncc_volume + wta_sub per view).  out may be disp (in place)."""
        V, H, W = l8.shape
        n = z1 - z0
        if disp is None:
            raise ValueError("ncc_sub_range needs the integer-level disp of ncc_wta_range")
        out = self.empty((n, H, W), torch.float32) if out is None else out
        for t in (disp, out):
            if tuple(t.shape) != (n, H, W) or not t.is_contiguous():
                raise ValueError("disp / out must be contiguous [z1 - z0, H, W]")
        self._stream()
        _lib.check(self.L.mvs_ncc_sub_range_d(self.ctx, W, H, _ptr(l8), _ptr(box), cam.desc(), K, int(z0), int(z1),
                                              _ptr(disp), _ptr(out)), "mvs_ncc_sub_range_d")
        return out

    # ---- refinement ------------------------------------------------------
    def refine(self, spixl, labels, rep, cam: CameraArray, S: int, gamma=2.0, alpha=6.0, fuse=1.0, kernel_step=13,
               kernel_size=1080, no_prop=5, fusion_compat=True, want_disp=True):
        V, H, W = labels.shape
        mw, mh = map_size(W, H, S)
        flat = self.empty((V, mh, mw, 2), torch.float32)
        st = self.empty((V, mh, mw, 6), torch.float32)
        st2 = self.empty((V, mh, mw, 6), torch.float32)
        disp = self.empty((V, H, W), torch.float32) if want_disp else None
        p = _lib.RefineParams(float(gamma), float(alpha), float(fuse), int(kernel_step), int(kernel_size),
                              int(no_prop), int(bool(fusion_compat)))
        self._stream()
        _lib.check(self.L.mvs_refine_d(self.ctx, W, H, S, _ptr(spixl), _ptr(labels), _ptr(rep), cam.desc(),
                                       C.byref(p), _ptr(flat), _ptr(st), _ptr(st2), _ptr(disp)), "mvs_refine_d")
        final = st
        if not fusion_compat and no_prop > 0:
            final = st2 if (no_prop - 1) % 2 == 0 else st
        return {"flat": flat, "state": final, "state_compat": st, "disp": disp}

    def flatness(self, spixl, gamma: float):
        V, mh, mw, _ = spixl.shape
        flat = self.empty((V, mh, mw, 2), torch.float32)
        self._stream()
        _lib.check(self.L.mvs_flatness_d(self.ctx, V, mw, mh, _ptr(spixl), C.c_float(gamma), _ptr(flat)),
                   "mvs_flatness_d")
        return flat

    def init_state(self, spixl, labels, rep, flat, cam: CameraArray, S, gamma, alpha, nks, kss, fuse):
        V, H, W = labels.shape
        mw, mh = map_size(W, H, S)
        st = self.empty((V, mh, mw, 6), torch.float32)
        self._stream()
        _lib.check(self.L.mvs_init_state_d(self.ctx, W, H, S, _ptr(spixl), _ptr(labels), _ptr(rep), _ptr(flat),
                                           cam.desc(), C.c_float(gamma), C.c_float(alpha), int(nks), C.c_float(kss),
                                           C.c_float(fuse), _ptr(st)), "mvs_init_state_d")
        return st

    def init_state_range(self, spixl, labels, rep, flat, cam: CameraArray, S, gamma, alpha, nks, kss, fuse, z0, z1,
                         state=None):
        """init_current_state for views [z0, z1) into a full [V, mh, mw, 6] state.
        labels: int32, or int16/uint16 (16-bit maps, mw * mh <= 65536)."""
        V, H, W = labels.shape
        mw, mh = map_size(W, H, S)
        st = self.empty((V, mh, mw, 6), torch.float32) if state is None else state
        self._stream()
        fn = _label_fn(self.L, "mvs_init_state_range", labels)
        _lib.check(fn(self.ctx, W, H, S, _ptr(spixl), _ptr(labels), _ptr(rep), _ptr(flat),
                                                 cam.desc(), C.c_float(gamma), C.c_float(alpha), int(nks),
                                                 C.c_float(kss), C.c_float(fuse), int(z0), int(z1), _ptr(st)),
                   fn.__name__)
        return st

    def propagate(self, spixl, labels, rep, flat, cam: CameraArray, S, it, alpha, gamma, fuse, nks, kss, st_in,
                  st_out, z0=0, z1=None):
        V, H, W = labels.shape
        z1 = V if z1 is None else z1
        self._stream()
        fn = _label_fn(self.L, "mvs_propagate", labels)
        _lib.check(fn(self.ctx, W, H, S, _ptr(spixl), _ptr(labels), _ptr(rep), _ptr(flat),
                                          cam.desc(), int(it), C.c_float(alpha), C.c_float(gamma), C.c_float(fuse),
                                          int(nks), C.c_float(kss), _ptr(st_in), _ptr(st_out), int(z0), int(z1)),
                   fn.__name__)
        return st_out

    def spixl_to_image(self, spixl, labels, state, S):
        V, H, W = labels.shape
        disp = self.empty((V, H, W), torch.float32)
        self._stream()
        fn = _label_fn(self.L, "mvs_spixl_to_image", labels)
        _lib.check(fn(self.ctx, V, W, H, S, _ptr(spixl), _ptr(labels), _ptr(state), _ptr(disp)), fn.__name__)
        return disp

    def filter(self, disp_full, array_width: int, bl_ratio: float, fuse: float = 1.0, z0: int = 0, z1=None,
               out=None):
        V, H, W = disp_full.shape
        z1 = V if z1 is None else z1
        proj = self.empty((V, H, W), torch.float32)
        out = torch.zeros((V, H, W), dtype=torch.float32, device=self.device) if out is None else out
        self._stream()
        _lib.check(self.L.mvs_filter_d(self.ctx, V, W, H, int(array_width), C.c_float(bl_ratio), C.c_float(fuse),
                                       _ptr(disp_full), _ptr(proj), _ptr(out), int(z0), int(z1)), "mvs_filter_d")
        return proj, out

    def proj_inv(self, disp_full, array_width: int, bl_ratio: float, z0: int, z1: int, proj=None, rows=None,
                 band=False):
        """project_to_reference_inv for references [z0, z1) into proj[z0:z1] ([V, H, W]);
        rows=(y0, y1): image rows [y0, y1) only -- with band=True `proj` is that row
        band alone, [V, y1 - y0, W] (the buffer its all-gather fills)."""
        V, H, W = disp_full.shape
        if band:
            if rows is None or proj is None or tuple(proj.shape) != (V, rows[1] - rows[0], W):
                raise ValueError("band=True needs rows=(y0, y1) and proj of shape [V, y1 - y0, W]")
        proj = self.empty((V, H, W), torch.float32) if proj is None else proj
        self._stream()
        if rows is None:
            _lib.check(self.L.mvs_proj_inv_d(self.ctx, V, W, H, int(array_width), C.c_float(bl_ratio),
                                             _ptr(disp_full), _ptr(proj), int(z0), int(z1)), "mvs_proj_inv_d")
        else:
            _lib.check(self.L.mvs_proj_inv_rows_d(self.ctx, V, W, H, int(array_width), C.c_float(bl_ratio),
                                                  _ptr(disp_full), _ptr(proj), int(bool(band)), int(z0), int(z1),
                                                  int(rows[0]), int(rows[1])), "mvs_proj_inv_rows_d")
        return proj

    def remove_inconsistency(self, disp_full, proj, array_width: int, bl_ratio: float, fuse: float, z0: int, z1: int,
                             out=None, rows=None, band=False):
        """remove_view_inconsistency for references [z0, z1) (every proj slice filled; rows=(y0, y1):
        image rows [y0, y1) only, which read only those rows of proj -- with band=True `proj` is
        that row band alone, [V, y1 - y0, W])."""
        V, H, W = disp_full.shape
        out = torch.zeros((V, H, W), dtype=torch.float32, device=self.device) if out is None else out
        if band and (rows is None or tuple(proj.shape) != (V, rows[1] - rows[0], W)):
            raise ValueError("band=True needs rows=(y0, y1) and proj of shape [V, y1 - y0, W]")
        self._stream()
        if rows is None:
            _lib.check(self.L.mvs_remove_inconsistency_d(self.ctx, V, W, H, int(array_width), C.c_float(bl_ratio),
                                                         C.c_float(fuse), _ptr(disp_full), _ptr(proj), _ptr(out),
                                                         int(z0), int(z1)), "mvs_remove_inconsistency_d")
        else:
            _lib.check(self.L.mvs_remove_inconsistency_rows_d(self.ctx, V, W, H, int(array_width),
                                                              C.c_float(bl_ratio), C.c_float(fuse), _ptr(disp_full),
                                                              _ptr(proj), int(bool(band)), _ptr(out), int(z0), int(z1),
                                                              int(rows[0]), int(rows[1])),
                       "mvs_remove_inconsistency_rows_d")
        return out

    def synchronize(self):
        _lib.check(self.L.mvs_synchronize(self.ctx), "mvs_synchronize")
