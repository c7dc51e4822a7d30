"""Host orchestration mirroring the reference's stage classes.

    SLIC              <- clSLIC              (clSLIC.cpp:67-122)
    PhotoConsistency  <- clPhotoConsistency  (photo_consistency.cpp:21-208)
    PixelSweep        <- build-defined per-pixel sweep (NCC KxK / SAD parity)
    DepthRefinement   <- clDepthRefinement   (depth_refinement.cpp:91-1470)
    ConsistencyFilter <- the reference's disabled fusion tail (1374-1453)
    Pipeline          <- pipeline            (pipeline.cpp:7-175)

All buffers live on the GPU for the whole run (HBM-resident stacks); every
stage is a HIP kernel in libmvs.so.  A Pipeline owns a contiguous block of
reference views [z0, z1) so one process per GPU can shard a large array by
reference view (see distributed.py).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import params
from .engine import CameraArray, Engine


class SLIC:
    """clSLIC: cvt + SLIC for a batch of views in one launch per kernel."""

    def __init__(self, engine: Engine, settings: params.Settings):
        self.e = engine
        self.st = settings

    def do_super_pixel_seg(self, rgbx: torch.Tensor):
        lab, l8 = self.e.cvt(rgbx, want_l8=True)
        spixl, labels = self.segment(lab)
        return lab, l8, spixl, labels

    def segment(self, lab: torch.Tensor):
        """The SLIC loop on converted views (everything after cvt)."""
        S = self.st.spixl_size
        if S == 1:
            return self.e.grid(lab, 1)
        return self.e.slic(lab, S, self.st.slic_color_weight, self.st.no_iter, self.st.enforce_connectivity,
                           search=self.st.slic_search)


class PhotoConsistency:
    """clPhotoConsistency::do_initial_depth_estimation: boundary + per-superpixel
    SAD plane sweep, one launch per reference view (photo_consistency.cpp:133)."""

    def __init__(self, engine: Engine, cam: CameraArray, S: int):
        self.e, self.cam, self.S = engine, cam, S

    def do_initial_depth_estimation(self, lab, spixl, labels, z0=0, z1=None):
        rep = self.e.boundary(spixl, labels, self.S)
        self.e.sweep_spixl(lab, spixl, rep, self.cam, self.S, z0, z1)
        return spixl, rep


class PixelSweep:
    """Per-pixel plane sweep.  cost="ncc": build-defined KxK NCC cost volume
    [D][H][W] per reference view, then WTA + confidence (the HBM-streaming
    pass); fused=True folds the WTA into the sweep kernel (mvs_ncc_wta_d: no
    volume in HBM, same disp/conf bits).  cost="sad": the reference sweep at
    S=1 grid semantics (parity).  subpixel=True (NCC only): run() also leaves
    the sub-level disparity (the parabola fit of include/mvs.h) of the views
    it swept in self.disp_sub; disp and conf are unchanged.  sgm=True (NCC
    only): run() also leaves the winner and confidence of the semi-globally
    aggregated volume (mvs_sgm_d, penalties sgm_p1 <= sgm_p2; sgm_paths is the
    path mask, 15 = the four axis-aligned paths, 255 = with the four diagonal
    ones, mvs_sgm8_d) in self.disp_agg and self.conf_agg [z1 - z0, H, W]:
    per view ncc_volume ->
    sgm -> wta, through one more [D, H, W] buffer; with fused=True the volume
    is computed for this alone.  disp, conf and disp_sub are unchanged.
    sgm_batch=B > 1: the views of a run are aggregated in groups of up to B,
    one mvs_sgm8_batch_d call per group (one launch per path over the whole
    group) through [min(B, V), D, H, W] buffers; every output keeps its bits.
    The two buffers take 2 * B * 4 * D * H * W bytes: 10.6 GB at 1920x1080,
    D = 128, B = 5.  With 1, the default, allocations and launches are as
    without the option.
    sgm_dtype="u16" (needs sgm=True and NCC cost; "f32", the default, changes
    nothing and allocates nothing new): the aggregation runs on 16-bit integer
    costs (include/mvs.h at mvs_sgm8_u16_batch_d).  The penalties become
    int(round(p * 2047)) and must obey 0 <= P1 <= P2 <= 4095.  Per group of up
    to B = sgm_batch views: ncc_volume into one reused float32 [D, H, W],
    quant_u16 of it into q[j], one sgm_u16_batch over the group, wta_u16 of
    agg[j] into disp_agg / conf_agg.  The buffers take
    4 * D * H * W + 2 * B * 2 * D * H * W bytes: 6.4 GB at 1920x1080, D = 128,
    B = 5, against 10.6 GB.  D <= 256.  disp, conf and disp_sub are as without
    the option; disp_agg and conf_agg are those of the 16-bit definition
    (tests/sgm16_ref.py), close to but not the float32 aggregate's.
    sgm_subpixel=True (needs sgm=True; independent of subpixel; False, the
    default, changes nothing): run() also leaves self.disp_agg_sub
    [z1 - z0, H, W] beside disp_agg and conf_agg, the sub-level disparity of
    the aggregate's winner: the parabola through the raw volume's costs at
    that winner (include/mvs.h at mvs_wta_agg_sub_d; tests/sgm_sub_ref.py).
    In each of the three aggregation paths the winner pass over agg becomes
    wta_agg_sub(agg, vol) or wta_u16_sub(agg[j], q[j]): agg is still read
    once, no buffer is added besides the output, every other output keeps
    its bits."""

    def __init__(self, engine: Engine, cam: CameraArray, W: int, H: int, cost: str = "ncc", window: int = 5,
                 fused: bool = False, subpixel: bool = False, sgm: bool = False, sgm_p1: float = 0.1,
                 sgm_p2: float = 0.8, sgm_paths: int = 15, sgm_batch: int = 1, sgm_dtype: str = "f32",
                 sgm_subpixel: bool = False):
        if subpixel and cost != "ncc":
            raise ValueError("subpixel=True needs cost=\"ncc\": the fit is defined on the NCC cost volume")
        if sgm and cost != "ncc":
            raise ValueError("sgm=True needs cost=\"ncc\": the aggregation runs on the NCC cost volume")
        if not 1 <= int(sgm_paths) <= 255:
            raise ValueError("sgm_paths must be a path mask in 1..255")
        if int(sgm_batch) < 1:
            raise ValueError("sgm_batch must be at least 1")
        if sgm_dtype not in ("f32", "u16"):
            raise ValueError("sgm_dtype must be \"f32\" or \"u16\"")
        if sgm_dtype == "u16" and not (sgm and cost == "ncc"):
            raise ValueError("sgm_dtype=\"u16\" needs sgm=True and cost=\"ncc\"")
        if sgm_subpixel and not sgm:
            raise ValueError("sgm_subpixel=True needs sgm=True: it is the sub-level disparity of the aggregate's winner")
        self.sgm_dtype, self.sgm_subpixel = sgm_dtype, bool(sgm_subpixel)
        self.q = None
        if sgm_dtype == "u16":
            self.p1_u16, self.p2_u16 = int(round(sgm_p1 * 2047)), int(round(sgm_p2 * 2047))
            if not 0 <= self.p1_u16 <= self.p2_u16 <= 4095:
                raise ValueError("sgm_dtype=\"u16\": the penalties times 2047 must obey 0 <= P1 <= P2 <= 4095")
            if cam.D > 256:
                raise ValueError("sgm_dtype=\"u16\" takes at most 256 levels")
        self.e, self.cam, self.W, self.H = engine, cam, W, H
        self.cost, self.K, self.fused, self.subpixel = cost, window, fused, subpixel
        self.sgm, self.sgm_p1, self.sgm_p2, self.sgm_paths = sgm, sgm_p1, sgm_p2, int(sgm_paths)
        self.disp_sub = None
        self.disp_agg = self.conf_agg = self.disp_agg_sub = None
        self.vol = self.agg = None
        # views per mvs_sgm8_batch_d call (1: one mvs_sgm_d / mvs_sgm8_d call per view)
        self.sgm_batch = min(int(sgm_batch), cam.view_count) if sgm else 1
        shape = (cam.D, H, W) if self.sgm_batch == 1 else (self.sgm_batch, cam.D, H, W)
        if sgm_dtype == "u16":  # one float32 volume, reused; the group lives in uint16
            self.vol = engine.empty((cam.D, H, W), torch.float32)
            self.q = engine.empty((self.sgm_batch, cam.D, H, W), torch.uint16)
            self.agg = engine.empty((self.sgm_batch, cam.D, H, W), torch.uint16)
        else:
            if cost == "ncc" and (sgm or not fused):
                self.vol = engine.empty(shape, torch.float32)
            if sgm:
                self.agg = engine.empty(shape, torch.float32)
        self.levels = engine.levels_dev(cam)

    def run(self, lab, l8, z0: int, z1: int, disp_out=None, conf_out=None, views=None):
        """Reference views [z0, z1).  views: the views whose window planes are
        built (default all; a view shard passes its block + neighbours)."""
        n = z1 - z0
        disp = self.e.empty((n, self.H, self.W), torch.float32) if disp_out is None else disp_out
        conf = None
        if self.cost == "sad":
            self.e.sweep_pixel_sad(lab, self.cam, z0, z1, out=disp)
            return disp, None
        conf = self.e.empty((n, self.H, self.W), torch.float32) if conf_out is None else conf_out
        if views is None:
            box = self.e.box_stats(l8, self.K)
        else:
            V, H, W = l8.shape
            box = self.e.box_stats_views(l8, self.K, views, self.e.empty((2, V, H + (H & 1), W, 2), torch.int32))
        if self.sgm:
            self.disp_agg = self.e.empty((n, self.H, self.W), torch.float32)
            self.conf_agg = self.e.empty((n, self.H, self.W), torch.float32)
            if self.sgm_subpixel:
                self.disp_agg_sub = self.e.empty((n, self.H, self.W), torch.float32)
        if self.fused:  # every reference view of the call, runs of views per launch
            self.e.ncc_wta_range(l8, box, self.cam, z0, z1, self.K, disp=disp, conf=conf)
            if self.subpixel:  # the post-pass over the whole range, one call
                self.disp_sub = self.e.ncc_sub_range(l8, box, self.cam, z0, z1, self.K, disp=disp)
            if self.sgm_dtype == "u16":
                self._run_groups_u16(l8, box, z0, z1, None, None)
            elif self.sgm_batch > 1:
                self._run_groups(l8, box, z0, z1, None, None)
            elif self.sgm:  # the volume the fused sweep never stores, for the aggregation alone
                for i, z in enumerate(range(z0, z1)):
                    self.e.ncc_volume(l8, box, self.cam, z, self.K, out=self.vol)
                    self._aggregate(i)
            return disp, conf
        if self.subpixel:
            self.disp_sub = self.e.empty((n, self.H, self.W), torch.float32)
        if self.sgm_dtype == "u16":
            self._run_groups_u16(l8, box, z0, z1, disp, conf)
            return disp, conf
        if self.sgm_batch > 1:
            self._run_groups(l8, box, z0, z1, disp, conf)
            return disp, conf
        for i, z in enumerate(range(z0, z1)):
            self.e.ncc_volume(l8, box, self.cam, z, self.K, out=self.vol)
            self.e.wta(self.vol, self.levels, disp=disp[i], conf=conf[i])
            if self.subpixel:
                self.e.wta_sub(self.vol, self.levels, out=self.disp_sub[i])
            if self.sgm:
                self._aggregate(i)
        return disp, conf

    def _run_groups(self, l8, box, z0: int, z1: int, disp, conf):
        """sgm_batch > 1: the views of [z0, z1) in groups of at most sgm_batch (the last may be shorter).  Per view
        of a group ncc_volume into vol[j] (and, in the two-pass form, where disp is given, wta / wta_sub of it), one
        sgm_batch over the group, then the winner pass (_winner) of agg[j] into view i of disp_agg / conf_agg."""
        B = self.sgm_batch
        for g0 in range(z0, z1, B):
            g = min(B, z1 - g0)
            for j in range(g):
                i = g0 - z0 + j
                self.e.ncc_volume(l8, box, self.cam, g0 + j, self.K, out=self.vol[j])
                if disp is not None:
                    self.e.wta(self.vol[j], self.levels, disp=disp[i], conf=conf[i])
                    if self.subpixel:
                        self.e.wta_sub(self.vol[j], self.levels, out=self.disp_sub[i])
            self.e.sgm_batch(self.vol[:g], self.sgm_p1, self.sgm_p2, self.sgm_paths, out=self.agg[:g])
            for j in range(g):
                i = g0 - z0 + j
                self._winner(self.agg[j], self.vol[j], i)

    def _run_groups_u16(self, l8, box, z0: int, z1: int, disp, conf):
        """sgm_dtype="u16": _run_groups with the group in uint16.  Per view of a group ncc_volume into the one
        float32 volume (and, in the two-pass form, wta / wta_sub of it), quant_u16 of it into q[j]; one sgm_u16_batch
        over the group; wta_u16 of agg[j] (with sgm_subpixel wta_u16_sub of agg[j] and q[j]) into view i of disp_agg /
        conf_agg."""
        B = self.sgm_batch
        for g0 in range(z0, z1, B):
            g = min(B, z1 - g0)
            for j in range(g):
                i = g0 - z0 + j
                self.e.ncc_volume(l8, box, self.cam, g0 + j, self.K, out=self.vol)
                if disp is not None:
                    self.e.wta(self.vol, self.levels, disp=disp[i], conf=conf[i])
                    if self.subpixel:
                        self.e.wta_sub(self.vol, self.levels, out=self.disp_sub[i])
                self.e.quant_u16(self.vol, out=self.q[j])
            self.e.sgm_u16_batch(self.q[:g], self.p1_u16, self.p2_u16, self.sgm_paths, out=self.agg[:g])
            for j in range(g):
                i = g0 - z0 + j
                if self.sgm_subpixel:
                    self.e.wta_u16_sub(self.agg[j], self.q[j], self.levels, disp=self.disp_agg[i],
                                       conf=self.conf_agg[i], out=self.disp_agg_sub[i])
                else:
                    self.e.wta_u16(self.agg[j], self.levels, disp=self.disp_agg[i], conf=self.conf_agg[i])

    def _aggregate(self, i: int):
        """self.vol -> sgm -> the winner pass into view i of disp_agg / conf_agg."""
        self.e.sgm(self.vol, self.sgm_p1, self.sgm_p2, self.sgm_paths, out=self.agg)
        self._winner(self.agg, self.vol, i)

    def _winner(self, agg, vol, i: int):
        """The float32 aggregate's winner pass into view i: wta, or with sgm_subpixel wta_agg_sub, which also fits
        through vol at that winner."""
        if self.sgm_subpixel:
            self.e.wta_agg_sub(agg, vol, self.levels, disp=self.disp_agg[i], conf=self.conf_agg[i],
                               out=self.disp_agg_sub[i])
        else:
            self.e.wta(agg, self.levels, disp=self.disp_agg[i], conf=self.conf_agg[i])


class DepthRefinement:
    """clDepthRefinement(...)->do_refinement(gamma, alpha, fuse, kernel_step,
    kernel_size, no_prop) + fusion (spixl_to_image)."""

    def __init__(self, engine: Engine, cam: CameraArray, S: int):
        self.e, self.cam, self.S = engine, cam, S

    def do_refinement(self, spixl, labels, rep, st: params.Settings, fusion_compat: bool = True):
        return self.e.refine(spixl, labels, rep, self.cam, self.S, st.gamma, st.alpha, st.fuse, st.kernel_step,
                             st.kernel_size, st.no_prop, fusion_compat)


class ConsistencyFilter:
    def __init__(self, engine: Engine, array_width: int, bl_ratio: float, fuse: float):
        self.e, self.aw, self.bl, self.fuse = engine, array_width, bl_ratio, fuse

    def run(self, disp_all: torch.Tensor, z0: int = 0, z1: int | None = None):
        return self.e.filter(disp_all, self.aw, self.bl, self.fuse, z0, z1)


@dataclass
class StepOutput:
    lab: torch.Tensor
    spixl: torch.Tensor
    labels: torch.Tensor
    rep: torch.Tensor
    disp: torch.Tensor | None = None
    conf: torch.Tensor | None = None
    disp_sub: torch.Tensor | None = None  # sub-level disparity (Pipeline(subpixel=True)), else None
    disp_agg: torch.Tensor | None = None  # winner of the semi-globally aggregated volume (Pipeline(sgm=True)), else None
    conf_agg: torch.Tensor | None = None  # its confidence
    disp_agg_sub: torch.Tensor | None = None  # its sub-level disparity (Pipeline(sgm_subpixel=True)), else None
    disp_refined: torch.Tensor | None = None
    disp_filtered: torch.Tensor | None = None


class Pipeline:
    """pipeline: segmentation -> depth init -> [refinement] -> [filter].

    The reference's exe_pipeline runs SLIC only (perform_depth_est is commented
    out, pipeline.cpp:60-64); this pipeline wires the depth stages in the order
    of pipeline::perform_depth_est (pipeline.cpp:108-175).

    concurrent=True: after the colour conversion the superpixel chain (SLIC,
    extents, superpixel sweep: latency/L2-bound gathers) runs on a second HIP
    stream with its own libmvs context, beside the per-pixel chain (window
    planes, fused NCC sweep + WTA) on the caller's stream; the caller's stream
    joins the side stream before refinement.  One stream is the default here
    and in bench.py (round 5: with the matrix-core sweep the side stream
    measured no gain); `bench.py --concurrent` runs the headline
    with it, and `bench.py --full` reports it as `concurrent_variant`."""

    def __init__(self, engine: Engine, settings: params.Settings, W: int, H: int,
                 view_subset: list[list[int]] | None = None, pixel_cost: str | None = "ncc",
                 refine: bool = False, filt: bool = False, concurrent: bool = False, fused: bool = False,
                 subpixel: bool = False, sgm: bool = False, sgm_p1: float = 0.1, sgm_p2: float = 0.8,
                 sgm_paths: int = 15, sgm_batch: int = 1, sgm_dtype: str = "f32", sgm_subpixel: bool = False):
        """sgm_batch: see PixelSweep (views aggregated per call; 2 * B * 4 * D * H * W bytes of buffers).
        sgm_dtype: "f32" (the default: nothing changes) or "u16", the aggregation on 16-bit integer costs, see
        PixelSweep; its buffers are 4 * D * H * W + 2 * B * 2 * D * H * W bytes.
        sgm_subpixel: with sgm=True, the result also carries disp_agg_sub, the sub-level disparity of the aggregate's
        winner (see PixelSweep)."""
        if int(sgm_batch) < 1:
            raise ValueError("sgm_batch must be at least 1")
        self.e, self.st, self.W, self.H = engine, settings, W, H
        vs = view_subset if view_subset is not None else params.neighbour_lists(
            settings.array_width, settings.array_height, settings.neib_hor, settings.neib_ver)
        mat, num = params.flatten_subsets(vs)
        levels = params.disparity_levels(settings.min_disp, settings.max_disp, settings.inc)
        self.cam = CameraArray(settings.array_width, settings.bl_ratio, levels, mat, num)
        self.slic = SLIC(engine, settings)
        self.photo = PhotoConsistency(engine, self.cam, settings.spixl_size)
        if subpixel and pixel_cost != "ncc":
            raise ValueError("subpixel=True needs pixel_cost=\"ncc\"")
        if sgm and pixel_cost != "ncc":
            raise ValueError("sgm=True needs pixel_cost=\"ncc\"")
        if sgm_dtype not in ("f32", "u16"):
            raise ValueError("sgm_dtype must be \"f32\" or \"u16\"")
        if sgm_dtype == "u16" and not (sgm and pixel_cost == "ncc"):
            raise ValueError("sgm_dtype=\"u16\" needs sgm=True and pixel_cost=\"ncc\"")
        if sgm_subpixel and not sgm:
            raise ValueError("sgm_subpixel=True needs sgm=True")
        self.pixel = (PixelSweep(engine, self.cam, W, H, pixel_cost, settings.window, fused, subpixel, sgm, sgm_p1,
                                 sgm_p2, sgm_paths, sgm_batch, sgm_dtype, sgm_subpixel)
                      if pixel_cost else None)
        self.refiner = DepthRefinement(engine, self.cam, settings.spixl_size) if refine else None
        self.filter = ConsistencyFilter(engine, settings.array_width, settings.bl_ratio, settings.fuse) if filt else None
        self.side = None
        if concurrent and self.pixel is not None:
            side_engine = Engine(engine.device.index)  # own context: own scratch, metadata and plans
            self.side = (torch.cuda.Stream(engine.device), SLIC(side_engine, settings),
                         PhotoConsistency(side_engine, self.cam, settings.spixl_size))

    def exe_pipeline(self, rgbx: torch.Tensor, z0: int = 0, z1: int | None = None,
                     gather=None) -> StepOutput:
        """rgbx [V,H,W,4] resident on the GPU.  [z0, z1) = reference views this
        process owns; `gather` (distributed.py) all-gathers per-view maps."""
        V = rgbx.shape[0]
        z1 = V if z1 is None else z1
        if self.side is None:
            lab, l8, spixl, labels = self.slic.do_super_pixel_seg(rgbx)
            spixl, rep = self.photo.do_initial_depth_estimation(lab, spixl, labels, z0, z1)
            out = StepOutput(lab, spixl, labels, rep)
            if self.pixel is not None:
                out.disp, out.conf = self.pixel.run(lab, l8, z0, z1)
        else:
            lab, l8 = self.e.cvt(rgbx, want_l8=True)
            main = torch.cuda.current_stream(self.e.device)
            stream, slic, photo = self.side
            stream.wait_stream(main)
            with torch.cuda.stream(stream):
                spixl, labels = slic.segment(lab)
                spixl, rep = photo.do_initial_depth_estimation(lab, spixl, labels, z0, z1)
            lab.record_stream(stream)  # allocated on main, read on the side stream
            disp, conf = self.pixel.run(lab, l8, z0, z1)
            main.wait_stream(stream)
            for t in (spixl, labels, rep):  # allocated on the side stream, used on main from here
                t.record_stream(main)
            out = StepOutput(lab, spixl, labels, rep, disp, conf)
        if self.pixel is not None and self.pixel.subpixel:
            out.disp_sub = self.pixel.disp_sub
        if self.pixel is not None and self.pixel.sgm:
            out.disp_agg, out.conf_agg = self.pixel.disp_agg, self.pixel.conf_agg
            out.disp_agg_sub = self.pixel.disp_agg_sub
        if self.refiner is not None:
            r = self.refiner.do_refinement(spixl, labels, rep, self.st)
            out.disp_refined = r["disp"]
        if self.filter is not None:
            src = out.disp_refined if out.disp_refined is not None else out.disp
            full = src if src.shape[0] == V else (gather(src) if gather else None)
            if full is None:
                raise ValueError("filter over a view shard needs a gather function")
            out.disp_filtered = self.filter.run(full, z0, z1)[1][z0:z1]
        return out
