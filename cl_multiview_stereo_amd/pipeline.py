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


def check_pixel_options(cost, subpixel, sgm, sgm_paths, sgm_batch, sgm_dtype, sgm_subpixel, arg: str = "cost"):
    """The option rules of the per-pixel sweep, for PixelSweep and for Pipeline (which names the cost `pixel_cost`):
    raises ValueError, and touches nothing else."""
    ncc = f"{arg}=\"ncc\""
    if subpixel and cost != "ncc":
        raise ValueError(f"subpixel=True needs {ncc}: the fit is defined on the NCC cost volume")
    if sgm and cost != "ncc":
        raise ValueError(f"sgm=True needs {ncc}: the aggregation runs on the NCC cost volume")
    if not 1 <= int(sgm_paths) <= 255:
        raise ValueError("sgm_paths must be a path mask in 1..255")
    if int(sgm_batch) < 1:
        raise ValueError("sgm_batch must be at least 1")
    if sgm_dtype not in ("f32", "u16"):
        raise ValueError("sgm_dtype must be \"f32\" or \"u16\"")
    if sgm_dtype == "u16" and not (sgm and cost == "ncc"):
        raise ValueError(f"sgm_dtype=\"u16\" needs sgm=True and {ncc}")
    if sgm_subpixel and not sgm:
        raise ValueError("sgm_subpixel=True needs sgm=True: it is the sub-level disparity of the aggregate's winner")


class PixelSweep:
    """Per-pixel plane sweep of the reference views [z0, z1) of a run().

    cost="sad": the reference sweep at S=1 grid semantics (parity); run() gives disp alone and no option applies.
    cost="ncc": the build-defined KxK NCC cost volume [D][H][W] of a view, then its winner and confidence (WTA).
    run() returns (disp, conf) [z1 - z0, H, W] and leaves the options' outputs, of the same shape, in attributes.
    No option changes the bits of another's output.

    fused         the WTA is folded into the sweep kernel (mvs_ncc_wta_d): no volume in HBM, same disp / conf bits.
                  Without it the volume is stored and read back (the HBM-streaming pass).
    subpixel      self.disp_sub: the sub-level disparity (the parabola fit of include/mvs.h).
    sgm           self.disp_agg, self.conf_agg: winner and confidence of the semi-globally aggregated volume
                  (mvs_sgm_d; penalties sgm_p1 <= sgm_p2; sgm_paths is the path mask, 15 = the four axis-aligned
                  paths, 255 = with the four diagonal ones, mvs_sgm8_d).  With fused=True the volume is computed
                  for this alone.
    sgm_batch=B   the views are aggregated in groups of up to min(B, V), one mvs_sgm8_batch_d call per group (one
                  launch per path over the whole group).  With 1, the default, one mvs_sgm_d / mvs_sgm8_d call per
                  view.
    sgm_dtype     "u16" (needs sgm=True): the aggregation runs on 16-bit integer costs (include/mvs.h at
                  mvs_sgm8_u16_batch_d), at every B.  The penalties become int(round(p * 2047)), self.p1_u16 and
                  self.p2_u16, and must obey 0 <= P1 <= P2 <= 4095; D <= 256.  disp_agg and conf_agg are those of
                  the 16-bit definition (tests/sgm16_ref.py), close to but not the float32 aggregate's.
    sgm_subpixel  (needs sgm=True; independent of subpixel) self.disp_agg_sub: the sub-level disparity of the
                  aggregate's winner, the parabola through the raw volume's costs at that winner (include/mvs.h at
                  mvs_wta_agg_sub_d; tests/sgm_sub_ref.py).  The winner pass becomes one that also reads the raw
                  volume: the aggregate is still read once and no buffer is added besides the output.

    One loop serves every option set (_run_groups): per group of up to B views, for each view ncc_volume into its
    staging volume, in the two-pass form wta (and wta_sub) of it, for "u16" quant_u16 of it into q[j]; then one
    aggregate call over the group and the winner pass of agg[j] per view.  What the cost types differ in:

                 staging of view j    raw volume   aggregate call            winner pass (with sgm_subpixel)
    "f32", B = 1 vol                  vol          sgm(vol -> agg)           wta (wta_agg_sub)
    "f32", B > 1 vol[j]               vol[j]       sgm_batch(vol[:g])        wta (wta_agg_sub)
    "u16"        vol, reused          q[j]         sgm_u16_batch(q[:g])      wta_u16 (wta_u16_sub)

    Buffers (self.vol, self.agg, self.q; None where not needed), with one = D * H * W:
    * no sgm: vol float32 [D, H, W], and none with fused=True.
    * "f32": vol and agg float32 [D, H, W] at B = 1, [B, D, H, W] above: 2 * B * 4 * one bytes, 10.6 GB at
      1920x1080, D = 128, B = 5.
    * "u16": vol float32 [D, H, W], q and agg uint16 [B, D, H, W]: 4 * one + 2 * B * 2 * one bytes, 6.4 GB at
      1920x1080, D = 128, B = 5, against 10.6 GB."""

    def __init__(self, engine: Engine, cam: CameraArray, W: int, H: int, cost: str = "ncc", window: int = 5,
                 fused: bool = False, subpixel: bool = False, sgm: bool = False, sgm_p1: float = 0.1,
                 sgm_p2: float = 0.8, sgm_paths: int = 15, sgm_batch: int = 1, sgm_dtype: str = "f32",
                 sgm_subpixel: bool = False):
        check_pixel_options(cost, subpixel, sgm, sgm_paths, sgm_batch, sgm_dtype, sgm_subpixel)
        u16 = sgm_dtype == "u16"
        if u16:
            self.p1_u16, self.p2_u16 = int(round(sgm_p1 * 2047)), int(round(sgm_p2 * 2047))
            if not 0 <= self.p1_u16 <= self.p2_u16 <= 4095:
                raise ValueError("sgm_dtype=\"u16\": the penalties times 2047 must obey 0 <= P1 <= P2 <= 4095")
            if cam.D > 256:
                raise ValueError("sgm_dtype=\"u16\" takes at most 256 levels")
        self.e, self.cam, self.W, self.H = engine, cam, W, H
        self.cost, self.K, self.fused, self.subpixel = cost, window, fused, subpixel
        self.sgm, self.sgm_p1, self.sgm_p2, self.sgm_paths = sgm, sgm_p1, sgm_p2, int(sgm_paths)
        self.sgm_dtype, self.sgm_subpixel = sgm_dtype, bool(sgm_subpixel)
        self.disp_sub = None
        self.disp_agg = self.conf_agg = self.disp_agg_sub = None
        self.vol = self.agg = self.q = None
        # views per aggregate call
        B = self.sgm_batch = min(int(sgm_batch), cam.view_count) if sgm else 1
        one = (cam.D, H, W)
        e = engine
        # The cost type, stated once: _stage[j] is where ncc_volume writes view j of a group, _raw[j] the volume the
        # aggregate call read for it (what the sub-level winner pass fits through), _aggs[j] its aggregate; _sgm is
        # the aggregate call with the buffer it reads and its penalties; _wta / _wta_sub are the winner passes.
        if u16:  # one float32 volume, reused; the group lives in uint16
            self.vol = e.empty(one, torch.float32)
            self.q = e.empty((B,) + one, torch.uint16)
            self.agg = e.empty((B,) + one, torch.uint16)
            self._stage, self._raw, self._aggs = [self.vol] * B, list(self.q), list(self.agg)
            self._sgm = (e.sgm_u16_batch, self.q, self.p1_u16, self.p2_u16)
            self._wta, self._wta_sub = e.wta_u16, e.wta_u16_sub
        elif cost == "ncc" and (sgm or not fused):
            self.vol = e.empty(one if B == 1 else (B,) + one, torch.float32)
            self._stage = self._raw = [self.vol] if B == 1 else list(self.vol)
            if sgm:
                self.agg = e.empty(tuple(self.vol.shape), torch.float32)
                self._aggs = [self.agg] if B == 1 else list(self.agg)
                self._sgm = (e.sgm if B == 1 else e.sgm_batch, self.vol, sgm_p1, sgm_p2)
                self._wta, self._wta_sub = e.wta, e.wta_agg_sub
        self.levels = engine.levels_dev(cam)

    def run(self, lab, l8, z0: int, z1: int, disp_out=None, conf_out=None, views=None):
        """Reference views [z0, z1).  views: the views whose window planes are
        built (default all; a view shard passes its block + neighbours)."""
        out = (z1 - z0, self.H, self.W)
        disp = self.e.empty(out, torch.float32) if disp_out is None else disp_out
        if self.cost == "sad":
            self.e.sweep_pixel_sad(lab, self.cam, z0, z1, out=disp)
            return disp, None
        conf = self.e.empty(out, torch.float32) if conf_out is None else conf_out
        if views is None:
            box = self.e.box_stats(l8, self.K)
        else:
            V, H, W = l8.shape
            box = self.e.box_stats_views(l8, self.K, views, self.e.empty((2, V, H + (H & 1), W, 2), torch.int32))
        if self.sgm:
            self.disp_agg = self.e.empty(out, torch.float32)
            self.conf_agg = self.e.empty(out, torch.float32)
            if self.sgm_subpixel:
                self.disp_agg_sub = self.e.empty(out, torch.float32)
        if self.fused:  # every reference view of the call, runs of views per launch
            self.e.ncc_wta_range(l8, box, self.cam, z0, z1, self.K, disp=disp, conf=conf)
            if self.subpixel:  # the post-pass over the whole range, one call
                self.disp_sub = self.e.ncc_sub_range(l8, box, self.cam, z0, z1, self.K, disp=disp)
        elif self.subpixel:
            self.disp_sub = self.e.empty(out, torch.float32)
        if not self.fused or self.sgm:  # (fused: the volume the fused sweep never stores, for the aggregation alone)
            self._run_groups(l8, box, z0, z1, disp, conf)
        return disp, conf

    def _run_groups(self, l8, box, z0: int, z1: int, disp, conf):
        """The views of [z0, z1) in groups of at most sgm_batch (the last may be shorter): the class docstring's
        loop.  View j of a group is view i of the outputs."""
        B = self.sgm_batch
        for g0 in range(z0, z1, B):
            g = min(B, z1 - g0)
            for j in range(g):
                i, vol = g0 - z0 + j, self._stage[j]
                self.e.ncc_volume(l8, box, self.cam, g0 + j, self.K, out=vol)
                if not self.fused:
                    self.e.wta(vol, self.levels, disp=disp[i], conf=conf[i])
                    if self.subpixel:
                        self.e.wta_sub(vol, self.levels, out=self.disp_sub[i])
                if self.q is not None:
                    self.e.quant_u16(vol, out=self.q[j])
            if not self.sgm:
                continue
            call, src, p1, p2 = self._sgm
            s = slice(None) if self.agg.dim() == 3 else slice(g)  # sgm takes the one volume, a batch call the group's
            call(src[s], p1, p2, self.sgm_paths, out=self.agg[s])
            for j in range(g):
                i = g0 - z0 + j
                if self.sgm_subpixel:
                    self._wta_sub(self._aggs[j], self._raw[j], self.levels, disp=self.disp_agg[i],
                                  conf=self.conf_agg[i], out=self.disp_agg_sub[i])
                else:
                    self._wta(self._aggs[j], self.levels, disp=self.disp_agg[i], conf=self.conf_agg[i])


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
        check_pixel_options(pixel_cost, subpixel, sgm, sgm_paths, sgm_batch, sgm_dtype, sgm_subpixel, arg="pixel_cost")
        self.e, self.st, self.W, self.H = engine, settings, W, H
        vs = view_subset if view_subset is not None else params.neighbour_lists(
            settings.array_width, settings.array_height, settings.neib_hor, settings.neib_ver)
        mat, num = params.flatten_subsets(vs)
        levels = params.disparity_levels(settings.min_disp, settings.max_disp, settings.inc)
        self.cam = CameraArray(settings.array_width, settings.bl_ratio, levels, mat, num)
        self.slic = SLIC(engine, settings)
        self.photo = PhotoConsistency(engine, self.cam, settings.spixl_size)
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
