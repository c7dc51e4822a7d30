"""The refinement kernels (k_flatness, k_init_state, k_propagate<LT, FAST>,
k_spixl_to_image{,4}; cl_multiview_stereo_amd/csrc/refine.hip) against the
oracle on built inputs (tests/refine_content.py; their states are pinned on
the CPU by tests/test_refine_content_cpu.py).

Each run hands spixl, labels, rep and the case's schedule to the stage entry
points as they are -- no SLIC, no k_boundary, no sweep -- and compares every
stage with the oracle's bit for bit (assert_bits, the project's bar): flatness,
the init state, every propagate iteration (each fed the oracle's state of the
step before, so one stage's fault does not hide behind another's), and the
fused map of the last state.  Once with uint32 labels and once with the uint16
views of the same labels.  The oracle's stages are computed once per case."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd import _lib
from cl_multiview_stereo_amd.engine import CameraArray, _ptr
from oracle import oracle as orc
from tests import refine_content as rc
from tests.test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

SENTINEL = -777.25


class Case:
    """The inputs of one refine_content case on the device."""

    def __init__(self, name, l16=False):
        m = self.m = rc.make(name)
        self.name, self.l16 = name, l16
        self.cam = CameraArray(m["aw"], m["bl"], np.zeros(1, np.float32), m["vs"], m["sn"])
        self.sp = torch.from_numpy(m["spixl"].copy()).cuda()
        self.rep = torch.from_numpy(m["rep"].copy()).cuda()
        if l16:
            assert m["mw"] * m["mh"] <= 65536
            self.lb = torch.from_numpy(m["labels"].astype(np.uint16).view(np.int16)).cuda()
        else:
            self.lb = torch.from_numpy(m["labels"].view(np.int32).copy()).cuda()
        self.tag = f"{name} ({'uint16' if l16 else 'uint32'} labels)"

    def flatness(self, engine):
        return engine.flatness(self.sp, self.m["rp"]["flat_gamma"])

    def init_state(self, engine, flat, z0=0, z1=None, state=None):
        m, rp = self.m, self.m["rp"]
        nks, kss = m["init"]
        if not self.l16 and state is None and z0 == 0 and z1 is None:
            return engine.init_state(self.sp, self.lb, self.rep, flat, self.cam, m["S"], rp["init_gamma"],
                                     rp["init_alpha"], nks, kss, rp["fuse"])
        return engine.init_state_range(self.sp, self.lb, self.rep, flat, self.cam, m["S"], rp["init_gamma"],
                                       rp["init_alpha"], nks, kss, rp["fuse"], z0, m["V"] if z1 is None else z1,
                                       state=state)

    def propagate(self, engine, flat, step, st_in, st_out=None, z0=0, z1=None):
        m, rp = self.m, self.m["rp"]
        it, nks, kss = step
        st_out = torch.full_like(st_in, SENTINEL) if st_out is None else st_out
        return engine.propagate(self.sp, self.lb, self.rep, flat, self.cam, m["S"], it, rp["prop_alpha"],
                                rp["prop_gamma"], rp["fuse"], nks, kss, st_in, st_out, z0, z1)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _check_stages(engine, name, l16):
    c, want = Case(name, l16), rc.oracle_stages(name)
    m = c.m
    flat = c.flatness(engine)
    assert_bits(flat.cpu().numpy(), want["flat"], f"{c.tag}: flatness")
    flat = _dev(want["flat"])
    st = c.init_state(engine, flat)
    assert_bits(st.cpu().numpy(), want["state0"], f"{c.tag}: init state (nks, kss) = {m['init']}")
    prev = want["state0"]
    for k, step in enumerate(m["props"]):
        out = c.propagate(engine, flat, step, _dev(prev))
        assert_bits(out.cpu().numpy(), want["states"][k], f"{c.tag}: propagate (iter, nks, kss) = {step}")
        prev = want["states"][k]
    disp = engine.spixl_to_image(c.sp, c.lb, _dev(prev), m["S"])
    assert_bits(disp.cpu().numpy(), want["disp"], f"{c.tag}: spixl_to_image")
    # the chain on the device's own states (what mvs_refine_d runs) ends at the same state
    cur = st
    for step in m["props"]:
        cur = c.propagate(engine, flat, step, cur)
    assert_bits(cur.cpu().numpy(), prev, f"{c.tag}: chained propagate")


OTHER = [n for n in rc.CASES if n not in rc.DENSE_M32]


@pytest.mark.parametrize("l16", [False, True], ids=["u32", "u16"])
@pytest.mark.parametrize("name", OTHER)
def test_stages(engine, name, l16):
    _check_stages(engine, name, l16)


# nks 13 (61 smoothness terms: the last lane-parallel launch) against 14 (65: one lane per candidate) and 16,
# kss 1.0 (every far term and candidate of the central cells valid) against 2.5, iterations 0 and 4, on the 32 x 32 map
DENSE = ["dense_n0_k1", "dense_n1_k25", "dense_n13_k1", "dense_n13_k25", "dense_n14_k1", "dense_n14_k25",
         "dense_n16_k1", "dense_n16_k25"]


@pytest.mark.parametrize("l16", [False, True], ids=["u32", "u16"])
@pytest.mark.parametrize("name", DENSE)
def test_dense_schedules(engine, name, l16):
    m = rc.make(name)
    assert (m["mw"], m["mh"]) == (32, 32) and [s[0] for s in m["props"]] == [0, 4]
    assert m["init"] == (int(name.split("_")[1][1:]), {"k1": 1.0, "k25": 2.5}[name.split("_")[2]])
    _check_stages(engine, name, l16)


def test_every_dense_case_is_listed():
    assert sorted(DENSE) == sorted(rc.DENSE_M32)
    assert {(rc.make(n)["init"]) for n in DENSE} >= {(13, 1.0), (14, 1.0), (13, 2.5), (14, 2.5), (16, 1.0), (0, 1.0)}


# ---- range launches on the 4 x 3 lists ----------------------------------------------------------
def _fast(sn, z0, z1, nks):
    """launch_propagate's choice of k_propagate<LT, FAST = true>, restated."""
    return nks <= 13 and max(int(n) for n in sn[z0:z1]) <= 8


SPLITS = [((0, 6), (6, 12)), ((0, 2), (2, 3), (3, 6), (6, 7), (7, 8), (8, 12))]


@pytest.mark.parametrize("l16", [False, True], ids=["u32", "u16"])
@pytest.mark.parametrize("name", ["l4x3_plane", "l4x3_half", "l4x3_dense"])
def test_range_launches_tile_the_full_launch(engine, name, l16):
    """max_nbr is taken over [z0, z1) only: views [0, 6) of the 4 x 3 lists
    hold at most 8 neighbours and launch k_propagate<LT, true>, the full launch
    (maximum 11) and views [6, 12) launch k_propagate<LT, false>, whose waves
    choose per superpixel.  The pieces, written into a state prefilled with a
    sentinel, tile the full launch's result (and the oracle's) bit for bit and
    leave every other row alone."""
    c, want = Case(name, l16), rc.oracle_stages(name)
    m, sn = c.m, c.m["sn"]
    lo, hi = rc.L43_LOW, (rc.L43_LOW[1], m["V"])
    flat = _dev(want["flat"])
    prev = want["state0"]
    for k, step in enumerate(m["props"]):
        nks = step[1]
        assert nks <= 13
        assert _fast(sn, *lo, nks) and not _fast(sn, *hi, nks) and not _fast(sn, 0, m["V"], nks)
        st_in = _dev(prev)
        full = c.propagate(engine, flat, step, st_in).cpu().numpy()
        assert_bits(full, want["states"][k], f"{c.tag}: full launch {step}")
        for split in SPLITS:
            tiled = torch.full_like(st_in, SENTINEL)
            for z0, z1 in split:
                piece = torch.full_like(st_in, SENTINEL)
                c.propagate(engine, flat, step, st_in, piece, z0, z1)
                p = piece.cpu().numpy()
                assert_bits(p[z0:z1], full[z0:z1], f"{c.tag}: propagate {step} views [{z0}, {z1})")
                assert (np.delete(p, np.s_[z0:z1], 0) == np.float32(SENTINEL)).all(), (name, step, z0, z1)
                c.propagate(engine, flat, step, st_in, tiled, z0, z1)
            assert_bits(tiled.cpu().numpy(), full, f"{c.tag}: propagate {step} tiled by {split}")
        prev = want["states"][k]
    for split in SPLITS:
        tiled = torch.full((m["V"], m["mh"], m["mw"], 6), SENTINEL, device="cuda")
        for z0, z1 in split:
            piece = torch.full_like(tiled, SENTINEL)
            c.init_state(engine, flat, z0, z1, state=piece)
            p = piece.cpu().numpy()
            assert_bits(p[z0:z1], want["state0"][z0:z1], f"{c.tag}: init_state_range views [{z0}, {z1})")
            assert (np.delete(p, np.s_[z0:z1], 0) == np.float32(SENTINEL)).all(), (name, z0, z1)
            c.init_state(engine, flat, z0, z1, state=tiled)
        assert_bits(tiled.cpu().numpy(), want["state0"], f"{c.tag}: init_state_range tiled by {split}")


# ---- mvs_refine_d end to end ------------------------------------------------------------------------
E2E = "half_3x3"  # the 13 x 9 map, 9 views of 3 to 8 neighbours, half-way shifts


@pytest.mark.parametrize("fusion_compat", [True, False])
@pytest.mark.parametrize("no_prop", [0, 1, 2, 5])
def test_refine_options(engine, no_prop, fusion_compat):
    """mvs_refine_d with no_prop in {0, 1, 2, 5} and both fusion_compat values
    against orc.refine with the same arguments: flatness, the state the flag
    names (compat: what the last odd iteration left in the first buffer, or the
    init state; else the last iteration's) and the map fused from it."""
    c = Case(E2E)
    m = c.m
    want = orc.refine(m["spixl"], m["labels"], m["rep"], m["vs"], m["sn"], m["aw"], m["bl"], m["S"], 2.0, 6.0, 1.0, 13,
                      1080, no_prop, fusion_compat)
    got = engine.refine(c.sp, c.lb, c.rep, c.cam, m["S"], 2.0, 6.0, 1.0, 13, 1080, no_prop, fusion_compat)
    assert len(want["states"]) == no_prop
    if fusion_compat:
        odd = [it for it in range(no_prop) if it % 2 == 1]
        state = want["states"][odd[-1]] if odd else want["state0"]
    else:
        state = want["states"][no_prop - 1] if no_prop else want["state0"]
    tag = f"no_prop {no_prop}, fusion_compat {fusion_compat}"
    assert_bits(got["flat"].cpu().numpy(), want["flat"], f"{tag}: flatness")
    assert_bits(got["state_compat" if fusion_compat else "state"].cpu().numpy(), state, f"{tag}: state")
    assert_bits(got["disp"].cpu().numpy(), want["disp"], f"{tag}: disp")
    if no_prop == 5:
        ref = rc.oracle_stages(E2E)
        assert_bits(want["states"][4], ref["states"][4], "orc.refine against the stage-wise oracle")


def _refine_raw(engine, c, p):
    m = c.m
    V, mh, mw, H, W = m["V"], m["mh"], m["mw"], m["H"], m["W"]
    flat = torch.full((V, mh, mw, 2), SENTINEL, device="cuda")
    st = torch.full((V, mh, mw, 6), SENTINEL, device="cuda")
    st2 = torch.full((V, mh, mw, 6), SENTINEL, device="cuda")
    disp = torch.full((V, H, W), SENTINEL, device="cuda")
    engine._stream()
    _lib.check(engine.L.mvs_refine_d(engine.ctx, W, H, m["S"], _ptr(c.sp), _ptr(c.lb), _ptr(c.rep), c.cam.desc(),
                                     C.byref(p), _ptr(flat), _ptr(st), _ptr(st2), _ptr(disp)), "mvs_refine_d")
    return [t.cpu().numpy() for t in (flat, st, st2, disp)]


def test_refine_prescaled(engine):
    """prescaled = 1 takes gamma, alpha and kernel_size as do_refinement
    receives them (2 gamma^2 = 8, 2 alpha^2 = 72, kernel_size / 2 = 540): bit
    for bit the prescaled = 0 call with (2, 6, 1080), which is the oracle's."""
    c = Case(E2E)
    m = c.m
    a = _refine_raw(engine, c, _lib.RefineParams(2.0, 6.0, 1.0, 13, 1080, 5, 1, prescaled=0))
    b = _refine_raw(engine, c, _lib.RefineParams(8.0, 72.0, 1.0, 13, 540, 5, 1, prescaled=1))
    for what, x, y in zip(("flat", "state", "state2", "disp"), a, b):
        assert_bits(y, x, f"prescaled: {what}")
    want = orc.refine(m["spixl"], m["labels"], m["rep"], m["vs"], m["sn"], m["aw"], m["bl"], m["S"], 2.0, 6.0, 1.0, 13,
                      1080, 5, True)
    assert_bits(b[1], want["states"][3], "prescaled: state against the oracle")
    assert_bits(b[2], want["states"][4], "prescaled: state2 against the oracle")
    assert_bits(b[3], want["disp"], "prescaled: disp against the oracle")
