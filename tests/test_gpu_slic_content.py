"""The SLIC kernels (cl_multiview_stereo_amd/csrc/slic.hip) against the oracle
on built Lab inputs (tests/slic_content.py; the state each case is there for
is pinned on the CPU by tests/test_slic_content_cpu.py).

Every case goes through engine.slic (mvs_slic_d) as plain float Lab -- no
k_cvt, so nothing keeps it on the 8-bit gamut lattice -- and is compared with
orc.slic_from_lab bit for bit (assert_bits, the project's bar): the labels,
spixl[..., :7] and, for edge mode 1, the overwritten Lab; with the other modes
the Lab must come back untouched.  Each case runs once per iteration count
(slic_content.passes: 0, 1, 2 and its own), so a wrong update shows at the
iteration where it happens, and once more per environment knob of the case
(MVS_SLIC_TILES9=1 at S = 32 and 64, MVS_SLIC_UPDATE=0 off the tile path).
The oracle runs once per (case, iteration count)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch

from cl_multiview_stereo_amd import _lib, params
from tests import slic_content as sc
from tests.cases import as_u32
from tests.test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

KNOBS = ("MVS_SLIC_TILES9", "MVS_SLIC_UPDATE")


def _set_env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _run(engine, name, no_iter, dev_lab=None):
    """engine.slic of the case at no_iter -> (spixl, labels, lab) on the host."""
    c = sc.CASES[name]
    if dev_lab is None:
        dev_lab = torch.from_numpy(np.array(sc.lab(name))).cuda()
    sp, lb = engine.slic(dev_lab, c["S"], c["weight"], no_iter, c["conn"], edge_enable=c["edge"], search=c["search"])
    return sp.cpu().numpy(), as_u32(lb), dev_lab.cpu().numpy()


def _check(engine, name, tag=""):
    c = sc.CASES[name]
    src = sc.lab(name)
    dev_lab = None
    for no_iter in sc.passes(name):
        if dev_lab is None or c["edge"] == 1:  # (mode 1 overwrites it)
            dev_lab = torch.from_numpy(np.array(src)).cuda()
        sp, lb, lab = _run(engine, name, no_iter, dev_lab)
        for v, want in enumerate(sc.oracle(name, no_iter)):
            what = f"{name}{tag} no_iter {no_iter} view {v}"
            assert_bits(lb[v], want[1], f"{what}: labels")
            assert_bits(sp[v][..., :7], want[0][..., :7], f"{what}: spixl")
            assert_bits(lab[v], want[2] if c["edge"] == 1 else src[v], f"{what}: lab")


RUNS = [(n, e) for n, c in sc.CASES.items() if c["legal"] for e in ({},) + c["env"]]


def _id(run):
    name, env = run
    return name + "".join(f"-{k[9:].lower()}{v}" for k, v in env.items())


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_case(engine, monkeypatch, run):
    name, env = run
    _set_env(monkeypatch, env)
    _check(engine, name, "".join(f" {k}={v}" for k, v in env.items()))


def test_every_route_is_listed():
    """The table runs both settings of each knob where it applies."""
    ids = {_id(r) for r in RUNS}
    for n in ("near_s32", "near_s64", "flat_s32", "empty_s32", "empty_s64", "blocks_s32"):
        assert {n, n + "-tiles91"} <= ids
    for n in ("near_s8", "near_s40", "empty_s8", "blocks_s40", "l32_s6", "l32_s12", "l16_s6", "legal_w_s7"):
        assert {n, n + "-update0"} <= ids
    for n, c in sc.CASES.items():  # every S = 32 / 64 case of the 2x2 loop, every case off the tile path
        if c["legal"] and c["S"] in (32, 64) and not c["search"]:
            assert n + "-tiles91" in ids
        if c["legal"] and c["S"] % 16:
            assert n + "-update0" in ids
    assert {"near_s16_search1", "near_s48_search1"} <= ids  # k_assign_tiles<true>
    assert not any(n.startswith("wide") for n, _ in RUNS)


@pytest.mark.parametrize("name", ["near_s32", "blocks_s40", "suppress_s8"])
def test_rerun_is_identical(engine, monkeypatch, name):
    _set_env(monkeypatch, {})
    a = _run(engine, name, sc.CASES[name]["no_iter"])
    b = _run(engine, name, sc.CASES[name]["no_iter"])
    for what, x, y in zip(("spixl", "labels", "lab"), a, b):
        assert_bits(y, x, f"{name} rerun: {what}")


# ---- the bound on W and H -------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.WIDE))
def test_wide_strips_fail_loudly(engine, name):
    """W > 65536: mvs_slic_d's bad-arguments failure, before anything is
    launched (the update kernels' integer tile sums would leave the reference's
    float tree there: tests/test_slic_content_cpu.py)."""
    c = sc.CASES[name]
    _, W, H = sc.WIDE[name]
    assert not c["legal"] and W > sc.MAX_DIM and W * H <= 2 ** 27
    lab = torch.zeros((1, H, W, 4), device="cuda")
    with pytest.raises(_lib.MvsError, match="mvs_slic_d: bad arguments"):
        engine.slic(lab, c["S"], c["weight"], c["no_iter"])


@pytest.mark.parametrize("W,H", [(65537, 8), (8, 65537)])
def test_one_past_the_bound_fails_loudly(engine, W, H):
    lab = torch.zeros((1, H, W, 4), device="cuda")
    for S in (7, 16, 32):
        with pytest.raises(_lib.MvsError, match="mvs_slic_d: bad arguments"):
            engine.slic(lab, S, 0.6, 1)
    # the host-pointer entry fails the same way, before it allocates or converts anything
    rgbx = np.zeros((H, W, 4), np.uint8)
    mw, mh = params.map_size(W, H, 16)
    sp = np.zeros((mh, mw, 8), np.float32)
    lb = np.zeros((H, W), np.uint32)
    p = _lib.SlicParams(16, 0.6, 1, 0, 0)
    with pytest.raises(_lib.MvsError, match="mvs_do_super_pixel_seg: bad arguments"):
        _lib.check(engine.L.mvs_do_super_pixel_seg(engine.ctx, rgbx.ctypes.data_as(C.c_void_p), W, H, C.byref(p), None,
                                                   sp.ctypes.data_as(C.c_void_p), lb.ctypes.data_as(C.c_void_p)),
                   "mvs_do_super_pixel_seg")
