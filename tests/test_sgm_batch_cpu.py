"""The boundary of the batched semi-global aggregation (include/mvs.h at
mvs_sgm8_batch_d) without a GPU: the export and its ctypes signature, the
version step, and the null-context error, which names the entry point.  What
the call computes is pinned on the GPU in tests/test_gpu_sgm_batch.py, its
planner on the CPU in tests/test_sgm_batch_plan_cpu.py."""
from __future__ import annotations

import ctypes as C

from cl_multiview_stereo_amd import _lib


def test_boundary_exports_the_entry_point():
    L = _lib.load()
    assert "mvs_sgm8_batch_d" in _lib.EXPORTS and hasattr(L, "mvs_sgm8_batch_d")
    assert L.mvs_sgm8_batch_d.restype is C.c_int
    assert L.mvs_sgm8_batch_d.argtypes is not None and len(L.mvs_sgm8_batch_d.argtypes) == 12
    # the strides are size_t, in floats
    assert L.mvs_sgm8_batch_d.argtypes[6] is C.c_size_t and L.mvs_sgm8_batch_d.argtypes[11] is C.c_size_t


def test_version_has_the_new_step():
    v = _lib.load().mvs_version()
    assert b"0.9.1.1.1" in v and b"0.9.1.1" in v and b"0.9.1" in v and b"0.9" in v


def test_null_context_is_an_argument_error_that_names_the_entry_point():
    L = _lib.load()
    assert L.mvs_sgm8_batch_d(None, 4, 4, 3, 2, None, 48, 0.1, 0.8, 255, None, 48) == -1
    assert b"mvs_sgm8_batch_d" in L.mvs_last_error()
    # mvs_sgm8_d's own message still names mvs_sgm8_d, not the batch entry
    assert L.mvs_sgm8_d(None, 4, 4, 3, None, 0.1, 0.8, 255, None) == -1
    assert b"mvs_sgm8_d" in L.mvs_last_error() and b"mvs_sgm8_batch_d" not in L.mvs_last_error()
    assert L.mvs_sgm_d(None, 4, 4, 3, None, C.c_float(0.1), C.c_float(0.8), 15, None) == -1
    assert b"mvs_sgm_d" in L.mvs_last_error() and b"batch" not in L.mvs_last_error()
