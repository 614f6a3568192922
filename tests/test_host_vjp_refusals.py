"""The host library's VJP entry points (ort_host_trace_sequential_vjp,
ort_host_trace_pupil_vjp) refuse a bad call with ORT_ERR_ARG before anything is traced, and
accept an empty one. The table (tests/_vjp_refusals.py) is shared with the device library's
test; its expected codes are read off csrc/ort_host.cpp. 64 rays of the lowered tma_fringe
golden lens; a closed-form lens (zern_param), a thin-lens lens and a grid-sag lens where a
row needs one.
"""

import numpy as np
import pytest

from tests import _vjp_refusals as T


@pytest.fixture(scope="module")
def lib():
    from optiland_pr_amd import _native

    return _native.load_host()


@pytest.fixture(scope="module")
def lenses():
    from optiland_pr_amd.host import HostLens

    out = {}
    for name in T.LENSES:
        table, segs = T.lowered(name)
        out[name] = (HostLens(table), table, segs)
    return out


def _alloc(arr):
    a = np.array(arr, copy=True)
    return a, a.ctypes.data


def _call(lenses, lens, form, mode):
    hl, table, segs = lenses[lens]
    c = T.Call(form, mode, hl.c, table, segs, _alloc)
    c.keep.append(hl)
    return c


def _run(lib, c):
    if c.form == "seq":
        gin = None if c.gin is None else T.C.byref(c.gin)
        return lib.ort_host_trace_sequential_vjp(
            T.C.byref(c.lens), T.C.byref(c.rays_in), c.ref("batch"), c.ref("opt"),
            c.ref("params"), c.ref("cot"), c.rec_cot, c.rec, c.grad, gin)
    return lib.ort_host_trace_pupil_vjp(T.C.byref(c.lens), c.px, c.py, c.ref("batch"),
                                        c.ref("opt"), c.ref("params"), c.ref("cot"), c.grad)


ROWS = T.rows(device=False)


@pytest.mark.parametrize("lens,form,mode,mutate", [r[1:] for r in ROWS],
                         ids=[r[0] for r in ROWS])
def test_refused(lib, lenses, lens, form, mode, mutate):
    c = _call(lenses, lens, form, mode)
    mutate(c)
    assert _run(lib, c) == T.ERR_ARG
    assert np.all(c.grad_keep == T.SENTINEL)  # (grad_init = 0: nothing was written)


@pytest.mark.parametrize("form", T.BOTH)
@pytest.mark.parametrize("lens,mode", T.BASE_ACCEPTED)
def test_base_call_is_accepted(lib, lenses, lens, mode, form):
    """The table's unmutated base call returns ORT_OK and writes a finite gradient."""
    c = _call(lenses, lens, form, mode)
    c.params.grad_init = 1
    assert _run(lib, c) == T.OK
    assert np.all(np.isfinite(c.grad_keep)) and np.all(c.grad_keep != T.SENTINEL)


@pytest.mark.parametrize("form", T.BOTH)
@pytest.mark.parametrize("mode", (T.A, T.U))
def test_empty_batch_zeroes_an_overwritten_gradient(lib, lenses, form, mode):
    c = _call(lenses, "tma_fringe", form, mode)
    T.empty_batch_grad_init(c)
    assert _run(lib, c) == T.OK
    assert np.all(c.grad_keep == 0.0)


@pytest.mark.parametrize("form", T.BOTH)
@pytest.mark.parametrize("mode", (T.A, T.U))
def test_no_parameter_and_no_grad_in_is_accepted(lib, lenses, form, mode):
    c = _call(lenses, "tma_fringe", form, mode)
    T.no_param_no_grad_in(c)
    assert _run(lib, c) == T.OK
    assert np.all(c.grad_keep == T.SENTINEL)
