"""GPU: the device library's VJP entry points (ort_trace_sequential_vjp,
ort_trace_pupil_vjp) refuse a bad call with ORT_ERR_ARG before any launch (the gradient
buffer keeps its bytes), and accept an empty one. The host library's table
(tests/_vjp_refusals.py, expected codes read off csrc/ort_api.hip) with device buffers for
64 rays, plus the rows only the device has: ORT_NEWTON_WAVE, a workspace that is too small
or NULL. One accepted 64-ray adjoint call is compared with the unrolled mode's gradient at
tests/test_gpu_adjoint.py's tolerance for the lens (tma_fringe: rtol 1e-7).
"""

import ctypes as C

import numpy as np
import pytest

from tests import _vjp_refusals as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("needs the MI355X")
    return torch


@pytest.fixture(scope="module")
def lib(torch):
    from optiland_pr_amd import _native

    return _native.load()


@pytest.fixture(scope="module")
def lenses(torch):
    from optiland_pr_amd.raytrace import DeviceLens

    out = {}
    for name in T.LENSES:
        table, segs = T.lowered(name)
        out[name] = (DeviceLens(table), table, segs)
    return out


def _call(torch, lib, lenses, lens, form, mode):
    """The base call with a workspace of the size the library asks for."""
    dl, table, segs = lenses[lens]

    def alloc(arr):
        a = np.ascontiguousarray(arr)
        t = torch.from_numpy(a.view(np.uint8).reshape(-1).copy() if a.dtype.fields
                             else a.copy()).cuda()
        return t, t.data_ptr()

    c = T.Call(form, mode, dl.c, table, segs, alloc)
    c.keep.append(dl)
    size = lib.ort_vjp_workspace_size(C.byref(c.lens), C.byref(c.batch), C.byref(c.params))
    if size >= 0:  # (a lens or mode the library sizes no workspace for is refused anyway)
        ws = torch.empty(max(int(size), 256), dtype=torch.uint8, device="cuda")
        c.keep.append(ws)
        c.params.workspace = ws.data_ptr()
        c.params.workspace_size = ws.numel()
    return c


def _run(torch, lib, c):
    from optiland_pr_amd.raytrace import _stream_handle

    if c.form == "seq":
        gin = None if c.gin is None else C.byref(c.gin)
        rc = lib.ort_trace_sequential_vjp(
            C.byref(c.lens), C.byref(c.rays_in), c.ref("batch"), c.ref("opt"), c.ref("params"),
            c.ref("cot"), c.rec_cot, c.rec, c.grad, gin, _stream_handle())
    else:
        rc = lib.ort_trace_pupil_vjp(C.byref(c.lens), c.px, c.py, c.ref("batch"), c.ref("opt"),
                                     c.ref("params"), c.ref("cot"), c.grad, _stream_handle())
    torch.cuda.synchronize()
    return rc


def _workspace_short(c):
    c.params.workspace_size = c.params.workspace_size - 256 if c.mode == T.A else 0


DEVICE_ONLY = [
    ("newton_wave", T._set("opt", "newton_mode", T._abi.NEWTON_WAVE)),
    ("workspace_too_small", _workspace_short),
    ("workspace_null", T._set("params", "workspace", None)),
]
ROWS = T.rows(device=True) + [
    (f"{name}-{form}-mode{mode}", "tma_fringe", form, mode, mutate)
    for name, mutate in DEVICE_ONLY for form in T.BOTH for mode in (T.A, T.U)]


@pytest.mark.parametrize("lens,form,mode,mutate", [r[1:] for r in ROWS],
                         ids=[r[0] for r in ROWS])
def test_refused_before_any_launch(torch, lib, lenses, lens, form, mode, mutate):
    c = _call(torch, lib, lenses, lens, form, mode)
    mutate(c)
    assert _run(torch, lib, c) == T.ERR_ARG
    assert bool((c.grad_keep == T.SENTINEL).all())


@pytest.mark.parametrize("form", T.BOTH)
@pytest.mark.parametrize("mode", (T.A, T.U))
def test_empty_batch_zeroes_an_overwritten_gradient(torch, lib, lenses, form, mode):
    c = _call(torch, lib, lenses, "tma_fringe", form, mode)
    T.empty_batch_grad_init(c)
    assert _run(torch, lib, c) == T.OK
    assert bool((c.grad_keep == 0.0).all())


@pytest.mark.parametrize("form", T.BOTH)
@pytest.mark.parametrize("mode", (T.A, T.U))
def test_no_parameter_and_no_grad_in_is_accepted(torch, lib, lenses, form, mode):
    c = _call(torch, lib, lenses, "tma_fringe", form, mode)
    T.no_param_no_grad_in(c)
    assert _run(torch, lib, c) == T.OK
    assert bool((c.grad_keep == T.SENTINEL).all())


def test_accepted_adjoint_equals_unrolled(torch, lib, lenses):
    """The base pupil call itself, 64 rays: the adjoint's gradient against the forward
    mode's (test_gpu_adjoint.py's tolerance for tma_fringe)."""
    grads = []
    for mode in (T.A, T.U):
        c = _call(torch, lib, lenses, "tma_fringe", "pupil", mode)
        c.params.grad_init = 1
        assert _run(torch, lib, c) == T.OK
        grads.append(c.grad_keep.cpu().numpy())
    ga, gu = grads
    print("adjoint", ga, "unrolled", gu)
    assert np.all(np.isfinite(ga)) and np.any(gu != 0.0)
    rtol = 1e-7
    np.testing.assert_allclose(ga, gu, rtol=rtol, atol=rtol * 1e-2 * np.max(np.abs(gu)))
