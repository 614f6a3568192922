"""torch.ops.ort.trace_pupil_polarized on the CPU dispatch key (the host build): equal to
the class path bit for bit, torch.library.opcheck's schema / fake / autograd-registration /
AOT-dispatch checks, and a backward through it raises."""

import numpy as np
import pytest
import torch

from optiland_pr_amd import _abi, host, ops, polarization as pz
from optiland_pr_amd.distribution import create_distribution
from optiland_pr_amd.lowering import (lower_apodization, lower_surface_group, pupil_scalars,
                                      segment_params)
from tests import _polarized as P


def _args(case, state, want_p=True, requires_grad=False):
    trace = P.cases.CASES[case]["traces"][0]
    hx, hy, wl, rings = trace[2]
    lens = P.build(case, state)
    lens.surface_group.record = None
    table = lower_surface_group(lens.surface_group, [wl], polarized=True)
    table.apod = lower_apodization(lens)
    hl = host.HostLens(table)
    EPL, EPD = pupil_scalars(lens)
    segs = np.stack([segment_params(lens, hx, hy, 0, EPL, EPD)])
    d = create_distribution("hexapolar")
    d.generate_points(rings)
    px, py = (torch.as_tensor(np.array(v, dtype=np.float64)).requires_grad_(requires_grad)
              for v in (d.x, d.y))
    mode = pz.polarization_mode(lens.polarization)
    args = ops.polarized_args(hl, segs, px, py, px.numel(), px.numel(), mode,
                              lens.polarization, want_p=want_p)
    return lens, hl, trace, args


@pytest.mark.parametrize("case,state", [("cooke_fresnel", "LCP"), ("cooke_fresnel", "unpolarized"),
                                        ("cooke_clip_apod", "unpolarized"), ("asphere", "unpolarized"),
                                        ("cooke_simple", "ignore")])
def test_op_equals_class_path(case, state):
    _, hl, trace, args = _args(case, state)
    rays, planes = torch.ops.ort.trace_pupil_polarized(*args)
    n = args[-1][0]
    assert rays.shape == (8, n) and planes.shape == (18, n)
    _, ref = P.run(case, trace, state, "cpu")
    for k, a in enumerate(_abi.RAY_FIELDS):
        assert torch.equal(rays[k], getattr(ref, a)), a
    if state != "ignore":
        assert torch.equal(pz.planes_to_p(planes.reshape(-1), n), ref.p)
    _, _, _, args0 = _args(case, state, want_p=False)
    rays0, planes0 = torch.ops.ort.trace_pupil_polarized(*args0)
    assert planes0.shape == (18, 0) and torch.equal(rays0, rays)


@pytest.mark.parametrize("want_p", [True, False])
def test_opcheck(want_p):
    _, hl, _, args = _args("cooke_fresnel", "RCP", want_p=want_p)
    res = torch.library.opcheck(torch.ops.ort.trace_pupil_polarized.default, args)
    assert all(v == "SUCCESS" for v in res.values()), res


def test_backward_raises():
    _, hl, _, args = _args("cooke_fresnel", "H", requires_grad=True)
    rays, planes = torch.ops.ort.trace_pupil_polarized(*args)
    assert rays.requires_grad
    with pytest.raises(RuntimeError, match="forward only"):
        (rays.sum() + planes.sum()).backward()
