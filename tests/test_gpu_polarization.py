"""Coatings and polarized ray tracing on the MI355X (trace_kernel<F_POL>,
csrc/ort_k_trace_pol.hip): the golden cases of tests/golden/polarized_cases.py through the
pupil and the sequential entry points, p_out NULL against non-NULL, the ray geometry
against the generic kernel family without polarization, P against the host build, and one
case under per-surface records. Tolerances: tests/_polarized.py."""

import numpy as np
import pytest
import torch

from optiland_pr_amd import _abi, polarization as pz, raytrace
from optiland_pr_amd.lowering import pupil_scalars, segment_params
from tests import _polarized as P

pytestmark = pytest.mark.gpu

RUNS = [pytest.param(c, t, s, id=f"{c}-{t[0]}-{s}") for c, t, s in P.all_runs()]
GEOM = ("x", "y", "z", "L", "M", "N", "opd")


@pytest.mark.parametrize("case,trace,state", RUNS)
def test_golden_parity_pupil_entry(case, trace, state):
    """Optic.trace / trace_generic with every surface recorded (the F_REC kernels)."""
    lens, rays = P.run(case, trace, state, None)
    assert rays.x.is_cuda
    g = P.fixture()
    base = f"{case}/{trace[0]}"
    dp, di, dsi = P.deviations(case, trace, state, rays, lens)
    print(case, trace[0], state, "dp", dp, "di", di, "dsi", dsi)
    tol = P.tol_of(case)
    assert dp <= tol and di <= tol and dsi <= tol
    geo_tol = 1e-9 if case in P.cases.NEWTON_CASES else 0.0
    for a in GEOM:
        np.testing.assert_allclose(getattr(rays, a).cpu().numpy(), g[f"{base}/{a}"], rtol=0,
                                   atol=geo_tol, err_msg=a)


def _pupil_inputs(lens, trace, dev):
    hx, hy, wl, rings = trace[2]
    EPL, EPD = pupil_scalars(lens)
    segs = np.stack([segment_params(lens, hx, hy, 0, EPL, EPD)])
    px, py = raytrace.pupil_arrays("hexapolar", rings, dev)
    return segs, px, py, wl


@pytest.mark.parametrize("case", ["cooke_fresnel", "cooke_fresnel_271", "mirror", "slab",
                                  "asphere"])
def test_sequential_entry_p_out_and_generic_family(case):
    """Without records (the kernels without F_REC): the sequential entry on generated rays
    equals the pupil entry bit for bit; p_out NULL leaves i unchanged; x .. N, opd are those
    of the existing trace of the same lens without coatings, bit for bit: the generic
    trace_kernel family for the Newton lens, the closed-form kernel's exact sequences
    (ORT_OPT_EXACT) for the others, which never reach that family."""
    trace = P.cases.CASES[case]["traces"][0]
    lens = P.build(case, "unpolarized")
    lens.surface_group.record = None
    dev = raytrace.get_device()
    segs, px, py, wl = _pupil_inputs(lens, trace, dev)
    n = px.numel()
    dl = raytrace.lens_for(lens, [wl], polarized=True)
    outs, planes = pz.trace_pupil_polarized(dl, segs, px, py, n, n, _abi.POL_UNPOLARIZED, None)
    outs0, none = pz.trace_pupil_polarized(dl, segs, px, py, n, n, _abi.POL_UNPOLARIZED, None,
                                           want_p=False)
    assert none is None
    for a, b in zip(outs, outs0, strict=True):
        torch.testing.assert_close(a, b, rtol=0, atol=0, equal_nan=True)
    # sequential entry: the generated rays as resident input
    r0 = raytrace.RealRays.empty(n, wl, device=dev)
    raytrace.generate_rays(segs, px, py, r0, n, n, apod=dl.apod)
    dls = raytrace.DeviceLens(dl.table, device=dev)
    seq, planes_s = pz.trace_sequential_polarized(
        dls, [getattr(r0, a) for a in _abi.RAY_FIELDS], _abi.POL_UNPOLARIZED, None)
    for a, b in zip(outs, seq, strict=True):
        assert torch.equal(a, b)
    assert torch.equal(planes, planes_s)
    # the same lens without coatings or a state through the existing kernels
    plain = P.cases.build(P.cases.CASES[case]["lens"], P.NS)
    for s in plain.surface_group.surfaces:
        s.interaction_model.coating = None
    plain.set_polarization("ignore")
    ref = raytrace.RealRays.empty(n, wl, device=dev)
    raytrace.trace_pupil(raytrace.lens_for(plain, [wl]), segs, px, py, ref, n, n, n,
                         exact_only=True)
    for k, a in enumerate(_abi.RAY_FIELDS):
        if a != "i":
            assert torch.equal(outs[k], getattr(ref, a)), a


def test_gpu_p_equals_host_build():
    case = "cooke_fresnel_271"
    trace = P.cases.CASES[case]["traces"][0]
    _, dev_rays = P.run(case, trace, "RCP", None)
    _, cpu_rays = P.run(case, trace, "RCP", "cpu")
    d = float((dev_rays.p.cpu() - cpu_rays.p).abs().max())
    di = float((dev_rays.i.cpu() - cpu_rays.i).abs().max())
    print("gpu vs host: p", d, "i", di)
    assert d <= P.TOL and di <= P.TOL
    for a in GEOM:
        assert torch.equal(getattr(dev_rays, a).cpu(), getattr(cpu_rays, a)), a


def test_custom_op_equals_class_path():
    """torch.ops.ort.trace_pupil_polarized on the CUDA key against Optic.trace."""
    from optiland_pr_amd import ops

    case = "cooke_fresnel_271"
    trace = P.cases.CASES[case]["traces"][0]
    lens, ref = P.run(case, trace, "RCP", None)
    lens.surface_group.record = None
    dev = raytrace.get_device()
    segs, px, py, wl = _pupil_inputs(lens, trace, dev)
    n = px.numel()
    dl = raytrace.lens_for(lens, [wl], polarized=True)
    args = ops.polarized_args(dl, segs, px, py, n, n, _abi.POL_POLARIZED, lens.polarization)
    rays, planes = torch.ops.ort.trace_pupil_polarized(*args)
    assert rays.is_cuda and planes.shape == (18, n)
    for k, a in enumerate(_abi.RAY_FIELDS):
        assert torch.equal(rays[k], getattr(ref, a)), a
    assert torch.equal(pz.planes_to_p(planes.reshape(-1), n), ref.p)
