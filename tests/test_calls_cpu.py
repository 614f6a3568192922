"""The Python call layer (_calls.py): the argument structs every entry point builds from
tensors, checked on host memory alone -- no library call, no GPU."""

import ctypes as C
import types

import numpy as np
import pytest
import torch

from optiland_pr_amd import _abi, _calls, _native

BATCH_FIELDS = [f for f, _ in _native.ort_batch._fields_]


def _fields(b):
    return [getattr(b, f) for f in BATCH_FIELDS]


def test_addr_of_tensors_arrays_and_none():
    t, a = torch.zeros(3, dtype=torch.float64), np.zeros(3)
    assert _calls.addr(None) is None
    assert _calls.addr(t) == t.data_ptr() and _calls.addr(a) == a.ctypes.data


def test_rays_struct_maps_none_to_null_and_tensors_to_their_addresses():
    ts = [torch.zeros(2, dtype=torch.float64) if k % 3 else None for k in range(8)]
    r = _calls.rays_struct(ts)
    for name, t in zip(_abi.RAY_FIELDS, ts, strict=True):
        assert getattr(r, name) == (None if t is None else t.data_ptr())


@pytest.mark.parametrize("n", [0, 1, 5])
def test_pupil_batch_fields(n):
    seg = torch.zeros(3 * _abi.SEGMENT.itemsize, dtype=torch.uint8)
    apod = torch.zeros(16, dtype=torch.uint8)
    # the lengths go as given with rays; an empty batch (no ray reads them) is raised to the
    # 1 the C front end requires
    b = _calls.pupil_batch(n, 2, n, seg, True, apod)
    assert _fields(b) == [n, 2, max(n, 1), 3, 1, seg.data_ptr(), None, apod.data_ptr()]
    b = _calls.pupil_batch(n, 0, 0, seg)
    lo = 0 if n else 1
    assert _fields(b) == [n, lo, lo, 3, 0, seg.data_ptr(), None, None]


@pytest.mark.parametrize("n", [0, 1, 5])
def test_resident_batch_fields(n):
    assert _fields(_calls.resident_batch(n)) == [n, max(n, 1), max(n, 1), 0, 0, None, None, None]
    seg = torch.zeros(2 * _abi.SEGMENT.itemsize, dtype=torch.uint8)
    b = _calls.resident_batch(n, group_len=4, seg=seg, seg_len=2)
    assert _fields(b) == [n, 2, 4, 2, 0, seg.data_ptr(), None, None]


def _table(abbe):
    mt = np.zeros(2, dtype=_abi.MATERIAL)
    if abbe:
        mt["kind"][1] = _abi.MAT_ABBE
    return types.SimpleNamespace(mat_table=mt)


def test_per_ray_wavelengths_expands_one_value_and_passes_n_through():
    cpu = torch.device("cpu")
    w = _calls.per_ray_wavelengths(_table(False), torch.tensor([0.55], dtype=torch.float64), 4, cpu, True)
    assert w.dtype == torch.float64 and w.is_contiguous() and w.tolist() == [0.55] * 4
    src = torch.linspace(0.4, 0.7, 4, dtype=torch.float64)
    assert _calls.per_ray_wavelengths(_table(False), src, 4, cpu, True).data_ptr() == src.data_ptr()
    w32 = _calls.per_ray_wavelengths(_table(False), src.float().reshape(2, 2), 4, cpu, True)
    assert w32.dtype == torch.float64 and w32.shape == (4,)
    with pytest.raises(ValueError, match="rays.w must hold one wavelength per ray"):
        _calls.per_ray_wavelengths(_table(False), src, 5, cpu, True)


def test_per_ray_wavelengths_abbe_range():
    cpu = torch.device("cpu")
    lo = torch.tensor([0.5, 0.379], dtype=torch.float64)
    ok = torch.tensor([0.380, 0.750], dtype=torch.float64)
    with pytest.raises(ValueError, match="Wavelength out of range for this model."):
        _calls.per_ray_wavelengths(_table(True), lo, 2, cpu, True)
    with pytest.raises(ValueError, match="Wavelength out of range for this model."):
        _calls.per_ray_wavelengths(_table(True), torch.tensor([0.751], dtype=torch.float64), 3, cpu, True)
    assert _calls.per_ray_wavelengths(_table(True), ok, 2, cpu, True).tolist() == [0.380, 0.750]
    # only the Abbe model has the range; a table without materials has none either
    _calls.per_ray_wavelengths(_table(False), lo, 2, cpu, True)
    _calls.per_ray_wavelengths(types.SimpleNamespace(mat_table=None), lo, 2, cpu, True)


def test_per_ray_wavelengths_without_validation_reads_no_data():
    """validate=False (the VJPs): out-of-range values pass, and a tensor without storage --
    any read of its values would raise -- goes through."""
    cpu = torch.device("cpu")
    bad = torch.tensor([0.1, 9.0], dtype=torch.float64)
    assert _calls.per_ray_wavelengths(_table(True), bad, 2, cpu, False).data_ptr() == bad.data_ptr()
    meta = torch.empty(3, dtype=torch.float64, device="meta")
    out = _calls.per_ray_wavelengths(_table(True), meta, 3, torch.device("meta"), False)
    assert out.shape == (3,)
    with pytest.raises((RuntimeError, NotImplementedError)):  # validating has to read it
        _calls.per_ray_wavelengths(_table(True), meta, 3, torch.device("meta"), True)


def test_workspace_is_reused_grown_and_kept_per_pool():
    cpu = torch.device("cpu")
    a = _calls.workspace("test_pool_a", cpu, 100)
    assert a.dtype == torch.uint8 and a.numel() == 100
    assert _calls.workspace("test_pool_a", cpu, 100) is a
    assert _calls.workspace("test_pool_a", cpu, 40) is a  # a smaller request: the same one
    big = _calls.workspace("test_pool_a", cpu, 101)
    assert big is not a and big.numel() == 101
    assert _calls.workspace("test_pool_a", cpu, 100) is big
    b = _calls.workspace("test_pool_b", cpu, 100)
    assert b is not big and b.data_ptr() != big.data_ptr()
    assert _calls.workspace("test_pool_c", cpu, 0).numel() == 8  # never a NULL address


def test_vjp_params_fields():
    table = types.SimpleNamespace(surfaces=np.zeros(2, dtype=_abi.SURFACE))
    zp = torch.full((3,), -1, dtype=torch.int32)
    need = torch.zeros(10, dtype=torch.int32)
    p = _calls.vjp_params(table, 4, _abi.VJP_UNROLLED, (zp, None, None), need, True)
    assert (p.n_param, p.mode, p.zern_param, p.surf_tangent, p.final_tangent) == (
        4, _abi.VJP_UNROLLED, zp.data_ptr(), None, None)
    assert (p.n_zern, p.grad_init, p.workspace, p.workspace_size) == (3, 1, None, 0)
    assert (p.slot_need, p.tape, p.n_mono, p.rms_stats, p.rms_grad) == (
        need.data_ptr(), None, 0, None, None)
    stats, g = torch.zeros(5, dtype=torch.float64), torch.zeros(1, dtype=torch.float64)
    tape = torch.zeros(7, dtype=torch.float64)
    primal = [torch.zeros(1, dtype=torch.float64) for _ in range(8)]
    p = _calls.vjp_params(table, 0, _abi.VJP_ADJOINT, (None, None, None), None, False,
                          tape=tape, primal=primal, rms=(stats, g))
    assert (p.n_zern, p.grad_init, p.zern_param, p.slot_need, p.n_mono) == (0, 0, None, None, 0)
    assert (p.tape, p.primal.x, p.primal.opd) == (tape.data_ptr(), primal[0].data_ptr(),
                                                  primal[7].data_ptr())
    assert (p.rms_stats, p.rms_grad) == (stats.data_ptr(), g.data_ptr())


def test_exports_are_the_prototype_tables():
    for exports, table in ((_native.EXPORTS, _native.DEVICE_PROTOTYPES),
                           (_native.HOST_EXPORTS, _native.HOST_PROTOTYPES)):
        assert len(exports) == len(set(exports)) and set(exports) == set(table)
        for name, (restype, argtypes) in table.items():
            assert name.startswith("ort_")
            assert restype is None or issubclass(restype, C._SimpleCData), name
            assert isinstance(argtypes, list), name
    assert "ort_abi_version" in _native.EXPORTS and "ort_host_abi_version" in _native.HOST_EXPORTS


def test_host_library_carries_every_prototype():
    lib = _native.load_host()
    for name, (restype, argtypes) in _native.HOST_PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
