"""The Python call layer (_calls.py): the argument structs every entry point builds from
tensors, checked on host memory alone -- no library call, no GPU -- and the forward-trace
entry table, its one status path and the shared helpers, checked on a recording stand-in
library."""

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


# --------------------------------------------------------------------------------------
# the forward-trace entry table, on a recording stand-in library
# --------------------------------------------------------------------------------------
class _Recorder:
    """A stand-in library: every symbol records (name, args) and returns rc."""

    def __init__(self, rc=0):
        self.calls, self.rc = [], rc

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return self.rc

        return fn


EXTRA_STRUCT = {None: None, "polarized": _native.ort_polarization, "scatter": _native.ort_scatter}
STREAM = C.c_void_p(0x5EED)


def _parts(key):
    library, kind, extra = key
    f64 = [torch.zeros(3, dtype=torch.float64) for _ in range(3)]
    p = types.SimpleNamespace(
        lens=_native.ort_lens(), out=_native.ort_rays(), batch=_native.ort_batch(),
        opt=_native.ort_options(), rec=f64[0], counts=torch.zeros(4, dtype=torch.int32),
        status=np.zeros(1, dtype=np.int32),
        src=(f64[1], f64[2]) if kind == "pupil" else _native.ort_rays(),
        extra=None if extra is None else EXTRA_STRUCT[extra]())
    return p


def _call(lib, key, p):
    _calls.call_forward(lib, _calls.FORWARD[key], p.lens, p.src, p.out, p.batch, p.opt, p.rec,
                        p.counts, p.status, p.extra, STREAM)


def test_forward_table_is_every_forward_symbol_of_both_libraries():
    import re

    pat = re.compile(r"ort_(host_)?trace_(pupil|sequential)(_polarized|_scatter)?$")
    declared = {n for n in (*_native.DEVICE_PROTOTYPES, *_native.HOST_PROTOTYPES) if pat.match(n)}
    assert len(_calls.FORWARD) == 12
    assert {e.name for e in _calls.FORWARD.values()} == declared
    assert set(_calls.FORWARD) == {(lib, kind, extra) for lib in ("device", "host")
                                   for kind in ("pupil", "sequential")
                                   for extra in (None, "polarized", "scatter")}


@pytest.mark.parametrize("key", list(_calls.FORWARD), ids=lambda k: "-".join(map(str, k)))
def test_forward_call_matches_the_declared_prototype(key):
    library, kind, extra = key
    entry = _calls.FORWARD[key]
    table = _native.HOST_PROTOTYPES if library == "host" else _native.DEVICE_PROTOTYPES
    assert entry.name.startswith("ort_host_") == (library == "host")
    assert (kind in entry.name) and (extra is None or entry.name.endswith("_" + extra))
    argtypes = table[entry.name][1]  # the symbol is one _native declares
    lib, p = _Recorder(), _parts(key)
    _call(lib, key, p)
    (name, args), = lib.calls
    assert name == entry.name and len(args) == len(argtypes)
    # the order: every struct argument is a reference to the part of that type, at the place
    # the prototype has a pointer to it; everything else is a plain address where it has PTR
    for a, t in zip(args, argtypes, strict=True):
        if t is _native.PTR:
            assert a is None or isinstance(a, (int, C.c_void_p)), (name, a)
        else:
            assert isinstance(a._obj, t._type_), (name, a._obj, t)
    assert args[0]._obj is p.lens
    if kind == "pupil":
        assert args[1:3] == (p.src[0].data_ptr(), p.src[1].data_ptr()) and args[3]._obj is p.out
        rest = args[4:]
    else:
        assert args[1]._obj is p.src and args[2]._obj is p.out
        rest = args[3:]
    assert rest[0]._obj is p.batch and rest[1]._obj is p.opt
    tail = [p.counts.data_ptr(), p.status.ctypes.data]
    # rec is absent only for ort_host_trace_pupil
    has_rec = p.rec.data_ptr() in [a for a in args if isinstance(a, int)]
    assert has_rec == (entry.name != "ort_host_trace_pupil") == entry.has_rec
    assert list(rest[2:4 + has_rec]) == ([p.rec.data_ptr()] if has_rec else []) + tail
    # the extra struct: last on host entries, last but one (before the stream) on device ones
    if library == "host":
        assert STREAM not in args
        if extra is not None:
            assert args[-1]._obj is p.extra
    else:
        assert args[-1] is STREAM
        if extra is not None:
            assert args[-2]._obj is p.extra
    assert len(rest) == 4 + has_rec + (extra is not None) + (library == "device")


@pytest.mark.parametrize("key", list(_calls.FORWARD), ids=lambda k: "-".join(map(str, k)))
def test_forward_call_checks_the_return_code_by_symbol(key):
    name = _calls.FORWARD[key].name
    with pytest.raises(RuntimeError, match=f"^{name} failed: ORT_ERR_ARG$"):
        _call(_Recorder(rc=-1), key, _parts(key))
    with pytest.raises(RuntimeError, match=f"^{name} failed: ORT_ERR_LAUNCH$"):
        _call(_Recorder(rc=-3), key, _parts(key))


def test_forward_entry_picks_the_cell_of_the_extra_struct():
    pol, scat = _native.ort_polarization(), _native.ort_scatter()
    for library in ("device", "host"):
        for kind in ("pupil", "sequential"):
            assert _calls.forward_entry(library, kind) == (_calls.FORWARD[library, kind, None], None)
            e, x = _calls.forward_entry(library, kind, pol=pol)
            assert e is _calls.FORWARD[library, kind, "polarized"] and x is pol
            e, x = _calls.forward_entry(library, kind, scat=scat)
            assert e is _calls.FORWARD[library, kind, "scatter"] and x is scat
    with pytest.raises(ValueError, match="BSDF surfaces together with coatings"):
        _calls.forward_entry("host", "pupil", pol, scat)


@pytest.mark.parametrize("library", ["device", "host"])
def test_generate_call_matches_the_declared_prototype(library):
    table = _native.HOST_PROTOTYPES if library == "host" else _native.DEVICE_PROTOTYPES
    name = _calls.GENERATE[library]
    argtypes = table[name][1]
    px, py = (torch.zeros(2, dtype=torch.float64) for _ in range(2))
    out, batch, lib = _native.ort_rays(), _native.ort_batch(), _Recorder()
    _calls.call_generate(lib, library, px, py, out, batch, STREAM)
    (got, args), = lib.calls
    assert got == name and len(args) == len(argtypes)
    assert args[:2] == (px.data_ptr(), py.data_ptr())
    assert args[2]._obj is out and args[3]._obj is batch
    assert (args[-1] is STREAM) == (library == "device")
    with pytest.raises(RuntimeError, match=f"^{name} failed: ORT_ERR_ARG$"):
        _calls.call_generate(_Recorder(rc=-1), library, px, py, out, batch, STREAM)


# --------------------------------------------------------------------------------------
# the one status path
# --------------------------------------------------------------------------------------
def _bsdf_table(has):
    bsdf = np.zeros(3, dtype=_abi.BSDF)
    if has:
        bsdf[1] = (_abi.BSDF_GAUSSIAN, 0, 0.25)
        bsdf[2] = (_abi.BSDF_LAMBERTIAN, 0, 0.0)
    return types.SimpleNamespace(bsdf=bsdf, has_bsdf=has)


def test_status_bits_raise_their_exceptions():
    from optiland_pr_amd import raytrace, scatter

    cases = [
        (_abi.STATUS_BAD_APODIZATION, ValueError,
         "the apodization record holds a kind the trace core does not know"),
        (_abi.STATUS_BAD_GEOMETRY, ValueError,
         "the lens table holds a geometry id the trace core does not know "
         "(library / host ABI mismatch?)"),
        (_abi.STATUS_ZERNIKE_RANGE, raytrace.ZernikeRangeError,
         "Zernike coordinates must be normalized to [-1, 1]. Consider updating the "
         "normalization radius to 1.1x the surface aperture."),
        (_abi.STATUS_CHEBYSHEV_RANGE, raytrace.ChebyshevRangeError,
         "Chebyshev input coordinates must be normalized to [-1, 1]. Consider "
         "updating the normalization factors."),
        (_abi.STATUS_SCATTER_ATTEMPTS, scatter.ScatterAttemptsError,
         "BSDF scattering used up its attempts"),
    ]
    assert len({bit for bit, _, _ in cases}) == 5
    for bit, exc, msg in cases:
        for table in (None, _bsdf_table(False)):
            with pytest.raises(exc) as e:
                _calls.raise_status(bit, table, 9)
            assert type(e.value) is exc and str(e.value) == msg
    assert raytrace.ZernikeRangeError is _calls.ZernikeRangeError
    assert issubclass(_calls.ZernikeRangeError, ValueError)
    assert issubclass(_calls.ChebyshevRangeError, ValueError)
    assert issubclass(scatter.ScatterAttemptsError, ValueError)
    # the order of the parent's checks when several bits are set
    both = _abi.STATUS_ZERNIKE_RANGE | _abi.STATUS_CHEBYSHEV_RANGE | _abi.STATUS_SCATTER_ATTEMPTS
    with pytest.raises(raytrace.ZernikeRangeError):
        _calls.raise_status(both)
    with pytest.raises(ValueError, match="apodization record"):
        _calls.raise_status(both | _abi.STATUS_BAD_APODIZATION | _abi.STATUS_BAD_GEOMETRY)


def test_status_scatter_attempts_names_surface_and_sigma():
    from optiland_pr_amd import scatter

    with pytest.raises(scatter.ScatterAttemptsError) as e:
        _calls.raise_status(_abi.STATUS_SCATTER_ATTEMPTS, _bsdf_table(True), 7)
    assert str(e.value) == (
        "BSDF scattering: a ray was rejected 7 times (scatter_max_attempts) at "
        "surface 2 (GaussianBSDF, sigma=0.25), surface 3 (LambertianBSDF); its direction is "
        "NaN. A Lambertian draw is accepted with probability >= 0.39, so this means a sigma far "
        "too large for a direction cosine.")
    assert str(e.value) == str(scatter.attempts_error(scatter.describe(_bsdf_table(True)), 7))
    # the lens's default cap when none is given
    with pytest.raises(scatter.ScatterAttemptsError,
                       match=f"rejected {scatter.DEFAULT_MAX_ATTEMPTS} times"):
        _calls.raise_status(_abi.STATUS_SCATTER_ATTEMPTS, _bsdf_table(True))


def test_zero_status_raises_nothing():
    assert _calls.raise_status(0) is None
    assert _calls.raise_status(0, _bsdf_table(True), 7) is None


def test_deferred_and_direct_device_status_take_the_same_path():
    """raytrace._raise_status (the launches' and check_pending's reader) hands the lens's
    table and attempt cap to _calls.raise_status; None (no status kept) and 0 pass."""
    from optiland_pr_amd import raytrace, scatter

    lens = types.SimpleNamespace(table=_bsdf_table(True), scatter=(3, 5))
    assert raytrace._raise_status(None, lens) is None
    assert raytrace._raise_status(0, lens) is None
    assert raytrace._raise_status(torch.zeros(1, dtype=torch.int32), lens) is None
    with pytest.raises(scatter.ScatterAttemptsError, match="rejected 5 times .* at surface 2"):
        raytrace._raise_status(torch.tensor([_abi.STATUS_SCATTER_ATTEMPTS], dtype=torch.int32),
                               lens)
    with pytest.raises(raytrace.ChebyshevRangeError):
        raytrace._raise_status(_abi.STATUS_CHEBYSHEV_RANGE)


# --------------------------------------------------------------------------------------
# the shared helpers
# --------------------------------------------------------------------------------------
def test_real_rays_of_aliases_its_tensors_and_keeps_the_subclass():
    from optiland_pr_amd.polarization import PolarizedRays
    from optiland_pr_amd.raytrace import RealRays

    fields = [torch.full((3,), float(k), dtype=torch.float64) for k in range(8)]
    r = RealRays.of(fields)
    assert type(r) is RealRays and len(r) == 3 and r.is_normalized
    for a, t in zip(_abi.RAY_FIELDS, fields, strict=True):
        assert getattr(r, a).data_ptr() == t.data_ptr() and getattr(r, a) is t
    assert not hasattr(r, "w")  # set only when given
    w = torch.full((3,), 0.55, dtype=torch.float64)
    rw = RealRays.of(fields, w)
    assert rw.w is w and rw.x.data_ptr() == fields[0].data_ptr()
    c = r.c_struct()
    assert [getattr(c, a) for a in _abi.RAY_FIELDS] == [t.data_ptr() for t in fields]
    p = PolarizedRays.of(fields, w)
    assert type(p) is PolarizedRays and p.opd.data_ptr() == fields[7].data_ptr() and p.w is w
    with pytest.raises(ValueError):
        RealRays.of(fields[:7])
    e = RealRays.empty(4, 0.6, device=torch.device("cpu"))
    assert len(e) == 4 and e.w.tolist() == [0.6] * 4 and e.is_normalized
    assert len({getattr(e, a).data_ptr() for a in _abi.RAY_FIELDS}) == 8


def test_bytes_tensor_round_trips_a_structured_array():
    arr = np.zeros(2, dtype=_abi.SEGMENT)
    arr.view(np.uint8)[:] = np.arange(arr.nbytes, dtype=np.uint64) * 37 % 251
    raw = arr.tobytes()
    t = _calls.bytes_tensor(arr)
    assert t.dtype == torch.uint8 and t.shape == (2 * _abi.SEGMENT.itemsize,)
    assert t.numpy().tobytes() == raw
    back = np.frombuffer(t.numpy().tobytes(), dtype=_abi.SEGMENT)
    assert back.tobytes() == raw and back.shape == (2,)
    arr.view(np.uint8)[:] = 0  # its own memory: the source can change afterwards
    assert t.numpy().tobytes() == raw
    # a non-contiguous view goes as its own elements' bytes
    two = np.zeros(4, dtype=_abi.SEGMENT)
    two.view(np.uint8)[:] = np.arange(two.nbytes, dtype=np.uint64) % 256
    assert _calls.bytes_tensor(two[::2]).numpy().tobytes() == two[::2].tobytes()


def test_segments_of_passes_tensors_and_uploads_arrays_through_the_lens():
    seen = []

    class Lens:
        def resident(self, slot, arr):
            seen.append((slot, arr))
            return "resident"

    t = torch.zeros(_abi.SEGMENT.itemsize, dtype=torch.uint8)
    assert _calls.segments_of(Lens(), t) is t and not seen
    segs = np.zeros(2, dtype=_abi.SEGMENT)
    assert _calls.segments_of(Lens(), segs) == "resident"
    (slot, arr), = seen
    assert slot == "segments" and arr.dtype == _abi.SEGMENT and arr.shape == (2,)


def test_host_lens_resident_keeps_structured_tables_as_bytes():
    from optiland_pr_amd import host

    hl = host.HostLens.__new__(host.HostLens)
    hl._resident = {}
    segs = np.zeros(2, dtype=_abi.SEGMENT)
    segs.view(np.uint8)[:] = 7
    t = hl.resident("segments", segs)
    assert t.dtype == torch.uint8 and t.numpy().tobytes() == segs.tobytes()
    assert hl.resident("segments", segs.copy()) is t  # unchanged bytes: the same tensor
    segs.view(np.uint8)[0] = 9
    assert hl.resident("segments", segs) is not t
    f = hl.resident("plain", np.arange(3.0))
    assert f.dtype == torch.float64 and f.tolist() == [0.0, 1.0, 2.0]
