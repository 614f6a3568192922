"""No GPU: optiland_pr_amd.tolerancing against the reference's tolerancing module
(tests/golden/tolerancing.npz, gen_tolerancing_golden.py) through the per-trial loop on the
host build, the interface's errors and names, and the stacked tables ort_trace_ensemble
reads."""

import numpy as np
import pytest

from tests import _tolerancing as TT
from optiland_pr_amd import _abi
from optiland_pr_amd import tolerancing as T
from optiland_pr_amd.samples import CookeTriplet, ReverseTelephotoAsphere

A_COLUMNS = ["Radius of Curvature, Surface 1", "Thickness, Surface 1", "Tilt X, Surface 3",
             "Decenter Y, Surface 4", "Refractive Index, Surface 1", "0: rms spot size",
             "1: rms spot size", "2: rms spot size"]


@pytest.fixture(scope="module")
def golden():
    return TT.fixture()


@pytest.fixture(scope="module")
def monte_carlo_cpu():
    t = TT.case_a(device="cpu")
    mc = T.MonteCarlo(t)
    mc.run(TT.TRIALS)
    return t, mc


def test_sampled_values_equal_the_fixture_bit_for_bit(golden, monte_carlo_cpu):
    _, mc = monte_carlo_cpu
    for c in A_COLUMNS[:5]:
        assert mc.results[c].dtype == np.float64
        assert mc.results[c].tobytes() == golden[f"A/{c}"].tobytes(), c


def test_columns_and_order(golden, monte_carlo_cpu):
    _, mc = monte_carlo_cpu
    assert list(mc.results) == A_COLUMNS == [str(c) for c in golden["A/columns"]]
    assert all(v.dtype == np.float64 and v.shape == (TT.TRIALS,) for v in mc.results.values())
    df = mc.get_results()
    pd = pytest.importorskip("pandas")
    assert isinstance(df, pd.DataFrame) and list(df.columns) == A_COLUMNS


def test_monte_carlo_operands_against_the_fixture(golden, monte_carlo_cpu):
    t, mc = monte_carlo_cpu
    assert t.timing["mode"] == "loop"  # CPU tensors: the per-trial loop
    trials = [[golden[f"A/{c}"][i] for c in A_COLUMNS[:5]] for i in range(TT.TRIALS)]
    got = np.stack([mc.results[c] for c in A_COLUMNS[5:]], axis=1)
    want = np.stack([golden[f"A/{c}"] for c in A_COLUMNS[5:]], axis=1)
    assert np.all(np.isfinite(got))
    worst = TT.check_against_fixture("A host loop", t, trials, got, want, TT.K_HOST)
    print("worst error / bound, case A on the host build:", worst)


def test_nominal_targets(golden):
    t = TT.case_a(device="cpu")
    want = golden["A/targets"]
    got = np.array([[op.target for op in t.operands]])
    TT.check_against_fixture("A nominal", t, [[None] * 5], got, want[None], TT.K_HOST)


def test_sensitivity_analysis_against_the_fixture(golden):
    t = TT.case_b(device="cpu")
    sa = T.SensitivityAnalysis(t)
    sa.run()
    assert list(sa.results) == [str(c) for c in golden["B/columns"]] == [
        "perturbation_type", "perturbation_value", "0: rms spot size"]
    assert [str(v) for v in sa.results["perturbation_type"]] == [
        str(v) for v in golden["B/perturbation_type"]] == ["Radius of Curvature, Surface 1"] * 5
    pv = sa.results["perturbation_value"]
    assert pv.dtype == np.float64 and pv.tobytes() == golden["B/perturbation_value"].tobytes()
    got = sa.results["0: rms spot size"][:, None]
    worst = TT.check_against_fixture("B host loop", t, [[v] for v in pv], got,
                                     golden["B/0: rms spot size"][:, None], TT.K_HOST)
    print("worst error / bound, case B on the host build:", worst)


def test_validate_errors():
    lens = CookeTriplet()
    t = T.Tolerancing(lens, device="cpu")
    for cls in (T.SensitivityAnalysis, T.MonteCarlo):
        with pytest.raises(ValueError, match="No operands found in the tolerancing system."):
            cls(t)
    t.add_operand("rms_spot_size", TT.operand_data(lens, (0, 0)), target=0.0)
    for cls in (T.SensitivityAnalysis, T.MonteCarlo):
        with pytest.raises(ValueError, match="No perturbations found in the tolerancing system."):
            cls(t)
    for k in range(7):
        t.add_perturbation("radius", T.RangeSampler(20, 21, 2), surface_number=1 + k % 6)
    with pytest.raises(ValueError, match="Sensitivity analysis is limited to 6 perturbations."):
        T.SensitivityAnalysis(t)
    T.MonteCarlo(t)  # no such limit
    t.perturbations = t.perturbations[:1]
    for _ in range(6):
        t.add_operand("rms_spot_size", TT.operand_data(lens, (0, 0)), target=0.0)
    with pytest.raises(ValueError, match="Sensitivity analysis is limited to 6 operands."):
        T.SensitivityAnalysis(t)


def test_sensitivity_analysis_takes_range_samplers_only():
    t = TT.case_a(device="cpu")
    with pytest.raises(ValueError, match="Only range samplers are supported."):
        T.SensitivityAnalysis(t).run()


def test_perturbation_names_and_argument_errors():
    lens = CookeTriplet()
    names = {("radius", ()): "Radius of Curvature, Surface 2", ("conic", ()): "Conic Constant, Surface 2",
             ("thickness", ()): "Thickness, Surface 2", ("tilt", (("axis", "y"),)): "Tilt Y, Surface 2",
             ("decenter", (("axis", "x"),)): "Decenter X, Surface 2",
             ("index", (("wavelength", 0.55),)): "Refractive Index, Surface 2"}
    for (kind, kw), name in names.items():
        p = T.Perturbation(lens, kind, T.ScalarSampler(1.0), surface_number=2, **dict(kw))
        assert str(p.variable) == name
    with pytest.raises(ValueError, match='Invalid variable type "sag"'):
        T.Perturbation(lens, "sag", T.ScalarSampler(1.0), surface_number=2)
    with pytest.raises(ValueError, match='Invalid axis "z" for tilt variable.'):
        T.Perturbation(lens, "tilt", T.ScalarSampler(1.0), surface_number=2, axis="z")
    with pytest.raises(ValueError, match="Invalid parameter: mean"):
        T.DistributionSampler("normal", mean=0.0)
    with pytest.raises(ValueError, match="Unknown distribution: cauchy"):
        T.DistributionSampler("cauchy").sample()
    with pytest.raises(NotImplementedError):
        T.Tolerancing(lens).add_compensator("thickness", surface_number=2)
    with pytest.raises(ValueError, match="not supported"):
        T.Tolerancing(lens).add_operand("f2", {"optic": lens}, target=1.0)


def test_samplers():
    r = T.RangeSampler(1.0, 2.0, 3)
    assert [float(r.sample()) for _ in range(5)] == [1.0, 1.5, 2.0, 1.0, 1.5]  # wraps around
    assert T.ScalarSampler(3).sample() == 3 and T.ScalarSampler(3).size == 1
    g = np.random.default_rng(7)
    s = T.DistributionSampler("normal", seed=7, loc=2.0, scale=0.5)
    assert [s.sample() for _ in range(4)] == [g.normal(2.0, 0.5) for _ in range(4)]
    g = np.random.default_rng(8)
    s = T.DistributionSampler("uniform", seed=8, low=-1.0, high=3.0)
    assert [s.sample() for _ in range(4)] == [g.uniform(-1.0, 3.0) for _ in range(4)]


def _state(t):
    sg = t.optic.surface_group
    vals = [float(p.variable.value) for p in t.perturbations]
    vals += [float(v) for v in sg.positions.ravel()] + [float(v) for v in sg.radii]
    for s in sg.surfaces:
        cs = s.geometry.cs
        vals += [cs.x, cs.y, cs.z, cs.rx, cs.ry, cs.rz]
    return np.array(vals, dtype=np.float64).tobytes()


def test_reset_restores_every_parameter_bit_for_bit():
    t = TT.case_a(device="cpu")
    t.reset()  # (the index perturbation's ideal material: the state every trial starts from)
    before = _state(t)
    for _ in range(3):
        for p in t.perturbations:
            p.apply()
        assert _state(t) != before
        t.reset()
        assert _state(t) == before
    assert [p.value for p in t.perturbations] == [p.variable.initial_value
                                                  for p in t.perturbations]


# -- the stacked tables -------------------------------------------------------------------
def _variants(t, trials, pairs):
    tables, segs = [], []
    for values in trials:
        t.reset()
        for p, v in zip(t.perturbations, values, strict=True):
            if v is not None:
                p.set(v)
        table, seg = t.lower_variant(pairs)
        tables.append(table)
        segs.append(seg)
    t.reset()
    return tables, np.stack(segs)


def test_stacked_table_invariants(golden):
    t = TT.case_a(device="cpu")
    pairs = [(hx, hy, TT.WAVELENGTH) for hx, hy in t.optic.fields.get_field_coords()]
    cols = A_COLUMNS[:5]
    axial = [[golden[f"A/{c}"][i] if k in (0, 1, 4) else None for k, c in enumerate(cols)]
             for i in range(3)]
    tilted = axial[:2] + [[golden[f"A/{c}"][2] for c in cols]]
    tables, segs = _variants(t, axial, pairs)
    e = T.EnsembleTable(tables)
    S = tables[0].n_surfaces
    assert e.surfaces.shape == (3, S) and e.optics.shape == (3, 1, S)
    assert e.n_tab.shape == e.alpha_tab.shape == (3, 1, e.n_mat)
    assert e.cs_ops.shape == (3, e.cs_stride) and e.final_thickness.shape == (3,)
    assert segs.shape == (3, 3) and segs.dtype == _abi.SEGMENT
    assert e.meta(3)[8:] == [3, 3, e.cs_stride]
    for v, tb in enumerate(tables):
        assert e.surfaces[v].tobytes() == tb.surfaces.tobytes()
        assert e.optics[v].tobytes() == tb.optics.tobytes()
        assert e.final_thickness[v] == tb.final_thickness
    assert e.frame_flags == tables[0].frame_flags and e.frame_flags & _abi.LENS_AXIAL
    assert e.frame_flags & _abi.LENS_PLAIN and e.form_flags == _abi.LENS_SPHERES
    # one tilted, decentred variant: the flags are ANDed, the frame ops stay in its own block
    tables, _ = _variants(t, tilted, pairs)
    e = T.EnsembleTable(tables)
    assert [tb.frame_flags & _abi.LENS_AXIAL for tb in tables] == [1, 1, 0]
    assert not e.frame_flags & _abi.LENS_AXIAL
    assert e.frame_flags == tables[0].frame_flags & tables[1].frame_flags & tables[2].frame_flags
    assert e.cs_stride == max(len(tb.cs_ops) for tb in tables) >= 2
    for v in range(3):
        s = e.surfaces[v]
        assert np.all(s["cs_loc_off"] + s["n_cs_loc"] <= e.cs_stride)
        assert np.all(s["cs_glob_off"] + s["n_cs_glob"] <= e.cs_stride)
        assert np.all(s["cs_loc_off"] >= 0) and np.all(s["cs_glob_off"] >= 0)
        n = len(tables[v].cs_ops)
        assert e.cs_ops[v, :n].tobytes() == tables[v].cs_ops.tobytes()
    assert e.surfaces[2]["n_cs_loc"].sum() > 0 and e.surfaces[0]["n_cs_loc"].sum() == 0
    lens, ft = e.tensors("cpu")
    assert len(lens) == 9 and ft.numel() == 3
    assert lens[0].numel() == 3 * S * _abi.SURFACE.itemsize


def test_unsupported_lenses_do_not_stack():
    lens = ReverseTelephotoAsphere()
    t = T.Tolerancing(lens, device="cpu")
    t.add_perturbation("radius", T.ScalarSampler(30.0), surface_number=1)
    table, _ = t.lower_variant([(0.0, 0.0, 0.55)])
    with pytest.raises(T.UnsupportedEnsemble):
        T.EnsembleTable([table, table])
