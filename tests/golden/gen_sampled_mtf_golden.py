"""Zernike fit, ZernikeOPD, SampledMTF and ThroughFocusMTF golden vectors: the REFERENCE's
ZernikeFit (optiland/zernike/fit.py), ZernikeOPD (optiland/wavefront/zernike_opd.py),
SampledMTF (optiland/mtf/sampled.py) and ThroughFocusMTF (optiland/analysis/
through_focus_mtf.py) with the NumPy backend on small pupils of the sample lenses.

Test infrastructure only, run in the build container (never on the GPU box):

    PYTHONPATH=tests/golden/shims:/root/reference PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/gen_sampled_mtf_golden.py

Writes tests/golden/sampled_mtf.npz, arrays "<case>/<name>". Per SampledMTF case: the pupil
the reference sheared (x_norm, y_norm, intensity, opd_waves), xpd, xpl, wavelength, the fitted
coefficients, the frequencies and the reference's MTF values, and two noise floors of the
reference itself: ref_self_diff, the largest difference between its MTF values and the same
sums recomputed here in another association (Horner radial sums, cos / sin by the angle
recurrence, one folded exponential of the range-reduced phase, numpy.sum), and
coeff_self_diff, the 2-norm of the difference between its coefficients and a Householder QR
solve of the same design matrix. Both are asserted to sit a factor 10 inside the tests'
bounds (tests/_sampled_mtf.py, restated below). Every pupil is asserted finite with no
zero-intensity point. ZernikeOPD cases add the design matrix. The ThroughFocusMTF case stores
per step the image-plane position, xpd, xpl, every field's pupil and the results.
"""

from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

import optiland.backend as be  # noqa: E402
from optiland.analysis.through_focus_mtf import ThroughFocusMTF  # noqa: E402
from optiland.mtf import SampledMTF  # noqa: E402
from optiland.samples.objectives import CookeTriplet, DoubleGauss  # noqa: E402
from optiland.wavefront import ZernikeOPD  # noqa: E402

be.set_backend("numpy")

NUM_RAYS = 32
FREQS = [(0.0, 0.0), (20.0, 0.0), (0.0, 20.0), (50.0, 50.0), (400.0, 0.0)]
LENSES = {"cooke": CookeTriplet, "dg": DoubleGauss}
# name -> (lens, field, zernike_type, zernike_terms)
MTF_CASES = {}
for _lens in LENSES:
    for _tag, _field in (("00", (0, 0)), ("07", (0, 0.7)), ("10", (0, 1))):
        MTF_CASES[f"{_lens}_{_tag}_fringe37"] = (_lens, _field, "fringe", 37)
MTF_CASES["cooke_07_standard37"] = ("cooke", (0, 0.7), "standard", 37)
MTF_CASES["dg_10_noll37"] = ("dg", (0, 1), "noll", 37)
MTF_CASES["cooke_10_fringe1"] = ("cooke", (0, 1), "fringe", 1)
MTF_CASES["cooke_10_fringe4"] = ("cooke", (0, 1), "fringe", 4)
OPD_CASES = {"zopd_cooke": ("cooke", (0, 0.7), "fringe"), "zopd_dg": ("dg", (0, 1), "standard")}
TF_CASE = dict(lens="cooke", num_steps=3, delta_focus=0.05, num_rays=NUM_RAYS, freq=20.0)
CHUNK = 256  # ORT_SAMPLED_OTF_CHUNK


# -- tests/_sampled_mtf.py, restated ------------------------------------------------------
def structure(zernike):
    """(n, m, norm, a_k) per term from the reference's own basis object."""
    out = []
    for n, m in zernike.indices:
        n, m = int(n), int(m)
        a = []
        for k in range((n - abs(m)) // 2 + 1):
            num = be.factorial(np.array(n - k))
            den = (be.factorial(np.array(k)) * be.factorial(np.array((n + abs(m)) // 2 - k))
                   * be.factorial(np.array((n - abs(m)) // 2 - k)))
            a.append(float((-1) ** k * num / den))
        out.append((n, m, float(zernike._norm_constant(n, m)), a))
    return out


def horner_terms(st, xs, ys):
    """Unit-coefficient term values [N, T] at Cartesian points: Horner in r^2, the angle by
    the addition recurrence from (xs, ys) / r; r as NumPy forms it."""
    r = np.sqrt(xs * xs + ys * ys)
    with np.errstate(invalid="ignore", divide="ignore"):
        c1 = np.where(r > 0, xs / r, 1.0)
        s1 = np.where(r > 0, ys / r, 0.0)
    r2 = r * r
    cols = []
    for n, m, norm, a in st:
        cm, sm, pm = np.ones_like(r), np.zeros_like(r), np.ones_like(r)
        for _ in range(abs(m)):
            cm, sm = cm * c1 - sm * s1, sm * c1 + cm * s1
            pm = pm * r
        P = np.full_like(r, a[0])
        for ak in a[1:]:
            P = P * r2 + ak
        cols.append(norm * (P * pm) * (cm if m >= 0 else sm))
    return np.stack(cols, axis=1), r


def folded_mtf(st, coeffs, x, y, inten, opd, sx, sy):
    A, r = horner_terms(st, x - sx, y - sy)
    t = opd - A @ coeffs
    term = np.where(r > 1.0, 0.0, inten * np.exp(2j * np.pi * (t - np.rint(t))))
    return abs(np.sum(term)) / np.sum(inten)


def weight_sum(st, coeffs):
    return float(sum(abs(c) * norm * sum(abs(v) for v in a)
                     for c, (_, _, norm, a) in zip(coeffs, st, strict=True)))


def mtf_bound(st, coeffs, opd, n):
    chunks = max(1, -(-n // CHUNK))
    s = weight_sum(st, coeffs)
    opd_max = float(np.max(np.abs(opd))) if n else 0.0
    return (2 * np.pi * (136.0 * s + 8.0 * opd_max) + chunks + np.log2(max(n, 2)) + 32.0) * 2.0**-53


def coeff_bound(cond, coeffs, n):
    t = len(coeffs)
    return 4.0 * np.sqrt(max(n, 1) * max(t, 1)) * cond * 2.0**-52 * float(np.linalg.norm(coeffs))


# -- the cases ----------------------------------------------------------------------------
def fit_record(fit, key):
    """Coefficients, the design matrix's condition number and the QR noise floor."""
    coeffs = np.asarray(fit.coeffs, dtype=np.float64)
    ones = type(fit.zernike)(np.ones(len(coeffs)))
    A = np.stack(ones.terms(np.asarray(fit.radius), np.asarray(fit.phi)), axis=1)
    sv = np.linalg.svd(A, compute_uv=False)
    cond = float(sv[0] / sv[-1])
    q, rr = np.linalg.qr(A)
    again = np.linalg.solve(rr, q.T @ np.asarray(fit.z))
    diff = float(np.linalg.norm(again - coeffs))
    bound = coeff_bound(cond, coeffs, A.shape[0])
    assert diff < bound / 10, (key, diff, bound)
    return coeffs, A, cond, float(sv[-1]), diff


def mtf_case(key, lens, field, kind, terms):
    m = SampledMTF(LENSES[lens](), field, "primary", num_rays=NUM_RAYS, zernike_terms=terms,
                   zernike_type=kind)
    x, y = np.asarray(m.x_norm, float), np.asarray(m.y_norm, float)
    inten, opd = np.asarray(m.intensity, float), np.asarray(m.opd_waves, float)
    assert np.all(np.isfinite(opd)) and np.all(inten > 0), key
    coeffs, _, cond, smin, cdiff = fit_record(m.zernike_fit, key)
    mtf = np.array([float(v) for v in m.calculate_mtf(FREQS)])
    # past the cutoff exactly 0; at zero frequency not 1 (W is the fit, not the raw OPD)
    assert mtf[-1] == 0.0 and (mtf[0] < 1.0 - 1e-9 or key != "cooke_10_fringe37"), (key, mtf)
    st = structure(m.zernike_fit.zernike)
    wl_mm = m.wavelength * 1e-3
    again = np.array([folded_mtf(st, coeffs, x, y, inten, opd,
                                 m.xpl * (wl_mm * fx) / (m.xpd / 2),
                                 m.xpl * (wl_mm * fy) / (m.xpd / 2)) for fx, fy in FREQS])
    diff = float(np.max(np.abs(again - mtf)))
    bound = mtf_bound(st, coeffs, opd, len(x))
    assert diff < bound / 10, (key, diff, bound)
    print(f"{key}: N {len(x)}, cond {cond:.3g}, max |c| {np.max(np.abs(coeffs)):.3g}, mtf "
          f"{mtf}, self diff {diff:.3g} (bound {bound:.3g}), coeff self diff {cdiff:.3g}")
    return dict(x_norm=x, y_norm=y, intensity=inten, opd_waves=opd, xpd=float(m.xpd),
                xpl=float(m.xpl), wavelength=float(m.wavelength), coeffs=coeffs,
                freqs=np.array(FREQS), mtf=mtf, cond=cond, sigma_min=smin, ref_self_diff=diff,
                coeff_self_diff=cdiff, field=np.array(field, float))


def opd_case(key, lens, field, kind):
    z = ZernikeOPD(LENSES[lens](), field, "primary", num_rings=6, zernike_type=kind,
                   num_terms=37)
    coeffs, A, cond, smin, cdiff = fit_record(z, key)
    assert z.num_pts == 127, key
    print(f"{key}: N {z.num_pts}, cond {cond:.3g}, coeff self diff {cdiff:.3g}")
    return dict(x=np.asarray(z.x, float), y=np.asarray(z.y, float), z=np.asarray(z.z, float),
                coeffs=coeffs, design=A, cond=cond, sigma_min=smin, coeff_self_diff=cdiff,
                field=np.array(field, float), rms=float(z.rms()))


def through_focus_case():
    c = TF_CASE
    lens = LENSES[c["lens"]]()
    pupils = []

    class Recording(SampledMTF):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            pupils.append(self)

    import optiland.analysis.through_focus_mtf as mod
    mod.SampledMTF = Recording
    try:
        tf = ThroughFocusMTF(lens, c["freq"], delta_focus=c["delta_focus"],
                             num_steps=c["num_steps"], num_rays=c["num_rays"])
    finally:
        mod.SampledMTF = SampledMTF
    nf = len(tf.fields)
    out = dict(positions=np.array([float(p) for p in tf.positions]),
               nominal_focus=float(tf.nominal_focus), n_fields=nf, num_steps=c["num_steps"],
               delta_focus=c["delta_focus"], freq=c["freq"], wavelength=float(tf.wavelength),
               fields=np.array([tuple(f) for f in tf.fields], float),
               x_norm=np.asarray(pupils[0].x_norm, float),
               y_norm=np.asarray(pupils[0].y_norm, float))
    worst = 0.0
    for s in range(c["num_steps"]):
        for f in range(nf):
            m = pupils[s * nf + f]
            inten, opd = np.asarray(m.intensity, float), np.asarray(m.opd_waves, float)
            assert np.all(np.isfinite(opd)) and np.all(inten > 0), (s, f)
            coeffs = np.asarray(m.zernike_fit.coeffs, float)
            st = structure(m.zernike_fit.zernike)
            got = np.array([float(tf.results[s][f]["tangential"]),
                            float(tf.results[s][f]["sagittal"])])
            wl_mm = m.wavelength * 1e-3
            sh = m.xpl * (wl_mm * c["freq"]) / (m.xpd / 2)
            again = np.array([folded_mtf(st, coeffs, out["x_norm"], out["y_norm"], inten, opd,
                                         sh, 0.0),
                              folded_mtf(st, coeffs, out["x_norm"], out["y_norm"], inten, opd,
                                         0.0, sh)])
            diff = float(np.max(np.abs(again - got)))
            bound = mtf_bound(st, coeffs, opd, len(inten))
            assert diff < bound / 10, (s, f, diff, bound)
            worst = max(worst, diff)
            out.update({f"intensity_{s}_{f}": inten, f"opd_{s}_{f}": opd, f"coeffs_{s}_{f}": coeffs,
                        f"mtf_{s}_{f}": got})
        out[f"xpd_{s}"] = float(pupils[s * nf].xpd)
        out[f"xpl_{s}"] = float(pupils[s * nf].xpl)
    out["ref_self_diff"] = worst
    print(f"through_focus: positions {out['positions']}, {nf} fields, self diff {worst:.3g}")
    print("  results", [[(round(r['tangential'], 6), round(r['sagittal'], 6)) for r in step]
                        for step in tf.results])
    return out


def main():
    arrays = {}
    for key, (lens, field, kind, terms) in MTF_CASES.items():
        for name, v in mtf_case(key, lens, field, kind, terms).items():
            arrays[f"{key}/{name}"] = np.asarray(v, dtype=np.float64)
    for key, (lens, field, kind) in OPD_CASES.items():
        for name, v in opd_case(key, lens, field, kind).items():
            arrays[f"{key}/{name}"] = np.asarray(v, dtype=np.float64)
    for name, v in through_focus_case().items():
        arrays[f"through_focus/{name}"] = np.asarray(v, dtype=np.float64)
    path = os.path.join(HERE, "sampled_mtf.npz")
    np.savez_compressed(path, **arrays)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
