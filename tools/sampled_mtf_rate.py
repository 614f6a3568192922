"""Time of SampledMTF's overlap sum (measurement tooling, not product): the CookeTriplet at
field (0, 0.7), the reference's default pupil (num_rays=128, uniform: 12,868 points), fringe,
37 terms, at F = 2 frequencies (what ThroughFocusMTF issues per step) and F = 64 (a sweep).

  * torch.ops.ort.sampled_otf (both launches), against
  * the same sum as eager torch on the same GPU, vectorised over the frequencies by
    broadcasting [F, N] -- the reference's per-frequency whole-array operations
    (mtf/sampled.py:162-205, zernike/base.py:42-102) without its Python loop over frequencies.
  Each side: HIP events around `--inner` back-to-back calls per sample, the two sides
  interleaved, the median of 7 samples after warm-up.
  * where one SampledMTF(...) plus calculate_mtf(64 frequencies) spends its time: the
    Wavefront (traces and the OPD kernel), the read-back plus host lstsq of ZernikeFit, the
    paraxial XPD / XPL, and calculate_mtf with its read-back (host clock, each phase ended by
    a device synchronise; median of 7).

Prints one JSON line. A run without a GPU fails (a CPU time says nothing about the MI355X).

    python tools/sampled_mtf_rate.py [--num-rays 128] [--inner 20]
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def eager_otf(x, y, inten, opd, coeffs, structure, sx, sy):
    """otf [F] complex by whole-tensor operations on [F, N] (complex128), the reference's
    operations: power sums, cos / sin of m * arctan2, two exponentials, mask, product, sum."""
    xs = x[None, :] - sx[:, None]
    ys = y[None, :] - sy[:, None]
    r = torch.sqrt(xs**2 + ys**2)
    phi = torch.arctan2(ys, xs)
    w = torch.zeros_like(r)
    for c, (norm, n, m, a, _) in zip(coeffs.unbind(0), structure, strict=True):
        radial = torch.zeros_like(r)
        for k, ak in enumerate(a):
            radial = radial + ak * r ** (n - 2 * k)
        az = torch.cos(m * phi) if m >= 0 else torch.sin(abs(m) * phi)
        w = w + c * norm * radial * az
    p1 = torch.sqrt(inten) * torch.exp(1j * 2 * torch.pi * opd)
    p2 = torch.sqrt(inten) * torch.exp(-1j * 2 * torch.pi * w)
    p2 = torch.where(r > 1.0, torch.zeros_like(p2), p2)
    return torch.sum(p1[None, :] * p2, dim=1)


def sample_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def interleaved(fa, fb, inner, samples=7, warmup=3):
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(samples):
        a.append(sample_ms(fa, inner))
        b.append(sample_ms(fb, max(1, inner // 4)))
    return statistics.median(a), statistics.median(b), a, b


def main():
    from optiland_pr_amd import SampledMTF
    from optiland_pr_amd.analysis import Wavefront
    from optiland_pr_amd.geometries import _zernike_structure
    from optiland_pr_amd.samples import CookeTriplet
    from optiland_pr_amd.zernike import ZernikeFit

    if not torch.cuda.is_available():
        raise SystemExit("sampled_mtf_rate: needs the MI355X")
    num_rays, inner = _arg("--num-rays", 128), _arg("--inner", 20)
    lens, field = CookeTriplet(), (0, 0.7)
    m = SampledMTF(lens, field, "primary", num_rays=num_rays)
    dev = m.opd_waves.device
    structure = _zernike_structure("fringe", 37)
    cutoff = 0.8 * abs(float(m.xpd)) / (abs(float(m.xpl)) * m.wavelength * 1e-3)
    out = {"lens": "CookeTriplet (0, 0.7) primary", "num_rays": num_rays,
           "pupil_points": int(m.x_norm.numel()), "terms": 37, "inner_calls_per_sample": inner}
    for nf in (2, 64):
        f = np.linspace(0.0, cutoff, nf)
        from optiland_pr_amd.mtf import pupil_shears
        sx, sy = pupil_shears([(v, 0.5 * v) for v in f], m.wavelength, m.xpd, m.xpl)
        sx, sy = torch.as_tensor(sx, device=dev), torch.as_tensor(sy, device=dev)

        def op():
            return torch.ops.ort.sampled_otf(m.x_norm, m.y_norm, m.intensity, m.opd_waves,
                                             m.zernike_fit.coeffs, "fringe", sx, sy)

        def eager():
            return eager_otf(m.x_norm, m.y_norm, m.intensity, m.opd_waves,
                             m.zernike_fit.coeffs, structure, sx, sy)

        ms_op, ms_eager, a, b = interleaved(op, eager, inner)
        o, e = op(), eager()
        diff = float(torch.max(torch.abs(torch.complex(o[:, 0], o[:, 1]) - e))
                     / m.otf_at_zero)
        out[f"F{nf}"] = {"kernel_ms": ms_op, "eager_ms": ms_eager,
                         "eager_over_kernel": ms_eager / ms_op,
                         "kernel_ms_min_max": [min(a), max(a)],
                         "eager_ms_min_max": [min(b), max(b)],
                         "max_otf_diff_over_sum_I": diff}
    # where a whole SampledMTF + calculate_mtf(64) goes
    freqs = [(float(v), 0.0) for v in np.linspace(0.0, cutoff, 64)]
    phases = {"wavefront_ms": [], "fit_ms": [], "paraxial_ms": [], "calculate_mtf_ms": [],
              "total_ms": []}
    for k in range(8):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wf = Wavefront(lens, fields=[field], wavelengths=[m.wavelength], num_rays=num_rays,
                       distribution="uniform")
        d = wf.get_data(field, m.wavelength)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ZernikeFit(m.x_norm, m.y_norm, d.opd, "fringe", 37)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        lens.paraxial.XPD(), lens.paraxial.XPL()
        t3 = time.perf_counter()
        m.calculate_mtf(freqs)
        t4 = time.perf_counter()
        SampledMTF(lens, field, "primary", num_rays=num_rays).calculate_mtf(freqs)
        t5 = time.perf_counter()
        if k == 0:
            continue  # warm-up
        for name, dt in zip(phases, (t1 - t0, t2 - t1, t3 - t2, t4 - t3, t5 - t4), strict=True):
            phases[name].append(dt * 1e3)
    out["sampled_mtf_64_frequencies"] = {k: statistics.median(v) for k, v in phases.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
