"""Throughput of the Huygens-Fresnel PSF (measurement tooling, not product): the DoubleGauss
at field (0, 0.7), the reference's default sizes (128-wide uniform pupil, 128 x 128 image).

  * the summation op alone (torch.ops.ort.huygens_psf: both launches), HIP events around
    N calls on the current stream after warm-up;
  * the whole HuygensPSF construction (traces, wavefront, image grid, both sums), host
    clock around constructions that end in a device synchronise;
  * the same sum as batched eager torch tensor operations on the same GPU, 1024 image
    points per batch -- the algorithm of the reference's TorchSummation
    (psf/huygens_fresnel_strategies.py:175-267) restated here: what a user of the
    reference's torch backend gets on this card.

Prints one JSON line. A run without a GPU fails (a CPU time says nothing about the MI355X).

    python tools/huygens_rate.py [--num-rays 128] [--image-size 128] [--steps 20] [--once]

--once: build one PSF and run the op once (for a rocprofv3 --kernel-trace --stats run).
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def eager_sum(image, pupil, wavelength_mm, rp, batch=1024):
    """|field|^2 by batched whole-tensor operations (complex128)."""
    ix, iy, iz = (t.reshape(-1) for t in image)
    px, py, pz, amp, opd = (t.reshape(1, -1) for t in pupil)
    k = 2.0 * torch.pi / wavelength_mm
    field = torch.zeros(ix.numel(), dtype=torch.complex128, device=ix.device)
    phase_p = torch.exp(-1j * k * opd)
    nx, ny, nz = px / rp, py / rp, pz / rp
    for i in range(0, ix.numel(), batch):
        dx = ix[i:i + batch].reshape(-1, 1) - px
        dy = iy[i:i + batch].reshape(-1, 1) - py
        dz = iz[i:i + batch].reshape(-1, 1) - pz
        R = torch.sqrt(dx**2 + dy**2 + dz**2)
        wave = torch.exp(1j * k * R) / R
        obliq = 0.5 * (1.0 + (dx * nx + dy * ny + dz * nz) / R)
        field[i:i + batch] = torch.sum(amp * phase_p * wave * obliq, dim=1)
    return (torch.abs(field) ** 2).reshape(image[0].shape)


def events_ms(fn, steps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def main():
    from optiland_pr_amd import HuygensPSF
    from optiland_pr_amd.samples import DoubleGauss

    if not torch.cuda.is_available():
        raise SystemExit("huygens_rate: needs the MI355X")
    num_rays, size = _arg("--num-rays", 128), _arg("--image-size", 128)
    steps = _arg("--steps", 20)
    field, wl = (0, 0.7), 0.5876
    lens = DoubleGauss()
    p = HuygensPSF(lens, field, wl, num_rays=num_rays, image_size=size)
    d = p.get_data(p.fields[0], p.wavelengths[0])
    image = p._get_image_coordinates()
    pupil = (d.pupil_x, d.pupil_y, d.pupil_z, d.intensity, d.opd * (wl * 1e-3))
    rp = float(d.radius)

    def op():
        return torch.ops.ort.huygens_psf(*image, *pupil, wl * 1e-3, rp)

    if "--once" in sys.argv:
        op()
        torch.cuda.synchronize()
        return
    terms = image[0].numel() * pupil[0].numel()
    ms_op = events_ms(op, steps)
    ms_eager = events_ms(lambda: eager_sum(image, pupil, wl * 1e-3, rp), max(2, steps // 4), 1)
    norm = p._get_normalization()
    diff = float(torch.max(torch.abs(op() - eager_sum(image, pupil, wl * 1e-3, rp))) / norm * 100.0)
    t0 = time.perf_counter()
    for _ in range(3):
        HuygensPSF(lens, field, wl, num_rays=num_rays, image_size=size)
        torch.cuda.synchronize()
    ms_total = (time.perf_counter() - t0) / 3 * 1e3
    print(json.dumps({"lens": "DoubleGauss (0, 0.7) 0.5876 um", "num_rays": num_rays,
                      "image_size": size, "image_points": image[0].numel(),
                      "pupil_points": pupil[0].numel(), "terms": terms,
                      "ms_per_psf_sum": ms_op, "terms_per_s": terms / (ms_op * 1e-3),
                      "ms_per_huygens_psf_construction": ms_total,
                      "eager_torch_ms": ms_eager, "eager_over_kernel": ms_eager / ms_op,
                      "max_psf_diff_vs_eager": diff, "strehl": p.strehl_ratio()}))


if __name__ == "__main__":
    main()
