"""Throughput of the FFT / MMDFT PSF transform (measurement tooling, not product):
torch.ops.ort.dft_psf (both launches) against the same transform in eager torch on the same
GPU, on seeded circular pupils with a few waves of OPD, at

  * (n, m) = (64, 256)     the default FFTPSF (num_rays=128 -> 64 rays, grid 256);
  * (n, m) = (128, 1024)   the reference documentation's explicit size;
  * B = 3 of the latter    the fields of an FFTMTF in one call.

Eager counterparts, each including everything it needs from the real amp / opd grids:
  matmul   complex128 L @ (g @ R): building g = amp exp(-2 pi i opd), the twiddle matrices
           L, R = exp(-2 pi i outer / pad) (psf/mmdft.py:273-289) and |.|^2;
  fft2     (integer pad) |fft2 of the zero-padded complex pupil|^2 (psf/fft.py:199-234; the
           fftshift only permutes pixels and is left out).

One fresh process. Every figure is the median of 7 windows, each `--steps` calls between two
device events after warm-up. Prints one JSON line per size; a run without a GPU fails (a CPU
time says nothing about the MI355X).

    python tools/dft_psf_rate.py [--steps 20]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

FP64_PEAK_FLOPS = 78.6e12  # MI355X fp64 vector peak (AMD's published figure)
SIZES = ((1, 64, 256), (1, 128, 1024), (3, 128, 1024))


def _arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def pupil(batch, n, dev):
    g = torch.Generator().manual_seed(1000 * n + batch)
    x = torch.linspace(-1, 1, n, dtype=torch.float64)
    inside = (x[None, :] ** 2 + x[:, None] ** 2) <= 1
    amp = (0.5 + 0.5 * torch.rand(batch, n, n, generator=g, dtype=torch.float64)) * inside
    opd = 6.0 * torch.rand(batch, n, n, generator=g, dtype=torch.float64) - 3.0
    return amp.to(dev).contiguous(), opd.to(dev).contiguous()


def eager_matmul(amp, opd, m, pad):
    n = amp.shape[-1]
    g = amp * torch.exp(-2j * torch.pi * opd)
    pc = torch.arange(n, device=amp.device, dtype=torch.float64) - n // 2
    ic = torch.arange(m, device=amp.device, dtype=torch.float64) - m // 2
    right = torch.exp(-2j * torch.pi * torch.outer(pc, ic) / pad)
    left = torch.exp(-2j * torch.pi * torch.outer(ic, pc) / pad)
    field = left @ (g @ right)
    return field.real ** 2 + field.imag ** 2


def eager_fft2(amp, opd, m):
    n = amp.shape[-1]
    before = (m - n) // 2
    after = before + (m - n) % 2
    g = amp * torch.exp(-2j * torch.pi * opd)
    field = torch.fft.fft2(torch.nn.functional.pad(g, (before, after, before, after)))
    return field.real ** 2 + field.imag ** 2


def median_ms(fn, steps, windows=7, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return statistics.median(out)


def main():
    import optiland_pr_amd  # noqa: F401  (registers the op)

    if not torch.cuda.is_available():
        raise SystemExit("dft_psf_rate: needs the MI355X")
    dev = torch.device("cuda")
    steps = _arg("--steps", 20)
    for batch, n, m in SIZES:
        amp, opd = pupil(batch, n, dev)
        pad = float(m)
        ms_op = median_ms(lambda: torch.ops.ort.dft_psf(amp, opd, m, pad), steps)
        ms_mm = median_ms(lambda: eager_matmul(amp, opd, m, pad), steps)
        ms_fft = median_ms(lambda: eager_fft2(amp, opd, m), steps)
        ours = torch.ops.ort.dft_psf(amp, opd, m, pad)
        scale = 100.0 / amp.sum(dim=(-2, -1), keepdim=True) ** 2  # ideal peak 100
        diff_mm = float(torch.max(torch.abs(ours - eager_matmul(amp, opd, m, pad)) * scale))
        shifted = torch.fft.fftshift(eager_fft2(amp, opd, m), dim=(-2, -1))
        diff_fft = float(torch.max(torch.abs(ours - shifted) * scale))
        flops = 8.0 * batch * (n * n * m + n * m * m)
        print(json.dumps({
            "batch": batch, "n": n, "m": m, "pad": pad, "steps": steps,
            "dft_psf_ms": ms_op, "eager_matmul_ms": ms_mm, "eager_fft2_ms": ms_fft,
            "eager_matmul_over_kernel": ms_mm / ms_op, "eager_fft2_over_kernel": ms_fft / ms_op,
            "flops": flops, "kernel_tflops": flops / (ms_op * 1e-3) / 1e12,
            "fp64_peak_tflops": FP64_PEAK_FLOPS / 1e12,
            "arithmetic_bound_ms": flops / FP64_PEAK_FLOPS * 1e3,
            "fraction_of_fp64_peak": flops / (ms_op * 1e-3) / FP64_PEAK_FLOPS,
            "max_psf_diff_vs_eager_matmul": diff_mm, "max_psf_diff_vs_eager_fft2": diff_fft}),
            flush=True)


if __name__ == "__main__":
    main()
