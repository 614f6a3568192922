"""Launch time of the scattering trace (measurement tooling, not product): the DoubleGauss
pupil trace of 2^20 rays, one field and wavelength. The timed callable is the C entry point
alone (outputs, segments and structs prepared once; a closed-form lens needs no Newton
schedule round), HIP events around N back-to-back calls on the current stream after warm-up,
repeated R times with the variants interleaved; min / median / max of the repeats are
reported, for

  * scatter_one:   a GaussianBSDF(sigma) on one surface (the stop's neighbour, traced
                   surface 5), trace_kernel<F_SCAT | F_GEN>;
  * scatter_all:   the same BSDF on every traced surface;
  * scatter_none:  the F_SCAT family on the lens's all-NONE table (the family's own cost
                   without a draw: every Newton kind compiled in, no fast pass);
  * closed:        the same lens without BSDFs through the closed-form kernel as shipped
                   (the flagship path, the unpolarized launch).

Reported: ms per launch, rays x surfaces per second (median) and the share of NaN rays of
the two scattering launches (rays that met total internal reflection after a scatter).

Prints one JSON line and, with --out FILE, writes it there. A run without a GPU fails.

    python tools/bsdf_rate.py [--log2-rays 20] [--steps 20] [--repeats 7] [--sigma 0.02] [--out profiles/bsdf_rate.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def _arg(name, default, kind=int):
    return kind(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


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
    import ctypes as C

    from optiland_pr_amd import _abi, _native, raytrace, scatter
    from optiland_pr_amd.lowering import pupil_scalars, segment_params
    from optiland_pr_amd.samples import DoubleGauss

    n = 1 << _arg("--log2-rays", 20)
    steps = _arg("--steps", 20)
    repeats = _arg("--repeats", 7)
    sigma = _arg("--sigma", 0.02, float)
    dev = raytrace.get_device()
    wl = 0.5876
    plain = DoubleGauss()
    one = DoubleGauss()
    one.surface_group.surfaces[5].interaction_model.bsdf = scatter.GaussianBSDF(sigma)
    every = DoubleGauss()
    for s in every.surface_group.surfaces[1:]:
        s.interaction_model.bsdf = scatter.GaussianBSDF(sigma)
    EPL, EPD = pupil_scalars(plain)
    segs = np.stack([segment_params(plain, 0.0, 0.7, 0, EPL, EPD)])
    rng = np.random.default_rng(0)
    r = np.sqrt(rng.random(n))
    th = 2 * np.pi * rng.random(n)
    px = torch.as_tensor(r * np.cos(th), device=dev)
    py = torch.as_tensor(r * np.sin(th), device=dev)
    dl = raytrace.lens_for(plain, [wl])
    dl_one = raytrace.lens_for(one, [wl])
    dl_all = raytrace.lens_for(every, [wl])
    assert dl_one.table.has_bsdf and dl_all.table.has_bsdf and not dl.table.has_bsdf
    n_surf = dl.table.n_surfaces
    lib = _native.load()
    out = raytrace.RealRays.empty(n, wl, device=dev)
    out_c = out.c_struct()
    seg_dev = raytrace.upload_segments(segs, dev)
    batch = _native.ort_batch(n, n, n, 1, 0, seg_dev.data_ptr())
    stream = raytrace._stream_handle()
    null = C.c_void_p(0)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    keep = []

    def scat(lens, st=null):  # (st: the status word, one memset more per call; untimed)
        sc, tab = scatter.scatter_struct(lens)
        keep.append(tab)
        opt = _native.ort_options(_abi.NEWTON_SCHEDULE, 0, None)

        def call():
            rc = lib.ort_trace_pupil_scatter(
                C.byref(lens.c), raytrace._ptr(px), raytrace._ptr(py), C.byref(out_c),
                C.byref(batch), C.byref(opt), null, null, st, C.byref(sc),
                stream)
            assert rc == 0, rc
        return call

    def base():
        opt = _native.ort_options(_abi.NEWTON_SCHEDULE, 0, None)

        def call():
            rc = lib.ort_trace_pupil(C.byref(dl.c), raytrace._ptr(px), raytrace._ptr(py),
                                     C.byref(out_c), C.byref(batch), C.byref(opt), null, null,
                                     null, stream)
            assert rc == 0, rc
        return call

    res = {"rays": n, "surfaces": n_surf, "steps": steps, "repeats": repeats, "sigma": sigma}
    fns = (("scatter_one", scat(dl_one)), ("scatter_all", scat(dl_all)),
           ("scatter_none", scat(dl)), ("closed", base()))
    # what the scattering launches leave behind
    for name, lens in (("scatter_one", dl_one), ("scatter_all", dl_all)):
        scat(lens, raytrace._ptr(status))()
        torch.cuda.synchronize()
        res[name + "_nan_share"] = float(torch.isnan(out.L).double().mean().item())
        res[name + "_status"] = int(status.item())
    samples = {name: [] for name, _ in fns}
    for _ in range(repeats):  # interleaved, so a drift hits every variant alike
        for name, fn in fns:
            samples[name].append(events_ms(fn, steps))
    for name, v in samples.items():
        v.sort()
        res[name + "_ms"] = {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}
        res[name + "_ray_surfaces_per_s"] = n * n_surf / (v[len(v) // 2] * 1e-3)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
