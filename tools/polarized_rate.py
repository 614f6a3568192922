"""Launch time of the polarized trace (measurement tooling, not product): the DoubleGauss
pupil trace of 2^20 rays, one field and wavelength. The timed callable is the C entry point
alone (outputs, segments and structs prepared once; a closed-form lens needs no Newton
schedule round), HIP events around N back-to-back calls on the current stream after warm-up,
repeated R times with the variants interleaved; min / median / max of the repeats are
reported, for

  * polarized:      Fresnel coatings on every surface, unpolarized light, p_out NULL;
  * polarized_p:    the same with the [18][n] planes of P written;
  * closed_exact:   the same lens without coatings with ORT_OPT_EXACT: the closed-form
                    kernel re-tracing every lane on the exact sequences (a lens without
                    Newton surfaces never reaches the generic trace_kernel family, so this
                    is the nearest unpolarized launch with the exact per-operation math);
  * closed:         the same through the closed-form kernel as shipped (the flagship path).

Reported: ms per launch, rays x surfaces per second of the polarized launch (median), and
the extra time of p_out with the bytes per ray it would be at the peak bandwidth, against
the algorithmic 144 B (18 doubles). That is a time difference, not a byte counter.

Prints one JSON line and, with --out FILE, writes it there. A run without a GPU fails.

    python tools/polarized_rate.py [--log2-rays 20] [--steps 20] [--repeats 7] [--out profiles/polarized_rate.json]
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X peak HBM3E bandwidth


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

    from optiland_pr_amd import _abi, _native, polarization as pz, raytrace
    from optiland_pr_amd.lowering import pupil_scalars, segment_params
    from optiland_pr_amd.samples import DoubleGauss

    n = 1 << _arg("--log2-rays", 20)
    steps = _arg("--steps", 20)
    repeats = _arg("--repeats", 7)
    dev = raytrace.get_device()
    wl = 0.5876
    plain = DoubleGauss()
    coated = DoubleGauss()
    coated.surface_group.set_fresnel_coatings()
    EPL, EPD = pupil_scalars(plain)
    segs = np.stack([segment_params(plain, 0.0, 0.7, 0, EPL, EPD)])
    rng = np.random.default_rng(0)
    r = np.sqrt(rng.random(n))
    th = 2 * np.pi * rng.random(n)
    px = torch.as_tensor(r * np.cos(th), device=dev)
    py = torch.as_tensor(r * np.sin(th), device=dev)
    dl_pol = raytrace.lens_for(coated, [wl], polarized=True)
    dl = raytrace.lens_for(plain, [wl])
    n_surf = dl.table.n_surfaces
    # everything preallocated; the timed callable is the C entry point alone (a closed-form
    # lens has no Newton schedule, so one call is one launch)
    lib = _native.load()
    out = raytrace.RealRays.empty(n, wl, device=dev)
    out_c = out.c_struct()
    planes = torch.empty(18 * n, dtype=torch.float64, device=dev)
    seg_dev = raytrace.upload_segments(segs, dev)
    batch = _native.ort_batch(n, n, n, 1, 0, seg_dev.data_ptr())
    coat = pz._coatings_of(dl_pol)
    stream = raytrace._stream_handle()
    null = C.c_void_p(0)

    def pol(want_p):
        ps = pz.polarization_struct(_abi.POL_UNPOLARIZED, None, coat.data_ptr(),
                                    planes.data_ptr() if want_p else None)
        opt = _native.ort_options(_abi.NEWTON_SCHEDULE, 0, None)

        def call():
            rc = lib.ort_trace_pupil_polarized(
                C.byref(dl_pol.c), raytrace._ptr(px), raytrace._ptr(py), C.byref(out_c),
                C.byref(batch), C.byref(opt), null, null, null, C.byref(ps), stream)
            assert rc == 0, rc
        return call

    def base(exact):
        opt = _native.ort_options(_abi.NEWTON_SCHEDULE, 0, None)
        if exact:
            opt.flags |= _abi.OPT_EXACT

        def call():
            rc = lib.ort_trace_pupil(C.byref(dl.c), raytrace._ptr(px), raytrace._ptr(py),
                                     C.byref(out_c), C.byref(batch), C.byref(opt), null, null,
                                     null, stream)
            assert rc == 0, rc
        return call

    res = {"rays": n, "surfaces": n_surf, "steps": steps, "repeats": repeats}
    fns = (("polarized", pol(False)), ("polarized_p", pol(True)),
           ("closed_exact", base(True)), ("closed", base(False)))
    samples = {name: [] for name, _ in fns}
    for _ in range(repeats):  # interleaved, so a drift hits every variant alike
        for name, fn in fns:
            samples[name].append(events_ms(fn, steps))
    for name, v in samples.items():
        v.sort()
        res[name + "_ms"] = {"min": v[0], "median": v[len(v) // 2], "max": v[-1]}
    med = {k: res[k + "_ms"]["median"] for k in samples}
    res["polarized_ray_surfaces_per_s"] = n * n_surf / (med["polarized"] * 1e-3)
    extra_s = (med["polarized_p"] - med["polarized"]) * 1e-3
    res["p_out_extra_us"] = extra_s * 1e6
    res["p_out_bytes_per_ray_at_peak_bw"] = extra_s * HBM_BYTES_PER_S / n
    res["p_out_bytes_per_ray_algorithmic"] = 144
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
