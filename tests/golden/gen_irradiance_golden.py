"""Incoherent-irradiance golden vectors: the REFERENCE's IncoherentIrradiance
(optiland/analysis/irradiance.py) on the Cooke triplet with a RectangularAperture on the
image surface, small resolutions and ray counts.

Test infrastructure only; it needs a checkout of the reference (no test imports it):

    PYTHONPATH=tests/golden/shims:<reference checkout> PYTHONDONTWRITEBYTECODE=1 \
        python tests/golden/gen_irradiance_golden.py

Writes tests/golden/irradiance.npz, arrays "<case>/<name>". Per case: the traced image
points in the global frame (gx, gy, gz) and in the detector's frame (x, y), their power, the
edges, pixel_area, the reference's map `irr`, `counts` (contributions per pixel, in the map's
orientation) and `spec` = [field Hx, Hy, wavelength, num_rays, res x, res y, px_size x, y
(0: none), aperture x_min, x_max, y_min, y_max]. CASES below names the distribution and the
lens of each case (tests/_irradiance.py builds the same ones from this package).

The last case runs the reference's torch backend with grad_mode enabled: its map is the
bilinear splat ([ny][nx]); `mask` is a fixed random image and grad_x / grad_y / grad_power are
torch autograd's gradients of sum(irr * mask) with respect to the localised x, y and power,
through the reference's own be.get_bilinear_weights and index_put(accumulate=True).
"""

from __future__ import annotations

import os
import sys

sys.dont_write_bytecode = True

import numpy as np  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))

import optiland.backend as be  # noqa: E402
from optiland.analysis.irradiance import IncoherentIrradiance  # noqa: E402
from optiland.physical_apertures import RectangularAperture  # noqa: E402
from optiland.rays import RealRays  # noqa: E402
from optiland.samples.objectives import CookeTriplet  # noqa: E402
from optiland.visualization.system.utils import transform  # noqa: E402

APERTURE = (-0.005, 0.006, -0.0045, 0.0055)  # mm: cuts the on-axis spot, some rays fall outside

# name -> (distribution, num_rays, res, px_size, wavelength, kind)
CASES = {
    "res_8x6": ("uniform", 24, (8, 6), None, 0.55, "plain"),
    "res_5x5": ("hexapolar", 8, (5, 5), None, 0.4861, "plain"),
    "px_size": ("uniform", 20, (3, 3), (0.002, 0.0025), 0.55, "plain"),
    "user_rays": ("uniform", 0, (6, 7), None, 0.55, "user"),
    "apodised": ("uniform", 24, (8, 6), None, 0.55, "apodised"),
    "grad_mode": ("hexapolar", 7, (6, 5), None, 0.55, "grad"),
}


def user_rays_arrays():
    """A 17 x 15 bundle parallel to the axis in front of the first surface, with a power that
    varies over it (a few rays carry none)."""
    gx, gy = np.meshgrid(np.linspace(-7.0, 7.0, 17), np.linspace(-6.0, 6.5, 15))
    x, y = gx.reshape(-1), gy.reshape(-1)
    power = 1.0 + 0.3 * np.sin(1.7 * x) * np.cos(0.9 * y)
    power[::23] = 0.0
    return x, y, power


def build(kind):
    lens = CookeTriplet()
    lens.surface_group.surfaces[-1].aperture = RectangularAperture(*APERTURE)
    if kind == "apodised":
        lens.set_apodization("GaussianApodization", sigma=0.6)
    return lens


def traced(lens, kind, dist, num_rays, wl):
    if kind == "user":
        x, y, p = user_rays_arrays()
        z = np.full_like(x, -5.0)
        rays = RealRays(x, y, z, np.zeros_like(x), np.zeros_like(x), np.ones_like(x), p,
                        np.full_like(x, wl))
        lens.surface_group.trace(rays)
        return rays
    return lens.trace(0.0, 0.0, wl, num_rays, dist)


def counts_of(x, y, p, xe, ye):
    keep = p > 0.0
    return np.histogram2d(x[keep], y[keep], bins=[xe, ye])[0]


def main():
    arrays = {}
    for key, (dist, num_rays, res, px, wl, kind) in CASES.items():
        grad = kind == "grad"
        be.set_backend("torch" if grad else "numpy")
        if grad:
            be.set_precision("float64")
            be.grad_mode.enable()
        lens = build(kind)
        kw = {}
        if kind == "user":
            x0, y0, p0 = user_rays_arrays()
            kw["user_initial_rays"] = RealRays(
                x0, y0, np.full_like(x0, -5.0), np.zeros_like(x0), np.zeros_like(x0),
                np.ones_like(x0), p0, np.full_like(x0, wl))
        a = IncoherentIrradiance(lens, num_rays=num_rays, res=res, px_size=px,
                                 fields=[(0.0, 0.0)], wavelengths=[wl], distribution=dist, **kw)
        irr, xe, ye = a.data[0][0]
        rays = traced(lens, kind, dist, num_rays, wl)
        surf = lens.surface_group.surfaces[-1]
        xl, yl, _ = transform(rays.x, rays.y, rays.z, surf, is_global=True)
        g = [np.asarray(be.to_numpy(v), dtype=np.float64) for v in (rays.x, rays.y, rays.z)]
        x, y, p = (np.asarray(be.to_numpy(v), dtype=np.float64) for v in (xl, yl, rays.i))
        area = (px[0] * px[1]) if px else (xe[1] - xe[0]) * (ye[1] - ye[0])
        irr = np.asarray(be.to_numpy(irr), dtype=np.float64)
        out = dict(gx=g[0], gy=g[1], gz=g[2], x=x, y=y, power=p, x_edges=xe, y_edges=ye,
                   pixel_area=area, irr=irr,
                   spec=[0.0, 0.0, wl, num_rays, a.npix_x, a.npix_y, *(px or (0.0, 0.0)),
                         *APERTURE])
        if grad:
            import torch

            tx, ty, tp = (torch.tensor(v, dtype=torch.float64, requires_grad=True)
                          for v in (x, y, p))
            idx, w = be.get_bilinear_weights(torch.stack([tx, ty], dim=1),
                                             (torch.tensor(xe), torch.tensor(ye)))
            pm = torch.zeros((a.npix_y, a.npix_x), dtype=torch.float64)
            cnt = torch.zeros((a.npix_y, a.npix_x), dtype=torch.float64)
            for i in range(4):
                at = (idx[:, i, 1].long(), idx[:, i, 0].long())
                pm = pm.index_put(at, w[:, i] * tp, accumulate=True)
                cnt = cnt.index_put(at, torch.ones_like(tp), accumulate=True)
            again = pm / area
            assert np.array_equal(again.detach().numpy(), irr), key
            mask = np.random.default_rng(7).uniform(-1.0, 1.0, irr.shape)
            (again * torch.tensor(mask)).sum().backward()
            out.update(mask=mask, grad_x=tx.grad.numpy(), grad_y=ty.grad.numpy(),
                       grad_power=tp.grad.numpy(), counts=cnt.numpy())
            be.grad_mode.disable()
        else:
            out["counts"] = counts_of(x, y, p, xe, ye)
            again = np.histogram2d(x[p > 0], y[p > 0], bins=[xe, ye], weights=p[p > 0])[0] / area
            assert np.array_equal(again, irr), key
        for name, v in out.items():
            arrays[f"{key}/{name}"] = np.asarray(v, dtype=np.float64)
        print(f"{key}: {x.size} rays, map {irr.shape}, {int(out['counts'].sum())} "
              f"contributions, {int((p > 0).sum())} with power, peak {irr.max():.6g}")
    be.set_backend("numpy")
    np.savez_compressed(os.path.join(HERE, "irradiance.npz"), **arrays)


if __name__ == "__main__":
    main()
