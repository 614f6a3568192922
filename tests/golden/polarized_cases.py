"""The polarized / coated golden cases, written against the lens-building API that the
reference and this package share (Optic.add_surface / set_aperture / add_field /
add_wavelength / set_polarization / set_apodization, surface_group.set_fresnel_coatings).

`build(case, ns)` builds one case's lens from the classes in the namespace `ns`:
CookeTriplet, Optic, IdealMaterial, FresnelCoating, SimpleCoating, GaussianApodization,
RadialAperture. gen_polarized_golden.py passes the reference's, tests/_polarized.py this
package's. This module imports neither.

CASES[name] = dict(lens=..., traces=[(tag, kind, args)], states=[...]):
  kind "trace":   Optic.trace(Hx, Hy, wavelength, num_rays, "hexapolar")
  kind "generic": Optic.trace_generic(Hx, Hy, Px, Py, wavelength)
A state is a create_polarization name or "ignore".
"""

WL = 0.55
ALL_STATES = ("unpolarized", "H", "V", "L+45", "L-45", "RCP", "LCP")

CASES = {
    # 1: partial block; the on-axis chief ray takes the exact mag == 0 fallback everywhere
    "cooke_fresnel": dict(lens="cooke_fresnel", states=ALL_STATES,
                          traces=[("f1", "trace", (0.0, 1.0, WL, 6)),
                                  ("f0", "trace", (0.0, 0.0, WL, 6))]),
    # 2: two blocks, ragged tail
    "cooke_fresnel_271": dict(lens="cooke_fresnel", states=("unpolarized", "RCP"),
                              traces=[("f07", "trace", (0.0, 0.7, WL, 9))]),
    # 3: no coating: P is a product of rotations
    "cooke_uncoated": dict(lens="cooke", states=("H", "unpolarized"),
                           traces=[("f1", "trace", (0.0, 1.0, WL, 6))]),
    # 4: the reflect branch, a coating whose materials are not the surface's own
    "mirror": dict(lens="mirror", states=("unpolarized", "L+45"),
                   traces=[("f1", "trace", (0.0, 1.0, WL, 6))]),
    # 5: a slab under a steep field; the exit coating's own materials put sin^2 above n^2:
    #    the complex root of the Fresnel coefficients
    "slab": dict(lens="slab", states=("unpolarized", "V"),
                 traces=[("f1", "trace", (0.0, 1.0, WL, 6))]),
    # 6: the Newton path
    "asphere": dict(lens="asphere", states=("unpolarized",),
                    traces=[("f1", "trace", (0.0, 1.0, WL, 6))]),
    # 7: a SimpleCoating: "ignore" gives plain rays, a state skips that surface's update
    "cooke_simple": dict(lens="cooke_simple", states=("ignore", "H"),
                         traces=[("f1", "trace", (0.0, 1.0, WL, 6))]),
    # 8: clipping aperture + Gaussian apodization: the two intensity quirks
    "cooke_clip_apod": dict(lens="cooke_clip_apod", states=("H", "unpolarized"),
                            traces=[("f1", "trace", (0.0, 1.0, WL, 6))]),
    # 9: trace_generic: P present, the intensity not updated
    "generic": dict(lens="cooke_fresnel", states=("RCP",),
                    traces=[("g5", "generic", ([0.0, 0.0, 0.3, -0.5, 1.0],
                                               [0.0, 1.0, 0.7, 0.2, -1.0],
                                               [0.0, 0.2, -0.6, 0.9, 0.1],
                                               [0.0, -0.3, 0.5, 0.1, -0.8], WL))]),
}
NEWTON_CASES = ("asphere",)


def build(lens, ns):
    if lens == "cooke":
        return ns.CookeTriplet()
    if lens == "cooke_fresnel":
        o = ns.CookeTriplet()
        o.surface_group.set_fresnel_coatings()
        return o
    if lens == "cooke_simple":
        o = ns.CookeTriplet()
        o.surface_group.surfaces[2].interaction_model.coating = ns.SimpleCoating(0.9, 0.1)
        return o
    if lens == "cooke_clip_apod":
        o = ns.CookeTriplet()
        o.surface_group.set_fresnel_coatings()
        o.surface_group.surfaces[3].aperture = ns.RadialAperture(r_max=3.5)
        o.set_apodization(ns.GaussianApodization(sigma=0.8))
        return o
    o = ns.Optic()
    if lens == "mirror":
        o.add_surface(index=0, radius=float("inf"), thickness=float("inf"))
        o.add_surface(index=1, radius=-120.0, thickness=-55.0, material="mirror", is_stop=True)
        o.add_surface(index=2)
        # assigned after the surfaces are linked: the linking would replace it
        o.surface_group.surfaces[1].interaction_model.coating = ns.FresnelCoating(
            ns.IdealMaterial(1.0), ns.IdealMaterial(1.5))
        o.set_aperture(aperture_type="EPD", value=20.0)
        o.set_field_type(field_type="angle")
        o.add_field(y=0.0)
        o.add_field(y=3.0)
    elif lens == "slab":
        o.add_surface(index=0, radius=float("inf"), thickness=float("inf"))
        o.add_surface(index=1, radius=float("inf"), thickness=5.0,
                      material=ns.IdealMaterial(1.5), is_stop=True, coating="fresnel")
        o.add_surface(index=2, radius=float("inf"), thickness=10.0)
        o.add_surface(index=3)
        o.surface_group.surfaces[2].interaction_model.coating = ns.FresnelCoating(
            ns.IdealMaterial(2.5), ns.IdealMaterial(1.0))
        o.set_aperture(aperture_type="EPD", value=4.0)
        o.set_field_type(field_type="angle")
        o.add_field(y=0.0)
        o.add_field(y=40.0)
    elif lens == "asphere":
        o.add_surface(index=0, radius=float("inf"), thickness=float("inf"))
        o.add_surface(index=1, surface_type="even_asphere", radius=40.0, conic=-0.5,
                      thickness=6.0, material=ns.IdealMaterial(1.6), is_stop=True,
                      coefficients=[0.0, 2e-6, -3e-9], coating="fresnel")
        o.add_surface(index=2, radius=-70.0, thickness=45.0, coating="fresnel")
        o.add_surface(index=3)
        o.set_aperture(aperture_type="EPD", value=12.0)
        o.set_field_type(field_type="angle")
        o.add_field(y=0.0)
        o.add_field(y=6.0)
    else:
        raise KeyError(lens)
    o.add_wavelength(value=WL, is_primary=True)
    return o
