"""optiland_pr_amd -- MI355X-native sequential real-ray trace core for Optiland.

The hot path of Optiland (PriUVBio/optiland_Pr) -- SurfaceGroup.trace and the ray
construction feeding it -- re-built as fused fp64 HIP kernels for gfx950, behind the
C ABI in include/optiland_rt.h, with a host-side mirror of the reference's Optic /
SurfaceGroup / RealRays / SpotDiagram / Wavefront interface.
"""

from . import _abi
from . import ops  # noqa: F401  (registers torch.ops.ort.trace_sequential / trace_pupil / huygens_psf /
# dft_psf / sampled_otf / irradiance_bin)
from .distribution import create_distribution
from .irradiance import IncoherentIrradiance
from .materials import IdealMaterial, Material
from .analysis import ZernikeOPD
from .mtf import FFTMTF, SampledMTF
from .optic import Optic
from .psf import FFTPSF, MMDFTPSF, HuygensPSF
from .through_focus import ThroughFocusMTF
from .zernike import ZernikeFit, ZernikeFringe, ZernikeNoll, ZernikeStandard

__all__ = ["Optic", "IdealMaterial", "Material", "HuygensPSF", "FFTPSF", "MMDFTPSF", "FFTMTF",
           "IncoherentIrradiance", "SampledMTF", "ThroughFocusMTF", "ZernikeOPD", "ZernikeFit",
           "ZernikeStandard", "ZernikeFringe", "ZernikeNoll",
           "create_distribution", "_abi"]
__version__ = "0.1.0"
