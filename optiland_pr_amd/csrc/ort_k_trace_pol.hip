// ort_k_trace_pol.hip -- trace kernels for coated / polarized lenses (F_POL: the 3x3
// complex polarization matrix per ray and the coatings' Jones factors, ort_polar.h; every
// Newton kind compiled in, 4 specialisations: generated or resident rays, with or without
// per-surface records)
// (kernel templates: ort_kernels.h; compiled as its own translation unit)

#include "ort_kernels.h"

namespace ortk {

KernelFn select_trace_pol(uint32_t feat) {
  constexpr uint32_t kAll = 15u;  // every Newton kind
  switch (feat & (F_GEN | F_REC)) {
#define ORT_C(F) \
  case (F):      \
    return trace_kernel<F_POL | kAll | (F)>;
    ORT_C(0) ORT_C(F_GEN) ORT_C(F_REC) ORT_C(F_GEN | F_REC)
#undef ORT_C
    default:
      return nullptr;
  }
}

}  // namespace ortk
