// Host build of the per-ray dispersion (csrc/ort_material.h: the functions every F_WRAY
// kernel, material_nk_kernel and ort_host.cpp call) for tests/test_dispersion_cpu.py,
// compiled with g++ -ffp-contract=off as the host library is.
//   stdin:  int64 n_coef_total, n_w; ort_material (offsets into coef); double coef[], w[]
//   stdout: double n[n_w], k[n_w]
#define ORT_HD
#include <cstdio>
#include <vector>

#include "../../optiland_pr_amd/csrc/ort_material.h"

int main() {
  int64_t head[2];
  ort_material m;
  if (fread(head, sizeof head, 1, stdin) != 1 || fread(&m, sizeof m, 1, stdin) != 1) return 2;
  if (head[0] < 0 || head[1] < 0) return 2;
  std::vector<double> coef(head[0]), w(head[1]), out(2 * head[1]);
  if (head[0] && fread(coef.data(), sizeof(double), coef.size(), stdin) != coef.size()) return 2;
  if (head[1] && fread(w.data(), sizeof(double), w.size(), stdin) != w.size()) return 2;
  // the record must stay inside coef: the kernels trust the host's lowering for this
  const int64_t n_len = m.kind == ORT_MAT_TABULATED ? 2 * (int64_t)m.n_coef : m.n_coef;
  if (m.coef_off < 0 || m.coef_off + n_len > head[0]) return 3;
  if (m.k_len > 0 && (m.k_off < 0 || m.k_off + 2 * (int64_t)m.k_len > head[0])) return 3;
  const double* c = coef.data();
  for (int64_t i = 0; i < head[1]; ++i) {
    out[i] = ort::material_n(m, c, w[i]);
    out[head[1] + i] = ort::material_k(m, c, w[i]);
  }
  fwrite(out.data(), sizeof(double), out.size(), stdout);
  return 0;
}
