// view_grad_check — the one-Gaussian chain of the view backward (spz_view_backward_core.hpp) built for the host, for a
// run under AddressSanitizer + UBSan (`make view-grad-check`; CPU only).  Reads the scene tools/view_grad_check.py
// wrote, runs view_backward_one over every Gaussian and prints the 12 sums (index order) and the 12 sums of absolute
// contributions, which the script compares with tests/view_grad_ref.py.
//
// File: int32 n, sh_degree, antialiased, reserved; spz_amd_render_params; float32 positions[3n], scales[3n],
// rotations[4n], alphas[n], colors[3n], sh[3 n dim]; spz_amd_render_record[n]; float32 record_grads[9n].
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../spz_amd/csrc/spz_view_backward_core.hpp"

using namespace spz_amd_detail;

template <typename T>
static std::vector<T> take(FILE *f, size_t count) {
  std::vector<T> v(count);
  if (count && std::fread(v.data(), sizeof(T), count, f) != count) {
    std::fprintf(stderr, "view_grad_check: short file\n");
    std::exit(2);
  }
  return v;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: view_grad_check scene.bin\n");
    return 2;
  }
  FILE *f = std::fopen(argv[1], "rb");
  if (f == nullptr) {
    std::fprintf(stderr, "view_grad_check: cannot open %s\n", argv[1]);
    return 2;
  }
  const std::vector<int32_t> head = take<int32_t>(f, 4);
  const size_t n = (size_t)head[0];
  const int deg = head[1], aa = head[2];
  const std::vector<spz_amd_render_params> params = take<spz_amd_render_params>(f, 1);
  const int dim = sh_dim_for_degree(deg);
  if (dim < 0 || check_params(&params[0]) != SPZ_AMD_OK) {
    std::fprintf(stderr, "view_grad_check: bad scene\n");
    return 2;
  }
  const std::vector<float> positions = take<float>(f, 3 * n), scales = take<float>(f, 3 * n),
                           rotations = take<float>(f, 4 * n), alphas = take<float>(f, n), colors = take<float>(f, 3 * n),
                           sh = take<float>(f, 3 * n * (size_t)dim);
  const std::vector<spz_amd_render_record> rec = take<spz_amd_render_record>(f, n);
  const std::vector<float> rec_grad = take<float>(f, 9 * n);
  std::fclose(f);
  const unsigned long long total = 0;
  ViewBackwardParams p = {};
  p.src = FloatSrc{positions.data(), scales.data(), rotations.data(), alphas.data(), colors.data(), sh.data(), (uint32_t)dim};
  p.cam = make_cam(&params[0], deg, aa);
  p.rec = rec.data();
  p.rec_grad = rec_grad.data();
  p.total = &total;
  p.n = (uint32_t)n;
  double sum[kViewGrads] = {}, mag[kViewGrads] = {};
  for (uint32_t i = 0; i < p.n; ++i) {
    double c[kViewGrads];
    view_backward_one(p, i, c);
    for (uint32_t e = 0; e < kViewGrads; ++e) {
      sum[e] += c[e];
      mag[e] += c[e] < 0.0 ? -c[e] : c[e];
    }
  }
  for (uint32_t e = 0; e < kViewGrads; ++e) std::printf("%.17g %.17g\n", sum[e], mag[e]);
  return 0;
}
