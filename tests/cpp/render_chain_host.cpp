// render_chain_host — the two per-Gaussian chains of the render backward built for the host: preprocess_backward_one
// (spz_preprocess_backward_core.hpp) and view_backward_one (spz_view_backward_core.hpp), the functions the device
// kernels call, run over every Gaussian of a scene that tests/test_render_frustum_host.py wrote.  CPU only; no HIP
// call is made.
//
// In:  int32 n, sh_degree, antialiased, has_depth; spz_amd_render_params; float32 positions[3n], scales[3n],
//      rotations[4n], alphas[n], colors[3n], sh[3 n dim]; spz_amd_render_record[n]; float32 record_grads[9n];
//      float32 depth_grads[n] when has_depth.
// Out: float32 positions[3n], scales[3n], rotations[4n], alphas[n], colors[3n], sh[3 n dim] (the six gradients, each
//      filled with NaN before the run, so an element the chain does not write shows); float64 view[12n] (each
//      Gaussian's 12 contributions to [R | t]).
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../spz_amd/csrc/spz_preprocess_backward_core.hpp"
#include "../../spz_amd/csrc/spz_view_backward_core.hpp"

using namespace spz_amd_detail;

template <typename T>
static std::vector<T> take(FILE *f, size_t count) {
  std::vector<T> v(count);
  if (count && std::fread(v.data(), sizeof(T), count, f) != count) {
    std::fprintf(stderr, "render_chain_host: short file\n");
    std::exit(2);
  }
  return v;
}

template <typename T>
static void put(FILE *f, const std::vector<T> &v) {
  if (!v.empty() && std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) {
    std::fprintf(stderr, "render_chain_host: cannot write\n");
    std::exit(2);
  }
}

int main(int argc, char **argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: render_chain_host scene.bin out.bin\n");
    return 2;
  }
  FILE *f = std::fopen(argv[1], "rb");
  if (f == nullptr) {
    std::fprintf(stderr, "render_chain_host: cannot open %s\n", argv[1]);
    return 2;
  }
  const std::vector<int32_t> head = take<int32_t>(f, 4);
  const size_t n = (size_t)head[0];
  const int deg = head[1], aa = head[2], has_depth = head[3];
  const std::vector<spz_amd_render_params> params = take<spz_amd_render_params>(f, 1);
  const int dim = sh_dim_for_degree(deg);
  if (dim < 0 || check_params(&params[0]) != SPZ_AMD_OK) {
    std::fprintf(stderr, "render_chain_host: bad scene\n");
    return 2;
  }
  const std::vector<float> positions = take<float>(f, 3 * n), scales = take<float>(f, 3 * n),
                           rotations = take<float>(f, 4 * n), alphas = take<float>(f, n), colors = take<float>(f, 3 * n),
                           sh = take<float>(f, 3 * n * (size_t)dim);
  const std::vector<spz_amd_render_record> rec = take<spz_amd_render_record>(f, n);
  const std::vector<float> rec_grad = take<float>(f, 9 * n);
  const std::vector<float> depth_grad = take<float>(f, has_depth ? n : 0);
  std::fclose(f);
  const unsigned long long total = 0;
  const float nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<float> g_positions(3 * n, nan), g_scales(3 * n, nan), g_rotations(4 * n, nan), g_alphas(n, nan),
      g_colors(3 * n, nan), g_sh(3 * n * (size_t)dim, nan);
  const FloatSrc src = {positions.data(), scales.data(), rotations.data(), alphas.data(), colors.data(), sh.data(),
                        (uint32_t)dim};
  PreprocessBackwardParams p = {};
  p.src = src;
  p.cam = make_cam(&params[0], deg, aa);
  p.rec = rec.data();
  p.rec_grad = rec_grad.data();
  p.total = &total;
  p.positions = g_positions.data();
  p.scales = g_scales.data();
  p.rotations = g_rotations.data();
  p.alphas = g_alphas.data();
  p.colors = g_colors.data();
  p.sh = g_sh.data();
  p.n = (uint32_t)n;
  p.depth_grad = has_depth ? depth_grad.data() : nullptr;
  ViewBackwardParams v = {};
  v.src = src;
  v.cam = p.cam;
  v.rec = rec.data();
  v.rec_grad = rec_grad.data();
  v.total = &total;
  v.n = (uint32_t)n;
  std::vector<double> view(kViewGrads * n);
  for (uint32_t i = 0; i < p.n; ++i) {
    preprocess_backward_one(p, i);
    view_backward_one(v, i, view.data() + (size_t)i * kViewGrads);
  }
  FILE *o = std::fopen(argv[2], "wb");
  if (o == nullptr) {
    std::fprintf(stderr, "render_chain_host: cannot open %s\n", argv[2]);
    return 2;
  }
  put(o, g_positions);
  put(o, g_scales);
  put(o, g_rotations);
  put(o, g_alphas);
  put(o, g_colors);
  put(o, g_sh);
  put(o, view);
  return std::fclose(o) == 0 ? 0 : 2;
}
