// spz_cli.cpp — the three command-line tools of the reference (cli_tools/src/*.cpp) over the
// MI355X drop-in layer: ply_to_spz, spz_to_ply, spz_info; and spz_filter (spz::filterSpz),
// spz_transform (spz::transformSpz), spz_merge (spz::mergeSpz), spz_sort (spz::sortSpz), spz_decimate
// (spz::decimateSpz), spz_tile (spz::tileSpz), spz_clean (spz::cleanSpz), spz_render (spz::renderSpz), spz_prune
// (spz::pruneSpz), spz_compare (spz::compareSpz), spz_align (spz::alignSpz), spz_level (spz::levelSpz),
// spz_refine (spz::refineSpz),
// spz_locate (spz::locateSpz) and spz_mesh (spz::meshSpz), which have no counterpart in the reference.  One binary,
// dispatched on argv[0] (the Makefile installs it under the seventeen names) or on a first argument naming the tool.
// spz_refine, spz_locate and spz_mesh exit 0 on success and 1 on a failure.
// spz_align exits 0 on success, 1 on a failure and 2 when the run ends degenerate; its --output is written by
// transformSpz, at --fractional-bits (12 unless given, as for spz_transform).
// spz_compare exits 0 on success, 1 on a failure and 2 when a view misses --min-psnr or --min-ssim.
// Same behaviour as the reference mains: default (UNSPECIFIED) pack/unpack options, exit code 0
// once the arguments are there (the reference ignores the save/load results), usage -> 1.
// spz_filter, spz_transform, spz_merge, spz_sort, spz_decimate, spz_clean, spz_render and spz_prune exit 1 when the
// filter / transform / merge / sort / decimation / clean / render / prune fails as well.
// Those eight read their arguments with one reader (Args): <input> <output> come first and may not start with '-'
// (spz_merge takes its inputs anywhere, and -o); each option may be given once; an integer is decimal digits only,
// leading zeros allowed, no sign or space, range-checked; a real is all of its argument, by strtof for a float field
// and strtod for a double field.  Anything else prints the tool's usage line.
#include <algorithm>
#include <stdexcept>
#include <array>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <iostream>
#include <iterator>
#include <set>
#include <string>
#include <vector>

#include "spz_amd_host.hpp"

namespace {

int plyToSpz(int argc, char **argv) {
  if (argc < 3) {
    std::cerr << "Usage: ply_to_spz <input.ply> <output.spz>" << std::endl;
    return 1;
  }
  spz::GaussianCloud splat = spz::loadSplatFromPly(argv[1], spz::UnpackOptions{});
  spz::saveSpz(splat, spz::PackOptions{}, std::string(argv[2]));
  return 0;
}

int spzToPly(int argc, char **argv) {
  if (argc < 3) {
    std::cerr << "Usage: spz_to_ply <input.spz> <output.ply>" << std::endl;
    return 1;
  }
  spz::GaussianCloud splat = spz::loadSpz(std::string(argv[1]), spz::UnpackOptions{});
  spz::saveSplatToPly(splat, spz::PackOptions{}, argv[2]);
  return 0;
}

int spzInfo(int argc, char **argv) {
  if (argc < 2) {
    std::cerr << "Usage: spz_info <input.spz>" << std::endl;
    return 1;
  }
  const spz::GaussianCloud cloud = spz::loadSpz(std::string(argv[1]), spz::UnpackOptions{});
  std::cout << "Number of points: " << cloud.positions.size() / 3 << std::endl;
  if (!cloud.positions.empty()) {
    float lo[3] = {cloud.positions[0], cloud.positions[1], cloud.positions[2]};
    float hi[3] = {lo[0], lo[1], lo[2]};
    for (size_t i = 0; i + 2 < cloud.positions.size(); i += 3) {
      for (int a = 0; a < 3; ++a) {
        lo[a] = std::min(lo[a], cloud.positions[i + a]);
        hi[a] = std::max(hi[a], cloud.positions[i + a]);
      }
    }
    std::cout << "Bounding box:" << std::endl;
    const char *axis = "XYZ";
    for (int a = 0; a < 3; ++a) std::cout << "  " << axis[a] << ": " << lo[a] << " to " << hi[a] << std::endl;
  }
  return 0;
}

// The --coord names: as the usage lines list them, and in spz::CoordinateSystem's order.
#define SPZ_COORD_NAMES "RUB|RDF|LUF|RUF|LDB|RDB|LUB|LDF|UNSPECIFIED"
const char *const kCoordNames[] = {"UNSPECIFIED", "LDB", "RDB", "LUB", "RUB", "LDF", "RDF", "LUF", "RUF"};

// One tool's arguments, read in the tool's own loop: next() steps to an argument, is() names it, and the value
// readers take the option's values after it.  A value reader returns false when fewer values are left than it needs or
// one is malformed; the tool then returns usage().
class Args {
 public:
  Args(int argc, char **argv, const char *usage) : argc_(argc), argv_(argv), usage_(usage) {}

  int usage() const {
    std::cerr << usage_ << std::endl;
    return 1;
  }
  // <input> <output> (spz_refine: three files): all there, none starting with '-'.  The options follow them.
  bool files(int count = 2) {
    at_ = count + 1;
    if (argc_ <= count) return false;
    for (int k = 1; k <= count; ++k) {
      if (argv_[k][0] == '-') return false;
    }
    return true;
  }
  bool next() {
    if (at_ >= argc_) return false;
    arg_ = argv_[at_++];
    repeat_ = !given_.insert(arg_).second;
    return true;
  }
  const char *arg() const { return arg_; }
  // Whether the argument is `option`, given for the first time: a repeated option is no option at all.
  bool is(const char *option) const { return !repeat_ && std::strcmp(arg_, option) == 0; }
  bool given(const char *option) const { return given_.count(option) != 0; }

  bool text(std::string *v) {
    char **s = values(1);
    if (s) *v = s[0];
    return s != nullptr;
  }
  bool coord(spz::CoordinateSystem *c) {
    std::string name;
    if (!text(&name)) return false;
    const auto *n = std::find(std::begin(kCoordNames), std::end(kCoordNames), name);
    if (n == std::end(kCoordNames)) return false;
    *c = static_cast<spz::CoordinateSystem>(n - std::begin(kCoordNames));
    return true;
  }
  template <class T>
  bool integer(T *v, uint64_t lo, uint64_t hi, int k = 1) {
    char **s = values(k);
    for (int j = 0; s && j < k; ++j) {
      const char *c = s[j];
      uint64_t x = 0;
      for (; *c >= '0' && *c <= '9' && x <= (UINT64_MAX - (*c - '0')) / 10; ++c) x = 10 * x + (*c - '0');
      if (c == s[j] || *c != '\0' || x < lo || x > hi) return false;
      v[j] = static_cast<T>(x);
    }
    return s != nullptr;
  }
  bool real(float *v, int k = 1) { return reals(v, k, std::strtof); }
  bool real(double *v, int k = 1) { return reals(v, k, std::strtod); }

 private:
  char **values(int k) {
    if (at_ + k > argc_) return nullptr;
    at_ += k;
    return argv_ + at_ - k;
  }
  template <class T>
  bool reals(T *v, int k, T (*convert)(const char *, char **)) {
    char **s = values(k);
    for (int j = 0; s && j < k; ++j) {
      char *end = nullptr;
      v[j] = convert(s[j], &end);
      if (end == s[j] || *end != '\0') return false;
    }
    return s != nullptr;
  }

  int argc_;
  char **argv_;
  const char *usage_;
  int at_ = 1;
  const char *arg_ = "";
  bool repeat_ = false;
  std::set<std::string> given_;
};

bool allFinite(const float *v, int k) {
  return std::all_of(v, v + k, [](float x) { return std::isfinite(x); });
}

const char *kFilterUsage =
    "Usage: spz_filter <input.spz> <output.spz> [--sh-degree D] [--min-alpha A] [--box x0 y0 z0 x1 y1 z1] "
    "[--coord " SPZ_COORD_NAMES "]";

int spzFilter(int argc, char **argv) {
  Args a(argc, argv, kFilterUsage);
  if (!a.files()) return a.usage();
  spz::FilterOptions f;
  while (a.next()) {
    bool good = false;
    if (a.is("--sh-degree")) good = a.integer(&f.shDegree, 0, 3);
    else if (a.is("--min-alpha")) good = a.real(&f.minAlpha.emplace());
    else if (a.is("--box")) good = a.real(f.box.emplace().lo.data(), 3) && a.real(f.box->hi.data(), 3);
    else if (a.is("--coord")) good = a.coord(&f.coord);
    if (!good) return a.usage();
  }
  int64_t kept = 0;
  if (!spz::filterSpz(std::string(argv[1]), std::string(argv[2]), f, &kept)) return 1;
  std::cout << "Points kept: " << kept << std::endl;
  return 0;
}

const char *kTransformUsage =
    "Usage: spz_transform <input.spz> <output.spz> [--rotate x y z w] [--translate x y z] [--scale s] "
    "[--coord " SPZ_COORD_NAMES "] [--fractional-bits n]";

int spzTransform(int argc, char **argv) {
  Args a(argc, argv, kTransformUsage);
  if (!a.files()) return a.usage();
  spz::TransformOptions o;
  while (a.next()) {
    bool good = false;
    if (a.is("--rotate")) good = a.real(o.rotation.data(), 4);
    else if (a.is("--translate")) good = a.real(o.translation.data(), 3);
    else if (a.is("--scale")) good = a.real(&o.scale);
    else if (a.is("--coord")) good = a.coord(&o.coord);
    else if (a.is("--fractional-bits")) good = a.integer(&o.fractionalBits, 0, 24);
    if (!good) return a.usage();
  }
  return spz::transformSpz(std::string(argv[1]), std::string(argv[2]), o) ? 0 : 1;
}

const char *kMergeUsage =
    "Usage: spz_merge <input.spz>... -o <output.spz> [--sh-degree D] [--fractional-bits B] [--antialiased 0|1]";

int spzMerge(int argc, char **argv) {
  Args a(argc, argv, kMergeUsage);
  spz::MergeOptions o;
  std::vector<std::string> inputs;
  std::string output;
  while (a.next()) {
    if (a.arg()[0] != '-') {
      inputs.push_back(a.arg());
      continue;
    }
    bool good = false;
    if (a.is("-o")) good = a.text(&output);
    else if (a.is("--sh-degree")) good = a.integer(&o.shDegree, 0, 3);
    else if (a.is("--fractional-bits")) good = a.integer(&o.fractionalBits, 0, 24);
    else if (a.is("--antialiased")) good = a.integer(&o.antialiased, 0, 1);
    if (!good) return a.usage();
  }
  if (inputs.empty() || output.empty()) return a.usage();
  return spz::mergeSpz(inputs, output, o) ? 0 : 1;
}

const char *kSortUsage = "Usage: spz_sort <input.spz> <output.spz> [--keys <keys.f32>] [--descending]";

int spzSort(int argc, char **argv) {
  Args a(argc, argv, kSortUsage);
  if (!a.files()) return a.usage();
  spz::SortOptions o;
  std::string keys;
  while (a.next()) {
    bool good = false;
    if (a.is("--keys")) good = a.text(&keys);
    else if (a.is("--descending")) good = o.descending = true;
    if (!good) return a.usage();
  }
  if (a.given("--keys")) {
    // raw little-endian float32, one per point
    std::ifstream f(keys, std::ios::binary | std::ios::ate);
    if (!f) {
      std::cerr << "[SPZ ERROR] spz_sort: unable to read " << keys << std::endl;
      return 1;
    }
    const std::streamoff bytes = f.tellg();
    if (bytes < 0 || bytes % 4 != 0) {
      std::cerr << "[SPZ ERROR] spz_sort: " << keys << " is not a whole number of float32 values" << std::endl;
      return 1;
    }
    std::vector<float> k(static_cast<size_t>(bytes / 4));
    f.seekg(0);
    if (!k.empty() && !f.read(reinterpret_cast<char *>(k.data()), bytes)) {
      std::cerr << "[SPZ ERROR] spz_sort: unable to read " << keys << std::endl;
      return 1;
    }
    o.keys = std::move(k);
  }
  return spz::sortSpz(std::string(argv[1]), std::string(argv[2]), o) ? 0 : 1;
}

const char *kDecimateUsage = "Usage: spz_decimate <input.spz> <output.spz> (--level <L> | --target <N>)";

int spzDecimate(int argc, char **argv) {
  Args a(argc, argv, kDecimateUsage);
  if (!a.files()) return a.usage();
  spz::DecimateOptions o;
  const uint64_t maxTarget = 9999999999999999999ull;  // the largest --target spz_decimate has taken
  while (a.next()) {
    bool good = false;
    if (a.is("--level")) good = a.integer(&o.level.emplace(), 0, 24);
    else if (a.is("--target")) good = a.integer(&o.targetPoints.emplace(), 1, maxTarget);
    if (!good) return a.usage();
  }
  if (o.level.has_value() == o.targetPoints.has_value()) return a.usage();
  return spz::decimateSpz(std::string(argv[1]), std::string(argv[2]), o) ? 0 : 1;
}

const char *kTileUsage =
    "Usage: spz_tile <input.spz> <outdir> --max-points <N> [--max-tiles <M>] [--coord " SPZ_COORD_NAMES "]";

int spzTile(int argc, char **argv) {
  Args a(argc, argv, kTileUsage);
  if (!a.files()) return a.usage();
  spz::TileOptions o;
  while (a.next()) {
    bool good = false;
    if (a.is("--max-points")) good = a.integer(&o.maxPoints, 1, 10000000);
    else if (a.is("--max-tiles")) good = a.integer(&o.maxTiles, 1, 2147483647);
    else if (a.is("--coord")) good = a.coord(&o.coord);
    if (!good) return a.usage();
  }
  if (!a.given("--max-points")) return a.usage();
  return spz::tileSpz(std::string(argv[1]), std::string(argv[2]), o) ? 0 : 1;
}

const char *kCleanUsage =
    "Usage: spz_clean <input.spz> <output.spz> [--k <K> [--std-ratio <S>]] [--radius <R> --min-neighbors <M>]";

int spzClean(int argc, char **argv) {
  Args a(argc, argv, kCleanUsage);
  if (!a.files()) return a.usage();
  spz::CleanOptions::Statistical st;
  spz::CleanOptions::Radius rd;
  while (a.next()) {
    bool good = false;
    if (a.is("--k")) good = a.integer(&st.k, 1, 64);
    else if (a.is("--std-ratio")) good = a.real(&st.stdRatio) && std::isfinite(st.stdRatio);
    else if (a.is("--radius")) good = a.real(&rd.radius) && std::isfinite(rd.radius) && rd.radius > 0.0;
    else if (a.is("--min-neighbors")) good = a.integer(&rd.minNeighbors, 1, 256);
    if (!good) return a.usage();
  }
  const bool hasK = a.given("--k"), hasRadius = a.given("--radius");
  if ((a.given("--std-ratio") && !hasK) || hasRadius != a.given("--min-neighbors") || (!hasK && !hasRadius)) {
    return a.usage();
  }
  spz::CleanOptions o;
  if (hasK) o.statistical = st;
  if (hasRadius) o.radius = rd;
  return spz::cleanSpz(std::string(argv[1]), std::string(argv[2]), o) ? 0 : 1;
}

const char *kRenderUsage =
    "Usage: spz_render <in.spz> <out.ppm|out.pfm> --size W H (--fov-y DEG | --intrinsics fx fy cx cy) --eye x y z "
    "--target x y z [--up x y z] [--coord " SPZ_COORD_NAMES "] [--background r g b] "
    "[--sh-degree D] [--near N] [--depth FILE.pfm [--depth-kind expected|median]] [--ids FILE.bin] [--pick X Y]...\n"
    "  --depth  the depth map as a one-channel PFM (rows bottom to top; +inf where there is none): expected = the blend's\n"
    "           depth sum over alpha, median = the depth at which the transmittance falls below 0.5\n"
    "  --ids    the median splat's index per pixel: raw little-endian uint32, rows top to bottom, 4294967295 for none\n"
    "  --pick   print `index depth` of the median splat at pixel X Y, or `none` (one line per --pick, in order)";

bool endsWith(const std::string &s, const char *suffix) {
  const size_t n = std::strlen(suffix);
  return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

// PPM: clamp to [0, 1], round(255 v), rows top to bottom.  PFM: float RGB, little-endian, rows bottom to top.
bool writeImage(const std::string &path, const std::vector<float> &rgba, int w, int h, bool pfm) {
  std::ofstream out(path, std::ios::binary);
  if (!out) return false;
  if (pfm) {
    out << "PF\n" << w << " " << h << "\n-1.0\n";
    std::vector<float> row(static_cast<size_t>(w) * 3);
    for (int y = h - 1; y >= 0; --y) {
      for (int x = 0; x < w; ++x) {
        for (int c = 0; c < 3; ++c) row[x * 3 + c] = rgba[(static_cast<size_t>(y) * w + x) * 4 + c];
      }
      out.write(reinterpret_cast<const char *>(row.data()), static_cast<std::streamsize>(row.size() * sizeof(float)));
    }
  } else {
    out << "P6\n" << w << " " << h << "\n255\n";
    std::vector<unsigned char> row(static_cast<size_t>(w) * 3);
    for (int y = 0; y < h; ++y) {
      for (int x = 0; x < w; ++x) {
        for (int c = 0; c < 3; ++c) {
          float v = rgba[(static_cast<size_t>(y) * w + x) * 4 + c];
          v = std::isnan(v) ? 0.0f : std::min(1.0f, std::max(0.0f, v));
          row[x * 3 + c] = static_cast<unsigned char>(std::lround(255.0f * v));
        }
      }
      out.write(reinterpret_cast<const char *>(row.data()), static_cast<std::streamsize>(row.size()));
    }
  }
  return static_cast<bool>(out);
}

// One-channel PFM ("Pf"): little-endian floats, rows bottom to top, non-finite values kept.
bool writeDepthPfm(const std::string &path, const std::vector<float> &depth, int w, int h) {
  std::ofstream out(path, std::ios::binary);
  if (!out) return false;
  out << "Pf\n" << w << " " << h << "\n-1.0\n";
  for (int y = h - 1; y >= 0; --y) {
    out.write(reinterpret_cast<const char *>(depth.data() + static_cast<size_t>(y) * w),
              static_cast<std::streamsize>(static_cast<size_t>(w) * sizeof(float)));
  }
  return static_cast<bool>(out);
}

bool writeIds(const std::string &path, const std::vector<uint32_t> &index) {
  std::ofstream out(path, std::ios::binary);
  if (!out) return false;
  out.write(reinterpret_cast<const char *>(index.data()), static_cast<std::streamsize>(index.size() * sizeof(uint32_t)));
  return static_cast<bool>(out);
}

int spzRender(int argc, char **argv) {
  Args a(argc, argv, kRenderUsage);
  if (!a.files()) return a.usage();
  const std::string outPath = argv[2];
  const bool pfm = endsWith(outPath, ".pfm");
  if (!pfm && !endsWith(outPath, ".ppm")) return a.usage();
  spz::RenderOptions o;
  int size[2] = {0, 0};
  float fovY = 0.0f, intr[4] = {0, 0, 0, 0};
  std::array<float, 3> eye{}, target{}, up{};
  std::string depthPath, depthKind = "expected", idsPath;
  std::vector<std::array<int, 2>> picks;
  while (a.next()) {
    bool good = false;
    if (std::strcmp(a.arg(), "--pick") == 0) {  // the one option that may be repeated
      picks.emplace_back();
      good = a.integer(picks.back().data(), 0, 16383, 2);
    } else if (a.is("--depth")) good = a.text(&depthPath) && endsWith(depthPath, ".pfm");
    else if (a.is("--depth-kind")) good = a.text(&depthKind) && (depthKind == "expected" || depthKind == "median");
    else if (a.is("--ids")) good = a.text(&idsPath) && !idsPath.empty();
    else if (a.is("--size")) good = a.integer(size, 1, 16384, 2);
    else if (a.is("--fov-y")) good = a.real(&fovY) && fovY > 0.0f && fovY < 180.0f;
    else if (a.is("--intrinsics")) good = a.real(intr, 4) && allFinite(intr, 4);
    else if (a.is("--eye")) good = a.real(eye.data(), 3) && allFinite(eye.data(), 3);
    else if (a.is("--target")) good = a.real(target.data(), 3) && allFinite(target.data(), 3);
    else if (a.is("--up")) good = a.real(up.data(), 3) && allFinite(up.data(), 3);
    else if (a.is("--background")) good = a.real(o.background.data(), 3) && allFinite(o.background.data(), 3);
    else if (a.is("--near")) good = a.real(&o.nearPlane) && std::isfinite(o.nearPlane) && o.nearPlane > 0.0f;
    else if (a.is("--sh-degree")) good = a.integer(&o.maxShDegree, 0, 3);
    else if (a.is("--coord")) good = a.coord(&o.coord);
    if (!good) return a.usage();
  }
  const bool hasFov = a.given("--fov-y");
  if (!a.given("--size") || hasFov == a.given("--intrinsics") || !a.given("--eye") || !a.given("--target")) {
    return a.usage();
  }
  o.width = size[0];
  o.height = size[1];
  if (a.given("--depth-kind") && !a.given("--depth")) return a.usage();
  for (const auto &px : picks) {
    if (px[0] >= o.width || px[1] >= o.height) return a.usage();
  }
  if (hasFov) {
    o.fy = static_cast<float>(0.5 * o.height / std::tan(0.5 * fovY * 3.14159265358979323846 / 180.0));
    o.fx = o.fy;
    o.cx = 0.5f * static_cast<float>(o.width);
    o.cy = 0.5f * static_cast<float>(o.height);
  } else {
    o.fx = intr[0];
    o.fy = intr[1];
    o.cx = intr[2];
    o.cy = intr[3];
    if (!(o.fx > 0.0f) || !(o.fy > 0.0f)) return a.usage();
  }
  if (!a.given("--up")) {  // the frame's U axis (UNSPECIFIED: the stored RUB frame)
    const int c = static_cast<int>(o.coord) == 0 ? 4 : static_cast<int>(o.coord);
    const bool yDown = (((c - 1) >> 1) & 1) == 0;  // LDB, RDB, LDF, RDF
    up = {0.0f, yDown ? -1.0f : 1.0f, 0.0f};
  }
  try {
    o.worldToCamera = spz::lookAt(eye, target, up);
  } catch (const std::invalid_argument &) {
    return a.usage();
  }
  std::vector<float> rgba;
  spz::DepthMaps maps;
  const bool wantDepth = a.given("--depth") || a.given("--ids") || !picks.empty();
  if (!(wantDepth ? spz::renderSpzDepth(std::string(argv[1]), o, &maps, &rgba) : spz::renderSpz(std::string(argv[1]), o, &rgba))) {
    return 1;
  }
  if (!writeImage(outPath, rgba, o.width, o.height, pfm)) {
    std::cerr << "spz_render: unable to write " << outPath << std::endl;
    return 1;
  }
  if (a.given("--depth") && !writeDepthPfm(depthPath, depthKind == "median" ? maps.median : maps.expected, o.width, o.height)) {
    std::cerr << "spz_render: unable to write " << depthPath << std::endl;
    return 1;
  }
  if (a.given("--ids") && !writeIds(idsPath, maps.index)) {
    std::cerr << "spz_render: unable to write " << idsPath << std::endl;
    return 1;
  }
  for (const auto &px : picks) {
    const size_t at = static_cast<size_t>(px[1]) * o.width + px[0];
    if (maps.index[at] == 0xffffffffu) {
      std::cout << "none" << std::endl;
    } else {
      char line[64];
      std::snprintf(line, sizeof line, "%u %.9g", maps.index[at], static_cast<double>(maps.median[at]));
      std::cout << line << std::endl;
    }
  }
  return 0;
}

// The view arguments spz_prune, spz_compare and spz_refine share: --views FILE, or --orbit N --size W H --fov-y DEG
// [--center x y z --radius R] [--distance K].
struct ViewArgs {
  std::string viewsFile;
  int orbit = 0, size[2] = {0, 0};
  float fovY = 0.0f, radius = 0.0f, distance = 2.5f;
  std::array<float, 3> center{};

  // Whether the current argument is one of these; *good: whether its values parsed.
  bool take(Args &a, bool *good) {
    if (a.is("--views")) *good = a.text(&viewsFile);
    else if (a.is("--orbit")) *good = a.integer(&orbit, 1, 1024);
    else if (a.is("--size")) *good = a.integer(size, 1, 16384, 2);
    else if (a.is("--fov-y")) *good = a.real(&fovY) && fovY > 0.0f && fovY < 180.0f;
    else if (a.is("--center")) *good = a.real(center.data(), 3) && allFinite(center.data(), 3);
    else if (a.is("--radius")) *good = a.real(&radius) && std::isfinite(radius) && radius > 0.0f;
    else if (a.is("--distance")) *good = a.real(&distance) && std::isfinite(distance) && distance > 0.0f;
    else return false;
    return true;
  }
  // Exactly one of the two forms, each with what it needs and nothing of the other.
  bool consistent(const Args &a) const {
    const bool hasViews = a.given("--views"), hasOrbit = a.given("--orbit"), hasCenter = a.given("--center");
    if (hasViews == hasOrbit) return false;
    const bool hasSize = a.given("--size"), hasFov = a.given("--fov-y"), hasRadius = a.given("--radius");
    if (hasViews && (hasSize || hasFov || hasCenter || hasRadius || a.given("--distance"))) return false;
    return !hasOrbit || (hasSize && hasFov && hasCenter == hasRadius);
  }
  // The views; an orbit without --center takes the box of `file`'s decoded positions.  0, 1 (failed, said why) or 2
  // (usage).
  int resolve(const Args &a, const char *tool, const char *file, spz::CoordinateSystem coord,
              std::vector<spz::PruneOptions::View> *views) {
    try {
      if (a.given("--views")) {
        *views = spz::loadViewsFile(viewsFile);
      } else {
        if (!a.given("--center")) {
          spz::UnpackOptions u;
          u.to = coord;
          const spz::GaussianCloud g = spz::loadSpz(std::string(file), u);
          if (g.numPoints <= 0 || !spz::boundingSphere(g.positions, &center, &radius)) {
            std::cerr << tool << ": " << file << " has no points to take a centre and radius from" << std::endl;
            return 1;
          }
        }
        *views = spz::orbitViews(orbit, center, radius, size[0], size[1], fovY, distance);
      }
    } catch (const std::invalid_argument &e) {
      std::cerr << e.what() << std::endl;
      return 2;
    }
    return 0;
  }
};

const char *kPruneUsage =
    "Usage: spz_prune <in.spz> <out.spz> (--views FILE | --orbit N --size W H --fov-y DEG [--center x y z --radius R] "
    "[--distance K]) (--keep N | --keep-fraction F | --min-score S) [--score sum|max] "
    "[--coord " SPZ_COORD_NAMES "]";

int spzPrune(int argc, char **argv) {
  Args a(argc, argv, kPruneUsage);
  if (!a.files()) return a.usage();
  spz::PruneOptions o;
  ViewArgs va;
  std::string score;
  while (a.next()) {
    bool good = false;
    if (va.take(a, &good)) {}
    else if (a.is("--keep")) good = a.integer(&o.keepCount.emplace(), 0, 0x7fffffff);
    else if (a.is("--keep-fraction")) good = a.real(&o.keepFraction.emplace()) && *o.keepFraction >= 0.0 &&
                                             *o.keepFraction <= 1.0;
    else if (a.is("--min-score")) good = a.real(&o.minScore.emplace()) && std::isfinite(*o.minScore);
    else if (a.is("--score")) good = a.text(&score) && (score == "sum" || score == "max");
    else if (a.is("--coord")) good = a.coord(&o.coord);
    if (!good) return a.usage();
  }
  if (score == "max") o.score = spz::PruneOptions::Max;
  const int rules = a.given("--keep") + a.given("--keep-fraction") + a.given("--min-score");
  if (rules != 1 || !va.consistent(a)) return a.usage();
  const int vr = va.resolve(a, "spz_prune", argv[1], o.coord, &o.views);
  if (vr != 0) return vr == 2 ? a.usage() : 1;
  int64_t kept = 0;
  if (!spz::pruneSpz(std::string(argv[1]), std::string(argv[2]), o, &kept)) return 1;
  std::cout << "kept " << kept << std::endl;
  return 0;
}

const char *kCompareUsage =
    "Usage: spz_compare <a.spz> <b.spz> (--views FILE | --orbit N --size W H --fov-y DEG [--center x y z --radius R] "
    "[--distance K]) [--coord " SPZ_COORD_NAMES "] [--background r g b] [--max-sh-degree D] [--near Z] "
    "[--ssim-maps PREFIX] [--min-psnr DB] [--min-ssim S]";

// A greyscale PFM ("Pf"): little-endian floats, rows bottom to top.
bool writeMap(const std::string &path, const std::vector<float> &map, int w, int h) {
  std::ofstream out(path, std::ios::binary);
  if (!out) return false;
  out << "Pf\n" << w << " " << h << "\n-1.0\n";
  for (int y = h - 1; y >= 0; --y) {
    out.write(reinterpret_cast<const char *>(map.data() + static_cast<size_t>(y) * w),
              static_cast<std::streamsize>(static_cast<size_t>(w) * sizeof(float)));
  }
  return static_cast<bool>(out);
}

// One line per view, then the mean PSNR and SSIM over the views and the worst view of each.  Exit 2 when a view misses
// --min-psnr or --min-ssim.
int spzCompare(int argc, char **argv) {
  Args a(argc, argv, kCompareUsage);
  if (!a.files()) return a.usage();
  spz::CompareOptions o;
  ViewArgs va;
  std::string mapPrefix;
  double minPsnr = 0.0, minSsim = 0.0;
  while (a.next()) {
    bool good = false;
    if (va.take(a, &good)) {}
    else if (a.is("--coord")) good = a.coord(&o.coord);
    else if (a.is("--background")) good = a.real(o.background.data(), 3) && allFinite(o.background.data(), 3);
    else if (a.is("--max-sh-degree")) good = a.integer(&o.maxShDegree, 0, 3);
    else if (a.is("--near")) good = a.real(&o.nearPlane) && std::isfinite(o.nearPlane) && o.nearPlane > 0.0f;
    else if (a.is("--ssim-maps")) good = a.text(&mapPrefix) && !mapPrefix.empty();
    else if (a.is("--min-psnr")) good = a.real(&minPsnr) && !std::isnan(minPsnr);
    else if (a.is("--min-ssim")) good = a.real(&minSsim) && !std::isnan(minSsim);
    if (!good) return a.usage();
  }
  if (!va.consistent(a)) return a.usage();
  const int vr = va.resolve(a, "spz_compare", argv[1], o.coord, &o.views);
  if (vr != 0) return vr == 2 ? a.usage() : 1;
  std::vector<spz::ImageMetrics> m;
  std::vector<std::vector<float>> maps;
  if (!spz::compareSpz(std::string(argv[1]), std::string(argv[2]), o, &m, mapPrefix.empty() ? nullptr : &maps)) {
    return 1;
  }
  double psnrSum = 0.0, ssimSum = 0.0;
  size_t worstPsnr = 0, worstSsim = 0;
  bool missed = false;
  for (size_t v = 0; v < m.size(); ++v) {
    std::printf("view %zu psnr %.17g ssim %.17g mse %.17g l1 %.17g max_abs %.17g\n", v, m[v].psnr, m[v].ssim, m[v].mse,
                m[v].l1, m[v].maxAbs);
    psnrSum += m[v].psnr;
    ssimSum += m[v].ssim;
    if (m[v].psnr < m[worstPsnr].psnr) worstPsnr = v;
    if (m[v].ssim < m[worstSsim].ssim) worstSsim = v;
    if ((a.given("--min-psnr") && m[v].psnr < minPsnr) || (a.given("--min-ssim") && m[v].ssim < minSsim)) missed = true;
    if (!mapPrefix.empty()) {
      const std::string path = mapPrefix + "_" + std::to_string(v) + ".pfm";
      if (!writeMap(path, maps[v], o.views[v].width, o.views[v].height)) {
        std::cerr << "spz_compare: unable to write " << path << std::endl;
        return 1;
      }
    }
  }
  const double n = static_cast<double>(m.size());
  std::printf("mean psnr %.17g ssim %.17g worst psnr %.17g view %zu worst ssim %.17g view %zu\n", psnrSum / n,
              ssimSum / n, m[worstPsnr].psnr, worstPsnr, m[worstSsim].ssim, worstSsim);
  std::fflush(stdout);
  return missed ? 2 : 0;
}

// The options spz_refine and spz_fit share, as their usage lines spell them.
#define SPZ_REFINE_OPTION_NAMES                                                                                         \
  "[--iters N] [--lambda-dssim L] [--lr-positions X] [--lr-scales X] [--lr-rotations X] "                              \
  "[--lr-alphas X] [--lr-colors X] [--lr-sh X] [--train positions,scales,rotations,alphas,colors,sh] "                  \
  "[--coord " SPZ_COORD_NAMES "] [--background r g b] [--max-sh-degree D] [--near Z] [--densify-interval N "            \
  "[--densify-from I] [--densify-until I] [--grad-threshold X] [--percent-dense X] [--extent X] [--min-opacity X] "     \
  "[--max-scale X] [--max-points N] [--opacity-reset-interval N] [--seed S]]"

const char *kRefineUsage =
    "Usage: spz_refine <in.spz> <target.spz> <out.spz> (--views FILE | --orbit N --size W H --fov-y DEG [--center x y z "
    "--radius R] [--distance K]) " SPZ_REFINE_OPTION_NAMES;

// Those options' parsing: take() reads the current one into `o` (false: it is not one of them), finish() settles the
// densify defaults and --train once all are read (false: a usage error).
struct RefineArgs {
  std::string train;

  bool take(Args &a, spz::RefineOptions &o, bool *ok) {
    spz::DensifyOptions &dn = o.densify;
    auto rate = [&](double *x) { return a.real(x) && std::isfinite(*x) && *x >= 0.0; };
    bool good = false;
    if (a.is("--iters")) good = a.integer(&o.iterations, 0, 0x7fffffff);
    else if (a.is("--lambda-dssim")) good = a.real(&o.lambdaDssim) && o.lambdaDssim >= 0.0 && o.lambdaDssim <= 1.0;
    else if (a.is("--lr-positions")) good = rate(&o.positionLr.emplace());
    else if (a.is("--lr-scales")) good = rate(&o.scaleLr);
    else if (a.is("--lr-rotations")) good = rate(&o.rotationLr);
    else if (a.is("--lr-alphas")) good = rate(&o.alphaLr);
    else if (a.is("--lr-colors")) good = rate(&o.colorLr);
    else if (a.is("--lr-sh")) good = rate(&o.shLr);
    else if (a.is("--train")) good = a.text(&train) && !train.empty();
    else if (a.is("--coord")) good = a.coord(&o.coord);
    else if (a.is("--background")) good = a.real(o.background.data(), 3) && allFinite(o.background.data(), 3);
    else if (a.is("--max-sh-degree")) good = a.integer(&o.maxShDegree, 0, 3);
    else if (a.is("--near")) good = a.real(&o.nearPlane) && std::isfinite(o.nearPlane) && o.nearPlane > 0.0f;
    else if (a.is("--densify-interval")) good = a.integer(&dn.interval, 0, 0x7fffffff);
    else if (a.is("--densify-from")) good = a.integer(&dn.fromIter, 0, 0x7fffffff);
    else if (a.is("--densify-until")) good = a.integer(&dn.untilIter, 0, 0x7fffffff);
    else if (a.is("--opacity-reset-interval")) good = a.integer(&dn.opacityResetInterval, 0, 0x7fffffff);
    else if (a.is("--grad-threshold")) good = rate(&dn.gradThreshold);
    else if (a.is("--percent-dense")) good = rate(&dn.percentDense) && dn.percentDense > 0.0;
    else if (a.is("--extent")) good = rate(&dn.extent);
    else if (a.is("--min-opacity")) good = rate(&dn.minOpacity) && dn.minOpacity > 0.0 && dn.minOpacity < 1.0;
    else if (a.is("--max-scale")) good = rate(&dn.maxScale);
    else if (a.is("--max-points")) good = a.integer(&dn.maxPoints, 0, 0x7fffffff);
    else if (a.is("--seed")) good = a.integer(&dn.seed, 0, UINT64_MAX);
    else return false;
    *ok = good;
    return true;
  }

  bool finish(Args &a, spz::RefineOptions &o) {
    spz::DensifyOptions &dn = o.densify;
    static const char *const kDensifyOnly[] = {"--densify-from", "--densify-until", "--grad-threshold", "--percent-dense",
                                               "--extent", "--min-opacity", "--max-scale", "--max-points",
                                               "--opacity-reset-interval", "--seed"};
    for (const char *name : kDensifyOnly) {
      if (a.given(name) && !a.given("--densify-interval")) return false;
    }
    if (dn.interval > 0) {
      if (!a.given("--densify-from")) dn.fromIter = dn.interval;
      if (!a.given("--densify-until")) dn.untilIter = std::max(dn.fromIter, o.iterations / 2);
      if (dn.untilIter < dn.fromIter) return false;
    }
    if (a.given("--train")) {
      static const char *const kArrays[6] = {"positions", "scales", "rotations", "alphas", "colors", "sh"};
      o.train = 0;
      size_t at = 0;
      while (at <= train.size()) {
        const size_t comma = std::min(train.find(',', at), train.size());
        const std::string name = train.substr(at, comma - at);
        const auto *n = std::find(std::begin(kArrays), std::end(kArrays), name);
        if (n == std::end(kArrays)) return false;
        o.train |= 1u << (n - std::begin(kArrays));
        at = comma + 1;
      }
    }
    return true;
  }
};

// spz_refine's and spz_fit's lines: one per view with its PSNR and SSIM before and after, then their means and the
// loss; with densify one line per round and the final count.
void printRefineReport(const spz::RefineReport &r, const spz::DensifyOptions &dn) {
  double sums[4] = {0.0, 0.0, 0.0, 0.0};
  for (size_t v = 0; v < r.before.size(); ++v) {
    std::printf("view %zu psnr %.17g -> %.17g ssim %.17g -> %.17g\n", v, r.before[v].psnr, r.after[v].psnr,
                r.before[v].ssim, r.after[v].ssim);
    sums[0] += r.before[v].psnr;
    sums[1] += r.after[v].psnr;
    sums[2] += r.before[v].ssim;
    sums[3] += r.after[v].ssim;
  }
  const double n = static_cast<double>(r.before.size());
  std::printf("mean psnr %.17g -> %.17g ssim %.17g -> %.17g\n", sums[0] / n, sums[1] / n, sums[2] / n, sums[3] / n);
  if (!r.history.empty()) {
    std::printf("loss %.17g -> %.17g over %zu iterations, %llu non-finite elements skipped\n", r.history.front(),
                r.history.back(), r.history.size(), static_cast<unsigned long long>(r.skipped));
  }
  if (dn.interval > 0) {
    for (const spz::DensifyRound &x : r.rounds) {
      std::printf("densify iteration %d cloned %llu split %llu culled %llu refused %llu points %llu\n", x.iteration,
                  static_cast<unsigned long long>(x.cloned), static_cast<unsigned long long>(x.split),
                  static_cast<unsigned long long>(x.culled), static_cast<unsigned long long>(x.refused),
                  static_cast<unsigned long long>(x.numPoints));
    }
    std::printf("points %llu\n", static_cast<unsigned long long>(r.numPoints));
  }
  std::fflush(stdout);
}

// One line per view with its PSNR and SSIM before and after, then their means.  An orbit without --center is taken
// around the target.  With --densify-interval N (alone: from = N, until = iterations / 2) one line per densify round
// and the final count follow.
int spzRefine(int argc, char **argv) {
  Args a(argc, argv, kRefineUsage);
  if (!a.files(3)) return a.usage();
  spz::RefineOptions o;
  ViewArgs va;
  RefineArgs ra;
  while (a.next()) {
    bool good = false;
    if (va.take(a, &good)) {}
    else if (ra.take(a, o, &good)) {}
    if (!good) return a.usage();
  }
  if (!va.consistent(a) || !ra.finish(a, o)) return a.usage();
  const int vr = va.resolve(a, "spz_refine", argv[2], o.coord, &o.views);
  if (vr != 0) return vr == 2 ? a.usage() : 1;
  spz::RefineReport r;
  if (!spz::refineSpz(std::string(argv[1]), std::string(argv[2]), std::string(argv[3]), o, &r)) return 1;
  printRefineReport(r, o.densify);
  return 0;
}

const char *kFitUsage =
    "Usage: spz_fit <in.spz> <out.spz> --views FILE --images a.ppm|a.pfm [b ...] [--masks m.ppm|m.pfm [n ...]] "
    "[--fit-exposure [--lr-exposure X] [--exposures-out FILE]] [--depths d0.pfm|none [d1 ...] [--depth-weight W] "
    "[--depth-kind l1|inverse] [--depth-min-alpha A]] " SPZ_REFINE_OPTION_NAMES;

// spz_refine against photographs: image i (and mask i, whose first channel is the weight) belongs to view i of the
// views file, as spz_locate writes it.  Prints spz_refine's lines; --exposures-out writes one line of 12 numbers
// [M | o], row-major, per view.  --depths: depth map i (a PFM as spz_render --depth writes it, or "none") belongs to
// view i; the depth error before -> after is printed per view that has a map.
int spzFit(int argc, char **argv) {
  Args a(argc, argv, kFitUsage);
  if (!a.files(2)) return a.usage();
  spz::RefineOptions o;
  spz::PhotoOptions p;
  RefineArgs ra;
  std::string viewsFile, exposuresOut;
  std::vector<std::string> images, masks, depths;
  std::string depthKind;
  double depthMinAlpha = 0.5;
  std::vector<std::string> *list = nullptr;  // the list a bare argument continues
  while (a.next()) {
    if (list != nullptr && a.arg()[0] != '-') {
      list->push_back(a.arg());
      continue;
    }
    list = nullptr;
    bool good = false;
    if (a.is("--views")) good = a.text(&viewsFile);
    else if (a.is("--images")) good = a.text(&images.emplace_back()) && (list = &images) != nullptr;
    else if (a.is("--masks")) good = a.text(&masks.emplace_back()) && (list = &masks) != nullptr;
    else if (a.is("--fit-exposure")) good = p.fitExposure = true;
    else if (a.is("--lr-exposure")) good = a.real(&p.exposureLr) && std::isfinite(p.exposureLr) && p.exposureLr >= 0.0;
    else if (a.is("--exposures-out")) good = a.text(&exposuresOut);
    else if (a.is("--depths")) good = a.text(&depths.emplace_back()) && (list = &depths) != nullptr;
    else if (a.is("--depth-weight")) good = a.real(&p.depthWeight) && std::isfinite(p.depthWeight) && p.depthWeight >= 0.0;
    else if (a.is("--depth-kind")) good = a.text(&depthKind) && (depthKind == "l1" || depthKind == "inverse");
    else if (a.is("--depth-min-alpha")) good = a.real(&depthMinAlpha) && depthMinAlpha > 0.0 && depthMinAlpha <= 1.0;
    else if (ra.take(a, o, &good)) {}
    if (!good) return a.usage();
  }
  if (!a.given("--views") || !a.given("--images") || !ra.finish(a, o)) return a.usage();
  if ((a.given("--lr-exposure") || a.given("--exposures-out")) && !p.fitExposure) return a.usage();
  if ((a.given("--depth-weight") || a.given("--depth-kind") || a.given("--depth-min-alpha")) && !a.given("--depths")) {
    return a.usage();
  }
  p.depthKind = depthKind == "inverse" ? spz::PhotoOptions::InverseL1 : spz::PhotoOptions::L1;
  p.depthMinAlpha = static_cast<float>(depthMinAlpha);
  try {
    o.views = spz::loadViewsFile(viewsFile);
  } catch (const std::invalid_argument &e) {
    std::cerr << "[SPZ ERROR] spz_fit: " << e.what() << std::endl;
    return 1;
  }
  if (o.views.size() != images.size() || (!masks.empty() && masks.size() != images.size())) {
    std::cerr << "[SPZ ERROR] spz_fit: " << o.views.size() << " views but " << images.size() << " images"
              << (masks.empty() ? std::string() : " and " + std::to_string(masks.size()) + " masks") << std::endl;
    return a.usage();
  }
  if (!depths.empty() && depths.size() != images.size()) {
    std::cerr << "[SPZ ERROR] spz_fit: " << o.views.size() << " views but " << depths.size() << " depths" << std::endl;
    return a.usage();
  }
  std::vector<std::vector<float>> zmaps(depths.size());
  std::vector<std::vector<float>> pixels(images.size()), weights(masks.size());
  for (size_t v = 0; v < images.size(); ++v) {
    for (int kind = 0; kind < (masks.empty() ? 1 : 2); ++kind) {
      const std::string &file = kind == 0 ? images[v] : masks[v];
      std::vector<float> rgb;
      int w = 0, h = 0;
      try {
        spz::loadImageFile(file, &rgb, &w, &h);
      } catch (const std::invalid_argument &e) {
        std::cerr << "[SPZ ERROR] spz_fit: " << e.what() << std::endl;
        return 1;
      }
      if (w != o.views[v].width || h != o.views[v].height) {
        std::cerr << "[SPZ ERROR] spz_fit: view " << v << " is " << o.views[v].width << " x " << o.views[v].height
                  << " but " << file << " is " << w << " x " << h << std::endl;
        return 1;
      }
      if (kind == 0) {
        pixels[v].swap(rgb);
      } else {  // the first channel
        weights[v].resize(static_cast<size_t>(w) * static_cast<size_t>(h));
        for (size_t k = 0; k < weights[v].size(); ++k) weights[v][k] = rgb[3 * k];
      }
    }
    p.images.push_back(spz::PhotoImage{pixels[v].data(), o.views[v].width, o.views[v].height, 3,
                                       masks.empty() ? nullptr : weights[v].data()});
    if (!depths.empty() && depths[v] != "none") {
      int w = 0, h = 0;
      try {
        spz::loadDepthFile(depths[v], &zmaps[v], &w, &h);
      } catch (const std::invalid_argument &e) {
        std::cerr << "[SPZ ERROR] spz_fit: " << e.what() << std::endl;
        return 1;
      }
      if (w != o.views[v].width || h != o.views[v].height) {
        std::cerr << "[SPZ ERROR] spz_fit: view " << v << " is " << o.views[v].width << " x " << o.views[v].height
                  << " but " << depths[v] << " is " << w << " x " << h << std::endl;
        return 1;
      }
      p.images.back().depth = zmaps[v].data();
    }
  }
  spz::PhotoReport r;
  if (!spz::refineSpzToImages(std::string(argv[1]), std::string(argv[2]), o, p, &r)) return 1;
  printRefineReport(r.refine, o.densify);
  for (size_t v = 0; v < r.depthError.size(); ++v) {
    if (r.depthError[v][0] < 0.0) continue;  // no map
    std::printf("view %zu depth error %.17g -> %.17g\n", v, r.depthError[v][0], r.depthError[v][1]);
  }
  std::fflush(stdout);
  if (!exposuresOut.empty()) {
    std::ofstream out(exposuresOut);
    char buf[64];
    for (const std::array<double, 12> &e : r.exposures) {
      for (size_t k = 0; k < 12; ++k) {
        std::snprintf(buf, sizeof(buf), "%.17g", e[k]);
        out << (k ? " " : "") << buf;
      }
      out << "\n";
    }
    out.flush();
    if (!out) {
      std::cerr << "[SPZ ERROR] spz_fit: unable to write " << exposuresOut << std::endl;
      return 1;
    }
  }
  return 0;
}

const char *kAlignUsage =
    "Usage: spz_align <source.spz> <target.spz> [--output aligned.spz] [--scale] [--overlap F] [--max-distance D] "
    "[--stride K] [--iterations N] [--init-centroids] [--rotate x y z w] [--translate x y z] [--init-scale S] "
    "[--coord " SPZ_COORD_NAMES "] [--fractional-bits n]";

// Prints the placement in spz_transform's own spelling, then fitness, rmse and iterations; exit 2 when the run ends
// degenerate.
int spzAlign(int argc, char **argv) {
  Args a(argc, argv, kAlignUsage);
  if (!a.files()) return a.usage();
  spz::AlignOptions o;
  std::string output;
  int32_t fractionalBits = 12;
  while (a.next()) {
    bool good = false;
    if (a.is("--output")) good = a.text(&output);
    else if (a.is("--scale")) good = o.estimateScale = true;
    else if (a.is("--overlap")) good = a.real(&o.overlap);
    else if (a.is("--max-distance")) good = a.real(&o.maxDistance.emplace());
    else if (a.is("--stride")) good = a.integer(&o.stride, 1, UINT32_MAX);
    else if (a.is("--iterations")) good = a.integer(&o.maxIterations, 1, 1000);
    else if (a.is("--init-centroids")) good = o.initCentroids = true;
    else if (a.is("--rotate")) good = a.real(o.rotation.data(), 4);
    else if (a.is("--translate")) good = a.real(o.translation.data(), 3);
    else if (a.is("--init-scale")) good = a.real(&o.scale);
    else if (a.is("--coord")) good = a.coord(&o.coord);
    else if (a.is("--fractional-bits")) good = a.integer(&fractionalBits, 0, 24);
    if (!good) return a.usage();
  }
  spz::AlignResult r;
  if (!spz::alignSpz(std::string(argv[1]), std::string(argv[2]), o, &r)) return 1;
  std::printf("--rotate %.17g %.17g %.17g %.17g --translate %.17g %.17g %.17g --scale %.17g --coord %s\n", r.rotation[0],
              r.rotation[1], r.rotation[2], r.rotation[3], r.translation[0], r.translation[1], r.translation[2], r.scale,
              kCoordNames[static_cast<int>(o.coord)]);
  std::printf("fitness %.17g rmse %.17g inliers %llu iterations %u converged %d\n", r.fitness, r.inlierRmse,
              static_cast<unsigned long long>(r.inliers), r.iterations, r.converged ? 1 : 0);
  std::fflush(stdout);
  if (r.degenerate) {
    std::cerr << "spz_align: the correspondences do not determine a rotation (fewer than three, or on one line)" << std::endl;
    return 2;
  }
  if (!output.empty()) {
    spz::TransformOptions t;
    t.rotation = r.rotation;
    t.translation = r.translation;
    t.scale = r.scale;
    t.coord = o.coord;
    t.fractionalBits = fractionalBits;
    if (!spz::transformSpz(std::string(argv[1]), output, t)) return 1;
  }
  return 0;
}

const char *kLevelUsage =
    "Usage: spz_level <in.spz> [out.spz] --threshold TAU [--hypotheses H] [--seed S] [--stride K] [--refine R] "
    "[--planes K] [--min-inliers N|FRACTION] [--axis X Y Z --max-tilt DEG] [--up-hint X Y Z] "
    "[--coord " SPZ_COORD_NAMES "] [--no-translate] [--select plane|off-plane|above|below] [--fractional-bits n]";

// Prints each plane, then the first plane's placement in spz_transform's own spelling.  With out.spz: the levelled file,
// or with --select that subset of the input.  Exit 2 when no plane reaches --min-inliers.
int spzLevel(int argc, char **argv) {
  Args a(argc, argv, kLevelUsage);
  const bool hasOut = argc > 2 && argv[2][0] != '-';
  if (!a.files(hasOut ? 2 : 1)) return a.usage();
  spz::LevelOptions o;
  while (a.next()) {
    bool good = false;
    if (a.is("--threshold")) good = a.real(&o.threshold) && !std::isnan(o.threshold);
    else if (a.is("--hypotheses")) good = a.integer(&o.hypotheses, 1, 65536);
    else if (a.is("--seed")) good = a.integer(&o.seed, 0, UINT64_MAX);
    else if (a.is("--stride")) good = a.integer(&o.stride, 1, UINT32_MAX);
    else if (a.is("--refine")) good = a.integer(&o.refine, 0, 16);
    else if (a.is("--planes")) good = a.integer(&o.planes, 1, 255);
    else if (a.is("--min-inliers")) {
      std::string v;
      good = a.text(&v) && !v.empty();
      if (good && v.find_first_not_of("0123456789") == std::string::npos) {  // a count
        char *end = nullptr;
        errno = 0;
        o.minInliers = std::strtoull(v.c_str(), &end, 10);
        good = errno == 0;
      } else if (good) {  // a fraction of the points taking part
        char *end = nullptr;
        o.minInlierFraction = std::strtod(v.c_str(), &end);
        good = end != v.c_str() && *end == '\0' && o.minInlierFraction >= 0.0 && o.minInlierFraction <= 1.0;
      }
    } else if (a.is("--axis")) good = a.real(o.axis.emplace().data(), 3);
    else if (a.is("--max-tilt")) good = a.real(&o.maxTilt);
    else if (a.is("--up-hint")) good = a.real(o.upHint.emplace().data(), 3);
    else if (a.is("--coord")) good = a.coord(&o.coord);
    else if (a.is("--no-translate")) good = o.noTranslate = true;
    else if (a.is("--fractional-bits")) good = a.integer(&o.fractionalBits, 0, 24);
    else if (a.is("--select")) {
      std::string v;
      good = a.text(&v);
      if (v == "plane") o.select = spz::LevelOptions::Select::Plane;
      else if (v == "off-plane") o.select = spz::LevelOptions::Select::OffPlane;
      else if (v == "above") o.select = spz::LevelOptions::Select::Above;
      else if (v == "below") o.select = spz::LevelOptions::Select::Below;
      else good = false;
    }
    if (!good) return a.usage();
  }
  if (!a.given("--threshold") || a.given("--max-tilt") != a.given("--axis") || (a.given("--select") && !hasOut)) {
    return a.usage();
  }
  spz::LevelResult r;
  const bool ok = hasOut ? spz::levelSpz(std::string(argv[1]), std::string(argv[2]), o, &r)
                         : spz::detectPlanes(std::string(argv[1]), o, &r);
  if (!ok) return 1;
  for (size_t k = 0; k < r.planes.size(); ++k) {
    const spz::DetectedPlane &p = r.planes[k];
    std::printf("plane %zu normal %.17g %.17g %.17g offset %.17g inliers %llu of %llu fitness %.17g mean-distance %.17g "
                "integers %d %d %d %lld\n", k + 1, p.normal[0], p.normal[1], p.normal[2], p.offset,
                static_cast<unsigned long long>(p.inliers), static_cast<unsigned long long>(p.points), p.fitness,
                p.meanDistance, p.normalInt[0], p.normalInt[1], p.normalInt[2], static_cast<long long>(p.offsetInt));
  }
  if (r.planes.empty()) {
    std::fflush(stdout);
    std::cerr << "spz_level: no plane reaches --min-inliers" << std::endl;
    return 2;
  }
  const spz::DetectedPlane &f = r.planes[0];
  std::printf("--rotate %.17g %.17g %.17g %.17g --translate %.17g %.17g %.17g --scale 1 --coord %s\n", f.rotation[0],
              f.rotation[1], f.rotation[2], f.rotation[3], f.translation[0], f.translation[1], f.translation[2],
              kCoordNames[static_cast<int>(o.coord)]);
  if (r.kept >= 0) std::printf("kept %lld\n", static_cast<long long>(r.kept));
  std::fflush(stdout);
  return 0;
}

const char *kLocateUsage =
    "Usage: spz_locate <scene.spz> --views FILE --images a.pfm|a.ppm [b ...] [--out FILE] [--iterations N] "
    "[--lr-rotation R] [--lr-translation T] [--lambda L] [--levels K] [--coord " SPZ_COORD_NAMES "] "
    "[--background r g b] [--max-sh-degree D] [--near Z]";

// View i of the views file is fitted to image i.  Writes the fitted views in the views file's own spelling (to --out,
// or to stdout), so they feed spz_prune, spz_compare and spz_refine --views: per view a '#' comment line with its PSNR
// before and after, then the view's line.  With --out the PSNR lines also go to stdout.
int spzLocate(int argc, char **argv) {
  Args a(argc, argv, kLocateUsage);
  if (!a.files(1)) return a.usage();
  spz::LocateOptions o;
  std::string viewsFile, outFile;
  std::vector<std::string> images;
  bool inImages = false;
  while (a.next()) {
    if (inImages && a.arg()[0] != '-') {  // the rest of --images' list
      images.push_back(a.arg());
      continue;
    }
    inImages = false;
    bool good = false;
    if (a.is("--views")) good = a.text(&viewsFile);
    else if (a.is("--images")) good = inImages = a.text(&images.emplace_back());
    else if (a.is("--out")) good = a.text(&outFile);
    else if (a.is("--iterations")) good = a.integer(&o.iterations, 0, 0x7fffffff);
    else if (a.is("--lr-rotation")) good = a.real(&o.rotationLr) && std::isfinite(o.rotationLr) && o.rotationLr >= 0.0;
    else if (a.is("--lr-translation")) {
      good = a.real(&o.translationLr.emplace()) && std::isfinite(*o.translationLr) && *o.translationLr >= 0.0;
    }
    else if (a.is("--lambda")) good = a.real(&o.lambdaDssim) && o.lambdaDssim >= 0.0 && o.lambdaDssim <= 1.0;
    else if (a.is("--levels")) good = a.integer(&o.levels, 1, 8);
    else if (a.is("--coord")) good = a.coord(&o.coord);
    else if (a.is("--background")) good = a.real(o.background.data(), 3) && allFinite(o.background.data(), 3);
    else if (a.is("--max-sh-degree")) good = a.integer(&o.maxShDegree, 0, 3);
    else if (a.is("--near")) good = a.real(&o.nearPlane) && std::isfinite(o.nearPlane) && o.nearPlane > 0.0f;
    if (!good) return a.usage();
  }
  if (!a.given("--views") || !a.given("--images")) return a.usage();
  std::vector<spz::PruneOptions::View> views;
  try {
    views = spz::loadViewsFile(viewsFile);
  } catch (const std::invalid_argument &e) {
    std::cerr << "[SPZ ERROR] spz_locate: " << e.what() << std::endl;
    return 1;
  }
  if (views.size() != images.size()) {
    std::cerr << "[SPZ ERROR] spz_locate: " << views.size() << " views but " << images.size() << " images" << std::endl;
    return 1;
  }
  std::vector<std::string> lines, notes;
  for (size_t v = 0; v < views.size(); ++v) {
    std::vector<float> pixels;
    int w = 0, h = 0;
    try {
      spz::loadImageFile(images[v], &pixels, &w, &h);
    } catch (const std::invalid_argument &e) {
      std::cerr << "[SPZ ERROR] spz_locate: " << e.what() << std::endl;
      return 1;
    }
    if (w != views[v].width || h != views[v].height) {
      std::cerr << "[SPZ ERROR] spz_locate: view " << v << " is " << views[v].width << " x " << views[v].height << " but "
                << images[v] << " is " << w << " x " << h << std::endl;
      return 1;
    }
    spz::LocateReport r;
    if (!spz::locateSpz(std::string(argv[1]), views[v], pixels.data(), 3, o, &r)) return 1;
    char buf[1024];
    const std::array<float, 12> &m = r.view.worldToCamera;
    std::snprintf(buf, sizeof(buf), "%d %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g",
                  r.view.width, r.view.height, r.view.fx, r.view.fy, r.view.cx, r.view.cy, m[0], m[1], m[2], m[3], m[4], m[5],
                  m[6], m[7], m[8], m[9], m[10], m[11]);
    lines.push_back(buf);
    std::snprintf(buf, sizeof(buf), "view %zu psnr %.17g -> %.17g after %d iterations", v, r.before.psnr, r.after.psnr,
                  r.iterations);
    notes.push_back(buf);
  }
  if (!outFile.empty()) {
    std::ofstream out(outFile);
    for (size_t v = 0; v < lines.size(); ++v) out << "# " << notes[v] << "\n" << lines[v] << "\n";
    out.flush();
    if (!out) {
      std::cerr << "[SPZ ERROR] spz_locate: unable to write " << outFile << std::endl;
      return 1;
    }
    for (const std::string &n : notes) std::cout << n << std::endl;
  } else {
    for (size_t v = 0; v < lines.size(); ++v) std::cout << "# " << notes[v] << "\n" << lines[v] << std::endl;
  }
  return 0;
}

const char *kMeshUsage =
    "Usage: spz_mesh <in.spz> <out.ply> (--views FILE | --orbit N --size W H --fov-y DEG [--center x y z --radius R] "
    "[--distance K]) [--voxel S | --resolution N] [--box x0 y0 z0 x1 y1 z1] [--truncation T] [--depth median|expected] "
    "[--min-alpha A] [--min-weight W] [--near Z] [--coord " SPZ_COORD_NAMES "]";

// The file's triangle mesh (spz::meshSpz) as a binary PLY; prints the vertex and triangle counts and the volume.
int spzMesh(int argc, char **argv) {
  Args a(argc, argv, kMeshUsage);
  if (!a.files()) return a.usage();
  spz::MeshOptions o;
  ViewArgs va;
  std::string depth;
  while (a.next()) {
    bool good = false;
    if (va.take(a, &good)) {}
    else if (a.is("--voxel")) good = a.real(&o.voxelSize.emplace()) && std::isfinite(*o.voxelSize) && *o.voxelSize > 0.0;
    else if (a.is("--resolution")) good = a.integer(&o.resolution.emplace(), 1, 2046);
    else if (a.is("--box")) {
      std::array<double, 6> &b = o.box.emplace();
      good = a.real(b.data(), 6) && std::all_of(b.begin(), b.end(), [](double v) { return std::isfinite(v); }) &&
             b[3] > b[0] && b[4] > b[1] && b[5] > b[2];
    }
    else if (a.is("--truncation")) good = a.real(&o.truncation.emplace()) && std::isfinite(*o.truncation) && *o.truncation > 0.0;
    else if (a.is("--depth")) good = a.text(&depth) && (depth == "median" || depth == "expected");
    else if (a.is("--min-alpha")) good = a.real(&o.minAlpha) && o.minAlpha >= 0.0f && o.minAlpha <= 1.0f;
    else if (a.is("--min-weight")) good = a.real(&o.minWeight) && std::isfinite(o.minWeight) && o.minWeight > 0.0f;
    else if (a.is("--near")) good = a.real(&o.nearPlane) && std::isfinite(o.nearPlane) && o.nearPlane > 0.0f;
    else if (a.is("--coord")) good = a.coord(&o.coord);
    if (!good) return a.usage();
  }
  if (depth == "expected") o.depth = spz::MeshOptions::Expected;
  if ((a.given("--voxel") && a.given("--resolution")) || !va.consistent(a)) return a.usage();
  const int vr = va.resolve(a, "spz_mesh", argv[1], o.coord, &o.views);
  if (vr != 0) return vr == 2 ? a.usage() : 1;
  spz::TriangleMesh mesh;
  if (!spz::meshSpz(std::string(argv[1]), o, &mesh)) return 1;
  if (!spz::saveMeshPly(std::string(argv[2]), mesh)) return 1;
  std::cout << mesh.vertices.size() / 3 << " vertices, " << mesh.triangles.size() / 3 << " triangles; lattice "
            << mesh.dims[0] << " x " << mesh.dims[1] << " x " << mesh.dims[2] << " at " << mesh.voxelSize << " from ("
            << mesh.lo[0] << ", " << mesh.lo[1] << ", " << mesh.lo[2] << "), truncation " << mesh.truncation << std::endl;
  return 0;
}

const char *kSeedUsage =
    "Usage: spz_seed <out.spz> --views FILE --images a.ppm|a.pfm [b ...] --depths d0.pfm [d1 ...] "
    "[--masks m.ppm|m.pfm [n ...]] [--onto base.spz] [--stride S] [--scale-factor F] [--opacity O] [--no-cover] "
    "[--cover-alpha A] [--cover-tolerance T] [--sh-degree D] [--max-points N] [--near Z] [--coord " SPZ_COORD_NAMES "]";

// A file from posed photographs with depth maps (spz::seedSpz): image i, depth map i (a PFM as spz_render --depth writes
// it) and mask i (its first channel above 0.5: the sample counts) belong to view i of the views file.  With --onto only
// the points the base does not explain are written; spz_merge joins the two.  Prints one line per view and the total.
int spzSeed(int argc, char **argv) {
  Args a(argc, argv, kSeedUsage);
  if (!a.files(1)) return a.usage();
  spz::SeedOptions o;
  ViewArgs va;
  std::vector<std::string> images, masks, depths;
  std::string onto;
  std::vector<std::string> *list = nullptr;  // the list a bare argument continues
  while (a.next()) {
    if (list != nullptr && a.arg()[0] != '-') {
      list->push_back(a.arg());
      continue;
    }
    list = nullptr;
    bool good = false;
    if (va.take(a, &good)) {}
    else if (a.is("--images")) good = a.text(&images.emplace_back()) && (list = &images) != nullptr;
    else if (a.is("--depths")) good = a.text(&depths.emplace_back()) && (list = &depths) != nullptr;
    else if (a.is("--masks")) good = a.text(&masks.emplace_back()) && (list = &masks) != nullptr;
    else if (a.is("--onto")) good = a.text(&onto);
    else if (a.is("--stride")) good = a.integer(&o.stride, 1, 64);
    else if (a.is("--scale-factor")) good = a.real(&o.scaleFactor) && std::isfinite(o.scaleFactor) && o.scaleFactor > 0.0;
    else if (a.is("--opacity")) good = a.real(&o.opacity);  // its range is seedSpz's to refuse
    else if (a.is("--no-cover")) good = !(o.cover = false);
    else if (a.is("--cover-alpha")) good = a.real(&o.coverAlpha) && o.coverAlpha >= 0.0f && o.coverAlpha <= 1.0f;
    else if (a.is("--cover-tolerance")) good = a.real(&o.coverTolerance) && std::isfinite(o.coverTolerance) && o.coverTolerance >= 0.0f;
    else if (a.is("--sh-degree")) good = a.integer(&o.shDegree, 0, 3);
    else if (a.is("--max-points")) good = a.integer(&o.maxPoints, 0, 10000000);
    else if (a.is("--near")) good = a.real(&o.nearPlane) && std::isfinite(o.nearPlane) && o.nearPlane > 0.0f;
    else if (a.is("--coord")) good = a.coord(&o.coord);
    if (!good) return a.usage();
  }
  if (!a.given("--views") || !va.consistent(a) || !a.given("--images") || !a.given("--depths")) return a.usage();
  if (depths.size() != images.size() || (!masks.empty() && masks.size() != images.size())) {
    std::cerr << "[SPZ ERROR] spz_seed: " << images.size() << " images but " << depths.size() << " depths"
              << (masks.empty() ? std::string() : " and " + std::to_string(masks.size()) + " masks") << std::endl;
    return a.usage();
  }
  const int vr = va.resolve(a, "spz_seed", argv[1], o.coord, &o.views);
  if (vr != 0) return vr == 2 ? a.usage() : 1;
  if (!onto.empty()) o.base = onto;
  // every file at its own size: seedSpz compares an image with its view, an image's depth and mask are compared here
  std::vector<std::vector<float>> pixels(images.size()), zmaps(images.size()), weights(masks.size());
  std::vector<spz::PhotoImage> photos;
  for (size_t v = 0; v < images.size(); ++v) {
    int w = 0, h = 0;
    try {
      spz::loadImageFile(images[v], &pixels[v], &w, &h);
      photos.push_back(spz::PhotoImage{pixels[v].data(), w, h, 3, nullptr, nullptr});
      for (int kind = 0; kind < (masks.empty() ? 1 : 2); ++kind) {
        const std::string &file = kind == 0 ? depths[v] : masks[v];
        int fw = 0, fh = 0;
        std::vector<float> rgb;
        if (kind == 0) spz::loadDepthFile(file, &zmaps[v], &fw, &fh);
        else spz::loadImageFile(file, &rgb, &fw, &fh);
        if (fw != w || fh != h) {
          std::cerr << "[SPZ ERROR] spz_seed: " << images[v] << " is " << w << " x " << h << " but " << file << " is " << fw
                    << " x " << fh << std::endl;
          return 1;
        }
        if (kind == 0) {
          photos.back().depth = zmaps[v].data();
        } else {  // the first channel
          weights[v].resize(static_cast<size_t>(w) * static_cast<size_t>(h));
          for (size_t k = 0; k < weights[v].size(); ++k) weights[v][k] = rgb[3 * k];
          photos.back().weights = weights[v].data();
        }
      }
    } catch (const std::invalid_argument &e) {
      std::cerr << "[SPZ ERROR] spz_seed: " << e.what() << std::endl;
      return 1;
    }
  }
  spz::SeedReport r;
  if (!spz::seedSpz(o, photos, std::string(argv[1]), &r)) return 1;
  for (size_t v = 0; v < r.views.size(); ++v) {
    std::printf("view %zu valid %llu appended %llu refused %llu\n", v, static_cast<unsigned long long>(r.views[v].valid),
                static_cast<unsigned long long>(r.views[v].appended), static_cast<unsigned long long>(r.views[v].refused));
  }
  std::printf("points %llu\n", static_cast<unsigned long long>(r.numPoints));
  std::fflush(stdout);
  return 0;
}

const struct {
  const char *name;
  int (*run)(int, char **);
} kTools[] = {{"ply_to_spz", plyToSpz},     {"spz_to_ply", spzToPly},         {"spz_info", spzInfo},
              {"spz_filter", spzFilter},    {"spz_transform", spzTransform},  {"spz_merge", spzMerge},
              {"spz_sort", spzSort},        {"spz_decimate", spzDecimate},    {"spz_clean", spzClean},
              {"spz_render", spzRender},    {"spz_mesh", spzMesh},            {"spz_prune", spzPrune},
              {"spz_compare", spzCompare},  {"spz_tile", spzTile},            {"spz_align", spzAlign},           {"spz_level", spzLevel},
              {"spz_refine", spzRefine},    {"spz_fit", spzFit},              {"spz_seed", spzSeed},
              {"spz_locate", spzLocate}};

int dispatch(const std::string &tool, int argc, char **argv) {
  for (const auto &t : kTools) {
    if (tool == t.name) return t.run(argc, argv);
  }
  return -1;
}

}  // namespace

int main(int argc, char **argv) {
  try {
    std::string self = argc > 0 ? argv[0] : "";
    const size_t slash = self.find_last_of('/');
    if (slash != std::string::npos) self = self.substr(slash + 1);
    int rc = dispatch(self, argc, argv);
    if (rc >= 0) return rc;
    if (argc >= 2) {
      rc = dispatch(argv[1], argc - 1, argv + 1);
      if (rc >= 0) return rc;
    }
    std::cerr << "Usage: spz_tool {";
    for (const auto &t : kTools) std::cerr << (&t == kTools ? "" : "|") << t.name;
    std::cerr << "} <args...>" << std::endl;
    return 1;
  } catch (const std::exception &e) {
    std::cerr << "Error: " << e.what() << std::endl;
    return 1;
  }
}
