// spz_cli.cpp — the three command-line tools of the reference (cli_tools/src/*.cpp) over the
// MI355X drop-in layer: ply_to_spz, spz_to_ply, spz_info; and spz_filter (spz::filterSpz),
// spz_transform (spz::transformSpz), spz_merge (spz::mergeSpz), spz_sort (spz::sortSpz), spz_decimate
// (spz::decimateSpz), spz_clean (spz::cleanSpz), spz_render (spz::renderSpz) and spz_prune (spz::pruneSpz), which have
// no counterpart in the reference.  One binary, dispatched on argv[0] (the Makefile installs it under the eleven names)
// or on a first argument naming the tool.
// Same behaviour as the reference mains: default (UNSPECIFIED) pack/unpack options, exit code 0
// once the arguments are there (the reference ignores the save/load results), usage -> 1.
// spz_filter, spz_transform, spz_merge, spz_sort, spz_decimate, spz_clean, spz_render and spz_prune exit 1 when the
// filter / transform / merge / sort / decimation / clean / render / prune fails as well.
#include <algorithm>
#include <stdexcept>
#include <array>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <fstream>
#include <iostream>
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

const char *kFilterUsage =
    "Usage: spz_filter <input.spz> <output.spz> [--sh-degree D] [--min-alpha A] [--box x0 y0 z0 x1 y1 z1] "
    "[--coord RUB|RDF|LUF|RUF|LDB|RDB|LUB|LDF|UNSPECIFIED]";

bool parseFloat(const char *s, float *v) {
  char *end = nullptr;
  *v = std::strtof(s, &end);
  return end != s && *end == '\0';
}

int spzFilter(int argc, char **argv) {
  auto usage = [] {
    std::cerr << kFilterUsage << std::endl;
    return 1;
  };
  if (argc < 3) return usage();
  spz::FilterOptions f;
  for (int i = 3; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--sh-degree" && i + 1 < argc) {
      char *end = nullptr;
      const long d = std::strtol(argv[++i], &end, 10);
      if (*end != '\0' || d < 0 || d > 3) return usage();
      f.shDegree = static_cast<int32_t>(d);
    } else if (a == "--min-alpha" && i + 1 < argc) {
      float v = 0;
      if (!parseFloat(argv[++i], &v)) return usage();
      f.minAlpha = v;
    } else if (a == "--box" && i + 6 < argc) {
      spz::FilterOptions::Box b;
      for (int k = 0; k < 6; ++k) {
        if (!parseFloat(argv[i + 1 + k], k < 3 ? &b.lo[k] : &b.hi[k - 3])) return usage();
      }
      i += 6;
      f.box = b;
    } else if (a == "--coord" && i + 1 < argc) {
      static const char *names[] = {"UNSPECIFIED", "LDB", "RDB", "LUB", "RUB", "LDF", "RDF", "LUF", "RUF"};
      const std::string c = argv[++i];
      int found = -1;
      for (int k = 0; k < 9; ++k) {
        if (c == names[k]) found = k;
      }
      if (found < 0) return usage();
      f.coord = static_cast<spz::CoordinateSystem>(found);
    } else {
      return usage();
    }
  }
  int64_t kept = 0;
  if (!spz::filterSpz(std::string(argv[1]), std::string(argv[2]), f, &kept)) return 1;
  std::cout << "Points kept: " << kept << std::endl;
  return 0;
}

const char *kTransformUsage =
    "Usage: spz_transform <input.spz> <output.spz> [--rotate x y z w] [--translate x y z] [--scale s] "
    "[--coord RUB|RDF|LUF|RUF|LDB|RDB|LUB|LDF|UNSPECIFIED] [--fractional-bits n]";

bool parseDouble(const char *s, double *v) {
  char *end = nullptr;
  *v = std::strtod(s, &end);
  return end != s && *end == '\0';
}

int spzTransform(int argc, char **argv) {
  auto usage = [] {
    std::cerr << kTransformUsage << std::endl;
    return 1;
  };
  if (argc < 3) return usage();
  spz::TransformOptions o;
  for (int i = 3; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--rotate" && i + 4 < argc) {
      for (int k = 0; k < 4; ++k) {
        if (!parseDouble(argv[i + 1 + k], &o.rotation[k])) return usage();
      }
      i += 4;
    } else if (a == "--translate" && i + 3 < argc) {
      for (int k = 0; k < 3; ++k) {
        if (!parseDouble(argv[i + 1 + k], &o.translation[k])) return usage();
      }
      i += 3;
    } else if (a == "--scale" && i + 1 < argc) {
      if (!parseDouble(argv[++i], &o.scale)) return usage();
    } else if (a == "--coord" && i + 1 < argc) {
      static const char *names[] = {"UNSPECIFIED", "LDB", "RDB", "LUB", "RUB", "LDF", "RDF", "LUF", "RUF"};
      const std::string c = argv[++i];
      int found = -1;
      for (int k = 0; k < 9; ++k) {
        if (c == names[k]) found = k;
      }
      if (found < 0) return usage();
      o.coord = static_cast<spz::CoordinateSystem>(found);
    } else if (a == "--fractional-bits" && i + 1 < argc) {
      char *end = nullptr;
      const long d = std::strtol(argv[++i], &end, 10);
      if (*end != '\0' || d < 0 || d > 24) return usage();
      o.fractionalBits = static_cast<int32_t>(d);
    } else {
      return usage();
    }
  }
  return spz::transformSpz(std::string(argv[1]), std::string(argv[2]), o) ? 0 : 1;
}

const char *kMergeUsage =
    "Usage: spz_merge <input.spz>... -o <output.spz> [--sh-degree D] [--fractional-bits B] [--antialiased 0|1]";

bool parseInt(const char *s, long lo, long hi, int32_t *v) {
  char *end = nullptr;
  const long d = std::strtol(s, &end, 10);
  if (end == s || *end != '\0' || d < lo || d > hi) return false;
  *v = static_cast<int32_t>(d);
  return true;
}

int spzMerge(int argc, char **argv) {
  auto usage = [] {
    std::cerr << kMergeUsage << std::endl;
    return 1;
  };
  spz::MergeOptions o;
  std::vector<std::string> inputs;
  std::string output;
  bool have_output = false;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "-o" && i + 1 < argc && !have_output) {
      output = argv[++i];
      have_output = true;
    } else if (a == "--sh-degree" && i + 1 < argc) {
      if (!parseInt(argv[++i], 0, 3, &o.shDegree)) return usage();
    } else if (a == "--fractional-bits" && i + 1 < argc) {
      if (!parseInt(argv[++i], 0, 24, &o.fractionalBits)) return usage();
    } else if (a == "--antialiased" && i + 1 < argc) {
      if (!parseInt(argv[++i], 0, 1, &o.antialiased)) return usage();
    } else if (!a.empty() && a[0] == '-') {
      return usage();
    } else {
      inputs.push_back(a);
    }
  }
  if (inputs.empty() || !have_output || output.empty()) return usage();
  return spz::mergeSpz(inputs, output, o) ? 0 : 1;
}

const char *kSortUsage = "Usage: spz_sort <input.spz> <output.spz> [--keys <keys.f32>] [--descending]";

int spzSort(int argc, char **argv) {
  auto usage = [] {
    std::cerr << kSortUsage << std::endl;
    return 1;
  };
  if (argc < 3 || argv[1][0] == '-' || argv[2][0] == '-') return usage();
  spz::SortOptions o;
  const char *keys = nullptr;
  for (int i = 3; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--keys" && i + 1 < argc && keys == nullptr) {
      keys = argv[++i];
    } else if (a == "--descending" && !o.descending) {
      o.descending = true;
    } else {
      return usage();
    }
  }
  if (keys != nullptr) {
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
  auto usage = [] {
    std::cerr << kDecimateUsage << std::endl;
    return 1;
  };
  if (argc != 5 || argv[1][0] == '-' || argv[2][0] == '-') return usage();
  const std::string flag = argv[3], value = argv[4];
  // a plain decimal number, nothing else
  if (value.empty() || value.size() > 19 || value.find_first_not_of("0123456789") != std::string::npos) return usage();
  const unsigned long long v = std::strtoull(value.c_str(), nullptr, 10);
  spz::DecimateOptions o;
  if (flag == "--level" && v <= 24) {
    o.level = static_cast<int>(v);
  } else if (flag == "--target" && v >= 1) {
    o.targetPoints = static_cast<uint64_t>(v);
  } else {
    return usage();
  }
  return spz::decimateSpz(std::string(argv[1]), std::string(argv[2]), o) ? 0 : 1;
}

const char *kCleanUsage =
    "Usage: spz_clean <input.spz> <output.spz> [--k <K> [--std-ratio <S>]] [--radius <R> --min-neighbors <M>]";

// a plain decimal integer in lo..hi
bool parseCount(const char *s, int lo, int hi, int *v) {
  const std::string t = s;
  if (t.empty() || t.size() > 4 || t.find_first_not_of("0123456789") != std::string::npos) return false;
  *v = std::atoi(s);
  return *v >= lo && *v <= hi;
}

int spzClean(int argc, char **argv) {
  auto usage = [] {
    std::cerr << kCleanUsage << std::endl;
    return 1;
  };
  if (argc < 5 || argv[1][0] == '-' || argv[2][0] == '-' || (argc - 3) % 2 != 0) return usage();
  bool hasK = false, hasRatio = false, hasRadius = false, hasMin = false;
  spz::CleanOptions::Statistical st;
  spz::CleanOptions::Radius rd;
  for (int i = 3; i < argc; i += 2) {
    const std::string flag = argv[i];
    const char *value = argv[i + 1];
    if (flag == "--k" && !hasK) {
      if (!parseCount(value, 1, 64, &st.k)) return usage();
      hasK = true;
    } else if (flag == "--std-ratio" && !hasRatio) {
      if (!parseDouble(value, &st.stdRatio) || !std::isfinite(st.stdRatio)) return usage();
      hasRatio = true;
    } else if (flag == "--radius" && !hasRadius) {
      if (!parseDouble(value, &rd.radius) || !std::isfinite(rd.radius) || !(rd.radius > 0.0)) return usage();
      hasRadius = true;
    } else if (flag == "--min-neighbors" && !hasMin) {
      if (!parseCount(value, 1, 256, &rd.minNeighbors)) return usage();
      hasMin = true;
    } else {
      return usage();
    }
  }
  if ((hasRatio && !hasK) || hasRadius != hasMin || (!hasK && !hasRadius)) return usage();
  spz::CleanOptions o;
  if (hasK) o.statistical = st;
  if (hasRadius) o.radius = rd;
  return spz::cleanSpz(std::string(argv[1]), std::string(argv[2]), o) ? 0 : 1;
}

const char *kRenderUsage =
    "Usage: spz_render <in.spz> <out.ppm|out.pfm> --size W H (--fov-y DEG | --intrinsics fx fy cx cy) --eye x y z "
    "--target x y z [--up x y z] [--coord RUB|RDF|LUF|RUF|LDB|RDB|LUB|LDF|UNSPECIFIED] [--background r g b] "
    "[--sh-degree D] [--near N]";

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

int spzRender(int argc, char **argv) {
  auto usage = [] {
    std::cerr << kRenderUsage << std::endl;
    return 1;
  };
  if (argc < 3 || argv[1][0] == '-' || argv[2][0] == '-') return usage();
  const std::string outPath = argv[2];
  const bool pfm = endsWith(outPath, ".pfm");
  if (!pfm && !endsWith(outPath, ".ppm")) return usage();
  spz::RenderOptions o;
  bool hasSize = false, hasFov = false, hasIntr = false, hasEye = false, hasTarget = false, hasUp = false;
  bool hasBackground = false, hasNear = false, hasShDegree = false, hasCoord = false;
  float fovY = 0.0f, intr[4] = {0, 0, 0, 0};
  std::array<float, 3> eye{}, target{}, up{};
  auto floats = [&](int &i, int k, float *dst) {
    if (i + k >= argc) return false;
    for (int j = 0; j < k; ++j) {
      if (!parseFloat(argv[i + 1 + j], &dst[j]) || !std::isfinite(dst[j])) return false;
    }
    i += k;
    return true;
  };
  for (int i = 3; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--size" && !hasSize && i + 2 < argc) {
      int v[2];
      for (int k = 0; k < 2; ++k) {
        const std::string t = argv[i + 1 + k];
        if (t.empty() || t.size() > 5 || t.find_first_not_of("0123456789") != std::string::npos) return usage();
        v[k] = std::atoi(t.c_str());
        if (v[k] < 1 || v[k] > 16384) return usage();
      }
      o.width = v[0];
      o.height = v[1];
      i += 2;
      hasSize = true;
    } else if (a == "--fov-y" && !hasFov && !hasIntr) {
      if (!floats(i, 1, &fovY) || !(fovY > 0.0f && fovY < 180.0f)) return usage();
      hasFov = true;
    } else if (a == "--intrinsics" && !hasFov && !hasIntr) {
      if (!floats(i, 4, intr)) return usage();
      hasIntr = true;
    } else if (a == "--eye" && !hasEye) {
      if (!floats(i, 3, eye.data())) return usage();
      hasEye = true;
    } else if (a == "--target" && !hasTarget) {
      if (!floats(i, 3, target.data())) return usage();
      hasTarget = true;
    } else if (a == "--up" && !hasUp) {
      if (!floats(i, 3, up.data())) return usage();
      hasUp = true;
    } else if (a == "--background" && !hasBackground) {
      if (!floats(i, 3, o.background.data())) return usage();
      hasBackground = true;
    } else if (a == "--near" && !hasNear) {
      if (!floats(i, 1, &o.nearPlane) || !(o.nearPlane > 0.0f)) return usage();
      hasNear = true;
    } else if (a == "--sh-degree" && !hasShDegree && i + 1 < argc) {
      const std::string t = argv[++i];
      if (t.size() != 1 || t[0] < '0' || t[0] > '3') return usage();
      o.maxShDegree = t[0] - '0';
      hasShDegree = true;
    } else if (a == "--coord" && !hasCoord && i + 1 < argc) {
      hasCoord = true;
      static const char *names[] = {"UNSPECIFIED", "LDB", "RDB", "LUB", "RUB", "LDF", "RDF", "LUF", "RUF"};
      const std::string c = argv[++i];
      int found = -1;
      for (int k = 0; k < 9; ++k) {
        if (c == names[k]) found = k;
      }
      if (found < 0) return usage();
      o.coord = static_cast<spz::CoordinateSystem>(found);
    } else {
      return usage();
    }
  }
  if (!hasSize || (!hasFov && !hasIntr) || !hasEye || !hasTarget) return usage();
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
    if (!(o.fx > 0.0f) || !(o.fy > 0.0f)) return usage();
  }
  if (!hasUp) {  // the frame's U axis (UNSPECIFIED: the stored RUB frame)
    const int c = static_cast<int>(o.coord) == 0 ? 4 : static_cast<int>(o.coord);
    const bool yDown = (((c - 1) >> 1) & 1) == 0;  // LDB, RDB, LDF, RDF
    up = {0.0f, yDown ? -1.0f : 1.0f, 0.0f};
  }
  try {
    o.worldToCamera = spz::lookAt(eye, target, up);
  } catch (const std::invalid_argument &) {
    return usage();
  }
  std::vector<float> rgba;
  if (!spz::renderSpz(std::string(argv[1]), o, &rgba)) return 1;
  if (!writeImage(outPath, rgba, o.width, o.height, pfm)) {
    std::cerr << "spz_render: unable to write " << outPath << std::endl;
    return 1;
  }
  return 0;
}

const char *kPruneUsage =
    "Usage: spz_prune <in.spz> <out.spz> (--views FILE | --orbit N --size W H --fov-y DEG [--center x y z --radius R] "
    "[--distance K]) (--keep N | --keep-fraction F | --min-score S) [--score sum|max] "
    "[--coord RUB|RDF|LUF|RUF|LDB|RDB|LUB|LDF|UNSPECIFIED]";

int spzPrune(int argc, char **argv) {
  auto usage = [] {
    std::cerr << kPruneUsage << std::endl;
    return 1;
  };
  if (argc < 3 || argv[1][0] == '-' || argv[2][0] == '-') return usage();
  spz::PruneOptions o;
  std::string viewsFile;
  int orbit = 0, size[2] = {0, 0};
  float fovY = 0.0f, radius = 0.0f, distance = 2.5f;
  std::array<float, 3> center{};
  bool hasViews = false, hasOrbit = false, hasSize = false, hasFov = false, hasCenter = false, hasRadius = false;
  bool hasDistance = false, hasScore = false, hasCoord = false;
  auto floats = [&](int &i, int k, float *dst) {
    if (i + k >= argc) return false;
    for (int j = 0; j < k; ++j) {
      if (!parseFloat(argv[i + 1 + j], &dst[j]) || !std::isfinite(dst[j])) return false;
    }
    i += k;
    return true;
  };
  auto integer = [](const char *s, int lo, int hi, int *v) {
    const std::string t = s;
    if (t.empty() || t.size() > 10 || t.find_first_not_of("0123456789") != std::string::npos) return false;
    const long long x = std::atoll(s);
    if (x < lo || x > hi) return false;
    *v = static_cast<int>(x);
    return true;
  };
  for (int i = 3; i < argc; ++i) {
    const std::string a = argv[i];
    const bool more = i + 1 < argc;
    if (a == "--views" && !hasViews && more) {
      viewsFile = argv[++i];
      hasViews = true;
    } else if (a == "--orbit" && !hasOrbit && more) {
      if (!integer(argv[++i], 1, 1024, &orbit)) return usage();
      hasOrbit = true;
    } else if (a == "--size" && !hasSize && i + 2 < argc) {
      for (int k = 0; k < 2; ++k) {
        if (!integer(argv[i + 1 + k], 1, 16384, &size[k])) return usage();
      }
      i += 2;
      hasSize = true;
    } else if (a == "--fov-y" && !hasFov) {
      if (!floats(i, 1, &fovY) || !(fovY > 0.0f && fovY < 180.0f)) return usage();
      hasFov = true;
    } else if (a == "--center" && !hasCenter) {
      if (!floats(i, 3, center.data())) return usage();
      hasCenter = true;
    } else if (a == "--radius" && !hasRadius) {
      if (!floats(i, 1, &radius) || !(radius > 0.0f)) return usage();
      hasRadius = true;
    } else if (a == "--distance" && !hasDistance) {
      if (!floats(i, 1, &distance) || !(distance > 0.0f)) return usage();
      hasDistance = true;
    } else if (a == "--keep" && !o.keepCount && more) {
      int k = 0;
      if (!integer(argv[++i], 0, 0x7fffffff, &k)) return usage();
      o.keepCount = k;
    } else if (a == "--keep-fraction" && !o.keepFraction && more) {
      double f = 0.0;
      if (!parseDouble(argv[++i], &f) || !(f >= 0.0 && f <= 1.0)) return usage();
      o.keepFraction = f;
    } else if (a == "--min-score" && !o.minScore && more) {
      double s = 0.0;
      if (!parseDouble(argv[++i], &s) || !std::isfinite(s)) return usage();
      o.minScore = s;
    } else if (a == "--score" && !hasScore && more) {
      const std::string v = argv[++i];
      if (v == "sum") {
        o.score = spz::PruneOptions::Sum;
      } else if (v == "max") {
        o.score = spz::PruneOptions::Max;
      } else {
        return usage();
      }
      hasScore = true;
    } else if (a == "--coord" && !hasCoord && more) {
      hasCoord = true;
      static const char *names[] = {"UNSPECIFIED", "LDB", "RDB", "LUB", "RUB", "LDF", "RDF", "LUF", "RUF"};
      const std::string c = argv[++i];
      int found = -1;
      for (int k = 0; k < 9; ++k) {
        if (c == names[k]) found = k;
      }
      if (found < 0) return usage();
      o.coord = static_cast<spz::CoordinateSystem>(found);
    } else {
      return usage();
    }
  }
  const int rules = (o.keepCount ? 1 : 0) + (o.keepFraction ? 1 : 0) + (o.minScore ? 1 : 0);
  if (rules != 1 || hasViews == hasOrbit) return usage();
  if (hasViews && (hasSize || hasFov || hasCenter || hasRadius || hasDistance)) return usage();
  if (hasOrbit && (!hasSize || !hasFov || hasCenter != hasRadius)) return usage();
  try {
    if (hasViews) {
      o.views = spz::loadViewsFile(viewsFile);
    } else {
      if (!hasCenter) {  // the box of the decoded positions
        spz::UnpackOptions u;
        u.to = o.coord;
        const spz::GaussianCloud g = spz::loadSpz(std::string(argv[1]), u);
        if (g.numPoints <= 0 || !spz::boundingSphere(g.positions, &center, &radius)) {
          std::cerr << "spz_prune: " << argv[1] << " has no points to take a centre and radius from" << std::endl;
          return 1;
        }
      }
      o.views = spz::orbitViews(orbit, center, radius, size[0], size[1], fovY, distance);
    }
  } catch (const std::invalid_argument &e) {
    std::cerr << e.what() << std::endl;
    return usage();
  }
  int64_t kept = 0;
  if (!spz::pruneSpz(std::string(argv[1]), std::string(argv[2]), o, &kept)) return 1;
  std::cout << "kept " << kept << std::endl;
  return 0;
}

int dispatch(const std::string &tool, int argc, char **argv) {
  if (tool == "ply_to_spz") return plyToSpz(argc, argv);
  if (tool == "spz_to_ply") return spzToPly(argc, argv);
  if (tool == "spz_info") return spzInfo(argc, argv);
  if (tool == "spz_filter") return spzFilter(argc, argv);
  if (tool == "spz_transform") return spzTransform(argc, argv);
  if (tool == "spz_merge") return spzMerge(argc, argv);
  if (tool == "spz_sort") return spzSort(argc, argv);
  if (tool == "spz_decimate") return spzDecimate(argc, argv);
  if (tool == "spz_clean") return spzClean(argc, argv);
  if (tool == "spz_render") return spzRender(argc, argv);
  if (tool == "spz_prune") return spzPrune(argc, argv);
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
    std::cerr << "Usage: spz_tool {ply_to_spz|spz_to_ply|spz_info|spz_filter|spz_transform|spz_merge|spz_sort|spz_decimate|spz_clean|spz_render|spz_prune} <args...>" << std::endl;
    return 1;
  } catch (const std::exception &e) {
    std::cerr << "Error: " << e.what() << std::endl;
    return 1;
  }
}
