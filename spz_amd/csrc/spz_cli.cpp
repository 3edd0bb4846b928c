// spz_cli.cpp — the three command-line tools of the reference (cli_tools/src/*.cpp) over the
// MI355X drop-in layer: ply_to_spz, spz_to_ply, spz_info; and spz_filter (spz::filterSpz),
// spz_transform (spz::transformSpz), spz_merge (spz::mergeSpz), spz_sort (spz::sortSpz), spz_decimate
// (spz::decimateSpz) and spz_clean (spz::cleanSpz), which have no counterpart in the reference.  One binary, dispatched
// on argv[0] (the Makefile installs it under the nine names) or on a first argument naming the tool.
// Same behaviour as the reference mains: default (UNSPECIFIED) pack/unpack options, exit code 0
// once the arguments are there (the reference ignores the save/load results), usage -> 1.
// spz_filter, spz_transform, spz_merge, spz_sort, spz_decimate and spz_clean exit 1 when the filter / transform / merge /
// sort / decimation / clean fails as well.
#include <algorithm>
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
    std::cerr << "Usage: spz_tool {ply_to_spz|spz_to_ply|spz_info|spz_filter|spz_transform|spz_merge|spz_sort|spz_decimate|spz_clean} <args...>" << std::endl;
    return 1;
  } catch (const std::exception &e) {
    std::cerr << "Error: " << e.what() << std::endl;
    return 1;
  }
}
