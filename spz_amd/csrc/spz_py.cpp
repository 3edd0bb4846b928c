// spz_py.cpp — Python module `spz` (imported as spz_amd.spz) over the C++ drop-in layer.
//
// Same surface as the reference's nanobind shim (/root/reference/src/python/spz/spz.cc:110-362):
// CoordinateSystem enum with exported values, PackOptions.from_coord, UnpackOptions.to_coord,
// GaussianCloud with copying float32 array properties and the shim's validation messages,
// load_spz / save_spz / load_splat_from_ply / save_splat_to_ply.  nanobind is not available in
// this image; pybind11 is, so the dtype/ndim gate that nanobind's ndarray caster applies
// (numeric dtypes convert to float32, anything else -> TypeError "incompatible function
// arguments") is written out by hand in `toFloatVector`.
#include <chrono>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <optional>
#include <cstring>
#include <stdexcept>
#include <sstream>
#include <memory>
#include <string>
#include <vector>

#include "spz_amd.h"
#include "spz_amd_host.hpp"
#include "spz_deflate.hpp"
#include "spz_inflate.hpp"

namespace py = pybind11;

namespace {
// The bytes of a Python bytes object, in place (the std::string conversion would copy them: 409 MB for a 10 M-point file).
struct BytesView {
  const uint8_t *p;
  size_t n;
};
BytesView viewOf(const py::bytes &b) {
  char *buf = nullptr;
  Py_ssize_t len = 0;
  if (PyBytes_AsStringAndSize(b.ptr(), &buf, &len) != 0) throw py::error_already_set();
  return {reinterpret_cast<const uint8_t *>(buf), static_cast<size_t>(len)};
}
}  // namespace

namespace {

// Accepts what nb::ndarray<numpy, float, ndim<1>, c_contig, device::cpu> accepts: a 1-D array (or
// array-like) of a bool/int/uint/float dtype, converted to float32.  Everything else is the
// overload-resolution failure nanobind reports.
std::vector<float> toFloatVector(const py::object &obj, const char *prop) {
  auto reject = [&]() {
    throw py::type_error(std::string("__set__(): incompatible function arguments. ") + prop +
                         " expects a 1-D numeric numpy array convertible to float32");
  };
  py::array arr;
  try {
    arr = py::array::ensure(obj);
  } catch (const py::error_already_set &) {
    PyErr_Clear();
  }
  if (!arr) reject();
  const char kind = arr.dtype().kind();
  if (!(kind == 'b' || kind == 'i' || kind == 'u' || kind == 'f')) reject();
  if (arr.ndim() != 1) reject();
  py::array_t<float, py::array::c_style | py::array::forcecast> f(arr);
  std::vector<float> out(static_cast<size_t>(f.size()));
  if (!out.empty()) std::memcpy(out.data(), f.data(), out.size() * sizeof(float));
  return out;
}

// New owning 1-D copy (spz.cc:47-79), of element type E (a mask's bytes: bool).
template <class T, class E = T>
py::array_t<E> toArray(const std::vector<T> &v) {
  static_assert(sizeof(E) == sizeof(T), "a copy of the elements' bytes");
  py::array_t<E> a(static_cast<py::ssize_t>(v.size()));
  if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
  return a;
}

void ensureMultiple(const char *name, size_t size, size_t k) {  // spz.cc:27-37
  if (k == 0) throw py::value_error("internal error: divisor cannot be zero");
  if (size % k != 0) {
    throw py::value_error(std::string(name) + " length must be a multiple of " + std::to_string(k) + ", got " +
                          std::to_string(size));
  }
}

// The product has no CPU fallback: an unusable device is raised, not returned as an empty cloud.
void raiseIfDeviceUnusable() {
  const int st = spz::lastDeviceStatus();
  if (st == SPZ_AMD_ERR_NO_DEVICE || st == SPZ_AMD_ERR_HIP) {
    throw std::runtime_error(std::string("spz_amd: ") + spz_amd_status_string(st) +
                             " (the SPZ hot path runs on the GPU only)");
  }
}

// RenderOptions from render_spz / render_cloud's keyword arguments (the camera itself is checked by the C++ layer).
spz::RenderOptions renderOptions(const py::object &world_to_camera, int width, int height, float fx, float fy, float cx,
                                 float cy, float near_plane, const py::object &background, int max_sh_degree,
                                 spz::CoordinateSystem coord) {
  spz::RenderOptions o;
  py::array_t<float, py::array::c_style | py::array::forcecast> m(world_to_camera);
  if (m.ndim() != 2 || m.shape(0) != 3 || m.shape(1) != 4) throw py::value_error("world_to_camera must be 3x4");
  for (int k = 0; k < 12; ++k) o.worldToCamera[k] = m.data()[k];
  py::array_t<float, py::array::c_style | py::array::forcecast> bg(background);
  if (bg.size() != 3) throw py::value_error("background must have three values");
  for (int k = 0; k < 3; ++k) o.background[k] = bg.data()[k];
  o.width = width;
  o.height = height;
  o.fx = fx;
  o.fy = fy;
  o.cx = cx;
  o.cy = cy;
  o.nearPlane = near_plane;
  o.maxShDegree = max_sh_degree;
  o.coord = coord;
  return o;
}

// The exception of a failed call: the unusable device's RuntimeError; a ValueError `refused` when the call refused its
// arguments (SPZ_AMD_ERR_INVALID_ARG, and SPZ_AMD_ERR_UNSUPPORTED where `unsupportedRefused`); else a RuntimeError `failed`.
[[noreturn]] void raiseFailure(const std::string &refused, const std::string &failed, bool unsupportedRefused = false) {
  raiseIfDeviceUnusable();
  const int st = spz::lastDeviceStatus();
  if (st == SPZ_AMD_ERR_INVALID_ARG || (unsupportedRefused && st == SPZ_AMD_ERR_UNSUPPORTED)) throw py::value_error(refused);
  throw std::runtime_error(failed);
}

// The (height, width, 4) array of a render, or the exception of its failure.
py::object renderedImage(bool ok, const std::vector<float> &img, const spz::RenderOptions &o, const char *what) {
  if (!ok) {
    raiseFailure(std::string(what) + ": refused (see the [SPZ ERROR] line)",
                 std::string(what) + " failed (see the [SPZ ERROR] line)");
  }
  py::array_t<float> out({static_cast<py::ssize_t>(o.height), static_cast<py::ssize_t>(o.width), py::ssize_t(4)});
  std::memcpy(out.mutable_data(), img.data(), img.size() * sizeof(float));
  return out;
}

// The dict of a depth render (each map (height, width); index int32 with -1 for none), or the exception of its failure.
py::object renderedDepth(bool ok, spz::DepthMaps &maps, const spz::RenderOptions &o, const char *what) {
  if (!ok) {
    raiseFailure(std::string(what) + ": refused (see the [SPZ ERROR] line)",
                 std::string(what) + " failed (see the [SPZ ERROR] line)");
  }
  const std::vector<py::ssize_t> shape = {static_cast<py::ssize_t>(o.height), static_cast<py::ssize_t>(o.width)};
  py::dict d;
  const std::pair<const char *, const std::vector<float> *> maps_f[] = {
      {"expected", &maps.expected}, {"median", &maps.median}, {"accumulated", &maps.accumulated}, {"alpha", &maps.alpha}};
  for (const auto &kv : maps_f) {
    py::array_t<float> a(shape);
    std::memcpy(a.mutable_data(), kv.second->data(), kv.second->size() * sizeof(float));
    d[kv.first] = a;
  }
  py::array_t<int32_t> idx(shape);
  std::memcpy(idx.mutable_data(), maps.index.data(), maps.index.size() * sizeof(uint32_t));  // 0xffffffff reads as -1
  d["index"] = idx;
  return d;
}

// A prune view from a mapping with world_to_camera (3x4), fx, fy, cx, cy, width, height (what orbit_views and
// load_3dgs_cameras return); every problem is a ValueError that names the view.
spz::PruneOptions::View pruneView(const py::handle &h, size_t k, spz::CoordinateSystem coord, float near_plane) {
  const std::string at = "view " + std::to_string(k) + ": ";
  if (!py::isinstance<py::dict>(h)) throw py::value_error(at + "must be a dict (world_to_camera, fx, fy, cx, cy, width, height)");
  const py::dict d = py::reinterpret_borrow<py::dict>(h);
  for (const char *key : {"world_to_camera", "fx", "fy", "cx", "cy", "width", "height"}) {
    if (!d.contains(key)) throw py::value_error(at + "has no " + key);
  }
  if (d.contains("coord") && !d["coord"].is_none() && d["coord"].cast<spz::CoordinateSystem>() != coord) {
    throw py::value_error(at + "its coord differs from the prune's coord (every view is in one frame)");
  }
  spz::PruneOptions::View v;
  py::array_t<float, py::array::c_style | py::array::forcecast> m(d["world_to_camera"]);
  if (m.ndim() != 2 || m.shape(0) != 3 || m.shape(1) != 4) throw py::value_error(at + "world_to_camera must be 3x4");
  for (int i = 0; i < 12; ++i) v.worldToCamera[i] = m.data()[i];
  try {
    v.fx = d["fx"].cast<float>();
    v.fy = d["fy"].cast<float>();
    v.cx = d["cx"].cast<float>();
    v.cy = d["cy"].cast<float>();
    v.width = d["width"].cast<int>();
    v.height = d["height"].cast<int>();
  } catch (const py::cast_error &) {
    throw py::value_error(at + "fx, fy, cx, cy must be numbers and width, height ints");
  }
  spz_amd_render_params p = {};
  for (int i = 0; i < 12; ++i) p.world_to_camera[i] = v.worldToCamera[i];
  p.fx = v.fx;
  p.fy = v.fy;
  p.cx = v.cx;
  p.cy = v.cy;
  p.width = static_cast<uint32_t>(v.width < 0 ? 0 : v.width);
  p.height = static_cast<uint32_t>(v.height < 0 ? 0 : v.height);
  p.near_plane = near_plane;
  p.coord = static_cast<int32_t>(coord);
  if (spz_amd_render_check_params(&p) != SPZ_AMD_OK) {
    throw py::value_error(at + "bad camera: world_to_camera must be [R | t] with R a rotation (to 1e-4), fx, fy > 0, "
                               "width and height in 1..16384, near_plane > 0, values finite");
  }
  return v;
}

py::dict viewDict(const spz::PruneOptions::View &v) {
  py::dict d;
  py::array_t<float> m({py::ssize_t(3), py::ssize_t(4)});
  std::memcpy(m.mutable_data(), v.worldToCamera.data(), sizeof(float) * 12);
  d["world_to_camera"] = m;
  d["fx"] = v.fx;
  d["fy"] = v.fy;
  d["cx"] = v.cx;
  d["cy"] = v.cy;
  d["width"] = v.width;
  d["height"] = v.height;
  return d;
}

// compare_spz / compare_images' result of one image pair.
py::dict metricsDict(const spz::ImageMetrics &m) {
  py::dict d;
  d["mse"] = m.mse;
  d["psnr"] = m.psnr;
  d["ssim"] = m.ssim;
  d["l1"] = m.l1;
  d["max_abs"] = m.maxAbs;
  return d;
}

py::array_t<float> mapArray(const std::vector<float> &map, int height, int width) {
  py::array_t<float> out({static_cast<py::ssize_t>(height), static_cast<py::ssize_t>(width)});
  if (!map.empty()) std::memcpy(out.mutable_data(), map.data(), map.size() * sizeof(float));
  return out;
}

// filter_spz's arguments as spz::FilterOptions; every problem is a ValueError, raised before any device work.
spz::FilterOptions filterOptions(const py::object &mask, const py::object &indices, const py::object &box,
                                 spz::CoordinateSystem coord, const py::object &min_alpha, const py::object &sh_degree) {
  spz::FilterOptions f;
  f.coord = coord;
  if (!sh_degree.is_none()) {
    if (!py::isinstance<py::int_>(sh_degree) || py::isinstance<py::bool_>(sh_degree)) throw py::value_error("sh_degree must be None or an int in [-1, 3]");
    const long d = py::cast<long>(sh_degree);
    if (d < -1 || d > 3) throw py::value_error("sh_degree must be None or an int in [-1, 3], got " + std::to_string(d));
    f.shDegree = static_cast<int32_t>(d);
  }
  if (!indices.is_none() && (!mask.is_none() || !box.is_none() || !min_alpha.is_none())) {
    throw py::value_error("indices cannot be combined with mask, box or min_alpha");
  }
  auto asArray = [](const py::object &o, const char *name) {
    py::array a;
    try {
      a = py::array::ensure(o);
    } catch (const py::error_already_set &) {
      PyErr_Clear();
    }
    if (!a) throw py::value_error(std::string(name) + " must be a numpy array");
    return a;
  };
  if (!box.is_none()) {
    py::array a = asArray(box, "box");
    const char k = a.dtype().kind();
    if (!(k == 'i' || k == 'u' || k == 'f')) throw py::value_error("box must be numeric");
    if (a.ndim() != 2 || a.shape(0) != 2 || a.shape(1) != 3) throw py::value_error("box must have shape (2, 3): [[x0, y0, z0], [x1, y1, z1]]");
    py::array_t<float, py::array::c_style | py::array::forcecast> b(a);
    spz::FilterOptions::Box bb;
    for (int i = 0; i < 3; ++i) {
      bb.lo[i] = b.at(0, i);
      bb.hi[i] = b.at(1, i);
      if (std::isnan(bb.lo[i]) || std::isnan(bb.hi[i])) throw py::value_error("box bounds must not be NaN");
    }
    f.box = bb;
  }
  if (!min_alpha.is_none()) {
    const float v = py::cast<float>(min_alpha);
    if (std::isnan(v)) throw py::value_error("min_alpha must not be NaN");
    f.minAlpha = v;
  }
  if (!mask.is_none()) {
    py::array a = asArray(mask, "mask");
    const char k = a.dtype().kind();
    if (!(k == 'b' || k == 'i' || k == 'u')) throw py::value_error("mask must be a bool or integer array");
    if (a.ndim() != 1) throw py::value_error("mask must be one-dimensional");
    py::array_t<bool, py::array::c_style | py::array::forcecast> b(a);
    std::vector<uint8_t> v(static_cast<size_t>(b.size()));
    const bool *q = b.data();
    for (size_t i = 0; i < v.size(); ++i) v[i] = q[i] ? 1 : 0;
    f.mask = std::move(v);
  }
  if (!indices.is_none()) {
    py::array a = asArray(indices, "indices");
    const char k = a.dtype().kind();
    if (!(k == 'i' || k == 'u')) throw py::value_error("indices must be an integer array");
    if (a.ndim() != 1) throw py::value_error("indices must be one-dimensional");
    if (static_cast<uint64_t>(a.size()) > SPZ_AMD_REFERENCE_MAX_POINTS) throw py::value_error("more than 10 M indices: the reference reads at most 10 M points");
    std::vector<uint32_t> v(static_cast<size_t>(a.size()));
    if (k == 'u') {
      py::array_t<uint64_t, py::array::c_style | py::array::forcecast> b(a);
      for (size_t i = 0; i < v.size(); ++i) {
        if (b.data()[i] > 0xffffffffull) throw py::value_error("index " + std::to_string(b.data()[i]) + " does not fit 32 bits");
        v[i] = static_cast<uint32_t>(b.data()[i]);
      }
    } else {
      py::array_t<int64_t, py::array::c_style | py::array::forcecast> b(a);
      for (size_t i = 0; i < v.size(); ++i) {
        const int64_t x = b.data()[i];
        if (x < 0) throw py::value_error("negative index " + std::to_string(x));
        if (x > 0xffffffffll) throw py::value_error("index " + std::to_string(x) + " does not fit 32 bits");
        v[i] = static_cast<uint32_t>(x);
      }
    }
    f.indices = std::move(v);
  }
  return f;
}

// transform_spz / transform_cloud's arguments as spz::TransformOptions; every problem is a ValueError, raised before any
// device work (the parameter block is built on the host, spz_amd_transform_params).
spz::TransformOptions transformOptions(const py::object &rotation, const py::object &translation, const py::object &scale,
                                       spz::CoordinateSystem coord, const py::object &fractional_bits) {
  spz::TransformOptions o;
  o.coord = coord;
  auto vec = [](const py::object &v, size_t n, const char *name) {
    const std::string what = std::string(name) + " must be a sequence of " + std::to_string(n) + " finite numbers";
    py::array a;
    try {
      a = py::array::ensure(v);
    } catch (const py::error_already_set &) {
      PyErr_Clear();
    }
    if (!a) throw py::value_error(what);
    const char k = a.dtype().kind();
    if (!(k == 'i' || k == 'u' || k == 'f') || a.ndim() != 1 || static_cast<size_t>(a.size()) != n) throw py::value_error(what);
    py::array_t<double, py::array::c_style | py::array::forcecast> d(a);
    std::vector<double> out(d.data(), d.data() + n);
    for (double x : out) {
      if (!std::isfinite(x)) throw py::value_error(what);
    }
    return out;
  };
  if (!rotation.is_none()) {
    const std::vector<double> q = vec(rotation, 4, "rotation (x, y, z, w)");
    std::copy(q.begin(), q.end(), o.rotation.begin());
    if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0) throw py::value_error("rotation must not be zero");
  }
  if (!translation.is_none()) {
    const std::vector<double> t = vec(translation, 3, "translation (x, y, z)");
    std::copy(t.begin(), t.end(), o.translation.begin());
  }
  if (py::isinstance<py::bool_>(scale) || !(py::isinstance<py::int_>(scale) || py::isinstance<py::float_>(scale))) {
    throw py::value_error("scale must be a number");
  }
  o.scale = py::cast<double>(scale);
  if (!std::isfinite(o.scale) || !(o.scale > 0.0)) throw py::value_error("scale must be finite and > 0");
  if (!py::isinstance<py::int_>(fractional_bits) || py::isinstance<py::bool_>(fractional_bits)) {
    throw py::value_error("fractional_bits must be an int in [0, 24]");
  }
  const long fb = py::cast<long>(fractional_bits);
  if (fb < 0 || fb > 24) throw py::value_error("fractional_bits must be an int in [0, 24], got " + std::to_string(fb));
  o.fractionalBits = static_cast<int32_t>(fb);
  spz_amd_transform xf;
  if (spz_amd_transform_params(o.rotation.data(), o.translation.data(), o.scale, static_cast<int>(coord), &xf) != SPZ_AMD_OK) {
    throw py::value_error("the transform has no f32 parameter block (scale or translation out of the f32 range?)");
  }
  return o;
}

// merge_spz's arguments as spz::MergeOptions; every problem is a ValueError, raised before any device work.  Each
// transforms entry is None or a dict of rotation / translation / scale / coord, checked by transform_spz's code.
spz::MergeOptions mergeOptions(size_t k, const py::object &transforms, const py::object &sh_degree,
                               const py::object &fractional_bits, const py::object &antialiased) {
  spz::MergeOptions o;
  auto opt = [](const py::object &v, long lo, long hi, const char *name) -> int32_t {
    if (v.is_none()) return -1;
    if (!py::isinstance<py::int_>(v) || py::isinstance<py::bool_>(v)) {
      throw py::value_error(std::string(name) + " must be None or an int in [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
    }
    const long d = py::cast<long>(v);
    if (d < lo || d > hi) {
      throw py::value_error(std::string(name) + " must be None or an int in [" + std::to_string(lo) + ", " + std::to_string(hi) +
                            "], got " + std::to_string(d));
    }
    return static_cast<int32_t>(d);
  };
  o.shDegree = opt(sh_degree, 0, 3, "sh_degree");
  o.fractionalBits = opt(fractional_bits, 0, 24, "fractional_bits");
  o.antialiased = opt(antialiased, 0, 1, "antialiased");
  if (k == 0) throw py::value_error("merge_spz: no inputs");
  if (k > SPZ_AMD_MERGE_MAX_INPUTS) {
    throw py::value_error("merge_spz: " + std::to_string(k) + " inputs, at most " + std::to_string(SPZ_AMD_MERGE_MAX_INPUTS));
  }
  if (transforms.is_none()) return o;
  if (!py::isinstance<py::sequence>(transforms) || py::isinstance<py::str>(transforms)) {
    throw py::value_error("transforms must be None or a list with one entry per input");
  }
  const py::sequence seq = transforms.cast<py::sequence>();
  if (static_cast<size_t>(py::len(seq)) != k) {
    throw py::value_error("transforms has " + std::to_string(py::len(seq)) + " entries for " + std::to_string(k) + " inputs");
  }
  for (size_t i = 0; i < k; ++i) {
    const py::object e = seq[i];
    if (e.is_none()) {
      o.transforms.emplace_back(std::nullopt);
      continue;
    }
    if (!py::isinstance<py::dict>(e)) throw py::value_error("transforms[" + std::to_string(i) + "] must be None or a dict");
    const py::dict d = e.cast<py::dict>();
    for (const auto &kv : d) {
      const std::string key = py::str(kv.first);
      if (key != "rotation" && key != "translation" && key != "scale" && key != "coord") {
        throw py::value_error("transforms[" + std::to_string(i) + "]: unknown key '" + key + "'");
      }
    }
    spz::CoordinateSystem coord = spz::CoordinateSystem::UNSPECIFIED;
    if (d.contains("coord")) {
      const py::object c = d["coord"];
      if (py::isinstance<spz::CoordinateSystem>(c)) {
        coord = c.cast<spz::CoordinateSystem>();
      } else if (py::isinstance<py::int_>(c) && !py::isinstance<py::bool_>(c) && py::cast<long>(c) >= 0 && py::cast<long>(c) <= 8) {
        coord = static_cast<spz::CoordinateSystem>(py::cast<long>(c));
      } else {
        throw py::value_error("transforms[" + std::to_string(i) + "]: coord must be a CoordinateSystem");
      }
    }
    const py::object none = py::none();
    o.transforms.emplace_back(transformOptions(d.contains("rotation") ? py::object(d["rotation"]) : none,
                                               d.contains("translation") ? py::object(d["translation"]) : none,
                                               d.contains("scale") ? py::object(d["scale"]) : py::object(py::float_(1.0)),
                                               coord, py::int_(12)));
  }
  return o;
}

}  // namespace

namespace {
py::dict tilesetToDict(const spz::Tileset &t) {
  py::dict d;
  d["format"] = "spz-tileset";
  d["version"] = 1;
  d["coord"] = t.coord;
  d["num_points"] = t.numPoints;
  d["sh_degree"] = t.shDegree;
  d["fractional_bits"] = t.fractionalBits;
  d["max_points"] = t.maxPoints;
  py::list tiles;
  for (const spz::Tile &k : t.tiles) {
    py::dict e;
    e["id"] = k.id;
    e["file"] = k.file;
    e["parent"] = k.parent;
    e["children"] = k.children;
    e["level"] = k.level;
    e["cell"] = py::make_tuple(k.cell[0], k.cell[1], k.cell[2]);
    e["content_level"] = k.contentLevel;
    e["num_points"] = k.numPoints;
    e["geometric_error"] = k.geometricError;
    e["box"] = py::make_tuple(py::make_tuple(k.boxMin[0], k.boxMin[1], k.boxMin[2]),
                              py::make_tuple(k.boxMax[0], k.boxMax[1], k.boxMax[2]));
    e["max_radius"] = k.maxRadius;
    tiles.append(e);
  }
  d["tiles"] = tiles;
  return d;
}

spz::Tileset tilesetFromDict(const py::dict &d) {
  spz::Tileset t;
  try {
    t.coord = py::cast<spz::CoordinateSystem>(d["coord"]);
    t.numPoints = py::cast<uint64_t>(d["num_points"]);
    t.shDegree = py::cast<int>(d["sh_degree"]);
    t.fractionalBits = py::cast<int>(d["fractional_bits"]);
    t.maxPoints = py::cast<uint32_t>(d["max_points"]);
    for (const py::handle &h : py::cast<py::list>(d["tiles"])) {
      const py::dict e = py::cast<py::dict>(h);
      spz::Tile k;
      k.id = py::cast<uint32_t>(e["id"]);
      k.file = py::cast<std::string>(e["file"]);
      k.parent = py::cast<int32_t>(e["parent"]);
      k.children = py::cast<std::vector<uint32_t>>(e["children"]);
      k.level = py::cast<int32_t>(e["level"]);
      k.cell = py::cast<std::array<uint32_t, 3>>(e["cell"]);
      k.contentLevel = py::cast<int32_t>(e["content_level"]);
      k.numPoints = py::cast<uint32_t>(e["num_points"]);
      k.geometricError = py::cast<float>(e["geometric_error"]);
      const auto box = py::cast<std::array<std::array<float, 3>, 2>>(e["box"]);
      k.boxMin = box[0];
      k.boxMax = box[1];
      k.maxRadius = py::cast<float>(e["max_radius"]);
      if (k.id != t.tiles.size()) throw py::value_error("tile ids must count from 0");
      for (const uint32_t c : k.children) {
        if (c <= k.id) throw py::value_error("a child's id must be above its parent's");
      }
      t.tiles.push_back(std::move(k));
    }
    for (const spz::Tile &k : t.tiles) {
      for (const uint32_t c : k.children) {
        if (c >= t.tiles.size()) throw py::value_error("a child id is out of range");
      }
    }
  } catch (const py::cast_error &) {
    throw py::value_error("not a tileset dict (see load_tileset)");
  } catch (const py::error_already_set &) {
    throw py::value_error("not a tileset dict (see load_tileset)");
  }
  return t;
}
}  // namespace

PYBIND11_MODULE(spz, m) {
  m.doc() = "MI355X-native drop-in for the `spz` Python bindings (Gaussian splat .spz codec).";

  py::enum_<spz::CoordinateSystem>(m, "CoordinateSystem",
                                   "Axis conventions: Right/Left, Up/Down, Front/Back (RDF = PLY, RUB = three.js, "
                                   "LUF = glTF, RUF = Unity).")
      .value("UNSPECIFIED", spz::CoordinateSystem::UNSPECIFIED)
      .value("LDB", spz::CoordinateSystem::LDB)
      .value("RDB", spz::CoordinateSystem::RDB)
      .value("LUB", spz::CoordinateSystem::LUB)
      .value("RUB", spz::CoordinateSystem::RUB)
      .value("LDF", spz::CoordinateSystem::LDF)
      .value("RDF", spz::CoordinateSystem::RDF)
      .value("LUF", spz::CoordinateSystem::LUF)
      .value("RUF", spz::CoordinateSystem::RUF)
      .export_values();

  py::class_<spz::PackOptions>(m, "PackOptions")
      .def(py::init<>())
      .def_readwrite("from_coord", &spz::PackOptions::from, "Coordinate system of the input splat");
  py::class_<spz::UnpackOptions>(m, "UnpackOptions")
      .def(py::init<>())
      .def_readwrite("to_coord", &spz::UnpackOptions::to, "Desired coordinate system of the output splat");

  using Cloud = spz::GaussianCloud;
  py::class_<Cloud>(m, "GaussianCloud")
      .def(py::init<>(), "Construct an empty GaussianCloud.")
      .def_property_readonly("num_points",
                             [](const Cloud &c) { return static_cast<int32_t>(c.positions.size() / 3); })
      .def("__len__", [](const Cloud &c) { return static_cast<int32_t>(c.positions.size() / 3); })
      .def("__repr__",
           [](const Cloud &c) {
             return py::str("GaussianCloud(num_points={}, sh_degree={}, antialiased={})")
                 .format(static_cast<int32_t>(c.positions.size() / 3), c.shDegree, c.antialiased);
           })
      .def_property(
          "sh_degree", [](const Cloud &c) { return c.shDegree; },
          [](Cloud &c, int32_t deg) {
            if (deg < 0 || deg > 3) throw py::value_error("sh_degree must be in [0, 3]");
            c.shDegree = deg;
          })
      .def_readwrite("antialiased", &Cloud::antialiased)
      .def_property(
          "positions", [](const Cloud &c) { return toArray(c.positions); },
          [](Cloud &c, const py::object &o) {
            std::vector<float> v = toFloatVector(o, "positions");
            ensureMultiple("positions", v.size(), 3);
            c.positions = std::move(v);
            c.numPoints = static_cast<int32_t>(c.positions.size() / 3);  // positions define num_points
          })
      .def_property(
          "scales", [](const Cloud &c) { return toArray(c.scales); },
          [](Cloud &c, const py::object &o) {
            std::vector<float> v = toFloatVector(o, "scales");
            ensureMultiple("scales", v.size(), 3);
            c.scales = std::move(v);
            if (c.numPoints > 0 && c.scales.size() != static_cast<size_t>(c.numPoints) * 3) {
              throw py::value_error("scales length must equal num_points * 3");
            }
          })
      .def_property(
          "rotations", [](const Cloud &c) { return toArray(c.rotations); },
          [](Cloud &c, const py::object &o) {
            std::vector<float> v = toFloatVector(o, "rotations");
            ensureMultiple("rotations", v.size(), 4);
            c.rotations = std::move(v);
            if (c.numPoints > 0 && c.rotations.size() != static_cast<size_t>(c.numPoints) * 4) {
              throw py::value_error("rotations length must equal num_points * 4");
            }
          })
      .def_property(
          "alphas", [](const Cloud &c) { return toArray(c.alphas); },
          [](Cloud &c, const py::object &o) {
            c.alphas = toFloatVector(o, "alphas");
            if (c.numPoints > 0 && c.alphas.size() != static_cast<size_t>(c.numPoints)) {
              throw py::value_error("alphas length must equal num_points");
            }
          })
      .def_property(
          "colors", [](const Cloud &c) { return toArray(c.colors); },
          [](Cloud &c, const py::object &o) {
            std::vector<float> v = toFloatVector(o, "colors");
            ensureMultiple("colors", v.size(), 3);
            c.colors = std::move(v);
            if (c.numPoints > 0 && c.colors.size() != static_cast<size_t>(c.numPoints) * 3) {
              throw py::value_error("colors length must equal num_points * 3");
            }
          })
      .def_property(
          "sh", [](const Cloud &c) { return toArray(c.sh); },
          [](Cloud &c, const py::object &o) {
            std::vector<float> v = toFloatVector(o, "sh");
            ensureMultiple("sh", v.size(), 3);
            const int deg = c.shDegree;
            const size_t perChannel = (deg == 0) ? 0 : static_cast<size_t>((deg + 1) * (deg + 1) - 1);
            if (perChannel == 0) {
              if (!v.empty()) throw py::value_error("sh must be empty when sh_degree == 0");
            } else {
              ensureMultiple("sh", v.size(), perChannel * 3);
            }
            c.sh = std::move(v);
            if (c.numPoints > 0 && c.sh.size() != static_cast<size_t>(c.numPoints) * perChannel * 3) {
              throw py::value_error("sh length must equal num_points * ((sh_degree+1)^2 - 1) * 3");
            }
          })
      .def("convert_coordinates",
           [](Cloud &c, spz::CoordinateSystem from, spz::CoordinateSystem to) {
             c.convertCoordinates(from, to);
             if (c.numPoints) raiseIfDeviceUnusable();
           },
           py::arg("from_coord"), py::arg("to_coord"), "Convert between two coordinate systems in-place.")
      .def("rotate_180_deg_about_x",
           [](Cloud &c) {
             c.rotate180DegAboutX();
             if (c.numPoints) raiseIfDeviceUnusable();
           },
           "RUB <-> RDF conversion (180 degrees about X).")
      .def("median_volume", [](const Cloud &c) {
             spz::setLastDeviceStatus(SPZ_AMD_OK);
             const float v = c.medianVolume();   // selection runs on the device
             raiseIfDeviceUnusable();
             return v;
           }, "Return the median Gaussian volume.");

  // Device-resident packed load (an extra of this implementation): the stream stays in HBM.
  py::class_<spz::DevicePackedGaussians>(m, "DevicePackedGaussians",
                                         "A .spz file's packed sections left in device memory (spz::loadSpzPackedDevice). "
                                         "Pointers are device addresses (ints); the object owns the memory until release().")
      .def_readonly("num_points", &spz::DevicePackedGaussians::numPoints)
      .def_readonly("sh_degree", &spz::DevicePackedGaussians::shDegree)
      .def_readonly("fractional_bits", &spz::DevicePackedGaussians::fractionalBits)
      .def_readonly("antialiased", &spz::DevicePackedGaussians::antialiased)
      .def_readonly("version", &spz::DevicePackedGaussians::version)
      .def_readonly("uses_quaternion_smallest_three", &spz::DevicePackedGaussians::usesQuaternionSmallestThree)
      .def_readonly("device", &spz::DevicePackedGaussians::device)
      .def_readonly("inflated_on_device", &spz::DevicePackedGaussians::inflatedOnDevice)
      .def_property_readonly("uses_float16", [](const spz::DevicePackedGaussians &d) { return d.usesFloat16(); })
      .def_property_readonly("valid", [](const spz::DevicePackedGaussians &d) { return d.valid(); })
      .def_property_readonly("stream_ptr", [](const spz::DevicePackedGaussians &d) { return reinterpret_cast<uintptr_t>(d.stream); })
      .def_property_readonly("stream_bytes", [](const spz::DevicePackedGaussians &d) { return d.streamBytes; })
      .def_property_readonly("sections", [](const spz::DevicePackedGaussians &d) {
             py::dict r;
             auto put = [&](const char *name, const uint8_t *p, size_t n) { r[name] = py::make_tuple(reinterpret_cast<uintptr_t>(p), n); };
             put("positions", d.positions, d.positionsBytes);
             put("alphas", d.alphas, d.alphasBytes);
             put("colors", d.colors, d.colorsBytes);
             put("scales", d.scales, d.scalesBytes);
             put("rotations", d.rotations, d.rotationsBytes);
             put("sh", d.sh, d.shBytes);
             return r;
           }, "name -> (device address, bytes) of the six sections, in PackedGaussians' naming.")
      .def("release", &spz::DevicePackedGaussians::release, "Return the device memory; the object becomes empty.")
      .def("unpack", [](const spz::DevicePackedGaussians &d, const spz::UnpackOptions &o) {
             spz::GaussianCloud g;
             {
               py::gil_scoped_release release;
               g = d.unpack(o);
             }
             if (g.numPoints == 0) raiseIfDeviceUnusable();
             return g;
           }, py::arg("options") = spz::UnpackOptions(), "unpackGaussians of all points, from where the stream lies.")
      .def("unpack_indices", [](const spz::DevicePackedGaussians &d, const std::vector<uint32_t> &indices, const spz::UnpackOptions &o) {
             spz::GaussianCloud g = d.unpackIndices(indices, o);
             if (g.numPoints == 0 && !indices.empty()) raiseIfDeviceUnusable();
             return g;
           }, py::arg("indices"), py::arg("options") = spz::UnpackOptions(), "One gather launch over the resident stream.");
  m.def("load_spz_packed_device", [](const std::string &filename) {
          spz::DevicePackedGaussians d;
          {
            py::gil_scoped_release release;
            d = spz::loadSpzPackedDevice(filename);
          }
          if (!d.valid()) raiseIfDeviceUnusable();
          return d;
        }, py::arg("filename"), "loadSpzPacked with the packed sections left in device memory.");
  m.def("_load_spz_packed_device_bytes", [](const py::bytes &data) {
          const BytesView in = viewOf(data);
          spz::DevicePackedGaussians d = spz::loadSpzPackedDevice(in.p, static_cast<int32_t>(in.n));
          if (!d.valid()) raiseIfDeviceUnusable();
          return d;
        }, py::arg("data"), "The same from .spz bytes in memory.");

  m.def("load_spz",
        [](const std::string &filename, const spz::UnpackOptions &o) {
          spz::GaussianCloud g;
          {
            py::gil_scoped_release release;  // other Python threads run meanwhile (the library is re-entrant)
            g = spz::loadSpz(filename, o);
          }
          if (g.numPoints == 0) raiseIfDeviceUnusable();
          return g;
        },
        py::arg("filename"), py::arg("options") = spz::UnpackOptions(), "Load a *.spz* file and return a GaussianCloud.");
  m.def("filter_spz",
        [](const std::string &input, const std::string &output, const py::object &mask, const py::object &indices,
           const py::object &box, spz::CoordinateSystem coord, const py::object &min_alpha, const py::object &sh_degree) {
          const spz::FilterOptions f = filterOptions(mask, indices, box, coord, min_alpha, sh_degree);
          int64_t kept = 0;
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::filterSpz(input, output, f, &kept);
          }
          if (!ok) {
            raiseFailure("filter_spz: invalid argument for this file (see the [SPZ ERROR] line)",
                         "filter_spz: " + input + " -> " + output + " failed (see the [SPZ ERROR] line)");
          }
          return kept;
        },
        py::arg("input_filename"), py::arg("output_filename"), py::kw_only(), py::arg("mask") = py::none(),
        py::arg("indices") = py::none(), py::arg("box") = py::none(), py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        py::arg("min_alpha") = py::none(), py::arg("sh_degree") = py::none(),
        "A smaller .spz out of an existing one without requantising (spz::filterSpz): the points `indices`, or those "
        "selected by mask / box (inclusive, positions in `coord`) / min_alpha (decoded logit), with sh lowered to "
        "`sh_degree`.  Returns the number of points kept.");
  m.def("transform_spz",
        [](const std::string &input, const std::string &output, const py::object &rotation, const py::object &translation,
           const py::object &scale, spz::CoordinateSystem coord, const py::object &fractional_bits) {
          const spz::TransformOptions o = transformOptions(rotation, translation, scale, coord, fractional_bits);
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::transformSpz(input, output, o);
          }
          if (!ok) {
            raiseFailure("transform_spz: refused for this file (see the [SPZ ERROR] line)",
                         "transform_spz: " + input + " -> " + output + " failed (see the [SPZ ERROR] line)");
          }
        },
        py::arg("input_filename"), py::arg("output_filename"), py::kw_only(), py::arg("rotation") = py::none(),
        py::arg("translation") = py::none(), py::arg("scale") = 1.0, py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        py::arg("fractional_bits") = 12,
        "Place a scene (spz::transformSpz): p -> scale * R(rotation) * p + translation, stated in `coord`, with the "
        "rotation applied to the quaternions and the sh bands; rotation is (x, y, z, w).  The output is a v3 file with "
        "positions at `fractional_bits`; a position that does not fit is refused (ValueError).");
  m.def("transform_cloud",
        [](spz::GaussianCloud &g, const py::object &rotation, const py::object &translation, const py::object &scale,
           spz::CoordinateSystem coord) {
          const spz::TransformOptions o = transformOptions(rotation, translation, scale, coord, py::int_(12));
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::transformCloud(g, o);
          }
          if (!ok) raiseFailure("transform_cloud: the cloud's arrays do not match", "transform_cloud failed (see the [SPZ ERROR] line)");
        },
        py::arg("cloud"), py::kw_only(), py::arg("rotation") = py::none(), py::arg("translation") = py::none(),
        py::arg("scale") = 1.0, py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        "transform_spz's transform in place on a GaussianCloud (spz::transformCloud), in f32 without quantising.");
  m.def("merge_spz",
        [](const std::vector<std::string> &inputs, const std::string &output, const py::object &transforms,
           const py::object &sh_degree, const py::object &fractional_bits, const py::object &antialiased) {
          const spz::MergeOptions o = mergeOptions(inputs.size(), transforms, sh_degree, fractional_bits, antialiased);
          bool ok;
          int64_t points = 0;
          {
            py::gil_scoped_release release;
            ok = spz::mergeSpz(inputs, output, o, &points);
          }
          if (!ok) {
            raiseFailure("merge_spz: refused for these files (see the [SPZ ERROR] line)",
                         "merge_spz: -> " + output + " failed (see the [SPZ ERROR] line)");
          }
          return points;
        },
        py::arg("inputs"), py::arg("output_filename"), py::kw_only(), py::arg("transforms") = py::none(),
        py::arg("sh_degree") = py::none(), py::arg("fractional_bits") = py::none(), py::arg("antialiased") = py::none(),
        "One v3 .spz out of several (spz::mergeSpz): input 0's points, then input 1's, ...; bytes are copied wherever the "
        "encoding and the placement allow.  transforms: None or one entry per input, None or a dict of rotation / "
        "translation / scale / coord (as transform_spz).  sh_degree (None: the largest), fractional_bits (None: the "
        "inputs' common value, else 12), antialiased (None: the inputs must agree).  Returns the number of points.");
  m.def("sort_spz",
        [](const std::string &input, const std::string &output, const py::object &keys, const py::object &descending) {
          // the arguments first: every problem is a ValueError before any device work
          spz::SortOptions o;
          if (!py::isinstance<py::bool_>(descending)) throw py::value_error("descending must be a bool");
          o.descending = py::cast<bool>(descending);
          if (!keys.is_none()) {
            if (!py::isinstance<py::array>(keys)) throw py::value_error("keys must be a 1-D float32 numpy array");
            py::array a = py::reinterpret_borrow<py::array>(keys);
            if (!a.dtype().is(py::dtype::of<float>()) || a.ndim() != 1) {
              throw py::value_error("keys must be a 1-D float32 numpy array");
            }
            py::array_t<float, py::array::c_style> k(a);  // a copy only when `a` is strided
            o.keys = std::vector<float>(k.data(), k.data() + k.size());
          }
          std::vector<uint32_t> order;
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::sortSpz(input, output, o, &order);
          }
          if (!ok) {
            raiseFailure("sort_spz: refused for this file (see the [SPZ ERROR] line)",
                         "sort_spz: " + input + " -> " + output + " failed (see the [SPZ ERROR] line)", true);
          }
          return toArray(order);
        },
        py::arg("input_filename"), py::arg("output_filename"), py::kw_only(), py::arg("keys") = py::none(),
        py::arg("descending") = false,
        "The same points in a new order without requantising (spz::sortSpz): by `keys` (a 1-D float32 array, one per "
        "point; numpy's argsort(kind='stable') order, NaN last), or by the Morton key of the stored positions; ties keep "
        "input order.  Returns the order (uint32): output point k is input point order[k].");
  m.def("decimate_spz",
        [](const std::string &input, const std::string &output, const py::object &level, const py::object &target,
           const py::object &return_parents) -> py::object {
          // the arguments first: every problem is a ValueError before any device work
          auto is_int = [](const py::object &v) { return py::isinstance<py::int_>(v) && !py::isinstance<py::bool_>(v); };
          if (!py::isinstance<py::bool_>(return_parents)) throw py::value_error("return_parents must be a bool");
          if (level.is_none() == target.is_none()) throw py::value_error("give exactly one of level and target_points");
          spz::DecimateOptions o;
          if (!level.is_none()) {
            if (!is_int(level)) throw py::value_error("level must be an int in 0..24");
            const long long v = py::cast<long long>(level);
            if (v < 0 || v > 24) throw py::value_error("level must be an int in 0..24");
            o.level = static_cast<int>(v);
          } else {
            if (!is_int(target)) throw py::value_error("target_points must be an int >= 1");
            const py::int_ t = py::reinterpret_borrow<py::int_>(target);
            if (t < py::int_(1) || t > py::int_(UINT64_MAX)) throw py::value_error("target_points must be an int >= 1");
            o.targetPoints = py::cast<uint64_t>(t);
          }
          const bool want_parents = py::cast<bool>(return_parents);
          std::vector<uint32_t> parents;
          int used = -1;
          int64_t points = 0;
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::decimateSpz(input, output, o, want_parents ? &parents : nullptr, &used, &points);
          }
          if (!ok) {
            raiseFailure("decimate_spz: refused for this file (see the [SPZ ERROR] line)",
                         "decimate_spz: " + input + " -> " + output + " failed (see the [SPZ ERROR] line)", true);
          }
          if (!want_parents) return py::make_tuple(used, points);
          return py::make_tuple(used, points, toArray(parents));
        },
        py::arg("input_filename"), py::arg("output_filename"), py::kw_only(), py::arg("level") = py::none(),
        py::arg("target_points") = py::none(), py::arg("return_parents") = false,
        "A coarser version of a v2/v3 file (spz::decimateSpz): one point per occupied octree cell of edge 2^level "
        "quanta, in Morton order; a cell of several points becomes one Gaussian matching their moments.  Exactly one "
        "of level (0..24) and target_points (>= 1: the smallest level with at most that many cells).  Returns (level, "
        "points), plus parents (uint32: the output index of every input point's cell) when return_parents.");
  m.def("tile_spz",
        [](const std::string &input, const std::string &out_dir, const py::object &max_points, const py::object &max_tiles,
           spz::CoordinateSystem coord) -> py::object {
          auto is_int = [](const py::object &v) { return py::isinstance<py::int_>(v) && !py::isinstance<py::bool_>(v); };
          if (!is_int(max_points) || py::int_(max_points) < py::int_(1) || py::int_(max_points) > py::int_(10000000)) {
            throw py::value_error("max_points must be an int in 1..10000000");
          }
          if (!is_int(max_tiles) || py::int_(max_tiles) < py::int_(1) || py::int_(max_tiles) > py::int_(2147483647)) {
            throw py::value_error("max_tiles must be an int in 1..2^31 - 1");
          }
          spz::TileOptions o;
          o.maxPoints = py::cast<uint32_t>(max_points);
          o.maxTiles = py::cast<uint32_t>(max_tiles);
          o.coord = coord;
          spz::Tileset t;
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::tileSpz(input, out_dir, o, &t);
          }
          if (!ok) {
            raiseFailure("tile_spz: refused (see the [SPZ ERROR] line)",
                         "tile_spz: " + input + " -> " + out_dir + " failed (see the [SPZ ERROR] line)", true);
          }
          return tilesetToDict(t);
        },
        py::arg("input_filename"), py::arg("out_dir"), py::kw_only(), py::arg("max_points"),
        py::arg("max_tiles") = 65536, py::arg("coord") = spz::CoordinateSystem::RUB,
        "Cut a v2/v3 file into an octree of level-of-detail tiles (spz::tileSpz): out_dir/tile_%06u.spz per tile and "
        "out_dir/tileset.json; out_dir must be absent or empty.  Returns the tileset as load_tileset does.");
  m.def("load_tileset",
        [](const std::string &path) -> py::object {
          spz::Tileset t;
          if (!spz::loadTileset(path, &t)) throw py::value_error("load_tileset: " + path + " is not a readable tileset.json");
          return tilesetToDict(t);
        },
        py::arg("path"), "A tileset.json as a dict: format fields and `tiles`, a list of dicts (spz::loadTileset).");
  m.def("save_tileset",
        [](const py::dict &tileset, const std::string &path) {
          if (!spz::saveTileset(tilesetFromDict(tileset), path)) throw std::runtime_error("save_tileset: unable to write " + path);
        },
        py::arg("tileset"), py::arg("path"), "Write a tileset dict as tileset.json (spz::saveTileset).");
  m.def("select_tiles",
        [](const py::dict &tileset, const py::object &world_to_camera, float fx, float fy, double max_pixel_error,
           double near_plane) -> py::object {
          const std::vector<float> m = py::cast<std::vector<float>>(
              py::module_::import("numpy").attr("asarray")(world_to_camera).attr("reshape")(-1).attr("tolist")());
          if (m.size() != 12) throw py::value_error("world_to_camera must hold 12 values ([R | t] row-major)");
          if (!(max_pixel_error >= 0.0) || !(near_plane > 0.0) || !(fx > 0.0f) || !(fy > 0.0f)) {
            throw py::value_error("max_pixel_error must be >= 0, near_plane, fx and fy > 0");
          }
          spz::PruneOptions::View v;
          for (int i = 0; i < 12; ++i) v.worldToCamera[i] = m[i];
          v.fx = fx;
          v.fy = fy;
          return py::cast(spz::selectTiles(tilesetFromDict(tileset), v, max_pixel_error, near_plane));
        },
        py::arg("tileset"), py::arg("world_to_camera"), py::arg("fx"), py::arg("fy"), py::arg("max_pixel_error"),
        py::arg("near_plane") = 0.2,
        "The screen-space-error cut through a tileset (spz::selectTiles, float64): the tile ids to draw, in tile order.");
  m.def("render_spz",
        [](const py::object &input, const py::object &world_to_camera, int width, int height, float fx, float fy,
           float cx, float cy, float near_plane, const py::object &background, int max_sh_degree,
           spz::CoordinateSystem coord) -> py::object {
          // renderSpz checks the camera before it reads the file: a bad one is a ValueError before any device work
          const spz::RenderOptions o = renderOptions(world_to_camera, width, height, fx, fy, cx, cy, near_plane, background,
                                                     max_sh_degree, coord);
          std::vector<float> img;
          bool ok;
          if (py::isinstance<py::bytes>(input)) {
            const std::string b = input.cast<std::string>();
            if (b.size() > static_cast<size_t>(INT32_MAX)) throw py::value_error("input is larger than 2 GiB");
            py::gil_scoped_release release;
            ok = spz::renderSpz(reinterpret_cast<const uint8_t *>(b.data()), static_cast<int32_t>(b.size()), o, &img);
          } else {
            const std::string fn = py::str(input).cast<std::string>();
            py::gil_scoped_release release;
            ok = spz::renderSpz(fn, o, &img);
          }
          return renderedImage(ok, img, o, "render_spz");
        },
        py::arg("input"), py::kw_only(), py::arg("world_to_camera"), py::arg("width"), py::arg("height"), py::arg("fx"),
        py::arg("fy"), py::arg("cx"), py::arg("cy"), py::arg("near") = 0.2f,
        py::arg("background") = py::make_tuple(0.0f, 0.0f, 0.0f), py::arg("max_sh_degree") = 3,
        py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        "Render one pinhole view of a .spz file (a path or the file's bytes) on the device (spz::renderSpz; the "
        "contract is in include/spz_amd.h \"render\").  world_to_camera: 3x4 [R | t], OpenCV axes (x right, y down, z "
        "forward), in the frame `coord` (the file as load_spz(to = coord) returns it).  Returns a (height, width, 4) "
        "float32 array: RGB + alpha, not clamped.");
  m.def("render_cloud",
        [](const spz::GaussianCloud &cloud, const py::object &world_to_camera, int width, int height, float fx, float fy,
           float cx, float cy, float near_plane, const py::object &background, int max_sh_degree) -> py::object {
          const spz::RenderOptions o = renderOptions(world_to_camera, width, height, fx, fy, cx, cy, near_plane, background,
                                                     max_sh_degree, spz::CoordinateSystem::UNSPECIFIED);
          std::vector<float> img;
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::renderCloud(cloud, o, &img);
          }
          return renderedImage(ok, img, o, "render_cloud");
        },
        py::arg("cloud"), py::kw_only(), py::arg("world_to_camera"), py::arg("width"), py::arg("height"), py::arg("fx"),
        py::arg("fy"), py::arg("cx"), py::arg("cy"), py::arg("near") = 0.2f,
        py::arg("background") = py::make_tuple(0.0f, 0.0f, 0.0f), py::arg("max_sh_degree") = 3,
        "Render one pinhole view of a GaussianCloud in host memory on the device (spz::renderCloud): the cloud is "
        "uploaded and rendered as it is, in the frame of world_to_camera.  Returns a (height, width, 4) float32 array.");
  m.def("render_depth_spz",
        [](const py::object &input, const py::object &world_to_camera, int width, int height, float fx, float fy,
           float cx, float cy, float near_plane, const py::object &background, int max_sh_degree,
           spz::CoordinateSystem coord) -> py::object {
          const spz::RenderOptions o = renderOptions(world_to_camera, width, height, fx, fy, cx, cy, near_plane, background,
                                                     max_sh_degree, coord);
          spz::DepthMaps maps;
          bool ok;
          if (py::isinstance<py::bytes>(input)) {
            const std::string b = input.cast<std::string>();
            if (b.size() > static_cast<size_t>(INT32_MAX)) throw py::value_error("input is larger than 2 GiB");
            py::gil_scoped_release release;
            ok = spz::renderSpzDepth(reinterpret_cast<const uint8_t *>(b.data()), static_cast<int32_t>(b.size()), o, &maps);
          } else {
            const std::string fn = py::str(input).cast<std::string>();
            py::gil_scoped_release release;
            ok = spz::renderSpzDepth(fn, o, &maps);
          }
          return renderedDepth(ok, maps, o, "render_depth_spz");
        },
        py::arg("input"), py::kw_only(), py::arg("world_to_camera"), py::arg("width"), py::arg("height"), py::arg("fx"),
        py::arg("fy"), py::arg("cx"), py::arg("cy"), py::arg("near") = 0.2f,
        py::arg("background") = py::make_tuple(0.0f, 0.0f, 0.0f), py::arg("max_sh_degree") = 3,
        py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        "The depth maps of one pinhole view of a .spz file (a path or the file's bytes) on the device "
        "(spz::renderSpzDepth; the contract is in include/spz_amd.h \"render depth\"); the arguments are render_spz's.  "
        "Returns a dict of (height, width) arrays: expected (float32: accumulated / alpha, +inf where alpha is 0), median "
        "(float32: the depth at which the transmittance falls below 0.5, +inf for none), alpha (float32), index (int32: "
        "the median Gaussian's index in the file, -1 for none) and accumulated (float32: the sum of (T a) z).");
  m.def("render_depth_cloud",
        [](const spz::GaussianCloud &cloud, const py::object &world_to_camera, int width, int height, float fx, float fy,
           float cx, float cy, float near_plane, const py::object &background, int max_sh_degree) -> py::object {
          const spz::RenderOptions o = renderOptions(world_to_camera, width, height, fx, fy, cx, cy, near_plane, background,
                                                     max_sh_degree, spz::CoordinateSystem::UNSPECIFIED);
          spz::DepthMaps maps;
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::renderCloudDepth(cloud, o, &maps);
          }
          return renderedDepth(ok, maps, o, "render_depth_cloud");
        },
        py::arg("cloud"), py::kw_only(), py::arg("world_to_camera"), py::arg("width"), py::arg("height"), py::arg("fx"),
        py::arg("fy"), py::arg("cx"), py::arg("cy"), py::arg("near") = 0.2f,
        py::arg("background") = py::make_tuple(0.0f, 0.0f, 0.0f), py::arg("max_sh_degree") = 3,
        "The depth maps of one pinhole view of a GaussianCloud in host memory (spz::renderCloudDepth): the dict of "
        "render_depth_spz, the cloud uploaded and taken as it is, in the frame of world_to_camera.");
  m.def("look_at",
        [](const std::array<float, 3> &eye, const std::array<float, 3> &target, const std::array<float, 3> &up) {
          std::array<float, 12> r;
          try {
            r = spz::lookAt(eye, target, up);
          } catch (const std::invalid_argument &e) {
            throw py::value_error(e.what());
          }
          py::array_t<float> out({py::ssize_t(3), py::ssize_t(4)});
          std::memcpy(out.mutable_data(), r.data(), sizeof(r));
          return out;
        },
        py::arg("eye"), py::arg("target"), py::arg("up"),
        "The 3x4 world_to_camera (float32) of a camera at eye looking at target, OpenCV axes: up maps to -y.");
  m.def("prune_spz",
        [](const std::string &input, const std::string &output, const py::object &views, const py::object &keep,
           const py::object &keep_fraction, const py::object &min_score, const std::string &score,
           spz::CoordinateSystem coord, float near_plane, const py::object &return_scores) -> py::object {
          // the arguments first: every problem is a ValueError before any device work
          auto is_int = [](const py::object &v) { return py::isinstance<py::int_>(v) && !py::isinstance<py::bool_>(v); };
          auto is_real = [](const py::object &v) {
            return (py::isinstance<py::float_>(v) || py::isinstance<py::int_>(v)) && !py::isinstance<py::bool_>(v);
          };
          if (!py::isinstance<py::bool_>(return_scores)) throw py::value_error("return_scores must be a bool");
          const int rules = (keep.is_none() ? 0 : 1) + (keep_fraction.is_none() ? 0 : 1) + (min_score.is_none() ? 0 : 1);
          if (rules != 1) throw py::value_error("give exactly one of keep, keep_fraction, min_score");
          spz::PruneOptions o;
          if (!keep.is_none()) {
            if (!is_int(keep) || py::reinterpret_borrow<py::int_>(keep) < py::int_(0) ||
                py::reinterpret_borrow<py::int_>(keep) > py::int_(0x7fffffff)) {
              throw py::value_error("keep must be an int in 0..n");
            }
            o.keepCount = py::cast<int64_t>(keep);
          }
          if (!keep_fraction.is_none()) {
            const double f = is_real(keep_fraction) ? py::cast<double>(keep_fraction) : -1.0;
            if (!(f >= 0.0 && f <= 1.0)) throw py::value_error("keep_fraction must be a number in [0, 1]");
            o.keepFraction = f;
          }
          if (!min_score.is_none()) {
            const double v = is_real(min_score) ? py::cast<double>(min_score) : __builtin_nan("");
            if (!std::isfinite(v)) throw py::value_error("min_score must be a finite number");
            o.minScore = v;
          }
          if (score == "sum") {
            o.score = spz::PruneOptions::Sum;
          } else if (score == "max") {
            o.score = spz::PruneOptions::Max;
          } else {
            throw py::value_error("score must be 'sum' or 'max'");
          }
          if (!std::isfinite(near_plane) || !(near_plane > 0.0f)) throw py::value_error("near_plane must be > 0");
          o.coord = coord;
          o.nearPlane = near_plane;
          if (py::isinstance<py::dict>(views) || py::isinstance<py::str>(views) || !py::isinstance<py::sequence>(views)) {
            throw py::value_error("views must be a sequence of view dicts (orbit_views, load_3dgs_cameras)");
          }
          const py::sequence seq = py::reinterpret_borrow<py::sequence>(views);
          if (seq.size() < 1 || seq.size() > SPZ_AMD_PRUNE_MAX_VIEWS) {
            throw py::value_error("give 1..1024 views, got " + std::to_string(seq.size()));
          }
          for (size_t k = 0; k < seq.size(); ++k) o.views.push_back(pruneView(seq[k], k, coord, near_plane));
          const bool details = py::cast<bool>(return_scores);
          std::vector<uint8_t> mask;
          std::vector<uint64_t> sums;
          std::vector<float> maxima;
          int64_t kept = 0;
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::pruneSpz(input, output, o, &kept, details ? &mask : nullptr, details ? &sums : nullptr,
                               details ? &maxima : nullptr);
          }
          if (!ok) {
            raiseFailure("prune_spz: refused for this file (see the [SPZ ERROR] line)",
                         "prune_spz: " + input + " -> " + output + " failed (see the [SPZ ERROR] line)");
          }
          if (!details) return py::int_(kept);
          return py::make_tuple(kept, toArray<uint8_t, bool>(mask), toArray(sums), toArray(maxima));
        },
        py::arg("input_filename"), py::arg("output_filename"), py::arg("views"), py::kw_only(),
        py::arg("keep") = py::none(), py::arg("keep_fraction") = py::none(), py::arg("min_score") = py::none(),
        py::arg("score") = "sum", py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED, py::arg("near_plane") = 0.2f,
        py::arg("return_scores") = false,
        "Drop the splats that contribute least to a set of views, without requantising (spz::pruneSpz; the contract is "
        "in include/spz_amd.h \"prune\").  views: 1..1024 dicts with world_to_camera (3x4, OpenCV axes, in the frame "
        "`coord`), fx, fy, cx, cy, width, height (orbit_views, load_3dgs_cameras).  score 'sum': the blend weight T a "
        "summed over every pixel of every view (pixel units); 'max': its maximum.  Exactly one rule: keep (a count), "
        "keep_fraction (K = ceil(f n)) or min_score (keep score >= s).  Ties go by input index.  Returns the kept count, "
        "or (kept, mask (bool per input point), weight_sum (uint64, pixel units times 2^24), weight_max (float32)) when "
        "return_scores.  The output equals filter_spz's with the mask.");
  m.def("orbit_views",
        [](int n, int width, int height, float fov_y, const py::object &center, const py::object &radius,
           float distance, const py::object &scene, spz::CoordinateSystem coord) -> py::list {
          std::array<float, 3> c = {0.0f, 0.0f, 0.0f};
          float r = 0.0f;
          if (center.is_none() || radius.is_none()) {
            if (scene.is_none()) throw py::value_error("give center and radius, or a scene to take them from");
            std::vector<float> pos;
            if (py::isinstance<spz::GaussianCloud>(scene)) {
              pos = scene.cast<const spz::GaussianCloud &>().positions;
            } else {
              spz::UnpackOptions u;
              u.to = coord;
              spz::GaussianCloud g;
              if (py::isinstance<py::bytes>(scene)) {
                const std::string b = scene.cast<std::string>();
                py::gil_scoped_release release;
                g = spz::loadSpz(reinterpret_cast<const uint8_t *>(b.data()), static_cast<int32_t>(b.size()), u);
              } else {
                const std::string fn = py::str(scene).cast<std::string>();
                py::gil_scoped_release release;
                g = spz::loadSpz(fn, u);
              }
              if (g.numPoints <= 0) {
                raiseIfDeviceUnusable();
                throw py::value_error("orbit_views: the scene has no points, or does not load");
              }
              pos.swap(g.positions);
            }
            if (!spz::boundingSphere(pos, &c, &r)) throw py::value_error("orbit_views: the scene has no finite positions");
          }
          if (!center.is_none()) {
            const auto cc = center.cast<std::vector<float>>();
            if (cc.size() != 3) throw py::value_error("center must have three values");
            for (int k = 0; k < 3; ++k) c[k] = cc[k];
          }
          if (!radius.is_none()) r = radius.cast<float>();
          std::vector<spz::PruneOptions::View> v;
          try {
            v = spz::orbitViews(n, c, r, width, height, fov_y, distance);
          } catch (const std::invalid_argument &e) {
            throw py::value_error(e.what());
          }
          py::list out;
          for (const auto &x : v) out.append(viewDict(x));
          return out;
        },
        py::arg("n"), py::kw_only(), py::arg("width"), py::arg("height"), py::arg("fov_y"),
        py::arg("center") = py::none(), py::arg("radius") = py::none(), py::arg("distance") = 2.5f,
        py::arg("scene") = py::none(), py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        "n view dicts (prune_spz's form) on a Fibonacci sphere around center at distance * radius, each looking at the "
        "centre, fov_y in degrees (spz::orbitViews).  Without center or radius they come from the axis-aligned box of "
        "`scene` (a .spz path, its bytes or a GaussianCloud; files are decoded to `coord`): its centre and half "
        "diagonal.  Floaters inflate that box: clean first, or pass both.");
  m.def("load_views_file",
        [](const std::string &filename) {
          std::vector<spz::PruneOptions::View> v;
          try {
            v = spz::loadViewsFile(filename);
          } catch (const std::invalid_argument &e) {
            throw py::value_error(e.what());
          }
          py::list out;
          for (const auto &x : v) out.append(viewDict(x));
          return out;
        },
        py::arg("filename"),
        "The views of a plain-text views file (spz_prune --views; spz::loadViewsFile) as prune_spz's view dicts: one "
        "view per line, 'width height fx fy cx cy r00 r01 r02 t0 r10 r11 r12 t1 r20 r21 r22 t2', '#' starts a comment.");
  m.def("align_spz",
        [](const py::object &source, const py::object &target, const py::object &rotation, const py::object &translation,
           double scale, spz::CoordinateSystem coord, bool estimate_scale, double overlap, const py::object &max_distance,
           const py::object &stride, const py::object &max_iterations, double relative_fitness, double relative_rmse,
           bool init_centroids) {
          // the arguments first: every problem is a ValueError before any device work
          spz::AlignOptions o;
          if (!rotation.is_none()) {
            py::array_t<double, py::array::c_style | py::array::forcecast> q(rotation);
            if (q.size() != 4) throw py::value_error("rotation must be (x, y, z, w)");
            for (int k = 0; k < 4; ++k) o.rotation[k] = q.data()[k];
          }
          if (!translation.is_none()) {
            py::array_t<double, py::array::c_style | py::array::forcecast> t(translation);
            if (t.size() != 3) throw py::value_error("translation must be (x, y, z)");
            for (int k = 0; k < 3; ++k) o.translation[k] = t.data()[k];
          }
          auto count = [](const py::object &v, const char *name, long long hi) {
            if (py::isinstance<py::bool_>(v) || !py::isinstance<py::int_>(v)) {
              throw py::value_error(std::string(name) + " must be an int");
            }
            const long long x = v.cast<long long>();
            if (x < 1 || x > hi) throw py::value_error(std::string(name) + " must be in 1.." + std::to_string(hi));
            return static_cast<uint32_t>(x);
          };
          o.stride = count(stride, "stride", 0xffffffffll);
          o.maxIterations = count(max_iterations, "max_iterations", 1000);
          o.scale = scale;
          o.coord = coord;
          o.estimateScale = estimate_scale;
          o.overlap = overlap;
          if (!max_distance.is_none()) o.maxDistance = max_distance.cast<double>();
          o.relativeFitness = relative_fitness;
          o.relativeRmse = relative_rmse;
          o.initCentroids = init_centroids;
          if (!(overlap > 0.0) || !(overlap <= 1.0)) throw py::value_error("overlap must be in (0, 1]");
          if (o.maxDistance && (!std::isfinite(*o.maxDistance) || !(*o.maxDistance > 0.0))) {
            throw py::value_error("max_distance must be None or a finite number > 0");
          }
          if (!std::isfinite(scale) || !(scale > 0.0)) throw py::value_error("scale must be a finite number > 0");
          if (py::isinstance<py::bytes>(source) != py::isinstance<py::bytes>(target)) {
            throw py::value_error("give source and target both as paths or both as bytes");
          }
          spz::AlignResult r;
          bool ok;
          if (py::isinstance<py::bytes>(source)) {
            const std::string a = source.cast<std::string>(), b = target.cast<std::string>();
            if (a.size() > static_cast<size_t>(INT32_MAX) || b.size() > static_cast<size_t>(INT32_MAX)) {
              throw py::value_error("an input is larger than 2 GiB");
            }
            py::gil_scoped_release release;
            ok = spz::alignSpz(reinterpret_cast<const uint8_t *>(a.data()), static_cast<int32_t>(a.size()),
                               reinterpret_cast<const uint8_t *>(b.data()), static_cast<int32_t>(b.size()), o, &r);
          } else {
            const std::string fa = py::str(source).cast<std::string>(), fb = py::str(target).cast<std::string>();
            py::gil_scoped_release release;
            ok = spz::alignSpz(fa, fb, o, &r);
          }
          if (!ok) {
            raiseFailure("align_spz: refused (see the [SPZ ERROR] line)", "align_spz failed (see the [SPZ ERROR] line)",
                         /*unsupportedRefused=*/true);
          }
          py::dict d;
          d["rotation"] = py::make_tuple(r.rotation[0], r.rotation[1], r.rotation[2], r.rotation[3]);
          d["translation"] = py::make_tuple(r.translation[0], r.translation[1], r.translation[2]);
          d["scale"] = r.scale;
          d["fitness"] = r.fitness;
          d["inlier_rmse"] = r.inlierRmse;
          d["inliers"] = r.inliers;
          d["iterations"] = r.iterations;
          d["converged"] = r.converged;
          d["degenerate"] = r.degenerate;
          py::list h;
          for (const auto &s : r.history) h.append(py::make_tuple(s.fitness, s.inlierRmse, s.inliers));
          d["history"] = h;
          return d;
        },
        py::arg("source"), py::arg("target"), py::kw_only(), py::arg("rotation") = py::none(),
        py::arg("translation") = py::none(), py::arg("scale") = 1.0,
        py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED, py::arg("estimate_scale") = false,
        py::arg("overlap") = 1.0, py::arg("max_distance") = py::none(), py::arg("stride") = 1,
        py::arg("max_iterations") = 30, py::arg("relative_fitness") = 1e-6, py::arg("relative_rmse") = 1e-6,
        py::arg("init_centroids") = false,
        "The similarity that places the source .spz on the target .spz (paths, or both files' bytes), by a trimmed "
        "point-to-point ICP with an optional scale on the device (spz::alignSpz; the contract is in include/spz_amd.h "
        "\"align\").  rotation (x, y, z, w), translation and scale are the initial placement in the frame `coord`.  "
        "Returns a dict: rotation, translation, scale (in `coord`, ready for transform_spz or a merge placement), "
        "fitness, inlier_rmse, inliers, iterations, converged, degenerate and history, a list of (fitness, "
        "inlier_rmse, inliers) per step.");
  m.def("compare_spz",
        [](const py::object &a, const py::object &b, const py::object &views, spz::CoordinateSystem coord,
           const py::object &background, int max_sh_degree, float near_plane, const py::object &return_maps) {
          // the arguments first: every problem is a ValueError before any device work
          if (!py::isinstance<py::bool_>(return_maps)) throw py::value_error("return_maps must be a bool");
          if (!std::isfinite(near_plane) || !(near_plane > 0.0f)) throw py::value_error("near must be > 0");
          if (max_sh_degree < 0 || max_sh_degree > 3) throw py::value_error("max_sh_degree must be 0..3");
          spz::CompareOptions o;
          py::array_t<float, py::array::c_style | py::array::forcecast> bg(background);
          if (bg.size() != 3) throw py::value_error("background must have three values");
          for (int k = 0; k < 3; ++k) {
            o.background[k] = bg.data()[k];
            if (!std::isfinite(o.background[k])) throw py::value_error("background must be finite");
          }
          o.coord = coord;
          o.nearPlane = near_plane;
          o.maxShDegree = max_sh_degree;
          if (py::isinstance<py::dict>(views) || py::isinstance<py::str>(views) || !py::isinstance<py::sequence>(views)) {
            throw py::value_error("views must be a sequence of view dicts (orbit_views, load_3dgs_cameras)");
          }
          const py::sequence seq = py::reinterpret_borrow<py::sequence>(views);
          if (seq.size() < 1 || seq.size() > SPZ_AMD_COMPARE_MAX_VIEWS) {
            throw py::value_error("give 1..1024 views, got " + std::to_string(seq.size()));
          }
          for (size_t k = 0; k < seq.size(); ++k) o.views.push_back(pruneView(seq[k], k, coord, near_plane));
          const bool maps = py::cast<bool>(return_maps);
          std::vector<spz::ImageMetrics> got;
          std::vector<std::vector<float>> ssim;
          bool ok;
          if (py::isinstance<py::bytes>(a) != py::isinstance<py::bytes>(b)) {
            throw py::value_error("give a and b both as paths or both as bytes");
          }
          if (py::isinstance<py::bytes>(a)) {
            const std::string ba = a.cast<std::string>(), bb = b.cast<std::string>();
            if (ba.size() > static_cast<size_t>(INT32_MAX) || bb.size() > static_cast<size_t>(INT32_MAX)) {
              throw py::value_error("an input is larger than 2 GiB");
            }
            py::gil_scoped_release release;
            ok = spz::compareSpz(reinterpret_cast<const uint8_t *>(ba.data()), static_cast<int32_t>(ba.size()),
                                 reinterpret_cast<const uint8_t *>(bb.data()), static_cast<int32_t>(bb.size()), o, &got,
                                 maps ? &ssim : nullptr);
          } else {
            const std::string fa = py::str(a).cast<std::string>(), fb = py::str(b).cast<std::string>();
            py::gil_scoped_release release;
            ok = spz::compareSpz(fa, fb, o, &got, maps ? &ssim : nullptr);
          }
          if (!ok) {
            raiseFailure("compare_spz: refused (see the [SPZ ERROR] line)",
                         "compare_spz failed (see the [SPZ ERROR] line)");
          }
          py::list out;
          for (size_t v = 0; v < got.size(); ++v) {
            py::dict d = metricsDict(got[v]);
            if (maps) d["ssim_map"] = mapArray(ssim[v], o.views[v].height, o.views[v].width);
            out.append(d);
          }
          return out;
        },
        py::arg("a"), py::arg("b"), py::arg("views"), py::kw_only(),
        py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        py::arg("background") = py::make_tuple(0.0f, 0.0f, 0.0f), py::arg("max_sh_degree") = 3,
        py::arg("near") = 0.2f, py::arg("return_maps") = false,
        "Render two .spz files (paths, or both files' bytes) from every view on the device and compare each view's two "
        "images (spz::compareSpz; the contract is in include/spz_amd.h \"image metrics\" and \"compare\").  views: "
        "1..1024 dicts as orbit_views, load_views_file and load_3dgs_cameras return them, in the frame `coord`.  Returns "
        "one dict per view: mse, psnr (dB; inf when the images are equal), ssim, l1, max_abs; with return_maps also "
        "ssim_map, a (height, width) float32 array of S averaged over the channels.");
  m.def("refine_spz",
        [](const py::object &input, const py::object &target, const py::object &output, const py::object &views,
           int iterations, spz::CoordinateSystem coord, const py::object &background, int max_sh_degree,
           float near_plane, double lambda_dssim, const py::object &lrs, double beta1, double beta2, double eps,
           const py::object &train, const py::object &densify) {
          // the arguments first: every problem is a ValueError before any device work
          static const char *const kArrays[6] = {"positions", "scales", "rotations", "alphas", "colors", "sh"};
          if (iterations < 0) throw py::value_error("iterations must be >= 0");
          if (!std::isfinite(near_plane) || !(near_plane > 0.0f)) throw py::value_error("near must be > 0");
          if (max_sh_degree < 0 || max_sh_degree > 3) throw py::value_error("max_sh_degree must be 0..3");
          if (!(lambda_dssim >= 0.0 && lambda_dssim <= 1.0)) throw py::value_error("lambda_dssim must be in [0, 1]");
          if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) {
            throw py::value_error("beta1 and beta2 must be in [0, 1)");
          }
          if (!std::isfinite(eps) || eps < 0.0) throw py::value_error("eps must be finite and >= 0");
          spz::RefineOptions o;
          py::array_t<float, py::array::c_style | py::array::forcecast> bg(background);
          if (bg.size() != 3) throw py::value_error("background must have three values");
          for (int k = 0; k < 3; ++k) {
            o.background[k] = bg.data()[k];
            if (!std::isfinite(o.background[k])) throw py::value_error("background must be finite");
          }
          o.coord = coord;
          o.nearPlane = near_plane;
          o.maxShDegree = max_sh_degree;
          o.iterations = iterations;
          o.lambdaDssim = lambda_dssim;
          o.beta1 = beta1;
          o.beta2 = beta2;
          o.eps = eps;
          if (!lrs.is_none()) {
            if (!py::isinstance<py::dict>(lrs)) throw py::value_error("lrs must be a dict by array name");
            double *const slot[6] = {nullptr, &o.scaleLr, &o.rotationLr, &o.alphaLr, &o.colorLr, &o.shLr};
            for (auto item : py::reinterpret_borrow<py::dict>(lrs)) {
              const std::string name = py::str(item.first).cast<std::string>();
              const double x = py::cast<double>(item.second);
              if (!std::isfinite(x) || x < 0.0) throw py::value_error("lrs[" + name + "] must be finite and >= 0");
              int k = 0;
              while (k < 6 && name != kArrays[k]) ++k;
              if (k == 6) throw py::value_error("lrs: unknown array '" + name + "'");
              if (k == 0) o.positionLr = x; else *slot[k] = x;
            }
          }
          if (!train.is_none()) {
            if (py::isinstance<py::str>(train) || !py::isinstance<py::sequence>(train)) {
              throw py::value_error("train must be a sequence of array names");
            }
            o.train = 0;
            for (auto item : py::reinterpret_borrow<py::sequence>(train)) {
              const std::string name = py::str(item).cast<std::string>();
              int k = 0;
              while (k < 6 && name != kArrays[k]) ++k;
              if (k == 6) throw py::value_error("train: unknown array '" + name + "'");
              o.train |= 1u << k;
            }
            if (o.train == 0) throw py::value_error("train must name at least one array");
          }
          if (!densify.is_none()) {
            // a dict, or an options object with the same names (spz_amd.abi.DensifyOptions)
            static const char *const kInts[4] = {"interval", "from_iter", "until_iter", "opacity_reset_interval"};
            static const char *const kReals[5] = {"grad_threshold", "percent_dense", "extent", "min_opacity", "max_scale"};
            static const char *const kCounts[2] = {"max_points", "seed"};
            spz::DensifyOptions &dn = o.densify;
            int *const ints[4] = {&dn.interval, &dn.fromIter, &dn.untilIter, &dn.opacityResetInterval};
            double *const reals[5] = {&dn.gradThreshold, &dn.percentDense, &dn.extent, &dn.minOpacity, &dn.maxScale};
            uint64_t *const counts[2] = {&dn.maxPoints, &dn.seed};
            const bool isDict = py::isinstance<py::dict>(densify);
            size_t known = 0;
            auto field = [&](const char *name) -> py::object {
              if (isDict) {
                const py::dict dd = py::reinterpret_borrow<py::dict>(densify);
                if (!dd.contains(name)) return py::none();
                ++known;
                return dd[name];
              }
              if (!py::hasattr(densify, name)) throw py::value_error("densify must be a dict or a densify options object");
              return densify.attr(name);
            };
            try {
              for (int k = 0; k < 4; ++k) {
                const py::object x = field(kInts[k]);
                if (x.is_none()) continue;
                if (!py::isinstance<py::int_>(x) || py::isinstance<py::bool_>(x)) throw py::cast_error();
                const long long v = x.cast<long long>();
                if (v < 0 || v > 0x7fffffffLL) throw py::cast_error();
                *ints[k] = static_cast<int>(v);
              }
              for (int k = 0; k < 5; ++k) {
                const py::object x = field(kReals[k]);
                if (!x.is_none()) *reals[k] = x.cast<double>();
              }
              for (int k = 0; k < 2; ++k) {
                const py::object x = field(kCounts[k]);
                if (x.is_none()) continue;
                if (!py::isinstance<py::int_>(x) || py::isinstance<py::bool_>(x)) throw py::cast_error();
                *counts[k] = x.cast<uint64_t>();
              }
            } catch (const py::cast_error &) {
              throw py::value_error("densify: a field has the wrong type or is out of range");
            }
            if (isDict && known != py::reinterpret_borrow<py::dict>(densify).size()) {
              throw py::value_error("densify: unknown field (interval, from_iter, until_iter, opacity_reset_interval, "
                                    "grad_threshold, percent_dense, extent, min_opacity, max_scale, max_points, seed)");
            }
            const double realsNow[5] = {dn.gradThreshold, dn.percentDense, dn.extent, dn.minOpacity, dn.maxScale};
            for (double x : realsNow) {
              if (!std::isfinite(x) || x < 0.0) throw py::value_error("densify: values must be finite and >= 0");
            }
            if (dn.untilIter < dn.fromIter) throw py::value_error("densify: until_iter is below from_iter");
            if (!(dn.minOpacity > 0.0 && dn.minOpacity < 1.0)) throw py::value_error("densify: min_opacity must be in (0, 1)");
            if (dn.interval > 0 && !(dn.percentDense > 0.0)) throw py::value_error("densify: percent_dense must be > 0");
            if (dn.interval > 0 && (o.train & 3u) != 3u) {
              throw py::value_error("densify needs positions and scales among the trained arrays");
            }
            if (dn.interval > 0 && dn.opacityResetInterval > 0 && (o.train & 8u) == 0u) {
              throw py::value_error("densify: the opacity reset needs alphas among the trained arrays");
            }
          }
          if (py::isinstance<py::dict>(views) || py::isinstance<py::str>(views) || !py::isinstance<py::sequence>(views)) {
            throw py::value_error("views must be a sequence of view dicts (orbit_views, load_3dgs_cameras)");
          }
          const py::sequence seq = py::reinterpret_borrow<py::sequence>(views);
          if (seq.size() < 1 || seq.size() > SPZ_AMD_REFINE_MAX_VIEWS) {
            throw py::value_error("give 1..1024 views, got " + std::to_string(seq.size()));
          }
          for (size_t k = 0; k < seq.size(); ++k) o.views.push_back(pruneView(seq[k], k, coord, near_plane));
          if (py::isinstance<py::bytes>(input) != py::isinstance<py::bytes>(target)) {
            throw py::value_error("give input and target both as paths or both as bytes");
          }
          spz::RefineReport rep;
          std::vector<uint8_t> bytes;
          bool ok;
          const bool fromBytes = py::isinstance<py::bytes>(input);
          if (fromBytes) {
            if (!output.is_none()) throw py::value_error("with bytes in, output must be None: the bytes are returned");
            const std::string ba = input.cast<std::string>(), bb = target.cast<std::string>();
            if (ba.size() > static_cast<size_t>(INT32_MAX) || bb.size() > static_cast<size_t>(INT32_MAX)) {
              throw py::value_error("an input is larger than 2 GiB");
            }
            py::gil_scoped_release release;
            ok = spz::refineSpz(reinterpret_cast<const uint8_t *>(ba.data()), static_cast<int32_t>(ba.size()),
                                reinterpret_cast<const uint8_t *>(bb.data()), static_cast<int32_t>(bb.size()), o, &bytes,
                                &rep);
          } else {
            if (output.is_none()) throw py::value_error("with paths in, give the output path");
            const std::string fi = py::str(input).cast<std::string>(), ft = py::str(target).cast<std::string>(),
                              fo = py::str(output).cast<std::string>();
            py::gil_scoped_release release;
            ok = spz::refineSpz(fi, ft, fo, o, &rep);
          }
          if (!ok) {
            raiseFailure("refine_spz: refused (see the [SPZ ERROR] line)", "refine_spz failed (see the [SPZ ERROR] line)");
          }
          py::dict d;
          d["history"] = rep.history;
          py::list before, after;
          for (const spz::ImageMetrics &x : rep.before) before.append(metricsDict(x));
          for (const spz::ImageMetrics &x : rep.after) after.append(metricsDict(x));
          d["before"] = before;
          d["after"] = after;
          d["skipped"] = rep.skipped;
          d["position_lr"] = rep.positionLr;
          d["ms"] = py::make_tuple(rep.ms[0], rep.ms[1], rep.ms[2]);
          d["num_points"] = rep.numPoints;
          py::list rounds;
          for (const spz::DensifyRound &x : rep.rounds) {
            py::dict r;
            r["iteration"] = x.iteration;
            r["cloned"] = x.cloned;
            r["split"] = x.split;
            r["culled"] = x.culled;
            r["refused"] = x.refused;
            r["num_points"] = x.numPoints;
            rounds.append(r);
          }
          d["rounds"] = rounds;
          if (fromBytes) d["data"] = py::bytes(reinterpret_cast<const char *>(bytes.data()), bytes.size());
          return d;
        },
        py::arg("input"), py::arg("target"), py::arg("output"), py::arg("views"), py::kw_only(),
        py::arg("iterations") = 200, py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        py::arg("background") = py::make_tuple(0.0f, 0.0f, 0.0f), py::arg("max_sh_degree") = 3, py::arg("near") = 0.2f,
        py::arg("lambda_dssim") = 0.2, py::arg("lrs") = py::none(), py::arg("beta1") = 0.9, py::arg("beta2") = 0.999,
        py::arg("eps") = 1e-15, py::arg("train") = py::none(), py::arg("densify") = py::none(),
        "Fit the .spz file `input` to the file `target` over `views` on the device and write `output` (spz::refineSpz; "
        "the contract is in include/spz_amd.h \"refine\"): the target is rendered once per view, then `iterations` Adam "
        "steps on the 3DGS loss (1 - lambda_dssim) l1 + lambda_dssim (1 - ssim), view i mod V at step i, over the "
        "arrays `train` names (default: all six of positions, scales, rotations, alphas, colors, sh); sections of "
        "untrained arrays keep the input's bytes.  lrs: a dict by array name replacing 3DGS's published rates (the "
        "position rate defaults to 1.6e-4 times the target's bounding-sphere radius).  Paths in: `output` is written; "
        "bytes in (output None): the dict carries \"data\".  Returns a dict: history (the loss before each step), "
        "before and after (one metrics dict per view, the latter of the written stream), skipped, position_lr, ms, "
        "num_points and rounds.  densify: None, or a dict (or spz_amd.abi.DensifyOptions) of interval, from_iter, "
        "until_iter, grad_threshold, percent_dense, extent, min_opacity, max_scale, max_points, opacity_reset_interval, "
        "seed: with interval > 0 Gaussians are cloned, split and culled every `interval` iterations (include/spz_amd.h "
        "\"densify\"), the output's count is num_points and rounds has one dict per round.");
  m.def("locate_spz",
        [](const py::object &input, const py::object &view, const py::object &image, int iterations, int levels,
           spz::CoordinateSystem coord, const py::object &background, int max_sh_degree, float near_plane,
           double lambda_dssim, double lr_rotation, const py::object &lr_translation, double lr_final_factor, double beta1,
           double beta2, double eps) {
          // the arguments first: every problem is a ValueError before any device work
          if (iterations < 0) throw py::value_error("iterations must be >= 0");
          if (levels < 1 || levels > SPZ_AMD_LOCATE_MAX_LEVELS) throw py::value_error("levels must be 1..8");
          if (!std::isfinite(near_plane) || !(near_plane > 0.0f)) throw py::value_error("near must be > 0");
          if (max_sh_degree < 0 || max_sh_degree > 3) throw py::value_error("max_sh_degree must be 0..3");
          if (!(lambda_dssim >= 0.0 && lambda_dssim <= 1.0)) throw py::value_error("lambda_dssim must be in [0, 1]");
          if (!std::isfinite(lr_rotation) || lr_rotation < 0.0) throw py::value_error("lr_rotation must be finite and >= 0");
          if (!(lr_final_factor > 0.0 && lr_final_factor <= 1.0)) throw py::value_error("lr_final_factor must be in (0, 1]");
          if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) {
            throw py::value_error("beta1 and beta2 must be in [0, 1)");
          }
          if (!std::isfinite(eps) || eps < 0.0) throw py::value_error("eps must be finite and >= 0");
          spz::LocateOptions o;
          py::array_t<float, py::array::c_style | py::array::forcecast> bg(background);
          if (bg.size() != 3) throw py::value_error("background must have three values");
          for (int k = 0; k < 3; ++k) {
            o.background[k] = bg.data()[k];
            if (!std::isfinite(o.background[k])) throw py::value_error("background must be finite");
          }
          o.coord = coord;
          o.nearPlane = near_plane;
          o.maxShDegree = max_sh_degree;
          o.iterations = iterations;
          o.levels = levels;
          o.lambdaDssim = lambda_dssim;
          o.rotationLr = lr_rotation;
          if (!lr_translation.is_none()) {
            const double x = py::cast<double>(lr_translation);
            if (!std::isfinite(x) || x < 0.0) throw py::value_error("lr_translation must be finite and >= 0");
            o.translationLr = x;
          }
          o.lrFinalFactor = lr_final_factor;
          o.beta1 = beta1;
          o.beta2 = beta2;
          o.eps = eps;
          const spz::PruneOptions::View v = pruneView(view, 0, coord, near_plane);
          if (!py::isinstance<py::array>(image)) throw py::value_error("image must be a numpy array");
          const py::array arr = py::reinterpret_borrow<py::array>(image);
          if (!arr.dtype().is(py::dtype::of<float>())) throw py::value_error("image must be float32");
          if (arr.ndim() != 3 || (arr.shape(2) != 3 && arr.shape(2) != 4) || arr.shape(0) != v.height ||
              arr.shape(1) != v.width) {
            throw py::value_error("image must be the view's height x width x 3 or 4");
          }
          if (v.width % (1 << (levels - 1)) != 0 || v.height % (1 << (levels - 1)) != 0) {
            throw py::value_error("width and height must be divisible by 2^(levels - 1)");
          }
          const py::array_t<float, py::array::c_style | py::array::forcecast> pixels(arr);
          const int channels = static_cast<int>(arr.shape(2));
          spz::LocateReport rep;
          bool ok;
          if (py::isinstance<py::bytes>(input)) {
            const std::string b = input.cast<std::string>();
            if (b.size() > static_cast<size_t>(INT32_MAX)) throw py::value_error("the input is larger than 2 GiB");
            py::gil_scoped_release release;
            ok = spz::locateSpz(reinterpret_cast<const uint8_t *>(b.data()), static_cast<int32_t>(b.size()), v,
                                pixels.data(), channels, o, &rep);
          } else {
            const std::string f = py::str(input).cast<std::string>();
            py::gil_scoped_release release;
            ok = spz::locateSpz(f, v, pixels.data(), channels, o, &rep);
          }
          if (!ok) {
            raiseFailure("locate_spz: refused (see the [SPZ ERROR] line)", "locate_spz failed (see the [SPZ ERROR] line)");
          }
          py::dict d;
          d["history"] = rep.history;
          d["before"] = metricsDict(rep.before);
          d["after"] = metricsDict(rep.after);
          d["iterations"] = rep.iterations;
          d["lr_translation"] = rep.translationLr;
          d["ms"] = py::make_tuple(rep.ms[0], rep.ms[1], rep.ms[2]);
          return py::make_tuple(viewDict(rep.view), d);
        },
        py::arg("input"), py::arg("view"), py::arg("image"), py::kw_only(), py::arg("iterations") = 300,
        py::arg("levels") = 1, py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        py::arg("background") = py::make_tuple(0.0f, 0.0f, 0.0f), py::arg("max_sh_degree") = 3, py::arg("near") = 0.2f,
        py::arg("lambda_dssim") = 0.2, py::arg("lr_rotation") = 2e-3, py::arg("lr_translation") = py::none(),
        py::arg("lr_final_factor") = 0.1, py::arg("beta1") = 0.9, py::arg("beta2") = 0.999, py::arg("eps") = 1e-15,
        "Fit the pose of `view` (a view dict with a rough world_to_camera) so that the .spz file `input` (a path, or the "
        "file's bytes) renders as `image`, a (height, width, 3 or 4) float32 array (spz::locateSpz; the contract is in "
        "include/spz_amd.h \"locate\"): `iterations` Adam steps on the six values of a twist, down the gradient of the "
        "3DGS loss; with levels > 1 the first steps run on 2 x 2 box means of the image.  lr_translation None: "
        "lr_rotation times the distance from the camera to the scene's centre.  Returns (view, report): the view with "
        "its matrix replaced, and a dict of history (the loss before each step taken), before and after (metrics "
        "dicts), iterations, lr_translation and ms.");
  m.def("load_image",
        [](const std::string &path) {
          std::vector<float> pixels;
          int w = 0, h = 0;
          try {
            spz::loadImageFile(path, &pixels, &w, &h);
          } catch (const std::invalid_argument &e) {
            throw py::value_error(e.what());
          }
          py::array_t<float> out({static_cast<py::ssize_t>(h), static_cast<py::ssize_t>(w), py::ssize_t(3)});
          std::memcpy(out.mutable_data(), pixels.data(), pixels.size() * sizeof(float));
          return out;
        },
        py::arg("path"),
        "A picture as spz_render writes it, as locate_spz takes it: a binary PPM (P6, maxval 255) or a colour PFM (PF, "
        "either byte order) as a (height, width, 3) float32 array, rows top to bottom.  ValueError when the file does "
        "not open or is neither.");
  m.def("compare_images",
        [](const py::object &a, const py::object &b, const py::object &return_map) {
          if (!py::isinstance<py::bool_>(return_map)) throw py::value_error("return_map must be a bool");
          auto image = [](const py::object &o, const char *name) {
            if (!py::isinstance<py::array>(o)) throw py::value_error(std::string(name) + " must be a numpy array");
            const py::array arr = py::reinterpret_borrow<py::array>(o);
            if (!arr.dtype().is(py::dtype::of<float>())) throw py::value_error(std::string(name) + " must be float32");
            if (arr.ndim() != 3 || (arr.shape(2) != 3 && arr.shape(2) != 4)) {
              throw py::value_error(std::string(name) + " must be height x width x 3 or 4");
            }
            return py::array_t<float, py::array::c_style | py::array::forcecast>(arr);
          };
          const auto fa = image(a, "a"), fb = image(b, "b");
          if (fa.shape(0) != fb.shape(0) || fa.shape(1) != fb.shape(1)) {
            throw py::value_error("a and b must have the same height and width");
          }
          if (fa.shape(0) < 1 || fa.shape(0) > 16384 || fa.shape(1) < 1 || fa.shape(1) > 16384) {
            throw py::value_error("height and width must be in 1..16384");
          }
          const int h = static_cast<int>(fa.shape(0)), w = static_cast<int>(fa.shape(1));
          const int ca = static_cast<int>(fa.shape(2)), cb = static_cast<int>(fb.shape(2));
          const bool want = py::cast<bool>(return_map);
          spz::ImageMetrics m;
          std::vector<float> map;
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::compareImages(fa.data(), ca, fb.data(), cb, w, h, &m, want ? &map : nullptr);
          }
          if (!ok) {
            raiseFailure("compare_images: refused (see the [SPZ ERROR] line)",
                         "compare_images failed (see the [SPZ ERROR] line)");
          }
          py::dict d = metricsDict(m);
          if (want) d["ssim_map"] = mapArray(map, h, w);
          return d;
        },
        py::arg("a"), py::arg("b"), py::kw_only(), py::arg("return_map") = false,
        "PSNR, MSE, L1, max error and SSIM of two (height, width, 3 or 4) float32 images on the device "
        "(spz::compareImages; include/spz_amd.h \"image metrics\"): values clamped to [0, 1] (NaN -> 0), the first three "
        "channels, an 11x11 Gaussian window of sigma 1.5 with zero padding.  Returns a dict: mse, psnr, ssim, l1, "
        "max_abs; with return_map also ssim_map, (height, width) float32.");
  m.def("clean_spz",
        [](const std::string &input, const std::string &output, const py::object &k, const py::object &std_ratio,
           const py::object &radius, const py::object &min_neighbors, const py::object &return_details) -> py::object {
          // the arguments first: every problem is a ValueError before any device work
          auto is_int = [](const py::object &v) { return py::isinstance<py::int_>(v) && !py::isinstance<py::bool_>(v); };
          auto is_real = [](const py::object &v) {
            return (py::isinstance<py::float_>(v) || py::isinstance<py::int_>(v)) && !py::isinstance<py::bool_>(v);
          };
          if (!py::isinstance<py::bool_>(return_details)) throw py::value_error("return_details must be a bool");
          if (k.is_none() && radius.is_none() && min_neighbors.is_none()) {
            throw py::value_error("give k, or radius and min_neighbors, or both");
          }
          if (radius.is_none() != min_neighbors.is_none()) {
            throw py::value_error("radius and min_neighbors go together");
          }
          spz::CleanOptions o;
          if (!k.is_none()) {
            if (!is_int(k)) throw py::value_error("k must be an int in 1..64");
            const py::int_ kv = py::reinterpret_borrow<py::int_>(k);
            if (kv < py::int_(1) || kv > py::int_(64)) throw py::value_error("k must be an int in 1..64");
            if (!is_real(std_ratio)) throw py::value_error("std_ratio must be a finite number");
            const double s = py::cast<double>(std_ratio);
            if (!std::isfinite(s)) throw py::value_error("std_ratio must be a finite number");
            o.statistical = spz::CleanOptions::Statistical{py::cast<int>(kv), s};
          }
          if (!radius.is_none()) {
            if (!is_real(radius)) throw py::value_error("radius must be a finite number > 0");
            const double r = py::cast<double>(radius);
            if (!std::isfinite(r) || !(r > 0.0)) throw py::value_error("radius must be a finite number > 0");
            if (!is_int(min_neighbors)) throw py::value_error("min_neighbors must be an int in 1..256");
            const py::int_ mv = py::reinterpret_borrow<py::int_>(min_neighbors);
            if (mv < py::int_(1) || mv > py::int_(256)) throw py::value_error("min_neighbors must be an int in 1..256");
            o.radius = spz::CleanOptions::Radius{r, py::cast<int>(mv)};
          }
          const bool details = py::cast<bool>(return_details);
          std::vector<uint8_t> mask;
          std::vector<double> scores;
          int64_t kept = 0;
          double thr = 0.0;
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::cleanSpz(input, output, o, &kept, details ? &mask : nullptr, details ? &scores : nullptr, &thr);
          }
          if (!ok) {
            raiseFailure("clean_spz: refused for this file (see the [SPZ ERROR] line)",
                         "clean_spz: " + input + " -> " + output + " failed (see the [SPZ ERROR] line)", true);
          }
          if (!details) return py::int_(kept);
          py::object sc = py::none(), th = py::none();
          if (o.statistical) {
            sc = toArray(scores);
            th = py::float_(thr);
          }
          return py::make_tuple(kept, toArray<uint8_t, bool>(mask), sc, th);
        },
        py::arg("input_filename"), py::arg("output_filename"), py::kw_only(), py::arg("k") = py::none(),
        py::arg("std_ratio") = 2.0, py::arg("radius") = py::none(), py::arg("min_neighbors") = py::none(),
        py::arg("return_details") = false,
        "Remove floaters from a v2/v3 file without requantising (spz::cleanSpz).  Statistical rule (k in 1..64): drop a "
        "point whose mean distance to its k nearest neighbours is above mean + std_ratio * std of all of them.  Radius "
        "rule (radius > 0 in world units, min_neighbors in 1..256): drop a point with fewer than min_neighbors others "
        "within radius.  Both: a point must pass both.  Returns the kept count, or (kept, mask (bool per input point), "
        "scores (float64, None without k), threshold (None without k)) when return_details.");
  m.def("save_spz",
        [](const spz::GaussianCloud &g, const spz::PackOptions &o, const std::string &filename) {
          bool ok;
          {
            py::gil_scoped_release release;
            ok = spz::saveSpz(g, o, filename);
          }
          if (!ok) raiseIfDeviceUnusable();
          return ok;
        },
        py::arg("gaussians"), py::arg("options"), py::arg("filename"), "Save a GaussianCloud to a *.spz* file.");
  // Extras of this implementation (underscore-prefixed: not part of the reference surface).
  m.def("_compress_gzipped", [](const py::bytes &data) {
    const BytesView in = viewOf(data);
    std::vector<uint8_t> out;
    bool ok;
    {
      py::gil_scoped_release release;
      ok = spz::compressGzipped(in.p, in.n, &out);
    }
    if (!ok) throw std::runtime_error("compressGzipped failed");
    return py::bytes(reinterpret_cast<const char *>(out.data()), out.size());
  }, "gzip wrapper of saveSpz (host zlib, parameters of load-spz.cc:190).");
  m.def("_compress_gzipped_parallel", [](const py::bytes &data, int threads) {
    const BytesView in = viewOf(data);
    std::vector<uint8_t> out;
    bool ok;
    {
      py::gil_scoped_release release;
      ok = spz::compressGzippedParallel(in.p, in.n, &out, threads);
    }
    if (!ok) throw std::runtime_error("compressGzippedParallel failed");
    return py::bytes(reinterpret_cast<const char *>(out.data()), out.size());
  }, py::arg("data"), py::arg("threads"), "Opt-in multi-threaded gzip (one member, independent deflate blocks).");
  m.def("_compress_gzipped_exact", [](const py::bytes &data, int threads, int windows_per_chunk, size_t verify_prefix) -> py::object {
    const BytesView in = viewOf(data);
    std::vector<uint8_t> out;
    bool ok;
    {
      py::gil_scoped_release release;
      ok = spz::exactgz::compress(in.p, in.n, threads, windows_per_chunk, &out,
                                  verify_prefix);
    }
    if (!ok) return py::none();
    return py::bytes(reinterpret_cast<const char *>(out.data()), out.size());
  }, py::arg("data"), py::arg("threads") = 8, py::arg("windows_per_chunk") = 32, py::arg("verify_prefix") = 0,
     "The multi-threaded writer with zlib's exact bytes (None when it declines the input).");
  m.def("_compress_gzipped_exact_model", [](const py::bytes &data, int threads, size_t verify_prefix) -> py::object {
    const BytesView in = viewOf(data);
    std::vector<uint8_t> out;
    bool ok;
    {
      py::gil_scoped_release release;
      std::unique_ptr<spz::exactgz::HeadParser> parser(spz::exactgz::newModelHeadParser());
      ok = spz::exactgz::compressWithHeadParser(in.p, in.n, threads, *parser, &out, verify_prefix);
    }
    if (!ok) return py::none();
    return py::bytes(reinterpret_cast<const char *>(out.data()), out.size());
  }, py::arg("data"), py::arg("threads") = 4, py::arg("verify_prefix") = 0,
     "Test hook: the exact writer with its parse done by the serial host model of the device stages "
     "(links, match tables, lazy state machine, record-window splice); None when declined.");
  m.def("_device_inflate_count", []() { return spz::deviceInflateCount(); },
        "gzip members inflated on the device so far.");
  m.def("_device_inflate_last_decline", []() { return std::string(spz::deviceInflateLastDecline()); },
        "Why the device reader last stood down on this thread ('' = it did not).");
  m.def("_device_gzip_parse_count", []() { return spz::deviceGzipParseCount(); },
        "gzip members written so far with their LZ77 parse done on the device.");
  m.def("_device_gzip_reject_count", []() { return spz::deviceGzipRejectCount(); },
        "members of the device gzip writer discarded because one of its self-checks failed.");
  m.def("_effective_cpu_count", []() { return spz::effectiveCpuCount(); },
        "CPUs the worker pools of the container stage size themselves by (online, affinity mask, cgroup quota).");
  m.def("_parallel_inflate_count", []() { return spz::pinflate::successCount(); },
        "Members inflated by the parallel single-stream reader so far in this process.");
  m.def("_decompress_gzipped", [](const py::bytes &data) -> py::object {
    const BytesView in = viewOf(data);
    std::vector<uint8_t> out;
    bool ok;
    {
      py::gil_scoped_release release;
      ok = spz::decompressGzipped(in.p, in.n, &out);
    }
    if (!ok) return py::none();
    return py::bytes(reinterpret_cast<const char *>(out.data()), out.size());
  }, "Inverse of _compress_gzipped; None on failure.");
  m.def("_save_spz_bytes", [](const spz::GaussianCloud &g, const spz::PackOptions &o) -> py::object {
    std::vector<uint8_t> out;
    bool ok;
    {
      py::gil_scoped_release release;
      ok = spz::saveSpz(g, o, &out);
    }
    if (!ok) {
      raiseIfDeviceUnusable();
      return py::none();
    }
    return py::bytes(reinterpret_cast<const char *>(out.data()), out.size());
  }, py::arg("gaussians"), py::arg("options"), "saveSpz(cloud, options, &vector) -> .spz bytes in memory.");
  m.def("_load_spz_bytes", [](const py::bytes &data, const spz::UnpackOptions &o) {
    const BytesView in = viewOf(data);
    spz::GaussianCloud g;
    {
      py::gil_scoped_release release;
      g = spz::loadSpz(in.p, static_cast<int32_t>(in.n), o);
    }
    if (g.numPoints == 0) raiseIfDeviceUnusable();
    return g;
  }, py::arg("data"), py::arg("options") = spz::UnpackOptions(), "loadSpz(ptr, size, options) from .spz bytes.");
  m.def("_packed_unpack", [](const py::bytes &data, int32_t index, spz::CoordinateSystem from, spz::CoordinateSystem to,
                              bool gzipped) -> py::object {
    // loadSpzPacked (or deserializePackedGaussians for a raw stream) + PackedGaussians::at / unpack:
    // returns (65 packed bytes, 59 floats) in the field order of PackedGaussian / UnpackedGaussian.
    const BytesView in = viewOf(data);
    spz::PackedGaussians packed;
    if (gzipped) {
      packed = spz::loadSpzPacked(in.p, static_cast<int32_t>(in.n));
    } else {
      std::istringstream ss(std::string(reinterpret_cast<const char *>(in.p), in.n));
      packed = spz::deserializePackedGaussians(ss);
    }
    if (index < 0 || index >= packed.numPoints) return py::none();
    spz::setLastDeviceStatus(SPZ_AMD_OK);
    const spz::PackedGaussian one = packed.at(index);
    const spz::UnpackedGaussian u = packed.unpack(index, spz::coordinateConverter(from, to));
    raiseIfDeviceUnusable();
    std::string b;
    auto putb = [&](const uint8_t *p, size_t n) { b.append(reinterpret_cast<const char *>(p), n); };
    putb(one.position.data(), 9); putb(one.rotation.data(), 4); putb(one.scale.data(), 3); putb(one.color.data(), 3);
    putb(&one.alpha, 1); putb(one.shR.data(), 15); putb(one.shG.data(), 15); putb(one.shB.data(), 15);
    std::vector<float> f;
    auto putf = [&](const float *p, size_t n) { f.insert(f.end(), p, p + n); };
    putf(u.position.data(), 3); putf(u.rotation.data(), 4); putf(u.scale.data(), 3); putf(u.color.data(), 3);
    putf(&u.alpha, 1); putf(u.shR.data(), 15); putf(u.shG.data(), 15); putf(u.shB.data(), 15);
    return py::make_tuple(py::bytes(b), toArray(f));
  }, py::arg("data"), py::arg("index"), py::arg("from_coord"), py::arg("to_coord"), py::arg("gzipped") = true,
     "PackedGaussians::at(i) bytes and PackedGaussians::unpack(i, coordinateConverter(from, to)) floats.");
  m.def("_unpack_indices", [](const py::bytes &data, const std::vector<uint32_t> &indices, const spz::UnpackOptions &o,
                               bool gzipped) {
    const BytesView in = viewOf(data);
    spz::PackedGaussians packed;
    if (gzipped) {
      packed = spz::loadSpzPacked(in.p, static_cast<int32_t>(in.n));
    } else {
      std::istringstream ss(std::string(reinterpret_cast<const char *>(in.p), in.n));
      packed = spz::deserializePackedGaussians(ss);
    }
    spz::setLastDeviceStatus(SPZ_AMD_OK);
    spz::GaussianCloud g = spz::unpackIndices(packed, indices, o);
    if (g.numPoints == 0) raiseIfDeviceUnusable();
    return g;
  }, py::arg("data"), py::arg("indices"), py::arg("options") = spz::UnpackOptions(), py::arg("gzipped") = true,
     "unpackIndices(loadSpzPacked(data), indices, options): one gather launch.");
  m.def("_unpack_from_stream", [](const py::bytes &data, const spz::UnpackOptions &o) {
    const BytesView in = viewOf(data);
    spz::GaussianCloud g = spz::unpackFromStream(in.p, in.n, o);
    if (g.numPoints == 0) raiseIfDeviceUnusable();
    return g;
  }, py::arg("data"), py::arg("options") = spz::UnpackOptions(), "Cloud of a raw (pre-gzip) stream: loadSpz without the gunzip step.");
  m.def("_pack_unpack_seconds", [](const spz::GaussianCloud &g, const spz::PackOptions &o, const spz::UnpackOptions &u) {
    // spz::packToStream / spz::unpackFromStream timed around the C++ calls themselves (fresh vectors), without the copy
    // into a Python bytes object that _pack_to_stream pays on top
    std::vector<uint8_t> stream;
    auto t0 = std::chrono::steady_clock::now();
    const bool ok = spz::packToStream(g, o, &stream);
    const double pack_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!ok) raiseIfDeviceUnusable();
    t0 = std::chrono::steady_clock::now();
    spz::GaussianCloud back = spz::unpackFromStream(stream.data(), stream.size(), u);
    const double unpack_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return py::make_tuple(pack_s, unpack_s, static_cast<int64_t>(back.numPoints));
  }, py::arg("gaussians"), py::arg("pack_options"), py::arg("unpack_options"), "Seconds of packToStream and unpackFromStream at the C++ boundary.");
  m.def("_save_load_seconds", [](const spz::GaussianCloud &g, const spz::PackOptions &o, const spz::UnpackOptions &u) {
    // spz::saveSpz / spz::loadSpz (the reference's vector overloads, load-spz.h) timed around the C++ calls themselves
    std::vector<uint8_t> file;
    const uint64_t parses_before = spz::deviceGzipParseCount();
    auto t0 = std::chrono::steady_clock::now();
    const bool ok = spz::saveSpz(g, o, &file);
    const double save_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (!ok) raiseIfDeviceUnusable();
    const bool gzip_on_device = spz::deviceGzipParseCount() != parses_before;
    t0 = std::chrono::steady_clock::now();
    spz::GaussianCloud back = spz::loadSpz(file, u);
    const double load_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return py::make_tuple(save_s, load_s, static_cast<int64_t>(file.size()), static_cast<int64_t>(back.numPoints), gzip_on_device);
  }, py::arg("gaussians"), py::arg("pack_options"), py::arg("unpack_options"),
     "Seconds of saveSpz and loadSpz at the C++ boundary, file bytes, points read back, whether the gzip stage ran on the device.");
  m.def("_pack_to_stream", [](const spz::GaussianCloud &g, const spz::PackOptions &o) -> py::object {
    std::vector<uint8_t> out;
    if (!spz::packToStream(g, o, &out)) {
      raiseIfDeviceUnusable();
      return py::none();
    }
    return py::bytes(reinterpret_cast<const char *>(out.data()), out.size());
  }, py::arg("gaussians"), py::arg("options"), "Raw (pre-gzip) stream of a cloud.");

  m.def("load_splat_from_ply",
        [](const std::string &filename, const spz::UnpackOptions &o) {
          spz::setLastDeviceStatus(SPZ_AMD_OK);
          spz::GaussianCloud g = spz::loadSplatFromPly(filename, o);
          if (g.numPoints == 0) raiseIfDeviceUnusable();
          return g;
        },
        py::arg("filename"), py::arg("options") = spz::UnpackOptions(), "Read GaussianCloud data from a *.ply* file.");
  m.def("save_splat_to_ply",
        [](const spz::GaussianCloud &g, const spz::PackOptions &o, const std::string &filename) {
          spz::setLastDeviceStatus(SPZ_AMD_OK);
          const bool ok = spz::saveSplatToPly(g, o, filename);
          if (!ok) raiseIfDeviceUnusable();
          return ok;
        },
        py::arg("gaussians"), py::arg("options"), py::arg("filename"), "Write GaussianCloud data to a *.ply* file.");
  // the reader of 3DGS's cameras.json is plain Python (spz_amd/cameras.py)
  m.attr("load_3dgs_cameras") = py::module_::import("spz_amd.cameras").attr("load_3dgs_cameras");
  m.attr("unproject_depth") = py::module_::import("spz_amd.cameras").attr("unproject_depth");
}
