// spz_py_args.hpp — how spz_py.cpp reads what Python hands it and shapes what it hands back: one definition of every
// rule that more than one function of the module applies (numbers, flags, a path or bytes, view lists, the render
// frame, images, the failure of a call), then the options and results of each operation.  Every problem with an
// argument is a ValueError raised before any file is opened and before any device work.  Included by spz_py.cpp only.
//
// The surface is the reference's nanobind shim (src/python/spz/spz.cc:110-362) built with pybind11, so the dtype/ndim
// gate that nanobind's ndarray caster applies (numeric dtypes convert to float32, anything else -> TypeError
// "incompatible function arguments") is written out in `toFloatVector`.
#pragma once
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "spz_amd.h"
#include "spz_amd_host.hpp"

namespace py = pybind11;

namespace {
using View = spz::PruneOptions::View;
using FloatArray = py::array_t<float, py::array::c_style | py::array::forcecast>;

// ---- bytes and arrays ----------------------------------------------------------------------------------------------
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

// `f()` while other Python threads run (the library is re-entrant).
template <class F>
auto unlocked(F &&f) {
  py::gil_scoped_release release;
  return f();
}

// `o` as a numpy array, or an empty handle.
py::array arrayOrNull(const py::object &o) {
  py::array a;
  try {
    a = py::array::ensure(o);
  } catch (const py::error_already_set &) {
    PyErr_Clear();
  }
  return a;
}

// Accepts what nb::ndarray<numpy, float, ndim<1>, c_contig, device::cpu> accepts: a 1-D array (or
// array-like) of a bool/int/uint/float dtype, converted to float32.  Everything else is the
// overload-resolution failure nanobind reports.
std::vector<float> toFloatVector(const py::object &obj, const char *prop) {
  const py::array arr = arrayOrNull(obj);
  const char kind = arr ? arr.dtype().kind() : '?';
  if (!(kind == 'b' || kind == 'i' || kind == 'u' || kind == 'f') || arr.ndim() != 1) {
    throw py::type_error(std::string("__set__(): incompatible function arguments. ") + prop +
                         " expects a 1-D numeric numpy array convertible to float32");
  }
  FloatArray f(arr);
  return std::vector<float>(f.data(), f.data() + f.size());
}

// New owning 1-D copy (spz.cc:47-79), of element type E (a mask's bytes: bool).
template <class T, class E = T>
py::array_t<E> toArray(const std::vector<T> &v) {
  static_assert(sizeof(E) == sizeof(T), "a copy of the elements' bytes");
  py::array_t<E> a(static_cast<py::ssize_t>(v.size()));
  if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(T));
  return a;
}

// New owning float32 array of `shape` holding `v` (all of it, or nothing while v is empty).
py::array_t<float> toArray(const std::vector<float> &v, std::vector<py::ssize_t> shape) {
  py::array_t<float> a(std::move(shape));
  if (!v.empty()) std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(float));
  return a;
}

void ensureMultiple(const char *name, size_t size, size_t k) {  // spz.cc:27-37
  if (k == 0) throw py::value_error("internal error: divisor cannot be zero");
  if (size % k != 0) {
    throw py::value_error(std::string(name) + " length must be a multiple of " + std::to_string(k) + ", got " +
                          std::to_string(size));
  }
}

// A GaussianCloud array from its property: a multiple of k floats, and num_points * k of them once the positions
// have set num_points.  The array is replaced before the second check, as the shim does.
void setCloudArray(spz::GaussianCloud &c, std::vector<float> spz::GaussianCloud::*field, const py::object &o,
                   const char *name, size_t k) {
  std::vector<float> v = toFloatVector(o, name);
  ensureMultiple(name, v.size(), k);
  c.*field = std::move(v);
  if (c.numPoints > 0 && (c.*field).size() != static_cast<size_t>(c.numPoints) * k) {
    throw py::value_error(std::string(name) + " length must equal num_points" + (k == 1 ? "" : " * " + std::to_string(k)));
  }
}

// ---- the failure of a call -----------------------------------------------------------------------------------------
// The product has no CPU fallback: an unusable device is raised, not returned as an empty cloud.
void raiseIfDeviceUnusable() {
  const int st = spz::lastDeviceStatus();
  if (st == SPZ_AMD_ERR_NO_DEVICE || st == SPZ_AMD_ERR_HIP) {
    throw std::runtime_error(std::string("spz_amd: ") + spz_amd_status_string(st) +
                             " (the SPZ hot path runs on the GPU only)");
  }
}

// The exception of the failed call `op`: the unusable device's RuntimeError; the ValueError "op: refused [forWhat]"
// when the call refused its arguments (SPZ_AMD_ERR_INVALID_ARG, and SPZ_AMD_ERR_UNSUPPORTED where
// `unsupportedRefused`); else the RuntimeError "op[: route] failed".  Both point at the library's [SPZ ERROR] line.
[[noreturn]] void raiseFailure(const std::string &op, const std::string &forWhat = "", const std::string &route = "",
                               bool unsupportedRefused = false) {
  raiseIfDeviceUnusable();
  const int st = spz::lastDeviceStatus();
  const char *see = " (see the [SPZ ERROR] line)";
  if (st == SPZ_AMD_ERR_INVALID_ARG || (unsupportedRefused && st == SPZ_AMD_ERR_UNSUPPORTED)) {
    throw py::value_error(op + ": refused" + (forWhat.empty() ? "" : " " + forWhat) + see);
  }
  throw std::runtime_error(op + (route.empty() ? "" : ": " + route) + " failed" + see);
}
// The same of a file-to-file call: refused "for this file", failed "input -> output".
[[noreturn]] void raiseFileFailure(const std::string &op, const std::string &input, const std::string &output,
                                   bool unsupportedRefused = false) {
  raiseFailure(op, "for this file", input + " -> " + output, unsupportedRefused);
}

// ---- numbers and flags ---------------------------------------------------------------------------------------------
bool isInt(const py::handle &v) { return py::isinstance<py::int_>(v) && !py::isinstance<py::bool_>(v); }  // not a bool
bool isReal(const py::handle &v) { return py::isinstance<py::float_>(v) || isInt(v); }                    // not a bool

// v when it is an int (not a bool) in [lo, hi], compared as Python ints so that no value wraps.
template <class T>
std::optional<T> asIntIn(const py::handle &v, T lo, T hi) {
  if (!isInt(v) || v < py::int_(lo) || v > py::int_(hi)) return std::nullopt;
  return py::cast<T>(v);
}

// The int parameter in [lo, hi], or the ValueError `what`.
template <class T>
T intIn(const py::handle &v, T lo, T hi, const std::string &what) {
  const std::optional<T> x = asIntIn(v, lo, hi);
  if (!x) throw py::value_error(what);
  return *x;
}
// filter, transform and merge word the rule "<name> must be [None or ]an int in [lo, hi]" and name an int out of range.
int32_t intInBrackets(const py::handle &v, int lo, int hi, const std::string &name, bool orNone) {
  const std::string what = name + " must be " + (orNone ? "None or " : "") + "an int in [" + std::to_string(lo) + ", " +
                           std::to_string(hi) + "]";
  return intIn(v, lo, hi, isInt(v) ? what + ", got " + std::to_string(py::cast<long>(v)) : what);
}

// x when it is finite and within the bound, else the ValueError `what`.
enum class Bound { Any, Positive, NonNegative };
double finite(double x, Bound bound, const std::string &what) {
  if (!std::isfinite(x) || (bound == Bound::Positive && !(x > 0.0)) || (bound == Bound::NonNegative && x < 0.0)) {
    throw py::value_error(what);
  }
  return x;
}
// The same of an object that must be a real number (an int or a float, not a bool).
double finiteReal(const py::handle &v, Bound bound, const std::string &what) {
  if (!isReal(v)) throw py::value_error(what);
  return finite(py::cast<double>(v), bound, what);
}

bool flag(const py::handle &v, const char *name) {
  if (!py::isinstance<py::bool_>(v)) throw py::value_error(std::string(name) + " must be a bool");
  return py::cast<bool>(v);
}

// ---- a .spz file: a path, or the file's bytes ----------------------------------------------------------------------
struct Input {
  std::optional<BytesView> bytes;
  std::string path;
  explicit Input(const py::object &o) {
    if (py::isinstance<py::bytes>(o)) {
      // viewed in place, not copied: the caller's argument keeps the object alive for the whole call, and a bytes
      // object is immutable, so the view stays valid while the GIL is released
      bytes = viewOf(py::reinterpret_borrow<py::bytes>(o));
      if (bytes->n > static_cast<size_t>(INT32_MAX)) throw py::value_error("an input is larger than 2 GiB");
    } else {
      path = py::str(o).cast<std::string>();
    }
  }
};

// f(data, size) or f(path), whichever `in` holds, without the GIL: the bytes overload or the path overload of a host
// function when f passes `file...` on.
template <class F>
auto callOn(const Input &in, F &&f) {
  py::gil_scoped_release release;
  return in.bytes ? f(in.bytes->p, static_cast<int32_t>(in.bytes->n)) : f(in.path);
}
// The same of two files, f(dataA, sizeA, dataB, sizeB) or f(pathA, pathB); a path with bytes is a ValueError.
template <class F>
auto callOn(const Input &a, const Input &b, const char *nameA, const char *nameB, F &&f) {
  if (a.bytes.has_value() != b.bytes.has_value()) {
    throw py::value_error(std::string("give ") + nameA + " and " + nameB + " both as paths or both as bytes");
  }
  py::gil_scoped_release release;
  return a.bytes ? f(a.bytes->p, static_cast<int32_t>(a.bytes->n), b.bytes->p, static_cast<int32_t>(b.bytes->n))
                 : f(a.path, b.path);
}

// ---- views ---------------------------------------------------------------------------------------------------------
// The part of a view that select_tiles has too: the pose and the focal lengths.
void setPose(View &v, const float *worldToCamera, float fx, float fy) {
  std::copy(worldToCamera, worldToCamera + 12, v.worldToCamera.begin());
  v.fx = fx;
  v.fy = fy;
}

// The 3x4 world_to_camera of a camera argument; `at` names the view it belongs to.
FloatArray poseArray(const py::handle &o, const std::string &at = "") {
  FloatArray m(py::reinterpret_borrow<py::object>(o));
  if (m.ndim() != 2 || m.shape(0) != 3 || m.shape(1) != 4) throw py::value_error(at + "world_to_camera must be 3x4");
  return m;
}

// A view from a mapping with world_to_camera (3x4), fx, fy, cx, cy, width, height (what orbit_views and
// load_3dgs_cameras return); every problem is a ValueError that names the view.
View pruneView(const py::handle &h, size_t k, spz::CoordinateSystem coord, float near_plane) {
  const std::string at = "view " + std::to_string(k) + ": ";
  if (!py::isinstance<py::dict>(h)) throw py::value_error(at + "must be a dict (world_to_camera, fx, fy, cx, cy, width, height)");
  const py::dict d = py::reinterpret_borrow<py::dict>(h);
  for (const char *key : {"world_to_camera", "fx", "fy", "cx", "cy", "width", "height"}) {
    if (!d.contains(key)) throw py::value_error(at + "has no " + key);
  }
  if (d.contains("coord") && !d["coord"].is_none() && d["coord"].cast<spz::CoordinateSystem>() != coord) {
    throw py::value_error(at + "its coord differs from the prune's coord (every view is in one frame)");
  }
  View v;
  const FloatArray m = poseArray(d["world_to_camera"], at);
  try {
    setPose(v, m.data(), d["fx"].cast<float>(), d["fy"].cast<float>());
    v.cx = d["cx"].cast<float>();
    v.cy = d["cy"].cast<float>();
    v.width = d["width"].cast<int>();
    v.height = d["height"].cast<int>();
  } catch (const py::cast_error &) {
    throw py::value_error(at + "fx, fy, cx, cy must be numbers and width, height ints");
  }
  spz_amd_render_params p = {};
  std::copy(v.worldToCamera.begin(), v.worldToCamera.end(), p.world_to_camera);
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

// A sequence of 1..maxViews view dicts.
std::vector<View> viewList(const py::object &views, size_t maxViews, spz::CoordinateSystem coord, float near_plane) {
  if (py::isinstance<py::dict>(views) || py::isinstance<py::str>(views) || !py::isinstance<py::sequence>(views)) {
    throw py::value_error("views must be a sequence of view dicts (orbit_views, load_3dgs_cameras)");
  }
  const py::sequence seq = py::reinterpret_borrow<py::sequence>(views);
  if (seq.size() < 1 || seq.size() > maxViews) {
    throw py::value_error("give 1.." + std::to_string(maxViews) + " views, got " + std::to_string(seq.size()));
  }
  std::vector<View> out;
  for (size_t k = 0; k < seq.size(); ++k) out.push_back(pruneView(seq[k], k, coord, near_plane));
  return out;
}

py::dict viewDict(const View &v) {
  py::dict d;
  d["world_to_camera"] = toArray(std::vector<float>(v.worldToCamera.begin(), v.worldToCamera.end()), {3, 4});
  d["fx"] = v.fx;
  d["fy"] = v.fy;
  d["cx"] = v.cx;
  d["cy"] = v.cy;
  d["width"] = v.width;
  d["height"] = v.height;
  return d;
}
py::list viewDicts(const std::vector<View> &views) {
  py::list out;
  for (const View &v : views) out.append(viewDict(v));
  return out;
}

// ---- the render frame, the optimiser, images -----------------------------------------------------------------------
// coord, near, max_sh_degree and background into the options of a render, compare, refine or locate.  `checked`: near
// must be > 0, max_sh_degree 0..3 and the background finite; render_* leaves those three to the host layer's camera
// check, whose refusal is the ValueError there (so a non-finite background is "refused", not "must be finite").
template <class Options>
void frameInto(Options &o, spz::CoordinateSystem coord, float near_plane, int max_sh_degree, const py::object &background,
               bool checked) {
  if (checked) finite(near_plane, Bound::Positive, "near must be > 0");
  if (checked && (max_sh_degree < 0 || max_sh_degree > 3)) throw py::value_error("max_sh_degree must be 0..3");
  FloatArray bg(background);
  if (bg.size() != 3) throw py::value_error("background must have three values");
  for (int k = 0; k < 3; ++k) {
    o.background[k] = bg.data()[k];
    if (checked && !std::isfinite(o.background[k])) throw py::value_error("background must be finite");
  }
  o.coord = coord;
  o.nearPlane = near_plane;
  o.maxShDegree = max_sh_degree;
}

// The loss weight and Adam's constants into the options of a refine or a locate.
template <class Options>
void optimiserInto(Options &o, double lambda_dssim, double beta1, double beta2, double eps) {
  if (!(lambda_dssim >= 0.0 && lambda_dssim <= 1.0)) throw py::value_error("lambda_dssim must be in [0, 1]");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) {
    throw py::value_error("beta1 and beta2 must be in [0, 1)");
  }
  o.lambdaDssim = lambda_dssim;
  o.beta1 = beta1;
  o.beta2 = beta2;
  o.eps = finite(eps, Bound::NonNegative, "eps must be finite and >= 0");
}

// RenderOptions from render_spz / render_cloud's keyword arguments (the camera itself is checked by the C++ layer).
spz::RenderOptions renderOptions(const py::object &world_to_camera, int width, int height, float fx, float fy, float cx,
                                 float cy, float near_plane, const py::object &background, int max_sh_degree,
                                 spz::CoordinateSystem coord) {
  spz::RenderOptions o;
  const FloatArray m = poseArray(world_to_camera);
  std::copy(m.data(), m.data() + 12, o.worldToCamera.begin());
  frameInto(o, coord, near_plane, max_sh_degree, background, /*checked=*/false);
  o.width = width;
  o.height = height;
  o.fx = fx;
  o.fy = fy;
  o.cx = cx;
  o.cy = cy;
  return o;
}

// The float32 (height, width, 3 or 4) image of the parameter `name`, C-contiguous; of the view's size where one is given.
FloatArray imageArray(const py::object &o, const char *name, const View *view = nullptr) {
  if (!py::isinstance<py::array>(o)) throw py::value_error(std::string(name) + " must be a numpy array");
  const py::array arr = py::reinterpret_borrow<py::array>(o);
  if (!arr.dtype().is(py::dtype::of<float>())) throw py::value_error(std::string(name) + " must be float32");
  if (arr.ndim() != 3 || (arr.shape(2) != 3 && arr.shape(2) != 4) ||
      (view && (arr.shape(0) != view->height || arr.shape(1) != view->width))) {
    throw py::value_error(std::string(name) + " must be " + (view ? "the view's " : "") + "height x width x 3 or 4");
  }
  return FloatArray(arr);
}

// ---- results -------------------------------------------------------------------------------------------------------
// The (height, width, 4) array of a render, or the exception of its failure.
py::object renderedImage(bool ok, const std::vector<float> &img, const spz::RenderOptions &o, const char *op) {
  if (!ok) raiseFailure(op);
  return toArray(img, {o.height, o.width, 4});
}

// The dict of a depth render (each map (height, width); index int32 with -1 for none), or the exception of its failure.
py::object renderedDepth(bool ok, const spz::DepthMaps &maps, const spz::RenderOptions &o, const char *op) {
  if (!ok) raiseFailure(op);
  py::dict d;
  d["expected"] = toArray(maps.expected, {o.height, o.width});
  d["median"] = toArray(maps.median, {o.height, o.width});
  d["accumulated"] = toArray(maps.accumulated, {o.height, o.width});
  d["alpha"] = toArray(maps.alpha, {o.height, o.width});
  py::array_t<int32_t> idx(std::vector<py::ssize_t>{o.height, o.width});
  std::memcpy(idx.mutable_data(), maps.index.data(), maps.index.size() * sizeof(uint32_t));  // 0xffffffff reads as -1
  d["index"] = idx;
  return d;
}

// compare_spz / compare_images' result of one image pair, with the SSIM map where one was asked for.
py::dict metricsDict(const spz::ImageMetrics &m, const std::vector<float> *ssimMap = nullptr, int height = 0, int width = 0) {
  py::dict d;
  d["mse"] = m.mse;
  d["psnr"] = m.psnr;
  d["ssim"] = m.ssim;
  d["l1"] = m.l1;
  d["max_abs"] = m.maxAbs;
  if (ssimMap) d["ssim_map"] = toArray(*ssimMap, {height, width});
  return d;
}
py::list metricsDicts(const std::vector<spz::ImageMetrics> &metrics, const std::vector<std::vector<float>> *ssimMaps = nullptr,
                      const std::vector<View> *views = nullptr) {
  py::list out;
  for (size_t v = 0; v < metrics.size(); ++v) {
    out.append(ssimMaps ? metricsDict(metrics[v], &(*ssimMaps)[v], (*views)[v].height, (*views)[v].width)
                        : metricsDict(metrics[v]));
  }
  return out;
}

// decimate_spz's (level, points), with the parents where they were asked for.
py::object decimateResult(int level, int64_t points, const std::vector<uint32_t> *parents) {
  if (!parents) return py::make_tuple(level, points);
  return py::make_tuple(level, points, toArray(*parents));
}

// prune_spz's kept count, or with `details` (kept, mask, weight_sum, weight_max).
py::object pruneResult(int64_t kept, bool details, const std::vector<uint8_t> &mask, const std::vector<uint64_t> &sums,
                       const std::vector<float> &maxima) {
  if (!details) return py::int_(kept);
  return py::make_tuple(kept, toArray<uint8_t, bool>(mask), toArray(sums), toArray(maxima));
}

// clean_spz's kept count, or with `details` (kept, mask, scores, threshold), the last two None without the
// statistical rule.
py::object cleanResult(int64_t kept, bool details, const std::vector<uint8_t> &mask, bool statistical,
                       const std::vector<double> &scores, double threshold) {
  if (!details) return py::int_(kept);
  if (!statistical) return py::make_tuple(kept, toArray<uint8_t, bool>(mask), py::none(), py::none());
  return py::make_tuple(kept, toArray<uint8_t, bool>(mask), toArray(scores), threshold);
}

py::dict alignDict(const spz::AlignResult &r) {
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
}

// level_spz's result: the planes, the first plane's placement, the labels and the stages' times.
py::dict levelDict(const spz::LevelResult &r) {
  py::dict d;
  py::list planes;
  for (const spz::DetectedPlane &p : r.planes) {
    py::dict q;
    q["integers"] = py::make_tuple(p.normalInt[0], p.normalInt[1], p.normalInt[2], p.offsetInt);
    q["normal"] = py::make_tuple(p.normal[0], p.normal[1], p.normal[2]);
    q["offset"] = p.offset;
    q["inliers"] = p.inliers;
    q["sum_abs"] = p.sumAbs;
    q["points"] = p.points;
    q["above"] = p.above;
    q["below"] = p.below;
    q["best_hypothesis"] = p.bestHypothesis;
    q["refinements"] = p.refinements;
    q["fitness"] = p.fitness;
    q["mean_distance"] = p.meanDistance;
    q["rotation"] = py::make_tuple(p.rotation[0], p.rotation[1], p.rotation[2], p.rotation[3]);
    q["translation"] = py::make_tuple(p.translation[0], p.translation[1], p.translation[2]);
    planes.append(q);
  }
  d["planes"] = planes;
  if (r.planes.empty()) {
    d["rotation"] = py::none();
    d["translation"] = py::none();
  } else {
    d["rotation"] = planes[0]["rotation"];
    d["translation"] = planes[0]["translation"];
  }
  d["scale"] = 1.0;
  d["threshold"] = r.threshold;
  d["labels"] = toArray(r.labels);
  d["kept"] = r.kept < 0 ? py::object(py::none()) : py::object(py::int_(r.kept));
  d["ms"] = py::make_tuple(r.prepareMs, r.scoreMs, r.refineMs);
  return d;
}

// refine_spz's report; `data` is the written file where the inputs were bytes.
py::dict refineDict(const spz::RefineReport &rep, const std::vector<uint8_t> *data) {
  py::dict d;
  d["history"] = rep.history;
  d["before"] = metricsDicts(rep.before);
  d["after"] = metricsDicts(rep.after);
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
  if (data) d["data"] = py::bytes(reinterpret_cast<const char *>(data->data()), data->size());
  return d;
}

// locate_spz's (view, report).
auto locateResult(const spz::LocateReport &rep) {
  py::dict d;
  d["history"] = rep.history;
  d["before"] = metricsDict(rep.before);
  d["after"] = metricsDict(rep.after);
  d["iterations"] = rep.iterations;
  d["lr_translation"] = rep.translationLr;
  d["ms"] = py::make_tuple(rep.ms[0], rep.ms[1], rep.ms[2]);
  return py::make_tuple(viewDict(rep.view), d);
}

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

// ---- the options of each operation ---------------------------------------------------------------------------------
// A numpy array of one of `kinds` (dtype kind letters) for the parameter `name`; `mustBe` ends the ValueError.
py::array arrayOfKind(const py::object &o, const char *name, const char *kinds, const char *mustBe) {
  const py::array a = arrayOrNull(o);
  if (!a) throw py::value_error(std::string(name) + " must be a numpy array");
  if (!std::strchr(kinds, a.dtype().kind())) throw py::value_error(std::string(name) + " must be " + mustBe);
  return a;
}

// filter_spz's arguments as spz::FilterOptions.
spz::FilterOptions filterOptions(const py::object &mask, const py::object &indices, const py::object &box,
                                 spz::CoordinateSystem coord, const py::object &min_alpha, const py::object &sh_degree) {
  spz::FilterOptions f;
  f.coord = coord;
  if (!sh_degree.is_none()) f.shDegree = intInBrackets(sh_degree, -1, 3, "sh_degree", /*orNone=*/true);
  if (!indices.is_none() && (!mask.is_none() || !box.is_none() || !min_alpha.is_none())) {
    throw py::value_error("indices cannot be combined with mask, box or min_alpha");
  }
  if (!box.is_none()) {
    const py::array a = arrayOfKind(box, "box", "iuf", "numeric");
    if (a.ndim() != 2 || a.shape(0) != 2 || a.shape(1) != 3) throw py::value_error("box must have shape (2, 3): [[x0, y0, z0], [x1, y1, z1]]");
    FloatArray b(a);
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
    const py::array a = arrayOfKind(mask, "mask", "biu", "a bool or integer array");
    if (a.ndim() != 1) throw py::value_error("mask must be one-dimensional");
    py::array_t<bool, py::array::c_style | py::array::forcecast> b(a);
    std::vector<uint8_t> v(static_cast<size_t>(b.size()));
    const bool *q = b.data();
    for (size_t i = 0; i < v.size(); ++i) v[i] = q[i] ? 1 : 0;
    f.mask = std::move(v);
  }
  if (!indices.is_none()) {
    const py::array a = arrayOfKind(indices, "indices", "iu", "an integer array");
    if (a.ndim() != 1) throw py::value_error("indices must be one-dimensional");
    if (static_cast<uint64_t>(a.size()) > SPZ_AMD_REFERENCE_MAX_POINTS) throw py::value_error("more than 10 M indices: the reference reads at most 10 M points");
    std::vector<uint32_t> v(static_cast<size_t>(a.size()));
    if (a.dtype().kind() == 'u') {
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

// The n finite numbers of a transform's rotation or translation.
std::vector<double> finiteVector(const py::object &v, size_t n, const char *name) {
  const std::string what = std::string(name) + " must be a sequence of " + std::to_string(n) + " finite numbers";
  const py::array a = arrayOrNull(v);
  if (!a || !std::strchr("iuf", a.dtype().kind()) || a.ndim() != 1 || static_cast<size_t>(a.size()) != n) {
    throw py::value_error(what);
  }
  py::array_t<double, py::array::c_style | py::array::forcecast> d(a);
  std::vector<double> out(d.data(), d.data() + n);
  for (double x : out) finite(x, Bound::Any, what);
  return out;
}

// transform_spz / transform_cloud's arguments as spz::TransformOptions (the parameter block is built on the host,
// spz_amd_transform_params).
spz::TransformOptions transformOptions(const py::object &rotation, const py::object &translation, const py::object &scale,
                                       spz::CoordinateSystem coord, const py::object &fractional_bits) {
  spz::TransformOptions o;
  o.coord = coord;
  if (!rotation.is_none()) {
    const std::vector<double> q = finiteVector(rotation, 4, "rotation (x, y, z, w)");
    std::copy(q.begin(), q.end(), o.rotation.begin());
    if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0) throw py::value_error("rotation must not be zero");
  }
  if (!translation.is_none()) {
    const std::vector<double> t = finiteVector(translation, 3, "translation (x, y, z)");
    std::copy(t.begin(), t.end(), o.translation.begin());
  }
  if (!isReal(scale)) throw py::value_error("scale must be a number");
  o.scale = finite(py::cast<double>(scale), Bound::Positive, "scale must be finite and > 0");
  o.fractionalBits = intInBrackets(fractional_bits, 0, 24, "fractional_bits", /*orNone=*/false);
  spz_amd_transform xf;
  if (spz_amd_transform_params(o.rotation.data(), o.translation.data(), o.scale, static_cast<int>(coord), &xf) != SPZ_AMD_OK) {
    throw py::value_error("the transform has no f32 parameter block (scale or translation out of the f32 range?)");
  }
  return o;
}

// merge_spz's arguments as spz::MergeOptions.  Each transforms entry is None or a dict of rotation / translation /
// scale / coord, checked by transform_spz's code.
spz::MergeOptions mergeOptions(size_t k, const py::object &transforms, const py::object &sh_degree,
                               const py::object &fractional_bits, const py::object &antialiased) {
  spz::MergeOptions o;
  if (!sh_degree.is_none()) o.shDegree = intInBrackets(sh_degree, 0, 3, "sh_degree", /*orNone=*/true);
  if (!fractional_bits.is_none()) o.fractionalBits = intInBrackets(fractional_bits, 0, 24, "fractional_bits", true);
  if (!antialiased.is_none()) o.antialiased = intInBrackets(antialiased, 0, 1, "antialiased", true);
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
    const std::string at = "transforms[" + std::to_string(i) + "]";
    const py::object e = seq[i];
    if (e.is_none()) {
      o.transforms.emplace_back(std::nullopt);
      continue;
    }
    if (!py::isinstance<py::dict>(e)) throw py::value_error(at + " must be None or a dict");
    const py::dict d = e.cast<py::dict>();
    for (const auto &kv : d) {
      const std::string key = py::str(kv.first);
      if (key != "rotation" && key != "translation" && key != "scale" && key != "coord") {
        throw py::value_error(at + ": unknown key '" + key + "'");
      }
    }
    spz::CoordinateSystem coord = spz::CoordinateSystem::UNSPECIFIED;
    if (d.contains("coord")) {
      const py::object c = d["coord"];
      if (py::isinstance<spz::CoordinateSystem>(c)) {
        coord = c.cast<spz::CoordinateSystem>();
      } else if (const std::optional<int> x = asIntIn(c, 0, 8)) {
        coord = static_cast<spz::CoordinateSystem>(*x);
      } else {
        throw py::value_error(at + ": coord must be a CoordinateSystem");
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

spz::SortOptions sortOptions(const py::object &keys, const py::object &descending) {
  spz::SortOptions o;
  o.descending = flag(descending, "descending");
  if (!keys.is_none()) {
    const char *what = "keys must be a 1-D float32 numpy array";
    if (!py::isinstance<py::array>(keys)) throw py::value_error(what);
    const py::array a = py::reinterpret_borrow<py::array>(keys);
    if (!a.dtype().is(py::dtype::of<float>()) || a.ndim() != 1) throw py::value_error(what);
    py::array_t<float, py::array::c_style> k(a);  // a copy only when `a` is strided
    o.keys = std::vector<float>(k.data(), k.data() + k.size());
  }
  return o;
}

spz::DecimateOptions decimateOptions(const py::object &level, const py::object &target) {
  if (level.is_none() == target.is_none()) throw py::value_error("give exactly one of level and target_points");
  spz::DecimateOptions o;
  if (!level.is_none()) {
    o.level = intIn(level, 0, 24, "level must be an int in 0..24");
  } else {
    o.targetPoints = intIn<uint64_t>(target, 1, UINT64_MAX, "target_points must be an int >= 1");
  }
  return o;
}

spz::TileOptions tileOptions(const py::object &max_points, const py::object &max_tiles, spz::CoordinateSystem coord) {
  spz::TileOptions o;
  o.maxPoints = intIn<uint32_t>(max_points, 1, 10000000, "max_points must be an int in 1..10000000");
  o.maxTiles = intIn<uint32_t>(max_tiles, 1, 2147483647, "max_tiles must be an int in 1..2^31 - 1");
  o.coord = coord;
  return o;
}

// prune_spz's arguments as spz::PruneOptions.
spz::PruneOptions pruneOptions(const py::object &views, const py::object &keep, const py::object &keep_fraction,
                               const py::object &min_score, const std::string &score, spz::CoordinateSystem coord,
                               float near_plane) {
  const int rules = (keep.is_none() ? 0 : 1) + (keep_fraction.is_none() ? 0 : 1) + (min_score.is_none() ? 0 : 1);
  if (rules != 1) throw py::value_error("give exactly one of keep, keep_fraction, min_score");
  spz::PruneOptions o;
  if (!keep.is_none()) o.keepCount = intIn<int64_t>(keep, 0, 0x7fffffff, "keep must be an int in 0..n");
  if (!keep_fraction.is_none()) {
    const char *what = "keep_fraction must be a number in [0, 1]";
    o.keepFraction = isReal(keep_fraction) ? py::cast<double>(keep_fraction) : -1.0;
    if (!(*o.keepFraction >= 0.0 && *o.keepFraction <= 1.0)) throw py::value_error(what);
  }
  if (!min_score.is_none()) o.minScore = finiteReal(min_score, Bound::Any, "min_score must be a finite number");
  if (score == "sum") {
    o.score = spz::PruneOptions::Sum;
  } else if (score == "max") {
    o.score = spz::PruneOptions::Max;
  } else {
    throw py::value_error("score must be 'sum' or 'max'");
  }
  o.coord = coord;
  o.nearPlane = static_cast<float>(finite(near_plane, Bound::Positive, "near_plane must be > 0"));
  o.views = viewList(views, SPZ_AMD_PRUNE_MAX_VIEWS, coord, near_plane);
  return o;
}

// align_spz's stride and max_iterations: one text for the type, one for the range.
uint32_t alignCount(const py::object &v, const std::string &name, uint32_t hi) {
  if (!isInt(v)) throw py::value_error(name + " must be an int");
  return intIn<uint32_t>(v, 1, hi, name + " must be in 1.." + std::to_string(hi));
}
// align_spz's arguments as spz::AlignOptions.
spz::AlignOptions alignOptions(const py::object &rotation, const py::object &translation, double scale,
                               spz::CoordinateSystem coord, bool estimate_scale, double overlap,
                               const py::object &max_distance, const py::object &stride, const py::object &max_iterations,
                               double relative_fitness, double relative_rmse, bool init_centroids) {
  spz::AlignOptions o;
  if (!rotation.is_none()) {
    py::array_t<double, py::array::c_style | py::array::forcecast> q(rotation);
    if (q.size() != 4) throw py::value_error("rotation must be (x, y, z, w)");
    std::copy(q.data(), q.data() + 4, o.rotation.begin());
  }
  if (!translation.is_none()) {
    py::array_t<double, py::array::c_style | py::array::forcecast> t(translation);
    if (t.size() != 3) throw py::value_error("translation must be (x, y, z)");
    std::copy(t.data(), t.data() + 3, o.translation.begin());
  }
  o.stride = alignCount(stride, "stride", 0xffffffffu);
  o.maxIterations = alignCount(max_iterations, "max_iterations", 1000);
  o.coord = coord;
  o.estimateScale = estimate_scale;
  o.relativeFitness = relative_fitness;
  o.relativeRmse = relative_rmse;
  o.initCentroids = init_centroids;
  if (!(overlap > 0.0) || !(overlap <= 1.0)) throw py::value_error("overlap must be in (0, 1]");
  o.overlap = overlap;
  if (!max_distance.is_none()) {
    o.maxDistance = finite(max_distance.cast<double>(), Bound::Positive, "max_distance must be None or a finite number > 0");
  }
  o.scale = finite(scale, Bound::Positive, "scale must be a finite number > 0");
  return o;
}

// A direction argument of level_spz: None, or three numbers.
std::optional<std::array<double, 3>> levelVector(const py::object &v, const char *name) {
  if (v.is_none()) return std::nullopt;
  py::array_t<double, py::array::c_style | py::array::forcecast> a(v);
  if (a.size() != 3) throw py::value_error(std::string(name) + " must be None or (x, y, z)");
  return std::array<double, 3>{a.data()[0], a.data()[1], a.data()[2]};
}
// level_spz's arguments as spz::LevelOptions.
spz::LevelOptions levelOptions(const py::object &threshold, const py::object &hypotheses, const py::object &seed,
                               const py::object &stride, const py::object &refine, const py::object &planes,
                               const py::object &min_inliers, const py::object &axis, const py::object &max_tilt,
                               const py::object &up_hint, spz::CoordinateSystem coord, bool no_translate,
                               const py::object &select, const py::object &fractional_bits) {
  spz::LevelOptions o;
  o.threshold = finiteReal(threshold, Bound::NonNegative, "threshold must be a finite number >= 0 (world units)");
  o.hypotheses = intIn<uint32_t>(hypotheses, 1, 65536, "hypotheses must be an int in 1..65536");
  o.seed = intIn<uint64_t>(seed, 0, UINT64_MAX, "seed must be an int in 0..2^64 - 1");
  o.stride = intIn<uint32_t>(stride, 1, 0xffffffffu, "stride must be an int >= 1");
  o.refine = intIn<uint32_t>(refine, 0, 16, "refine must be an int in 0..16");
  o.planes = intIn<uint32_t>(planes, 1, 255, "planes must be an int in 1..255");
  const char *floorText = "min_inliers must be an int >= 0 (a count) or a float in [0, 1] (a fraction)";
  if (isInt(min_inliers)) {
    o.minInliers = intIn<uint64_t>(min_inliers, 0, UINT64_MAX, floorText);
  } else {
    o.minInlierFraction = finiteReal(min_inliers, Bound::NonNegative, floorText);
    if (o.minInlierFraction > 1.0) throw py::value_error(floorText);
  }
  o.axis = levelVector(axis, "axis");
  o.upHint = levelVector(up_hint, "up_hint");
  if (o.axis.has_value() != !max_tilt.is_none()) throw py::value_error("give axis and max_tilt together");
  if (!max_tilt.is_none()) {
    o.maxTilt = finiteReal(max_tilt, Bound::NonNegative, "max_tilt must be a number in [0, 90] (degrees)");
    if (o.maxTilt > 90.0) throw py::value_error("max_tilt must be a number in [0, 90] (degrees)");
  }
  o.coord = coord;
  o.noTranslate = no_translate;
  if (!select.is_none()) {
    const std::string v = py::isinstance<py::str>(select) ? select.cast<std::string>() : "";
    if (v == "plane") o.select = spz::LevelOptions::Select::Plane;
    else if (v == "off-plane") o.select = spz::LevelOptions::Select::OffPlane;
    else if (v == "above") o.select = spz::LevelOptions::Select::Above;
    else if (v == "below") o.select = spz::LevelOptions::Select::Below;
    else throw py::value_error("select must be None, 'plane', 'off-plane', 'above' or 'below'");
  }
  o.fractionalBits = intInBrackets(fractional_bits, 0, 24, "fractional_bits", false);
  return o;
}

// ---- mesh ----------------------------------------------------------------------------------------------------------
// MeshOptions from mesh_spz's keyword arguments.
spz::MeshOptions meshOptions(const py::object &views, const py::object &box, const py::object &voxel_size,
                             const py::object &resolution, const py::object &truncation, const std::string &depth,
                             const py::object &min_alpha, const py::object &min_weight, float near_plane,
                             spz::CoordinateSystem coord) {
  spz::MeshOptions o;
  finite(near_plane, Bound::Positive, "near must be > 0");
  o.coord = coord;
  o.nearPlane = near_plane;
  if (!voxel_size.is_none() && !resolution.is_none()) throw py::value_error("give voxel_size or resolution, not both");
  if (!voxel_size.is_none()) o.voxelSize = finiteReal(voxel_size, Bound::Positive, "voxel_size must be a finite number > 0");
  if (!resolution.is_none()) o.resolution = intIn<int>(resolution, 1, 2046, "resolution must be an int in 1..2046");
  if (!truncation.is_none()) o.truncation = finiteReal(truncation, Bound::Positive, "truncation must be a finite number > 0");
  if (depth == "median") {
    o.depth = spz::MeshOptions::Median;
  } else if (depth == "expected") {
    o.depth = spz::MeshOptions::Expected;
  } else {
    throw py::value_error("depth must be 'median' or 'expected'");
  }
  const double a = finiteReal(min_alpha, Bound::NonNegative, "min_alpha must be a number in [0, 1]");
  if (a > 1.0) throw py::value_error("min_alpha must be a number in [0, 1]");
  o.minAlpha = static_cast<float>(a);
  o.minWeight = static_cast<float>(finiteReal(min_weight, Bound::Positive, "min_weight must be a finite number > 0"));
  if (!box.is_none()) {
    const char *what = "box must be six finite numbers x0, y0, z0, x1, y1, z1 with x1 > x0, y1 > y0, z1 > z0";
    if (py::isinstance<py::str>(box) || !py::isinstance<py::sequence>(box)) throw py::value_error(what);
    const py::sequence seq = py::reinterpret_borrow<py::sequence>(box);
    if (seq.size() != 6) throw py::value_error(what);
    std::array<double, 6> b;
    for (size_t k = 0; k < 6; ++k) b[k] = finiteReal(seq[k], Bound::Any, what);
    for (size_t k = 0; k < 3; ++k) {
      if (!(b[3 + k] > b[k])) throw py::value_error(what);
    }
    o.box = b;
  }
  o.views = viewList(views, SPZ_AMD_MESH_MAX_VIEWS, coord, near_plane);
  return o;
}

// The (n, 3) arrays of a triangle mesh argument: float32 vertices and colours of one length, uint32 triangles below it.
using IndexArray = py::array_t<uint32_t, py::array::c_style | py::array::forcecast>;
FloatArray meshFloats(const py::object &o, const char *name) {
  if (!py::isinstance<py::array>(o)) throw py::value_error(std::string(name) + " must be a numpy array of shape (n, 3)");
  FloatArray a(o);
  if (a.ndim() != 2 || a.shape(1) != 3) throw py::value_error(std::string(name) + " must be a numpy array of shape (n, 3)");
  return a;
}
IndexArray meshIndices(const py::object &o) {
  const char *what = "triangles must be an integer numpy array of shape (n, 3)";
  if (!py::isinstance<py::array>(o)) throw py::value_error(what);
  const py::array raw = py::reinterpret_borrow<py::array>(o);
  if (raw.ndim() != 2 || raw.shape(1) != 3 || (raw.dtype().kind() != 'i' && raw.dtype().kind() != 'u')) {
    throw py::value_error(what);
  }
  return IndexArray(o);
}

py::dict meshResult(const spz::TriangleMesh &m) {
  const py::ssize_t nv = static_cast<py::ssize_t>(m.vertices.size() / 3u), nt = static_cast<py::ssize_t>(m.triangles.size() / 3u);
  py::dict d, vol;
  d["vertices"] = toArray(m.vertices, {nv, 3});
  d["colors"] = toArray(m.colors, {nv, 3});
  py::array_t<uint32_t> tri(std::vector<py::ssize_t>{nt, 3});
  if (nt) std::memcpy(tri.mutable_data(), m.triangles.data(), m.triangles.size() * sizeof(uint32_t));
  d["triangles"] = tri;
  vol["lo"] = py::make_tuple(m.lo[0], m.lo[1], m.lo[2]);
  vol["voxel_size"] = m.voxelSize;
  vol["dims"] = py::make_tuple(m.dims[0], m.dims[1], m.dims[2]);
  vol["truncation"] = m.truncation;
  d["volume"] = vol;
  d["ms"] = py::make_tuple(m.ms[0], m.ms[1], m.ms[2]);
  return d;
}

// The index of a GaussianCloud array's name among positions, scales, rotations, alphas, colors, sh; `list` ("lrs",
// "train") names the argument in the ValueError.
int cloudArrayIndex(const std::string &name, const char *list) {
  static const char *const kArrays[6] = {"positions", "scales", "rotations", "alphas", "colors", "sh"};
  for (int k = 0; k < 6; ++k) {
    if (name == kArrays[k]) return k;
  }
  throw py::value_error(std::string(list) + ": unknown array '" + name + "'");
}

// refine_spz's densify: a dict, or an options object with the same names (spz_amd.abi.DensifyOptions).  `train` is the
// refine's mask of trained arrays.
spz::DensifyOptions densifyOptions(const py::object &densify, unsigned train) {
  spz::DensifyOptions dn;
  const std::pair<const char *, int *> ints[4] = {{"interval", &dn.interval}, {"from_iter", &dn.fromIter},
                                                  {"until_iter", &dn.untilIter},
                                                  {"opacity_reset_interval", &dn.opacityResetInterval}};
  const std::pair<const char *, double *> reals[5] = {{"grad_threshold", &dn.gradThreshold}, {"percent_dense", &dn.percentDense},
                                                      {"extent", &dn.extent}, {"min_opacity", &dn.minOpacity},
                                                      {"max_scale", &dn.maxScale}};
  const std::pair<const char *, uint64_t *> counts[2] = {{"max_points", &dn.maxPoints}, {"seed", &dn.seed}};
  const bool isDict = py::isinstance<py::dict>(densify);
  size_t known = 0;
  const char *wrong = "densify: a field has the wrong type or is out of range";
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
    for (const auto &f : ints) {
      const py::object x = field(f.first);
      if (!x.is_none()) *f.second = intIn(x, 0, 0x7fffffff, wrong);
    }
    for (const auto &f : reals) {
      const py::object x = field(f.first);
      if (!x.is_none()) *f.second = x.cast<double>();
    }
    for (const auto &f : counts) {
      const py::object x = field(f.first);
      if (!x.is_none()) *f.second = intIn<uint64_t>(x, 0, UINT64_MAX, wrong);
    }
  } catch (const py::cast_error &) {
    throw py::value_error(wrong);
  }
  if (isDict && known != py::reinterpret_borrow<py::dict>(densify).size()) {
    throw py::value_error("densify: unknown field (interval, from_iter, until_iter, opacity_reset_interval, "
                          "grad_threshold, percent_dense, extent, min_opacity, max_scale, max_points, seed)");
  }
  for (const auto &f : reals) finite(*f.second, Bound::NonNegative, "densify: values must be finite and >= 0");
  if (dn.untilIter < dn.fromIter) throw py::value_error("densify: until_iter is below from_iter");
  if (!(dn.minOpacity > 0.0 && dn.minOpacity < 1.0)) throw py::value_error("densify: min_opacity must be in (0, 1)");
  if (dn.interval > 0 && !(dn.percentDense > 0.0)) throw py::value_error("densify: percent_dense must be > 0");
  if (dn.interval > 0 && (train & 3u) != 3u) {
    throw py::value_error("densify needs positions and scales among the trained arrays");
  }
  if (dn.interval > 0 && dn.opacityResetInterval > 0 && (train & 8u) == 0u) {
    throw py::value_error("densify: the opacity reset needs alphas among the trained arrays");
  }
  return dn;
}

// refine_spz's arguments as spz::RefineOptions.
spz::RefineOptions refineOptions(const py::object &views, int iterations, spz::CoordinateSystem coord,
                                 const py::object &background, int max_sh_degree, float near_plane, double lambda_dssim,
                                 const py::object &lrs, double beta1, double beta2, double eps, const py::object &train,
                                 const py::object &densify) {
  spz::RefineOptions o;
  if (iterations < 0) throw py::value_error("iterations must be >= 0");
  o.iterations = iterations;
  frameInto(o, coord, near_plane, max_sh_degree, background, /*checked=*/true);
  optimiserInto(o, lambda_dssim, beta1, beta2, eps);
  if (!lrs.is_none()) {
    if (!py::isinstance<py::dict>(lrs)) throw py::value_error("lrs must be a dict by array name");
    double *const slot[6] = {nullptr, &o.scaleLr, &o.rotationLr, &o.alphaLr, &o.colorLr, &o.shLr};
    for (auto item : py::reinterpret_borrow<py::dict>(lrs)) {
      const std::string name = py::str(item.first).cast<std::string>();
      const double x = finite(py::cast<double>(item.second), Bound::NonNegative, "lrs[" + name + "] must be finite and >= 0");
      const int k = cloudArrayIndex(name, "lrs");
      if (k == 0) o.positionLr = x; else *slot[k] = x;
    }
  }
  if (!train.is_none()) {
    if (py::isinstance<py::str>(train) || !py::isinstance<py::sequence>(train)) {
      throw py::value_error("train must be a sequence of array names");
    }
    o.train = 0;
    for (auto item : py::reinterpret_borrow<py::sequence>(train)) {
      o.train |= 1u << cloudArrayIndex(py::str(item).cast<std::string>(), "train");
    }
    if (o.train == 0) throw py::value_error("train must name at least one array");
  }
  if (!densify.is_none()) o.densify = densifyOptions(densify, o.train);
  o.views = viewList(views, SPZ_AMD_REFINE_MAX_VIEWS, coord, near_plane);
  return o;
}

// refine_spz_to_images' images, weights and exposure arguments as spz::PhotoOptions; `keep` holds the arrays the
// options point into.
spz::PhotoOptions photoOptions(const py::object &images, const py::object &weights, const py::object &fit_exposure,
                               double lr_exposure, const std::vector<View> &views, std::vector<FloatArray> *keep) {
  spz::PhotoOptions p;
  p.fitExposure = flag(fit_exposure, "fit_exposure");
  p.exposureLr = finite(lr_exposure, Bound::NonNegative, "lr_exposure must be finite and >= 0");
  if (py::isinstance<py::str>(images) || py::isinstance<py::array>(images) || !py::isinstance<py::sequence>(images)) {
    throw py::value_error("images must be a sequence of numpy arrays, one per view");
  }
  const py::sequence ims = py::reinterpret_borrow<py::sequence>(images);
  if (ims.size() != views.size()) {
    throw py::value_error("images must have one array per view: " + std::to_string(views.size()) + " views, " +
                          std::to_string(ims.size()) + " images");
  }
  py::sequence wts;
  if (!weights.is_none()) {
    if (py::isinstance<py::str>(weights) || py::isinstance<py::array>(weights) || !py::isinstance<py::sequence>(weights)) {
      throw py::value_error("weights must be None or a sequence of numpy arrays or None, one per view");
    }
    wts = py::reinterpret_borrow<py::sequence>(weights);
    if (wts.size() != views.size()) {
      throw py::value_error("weights must have one entry per view: " + std::to_string(views.size()) + " views, " +
                            std::to_string(wts.size()) + " weights");
    }
  }
  keep->reserve(2 * views.size());
  for (size_t k = 0; k < views.size(); ++k) {
    const std::string name = "images[" + std::to_string(k) + "]";
    keep->push_back(imageArray(py::reinterpret_borrow<py::object>(ims[k]), name.c_str(), &views[k]));
    const FloatArray &im = keep->back();
    spz::PhotoImage pi;
    pi.pixels = im.data();
    pi.width = views[k].width;
    pi.height = views[k].height;
    pi.channels = static_cast<int>(im.shape(2));
    if (pi.channels != static_cast<int>((*keep)[0].shape(2))) {
      throw py::value_error(name + " has " + std::to_string(pi.channels) + " channels but images[0] has " +
                            std::to_string((*keep)[0].shape(2)));
    }
    p.images.push_back(pi);
  }
  for (size_t k = 0; !weights.is_none() && k < views.size(); ++k) {
    const py::object w = py::reinterpret_borrow<py::object>(wts[k]);
    if (w.is_none()) continue;
    const std::string bad = "weights[" + std::to_string(k) + "] must be a float32 array of the view's height x width";
    if (!py::isinstance<py::array>(w)) throw py::value_error(bad);
    const py::array arr = py::reinterpret_borrow<py::array>(w);
    if (!arr.dtype().is(py::dtype::of<float>()) || arr.ndim() != 2 || arr.shape(0) != views[k].height ||
        arr.shape(1) != views[k].width) {
      throw py::value_error(bad);
    }
    keep->push_back(FloatArray(arr));
    p.images[k].weights = keep->back().data();
  }
  return p;
}

// refine_spz_to_images' depths and depth_* arguments into p (after photoOptions: its checks come first).
void depthOptionsInto(spz::PhotoOptions &p, const py::object &depths, double depth_weight, const py::object &depth_kind,
                      double depth_min_alpha, const std::vector<View> &views, std::vector<FloatArray> *keep) {
  p.depthWeight = finite(depth_weight, Bound::NonNegative, "depth_weight must be finite and >= 0");
  if (!(depth_min_alpha > 0.0 && depth_min_alpha <= 1.0)) throw py::value_error("depth_min_alpha must be in (0, 1]");
  p.depthMinAlpha = static_cast<float>(depth_min_alpha);
  const std::string kind = py::isinstance<py::str>(depth_kind) ? depth_kind.cast<std::string>() : std::string();
  if (kind != "l1" && kind != "inverse") throw py::value_error("depth_kind must be 'l1' or 'inverse'");
  p.depthKind = kind == "l1" ? spz::PhotoOptions::L1 : spz::PhotoOptions::InverseL1;
  if (depths.is_none()) return;
  if (py::isinstance<py::str>(depths) || py::isinstance<py::array>(depths) || !py::isinstance<py::sequence>(depths)) {
    throw py::value_error("depths must be None or a sequence of numpy arrays or None, one per view");
  }
  const py::sequence ds = py::reinterpret_borrow<py::sequence>(depths);
  if (ds.size() != views.size()) {
    throw py::value_error("depths must have one entry per view: " + std::to_string(views.size()) + " views, " +
                          std::to_string(ds.size()) + " depths");
  }
  for (size_t k = 0; k < views.size(); ++k) {
    const py::object d = py::reinterpret_borrow<py::object>(ds[k]);
    if (d.is_none()) continue;
    const std::string bad = "depths[" + std::to_string(k) + "] must be a float32 array of the view's height x width";
    if (!py::isinstance<py::array>(d)) throw py::value_error(bad);
    const py::array arr = py::reinterpret_borrow<py::array>(d);
    if (!arr.dtype().is(py::dtype::of<float>()) || arr.ndim() != 2 || arr.shape(0) != views[k].height ||
        arr.shape(1) != views[k].width) {
      throw py::value_error(bad);
    }
    keep->push_back(FloatArray(arr));
    p.images[k].depth = keep->back().data();
  }
}

// seed_spz's keyword arguments as spz::SeedOptions (the views first: an image is checked against its view).
spz::SeedOptions seedOptions(const py::object &views, const py::object &base, const py::object &stride, double scale_factor,
                             double opacity, const py::object &cover, double cover_alpha, double cover_tolerance,
                             const py::object &sh_degree, const py::object &max_points, spz::CoordinateSystem coord,
                             float near_plane) {
  spz::SeedOptions o;
  finite(near_plane, Bound::Positive, "near_plane must be > 0");
  o.coord = coord;
  o.nearPlane = near_plane;
  o.stride = intIn<int>(stride, 1, 64, "stride must be an int in 1..64");
  o.scaleFactor = finite(scale_factor, Bound::Positive, "scale_factor must be finite and > 0");
  if (!(opacity > 0.0 && opacity < 1.0)) throw py::value_error("opacity must be in (0, 1)");
  o.opacity = opacity;
  o.cover = flag(cover, "cover");
  if (!(cover_alpha >= 0.0 && cover_alpha <= 1.0)) throw py::value_error("cover_alpha must be in [0, 1]");
  o.coverAlpha = static_cast<float>(cover_alpha);
  o.coverTolerance = static_cast<float>(finite(cover_tolerance, Bound::NonNegative, "cover_tolerance must be finite and >= 0"));
  o.shDegree = intIn<int>(sh_degree, 0, 3, "sh_degree must be an int in 0..3");
  o.maxPoints = intIn<uint64_t>(max_points, 0, SPZ_AMD_REFERENCE_MAX_POINTS, "max_points must be an int in 0..10000000");
  if (!base.is_none()) {
    const Input in(base);
    if (in.bytes) {
      o.baseData.assign(in.bytes->p, in.bytes->p + in.bytes->n);
      if (o.baseData.empty()) throw py::value_error("base must be a path or the bytes of a .spz file");
    } else {
      o.base = in.path;
    }
  }
  o.views = viewList(views, SPZ_AMD_SEED_MAX_VIEWS, coord, near_plane);
  return o;
}

py::dict seedDict(const spz::SeedReport &rep, const std::vector<uint8_t> *data) {
  py::dict d;
  py::list views;
  for (const spz::SeedReport::View &v : rep.views) {
    py::dict x;
    x["valid"] = v.valid;
    x["appended"] = v.appended;
    x["refused"] = v.refused;
    views.append(x);
  }
  d["views"] = views;
  d["num_points"] = rep.numPoints;
  d["ms"] = py::make_tuple(rep.ms[0], rep.ms[1], rep.ms[2]);
  if (data) d["data"] = py::bytes(reinterpret_cast<const char *>(data->data()), data->size());
  return d;
}

// locate_spz's arguments as spz::LocateOptions.
spz::LocateOptions locateOptions(int iterations, int levels, spz::CoordinateSystem coord, const py::object &background,
                                 int max_sh_degree, float near_plane, double lambda_dssim, double lr_rotation,
                                 const py::object &lr_translation, double lr_final_factor, double beta1, double beta2,
                                 double eps) {
  spz::LocateOptions o;
  if (iterations < 0) throw py::value_error("iterations must be >= 0");
  if (levels < 1 || levels > SPZ_AMD_LOCATE_MAX_LEVELS) throw py::value_error("levels must be 1..8");
  o.iterations = iterations;
  o.levels = levels;
  frameInto(o, coord, near_plane, max_sh_degree, background, /*checked=*/true);
  optimiserInto(o, lambda_dssim, beta1, beta2, eps);
  o.rotationLr = finite(lr_rotation, Bound::NonNegative, "lr_rotation must be finite and >= 0");
  if (!lr_translation.is_none()) {
    o.translationLr = finite(py::cast<double>(lr_translation), Bound::NonNegative, "lr_translation must be finite and >= 0");
  }
  if (!(lr_final_factor > 0.0 && lr_final_factor <= 1.0)) throw py::value_error("lr_final_factor must be in (0, 1]");
  o.lrFinalFactor = lr_final_factor;
  return o;
}

// clean_spz's arguments as spz::CleanOptions.
spz::CleanOptions cleanOptions(const py::object &k, const py::object &std_ratio, const py::object &radius,
                               const py::object &min_neighbors) {
  if (k.is_none() && radius.is_none() && min_neighbors.is_none()) {
    throw py::value_error("give k, or radius and min_neighbors, or both");
  }
  if (radius.is_none() != min_neighbors.is_none()) throw py::value_error("radius and min_neighbors go together");
  spz::CleanOptions o;
  if (!k.is_none()) {
    const int kv = intIn(k, 1, 64, "k must be an int in 1..64");
    o.statistical = spz::CleanOptions::Statistical{kv, finiteReal(std_ratio, Bound::Any, "std_ratio must be a finite number")};
  }
  if (!radius.is_none()) {
    const double r = finiteReal(radius, Bound::Positive, "radius must be a finite number > 0");
    o.radius = spz::CleanOptions::Radius{r, intIn(min_neighbors, 1, 256, "min_neighbors must be an int in 1..256")};
  }
  return o;
}

// orbit_views' scene (a GaussianCloud, a .spz path or the file's bytes, decoded to `coord`) as its positions.
std::vector<float> scenePositions(const py::object &scene, spz::CoordinateSystem coord) {
  if (py::isinstance<spz::GaussianCloud>(scene)) return scene.cast<const spz::GaussianCloud &>().positions;
  spz::UnpackOptions u;
  u.to = coord;
  spz::GaussianCloud g = callOn(Input(scene), [&](auto... file) { return spz::loadSpz(file..., u); });
  if (g.numPoints <= 0) {
    raiseIfDeviceUnusable();
    throw py::value_error("orbit_views: the scene has no points, or does not load");
  }
  return std::move(g.positions);
}
}  // namespace
