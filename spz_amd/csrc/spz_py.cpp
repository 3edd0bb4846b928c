// spz_py.cpp — Python module `spz` (imported as spz_amd.spz) over the C++ drop-in layer: the module table.
//
// Same surface as the reference's nanobind shim: CoordinateSystem enum with exported values, PackOptions.from_coord,
// UnpackOptions.to_coord, GaussianCloud with copying float32 array properties and the shim's validation messages,
// load_spz / save_spz / load_splat_from_ply / save_splat_to_ply, then this implementation's own operations.  How
// arguments are read and results shaped is in spz_py_args.hpp.
#include <chrono>
#include <memory>
#include <sstream>

#include "spz_py_args.hpp"
#include "spz_deflate.hpp"
#include "spz_inflate.hpp"

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
          [](Cloud &c, const py::object &o) { setCloudArray(c, &Cloud::scales, o, "scales", 3); })
      .def_property(
          "rotations", [](const Cloud &c) { return toArray(c.rotations); },
          [](Cloud &c, const py::object &o) { setCloudArray(c, &Cloud::rotations, o, "rotations", 4); })
      .def_property(
          "alphas", [](const Cloud &c) { return toArray(c.alphas); },
          [](Cloud &c, const py::object &o) { setCloudArray(c, &Cloud::alphas, o, "alphas", 1); })
      .def_property(
          "colors", [](const Cloud &c) { return toArray(c.colors); },
          [](Cloud &c, const py::object &o) { setCloudArray(c, &Cloud::colors, o, "colors", 3); })
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
          if (!unlocked([&] { return spz::filterSpz(input, output, f, &kept); })) {
            raiseFileFailure("filter_spz", input, output);
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
          if (!unlocked([&] { return spz::transformSpz(input, output, o); })) {
            raiseFileFailure("transform_spz", input, output);
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
          if (!unlocked([&] { return spz::transformCloud(g, o); })) raiseFailure("transform_cloud");
        },
        py::arg("cloud"), py::kw_only(), py::arg("rotation") = py::none(), py::arg("translation") = py::none(),
        py::arg("scale") = 1.0, py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        "transform_spz's transform in place on a GaussianCloud (spz::transformCloud), in f32 without quantising.");
  m.def("merge_spz",
        [](const std::vector<std::string> &inputs, const std::string &output, const py::object &transforms,
           const py::object &sh_degree, const py::object &fractional_bits, const py::object &antialiased) {
          const spz::MergeOptions o = mergeOptions(inputs.size(), transforms, sh_degree, fractional_bits, antialiased);
          int64_t points = 0;
          if (!unlocked([&] { return spz::mergeSpz(inputs, output, o, &points); })) {
            raiseFailure("merge_spz", "for these files", "-> " + output);
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
          const spz::SortOptions o = sortOptions(keys, descending);
          std::vector<uint32_t> order;
          if (!unlocked([&] { return spz::sortSpz(input, output, o, &order); })) {
            raiseFileFailure("sort_spz", input, output, /*unsupportedRefused=*/true);
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
          const bool want_parents = flag(return_parents, "return_parents");
          const spz::DecimateOptions o = decimateOptions(level, target);
          std::vector<uint32_t> parents;
          int used = -1;
          int64_t points = 0;
          if (!unlocked([&] {
                return spz::decimateSpz(input, output, o, want_parents ? &parents : nullptr, &used, &points);
              })) {
            raiseFileFailure("decimate_spz", input, output, /*unsupportedRefused=*/true);
          }
          return decimateResult(used, points, want_parents ? &parents : nullptr);
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
          const spz::TileOptions o = tileOptions(max_points, max_tiles, coord);
          spz::Tileset t;
          if (!unlocked([&] { return spz::tileSpz(input, out_dir, o, &t); })) {
            raiseFailure("tile_spz", "", input + " -> " + out_dir, /*unsupportedRefused=*/true);
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
          View v;
          setPose(v, m.data(), fx, fy);
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
          const bool ok = callOn(Input(input), [&](auto... file) { return spz::renderSpz(file..., o, &img); });
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
          const bool ok = unlocked([&] { return spz::renderCloud(cloud, o, &img); });
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
          const bool ok = callOn(Input(input), [&](auto... file) { return spz::renderSpzDepth(file..., o, &maps); });
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
          const bool ok = unlocked([&] { return spz::renderCloudDepth(cloud, o, &maps); });
          return renderedDepth(ok, maps, o, "render_depth_cloud");
        },
        py::arg("cloud"), py::kw_only(), py::arg("world_to_camera"), py::arg("width"), py::arg("height"), py::arg("fx"),
        py::arg("fy"), py::arg("cx"), py::arg("cy"), py::arg("near") = 0.2f,
        py::arg("background") = py::make_tuple(0.0f, 0.0f, 0.0f), py::arg("max_sh_degree") = 3,
        "The depth maps of one pinhole view of a GaussianCloud in host memory (spz::renderCloudDepth): the dict of "
        "render_depth_spz, the cloud uploaded and taken as it is, in the frame of world_to_camera.");
  m.def("look_at",
        [](const std::array<float, 3> &eye, const std::array<float, 3> &target, const std::array<float, 3> &up) {
          try {
            const std::array<float, 12> r = spz::lookAt(eye, target, up);
            return toArray(std::vector<float>(r.begin(), r.end()), {3, 4});
          } catch (const std::invalid_argument &e) {
            throw py::value_error(e.what());
          }
        },
        py::arg("eye"), py::arg("target"), py::arg("up"),
        "The 3x4 world_to_camera (float32) of a camera at eye looking at target, OpenCV axes: up maps to -y.");
  m.def("prune_spz",
        [](const std::string &input, const std::string &output, const py::object &views, const py::object &keep,
           const py::object &keep_fraction, const py::object &min_score, const std::string &score,
           spz::CoordinateSystem coord, float near_plane, const py::object &return_scores) -> py::object {
          const bool details = flag(return_scores, "return_scores");
          const spz::PruneOptions o = pruneOptions(views, keep, keep_fraction, min_score, score, coord, near_plane);
          std::vector<uint8_t> mask;
          std::vector<uint64_t> sums;
          std::vector<float> maxima;
          int64_t kept = 0;
          if (!unlocked([&] {
                return spz::pruneSpz(input, output, o, &kept, details ? &mask : nullptr, details ? &sums : nullptr,
                                     details ? &maxima : nullptr);
              })) {
            raiseFileFailure("prune_spz", input, output);
          }
          return pruneResult(kept, details, mask, sums, maxima);
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
            if (!spz::boundingSphere(scenePositions(scene, coord), &c, &r)) {
              throw py::value_error("orbit_views: the scene has no finite positions");
            }
          }
          if (!center.is_none()) {
            const auto cc = center.cast<std::vector<float>>();
            if (cc.size() != 3) throw py::value_error("center must have three values");
            for (int k = 0; k < 3; ++k) c[k] = cc[k];
          }
          if (!radius.is_none()) r = radius.cast<float>();
          try {
            return viewDicts(spz::orbitViews(n, c, r, width, height, fov_y, distance));
          } catch (const std::invalid_argument &e) {
            throw py::value_error(e.what());
          }
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
          try {
            return viewDicts(spz::loadViewsFile(filename));
          } catch (const std::invalid_argument &e) {
            throw py::value_error(e.what());
          }
        },
        py::arg("filename"),
        "The views of a plain-text views file (spz_prune --views; spz::loadViewsFile) as prune_spz's view dicts: one "
        "view per line, 'width height fx fy cx cy r00 r01 r02 t0 r10 r11 r12 t1 r20 r21 r22 t2', '#' starts a comment.");
  m.def("align_spz",
        [](const py::object &source, const py::object &target, const py::object &rotation, const py::object &translation,
           double scale, spz::CoordinateSystem coord, bool estimate_scale, double overlap, const py::object &max_distance,
           const py::object &stride, const py::object &max_iterations, double relative_fitness, double relative_rmse,
           bool init_centroids) {
          const spz::AlignOptions o = alignOptions(rotation, translation, scale, coord, estimate_scale, overlap, max_distance,
                                                   stride, max_iterations, relative_fitness, relative_rmse, init_centroids);
          spz::AlignResult r;
          if (!callOn(Input(source), Input(target), "source", "target",
                      [&](auto... files) { return spz::alignSpz(files..., o, &r); })) {
            raiseFailure("align_spz", "", "", /*unsupportedRefused=*/true);
          }
          return alignDict(r);
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
  m.def("level_spz",
        [](const py::object &input, const py::object &output, const py::object &threshold, const py::object &hypotheses,
           const py::object &seed, const py::object &stride, const py::object &refine, const py::object &planes,
           const py::object &min_inliers, const py::object &axis, const py::object &max_tilt, const py::object &up_hint,
           spz::CoordinateSystem coord, bool no_translate, const py::object &select, const py::object &fractional_bits) {
          const spz::LevelOptions o = levelOptions(threshold, hypotheses, seed, stride, refine, planes, min_inliers, axis,
                                                   max_tilt, up_hint, coord, no_translate, select, fractional_bits);
          if (output.is_none() && !select.is_none()) throw py::value_error("select needs an output file");
          const Input in(input);
          spz::LevelResult r;
          bool ok;
          if (output.is_none()) {
            ok = callOn(in, [&](auto... file) { return spz::detectPlanes(file..., o, &r); });
          } else {
            if (in.bytes) throw py::value_error("with an output file the input must be a path");
            const std::string out = py::str(output).cast<std::string>();
            ok = unlocked([&] { return spz::levelSpz(in.path, out, o, &r); });
          }
          if (!ok) raiseFailure("level_spz", "", "", /*unsupportedRefused=*/true);
          return levelDict(r);
        },
        py::arg("input"), py::arg("output") = py::none(), py::kw_only(), py::arg("threshold"),
        py::arg("hypotheses") = 4096, py::arg("seed") = 0, py::arg("stride") = 1, py::arg("refine") = 3,
        py::arg("planes") = 1, py::arg("min_inliers") = 0, py::arg("axis") = py::none(),
        py::arg("max_tilt") = py::none(), py::arg("up_hint") = py::none(),
        py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED, py::arg("no_translate") = false,
        py::arg("select") = py::none(), py::arg("fractional_bits") = 12,
        "The dominant plane of a v2/v3 .spz (a path, or the file's bytes), or up to `planes` of them, by MSAC over seeded "
        "hypotheses on the stored integers with an exact least-squares refinement on the device (spz::detectPlanes / "
        "spz::levelSpz; the contract is in include/spz_amd.h \"plane\").  threshold is the inlier distance in world "
        "units; min_inliers an int count or a float fraction of the points taking part.  With output and no select the "
        "file is written levelled on the first plane (transform_spz); with select ('plane', 'off-plane', 'above', "
        "'below') that subset of the input is written without requantising.  Returns a dict: planes (a list of dicts: "
        "integers (a, b, c, e), normal, offset, inliers, points, fitness, mean_distance, rotation, translation, ...), "
        "rotation, translation and scale of the first plane's placement in `coord` (None without a plane; nothing is "
        "written then), threshold (T), labels (uint8 per point), kept, and ms (prepare, score, refine).");
  m.def("compare_spz",
        [](const py::object &a, const py::object &b, const py::object &views, spz::CoordinateSystem coord,
           const py::object &background, int max_sh_degree, float near_plane, const py::object &return_maps) {
          const bool maps = flag(return_maps, "return_maps");
          spz::CompareOptions o;
          frameInto(o, coord, near_plane, max_sh_degree, background, /*checked=*/true);
          o.views = viewList(views, SPZ_AMD_COMPARE_MAX_VIEWS, coord, near_plane);
          std::vector<spz::ImageMetrics> got;
          std::vector<std::vector<float>> ssim;
          if (!callOn(Input(a), Input(b), "a", "b",
                      [&](auto... files) { return spz::compareSpz(files..., o, &got, maps ? &ssim : nullptr); })) {
            raiseFailure("compare_spz");
          }
          return metricsDicts(got, maps ? &ssim : nullptr, &o.views);
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
          const spz::RefineOptions o = refineOptions(views, iterations, coord, background, max_sh_degree, near_plane,
                                                     lambda_dssim, lrs, beta1, beta2, eps, train, densify);
          const Input in(input), tg(target);
          if (in.bytes && tg.bytes && !output.is_none()) {
            throw py::value_error("with bytes in, output must be None: the bytes are returned");
          }
          if (!in.bytes && !tg.bytes && output.is_none()) throw py::value_error("with paths in, give the output path");
          const std::string out = output.is_none() ? std::string() : py::str(output).cast<std::string>();  // paths only
          spz::RefineReport rep;
          std::vector<uint8_t> data;
          // refineSpz's two overloads end differently, so the lambda tells them apart by what callOn hands it:
          // (data, size, data, size) for bytes, which are returned, or (path, path), which take the output path
          if (!callOn(in, tg, "input", "target", [&](auto... files) {
                if constexpr (sizeof...(files) == 4) {
                  return spz::refineSpz(files..., o, &data, &rep);
                } else {
                  return spz::refineSpz(files..., out, o, &rep);
                }
              })) {
            raiseFailure("refine_spz");
          }
          return refineDict(rep, in.bytes ? &data : nullptr);
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
  m.def("refine_spz_to_images",
        [](const py::object &input, const py::object &output, const py::object &views, const py::object &images,
           const py::object &weights, const py::object &fit_exposure, double lr_exposure, int iterations,
           spz::CoordinateSystem coord, const py::object &background, int max_sh_degree, float near_plane,
           double lambda_dssim, const py::object &lrs, double beta1, double beta2, double eps, const py::object &train,
           const py::object &densify, const py::object &depths, double depth_weight, const py::object &depth_kind,
           double depth_min_alpha) {
          const spz::RefineOptions o = refineOptions(views, iterations, coord, background, max_sh_degree, near_plane,
                                                     lambda_dssim, lrs, beta1, beta2, eps, train, densify);
          std::vector<FloatArray> keep;
          spz::PhotoOptions p = photoOptions(images, weights, fit_exposure, lr_exposure, o.views, &keep);
          depthOptionsInto(p, depths, depth_weight, depth_kind, depth_min_alpha, o.views, &keep);
          const Input in(input);
          if (in.bytes && !output.is_none()) {
            throw py::value_error("with bytes in, output must be None: the bytes are returned");
          }
          if (!in.bytes && output.is_none()) throw py::value_error("with a path in, give the output path");
          const std::string out = output.is_none() ? std::string() : py::str(output).cast<std::string>();
          spz::PhotoReport rep;
          std::vector<uint8_t> data;
          if (!callOn(in, [&](auto... file) {
                if constexpr (sizeof...(file) == 2) {
                  return spz::refineSpzToImages(file..., o, p, &data, &rep);
                } else {
                  return spz::refineSpzToImages(file..., out, o, p, &rep);
                }
              })) {
            raiseFailure("refine_spz_to_images");
          }
          py::dict d = refineDict(rep.refine, in.bytes ? &data : nullptr);
          py::array_t<double> ex(std::vector<py::ssize_t>{static_cast<py::ssize_t>(rep.exposures.size()), 3, 4});
          for (size_t v = 0; v < rep.exposures.size(); ++v) {
            std::copy(rep.exposures[v].begin(), rep.exposures[v].end(), ex.mutable_data() + 12 * v);
          }
          d["exposures"] = ex;
          if (!rep.depthError.empty()) {
            d["depth_history"] = rep.depthHistory;
            py::array_t<double> de(std::vector<py::ssize_t>{static_cast<py::ssize_t>(rep.depthError.size()), 2});
            for (size_t v = 0; v < rep.depthError.size(); ++v) {
              std::copy(rep.depthError[v].begin(), rep.depthError[v].end(), de.mutable_data() + 2 * v);
            }
            d["depth_error"] = de;
          }
          return d;
        },
        py::arg("input"), py::arg("output"), py::arg("views"), py::arg("images"), py::arg("weights") = py::none(),
        py::arg("fit_exposure") = false, py::arg("lr_exposure") = 0.01, py::kw_only(), py::arg("iterations") = 200,
        py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED, py::arg("background") = py::make_tuple(0.0f, 0.0f, 0.0f),
        py::arg("max_sh_degree") = 3, py::arg("near") = 0.2f, py::arg("lambda_dssim") = 0.2, py::arg("lrs") = py::none(),
        py::arg("beta1") = 0.9, py::arg("beta2") = 0.999, py::arg("eps") = 1e-15, py::arg("train") = py::none(),
        py::arg("densify") = py::none(), py::arg("depths") = py::none(), py::arg("depth_weight") = 1.0,
        py::arg("depth_kind") = "l1", py::arg("depth_min_alpha") = 0.5,
        "refine_spz against photographs (spz::refineSpzToImages; the contract is in include/spz_amd.h \"photo loss\" and "
        "\"refine images\"): fit the .spz file `input` (a path, or the file's bytes with output None) to `images`, one "
        "(height, width, 3 or 4) float32 array per view of `views`, of the view's size, values in [0, 1] (load_image).  "
        "weights: None, or one entry per view, each None or a (height, width) float32 array in [0, 1]: what each pixel "
        "counts in the loss.  fit_exposure: fit a 3 x 4 colour transform per image beside the cloud, at rate lr_exposure.  "
        "The other keywords are refine_spz's (the position rate defaults to 1.6e-4 times the input's bounding-sphere "
        "radius; densify needs max_points).  Returns refine_spz's dict and \"exposures\", a (views, 3, 4) float64 array "
        "[M | o], the identity without fit_exposure; \"after\" is of the written stream through the fitted exposure.  "
        "depths: None, or one entry per view, each None or a (height, width) float32 array of metric depth along the "
        "camera's z (load_depth; not finite or <= 0: no measurement): the loss gains depth_weight times the depth loss "
        "(include/spz_amd.h \"depth loss\"), depth_kind \"l1\" or \"inverse\", over the pixels of alpha >= "
        "depth_min_alpha; the dict then also has \"depth_history\" and \"depth_error\", a (views, 2) float64 array: "
        "the depth loss of the input and of the written stream against each map, -1 for a view without one.");
  m.def("seed_spz",
        [](const py::object &views, const py::object &images, const py::object &depths, const py::object &masks,
           const py::object &out, const py::object &base, const py::object &stride, double scale_factor, double opacity,
           const py::object &cover, double cover_alpha, double cover_tolerance, const py::object &sh_degree,
           const py::object &max_points, spz::CoordinateSystem coord, float near_plane) {
          const spz::SeedOptions o = seedOptions(views, base, stride, scale_factor, opacity, cover, cover_alpha,
                                                 cover_tolerance, sh_degree, max_points, coord, near_plane);
          std::vector<FloatArray> keep;
          spz::PhotoOptions p = photoOptions(images, masks, py::bool_(false), 0.0, o.views, &keep);
          if (depths.is_none()) throw py::value_error("depths must be a sequence of numpy arrays, one per view");
          depthOptionsInto(p, depths, 1.0, py::str("l1"), 0.5, o.views, &keep);
          const std::string path = out.is_none() ? std::string() : py::str(out).cast<std::string>();
          spz::SeedReport rep;
          std::vector<uint8_t> data;
          const bool toBytes = out.is_none();
          if (!unlocked([&] { return toBytes ? spz::seedSpz(o, p.images, &data, &rep) : spz::seedSpz(o, p.images, path, &rep); })) {
            raiseFailure("seed_spz");
          }
          return seedDict(rep, toBytes ? &data : nullptr);
        },
        py::arg("views"), py::arg("images"), py::arg("depths"), py::kw_only(), py::arg("masks") = py::none(),
        py::arg("out") = py::none(), py::arg("base") = py::none(), py::arg("stride") = 1, py::arg("scale_factor") = 1.0,
        py::arg("opacity") = 0.5, py::arg("cover") = true, py::arg("cover_alpha") = 0.5, py::arg("cover_tolerance") = 0.05,
        py::arg("sh_degree") = 0, py::arg("max_points") = 0, py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        py::arg("near_plane") = 0.2f,
        "A .spz file from posed photographs with depth maps (spz::seedSpz; the contract is in include/spz_amd.h \"seed\"): "
        "`images`, one (height, width, 3 or 4) float32 array per view of `views` (dicts as orbit_views returns them, in the "
        "frame `coord`), and `depths`, one (height, width) float32 array of metric depth along the camera's z per view "
        "(load_depth; not finite or not > near_plane: no measurement).  masks: None, or one entry per view, each None or a "
        "(height, width) float32 array: a sample counts above 0.5.  Every stride-th pixel with a measurement that the "
        "cloud built so far does not explain (rendered alpha under cover_alpha, or expected depth off by more than "
        "cover_tolerance times the measurement) becomes an isotropic Gaussian of the lattice's spacing at that depth "
        "times scale_factor, with the pixel's colour and `opacity`; cover False lifts every sample.  max_points 0: the "
        "sum of the views' sample counts.  base: a .spz file (a path or its bytes) of the same sh_degree to seed onto: "
        "it is used for the cover test only, the NEW points alone are written, and merge_spz joins the two.  Returns a "
        "dict: views (valid, appended and refused per view), num_points, ms (cover renders, seeds, encode) and, with out "
        "None, data, the file's bytes; with out a path the file is written there.");
  m.def("locate_spz",
        [](const py::object &input, const py::object &view, const py::object &image, int iterations, int levels,
           spz::CoordinateSystem coord, const py::object &background, int max_sh_degree, float near_plane,
           double lambda_dssim, double lr_rotation, const py::object &lr_translation, double lr_final_factor, double beta1,
           double beta2, double eps) {
          const spz::LocateOptions o = locateOptions(iterations, levels, coord, background, max_sh_degree, near_plane,
                                                     lambda_dssim, lr_rotation, lr_translation, lr_final_factor, beta1, beta2,
                                                     eps);
          const View v = pruneView(view, 0, coord, near_plane);
          const FloatArray pixels = imageArray(image, "image", &v);
          if (v.width % (1 << (levels - 1)) != 0 || v.height % (1 << (levels - 1)) != 0) {
            throw py::value_error("width and height must be divisible by 2^(levels - 1)");
          }
          const int channels = static_cast<int>(pixels.shape(2));
          spz::LocateReport rep;
          if (!callOn(Input(input), [&](auto... file) { return spz::locateSpz(file..., v, pixels.data(), channels, o, &rep); })) {
            raiseFailure("locate_spz");
          }
          return locateResult(rep);
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
          return toArray(pixels, {h, w, 3});
        },
        py::arg("path"),
        "A picture as spz_render writes it, as locate_spz takes it: a binary PPM (P6, maxval 255) or a colour PFM (PF, "
        "either byte order) as a (height, width, 3) float32 array, rows top to bottom.  ValueError when the file does "
        "not open or is neither.");
  m.def("load_depth",
        [](const std::string &path) {
          std::vector<float> pixels;
          int w = 0, h = 0;
          try {
            spz::loadDepthFile(path, &pixels, &w, &h);
          } catch (const std::invalid_argument &e) {
            throw py::value_error(e.what());
          }
          return toArray(pixels, {h, w});
        },
        py::arg("path"),
        "A depth map as spz_render --depth writes it, as refine_spz_to_images takes it: a one-channel PFM (Pf), or the "
        "first channel of a colour PFM (PF), either byte order, as a (height, width) float32 array, rows top to bottom, "
        "the floats' bits kept.  ValueError when the file does not open or is neither.");
  m.def("compare_images",
        [](const py::object &a, const py::object &b, const py::object &return_map) {
          const bool want = flag(return_map, "return_map");
          const FloatArray fa = imageArray(a, "a"), fb = imageArray(b, "b");
          if (fa.shape(0) != fb.shape(0) || fa.shape(1) != fb.shape(1)) {
            throw py::value_error("a and b must have the same height and width");
          }
          if (fa.shape(0) < 1 || fa.shape(0) > 16384 || fa.shape(1) < 1 || fa.shape(1) > 16384) {
            throw py::value_error("height and width must be in 1..16384");
          }
          const int h = static_cast<int>(fa.shape(0)), w = static_cast<int>(fa.shape(1));
          const int ca = static_cast<int>(fa.shape(2)), cb = static_cast<int>(fb.shape(2));
          spz::ImageMetrics m;
          std::vector<float> map;
          if (!unlocked([&] { return spz::compareImages(fa.data(), ca, fb.data(), cb, w, h, &m, want ? &map : nullptr); })) {
            raiseFailure("compare_images");
          }
          return metricsDict(m, want ? &map : nullptr, h, w);
        },
        py::arg("a"), py::arg("b"), py::kw_only(), py::arg("return_map") = false,
        "PSNR, MSE, L1, max error and SSIM of two (height, width, 3 or 4) float32 images on the device "
        "(spz::compareImages; include/spz_amd.h \"image metrics\"): values clamped to [0, 1] (NaN -> 0), the first three "
        "channels, an 11x11 Gaussian window of sigma 1.5 with zero padding.  Returns a dict: mse, psnr, ssim, l1, "
        "max_abs; with return_map also ssim_map, (height, width) float32.");
  m.def("mesh_spz",
        [](const py::object &input, const py::object &views, const py::object &box, const py::object &voxel_size,
           const py::object &resolution, const py::object &truncation, const std::string &depth,
           const py::object &min_alpha, const py::object &min_weight, float near_plane, spz::CoordinateSystem coord) {
          const spz::MeshOptions o = meshOptions(views, box, voxel_size, resolution, truncation, depth, min_alpha,
                                                 min_weight, near_plane, coord);
          spz::TriangleMesh mesh;
          if (!callOn(Input(input), [&](auto... file) { return spz::meshSpz(file..., o, &mesh); })) {
            raiseFailure("mesh_spz");
          }
          return meshResult(mesh);
        },
        py::arg("input"), py::arg("views"), py::kw_only(), py::arg("box") = py::none(),
        py::arg("voxel_size") = py::none(), py::arg("resolution") = py::none(), py::arg("truncation") = py::none(),
        py::arg("depth") = "median", py::arg("min_alpha") = 0.5, py::arg("min_weight") = 1.0, py::arg("near") = 0.2f,
        py::arg("coord") = spz::CoordinateSystem::UNSPECIFIED,
        "The triangle mesh of a .spz file (a path or the file's bytes) on the device (spz::meshSpz; the contract is in "
        "include/spz_amd.h \"mesh\"): the depth maps of `views` (1..1024 dicts as orbit_views returns them, in the frame "
        "`coord`) fused into a truncated signed distance volume, its zero level set by marching tetrahedra.  box (x0, y0, "
        "z0, x1, y1, z1): None = the bounding box of the file's positions (floaters inflate it: clean_spz first, or pass "
        "one).  voxel_size or resolution (cells along the longest side; neither: 256); truncation: None = 4 voxels; "
        "depth 'median' or 'expected' (then pixels under min_alpha are not fused); min_weight: the views that must have "
        "seen every corner of a cube.  Returns a dict: vertices (n, 3) float32, colors (n, 3) float32 (not clamped), "
        "triangles (m, 3) uint32, volume (lo, voxel_size, dims, truncation) and ms (renders, fuses, extraction).");
  m.def("save_mesh_ply",
        [](const std::string &path, const py::object &vertices, const py::object &colors, const py::object &triangles) {
          const FloatArray v = meshFloats(vertices, "vertices"), c = meshFloats(colors, "colors");
          if (c.shape(0) != v.shape(0)) throw py::value_error("colors must have one row per vertex");
          const IndexArray t = meshIndices(triangles);
          if (!unlocked([&] {
                return spz::saveMeshPly(path, v.data(), c.data(), static_cast<size_t>(v.shape(0)), t.data(),
                                        static_cast<size_t>(t.shape(0)));
              })) {
            raiseFailure("save_mesh_ply", "", path);
          }
        },
        py::arg("path"), py::arg("vertices"), py::arg("colors"), py::arg("triangles"),
        "Write a triangle mesh as a binary little-endian PLY (spz::saveMeshPly): x y z float, red green blue uchar "
        "(rint(255 clamp(c, 0, 1))), faces as list uchar uint vertex_indices.  ValueError when an index is not below "
        "the vertex count.");
  m.def("clean_spz",
        [](const std::string &input, const std::string &output, const py::object &k, const py::object &std_ratio,
           const py::object &radius, const py::object &min_neighbors, const py::object &return_details) -> py::object {
          const bool details = flag(return_details, "return_details");
          const spz::CleanOptions o = cleanOptions(k, std_ratio, radius, min_neighbors);
          std::vector<uint8_t> mask;
          std::vector<double> scores;
          int64_t kept = 0;
          double thr = 0.0;
          if (!unlocked([&] {
                return spz::cleanSpz(input, output, o, &kept, details ? &mask : nullptr, details ? &scores : nullptr, &thr);
              })) {
            raiseFileFailure("clean_spz", input, output, /*unsupportedRefused=*/true);
          }
          return cleanResult(kept, details, mask, o.statistical.has_value(), scores, thr);
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
