// spz_amd_host.hpp — C++ drop-in layer over the C ABI (include/spz_amd.h).
//
// Keeps the public C++ surface of lanxinger/spz for the save/load path so that
// code written against the reference compiles against this header unchanged:
//   namespace spz, GaussianCloud / PackedGaussians / PackOptions / UnpackOptions /
//   CoordinateSystem (reference: src/cc/splat-types.h:24-34,90-186, src/cc/load-spz.h:42-67),
//   saveSpz / loadSpz / loadSpzPacked / serializePackedGaussians / compressGzipped
//   (reference: src/cc/load-spz.h:69-100) with the same argument meaning, ownership
//   (everything by value / caller-owned vectors) and error behaviour (never throws; save ->
//   false, load -> default-constructed cloud plus one "[SPZ ERROR] ..." line on stdout).
//
// The per-Gaussian quantise / dequantise work runs on the GPU through libspz_amd.so.  The gzip container
// (load-spz.cc:141-214) keeps zlib's bytes and zlib's verdicts, but where it runs depends on the size: streams of
// 2 MiB and more are deflated, and members from about 30 MB (on 16 cores) inflated, ON THE DEVICE by default (spz_lz77.hip / spz_inflate_dev.hip: zlib
// 1.2.11's level-6 output reproduced bit for bit, every member's symbols checked against the input on the device;
// SPZ_AMD_GZIP_DEVICE / SPZ_AMD_GUNZIP_DEVICE = 0 keep the stage on the host), smaller ones and every case the device
// declines on the host (multi-threaded exact writer / parallel reader from 1 / 4 MiB, zlib itself below and as the last
// resort).  BASELINE.json's north_star kept gzip on the host; SURVEY §8(f)-2 is the row this widening belongs to.
// There is no CPU fallback for the quantise step: without a usable HIP device saveSpz returns
// false and loadSpz returns an empty cloud, each after logging
// "[SPZ ERROR] spz_amd: <status>".  The device used is $SPZ_AMD_DEVICE (default 0).
// Between calls the library keeps device memory (the host path's workspace, up to 32 GiB of container-stage scratch:
// SPZ_AMD_SCRATCH_KEEP_MIB) and one host buffer (<= 1 GiB); spz_amd_release_device_memory() and
// spz::releaseHostMemory() return them.  INTEGRATION.md "Memory the library keeps" has the figures.
#pragma once

#include <array>
#include <cstdint>
#include <iosfwd>
#include <limits>
#include <optional>
#include <string>
#include <vector>

#include "spz_amd_c_types.h"

namespace spz {

// splat-types.h:24-34
enum class CoordinateSystem {
  UNSPECIFIED = 0,
  LDB = 1,
  RDB = 2,
  LUB = 3,
  RUB = 4,
  LDF = 5,
  RDF = 6,
  LUF = 7,
  RUF = 8,
};

// splat-types.h:36-41: the three sign tables of a conversion.
struct CoordinateConverter {
  std::array<float, 3> flipP = {1.0f, 1.0f, 1.0f};
  std::array<float, 3> flipQ = {1.0f, 1.0f, 1.0f};
  std::array<float, 15> flipSh = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f,
                                  1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
};

// splat-types.h:43-81
CoordinateConverter coordinateConverter(CoordinateSystem from, CoordinateSystem to);

// splat-types.h:90-186.  Same field names and layout semantics as the reference struct.
struct GaussianCloud {
  int32_t numPoints = 0;
  int32_t shDegree = 0;
  bool antialiased = false;
  std::vector<float> positions;  // xyz
  std::vector<float> scales;     // log scale xyz
  std::vector<float> rotations;  // xyzw
  std::vector<float> alphas;     // pre-sigmoid
  std::vector<float> colors;     // SH DC rgb
  std::vector<float> sh;         // [point][coeff][rgb]

  // In-place flip between coordinate systems (splat-types.h:134-164); runs the GPU flip pass.
  void convertCoordinates(CoordinateSystem from, CoordinateSystem to);
  void rotate180DegAboutX() { convertCoordinates(CoordinateSystem::RUB, CoordinateSystem::RDF); }
  // splat-types.h:170-185 (host utility, not on the hot path).
  float medianVolume() const;
  // splat-types.h:117-130: copies of the six arrays in new float[] buffers the CALLER frees.
  GaussianCloudData data() const;
};

// load-spz.h:11-22: one inflated Gaussian (236 bytes).
struct UnpackedGaussian {
  std::array<float, 3> position;  // x, y, z
  std::array<float, 4> rotation;  // x, y, z, w
  std::array<float, 3> scale;     // log scale
  std::array<float, 3> color;     // rgb sh0 encoding
  float alpha;                    // inverse logistic
  std::array<float, 15> shR;
  std::array<float, 15> shG;
  std::array<float, 15> shB;
};

// load-spz.h:24-38: one packed Gaussian, always 65 bytes (missing sh coefficients are 128 = 0.0).
struct PackedGaussian {
  std::array<uint8_t, 9> position{};
  std::array<uint8_t, 4> rotation{};
  std::array<uint8_t, 3> scale{};
  std::array<uint8_t, 3> color{};
  uint8_t alpha = 0;
  std::array<uint8_t, 15> shR{};
  std::array<uint8_t, 15> shG{};
  std::array<uint8_t, 15> shB{};

  // load-spz.cc:383-431.  Runs the decode kernel on this one point (a 1-point stream through
  // spz_amd_decode_host): bit-identical to the reference, but a device round trip per call — use
  // unpackIndices / spz_amd_decode_gather_* for more than a handful of points.  `c` must be a table
  // that coordinateConverter() can produce (every from/to pair is; hand-edited tables are rejected
  // with a log line and a zeroed result).
  UnpackedGaussian unpack(bool usesFloat16, bool usesQuaternionSmallestThree, int32_t fractionalBits,
                          const CoordinateConverter &c) const;
};

// load-spz.h:42-59.
struct PackedGaussians {
  int32_t numPoints = 0;
  int32_t shDegree = 0;
  int32_t fractionalBits = 0;
  bool antialiased = false;
  bool usesQuaternionSmallestThree = true;
  std::vector<uint8_t> positions;
  std::vector<uint8_t> scales;
  std::vector<uint8_t> rotations;
  std::vector<uint8_t> alphas;
  std::vector<uint8_t> colors;
  std::vector<uint8_t> sh;

  bool usesFloat16() const;  // load-spz.cc:465
  PackedGaussian at(int32_t i) const;                                         // load-spz.cc:433-459 (bytes only)
  UnpackedGaussian unpack(int32_t i, const CoordinateConverter &c) const;     // load-spz.cc:461-463
};

// load-spz.h:61-67
struct PackOptions {
  CoordinateSystem from = CoordinateSystem::UNSPECIFIED;
};
struct UnpackOptions {
  CoordinateSystem to = CoordinateSystem::UNSPECIFIED;
};

// load-spz.h:69-100 -------------------------------------------------------------------------
bool saveSpz(const GaussianCloud &gaussians, const PackOptions &options, std::vector<uint8_t> *output);
bool saveSpz(const GaussianCloud &gaussians, const PackOptions &options, const std::string &filename);
GaussianCloud loadSpz(const std::vector<uint8_t> &data, const UnpackOptions &options);
GaussianCloud loadSpz(const uint8_t *data, int32_t size, const UnpackOptions &options);
GaussianCloud loadSpz(const std::string &filename, const UnpackOptions &options);
PackedGaussians loadSpzPacked(const std::string &filename);
PackedGaussians loadSpzPacked(const uint8_t *data, int32_t size);
PackedGaussians loadSpzPacked(const std::vector<uint8_t> &data);
// .ply pair (load-spz.cc:691-934): binary little-endian 3DGS layout, RDF on disk.
bool saveSplatToPly(const GaussianCloud &gaussians, const PackOptions &options, const std::string &filename);
GaussianCloud loadSplatFromPly(const std::string &filename, const UnpackOptions &options);
void serializePackedGaussians(const PackedGaussians &packed, std::ostream *out);
// load-spz.cc:186-214.  The bytes are zlib's (level 6, one deflate stream, gzip wrapper), whoever writes them:
//   >= 2 MiB and a device answers   the device writer (spz_lz77.hip; SPZ_AMD_GZIP_DEVICE=0 never, =1 from 1 MiB).  Every
//                                   symbol it codes is checked against the input on the device before the member is
//                                   handed out (always on); a member that fails is discarded, logged and counted
//                                   (deviceGzipRejectCount) and the next writer down produces it.
//   >= 1 MiB                        the multi-threaded host writer that reproduces zlib 1.2.11's output exactly
//                                   (SPZ_AMD_GZIP_EXACT_THREADS, default min(usable CPUs, 32); 1 = zlib itself)
//   otherwise, or when the machine has less free memory than 4.5 x the input, or for another zlib version: zlib.
// SPZ_AMD_GZIP_VERIFY=1 additionally inflates the finished member (device route: on the device, where the body still
// lies) and compares it with the input byte for byte before returning it; =2 also compares it with zlib's own member.
bool compressGzipped(const uint8_t *data, size_t size, std::vector<uint8_t> *out);

// ---- device-resident packed load (second half) ----------------------------------------------------
// loadSpzPacked (load-spz.cc:609-632) hands a renderer the packed sections in HOST vectors.  A renderer on the GPU wants
// them where it draws: loadSpzPackedDevice inflates the file (on the device when the device reader takes the member,
// otherwise on the host followed by one upload), applies deserializePackedGaussians' header checks with the reference's
// log lines (load-spz.cc:553-568,591-594) and leaves the stream IN DEVICE MEMORY.  The object owns that memory
// (move-only; release() or the destructor returns it) and exposes the six section pointers of
// deserializePackedGaussians' slicing (:569-590), the whole stream and its header — exactly the arguments of
// spz_amd_decode_device / spz_amd_decode_gather_device (spz_amd.h), so a caller decodes what it needs, when it needs it,
// without the bytes ever crossing PCIe again.  An empty object (numPoints == 0, null pointers) is the failure result,
// as the empty PackedGaussians is for loadSpzPacked.
class DevicePackedGaussians {
 public:
  DevicePackedGaussians() = default;
  DevicePackedGaussians(DevicePackedGaussians &&o) noexcept;
  DevicePackedGaussians &operator=(DevicePackedGaussians &&o) noexcept;
  DevicePackedGaussians(const DevicePackedGaussians &) = delete;
  DevicePackedGaussians &operator=(const DevicePackedGaussians &) = delete;
  ~DevicePackedGaussians();

  int32_t numPoints = 0;
  int32_t shDegree = 0;
  int32_t fractionalBits = 0;
  bool antialiased = false;
  bool usesQuaternionSmallestThree = true;
  uint32_t version = 0;                 // of the stream: 1, 2 or 3
  bool usesFloat16() const { return version == 1; }
  // device pointers into `stream` (null when the section is empty), section sizes as in PackedGaussians
  const uint8_t *positions = nullptr, *alphas = nullptr, *colors = nullptr, *scales = nullptr, *rotations = nullptr, *sh = nullptr;
  size_t positionsBytes = 0, alphasBytes = 0, colorsBytes = 0, scalesBytes = 0, rotationsBytes = 0, shBytes = 0;
  const uint8_t *stream = nullptr;      // header + sections, device memory
  size_t streamBytes = 0;
  int device = 0;
  bool inflatedOnDevice = false;        // which reader produced the stream (the bytes are the same)

  bool valid() const { return stream != nullptr; }
  void release();                       // returns the device memory; the object becomes the empty one
  // unpackGaussians (load-spz.cc:467-531) of all points / of an index list, from where the stream lies: only the
  // floats cross PCIe.  Same results as loadSpz / unpackIndices on the same file.
  GaussianCloud unpack(const UnpackOptions &o) const;
  GaussianCloud unpackIndices(const std::vector<uint32_t> &indices, const UnpackOptions &o) const;

 private:
  void *owner_ = nullptr;               // the C ABI's inflate context (spz_amd_inflate_close)
  friend DevicePackedGaussians loadSpzPackedDevice(const uint8_t *data, int32_t size);
};
DevicePackedGaussians loadSpzPackedDevice(const std::string &filename);
DevicePackedGaussians loadSpzPackedDevice(const uint8_t *data, int32_t size);
DevicePackedGaussians loadSpzPackedDevice(const std::vector<uint8_t> &data);

// External-linkage internals of the reference (load-spz.cc:257,467,548), kept because
// downstream code forward-declares them to skip gzip.
PackedGaussians packGaussians(const GaussianCloud &g, const PackOptions &o);
GaussianCloud unpackGaussians(const PackedGaussians &packed, const UnpackOptions &o);
PackedGaussians deserializePackedGaussians(std::istream &in);

// Extras of this implementation -------------------------------------------------------------
// Inverse of compressGzipped (the reference keeps it file-local, load-spz.cc:141-182).  Ordinary members of
// 4 MiB and more are inflated in parallel and verified by CRC-32 (from 8 threads up).  Members written
// by compressGzippedParallel are inflated piece-parallel (SPZ_AMD_GUNZIP_THREADS, default min(cores, 32));
// other members go through libdeflate when the system has libdeflate.so.0 (SPZ_AMD_NO_LIBDEFLATE=1 turns
// that off); zlib's streaming inflate, what the reference uses, is the fallback and decides every case
// the fast readers decline, so acceptance and output are zlib's.
bool decompressGzipped(const uint8_t *compressed, size_t size, std::vector<uint8_t> *out);
// Opt-in multi-threaded gzip (pigz's independent-blocks construction: 1 MiB raw-deflate pieces in one
// gzip member, their sizes listed in an FEXTRA subfield "SZ" that other readers skip).  Readable by
// every gzip reader including the reference's loadSpz, NOT byte-identical to compressGzipped.  saveSpz uses it when the environment sets SPZ_AMD_GZIP_THREADS > 1.
bool compressGzippedParallel(const uint8_t *data, size_t size, std::vector<uint8_t> *out, int threads);
// Bulk random access: the points `indices` of a packed cloud, decoded by one gather
// launch into a GaussianCloud of indices.size() points (same arithmetic as unpackGaussians).  An index
// past the end is an error: empty cloud + log line, lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG (the
// device-pointer form spz_amd_decode_gather_device clamps instead, as its header says).  Empty cloud on failure.
GaussianCloud unpackIndices(const PackedGaussians &packed, const std::vector<uint32_t> &indices,
                            const UnpackOptions &o);
// Raw (pre-gzip) stream <-> cloud, i.e. saveSpz / loadSpz without the zlib step.
bool packToStream(const GaussianCloud &g, const PackOptions &o, std::vector<uint8_t> *stream);
GaussianCloud unpackFromStream(const uint8_t *stream, size_t size, const UnpackOptions &o);
// CPUs this process may use (online count, affinity mask, cgroup quota): what the thread-count defaults of the
// gzip writer / readers derive from.
unsigned effectiveCpuCount();
// Members compressGzipped has written in this process with their LZ77 parse done on the device (spz_lz77.hip;
// environment SPZ_AMD_GZIP_DEVICE = 0 never, 1 always, unset: inputs of 2 MiB and more).  The bytes are zlib's
// whichever way the parse ran; this says which way it was.
uint64_t deviceGzipParseCount();
// Members of the device writer that failed one of its checks (symbols that do not reproduce the input; with
// SPZ_AMD_GZIP_VERIFY=1 a member that does not inflate back to it) and were discarded: the caller got the host writer's
// bytes instead, and a "[SPZ ERROR] spz_amd: the device gzip writer ..." line.  Anything but 0 is a defect to report.
uint64_t deviceGzipRejectCount();
// Members decompressGzipped has inflated on the device in this process (spz_inflate_dev.hip; SPZ_AMD_GUNZIP_DEVICE = 0
// never, 1 from 1 MiB, unset: by size and usable CPUs, from about 30 MB on 16 cores); believed only after the CRC-32 and ISIZE of the trailer matched.
uint64_t deviceInflateCount();
// Why the device reader stood down the last time this thread asked it ("" = it did not, or was not asked): the names
// spz_amd_inflate_last_decline() documents, or "crc" when it inflated something the trailer does not confirm.
const char *deviceInflateLastDecline();
// saveSpz keeps its transient stream buffer (65 bytes per Gaussian, at most 1 GiB) for the next save, because returning
// memory that device copies have pinned costs ~80 ms per GB; this drops it.  (The device side: spz_amd_release_device_memory().)
void releaseHostMemory();
// Filter (DESIGN §8 "filter"): a smaller .spz out of an existing one without requantising.  The member is inflated
// (loadSpzPackedDevice, on the device where the device reader takes it), the points are chosen and the K-point stream is
// cut out of the packed sections in HBM (spz_amd_filter_open: spz_amd_select_device + spz_amd_subset_device), and the
// stream goes through compressGzipped — with zlib's level-6 bytes, as saveSpz's.  Output point k is input point idx[k]
// with all its bytes (so the kept points decode to the same floats, bit for bit); its sh bytes are the first 3*dim(d') of
// its record.  The header keeps the input's version, fractionalBits and antialiased bit (reserved 0).
// Choosing idx: EITHER `indices` (any order, duplicates allowed, each < numPoints, at most 10 M) OR the selection — the
// points for which every given predicate holds, in input order: mask[i] != 0 (numPoints bytes); box lo <= p <= hi on
// every axis (inclusive; p the position loadSpz(…, UnpackOptions{coord}) returns, NaN never inside); decoded alpha (the
// logit loadSpz returns) >= minAlpha.  No predicate: every point.  shDegree -1 keeps the input's degree, 0 … the
// input's lowers it.  Keeping every point at the same degree gives back the input's stream byte for byte.
// false + one "[SPZ ERROR] filterSpz: …" line on a bad argument (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG), an input
// that does not load, or a device failure.  *kept: K.  SPZ_AMD_FILTER_TIMING=1 prints the stages' times to stderr.
struct FilterOptions {
  struct Box {
    std::array<float, 3> lo{}, hi{};
  };
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;  // of the positions the box is tested on
  std::optional<Box> box;
  std::optional<float> minAlpha;
  std::optional<std::vector<uint8_t>> mask;
  std::optional<std::vector<uint32_t>> indices;
  int32_t shDegree = -1;
};
bool filterSpz(const uint8_t *data, int32_t size, const FilterOptions &options, std::vector<uint8_t> *out,
               int64_t *kept = nullptr);
bool filterSpz(const std::string &inputFilename, const std::string &outputFilename, const FilterOptions &options,
               int64_t *kept = nullptr);
// Transform (DESIGN "Transform"): place a scene, p -> scale * R(rotation) * p + translation, stated in `coord`, with the
// rotation applied to every quaternion and to the sh bands (3DGS real-SH basis) and log(scale) added to every log-scale.
// rotation (x, y, z, w) need not be unit length (zero or non-finite is a bad argument); scale finite and > 0.  The
// parameter block and the per-point arithmetic are spz_amd_transform_params' (include/spz_amd.h).
// transformSpz: the member is inflated (loadSpzPackedDevice), the stream transformed in HBM in one pass
// (spz_amd_transform_open; any version 1/2/3 input, a v3 output with positions at fractionalBits, 0 ... 24; saveSpz writes
// 12), and compressed with zlib's level-6 bytes.  A point whose new position does not fit the 24-bit field at
// fractionalBits is refused (saveSpz would wrap it): the count is named, and no output is written.
// transformCloud: in place on the cloud's arrays (upload, kernel, download).
// false + one "[SPZ ERROR] transformSpz: …" (transformCloud: …) line on a bad argument (lastDeviceStatus() =
// SPZ_AMD_ERR_INVALID_ARG), an input that does not load, points out of range, or a device failure.
// SPZ_AMD_TRANSFORM_TIMING=1 prints the stages' times to stderr.
struct TransformOptions {
  std::array<double, 4> rotation = {0.0, 0.0, 0.0, 1.0};
  std::array<double, 3> translation = {0.0, 0.0, 0.0};
  double scale = 1.0;
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;  // of rotation and translation
  int32_t fractionalBits = 12;                             // of the output positions (transformSpz)
};
bool transformSpz(const uint8_t *data, int32_t size, const TransformOptions &options, std::vector<uint8_t> *out);
bool transformSpz(const std::string &inputFilename, const std::string &outputFilename, const TransformOptions &options);
bool transformCloud(GaussianCloud &gaussians, const TransformOptions &options);
// Merge (DESIGN "Merge"): one v3 .spz out of K >= 1 (at most SPZ_AMD_MERGE_MAX_INPUTS) inputs of any version, input
// 0's points first.  Bytes are copied wherever the encoding and the placement allow (so v3 inputs at the output's
// fractionalBits and degree with no placement merge losslessly, and a lone such file comes back byte for byte);
// positions, rotations, scales and sh are re-encoded with the transform's arithmetic only where they must be
// (spz_amd_merge_resolve / spz_amd_merge_device in include/spz_amd.h).  Every input is inflated on the device
// (loadSpzPackedDevice), one kernel writes the output, the inputs' device memory is released, and the stream is
// compressed with zlib's level-6 bytes.  A position that does not fit 24 bits at fractionalBits is refused (the count is
// named, no output is written).  false + one "[SPZ ERROR] mergeSpz: …" line on a bad argument or a conflict
// (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG), an input that does not load, or a device failure.
struct MergeOptions {
  int32_t shDegree = -1;         // -1: the largest input degree; 0 ... 3
  int32_t fractionalBits = -1;   // -1: the value all v2/v3 inputs share, else 12; 0 ... 24
  int32_t antialiased = -1;      // -1: the inputs must agree; 0 / 1 overrides
  // empty, or one entry per input: its placement (nullopt: none).  The entries' fractionalBits field is ignored: the
  // output's is the merge's.
  std::vector<std::optional<TransformOptions>> transforms;
};
bool mergeSpz(const std::vector<std::vector<uint8_t>> &inputs, const MergeOptions &options, std::vector<uint8_t> *out,
              int64_t *points = nullptr);
bool mergeSpz(const std::vector<std::string> &inputFilenames, const std::string &outputFilename,
              const MergeOptions &options, int64_t *points = nullptr);
// Sort (DESIGN §8 "sort"): the same points in a new order, without requantising.  The member is inflated
// (loadSpzPackedDevice), the order is computed on the device (spz_amd_sort_open: spz_amd_morton_order_device or
// spz_amd_argsort_f32_device, then spz_amd_subset_device) and the stream is compressed with zlib's level-6 bytes.
// Output point k is input point order[k] with all its bytes, at the input's degree; the header keeps the input's
// version, fractionalBits and antialiased bit.  Order: `keys` (one float per point) ascending, or descending, as numpy's
// argsort(k, kind="stable") (argsort(-k)): -0 == +0, every NaN last in both directions; no keys: the 72-bit Morton key of
// the stored 24-bit positions (include/spz_amd.h), not available for version 1 files (SPZ_AMD_ERR_UNSUPPORTED;
// transformSpz with the identity writes a v3 copy).  Ties keep input order, so sorting a sorted file gives the same bytes.
// *order (may be NULL): order[k].  false + one "[SPZ ERROR] sortSpz: …" line on a bad argument (a key count that is not
// numPoints: lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG), an input that does not load, or a device failure.
// SPZ_AMD_SORT_TIMING=1 prints the stages' times to stderr.
struct SortOptions {
  std::optional<std::vector<float>> keys;
  bool descending = false;
};
bool sortSpz(const uint8_t *data, int32_t size, const SortOptions &options, std::vector<uint8_t> *out,
             std::vector<uint32_t> *order = nullptr);
bool sortSpz(const std::string &inputFilename, const std::string &outputFilename, const SortOptions &options,
             std::vector<uint32_t> *order = nullptr);
// Decimate (DESIGN §8 "Decimate"): one point per occupied octree cell of edge 2^L quanta, in Morton order of the cells
// (include/spz_amd.h states the contract).  The member is inflated (loadSpzPackedDevice), decimated on the device
// (spz_amd_decimate_open) and the v3 stream is compressed with zlib's level-6 bytes.  Exactly one of `level` (0..24) and
// `targetPoints` (>= 1: the smallest level with at most that many cells) is set.  A cell of one point keeps its bytes
// (a v2 rotation is re-encoded); a cell of several is one Gaussian matching their moments.  Version 1 files are refused
// (SPZ_AMD_ERR_UNSUPPORTED).  *parents (may be NULL): the output index of every input point's cell; *level (may be NULL):
// the level used; *points (may be NULL): the output's point count.  false + one "[SPZ ERROR] decimateSpz: …" line on a bad argument (lastDeviceStatus() =
// SPZ_AMD_ERR_INVALID_ARG), an input that does not load, or a device failure.  SPZ_AMD_DECIMATE_TIMING=1 prints the
// stages' times to stderr.
struct DecimateOptions {
  std::optional<int> level;
  std::optional<uint64_t> targetPoints;
};
bool decimateSpz(const uint8_t *data, int32_t size, const DecimateOptions &options, std::vector<uint8_t> *out,
                 std::vector<uint32_t> *parents = nullptr, int *level = nullptr, int64_t *points = nullptr);
bool decimateSpz(const std::string &inputFilename, const std::string &outputFilename, const DecimateOptions &options,
                 std::vector<uint32_t> *parents = nullptr, int *level = nullptr, int64_t *points = nullptr);
// Clean (DESIGN §8 "Clean"): floater removal by the statistical (k nearest neighbours) and / or the radius outlier rule
// (include/spz_amd.h states the contract).  The member is inflated (loadSpzPackedDevice), cleaned on the device
// (spz_amd_clean_open) and the kept points' bytes are compressed with zlib's level-6 bytes: the stream equals filterSpz's
// with the keep mask.  At least one rule is set: statistical (k 1..64, stdRatio finite), radius (radius finite > 0,
// minNeighbors 1..256).  Version 1 files are refused (SPZ_AMD_ERR_UNSUPPORTED).  *kept (may be NULL): the kept count;
// *keepMask (may be NULL): one byte per input point, 1 = kept; *scores (may be NULL): the statistical scores (empty
// without that rule); *threshold (may be NULL): the threshold (NaN without that rule).  false + one
// "[SPZ ERROR] cleanSpz: …" line on a bad argument (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG), an input that does
// not load, or a device failure.  SPZ_AMD_CLEAN_TIMING=1 prints the stages' times to stderr.
struct CleanOptions {
  struct Statistical {
    int k = 20;
    double stdRatio = 2.0;
  };
  struct Radius {
    double radius = 0.0;
    int minNeighbors = 0;
  };
  std::optional<Statistical> statistical;
  std::optional<Radius> radius;
};
bool cleanSpz(const uint8_t *data, int32_t size, const CleanOptions &options, std::vector<uint8_t> *out,
              int64_t *kept = nullptr, std::vector<uint8_t> *keepMask = nullptr, std::vector<double> *scores = nullptr,
              double *threshold = nullptr);
bool cleanSpz(const std::string &inputFilename, const std::string &outputFilename, const CleanOptions &options,
              int64_t *kept = nullptr, std::vector<uint8_t> *keepMask = nullptr, std::vector<double> *scores = nullptr,
              double *threshold = nullptr);
// Align (DESIGN §8 "Align"): the similarity that places a source .spz on a target .spz, by a point-to-point, trimmed ICP
// with an optional scale on the stored integers of both files (include/spz_amd.h "align" states the contract).  Both
// members are inflated (loadSpzPackedDevice) and the run happens on the device (spz_amd_align_host).  rotation,
// translation and scale are the initial placement, stated in `coord`; the result's are stated in `coord` too, ready for
// TransformOptions or a merge placement.  Version 1 files are refused (SPZ_AMD_ERR_UNSUPPORTED), and so is a target
// without points.  A run that ends degenerate (fewer than three inliers, or source points on one line) returns true with
// degenerate set and converged false.  false + one "[SPZ ERROR] alignSpz: …" line on a bad argument (lastDeviceStatus()
// = SPZ_AMD_ERR_INVALID_ARG), an input that does not load, or a device failure.  SPZ_AMD_ALIGN_TIMING=1 prints the
// stages' times to stderr.
struct AlignOptions {
  std::array<double, 4> rotation = {0.0, 0.0, 0.0, 1.0};
  std::array<double, 3> translation = {0.0, 0.0, 0.0};
  double scale = 1.0;
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;
  bool estimateScale = false;
  double overlap = 1.0;                 // (0, 1]: the fraction of the candidates kept, nearest first
  std::optional<double> maxDistance;    // world units
  uint32_t stride = 1;                  // source points i with i % stride == 0 take part
  uint32_t maxIterations = 30;          // 1 ... 1000
  double relativeFitness = 1e-6, relativeRmse = 1e-6;
  bool initCentroids = false;
};
struct AlignResult {
  std::array<double, 4> rotation = {0.0, 0.0, 0.0, 1.0};
  std::array<double, 3> translation = {0.0, 0.0, 0.0};
  double scale = 1.0;
  double fitness = 0.0, inlierRmse = 0.0;
  uint64_t inliers = 0;
  uint32_t iterations = 0;
  bool converged = false, degenerate = false;
  struct Step {
    double fitness, inlierRmse;
    uint64_t inliers;
  };
  std::vector<Step> history;
};
bool alignSpz(const uint8_t *source, int32_t sourceSize, const uint8_t *target, int32_t targetSize,
              const AlignOptions &options, AlignResult *result);
bool alignSpz(const std::string &sourceFilename, const std::string &targetFilename, const AlignOptions &options,
              AlignResult *result);
// Level (DESIGN §8 "Level"): the dominant plane of a .spz, or up to `planes` of them, by MSAC over seeded hypotheses on
// the stored integers with an exact least-squares refinement (include/spz_amd.h "plane" states the contract), and the
// placement that levels the scene on the first plane.  detectPlanes: the member is inflated (loadSpzPackedDevice, or
// the caller's packed device stream) and the run happens on the device (spz_amd_plane_host); it returns true with no
// plane when none reaches minInliers.  levelSpz: detectPlanes, then with select == None the file placed by the first
// plane's rotation and translation (transformSpz at fractionalBits), otherwise the chosen subset of the input without
// requantising (filterSpz with a mask): Plane is |d| <= T of the first plane over every point, OffPlane the rest, Above
// d > T, Below d < -T.  No plane found: levelSpz returns true with no plane, an empty *out, and writes no file.
// threshold (world units) has no default.  The inlier floor is the larger of minInliers and ceil(minInlierFraction *
// the points taking part in the first round).  axis, upHint and the results' normal, rotation and translation are stated
// in `coord`.  Version 1 files are refused (SPZ_AMD_ERR_UNSUPPORTED).  false + one "[SPZ ERROR] levelSpz: …" line on a
// bad argument, an input that does not load, or a device failure.  SPZ_AMD_LEVEL_TIMING=1 prints the stages' times.
struct LevelOptions {
  enum class Select { None, Plane, OffPlane, Above, Below };
  double threshold = std::numeric_limits<double>::quiet_NaN();
  uint32_t hypotheses = 4096;           // 1 ... 65536
  uint64_t seed = 0;
  uint32_t stride = 1;
  uint32_t refine = 3;                  // 0 ... 16
  uint32_t planes = 1;                  // 1 ... 255
  uint64_t minInliers = 0;
  double minInlierFraction = 0.0;       // 0 ... 1
  std::optional<std::array<double, 3>> axis;
  double maxTilt = 90.0;                // degrees, with axis
  std::optional<std::array<double, 3>> upHint;
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;
  bool noTranslate = false;
  Select select = Select::None;         // levelSpz
  int32_t fractionalBits = 12;          // of the levelled file's positions (levelSpz, select == None)
};
struct DetectedPlane {
  std::array<int32_t, 3> normalInt = {0, 0, 0};   // (a, b, c), stored frame
  int64_t offsetInt = 0;                           // e
  uint64_t inliers = 0, sumAbs = 0, points = 0, above = 0, below = 0;
  uint32_t bestHypothesis = 0, refinements = 0;
  double fitness = 0.0, meanDistance = 0.0;
  std::array<double, 3> normal = {0.0, 0.0, 0.0};
  double offset = 0.0;
  std::array<double, 4> rotation = {0.0, 0.0, 0.0, 1.0};
  std::array<double, 3> translation = {0.0, 0.0, 0.0};
};
struct LevelResult {
  std::vector<DetectedPlane> planes;
  std::vector<uint8_t> labels;          // per input point: 0, or the 1-based plane it is an inlier of
  uint64_t threshold = 0;               // T
  double prepareMs = 0.0, scoreMs = 0.0, refineMs = 0.0;
  int64_t kept = -1;                    // levelSpz with a selection: the points written
};
bool detectPlanes(const DevicePackedGaussians &packed, const LevelOptions &options, LevelResult *result);
bool detectPlanes(const uint8_t *data, int32_t size, const LevelOptions &options, LevelResult *result);
bool detectPlanes(const std::string &filename, const LevelOptions &options, LevelResult *result);
bool levelSpz(const uint8_t *data, int32_t size, const LevelOptions &options, std::vector<uint8_t> *out,
              LevelResult *result);
bool levelSpz(const std::string &inputFilename, const std::string &outputFilename, const LevelOptions &options,
              LevelResult *result);
// Render (DESIGN §8 "Render"): the image of one pinhole view on the device (include/spz_amd.h "render" states the
// contract).  worldToCamera: [R | t] row-major, OpenCV axes (x right, y down, z forward), in the `coord` frame: the file
// is rendered as loadSpz(to = coord) returns it (renderCloud: the cloud as it is; coord is ignored).  *rgba: height x
// width x 4 floats, RGB + alpha, not clamped.  *entries (may be NULL): the (tile, Gaussian) entry count.  false + one
// "[SPZ ERROR] renderSpz: …" line on a bad argument (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG), an input that does
// not load, or a device failure.  renderCloud uploads the cloud and renders it on the device SPZ_AMD_DEVICE names
// (default 0), like the other host-memory entry points.  SPZ_AMD_RENDER_TIMING=1 prints the stages' times to stderr.
struct RenderOptions {
  std::array<float, 12> worldToCamera = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  float fx = 0.0f, fy = 0.0f, cx = 0.0f, cy = 0.0f;
  int width = 0, height = 0;
  float nearPlane = 0.2f;
  std::array<float, 3> background = {0.0f, 0.0f, 0.0f};
  int maxShDegree = 3;
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;
};
bool renderSpz(const std::string &filename, const RenderOptions &options, std::vector<float> *rgba,
               int64_t *entries = nullptr);
bool renderSpz(const uint8_t *data, int32_t size, const RenderOptions &options, std::vector<float> *rgba,
               int64_t *entries = nullptr);
bool renderCloud(const GaussianCloud &g, const RenderOptions &options, std::vector<float> *rgba,
                 int64_t *entries = nullptr);
// Depth maps (DESIGN §8 "Render"; include/spz_amd.h "render depth" states the contract): the view of renderSpz again,
// with per pixel the blend's depth sum `accumulated` = sum (T a) z, `alpha` = 1 - T, `expected` = accumulated / alpha in
// f32 (+inf where alpha == 0), `median` = the depth of the first Gaussian after which T < 0.5 (+inf: none) and `index`
// = that Gaussian's input index (0xffffffff: none), each height x width, row-major.  *rgba (may be NULL): the image,
// bit-identical to renderSpz's.  Errors as renderSpz's, the line naming renderSpzDepth.
struct DepthMaps {
  std::vector<float> expected, median, accumulated, alpha;
  std::vector<uint32_t> index;
};
bool renderSpzDepth(const std::string &filename, const RenderOptions &options, DepthMaps *maps,
                    std::vector<float> *rgba = nullptr, int64_t *entries = nullptr);
bool renderSpzDepth(const uint8_t *data, int32_t size, const RenderOptions &options, DepthMaps *maps,
                    std::vector<float> *rgba = nullptr, int64_t *entries = nullptr);
bool renderCloudDepth(const GaussianCloud &g, const RenderOptions &options, DepthMaps *maps,
                      std::vector<float> *rgba = nullptr, int64_t *entries = nullptr);
// The worldToCamera of a camera at `eye` looking at `target`: z = normalize(target - eye), x = normalize(z x up),
// y = z x x, so that `up` maps to -y (up on the screen).  std::invalid_argument when eye == target, up is zero or
// parallel to the view direction, or a value is not finite.
std::array<float, 12> lookAt(const std::array<float, 3> &eye, const std::array<float, 3> &target,
                             const std::array<float, 3> &up);
// Prune (DESIGN §8 "Prune"): significance pruning (include/spz_amd.h "render scores" and "prune" state the contract).
// Every Gaussian's blend weight T a is summed (and maximised) over the views on the device, the points are ranked by
// score (descending, then input index) and the kept ones are written as filterSpz would with the keep mask.  views:
// 1..1024 pinhole cameras (the camera fields of RenderOptions), all in the `coord` frame.  Exactly one rule: keepCount
// (0..n), keepFraction ([0, 1], K = min(n, ceil(f n))) or minScore (finite; the sum in pixel units, q 2^-24).  *kept
// (may be NULL): the kept count; *keepMask: one byte per input point, 1 = kept; *weightSum: the u64 sums q (pixel
// units times 2^24); *weightMax: the f32 maxima.  false + one "[SPZ ERROR] pruneSpz: …" line on a bad argument
// (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG; a bad view is named by its index), an input that does not load, or a
// device failure.  SPZ_AMD_PRUNE_TIMING=1 prints the stages' times to stderr.
struct PruneOptions {
  struct View {
    std::array<float, 12> worldToCamera = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    float fx = 0.0f, fy = 0.0f, cx = 0.0f, cy = 0.0f;
    int width = 0, height = 0;
  };
  enum Score { Sum = 0, Max = 1 };
  std::vector<View> views;
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;
  float nearPlane = 0.2f;
  Score score = Sum;
  std::optional<int64_t> keepCount;
  std::optional<double> keepFraction;
  std::optional<double> minScore;
};
bool pruneSpz(const uint8_t *data, int32_t size, const PruneOptions &options, std::vector<uint8_t> *out,
              int64_t *kept = nullptr, std::vector<uint8_t> *keepMask = nullptr,
              std::vector<uint64_t> *weightSum = nullptr, std::vector<float> *weightMax = nullptr);
bool pruneSpz(const std::string &inputFilename, const std::string &outputFilename, const PruneOptions &options,
              int64_t *kept = nullptr, std::vector<uint8_t> *keepMask = nullptr,
              std::vector<uint64_t> *weightSum = nullptr, std::vector<float> *weightMax = nullptr);
// n cameras (1..1024) on a Fibonacci sphere around `center` at distance distanceFactor * radius, each looking at the
// centre (lookAt), fx = fy = height / 2 / tan(fovY / 2), cx, cy = width / 2, height / 2.  up is +y, or +z for a view
// direction within 2.6 degrees of +-y, so no view is degenerate.  Callers without a centre and radius take them from the
// axis-aligned box of the decoded positions (centre and half diagonal); floaters inflate that box, so clean first or
// pass both.  std::invalid_argument on n outside 1..1024, a size outside 1..16384, fovY outside (0, 180), radius or
// distanceFactor not finite and > 0, or a centre that is not finite.
std::vector<PruneOptions::View> orbitViews(int n, const std::array<float, 3> &center, float radius, int width,
                                           int height, float fovY, float distanceFactor = 2.5f);
// The centre and half diagonal of the axis-aligned box of the finite positions (x, y, z triples) — orbitViews' defaults
// (the radius is at least 1e-6).  false when no position is finite.
bool boundingSphere(const std::vector<float> &positions, std::array<float, 3> *center, float *radius);
// A plain-text views file: one view per line, "width height fx fy cx cy r00 r01 r02 t0 r10 r11 r12 t1 r20 r21 r22 t2",
// blank lines and text after '#' ignored.  std::invalid_argument naming the line on a line that does not parse, a file
// that does not open or holds no view.  The cameras themselves are checked by pruneSpz.
std::vector<PruneOptions::View> loadViewsFile(const std::string &filename);
// Compare (DESIGN §8 "Compare"): PSNR, MSE, L1, max error and SSIM of two images on the device, in the convention of the
// 3DGS evaluation code (include/spz_amd.h "image metrics" states the contract: values clamped to [0, 1], NaN -> 0; the
// first three channels; an 11x11 Gaussian window of sigma 1.5 with zero padding).  compareSpz renders both files from
// every view (as renderSpz would, in the `coord` frame) and compares the two images of each view; the files may differ
// in point count, SH degree and version.  views: 1..1024 pinhole cameras (orbitViews, loadViewsFile).  *metrics: one
// result per view; *ssimMaps (may be NULL): per view the height x width map of S averaged over the channels.
// compareImages: two height x width x channels float32 images in host memory (channels 3 or 4 each), compared on the
// device SPZ_AMD_DEVICE names (default 0).  false + one "[SPZ ERROR] compareSpz: …" (compareImages: …) line on a bad
// argument (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG; a bad view is named by its index), an input that does not
// load, or a device failure.  SPZ_AMD_COMPARE_TIMING=1 prints the stages' times to stderr.
struct ImageMetrics {
  double mse = 0.0, psnr = 0.0, ssim = 0.0, l1 = 0.0, maxAbs = 0.0;
};
struct CompareOptions {
  std::vector<PruneOptions::View> views;
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;
  float nearPlane = 0.2f;
  std::array<float, 3> background = {0.0f, 0.0f, 0.0f};
  int maxShDegree = 3;
};
bool compareSpz(const std::string &fileA, const std::string &fileB, const CompareOptions &options,
                std::vector<ImageMetrics> *metrics, std::vector<std::vector<float>> *ssimMaps = nullptr);
bool compareSpz(const uint8_t *dataA, int32_t sizeA, const uint8_t *dataB, int32_t sizeB,
                const CompareOptions &options, std::vector<ImageMetrics> *metrics,
                std::vector<std::vector<float>> *ssimMaps = nullptr);
bool compareImages(const float *a, int channelsA, const float *b, int channelsB, int width, int height,
                   ImageMetrics *metrics, std::vector<float> *ssimMap = nullptr);
// Refine (DESIGN §8 "Refine"): a file fitted to a target file over views, closed-loop: the lossy edits (decimateSpz,
// pruneSpz, filterSpz to a lower degree, the coarse tiles of tileSpz) write a smaller file, compareSpz says what that
// cost, and refineSpz gives some of it back (include/spz_amd.h "image loss", "adam step" and "refine" state the
// contract).  The target is rendered once from every view; then `iterations` steps of Adam on the 3DGS loss
// (1 - lambdaDssim) l1 + lambdaDssim (1 - ssim), view i mod V at step i, over the arrays `train` names; then the trained
// sections are encoded again under the input's header, and the sections of untrained arrays keep the input's bytes.
// The defaults are 3DGS's published arguments; positionLr unset: 1.6e-4 times the radius of boundingSphere of the
// target's positions.  The report's "after" metrics are of the written stream, quantisation included.  The backward sums
// with f32 atomics, so two runs may differ in the last bits.  false + one "[SPZ ERROR] refineSpz: …" line on a bad
// argument (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG; a bad view is named by its index), an input that does not load,
// a version 1 input (SPZ_AMD_ERR_UNSUPPORTED), or a device failure.  SPZ_AMD_REFINE_TIMING=1 prints the stages' times.
// Densify (DESIGN §8 "Densify"; include/spz_amd.h "densify"): with interval > 0 refineSpz runs 3DGS's adaptive density
// control while it fits: after every `interval` iterations in [fromIter, untilIter) the Gaussians whose mean screen-space
// position gradient is at least gradThreshold are cloned (largest scale <= percentDense * extent) or split in two, and
// those with opacity under minOpacity (or a scale above maxScale, when set) are culled, never growing past maxPoints (0:
// the target's count).  extent 0: derived from the views' camera centres, as 3DGS does; one view cannot give one.
// Positions and scales must be trained, and alphas when opacityResetInterval > 0.  The output's header carries the new
// count; untrained sections keep the input's bytes, gathered from the point each output point descends from.
struct DensifyOptions {
  int interval = 0;  // 0 = off
  int fromIter = 500, untilIter = 15000;
  int opacityResetInterval = 0;  // 0 = off
  double gradThreshold = 2e-4, percentDense = 0.01, extent = 0.0, minOpacity = 0.005, maxScale = 0.0;
  uint64_t maxPoints = 0;
  uint64_t seed = 0;
};
struct DensifyRound {
  int iteration = 0;
  uint64_t cloned = 0, split = 0, culled = 0, refused = 0, numPoints = 0;
};
struct RefineOptions {
  enum Train { Positions = 1, Scales = 2, Rotations = 4, Alphas = 8, Colors = 16, Sh = 32, All = 63 };
  std::vector<PruneOptions::View> views;
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;
  float nearPlane = 0.2f;
  std::array<float, 3> background = {0.0f, 0.0f, 0.0f};
  int maxShDegree = 3;
  int iterations = 200;
  double lambdaDssim = 0.2;
  std::optional<double> positionLr;
  double scaleLr = 5e-3, rotationLr = 1e-3, alphaLr = 5e-2, colorLr = 2.5e-3, shLr = 2.5e-3 / 20.0;
  double beta1 = 0.9, beta2 = 0.999, eps = 1e-15;
  unsigned train = All;
  DensifyOptions densify;  // off by default
};
struct RefineReport {
  std::vector<double> history;               // the loss before each step
  std::vector<ImageMetrics> before, after;   // per view, against the target's render
  uint64_t skipped = 0;                      // non-finite elements the steps left alone, summed over the steps
  double positionLr = 0.0;                   // the rate used
  float ms[3] = {0.0f, 0.0f, 0.0f};          // targets + before, iterations + encode, after
  uint64_t numPoints = 0;                    // of the output (the input's, without densify)
  std::vector<DensifyRound> rounds;          // what each densify round did
};
bool refineSpz(const uint8_t *data, int32_t size, const uint8_t *target, int32_t targetSize, const RefineOptions &options,
               std::vector<uint8_t> *out, RefineReport *report = nullptr);
bool refineSpz(const std::vector<uint8_t> &data, const std::vector<uint8_t> &target, const RefineOptions &options,
               std::vector<uint8_t> *out, RefineReport *report = nullptr);
bool refineSpz(const std::string &inputFilename, const std::string &targetFilename, const std::string &outputFilename,
               const RefineOptions &options, RefineReport *report = nullptr);
// Fit (DESIGN §8 "Fit"): refineSpz against photographs instead of a target file (include/spz_amd.h "photo loss" and
// "refine images" state the contract).  images: one per view of `options.views`, of the view's size: pixels height x
// width x channels float32 (channels 3 or 4, the same for all), rows top to bottom, values in [0, 1] (loadImageFile);
// weights: null, or height x width float32 in [0, 1], what each pixel counts in the loss (an object mask, the sky, the
// rim of an undistorted frame).  fitExposure: a 3 x 4 colour transform [M | o] per image is fitted beside the cloud, as
// 3DGS does for auto-exposure and white balance, at rate exposureLr; the exposures start at the identity, come back in
// the report, and are never written into the file.  Every option of RefineOptions holds as in refineSpz; positionLr
// unset: 1.6e-4 times the radius of boundingSphere of the INPUT's positions; densify needs maxPoints (there is no
// target count).  The report's "before" is the input's render against the images, "after" the written stream's render,
// passed through that image's fitted exposure when fitExposure is set, against the images, both unweighted.  false + one
// "[SPZ ERROR] refineSpzToImages: …" line as refineSpz; an image whose size is not its view's names the view and both
// sizes.  SPZ_AMD_REFINE_TIMING=1 prints the stages' times.
// Depth (DESIGN §8 "Depth fit"; include/spz_amd.h "depth loss" and "refine images with depth"): an image may carry a
// measured depth map, height x width float32 of metric depth along the camera's z in scene units (LiDAR, an RGB-D rig,
// MVS, a render of a mesh; loadDepthFile), a value that is not finite or not > 0 meaning "no measurement".  The loss of
// an iteration on such a view gains depthWeight times the depth loss: the mean over the pixels with a measurement and
// an alpha of at least depthMinAlpha, weighted by the image's weights, of |expected depth - measured| (L1) or of the
// difference of their reciprocals (InverseL1, which counts near errors more).  With no image carrying a depth
// everything is as without these fields.  The report's depthHistory is the depth loss before each step (0 for a view
// without a map), depthError per view that of the input's and of the written stream's depth render against the map
// (-1 for a view without one); both are empty when no image carries a depth.
struct PhotoImage {
  const float *pixels = nullptr;
  int width = 0, height = 0, channels = 3;
  const float *weights = nullptr;
  const float *depth = nullptr;  // height x width, metric z
};
struct PhotoOptions {
  std::vector<PhotoImage> images;
  bool fitExposure = false;
  double exposureLr = 0.01;  // 3DGS's exposure_lr_init
  double depthWeight = 1.0;
  enum DepthKind { L1, InverseL1 } depthKind = L1;
  float depthMinAlpha = 0.5f;
};
struct PhotoReport {
  RefineReport refine;
  std::vector<std::array<double, 12>> exposures;  // per view, row-major [M | o]
  std::vector<double> depthHistory;
  std::vector<std::array<double, 2>> depthError;  // per view: before, after
};
bool refineSpzToImages(const uint8_t *data, int32_t size, const RefineOptions &options, const PhotoOptions &photo,
                       std::vector<uint8_t> *out, PhotoReport *report = nullptr);
bool refineSpzToImages(const std::vector<uint8_t> &data, const RefineOptions &options, const PhotoOptions &photo,
                       std::vector<uint8_t> *out, PhotoReport *report = nullptr);
bool refineSpzToImages(const std::string &inputFilename, const std::string &outputFilename, const RefineOptions &options,
                       const PhotoOptions &photo, PhotoReport *report = nullptr);
// Locate (DESIGN §8 "Locate"): the pose of the camera that took a picture of the scene in a file, from a rough guess
// (include/spz_amd.h "render view backward" and "locate" state the contract).  initial: the view with the rough pose, in
// the `coord` frame; image: height x width x channels float32 (channels 3 or 4), the picture, in the render's
// convention (rows top to bottom, values in [0, 1]).  `iterations` steps of Adam on the six values of a twist move the
// pose down the gradient of the 3DGS loss of the file's render against the picture; with levels > 1 the first steps run
// on 2 x 2 box means of the picture (width and height divisible by 2^(levels - 1)).  rotationLr: radians per step.
// translationLr unset: rotationLr times the distance from the initial camera centre to the centre of boundingSphere of
// the file's positions, and at least rotationLr times that sphere's radius.  The report's view is `initial` with its
// matrix replaced.  No search: the guess must be close enough for the two images to overlap.  The backward sums with
// f32 atomics, so two runs may differ in the last bits.  false + one "[SPZ ERROR] locateSpz: …" line on a bad argument
// (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG), an input that does not load, or a device failure.
// SPZ_AMD_LOCATE_TIMING=1 prints the stages' times.
struct LocateOptions {
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;
  float nearPlane = 0.2f;
  std::array<float, 3> background = {0.0f, 0.0f, 0.0f};
  int maxShDegree = 3;
  int iterations = 300;
  int levels = 1;
  double lambdaDssim = 0.2;
  double rotationLr = 2e-3;
  std::optional<double> translationLr;
  double lrFinalFactor = 0.1;
  double beta1 = 0.9, beta2 = 0.999, eps = 1e-15;
};
struct LocateReport {
  PruneOptions::View view;             // the initial view at the fitted pose
  std::vector<double> history;         // the loss before each step taken
  ImageMetrics before, after;          // the file's render against the picture at the initial and the fitted pose
  int iterations = 0;                  // steps taken (fewer than asked for: a gradient was not finite)
  double translationLr = 0.0;          // the rate used
  float ms[3] = {0.0f, 0.0f, 0.0f};    // before, iterations, after
};
bool locateSpz(const uint8_t *data, int32_t size, const PruneOptions::View &initial, const float *image, int channels,
               const LocateOptions &options, LocateReport *report);
bool locateSpz(const std::vector<uint8_t> &data, const PruneOptions::View &initial, const float *image, int channels,
               const LocateOptions &options, LocateReport *report);
bool locateSpz(const std::string &filename, const PruneOptions::View &initial, const float *image, int channels,
               const LocateOptions &options, LocateReport *report);
// A picture as spz_render writes it, as locateSpz takes it: a binary PPM ("P6", maxval 255: v / 255) or a colour PFM
// ("PF", either byte order, rows bottom to top in the file), three channels, rows top to bottom in *pixels.
// std::invalid_argument naming the file when it does not open or is neither.
void loadImageFile(const std::string &filename, std::vector<float> *pixels, int *width, int *height);
// A depth map as spz_render --depth writes it, as PhotoImage::depth takes it: a one-channel PFM ("Pf"), or the first
// channel of a colour PFM ("PF"); either byte order, rows bottom to top in the file and top to bottom in *pixels, the
// floats' bits kept (+inf stays +inf: no measurement).  std::invalid_argument naming the file when it does not open or
// is neither.
void loadDepthFile(const std::string &filename, std::vector<float> *pixels, int *width, int *height);
// Mesh (DESIGN §8 "Mesh"): a triangle mesh of a file, for software that does not speak Gaussians (include/spz_amd.h
// "mesh" states the contract).  The file's depth maps over the views (renderSpzDepth's, median depth by default) are
// fused on the device into a truncated signed distance volume, and its zero level set is extracted by marching
// tetrahedra: vertices, per-vertex colours (not clamped) and triangles, in a fixed order; a run repeats its bytes.
// views: 1..1024 pinhole cameras (orbitViews, loadViewsFile), all in the `coord` frame.  box: x0 y0 z0 x1 y1 z1 in
// `coord`; unset: the exact bounding box of the file's finite decoded positions, which floaters inflate (cleanSpz first,
// or pass a box).  Exactly one of voxelSize and resolution (lattice cells along the longest side of the box); neither:
// resolution 256.  truncation unset: 4 voxelSize.  Projective fusion marks up to `truncation` behind a surface seen at
// a grazing angle as inside, so the mesh of a closed object may open at the limbs of the view set.  false + one
// "[SPZ ERROR] meshSpz: …" line on a bad argument (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG; a bad view is named by
// its index), an input that does not load, or a device failure.  SPZ_AMD_MESH_TIMING=1 prints the stages' times.
struct MeshOptions {
  enum Depth { Median = 0, Expected = 1 };
  std::vector<PruneOptions::View> views;
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;
  float nearPlane = 0.2f;
  std::optional<std::array<double, 6>> box;
  std::optional<double> voxelSize;
  std::optional<int> resolution;
  std::optional<double> truncation;
  Depth depth = Median;
  float minAlpha = 0.5f;   // Expected: pixels of less alpha are not fused
  float minWeight = 1.0f;  // a cube emits when all 8 corners were seen by at least this many views
};
struct TriangleMesh {
  std::vector<float> vertices;      // x y z per vertex
  std::vector<float> colors;        // r g b per vertex, not clamped
  std::vector<uint32_t> triangles;  // three vertex numbers per triangle
  std::array<float, 3> lo = {0, 0, 0};  // the volume used: lattice points at lo + (i, j, k) voxelSize
  float voxelSize = 0.0f, truncation = 0.0f;
  std::array<uint32_t, 3> dims = {0, 0, 0};
  float ms[3] = {0.0f, 0.0f, 0.0f};  // renders, fuses, extraction
};
bool meshSpz(const uint8_t *data, int32_t size, const MeshOptions &options, TriangleMesh *mesh);
bool meshSpz(const std::string &filename, const MeshOptions &options, TriangleMesh *mesh);
// Seed (DESIGN §8 "Seed"): a file from posed photographs with depth maps (include/spz_amd.h "seed" states the contract):
// the first link of seedSpz -> refineSpzToImages with depths and densify -> cleanSpz -> tileSpz.  views: 1..1024 pinhole
// cameras in the `coord` frame; images: one per view, of the view's size, each with pixels (channels 3 or 4), depth
// (metric z; not finite or not > nearPlane: no measurement) and optionally weights (a sample counts above 0.5).  Every
// `stride`-th pixel with a measurement that the cloud built so far does not explain (its rendered alpha below coverAlpha,
// or its expected depth off by more than coverTolerance times the measurement) becomes an isotropic Gaussian of the
// lattice's spacing at that depth times scaleFactor, with the pixel's colour and `opacity`.  cover = false lifts every
// sample.  maxPoints 0: the sum of the views' sample counts, at most 10 M.  base / baseData: an existing file (its name,
// or its bytes when base is unset and baseData is not empty) of the same shDegree, decoded as the start of the cloud
// and used for the cover test only: the output holds the NEW points alone, under a version 3 header in `coord`, and
// mergeSpz joins it to the base without requantising.  A run repeats its bytes.  false + one "[SPZ ERROR] seedSpz: …"
// line on a bad argument (lastDeviceStatus() = SPZ_AMD_ERR_INVALID_ARG; a bad view is named by its index; an image
// whose size is not its view's names the view and both sizes; an image without depth names the view), a base that does
// not load, or a device failure.  SPZ_AMD_SEED_TIMING=1 prints the stages' times.
struct SeedOptions {
  std::vector<PruneOptions::View> views;
  CoordinateSystem coord = CoordinateSystem::UNSPECIFIED;
  float nearPlane = 0.2f;
  int stride = 1;
  double scaleFactor = 1.0;
  double opacity = 0.5;
  bool cover = true;
  float coverAlpha = 0.5f;
  float coverTolerance = 0.05f;
  int shDegree = 0;
  uint64_t maxPoints = 0;
  std::optional<std::string> base;
  std::vector<uint8_t> baseData;
};
struct SeedReport {
  struct View {
    uint64_t valid = 0, appended = 0, refused = 0;
  };
  std::vector<View> views;
  uint64_t numPoints = 0;            // of the output: the sum of the views' appended counts
  float ms[3] = {0.0f, 0.0f, 0.0f};  // cover renders, uploads + selects + emits, encode
};
bool seedSpz(const SeedOptions &options, const std::vector<PhotoImage> &images, std::vector<uint8_t> *out,
             SeedReport *report = nullptr);
bool seedSpz(const SeedOptions &options, const std::vector<PhotoImage> &images, const std::string &outputFilename,
             SeedReport *report = nullptr);
// A binary little-endian PLY: vertex properties x y z (float) and red green blue (uchar, rint(255 clamp(c, 0, 1)), NaN as
// 0), faces as "list uchar uint vertex_indices".  false + one "[SPZ ERROR] saveMeshPly: …" line when the arrays' sizes
// do not match (3 numVertices floats each, 3 numTriangles indices, every index below numVertices) or the file cannot be
// written.
bool saveMeshPly(const std::string &filename, const float *vertices, const float *colors, size_t numVertices,
                 const uint32_t *triangles, size_t numTriangles);
bool saveMeshPly(const std::string &filename, const TriangleMesh &mesh);
// Status (spz_amd.h codes) of the last device call made by this thread; 0 = ok.
int lastDeviceStatus();
void setLastDeviceStatus(int status);

// Tile (DESIGN §8 "Tile"): a file cut into an octree of level-of-detail tiles for streaming (include/spz_amd.h, "tile",
// states the contract).  The member is inflated (loadSpzPackedDevice), tiled on the device (spz_amd_tile_open), and every
// tile's stream is written as outDir/tile_%06u.spz with zlib's level-6 bytes (members under 1 MiB by zlib on at most 16
// threads, larger ones through compressGzipped), with outDir/tileset.json beside them.  outDir must be absent (it is
// created) or an empty directory; nothing is written when the arguments, the input or the tree (more than maxTiles tiles)
// are refused.  coord only flips the boxes' axes as coordinateConverter(RUB, coord) does; the tiles' bytes stay in the
// stored frame.  false + one "[SPZ ERROR] tileSpz: …" line on failure.  SPZ_AMD_TILE_TIMING=1 prints the stages' times.
struct TileOptions {
  uint32_t maxPoints = 65536;
  uint32_t maxTiles = 65536;
  CoordinateSystem coord = CoordinateSystem::RUB;
};
struct Tile {
  uint32_t id = 0;
  std::string file;
  int32_t parent = -1;
  std::vector<uint32_t> children;   // ascending Morton order
  int32_t level = 0;
  std::array<uint32_t, 3> cell = {0, 0, 0};
  int32_t contentLevel = -1;        // -1: a leaf
  uint32_t numPoints = 0;
  float geometricError = 0.0f;
  std::array<float, 3> boxMin = {0, 0, 0}, boxMax = {0, 0, 0};   // NaN for a tile without points
  float maxRadius = 0.0f;
};
struct Tileset {
  CoordinateSystem coord = CoordinateSystem::RUB;
  uint64_t numPoints = 0;
  int shDegree = 0, fractionalBits = 0;
  uint32_t maxPoints = 0;
  std::vector<Tile> tiles;          // tiles[i].id == i
};
bool tileSpz(const std::string &inputFilename, const std::string &outDir, const TileOptions &options,
             Tileset *tileset = nullptr);
// tileset.json written / read: floats are written so that they read back to the same f32 (NaN as null).
bool saveTileset(const Tileset &tileset, const std::string &path);
bool loadTileset(const std::string &path, Tileset *tileset);
// The screen-space-error cut, host only, float64.  A tile's sphere: the centre and half-diagonal of its box plus
// maxRadius; d = max(|centre - eye| - radius, nearPlane), eye = -R^T t of view.worldToCamera (in the tileset's coord
// frame); sse = geometricError max(fx, fy) / d.  Descends while sse > maxPixelError and the tile has children, else
// takes it.  Tile ids in tile order; every leaf has exactly one ancestor-or-self in the result.
std::vector<uint32_t> selectTiles(const Tileset &tileset, const PruneOptions::View &view, double maxPixelError,
                                  double nearPlane = 0.2);

}  // namespace spz
