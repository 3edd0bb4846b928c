// spz_host.cpp — C++ drop-in layer (namespace spz) over the C ABI of libspz_amd.so.
//
// Host-side mirror of the reference's save/load plumbing (/root/reference/src/cc/load-spz.cc
// :141-214 gzip, :533-596 (de)serialise, :598-668 saveSpz/loadSpz overloads), re-plumbed so
// that the per-Gaussian work goes through spz_amd_encode_host / spz_amd_decode_host and the
// stream is written/read in place (no stringstream double copy).
#include "spz_amd_host.hpp"

#include <dlfcn.h>
#include <unistd.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <dirent.h>
#include <cerrno>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <cctype>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <istream>
#include <limits>
#include <mutex>
#include <ostream>
#include <stdexcept>
#include <thread>

#include "spz_amd.h"
#include "spz_deflate.hpp"
#include "spz_host_util.hpp"
#include "spz_inflate.hpp"

namespace spz {
namespace {

thread_local int g_last_status = SPZ_AMD_OK;

// SpzLog, load-spz.cc:29-35: printf to stdout + newline + flush.
void logLine(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  std::vprintf(fmt, ap);
  va_end(ap);
  std::printf("\n");
  std::fflush(stdout);
}

int deviceIndex() {
  const char *e = std::getenv("SPZ_AMD_DEVICE");
  return e ? std::atoi(e) : 0;
}

int dimForDegree(int degree) {  // load-spz.cc:58-72
  switch (degree) {
    case 0: return 0;
    case 1: return 3;
    case 2: return 8;
    case 3: return 15;
    default:
      logLine("[SPZ: ERROR] Unsupported SH degree: %d\n", degree);
      return 0;
  }
}

#define SPZ_CHECK(x)                                             \
  if (!(x)) {                                                    \
    logLine("[SPZ: ERROR] Check failed: %s:%d: %s", __FILE__, __LINE__, #x); \
    return false;                                                \
  }

// checkSizes(const GaussianCloud&), load-spz.cc:106-117
bool checkSizes(const GaussianCloud &g) {
  SPZ_CHECK(g.numPoints >= 0);
  SPZ_CHECK(g.shDegree >= 0);
  SPZ_CHECK(g.shDegree <= 3);
  const size_t n = static_cast<size_t>(g.numPoints);
  SPZ_CHECK(g.positions.size() == n * 3);
  SPZ_CHECK(g.scales.size() == n * 3);
  SPZ_CHECK(g.rotations.size() == n * 4);
  SPZ_CHECK(g.alphas.size() == n);
  SPZ_CHECK(g.colors.size() == n * 3);
  SPZ_CHECK(g.sh.size() == n * dimForDegree(g.shDegree) * 3);
  return true;
}

// checkSizes(const PackedGaussians&, ...), load-spz.cc:119-127
bool checkSizes(const PackedGaussians &p, int32_t numPoints, int32_t shDim, bool usesFloat16) {
  const size_t n = static_cast<size_t>(numPoints);
  SPZ_CHECK(p.positions.size() == n * 3 * (usesFloat16 ? 2 : 3));
  SPZ_CHECK(p.scales.size() == n * 3);
  SPZ_CHECK(p.rotations.size() == n * (p.usesQuaternionSmallestThree ? 4 : 3));
  SPZ_CHECK(p.alphas.size() == n);
  SPZ_CHECK(p.colors.size() == n * 3);
  SPZ_CHECK(p.sh.size() == n * shDim * 3);
  return true;
}

bool deviceFailed(int rc, const char *what) {
  g_last_status = rc;
  if (rc == SPZ_AMD_OK) return false;
  logLine("[SPZ ERROR] spz_amd: %s: %s", what, spz_amd_status_string(rc));
  return true;
}

// Header checks of deserializePackedGaussians (load-spz.cc:551-568,591-594) with its log lines.
bool peekHeaderLogged(const uint8_t *stream, size_t size, spz_amd_header *hdr) {
  const int rc = spz_amd_peek_header(stream, size, hdr);
  switch (rc) {
    case SPZ_AMD_OK: return true;
    case SPZ_AMD_ERR_HEADER_NOT_FOUND:
      logLine("[SPZ ERROR] deserializePackedGaussians: header not found");
      break;
    case SPZ_AMD_ERR_VERSION: {
      uint32_t v = 0;
      std::memcpy(&v, stream + 4, 4);
      logLine("[SPZ ERROR] deserializePackedGaussians: version not supported: %d", v);
      break;
    }
    case SPZ_AMD_ERR_TOO_MANY_POINTS: {
      uint32_t n = 0;
      std::memcpy(&n, stream + 8, 4);
      logLine("[SPZ ERROR] deserializePackedGaussians: Too many points: %d", n);
      break;
    }
    case SPZ_AMD_ERR_SH_DEGREE:
      logLine("[SPZ ERROR] deserializePackedGaussians: Unsupported SH degree: %d", stream[12]);
      break;
    case SPZ_AMD_ERR_SHORT_STREAM:
      logLine("[SPZ ERROR] deserializePackedGaussians: read error");
      break;
    default:
      logLine("[SPZ ERROR] deserializePackedGaussians: %s", spz_amd_status_string(rc));
      break;
  }
  return false;
}

// File I/O of the overloads that take a file name (load-spz.cc:634-650, 652-668 use an ifstream / ofstream).  A 409 MB
// .spz through a zero-filled vector and one read() takes 0.15 s — more than the load itself — and a vector of 4 KiB
// pages then uploads at a tenth of the link's rate: the buffer is sized without being written, mapped with huge pages by
// several threads, and filled in 8 MiB pieces by several threads with pread: 409 MB 0.247 -> 0.133 s for the whole
// loadSpz(name).  Anything that is not a regular file of 16 MiB or more takes the reference's stream route.
using detail::fileIoThreads;
using detail::kParallelIoMin;
using detail::parallelRead;

bool readFileStream(const std::string &filename, std::vector<uint8_t> *data, bool log) {
  std::ifstream in(filename, std::ios::binary | std::ios::ate);
  if (!in.good()) {
    if (log) logLine("[SPZ ERROR] Unable to open: %s", filename.c_str());
    return false;
  }
  data->resize(static_cast<size_t>(in.tellg()));
  in.seekg(0, std::ios::beg);
  in.read(reinterpret_cast<char *>(data->data()), static_cast<std::streamsize>(data->size()));
  if (!in.good()) {
    if (log) logLine("[SPZ ERROR] Unable to load data from: %s", filename.c_str());
    return false;
  }
  return true;
}

bool readFile(const std::string &filename, std::vector<uint8_t> *data, bool log) {
  const int fd = fileIoThreads() == 0 ? -1 : ::open(filename.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd < 0) return readFileStream(filename, data, log);  // (its message for a file that cannot be opened)
  struct stat st;
  if (::fstat(fd, &st) != 0 || !S_ISREG(st.st_mode) || static_cast<size_t>(st.st_size) < kParallelIoMin) {
    ::close(fd);
    return readFileStream(filename, data, log);
  }
  const size_t size = static_cast<size_t>(st.st_size);
  data->clear();
  detail::resizeUninitialized(data, size);
  {
    detail::Prefault pf;
    pf.add(data->data(), size);
    pf.start();
    pf.join();
  }
  const bool ok = parallelRead(fd, data->data(), size);
  ::close(fd);
  if (!ok && log) logLine("[SPZ ERROR] Unable to load data from: %s", filename.c_str());
  return ok;
}

// The whole buffer into a new (or truncated) file; the result is what the reference's out.good() after close() says.
// (In pieces by several threads with pwrite, as the read: measured slower — 409 MB into a file in memory 127 ms with
// 8 threads, 183 with 4, against 82 ms for the one write() of the stream — the threads wait for each other where the
// file's pages are allocated.  So the reference's way.)
bool writeFile(const std::string &filename, const std::vector<uint8_t> &data) {
  std::ofstream out(filename, std::ios::binary | std::ios::out);
  out.write(reinterpret_cast<const char *>(data.data()), static_cast<std::streamsize>(data.size()));
  out.close();
  return out.good();
}

}  // namespace

unsigned effectiveCpuCount() { return detail::effectiveCpuCount(); }
int lastDeviceStatus() { return g_last_status; }
void setLastDeviceStatus(int status) { g_last_status = status; }

// ---- splat-types.h:43-81 ---------------------------------------------------------------------
CoordinateConverter coordinateConverter(CoordinateSystem from, CoordinateSystem to) {
  const int a = static_cast<int>(from) - 1, b = static_cast<int>(to) - 1;
  bool mx = true, my = true, mz = true;
  if (a >= 0 && b >= 0) {
    mx = ((a >> 0) & 1) == ((b >> 0) & 1);
    my = ((a >> 1) & 1) == ((b >> 1) & 1);
    mz = ((a >> 2) & 1) == ((b >> 2) & 1);
  }
  const float x = mx ? 1.0f : -1.0f, y = my ? 1.0f : -1.0f, z = mz ? 1.0f : -1.0f;
  CoordinateConverter c;
  c.flipP = {x, y, z};
  c.flipQ = {y * z, x * z, x * y};
  c.flipSh = {y, z, x, x * y, y * z, 1.0f, x * z, 1.0f, y, x * y * z, y, z, x, z, x};
  return c;
}

// ---- GaussianCloud methods ---------------------------------------------------------------------
void GaussianCloud::convertCoordinates(CoordinateSystem from, CoordinateSystem to) {
  g_last_status = SPZ_AMD_OK;
  if (numPoints == 0) return;  // splat-types.h:135-138
  // The reference derives the per-point sh count from the array sizes (splat-types.h:151-152).
  const size_t coeffs = sh.size() / 3 / static_cast<size_t>(numPoints);
  int degree = -1;
  for (int d = 0; d <= 3; ++d) {
    if (static_cast<size_t>(dimForDegree(d)) == coeffs) degree = d;
  }
  if (degree < 0) {
    logLine("[SPZ ERROR] spz_amd: convertCoordinates: unsupported sh size %zu for %d points", sh.size(),
            numPoints);
    return;
  }
  const int f = static_cast<int>(from), t = static_cast<int>(to), dev = deviceIndex();
  const size_t n = static_cast<size_t>(numPoints);
  if (positions.size() == n * 3 && rotations.size() == n * 4 && sh.size() == n * coeffs * 3) {
    deviceFailed(spz_amd_convert_coordinates_host(positions.empty() ? nullptr : positions.data(),
                                                  rotations.empty() ? nullptr : rotations.data(),
                                                  sh.empty() ? nullptr : sh.data(), n, degree, f, t, dev),
                 "convertCoordinates");
    return;
  }
  // Inconsistent sizes: each array is walked over its own length, like the reference loops.
  if (positions.size() >= 3) {
    deviceFailed(spz_amd_convert_coordinates_host(positions.data(), nullptr, nullptr, positions.size() / 3, 0, f,
                                                  t, dev), "convertCoordinates");
  }
  if (rotations.size() >= 4) {
    deviceFailed(spz_amd_convert_coordinates_host(nullptr, rotations.data(), nullptr, rotations.size() / 4, 0, f,
                                                  t, dev), "convertCoordinates");
  }
  if (coeffs > 0) {
    deviceFailed(spz_amd_convert_coordinates_host(nullptr, nullptr, sh.data(), n, degree, f, t, dev),
                 "convertCoordinates");
  }
}

float GaussianCloud::medianVolume() const {  // splat-types.h:170-185
  g_last_status = SPZ_AMD_OK;
  if (numPoints == 0 || scales.size() < 3) return 0.01f;
  // Selection of the middle scale sum on the device (no sort); the volume is one scalar on top of it.
  float median = 0.0f;
  if (deviceFailed(spz_amd_median_scale_sum_host(scales.data(), scales.size() / 3, &median, deviceIndex()),
                   "medianVolume")) {
    return 0.01f;
  }
  return static_cast<float>((M_PI * 4 / 3) * std::exp(median));
}

GaussianCloudData GaussianCloud::data() const {  // splat-types.h:14-22,117-130
  auto copy = [](const std::vector<float> &v) {
    SpzFloatBuffer b = {0, nullptr};
    if (!v.empty()) {
      b.count = v.size();
      b.data = new float[b.count];
      std::memcpy(b.data, v.data(), b.count * sizeof(float));
    }
    return b;
  };
  GaussianCloudData d;
  d.numPoints = numPoints;
  d.shDegree = shDegree;
  d.antialiased = antialiased;
  d.positions = copy(positions);
  d.scales = copy(scales);
  d.rotations = copy(rotations);
  d.alphas = copy(alphas);
  d.colors = copy(colors);
  d.sh = copy(sh);
  return d;
}

// ---- per-splat access, load-spz.cc:383-463 --------------------------------------------------------
PackedGaussian PackedGaussians::at(int32_t i) const {  // byte moves only
  PackedGaussian r;
  const size_t k = static_cast<size_t>(i);
  const size_t positionBytes = usesFloat16() ? 6 : 9;
  std::copy_n(positions.data() + k * positionBytes, positionBytes, r.position.data());
  std::copy_n(scales.data() + k * 3, 3, r.scale.data());
  const size_t rotationBytes = usesQuaternionSmallestThree ? 4 : 3;
  std::copy_n(rotations.data() + k * rotationBytes, rotationBytes, r.rotation.data());
  std::copy_n(colors.data() + k * 3, 3, r.color.data());
  r.alpha = alphas[k];
  const size_t shDim = static_cast<size_t>(dimForDegree(shDegree));
  const uint8_t *p = sh.data() + k * shDim * 3;
  for (size_t j = 0; j < 15; ++j) {
    const bool have = j < shDim;
    r.shR[j] = have ? p[3 * j + 0] : 128;
    r.shG[j] = have ? p[3 * j + 1] : 128;
    r.shB[j] = have ? p[3 * j + 2] : 128;
  }
  return r;
}

UnpackedGaussian PackedGaussians::unpack(int32_t i, const CoordinateConverter &c) const {
  return at(i).unpack(usesFloat16(), usesQuaternionSmallestThree, fractionalBits, c);
}

namespace {

// The coordinate system X for which coordinateConverter(RUB, X) equals `c`, or -1 when `c` is not a
// table coordinateConverter can produce.  (enum - 1: bit 0 = R, bit 1 = U, bit 2 = F; RUB = 0b011.)
int targetSystemOf(const CoordinateConverter &c) {
  for (float v : c.flipP) {
    if (v != 1.0f && v != -1.0f) return -1;
  }
  const int bits = (c.flipP[0] > 0 ? 1 : 0) | (c.flipP[1] > 0 ? 2 : 0) | (c.flipP[2] > 0 ? 0 : 4);
  const CoordinateSystem to = static_cast<CoordinateSystem>(bits + 1);
  const CoordinateConverter want = coordinateConverter(CoordinateSystem::RUB, to);
  if (want.flipP != c.flipP || want.flipQ != c.flipQ || want.flipSh != c.flipSh) return -1;
  return static_cast<int>(to);
}

// One point as a complete SH3 stream: header + the six sections (load-spz.cc:540-545).
size_t onePointStream(const PackedGaussian &g, uint32_t version, int32_t fractionalBits, uint8_t *out) {
  spz_amd_header h = {};
  h.version = version;
  h.num_points = 1;
  h.sh_degree = 3;
  h.fractional_bits = static_cast<uint8_t>(fractionalBits);
  spz_amd_write_header(&h, out);
  uint8_t *p = out + 16;
  const size_t positionBytes = version == 1 ? 6 : 9, rotationBytes = version >= 3 ? 4 : 3;
  p = std::copy_n(g.position.data(), positionBytes, p);
  *p++ = g.alpha;
  p = std::copy_n(g.color.data(), 3, p);
  p = std::copy_n(g.scale.data(), 3, p);
  p = std::copy_n(g.rotation.data(), rotationBytes, p);
  for (size_t j = 0; j < 15; ++j) {
    *p++ = g.shR[j];
    *p++ = g.shG[j];
    *p++ = g.shB[j];
  }
  return static_cast<size_t>(p - out);
}

struct OnePoint {
  float position[3], scale[3], rotation[4], alpha[1], color[3], sh[45];
};

bool decodeOnePoint(const PackedGaussian &g, uint32_t version, int32_t fractionalBits, int to, OnePoint *r) {
  uint8_t stream[16 + 9 + 1 + 3 + 3 + 4 + 45];
  const size_t size = onePointStream(g, version, fractionalBits, stream);
  spz_amd_cloud_out out = {r->position, r->scale, r->rotation, r->alpha, r->color, r->sh};
  return !deviceFailed(spz_amd_decode_host_ex(stream, size, 0, to, &out, deviceIndex()), "PackedGaussian::unpack");
}

}  // namespace

UnpackedGaussian PackedGaussian::unpack(bool usesFloat16, bool usesQuaternionSmallestThree, int32_t fractionalBits,
                                        const CoordinateConverter &c) const {
  g_last_status = SPZ_AMD_OK;
  UnpackedGaussian result = {};
  const int to = targetSystemOf(c);
  if (to < 0) {
    logLine("[SPZ ERROR] spz_amd: PackedGaussian::unpack: the CoordinateConverter is not one coordinateConverter() makes");
    g_last_status = SPZ_AMD_ERR_INVALID_ARG;
    return result;
  }
  // stream versions: 1 = float16 positions + first-three rotations, 2 = 24-bit + first-three,
  // 3 = 24-bit + smallest-three.  The fourth combination the signature allows (float16 with
  // smallest-three, which no stream version encodes) takes positions from a v1 and the rest from a v3 decode.
  OnePoint a;
  const uint32_t version = usesQuaternionSmallestThree ? 3u : (usesFloat16 ? 1u : 2u);
  if (!decodeOnePoint(*this, version, fractionalBits, to, &a)) return result;
  if (usesFloat16 && usesQuaternionSmallestThree) {
    OnePoint b;
    if (!decodeOnePoint(*this, 1u, fractionalBits, to, &b)) return result;
    std::copy_n(b.position, 3, a.position);
  }
  std::copy_n(a.position, 3, result.position.data());
  std::copy_n(a.rotation, 4, result.rotation.data());
  std::copy_n(a.scale, 3, result.scale.data());
  std::copy_n(a.color, 3, result.color.data());
  result.alpha = a.alpha[0];
  for (size_t j = 0; j < 15; ++j) {
    result.shR[j] = a.sh[3 * j + 0];
    result.shG[j] = a.sh[3 * j + 1];
    result.shB[j] = a.sh[3 * j + 2];
  }
  return result;
}

bool PackedGaussians::usesFloat16() const {  // load-spz.cc:465
  return positions.size() == static_cast<size_t>(numPoints) * 3 * 2;
}

// ---- gzip, load-spz.cc:141-214 -------------------------------------------------------------------
namespace {
// Threads for the byte-identical parallel writer (spz_deflate.cpp): SPZ_AMD_GZIP_EXACT_THREADS, default
// min(cores, 32); 0 or 1 keeps everything in zlib.
int exactGzipThreads() {
  const char *e = std::getenv("SPZ_AMD_GZIP_EXACT_THREADS");
  if (e) return std::max(0, std::atoi(e));
  return static_cast<int>(std::min<unsigned>(detail::effectiveCpuCount(), 32u));
}
}  // namespace

namespace {

// Physical memory the machine has free right now (0 if unknown).
size_t availablePhysicalBytes() {
  const long pages = sysconf(_SC_AVPHYS_PAGES), page = sysconf(_SC_PAGESIZE);
  return (pages > 0 && page > 0) ? static_cast<size_t>(pages) * static_cast<size_t>(page) : 0;
}

// What a member of the parallel writers has been through before it is returned:
//   always        the first 64-256 KiB compared with zlib's own output; every Huffman block's bit count compared with the
//                 layout's plan; and on the device route every symbol checked against the input on the device
//                 (lz_validate_kernel: literals are their input bytes, matches copy equal bytes, blocks cover their
//                 ranges) — the LZ77 stage can only be lossless, whatever the parse kernels did.
//   SPZ_AMD_GZIP_VERIFY=1  additionally the finished member is inflated and compared with the input byte for byte
//                 before it is returned: on the device route by the device reader on the body still in HBM
//                 (spz_amd_zlib_verify_member, ~0.1 s for a 650 MB stream), otherwise by the host readers.
//   SPZ_AMD_GZIP_VERIFY=2  additionally zlib itself runs over the whole input and the two members are compared byte for
//                 byte (the identity claim itself, at zlib's price).
// A failed check discards the member, logs, and the next writer down (host writer, then zlib) produces it.
int gzipVerifyLevel() {
  const char *e = std::getenv("SPZ_AMD_GZIP_VERIFY");
  return e ? std::max(0, std::atoi(e)) : 0;
}

bool compressGzippedZlib(const uint8_t *data, size_t size, std::vector<uint8_t> *out);

bool verifiedExact(const uint8_t *data, size_t size, const std::vector<uint8_t> &member, int level, bool inflated_already = false) {
  if (level >= 1 && !inflated_already) {
    std::vector<uint8_t> back;
    if (!decompressGzipped(member.data(), member.size(), &back) || back.size() != size ||
        std::memcmp(back.data(), data, size) != 0) {
      logLine("[SPZ ERROR] spz_amd: the parallel gzip writer's member does not inflate to its input; using zlib");
      return false;
    }
  }
  if (level >= 2) {
    std::vector<uint8_t> z;
    if (!compressGzippedZlib(data, size, &z) || z != member) {
      logLine("[SPZ ERROR] spz_amd: the parallel gzip writer's bytes differ from zlib's; using zlib");
      return false;
    }
  }
  return true;
}

std::atomic<uint64_t> g_device_rejects{0};  // members of the device writer that failed a check and were not returned

// The LZ77 parse of the exact writer on the MI355X (spz_lz77.hip): SPZ_AMD_GZIP_DEVICE = 0 never, 1 whenever a
// device answers, unset: for inputs of 2 MiB and more when a device answers.
struct DeviceHeadParser final : exactgz::HeadParser {
  void *ctx = nullptr;
  int status = SPZ_AMD_OK;
  const uint8_t *d_copy = nullptr;  // the input's bytes on the device already (saveSpz), or null
  void *session = nullptr;          // a parse whose first stages were fed while the input was produced (saveSpz), or null
  ~DeviceHeadParser() override {
    spz_amd_zlib_parse_close(ctx);
    spz_amd_zlib_session_close(session);
  }
  int open(const uint8_t *data, size_t size, uint64_t tail_begin, const uint32_t *tail_rec, uint32_t n_rec, void (*produce)(void *),
           void *arg, uint64_t *num_symbols, uint32_t *tail_first_symbol) {
    if (session != nullptr) {  // consumed by the call, whatever it returns
      void *q = session;
      session = nullptr;
      return spz_amd_zlib_parse_open_session(q, data, d_copy, size, tail_begin, tail_rec, n_rec, &ctx, num_symbols, tail_first_symbol,
                                             produce, arg);
    }
    return spz_amd_zlib_parse_open_dev(data, d_copy, size, tail_begin, tail_rec, n_rec, deviceIndex(), &ctx, num_symbols,
                                       tail_first_symbol, produce, arg);
  }
  bool parse(const uint8_t *data, size_t size, uint64_t tail_begin, const uint32_t *tail_rec, uint32_t n_rec,
             uint64_t *num_symbols, uint32_t *tail_first_symbol) override {
    status = open(data, size, tail_begin, tail_rec, n_rec, nullptr, nullptr, num_symbols, tail_first_symbol);
    return status == SPZ_AMD_OK;
  }
  bool parseLate(const uint8_t *data, size_t size, uint64_t tail_begin, const uint32_t *tail_rec, uint32_t n_rec,
                 void (*produce)(void *), void *arg, uint64_t *num_symbols, uint32_t *tail_first_symbol) override {
    status = open(data, size, tail_begin, tail_rec, n_rec, produce, arg, num_symbols, tail_first_symbol);
    return status == SPZ_AMD_OK;
  }
  bool fetch(uint16_t *dist, uint8_t *lc) override {
    status = spz_amd_zlib_parse_fetch(ctx, dist, lc);
    return status == SPZ_AMD_OK;
  }
  // SPZ_AMD_GZIP_DEVICE_HUFFMAN=0: symbols come back and the host codes them (the parse alone on the device)
  bool canFinish() const override {
    const char *e = std::getenv("SPZ_AMD_GZIP_DEVICE_HUFFMAN");
    return !(e && e[0] == '0');
  }
  bool append(const uint16_t *dist, const uint8_t *lc, size_t n) override {
    status = spz_amd_zlib_parse_append(ctx, dist, lc, n);
    return status == SPZ_AMD_OK;
  }
  bool blockStats(const spz_amd_deflate_static &t, uint32_t block_syms, uint32_t nblocks, uint16_t *lfreq, uint16_t *dfreq,
                  uint32_t *bytes, uint32_t *last_len) override {
    status = spz_amd_zlib_block_stats(ctx, &t, block_syms, nblocks, lfreq, dfreq, bytes, last_len);
    return status == SPZ_AMD_OK;
  }
  bool canBuildTrees() const override {
    const char *e = std::getenv("SPZ_AMD_GZIP_DEVICE_TREES");
    return !(e && e[0] == '0');
  }
  bool blockTrees(uint32_t total, spz_amd_deflate_plan *plan) override {
    status = spz_amd_zlib_block_trees(ctx, total, plan);
    return status == SPZ_AMD_OK;
  }
  bool encodePlanned(const spz_amd_deflate_static &t, uint32_t block_syms, uint32_t total, const spz_amd_deflate_block *blocks,
                     uint64_t body_bytes) override {
    status = spz_amd_zlib_encode_planned(ctx, &t, block_syms, total, blocks, body_bytes);
    return status == SPZ_AMD_OK;
  }
  bool encodeGroup(const spz_amd_deflate_static &t, uint32_t block_syms, uint32_t total, uint32_t first, uint32_t n,
                   const spz_amd_deflate_block *blocks, const spz_amd_deflate_codes *codes, const uint32_t *words, uint64_t nwords,
                   uint64_t body_bytes_bound) override {
    status = spz_amd_zlib_encode_group(ctx, &t, block_syms, total, first, n, blocks, codes, words, nwords, body_bytes_bound);
    return status == SPZ_AMD_OK;
  }
  bool encodeFinish(uint32_t total, uint64_t body_bytes, uint8_t *body, uint64_t *symbol_bits, uint32_t *header_bits) override {
    status = spz_amd_zlib_encode_finish_ex(ctx, total, body_bytes, body, symbol_bits, header_bits);
    return status == SPZ_AMD_OK;
  }
  // SPZ_AMD_GZIP_VERIFY >= 1: the body, still in device memory, inflated there and compared with the input byte for byte
  int verifyMember(uint64_t body_bytes) { return spz_amd_zlib_verify_member(ctx, body_bytes); }
};

bool deviceParseWanted(size_t size) {
  const char *e = std::getenv("SPZ_AMD_GZIP_DEVICE");
  if (e && e[0] == '0') return false;
  const bool forced = e && e[0] == '1';
  // profiles/r03_size_sweep.json: the device writer wins from the smallest stream measured (60 k points SH3, 3.9 MB:
  // 13 ms against 53 ms for the multi-threaded host writer on the box's 16 CPUs)
  if (!forced && size < (size_t(2) << 20)) return false;
  return spz_amd_device_count() > 0;
}

std::atomic<uint64_t> g_device_parses{0};

}  // namespace

uint64_t deviceGzipParseCount() { return g_device_parses.load(); }
uint64_t deviceGzipRejectCount() { return g_device_rejects.load(); }

namespace {
// A saveSpz whose container stage has been fed beside the upload: the session, and the writer's tail job started as soon
// as the stream's last bytes were on the host
struct SaveAhead {
  void *session = nullptr;
  exactgz::TailAhead *tail = nullptr;
  const uint8_t *stream = nullptr;
  size_t size = 0;
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  ~SaveAhead() {
    if (session) spz_amd_zlib_session_close(session);
    exactgz::tailAheadDrop(tail);
  }
};
bool compressGzippedWithCopy(const uint8_t *data, size_t size, std::vector<uint8_t> *out, const uint8_t *d_copy, SaveAhead *ahead = nullptr);
}
bool compressGzipped(const uint8_t *data, size_t size, std::vector<uint8_t> *out) {
  return compressGzippedWithCopy(data, size, out, nullptr);
}
namespace {
// d_copy: the same bytes on the device (spz_amd_encode_host_keep), or null; ahead: a parse already fed with them and the
// tail job already started on them (both taken; what is not consumed here goes with *ahead)
bool compressGzippedWithCopy(const uint8_t *data, size_t size, std::vector<uint8_t> *out, const uint8_t *d_copy, SaveAhead *ahead) {
  // Large inputs: the writer that reproduces zlib's bytes exactly with its parse on the device or on all
  // cores (it checks itself against zlib on a prefix, and declines inputs it cannot split); zlib itself
  // otherwise and as the fallback.
  constexpr size_t kExactMinBytes = size_t(1) << 20;
  if (size >= kExactMinBytes && std::strcmp(zlibVersion(), "1.2.11") == 0) {
    const int threads = exactGzipThreads();
    if (threads >= 1 && deviceParseWanted(size)) {
      const size_t verify = std::min<size_t>(size_t(256) << 10, std::max<size_t>(size_t(64) << 10, size / 16));
      const size_t avail = availablePhysicalBytes();
      if (avail == 0 || size / 2 * 9 < avail) {
        static const bool timing = std::getenv("SPZ_AMD_EXACT_GZIP_TIMING") != nullptr;
        const auto t0 = std::chrono::steady_clock::now();
        bool ok;
        const int level = gzipVerifyLevel();
        bool inflated_on_device = false;
        {
          DeviceHeadParser parser;
          parser.d_copy = d_copy;
          exactgz::TailAhead *tail = nullptr;
          if (ahead && d_copy) {
            parser.session = ahead->session;
            ahead->session = nullptr;
            tail = ahead->tail;
            ahead->tail = nullptr;
          }
          ok = exactgz::compressWithHeadParser(data, size, std::max(threads, 1), parser, out, verify, tail);
          if (timing) {
            std::fprintf(stderr, "[exactgz] writer     %.3f s in all\n",
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
          }
          if (!ok && parser.status == SPZ_AMD_ERR_VERIFY) {
            g_device_rejects.fetch_add(1);
            logLine("[SPZ ERROR] spz_amd: the device gzip writer's symbols do not reproduce the input; using the host writer");
          }
          if (ok && level >= 1 && out->size() > 18) {
            const int rc = parser.verifyMember(out->size() - 18);
            if (rc == SPZ_AMD_OK) {
              inflated_on_device = true;
            } else if (rc == SPZ_AMD_ERR_VERIFY) {
              g_device_rejects.fetch_add(1);
              logLine("[SPZ ERROR] spz_amd: the device gzip writer's member does not inflate to its input; using the host writer");
              ok = false;
            }  // anything else: the device reader declined, the host inflates below
            if (timing) {
              std::fprintf(stderr, "[exactgz] + verify   %.3f s in all (device reader: %s)\n",
                           std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(), spz_amd_status_string(rc));
            }
          }
        }
        if (timing) {
          std::fprintf(stderr, "[exactgz] + release  %.3f s in all\n",
                       std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        }
        if (ok) {
          // level 1 is done when the device has inflated and compared; level 2 (zlib's own member) is the host's either way
          if (level == 0 || (level == 1 && inflated_on_device) || verifiedExact(data, size, *out, inflated_on_device ? 2 : level, inflated_on_device)) {
            g_device_parses.fetch_add(1);
            return true;
          }
        }
      }
    }
    // parse jobs of 1 MiB; smaller ones (down to 128 KiB) when that is what it takes to give every thread two
    const int windows = static_cast<int>(std::min<size_t>(32, std::max<size_t>(4, size / (size_t(threads > 0 ? threads : 1) * 2 * 32768))));
    const size_t verify = std::min<size_t>(size_t(256) << 10, std::max<size_t>(size_t(64) << 10, size / 16));
    // The writer keeps every job's symbols until assembly: about 3 bytes per input byte plus the output, where
    // zlib needs under 1 MB.  A host that does not have that to spare gets zlib's pace instead of the OOM killer.
    const size_t avail = availablePhysicalBytes();
    const bool fits = avail == 0 || size / 2 * 9 < avail;   // 4.5 x the input
    if (threads > 1 && fits && exactgz::compress(data, size, threads, windows, out, verify)) {
      const int level = gzipVerifyLevel();
      if (level == 0 || verifiedExact(data, size, *out, level)) return true;
    }
  }
  return compressGzippedZlib(data, size, out);
}
}  // namespace

namespace {
bool compressGzippedZlib(const uint8_t *data, size_t size, std::vector<uint8_t> *out) {
  z_stream stream = {};
  // Same parameters as load-spz.cc:190: default level, gzip wrapper, memLevel 9.
  if (deflateInit2(&stream, Z_DEFAULT_COMPRESSION, Z_DEFLATED, 16 + MAX_WBITS, 9, Z_DEFAULT_STRATEGY) != Z_OK) {
    return false;
  }
  out->clear();
  std::vector<uint8_t> buffer(1u << 20);
  const uint8_t *next = data;
  size_t left = size;
  bool success = false;
  while (true) {
    // deflate output does not depend on how the input is chunked; feed at most 1 GiB per call.
    const size_t chunk = std::min<size_t>(left, size_t(1) << 30);
    stream.next_in = const_cast<Bytef *>(reinterpret_cast<const Bytef *>(next));
    stream.avail_in = static_cast<uInt>(chunk);
    next += chunk;
    left -= chunk;
    const int flush = (left == 0) ? Z_FINISH : Z_NO_FLUSH;
    int res = Z_OK;
    do {
      stream.next_out = buffer.data();
      stream.avail_out = static_cast<uInt>(buffer.size());
      res = deflate(&stream, flush);
      if (res != Z_OK && res != Z_STREAM_END && res != Z_BUF_ERROR) break;
      out->insert(out->end(), buffer.data(), buffer.data() + (buffer.size() - stream.avail_out));
    } while (stream.avail_out == 0 || (flush == Z_FINISH && res != Z_STREAM_END));
    if (res == Z_STREAM_END) {
      success = true;
      break;
    }
    if ((res != Z_OK && res != Z_BUF_ERROR) || left == 0) break;
  }
  deflateEnd(&stream);
  return success;
}
}  // namespace

// ---- opt-in parallel gzip ---------------------------------------------------------
// zlib is ~87 % of an end-to-end saveSpz.  This is pigz's "independent blocks"
// construction: the input is cut into blocks, every block is deflated on its own (raw deflate, ended
// on a byte boundary with Z_SYNC_FLUSH; the last one with Z_FINISH), and the pieces are concatenated
// inside ONE gzip member whose CRC-32 is folded together with crc32_combine.  Any gzip reader, the
// reference's loadSpz included, reads the result; the bytes differ from single-stream deflate, so it
// is used only when asked for (threads > 1).  The member's header carries an FEXTRA subfield "SZ"
// (RFC 1952 §2.3.1.1; readers that do not know it skip it) listing the compressed size of every piece,
// which is what lets decompressGzipped below inflate the pieces concurrently.
namespace {

constexpr uint8_t kIndexId1 = 'S', kIndexId2 = 'Z';
constexpr uint32_t kIndexVersion = 1;

struct GzipIndex {
  uint32_t blockBytes = 0;            // uncompressed bytes per piece (the last may be shorter)
  uint64_t totalBytes = 0;            // uncompressed size of the member
  std::vector<uint32_t> pieceBytes;   // compressed size of every piece
};

void putLe(std::vector<uint8_t> *v, uint64_t x, int bytes) {
  for (int k = 0; k < bytes; ++k) v->push_back(static_cast<uint8_t>(x >> (8 * k)));
}
uint64_t getLe(const uint8_t *p, int bytes) {
  uint64_t x = 0;
  for (int k = 0; k < bytes; ++k) x |= static_cast<uint64_t>(p[k]) << (8 * k);
  return x;
}

// Walks a gzip member header (RFC 1952 §2.3).  Returns its length, 0 if it is not one; fills *idx when
// an "SZ" subfield of the known version is present.
size_t parseGzipHeader(const uint8_t *p, size_t n, GzipIndex *idx) {
  if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || (p[3] & 0xe0)) return 0;
  const uint8_t flg = p[3];
  size_t pos = 10;
  if (flg & 4) {  // FEXTRA
    if (pos + 2 > n) return 0;
    const size_t xlen = getLe(p + pos, 2);
    pos += 2;
    if (pos + xlen > n) return 0;
    size_t q = pos;
    while (q + 4 <= pos + xlen) {
      const size_t len = getLe(p + q + 2, 2);
      if (q + 4 + len > pos + xlen) break;
      const uint8_t *d = p + q + 4;
      if (p[q] == kIndexId1 && p[q + 1] == kIndexId2 && len >= 20 && getLe(d, 4) == kIndexVersion) {
        const uint64_t nb = getLe(d + 16, 4);
        if (20 + 4 * nb == len) {
          idx->blockBytes = static_cast<uint32_t>(getLe(d + 4, 4));
          idx->totalBytes = getLe(d + 8, 8);
          idx->pieceBytes.resize(nb);
          for (uint64_t i = 0; i < nb; ++i) idx->pieceBytes[i] = static_cast<uint32_t>(getLe(d + 20 + 4 * i, 4));
        }
      }
      q += 4 + len;
    }
    pos += xlen;
  }
  for (int f = 8; f <= 16; f <<= 1) {  // FNAME, FCOMMENT: zero-terminated
    if (flg & f) {
      while (pos < n && p[pos] != 0) ++pos;
      if (pos >= n) return 0;
      ++pos;
    }
  }
  // FHCRC: zlib checks the header CRC16 and rejects a member whose CRC16 is wrong; the fast readers start
  // behind the header and would not.  The reference writer never sets it, so such members go to zlib.
  if (flg & 2) return 0;
  return pos + 8 <= n ? pos : 0;
}

int gunzipThreads(size_t pieces) {
  const char *e = std::getenv("SPZ_AMD_GUNZIP_THREADS");
  size_t t = e ? static_cast<size_t>(std::max(1, std::atoi(e))) : std::min<size_t>(detail::effectiveCpuCount(), 32);
  return static_cast<int>(std::max<size_t>(1, std::min(t, pieces)));
}

// Inflates the pieces of an indexed member concurrently, straight into their final positions.  Every
// size, the CRC-32 and ISIZE are checked; on ANY inconsistency the caller falls back to the serial
// reader, which is the authority on what is and is not a valid gzip file.
bool inflateIndexed(const uint8_t *p, size_t n, size_t headerLen, const GzipIndex &idx, std::vector<uint8_t> *out) {
  const size_t nb = idx.pieceBytes.size();
  if (nb == 0 || idx.blockBytes == 0) return false;
  if ((idx.totalBytes + idx.blockBytes - 1) / idx.blockBytes != nb) return false;
  std::vector<size_t> off(nb + 1, headerLen);
  for (size_t i = 0; i < nb; ++i) off[i + 1] = off[i] + idx.pieceBytes[i];
  if (off[nb] + 8 != n) return false;  // exactly one member, nothing after it
  if (idx.totalBytes > (n - headerLen) * 1032 + 1024) return false;  // beyond deflate's maximum expansion
  out->clear();
  detail::resizeUninitialized(out, idx.totalBytes);  // every piece is checked to fill its range exactly
  std::vector<uLong> crcs(nb);
  std::atomic<size_t> next{0};
  std::atomic<bool> failed{false};
  auto worker = [&]() {
    for (;;) {
      const size_t b = next.fetch_add(1);
      if (b >= nb || failed.load()) return;
      const size_t uoff = b * static_cast<size_t>(idx.blockBytes);
      const size_t ulen = std::min<size_t>(idx.blockBytes, idx.totalBytes - uoff);
      z_stream zs = {};
      if (inflateInit2(&zs, -MAX_WBITS) != Z_OK) {
        failed = true;
        return;
      }
      zs.next_in = const_cast<Bytef *>(p + off[b]);
      zs.avail_in = idx.pieceBytes[b];
      zs.next_out = out->data() + uoff;
      zs.avail_out = static_cast<uInt>(ulen);
      int rc = inflate(&zs, Z_SYNC_FLUSH);
      if (rc == Z_OK && zs.avail_in > 0) rc = inflate(&zs, Z_SYNC_FLUSH);  // the empty stored block after a full buffer
      const bool last = (b + 1 == nb);
      const bool ok = zs.total_out == ulen && zs.avail_in == 0 && (last ? rc == Z_STREAM_END : (rc == Z_OK || rc == Z_BUF_ERROR));
      inflateEnd(&zs);
      if (!ok) {
        failed = true;
        return;
      }
      crcs[b] = crc32(crc32(0L, Z_NULL, 0), out->data() + uoff, static_cast<uInt>(ulen));
    }
  };
  std::vector<std::thread> pool;
  const int nt = gunzipThreads(nb);
  for (int t = 1; t < nt; ++t) pool.emplace_back(worker);
  worker();
  for (auto &t : pool) t.join();
  if (failed) return false;
  uLong crc = crc32(0L, Z_NULL, 0);
  for (size_t b = 0; b < nb; ++b) {
    const size_t ulen = std::min<size_t>(idx.blockBytes, idx.totalBytes - b * static_cast<size_t>(idx.blockBytes));
    crc = crc32_combine(crc, crcs[b], static_cast<z_off_t>(ulen));
  }
  return getLe(p + n - 8, 4) == static_cast<uint32_t>(crc) && getLe(p + n - 4, 4) == (idx.totalBytes & 0xffffffffu);
}

// libdeflate (a whole-buffer inflater, about twice zlib's speed) is used when the system has it; it is
// looked up at run time so that nothing depends on it being there.  SPZ_AMD_NO_LIBDEFLATE=1 disables it.
struct LibDeflate {
  void *(*alloc)() = nullptr;
  int (*gunzip)(void *, const void *, size_t, void *, size_t, size_t *) = nullptr;
  void (*release)(void *) = nullptr;
  LibDeflate() {
    const char *e = std::getenv("SPZ_AMD_NO_LIBDEFLATE");
    if (e && std::atoi(e) != 0) return;
    void *h = dlopen("libdeflate.so.0", RTLD_NOW | RTLD_LOCAL);
    if (!h) return;
    alloc = reinterpret_cast<void *(*)()>(dlsym(h, "libdeflate_alloc_decompressor"));
    gunzip = reinterpret_cast<int (*)(void *, const void *, size_t, void *, size_t, size_t *)>(
        dlsym(h, "libdeflate_gzip_decompress"));
    release = reinterpret_cast<void (*)(void *)>(dlsym(h, "libdeflate_free_decompressor"));
    if (!alloc || !gunzip || !release) alloc = nullptr;
  }
  bool usable() const { return alloc != nullptr; }
};

bool inflateWholeBuffer(const uint8_t *p, size_t n, std::vector<uint8_t> *out) {
  static const LibDeflate lib;
  if (!lib.usable()) return false;
  const uint64_t isize = getLe(p + n - 4, 4);  // mod 2^32; a mismatch sends the caller to the serial reader
  if (isize == 0 || isize > n * 1032 + 1024) return false;
  void *d = lib.alloc();
  if (!d) return false;
  out->clear();
  detail::resizeUninitialized(out, isize);  // accepted only when libdeflate wrote all of it (got == isize)
  size_t got = 0;
  const int rc = lib.gunzip(d, p, n, out->data(), out->size(), &got);
  lib.release(d);
  return rc == 0 && got == isize;
}

}  // namespace

bool compressGzippedParallel(const uint8_t *data, size_t size, std::vector<uint8_t> *out, int threads) {
  if (threads <= 1 || size < (1u << 20)) return compressGzipped(data, size, out);
  size_t blockBytes = size_t(1) << 20;  // 1 MiB of input per deflate job
  while ((size + blockBytes - 1) / blockBytes > 16000) blockBytes <<= 1;  // the index must fit FEXTRA's 64 KiB
  const size_t kBlock = blockBytes;
  const size_t nblocks = (size + kBlock - 1) / kBlock;
  std::vector<std::vector<uint8_t>> pieces(nblocks);
  std::vector<uLong> crcs(nblocks);
  std::atomic<size_t> next{0};
  std::atomic<bool> failed{false};
  auto worker = [&]() {
    std::vector<uint8_t> buf;
    for (;;) {
      const size_t b = next.fetch_add(1);
      if (b >= nblocks || failed.load()) return;
      const size_t off = b * kBlock, len = std::min(kBlock, size - off);
      z_stream zs = {};
      if (deflateInit2(&zs, Z_DEFAULT_COMPRESSION, Z_DEFLATED, -MAX_WBITS, 9, Z_DEFAULT_STRATEGY) != Z_OK) {
        failed = true;
        return;
      }
      buf.resize(deflateBound(&zs, static_cast<uLong>(len)) + 16);
      zs.next_in = const_cast<Bytef *>(data + off);
      zs.avail_in = static_cast<uInt>(len);
      zs.next_out = buf.data();
      zs.avail_out = static_cast<uInt>(buf.size());
      const bool last = (b + 1 == nblocks);
      const int rc = deflate(&zs, last ? Z_FINISH : Z_SYNC_FLUSH);
      const bool ok = last ? (rc == Z_STREAM_END) : (rc == Z_OK && zs.avail_in == 0 && zs.avail_out > 0);
      if (!ok) failed = true;
      pieces[b].assign(buf.data(), buf.data() + (buf.size() - zs.avail_out));
      deflateEnd(&zs);
      crcs[b] = crc32(crc32(0L, Z_NULL, 0), data + off, static_cast<uInt>(len));
    }
  };
  std::vector<std::thread> pool;
  const int nt = static_cast<int>(std::min<size_t>(static_cast<size_t>(threads), nblocks));
  for (int t = 0; t < nt; ++t) pool.emplace_back(worker);
  for (auto &t : pool) t.join();
  if (failed) return false;
  const size_t indexBytes = 20 + 4 * nblocks;
  size_t total = 10 + 2 + 4 + indexBytes + 8;
  for (const auto &p : pieces) total += p.size();
  out->clear();
  out->reserve(total);
  // zlib's own 10-byte header (magic, deflate, mtime 0, xfl 0, OS 3 = Unix) with FLG.FEXTRA set
  const uint8_t header[10] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0x00, 0x03};
  out->insert(out->end(), header, header + 10);
  putLe(out, 4 + indexBytes, 2);  // XLEN
  out->push_back(kIndexId1);
  out->push_back(kIndexId2);
  putLe(out, indexBytes, 2);
  putLe(out, kIndexVersion, 4);
  putLe(out, kBlock, 4);
  putLe(out, size, 8);
  putLe(out, nblocks, 4);
  for (const auto &p : pieces) putLe(out, p.size(), 4);
  uLong crc = crc32(0L, Z_NULL, 0);
  for (size_t b = 0; b < nblocks; ++b) {
    out->insert(out->end(), pieces[b].begin(), pieces[b].end());
    crc = crc32_combine(crc, crcs[b], static_cast<z_off_t>(std::min(kBlock, size - b * kBlock)));
  }
  putLe(out, static_cast<uint32_t>(crc), 4);
  putLe(out, size & 0xffffffffu, 4);
  return true;
}

// gunzip (load-spz.cc:141-182).  Three readers with one result: members written by
// compressGzippedParallel are inflated piece-parallel through their index; anything else goes through
// libdeflate when the system has it; and the zlib loop the reference uses is the fallback for every
// case the fast readers decline or fail on, so acceptance and rejection are exactly zlib's.
namespace {
// The device reader (spz_inflate_dev.hip): SPZ_AMD_GUNZIP_DEVICE = 0 never, 1 for members of 1 MiB and more, unset:
// of 8 MiB and more on hosts with fewer than 32 usable CPUs.  The result is believed only when its length matches ISIZE and its CRC-32 the trailer's.
std::atomic<uint64_t> g_device_inflates{0};

thread_local const char *g_inflate_decline = "";  // deviceInflateLastDecline()

// CRC-32 (the reflected polynomial 0xedb88320) as polynomial arithmetic: a * b mod P, and x^(8 n) mod P (bit 31 = x^0).
uint32_t crcMultModP(uint32_t a, uint32_t b) {
  uint32_t m = 1u << 31, p = 0u;
  for (;;) {
    if (a & m) {
      p ^= b;
      if ((a & (m - 1u)) == 0u) break;
    }
    m >>= 1;
    b = (b & 1u) ? (b >> 1) ^ 0xedb88320u : b >> 1;
  }
  return p;
}
uint32_t crcShiftFactor(uint64_t nbytes) {  // x^(8 nbytes) mod P
  uint32_t sq = 1u << 30, f = 1u << 31;     // x^1, x^0
  for (uint64_t n = nbytes << 3; n != 0; n >>= 1) {
    if (n & 1u) f = crcMultModP(sq, f);
    sq = crcMultModP(sq, sq);
  }
  return f;
}

// Is a member of this size one the device reader will be asked about (SPZ_AMD_GUNZIP_DEVICE, size, core count)?
bool deviceInflateWanted(size_t size, size_t header_len) {
  const char *e = std::getenv("SPZ_AMD_GUNZIP_DEVICE");
  if (e && e[0] == '0') return false;
  const bool forced = e && e[0] == '1';
  if (size < header_len + 8 + (size_t(1) << 20)) return false;
  if (!forced) {
    // profiles/r03_load_sweep.txt (16 usable CPUs; file MB: device / host ms): 10: 26 / 15, 20: 32 / 21, 41: 25 / 41,
    // 82: 37 / 71, 163: 80 / 165, 409: 99 / 353.  The device reader costs ~20 ms whatever the size (a wave takes that
    // long for one of zlib's blocks) and 0.2 ms per MB; the parallel host reader 13.9 ms per MB and core, if it scales
    // (it does to 16).  The faster of the two by that account: from ~30 MB with 16 cores, ~85 MB with 32.
    const double mb = static_cast<double>(size) / 1e6, cores = static_cast<double>(std::max(1u, detail::effectiveCpuCount()));
    if (20.0 + 0.2 * mb >= 13.9 * mb / cores) return false;
  }
  return spz_amd_device_count() > 0;
}

// The first `want` bytes a raw deflate stream inflates to (zlib); returns how many it got.
size_t inflatePrefix(const uint8_t *deflate, size_t n, uint8_t *out, size_t want) {
  z_stream zs = {};
  if (inflateInit2(&zs, -MAX_WBITS) != Z_OK) return 0;
  zs.next_in = const_cast<Bytef *>(deflate);
  zs.avail_in = static_cast<uInt>(std::min<size_t>(n, size_t(1) << 16));
  zs.next_out = out;
  zs.avail_out = static_cast<uInt>(want);
  (void)inflate(&zs, Z_SYNC_FLUSH);
  const size_t got = want - zs.avail_out;
  inflateEnd(&zs);
  return got;
}

// Inflates the member on the device and checks length and CRC-32 against its trailer; nullptr: declined or wrong.
void *openVerifiedDeviceInflate(const uint8_t *gz, size_t size, size_t header_len, uint64_t *out_bytes,
                                void (*after_upload)(void *) = nullptr, void *after_arg = nullptr) {
  if (!deviceInflateWanted(size, header_len)) return nullptr;
  const size_t nbytes = size - header_len - 8;
  auto le32 = [&](const uint8_t *q) {
    return static_cast<uint32_t>(q[0]) | (static_cast<uint32_t>(q[1]) << 8) | (static_cast<uint32_t>(q[2]) << 16) |
           (static_cast<uint32_t>(q[3]) << 24);
  };
  const uint32_t want_crc = le32(gz + size - 8), isize = le32(gz + size - 4);
  void *ctx = nullptr;
  g_inflate_decline = "";
  const int open_rc = spz_amd_inflate_open_ex(gz + header_len, nbytes, deviceIndex(), &ctx, out_bytes, after_upload, after_arg);
  if (open_rc != SPZ_AMD_OK) {
    g_inflate_decline = open_rc == SPZ_AMD_ERR_UNSUPPORTED ? spz_amd_inflate_last_decline() : spz_amd_status_string(open_rc);
    return nullptr;
  }
  bool ok = static_cast<uint32_t>(*out_bytes & 0xffffffffull) == isize;
  if (ok) {
    const uint32_t piece = spz_amd_inflate_crc_piece_bytes();
    std::vector<uint32_t> crcs(static_cast<size_t>((*out_bytes + piece - 1) / piece));
    uint32_t n_pieces = 0;
    ok = spz_amd_inflate_piece_crcs(ctx, crcs.data(), static_cast<uint32_t>(crcs.size()), &n_pieces) == SPZ_AMD_OK &&
         n_pieces == crcs.size();
    if (ok) {
      // crc(A || B) = crc(A) * x^(8 |B|) mod P  xor  crc(B).  zlib 1.2.11's crc32_combine rebuilds that operator (a
      // 32 x 32 matrix, squared log |B| times) on every call: 2 480 calls for a 650 MB stream were several
      // milliseconds of a loadSpz; every piece but the last has the same length, so the factor is computed twice.
      uint32_t crc = crcs.empty() ? 0u : crcs[0];
      const uint32_t full = crcShiftFactor(piece);
      for (size_t i = 1; i < crcs.size(); ++i) {
        const uint64_t len = std::min<uint64_t>(piece, *out_bytes - static_cast<uint64_t>(i) * piece);
        crc = crcMultModP(len == piece ? full : crcShiftFactor(len), crc) ^ crcs[i];
      }
      ok = crc == want_crc;
    }
  }
  if (!ok) {
    g_inflate_decline = "crc";
    spz_amd_inflate_close(ctx);
    return nullptr;
  }
  return ctx;
}

bool inflateOnDevice(const uint8_t *gz, size_t size, size_t header_len, std::vector<uint8_t> *out) {
  uint64_t out_bytes = 0;
  void *ctx = openVerifiedDeviceInflate(gz, size, header_len, &out_bytes);
  if (ctx == nullptr) return false;
  struct Close {
    void *c;
    ~Close() { spz_amd_inflate_close(c); }
  } closer{ctx};
  out->clear();
  detail::resizeUninitialized(out, static_cast<size_t>(out_bytes));
  {
    detail::Prefault pf;
    pf.add(out->data(), out->size());
    pf.start();
    pf.join();
  }
  if (spz_amd_inflate_fetch(ctx, out->data()) != SPZ_AMD_OK) return false;
  g_device_inflates.fetch_add(1);
  return true;
}

}  // namespace

uint64_t deviceInflateCount() { return g_device_inflates.load(); }
const char *deviceInflateLastDecline() { return g_inflate_decline; }

namespace {
bool decompressGzippedWith(const uint8_t *compressed, size_t size, std::vector<uint8_t> *out, bool try_device);
}  // namespace

bool decompressGzipped(const uint8_t *compressed, size_t size, std::vector<uint8_t> *out) {
  return decompressGzippedWith(compressed, size, out, true);
}

namespace {
bool decompressGzippedWith(const uint8_t *compressed, size_t size, std::vector<uint8_t> *out, bool try_device) {
  if (compressed != nullptr) {
    GzipIndex idx;
    const size_t headerLen = parseGzipHeader(compressed, size, &idx);
    if (headerLen != 0) {
      if (!idx.pieceBytes.empty() && inflateIndexed(compressed, size, headerLen, idx, out)) return true;
      // an ordinary single deflate stream (what the reference writes): on the device when it is large and one answers
      if (try_device && inflateOnDevice(compressed, size, headerLen, out)) return true;
      // ... or decoded in parallel on the host
      if (size >= (size_t(4) << 20)) {
        const int threads = gunzipThreads(size_t(1) << 20);
        // two decoding passes with a plain decoder: pays off from about 8 threads (measured), see spz_inflate.cpp
        if (threads >= 8 && pinflate::inflate(compressed, size, headerLen, threads, out)) return true;
      }
      if (inflateWholeBuffer(compressed, size, out)) return true;
    }
  }
  z_stream stream = {};
  // 16 | MAX_WBITS: gzip wrapper only (load-spz.cc:172).
  if (inflateInit2(&stream, 16 | MAX_WBITS) != Z_OK) return false;
  out->clear();
  std::vector<uint8_t> buffer(1u << 20);
  const uint8_t *next = compressed;
  size_t left = size;
  bool success = false;
  int res = Z_OK;
  while (res != Z_STREAM_END) {
    if (stream.avail_in == 0) {
      const size_t chunk = std::min<size_t>(left, size_t(1) << 30);
      stream.next_in = const_cast<Bytef *>(next);
      stream.avail_in = static_cast<uInt>(chunk);
      next += chunk;
      left -= chunk;
    }
    stream.next_out = buffer.data();
    stream.avail_out = static_cast<uInt>(buffer.size());
    res = inflate(&stream, Z_NO_FLUSH);
    if (res != Z_OK && res != Z_STREAM_END) break;  // incl. Z_BUF_ERROR on truncated input
    out->insert(out->end(), buffer.data(), buffer.data() + (buffer.size() - stream.avail_out));
    if (res == Z_STREAM_END) success = true;
  }
  inflateEnd(&stream);
  return success;
}
}  // namespace

// ---- (de)serialise, load-spz.cc:533-596 ----------------------------------------------------------
void serializePackedGaussians(const PackedGaussians &packed, std::ostream *out) {
  spz_amd_header h = {};
  h.version = 3;  // the reference writer never sets another version (load-spz.cc:133,534-539)
  h.num_points = static_cast<uint32_t>(packed.numPoints);
  h.sh_degree = static_cast<uint8_t>(packed.shDegree);
  h.fractional_bits = static_cast<uint8_t>(packed.fractionalBits);
  h.flags = static_cast<uint8_t>(packed.antialiased ? 1 : 0);
  uint8_t raw[16];
  spz_amd_write_header(&h, raw);
  out->write(reinterpret_cast<const char *>(raw), 16);
  auto put = [&](const std::vector<uint8_t> &v) {
    out->write(reinterpret_cast<const char *>(v.data()), static_cast<std::streamsize>(v.size()));
  };
  put(packed.positions);
  put(packed.alphas);
  put(packed.colors);
  put(packed.scales);
  put(packed.rotations);
  put(packed.sh);
}

namespace {

PackedGaussians slicePacked(const uint8_t *stream, const spz_amd_header &hdr) {
  spz_amd_layout lay;
  spz_amd_stream_layout(hdr.num_points, hdr.sh_degree, static_cast<int>(hdr.version), &lay);
  PackedGaussians r;
  r.numPoints = static_cast<int32_t>(hdr.num_points);
  r.shDegree = hdr.sh_degree;
  r.fractionalBits = hdr.fractional_bits;
  r.antialiased = (hdr.flags & 1) != 0;
  r.usesQuaternionSmallestThree = hdr.version >= 3;
  auto take = [&](int s) {
    return std::vector<uint8_t>(stream + lay.offset[s], stream + lay.offset[s] + lay.bytes[s]);
  };
  r.positions = take(SPZ_AMD_SEC_POSITIONS);
  r.alphas = take(SPZ_AMD_SEC_ALPHAS);
  r.colors = take(SPZ_AMD_SEC_COLORS);
  r.scales = take(SPZ_AMD_SEC_SCALES);
  r.rotations = take(SPZ_AMD_SEC_ROTATIONS);
  r.sh = take(SPZ_AMD_SEC_SH);
  return r;
}

}  // namespace

PackedGaussians deserializePackedGaussians(std::istream &in) {
  std::vector<uint8_t> data((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
  spz_amd_header hdr;
  if (!peekHeaderLogged(data.data(), data.size(), &hdr)) return {};
  return slicePacked(data.data(), hdr);
}

// ---- pack / unpack -------------------------------------------------------------------------------
namespace {
// Sizes the six arrays of a cloud that a device copy is about to fill completely.
void sizeCloudArrays(GaussianCloud *r, size_t n, size_t shDim, detail::Prefault *prefault) {
  std::vector<float> *arrays[6] = {&r->positions, &r->scales, &r->rotations, &r->alphas, &r->colors, &r->sh};
  const size_t counts[6] = {n * 3, n * 3, n * 4, n, n * 3, n * shDim * 3};
  for (int i = 0; i < 6; ++i) {
    detail::resizeUninitialized(arrays[i], counts[i]);
    prefault->add(arrays[i]->data(), counts[i] * sizeof(float));
  }
}
}  // namespace

namespace {
bool packToStreamKeep(const GaussianCloud &g, const PackOptions &o, std::vector<uint8_t> *stream, const uint8_t **d_copy,
                      SaveAhead *ahead = nullptr);
}
bool packToStream(const GaussianCloud &g, const PackOptions &o, std::vector<uint8_t> *stream) {
  return packToStreamKeep(g, o, stream, nullptr);
}
namespace {
// d_copy != null: *d_copy receives the device's copy of the stream (or null), to be given back with spz_amd_kept_stream_release
bool packToStreamKeep(const GaussianCloud &g, const PackOptions &o, std::vector<uint8_t> *stream, const uint8_t **d_copy,
                      SaveAhead *ahead) {
  if (d_copy) *d_copy = nullptr;
  g_last_status = SPZ_AMD_OK;
  if (!checkSizes(g)) {
    // packGaussians returns an empty PackedGaussians{} (load-spz.cc:258-260) and saveSpz goes on
    // to write it: a 0-point stream whose header carries the defaults (fractionalBits 0).
    spz_amd_header h = {};
    h.version = 3;
    stream->assign(16, 0);
    spz_amd_write_header(&h, stream->data());
    return true;
  }
  spz_amd_layout lay;
  if (spz_amd_stream_layout(static_cast<uint64_t>(g.numPoints), g.shDegree, 3, &lay) != SPZ_AMD_OK) return false;
  // every byte of the stream is written by the device copy: no zero fill, pages mapped in the background
  stream->clear();
  detail::resizeUninitialized(stream, lay.total_bytes);
  detail::Prefault prefault;
  prefault.add(stream->data(), stream->size());
  prefault.start();
  spz_amd_cloud_in in = {g.positions.data(), g.scales.data(), g.rotations.data(),
                         g.alphas.data(),    g.colors.data(), g.sh.empty() ? nullptr : g.sh.data()};
  void *zlib_session = ahead ? ahead->session : nullptr;
  auto tail_ready = [](void *p) {
    SaveAhead *a = static_cast<SaveAhead *>(p);
    try {
      a->tail = exactgz::tailAheadStart(a->stream, a->size);
    } catch (...) {  // on the C library's download thread: the writer then runs its tail job itself
      a->tail = nullptr;
    }
    if (std::getenv("SPZ_AMD_EXACT_GZIP_TIMING")) {
      std::fprintf(stderr, "[saveSpz] the stream's end is on the host %.4f s into the pack\n",
                   std::chrono::duration<double>(std::chrono::steady_clock::now() - a->t0).count());
    }
  };
  if (ahead) {
    ahead->stream = stream->data();
    ahead->size = stream->size();
    ahead->t0 = std::chrono::steady_clock::now();
  }
  const size_t tail_bytes = zlib_session ? exactgz::tailAheadBytes(stream->size()) : 0;
  const int rc = d_copy ? spz_amd_encode_host_keep_session_tail(&in, static_cast<uint64_t>(g.numPoints), g.shDegree, g.antialiased ? 1 : 0,
                                                                static_cast<int>(o.from), 3, stream->data(), stream->size(), deviceIndex(),
                                                                d_copy, zlib_session, tail_bytes, tail_bytes ? +tail_ready : nullptr, ahead)
                        : spz_amd_encode_host(&in, static_cast<uint64_t>(g.numPoints), g.shDegree, g.antialiased ? 1 : 0,
                                              static_cast<int>(o.from), 3, stream->data(), stream->size(), deviceIndex());
  return !deviceFailed(rc, "encode");
}
}  // namespace

GaussianCloud unpackFromStream(const uint8_t *stream, size_t size, const UnpackOptions &o) {
  g_last_status = SPZ_AMD_OK;
  spz_amd_header hdr;
  if (!peekHeaderLogged(stream, size, &hdr)) return {};
  GaussianCloud r;
  r.numPoints = static_cast<int32_t>(hdr.num_points);
  r.shDegree = hdr.sh_degree;
  r.antialiased = (hdr.flags & 1) != 0;
  const size_t n = hdr.num_points;
  detail::Prefault prefault;
  sizeCloudArrays(&r, n, static_cast<size_t>(dimForDegree(hdr.sh_degree)), &prefault);
  prefault.start();
  spz_amd_cloud_out out = {r.positions.data(), r.scales.data(), r.rotations.data(),
                           r.alphas.data(),    r.colors.data(), r.sh.empty() ? nullptr : r.sh.data()};
  const int rc = spz_amd_decode_host(stream, size, static_cast<int>(o.to), &out, deviceIndex());
  prefault.join();
  if (deviceFailed(rc, "decode")) return {};
  return r;
}

PackedGaussians packGaussians(const GaussianCloud &g, const PackOptions &o) {
  if (!checkSizes(g)) return {};
  std::vector<uint8_t> stream;
  if (!packToStream(g, o, &stream)) return {};
  spz_amd_header hdr;
  if (spz_amd_peek_header_ex(stream.data(), stream.size(), 0, &hdr) != SPZ_AMD_OK) return {};
  return slicePacked(stream.data(), hdr);
}

GaussianCloud unpackGaussians(const PackedGaussians &packed, const UnpackOptions &o) {
  g_last_status = SPZ_AMD_OK;
  const int32_t shDim = dimForDegree(packed.shDegree);
  const bool f16 = packed.usesFloat16();
  if (!checkSizes(packed, packed.numPoints, shDim, f16)) return {};
  // Re-assemble the stream (host memcpy) so that one fused decode launch handles it.
  spz_amd_header h = {};
  h.version = f16 ? 1u : (packed.usesQuaternionSmallestThree ? 3u : 2u);
  if (packed.numPoints == 0) h.version = packed.usesQuaternionSmallestThree ? 3u : 2u;
  h.num_points = static_cast<uint32_t>(packed.numPoints);
  h.sh_degree = static_cast<uint8_t>(packed.shDegree);
  h.fractional_bits = static_cast<uint8_t>(packed.fractionalBits);
  h.flags = packed.antialiased ? 1 : 0;
  std::vector<uint8_t> stream(16);
  spz_amd_write_header(&h, stream.data());
  stream.reserve(16 + packed.positions.size() + packed.alphas.size() + packed.colors.size() + packed.scales.size() +
                 packed.rotations.size() + packed.sh.size());
  for (const auto *v : {&packed.positions, &packed.alphas, &packed.colors, &packed.scales, &packed.rotations,
                        &packed.sh}) {
    stream.insert(stream.end(), v->begin(), v->end());
  }
  spz_amd_header hdr;
  const int prc = spz_amd_peek_header_ex(stream.data(), stream.size(), 0, &hdr);
  if (prc != SPZ_AMD_OK) {
    deviceFailed(prc, "unpackGaussians");
    return {};
  }
  GaussianCloud r;
  r.numPoints = packed.numPoints;
  r.shDegree = packed.shDegree;
  r.antialiased = packed.antialiased;
  const size_t n = static_cast<size_t>(packed.numPoints);
  if (n == 0) return r;
  detail::Prefault prefault;
  sizeCloudArrays(&r, n, static_cast<size_t>(shDim), &prefault);
  prefault.start();
  spz_amd_cloud_out out = {r.positions.data(), r.scales.data(), r.rotations.data(),
                           r.alphas.data(),    r.colors.data(), r.sh.empty() ? nullptr : r.sh.data()};
  // no point limit here: the reference's 10 M cap lives in deserializePackedGaussians (load-spz.cc:549,561),
  // unpackGaussians (:467-531) has none
  const int rc = spz_amd_decode_host_ex(stream.data(), stream.size(), 0, static_cast<int>(o.to), &out, deviceIndex());
  prefault.join();
  if (deviceFailed(rc, "decode")) return {};
  return r;
}

GaussianCloud unpackIndices(const PackedGaussians &packed, const std::vector<uint32_t> &indices,
                            const UnpackOptions &o) {
  g_last_status = SPZ_AMD_OK;
  const int32_t shDim = dimForDegree(packed.shDegree);
  const bool f16 = packed.usesFloat16();
  if (!checkSizes(packed, packed.numPoints, shDim, f16)) return {};
  GaussianCloud r;
  r.shDegree = packed.shDegree;
  r.antialiased = packed.antialiased;
  if (indices.empty()) return r;
  if (packed.numPoints == 0) {
    logLine("[SPZ ERROR] spz_amd: unpackIndices: the packed cloud is empty");
    return {};
  }
  spz_amd_header h = {};
  h.version = f16 ? 1u : (packed.usesQuaternionSmallestThree ? 3u : 2u);
  h.num_points = static_cast<uint32_t>(packed.numPoints);
  h.sh_degree = static_cast<uint8_t>(packed.shDegree);
  h.fractional_bits = static_cast<uint8_t>(packed.fractionalBits);
  h.flags = packed.antialiased ? 1 : 0;
  std::vector<uint8_t> stream(16);
  spz_amd_write_header(&h, stream.data());
  for (const auto *v : {&packed.positions, &packed.alphas, &packed.colors, &packed.scales, &packed.rotations,
                        &packed.sh}) {
    stream.insert(stream.end(), v->begin(), v->end());
  }
  const size_t n = indices.size();
  r.numPoints = static_cast<int32_t>(n);
  r.positions.resize(n * 3);
  r.scales.resize(n * 3);
  r.rotations.resize(n * 4);
  r.alphas.resize(n);
  r.colors.resize(n * 3);
  r.sh.resize(n * shDim * 3);
  spz_amd_cloud_out out = {r.positions.data(), r.scales.data(), r.rotations.data(),
                           r.alphas.data(),    r.colors.data(), r.sh.empty() ? nullptr : r.sh.data()};
  const int rc = spz_amd_decode_gather_host(stream.data(), stream.size(), 0, indices.data(), n, static_cast<int>(o.to),
                                            &out, deviceIndex());
  if (deviceFailed(rc, "unpackIndices")) return {};
  return r;
}

// ---- saveSpz / loadSpz overloads, load-spz.cc:598-668 ---------------------------------------------
namespace {
std::mutex g_stream_cache_mutex;
std::vector<uint8_t> g_stream_cache;
}  // namespace

bool saveSpz(const GaussianCloud &g, const PackOptions &o, std::vector<uint8_t> *out) {
  static const bool timing = std::getenv("SPZ_AMD_EXACT_GZIP_TIMING") != nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  struct Report {
    std::chrono::steady_clock::time_point t0;
    bool on;
    ~Report() {
      if (on) std::fprintf(stderr, "[saveSpz] %.3f s in all (stream freed)\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
  } report{t0, timing};
  // The stream is a transient of this call, 65 bytes per Gaussian.  Giving such a buffer back costs ~80 ms per GB once
  // device copies have pinned it (measured: 52 ms of a 0.36 s save), in the foreground or — contending with
  // whatever the caller does next — in the background; so one buffer of up to 1 GiB is kept for the next save
  // (spz::releaseHostMemory() drops it).  A second save at the same time uses a buffer of its own.
  std::vector<uint8_t> local;
  static const bool keep = [] {
    const char *e = std::getenv("SPZ_AMD_KEEP_STREAM_BUFFER");
    return !(e && e[0] == '0');
  }();
  std::unique_lock<std::mutex> cache_lock(g_stream_cache_mutex, std::defer_lock);
  if (keep) (void)cache_lock.try_lock();
  std::vector<uint8_t> &stream = cache_lock.owns_lock() ? g_stream_cache : local;
  struct Trim {
    std::vector<uint8_t> &v;
    bool cached;
    ~Trim() {
      if (cached && v.capacity() > (size_t(1) << 30)) std::vector<uint8_t>().swap(v);
    }
  } trim{stream, cache_lock.owns_lock()};
  // the stream stays on the device as well when its container stage is going to run there: no second upload
  const uint8_t *d_copy = nullptr;
  struct Kept {
    const uint8_t **p;
    ~Kept() { spz_amd_kept_stream_release(deviceIndex(), *p); }
  } kept{&d_copy};
  spz_amd_layout lay;
  const bool keep_on_device = g.numPoints > 0 && spz_amd_stream_layout(static_cast<uint64_t>(g.numPoints), g.shDegree, 3, &lay) == SPZ_AMD_OK &&
                              lay.total_bytes >= (size_t(1) << 20) && exactGzipThreads() >= 1 && deviceParseWanted(lay.total_bytes);
  // Default: the reference's single deflate stream (byte-identical files).  SPZ_AMD_GZIP_THREADS=n>1
  // opts into the parallel container (same content, different bytes, n x faster).
  const char *e = std::getenv("SPZ_AMD_GZIP_THREADS");
  const int threads = e ? std::atoi(e) : 1;
  // ... and its first stages (hash chains, match tables: a pure function of the stream's bytes) run on the finished
  // sections while the rest of the floats still upload: SPZ_AMD_GZIP_OVERLAP=0 starts them after the pack, as before
  SaveAhead ahead;
  static const bool overlap = [] {
    const char *v = std::getenv("SPZ_AMD_GZIP_OVERLAP");
    return !(v && v[0] == '0');
  }();
  if (keep_on_device && overlap && threads <= 1 && std::strcmp(zlibVersion(), "1.2.11") == 0) {
    const size_t avail = availablePhysicalBytes();
    if ((avail == 0 || lay.total_bytes / 2 * 9 < avail) &&
        spz_amd_zlib_session_open(lay.total_bytes, deviceIndex(), &ahead.session) != SPZ_AMD_OK) {
      ahead.session = nullptr;  // declined (size, memory): the stage starts after the pack, or runs on the host
    }
  }
  if (!packToStreamKeep(g, o, &stream, keep_on_device ? &d_copy : nullptr, &ahead)) return false;
  if (timing) std::fprintf(stderr, "[saveSpz] pack %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  if (threads <= 1) return compressGzippedWithCopy(stream.data(), stream.size(), out, d_copy, &ahead);
  return compressGzippedParallel(stream.data(), stream.size(), out, threads);
}

void releaseHostMemory() {
  std::lock_guard<std::mutex> lock(g_stream_cache_mutex);
  std::vector<uint8_t>().swap(g_stream_cache);
}

bool saveSpz(const GaussianCloud &g, const PackOptions &o, const std::string &filename) {
  std::vector<uint8_t> data;
  if (!saveSpz(g, o, &data)) return false;
  // The file is opened only after encoding succeeded; result is out.good() (load-spz.cc:647-650).
  return writeFile(filename, data);
}

PackedGaussians loadSpzPacked(const uint8_t *data, int32_t size) {
  std::vector<uint8_t> stream;
  if (!decompressGzipped(data, static_cast<size_t>(size), &stream)) return {};
  spz_amd_header hdr;
  if (!peekHeaderLogged(stream.data(), stream.size(), &hdr)) return {};
  return slicePacked(stream.data(), hdr);
}

PackedGaussians loadSpzPacked(const std::vector<uint8_t> &data) {
  return loadSpzPacked(data.data(), static_cast<int>(data.size()));
}

PackedGaussians loadSpzPacked(const std::string &filename) {
  std::vector<uint8_t> data;
  if (!readFile(filename, &data, /*log=*/false)) return {};
  return loadSpzPacked(data);
}

// ---- device-resident packed load -----------------------------------------------------------------------------
DevicePackedGaussians::DevicePackedGaussians(DevicePackedGaussians &&o) noexcept { *this = std::move(o); }

DevicePackedGaussians &DevicePackedGaussians::operator=(DevicePackedGaussians &&o) noexcept {
  if (this == &o) return *this;
  release();
  numPoints = o.numPoints;
  shDegree = o.shDegree;
  fractionalBits = o.fractionalBits;
  antialiased = o.antialiased;
  usesQuaternionSmallestThree = o.usesQuaternionSmallestThree;
  version = o.version;
  positions = o.positions; alphas = o.alphas; colors = o.colors; scales = o.scales; rotations = o.rotations; sh = o.sh;
  positionsBytes = o.positionsBytes; alphasBytes = o.alphasBytes; colorsBytes = o.colorsBytes;
  scalesBytes = o.scalesBytes; rotationsBytes = o.rotationsBytes; shBytes = o.shBytes;
  stream = o.stream;
  streamBytes = o.streamBytes;
  device = o.device;
  inflatedOnDevice = o.inflatedOnDevice;
  owner_ = o.owner_;
  o.owner_ = nullptr;
  o.release();
  return *this;
}

DevicePackedGaussians::~DevicePackedGaussians() { release(); }

void DevicePackedGaussians::release() {
  if (owner_ != nullptr) spz_amd_inflate_close(owner_);
  owner_ = nullptr;
  numPoints = shDegree = fractionalBits = 0;
  antialiased = false;
  usesQuaternionSmallestThree = true;
  version = 0;
  positions = alphas = colors = scales = rotations = sh = stream = nullptr;
  positionsBytes = alphasBytes = colorsBytes = scalesBytes = rotationsBytes = shBytes = streamBytes = 0;
  inflatedOnDevice = false;
}

namespace {
spz_amd_header headerOf(const DevicePackedGaussians &p) {
  spz_amd_header h = {};
  h.version = p.version;
  h.num_points = static_cast<uint32_t>(p.numPoints);
  h.sh_degree = static_cast<uint8_t>(p.shDegree);
  h.fractional_bits = static_cast<uint8_t>(p.fractionalBits);
  h.flags = p.antialiased ? 1 : 0;
  return h;
}
}  // namespace

GaussianCloud DevicePackedGaussians::unpack(const UnpackOptions &o) const {
  g_last_status = SPZ_AMD_OK;
  if (!valid()) return {};
  const spz_amd_header hdr = headerOf(*this);
  GaussianCloud r;
  r.numPoints = numPoints;
  r.shDegree = shDegree;
  r.antialiased = antialiased;
  detail::Prefault prefault;
  sizeCloudArrays(&r, hdr.num_points, static_cast<size_t>(dimForDegree(shDegree)), &prefault);
  prefault.start();
  spz_amd_cloud_out out = {r.positions.data(), r.scales.data(), r.rotations.data(),
                           r.alphas.data(),    r.colors.data(), r.sh.empty() ? nullptr : r.sh.data()};
  const int rc = spz_amd_decode_host_from_device(stream, streamBytes, &hdr, static_cast<int>(o.to), &out, device);
  prefault.join();
  if (deviceFailed(rc, "DevicePackedGaussians::unpack")) return {};
  return r;
}

GaussianCloud DevicePackedGaussians::unpackIndices(const std::vector<uint32_t> &indices, const UnpackOptions &o) const {
  g_last_status = SPZ_AMD_OK;
  if (!valid()) return {};
  GaussianCloud r;
  r.shDegree = shDegree;
  r.antialiased = antialiased;
  if (indices.empty()) return r;
  if (numPoints == 0) {
    logLine("[SPZ ERROR] spz_amd: unpackIndices: the packed cloud is empty");
    return {};
  }
  const spz_amd_header hdr = headerOf(*this);
  const size_t n = indices.size(), shDim = static_cast<size_t>(dimForDegree(shDegree));
  r.numPoints = static_cast<int32_t>(n);
  r.positions.resize(n * 3);
  r.scales.resize(n * 3);
  r.rotations.resize(n * 4);
  r.alphas.resize(n);
  r.colors.resize(n * 3);
  r.sh.resize(n * shDim * 3);
  spz_amd_cloud_out out = {r.positions.data(), r.scales.data(), r.rotations.data(),
                           r.alphas.data(),    r.colors.data(), r.sh.empty() ? nullptr : r.sh.data()};
  const int rc = spz_amd_decode_gather_host_from_device(stream, streamBytes, &hdr, indices.data(), n, static_cast<int>(o.to), &out, device);
  if (deviceFailed(rc, "DevicePackedGaussians::unpackIndices")) return {};
  return r;
}

DevicePackedGaussians loadSpzPackedDevice(const uint8_t *data, int32_t size) {
  g_last_status = SPZ_AMD_OK;
  DevicePackedGaussians r;
  if (data == nullptr || size <= 0) return r;
  GzipIndex idx;
  const size_t headerLen = parseGzipHeader(data, static_cast<size_t>(size), &idx);
  uint64_t stream_bytes = 0;
  void *ctx = (headerLen != 0 && idx.pieceBytes.empty()) ? openVerifiedDeviceInflate(data, static_cast<size_t>(size), headerLen, &stream_bytes)
                                                         : nullptr;
  bool on_device = ctx != nullptr;
  if (ctx == nullptr) {  // the host readers (same bytes), then one upload
    std::vector<uint8_t> stream;
    if (!decompressGzippedWith(data, static_cast<size_t>(size), &stream, false)) return r;  // silently, load-spz.cc:609-612
    spz_amd_header hdr;
    if (!peekHeaderLogged(stream.data(), stream.size(), &hdr)) return r;
    const int rc = spz_amd_stream_to_device(stream.data(), stream.size(), deviceIndex(), &ctx);
    if (deviceFailed(rc, "loadSpzPackedDevice")) return r;
    stream_bytes = stream.size();
  }
  struct Close {
    void *c;
    ~Close() {
      if (c) spz_amd_inflate_close(c);
    }
  } closer{ctx};
  const uint8_t *d_stream = spz_amd_inflate_device_data(ctx);
  uint8_t first16[16] = {};
  spz_amd_header hdr;
  const int prc = stream_bytes >= 16 ? spz_amd_peek_header_device(d_stream, static_cast<size_t>(stream_bytes), 0, &hdr, nullptr) : SPZ_AMD_ERR_HEADER_NOT_FOUND;
  if (prc != SPZ_AMD_OK || spz_amd_write_header(&hdr, first16) != SPZ_AMD_OK) {
    // a stream the device inflated but whose header is not one: the reference's log line from the host-side check
    std::vector<uint8_t> whole;
    detail::resizeUninitialized(&whole, static_cast<size_t>(stream_bytes));
    if (spz_amd_inflate_fetch(ctx, whole.data()) == SPZ_AMD_OK) (void)peekHeaderLogged(whole.data(), whole.size(), &hdr);
    return r;
  }
  if (!peekHeaderLogged(first16, static_cast<size_t>(stream_bytes), &hdr)) return r;  // limits and short streams, with the log lines
  spz_amd_layout lay;
  if (spz_amd_stream_layout(hdr.num_points, hdr.sh_degree, static_cast<int>(hdr.version), &lay) != SPZ_AMD_OK) return r;
  r.numPoints = static_cast<int32_t>(hdr.num_points);
  r.shDegree = hdr.sh_degree;
  r.fractionalBits = hdr.fractional_bits;
  r.antialiased = (hdr.flags & 1) != 0;
  r.version = hdr.version;
  r.usesQuaternionSmallestThree = hdr.version >= 3;
  auto sec = [&](int s) { return lay.bytes[s] ? d_stream + lay.offset[s] : nullptr; };
  r.positions = sec(SPZ_AMD_SEC_POSITIONS);
  r.alphas = sec(SPZ_AMD_SEC_ALPHAS);
  r.colors = sec(SPZ_AMD_SEC_COLORS);
  r.scales = sec(SPZ_AMD_SEC_SCALES);
  r.rotations = sec(SPZ_AMD_SEC_ROTATIONS);
  r.sh = sec(SPZ_AMD_SEC_SH);
  r.positionsBytes = lay.bytes[SPZ_AMD_SEC_POSITIONS];
  r.alphasBytes = lay.bytes[SPZ_AMD_SEC_ALPHAS];
  r.colorsBytes = lay.bytes[SPZ_AMD_SEC_COLORS];
  r.scalesBytes = lay.bytes[SPZ_AMD_SEC_SCALES];
  r.rotationsBytes = lay.bytes[SPZ_AMD_SEC_ROTATIONS];
  r.shBytes = lay.bytes[SPZ_AMD_SEC_SH];
  r.stream = d_stream;
  r.streamBytes = static_cast<size_t>(stream_bytes);
  r.device = deviceIndex();
  r.inflatedOnDevice = on_device;
  r.owner_ = ctx;
  closer.c = nullptr;
  if (on_device) g_device_inflates.fetch_add(1);
  return r;
}

DevicePackedGaussians loadSpzPackedDevice(const std::vector<uint8_t> &data) {
  return loadSpzPackedDevice(data.data(), static_cast<int32_t>(data.size()));
}

DevicePackedGaussians loadSpzPackedDevice(const std::string &filename) {
  std::vector<uint8_t> data;
  if (!readFile(filename, &data, /*log=*/false)) return {};
  return loadSpzPackedDevice(data);
}

GaussianCloud loadSpz(const uint8_t *data, int32_t size, const UnpackOptions &o) {
  g_last_status = SPZ_AMD_OK;
  static const bool timing = std::getenv("SPZ_AMD_EXACT_GZIP_TIMING") != nullptr;
  const auto t_load = std::chrono::steady_clock::now();
  auto lap = [&](const char *what) {
    if (timing) std::fprintf(stderr, "[loadSpz] %-22s %.3f s since the call\n", what, std::chrono::duration<double>(std::chrono::steady_clock::now() - t_load).count());
  };
  // An ordinary member that the device inflates stays there: the decode kernels read the stream where it is and only
  // the floats cross PCIe.
  bool device_declined = false;
  if (data != nullptr && size > 0) {
    GzipIndex idx;
    const size_t headerLen = parseGzipHeader(data, static_cast<size_t>(size), &idx);
    uint64_t stream_bytes = 0;
    // The output arrays can be sized — and their pages mapped, 25-30 ms for a 10 M-point cloud — while the device
    // inflates: the stream's first 16 bytes say how many points are coming, and zlib has them in microseconds.  Only
    // for members the device reader is going to be asked about; what it finds later must agree with this peek.
    GaussianCloud r;
    detail::Prefault prefault;
    spz_amd_header early = {};
    bool sized_early = false;
    if (headerLen != 0 && idx.pieceBytes.empty() && deviceInflateWanted(static_cast<size_t>(size), headerLen)) {
      uint8_t first[16];
      if (inflatePrefix(data + headerLen, static_cast<size_t>(size) - headerLen, first, sizeof(first)) == sizeof(first)) {
        // the header's own fields (spz_amd_peek_header would also want the whole stream behind them); the gzip trailer's
        // ISIZE must be what a stream of that many points takes, or the peek is not believed
        auto u32 = [&](const uint8_t *q) {
          return static_cast<uint32_t>(q[0]) | (static_cast<uint32_t>(q[1]) << 8) | (static_cast<uint32_t>(q[2]) << 16) |
                 (static_cast<uint32_t>(q[3]) << 24);
        };
        early.version = u32(first + 4);
        early.num_points = u32(first + 8);
        early.sh_degree = first[12];
        spz_amd_layout lay;
        if (u32(first) == 0x5053474eu && early.version >= 1 && early.version <= 3 && early.sh_degree <= 3 &&
            early.num_points > 0 && early.num_points <= SPZ_AMD_REFERENCE_MAX_POINTS &&
            spz_amd_stream_layout(early.num_points, early.sh_degree, static_cast<int>(early.version), &lay) == SPZ_AMD_OK &&
            static_cast<uint32_t>(lay.total_bytes & 0xffffffffull) == u32(data + size - 4)) {
          sizeCloudArrays(&r, early.num_points, static_cast<size_t>(dimForDegree(early.sh_degree)), &prefault);
          sized_early = true;  // mapped once the member is on the device: beside the upload the two contend (+80 ms)
        }
      }
      lap("sized from a peek");
    }
    auto map_pages = [](void *p) { static_cast<detail::Prefault *>(p)->startBeside(); };
    void *ctx = (headerLen != 0 && idx.pieceBytes.empty())
                    ? openVerifiedDeviceInflate(data, static_cast<size_t>(size), headerLen, &stream_bytes,
                                                sized_early ? +map_pages : nullptr, &prefault)
                    : nullptr;
    if (ctx != nullptr) {
      lap("inflated on the device");
      struct Close {
        void *c;
        ~Close() { spz_amd_inflate_close(c); }
      } closer{ctx};
      const uint8_t *d_stream = spz_amd_inflate_device_data(ctx);
      uint8_t first16[16] = {};
      spz_amd_header hdr;
      if (stream_bytes >= 16 && spz_amd_peek_header_device(d_stream, static_cast<size_t>(stream_bytes), 0, &hdr, nullptr) == SPZ_AMD_OK &&
          spz_amd_write_header(&hdr, first16) == SPZ_AMD_OK) {
        // the reference's checks and log lines (load-spz.cc:553-568), on the 16 header bytes and the stream's size
        if (!peekHeaderLogged(first16, static_cast<size_t>(stream_bytes), &hdr)) return {};
        r.numPoints = static_cast<int32_t>(hdr.num_points);
        r.shDegree = hdr.sh_degree;
        r.antialiased = (hdr.flags & 1) != 0;
        prefault.join();   // mapped before the downloads begin (beside them the two contend: spz_host_util.hpp)
        lap("pages mapped");
        detail::Prefault late;
        if (!sized_early || early.num_points != hdr.num_points || early.sh_degree != hdr.sh_degree) {
          sizeCloudArrays(&r, hdr.num_points, static_cast<size_t>(dimForDegree(hdr.sh_degree)), &late);
          late.start();
        }
        spz_amd_cloud_out out = {r.positions.data(), r.scales.data(), r.rotations.data(),
                                 r.alphas.data(),    r.colors.data(), r.sh.empty() ? nullptr : r.sh.data()};
        const int rc = spz_amd_decode_host_from_device(d_stream, static_cast<size_t>(stream_bytes), &hdr, static_cast<int>(o.to),
                                                       &out, deviceIndex());
        late.join();
        lap("decoded and downloaded");
        if (rc == SPZ_AMD_OK) {
          g_device_inflates.fetch_add(1);
          return r;
        }
      }
      // anything unusual about the stream (bad header, short stream): the reference's log line and result come from
      // the ordinary decode of the bytes this context already holds — the member is not inflated a second time
      std::vector<uint8_t> inflated;
      detail::resizeUninitialized(&inflated, static_cast<size_t>(stream_bytes));
      if (spz_amd_inflate_fetch(ctx, inflated.data()) == SPZ_AMD_OK) return unpackFromStream(inflated.data(), inflated.size(), o);
      device_declined = true;
    } else if (headerLen != 0 && idx.pieceBytes.empty()) {
      device_declined = true;  // not asked a second time by decompressGzipped
    }
  }
  std::vector<uint8_t> stream;
  // A failed gunzip yields an empty PackedGaussians and hence an empty cloud, silently
  // (load-spz.cc:609-612).
  if (!decompressGzippedWith(data, static_cast<size_t>(size), &stream, !device_declined)) return {};
  return unpackFromStream(stream.data(), stream.size(), o);
}

// ---- the packed operations' shared steps -----------------------------------------------------------------------
// filter, transform, merge, sort, decimate, clean and prune: the input loaded onto the device, spz_amd_<op>_open, the
// input's device memory released, the result fetched and gzipped from its device copy, closed.  Their file-name forms
// read the input, call the buffer form and write its file image.
namespace {
// The "[SPZ ERROR] <who>: ..." line of a refused call, with `status` left for lastDeviceStatus(); false.
bool opRejected(const char *who, int status, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  char msg[256];
  std::vsnprintf(msg, sizeof(msg), fmt, ap);
  va_end(ap);
  logLine("[SPZ ERROR] %s: %s", who, msg);
  g_last_status = status;
  return false;
}

// Stage times on stderr while the environment variable `env` is set: "[<who>] <stage> <x> ms".
class Laps {
 public:
  Laps(const char *who, const char *env) : who_(who), on_(std::getenv(env) != nullptr) {}
  // The time since the last lap (or since construction) as stage `what`.
  void lap(const char *what) {
    const auto now = std::chrono::steady_clock::now();
    stage(what, std::chrono::duration<double, std::milli>(now - t_).count());
    t_ = now;
  }
  // A stage the device timed (an open's h_ms), `note` after the unit.
  void stage(const char *what, double ms, const char *note = "") const {
    if (on_) std::fprintf(stderr, "[%s] %-8s %.3f ms%s\n", who_, what, ms, note);
  }

 private:
  const char *who_;
  bool on_;
  std::chrono::steady_clock::time_point t_ = std::chrono::steady_clock::now();
};

// The input on the device, or false with "<who>: the input is not a readable .spz" where the load logged no reason.
bool loadInput(const char *who, const uint8_t *data, int32_t size, DevicePackedGaussians *d) {
  *d = loadSpzPackedDevice(data, size);
  if (d->valid()) return true;
  if (g_last_status == SPZ_AMD_OK) logLine("[SPZ ERROR] %s: the input is not a readable .spz", who);
  return false;
}

// The ctx of an operation's spz_amd_<op>_open with the operation's fetch, device_data and close; closed when this goes.
class OpenResult {
 public:
  OpenResult(int (*fetch)(void *, uint8_t *), const uint8_t *(*deviceData)(void *), void (*close)(void *))
      : fetch_(fetch), deviceData_(deviceData), close_(close) {}
  OpenResult(const OpenResult &) = delete;
  OpenResult &operator=(const OpenResult &) = delete;
  ~OpenResult() { close_(ctx); }

  // The result's `bytes` of stream as a .spz file image in *out, then closed.  The device writer reads the result's own
  // device copy instead of uploading the host one.  The caller has released the input's device memory by now: the
  // container stage takes its own.
  bool finish(const char *who, uint64_t bytes, Laps *laps, std::vector<uint8_t> *out) {
    std::vector<uint8_t> stream;
    detail::resizeUninitialized(&stream, static_cast<size_t>(bytes));
    if (deviceFailed(fetch_(ctx, stream.data()), who)) return false;
    if (laps) laps->lap("download");
    if (!compressGzippedWithCopy(stream.data(), stream.size(), out, deviceData_(ctx))) {
      logLine("[SPZ ERROR] %s: compressGzipped failed", who);
      return false;
    }
    if (laps) laps->lap("gzip");
    close_(ctx);
    ctx = nullptr;
    return true;
  }

  void *ctx = nullptr;

 private:
  int (*fetch_)(void *, uint8_t *);
  const uint8_t *(*deviceData_)(void *);
  void (*close_)(void *);
};

// The input file of a file-name form, or false with the reader's line or "<who>: <name> is larger than 2 GiB".
bool readInput(const char *who, const std::string &filename, std::vector<uint8_t> *data) {
  if (!readFile(filename, data, /*log=*/true)) return false;
  if (data->size() > static_cast<size_t>(INT32_MAX)) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "%s is larger than 2 GiB", filename.c_str());
  }
  return true;
}

// The file image written, or false with "<who>: unable to write <name>".
bool writeOutput(const char *who, const std::string &filename, const std::vector<uint8_t> &file) {
  if (writeFile(filename, file)) return true;
  logLine("[SPZ ERROR] %s: unable to write %s", who, filename.c_str());
  return false;
}

// The file-name form of an operation whose options the caller has checked: the input read, `run` (the buffer form, its
// results into the caller's temporaries) on its bytes, the file image written as the "write" lap under `env`.  The
// caller sets its out-parameters from the temporaries only when this returns true.
template <class Run>
bool fileToFile(const char *who, const char *env, const std::string &input, const std::string &output, Run run) {
  std::vector<uint8_t> data;
  if (!readInput(who, input, &data)) return false;
  std::vector<uint8_t> file;
  if (!run(data.data(), static_cast<int32_t>(data.size()), &file)) return false;
  Laps laps(who, env);
  if (!writeOutput(who, output, file)) return false;
  laps.lap("write");
  return true;
}
}  // namespace

// ---- filter ------------------------------------------------------------------------------------------------------
namespace {
// Every check that needs no input.
bool filterOptionsOk(const FilterOptions &f) {
  const char *who = "filterSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  if (f.shDegree < -1 || f.shDegree > 3) return opRejected(who, invalid, "shDegree %d is outside -1 ... 3", f.shDegree);
  if (f.indices && (f.mask || f.box || f.minAlpha)) return opRejected(who, invalid, "indices cannot be combined with a mask, a box or minAlpha");
  if (static_cast<int>(f.coord) < 0 || static_cast<int>(f.coord) > 8) return opRejected(who, invalid, "unknown coordinate system %d", static_cast<int>(f.coord));
  if (f.box) {
    for (int a = 0; a < 3; ++a) {
      if (std::isnan(f.box->lo[a]) || std::isnan(f.box->hi[a])) return opRejected(who, invalid, "a box bound is NaN");
    }
  }
  if (f.minAlpha && std::isnan(*f.minAlpha)) return opRejected(who, invalid, "minAlpha is NaN");
  if (f.indices && f.indices->size() > SPZ_AMD_REFERENCE_MAX_POINTS) {
    return opRejected(who, invalid, "%zu indices: the reference reads at most %u points", f.indices->size(), SPZ_AMD_REFERENCE_MAX_POINTS);
  }
  return true;
}
}  // namespace

bool filterSpz(const uint8_t *data, int32_t size, const FilterOptions &f, std::vector<uint8_t> *out, int64_t *kept) {
  const char *who = "filterSpz";
  g_last_status = SPZ_AMD_OK;
  if (kept) *kept = 0;
  // the arguments first: nothing touches the device before they are known to be good
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  if (!filterOptionsOk(f)) return false;
  Laps laps(who, "SPZ_AMD_FILTER_TIMING");
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  laps.lap("inflate");
  const uint32_t n = static_cast<uint32_t>(d.numPoints);
  if (f.shDegree > d.shDegree) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "shDegree %d is above the input's %d", f.shDegree, d.shDegree);
  if (f.mask && f.mask->size() != n) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "the mask has %zu bytes for %u points", f.mask->size(), n);
  if (f.indices) {
    for (const uint32_t i : *f.indices) {
      if (i >= n) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "index %u is out of range for %u points", i, n);
    }
  }
  const spz_amd_header hdr = headerOf(d);
  spz_amd_selection sel = {};
  sel.to_coord = static_cast<int32_t>(f.coord);
  if (f.box) {
    sel.use_box = 1;
    for (int a = 0; a < 3; ++a) {
      sel.box_lo[a] = f.box->lo[a];
      sel.box_hi[a] = f.box->hi[a];
    }
  }
  if (f.minAlpha) {
    sel.use_min_alpha = 1;
    sel.min_alpha = *f.minAlpha;
  }
  OpenResult r(spz_amd_filter_fetch, spz_amd_filter_device_data, spz_amd_filter_close);
  uint64_t count = 0, bytes = 0;
  float ms[2] = {0.0f, 0.0f};
  const int rc = spz_amd_filter_open(d.stream, d.streamBytes, &hdr, &sel, f.mask ? f.mask->data() : nullptr, f.indices ? 1 : 0,
                                     f.indices ? f.indices->data() : nullptr, f.indices ? f.indices->size() : 0, f.shDegree,
                                     d.device, &r.ctx, &count, &bytes, ms);
  if (deviceFailed(rc, who)) return false;
  laps.stage("select", ms[0]);
  laps.stage("subset", ms[1]);
  laps.lap("filter");
  d.release();
  if (!r.finish(who, bytes, &laps, out)) return false;
  if (kept) *kept = static_cast<int64_t>(count);
  return true;
}

bool filterSpz(const std::string &inputFilename, const std::string &outputFilename, const FilterOptions &f, int64_t *kept) {
  g_last_status = SPZ_AMD_OK;
  if (kept) *kept = 0;
  if (!filterOptionsOk(f)) return false;
  int64_t k = 0;
  if (!fileToFile("filterSpz", "SPZ_AMD_FILTER_TIMING", inputFilename, outputFilename,
                  [&](const uint8_t *data, int32_t size, std::vector<uint8_t> *file) { return filterSpz(data, size, f, file, &k); })) {
    return false;
  }
  if (kept) *kept = k;
  return true;
}

// ---- transform ---------------------------------------------------------------------------------------------------
namespace {
// The parameter block of `o`, or false + the [SPZ ERROR] line: every check that needs no device.
bool transformBlock(const char *who, const TransformOptions &o, bool packed, spz_amd_transform *xf) {
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  if (static_cast<int>(o.coord) < 0 || static_cast<int>(o.coord) > 8) return opRejected(who, invalid, "unknown coordinate system %d", static_cast<int>(o.coord));
  if (packed && (o.fractionalBits < 0 || o.fractionalBits > 24)) return opRejected(who, invalid, "fractionalBits %d is outside 0 ... 24", o.fractionalBits);
  if (spz_amd_transform_params(o.rotation.data(), o.translation.data(), o.scale, static_cast<int>(o.coord), xf) != SPZ_AMD_OK) {
    return opRejected(who, invalid, "the rotation must be finite and nonzero, the translation finite, the scale finite and > 0");
  }
  return true;
}

// A placement's positions that did not fit 24 bits: refused.
bool outOfRange(const char *who, uint64_t bad, uint32_t points, int fractionalBits) {
  return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "%llu of %u points have a position that does not fit 24 bits at %d fractional bits "
                    "(lower fractionalBits)", static_cast<unsigned long long>(bad), points, fractionalBits);
}
}  // namespace

bool transformSpz(const uint8_t *data, int32_t size, const TransformOptions &o, std::vector<uint8_t> *out) {
  const char *who = "transformSpz";
  g_last_status = SPZ_AMD_OK;
  // the arguments first: nothing touches the device before they are known to be good
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  spz_amd_transform xf;
  if (!transformBlock(who, o, true, &xf)) return false;
  Laps laps(who, "SPZ_AMD_TRANSFORM_TIMING");
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  laps.lap("inflate");
  const spz_amd_header hdr = headerOf(d);
  OpenResult r(spz_amd_transform_fetch, spz_amd_transform_device_data, spz_amd_transform_close);
  uint64_t bytes = 0, bad = 0;
  float ms = 0.0f;
  const int rc = spz_amd_transform_open(d.stream, d.streamBytes, &hdr, &xf, o.fractionalBits, d.device, &r.ctx, &bytes, &bad, &ms);
  if (deviceFailed(rc, who)) return false;
  laps.stage("kernel", ms);
  laps.lap("transform");
  if (bad > 0) return outOfRange(who, bad, hdr.num_points, o.fractionalBits);
  d.release();
  return r.finish(who, bytes, &laps, out);
}

bool transformSpz(const std::string &inputFilename, const std::string &outputFilename, const TransformOptions &o) {
  g_last_status = SPZ_AMD_OK;
  spz_amd_transform xf;
  if (!transformBlock("transformSpz", o, true, &xf)) return false;
  return fileToFile("transformSpz", "SPZ_AMD_TRANSFORM_TIMING", inputFilename, outputFilename,
                    [&](const uint8_t *data, int32_t size, std::vector<uint8_t> *file) { return transformSpz(data, size, o, file); });
}

bool transformCloud(GaussianCloud &g, const TransformOptions &o) {
  g_last_status = SPZ_AMD_OK;
  spz_amd_transform xf;
  if (!transformBlock("transformCloud", o, false, &xf)) return false;
  if (!checkSizes(g)) return opRejected("transformCloud", SPZ_AMD_ERR_INVALID_ARG, "the cloud's arrays do not match numPoints / shDegree");
  const int rc = spz_amd_transform_cloud_host(g.positions.data(), g.scales.data(), g.rotations.data(),
                                              g.sh.empty() ? nullptr : g.sh.data(), static_cast<uint64_t>(g.numPoints),
                                              g.shDegree, &xf, deviceIndex());
  return !deviceFailed(rc, "transformCloud");
}

// ---- merge -------------------------------------------------------------------------------------------------------
namespace {
// The placement blocks of `o` for k inputs (nullopt: none), or false + the [SPZ ERROR] line: every check that needs no
// device and no header.
bool mergeArguments(size_t k, const MergeOptions &o, std::vector<std::optional<spz_amd_transform>> *xfs) {
  const char *who = "mergeSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  if (k == 0) return opRejected(who, invalid, "no inputs");
  if (k > SPZ_AMD_MERGE_MAX_INPUTS) return opRejected(who, invalid, "%zu inputs: at most %u can be merged", k, SPZ_AMD_MERGE_MAX_INPUTS);
  if (o.shDegree < -1 || o.shDegree > 3) return opRejected(who, invalid, "shDegree %d is outside -1 ... 3", o.shDegree);
  if (o.fractionalBits < -1 || o.fractionalBits > 24) return opRejected(who, invalid, "fractionalBits %d is outside -1 ... 24", o.fractionalBits);
  if (o.antialiased < -1 || o.antialiased > 1) return opRejected(who, invalid, "antialiased %d is not -1, 0 or 1", o.antialiased);
  if (!o.transforms.empty() && o.transforms.size() != k) {
    return opRejected(who, invalid, "%zu transforms for %zu inputs (give none or one per input)", o.transforms.size(), k);
  }
  xfs->assign(k, std::nullopt);
  for (size_t i = 0; i < o.transforms.size(); ++i) {
    if (!o.transforms[i]) continue;
    spz_amd_transform xf;
    if (!transformBlock(who, *o.transforms[i], false, &xf)) return false;
    (*xfs)[i] = xf;
  }
  return true;
}

// spz_amd_merge_resolve's refusals, each with its reason.
bool mergeResolved(const std::vector<spz_amd_header> &h, const MergeOptions &o, spz_amd_header *oh) {
  const char *who = "mergeSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  const int rc = spz_amd_merge_resolve(h.data(), h.size(), o.shDegree, o.fractionalBits, o.antialiased, oh, nullptr);
  if (rc == SPZ_AMD_OK) return true;
  uint64_t total = 0;
  for (const spz_amd_header &x : h) total += x.num_points;
  if (rc == SPZ_AMD_ERR_TOO_MANY_POINTS) {
    return opRejected(who, invalid, "%llu points in all: the reference reads at most %u", static_cast<unsigned long long>(total),
                      SPZ_AMD_REFERENCE_MAX_POINTS);
  }
  for (size_t i = 1; i < h.size() && o.antialiased < 0; ++i) {
    if ((h[i].flags & 1) != (h[0].flags & 1)) {
      return opRejected(who, invalid, "input 0 has antialiased = %d and input %zu has antialiased = %d (set antialiased)",
                        h[0].flags & 1, i, h[i].flags & 1);
    }
  }
  return opRejected(who, invalid, "the inputs cannot be merged (%s)", spz_amd_status_string(rc));
}
}  // namespace

bool mergeSpz(const std::vector<std::vector<uint8_t>> &inputs, const MergeOptions &o, std::vector<uint8_t> *out, int64_t *points) {
  const char *who = "mergeSpz";
  g_last_status = SPZ_AMD_OK;
  if (points) *points = 0;
  // the arguments first: nothing touches the device before they are known to be good
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  std::vector<std::optional<spz_amd_transform>> xfs;
  if (!mergeArguments(inputs.size(), o, &xfs)) return false;
  for (size_t i = 0; i < inputs.size(); ++i) {
    if (inputs[i].size() > static_cast<size_t>(INT32_MAX)) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "input %zu is larger than 2 GiB", i);
  }
  const size_t k = inputs.size();
  std::vector<DevicePackedGaussians> d(k);
  std::vector<spz_amd_header> hdrs(k);
  for (size_t i = 0; i < k; ++i) {
    d[i] = loadSpzPackedDevice(inputs[i].data(), static_cast<int32_t>(inputs[i].size()));
    if (!d[i].valid()) {
      if (g_last_status == SPZ_AMD_OK) logLine("[SPZ ERROR] mergeSpz: input %zu is not a readable .spz", i);
      return false;
    }
    hdrs[i] = headerOf(d[i]);
  }
  spz_amd_header oh;
  if (!mergeResolved(hdrs, o, &oh)) return false;
  std::vector<spz_amd_merge_input> in(k);
  for (size_t i = 0; i < k; ++i) {
    if (d[i].device != d[0].device) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "the inputs were loaded on different devices");
    in[i].d_stream = d[i].stream;
    in[i].size = d[i].streamBytes;
    in[i].hdr = hdrs[i];
    in[i].xf = xfs[i] ? &*xfs[i] : nullptr;
  }
  OpenResult r(spz_amd_merge_fetch, spz_amd_merge_device_data, spz_amd_merge_close);
  uint64_t bytes = 0, bad = 0;
  const int rc = spz_amd_merge_open(in.data(), k, o.shDegree, o.fractionalBits, o.antialiased, d[0].device, &r.ctx, &oh, &bytes, &bad, nullptr);
  if (deviceFailed(rc, who)) return false;
  if (bad > 0) return outOfRange(who, bad, oh.num_points, oh.fractional_bits);
  d.clear();
  if (!r.finish(who, bytes, nullptr, out)) return false;
  if (points) *points = oh.num_points;
  return true;
}

bool mergeSpz(const std::vector<std::string> &inputFilenames, const std::string &outputFilename, const MergeOptions &o,
              int64_t *points) {
  g_last_status = SPZ_AMD_OK;
  if (points) *points = 0;
  std::vector<std::optional<spz_amd_transform>> xfs;
  if (!mergeArguments(inputFilenames.size(), o, &xfs)) return false;
  std::vector<std::vector<uint8_t>> data(inputFilenames.size());
  for (size_t i = 0; i < inputFilenames.size(); ++i) {
    if (!readFile(inputFilenames[i], &data[i], /*log=*/true)) return false;
  }
  std::vector<uint8_t> file;
  int64_t n = 0;
  if (!mergeSpz(data, o, &file, &n) || !writeOutput("mergeSpz", outputFilename, file)) return false;
  if (points) *points = n;
  return true;
}

// ---- sort --------------------------------------------------------------------------------------------------------
namespace {
bool sortOptionsOk(const SortOptions &o) {
  if (o.keys && o.keys->size() > SPZ_AMD_REFERENCE_MAX_POINTS) {
    return opRejected("sortSpz", SPZ_AMD_ERR_INVALID_ARG, "%zu keys: the reference reads at most %u points", o.keys->size(),
                      SPZ_AMD_REFERENCE_MAX_POINTS);
  }
  return true;
}
}  // namespace

bool sortSpz(const uint8_t *data, int32_t size, const SortOptions &o, std::vector<uint8_t> *out,
             std::vector<uint32_t> *order) {
  const char *who = "sortSpz";
  g_last_status = SPZ_AMD_OK;
  if (order) order->clear();
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  if (!sortOptionsOk(o)) return false;
  Laps laps(who, "SPZ_AMD_SORT_TIMING");
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  laps.lap("inflate");
  const uint64_t n = static_cast<uint64_t>(d.numPoints);
  if (o.keys && o.keys->size() != n) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "%zu keys for %llu points", o.keys->size(), (unsigned long long)n);
  }
  if (!o.keys && d.version == 1) {
    return opRejected(who, SPZ_AMD_ERR_UNSUPPORTED,
                      "a version 1 file has float16 positions and no Morton key; transformSpz with the identity "
                      "writes a v3 copy");
  }
  const spz_amd_header hdr = headerOf(d);
  std::vector<uint32_t> ord;
  if (order) detail::resizeUninitialized(&ord, static_cast<size_t>(n));
  OpenResult r(spz_amd_sort_fetch, spz_amd_sort_device_data, spz_amd_sort_close);
  uint64_t bytes = 0;
  float ms[2] = {0.0f, 0.0f};
  const int rc = spz_amd_sort_open(d.stream, d.streamBytes, &hdr, o.keys ? o.keys->data() : nullptr, o.descending ? 1 : 0,
                                   d.device, &r.ctx, &bytes, order ? ord.data() : nullptr, ms);
  if (deviceFailed(rc, who)) return false;
  laps.stage("order", ms[0]);
  laps.stage("subset", ms[1]);
  laps.lap("sort");
  d.release();
  if (!r.finish(who, bytes, &laps, out)) return false;
  if (order) order->swap(ord);
  return true;
}

bool sortSpz(const std::string &inputFilename, const std::string &outputFilename, const SortOptions &o,
             std::vector<uint32_t> *order) {
  g_last_status = SPZ_AMD_OK;
  if (order) order->clear();
  if (!sortOptionsOk(o)) return false;
  std::vector<uint32_t> ord;
  if (!fileToFile("sortSpz", "SPZ_AMD_SORT_TIMING", inputFilename, outputFilename,
                  [&](const uint8_t *data, int32_t size, std::vector<uint8_t> *file) {
                    return sortSpz(data, size, o, file, order ? &ord : nullptr);
                  })) {
    return false;
  }
  if (order) order->swap(ord);
  return true;
}

// ---- decimate ----------------------------------------------------------------------------------------------------
namespace {
// Exactly one of the two, each in range.
bool decimateOptionsOk(const DecimateOptions &o) {
  const char *who = "decimateSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  if (o.level.has_value() == o.targetPoints.has_value()) {
    return opRejected(who, invalid, "exactly one of level and targetPoints must be set");
  }
  if (o.level && (*o.level < 0 || *o.level > 24)) return opRejected(who, invalid, "level %d is outside 0..24", *o.level);
  if (o.targetPoints && *o.targetPoints == 0) return opRejected(who, invalid, "targetPoints must be >= 1");
  return true;
}
}  // namespace

bool decimateSpz(const uint8_t *data, int32_t size, const DecimateOptions &o, std::vector<uint8_t> *out,
                 std::vector<uint32_t> *parents, int *level, int64_t *points) {
  const char *who = "decimateSpz";
  g_last_status = SPZ_AMD_OK;
  if (parents) parents->clear();
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  if (!decimateOptionsOk(o)) return false;
  Laps laps(who, "SPZ_AMD_DECIMATE_TIMING");
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  laps.lap("inflate");
  if (d.version == 1) {
    return opRejected(who, SPZ_AMD_ERR_UNSUPPORTED,
                      "a version 1 file has float16 positions and no integer cell; transformSpz with the "
                      "identity writes a v3 copy");
  }
  const uint64_t n = static_cast<uint64_t>(d.numPoints);
  const spz_amd_header hdr = headerOf(d);
  std::vector<uint32_t> par;
  if (parents) detail::resizeUninitialized(&par, static_cast<size_t>(n));
  OpenResult r(spz_amd_decimate_fetch, spz_amd_decimate_device_data, spz_amd_decimate_close);
  uint64_t bytes = 0;
  int used = -1;
  spz_amd_header outHdr = {};
  float ms[3] = {0.0f, 0.0f, 0.0f};
  const int rc = spz_amd_decimate_open(d.stream, d.streamBytes, &hdr, o.level ? *o.level : -1,
                                       o.targetPoints ? *o.targetPoints : 0, d.device, &r.ctx, &bytes, &used, &outHdr,
                                       parents ? par.data() : nullptr, ms);
  if (deviceFailed(rc, who)) return false;
  laps.stage("sort", ms[0]);
  laps.stage("levels", ms[1]);
  laps.stage("reduce", ms[2]);
  laps.lap("decimate");
  d.release();
  if (!r.finish(who, bytes, &laps, out)) return false;
  if (parents) parents->swap(par);
  if (level) *level = used;
  if (points) *points = outHdr.num_points;
  return true;
}

bool decimateSpz(const std::string &inputFilename, const std::string &outputFilename, const DecimateOptions &o,
                 std::vector<uint32_t> *parents, int *level, int64_t *points) {
  g_last_status = SPZ_AMD_OK;
  if (parents) parents->clear();
  if (!decimateOptionsOk(o)) return false;
  std::vector<uint32_t> par;
  int used = -1;
  int64_t count = 0;
  if (!fileToFile("decimateSpz", "SPZ_AMD_DECIMATE_TIMING", inputFilename, outputFilename,
                  [&](const uint8_t *data, int32_t size, std::vector<uint8_t> *file) {
                    return decimateSpz(data, size, o, file, parents ? &par : nullptr, &used, &count);
                  })) {
    return false;
  }
  if (parents) parents->swap(par);
  if (level) *level = used;
  if (points) *points = count;
  return true;
}

// ---- clean -------------------------------------------------------------------------------------------------------
namespace {
// At least one rule, each in range.
bool cleanOptionsOk(const CleanOptions &o) {
  const char *who = "cleanSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  if (!o.statistical && !o.radius) return opRejected(who, invalid, "set statistical, radius or both");
  if (o.statistical) {
    if (o.statistical->k < 1 || o.statistical->k > 64) return opRejected(who, invalid, "k %d is outside 1..64", o.statistical->k);
    if (!std::isfinite(o.statistical->stdRatio)) return opRejected(who, invalid, "stdRatio must be finite");
  }
  if (o.radius) {
    if (!std::isfinite(o.radius->radius) || !(o.radius->radius > 0.0)) return opRejected(who, invalid, "radius must be finite and > 0");
    if (o.radius->minNeighbors < 1 || o.radius->minNeighbors > 256) {
      return opRejected(who, invalid, "minNeighbors %d is outside 1..256", o.radius->minNeighbors);
    }
  }
  return true;
}
}  // namespace

bool cleanSpz(const uint8_t *data, int32_t size, const CleanOptions &o, std::vector<uint8_t> *out, int64_t *kept,
              std::vector<uint8_t> *keepMask, std::vector<double> *scores, double *threshold) {
  const char *who = "cleanSpz";
  g_last_status = SPZ_AMD_OK;
  if (keepMask) keepMask->clear();
  if (scores) scores->clear();
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  if (!cleanOptionsOk(o)) return false;
  Laps laps(who, "SPZ_AMD_CLEAN_TIMING");
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  laps.lap("inflate");
  if (d.version == 1) {
    return opRejected(who, SPZ_AMD_ERR_UNSUPPORTED,
                      "a version 1 file has float16 positions and no integer distances; transformSpz with the "
                      "identity writes a v3 copy");
  }
  const uint64_t n = static_cast<uint64_t>(d.numPoints);
  const spz_amd_header hdr = headerOf(d);
  std::vector<uint8_t> mask;
  std::vector<double> sc;
  if (keepMask) detail::resizeUninitialized(&mask, static_cast<size_t>(n));
  if (scores && o.statistical) detail::resizeUninitialized(&sc, static_cast<size_t>(n));
  OpenResult r(spz_amd_clean_fetch, spz_amd_clean_device_data, spz_amd_clean_close);
  uint64_t bytes = 0, count = 0;
  double thr = 0.0;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  const int rc = spz_amd_clean_open(d.stream, d.streamBytes, &hdr, o.statistical ? o.statistical->k : 0,
                                    o.statistical ? o.statistical->stdRatio : 0.0, o.radius ? o.radius->radius : 0.0,
                                    o.radius ? static_cast<uint32_t>(o.radius->minNeighbors) : 0u, d.device, &r.ctx, &bytes,
                                    &count, &thr, keepMask ? mask.data() : nullptr,
                                    scores && o.statistical ? sc.data() : nullptr, ms);
  if (deviceFailed(rc, who)) return false;
  laps.stage("sort", ms[0]);
  laps.stage("search", ms[1]);
  laps.stage("subset", ms[2]);
  laps.lap("clean");
  d.release();
  if (!r.finish(who, bytes, &laps, out)) return false;
  if (kept) *kept = static_cast<int64_t>(count);
  if (keepMask) keepMask->swap(mask);
  if (scores) scores->swap(sc);
  if (threshold) *threshold = thr;
  return true;
}

bool cleanSpz(const std::string &inputFilename, const std::string &outputFilename, const CleanOptions &o,
              int64_t *kept, std::vector<uint8_t> *keepMask, std::vector<double> *scores, double *threshold) {
  g_last_status = SPZ_AMD_OK;
  if (keepMask) keepMask->clear();
  if (scores) scores->clear();
  if (!cleanOptionsOk(o)) return false;
  std::vector<uint8_t> mask;
  std::vector<double> sc;
  int64_t count = 0;
  double thr = 0.0;
  if (!fileToFile("cleanSpz", "SPZ_AMD_CLEAN_TIMING", inputFilename, outputFilename,
                  [&](const uint8_t *data, int32_t size, std::vector<uint8_t> *file) {
                    return cleanSpz(data, size, o, file, &count, keepMask ? &mask : nullptr, scores ? &sc : nullptr, &thr);
                  })) {
    return false;
  }
  if (kept) *kept = count;
  if (keepMask) keepMask->swap(mask);
  if (scores) scores->swap(sc);
  if (threshold) *threshold = thr;
  return true;
}

// ---- render ------------------------------------------------------------------------------------------------------
namespace {
// What a view is rendered with beside its camera: the option fields that vary between the callers, and how their
// "bad camera" line ends.
struct ViewFrame {
  float nearPlane;
  CoordinateSystem coord;
  const std::array<float, 3> *background;  // NULL: black
  int maxShDegree;
  const char *alsoChecked;  // what the caller's "bad camera" line names after "values finite" (the texts differ)
};

// One view as render params, checked; `label` ("view 3: " or "") leads the line of a refused one.
bool viewParams(const char *who, const char *label, const PruneOptions::View &w, const ViewFrame &f,
                spz_amd_render_params *p) {
  *p = spz_amd_render_params{};
  if (w.width < 1 || w.width > 16384 || w.height < 1 || w.height > 16384) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "%simage size %d x %d is outside 1..16384", label, w.width, w.height);
  }
  for (int k = 0; k < 12; ++k) p->world_to_camera[k] = w.worldToCamera[k];
  p->fx = w.fx;
  p->fy = w.fy;
  p->cx = w.cx;
  p->cy = w.cy;
  p->width = static_cast<uint32_t>(w.width);
  p->height = static_cast<uint32_t>(w.height);
  p->near_plane = f.nearPlane;
  for (int k = 0; k < 3; ++k) p->background[k] = f.background ? (*f.background)[k] : 0.0f;
  p->max_sh_degree = f.maxShDegree;
  p->coord = static_cast<int32_t>(f.coord);
  if (spz_amd_render_check_params(p) != SPZ_AMD_OK) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG,
                      "%sbad camera: R must be a rotation (to 1e-4), fx, fy > 0, nearPlane > 0, values finite%s", label,
                      f.alsoChecked);
  }
  return true;
}

// The views of prune, compare and refine as render params: 1..maxViews of them, each checked and named by its index.
bool viewListParams(const char *who, const std::vector<PruneOptions::View> &views, int maxViews, const ViewFrame &f,
                    std::vector<spz_amd_render_params> *params) {
  if (views.empty() || views.size() > static_cast<size_t>(maxViews)) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "%zu views: give 1..%d", views.size(), maxViews);
  }
  params->assign(views.size(), spz_amd_render_params{});
  for (size_t v = 0; v < views.size(); ++v) {
    const std::string label = "view " + std::to_string(v) + ": ";
    if (!viewParams(who, label.c_str(), views[v], f, &(*params)[v])) return false;
  }
  return true;
}

// After a multi-view device call: true when it failed, with the view the device named in the line.
bool viewsFailed(const char *who, int rc, int32_t bad) {
  if (rc == SPZ_AMD_ERR_CAPACITY && bad >= 0) return !opRejected(who, rc, "view %d: more than 2^31 - 1 tile entries", bad);
  if (rc != SPZ_AMD_OK && bad >= 0) logLine("[SPZ ERROR] %s: view %d failed", who, bad);
  return deviceFailed(rc, who);
}

bool renderParams(const RenderOptions &o, spz_amd_render_params *p, const char *op) {
  PruneOptions::View w;
  w.worldToCamera = o.worldToCamera;
  w.fx = o.fx;
  w.fy = o.fy;
  w.cx = o.cx;
  w.cy = o.cy;
  w.width = o.width;
  w.height = o.height;
  return viewParams(op, "", w, {o.nearPlane, o.coord, &o.background, o.maxShDegree, ", maxShDegree 0..3"}, p);
}

void renderTiming(const float *ms, uint64_t entries, const char *op = "renderSpz") {
  const Laps laps(op, "SPZ_AMD_RENDER_TIMING");
  laps.stage("preprocess", ms[0]);
  laps.stage("entries", ms[1], (" (" + std::to_string(entries) + ")").c_str());
  laps.stage("blend", ms[2]);
}

// The cloud's arrays as the C ABI takes them; false when they do not match numPoints and shDegree.
bool cloudArrays(const GaussianCloud &g, spz_amd_cloud_in *c, size_t *n) {
  *n = g.numPoints < 0 ? 0 : static_cast<size_t>(g.numPoints);
  const int sd = g.shDegree == 0 ? 0 : g.shDegree == 1 ? 3 : g.shDegree == 2 ? 8 : g.shDegree == 3 ? 15 : -1;
  if (g.numPoints < 0 || sd < 0 || g.positions.size() != *n * 3 || g.scales.size() != *n * 3 ||
      g.rotations.size() != *n * 4 || g.alphas.size() != *n || g.colors.size() != *n * 3 ||
      g.sh.size() != *n * static_cast<size_t>(sd) * 3) {
    return false;
  }
  *c = {g.positions.data(), g.scales.data(), g.rotations.data(), g.alphas.data(), g.colors.data(),
        sd ? g.sh.data() : nullptr};
  return true;
}

// The buffers a depth call fills, and the maps derived from them once it has succeeded.
struct DepthBuffers {
  std::vector<float> img, depth;
  std::vector<uint32_t> index;
  explicit DepthBuffers(const RenderOptions &o) {
    const size_t px = static_cast<size_t>(o.width) * static_cast<size_t>(o.height);
    detail::resizeUninitialized(&img, px * 4u);
    detail::resizeUninitialized(&depth, px * 2u);
    index.resize(px);
  }
  void finish(DepthMaps *maps, std::vector<float> *rgba) {
    const size_t px = index.size();
    DepthMaps m;
    m.expected.resize(px);
    m.median.resize(px);
    m.accumulated.resize(px);
    m.alpha.resize(px);
    for (size_t i = 0; i < px; ++i) {
      const float acc = depth[i * 2], alpha = img[i * 4 + 3];
      m.accumulated[i] = acc;
      m.median[i] = depth[i * 2 + 1];
      m.alpha[i] = alpha;
      m.expected[i] = alpha > 0.0f ? acc / alpha : std::numeric_limits<float>::infinity();
    }
    m.index.swap(index);
    *maps = std::move(m);
    if (rgba) rgba->swap(img);
  }
};
}  // namespace

namespace {
// The four render entry points: a packed input (`data`) or a cloud (`g`), into the image alone or (wantMaps) into
// depth maps with an optional image.  `op` names the call in its rejections and timings, `deviceOp` in a device failure.
bool renderAny(const char *op, const char *deviceOp, const uint8_t *data, int32_t size, const GaussianCloud *g,
               const RenderOptions &o, DepthMaps *maps, bool wantMaps, std::vector<float> *rgba, int64_t *entries) {
  g_last_status = SPZ_AMD_OK;
  if (wantMaps && maps == nullptr) return opRejected(op, SPZ_AMD_ERR_INVALID_ARG, "no output maps");
  if (!wantMaps && rgba == nullptr) return opRejected(op, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  spz_amd_render_params p;
  if (!renderParams(o, &p, op)) return false;
  DevicePackedGaussians d;
  spz_amd_header hdr = {};
  spz_amd_cloud_in c = {};
  size_t n = 0;
  if (g == nullptr) {
    if (!loadInput(op, data, size, &d)) return false;
    hdr = headerOf(d);
  } else if (!cloudArrays(*g, &c, &n)) {
    return opRejected(op, SPZ_AMD_ERR_INVALID_ARG, "the cloud's arrays do not match numPoints and shDegree");
  }
  const int aa = g && g->antialiased ? 1 : 0, device = g ? deviceIndex() : d.device;
  std::vector<float> img;
  std::optional<DepthBuffers> b;
  if (wantMaps) {
    b.emplace(o);
  } else {
    detail::resizeUninitialized(&img, static_cast<size_t>(o.width) * static_cast<size_t>(o.height) * 4u);
  }
  uint64_t count = 0;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  int rc;
  if (wantMaps) {
    rc = g ? spz_amd_render_depth_cloud_host(&c, n, g->shDegree, aa, &p, device, b->img.data(), b->depth.data(),
                                             b->index.data(), &count, ms)
           : spz_amd_render_depth_host(d.stream, d.streamBytes, &hdr, &p, device, b->img.data(), b->depth.data(),
                                       b->index.data(), &count, ms);
  } else {
    rc = g ? spz_amd_render_cloud_host(&c, n, g->shDegree, aa, &p, device, img.data(), &count, ms)
           : spz_amd_render_host(d.stream, d.streamBytes, &hdr, &p, device, img.data(), &count, ms);
  }
  if (deviceFailed(rc, deviceOp)) return false;
  renderTiming(ms, count, op);
  if (wantMaps) {
    b->finish(maps, rgba);
  } else {
    rgba->swap(img);
  }
  if (entries) *entries = static_cast<int64_t>(count);
  return true;
}
}  // namespace

bool renderSpz(const uint8_t *data, int32_t size, const RenderOptions &o, std::vector<float> *rgba, int64_t *entries) {
  return renderAny("renderSpz", "renderSpz", data, size, nullptr, o, nullptr, false, rgba, entries);
}

bool renderSpz(const std::string &filename, const RenderOptions &o, std::vector<float> *rgba, int64_t *entries) {
  g_last_status = SPZ_AMD_OK;
  spz_amd_render_params p;
  if (!renderParams(o, &p, "renderSpz")) return false;
  std::vector<uint8_t> data;
  if (!readInput("renderSpz", filename, &data)) return false;
  return renderSpz(data.data(), static_cast<int32_t>(data.size()), o, rgba, entries);
}

bool renderCloud(const GaussianCloud &g, const RenderOptions &o, std::vector<float> *rgba, int64_t *entries) {
  return renderAny("renderSpz", "renderCloud", nullptr, 0, &g, o, nullptr, false, rgba, entries);
}

bool renderSpzDepth(const uint8_t *data, int32_t size, const RenderOptions &o, DepthMaps *maps, std::vector<float> *rgba,
                    int64_t *entries) {
  return renderAny("renderSpzDepth", "renderSpzDepth", data, size, nullptr, o, maps, true, rgba, entries);
}

bool renderSpzDepth(const std::string &filename, const RenderOptions &o, DepthMaps *maps, std::vector<float> *rgba,
                    int64_t *entries) {
  g_last_status = SPZ_AMD_OK;
  if (maps == nullptr) return opRejected("renderSpzDepth", SPZ_AMD_ERR_INVALID_ARG, "no output maps");
  spz_amd_render_params p;
  if (!renderParams(o, &p, "renderSpzDepth")) return false;
  std::vector<uint8_t> data;
  if (!readInput("renderSpzDepth", filename, &data)) return false;
  return renderSpzDepth(data.data(), static_cast<int32_t>(data.size()), o, maps, rgba, entries);
}

bool renderCloudDepth(const GaussianCloud &g, const RenderOptions &o, DepthMaps *maps, std::vector<float> *rgba,
                      int64_t *entries) {
  return renderAny("renderSpzDepth", "renderSpzDepth", nullptr, 0, &g, o, maps, true, rgba, entries);
}

std::array<float, 12> lookAt(const std::array<float, 3> &eye, const std::array<float, 3> &target,
                             const std::array<float, 3> &up) {
  double f[3], u[3], e[3];
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(eye[k]) || !std::isfinite(target[k]) || !std::isfinite(up[k])) {
      throw std::invalid_argument("lookAt: values must be finite");
    }
    e[k] = eye[k];
    f[k] = static_cast<double>(target[k]) - eye[k];
    u[k] = up[k];
  }
  auto norm = [](double *v) {
    const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(l > 0.0)) return false;
    for (int k = 0; k < 3; ++k) v[k] /= l;
    return true;
  };
  auto cross = [](const double *a, const double *b, double *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
  };
  if (!norm(f) || !norm(u)) throw std::invalid_argument("lookAt: eye equals target, or up is zero");
  double x[3], y[3];
  cross(f, u, x);
  const double sx = std::sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  if (!(sx > 1e-6)) throw std::invalid_argument("lookAt: up is parallel to the view direction");
  norm(x);
  cross(f, x, y);
  std::array<float, 12> m;
  const double *rows[3] = {x, y, f};
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) m[r * 4 + k] = static_cast<float>(rows[r][k]);
    m[r * 4 + 3] = static_cast<float>(-(rows[r][0] * e[0] + rows[r][1] * e[1] + rows[r][2] * e[2]));
  }
  return m;
}

// ---- prune -------------------------------------------------------------------------------------------------------
namespace {
// The views as render params, and exactly one rule in range (keepCount's upper bound needs n: checked later).
bool pruneOptionsOk(const PruneOptions &o, std::vector<spz_amd_render_params> *params) {
  const char *who = "pruneSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  const int rules = (o.keepCount ? 1 : 0) + (o.keepFraction ? 1 : 0) + (o.minScore ? 1 : 0);
  if (rules != 1) return opRejected(who, invalid, "set exactly one of keepCount, keepFraction, minScore");
  if (o.keepCount && *o.keepCount < 0) {
    return opRejected(who, invalid, "keepCount %lld is negative", static_cast<long long>(*o.keepCount));
  }
  if (o.keepFraction && !(*o.keepFraction >= 0.0 && *o.keepFraction <= 1.0)) {
    return opRejected(who, invalid, "keepFraction must be in [0, 1]");
  }
  if (o.minScore && !std::isfinite(*o.minScore)) return opRejected(who, invalid, "minScore must be finite");
  if (o.score != PruneOptions::Sum && o.score != PruneOptions::Max) return opRejected(who, invalid, "score must be Sum or Max");
  // max SH degree 0: colours do not change a weight
  return viewListParams(who, o.views, SPZ_AMD_PRUNE_MAX_VIEWS, {o.nearPlane, o.coord, nullptr, 0, ", coord valid"}, params);
}
}  // namespace

bool pruneSpz(const uint8_t *data, int32_t size, const PruneOptions &o, std::vector<uint8_t> *out, int64_t *kept,
              std::vector<uint8_t> *keepMask, std::vector<uint64_t> *weightSum, std::vector<float> *weightMax) {
  const char *who = "pruneSpz";
  g_last_status = SPZ_AMD_OK;
  if (keepMask) keepMask->clear();
  if (weightSum) weightSum->clear();
  if (weightMax) weightMax->clear();
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  std::vector<spz_amd_render_params> params;
  if (!pruneOptionsOk(o, &params)) return false;
  Laps laps(who, "SPZ_AMD_PRUNE_TIMING");
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  laps.lap("inflate");
  const uint64_t n = static_cast<uint64_t>(d.numPoints);
  if (o.keepCount && static_cast<uint64_t>(*o.keepCount) > n) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "keepCount %lld is above the %llu points",
                      static_cast<long long>(*o.keepCount), static_cast<unsigned long long>(n));
  }
  const spz_amd_header hdr = headerOf(d);
  std::vector<uint8_t> mask;
  std::vector<uint64_t> sums;
  std::vector<float> maxima;
  if (keepMask) detail::resizeUninitialized(&mask, static_cast<size_t>(n));
  if (weightSum) detail::resizeUninitialized(&sums, static_cast<size_t>(n));
  if (weightMax) detail::resizeUninitialized(&maxima, static_cast<size_t>(n));
  const int rule = o.keepCount ? SPZ_AMD_PRUNE_KEEP_COUNT : o.keepFraction ? SPZ_AMD_PRUNE_KEEP_FRACTION
                                                                           : SPZ_AMD_PRUNE_MIN_SCORE;
  const double value = o.keepCount ? static_cast<double>(*o.keepCount) : o.keepFraction ? *o.keepFraction : *o.minScore;
  OpenResult r(spz_amd_prune_fetch, spz_amd_prune_device_data, spz_amd_prune_close);
  uint64_t bytes = 0, count = 0;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  int32_t bad = -1;
  const int rc = spz_amd_prune_open(d.stream, d.streamBytes, &hdr, params.data(), static_cast<int>(params.size()),
                                    static_cast<int>(o.score), rule, value, d.device, &r.ctx, &bytes, &count,
                                    keepMask ? mask.data() : nullptr, weightSum ? sums.data() : nullptr,
                                    weightMax ? maxima.data() : nullptr, ms, &bad);
  if (viewsFailed(who, rc, bad)) return false;
  laps.stage("score", ms[0], (" (" + std::to_string(params.size()) + " views)").c_str());
  laps.stage("rank", ms[1]);
  laps.stage("subset", ms[2]);
  laps.lap("prune");
  d.release();
  if (!r.finish(who, bytes, &laps, out)) return false;
  if (kept) *kept = static_cast<int64_t>(count);
  if (keepMask) keepMask->swap(mask);
  if (weightSum) weightSum->swap(sums);
  if (weightMax) weightMax->swap(maxima);
  return true;
}

bool pruneSpz(const std::string &inputFilename, const std::string &outputFilename, const PruneOptions &o,
              int64_t *kept, std::vector<uint8_t> *keepMask, std::vector<uint64_t> *weightSum,
              std::vector<float> *weightMax) {
  g_last_status = SPZ_AMD_OK;
  if (keepMask) keepMask->clear();
  if (weightSum) weightSum->clear();
  if (weightMax) weightMax->clear();
  std::vector<spz_amd_render_params> params;
  if (!pruneOptionsOk(o, &params)) return false;
  std::vector<uint8_t> mask;
  std::vector<uint64_t> sums;
  std::vector<float> maxima;
  int64_t count = 0;
  if (!fileToFile("pruneSpz", "SPZ_AMD_PRUNE_TIMING", inputFilename, outputFilename,
                  [&](const uint8_t *data, int32_t size, std::vector<uint8_t> *file) {
                    return pruneSpz(data, size, o, file, &count, keepMask ? &mask : nullptr, weightSum ? &sums : nullptr,
                                    weightMax ? &maxima : nullptr);
                  })) {
    return false;
  }
  if (kept) *kept = count;
  if (keepMask) keepMask->swap(mask);
  if (weightSum) weightSum->swap(sums);
  if (weightMax) weightMax->swap(maxima);
  return true;
}

std::vector<PruneOptions::View> orbitViews(int n, const std::array<float, 3> &center, float radius, int width,
                                           int height, float fovY, float distanceFactor) {
  if (n < 1 || n > SPZ_AMD_PRUNE_MAX_VIEWS) throw std::invalid_argument("orbitViews: n must be in 1..1024");
  if (width < 1 || width > 16384 || height < 1 || height > 16384) {
    throw std::invalid_argument("orbitViews: width and height must be in 1..16384");
  }
  if (!(fovY > 0.0f && fovY < 180.0f)) throw std::invalid_argument("orbitViews: fovY must be in (0, 180) degrees");
  if (!std::isfinite(radius) || !(radius > 0.0f) || !std::isfinite(distanceFactor) || !(distanceFactor > 0.0f)) {
    throw std::invalid_argument("orbitViews: radius and distanceFactor must be finite and > 0");
  }
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(center[k])) throw std::invalid_argument("orbitViews: center must be finite");
  }
  const double pi = 3.14159265358979323846;
  const double golden = pi * (3.0 - std::sqrt(5.0));
  const double dist = static_cast<double>(radius) * distanceFactor;
  const double f = 0.5 * height / std::tan(0.5 * fovY * pi / 180.0);
  std::vector<PruneOptions::View> out(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) {
    const double y = 1.0 - 2.0 * (i + 0.5) / n;
    const double r = std::sqrt(std::max(0.0, 1.0 - y * y));
    const double phi = golden * i;
    const double dir[3] = {r * std::cos(phi), y, r * std::sin(phi)};
    std::array<float, 3> eye;
    for (int k = 0; k < 3; ++k) eye[k] = static_cast<float>(center[k] + dist * dir[k]);
    const std::array<float, 3> up = std::fabs(y) > 0.999 ? std::array<float, 3>{0.0f, 0.0f, 1.0f}
                                                         : std::array<float, 3>{0.0f, 1.0f, 0.0f};
    PruneOptions::View &v = out[static_cast<size_t>(i)];
    v.worldToCamera = lookAt(eye, center, up);
    v.fx = v.fy = static_cast<float>(f);
    v.cx = 0.5f * width;
    v.cy = 0.5f * height;
    v.width = width;
    v.height = height;
  }
  return out;
}

bool boundingSphere(const std::vector<float> &positions, std::array<float, 3> *center, float *radius) {
  double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (size_t i = 0; i + 2 < positions.size(); i += 3) {
    if (!std::isfinite(positions[i]) || !std::isfinite(positions[i + 1]) || !std::isfinite(positions[i + 2])) continue;
    for (int k = 0; k < 3; ++k) {
      lo[k] = std::min(lo[k], static_cast<double>(positions[i + k]));
      hi[k] = std::max(hi[k], static_cast<double>(positions[i + k]));
    }
  }
  if (!(lo[0] <= hi[0])) return false;
  double d2 = 0.0;
  for (int k = 0; k < 3; ++k) {
    (*center)[k] = static_cast<float>(0.5 * (lo[k] + hi[k]));
    d2 += (hi[k] - lo[k]) * (hi[k] - lo[k]);
  }
  *radius = static_cast<float>(std::max(0.5 * std::sqrt(d2), 1e-6));
  return true;
}

std::vector<PruneOptions::View> loadViewsFile(const std::string &filename) {
  std::ifstream in(filename);
  if (!in) throw std::invalid_argument("loadViewsFile: unable to open " + filename);
  std::vector<PruneOptions::View> views;
  std::string line;
  int lineNo = 0;
  while (std::getline(in, line)) {
    ++lineNo;
    const size_t hash = line.find('#');
    if (hash != std::string::npos) line.resize(hash);
    std::istringstream ss(line);
    std::vector<std::string> tok;
    std::string t;
    while (ss >> t) tok.push_back(t);
    if (tok.empty()) continue;
    const std::string at = "loadViewsFile: " + filename + " line " + std::to_string(lineNo) + ": ";
    if (tok.size() != 18) {
      throw std::invalid_argument(at + "expected 18 values (width height fx fy cx cy and the 3x4 [R | t]), got " +
                                  std::to_string(tok.size()));
    }
    double v[18];
    for (int k = 0; k < 18; ++k) {
      char *end = nullptr;
      v[k] = std::strtod(tok[k].c_str(), &end);
      if (end == tok[k].c_str() || *end != '\0' || !std::isfinite(v[k])) {
        throw std::invalid_argument(at + "'" + tok[k] + "' is not a finite number");
      }
    }
    PruneOptions::View w;
    for (int k = 0; k < 2; ++k) {
      if (v[k] != std::floor(v[k]) || v[k] < 1.0 || v[k] > 16384.0) {
        throw std::invalid_argument(at + "width and height must be integers in 1..16384");
      }
    }
    w.width = static_cast<int>(v[0]);
    w.height = static_cast<int>(v[1]);
    w.fx = static_cast<float>(v[2]);
    w.fy = static_cast<float>(v[3]);
    w.cx = static_cast<float>(v[4]);
    w.cy = static_cast<float>(v[5]);
    for (int k = 0; k < 12; ++k) w.worldToCamera[k] = static_cast<float>(v[6 + k]);
    views.push_back(w);
  }
  if (views.empty()) throw std::invalid_argument("loadViewsFile: " + filename + " holds no view");
  return views;
}

// ---- compare -----------------------------------------------------------------------------------------------------
namespace {
// The views as render params with the options' frame, near plane, background and degree.
bool compareOptionsOk(const CompareOptions &o, std::vector<spz_amd_render_params> *params) {
  return viewListParams("compareSpz", o.views, SPZ_AMD_COMPARE_MAX_VIEWS,
                        {o.nearPlane, o.coord, &o.background, o.maxShDegree, ", maxShDegree 0..3, coord valid"}, params);
}

ImageMetrics toMetrics(const spz_amd_image_metrics &m) {
  ImageMetrics r;
  r.mse = m.mse;
  r.psnr = m.psnr;
  r.ssim = m.ssim;
  r.l1 = m.l1;
  r.maxAbs = m.max_abs;
  return r;
}
}  // namespace

bool compareSpz(const uint8_t *dataA, int32_t sizeA, const uint8_t *dataB, int32_t sizeB, const CompareOptions &o,
                std::vector<ImageMetrics> *metrics, std::vector<std::vector<float>> *ssimMaps) {
  const char *who = "compareSpz";
  g_last_status = SPZ_AMD_OK;
  if (ssimMaps) ssimMaps->clear();
  if (metrics == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  metrics->clear();
  std::vector<spz_amd_render_params> params;
  if (!compareOptionsOk(o, &params)) return false;
  Laps laps(who, "SPZ_AMD_COMPARE_TIMING");
  DevicePackedGaussians da, db;
  if (!loadInput(who, dataA, sizeA, &da) || !loadInput(who, dataB, sizeB, &db)) return false;
  laps.lap("inflate");
  if (da.device != db.device) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "the inputs were loaded on different devices");
  const spz_amd_header ha = headerOf(da), hb = headerOf(db);
  const size_t nv = params.size();
  std::vector<spz_amd_image_metrics> m(nv);
  std::vector<float> maps;
  if (ssimMaps) {
    size_t floats = 0;
    for (const spz_amd_render_params &p : params) floats += static_cast<size_t>(p.width) * p.height;
    detail::resizeUninitialized(&maps, floats);
  }
  std::vector<uint64_t> entries(2 * nv);
  float ms[2] = {0.0f, 0.0f};
  int32_t bad = -1;
  const int rc = spz_amd_compare_host(da.stream, da.streamBytes, &ha, db.stream, db.streamBytes, &hb, params.data(),
                                      static_cast<int>(nv), da.device, m.data(), ssimMaps ? maps.data() : nullptr,
                                      entries.data(), ms, &bad);
  if (viewsFailed(who, rc, bad)) return false;
  uint64_t ea = 0, eb = 0;
  for (size_t v = 0; v < nv; ++v) {
    ea += entries[2 * v];
    eb += entries[2 * v + 1];
  }
  laps.stage("render", ms[0], (" (" + std::to_string(nv) + " views; entries " + std::to_string(ea) + " + " +
                               std::to_string(eb) + ")").c_str());
  laps.stage("metrics", ms[1]);
  laps.lap("compare");
  metrics->resize(nv);
  for (size_t v = 0; v < nv; ++v) (*metrics)[v] = toMetrics(m[v]);
  if (ssimMaps) {
    ssimMaps->resize(nv);
    size_t at = 0;
    for (size_t v = 0; v < nv; ++v) {
      const size_t px = static_cast<size_t>(params[v].width) * params[v].height;
      (*ssimMaps)[v].assign(maps.begin() + static_cast<std::ptrdiff_t>(at),
                            maps.begin() + static_cast<std::ptrdiff_t>(at + px));
      at += px;
    }
  }
  return true;
}

bool compareSpz(const std::string &fileA, const std::string &fileB, const CompareOptions &o,
                std::vector<ImageMetrics> *metrics, std::vector<std::vector<float>> *ssimMaps) {
  const char *who = "compareSpz";
  g_last_status = SPZ_AMD_OK;
  if (ssimMaps) ssimMaps->clear();
  if (metrics == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  metrics->clear();
  std::vector<spz_amd_render_params> params;
  if (!compareOptionsOk(o, &params)) return false;
  std::vector<uint8_t> a, b;
  if (!readInput(who, fileA, &a) || !readInput(who, fileB, &b)) return false;
  return compareSpz(a.data(), static_cast<int32_t>(a.size()), b.data(), static_cast<int32_t>(b.size()), o, metrics,
                    ssimMaps);
}

// ---- refine ------------------------------------------------------------------------------------------------------
namespace {
// The views as render params, and the options but the position rate as the C ABI's.
bool refineOptionsOk(const RefineOptions &o, std::vector<spz_amd_render_params> *params, spz_amd_refine_options *c,
                     spz_amd_densify_options *d, const char *who = "refineSpz") {
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  if (o.iterations < 0) return opRejected(who, invalid, "iterations %d is negative", o.iterations);
  if (!(o.lambdaDssim >= 0.0 && o.lambdaDssim <= 1.0)) return opRejected(who, invalid, "lambdaDssim must be in [0, 1]");
  if (o.train == 0 || o.train > RefineOptions::All) return opRejected(who, invalid, "train must name at least one array");
  spz_amd_refine_default_options(c);
  c->iterations = o.iterations;
  c->train_mask = o.train;
  c->lambda_dssim = o.lambdaDssim;
  c->lr[0] = o.positionLr ? *o.positionLr : 0.0;
  c->lr[1] = o.scaleLr;
  c->lr[2] = o.rotationLr;
  c->lr[3] = o.alphaLr;
  c->lr[4] = o.colorLr;
  c->lr[5] = o.shLr;
  c->beta1 = o.beta1;
  c->beta2 = o.beta2;
  c->eps = o.eps;
  if (spz_amd_refine_check(c) != SPZ_AMD_OK) {
    return opRejected(who, invalid, "learning rates must be finite and >= 0, beta1 and beta2 in [0, 1), eps finite and >= 0");
  }
  spz_amd_densify_default_options(d);
  const DensifyOptions &dn = o.densify;
  d->interval = dn.interval;
  d->from_iter = dn.fromIter;
  d->until_iter = dn.untilIter;
  d->opacity_reset_interval = dn.opacityResetInterval;
  d->grad_threshold = dn.gradThreshold;
  d->percent_dense = dn.percentDense;
  d->extent = dn.extent;
  d->min_opacity = dn.minOpacity;
  d->max_scale = dn.maxScale;
  d->max_points = dn.maxPoints;
  d->seed = dn.seed;
  if (spz_amd_densify_check(d) != SPZ_AMD_OK) {
    return opRejected(who, invalid, "densify: values must be finite and >= 0, untilIter >= fromIter, minOpacity in (0, 1), "
                      "percentDense > 0 when interval > 0");
  }
  if (dn.interval > 0) {
    if ((o.train & 3u) != 3u) return opRejected(who, invalid, "densify needs positions and scales among the trained arrays");
    if (dn.opacityResetInterval > 0 && (o.train & 8u) == 0u) {
      return opRejected(who, invalid, "the opacity reset needs alphas among the trained arrays");
    }
  }
  return viewListParams(who, o.views, SPZ_AMD_REFINE_MAX_VIEWS,
                        {o.nearPlane, o.coord, &o.background, o.maxShDegree, ", maxShDegree 0..3, coord valid"}, params);
}

// What refineSpz and refineSpzToImages do around their open entries: the options as the C ABI's, the position rate
// from the scene's extent, the densify pre-check, the host-side result arrays, and after the entry the messages, the
// stage laps and the RefineReport.
struct RefineCall {
  const char *who;
  const RefineOptions &o;
  std::vector<spz_amd_render_params> params;
  spz_amd_refine_options c;
  spz_amd_densify_options d;
  std::vector<spz_amd_image_metrics> before, after;
  std::vector<double> history;
  std::vector<spz_amd_densify_round> rounds;
  OpenResult r{spz_amd_refine_fetch, spz_amd_refine_device_data, spz_amd_refine_close};
  uint64_t bytes = 0, skipped = 0, numPoints = 0;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  int32_t bad = -1;
  int numRounds = 0;

  RefineCall(const char *name, const RefineOptions &options) : who(name), o(options) {}
  bool densify() const { return d.interval > 0; }
  int views() const { return static_cast<int>(params.size()); }

  // 3DGS scales the position rate by the scene's extent.
  void positionRate(const DevicePackedGaussians &scene, Laps *laps) {
    if (o.positionLr) return;
    UnpackOptions u;
    u.to = o.coord;
    const GaussianCloud t = scene.unpack(u);
    std::array<float, 3> centre;
    float radius = 1.0f;
    if (!boundingSphere(t.positions, &centre, &radius)) radius = 1.0f;
    c.lr[0] = 1.6e-4 * static_cast<double>(radius);
    laps->lap("extent");
  }

  // With densify: the views give an extent, and the cloud may grow to `cap` points, not below the input's.
  bool densifyFits(const spz_amd_header &ha, uint64_t cap) const {
    if (!densify()) return true;
    spz_amd_densify_limits lim;
    if (spz_amd_densify_thresholds(&d, params.data(), views(), &lim) != SPZ_AMD_OK) {
      return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "densify: the views' camera centres coincide, so they give no "
                        "extent: set densify.extent");
    }
    if (cap < ha.num_points) {
      return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "densify: maxPoints %llu is below the input's %u points",
                        static_cast<unsigned long long>(cap), ha.num_points);
    }
    return true;
  }

  void allocate(const spz_amd_header &ha) {
    before.resize(params.size());
    after.resize(params.size());
    history.resize(static_cast<size_t>(o.iterations) + 1);
    rounds.resize(densify() ? static_cast<size_t>(o.iterations / d.interval) + 1 : 0);
    numPoints = ha.num_points;
  }

  // What the entry answered: its refusals as messages, then its three stages (the first is `firstStage`).
  bool opened(int rc, const spz_amd_header &ha, const char *firstStage, Laps *laps) const {
    if (rc == SPZ_AMD_ERR_UNSUPPORTED) {
      return opRejected(who, rc, "the encoder writes versions 2 and 3 and positions at 12 fractional bits: the input has "
                        "version %u and %u", ha.version, static_cast<unsigned>(ha.fractional_bits));
    }
    if (viewsFailed(who, rc, bad)) return false;
    laps->stage(firstStage, ms[0], (" (" + std::to_string(params.size()) + " views)").c_str());
    laps->stage("iterations", ms[1], (" (" + std::to_string(o.iterations) + ")").c_str());
    laps->stage("after", ms[2]);
    laps->lap("refine");
    return true;
  }

  // The output file's image, and the report.  The caller has released the inputs' device memory.
  bool finish(Laps *laps, std::vector<uint8_t> *out, RefineReport *report) {
    if (!r.finish(who, bytes, laps, out)) return false;
    if (report == nullptr) return true;
    history.resize(static_cast<size_t>(o.iterations));
    report->history.swap(history);
    for (const spz_amd_image_metrics &m : before) report->before.push_back(toMetrics(m));
    for (const spz_amd_image_metrics &m : after) report->after.push_back(toMetrics(m));
    report->skipped = skipped;
    report->positionLr = c.lr[0];
    for (int k = 0; k < 3; ++k) report->ms[k] = ms[k];
    report->numPoints = numPoints;
    for (int k = 0; k < numRounds && static_cast<size_t>(k) < rounds.size(); ++k) {
      const spz_amd_densify_round &x = rounds[static_cast<size_t>(k)];
      report->rounds.push_back(DensifyRound{x.iteration, x.cloned, x.split, x.culled, x.refused, x.num_points});
    }
    return true;
  }
};
}  // namespace

bool refineSpz(const uint8_t *data, int32_t size, const uint8_t *target, int32_t targetSize, const RefineOptions &o,
               std::vector<uint8_t> *out, RefineReport *report) {
  const char *who = "refineSpz";
  g_last_status = SPZ_AMD_OK;
  if (report) *report = RefineReport{};
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  RefineCall call(who, o);
  if (!refineOptionsOk(o, &call.params, &call.c, &call.d)) return false;
  Laps laps(who, "SPZ_AMD_REFINE_TIMING");
  DevicePackedGaussians da, db;
  if (!loadInput(who, data, size, &da) || !loadInput(who, target, targetSize, &db)) return false;
  laps.lap("inflate");
  if (da.device != db.device) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "the inputs were loaded on different devices");
  call.positionRate(db, &laps);
  const spz_amd_header ha = headerOf(da), hb = headerOf(db);
  if (!call.densifyFits(ha, call.d.max_points ? call.d.max_points : hb.num_points)) return false;
  call.allocate(ha);
  const int rc = call.densify()
      ? spz_amd_refine_densify_open(da.stream, da.streamBytes, &ha, db.stream, db.streamBytes, &hb, call.params.data(),
                                    call.views(), &call.c, &call.d, da.device, &call.r.ctx, &call.bytes,
                                    call.history.data(), call.before.data(), call.after.data(), &call.skipped, call.ms,
                                    &call.bad, &call.numPoints, call.rounds.data(),
                                    static_cast<int>(call.rounds.size()), &call.numRounds, nullptr)
      : spz_amd_refine_open(da.stream, da.streamBytes, &ha, db.stream, db.streamBytes, &hb, call.params.data(),
                            call.views(), &call.c, da.device, &call.r.ctx, &call.bytes, call.history.data(),
                            call.before.data(), call.after.data(), &call.skipped, call.ms, &call.bad);
  if (!call.opened(rc, ha, "targets", &laps)) return false;
  da.release();
  db.release();
  return call.finish(&laps, out, report);
}


bool refineSpz(const std::vector<uint8_t> &data, const std::vector<uint8_t> &target, const RefineOptions &o,
               std::vector<uint8_t> *out, RefineReport *report) {
  if (data.size() > static_cast<size_t>(INT32_MAX) || target.size() > static_cast<size_t>(INT32_MAX)) {
    return opRejected("refineSpz", SPZ_AMD_ERR_INVALID_ARG, "an input is larger than 2 GiB");
  }
  return refineSpz(data.data(), static_cast<int32_t>(data.size()), target.data(), static_cast<int32_t>(target.size()), o,
                   out, report);
}

bool refineSpz(const std::string &inputFilename, const std::string &targetFilename, const std::string &outputFilename,
               const RefineOptions &o, RefineReport *report) {
  const char *who = "refineSpz";
  g_last_status = SPZ_AMD_OK;
  if (report) *report = RefineReport{};
  std::vector<spz_amd_render_params> params;
  spz_amd_refine_options c;
  spz_amd_densify_options d;
  if (!refineOptionsOk(o, &params, &c, &d)) return false;
  std::vector<uint8_t> target;
  if (!readInput(who, targetFilename, &target)) return false;
  RefineReport rep;
  if (!fileToFile(who, "SPZ_AMD_REFINE_TIMING", inputFilename, outputFilename,
                  [&](const uint8_t *data, int32_t size, std::vector<uint8_t> *file) {
                    return refineSpz(data, size, target.data(), static_cast<int32_t>(target.size()), o, file, &rep);
                  })) {
    return false;
  }
  if (report) *report = std::move(rep);
  return true;
}

// ---- fit ---------------------------------------------------------------------------------------------------------
namespace {
// One image per view, each of its view's size, one channel count; the options as the C ABI's.
bool photoOptionsOk(const char *who, const RefineOptions &o, const PhotoOptions &p, spz_amd_photo_options *c,
                    spz_amd_depth_options *z) {
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  if (p.images.size() != o.views.size()) {
    return opRejected(who, invalid, "%zu views but %zu images", o.views.size(), p.images.size());
  }
  for (size_t v = 0; v < p.images.size(); ++v) {
    const PhotoImage &im = p.images[v];
    if (im.pixels == nullptr) return opRejected(who, invalid, "image %zu has no pixels", v);
    if (im.channels != 3 && im.channels != 4) return opRejected(who, invalid, "image %zu has %d channels: 3 or 4", v, im.channels);
    if (im.channels != p.images[0].channels) {
      return opRejected(who, invalid, "image %zu has %d channels but image 0 has %d", v, im.channels, p.images[0].channels);
    }
    if (im.width != o.views[v].width || im.height != o.views[v].height) {
      return opRejected(who, invalid, "view %zu is %d x %d but its image is %d x %d", v, o.views[v].width,
                        o.views[v].height, im.width, im.height);
    }
  }
  spz_amd_photo_default_options(c);
  c->fit_exposure = p.fitExposure ? 1 : 0;
  c->lr_exposure = p.exposureLr;
  if (spz_amd_photo_check(c) != SPZ_AMD_OK) return opRejected(who, invalid, "exposureLr must be finite and >= 0");
  spz_amd_depth_default_options(z);
  z->weight = p.depthWeight;
  z->min_alpha = p.depthMinAlpha;
  z->kind = p.depthKind == PhotoOptions::InverseL1 ? SPZ_AMD_DEPTH_INVERSE_L1 : SPZ_AMD_DEPTH_L1;
  if (p.depthKind != PhotoOptions::L1 && p.depthKind != PhotoOptions::InverseL1) {
    return opRejected(who, invalid, "depthKind must be L1 or InverseL1");
  }
  if (spz_amd_depth_check(z) != SPZ_AMD_OK) {
    return opRejected(who, invalid, "depthWeight must be finite and >= 0 and depthMinAlpha in (0, 1]");
  }
  return true;
}
}  // namespace

bool refineSpzToImages(const uint8_t *data, int32_t size, const RefineOptions &o, const PhotoOptions &p,
                       std::vector<uint8_t> *out, PhotoReport *report) {
  const char *who = "refineSpzToImages";
  g_last_status = SPZ_AMD_OK;
  if (report) *report = PhotoReport{};
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  RefineCall call(who, o);
  spz_amd_photo_options pc;
  spz_amd_depth_options zc;
  if (!refineOptionsOk(o, &call.params, &call.c, &call.d, who) || !photoOptionsOk(who, o, p, &pc, &zc)) return false;
  if (call.densify() && call.d.max_points == 0) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "densify: there is no target to take a count from: set densify.maxPoints");
  }
  Laps laps(who, "SPZ_AMD_REFINE_TIMING");
  DevicePackedGaussians da;
  if (!loadInput(who, data, size, &da)) return false;
  laps.lap("inflate");
  call.positionRate(da, &laps);
  const spz_amd_header ha = headerOf(da);
  if (!call.densifyFits(ha, call.d.max_points)) return false;
  const size_t nv = call.params.size();
  std::vector<const float *> targets(nv), weights(nv), depths(nv);
  bool anyWeights = false, anyDepth = false;
  for (size_t v = 0; v < nv; ++v) {
    targets[v] = p.images[v].pixels;
    weights[v] = p.images[v].weights;
    depths[v] = p.images[v].depth;
    anyWeights = anyWeights || weights[v] != nullptr;
    anyDepth = anyDepth || depths[v] != nullptr;
  }
  std::vector<double> depthHistory(anyDepth ? static_cast<size_t>(o.iterations) + 1 : 0), depthError(anyDepth ? 2 * nv : 0);
  std::vector<double> exposures(12 * nv);
  call.allocate(ha);
  const spz_amd_densify_options *dn = call.densify() ? &call.d : nullptr;
  const int nr = static_cast<int>(call.rounds.size());
  const int rc =
      anyDepth ? spz_amd_refine_images_depth_host_open(
                     da.stream, da.streamBytes, &ha, call.params.data(), call.views(), targets.data(),
                     p.images[0].channels, anyWeights ? weights.data() : nullptr, depths.data(), &zc, &call.c, &pc, dn,
                     da.device, &call.r.ctx, &call.bytes, call.history.data(), call.before.data(), call.after.data(),
                     &call.skipped, call.ms, &call.bad, &call.numPoints, call.rounds.data(), nr, &call.numRounds, nullptr,
                     exposures.data(), depthHistory.data(), depthError.data())
               : spz_amd_refine_images_host_open(
                     da.stream, da.streamBytes, &ha, call.params.data(), call.views(), targets.data(),
                     p.images[0].channels, anyWeights ? weights.data() : nullptr, &call.c, &pc, dn, da.device,
                     &call.r.ctx, &call.bytes, call.history.data(), call.before.data(), call.after.data(), &call.skipped,
                     call.ms, &call.bad, &call.numPoints, call.rounds.data(), nr, &call.numRounds, nullptr,
                     exposures.data());
  if (!call.opened(rc, ha, "before", &laps)) return false;
  da.release();
  if (!call.finish(&laps, out, report ? &report->refine : nullptr)) return false;
  if (report) {  // on top of the RefineReport: the exposures and, with a depth map, the depth losses
    report->exposures.resize(nv);
    for (size_t v = 0; v < nv; ++v) {
      std::copy(exposures.begin() + 12 * v, exposures.begin() + 12 * (v + 1), report->exposures[v].begin());
    }
    if (anyDepth) {
      depthHistory.resize(static_cast<size_t>(o.iterations));
      report->depthHistory.swap(depthHistory);
      report->depthError.resize(nv);
      for (size_t v = 0; v < nv; ++v) report->depthError[v] = {depthError[2 * v], depthError[2 * v + 1]};
    }
  }
  return true;
}

bool refineSpzToImages(const std::vector<uint8_t> &data, const RefineOptions &o, const PhotoOptions &p,
                       std::vector<uint8_t> *out, PhotoReport *report) {
  if (data.size() > static_cast<size_t>(INT32_MAX)) {
    return opRejected("refineSpzToImages", SPZ_AMD_ERR_INVALID_ARG, "the input is larger than 2 GiB");
  }
  return refineSpzToImages(data.data(), static_cast<int32_t>(data.size()), o, p, out, report);
}

bool refineSpzToImages(const std::string &inputFilename, const std::string &outputFilename, const RefineOptions &o,
                       const PhotoOptions &p, PhotoReport *report) {
  const char *who = "refineSpzToImages";
  g_last_status = SPZ_AMD_OK;
  if (report) *report = PhotoReport{};
  std::vector<spz_amd_render_params> params;
  spz_amd_refine_options c;
  spz_amd_densify_options d;
  spz_amd_photo_options pc;
  spz_amd_depth_options zc;
  if (!refineOptionsOk(o, &params, &c, &d, who) || !photoOptionsOk(who, o, p, &pc, &zc)) return false;
  PhotoReport rep;
  if (!fileToFile(who, "SPZ_AMD_REFINE_TIMING", inputFilename, outputFilename,
                  [&](const uint8_t *data, int32_t size, std::vector<uint8_t> *file) {
                    return refineSpzToImages(data, size, o, p, file, &rep);
                  })) {
    return false;
  }
  if (report) *report = std::move(rep);
  return true;
}

// ---- locate ------------------------------------------------------------------------------------------------------
namespace {
// The initial view as render params, and the options but the translation's rate as the C ABI's.
bool locateOptionsOk(const PruneOptions::View &initial, const float *image, int channels, const LocateOptions &o,
                     spz_amd_render_params *p, spz_amd_locate_options *c) {
  const char *who = "locateSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  if (image == nullptr) return opRejected(who, invalid, "no image");
  if (channels != 3 && channels != 4) return opRejected(who, invalid, "channels %d: give 3 or 4", channels);
  if (o.iterations < 0) return opRejected(who, invalid, "iterations %d is negative", o.iterations);
  if (o.levels < 1 || o.levels > SPZ_AMD_LOCATE_MAX_LEVELS) {
    return opRejected(who, invalid, "levels %d is outside 1..%d", o.levels, SPZ_AMD_LOCATE_MAX_LEVELS);
  }
  if (!(o.lambdaDssim >= 0.0 && o.lambdaDssim <= 1.0)) return opRejected(who, invalid, "lambdaDssim must be in [0, 1]");
  spz_amd_locate_default_options(c);
  c->iterations = o.iterations;
  c->levels = o.levels;
  c->lambda_dssim = o.lambdaDssim;
  c->lr_rotation = o.rotationLr;
  c->lr_translation = o.translationLr ? *o.translationLr : 0.0;
  c->lr_final_factor = o.lrFinalFactor;
  c->beta1 = o.beta1;
  c->beta2 = o.beta2;
  c->eps = o.eps;
  if (spz_amd_locate_check(c) != SPZ_AMD_OK) {
    return opRejected(who, invalid, "step sizes must be finite and >= 0, lrFinalFactor in (0, 1], beta1 and beta2 in "
                      "[0, 1), eps finite and >= 0");
  }
  if (!viewParams(who, "", initial, {o.nearPlane, o.coord, &o.background, o.maxShDegree, ", maxShDegree 0..3, coord valid"},
                  p)) {
    return false;
  }
  const int f = 1 << (o.levels - 1);
  if (initial.width % f != 0 || initial.height % f != 0) {
    return opRejected(who, invalid, "image size %d x %d is not divisible by %d (levels %d)", initial.width, initial.height,
                      f, o.levels);
  }
  return true;
}
}  // namespace

bool locateSpz(const uint8_t *data, int32_t size, const PruneOptions::View &initial, const float *image, int channels,
               const LocateOptions &o, LocateReport *report) {
  const char *who = "locateSpz";
  g_last_status = SPZ_AMD_OK;
  if (report == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no report");
  *report = LocateReport{};
  spz_amd_render_params p;
  spz_amd_locate_options c;
  if (!locateOptionsOk(initial, image, channels, o, &p, &c)) return false;
  Laps laps(who, "SPZ_AMD_LOCATE_TIMING");
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  laps.lap("inflate");
  if (!o.translationLr) {  // a step of the rotation's size, seen from the scene's centre
    UnpackOptions u;
    u.to = o.coord;
    const GaussianCloud g = d.unpack(u);
    std::array<float, 3> centre = {0.0f, 0.0f, 0.0f};
    float radius = 1.0f;
    if (!boundingSphere(g.positions, &centre, &radius)) radius = 1.0f;
    const float *m = p.world_to_camera;
    double dist2 = 0.0;
    for (int k = 0; k < 3; ++k) {  // the camera centre is -R^T t
      const double eye = -(static_cast<double>(m[k]) * m[3] + static_cast<double>(m[4 + k]) * m[7] +
                           static_cast<double>(m[8 + k]) * m[11]);
      dist2 += (eye - centre[static_cast<size_t>(k)]) * (eye - centre[static_cast<size_t>(k)]);
    }
    c.lr_translation = o.rotationLr * std::max(std::sqrt(dist2), static_cast<double>(radius));
    laps.lap("extent");
  }
  const spz_amd_header h = headerOf(d);
  std::vector<double> history(static_cast<size_t>(o.iterations) + 1);
  spz_amd_image_metrics before, after;
  std::array<float, 12> pose{};
  int32_t ran = 0;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  const int rc = spz_amd_locate_image_host(d.stream, d.streamBytes, &h, &p, image, channels, &c, d.device, pose.data(),
                                           history.data(), &before, &after, &ran, ms);
  if (rc == SPZ_AMD_ERR_CAPACITY) return opRejected(who, rc, "more than 2^31 - 1 tile entries");
  if (deviceFailed(rc, who)) return false;
  laps.stage("before", ms[0]);
  laps.stage("iterations", ms[1], (" (" + std::to_string(ran) + ")").c_str());
  laps.stage("after", ms[2]);
  laps.lap("locate");
  report->view = initial;
  report->view.worldToCamera = pose;
  history.resize(static_cast<size_t>(ran));
  report->history.swap(history);
  report->before = toMetrics(before);
  report->after = toMetrics(after);
  report->iterations = ran;
  report->translationLr = c.lr_translation;
  for (int k = 0; k < 3; ++k) report->ms[k] = ms[k];
  return true;
}

bool locateSpz(const std::vector<uint8_t> &data, const PruneOptions::View &initial, const float *image, int channels,
               const LocateOptions &o, LocateReport *report) {
  if (data.size() > static_cast<size_t>(INT32_MAX)) {
    return opRejected("locateSpz", SPZ_AMD_ERR_INVALID_ARG, "the input is larger than 2 GiB");
  }
  return locateSpz(data.data(), static_cast<int32_t>(data.size()), initial, image, channels, o, report);
}

bool locateSpz(const std::string &filename, const PruneOptions::View &initial, const float *image, int channels,
               const LocateOptions &o, LocateReport *report) {
  const char *who = "locateSpz";
  g_last_status = SPZ_AMD_OK;
  if (report == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no report");
  *report = LocateReport{};
  spz_amd_render_params p;
  spz_amd_locate_options c;
  if (!locateOptionsOk(initial, image, channels, o, &p, &c)) return false;
  std::vector<uint8_t> data;
  if (!readInput(who, filename, &data)) return false;
  return locateSpz(data, initial, image, channels, o, report);
}

namespace {
// loadImageFile (depth false: P6 or PF, three channels out) and loadDepthFile (depth true: Pf, or the first channel of a
// PF; one channel out).
void loadPixelFile(const char *who, bool depth, const std::string &filename, std::vector<float> *pixels, int *width,
                   int *height) {
  auto bad = [&](const char *why) { return std::invalid_argument(std::string(who) + ": " + filename + ": " + why); };
  if (pixels == nullptr || width == nullptr || height == nullptr) throw bad("no output");
  std::ifstream f(filename, std::ios::binary);
  if (!f) throw bad("unable to open");
  // the header: a magic, then width, height and maxval (PPM) or scale (PFM), separated by white space, '#' comments
  auto token = [&]() {
    std::string t;
    int ch = f.get();
    while (ch != EOF) {
      if (ch == '#') {
        while (ch != EOF && ch != '\n') ch = f.get();
      } else if (!std::isspace(ch)) {
        break;
      }
      ch = f.get();
    }
    for (; ch != EOF && !std::isspace(ch); ch = f.get()) t.push_back(static_cast<char>(ch));
    return t;  // the one white-space character after the token is consumed
  };
  const std::string magic = token();
  if (depth) {
    if (magic != "Pf" && magic != "PF") throw bad("neither a one-channel PFM (Pf) nor a colour PFM (PF)");
  } else if (magic != "P6" && magic != "PF") {
    throw bad("neither a binary PPM (P6) nor a colour PFM (PF)");
  }
  const size_t in_ch = magic == "Pf" ? 1u : 3u, out_ch = depth ? 1u : 3u;  // of a PF a depth map is the first channel
  char *end = nullptr;
  const std::string ws = token(), hs = token(), last = token();
  const long w = std::strtol(ws.c_str(), &end, 10);
  if (ws.empty() || *end != '\0' || w < 1 || w > 16384) throw bad("bad width");
  const long h = std::strtol(hs.c_str(), &end, 10);
  if (hs.empty() || *end != '\0' || h < 1 || h > 16384) throw bad("bad height");
  const size_t count = static_cast<size_t>(w) * static_cast<size_t>(h) * in_ch;
  pixels->assign(static_cast<size_t>(w) * static_cast<size_t>(h) * out_ch, 0.0f);
  if (magic == "P6") {
    if (last != "255") throw bad("maxval must be 255");
    std::vector<uint8_t> raw(count);
    if (!f.read(reinterpret_cast<char *>(raw.data()), static_cast<std::streamsize>(count))) throw bad("short file");
    for (size_t k = 0; k < count; ++k) (*pixels)[k] = static_cast<float>(raw[k]) / 255.0f;
  } else {
    const double scale = std::strtod(last.c_str(), &end);
    if (last.empty() || *end != '\0' || !std::isfinite(scale) || scale == 0.0) throw bad("bad scale");
    std::vector<uint8_t> raw(count * 4u);
    if (!f.read(reinterpret_cast<char *>(raw.data()), static_cast<std::streamsize>(raw.size()))) throw bad("short file");
    const bool little = scale < 0.0;
    const size_t row = static_cast<size_t>(w) * out_ch;
    for (size_t y = 0; y < static_cast<size_t>(h); ++y) {
      // the file's rows run bottom to top
      const uint8_t *src = raw.data() + (static_cast<size_t>(h) - 1u - y) * static_cast<size_t>(w) * in_ch * 4u;
      for (size_t k = 0; k < row; ++k) {
        const uint8_t *b = src + 4u * (k / out_ch * in_ch + k % out_ch);
        const uint32_t bits = little ? (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24)
                                     : (uint32_t)b[3] | ((uint32_t)b[2] << 8) | ((uint32_t)b[1] << 16) | ((uint32_t)b[0] << 24);
        float v;
        std::memcpy(&v, &bits, 4);
        (*pixels)[y * row + k] = v;
      }
    }
  }
  *width = static_cast<int>(w);
  *height = static_cast<int>(h);
}
}  // namespace

void loadImageFile(const std::string &filename, std::vector<float> *pixels, int *width, int *height) {
  loadPixelFile("loadImageFile", false, filename, pixels, width, height);
}

void loadDepthFile(const std::string &filename, std::vector<float> *pixels, int *width, int *height) {
  loadPixelFile("loadDepthFile", true, filename, pixels, width, height);
}

// ---- mesh --------------------------------------------------------------------------------------------------------
namespace {
bool meshOptionsOk(const MeshOptions &o, spz_amd_mesh_options *c, std::vector<spz_amd_render_params> *params) {
  const char *who = "meshSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  spz_amd_mesh_default_options(c);
  if (o.voxelSize && o.resolution) return opRejected(who, invalid, "set at most one of voxelSize and resolution");
  if (o.voxelSize) {
    if (!(*o.voxelSize > 0.0) || !std::isfinite(*o.voxelSize)) return opRejected(who, invalid, "voxelSize must be finite and > 0");
    c->voxel_size = *o.voxelSize;
    c->resolution = 0;
  }
  if (o.resolution) {
    if (*o.resolution < 1 || *o.resolution > 2046) return opRejected(who, invalid, "resolution %d is outside 1..2046", *o.resolution);
    c->resolution = *o.resolution;
  }
  if (o.truncation) {
    if (!(*o.truncation > 0.0) || !std::isfinite(*o.truncation)) return opRejected(who, invalid, "truncation must be finite and > 0");
    c->truncation = *o.truncation;
  }
  if (o.box) {
    c->has_box = 1;
    for (int k = 0; k < 6; ++k) c->box[k] = (*o.box)[k];
  }
  c->depth_kind = static_cast<int32_t>(o.depth);
  c->min_alpha = o.minAlpha;
  c->min_weight = o.minWeight;
  if (spz_amd_mesh_check(c) != SPZ_AMD_OK) {
    return opRejected(who, invalid,
                      "bad options: box finite with x1 > x0, y1 > y0, z1 > z0; depth Median or Expected; minAlpha in [0, 1]; "
                      "minWeight finite and > 0");
  }
  return viewListParams(who, o.views, SPZ_AMD_MESH_MAX_VIEWS, {o.nearPlane, o.coord, nullptr, 3, ", coord valid"}, params);
}
}  // namespace

bool meshSpz(const uint8_t *data, int32_t size, const MeshOptions &o, TriangleMesh *mesh) {
  const char *who = "meshSpz";
  g_last_status = SPZ_AMD_OK;
  if (mesh == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output mesh");
  spz_amd_mesh_options c;
  std::vector<spz_amd_render_params> params;
  if (!meshOptionsOk(o, &c, &params)) return false;
  Laps laps(who, "SPZ_AMD_MESH_TIMING");
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  laps.lap("inflate");
  const spz_amd_header hdr = headerOf(d);
  void *ctx = nullptr;
  uint64_t counts[2] = {0, 0};
  spz_amd_tsdf_volume vol = {};
  float ms[3] = {0.0f, 0.0f, 0.0f};
  int32_t bad = -1;
  const int rc = spz_amd_mesh_open(d.stream, d.streamBytes, &hdr, params.data(), static_cast<int>(params.size()), &c,
                                   d.device, &ctx, counts, &vol, ms, &bad);
  if (rc == SPZ_AMD_ERR_INVALID_ARG && bad < 0) {
    return opRejected(who, rc, "no volume: the file has no finite position, the box is empty, or the lattice would "
                               "have a side above 2048 points or more than 2^28 points");
  }
  if (viewsFailed(who, rc, bad)) return false;
  laps.stage("render", ms[0], (" (" + std::to_string(params.size()) + " views)").c_str());
  laps.stage("fuse", ms[1]);
  laps.stage("extract", ms[2]);
  d.release();
  TriangleMesh m;
  detail::resizeUninitialized(&m.vertices, static_cast<size_t>(counts[0]) * 3u);
  detail::resizeUninitialized(&m.colors, static_cast<size_t>(counts[0]) * 3u);
  m.triangles.resize(static_cast<size_t>(counts[1]) * 3u);
  const int frc = spz_amd_mesh_fetch(ctx, m.vertices.data(), m.colors.data(), m.triangles.data());
  spz_amd_mesh_close(ctx);
  if (deviceFailed(frc, who)) return false;
  laps.lap("fetch");
  for (int k = 0; k < 3; ++k) {
    m.lo[k] = vol.lo[k];
    m.dims[k] = vol.dims[k];
    m.ms[k] = ms[k];
  }
  m.voxelSize = vol.voxel_size;
  m.truncation = vol.truncation;
  *mesh = std::move(m);
  return true;
}

bool meshSpz(const std::string &filename, const MeshOptions &o, TriangleMesh *mesh) {
  g_last_status = SPZ_AMD_OK;
  if (mesh == nullptr) return opRejected("meshSpz", SPZ_AMD_ERR_INVALID_ARG, "no output mesh");
  spz_amd_mesh_options c;
  std::vector<spz_amd_render_params> params;
  if (!meshOptionsOk(o, &c, &params)) return false;
  std::vector<uint8_t> data;
  if (!readInput("meshSpz", filename, &data)) return false;
  return meshSpz(data.data(), static_cast<int32_t>(data.size()), o, mesh);
}

// ---- seed --------------------------------------------------------------------------------------------------------
namespace {
// Everything that needs no device: the options, the views, and the images against the views.
bool seedOptionsOk(const SeedOptions &o, const std::vector<PhotoImage> &images, spz_amd_seed_options *c,
                   std::vector<spz_amd_render_params> *params) {
  const char *who = "seedSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  spz_amd_seed_default_options(c);
  if (o.stride < 1 || o.stride > 64) return opRejected(who, invalid, "stride %d is outside 1..64", o.stride);
  if (!(o.opacity > 0.0 && o.opacity < 1.0)) return opRejected(who, invalid, "opacity must be in (0, 1)");
  if (o.shDegree < 0 || o.shDegree > 3) return opRejected(who, invalid, "shDegree %d is outside 0..3", o.shDegree);
  if (o.maxPoints > SPZ_AMD_REFERENCE_MAX_POINTS) {
    return opRejected(who, invalid, "maxPoints %llu: the reference reads at most %u points",
                      static_cast<unsigned long long>(o.maxPoints), SPZ_AMD_REFERENCE_MAX_POINTS);
  }
  c->stride = static_cast<uint32_t>(o.stride);
  c->scale_factor = static_cast<float>(o.scaleFactor);
  c->alpha = static_cast<float>(std::log(o.opacity / (1.0 - o.opacity)));
  c->cover_alpha = o.coverAlpha;
  c->cover_tolerance = o.coverTolerance;
  c->cover = o.cover ? 1 : 0;
  c->sh_degree = o.shDegree;
  if (spz_amd_seed_check(c) != SPZ_AMD_OK) {
    return opRejected(who, invalid, "bad options: scaleFactor finite and > 0, coverAlpha in [0, 1], coverTolerance "
                                    "finite and >= 0");
  }
  if (!viewListParams(who, o.views, SPZ_AMD_SEED_MAX_VIEWS, {o.nearPlane, o.coord, nullptr, o.shDegree, ", coord valid"},
                      params)) {
    return false;
  }
  if (images.size() != o.views.size()) {
    return opRejected(who, invalid, "%zu views but %zu images", o.views.size(), images.size());
  }
  for (size_t v = 0; v < images.size(); ++v) {
    const PhotoImage &im = images[v];
    if (im.pixels == nullptr) return opRejected(who, invalid, "image %zu has no pixels", v);
    if (im.channels != 3 && im.channels != 4) return opRejected(who, invalid, "image %zu has %d channels: 3 or 4", v, im.channels);
    if (im.depth == nullptr) return opRejected(who, invalid, "image %zu has no depth", v);
    if (im.width != o.views[v].width || im.height != o.views[v].height) {
      return opRejected(who, invalid, "view %zu is %d x %d but its image is %d x %d", v, o.views[v].width,
                        o.views[v].height, im.width, im.height);
    }
  }
  return true;
}
}  // namespace

bool seedSpz(const SeedOptions &o, const std::vector<PhotoImage> &images, std::vector<uint8_t> *out, SeedReport *report) {
  const char *who = "seedSpz";
  g_last_status = SPZ_AMD_OK;
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no output vector");
  spz_amd_seed_options c;
  std::vector<spz_amd_render_params> params;
  if (!seedOptionsOk(o, images, &c, &params)) return false;
  Laps laps(who, "SPZ_AMD_SEED_TIMING");
  DevicePackedGaussians d;
  std::vector<uint8_t> baseFile;
  const bool onto = o.base.has_value() || !o.baseData.empty();
  if (onto) {
    const std::vector<uint8_t> *file = &o.baseData;
    if (o.base) {
      if (!readInput(who, *o.base, &baseFile)) return false;
      file = &baseFile;
    }
    if (file->size() > static_cast<size_t>(INT32_MAX)) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "the base is larger than 2 GiB");
    if (!loadInput(who, file->data(), static_cast<int32_t>(file->size()), &d)) return false;
    laps.lap("inflate");
    if (d.shDegree != o.shDegree) {
      return opRejected(who, SPZ_AMD_ERR_SH_DEGREE, "the base has shDegree %d and the seed %d: they must be equal (filterSpz "
                                                    "lowers a file's)", d.shDegree, o.shDegree);
    }
  }
  const spz_amd_header hdr = onto ? headerOf(d) : spz_amd_header{};
  const size_t nv = images.size();
  std::vector<const float *> pix(nv), dep(nv), wts(nv);
  std::vector<int32_t> ch(nv);
  for (size_t v = 0; v < nv; ++v) {
    pix[v] = images[v].pixels;
    dep[v] = images[v].depth;
    wts[v] = images[v].weights;
    ch[v] = images[v].channels;
  }
  std::vector<uint64_t> counts(3u * nv, 0);
  OpenResult r(spz_amd_seed_fetch, spz_amd_seed_device_data, spz_amd_seed_close);
  uint64_t bytes = 0, added = 0;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  int32_t bad = -1;
  const int rc = spz_amd_seed_open(params.data(), static_cast<int>(nv), &c, pix.data(), ch.data(), dep.data(), wts.data(),
                                   onto ? d.stream : nullptr, onto ? d.streamBytes : 0, onto ? &hdr : nullptr, o.maxPoints,
                                   onto ? d.device : deviceIndex(), &r.ctx, &bytes, counts.data(), &added, ms, &bad);
  if (viewsFailed(who, rc, bad)) return false;
  laps.stage("cover", ms[0], (" (" + std::to_string(nv) + " views)").c_str());
  laps.stage("seed", ms[1]);
  laps.stage("encode", ms[2]);
  if (onto) d.release();
  if (!r.finish(who, bytes, &laps, out)) return false;
  if (report) {
    SeedReport rep;
    rep.views.resize(nv);
    for (size_t v = 0; v < nv; ++v) rep.views[v] = {counts[3u * v], counts[3u * v + 1u], counts[3u * v + 2u]};
    rep.numPoints = added;
    for (int k = 0; k < 3; ++k) rep.ms[k] = ms[k];
    *report = std::move(rep);
  }
  return true;
}

bool seedSpz(const SeedOptions &o, const std::vector<PhotoImage> &images, const std::string &outputFilename,
             SeedReport *report) {
  const char *who = "seedSpz";
  std::vector<uint8_t> file;
  SeedReport rep;
  if (!seedSpz(o, images, &file, &rep)) return false;
  Laps laps(who, "SPZ_AMD_SEED_TIMING");
  if (!writeOutput(who, outputFilename, file)) return false;
  laps.lap("write");
  if (report) *report = std::move(rep);
  return true;
}

bool saveMeshPly(const std::string &filename, const float *vertices, const float *colors, size_t numVertices,
                 const uint32_t *triangles, size_t numTriangles) {
  const char *who = "saveMeshPly";
  g_last_status = SPZ_AMD_OK;
  if ((numVertices && (vertices == nullptr || colors == nullptr)) || (numTriangles && triangles == nullptr)) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "an array is missing");
  }
  if (numVertices > 0xffffffffull) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "more than 2^32 - 1 vertices");
  for (size_t k = 0; k < numTriangles * 3u; ++k) {
    if (triangles[k] >= numVertices) {
      return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "triangle %zu names vertex %u of %zu", k / 3u, triangles[k], numVertices);
    }
  }
  const std::string head = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(numVertices) +
                           "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\nproperty uchar green\n"
                           "property uchar blue\nelement face " + std::to_string(numTriangles) +
                           "\nproperty list uchar uint vertex_indices\nend_header\n";
  std::vector<uint8_t> bytes(head.size() + numVertices * 15u + numTriangles * 13u);
  std::memcpy(bytes.data(), head.data(), head.size());
  uint8_t *at = bytes.data() + head.size();
  for (size_t v = 0; v < numVertices; ++v) {
    std::memcpy(at, vertices + 3u * v, 12);  // little-endian hosts only, like the .ply writer of the clouds
    for (int k = 0; k < 3; ++k) {
      const float c = colors[3u * v + static_cast<size_t>(k)];
      const float clamped = c >= 0.0f ? (c <= 1.0f ? c : 1.0f) : 0.0f;  // NaN -> 0
      at[12 + k] = static_cast<uint8_t>(std::rint(255.0f * clamped));
    }
    at += 15;
  }
  for (size_t t = 0; t < numTriangles; ++t) {
    *at = 3;
    std::memcpy(at + 1, triangles + 3u * t, 12);
    at += 13;
  }
  return writeOutput(who, filename, bytes);
}

bool saveMeshPly(const std::string &filename, const TriangleMesh &m) {
  if (m.vertices.size() % 3u != 0 || m.colors.size() != m.vertices.size() || m.triangles.size() % 3u != 0) {
    g_last_status = SPZ_AMD_OK;
    return opRejected("saveMeshPly", SPZ_AMD_ERR_INVALID_ARG, "the mesh's arrays do not match");
  }
  return saveMeshPly(filename, m.vertices.data(), m.colors.data(), m.vertices.size() / 3u, m.triangles.data(),
                     m.triangles.size() / 3u);
}

// ---- align -------------------------------------------------------------------------------------------------------
namespace {
bool alignOptionsOk(const AlignOptions &o, spz_amd_align_options *c) {
  spz_amd_align_default_options(c);
  for (int k = 0; k < 4; ++k) c->rotation[k] = o.rotation[k];
  for (int k = 0; k < 3; ++k) c->translation[k] = o.translation[k];
  c->scale = o.scale;
  c->coord = static_cast<int32_t>(o.coord);
  c->estimate_scale = o.estimateScale ? 1 : 0;
  c->overlap = o.overlap;
  c->has_max_distance = o.maxDistance ? 1 : 0;
  c->max_distance = o.maxDistance ? *o.maxDistance : 0.0;
  c->stride = o.stride;
  c->max_iterations = o.maxIterations;
  c->init_centroids = o.initCentroids ? 1 : 0;
  c->relative_fitness = o.relativeFitness;
  c->relative_rmse = o.relativeRmse;
  if (spz_amd_align_check(c) == SPZ_AMD_OK) return true;
  return opRejected("alignSpz", SPZ_AMD_ERR_INVALID_ARG,
                    "bad options: stride >= 1, overlap in (0, 1], maxDistance > 0, maxIterations 1..1000, tolerances "
                    ">= 0, a nonzero rotation, scale > 0, coord valid, all finite");
}
}  // namespace

bool alignSpz(const uint8_t *source, int32_t sourceSize, const uint8_t *target, int32_t targetSize,
              const AlignOptions &o, AlignResult *result) {
  const char *who = "alignSpz";
  g_last_status = SPZ_AMD_OK;
  if (result == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no result");
  *result = AlignResult{};
  spz_amd_align_options c;
  if (!alignOptionsOk(o, &c)) return false;
  Laps laps(who, "SPZ_AMD_ALIGN_TIMING");
  DevicePackedGaussians ds, dt;
  if (!loadInput(who, source, sourceSize, &ds) || !loadInput(who, target, targetSize, &dt)) return false;
  laps.lap("inflate");
  if (ds.device != dt.device) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "the inputs were loaded on different devices");
  const spz_amd_align_cloud cs = {ds.stream, ds.streamBytes, headerOf(ds)}, ct = {dt.stream, dt.streamBytes, headerOf(dt)};
  if (cs.hdr.version == 1 || ct.hdr.version == 1) {
    return opRejected(who, SPZ_AMD_ERR_UNSUPPORTED, "a version 1 file has float16 positions (transformSpz with the identity writes a v3 copy)");
  }
  if (ct.hdr.num_points == 0) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "the target has no points");
  spz_amd_align_result r;
  std::vector<spz_amd_align_history> hist(c.max_iterations);
  float ms[3] = {0.0f, 0.0f, 0.0f};
  const int rc = spz_amd_align_host(&cs, &ct, &c, ds.device, &r, hist.data(), c.max_iterations, ms);
  if (deviceFailed(rc, who)) return false;
  laps.stage("prepare", ms[0]);
  laps.stage("query", ms[1], (" (" + std::to_string(r.iterations) + " steps)").c_str());
  laps.stage("solve", ms[2]);
  laps.lap("align");
  for (int k = 0; k < 4; ++k) result->rotation[k] = r.rotation[k];
  for (int k = 0; k < 3; ++k) result->translation[k] = r.translation[k];
  result->scale = r.scale;
  result->fitness = r.fitness;
  result->inlierRmse = r.inlier_rmse;
  result->inliers = r.inliers;
  result->iterations = r.iterations;
  result->converged = r.converged != 0;
  result->degenerate = r.degenerate != 0;
  for (uint32_t k = 0; k < r.iterations; ++k) {
    result->history.push_back({hist[k].fitness, hist[k].inlier_rmse, hist[k].inliers});
  }
  return true;
}

bool alignSpz(const std::string &sourceFilename, const std::string &targetFilename, const AlignOptions &o,
              AlignResult *result) {
  const char *who = "alignSpz";
  g_last_status = SPZ_AMD_OK;
  if (result == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no result");
  *result = AlignResult{};
  spz_amd_align_options c;
  if (!alignOptionsOk(o, &c)) return false;
  std::vector<uint8_t> a, b;
  if (!readInput(who, sourceFilename, &a) || !readInput(who, targetFilename, &b)) return false;
  return alignSpz(a.data(), static_cast<int32_t>(a.size()), b.data(), static_cast<int32_t>(b.size()), o, result);
}

// ---- level -------------------------------------------------------------------------------------------------------
namespace {
bool levelOptionsOk(const LevelOptions &o, spz_amd_plane_options *c) {
  const char *who = "levelSpz";
  spz_amd_plane_default_options(c);
  c->threshold = o.threshold;
  c->hypotheses = o.hypotheses;
  c->refine = o.refine;
  c->max_planes = o.planes;
  c->stride = o.stride;
  c->seed = o.seed;
  c->min_inliers = o.minInliers;
  c->has_axis = o.axis ? 1 : 0;
  c->has_up_hint = o.upHint ? 1 : 0;
  for (int k = 0; k < 3; ++k) {
    c->axis[k] = o.axis ? (*o.axis)[k] : 0.0;
    c->up_hint[k] = o.upHint ? (*o.upHint)[k] : 0.0;
  }
  c->max_tilt = o.maxTilt;
  c->coord = static_cast<int32_t>(o.coord);
  c->no_translate = o.noTranslate ? 1 : 0;
  if (std::isnan(o.threshold)) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "a threshold (world units) is required");
  if (!(o.minInlierFraction >= 0.0) || !(o.minInlierFraction <= 1.0)) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "minInlierFraction %g is outside 0 ... 1", o.minInlierFraction);
  }
  if (o.fractionalBits < 0 || o.fractionalBits > 24) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "fractionalBits %d is outside 0 ... 24", o.fractionalBits);
  }
  if (spz_amd_plane_check(c) == SPZ_AMD_OK) return true;
  return opRejected(who, SPZ_AMD_ERR_INVALID_ARG,
                    "bad options: threshold >= 0, hypotheses 1..65536, refine 0..16, planes 1..255, stride >= 1, a nonzero "
                    "axis and upHint, maxTilt 0..90, coord valid, all finite");
}
}  // namespace

bool detectPlanes(const DevicePackedGaussians &d, const LevelOptions &o, LevelResult *result) {
  const char *who = "levelSpz";
  g_last_status = SPZ_AMD_OK;
  if (result == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no result");
  *result = LevelResult{};
  spz_amd_plane_options c;
  if (!levelOptionsOk(o, &c)) return false;
  if (!d.valid()) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "the packed stream is empty");
  const spz_amd_header hdr = headerOf(d);
  if (hdr.version == 1) {
    return opRejected(who, SPZ_AMD_ERR_UNSUPPORTED, "a version 1 file has float16 positions (transformSpz with the identity writes a v3 copy)");
  }
  if (spz_amd_plane_threshold(o.threshold, static_cast<int>(hdr.fractional_bits), &result->threshold) != SPZ_AMD_OK) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "the threshold %g is too large at %u fractional bits", o.threshold,
                      static_cast<unsigned>(hdr.fractional_bits));
  }
  const uint64_t taking = (static_cast<uint64_t>(hdr.num_points) + o.stride - 1) / o.stride;
  const uint64_t floorCount = static_cast<uint64_t>(std::ceil(o.minInlierFraction * static_cast<double>(taking)));
  if (floorCount > c.min_inliers) c.min_inliers = floorCount;
  Laps laps(who, "SPZ_AMD_LEVEL_TIMING");
  std::vector<spz_amd_plane_result> found(c.max_planes);
  result->labels.assign(hdr.num_points, 0);
  uint32_t count = 0;
  float ms[3] = {0.0f, 0.0f, 0.0f};
  const int rc = spz_amd_plane_host(d.stream, d.streamBytes, &hdr, &c, d.device, found.data(), c.max_planes, &count,
                                    result->labels.data(), ms);
  if (deviceFailed(rc, who)) return false;
  laps.stage("prepare", ms[0]);
  laps.stage("score", ms[1]);
  laps.stage("refine", ms[2]);
  laps.lap("planes");
  result->prepareMs = ms[0];
  result->scoreMs = ms[1];
  result->refineMs = ms[2];
  for (uint32_t k = 0; k < count; ++k) {
    const spz_amd_plane_result &r = found[k];
    DetectedPlane p;
    p.normalInt = {r.plane.a, r.plane.b, r.plane.c};
    p.offsetInt = r.plane.e;
    p.inliers = r.inliers;
    p.sumAbs = r.sum_abs;
    p.points = r.points;
    p.above = r.above;
    p.below = r.below;
    p.bestHypothesis = r.best_hypothesis;
    p.refinements = r.refinements;
    p.fitness = r.fitness;
    p.meanDistance = r.mean_distance;
    p.offset = r.offset;
    for (int a = 0; a < 3; ++a) {
      p.normal[a] = r.normal[a];
      p.translation[a] = r.translation[a];
    }
    for (int a = 0; a < 4; ++a) p.rotation[a] = r.rotation[a];
    result->planes.push_back(p);
  }
  return true;
}

bool detectPlanes(const uint8_t *data, int32_t size, const LevelOptions &o, LevelResult *result) {
  const char *who = "levelSpz";
  g_last_status = SPZ_AMD_OK;
  if (result == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no result");
  *result = LevelResult{};
  spz_amd_plane_options c;
  if (!levelOptionsOk(o, &c)) return false;
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  return detectPlanes(d, o, result);
}

bool detectPlanes(const std::string &filename, const LevelOptions &o, LevelResult *result) {
  const char *who = "levelSpz";
  g_last_status = SPZ_AMD_OK;
  if (result == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no result");
  *result = LevelResult{};
  spz_amd_plane_options c;
  if (!levelOptionsOk(o, &c)) return false;
  std::vector<uint8_t> data;
  if (!readInput(who, filename, &data)) return false;
  return detectPlanes(data.data(), static_cast<int32_t>(data.size()), o, result);
}

bool levelSpz(const uint8_t *data, int32_t size, const LevelOptions &o, std::vector<uint8_t> *out, LevelResult *result) {
  const char *who = "levelSpz";
  g_last_status = SPZ_AMD_OK;
  if (result == nullptr || out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no result or no output vector");
  *result = LevelResult{};
  spz_amd_plane_options c;
  if (!levelOptionsOk(o, &c)) return false;
  DevicePackedGaussians d;
  if (!loadInput(who, data, size, &d)) return false;
  if (!detectPlanes(d, o, result)) return false;
  out->clear();
  if (result->planes.empty()) return true;  // no plane reaches the floor: no output
  const DetectedPlane &first = result->planes[0];
  if (o.select == LevelOptions::Select::None) {
    d.release();
    TransformOptions t;
    t.rotation = first.rotation;
    t.translation = first.translation;
    t.coord = o.coord;
    t.fractionalBits = o.fractionalBits;
    return transformSpz(data, size, t, out);
  }
  const spz_amd_header hdr = headerOf(d);
  const spz_amd_plane plane = {first.normalInt[0], first.normalInt[1], first.normalInt[2], 0, first.offsetInt};
  std::vector<uint8_t> side(hdr.num_points);
  const int rc = spz_amd_plane_sides_host(d.stream, d.streamBytes, &hdr, &plane, result->threshold, d.device, side.data());
  if (deviceFailed(rc, who)) return false;
  d.release();
  FilterOptions f;
  f.mask.emplace(side.size());
  for (size_t i = 0; i < side.size(); ++i) {
    bool keep = false;
    switch (o.select) {
      case LevelOptions::Select::Plane: keep = side[i] == 0; break;
      case LevelOptions::Select::OffPlane: keep = side[i] != 0; break;
      case LevelOptions::Select::Above: keep = side[i] == 1; break;
      case LevelOptions::Select::Below: keep = side[i] == 2; break;
      case LevelOptions::Select::None: break;
    }
    (*f.mask)[i] = keep ? 1 : 0;
  }
  int64_t kept = 0;
  if (!filterSpz(data, size, f, out, &kept)) return false;
  result->kept = kept;
  return true;
}

bool levelSpz(const std::string &inputFilename, const std::string &outputFilename, const LevelOptions &o,
              LevelResult *result) {
  g_last_status = SPZ_AMD_OK;
  if (result == nullptr) return opRejected("levelSpz", SPZ_AMD_ERR_INVALID_ARG, "no result");
  *result = LevelResult{};
  spz_amd_plane_options c;
  if (!levelOptionsOk(o, &c)) return false;
  const char *who = "levelSpz";
  std::vector<uint8_t> data, file;
  if (!readInput(who, inputFilename, &data)) return false;
  if (!levelSpz(data.data(), static_cast<int32_t>(data.size()), o, &file, result)) return false;
  if (result->planes.empty()) return true;  // nothing is written
  return writeOutput(who, outputFilename, file);
}

bool compareImages(const float *a, int channelsA, const float *b, int channelsB, int width, int height,
                   ImageMetrics *metrics, std::vector<float> *ssimMap) {
  const char *who = "compareImages";
  g_last_status = SPZ_AMD_OK;
  if (ssimMap) ssimMap->clear();
  if (a == nullptr || b == nullptr || metrics == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no image or no output");
  if (spz_amd_image_metrics_check(width, height, channelsA, channelsB) != SPZ_AMD_OK) {
    return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "%d x %d with %d and %d channels: sides 1..16384, channels 3 or 4",
                      width, height, channelsA, channelsB);
  }
  Laps laps(who, "SPZ_AMD_COMPARE_TIMING");
  std::vector<float> map;
  if (ssimMap) detail::resizeUninitialized(&map, static_cast<size_t>(width) * static_cast<size_t>(height));
  spz_amd_image_metrics m = {};
  const int rc = spz_amd_image_metrics_host(a, channelsA, b, channelsB, width, height, deviceIndex(), &m,
                                            ssimMap ? map.data() : nullptr);
  if (deviceFailed(rc, who)) return false;
  laps.lap("metrics");
  *metrics = toMetrics(m);
  if (ssimMap) ssimMap->swap(map);
  return true;
}

GaussianCloud loadSpz(const std::vector<uint8_t> &data, const UnpackOptions &o) {
  return loadSpz(data.data(), static_cast<int32_t>(data.size()), o);
}

GaussianCloud loadSpz(const std::string &filename, const UnpackOptions &o) {
  g_last_status = SPZ_AMD_OK;
  std::vector<uint8_t> data;
  if (!readFile(filename, &data, /*log=*/true)) return {};
  return loadSpz(data, o);
}

// ---- tile --------------------------------------------------------------------------------------------------------
namespace {
const char *const kCoordNames[9] = {"UNSPECIFIED", "LDB", "RDB", "LUB", "RUB", "LDF", "RDF", "LUF", "RUF"};

// Axis a of the stored RUB frame is negated in `coord` (enum - 1: bit 0 = R, bit 1 = U, bit 2 = F; UNSPECIFIED: none).
bool axisFlipped(CoordinateSystem coord, int a) {
  const int c = static_cast<int>(coord) - 1;
  if (c < 0) return false;
  return ((c >> a) & 1) != (((static_cast<int>(CoordinateSystem::RUB) - 1) >> a) & 1);
}

void jsonFloat(std::string *o, float v) {
  if (std::isnan(v)) {
    *o += "null";
    return;
  }
  char b[40];
  std::snprintf(b, sizeof(b), "%.9g", static_cast<double>(v));
  *o += b;
}

// A reader for the JSON tileset.json holds: objects, arrays, numbers, strings without escapes, null.
struct JsonIn {
  const char *p, *e;
  bool ok = true;
  void ws() {
    while (p < e && (*p == ' ' || *p == '\n' || *p == '\r' || *p == '\t')) ++p;
  }
  bool eat(char c) {
    ws();
    if (p < e && *p == c) {
      ++p;
      return true;
    }
    return false;
  }
  bool need(char c) {
    if (!eat(c)) ok = false;
    return ok;
  }
  std::string str() {
    std::string r;
    if (!need('"')) return r;
    while (p < e && *p != '"') r += *p++;
    need('"');
    return r;
  }
  double num() {   // null: NaN
    ws();
    if (e - p >= 4 && std::strncmp(p, "null", 4) == 0) {
      p += 4;
      return std::nan("");
    }
    char *end = nullptr;
    const std::string t(p, std::min<size_t>(static_cast<size_t>(e - p), 64));
    const double v = std::strtod(t.c_str(), &end);
    if (end == t.c_str()) ok = false;
    p += end - t.c_str();
    return v;
  }
  template <class F>
  void array(F each) {
    if (!need('[')) return;
    if (eat(']')) return;
    do each(); while (ok && eat(','));
    need(']');
  }
  template <class F>
  void object(F field) {   // field(key): reads the value
    if (!need('{')) return;
    if (eat('}')) return;
    do {
      const std::string k = str();
      if (!need(':')) return;
      field(k);
    } while (ok && eat(','));
    need('}');
  }
};
}  // namespace

bool saveTileset(const Tileset &t, const std::string &path) {
  std::string o = "{\"format\": \"spz-tileset\", \"version\": 1, \"coord\": \"";
  const int c = static_cast<int>(t.coord);
  o += kCoordNames[c < 0 || c > 8 ? 0 : c];
  o += "\", \"num_points\": " + std::to_string(t.numPoints) + ", \"sh_degree\": " + std::to_string(t.shDegree) +
       ", \"fractional_bits\": " + std::to_string(t.fractionalBits) + ", \"max_points\": " + std::to_string(t.maxPoints) +
       ", \"tiles\": [";
  for (size_t i = 0; i < t.tiles.size(); ++i) {
    const Tile &k = t.tiles[i];
    o += i ? ",\n  {" : "\n  {";
    o += "\"id\": " + std::to_string(k.id) + ", \"file\": \"" + k.file + "\", \"parent\": " + std::to_string(k.parent) +
         ", \"children\": [";
    for (size_t j = 0; j < k.children.size(); ++j) o += (j ? ", " : "") + std::to_string(k.children[j]);
    o += "], \"level\": " + std::to_string(k.level) + ", \"cell\": [" + std::to_string(k.cell[0]) + ", " +
         std::to_string(k.cell[1]) + ", " + std::to_string(k.cell[2]) + "], \"content_level\": " +
         std::to_string(k.contentLevel) + ", \"num_points\": " + std::to_string(k.numPoints) + ", \"geometric_error\": ";
    jsonFloat(&o, k.geometricError);
    o += ", \"box\": [[";
    for (int a = 0; a < 3; ++a) {
      if (a) o += ", ";
      jsonFloat(&o, k.boxMin[a]);
    }
    o += "], [";
    for (int a = 0; a < 3; ++a) {
      if (a) o += ", ";
      jsonFloat(&o, k.boxMax[a]);
    }
    o += "]], \"max_radius\": ";
    jsonFloat(&o, k.maxRadius);
    o += "}";
  }
  o += "\n]}\n";
  return writeFile(path, std::vector<uint8_t>(o.begin(), o.end()));
}

bool loadTileset(const std::string &path, Tileset *out) {
  const char *who = "loadTileset";
  g_last_status = SPZ_AMD_OK;
  if (out == nullptr) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "no tileset to fill");
  std::vector<uint8_t> data;
  if (!readFile(path, &data, /*log=*/true)) return false;
  Tileset t;
  std::string format;
  int version = 0;
  bool coordOk = false;
  JsonIn in{reinterpret_cast<const char *>(data.data()), reinterpret_cast<const char *>(data.data()) + data.size()};
  in.object([&](const std::string &k) {
    if (k == "format") format = in.str();
    else if (k == "version") version = static_cast<int>(in.num());
    else if (k == "coord") {
      const std::string c = in.str();
      for (int i = 0; i < 9; ++i) {
        if (c == kCoordNames[i]) {
          t.coord = static_cast<CoordinateSystem>(i);
          coordOk = true;
        }
      }
    } else if (k == "num_points") t.numPoints = static_cast<uint64_t>(in.num());
    else if (k == "sh_degree") t.shDegree = static_cast<int>(in.num());
    else if (k == "fractional_bits") t.fractionalBits = static_cast<int>(in.num());
    else if (k == "max_points") t.maxPoints = static_cast<uint32_t>(in.num());
    else if (k == "tiles") {
      in.array([&] {
        Tile tile;
        in.object([&](const std::string &f) {
          if (f == "id") tile.id = static_cast<uint32_t>(in.num());
          else if (f == "file") tile.file = in.str();
          else if (f == "parent") tile.parent = static_cast<int32_t>(in.num());
          else if (f == "children") in.array([&] { tile.children.push_back(static_cast<uint32_t>(in.num())); });
          else if (f == "level") tile.level = static_cast<int32_t>(in.num());
          else if (f == "cell") {
            int a = 0;
            in.array([&] {
              const double v = in.num();
              if (a < 3) tile.cell[a++] = static_cast<uint32_t>(v);
            });
          } else if (f == "content_level") tile.contentLevel = static_cast<int32_t>(in.num());
          else if (f == "num_points") tile.numPoints = static_cast<uint32_t>(in.num());
          else if (f == "geometric_error") tile.geometricError = static_cast<float>(in.num());
          else if (f == "box") {
            int row = 0;
            in.array([&] {
              int a = 0;
              in.array([&] {
                const float v = static_cast<float>(in.num());
                if (row < 2 && a < 3) (row ? tile.boxMax : tile.boxMin)[a] = v;
                ++a;
              });
              ++row;
            });
          } else if (f == "max_radius") tile.maxRadius = static_cast<float>(in.num());
          else in.ok = false;
        });
        t.tiles.push_back(std::move(tile));
      });
    } else in.ok = false;
  });
  in.ws();
  bool ok = in.ok && in.p == in.e && format == "spz-tileset" && version == 1 && coordOk && !t.tiles.empty();
  for (size_t i = 0; ok && i < t.tiles.size(); ++i) {
    const Tile &k = t.tiles[i];
    ok = k.id == i && k.parent >= -1 && k.parent < static_cast<int32_t>(i);
    for (const uint32_t c : k.children) ok = ok && c > i && c < t.tiles.size();
  }
  if (!ok) return opRejected(who, SPZ_AMD_ERR_INVALID_ARG, "%s is not a version 1 spz-tileset", path.c_str());
  *out = std::move(t);
  return true;
}

std::vector<uint32_t> selectTiles(const Tileset &t, const PruneOptions::View &view, double maxPixelError,
                                  double nearPlane) {
  std::vector<uint32_t> out;
  if (t.tiles.empty()) return out;
  const auto &m = view.worldToCamera;   // eye = -R^T t
  double eye[3];
  for (int a = 0; a < 3; ++a) {
    eye[a] = -(static_cast<double>(m[a]) * m[3] + static_cast<double>(m[4 + a]) * m[7] + static_cast<double>(m[8 + a]) * m[11]);
  }
  const double focal = std::max(static_cast<double>(view.fx), static_cast<double>(view.fy));
  std::vector<uint32_t> stack = {0};
  while (!stack.empty()) {
    const uint32_t i = stack.back();
    stack.pop_back();
    const Tile &k = t.tiles[i];
    if (!k.children.empty()) {
      double d2 = 0.0, diag2 = 0.0;
      for (int a = 0; a < 3; ++a) {
        const double lo = k.boxMin[a], hi = k.boxMax[a];
        const double c = (lo + hi) / 2.0 - eye[a];
        d2 += c * c;
        diag2 += (hi - lo) * (hi - lo);
      }
      const double radius = std::sqrt(diag2) / 2.0 + static_cast<double>(k.maxRadius);
      const double d = std::max(std::sqrt(d2) - radius, nearPlane);
      if (static_cast<double>(k.geometricError) * focal / d > maxPixelError) {
        for (size_t j = k.children.size(); j-- > 0;) stack.push_back(k.children[j]);
        continue;
      }
    }
    out.push_back(i);
  }
  std::sort(out.begin(), out.end());
  return out;
}

bool tileSpz(const std::string &inputFilename, const std::string &outDir, const TileOptions &o, Tileset *tileset) {
  const char *who = "tileSpz";
  const int invalid = SPZ_AMD_ERR_INVALID_ARG;
  g_last_status = SPZ_AMD_OK;
  if (o.maxPoints < 1 || o.maxPoints > SPZ_AMD_REFERENCE_MAX_POINTS) {
    return opRejected(who, invalid, "maxPoints %u is outside 1..%u", o.maxPoints, SPZ_AMD_REFERENCE_MAX_POINTS);
  }
  if (o.maxTiles < 1 || o.maxTiles > 0x7fffffffu) return opRejected(who, invalid, "maxTiles %u is outside 1..2^31 - 1", o.maxTiles);
  if (static_cast<int>(o.coord) < 0 || static_cast<int>(o.coord) > 8) return opRejected(who, invalid, "unknown coordinate system %d", static_cast<int>(o.coord));
  if (outDir.empty()) return opRejected(who, invalid, "no output directory");
  struct stat sb;
  const bool exists = ::stat(outDir.c_str(), &sb) == 0;
  if (exists) {
    if (!S_ISDIR(sb.st_mode)) return opRejected(who, invalid, "%s is not a directory", outDir.c_str());
    bool empty = true;
    if (DIR *dir = ::opendir(outDir.c_str())) {
      while (const dirent *e = ::readdir(dir)) {
        if (std::strcmp(e->d_name, ".") != 0 && std::strcmp(e->d_name, "..") != 0) empty = false;
      }
      ::closedir(dir);
    } else {
      empty = false;
    }
    if (!empty) return opRejected(who, invalid, "%s is not empty", outDir.c_str());
  }
  Laps laps(who, "SPZ_AMD_TILE_TIMING");
  std::vector<uint8_t> data;
  if (!readInput(who, inputFilename, &data)) return false;
  DevicePackedGaussians d;
  if (!loadInput(who, data.data(), static_cast<int32_t>(data.size()), &d)) return false;
  laps.lap("inflate");
  if (d.version == 1) {
    return opRejected(who, SPZ_AMD_ERR_UNSUPPORTED,
                      "a version 1 file has float16 positions and no integer cell; transformSpz with the "
                      "identity writes a v3 copy");
  }
  const spz_amd_header hdr = headerOf(d);
  void *ctx = nullptr;
  struct Closer {
    void **c;
    ~Closer() { spz_amd_tile_close(*c); }
  } closer{&ctx};
  uint64_t count = 0, arenaBytes = 0;
  float ms[4] = {0, 0, 0, 0};
  const int rc = spz_amd_tile_open(d.stream, d.streamBytes, &hdr, o.maxPoints, o.maxTiles, d.device, &ctx, &count,
                                   &arenaBytes, ms);
  if (rc == SPZ_AMD_ERR_CAPACITY) return opRejected(who, rc, "the tree has more than maxTiles = %u tiles", o.maxTiles);
  if (deviceFailed(rc, who)) return false;
  laps.stage("sort", ms[0]);
  laps.stage("tree", ms[1]);
  laps.stage("decimate", ms[2]);
  laps.stage("emit", ms[3]);
  laps.lap("tile");
  d.release();
  std::vector<spz_amd_tile_info> table(static_cast<size_t>(count));
  std::vector<uint8_t> arena;
  detail::resizeUninitialized(&arena, static_cast<size_t>(arenaBytes));
  if (deviceFailed(spz_amd_tile_table(ctx, table.data()), who)) return false;
  if (deviceFailed(spz_amd_tile_fetch_arena(ctx, arena.data()), who)) return false;
  spz_amd_tile_close(ctx);
  ctx = nullptr;
  laps.lap("download");
  Tileset t;
  t.coord = o.coord;
  t.numPoints = static_cast<uint64_t>(hdr.num_points);
  t.shDegree = hdr.sh_degree;
  t.fractionalBits = hdr.fractional_bits;
  t.maxPoints = o.maxPoints;
  t.tiles.resize(table.size());
  for (size_t i = 0; i < table.size(); ++i) {
    const spz_amd_tile_info &r = table[i];
    Tile &k = t.tiles[i];
    char name[32];
    std::snprintf(name, sizeof(name), "tile_%06u.spz", r.id);
    k.id = r.id;
    k.file = name;
    k.parent = r.parent;
    if (r.parent >= 0) t.tiles[static_cast<size_t>(r.parent)].children.push_back(r.id);
    k.level = r.level;
    k.cell = {r.cell[0], r.cell[1], r.cell[2]};
    k.contentLevel = r.content_level;
    k.numPoints = r.num_points;
    k.geometricError = r.geometric_error;
    k.maxRadius = r.max_radius;
    for (int a = 0; a < 3; ++a) {
      const bool f = axisFlipped(o.coord, a);
      k.boxMin[a] = f ? -r.box_max[a] : r.box_min[a];
      k.boxMax[a] = f ? -r.box_min[a] : r.box_max[a];
    }
  }
  // the container stage: thousands of small members must not pay the device writer's floor one after another, so
  // members under 1 MiB go to zlib on at most 16 threads; the few larger ones take compressGzipped's routes after them
  constexpr uint64_t kSmall = uint64_t(1) << 20;
  std::vector<std::vector<uint8_t>> files(table.size());
  std::atomic<size_t> next{0};
  std::atomic<bool> failed{false};
  const unsigned hw = std::thread::hardware_concurrency();
  size_t most = 16;   // SPZ_AMD_TILE_GZIP_THREADS = 1..16 lowers it (measurements)
  if (const char *e = std::getenv("SPZ_AMD_TILE_GZIP_THREADS")) {
    const int v = std::atoi(e);
    if (v >= 1 && v <= 16) most = static_cast<size_t>(v);
  }
  const size_t workers = std::max<size_t>(1, std::min<size_t>({most, hw ? hw : 1, table.size()}));
  auto work = [&] {
    for (size_t i = next.fetch_add(1); i < table.size(); i = next.fetch_add(1)) {
      if (table[i].bytes >= kSmall) continue;
      if (!compressGzippedZlib(arena.data() + table[i].offset, static_cast<size_t>(table[i].bytes), &files[i])) failed = true;
    }
  };
  std::vector<std::thread> pool;
  for (size_t w = 1; w < workers; ++w) pool.emplace_back(work);
  work();
  for (std::thread &th : pool) th.join();
  for (size_t i = 0; i < table.size() && !failed; ++i) {
    if (table[i].bytes < kSmall) continue;
    if (!compressGzipped(arena.data() + table[i].offset, static_cast<size_t>(table[i].bytes), &files[i])) failed = true;
  }
  if (failed) {
    logLine("[SPZ ERROR] %s: compressGzipped failed", who);
    return false;
  }
  laps.lap("gzip");
  if (!exists && ::mkdir(outDir.c_str(), 0777) != 0) return opRejected(who, invalid, "unable to create %s", outDir.c_str());
  for (size_t i = 0; i < table.size(); ++i) {
    if (!writeOutput(who, outDir + "/" + t.tiles[i].file, files[i])) return false;
  }
  if (!saveTileset(t, outDir + "/tileset.json")) {
    logLine("[SPZ ERROR] %s: unable to write %s/tileset.json", who, outDir.c_str());
    return false;
  }
  laps.lap("write");
  if (tileset) *tileset = std::move(t);
  return true;
}

}  // namespace spz
