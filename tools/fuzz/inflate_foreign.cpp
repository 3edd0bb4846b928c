// Sanitizer harness for the decoder source the host and device readers share (spz_inflate_core.hpp), over the members
// of tests/deflate_craft.py — valid deflate that zlib's writer never emits, and members that are invalid in one chosen
// way: `python tests/deflate_craft.py DIR` writes them, `inflate_foreign DIR/*.gz` reads each one three ways:
//   the parallel host reader (whatever it accepts, zlib must accept, with the same bytes);
//   the block decoder from the first bit to the final block (the device's chunk 0 does that when no start is found);
//   the block-start test of the device's search at every bit position of the first 256 KiB.
// Built with ASan + UBSan by `make fuzz-foreign`; must finish without a report.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../spz_amd/csrc/spz_inflate.hpp"
#include "../../spz_amd/csrc/spz_inflate_core.hpp"

static bool zlibInflate(const std::vector<uint8_t> &gz, std::vector<uint8_t> *out) {
  z_stream s = {};
  if (inflateInit2(&s, 16 + MAX_WBITS) != Z_OK) return false;
  out->assign(gz.size() * 40 + (64u << 20), 0);
  s.next_in = const_cast<Bytef *>(gz.data());
  s.avail_in = static_cast<uInt>(gz.size());
  s.next_out = out->data();
  s.avail_out = static_cast<uInt>(out->size());
  const int rc = inflate(&s, Z_FINISH);
  out->resize(s.total_out);
  inflateEnd(&s);
  return rc == Z_STREAM_END;
}

// RFC 1952 2.3; 0: not a header this reader starts behind
static size_t headerLength(const std::vector<uint8_t> &m) {
  if (m.size() < 18 || m[0] != 0x1f || m[1] != 0x8b || m[2] != 8 || (m[3] & 0xe0)) return 0;
  size_t pos = 10;
  if (m[3] & 4) pos += 2 + (m[10] | (m[11] << 8));
  for (int f = 8; f <= 16; f <<= 1) {
    if (m[3] & f) {
      while (pos < m.size() && m[pos] != 0) ++pos;
      ++pos;
    }
  }
  if (m[3] & 2) return 0;  // FHCRC: zlib checks it, the fast readers are not asked (parseGzipHeader, spz_host.cpp)
  return pos + 8 <= m.size() ? pos : 0;
}

int main(int argc, char **argv) {
  using namespace spz::pinflate;
  int accepted = 0, declined = 0, walked = 0;
  for (int a = 1; a < argc; ++a) {
    std::ifstream f(argv[a], std::ios::binary);
    const std::vector<uint8_t> m((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    const size_t h = headerLength(m);
    if (h == 0) continue;
    std::vector<uint8_t> got, want;
    const bool zok = zlibInflate(m, &want);
    if (inflate(m.data(), m.size(), h, 8, &got)) {
      ++accepted;
      if (!zok || want != got) {
        std::printf("inflate_foreign: %s: accepted what zlib does not\n", argv[a]);
        return 1;
      }
    } else {
      ++declined;
    }
    const size_t dbytes = m.size() - h - 8;
    const Bits in{m.data() + h, 8ull * dbytes, dbytes};
    static HuffLit lit;
    static HuffDist dist;
    NullSink sink;
    sink.n = 0;
    uint64_t end = 0;
    const Outcome r = decodeBlocks(in, 0, NONE, sink, &end, &lit, &dist);
    if (r == FINAL && ((end + 7) >> 3) == dbytes) {
      ++walked;
      if (!zok) std::printf("inflate_foreign: %s: the block decoder walks to the end of what zlib refuses (%llu bytes; the CRC-32 decides)\n", argv[a],
                            (unsigned long long)sink.n);
      else if (sink.n != want.size()) {
        std::printf("inflate_foreign: %s: %llu bytes, zlib %zu\n", argv[a], (unsigned long long)sink.n, want.size());
        return 1;
      }
    }
    static HeaderWork work;
    uint64_t starts = 0;
    for (uint64_t p = 0; p < in.nbits && p < (8ull * 262144); ++p) starts += hasValidDynamicHeader(in, p, &work) ? 1 : 0;
    std::printf("%-50s zlib %s  parallel reader %s  block walk %s  %llu header candidates\n", argv[a], zok ? "ok    " : "refuse", got.empty() ? "declined" : "accepted",
                r == FINAL ? "final " : "failed", (unsigned long long)starts);
  }
  std::printf("inflate_foreign: %d accepted (all equal to zlib), %d declined, %d walked to the final block\n", accepted, declined, walked);
  return 0;
}
