/*
 * spz_amd.h — C ABI of the MI355X-native SPZ pack/unpack path (libspz_amd.so).
 *
 * This is the drop-in boundary for the hot path of lanxinger/spz: everything a
 * binding of the reference's packGaussians / unpackGaussians / (de)serialize
 * step would need, as plain C: pointers, sizes, ints.  No C++ types, no torch
 * types, no exceptions, no caller-visible allocation.  Citations are to
 * /root/reference/src/cc (the interface each entry point replaces).
 *
 * Byte stream ("raw stream", pre-gzip), little-endian, load-spz.cc:131-139,533-546:
 *   16-byte header | positions | alphas | colors | scales | rotations | sh
 * gzip stays on the host (libspz_host.so, include/spz_amd_host.hpp).
 *
 * Float side: the six flat float32 arrays of GaussianCloud (splat-types.h:90-115):
 *   positions[3N] xyz, scales[3N], rotations[4N] xyzw, alphas[N], colors[3N],
 *   sh[N*shDim*3] laid out [point][coeff][rgb], shDim = 0,3,8,15.
 *
 * Memory spaces: *_device entry points take DEVICE pointers valid on the current
 * HIP device and enqueue on `hip_stream` (a hipStream_t passed as void*, NULL =
 * default stream) without synchronising.  *_host entry points take HOST pointers,
 * stage through device memory on `device`, and return when the result is in
 * host memory.  Every compute entry point fails with SPZ_AMD_ERR_NO_DEVICE when
 * no HIP device is usable: there is no CPU fallback in this library.
 *
 * Alignment: float arrays need 4-byte alignment; stream pointers need none.
 */
#ifndef SPZ_AMD_H_
#define SPZ_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPZ_AMD_ABI_VERSION 1

/* Status codes.  The header-validation codes mirror, one for one, the rejection
 * branches of deserializePackedGaussians (load-spz.cc:553-568,591-594). */
enum {
  SPZ_AMD_OK = 0,
  SPZ_AMD_ERR_INVALID_ARG = -1,     /* NULL pointer, bad degree/version/coord, checkSizes load-spz.cc:106-127 */
  SPZ_AMD_ERR_HEADER_NOT_FOUND = -2, /* short header or wrong magic, load-spz.cc:553-556 */
  SPZ_AMD_ERR_VERSION = -3,         /* version outside [1,3], load-spz.cc:557-560 */
  SPZ_AMD_ERR_TOO_MANY_POINTS = -4, /* numPoints > limit, load-spz.cc:561-564 */
  SPZ_AMD_ERR_SH_DEGREE = -5,       /* shDegree > 3, load-spz.cc:565-568 */
  SPZ_AMD_ERR_SHORT_STREAM = -6,    /* "read error", load-spz.cc:591-594 */
  SPZ_AMD_ERR_CAPACITY = -7,        /* output buffer too small */
  SPZ_AMD_ERR_NO_DEVICE = -8,       /* no usable HIP device / runtime */
  SPZ_AMD_ERR_HIP = -9,             /* a HIP call failed (see spz_amd_last_hip_error) */
  SPZ_AMD_ERR_UNSUPPORTED = -10,    /* e.g. encode of version 1; RCCL not loadable */
  SPZ_AMD_ERR_COMM = -11,           /* an RCCL call failed (see spz_amd_last_rccl_error) */
  SPZ_AMD_ERR_VERIFY = -12          /* a result failed the library's own check (container stage: symbols that do not
                                       reproduce their input, a member that does not inflate back to it) */
};

/* CoordinateSystem values, splat-types.h:24-34. */
enum {
  SPZ_AMD_UNSPECIFIED = 0, SPZ_AMD_LDB = 1, SPZ_AMD_RDB = 2, SPZ_AMD_LUB = 3, SPZ_AMD_RUB = 4,
  SPZ_AMD_LDF = 5, SPZ_AMD_RDF = 6, SPZ_AMD_LUF = 7, SPZ_AMD_RUF = 8
};

/* Reader limit of the reference, load-spz.cc:549. */
#define SPZ_AMD_REFERENCE_MAX_POINTS 10000000u

/* PackedGaussiansHeader minus the magic, load-spz.cc:131-139. */
typedef struct {
  uint32_t version;        /* 1, 2 or 3 */
  uint32_t num_points;
  uint8_t sh_degree;       /* 0..3 */
  uint8_t fractional_bits; /* writer: 12, load-spz.cc:270 */
  uint8_t flags;           /* bit0 = antialiased, load-spz.cc:129 */
  uint8_t reserved;
} spz_amd_header;

/* Section order of the stream, load-spz.cc:540-545. */
enum { SPZ_AMD_SEC_POSITIONS = 0, SPZ_AMD_SEC_ALPHAS, SPZ_AMD_SEC_COLORS, SPZ_AMD_SEC_SCALES,
       SPZ_AMD_SEC_ROTATIONS, SPZ_AMD_SEC_SH, SPZ_AMD_NUM_SECTIONS };

typedef struct {
  uint64_t total_bytes;                      /* 16 + sum(bytes) */
  uint64_t offset[SPZ_AMD_NUM_SECTIONS];     /* byte offset of each section from stream start */
  uint64_t bytes[SPZ_AMD_NUM_SECTIONS];      /* byte length of each section */
  uint32_t bytes_per_point[SPZ_AMD_NUM_SECTIONS];
} spz_amd_layout;

/* GaussianCloud's arrays (splat-types.h:101-115) as raw pointers. sh may be NULL iff sh_degree==0. */
typedef struct {
  const float *positions, *scales, *rotations, *alphas, *colors, *sh;
} spz_amd_cloud_in;
typedef struct {
  float *positions, *scales, *rotations, *alphas, *colors, *sh;
} spz_amd_cloud_out;

/* ---- introspection ---------------------------------------------------------------------- */
int spz_amd_abi_version(void);
const char *spz_amd_status_string(int status);
/* Number of usable HIP devices (0 when there is none or the runtime fails to initialise). */
int spz_amd_device_count(void);
/* hipError_t value of the last failing HIP call on this thread (0 if none). */
int spz_amd_last_hip_error(void);

/* Frees what the library keeps on the devices between calls (decode tables / thresholds, the cached
 * workspace of the *_host entry points, up to three large blocks of the gzip container stage: ~25 bytes per byte of
 * the largest stream compressed so far).  Optional: everything is re-created on demand.  Must not
 * run concurrently with other calls into the library. */
int spz_amd_release_device_memory(void);

/* ---- stream geometry: replaces the size arithmetic spread over packGaussians
 *      (load-spz.cc:273-278), serializePackedGaussians (:540-545) and
 *      deserializePackedGaussians (:578-590).  Pure host function. ------------------------ */
int spz_amd_stream_layout(uint64_t num_points, int sh_degree, int version, spz_amd_layout *out);

/* ---- header: PackedGaussiansHeader write (load-spz.cc:534-539) / checks (:551-568).
 *      Pure host functions on HOST memory.  spz_amd_peek_header applies the reference's
 *      10 M point limit; the _ex form takes the limit (0 = none) for shards that are
 *      reassembled into a stream larger than the reference itself can read. --------------- */
int spz_amd_write_header(const spz_amd_header *hdr, uint8_t out16[16]);
int spz_amd_peek_header(const uint8_t *stream, size_t size, spz_amd_header *out);
int spz_amd_peek_header_ex(const uint8_t *stream, size_t size, uint64_t max_points, spz_amd_header *out);
/* Same checks for a stream that lives in DEVICE memory (e.g. fragments reassembled over RCCL): copies
 * the 16 header bytes to the host on `hip_stream` and waits for that copy. */
int spz_amd_peek_header_device(const uint8_t *d_stream, size_t size, uint64_t max_points, spz_amd_header *out,
                               void *hip_stream);

/* ---- encode: packGaussians (load-spz.cc:257-331) + serializePackedGaussians (:533-546)
 *      fused: float SoA -> header + six sections written in place.
 *      version: 3 (what the reference writes, :272) or 2 (first-three quaternions; the
 *      reference has no v2 encoder, parity unpinned).  from_coord: PackOptions::from. -------- */
int spz_amd_encode_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree,
                          int antialiased, int from_coord, int version, uint8_t *d_stream,
                          size_t capacity, void *hip_stream);

/* ---- decode: the body of deserializePackedGaussians (section slicing, :569-590) +
 *      unpackGaussians (:467-531) with the trailing convertCoordinates(RUB, to)
 *      pass (:529, splat-types.h:134-164) fused into the same kernel.
 *      `hdr` is the header the caller obtained from spz_amd_peek_header (the first 16
 *      bytes of d_stream are not re-read).  to_coord: UnpackOptions::to. -------------------- */
int spz_amd_decode_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                          int to_coord, const spz_amd_cloud_out *d_cloud, void *hip_stream);

/* ---- point-range shards (multi-GPU / multi-stream).  The stream is attribute-major, so a
 *      shard [first, first+count) of a num_points-total stream is six fragments at
 *      offset[s] + first*bytes_per_point[s].  d_cloud holds only the shard's points.
 *      encode_shard writes the fragments (and the header iff write_header != 0) into the
 *      FULL stream buffer d_stream; decode_shard reads them from it. ------------------------ */
int spz_amd_encode_shard_device(const spz_amd_cloud_in *d_cloud, uint64_t first, uint64_t count,
                                uint64_t num_points_total, int sh_degree, int antialiased,
                                int from_coord, int version, int write_header, uint8_t *d_stream,
                                size_t capacity, void *hip_stream);
int spz_amd_decode_shard_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                uint64_t first, uint64_t count, int to_coord,
                                const spz_amd_cloud_out *d_cloud, void *hip_stream);

/* Same as spz_amd_encode_shard_device for a subset of the sections: bit s of section_mask selects section s
 * (SPZ_AMD_SEC_*).  Lets a multi-GPU caller encode the five small sections (20 B/point), hand their
 * fragments to the exchange, and encode the sh section (up to 45 B/point) while they travel. */
int spz_amd_encode_shard_sections_device(const spz_amd_cloud_in *d_cloud, uint64_t first, uint64_t count,
                                         uint64_t num_points_total, int sh_degree, int antialiased,
                                         int from_coord, int version, int write_header, unsigned section_mask,
                                         uint8_t *d_stream, size_t capacity, void *hip_stream);

/* ---- the exchange step of the multi-GPU path: the stream of R point-range shards lands on one
 *      device.  spz_amd_shard_fragments gives the six byte ranges of a shard: where they sit in the full
 *      stream (global_offset) and in a stream that holds the shard alone (local_offset).
 *
 *      RCCL route: spz_amd_gatherv_rccl issues ONE ncclGroupStart/End with the six ncclSend of every
 *      non-root rank matched by ncclRecv on the root straight at the final offsets (RCCL has no gatherv).
 *      comm is an ncclComm_t the caller owns (spz_amd_rccl_comm_init wraps ncclCommInitRank for callers that
 *      have none; the 128-byte id comes from spz_amd_rccl_unique_id on one rank and travels by any means).
 *      first[r], count[r]: the contiguous point ranges in rank order.  d_local_stream: this rank's own
 *      stream (header + its fragments); the root passes NULL when it encoded straight into
 *      d_global_stream (spz_amd_encode_shard_device).  Enqueued on hip_stream, no synchronisation.
 *      RCCL is looked up at run time (dlopen): SPZ_AMD_ERR_UNSUPPORTED when it cannot be found.
 *
 *      IPC route: the root allocates the stream with spz_amd_ipc_alloc and passes the 64-byte handle to its
 *      peers (same node); a peer maps it with spz_amd_ipc_open and hands the mapped pointer to
 *      spz_amd_encode_shard_device as d_stream: the encode kernel's stores write the fragments into the
 *      root's memory over xGMI, no second pass.  The root may read after the peer's stream has completed. -- */
typedef struct {
  uint64_t global_offset[SPZ_AMD_NUM_SECTIONS], local_offset[SPZ_AMD_NUM_SECTIONS], bytes[SPZ_AMD_NUM_SECTIONS];
} spz_amd_fragments;
int spz_amd_shard_fragments(uint64_t first, uint64_t count, uint64_t num_points_total, int sh_degree, int version,
                            spz_amd_fragments *out);
#define SPZ_AMD_RCCL_UNIQUE_ID_BYTES 128
int spz_amd_rccl_available(void);
int spz_amd_last_rccl_error(void); /* ncclResult_t of the last failing RCCL call on this thread */
int spz_amd_rccl_unique_id(uint8_t id[SPZ_AMD_RCCL_UNIQUE_ID_BYTES]);
int spz_amd_rccl_comm_init(const uint8_t id[SPZ_AMD_RCCL_UNIQUE_ID_BYTES], int world, int rank, void **comm);
int spz_amd_rccl_comm_destroy(void *comm);
int spz_amd_gatherv_rccl(void *comm, int rank, int world, int root, const uint64_t *first, const uint64_t *count,
                         int sh_degree, int version, const uint8_t *d_local_stream, uint8_t *d_global_stream,
                         unsigned section_mask, void *hip_stream);
/* The mirror image for the decode direction when the stream starts on the root only: every rank receives its six
 * fragments into a stream of its own (d_local_stream: layout of spz_amd_stream_layout(count[rank]); the header is the
 * caller's to write) and decodes them with spz_amd_decode_device.  Same group construction, 65 B/point for SH3. */
int spz_amd_scatterv_rccl(void *comm, int rank, int world, int root, const uint64_t *first, const uint64_t *count,
                          int sh_degree, int version, const uint8_t *d_global_stream, uint8_t *d_local_stream,
                          unsigned section_mask, void *hip_stream);
#define SPZ_AMD_IPC_HANDLE_BYTES 64
int spz_amd_ipc_alloc(size_t bytes, void **d_ptr, uint8_t handle[SPZ_AMD_IPC_HANDLE_BYTES]);
int spz_amd_ipc_free(void *d_ptr);
int spz_amd_ipc_open(const uint8_t handle[SPZ_AMD_IPC_HANDLE_BYTES], void **d_ptr);
int spz_amd_ipc_close(void *d_ptr);

/* ---- random access: decode only the points d_indices[0..count) out of a stream that
 *      stays packed in device memory — the bulk form of PackedGaussians::unpack(i, converter)
 *      (load-spz.cc:383-463), output in the GaussianCloud array layout (d_cloud holds `count` points).
 *      Indices >= hdr->num_points are clamped to the last point.  Same arithmetic as decode. ------- */
int spz_amd_decode_gather_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                 const uint32_t *d_indices, uint64_t count, int to_coord,
                                 const spz_amd_cloud_out *d_cloud, void *hip_stream);

/* ---- filter: a smaller stream out of a packed one without requantising (spz_filter.hip; DESIGN §8 "filter").  The
 *      reference has no counterpart (its only route is load -> floats -> save, which re-encodes).  Output point k is
 *      input point idx[k] with all its bytes; its sh bytes are the first 3*dim(d') of its 3*dim(d) (layout
 *      [N][coeff][rgb], lower bands first, so lowering the degree drops a suffix of every record).
 *
 *      select: the indices of the points whose predicates all hold, in input order: d_mask[i] != 0 (d_mask: NULL or
 *      num_points bytes of device memory), the box lo[a] <= p[a] <= hi[a] on every axis with p the position as
 *      decode (to_coord) returns it (a NaN position is never inside), the decoded alpha logit >= min_alpha (byte 0 is
 *      -inf, byte 255 +inf).  sel == NULL, or no flag set, and no mask: every point.  A NaN bound or threshold is
 *      SPZ_AMD_ERR_INVALID_ARG.  d_indices: room for hdr->num_points indices; d_workspace:
 *      spz_amd_filter_workspace_bytes(num_points) bytes of device memory owned by the caller for the call (any
 *      alignment).  Three launches on hip_stream (select, scan of the tile counts, compaction), then it BLOCKS until
 *      the count is in *h_count.
 *      subset: writes the count-point stream (header: count, degree d', the input's version, fractionalBits and
 *      antialiased bit, reserved 0; then the six sections) into d_out (capacity >= spz_amd_stream_layout(count, d',
 *      version).total_bytes).  sh_degree: -1 = the input's, 0 .. the input's = lower it; higher is
 *      SPZ_AMD_ERR_INVALID_ARG.  Indices >= hdr->num_points are clamped to the last point (check them first: the host
 *      form, spz::filterSpz and spz_amd.device.subset reject them).  Enqueued on hip_stream, no synchronisation. --- */
typedef struct {
  int32_t to_coord;        /* UnpackOptions::to of the positions the box is tested on */
  int32_t use_box;         /* != 0: box_lo / box_hi apply (inclusive) */
  float box_lo[3], box_hi[3];
  int32_t use_min_alpha;   /* != 0: min_alpha applies */
  float min_alpha;
} spz_amd_selection;
uint64_t spz_amd_filter_workspace_bytes(uint64_t num_points);
int spz_amd_select_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_selection *sel,
                          const uint8_t *d_mask, uint32_t *d_indices, void *d_workspace, uint64_t *h_count,
                          void *hip_stream);
int spz_amd_subset_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const uint32_t *d_indices,
                          uint64_t count, int sh_degree, uint8_t *d_out, size_t capacity, void *hip_stream);
/* Host form of the pair for a stream already in device memory (spz_amd_inflate_device_data, spz::filterSpz): either
 * the caller's index list (use_indices != 0; h_indices[0 .. num_indices), each < num_points, else
 * SPZ_AMD_ERR_INVALID_ARG before anything is copied; sel must then set no predicate and h_mask be NULL) or the
 * selection of sel / h_mask (host memory, num_points bytes) goes through the two calls above on `device`, on a stream
 * of the call's own.  Blocking.  The result stays in device memory in *ctx: *h_count points, *h_out_bytes bytes; fetch
 * copies it out, device_data is its address (valid until close), close frees it.  h_ms (may be NULL): [0] wall-clock
 * milliseconds of upload + select, [1] of the subset. */
int spz_amd_filter_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_selection *sel,
                        const uint8_t *h_mask, int use_indices, const uint32_t *h_indices, uint64_t num_indices,
                        int sh_degree, int device, void **ctx, uint64_t *h_count, uint64_t *h_out_bytes, float *h_ms);
int spz_amd_filter_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_filter_device_data(void *ctx);
void spz_amd_filter_close(void *ctx);

/* ---- transform: place a scene, p -> s*R*p + t, on a resident cloud or on a packed stream (spz_transform.hip; DESIGN
 *      "Transform").  The reference has only the axis flips of convertCoordinates.
 *
 *      transform_params (host only, no GPU): rotation q = (x, y, z, w) (NULL: identity; any nonzero finite length),
 *      translation t (NULL: 0; finite), uniform scale s (finite, > 0, and so in f32), all stated in `coord`; they are
 *      conjugated into the stored RUB frame in double with the axis flips of coordinateConverter(coord, RUB), and every
 *      entry of the block is rounded to f32 once.  D1 / D2 / D3 rotate the sh bands 1..3 in the 3DGS real-SH basis with
 *      its signs (D_l[k][m] = sum_q w_q Y_k(R^T d_q) Y_m(d_q); new c[m] = sum_k D_l[k][m] c[k]).  Entries within 1e-12
 *      of 0 or +-1 are snapped, so axis-aligned turns give signed permutations.  A bad argument: SPZ_AMD_ERR_INVALID_ARG.
 *      The flags say which steps run: positions unless the map is the identity, log-scales (+ ln_s) unless s == 1,
 *      rotations (q' = q_R * q, Hamilton) and sh unless R is the identity.  The default block is a bitwise no-op.
 *
 *      Per point, in f32 with every product and sum rounded on its own: p'_i = ((M_i0 x + M_i1 y) + M_i2 z) + t_i;
 *      l' = l + ln_s; q' = q_R * q (not normalised); c'[m] = sum over k ascending, starting from the k = 0 product.
 *      Alphas and colours are untouched.
 *
 *      transform_cloud_device: in place on device arrays (any pointer may be NULL).  transform_packed_device: any
 *      version 1/2/3 stream (any fractionalBits) -> a v3 stream of the same points, sh degree and antialiased bit, with
 *      positions at `fractional_bits` (0..24; saveSpz writes 12), in one pass: every float is the decoder's, every byte
 *      the encoder's.  d_out: capacity >= spz_amd_stream_layout(n, degree, 3).total_bytes.  d_out_of_range (device
 *      memory, may be NULL): set to the number of points whose new position is not finite or does not fit the 24-bit
 *      field at fractional_bits (their bytes wrap, as saveSpz's would).  Both are enqueued on hip_stream, no
 *      synchronisation.  The host form (open / fetch / device_data / close, shaped like the filter's) takes a stream
 *      already in device memory, runs on `device` on a stream of its own and blocks; h_ms (may be NULL): [0] wall-clock
 *      milliseconds of the kernel.  transform_cloud_host: host arrays in place (upload, kernel, download; blocking). */
typedef struct {
  float m[9];                 /* s * R, row-major */
  float t[3];
  float ln_s;                 /* log(s) */
  float q[4];                 /* unit q_R, (x, y, z, w) */
  float d1[9], d2[25], d3[49];  /* D_l[k][m], row-major */
  int32_t apply_positions, apply_scales, apply_rotation;
} spz_amd_transform;
int spz_amd_transform_params(const double rotation[4], const double translation[3], double scale, int coord,
                             spz_amd_transform *out);
int spz_amd_transform_cloud_device(float *d_positions, float *d_scales, float *d_rotations, float *d_sh,
                                   uint64_t num_points, int sh_degree, const spz_amd_transform *xf, void *hip_stream);
int spz_amd_transform_packed_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                    const spz_amd_transform *xf, int fractional_bits, uint8_t *d_out, size_t capacity,
                                    uint64_t *d_out_of_range, void *hip_stream);
int spz_amd_transform_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_transform *xf,
                           int fractional_bits, int device, void **ctx, uint64_t *h_out_bytes, uint64_t *h_out_of_range,
                           float *h_ms);
int spz_amd_transform_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_transform_device_data(void *ctx);
void spz_amd_transform_close(void *ctx);
int spz_amd_transform_cloud_host(float *h_positions, float *h_scales, float *h_rotations, float *h_sh,
                                 uint64_t num_points, int sh_degree, const spz_amd_transform *xf, int device);

/* ---- merge: K packed streams -> one version 3 stream (spz_merge.hip; DESIGN "Merge").  The reference has no
 *      counterpart (its only route is load every file -> concatenate floats -> save, which requantises).
 *
 *      Output: input 0's points, then input 1's, ...  Header (merge_resolve, host only, no GPU): num_points = sum n_i
 *      (above SPZ_AMD_REFERENCE_MAX_POINTS: SPZ_AMD_ERR_TOO_MANY_POINTS); sh_degree d' (-1: the largest input degree;
 *      0..3); fractionalBits f' (-1: the value every v2/v3 input shares when they agree, else 12 (v1 inputs do not
 *      vote); 0..24); antialiased (-1: every input must agree, else SPZ_AMD_ERR_INVALID_ARG; 0/1 overrides); reserved
 *      0.  k == 0, k > SPZ_AMD_MERGE_MAX_INPUTS or a request out of range: SPZ_AMD_ERR_INVALID_ARG.  *out_bytes (may
 *      be NULL) = spz_amd_stream_layout(sum n_i, d', 3).total_bytes.
 *
 *      Per input and section, bytes are copied unless the encoding or the placement forces a change: alphas and
 *      colours always; scales unless the placement scales (then + ln s per byte); positions when v2/v3 at f' and not
 *      moved (else the decoder's floats, placed, the encoder's bytes at f'); rotations when v3 and not rotated (else
 *      decoded, q_R * q, packed smallest-three); sh records unless the placement rotates (then rotated at the input's
 *      degree and re-quantised), cut to 3*dim(d') bytes or padded with byte 128 (0.0).  Each input's xf (host memory,
 *      NULL = identity) is a block of spz_amd_transform_params.
 *
 *      merge_device: d_out (capacity >= out_bytes), d_workspace (spz_amd_merge_workspace_bytes(k) bytes of device
 *      memory owned by the caller for the call; the descriptor table is copied into it), d_out_of_range (device
 *      memory, may be NULL: set to the number of points whose position is not finite or does not fit 24 bits at f'; their
 *      bytes wrap).  out_hdr is merge_resolve's.  Enqueued on hip_stream, no synchronisation; no host memory is read
 *      by the device after it returns.  The host form (open / fetch / device_data / close, shaped like the filter's)
 *      resolves the header, runs on `device` on a stream of its own and blocks; h_ms (may be NULL): [0] wall-clock
 *      milliseconds of the table upload and the kernel. */
#define SPZ_AMD_MERGE_MAX_INPUTS 1024u
typedef struct {
  const uint8_t *d_stream;       /* device memory: header + sections */
  size_t size;
  spz_amd_header hdr;
  const spz_amd_transform *xf;   /* host memory; NULL: no placement */
} spz_amd_merge_input;
int spz_amd_merge_resolve(const spz_amd_header *headers, uint64_t k, int sh_degree, int fractional_bits, int antialiased,
                          spz_amd_header *out_hdr, uint64_t *out_bytes);
uint64_t spz_amd_merge_workspace_bytes(uint64_t k);
int spz_amd_merge_device(const spz_amd_merge_input *inputs, uint64_t k, const spz_amd_header *out_hdr, uint8_t *d_out,
                         size_t capacity, void *d_workspace, uint64_t *d_out_of_range, void *hip_stream);
int spz_amd_merge_open(const spz_amd_merge_input *inputs, uint64_t k, int sh_degree, int fractional_bits, int antialiased,
                       int device, void **ctx, spz_amd_header *out_hdr, uint64_t *h_out_bytes, uint64_t *h_out_of_range,
                       float *h_ms);
int spz_amd_merge_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_merge_device_data(void *ctx);
void spz_amd_merge_close(void *ctx);

/* ---- sort: the points of a packed stream in a new order, without requantising (spz_sort.hip; DESIGN §8 "sort").  The
 *      reference has no counterpart.  The output is the filter's subset(input, order) at the input's degree: point k is
 *      input point order[k] with all its bytes; the header keeps version, fractionalBits and antialiased (reserved 0).
 *
 *      Order: key ascending (descending != 0: descending); ties by input index ascending (stable), so the output is a
 *      function of the input and the options, and sorting a sorted stream gives the same bytes.
 *      Morton key (morton_order_device): per axis a (x = 0, y = 1, z = 2) u_a = the stored 24-bit little-endian field
 *      XOR 0x800000 (orders like the sign-extended value); key bit 3*b + a = bit b of u_a, b = 0..23 (72 bits, the
 *      stored RUB frame, independent of fractionalBits); descending sorts the complemented key.  Version 1 (float16
 *      positions): SPZ_AMD_ERR_UNSUPPORTED (transform_packed with the identity writes a v3 copy).
 *      f32 keys (argsort_f32_device): the order of numpy's argsort(k, kind="stable") (descending: of argsort(-k)): -0 ==
 *      +0, +-inf sort normally, every NaN last in both directions, in input order.  n < 2^31.
 *
 *      sort_workspace_bytes (host only, no GPU): device memory for either device form at n points (any alignment).
 *      morton_order_device / argsort_f32_device write the n indices into d_order (device memory).  A stable LSD radix
 *      sort with 8-bit digits (9 passes for Morton keys, 4 for f32), each pass a tile histogram, a scan of the tile
 *      counts and a scatter.  Enqueued on hip_stream, no synchronisation.  n == 0 launches nothing.
 *      chunk_bounds_device: for runs of `chunk` (>= 1) consecutive points (the last may be partial), d_bounds[c][0][a] /
 *      d_bounds[c][1][a] = min / max over the run of the sign-extended stored integer of axis a times
 *      2^-fractionalBits, in f32 (exact), stored frame; d_bounds holds ceil(n / chunk) * 6 floats.  v1: UNSUPPORTED.
 *      Every argument error is returned before anything is launched.
 *      The host form (open / fetch / device_data / close, shaped like the filter's) takes a stream already in device
 *      memory, orders it by h_keys (host memory, hdr->num_points floats; NULL: the Morton key), then runs
 *      spz_amd_subset_device, on `device` on a stream of its own, and blocks.  Streams above
 *      SPZ_AMD_REFERENCE_MAX_POINTS: SPZ_AMD_ERR_TOO_MANY_POINTS.  h_order (may be NULL): the order, num_points
 *      entries.  h_ms (may be NULL): [0] wall-clock milliseconds of the key upload and the order, [1] of the subset. */
uint64_t spz_amd_sort_workspace_bytes(uint64_t num_points);
int spz_amd_morton_order_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int descending,
                                uint32_t *d_order, void *d_workspace, void *hip_stream);
int spz_amd_argsort_f32_device(const float *d_keys, uint64_t n, int descending, uint32_t *d_order, void *d_workspace,
                               void *hip_stream);
int spz_amd_chunk_bounds_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint32_t chunk,
                                float *d_bounds, void *hip_stream);
int spz_amd_sort_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const float *h_keys,
                      int descending, int device, void **ctx, uint64_t *h_out_bytes, uint32_t *h_order, float *h_ms);
int spz_amd_sort_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_sort_device_data(void *ctx);
void spz_amd_sort_close(void *ctx);

/* ---- decimate: one point per occupied octree cell, a coarser version of a packed stream (spz_decimate.hip; DESIGN §8
 *      "Decimate").  The reference has no counterpart.  Input v2 or v3 (version 1, float16 positions:
 *      SPZ_AMD_ERR_UNSUPPORTED, as for the sort).  Everything is in the stored RUB frame.
 *
 *      Cells: per axis u_a = the stored 24-bit field XOR 0x800000 (the sort's Morton convention); at level L (0..24)
 *      a point's cell is (u_x >> L, u_y >> L, u_z >> L), its origin (u >> L) << L, its world edge 2^(L - fractionalBits).
 *      With key_i the Morton keys in sorted order, cells(L) = 1 + #{i >= 1 : msb(key_i ^ key_i-1) >= 3L} (n >= 1).
 *      Output: a v3 stream of one point per occupied cell in ascending Morton order of the cells; the header keeps
 *      fractionalBits, shDegree and the antialiased bit (flags bit 0), reserved 0.  parents[i] (optional, n uint32) =
 *      the output index of input point i's cell.
 *      A cell of one point: the point's bytes (a v2 rotation re-encoded with the smallest-three encoder), as mergeSpz
 *      copies it; so a v3 stream with distinct stored positions at L = 0 decimates to its sort_spz bytes.
 *      A cell of several points: one Gaussian that matches their moments.  alpha_i = alpha_byte / 255, V_i =
 *      exp(ls_x + ls_y + ls_z), w_i = alpha_i V_i, W = sum w_i (W == 0: w_i = 1 and the output alpha is 0); p_i from
 *      the cell origin; mu = sum w_i p_i / W; Sigma = sum w_i (R_i diag(s_i^2) R_i^T + (p_i - mu)(p_i - mu)^T) / W (R_i of
 *      the normalised decoded quaternion; f64 accumulators).  Symmetric eigen-decomposition (cyclic Jacobi, fixed
 *      sweeps), eigenvalues descending -> x, y, z, each floored at exp(-20); log scale = ln(lambda) / 2 through the
 *      scale encoder; the eigenvectors with det +1 (third column flipped) as a quaternion through the smallest-three
 *      encoder.  alpha = min(1, W / exp(sum of the log scales before the encoder's clamp)), byte =
 *      clamp(round_half_away(255 alpha)).  Colour and every sh coefficient: the w-weighted means of the decoded floats
 *      through their encoders.  Position: origin + round_half_away(mu in quanta), clamped into the cell.
 *      Deterministic: no float atomics; every sum runs in an order fixed by n, so a run repeats its bytes.
 *
 *      decimate_workspace_bytes (host only, no GPU): device memory for either device form at n points of sh_degree.
 *      level_counts_device: sorts (spz_amd_morton_order_device + spz_amd_subset_device into the workspace), then writes
 *      cells(L) for L = 0..24 into d_counts (25 uint64, device memory; all 0 for n == 0).
 *      decimate_device: sorts, then writes the stream at `level` into d_out (device memory) and, when d_parents (device
 *      memory, n entries) is not NULL, the parents.  capacity >= spz_amd_stream_layout(cells(level), sh_degree,
 *      3).total_bytes (cells from level_counts_device); the kernels check the cell count against capacity on the
 *      device and write nothing to d_out when it does not fit.  capacity < 16: SPZ_AMD_ERR_CAPACITY.  Both enqueue on
 *      hip_stream without synchronising; every argument error is returned before anything is launched.
 *      The host form (open / fetch / device_data / close, shaped like the sort's) takes a stream already in device
 *      memory and exactly one of level (0..24, target_points 0) or target_points (>= 1, level -1: the smallest L with
 *      cells(L) <= target_points; the level counts are the one value read back), runs on `device` on a stream of its
 *      own and blocks.  Streams above SPZ_AMD_REFERENCE_MAX_POINTS: SPZ_AMD_ERR_TOO_MANY_POINTS.  *h_level (may be
 *      NULL): the level used; *h_out_hdr (may be NULL): the output header; h_parents (may be NULL): num_points entries;
 *      h_ms (may be NULL): [0] wall-clock milliseconds of the sort, [1] of the level counts, [2] of the reduction. */
uint64_t spz_amd_decimate_workspace_bytes(uint64_t num_points, int sh_degree);
int spz_amd_decimate_level_counts_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                         uint64_t *d_counts, void *d_workspace, void *hip_stream);
int spz_amd_decimate_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int level, uint8_t *d_out,
                            size_t capacity, uint32_t *d_parents, void *d_workspace, void *hip_stream);
int spz_amd_decimate_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int level,
                          uint64_t target_points, int device, void **ctx, uint64_t *h_out_bytes, int *h_level,
                          spz_amd_header *h_out_hdr, uint32_t *h_parents, float *h_ms);
int spz_amd_decimate_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_decimate_device_data(void *ctx);
void spz_amd_decimate_close(void *ctx);

/* ---- tile: an octree of LOD tiles over a packed stream (spz_tile.hip; DESIGN §8 "Tile").  The reference has no
 *      counterpart.  Input v2 or v3 (version 1: SPZ_AMD_ERR_UNSUPPORTED, as sort and decimate); above
 *      SPZ_AMD_REFERENCE_MAX_POINTS: SPZ_AMD_ERR_TOO_MANY_POINTS.  Everything is in the stored RUB frame and in the
 *      sort's and the decimate's conventions (u_a, cell = u >> L, cells(L), Morton order of the cells).
 *
 *      With the points in Morton order (spz_amd_morton_order_device, stable) and cap = max_points >= 1:
 *      A node (L, c) is an occupied cell c at level L (0..24); count(L, c) its number of points, a contiguous range
 *      [s, e) of the sorted order; cells_l(node) the number of occupied level-l cells inside it (l <= L; cells_L = 1,
 *      cells_0 = distinct stored positions).
 *      The root is the cell at the smallest L with cells(L) == 1.  A node is a leaf iff count <= cap or L == 0 (a pile
 *      of more than cap points on one lattice position is a leaf above the cap: the one exception to the cap).  Any
 *      other node is interior; its children are its occupied level L - 1 cells.  An interior node with exactly one
 *      occupied child is not emitted: the child takes its place, so every emitted interior tile has >= 2 children and
 *      there are at most 2 leaves - 1 tiles.
 *      Leaf content: points [s, e) of the sorted stream with all their bytes, i.e. spz_amd_subset_device(stream,
 *      order[s..e)) at the input's degree (the header keeps version, fractionalBits and the antialiased bit).
 *      content_level = -1, content_begin = s, geometric_error = 0.
 *      Interior content: content_level l = the smallest l in 0..L with cells_l(node) <= cap; the content is the index
 *      range [content_begin, content_begin + num_points) of spz_amd_decimate_device(stream, level = l) whose cells lie
 *      in the node, byte for byte (a v3 stream, the decimate's header).  geometric_error = 2^(l - fractionalBits), the
 *      cell edge in world units.  So num_points = cells_l(node) <= cap, cells_(l-1)(node) > cap when l > 0, and a
 *      child's content_level never exceeds its parent's (the child's cells are a subset of the parent's at every level).
 *      Order and ids: pre-order, i.e. ascending range start, the larger L first; id = the position in that order, so
 *      an interior tile's first child is id + 1 and a parent's children are in ascending Morton order.  A function of
 *      the input and cap only.
 *      Bounds, over a tile's content points: min / max per axis of the sign-extended stored integers times
 *      2^-fractionalBits (exact in f32, as spz_amd_chunk_bounds_device), and max_radius = 3 exp(scale) in f32 of the
 *      largest scale byte of the content (exp in f64 of the f32 log scale byte / 16 - 10, rounded to f32, from a table
 *      the host's libm fills).  A tile without points: NaN boxes, max_radius 0.
 *      Arena: the tiles' streams in id order, each at `offset` (a multiple of 16) and `bytes` long, zeros between them.
 *      Deterministic: no float atomics; integer atomics and fixed-order scans only: a run repeats its table and bytes.
 *      Arguments: max_points 1..SPZ_AMD_REFERENCE_MAX_POINTS, max_tiles 1..2^31 - 1; a bad one is
 *      SPZ_AMD_ERR_INVALID_ARG before anything is launched.  n == 0: one empty leaf (level 0, 16 bytes).
 *
 *      tile_workspace_bytes (host only, no GPU): device memory for tile_tree_device.
 *      tile_tree_device: sorts, then writes the summary and, when the tree has at most max_tiles tiles (summary.ok),
 *      the table rows (d_table: min(max_tiles, max(1, 2 n - 1)) rows) with every integer field, the arena layout and the
 *      leaves' bounds; interior boxes are NaN and their max_radius 0.  Enqueue-only; nothing is read back.
 *      tile_content_device: for the num_tiles rows whose content_level is `content_level` (-1: the leaves), with
 *      d_source the stream their content is cut from (the sorted stream; the decimate's output at that level; its
 *      header is read on the device): the bounds into the table and, when d_arena is not NULL, header + six sections
 *      of every such tile into the arena at the table's offsets.  One launch per source, work items of 1024 points; a
 *      row whose range does not lie in the source or the arena is left alone.  Enqueue-only.
 *      The host form takes a stream already in device memory, runs on `device` on a stream of its own and blocks: the
 *      tree, one readback of the summary and the table (more than max_tiles tiles: SPZ_AMD_ERR_CAPACITY, before any
 *      content is produced), then per distinct content_level one spz_amd_decimate_device into a reused buffer and its
 *      tile_content_device, then the leaves', all enqueued without readbacks; the finished table is read once at the
 *      end.  h_ms (may be NULL): wall-clock milliseconds of [0] the sort, [1] the tree, [2] the decimates, [3] bounds
 *      and emit.  tile_table: the rows; tile_fetch / tile_device_data: one tile's stream; tile_fetch_arena: all. */
typedef struct {
  uint32_t id;
  int32_t parent;          /* -1: the root */
  int32_t first_child;     /* id + 1, or -1 for a leaf */
  uint32_t child_count;
  int32_t level;           /* L */
  uint32_t cell[3];        /* u_a >> L of the tile's points */
  uint32_t range_begin, range_end;   /* [s, e) of the sorted order */
  int32_t content_level;   /* -1: a leaf */
  uint32_t num_points;     /* of the content */
  uint32_t content_begin;  /* first index of the content in its source stream */
  uint32_t reserved;
  uint64_t offset, bytes;  /* of the tile's stream in the arena */
  float box_min[3], box_max[3];
  float max_radius;
  float geometric_error;
} spz_amd_tile_info;       /* 104 bytes */
typedef struct {
  uint64_t num_tiles;
  uint64_t arena_bytes;
  uint32_t ok;             /* num_tiles <= max_tiles: the table is written */
  uint32_t root_level;
  uint64_t cells[25];      /* cells(L) of the whole stream */
} spz_amd_tile_summary;
uint64_t spz_amd_tile_workspace_bytes(uint64_t num_points, int sh_degree, uint64_t max_tiles);
uint64_t spz_amd_tile_content_workspace_bytes(uint64_t num_tiles);
int spz_amd_tile_tree_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint32_t max_points,
                             uint32_t max_tiles, spz_amd_tile_info *d_table, spz_amd_tile_summary *d_summary,
                             void *d_workspace, void *hip_stream);
int spz_amd_tile_content_device(spz_amd_tile_info *d_table, uint32_t num_tiles, int content_level,
                                const uint8_t *d_source, size_t source_size, uint8_t *d_arena, uint64_t arena_bytes,
                                void *d_workspace, void *hip_stream);
int spz_amd_tile_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint32_t max_points,
                      uint32_t max_tiles, int device, void **ctx, uint64_t *h_num_tiles, uint64_t *h_arena_bytes,
                      float *h_ms);
int spz_amd_tile_table(void *ctx, spz_amd_tile_info *h_table);
int spz_amd_tile_fetch(void *ctx, uint32_t id, uint8_t *h_out);
int spz_amd_tile_fetch_arena(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_tile_device_data(void *ctx, uint32_t id);
void spz_amd_tile_close(void *ctx);

/* ---- clean: floater removal, the statistical (k nearest neighbours) and the radius outlier rules (spz_clean.hip;
 *      DESIGN §8 "Clean").  The reference has no counterpart.  Input v2 or v3 (version 1, float16 positions:
 *      SPZ_AMD_ERR_UNSUPPORTED, as for the sort).  Streams above SPZ_AMD_REFERENCE_MAX_POINTS:
 *      SPZ_AMD_ERR_TOO_MANY_POINTS.
 *
 *      Distances: the stored RUB frame, P_i the sign-extended stored 24-bit integers; d2(i, j) = sum_a (P_ia - P_ja)^2,
 *      exact (< 2^50).  The neighbours of i are the other points by index; duplicates count, at distance 0.
 *      Statistical rule: k_eff = min(k, n - 1); score_i = (sum_{j=1..k_eff} sqrt(d2_(j))) / k_eff * 2^-fractionalBits in
 *      f64, d2_(1) <= ... <= d2_(k_eff) the k_eff smallest, summed in ascending order, sqrt correctly rounded.
 *      thr = mean + std_ratio * std over the n scores, std with the n - 1 divisor, f64 sums in an order fixed by n.
 *      Keep i iff score_i <= thr.  n == 1: score 0.
 *      Radius rule: R2 = floor(fl((radius * 2^fractionalBits)^2)) in f64 on the host (clean_radius_r2);
 *      count_i = min(#{j != i : d2(i, j) <= R2}, min_neighbors).  Keep i iff count_i >= min_neighbors.
 *      Both rules: a point is kept iff it passes both.  n <= 1: every point is kept.
 *      Output: spz_amd_subset_device of the kept indices in input order at the input's degree, so the stream is
 *      byte-identical to the filter's with the keep mask (header: version, fractionalBits and antialiased bit kept).
 *      Arguments: k 1..64, std_ratio finite, radius finite and > 0, min_neighbors 1..256, at least one rule; a bad one is
 *      SPZ_AMD_ERR_INVALID_ARG, returned before anything is launched.
 *
 *      clean_workspace_bytes (host only, no GPU): device memory for either device form at n points (any alignment).
 *      clean_radius_r2 (host only): R2 of the radius rule (>= 2^64: UINT64_MAX).
 *      knn_scores_device: the n scores into d_scores (device memory, f64, input order) and, when d_kth_d2 (device
 *      memory, n uint64) is not NULL, d2_(k_eff) of every point.  radius_counts_device: the n counts into d_counts
 *      (device memory, uint32) for a given R2.  Both Morton-sort the positions into the workspace first
 *      (spz_amd_morton_order_device), enqueue on hip_stream and do not synchronise.
 *      The host form (open / fetch / device_data / close, shaped like the decimate's) takes a stream already in device
 *      memory and the rules (k == 0: no statistical rule; min_neighbors == 0: no radius rule, radius ignored), runs the
 *      scores and / or counts, the threshold, the keep mask, spz_amd_select_device and spz_amd_subset_device on
 *      `device` on a stream of its own, and blocks.  *h_kept (may be NULL): the kept count; *h_threshold (may be NULL):
 *      thr (NaN without the statistical rule); h_mask (may be NULL): num_points bytes, 1 = kept; h_scores (may be NULL;
 *      only with the statistical rule): num_points f64; h_ms (may be NULL): [0] wall-clock milliseconds of the sort,
 *      [1] of the scores and counts, [2] of the threshold, the mask and the subset. */
uint64_t spz_amd_clean_workspace_bytes(uint64_t num_points);
int spz_amd_clean_radius_r2(double radius, int fractional_bits, uint64_t *r2);
int spz_amd_knn_scores_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int k, double *d_scores,
                              uint64_t *d_kth_d2, void *d_workspace, void *hip_stream);
int spz_amd_radius_counts_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint64_t r2,
                                 uint32_t min_neighbors, uint32_t *d_counts, void *d_workspace, void *hip_stream);
int spz_amd_clean_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int k, double std_ratio,
                       double radius, uint32_t min_neighbors, int device, void **ctx, uint64_t *h_out_bytes,
                       uint64_t *h_kept, double *h_threshold, uint8_t *h_mask, double *h_scores, float *h_ms);
int spz_amd_clean_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_clean_device_data(void *ctx);
void spz_amd_clean_close(void *ctx);

/* ---- align: the similarity that places a source stream on a target stream, by a point-to-point, trimmed ICP with an
 *      optional scale (spz_align.hip; DESIGN §8 "Align").  The reference has no counterpart.  The convention of Open3D's
 *      registration_icp(TransformationEstimationPointToPoint(with_scaling)) with the trimming of Chetverikov's TrICP.
 *      Source S (n_s points, fractionalBits f_s) and target T (n_t >= 1 points, f_t; n_t == 0: SPZ_AMD_ERR_INVALID_ARG),
 *      both v2 or v3 (version 1, float16 positions: SPZ_AMD_ERR_UNSUPPORTED, as for sort and clean), both at most
 *      SPZ_AMD_REFERENCE_MAX_POINTS (SPZ_AMD_ERR_TOO_MANY_POINTS).  All geometry is in the stored RUB frame; align_host
 *      conjugates the options' placement into it and the result out of it with the axis flips of
 *      spz_amd_transform_params (R = F R_c F, t = F t_c), in f64.
 *
 *      One step for a map (map[0..9) = M = s R row-major, map[9..12) = t, f64):
 *      1. x_i = P_i 2^-f_s, P_i the sign-extended stored integers (exact).  Only i with i % stride == 0 take part.
 *      2. y_a = ((M_a0 x + M_a1 y) + M_a2 z) + t_a in f64, every product and sum rounded on its own (no fused
 *         multiply-add).  Query Q_i = rint(y_i 2^f_t) (ties to even), each component saturated to [-2^26, 2^26]; a
 *         non-finite y_i makes i invalid.
 *      3. j(i) = the target point with the smallest d2(i, j) = sum_a (Q_ia - P^T_ja)^2, an exact integer below 2^56
 *         (uint64); ties go to the smallest target input index.
 *      4. With a limit R2 (spz_amd_clean_radius_r2(max_distance, f_t); UINT64_MAX: none) i is a candidate iff
 *         d2 <= R2; without one every valid i is.  With overlap f in (0, 1], K = min(c, ceil(f c)) in f64 over the c
 *         candidates, and the inliers are the K candidates smallest by (d2, source index): an exact rank on integer
 *         keys (a stable radix sort).
 *      5. Moments over the inliers, a = x_i, b = P^T_j(i) 2^-f_t, in f64: sum a, sum b, sum a b^T (sum_ab[3 r + c] =
 *         sum a_r b_c), sum |a|^2, sum |b|^2 (|v|^2 = (x x + y y) + z z), and as integers the count K and sum d2
 *         (sum_d2_hi 2^64 + sum_d2_lo).  No float atomics: per tile of 2048 source points a pairwise sum in a fixed
 *         tree, then one workgroup over the tiles, so the order depends on n_s alone and a run repeats its bits; every
 *         f64 sum is within (ceil(log2 n_s) + 2) 2^-53 sum |term| of the exact one.
 *      6. align_solve (host only, no GPU, f64; a 3x3 one-sided Jacobi SVD): ma = sum a / K, mb = sum b / K,
 *         H = sum_ab^T / K - mb ma^T = U D V^T, S = diag(1, 1, sign(det U det V)), R = U S V^T, s = tr(D S) / var_a
 *         (var_a = sum |a|^2 / K - |ma|^2) when estimate_scale, else scale_in; t = mb - s R ma.  *degenerate = 1 (and
 *         map_out untouched) when K < 3, var_a is not > 0 or D_1 <= 1e-12 D_0 (a line or a point: no rotation).
 *      fitness = K / (number of source points taking part); inlier_rmse = sqrt(sum d2 / K) 2^-f_t (0 for K == 0).
 *
 *      The run (align_host; blocking, on `device`, on a stream of its own; both streams already in device memory): from
 *      the options' rotation (x, y, z, w; any nonzero finite length), translation and scale, stated in coord (with
 *      init_centroids the translation is first replaced so that the centroid of the taking-part source points lands on
 *      the target's centroid), step and solve until max_iterations steps ran or, after a step, both |fitness -
 *      previous| <= relative_fitness max(fitness, previous) and |rmse - previous| <= relative_rmse max(rmse, previous)
 *      (converged = 1).  A degenerate solve ends the run (degenerate = 1, converged = 0).  The result is the map USED BY
 *      THE LAST STEP with that step's fitness, rmse and inlier count: map in the stored frame; rotation (unit, w >= 0),
 *      translation and scale stated in coord, ready for spz_amd_transform_params.  history (may be NULL): one entry per
 *      step, up to capacity.  h_ms (may be NULL): [0] wall-clock milliseconds of the preparation, [1] of the queries,
 *      [2] of the selections, moments and solves.  The two clouds are put in Morton order once per run.
 *      align_check (host only, no GPU): stride >= 1; overlap in (0, 1]; max_distance (when has_max_distance) finite and
 *      > 0; max_iterations 1..1000; tolerances finite and >= 0; rotation of nonzero finite length, translation finite,
 *      scale finite and > 0; coord 0..8.  A bad one is SPZ_AMD_ERR_INVALID_ARG before anything is launched.
 *      align_default_options: identity, overlap 1, no max_distance, stride 1, 30 iterations, tolerances 1e-6.
 *
 *      Device forms (enqueue on hip_stream, no synchronisation; d_workspace: align_workspace_bytes(n_s, n_t) bytes of
 *      device memory, any alignment, the same for every call on one pair).  align_prepare_device: the Morton order and
 *      the sorted positions of both clouds.  nearest_device: steps 1-3 for a prepared pair, results in source input
 *      order (d_index: n_s uint32, d_d2: n_s uint64); 0xFFFFFFFF / UINT64_MAX for points not taking part, invalid, or
 *      without a neighbour within r2.  align_step_device: steps 1-5 (d_index, d_d2 and d_inlier, n_s bytes, may be
 *      NULL: kept in the workspace) into *d_out (device memory). */
typedef struct {
  const uint8_t *d_stream;       /* device memory: header + sections */
  size_t size;
  spz_amd_header hdr;
} spz_amd_align_cloud;
typedef struct {
  double rotation[4];            /* (x, y, z, w), in coord */
  double translation[3];
  double scale;
  int32_t coord;
  int32_t estimate_scale;
  double overlap;
  double max_distance;           /* world units; read when has_max_distance */
  int32_t has_max_distance;
  uint32_t stride;
  uint32_t max_iterations;
  int32_t init_centroids;
  double relative_fitness, relative_rmse;
} spz_amd_align_options;
typedef struct {
  uint64_t count;                /* K */
  uint64_t taking_part;
  uint64_t candidates;           /* c */
  uint64_t sum_d2_lo, sum_d2_hi;
  double sum_a[3], sum_b[3], sum_ab[9], sum_aa, sum_bb;
} spz_amd_align_moments;
typedef struct {
  double fitness, inlier_rmse;
  uint64_t inliers;
} spz_amd_align_history;
typedef struct {
  double rotation[4], translation[3], scale;   /* in coord */
  double map[12];                               /* stored frame */
  double fitness, inlier_rmse;
  uint64_t inliers;
  uint32_t iterations;
  int32_t converged, degenerate;
} spz_amd_align_result;
int spz_amd_align_default_options(spz_amd_align_options *options);
int spz_amd_align_check(const spz_amd_align_options *options);
uint64_t spz_amd_align_workspace_bytes(uint64_t num_source, uint64_t num_target);
int spz_amd_align_prepare_device(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target, void *d_workspace,
                                 void *hip_stream);
int spz_amd_nearest_device(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target, uint32_t stride,
                           const double map[12], uint64_t r2, uint32_t *d_index, uint64_t *d_d2, void *d_workspace,
                           void *hip_stream);
int spz_amd_align_step_device(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target, uint32_t stride,
                              const double map[12], uint64_t r2, double overlap, uint32_t *d_index, uint64_t *d_d2,
                              uint8_t *d_inlier, spz_amd_align_moments *d_out, void *d_workspace, void *hip_stream);
int spz_amd_align_solve(const spz_amd_align_moments *moments, int estimate_scale, double scale_in, double map_out[12],
                        double *scale_out, int *degenerate);
int spz_amd_align_host(const spz_amd_align_cloud *source, const spz_amd_align_cloud *target,
                       const spz_amd_align_options *options, int device, spz_amd_align_result *result,
                       spz_amd_align_history *history, uint32_t capacity, float *h_ms);

/* ---- plane: the dominant plane of a packed stream, or up to K of them, by MSAC over seeded hypotheses with an exact
 *      least-squares refinement, and the placement that levels the scene on it (spz_plane.hip; DESIGN §8 "Level").  The
 *      reference has no counterpart.  Everything after the hypotheses' normals is integer arithmetic on the stored 24-bit
 *      positions, so a restatement in Python integers agrees count for count.  v2 or v3 (version 1, float16 positions:
 *      SPZ_AMD_ERR_UNSUPPORTED), at most SPZ_AMD_REFERENCE_MAX_POINTS (SPZ_AMD_ERR_TOO_MANY_POINTS).  All geometry is in
 *      the stored RUB frame; plane_host conjugates the options in and the results out with the axis flips of
 *      spz_amd_transform_params.
 *
 *      1. Points.  P_i = the sign-extended stored integers (fractionalBits f).  Point i takes part iff i % stride == 0
 *         and labels[i] == 0 (labels: uint8 per point, device memory; NULL: all zero).  plane_prepare_device compacts the
 *         taking-part points, in input order, into the workspace (int32 X, Y, Z and the input index), and blocks until
 *         their count m is in *h_count, as select_device does.
 *      2. Plane (a, b, c, e): int32 a, b, c in [-2^16, 2^16], int64 e.  The signed distance of P is the exact integer
 *         d = a X + b Y + c Z - e, |d| < 2^43.  Threshold T = floor(tau 2^(f+16)) for tau in world units
 *         (plane_threshold, host only; tau not finite, < 0, or T > 2^36: SPZ_AMD_ERR_INVALID_ARG).  P is an inlier iff
 *         |d| <= T.  A plane with a = b = c = 0 is invalid.
 *      3. Score (plane_score_device): for each of H planes (device memory) over the m prepared points, K = the number of
 *         inliers, S = sum |d| over them (< 2^60), cost = S + T (m - K), the MSAC cost.  An invalid plane: K = S = 0,
 *         cost = UINT64_MAX.  Integers: a run repeats its bits however it is summed.
 *      4. Hypotheses (plane_hypotheses; host only, no GPU, f64).  idx(r, h, k) = mix64(seed + (r << 48) + 3 h + k) mod m
 *         (uint64 arithmetic, wrapping) for round r, hypothesis h, k = 0..2, with splitmix64's finaliser
 *             mix64(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
 *         h_indices (3 H, may be NULL) receives them; with h_points (3 H x 3 int32: prepared point idx(r, h, k) at row
 *         3 h + k, what plane_gather_device returns for those indices) h_planes receives the planes:
 *         N = (P_1 - P_0) x (P_2 - P_0) in exact int64 (components below 2^52); two equal indices or N = 0: invalid
 *         (a = b = c = e = 0).  Else each component to f64, L = sqrt((Nx Nx + Ny Ny) + Nz Nz), every product and sum
 *         rounded on its own, (a, b, c) = rint(65536 N / L) (the product first), e = a X_0 + b Y_0 + c Z_0.  With a
 *         constraint (axis: 3 doubles, stored frame, nonzero, normalised by sqrt((x x + y y) + z z); NULL: none) a plane
 *         with |(a u_x + b u_y) + c u_z| < 65536 cos(max_tilt pi / 180) is invalid.
 *      5. Moments (plane_moments_device; one plane by value, one lane per prepared point): K and S as above, the side
 *         counts above (d > T) and below (d < -T), and over the inliers sum P (3 int64) and sum XX, XY, XZ, YY, YZ, ZZ as
 *         exact 128-bit integers (hi 2^64 + lo, two's complement).  int64 sums per tile of 2048 points (2048 2^46 <
 *         2^63), joined with carries: exact, so a run repeats its bits.
 *      6. Solve (plane_solve; host only, no GPU): M = K sum P P^T - sum P sum P^T in exact 128-bit integers (< 2^96),
 *         each entry rounded once to f64; a cyclic Jacobi eigen-solve of the symmetric 3 x 3 (sweeps over (0,1), (0,2),
 *         (1,2) until no rotation is left; a pair is rotated unless |m_pq| <= 1e-17 sqrt(|m_pp|) sqrt(|m_qq|));
 *         n = the unit eigenvector of the smallest eigenvalue, (a, b, c) = rint(65536 n),
 *         e = (a sum X + b sum Y + c sum Z) / K rounded to the nearest integer, ties to even, in exact integers.
 *         *degenerate = 1 (and *out untouched) when K < 3 or the middle eigenvalue is <= 1e-12 of the largest (a line or
 *         a point), the rule and constant of align_solve.  normal (3 doubles) and eigenvalues (3 doubles, descending;
 *         both may be NULL) receive n and the eigenvalues of M before the rounding.
 *      7. The run (plane_host; blocking, on `device`, on a stream of its own; the stream already in device memory).  For
 *         round r = 0 .. max_planes - 1: prepare (stop if m < 3); the H hypotheses, scored; the best is the smallest cost,
 *         ties to the smallest h (stop if none is valid); up to `refine` times moments of the current plane, solve, score
 *         of the solved plane, accepted only when its cost is strictly smaller (the first rejected or degenerate solve
 *         ends the refinement); stop if the final K < min_inliers; orientation: with has_up_hint negate (a, b, c, e) if
 *         n . hint < 0, else negate if below > above (the scene lies on the positive side of its floor), and on
 *         above == below choose b >= 0 (stored +Y is up); plane_mark_device writes r + 1 into labels at the input indices
 *         of the inliers.  Per plane the result holds the integers, K, S, m, above, below, the winning h, the accepted
 *         refinements, fitness = K / m, mean_distance = S / K 2^-(f+16), the unit normal n = (a, b, c) / |(a, b, c)| and
 *         offset d = e / |(a, b, c)| 2^-f (n . p = d, world units) with n stated in coord, and the levelling placement:
 *         the shortest arc that takes n to the up axis of coord (+-Y by its U / D letter: stored +Y), q = (-n_z, 0, n_x,
 *         w) normalised with w = 1 + n_y, or (n_x^2 + n_z^2) / (1 - n_y) for n_y < 0, and a half turn about stored X
 *         when w < 1e-12 (n opposite to up); translation -d up (0 under no_translate); scale 1; stated in coord as
 *         (x, y, z, w), w >= 0, ready for spz_amd_transform_params.  h_labels (may be NULL): num_points bytes, 0 or the
 *         1-based plane of each point.  *h_found: the number of planes written (at most `capacity`, which must be >=
 *         max_planes).  h_ms (may be NULL): [0] wall-clock milliseconds of prepare + gather, [1] of the scoring, [2] of
 *         moments, solves and marks.
 *      plane_check (host only, no GPU): hypotheses 1..65536; refine 0..16; max_planes 1..255; stride >= 1; tau finite
 *      and >= 0; a finite, nonzero axis (when has_axis) and hint (when has_up_hint); max_tilt in [0, 90]; coord 0..8.
 *      plane_default_options: 4096 hypotheses, refine 3, one plane, stride 1, seed 0, no constraint, min_inliers 0,
 *      tau = NaN (it has no default and must be given).
 *
 *      Device forms (enqueue on hip_stream; only prepare blocks; d_workspace: plane_workspace_bytes(num_points) bytes of
 *      device memory, any alignment, the same for every call on one stream).  plane_gather_device: d_out[k] (3 int32) =
 *      prepared point d_indices[k], k < count (an index >= m is clamped to m - 1).  d_scores: 3 H uint64 (K, S, cost per
 *      plane).  d_moments: one spz_amd_plane_moments.  plane_mark_device: d_labels[index] = value for the inliers.
 *      plane_placement (host only, no GPU): the plane, normal, offset, rotation, translation and scale of *out for an
 *      oriented plane at fractional_bits, as plane_host reports them; the other members are untouched.
 *      plane_sides_host (blocking, on `device`, the stream in device memory): h_side[i] = 0 (|d| <= T), 1 (d > T) or 2
 *      (d < -T) for every point i of the stream, whatever stride and labels a run used: the masks of a selection.
 *      A plane whose a, b, c lie outside [-2^16, 2^16] or whose |e| > 2^42 counts as invalid wherever a = b = c = 0 does
 *      (the forms that take one plane by value return SPZ_AMD_ERR_INVALID_ARG for an invalid one). */
typedef struct {
  int32_t a, b, c, reserved;
  int64_t e;
} spz_amd_plane;
typedef struct {
  double threshold;              /* tau, world units */
  uint32_t hypotheses, refine, max_planes, stride;
  uint64_t seed;
  uint64_t min_inliers;
  int32_t has_axis;
  double axis[3];                /* in coord */
  double max_tilt;               /* degrees */
  int32_t has_up_hint;
  double up_hint[3];             /* in coord */
  int32_t coord;
  int32_t no_translate;
} spz_amd_plane_options;
typedef struct {
  uint64_t count;                /* K */
  uint64_t sum_abs;              /* S */
  uint64_t above, below;
  uint64_t points;               /* m */
  int64_t sum_p[3];
  uint64_t sum_pp_lo[6];         /* XX, XY, XZ, YY, YZ, ZZ */
  int64_t sum_pp_hi[6];
} spz_amd_plane_moments;
typedef struct {
  spz_amd_plane plane;           /* stored frame, oriented */
  uint64_t inliers, sum_abs, points, above, below;
  uint32_t best_hypothesis, refinements;
  double fitness, mean_distance;
  double normal[3], offset;      /* in coord, world units */
  double rotation[4], translation[3], scale;   /* the levelling placement, in coord */
} spz_amd_plane_result;
int spz_amd_plane_default_options(spz_amd_plane_options *options);
int spz_amd_plane_check(const spz_amd_plane_options *options);
int spz_amd_plane_threshold(double tau, int fractional_bits, uint64_t *threshold);
uint64_t spz_amd_plane_workspace_bytes(uint64_t num_points);
int spz_amd_plane_prepare_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, uint32_t stride,
                                 const uint8_t *d_labels, void *d_workspace, uint64_t *h_count, void *hip_stream);
int spz_amd_plane_gather_device(const void *d_workspace, uint64_t num_points, uint64_t m, const uint32_t *d_indices,
                                uint64_t count, int32_t *d_out, void *hip_stream);
int spz_amd_plane_hypotheses(uint64_t seed, uint32_t round, uint32_t hypotheses, uint64_t m, const int32_t *h_points,
                             const double *axis, double max_tilt, uint32_t *h_indices, spz_amd_plane *h_planes);
int spz_amd_plane_score_device(void *d_workspace, uint64_t num_points, uint64_t m, const spz_amd_plane *d_planes,
                               uint32_t hypotheses, uint64_t threshold, uint64_t *d_scores, void *hip_stream);
int spz_amd_plane_moments_device(void *d_workspace, uint64_t num_points, uint64_t m, const spz_amd_plane *plane,
                                 uint64_t threshold, spz_amd_plane_moments *d_moments, void *hip_stream);
int spz_amd_plane_solve(const spz_amd_plane_moments *moments, spz_amd_plane *out, double *normal, double *eigenvalues,
                        int *degenerate);
int spz_amd_plane_mark_device(const void *d_workspace, uint64_t num_points, uint64_t m, const spz_amd_plane *plane,
                              uint64_t threshold, uint8_t value, uint8_t *d_labels, void *hip_stream);
int spz_amd_plane_placement(const spz_amd_plane *plane, int fractional_bits, int coord, int no_translate,
                            spz_amd_plane_result *out);
int spz_amd_plane_sides_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_plane *plane,
                             uint64_t threshold, int device, uint8_t *h_side);
int spz_amd_plane_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                       const spz_amd_plane_options *options, int device, spz_amd_plane_result *results,
                       uint32_t capacity, uint32_t *h_found, uint8_t *h_labels, float *h_ms);

/* ---- render: a forward 3D Gaussian splat rasteriser (spz_render.hip; DESIGN §8 "Render").  The reference has no
 *      counterpart.  The image of one pinhole view, computed on the device with no display attached.
 *
 *      Input.  The cloud as loadSpz(to = coord) returns it: the packed forms decode every Gaussian with the per-field
 *      decoders of the decode kernel (positions, scales, quaternions, alpha, colour, sh and the coordinate flips), then
 *      run the code of the float forms, so a stream and its decoded floats give bit-identical images.  Versions 1, 2
 *      and 3.  The float forms take the GaussianCloud arrays (spz_amd_cloud_in) as they are; coord is ignored there.
 *      Camera: OpenCV axes (x right, y down, z forward).  world_to_camera: [R | t] row-major 3x4 in the coord frame;
 *      R orthonormal to within 1e-4 per entry of R R^T - I, det R > 0.  fx, fy > 0; cx, cy finite; width, height
 *      1..16384; near_plane > 0 (0.2 by default in the C++ and Python layers); background RGB finite; max_sh_degree
 *      0..3 (the degree used is min(file's, max_sh_degree)); coord 0..8.  A bad one: SPZ_AMD_ERR_INVALID_ARG.
 *
 *      Per Gaussian (3DGS forward pass, Kerbl et al. 2023, with gsplat's general principal point).  The arithmetic
 *      runs in f64 from the f32 inputs; the record holds f32.  p_c = R p + t; z <= near: invisible.
 *      mean m = (fx x/z + cx - 0.5, fy y/z + cy - 0.5) in pixel-index units.  Sigma = M M^T, M = R_q diag(exp(log
 *      scale)), R_q of the normalised quaternion (x, y, z, w).  J of x/z clamped to [-(cx/fx + 0.3 W/fx),
 *      (W - cx)/fx + 0.3 W/fx] (likewise y with cy, fy, H).  Sigma' = J R Sigma R^T J^T, then + 0.3 on the diagonal.
 *      Antialiased bit (flags bit 0, or the float forms' argument): opacity *= sqrt(max(0, det_before) / det_after).
 *      det_after <= 0: invisible.  conic = Sigma'^-1 as (A, B, C).  radius = ceil(3 sqrt(mid + sqrt(max(0.1, mid^2 -
 *      det)))), mid = (a + c) / 2.  Tiles are 16x16: rect x0 = clamp(floor((m_x - radius) / 16), 0, tiles_x), x1 =
 *      clamp(floor((m_x + radius + 15) / 16), 0, tiles_x), likewise y; empty: invisible.  rgb = max(0, C0 colour + the
 *      higher sh bands of 3DGS (constants and band order) at normalize(p - c), c = -R^T t, + 0.5).  opacity =
 *      sigmoid(alpha).  A non-finite mean, conic, radius or opacity (a NaN alpha): invisible.  An invisible
 *      Gaussian's record is all zero but for depth = +inf.
 *      Order: within a tile, ascending (f32 depth z, input index).  Blend per pixel (u, v), d = (u - m_x, v - m_y),
 *      T = 1, C = 0, in that order: power = -0.5 (A dx^2 + C dy^2) - B dx dy, skip if power > 0; a = min(0.99,
 *      opacity exp(power)), skip if a < 1/255; T' = T (1 - a), stop if T' < 1e-4; C += T a rgb; T = T'.
 *      Image: height x width x 4 float32, row-major, RGB = C + T background, alpha = 1 - T, not clamped.
 *      Deterministic: no float atomics; a run repeats its bits.  (That is the forward's promise alone: "render backward"
 *      below sums with f32 atomic adds and need not repeat its bits.)
 *
 *      render_check_params (host only, no GPU): the argument checks above.  render_workspace_bytes (host only): device
 *      memory for the device forms at n Gaussians and max_entries (tile, Gaussian) entries; the prepare step touches
 *      only the first render_workspace_bytes(n, 0) bytes, so that prefix may be copied to the front of a larger one.
 *      prepare_packed_device / prepare_cloud_device: decode + preprocess (records, tile counts, depth keys), the depth
 *      order (spz_amd_argsort_f32_device, stable) and the scan of the tile counts in that order; *d_total (device
 *      memory, uint64) = the number of entries; d_records (device memory, may be NULL) gets the n records in input
 *      order.  render_finish_device: with the same n, params and workspace, and max_entries <= 2^31 - 1: the entries in
 *      depth order, their stable radix sort by tile id, the tile ranges and the blend into d_image (device memory,
 *      height x width x 4 floats).  *d_status (device memory, uint32) = 0, or 1 when the total is above max_entries:
 *      then nothing is written to d_image.  All enqueue on hip_stream and do not synchronise.
 *      The host forms take a stream already in device memory (render_host) or a cloud in host memory
 *      (render_cloud_host), run on `device` on a stream of their own, read the total back once, size their own
 *      workspace and block.  A total above 2^31 - 1: SPZ_AMD_ERR_CAPACITY.  h_rgba: height x width x 4 floats;
 *      *h_entries (may be NULL): the total; h_ms (may be NULL): [0] wall-clock milliseconds of the preprocess (with
 *      the depth order and the scan), [1] of the tile entries and their sort, [2] of the blend. */
typedef struct {
  float world_to_camera[12];
  float fx, fy, cx, cy;
  uint32_t width, height;
  float near_plane;
  float background[3];
  int32_t max_sh_degree;
  int32_t coord;
} spz_amd_render_params;

/* One preprocessed Gaussian (48 bytes): rect = tile x0, y0, x1, y1 (half-open). */
typedef struct {
  float mean[2];
  float conic[3];
  float opacity;
  float rgb[3];
  float depth;
  uint16_t rect[4];
} spz_amd_render_record;

int spz_amd_render_check_params(const spz_amd_render_params *params);
uint64_t spz_amd_render_workspace_bytes(uint64_t num_points, uint64_t max_entries);
int spz_amd_render_prepare_packed_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                         const spz_amd_render_params *params, uint64_t *d_total,
                                         spz_amd_render_record *d_records, void *d_workspace, void *hip_stream);
int spz_amd_render_prepare_cloud_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree,
                                        int antialiased, const spz_amd_render_params *params, uint64_t *d_total,
                                        spz_amd_render_record *d_records, void *d_workspace, void *hip_stream);
int spz_amd_render_finish_device(uint64_t num_points, const spz_amd_render_params *params, uint64_t max_entries,
                                 float *d_image, uint32_t *d_status, void *d_workspace, void *hip_stream);
int spz_amd_render_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                        const spz_amd_render_params *params, int device, float *h_rgba, uint64_t *h_entries,
                        float *h_ms);
int spz_amd_render_cloud_host(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_degree, int antialiased,
                              const spz_amd_render_params *params, int device, float *h_rgba, uint64_t *h_entries,
                              float *h_ms);

/* ---- render backward: the gradients of one view to a float cloud (spz_render_backward.hip; DESIGN §8 "Render
 *      backward").  The reference has no counterpart.  Given G (height x width x 4 float32), the gradient of a scalar
 *      loss to the image of render_finish_device, it produces that loss's gradient to the six arrays of the float cloud
 *      the image was prepared from: positions, log scales, rotations (xyzw, unnormalised), alphas (pre-sigmoid), colours
 *      and sh, in the shapes and order of spz_amd_cloud_in.  The packed streams have no backward.
 *
 *      It is the exact derivative of the forward as "render" words it, with every discrete decision held constant:
 *      visibility, radius, tile rectangle, depth order, "skip if power > 0", "skip if a < 1/255" and "stop if T' < 1e-4".
 *      Skipped pairs, the stopping pair and everything after it contribute nothing.  a = min(0.99, .) passes no gradient
 *      where it clamps (the pair's rgb still gets its own).  max(0, rgb) passes none where it clamps: not to colour and
 *      sh, and not to the position through the view direction.  The clamp of x/z and y/z in J passes none through the
 *      clamped quotient where it clamps (J still depends on z there); where it does not clamp, J's dependence on the
 *      position is differentiated.  The position gets gradient through the mean, through J and through the normalised
 *      view direction of the sh bands; the quaternion through its normalisation to the raw xyzw.  With the antialiased
 *      flag sqrt(max(0, det_before) / det_after) is differentiated, and is zero where det_before <= 0.  The background
 *      term T_final background and the alpha channel 1 - T_final are part of the image and are differentiated.  Sh
 *      coefficients above min(file degree, max_sh_degree) get exactly 0; an invisible Gaussian gets exactly 0 in every
 *      array.  Every element of the six arrays is written (not accumulated into).
 *      Arithmetic.  The blend's part re-evaluates power, a, T' and the three tests with the forward blend's f32
 *      expressions, so it uses the pairs the image used, and forms each used pair's gradient to the record's nine floats
 *      (mean 2, conic 3, opacity 1, rgb 3) in f32.  They are summed per Gaussian with f32 atomic adds, in an order that
 *      is not fixed: a run need not repeat its bits.  The per-Gaussian chain from those nine values to the six arrays
 *      runs in f64 from the f32 inputs, like the forward's preprocess, and uses no atomics.
 *
 *      render_backward_workspace_bytes (host only): device memory for the n x 9 record gradients.
 *      render_backward_device: d_cloud, num_points, sh_degree, antialiased, params and max_entries as given to
 *      prepare_cloud_device and render_finish_device; d_render_workspace exactly as render_finish_device left it (the
 *      records, the sorted entries, the tile ranges and the total are read; nothing is sorted again and nothing in it is
 *      written).  d_image: the image render_finish_device wrote, or NULL; it is not read, because alpha = 1 - T_final
 *      keeps T_final only to 2^-24 absolute: each pixel's final colour sum and T are blended again instead.
 *      d_grad_image: G.  d_grads: six device pointers (sh may be NULL iff sh_degree == 0).  d_record_grads (may be NULL):
 *      n x 9 floats out, the record gradients in input order.  *d_status (device memory, uint32) = 0, or 1 when the
 *      total is above max_entries: then no gradient is written.  Arguments are checked on the host before any launch
 *      (a bad one: SPZ_AMD_ERR_INVALID_ARG; no device: SPZ_AMD_ERR_NO_DEVICE).  Enqueues on hip_stream and does not
 *      synchronise. */
typedef struct {
  float *positions, *scales, *rotations, *alphas, *colors, *sh;
} spz_amd_cloud_grads;

uint64_t spz_amd_render_backward_workspace_bytes(uint64_t num_points);
int spz_amd_render_backward_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree, int antialiased,
                                   const spz_amd_render_params *params, uint64_t max_entries, const float *d_image,
                                   const float *d_grad_image, const spz_amd_cloud_grads *d_grads, float *d_record_grads,
                                   uint32_t *d_status, const void *d_render_workspace, void *d_backward_workspace,
                                   void *hip_stream);

/* ---- render depth backward: the gradients of one view's image AND accumulated depth to a float cloud
 *      (spz_render_backward.hip; DESIGN §8 "Depth fit").  The reference has no counterpart.  "render backward" with
 *      the depth sum of "render depth" in it: given G (height x width x 4 float32, or NULL for all zero), the gradient
 *      of a scalar loss to the image, and G_D (height x width float32), its gradient to channel 0 of d_depth (the
 *      un-normalised sum D of (T a) z over the used pairs, z the record's f32 depth), it produces that loss's gradient
 *      to the six arrays.  The median channel and the index are discrete and carry no gradient.
 *      Everything "render backward" holds constant is held constant here, and depth adds no decision.  Per used pair
 *      i, with T the transmittance before it, w = T a, C_i and D_i the prefixes that include it, C_f, D_f and T_f the
 *      pixel's finals and tail = T_f (g_rgb . bg - g_alpha):
 *        dL/drgb_i = w g_rgb;  dL/dz_i = w g_D;
 *        dL/da_i = T (g_rgb . rgb_i + g_D z_i) - (g_rgb . (C_f - C_i) + g_D (D_f - D_i) + tail) / (1 - a),
 *      and dL/da reaches opacity and power only where a = min(0.99, .) does not clamp.  The ten values per Gaussian are
 *      summed with f32 atomic adds (a run need not repeat its bits).  The chain is that of "render backward" with one
 *      more term: z = (R p + t)_z is computed in f64 and rounded to f32, straight through, so dL/dp += R[2, :] dL/dz
 *      in f64.
 *
 *      render_depth_backward_workspace_bytes (host only): device memory for the n x 9 record gradients and the n
 *      depth gradients.  render_depth_backward_device: as render_backward_device, with d_render_workspace as
 *      render_finish_device OR render_depth_device left it (both leave the same records, entries, ranges and total).
 *      d_grad_image: G, may be NULL.  d_grad_depth: G_D.  d_record_grads (may be NULL): n x 9 floats out;
 *      d_depth_grads (may be NULL): n floats out, dL/dz per Gaussian in input order.  *d_status = 0, or 1 when the
 *      total is above max_entries: then no gradient is written.  Every element of the six arrays is written; an
 *      invisible Gaussian gets exact zeros.  Arguments are checked on the host before any launch, with
 *      render_backward_device's codes.  Enqueues on hip_stream and does not synchronise. */
uint64_t spz_amd_render_depth_backward_workspace_bytes(uint64_t num_points);
int spz_amd_render_depth_backward_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree,
                                         int antialiased, const spz_amd_render_params *params, uint64_t max_entries,
                                         const float *d_grad_image, const float *d_grad_depth,
                                         const spz_amd_cloud_grads *d_grads, float *d_record_grads, float *d_depth_grads,
                                         uint32_t *d_status, const void *d_render_workspace, void *d_backward_workspace,
                                         void *hip_stream);

/* ---- render scores: per-Gaussian blend weights of one view (spz_render.hip; DESIGN §8 "Prune").  The reference has
 *      no counterpart.  With the workspace of a prepare step (as for render_finish_device), the blend of the render
 *      contract runs again, pixel for pixel; for every (pixel i, Gaussian j) pair the blend USES (not skipped for power
 *      > 0 or a < 1/255, and not the Gaussian whose T' would fall under 1e-4, which ends the pixel unused):
 *        w_ij = T a in f32, exactly as the blend computes it;  q_ij = rint(w_ij 2^24), an integer: w <= 0.99, so
 *        q < 2^24, and w >= 1e-4 / 255, so q >= 7 (a Gaussian's sum is 0 exactly when it was never used);
 *        d_weight_sum[j] += sum_i q_ij (uint64: at most 2^52 per view of <= 2^28 pixels, so 1024 views stay below
 *        2^62, which torch's int64 holds);  d_weight_max[j] = max(d_weight_max[j], max_i w_ij) (f32, 0 when unused).
 *      Integer sums and f32 maxima do not depend on the order of the additions: a run repeats its bits, and a stream and
 *      its decoded floats give the same scores.  No float atomics (vector integer atomics in LDS and global memory).
 *      sum_j weight_sum_j 2^-24 over a view is the image's alpha sum (sum_i 1 - T_i), to the rounding of q.
 *      Removing the Gaussians of zero sum keeps every scoring view's image, with one caveat: the Gaussian that ends a
 *      pixel (T' = T (1 - a) < 1e-4) is not counted there, so when it scores zero everywhere, removing it lets the
 *      Gaussians behind it into that pixel.  Such a pixel had T < 1e-4 / (1 - a) <= 0.01 (a <= 0.99), so alpha >=
 *      0.99, and each channel moves by at most T (max |rgb| + |background|).
 *      render_score_device: the entries, their sort and ranges as render_finish_device, then the scoring blend; the
 *      caller zeroes d_weight_sum (uint64[n]) and d_weight_max (f32[n]) once and loops over views (prepare, score).
 *      d_image (may be NULL): the image, bit-identical to render_finish_device's.  *d_status = 0, or 1 when the total
 *      is above max_entries: then neither the image nor the scores are touched.  Enqueue only; no synchronisation.
 *
 * ---- prune: significance pruning over a set of views (spz_prune.hip; DESIGN §8 "Prune").  Versions 1, 2 and 3.
 *      views: 1..SPZ_AMD_PRUNE_MAX_VIEWS render params, each passing render_check_params, all with one coord (the
 *      frame the file is decoded to); background and max_sh_degree do not change a weight.  Per view: prepare, the
 *      total read back, the workspace grown (grow-only), score.  A total above 2^31 - 1: SPZ_AMD_ERR_CAPACITY.
 *      score_kind: SPZ_AMD_PRUNE_SCORE_SUM (weight_sum) or _MAX (weight_max).  Rank: score descending, then input
 *      index ascending, exact on the u64 / u32 keys (a stable radix sort).  rule (exactly one):
 *        KEEP_COUNT K = rule_value, an integer in 0..n;  KEEP_FRACTION f = rule_value in [0, 1], K = min(n, ceil(f n))
 *        in f64 (spz_amd_prune_keep_count, host only, computes K);  MIN_SCORE s = rule_value, finite: keep j iff
 *        score_j >= s, the sum compared as q 2^-24 (pixel units) in f64.
 *      Output: spz_amd_select_device + spz_amd_subset_device of the kept indices at the input's degree, so the stream
 *      is byte-identical to the filter's with the keep mask.  A bad argument is SPZ_AMD_ERR_INVALID_ARG before anything
 *      is launched.  open (shaped like clean's) runs on `device` on a stream of its own and blocks.  *h_kept (may be
 *      NULL): the kept count; h_mask (may be NULL): n bytes, 1 = kept; h_weight_sum / h_weight_max (may be NULL): n
 *      uint64 / f32; h_ms (may be NULL): [0] wall-clock milliseconds of the views' scores, [1] of the rank and mask,
 *      [2] of the subset; *h_bad_view (may be NULL): the index of the view a failure concerns (a bad view, a
 *      different coord, the entry cap), else -1. */
enum {
  SPZ_AMD_PRUNE_MAX_VIEWS = 1024,
  SPZ_AMD_PRUNE_SCORE_SUM = 0,
  SPZ_AMD_PRUNE_SCORE_MAX = 1,
  SPZ_AMD_PRUNE_KEEP_COUNT = 0,
  SPZ_AMD_PRUNE_KEEP_FRACTION = 1,
  SPZ_AMD_PRUNE_MIN_SCORE = 2
};
int spz_amd_render_score_device(uint64_t num_points, const spz_amd_render_params *params, uint64_t max_entries,
                                float *d_image, uint64_t *d_weight_sum, float *d_weight_max, uint32_t *d_status,
                                void *d_workspace, void *hip_stream);
int spz_amd_prune_keep_count(uint64_t num_points, int rule, double rule_value, uint64_t *k);
int spz_amd_prune_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                       const spz_amd_render_params *views, int num_views, int score_kind, int rule, double rule_value,
                       int device, void **ctx, uint64_t *h_out_bytes, uint64_t *h_kept, uint8_t *h_mask,
                       uint64_t *h_weight_sum, float *h_weight_max, float *h_ms, int32_t *h_bad_view);
int spz_amd_prune_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_prune_device_data(void *ctx);
void spz_amd_prune_close(void *ctx);

/* ---- render depth: expected depth, median depth and the median Gaussian of one view (spz_render.hip; DESIGN §8
 *      "Render").  The reference has no counterpart.  With the workspace of a prepare step (as for
 *      render_finish_device), the blend of the render contract runs again, pixel for pixel: the same skips, the same
 *      stop, the same f32 operations in the same order.  For every pair the blend USES (as "render scores" defines it),
 *      with z the record's f32 depth and g the Gaussian's input index, D = 0 at first:
 *        D = D + (T a) z in f32: w = T a, then w z, then the add, not contracted;
 *        after T' = T (1 - a): when no median has been taken and T' < 0.5f, median depth = z and median index = g.
 *      d_depth: height x width x 2 f32.  Channel 0 = D, un-normalised (0 where nothing was blended); channel 1 = the
 *      median depth, +inf when T never fell below 0.5.  d_index (may be NULL): height x width u32, the median
 *      Gaussian's input index, 0xffffffff without a median.  d_image (may be NULL): the image, bit-identical to
 *      render_finish_device's.  The normalised expected depth is D / alpha in f32 where alpha = 1 - T > 0, +inf
 *      elsewhere: the layers above derive it, the kernel does not.  No atomics: a run repeats its bits, and a stream and
 *      its decoded floats give the same bits.
 *      render_depth_device: the entries, their sort and ranges as render_finish_device, then the depth blend.
 *      *d_status = 0, or 1 when the total is above max_entries: then nothing is written to the three outputs.  A NULL
 *      d_depth, d_status or d_workspace or bad params: SPZ_AMD_ERR_INVALID_ARG; max_entries above 2^31 - 1:
 *      SPZ_AMD_ERR_CAPACITY; both before anything is launched.  Enqueue only; no synchronisation.
 *      render_depth_host / render_depth_cloud_host: as render_host / render_cloud_host.  h_rgba (may be NULL): height x
 *      width x 4 floats; h_depth: height x width x 2 floats; h_index (may be NULL): height x width u32; h_ms[2]: the
 *      depth blend.  A total above 2^31 - 1: SPZ_AMD_ERR_CAPACITY. */
int spz_amd_render_depth_device(uint64_t num_points, const spz_amd_render_params *params, uint64_t max_entries,
                                float *d_image, float *d_depth, uint32_t *d_index, uint32_t *d_status,
                                void *d_workspace, void *hip_stream);
int spz_amd_render_depth_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                              const spz_amd_render_params *params, int device, float *h_rgba, float *h_depth,
                              uint32_t *h_index, uint64_t *h_entries, float *h_ms);
int spz_amd_render_depth_cloud_host(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_degree,
                                    int antialiased, const spz_amd_render_params *params, int device, float *h_rgba,
                                    float *h_depth, uint32_t *h_index, uint64_t *h_entries, float *h_ms);

/* ---- mesh: a triangle mesh of a scene (spz_mesh.hip; DESIGN §8 "Mesh").  The reference has no counterpart.  Depth
 *      maps of a set of views are fused into a truncated signed distance volume (TSDF), and the zero level set of the
 *      volume is extracted by marching tetrahedra: vertices, per-vertex colours and triangles.
 *
 *      The volume.  A lattice of nx x ny x nz sample points at lo + (i, j, k) s in the views' coord frame (dims = nx,
 *      ny, nz; s = voxel_size).  Each dimension 2..2048, nx ny nz <= 2^28, s and truncation finite and > 0, lo finite.
 *      The grid is five f32 planes of nx ny nz values each, in this order: W (weight), S (sum of truncated distances),
 *      Cr, Cg, Cb (colour sums); the linear index of a point is (k ny + j) nx + i.  A new grid is all zero.
 *      tsdf_check, tsdf_bytes (20 nx ny nz; 0 for a bad volume) and tsdf_volume_from_box are host only.
 *      volume_from_box: lo = (float)lo, dims_a = floor((hi_a - lo_a) / s) + 2 in f64 (the lattice reaches past hi),
 *      hi_a >= lo_a; a dimension above 2048 or a lattice above 2^28: SPZ_AMD_ERR_INVALID_ARG.
 *
 *      Fuse (tsdf_integrate_device): one view into the grid.  d_depth (H x W x 2) and d_image (H x W x 4) exactly as
 *      render_depth_device writes them; depth_kind SPZ_AMD_MESH_DEPTH_MEDIAN or _EXPECTED; min_alpha in [0, 1].  Per
 *      lattice point, every operation rounded on its own (no contraction):
 *        p = lo + (i, j, k) s in f64 from the f32 fields;  p_c = R p + t in f64, each row ((R0 px + R1 py) + R2 pz) + t;
 *        z = p_c.z; skip unless z > near_plane.  u = floor(fx (x / z) + cx), v = floor(fy (y / z) + cy) (the render's
 *        pixel centre is at index + 0.5); skip unless 0 <= u < W and 0 <= v < H.
 *        MEDIAN: D = depth[v][u][1].  EXPECTED: a = image[v][u][3], skip unless a >= min_alpha, D = depth[v][u][0] / a
 *        in f32.  Skip unless D is finite and > 0.  sdf = (double)D - z; skip if sdf < -truncation;
 *        d = (float)min(1.0, sdf / truncation).  Then, with f32 adds: W += 1, S += d, C += image[v][u][0..2] (unclamped).
 *      A skipped point is not written.  No atomics; views are fused one call after another, so a run repeats its bits,
 *      and a stream and its decoded floats give the same grid.  background and max_sh_degree of params are not read.
 *      Projective fusion marks up to `truncation` behind a surface seen at a grazing angle as inside: a known artefact
 *      of the method, which opens the mesh at the limbs of a view set.
 *
 *      Extract (mesh_count_device, mesh_emit_device).  f = S / W (f32 division) at a lattice point; inside iff f < 0.
 *      A cube is the 8 points (i..i+1, j..j+1, k..k+1); it is valid iff all 8 have W >= min_weight (finite, > 0); only
 *      valid cubes emit.  Corners are numbered dx + 2 dy + 4 dz.  Each cube splits into the six Kuhn tetrahedra around
 *      the diagonal from corner 0 to corner 7: for the axis permutations p in lexicographic order (xyz, xzy, yxz, yzx,
 *      zxy, zyx) v0 = corner 0, v1 = v0 + e_p0, v2 = v1 + e_p1, v3 = corner 7.  Cubes that share a face split it along
 *      the same diagonal, so the surface is watertight across cubes.
 *      Every tet edge runs from a lattice point a to a + delta, delta in {0,1}^3 \ {0}; its id is 7 lin(a) + (dx + 2 dy
 *      + 4 dz - 1).  One vertex per edge that at least one emitted triangle uses.  t = f_a / (f_a - f_b) in f64;
 *      position = lo + (idx_a + t delta) s per axis in f64, rounded to f32; colour = c_a + t (c_b - c_a) with c = C / W
 *      (f32 division), in f64, rounded to f32.
 *      Tet edges are numbered by vertex pairs (0,1), (0,2), (0,3), (1,2), (1,3), (2,3).  One vertex i alone on its
 *      side: one triangle, the three edges at i in ascending number.  A 2-2 split {0, j} | {k, l}, k < l: the quad q =
 *      (0k, 0l, jl, jk) as (q0, q1, q2) and (q0, q2, q3).  A triangle's last two indices are swapped where needed so
 *      that (b - a) x (c - a) points from the centroid of the tet's inside vertices to that of its outside vertices,
 *      judged with the edge midpoints as positions.  The table is generated from this rule (mesh_tet_table, host only:
 *      corners[tet][4], num_triangles[tet][mask], edges[tet][mask][6], mask bit v = tet vertex v inside).
 *      Order: vertices in ascending edge id; triangles by ascending cube (linear index of corner 0), then tet, then
 *      the case's order.  No atomic decides an order: a run repeats its bits.  Where f == 0 exactly at a lattice point
 *      the triangles around it have zero area; they are kept, because the topology stays manifold.
 *      mesh_workspace_bytes (host only; 0 for a bad volume): 33 bytes per lattice point (a dense edge map) and the
 *      scans' block sums.  mesh_count_device: the classification and the two scans; d_counts (device memory, 2 uint64)
 *      = the number of vertices, of triangles.  The caller reads them back once, then mesh_emit_device with the same
 *      volume, grid and workspace writes d_positions and d_colors (num_vertices x 3 f32) and d_triangles
 *      (num_triangles x 3 u32).  A capacity below its count: SPZ_AMD_ERR_CAPACITY, nothing written.  The host form
 *      refuses more than 2^32 - 1 vertices the same way.
 *      All device forms check their arguments on the host before any launch (a bad one: SPZ_AMD_ERR_INVALID_ARG; no
 *      device: SPZ_AMD_ERR_NO_DEVICE), enqueue on hip_stream and do not synchronise.
 *
 *      The host form (mesh_open / _fetch / _close, shaped like prune's) takes a stream already in device memory.
 *      views: 1..SPZ_AMD_MESH_MAX_VIEWS, each passing render_check_params, all with one coord.  options (mesh_check,
 *      host only): has_box and box = lo xyz, hi xyz with hi > lo; exactly one of voxel_size (> 0) and resolution
 *      (1..2046 lattice cells along the longest side of the box; mesh_default_options sets 256) non-zero; truncation
 *      (0: 4 voxel_size); depth_kind; min_alpha; min_weight.  Without a box: the exact bounding box of the file's
 *      finite decoded positions in coord, computed on the device (no finite position: SPZ_AMD_ERR_INVALID_ARG); a
 *      file with floaters wants a clean first, or a box.  Per view: prepare, render_depth_device, the fuse; then the
 *      extraction.  It runs on `device` on a stream of its own and blocks.  h_counts[2]: vertices, triangles;
 *      *h_volume (may be NULL): the volume used; h_ms (may be NULL): [0] wall-clock milliseconds of the views' renders,
 *      [1] of the fuses, [2] of the extraction; *h_bad_view (may be NULL): the view a failure concerns, else -1.  An
 *      entry total above 2^31 - 1: SPZ_AMD_ERR_CAPACITY.  mesh_fetch: the three arrays into host memory. */
enum { SPZ_AMD_MESH_MAX_VIEWS = 1024, SPZ_AMD_MESH_DEPTH_MEDIAN = 0, SPZ_AMD_MESH_DEPTH_EXPECTED = 1 };
typedef struct {
  float lo[3];
  float voxel_size;
  uint32_t dims[3];
  float truncation;
} spz_amd_tsdf_volume;
typedef struct {
  double box[6];
  double voxel_size;
  double truncation;
  int32_t has_box;
  int32_t resolution;
  int32_t depth_kind;
  float min_alpha;
  float min_weight;
  int32_t reserved;
} spz_amd_mesh_options;

int spz_amd_tsdf_check(const spz_amd_tsdf_volume *volume);
uint64_t spz_amd_tsdf_bytes(const spz_amd_tsdf_volume *volume);
int spz_amd_tsdf_volume_from_box(const double lo[3], const double hi[3], double voxel_size, double truncation,
                                 spz_amd_tsdf_volume *out);
int spz_amd_tsdf_integrate_device(const spz_amd_tsdf_volume *volume, float *d_grid, const spz_amd_render_params *params,
                                  const float *d_depth, const float *d_image, int depth_kind, float min_alpha,
                                  void *hip_stream);
int spz_amd_mesh_tet_table(uint8_t corners[24], uint8_t num_triangles[96], uint8_t edges[576]);
uint64_t spz_amd_mesh_workspace_bytes(const spz_amd_tsdf_volume *volume);
int spz_amd_mesh_count_device(const spz_amd_tsdf_volume *volume, const float *d_grid, float min_weight,
                              uint64_t *d_counts, void *d_workspace, void *hip_stream);
int spz_amd_mesh_emit_device(const spz_amd_tsdf_volume *volume, const float *d_grid, uint64_t num_vertices,
                             uint64_t num_triangles, uint64_t vertex_capacity, uint64_t triangle_capacity,
                             float *d_positions, float *d_colors, uint32_t *d_triangles, const void *d_workspace,
                             void *hip_stream);
int spz_amd_mesh_default_options(spz_amd_mesh_options *options);
int spz_amd_mesh_check(const spz_amd_mesh_options *options);
int spz_amd_mesh_open(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, const spz_amd_render_params *views,
                      int num_views, const spz_amd_mesh_options *options, int device, void **ctx, uint64_t *h_counts,
                      spz_amd_tsdf_volume *h_volume, float *h_ms, int32_t *h_bad_view);
int spz_amd_mesh_fetch(void *ctx, float *h_positions, float *h_colors, uint32_t *h_triangles);
void spz_amd_mesh_close(void *ctx);

/* ---- seed: Gaussians from posed RGB-D views (spz_seed.hip; DESIGN §8 "Seed").  The reference has no counterpart.
 *      Each view's valid depth samples that the cloud built so far does not already explain are lifted to Gaussians
 *      and appended to a float cloud, view after view in the order given.
 *
 *      Inputs per view.  params: a pinhole view as "render" defines it, in its coord frame (background and
 *      max_sh_degree are not read).  image: height x width x channels f32, channels 3 or 4, rows top to bottom.  depth:
 *      height x width f32, metric z in scene units; a value that is not finite or not > near_plane is no measurement.
 *      weights (may be NULL): height x width f32; a sample counts when its weight is > 0.5.
 *      Options (seed_default_options; seed_check, host only, refuses anything else with SPZ_AMD_ERR_INVALID_ARG):
 *      stride 1..64 (1); scale_factor > 0, finite (1); alpha, the pre-sigmoid opacity, finite (0: opacity 0.5; the
 *      layers above take opacity in (0, 1) and convert once); cover_alpha in [0, 1] (0.5); cover_tolerance >= 0,
 *      finite, relative (0.05); cover 0 or 1 (1); sh_degree 0..3 (0).
 *
 *      Lattice.  The samples are the pixels u = stride i + stride / 2, v = stride j + stride / 2 (integer division) for
 *      all i, j >= 0 with u < width and v < height, in row-major (j, i) order; seed_samples (host only) counts them (0
 *      for a size or stride out of range).  A sample is valid when its depth is a measurement, its weight (if given)
 *      counts and its three colour values are finite; the tests run in that order and a plane is not read after a
 *      test before it failed.
 *      Cover test: only with cover set, num_points > 0 and the two maps given.  d_cover_image (height x width x 4) and
 *      d_cover_depth (height x width x 2) are render_depth_device's image and depth of the cloud so far for this view,
 *      prepared with antialiased = 0, max_sh_degree = sh_degree and background 0.  A valid sample is covered when
 *      A = image alpha >= cover_alpha and |e - d| <= cover_tolerance d, e = depth[..][0] / A in f32 (expected_depth's
 *      division), the difference, the product and the comparison in f64 from the f32 values.
 *      Selection: the valid, uncovered samples in lattice order.  The first capacity - num_points of them are
 *      appended, at num_points + rank; the rest are counted as refused.
 *      Each appended Gaussian, in f64 from the f32 inputs, operations in the order written, no contraction, each
 *      result rounded to f32 once: z = d; q = (((u + 0.5 - cx) / fx) z - t_x, ((v + 0.5 - cy) / fy) z - t_y, z - t_z);
 *      position_k = (q_x R[0][k] + q_y R[1][k]) + q_z R[2][k], which is R^T (z ray - t); the three log scales =
 *      log((((scale_factor stride) z) 0.5) (1 / fx + 1 / fy)), the lattice's world-space spacing at that depth;
 *      rotation (0, 0, 0, 1); alpha = the option; colour = (rgb - 0.5) / C0 with the render's C0; sh zeros.
 *      No atomics: a scan of per-block counts fixes the order, and a run repeats its bytes.
 *
 *      seed_workspace_bytes (host only; 0 for a size or stride out of range): a flag byte per sample and the block
 *      counts.  seed_view_device: d_cloud's six arrays hold num_points Gaussians and have room for capacity (<= 2^31 -
 *      1; sh may be NULL iff sh_degree == 0); sh_degree must equal the options'.  d_counts (device memory, 3 uint64):
 *      valid, appended, refused.  Arguments are checked on the host before any launch (a bad one:
 *      SPZ_AMD_ERR_INVALID_ARG; no device: SPZ_AMD_ERR_NO_DEVICE).  It enqueues on hip_stream and does not synchronise;
 *      the caller renders, so a cloud that is being trained can be seeded in place.
 *
 *      The host form (seed_open / _fetch / _device_data / _close, shaped like decimate's).  views: 1..
 *      SPZ_AMD_SEED_MAX_VIEWS, each passing render_check_params, all with one coord.  h_images, channels, h_depths:
 *      one per view, host memory; h_weights: NULL, or one pointer per view, each of which may be NULL.  base_hdr NULL:
 *      the cloud starts empty.  Otherwise d_base / base_size / base_hdr is a stream already in device memory whose
 *      degree equals sh_degree (else SPZ_AMD_ERR_SH_DEGREE); it is decoded to coord as the start of the cloud and is
 *      used for the cover test only.  max_points: the most new points (0: the sum of the views' sample counts, at most
 *      SPZ_AMD_REFERENCE_MAX_POINTS; above that: SPZ_AMD_ERR_TOO_MANY_POINTS).  Per view: with cover set and a
 *      non-empty cloud, prepare (the entry total read back once, the workspace grown), render_depth_device; then the
 *      upload and seed_view_device.  The output is the NEW points alone, encoded from coord under a fresh version 3
 *      header (12 fractional bits, not antialiased); spz_amd_merge_* joins it to the base without requantising.
 *      h_counts (may be NULL): 3 uint64 per view; *h_num_points (may be NULL): the points written; h_ms (may be NULL):
 *      [0] wall-clock milliseconds of the cover renders, [1] of the uploads, selects and emits, [2] of the encode;
 *      *h_bad_view (may be NULL): the view a failure concerns, else -1.  An entry total above 2^31 - 1:
 *      SPZ_AMD_ERR_CAPACITY.  It runs on `device` on a stream of its own and blocks. */
enum { SPZ_AMD_SEED_MAX_VIEWS = 1024 };
typedef struct {
  uint32_t stride;
  float scale_factor;
  float alpha;
  float cover_alpha;
  float cover_tolerance;
  int32_t cover;
  int32_t sh_degree;
  int32_t reserved;
} spz_amd_seed_options;

int spz_amd_seed_default_options(spz_amd_seed_options *options);
int spz_amd_seed_check(const spz_amd_seed_options *options);
uint64_t spz_amd_seed_samples(uint32_t width, uint32_t height, uint32_t stride);
uint64_t spz_amd_seed_workspace_bytes(uint32_t width, uint32_t height, uint32_t stride);
int spz_amd_seed_view_device(const spz_amd_cloud_out *d_cloud, uint64_t num_points, uint64_t capacity, int sh_degree,
                             const spz_amd_render_params *params, const spz_amd_seed_options *options,
                             const float *d_image, int channels, const float *d_depth, const float *d_weights,
                             const float *d_cover_image, const float *d_cover_depth, uint64_t *d_counts,
                             void *d_workspace, void *hip_stream);
int spz_amd_seed_open(const spz_amd_render_params *views, int num_views, const spz_amd_seed_options *options,
                      const float *const *h_images, const int32_t *channels, const float *const *h_depths,
                      const float *const *h_weights, const uint8_t *d_base, size_t base_size,
                      const spz_amd_header *base_hdr, uint64_t max_points, int device, void **ctx,
                      uint64_t *h_out_bytes, uint64_t *h_counts, uint64_t *h_num_points, float *h_ms,
                      int32_t *h_bad_view);
int spz_amd_seed_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_seed_device_data(void *ctx);
void spz_amd_seed_close(void *ctx);

/* ---- image metrics: PSNR, MSE, L1, max error and SSIM of two images (spz_metrics.hip; DESIGN §8 "Compare").  The
 *      reference has no counterpart.  The convention of the 3DGS evaluation code (Kerbl et al. 2023, loss_utils.ssim and
 *      image_utils.psnr), so the numbers compare with published tables.
 *
 *      Inputs.  Two images a, b, each height x width x C float32, row-major and contiguous, C in {3, 4}; the two may
 *      have different C (a render's RGBA against a photo's RGB).  Only the first three channels are used.  Each used
 *      value is clamped first: v = fminf(fmaxf(v, 0), 1), so NaN becomes 0, +inf 1 and -inf 0 (a render's images are
 *      not clamped).  width, height 1..16384.
 *      Per pixel, with d = a - b on the clamped values (f64):  mse = sum d^2 / (3 H W);  psnr = 10 log10(1 / mse), or +inf
 *      when mse == 0;  l1 = sum |d| / (3 H W);  max_abs = max |d|.
 *      SSIM, per channel.  Window g: the 11x11 Gaussian, the outer product of w_k = exp(-(k - 5)^2 / (2 1.5^2)) / sum_j
 *      exp(-(j - 5)^2 / (2 1.5^2)), k = 0..10.  Convolution: "same" size with zero padding (pixels outside the image
 *      count as 0 and stay in the window's weight, as conv2d(padding = 5)), separable: along rows, then along columns,
 *      taps in k order, in f64.  mu_a = g*a, mu_b = g*b, s_a = g*a^2 - mu_a^2, s_b = g*b^2 - mu_b^2, s_ab = g*(ab) -
 *      mu_a mu_b;  S = ((2 mu_a mu_b + C1)(2 s_ab + C2)) / ((mu_a^2 + mu_b^2 + C1)(s_a + s_b + C2)), C1 = 0.01^2,
 *      C2 = 0.03^2.  ssim = the mean of S over all 3 H W values.  The SSIM map (optional): height x width float32, the
 *      mean of S over the three channels at each pixel.
 *      Precision against a float64 restatement: mse, l1 and max_abs within 1e-12 relative, ssim within 1e-7 absolute,
 *      each map value within 1e-6.  Deterministic: no float atomics; each workgroup writes its partial sums to a slab in
 *      a fixed order and one pass reduces the slab in a fixed order (max_abs through the u64 bit pattern of the f64
 *      |d|).  A run repeats its bits, and swapping a and b gives bit-identical results (every expression is symmetric).
 *
 *      image_metrics_check (host only, no GPU): SPZ_AMD_ERR_INVALID_ARG when a side is outside 1..16384 or a channel
 *      count is not 3 or 4.  image_metrics_workspace_bytes (host only): device memory for the device form (0 for a bad
 *      size).  image_metrics_device: enqueues on hip_stream, no synchronisation; *d_out (device memory, 8-aligned) gets
 *      the five results; d_ssim_map (device memory, may be NULL); d_workspace 8-aligned.  image_metrics_host: host
 *      images in, *h_out and h_ssim_map (may be NULL) out, on `device`, blocking.
 *
 * ---- compare: two packed streams rendered from a set of views, and the metrics above of each view's two images
 *      (spz_metrics.hip; DESIGN §8 "Compare").  Versions 1, 2 and 3; the two streams may differ in point count, SH degree
 *      and version.  views: 1..SPZ_AMD_COMPARE_MAX_VIEWS render params, each passing render_check_params, all with one
 *      coord (a bad one: SPZ_AMD_ERR_INVALID_ARG before anything is launched, the view in *h_bad_view).  Per view: A
 *      rendered, B rendered (render_prepare_packed_device, the total read back, render_finish_device: the images are
 *      bit-identical to render_host's), then image_metrics_device of the two RGBA images.  The render workspace and
 *      the two images are grow-only and reused across views.  A 0-point input renders as render_host renders it (the
 *      background, alpha 0).  A total above 2^31 - 1: SPZ_AMD_ERR_CAPACITY, the view in *h_bad_view.  Runs on `device`
 *      on a stream of its own and blocks.  h_metrics: num_views results; h_ssim_maps (may be NULL): sum_i W_i H_i floats,
 *      view after view; h_entries (may be NULL): 2 num_views totals, A then B per view; h_ms (may be NULL): [0]
 *      wall-clock milliseconds of the renders, [1] of the metrics; *h_bad_view (may be NULL): the view a failure
 *      concerns, else -1. */
enum { SPZ_AMD_COMPARE_MAX_VIEWS = 1024 };
typedef struct {
  double mse, psnr, ssim, l1, max_abs;
} spz_amd_image_metrics;
int spz_amd_image_metrics_check(int width, int height, int channels_a, int channels_b);
uint64_t spz_amd_image_metrics_workspace_bytes(int width, int height);
int spz_amd_image_metrics_device(const float *d_a, int channels_a, const float *d_b, int channels_b, int width,
                                 int height, spz_amd_image_metrics *d_out, float *d_ssim_map, void *d_workspace,
                                 void *hip_stream);
int spz_amd_image_metrics_host(const float *h_a, int channels_a, const float *h_b, int channels_b, int width,
                               int height, int device, spz_amd_image_metrics *h_out, float *h_ssim_map);
int spz_amd_compare_host(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                         const uint8_t *d_stream_b, size_t size_b, const spz_amd_header *hdr_b,
                         const spz_amd_render_params *views, int num_views, int device,
                         spz_amd_image_metrics *h_metrics, float *h_ssim_maps, uint64_t *h_entries, float *h_ms,
                         int32_t *h_bad_view);

/* ---- image loss: the 3DGS training loss of a render against a target, and its gradient to the render
 *      (spz_metrics.hip; DESIGN §8 "Refine").  The reference has no counterpart.
 *        L = (1 - lambda) l1 + lambda (1 - ssim)           (Kerbl et al. 2023, loss_utils)
 *      with l1 and ssim exactly the quantities of "image metrics" above: the first three channels, each value clamped to
 *      [0, 1] first (NaN -> 0), the 11x11 window with zero padding, means over 3 H W, in f64.  lambda in [0, 1].
 *      Inputs.  a (the render) and b (the target): height x width x C float32, C in {3, 4}, independently; width,
 *      height 1..16384 (image_metrics_check).  d_loss (device memory, 8-aligned): three doubles, L, l1 and ssim; l1 and
 *      ssim carry the bits image_metrics_device gives for the same pair.  d_grad (device memory): dL/da, height x width
 *      x C_a float32; with C_a = 4 it is the d_grad_image of render_backward_device.
 *      Gradient.  Every element of d_grad is written.  A fourth channel gets exactly 0.  The clamp passes gradient where
 *      0 <= a <= 1, both ends included (as torch.clamp: a render over a black background is exactly 0 over much of the
 *      image), and nothing elsewhere or for NaN.  The L1 part is sign(a - b) / (3 H W) on the clamped values, sign(0) =
 *      0.  The SSIM part, per channel and window q with A1 = 2 mu_a mu_b + C1, A2 = 2 s_ab + C2, B1 = mu_a^2 + mu_b^2 +
 *      C1, B2 = s_a + s_b + C2, S = A1 A2 / (B1 B2):  P = 2 A1 / (B1 B2) (to g*(ab)), Q = -S / B2 (to g*a^2), M =
 *      2 mu_b (A2 - A1) / (B1 B2) - 2 mu_a S (1 / B1 - 1 / B2) (to mu_a, in total);  d ssim / d a(p) = ((g*M)(p) +
 *      2 a(p) (g*Q)(p) + b(p) (g*P)(p)) / (3 H W), the same zero-padded "same" convolutions, the maps zero outside the
 *      image.  dL/da = (1 - lambda) dl1/da - lambda dssim/da.
 *      Arithmetic.  Two passes: the metrics' tile pass, which also stores M, Q and P of each channel as nine f64 planes,
 *      and a tile pass that filters them.  Everything is f64 up to the one rounding of each gradient value to f32.  No
 *      float atomics; the partial sums go through the metrics' slab in its fixed order: a run repeats its bits.
 *      image_loss_workspace_bytes (host only): device memory for the device form, 72 H W bytes and the slab (0 for a bad
 *      size).  image_loss_device: arguments checked on the host before any launch (SPZ_AMD_ERR_INVALID_ARG; no device:
 *      SPZ_AMD_ERR_NO_DEVICE); enqueues on hip_stream and does not synchronise.
 *
 * ---- adam step: one Adam update of the trained arrays of a float cloud (spz_refine.hip; DESIGN §8 "Refine").  The
 *      reference has no counterpart.  d_params, d_grads, d_m, d_v: the six arrays (as spz_amd_cloud_in orders and shapes
 *      them), their gradients and their first and second moments.  train_mask: bit 0 positions, 1 scales, 2 rotations,
 *      3 alphas, 4 colours, 5 sh; non-zero.  An array whose bit is clear is neither read nor written, and its four
 *      pointers may be NULL; sh may be NULL when sh_degree == 0 as well.
 *      Scalars (spz_amd_adam_scalars_of, host only, computes them in f64 for step t >= 1 and rounds each to f32):
 *      beta1, c1 = 1 - beta1, beta2, c2 = 1 - beta2, eps, r = sqrt(1 - beta2^t), and per array s = lr / (1 - beta1^t).
 *      Per element, in f32, each operation rounded once and none contracted (torch's form of Adam):
 *        m' = beta1 m + c1 g;  v' = beta2 v + (c2 g) g;  den = sqrt(v') / r + eps;  p' = p - s (m' / den).
 *      An element whose p or g is not finite is left untouched, moments included (the decoded alphas of bytes 0 and 255
 *      are -inf and +inf and stay so), and counted: *d_skipped (device memory, uint32, zeroed by the caller) grows by
 *      their number, with one vector integer atomic per workgroup that has any.  One launch; 16-byte accesses from the
 *      first 16-aligned parameter address of each array, scalar elements before and after.  Arguments checked on the
 *      host before the launch; enqueues on hip_stream and does not synchronise.
 *
 * ---- refine: a packed stream fitted to a target stream over a set of views (spz_refine.hip; DESIGN §8 "Refine").
 *      A (the stream to improve) and B (the target), both in device memory with their headers; they may differ in point
 *      count, SH degree and version, as in compare.  views: 1..SPZ_AMD_REFINE_MAX_VIEWS render params, each passing
 *      render_check_params, all with one coord (a bad one: SPZ_AMD_ERR_INVALID_ARG before anything is launched, the view
 *      in *h_bad_view).  options: iterations >= 0; lambda_dssim in [0, 1]; lr[6] >= 0 in the train_mask's order; beta1,
 *      beta2 in [0, 1); eps >= 0; train_mask non-zero (refine_check, host only; refine_default_options: 3DGS's published
 *      arguments, every array trained, lr[0] = 1.6e-4 for a scene of unit extent).
 *      Run.  Every view of B rendered once with the packed path and kept (16 W H bytes per view, beside four float
 *      clouds of A's size and 104 W H bytes for the largest view); the "before" metrics (image_metrics_device) of A's
 *      packed render against it.  A decoded once to a float cloud in the views' coord, the moments zeroed.  Iteration i
 *      uses view i mod V: render_prepare_cloud_device with A's antialiased flag, the total read back, the workspace
 *      grown (grow-only), render_finish_device; image_loss_device against the kept target; render_backward_device;
 *      adam_step_device with t = i + 1.  A total above 2^31 - 1: SPZ_AMD_ERR_CAPACITY, the view in *h_bad_view.
 *      h_history[i] (iterations doubles) = L before step i.
 *      Output: a stream with A's header (version, fractional bits, sh degree, antialiased flag, point count).  The
 *      sections of trained arrays are encoded from the floats with the encode kernel, from the views' coord back to the
 *      file's; the sections of untrained arrays are A's bytes: refine does not requantise what it does not train.  With
 *      iterations == 0 the output is A's bytes and after equals before.  The encode kernel writes versions 2 and 3 and
 *      positions at 12 fractional bits: a version 1 input, or trained positions at another precision, with iterations
 *      > 0: SPZ_AMD_ERR_UNSUPPORTED.  h_after: the metrics of the OUTPUT STREAM, rendered with the packed path, against
 *      the kept targets: the claim is about the file, quantisation included.
 *      The backward sums with f32 atomic adds, so a refine need not repeat its bits; with at least one iteration
 *      h_history[0] does, because it comes before any step.
 *      open (shaped like prune's) runs on `device` on a stream of its own and blocks.  h_before, h_after (may be NULL):
 *      num_views results each; *h_skipped (may be NULL): the non-finite elements the steps left alone, summed over the
 *      steps; h_ms (may be NULL): [0] wall-clock milliseconds of the targets and "before" metrics, [1] of the
 *      iterations and the encode, [2] of the "after" metrics; *h_bad_view (may be NULL): the view a failure concerns,
 *      else -1.  Every refusal of every open entry of this family (refine, densify, images, images with depth, and
 *      their host forms) leaves *ctx NULL, *h_out_bytes 0, *h_bad_view -1 unless a view is at fault, and, where the
 *      entry has them, *h_num_points 0 and *h_num_rounds 0. */
enum {
  SPZ_AMD_REFINE_MAX_VIEWS = 1024,
  SPZ_AMD_TRAIN_POSITIONS = 1,
  SPZ_AMD_TRAIN_SCALES = 2,
  SPZ_AMD_TRAIN_ROTATIONS = 4,
  SPZ_AMD_TRAIN_ALPHAS = 8,
  SPZ_AMD_TRAIN_COLORS = 16,
  SPZ_AMD_TRAIN_SH = 32,
  SPZ_AMD_TRAIN_ALL = 63
};
typedef struct {
  float beta1, c1, beta2, c2, eps, r;
  float s[6];
} spz_amd_adam_scalars;
typedef struct {
  int32_t iterations;
  uint32_t train_mask;
  double lambda_dssim;
  double lr[6];
  double beta1, beta2, eps;
} spz_amd_refine_options;
uint64_t spz_amd_image_loss_workspace_bytes(int width, int height);
int spz_amd_image_loss_device(const float *d_a, int channels_a, const float *d_b, int channels_b, int width, int height,
                              double lambda_dssim, double *d_loss, float *d_grad, void *d_workspace, void *hip_stream);
int spz_amd_adam_scalars_of(int t, const double lr[6], double beta1, double beta2, double eps,
                            spz_amd_adam_scalars *out);
int spz_amd_adam_step_device(const spz_amd_cloud_grads *d_params, const spz_amd_cloud_grads *d_grads,
                             const spz_amd_cloud_grads *d_m, const spz_amd_cloud_grads *d_v, uint64_t num_points,
                             int sh_degree, unsigned train_mask, spz_amd_adam_scalars scalars, uint32_t *d_skipped,
                             void *hip_stream);
int spz_amd_refine_default_options(spz_amd_refine_options *options);
int spz_amd_refine_check(const spz_amd_refine_options *options);
int spz_amd_refine_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                        const uint8_t *d_stream_b, size_t size_b, const spz_amd_header *hdr_b,
                        const spz_amd_render_params *views, int num_views, const spz_amd_refine_options *options,
                        int device, void **ctx, uint64_t *h_out_bytes, double *h_history,
                        spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after, uint64_t *h_skipped, float *h_ms,
                        int32_t *h_bad_view);
int spz_amd_refine_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_refine_device_data(void *ctx);
void spz_amd_refine_close(void *ctx);

/* ---- densify: 3DGS's adaptive density control over a float cloud and its Adam moments (spz_densify.hip; DESIGN §8
 *      "Densify").  The reference has no counterpart.  Gaussians whose screen-space position gradient stays high are
 *      cloned (small ones) or split in two (large ones), transparent ones are culled, opacities can be reset.  No float
 *      atomics anywhere: given the same inputs every entry repeats its bits.  Arguments are checked on the host before
 *      any launch; the device entries enqueue on hip_stream and do not synchronise, unless stated.
 *
 *      Options (densify_default_options: 3DGS's published values; interval and opacity_reset_interval are 0 = off, as
 *      every layer above has densify off unless asked; 3DGS runs them at 100 and 3000).  densify_check (host only)
 *      refuses negative values, until_iter < from_iter, NaN or infinities, min_opacity outside (0, 1), and percent_dense
 *      <= 0 when interval > 0.
 *      Thresholds (densify_thresholds, host only, f64 then rounded to f32): extent = options->extent, or when that is 0
 *      3DGS's 1.1 max_v |c_v - mean c| over the views' camera centres c = -R^T t (a result of 0, or no views:
 *      SPZ_AMD_ERR_INVALID_ARG); log_dense = log(percent_dense extent); alpha_min = log(min_opacity / (1 -
 *      min_opacity)); log_max_scale = log(max_scale), use_max_scale = 0 when max_scale is 0.  The kernels compare floats
 *      and never evaluate exp or a sigmoid.
 *
 *      accumulate: one thread per Gaussian.  d_records: the n records of the view's prepare step (the front of the
 *      render workspace); d_record_grads: the n x 9 record gradients of render_backward_device, mean first, in pixels.
 *      For a record of finite depth (the forward's "visible"): d_accum[i] += sqrt((gx 0.5 W)^2 + (gy 0.5 H)^2), in f32,
 *      each operation rounded once and none contracted, the square root correctly rounded; a non-finite norm adds 0;
 *      d_denom[i] += 1 (uint32) either way.  The scaling puts the gradient in 3DGS's NDC units.
 *
 *      plan: d_action[n] (uint8: 0 keep, 1 clone, 2 split, 3 cull), then the output lists d_parent[n'] (uint32: the
 *      input index) and d_child[n'] (uint8: 0 the Gaussian itself, 1 a clone's copy, 2 and 3 a split's children), and
 *      d_counts[5] (uint64, device memory: n', cloned, split, culled, refused).  Per Gaussian, with ms = the largest of
 *      its three log scales (NaN ignored): cull if alpha < alpha_min (-inf is culled, NaN is not) or, with use_max_scale,
 *      ms > log_max_scale; else a candidate if g >= grad_threshold, g = denom > 0 ? accum / denom : 0, NaN as 0; a
 *      candidate is a split if ms > log_dense, else a clone.  Every candidate adds one point; the budget is max(0,
 *      max_points - (n - culled)); candidates are granted in descending g, ties to the lower index (argsort_f32_device,
 *      stable): rank r is granted iff r < budget; a refused candidate is a keep and is counted.  Output order is input
 *      order, each Gaussian replaced in place by its outputs: keep -> itself; clone -> itself, then the copy; split ->
 *      child 2, child 3; cull -> nothing.  Offsets: an exclusive scan per 256 Gaussians and one of the workgroups' sums.
 *      list_capacity (entries of d_parent and d_child) must be at least min(2 n, max(max_points, n)), which bounds n'.
 *      densify_plan_workspace_bytes (host only): device memory for n Gaussians.  densify_plan_host: the same, then
 *      blocks and copies the five counts to h_counts.  n < 2^31.
 *
 *      apply: one launch, a gather through d_parent (entries clamped to n_src - 1) of the six arrays of the parameters
 *      and both moments into destination sets that do not overlap the sources.  keep and a clone's child 0: parameters
 *      and moments copied; child 1: parameters copied, moments 0; children 2 and 3: moments 0, log scales - (float)log
 *      1.6 in f32 (3DGS's / (0.8 * 2)), position p + R(q / |q|) (exp(ls) (.) z_k) in f64 from the f32 inputs, rounded
 *      once (R as the render's preprocess forms it from xyzw); a child whose position is not finite takes the parent's;
 *      everything else copied.  z_2, z_3: standard normals from counters, with sm = splitmix64 (x += 0x9E3779B97F4A7C15;
 *      x = (x ^ x >> 30) 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) 0x94D049BB133111EB; x ^ x >> 31): key = sm(sm(seed ^
 *      round) + i), i the parent's index; for j = 0..2: a = sm(key + 2 j + 1), b = sm(key + 2 j + 2), u1 = ((a >> 11) +
 *      1) 2^-53, u2 = (b >> 11) 2^-53, r = sqrt(-2 ln u1), z_2[j] = r cos(2 pi u2), z_3[j] = r sin(2 pi u2).  n_new
 *      above dst_capacity (points): SPZ_AMD_ERR_CAPACITY.  sh may be NULL when sh_degree == 0.
 *      reset_opacity: alpha = min(alpha, (float)logit(0.01)), NaN left alone; the alphas' two moments zeroed.
 *
 *      refine_densify_open: spz_amd_refine_open with densify.  densify NULL or interval == 0: exactly refine_open
 *      (*h_num_points = A's count, no rounds).  Else positions and scales must be in the train mask, and alphas when
 *      opacity_reset_interval > 0 (SPZ_AMD_ERR_INVALID_ARG); max_points (0: B's count) below A's count:
 *      SPZ_AMD_ERR_INVALID_ARG, above 2^31 - 1: SPZ_AMD_ERR_TOO_MANY_POINTS.  After the backward of each iteration i in
 *      [from_iter, until_iter): accumulate.  After the Adam step of such an i with (i + 1) % interval == 0: plan_host,
 *      apply, the sets swapped, accum and denom zeroed.  After the Adam step of any i with (i + 1) %
 *      opacity_reset_interval == 0: reset.  Adam's t stays i + 1 for everyone.  Every buffer is allocated once at
 *      capacity max_points: seven float clouds (parameters, gradients, two moments, and the apply's three destinations)
 *      beside 9 + 2 floats, 14 bytes of lists and origin maps and the plan's workspace per point: about 7 x 4 x (14 + 3
 *      sh_dim) + 58 bytes + densify_plan_workspace_bytes(max_points) / max_points per point of max_points.  apply's
 *      `round` is the count of rounds so far, from 0.
 *      Output: A's header with num_points =
 *      n'; sections of trained arrays encoded from the floats; sections of untrained arrays A's bytes gathered through
 *      the origin map (the index in A of each output point, carried through every round) with subset_device.  h_rounds
 *      (may be NULL): the first rounds_capacity rounds; *h_num_rounds (may be NULL): how many ran.  h_origin (may be
 *      NULL): max_points entries of room, n' written. */
typedef struct {
  int32_t interval;               /* a round every `interval` iterations; 0 = off */
  int32_t from_iter, until_iter;  /* rounds and accumulation run for iterations in [from_iter, until_iter) */
  int32_t opacity_reset_interval; /* 0 = off */
  double grad_threshold;          /* 2e-4 */
  double percent_dense;           /* 0.01 */
  double extent;                  /* 0 = derive from the views */
  double min_opacity;             /* 0.005 */
  double max_scale;               /* 0 = off */
  uint64_t max_points;            /* 0 = the target's count */
  uint64_t seed;
} spz_amd_densify_options;
typedef struct {
  float grad_threshold, log_dense, alpha_min, log_max_scale;
  int32_t use_max_scale;
  int32_t reserved;
  double extent;
} spz_amd_densify_limits;
typedef struct {
  int32_t iteration;
  int32_t reserved;
  uint64_t cloned, split, culled, refused, num_points;
} spz_amd_densify_round;
int spz_amd_densify_default_options(spz_amd_densify_options *options);
int spz_amd_densify_check(const spz_amd_densify_options *options);
int spz_amd_densify_thresholds(const spz_amd_densify_options *options, const spz_amd_render_params *views,
                               int num_views, spz_amd_densify_limits *limits);
int spz_amd_densify_accumulate_device(const spz_amd_render_record *d_records, const float *d_record_grads,
                                      uint64_t num_points, uint32_t width, uint32_t height, float *d_accum,
                                      uint32_t *d_denom, void *hip_stream);
uint64_t spz_amd_densify_plan_workspace_bytes(uint64_t num_points);
int spz_amd_densify_plan_device(const float *d_accum, const uint32_t *d_denom, const float *d_scales,
                                const float *d_alphas, uint64_t num_points, const spz_amd_densify_limits *limits,
                                uint64_t max_points, uint64_t list_capacity, uint8_t *d_action, uint32_t *d_parent,
                                uint8_t *d_child, uint64_t *d_counts, void *d_workspace, void *hip_stream);
int spz_amd_densify_plan_host(const float *d_accum, const uint32_t *d_denom, const float *d_scales,
                              const float *d_alphas, uint64_t num_points, const spz_amd_densify_limits *limits,
                              uint64_t max_points, uint64_t list_capacity, uint8_t *d_action, uint32_t *d_parent,
                              uint8_t *d_child, uint64_t *d_counts, void *d_workspace, uint64_t *h_counts,
                              void *hip_stream);
int spz_amd_densify_apply_device(const spz_amd_cloud_grads *d_src_params, const spz_amd_cloud_grads *d_src_m,
                                 const spz_amd_cloud_grads *d_src_v, const spz_amd_cloud_grads *d_dst_params,
                                 const spz_amd_cloud_grads *d_dst_m, const spz_amd_cloud_grads *d_dst_v,
                                 const uint32_t *d_parent, const uint8_t *d_child, uint64_t n_src, uint64_t n_new,
                                 uint64_t dst_capacity, int sh_degree, uint64_t seed, uint32_t round, void *hip_stream);
int spz_amd_densify_reset_opacity_device(float *d_alphas, float *d_alphas_m, float *d_alphas_v, uint64_t num_points,
                                         void *hip_stream);
int spz_amd_refine_densify_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                const uint8_t *d_stream_b, size_t size_b, const spz_amd_header *hdr_b,
                                const spz_amd_render_params *views, int num_views, const spz_amd_refine_options *options,
                                const spz_amd_densify_options *densify, int device, void **ctx, uint64_t *h_out_bytes,
                                double *h_history, spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                                uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view, uint64_t *h_num_points,
                                spz_amd_densify_round *h_rounds, int rounds_capacity, int *h_num_rounds,
                                uint32_t *h_origin);

/* ---- photo loss: the image loss of a render against a photograph, with per-pixel weights and a per-image exposure of
 *      the render (spz_photo.hip; DESIGN §8 "Fit").  The reference has no counterpart.  Everything "image loss" says
 *      holds unless this says otherwise; a, b, d_loss and d_grad are its arguments.
 *      Exposure.  h_exposure (host memory): 12 doubles, row-major [M | o], 3DGS's 3 x 4 colour transform of one image;
 *      every value finite.  NULL: the identity, and nothing is multiplied.  The exposed render of a pixel is t_c =
 *      ((o_c + M_c0 a_0) + M_c1 a_1) + M_c2 a_2 in f64 from the f32 values; a' = t clamped to [0, 1], NaN -> 0; the gate
 *      of (pixel, channel) is open where 0 <= t <= 1, both ends included, and closed elsewhere and for NaN.
 *      Weights.  d_weight (device memory): height x width float32, NULL: every weight 1.  Each is clamped to [0, 1],
 *      NaN -> 0.  W = sum_p w_p in f64.
 *      Loss.  L = (1 - lambda) l1 + lambda (1 - ssim), l1 = sum_p w_p sum_c |a'_pc - b_pc| / (3 W), ssim = sum_p w_p
 *      sum_c S_pc / (3 W), S the per-pixel, per-channel SSIM of "image metrics" over the UNWEIGHTED 11 x 11 zero-padded
 *      windows of a' and the clamped b.  W == 0: L = l1 = 0, ssim = 1, and every gradient is exactly 0.
 *      Gradient to the exposed render: image loss's formulas with w_p / (3 W) for 1 / (3 H W) in the L1 part, and the
 *      maps M, Q, P multiplied by w_q before they are filtered, then divided by 3 W.  A pixel of weight 0 still gets
 *      gradient from the windows centred on weighted neighbours: that is the derivative.
 *      d_grad = dL/da = M^T (gate . dL/da') in the rgb channels, each value summed in f64 over the open gates in channel
 *      order and rounded once to f32; without an exposure gate . dL/da' itself.  A fourth channel gets exactly 0; every
 *      element is written.  d_exposure_grad (device memory, 8-aligned, 12 doubles, row-major as h_exposure; required
 *      with h_exposure, else it may be NULL): dL/dM_ck = sum_p gate_pc dL/da'_pc a_pk, dL/do_c = sum_p gate_pc
 *      dL/da'_pc.  A (pixel, channel) whose gate is closed is skipped, not multiplied by zero (its a may be infinite: a
 *      non-finite a_k makes every t_c of its pixel infinite or NaN, which closes all three gates); a term whose a_pk is
 *      not finite is skipped as well, which matters without an exposure, where the gate of channel c is that of a_c
 *      alone.
 *      Arithmetic.  The image loss's two passes with the products above, every one an f64 product, then a reduction of
 *      the 12 sums: per tile over the wave, the waves in order, one row of `tiles` per value, summed by one workgroup in
 *      a fixed order.  No float atomics: a run repeats its bits.  With d_weight == NULL and h_exposure == NULL every
 *      product is by 1.0, W = H W exactly, and d_loss and d_grad carry exactly the bits of image_loss_device.  The
 *      exposure path reads a's three channels for each channel it forms: a is read once more than the loss reads it.
 *      photo_loss_workspace_bytes (host only; 0 for a bad size): 72 H W bytes, the slab, and 96 bytes per tile.
 *      photo_loss_device: arguments checked on the host before any launch (SPZ_AMD_ERR_INVALID_ARG; no device:
 *      SPZ_AMD_ERR_NO_DEVICE); enqueues on hip_stream and does not synchronise.
 *      image_exposure_device: out_c = ((o_c + M_c0 a_0) + M_c1 a_1) + M_c2 a_2, unclamped, in f32 with the 12 values
 *      rounded to f32 first, each operation rounded once in that order, none contracted.  channels in {3, 4}; a fourth
 *      channel is copied; d_out == d_in is allowed.  h_exposure NULL or not finite: SPZ_AMD_ERR_INVALID_ARG.
 *
 * ---- refine images: a packed stream fitted to photographs (spz_refine.hip; DESIGN §8 "Fit").  "refine" and "densify"
 *      with the targets given instead of rendered: there is no stream B.  d_targets: a host array of num_views device
 *      pointers, target v height_v x width_v x channels float32 of view v's size, channels in {3, 4}; d_weights: NULL, or
 *      a host array of num_views device pointers to height_v x width_v float32, any of them NULL (photo loss's weights).
 *      A NULL or misaligned target, a misaligned weight map, or a view larger than image_metrics_check allows:
 *      SPZ_AMD_ERR_INVALID_ARG with the view in *h_bad_view; channels outside {3, 4}: SPZ_AMD_ERR_INVALID_ARG.  The
 *      targets are used in place and must stay until the call returns; the block no longer holds 16 W H bytes per view.
 *      photo (photo_default_options: fit_exposure 0, lr_exposure 0.01, 3DGS's exposure_lr_init; photo_check, host only:
 *      fit_exposure 0 or 1, lr_exposure >= 0 and finite).  densify: NULL, or as refine_densify_open; with interval > 0
 *      max_points == 0 is refused (SPZ_AMD_ERR_INVALID_ARG): there is no target count to default to.
 *      Run.  Iteration i uses view v = i mod V: the render; photo_loss with view v's weights and, with fit_exposure,
 *      view v's exposure read from device memory; render_backward_device with that d_grad; then everything refine does.
 *      With fit_exposure view v's 12 values then take one Adam step in f64 on the device (one workgroup; m' = beta1 m +
 *      (1 - beta1) g, v' = beta2 v + ((1 - beta2) g) g, e' = e - lr_exposure / (1 - beta1^t) (m' / (sqrt(v') / sqrt(1 -
 *      beta2^t) + eps)), with options' betas and eps and t the number of visits of that view, from 1; a non-finite
 *      gradient value leaves its element alone): the loop gains no host synchronisation.  Exposures start at the
 *      identity and are never written into the file.  Without fit_exposure no exposure is applied anywhere.
 *      h_history[i] = L before step i.  h_before: image_metrics_device of A's packed render against the target,
 *      unweighted, identity exposure.  h_after: the OUTPUT STREAM's packed render, passed through that view's fitted
 *      exposure with image_exposure_device when fit_exposure is set, against the target, unweighted.  h_exposures (may
 *      be NULL): 12 doubles per view, exactly the identity without fit_exposure.  The other outputs are
 *      refine_densify_open's; the result is fetched and closed with refine_fetch, refine_device_data, refine_close.
 *      refine_images_host_open: the same with the images and weight maps in host memory (h_targets, h_weights, shaped
 *      as above): every argument is checked first, as refine_images_open checks it (but a host map may lie at any
 *      address), then the images are copied to `device` and kept there until the call returns. */
typedef struct {
  int32_t fit_exposure; /* 0 or 1 */
  int32_t reserved;
  double lr_exposure;   /* 0.01 */
} spz_amd_photo_options;
uint64_t spz_amd_photo_loss_workspace_bytes(int width, int height);
int spz_amd_photo_loss_device(const float *d_a, int channels_a, const float *d_b, int channels_b, const float *d_weight,
                              const double *h_exposure, int width, int height, double lambda_dssim, double *d_loss,
                              float *d_grad, double *d_exposure_grad, void *d_workspace, void *hip_stream);
int spz_amd_image_exposure_device(const float *d_in, int channels, const double *h_exposure, int width, int height,
                                  float *d_out, void *hip_stream);
int spz_amd_photo_default_options(spz_amd_photo_options *options);
int spz_amd_photo_check(const spz_amd_photo_options *options);
int spz_amd_refine_images_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                               const spz_amd_render_params *views, int num_views, const float *const *d_targets,
                               int channels, const float *const *d_weights, const spz_amd_refine_options *options,
                               const spz_amd_photo_options *photo, const spz_amd_densify_options *densify, int device,
                               void **ctx, uint64_t *h_out_bytes, double *h_history, spz_amd_image_metrics *h_before,
                               spz_amd_image_metrics *h_after, uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view,
                               uint64_t *h_num_points, spz_amd_densify_round *h_rounds, int rounds_capacity,
                               int *h_num_rounds, uint32_t *h_origin, double *h_exposures);
int spz_amd_refine_images_host_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                    const spz_amd_render_params *views, int num_views, const float *const *h_targets,
                                    int channels, const float *const *h_weights, const spz_amd_refine_options *options,
                                    const spz_amd_photo_options *photo, const spz_amd_densify_options *densify,
                                    int device, void **ctx, uint64_t *h_out_bytes, double *h_history,
                                    spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after, uint64_t *h_skipped,
                                    float *h_ms, int32_t *h_bad_view, uint64_t *h_num_points,
                                    spz_amd_densify_round *h_rounds, int rounds_capacity, int *h_num_rounds,
                                    uint32_t *h_origin, double *h_exposures);

/* ---- depth loss: the loss of a depth render against a measured depth map, and its gradient to the render
 *      (spz_depth_loss.hip; DESIGN §8 "Depth fit").  The reference has no counterpart.
 *      d_depth: height x width x 2 float32 as render_depth_device writes it; only channel 0, D, is read.  d_image:
 *      height x width x 4; only channel 3, alpha, is read.  d_target: height x width float32, metric depth along the
 *      camera's z in scene units.  d_weight: NULL (every weight 1), or height x width float32, each clamped to [0, 1],
 *      NaN -> 0: the photo loss's rule.  kind: SPZ_AMD_DEPTH_L1 or SPZ_AMD_DEPTH_INVERSE_L1.  min_alpha in (0, 1].
 *      scale >= 0 and finite: the weight of this term in the caller's total loss; it scales the gradients, not L.
 *      A pixel is valid iff w_p > 0, the target is finite and > 0, alpha >= min_alpha (both f32) and D is finite and
 *      > 0.  In f64 from the f32 values: e = D / alpha - t (L1) or alpha / D - 1 / t (inverse); W_v = sum_valid w_p;
 *      L = sum_valid w_p |e_p| / W_v.  W_v == 0: L = 0 and every gradient is exactly 0.
 *      Gradients, the validity held constant, with s = scale sign(e) w_p / W_v and sign(0) = 0.  L1: g_D = s / alpha,
 *      g_alpha = -s D / alpha^2.  Inverse: g_D = -s alpha / D^2, g_alpha = s / D.  Each is rounded once to f32.
 *      d_loss (device memory, 8-aligned): two doubles, L (not scaled) and W_v.  d_grad_depth: height x width float32,
 *      every element written, exact 0 where the pixel is invalid; it is the d_grad_depth of
 *      render_depth_backward_device.  d_grad_image (may be NULL): height x width x 4; channel 3 gets += g_alpha, one
 *      lane per pixel, the other channels are not touched: run it after the photo loss, which writes an exact 0 there.
 *      Arithmetic.  Per-workgroup partial sums in a fixed tree, summed by one workgroup in a fixed order; the gradient
 *      pass reads W_v from d_loss.  No float atomics and no host synchronisation: a run repeats its bits.
 *      depth_loss_workspace_bytes (host only; 0 for a bad size): 16 bytes per 256 pixels.  depth_loss_device: arguments
 *      checked on the host before any launch (sizes as image_metrics_check, 4-byte alignment, kind, min_alpha, scale:
 *      SPZ_AMD_ERR_INVALID_ARG; no device: SPZ_AMD_ERR_NO_DEVICE); enqueues on hip_stream and does not synchronise. */
enum { SPZ_AMD_DEPTH_L1 = 0, SPZ_AMD_DEPTH_INVERSE_L1 = 1 };
uint64_t spz_amd_depth_loss_workspace_bytes(int width, int height);
int spz_amd_depth_loss_device(const float *d_depth, const float *d_image, const float *d_target, const float *d_weight,
                              int width, int height, int kind, float min_alpha, double scale, double *d_loss,
                              float *d_grad_depth, float *d_grad_image, void *d_workspace, void *hip_stream);

/* ---- refine images with depth: "refine images" with a measured depth map for some or all of the views
 *      (spz_refine.hip; DESIGN §8 "Depth fit").  The two entries are refine_images_open and refine_images_host_open
 *      with, after the weights, d_depth_targets (h_depth_targets for the host form): NULL, or a host array of num_views
 *      pointers, any of them NULL, to height_v x width_v float32 maps as "depth loss" takes them (a value that is not
 *      finite or not > 0 means no measurement there); and depth (depth_default_options: weight 1.0, min_alpha 0.5,
 *      SPZ_AMD_DEPTH_L1; depth_check, host only: weight >= 0 and finite, min_alpha in (0, 1], a known kind).  A
 *      misaligned map: SPZ_AMD_ERR_INVALID_ARG with the view in *h_bad_view.  The maps are used in place.
 *      Run.  An iteration whose view has a map, with weight > 0: prepare; render_depth_device (its image is
 *      render_finish_device's, bit for bit); the photo loss; depth_loss_device with view v's weights and scale = weight,
 *      adding its gradient to alpha into the photo loss's d_grad; render_depth_backward_device with both gradients;
 *      then Adam, the exposure step and densify as "refine images" has them.  Densify's screen-space accumulator reads
 *      the record gradients of that backward, so it sees the depth term's mean gradient too.  A view without a map, or
 *      weight == 0, takes the path of "refine images" unchanged; with no map at all h_history and h_before carry
 *      exactly the bits refine_images_open gives.
 *      h_history[i] = L_photo + weight L_depth before step i.  h_depth_history (may be NULL): iterations doubles,
 *      L_depth before step i, 0 for a view without a map or with weight == 0.  h_depth_error (may be NULL): 2 doubles
 *      per view; [2 v] is the depth loss (view v's weights, the options' kind and min_alpha) of A's packed depth render
 *      against the map, [2 v + 1] that of the OUTPUT STREAM's packed depth render (with iterations == 0: the same
 *      value); -1 for a view without a map.
 *      Memory grows by 12 W H bytes for the depth render and its gradient and by the depth loss's workspace, all for
 *      the largest view, and the backward workspace by 4 bytes per Gaussian. */
typedef struct {
  double weight;   /* 1.0: the depth term's weight in the loss */
  float min_alpha; /* 0.5 */
  int32_t kind;    /* SPZ_AMD_DEPTH_L1 */
} spz_amd_depth_options;
int spz_amd_depth_default_options(spz_amd_depth_options *options);
int spz_amd_depth_check(const spz_amd_depth_options *options);
int spz_amd_refine_images_depth_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                     const spz_amd_render_params *views, int num_views, const float *const *d_targets,
                                     int channels, const float *const *d_weights, const float *const *d_depth_targets,
                                     const spz_amd_depth_options *depth, const spz_amd_refine_options *options,
                                     const spz_amd_photo_options *photo, const spz_amd_densify_options *densify,
                                     int device, void **ctx, uint64_t *h_out_bytes, double *h_history,
                                     spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                                     uint64_t *h_skipped, float *h_ms, int32_t *h_bad_view, uint64_t *h_num_points,
                                     spz_amd_densify_round *h_rounds, int rounds_capacity, int *h_num_rounds,
                                     uint32_t *h_origin, double *h_exposures, double *h_depth_history,
                                     double *h_depth_error);
int spz_amd_refine_images_depth_host_open(const uint8_t *d_stream_a, size_t size_a, const spz_amd_header *hdr_a,
                                          const spz_amd_render_params *views, int num_views,
                                          const float *const *h_targets, int channels, const float *const *h_weights,
                                          const float *const *h_depth_targets, const spz_amd_depth_options *depth,
                                          const spz_amd_refine_options *options, const spz_amd_photo_options *photo,
                                          const spz_amd_densify_options *densify, int device, void **ctx,
                                          uint64_t *h_out_bytes, double *h_history, spz_amd_image_metrics *h_before,
                                          spz_amd_image_metrics *h_after, uint64_t *h_skipped, float *h_ms,
                                          int32_t *h_bad_view, uint64_t *h_num_points, spz_amd_densify_round *h_rounds,
                                          int rounds_capacity, int *h_num_rounds, uint32_t *h_origin,
                                          double *h_exposures, double *h_depth_history, double *h_depth_error);

/* ---- render view backward: the gradient of one view to its camera (spz_render_view_backward.hip; DESIGN §8
 *      "Locate").  The reference has no counterpart.  Given the n x 9 record gradients of a view (mean 2, conic 3,
 *      opacity 1, rgb 3, as "render backward" forms them), it produces the gradient of the same scalar loss to the 12
 *      entries of world_to_camera = [R | t], taken as independent: it is not projected onto the rotation group, just as
 *      the raw quaternion gets its gradient.  Intrinsics get none.
 *
 *      It is the exact derivative of the forward as "render" words it, with the discrete decisions "render backward"
 *      holds constant: visibility, radius, tile rectangle and depth order; the three blend tests; the clamp of x/z and
 *      y/z in J, which passes nothing through the clamped quotient; max(0, rgb), which passes nothing where it clamps;
 *      the antialiased factor, which is zero where det_before <= 0.  The camera enters three times and all three are
 *      differentiated: p_c = R p + t, which feeds the mean and J; R in Sigma' = J R Sigma R^T J^T; and the camera
 *      centre c = -R^T t in the view direction normalize(p - c) of the sh bands.  The record's depth carries no
 *      gradient (the colour image does not read it).  An invisible Gaussian contributes exactly 0.
 *      Arithmetic.  One lane per Gaussian runs the chain in f64 from the f32 inputs and forms its 12 contributions.
 *      They are summed without atomics: over the wave by a fixed tree of 64-lane shuffles, over the workgroup's waves
 *      through LDS in wave order, one row of 12 doubles per workgroup; a second launch of one workgroup adds the rows
 *      in a fixed order.  Given the same record gradients a run repeats its bits.  The record gradients come from f32
 *      atomic adds, so the whole chain from G need not.
 *
 *      render_records_backward_device: the blend half of render_backward_device on its own, for a caller that needs
 *      no gradients to the six cloud arrays.  d_render_workspace exactly as render_finish_device left it; d_grad_image:
 *      G, height x width x 4 floats; d_record_grads: n x 9 floats out (written, not accumulated into; may be NULL iff
 *      num_points == 0).  *d_status = 0, or 1 when the total is above max_entries: then nothing is written.
 *      render_view_backward_workspace_bytes (host only): device memory for the workgroups' rows.
 *      render_view_backward_device: d_cloud, num_points, sh_degree, antialiased, params and max_entries as given to
 *      prepare_cloud_device and render_finish_device; d_record_grads: n x 9 floats in; d_render_workspace as
 *      render_finish_device left it (the records and the total are read; nothing in it is written).  d_view_grad
 *      (device memory, 8-aligned): 12 doubles out, row-major 3 x 4.  *d_status (device memory, uint32) = 0, or 1 when
 *      the total is above max_entries: then d_view_grad is not written.  num_points == 0 or nothing visible: twelve
 *      zeros.
 *      Both check their arguments on the host before any launch (a bad one: SPZ_AMD_ERR_INVALID_ARG; more than 2^31 - 1
 *      points: SPZ_AMD_ERR_TOO_MANY_POINTS; no device: SPZ_AMD_ERR_NO_DEVICE), enqueue on hip_stream and do not
 *      synchronise. */
int spz_amd_render_records_backward_device(uint64_t num_points, const spz_amd_render_params *params,
                                           uint64_t max_entries, const float *d_grad_image, float *d_record_grads,
                                           uint32_t *d_status, const void *d_render_workspace, void *hip_stream);
uint64_t spz_amd_render_view_backward_workspace_bytes(uint64_t num_points);
int spz_amd_render_view_backward_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree,
                                        int antialiased, const spz_amd_render_params *params, uint64_t max_entries,
                                        const float *d_record_grads, double *d_view_grad, uint32_t *d_status,
                                        const void *d_render_workspace, void *d_workspace, void *hip_stream);

/* ---- locate: the pose of a camera in a scene, fitted to a picture (spz_locate.hip; DESIGN §8 "Locate").  The
 *      reference has no counterpart.  Given a scene, a view with a rough pose and the picture taken from the true one,
 *      it moves the pose down the gradient of the 3DGS loss ("image loss") of the scene's render against the picture.
 *      No search: the initial pose must be close enough for the two images to overlap.
 *      options: iterations >= 0; levels 1..SPZ_AMD_LOCATE_MAX_LEVELS; lambda_dssim in [0, 1]; lr_rotation (radians) and
 *      lr_translation (scene units) >= 0; lr_final_factor in (0, 1]; beta1, beta2 in [0, 1); eps >= 0 (locate_check,
 *      host only; locate_default_options: 300 iterations, 1 level, lambda 0.2, both step sizes 2e-3 — the translation's
 *      for a camera at unit distance, the layers above scale it — final factor 0.1, 0.9, 0.999, 1e-15).
 *      target: height x width x C float32 in device memory, C in {3, 4}, the size of params.
 *      Run.  The "before" metrics (image_metrics_device) of the input's render (the packed path for a stream) at the
 *      initial pose.  A stream is decoded once to a float cloud in params.coord.  One iteration: render_prepare_cloud_
 *      device, the total read back, the workspace grown (grow-only), render_finish_device; image_loss_device against
 *      the target; render_records_backward_device; render_view_backward_device; the 12 doubles read back.  A total
 *      above 2^31 - 1: SPZ_AMD_ERR_CAPACITY.
 *      Update, in f64 on the host; the pose is kept in f64 and rounded to f32 only into the params.  With G = [G_R |
 *      G_t] and A = G_R R^T + G_t t^T, the gradient to the twist (w, v) of L(Exp(w) R, Exp(w) t + v) at 0 is g_w = (A21 -
 *      A12, A02 - A20, A10 - A01), g_v = G_t (locate_twist_gradient, host only).  Adam over the six values with bias
 *      correction, t = i + 1: m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2; d = -lr f_i (m / (1 -
 *      beta1^t)) / (sqrt(v / (1 - beta2^t)) + eps), 0 where m is 0; lr = lr_rotation for w and lr_translation for v;
 *      f_i = lr_final_factor^(i / iterations).  Then R <- Exp(d_w) R, t <- Exp(d_w) t + d_v, Exp by Rodrigues' formula,
 *      below |d_w| = 1e-4 with the series 1 - x/6 and 1/2 - x/24 in x = |d_w|^2 (locate_pose_step, host only: one
 *      update of pose, m and v in place for iteration i in 0..iterations - 1).  A gradient with a non-finite entry stops
 *      the run at the last pose; *h_iterations says how many steps were taken.
 *      Coarse to fine.  Level k runs from levels - 1 down to 0 at (width / 2^k) x (height / 2^k) with fx, fy, cx, cy
 *      divided by 2^k (locate_level_params, host only): the exact pinhole of the box-averaged image under m = f x/z + c -
 *      0.5.  Its target is the k-fold 2 x 2 box mean of the target (image_halve_device: f32, ((top left + top right) +
 *      (bottom left + bottom right)) / 4, channels kept, width and height even).  Width and height must be divisible
 *      by 2^(levels - 1): otherwise SPZ_AMD_ERR_INVALID_ARG.  iterations / levels iterations per level, the remainder
 *      to level 0; Adam's state and f_i run through all levels.
 *      The host forms run on `device` on a stream of their own and block; every argument is checked before the first
 *      HIP call.  locate_host: a packed stream; locate_image_host: the same with the target in host memory, uploaded
 *      once; locate_cloud_host: a float cloud in device memory, rendered as it is (params.coord is ignored).  h_world_to_camera: the final pose, 12 floats.  h_history (iterations doubles; may be NULL iff
 *      iterations == 0): [i] = L before step i, 0 from *h_iterations on.  h_before, h_after (may be NULL): the metrics
 *      at the initial and the final pose; equal when no step was taken.  h_ms (may be NULL): [0] wall-clock
 *      milliseconds of the "before" metrics, [1] of the iterations, [2] of the "after" metrics.
 *      The record gradients come from f32 atomic adds, so a run need not repeat its bits; h_history[0] and h_before
 *      do. */
enum { SPZ_AMD_LOCATE_MAX_LEVELS = 8 };
typedef struct {
  int32_t iterations;
  int32_t levels;
  double lambda_dssim;
  double lr_rotation, lr_translation, lr_final_factor;
  double beta1, beta2, eps;
} spz_amd_locate_options;
int spz_amd_locate_default_options(spz_amd_locate_options *options);
int spz_amd_locate_check(const spz_amd_locate_options *options);
int spz_amd_locate_level_params(const spz_amd_render_params *params, int level, spz_amd_render_params *out);
int spz_amd_locate_twist_gradient(const double pose[12], const double view_grad[12], double twist_grad[6]);
int spz_amd_locate_pose_step(const spz_amd_locate_options *options, int iteration, const double twist_grad[6],
                             double m[6], double v[6], double pose[12]);
int spz_amd_image_halve_device(const float *d_in, int channels, int width, int height, float *d_out, void *hip_stream);
int spz_amd_locate_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                        const spz_amd_render_params *params, const float *d_target, int channels,
                        const spz_amd_locate_options *options, int device, float *h_world_to_camera, double *h_history,
                        spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after, int32_t *h_iterations,
                        float *h_ms);
int spz_amd_locate_image_host(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                              const spz_amd_render_params *params, const float *h_target, int channels,
                              const spz_amd_locate_options *options, int device, float *h_world_to_camera,
                              double *h_history, spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                              int32_t *h_iterations, float *h_ms);
int spz_amd_locate_cloud_host(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_degree, int antialiased,
                              const spz_amd_render_params *params, const float *d_target, int channels,
                              const spz_amd_locate_options *options, int device, float *h_world_to_camera,
                              double *h_history, spz_amd_image_metrics *h_before, spz_amd_image_metrics *h_after,
                              int32_t *h_iterations, float *h_ms);

/* ---- device buffers for a resident cloud, placed for speed (spz_place.hip).  Whether an sh3 decode runs
 *      at 0.46 ms or at 0.55 ms is decided by whether the sh float array shares a physical region of HBM with the other
 *      arrays of the launch; that cannot be asked for, but it shows in one launch.  alloc: the five small arrays (and a
 *      stream buffer, unless d_stream brings one) in one block, the sh array in an allocation of its own, chosen among
 *      up to max_candidates (1 = the first) by timing the launch the buffers are for — probe 1: a decode (d_stream
 *      read, cloud written), 2: an encode (cloud read, the stream OVERWRITTEN), 0: no timing — on `hip_stream`, with the
 *      buffers' contents zeroed.  Blocking; tens of milliseconds, once per set of long-lived buffers.  The reference has
 *      no counterpart (it holds clouds in host vectors); callers of the *_device entry points own their buffers and
 *      may use this to make them. ------------------------------------------------------------------------------- */
typedef struct {
  spz_amd_cloud_out cloud;      /* six float arrays in device memory (sh NULL for degree 0) */
  uint8_t *stream;              /* the stream buffer: this call's (stream_capacity bytes) or the caller's d_stream */
  size_t stream_capacity;
  void *owner;                  /* what spz_amd_cloud_buffers_free releases */
  int32_t candidates;           /* sh placements timed (1 when nothing was timed) */
  float probe_ms_first, probe_ms_chosen, probe_ms_worst;
} spz_amd_cloud_buffers;
int spz_amd_cloud_buffers_alloc(uint64_t num_points, int sh_degree, int version, uint8_t *d_stream, int probe,
                                int max_candidates, void *hip_stream, spz_amd_cloud_buffers *out);
int spz_amd_cloud_buffers_free(spz_amd_cloud_buffers *b);

/* ---- GaussianCloud::convertCoordinates (splat-types.h:134-164) as a standalone in-place
 *      device pass (the reference-shaped, un-fused second pass; kept for API parity and
 *      for the fused-vs-unfused measurement).  Any of the three pointers may be NULL. ------- */
int spz_amd_convert_coordinates_device(float *d_positions, float *d_rotations, float *d_sh,
                                       uint64_t num_points, int sh_degree, int from_coord,
                                       int to_coord, void *hip_stream);

/* ---- host-pointer entry points: H2D, kernel, D2H on `device`; blocking.  Calls of more than 160 MiB of
 *      floats run as a pipeline of point-range chunks (upload of chunk k+1, kernel on chunk k and
 *      download of chunk k-1 overlap; environment SPZ_AMD_HOST_CHUNK_MIB sets the chunk size).  The device
 *      staging memory is one grow-only allocation per device, kept until spz_amd_release_device_memory().
 *      spz_amd_decode_host applies the reference reader's 10 M point limit (load-spz.cc:549,561), which
 *      belongs to deserializePackedGaussians; the _ex form takes the limit (0 = none), for callers that
 *      mirror unpackGaussians (:467-531), which has none. --------------------------------------------- */
int spz_amd_encode_host(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_degree,
                        int antialiased, int from_coord, int version, uint8_t *h_stream,
                        size_t capacity, int device);
/* The same for a caller that goes on to the container stage (saveSpz, load-spz.cc:639-645: packGaussians then
 * compressGzipped): *d_stream = a device copy of the stream that stays valid until spz_amd_kept_stream_release — what
 * spz_amd_zlib_parse_open_dev takes instead of uploading the stream again — or NULL when the one such buffer per
 * device is in use (or num_points is 0). */
int spz_amd_encode_host_keep(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_degree,
                             int antialiased, int from_coord, int version, uint8_t *h_stream,
                             size_t capacity, int device, const uint8_t **d_stream);
void spz_amd_kept_stream_release(int device, const uint8_t *d_stream);
/* The same with the stream already in device memory (what spz_amd_inflate_device_data() returns): no upload, the
 * decoded floats come back to the host arrays through the same chunked pipeline.  `hdr`: the stream's header
 * (spz_amd_peek_header_device, or _ex on its first 16 bytes). */
int spz_amd_decode_host_from_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr, int to_coord,
                                    const spz_amd_cloud_out *h_cloud, int device);
int spz_amd_decode_host(const uint8_t *h_stream, size_t size, int to_coord,
                        const spz_amd_cloud_out *h_cloud, int device);
int spz_amd_decode_host_ex(const uint8_t *h_stream, size_t size, uint64_t max_points, int to_coord,
                           const spz_amd_cloud_out *h_cloud, int device);
int spz_amd_convert_coordinates_host(float *h_positions, float *h_rotations, float *h_sh,
                                     uint64_t num_points, int sh_degree, int from_coord,
                                     int to_coord, int device);
/* Host form of spz_amd_decode_gather_device: the packed stream and the index list are in host memory,
 * the `count` decoded points land in host arrays.  The header is read from the stream with the checks
 * of spz_amd_peek_header_ex(max_points).  Unlike the device form, which clamps, an index >= num_points
 * is rejected here with SPZ_AMD_ERR_INVALID_ARG before anything is copied. */
int spz_amd_decode_gather_host(const uint8_t *h_stream, size_t size, uint64_t max_points,
                               const uint32_t *h_indices, uint64_t count, int to_coord,
                               const spz_amd_cloud_out *h_cloud, int device);
/* The same for a stream that is in device memory already (spz_amd_inflate_device_data): only the index list goes
 * up and the `count` decoded points come down.  `hdr`: the stream's header. */
int spz_amd_decode_gather_host_from_device(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr,
                                           const uint32_t *h_indices, uint64_t count, int to_coord,
                                           const spz_amd_cloud_out *h_cloud, int device);

/* ---- GaussianCloud::medianVolume's selection step (splat-types.h:170-185): the
 *      element of rank num_points/2 among the per-point sums (s0 + s1) + s2 of the log scales, found by
 *      radix selection instead of a sort (4 streaming passes over d_scales, 48 B read per point).
 *      d_workspace: SPZ_AMD_MEDIAN_WORKSPACE_BYTES of device memory owned by the caller for the
 *      duration of the call's work on hip_stream; d_median: one float in device memory.  The volume
 *      itself, 4/3*pi*exp(median), is one scalar the caller computes.  num_points must be >= 1. ---- */
#define SPZ_AMD_MEDIAN_WORKSPACE_BYTES 8192
int spz_amd_median_scale_sum_device(const float *d_scales, uint64_t num_points, void *d_workspace,
                                    float *d_median, void *hip_stream);
int spz_amd_median_scale_sum_host(const float *h_scales, uint64_t num_points, float *h_median, int device);

/* ---- .ply vertex rows <-> GaussianCloud arrays (the step on the far side of
 *      the hot path).  A binary-LE 3DGS .ply stores one row of `property float` columns per
 *      Gaussian (load-spz.cc:728-740); the column map below is what the header parse yields
 *      (:742-786).  rows_to_cloud replaces the AoS->SoA loop of loadSplatFromPly incl. the
 *      [channel][coeff] -> [coeff][channel] sh transpose (:814-839) and the trailing
 *      convertCoordinates(RDF, to) (:842); cloud_to_rows replaces the row assembly of
 *      saveSplatToPly with its from->RDF flips (:858-893).  sh_dim is the number of sh
 *      coefficients per channel actually present (0..15; 0,3,8,15 for degrees 0..3). ------------ */
typedef struct {
  int32_t stride;      /* floats per row (= number of properties), 14 + 3*sh_dim .. 255 */
  int32_t sh_dim;      /* 0..15 */
  int32_t position[3]; /* x, y, z */
  int32_t scale[3];    /* scale_0, scale_1, scale_2 */
  int32_t rotation[4]; /* rot_1, rot_2, rot_3, rot_0  (cloud order x y z w; the file is w x y z) */
  int32_t alpha;       /* opacity */
  int32_t color[3];    /* f_dc_0, f_dc_1, f_dc_2 */
  int32_t sh[45];      /* f_rest_i, i < 3*sh_dim, file order [channel][coeff] */
} spz_amd_ply_columns;

/* The layout saveSplatToPly writes (load-spz.cc:900-922): x y z nx ny nz f_dc_0..2 f_rest_* opacity
 * scale_0..2 rot_0..3; stride = 17 + 3*sh_dim. */
int spz_amd_ply_default_columns(int sh_dim, spz_amd_ply_columns *out);
int spz_amd_ply_rows_to_cloud_device(const float *d_rows, uint64_t num_points, const spz_amd_ply_columns *cols,
                                     int to_coord, const spz_amd_cloud_out *d_cloud, void *hip_stream);
int spz_amd_cloud_to_ply_rows_device(const spz_amd_cloud_in *d_cloud, uint64_t num_points, int sh_dim,
                                     int from_coord, float *d_rows, void *hip_stream);
int spz_amd_ply_rows_to_cloud_host(const float *h_rows, uint64_t num_points, const spz_amd_ply_columns *cols,
                                   int to_coord, const spz_amd_cloud_out *h_cloud, int device);
int spz_amd_cloud_to_ply_rows_host(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_dim,
                                   int from_coord, float *h_rows, int device);

/* ---- tables.  The alpha / colour decode tables (invSigmoid(b/255) load-spz.cc:87,518;
 *      ((b/255)-0.5)/0.15 :522) and the 255 alpha-encode thresholds (smallest float whose
 *      toUint8(sigmoid(a)*255) (:85,301) is >= v) are computed once on the host with the
 *      reference's own expressions and libm, then kept in device memory.  This accessor
 *      returns the host copies (for tests); any pointer may be NULL. ------------------------ */
int spz_amd_get_tables(float alpha_decode[256], float color_decode[256], float alpha_thresholds[255]);

/* ---- self test of the kernels' arithmetic.  Inside an exponent window the quaternion kernels divide
 *      without the IEEE expansion's operand scaling (reciprocal multiply + fma residual corrections,
 *      spz_kernels.hip); this runs, on the device, the comparison of each such form with the plain IEEE
 *      operation it replaces over inputs begin .. begin+count of `mode`:
 *        0  x / 0.70710677f (load-spz.cc:46,244)   x = the float with bit pattern i, window [2^-100, 2^126] and 0
 *        1  x / 511.0f      (load-spz.cc:366)      likewise
 *        2  sqrt            (splat-types.cc:72)    x = bit pattern i, window [2^-80, 2^82]
 *        3  x_i / norm      (splat-types.cc:73)    operand pair hashed from i
 *        4  packQuaternionSmallestThree, 5 the v2 first-three encoder: quaternion hashed from i
 *        6  unpackQuaternionSmallestThree: comp = low 32 bits of i, flips = bits 32..34
 *      result[0] = inputs whose bits differ (must be 0), result[1] = the smallest such i (~0 if none),
 *      result[2] = inputs actually compared (those inside the mode's window).  Blocking. -------------- */
int spz_amd_selftest_device(int mode, uint64_t begin, uint64_t count, uint64_t result[3], void *hip_stream);

/* ---- container stage: zlib's LZ77 parse on the device, exact.  compressGzipped
 *      (load-spz.cc:186-214: one zlib stream, Z_DEFAULT_COMPRESSION, memLevel 9) is what is left of a saveSpz once
 *      the quantise step runs on the GPU, and its output has to stay the reference's bytes.  These entry points
 *      produce the literal/match symbols zlib 1.2.11's deflate_slow + longest_match produce for h_data[0 .. ) up to
 *      the point where they meet the caller's own serial parse of the input's end (`tail_begin`, a multiple of
 *      32768 with 64-96 KiB after it; h_tail_rec: 32768 pairs {lazy-match state, symbols emitted so far} recorded at the
 *      loop tops tail_begin + k of that parse, state 0 where k is not a loop top — spz_deflate.cpp's TopRec).
 *      open: uploads, runs the stages (spz_lz77.hip), returns the symbol count and the index of the first symbol
 *      the tail parse contributes; fetch: copies the symbols out (distance, 0 = literal; literal byte or
 *      length - 3); close: frees the device memory.  SPZ_AMD_ERR_UNSUPPORTED = declined (two neighbouring jobs did not
 *      meet even with parse jobs of 1 MiB, or not enough free device memory: ~25 bytes per input byte): the caller parses on
 *      the host, with the same result.  Blocking; Huffman coding and the gzip framing stay on the host. ---------- */
int spz_amd_zlib_parse_open(const uint8_t *h_data, uint64_t size, uint64_t tail_begin, const uint32_t *h_tail_rec,
                            uint32_t n_rec, int device, void **ctx, uint64_t *num_symbols,
                            uint32_t *tail_first_symbol);
/* The same; produce_tail_rec(arg), if given, is called on the calling thread once the input is on the device and the
 * table and match kernels are running (~90 ms of device work for 650 MB): h_tail_rec need not be filled before it
 * returns, so the caller's serial parse of the input's end can run there instead of before the call. */
int spz_amd_zlib_parse_open_ex(const uint8_t *h_data, uint64_t size, uint64_t tail_begin, const uint32_t *h_tail_rec,
                               uint32_t n_rec, int device, void **ctx, uint64_t *num_symbols,
                               uint32_t *tail_first_symbol, void (*produce_tail_rec)(void *), void *produce_arg);
/* The same for a caller whose input is what spz_amd_encode_host_keep just produced: d_copy (may be NULL) = the
 * device copy of h_data's bytes, on `device`; the upload is then a device-to-device copy. */
int spz_amd_zlib_parse_open_dev(const uint8_t *h_data, const uint8_t *d_copy, uint64_t size, uint64_t tail_begin,
                                const uint32_t *h_tail_rec, uint32_t n_rec, int device, void **ctx,
                                uint64_t *num_symbols, uint32_t *tail_first_symbol, void (*produce_tail_rec)(void *),
                                void *produce_arg);
int spz_amd_zlib_parse_fetch(void *ctx, uint16_t *h_dist, uint8_t *h_lc);
void spz_amd_zlib_parse_close(void *ctx);

/* The Huffman stage of the same member, with the symbols still on the device (trees.c: _tr_tally's counts and
 * compress_block's bit string; the trees — build_tree / gen_bitlen / gen_codes, the stored / static / dynamic
 * choice and the tree headers — are built by the caller from the counts, spz_deflate.cpp).
 *   append        the caller's own symbols of the input's end behind the device's;
 *   block_stats   block b = symbols [b * block_symbols, ...): literal/length and distance frequencies
 *                 ([num_blocks][286], [num_blocks][30]; END_BLOCK not counted), input bytes covered, length of the
 *                 last symbol;
 *   encode_blocks writes every block's header words (placed by the caller on the 32-bit grid of the deflate body,
 *                 which starts at bit 0) and its symbols with the block's codes (or, choice 0, the stored input
 *                 bytes) into a body of body_bytes and copies it to h_body; h_symbol_bits[b] = bits the block's
 *                 symbols + END_BLOCK took (for the caller's check against its plan).
 * The static tables of trees.c (length_code, dist_code, base_length, base_dist, extra bits) come from the caller. */
typedef struct {
  uint8_t length_code[256];
  uint8_t dist_code[512];
  uint16_t base_length[29];
  uint16_t base_dist[30];
  uint8_t extra_lbits[29];
  uint8_t extra_dbits[30];
  uint8_t pad_[3];
} spz_amd_deflate_static;
typedef struct {
  uint64_t bit_start;          /* of the block in the deflate body */
  uint32_t header_word_begin;  /* index into the header word array */
  uint32_t header_words;       /* words, the first one aligned down to the 32-bit grid at bit_start */
  uint32_t header_bits;        /* bits from bit_start to the first symbol (stored: to the first input byte) */
  uint32_t choice;             /* 0 stored, 1 static, 2 dynamic */
  uint32_t input_begin;        /* stored blocks: the input range */
  uint32_t input_bytes;
} spz_amd_deflate_block;
typedef struct {
  uint16_t lcode[286];
  uint16_t dcode[30];
  uint8_t llen[286];
  uint8_t dlen[30];
} spz_amd_deflate_codes;
int spz_amd_zlib_parse_append(void *ctx, const uint16_t *h_dist, const uint8_t *h_lc, uint64_t n);
int spz_amd_zlib_block_stats(void *ctx, const spz_amd_deflate_static *tables, uint32_t block_symbols,
                             uint32_t num_blocks, uint16_t *h_lfreq, uint16_t *h_dfreq, uint32_t *h_bytes,
                             uint32_t *h_last_len);
/* The trees on the device as well (same source as the caller's: spz_huff_core.hpp).  block_trees (after block_stats,
 * whose h_lfreq / h_dfreq may then both be NULL) builds every block's three trees and returns the two lengths
 * _tr_flush_block chooses by; the caller lays the blocks out (bit_start, choice, stored input range; the header_*
 * fields are filled on the device), encode_planned enqueues the writing of headers and symbols and
 * encode_finish_ex (below) copies out the body and each block's symbol bits and header bits.  The order is
 * enforced: block_trees returns SPZ_AMD_ERR_INVALID_ARG unless block_stats has run for the same num_blocks, and
 * encode_planned unless block_trees has. */
typedef struct {
  int64_t opt_len;
  int64_t static_len;
} spz_amd_deflate_plan;
int spz_amd_zlib_block_trees(void *ctx, uint32_t num_blocks, spz_amd_deflate_plan *h_plan);
int spz_amd_zlib_encode_planned(void *ctx, const spz_amd_deflate_static *tables, uint32_t block_symbols,
                                uint32_t num_blocks, const spz_amd_deflate_block *h_blocks, uint64_t body_bytes);
/* encode_blocks in pieces: encode_group enqueues blocks [first_block, first_block + group_blocks) of total_blocks (the
 * arrays hold the group's entries, header_word_begin counts from the group's first header word; the first group zeroes
 * a body of body_bytes_bound) and returns without waiting — the caller builds the next group's trees meanwhile;
 * encode_finish waits and copies the body and every block's bit count out. */
int spz_amd_zlib_encode_group(void *ctx, const spz_amd_deflate_static *tables, uint32_t block_symbols,
                              uint32_t total_blocks, uint32_t first_block, uint32_t group_blocks,
                              const spz_amd_deflate_block *h_blocks, const spz_amd_deflate_codes *h_codes,
                              const uint32_t *h_header_words, uint64_t num_header_words, uint64_t body_bytes_bound);
int spz_amd_zlib_encode_finish(void *ctx, uint32_t total_blocks, uint64_t body_bytes, uint8_t *h_body,
                               uint64_t *h_symbol_bits);
int spz_amd_zlib_encode_finish_ex(void *ctx, uint32_t total_blocks, uint64_t body_bytes, uint8_t *h_body,
                                  uint64_t *h_symbol_bits, uint32_t *h_header_bits /* may be NULL */);
/* The same parse with its table and match stages fed while the input is still being produced (saveSpz: the quantise step's
 * sections become final one after the other while the floats upload, and the device would idle through that upload).
 * session_open(size): the parse's device memory for an input of `size` bytes (SPZ_AMD_ERR_UNSUPPORTED: declined, as
 * parse_open_dev would).  session_feed: bytes [0, final_upto) of d_stream are final once the work queued on
 * `producer_stream` so far is done — they are copied and the table / match kernels for what they cover are enqueued on
 * the session's own stream; returns at once; final_upto must not decrease.  parse_open_session consumes the session
 * (also on failure): whatever has not been fed comes from d_stream (all of it final by now) and the call goes on as
 * parse_open_dev.  session_close: for a session that is not going to be consumed.  spz_amd_encode_host_keep_session is
 * spz_amd_encode_host_keep feeding such a session: the five small sections of all points first, then sh chunk by chunk. */
int spz_amd_zlib_session_open(uint64_t size, int device, void **session);
int spz_amd_zlib_session_feed(void *session, const uint8_t *d_stream, uint64_t final_upto, void *producer_stream);
void spz_amd_zlib_session_close(void *session);
int spz_amd_zlib_parse_open_session(void *session, const uint8_t *h_data, const uint8_t *d_stream, uint64_t size, uint64_t tail_begin,
                                    const uint32_t *h_tail_rec, uint32_t n_rec, void **ctx, uint64_t *num_symbols,
                                    uint32_t *tail_first_symbol, void (*produce_tail_rec)(void *), void *produce_arg);
int spz_amd_encode_host_keep_session(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_degree, int antialiased,
                                     int from_coord, int version, uint8_t *h_stream, size_t capacity, int device,
                                     const uint8_t **d_stream, void *zlib_session);
/* The same for a caller with work of its own on the END of the stream (the container stage's serial tail job: ~8 ms of one
 * host core on the last 64 ... 128 KiB): the sh of the last points go up first, and tail_ready(tail_arg) is called — on
 * the call's download thread; it must return quickly, e.g. after starting a thread — as soon as the stream's last
 * tail_bytes (at least) are in h_stream, long before the call returns.  Not called when tail_bytes is 0, the cloud has
 * no sh, or it is too small for the reordering to pay (the caller then does that work after the call, as without this). */
int spz_amd_encode_host_keep_session_tail(const spz_amd_cloud_in *h_cloud, uint64_t num_points, int sh_degree, int antialiased,
                                          int from_coord, int version, uint8_t *h_stream, size_t capacity, int device,
                                          const uint8_t **d_stream, void *zlib_session, size_t tail_bytes,
                                          void (*tail_ready)(void *), void *tail_arg);
/* Every encode_finish(_ex) returns SPZ_AMD_ERR_VERIFY instead of a body when the symbols it was coded from do not
 * reproduce the input (checked on the device for every block, always: each literal is its input byte, each match
 * copies equal bytes from at most 32 KiB back, each block covers exactly its input range).
 * verify_member (after encode_finish(_ex), before close): inflates the body where it still lies in device memory with
 * the device reader below and compares the result with the input byte for byte: SPZ_AMD_OK = equal, SPZ_AMD_ERR_VERIFY =
 * not, SPZ_AMD_ERR_UNSUPPORTED = the device reader declines this body (the caller checks on the host). */
int spz_amd_zlib_verify_member(void *ctx, uint64_t body_bytes);
int spz_amd_zlib_encode_blocks(void *ctx, const spz_amd_deflate_static *tables, uint32_t block_symbols,
                               uint32_t num_blocks, const spz_amd_deflate_block *h_blocks,
                               const spz_amd_deflate_codes *h_codes, const uint32_t *h_header_words,
                               uint64_t num_header_words, uint64_t body_bytes, uint8_t *h_body,
                               uint64_t *h_symbol_bits);

/* ---- container stage, reading: inflate of one ordinary deflate stream on the device (spz_inflate_dev.hip).  The
 *      reference's files are a single zlib stream (decompressGzipped, load-spz.cc:141-184); it is cut into 64 KiB
 *      chunks whose block starts are found by search, decoded in parallel without their left context and resolved
 *      afterwards (the scheme of spz_inflate.cpp).  h_deflate: the raw deflate data of a gzip member (after its
 *      header, before its 8-byte trailer).  open: decodes; *out_bytes = size of the result, which stays on the
 *      device.  piece_crcs: CRC-32 of consecutive pieces of crc_piece_bytes() of the result — the caller folds them
 *      (crc32_combine) and compares with the trailer's CRC-32 and ISIZE before it believes the result.  fetch: the
 *      bytes; device_data: the device pointer (a decode can read the stream where it is).  close: frees.
 *      SPZ_AMD_ERR_UNSUPPORTED = declined (no usable block starts, chunks that do not link up, a chunk that expands
 *      more than 8 x, not enough device memory): the caller's host readers take over.  Blocking. ------------------- */
int spz_amd_inflate_open(const uint8_t *h_deflate, uint64_t nbytes, int device, void **ctx, uint64_t *out_bytes);
/* inflate_open with a callback that runs on the calling thread once the deflate data is on the device (an upload that is
 * blocking: the data is there when it runs) and before the kernels are waited for: host-side work of the caller that would
 * contend with the upload but not with the kernels (loadSpz maps its output pages there).  Not called when the open
 * fails before or during the upload. */
int spz_amd_inflate_open_ex(const uint8_t *h_deflate, uint64_t nbytes, int device, void **ctx, uint64_t *out_bytes,
                            void (*after_upload)(void *), void *after_arg);
/* the same for deflate data that is in device memory already; equals_device: is the result these nbytes (device memory)? */
int spz_amd_inflate_open_device(const uint8_t *d_deflate, uint64_t nbytes, int device, void **ctx, uint64_t *out_bytes);
int spz_amd_inflate_equals_device(void *ctx, const uint8_t *d_expected, uint64_t nbytes);
/* A context of the same kind around a stream the CALLER has inflated (a member the device reader declines, a raw
 * stream): the bytes are uploaded and stay in device memory until spz_amd_inflate_close; device_data / piece_crcs /
 * fetch work as after inflate_open.  With it "file -> packed sections left in HBM" (loadSpzPacked for renderers,
 * load-spz.cc:609-632) has one shape whichever reader inflated the member. */
int spz_amd_stream_to_device(const uint8_t *h_stream, uint64_t nbytes, int device, void **ctx);
uint32_t spz_amd_inflate_crc_piece_bytes(void);
/* Why the last inflate_open(_device) of this thread returned SPZ_AMD_ERR_UNSUPPORTED ("" when it did not): one of
 * size, stored-first, memory, no-block-starts, symbol-budget, expansion, no-final-block, not-linked, trailing-bytes,
 * empty, window-chains, bad-reference.  The caller's host readers give the same bytes; this tells a slowdown's cause. */
const char *spz_amd_inflate_last_decline(void);
int spz_amd_inflate_piece_crcs(void *ctx, uint32_t *h_crcs, uint32_t capacity, uint32_t *num_pieces);
int spz_amd_inflate_fetch(void *ctx, uint8_t *h_out);
const uint8_t *spz_amd_inflate_device_data(void *ctx);
void spz_amd_inflate_close(void *ctx);

#ifdef __cplusplus
}
#endif
#endif /* SPZ_AMD_H_ */
