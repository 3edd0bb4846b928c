// spz_view_pass.hpp — what prune, compare and refine share above the rasteriser's device entry points (host code only):
// the argument checks of a view list and of a packed input, and the first stage of one view.
//
//   per view                       prepare_view: the render workspace made large enough for the prepare part,
//                                  spz_amd_render_prepare_{packed,cloud}_device, the entry total read back, then the
//                                  workspace grown for that total (grow-only, the prepare part copied to the front of
//                                  the new block).  The second stage (score, finish, backward) is the caller's, on the
//                                  same workspace and total.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "spz_amd.h"
#include "spz_common.hpp"

namespace spz_amd_detail {

// What a view is rendered from: a packed stream with its header, or a float cloud (`cloud` set).
struct RenderSource {
  const uint8_t *d_stream = nullptr;  // packed
  size_t size = 0;
  const spz_amd_header *hdr = nullptr;
  const spz_amd_cloud_in *cloud = nullptr;  // float
  uint64_t n = 0;
  int sh_degree = 0, antialiased = 0;
};

inline RenderSource packed_render_source(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr) {
  RenderSource s;
  s.d_stream = d_stream;
  s.size = size;
  s.hdr = hdr;
  s.n = hdr->num_points;
  return s;
}

// A view list: 1..max_views views that pass spz_amd_render_check_params, all in the frame of the first.  The index of
// the first view that does not into *h_bad_view (may be NULL; the caller has set it to -1).
inline int check_views(const spz_amd_render_params *views, int num_views, int max_views, int32_t *h_bad_view) {
  if (views == nullptr || num_views < 1 || num_views > max_views) return SPZ_AMD_ERR_INVALID_ARG;
  for (int v = 0; v < num_views; ++v) {
    if (spz_amd_render_check_params(&views[v]) != SPZ_AMD_OK || views[v].coord != views[0].coord) {
      if (h_bad_view) *h_bad_view = v;
      return SPZ_AMD_ERR_INVALID_ARG;
    }
  }
  return SPZ_AMD_OK;
}

// A packed input of a view pass, before anything is launched: check_packed_stream's order, with the rasteriser's cap
// on the point count in front of the stream's length.
inline int check_render_input(const uint8_t *d_stream, size_t size, const spz_amd_header *hdr) {
  spz_amd_layout lay;
  const int rc = check_packed_stream(d_stream, size, hdr, &lay);
  if ((rc == SPZ_AMD_OK || rc == SPZ_AMD_ERR_SHORT_STREAM) && hdr->num_points > kMaxEntries) {
    return SPZ_AMD_ERR_TOO_MANY_POINTS;
  }
  return rc;
}

// The first stage of one view of `src` in the caller's render workspace *ws of *cap bytes (NULL and 0 at first; the
// caller frees it): prepare, the entry total into *h_total, the workspace grown to hold that total's entries.  Work
// enqueued earlier on `st` may still read *ws.  A total above the sort's limit: SPZ_AMD_ERR_CAPACITY, *h_total set.
inline int prepare_view(uint8_t **ws, uint64_t *cap, const RenderSource &src, const spz_amd_render_params *p,
                        uint64_t *d_total, hipStream_t st, uint64_t *h_total) {
  const uint64_t prefix = spz_amd_render_workspace_bytes(src.n, 0) - 256u;
  if (*cap < prefix + 256u) {
    if (*ws) {
      SPZ_HIP_TRY(hipStreamSynchronize(st));  // an earlier view's blend may still read it
      SPZ_HIP_TRY(hipFree(*ws));
    }
    *ws = nullptr;
    *cap = 0;
    SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(ws), prefix + 256u));
    *cap = prefix + 256u;
  }
  const int rc = src.cloud ? spz_amd_render_prepare_cloud_device(src.cloud, src.n, src.sh_degree, src.antialiased, p,
                                                                  d_total, nullptr, *ws, st)
                           : spz_amd_render_prepare_packed_device(src.d_stream, src.size, src.hdr, p, d_total, nullptr,
                                                                  *ws, st);
  if (rc != SPZ_AMD_OK) return rc;
  *h_total = 0;
  SPZ_HIP_TRY(hipMemcpyAsync(h_total, d_total, 8, hipMemcpyDeviceToHost, st));
  SPZ_HIP_TRY(hipStreamSynchronize(st));
  if (*h_total > kMaxEntries) return SPZ_AMD_ERR_CAPACITY;
  const uint64_t need = spz_amd_render_workspace_bytes(src.n, *h_total);
  if (need > *cap) {
    uint8_t *bigger = nullptr;
    SPZ_HIP_TRY(hipMalloc(reinterpret_cast<void **>(&bigger), need));
    if (prefix) {
      const hipError_t e = hipMemcpyAsync(align_ws(bigger), align_ws(*ws), prefix, hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess) (void)hipStreamSynchronize(st);
      if (e != hipSuccess) {
        (void)hipFree(bigger);
        g_last_hip_error = (int)e;
        return SPZ_AMD_ERR_HIP;
      }
    }
    SPZ_HIP_TRY(hipFree(*ws));
    *ws = bigger;
    *cap = need;
  }
  return SPZ_AMD_OK;
}

// One view of `src` into d_image: prepare_view, then the entries and the blend.
inline int render_view(uint8_t **ws, uint64_t *cap, const RenderSource &src, const spz_amd_render_params *p,
                       uint64_t *d_total, uint32_t *d_status, float *d_image, hipStream_t st, uint64_t *h_total) {
  const int rc = prepare_view(ws, cap, src, p, d_total, st, h_total);
  if (rc != SPZ_AMD_OK) return rc;
  return spz_amd_render_finish_device(src.n, p, *h_total, d_image, d_status, *ws, st);
}

}  // namespace spz_amd_detail
