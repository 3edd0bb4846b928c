"""Device-resident encode / decode over the C ABI, with torch tensors as the memory owner.

torch is plumbing here: it allocates HBM and names the HIP stream; every byte of work is done
by libspz_amd.so through raw pointers (spz_amd.abi).  Clouds are dicts of flat float32 CUDA
tensors keyed like the reference's GaussianCloud fields (splat-types.h:101-115):
positions[3N], scales[3N], rotations[4N], alphas[N], colors[3N], sh[N*shDim*3].
"""
import ctypes as C
import math

import torch

from . import abi
from .synth import FIELDS, SH_DIM, floats_per_point


def _stream_handle(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _ptrs(cloud, sh_degree, n, device):
    p = abi.CloudPtrs()
    for k in FIELDS:
        t = cloud.get(k)
        need = n * floats_per_point(k, sh_degree)
        if need == 0:
            setattr(p, k, None)
            continue
        if t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != need:
            raise ValueError(f"cloud[{k!r}] must be a contiguous float32 CUDA tensor of {need} elements")
        if t.device != device:
            raise ValueError(f"cloud[{k!r}] is on {t.device}, expected {device}")
        setattr(p, k, t.data_ptr())
    return p


def alloc_cloud(n, sh_degree, device):
    return {k: torch.empty(n * floats_per_point(k, sh_degree), dtype=torch.float32, device=device) for k in FIELDS}


class _DeviceArray:
    """A typed view of device memory somebody else owns (kept alive through `owner`), for torch.as_tensor."""

    def __init__(self, ptr, count, typestr, owner):
        self.ptr, self.count, self.typestr, self.owner = int(ptr), int(count), typestr, owner

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.count,), "typestr": self.typestr, "data": (self.ptr, False), "version": 2, "strides": None}


class PlacedBuffers:
    """Device buffers of one resident cloud made by spz_amd_cloud_buffers_alloc (spz_place.hip): `cloud` is the usual
    dict of flat float32 CUDA tensors, `stream` a uint8 CUDA tensor (this object's, or the caller's), `report` what
    the placement probe saw.  The memory goes when the object does (or at free()); tensors made from it must not
    outlive it."""

    def __init__(self, raw, n, sh_degree, device, stream_tensor=None):
        self._raw, self._freed = raw, False
        self.cloud = {}
        for k in FIELDS:
            cnt = n * floats_per_point(k, sh_degree)
            ptr = getattr(raw.cloud, k)
            self.cloud[k] = (torch.as_tensor(_DeviceArray(ptr, cnt, "<f4", self), device=device) if cnt
                             else torch.empty(0, dtype=torch.float32, device=device))
        self.stream = stream_tensor if stream_tensor is not None else torch.as_tensor(
            _DeviceArray(raw.stream, raw.stream_capacity, "|u1", self), device=device)
        self.report = {"sh_placements_timed": int(raw.candidates), "probe_ms_first": round(float(raw.probe_ms_first), 4),
                       "probe_ms_chosen": round(float(raw.probe_ms_chosen), 4), "probe_ms_slowest": round(float(raw.probe_ms_worst), 4)}

    def free(self):
        if not self._freed:
            self._freed = True
            self.cloud, self.stream = {}, None
            abi.load_library().spz_amd_cloud_buffers_free(C.byref(self._raw))

    def __del__(self):
        try:
            self.free()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def alloc_placed(n, sh_degree, device, version=3, stream_t=None, probe="decode", max_candidates=6, stream=None):
    """Buffers for a resident cloud of n points with the sh array placed for speed: the library times the
    launch they are for — probe "decode" (stream read, cloud written), "encode" (cloud read; the stream is OVERWRITTEN
    with zeros' code) or None — on up to `max_candidates` placements of the sh array and keeps the fastest.  `stream_t`:
    an existing stream tensor to place against (otherwise one is allocated with the small arrays)."""
    L = abi.load_library()
    raw = abi.CloudBuffers()
    mode = {None: 0, "none": 0, "decode": 1, "encode": 2}[probe]
    with torch.cuda.device(device):
        rc = L.spz_amd_cloud_buffers_alloc(int(n), int(sh_degree), int(version), stream_t.data_ptr() if stream_t is not None else None,
                                           mode, int(max_candidates), _stream_handle(stream), C.byref(raw))
    abi.check(rc, "spz_amd_cloud_buffers_alloc")
    return PlacedBuffers(raw, n, sh_degree, device, stream_t)


def make_header(num_points, sh_degree, version=3, fractional_bits=12, antialiased=False):
    return abi.Header(int(version), int(num_points), int(sh_degree), int(fractional_bits),
                      1 if antialiased else 0, 0)


def peek_header(stream_t, max_points=abi.REFERENCE_MAX_POINTS, stream=None):
    """Header checks of deserializePackedGaussians (load-spz.cc:551-568,591-594) on a device-resident
    stream.  Returns (status, Header or None)."""
    L = abi.load_library()
    h = abi.Header()
    with torch.cuda.device(stream_t.device):
        rc = L.spz_amd_peek_header_device(stream_t.data_ptr(), stream_t.numel(), int(max_points), C.byref(h),
                                          _stream_handle(stream))
    return rc, (h if rc == abi.OK else None)


class RawStream:
    """A device byte buffer known by address only (spz_amd_ipc_alloc / spz_amd_ipc_open).  `tensor()` gives a
    uint8 view of it for checks (through __cuda_array_interface__; the buffer must outlive the view)."""

    def __init__(self, ptr, nbytes):
        self.ptr, self.nbytes = int(ptr), int(nbytes)

    @property
    def __cuda_array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2, "strides": None}

    def tensor(self, device):
        return torch.as_tensor(self, device=device)


def encode(cloud, num_points, sh_degree, antialiased=False, from_coord=0, version=3, out=None, stream=None):
    """packGaussians + serializePackedGaussians on the GPU -> uint8 CUDA tensor holding the raw
    (pre-gzip) stream.  Asynchronous on `stream` (default: torch's current stream)."""
    L = abi.load_library()
    device = cloud["positions"].device if num_points else (out.device if out is not None else torch.device("cuda"))
    lay = abi.stream_layout(num_points, sh_degree, version)
    if out is None:
        out = torch.empty(lay.total_bytes, dtype=torch.uint8, device=device)
    p = _ptrs(cloud, sh_degree, num_points, device)
    with torch.cuda.device(device):
        rc = L.spz_amd_encode_device(C.byref(p), num_points, sh_degree, int(bool(antialiased)), from_coord, version,
                                     out.data_ptr(), out.numel(), _stream_handle(stream))
    abi.check(rc, "spz_amd_encode_device")
    return out[:lay.total_bytes]


def decode(stream_t, header, to_coord=0, out=None, stream=None):
    """unpackGaussians (+ fused coordinate flip) on the GPU.  `header` is an abi.Header (from
    abi.peek_header on host bytes, or make_header for a stream this process encoded)."""
    L = abi.load_library()
    n, deg = header.num_points, header.sh_degree
    if out is None:
        out = alloc_cloud(n, deg, stream_t.device)
    p = _ptrs(out, deg, n, stream_t.device)
    with torch.cuda.device(stream_t.device):
        rc = L.spz_amd_decode_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), to_coord, C.byref(p),
                                     _stream_handle(stream))
    abi.check(rc, "spz_amd_decode_device")
    return out


def encode_shard(cloud, first, count, num_points_total, sh_degree, out, antialiased=False, from_coord=0, version=3,
                 write_header=False, stream=None, section_mask=abi.ALL_SECTIONS):
    """Encode points [first, first+count) (cloud holds only those) into the FULL stream `out`: a uint8 CUDA
    tensor, or a RawStream (pointer + size: e.g. another process's buffer mapped over IPC).  section_mask
    restricts the launch to some of the six sections (abi.SMALL_SECTIONS / abi.SH_SECTION)."""
    L = abi.load_library()
    device = cloud["positions"].device
    p = _ptrs(cloud, sh_degree, count, device)
    ptr, size = (out.ptr, out.nbytes) if isinstance(out, RawStream) else (out.data_ptr(), out.numel())
    with torch.cuda.device(device):
        rc = L.spz_amd_encode_shard_sections_device(C.byref(p), first, count, num_points_total, sh_degree,
                                                    int(bool(antialiased)), from_coord, version, int(bool(write_header)),
                                                    int(section_mask), ptr, size, _stream_handle(stream))
    abi.check(rc, "spz_amd_encode_shard_sections_device")
    return out


def decode_shard(stream_t, header, first, count, to_coord=0, out=None, stream=None):
    L = abi.load_library()
    deg = header.sh_degree
    if out is None:
        out = alloc_cloud(count, deg, stream_t.device)
    p = _ptrs(out, deg, count, stream_t.device)
    with torch.cuda.device(stream_t.device):
        rc = L.spz_amd_decode_shard_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), first, count,
                                           to_coord, C.byref(p), _stream_handle(stream))
    abi.check(rc, "spz_amd_decode_shard_device")
    return out


def decode_gather(stream_t, header, indices, to_coord=0, out=None, stream=None):
    """Decode only the points `indices` (uint32/int32 CUDA tensor) of a packed device stream."""
    L = abi.load_library()
    count, deg = indices.numel(), header.sh_degree
    if indices.dtype not in (torch.int32, torch.uint32) or not indices.is_cuda or not indices.is_contiguous():
        raise ValueError("indices must be a contiguous int32/uint32 CUDA tensor")
    if out is None:
        out = alloc_cloud(count, deg, stream_t.device)
    p = _ptrs(out, deg, count, stream_t.device)
    with torch.cuda.device(stream_t.device):
        rc = L.spz_amd_decode_gather_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), indices.data_ptr(),
                                            count, to_coord, C.byref(p), _stream_handle(stream))
    abi.check(rc, "spz_amd_decode_gather_device")
    return out


def _selection(box, min_alpha, to_coord):
    import math
    sel = abi.Selection()
    sel.to_coord = int(to_coord)
    if not 0 <= sel.to_coord <= 8:
        raise ValueError(f"to_coord must be a CoordinateSystem value 0..8, got {to_coord}")
    if box is not None:
        rows = [[float(v) for v in row] for row in box]
        if len(rows) != 2 or any(len(r) != 3 for r in rows):
            raise ValueError("box must be [[x0, y0, z0], [x1, y1, z1]]")
        if any(math.isnan(v) for r in rows for v in r):
            raise ValueError("box bounds must not be NaN")
        sel.use_box = 1
        for a in range(3):
            sel.box_lo[a], sel.box_hi[a] = rows[0][a], rows[1][a]
    if min_alpha is not None:
        if math.isnan(float(min_alpha)):
            raise ValueError("min_alpha must not be NaN")
        sel.use_min_alpha, sel.min_alpha = 1, float(min_alpha)
    return sel


def select(stream_t, header, *, mask=None, box=None, min_alpha=None, to_coord=0, stream=None):
    """The indices (int32 CUDA tensor, input order) of the points of a packed device stream whose predicates all hold:
    mask[i] != 0 (a bool/uint8 CUDA tensor of num_points), the box [[x0, y0, z0], [x1, y1, z1]] (inclusive, positions
    as decode(to_coord) gives them), the decoded alpha logit >= min_alpha.  None of them: every point.  Blocks until the
    count is known (spz_amd_select_device)."""
    L = abi.load_library()
    sel = _selection(box, min_alpha, to_coord)
    n, dev = header.num_points, stream_t.device
    if mask is not None:
        if mask.dtype not in (torch.bool, torch.uint8) or not mask.is_cuda or not mask.is_contiguous() or mask.numel() != n:
            raise ValueError(f"mask must be a contiguous bool/uint8 CUDA tensor of {n} elements")
        if mask.device != dev:
            raise ValueError(f"mask is on {mask.device}, expected {dev}")
    out = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.spz_amd_filter_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    count = C.c_uint64(0)
    with torch.cuda.device(dev):
        rc = L.spz_amd_select_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), C.byref(sel),
                                     mask.data_ptr() if mask is not None else None, out.data_ptr() if n else None,
                                     ws.data_ptr() if n else None, C.byref(count), _stream_handle(stream))
    abi.check(rc, "spz_amd_select_device")
    return out[:count.value]


def subset(stream_t, header, indices, sh_degree=None, out=None, stream=None):
    """The stream of the points `indices` (int32/uint32 CUDA tensor; any order, duplicates allowed) of a packed device
    stream, with sh lowered to `sh_degree` (None: the input's): a uint8 CUDA tensor, no requantising.  An index >=
    num_points raises ValueError before the launch (the C ABI's device form clamps)."""
    L = abi.load_library()
    deg = -1 if sh_degree is None else int(sh_degree)
    if not -1 <= deg <= header.sh_degree:
        raise ValueError(f"sh_degree must be None, -1 or 0..{header.sh_degree}, got {sh_degree}")
    if indices.dtype not in (torch.int32, torch.uint32) or not indices.is_cuda or not indices.is_contiguous():
        raise ValueError("indices must be a contiguous int32/uint32 CUDA tensor")
    count, n = indices.numel(), header.num_points
    if count:
        wide = indices.view(torch.int32).to(torch.int64) & 0xffffffff
        if int(wide.max()) >= n or (indices.dtype == torch.int32 and int(indices.min()) < 0):
            raise ValueError(f"an index is out of range for {n} points")
    lay = abi.stream_layout(count, header.sh_degree if deg < 0 else deg, header.version)
    if out is None:
        out = torch.empty(lay.total_bytes, dtype=torch.uint8, device=stream_t.device)
    with torch.cuda.device(stream_t.device):
        rc = L.spz_amd_subset_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header),
                                     indices.data_ptr() if count else None, count, deg, out.data_ptr(), out.numel(),
                                     _stream_handle(stream))
    abi.check(rc, "spz_amd_subset_device")
    return out[:lay.total_bytes]


def transform(cloud, num_points, sh_degree, *, rotation=None, translation=None, scale=1.0, coord=0, stream=None):
    """p -> scale * R(rotation) * p + translation (stated in `coord`) in place on device tensors: positions, log-scales
    (+ log(scale)), rotations (q_R * q) and the sh bands (spz_amd_transform_cloud_device).  Any of the four may be
    missing.  A bad argument raises ValueError before the launch."""
    L = abi.load_library()
    xf = abi.transform_params(rotation, translation, scale, coord)
    if int(sh_degree) not in SH_DIM:
        raise ValueError(f"sh_degree must be 0..3, got {sh_degree}")
    dev = None
    ptrs = []
    for k in ("positions", "scales", "rotations", "sh"):
        t = cloud.get(k)
        need = num_points * floats_per_point(k, sh_degree)
        if t is None or need == 0:
            ptrs.append(None)
            continue
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != need:
            raise ValueError(f"cloud[{k!r}] must be a contiguous float32 CUDA tensor of {need} elements")
        if dev is not None and t.device != dev:
            raise ValueError(f"cloud[{k!r}] is on {t.device}, expected {dev}")
        dev = t.device
        ptrs.append(t.data_ptr())
    if dev is None:
        return cloud
    with torch.cuda.device(dev):
        rc = L.spz_amd_transform_cloud_device(*ptrs, num_points, sh_degree, C.byref(xf), _stream_handle(stream))
    abi.check(rc, "spz_amd_transform_cloud_device")
    return cloud


def transform_packed(stream_t, header, *, rotation=None, translation=None, scale=1.0, coord=0, fractional_bits=12,
                     out=None, stream=None):
    """transform() on a packed device stream (any version) in one pass: returns (v3 stream as a uint8 CUDA tensor with
    positions at `fractional_bits`, out-of-range count as a 1-element int64 CUDA tensor).  The count is of the points
    whose new position does not fit the 24-bit field; their bytes wrap (spz_amd_transform_packed_device)."""
    L = abi.load_library()
    xf = abi.transform_params(rotation, translation, scale, coord)
    if isinstance(fractional_bits, bool) or not isinstance(fractional_bits, int) or not 0 <= fractional_bits <= 24:
        raise ValueError(f"fractional_bits must be an int in [0, 24], got {fractional_bits!r}")
    if stream_t.dtype != torch.uint8 or not stream_t.is_cuda or not stream_t.is_contiguous():
        raise ValueError("stream_t must be a contiguous uint8 CUDA tensor")
    lay = abi.stream_layout(header.num_points, header.sh_degree, 3)
    if out is None:
        out = torch.empty(lay.total_bytes, dtype=torch.uint8, device=stream_t.device)
    bad = torch.empty(1, dtype=torch.int64, device=stream_t.device)
    with torch.cuda.device(stream_t.device):
        rc = L.spz_amd_transform_packed_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), C.byref(xf),
                                               fractional_bits, out.data_ptr(), out.numel(), bad.data_ptr(),
                                               _stream_handle(stream))
    abi.check(rc, "spz_amd_transform_packed_device")
    return out[:lay.total_bytes], bad


def merge_packed(streams, headers, *, transforms=None, sh_degree=None, fractional_bits=None, antialiased=None, out=None,
                 stream=None):
    """K packed device streams (any version) -> one v3 stream, input 0's points first, in one launch
    (spz_amd_merge_device): bytes are copied wherever the encoding and the placement allow.  transforms: None or one
    entry per input, None or a dict of rotation / translation / scale / coord (transform's arguments).  sh_degree (None:
    the largest input degree), fractional_bits (None: the v2/v3 inputs' common value, else 12), antialiased (None: the
    inputs must agree).  Returns (uint8 CUDA tensor, output Header, out-of-range count as a 1-element int64 CUDA tensor:
    the points whose position does not fit 24 bits at the output's fractional_bits; their bytes wrap).  A bad argument
    or a conflict raises ValueError before any device work."""
    L = abi.load_library()
    streams, headers = list(streams), list(headers)
    k = len(streams)
    if k == 0 or k > abi.MERGE_MAX_INPUTS:
        raise ValueError(f"merge_packed takes 1 ... {abi.MERGE_MAX_INPUTS} streams, got {k}")
    if len(headers) != k:
        raise ValueError(f"{len(headers)} headers for {k} streams")
    for name, v, hi in (("sh_degree", sh_degree, 3), ("fractional_bits", fractional_bits, 24), ("antialiased", antialiased, 1)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= hi):
            raise ValueError(f"{name} must be None or an int in [0, {hi}], got {v!r}")
    if transforms is not None:
        transforms = list(transforms)
        if len(transforms) != k:
            raise ValueError(f"{len(transforms)} transforms for {k} streams")
    xfs = []
    for i in range(k):
        t = None if transforms is None else transforms[i]
        if t is None:
            xfs.append(None)
            continue
        if not isinstance(t, dict) or not set(t) <= {"rotation", "translation", "scale", "coord"}:
            raise ValueError(f"transforms[{i}] must be None or a dict of rotation / translation / scale / coord")
        xfs.append(abi.transform_params(t.get("rotation"), t.get("translation"), t.get("scale", 1.0),
                                        int(t.get("coord", abi.UNSPECIFIED))))
    dev = None
    for i, st in enumerate(streams):
        if st.dtype != torch.uint8 or not st.is_cuda or not st.is_contiguous():
            raise ValueError(f"streams[{i}] must be a contiguous uint8 CUDA tensor")
        if dev is not None and st.device != dev:
            raise ValueError(f"streams[{i}] is on {st.device}, expected {dev}")
        dev = st.device
    rc, hdr, nbytes = abi.merge_resolve(headers, sh_degree, fractional_bits, antialiased)
    if rc != abi.OK:
        aa = [h.flags & 1 for h in headers]
        if antialiased is None and len(set(aa)) > 1:
            j = next(i for i, a in enumerate(aa) if a != aa[0])
            raise ValueError(f"input 0 has antialiased = {aa[0]} and input {j} has antialiased = {aa[j]} (set antialiased)")
        raise ValueError(f"the streams cannot be merged: {abi.status_string(rc)}")
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(int(L.spz_amd_merge_workspace_bytes(k)), dtype=torch.uint8, device=dev)
    bad = torch.empty(1, dtype=torch.int64, device=dev)
    ins = (abi.MergeInput * k)()
    for i in range(k):
        ins[i].d_stream = streams[i].data_ptr()
        ins[i].size = streams[i].numel()
        ins[i].hdr = headers[i]
        ins[i].xf = C.pointer(xfs[i]) if xfs[i] is not None else None
    with torch.cuda.device(dev):
        rc = L.spz_amd_merge_device(ins, k, C.byref(hdr), out.data_ptr(), out.numel(), ws.data_ptr(), bad.data_ptr(),
                                    _stream_handle(stream))
    abi.check(rc, "spz_amd_merge_device")
    if stream is not None:  # the workspace was allocated on the current stream; the launch reads it on `stream`
        ws.record_stream(stream)
    return out[:nbytes], hdr, bad


def _check_stream_tensor(stream_t):
    if stream_t.dtype != torch.uint8 or not stream_t.is_cuda or not stream_t.is_contiguous():
        raise ValueError("the stream must be a contiguous uint8 CUDA tensor")


def _check_descending(descending):
    if not isinstance(descending, bool):
        raise ValueError(f"descending must be a bool, got {descending!r}")


def morton_order(stream_t, header, descending=False, stream=None):
    """The point order of a packed device stream by the 72-bit Morton key of its stored 24-bit positions (int32 CUDA
    tensor of num_points; spz_amd_morton_order_device): key ascending (or descending), ties in input order.  subset(
    stream_t, header, order) is the sorted stream.  A version 1 stream (float16 positions) raises ValueError."""
    L = abi.load_library()
    _check_stream_tensor(stream_t)
    _check_descending(descending)
    if header.version == 1:
        raise ValueError("a version 1 stream has float16 positions and no Morton key (transform_packed writes a v3 copy)")
    n, dev = header.num_points, stream_t.device
    out = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.spz_amd_sort_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.spz_amd_morton_order_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), 1 if descending else 0,
                                           out.data_ptr() if n else None, ws.data_ptr() if n else None,
                                           _stream_handle(stream))
    abi.check(rc, "spz_amd_morton_order_device")
    if stream is not None:  # the workspace was allocated on the current stream; the launches use it on `stream`
        ws.record_stream(stream)
    return out


def argsort(keys_t, descending=False, stream=None):
    """The stable argsort of a 1-D float32 CUDA tensor (int32 CUDA tensor; spz_amd_argsort_f32_device): the order of
    numpy's argsort(k, kind="stable"), or of argsort(-k) when descending: -0 == +0, every NaN last in both directions.
    A resident cloud is reordered with index_select on each array's (num_points, -1) view."""
    L = abi.load_library()
    _check_descending(descending)
    if keys_t.dtype != torch.float32 or not keys_t.is_cuda or keys_t.dim() != 1 or not keys_t.is_contiguous():
        raise ValueError("keys must be a contiguous 1-D float32 CUDA tensor")
    n, dev = keys_t.numel(), keys_t.device
    if n >= 2 ** 31:
        raise ValueError(f"{n} keys: at most 2^31 - 1")
    out = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.spz_amd_sort_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.spz_amd_argsort_f32_device(keys_t.data_ptr() if n else None, n, 1 if descending else 0,
                                          out.data_ptr() if n else None, ws.data_ptr() if n else None,
                                          _stream_handle(stream))
    abi.check(rc, "spz_amd_argsort_f32_device")
    if stream is not None:
        ws.record_stream(stream)
    return out


def chunk_bounds(stream_t, header, chunk=256, stream=None):
    """Per run of `chunk` consecutive points of a packed v2/v3 device stream (the last may be partial), the min and max
    of the stored positions per axis as float32 (the integer times 2^-fractional_bits, exact; stored RUB frame): a
    float32 CUDA tensor of shape (ceil(num_points / chunk), 2, 3) (spz_amd_chunk_bounds_device)."""
    L = abi.load_library()
    _check_stream_tensor(stream_t)
    if isinstance(chunk, bool) or not isinstance(chunk, int) or not 1 <= chunk <= 0xffffffff:
        raise ValueError(f"chunk must be an int >= 1, got {chunk!r}")
    if header.version == 1:
        raise ValueError("a version 1 stream has float16 positions (transform_packed writes a v3 copy)")
    n = header.num_points
    c = (n + chunk - 1) // chunk
    out = torch.empty((c, 2, 3), dtype=torch.float32, device=stream_t.device)
    with torch.cuda.device(stream_t.device):
        rc = L.spz_amd_chunk_bounds_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), chunk,
                                           out.data_ptr() if n else None, _stream_handle(stream))
    abi.check(rc, "spz_amd_chunk_bounds_device")
    return out


def _check_decimate_stream(stream_t, header):
    _check_stream_tensor(stream_t)
    if header.version == 1:
        raise ValueError("a version 1 stream has float16 positions and no integer cell (transform_packed writes a v3 "
                         "copy)")


def level_counts(stream_t, header, stream=None):
    """cells(L) for L = 0..24 of a packed v2/v3 device stream (int64 CUDA tensor of 25;
    spz_amd_decimate_level_counts_device): the number of occupied octree cells of edge 2^L quanta, counted over the
    Morton-sorted stream."""
    L = abi.load_library()
    _check_decimate_stream(stream_t, header)
    n, dev = header.num_points, stream_t.device
    out = torch.empty(25, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.spz_amd_decimate_workspace_bytes(n, header.sh_degree)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.spz_amd_decimate_level_counts_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header),
                                                    out.data_ptr(), ws.data_ptr(), _stream_handle(stream))
    abi.check(rc, "spz_amd_decimate_level_counts_device")
    if stream is not None:  # the workspace was allocated on the current stream; the launches use it on `stream`
        ws.record_stream(stream)
    return out


def decimate_packed(stream_t, header, level, stream=None):
    """One point per occupied octree cell of edge 2^level quanta of a packed v2/v3 device stream
    (spz_amd_decimate_device; the contract is in include/spz_amd.h).  Returns (stream uint8 CUDA tensor, Header,
    parents int32 CUDA tensor of num_points: the output index of every input point's cell).  The cell count comes from
    level_counts first (one small read-back), so the stream is sorted twice."""
    L = abi.load_library()
    _check_decimate_stream(stream_t, header)
    if isinstance(level, bool) or not isinstance(level, int) or not 0 <= level <= 24:
        raise ValueError(f"level must be an int in 0..24, got {level!r}")
    n, dev = header.num_points, stream_t.device
    m = 0
    if n:
        counts = level_counts(stream_t, header, stream)
        if stream is not None:
            stream.synchronize()
        m = int(counts[level].item())
    nbytes = abi.stream_layout(m, header.sh_degree, 3).total_bytes
    out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    parents = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.spz_amd_decimate_workspace_bytes(n, header.sh_degree)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.spz_amd_decimate_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), level, out.data_ptr(),
                                       nbytes, parents.data_ptr() if n else None, ws.data_ptr(),
                                       _stream_handle(stream))
    abi.check(rc, "spz_amd_decimate_device")
    if stream is not None:
        ws.record_stream(stream)
    hdr = make_header(m, header.sh_degree, 3, header.fractional_bits, bool(header.flags & 1))
    return out, hdr, parents


def _check_tile_args(stream_t, header, max_points, max_tiles):
    if isinstance(max_points, bool) or not isinstance(max_points, int) or not 1 <= max_points <= abi.REFERENCE_MAX_POINTS:
        raise ValueError(f"max_points must be an int in 1..{abi.REFERENCE_MAX_POINTS}, got {max_points!r}")
    if isinstance(max_tiles, bool) or not isinstance(max_tiles, int) or not 1 <= max_tiles <= 2 ** 31 - 1:
        raise ValueError(f"max_tiles must be an int in 1..2^31 - 1, got {max_tiles!r}")
    _check_decimate_stream(stream_t, header)
    if header.num_points > abi.REFERENCE_MAX_POINTS:
        raise ValueError(f"{header.num_points} points is above the reader limit {abi.REFERENCE_MAX_POINTS}")


def tile_table_numpy(table_t, count):
    """The first `count` rows of a device tile table as a numpy structured array (abi.TileInfo's fields)."""
    import numpy as np
    raw = table_t[:count].cpu().numpy().reshape(-1)
    return np.frombuffer(raw.tobytes(), dtype=np.dtype(abi.TileInfo), count=count)


def _tile_tree_on(L, stream_t, header, max_points, max_tiles, st):
    """tile_tree's allocations, fills and launches, all on the current stream `st`."""
    n, dev = header.num_points, stream_t.device
    rows = min(max_tiles, max(1, 2 * n - 1))
    table = torch.zeros((rows, C.sizeof(abi.TileInfo)), dtype=torch.uint8, device=dev)
    summary = torch.zeros(C.sizeof(abi.TileSummary), dtype=torch.uint8, device=dev)
    ws = torch.empty(int(L.spz_amd_tile_workspace_bytes(n, header.sh_degree, max_tiles)), dtype=torch.uint8, device=dev)
    rc = L.spz_amd_tile_tree_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), max_points, max_tiles,
                                    table.data_ptr(), summary.data_ptr(), ws.data_ptr(), C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_tile_tree_device")
    return table, summary


def tile_tree(stream_t, header, max_points, max_tiles=abi.TILE_DEFAULT_MAX_TILES, stream=None):
    """The octree of LOD tiles of a packed v2/v3 device stream (spz_amd_tile_tree_device; the contract is in
    include/spz_amd.h, "tile").  Returns (table, summary): a uint8 CUDA tensor of (rows, 104) tile rows and one of
    sizeof(abi.TileSummary) bytes.  Nothing is read back: the tile count is in the summary (tile_summary reads it), and
    the rows are written only when it is at most max_tiles.  Interior boxes are NaN until tile_packed fills them.
    Every allocation, fill and launch is enqueued on `stream` (after the current stream's work), or the current one."""
    L = abi.load_library()
    _check_tile_args(stream_t, header, max_points, max_tiles)
    dev = stream_t.device
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            return _tile_tree_on(L, stream_t, header, max_points, max_tiles, st)


def tile_summary(summary_t):
    """The summary of tile_tree on the host (an abi.TileSummary; one small read-back on the current stream)."""
    return abi.TileSummary.from_buffer_copy(summary_t.cpu().numpy().tobytes())


def tile_packed(stream_t, header, max_points, max_tiles=abi.TILE_DEFAULT_MAX_TILES, stream=None):
    """The tileset of a packed v2/v3 device stream, all in device memory: tile_tree, one read-back of the summary and
    the table, then per distinct content level one decimate_packed and one spz_amd_tile_content_device (bounds + the
    batched emit), then the leaves' from the sorted stream.  Returns (table: numpy structured array of the finished
    rows, tiles: a list of uint8 CUDA tensors, views of `arena`, one stream per tile in id order, arena).  More than
    max_tiles tiles raises abi.SpzAmdError(SPZ_AMD_ERR_CAPACITY) before any content is produced.  Everything is
    enqueued on `stream` (after the current stream's work), or the current one; the call waits for it."""
    L = abi.load_library()
    _check_tile_args(stream_t, header, max_points, max_tiles)
    dev = stream_t.device
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            table_t, summary_t = _tile_tree_on(L, stream_t, header, max_points, max_tiles, st)
            s = tile_summary(summary_t)
            if not s.ok:
                raise abi.SpzAmdError(abi.ERR_CAPACITY, f"tile_packed: {s.num_tiles} tiles, max_tiles {max_tiles}")
            count = int(s.num_tiles)
            rows = tile_table_numpy(table_t, count)
            arena = torch.zeros(int(s.arena_bytes), dtype=torch.uint8, device=dev)
            ws = torch.empty(int(L.spz_amd_tile_content_workspace_bytes(count)), dtype=torch.uint8, device=dev)
            for level in sorted(set(int(l) for l in rows["content_level"])):
                if level >= 0:
                    source = decimate_packed(stream_t, header, level)[0]
                elif header.num_points:
                    source = subset(stream_t, header, morton_order(stream_t, header))
                else:
                    source = stream_t
                rc = L.spz_amd_tile_content_device(table_t.data_ptr(), count, level, source.data_ptr(), source.numel(),
                                                   arena.data_ptr(), arena.numel(), ws.data_ptr(),
                                                   C.c_void_p(st.cuda_stream))
                abi.check(rc, "spz_amd_tile_content_device")
            rows = tile_table_numpy(table_t, count)   # a blocking copy on st: everything above is done
            st.synchronize()
    tiles = [arena[int(r["offset"]):int(r["offset"]) + int(r["bytes"])] for r in rows]
    return rows, tiles, arena


def _check_clean_stream(stream_t, header):
    _check_stream_tensor(stream_t)
    if header.version == 1:
        raise ValueError("a version 1 stream has float16 positions and no integer distances (transform_packed writes a "
                         "v3 copy)")
    if header.num_points > abi.REFERENCE_MAX_POINTS:
        raise ValueError(f"{header.num_points} points is above the reader limit {abi.REFERENCE_MAX_POINTS}")


def knn_scores(stream_t, header, k, stream=None):
    """The statistical outlier scores of a packed v2/v3 device stream (spz_amd_knn_scores_device; the contract is in
    include/spz_amd.h "clean"): for every point in input order, the mean distance to its k_eff = min(k, n - 1) nearest
    other points in world units (float64 CUDA tensor), and the k_eff-th squared distance in stored quanta (int64 CUDA
    tensor).  Exact: the scores equal a brute-force k-NN over the stored integers bit for bit."""
    L = abi.load_library()
    _check_clean_stream(stream_t, header)
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= 64:
        raise ValueError(f"k must be an int in 1..64, got {k!r}")
    n, dev = header.num_points, stream_t.device
    scores = torch.empty(n, dtype=torch.float64, device=dev)
    kth = torch.empty(n, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.spz_amd_clean_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.spz_amd_knn_scores_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), k,
                                         scores.data_ptr(), kth.data_ptr(), ws.data_ptr(), _stream_handle(stream))
    abi.check(rc, "spz_amd_knn_scores_device")
    if stream is not None:  # the workspace was allocated on the current stream; the launches use it on `stream`
        ws.record_stream(stream)
    return scores, kth


def radius_counts(stream_t, header, radius, min_neighbors, stream=None):
    """The radius-rule counts of a packed v2/v3 device stream (spz_amd_radius_counts_device): for every point in input
    order, the number of other points within `radius` (world units, > 0), saturated at min_neighbors (1..256); int32
    CUDA tensor.  counts >= min_neighbors is the keep mask of the radius rule."""
    L = abi.load_library()
    _check_clean_stream(stream_t, header)
    if isinstance(radius, bool) or not isinstance(radius, (int, float)) or not math.isfinite(radius) or not radius > 0:
        raise ValueError(f"radius must be a finite number > 0, got {radius!r}")
    if isinstance(min_neighbors, bool) or not isinstance(min_neighbors, int) or not 1 <= min_neighbors <= 256:
        raise ValueError(f"min_neighbors must be an int in 1..256, got {min_neighbors!r}")
    r2 = C.c_uint64(0)
    abi.check(L.spz_amd_clean_radius_r2(float(radius), header.fractional_bits, C.byref(r2)), "spz_amd_clean_radius_r2")
    n, dev = header.num_points, stream_t.device
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    ws = torch.empty(int(L.spz_amd_clean_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.spz_amd_radius_counts_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), r2.value,
                                            min_neighbors, counts.data_ptr(), ws.data_ptr(), _stream_handle(stream))
    abi.check(rc, "spz_amd_radius_counts_device")
    if stream is not None:
        ws.record_stream(stream)
    return counts


def _align_pair(source_t, source_hdr, target_t, target_hdr):
    _check_clean_stream(source_t, source_hdr)
    _check_clean_stream(target_t, target_hdr)
    if source_t.device != target_t.device:
        raise ValueError("the source and the target are on different devices")
    if target_hdr.num_points == 0:
        raise ValueError("the target has no points")
    return (abi.AlignCloud(source_t.data_ptr(), source_t.numel(), source_hdr),
            abi.AlignCloud(target_t.data_ptr(), target_t.numel(), target_hdr))


def _align_map(map):
    m = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0] if map is None else [float(v) for v in map]
    if len(m) != 12 or not all(math.isfinite(v) for v in m):
        raise ValueError("map must be twelve finite numbers: M = s R row-major, then t")
    return (C.c_double * 12)(*m)


def _align_stride(stride):
    if isinstance(stride, bool) or not isinstance(stride, int) or stride < 1:
        raise ValueError(f"stride must be an int >= 1, got {stride!r}")
    return stride


def _align_r2(max_distance, fractional_bits):
    if max_distance is None:
        return abi.NO_LIMIT_R2
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float)) or \
            not math.isfinite(max_distance) or not max_distance > 0:
        raise ValueError(f"max_distance must be None or a finite number > 0, got {max_distance!r}")
    r2 = C.c_uint64(0)
    abi.check(abi.load_library().spz_amd_clean_radius_r2(float(max_distance), fractional_bits, C.byref(r2)),
              "spz_amd_clean_radius_r2")
    return r2.value


def nearest_packed(source_t, source_hdr, target_t, target_hdr, map=None, stride=1, max_distance=None, stream=None):
    """The nearest target point of every source point of two packed v2/v3 device streams under a map (twelve floats:
    M = s R row-major, then t, in the stored RUB frame; None: the identity), exact on the stored integers (include/
    spz_amd.h "align", steps 1-3): (index, d2), an int64 and a uint64-valued int64 CUDA tensor in source input order.
    index is -1 (and d2 -1) for points not taking part (i % stride != 0), mapped to a non-finite place, or without a
    target point within max_distance (world units)."""
    L = abi.load_library()
    src, tgt = _align_pair(source_t, source_hdr, target_t, target_hdr)
    m = _align_map(map)
    stride = _align_stride(stride)
    r2 = _align_r2(max_distance, target_hdr.fractional_bits)
    ns, dev = source_hdr.num_points, source_t.device
    index = torch.empty(ns, dtype=torch.int32, device=dev)
    d2 = torch.empty(ns, dtype=torch.int64, device=dev)
    ws = torch.empty(int(L.spz_amd_align_workspace_bytes(ns, target_hdr.num_points)), dtype=torch.uint8, device=dev)
    st = _stream_handle(stream)
    with torch.cuda.device(dev):
        abi.check(L.spz_amd_align_prepare_device(C.byref(src), C.byref(tgt), ws.data_ptr(), st),
                  "spz_amd_align_prepare_device")
        abi.check(L.spz_amd_nearest_device(C.byref(src), C.byref(tgt), stride, m, r2, index.data_ptr(), d2.data_ptr(),
                                           ws.data_ptr(), st), "spz_amd_nearest_device")
    if stream is not None:
        ws.record_stream(stream)
    return index.to(torch.int64), d2   # 0xFFFFFFFF -> -1, UINT64_MAX -> -1


def align_step_packed(source_t, source_hdr, target_t, target_hdr, map=None, stride=1, max_distance=None, overlap=1.0,
                      stream=None):
    """One step of the alignment (include/spz_amd.h "align", steps 1-5) under a map: (index, d2, inlier mask as a bool
    CUDA tensor, abi.AlignMoments).  Synchronises to read the moments."""
    L = abi.load_library()
    src, tgt = _align_pair(source_t, source_hdr, target_t, target_hdr)
    m = _align_map(map)
    stride = _align_stride(stride)
    r2 = _align_r2(max_distance, target_hdr.fractional_bits)
    if isinstance(overlap, bool) or not isinstance(overlap, (int, float)) or not 0 < overlap <= 1:
        raise ValueError(f"overlap must be in (0, 1], got {overlap!r}")
    ns, dev = source_hdr.num_points, source_t.device
    index = torch.empty(ns, dtype=torch.int32, device=dev)
    d2 = torch.empty(ns, dtype=torch.int64, device=dev)
    inlier = torch.empty(ns, dtype=torch.uint8, device=dev)
    mom_t = torch.empty(C.sizeof(abi.AlignMoments), dtype=torch.uint8, device=dev)
    ws = torch.empty(int(L.spz_amd_align_workspace_bytes(ns, target_hdr.num_points)), dtype=torch.uint8, device=dev)
    st = _stream_handle(stream)
    with torch.cuda.device(dev):
        abi.check(L.spz_amd_align_prepare_device(C.byref(src), C.byref(tgt), ws.data_ptr(), st),
                  "spz_amd_align_prepare_device")
        abi.check(L.spz_amd_align_step_device(C.byref(src), C.byref(tgt), stride, m, r2, float(overlap),
                                              index.data_ptr(), d2.data_ptr(), inlier.data_ptr(), mom_t.data_ptr(),
                                              ws.data_ptr(), st), "spz_amd_align_step_device")
        (stream or torch.cuda.current_stream(dev)).synchronize()
    mom = abi.AlignMoments.from_buffer_copy(mom_t.cpu().numpy().tobytes())
    return index.to(torch.int64), d2, inlier.bool(), mom


def align_packed(source_t, source_hdr, target_t, target_hdr, *, rotation=None, translation=None, scale=1.0, coord=0,
                 estimate_scale=False, overlap=1.0, max_distance=None, stride=1, max_iterations=30,
                 relative_fitness=1e-6, relative_rmse=1e-6, init_centroids=False):
    """The similarity that places the source stream on the target stream (spz_amd_align_host; include/spz_amd.h
    "align"): a dict with rotation (x, y, z, w), translation and scale stated in `coord` (ready for transform_packed or
    a merge placement), map (twelve floats, stored frame), fitness, inlier_rmse, inliers, iterations, converged,
    degenerate, history (a list of (fitness, inlier_rmse, inliers) per step) and ms (prepare, queries, the rest).
    Blocking; runs on a stream of its own."""
    L = abi.load_library()
    src, tgt = _align_pair(source_t, source_hdr, target_t, target_hdr)
    o = abi.AlignOptions()
    abi.check(L.spz_amd_align_default_options(C.byref(o)), "spz_amd_align_default_options")
    if rotation is not None:
        rotation = [float(v) for v in rotation]
        if len(rotation) != 4:
            raise ValueError("rotation must be (x, y, z, w)")
        o.rotation[:] = rotation
    if translation is not None:
        translation = [float(v) for v in translation]
        if len(translation) != 3:
            raise ValueError("translation must be (x, y, z)")
        o.translation[:] = translation
    for name, v in (("stride", stride), ("max_iterations", max_iterations)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 32:
            raise ValueError(f"{name} must be a non-negative int, got {v!r}")
    o.scale = float(scale)
    o.coord = int(coord)
    o.estimate_scale = 1 if estimate_scale else 0
    o.overlap = float(overlap)
    o.has_max_distance = 0 if max_distance is None else 1
    o.max_distance = 0.0 if max_distance is None else float(max_distance)
    o.stride = stride
    o.max_iterations = max_iterations
    o.init_centroids = 1 if init_centroids else 0
    o.relative_fitness = float(relative_fitness)
    o.relative_rmse = float(relative_rmse)
    if L.spz_amd_align_check(C.byref(o)) != abi.OK:
        raise ValueError("invalid align options: stride >= 1, overlap in (0, 1], max_distance > 0, max_iterations "
                         "1..1000, tolerances >= 0, a nonzero rotation, scale > 0, coord 0..8, all finite")
    res = abi.AlignResult()
    hist = (abi.AlignHistory * max_iterations)()
    ms = (C.c_float * 3)()
    dev = source_t.device
    torch.cuda.current_stream(dev).synchronize()   # the streams' producers: the run uses a stream of its own
    rc = L.spz_amd_align_host(C.byref(src), C.byref(tgt), C.byref(o), dev.index or 0, C.byref(res), hist,
                              max_iterations, ms)
    abi.check(rc, "spz_amd_align_host")
    return dict(rotation=tuple(res.rotation), translation=tuple(res.translation), scale=res.scale, map=tuple(res.map),
                fitness=res.fitness, inlier_rmse=res.inlier_rmse, inliers=int(res.inliers),
                iterations=int(res.iterations), converged=bool(res.converged), degenerate=bool(res.degenerate),
                history=[(h.fitness, h.inlier_rmse, int(h.inliers)) for h in hist[:res.iterations]],
                ms=tuple(ms))


def plane_threshold(threshold, fractional_bits):
    """T = floor(threshold 2^(f+16)) of a threshold in world units (spz_amd_plane_threshold); ValueError outside
    [0, 2^36]."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
        raise ValueError(f"threshold must be a finite number >= 0, got {threshold!r}")
    T = C.c_uint64(0)
    if abi.load_library().spz_amd_plane_threshold(float(threshold), int(fractional_bits), C.byref(T)) != abi.OK:
        raise ValueError(f"threshold must be a finite number >= 0 with floor(threshold 2^(f+16)) <= 2^36, got {threshold!r}")
    return T.value


def _plane_T(header, threshold, T):
    if (threshold is None) == (T is None):
        raise ValueError("give exactly one of threshold (world units) and T (the integer threshold)")
    if T is None:
        return plane_threshold(threshold, header.fractional_bits)
    if isinstance(T, bool) or not isinstance(T, int) or not 0 <= T <= 1 << 36:
        raise ValueError(f"T must be an int in 0..2^36, got {T!r}")
    return T


def _plane_struct(plane):
    p = [int(v) for v in plane]
    if len(p) != 4 or any(abs(v) > 65536 for v in p[:3]) or abs(p[3]) > 1 << 42 or not any(p[:3]):
        raise ValueError("plane must be (a, b, c, e): a, b, c in [-2^16, 2^16] and not all zero, |e| <= 2^42")
    return abi.Plane(p[0], p[1], p[2], 0, p[3])


def plane_prepare(stream_t, header, stride=1, labels=None, stream=None):
    """The taking-part points of a packed v2/v3 device stream (include/spz_amd.h "plane", step 1: i % stride == 0 and
    labels[i] == 0; labels: None or a uint8 CUDA tensor of num_points), compacted into a workspace: (workspace, m).
    Blocks until the count m is known.  The workspace serves plane_gather and the prepared= argument of plane_score,
    plane_moments and plane_mark."""
    L = abi.load_library()
    _check_clean_stream(stream_t, header)
    stride = _align_stride(stride)
    n, dev = header.num_points, stream_t.device
    if labels is not None and (labels.dtype != torch.uint8 or labels.numel() != n or labels.device != dev
                               or not labels.is_contiguous()):
        raise ValueError("labels must be a contiguous uint8 tensor of num_points on the stream's device")
    ws = torch.empty(int(L.spz_amd_plane_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    m = C.c_uint64(0)
    with torch.cuda.device(dev):
        rc = L.spz_amd_plane_prepare_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header), stride,
                                            labels.data_ptr() if labels is not None else None, ws.data_ptr(),
                                            C.byref(m), _stream_handle(stream))
    abi.check(rc, "spz_amd_plane_prepare_device")
    if stream is not None:
        ws.record_stream(stream)
    return ws, int(m.value)


def plane_gather(prepared, header, indices, stream=None):
    """Prepared points by their place among the prepared ones: an int32 (k, 3) CUDA tensor of the stored integers."""
    L = abi.load_library()
    ws, m = prepared
    idx = torch.as_tensor(indices, dtype=torch.int64, device=ws.device).reshape(-1)
    if m == 0 or (idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= m)):
        raise ValueError("an index is out of range for the prepared points")
    idx32 = idx.to(torch.int32)   # m < 2^31
    out = torch.empty((idx.numel(), 3), dtype=torch.int32, device=ws.device)
    with torch.cuda.device(ws.device):
        rc = L.spz_amd_plane_gather_device(ws.data_ptr(), header.num_points, m, idx32.data_ptr(), idx.numel(),
                                           out.data_ptr(), _stream_handle(stream))
    abi.check(rc, "spz_amd_plane_gather_device")
    return out


def plane_score(stream_t, header, planes, threshold=None, T=None, stride=1, labels=None, prepared=None, stream=None):
    """The MSAC score of H planes over the taking-part points (include/spz_amd.h "plane", step 3).  planes: an (H, 4)
    integer array of (a, b, c, e); a plane with a = b = c = 0, or out of range, is invalid.  Returns (K, S, cost), int64
    CUDA tensors of H; an invalid plane has K = S = 0 and cost -1 (UINT64_MAX)."""
    L = abi.load_library()
    T = _plane_T(header, threshold, T)
    ws, m = prepared if prepared is not None else plane_prepare(stream_t, header, stride, labels, stream)
    import numpy as np
    p = np.asarray(planes, dtype=np.int64).reshape(-1, 4)
    H = p.shape[0]
    if not 1 <= H <= 65536:
        raise ValueError("between 1 and 65536 planes")
    if np.any(np.abs(p[:, :3]) >= 1 << 31):
        raise ValueError("a, b, c must fit 32 bits")
    rec = np.zeros(H, dtype=[("a", "<i4"), ("b", "<i4"), ("c", "<i4"), ("r", "<i4"), ("e", "<i8")])
    rec["a"], rec["b"], rec["c"], rec["e"] = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    dev = ws.device
    planes_t = torch.from_numpy(rec.view(np.uint8).copy()).to(dev)
    scores = torch.empty((H, 3), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        rc = L.spz_amd_plane_score_device(ws.data_ptr(), header.num_points, m, planes_t.data_ptr(), H, T,
                                          scores.data_ptr(), _stream_handle(stream))
    abi.check(rc, "spz_amd_plane_score_device")
    if stream is not None:
        planes_t.record_stream(stream)
    return scores[:, 0].contiguous(), scores[:, 1].contiguous(), scores[:, 2].contiguous()


def plane_moments(stream_t, header, plane, threshold=None, T=None, stride=1, labels=None, prepared=None, stream=None):
    """The exact moments of one plane (a, b, c, e) over the taking-part points (include/spz_amd.h "plane", step 5): a
    dict of Python ints: count, sum_abs, above, below, points, sum_p (3) and sum_pp (6: XX, XY, XZ, YY, YZ, ZZ), and
    `struct`, the abi.PlaneMoments for spz_amd_plane_solve.  Synchronises to read them."""
    L = abi.load_library()
    T = _plane_T(header, threshold, T)
    q = _plane_struct(plane)
    ws, m = prepared if prepared is not None else plane_prepare(stream_t, header, stride, labels, stream)
    dev = ws.device
    mom_t = torch.empty(C.sizeof(abi.PlaneMoments), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.spz_amd_plane_moments_device(ws.data_ptr(), header.num_points, m, C.byref(q), T, mom_t.data_ptr(),
                                            _stream_handle(stream))
        abi.check(rc, "spz_amd_plane_moments_device")
        (stream or torch.cuda.current_stream(dev)).synchronize()
    mo = abi.PlaneMoments.from_buffer_copy(mom_t.cpu().numpy().tobytes())
    return dict(count=int(mo.count), sum_abs=int(mo.sum_abs), above=int(mo.above), below=int(mo.below),
                points=int(mo.points), sum_p=[int(v) for v in mo.sum_p],
                sum_pp=[(int(h) << 64) + int(l) for l, h in zip(mo.sum_pp_lo, mo.sum_pp_hi)], struct=mo)


def plane_mark(stream_t, header, plane, value, labels_out, threshold=None, T=None, stride=1, labels=None,
               prepared=None, stream=None):
    """labels_out[i] = value (1..255) for the inliers of one plane among the taking-part points, in place
    (spz_amd_plane_mark_device); every other entry keeps its value.  Returns labels_out."""
    L = abi.load_library()
    T = _plane_T(header, threshold, T)
    q = _plane_struct(plane)
    if isinstance(value, bool) or not isinstance(value, int) or not 0 <= value <= 255:
        raise ValueError(f"value must be an int in 0..255, got {value!r}")
    ws, m = prepared if prepared is not None else plane_prepare(stream_t, header, stride, labels, stream)
    if labels_out.dtype != torch.uint8 or labels_out.numel() != header.num_points or labels_out.device != ws.device \
            or not labels_out.is_contiguous():
        raise ValueError("labels_out must be a contiguous uint8 tensor of num_points on the stream's device")
    with torch.cuda.device(ws.device):
        rc = L.spz_amd_plane_mark_device(ws.data_ptr(), header.num_points, m, C.byref(q), T, value,
                                         labels_out.data_ptr(), _stream_handle(stream))
    abi.check(rc, "spz_amd_plane_mark_device")
    return labels_out


def detect_planes_packed(stream_t, header, *, threshold, hypotheses=4096, seed=0, stride=1, refine=3, planes=1,
                         min_inliers=0, axis=None, max_tilt=None, up_hint=None, coord=0, no_translate=False):
    """The dominant planes of a packed v2/v3 device stream (spz_amd_plane_host; include/spz_amd.h "plane"): a dict with
    planes (a list of dicts: integers (a, b, c, e), inliers, sum_abs, points, above, below, best_hypothesis,
    refinements, fitness, mean_distance, normal, offset, rotation (x, y, z, w), translation, scale: the levelling
    placement in `coord`), labels (a uint8 CUDA tensor: 0 or the 1-based plane of each point), threshold (T) and ms
    (prepare, score, refine).  min_inliers: an int count, or a float fraction of the points taking part.  Blocking; runs
    on a stream of its own."""
    L = abi.load_library()
    _check_clean_stream(stream_t, header)
    o = abi.PlaneOptions()
    abi.check(L.spz_amd_plane_default_options(C.byref(o)), "spz_amd_plane_default_options")
    for name, v in (("hypotheses", hypotheses), ("stride", stride), ("refine", refine), ("planes", planes)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 2 ** 32:
            raise ValueError(f"{name} must be a non-negative int, got {v!r}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be an int in 0..2^64 - 1, got {seed!r}")
    T = plane_threshold(threshold, header.fractional_bits)
    o.threshold = float(threshold)
    o.hypotheses, o.stride, o.refine, o.max_planes, o.seed = hypotheses, stride, refine, planes, seed
    if isinstance(min_inliers, bool) or not isinstance(min_inliers, (int, float)) or min_inliers < 0:
        raise ValueError("min_inliers must be an int >= 0 (a count) or a float in [0, 1] (a fraction)")
    if isinstance(min_inliers, float):
        if not min_inliers <= 1.0:
            raise ValueError("min_inliers must be an int >= 0 (a count) or a float in [0, 1] (a fraction)")
        taking = (header.num_points + max(stride, 1) - 1) // max(stride, 1)
        o.min_inliers = math.ceil(min_inliers * float(taking))
    else:
        o.min_inliers = min_inliers
    if (axis is None) != (max_tilt is None):
        raise ValueError("give axis and max_tilt together")
    for name, v, has in (("axis", axis, "has_axis"), ("up_hint", up_hint, "has_up_hint")):
        if v is not None:
            v = [float(t) for t in v]
            if len(v) != 3:
                raise ValueError(f"{name} must be (x, y, z)")
            getattr(o, name)[:] = v
            setattr(o, has, 1)
    if max_tilt is not None:
        o.max_tilt = float(max_tilt)
    o.coord = int(coord)
    o.no_translate = 1 if no_translate else 0
    if L.spz_amd_plane_check(C.byref(o)) != abi.OK:
        raise ValueError("invalid plane options: threshold >= 0, hypotheses 1..65536, refine 0..16, planes 1..255, "
                         "stride >= 1, a nonzero axis and up_hint, max_tilt 0..90, coord 0..8, all finite")
    import numpy as np
    res = (abi.PlaneResult * planes)()
    found = C.c_uint32(0)
    ms = (C.c_float * 3)()
    labels = np.zeros(header.num_points, np.uint8)
    dev = stream_t.device
    torch.cuda.current_stream(dev).synchronize()   # the stream's producers: the run uses a stream of its own
    rc = L.spz_amd_plane_host(stream_t.data_ptr(), stream_t.numel(), C.byref(header), C.byref(o), dev.index or 0, res,
                              planes, C.byref(found), labels.ctypes.data, ms)
    abi.check(rc, "spz_amd_plane_host")
    out = []
    for r in res[:found.value]:
        out.append(dict(integers=(r.plane.a, r.plane.b, r.plane.c, r.plane.e), inliers=int(r.inliers),
                        sum_abs=int(r.sum_abs), points=int(r.points), above=int(r.above), below=int(r.below),
                        best_hypothesis=int(r.best_hypothesis), refinements=int(r.refinements), fitness=r.fitness,
                        mean_distance=r.mean_distance, normal=tuple(r.normal), offset=r.offset,
                        rotation=tuple(r.rotation), translation=tuple(r.translation), scale=r.scale))
    return dict(planes=out, labels=torch.from_numpy(labels).to(dev), threshold=T, ms=tuple(ms))


def _cloud_render_args(cloud, num_points, sh_degree):
    if int(sh_degree) not in SH_DIM:
        raise ValueError(f"sh_degree must be 0..3, got {sh_degree}")
    dev = cloud["positions"].device
    return _ptrs(cloud, sh_degree, num_points, dev), dev


def _cloud_source(cloud, num_points, sh_degree, antialiased):
    """The float source of _render_prepare for a cloud, with its pointers and its device: (source, ptrs, dev)."""
    ptrs, dev = _cloud_render_args(cloud, num_points, sh_degree)
    return ("cloud", ptrs, num_points, int(sh_degree), antialiased), ptrs, dev


def _render_prepare(L, source, params, total, records, ws, st):
    """Enqueue the prepare step of a packed ("packed", stream_t, header) or float ("cloud", ptrs, n, sh_degree,
    antialiased) source into ws on the torch stream st."""
    rec = records.data_ptr() if records is not None else None
    if source[0] == "packed":
        _, stream_t, header = source
        rc = L.spz_amd_render_prepare_packed_device(stream_t.data_ptr(), stream_t.numel(), C.byref(header),
                                                    C.byref(params), total.data_ptr(), rec, ws.data_ptr(),
                                                    C.c_void_p(st.cuda_stream))
    else:
        _, ptrs, n, sh_degree, aa = source
        rc = L.spz_amd_render_prepare_cloud_device(C.byref(ptrs), n, sh_degree, 1 if aa else 0, C.byref(params),
                                                   total.data_ptr(), rec, ws.data_ptr(), C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_render_prepare")


def _on_stream(dev, stream):
    """The stream the render runs on: `stream`, made to wait for the current stream first (which produced the inputs),
    or the current stream.  Every allocation, copy, launch and read-back of a render is enqueued on it."""
    cur = torch.cuda.current_stream(dev)
    if stream is None or stream == cur:
        return cur
    stream.wait_stream(cur)
    return stream


def _aligned_view(t, nbytes):
    """The nbytes of uint8 tensor t from its first 256-aligned byte: where the C ABI puts the workspace's base."""
    off = (-t.data_ptr()) % 256
    return t[off: off + nbytes]


def _check_render_args(L, params, max_entries):
    if not isinstance(params, abi.RenderParams):
        raise ValueError("params must be an abi.RenderParams (abi.render_params)")
    abi.check(L.spz_amd_render_check_params(C.byref(params)), "spz_amd_render_check_params")
    if max_entries is not None and (isinstance(max_entries, bool) or not isinstance(max_entries, int)
                                    or not 0 <= max_entries <= 0x7fffffff):
        raise ValueError(f"max_entries must be an int in 0..2^31-1, got {max_entries!r}")


def _prepared_workspace(L, source, n, params, dev, max_entries, total, st):
    """Enqueue the prepare step on st and return (workspace, m): the workspace holds the prepare part and has room for m
    entries, m = max_entries or, when that is None, the total read back."""
    if max_entries is None:
        # the prepare step writes only the first workspace_bytes(n, 0) - 256 bytes from the workspace's aligned
        # base: prepare, read the total, then move that prefix to the front of a workspace with room for the
        # entries
        ws0_bytes = int(L.spz_amd_render_workspace_bytes(n, 0))
        ws0 = torch.empty(ws0_bytes, dtype=torch.uint8, device=dev)
        _render_prepare(L, source, params, total, None, ws0, st)
        m = int(total.cpu()[0])  # on st: waits for the prepare step
        if m > 0x7fffffff:
            raise RuntimeError(f"{m} tile entries is above the sort's limit of 2^31 - 1")
        ws = torch.empty(int(L.spz_amd_render_workspace_bytes(n, m)), dtype=torch.uint8, device=dev)
        prefix = ws0_bytes - 256
        _aligned_view(ws, prefix).copy_(_aligned_view(ws0, prefix))
    else:
        m = max_entries
        ws = torch.empty(int(L.spz_amd_render_workspace_bytes(n, m)), dtype=torch.uint8, device=dev)
        _render_prepare(L, source, params, total, None, ws, st)
    return ws, m


def _check_out(name, t, shape, dtype, dev):
    if t is not None and (t.dtype != dtype or t.device != dev or not t.is_contiguous() or tuple(t.shape) != shape):
        raise ValueError(f"{name} must be a contiguous {str(dtype).split('.')[-1]} tensor of shape {shape} on {dev}")


def _prepare_finish(L, source, n, params, dev, max_entries, st, image, depth=None, index=None):
    """Prepare + finish on st into the given tensors, keeping the workspace: (total, status, workspace, m).  With a
    depth map the finish step is spz_amd_render_depth_device (image and index may then be None), without one
    spz_amd_render_finish_device."""
    # the prepare step always writes the total, the finish step always writes the status
    total = torch.empty(1, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws, m = _prepared_workspace(L, source, n, params, dev, max_entries, total, st)
    tail = (status.data_ptr(), ws.data_ptr(), C.c_void_p(st.cuda_stream))
    if depth is None:
        rc = L.spz_amd_render_finish_device(n, C.byref(params), m, image.data_ptr(), *tail)
        abi.check(rc, "spz_amd_render_finish_device")
    else:
        rc = L.spz_amd_render_depth_device(n, C.byref(params), m, image.data_ptr() if image is not None else None,
                                           depth.data_ptr(), index.data_ptr() if index is not None else None, *tail)
        abi.check(rc, "spz_amd_render_depth_device")
    return total, status, ws, m


def _render(source, n, params, dev, max_entries, out, return_info, stream):
    L = abi.load_library()
    _check_render_args(L, params, max_entries)
    h, w = params.height, params.width
    if out is not None and (out.dtype != torch.float32 or out.device != dev or not out.is_contiguous()
                            or tuple(out.shape) != (h, w, 4)):
        raise ValueError(f"out must be a contiguous float32 tensor of shape ({h}, {w}, 4) on {dev}")
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            if out is None:
                out = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
            total, status, _, _ = _prepare_finish(L, source, n, params, dev, max_entries, st, out)
    return (out, total, status) if return_info else out


def _render_depth(source, n, params, dev, max_entries, return_image, return_index, out, return_info, stream):
    L = abi.load_library()
    _check_render_args(L, params, max_entries)
    h, w = params.height, params.width
    out = dict(out or {})
    if set(out) - {"depth", "index", "image"}:
        raise ValueError("out may hold depth, index and image")
    _check_out("out['depth']", out.get("depth"), (h, w, 2), torch.float32, dev)
    _check_out("out['index']", out.get("index"), (h, w), torch.int32, dev)
    _check_out("out['image']", out.get("image"), (h, w, 4), torch.float32, dev)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            depth = out.get("depth")
            if depth is None:
                depth = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
            index = out.get("index")
            if index is None and return_index:
                index = torch.empty((h, w), dtype=torch.int32, device=dev)
            image = out.get("image")
            if image is None and return_image:
                image = torch.empty((h, w, 4), dtype=torch.float32, device=dev)
            total, status, _, _ = _prepare_finish(L, source, n, params, dev, max_entries, st, image, depth, index)
    res = (depth,)
    if index is not None:
        res += (index,)
    if image is not None:
        res += (image,)
    if return_info:
        res += (total, status)
    return res[0] if len(res) == 1 else res


def render(cloud, num_points, sh_degree, params, antialiased=False, max_entries=None, out=None, return_info=False,
           stream=None):
    """The image of a float cloud on the device (spz_amd_render_prepare_cloud_device + finish; the contract is in
    include/spz_amd.h "render"): a (height, width, 4) float32 CUDA tensor, RGB + alpha.  cloud: device tensors keyed like
    the GaussianCloud fields, already in the frame of the camera `params` (abi.render_params; its coord is ignored).
    max_entries None: the prepare step's total sizes the workspace (one value is read back); an int: the workspace is
    sized for it, and when the total is above it nothing is written to the image and the status word is 1.
    return_info: (image, total (int64 tensor [1]), status (int32 tensor [1])).  stream: a torch stream that first waits
    for the current one, then takes every allocation, copy, launch and read-back of the render; the results belong to it
    (synchronise with it before using them on another stream)."""
    source, _, dev = _cloud_source(cloud, num_points, sh_degree, antialiased)
    return _render(source, num_points, params, dev, max_entries, out, return_info, stream)


def _rendered_workspace(L, source, n, params, dev, max_entries, st, depth=False):
    """Prepare + finish on st, keeping the workspace: (image, workspace, m), or with depth, where the finish step is
    spz_amd_render_depth_device, (image, depth, workspace, m).  Raises when the total is above max_entries (one word is
    read back)."""
    h, w = params.height, params.width
    maps = [torch.empty((h, w, 4), dtype=torch.float32, device=dev)]
    if depth:
        maps.append(torch.empty((h, w, 2), dtype=torch.float32, device=dev))
    total, status, ws, m = _prepare_finish(L, source, n, params, dev, max_entries, st, *maps)
    if max_entries is not None and int(status.cpu()[0]) != 0:  # on st: waits for the finish step
        raise RuntimeError(f"{int(total.cpu()[0])} tile entries is above max_entries = {max_entries}")
    return (*maps, ws, m)


def _render_backward(L, ptrs, n, sh_degree, antialiased, params, m, image, grad_image, grad_depth, ws, dev,
                     want_records, st):
    """Enqueue the backward on st over the workspace ws of a finished or depth render: (grads, record_grads,
    depth_grads).  With grad_depth it is spz_amd_render_depth_backward_device (grad_image may then be None, and image
    is not read), and depth_grads is (n,) when the records are wanted; without, spz_amd_render_backward_device, and
    depth_grads is None."""
    depth = grad_depth is not None
    grads = alloc_cloud(n, sh_degree, dev)
    gp = abi.CloudPtrs(*[grads[k].data_ptr() if grads[k].numel() else None for k in FIELDS])
    rec = torch.empty((n, 9), dtype=torch.float32, device=dev) if want_records else None
    dz = torch.empty(n, dtype=torch.float32, device=dev) if want_records and depth else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws_bytes = L.spz_amd_render_depth_backward_workspace_bytes if depth else L.spz_amd_render_backward_workspace_bytes
    bws = torch.empty(int(ws_bytes(n)), dtype=torch.uint8, device=dev)
    head = (C.byref(ptrs), n, sh_degree, 1 if antialiased else 0, C.byref(params), m)
    rec_ptr = rec.data_ptr() if rec is not None and n else None
    tail = (status.data_ptr(), ws.data_ptr(), bws.data_ptr(), C.c_void_p(st.cuda_stream))
    if depth:
        rc = L.spz_amd_render_depth_backward_device(*head, grad_image.data_ptr() if grad_image is not None else None,
                                                    grad_depth.data_ptr(), C.byref(gp), rec_ptr,
                                                    dz.data_ptr() if dz is not None and n else None, *tail)
        abi.check(rc, "spz_amd_render_depth_backward_device")
    else:
        rc = L.spz_amd_render_backward_device(*head, image.data_ptr(), grad_image.data_ptr(), C.byref(gp), rec_ptr,
                                              *tail)
        abi.check(rc, "spz_amd_render_backward_device")
    return grads, rec, dz


def _check_grad(name, t, shape, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or tuple(t.shape) != shape:
        raise ValueError(f"{name} must be a float32 tensor of shape {shape} on {dev}")
    return t.contiguous()


def _check_grad_image(grad_image, params, dev):
    return _check_grad("grad_image", grad_image, (params.height, params.width, 4), dev)


def _check_grad_depth(grad_depth, params, dev):
    return _check_grad("grad_depth", grad_depth, (params.height, params.width), dev)


def _render_then_backward(cloud, num_points, sh_degree, params, grad_image, grad_depth, depth, antialiased, max_entries,
                          return_record_grads, stream):
    """render_backward() (depth False) and render_depth_backward() (depth True: grad_depth is required and grad_image may
    be None): check, render keeping the workspace, and the backward over it, all on the stream."""
    source, ptrs, dev = _cloud_source(cloud, num_points, sh_degree, antialiased)
    L = abi.load_library()
    _check_render_args(L, params, max_entries)
    if grad_image is not None or not depth:
        grad_image = _check_grad_image(grad_image, params, dev)
    if depth:
        grad_depth = _check_grad_depth(grad_depth, params, dev)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            image, ws, m = _rendered_workspace(L, source, num_points, params, dev, max_entries, st)
            grads, rec, dz = _render_backward(L, ptrs, num_points, int(sh_degree), antialiased, params, m, image,
                                              grad_image, grad_depth, ws, dev, return_record_grads, st)
    if return_record_grads:
        grads["records"] = rec
        if depth:
            grads["depth"] = dz
    return grads


def render_backward(cloud, num_points, sh_degree, params, grad_image, *, antialiased=False, max_entries=None,
                    return_record_grads=False, stream=None):
    """The gradients of a scalar loss to a float cloud, given grad_image = its gradient to the image of render() (a
    (height, width, 4) float32 CUDA tensor): renders (prepare + finish), then spz_amd_render_backward_device over the
    same workspace (include/spz_amd.h "render backward").  Returns a dict of six flat float32 CUDA tensors keyed and
    shaped like the cloud; with return_record_grads also "records", (n, 9): the gradients to each Gaussian's mean 2,
    conic 3, opacity 1 and rgb 3.  Sums with f32 atomic adds: two runs may differ in the last bits.  max_entries: as
    render(), but a total above it raises RuntimeError.  stream: as render()."""
    return _render_then_backward(cloud, num_points, sh_degree, params, grad_image, None, False, antialiased, max_entries,
                                 return_record_grads, stream)


def render_depth_backward(cloud, num_points, sh_degree, params, grad_image, grad_depth, *, antialiased=False,
                          max_entries=None, return_record_grads=False, stream=None):
    """render_backward() with the accumulated depth in it (include/spz_amd.h "render depth backward"): the gradients of
    a scalar loss to a float cloud, given grad_image = its gradient to the image (or None: all zero) and grad_depth =
    its gradient to render_depth()[..., 0], a (height, width) float32 CUDA tensor.  Renders (prepare + finish), then
    spz_amd_render_depth_backward_device over the same workspace.  With return_record_grads also "records", (n, 9), and
    "depth", (n,): the gradient to each Gaussian's record depth z.  Otherwise as render_backward()."""
    return _render_then_backward(cloud, num_points, sh_degree, params, grad_image, grad_depth, True, antialiased,
                                 max_entries, return_record_grads, stream)


def _records_backward(L, n, params, m, grad_image, ws, dev, st):
    """Enqueue spz_amd_render_records_backward_device on st over the workspace ws of a finished render: (n, 9)."""
    rec = torch.empty((n, 9), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    rc = L.spz_amd_render_records_backward_device(n, C.byref(params), m, grad_image.data_ptr(),
                                                  rec.data_ptr() if n else None, status.data_ptr(), ws.data_ptr(),
                                                  C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_render_records_backward_device")
    return rec


def _view_backward(L, ptrs, n, sh_degree, antialiased, params, m, rec, ws, dev, st):
    """Enqueue spz_amd_render_view_backward_device on st: the (3, 4) float64 gradient to [R | t]."""
    out = torch.empty((3, 4), dtype=torch.float64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    vws = torch.empty(int(L.spz_amd_render_view_backward_workspace_bytes(n)), dtype=torch.uint8, device=dev)
    rc = L.spz_amd_render_view_backward_device(C.byref(ptrs), n, sh_degree, 1 if antialiased else 0, C.byref(params), m,
                                               rec.data_ptr() if n else None, out.data_ptr(), status.data_ptr(),
                                               ws.data_ptr(), vws.data_ptr(), C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_render_view_backward_device")
    return out


def render_view_backward(cloud, num_points, sh_degree, params, grad_image, *, antialiased=False, max_entries=None,
                         record_grads=None, return_record_grads=False, stream=None):
    """The gradient of a scalar loss to the camera [R | t] of params, given grad_image = its gradient to the image of
    render(): a (3, 4) float64 CUDA tensor, the 12 entries taken as independent (include/spz_amd.h "render view
    backward").  Renders (prepare + finish), then the blend half of the backward
    (spz_amd_render_records_backward_device) and spz_amd_render_view_backward_device over the same workspace.
    record_grads: an (n, 9) float32 CUDA tensor to use instead of the blend half's (grad_image may then be None): the
    sum over the Gaussians uses no atomics, so the same record gradients give the same bits.  return_record_grads:
    (view_grad, record_grads).  max_entries and stream: as render_backward()."""
    source, ptrs, dev = _cloud_source(cloud, num_points, sh_degree, antialiased)
    L = abi.load_library()
    _check_render_args(L, params, max_entries)
    if record_grads is None:
        grad_image = _check_grad_image(grad_image, params, dev)
    elif (not isinstance(record_grads, torch.Tensor) or record_grads.dtype != torch.float32
          or record_grads.device != dev or tuple(record_grads.shape) != (num_points, 9)):
        raise ValueError(f"record_grads must be a float32 tensor of shape ({num_points}, 9) on {dev}")
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            image, ws, m = _rendered_workspace(L, source, num_points, params, dev, max_entries, st)
            if record_grads is None:
                rec = _records_backward(L, num_points, params, m, grad_image, ws, dev, st)
            else:
                rec = record_grads.contiguous()
            out = _view_backward(L, ptrs, num_points, int(sh_degree), antialiased, params, m, rec, ws, dev, st)
    return (out, rec) if return_record_grads else out


def _params_with_pose(params, world_to_camera):
    """A copy of params with its matrix replaced by the (3, 4) tensor world_to_camera, rounded to float32."""
    if not isinstance(world_to_camera, torch.Tensor) or tuple(world_to_camera.shape) != (3, 4) \
            or not world_to_camera.is_floating_point():
        raise ValueError("world_to_camera must be a floating-point tensor of shape (3, 4)")
    p = abi.RenderParams.from_buffer_copy(params)
    for k, x in enumerate(world_to_camera.detach().to(torch.float32).cpu().reshape(-1).tolist()):
        p.world_to_camera[k] = x
    return p


def _autograd_forward(ctx, num_points, sh_degree, params, antialiased, max_entries, arrays, depth=False):
    """The forward of the three render Functions: check, render on the current stream keeping the workspace (a tensor of
    this call alone, never reused), and leave in ctx.args what the backward needs beside the saved tensors.  Returns
    _rendered_workspace's maps and the workspace: (image, workspace) or, with depth, (image, depth, workspace)."""
    cloud = dict(zip(FIELDS, (a.detach() for a in arrays)))
    source, _, dev = _cloud_source(cloud, num_points, sh_degree, antialiased)
    L = abi.load_library()
    _check_render_args(L, params, max_entries)
    with torch.cuda.device(dev):
        *maps, ws, m = _rendered_workspace(L, source, num_points, params, dev, max_entries,
                                           torch.cuda.current_stream(dev), depth)
    ctx.args = (num_points, int(sh_degree), params, bool(antialiased), m)
    return (*maps, ws)


def _autograd_backward(ctx, mode, image, ws, arrays, grad_image, grad_depth, need, need_pose=False):
    """The backward of the three render Functions on the current stream, over the workspace the forward kept:
    (array_grads, pose_grad).  array_grads: the gradients to the six saved arrays, None where need says so.  mode
    "image": spz_amd_render_backward_device.  mode "depth": spz_amd_render_depth_backward_device, where a grad_image
    of None is all zero, as is a grad_depth of None.  mode "pose": as "image", and with need_pose also the (3, 4)
    float64 gradient to [R | t] from spz_amd_render_view_backward_device (from the blend half alone when no array
    needs a gradient); pose_grad is None otherwise."""
    num_points, sh_degree, params, antialiased, m = ctx.args
    cloud = dict(zip(FIELDS, (a.detach() for a in arrays)))
    ptrs, dev = _cloud_render_args(cloud, num_points, sh_degree)
    L = abi.load_library()
    if grad_image is not None or mode != "depth":
        grad_image = _check_grad_image(grad_image, params, dev)
    if mode == "depth":
        if grad_depth is None:
            grad_depth = torch.zeros((params.height, params.width), dtype=torch.float32, device=dev)
        grad_depth = _check_grad_depth(grad_depth, params, dev)
    need_pose = need_pose and mode == "pose"
    grads, rec, pose = None, None, None
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev)
        if any(need) or mode != "pose":
            grads, rec, _ = _render_backward(L, ptrs, num_points, sh_degree, antialiased, params, m, image, grad_image,
                                             grad_depth, ws, dev, need_pose, st)
        elif need_pose:
            rec = _records_backward(L, num_points, params, m, grad_image, ws, dev, st)
        if need_pose:
            pose = _view_backward(L, ptrs, num_points, sh_degree, antialiased, params, m, rec, ws, dev, st)
    return tuple(grads[k].view_as(a) if n else None for k, a, n in zip(FIELDS, arrays, need)), pose


class _RenderFunction(torch.autograd.Function):
    """render() with a backward: the forward keeps its workspace (a tensor of this call alone, never reused), the
    backward runs spz_amd_render_backward_device over it on the current stream.  The six arrays are saved with
    save_for_backward, so changing one in place before the backward raises torch's usual error."""

    @staticmethod
    def forward(ctx, num_points, sh_degree, params, antialiased, max_entries, *arrays):
        image, ws = _autograd_forward(ctx, num_points, sh_degree, params, antialiased, max_entries, arrays)
        ctx.save_for_backward(image, ws, *arrays)
        return image

    @staticmethod
    def backward(ctx, grad_image):
        image, ws, *arrays = ctx.saved_tensors
        out, _ = _autograd_backward(ctx, "image", image, ws, arrays, grad_image, None, ctx.needs_input_grad[5:])
        return (None,) * 5 + out


class _RenderDepthFunction(torch.autograd.Function):
    """_RenderFunction with two outputs, the image and channel 0 of the depth map: the forward is render_depth_device
    (its image is render()'s, bit for bit), the backward spz_amd_render_depth_backward_device over the kept workspace."""

    @staticmethod
    def forward(ctx, num_points, sh_degree, params, antialiased, max_entries, *arrays):
        image, depth, ws = _autograd_forward(ctx, num_points, sh_degree, params, antialiased, max_entries, arrays, True)
        ctx.save_for_backward(ws, *arrays)
        return image, depth[..., 0].contiguous()

    @staticmethod
    def backward(ctx, grad_image, grad_depth):
        ws, *arrays = ctx.saved_tensors
        out, _ = _autograd_backward(ctx, "depth", None, ws, arrays, grad_image, grad_depth, ctx.needs_input_grad[5:])
        return (None,) * 5 + out


class _RenderPoseFunction(torch.autograd.Function):
    """_RenderFunction with the camera's [R | t] as one more differentiable input: the forward renders params with the
    matrix replaced, the backward also runs spz_amd_render_view_backward_device over the kept workspace."""

    @staticmethod
    def forward(ctx, num_points, sh_degree, params, antialiased, max_entries, world_to_camera, *arrays):
        params = _params_with_pose(params, world_to_camera)
        image, ws = _autograd_forward(ctx, num_points, sh_degree, params, antialiased, max_entries, arrays)
        ctx.save_for_backward(image, ws, world_to_camera, *arrays)
        return image

    @staticmethod
    def backward(ctx, grad_image):
        image, ws, world_to_camera, *arrays = ctx.saved_tensors
        out, pose = _autograd_backward(ctx, "pose", image, ws, arrays, grad_image, None, ctx.needs_input_grad[6:],
                                       ctx.needs_input_grad[5])
        if pose is not None:
            pose = pose.to(device=world_to_camera.device, dtype=world_to_camera.dtype)
        return (None,) * 5 + (pose,) + out


def _six_arrays(cloud):
    """The six arrays of cloud in FIELDS order, with an empty sh for a cloud (of degree 0) that leaves it out."""
    return [t if t is not None else torch.empty(0, dtype=torch.float32, device=cloud["positions"].device)
            for t in map(cloud.get, FIELDS)]


def render_depth_autograd(cloud, num_points, sh_degree, params, antialiased=False, max_entries=None):
    """render() and the accumulated depth as one differentiable torch operation: (image, depth0), image bit-identical
    to render()'s and depth0 (height, width) bit-identical to render_depth()[..., 0]; backward() gives the six arrays of
    cloud their gradients through both (include/spz_amd.h "render depth backward").  The median depth and the index
    carry no gradient and are not returned.  Otherwise as render_autograd()."""
    return _RenderDepthFunction.apply(num_points, sh_degree, params, antialiased, max_entries, *_six_arrays(cloud))


def render_autograd(cloud, num_points, sh_degree, params, antialiased=False, max_entries=None, world_to_camera=None):
    """render() as a differentiable torch operation: the (height, width, 4) image, bit-identical to render()'s, whose
    backward() gives the six arrays of cloud their gradients (those that require grad; the others get None).  Runs on
    the current stream.  The backward is the exact derivative of the forward with its discrete decisions held constant
    (include/spz_amd.h "render backward") and sums with f32 atomic adds.  A total above max_entries raises
    RuntimeError.  A cloud without sh (degree 0) may leave "sh" out.
    world_to_camera: a (3, 4) floating-point tensor that replaces the matrix of params (rounded to float32; it must
    still pass the render's checks) and, when it requires grad, receives the gradient to its 12 entries taken as
    independent (include/spz_amd.h "render view backward").  None: params as they are."""
    arrays = _six_arrays(cloud)
    if world_to_camera is not None:
        return _RenderPoseFunction.apply(num_points, sh_degree, params, antialiased, max_entries, world_to_camera,
                                         *arrays)
    return _RenderFunction.apply(num_points, sh_degree, params, antialiased, max_entries, *arrays)


def render_packed(stream_t, header, params, max_entries=None, out=None, return_info=False, stream=None):
    """The image of a packed device stream (any version), decoded as loadSpz(to = params.coord) would: bit-identical to
    render() of the decoded floats.  Otherwise as render()."""
    _check_stream_tensor(stream_t)
    return _render(("packed", stream_t, header), header.num_points, params, stream_t.device, max_entries, out,
                   return_info, stream)


def render_depth(cloud, num_points, sh_degree, params, antialiased=False, max_entries=None, return_image=False,
                 return_index=True, out=None, return_info=False, stream=None):
    """The depth maps of a float cloud on the device (spz_amd_render_prepare_cloud_device + spz_amd_render_depth_device;
    the contract is in include/spz_amd.h "render depth"): (depth, index, image), without index when return_index is
    False and without image unless return_image.  depth: (height, width, 2) float32, channel 0 the accumulated depth
    sum (T a) z, un-normalised, channel 1 the median depth (+inf: none).  index: (height, width) int32, the median
    Gaussian's input index or -1 for none (the C ABI's uint32 0xffffffff: torch has no uint32 arithmetic).  image: as
    render(), bit for bit.  expected_depth() normalises channel 0.  out: a dict of tensors to write into (depth, index,
    image; a given one is also returned).  cloud, max_entries, return_info (appends total and status) and stream: as
    render(); with status 1 no output is written."""
    source, _, dev = _cloud_source(cloud, num_points, sh_degree, antialiased)
    return _render_depth(source, num_points, params, dev, max_entries, return_image, return_index, out, return_info,
                         stream)


def render_depth_packed(stream_t, header, params, max_entries=None, return_image=False, return_index=True, out=None,
                        return_info=False, stream=None):
    """The depth maps of a packed device stream (any version), decoded as loadSpz(to = params.coord) would:
    bit-identical to render_depth() of the decoded floats.  Otherwise as render_depth()."""
    _check_stream_tensor(stream_t)
    return _render_depth(("packed", stream_t, header), header.num_points, params, stream_t.device, max_entries,
                         return_image, return_index, out, return_info, stream)


def expected_depth(depth, alpha):
    """The normalised expected depth of render_depth(): depth[..., 0] / alpha in float32 where alpha > 0 (the image's
    alpha channel, 1 - T), +inf elsewhere."""
    acc = depth[..., 0]
    return torch.where(alpha > 0, acc / alpha, torch.full_like(acc, float("inf")))


def _score(source, n, views, dev, max_entries, images, return_status, stream):
    L = abi.load_library()
    views = list(views)
    if not 1 <= len(views) <= abi.PRUNE_MAX_VIEWS:
        raise ValueError(f"give 1..{abi.PRUNE_MAX_VIEWS} views, got {len(views)}")
    for k, p in enumerate(views):
        if not isinstance(p, abi.RenderParams):
            raise ValueError(f"view {k}: must be an abi.RenderParams (abi.render_params)")
        if L.spz_amd_render_check_params(C.byref(p)) != abi.OK:
            raise ValueError(f"view {k}: bad render parameters")
        if p.coord != views[0].coord:
            raise ValueError(f"view {k}: coord {p.coord} differs from view 0's {views[0].coord}")
    if max_entries is not None and (isinstance(max_entries, bool) or not isinstance(max_entries, int)
                                    or not 0 <= max_entries <= 0x7fffffff):
        raise ValueError(f"max_entries must be an int in 0..2^31-1, got {max_entries!r}")
    imgs = []
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            wsum = torch.zeros(n, dtype=torch.int64, device=dev)
            wmax = torch.zeros(n, dtype=torch.float32, device=dev)
            total = torch.empty(1, dtype=torch.int64, device=dev)
            status = torch.empty(len(views), dtype=torch.int32, device=dev)
            ws = None
            prefix = int(L.spz_amd_render_workspace_bytes(n, 0)) - 256
            for k, p in enumerate(views):
                if max_entries is None:
                    # prepare into the current workspace (its prefix is the prepare part), read the total, grow
                    if ws is None:
                        ws = torch.empty(prefix + 256, dtype=torch.uint8, device=dev)
                    _render_prepare(L, source, p, total, None, ws, st)
                    m = int(total.cpu()[0])  # on st: waits for the prepare step
                    if m > 0x7fffffff:
                        raise RuntimeError(f"view {k}: {m} tile entries is above the sort's limit of 2^31 - 1")
                    need = int(L.spz_amd_render_workspace_bytes(n, m))
                    if need > ws.numel():
                        bigger = torch.empty(need, dtype=torch.uint8, device=dev)
                        _aligned_view(bigger, prefix).copy_(_aligned_view(ws, prefix))
                        ws = bigger
                else:
                    m = max_entries
                    if ws is None:
                        ws = torch.empty(int(L.spz_amd_render_workspace_bytes(n, m)), dtype=torch.uint8, device=dev)
                    _render_prepare(L, source, p, total, None, ws, st)
                img = None
                if images:
                    img = torch.empty((p.height, p.width, 4), dtype=torch.float32, device=dev)
                    imgs.append(img)
                rc = L.spz_amd_render_score_device(n, C.byref(p), m, img.data_ptr() if img is not None else None,
                                                   wsum.data_ptr(), wmax.data_ptr(), status[k:].data_ptr(),
                                                   ws.data_ptr(), C.c_void_p(st.cuda_stream))
                abi.check(rc, "spz_amd_render_score_device")
    out = (wsum, wmax)
    if images:
        out += (imgs,)
    if return_status:
        out += (status,)
    return out


def score(cloud, num_points, sh_degree, views, antialiased=False, max_entries=None, images=False, return_status=False,
          stream=None):
    """Per-Gaussian blend weights of a float cloud over views (spz_amd_render_prepare_cloud_device +
    spz_amd_render_score_device per view; include/spz_amd.h "render scores"): (weight_sum, weight_max), an int64 tensor
    (the u64 sums of rint(T a 2^24); below 2^62) and a float32 tensor of n on the device.  views: abi.RenderParams, one
    coord.  max_entries None: each view's total sizes the workspace (one value read back per view); an int: the
    workspace is sized for it, and a view whose total is above it adds nothing and gets status 1.  images: also the
    list of the views' images (bit-identical to render()).  return_status: also the int32 status word of every view.
    stream: as render()."""
    source, _, dev = _cloud_source(cloud, num_points, sh_degree, antialiased)
    return _score(source, num_points, views, dev, max_entries, images,
                  return_status, stream)


def score_packed(stream_t, header, views, max_entries=None, images=False, return_status=False, stream=None):
    """The scores of a packed device stream (any version), decoded as loadSpz(to = coord) would: bit-identical to
    score() of the decoded floats.  Otherwise as score()."""
    _check_stream_tensor(stream_t)
    return _score(("packed", stream_t, header), header.num_points, views, stream_t.device, max_entries, images,
                  return_status, stream)


def _records(rec_t):
    f = rec_t.view(torch.float32).view(-1, 12)
    r16 = rec_t.view(torch.int16).view(-1, 24)
    return {"mean": f[:, 0:2], "conic": f[:, 2:5], "opacity": f[:, 5], "rgb": f[:, 6:9], "depth": f[:, 9],
            "rect": r16[:, 20:24].to(torch.int32)}


def _preprocess(source, n, params, dev, stream):
    L = abi.load_library()
    if not isinstance(params, abi.RenderParams):
        raise ValueError("params must be an abi.RenderParams (abi.render_params)")
    abi.check(L.spz_amd_render_check_params(C.byref(params)), "spz_amd_render_check_params")
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            total = torch.empty(1, dtype=torch.int64, device=dev)
            rec = torch.empty(n * abi.RENDER_RECORD_BYTES, dtype=torch.uint8, device=dev)
            ws = torch.empty(int(L.spz_amd_render_workspace_bytes(n, 0)), dtype=torch.uint8, device=dev)
            _render_prepare(L, source, params, total, rec, ws, st)
            out = _records(rec)  # the rect widening is a launch: on st too
    out["total"] = total
    return out


def preprocess(cloud, num_points, sh_degree, params, antialiased=False, stream=None):
    """The per-Gaussian records of render() (input order) as CUDA tensors: mean (n, 2), conic (n, 3: A, B, C), opacity,
    rgb (n, 3), depth (+inf: invisible), rect (n, 4 int32: tile x0, y0, x1, y1); and total (the entry count)."""
    source, _, dev = _cloud_source(cloud, num_points, sh_degree, antialiased)
    return _preprocess(source, num_points, params, dev, stream)


def preprocess_packed(stream_t, header, params, stream=None):
    """The records of render_packed(), as preprocess()."""
    _check_stream_tensor(stream_t)
    return _preprocess(("packed", stream_t, header), header.num_points, params, stream_t.device, stream)


def image_metrics(a_t, b_t, ssim_map=None, stream=None):
    """PSNR, MSE, L1, max error and SSIM of two (height, width, 3 or 4) float32 CUDA tensors on one device
    (spz_amd_image_metrics_device; the contract is in include/spz_amd.h "image metrics"): a float64 tensor [mse, psnr,
    ssim, l1, max_abs] on the device, not synchronised, so it can follow render() in a loop.  ssim_map: a contiguous
    (height, width) float32 tensor that gets the map.  stream: as render()."""
    L = abi.load_library()
    for name, t in (("a", a_t), ("b", b_t)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() \
                or t.dim() != 3 or t.shape[2] not in (3, 4):
            raise ValueError(f"{name} must be a contiguous float32 CUDA tensor of shape (height, width, 3 or 4)")
    dev = a_t.device
    if b_t.device != dev or tuple(a_t.shape[:2]) != tuple(b_t.shape[:2]):
        raise ValueError("a and b must have the same height and width, on one device")
    h, w = int(a_t.shape[0]), int(a_t.shape[1])
    abi.check(L.spz_amd_image_metrics_check(w, h, int(a_t.shape[2]), int(b_t.shape[2])), "spz_amd_image_metrics_check")
    if ssim_map is not None and (not isinstance(ssim_map, torch.Tensor) or ssim_map.dtype != torch.float32
                                 or ssim_map.device != dev or not ssim_map.is_contiguous()
                                 or tuple(ssim_map.shape) != (h, w)):
        raise ValueError(f"ssim_map must be a contiguous float32 tensor of shape ({h}, {w}) on {dev}")
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            out = torch.empty(5, dtype=torch.float64, device=dev)
            ws = torch.empty(max(8, int(L.spz_amd_image_metrics_workspace_bytes(w, h))), dtype=torch.uint8, device=dev)
            rc = L.spz_amd_image_metrics_device(a_t.data_ptr(), int(a_t.shape[2]), b_t.data_ptr(), int(b_t.shape[2]), w,
                                                h, out.data_ptr(), ssim_map.data_ptr() if ssim_map is not None else None,
                                                ws.data_ptr(), C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_image_metrics_device")
    return out


def _check_image(name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous() \
            or t.dim() != 3 or t.shape[2] not in (3, 4):
        raise ValueError(f"{name} must be a contiguous float32 CUDA tensor of shape (height, width, 3 or 4)")


def image_loss(a_t, b_t, lambda_dssim, grad=None, stream=None):
    """The 3DGS training loss L = (1 - lambda) l1 + lambda (1 - ssim) of a render a_t against a target b_t, two (height,
    width, 3 or 4) float32 CUDA tensors on one device, and its gradient to a_t (spz_amd_image_loss_device; the contract
    is in include/spz_amd.h "image loss"): (loss_t, grad_t).  loss_t: a float64 tensor [L, l1, ssim] on the device, not
    synchronised.  grad_t: float32, shaped like a_t (with four channels it is render_backward()'s grad_image); `grad`: a
    tensor to write it into.  stream: as render()."""
    L = abi.load_library()
    _check_image("a", a_t)
    _check_image("b", b_t)
    dev = a_t.device
    if b_t.device != dev or tuple(a_t.shape[:2]) != tuple(b_t.shape[:2]):
        raise ValueError("a and b must have the same height and width, on one device")
    h, w, ca, cb = int(a_t.shape[0]), int(a_t.shape[1]), int(a_t.shape[2]), int(b_t.shape[2])
    abi.check(L.spz_amd_image_metrics_check(w, h, ca, cb), "spz_amd_image_metrics_check")
    lam = float(lambda_dssim)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1], got {lambda_dssim!r}")
    _check_out("grad", grad, (h, w, ca), torch.float32, dev)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            loss = torch.empty(3, dtype=torch.float64, device=dev)
            if grad is None:
                grad = torch.empty((h, w, ca), dtype=torch.float32, device=dev)
            ws = torch.empty(int(L.spz_amd_image_loss_workspace_bytes(w, h)), dtype=torch.uint8, device=dev)
            rc = L.spz_amd_image_loss_device(a_t.data_ptr(), ca, b_t.data_ptr(), cb, w, h, lam, loss.data_ptr(),
                                             grad.data_ptr(), ws.data_ptr(), C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_image_loss_device")
    return loss, grad


def photo_loss(a_t, b_t, lambda_dssim, weight=None, exposure=None, grad=None, stream=None):
    """image_loss() of a render a_t against a photograph b_t with per-pixel weights and an exposure of the render
    (spz_amd_photo_loss_device; the contract is in include/spz_amd.h "photo loss"): (loss_t, grad_t, exposure_grad_t).
    weight: None, or a contiguous (height, width) float32 CUDA tensor, clamped to [0, 1].  exposure: None (the
    identity), or a (3, 4) array-like [M | o] of finite numbers on the host.  exposure_grad_t: a float64 CUDA tensor
    (3, 4), dL/d[M | o], or None without an exposure.  With neither, loss_t and grad_t carry image_loss()'s bits.
    Not synchronised.  stream: as render()."""
    L = abi.load_library()
    _check_image("a", a_t)
    _check_image("b", b_t)
    dev = a_t.device
    if b_t.device != dev or tuple(a_t.shape[:2]) != tuple(b_t.shape[:2]):
        raise ValueError("a and b must have the same height and width, on one device")
    h, w, ca, cb = int(a_t.shape[0]), int(a_t.shape[1]), int(a_t.shape[2]), int(b_t.shape[2])
    abi.check(L.spz_amd_image_metrics_check(w, h, ca, cb), "spz_amd_image_metrics_check")
    lam = float(lambda_dssim)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_dssim must be in [0, 1], got {lambda_dssim!r}")
    if weight is not None and (not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32
                               or weight.device != dev or not weight.is_contiguous() or tuple(weight.shape) != (h, w)):
        raise ValueError(f"weight must be a contiguous float32 tensor of shape ({h}, {w}) on {dev}")
    ex = abi.exposure_values(exposure) if exposure is not None else None
    _check_out("grad", grad, (h, w, ca), torch.float32, dev)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            loss = torch.empty(3, dtype=torch.float64, device=dev)
            if grad is None:
                grad = torch.empty((h, w, ca), dtype=torch.float32, device=dev)
            egrad = torch.empty((3, 4), dtype=torch.float64, device=dev) if ex is not None else None
            ws = torch.empty(int(L.spz_amd_photo_loss_workspace_bytes(w, h)), dtype=torch.uint8, device=dev)
            rc = L.spz_amd_photo_loss_device(a_t.data_ptr(), ca, b_t.data_ptr(), cb,
                                             weight.data_ptr() if weight is not None else None, ex, w, h, lam,
                                             loss.data_ptr(), grad.data_ptr(),
                                             egrad.data_ptr() if egrad is not None else None, ws.data_ptr(),
                                             C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_photo_loss_device")
    return loss, grad, egrad


DEPTH_KINDS = {"l1": abi.DEPTH_L1, "inverse": abi.DEPTH_INVERSE_L1}


def depth_loss(depth_t, image_t, target_t, *, weight=None, kind="l1", min_alpha=0.5, scale=1.0, grad_image=None,
               stream=None):
    """The loss of a depth render against a measured depth map and its gradient to the render
    (spz_amd_depth_loss_device; the contract is in include/spz_amd.h "depth loss"): (loss_t, grad_depth_t).
    depth_t: render_depth()'s (height, width, 2) float32 CUDA tensor (channel 0 is read); image_t: its (height, width,
    4) image (alpha is read); target_t: (height, width) float32, metric z, not finite or <= 0 where there is no
    measurement.  weight: as photo_loss().  kind: "l1" (|D / alpha - t|) or "inverse" (|alpha / D - 1 / t|).  A pixel
    counts where its weight is > 0, the target is valid, alpha >= min_alpha and D > 0.  scale multiplies the gradients,
    not the loss.  loss_t: a float64 tensor [L, W_v] on the device, not synchronised.  grad_depth_t: (height, width)
    float32, render_depth_backward()'s grad_depth.  grad_image: None, or a contiguous (height, width, 4) float32 tensor
    whose alpha channel the loss's gradient to alpha is added into (photo_loss()'s grad).  stream: as render()."""
    L = abi.load_library()
    if not isinstance(image_t, torch.Tensor) or not image_t.is_cuda:
        raise ValueError("image must be a contiguous float32 CUDA tensor of shape (height, width, 4)")
    dev = image_t.device
    if image_t.dtype != torch.float32 or not image_t.is_contiguous() or image_t.dim() != 3 or image_t.shape[2] != 4:
        raise ValueError("image must be a contiguous float32 CUDA tensor of shape (height, width, 4)")
    h, w = int(image_t.shape[0]), int(image_t.shape[1])
    abi.check(L.spz_amd_image_metrics_check(w, h, 4, 4), "spz_amd_image_metrics_check")
    for name, t, shape in (("depth", depth_t, (h, w, 2)), ("target", target_t, (h, w))):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous()
                or tuple(t.shape) != shape):
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape} on {dev}")
    if weight is not None and (not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32
                               or weight.device != dev or not weight.is_contiguous() or tuple(weight.shape) != (h, w)):
        raise ValueError(f"weight must be a contiguous float32 tensor of shape ({h}, {w}) on {dev}")
    if kind not in DEPTH_KINDS:
        raise ValueError(f"kind must be 'l1' or 'inverse', got {kind!r}")
    min_alpha, scale = float(min_alpha), float(scale)
    if not 0.0 < min_alpha <= 1.0:
        raise ValueError(f"min_alpha must be in (0, 1], got {min_alpha!r}")
    if not 0.0 <= scale < float("inf"):
        raise ValueError(f"scale must be finite and >= 0, got {scale!r}")
    _check_out("grad_image", grad_image, (h, w, 4), torch.float32, dev)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            loss = torch.empty(2, dtype=torch.float64, device=dev)
            grad = torch.empty((h, w), dtype=torch.float32, device=dev)
            ws = torch.empty(int(L.spz_amd_depth_loss_workspace_bytes(w, h)), dtype=torch.uint8, device=dev)
            rc = L.spz_amd_depth_loss_device(depth_t.data_ptr(), image_t.data_ptr(), target_t.data_ptr(),
                                             weight.data_ptr() if weight is not None else None, w, h, DEPTH_KINDS[kind],
                                             min_alpha, scale, loss.data_ptr(), grad.data_ptr(),
                                             grad_image.data_ptr() if grad_image is not None else None, ws.data_ptr(),
                                             C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_depth_loss_device")
    return loss, grad


def image_exposure(image_t, exposure, out=None, stream=None):
    """out = M a + o over the rgb channels of a (height, width, 3 or 4) float32 CUDA image, unclamped, in f32
    (spz_amd_image_exposure_device): exposure a (3, 4) array-like [M | o]; a fourth channel is copied.  out: None (a
    new tensor), or a tensor shaped like the image, which may be the image itself.  stream: as render()."""
    L = abi.load_library()
    _check_image("image", image_t)
    dev = image_t.device
    h, w, ch = (int(x) for x in image_t.shape)
    abi.check(L.spz_amd_image_metrics_check(w, h, ch, ch), "spz_amd_image_metrics_check")
    ex = abi.exposure_values(exposure)
    _check_out("out", out, (h, w, ch), torch.float32, dev)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            if out is None:
                out = torch.empty_like(image_t)
            rc = L.spz_amd_image_exposure_device(image_t.data_ptr(), ch, ex, w, h, out.data_ptr(),
                                                 C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_image_exposure_device")
    return out


def _train_ptrs(cloud, sh_degree, n, device, mask):
    """CloudPtrs of the arrays a train mask names (checked like _ptrs); the others NULL."""
    p = abi.CloudPtrs()
    for i, k in enumerate(abi.TRAIN_ARRAYS):
        need = n * floats_per_point(k, sh_degree)
        if need == 0 or not (mask >> i) & 1:
            setattr(p, k, None)
            continue
        t = cloud.get(k)
        if t is None or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() != need \
                or t.device != device:
            raise ValueError(f"[{k!r}] must be a contiguous float32 tensor of {need} elements on {device}")
        setattr(p, k, t.data_ptr())
    return p


def adam_step(cloud, grads, m, v, num_points, sh_degree, t, lrs, beta1=0.9, beta2=0.999, eps=1e-15, train=abi.TRAIN_ALL,
              skipped=None, stream=None):
    """One Adam step, in place, over the trained arrays of a float cloud (spz_amd_adam_step_device; the contract is in
    include/spz_amd.h "adam step").  cloud, grads, m, v: dicts of flat float32 CUDA tensors keyed and shaped like the
    cloud (m and v zero before step 1); the arrays `train` (names, or a mask) leaves out may be missing.  t: the step,
    from 1.  lrs: six learning rates in abi.TRAIN_ARRAYS' order, or a dict by name.  Elements whose parameter or
    gradient is not finite are left alone and counted into `skipped`, an int32 CUDA tensor [1] (a zeroed one is made
    when None) that is returned, not synchronised.  stream: as render()."""
    L = abi.load_library()
    if int(sh_degree) not in SH_DIM:
        raise ValueError(f"sh_degree must be 0..3, got {sh_degree}")
    mask = abi.train_mask(train)
    if isinstance(lrs, dict):
        lrs = [float(lrs.get(k, 0.0)) for k in abi.TRAIN_ARRAYS]
    sc = abi.adam_scalars(t, lrs, beta1, beta2, eps)
    first = next(x for x in cloud.values() if x is not None)
    dev = first.device
    n = int(num_points)
    ptrs = [_train_ptrs(c, sh_degree, n, dev, mask) for c in (cloud, grads, m, v)]
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            if skipped is None:
                skipped = torch.zeros(1, dtype=torch.int32, device=dev)
            _check_out("skipped", skipped, (1,), torch.int32, dev)
            rc = L.spz_amd_adam_step_device(C.byref(ptrs[0]), C.byref(ptrs[1]), C.byref(ptrs[2]), C.byref(ptrs[3]), n,
                                            int(sh_degree), mask, sc, skipped.data_ptr(), C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_adam_step_device")
    return skipped


def _metrics_dict(m):
    return {"mse": m.mse, "psnr": m.psnr, "ssim": m.ssim, "l1": m.l1, "max_abs": m.max_abs}


class RefineResult:
    """The output of refine_packed(): `report` (history, before, after, skipped, ms, out_bytes) and the output stream
    in device memory until close().  tensor(): a uint8 CUDA view of it (not valid after close()); fetch(): its bytes as
    a numpy array.  After close() both raise."""

    def __init__(self, ctx, out_bytes, device, report):
        self._ctx, self.out_bytes, self.device, self.report = ctx, int(out_bytes), device, report

    def _open(self):
        if self._ctx is None:
            raise RuntimeError("the refine result is closed")
        return self._ctx

    def tensor(self):
        ptr = abi.load_library().spz_amd_refine_device_data(self._open())
        return torch.as_tensor(_DeviceArray(ptr, self.out_bytes, "|u1", self), device=self.device)

    def fetch(self):
        import numpy as np
        out = np.empty(self.out_bytes, dtype=np.uint8)
        abi.check(abi.load_library().spz_amd_refine_fetch(self._open(), out.ctypes.data), "spz_amd_refine_fetch")
        return out

    def close(self):
        if self._ctx is not None:
            ctx, self._ctx = self._ctx, None
            abi.load_library().spz_amd_refine_close(ctx)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def _flat(name, t, dtype, count, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() \
            or t.numel() != count or (dev is not None and t.device != dev):
        raise ValueError(f"{name} must be a contiguous {dtype} CUDA tensor of {count} elements"
                         + (f" on {dev}" if dev is not None else ""))
    return t


def densify_accumulate(records, record_grads, width, height, accum, denom, stream=None):
    """Add one view's screen-space position gradient norms to accum (float32 [n]) and count the view in denom (int32
    [n]) for every visible Gaussian (spz_amd_densify_accumulate_device; include/spz_amd.h "densify").  records: the
    view's n raw 48-byte render records, a uint8 CUDA tensor of 48 n bytes (the front of a render workspace, 256-aligned);
    record_grads: render_backward(..., return_record_grads=True)["records"], (n, 9) float32.  In place; returns None."""
    L = abi.load_library()
    n = int(accum.numel()) if isinstance(accum, torch.Tensor) else -1
    dev = accum.device if isinstance(accum, torch.Tensor) else None
    _flat("accum", accum, torch.float32, n, None)
    _flat("denom", denom, torch.int32, n, dev)
    _flat("records", records, torch.uint8, n * abi.RENDER_RECORD_BYTES, dev)
    _flat("record_grads", record_grads, torch.float32, n * 9, dev)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        rc = L.spz_amd_densify_accumulate_device(records.data_ptr(), record_grads.data_ptr(), n, int(width), int(height),
                                                 accum.data_ptr(), denom.data_ptr(), C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_densify_accumulate_device")


def densify_plan(accum, denom, scales, alphas, limits, max_points, stream=None):
    """Decide one densify round (spz_amd_densify_plan_host; include/spz_amd.h "densify"): accum (float32 [n]), denom
    (int32 [n]), the cloud's flat log scales [3 n] and alpha logits [n], limits (abi.densify_thresholds) and the cap
    max_points.  Blocks for the counts.  Returns a dict: action (uint8 [n]: abi.DENSIFY_KEEP / CLONE / SPLIT / CULL),
    parent (int32 [n']) and child (uint8 [n']) for densify_apply, and num_points, cloned, split, culled, refused."""
    L = abi.load_library()
    if not isinstance(limits, abi.DensifyLimits):
        raise ValueError("limits must be an abi.DensifyLimits (abi.densify_thresholds)")
    if isinstance(max_points, bool) or not isinstance(max_points, int) or max_points < 0:
        raise ValueError(f"max_points must be a non-negative int, got {max_points!r}")
    n = int(accum.numel()) if isinstance(accum, torch.Tensor) else -1
    dev = accum.device if isinstance(accum, torch.Tensor) else None
    _flat("accum", accum, torch.float32, n, None)
    _flat("denom", denom, torch.int32, n, dev)
    _flat("scales", scales, torch.float32, 3 * n, dev)
    _flat("alphas", alphas, torch.float32, n, dev)
    cap = min(2 * n, max(max_points, n))
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            action = torch.empty(n, dtype=torch.uint8, device=dev)
            parent = torch.empty(cap, dtype=torch.int32, device=dev)
            child = torch.empty(cap, dtype=torch.uint8, device=dev)
            counts = torch.empty(5, dtype=torch.int64, device=dev)
            ws = torch.empty(max(8, int(L.spz_amd_densify_plan_workspace_bytes(n))), dtype=torch.uint8, device=dev)
            h = (C.c_uint64 * 5)()
            rc = L.spz_amd_densify_plan_host(accum.data_ptr(), denom.data_ptr(), scales.data_ptr(), alphas.data_ptr(), n,
                                             C.byref(limits), max_points, cap, action.data_ptr(), parent.data_ptr(),
                                             child.data_ptr(), counts.data_ptr(), ws.data_ptr(), h,
                                             C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_densify_plan_host")
    m = int(h[0])
    return {"action": action, "parent": parent[:m], "child": child[:m], "num_points": m, "cloned": int(h[1]),
            "split": int(h[2]), "culled": int(h[3]), "refused": int(h[4])}


def densify_apply(cloud, m, v, num_points, sh_degree, parent, child, seed=0, round=0, stream=None):
    """Rewrite a float cloud and its two Adam moments at a plan's new count (spz_amd_densify_apply_device; include/
    spz_amd.h "densify"): one launch gathering all 18 arrays through parent.  cloud, m, v: dicts of flat float32 CUDA
    tensors of num_points Gaussians (sh may be missing at degree 0).  Returns (cloud', m', v') as new dicts."""
    L = abi.load_library()
    if int(sh_degree) not in SH_DIM:
        raise ValueError(f"sh_degree must be 0..3, got {sh_degree}")
    n = int(num_points)
    dev = cloud["positions"].device
    n_new = int(parent.numel()) if isinstance(parent, torch.Tensor) else -1
    _flat("parent", parent, torch.int32, n_new, dev)
    _flat("child", child, torch.uint8, n_new, dev)
    src = [_ptrs(c, sh_degree, n, dev) for c in (cloud, m, v)]
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            out = [alloc_cloud(n_new, sh_degree, dev) for _ in range(3)]
            dst = [_ptrs(c, sh_degree, n_new, dev) for c in out]
            rc = L.spz_amd_densify_apply_device(C.byref(src[0]), C.byref(src[1]), C.byref(src[2]), C.byref(dst[0]),
                                                C.byref(dst[1]), C.byref(dst[2]), parent.data_ptr(), child.data_ptr(), n,
                                                n_new, n_new, int(sh_degree), int(seed), int(round),
                                                C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_densify_apply_device")
    return tuple(out)


def reset_opacity(alphas, m=None, v=None, stream=None):
    """3DGS's opacity reset, in place (spz_amd_densify_reset_opacity_device): alphas = min(alphas, logit(0.01)), NaN
    left alone; the alphas' Adam moments m and v (float32 [n], or None) zeroed."""
    L = abi.load_library()
    n = int(alphas.numel()) if isinstance(alphas, torch.Tensor) else -1
    dev = alphas.device if isinstance(alphas, torch.Tensor) else None
    _flat("alphas", alphas, torch.float32, n, None)
    for name, t in (("m", m), ("v", v)):
        if t is not None:
            _flat(name, t, torch.float32, n, dev)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        rc = L.spz_amd_densify_reset_opacity_device(alphas.data_ptr(), m.data_ptr() if m is not None else None,
                                                    v.data_ptr() if v is not None else None, n,
                                                    C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_densify_reset_opacity_device")


def _refine_open(entry, head, opts, mid, dev, nv, room=None, origin_room=0, extra=()):
    """What the refine forms share: the outputs every open entry has, the call entry(*head, &opts, *mid, device, the
    shared outputs[, densify's outputs], *extra), SpzAmdError with `.view` on a refusal, and the common part of the
    report.  room: None for spz_amd_refine_open, which has no densify outputs; otherwise the rounds the caller has room
    for, and origin_room the points.  Returns (ctx, report, origin); the report has num_points and rounds, and origin is
    the output's origin map, only with room."""
    import numpy as np
    ctx, out_bytes, skipped, bad = C.c_void_p(), C.c_uint64(), C.c_uint64(), C.c_int32(-1)
    history = (C.c_double * max(1, opts.iterations))()
    before, after = (abi.ImageMetrics * nv)(), (abi.ImageMetrics * nv)()
    ms = (C.c_float * 3)()
    densify_out = ()
    if room is not None:
        h_rounds, n_rounds, n_out = (abi.DensifyRound * max(1, room))(), C.c_int32(), C.c_uint64()
        origin = np.empty(origin_room, dtype=np.uint32)
        densify_out = (C.byref(n_out), h_rounds, room, C.byref(n_rounds), origin.ctypes.data)
    torch.cuda.current_stream(dev).synchronize()  # the producers of the streams and the images
    device_index = dev.index if dev.index is not None else torch.cuda.current_device()
    rc = getattr(abi.load_library(), entry)(*head, C.byref(opts), *mid, device_index, C.byref(ctx), C.byref(out_bytes),
                                            history, before, after, C.byref(skipped), ms, C.byref(bad), *densify_out,
                                            *extra)
    if rc != abi.OK:
        err = abi.SpzAmdError(rc, entry + (f" (view {bad.value})" if bad.value >= 0 else ""))
        err.view = bad.value
        raise err
    report = {"history": [history[i] for i in range(max(0, opts.iterations))],
              "before": [_metrics_dict(x) for x in before], "after": [_metrics_dict(x) for x in after],
              "skipped": int(skipped.value), "ms": tuple(ms), "out_bytes": int(out_bytes.value)}
    if room is None:
        return ctx, report, None
    report["num_points"] = int(n_out.value)
    report["rounds"] = [{k: int(getattr(r, k)) for k in ("iteration", "cloned", "split", "culled", "refused",
                                                         "num_points")} for r in h_rounds[:min(room, n_rounds.value)]]
    return ctx, report, origin[:report["num_points"]].copy()


def refine_packed(stream_a, header_a, stream_b, header_b, views, iterations, *, lambda_dssim=None, lrs=None, beta1=None,
                  beta2=None, eps=None, train=None, densify=None):
    """Fit the resident packed stream A to the target B over `views` (a sequence of abi.RenderParams, one coord):
    spz_amd_refine_open (include/spz_amd.h "refine").  Options left None take spz_amd_refine_default_options' values
    (lrs[0], the position rate, is for a scene of unit extent: scale it by the scene's).  Blocks; runs on a stream of
    the library's own after the current stream has drained.  Returns a RefineResult; a bad view raises
    abi.SpzAmdError whose `view` attribute names it.
    densify: None, or a dict / abi.DensifyOptions (abi.densify_options) for spz_amd_refine_densify_open: Gaussians are
    cloned, split and culled while fitting, up to max_points (0: B's count).  The report's num_points is the output's
    count, rounds one dict per round (iteration, cloned, split, culled, refused, num_points), and origin the index in A
    of every output point (a numpy uint32 array)."""
    _check_stream_tensor(stream_a)
    _check_stream_tensor(stream_b)
    dev = stream_a.device
    if stream_b.device != dev:
        raise ValueError("the two streams must be on one device")
    views = list(views)
    if not 1 <= len(views) <= abi.REFINE_MAX_VIEWS or not all(isinstance(p, abi.RenderParams) for p in views):
        raise ValueError(f"views must be 1..{abi.REFINE_MAX_VIEWS} abi.RenderParams")
    opts = abi.refine_options(iterations, lambda_dssim=lambda_dssim, lrs=lrs, beta1=beta1, beta2=beta2, eps=eps,
                              train=train)
    head = (stream_a.data_ptr(), stream_a.numel(), C.byref(header_a), stream_b.data_ptr(), stream_b.numel(),
            C.byref(header_b), (abi.RenderParams * len(views))(*views), len(views))
    if densify is None:
        ctx, report, _ = _refine_open("spz_amd_refine_open", head, opts, (), dev, len(views))
        report.update(num_points=int(header_a.num_points), rounds=[])
    else:
        dopts = abi.densify_options(densify)
        ctx, report, origin = _refine_open(
            "spz_amd_refine_densify_open", head, opts, (C.byref(dopts),), dev, len(views),
            room=max(1, opts.iterations // max(1, dopts.interval)),
            origin_room=max(int(dopts.max_points) or int(header_b.num_points), int(header_a.num_points), 1))
        report["origin"] = origin
    return RefineResult(ctx, report["out_bytes"], dev, report)


def refine_packed_images(stream_a, header_a, views, images, iterations, *, weights=None, fit_exposure=False,
                         lr_exposure=None, lambda_dssim=None, lrs=None, beta1=None, beta2=None, eps=None, train=None,
                         densify=None, depths=None, depth_weight=None, depth_kind=None, depth_min_alpha=None):
    """refine_packed() against photographs: spz_amd_refine_images_open (include/spz_amd.h "refine images").  images: one
    contiguous (height, width, C) float32 CUDA tensor per view, of the view's size, C in {3, 4} and the same for all;
    they are used in place.  weights: None, or one entry per view, each None or a contiguous (height, width) float32
    CUDA tensor.  fit_exposure: fit a 3 x 4 exposure per view beside the cloud, at rate lr_exposure (None: 0.01).
    densify: as refine_packed(), but max_points must be given.  Returns a RefineResult whose report also has
    `exposures`, a float64 numpy array (views, 3, 4): the identity without fit_exposure.
    depths: None, or one entry per view, each None or a contiguous (height, width) float32 CUDA tensor of metric depth
    along the camera's z (not finite or <= 0: no measurement): spz_amd_refine_images_depth_open (include/spz_amd.h
    "refine images with depth") adds depth_weight (None: 1.0) times the depth loss of kind depth_kind ("l1", the
    default, or "inverse") over the pixels of alpha >= depth_min_alpha (None: 0.5).  The report then also has
    `depth_history` (the depth loss before each step, 0 for a view without a map) and `depth_error`, a float64 numpy
    array (views, 2): the depth loss of A and of the output against the map, -1 for a view without one."""
    import numpy as np
    _check_stream_tensor(stream_a)
    dev = stream_a.device
    views = list(views)
    if not 1 <= len(views) <= abi.REFINE_MAX_VIEWS or not all(isinstance(p, abi.RenderParams) for p in views):
        raise ValueError(f"views must be 1..{abi.REFINE_MAX_VIEWS} abi.RenderParams")
    images = list(images)
    if len(images) != len(views):
        raise ValueError(f"images must have one entry per view: {len(images)} images, {len(views)} views")
    weights = [None] * len(views) if weights is None else list(weights)
    if len(weights) != len(views):
        raise ValueError(f"weights must have one entry per view: {len(weights)} weights, {len(views)} views")
    channels = None
    for k, (p, img, wt) in enumerate(zip(views, images, weights)):
        _check_image(f"images[{k}]", img)
        shape = (int(p.height), int(p.width))
        if img.device != dev or tuple(img.shape[:2]) != shape:
            raise ValueError(f"images[{k}] must be {shape[0]} x {shape[1]} (view {k}'s size) on {dev}, got "
                             f"{tuple(img.shape[:2])} on {img.device}")
        if channels is None:
            channels = int(img.shape[2])
        if int(img.shape[2]) != channels:
            raise ValueError(f"every image must have {channels} channels, images[{k}] has {int(img.shape[2])}")
        if wt is not None and (not isinstance(wt, torch.Tensor) or wt.dtype != torch.float32 or wt.device != dev
                               or not wt.is_contiguous() or tuple(wt.shape) != shape):
            raise ValueError(f"weights[{k}] must be a contiguous float32 tensor of shape {shape} on {dev}")
    opts = abi.refine_options(iterations, lambda_dssim=lambda_dssim, lrs=lrs, beta1=beta1, beta2=beta2, eps=eps,
                              train=train)
    popts = abi.photo_options(fit_exposure, lr_exposure)
    dopts = abi.densify_options(densify) if densify is not None else None
    nv = len(views)
    if depths is None:
        if depth_weight is not None or depth_kind is not None or depth_min_alpha is not None:
            raise ValueError("depth_weight, depth_kind and depth_min_alpha need depths")
    else:
        depths = list(depths)
        if len(depths) != nv:
            raise ValueError(f"depths must have one entry per view: {len(depths)} depths, {nv} views")
        for k, (p, dm) in enumerate(zip(views, depths)):
            shape = (int(p.height), int(p.width))
            if dm is not None and (not isinstance(dm, torch.Tensor) or dm.dtype != torch.float32 or dm.device != dev
                                   or not dm.is_contiguous() or tuple(dm.shape) != shape):
                raise ValueError(f"depths[{k}] must be a contiguous float32 tensor of shape {shape} on {dev}")
        zopts = abi.depth_options(depth_weight, depth_kind, depth_min_alpha)
        zptrs = (C.c_void_p * nv)(*[dm.data_ptr() if dm is not None else None for dm in depths])
        depth_history = (C.c_double * max(1, opts.iterations))()
        depth_error = np.zeros((nv, 2), dtype=np.float64)
    head = (stream_a.data_ptr(), stream_a.numel(), C.byref(header_a), (abi.RenderParams * nv)(*views), nv,
            (C.c_void_p * nv)(*[img.data_ptr() for img in images]), channels,
            (C.c_void_p * nv)(*[wt.data_ptr() if wt is not None else None for wt in weights])
            if any(wt is not None for wt in weights) else None)
    exposures = np.zeros((nv, 3, 4), dtype=np.float64)
    entry, extra = "spz_amd_refine_images_open", (exposures.ctypes.data,)
    if depths is not None:
        entry, extra = "spz_amd_refine_images_depth_open", extra + (depth_history, depth_error.ctypes.data)
        head += (zptrs if any(dm is not None for dm in depths) else None, C.byref(zopts))
    ctx, report, origin = _refine_open(
        entry, head, opts, (C.byref(popts), C.byref(dopts) if dopts is not None else None), dev, nv,
        room=max(1, opts.iterations // max(1, dopts.interval)) if dopts is not None else 0,
        origin_room=max(int(dopts.max_points) if dopts is not None else 0, int(header_a.num_points), 1), extra=extra)
    report["exposures"] = exposures
    if dopts is not None:
        report["origin"] = origin
    if depths is not None:
        report["depth_history"] = [depth_history[i] for i in range(max(0, opts.iterations))]
        report["depth_error"] = depth_error
    return RefineResult(ctx, report["out_bytes"], dev, report)


def image_halve(image_t, stream=None):
    """The 2 x 2 box mean of a (height, width, 3 or 4) float32 CUDA image with even sides
    (spz_amd_image_halve_device): ((top left + top right) + (bottom left + bottom right)) / 4 in f32, channels kept.
    The target of the next coarser level of locate().  stream: as render()."""
    L = abi.load_library()
    _check_image("image", image_t)
    h, w, ch = (int(x) for x in image_t.shape)
    if h % 2 or w % 2:
        raise ValueError(f"width and height must be even, got {w} x {h}")
    dev = image_t.device
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            out = torch.empty((h // 2, w // 2, ch), dtype=torch.float32, device=dev)
            rc = L.spz_amd_image_halve_device(image_t.data_ptr(), ch, w, h, out.data_ptr(), C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_image_halve_device")
    return out


def _locate(entry, call, params, target, options):
    import numpy as np
    if not isinstance(params, abi.RenderParams):
        raise ValueError("params must be an abi.RenderParams (abi.render_params)")
    _check_image("target", target)
    if tuple(target.shape[:2]) != (params.height, params.width):
        raise ValueError(f"target must be ({params.height}, {params.width}, 3 or 4)")
    opts = abi.locate_options(**options)
    pose = (C.c_float * 12)()
    history = (C.c_double * max(1, opts.iterations))()
    before, after = abi.ImageMetrics(), abi.ImageMetrics()
    ran = C.c_int32()
    ms = (C.c_float * 3)()
    dev = target.device
    torch.cuda.current_stream(dev).synchronize()  # the inputs' producers
    device_index = dev.index if dev.index is not None else torch.cuda.current_device()
    rc = call(C.byref(params), target.data_ptr(), int(target.shape[2]), C.byref(opts), device_index, pose, history,
              C.byref(before), C.byref(after), C.byref(ran), ms)
    abi.check(rc, entry)
    return {"world_to_camera": np.array(list(pose), dtype=np.float32).reshape(3, 4),
            "history": [history[i] for i in range(ran.value)], "iterations": int(ran.value),
            "before": _metrics_dict(before), "after": _metrics_dict(after), "ms": tuple(ms)}


def locate(cloud, num_points, sh_degree, params, target, *, antialiased=False, **options):
    """The pose of the camera that took `target` in the scene `cloud` (device tensors, as render() takes them), from
    the rough pose in params (spz_amd_locate_cloud_host; the contract is in include/spz_amd.h "locate").  target: a
    (height, width, 3 or 4) float32 CUDA tensor of params' size.  options: abi.LOCATE_FIELDS (iterations, levels,
    lambda_dssim, lr_rotation, lr_translation, lr_final_factor, beta1, beta2, eps).  Blocks.  Returns a dict:
    world_to_camera (a (3, 4) float32 numpy array), history (the loss before each step taken), iterations (steps
    taken), before and after (the metrics of the render against the target at the initial and the final pose), ms."""
    ptrs, dev = _cloud_render_args(cloud, num_points, sh_degree)
    L = abi.load_library()
    if isinstance(target, torch.Tensor) and target.device != dev:
        raise ValueError("the cloud and the target must be on one device")
    return _locate("spz_amd_locate_cloud_host",
                   lambda *a: L.spz_amd_locate_cloud_host(C.byref(ptrs), num_points, int(sh_degree),
                                                          1 if antialiased else 0, *a), params, target, options)


def locate_packed(stream_t, header, params, target, **options):
    """locate() of a packed device stream (any version), decoded once as loadSpz(to = params.coord) would
    (spz_amd_locate_host); before and after are the metrics of the packed render."""
    _check_stream_tensor(stream_t)
    L = abi.load_library()
    if isinstance(target, torch.Tensor) and target.device != stream_t.device:
        raise ValueError("the stream and the target must be on one device")
    return _locate("spz_amd_locate_host",
                   lambda *a: L.spz_amd_locate_host(stream_t.data_ptr(), stream_t.numel(), C.byref(header), *a), params,
                   target, options)


def _check_volume(volume):
    if not isinstance(volume, abi.TsdfVolume):
        raise ValueError("volume must be an abi.TsdfVolume (abi.tsdf_volume, abi.tsdf_volume_from_box)")
    abi.check(abi.load_library().spz_amd_tsdf_check(C.byref(volume)), "spz_amd_tsdf_check")
    return tuple(int(d) for d in volume.dims)


def _check_grid(grid, volume):
    nx, ny, nz = _check_volume(volume)
    if not isinstance(grid, torch.Tensor) or not grid.is_cuda or grid.dtype != torch.float32 \
            or not grid.is_contiguous() or tuple(grid.shape) != (5, nz, ny, nx):
        raise ValueError(f"grid must be a contiguous float32 CUDA tensor of shape (5, {nz}, {ny}, {nx})")
    return grid.device


def tsdf_alloc(volume, device):
    """A new, all-zero grid of `volume` (an abi.TsdfVolume) on `device`: a (5, nz, ny, nx) float32 tensor, the planes
    W, S, Cr, Cg, Cb of include/spz_amd.h "mesh"."""
    nx, ny, nz = _check_volume(volume)
    return torch.zeros((5, nz, ny, nx), dtype=torch.float32, device=device)


def tsdf_integrate(grid, volume, params, depth, image, depth_kind="median", min_alpha=0.5, stream=None):
    """Fuse one view into `grid` in place (spz_amd_tsdf_integrate_device; the contract is in include/spz_amd.h "mesh").
    depth (height, width, 2) and image (height, width, 4): float32 CUDA tensors as render_depth(return_image=True)
    returns them.  depth_kind: "median" or "expected".  Enqueues; returns grid."""
    L = abi.load_library()
    dev = _check_grid(grid, volume)
    _check_render_args(L, params, None)
    h, w = params.height, params.width
    for name, t, ch in (("depth", depth, 2), ("image", image, 4)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() \
                or tuple(t.shape) != (h, w, ch):
            raise ValueError(f"{name} must be a contiguous float32 tensor of shape ({h}, {w}, {ch}) on {dev}")
    if depth_kind not in abi.MESH_DEPTH_KINDS:
        raise ValueError(f"depth_kind must be 'median' or 'expected', got {depth_kind!r}")
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        rc = L.spz_amd_tsdf_integrate_device(C.byref(volume), grid.data_ptr(), C.byref(params), depth.data_ptr(),
                                             image.data_ptr(), abi.MESH_DEPTH_KINDS[depth_kind], float(min_alpha),
                                             C.c_void_p(st.cuda_stream))
    abi.check(rc, "spz_amd_tsdf_integrate_device")
    return grid


def tsdf_extract(grid, volume, min_weight=1.0, stream=None):
    """The zero level set of `grid` by marching tetrahedra (spz_amd_mesh_count_device, the two counts read back,
    spz_amd_mesh_emit_device): (vertices (n_v, 3) float32, colors (n_v, 3) float32, triangles (n_t, 3) int32 holding
    the uint32 vertex numbers) as CUDA tensors, in the fixed order of include/spz_amd.h "mesh"."""
    L = abi.load_library()
    dev = _check_grid(grid, volume)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            ws = torch.empty(int(L.spz_amd_mesh_workspace_bytes(C.byref(volume))), dtype=torch.uint8, device=dev)
            counts = torch.empty(2, dtype=torch.int64, device=dev)
            rc = L.spz_amd_mesh_count_device(C.byref(volume), grid.data_ptr(), float(min_weight), counts.data_ptr(),
                                             ws.data_ptr(), C.c_void_p(st.cuda_stream))
            abi.check(rc, "spz_amd_mesh_count_device")
            nv, nt = (int(x) for x in counts.cpu())  # on st: waits for the scans
            if nv > 0xffffffff:
                raise RuntimeError(f"{nv} vertices is above the limit of 2^32 - 1")
            vertices = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            colors = torch.empty((nv, 3), dtype=torch.float32, device=dev)
            triangles = torch.empty((nt, 3), dtype=torch.int32, device=dev)
            rc = L.spz_amd_mesh_emit_device(C.byref(volume), grid.data_ptr(), nv, nt, nv, nt, vertices.data_ptr(),
                                            colors.data_ptr(), triangles.data_ptr(), ws.data_ptr(),
                                            C.c_void_p(st.cuda_stream))
            abi.check(rc, "spz_amd_mesh_emit_device")
    return vertices, colors, triangles


def volume_dict(volume):
    """An abi.TsdfVolume as plain values: lo, voxel_size, dims, truncation."""
    return {"lo": tuple(float(x) for x in volume.lo), "voxel_size": float(volume.voxel_size),
            "dims": tuple(int(x) for x in volume.dims), "truncation": float(volume.truncation)}


def mesh_packed(stream_t, header, views, **options):
    """The triangle mesh of a packed device stream over `views` (a sequence of abi.RenderParams, one coord):
    spz_amd_mesh_open (include/spz_amd.h "mesh").  options: abi.MESH_FIELDS (box, voxel_size or resolution, truncation,
    depth, min_alpha, min_weight).  Blocks; runs on a stream of the library's own after the current stream has
    drained.  Returns a dict: vertices (n_v, 3) float32, colors (n_v, 3) float32 and triangles (n_t, 3) uint32 numpy
    arrays, volume (volume_dict) and ms (renders, fuses, extraction).  A bad view raises abi.SpzAmdError whose `view`
    attribute names it."""
    import numpy as np
    L = abi.load_library()
    _check_stream_tensor(stream_t)
    dev = stream_t.device
    views = list(views)
    if not 1 <= len(views) <= abi.MESH_MAX_VIEWS or not all(isinstance(p, abi.RenderParams) for p in views):
        raise ValueError(f"views must be 1..{abi.MESH_MAX_VIEWS} abi.RenderParams")
    opts = abi.mesh_options(**options)
    arr = (abi.RenderParams * len(views))(*views)
    ctx, bad, vol = C.c_void_p(), C.c_int32(-1), abi.TsdfVolume()
    counts, ms = (C.c_uint64 * 2)(), (C.c_float * 3)()
    torch.cuda.current_stream(dev).synchronize()  # the stream's producers
    device_index = dev.index if dev.index is not None else torch.cuda.current_device()
    rc = L.spz_amd_mesh_open(stream_t.data_ptr(), stream_t.numel(), C.byref(header), arr, len(views), C.byref(opts),
                             device_index, C.byref(ctx), counts, C.byref(vol), ms, C.byref(bad))
    if rc != abi.OK:
        err = abi.SpzAmdError(rc, "spz_amd_mesh_open" + (f" (view {bad.value})" if bad.value >= 0 else ""))
        err.view = bad.value
        raise err
    try:
        vertices = np.empty((counts[0], 3), np.float32)
        colors = np.empty((counts[0], 3), np.float32)
        triangles = np.empty((counts[1], 3), np.uint32)
        abi.check(L.spz_amd_mesh_fetch(ctx, vertices.ctypes.data, colors.ctypes.data, triangles.ctypes.data),
                  "spz_amd_mesh_fetch")
    finally:
        L.spz_amd_mesh_close(ctx)
    return {"vertices": vertices, "colors": colors, "triangles": triangles, "volume": volume_dict(vol), "ms": tuple(ms)}


def _seed_capacity_ptrs(cloud, capacity, sh_degree, dev):
    p = abi.CloudPtrs()
    for k in FIELDS:
        need = capacity * floats_per_point(k, sh_degree)
        t = cloud.get(k)
        if need == 0:
            setattr(p, k, None)
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() \
                or t.numel() < need:
            raise ValueError(f"cloud[{k!r}] must be a contiguous float32 tensor of at least {need} elements on {dev}")
        setattr(p, k, t.data_ptr())
    return p


def _check_map(name, t, shape, dev):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev or not t.is_contiguous() \
            or tuple(t.shape) != shape:
        raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape} on {dev}")


def seed_view(cloud, num_points, capacity, sh_degree, params, image, depth, *, weights=None, cover=True, stride=1,
              scale_factor=1.0, opacity=0.5, cover_alpha=0.5, cover_tolerance=0.05, max_entries=None, stream=None):
    """Seed one posed RGB-D view into a float cloud in place (the cover render of the first num_points Gaussians, then
    spz_amd_seed_view_device; the contract is in include/spz_amd.h "seed").  cloud: device tensors keyed like the
    GaussianCloud fields, each with room for `capacity` Gaussians, in the frame of the camera `params`
    (abi.render_params).  image (height, width, 3 or 4), depth (height, width) and weights (height, width, or None):
    float32 CUDA tensors.  With cover set and num_points > 0 the cloud so far is rendered (render_depth, not
    antialiased, max_sh_degree = sh_degree, background 0) and samples it explains are skipped.  max_entries: as render();
    a cover render whose entry total is above it raises RuntimeError before anything is appended.  Returns
    (new_num_points, counts): counts = (valid, appended, refused), read back once."""
    L = abi.load_library()
    _check_render_args(L, params, max_entries)
    opts = abi.seed_options(stride=stride, scale_factor=scale_factor, opacity=opacity, cover=cover,
                            cover_alpha=cover_alpha, cover_tolerance=cover_tolerance, sh_degree=sh_degree)
    for name, x in (("num_points", num_points), ("capacity", capacity)):
        if isinstance(x, bool) or not isinstance(x, int) or x < 0:
            raise ValueError(f"{name} must be a non-negative int, got {x!r}")
    if num_points > capacity:
        raise ValueError(f"num_points {num_points} is above capacity {capacity}")
    dev = depth.device if isinstance(depth, torch.Tensor) else None
    h, w = params.height, params.width
    _check_map("depth", depth, (h, w), dev)
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or image.shape[2] not in (3, 4):
        raise ValueError(f"image must be a float32 tensor of shape ({h}, {w}, 3 or 4)")
    _check_map("image", image, (h, w, int(image.shape[2])), dev)
    if weights is not None:
        _check_map("weights", weights, (h, w), dev)
    ptrs = _seed_capacity_ptrs(cloud, capacity, sh_degree, dev)
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            cimage = cdepth = None
            if opts.cover and num_points > 0:
                view = abi.RenderParams.from_buffer_copy(params)
                view.max_sh_degree = int(sh_degree)
                for a in range(3):
                    view.background[a] = 0.0
                head = {k: cloud[k][: num_points * floats_per_point(k, sh_degree)] for k in FIELDS
                        if floats_per_point(k, sh_degree)}
                cdepth, cimage, total, status = render_depth(head, num_points, sh_degree, view, antialiased=False,
                                                             max_entries=max_entries, return_image=True,
                                                             return_index=False, return_info=True, stream=st)
                # with status 1 the render wrote neither map: nothing may be decided on them
                if max_entries is not None and int(status.cpu()[0]) != 0:  # on st: waits for the depth blend
                    raise RuntimeError(f"{int(total.cpu()[0])} tile entries is above max_entries = {max_entries}")
            ws = torch.empty(int(L.spz_amd_seed_workspace_bytes(w, h, opts.stride)), dtype=torch.uint8, device=dev)
            counts = torch.empty(3, dtype=torch.int64, device=dev)
            rc = L.spz_amd_seed_view_device(C.byref(ptrs), num_points, capacity, int(sh_degree), C.byref(params),
                                            C.byref(opts), image.data_ptr(), int(image.shape[2]), depth.data_ptr(),
                                            weights.data_ptr() if weights is not None else None,
                                            cimage.data_ptr() if cimage is not None else None,
                                            cdepth.data_ptr() if cdepth is not None else None, counts.data_ptr(),
                                            ws.data_ptr(), C.c_void_p(st.cuda_stream))
            abi.check(rc, "spz_amd_seed_view_device")
            got = tuple(int(x) for x in counts.cpu())  # on st: waits for the emit
    return num_points + got[1], got


def seed(views, images, depths, *, weights=None, sh_degree=0, max_points=0, stream=None, **options):
    """A float cloud from posed RGB-D views on device tensors: seed_view over `views` (a sequence of abi.RenderParams,
    one coord) in order, into a cloud allocated for max_points Gaussians (0: the sum of the views' sample counts, at
    most abi.REFERENCE_MAX_POINTS).  images, depths and weights (None, or one tensor or None per view): as seed_view.
    options: seed_view's keywords.  Returns (cloud, num_points, counts): the cloud trimmed to num_points, and one
    (valid, appended, refused) per view."""
    views, images, depths = list(views), list(images), list(depths)
    if not 1 <= len(views) <= abi.SEED_MAX_VIEWS or not all(isinstance(p, abi.RenderParams) for p in views):
        raise ValueError(f"views must be 1..{abi.SEED_MAX_VIEWS} abi.RenderParams")
    if len(images) != len(views) or len(depths) != len(views):
        raise ValueError(f"{len(views)} views, {len(images)} images and {len(depths)} depths: the counts differ")
    weights = [None] * len(views) if weights is None else list(weights)
    if len(weights) != len(views):
        raise ValueError(f"{len(views)} views and {len(weights)} weights: the counts differ")
    if any(p.coord != views[0].coord for p in views):
        raise ValueError("views must share one coord")
    if isinstance(max_points, bool) or not isinstance(max_points, int) or not 0 <= max_points <= abi.REFERENCE_MAX_POINTS:
        raise ValueError(f"max_points must be an int in 0..{abi.REFERENCE_MAX_POINTS}, got {max_points!r}")
    stride = options.get("stride", 1)
    abi.seed_options(stride=stride, sh_degree=sh_degree)
    capacity = max_points or min(abi.REFERENCE_MAX_POINTS,
                                 sum(abi.seed_samples(p.width, p.height, stride) for p in views))
    if not isinstance(depths[0], torch.Tensor) or not depths[0].is_cuda:
        raise ValueError("depths must be float32 CUDA tensors")
    dev = depths[0].device
    with torch.cuda.device(dev):
        st = _on_stream(dev, stream)
        with torch.cuda.stream(st):
            cloud = alloc_cloud(capacity, sh_degree, dev)
            n, counts = 0, []
            for p, image, depth, weight in zip(views, images, depths, weights):
                n, got = seed_view(cloud, n, capacity, sh_degree, p, image, depth, weights=weight, stream=st, **options)
                counts.append(got)
            cloud = {k: cloud[k][: n * floats_per_point(k, sh_degree)] for k in FIELDS}
    return cloud, n, counts


def convert_coordinates(cloud, num_points, sh_degree, from_coord, to_coord, stream=None):
    """In-place GaussianCloud::convertCoordinates on device tensors (positions, rotations, sh)."""
    L = abi.load_library()
    dev = cloud["positions"].device

    def ptr(k):
        t = cloud.get(k)
        return t.data_ptr() if t is not None and t.numel() else None

    with torch.cuda.device(dev):
        rc = L.spz_amd_convert_coordinates_device(ptr("positions"), ptr("rotations"), ptr("sh"), num_points,
                                                  sh_degree, from_coord, to_coord, _stream_handle(stream))
    abi.check(rc, "spz_amd_convert_coordinates_device")
    return cloud


def to_device(cloud_np, device):
    return {k: torch.from_numpy(cloud_np[k]).to(device) for k in FIELDS}


def to_numpy(cloud_t):
    return {k: cloud_t[k].cpu().numpy() for k in FIELDS}


__all__ = ["encode", "decode", "encode_shard", "decode_shard", "decode_gather", "peek_header", "convert_coordinates",
           "select", "subset", "transform", "transform_packed", "merge_packed",
           "alloc_cloud", "image_loss", "adam_step", "refine_packed",
           "densify_accumulate", "densify_plan", "densify_apply", "reset_opacity",
           "render_view_backward", "image_halve", "locate", "locate_packed",
           "tsdf_alloc", "tsdf_integrate", "tsdf_extract", "mesh_packed", "seed_view", "seed",
           "make_header", "to_device", "to_numpy", "SH_DIM"]
