"""A test-side deflate WRITER (RFC 1951 / 1952): gzip members that are valid — or invalid in one chosen way — but that
zlib's deflate would never emit.  Every choice an encoder makes for itself is a parameter here: the block type, the code
lengths, HLIT / HDIST / HCLEN, how a length or distance is written, the block size, the gzip header.

A member is a gzip header, byte-aligned raw-deflate SEGMENTS and the trailer.  A segment is crafted (tokens -> bits, by
BitWriter below) or the output of one zlib.compressobj ended with a flush; the last one carries BFINAL.  The bulk that
lifts a member over a reader's size threshold comes from zlib, so the pure-Python writer only ever sees crafted segments.

The helper is trusted only through zlib: check() passes every member through zlib.decompressobj(31); a member meant to
be valid must give exactly the intended bytes, one meant to be invalid must be refused.  CASES is the one case table of
tests/test_inflate_foreign_host.py, tests/test_gpu_inflate_foreign.py and tools/inflate_coverage.py --foreign."""
import functools
import heapq
import struct
import zlib

import numpy as np

LEN_BASE = np.array([3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258])
LEN_EXTRA = np.array([0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0])
DIST_BASE = np.array([1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                      8193, 12289, 16385, 24577])
DIST_EXTRA = np.array([0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13])
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = np.array([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = np.array([5] * 32)


# ---- bits -------------------------------------------------------------------------------------------------------
class BitWriter:
    """Fields (value, width <= 16) in stream order, least significant bit first; packed once, with numpy."""

    def __init__(self):
        self._v, self._n, self._pv, self._pn = [], [], [], []
        self.nbits = 0

    def put(self, value, width):
        assert 0 <= width <= 16 and 0 <= value < (1 << width) or width == 0
        self._pv.append(value)
        self._pn.append(width)
        self.nbits += width

    def _flush(self):
        if self._pv:
            self._v.append(np.array(self._pv, np.int64))
            self._n.append(np.array(self._pn, np.int64))
            self._pv, self._pn = [], []

    def put_many(self, values, widths):
        self._flush()
        self._v.append(np.asarray(values, np.int64))
        self._n.append(np.asarray(widths, np.int64))
        self.nbits += int(self._n[-1].sum())

    def align(self):
        self.put(0, -self.nbits % 8)

    def put_bytes(self, b):
        assert self.nbits % 8 == 0
        self.put_many(np.frombuffer(b, np.uint8), np.full(len(b), 8))

    def bytes(self):
        self._flush()
        if not self._v:
            return b""
        v, n = np.concatenate(self._v), np.concatenate(self._n)
        off = np.cumsum(n) - n
        byte, x = off >> 3, v << (off & 7)            # < 2^23
        size = (self.nbits + 7) // 8
        out = np.zeros(size + 3)
        for k in range(3):                             # bits of different fields never meet: a sum is an or
            out += np.bincount(byte + k, weights=(x >> (8 * k)) & 255, minlength=size + 3)
        return out[:size].astype(np.uint8).tobytes()


def canonical_codes(lens):
    """Bit-reversed canonical codes (RFC 1951 3.2.2) of a list of code lengths; an over-subscribed set wraps."""
    return _canonical_codes(tuple(int(l) for l in lens))


@functools.lru_cache(maxsize=64)
def _canonical_codes(lens):
    lens = np.asarray(lens, np.int64)
    count = np.bincount(lens, minlength=16)
    count[0] = 0
    nxt, code = np.zeros(17, np.int64), 0
    for bits in range(1, 16):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    codes = np.zeros(len(lens), np.int64)
    for s in np.argsort(lens, kind="stable"):
        if lens[s]:
            codes[s] = nxt[lens[s]] & ((1 << lens[s]) - 1)
            nxt[lens[s]] += 1
    rev = np.zeros_like(codes)
    for b in range(15):
        rev |= ((codes >> b) & 1) << np.maximum(lens - 1 - b, 0) * (lens > b)
    return rev


def kraft(lens):
    return sum(1 << (15 - l) for l in lens if l)       # 32768 = complete


def limited_lengths(freq, limit):
    """Huffman code lengths for the symbols of non-zero frequency, none longer than `limit`; complete from two symbols
    on (Huffman, then the overflow moved down the way miniz does)."""
    freq = np.asarray(freq)
    used = [int(s) for s in np.nonzero(freq)[0]]
    lens = np.zeros(len(freq), np.int64)
    if len(used) == 1:
        lens[used[0]] = 1
        return lens
    heap = [(int(freq[s]), s, None, None) for s in used]
    heapq.heapify(heap)
    tie = len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], tie, a, b))
        tie += 1
    depth = {}
    stack = [(heap[0], 0)]
    while stack:
        (f, s, a, b), d = stack.pop()
        if a is None:
            depth[s] = d
        else:
            stack += [(a, d + 1), (b, d + 1)]
    count = np.zeros(limit + 1, np.int64)
    for d in depth.values():
        count[min(d, limit)] += 1
    total = sum(int(count[i]) << (limit - i) for i in range(1, limit + 1))
    while total > (1 << limit):
        count[limit] -= 1
        for i in range(limit - 1, 0, -1):
            if count[i]:
                count[i] -= 1
                count[i + 1] += 2
                break
        total -= 1
    order = sorted(used, key=lambda s: (-int(freq[s]), s))      # the most frequent get the shortest
    k = 0
    for l in range(1, limit + 1):
        for _ in range(int(count[l])):
            lens[order[k]] = l
            k += 1
    assert k == len(used) and kraft(lens) == 32768
    return lens


def long_lengths(freq, nsym):
    """Every USED symbol gets a code of 10 to 15 bits (one of 15 at least); the short codes, 1 to 9 bits, go to nine
    symbols the block never uses.  Complete.  No fast table of up to 9 bits holds a symbol of the block."""
    used = [int(s) for s in np.nonzero(np.asarray(freq)[:nsym])[0]]
    decoys = [s for s in range(nsym) if s not in used][:9]
    assert len(decoys) == 9 and 2 <= len(used) <= 60
    lens = np.zeros(len(freq), np.int64)
    for k, s in enumerate(decoys):
        lens[s] = k + 1
    units = {s: 1 for s in used}                             # of 2^-15; 64 are left
    grew = True
    while sum(units.values()) < 64 and grew:
        grew = False
        for s in sorted(used, key=lambda s: (-int(freq[s]), s))[:-1]:   # the rarest stays at 15 bits
            if units[s] < 32 and sum(units.values()) + units[s] <= 64:
                units[s] *= 2
                grew = True
                break
    for s in used:
        lens[s] = 15 - int(units[s]).bit_length() + 1
    assert kraft(lens) == 32768 and max(lens) == 15 and all(lens[s] >= 10 for s in used)
    return lens


# ---- tokens -----------------------------------------------------------------------------------------------------
class Tokens:
    """L[i], D[i]: literal byte L (D = 0) or a match of length L at distance D; ALT[i]: length 258 written as code 284
    with extra bits 31 instead of code 285."""

    def __init__(self, L=(), D=(), ALT=None):
        self.L, self.D = np.asarray(L, np.int64), np.asarray(D, np.int64)
        self.ALT = np.zeros(len(self.L), bool) if ALT is None else np.asarray(ALT, bool)

    def __len__(self):
        return len(self.L)

    def __add__(self, o):
        return Tokens(np.concatenate([self.L, o.L]), np.concatenate([self.D, o.D]), np.concatenate([self.ALT, o.ALT]))

    def slice(self, a, b):
        return Tokens(self.L[a:b], self.D[a:b], self.ALT[a:b])


def lits(data):
    a = np.frombuffer(bytes(data), np.uint8)
    return Tokens(a, np.zeros(len(a), np.int64))


def match(length, dist, alt=False, times=1):
    assert 3 <= length <= 258 and 1 <= dist <= 32768 and (not alt or length == 258)
    return Tokens([length] * times, [dist] * times, [alt] * times)


def expand(tok, history=b""):
    """What the tokens stand for, after `history` (the member's output so far)."""
    out = bytearray(history)
    base = len(out)
    at = 0
    for i in np.nonzero(tok.D)[0]:
        out += tok.L[at:i].astype(np.uint8).tobytes()
        l, d = int(tok.L[i]), int(tok.D[i])
        assert d <= len(out), "a distance further back than the output"
        if d >= l:
            out += out[len(out) - d:len(out) - d + l]
        else:
            out += (bytes(out[-d:]) * (l // d + 1))[:l]
        at = i + 1
    out += tok.L[at:].astype(np.uint8).tobytes()
    return bytes(out[base:])


def _symbols(tok):
    is_m = tok.D > 0
    li = np.searchsorted(LEN_BASE, tok.L, "right") - 1
    li = np.where(tok.ALT, 27, np.where(is_m, li, 0))
    di = np.where(is_m, np.searchsorted(DIST_BASE, np.maximum(tok.D, 1), "right") - 1, 0)
    return is_m, np.where(is_m, 257 + li, tok.L), li, di


def frequencies(tok):
    is_m, sym, li, di = _symbols(tok)
    lf = np.bincount(sym, minlength=286)
    lf[256] += 1
    return lf, np.bincount(di[is_m], minlength=30)


def put_tokens(bw, tok, lit_lens, dist_lens):
    if not len(tok):
        return
    is_m, sym, li, di = _symbols(tok)
    lit_lens, dist_lens = np.asarray(lit_lens), np.asarray(dist_lens)
    lc, dc = canonical_codes(lit_lens), canonical_codes(dist_lens)
    assert (lit_lens[sym] > 0).all() and (dist_lens[di[is_m]] > 0).all(), "a token without a code"
    v, n = np.zeros((len(tok), 4), np.int64), np.zeros((len(tok), 4), np.int64)
    v[:, 0], n[:, 0] = lc[sym], lit_lens[sym]
    v[:, 1], n[:, 1] = np.where(is_m, tok.L - LEN_BASE[li], 0), np.where(is_m, LEN_EXTRA[li], 0)
    v[:, 2], n[:, 2] = np.where(is_m, dc[di], 0), np.where(is_m, dist_lens[di], 0)
    v[:, 3], n[:, 3] = np.where(is_m, tok.D - DIST_BASE[di], 0), np.where(is_m, DIST_EXTRA[di], 0)
    bw.put_many(v.ravel(), n.ravel())


# ---- blocks -----------------------------------------------------------------------------------------------------
def stored_block(bw, data, final=False, nlen=None):
    assert len(data) < 65536
    bw.put(int(final), 1)
    bw.put(0, 2)
    bw.align()
    bw.put(len(data), 16)
    bw.put(len(data) ^ 0xffff if nlen is None else nlen, 16)
    if data:
        bw.put_bytes(data)


def fixed_block(bw, tok, final=False, eob=True):
    bw.put(int(final), 1)
    bw.put(1, 2)
    put_tokens(bw, tok, FIXED_LIT, FIXED_DIST)
    if eob:
        bw.put(int(canonical_codes(FIXED_LIT)[256]), 7)


def rle(lens):
    """Code-length symbols (symbol, extra value) of a run of code lengths, with the repeat codes 16 / 17 / 18."""
    out, i, n = [], 0, len(lens)
    while i < n:
        v, j = int(lens[i]), i
        while j < n and lens[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                r = min(run, 138)
                out.append((18, r - 11))
                run -= r
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                r = min(run, 6)
                out.append((16, r - 3))
                run -= r
        out += [(v, 0)] * run
        i = j
    return out


CL_EXTRA = {16: 2, 17: 3, 18: 7}
CL7_PROFILE = [2, 2, 3] + [5] * 9 + [6] * 5 + [7] * 2          # 19 lengths, complete, two of 7 bits


def dynamic_block(bw, tok, final=False, lit_lens=None, dist_lens=None, mode=None, hlit=None, hdist=None, hclen=None,
                  cl_lens=None, cl_syms=None, cl7=False, cross=False, eob=True):
    """One dynamic block.  lit_lens / dist_lens: the caller's, or built from the tokens (mode "long": every used symbol
    10 to 15 bits).  hlit / hdist: sent counts (default: up to the last used).  cl_syms: the caller's code-length symbols
    (symbol, extra); cl_lens: the caller's code-length code; cl7: one whose rarest entries are 7 bits long; cross: repeat
    codes may run from the literal/length lengths into the distance lengths (zlib codes the two sets apart)."""
    lf, df = frequencies(tok)
    if lit_lens is None:
        if lf[:256].sum() == 0:
            lf[0] += 1                                  # two literal/length codes at least: a complete code
        lit_lens = long_lengths(lf, 286) if mode == "long" else limited_lengths(lf, 15)
    if dist_lens is None:
        if df.sum() == 0:
            dist_lens = np.zeros(30, np.int64)          # no distance codes: HDIST = 1, its one length 0
        elif mode == "long" and np.count_nonzero(df) >= 2:
            dist_lens = long_lengths(df, 30)
        else:
            dist_lens = limited_lengths(df, 15)
    lit_lens, dist_lens = np.asarray(lit_lens, np.int64), np.asarray(dist_lens, np.int64)
    if hlit is None:
        hlit = max(257, int(np.nonzero(lit_lens)[0].max()) + 1)
    if hdist is None:
        hdist = max(1, int(np.nonzero(dist_lens)[0].max()) + 1) if dist_lens.any() else 1
    ll = np.concatenate([lit_lens, np.zeros(288, np.int64)])[:hlit]
    dl = np.concatenate([dist_lens, np.zeros(32, np.int64)])[:hdist]
    if cl_syms is None:
        cl_syms = rle(np.concatenate([ll, dl])) if cross else rle(ll) + rle(dl)
    if cl_lens is None:
        cf = np.bincount([s for s, _ in cl_syms], minlength=19)
        if cl7:
            cl_lens = np.zeros(19, np.int64)
            for k, s in enumerate(sorted(range(19), key=lambda s: (-int(cf[s]), s))):
                cl_lens[s] = CL7_PROFILE[k]
        else:
            if np.count_nonzero(cf) == 1:
                cf[(int(np.nonzero(cf)[0][0]) + 1) % 19] += 1      # a complete code needs two
            cl_lens = limited_lengths(cf, 7)
    cl_lens = np.asarray(cl_lens, np.int64)
    if hclen is None:
        hclen = max(4, max(k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]))
    bw.put(int(final), 1)
    bw.put(2, 2)
    bw.put(hlit - 257, 5)
    bw.put(hdist - 1, 5)
    bw.put(hclen - 4, 4)
    for k in range(hclen):
        bw.put(int(cl_lens[CL_ORDER[k]]), 3)
    cc = canonical_codes(cl_lens)
    for s, extra in cl_syms:
        assert cl_lens[s] > 0
        bw.put(int(cc[s]), int(cl_lens[s]))
        if s >= 16:
            bw.put(extra, CL_EXTRA[s])
    put_tokens(bw, tok, lit_lens, dist_lens)
    if eob:
        bw.put(int(canonical_codes(lit_lens)[256]), int(lit_lens[256]))
    return lit_lens, dist_lens, cl_syms


def end_segment(bw, final=False):
    """The segment's bytes.  One that is not the last ends with an empty stored block (no flush went before it): the
    next segment starts on a byte boundary."""
    if not final:
        stored_block(bw, b"")
    bw.align()
    return bw.bytes()


def zseg(data, level=6, mem=9, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15, final=False, flush=zlib.Z_SYNC_FLUSH):
    co = zlib.compressobj(level, zlib.DEFLATED, -wbits, mem, strategy)
    return co.compress(data) + co.flush(zlib.Z_FINISH if final else flush)


# ---- gzip -------------------------------------------------------------------------------------------------------
def gzip_header(extra=None, name=None, comment=None, hcrc=None, mtime=0, xfl=0, os_=3, reserved=0):
    """extra: the FEXTRA field's bytes; hcrc: None, "right" or "wrong"; reserved: FLG bits 5-7."""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0) | reserved
    h = struct.pack("<BBBBIBB", 0x1f, 0x8b, 8, flg, mtime, xfl, os_)
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", (zlib.crc32(h) & 0xffff) ^ (0 if hcrc == "right" else 0x0100))
    return h


def sz_subfield(version, claimed, sizes):
    """An FEXTRA subfield with the "SZ" id of the project's own piece index: version, block bytes, total bytes, the
    number of pieces it claims and `sizes` piece sizes (consistent when claimed == sizes)."""
    body = struct.pack("<IIQI", version, 65536, 123456, claimed) + b"".join(struct.pack("<I", 1000 + k) for k in range(sizes))
    return b"SZ" + struct.pack("<H", len(body)) + body


def member(segments, data, header=None):
    return (gzip_header() if header is None else header) + b"".join(segments) + struct.pack("<II", zlib.crc32(data), len(data) & 0xffffffff)


def zlib_verdict(b):
    """(bytes or None, bytes left over after the member, zlib's complaint)"""
    d = zlib.decompressobj(31)
    try:
        out = d.decompress(b)
    except zlib.error as e:
        return None, b"", str(e).split(": ", 1)[-1]
    return (out, d.unused_data, "") if d.eof else (None, b"", "truncated")


def check(kind, gz, want, why=None):
    """The self-check: zlib's verdict on the member is the intended one (an invalid one is refused, and for the reason it
    was built for).  Returns what a reader must return."""
    got, rest, said = zlib_verdict(gz)
    if kind == "valid":
        assert got is not None and got == want and rest == b"", "the helper wrote a member zlib does not read as intended"
    elif kind == "invalid":
        assert got is None, "the helper meant this member to be invalid and zlib accepts it"
        assert why is None or said == why, f"zlib refuses it for another reason: {said!r}, not {why!r}"
    else:                                                   # "trailing": a valid member and more bytes behind it
        assert got == want and rest != b""
    return got


# ---- the cases --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def texture(n, seed=5):
    """Bucketed values around 128, like the sh section of a stream: dynamic blocks of literals and short matches."""
    rng = np.random.default_rng(seed)
    return np.clip(np.round(rng.normal(128, 20, n) / 8) * 8, 0, 255).astype(np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def zlib_bulk(target, final, seed=5, **kw):
    """(data, segment): one zlib segment of `target` compressed bytes at least."""
    if target <= 0:
        return b"", (zseg(b"", final=True) if final else b"")
    ratio = len(zseg(texture(1 << 18, seed), **kw)) / (1 << 18)
    n = int(target / ratio * 1.04) + 4096
    while True:
        data = texture(n, seed)
        seg = zseg(data, final=final, **kw)
        if len(seg) >= target:
            return data, seg
        n = n * 5 // 4


def around(craft, size, deep=False, lead=20000):
    """lead | crafted | fill: the crafted segment(s) early (behind `lead` bytes of zlib's, which they may reference) or,
    deep, past the middle of the member.  craft(history) -> (segments' bytes, their output, or None when the segment
    is invalid)."""
    if deep:
        a_data, a_seg = zlib_bulk(size * 11 // 20, False, level=1)
    else:
        a_data, a_seg = (texture(lead, 9), zseg(texture(lead, 9))) if lead else (b"", b"")
    seg, out = craft(a_data)
    b_data, b_seg = zlib_bulk(-(-(size - len(a_seg) - len(seg) + 64) // 65536) * 65536, True, seed=6, level=1)
    return member([a_seg, seg, b_seg], a_data + (out or b"") + b_data), a_data + (out or b"") + b_data


def nibbles(n, seed):
    return np.random.default_rng(seed).integers(0, 16, n, dtype=np.uint8).tobytes()


def crafted(blocks):
    """craft(history) from a function (bw, history) -> tokens-in-order list, or the output bytes"""
    def craft(history):
        bw = BitWriter()
        out = blocks(bw, history)
        return end_segment(bw), out
    return craft


LONG_DISTANCES = [1, 7, 40, 150, 600, 1100, 2500, 9000, 4100, 5000, 7000, 13000]     # eleven distance codes


def _long_codes(bw, hist):
    # literals and matches (into the segment before, too) under codes of 10 to 15 bits, code-length code of 7 bits
    rng = np.random.default_rng(3)
    out = b""
    for k in range(6):
        tok = Tokens()
        for j in range(40):
            tok = tok + lits(nibbles(400, 100 * k + j)) + match(int(rng.integers(3, 259)), int(rng.choice(LONG_DISTANCES))) + \
                match(3, int(rng.choice(LONG_DISTANCES[-4:])))
        dynamic_block(bw, tok, mode="long", cl7=True)
        out += expand(tok, hist + out)
    return out


def _one_dist_code(bw, hist):
    a = lits(nibbles(3000, 1))                                                   # HLIT = 257, one unused 1-bit distance code
    dynamic_block(bw, a, hlit=257, hdist=1, dist_lens=[1])
    b = Tokens()
    for j in range(200):                                                         # matches, all of distance code 10 (33 .. 48)
        b = b + lits(nibbles(20, j)) + match(3 + j, 33 + j % 16)
    _, dl, _ = dynamic_block(bw, b)
    assert list(np.nonzero(dl)[0]) == [10] and dl[10] == 1
    return expand(a + b, hist)


def _no_dist_codes(bw, hist):
    out = b""
    for k in range(8):
        data = nibbles(9000, 50 + k)
        dynamic_block(bw, lits(data), hdist=1, dist_lens=[0])
        out += data
    return out


def _extremes(bw, hist):
    tok = lits(nibbles(5000, 7)) + match(17, 300) + lits(bytes(range(200))) + match(100, 5000)
    dynamic_block(bw, tok, hlit=286, hdist=30)                                  # all 316 lengths sent, the last ones zero
    tok2 = lits(nibbles(5000, 8))
    dynamic_block(bw, tok2, hlit=286, hdist=30, hclen=19)
    return expand(tok + tok2, hist)


def _repeat_across(bw, hist):
    # literal/length lengths that end as the distance lengths begin: one repeat code 16 covers the last of the one and
    # the first of the other.  Symbols 0 .. 15 and 256 .. 259 at 5 bits (20 codes), 260 .. 283 at 6 (24): 20/32 + 24/64 = 1.
    lit = np.zeros(286, np.int64)
    lit[0:16] = 5
    lit[256:260] = 5
    lit[260:284] = 6
    dist = np.array([6] * 4 + [4] * 15, np.int64)                                # 4/64 + 15/16 = 1
    tok = Tokens()
    for j in range(300):
        tok = tok + lits(nibbles(30, 300 + j)) + match(3 + j % 200, 1 + j)
    _, _, syms = dynamic_block(bw, tok, lit_lens=lit, dist_lens=dist, hlit=284, hdist=19, cross=True)
    n = 0
    crossing = False
    for s, e in syms:
        r = 1 if s < 16 else (3 + e if s < 18 else 11 + e)
        crossing |= n < 284 < n + r and s == 16
        n += r
    assert crossing and n == 284 + 19
    return expand(tok, hist)


def _len258(bw, hist):
    tok = lits(nibbles(600, 11))
    for j in range(120):
        tok = tok + match(258, 300 + j, alt=bool(j % 2)) + lits(nibbles(5, j))
    dynamic_block(bw, tok)
    fixed_block(bw, tok)
    return expand(tok + tok, hist)


def _dist_32768(bw, hist):
    # needs 32768 bytes before it: 40000 literals first, then matches at the window's far edge and, three bytes long,
    # at distances zlib's TOO_FAR never allows
    seed = lits(np.random.default_rng(4).integers(0, 256, 40000, dtype=np.uint8).tobytes())
    dynamic_block(bw, seed)
    tok = Tokens()
    for j in range(300):
        tok = tok + match(3 + j % 256, 32768) + match(3, 4097 + 90 * j) + lits(nibbles(7, j)) + match(258, 32768 - j)
    dynamic_block(bw, tok)
    fixed_block(bw, tok)
    return expand(seed + tok + tok, hist)


def _straddle(bw, hist):
    # the first match starts 100 bytes before the previous segment's end and goes on through its own first 158 bytes;
    # the second copies 100 bytes of the previous segment and the 100 that follow them here
    tok = match(258, 100) + lits(nibbles(3000, 12)) + match(200, 3258 + 100)
    dynamic_block(bw, tok)
    return expand(tok, hist)


def _rle_258(bw, hist):
    tok = lits(b"\x5a") + match(258, 1, times=(2 << 20) // 258)
    dynamic_block(bw, tok)
    return expand(tok, hist)


def _tiny_blocks(bw, hist):
    # ~100-byte dynamic blocks (100 literals of 16 values: a 40-byte header and 50 bytes of codes), 256 KiB of them;
    # every eighth is empty (end-of-block only), dynamic or fixed in turn, and now and then an empty stored block
    out, k = b"", 0
    lens = limited_lengths(frequencies(lits(bytes(range(16)) * 9 + b"\0\1\2"))[0], 15)     # caller-supplied: one code for all
    while bw.nbits < 8 * (256 << 10):
        data = nibbles(100, 1000 + k)
        dynamic_block(bw, lits(data), lit_lens=lens, dist_lens=[0], hdist=1)
        out += data
        if k % 8 == 0:
            dynamic_block(bw, Tokens()) if k % 16 else fixed_block(bw, Tokens())
        if k % 50 == 0:
            stored_block(bw, b"")
        k += 1
    return out


def _huge_block(bw, hist):
    data = nibbles(330_000, 13)
    tok = lits(data[:165_000]) + match(258, 32768) + lits(data[165_000:])
    dynamic_block(bw, tok)
    return expand(tok, hist)


CHAIN_MATCH = 3          # length of the chain's matches: 15 bits for 3 bytes, an expansion of 1.6


@functools.lru_cache(maxsize=None)
def _chain_piece():
    """One byte-aligned segment of nothing but matches at distance 32768 (a dynamic block of two literal/length codes and
    one distance code, then an empty stored block): 2 KiB of deflate data that repeat the 4092 bytes 32 KiB back."""
    bw = BitWriter()
    dynamic_block(bw, match(CHAIN_MATCH, 32768, times=1364))
    return end_segment(bw), 1364 * CHAIN_MATCH


def window_chain(deflate_bytes):
    """A 32 KiB random seed (stored), then only matches of distance 32768: every byte of the output is carried unchanged
    through every 32 KiB of it, and — at 1.6 bytes out per byte in — through every chunk of compressed bytes."""
    seed = np.random.default_rng(8).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    bw = BitWriter()
    stored_block(bw, seed)
    piece, n_out = _chain_piece()
    reps = max(1, (deflate_bytes - 32768) // len(piece))
    total = reps * n_out
    data = seed + (seed * (total // 32768 + 1))[:total]
    last = BitWriter()
    stored_block(last, b"", final=True)
    return member([end_segment(bw), piece * reps, end_segment(last, final=True)], data), data


def _whole(size, flushes=None, **kw):
    """One zlib stream of `size` compressed bytes at least; flushes: (kind, every-so-many input bytes)."""
    wb = kw.pop("wbits", 15)
    n = int(size * 1.06 / (len(zseg(texture(1 << 18), wbits=wb, **kw)) / (1 << 18))) + 4096
    while True:
        data = texture(n)
        co = zlib.compressobj(kw.get("level", 6), zlib.DEFLATED, -wb, kw.get("mem", 9), kw.get("strategy", zlib.Z_DEFAULT_STRATEGY))
        if flushes:
            seg = b"".join(co.compress(data[i:i + flushes[1]]) + co.flush(flushes[0]) for i in range(0, n, flushes[1])) + co.flush()
        else:
            seg = co.compress(data) + co.flush()
        if len(seg) >= size:
            return member([seg], data), data
        n = n * 5 // 4


def _prefixed(first, size):
    data, seg = first
    b_data, b_seg = zlib_bulk(size - len(seg) + 64, True, seed=6, level=6)
    return member([seg, b_seg], data + b_data), data + b_data


HEADERS = {
    "plain": dict(),
    "mtime-xfl-os": dict(mtime=1_700_000_000, xfl=2, os_=255),
    "name-comment": dict(name=b"scene.bin", comment=b"written elsewhere"),
    "extra-foreign": dict(extra=b"AP\x04\x00abcd"),
    "extra-sz-wrong-version": dict(extra=sz_subfield(2, 3, 3)),
    "extra-sz-wrong-length": dict(extra=sz_subfield(1, 5, 2)),
    "extra-sz-wrong-pieces": dict(extra=b"AP\x01\x00z" + sz_subfield(1, 2, 2)),      # well-formed, and not this member's
    "everything": dict(extra=b"AP\x02\x00xy", name=b"n", comment=b"c", mtime=7, xfl=4, os_=11),
    "fhcrc": dict(hcrc="right", name=b"with a header crc"),
}


def _headers(which, size):
    data, seg = zlib_bulk(size, True, seed=6, level=6)
    return member([seg], data, gzip_header(**HEADERS[which])), data


# -- invalid constructs: craft(history) -> (segment, None)
def _raw(fn):
    def craft(history):
        bw = BitWriter()
        out = fn(bw, history)
        return end_segment(bw), out if isinstance(out, bytes) else None
    return craft


def _bad_distance(bw, hist):           # (behind `lead` bytes of output only: further back than there is any)
    dynamic_block(bw, lits(nibbles(500, 1)) + match(10, len(hist) + 500 + 1000))


def _fixed_raw(sym=None, dist=None):
    def fn(bw, hist):
        bw.put(0, 1)
        bw.put(1, 2)
        put_tokens(bw, lits(nibbles(200, 2)), FIXED_LIT, FIXED_DIST)
        if sym is not None:
            bw.put(int(canonical_codes(FIXED_LIT)[sym]), 8)
        else:
            bw.put(int(canonical_codes(FIXED_LIT)[260]), 7)          # length 6
            bw.put(int(canonical_codes(FIXED_DIST)[dist]), 5)
        put_tokens(bw, lits(nibbles(200, 3)), FIXED_LIT, FIXED_DIST)
        bw.put(0, 7)
    return fn


def _lens_case(lit=None, cl_lens=None, cl_syms=None, eob=True):
    def fn(bw, hist):
        tok = lits(b"\0\1" * 50)
        if cl_syms is not None:
            dynamic_block(bw, tok, lit_lens=_two_plus_eob(), dist_lens=[0], hlit=257, hdist=1, cl_syms=cl_syms, cl_lens=cl_lens)
        else:
            dynamic_block(bw, tok, lit_lens=lit if lit is not None else _two_plus_eob(), dist_lens=[0], hdist=1, cl_lens=cl_lens, eob=eob)
    return fn


def _two_plus_eob(a=1, b=2, e=2):
    l = np.zeros(286, np.int64)
    l[0], l[1], l[256] = a, b, e
    return l


def _one_long_dist_code(bw, hist):
    # A single distance code of TWO bits.  RFC 1951 allows one distance code "of one bit"; zlib refuses any other
    # incomplete set.  The block is otherwise sound and the trailer's CRC-32 is that of what it would stand for, so a
    # reader that takes the code gives bytes where zlib gives an error.
    tok = lits(nibbles(300, 6))
    for j in range(50):
        tok = tok + match(4 + j, 1) + lits(nibbles(9, j))
    dynamic_block(bw, tok, dist_lens=[2], hdist=1)
    return expand(tok, hist)


# construct -> (writer, zlib's complaint)
INVALID = {
    "one-dist-code-of-two-bits": (_one_long_dist_code, "invalid distances set"),
    "oversubscribed-lit": (_lens_case(lit=_two_plus_eob(1, 1, 1)), "invalid literal/lengths set"),
    "incomplete-lit": (_lens_case(lit=_two_plus_eob(2, 2, 2)), "invalid literal/lengths set"),
    "incomplete-cl": (_lens_case(cl_lens=[2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3]), "invalid code lengths set"),
    "no-eob-code": (_lens_case(lit=_two_plus_eob(1, 1, 0), eob=False), "invalid code -- missing end-of-block"),
    "repeat-without-previous": (_lens_case(cl_syms=[(16, 0), (1, 0), (2, 0), (18, 127), (18, 92), (2, 0), (0, 0)],
                                          cl_lens=[2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 3]), "invalid bit length repeat"),
    "repeat-overruns": (_lens_case(cl_syms=[(1, 0), (2, 0), (18, 127), (18, 105), (2, 0), (18, 0)],
                                  cl_lens=[0, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1]), "invalid bit length repeat"),
    "lit-286": (_fixed_raw(sym=286), "invalid literal/length code"),
    "lit-287": (_fixed_raw(sym=287), "invalid literal/length code"),
    "dist-30": (_fixed_raw(dist=30), "invalid distance code"),
    "dist-31": (_fixed_raw(dist=31), "invalid distance code"),
    "stored-len-nlen": (lambda bw, hist: stored_block(bw, nibbles(2000, 4), nlen=0x1234), "invalid stored block lengths"),
    "block-type-3": (lambda bw, hist: (bw.put(0, 1), bw.put(3, 2), bw.put_many(np.frombuffer(nibbles(300, 5), np.uint8), np.full(300, 8))), "invalid block type"),
}


WHY = {"bad-distance-first-block": "invalid distance too far back", "bad-distance-behind-full-flush": "invalid distance too far back",
       "bad-fhcrc": "header crc mismatch", "bad-reserved-flg": "unknown header flags set"}      # case -> zlib's complaint


def _case_table():
    T = {}                      # name -> (kind, build(size) -> (member, intended bytes))
    for s, z in (("filtered", zlib.Z_FILTERED), ("rle", zlib.Z_RLE), ("huffman-only", zlib.Z_HUFFMAN_ONLY), ("fixed", zlib.Z_FIXED)):
        T[f"strategy-{s}"] = ("valid", functools.partial(_whole, strategy=z))
    for m in (1, 4, 7):
        T[f"memlevel-{m}"] = ("valid", functools.partial(_whole, mem=m))
    for w in (9, 12):
        T[f"wbits-{w}"] = ("valid", functools.partial(_whole, wbits=w))
    T["sync-flush"] = ("valid", functools.partial(_whole, flushes=(zlib.Z_SYNC_FLUSH, 65536)))
    T["full-flush"] = ("valid", functools.partial(_whole, flushes=(zlib.Z_FULL_FLUSH, 1 << 20)))
    T["fixed-then-dynamic"] = ("valid", lambda size: _prefixed(zlib_bulk(300 << 10, False, strategy=zlib.Z_FIXED), size))
    T["stored-first"] = ("valid", lambda size: _prefixed((nibbles(100_000, 1), zseg(nibbles(100_000, 1), level=0)), size))
    for name, fn in (("long-codes", _long_codes), ("one-dist-code", _one_dist_code), ("no-dist-codes", _no_dist_codes),
                     ("hlit-hdist-extremes", _extremes), ("repeat-across-boundary", _repeat_across), ("len258-two-ways", _len258),
                     ("dist-32768", _dist_32768), ("straddling-match", _straddle), ("rle-258", _rle_258), ("tiny-blocks", _tiny_blocks),
                     ("huge-block", _huge_block)):
        T[name] = ("valid", functools.partial(lambda size, fn: around(crafted(fn), size), fn=fn))
        if name in ("long-codes", "one-dist-code", "dist-32768", "tiny-blocks"):       # ... and where a chunk's wave meets them
            T[name + "-deep"] = ("valid", functools.partial(lambda size, fn: around(crafted(fn), size, deep=True), fn=fn))
    for h in HEADERS:
        T[f"headers-{h}"] = ("valid", functools.partial(_headers, h))
    # invalid: each construct in the first 64 KiB of the deflate data and past the member's middle
    for name, (fn, why) in INVALID.items():
        for deep in (False, True):
            T[f"bad-{name}-{'deep' if deep else 'early'}"] = ("invalid", functools.partial(lambda size, fn, deep: around(_raw(fn), size, deep=deep), fn=fn, deep=deep))
            WHY[f"bad-{name}-{'deep' if deep else 'early'}"] = why
    # a distance further back than the output so far exists only while the output is short: in the first block, and right
    # behind a Z_FULL_FLUSH that ends a short first segment (no deep placement: past 32 KiB every distance is in reach)
    T["bad-distance-first-block"] = ("invalid", lambda size: around(_raw(_bad_distance), size, lead=0))
    T["bad-distance-behind-full-flush"] = ("invalid", lambda size: _behind_full_flush(size))
    T["bad-fhcrc"] = ("invalid", lambda size: _bad_header(size, hcrc="wrong"))
    T["bad-reserved-flg"] = ("invalid", lambda size: _bad_header(size, reserved=0x20))
    T["then-second-member"] = ("trailing", lambda size: _trailing(size, None))
    T["then-garbage"] = ("trailing", lambda size: _trailing(size, nibbles(5000, 77)))
    return T


def _behind_full_flush(size):
    a = texture(3000, 9)
    a_seg = zseg(a, flush=zlib.Z_FULL_FLUSH)
    seg, _ = _raw(_bad_distance)(a)
    b_data, b_seg = zlib_bulk(size, True, seed=6, level=1)
    return member([a_seg, seg, b_seg], a + b_data), a + b_data


def _bad_header(size, **kw):
    data, seg = zlib_bulk(size, True, seed=6, level=6)
    return member([seg], data, gzip_header(**kw)), data


def _trailing(size, tail):
    data, seg = zlib_bulk(size, True, seed=6, level=6)
    m = member([seg], data)
    return m + (m if tail is None else tail), data


CASES = _case_table()


@functools.lru_cache(maxsize=4)
def build(name, size):
    """(kind, member, what a reader must return: the bytes, or None) of a case, for a member of `size` bytes at least
    (the window chains: `size` bytes of deflate data).  Checked against zlib before it is returned."""
    if name.startswith("window-chain-"):
        kind, (gz, data) = "valid", window_chain(size)
    else:
        kind, fn = CASES[name]
        gz, data = fn(size)
        assert len(gz) >= size, (name, len(gz), size)
    return kind, gz, check(kind, gz, data, WHY.get(name))


def case_names(chain_sizes=()):
    """Every case of the table, and a window chain for each (name suffix, bytes of deflate data) asked for."""
    return list(CASES) + [f"window-chain-{k}" for k, _ in chain_sizes]


if __name__ == "__main__":      # python tests/deflate_craft.py DIR [member bytes]: every member as a file (tools/fuzz/inflate_foreign.cpp)
    import os
    import sys
    size = int(sys.argv[2]) if len(sys.argv) > 2 else (4 << 20) + 200_000
    os.makedirs(sys.argv[1], exist_ok=True)
    for name in list(CASES) + ["window-chain-x"]:
        with open(os.path.join(sys.argv[1], name + ".gz"), "wb") as f:
            f.write(build(name, size)[1])
