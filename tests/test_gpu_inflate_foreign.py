"""The device inflate (spz_amd/csrc/spz_inflate_dev.hip) on members zlib's deflate never writes — the case table of
tests/deflate_craft.py, every member checked against zlib in there.  Hard, for every case: decompressGzipped gives zlib's
verdict.  For the valid ones also WHO gave it: a wrong decode is rescued by the CRC check and the host readers every time, so
only the counter shows a decoder path that never works.  Each case is on exactly one of two lists, written down from the
code before the first run on a device:

  ENGAGES       the device reader must be the one that inflated it;
  MAY_DECLINE   it may stand down, and then with exactly the reason given (at most 8 entries).

An invalid member gets zlib's error, and the device counter does not move."""
import os

import pytest

import deflate_craft as dc
import spz_amd.spz as spz

pytestmark = pytest.mark.gpu

# deviceInflateWanted (spz_host.cpp): forced, a member of header + 8 + 1 MiB and more; inflate_open_impl: 128 KiB of deflate
# data (4 x kMinChunkBytes) and more.  Just over both.
SIZE = (1 << 20) + 100_000
# Window chains (bytes of deflate data; a chunk is kMinChunkBytes = 32768 of them while there are fewer chunks than 95 % of
# the decode kernel's wave slots, 5593 on 256 CUs, and every chunk has a block start: a chain piece is 2.5 KiB).  The output
# is a 32 KiB seed repeated by matches of distance 32768 and nothing else, so every byte of chunk c is carried through c
# windows.  The matches are 3 bytes long, 15 bits each: 1.6 bytes out per byte in — at 258 bytes per match a chunk would
# expand 137-fold and the member would decline for its "expansion" (kExpand = 8) before any window is looked at.
# inf_window_resolve_kernel follows kChainSteps = 32 chunks per pass and the host gives it 64 passes: chains through
# 2048 chunks are resolved for certain; longer ones only as far as threads find entries that others have resolved
# in the same pass, which the order of execution decides.
CHAINS = [("short", 40 * 32768 + 5000), ("2040-chunks", 2040 * 32768 + 5000), ("2100-chunks", 2100 * 32768 + 5000)]
NAMES = dc.case_names(CHAINS)
CHAIN_SIZE = {f"window-chain-{k}": v for k, v in CHAINS}

# The device reader must be the one that inflates these.  Why, from the code:
#  strategy-filtered / -rle / -huffman-only, memlevel-4 / -7, wbits-*, sync-flush, full-flush, headers-*: dynamic blocks of
#    zlib's, a few KiB each, so every 32 KiB chunk's search finds a header (hasValidDynamicHeader) within its own bytes; the
#    empty stored blocks of a flush are blocks like any other to decodeBlocksWith (raw() of no bytes).  A header's FEXTRA,
#    name and comment are skipped by parseGzipHeader; an "SZ" subfield of another version or a length that does not fit its
#    count is not an index, and one that is well-formed but not this member's fails inflateIndexed's size check, after
#    which decompressGzippedWith asks the device reader as for any member.
#  stored-first: "(A member that opens with a stored block was declined until round 3 ...) it is decoded here now"
#    (inflate_open_impl); chunk 0 starts at bit 0 whatever the block type.
#  fixed-then-dynamic: chunk 0 walks the 300 KiB of fixed blocks (1.5 bytes out per byte in, kExpand allows 8); chunks that
#    start within kSearchBytes = 128 KiB of the first dynamic block find it, so there are two jobs and more.
#  long-codes(-deep): every symbol's fast-table entry is 0 -> F_MISS -> the serial L.lookup()/D.lookup() canonical walk;
#    the headers are complete codes, which is all the search asks.  3 bytes out per byte in.
#  one-dist-code(-deep), no-dist-codes: HuffT::build takes a set with no code and a single code of one bit.
#  hlit-hdist-extremes, repeat-across-boundary: readCodeLengths reads HLIT + HDIST lengths as one sequence (RFC 1951).
#  len258-two-ways, dist-32768(-deep), straddling-match: lenBase/lenExtra hold code 284 + 31; copy_at turns a source before
#    the chunk into 256 + W + src >= 256 (src >= -32768), resolved from the predecessor's window.
#  memlevel-1, tiny-blocks(-deep): blocks of ~100 bytes are ~80 true starts per batch of 65536 bit positions, and
#    look-alikes add 7.5 per 16384 (the kernel's own comment): about 110 candidates, under kMaxCand = 192 — and were
#    there more, the first valid one of those kept is still a true start, which is all a chunk needs; "ncand > kMaxCand"
#    only ends the search of a chunk that found none.  Region capacity: 8 symbols per byte + 95, under the budget's
#    + 128 per chunk.
#  huge-block: the chunks inside the 165 KiB block find no start of their own or the one behind it (found again: one
#    job); the job before takes the span and 8 x its bytes of symbols, the block needs 2 x.
#  window-chain-short, -2040-chunks: chains of up to 2048 chunks resolve within the 64 passes (above).
ENGAGES = {"strategy-filtered", "strategy-rle", "strategy-huffman-only", "memlevel-1", "memlevel-4", "memlevel-7", "wbits-9", "wbits-12",
           "full-flush", "sync-flush", "fixed-then-dynamic", "stored-first", "long-codes", "long-codes-deep", "one-dist-code",
           "one-dist-code-deep", "no-dist-codes", "hlit-hdist-extremes", "repeat-across-boundary", "len258-two-ways", "dist-32768",
           "dist-32768-deep", "straddling-match", "tiny-blocks", "tiny-blocks-deep", "huge-block", "window-chain-short",
           "window-chain-2040-chunks"} | {f"headers-{h}" for h in dc.HEADERS if h != "fhcrc"}
# ... and these may stand down, with this reason and no other:
MAY_DECLINE = {
    # Z_FIXED writes no dynamic block: no chunk's search finds a header, one job, "if (n < 2) return decline(...)".  (A
    # look-alike that passes the full header check would be dropped again by the linking rounds.)
    "strategy-fixed": "no-block-starts",
    # 2 MiB from 2 KiB of matches inside chunk 0, whose region holds 8 symbols per byte of its span:
    # "if (res[j].overflow) return decline("expansion");  // a chunk that expands more than 8 x"
    "rle-258": "expansion",
    # 2100 chunks: past what the 64 passes are certain to resolve: "bytes carried through more than 2048 chunks: the host readers"
    "window-chain-2100-chunks": "window-chains",
    # "FHCRC: zlib checks the header CRC16 ... such members go to zlib" (parseGzipHeader returns 0): the device reader is not
    # asked, so there is no reason of its own to read
    "headers-fhcrc": None,
}
assert len(MAY_DECLINE) <= 8 and not (ENGAGES & set(MAY_DECLINE))


@pytest.fixture(autouse=True)
def force_device_inflate():
    old = os.environ.get("SPZ_AMD_GUNZIP_DEVICE")
    os.environ["SPZ_AMD_GUNZIP_DEVICE"] = "1"
    yield
    if old is None:
        os.environ.pop("SPZ_AMD_GUNZIP_DEVICE", None)
    else:
        os.environ["SPZ_AMD_GUNZIP_DEVICE"] = old


@pytest.mark.parametrize("name", NAMES)
def test_foreign_member_on_the_device(name):
    kind, gz, want = dc.build(name, CHAIN_SIZE.get(name, SIZE))       # (checked against zlib in there)
    before = spz._device_inflate_count()
    got = spz._decompress_gzipped(gz)
    took = spz._device_inflate_count() - before
    reason = spz._device_inflate_last_decline()
    print(f"{name}: {len(gz)} -> {None if want is None else len(want)} bytes, {'device' if took else 'declined: ' + repr(reason)}")
    assert got == want, f"{name}: {'accepted' if got is not None else 'rejected'}, zlib {'accepts' if want is not None else 'rejects'}"
    if kind != "valid":
        assert took == 0, f"{name}: the device reader accepted it"
    elif name in ENGAGES:
        assert took == 1, f"{name}: the device did not inflate it ({reason!r})"
    else:
        assert name in MAY_DECLINE, f"{name} is on neither list"
        if MAY_DECLINE[name] is None:
            assert took == 0, f"{name}: a member whose header the fast readers do not start behind"
        else:
            assert took == 1 or reason == MAY_DECLINE[name], f"{name}: declined for {reason!r}, not {MAY_DECLINE[name]!r}"
