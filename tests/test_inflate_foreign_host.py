"""decompressGzipped on members zlib's deflate never writes (tests/deflate_craft.py): other strategies, memory levels
and windows, flushes, codes of 15 bits, HLIT / HDIST at their extremes, blocks of 100 bytes and of 300 000 symbols, window
chains, every gzip header field — and members that are invalid in one chosen way, early in the member and past its middle.
The answer is zlib's, for every one; the parallel host reader (spz_amd/csrc/spz_inflate.cpp, members from 4 MiB, 8
threads) is never the one that accepted an invalid member, and takes the valid ones the project says it takes."""
import pytest

import deflate_craft as dc
import spz_amd.spz as spz
from test_parallel_inflate import eight_threads, parallel  # noqa: F401  (the fixture applies to every test here)

SIZE = (4 << 20) + 200_000          # over the parallel reader's 4 MiB
NAMES = dc.case_names([("host", SIZE)])

# Valid members the parallel reader must be the one to inflate: what tests/test_parallel_inflate.py already claims
# (sync flushes, a named member, other mtime / XFL / OS), and zlib's other strategies and memory levels from 4 up (dynamic
# blocks of a thousand symbols and more: isBlockStart finds them like any others).
PARALLEL = {"sync-flush", "headers-name-comment", "headers-mtime-xfl-os", "headers-plain", "strategy-filtered", "strategy-rle",
            "strategy-huffman-only", "memlevel-4", "memlevel-7"}
assert PARALLEL <= set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_foreign_member_gets_zlibs_verdict(name):
    kind, gz, want = dc.build(name, SIZE)           # (checked against zlib in there)
    got, used = parallel(gz)
    assert got == want, f"{name}: {'accepted' if got is not None else 'rejected'}, zlib {'accepts' if want is not None else 'rejects'}"
    if kind != "valid":
        assert not used, f"{name}: the parallel reader accepted it"
    print(f"{name}: {len(gz)} -> {None if want is None else len(want)} bytes, {'parallel reader' if used else 'serial readers'}")
    if name in PARALLEL:
        assert used, f"{name}: the parallel reader did not take it"
