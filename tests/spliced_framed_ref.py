"""CPU-side fixtures of the spliced framed read tests (tests/test_gpu_inflate_spliced_framed.py,
tests/test_host_cpp_spliced_framed_read.py): one zlib stream or gzip member around the oracle's spliced stream, with
its index and the bytes every piece inflates to.  Everything comes from the CPU: oracle.deflate_spliced for the raw
stream and its index, oracle.frame for the member, oracle.inflate for what a reader of the raw stream produces;
Python's zlib / gzip must accept every member (a precondition, independent of the oracle)."""
import gzip
import zlib

import numpy as np

from test_splice import SPECS
from util import make_streams

HEADER = {"zlib": 2, "gzip": 10}
TRAILER = {"zlib": 4, "gzip": 8}


class Member:
    """member = header | raw | trailer; bit_off[n + 1] counted from raw's first byte; pieces[i] = piece i's bytes."""

    def __init__(self, oracle, specs, wrap, compat="moonbit", seed=13):
        data, off = make_streams(specs, seed=seed)
        cm = oracle.COMPAT_GO if compat == "go" else oracle.COMPAT_MOONBIT
        self.wrap = wrap
        self.raw, self.bit_off = oracle.deflate_spliced(data, off, cm)
        self.whole = data[:int(off[-1])].tobytes()
        self.member = oracle.frame(oracle.FRAME_ZLIB if wrap == "zlib" else oracle.FRAME_GZIP, self.raw, self.whole)
        self.hl, self.tl = HEADER[wrap], TRAILER[wrap]
        assert self.member[self.hl:len(self.member) - self.tl] == self.raw
        assert (zlib.decompress(self.member) if wrap == "zlib" else gzip.decompress(self.member)) == self.whole
        assert oracle.inflate(self.raw, len(self.whole)) == self.whole
        self.pieces = [self.whole[int(off[i]):int(off[i + 1])] for i in range(len(specs))]
        self.sizes = [len(p) for p in self.pieces]

    @property
    def trailer(self):
        return self.member[len(self.member) - self.tl:]


def fixture_members(oracle):
    """{(compat, wrap): Member} over test_splice's SPECS: stored tails of 1..16 bytes, Huffman-only, dynamic,
    multi-window and empty streams."""
    return {(c, w): Member(oracle, SPECS, w, c) for c in ("moonbit", "go") for w in ("zlib", "gzip")}


def many_pieces_specs(n=3000, seed=9):
    """n pieces of 0..300 bytes, a random third of them empty: more than one chunk of the join kernel's walk."""
    rng = np.random.default_rng(seed)
    kinds = ["text", "rand", "zero", "low"]
    return [(kinds[int(rng.integers(len(kinds)))], 0 if rng.integers(3) == 0 else int(rng.integers(1, 301)))
            for _ in range(n)]
