"""CPU-side reference of ONE stream written in parts (flate_hip_one_writer_*; tests/test_one_writer_rule_model.py,
tests/test_one_writer_abi.py, tests/test_gpu_one_writer.py).  The whole stream and its index come from the oracle, the
way tests/spliced_framed_ref.py builds them: oracle.deflate_spliced over the pieces {0, P, 2P, ..., T}, oracle.frame
around it; Python's zlib / gzip must accept it.  From those and a list of part sizes follows what every call returns:
call j delivers whole[B_j, B_{j+1}) with B = header + (end bit of the pieces consumed so far >> 3), and everything on
the final call.  Nothing here comes from the code under test."""
import collections
import gzip
import zlib

import numpy as np

RAW, ZLIB, GZIP = 0, 1, 2
WRAP_NAME = {RAW: "raw", ZLIB: "zlib", GZIP: "gzip"}
HEADER = {RAW: 0, ZLIB: 2, GZIP: 10}
TRAILER = {RAW: 0, ZLIB: 4, GZIP: 8}
OK, STREAM_END, E_INVALID, E_OUT_TOO_SMALL, E_TOO_LARGE = 0, 1, -1, -2, -6
PIECE_DEFAULT = 65535
CLOSING = bytes([0x01, 0x00, 0x00, 0xff, 0xff])

# one call as the library reports it (bit_off: the k pieces' start bits, and on a final call the end bit), the bytes it
# delivers, and what the rule decides on the way: header / close, the scan's start bit in the call's buffer, the bits
# the consumed pieces span, the carry the handle keeps
Call = collections.namedtuple("Call", "rc in_used out_len n_pieces bit_off data in_len final header close start_bit span carry")


def piece_offsets(total, piece):
    """in_off of the whole call: {0, P, 2P, ..., T}, ceil(T / P) pieces."""
    piece = piece or PIECE_DEFAULT
    off = list(range(0, total, piece)) + [total]
    return np.array(off, dtype=np.uint64)


class Whole:
    """member = header | raw | trailer of `plain` cut every `piece` bytes; bit_off[n + 1] counted from raw's first byte
    (entry n: where the closing block starts)."""

    def __init__(self, oracle, plain, piece, wrap, compat="moonbit"):
        plain = bytes(plain)
        self.plain, self.piece, self.wrap = plain, piece or PIECE_DEFAULT, wrap
        self.hl, self.tl = HEADER[wrap], TRAILER[wrap]
        self.in_off = piece_offsets(len(plain), piece)
        self.n = self.in_off.size - 1
        if self.n:
            cm = oracle.COMPAT_GO if compat == "go" else oracle.COMPAT_MOONBIT
            src = np.frombuffer(plain, dtype=np.uint8)
            self.raw, bit_off = oracle.deflate_spliced(src, self.in_off, cm)
            self.bit_off = [int(b) for b in bit_off]
        else:  # nothing but the closing block of Writer::close
            self.raw, self.bit_off = CLOSING, [0]
        if wrap == RAW:
            self.member = self.raw
        else:
            self.member = oracle.frame(oracle.FRAME_ZLIB if wrap == ZLIB else oracle.FRAME_GZIP, self.raw, plain)
        assert self.member[self.hl:len(self.member) - self.tl] == self.raw
        # the closing block starts at the last entry: 3 bits, the padding, LEN, NLEN
        assert (self.bit_off[-1] + 3 + 7) // 8 + 4 == len(self.raw)
        assert self.inflate(self.member) == plain

    def inflate(self, member):
        if self.wrap == RAW:
            d = zlib.decompressobj(-15)
            out = d.decompress(bytes(member))
            assert d.eof and d.unused_data == b""
            return out
        return zlib.decompress(bytes(member)) if self.wrap == ZLIB else gzip.decompress(bytes(member))

    def calls(self, sizes):
        """sizes: the NEW bytes every call that is not final brings (the bytes the call before left unused stand in
        front of them); the final call brings the rest.  -> [Call]."""
        P, T, hl = self.piece, len(self.plain), self.hl
        out, fed, done, pieces, at = [], 0, 0, 0, 0  # bytes handed over, bytes consumed, pieces consumed, bytes delivered
        started = False
        plan = [(min(s, T - fed_), False) for s, fed_ in zip(sizes, _running(sizes, T))] + [(None, True)]
        for new, final in plan:
            fed = T if final else fed + new
            in_len = fed - done
            k = (in_len + P - 1) // P if final else in_len // P
            used = in_len if final else k * P
            if not final and k == 0:
                out.append(Call(OK, 0, 0, 0, [], b"", in_len, False, 0, 0, 0, 0, None))
                continue
            header = 0 if started else 1
            first_bit, end_bit = self.bit_off[pieces], self.bit_off[pieces + k]
            start_bit = 8 * hl if header else first_bit % 8
            if final:
                data, idx = self.member[at:], self.bit_off[pieces:pieces + k + 1]
            else:
                data, idx = self.member[at:hl + (end_bit >> 3)], self.bit_off[pieces:pieces + k]
            out.append(Call(STREAM_END if final else OK, used, len(data), k, idx, data, in_len, final, header, int(final),
                            start_bit, end_bit - first_bit, 0 if final else end_bit % 8))
            started, done, pieces, at = True, done + used, pieces + k, at + len(data)
        assert done == T and pieces == self.n and at == len(self.member)
        assert b"".join(c.data for c in out) == self.member
        assert [b for c in out for b in c.bit_off] == self.bit_off
        return out


def _running(sizes, total):
    fed = 0
    for s in sizes:
        yield fed
        fed = min(total, fed + s)


def bound(in_len, piece):
    """flate_hip_one_writer_bound as the header states it: every piece within flate_hip_deflate_bound of its length
    (2 n + 320 per window + 16), and 32 bytes for header, carried byte, closing block and trailer."""
    piece = piece or PIECE_DEFAULT
    pieces = in_len // piece + 1
    return 2 * in_len + 320 * (in_len // 65535 + pieces) + 16 * pieces + 32


def feed(write, plain, sizes):
    """Drive a writer the way a caller does: write(buf, final) -> (in_used, bytes, result); the unused bytes stand in
    front of the next call's.  -> [(in_used, bytes, result)]."""
    plain = bytes(plain)
    res, fed, done = [], 0, 0
    for s in list(sizes) + [None]:
        final = s is None
        fed = len(plain) if final else min(len(plain), fed + s)
        r = write(plain[done:fed], final)
        res.append(r)
        done += r[0]
    return res


# ---- part lists ----

def fixed(total, size):
    return [size] * (total // max(size, 1) + 1) if size else []


def growing(total, first=1, factor=3):
    out, s, fed = [], first, 0
    while fed < total:
        out.append(s)
        fed += s
        s *= factor
    return out


def random_sizes(total, mean, seed):
    rng = np.random.default_rng(seed)
    out, fed = [], 0
    while fed < total:
        s = int(rng.integers(0, 2 * mean + 1))
        out.append(s)
        fed += s
    return out
