"""What flate_hip_deflate_fast_grouped_framed must write, built from what the project already trusts: for every
group the container's header, pyoracle.deflate_spliced over the group's pieces, and the trailer from zlib's checksums.
The index slices are the oracle's bit_off.  Shared by tests/test_grouped_ref.py (CPU) and tests/test_gpu_grouped.py."""
import struct
import zlib

import numpy as np

from oracle import pyoracle

ZLIB_HEADER = b"\x78\x01"
GZIP_HEADER = b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x04\xff"
HEADERS = {"raw": b"", "zlib": ZLIB_HEADER, "gzip": GZIP_HEADER}


def trailer(wrap, data):
    data = bytes(data)
    if wrap == "zlib":
        return struct.pack(">I", zlib.adler32(data) & 0xffffffff)
    if wrap == "gzip":
        return struct.pack("<II", zlib.crc32(data) & 0xffffffff, len(data) & 0xffffffff)
    return b""


def compat_of(compat_go):
    return pyoracle.COMPAT_GO if compat_go else pyoracle.COMPAT_MOONBIT


class Expect:
    """One input, one layout, one compat mode: the groups' spliced streams (computed once) and, per wrap, the members."""

    def __init__(self, data, in_off, group_off, compat_go=False):
        self.data = np.ascontiguousarray(data, dtype=np.uint8)
        self.in_off = np.ascontiguousarray(in_off, dtype=np.uint64)
        self.group_off = np.ascontiguousarray(group_off, dtype=np.uint32)
        self.compat_go = compat_go
        self.n_pieces = self.in_off.size - 1
        self.n_groups = self.group_off.size - 1
        self.inputs, self.raws, bit_off = [], [], []
        off = [int(x) for x in self.in_off]
        for g in range(self.n_groups):
            lo, hi = int(self.group_off[g]), int(self.group_off[g + 1])
            base = off[lo]
            sub = self.data[base:off[hi]]
            rel = np.array([x - base for x in off[lo:hi + 1]], dtype=np.uint64)
            raw, bits = pyoracle.deflate_spliced(sub, rel, compat_of(compat_go))
            self.inputs.append(sub.tobytes())
            self.raws.append(bytes(raw))
            bit_off += [int(b) for b in bits]
        self.bit_off = np.array(bit_off, dtype=np.uint64)

    def members(self, wrap):
        return [HEADERS[wrap] + r + trailer(wrap, p) for r, p in zip(self.raws, self.inputs)]

    def want(self, wrap):
        """(bytes of all members, out_off[n_groups + 1])"""
        m = self.members(wrap)
        out_off = np.zeros(len(m) + 1, dtype=np.uint64)
        np.cumsum([len(x) for x in m], out=out_off[1:])
        return b"".join(m), out_off


def expected(data, in_off, group_off, wrap, compat_go=False):
    """(bytes of all members, out_off[n_groups + 1], bit_off[n_pieces + n_groups]) of the grouped call."""
    e = Expect(data, in_off, group_off, compat_go)
    return e.want(wrap) + (e.bit_off,)


SMALL_LENS = [0, 1, 17, 127, 128, 300, 3000]
KINDS = ["text", "zero", "rand"]
MIXED = [1, 2, 7, 1, 40] * 2


def corpus():
    """102 pieces: every small length as text, zeros and random bytes (random data makes stored blocks, so byte padding
    inside a member is exercised), and one piece of 70 000 bytes, two LZ77 windows."""
    spec = [(k, n) for _ in range(5) for n in SMALL_LENS for k in KINDS][:101]
    spec.insert(5, ("text", 70000))
    return pieces(spec, seed=11)


def layouts(n):
    """The group layouts over n = 102 pieces, by name."""
    assert n == sum(MIXED)
    return {"ones": layout([1] * n), "one": layout([n]), "mixed": layout(MIXED)}


def empties():
    """(data, in_off, group_off): group 1 is one empty piece, group 2 is empty pieces only."""
    data, off = pieces([("text", 300), ("zero", 0), ("zero", 0), ("zero", 0), ("zero", 0), ("rand", 300)], seed=12)
    return data, off, layout([1, 1, 3, 1])


def many(n):
    """n pieces of about 40 bytes in groups of 3 (the last one shorter where 3 does not divide n)."""
    kinds = ["text", "rand", "text", "zero"]
    data, off = pieces([(kinds[i % 4], 37 + i % 7) for i in range(n)], seed=13)
    sizes = [3] * (n // 3) + ([n % 3] if n % 3 else [])
    return data, off, layout(sizes)


def zip_pieces(entry_off, P):
    """(the pieces' in_off, group_off, long entries) of flate_hip_zip_write with "zip_piece_bytes" = P."""
    entry_off = [int(x) for x in entry_off]
    pin, goff, longs = [], [0], 0
    for lo, hi in zip(entry_off, entry_off[1:]):
        if P >= 1 and hi - lo > P:
            pin += list(range(lo, hi, P))
            longs += 1
        else:
            pin.append(lo)
        goff.append(len(pin))
    return np.array(pin + [entry_off[-1]], dtype=np.uint64), np.array(goff, dtype=np.uint32), longs


def zip_archive(data, entry_off, names, P, compat_go=False):
    """(archive bytes, entry_off with the directory's offset last, long entries, pieces): tests/zip_ref.py's archive
    over the spliced streams of the entries' pieces."""
    import zip_ref
    pin, goff, longs = zip_pieces(entry_off, P)
    e = Expect(data, pin, goff, compat_go)
    raw_names = [n.encode("utf-8") if isinstance(n, str) else bytes(n) for n in names]
    crcs = [zlib.crc32(p) & 0xffffffff for p in e.inputs]
    arc, off = zip_ref.write_archive(e.raws, raw_names, crcs, [len(p) for p in e.inputs])
    return arc, off, longs, pin.size - 1


def member_index(bit_off, group_off, g):
    """Group g's slice of the grouped index: n_g + 1 entries."""
    return bit_off[int(group_off[g]) + g:int(group_off[g + 1]) + g + 1]


def layout(sizes):
    """group_off of groups with these piece counts."""
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


def pieces(kinds_and_lens, seed=7):
    """(data, in_off) of pieces [(kind, len)]: kind "text" (compressible), "zero", "rand" (stored blocks)."""
    rng = np.random.RandomState(seed)
    words = [b"the ", b"quick ", b"brown ", b"fox ", b"jumps ", b"over ", b"lazy ", b"dog ", b"and ", b"again "]
    parts = []
    for kind, n in kinds_and_lens:
        if kind == "zero":
            parts.append(np.zeros(n, dtype=np.uint8))
        elif kind == "rand":
            parts.append(rng.randint(0, 256, n).astype(np.uint8))
        else:
            t = b"".join(words[k] for k in rng.randint(0, len(words), n // 4 + 2))[:n]
            parts.append(np.frombuffer(t, dtype=np.uint8))
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    np.cumsum([p.size for p in parts], out=off[1:])
    data = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return np.ascontiguousarray(data, dtype=np.uint8), off
