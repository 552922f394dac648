"""CPU expectations for reading zlib / gzip members (flate_hip_inflate_batch_framed), shared by
tests/test_gpu_inflate_framed.py and tests/test_host_cpp_framed_read.py: what one member must come out as, by the
host mirrors' header helpers, the oracle's inflate on the exact payload range and the oracle's checksums -- and the
hand-built members both tests read."""
import importlib
import struct
import zlib

import numpy as np

from util import STATUS_OF_ORACLE, flate, make_streams

engine = importlib.import_module("moonbit-flate_amd.engine")
NO_DICT = engine.NO_DICT
LENGTHS = [0, 1, 16, 17, 127, 128, 1023, 1024, 1025, 5552, 65535, 65536, 65537, 131072, 200000]
FILLS = ["text", "rand", "zero", "ramp", "low", "period", "runs"]


def make_payloads():
    """One payload per length of LENGTHS, mixed fills."""
    data, off = make_streams([(FILLS[k % len(FILLS)], n) for k, n in enumerate(LENGTHS)], seed=77)
    return [data[int(off[i]):int(off[i + 1])].tobytes() for i in range(len(LENGTHS))]


def expected(oracle, member, wrap, slot, dicts, size_only=False):
    """(status, err_off, bytes delivered, dict_used) of one member, by the rules of include/flate_hip.h.  size_only:
    nothing is stored, so nothing can be summed -- the verdict covers header and decode only."""
    if wrap == "zlib":
        h, t, j = engine.zlib_member_header(member, engine.zlib_dict_ids(dicts) if dicts else None)
    else:
        (h, t), j = engine.parse_container_header(member, "gzip"), NO_DICT
    if h < 0 or len(member) < h + t:
        return -4, 0, b"", NO_DICT
    rc, got, _, eoff = oracle.inflate(member[h:len(member) - t], slot, full=True,
                                      zdict=bytes(dicts[j]) if j != NO_DICT else None)
    if rc != 0 or size_only:
        return STATUS_OF_ORACLE[rc], eoff, got, j
    tr = member[len(member) - t:]
    if wrap == "zlib":
        ok = oracle.adler32(got) == int.from_bytes(tr, "big")
    else:
        ok = oracle.crc32(got) == int.from_bytes(tr[:4], "little") and \
            (len(got) & 0xFFFFFFFF) == int.from_bytes(tr[4:], "little")
    return (0, eoff, got, j) if ok else (-4, len(member), got, j)


def kind_of(oracle, wrap):
    return oracle.FRAME_ZLIB if wrap == "zlib" else oracle.FRAME_GZIP


def oracle_member(oracle, wrap, p):
    return oracle.frame(kind_of(oracle, wrap), oracle.deflate(np.frombuffer(p, np.uint8)), p)


def zmember(p, d=None, level=6):
    """A zlib member of p, with FDICT + DICTID when a dictionary (also an empty one) is given."""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, zdict=d) if d else zlib.compressobj(level, zlib.DEFLATED, -15)
    raw = co.compress(p) + co.flush()
    return (engine.zlib_dict_header(d) if d is not None else b"\x78\x01") + raw + zlib.adler32(p).to_bytes(4, "big")


def gzmember(p, flg=0, extra=b"", name=b"a name\0", comment=b"a comment\0", raw=None):
    """A gzip member with a hand-built header: any combination of FHCRC (2), FEXTRA (4), FNAME (8), FCOMMENT (16)."""
    if raw is None:
        co = zlib.compressobj(6, zlib.DEFLATED, -15)
        raw = co.compress(p) + co.flush()
    h = bytes([0x1f, 0x8b, 8, flg, 1, 2, 3, 4, 0, 3])
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name
    if flg & 16:
        h += comment
    if flg & 2:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + raw + struct.pack("<II", zlib.crc32(p), len(p) & 0xFFFFFFFF)


def dict_batch(oracle):
    """(members, slots, dicts): several dictionaries, members with and without FDICT, a duplicate dictionary (the first
    wins), an empty one, one longer than 32 KiB (the id covers all of it, the tail is the history), an unknown id."""
    words = lambda seed, n: flate.synth("text", 1, n, seed=seed).tobytes()
    dicts = [words(31, 3000), words(32, 40000), b"", words(31, 3000), words(33, 17)]
    members = []
    for k in range(14):
        j = [0, 1, NO_DICT, 2, 3, 4, 1][k % 7]
        n = [2000, 300, 70000, 0, 5000, 131072][k % 6]
        d = dicts[j] if j != NO_DICT else None
        p = ((d or b"")[-400:] + words(40 + k, n))[:n]
        members.append(zmember(p, d))
    stranger = zmember(words(50, 900), words(51, 500))  # a DICTID that no dictionary of the call has
    members.insert(5, stranger)
    slots = [200000 if i % 2 else 131072 for i in range(len(members))]
    return members, slots, dicts


def bad_members(oracle, wrap, payloads):
    """[(what, member, slot)]: bad members, each followed by a good one."""
    text, rand = payloads[LENGTHS.index(1024)], payloads[LENGTHS.index(1025)]
    assert FILLS[LENGTHS.index(1024) % len(FILLS)] == "text"
    assert FILLS[LENGTHS.index(1025) % len(FILLS)] == "rand"  # (stored blocks: a flipped payload byte still decodes)
    good, stored = oracle_member(oracle, wrap, text), oracle_member(oracle, wrap, rand)
    hl, tl = (2, 4) if wrap == "zlib" else (10, 8)
    raw, trailer = good[hl:-tl], good[-tl:]
    cases = [("length %d" % k, good[:k], len(text)) for k in (0, 1, 9, 10, hl + tl - 1)]

    def flip(m, at, bit=1):
        b = bytearray(m)
        b[at] ^= bit
        return bytes(b)
    if wrap == "zlib":
        fcheck = lambda cmf: bytes([cmf, (31 - (cmf << 8) % 31) % 31])  # (FCHECK right: only CMF is wrong)
        cases += [("wrong CM", fcheck(0x77) + good[2:], len(text)),
                  ("CINFO = 8", fcheck(0x88) + good[2:], len(text)),
                  ("wrong FCHECK", flip(good, 1), len(text))]
        assert all(int.from_bytes(fcheck(c), "big") % 31 == 0 and not fcheck(c)[1] & 0x20 for c in (0x77, 0x88))
    else:
        cases += [("wrong magic", flip(good, 0), len(text)), ("wrong magic 2", flip(good, 1), len(text)),
                  ("wrong CM", flip(good, 2, 1), len(text)),
                  ("reserved flag bit 5", flip(good, 3, 0x20), len(text)),
                  ("reserved flag bit 7", flip(good, 3, 0x80), len(text)),
                  ("FNAME without a NUL", flip(good[:10], 3, 8) + b"name that never ends " * 3, len(text)),
                  ("FEXTRA past the end", flip(good[:10], 3, 4) + struct.pack("<H", 60000) + raw + trailer, len(text)),
                  ("FEXTRA without its length", flip(good[:10], 3, 4) + b"\x01", len(text)),
                  ("a flipped ISIZE bit", flip(good, len(good) - 3, 0x10), len(text))]
    cases += [("a flipped checksum bit", flip(good, len(good) - tl + 2, 0x04), len(text)),
              ("a flipped payload byte that still decodes", flip(stored, hl + 5 + 300, 0x40), len(rand)),
              ("a payload cut short", good[:hl] + raw[:-7] + trailer, len(text)),
              ("a payload cut to nothing", good[:hl] + trailer, len(text)),
              ("a corrupt payload", good[:hl] + b"\x07" + raw[1:] + trailer, len(text)),       # BTYPE = 3
              ("a corrupt payload later on", good[:hl] + raw[:200] + b"\xff" * 40 + raw[240:] + trailer, len(text)),
              ("good: bytes behind the final block are not examined", good[:hl] + raw + b"\xff" * 40 + trailer, len(text)),
              ("a slot too small", good, len(text) - 1),
              ("a slot of nothing", good, 0)]
    out = []
    for what, m, slot in cases:
        out.append((what, m, slot))
        out.append(("good", stored if len(out) % 4 else good, len(rand) if len(out) % 4 else len(text)))
    return out
