"""ZIP archives as flate_hip_zip_write / _index / _read define them (include/flate_hip.h), stated independently of
moonbit-flate_amd/csrc/zip_rule.h with struct: a serial reader (Index), a writer that assembles the expected archive
from given raw streams (write_archive), and the corpora the CPU model and the GPU tests share."""
import io
import struct
import zipfile
import zlib
from collections import namedtuple

OK, OUT_TOO_SMALL, CORRUPT, TOO_LARGE, UNEXPECTED_EOF, UNSUPPORTED = 0, -2, -4, -6, -7, -10
ALL32 = 0xFFFFFFFF
TAIL_WINDOW = 65557

Entry = namedtuple("Entry", "name_off header_off data_off comp_size size crc32 name_len method flags status")
ENTRY_DTYPE = [("name_off", "<u8"), ("header_off", "<u8"), ("data_off", "<u8"), ("comp_size", "<u8"), ("size", "<u8"),
               ("crc32", "<u4"), ("name_len", "<u2"), ("method", "<u2"), ("flags", "<u2"), ("reserved", "<u2"),
               ("status", "<i4"), ("reserved2", "<u4")]


# ---- writing ----

def local_header(name, crc, comp_size, size):
    return struct.pack("<4sHHHHHIIIHH", b"PK\3\4", 20, 0x0800, 8, 0, 0x0021, crc, comp_size, size, len(name), 0) + name


def central_record(name, crc, comp_size, size, header_off):
    z = header_off >= ALL32
    ver = 45 if z else 20
    extra = struct.pack("<HHQ", 1, 8, header_off) if z else b""
    return struct.pack("<4sHHHHHHIIIHHHHHII", b"PK\1\2", ver, ver, 0x0800, 8, 0, 0x0021, crc, comp_size, size, len(name),
                       len(extra), 0, 0, 0, 0, ALL32 if z else header_off) + name + extra


def needs_zip64_end(n, cd_off, cd_size):
    return n >= 65535 or cd_off >= ALL32 or cd_size >= ALL32


def end_records(n, cd_off, cd_size):
    out = b""
    z = needs_zip64_end(n, cd_off, cd_size)
    if z:
        out += struct.pack("<4sQHHIIQQQQ", b"PK\6\6", 44, 45, 45, 0, 0, n, n, cd_size, cd_off)
        out += struct.pack("<4sIQI", b"PK\6\7", 0, cd_off + cd_size, 1)
    return out + struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, 0xFFFF if z else n, 0xFFFF if z else n,
                             ALL32 if z else cd_size, ALL32 if z else cd_off, 0)


def write_archive(raws, names, crcs, sizes):
    """The archive of these raw DEFLATE streams: (bytes, entry_off with the directory's offset as its last entry)."""
    out, entry_off = io.BytesIO(), []
    for raw, name, crc, size in zip(raws, names, crcs, sizes):
        entry_off.append(out.tell())
        out.write(local_header(name, crc, len(raw), size))
        out.write(raw)
    cd_off = out.tell()
    entry_off.append(cd_off)
    for i, (raw, name, crc, size) in enumerate(zip(raws, names, crcs, sizes)):
        out.write(central_record(name, crc, len(raw), size, entry_off[i]))
    out.write(end_records(len(raws), cd_off, out.tell() - cd_off))
    return out.getvalue(), entry_off


def central_place_serial(sizes_of_members, name_lens, base=0):
    """Where every central record starts inside the directory, by the serial sum: (places with the directory's size as
    the last entry, k0).  Sizes only; base: the first header's offset (0 in an archive)."""
    at, off, places, k0 = 0, base, [], len(name_lens)
    for i, (m, nl) in enumerate(zip(sizes_of_members, name_lens)):
        places.append(at)
        if off >= ALL32 and k0 == len(name_lens):
            k0 = i
        at += 46 + nl + (12 if off >= ALL32 else 0)
        off += m
    places.append(at)
    return places, k0


# ---- reading ----

def find_end(f):
    """The highest p of the tail window with the signature and p + 22 + comment length == len(f), or -1."""
    lo = max(0, len(f) - TAIL_WINDOW)
    p = f.rfind(b"PK\5\6", lo)
    while p >= 0:
        if p + 22 <= len(f) and p + 22 + struct.unpack_from("<H", f, p + 20)[0] == len(f):
            return p
        p = f.rfind(b"PK\5\6", lo, p + 3) if p > lo else -1
    return -1


End = namedtuple("End", "end_off rec_off n cd_off cd_size zip64")


def read_end(f, p):
    """The values of the end record at p, or None: refused."""
    rec_off, z = p, 0
    if p >= 20 and f[p - 20:p - 16] == b"PK\6\7":
        disk, r, disks = struct.unpack_from("<IQI", f, p - 16)
        if disk != 0 or disks != 1 or p < 76 or r > p - 76 or f[r:r + 4] != b"PK\6\6":
            return None
        disk, cd_disk, here, n, cd_size, cd_off = struct.unpack_from("<IIQQQQ", f, r + 16)
        rec_off, z = r, 1
    else:
        disk, cd_disk, here, n, cd_size, cd_off = struct.unpack_from("<HHHHII", f, p + 4)
    if disk or cd_disk or here != n or cd_off + cd_size > rec_off:
        return None
    return End(p, rec_off, n, cd_off, cd_size, z)


def central_read(f, at, cd_end):
    """The record at directory offset `at`: (total, flags, method, crc, comp_size, size, name_len, header_off) or None."""
    if cd_end - at < 46 or f[at:at + 4] != b"PK\1\2":
        return None
    flags, method, _, _, crc, comp, size, nl, xl, cl, _, _, _, hoff = struct.unpack_from("<HHHHIIIHHHHHII", f, at + 8)
    total = 46 + nl + xl + cl
    if at + total > cd_end:
        return None
    if ALL32 in (size, comp, hoff):
        extra, vals = f[at + 46 + nl:at + 46 + nl + xl], None
        while len(extra) >= 4:
            tp, ln = struct.unpack_from("<HH", extra)
            if 4 + ln > len(extra):
                break
            if tp == 1:
                vals = extra[4:4 + ln]
                break
            extra = extra[4 + ln:]
        vals = vals or b""
        got = []
        for v in (size, comp, hoff):
            if v == ALL32:
                if len(vals) < 8:
                    return None
                v, vals = struct.unpack_from("<Q", vals)[0], vals[8:]
            got.append(v)
        size, comp, hoff = got
    return total, flags, method, crc, comp, size, nl, hoff


def make_entry(f, cd_off, at, rec):
    _, flags, method, crc, comp, size, nl, hoff = rec
    e = dict(name_off=at + 46, header_off=hoff, data_off=0, comp_size=comp, size=size, crc32=crc, name_len=nl,
             method=method, flags=flags, status=OK)
    if (flags & 0x61) or method not in (0, 8):
        e["status"] = UNSUPPORTED
        return Entry(**e)
    e["status"] = CORRUPT
    if hoff + 30 > cd_off or f[hoff:hoff + 4] != b"PK\3\4":
        return Entry(**e)
    ln, le = struct.unpack_from("<HH", f, hoff + 26)
    e["data_off"] = hoff + 30 + ln + le
    if e["data_off"] + comp > cd_off or (method == 0 and comp != size):
        return Entry(**e)
    e["status"] = OK
    return Entry(**e)


class Index:
    """flate_hip_zip_index, serially: rc, err_off (-1), n_entries, end, entries, out_off, out_bytes."""

    def __init__(self, f):
        f = bytes(f)
        self.rc, self.err_off, self.n_entries, self.entries, self.out_off, self.out_bytes, self.end = CORRUPT, -1, 0, [], [0], 0, None
        p = find_end(f)
        if p < 0:
            self.err_off = len(f)
            return
        self.end = read_end(f, p)
        if self.end is None:
            self.err_off = p
            return
        E = self.end
        at, cd_end = E.cd_off, E.cd_off + E.cd_size
        for _ in range(E.n):
            rec = central_read(f, at, cd_end)
            if rec is None:
                self.err_off = at
                return
            self.entries.append(make_entry(f, E.cd_off, at, rec))
            self.n_entries += 1
            at += rec[0]
        if at != cd_end:
            self.err_off = at
            return
        self.rc = OK
        for e in self.entries:
            self.out_off.append(self.out_off[-1] + (e.size if e.status == OK else 0))
        self.out_bytes = self.out_off[-1]
        self.names = [f[e.name_off:e.name_off + e.name_len] for e in self.entries]


def read_entry(f, e):
    """What flate_hip_zip_read delivers for one entry: (status, err_off or None where the decoder decides it, bytes)."""
    if e.status:
        return e.status, -1, b""
    data = bytes(f[e.data_off:e.data_off + e.comp_size])
    if e.method == 0:
        out = data
    else:
        d = zlib.decompressobj(-15)
        try:
            out = d.decompress(data)
        except zlib.error:
            return CORRUPT, None, None
        if not d.eof:
            return UNEXPECTED_EOF, None, None
    if len(out) > e.size:
        return OUT_TOO_SMALL, None, None
    if len(out) != e.size or zlib.crc32(out) != e.crc32:
        return CORRUPT, e.comp_size, None
    return OK, -1, out


# ---- the corpora ----

class _Unseekable(io.RawIOBase):
    """A sink zipfile cannot seek in: it sets flag bit 3 and writes data descriptors."""

    def __init__(self):
        self.buf = io.BytesIO()

    def writable(self):
        return True

    def write(self, b):
        return self.buf.write(b)

    def flush(self):
        pass


def _text(n, seed):
    words = [b"alpha", b"beta", b"gamma", b"delta", b"stream", b"zip", b"archive", b"entry", b"\n", b" "]
    out, x = bytearray(), seed * 2654435761 % (1 << 32)
    while len(out) < n:
        x = (x * 1103515245 + 12345) % (1 << 31)
        out += words[x % len(words)] + b" "
    return bytes(out[:n])


def _rand(n, seed):
    import random
    return random.Random(seed).randbytes(n)


def payloads():
    return [("empty.txt", b""), ("one", b"x"), ("dir/text17.txt", _text(17, 1)), ("r127.bin", _rand(127, 2)),
            ("t4096.txt", _text(4096, 3)), ("z70000", bytes(70000)), ("t70000.txt", _text(70000, 4)),
            ("äö☃/r300.bin", _rand(300, 5))]


def _zf(items, compression, level=None, comment=b"", sink=None, force64=False, mixed=False):
    buf = sink or io.BytesIO()
    with zipfile.ZipFile(buf, "w", compression, compresslevel=level) as z:
        z.comment = comment
        for k, (name, data) in enumerate(items):
            zi = zipfile.ZipInfo(name)
            zi.compress_type = (zipfile.ZIP_STORED if k % 2 else zipfile.ZIP_DEFLATED) if mixed else compression
            if force64:
                with z.open(zi, "w", force_zip64=True) as w:
                    w.write(data)
            else:
                z.writestr(zi, data, compresslevel=(1 + 4 * (k % 3)) if mixed else level)
    return (buf.buf if sink else buf).getvalue()


_cache = {}


def many(n):
    """An archive of n tiny stored-or-deflated entries of 0 - 3 bytes, written by zipfile."""
    if n not in _cache:
        _cache[n] = _zf([("e%d" % i, b"abc"[:i % 4]) for i in range(n)], zipfile.ZIP_DEFLATED, 1)
    return _cache[n]


def zipfile_corpus(big=True):
    """(what, archive) for archives zipfile wrote."""
    if "corpus" not in _cache:
        P = payloads()
        _cache["corpus"] = [
            ("stored", _zf(P, zipfile.ZIP_STORED)),
            ("deflated 1", _zf(P, zipfile.ZIP_DEFLATED, 1)),
            ("deflated 6", _zf(P, zipfile.ZIP_DEFLATED, 6)),
            ("deflated 9", _zf(P, zipfile.ZIP_DEFLATED, 9)),
            ("mixed", _zf(P, zipfile.ZIP_DEFLATED, mixed=True)),
            ("archive comment", _zf(P, zipfile.ZIP_DEFLATED, 6, comment=b"a comment of the archive")),
            ("unseekable sink", _zf(P, zipfile.ZIP_DEFLATED, 6, sink=_Unseekable())),
            ("force_zip64", _zf(P, zipfile.ZIP_DEFLATED, 6, force64=True)),
            ("empty archive", _zf([], zipfile.ZIP_DEFLATED)),
        ]
    out = list(_cache["corpus"])
    if big:
        out += [("%d entries" % n, many(n)) for n in (65535, 65536, 70000)]
    return out


def three():
    """The 3-entry archive of the hostile cases."""
    return _zf([("a.txt", _text(200, 7)), ("b.bin", _rand(40, 8)), ("c", b"")], zipfile.ZIP_DEFLATED, 6)


def _patch(f, at, fmt, *v):
    b = bytearray(f)
    struct.pack_into(fmt, b, at, *v)
    return bytes(b)


def hostile_corpus():
    """(what, bytes): archive-level cases; their verdicts are Index's."""
    base = three()
    p = find_end(base)
    E = read_end(base, p)
    inner = three()
    fake_end = struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, 0, 0, 0, 0, 0)
    out = [
        # an end-record signature inside the comment: one that fails the equation, one that satisfies it (and wins,
        # being higher: an empty archive)
        ("signature in the comment, inconsistent", _zf([("a", b"abc")], zipfile.ZIP_STORED, comment=b"xx" + fake_end[:21] + b"\7yy")),
        ("signature in the comment, consistent", _zf([("a", b"abc")], zipfile.ZIP_STORED, comment=b"xx" + fake_end)),
        ("a stored entry that holds an archive", _zf([("inner.zip", inner), ("b", b"tail")], zipfile.ZIP_STORED)),
        ("count one too many", _patch(base, p + 8, "<HH", E.n + 1, E.n + 1)),
        ("count one too few", _patch(base, p + 8, "<HH", E.n - 1, E.n - 1)),
        ("this disk's count differs", _patch(base, p + 8, "<H", E.n - 1)),
        ("disk number 1", _patch(base, p + 4, "<H", 1)),
        ("directory on disk 1", _patch(base, p + 6, "<H", 1)),
        ("directory past the end record", _patch(base, p + 16, "<I", E.cd_off + 1)),
        ("directory size one short", _patch(base, p + 12, "<I", E.cd_size - 1)),
        ("a broken record signature", _patch(base, E.cd_off + 46 + 5, "<B", 0x50) if False else
         _patch(base, E.cd_off, "<I", 0x02014b51)),
        ("no end record", base[:p] + b"QK" + base[p + 2:]),
        ("nothing", b""),
        ("21 bytes", fake_end[:21]),
    ]
    # the same archive with a Zip64 end record and locator in front of an all-ones end record
    cd_end = E.cd_off + E.cd_size
    z64 = (base[:cd_end] + struct.pack("<4sQHHIIQQQQ", b"PK\6\6", 44, 45, 45, 0, 0, E.n, E.n, E.cd_size, E.cd_off) +
           struct.pack("<4sIQI", b"PK\6\7", 0, cd_end, 1) +
           struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, 0xFFFF, 0xFFFF, ALL32, ALL32, 0))
    q = cd_end + 76
    out += [
        ("zip64: a small archive", z64),
        ("zip64: two disks in the locator", _patch(z64, q - 4, "<I", 2)),
        ("zip64: the locator names disk 1", _patch(z64, q - 16, "<I", 1)),
        ("zip64: record offset past the locator", _patch(z64, q - 12, "<Q", q - 75)),
        ("zip64: no record signature", _patch(z64, cd_end, "<I", 0)),
        ("zip64: this disk's count differs", _patch(z64, cd_end + 24, "<Q", E.n - 1)),
        ("zip64: the directory on disk 1", _patch(z64, cd_end + 20, "<I", 1)),
    ]
    out += [("truncated to %d" % k, base[:k]) for k in range(len(base))]
    return out


def entry_cases():
    """(what, bytes, entry, status, err_off or None): one entry of the 3-entry archive damaged; the others read."""
    base = three()
    ix = Index(base)
    E = ix.end
    rec = [e.name_off - 46 for e in ix.entries]
    e0 = ix.entries[0]
    return [
        ("a wrong CRC in the directory", _patch(base, rec[0] + 16, "<I", e0.crc32 ^ 1), 0, CORRUPT, e0.comp_size),
        ("a size one too large", _patch(base, rec[0] + 24, "<I", e0.size + 1), 0, CORRUPT, e0.comp_size),
        ("a size one too small", _patch(base, rec[0] + 24, "<I", e0.size - 1), 0, OUT_TOO_SMALL, None),
        ("a broken local signature", _patch(base, ix.entries[1].header_off, "<B", 0x51), 1, CORRUPT, -1),
        ("data past the directory", _patch(base, rec[1] + 20, "<I", E.cd_off), 1, CORRUPT, -1),
        ("a stream cut short", _patch(base, rec[0] + 20, "<I", e0.comp_size - 3), 0, UNEXPECTED_EOF, None),
        ("method 12", _patch(base, rec[1] + 10, "<H", 12), 1, UNSUPPORTED, -1),
        ("the encrypted flag", _patch(base, rec[0] + 8, "<H", ix.entries[0].flags | 1), 0, UNSUPPORTED, -1),
    ]
