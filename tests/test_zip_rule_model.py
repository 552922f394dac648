"""The ZIP rule and argument checks on the CPU: moonbit-flate_amd/csrc/zip_rule.h -- the functions the kernels and the
library's host code compile -- built with g++ into a stand-alone program under AddressSanitizer and UBSan (every
archive in an allocation of exactly its size) and compared with tests/zip_ref.py and with Python's zipfile: the serial
reader on archives zipfile wrote and on hostile ones, the writer through zipfile, the closed form of the central
records' places against the serial sum.  The same program drives the ZIP checks of api_checks.h."""
import io
import os
import struct
import subprocess
import zipfile
import zlib

import pytest

import zip_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host_model", "zip_rule_model.cpp")
CSRC = os.path.join(ROOT, "moonbit-flate_amd", "csrc")
INC = os.path.join(ROOT, "include")
DEPS = [SRC, os.path.join(CSRC, "zip_rule.h"), os.path.join(CSRC, "api_checks.h"), os.path.join(INC, "flate_hip.h")]
EXE = os.path.join(HERE, "host_model", "zip_rule_model")
INVALID = -1


@pytest.fixture(scope="module")
def exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(d) for d in DEPS):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I" + CSRC, "-I" + INC, SRC, "-o", EXE])
    return EXE


def model_index(exe, files, tmp_path):
    path = tmp_path / "cases.bin"
    path.write_bytes(struct.pack("<I", len(files)) + b"".join(struct.pack("<Q", len(f)) + f for f in files))
    lines = subprocess.run([exe, "index", str(path)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(files)
    out = []
    for line in lines:
        head, end, ents = [part.split() for part in line.split("|")]
        out.append(([int(x) for x in head], [int(x) for x in end], [tuple(int(x) for x in e.split(",")) for e in ents]))
    return out


def check_against_ref(what, f, got):
    head, end, ents = got
    ix = ref.Index(f)
    assert head == [ix.rc, ix.n_entries, ix.err_off], what
    assert end == (list(ix.end) if ix.end else []), what
    assert ents == [tuple(e) for e in ix.entries], what
    return ix


def test_reader_equals_the_reference_and_zipfile_on_archives_zipfile_wrote(exe, tmp_path):
    corpus = ref.zipfile_corpus()
    for (what, f), got in zip(corpus, model_index(exe, [f for _, f in corpus], tmp_path)):
        ix = check_against_ref(what, f, got)
        assert ix.rc == 0, what
        infos = zipfile.ZipFile(io.BytesIO(f)).infolist()
        assert len(infos) == ix.n_entries, what
        for zi, e, name in zip(infos, ix.entries, ix.names):
            assert (zi.header_offset, zi.compress_size, zi.file_size, zi.CRC, zi.compress_type, zi.flag_bits) == \
                   (e.header_off, e.comp_size, e.size, e.crc32, e.method, e.flags), what
            assert e.status == 0 and name == zi.filename.encode("utf-8"), what
    by = dict(corpus)
    assert any(e.flags & 8 for e in ref.Index(by["unseekable sink"]).entries)
    z64 = ref.Index(by["force_zip64"])
    # (a local extra the directory does not have: data_off follows the LOCAL lengths)
    assert any(e.data_off != e.header_off + 30 + e.name_len for e in z64.entries)
    # (zipfile itself adds the Zip64 end record above 65535 entries; this library's writer from 65535 on)
    assert [ref.Index(by["%d entries" % n]).end.zip64 for n in (65535, 65536, 70000)] == [0, 1, 1]
    for e, (_, data) in zip(ref.Index(by["mixed"]).entries, ref.payloads()):
        assert ref.read_entry(by["mixed"], e) == (0, -1, data)


def test_hostile_archives_get_the_reference_verdicts(exe, tmp_path):
    cases = ref.hostile_corpus()
    for (what, f), got in zip(cases, model_index(exe, [f for _, f in cases], tmp_path)):
        check_against_ref(what, f, got)
    v = {what: ref.Index(f) for what, f in cases}
    base = ref.three()
    p = ref.find_end(base)
    E = ref.read_end(base, p)
    assert (v["signature in the comment, inconsistent"].rc, v["signature in the comment, inconsistent"].n_entries) == (0, 1)
    # (the consistent one is the highest: the rule takes it, an empty archive whose directory range is 0, 0)
    assert (v["signature in the comment, consistent"].rc, v["signature in the comment, consistent"].n_entries) == (0, 0)
    inner = v["a stored entry that holds an archive"]
    assert (inner.rc, inner.n_entries, [e.method for e in inner.entries]) == (0, 2, [0, 0])
    assert (v["count one too many"].rc, v["count one too many"].err_off, v["count one too many"].n_entries) == (ref.CORRUPT, E.cd_off + E.cd_size, 3)
    last = ref.Index(base).entries[2].name_off - 46
    assert (v["count one too few"].rc, v["count one too few"].err_off, v["count one too few"].n_entries) == (ref.CORRUPT, last, 2)
    for what in ("this disk's count differs", "disk number 1", "directory on disk 1", "directory past the end record"):
        assert (v[what].rc, v[what].err_off, v[what].n_entries) == (ref.CORRUPT, p, 0), what
    assert (v["directory size one short"].err_off, v["directory size one short"].n_entries) == (last, 2)
    assert (v["a broken record signature"].err_off, v["a broken record signature"].n_entries) == (E.cd_off, 0)
    assert v["no end record"].err_off == len(base) and v["nothing"].err_off == 0 and v["21 bytes"].err_off == 21
    for what, f in cases:
        if what == "zip64: a small archive":
            assert (v[what].rc, v[what].n_entries, v[what].end.zip64, zipfile.ZipFile(io.BytesIO(f)).testzip()) == (0, 3, 1, None)
        elif what.startswith("zip64"):
            assert (v[what].rc, v[what].err_off) == (ref.CORRUPT, ref.find_end(f)), what
        if what.startswith("truncated"):
            assert v[what].rc == ref.CORRUPT, what


def test_entry_cases_have_the_stated_verdicts(exe, tmp_path):
    cases = ref.entry_cases()
    for (what, f, k, status, err_off), got in zip(cases, model_index(exe, [c[1] for c in cases], tmp_path)):
        ix = check_against_ref(what, f, got)
        assert ix.rc == 0, what
        for i, e in enumerate(ix.entries):
            st, eo, _ = ref.read_entry(f, e)
            assert (st, eo) == ((status, err_off) if i == k else (0, -1)), (what, i)


def test_writer_through_zipfile(exe, tmp_path):
    items = ref.payloads() + [("n" * 255, b"name of 255 bytes"), ("é" * 150, b"name of 300 bytes")]
    raws, names = [], []
    for name, data in items:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        raws.append(c.compress(data) + c.flush())
        names.append(name.encode("utf-8"))
    crcs, sizes = [zlib.crc32(d) for _, d in items], [len(d) for _, d in items]
    for upto in (0, 1, len(items)):
        blob = struct.pack("<I", upto)
        for i in range(upto):
            blob += struct.pack("<IQQ", crcs[i], sizes[i], len(names[i])) + names[i] + struct.pack("<Q", len(raws[i])) + raws[i]
        (tmp_path / "in.bin").write_bytes(blob)
        out = subprocess.run([exe, "write", str(tmp_path / "in.bin"), str(tmp_path / "out.zip")], check=True,
                             capture_output=True, text=True).stdout
        got = (tmp_path / "out.zip").read_bytes()
        want, entry_off = ref.write_archive(raws[:upto], names[:upto], crcs[:upto], sizes[:upto])
        assert got == want and [int(x) for x in out.split()] == entry_off
        z = zipfile.ZipFile(io.BytesIO(got))
        assert z.testzip() is None and z.namelist() == [n for n, _ in items[:upto]]
        assert [z.read(n) for n, _ in items[:upto]] == [d for _, d in items[:upto]]
        assert ref.Index(got).rc == 0 and ref.Index(got).n_entries == upto


def test_zip64_end_records_through_zipfile(exe, tmp_path):
    n = 70000
    blob = struct.pack("<I", n)
    raw = b"\x01\x00\x00\xff\xff"
    for i in range(n):
        name = b"e%d" % i
        blob += struct.pack("<IQQ", 0, 0, len(name)) + name + struct.pack("<Q", len(raw)) + raw
    (tmp_path / "in.bin").write_bytes(blob)
    subprocess.run([exe, "write", str(tmp_path / "in.bin"), str(tmp_path / "out.zip")], check=True, capture_output=True)
    got = (tmp_path / "out.zip").read_bytes()
    assert got == ref.write_archive([raw] * n, [b"e%d" % i for i in range(n)], [0] * n, [0] * n)[0]
    assert got[-22:] == struct.pack("<4sHHHHIIH", b"PK\5\6", 0, 0, 0xffff, 0xffff, 0xffffffff, 0xffffffff, 0)
    z = zipfile.ZipFile(io.BytesIO(got))
    assert len(z.namelist()) == n and z.read("e69999") == b"" and z.testzip() is None
    ix = ref.Index(got)
    assert (ix.rc, ix.n_entries, ix.end.zip64) == (0, n, 1)


@pytest.mark.parametrize("where", ["k0 = 0", "k0 in the middle", "k0 = n"])
def test_closed_form_of_the_record_places(exe, tmp_path, where):
    # sizes only, no buffers: members of 1.5 GiB put the header offsets above 4 GiB from entry 3 on; a synthetic first
    # offset puts them there from entry 0 on; small members never
    n = 9
    member = [1000 + i for i in range(n)] if where == "k0 = n" else [(3 << 29) + 1000 * i for i in range(n)]
    base = 0xffffffff if where == "k0 = 0" else 0
    name_len = [1, 2, 255, 300, 65535, 7, 1, 9, 40]
    places, k0 = ref.central_place_serial(member, name_len, base)
    assert k0 == {"k0 = 0": 0, "k0 in the middle": 3, "k0 = n": n}[where]
    (tmp_path / "sizes.bin").write_bytes(struct.pack("<IQ", n, base) + b"".join(
        struct.pack("<QI", m, nl) for m, nl in zip(member, name_len)))
    out = [int(x) for x in subprocess.run([exe, "places", str(tmp_path / "sizes.bin")], check=True, capture_output=True,
                                          text=True).stdout.split()]
    assert out[0] == k0 and out[1:-1] == places
    assert out[-1] == (22 if where == "k0 = n" else 98)


def test_argument_checks(exe):
    out = subprocess.run([exe, "checks"], check=True, capture_output=True, text=True).stdout
    got = dict((k, int(v)) for k, v in (line.split() for line in out.splitlines()))
    bound = lambda n: 2 * n + 400  # (bound_model of the program)
    assert got == {
        "write_ok": 0, "write_n0_ok": 0, "write_name_max_ok": 0, "write_name_empty": INVALID, "write_name_long": INVALID,
        "write_name_off_back": INVALID, "write_in_off_back": INVALID, "write_no_in": INVALID, "write_no_in_off": INVALID,
        "write_no_names": INVALID, "write_no_name_off": INVALID, "write_no_out": INVALID, "write_no_len": INVALID,
        "write_flag_size_only": INVALID,
        "bound_0": 98, "bound_2": 98 + 2 * 88 + 2 * 3 + bound(4) + bound(0), "bound_refused": 0,
        "index_ok": 0, "index_query_ok": 0, "index_one_array": INVALID, "index_other_array": INVALID,
        "index_no_count": INVALID, "index_no_bytes": INVALID, "index_no_in": INVALID, "index_flag_go": INVALID,
        "read_ok": 0, "read_all_ok": 0, "read_query_ok": 0, "read_sel_over_cap": INVALID, "read_count_without_sel": INVALID,
        "read_no_out": INVALID, "read_no_out_off": INVALID, "read_no_len": INVALID, "read_no_status": INVALID,
        "read_no_err_off": INVALID, "read_no_in": INVALID, "read_flag_size_only": INVALID,
        "first_cap_small": 51, "first_cap_many": 74096,
    }
