"""The forms of a gzip file agree on the GPU: flate_hip_gzfile_read of a file against a fresh flate_hip_gzfile_reader_*
handle that is given the same file as ONE final part with room for everything -- the whole file is the part that is
final and starts at a BOUNDARY, and one set of kernels runs both.  With "gzfile_serial_max" / set_serial_max at 0 and
at S, host and device pointers: the same bytes, status, bad_member, err_off, stream_err_off, member and unit counts,
and -- S >= 1 -- the same serial_members and find_from of the two last_route calls.

Two relations are the documented behaviour of the two calls and not equalities (include/flate_hip.h):
  * a reader's final call that reaches the file's end returns FLATE_HIP_STREAM_END (1) where the whole call's status is
    0, and reports in_used = len(file);
  * chain good, a trailer wrong: the whole call delivers every member; the reader delivers up to and including that
    member's last byte and nothing behind it, and counts the members and units in front of that point (with them the
    whole members among the units it delivered).  Status and the three words are the same."""
import numpy as np
import pytest

import gzfile_parts_serial_ref as R
import gzfile_ref as ref
import gzfile_serial_ref as sref
import test_gpu_gzfile as base
import test_gpu_gzfile_parts_serial as ps
from util import flate

pytestmark = pytest.mark.gpu

S = ps.S
STREAM_END = R.STREAM_END


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def files():
    """[(what, file, the member whose trailer is wrong or None)]: the smallest inputs that reach each branch the two
    forms share."""
    three = b"".join(x for x, _ in ref.three_members())
    w = ref.Walk(three)
    assert w.n_members == 3 and w.member_unit[2] - w.member_unit[1] >= 2 and w.member_off[2] - w.member_off[1] > S
    header = bytearray(three)
    header[w.member_off[1]] ^= 1  # ID1 of the second member
    crc = bytearray(three)
    crc[w.member_off[2] - 8] ^= 0x40  # the middle member's CRC-32
    tiny = ref.tiny_file()[0]
    assert any(s == 0 for s in ref.Walk(tiny).sizes)  # members with ISIZE 0
    return [("three members, the middle one of several units", three, None),
            ("forty short members", ps.forty_members()[0], None),
            ("one junk byte behind the last trailer", three + b"j", None),
            ("cut inside the last trailer", three[:-3], None),
            ("a corrupt second header", bytes(header), None),
            ("a wrong CRC-32 in the middle member", bytes(crc), 1),
            ("empty members", tiny, None)]


@pytest.mark.parametrize("case", files(), ids=[c[0] for c in files()])
def test_the_whole_call_and_one_final_part_agree(eng, case):
    what, f, wrong = case
    room = ref.Walk(f).out_len + 64
    for serial in (0, S):
        for device in (False, True):
            eng.set_option("gzfile_serial_max", serial)
            try:
                rc, got, out_len, words, n_members, n_units, _ = base.read(eng, f, room, device=device)
                route = eng.gzfile_last_route()
                ix = base.index(eng, f)
            finally:
                eng.set_option("gzfile_serial_max", 0)
            routes = []
            rd = eng.open_gzfile_reader(device=device, serial_max=serial)
            try:
                c, part = ps.reader(rd, device, routes)(f, True, room)
            finally:
                rd.close()
            print(what, serial, device, (rc, out_len, words, n_members, n_units, route), c, routes)
            tag = (what, serial, device)
            status = words[0]
            assert rc == status and c.rc == (status if status else STREAM_END), tag
            assert c.in_used == (0 if status else len(f)), tag
            assert (c.bad_member, c.err_off, c.stream_err_off) == words[1:], tag
            assert routes[0][1] == 0 and routes[0][2] == route[2], tag  # a final part has no OPEN stop; find_from
            if wrong is None:
                assert part == got and c.out_len == out_len, tag
                assert (c.n_members, c.n_units) == (n_members, n_units), tag
                assert routes[0][0] == (route[0] if serial else 0), tag
            else:  # the documented relation: up to and including the member's last byte
                out_off, member_unit = ix[3], ix[5]
                end_unit = member_unit[wrong + 1]
                assert status == ref.CORRUPT and words[1] == wrong and n_members == 3 and out_len == len(got), tag
                assert c.out_len == out_off[end_unit] < out_len and part == got[:c.out_len], tag
                assert (c.n_members, c.n_units) == (wrong, end_unit), tag
                whole = sref.Model(f, serial, ref.Walk(f)).whole if serial else []  # per member, from the file's bytes
                assert route[0] == sum(whole) and routes[0][0] == sum(whole[:wrong + 1]), tag
