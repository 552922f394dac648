"""GPU tests of flate_hip_zip_write with the option "zip_piece_bytes": an entry longer than P bytes is written from
pieces, spliced into one stream.  Every archive is compared BYTE FOR BYTE with tests/grouped_ref.py's (tests/zip_ref.py's
archive over the oracle's spliced streams of the pieces), opened by zipfile, read back by flate_hip_zip_read with
"zip_unit_min" 0 and 1, and the route query must report the expected pieces.  The expectations are computed once."""
import io
import zipfile

import numpy as np
import pytest

import grouped_ref as ref
from util import flate

pytestmark = pytest.mark.gpu

E_OUT_TOO_SMALL = -2
LENS = [0, 5, 300, 3000, 70000, 200000]
NAME_LENS = [1, 2, 17, 64, 199, 200]
SIZES = [1000, 4096, 65535, 65536]
GUARD = 64


@pytest.fixture(scope="module")
def eng():
    flate.build()
    e = flate.FlateEngine(0)
    yield e
    e.set_option("zip_piece_bytes", 0)
    e.set_option("zip_unit_min", 0)
    e.close()


@pytest.fixture(scope="module")
def entries(oracle):
    kinds = ["text", "text", "rand", "text", "text", "text"]
    data, off = ref.pieces(list(zip(kinds, LENS)), seed=31)
    names = [("n%d" % k + "x" * 200)[:n] for k, n in enumerate(NAME_LENS)]
    return np.concatenate([data, np.zeros(16, np.uint8)]), off, names


@pytest.fixture(scope="module")
def wants(oracle, entries):
    """{P: (archive, entry_off, long entries, pieces)}; P = 0: the archive of the option at 0."""
    data, off, names = entries
    return {P: ref.zip_archive(data, off, names, P) for P in [0] + SIZES + [200000, 1 << 40]}


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def payload(entries, i):
    data, off, _ = entries
    return data[int(off[i]):int(off[i + 1])].tobytes()


@pytest.mark.parametrize("P", SIZES)
def test_the_archive_equals_the_reference_and_every_reader_opens_it(eng, entries, wants, P):
    data, off, names = entries
    want, want_off, longs, pieces = wants[P]
    assert longs >= 1 and pieces > len(names)
    eng.set_option("zip_piece_bytes", P)
    got, entry_off = eng.zip_write(data, off, names, index=True)
    assert eng.zip_write_last_route() == (longs, pieces)
    assert entry_off.tolist() == want_off
    assert got == want
    assert len(got) <= flate.zip_bound(off, names)
    dev, dev_len = eng.zip_write(to_dev(data), off, names)
    assert dev.cpu().numpy()[:dev_len].tobytes() == want
    z = zipfile.ZipFile(io.BytesIO(got))
    assert z.testzip() is None and z.namelist() == names
    for i, n in enumerate(names):
        assert z.read(n) == payload(entries, i), i
    arc = np.frombuffer(got, dtype=np.uint8)
    for unit_min in (0, 1):
        eng.set_option("zip_unit_min", unit_min)
        out, r = eng.zip_read(arc)
        assert r.rc == 0 and (r.status == 0).all()
        for i in range(len(names)):
            assert out[int(r.out_off[i]):int(r.out_off[i]) + int(r.out_len[i])].tobytes() == payload(entries, i), (unit_min, i)
    eng.set_option("zip_unit_min", 0)


@pytest.mark.parametrize("P", [0, 200000, 1 << 40])
def test_no_long_entry_is_the_unchanged_route_and_the_same_bytes(eng, entries, wants, P):
    data, off, names = entries
    eng.set_option("zip_piece_bytes", 0)
    plain = eng.zip_write(data, off, names)
    assert eng.zip_write_last_route() == (0, 0)
    assert plain == wants[0][0] == wants[P][0] and wants[P][2] == 0
    eng.set_option("zip_piece_bytes", P)
    assert eng.zip_write(data, off, names) == plain
    assert eng.zip_write_last_route() == (0, 0)


def test_the_route_is_reset_by_the_next_plain_write(eng, entries, wants):
    data, off, names = entries
    eng.set_option("zip_piece_bytes", 4096)
    eng.zip_write(data, off, names)
    assert eng.zip_write_last_route() == wants[4096][2:]
    eng.set_option("zip_piece_bytes", 0)
    eng.zip_write(data, off, names)
    assert eng.zip_write_last_route() == (0, 0)


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_device_pointers_at_every_misalignment_exact_room_and_one_byte_less(eng, entries, wants, shift):
    import torch
    data, off, names = entries
    want = wants[4096][0]
    total = len(want)
    eng.set_option("zip_piece_bytes", 4096)
    buf = torch.full((GUARD + 4 + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = buf[GUARD + shift:GUARD + shift + total]
    with pytest.raises(flate.FlateError) as ei:
        eng.zip_write(to_dev(data), off, names, out=out, out_cap=total - 1)
    assert ei.value.code == E_OUT_TOO_SMALL
    assert (buf.cpu().numpy() == 0xA5).all(), "a refused call wrote"
    _, n = eng.zip_write(to_dev(data), off, names, out=out, out_cap=total)
    b = buf.cpu().numpy()
    assert n == total and b[GUARD + shift:GUARD + shift + total].tobytes() == want
    assert (b[:GUARD + shift] == 0xA5).all() and (b[GUARD + shift + total:] == 0xA5).all()


def test_what_the_call_refuses_it_refuses_with_the_option_on(eng, entries):
    data, off, names = entries
    eng.set_option("zip_piece_bytes", 1000)
    with pytest.raises(flate.FlateError) as ei:
        eng.zip_write(data, off, names[:-1] + [""])
    assert ei.value.code == -1
    with pytest.raises(flate.FlateError) as ei:
        eng.zip_write(data, off, names[:-1] + ["y" * 65536])
    assert ei.value.code == -1
    with pytest.raises(flate.FlateError):
        eng.set_option("zip_piece_bytes", -1)
    assert eng.zip_write(data[:0], [0], []) == bytes([0x50, 0x4b, 5, 6] + [0] * 18)
    assert eng.zip_write_last_route() == (0, 0)
