"""The reference of the gzip file reader in parts (tests/gzfile_parts_ref.py) held against zlib: for EVERY cut position
of two small files the bytes, the end of the file and the sum of in_used must be what gzfile_ref.members_of says."""
import pytest

import gzfile_parts_ref as ref
import gzfile_ref as gf


def _files():
    three = b"".join(m for m, _ in gf.three_members())
    return [("three_members", three), ("tiny_file", gf.tiny_file()[0])]


@pytest.mark.parametrize("what,f", _files(), ids=[w for w, _ in _files()])
def test_every_cut_against_zlib(what, f):
    plain = b"".join(gf.members_of(f))
    n_members = len(gf.members_of(f))
    m = ref.Model(f)
    assert m.plain == plain
    for cut in range(0, len(f) + 1):
        m.reset()
        calls, out, rest = ref.feed(ref.model_reader(m), f, [cut], None, 8, grow=len(f))
        assert out == plain, cut
        assert calls[-1].rc == ref.STREAM_END and rest == b"", cut
        assert sum(c.in_used for c in calls) == len(f), cut
        assert sum(c.n_members for c in calls) == n_members, cut


@pytest.mark.parametrize("out_cap", [1, 700, 4096])
def test_small_out_cap(out_cap):
    f, plain = gf.tiny_file()
    m = ref.Model(f)
    for step in (64, 1000):
        m.reset()
        calls, out, rest = ref.feed(ref.model_reader(m), f, iter([step] * (len(f) // step + 2)), out_cap, 4000, grow=step)
        if calls[-1].rc == ref.OUT_TOO_SMALL:
            assert calls[-1].out_len > out_cap and plain.startswith(out)
        else:
            assert out == plain and calls[-1].rc == ref.STREAM_END
