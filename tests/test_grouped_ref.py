"""tests/grouped_ref.py is a reference worth comparing with: every expected member of a grouped call inflates with
zlib / gzip to its group's input, a group of one piece is the oracle's single stream, and the index slices are what the
oracle returns for the group alone.  Both compat modes.  (CPU only.)"""
import gzip
import zlib

import numpy as np
import pytest

import grouped_ref as ref

MODES = [False, True]


@pytest.fixture(scope="module")
def corpus(oracle):
    return ref.corpus()


@pytest.fixture(scope="module")
def expects(oracle, corpus):
    data, off = corpus
    return {(name, go): ref.Expect(data, off, lay, go) for name, lay in ref.layouts(off.size - 1).items() for go in MODES}


def cpu_read(wrap, member):
    if wrap == "raw":
        return zlib.decompress(member, -15)
    return zlib.decompress(member) if wrap == "zlib" else gzip.decompress(member)


@pytest.mark.parametrize("go", MODES)
@pytest.mark.parametrize("name", ["ones", "one", "mixed"])
def test_every_member_inflates_to_its_groups_input(expects, name, go):
    e = expects[(name, go)]
    for wrap in ("raw", "zlib", "gzip"):
        whole, out_off = e.want(wrap)
        assert int(out_off[-1]) == len(whole)
        for g in range(e.n_groups):
            member = whole[int(out_off[g]):int(out_off[g + 1])]
            assert cpu_read(wrap, member) == e.inputs[g], (wrap, g)


@pytest.mark.parametrize("go", MODES)
def test_a_group_of_one_piece_is_the_oracles_single_stream(oracle, corpus, expects, go):
    data, off = corpus
    e = expects[("ones", go)]
    for i in range(e.n_pieces):
        p = data[int(off[i]):int(off[i + 1])]
        assert e.raws[i] == oracle.deflate(p, compat=ref.compat_of(go)), i
        assert ref.member_index(e.bit_off, e.group_off, i)[0] == 0


@pytest.mark.parametrize("go", MODES)
def test_one_group_of_everything_is_the_spliced_stream(oracle, corpus, expects, go):
    data, off = corpus
    e = expects[("one", go)]
    raw, bits = oracle.deflate_spliced(data, off, ref.compat_of(go))
    assert e.raws == [bytes(raw)] and np.array_equal(e.bit_off, bits)
    assert e.bit_off.size == e.n_pieces + 1


def test_the_index_has_one_slice_per_group(expects):
    e = expects[("mixed", False)]
    assert e.bit_off.size == e.n_pieces + e.n_groups
    for g in range(e.n_groups):
        s = ref.member_index(e.bit_off, e.group_off, g)
        assert s.size == int(e.group_off[g + 1]) - int(e.group_off[g]) + 1
        assert s[0] == 0 and (np.diff(s.astype(np.int64)) >= 0).all()
        assert int(s[-1]) <= 8 * len(e.raws[g])


def test_empty_groups_and_many_small_ones(oracle):
    data, off, lay = ref.empties()
    e = ref.Expect(data, off, lay)
    assert e.raws[1] == b"\x01\x00\x00\xff\xff" and e.raws[2] == b"\x01\x00\x00\xff\xff"
    for wrap in ("zlib", "gzip"):
        for m, p in zip(e.members(wrap), e.inputs):
            assert cpu_read(wrap, m) == p
    data, off, lay = ref.many(1025)
    e = ref.Expect(data, off, lay)
    assert e.n_groups == 342 and all(cpu_read("gzip", m) == p for m, p in zip(e.members("gzip"), e.inputs))
