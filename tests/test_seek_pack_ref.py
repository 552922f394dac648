"""The keep rule on the CPU, against zlib: for every multi-unit stream of the two corpora and every span, every
segment's own bits -- cut out of the stream at the segment's first and last bit -- inflate under zlib with the SPARSE
window as the preset dictionary to exactly plain[P0:P1].  So no byte the rule drops is ever read.  (tests/seek_pack_ref.py
is the reference the GPU tests hold the library against; this file holds the reference against zlib.)"""
import zlib

import pytest

import one_ref as ref
import one_window_corpus as owc
import seek_pack_ref as sp
import seek_ref as sk

SPANS = (1, 4096, 40000, sk.SPAN_NONE)
FULL_FLUSH = 5  # the index of the Z_FULL_FLUSH file in one_ref.good_streams()


@pytest.fixture(scope="module")
def corpus():
    """[(what, raw stream, plain, Walk, copies)] of every stream of more than one unit: computed once, never changed."""
    out = []
    for what, raw, plain in ref.good_streams() + [s[:3] for s in owc.good_streams()]:
        w = ref.Walk(raw)
        if w.n_units > 1:
            out.append((what, raw, plain, w, sp.copies(raw)))
    return out


def test_the_corpus_is_not_vacuous(corpus):
    assert len(corpus) >= 25
    assert sum(1 for c in corpus if len(sk.points(c[3].out_off, 1)) >= 100) >= 2
    assert "Z_FULL_FLUSH" in ref.good_streams()[FULL_FLUSH][0]


def test_copies_walks_every_stream_to_its_end(corpus):
    for what, raw, plain, w, cps in corpus:
        assert all(0 < d <= min(q, 32768) and 3 <= ln <= 258 for q, ln, d in cps), what
        assert cps == sorted(cps) and (not cps or cps[-1][0] + cps[-1][1] <= len(plain)), what


def test_every_segment_inflates_from_its_sparse_window(corpus):
    n_segments = n_dropped = 0
    for what, raw, plain, w, cps in corpus:
        for span in SPANS:
            pts = sk.points(w.out_off, span)
            blks, kept = sp.blocks(plain, w.out_off, pts, sp.COMPRESS | sp.SPARSE, cps)
            assert len(blks) == len(pts) - 1 and 0 <= kept <= len(blks) * sp.WINDOW, (what, span)
            for i in range(1, len(pts)):
                P0 = w.out_off[pts[i]]
                P1 = w.out_off[pts[i + 1]] if i + 1 < len(pts) else w.out_off[-1]
                stream, zdict, skip = sp.segment_stream(raw, w.unit_bit, pts, i, blks[i - 1])
                d = zlib.decompressobj(-15, zdict=zdict)
                got = d.decompress(stream)
                assert got[skip:] == plain[P0:P1] and d.eof, (what, span, i)
                n_segments += 1
                n_dropped += blks[i - 1] != sk.window(plain, P0)
    assert n_segments > 700 and n_dropped > 400  # (the rule did drop bytes)


def test_the_full_flush_stream_has_only_empty_blocks(corpus):
    what, raw, plain = ref.good_streams()[FULL_FLUSH]
    w, cps = ref.Walk(raw), sp.copies(raw)
    for span in SPANS:
        pts = sk.points(w.out_off, span)
        blks, kept = sp.blocks(plain, w.out_off, pts, sp.COMPRESS | sp.SPARSE, cps)
        assert kept == 0 and not any(any(b) for b in blks), span
        assert sp.pack(blks, None) == ([0] * len(pts), b""), span
    assert len(sk.points(w.out_off, 1)) >= 20


def test_the_share_of_kept_bytes_is_what_the_issue_measured(corpus):
    what, raw, plain = ref.good_streams()[ref.MANY_UNITS]
    w, cps = ref.Walk(raw), sp.copies(raw)
    pts = sk.points(w.out_off, 1)
    blks, kept = sp.blocks(plain, w.out_off, pts, sp.COMPRESS | sp.SPARSE, cps)
    assert len(blks) == 229 and 0.02 < kept / (len(blks) * sp.WINDOW) < 0.05
