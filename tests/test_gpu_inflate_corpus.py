"""The hand-built DEFLATE edge corpus (tests/deflate_corpus.py) through every batch decoder configuration, plain and
with preset dictionaries, through FLATE_HIP_SIZE_ONLY and through the piecewise stream decoder.  Every stream --
base cases, other output slots, every byte-boundary truncation, the cases behind a prefix block -- must give the
oracle's status, err_off, out_len and output bytes, whatever the status.  Valid streams from zlib are mixed into
the batches, so that lanes of one wavefront take different paths."""
import zlib

import numpy as np
import pytest

import deflate_corpus as D
from util import INFLATE_CONFIGS, STATUS_OF_ORACLE, flate, force_inflate_config

pytestmark = pytest.mark.gpu

NO_DICT = flate.NO_DICT
STREAM_END = 1  # FLATE_HIP_STREAM_END
SHARED_DICT = bytes((i * 29 + 7) & 255 for i in range(300)) + D.TEXT * 3


def _entries():
    """(name, stream, cap, zdict): the base cases and all their variants."""
    base = [(c.name, c.data, c.cap, c.zdict) for c in D.CASES]
    return base + D.variants()


def _good(k):
    raw = flate.synth("text", 1, 300 + 97 * k, seed=50 + k).tobytes()
    co = zlib.compressobj(1 + k % 9, zlib.DEFLATED, -15)
    return "good%d" % k, co.compress(raw) + co.flush(), len(raw), b""


def _mixed(entries):
    out = []
    for i, e in enumerate(entries):
        out.append(e)
        if i % 5 == 4:
            out.append(_good(i // 5 % 40))
    return out


def _pack(blobs):
    off = np.zeros(len(blobs) + 1, np.uint64)
    np.cumsum(np.array([len(b) for b in blobs], dtype=np.uint64), out=off[1:])
    return np.frombuffer(b"".join(blobs) + b"\0" * 8, dtype=np.uint8).copy(), off


def _check_batch(oracle, entries, zdict_of, res):
    out, ooff, olen, status, err = res
    bad = []
    for i, (name, data, cap, _) in enumerate(entries):
        zd = zdict_of(i)
        rc, want, _, eoff = oracle.inflate(data, cap, full=True, zdict=zd or None)
        got = bytes(out[int(ooff[i]):int(ooff[i]) + int(olen[i])])
        have = (int(status[i]), int(err[i]), int(olen[i]))
        if have != (STATUS_OF_ORACLE[rc], eoff, len(want)) or got != want:
            bad.append((name, have, (STATUS_OF_ORACLE[rc], eoff, len(want)), got == want))
    assert not bad, "%d of %d streams differ from the oracle, first: %s" % (len(bad), len(entries), bad[:12])


@pytest.fixture(scope="module", params=INFLATE_CONFIGS)
def eng(request):
    flate.build()
    e = force_inflate_config(flate.FlateEngine(0), request.param)
    yield e
    e.close()


def test_corpus_plain(eng, oracle):
    entries = _mixed([e for e in _entries() if not e[3]])
    data, off = _pack([e[1] for e in entries])
    res = eng.inflate_batch(data, off, [e[2] for e in entries], check=False)
    _check_batch(oracle, entries, lambda i: None, res)


def test_corpus_with_dictionaries(eng, oracle):
    """The dictionary cases with their own dictionaries, and the plain corpus with one shared dictionary (the
    dictionary build of each decoder)."""
    entries = _entries()
    own = [e for e in entries if e[3]]
    plain = [e for e in entries if not e[3]]
    entries = _mixed(own + [(n + "/shared_dict", d, c, SHARED_DICT) for n, d, c, _ in plain])
    dicts = sorted({e[3] for e in entries if e[3]}, key=len)
    dict_of = [dicts.index(e[3]) if e[3] else NO_DICT for e in entries]
    data, off = _pack([e[1] for e in entries])
    res = eng.inflate_batch(data, off, [e[2] for e in entries], check=False, zdicts=dicts, dict_of=dict_of)
    _check_batch(oracle, entries, lambda i: entries[i][3], res)


def test_corpus_size_only(eng, oracle):
    """FLATE_HIP_SIZE_ONLY: the size up to the end or the error, the status and the error offset of an unlimited
    output."""
    bad, total = [], 0
    for with_dict in (False, True):  # the plain call, and the dictionary build
        entries = _mixed([e for e in _entries() if bool(e[3]) == with_dict])
        data, off = _pack([e[1] for e in entries])
        if with_dict:
            dicts = sorted({e[3] for e in entries if e[3]}, key=len)
            dict_of = [dicts.index(e[3]) if e[3] else NO_DICT for e in entries]
            olen, status, err = eng.inflate_sizes(data, off, zdicts=dicts, dict_of=dict_of)
        else:
            olen, status, err = eng.inflate_sizes(data, off)
        total += len(entries)
        for i, (name, stream, _, zd) in enumerate(entries):
            rc, want, _, eoff = oracle.inflate(stream, 1 << 17, full=True, zdict=zd or None)
            have = (int(status[i]), int(err[i]), int(olen[i]))
            if have != (STATUS_OF_ORACLE[rc], eoff, len(want)):
                bad.append((name, have, (STATUS_OF_ORACLE[rc], eoff, len(want))))
    assert not bad, "%d of %d streams differ from the oracle, first: %s" % (len(bad), total, bad[:12])


# ---- the piecewise stream decoder (flate_hip_inflate_stream_*): no output slot, its end code is STREAM_END ----

@pytest.fixture(scope="module")
def stream_eng():
    flate.build()
    e = flate.FlateEngine(0)
    yield e
    e.close()


def _pieces(eng, data, cut, zdict, room):
    """data[:cut] without final_in, then the rest with it; then calls without input until the decoder ends.
    Returns (out, status, err_off, input consumed)."""
    r = eng.open_inflate_stream(zdict or None)
    try:
        outs = []
        o, rc = r.feed(data[:cut], final=False, room=room)
        outs.append(o.tobytes())
        if rc == 0:
            o, rc = r.feed(data[cut:], final=True, room=room)
            outs.append(o.tobytes())
        calls = 0
        while rc == 0:
            calls += 1
            assert calls < 100000, "no progress"
            o, rc = r.feed(b"", final=True, room=room)
            outs.append(o.tobytes())
        return b"".join(outs), rc, r.err_off, r.total_in
    finally:
        r.free()


def test_corpus_piecewise(stream_eng, oracle):
    """Whole input with final_in, and two pieces that break one byte before, at and one byte after the point where
    the oracle fails or ends, for every base case and every case behind a prefix block; small outputs also taken
    seven bytes at a time."""
    entries = [(c.name, c.data, c.zdict) for c in D.CASES]
    entries += [(n, d, z) for n, d, _, z in D.variants() if "/prefix" in n]
    bad, runs = [], 0
    for name, data, zd in entries:
        rc0, want, used0, eoff0 = oracle.inflate(data, 1 << 17, full=True, zdict=zd or None)
        want_rc = STREAM_END if rc0 == 0 else STATUS_OF_ORACLE[rc0]
        point = eoff0 if rc0 == D.E_CORRUPT else used0
        cuts = sorted({len(data), max(point - 1, 0), point, min(point + 1, len(data))})
        rooms = [len(want) + 64] + ([7] if len(data) < 200 else [])
        for cut in cuts:
            for room in rooms:
                got, rc, eoff, used = _pieces(stream_eng, data, cut, zd, room)
                runs += 1
                if (rc, eoff, len(got)) != (want_rc, eoff0, len(want)) or got != want or (rc0 == 0 and used != used0):
                    bad.append((name, cut, room, (rc, eoff, len(got), used), (want_rc, eoff0, len(want), used0)))
    assert not bad, "%d of %d piecewise runs differ from the oracle, first: %s" % (len(bad), runs, bad[:12])
