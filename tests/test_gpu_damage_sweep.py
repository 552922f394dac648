"""The damage sweep of the unit decoders on the GPU: every path behind flate_hip_inflate_one_index on the damaged
multi-unit streams of tests/damage_corpus.py.  Every expectation comes from that corpus -- the oracle (status, err_off,
out_len, the bytes), one_ref.Walk (units, reach), zlib -- and from the CPU references built on them (seek_ref,
gzfile_ref, one_parts_ref); none comes from another call of the library, and every comparison is exact.  Container
kind, pointer side and address shift rotate with the stream's index.  Every call is held against FLATE_HIP_E_HIP
(-3) with the runtime's text; device-pointer calls decode into 0xA5-prefilled buffers between guard regions (the
helpers of the existing tests, reused here, assert that nothing outside out[0, out_len) changed)."""
import collections

import numpy as np
import pytest

import damage_corpus as D
import gzfile_ref
import one_parts_ref as R
import one_ref as ref
import seek_ref as sk
import util
from test_gpu_gzfile import check_index as gz_check_index, read as gz_read
from test_gpu_inflate_one import index
from test_gpu_inflate_one_read import read as read_one
from test_gpu_one_parts import fixed, reader
from test_gpu_one_seek import GUARD, GUARD_WORD, build as seek_build, read as seek_read
from util import flate

pytestmark = pytest.mark.gpu

KINDS = (ref.RAW, ref.ZLIB, ref.GZIP)
SHIFTS = (0, 1, 3)
SAME_LENGTH = ("header", "eob", "body", "stored", "overwrite")
CLASSES = ("corrupt", "eof", "valid_same_bytes", "valid_other_bytes", "history_only", "past_header", "other_chain",
           "good_units_behind_damage", "later_unit", "stored_header")
# the issue's minima per class: a thinned rotation keeps at least a tenth of each
MINIMA = {"past_header": 150, "other_chain": 30, "valid_other_bytes": 200, "eof": 25, "history_only": 8, "later_unit": 100,
          "stored_header": 10}


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def corpus(oracle):
    assert D.STATUS_OF_ORACLE == util.STATUS_OF_ORACLE
    return D.corpus(oracle)


def hip(eng, rc, what):
    """FLATE_HIP_E_HIP ends the session: nothing more is started on a card after a call that failed in the runtime."""
    if rc == -3:
        pytest.exit("%s: HIP failure: %s" % (what, eng._L.flate_hip_last_hip_error(eng._ctx).decode()), returncode=3)
    return rc


def rotation(i):
    """(kind, device pointers, address shift) of stream i."""
    return KINDS[i % 3], (i // 3) % 2 == 1, SHIFTS[(i // 6) % 3]


def keeps_a_tenth(cases):
    got = D.counts(cases)
    for flag, least in MINIMA.items():
        assert 10 * got[flag] >= least, (flag, got[flag], least)


# ---- flate_hip_inflate_one_index ----

def test_index_of_every_stream_is_the_walks(eng, corpus):
    for i, c in enumerate(corpus.cases):
        kind, device, shift = rotation(i)
        w, name = c.walk, c.damage.name
        rc, nu, ob, nc, st, eo, ubit, ooff = index(eng, ref.wrap(c.damage.raw, c.out, kind), kind, w.n_units, device=device,
                                                   shift=shift)
        hip(eng, rc, name)
        # (of a history_only stream the index says OK, as the walk does: the documented exception)
        assert (rc, st, eo, nu, ob) == (w.status, w.status, w.err_off, w.n_units, w.out_bytes), (name, kind, rc, st, eo, nu, ob)
        assert list(ubit[:nu + 1]) == w.unit_bit and list(ooff[:nu + 1]) == w.out_off, (name, kind)
        if kind == ref.RAW:
            assert nc >= w.n_units, (name, nc)


# ---- flate_hip_inflate_one ----

def check_one(eng, c, f, kind, want, i, units=True):
    _, device, shift = rotation(i)
    st_w, eo_w, out_w = want
    rc, got, ol, st, eo, nu, nc, _ = read_one(eng, f, kind, c.walk.out_len + 600, device=device, shift=shift, out_shift=shift)
    hip(eng, rc, c.damage.name)
    assert (rc, st, eo, ol) == (st_w, st_w, eo_w, len(out_w)), (c.damage.name, kind, rc, st, eo, ol, st_w, eo_w, len(out_w))
    assert got == out_w, (c.damage.name, kind)
    if units and st_w == 0:
        assert nu == c.walk.n_units, (c.damage.name, nu)


def test_inflate_one_raw_is_the_oracles(eng, corpus):
    for i, c in enumerate(corpus.cases):
        check_one(eng, c, c.damage.raw, ref.RAW, (c.status, c.err_off, c.out), i)


@pytest.mark.parametrize("kind", (ref.ZLIB, ref.GZIP))
def test_inflate_one_framed_in_two_framings(eng, corpus, kind):
    seen = collections.Counter()
    for i, c in enumerate(corpus.cases):
        if i % 3 != kind:
            continue
        base = corpus.bases[c.damage.base]
        for plain in (base.plain, c.out):  # the trailer of the base's plain; the trailer recomputed from the oracle's bytes
            f = ref.wrap(c.damage.raw, plain, kind)
            want = D.framed_expect(c, f)
            if c.status == 0 and plain is c.out:
                assert want[:2] == (0, -1)
            if "valid_other_bytes" in c.flags and plain is base.plain:
                assert want == (ref.CORRUPT, len(f), c.out)
                seen["trailer"] += 1
            check_one(eng, c, f, kind, want, i + (plain is c.out))
    assert seen["trailer"] >= 20


def test_inflate_one_raw_in_rounds_of_two_units(eng, corpus):
    picked = [(i, c) for i, c in enumerate(corpus.cases) if i % 2 == 1]  # (every stream took 15 s: every second one)
    keeps_a_tenth([c for _, c in picked])
    places = collections.Counter(c.walk.n_units % 2 for _, c in picked if c.walk.status)
    assert places[0] >= 20 and places[1] >= 20, places  # the failing unit is the first / the last of its round
    try:
        eng.set_option("one_round_units", 2)
        for i, c in picked:
            check_one(eng, c, c.damage.raw, ref.RAW, (c.status, c.err_off, c.out), i + 1)
    finally:
        eng.set_option("one_round_units", 4096)


def test_inflate_one_with_stored_headers_as_units(eng, corpus):
    """Base (b): bytes, status and err_off never change with "one_stored_units"; the units do, and are not asserted."""
    cases = [(i, c) for i, c in enumerate(corpus.cases) if c.damage.base == "b"]
    assert sum(1 for _, c in cases if "stored_header" in c.flags) >= 10
    try:
        eng.set_option("one_stored_units", 1)
        for i, c in cases:
            check_one(eng, c, c.damage.raw, ref.RAW, (c.status, c.err_off, c.out), i + 2, units=False)
    finally:
        eng.set_option("one_stored_units", 0)


# ---- flate_hip_one_reader_* in parts ----

PATTERNS = ("thirds", "one byte in front of the damaged byte", "at the damaged byte", "one byte behind the damaged byte",
            "at the reach of the unit in front")
# (every second stream with host and every fourth with device pointers took 12 to 35 s per pattern on one MI355X: thinned
# once, and the three boundaries around the damaged byte made cases of their own)
HOST_EVERY, DEVICE_EVERY = 4, 8


def cuts_of(c, base, pattern):
    """[first-part sizes] of one feeding pattern; every later part is whatever is left."""
    d, n = c.damage, len(c.damage.raw)
    if pattern == PATTERNS[0]:
        return [None]
    if pattern in PATTERNS[1:4]:
        p = d.at >> 3 if d.kind in ("header", "eob", "body", "stored") else d.at
        return [min(max(p + PATTERNS.index(pattern) - 2, 1), n)]
    return [min(base.walk.reach[d.unit - 1], n)]


def model_covers(c):
    """one_parts_ref.Model is built on the history-free walk: it covers every stream no distance of which reaches in
    front of the stream (valid, corrupt and cut ones alike), and none of the others."""
    return not c.walk.far


@pytest.mark.parametrize("pattern", PATTERNS)
def test_reader_in_parts_is_the_oracles(eng, corpus, pattern):
    picked = [(i, c) for i, c in enumerate(corpus.cases) if i % HOST_EVERY == 0]
    keeps_a_tenth([c for _, c in picked])
    keeps_a_tenth([c for i, c in picked if i % DEVICE_EVERY == 0])
    handles = {False: eng.open_one_reader("raw", device=False), True: eng.open_one_reader("raw", device=True)}
    uncovered = collections.Counter()
    try:
        for i, c in picked:
            raw, name = c.damage.raw, c.damage.name
            base = corpus.bases[c.damage.base]
            grow = max(len(raw) // 12, 1)
            covered = model_covers(c)
            if not covered:
                uncovered.update(c.flags & {"corrupt", "valid_other_bytes", "valid_same_bytes", "history_only", "eof"})
            for cut in cuts_of(c, base, pattern):
                sizes_of = (lambda: fixed(max(len(raw) // 3, 1))) if cut is None else (lambda: iter([cut]))
                want_calls = None
                if covered:
                    m = R.Model(raw, ref.RAW, walk=c.walk, plain=c.out)
                    want_calls, want, _ = R.feed(R.model_reader(m), raw, sizes_of(), None, 64, grow)
                    assert want == c.out, (name, "the model against the oracle")
                for device in ((False, True) if i % DEVICE_EVERY == 0 else (False,)):
                    rd = handles[device]
                    rd.reset()
                    calls, got, rest = R.feed(reader(rd, device, guard=device), raw, sizes_of(), None, 3 + 12 + 16, grow)
                    last = calls[-1]
                    for k in calls:
                        hip(eng, k.rc, name)
                    tag = (name, pattern, cut, device, last)
                    assert (0 if last.rc == R.STREAM_END else last.rc, last.err_off) == (c.status, c.err_off), tag
                    assert got == c.out and sum(k.out_len for k in calls) == len(c.out), tag
                    again = reader(rd, device, guard=device)(raw[:4], True, 64)  # sticky: the same status, no output
                    assert again == (R.Call(last.rc, 0, 0, 0, last.err_off), b""), tag
                    if want_calls is not None:
                        assert calls == want_calls, (tag, [(j, a, b) for j, (a, b) in enumerate(zip(calls, want_calls)) if a != b][:3])
    finally:
        for rd in handles.values():
            rd.close()
    print("reader in parts, %s: %d streams, not covered by one_parts_ref.Model: %s" % (pattern, len(picked), dict(uncovered)))
    assert uncovered["history_only"] >= 1  # (the classes the model does not cover are counted, not dropped: the oracle judges them)


# ---- flate_hip_inflate_one_seek_index ----

def test_seek_index_of_every_fourth_stream(eng, corpus):
    picked = [(i, c) for i, c in enumerate(corpus.cases) if i % 4 == 1]
    keeps_a_tenth([c for _, c in picked])
    chains = 0
    for i, c in picked:
        kind, device, shift = rotation(i)
        raw, name, w = c.damage.raw, c.damage.name, c.walk
        f = ref.wrap(raw, c.out, kind)
        if c.status:
            # (both sizes are judged in front of TAIL, from the history-free discovery: room for what the walk counts)
            words = len(sk.index_words(w, c.out, len(raw), kind, 4096)) if w.status == 0 else 64
            room = (len(sk.points(w.out_off, 4096)) - 1) * sk.WINDOW if w.status == 0 else 0
            g = seek_build(eng, f, kind, 4096, device=device, shift=shift, wshift=shift, words=words, room=room)
            hip(eng, g["rc"], name)
            assert (g["rc"], g["status"], g["err_off"]) == (c.status, c.status, c.err_off), (name, kind, g["rc"], g["status"], g["err_off"])
            assert (g["index_words"], g["windows_bytes"], g["n_points"]) == (0, 0, 0), name
            assert (g["index"] == GUARD_WORD).all(), (name, "a failing stream got index words")
            continue
        chains += "other_chain" in c.flags
        for span in (1, 4096) if "other_chain" in c.flags else (4096,):
            want = sk.index_words(w, c.out, len(raw), kind, span)  # ITS OWN walk's index
            pts = sk.points(w.out_off, span)
            wins = sk.windows(c.out, w.out_off, pts)
            g = seek_build(eng, f, kind, span, device=device, shift=shift, wshift=shift, words=len(want), room=len(wins))
            hip(eng, g["rc"], name)
            assert (g["rc"], g["status"], g["err_off"]) == (0, 0, -1), (name, kind, span, g["rc"], g["status"], g["err_off"])
            assert (g["index_words"], g["windows_bytes"], g["n_units"], g["n_points"], g["out_bytes"]) == \
                (len(want), len(wins), w.n_units, len(pts), len(c.out)), (name, kind, span)
            assert [int(x) for x in g["index"]] == want, (name, kind, span)
            assert g["windows"].tobytes() == wins, (name, kind, span)
    assert chains >= 3


# ---- flate_hip_inflate_one_ranges through the BASE's index ----

def range_cases(corpus):
    """About 40 same-length damages, five of every class, the bases in turn."""
    out, seen = [], set()
    for flag in CLASSES:
        took = collections.Counter()
        for i, c in enumerate(corpus.cases):
            if flag in c.flags and c.damage.kind in SAME_LENGTH and took[c.damage.base] < 2 and sum(took.values()) < 5 \
                    and i % 7 == len(flag) % 7 and c.damage.name not in seen:
                took[c.damage.base] += 1
                seen.add(c.damage.name)
                out.append((i, c))
    return out


def test_ranges_through_the_bases_index_on_a_damaged_stream(eng, corpus):
    cases = range_cases(corpus)
    got = D.counts([c for _, c in cases])
    assert len(cases) >= 30 and all(got[f] >= 2 for f in CLASSES if f != "eof"), (len(cases), got)  # (eof: cuts change the length)
    must_fail = bad_seen = clean_seen = 0
    for i, c in cases:
        _, device, shift = rotation(i)
        base = corpus.bases[c.damage.base]
        bw, d, name = base.walk, c.damage.unit, c.damage.name
        # a history-free failure inside the damaged unit's own bits: the piece decoder meets it too
        inside = c.status == ref.CORRUPT and c.walk.status == ref.CORRUPT and c.walk.err_off == c.err_off \
            and 8 * c.err_off <= bw.unit_bit[d + 1] and c.walk.n_units == d
        must_fail += inside
        for span in (1, 4096):
            pts = sk.points(bw.out_off, span)
            words = np.array(sk.index_words(bw, base.plain, len(base.raw), ref.RAW, span), np.uint64)
            wins = sk.windows(base.plain, bw.out_off, pts)
            ranges = sk.edge_ranges(bw.out_off, pts)
            begin, end = [r[0] for r in ranges], [r[1] for r in ranges]
            _, off_m, _, nd_m, _, data_m = sk.read(base.plain, bw.out_off, pts, begin, end)
            rc, off, st, nd, bad, body = seek_read(eng, c.damage.raw, ref.RAW, words, wins, begin, end, off_m[-1] + 32,
                                                   device=device, shift=shift, wshift=shift, out_shift=shift)
            hip(eng, rc, name)
            tag = (name, span, device)
            assert (off, nd) == (off_m, nd_m), tag
            assert (body[off[-1]:] == GUARD).all(), (tag, "bytes behind the total touched")
            for r, rng in enumerate(ranges):
                if d not in sk.decoded(bw.out_off, pts, [rng]):
                    # another segment, or in front of the damage: the damage must never change it
                    assert st[r] == 0 and body[off[r]:off[r + 1]].tobytes() == data_m[r], (tag, r, rng, st[r])
                    clean_seen += 1
                elif inside:
                    assert st[r] != 0, (tag, r, rng)
            if any(st):
                assert bad == d and rc != 0 and all(s in (0, rc) for s in st), (tag, bad, d, rc, sorted(set(st)))
                bad_seen += 1
            else:
                assert (rc, bad) == (0, sk.NO_UNIT), (tag, rc, bad)
    assert must_fail >= 3 and bad_seen >= 6 and clean_seen >= 1000, (must_fail, bad_seen, clean_seen)


# ---- flate_hip_gzfile_index / flate_hip_gzfile_read ----

def gzfile_cases(corpus):
    """About 60 damaged versions of base (a), ten of every class it has."""
    out, seen = [], set()
    for flag in CLASSES:
        took = 0
        for i, c in enumerate(corpus.cases):
            if c.damage.base == "a" and flag in c.flags and took < 10 and i % 5 == len(flag) % 5 and c.damage.name not in seen:
                took += 1
                seen.add(c.damage.name)
                out.append((i, c))
    return out


@pytest.fixture(scope="module")
def gzfiles(corpus, oracle):
    """[(name, i, file, gzfile_ref.Walk, verdict, delivered, history)]: computed once, shared, never changed."""
    three = gzfile_ref.three_members()
    base = corpus.bases["a"]
    out = []
    for i, c in gzfile_cases(corpus):
        for which, plain in (("the base's trailer", base.plain), ("the recomputed trailer", c.out)):
            if plain is c.out and c.out == base.plain:
                continue
            f = three[0][0] + gzfile_ref.wrap(c.damage.raw, plain) + three[2][0]
            w = gzfile_ref.Walk(f)
            out.append((c.damage.name + ", " + which, i, f, w) + D.gzfile_expect(oracle, f, w, three[0], three[2]))
    return out


@pytest.mark.parametrize("serial_max", (0, 1 << 20))
def test_gzfile_with_a_damaged_middle_member(eng, corpus, gzfiles, serial_max):
    got = D.counts([c for _, c in gzfile_cases(corpus)])
    assert len(gzfiles) >= 60 and all(got[f] >= 3 for f in CLASSES if f not in ("stored_header", "valid_same_bytes")), (len(gzfiles), got)
    verdicts = collections.Counter()
    try:
        eng.set_option("gzfile_serial_max", serial_max)
        for name, i, f, w, verdict, delivered, history in gzfiles:
            assert serial_max == 0 or serial_max > len(f)
            _, device, shift = rotation(i)
            if serial_max == 0 and not history:
                gz_check_index(eng, name, f, w, device=device, shift=shift)
            # (the total is known after the history-free discovery: room for what the walk counts, too)
            # with the option on, whole members behind a failure that only TAIL finds have been decoded by then: the
            # header leaves out[out_len, T) unspecified there, T the size the history-free discovery reports
            loose = w.out_len if serial_max and history and w.status == 0 else None
            rc, out, ol, words, nm, nu, body = gz_read(eng, f, max(len(delivered), w.out_len) + 100, device, shift=shift,
                                                       out_shift=shift, untouched_from=loose)
            hip(eng, rc, name)
            assert (rc, words) == (verdict[0], verdict), (name, serial_max, rc, words, verdict)
            assert ol == len(delivered) and out == delivered, (name, serial_max, ol, len(delivered))
            if verdict[0]:
                assert (body[ol if loose is None else loose:] == GUARD).all(), (name, "bytes behind the failure changed")
            if not history:
                assert nm == w.n_members, (name, nm, w.n_members)
                if serial_max == 0:
                    assert nu == w.n_units, (name, nu, w.n_units)
            verdicts[(verdict[0], verdict[1])] += 1
    finally:
        eng.set_option("gzfile_serial_max", 0)
    # the chain breaks in the middle member and behind it, a trailer fails, and files read cleanly
    assert verdicts[(ref.CORRUPT, 1)] >= 5 and verdicts[(0, gzfile_ref.NONE)] >= 5 and verdicts[(ref.CORRUPT, 2)] >= 1, verdicts
