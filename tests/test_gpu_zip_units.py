"""flate_hip_zip_read with the option "zip_unit_min": long entries decoded through units.  The contract is equality with
the same call at option 0, word for word and byte for byte (the slot of an entry whose status is not 0 excepted), and
flate_hip_zip_last_route says which path ran.  Expectations come from Python's zipfile, from zip_ref.read_entry, from
the CPU walks of one_ref / stored_ref (the unit counts) and from the option-0 call.  The archives are zip_ref's writer
around raw streams of one_ref.deflate; none is above about 1.5 MB, and every input is good or merely malformed."""
import io
import struct
import zipfile
import zlib

import numpy as np
import pytest

import gzip_ref
import one_ref
import one_window_corpus
import stored_ref
import zip_ref as ref
from test_gpu_zip import GUARD, check_read, zread
from util import flate, force_inflate_config

pytestmark = pytest.mark.gpu

_cache = {}


@pytest.fixture(scope="module")
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


def archive_of(items, names=None):
    """zip_ref's archive around (raw, plain) pairs; plain None: a method-0 entry whose data is raw."""
    names = names or [b"e%d" % k for k in range(len(items))]
    raws = [r for r, _ in items]
    plains = [r if p is None else p for r, p in items]
    f, _ = ref.write_archive(raws, names, [zlib.crc32(p) for p in plains], [len(p) for p in plains])
    ix = ref.Index(f)
    for e, (_, p) in zip(ix.entries, items):
        if p is None:  # method 0 in the local header and in the directory
            f = ref._patch(f, e.header_off + 8, "<H", 0)
            f = ref._patch(f, e.name_off - 46 + 10, "<H", 0)
    return f


def streams():
    """name -> (raw, plain): computed once."""
    if "streams" not in _cache:
        t = gzip_ref.text(300000, seed=21)
        r = gzip_ref.rand(70000, seed=8)
        mixed = t[:100000] + r + t[100000:200000]
        _cache["streams"] = {
            "many": (one_ref.deflate(t, 6, mem=1), t),
            "level6": (one_ref.deflate(t, 6), t),
            "random": (one_ref.deflate(r, 6), r),
            "mixed": (one_ref.deflate(mixed, 6), mixed),
            "one unit": (one_ref.deflate(t[:5000], 9), t[:5000]),
            "empty": (one_ref.deflate(b"", 6), b""),
            "stored": (t[:777], None),
        }
        assert one_ref.Walk(_cache["streams"]["many"][0]).n_units >= 8
    return _cache["streams"]


ORDER = ["many", "stored", "level6", "random", "empty", "mixed", "one unit"]


def main_archive():
    """The seven streams under names of 1, 2, 255 and 300 bytes, so that data_off takes every alignment."""
    if "main" not in _cache:
        S = streams()
        names = [[b"a", b"\xc3\xa4", b"%03d" % k + b"x" * 252, b"%02d" % k + b"y" * 298][k % 4] for k in range(len(ORDER))]
        assert sorted({len(n) for n in names}) == [1, 2, 255, 300]
        f = archive_of([S[k] for k in ORDER], names)
        assert len(f) < 1500000 and len({e.data_off % 4 for e in ref.Index(f).entries}) >= 3
        _cache["main"] = f
    return _cache["main"]


def units_of(name, stored):
    key = ("units", name, stored)
    if key not in _cache:
        raw = streams()[name][0]
        _cache[key] = stored_ref.Walk(raw, stored=True).n_units if stored else one_ref.Walk(raw).n_units
    return _cache[key]


def read_both(eng, f, unit_min=1, **kw):
    """The same read with the option at 0 and at unit_min: every result word equal, the image equal outside the
    slots of entries whose status is not 0 -> (the route, the option-on results)."""
    eng.set_option("zip_unit_min", 0)
    off = zread(eng, f, **kw)
    assert eng.zip_last_route() == (0, 0, 0, 0)
    eng.set_option("zip_unit_min", unit_min)
    try:
        on = zread(eng, f, **kw)
        route = eng.zip_last_route()
    finally:
        eng.set_option("zip_unit_min", 0)
    assert (on[0], on[6], on[7]) == (off[0], off[6], off[7])
    for a, b in zip(on[2:6], off[2:6]):
        assert np.array_equal(a, b)
    img_on, img_off = on[1].copy(), off[1].copy()
    ix = ref.Index(f)
    if ix.rc == 0 and on[0] != ref.OUT_TOO_SMALL:
        sel = kw.get("sel")
        ns = len(sel) if sel is not None else ix.n_entries
        for j in range(ns):
            if int(on[4][j]) != 0:  # (empty, or as far as it came)
                img_on[int(on[2][j]):int(on[2][j + 1])] = 0
                img_off[int(on[2][j]):int(on[2][j + 1])] = 0
    assert np.array_equal(img_on, img_off)
    return route, on


# ---- equality and route ----

@pytest.mark.parametrize("stored_units", [0, 1])
def test_equality_and_route(eng, stored_units):
    f = main_archive()
    eng.set_option("one_stored_units", stored_units)
    try:
        deflated = [k for k in ORDER if streams()[k][1] is not None]
        want_units = sum(units_of(k, stored_units) for k in deflated)
        for device, shift in [(False, 0)] + [(True, s) for s in range(4)]:
            route, _ = read_both(eng, f, device=device, shift=shift, out_shift=(3 - shift) if device else 0)
            assert route[:3] == (len(deflated), 0, want_units), (device, shift, route)
            assert route[3] >= want_units - len(deflated)
        eng.set_option("zip_unit_min", 1)
        out, ooff, st = check_read(eng, "main", f, device=True, shift=1, out_shift=2)
        z = zipfile.ZipFile(io.BytesIO(f))
        for j, zi in enumerate(z.infolist()):
            assert out[int(ooff[j]):int(ooff[j + 1])].tobytes() == z.read(zi)
        assert eng.zip_last_route()[0] == len(deflated)
    finally:
        eng.set_option("one_stored_units", 0)
        eng.set_option("zip_unit_min", 0)


def test_option_values(eng):
    with pytest.raises(flate.FlateError):
        eng.set_option("zip_unit_min", -1)
    eng.set_option("zip_unit_min", 1 << 40)
    eng.set_option("zip_unit_min", 0)


# ---- the threshold ----

def test_threshold_edge(eng):
    f = main_archive()
    sizes = sorted(e.comp_size for e in ref.Index(f).entries if e.method == 8)
    for v in sizes:
        at, _ = read_both(eng, f, unit_min=v, device=True)
        above, _ = read_both(eng, f, unit_min=v + 1, device=True)
        assert at[0] == sum(1 for s in sizes if s >= v) and above[0] == sum(1 for s in sizes if s > v)
        assert at[1] == above[1] == 0


# ---- selections ----

def test_selection(eng):
    f = main_archive()
    n = len(ORDER)
    route, _ = read_both(eng, f, sel=list(range(n))[::-1], device=True, shift=1)
    assert route[:2] == (n - 1, 0)
    route, _ = read_both(eng, f, sel=[5, 0, 1], device=True, out_shift=1)
    assert route[:2] == (2, 0) and route[2] == units_of("mixed", 0) + units_of("many", 0)
    route, on = read_both(eng, f, sel=[2, 0, 2, 6, 2], device=True)
    assert route[:2] == (3, 2)  # a duplicate is the batch decoders'
    want = streams()["level6"][1]
    for j in (0, 2, 4):
        assert on[1][int(on[2][j]):int(on[2][j + 1])].tobytes() == want
    route, _ = read_both(eng, f, sel=[2, 0, 2, 6, 2])
    assert route[:2] == (3, 2)
    assert read_both(eng, f, sel=[], device=True)[0] == (0, 0, 0, 0)
    assert read_both(eng, f, sel=[1], device=True)[0] == (0, 0, 0, 0)  # the stored entry alone


# ---- size and capacity ----

def test_size_query_and_capacity(eng):
    f = main_archive()
    ix = ref.Index(f)
    route, on = read_both(eng, f, query=True)
    assert on[0] == ref.OUT_TOO_SMALL and on[2][:ix.n_entries + 1].tolist() == ix.out_off and route == (0, 0, 0, 0)
    route, on = read_both(eng, f, device=True, cap=ix.out_bytes - 1)
    assert on[0] == ref.OUT_TOO_SMALL and (on[1] == GUARD).all() and route == (0, 0, 0, 0)


# ---- history ----

def window_archive():
    if "window" not in _cache:
        items, total = [], 0
        for what, raw, plain, _ in one_window_corpus.good_streams():
            if total + len(raw) > 1300000:
                continue
            items.append((raw, plain))
            total += len(raw)
        assert len(items) >= 8
        _cache["window"] = archive_of(items)
    return _cache["window"]


def test_history_across_unit_borders(eng):
    f = window_archive()
    n = ref.Index(f).n_entries
    for device in (False, True):
        route, on = read_both(eng, f, device=device, shift=2 if device else 0)
        assert on[0] == 0 and route[:2] == (n, 0) and route[2] > n
    eng.set_option("zip_unit_min", 1)
    try:
        check_read(eng, "window", f, device=True, shift=3, out_shift=1)
    finally:
        eng.set_option("zip_unit_min", 0)


def test_history_never_crosses_an_entry(eng):
    legal, plain, illegal = one_ref.history_pair()
    S = streams()
    # the illegal stream's first far distance reaches one byte in front of its own first byte, where another entry's
    # bytes lie in `out`
    f = archive_of([S["one unit"], (legal, plain), (illegal, plain), S["many"], S["level6"]])
    for device in (False, True):
        route, on = read_both(eng, f, device=device, shift=1 if device else 0)
        assert [int(s) for s in on[4][:5]] == [0, 0, ref.CORRUPT, 0, 0]
        assert route[0] == 2 and route[1] >= 1
        for j, k in ((3, "many"), (4, "level6")):
            assert on[1][int(on[2][j]):int(on[2][j + 1])].tobytes() == S[k][1]


# ---- hostile entries ----

def hostile_archives():
    S = streams()
    many, text = S["many"]
    base = archive_of([S["one unit"], S["many"], S["level6"]])
    ix = ref.Index(base)
    rec = [e.name_off - 46 for e in ix.entries]
    e1 = ix.entries[1]
    out = [
        ("a stream cut short", ref._patch(base, rec[1] + 20, "<I", e1.comp_size - 3)),
        ("a wrong CRC", ref._patch(base, rec[1] + 16, "<I", e1.crc32 ^ 1)),
        ("a size too small", ref._patch(base, rec[1] + 24, "<I", e1.size - 1)),
        ("a size too large", ref._patch(base, rec[1] + 24, "<I", e1.size + 1)),
    ]
    # BFINAL well in front of comp_size: the bytes behind it are not examined
    junk = archive_of([S["one unit"], (many + gzip_ref.rand(5000, seed=3), text), S["level6"]])
    out.append(("BFINAL well in front of comp_size", junk))
    # two records over the same data: the second record's header offset is the first's
    two = archive_of([S["many"], S["many"], S["one unit"]])
    jx = ref.Index(two)
    two = ref._patch(two, jx.entries[1].name_off - 46 + 42, "<I", jx.entries[0].header_off)
    assert ref.Index(two).entries[1].data_off == ref.Index(two).entries[0].data_off
    out.append(("two records over the same data", two))
    # a local header and a complete inner stream inside the stored blocks of a deflated entry
    inner = ref.local_header(b"decoy", 0, 10, 10) + one_ref.deflate(text[:9000], 6) + b"PK\3\4" + text[:300]
    out.append(("a local header and a stream inside stored blocks",
                archive_of([S["one unit"], (one_ref.deflate(inner, 0), inner), S["level6"]])))
    what, raw, plain = one_ref.decoy_streams()[3]
    out.append((what, archive_of([(raw, plain), S["one unit"]])))
    return out


def test_hostile_entries_equal_the_batch_path(eng):
    for k, (what, f) in enumerate(hostile_archives()):
        for device in (False, True):
            route, on = read_both(eng, f, device=device, shift=k % 4 if device else 0)
            assert route[0] + route[1] == 3 or "stored blocks" in what or "phase" in what, (what, route)
        if what in ("a stream cut short",):
            assert int(on[4][1]) == ref.UNEXPECTED_EOF and route[1] >= 1
        if what == "two records over the same data":
            assert route[:2] == (1, 2) and on[0] == 0
        if what == "BFINAL well in front of comp_size":
            assert on[0] == 0 and route[:2] == (3, 0)
    for what, f, bad, status, err_off in ref.entry_cases():
        route, on = read_both(eng, f, device=True)
        assert int(on[4][bad]) == status, what
        read_both(eng, f, sel=[2, bad, 1, bad], device=True)


def test_a_unit_above_one_unit_max(eng):
    f = main_archive()
    eng.set_option("one_unit_max", 20000)  # "level6" and "random" hold units that span more
    try:
        route, on = read_both(eng, f, device=True)
        assert on[0] == 0 and route[1] >= 1 and route[0] >= 1
    finally:
        eng.set_option("one_unit_max", 1 << 28)


# ---- rounds ----

def test_rounds_of_two_units(eng):
    S = streams()
    # 1 + 2 units in front: a round edge falls on an entry edge; "many" spans rounds
    two_units = one_ref.deflate(S["many"][1][:40000], 6, mem=1)
    n2 = one_ref.Walk(two_units).n_units
    f = archive_of([S["one unit"], (two_units, S["many"][1][:40000]), S["many"], S["one unit"], S["level6"]])
    eng.set_option("one_round_units", 2)
    try:
        for device in (False, True):
            route, on = read_both(eng, f, device=device, shift=3 if device else 0)
            assert on[0] == 0 and route[:2] == (5, 0)
            assert route[2] == 2 * units_of("one unit", 0) + n2 + units_of("many", 0) + units_of("level6", 0)
    finally:
        eng.set_option("one_round_units", 4096)


# ---- the fallback under every decoder ----

@pytest.mark.parametrize("config", ["wave_per_stream", "lane_per_stream", "speculative_wave_small_batch"])
def test_fallback_decoder(config):
    e = force_inflate_config(flate.FlateEngine(0), config)
    try:
        what, f = hostile_archives()[0]  # the middle entry is cut short: it and the entry behind it fall back
        route, on = read_both(e, f, device=True, shift=1)
        assert route[:2] == (1, 2) and [int(s) for s in on[4][:3]] == [0, ref.UNEXPECTED_EOF, 0]
        assert on[1][int(on[2][2]):int(on[2][3])].tobytes() == streams()["level6"][1]
        route, on = read_both(e, main_archive(), unit_min=60000)
        assert on[0] == 0 and route[0] >= 2
    finally:
        e.close()


# ---- context reuse ----

def test_context_reuse(eng):
    f = main_archive()
    g = hostile_archives()[0][1]

    def call(e, v, arc):
        e.set_option("zip_unit_min", v)
        try:
            return zread(e, arc, device=True, shift=1), e.zip_last_route()
        finally:
            e.set_option("zip_unit_min", 0)

    def same(a, b):
        return a[1] == b[1] and a[0][0] == b[0][0] and all(np.array_equal(x, y) for x, y in zip(a[0][1:6], b[0][1:6]))

    fresh = {}
    for v, arc, key in ((1, f, "on f"), (0, f, "off f"), (1, g, "on g")):
        e = flate.FlateEngine(0)
        try:
            fresh[key] = call(e, v, arc)
        finally:
            e.close()
    for v, arc, key in ((1, f, "on f"), (0, f, "off f"), (1, g, "on g"), (1, f, "on f"), (1, f, "on f")):
        assert same(call(eng, v, arc), fresh[key]), key
