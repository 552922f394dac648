"""No call's result may depend on the calls before it on the same flate_hip_ctx.

The ~25 entry points share about sixty grow-only device buffers and clear almost none of them: every word a kernel reads
has to be written earlier in the same call.  Every test here runs scenarios of tests/ctx_reuse_scenarios.py -- one ABI
call each, with an expectation computed on the CPU alone -- in an order chosen to leave the worst possible contents
behind: other families, dirty twins (same counts, other sizes, offsets and verdicts), big twins (stale words behind the
arrays), failures that stop a call half way, option changes, open stream handles, a second engine.  Every assertion is
`scenario.run(eng, device) == scenario.expected`; there are no tolerances and predecessor calls are the only poison."""
import zlib

import pytest

import ctx_reuse_scenarios as sc
from util import flate

pytestmark = pytest.mark.gpu

PRIMARY = [f["X"] for f in sc.FAMILIES.values()]


@pytest.fixture(scope="module", autouse=True)
def bound(oracle):
    """Every expectation computed once, before the first engine exists."""
    sc.bind(oracle)
    for s in sc.TABLE:
        s.expected


def short(v):
    if isinstance(v, (bytes, tuple)) and len(v) > 12:
        return "%s of %d: %r..." % (type(v).__name__, len(v), v[:12])
    return repr(v)


def check(s, eng, device, before=()):
    """One call, equal to its expectation word for word; the message names the scenario, what ran before it and the
    first word that differs (never the whole tuples: they hold the delivered bytes)."""
    try:
        got, want = s.run(eng, device), s.expected
    except flate.FlateError as e:
        if e.code == -3:   # a HIP error: nothing more is started on this device
            pytest.exit("HIP failure in %s after %s: %s" % (s.name, before, e), returncode=3)
        raise
    if got == want:
        return
    where = "length %d != %d" % (len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            where = "word %d: got %s, expected %s" % (k, short(g), short(w))
            if isinstance(g, tuple) and isinstance(w, tuple) and len(g) == len(w):
                j = next(j for j in range(len(g)) if g[j] != w[j])
                where += "; first at index %d: %s != %s" % (j, short(g[j]), short(w[j]))
            break
    pytest.fail("%s (%s pointers) after %s: %s" % (s.name, "device" if device else "host",
                                                  ", ".join(str(b) for b in before) or "nothing (a fresh ctx)", where),
                pytrace=False)


@pytest.fixture
def eng():
    e = flate.FlateEngine(0)
    yield e
    e.close()


# ---- a. a fresh ctx: every buffer grows from empty inside the call ----

@pytest.mark.parametrize("s", sc.TABLE, ids=str)
def test_first_and_only_call_on_a_new_ctx(s):
    for device in (False, True):
        e = flate.FlateEngine(0)
        try:
            check(s, e, device)
        finally:
            e.close()


# ---- b. every ordered pair: Y directly in front of every X ----

@pytest.mark.parametrize("y", sc.TABLE, ids=str)
def test_every_scenario_directly_behind(eng, y):
    for k, x in enumerate(sc.GOOD):
        check(y, eng, k % 2 == 1, before=[sc.GOOD[k - 1]] if k else ())
        check(x, eng, k % 2 == 0, before=[y])


# ---- c. dirty twin and big twin ----

@pytest.mark.parametrize("family", sorted(sc.FAMILIES))
def test_twins_grow_and_shrink_the_used_part(family):
    f = sc.FAMILIES[family]
    seq = [f["dirty"], f["X"], f["big"], f["X"], f["dirty"], f["big"]]
    for order in (seq, [f["big"]] + seq):   # buffers grow in the middle; the used part of large buffers shrinks
        e = flate.FlateEngine(0)
        try:
            for k, s in enumerate(order):
                check(s, e, k % 2 == 0, before=order[max(k - 3, 0):k])
        finally:
            e.close()


# ---- d. after a failure ----

@pytest.mark.parametrize("bad", sc.FAILS, ids=str)
def test_the_call_after_a_failure(eng, bad):
    for k, x in enumerate(PRIMARY):
        check(bad, eng, k % 2 == 0, before=[PRIMARY[k - 1]] if k else ())
        check(x, eng, k % 3 == 0, before=[bad])
    other = sc.FAILS[(sc.FAILS.index(bad) + 7) % len(sc.FAILS)]
    own = sc.FAMILIES[bad.family]["X"]
    check(bad, eng, True)
    check(other, eng, False, before=[bad])
    check(own, eng, True, before=[bad, other])


@pytest.mark.parametrize("bad", [s for s in sc.FAILS if s.fail == "invalid"], ids=str)
def test_a_refusal_leaves_the_same_error_text_as_on_a_new_ctx(bad):
    def text(e):
        return e._L.flate_hip_last_hip_error(e._ctx).decode()

    fresh = flate.FlateEngine(0)
    used = flate.FlateEngine(0)
    fam = sc.FAMILIES[bad.family]
    # calls that really fail, the family's own first: a text they leave behind would show after the refusal
    failing = [s for s in fam["fail"].values() if s.fail != "invalid"] + [sc.BY_NAME["bgzf_read/fail_corrupt"],
                                                                          sc.BY_NAME["inflate_batch/fail_capacity"]]
    try:
        check(bad, fresh, False)
        for s in [fam["big"], fam["dirty"]] + failing:
            check(s, used, True)
        check(bad, used, False, before=failing)
        assert text(used) == text(fresh), (bad, text(used), text(fresh))
        assert used._L.flate_hip_strerror(-1).decode()
        check(fam["X"], used, True, before=[bad])
    finally:
        fresh.close()
        used.close()


# ---- e. seeded walks ----

def run_walk(eng, steps, tag):
    done = []
    for k, step in enumerate(steps):
        if step[0] == "option":
            sc.apply_option(eng, step[1], step[2])
            done.append("%s=%s" % step[1:])
            continue
        s = sc.BY_NAME[step[1]]
        check(s, eng, step[2], before=["%s, step %d, the three steps in front:" % (tag, k)] + done[-3:])
        done.append("%s (%s)" % (s.name, "device" if step[2] else "host"))


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_seeded_walk_over_the_whole_table(eng, seed):
    run_walk(eng, sc.walk(seed), "seed %d" % seed)


def test_walk_with_the_limits_that_a_caller_can_only_lower(eng):
    """"one_unit_max" and "gzip_member_max" lowered for the engine's life, to limits every scenario stays under."""
    eng.set_option("one_unit_max", 1 << 20)
    eng.set_option("gzip_member_max", 1 << 20)
    steps = [s for s in sc.walk(sc.SEEDS[0]) if s[0] == "call" or s[1] != "gzip_member_max"]
    run_walk(eng, steps, "lowered limits")


# ---- f. open handles across other calls ----

def test_open_stream_handles_across_other_calls(eng, oracle):
    W = flate.engine.MAX_STORE_BLOCK_SIZE
    data = flate.synth("text", 1, 3 * W + 1000, seed=91)
    plain = flate.synth("text", 1, 150000, seed=92).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    stream = c.compress(plain) + c.flush()
    other = flate.synth("text", 1, 40000, seed=93).tobytes()
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    abandoned = c.compress(other) + c.flush()
    between = [sc.BY_NAME[n] for n in ("deflate_spliced/x", "deflate_batch/dirty", "zip_write/x", "bgzf_write/big",
                                       "inflate_batch/x", "gzfile_read/x", "deflate_spliced/big", "inflate_framed_gzip/dirty",
                                       "inflate_one/x", "deflate_framed_zlib_dict/x", "zip_read/x", "gzip_read/big")]
    w, r = eng.open_stream(), eng.open_inflate_stream()
    written, read, k = [], [], 0

    def interleave():
        nonlocal k
        check(between[k % len(between)], eng, k % 2 == 0, before=["a write or a feed on an open handle"])
        k += 1

    # the reader first decodes a part of another stream and is reset in the middle of it
    got, rc = r.feed(abandoned[:len(abandoned) // 2], room=1 << 20)
    assert rc == 0 and got.tobytes() == other[:len(got)]
    interleave()
    r.reset()
    pieces = [stream[i:i + 9000] for i in range(0, len(stream), 9000)]
    for i in range(3):
        written.append(w.write(data[i * W:(i + 1) * W]).tobytes())
        interleave()
    for i, p in enumerate(pieces):
        got, rc = r.feed(p, final=i == len(pieces) - 1, room=1 << 20)
        read.append(got.tobytes())
        assert rc == (1 if i == len(pieces) - 1 else 0), (i, rc)
        interleave()
    written.append(w.close(data[3 * W:]).tobytes())
    r.free()
    assert b"".join(written) == oracle.deflate(data), "the writer's bytes differ from the oracle's on the whole input"
    assert b"".join(read) == plain, "the reader's bytes differ from zlib's"
    check(sc.BY_NAME["deflate_spliced/x"], eng, False, before=["the handles' last calls"])


# ---- g. two engines on one device, in lock-step from one thread ----

def test_two_engines_alternating_and_a_third_in_freed_memory():
    a, b = flate.FlateEngine(0), flate.FlateEngine(0)
    c = None
    try:
        half = len(sc.TABLE) // 2
        for k, s in enumerate(sc.TABLE):
            if k == half:   # a new ctx may be handed the memory A just freed
                a.close()
                a = c = flate.FlateEngine(0)
            e = a if k % 2 else b
            check(s, e, k % 4 < 2, before=["engine %s, lock-step with another" % ("B" if e is b else "C" if e is c else "A")])
    finally:
        a.close()
        b.close()
