"""The match finder's progress guard on the CPU (tests/host_model/lz77_guard_model.cpp restates the rule of
lz77_stream, moonbit-flate_amd/csrc/lz77_kernels.hip): a dense batch made no progress if it ends with s where it found
it, not sparse and not done; a sparse batch that goes on must add at least one probe to e_idx.

A guard that fires on a healthy parser fails calls that are fine, and one that misses a stall leaves a wavefront
spinning for ever, so both directions are shown here, without a GPU: the rule never fires on the edge corpus
(tests/lz77_corpus.py) or on the fuzz set of tests/test_wave_model.py -- where the model's tokens are the oracle's, so
the statement is about the kernel's algorithm -- and it fires on every chunk whose k-th dense batch forgets what it did
(the kernel's debug_stall_batch hook), including a batch that had turned sparse, leaving only records the healthy run
has too.  The model also keeps the snapshot rule this guard replaced and counts disagreements between the two."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lz77_corpus as Z
from util import make_streams

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host_model", "lz77_guard_model.cpp")
LIB = os.path.join(HERE, "host_model", "liblz77_guard_model.so")
KINDS = ["text", "low", "period", "runs", "rand", "zero", "ramp"]  # tests/test_wave_model.py


@pytest.fixture(scope="module")
def model():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < os.path.getmtime(SRC):
        tmp = "%s.%d.tmp" % (LIB, os.getpid())
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", SRC, "-o", tmp])
        os.replace(tmp, LIB)
    L = C.CDLL(LIB)
    L.guard_model_lz77.argtypes = [C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.guard_model_lz77.restype = C.c_int
    return L


class Run:
    pass


def run(model, data, go=False, tags=False, multi=False, stall=0):
    sb = np.frombuffer(bytes(data), np.uint8)
    chunks = Z.lz_chunks(sb.size)
    nch = max(len(chunks), 1)
    pad = np.concatenate([sb, np.zeros(64, np.uint8)])
    recs = np.zeros((nch * 16384, 2), np.uint32)
    nm = np.zeros(nch, np.uint32)
    out = np.zeros(4, np.uint64)
    flags = (1 if go else 0) | (2 if tags else 0) | (4 if multi else 0)
    assert model.guard_model_lz77(pad.ctypes.data, sb.size, flags, stall, recs.ctypes.data, nm.ctypes.data,
                                  out.ctypes.data) == len(chunks)
    r = Run()
    r.recs = [recs[k * 16384:k * 16384 + int(nm[k])].copy() for k in range(len(chunks))]
    r.tokens = [Z.tokens_from_matches(sb[s:s + n], rr[:, 0], rr[:, 1]) for (s, n), rr in zip(chunks, r.recs)]
    r.dense, r.sparse, r.fired, r.disagree = (int(x) for x in out)
    return r


def healthy(model, oracle, name, data, go):
    want = Z.oracle_tokens(oracle, data, go)
    for multi in (False, True):
        for tags in (False, True):
            m = run(model, data, go=go, tags=tags, multi=multi)
            assert Z.same_tokens(m.tokens, want), (name, go, multi, tags)
            assert m.fired == 0 and m.disagree == 0, (name, go, multi, tags, m.fired, m.disagree)


@pytest.mark.parametrize("go", [False, True], ids=["default", "go"])
def test_the_guard_never_fires_on_the_corpus(model, oracle, go):
    for name, data in Z.cases():
        healthy(model, oracle, name, data, go)


@pytest.mark.parametrize("seed", range(6))
def test_the_guard_never_fires_on_the_fuzz_set(model, oracle, seed):
    rng = np.random.default_rng(seed)  # the streams of test_wave_model.test_model_fuzz
    specs = [(KINDS[int(rng.integers(0, len(KINDS)))], int(rng.integers(128, 140000))) for _ in range(25)]
    data, off = make_streams(specs, seed=seed)
    for i, (kind, n) in enumerate(specs):
        healthy(model, oracle, (kind, n), data[int(off[i]):int(off[i + 1])].tobytes(), bool(seed & 1))


STALLED = [("text", 65536), ("text", 200000), ("zero", 65536), ("ramp", 70000), ("rand", 65536), ("rand", 140000),
           ("runs", 129), ("text", 128)]


@pytest.mark.parametrize("multi", [False, True], ids=["plain", "modular"])
def test_the_guard_always_fires_on_a_stalled_batch(model, multi):
    data, off = make_streams(STALLED, seed=7)
    for i, (kind, n) in enumerate(STALLED):
        sb = data[int(off[i]):int(off[i + 1])].tobytes()
        ref = run(model, sb, multi=multi)
        nch = len(Z.lz_chunks(n))
        assert ref.fired == 0 and nch >= 1
        # the first batch of every chunk is a dense one (on incompressible bytes it is the batch that turns sparse):
        # every chunk stalls, every chunk is abandoned
        first = run(model, sb, multi=multi, tags=True, stall=1)
        assert first.fired == nch and first.disagree == 0, (kind, n, first.fired)
        assert all(r.shape[0] == 0 for r in first.recs), (kind, n)
        for k in (2, 3, 50):
            m = run(model, sb, multi=multi, stall=k)
            assert m.disagree == 0, (kind, n, k)
            # a chunk with fewer than k dense batches never meets the hook and ends as the healthy run's does
            if kind in ("text", "zero", "ramp") and n >= 65536 and (k <= 3 or kind == "text"):
                assert m.fired == nch, (kind, n, k, m.fired)
            # an abandoned chunk keeps a prefix of the healthy chunk's records: nothing is replayed (the first chunk:
            # a later one starts from the table an abandoned chunk left, which is not the healthy run's)
            got, want = m.recs[0], ref.recs[0]
            assert got.shape[0] <= want.shape[0] and np.array_equal(got, want[:got.shape[0]]), (kind, n, k)
        # rand: the stalled batch is one that had turned sparse -- the hook un-does that too, and the guard fires
        if kind == "rand":
            assert ref.sparse > 0
