"""Input BYTES for the dense batch's chase (lz77_stream, moonbit-flate_amd/csrc/lz77_kernels.hip): streams whose
dense batches hold runs of back-to-back short matches, so that the two-event chase (lz77_chase_rule.h) meets pairs,
pairs whose second event needs the general path, single events and the end of the window.  TEST INFRASTRUCTURE: a
stream is data from a seeded generator and states no expected tokens; tests/test_lz77_chase_inputs.py shows on the CPU
model which paths the streams reach, tests/test_gpu_lz77_chase.py compares the kernels' bytes with the oracle's.

A stream is words of a small vocabulary (4 .. 15 bytes each, so a word seen before is one fast match), written
back to back or with one to three fresh bytes between them, and interleaved with
 * phrases: 16 .. 60 bytes copied from further back (a match of 16 or more needs the general path),
 * echoes: a word written twice within 64 bytes (two lanes of one batch then share a table slot),
and it ends with a word, so that the last match runs into the end of the window."""
import numpy as np

W = 65535


def vocabulary(rng, words=24):
    return [rng.integers(0, 256, int(rng.integers(4, 16)), dtype=np.uint8).tobytes() for _ in range(words)]


def stream(n, seed, vocab=None):
    """n bytes; the first pass over the vocabulary plants the words, everything behind it matches."""
    rng = np.random.default_rng(seed)
    vocab = vocab or vocabulary(rng)
    out = bytearray()
    for w in vocab:  # plant every word once, a fresh byte between them
        out += w + bytes([int(rng.integers(0, 256))])
        if len(out) >= n // 3:
            break
    while len(out) < n:
        r = int(rng.integers(0, 100))
        if r < 62:  # a run of words back to back
            for _ in range(int(rng.integers(2, 9))):
                out += vocab[int(rng.integers(0, len(vocab)))]
        elif r < 74:  # fresh bytes between two words
            out += rng.integers(0, 256, int(rng.integers(1, 4)), dtype=np.uint8).tobytes()
        elif r < 88 and len(out) > 80:  # a phrase from further back
            ln = int(rng.integers(16, 61))
            at = int(rng.integers(0, len(out) - ln))
            out += out[at:at + ln]
        else:  # an echo: the same word twice, a few bytes apart
            w = vocab[int(rng.integers(0, len(vocab)))]
            out += w + rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes() + w
    tail = vocab[seed % len(vocab)]
    out = out[:n - len(tail)] + tail  # the last match ends where the window does
    return bytes(out[:n])


# 128 is the shortest stream that enters the match finder; 192 / 256 are one and two batches, the others lie around them
SMALL_LENGTHS = [128, 129, 143, 160, 191, 192, 193, 255, 256, 257, 300, 383, 500, 640, 1000, 1500, 2048, 3000, 4096]


def small_streams(count, seed=1):
    """`count` streams of SMALL_LENGTHS (cycled), one vocabulary per eight streams."""
    rng = np.random.default_rng(seed)
    vocabs = [vocabulary(rng, 12 + 4 * (i % 4)) for i in range((count + 7) // 8)]
    return [stream(SMALL_LENGTHS[i % len(SMALL_LENGTHS)], seed * 100003 + i, vocabs[i // 8]) for i in range(count)]


def two_window_streams(count, seed=2):
    """Two full windows and a few hundred bytes: 131 070 + 128 .. + 128 + 97 * count."""
    return [stream(2 * W + 128 + 97 * i, seed * 100003 + i) for i in range(count)]


def batch(streams):
    off = np.zeros(len(streams) + 1, np.uint64)
    np.cumsum(np.array([len(s) for s in streams], dtype=np.uint64), out=off[1:])
    return np.frombuffer(b"".join(streams) + b"\0" * 16, np.uint8).copy(), off
