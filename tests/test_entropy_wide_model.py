"""The eight-positions-per-lane tile walk and bit placement of the entropy stage (huff_pack_kernels.hip: walk_tile,
hist_block, pack_block, sink_place / sink_emit_pair), restated with numpy uint32 arithmetic (CPU only) and checked
  * against a position-by-position classification,
  * against the four-wide model of tests/test_tile_walk_model.py run on the tile's two 256-position halves with the
    cov_until each would see: the hand-over bytes (tile_meta) must be the same byte for byte,
  * for the rank of a match start from the two ballots, which is the record's index in the tile: register rank >> 6,
    lane rank & 63 of the two records every lane keeps in flight,
  * for the placement of a lane's two bit strings at every shift against Python's big-integer shift, and the bound
    on the ring the kernel's static_assert states."""
import numpy as np
import pytest

from test_tile_walk_model import byte_sum, udot4, walk_tile_model

TILE = 512
ROW = 256
M32 = np.uint64(0xffffffff)
ONES = np.uint64(0x01010101)


def low_bytes(t):   # 0x01 in the clamp04(t) lowest bytes
    t = np.clip(t, 0, 4).astype(np.uint64)
    return ((ONES << (np.uint64(8) * t)) >> np.uint64(32)) & M32


def lshl_add(x, s):  # v_lshl_add_u32 x, s, x
    return (x + (x << np.uint64(s))) & M32


def walk_wide_model(recs, P0, n, cov_until):
    """recs: ALL records from the walker's position on (pos, length), sorted, non-overlapping; the tile takes those
    below P0 + TILE.  Returns (meta[128] in position order, lit[128], start_k[128], rec_of[128], records taken,
    new cov_until) as the kernel computes them."""
    lane = np.arange(64)
    # two records in flight per lane: register 0 holds recs[lane], register 1 recs[64 + lane]
    reg = np.full((2, 64), 0xffffffff, np.int64)
    rlen = np.zeros((2, 64), np.int64)
    for i, (pos, ln) in enumerate(recs[:128]):
        reg[i >> 6][i & 63], rlen[i >> 6][i & 63] = pos, ln
    mine = reg < P0 + TILE
    cnt = int(mine[0].sum() + mine[1].sum())
    assert mine.reshape(-1)[:cnt].all() and not mine.reshape(-1)[cnt:].any()   # sorted: the first cnt of 128
    marks = np.zeros(TILE, np.uint8)   # 1: first covered position, 2: last covered position, 4: start
    for r in range(2):
        for L in range(64):
            if mine[r][L]:
                o, ln = int(reg[r][L]) - P0, int(rlen[r][L])
                for at, v in ((o, 4), (o + 1, 1), (o + ln - 1, 2)):
                    if at < TILE:
                        assert marks[at] == 0, "two marks on one position"   # plain byte stores
                        marks[at] = v
    m = marks.view("<u4").astype(np.uint64).reshape(64, 2)
    first, last = m & ONES, (m >> np.uint64(1)) & ONES
    tot0 = byte_sum(first[:, 0]).astype(np.int64) - byte_sum(last[:, 0]).astype(np.int64)
    tot = tot0 + byte_sum(first[:, 1]).astype(np.int64) - byte_sum(last[:, 1]).astype(np.int64)
    base0 = np.cumsum(tot) - tot               # ONE wave_incl_scan per tile
    base1 = base0 + tot0
    assert ((base0 == 0) | (base0 == 1)).all() and ((base1 == 0) | (base1 == 1)).all()
    pos = P0 + 8 * lane
    new_cov = cov_until
    if cnt:
        r, L = (cnt - 1) >> 6, (cnt - 1) & 63
        new_cov = int(reg[r][L] + rlen[r][L])
    meta = np.zeros(128, np.int64)
    lit_out = np.zeros(128, np.int64)
    start_k = np.full(128, -1)
    has = np.zeros((64, 2), bool)
    for h, base in ((0, base0), (1, base1)):
        low = low_bytes(cov_until - pos - 4 * h)
        act = low_bytes(n - pos - 4 * h)
        e = (first[:, h] + (np.uint64(1) << np.uint64(32)) - ((last[:, h] << np.uint64(8)) & M32)
             + base.astype(np.uint64)) & M32
        cov = lshl_add(lshl_add(e, 8), 16) | low
        assert ((cov & ~ONES) == 0).all()      # bytes are 0 or 1: no borrow, no carry
        start = (m[:, h] >> np.uint64(2)) & act
        lit = act & ~(cov | start) & M32
        b = udot4(lit, 0x08040201, udot4(start, 0x70503010))
        assert (b < 128).all()
        meta[h::2] = b.astype(np.int64)
        lit_out[h::2] = (b & np.uint64(15)).astype(np.int64)
        start_k[h::2] = np.where(b & np.uint64(16), (b >> np.uint64(5)).astype(np.int64), -1)
        has[:, h] = start != 0
    # the packer's rank: two ballots, the starts of the lanes below, plus the lane's own first half
    below = (np.cumsum(has[:, 0]) - has[:, 0]) + (np.cumsum(has[:, 1]) - has[:, 1])
    rank = np.stack([below, below + has[:, 0]], axis=1)
    rec_of = np.where(has, rank, -1).reshape(-1)
    for g in np.nonzero(rec_of >= 0)[0]:
        r = int(rec_of[g])
        assert r < cnt and reg[r >> 6][r & 63] == P0 + 4 * g + start_k[g]   # register rank >> 6, lane rank & 63
    return meta, lit_out, start_k, rec_of, cnt, new_cov


def classify(recs, n):
    """Position by position: 'L' literal, 'S' match start, 'C' covered."""
    kind = np.full(n, ord("L"), np.uint8)
    for pos, ln in recs:
        kind[pos] = ord("S")
        kind[pos + 1:pos + ln] = ord("C")
    return kind


def narrow_meta(recs_of_half, P0, n, cov_until):
    lit_mask, match_k, rec_of = walk_tile_model(recs_of_half, P0, n, cov_until)
    return lit_mask | np.where(match_k >= 0, 16 | (match_k << 5), 0), rec_of


def run_chunk(recs, n):
    """The walk of hist_block over a chunk of n positions: checks every tile against the four-wide model and the
    whole chunk against the classification.  Returns the meta bytes of the block's own rows."""
    for (p, ln), (q, _) in zip(recs, recs[1:]):
        assert ln >= 4 and p + ln <= q
    assert not recs or recs[-1][0] + recs[-1][1] <= n
    kind = classify(recs, n)
    rows = -(-n // ROW)
    out = np.full(rows * 64, -1, np.int64)
    mp, cov, cov4 = 0, 0, 0
    for P0 in range(0, n, TILE):
        meta, lit, start_k, rec_of, cnt, new_cov = walk_wide_model(recs[mp:], P0, n, cov)
        # against the four-wide walk of the two halves
        mp4 = mp
        for h in (0, 1):
            Q0 = P0 + ROW * h
            half = [r for r in recs if Q0 <= r[0] < Q0 + ROW]
            want, want_rec = narrow_meta(half, Q0, n, cov4)
            assert np.array_equal(meta[64 * h:64 * h + 64], want), (P0, h, n, recs[:4])
            assert np.array_equal(rec_of[64 * h:64 * h + 64], np.where(want_rec >= 0, want_rec + (mp4 - mp), -1))
            if half:
                cov4 = half[-1][0] + half[-1][1]
            mp4 += len(half)
        assert mp4 == mp + cnt and cov4 == new_cov or cnt == 0
        # against the classification
        for g in range(128):
            for k in range(4):
                p = P0 + 4 * g + k
                want_lit = p < n and kind[p] == ord("L")
                assert bool((lit[g] >> k) & 1) == want_lit, (p, n)
            starts = [k for k in range(4) if P0 + 4 * g + k < n and kind[P0 + 4 * g + k] == ord("S")]
            assert len(starts) <= 1 and start_k[g] == (starts[0] if starts else -1)
            if starts:
                assert recs[mp + rec_of[g]][0] == P0 + 4 * g + starts[0]
                assert lit[g] >> starts[0] == 0        # a group's literals all precede its match
        # the store rule: a lane's two bytes go out only inside the block's own rows (pos < rows * 256)
        for L in range(64):
            if P0 + 8 * L < rows * ROW:
                at = (P0 >> 2) + 2 * L
                assert out[at] == -1 and out[at + 1] == -1 and at + 1 < rows * 64
                out[at:at + 2] = meta[2 * L:2 * L + 2]
        mp += cnt
        cov = new_cov
    assert mp == len(recs)
    assert (out >= 0).all()                          # every byte of the block's rows is written, none twice
    assert (out[-(-n // 4):] == 0).all()             # zeros behind the chunk's end: the packer reads whole rows
    return out


def test_two_starts_in_one_lane():
    for L in (0, 1, 31, 63):
        for a in range(4):
            for b in range(a + 4, 8):
                base = 8 * L
                recs = [(base + a, 4), (base + b, 4)]
                out = run_chunk(recs, 2 * TILE)
                g = 2 * L
                assert out[g] == ((1 << a) - 1) | 16 | (a << 5)                 # literals before the first start
                k = b - 4
                want_lit = sum(1 << j for j in range(k) if 4 + j >= a + 4)    # ... and between the two
                assert out[g + 1] == want_lit | 16 | (k << 5)


@pytest.mark.parametrize("start", [0, 200, 253, 254, 255, 300, 508, 511])
def test_258_byte_match_across_tiles(start):
    # 254: ends exactly at position 511 of the tile; 255: ends at position 0 of the next; 511: starts on a tile's
    # last position and ends 257 positions into the next
    for lead in (0, TILE, 3 * TILE):
        recs = [(lead + start, 258)]
        if lead:
            recs.insert(0, (7, 9))
        recs.append((lead + start + 258 + 3, 5))
        run_chunk(recs, lead + 3 * TILE)


def test_cov_until_in_every_byte_of_a_lane():
    for L in (0, 5, 63):
        for j in range(9):
            end = TILE + 8 * L + j           # a match of the first tile that covers up to here in the second
            if end - 258 < 0:
                continue
            recs = [(end - 258, 258)] if end - 258 + 258 <= 2 * TILE else []
            run_chunk(recs, 3 * TILE)
            run_chunk(recs + [(end, 4), (end + 4, 7)], 3 * TILE)


@pytest.mark.parametrize("rem", [0, 1, 3, 4, 5, 7, 8, 255, 256, 257, 511])
def test_chunk_ends(rem):
    for tiles in (0, 1, 2):
        n = tiles * TILE + rem
        if n == 0:
            continue
        rng = np.random.default_rng(rem + 1000 * tiles)
        recs, pos = [], 0
        while True:
            pos += int(rng.integers(0, 6))
            ln = int(rng.choice([4, 5, 8, 17, 258]))
            if pos + ln > n:
                break
            recs.append((pos, ln))
            pos += ln
        run_chunk(recs, n)
        if n >= 4:                            # a match that ends on the chunk's last byte
            run_chunk([(n - 4, 4)], n)
        run_chunk([], n)


def test_128_starts_in_one_tile():
    for shift in range(4):
        recs = [(shift + 4 * i, 4) for i in range((3 * TILE - shift) // 4)]
        out = run_chunk(recs, 3 * TILE)
        assert (out[1:3 * TILE // 4 - 1] & 16).all()
        meta, _, _, rec_of, cnt, _ = walk_wide_model(recs[128:], TILE, 3 * TILE, recs[127][0] + 4)
        assert cnt == 128 and sorted(rec_of) == list(range(128))


@pytest.mark.parametrize("seed", range(6))
def test_random_chunks(seed):
    rng = np.random.default_rng(seed)
    for _ in range(12):
        n = int(rng.integers(1, 5 * TILE))
        dense = rng.random() < 0.5
        recs, pos = [], 0
        while True:
            pos += int(rng.integers(0, 3 if dense else 40))
            ln = int(rng.choice([4, 4, 5, 6, 9, 17, 64, 258]))
            if pos + ln > n:
                break
            recs.append((pos, ln))
            pos += ln
        run_chunk(recs, n)


# ---- bit placement -------------------------------------------------------------------------------
RING = 512
LANE_BITS_MAX = 2 * (3 * 15 + 48)


def sink_place(ring, q, lo, hi):
    """sink_place: the 96 bits (lo: 64, hi: 32) OR-ed into the ring at bit q, in 32-bit arithmetic."""
    w, sh = q >> 5, q & 31
    v0 = (lo << sh) & 0xffffffffffffffff
    d0, d1 = v0 & 0xffffffff, v0 >> 32
    d2 = ((hi << sh) & 0xffffffff) | (((lo >> 32) >> 1) >> (31 - sh))
    d3 = (hi >> 1) >> (31 - sh)
    top = w
    for k, d in enumerate((d0, d1, d2, d3)):
        if d:
            ring[(w + k) & (RING - 1)] |= d
            top = w + k
    return top


def test_two_halves_at_every_shift():
    rng = np.random.default_rng(5)
    shapes = [(93, 93), (93, 0), (0, 93), (45, 48), (1, 93), (64, 65), (60, 60), (32, 33), (93, 1)]
    for sh in range(32):
        for nb_a, nb_b in shapes + [tuple(rng.integers(0, 94, 2)) for _ in range(8)]:
            nb_a, nb_b = int(nb_a), int(nb_b)
            a = int(rng.integers(0, 1 << 62)) | (1 << 92) | 1
            b = int(rng.integers(0, 1 << 62)) | (1 << 92) | 1
            a &= (1 << nb_a) - 1
            b &= (1 << nb_b) - 1
            q = 32 * 7 + sh
            ring = [0] * RING
            if nb_a:
                sink_place(ring, q, a & 0xffffffffffffffff, a >> 64)
            if nb_b:
                sink_place(ring, q + nb_a, b & 0xffffffffffffffff, b >> 64)
            want = (a | (b << nb_a)) << q
            got = sum(d << (32 * i) for i, d in enumerate(ring))
            assert got == want, (sh, nb_a, nb_b)


def test_ring_bound():
    """What the static_assert at sink_emit_pair states: fewer than 64 pending dwords, the tile's bits, the partly
    filled dword they start in and sink_place's reach of three dwords stay inside the ring."""
    bound = 64 + 64 * LANE_BITS_MAX // 32 + 1 + 3
    assert LANE_BITS_MAX == 186 and bound <= RING
    for pending_bits in (0, 31, 63 * 32, 63 * 32 + 31):      # the flush loop leaves (bitpos >> 5) - flushed <= 63
        ring = [0] * RING
        q = pending_bits
        top = 0
        full = (1 << 93) - 1
        for _ in range(64):
            top = max(top, sink_place(ring, q, full & 0xffffffffffffffff, full >> 64))
            top = max(top, sink_place(ring, q + 93, full & 0xffffffffffffffff, full >> 64))
            q += 186
        assert top < bound
        assert (q - pending_bits) == 64 * 186 and ((q + 31) >> 5) <= bound
        # nothing wrapped onto a pending dword: the ring holds exactly the bits placed
        assert sum(d << (32 * i) for i, d in enumerate(ring)) == ((1 << (64 * 186)) - 1) << pending_bits
