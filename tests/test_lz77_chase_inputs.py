"""Which paths of the two-event chase (moonbit-flate_amd/csrc/lz77_chase_rule.h) the streams of
tests/lz77_chase_inputs.py reach, on the CPU: the lane-accurate host model (tests/host_model/lz77_wave_model.cpp) logs
every match with its path (fast / general), its start lane and whether the batch goes on behind it.  A chain is a run
of fast events of one batch -- what one call of the chase loop walks; the pair word of its k-th event states events k
and k + 1, so an event at an even place of its chain is a word's first hop and one at an odd place its second.
Nothing here is assumed from the generator: tests/test_gpu_lz77_chase.py runs these very streams."""
import numpy as np
import pytest

import lz77_chase_inputs as I
import lz77_corpus as Z


@pytest.fixture(scope="module")
def reached():
    """Facts over the first 190 small streams (every length ten times)."""
    f = dict(pairs=0, longest=0, second_general_long=0, second_general_slot=0, stop_first=0, stop_second=0,
             ends_first=0, ends_second=0, first_general=0, single_chain=0, lengths=set())
    for data in I.small_streams(190):
        r = Z.run_model(data, log=True)
        assert r.stats[Z.S_LOG_LOST] == 0
        judged = {int(row[1]) for row in r.log if row[0] == Z.LOG_GROUP_JUDGE}
        rows = [row for row in r.log if row[0] in (Z.LOG_MATCH, Z.LOG_NEXT)]
        place = 0  # of the next event in its chain
        for k, row in enumerate(rows):
            if row[0] != Z.LOG_MATCH or row[2] == Z.PATH_SPARSE:
                continue
            path, a, total = int(row[2]), (int(row[5]) >> 8) & 255, int(row[5]) >> 16
            nxt = rows[k + 1] if k + 1 < len(rows) and rows[k + 1][0] == Z.LOG_NEXT and rows[k + 1][1] == row[1] else None
            if a == 0:
                place = 0  # a batch's first event
            if path == Z.PATH_GENERAL:
                if place == 0:
                    f["first_general"] += 1
                elif place % 2 == 1:
                    f["second_general_long" if total >= 16 else "second_general_slot"] += int(total >= 16 or int(row[1]) in judged)
                place = 0
                continue
            f["lengths"].add(total)
            f["pairs"] += place % 2
            f["longest"] = max(f["longest"], place + 1)
            hop = "second" if place % 2 else "first"
            if nxt is None:
                f["ends_" + hop] += 1
            elif nxt[3] == 0:
                f["stop_" + hop] += 1
                f["single_chain"] += place == 0
            place += 1
    return f


def test_dense_batches_hold_pairs_and_long_chains(reached):
    assert reached["pairs"] >= 2000 and reached["longest"] >= 8, reached
    assert reached["lengths"] >= set(range(4, 16)), reached["lengths"]  # every fast length, 4 .. 15


def test_a_general_event_is_met_as_first_and_as_second_hop(reached):
    assert reached["first_general"] >= 50, reached
    assert reached["second_general_long"] >= 50, reached  # a repeat of 16 bytes or more behind a short match
    assert reached["second_general_slot"] >= 20, reached  # a same-slot lane judged behind a short match


def test_stop_and_end_of_window_on_either_hop(reached):
    assert reached["stop_first"] >= 50 and reached["stop_second"] >= 50, reached
    assert reached["ends_first"] >= 5 and reached["ends_second"] >= 5, reached
    assert reached["single_chain"] >= 5, reached  # a chain of one event that stops


def test_the_two_window_streams_are_two_windows_and_a_few_hundred_bytes():
    for s in I.two_window_streams(4):
        assert 2 * I.W + 128 <= len(s) <= 2 * I.W + 600 and len(Z.lz_chunks(len(s))) == 3
